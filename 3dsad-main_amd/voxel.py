"""Voxelization layers (SPEC.md §20): thin ``nn.Module``s over ``ops.voxelize`` / ``ops.voxel_index`` and the
differentiable ``autograd.voxel_reduce`` — the first device step of a voxel, pillar or point-voxel detector.

Input is the ragged layout of §17 (``points [total,C]`` + ``offsets [B+1]`` int32 on the GPU) or a batch ``points [B,N,C]``
with ``offsets=None``.  Everything is deterministic and bit-equal to the reference restatement; there is no CPU path."""
from typing import Optional, Sequence

import torch
from torch import nn

from . import autograd, ops


class Voxelization(nn.Module):
    """``max_points`` = T: hard voxelization -> (voxels [B,V,T,C], coors [B,V,3] (z,y,x), num_points [B,V], voxel_num [B]).
    ``max_points=None``: the dynamic form -> (point2voxel [total], coors [B,V,3], count [B,V], voxel_num [B])."""

    def __init__(self, voxel_size: Sequence[float], point_range: Sequence[float], max_points: Optional[int], max_voxels: int):
        super().__init__()
        if len(voxel_size) != 3 or len(point_range) != 6:
            raise ValueError("voxel_size = (vx,vy,vz), point_range = (x0,y0,z0,x1,y1,z1)")
        self.voxel_size = tuple(float(v) for v in voxel_size)
        self.point_range = tuple(float(v) for v in point_range)
        self.max_points = None if max_points is None else int(max_points)
        self.max_voxels = int(max_voxels)

    def forward(self, points: torch.Tensor, offsets: Optional[torch.Tensor] = None):
        with torch.no_grad():
            if self.max_points is None:
                return ops.voxel_index(points, offsets, self.voxel_size, self.point_range, self.max_voxels)
            return ops.voxelize(points, offsets, self.voxel_size, self.point_range, self.max_points, self.max_voxels)

    def extra_repr(self) -> str:
        return (f"voxel_size={self.voxel_size}, point_range={self.point_range}, max_points={self.max_points}, "
                f"max_voxels={self.max_voxels}")


class DynamicScatter(nn.Module):
    """Reduce point features over the voxels of a dynamic index: feat [total,Cf] (or [B,N,Cf] with ``offsets=None``),
    point2voxel [total] -> out [B,V,Cf] by ``mode`` "sum" / "mean" / "max"; differentiable in ``feat``."""

    def __init__(self, mode: str = "mean"):
        super().__init__()
        if mode not in ops.VOXEL_MODES:
            raise ValueError(f"mode must be one of {sorted(ops.VOXEL_MODES)}, got {mode!r}")
        self.mode = mode

    def forward(self, feat: torch.Tensor, point2voxel: torch.Tensor, offsets: Optional[torch.Tensor], max_voxels: int):
        if offsets is None:
            if feat.dim() != 3:
                raise ValueError("feat: [B,N,Cf] expected when offsets is None")
            B, N, Cf = feat.shape
            offsets = torch.arange(0, (B + 1) * N, N, dtype=torch.int32, device=feat.device) if N else \
                torch.zeros((B + 1,), dtype=torch.int32, device=feat.device)
            feat = feat.reshape(B * N, Cf)
        return autograd.voxel_reduce(feat, point2voxel, offsets, int(max_voxels), self.mode)

    def extra_repr(self) -> str:
        return f"mode={self.mode}"


class PillarFeatureNet(nn.Module):
    """Pillar / dynamic-voxel feature encoder (SPEC.md §24): a stack of fused decorate + linear (+ ReLU) + voxel-max layers.
    The first layer reads the points decorated with the offset to the mean of the voxel's members (``with_cluster_center``)
    and to the voxel's centre (``with_voxel_center``); a layer that is not the last has ``feat / 2`` output channels and hands
    the next layer its pointwise output next to its per-voxel maximum (rows ``[y | max]``).  ``weight`` / ``bias`` hold the
    linear layers with BatchNorm already folded in.  ``max_points`` = T keeps the first T points of a voxel (hard
    voxelization); ``None`` is the dynamic form.

    forward(points [total,C], point2voxel [total], offsets [B+1], coors [B,V,3]) -> [B,V,feat_channels[-1]], zero for a voxel
    without points: what ``SparseTensor.from_voxels`` or a BEV scatter takes."""

    def __init__(self, in_channels: int, feat_channels: Sequence[int] = (64,), voxel_size: Sequence[float] = (0.16, 0.16, 4),
                 point_range: Sequence[float] = (0, -39.68, -3, 69.12, 39.68, 1), with_cluster_center: bool = True,
                 with_voxel_center: bool = True, max_points: Optional[int] = None):
        super().__init__()
        if len(voxel_size) != 3 or len(point_range) != 6:
            raise ValueError("voxel_size = (vx,vy,vz), point_range = (x0,y0,z0,x1,y1,z1)")
        if len(feat_channels) < 1:
            raise ValueError("feat_channels: at least one layer")
        self.in_channels = int(in_channels)
        self.feat_channels = tuple(int(c) for c in feat_channels)
        self.voxel_size = tuple(float(v) for v in voxel_size)
        self.point_range = tuple(float(v) for v in point_range)
        self.with_cluster_center, self.with_voxel_center = bool(with_cluster_center), bool(with_voxel_center)
        self.max_points = None if max_points is None else int(max_points)
        cin = self.in_channels + 3 * self.with_cluster_center + 3 * self.with_voxel_center
        self.weight, self.bias = nn.ParameterList(), nn.ParameterList()
        for l, feat in enumerate(self.feat_channels):
            last = l == len(self.feat_channels) - 1
            if not last and feat % 2:
                raise ValueError(f"feat_channels[{l}] = {feat}: a layer that is not the last must have an even width")
            cout = feat if last else feat // 2
            w = torch.empty(cout, cin)
            nn.init.kaiming_uniform_(w, a=5 ** 0.5)
            self.weight.append(nn.Parameter(w))
            self.bias.append(nn.Parameter(torch.zeros(cout)))
            cin = 2 * cout

    def forward(self, points: torch.Tensor, point2voxel: torch.Tensor, offsets: Optional[torch.Tensor], coors: torch.Tensor):
        if offsets is None:
            if points.dim() != 3:
                raise ValueError("points: [B,N,C] expected when offsets is None")
            B, N, C = points.shape
            offsets = torch.arange(0, (B + 1) * N, N, dtype=torch.int32, device=points.device) if N else \
                torch.zeros((B + 1,), dtype=torch.int32, device=points.device)
            points = points.reshape(B * N, C)
        V = coors.shape[1]
        x, pooled = points, None
        n = len(self.feat_channels)
        for l in range(n):
            first, last = l == 0, l == n - 1
            res = autograd.voxel_encode(x, point2voxel, offsets, V, self.weight[l], self.bias[l], coors if first else None,
                                        self.voxel_size, self.point_range, first and self.with_cluster_center,
                                        first and self.with_voxel_center, True, pooled, self.max_points, not last)
            if last:
                return res
            pooled, x = res
        return pooled

    def extra_repr(self) -> str:
        return (f"in_channels={self.in_channels}, feat_channels={self.feat_channels}, voxel_size={self.voxel_size}, "
                f"point_range={self.point_range}, max_points={self.max_points}")
