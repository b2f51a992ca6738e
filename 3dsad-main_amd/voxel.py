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
