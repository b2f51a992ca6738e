"""Voxel RoI pooling (SPEC.md §30): the second stage of a voxel detector (Voxel R-CNN, the RoI-grid half of PV-RCNN) between
``nms_boxes`` / ``roi_targets`` and the RoI head's layers.  A G x G x G grid of points is laid in every RoI
(``ops.roi_grid_points``); at every backbone scale the non-empty voxels around each grid point are found through the coordinate
table (``ops.voxel_query``: no dense index volume, no pair tests against every voxel), and their features go through a small
shared MLP and a max (§6), scale beside scale.

The ragged voxels of a scale are ONE scene of the grouped operators: ``voxel_query`` returns global rows, so ``xyz`` = the voxel
centres [1,Nv,3], ``feat`` [1,Nv,C], the grid points [1,B*R*G^3,3] and ``idx`` / ``cnt`` viewed as [1,B*R*G^3,S] are exact.  The
centres are §24's formula evaluated by framework elementwise operations (a multiplication and an addition, each rounded on its
own), not by a kernel of this package.

Inference (no gradient asked for) runs the fused ``PackedMLP.grouped`` per scale into one zeroed buffer.  Training runs the same
rows through ``autograd.GroupPoints``, the module's layers as framework matrix products, and ``autograd.MaxPoolS`` - or, with
``fused_grad=True``, through the fused chain and its own backward (SPEC.md §32).  One set of
weights (BatchNorm folded in, as everywhere here) serves both; the packed chain is rebuilt when a weight changes, as the sparse
convolution layers rebuild theirs.  Parameters are created with ``requires_grad=False``, like those layers:
``module.requires_grad_(True)``, or features that require grad, select the training path.

A grid point with no voxel in reach (``cnt == 0``: also every point of a RoI beyond ``roi_count``, whose coordinates are NaN) pools
to exactly zero in both paths: the chain runs such a group on its padding row, and the module overwrites the result
(``masked_fill``, never a multiplication: NaN is in play)."""
from typing import Optional, Sequence

import numpy as np
import torch
from torch import nn

from . import autograd, ops
from .shared_mlp import grouped_chain, packed_for, wants_grad
from .spconv import SparseTensor


class VoxelRoIPool(nn.Module):
    """``scales``: one dict per backbone scale, in the order of ``forward``'s ``tensors``: ``in_channels`` (C of that scale's
    features), ``voxel_size`` (vx,vy,vz) AT THAT SCALE (base size x stride), ``max_range`` (rz,ry,rx) in cells, ``radius``,
    ``nsample`` (1 .. 64: the grouped chain's limit) and ``mlp`` = the layer widths [C1, ..., C_out]; ``point_range``
    (x0,y0,z0,x1,y1,z1) is the detector's.  ``weight[k]`` / ``bias[k]`` hold scale k's layers ([C_out,C_in] each, the first over
    [relative xyz (3) | features (C)]), ReLU after every layer.

    ``fused_grad``: the training path of a scale is the fused chain with the backward of SPEC.md §32 (``SharedMLP``'s path: the
    forward is the inference kernel, nothing but inputs and output is kept) instead of the unfused composition.

    forward(rois [B,R,D>=7], roi_count [B] int32 | None, tensors) -> pooled [B,R,G^3,sum C_out]."""

    def __init__(self, grid_size: int, scales: Sequence[dict], point_range: Sequence[float], fused_grad: bool = False):
        super().__init__()
        self.fused_grad = bool(fused_grad)
        self.grid_size = int(grid_size)
        if not 1 <= self.grid_size <= 16:
            raise ValueError(f"grid_size: expected 1 .. 16, got {grid_size}")
        if len(point_range) != 6:
            raise ValueError("point_range = (x0,y0,z0,x1,y1,z1)")
        if len(scales) < 1:
            raise ValueError("scales: at least one scale")
        self.point_range = tuple(float(v) for v in point_range)
        self.scales = []
        self.weight, self.bias = nn.ModuleList(), nn.ModuleList()
        for k, s in enumerate(scales):
            cfg = dict(in_channels=int(s["in_channels"]), voxel_size=tuple(float(v) for v in s["voxel_size"]),
                       max_range=tuple(int(v) for v in s["max_range"]), radius=float(s["radius"]), nsample=int(s["nsample"]),
                       mlp=tuple(int(c) for c in s["mlp"]))
            if len(cfg["voxel_size"]) != 3 or len(cfg["max_range"]) != 3:
                raise ValueError(f"scales[{k}]: voxel_size = (vx,vy,vz) and max_range = (rz,ry,rx)")
            if not 1 <= cfg["nsample"] <= 64:
                raise ValueError(f"scales[{k}]: nsample 1 .. 64 expected (the grouped chain's limit), got {cfg['nsample']}")
            if not 1 <= len(cfg["mlp"]) <= 4 or min(cfg["mlp"]) < 1 or cfg["in_channels"] < 1:
                raise ValueError(f"scales[{k}]: in_channels >= 1 and 1 .. 4 layer widths >= 1 expected")
            ws, bs = nn.ParameterList(), nn.ParameterList()
            cin = 3 + cfg["in_channels"]
            for cout in cfg["mlp"]:
                w = torch.empty(cout, cin)
                nn.init.kaiming_uniform_(w, a=5 ** 0.5)
                ws.append(nn.Parameter(w, requires_grad=False))
                bs.append(nn.Parameter(torch.zeros(cout), requires_grad=False))
                cin = cout
            self.weight.append(ws)
            self.bias.append(bs)
            self.scales.append(cfg)
        self.out_channels = sum(s["mlp"][-1] for s in self.scales)
        self._packed = [None] * len(self.scales)        # per scale: (key of the parameters it was made from, ops.PackedMLP)

    def packed(self, k: int) -> "ops.PackedMLP":
        """Scale k's layers as the fused chain reads them; repacked when a parameter was replaced or written."""
        self._packed[k] = packed_for(self._packed[k], self.weight[k], self.bias[k], True, name=f"voxel_roi_pool{k}")
        return self._packed[k][1]

    def centres(self, k: int, coors: torch.Tensor) -> torch.Tensor:
        """§24's voxel centres of scale k: coors [Nv,3] (z,y,x) -> [Nv,3] (x,y,z) = ((float)g * v) + ((0.5 * v) + lo)."""
        v = np.asarray(self.scales[k]["voxel_size"], np.float32)
        lo = np.asarray(self.point_range[:3], np.float32)
        half = np.float32(0.5) * v + lo
        g = coors.flip(1).to(torch.float32)
        return g * torch.from_numpy(v).to(coors.device) + torch.from_numpy(half).to(coors.device)

    def forward(self, rois: torch.Tensor, roi_count: Optional[torch.Tensor], tensors: Sequence[SparseTensor]) -> torch.Tensor:
        if len(tensors) != len(self.scales):
            raise ValueError(f"{len(self.scales)} sparse tensors expected (one per scale), got {len(tensors)}")
        for k, (t, s) in enumerate(zip(tensors, self.scales)):
            if t.feat.shape[1] != s["in_channels"]:
                raise ValueError(f"tensors[{k}]: {s['in_channels']} feature channels expected, got {t.feat.shape[1]}")
        train = wants_grad(*(t.feat for t in tensors), module=self)
        with torch.no_grad():
            pts = ops.roi_grid_points(rois, roi_count, self.grid_size)
        B, R, P, _ = pts.shape
        M = R * P
        new_xyz = pts.view(1, B * M, 3)
        out = None if train else torch.zeros((1, B * M, self.out_channels), dtype=torch.float32, device=rois.device)
        cols, col = [], 0
        for k, (t, s) in enumerate(zip(tensors, self.scales)):
            cout = s["mlp"][-1]
            Nv = t.feat.shape[0]
            if Nv == 0:                                 # nothing to pool from: the columns stay zero
                if train:
                    cols.append(torch.zeros((B * M, cout), dtype=torch.float32, device=rois.device))
                col += cout
                continue
            with torch.no_grad():
                idx, cnt = ops.voxel_query(t.coors, t.offsets, t.spatial_shape, s["voxel_size"], self.point_range, pts.view(B, M, 3),
                                           max_range=s["max_range"], radius=s["radius"], S=s["nsample"])
                idx, cnt = idx.view(1, B * M, s["nsample"]), cnt.view(1, B * M)
                xyz = self.centres(k, t.coors).unsqueeze(0)
                empty = cnt.view(B * M, 1) == 0
            if train and self.fused_grad:
                # the fused chain forward, its own backward (SPEC.md §32); empty groups (NaN coordinates among them) give no gradient
                rows = grouped_chain(self.packed(k), self.weight[k], self.bias[k], xyz, t.feat.unsqueeze(0), new_xyz, idx, cnt, skip_empty=True)
                cols.append(rows[0].masked_fill(empty, 0.0))
            elif train:
                cols.append(self._train_rows(k, t.feat, xyz, new_xyz, idx).masked_fill(empty, 0.0))
            else:
                with torch.no_grad():
                    self.packed(k).grouped(xyz, t.feat.detach().unsqueeze(0), new_xyz, idx, out=out, col_off=col, cnt=cnt)
                    out[0, :, col:col + cout].masked_fill_(empty, 0.0)
            col += cout
        if train:
            out = torch.cat(cols, 1)
        return out.view(B, R, P, self.out_channels)

    def _train_rows(self, k: int, feat: torch.Tensor, xyz: torch.Tensor, new_xyz: torch.Tensor, idx: torch.Tensor) -> torch.Tensor:
        """The differentiable form of scale k: feat [Nv,C], xyz [1,Nv,3], new_xyz [1,M,3], idx [1,M,S] -> [M,C_out]."""
        with torch.no_grad():
            rel = ops.group_points(xyz.transpose(1, 2).contiguous(), idx) - new_xyz.transpose(1, 2).unsqueeze(-1)     # [1,3,M,S]
            rel.nan_to_num_(0.0, 0.0, 0.0)              # (a NaN / Inf grid point: its rows are overwritten at the end)
        x = torch.cat([rel, autograd.GroupPoints.apply(feat.t().unsqueeze(0), idx)], 1)                              # [1,3+C,M,S]
        for w, b in zip(self.weight[k], self.bias[k]):
            x = torch.relu(torch.einsum("oc,bcms->boms", w, x) + b.view(1, -1, 1, 1))
        return autograd.MaxPoolS.apply(x.contiguous())[0].t()

    def extra_repr(self) -> str:
        return f"grid_size={self.grid_size}, point_range={self.point_range}, scales={self.scales}"
