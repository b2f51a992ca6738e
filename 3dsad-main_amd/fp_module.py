"""``FPModule``: PointNet++ feature propagation (SPEC.md §18) on the HIP path.

Drop-in surface of the FP layers of PointNet++-style code bases: ``forward(unknown_xyz [B,n,3], known_xyz [B,m,3],
unknown_feats [B,C1,n] | None, known_feats [B,C2,m]) -> [B,C',n]``.  Per call: ``three_nn`` (with the weights) ->
``three_interpolate`` point-major straight into columns [0, C2) of the MLP's input rows -> the skip features copied into
columns [C2, C2 + C1) (``sad_copy_rows_u32``) -> one plain-row chain (SPEC.md §6, no xyz prefix, ReLU on every layer).
No concatenation pass.  ``forward_pm`` takes and returns point-major features, as ``SAModuleMSG.forward_pm`` does.
"""
from typing import Optional, Sequence

import numpy as np
import torch
from torch import nn

from . import ops
from ._lib import check, lib
from .synth import make_mlp_weights


class FPModule(nn.Module):
    """Feature propagation: interpolated known features ‖ skip features -> shared MLP.  ``mlp`` = output widths of the
    layers; ``weights`` = [(W, b), ...] numpy arrays (BatchNorm folded), seeded Kaiming-uniform weights when omitted."""

    def __init__(self, known_channels: int, skip_channels: int, mlp: Sequence[int], device, weights=None, seed: int = 0):
        super().__init__()
        self.known_channels = int(known_channels)
        self.skip_channels = int(skip_channels)
        self.in_channels = self.known_channels + self.skip_channels
        self.device = torch.device(device)
        if weights is None:
            weights = make_mlp_weights([self.in_channels] + list(mlp), np.random.default_rng(seed))
        self.weights = weights
        self.mlp = ops.PackedMLP(weights, False, self.device, name="fp")
        if self.mlp.dims[0] != self.in_channels:
            raise ValueError(f"first layer takes {self.mlp.dims[0]} channels, expected {self.in_channels}")
        self.out_channels = self.mlp.out_channels

    def forward_pm(self, unknown_xyz: torch.Tensor, known_xyz: torch.Tensor, unknown_feats_pm: Optional[torch.Tensor],
                   known_feats_pm: torch.Tensor) -> torch.Tensor:
        """Point-major: unknown_feats_pm [B,n,C1] | None, known_feats_pm [B,m,C2] -> [B,n,C']."""
        B, n = unknown_xyz.shape[0], unknown_xyz.shape[1]
        if known_feats_pm.dim() != 3 or known_feats_pm.shape[2] != self.known_channels:
            raise ValueError(f"known_feats_pm: expected [B,m,{self.known_channels}]")
        if (unknown_feats_pm is None) != (self.skip_channels == 0):
            raise ValueError(f"this module takes {self.skip_channels} skip channels")
        _, idx, w = ops.three_nn(unknown_xyz, known_xyz)
        x = ops._empty((B, n, self.in_channels), dtype=torch.float32, device=unknown_xyz.device)
        ops.three_interpolate(known_feats_pm, idx, w, point_major=True, out=x, col_off=0)
        if self.skip_channels:
            skip = ops._need(unknown_feats_pm, "unknown_feats_pm", torch.float32, 3)
            if tuple(skip.shape) != (B, n, self.skip_channels):
                raise ValueError(f"unknown_feats_pm: expected [B,n,{self.skip_channels}]")
            check(lib().sad_copy_rows_u32(skip.data_ptr(), self.skip_channels, x.data_ptr() + 4 * self.known_channels,
                                          self.in_channels, B * n, self.skip_channels, ops._stream()), "sad_copy_rows_u32")
        return self.mlp.rows(x)

    def forward(self, unknown_xyz: torch.Tensor, known_xyz: torch.Tensor, unknown_feats: Optional[torch.Tensor],
                known_feats: torch.Tensor) -> torch.Tensor:
        """Drop-in surface: channel-major unknown_feats [B,C1,n] | None, known_feats [B,C2,m] -> [B,C',n]."""
        skip = unknown_feats.transpose(1, 2).contiguous() if unknown_feats is not None else None
        out = self.forward_pm(unknown_xyz, known_xyz, skip, known_feats.transpose(1, 2).contiguous())
        return out.transpose(1, 2).contiguous()
