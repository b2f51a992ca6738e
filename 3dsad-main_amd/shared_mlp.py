"""``SharedMLP``: a trainable shared-MLP chain (SPEC.md §6, backward §32).  One set of float32 parameters (BatchNorm folded in, as
everywhere here) serves both directions: without gradients the calls are the fused ``PackedMLP.grouped`` / ``.rows``, bit for bit;
with gradients they go through ``autograd.GroupedMLP`` / ``autograd.MLPRows``, whose forward is the same fused kernel and whose
backward recomputes the activations.  The packed chain is rebuilt when a parameter was replaced or written."""
from typing import Optional, Sequence

import numpy as np
import torch
from torch import nn

from . import autograd, ops


def packed_for(cache, weights, biases, first_has_xyz: bool, relu_mask: Optional[int] = None, name: str = ""):
    """``cache`` = None or (key, ops.PackedMLP) -> the same, repacked when a parameter's (data_ptr, _version) changed: the one
    definition behind ``SharedMLP.packed`` and ``VoxelRoIPool.packed``."""
    params = list(weights) + list(biases)
    key = tuple((p.data_ptr(), p._version) for p in params)
    if cache is None or cache[0] != key:
        layers = [(w.data, b.data) for w, b in zip(weights, biases)]
        cache = (key, ops.PackedMLP(layers, first_has_xyz, params[0].device, relu_mask=relu_mask, name=name))
    return cache


def _wants_grad(tensors) -> bool:
    return torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in tensors)


def grouped_chain(packed, weights, biases, xyz, feat_pm, new_xyz, idx, cnt=None, skip_empty: bool = False) -> torch.Tensor:
    """``packed.grouped`` of the chain whose unpacked parameters are ``weights`` / ``biases``: the fused call under ``no_grad`` or
    when nothing requires grad, else ``autograd.GroupedMLP``.  -> pooled [B,M,C_L]."""
    params = list(weights) + list(biases)
    if not _wants_grad(params + [feat_pm, xyz, new_xyz]):
        with torch.no_grad():
            return packed.grouped(xyz, feat_pm, new_xyz, idx, cnt=cnt)
    return autograd.GroupedMLP.apply(packed, skip_empty, xyz, feat_pm, new_xyz, idx, cnt, *params)


class SharedMLP(nn.Module):
    """``dims`` = [C_0, C_1, ..., C_L] (C_0 includes the 3 relative coordinates when ``first_has_xyz``), 1 .. 4 layers; ``relu_mask``
    bit l = ReLU after layer l (default: all; a grouped chain needs all).  ``weight[l]`` [C_{l+1}, C_l] / ``bias[l]`` are created
    with ``requires_grad=False`` like every layer here: ``module.requires_grad_(True)``, or inputs that require grad, select the
    training path.  ``layers`` = [(W, b)] (numpy or tensors) initialises them, else Kaiming-uniform weights and zero biases."""

    def __init__(self, dims: Sequence[int], first_has_xyz: bool, relu_mask: Optional[int] = None, layers=None, name: str = ""):
        super().__init__()
        dims = [int(d) for d in dims]
        if not 2 <= len(dims) <= 5 or min(dims) < 1:
            raise ValueError("dims: C_0 and 1 .. 4 layer widths >= 1 expected")
        if layers is not None and [int(np.shape(layers[0][0])[1])] + [int(np.shape(w)[0]) for w, _ in layers] != dims:
            raise ValueError("layers do not have the shapes of dims")
        self.dims, self.first_has_xyz, self.name = dims, bool(first_has_xyz), name
        self.relu_mask = (1 << (len(dims) - 1)) - 1 if relu_mask is None else int(relu_mask)
        self.weight, self.bias = nn.ParameterList(), nn.ParameterList()
        for l, (cin, cout) in enumerate(zip(dims[:-1], dims[1:])):
            if layers is None:
                w = torch.empty(cout, cin)
                nn.init.kaiming_uniform_(w, a=5 ** 0.5)
                b = torch.zeros(cout)
            else:
                w = torch.as_tensor(np.asarray(layers[l][0]), dtype=torch.float32).clone()
                b = torch.as_tensor(np.asarray(layers[l][1]), dtype=torch.float32).clone()
            self.weight.append(nn.Parameter(w, requires_grad=False))
            self.bias.append(nn.Parameter(b, requires_grad=False))
        self.out_channels = dims[-1]
        self._packed = None

    def packed(self) -> "ops.PackedMLP":
        """The layers as the fused chain reads them; repacked when a parameter was replaced or written."""
        self._packed = packed_for(self._packed, self.weight, self.bias, self.first_has_xyz, self.relu_mask, self.name)
        return self._packed[1]

    def grouped(self, xyz: torch.Tensor, feat_pm: Optional[torch.Tensor], new_xyz: torch.Tensor, idx: torch.Tensor,
                cnt: Optional[torch.Tensor] = None, skip_empty: bool = False) -> torch.Tensor:
        """Fused group -> MLP -> max (``PackedMLP.grouped``) -> [B,M,C_L], differentiable in the parameters, ``feat_pm``, ``xyz``
        and ``new_xyz``."""
        return grouped_chain(self.packed(), self.weight, self.bias, xyz, feat_pm, new_xyz, idx, cnt, skip_empty)

    def rows(self, x: torch.Tensor) -> torch.Tensor:
        """Plain rows x [..., C_0] -> [..., C_L] (``PackedMLP.rows``), differentiable in the parameters and ``x``."""
        params = list(self.weight) + list(self.bias)
        if not _wants_grad(params + [x]):
            with torch.no_grad():
                return self.packed().rows(x)
        return autograd.MLPRows.apply(self.packed(), x, *params)

    def export(self) -> list:
        """[(W, b)] as numpy arrays: what ``ops.PackedMLP`` and the inference modules take."""
        return [(w.detach().cpu().numpy().copy(), b.detach().cpu().numpy().copy()) for w, b in zip(self.weight, self.bias)]

    def extra_repr(self) -> str:
        return f"dims={self.dims}, first_has_xyz={self.first_has_xyz}, relu_mask={self.relu_mask}"
