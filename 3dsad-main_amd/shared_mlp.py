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


def wants_grad(*tensors, module: Optional[nn.Module] = None) -> bool:
    """Does this call train?  Gradient mode is on and a tensor (``None`` entries are skipped) or a parameter of ``module``
    requires grad: the one test every layer here puts in front of its choice between the fused call and its autograd form."""
    return torch.is_grad_enabled() and (any(t is not None and t.requires_grad for t in tensors)
                                        or (module is not None and any(p.requires_grad for p in module.parameters())))


def grouped_chain(packed, weights, biases, xyz, feat_pm, new_xyz, idx, cnt=None, skip_empty: bool = False) -> torch.Tensor:
    """``packed.grouped`` of the chain whose unpacked parameters are ``weights`` / ``biases``: the fused call under ``no_grad`` or
    when nothing requires grad, else ``autograd.GroupedMLP``.  -> pooled [B,M,C_L]."""
    params = list(weights) + list(biases)
    if not wants_grad(*params, feat_pm, xyz, new_xyz):
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
        if not wants_grad(*params, x):
            with torch.no_grad():
                return self.packed().rows(x)
        return autograd.MLPRows.apply(self.packed(), x, *params)

    def export(self) -> list:
        """[(W, b)] as numpy arrays: what ``ops.PackedMLP`` and the inference modules take."""
        return [(w.detach().cpu().numpy().copy(), b.detach().cpu().numpy().copy()) for w, b in zip(self.weight, self.bias)]

    def extra_repr(self) -> str:
        return f"dims={self.dims}, first_has_xyz={self.first_has_xyz}, relu_mask={self.relu_mask}"


class BranchGroup(nn.ModuleList):
    """The branches of a multi-radius layer: ``SharedMLP``s that pool the same (xyz, feat_pm, new_xyz), each over the ball query
    of its own radius, into one [B,M,``cat_channels``] tensor.  Without gradients the branches write into slices of one zeroed
    buffer, as the inference modules do; with gradients each branch returns its own pooled tensor (what its backward keeps) and
    the tensors are concatenated (one branch: its tensor, no copy).  The two forms are equal bit for bit."""

    def __init__(self, mlps):
        super().__init__(mlps)
        self.cat_channels = sum(mlp.out_channels for mlp in self)

    def forward(self, xyz: torch.Tensor, feat_pm: Optional[torch.Tensor], new_xyz: torch.Tensor, idxs, cnts) -> torch.Tensor:
        """``idxs`` / ``cnts``: one idx [B,M,S_b] and one cnt [B,M] per branch (``ops.ball_query_multi``) -> [B,M,sum C_b]."""
        if wants_grad(xyz, feat_pm, new_xyz, module=self):
            outs = [mlp.grouped(xyz, feat_pm, new_xyz, idx, cnt) for mlp, idx, cnt in zip(self, idxs, cnts)]
            return outs[0] if len(outs) == 1 else torch.cat(outs, 2)
        with torch.no_grad():
            cat = torch.zeros((new_xyz.shape[0], new_xyz.shape[1], self.cat_channels), dtype=torch.float32, device=xyz.device)
            off = 0
            for mlp, idx, cnt in zip(self, idxs, cnts):
                mlp.packed().grouped(xyz, feat_pm, new_xyz, idx, out=cat, col_off=off, cnt=cnt)
                off += mlp.out_channels
        return cat
