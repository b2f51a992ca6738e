"""Sparse 3-D convolution layers (SPEC.md §21, §22): ``SparseTensor`` and thin ``nn.Module``s over ``ops.sparse_conv_index`` /
``ops.sparse_conv`` / ``ops.sparse_to_dense`` — the backbone step of a voxel detector, directly behind ``voxel.py`` — and the
decoder side of a sparse U-Net: ``SparseMaxPool3d`` (§22.1) and ``SparseInverseConv3d`` (§22.3), which returns to the active set
its partner layer (named by ``indice_key``) came from, by that layer's own rulebook.

A ``SparseTensor`` is ``feat [Nv,C]`` f32, ``coors [Nv,3]`` int32 (z,y,x), ``offsets [B+1]`` int32 (all on the GPU) and a host
``spatial_shape`` (Gz,Gy,Gx).  It carries a rulebook cache, ``rulebooks``: one ``Rulebook`` record per ``indice_key``, shared by
every tensor derived from it (``derive``), so layers that name the same key (the submanifold layers of one resolution) build
``nbr`` once; a layer without a key builds an uncached record.  The forward is deterministic and equal to the reference
restatement under ``==``; there is no CPU path.

Training (SPEC.md §21.4).  Parameters are created with ``requires_grad=False`` and the layers then run the plain forward
under ``no_grad``; ``module.requires_grad_(True)`` (or an input whose ``feat`` requires grad) routes a layer through
``autograd.SparseConv``: grad_W / grad_bias by the weight-gradient kernel (float atomics: within the §21.4 bound, not bit-equal
from run to run), grad_feat by the forward kernel over the transposed rulebook, which is built at the first backward that needs
it and kept on the layer's ``Rulebook`` (``Rulebook.transposed()``; its collision count is read back once).
``dense()`` / ``bev()`` are differentiable the same way.  A scene that holds a coordinate twice has no gradient through a
submanifold layer (``ValueError`` in backward); ``from_voxels`` never produces one."""
from typing import Optional, Sequence

import torch
from torch import nn

from . import autograd, ops
from .shared_mlp import wants_grad


class Rulebook:
    """What one layer geometry made of one input tensor.  ``geometry`` = (subm, in_shape, kernel, stride, padding); ``in_coors`` /
    ``in_offsets`` are the input's own tensor objects, which an inverse layer (§22.3) hands on."""

    def __init__(self, geometry, in_coors, in_offsets, out_coors, out_offsets, nbr, out_shape, nbrT=None, collisions=None):
        self.geometry, self.in_coors, self.in_offsets = geometry, in_coors, in_offsets
        self.out_coors, self.out_offsets, self.nbr, self.out_shape = out_coors, out_offsets, nbr, out_shape
        self.nbrT, self.collisions = nbrT, collisions

    def transposed(self):
        """(nbrT, collisions): the transposed rulebook of §21.4, built (one synchronisation) for whichever asks first, the backward
        of the layer that owns the rulebook or the forward of its inverse, then kept."""
        if self.nbrT is None:
            with torch.no_grad():
                self.nbrT, col = ops.sparse_conv_index_transpose(self.nbr, self.in_coors.shape[0])
            self.collisions = int(col.item())
        return self.nbrT, self.collisions


class SparseTensor:
    def __init__(self, feat: torch.Tensor, coors: torch.Tensor, offsets: torch.Tensor, spatial_shape: Sequence[int],
                 rulebooks: Optional[dict] = None):
        if feat.dim() != 2 or coors.dim() != 2 or coors.shape[1] != 3 or coors.shape[0] != feat.shape[0]:
            raise ValueError(f"feat [Nv,C] and coors [Nv,3] expected, got {tuple(feat.shape)} and {tuple(coors.shape)}")
        if offsets.dim() != 1 or offsets.shape[0] < 2:
            raise ValueError("offsets [B+1] with B >= 1 expected")
        if len(spatial_shape) != 3 or min(int(g) for g in spatial_shape) < 1:
            raise ValueError(f"spatial_shape = (Gz,Gy,Gx), all >= 1, expected, got {spatial_shape!r}")
        self.feat, self.coors, self.offsets = feat, coors, offsets
        self.spatial_shape = tuple(int(g) for g in spatial_shape)
        self.rulebooks = {} if rulebooks is None else rulebooks     # indice_key -> Rulebook; shared by every tensor derived from this one

    @property
    def batch_size(self) -> int:
        return self.offsets.shape[0] - 1

    @classmethod
    def from_voxels(cls, feat: torch.Tensor, coors: torch.Tensor, voxel_num: torch.Tensor, spatial_shape: Sequence[int]) -> "SparseTensor":
        """The bridge from §20.3 / §20.4: feat [B,V,C] (``voxel_reduce`` output, or any per-voxel feature), coors [B,V,3],
        voxel_num [B] -> the rows v < voxel_num[b] of every scene, scene after scene.  Framework indexing; reads the row count
        back (one synchronisation)."""
        if feat.dim() != 3 or coors.dim() != 3 or tuple(coors.shape) != (feat.shape[0], feat.shape[1], 3) or voxel_num.shape != (feat.shape[0],):
            raise ValueError(f"feat [B,V,C], coors [B,V,3], voxel_num [B] expected, got {tuple(feat.shape)}, {tuple(coors.shape)}, "
                             f"{tuple(voxel_num.shape)}")
        B, V, C = feat.shape
        num = voxel_num.to(torch.int64).clamp(0, V)
        keep = (torch.arange(V, device=feat.device)[None, :] < num[:, None]).reshape(-1)
        offsets = torch.zeros((B + 1,), dtype=torch.int32, device=feat.device)
        offsets[1:] = torch.cumsum(num, 0).to(torch.int32)
        return cls(feat.reshape(B * V, C)[keep].to(torch.float32).contiguous(), coors.reshape(B * V, 3)[keep].to(torch.int32).contiguous(),
                   offsets, spatial_shape)

    def derive(self, feat: torch.Tensor, coors=None, offsets=None, spatial_shape=None) -> "SparseTensor":
        """A tensor that shares this one's rulebook cache; what is not given is this one's."""
        return SparseTensor(feat, self.coors if coors is None else coors, self.offsets if offsets is None else offsets,
                            self.spatial_shape if spatial_shape is None else spatial_shape, self.rulebooks)

    def replace_feature(self, feat: torch.Tensor) -> "SparseTensor":
        return self.derive(feat)

    def dense(self) -> torch.Tensor:
        """-> [B,C,Gz,Gy,Gx], zero where no voxel is (§21.3); differentiable with respect to ``feat`` (§21.4)."""
        if wants_grad(self.feat):
            return autograd.sparse_to_dense(self.feat, self.coors, self.offsets, self.spatial_shape)
        return ops.sparse_to_dense(self.feat, self.coors, self.offsets, self.spatial_shape)

    def bev(self) -> torch.Tensor:
        """The bird's-eye-view map of a voxel detector: ``dense()`` viewed as [B, C*Gz, Gy, Gx]."""
        d = self.dense()
        B, C, Gz, Gy, Gx = d.shape
        return d.view(B, C * Gz, Gy, Gx)


def _rulebook(x: SparseTensor, indice_key, subm: bool, kernel_size, stride, padding) -> Rulebook:
    """The ``Rulebook`` of a layer geometry on ``x``, built once per ``indice_key`` (uncached without one)."""
    geo = (subm, x.spatial_shape, kernel_size, stride, padding)
    rb = x.rulebooks.get(indice_key) if indice_key is not None else None
    if rb is not None:
        if rb.geometry != geo or rb.in_coors is not x.coors:
            raise ValueError(f"indice_key {indice_key!r} was built for another geometry or another sparse tensor")
        return rb
    out_shape = ops.sparse_conv_geometry(x.spatial_shape, kernel_size, stride, padding, subm)[4]
    rb = Rulebook(geo, x.coors, x.offsets, *ops.sparse_conv_index(x.coors, x.offsets, x.spatial_shape, kernel_size, stride, padding, subm),
                  out_shape)
    if indice_key is not None:
        x.rulebooks[indice_key] = rb
    return rb


class _SparseConvBase(nn.Module):
    subm = False

    def __init__(self, in_channels: int, out_channels: int, kernel_size=3, stride=1, padding=0, bias: bool = True, relu: bool = False,
                 indice_key: Optional[str] = None):
        super().__init__()
        # (shape checks on fixed sizes; the layer's own geometry is checked here so that a bad layer fails at construction)
        _, self.kernel_size, self.stride, self.padding, _ = ops.sparse_conv_geometry((3, 3, 3), kernel_size, stride, padding, self.subm)
        self.in_channels, self.out_channels = int(in_channels), int(out_channels)
        kvol = self.kernel_size[0] * self.kernel_size[1] * self.kernel_size[2]
        ops._sparse_limits(type(self).__name__, kvol, self.in_channels, self.out_channels)
        self.relu = bool(relu)
        self.indice_key = indice_key
        self.weight = nn.Parameter(torch.empty((kvol, self.out_channels, self.in_channels), dtype=torch.float32), requires_grad=False)
        self.bias = nn.Parameter(torch.zeros((self.out_channels,), dtype=torch.float32), requires_grad=False) if bias else None
        nn.init.uniform_(self.weight, -(kvol * in_channels) ** -0.5, (kvol * in_channels) ** -0.5)
        self._packed = None         # (key of the parameters it was made from, ops.PackedSparseWeight)
        self._packed_t = None       # the same for W^T (no bias): the weights of the input gradient (§21.4)

    @staticmethod
    def from_conv3d_weight(w: torch.Tensor) -> torch.Tensor:
        """``torch.nn.Conv3d`` weight [Cout,Cin,Kz,Ky,Kx] -> this module's [Kvol,Cout,Cin] (kk = (kz*Ky + ky)*Kx + kx)."""
        if w.dim() != 5:
            raise ValueError(f"[Cout,Cin,Kz,Ky,Kx] expected, got {tuple(w.shape)}")
        co, ci = w.shape[:2]
        return w.permute(2, 3, 4, 0, 1).reshape(-1, co, ci).contiguous()

    def packed(self) -> "ops.PackedSparseWeight":
        key = (self.weight.data_ptr(), self.weight._version, None if self.bias is None else (self.bias.data_ptr(), self.bias._version))
        if self._packed is None or self._packed[0] != key:
            self._packed = (key, ops.PackedSparseWeight(self.weight.data, None if self.bias is None else self.bias.data))
        return self._packed[1]

    def packed_t(self) -> "ops.PackedSparseWeight":
        key = (self.weight.data_ptr(), self.weight._version)
        if self._packed_t is None or self._packed_t[0] != key:
            self._packed_t = (key, ops.PackedSparseWeight(self.weight.data.transpose(1, 2).contiguous(), None))
        return self._packed_t[1]

    def rulebook(self, x: SparseTensor) -> Rulebook:
        return _rulebook(x, self.indice_key, self.subm, self.kernel_size, self.stride, self.padding)

    def forward(self, x: SparseTensor, residual: Optional[torch.Tensor] = None) -> SparseTensor:
        if x.feat.shape[1] != self.in_channels:
            raise ValueError(f"{self.in_channels} input channels expected, got {x.feat.shape[1]}")
        train = wants_grad(x.feat, self.weight, self.bias, residual)
        with torch.no_grad():
            rb = self.rulebook(x)
            if not train:
                out = ops.sparse_conv(x.feat, rb.nbr, self.packed(), None, residual, self.relu)
        if train:
            out = autograd.sparse_conv(x.feat, self.weight, self.bias, residual, rb.nbr, self.relu, rb.transposed, self.packed(), self.packed_t)
        return x.derive(out, rb.out_coors, rb.out_offsets, rb.out_shape)

    def extra_repr(self) -> str:
        return (f"{self.in_channels}, {self.out_channels}, kernel_size={self.kernel_size}, stride={self.stride}, padding={self.padding}, "
                f"bias={self.bias is not None}, relu={self.relu}, indice_key={self.indice_key!r}")


class SubMConv3d(_SparseConvBase):
    """Submanifold convolution: odd kernel, stride 1, padding K // 2; the active set does not grow (out rows = in rows)."""
    subm = True

    def __init__(self, in_channels: int, out_channels: int, kernel_size=3, bias: bool = True, relu: bool = False, indice_key: Optional[str] = None):
        super().__init__(in_channels, out_channels, kernel_size, 1, 0, bias, relu, indice_key)


class SparseConv3d(_SparseConvBase):
    """Strided sparse convolution: an output site is active iff its window holds an active input; numbered per scene in order of
    first appearance (§21.1).  Builds its rulebook with one synchronisation (the row count is read back)."""
    subm = False


class SparseInverseConv3d(_SparseConvBase):
    """Inverse convolution (SPEC.md §22.3): the up-sampling layer of a sparse U-Net.  Applied to the tensor that the strided layer
    named by ``indice_key`` (a ``SparseConv3d`` or a ``SparseMaxPool3d``) produced — possibly after submanifold layers or
    ``replace_feature``, which keep ``coors`` — it writes the rows of that layer's INPUT: ``sparse_conv`` over the transposed
    rulebook with this layer's own weights, the same ``kk`` in both directions (no flipped kernel).  The output carries the
    partner's input ``coors`` / ``offsets`` (the same tensor objects) and ``spatial_shape``, so skip connections line up row for
    row and a submanifold ``indice_key`` of that resolution is a cache hit.  An input row that no window of the partner covers gets
    the bias (+ residual) alone."""
    subm = False

    def __init__(self, in_channels: int, out_channels: int, kernel_size, indice_key: str, bias: bool = True, relu: bool = False):
        if indice_key is None:
            raise ValueError("SparseInverseConv3d needs the indice_key of the strided layer it inverts")
        super().__init__(in_channels, out_channels, kernel_size, 1, 0, bias, relu, indice_key)
        self.stride = self.padding = None          # the partner's, found with its rulebook

    def rulebook(self, x: SparseTensor) -> Rulebook:
        """-> the partner layer's rulebook, after the checks of §22.3."""
        key = self.indice_key
        rb = x.rulebooks.get(key)
        if rb is None:
            raise ValueError(f"SparseInverseConv3d: no rulebook under indice_key {key!r} (the strided layer it inverts must run first, on "
                             "a tensor this one derives from)")
        subm, _, kernel_size, _, _ = rb.geometry
        if subm:
            raise ValueError(f"SparseInverseConv3d: indice_key {key!r} names a submanifold rulebook; a strided layer is expected")
        if kernel_size != self.kernel_size:
            raise ValueError(f"SparseInverseConv3d: kernel_size {self.kernel_size} differs from {kernel_size} of indice_key {key!r}")
        if x.coors is not rb.out_coors:
            raise ValueError(f"SparseInverseConv3d: the input is not the tensor that the layer of indice_key {key!r} produced")
        return rb

    def forward(self, x: SparseTensor, residual: Optional[torch.Tensor] = None) -> SparseTensor:
        if x.feat.shape[1] != self.in_channels:
            raise ValueError(f"{self.in_channels} input channels expected, got {x.feat.shape[1]}")
        rb = self.rulebook(x)
        train = wants_grad(x.feat, self.weight, self.bias, residual)
        with torch.no_grad():
            nbrT, collisions = rb.transposed()
            if not train:
                out = ops.sparse_conv(x.feat, nbrT, self.packed(), None, residual, self.relu)
        if train:
            # (the roles of §21.4 swapped: the rulebook of this convolution is nbrT, and its transpose is nbr when nothing collided)
            out = autograd.sparse_conv(x.feat, self.weight, self.bias, residual, nbrT, self.relu, (rb.nbr, collisions), self.packed(), self.packed_t)
        return x.derive(out, rb.in_coors, rb.in_offsets, rb.geometry[1])

    def extra_repr(self) -> str:
        return (f"{self.in_channels}, {self.out_channels}, kernel_size={self.kernel_size}, indice_key={self.indice_key!r}, "
                f"bias={self.bias is not None}, relu={self.relu}")


class SparseMaxPool3d(nn.Module):
    """Sparse max pool (SPEC.md §22.1): the active output sites and the windows of a ``SparseConv3d`` of the same geometry (the two
    may share an ``indice_key``), per channel the maximum over the ACTIVE inputs of the window (an absent voxel is absent, not a
    zero).  No parameters.  Exact; its backward is a gather over the transposed rulebook (§22.2), exact as well."""

    def __init__(self, kernel_size, stride=None, padding=0, indice_key: Optional[str] = None):
        super().__init__()
        _, self.kernel_size, self.stride, self.padding, _ = ops.sparse_conv_geometry((3, 3, 3), kernel_size,
                                                                                      kernel_size if stride is None else stride, padding, False)
        self.indice_key = indice_key

    def rulebook(self, x: SparseTensor) -> Rulebook:
        return _rulebook(x, self.indice_key, False, self.kernel_size, self.stride, self.padding)

    def forward(self, x: SparseTensor) -> SparseTensor:
        train = wants_grad(x.feat)
        with torch.no_grad():
            rb = self.rulebook(x)
            if not train:
                out = ops.sparse_max_pool(x.feat, rb.nbr)[0]
        if train:
            out = autograd.sparse_max_pool(x.feat, rb.nbr, rb.transposed)
        return x.derive(out, rb.out_coors, rb.out_offsets, rb.out_shape)

    def extra_repr(self) -> str:
        return f"kernel_size={self.kernel_size}, stride={self.stride}, padding={self.padding}, indice_key={self.indice_key!r}"


class SparseSequential(nn.Sequential):
    """``nn.Sequential`` over sparse layers; a dense module in the chain (e.g. an activation) is applied to ``.feat``."""

    def forward(self, x: SparseTensor) -> SparseTensor:
        for m in self:
            if isinstance(m, (_SparseConvBase, SparseMaxPool3d, SparseSequential)):
                x = m(x)
            else:
                x = x.replace_feature(m(x.feat))
        return x
