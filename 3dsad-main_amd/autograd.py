"""Differentiable forms of the unfused operators (SPEC.md §16).

``group_points`` / ``gather_points`` / ``max_pool_s`` (and ``three_interpolate`` §18, ``voxel_reduce`` §20.5, ``sparse_conv`` /
``sparse_to_dense`` §21.4, ``sparse_max_pool`` §22.2) as ``torch.autograd.Function``s whose forward
AND backward are this package's HIP kernels (float32 only): the classic unfused
``group -> shared MLP (any torch layers) -> max over nsample`` stack becomes trainable without a
PyTorch-side scatter.  The fused chains have a backward of their own (SPEC.md §32): ``GroupedMLP`` / ``MLPRows`` run
``PackedMLP.grouped`` / ``.rows`` forward, keep the inputs and the output only, and recompute the activations in
``ops.grouped_mlp_grad`` / ``ops.mlp_rows_grad``.
"""
import torch
from torch.autograd.function import once_differentiable

from . import ops
from ._lib import check, lib


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _f32(t, name, ndim):
    if not t.is_cuda or t.dtype != torch.float32 or t.dim() != ndim:
        raise TypeError(f"{name}: expected a GPU float32 tensor with {ndim} dims (sad_amd has no CPU path)")
    return t.contiguous()


def group_points_grad(grad_out: torch.Tensor, idx: torch.Tensor, N: int, point_major: bool = False,
                      via_point_major: bool = True) -> torch.Tensor:
    """grad_out [B,C,M,S] (or [B,C,M] with idx [B,M]) -> grad_feat [B,C,N] (scatter-add), or
    [B,N,C] with ``point_major=True``.  By default the sum is formed point-major (contiguous float
    atomics, ~10x faster) and transposed at the end; ``via_point_major=False`` uses the direct
    channel-major scatter."""
    if grad_out.dim() == 3:
        grad_out, idx = grad_out.unsqueeze(-1), idx.unsqueeze(-1)
    grad_out = _f32(grad_out, "grad_out", 4)
    if idx.dtype != torch.int32 or not idx.is_cuda:
        raise TypeError("idx: expected a GPU int32 tensor")
    idx = idx.contiguous()
    B, C, M, S = grad_out.shape
    if tuple(idx.shape) != (B, M, S):
        raise ValueError("idx must be [B,M,S]")
    if point_major or via_point_major:
        g = torch.zeros((B, N, C), dtype=torch.float32, device=grad_out.device)
        check(lib().sad_group_points_grad_pm_f32(grad_out.data_ptr(), idx.data_ptr(), B, C, N, M, S, g.data_ptr(),
                                                 _stream()), "sad_group_points_grad_pm_f32")
        return g if point_major else g.transpose(1, 2).contiguous()
    g = torch.zeros((B, C, N), dtype=torch.float32, device=grad_out.device)
    check(lib().sad_group_points_grad_f32(grad_out.data_ptr(), idx.data_ptr(), B, C, N, M, S, g.data_ptr(),
                                          _stream()), "sad_group_points_grad_f32")
    return g


class GroupPoints(torch.autograd.Function):
    """features [B,C,N] f32, idx [B,M,S] int32 -> [B,C,M,S]."""

    @staticmethod
    def forward(ctx, features, idx):
        ctx.save_for_backward(idx)
        ctx.N = features.shape[2]
        return ops.group_points(_f32(features, "features", 3), idx)

    @staticmethod
    def backward(ctx, grad_out):
        (idx,) = ctx.saved_tensors
        return group_points_grad(grad_out, idx, ctx.N), None


class GatherPoints(torch.autograd.Function):
    """features [B,C,N] f32, idx [B,M] int32 -> [B,C,M]."""

    @staticmethod
    def forward(ctx, features, idx):
        ctx.save_for_backward(idx)
        ctx.N = features.shape[2]
        return ops.gather_points(_f32(features, "features", 3), idx)

    @staticmethod
    def backward(ctx, grad_out):
        (idx,) = ctx.saved_tensors
        return group_points_grad(grad_out, idx, ctx.N), None


def max_pool_s_with_arg(x: torch.Tensor):
    """x [B,C,M,S] -> (out [B,C,M], arg [B,C,M] int32); ties -> lowest s."""
    x = _f32(x, "x", 4)
    B, C, M, S = x.shape
    out = torch.empty((B, C, M), dtype=torch.float32, device=x.device)
    arg = torch.empty((B, C, M), dtype=torch.int32, device=x.device)
    check(lib().sad_max_pool_s_f32(x.data_ptr(), B, C, M, S, out.data_ptr(), arg.data_ptr(), _stream()),
          "sad_max_pool_s_f32")
    return out, arg


class MaxPoolS(torch.autograd.Function):
    """x [B,C,M,S] -> max over S, gradient routed to the arg-max slot."""

    @staticmethod
    def forward(ctx, x):
        out, arg = max_pool_s_with_arg(x)
        ctx.save_for_backward(arg)
        ctx.S = x.shape[3]
        return out

    @staticmethod
    def backward(ctx, grad_out):
        (arg,) = ctx.saved_tensors
        grad_out = _f32(grad_out, "grad_out", 3)
        B, C, M = grad_out.shape
        gx = torch.empty((B, C, M, ctx.S), dtype=torch.float32, device=grad_out.device)
        check(lib().sad_max_pool_s_grad_f32(grad_out.data_ptr(), arg.data_ptr(), B, C, M, ctx.S, gx.data_ptr(),
                                            _stream()), "sad_max_pool_s_grad_f32")
        return gx


def three_interpolate_grad(grad_out: torch.Tensor, idx: torch.Tensor, w: torch.Tensor, m: int,
                           point_major: bool = False) -> torch.Tensor:
    """SPEC.md §18: grad_out [B,C,n] (or [B,n,C] with ``point_major=True``), idx / w [B,n,3] -> grad_feat [B,C,m] (or [B,m,C]):
    ``grad_feat[.., idx_k] += w_k * grad_out``.  The sum is formed point-major (contiguous float atomics) and transposed at the
    end for the channel-major layout.  idx and w get no gradient."""
    grad_out = _f32(grad_out, "grad_out", 3)
    if idx.dtype != torch.int32 or not idx.is_cuda:
        raise TypeError("idx: expected a GPU int32 tensor")
    w = _f32(w, "w", 3)
    idx = idx.contiguous()
    if point_major:
        B, n, C = grad_out.shape
    else:
        B, C, n = grad_out.shape
    if tuple(idx.shape) != (B, n, 3) or tuple(w.shape) != (B, n, 3):
        raise ValueError("idx and w must be [B,n,3]")
    g = torch.zeros((B, m, C), dtype=torch.float32, device=grad_out.device)
    check(lib().sad_three_interpolate_grad_f32(grad_out.data_ptr(), idx.data_ptr(), w.data_ptr(), B, C, n, m, int(bool(point_major)),
                                               g.data_ptr(), _stream()), "sad_three_interpolate_grad_f32")
    return g if point_major else g.transpose(1, 2).contiguous()


class ThreeInterpolate(torch.autograd.Function):
    """features [B,C,m] f32 (or [B,m,C] with point_major), idx [B,n,3] int32, w [B,n,3] f32 -> [B,C,n] (or [B,n,C]).
    Gradient for the features only: idx and w get none (as in the libraries this replaces)."""

    @staticmethod
    def forward(ctx, features, idx, w, point_major=False):
        ctx.save_for_backward(idx, w)
        ctx.point_major = bool(point_major)
        ctx.m = features.shape[1] if point_major else features.shape[2]
        return ops.three_interpolate(_f32(features, "features", 3), idx, w, point_major=point_major)

    @staticmethod
    def backward(ctx, grad_out):
        idx, w = ctx.saved_tensors
        return three_interpolate_grad(grad_out, idx, w, ctx.m, point_major=ctx.point_major), None, None, None


class VoxelReduce(torch.autograd.Function):
    """feat [total,Cf] f32, point2voxel [total] int32, offsets [B+1] int32 -> out [B,V,Cf] (SPEC.md §20.5).  Gradient for the
    features only (a gather, exact); point2voxel and offsets get none.  ``mode`` "max" returns the values only."""

    @staticmethod
    def forward(ctx, feat, point2voxel, offsets, max_voxels, mode="mean"):
        feat = _f32(feat, "feat", 2)
        ctx.mode = mode
        aux = None
        if mode == "max":
            out, aux = ops.voxel_reduce(feat, point2voxel, offsets, max_voxels, "max")
        elif mode == "mean":
            out, aux = ops.voxel_reduce(feat, point2voxel, offsets, max_voxels, "mean", return_count=True)
        else:
            out = ops.voxel_reduce(feat, point2voxel, offsets, max_voxels, mode)
        ctx.has_aux = aux is not None
        ctx.save_for_backward(*((point2voxel, offsets) + ((aux,) if aux is not None else ())))
        return out

    @staticmethod
    def backward(ctx, grad_out):
        saved = ctx.saved_tensors
        g = ops.voxel_reduce_grad(_f32(grad_out, "grad_out", 3), saved[0], saved[1], ctx.mode, saved[2] if ctx.has_aux else None)
        return g, None, None, None, None


class VoxelEncode(torch.autograd.Function):
    """The voxel feature encoder (SPEC.md §24) with gradients for points, weight, bias and vox_feat.  The forward is the fused
    operator with ``arg``; the backward is a composition of existing operators: the routed gradient (``voxel_reduce_grad`` with
    ``arg``), the decorated rows (``voxel_decorate``), two matrix products and the ordered sum for ``vox_feat``.  The mean and the
    voxel centre are constants of the row: no gradient flows through them; point2voxel, offsets and coors get none."""

    @staticmethod
    def forward(ctx, points, point2voxel, offsets, max_voxels, weight, bias, coors, voxel_size, point_range, cluster_center, voxel_center,
                relu, vox_feat, max_points, return_pointwise):
        points = _f32(points, "points", 2)
        res = ops.voxel_encode(points, point2voxel, offsets, max_voxels, weight, bias, coors, voxel_size, point_range, cluster_center,
                               voxel_center, relu, vox_feat, max_points, return_arg=True, return_pointwise=return_pointwise)
        pooled, arg = res[0], res[1]
        pointwise = res[2] if return_pointwise else None
        ctx.cfg = (int(max_voxels), voxel_size, point_range, bool(cluster_center), bool(voxel_center), bool(relu), max_points)
        ctx.has = (coors is not None, vox_feat is not None, pointwise is not None)
        ctx.save_for_backward(*[t for t in (points, point2voxel, offsets, weight, arg, pooled, coors, vox_feat, pointwise) if t is not None])
        return (pooled, pointwise) if return_pointwise else pooled

    @staticmethod
    def backward(ctx, grad_pooled, grad_pointwise=None):
        V, voxel_size, point_range, cc, vc, relu, T = ctx.cfg
        saved = list(ctx.saved_tensors)
        points, p2v, offsets, weight, arg, pooled = saved[:6]
        rest = saved[6:]
        coors = rest.pop(0) if ctx.has[0] else None
        vox_feat = rest.pop(0) if ctx.has[1] else None
        pointwise = rest.pop(0) if ctx.has[2] else None
        total, C = points.shape
        gp = _f32(grad_pooled, "grad_pooled", 3)
        if relu:
            gp = torch.where(pooled > 0, gp, torch.zeros_like(gp))      # y of the arg row IS the pooled value
        g = ops.voxel_reduce_grad(gp, p2v, offsets, "max", arg)
        if pointwise is not None and grad_pointwise is not None:
            # rows that are not members have the constant output 0: a column of ones decorated alone marks the members
            member = ops.voxel_decorate(torch.ones((total, 1), dtype=torch.float32, device=points.device), p2v, offsets, V,
                                        cluster_center=False, voxel_center=False, max_points=T)
            live = (member > 0) & (pointwise > 0) if relu else (member > 0)
            g = g + torch.where(live, grad_pointwise, torch.zeros_like(grad_pointwise))
        rows = ops.voxel_decorate(points, p2v, offsets, V, coors, voxel_size, point_range, cc, vc, vox_feat, T)
        grad_w = g.t() @ rows if ctx.needs_input_grad[4] else None
        grad_b = g.sum(0) if ctx.needs_input_grad[5] else None
        grad_points = grad_vox = None
        if ctx.needs_input_grad[0] or (vox_feat is not None and ctx.needs_input_grad[12]):
            grad_rows = g @ weight
            if ctx.needs_input_grad[0]:
                grad_points = grad_rows[:, :C].clone()
                for k in range(int(cc) + int(vc)):
                    grad_points[:, :3] += grad_rows[:, C + 3 * k:C + 3 * k + 3]
            if vox_feat is not None and ctx.needs_input_grad[12]:
                Cv = vox_feat.shape[2]
                grad_vox = ops.voxel_reduce(grad_rows[:, grad_rows.shape[1] - Cv:].contiguous(), p2v, offsets, V, "sum")
        return (grad_points, None, None, None, grad_w, grad_b, None, None, None, None, None, None, grad_vox, None, None)


def voxel_encode(points, point2voxel, offsets, max_voxels, weight, bias, coors=None, voxel_size=None, point_range=None,
                 cluster_center=True, voxel_center=True, relu=True, vox_feat=None, max_points=None, return_pointwise=False):
    """Differentiable ``ops.voxel_encode`` (SPEC.md §24): points [total,C] + offsets [B+1] -> pooled [B,V,Cout], or (pooled,
    pointwise [total,Cout]) with ``return_pointwise``.  Gradients for points, weight, bias and vox_feat."""
    return VoxelEncode.apply(points, point2voxel, offsets, max_voxels, weight, bias, coors, voxel_size, point_range, cluster_center,
                             voxel_center, relu, vox_feat, max_points, return_pointwise)


def _transposed(transposed, nbr, Nv):
    """-> (nbrT, collisions as a Python int) from what ``SparseConv`` was given: None (built here, one synchronisation), a
    callable that returns the pair (a layer's cache) or the pair itself."""
    if transposed is None:
        nbrT, col = ops.sparse_conv_index_transpose(nbr, Nv)
        return nbrT, int(col.item())
    nbrT, col = transposed() if callable(transposed) else transposed
    return nbrT, int(col)


class SparseConv(torch.autograd.Function):
    """``ops.sparse_conv`` with its backward (SPEC.md §21.4): feat [Nv,Cin], weight [Kvol,Cout,Cin], bias [Cout] | None,
    residual [No,Cout] | None, nbr [No,Kvol] int32, relu -> out [No,Cout].  Gradients for feat, weight, bias and residual, each
    computed only where ``ctx.needs_input_grad`` asks: grad_W / grad_bias by ``sad_spconv_grad_weight_f32``, grad_feat by the
    forward kernel over the transposed rulebook and the packed W^T.  Optional: ``transposed`` = (nbrT, collisions) or a callable
    returning it (a layer's per-``indice_key`` cache; built on demand otherwise), ``packed`` = the ``PackedSparseWeight`` of
    (weight, bias) and ``packed_t`` = a callable returning the one of W^T (what the layers cache per parameter version).
    A transposed rulebook with collisions (an input that holds a coordinate twice, submanifold form) has no gradient for feat:
    ``ValueError``.  nbr gets no gradient."""

    @staticmethod
    def forward(ctx, feat, weight, bias, residual, nbr, relu=False, transposed=None, packed=None, packed_t=None):
        feat = _f32(feat, "feat", 2)
        weight = _f32(weight, "weight", 3)
        if packed is None:
            out = ops.sparse_conv(feat, nbr, weight, bias, residual, relu)
        else:
            out = ops.sparse_conv(feat, nbr, packed, None, residual, relu)
        ctx.relu, ctx.transposed, ctx.packed_t = bool(relu), transposed, packed_t
        ctx.save_for_backward(feat, weight, nbr, out if relu else None)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        feat, weight, nbr, out = ctx.saved_tensors
        need = ctx.needs_input_grad
        g = _f32(grad_out, "grad_out", 2)
        if ctx.relu:
            g = g * (out > 0)                      # exact: g or 0
        grad_feat = grad_w = grad_b = None
        if need[0]:
            nbrT, collisions = _transposed(ctx.transposed, nbr, feat.shape[0])
            if collisions:
                raise ValueError(f"sparse_conv backward: the rulebook maps {collisions} (output row, offset) pairs onto input rows that a "
                                 "lower row already holds: the input has a duplicate coordinate inside a scene (submanifold form), "
                                 "for which no gradient with respect to feat is defined (SPEC.md §21.4)")
            grad_feat = ops.sparse_conv_grad_input(g, nbrT, ctx.packed_t() if ctx.packed_t is not None else weight)
        if need[1] or need[2]:
            grad_w, grad_b = ops.sparse_conv_grad_weight(feat, nbr, g, bias=need[2], weight=need[1])   # (a frozen weight: no GEMM)
        return grad_feat, grad_w, grad_b, (g if need[3] else None), None, None, None, None, None


class SparseMaxPool(torch.autograd.Function):
    """``ops.sparse_max_pool`` with its backward (SPEC.md §22.1, §22.2): feat [Nv,C], nbr [No,Kvol] int32 -> out [No,C]; the forward
    keeps ``arg``.  Gradient for feat only, by ``ops.sparse_max_pool_grad`` over the transposed rulebook (a gather: exact and
    bit-equal from call to call).  Optional ``transposed`` as for ``SparseConv``: (nbrT, collisions), a callable returning it, or
    None (built at the backward, one synchronisation).  A transposed rulebook with collisions has no gradient: ``ValueError``."""

    @staticmethod
    def forward(ctx, feat, nbr, transposed=None):
        feat = _f32(feat, "feat", 2)
        out, arg = ops.sparse_max_pool(feat, nbr)
        ctx.Nv, ctx.transposed = feat.shape[0], transposed
        ctx.save_for_backward(arg, nbr)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        arg, nbr = ctx.saved_tensors
        if not ctx.needs_input_grad[0]:
            return None, None, None
        nbrT, collisions = _transposed(ctx.transposed, nbr, ctx.Nv)
        if collisions:
            raise ValueError(f"sparse_max_pool backward: the rulebook maps {collisions} (output row, offset) pairs onto input rows that a "
                             "lower row already holds: the input has a duplicate coordinate inside a scene (submanifold form), "
                             "for which no gradient with respect to feat is defined (SPEC.md §22.2)")
        return ops.sparse_max_pool_grad(_f32(grad_out, "grad_out", 2), arg, nbrT, ctx.Nv), None, None


class SparseToDense(torch.autograd.Function):
    """``ops.sparse_to_dense`` (SPEC.md §21.3) with its backward: feat [No,C], out_coors [No,3], out_offsets [B+1], out_shape ->
    dense [B,C,Oz,Oy,Ox].  grad_feat[o] = grad_dense at o's cell for the row that owns the cell (the lowest), zero for a shadowed
    duplicate and for a row outside ``out_shape`` — a framework gather over out_coors (exact; not a hot path; its transient memory
    is a few arrays of No entries, nothing of the size of the grid)."""

    @staticmethod
    def forward(ctx, feat, out_coors, out_offsets, out_shape):
        ctx.save_for_backward(out_coors, out_offsets)
        ctx.out_shape = tuple(int(v) for v in out_shape)
        return ops.sparse_to_dense(_f32(feat, "feat", 2), out_coors, out_offsets, out_shape)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_dense):
        coors, offsets = ctx.saved_tensors
        Oz, Oy, Ox = ctx.out_shape
        B = grad_dense.shape[0]
        No, dev = coors.shape[0], coors.device
        rows = torch.arange(No, device=dev)
        scene = (torch.searchsorted(offsets.to(torch.int64), rows, right=True) - 1).clamp(0, B - 1)
        z, y, x = (coors[:, d].to(torch.int64) for d in range(3))
        inside = (z >= 0) & (z < Oz) & (y >= 0) & (y < Oy) & (x >= 0) & (x < Ox)
        # the owner of a cell among the No rows only (nothing of the size of the grid is allocated): rows outside get ids of their own
        cell = torch.where(inside, ((scene * Oz + z) * Oy + y) * Ox + x, -1 - rows)
        _, group = torch.unique(cell, return_inverse=True)
        owner = torch.full((No,), No, dtype=torch.int64, device=dev).scatter_reduce_(0, group, rows, "amin")
        mine = inside & (owner[group] == rows)
        picked = grad_dense[scene, :, z.clamp(0, Oz - 1), y.clamp(0, Oy - 1), x.clamp(0, Ox - 1)]      # [No, C]
        return picked * mine[:, None].to(picked.dtype), None, None, None


group_points = GroupPoints.apply
sparse_conv = SparseConv.apply
sparse_max_pool = SparseMaxPool.apply
sparse_to_dense = SparseToDense.apply
voxel_reduce = VoxelReduce.apply
gather_points = GatherPoints.apply
max_pool_s = MaxPoolS.apply
three_interpolate = ThreeInterpolate.apply


def _scaled(grad: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    """grad [B,...] times w [B], broadcast per scene."""
    return grad * w.view(-1, *([1] * (grad.dim() - 1)))


class AnchorHeadLoss(torch.autograd.Function):
    """(cls, reg, dir | None, labels, reg_target, dir_target | None, cfg) -> loss [B,3] (SPEC.md §27.1), differentiable in the maps.
    The forward is ``ops.anchor_head_loss``, which already produced d loss[b, i] / d map for every component i: the backward
    multiplies the saved gradients by ``grad_loss[:, i]`` per scene (a torch multiply).  ``cfg``: the operator's keywords."""

    @staticmethod
    def forward(ctx, cls, reg, dir, labels, reg_target, dir_target, cfg):
        outs = ops.anchor_head_loss(cls, reg, dir, labels, reg_target, dir_target, **cfg)
        ctx.save_for_backward(*outs[2:5 if dir is not None else 4])
        ctx.mark_non_differentiable(outs[1])
        return outs[0], outs[1]

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_loss, _grad_num_pos):
        saved = ctx.saved_tensors
        grads = [_scaled(g, grad_loss[:, i]) for i, g in enumerate(saved)]
        return grads[0], grads[1], grads[2] if len(grads) == 3 else None, None, None, None, None


class CenterHeadLoss(torch.autograd.Function):
    """(hm, reg, height, dim, rot, vel | None, heatmap, ind, anno, cfg) -> loss [B,2] (SPEC.md §27.2), differentiable in the maps:
    grad_hm scales with ``grad_loss[:, 0]``, the regression gradients with ``grad_loss[:, 1]``."""

    @staticmethod
    def forward(ctx, hm, reg, height, dim, rot, vel, heatmap, ind, anno, cfg):
        outs = ops.center_head_loss(hm, reg, height, dim, rot, vel, heatmap, ind, anno, **cfg)
        ctx.save_for_backward(*outs[2:])
        ctx.mark_non_differentiable(outs[1])
        return outs[0], outs[1]

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_loss, _grad_num_pos):
        saved = ctx.saved_tensors
        grads = [_scaled(g, grad_loss[:, 0 if i == 0 else 1]) for i, g in enumerate(saved)]
        return (*grads, *([None] if len(grads) == 5 else []), None, None, None, None)


class RoIHeadLoss(torch.autograd.Function):
    """(rcnn_cls, rcnn_reg, cls_target, reg_valid, reg_target, rois | None, gt_local | None, cfg) -> loss [B,3], num [B,2]
    (SPEC.md §29), differentiable in the two predictions.  The forward is ``ops.roi_head_loss``, which already produced the
    gradient of every component: the backward returns ``grad_cls · g[:, 0]`` and ``grad_reg · g[:, 1] + grad_corner · g[:, 2]``
    broadcast per scene (torch multiplies), and ``None`` for the targets.  ``cfg``: the operator's keywords."""

    @staticmethod
    def forward(ctx, rcnn_cls, rcnn_reg, cls_target, reg_valid, reg_target, rois, gt_local, cfg):
        outs = ops.roi_head_loss(rcnn_cls, rcnn_reg, cls_target, reg_valid, reg_target, rois, gt_local, **cfg)
        ctx.save_for_backward(*outs[2:5 if rois is not None else 4])
        ctx.mark_non_differentiable(outs[1])
        return outs[0], outs[1]

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_loss, _grad_num):
        saved = ctx.saved_tensors
        greg = _scaled(saved[1], grad_loss[:, 1])
        if len(saved) == 3:
            greg = greg + _scaled(saved[2], grad_loss[:, 2])
        return _scaled(saved[0], grad_loss[:, 0]), greg, None, None, None, None, None, None


class PointHeadLoss(torch.autograd.Function):
    """(o, c | None, labels, centerness | None, reg_target, shift_target | None, size_target | None, cfg) -> loss [B,4], num_pos [B]
    (SPEC.md §31.2), differentiable in o and c.  The forward is ``ops.point_head_loss``, which already produced the gradient of
    every component: grad_o holds d loss[:, 0] in its first C columns and d loss[:, 1] in the last 7, grad_c d loss[:, 2] in
    columns 0..2 and d loss[:, 3] in 3..5, so the backward scales them per scene and per component (torch multiplies) and
    returns ``None`` for the targets.  ``cfg``: the operator's keywords."""

    @staticmethod
    def forward(ctx, o, c, labels, centerness, reg_target, shift_target, size_target, cfg):
        outs = ops.point_head_loss(o, c, labels, centerness, reg_target, shift_target, size_target, **cfg)
        ctx.save_for_backward(*outs[2:4 if c is not None else 3])
        ctx.mark_non_differentiable(outs[1])
        return outs[0], outs[1]

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_loss, _grad_num):
        saved = ctx.saved_tensors
        C = saved[0].shape[2] - 7
        w = torch.cat([grad_loss[:, 0:1].expand(-1, C), grad_loss[:, 1:2].expand(-1, 7)], 1)                # [B,C+7]
        go = saved[0] * w.unsqueeze(1)
        gc = None
        if len(saved) == 2:
            gc = saved[1] * torch.cat([grad_loss[:, 2:3].expand(-1, 3), grad_loss[:, 3:4].expand(-1, 3)], 1).unsqueeze(1)
        return go, gc, None, None, None, None, None, None


def _layers_of(params):
    """(W_1 .. W_L, b_1 .. b_L) -> [(W_l, b_l)]."""
    L = len(params) // 2
    return [(params[l], params[L + l]) for l in range(L)]


class GroupedMLP(torch.autograd.Function):
    """The fused grouped chain + max-pool (SPEC.md §6) with the backward of §32.  ``apply(packed, skip_empty, xyz [B,N,3],
    feat_pm [B,N,C] | None, new_xyz [B,M,3], idx [B,M,S], cnt [B,M] | None, W_1 .. W_L, b_1 .. b_L) -> pooled [B,M,C_L]``:
    ``packed`` is the ``PackedMLP`` of exactly these layers (the forward is its ``grouped``, unchanged), the unpacked tensors are
    what the backward reads and what receives the gradients.  Saved: the inputs and the output.  ``skip_empty``: groups with
    ``cnt == 0`` give no gradient (a caller that overwrites their output).  ``mismatch`` of the last backward (a 1-element int32
    GPU tensor, 0 when the recompute met every pooled value) is left in ``GroupedMLP.last_mismatch``."""
    last_mismatch = None

    @staticmethod
    def forward(ctx, packed, skip_empty, xyz, feat_pm, new_xyz, idx, cnt, *params):
        if len(params) != 2 * packed.L:
            raise ValueError("GroupedMLP: expected the chain's L weights followed by its L biases")
        out = packed.grouped(xyz, feat_pm, new_xyz, idx, cnt=cnt)
        ctx.save_for_backward(xyz, feat_pm, new_xyz, idx, cnt, out, *params)
        ctx.skip_empty = bool(skip_empty)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        xyz, feat_pm, new_xyz, idx, cnt, out, *params = ctx.saved_tensors
        want = ctx.needs_input_grad
        need = [n for n, w in (("xyz", want[2]), ("feat", want[3]), ("new_xyz", want[4]), ("params", any(want[7:]))) if w]
        gf, gx, gn, gW, gb, GroupedMLP.last_mismatch = ops.grouped_mlp_grad(
            xyz, feat_pm, new_xyz, idx, cnt, _layers_of(params), out, grad_out, skip_empty=ctx.skip_empty, need=need)
        gp = [g if w else None for g, w in zip((gW or []) + (gb or []), want[7:])] if gW is not None else [None] * len(params)
        return (None, None, gx, gf, gn, None, None, *gp)


class MLPRows(torch.autograd.Function):
    """The fused plain-row chain with the backward of §32: ``apply(packed, x [..., C_0], W_1 .. W_L, b_1 .. b_L) -> [..., C_L]``
    (``packed``: the ``PackedMLP`` of these layers, its ``relu_mask`` included).  Saved: the inputs."""

    @staticmethod
    def forward(ctx, packed, x, *params):
        if len(params) != 2 * packed.L:
            raise ValueError("MLPRows: expected the chain's L weights followed by its L biases")
        ctx.save_for_backward(x, *params)
        ctx.relu_mask = packed.relu_mask
        return packed.rows(x)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        x, *params = ctx.saved_tensors
        want = ctx.needs_input_grad
        need = [n for n, w in (("feat", want[1]), ("params", any(want[2:]))) if w]
        gx, gW, gb = ops.mlp_rows_grad(x, _layers_of(params), grad_out, relu_mask=ctx.relu_mask, need=need)
        gp = [g if w else None for g, w in zip((gW or []) + (gb or []), want[2:])] if gW is not None else [None] * len(params)
        return (None, gx, *gp)


class Candidates(torch.autograd.Function):
    """§8 steps 2-4 with the backward of §33.1: ``apply(xyz3 [B,M3,3], c [B,K,6], K, shift_max, r_min, r_max, anchor) -> (cand
    [B,K,3], radius [B,K])``.  The forward is ``ops.candidates``; ``radius`` is not differentiable (it feeds an index decision);
    the backward returns ``ops.candidates_grad`` for c.  No gradient with respect to xyz3 is offered: SA3's centroids are
    sampled input points."""

    @staticmethod
    def forward(ctx, xyz3, c, K, shift_max, r_min, r_max, anchor):
        cand, radius = ops.candidates(xyz3, c, K, shift_max, r_min, r_max, anchor)
        ctx.save_for_backward(c)
        ctx.shift_max = shift_max
        ctx.mark_non_differentiable(radius)
        return cand, radius

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_cand, _grad_radius):
        (c,) = ctx.saved_tensors
        return None, ops.candidates_grad(c, grad_cand.contiguous(), ctx.shift_max), None, None, None, None, None


class PrefixRows(torch.autograd.Function):
    """``apply(x [B,M,C] f32, K) -> x[:, :K]`` packed (``ops.prefix_rows``, one library launch) with the backward of §33.2
    (``ops.prefix_rows_grad``: the padded gradient in one launch, no zero fill).  ``K == M``: the identity, no copy."""

    @staticmethod
    def forward(ctx, x, K):
        ctx.M = x.shape[1]
        return x if K == ctx.M else ops.prefix_rows(_f32(x, "x", 3), K)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        if grad_out.shape[1] == ctx.M:
            return grad_out, None
        return ops.prefix_rows_grad(grad_out.contiguous(), ctx.M), None
