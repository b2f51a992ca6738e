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
from .ops import group_points_grad, max_pool_s_with_arg, three_interpolate_grad  # noqa: F401  (the backward operators live in ops)


class GroupPoints(torch.autograd.Function):
    """features [B,C,N] f32, idx [B,M,S] int32 -> [B,C,M,S]."""

    @staticmethod
    def forward(ctx, features, idx):
        ctx.save_for_backward(idx)
        ctx.N = features.shape[2]
        return ops.group_points(features, idx)

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
        return ops.gather_points(features, idx)

    @staticmethod
    def backward(ctx, grad_out):
        (idx,) = ctx.saved_tensors
        return group_points_grad(grad_out, idx, ctx.N), None


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
        return ops.max_pool_s_grad(grad_out, arg, ctx.S)


class ThreeInterpolate(torch.autograd.Function):
    """features [B,C,m] f32 (or [B,m,C] with point_major), idx [B,n,3] int32, w [B,n,3] f32 -> [B,C,n] (or [B,n,C]).
    Gradient for the features only: idx and w get none (as in the libraries this replaces)."""

    @staticmethod
    def forward(ctx, features, idx, w, point_major=False):
        ctx.save_for_backward(idx, w)
        ctx.point_major = bool(point_major)
        ctx.m = features.shape[1] if point_major else features.shape[2]
        return ops.three_interpolate(features, idx, w, point_major=point_major)

    @staticmethod
    def backward(ctx, grad_out):
        idx, w = ctx.saved_tensors
        return three_interpolate_grad(grad_out, idx, w, ctx.m, point_major=ctx.point_major), None, None, None


class VoxelReduce(torch.autograd.Function):
    """feat [total,Cf] f32, point2voxel [total] int32, offsets [B+1] int32 -> out [B,V,Cf] (SPEC.md §20.5).  Gradient for the
    features only (a gather, exact); point2voxel and offsets get none.  ``mode`` "max" returns the values only."""

    @staticmethod
    def forward(ctx, feat, point2voxel, offsets, max_voxels, mode="mean"):
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
        g = ops.voxel_reduce_grad(grad_out, saved[0], saved[1], ctx.mode, saved[2] if ctx.has_aux else None)
        return g, None, None, None, None


class VoxelEncode(torch.autograd.Function):
    """The voxel feature encoder (SPEC.md §24) with gradients for points, weight, bias and vox_feat.  The forward is the fused
    operator with ``arg``; the backward is a composition of existing operators: the routed gradient (``voxel_reduce_grad`` with
    ``arg``), the decorated rows (``voxel_decorate``), two matrix products and the ordered sum for ``vox_feat``.  The mean and the
    voxel centre are constants of the row: no gradient flows through them; point2voxel, offsets and coors get none."""

    @staticmethod
    def forward(ctx, points, point2voxel, offsets, max_voxels, weight, bias, coors, voxel_size, point_range, cluster_center, voxel_center,
                relu, vox_feat, max_points, return_pointwise):
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
        gp = grad_pooled
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


def _transposed(transposed, nbr, Nv, op: str, section: str):
    """-> nbrT of a backward of ``op`` (SPEC.md ``section``) from what its Function was given: None (built here, one
    synchronisation), a callable that returns the pair (nbrT, collisions) (a layer's cache) or the pair itself.  A transposed
    rulebook with collisions has no gradient: ``ValueError``."""
    if transposed is None:
        nbrT, col = ops.sparse_conv_index_transpose(nbr, Nv)
        col = col.item()
    else:
        nbrT, col = transposed() if callable(transposed) else transposed
    if int(col):
        raise ValueError(f"{op} backward: the rulebook maps {int(col)} (output row, offset) pairs onto input rows that a "
                         "lower row already holds: the input has a duplicate coordinate inside a scene (submanifold form), "
                         f"for which no gradient with respect to feat is defined (SPEC.md {section})")
    return nbrT


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
        if not feat.is_cuda:                       # (the type this Function has always raised; the operators raise RuntimeError)
            raise TypeError("feat: expected a GPU float32 tensor (sad_amd has no CPU path)")
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
        g = grad_out * (out > 0) if ctx.relu else grad_out      # exact: g or 0
        grad_feat = grad_w = grad_b = None
        if need[0]:
            nbrT = _transposed(ctx.transposed, nbr, feat.shape[0], "sparse_conv", "§21.4")
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
        nbrT = _transposed(ctx.transposed, nbr, ctx.Nv, "sparse_max_pool", "§22.2")
        return ops.sparse_max_pool_grad(grad_out, arg, nbrT, ctx.Nv), None, None


class SparseToDense(torch.autograd.Function):
    """``ops.sparse_to_dense`` (SPEC.md §21.3) with its backward: feat [No,C], out_coors [No,3], out_offsets [B+1], out_shape ->
    dense [B,C,Oz,Oy,Ox].  grad_feat[o] = grad_dense at o's cell for the row that owns the cell (the lowest), zero for a shadowed
    duplicate and for a row outside ``out_shape`` — a framework gather over out_coors (exact; not a hot path; its transient memory
    is a few arrays of No entries, nothing of the size of the grid)."""

    @staticmethod
    def forward(ctx, feat, out_coors, out_offsets, out_shape):
        ctx.save_for_backward(out_coors, out_offsets)
        ctx.out_shape = tuple(int(v) for v in out_shape)
        return ops.sparse_to_dense(feat, out_coors, out_offsets, out_shape)

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


def _scale_saved(saved, grad_loss: torch.Tensor, table) -> dict:
    """The backward of a loss whose forward already produced the gradient of every component: saved [g_0, g_1, ...] (each
    [B,...]), grad_loss [B,n] and ``table[i]`` = (input that g_i is a gradient of, columns of grad_loss that scale g_i per scene)
    -> {input: gradient}.  Columns: an int (the whole tensor), or ((width, column), ...) = blocks along the last axis of g_i, one
    width ``None`` = what the others leave.  Two saved tensors of one input are summed in the order of the table.  Every element
    is one float32 multiply (and that add).  A ``saved`` shorter than the table: the optional last gradient is absent."""
    grads = {}
    for g, (slot, cols) in zip(saved, table):
        if isinstance(cols, int):
            w = grad_loss[:, cols].view(-1, *([1] * (g.dim() - 1)))
        else:
            rest = g.shape[-1] - sum(n for n, _ in cols if n is not None)
            w = torch.cat([grad_loss[:, c:c + 1].expand(-1, rest if n is None else n) for n, c in cols], 1)
            w = w.view(-1, *([1] * (g.dim() - 2)), g.shape[-1])
        grads[slot] = g * w if slot not in grads else grads[slot] + g * w
    return grads


class _HeadLoss(torch.autograd.Function):
    """``apply(*inputs, cfg) -> (loss [B,n], counts)``, differentiable in the predictions.  The forward is ``op(*inputs, **cfg)``
    (``cfg``: the operator's keywords), which returns (loss, counts, one gradient per row of ``table``, ...): the gradients are
    saved, without the last when input ``optional`` is ``None``, the counts are not differentiable, and the backward is
    ``_scale_saved`` (torch multiplies), ``None`` for every other input.  A subclass declares ``op``, ``table`` and ``optional``
    (``forward`` / ``backward`` are class methods to read them)."""
    op = table = optional = None

    @classmethod
    def forward(cls, ctx, *args):
        outs = cls.op(*args[:-1], **args[-1])
        ctx.save_for_backward(*outs[2:2 + len(cls.table) - (args[cls.optional] is None)])
        ctx.mark_non_differentiable(outs[1])
        ctx.n_args = len(args)
        return outs[0], outs[1]

    @classmethod
    @once_differentiable
    def backward(cls, ctx, grad_loss, _grad_counts):
        grads = _scale_saved(ctx.saved_tensors, grad_loss, cls.table)
        return tuple(grads.get(i) for i in range(ctx.n_args))


class AnchorHeadLoss(_HeadLoss):
    """(cls, reg, dir | None, labels, reg_target, dir_target | None, cfg) -> loss [B,3], num_pos [B] (SPEC.md §27.1), differentiable
    in the maps: the gradient of map i scales with ``grad_loss[:, i]``."""
    op, optional = ops.anchor_head_loss, 2
    table = ((0, 0), (1, 1), (2, 2))


class CenterHeadLoss(_HeadLoss):
    """(hm, reg, height, dim, rot, vel | None, heatmap, ind, anno, cfg) -> loss [B,2], num_pos [B,2] (SPEC.md §27.2), differentiable
    in the maps: grad_hm scales with ``grad_loss[:, 0]``, the regression gradients with ``grad_loss[:, 1]``."""
    op, optional = ops.center_head_loss, 5
    table = ((0, 0), (1, 1), (2, 1), (3, 1), (4, 1), (5, 1))


class RoIHeadLoss(_HeadLoss):
    """(rcnn_cls, rcnn_reg, cls_target, reg_valid, reg_target, rois | None, gt_local | None, cfg) -> loss [B,3], num [B,2]
    (SPEC.md §29), differentiable in the two predictions: ``grad_cls · g[:, 0]`` and ``grad_reg · g[:, 1] + grad_corner · g[:, 2]``
    (the corner term with ``rois``)."""
    op, optional = ops.roi_head_loss, 5
    table = ((0, 0), (1, 1), (1, 2))


class PointHeadLoss(_HeadLoss):
    """(o, c | None, labels, centerness | None, reg_target, shift_target | None, size_target | None, cfg) -> loss [B,4], num_pos [B]
    (SPEC.md §31.2), differentiable in o and c: grad_o holds d loss[:, 0] in its first C columns and d loss[:, 1] in the last 7,
    grad_c d loss[:, 2] in columns 0..2 and d loss[:, 3] in 3..5."""
    op, optional = ops.point_head_loss, 1
    table = ((0, ((None, 0), (7, 1))), (1, ((3, 2), (3, 3))))


class RotatedIoULoss(torch.autograd.Function):
    """``apply(pred [...,Dp], target [...,Dt], weight [...] | None, rois [...,D] | None, cfg) -> (loss [...], iou [...])``
    (SPEC.md §34), differentiable in ``pred``; ``cfg`` = the operator's ``mode`` / ``kind`` / ``code``.  The forward runs
    ``ops.rotated_iou_loss`` and saves its ``grad``; the backward returns ``grad · g[..., None]`` (torch multiplies; zero in the
    columns of ``pred`` beyond the seventh) and ``None`` for target, weight and rois.  ``iou`` is not differentiable."""

    @staticmethod
    def forward(ctx, pred, target, weight, rois, cfg):
        loss, iou, grad = ops.rotated_iou_loss(pred, target, weight, rois=rois, need_grad=True, **cfg)
        ctx.save_for_backward(grad)
        ctx.mark_non_differentiable(iou)
        ctx.extra = pred.shape[-1] - 7
        return loss, iou

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_loss, _grad_iou):
        (grad,) = ctx.saved_tensors
        g = grad * grad_loss[..., None]
        return (torch.nn.functional.pad(g, (0, ctx.extra)) if ctx.extra else g), None, None, None, None


def _layers_of(params):
    """(W_1 .. W_L, b_1 .. b_L) -> [(W_l, b_l)]."""
    L = len(params) // 2
    return [(params[l], params[L + l]) for l in range(L)]


def _param_grads(gW, gb, want) -> list:
    """grad_W [L] and grad_b [L] of a chain's backward (both ``None`` when no parameter asked) -> the gradients of ``*params``
    (W_1 .. W_L, b_1 .. b_L), ``None`` where ``want`` (their ``needs_input_grad``) is false."""
    return [g if w else None for g, w in zip(gW + gb, want)] if gW is not None else [None] * len(want)


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
        return (None, None, gx, gf, gn, None, None, *_param_grads(gW, gb, want[7:]))


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
        return (None, gx, *_param_grads(gW, gb, want[2:]))


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
        return x if K == ctx.M else ops.prefix_rows(x.contiguous(), K)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        if grad_out.shape[1] == ctx.M:
            return grad_out, None
        return ops.prefix_rows_grad(grad_out.contiguous(), ctx.M), None
