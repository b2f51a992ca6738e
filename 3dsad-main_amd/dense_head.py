"""Dense BEV heads (SPEC.md §25): the raw maps of an anchor head (SECOND, PointPillars, PV-RCNN's RPN) or a centre head
(CenterPoint) -> ``(boxes, scores, labels)``, and on through ``ops.nms_boxes``.  The 2-D convolutions that produce the maps
are torch's; these modules hold the decode configuration only and have no parameters.  The decode is inference only.

The way back (SPEC.md §26): ``AnchorTargetAssigner`` / ``CenterTargetAssigner`` turn ground-truth boxes into what such a head
is trained against, from the same configuration (``decoder.assigner(...)``), and ``AnchorHeadLoss`` / ``CenterHeadLoss``
(SPEC.md §27, ``decoder.loss(...)``) are the losses on those targets: one fused pass that also writes the gradient of every
map, wrapped in an autograd Function, so ``loss.sum().backward()`` reaches the convolutions."""
from typing import Optional, Sequence, Tuple

import torch
from torch import nn

from . import ops


def anchor_grid(point_range: Sequence[float], H: int, W: int) -> Tuple[Tuple[float, float], Tuple[float, float]]:
    """``(origin, step)`` of the corner-aligned anchor grid of OpenPCDet's AnchorGenerator on a feature map of H x W cells:
    the first anchor stands on the low edge of ``point_range`` (x_lo, y_lo, z_lo, x_hi, y_hi, z_hi), the last on the high
    edge, so step = (hi - lo) / (n - 1), computed in double and rounded to float32 once; 0 for a single cell."""
    lo_x, lo_y, hi_x, hi_y = (float(point_range[i]) for i in (0, 1, 3, 4))
    if H < 1 or W < 1:
        raise ValueError(f"anchor_grid: need H, W >= 1 (got {H}, {W})")
    sx = (hi_x - lo_x) / (W - 1) if W > 1 else 0.0
    sy = (hi_y - lo_y) / (H - 1) if H > 1 else 0.0
    return (ops._f32(lo_x), ops._f32(lo_y)), (ops._f32(sx), ops._f32(sy))


def _predict(boxes, scores, labels, iou_thr, score_thr, pre_max, post_max, class_aware):
    keep, order, count = ops.nms_boxes(boxes, scores, labels if class_aware else None, iou_thr, score_thr, pre_max, post_max)
    return boxes, scores, labels, order, count


class AnchorHeadDecoder(nn.Module):
    """Decode configuration of an anchor head.  ``sizes`` [ns,3] (l,w,h), ``z_center`` [ns] (the anchors' centre heights:
    OpenPCDet's ``anchor_bottom_heights + h / 2``), ``rotations`` [nr]; ``origin`` / ``step`` from ``anchor_grid``."""

    def __init__(self, sizes, z_center, rotations, origin, step, dir_offset: float = 0.78539, dir_limit_offset: float = 0.0,
                 layout: str = "nchw"):
        super().__init__()
        self.sizes, self.z_center, self.rotations = ops._anchor_arrays(sizes, z_center, rotations)
        self.origin, self.step = (float(origin[0]), float(origin[1])), (float(step[0]), float(step[1]))
        self.dir_offset, self.dir_limit_offset, self.layout = float(dir_offset), float(dir_limit_offset), layout

    @property
    def num_anchors(self) -> int:
        return self.sizes.shape[0] * self.rotations.shape[0]

    def forward(self, cls: torch.Tensor, reg: torch.Tensor, dir: Optional[torch.Tensor] = None,
                index: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        return ops.anchor_decode(cls, reg, dir, sizes=self.sizes, z_center=self.z_center, rotations=self.rotations,
                                 origin=self.origin, step=self.step, dir_offset=self.dir_offset,
                                 dir_limit_offset=self.dir_limit_offset, layout=self.layout, index=index)

    def assigner(self, pos_thr, neg_thr, size_class=None, nb: int = 0) -> "AnchorTargetAssigner":
        """The target assigner on this decoder's anchors."""
        return AnchorTargetAssigner(self.sizes, self.z_center, self.rotations, self.origin, self.step, pos_thr, neg_thr, size_class,
                                    nb=nb, dir_offset=self.dir_offset)

    def loss(self, **cfg) -> "AnchorHeadLoss":
        """The loss module in this decoder's layout (keywords of ``AnchorHeadLoss``)."""
        return AnchorHeadLoss(layout=self.layout, **cfg)

    def predict(self, cls: torch.Tensor, reg: torch.Tensor, dir: Optional[torch.Tensor] = None, *, iou_thr: float,
                score_thr: float = 0.0, pre_max: Optional[int] = None, post_max: Optional[int] = None, class_aware: bool = True):
        """(boxes [B,K,7], scores, labels, order [B,P], count [B]): the decode, then ``ops.nms_boxes`` on its three tensors.
        ``order[b, :count[b]]`` are the kept rows of scene b, best first.  No synchronisation."""
        return _predict(*self.forward(cls, reg, dir), iou_thr, score_thr, pre_max, post_max, class_aware)


class CenterHeadDecoder(nn.Module):
    """Decode configuration of one task of a centre head.  ``origin`` = (x_lo, y_lo) of the point range, ``cell`` =
    ``out_stride * voxel_size`` in x and y."""

    def __init__(self, origin, cell, log_dim: bool = True, peak: bool = False, layout: str = "nchw"):
        super().__init__()
        self.origin, self.cell = (float(origin[0]), float(origin[1])), (float(cell[0]), float(cell[1]))
        self.log_dim, self.peak, self.layout = bool(log_dim), bool(peak), layout

    def forward(self, hm, reg, height, dim, rot, vel=None, index: Optional[torch.Tensor] = None):
        return ops.center_decode(hm, reg, height, dim, rot, vel, origin=self.origin, cell=self.cell, log_dim=self.log_dim,
                                 peak=self.peak, layout=self.layout, index=index)

    def assigner(self, C: int, min_overlap: float = 0.1, min_radius: int = 2, vel: bool = False) -> "CenterTargetAssigner":
        """The target assigner on this decoder's map geometry (C classes of the task)."""
        return CenterTargetAssigner(C, self.origin, self.cell, min_overlap, min_radius, vel, self.layout)

    def loss(self, **cfg) -> "CenterHeadLoss":
        """The loss module in this decoder's layout (keywords of ``CenterHeadLoss``)."""
        return CenterHeadLoss(layout=self.layout, **cfg)

    def predict(self, hm, reg, height, dim, rot, vel=None, *, iou_thr: float, score_thr: float = 0.0,
                pre_max: Optional[int] = None, post_max: Optional[int] = None, class_aware: bool = True):
        """(boxes [B,K,D], scores, labels, order [B,P], count [B]) as ``AnchorHeadDecoder.predict``."""
        return _predict(*self.forward(hm, reg, height, dim, rot, vel), iou_thr, score_thr, pre_max, post_max, class_aware)


class AnchorTargetAssigner(nn.Module):
    """Target assignment of an anchor head (``ops.anchor_targets``): the anchor fields of ``AnchorHeadDecoder`` plus
    ``pos_thr`` / ``neg_thr`` (a scalar or one per size) and ``size_class`` (the class each size is matched against; ``None``:
    class-agnostic).  ``nb`` >= 2 adds the direction-bin target."""

    def __init__(self, sizes, z_center, rotations, origin, step, pos_thr, neg_thr, size_class=None, nb: int = 0,
                 dir_offset: float = 0.78539):
        super().__init__()
        self.sizes, self.z_center, self.rotations = ops._anchor_arrays(sizes, z_center, rotations)
        self.origin, self.step = (float(origin[0]), float(origin[1])), (float(step[0]), float(step[1]))
        self.pos_thr, self.neg_thr, self.size_class = pos_thr, neg_thr, size_class
        self.nb, self.dir_offset = int(nb), float(dir_offset)

    @property
    def num_anchors(self) -> int:
        return self.sizes.shape[0] * self.rotations.shape[0]

    def forward(self, gt_boxes: torch.Tensor, gt_labels: torch.Tensor, H: int, W: int, out: Optional[tuple] = None) -> tuple:
        """(labels, match, reg_target, max_iou[, dir_target]) for a feature map of H x W cells."""
        return ops.anchor_targets(gt_boxes, gt_labels, H=H, W=W, sizes=self.sizes, z_center=self.z_center, rotations=self.rotations,
                                  origin=self.origin, step=self.step, pos_thr=self.pos_thr, neg_thr=self.neg_thr,
                                  size_class=self.size_class, nb=self.nb, dir_offset=self.dir_offset, out=out)


class CenterTargetAssigner(nn.Module):
    """Target assignment of one task of a centre head (``ops.center_targets``): ``origin`` / ``cell`` / ``layout`` as
    ``CenterHeadDecoder``, ``C`` classes."""

    def __init__(self, C: int, origin, cell, min_overlap: float = 0.1, min_radius: int = 2, vel: bool = False, layout: str = "nchw"):
        super().__init__()
        self.C = int(C)
        self.origin, self.cell = (float(origin[0]), float(origin[1])), (float(cell[0]), float(cell[1]))
        self.min_overlap, self.min_radius, self.vel, self.layout = float(min_overlap), int(min_radius), bool(vel), layout

    def forward(self, gt_boxes: torch.Tensor, gt_labels: torch.Tensor, H: int, W: int, out: Optional[tuple] = None):
        """(heatmap, ind, anno) for a map of H x W cells."""
        return ops.center_targets(gt_boxes, gt_labels, C=self.C, H=H, W=W, origin=self.origin, cell=self.cell,
                                  min_overlap=self.min_overlap, min_radius=self.min_radius, vel=self.vel, layout=self.layout, out=out)


class AnchorHeadLoss(nn.Module):
    """Losses of an anchor head (``ops.anchor_head_loss``, SPEC.md §27.1): the configuration only, no parameters.
    ``forward(cls, reg, dir, labels, reg_target, dir_target) -> loss [B,3]`` (classification, regression, direction), each
    already divided by the scene's positive count, differentiable in the maps.  The operator's second output is not returned:
    the module keeps ``num_pos`` [B] int32 of its LAST call as an attribute (``None`` before the first), for logging."""

    def __init__(self, alpha: float = 0.25, beta: float = 1.0 / 9.0, code_weights=None, sin_diff: bool = True, scale=(1.0, 1.0, 1.0),
                 normalize: bool = True, layout: str = "nchw"):
        super().__init__()
        self.cfg = dict(alpha=float(alpha), beta=float(beta), code_weights=None if code_weights is None else [float(v) for v in code_weights],
                        sin_diff=bool(sin_diff), scale=tuple(float(v) for v in scale), normalize=bool(normalize), layout=layout)
        self.num_pos = None

    def forward(self, cls: torch.Tensor, reg: torch.Tensor, dir: Optional[torch.Tensor], labels: torch.Tensor, reg_target: torch.Tensor,
                dir_target: Optional[torch.Tensor] = None) -> torch.Tensor:
        from .autograd import AnchorHeadLoss as _Fn
        loss, self.num_pos = _Fn.apply(cls, reg, dir, labels, reg_target, dir_target, self.cfg)
        return loss


class CenterHeadLoss(nn.Module):
    """Losses of one task of a centre head (``ops.center_head_loss``, SPEC.md §27.2).
    ``forward(hm, reg, height, dim, rot, vel, heatmap, ind, anno) -> loss [B,2]`` (heat map, regression), differentiable in the
    maps.  ``num_pos`` [B,2] int32 of the LAST call is kept as an attribute (``None`` before the first)."""

    def __init__(self, code_weights=None, scale=(1.0, 1.0), normalize: bool = True, layout: str = "nchw"):
        super().__init__()
        self.cfg = dict(code_weights=None if code_weights is None else [float(v) for v in code_weights],
                        scale=tuple(float(v) for v in scale), normalize=bool(normalize), layout=layout)
        self.num_pos = None

    def forward(self, hm, reg, height, dim, rot, vel, heatmap, ind, anno) -> torch.Tensor:
        from .autograd import CenterHeadLoss as _Fn
        loss, self.num_pos = _Fn.apply(hm, reg, height, dim, rot, vel, heatmap, ind, anno, self.cfg)
        return loss
