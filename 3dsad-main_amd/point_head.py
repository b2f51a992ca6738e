"""Point head training modules (SPEC.md §31): the target assigner and the loss of the size-adaptive cluster layer (§8) and the
box / class head (§9), or of any point-wise head with the same rows (3DSSD / IA-SSD candidate heads, a per-point head).
The point-path counterpart of ``dense_head.AnchorTargetAssigner`` / ``AnchorHeadLoss`` and ``roi_head.ProposalTargetLayer`` /
``RoIHeadLoss``: configuration only, no parameters; the work is ``ops.point_targets`` and ``ops.point_head_loss``."""
from collections import namedtuple
from typing import Optional

import torch
from torch import nn

from . import ops

PointTargets = namedtuple("PointTargets", ops.POINT_OUTPUTS)


class PointTargetAssigner(nn.Module):
    """``ops.point_targets`` with its constants: anchors [C,3] (§9's class anchors), size_anchor [3] (§8's ``anchor_car``),
    shift_max (§8 step 2's clamp) and extra_width (the ignored band around a box).  ``forward(xyz, cand, gt_boxes, gt_labels)
    -> PointTargets`` (labels, match, centerness, shift_target, size_target, reg_target); ``cand=None`` for a head that predicts
    from the points themselves.  No gradients."""

    def __init__(self, anchors, size_anchor, shift_max: float, extra_width: float = 0.2):
        super().__init__()
        self.anchors = tuple(tuple(float(v) for v in a) for a in anchors)
        self.size_anchor = tuple(float(v) for v in size_anchor)
        self.shift_max, self.extra_width = float(shift_max), float(extra_width)

    @classmethod
    def from_config(cls, cfg, extra_width: float = 0.2) -> "PointTargetAssigner":
        """§8 / §9's constants of a ``DetectorConfig``."""
        return cls(cfg.anchors, cfg.anchor_car, cfg.shift_max, extra_width)

    @property
    def num_classes(self) -> int:
        return len(self.anchors)

    @torch.no_grad()
    def forward(self, xyz: torch.Tensor, cand: Optional[torch.Tensor], gt_boxes: torch.Tensor, gt_labels: torch.Tensor,
                out: Optional[tuple] = None) -> PointTargets:
        return PointTargets(*ops.point_targets(xyz, cand, gt_boxes, gt_labels, anchors=self.anchors, size_anchor=self.size_anchor,
                                               shift_max=self.shift_max, extra_width=self.extra_width, out=out))

    def loss(self, **cfg) -> "PointHeadLoss":
        """The loss module on this assigner's targets: ``PointHeadLoss(shift_max=self.shift_max, **cfg)``."""
        return PointHeadLoss(shift_max=self.shift_max, **cfg)


class PointHeadLoss(nn.Module):
    """Losses of a point head (``ops.point_head_loss``, SPEC.md §31.2): the configuration only, no parameters.  ``cls_weight``,
    ``reg_weight``, ``shift_weight`` and ``size_weight`` are the operator's ``scale``; ``centerness=False`` trains the class
    channel against 1 instead of the centre-ness.  ``forward(o, c, targets) -> loss [B,4]`` (classification, box regression,
    shift, size), each already divided by the scene's own positive count, differentiable in o and c; ``targets`` is the
    ``PointTargets`` of ``PointTargetAssigner``, read where it is; ``c=None`` leaves the shift and size components out
    (``loss[:, 2:] = 0``).  o may come as [B,M,C+7] or [B*M,C+7] and c as [B,M,6] or [B*M,6]: contiguous views, never copied.
    The module keeps ``num_pos`` [B] int32 of its LAST call as an attribute (``None`` before the first), for logging."""

    def __init__(self, shift_max: Optional[float] = None, cls_loss: str = "bce", alpha: float = 0.25, beta: float = 1.0 / 9.0,
                 code_weights=None, cls_weight: float = 1.0, reg_weight: float = 1.0, shift_weight: float = 1.0,
                 size_weight: float = 1.0, centerness: bool = True, normalize: bool = True):
        super().__init__()
        self.cfg = dict(cls_loss=str(cls_loss), alpha=float(alpha), beta=float(beta),
                        code_weights=None if code_weights is None else [float(v) for v in code_weights],
                        shift_max=None if shift_max is None else float(shift_max),
                        scale=(float(cls_weight), float(reg_weight), float(shift_weight), float(size_weight)), normalize=bool(normalize))
        self.centerness = bool(centerness)
        self.num_pos = None

    def forward(self, o: torch.Tensor, c: Optional[torch.Tensor], targets: PointTargets) -> torch.Tensor:
        from .autograd import PointHeadLoss as _Fn
        B, M = targets.labels.shape
        if o.dim() not in (2, 3) or o.numel() % (B * M) or not o.is_contiguous():
            raise ValueError(f"o: expected contiguous rows for {B} x {M} points ([B,M,C+7] or [B*M,C+7]), got {tuple(o.shape)}")
        if c is not None and (c.numel() != B * M * 6 or not c.is_contiguous()):
            raise ValueError(f"c: expected contiguous rows for {B} x {M} points ([B,M,6] or [B*M,6]), got {tuple(c.shape)}")
        if c is not None and self.cfg["shift_max"] is None:
            raise ValueError("shift_max: the module was built without it and cannot take c")
        shift, size = (targets.shift_target, targets.size_target) if c is not None else (None, None)
        loss, self.num_pos = _Fn.apply(o.view(B, M, -1), None if c is None else c.view(B, M, 6), targets.labels,
                                       targets.centerness if self.centerness else None, targets.reg_target, shift, size, self.cfg)
        return loss
