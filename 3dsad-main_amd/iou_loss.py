"""Rotated IoU losses (SPEC.md §34): ``RotatedIoULoss`` is the box regression loss ``1 - IoU`` (or DIoU) of aligned pairs of
rotated boxes, differentiable in the prediction through the analytic gradient of ``ops.rotated_iou_loss``.  The configuration
only, no parameters.  The RoI head's form, on residuals and ``roi_targets``' outputs, is ``roi_head.RoIIoULoss``."""
from typing import Optional

import torch
from torch import nn

REDUCTIONS = ("none", "sum", "mean")


class RotatedIoULoss(nn.Module):
    """``forward(pred [...,Dp], target [...,Dt], weight [...] = None) -> loss``: ``weight · (1 - IoU)`` per pair (``kind="diou"``:
    plus the centre-distance term), ``mode`` "bev" or "3d"; ``reduction`` "none" keeps the leading shape, "sum" adds the pairs,
    "mean" divides that by their number.  Box rows (cx,cy,cz,l,w,h,yaw,...) with D >= 7, contiguous f32, read where they are.
    The target is a constant.  The module keeps the call's detached ``iou`` [...] as its attribute ``iou`` until the next call
    (``None`` before the first): the target of an IoU-prediction branch, or a metric."""

    def __init__(self, mode: str = "3d", kind: str = "iou", reduction: str = "none"):
        super().__init__()
        if reduction not in REDUCTIONS:
            raise ValueError(f"reduction: expected one of {REDUCTIONS}, got {reduction!r}")
        self.cfg = dict(mode=mode, kind=kind, code="box")
        self.reduction = reduction
        self.iou = None

    def forward(self, pred: torch.Tensor, target: torch.Tensor, weight: Optional[torch.Tensor] = None) -> torch.Tensor:
        from .autograd import RotatedIoULoss as _Fn
        loss, self.iou = _Fn.apply(pred, target, weight, None, self.cfg)
        if self.reduction == "none":
            return loss
        return loss.sum() if self.reduction == "sum" else loss.sum() / loss.numel()
