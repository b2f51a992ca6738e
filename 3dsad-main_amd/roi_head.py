"""RoI head (SPEC.md §28, §29): which of the ``ops.nms_boxes`` survivors a second stage (PV-RCNN, Voxel R-CNN, Part-A2, PointRCNN)
trains on, their matched ground truth in the RoI's frame with the residual code, the decode of that code at inference, and
the loss on those targets.  ``ProposalTargetLayer`` holds the sampling configuration only and has no parameters; the pooling
and the head's layers are the caller's.  No gradients pass through it: its outputs are targets.  ``RoIHeadLoss`` is the loss
of the head's two predictions against them, differentiable in the predictions; ``RoIIoULoss`` (SPEC.md §34) is the rotated
IoU / DIoU loss of the box residuals against the same targets."""
from collections import namedtuple
from typing import Optional

import torch
from torch import nn

from . import io as _io
from . import ops

RoiTargets = namedtuple("RoiTargets", ops.ROI_OUTPUTS)


class ProposalTargetLayer(nn.Module):
    """The sampler of the replaced code bases' ``ProposalTargetLayer`` on ``ops.roi_targets``, under their configuration names:
    ``roi_per_image`` slots per scene, at most ``round(fg_ratio * roi_per_image)`` of them foreground; a RoI is foreground from
    an IoU of ``min(reg_fg_thresh, cls_fg_thresh)``, hard background from ``cls_bg_thresh_lo`` up to there, easy background
    below; ``hard_bg_ratio`` of the background slots draw from the hard ones.  ``cls_score_type`` "roi_iou" gives the soft
    classification target between ``cls_bg_thresh`` and ``cls_fg_thresh``, "cls" the hard one with the band ignored (-1).
    ``by_class``: match a RoI against the ground truth of its predicted class only.  Every call mixes a step counter into
    ``seed``, so successive steps sample differently and a run is reproducible from (seed, step)."""

    def __init__(self, roi_per_image: int = 128, fg_ratio: float = 0.5, reg_fg_thresh: float = 0.55, cls_fg_thresh: float = 0.75,
                 cls_bg_thresh: float = 0.25, cls_bg_thresh_lo: float = 0.1, hard_bg_ratio: float = 0.8,
                 cls_score_type: str = "roi_iou", by_class: bool = True, seed: int = 0):
        super().__init__()
        self.roi_per_image, self.fg_max = int(roi_per_image), int(round(float(fg_ratio) * int(roi_per_image)))
        self.reg_fg_thresh, self.cls_fg_thresh, self.cls_bg_thresh = float(reg_fg_thresh), float(cls_fg_thresh), float(cls_bg_thresh)
        self.cls_bg_thresh_lo, self.hard_bg_ratio = float(cls_bg_thresh_lo), float(hard_bg_ratio)
        self.cls_score_type, self.by_class, self.seed = cls_score_type, bool(by_class), int(seed)
        self.step = 0

    def call_seed(self, step: int) -> int:
        """The seed of call number ``step``: SPEC.md §17's hash of (the layer's seed, the step) — the same integer mix the
        kernel then applies to (that seed, scene, row)."""
        return int(_io._h(self.seed, step, 0))

    def forward(self, rois: torch.Tensor, roi_labels: Optional[torch.Tensor], gt_boxes: torch.Tensor, gt_labels: torch.Tensor,
                roi_count: Optional[torch.Tensor] = None, out: Optional[tuple] = None) -> RoiTargets:
        """rois [B,R,D], roi_labels [B,R] int32 (read only with ``by_class``), padded ground truth -> ``RoiTargets``; advances
        the step counter."""
        seed = self.call_seed(self.step)
        self.step += 1
        return RoiTargets(*ops.roi_targets(
            rois, roi_count, roi_labels if self.by_class else None, gt_boxes, gt_labels, S=self.roi_per_image, fg_max=self.fg_max,
            fg_thr=min(self.reg_fg_thresh, self.cls_fg_thresh), bg_lo=self.cls_bg_thresh_lo, hard_ratio=self.hard_bg_ratio,
            reg_fg_thr=self.reg_fg_thresh, cls_fg_thr=self.cls_fg_thresh, cls_bg_thr=self.cls_bg_thresh,
            cls_mode=self.cls_score_type, seed=seed, out=out))

    def decode(self, rois: torch.Tensor, reg: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """``ops.roi_decode``: the head's residuals on their RoIs -> boxes [B,S,7]."""
        return ops.roi_decode(rois, reg, out)

    def loss(self, **cfg) -> "RoIHeadLoss":
        """The loss module on this layer's targets: ``RoIHeadLoss(**cfg)``."""
        return RoIHeadLoss(**cfg)

    def iou_loss(self, **cfg) -> "RoIIoULoss":
        """The rotated IoU loss on this layer's targets: ``RoIIoULoss(**cfg)``."""
        return RoIIoULoss(**cfg)


class RoIHeadLoss(nn.Module):
    """Losses of a RoI head (``ops.roi_head_loss``, SPEC.md §29): the configuration only, no parameters.  ``cls_weight``,
    ``reg_weight`` and ``corner_weight`` are the replaced code bases' ``LOSS_WEIGHTS`` (the operator's ``scale``);
    ``corner=False`` leaves the corner loss out.  ``forward(rcnn_cls, rcnn_reg, targets) -> loss [B,3]`` (classification,
    regression, corner), each already divided by the scene's own count, differentiable in the two predictions; ``targets`` is the
    ``RoiTargets`` of ``ProposalTargetLayer``, read where it is.  rcnn_cls may come as [B,S], [B,S,1] or [B*S,1], rcnn_reg as
    [B,S,7] or [B*S,7]: contiguous views, never copied.  The module keeps ``num`` [B,2] int32 = (n_cls, n_reg) of its LAST call
    as an attribute (``None`` before the first), for logging."""

    def __init__(self, beta: float = 1.0 / 9.0, code_weights=None, cls_weight: float = 1.0, reg_weight: float = 1.0,
                 corner_weight: float = 1.0, corner: bool = True, normalize: bool = True):
        super().__init__()
        self.cfg = dict(beta=float(beta), code_weights=None if code_weights is None else [float(v) for v in code_weights],
                        scale=(float(cls_weight), float(reg_weight), float(corner_weight)), normalize=bool(normalize))
        self.corner = bool(corner)
        self.num = None

    def forward(self, rcnn_cls: torch.Tensor, rcnn_reg: torch.Tensor, targets: RoiTargets) -> torch.Tensor:
        from .autograd import RoIHeadLoss as _Fn
        B, S = targets.cls_target.shape
        if rcnn_cls.numel() != B * S or rcnn_reg.numel() != B * S * 7 or not rcnn_cls.is_contiguous() or not rcnn_reg.is_contiguous():
            raise ValueError(f"rcnn_cls / rcnn_reg: expected contiguous predictions for {B} x {S} RoIs ([B,S], [B,S,1] or [B*S,1]; "
                             f"[B,S,7] or [B*S,7]), got {tuple(rcnn_cls.shape)} and {tuple(rcnn_reg.shape)}")
        rois, gt_local = (targets.rois_s, targets.gt_local) if self.corner else (None, None)
        loss, self.num = _Fn.apply(rcnn_cls.view(B, S), rcnn_reg.view(B, S, 7), targets.cls_target, targets.reg_valid,
                                   targets.reg_target, rois, gt_local, self.cfg)
        return loss


class RoIIoULoss(nn.Module):
    """Rotated IoU loss of a RoI head's box residuals (``ops.rotated_iou_loss`` with ``code="roi"``, SPEC.md §34): the
    configuration only, no parameters.  ``forward(rcnn_reg, targets) -> loss [B]``: ``1 - IoU`` (``kind="diou"``: plus the
    centre-distance term) of the box decoded in the RoI's frame against ``targets.gt_local``, over the rows with
    ``reg_valid != 0``, summed per scene and divided by ``max(n_reg, 1)`` (``normalize=False``: not divided), differentiable in
    ``rcnn_reg``, which may come as [B,S,7] or [B*S,7]: a contiguous view, never copied.  ``targets`` is the ``RoiTargets`` of
    ``ProposalTargetLayer``, read where it is.  The module keeps the call's detached ``iou`` [B,S] (of every row, valid or
    not) as its attribute ``iou`` until the next call: the target of an IoU-prediction branch."""

    def __init__(self, mode: str = "3d", kind: str = "iou", normalize: bool = True):
        super().__init__()
        self.cfg = dict(mode=mode, kind=kind, code="roi")
        self.normalize = bool(normalize)
        self.iou = None

    def forward(self, rcnn_reg: torch.Tensor, targets: RoiTargets) -> torch.Tensor:
        from .autograd import RotatedIoULoss as _Fn
        B, S = targets.reg_valid.shape
        if rcnn_reg.numel() != B * S * 7 or rcnn_reg.shape[-1] != 7 or not rcnn_reg.is_contiguous():
            raise ValueError(f"rcnn_reg: expected contiguous predictions for {B} x {S} RoIs ([B,S,7] or [B*S,7]), got {tuple(rcnn_reg.shape)}")
        valid = targets.reg_valid != 0
        loss, self.iou = _Fn.apply(rcnn_reg.view(B, S, 7), targets.gt_local, valid.to(torch.float32), targets.rois_s, self.cfg)
        loss = loss.sum(1)
        return loss / valid.sum(1).clamp(min=1).to(torch.float32) if self.normalize else loss
