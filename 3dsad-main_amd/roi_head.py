"""RoI head (SPEC.md §28): which of the ``ops.nms_boxes`` survivors a second stage (PV-RCNN, Voxel R-CNN, Part-A2, PointRCNN)
trains on, their matched ground truth in the RoI's frame with the residual code, and the decode of that code at inference.
``ProposalTargetLayer`` holds the sampling configuration only and has no parameters; the pooling and the head's layers are
the caller's.  No gradients pass through it: its outputs are targets."""
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
