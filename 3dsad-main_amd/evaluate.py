"""Detection evaluation (SPEC.md §36): average precision accumulated on the device.  ``DetectionEval`` holds the matching
configuration and preallocated row buffers; ``update`` matches a batch (``ops.det_match``) and appends its rows at an offset the
host knows, without reading anything back, so it can run inside a training or validation loop; ``compute`` runs ``ops.det_ap``
over what was accumulated and is the one place that synchronises.  The matching rule is the score-ordered greedy one of
nuScenes, Waymo and COCO, not KITTI's ground-truth-first rule; difficulty levels are expressed through ``gt_ignore``."""
from typing import Optional

import numpy as np
import torch

from . import ops

PRESETS = {"kitti_r40": (40, 1, 0.0), "kitti_r11": (10, 0, 0.0), "nuscenes": (100, 11, 0.1)}      # (points, first, floor)


class DetectionEval:
    """AP of ``num_classes`` classes at the thresholds ``thr`` ([C,T], [T] for every class, or one number) under ``metric``
    (``"iou3d"``, ``"iou_bev"``, ``"dist"``), sampled at recall k / ``points`` for k = ``first`` .. ``points`` with the precision
    floor ``floor`` (``PRESETS``).  ``capacity`` is the number of detection rows (scenes x K, dead rows included) the buffers
    hold; they are allocated by the first ``update`` on the device of its tensors."""

    def __init__(self, num_classes: int, thr, metric: str = "iou3d", points: int = 40, first: int = 1, floor: float = 0.0,
                 capacity: int = 1 << 20):
        C = int(num_classes)
        if not 1 <= C <= 64:
            raise ValueError(f"num_classes: expected 1 .. 64, got {num_classes}")
        t = np.asarray(thr, np.float32)
        if t.ndim == 0:
            t = t.reshape(1)
        if t.ndim == 1:
            t = np.broadcast_to(t[None], (C, t.shape[0]))
        if t.ndim != 2 or t.shape[0] != C or not 1 <= t.shape[1] <= 8:
            raise ValueError(f"thr: expected [C,T] with C = {C} and 1 <= T <= 8 ([T] or a number for every class), got {t.shape}")
        if metric not in ("iou3d", "iou_bev", "dist"):
            raise ValueError(f"metric: expected 'iou3d', 'iou_bev' or 'dist', got {metric!r}")
        points, first, floor = int(points), int(first), float(np.float32(floor))
        if not 1 <= points <= 128 or not 0 <= first <= points or not 0.0 <= floor < 1.0:
            raise ValueError(f"points, first, floor: need 1 <= points <= 128, 0 <= first <= points and 0 <= floor < 1 "
                             f"(got {points}, {first}, {floor})")
        if int(capacity) < 1 or int(capacity) * t.shape[1] >= 1 << 31:
            raise ValueError(f"capacity: expected 1 <= capacity and capacity * T < 2^31, got {capacity}")
        self.C, self.T, self.thr_host = C, t.shape[1], np.array(t, np.float32, order="C")
        self.metric, self.points, self.first, self.floor, self.capacity = metric, points, first, floor, int(capacity)
        self.rows = 0
        self.thr = self.scores = self.labels = self.code = self.n_gt = None

    def _allocate(self, dev) -> None:
        self.thr = torch.from_numpy(self.thr_host).to(dev)
        self.scores = torch.empty(self.capacity, dtype=torch.float32, device=dev)
        self.labels = torch.empty(self.capacity, dtype=torch.int32, device=dev)
        self.code = torch.empty((self.capacity, self.T), dtype=torch.int32, device=dev)
        self.n_gt = torch.zeros(self.C, dtype=torch.int32, device=dev)

    def _room(self, n: int) -> None:
        if self.rows + n > self.capacity:
            raise RuntimeError(f"DetectionEval: capacity {self.capacity} exceeded ({self.rows} rows held, {n} more)")

    def reset(self) -> None:
        """Forget every row and count; the buffers stay."""
        self.rows = 0
        if self.n_gt is not None:
            self.n_gt.zero_()

    def update(self, det_boxes: torch.Tensor, det_scores: torch.Tensor, det_labels: torch.Tensor, det_count: Optional[torch.Tensor],
               gt_boxes: torch.Tensor, gt_labels: torch.Tensor, gt_ignore: Optional[torch.Tensor] = None):
        """``ops.det_match``'s arguments (without ``thr``): matches the batch and appends its B*K rows, scene-major, dead rows
        included (code -1); adds the batch's ground-truth counts.  Returns (match, value, gt_det) of the batch.  No
        synchronisation; ``RuntimeError`` when ``capacity`` would be exceeded."""
        if not isinstance(det_boxes, torch.Tensor) or det_boxes.dim() != 3:
            raise ValueError("det_boxes: expected [B,K,D]")
        B, K = det_boxes.shape[:2]
        n = B * K
        self._room(n)
        if self.scores is None:
            if not det_boxes.is_cuda:
                raise RuntimeError("det_boxes: expected a GPU tensor (sad_amd has no CPU path)")
            self._allocate(det_boxes.device)
        G = gt_boxes.shape[1] if isinstance(gt_boxes, torch.Tensor) and gt_boxes.dim() == 3 else 0
        dev, i32 = self.scores.device, torch.int32
        code = self.code[self.rows:self.rows + n].view(B, K, self.T)
        out = (code, torch.empty((B, K, self.T), dtype=i32, device=dev), torch.empty((B, K, self.T), dtype=torch.float32, device=dev),
               torch.empty((B, G, self.T), dtype=i32, device=dev), torch.empty((B, self.C), dtype=i32, device=dev))
        _, match, value, gt_det, n_gt = ops.det_match(det_boxes, det_scores, det_labels, det_count, gt_boxes, gt_labels, gt_ignore,
                                                      self.thr, metric=self.metric, out=out)
        ops.copy_rows(det_scores, 0, n, 1, n, self.scores[self.rows:self.rows + n])
        ops.copy_rows(det_labels, 0, n, 1, n, self.labels[self.rows:self.rows + n])
        self.n_gt += n_gt.sum(0, dtype=i32)
        self.rows += n
        return match, value, gt_det

    def merge(self, other: "DetectionEval") -> None:
        """Append the rows of ``other`` (an evaluator of the same configuration that saw other scenes, e.g. another rank's
        shard, on this device) behind this one's and add its counts."""
        same = (self.C == other.C and self.T == other.T and self.metric == other.metric and np.array_equal(self.thr_host, other.thr_host)
                and (self.points, self.first, self.floor) == (other.points, other.first, other.floor))
        if not same:
            raise ValueError("merge: the two evaluators differ in configuration")
        n = other.rows
        self._room(n)
        if n == 0:
            return
        if self.scores is None:
            self._allocate(other.scores.device)
        if other.scores.device != self.scores.device:
            raise ValueError("merge: the two evaluators live on different devices")
        ops.copy_rows(other.scores, 0, n, 1, n, self.scores[self.rows:self.rows + n])
        ops.copy_rows(other.labels, 0, n, 1, n, self.labels[self.rows:self.rows + n])
        ops.copy_rows(other.code, 0, n * self.T, 1, n * self.T, self.code[self.rows:self.rows + n])
        self.n_gt += other.n_gt
        self.rows += n

    def compute(self) -> dict:
        """{"ap" [C,T], "prec" [C,T,points-first+1], "max_recall" [C,T], "n_det" [C,T], "n_gt" [C], "mean_ap" [T]} as numpy
        arrays; ``mean_ap`` is the mean over the classes with ground truth (ap >= 0), NaN when there is none.  The one
        synchronisation of the evaluator."""
        if self.scores is None:
            raise RuntimeError("DetectionEval.compute: nothing was accumulated")
        n = self.rows
        ap, prec, max_recall, n_det = ops.det_ap(self.scores[:n], self.labels[:n], self.code[:n], self.n_gt, points=self.points,
                                                 first=self.first, floor=self.floor)
        res = {"ap": ap.cpu().numpy(), "prec": prec.cpu().numpy(), "max_recall": max_recall.cpu().numpy(), "n_det": n_det.cpu().numpy(),
               "n_gt": self.n_gt.cpu().numpy()}
        valid = res["ap"] >= 0
        cnt = valid.sum(0)
        with np.errstate(invalid="ignore", divide="ignore"):
            res["mean_ap"] = (np.where(valid, res["ap"], np.float32(0)).sum(0, dtype=np.float64) / cnt).astype(np.float32)
        return res
