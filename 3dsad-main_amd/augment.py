"""Training augmentation on the device (SPEC.md §35): the ground-truth database and its sampler (``ops.gt_paste``), the global
flip / rotation / scale / translation (``ops.global_augment``) and ``TrainAugment``, which chains paste (with the transform fused
into its stores) and ``subsample_pad`` into the batch ``SADDetectorTrain`` and the target assigners take.  Everything after the
database's construction runs without a synchronisation and is reproducible from (seed, step)."""
import json
import os
from typing import Optional, Sequence

import numpy as np
import torch

from . import io as _io
from . import ops


class GTDatabase:
    """Objects cut from labelled scenes, resident on the device: ``db_points [sum P,Cp]``, ``db_offsets [Ndb+1]``, ``db_boxes
    [Ndb,D]`` and the host list ``class_offsets [C+1]``; entries are sorted by class (stable), so a class is an index range.
    ``objects``: a list of (points [n,Cp], box [D], label).  An object of more than ``max_obj_points`` rows is subsampled
    systematically (``io.select_rows``); ``Pmax`` is the longest object kept.  Difficulty and min-points filters are the
    caller's, before the list is handed over."""

    def __init__(self, objects: Sequence[tuple], num_classes: int, max_obj_points: int = 2048, device=None, seed: int = 0):
        C = int(num_classes)
        if not 1 <= C <= 16:
            raise ValueError(f"num_classes: expected 1 .. 16, got {num_classes}")
        if not objects:
            raise ValueError("GTDatabase: no objects")
        if int(max_obj_points) < 1:
            raise ValueError("max_obj_points must be >= 1")
        order = sorted(range(len(objects)), key=lambda i: int(objects[i][2]))
        pts, boxes, labels = [], [], []
        for k, i in enumerate(order):
            p, bx, lab = objects[i]
            p = np.ascontiguousarray(p, np.float32)
            bx = np.asarray(bx, np.float32).reshape(-1)
            if not 0 <= int(lab) < C:
                raise ValueError(f"object {i}: label {lab} outside [0, {C})")
            if p.ndim != 2 or p.shape[1] < 3 or (pts and p.shape[1] != pts[0].shape[1]):
                raise ValueError(f"object {i}: expected points [n,Cp] with the same Cp >= 3 for every object, got {p.shape}")
            if bx.shape[0] < 7 or (boxes and bx.shape[0] != boxes[0].shape[0]):
                raise ValueError(f"object {i}: expected a box row of the same D >= 7 columns for every object, got {bx.shape[0]}")
            if p.shape[0] > max_obj_points:
                p = np.ascontiguousarray(p[_io.select_rows(p.shape[0], int(max_obj_points), seed, k)])
            pts.append(p)
            boxes.append(bx)
            labels.append(int(lab))
        self.num_classes, self.max_obj_points = C, int(max_obj_points)
        self.points = np.concatenate(pts).reshape(-1, pts[0].shape[1])
        self.offsets = np.concatenate([[0], np.cumsum([p.shape[0] for p in pts])]).astype(np.int32)
        self.boxes = np.stack(boxes)
        self.labels = np.asarray(labels, np.int32)
        self.class_offsets = [int((self.labels < c).sum()) for c in range(C + 1)]
        self.Pmax = int(max(p.shape[0] for p in pts))
        self.db_points = self.db_offsets = self.db_boxes = None
        if device is not None:
            self.to(device)

    def __len__(self) -> int:
        return self.boxes.shape[0]

    def to(self, device) -> "GTDatabase":
        self.db_points = torch.from_numpy(self.points).to(device)
        self.db_offsets = torch.from_numpy(self.offsets).to(device)
        self.db_boxes = torch.from_numpy(self.boxes).to(device)
        return self

    @classmethod
    def from_scenes(cls, points, offsets, gt_boxes, gt_labels, num_classes: int, device, max_obj_points: int = 2048, seed: int = 0):
        """Cuts the objects out of labelled scenes with ``ops.points_in_boxes`` (a point belongs to the lowest box that holds
        it): host arrays points [total,Cp], offsets [B+1], gt_boxes [B,G,D], gt_labels [B,G]; padding rows are skipped."""
        points, offsets = np.ascontiguousarray(points, np.float32), np.asarray(offsets, np.int64)
        gt_boxes, gt_labels = np.ascontiguousarray(gt_boxes, np.float32), np.asarray(gt_labels, np.int64)
        objects = []
        for b in range(gt_boxes.shape[0]):
            scene = points[offsets[b]:offsets[b + 1]]
            valid = (gt_labels[b] >= 0) & (gt_labels[b] < num_classes) & (gt_boxes[b, :, 3:6] > 0).all(1)
            if not scene.shape[0] or not valid.any():
                continue
            idx = ops.points_in_boxes(torch.from_numpy(np.ascontiguousarray(scene[None, :, :3])).to(device),
                                      torch.from_numpy(gt_boxes[b:b + 1]).to(device))[0].cpu().numpy()
            objects += [(scene[idx == g], gt_boxes[b, g], int(gt_labels[b, g])) for g in np.flatnonzero(valid)]
        return cls(objects, num_classes, max_obj_points, device, seed)

    @classmethod
    def from_directory(cls, root: str, infos, num_classes: int, cols: int = 4, device=None, max_obj_points: int = 2048, seed: int = 0):
        """Per-object ``.bin`` files (float32 rows of ``cols`` columns, already in the scene's frame) plus an info list: ``infos``
        is a list of {"path", "box", "label"} or the name of a JSON file holding one; paths are relative to ``root``."""
        if isinstance(infos, str):
            with open(infos if os.path.isabs(infos) else os.path.join(root, infos)) as f:
                infos = json.load(f)
        return cls([(_io.read_bin(os.path.join(root, i["path"]), cols), i["box"], i["label"]) for i in infos], num_classes,
                   max_obj_points, device, seed)


class GTSampler:
    """``ops.gt_paste`` on a ``GTDatabase``: ``sample_num[c]`` = the count class c is filled up to (OpenPCDet's
    ``SAMPLE_GROUPS``), ``remove_extra_width`` widens the pasted boxes when scene points are removed."""

    def __init__(self, db: GTDatabase, sample_num: Sequence[int], remove_extra_width: float = 0.0, seed: int = 0):
        if db.db_points is None:
            raise ValueError("GTSampler: the database is not on a device (GTDatabase.to)")
        if len(sample_num) != db.num_classes:
            raise ValueError(f"sample_num: expected one count per class ({db.num_classes}), got {len(sample_num)}")
        self.db, self.sample_num, self.remove_extra_width, self.seed = db, [int(v) for v in sample_num], float(remove_extra_width), int(seed)
        self.Q = sum(self.sample_num)
        self.step = 0

    def rows(self, total: int, B: int) -> int:
        return ops.gt_paste_rows(total, B, self.Q, self.db.Pmax)

    def __call__(self, points, offsets, gt_boxes, gt_labels, params=None, with_velocity: bool = False, step: Optional[int] = None,
                 out: Optional[tuple] = None, workspace: Optional[torch.Tensor] = None) -> tuple:
        """-> ``ops.gt_paste``'s outputs; without ``step`` the sampler's own counter is used and advanced."""
        if step is None:
            step, self.step = self.step, self.step + 1
        db = self.db
        return ops.gt_paste(points, offsets, gt_boxes, gt_labels, db.db_points, db.db_offsets, db.db_boxes, db.class_offsets,
                            sample_num=self.sample_num, max_obj_points=db.Pmax, seed=self.seed, step=step,
                            remove_extra_width=self.remove_extra_width, params=params, with_velocity=with_velocity, out=out,
                            workspace=workspace)


class GlobalAugment:
    """``ops.global_augment`` under OpenPCDet's names: ``random_world_flip`` along x and / or y, ``random_world_rotation``,
    ``random_world_scaling`` and a uniform ``random_world_translation``."""

    def __init__(self, flip_x: bool = True, flip_y: bool = False, rot_range=(-0.78539816, 0.78539816), scale_range=(0.95, 1.05),
                 translate_range=(0.0, 0.0, 0.0), with_velocity: bool = False, seed: int = 0):
        self.cfg = dict(flip_x=bool(flip_x), flip_y=bool(flip_y), rot_range=tuple(rot_range), scale_range=tuple(scale_range),
                        translate_range=tuple(translate_range))
        self.with_velocity, self.seed, self.step = bool(with_velocity), int(seed), 0

    def _step(self, step: Optional[int]) -> int:
        if step is None:
            step, self.step = self.step, self.step + 1
        return step

    def params(self, B: int, device, step: Optional[int] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """params [B,8] of a step alone (what ``gt_paste(params=...)`` fuses): the launch on an empty batch."""
        pts = torch.empty((B, 0, 3), dtype=torch.float32, device=device)
        box = torch.empty((B, 0, 7), dtype=torch.float32, device=device)
        outs = None if out is None else (pts, box, out)
        return ops.global_augment(pts, None, box, seed=self.seed, step=self._step(step), out=outs, **self.cfg)[2]

    def __call__(self, points, offsets, gt_boxes, step: Optional[int] = None, out: Optional[tuple] = None) -> tuple:
        """-> (points_out, boxes_out, params)."""
        return ops.global_augment(points, offsets, gt_boxes, seed=self.seed, step=self._step(step), with_velocity=self.with_velocity,
                                  out=out, **self.cfg)


class TrainAugment:
    """A labelled ragged batch -> the training step's inputs: paste (``sampler``) with ``global_aug``'s transform fused into its
    stores, then ``subsample_pad`` to ``n_points`` rows per scene.  Returns (points [B,n_points,Cp], gt_boxes [B,G+Q,D],
    gt_labels [B,G+Q]) in the form ``SADDetectorTrain.targets`` and the dense-head assigners take.  Owns and reuses its buffers
    (the results of a call are overwritten by the next) and carries the step counter that enters every seed."""

    def __init__(self, sampler: GTSampler, global_aug: Optional[GlobalAugment], n_points: int, seed: int = 0):
        self.sampler, self.global_aug, self.n_points, self.seed, self.step = sampler, global_aug, int(n_points), int(seed), 0
        self._key, self._out, self._ws, self._params, self._padded = None, None, None, None, None

    def _buffers(self, total: int, B: int, G: int, D: int, Cp: int, dev):
        Q, need = self.sampler.Q, self.sampler.rows(total, B)
        key = (B, G, D, Cp, dev)
        if key != self._key or self._out[5].shape[0] < need:
            spec = ops.gt_paste_output_spec(B, G, D, Q, Cp, need)
            self._out = tuple(torch.empty(shape, dtype=dt, device=dev) for _, shape, dt in spec)
            self._params = torch.empty((B, 8), dtype=torch.float32, device=dev)
            self._padded = torch.empty((B, self.n_points, Cp), dtype=torch.float32, device=dev)
            self._key, self._ws = key, None
        nbytes = ops.lib().sad_gt_paste_workspace_bytes(B, Q, total)
        if self._ws is None or self._ws.numel() < nbytes:
            self._ws = ops.gt_paste_workspace(B, Q, total, dev)

    def __call__(self, points: torch.Tensor, offsets: torch.Tensor, gt_boxes: torch.Tensor, gt_labels: torch.Tensor,
                 step: Optional[int] = None) -> tuple:
        if step is None:
            step, self.step = self.step, self.step + 1
        B, G, D = gt_boxes.shape
        self._buffers(points.shape[0], B, G, D, points.shape[1], points.device)
        params, vel = None, False
        if self.global_aug is not None:
            params, vel = self.global_aug.params(B, points.device, step, self._params), self.global_aug.with_velocity
        outs = self.sampler(points, offsets, gt_boxes, gt_labels, params=params, with_velocity=vel, step=step, out=self._out,
                            workspace=self._ws)
        padded = ops.subsample_pad(outs[5], outs[6], self.n_points, seed=ops.augment_seed(self.seed, step), out=self._padded)
        return padded, outs[2], outs[3]
