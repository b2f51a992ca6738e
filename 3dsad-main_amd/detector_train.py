"""``SADDetectorTrain``: the trainable counterpart of ``SADDetector`` (f32; SPEC.md §33), in ``SAModuleMSGTrain``'s mould.

Built from the same ``DetectorConfig`` and weights dict.  Every chain is a ``SharedMLP`` (fused forward, the backward of §32); the
size-adaptive cluster layer (§8) is differentiable through ``autograd.PrefixRows`` (the first K rows in front of the candidate
MLP) and ``autograd.Candidates`` (the clamped shift).  Sampling and every ball query, the adaptive cluster query included, run
under ``no_grad``: they are index decisions.  Single stream, eager.  Under ``no_grad`` ``decode(forward(points))`` equals
``SADDetector(cfg, export(), device)(points)`` bit for bit, and the training path's forward tensors equal the ``no_grad`` ones:
the model that is trained is the model that is served.
"""
import ctypes
from collections import namedtuple
from typing import Optional

import torch
from torch import nn

from . import autograd, ops
from ._lib import check, lib
from .config import DetectorConfig
from .point_head import PointTargetAssigner, PointTargets
from .sa_module import SAModuleMSGTrain
from .shared_mlp import BranchGroup, SharedMLP
from .synth import make_weights

# o [B,K,C_cls+7] (the head's rows), c [B,K,6] (the candidate layer's rows), cand [B,K,3], xyz_k [B,K,3] (the first K SA3
# centroids), radius [B,K] (not differentiable), feat3 [B,M3,C3] (SA3's features)
TrainOutput = namedtuple("TrainOutput", ("o", "c", "cand", "xyz_k", "radius", "feat3"))


class SADDetectorTrain(nn.Module):
    """``SADDetectorTrain(cfg, device, weights=None, seed=0)``; ``weights=None`` draws ``synth.make_weights(cfg, seed)``.
    Submodules: ``stages`` (one ``SAModuleMSGTrain`` each), ``cand``, ``cluster_branches``, ``cluster_agg``, ``head``
    (``SharedMLP``s; ``cand`` and ``head`` with ReLU on all but the last layer).  Parameters are created with
    ``requires_grad=False``: ``requires_grad_(True)`` on the module or on any submodule selects what is trained."""

    def __init__(self, cfg: DetectorConfig, device, weights: Optional[dict] = None, seed: int = 0):
        super().__init__()
        if weights is None:
            weights = make_weights(cfg, seed)
        self.cfg = cfg
        c = cfg.in_feat
        stages = []
        for si, st in enumerate(cfg.stages):
            w = {f"b{i}": weights[f"sa{si + 1}.b{i}"] for i in range(len(st.mlps))}
            if st.agg:
                w["agg"] = weights[f"sa{si + 1}.agg"]
            stages.append(SAModuleMSGTrain(c, st, "cpu", w, name=f"sa{si + 1}"))
            c = stages[-1].out_channels
        self.stages = nn.ModuleList(stages)
        self.cand = SharedMLP([c] + list(cfg.cand_mlp), False, relu_mask=(1 << (len(cfg.cand_mlp) - 1)) - 1,
                              layers=weights["cand"], name="cand")
        self.cluster_branches = BranchGroup(SharedMLP([c + 3] + list(m), True, layers=weights[f"cluster.b{i}"], name=f"cluster.b{i}")
                                            for i, m in enumerate(cfg.cluster_mlps))
        self.cluster_agg = SharedMLP([self.cluster_branches.cat_channels, cfg.cluster_agg], False, layers=weights["cluster.agg"],
                                     name="cluster.agg")
        self.head = SharedMLP([cfg.cluster_agg] + list(cfg.head_mlp), False, relu_mask=(1 << (len(cfg.head_mlp) - 1)) - 1,
                              layers=weights["head"], name="head")
        self.assigner = PointTargetAssigner.from_config(cfg)
        self.num_pos = None                # num_pos [B] int32 of the last loss() call
        self._anchors = (ctypes.c_float * 9)(*[v for a in cfg.anchors for v in a])
        self.to(torch.device(device))

    def cluster_head(self, xyz3: torch.Tensor, feat3: torch.Tensor) -> TrainOutput:
        """SPEC.md §8 and §9 on SA3's output: xyz3 [B,M3,3], feat3 [B,M3,C3] -> ``TrainOutput``.  Gradients reach the parameters
        of ``cand``, the cluster branches, ``cluster_agg`` and ``head``, and feat3 (the branches' gathered rows plus the padded
        prefix behind the candidate MLP); ``cand`` receives gradient only from the branches' relative coordinates, and passes it
        to c[..., 0:3] where the shift was not clamped (§33.1)."""
        cfg = self.cfg
        M3, K = xyz3.shape[1], cfg.n_cand
        with torch.no_grad():
            xyz_k = xyz3 if K == M3 else ops.prefix_rows(xyz3, K)
        c = self.cand.rows(autograd.PrefixRows.apply(feat3, K))                                    # [B,K,6]
        cand, radius = autograd.Candidates.apply(xyz3, c, K, cfg.shift_max, cfg.r_min, cfg.r_max, cfg.anchor_car)
        with torch.no_grad():
            idxs, cnts = ops.ball_query_multi(cfg.cluster_scales, cfg.cluster_nsamples, xyz3, cand.detach(), radius,
                                              return_counts=True)
        cat = self.cluster_branches(xyz3, feat3, cand, idxs, cnts)
        o = self.head.rows(self.cluster_agg.rows(cat))                                             # [B,K,C_cls+7]
        return TrainOutput(o, c, cand, xyz_k, radius, feat3)

    def forward(self, points: torch.Tensor) -> TrainOutput:
        """points [B,N,3+in_feat] f32 on the GPU -> ``TrainOutput``.  The centroids are the ones ``SADDetector`` takes: stage 1
        samples, the later stages take the prefix of the stage before (SPEC.md §2)."""
        if not points.is_cuda:
            raise RuntimeError("points: expected a GPU tensor (sad_amd has no CPU path)")
        if points.dtype != torch.float32 or points.dim() != 3:
            raise TypeError("points: expected a float32 [B,N,3+C] tensor")
        with torch.no_grad():
            xyz, feat = ops.split_points(points.contiguous())
        cur_xyz, cur_feat = xyz, feat
        for m in self.stages:
            new_xyz = None
            if cur_xyz is not xyz and m.stage.npoint <= cur_xyz.shape[1]:
                with torch.no_grad():
                    new_xyz = ops.prefix_rows(cur_xyz, m.stage.npoint)
            cur_xyz, cur_feat = m.forward_pm(cur_xyz, cur_feat, new_xyz)
        return self.cluster_head(cur_xyz, cur_feat)

    @torch.no_grad()
    def decode(self, out: TrainOutput) -> torch.Tensor:
        """boxes [B,K,9] of an output (SPEC.md §9, ``sad_decode_boxes_f32``): what ``SADDetector`` returns."""
        B, K = out.o.shape[:2]
        if out.o.shape[2] != 10:
            raise ValueError("decode: the box decode takes 3 class logits + 7 box values per row")
        o, cand = out.o.detach().contiguous(), out.cand.detach().contiguous()
        boxes = torch.empty((B, K, 9), dtype=torch.float32, device=o.device)
        check(lib().sad_decode_boxes_f32(cand.data_ptr(), o.data_ptr(), B, K, self._anchors, boxes.data_ptr(), ops._stream()),
              "sad_decode_boxes_f32")
        return boxes

    def targets(self, out: TrainOutput, gt_boxes: torch.Tensor, gt_labels: torch.Tensor) -> PointTargets:
        """The ``PointTargets`` of an output (SPEC.md §31.1): assigned at ``xyz_k``, regression targets taken at ``cand`` as a
        constant (3DSSD's rule: no gradient reaches ``cand`` through a target)."""
        return self.assigner(out.xyz_k, out.cand.detach(), gt_boxes, gt_labels)

    def loss(self, out: TrainOutput, targets: PointTargets, **weights) -> torch.Tensor:
        """loss [B,4] (classification, box regression, shift, size; SPEC.md §31.2) through ``point_head.PointHeadLoss``;
        ``weights``: that module's keywords (``cls_weight=...``).  ``num_pos`` of the call is kept in ``self.num_pos``."""
        fn = self.assigner.loss(**weights)
        res = fn(out.o, out.c, targets)
        self.num_pos = fn.num_pos
        return res

    def export(self) -> dict:
        """The weights dict ``SADDetector`` takes: name -> [(W, b), ...] as numpy arrays (``config.mlp_layers`` names)."""
        w = {}
        for si, m in enumerate(self.stages):
            for k, v in m.export().items():
                w[f"sa{si + 1}.{k}"] = v
        w["cand"] = self.cand.export()
        for i, mlp in enumerate(self.cluster_branches):
            w[f"cluster.b{i}"] = mlp.export()
        w["cluster.agg"] = self.cluster_agg.export()
        w["head"] = self.head.export()
        return w
