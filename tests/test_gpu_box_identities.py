"""Device-against-device identities of the box kernels (-m gpu): what the operators promise one another, checked directly, without
a reference in between.  roi_targets' matching IoU is boxes_iou3d's value (§28.1 on §19.3: roi_match_kernel calls the helpers of
csrc/box_geom.h, boxes_iou_kernel keeps the same operations written out, so this test is what holds the two together); the
RoI-frame decode of rotated_iou_loss (§34, code="roi") is roi_decode's (§28.2), expf included (both call roi_decode_local)."""
import numpy as np
import pytest

import roi_head_ref as ref

pytestmark = pytest.mark.gpu

F = np.float32


def _t(a, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _bits(t):
    return t.cpu().numpy().view(np.int32)


def test_matching_iou_is_boxes_iou3d(dev):
    """B = 2, R = 17 (two workgroups of 16 RoIs), G = 5, S = 32, any class: every RoI stands near a box, so every slot is matched."""
    import torch
    from sad_amd import ops
    B, R, G = 2, 17, 5
    rng = np.random.default_rng(2817)
    rois, gts, labs = np.zeros((B, R, 7), F), np.zeros((B, G, 8), F), np.zeros((B, G), np.int32)
    for b in range(B):
        gt, lab = ref._gt(rng, G)
        gts[b], labs[b] = gt, lab
        rois[b], _ = ref._rois_near(rng, gt, lab, ["fg"] * R)
    assert (labs >= 0).all()
    rois_d, gt_d = _t(rois, dev), _t(gts, dev)
    out = dict(zip(ref.OUTPUTS, ops.roi_targets(rois_d, None, None, gt_d, _t(labs, dev), **dict(ref.DEFAULTS, S=32))))
    index, match = out["index"].long(), out["match"].long()
    assert index.shape == (B, 32) and (match >= 0).all() and (index >= 0).all()
    full = ops.boxes_iou3d(rois_d, gt_d)                                  # [B,R,G]
    want = full[torch.arange(B, device=full.device)[:, None], index, match]
    assert bool((want > 0).all())                                          # (every slot an overlapping pair, none zero against zero)
    np.testing.assert_array_equal(_bits(out["iou"]), _bits(want))


def test_roi_frame_decode_is_one_decode(dev):
    """B = 1, S = 257 (past a workgroup of 256), size residuals in +-1: columns 3..5 are expf(t) times the RoI's clamped extents."""
    from sad_amd import ops
    S = 257
    rng = np.random.default_rng(2834)
    gt, _ = ref._gt(rng, S)
    rois = gt[None, :, :7].astype(F)
    reg = rng.uniform(-1.0, 1.0, (1, S, 7)).astype(F)
    gt_local = np.concatenate([rng.uniform(-1, 1, (1, S, 3)), rng.uniform(0.5, 4.0, (1, S, 3)), rng.uniform(-1.5, 1.5, (1, S, 1))], -1).astype(F)
    rois_d, reg_d = _t(rois, dev), _t(reg, dev)
    boxes = ops.roi_decode(rois_d, reg_d)
    dec = ops.rotated_iou_loss(reg_d, _t(gt_local, dev), code="roi", rois=rois_d, decoded=True)[-1]
    assert dec.shape == boxes.shape == (1, S, 7)
    assert np.isfinite(boxes.cpu().numpy()).all()
    np.testing.assert_array_equal(_bits(dec[..., 3:6]), _bits(boxes[..., 3:6]))
