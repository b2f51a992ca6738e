"""The rotated-box kernels against the float64 truth of tests/box_truth.py, and exact under translation (-m gpu).

The older GPU tests pin every kernel bit for bit to the CPU oracle / tests/box_ref.py; tests/test_box_truth_cpu.py pins those to
the truth.  Here the kernels meet the truth directly, at offsets (0, 0), (70, -40), (1e5, -1e5) (and (1e6, 1e6) for the IoU
matrices): boxes_iou_bev / boxes_iou3d within tol of the true IoU, nms_bev (both forms) and nms_boxes equal to the greedy NMS
on the truth on scenes where no pair lies within tol of the threshold, roi_targets' match equal to the true argmax; and every
output bit-identical to the same call at offset 0, because all centres lie on a 1/16 m lattice and SPEC §13 clips a pair on the
difference of its centres.  A last case uses KITTI-shaped scenes whose centres are on no lattice.

With the global-frame corners of the earlier §13 the realistic case was 2.6e-5 from the truth, 6.9 x its tol of 3.8e-6 (measured
with that library on the GPU), and the lattice cases failed at every offset (figures in tests/test_box_truth_cpu.py)."""
import functools

import numpy as np
import pytest

import box_ref
import box_truth as bt
import roi_head_ref

pytestmark = pytest.mark.gpu

F = np.float32
GPU_OFFSETS = bt.OFFSETS[:2] + bt.OFFSETS[3:4]                    # (0, 0), (70, -40), (1e5, -1e5)
IOU_OFFSETS = GPU_OFFSETS + bt.OFFSETS[4:5]                       # ... and (1e6, 1e6)
# (B, Ka, Kb, Da, Db): a full tile grid, a partial one, and one past each tile size of boxes.hip (IOU_TA = 8, IOU_TB = 32)
IOU_CASES = [(1, 64, 64, 7, 9), (2, 3, 65, 9, 7), (1, 9, 33, 7, 7)]


def _t(a, dev):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _widen(boxes, D):
    """[...,7] -> [...,D] with NaN in the columns the operators must not read."""
    out = np.full(boxes.shape[:-1] + (D,), np.nan, F)
    out[..., :7] = boxes
    return out


@functools.lru_cache(maxsize=None)
def _iou_inputs():
    """Per case: a [B,Ka,7], b [B,Kb,7] at offset 0, the float32 references and the truths (bev, 3d) with their tol."""
    out = []
    for n, (B, Ka, Kb, Da, Db) in enumerate(IOU_CASES):
        ab = [bt.matrix_boxes(Ka, Kb, 10 * n + s) for s in range(B)]
        a, b = np.stack([x[0] for x in ab]), np.stack([x[1] for x in ab])
        ref = {m: box_ref.boxes_iou(a, b, m) for m in ("bev", "3d")}
        truth = {"bev": np.stack([bt.iou_bev64_matrix(a[s], b[s]) for s in range(B)]),
                 "3d": np.stack([bt.iou3d64_matrix(a[s], b[s]) for s in range(B)])}
        out.append((a, b, ref, truth, bt.tol_matrix(a, b)))
    for m in ("bev", "3d"):
        bt.coverage([c[3][m] for c in out])
    return out


@pytest.mark.parametrize("mode", ["bev", "3d"])
def test_boxes_iou_truth_and_translation(sad, dev, mode):
    from sad_amd import ops
    fn = ops.boxes_iou_bev if mode == "bev" else ops.boxes_iou3d
    for (B, Ka, Kb, Da, Db), (a, b, ref, truth, tol) in zip(IOU_CASES, _iou_inputs()):
        for off in IOU_OFFSETS:
            assert bt.is_exact_translation(a, off) and bt.is_exact_translation(b, off)
            got = fn(_t(_widen(bt.translate(a, off), Da), dev), _t(_widen(bt.translate(b, off), Db), dev)).cpu().numpy()
            err = np.abs(got.astype(np.float64) - truth[mode])
            print(f"{mode} {(B, Ka, Kb)} at {off}: max err {err.max():.3e}, err/tol {np.max(err / tol):.3f}, max IoU {got.max():.8f}")
            np.testing.assert_array_equal(got.view(np.int32), ref[mode].view(np.int32), err_msg=f"reference, {mode} {(B, Ka, Kb)} at {off}")
            assert (err <= tol).all(), f"{mode} {(B, Ka, Kb)} at {off}: {np.max(err - tol):.3e} beyond tol"
            assert (got <= 1 + tol).all()


def test_boxes_iou_realistic_scenes(sad, dev):
    """Two KITTI-shaped scenes (centres up to 70 m, on no lattice) against jittered copies of their boxes."""
    from sad_amd import ops, synth
    rng = np.random.default_rng(5)
    a = np.stack([synth.scene_boxes(s) for s in (0, 1)])
    b = a.copy()
    b[..., 0:3] += rng.uniform(-0.4, 0.4, b[..., 0:3].shape).astype(F)
    b[..., 3:6] *= rng.uniform(0.9, 1.1, b[..., 3:6].shape).astype(F)
    b[..., 6] += rng.uniform(-0.2, 0.2, b[..., 6].shape).astype(F)
    assert np.abs(a[..., 0:2]).max() > 60
    tol = bt.tol_matrix(a, b)
    for mode, fn, f64 in (("bev", ops.boxes_iou_bev, bt.iou_bev64_matrix), ("3d", ops.boxes_iou3d, bt.iou3d64_matrix)):
        want = np.stack([f64(a[s], b[s]) for s in range(2)])
        assert (want > 0.3).sum() >= 40 and (want == 0).mean() > 0.5
        got = fn(_t(a, dev), _t(b, dev)).cpu().numpy()
        err = np.abs(got.astype(np.float64) - want)
        print(f"realistic {mode}: max err {err.max():.3e}, err/tol {np.max(err / tol):.3f}")
        assert (err <= tol).all(), f"{mode}: {err.max():.3e} from the truth, tol {tol.max():.3e}"


# ---- NMS -------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _nms_case(K, thr, labels=False, pre_max=None, post_max=None, B=2):
    """B scenes of clustered boxes, their scores (and labels), and the greedy NMS on the truth; asserts that no pair of ranked
    boxes has a true IoU within tol of the threshold, so every correct float32 implementation decides alike."""
    boxes, scores, lab, keeps, orders = [], [], [], [], []
    for s in range(B):
        bx, sc = bt.nms_scene(K, s)
        lb = np.random.default_rng([7, K, s]).integers(0, 3, K).astype(np.int32) if labels else None
        keep, order, near = bt.nms64(bx, sc, thr, labels=lb, pre_max=pre_max, post_max=post_max)
        assert near == 0, f"K={K} scene {s}: {near} pairs within tol of {thr}"
        assert len(np.unique(sc)) == K
        boxes.append(bx), scores.append(sc), lab.append(lb), keeps.append(keep), orders.append(order)
    return np.stack(boxes), np.stack(scores), (np.stack(lab) if labels else None), np.stack(keeps), orders


def _same_nms(got, keeps, orders, what):
    keep, order, count = (g.cpu().numpy() for g in got)
    for s, want in enumerate(orders):
        assert count[s] == len(want) and order[s, :count[s]].tolist() == want, f"{what}, scene {s}: order differs from the NMS on the truth"
        assert (order[s, count[s]:] == -1).all()
    np.testing.assert_array_equal(keep, keeps, err_msg=what)
    return keep, order, count


@pytest.mark.parametrize("thr", [0.1, 0.5])
@pytest.mark.parametrize("K", [130, 512])
@pytest.mark.parametrize("single", [True, False], ids=["one_kernel", "three_kernels"])
def test_nms_bev_truth_and_translation(sad, dev, single, K, thr):
    from sad_amd import ops
    boxes, scores, _, keeps, orders = _nms_case(K, thr)
    for want in orders:
        assert 0.3 <= 1 - len(want) / K <= 0.7, "30 - 70 % of a scene are suppressed"
    first = None
    for off in GPU_OFFSETS:
        assert bt.is_exact_translation(boxes, off)
        bx = np.zeros(boxes.shape[:2] + (9,), F)
        bx[..., :7], bx[..., 7] = bt.translate(boxes, off), scores
        got = _same_nms(ops.nms_bev(_t(bx, dev), thr, 0.0, single_kernel=single), keeps, orders, f"K={K} thr={thr} at {off}")
        first = first or got
        for g, f in zip(got, first):
            np.testing.assert_array_equal(g, f, err_msg=f"moved by {off}")


# K <= 512: one chunked mask as in nms_bev; 1 500 scored boxes cut to 600: the radix pre-selection and the chip-wide mask
@pytest.mark.parametrize("K,pre_max,post_max", [(400, None, None), (1500, 600, None), (1500, 600, 100)])
@pytest.mark.parametrize("labels", [False, True], ids=["agnostic", "by_class"])
def test_nms_boxes_truth_and_translation(sad, dev, labels, K, pre_max, post_max):
    from sad_amd import ops
    thr = 0.3
    boxes, scores, lab, keeps, orders = _nms_case(K, thr, labels, pre_max, post_max)
    P = min(K, pre_max or K)
    for want in orders:
        print(f"nms_boxes K={K} labels={labels}: {len(want)} of {P} ranked boxes kept")
        assert len(want) <= 0.9 * P, "boxes are suppressed"
        assert post_max is None or len(want) == post_max, "the cap binds"
    first = None
    for off in GPU_OFFSETS:
        got = _same_nms(ops.nms_boxes(_t(_widen(bt.translate(boxes, off), 7), dev), _t(scores, dev), _t(lab, dev), thr, 0.0, pre_max, post_max),
                        keeps, orders, f"K={K} labels={labels} pre={pre_max} post={post_max} at {off}")
        first = first or got
        for g, f in zip(got, first):
            np.testing.assert_array_equal(g, f, err_msg=f"moved by {off}")


# ---- roi_targets -----------------------------------------------------------------------------------------------
ROI_B, ROI_R, ROI_G, ROI_S = 2, 130, 9, 64
ROI_KW = dict(roi_head_ref.DEFAULTS, S=ROI_S, fg_max=32, seed=11)


@functools.lru_cache(maxsize=None)
def _roi_case(with_labels):
    sc = [bt.roi_scene(ROI_R, ROI_G, s) for s in range(ROI_B)]
    rois, gt = np.stack([x[0] for x in sc]), np.stack([x[1] for x in sc])
    gl = np.stack([np.random.default_rng([3, s]).integers(0, 3, ROI_G) for s in range(ROI_B)]).astype(np.int32)
    gl[1, ROI_G - 1] = -1                                                   # a padding row: never eligible
    rl = None
    if with_labels:                                                         # the class of the box a RoI was made from, a tenth of them wrong
        rl = np.stack([gl[s][sc[s][2]] for s in range(ROI_B)]).astype(np.int32)
        rl = np.where(rl < 0, 0, rl).astype(np.int32)
        wrong = np.random.default_rng(4).random(rl.shape) < 0.1
        rl[wrong] = (rl[wrong] + 1) % 3
    return dict(rois=rois, roi_count=None, roi_labels=rl, gt_boxes=gt, gt_labels=gl, kw=ROI_KW)


@pytest.mark.parametrize("with_labels", [True, False], ids=["roi_labels", "any_class"])
def test_roi_targets_truth_and_translation(sad, dev, with_labels):
    from sad_amd import ops
    c = _roi_case(with_labels)
    first = None
    for off in GPU_OFFSETS:
        assert bt.is_exact_translation(c["rois"], off) and bt.is_exact_translation(c["gt_boxes"], off)
        rois, gt = bt.translate(c["rois"], off), bt.translate(c["gt_boxes"], off)
        got = ops.roi_targets(_t(rois, dev), None, _t(c["roi_labels"], dev), _t(gt, dev), _t(c["gt_labels"], dev), **c["kw"])
        got = {n: g.cpu().numpy() for n, g in zip(roi_head_ref.OUTPUTS, got)}
        got["rois_s"][..., 0] -= F(off[0])                                   # back to offset 0 (exact on the lattice);
        got["rois_s"][..., 1] -= F(off[1])                                   # gt_local and reg_target are RoI-relative
        if first is None:
            first = got
            want = roi_head_ref.roi_targets_vec(c)
            for n in ("index", "match", "labels", "iou", "cls_target", "reg_valid", "rois_s", "gt_local"):
                np.testing.assert_array_equal(got[n], want[n], err_msg=f"{n} against the float32 reference")
        for n in roi_head_ref.OUTPUTS:
            np.testing.assert_array_equal(got[n].view(np.int32), first[n].view(np.int32), err_msg=f"{n} moved by {off}")
        # against the truth: the IoU of every sampled RoI with its matched box, and the match itself
        qualify = total = 0
        for s in range(ROI_B):
            for i in range(ROI_S):
                roi, j = rois[s, got["index"][s, i]], got["match"][s, i]
                elig = c["gt_labels"][s] >= 0
                if with_labels:
                    elig = elig & (c["gt_labels"][s] == c["roi_labels"][s, got["index"][s, i]])
                total += 1
                if not elig.any():
                    assert j == -1
                    continue
                g = np.flatnonzero(elig)
                true = bt.iou3d64(np.repeat(roi[None], len(g), 0), gt[s, g])
                tol = bt.tol(np.repeat(roi[None], len(g), 0), gt[s, g])
                assert abs(float(got["iou"][s, i]) - true[g.tolist().index(j)]) <= tol[g.tolist().index(j)], f"iou of slot {(s, i)} at {off}"
                top = np.sort(true)[::-1]
                if len(g) == 1 or top[0] - top[1] > tol.max():
                    qualify += 1
                    assert j == g[np.argmax(true)], f"match of slot {(s, i)} at {off}"
        print(f"roi_targets at {off}: {qualify} of {total} slots have a clear best box")
        assert qualify >= 0.9 * total
