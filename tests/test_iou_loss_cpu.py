"""CPU checks of the rotated IoU loss (SPEC.md §34): the float32 reference (tests/iou_loss_ref.py) against box_ref's IoU and
against the binary64 truth with central differences (tests/iou_loss_truth.py).  No GPU."""
import functools

import numpy as np
import pytest

import box_ref
import box_truth as bt
import iou_loss_ref as ref
import iou_loss_truth as truth
import roi_head_ref

F = np.float32
SIZES = sorted(bt.SIZE_FAMILIES)
ONE_SIDED = ("identical", "edge", "yaw_step")
N_TRUTH = 600


@pytest.fixture(autouse=True)
def _oracle(orc):
    return orc


def _diagonal(a, b, mode):
    """box_ref.boxes_iou(a, b, mode)[i, i] without the matrix: every pair as a scene of its own."""
    return box_ref.boxes_iou(a[:, None, :], b[:, None, :], mode)[:, 0, 0]


# ---- 1: the value ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("family", bt.PAIR_FAMILIES)
def test_iou_is_the_diagonal_of_boxes_iou(family, size):
    a, b = bt.pair_family(family, size, 257, seed=2)
    for mode in ref.MODES:
        want = _diagonal(a, b, mode)
        for kind in ref.KINDS:
            loss, iou, grad, _ = ref.rotated_iou_loss(a, b, None, mode, kind)
            np.testing.assert_array_equal(iou, want, err_msg=f"{family} {size} {mode} {kind}")
            assert np.isfinite(loss).all() and np.isfinite(grad).all()
            if kind == "iou":
                np.testing.assert_array_equal(loss, F(1) - want)
    if family == "far":
        assert (want == 0).all()


@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("family", ONE_SIDED)
def test_one_sided_families_stay_finite(family, size):
    """identical, edge, yaw_step: an edge of pred lies on (or within rounding of) an edge of target, the derivative is one-sided or
    ill-conditioned and is not compared with a truth; value and gradient stay finite and the value is box_ref's."""
    a, b = bt.pair_family(family, size, 600, seed=1)
    for mode in ref.MODES:
        want = _diagonal(a, b, mode)
        for kind in ref.KINDS:
            loss, iou, grad, _ = ref.rotated_iou_loss(a, b, None, mode, kind)
            assert np.isfinite(loss).all() and np.isfinite(iou).all() and np.isfinite(grad).all(), f"{family} {size} {mode} {kind}"
            np.testing.assert_array_equal(iou, want)


# ---- 2, 3: the gradient against central differences of the binary64 loss ----------------------------------------------
@functools.lru_cache(maxsize=None)
def _against_truth(kind, mode):
    """{(family, size): (kept fraction, ill-conditioned fraction of the kept, max err / gscale over the rest, max |loss err| / tol)}."""
    out = {}
    for size in SIZES:
        for family in truth.TRUTH_FAMILIES:
            a, b = bt.pair_family(family, size, N_TRUTH, seed=1)
            keep = truth.well_conditioned(family, a, b)
            a, b = a[keep], b[keep]
            loss, iou, grad, _ = ref.rotated_iou_loss(a, b, None, mode, kind)
            l64, g64, ill = truth.grad64(a, b, mode, kind)
            err = np.abs(grad.astype(np.float64) - g64) / truth.gscale(a, b)
            lerr = np.abs(loss.astype(np.float64) - l64) / (bt.tol(a, b) + 2.0 ** -20)
            if family == "far":
                assert (iou == 0).all() and (loss >= 1).all()
                if kind == "iou":
                    assert (grad == 0).all() and (loss == 1).all()
            out[family, size] = (float(keep.mean()), float(ill.mean()), float(err[~ill].max()), float(lerr.max()))
    return out


@pytest.mark.parametrize("mode", ref.MODES)
@pytest.mark.parametrize("kind", ref.KINDS)
def test_gradient_against_the_truth(kind, mode):
    for (family, size), (kept, ill, g, lerr) in _against_truth(kind, mode).items():
        print(f"{kind} {mode} {family:9s} {size:6s}: kept {kept:.3f}, ill-conditioned {ill:.4f}, max gradient err / gscale {g:.3f}, "
              f"max loss err / tol {lerr:.3f}")
        assert kept >= 0.70, f"{family} {size}: only {kept:.3f} of the pairs are well-conditioned"
        assert ill < 0.01, f"{family} {size}: {ill:.4f} of the kept pairs are ill-conditioned by the h against h / 2 rule"
        assert g <= truth.G_TOL, f"{family} {size}: gradient error {g:.3f} x gscale"
        assert lerr <= 1.0, f"{family} {size}: loss error {lerr:.3f} x (tol + 2^-20)"


def test_gradient_tolerance_constant():
    """G_MEASURED of tests/iou_loss_truth.py is the measured constant: printed here, and a reference that drifted above G_TOL / 2
    fails."""
    worst = max(v[2] for kind in ref.KINDS for mode in ref.MODES for v in _against_truth(kind, mode).values())
    print(f"largest err / gscale of the float32 reference: {worst:.3f} (G_MEASURED = {truth.G_MEASURED}, G_TOL = {truth.G_TOL})")
    assert worst <= truth.G_TOL / 2
    assert truth.G_TOL == 4.0 * truth.G_MEASURED


def test_the_truth_moves_its_rows_in_binary64():
    """The truth's IoU is box_truth's on float32 rows, and it resolves a step of 1e-9 m that float32 rows cannot hold."""
    a, b = bt.pair_family("perturbed", "object", 32, seed=3)
    for mode, fn in (("bev", bt.iou_bev64), ("3d", bt.iou3d64)):
        got = np.array([truth.iou64(p, t, mode) for p, t in zip(a.astype(np.float64).tolist(), b.astype(np.float64).tolist())])
        np.testing.assert_allclose(got, fn(a, b), rtol=0, atol=1e-14)
    p, t = a[0].astype(np.float64).tolist(), b[0].astype(np.float64).tolist()
    q = list(p)
    q[0] += 1e-9
    assert truth.iou64(q, t, "bev") != truth.iou64(p, t, "bev")


# ---- weights ----------------------------------------------------------------------------------------------------------
def test_weights_select():
    a, b = bt.pair_family("perturbed", "object", 64, seed=4)
    l1, i1, g1, _ = ref.rotated_iou_loss(a, b, None, "3d", "diou")
    l2, i2, g2, _ = ref.rotated_iou_loss(a, b, np.ones(64, F), "3d", "diou")
    for x, y in ((l1, l2), (i1, i2), (g1, g2)):
        np.testing.assert_array_equal(x.view(np.int32), y.view(np.int32))
    wt = np.where(np.arange(64) % 3 == 0, 0, np.linspace(0.5, 2, 64)).astype(F)
    an, bn = a.copy(), b.copy()
    an[::6], bn[3::6] = np.nan, np.nan
    l3, i3, g3, _ = ref.rotated_iou_loss(an, bn, wt, "3d", "diou")
    off = wt == 0
    assert (l3[off].view(np.int32) == 0).all() and (g3[off].view(np.int32) == 0).all()
    np.testing.assert_array_equal(l3[~off], l1[~off] * wt[~off])
    np.testing.assert_array_equal(g3[~off], g1[~off] * wt[~off, None])


# ---- 4: code = roi ----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def roi_rows():
    """Rows of roi_head_ref's targets on box_truth.roi_scene: (rcnn_reg, gt_local, rois_s, valid as f32), [B*S, 7] each, and seeded
    residuals near the regression target."""
    B, R, G, S = 2, 96, 8, 48
    sc = [bt.roi_scene(R, G, s) for s in range(B)]
    c = dict(rois=np.stack([x[0] for x in sc]), roi_count=None, roi_labels=None, gt_boxes=np.stack([x[1] for x in sc]),
             gt_labels=np.zeros((B, G), np.int32), kw=dict(roi_head_ref.DEFAULTS, S=S, fg_max=S // 2, seed=5))
    tg = roi_head_ref.roi_targets_vec(c)
    valid = tg["reg_valid"].reshape(-1) != 0
    assert 8 <= valid.sum() < B * S
    rng = np.random.default_rng(6)
    reg = np.where(valid[:, None], tg["reg_target"].reshape(-1, 7), 0).astype(F) + rng.normal(0, 0.05, (B * S, 7)).astype(F)
    return reg, tg["gt_local"].reshape(-1, 7).astype(F), tg["rois_s"].reshape(-1, 7).astype(F), valid.astype(F)


@pytest.mark.parametrize("mode", ref.MODES)
@pytest.mark.parametrize("kind", ref.KINDS)
def test_roi_code(kind, mode):
    reg, gt_local, rois, wt = roi_rows()
    loss, iou, grad, dec = ref.rotated_iou_loss(reg, gt_local, wt, mode, kind, "roi", rois)
    np.testing.assert_array_equal(dec, ref.decode(reg, rois))
    lb, ib, gb, _ = ref.rotated_iou_loss(dec, gt_local, wt, mode, kind)
    np.testing.assert_array_equal(loss, lb)
    np.testing.assert_array_equal(iou, ib)
    la, wa, ha, dg = ref.roi_anchor(rois)
    jac = np.stack([dg, dg, ha, dec[:, 3], dec[:, 4], dec[:, 5], np.ones_like(dg)], 1)
    on = wt != 0
    np.testing.assert_array_equal(grad[on], (gb * jac)[on])
    assert (grad[~on].view(np.int32) == 0).all() and (loss[~on].view(np.int32) == 0).all()
    assert (iou[on] > 0.3).all(), "the valid rows are foreground: the decoded box overlaps its ground truth"
    assert np.abs(grad[on]).max() > 0
    # the value against the truth, on the decoded box
    l64 = np.array([truth.loss64(p, t, mode, kind) for p, t in zip(dec[on].astype(np.float64).tolist(), gt_local[on].astype(np.float64).tolist())])
    assert (np.abs(loss[on] - l64) <= bt.tol(dec[on], gt_local[on]) + 2.0 ** -20).all()
    # a RoI with D = 9 columns and a second copy of the call are the same bits
    wide = np.concatenate([rois, np.full((rois.shape[0], 2), np.nan, F)], 1)
    again = ref.rotated_iou_loss(reg, gt_local, wt, mode, kind, "roi", wide)
    for x, y in zip((loss, iou, grad, dec), again):
        np.testing.assert_array_equal(x.view(np.int32), y.view(np.int32))
