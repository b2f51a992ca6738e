"""The RoI head loss reference (tests/roi_loss_ref.py, SPEC.md §29) checked against itself and against the replaced code's
global-frame form, without a GPU: the float32 loop and whole-array forms agree bit for bit; the binary64 evaluation of the
RoI-frame formulas and of the hand-derived gradient agrees with torch autograd through decode + boxes_to_corners_3d + min +
Huber; the cases cover what tests/test_gpu_roi_loss.py relies on; no tolerance-checked row sits within the margin of the
flip or of the Huber kink; and float32 rounding uses at most a tenth of the GPU test's tolerance."""
import numpy as np
import pytest

import roi_loss_ref as ref

F = np.float32
D = np.float64
GRADS = ("grad_cls", "grad_reg", "grad_corner")


@pytest.mark.parametrize("name", ref.CASES)
def test_loop_and_vec_agree_bit_for_bit(orc, name):
    c = ref.case(name)
    loop, vec = ref.loss_loop(c), ref.expected(name)["f32"]
    assert ("grad_corner" in loop) == ("grad_corner" in vec) == (c["rois"] is not None)
    for k, v in loop.items():
        assert v.dtype == vec[k].dtype and v.shape == vec[k].shape, k
        assert not np.isnan(v).any(), f"{name}: NaN in {k}"
        assert np.array_equal(v.view(np.int32), vec[k].view(np.int32)), f"{name}: {k} differs between the two forms"


@pytest.mark.parametrize("name", [n for n in ref.CASES if n != "coincident"])      # (torch's norm has no gradient at distance 0)
def test_binary64_against_the_global_frame_composition(name):
    c = ref.case(name)
    want, gx, gr = ref.torch_composition(c)
    e = ref.expected(name)["f64"]
    mine = e["grad_reg"] + e.get("grad_corner", 0.0)
    errs = (np.abs(e["loss64"] - want).max(), np.abs(e["grad_cls"] - gx).max(), np.abs(mine - gr).max())
    print(f"{name}: loss {errs[0]:.3g}, grad_cls {errs[1]:.3g}, grad_reg + grad_corner {errs[2]:.3g}")
    assert max(errs) <= 1e-12, f"{name}: RoI-frame form against the global-frame form: {errs}"


def test_cases_cover_what_the_gpu_test_relies_on():
    shapes = {n: ref.case(n)["rcnn_cls"].shape for n in ref.CASES}
    assert {s[1] for s in shapes.values()} >= {1, 32, 128, 257, 1024} and {s[0] for s in shapes.values()} >= {1, 2, 3}
    nums = np.concatenate([ref.expected(n)["f32"]["num"] for n in ref.CASES])
    assert (nums[:, 1] == 0).any() and (nums[:, 0] == 0).any() and (nums[:, 1] > 0).any()
    assert (ref.case("no_gt")["reg_valid"][0] == 0).all() and (ref.case("no_gt")["cls_target"][0] >= 0).all()          # n_reg = 0, n_cls > 0
    assert (ref.case("ragged")["cls_target"][2] == -1).all()                                                           # empty slots
    assert (ref.case("on_threshold:cls")["cls_target"] == -1).any() and (ref.case("on_threshold:cls")["cls_target"] >= 0).any()
    t = ref.case("both")["cls_target"]
    assert ((t > 0) & (t < 1)).any() and (t == 0).any() and (t == 1).any()                                              # a soft target
    assert ref.case("odd")["rois"].shape[2] == 9 and ref.case("s257")["rois"].shape[2] == 9 and ref.case("both")["rois"].shape[2] == 7
    assert ref.case("both:nocorner")["rois"] is None and "grad_corner" not in ref.expected("both:nocorner")["f32"]
    assert (ref.expected("both:nocorner")["f32"]["per_roi"][..., 2] == 0).all()
    kw = ref.case("both")["kw"]
    assert any(w != 1 for w in kw["code_weights"]) and any(s != 1 for s in kw["scale"]) and ref.case("both:unit")["kw"]["beta"] == 1.0
    flips = quads = lins = below = above = 0
    for n in ref.CASES:
        c, e = ref.case(n), ref.expected(n)["f64"]
        valid = c["reg_valid"] != 0
        # NaN wherever a row is not valid, and none of it in a result
        assert np.isnan(c["reg_target"][~valid]).all()
        for k in ("per_roi",) + GRADS:
            assert k not in e or not np.isnan(e[k]).any(), (n, k)
        with np.errstate(all="ignore"):
            a = np.abs((c["rcnn_reg"].astype(D) - c["reg_target"]) * np.asarray(c["kw"]["code_weights"], F))[valid]
        below, above = below + int((a < F(c["kw"]["beta"])).sum()), above + int((a >= F(c["kw"]["beta"])).sum())
        if c["rois"] is None or n in ref.TIES:
            continue
        assert np.isnan(c["gt_local"][~valid]).all() and np.isnan(c["rois"][~valid]).all()
        d0, d1, dist = (e[k][valid] for k in ("d0", "d1", "dist"))
        flips, quads, lins = flips + int((d1 < d0).sum()), quads + int((dist < 1).sum()), lins + int((dist >= 1).sum())
    assert min(flips, quads, lins, below, above) >= 50, (flips, quads, lins, below, above)
    assert (ref.expected("both")["f64"]["d1"] < ref.expected("both")["f64"]["d0"]).any() and (ref.expected("both")["f64"]["dist"] < 1).any()


@pytest.mark.parametrize("name", [n for n in ref.CASES if ref.case(n)["rois"] is not None])
def test_no_row_within_the_margin_of_a_discontinuity(name):
    flip, kink = ref.margins(ref.case(name))
    assert (kink >= ref.MARGIN).all(), f"{name}: {int((kink < ref.MARGIN).sum())} rows within {ref.MARGIN} of dist = 1"
    if name in ref.TIES:
        assert (flip[ref.case(name)["reg_valid"] != 0] == 0).all()               # d0 == d1 exactly, in binary64 too
    else:
        assert (flip >= ref.MARGIN).all(), f"{name}: {int((flip < ref.MARGIN).sum())} rows within {ref.MARGIN} of d0 = d1"


def test_the_exact_cases():
    c, e = ref.case("coincident"), ref.expected("coincident")["f32"]
    valid = c["reg_valid"] != 0
    assert valid.sum() > 20 and (ref.expected("coincident")["f64"]["dist"][valid] == 0).all()
    assert (e["per_roi"][..., 2] == 0).all() and (e["grad_corner"] == 0).all() and (e["loss"][:, 2] == 0).all()
    assert not any(np.isnan(e[k]).any() for k in ("per_roi", "loss") + GRADS)
    c, e = ref.case("degenerate"), ref.expected("degenerate")["f32"]
    valid = c["reg_valid"] != 0
    assert (c["gt_local"][valid][:, 3:5] == 0).all() and (e["d0"][valid] == e["d1"][valid]).all() and (e["per_roi"][valid][:, 2] > 0).all()
    assert not any(np.isnan(e[k]).any() for k in ("per_roi", "loss") + GRADS)


@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("name", ref.CASES)
def test_float32_rounding_is_a_tenth_of_the_tolerance(name, normalize):
    """What test_gpu_roi_loss.py allows the device (1e-4 + 1e-4 |ref64|; grad_corner: 1e-4 + 1e-4 mag) leaves room for the
    rounding of a float32 evaluation ten times over: it has none for a wrong formula."""
    e32, e64 = ref.expected(name, normalize)["f32"], ref.expected(name, normalize)["f64"]
    assert np.array_equal(e32["num"], e64["num"])
    worst = {}
    for k, scale in (("per_roi", None), ("grad_cls", None), ("grad_reg", None), ("grad_corner", "mag")):
        if k not in e64:
            continue
        share = np.abs(e32[k].astype(D) - e64[k]) / ref.tolerance(e64[k], e64[scale] if scale else None)
        worst[k] = float(share.max())
    print(f"{name} normalize={normalize}: share of the tolerance {worst}")
    assert max(worst.values()) <= 0.1, worst
