"""The reference of SPEC.md §28 against itself (no GPU): tests/roi_head_ref.py's loop and array forms agree bit for bit, and every
named case reaches the branch it is named for, so that tests/test_gpu_roi_head.py compares the kernels on ground that is known
to be covered: the class counts of each case, pairs whose IoU equals a threshold exactly, a hard quota above the hard count,
class sizes that are no powers of two in every kind of draw, picks inside their classes, the round trip through the decoder
and the range of the heading."""
import numpy as np
import pytest

import roi_head_ref as ref

F = np.float32


def _plans(name):
    return ref.expected(name)["plans"]


def _n(plan):
    return len(plan["fg"]), len(plan["hard"]), len(plan["easy"])


@pytest.mark.parametrize("name", ref.CASES)
def test_loop_and_array_forms_agree(name):
    c = ref.case(name)
    vec, loop = ref.expected(name), ref.roi_targets_loop(c, ref.iou_of(name))
    for k in ref.OUTPUTS + ("m", "j"):
        assert vec[k].dtype == loop[k].dtype and vec[k].shape == loop[k].shape, k
        assert np.array_equal(vec[k].view(np.int32), loop[k].view(np.int32)), f"{name}: {k} differs between the forms"
    S = c["kw"]["S"]
    B = c["rois"].shape[0]
    for k in ref.OUTPUTS:
        assert vec[k].shape[:2] == (B, S) and not np.isnan(vec[k].astype(np.float64)).any(), k


def test_cases_reach_their_branches():
    kw = lambda name: ref.case(name)["kw"]                                                       # noqa: E731
    assert all(p["ranked"] and _n(p)[0] > kw("both")["fg_max"] and _n(p)[1] and _n(p)[2] for p in _plans("both"))
    assert all(p["ranked"] and 0 < _n(p)[0] < kw("few_fg")["fg_max"] and p["nf"] == _n(p)[0] for p in _plans("few_fg"))
    assert all(_n(p)[0] and not _n(p)[1] and not _n(p)[2] and p["nf"] == kw("fg_only")["S"] for p in _plans("fg_only"))
    assert all(not _n(p)[0] and _n(p)[1] and _n(p)[2] and p["nf"] == 0 for p in _plans("bg_only"))
    assert all(_n(p)[1] and not _n(p)[2] and p["nh"] == p["nb"] for p in _plans("hard_only"))
    assert [bool(_n(p)[0]) for p in _plans("hard_only")] == [True, False]
    assert all(not _n(p)[1] and _n(p)[2] and p["nh"] == 0 for p in _plans("easy_only"))
    assert [bool(_n(p)[0]) for p in _plans("easy_only")] == [True, False]
    # no ground truth: every candidate is unmatched and easy; the normal scene next to the all-padding one is not
    e = ref.expected("no_gt")
    assert (e["j"][0] == -1).all() and (e["m"][0] == 0).all() and _n(e["plans"][0])[:2] == (0, 0) and _n(e["plans"][1])[0] > 0
    assert (e["labels"][0] == -1).all() and (e["reg_valid"][0] == 0).all() and not e["reg_target"][0].any() and (e["cls_target"][0] == 0).all()
    e = ref.expected("no_gt:g0")
    assert ref.case("no_gt:g0")["gt_boxes"].shape[1] == 0 and (e["match"] == -1).all() and (e["index"] >= 0).all()
    # ragged: R, 1 and 0 candidates, NaN beyond; the empty scene's slots are the empty slot
    c, e = ref.case("ragged"), ref.expected("ragged")
    assert list(c["roi_count"]) == [c["rois"].shape[1], 1, 0] and np.isnan(c["rois"][1, 1:]).all() and np.isnan(c["rois"][2]).all()
    assert (e["index"][1] == 0).all() and (e["index"][2] == -1).all() and (e["cls_target"][2] == -1).all() and not e["rois_s"][2].any()
    assert (e["index"][0] < c["roi_count"][0]).all()
    # by_class: some RoI's best box over ALL boxes has another class than the RoI, and is therefore not its match
    c, e = ref.case("by_class"), ref.expected("by_class")
    other = 0
    for b, iou in enumerate(ref.iou_of("by_class")):
        best = iou.argmax(1)
        other += int(((iou.max(1) > 0.5) & (c["gt_labels"][b][best] != c["roi_labels"][b]) & (e["j"][b] != best)).sum())
    assert other >= 5
    # a hard quota above the hard count
    assert any(p["want"] > len(p["hard"]) > 0 and len(p["easy"]) and p["nh"] == len(p["hard"]) for p in _plans("few_fg"))
    assert any(p["want"] <= len(p["hard"]) and len(p["easy"]) and p["nh"] == p["want"] > 0 for p in _plans("both"))
    # odd sizes
    assert ref.case("odd")["rois"].shape[1:] == (65, 9) and kw("odd")["S"] == 1 and ref.expected("odd:fg0")["plans"][0]["nf"] == 0
    c = ref.case("odd:short")
    assert kw("odd:short")["S"] > c["rois"].shape[1] and _plans("odd:short")[0]["ranked"]
    c = ref.case("cap")
    assert c["rois"].shape[:2] == (1, 4096) and c["gt_boxes"].shape[1] == 2 and kw("cap")["S"] == 1024
    assert _plans("cap")[0]["ranked"] and _n(_plans("cap")[0])[0] > 1024 and all(_n(_plans("cap")[0]))


def test_iou_equal_to_a_threshold():
    for name in ("on_threshold", "on_threshold:cls"):
        kw, e = ref.case(name)["kw"], ref.expected(name)
        m = e["m"][0]
        assert F(kw["fg_thr"]) == F(kw["reg_fg_thr"]) == F(kw["cls_fg_thr"]) == F(0.5) and F(kw["bg_lo"]) == F(kw["cls_bg_thr"]) == F(0.25)
        assert list(np.flatnonzero(m == F(0.5))) == [0, 4] and list(np.flatnonzero(m == F(0.25))) == [1, 5]
        p = e["plans"][0]
        assert {0, 4} <= set(p["fg"]) and {1, 5} <= set(p["hard"]) and 3 in p["easy"]            # >= on both thresholds
        on_fg, on_bg = np.isin(e["index"][0], (0, 4)), np.isin(e["index"][0], (1, 5))
        assert on_fg.any() and on_bg.any()
        assert (e["reg_valid"][0][on_fg] == 0).all()                                             # m > reg_fg_thr is strict
        mid = F(1) if name == "on_threshold" else F(-1)                                          # m > cls_fg_thr is strict too
        assert (e["cls_target"][0][on_fg] == mid).all()
        assert (e["cls_target"][0][on_bg] == (F(0) if name == "on_threshold" else F(-1))).all()  # m < cls_bg_thr likewise


def test_picks_stay_inside_their_classes():
    """fg picks of a ranked scene are distinct members of fg in ascending (key, r); draws are members of their class; and the class
    sizes of the draws are no powers of two somewhere in every kind of draw."""
    sizes = dict(fg=set(), hard=set(), easy=set())
    for name in ref.CASES:
        c, e = ref.case(name), ref.expected(name)
        for b, p in enumerate(e["plans"]):
            idx = e["index"][b]
            if ref.counts_of(c)[b] == 0:
                continue
            nf, nh = p["nf"], p["nh"]
            assert np.isin(idx[:nf], p["fg"]).all() and np.isin(idx[nf:nf + nh], p["hard"]).all() and np.isin(idx[nf + nh:], p["easy"]).all()
            if p["ranked"]:
                assert len(set(idx[:nf])) == nf
                keys = [(int(ref.h(c["kw"]["seed"], b, int(r))), int(r)) for r in p["fg"]]
                assert [r for _, r in sorted(keys)[:nf]] == list(idx[:nf])
            elif nf:
                sizes["fg"].add(len(p["fg"]))
            if nh and nf + nh <= len(idx):
                sizes["hard"].add(len(p["hard"]))
            if len(idx) - nf - nh:
                sizes["easy"].add(len(p["easy"]))
    for kind, s in sizes.items():
        assert any(n & (n - 1) for n in s), f"{kind}: every class size drawn from is a power of two: {sorted(s)}"


def test_round_trip_and_heading_range():
    for name in ("both", "by_class", "heading", "cap"):
        c, e = ref.case(name), ref.expected(name)
        boxes = ref.roi_decode_vec(e["rois_s"], e["reg_target"])
        ref.check_round_trip(c, e, boxes)
        o = e["gt_local"][..., 6]
        assert (o >= -ref.HALF_PI).all() and (o <= ref.HALF_PI).all() and np.array_equal(o, e["reg_target"][..., 6])
    # the heading case: every RoI on the box got a slot; the flip leaves the box's axis where it was
    c, e = ref.case("heading"), ref.expected("heading")
    n = len(ref.HEADING_DR)
    assert set(e["index"][0][:n]) == set(range(n))
    for i in range(n):
        r = e["index"][0, i]
        dr = float(c["gt_boxes"][0, 0, 6]) - float(c["rois"][0, r, 6])
        o = float(e["gt_local"][0, i, 6])
        assert abs(np.sin(o - dr)) < 2e-5 or abs(abs(o) - np.pi / 2) < 2e-5, (r, dr, o)         # the same axis, modulo pi
    flipped = [abs(((float(e["gt_local"][0, i, 6]) - ref.HEADING_DR[e["index"][0, i]]) / np.pi)) for i in range(n)]
    assert any(round(f) % 2 == 1 for f in flipped) and any(round(f) % 2 == 0 for f in flipped)


def test_decode_forms_agree():
    e = ref.expected("both")
    rng = np.random.default_rng(5)
    reg = rng.normal(0, 0.3, e["reg_target"].shape).astype(F)
    a, b = ref.roi_decode_vec(e["rois_s"], reg), ref.roi_decode_loop(e["rois_s"], reg)
    assert np.array_equal(a.view(np.int32), b.view(np.int32))
