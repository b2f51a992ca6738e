"""The numpy reference of SPEC.md §23 (tests/nms_ref.py) against the oracle's independent nms_bev, its own limits against
each other, and — on the CPU, where a miss costs nothing — the coverage every GPU case of tests/test_gpu_nms_select.py
relies on.  If a family misses its coverage, change the generator's density, never the assertion."""
import numpy as np
import pytest

import nms_ref as ref

F = np.float32


def _eq(got, want, what=""):
    for name, g, w in zip(("keep", "order", "count"), got, want):
        np.testing.assert_array_equal(g, w, err_msg=f"{what} {name}")


@pytest.mark.parametrize("K", [1, 65, 513, 1500])
def test_reference_equals_oracle_nms_bev(orc, K):
    rng = np.random.default_rng(K)
    scores = rng.uniform(0.0, 1.0, (2, K)).astype(F)
    scores[:, ::7] = scores[:, 0:1]                                   # ties
    boxes = ref.with_scores(ref.crowded(rng, 2, K), scores)
    for iou_thr, score_thr in ((ref.IOU_THR, 0.0), (0.5, 0.3)):
        want = orc.nms_bev(boxes, iou_thr, score_thr)
        _eq(ref.nms_boxes(boxes, scores, None, iou_thr, score_thr), want, f"K={K}")
        _eq(ref.nms_boxes(boxes[..., :7], scores, None, iou_thr, score_thr), want, f"K={K}, 7 columns")
    if K > 1:
        assert want[2].sum() < 2 * K


def test_pre_max_is_nms_of_the_top_slice():
    c = ref.case("ties")
    boxes, scores, thr = c["boxes"], c["scores"], c["kw"]["score_thr"]
    for pre in (1, 64, 65, 200, 400):
        got = ref.nms_boxes(boxes, scores, None, ref.IOU_THR, thr, pre_max=pre)
        for b in range(2):
            top = ref.rank_candidates(scores[b], thr)[:pre]
            top_sorted = np.sort(top)                                  # slicing keeps index order, so ties rank alike
            sub = ref.nms_scene(boxes[b][top_sorted], scores[b][top_sorted], None, ref.IOU_THR, thr)
            np.testing.assert_array_equal(got[1][b, :got[2][b]], top_sorted[sub])
            assert (got[1][b, got[2][b]:] == -1).all()


def test_post_max_truncates_the_unlimited_order():
    full = ref.expected("post")
    for post in (1, 7, 100, 599, 600, 1000):
        got = ref.expected("post", post_max=post)
        assert got[1].shape == (2, min(600, post))
        for b in range(2):
            m = min(post, full[2][b])
            assert got[2][b] == m
            np.testing.assert_array_equal(got[1][b, :m], full[1][b, :m])
            assert (got[1][b, m:] == -1).all() and got[0][b].sum() == m


def test_class_aware_reference_is_per_class_nms():
    c = ref.case("classes:big")
    want = ref.expected("classes:big")
    for b in range(2):
        kept = []
        for v in np.unique(c["labels"][b]):
            sel = np.nonzero(c["labels"][b] == v)[0]
            kept += list(sel[ref.nms_scene(c["boxes"][b][sel], c["scores"][b][sel], None, ref.IOU_THR)])
        assert sorted(kept) == sorted(want[1][b, :want[2][b]])


def test_negative_threshold_and_narrowing():
    """iou_thr < 0: IoU 0 suppresses, so one box per scene survives; and the narrowing never changes a result
    (the oracle clips every pair)."""
    c = ref.case("layout:7")
    got = ref.nms_boxes(c["boxes"], c["scores"], None, -0.5)
    assert (got[2] == 1).all()


# ---- the coverage the GPU cases rely on ------------------------------------------------------------------------------
@pytest.mark.parametrize("K", ref.IDENTITY_K)
def test_coverage_identity(orc, K):
    name = f"identity:{K}"
    c = ref.case(name)
    np.testing.assert_array_equal(c["boxes"][..., 7], c["scores"])
    want = orc.nms_bev(c["boxes"], ref.IOU_THR, 0.0)
    _eq(ref.expected(name), want, name)
    if K >= 64:
        assert 0.2 < want[2].sum() / (2 * K) < 0.8


def test_coverage_chains():
    revived, far = ref.chain_coverage("chains")
    assert revived >= 1 and far >= 1


def test_coverage_ties():
    cuts, inside, in_zero = ref.tie_cuts("ties")
    assert sum(inside) >= 2 and any(in_zero)
    s0 = ref.case("ties")["scores"][0]
    assert (np.signbit(s0) & (s0 == 0)).any() and (~np.signbit(s0) & (s0 == 0)).any()
    r = ref.rank_candidates(s0, -0.0)                                 # a cut inside a tie group takes the lowest indices
    for p, i in zip(cuts, inside):
        if i:
            grp = np.nonzero(s0 == s0[r[p]])[0]
            taken = np.intersect1d(grp, r[:p])
            np.testing.assert_array_equal(taken, grp[:len(taken)])


def test_coverage_post():
    assert 5 < int(ref.expected("post")[2][0]) < 595


def test_coverage_head_and_cap():
    c = ref.case("head")
    for b in range(2):
        assert ref.cut_inside_tie(c["scores"][b], c["kw"]["score_thr"], 1000)
    want = ref.expected("head", post_max=None)
    assert (want[2] < 900).all() and (want[2] > 100).all()
    assert (ref.expected("head")[2] == 100).all()
    cap = ref.expected("cap")
    assert (cap[2] == 16384).all() and cap[1].shape == (2, 16384)


@pytest.mark.parametrize("which", ["small", "big"])
def test_coverage_classes(which):
    name = f"classes:{which}"
    c = ref.case(name)
    want = ref.expected(name)
    agnostic = ref.nms_boxes(c["boxes"], c["scores"], None, **c["kw"])
    assert not np.array_equal(want[0], agnostic[0]) and want[2].sum() / 800 < 0.9
    assert len(np.unique(c["labels"])) == 3


def test_coverage_layout():
    c7, c9 = ref.case("layout:7"), ref.case("layout:9")
    np.testing.assert_array_equal(c7["boxes"], c9["boxes"][..., :7])
    other = ref.nms_boxes(c9["boxes"], c9["boxes"][..., 7], None, **c9["kw"])
    assert not np.array_equal(ref.expected("layout:7")[1], other[1])
    _eq(ref.expected("layout:9"), ref.expected("layout:7"))


# ---- score regimes, stage boundaries and the walk's reach: the coverage (figures printed, then asserted by cover_*) -----
@pytest.mark.parametrize("family", ["logits", "mixed", "wide", "ladder", "runs", "thresholds", "stages", "post_chunk", "far",
                                    "crowded4k"])
def test_coverage_of_the_new_families(family):
    print(family, getattr(ref, f"cover_{family}")())


def test_score_key_is_monotone_in_the_float():
    """score_key_np orders as floats do, with both zeros on one key — over every score the new cases use."""
    names = ["logits", "mixed", "wide", "thresholds"] + [f"ladder:{q}" for q in ref.LADDER] + [f"runs:{p}" for p in ref.RUNS]
    s = np.unique(np.concatenate([ref.case(n)["scores"].ravel() for n in names]))        # ascending, -0.0 == +0.0 merged
    k = ref.score_key_np(s).astype(np.int64)
    assert len(s) > 5000 and (np.diff(k) > 0).all()
    assert ref.score_key_np(np.array([-0.0], F))[0] == ref.score_key_np(np.array([0.0], F))[0] == 0x80000000
    prof = ref.radix_profile(np.array([3.0, -1.0, 2.0, 2.0, -0.0, 0.0], F), 2.5, 2)
    assert prof == dict(key=int(ref.score_key_np(np.array([2.0], F))[0]), shared=(3, 2, 2, 2), decides="thr")
    assert ref.radix_profile(np.array([3.0, -1.0, 2.0], F), -2.0, 5)["key"] == int(ref.score_key_np(np.array([-1.0], F))[0])


SCORE_CASES = (["logits", "mixed", "wide", "thresholds", "crowded4k", "n5000"] + [f"ladder:{q}" for q in ref.LADDER]
               + [f"runs:{p}" for p in ref.RUNS] + [f"stride:{K}" for K in ref.STRIDE_K])


@pytest.mark.parametrize("name", SCORE_CASES)
def test_new_cases_equal_oracle_without_pre_max(orc, name):
    """Every score regime, without pre_max, against the oracle's nms_bev (scores in column 7): the ranking of negative,
    zero, subnormal, infinite and consecutive scores by the reference is the oracle's.  (`far` is left out: the oracle
    clips all 1.3e8 pairs of its 16 384 kept boxes; its expected result is asserted box by box in cover_far.)"""
    c = ref.case(name)
    thrs = [v for _, v in ref.threshold_values()] if name == "thresholds" else [c["kw"]["score_thr"]]
    for thr in thrs:
        want = orc.nms_bev(ref.with_scores(c["boxes"], c["scores"]), ref.IOU_THR, thr)
        got = ref.expected(name, pre_max=None, score_thr=float(thr)) if name == "thresholds" else \
            ref.nms_boxes(c["boxes"], c["scores"], None, ref.IOU_THR, thr)
        _eq(got, want, f"{name} score_thr={thr}")
