"""The reference of SPEC.md §36 (tests/det_eval_ref.py) checked on its own, without a GPU: hand-worked scenes whose answer is
known, a brute-force float64 re-implementation of the matching rule on the cases whose pair values keep 1e-5 clear of every
threshold (asserted, so no case is silently left out), and the coverage every case claims, asserted on the reference's outputs
(tests/test_gpu_det_eval.py relies on it)."""
import numpy as np
import pytest

import box_ref
import box_truth
import det_eval_ref as ref

F = np.float32


def _rows(codes, n_gt, scores=None):
    """One class, one threshold: rows in score order with the given codes."""
    n = len(codes)
    sc = np.linspace(1.0, 0.1, n).astype(F) if scores is None else np.asarray(scores, F)
    return ref.det_ap(sc, np.zeros(n, np.int32), np.asarray(codes, np.int32)[:, None], np.array([n_gt], np.int32))


def test_hand_worked_ap():
    perfect = _rows([1] * 7, 7)
    assert perfect["ap"][0, 0] == 1.0 and (perfect["prec"] == 1.0).all() and perfect["max_recall"][0, 0] == 1.0
    assert perfect["n_det"][0, 0] == 7
    none = _rows([0] * 5, 3)
    assert none["ap"][0, 0] == 0.0 and (none["prec"] == 0.0).all() and none["max_recall"][0, 0] == 0.0 and none["n_det"][0, 0] == 5
    # TP, FP, TP against two boxes: precision 1, 1/2, 2/3 at recall 1/2, 1/2, 1; envelope 1, 2/3, 2/3.  R40: the 20 positions up to
    # 0.5 sample 1, the 20 above sample 2/3: AP = (20 + 20 * 2/3) / 40 = 5/6
    two = _rows([1, 0, 1], 2)
    assert (two["prec"][0, 0, :20] == 1.0).all() and (two["prec"][0, 0, 20:] == F(2) / F(3)).all()
    assert abs(float(two["ap"][0, 0]) - 5 / 6) < 1e-6
    # ignored rows change nothing, wherever they stand; rows of equal score count in row order
    assert _rows([-1, 1, -1, 0, 1, -1], 2)["ap"][0, 0] == two["ap"][0, 0]
    assert _rows([1, 0, 1], 2, scores=[0.5, 0.5, 0.5])["ap"][0, 0] == two["ap"][0, 0]
    # recall stops at 1/2: the upper 20 positions sample 0; R11 on the same rows: positions 0 .. 5 sample 1 -> 6/11
    half = _rows([1, 0], 2)
    assert abs(float(half["ap"][0, 0]) - 0.5) < 1e-6 and half["max_recall"][0, 0] == 0.5
    r11 = ref.det_ap(np.array([.9, .8], F), np.zeros(2, np.int32), np.array([[1], [0]], np.int32), np.array([2], np.int32), 10, 0, 0.0)
    assert abs(float(r11["ap"][0, 0]) - 6 / 11) < 1e-6 and r11["prec"].shape == (1, 1, 11)
    # nuScenes' floors: a perfect detector still gets 1, precision 0.1 and below counts as 0
    ns = ref.det_ap(np.linspace(1, .1, 4).astype(F), np.zeros(4, np.int32), np.ones((4, 1), np.int32), np.array([4], np.int32), 100, 11, 0.1)
    assert abs(float(ns["ap"][0, 0]) - 1.0) < 1e-6 and ns["prec"].shape == (1, 1, 90)
    # a class without ground truth
    assert _rows([0, 0], 0)["ap"][0, 0] == -1.0


def test_hand_worked_scene():
    """tests/det_eval_ref.py::_hand, worked in its docstring."""
    e = ref.expected("hand")
    code, match, gt_det = e["code"][0], e["match"][0], e["gt_det"][0]
    # columns: thr 0.7, 0.5
    assert code.tolist() == [[0, 1], [1, 0], [1, 1], [1, 1], [-1, 1], [-1, -1], [-1, -1], [0, -1], [0, 0]]
    assert match.tolist() == [[-1, 0], [0, -1], [1, 1], [2, 2], [3, 4], [3, 3], [3, 3], [-1, 3], [-1, -1]]
    assert gt_det.tolist() == [[1, 0], [2, 2], [3, 3], [-1, -1], [-1, 4]]
    assert e["n_gt"].tolist() == [[4]]
    assert abs(float(e["value"][0, 0, 1]) - 3 / 5) < 1e-6 and abs(float(e["value"][0, 1, 0]) - 31 / 33) < 1e-6
    assert (e["value"][0][code == 0] == 0).all()


def test_the_pair_value_is_the_pairwise_iou():
    """vals[k,g] of the reference are box_ref's matrices, bit for bit, where the rule reads them."""
    for name, mode in (("basic", "3d"), ("basic:bev", "bev")):
        c, e = ref.case(name), ref.expected(name)
        full = box_ref.boxes_iou(c["det_boxes"][:1], c["gt_boxes"][:1], mode)
        read = ~np.isnan(e["vals"][0])
        assert read.sum() > 50 and (e["vals"][0][read] == full[0][read]).all()


def _values64(c, b):
    K, G = c["det_boxes"].shape[1], c["gt_boxes"].shape[1]
    C = c["thr"].shape[0]
    vals = np.full((K, G), np.nan)
    live, gl, dl = ref.live_mask(c, b), c["gt_labels"][b], c["det_labels"][b]
    pairs = [(k, g) for k in np.flatnonzero(live).tolist() for g in np.flatnonzero((gl == dl[k]) & (gl < C)).tolist()]
    if not pairs:
        return vals
    ks, gs = (np.array(x) for x in zip(*pairs))
    a, g = c["det_boxes"][b][ks], c["gt_boxes"][b][gs]
    if c["metric"] == "dist":
        v = np.hypot(a[:, 0].astype(np.float64) - g[:, 0], a[:, 1].astype(np.float64) - g[:, 1])
    else:
        v = (box_truth.iou3d64 if c["metric"] == "iou3d" else box_truth.iou_bev64)(a, g)
    vals[ks, gs] = v
    return vals


def _match64(c):
    """The rule of §36.1 restated on float64 values: per threshold, detections by descending score, each to the best free box."""
    B, K = c["det_labels"].shape
    G, (C, T) = c["gt_labels"].shape[1], c["thr"].shape
    code, match = np.full((B, K, T), -1, np.int32), np.full((B, K, T), -1, np.int32)
    sign = 1.0 if c["metric"] == "dist" else -1.0
    for b in range(B):
        v = _values64(c, b)
        ign = np.zeros(G, bool) if c["gt_ignore"] is None else c["gt_ignore"][b] != 0
        live = np.flatnonzero(ref.live_mask(c, b))
        order = live[np.lexsort((live, -c["det_scores"][b][live].astype(np.float64)))]
        for t in range(T):
            free = ~ign
            for k in order.tolist():
                th = float(c["thr"][c["det_labels"][b, k], t])
                ok = np.nan_to_num(sign * v[k], nan=np.inf) < sign * th
                pick = -1
                for pool, cd in ((ok & free, 1), (ok & ign, -1)):
                    if pool.any():
                        cand = np.flatnonzero(pool)
                        pick = int(cand[np.argmin(sign * v[k, cand])])       # (argmin: the first, i.e. lowest g, on a tie)
                        code[b, k, t], match[b, k, t] = cd, pick
                        if cd == 1:
                            free = free.copy()
                            free[pick] = False
                        break
                if pick < 0:
                    code[b, k, t] = 0
    return code, match


@pytest.mark.parametrize("name", ref.F64_CASES)
def test_float64_brute_force(name):
    margin = ref.threshold_margin(name)
    assert margin > 1e-5, f"{name}: a pair value lies {margin} from a threshold; the case cannot be judged in float64"
    code, match = _match64(ref.case(name))
    e = ref.expected(name)
    assert (code == e["code"]).all() and (match == e["match"]).all()


@pytest.mark.parametrize("name", ref.CASES)
def test_coverage_of_the_matching_cases(name):
    c, e = ref.case(name), ref.expected(name)
    missing = ref.CLAIMS[name] - ref.coverage(name)
    assert not missing, f"{name} does not show {sorted(missing)}"
    B, K = c["det_labels"].shape
    if name != "big" and name != "wave":
        assert B <= 4 and K <= 96 and c["gt_labels"].shape[1] <= 80
    # every output is consistent with the others
    for b in range(B):
        live = ref.live_mask(c, b)
        assert (e["code"][b][~live] == -1).all() and (e["match"][b][~live] == -1).all() and (e["value"][b][~live] == 0).all()
        for t in range(c["thr"].shape[1]):
            won = np.flatnonzero(e["code"][b, :, t] == 1)
            assert len(set(e["match"][b, won, t].tolist())) == len(won)               # a box is taken once
            assert (e["gt_det"][b, e["match"][b, won, t], t] == won).all()
            assert int((e["gt_det"][b, :, t] >= 0).sum()) == len(won)


def test_the_ties_case_tells_a_wrong_ranking_from_the_right_one(monkeypatch):
    """What `ties` is there for, shown on the reference: a ranking that compares the score BITS (-0 below +0) changes who gets a
    box in scene 1 (and nothing in scene 0, which holds no zero), and one that breaks ties by the HIGHER index changes scene 0."""
    c, e = ref.case("ties"), ref.expected("ties")

    def by_bits(scores, live):
        u = np.asarray(scores, F).view(np.uint32).astype(np.int64)
        asc = np.where(u >> 31, 0xFFFFFFFF - u, u + 0x80000000)
        return sorted(np.flatnonzero(live).tolist(), key=lambda i: (-int(asc[i]), i))

    monkeypatch.setattr(ref, "rank_order", by_bits)
    m = ref.det_match(c, vals=e["vals"])
    assert (m["match"][0] == e["match"][0]).all() and (m["gt_det"][1] != e["gt_det"][1]).any() and (m["code"][1] != e["code"][1]).any()
    # the boxes of the even groups (their lowest index holds -0) change hands, those of the odd groups do not
    changed = {int(g) for g in np.flatnonzero((m["gt_det"][1] != e["gt_det"][1]).any(1))}
    assert changed == {0, 2, 4}
    monkeypatch.setattr(ref, "rank_order", lambda s, live: sorted(np.flatnonzero(live).tolist(), key=lambda i: (-float(s[i]), -i)))
    assert (ref.det_match(c, vals=e["vals"])["gt_det"][0] != e["gt_det"][0]).any()


def test_the_presets_are_the_librarys(sad):
    """The reference and the module name the same (points, first, floor) presets, and the operators' output lists are the reference's."""
    from sad_amd import evaluate, ops
    assert evaluate.PRESETS == ref.PRESETS
    assert ops.DET_MATCH_OUTPUTS == ref.OUTPUTS and ops.DET_AP_OUTPUTS == ref.AP_OUTPUTS
    assert set(ref.case("basic")) - {"metric"} == {"det_boxes", "det_scores", "det_labels", "det_count", "gt_boxes", "gt_labels", "gt_ignore", "thr"}


def test_every_claim_is_made_somewhere():
    made = set().union(*ref.CLAIMS.values())
    assert made >= {"count0", "count1", "countK", "g0", "class_without_gt", "class_without_det", "labels_outside", "score_tie", "pm0",
                    "identical_gt", "greedy_steal", "diverge", "ignore_absorbs3", "nonignored_preferred", "on_thr", "class65", "class130",
                    "k1024g1024", "iou3d", "iou_bev", "dist", "d9", "t8"}
    assert {c["metric"] for c in map(ref.case, ("on_thr", "on_thr:bev", "on_thr:dist"))} == {"iou3d", "iou_bev", "dist"}
    assert {ref.case(n)["det_boxes"].shape[2] for n in ref.CASES} >= {7, 9}


def test_coverage_of_the_ap_cases():
    sizes = {ref.ap_case(n)["scores"].shape[0] for n in ref.AP_CASES}
    assert sizes >= {1, 255, 256, 257} and max(sizes) >= 5000
    assert {(c["points"], c["first"], F(c["floor"])) for c in map(ref.ap_case, ref.AP_CASES)} >= {
        (p, f, F(fl)) for p, f, fl in ref.PRESETS.values()}
    assert (ref.ap_case("all_ignored")["code"] == -1).all()
    e = ref.ap_expected("all_ignored")
    assert (e["n_det"] == 0).all() and e["ap"][0].tolist() == [0, 0] and e["ap"][1].tolist() == [-1, -1]
    assert len(np.unique(ref.ap_case("all_tied")["scores"])) <= 4
    e = ref.ap_expected("no_gt")
    assert (e["ap"][0] == -1).all() and (e["ap"][2] == -1).all() and (e["ap"][1] >= 0).all() and (e["prec"][0] == 0).all()
    e = ref.ap_expected("low_recall")
    assert (e["max_recall"] < 0.5).all() and (e["max_recall"] > 0).all() and (e["ap"] > 0).all() and (e["prec"][..., -1] == 0).all()
    assert (ref.ap_expected("all_fp")["ap"] == 0).all() and (ref.ap_expected("n1")["ap"] == 1).all()
    e = ref.ap_expected("n5000")
    assert e["max_recall"][0].max() == 1.0 and (e["max_recall"][1:] < 1).all() and ((e["ap"] > 0) & (e["ap"] < 1)).all()
    # the samples are an envelope: non-increasing in k
    for n in ref.AP_CASES:
        p = ref.ap_expected(n)["prec"]
        assert (p[..., 1:] <= p[..., :-1]).all(), n


def test_evaluate_is_batching_invariant():
    """The reference's own statement of §36.3: the scenes of a case one at a time give the rows of the whole case."""
    c = ref.case("basic")
    whole = ref.evaluate([c])
    singles = []
    for b in range(c["det_labels"].shape[0]):
        singles.append({k: (v[b:b + 1] if isinstance(v, np.ndarray) and k != "thr" else v) for k, v in c.items()})
    parts = ref.evaluate(singles)
    for k in whole:
        assert (whole[k] == parts[k]).all(), k
