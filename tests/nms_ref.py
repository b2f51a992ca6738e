"""Numpy reference of SPEC.md §23 (box selection and NMS at scale), written in the section's own order, plus the crowded
scene generator and the named cases the CPU and GPU tests share (tests/test_nms_select_cpu.py asserts on the CPU the
coverage the GPU cases rely on; tests/test_gpu_nms_select.py compares the kernels with `expected(case)`).

The walk asks the oracle's `iou_bev` for (kept, candidate) pairs, one batched call per candidate: no K x K matrix.  Before
the call the kept boxes are narrowed to those whose footprint can touch the candidate's: centres no farther apart than the
two half-diagonals plus 1 m.  Outside that distance the rectangles are separated by >= 1 m, every vertex the clipping
produces lies (to rounding, ~1e-5 m at these coordinates) inside polygon a and hence >= 0.7 m outside one of b's four
half-planes, so the clipped polygon is empty and §13's IoU is exactly 0.0 — which the reference then uses.  (For
`iou_thr < 0`, where IoU 0 suppresses, the narrowing is switched off.)  `oracle.nms_bev`, which clips every pair, is the
independent second form the CPU tests compare this with."""
import functools

import numpy as np

F = np.float32
CAR = (3.9, 1.6, 1.56)


def _oracle():
    import oracle
    oracle.build()
    return oracle


def rows9(boxes):
    """[..., D >= 7] -> [..., 9] float32 rows for the oracle (columns 7, 8 zero: iou_bev never reads them)."""
    boxes = np.asarray(boxes, F)
    out = np.zeros(boxes.shape[:-1] + (9,), F)
    out[..., :7] = boxes[..., :7]
    return out


def rank_candidates(scores, score_thr):
    """§23 steps 1: indices of the candidates of one scene in rank order (score descending, index ascending)."""
    scores = np.asarray(scores, F)
    cand = np.nonzero(scores >= F(score_thr))[0]
    return cand[np.lexsort((cand, -scores[cand]))]


def nms_scene(boxes, scores, labels, iou_thr, score_thr=0.0, pre_max=None, post_max=None):
    """One scene.  -> kept indices in rank order (int64 array)."""
    orc = _oracle()
    K = boxes.shape[0]
    thr = F(iou_thr)
    ranked = rank_candidates(scores, score_thr)                       # 1. candidates, ranked
    ranked = ranked[:K if pre_max is None else pre_max]                # 2. pre-selection
    cap = K if post_max is None else post_max
    b9 = rows9(boxes)
    xy = b9[:, :2].astype(np.float64)
    rad = 0.5 * np.hypot(b9[:, 3].astype(np.float64), b9[:, 4].astype(np.float64))
    # kept boxes binned by centre into square cells one reach wide (reach = the largest distance at which two footprints
    # of this scene can be within 1 m): a candidate's possible partners are in its own and the eight adjacent cells
    narrow = thr >= 0
    reach = 2.0 * float(rad.max()) + 1.0 if K else 1.0
    cell = np.floor(xy / reach).astype(np.int64)
    bins = {}
    kept = np.empty((len(ranked),), np.int64)
    nk = 0
    for p in ranked:                                                   # 3. greedy walk in rank order
        if nk >= cap:                                                  # 4. post cap
            break
        if narrow:
            cx, cy = int(cell[p, 0]), int(cell[p, 1])
            q = [i for dx in (-1, 0, 1) for dy in (-1, 0, 1) for i in bins.get((cx + dx, cy + dy), ())]
            q = np.array(sorted(q), np.int64)
            if len(q):
                d = np.hypot(xy[q, 0] - xy[p, 0], xy[q, 1] - xy[p, 1])
                q = q[d <= rad[q] + rad[p] + 1.0]
        else:
            q = kept[:nk]
        if labels is not None and len(q):
            q = q[labels[q] == labels[p]]
        if len(q) and (orc.iou_bev(b9[q], np.repeat(b9[p][None], len(q), 0)) > thr).any():
            continue
        kept[nk] = p
        nk += 1
        if narrow:
            bins.setdefault((int(cell[p, 0]), int(cell[p, 1])), []).append(int(p))
    return kept[:nk]


def nms_boxes(boxes, scores, labels, iou_thr, score_thr=0.0, pre_max=None, post_max=None):
    """§23.  boxes [B,K,D], scores [B,K], labels [B,K] or None -> (keep [B,K] int32, order [B,P] int32, count [B] int32)."""
    boxes, scores = np.asarray(boxes, F), np.asarray(scores, F)
    B, K = scores.shape
    P = min(K, K if pre_max is None else pre_max, K if post_max is None else post_max)
    keep = np.zeros((B, K), np.int32)
    order = np.full((B, P), -1, np.int32)
    count = np.zeros((B,), np.int32)
    for b in range(B):
        kept = nms_scene(boxes[b], scores[b], None if labels is None else np.asarray(labels[b]), iou_thr, score_thr, pre_max, post_max)
        keep[b, kept] = 1
        order[b, :len(kept)] = kept
        count[b] = len(kept)
    return keep, order, count


def iou_matrix(boxes):
    """Full K x K §13 IoU of one SMALL scene, [p, q] = iou_bev(a = p, b = q): for coverage statements only."""
    b9 = rows9(boxes)
    K = b9.shape[0]
    a = np.repeat(b9, K, 0)
    b = np.tile(b9, (K, 1))
    return _oracle().iou_bev(a, b).reshape(K, K)


# ---- generator -------------------------------------------------------------------------------------------------------
DENSITY = 0.35          # boxes per square metre of the crowded scenes: about a third of the boxes survive at IOU_THR
IOU_THR = 0.1


def crowded(rng, B, K, D=7, density=DENSITY, n_eff=None):
    """Car-sized boxes with uniform yaw, centres uniform in a square of area n_eff / density (n_eff = K: constant density;
    n_eff = pre_max when only the best pre_max of K boxes enter the walk)."""
    side = np.sqrt((K if n_eff is None else n_eff) / density)
    bx = np.zeros((B, K, D), F)
    bx[..., 0:2] = rng.uniform(0, side, (B, K, 2))
    bx[..., 2] = -1.0
    bx[..., 3:6] = CAR
    bx[..., 6] = rng.uniform(-np.pi, np.pi, (B, K))
    return bx


def with_scores(bx7, scores, labels=None):
    """[B,K,7] + scores (+ labels as floats) -> the detector's 9-column rows."""
    out = rows9(bx7)
    out[..., 7] = scores
    if labels is not None:
        out[..., 8] = labels
    return out


# ---- the named cases (inputs are built once per process and never modified) ------------------------------------------
IDENTITY_K = (1, 63, 64, 65, 511, 512, 513, 1025, 2049)
TIE_VALUES = np.array([0.75, 0.5, 0.0, -0.0, -1.0], F)


@functools.lru_cache(maxsize=None)
def case(name):
    """-> dict(boxes [B,K,D], scores [B,K], labels [B,K] or None, kw = dict(iou_thr, score_thr, pre_max, post_max))."""
    kind, _, arg = name.partition(":")
    kw = dict(iou_thr=IOU_THR, score_thr=0.0, pre_max=None, post_max=None)
    labels = None
    if kind == "identity":                                   # test 1: D = 9, scores = column 7, B = 2
        K = int(arg)
        rng = np.random.default_rng(1000 + K)
        scores = rng.uniform(0.05, 1.0, (2, K)).astype(F)
        boxes = with_scores(crowded(rng, 2, K), scores, rng.integers(0, 3, (2, K)))
    elif kind == "chains":                                   # test 2
        rng = np.random.default_rng(2)
        scores = rng.uniform(0.05, 1.0, (2, 200)).astype(F)
        boxes = crowded(rng, 2, 200, density=0.6)
    elif kind == "ties":                                     # test 3 (pre_max is set per cut by the tests)
        rng = np.random.default_rng(3)
        scores = TIE_VALUES[rng.choice(5, (2, 300), p=(0.15, 0.2, 0.25, 0.25, 0.15))]
        boxes = crowded(rng, 2, 300)
        kw["score_thr"] = -0.0
    elif kind == "post":                                     # test 4 (post_max is set by the tests)
        rng = np.random.default_rng(4)
        scores = rng.uniform(0.05, 1.0, (2, 600)).astype(F)
        boxes = crowded(rng, 2, 600)
    elif kind == "head":                                     # test 5, first instance: SECOND's KITTI grid
        rng = np.random.default_rng(5)
        K = 70400
        scores = rng.uniform(0.0, 1.0, (2, K)).astype(F)
        for b in range(2):
            scores[b, rng.choice(K, 2000, replace=False)] = F(0.99)
        boxes = crowded(rng, 2, K, n_eff=1000)
        kw.update(pre_max=1000, post_max=100, score_thr=0.3)
    elif kind == "cap":                                      # test 5, second instance: pre_max at the cap, boxes 10 m apart
        rng = np.random.default_rng(6)
        K = 65537
        scores = rng.uniform(0.0, 1.0, (2, K)).astype(F)
        boxes = np.zeros((2, K, 7), F)
        g = np.arange(K)
        boxes[..., 0] = (g % 257) * 10.0
        boxes[..., 1] = (g // 257) * 10.0
        boxes[..., 3:6] = CAR
        boxes[..., 6] = rng.uniform(-np.pi, np.pi, (2, K))
        kw.update(pre_max=16384)
    elif kind == "classes":                                  # test 6
        rng = np.random.default_rng(7)
        scores = rng.uniform(0.05, 1.0, (2, 400)).astype(F)
        boxes = crowded(rng, 2, 400, density=0.6)
        values = np.array([0, 1, 2] if arg == "small" else [-5, 0, 2 ** 30], np.int32)
        labels = values[rng.integers(0, 3, (2, 400))]
    elif kind == "layout":                                   # test 7: column 7 holds the scores in REVERSE order
        rng = np.random.default_rng(8)
        scores = rng.uniform(0.05, 1.0, (2, 150)).astype(F)
        boxes = crowded(rng, 2, 150, D=int(arg))
        if int(arg) == 9:
            boxes[..., 7] = scores[:, ::-1]
            boxes[..., 8] = 7.0
    else:
        raise KeyError(name)
    for a in (boxes, scores) + (() if labels is None else (labels,)):
        a.setflags(write=False)
    return dict(boxes=boxes, scores=scores, labels=labels, kw=kw)


@functools.lru_cache(maxsize=None)
def _expected(name, items):
    c = case(name)
    kw = dict(c["kw"])
    kw.update(dict(items))
    out = nms_boxes(c["boxes"], c["scores"], c["labels"], **kw)
    for a in out:
        a.setflags(write=False)
    return out


def expected(name, **override):
    """The reference's (keep, order, count) of a named case, computed once per process (read-only arrays)."""
    return _expected(name, tuple(sorted(override.items())))


def kept_fraction(name, **override):
    c = case(name)
    return float(expected(name, **override)[2].sum()) / c["scores"].size


def cut_inside_tie(scores, score_thr, pre_max):
    """Does the pre-selection cut fall strictly inside a group of equal scores (so that indices decide who goes on)?"""
    r = rank_candidates(scores, score_thr)
    return 0 < pre_max < len(r) and scores[r[pre_max - 1]] == scores[r[pre_max]]


def chain_coverage(name):
    """(boxes kept although a higher-ranked box overlaps them above the threshold — every such box was itself suppressed,
    boxes suppressed by a kept box more than 64 ranks above them), counted on the reference's result of a small case."""
    c, want = case(name), expected(name)
    revived = far = 0
    for b in range(c["scores"].shape[0]):
        r = rank_candidates(c["scores"][b], c["kw"]["score_thr"])
        hit = iou_matrix(c["boxes"][b][r]) > F(c["kw"]["iou_thr"])      # [p, q] in rank order
        kept = want[0][b][r].astype(bool)
        for q in range(len(r)):
            above = np.nonzero(hit[:q, q])[0]
            revived += bool(kept[q] and len(above) and not kept[above].any())
            far += bool(not kept[q] and (kept[above] & (q - above > 64)).any())
    return revived, far


def tie_cuts(name):
    """The pre_max values of the tie case (n = candidates of scene 0) -> (cuts, cut strictly inside a tie group of scene 0?,
    ... and that group is the one of the zeros, holding both signs?)."""
    c = case(name)
    s0, thr = c["scores"][0], c["kw"]["score_thr"]
    r = rank_candidates(s0, thr)
    n = len(r)
    assert n == int((s0 > -1).sum())                                     # both zeros are candidates, -1.0 is not
    cuts = (1, 64, 65, n - 1, n, n + 7)
    inside = [bool(cut_inside_tie(s0, thr, p)) for p in cuts]
    zeros = s0[r][s0[r] == 0]
    mixed = bool(np.signbit(zeros).any() and (~np.signbit(zeros)).any())
    in_zero = [i and mixed and s0[r[p - 1]] == 0 for i, p in zip(inside, cuts)]
    return cuts, inside, in_zero
