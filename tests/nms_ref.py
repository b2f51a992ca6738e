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


def score_key_np(scores):
    """§23's ordering as a uint32 that is monotone in the float, both zeros on one key (sign-flipped bits).  It only STATES
    coverage (which radix digits a case separates); expected results come from rank_candidates, which compares floats."""
    b = np.ascontiguousarray(scores, F).view(np.uint32)
    b = np.where((b & np.uint32(0x7FFFFFFF)) == 0, np.uint32(0), b)
    return np.where((b >> np.uint32(31)) != 0, ~b, b | np.uint32(0x80000000)).astype(np.uint32)


def radix_profile(scores, score_thr, P):
    """For the P-th largest key of one scene: key, shared = how many keys of the scene share its top 8, 16, 24 and 32 bits,
    decides = "thr" if score_thr's key lies above it (the threshold cuts the selection) else "key"."""
    keys = score_key_np(scores).ravel()
    kp = np.sort(keys)[::-1][min(P, len(keys)) - 1]
    shared = tuple(int(((keys >> np.uint32(sh)) == (kp >> np.uint32(sh))).sum()) for sh in (24, 16, 8, 0))
    kthr = score_key_np(np.array([score_thr], F))[0]
    return dict(key=int(kp), shared=shared, decides="thr" if kthr > kp else "key")


def first_drop(prof, K):
    """The first radix pass (0 .. 3) at which fewer than all K keys share the threshold key's prefix (None: all K equal)."""
    return next((p for p, c in enumerate(prof["shared"]) if c < K), None)


def key_bytes(prof):
    """The threshold key's digits at passes 0 .. 3."""
    return tuple((prof["key"] >> sh) & 255 for sh in (24, 16, 8, 0))


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

# score regimes (small crowded scenes) and stage boundaries; the cuts that depend on the drawn scores come from the
# *_cuts / *_values functions below, the rest are constants here
NINF = float("-inf")
MIXED_CUTS = (250, 450, 700)              # 300 positives, 300 zeros of both signs, 300 negatives
LADDER = {0: 0x3EFFFFFF, 1: 0x3F12FFFF, 2: 0x3F1234FF, 3: 0x3F1234FF}   # last bit pattern below the carry into pass q's digit
RUNS = ("equal", "asc", "desc", "alt")
STRIDE_K = (255, 256, 257, 1023, 1024, 4095, 4096, 4097)
N5000 = (15, 16, 17, 63, 64, 65, 127, 128, 129, 255, 256, 257, 2047, 2048, 2049, 4096)
BATCH37_N = (0, 1, 17, 64, 65, 300, 400)  # the last one is P = pre_max
FAR_D = (1, 63, 64, 65, 1024, 1087, 8192, 16000)


def _bits(a):
    return np.asarray(a, np.uint32).view(F)


def _case_scores_and_stages(kind, arg, kw):
    """-> (boxes, scores, labels, extra) of the score-regime, stage-boundary and walk-reach cases; sets kw."""
    labels, extra = None, {}
    if kind == "logits":                                     # raw logits: all negative, all distinct
        rng = np.random.default_rng(11)
        scores = (-np.abs(rng.normal(-4.0, 2.0, (2, 1000)))).astype(F)
        boxes = crowded(rng, 2, 1000, n_eff=400)
        kw.update(score_thr=-100.0, pre_max=400)
    elif kind == "mixed":                                    # (pre_max from MIXED_CUTS)
        rng = np.random.default_rng(12)
        zeros = np.where(rng.random((2, 300)) < 0.5, F(-0.0), F(0.0))
        scores = np.concatenate([rng.uniform(0.01, 1.0, (2, 300)), zeros, -rng.uniform(0.01, 1.0, (2, 300))], 1).astype(F)
        scores = rng.permuted(scores, axis=1)
        boxes = crowded(rng, 2, 900, n_eff=500)
        kw.update(score_thr=NINF)
    elif kind == "wide":                                     # log-uniform magnitudes over every exponent, both signs
        rng = np.random.default_rng(13)
        K = 1500
        u = lambda hi, n: rng.integers(0, hi, (2, n), dtype=np.uint32)
        scores = _bits((u(2, K) << np.uint32(31)) | (u(255, K) << np.uint32(23)) | u(1 << 23, K)).copy()
        sub = _bits((u(2, 80) << np.uint32(31)) | (u(1 << 23, 80) | np.uint32(1)))           # 80 more subnormals
        fi = np.finfo(F)
        special = np.array([np.inf, -np.inf, fi.max, -fi.max, fi.tiny, -fi.tiny, fi.smallest_subnormal, -fi.smallest_subnormal,
                            0.0, -0.0], F)
        for b in range(2):
            at = rng.choice(K, 80 + len(special), replace=False)
            scores[b, at[:80]] = sub[b]
            scores[b, at[80:]] = special
        boxes = crowded(rng, 2, K, n_eff=700)
        kw.update(score_thr=NINF)
    elif kind == "ladder":                                   # consecutive floats across the carry into radix digit q
        q = int(arg)
        rng = np.random.default_rng(140 + q)
        K, top = 384, LADDER[q]
        chain = np.arange(top - 255, top + 1, dtype=np.uint32) if q == 3 else np.arange(top - 159, top + 161, dtype=np.uint32)
        scores = np.empty((2, K), F)
        for b, sign in enumerate((0, 0x80000000)):           # scene 0: a positive chain, scene 1: the same one negated
            c = _bits(chain | np.uint32(sign))
            scores[b] = rng.permutation(np.concatenate([c, rng.choice(c, K - len(c))]))
        boxes = crowded(rng, 2, K, n_eff=250)
        kw.update(score_thr=NINF)
        extra = dict(chain=chain)
    elif kind == "runs":                                     # the histogram's run-length path at its extremes
        rng = np.random.default_rng(15)
        K = 1500
        if arg == "equal":
            scores = np.repeat(np.array([[0.5], [-1.25]], F), K, 1)
        elif arg in ("asc", "desc"):
            scores = np.sort(np.stack([rng.uniform(0.05, 1.0, K), -rng.uniform(0.05, 9.0, K)]).astype(F), 1)
            scores = np.ascontiguousarray(scores[:, ::-1]) if arg == "desc" else scores
        elif arg == "alt":
            scores = np.tile(np.array([[0.25, 0.75], [-1.0, -3.0]], F), (1, K // 2))
        else:
            raise KeyError(arg)
        boxes = crowded(rng, 2, K, n_eff=700)
        kw.update(score_thr=NINF, pre_max=700)
    elif kind == "thresholds":                               # scene 1 = scene 0 with one +Inf planted among the negatives
        rng = np.random.default_rng(16)
        s = np.concatenate([rng.uniform(0.1, 5.0, 350), np.full(50, 0.0), np.full(50, -0.0), -np.abs(rng.normal(-4.0, 2.0, 450)) - 0.01])
        s = rng.permutation(s.astype(F))
        scores = np.stack([s, s])
        scores[1, np.nonzero(s < 0)[0][7]] = np.inf
        boxes = crowded(rng, 2, 900, n_eff=500)
        kw.update(score_thr=NINF)
    elif kind == "stride":                                   # the strides of the two select kernels; no limits
        K = int(arg)
        rng = np.random.default_rng(1700 + K)
        scores = rng.uniform(0.05, 1.0, (1, K)).astype(F)
        boxes = crowded(rng, 1, K)
    elif kind == "n5000":                                    # n set by pre_max (P = n) or by score_thr (P = K)
        rng = np.random.default_rng(18)
        scores = rng.permutation(np.linspace(0.05, 1.0, 5000).astype(F))[None]
        boxes = crowded(rng, 1, 5000, n_eff=1000)
    elif kind == "batch37":                                  # one launch, scenes whose n differ widely
        rng = np.random.default_rng(19)
        B, K = 37, 600
        kw.update(score_thr=0.5, pre_max=400)
        u = rng.uniform(0.0, 1.0, (B, K)).astype(F)
        want = np.array([BATCH37_N[(b * 3) % 7] for b in range(B)])
        scores = np.empty((B, K), F)
        for b in range(B):                                   # scene-dependent offset: n of the scene's scores reach 0.5
            d = np.sort(u[b])[::-1].astype(np.float64)
            cut = d[0] + 0.1 if want[b] == 0 else d[-1] - 0.1 if want[b] == 400 else 0.5 * (d[want[b] - 1] + d[want[b]])
            scores[b] = (u[b].astype(np.float64) + (0.5 - cut)).astype(F)
        boxes = crowded(rng, B, K, n_eff=300)
        extra = dict(n=want)
    elif kind == "far":                                      # the walk's long reach: see _far
        boxes, scores, extra = _far()
    elif kind == "crowded4k":                                # dense suppression across all 64 chunks
        rng = np.random.default_rng(22)
        scores = rng.uniform(0.05, 1.0, (1, 4096)).astype(F)
        boxes = crowded(rng, 1, 4096)
        if arg == "classes":
            labels = rng.integers(0, 3, (1, 4096)).astype(np.int32)
    else:
        raise KeyError(kind)
    return boxes, scores, labels, extra


def _far():
    """K = n = 16 384 boxes 10 m apart (nothing overlaps by itself), ranks fixed through the scores, plus planted pairs
    (rank r, its copy at rank r + d: suppressed) and chains (A suppresses B, B overlaps C, A does not: C is kept)."""
    rng = np.random.default_rng(21)
    K = 16384
    g = np.arange(K)
    by_rank = np.zeros((K, 7), F)
    by_rank[:, 0], by_rank[:, 1] = (g % 128) * 10.0, (g // 128) * 10.0
    by_rank[:, 3:6] = CAR
    by_rank[:, 6] = rng.uniform(-np.pi, np.pi, K)
    pairs = []
    for i, d in enumerate(FAR_D):
        pairs.append((3 + 7 * i, 3 + 7 * i + d))                                   # suppressor in chunk 0
        r = 6405 + 200 * i if d <= 8192 else 300                                   # ... in a chunk >= 100 where r + d < K allows
        pairs.append((r, r + d))
    chains = [(60, 1160, 2360), (7700, 8800, 10000)]                             # chunks (0, 18, 36) and (120, 137, 156)
    slots = [r for pr in pairs + chains for r in pr]
    assert len(set(slots)) == len(slots) and max(slots) < K
    for r, q in pairs:
        by_rank[q] = by_rank[r]
    for a, b, c in chains:                                                       # car 3.9 m long, yaw 0: IoU(A,B) = IoU(B,C) = 0.32, IoU(A,C) = 0
        by_rank[a, 6] = 0.0
        by_rank[b], by_rank[c] = by_rank[a], by_rank[a]
        by_rank[b, 0] += 2.0
        by_rank[c, 0] += 4.0
    perm = rng.permutation(K)                                                    # perm[r] = index of the box of rank r
    boxes, scores = np.empty((1, K, 7), F), np.empty((1, K), F)
    boxes[0, perm] = by_rank
    scores[0, perm] = ((K - g) / K).astype(F)                                    # exact, distinct, descending in rank
    perm.setflags(write=False)
    return boxes, scores, dict(perm=perm, pairs=tuple(pairs), chains=tuple(chains))


@functools.lru_cache(maxsize=None)
def case(name):
    """-> dict(boxes [B,K,D], scores [B,K], labels [B,K] or None, kw = dict(iou_thr, score_thr, pre_max, post_max))."""
    kind, _, arg = name.partition(":")
    kw = dict(iou_thr=IOU_THR, score_thr=0.0, pre_max=None, post_max=None)
    labels, extra = None, {}
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
        boxes, scores, labels, extra = _case_scores_and_stages(kind, arg, kw)
    for a in (boxes, scores) + (() if labels is None else (labels,)):
        a.setflags(write=False)
    return dict(boxes=boxes, scores=scores, labels=labels, kw=kw, **extra)


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


def _hits_above(name, b):
    """Scene b of a case with iou_thr >= 0 -> (kept flags in rank order, [for each rank q: the ranks above q whose box
    overlaps q's above the threshold]).  Only pairs close enough to touch are clipped (the module docstring's narrowing)."""
    c, want = case(name), expected(name)
    thr = F(c["kw"]["iou_thr"])
    assert thr >= 0
    r = rank_candidates(c["scores"][b], c["kw"]["score_thr"])
    b9 = rows9(c["boxes"][b][r])
    xy = b9[:, :2].astype(np.float64)
    rad = 0.5 * np.hypot(b9[:, 3].astype(np.float64), b9[:, 4].astype(np.float64))
    lab = None if c["labels"] is None else c["labels"][b][r]
    above = []
    for q in range(len(r)):
        near = np.nonzero(np.hypot(xy[:q, 0] - xy[q, 0], xy[:q, 1] - xy[q, 1]) <= rad[:q] + rad[q] + 1.0)[0]
        if lab is not None:
            near = near[lab[near] == lab[q]]
        if len(near):
            near = near[_oracle().iou_bev(b9[near], np.repeat(b9[q][None], len(near), 0)) > thr]
        above.append(near)
    return want[0][b][r].astype(bool), above


def chain_coverage(name, reach=64):
    """(boxes kept although a higher-ranked box overlaps them above the threshold — every such box was itself suppressed,
    boxes suppressed by a kept box more than `reach` ranks above them), counted on the reference's result of a case."""
    revived = far = 0
    for b in range(case(name)["scores"].shape[0]):
        kept, above = _hits_above(name, b)
        for q, a in enumerate(above):
            revived += bool(kept[q] and len(a) and not kept[a].any())
            far += bool(not kept[q] and (kept[a] & (q - a > reach)).any())
    return revived, far


def sole_reach(name, chunks):
    """Boxes whose EVERY kept suppressor lies more than `chunks` 64-rank chunks before their own chunk: a walk that dropped
    the words beyond that distance would keep them."""
    sole = 0
    for b in range(case(name)["scores"].shape[0]):
        kept, above = _hits_above(name, b)
        for q, a in enumerate(above):
            a = a[kept[a]]
            sole += bool(not kept[q] and len(a) and ((q >> 6) - (a >> 6) > chunks).all())
    return sole


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


# ---- coverage of the score regimes, the stage boundaries and the walk's reach ----------------------------------------
# Each cover_* asserts, on the REFERENCE, what its family exists for and returns the figures (the CPU and the GPU tests
# both call it; computed once per process).  If one fails, change the generator, never the condition.
def selected_n(scores, score_thr, pre_max=None):
    n = int((np.asarray(scores, F) >= F(score_thr)).sum())
    return n if pre_max is None else min(n, pre_max)


@functools.lru_cache(maxsize=None)
def cover_logits():
    c = case("logits")
    out = []
    for s in c["scores"]:
        assert (s < 0).all() and len(np.unique(s)) == len(s)
        sel = s[rank_candidates(s, c["kw"]["score_thr"])[:c["kw"]["pre_max"]]]
        prof = radix_profile(s, c["kw"]["score_thr"], c["kw"]["pre_max"])
        assert len(sel) == c["kw"]["pre_max"] and sel[-1] < 0 and len(np.unique(sel)) >= 100 and prof["decides"] == "key"
        assert (np.diff(sel) < 0).all()                                  # ranked by value, not by magnitude
        out.append(dict(pth=float(sel[-1]), distinct_selected=len(np.unique(sel)), shared=prof["shared"]))
    return out


@functools.lru_cache(maxsize=None)
def cover_mixed():
    c = case("mixed")
    out = []
    for s in c["scores"]:
        r = rank_candidates(s, NINF)
        pth = [float(s[r[p - 1]]) for p in MIXED_CUTS]
        zeros = s[s == 0]
        assert pth[0] > 0 and pth[1] == 0 and pth[2] < 0 and cut_inside_tie(s, NINF, MIXED_CUTS[1])
        assert np.signbit(zeros).any() and (~np.signbit(zeros)).any()
        out.append(dict(pth=pth, zeros=len(zeros), neg_zeros=int(np.signbit(zeros).sum())))
    return out


def wide_cuts():
    """pre_max values of `wide`, from scene 0: P-th score = FLT_MAX (directly below +Inf), a positive normal, a positive
    subnormal, a negative subnormal, -FLT_MAX (directly above -Inf)."""
    s = case("wide")["scores"][0]
    sr = s[rank_candidates(s, NINF)]
    tiny = np.finfo(F).tiny
    mid = lambda m: int(np.nonzero(m)[0][int(m.sum()) // 2]) + 1
    return (2, mid(sr >= tiny), mid((sr > 0) & (sr < tiny)), mid((sr < 0) & (sr > -tiny)), len(s) - 1)


@functools.lru_cache(maxsize=None)
def cover_wide():
    c, fi = case("wide"), np.finfo(F)
    tops = [len(np.unique(score_key_np(s) >> np.uint32(24))) for s in c["scores"]]
    assert min(tops) >= 200
    s = c["scores"][0]
    sr = s[rank_candidates(s, NINF)]
    pth = [float(sr[p - 1]) for p in wide_cuts()]
    assert len(sr) == len(s) and np.isposinf(sr[0]) and np.isneginf(sr[-1]) and np.isfinite(sr[1:-1]).all()
    assert pth[0] == fi.max and pth[1] >= fi.tiny and 0 < pth[2] < fi.tiny and -fi.tiny < pth[3] < 0 and pth[4] == -fi.max
    return dict(top_bytes=tops, cuts=wide_cuts(), pth=pth)


def ladder_cuts(name):
    """pre_max values that put the P-th key of scene 0 or 1 on the chain's last value below the carry, on the first one
    above it and inside the chain (q = 3: on both ends of the 256-value block and inside it)."""
    c = case(name)
    at = (0, 255, 100) if len(c["chain"]) == 256 else (159, 160, 50)
    cuts = set()
    for s, sign in zip(c["scores"], (0, 0x80000000)):
        for v in _bits(c["chain"][list(at)] | np.uint32(sign)):
            cuts.add(int((s > v).sum()) + 1)
    return tuple(sorted(cuts))


@functools.lru_cache(maxsize=None)
def cover_ladder():
    drops, zero, ff = set(), 0, 0
    for q in LADDER:
        name = f"ladder:{q}"
        c = case(name)
        step = _bits(c["chain"])
        assert (np.nextafter(step[:-1], F(np.inf)) == step[1:]).all()     # consecutive floats
        for s in c["scores"]:
            for p in ladder_cuts(name):
                prof = radix_profile(s, NINF, p)
                assert first_drop(prof, len(s)) == q
                drops.add(q)
                zero += 0 in key_bytes(prof)[1:]
                ff += 255 in key_bytes(prof)[1:]
    assert drops == {0, 1, 2, 3} and zero >= 1 and ff >= 1
    return dict(first_drop_passes=sorted(drops), thresholds_with_00=zero, thresholds_with_ff=ff)


@functools.lru_cache(maxsize=None)
def cover_runs():
    out = {}
    for pat in RUNS:
        c = case(f"runs:{pat}")
        K, P = c["scores"].shape[1], c["kw"]["pre_max"]
        for s in c["scores"]:
            sel = np.sort(rank_candidates(s, NINF)[:P])
            want = {"equal": np.arange(P), "asc": np.arange(K - P, K), "desc": np.arange(P)}.get(pat)
            if pat == "alt":
                want = np.nonzero(s == s.max())[0][:P]
            np.testing.assert_array_equal(sel, want)
        out[pat] = [int(v) for v in expected(f"runs:{pat}")[2]]
    return out


def threshold_values():
    """(tag, score_thr) of `thresholds`, from scene 0's maximum and its 300-th score."""
    s = case("thresholds")["scores"][0]
    sr = s[rank_candidates(s, NINF)]
    mx, tp, inf = sr[0], sr[299], F(np.inf)
    return (("above_max", np.nextafter(mx, inf)), ("max", mx), ("P_up", np.nextafter(tp, inf)), ("P", tp),
            ("P_dn", np.nextafter(tp, -inf)), ("pos_zero", F(0.0)), ("neg_logit", F(-3.0)), ("ninf", -inf), ("pinf", inf))


@functools.lru_cache(maxsize=None)
def cover_thresholds():
    s0, s1 = case("thresholds")["scores"]
    assert len(np.unique(s0[s0 != 0])) == (s0 != 0).sum() and np.isposinf(s1).sum() == 1 and np.isfinite(s0).all()
    tv = dict(threshold_values())
    n0 = {t: selected_n(s0, v) for t, v in tv.items()}
    n1 = {t: selected_n(s1, v) for t, v in tv.items()}
    assert 0 == n0["above_max"] < n0["max"] == 1 < n0["P_up"] == 299 < n0["P"] == 300 == n0["P_dn"]
    assert n0["P_dn"] < n0["pos_zero"] == 450 < n0["neg_logit"] < n0["ninf"] == 900 and n0["pinf"] == 0 and n1["pinf"] == 1
    assert np.signbit(s0[s0 == 0]).sum() == 50 and n1["above_max"] == 1
    decides = {t: radix_profile(s0, v, 300)["decides"] for t, v in tv.items()}
    assert decides["P_up"] == "thr" and decides["P"] == "key" and decides["P_dn"] == "key" and decides["above_max"] == "thr"
    return dict(n_scene0=n0, n_scene1=n1, decides=decides)


def n5000_thresholds():
    """score_thr that leaves exactly n candidates of `n5000` (its scores are distinct), for n in N5000."""
    d = np.sort(case("n5000")["scores"][0])[::-1]
    return tuple(float(d[n - 1]) for n in N5000)


@functools.lru_cache(maxsize=None)
def cover_stages():
    s = case("n5000")["scores"][0]
    assert len(np.unique(s)) == 5000
    for n, t in zip(N5000, n5000_thresholds()):
        assert selected_n(s, 0.0, n) == n and selected_n(s, t) == n
    share = {}
    for K in STRIDE_K:
        c = case(f"stride:{K}")
        assert selected_n(c["scores"][0], 0.0) == K
        share[K] = round(float(expected(f"stride:{K}")[2][0]) / K, 3)
        assert 0.2 < share[K] < 0.8
    c = case("batch37")
    n = [selected_n(s, c["kw"]["score_thr"], c["kw"]["pre_max"]) for s in c["scores"]]
    np.testing.assert_array_equal(n, c["n"])
    assert set(n) == set(BATCH37_N)
    return dict(stride_kept_share=share, n5000_kept=[int(expected("n5000", pre_max=n)[2][0]) for n in N5000], batch37_n=n)


def post_chunk_cuts():
    """post_max values of `post` at which scene 0's kept count reaches the cap exactly on the last rank of a 64-rank chunk,
    and on the first rank of a chunk (chunks >= 1)."""
    s = case("post")["scores"][0]
    kept = expected("post")[0][0][rank_candidates(s, 0.0)].astype(bool)
    cum = np.cumsum(kept)
    last = next(64 * c + 63 for c in range(1, len(kept) // 64) if kept[64 * c + 63])
    first = next(64 * c for c in range(1, len(kept) // 64) if kept[64 * c])
    return int(cum[last]), int(cum[first])


@functools.lru_cache(maxsize=None)
def cover_post_chunk():
    s = case("post")["scores"][0]
    r = rank_candidates(s, 0.0)
    where = []
    for post, lane in zip(post_chunk_cuts(), (63, 0)):
        order = expected("post", post_max=post)[1][0]
        assert order[-1] >= 0 and int(np.nonzero(r == order[-1])[0][0]) % 64 == lane      # the cap is reached, on that lane
        where.append(int(np.nonzero(r == order[-1])[0][0]))
    return dict(post_max=post_chunk_cuts(), rank_of_last_kept=where)


@functools.lru_cache(maxsize=None)
def cover_far():
    c, want = case("far"), expected("far")
    thr = F(c["kw"]["iou_thr"])
    kept = want[0][0][c["perm"]].astype(bool)                            # in rank order
    b9 = rows9(c["boxes"][0][c["perm"]])
    iou = lambda p, q: float(_oracle().iou_bev(b9[p][None], b9[q][None])[0])
    assert int((~kept).sum()) == len(c["pairs"]) + len(c["chains"])       # the copies and the chains' middle boxes, nothing else
    gaps = []
    for r, q in c["pairs"]:
        assert kept[r] and not kept[q] and iou(r, q) > thr
        gaps.append((q >> 6) - (r >> 6))
    assert sorted(set(q - r for r, q in c["pairs"])) == sorted(FAR_D)
    assert max(gaps) >= 200 and any(17 <= g <= 64 for g in gaps)
    assert sum(r < 64 for r, _ in c["pairs"]) >= 3 and sum(r >= 6400 for r, _ in c["pairs"]) >= 3
    revived = 0
    for a, b, d in c["chains"]:
        assert kept[a] and not kept[b] and kept[d] and iou(a, b) > thr and iou(b, d) > thr and not iou(a, d) > thr
        assert (b >> 6) - (a >> 6) > 16 and (d >> 6) - (b >> 6) > 16
        revived += 1
    return dict(suppressed=int((~kept).sum()), chunk_gaps=sorted(gaps), revived=revived, kept=int(want[2][0]))


@functools.lru_cache(maxsize=None)
def cover_crowded4k():
    out = {}
    for name in ("crowded4k", "crowded4k:classes"):
        K = case(name)["scores"].shape[1]
        share = float(expected(name)[2][0]) / K
        revived, far = chain_coverage(name, reach=16 * 64)
        sole = sole_reach(name, 16)
        assert selected_n(case(name)["scores"][0], 0.0) == K and 0.2 < share < 0.8 and revived >= 1 and far >= 1 and sole >= 1
        out[name] = dict(kept_share=round(share, 3), revived=revived, suppressed_from_over_16_chunks=far, only_from_over_16_chunks=sole)
    assert not np.array_equal(expected("crowded4k")[0], expected("crowded4k:classes")[0])
    return out
