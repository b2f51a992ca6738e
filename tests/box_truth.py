"""The truth of the rotated-box operators (SPEC.md §13, §19.3, §23, §28): plain numpy / Python binary64, no code shared with the
oracle, tests/box_ref.py or the kernels, and the case families on which the float32 implementations are held against it.

Truth is defined on the STORED float32 box rows.  Corners come from np.sin / np.cos of the yaw widened to float64; both boxes of
a pair are translated by -b.centre in float64 before the Sutherland-Hodgman clip and the shoelace sum, so the truth has no
cancellation of its own however far from the origin the scene lies.

Every centre the builders make lies on a 1/16 m lattice, so a scene translates EXACTLY (in float32) to every offset of OFFSETS
(all below 2^20 m): an implementation whose pair test works on centre differences returns the same bits at every offset."""
import numpy as np

F = np.float32
LATTICE = 0.0625
OFFSETS = ((0.0, 0.0), (70.0, -40.0), (1000.0, 1000.0), (1e5, -1e5), (1e6, 1e6))
PAIR_FAMILIES = ("perturbed", "yaw_step", "identical", "nested", "edge", "far", "yaw1e3")
SIZE_FAMILIES = {"object": (0.3, 12.0), "thin": (0.05, 10.0)}

# tol(a, b) = C_TOL * 2^-24 * (D_a + D_b)^2 / min(l_a w_a, l_b w_b), D = hypot(l, w): one float32 rounding of a coordinate of
# size D_a + D_b (the extent of the pair in b's frame) moves the clipped area by about 2^-24 (D_a + D_b)^2, and the IoU by that
# over the smaller area.  C_TOL = 4 x the largest err / (2^-24 (D_a + D_b)^2 / min area) of the CPU oracle's iou_bev and of
# box_ref.iou3d_matrix over every pair family x size family x offset below.
# Measured (tests/test_box_truth_cpu.py::test_tol_constant prints it and fails above C_TOL / 2): 1.28, the same at every offset.
C_MEASURED = 1.28
C_TOL = 4.0 * C_MEASURED
OBJECT_ABS_CAP = 1e-5          # on the object family the absolute error is below this, whatever C_TOL is


# ---- geometry ------------------------------------------------------------------------------------------------
def _local_corners(boxes):
    """[K,D] float32 rows -> [K,4,2] float64 corner offsets from the box's own centre, counter-clockwise."""
    b = np.asarray(boxes, F).astype(np.float64)
    c, s = np.cos(b[:, 6]), np.sin(b[:, 6])
    hl, hw = b[:, 3] / 2, b[:, 4] / 2
    dx = np.stack([hl, -hl, -hl, hl], 1)
    dy = np.stack([hw, hw, -hw, -hw], 1)
    return np.stack([c[:, None] * dx - s[:, None] * dy, s[:, None] * dx + c[:, None] * dy], 2)


def _clip_area(poly, quad):
    """Area of polygon `poly` (list of (x, y) Python floats) clipped to the convex quad `quad`, both counter-clockwise."""
    for e in range(4):
        q0x, q0y = quad[e]
        q1x, q1y = quad[(e + 1) & 3]
        ex, ey = q1x - q0x, q1y - q0y
        out = []
        px, py = poly[-1]
        cp = ex * (py - q0y) - ey * (px - q0x)
        for cx, cy in poly:
            cc = ex * (cy - q0y) - ey * (cx - q0x)
            if (cc >= 0.0) != (cp >= 0.0):
                t = cp / (cp - cc)
                out.append((px + t * (cx - px), py + t * (cy - py)))
            if cc >= 0.0:
                out.append((cx, cy))
            px, py, cp = cx, cy, cc
        poly = out
        if not poly:
            return 0.0
    if len(poly) < 3:
        return 0.0
    sm = 0.0
    for i in range(len(poly)):
        xi, yi = poly[i]
        xj, yj = poly[(i + 1) % len(poly)]
        sm += xi * yj - xj * yi
    return 0.5 * abs(sm)


def _inter64(a, la, b, lb):
    """Clipped area of the pair (box rows a, b as float64; local corners la, lb) in b's frame."""
    dx, dy = float(a[0] - b[0]), float(a[1] - b[1])
    return _clip_area([(dx + x, dy + y) for x, y in la.tolist()], [(x, y) for x, y in lb.tolist()])


def _iou_of(inter, a, b, mode):
    if mode == "bev":
        den = a[3] * a[4] + b[3] * b[4] - inter
        return inter / den if den > 0 else 0.0
    top = min(a[2] + a[5] / 2, b[2] + b[5] / 2)
    bot = max(a[2] - a[5] / 2, b[2] - b[5] / 2)
    i3 = inter * max(top - bot, 0.0)
    den = a[3] * a[4] * a[5] + b[3] * b[4] * b[5] - i3
    return i3 / den if den > 0 else 0.0


def _pairs64(a, b, mode):
    a, b = np.atleast_2d(np.asarray(a, F)), np.atleast_2d(np.asarray(b, F))
    assert a.shape[0] == b.shape[0]
    la, lb = _local_corners(a), _local_corners(b)
    a64, b64 = a.astype(np.float64), b.astype(np.float64)
    return np.array([_iou_of(_inter64(a64[i], la[i], b64[i], lb[i]), a64[i], b64[i], mode) for i in range(a.shape[0])], np.float64)


def _matrix64(a, b, mode):
    a, b = np.asarray(a, F), np.asarray(b, F)
    la, lb = _local_corners(a), _local_corners(b)
    a64, b64 = a.astype(np.float64), b.astype(np.float64)
    out = np.empty((a.shape[0], b.shape[0]), np.float64)
    for i in range(a.shape[0]):
        for j in range(b.shape[0]):
            out[i, j] = _iou_of(_inter64(a64[i], la[i], b64[j], lb[j]), a64[i], b64[j], mode)
    return out


def iou_bev64(a, b):
    """True BEV IoU of the paired float32 rows a[i], b[i] ([N,D >= 7] each, or single rows) -> [N] float64."""
    return _pairs64(a, b, "bev")


def iou3d64(a, b):
    """True 3-D IoU (§19.3: BEV intersection x height overlap over the union of the volumes) of paired rows -> [N] float64."""
    return _pairs64(a, b, "3d")


def iou_bev64_matrix(a, b):
    """a [Ka,D], b [Kb,D] -> [Ka,Kb] float64, entry [i,j] = true BEV IoU of (a_i, b_j)."""
    return _matrix64(a, b, "bev")


def iou3d64_matrix(a, b):
    return _matrix64(a, b, "3d")


def _iou_float64(a, b):
    """Independent restatement in the GLOBAL frame: float64 corners from numpy sin/cos + Sutherland-Hodgman (the check of
    tests/test_oracle.py near the origin; iou_bev64 above is the one that holds at any distance)."""
    def corners(q):
        c, s = np.cos(np.float64(q[6])), np.sin(np.float64(q[6]))
        d = np.array([[1, 1], [-1, 1], [-1, -1], [1, -1]], np.float64) * np.array([q[3], q[4]], np.float64) / 2
        return np.stack([q[0] + c * d[:, 0] - s * d[:, 1], q[1] + s * d[:, 0] + c * d[:, 1]], 1)
    poly, clip = corners(a), corners(b)
    for e in range(4):
        q0, q1 = clip[e], clip[(e + 1) % 4]
        out = []
        for i in range(len(poly)):
            cur, prev = poly[i], poly[i - 1]
            cc = (q1[0] - q0[0]) * (cur[1] - q0[1]) - (q1[1] - q0[1]) * (cur[0] - q0[0])
            cp = (q1[0] - q0[0]) * (prev[1] - q0[1]) - (q1[1] - q0[1]) * (prev[0] - q0[0])
            if (cc >= 0) != (cp >= 0):
                out.append(prev + cp / (cp - cc) * (cur - prev))
            if cc >= 0:
                out.append(cur)
        poly = np.array(out) if out else np.zeros((0, 2))
        if len(poly) == 0:
            break
    inter = 0.0
    if len(poly) >= 3:
        x, y = poly[:, 0], poly[:, 1]
        inter = 0.5 * abs(np.sum(x * np.roll(y, -1) - np.roll(x, -1) * y))
    return inter / (a[3] * a[4] + b[3] * b[4] - inter)


def tol(a, b):
    """The float32 error bound of one pair (see C_TOL); broadcasts over leading axes of the box rows."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    d = np.hypot(a[..., 3], a[..., 4]) + np.hypot(b[..., 3], b[..., 4])
    return C_TOL * 2.0 ** -24 * d * d / np.minimum(a[..., 3] * a[..., 4], b[..., 3] * b[..., 4])


def tol_matrix(a, b):
    return tol(np.asarray(a)[..., :, None, :], np.asarray(b)[..., None, :, :])


# ---- greedy NMS on the truth -----------------------------------------------------------------------------------
def nms64(boxes, scores, thr, score_thr=-np.inf, labels=None, pre_max=None, post_max=None):
    """The greedy rule of §13 / §23 on iou_bev64, one scene.  boxes [K,D >= 7] f32, scores [K] f32 ->
    (keep [K] int32, order list of kept indices in rank order, near): candidates (score >= score_thr) ranked by (score desc,
    index asc), cut to the first pre_max; a box is kept iff no kept box of higher rank (and the same label, when labels are
    given) has iou_bev64(kept, box) > thr (strict); the walk stops at post_max kept boxes.  `near` counts the pairs of ranked
    boxes (same label) whose true IoU lies within tol of thr: with near == 0 every correct float32 implementation must make the
    same decisions.  Pairs further apart than the sum of their half diagonals are skipped: their IoU is exactly 0."""
    boxes = np.asarray(boxes, F)
    scores = np.asarray(scores, F)
    K = boxes.shape[0]
    cand = [i for i in range(K) if scores[i] >= F(score_thr)]
    cand.sort(key=lambda i: (-float(scores[i]), i))
    if pre_max is not None:
        cand = cand[:pre_max]
    rb = boxes[cand]
    n = len(cand)
    loc = _local_corners(rb) if n else np.zeros((0, 4, 2))
    b64 = rb.astype(np.float64)
    half = 0.5 * np.hypot(b64[:, 3], b64[:, 4])
    lab = None if labels is None else np.asarray(labels)[cand]
    sup = [[] for _ in range(n)]                 # sup[p]: the ranks q > p that p suppresses
    near = 0
    for p in range(n):
        dist = np.hypot(b64[p + 1:, 0] - b64[p, 0], b64[p + 1:, 1] - b64[p, 1])
        for q in (np.flatnonzero(dist <= half[p] + half[p + 1:]) + p + 1).tolist():
            if lab is not None and lab[p] != lab[q]:
                continue
            v = _iou_of(_inter64(b64[p], loc[p], b64[q], loc[q]), b64[p], b64[q], "bev")
            if abs(v - thr) <= tol(rb[p], rb[q]):
                near += 1
            if v > thr:
                sup[p].append(q)
    keep = np.zeros(K, np.int32)
    order = []
    dead = np.zeros(n, bool)
    for p in range(n):
        if dead[p]:
            continue
        if post_max is not None and len(order) >= post_max:
            break
        order.append(cand[p])
        keep[cand[p]] = 1
        dead[sup[p]] = True
    return keep, order, near


# ---- case builders ---------------------------------------------------------------------------------------------
def _snap(v):
    return np.round(np.asarray(v, np.float64) / LATTICE) * LATTICE


def _sizes(rng, n, family):
    lo, hi = SIZE_FAMILIES[family]
    return np.exp(rng.uniform(np.log(lo), np.log(hi), (n, 2)))


def base_boxes(rng, n, family, extent=8.0):
    """[n,7] float32: centres and z on the lattice within +-extent / +-2 m, l, w log-uniform in the family's range, h on the lattice
    in [1/16, 4], yaw uniform in +-pi."""
    a = np.zeros((n, 7), np.float64)
    a[:, 0:2] = _snap(rng.uniform(-extent, extent, (n, 2)))
    a[:, 2] = _snap(rng.uniform(-2, 2, n))
    a[:, 3:5] = _sizes(rng, n, family)
    a[:, 5] = np.maximum(_snap(rng.uniform(0, 4, n)), LATTICE)
    a[:, 6] = rng.uniform(-np.pi, np.pi, n)
    return a.astype(F)


def apply_family(kind, a, rng):
    """(a', b) with b = f(a') of one pair family; a' is a but for the families that constrain it (edge: yaw 0 and l on the lattice;
    yaw1e3: yaw near 1e3)."""
    a = np.array(a, F, copy=True)
    n = a.shape[0]
    if kind == "yaw1e3":
        a[:, 6] = (1000.0 + rng.uniform(-np.pi, np.pi, n)).astype(F)
    if kind == "edge":
        a[:, 6] = 0
        a[:, 3] = np.maximum(_snap(a[:, 3]), LATTICE)                 # l on the lattice, so that a.x + l is a lattice centre
    b = a.copy()
    if kind in ("perturbed", "yaw1e3"):
        b[:, 0:2] = a[:, 0:2] + (rng.integers(-8, 9, (n, 2)) * LATTICE).astype(F)
        b[:, 2] = a[:, 2] + (rng.integers(-8, 9, n) * LATTICE).astype(F)
        b[:, 6] = a[:, 6] + rng.uniform(-0.5, 0.5, n).astype(F)
        b[:, 3:5] = a[:, 3:5] * rng.uniform(0.9, 1.1, (n, 2)).astype(F)
    elif kind == "yaw_step":
        steps = np.array([1e-4, -1e-4, 1e-6, -1e-6, np.pi / 2, np.pi])
        b[:, 6] = (a[:, 6].astype(np.float64) + steps[np.arange(n) % len(steps)]).astype(F)
    elif kind == "nested":
        b[:, 3:5] = a[:, 3:5] * rng.uniform(0.8, 1.2, (n, 1)).astype(F)
    elif kind == "edge":
        b[:, 0] = a[:, 0] + a[:, 3]
    elif kind == "far":
        ang = rng.integers(0, 8, n) * (np.pi / 4)
        b[:, 0:2] = a[:, 0:2] + np.round(np.stack([np.cos(ang), np.sin(ang)], 1) * 100).astype(F)
        b[:, 6] = rng.uniform(-np.pi, np.pi, n).astype(F)
    return a, b


def pair_family(kind, family, n, seed, extent=8.0):
    """(a, b) float32 [n,7] at offset 0, b = f(a), of one pair family (PAIR_FAMILIES) and size family (SIZE_FAMILIES); the
    centres of a lie within +-extent."""
    rng = np.random.default_rng([seed, PAIR_FAMILIES.index(kind), sorted(SIZE_FAMILIES).index(family)])
    return apply_family(kind, base_boxes(rng, n, family, extent), rng)


def translate(boxes, off):
    """The boxes moved by off = (ox, oy) in float32 (exact for the builders' lattice centres and every offset of OFFSETS)."""
    out = np.array(boxes, F, copy=True)
    out[..., 0] = out[..., 0] + F(off[0])
    out[..., 1] = out[..., 1] + F(off[1])
    return out


def is_exact_translation(boxes, off):
    """True iff translate(boxes, off) moved every centre exactly (float32 sum == float64 sum)."""
    t = translate(boxes, off).astype(np.float64)
    b = np.asarray(boxes, F).astype(np.float64)
    return bool((t[..., 0] == b[..., 0] + off[0]).all() and (t[..., 1] == b[..., 1] + off[1]).all())


def nms_scene(K, seed, family="object", extent=60.0):
    """[K,7] float32 boxes in clusters of 3 - 8 perturbed copies (lattice centres) and [K] distinct float32 scores."""
    rng = np.random.default_rng([seed, K])
    out = np.zeros((K, 7), np.float64)
    k = 0
    while k < K:
        m = min(int(rng.integers(3, 9)), K - k)
        base = base_boxes(rng, 1, family, extent)[0].astype(np.float64)
        base[3:5] = np.clip(base[3:5], 1.0, 6.0) if family == "object" else base[3:5]
        out[k:k + m] = base
        # half the copies are tight (they overlap the cluster's first box by more than 0.5), the others loose (around 0.1)
        loose = (rng.random(m) < 0.5)[:, None]
        shift = np.where(loose, rng.uniform(-0.9, 0.9, (m, 2)) * base[3:5].max(), rng.uniform(-0.15, 0.15, (m, 2)) * base[3:5].min())
        out[k:k + m, 0:2] += _snap(shift)
        out[k:k + m, 3:5] *= np.where(loose, rng.uniform(0.85, 1.15, (m, 2)), rng.uniform(0.93, 1.07, (m, 2)))
        out[k:k + m, 6] += np.where(loose[:, 0], rng.uniform(-0.4, 0.4, m), rng.uniform(-0.08, 0.08, m))
        k += m
    scores = (rng.permutation(K) + 1).astype(np.float64) / (K + 1)          # distinct
    perm = rng.permutation(K)                                                # clusters scattered over the index range
    return out[perm].astype(F), scores.astype(F)


def matrix_boxes(Ka, Kb, seed, group=16):
    """a [Ka,7], b [Kb,7] for a pairwise matrix.  The rows come in groups of `group` tight copies of one anchor box (centre moved by
    up to a tenth of its smaller side, on the lattice; yaw +-0.15; sizes +-5 %), the size family alternating from group to group,
    so a group's block of the matrix holds large overlaps and the rest mostly none; b_i = f(a_i) with the pair family i mod 7, so the
    diagonal holds the pair families."""
    n = max(Ka, Kb)
    rng = np.random.default_rng([seed, Ka, Kb])
    A = np.zeros((n, 7), F)
    fams = sorted(SIZE_FAMILIES)
    for g0 in range(0, n, group):
        m = min(group, n - g0)
        anchor = base_boxes(rng, 1, fams[(g0 // group) % 2])[0].astype(np.float64)
        rows = np.repeat(anchor[None], m, 0)
        rows[:, 0:2] += _snap(rng.uniform(-0.1, 0.1, (m, 2)) * anchor[3:5].min())
        rows[:, 2] += rng.integers(-2, 3, m) * LATTICE
        rows[:, 3:5] *= rng.uniform(0.95, 1.05, (m, 2))
        rows[:, 6] += rng.uniform(-0.15, 0.15, m)
        A[g0:g0 + m] = rows
    Bm = np.zeros((n, 7), F)
    for k, kind in enumerate(PAIR_FAMILIES):
        A[k::len(PAIR_FAMILIES)], Bm[k::len(PAIR_FAMILIES)] = apply_family(kind, A[k::len(PAIR_FAMILIES)], rng)
    return A[:Ka].copy(), Bm[:Kb].copy()


def roi_scene(R, G, seed):
    """One scene for roi_targets: gt [G,7] boxes on a 24 m grid (lattice centres, z and h on the lattice), rois [R,7]: three in four
    are perturbed copies of a box (lattice shifts up to 0.5 m, yaw +-0.3, sizes +-10 %), the others background: a copy pushed
    along its box's heading until it overlaps it only a little, and every eighth RoI far from every box (IoU exactly 0)."""
    rng = np.random.default_rng([seed, R, G])
    gt = base_boxes(rng, G, "object")
    gt[:, 3:5] = np.clip(gt[:, 3:5], 1.5, 6.0)
    cells = rng.permutation(16)[:G]
    gt[:, 0] = ((cells % 4) * 24 - 36).astype(F) + gt[:, 0] / 8
    gt[:, 1] = ((cells // 4) * 24 - 36).astype(F) + gt[:, 1] / 8
    gt[:, 0:2] = _snap(gt[:, 0:2]).astype(F)
    src = rng.integers(0, G, R)
    rois = gt[src].copy()
    rois[:, 0:2] += (rng.integers(-8, 9, (R, 2)) * LATTICE).astype(F)
    rois[:, 2] += (rng.integers(-4, 5, R) * LATTICE).astype(F)
    rois[:, 3:6] *= rng.uniform(0.9, 1.1, (R, 3)).astype(F)
    rois[:, 6] += rng.uniform(-0.3, 0.3, R).astype(F)
    bg = np.arange(R) % 4 == 3
    push = _snap(0.8 * gt[src, 3:4] * np.stack([np.cos(gt[src, 6]), np.sin(gt[src, 6])], 1))
    rois[bg, 0:2] = (gt[src[bg], 0:2] + push[bg]).astype(F)
    far = np.arange(R) % 8 == 7
    rois[far, 0:2] = gt[src[far], 0:2] + F(12)
    return rois, gt, src


def coverage(truth):
    """Asserts that a set of true IoUs contains the cases a clip can get wrong: >= 10 % zero, >= 10 % positive, >= 5 % above 0.5."""
    v = np.concatenate([np.ravel(t) for t in truth])
    zero, pos, high = (v == 0).mean(), (v > 0).mean(), (v > 0.5).mean()
    print(f"true IoU entries: {v.size}, zero {zero:.3f}, positive {pos:.3f}, above 0.5 {high:.3f}")
    assert zero >= 0.10 and pos >= 0.10 and high >= 0.05
