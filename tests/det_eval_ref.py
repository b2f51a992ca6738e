"""float32 numpy reference of SPEC.md §36 (detection evaluation): ``det_match`` and ``det_ap`` in the spec's operation order,
every scalar an np.float32.  The pair value of the IoU metrics is tests/box_ref.py's bit-exact clip (pair_inter on the corner
lists), computed for the pairs the rule reads only (a live detection and a valid box of its class): the scalar clip does about
1e4 pairs a second.  ``CASES`` / ``case`` / ``expected`` are the matching cases, ``AP_CASES`` / ``ap_case`` / ``ap_expected`` the AP
ones; ``coverage(name)`` names what a case demonstrably contains, ``CLAIMS`` what each case is there for
(tests/test_det_eval_cpu.py asserts the one on the other)."""
import functools

import numpy as np

import box_ref

F = np.float32
ZERO, HALF = F(0.0), F(0.5)
OUTPUTS = ("code", "match", "value", "gt_det", "n_gt")
AP_OUTPUTS = ("ap", "prec", "max_recall", "n_det")
PRESETS = {"kitti_r40": (40, 1, 0.0), "kitti_r11": (10, 0, 0.0), "nuscenes": (100, 11, 0.1)}


# ---- det_match ----------------------------------------------------------------------------------------------------------------
def live_mask(c, b):
    K, C = c["det_labels"].shape[1], c["thr"].shape[0]
    n = K if c["det_count"] is None else min(max(int(c["det_count"][b]), 0), K)
    lab = c["det_labels"][b]
    return (np.arange(K) < n) & (lab >= 0) & (lab < C)


def rank_order(scores, live):
    """§23: the live indices by (score descending, index ascending), scores compared as floats (-0 and +0 tie)."""
    return sorted(np.flatnonzero(live).tolist(), key=lambda i: (-float(scores[i]), i))


def _iou_value(a, ca, b, cb, metric):
    inter = box_ref.pair_inter(a, ca, b, cb)
    if metric == "iou_bev":
        den = (a[3] * a[4] + b[3] * b[4]) - inter
        return inter / den if den > ZERO else ZERO
    ha, hb = HALF * a[5], HALF * b[5]
    oh = min(a[2] + ha, b[2] + hb) - max(a[2] - ha, b[2] - hb)
    oh = oh if oh > ZERO else ZERO
    i3 = inter * oh
    den = ((a[3] * a[4]) * a[5] + (b[3] * b[4]) * b[5]) - i3
    return i3 / den if den > ZERO else ZERO


def pair_values(c, b):
    """[K,G] f32: the pair value of (live detection k, valid box g of its class), NaN for every pair the rule does not read."""
    K, G, C = c["det_boxes"].shape[1], c["gt_boxes"].shape[1], c["thr"].shape[0]
    vals = np.full((K, G), np.nan, F)
    if G == 0:
        return vals
    live, glab = live_mask(c, b), c["gt_labels"][b]
    gvalid = (glab >= 0) & (glab < C)
    ks, gs = np.flatnonzero(live), np.flatnonzero(gvalid)
    det, gt = c["det_boxes"][b].astype(F), c["gt_boxes"][b].astype(F)
    if c["metric"] == "dist":
        dx = det[ks, None, 0] - gt[None, gs, 0]
        dy = det[ks, None, 1] - gt[None, gs, 1]
        v = np.sqrt((dx * dx) + (dy * dy))
        same = c["det_labels"][b][ks, None] == glab[None, gs]
        vals[np.ix_(ks, gs)] = np.where(same, v, np.nan)
        return vals
    cd = dict(zip(ks.tolist(), box_ref._corner_list(det[ks]))) if ks.size else {}
    cg = dict(zip(gs.tolist(), box_ref._corner_list(gt[gs]))) if gs.size else {}
    for k in ks.tolist():
        for g in gs[glab[gs] == c["det_labels"][b][k]].tolist():
            vals[k, g] = _iou_value(det[k], cd[k], gt[g], cg[g], c["metric"])
    return vals


def walk(vals, order, dlab, glab, gign, thr_c, t, dist, K, G):
    """One threshold column of one scene -> (code [K], match [K], value [K], gt_det [G]); rows that are not live keep (-1, -1, 0)."""
    code, match, value = np.full(K, -1, np.int32), np.full(K, -1, np.int32), np.zeros(K, F)
    gt_det = np.full(G, -1, np.int32)
    taken = np.zeros(G, bool)
    better = (lambda v, w: v < w) if dist else (lambda v, w: v > w)
    for k in order:
        cls = dlab[k]
        th = thr_c[cls, t]
        best, besti = -1, -1
        for g in np.flatnonzero(glab == cls).tolist():
            v = vals[k, g]
            if not (v < th if dist else v > th):
                continue
            if gign[g]:
                if besti < 0 or better(v, vals[k, besti]):
                    besti = g
            elif not taken[g] and (best < 0 or better(v, vals[k, best])):
                best = g
        if best >= 0:
            code[k], match[k], value[k] = 1, best, vals[k, best]
            taken[best] = True
            gt_det[best] = k
        elif besti >= 0:
            code[k], match[k], value[k] = -1, besti, vals[k, besti]
        else:
            code[k], match[k], value[k] = 0, -1, ZERO
    return code, match, value, gt_det


def det_match(c, vals=None):
    """c = dict(det_boxes, det_scores, det_labels, det_count | None, gt_boxes, gt_labels, gt_ignore | None, thr [C,T], metric) ->
    dict(code, match, value [B,K,T], gt_det [B,G,T], n_gt [B,C], vals [B,K,G])."""
    B, K = c["det_labels"].shape
    G, (C, T) = c["gt_labels"].shape[1], c["thr"].shape
    out = dict(code=np.empty((B, K, T), np.int32), match=np.empty((B, K, T), np.int32), value=np.empty((B, K, T), F),
               gt_det=np.empty((B, G, T), np.int32), n_gt=np.zeros((B, C), np.int32), vals=np.empty((B, K, G), F))
    for b in range(B):
        v = pair_values(c, b) if vals is None else vals[b]
        out["vals"][b] = v
        glab = c["gt_labels"][b]
        gign = np.zeros(G, bool) if c["gt_ignore"] is None else c["gt_ignore"][b] != 0
        order = rank_order(c["det_scores"][b], live_mask(c, b))
        for t in range(T):
            out["code"][b, :, t], out["match"][b, :, t], out["value"][b, :, t], out["gt_det"][b, :, t] = walk(
                v, order, c["det_labels"][b], glab, gign, c["thr"], t, c["metric"] == "dist", K, G)
        for cls in range(C):
            out["n_gt"][b, cls] = int(((glab == cls) & ~gign).sum())
    return out


# ---- det_ap -------------------------------------------------------------------------------------------------------------------
def det_ap(scores, labels, code, n_gt, points=40, first=1, floor=0.0):
    """scores [N] f32, labels [N] i32, code [N,T] i32, n_gt [C] i32 -> dict(ap [C,T], prec [C,T,P], max_recall [C,T], n_det [C,T])."""
    C, T, P = n_gt.shape[0], code.shape[1], points - first + 1
    ap, prec = np.empty((C, T), F), np.zeros((C, T, P), F)
    max_recall, n_det = np.zeros((C, T), F), np.zeros((C, T), np.int32)
    fl = F(floor)
    for c in range(C):
        for t in range(T):
            # (the rows that count are picked before they are ordered: a dead row rides along with whatever score bits it holds, NaN included)
            rows = sorted(np.flatnonzero((labels == c) & (code[:, t] != -1)).tolist(), key=lambda i: (-float(scores[i]), i))
            cd = code[rows, t] if rows else np.zeros(0, np.int32)
            n_det[c, t] = cd.size
            if n_gt[c] == 0:
                ap[c, t] = F(-1.0)
                continue
            tp, fp = np.cumsum(cd == 1), np.cumsum(cd == 0)
            rec = tp.astype(F) / F(n_gt[c])
            pr = tp.astype(F) / (tp + fp).astype(F)
            env = np.maximum.accumulate(pr[::-1])[::-1]
            sm = ZERO
            for k in range(first, points + 1):
                hit = np.flatnonzero(rec >= F(k) / F(points))
                s = env[hit[0]] if hit.size else ZERO
                prec[c, t, k - first] = s
                sm = sm + max(s - fl, ZERO)
            ap[c, t] = sm / (F(P) * (F(1.0) - fl))
            max_recall[c, t] = rec[-1] if rec.size else ZERO
    return dict(ap=ap, prec=prec, max_recall=max_recall, n_det=n_det)


def evaluate(cases, points=40, first=1, floor=0.0):
    """What DetectionEval computes over a list of matching cases of one configuration: the rows of all, scene-major, then det_ap."""
    outs = [det_match(c) for c in cases]
    T = cases[0]["thr"].shape[1]
    res = det_ap(np.concatenate([c["det_scores"].reshape(-1) for c in cases]), np.concatenate([c["det_labels"].reshape(-1) for c in cases]),
                 np.concatenate([o["code"].reshape(-1, T) for o in outs]), sum(o["n_gt"].sum(0) for o in outs).astype(np.int32),
                 points, first, floor)
    res["n_gt"] = sum(o["n_gt"].sum(0) for o in outs).astype(np.int32)
    return res


# ---- matching cases -----------------------------------------------------------------------------------------------------------
def _seed(name):
    return int.from_bytes(name.encode(), "little") % (2 ** 31)


def _gt(rng, G, C, D=8):
    """G boxes of car-like extents on a 12 m grid (no two overlap), any yaw; rows of D fields (those beyond 7 unread)."""
    gt = np.zeros((G, D), np.float64)
    i = np.arange(G)
    gt[:, 0] = 12.0 * (i % 32) + rng.uniform(-1, 1, G)
    gt[:, 1] = 12.0 * (i // 32) + rng.uniform(-1, 1, G)
    gt[:, 2] = rng.uniform(-1.5, 0.0, G)
    gt[:, 3:6] = np.array([3.9, 1.6, 1.56]) * rng.uniform(0.8, 1.25, (G, 3))
    gt[:, 6] = rng.uniform(-3.5, 3.5, G)
    gt[:, 7:] = 77.0
    return gt, rng.integers(0, C, G).astype(np.int32)


def _dets_near(rng, gt, lab, K, D, C, wrong=0.1):
    """K detections: half a small jitter of a random box (IoU about 0.7 and above), three in ten shifted 0.2 .. 0.6 lengths along it,
    the rest 50 m and more to the side; one in ten carries another class than the box it stands on.  Distinct scores in (0, 1)."""
    det, dl = np.zeros((K, D), np.float64), np.zeros(K, np.int32)
    G = len(gt)
    for k in range(K):
        g = int(rng.integers(0, G))
        box = gt[g, :7].copy()
        along = np.array([np.cos(box[6]), np.sin(box[6])])
        u = rng.random()
        if u < 0.5:
            box[:3] += rng.uniform(-0.06, 0.06, 3)
            box[3:6] *= rng.uniform(0.97, 1.03, 3)
            box[6] += rng.uniform(-0.03, 0.03)
        elif u < 0.8:
            box[:2] += along * box[3] * rng.uniform(0.2, 0.6) * rng.choice([-1, 1])
        else:
            box[1] += 500.0 + rng.uniform(0, 20)
        det[k, :7], dl[k] = box, lab[g] if rng.random() >= wrong else (lab[g] + 1) % C
    det[:, 7:] = -5.0
    scores = rng.permutation(K).astype(np.float64) / K + 0.5 / K
    return det, scores, dl


def _make(det, scores, dl, count, gt, gl, ign, thr, metric):
    return dict(det_boxes=np.asarray(det, F), det_scores=np.asarray(scores, F), det_labels=np.asarray(dl, np.int32),
                det_count=None if count is None else np.asarray(count, np.int32), gt_boxes=np.asarray(gt, F),
                gt_labels=np.asarray(gl, np.int32), gt_ignore=None if ign is None else np.asarray(ign, np.int32),
                thr=np.asarray(thr, F), metric=metric)


IOU_THR = [[0.7, 0.5], [0.5, 0.25], [0.5, 0.25]]
DIST_THR = [[0.5, 2.0], [0.5, 1.0], [1.0, 4.0]]


def _scenes(name, B, K, G, C=3, D=7, Dg=8, metric="iou3d", thr=None, ignore=False, wrong=0.1):
    rng = np.random.default_rng(_seed(name))
    det, sc, dl = np.zeros((B, K, D)), np.zeros((B, K)), np.zeros((B, K), np.int32)
    gt, gl = np.zeros((B, G, Dg)), np.zeros((B, G), np.int32)
    for b in range(B):
        gt[b], gl[b] = _gt(rng, G, C, Dg)
        det[b], sc[b], dl[b] = _dets_near(rng, gt[b], gl[b], K, D, C, wrong)
    ign = (rng.random((B, G)) < 0.25).astype(np.int32) if ignore else None
    if thr is None:
        thr = (DIST_THR if metric == "dist" else IOU_THR)[:C]
    return _make(det, sc, dl, None, gt, gl, ign, thr, metric)


def _counts():
    c = _scenes("counts", 4, 33, 9, D=9, ignore=True)
    c["det_count"] = np.array([0, 1, 33, 40], np.int32)             # (40: clamped to K)
    c["det_boxes"][0], c["det_boxes"][1, 1:] = np.nan, np.nan       # the rows beyond the count are never read
    c["det_scores"][0], c["det_scores"][1, 1:] = np.nan, np.nan
    c["det_labels"][0] = 1
    return c


def _g0():
    c = _scenes("g0", 2, 17, 4)
    c["gt_boxes"], c["gt_labels"] = np.zeros((2, 0, 7), F), np.zeros((2, 0), np.int32)
    return c


def _classes():
    """C = 4: class 2 has no ground truth, class 3 no detections; labels outside [0, C) on both sides; an all-padding scene."""
    c = _scenes("classes", 3, 48, 14, C=2, thr=[[0.5, 0.25]] * 4, wrong=0.0)
    dl, gl = c["det_labels"], c["gt_labels"]
    dl[:, 5::7] = 2
    dl[:, 3::11] = np.array([-1, 4, 7, -9, 64])[np.arange(dl[:, 3::11].shape[1]) % 5]
    gl[:, 4::5] = 3
    gl[:, 2::9] = np.array([-1, 4, 100])[np.arange(gl[:, 2::9].shape[1]) % 3]
    gl[2] = -1
    c["gt_boxes"][2] = np.nan                                        # (a padding row is never read)
    return c


def _ties():
    """Detections in groups on one box each whose best scores tie: the index decides.  Scene 0: nine groups of four equal scores.
    Scene 1: six groups of six on a box of their own, four zeros of alternating sign above -1 and -2; in the even groups the
    lowest index holds -0, in the odd ones +0, so a ranking that compares the score bits (-0 below +0) hands the box of every
    even group to another detection than the float compare does."""
    c = _scenes("ties", 2, 36, 6, wrong=0.0)
    sc = c["det_scores"]
    sc[0] = np.repeat(np.arange(9, dtype=F) / 8, 4)
    sc[1] = np.concatenate([np.array([-0.0, 0.0, -0.0, 0.0, -1.0, -2.0] if j % 2 == 0 else [0.0, -0.0, 0.0, -0.0, -1.0, -2.0], F)
                            for j in range(6)])
    for b in range(2):
        g = np.arange(36) // 4 % 6 if b == 0 else np.arange(36) // 6
        c["det_boxes"][b, :, :7] = c["gt_boxes"][b, g, :7]
        c["det_boxes"][b, :, 0] += (np.arange(36) % (4 if b == 0 else 6)).astype(F) * F(0.05)
        c["det_labels"][b] = c["gt_labels"][b, g]
    return c


def _axis(x, y=0.0, l=4.0, w=2.0, z=0.0, h=1.5, yaw=0.0):
    return [x, y, z, l, w, h, yaw]


def _hand():
    """Hand-made axis-aligned scene, class 0, thr (0.7, 0.5):
    box 0 at x = 0: detection 0 (score .9) shifted by 1 (IoU 3/5), detection 1 (score .8) shifted by .125 (IoU 31/33): at 0.5 the first
    takes the box although the second overlaps it better, at 0.7 the second does: the taken sets diverge.
    boxes 1, 2 identical at x = 20: detections 2, 3 on them take 1, then 2.
    box 3 at x = 40 ignored, box 4 at x = 41.5 not: detection 4 at x = 40.25 overlaps the ignored one better and takes box 4;
    detections 5, 6, 7 on box 3 alone are absorbed by it."""
    gt = [_axis(0), _axis(20), _axis(20), _axis(40), _axis(41.5)]
    det = [_axis(1), _axis(0.125), _axis(20.25), _axis(19.75), _axis(40.25), _axis(39.5), _axis(39.75), _axis(39.25), _axis(80)]
    sc = [.9, .8, .7, .6, .5, .4, .3, .2, .1]
    return _make([det], [sc], [[0] * 9], None, [gt], [[0] * 5], [[0, 0, 0, 1, 0]], [[0.7, 0.5]], "iou3d")


def _on_thr(metric):
    """thr column 0 is a pair's own f32 value (strict compare: no match), column 1 one ulp on the accepting side (match)."""
    gt = [_axis(0), _axis(30, yaw=0.3)]
    det = [_axis(0.7, 0.2, yaw=0.1), _axis(30.4, 0.3, yaw=0.45), _axis(60)]
    c = _make([det], [[.9, .8, .7]], [[0, 1, 0]], None, [gt], [[0, 1]], None, np.zeros((2, 2)), metric)
    v = pair_values(c, 0)
    for cls, (k, g) in enumerate(((0, 0), (1, 1))):
        c["thr"][cls] = v[k, g], np.nextafter(v[k, g], F(np.inf) if metric == "dist" else F(-np.inf))
    return c


def _wave():
    """G = 200: class 0 has 65 boxes, class 1 has 130 (the lanes of a wave, and the trips of its loop), 5 rows are padding."""
    c = _scenes("wave", 1, 40, 200, C=2, thr=[[0.5, 0.25]] * 2, wrong=0.0)
    gl = np.array([0] * 65 + [1] * 130 + [-1] * 5, np.int32)
    c["gt_labels"][0] = np.random.default_rng(5).permutation(gl)
    rng = np.random.default_rng(6)
    g = rng.integers(0, 200, 40)
    c["det_boxes"][0, :, :7] = c["gt_boxes"][0, g, :7]
    c["det_boxes"][0, :, 0] += rng.uniform(-0.3, 0.3, 40).astype(F)
    c["det_labels"][0] = np.where(c["gt_labels"][0, g] >= 0, c["gt_labels"][0, g], 0)
    return c


def _big():
    """One scene at the limits, K = G = 1024, 64 classes of 16 boxes and 16 detections each."""
    c = _scenes("big", 1, 1024, 1024, C=64, metric="iou_bev", thr=[[0.5, 0.25]] * 64, ignore=True)
    return c


BUILDERS = {
    "basic": lambda: _scenes("basic", 3, 40, 12, ignore=True),
    "basic:bev": lambda: _scenes("basic", 3, 40, 12, metric="iou_bev", ignore=True),
    "basic:dist": lambda: _scenes("basic", 3, 40, 12, metric="dist", ignore=True),
    "wide_rows": lambda: _scenes("wide_rows", 2, 65, 80, D=9, Dg=9, thr=[[0.7], [0.5], [0.3]]),      # T = 1, K = 65
    "t8": lambda: _scenes("t8", 1, 96, 30, C=1, thr=[[0.9, 0.8, 0.7, 0.6, 0.5, 0.4, 0.25, 0.1]]),      # T = 8
    "counts": _counts,
    "g0": _g0,
    "classes": _classes,
    "ties": _ties,
    "hand": _hand,
    "on_thr": lambda: _on_thr("iou3d"),
    "on_thr:bev": lambda: _on_thr("iou_bev"),
    "on_thr:dist": lambda: _on_thr("dist"),
    "wave": _wave,
    "big": _big,
}
CASES = list(BUILDERS)
# what each case is there for (coverage(name) must contain it)
CLAIMS = {
    "basic": {"matched", "false_positive", "absorbed", "iou3d"}, "basic:bev": {"matched", "iou_bev"}, "basic:dist": {"matched", "dist"},
    "wide_rows": {"d9", "matched"}, "t8": {"t8", "diverge"},
    "counts": {"count0", "count1", "countK", "d9"}, "g0": {"g0", "false_positive"},
    "classes": {"class_without_gt", "class_without_det", "labels_outside"},
    "ties": {"score_tie", "pm0"},
    "hand": {"identical_gt", "greedy_steal", "diverge", "ignore_absorbs3", "nonignored_preferred"},
    "on_thr": {"on_thr", "iou3d"}, "on_thr:bev": {"on_thr", "iou_bev"}, "on_thr:dist": {"on_thr", "dist"},
    "wave": {"class65", "class130", "matched"}, "big": {"k1024g1024", "matched", "absorbed"},
}
# the cases the float64 re-implementation of the CPU test is run on (no pair value within 1e-5 of a threshold)
F64_CASES = ("basic", "basic:bev", "basic:dist", "wide_rows", "t8", "counts", "classes", "ties", "hand", "wave")


def _freeze(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def case(name):
    """-> dict(det_boxes, det_scores, det_labels, det_count, gt_boxes, gt_labels, gt_ignore, thr, metric).  Treat as read-only."""
    return _freeze(BUILDERS[name]())


@functools.lru_cache(maxsize=None)
def expected(name):
    """The outputs (and aux: vals) of a case, computed once.  Treat as read-only."""
    return _freeze(det_match(case(name)))


def coverage(name):
    """The set of things case `name` demonstrably contains, read off the case and the reference's outputs."""
    c, e = case(name), expected(name)
    B, K = c["det_labels"].shape
    G, (C, T) = c["gt_labels"].shape[1], c["thr"].shape
    dist = c["metric"] == "dist"
    tags = {c["metric"]}
    code, match, vals = e["code"], e["match"], e["vals"]
    if (code == 1).any():
        tags.add("matched")
    if (code == 0).any():
        tags.add("false_positive")
    if ((code == -1) & (match >= 0)).any():
        tags.add("absorbed")
    if c["det_count"] is not None:
        tags |= {t for t, n in (("count0", 0), ("count1", 1)) if (c["det_count"] == n).any()}
        if (c["det_count"] >= K).any():
            tags.add("countK")
    if G == 0:
        tags.add("g0")
    if c["det_boxes"].shape[2] == 9:
        tags.add("d9")
    if T == 8:
        tags.add("t8")
    if K == 1024 and G == 1024:
        tags.add("k1024g1024")
    for b in range(B):
        live, dl, gl = live_mask(c, b), c["det_labels"][b], c["gt_labels"][b]
        n = K if c["det_count"] is None else min(max(int(c["det_count"][b]), 0), K)
        ign = np.zeros(G, bool) if c["gt_ignore"] is None else c["gt_ignore"][b] != 0
        if ((np.arange(K) < n) & ((dl < 0) | (dl >= C))).any() and (gl >= C).any() and (gl < 0).any():
            tags.add("labels_outside")
        for cls in range(C):
            nd, ng = int((live & (dl == cls)).sum()), int((gl == cls).sum())
            if nd and not ng and (gl >= 0).any():
                tags.add("class_without_gt")
            if ng and not nd and live.any():
                tags.add("class_without_det")
            if ng == 65:
                tags.add("class65")
            if ng == 130:
                tags.add("class130")
            ks = np.flatnonzero(live & (dl == cls))
            s = c["det_scores"][b][ks]
            matched = (code[b, ks] == 1).any(1)
            # equal scores among detections that are matched or compete: the index decided
            if any((s[i] == s[j]) and (matched[i] or matched[j]) for i in range(len(ks)) for j in range(i + 1, len(ks))):
                tags.add("score_tie")
            # a matched detection that holds -0 won its box against a LATER detection that holds +0 and is accepted for the same box:
            # a compare of the score bits (-0 below +0) would have given the box to the other one
            for k in ks[(s == 0) & np.signbit(s)].tolist():
                for t in np.flatnonzero(code[b, k] == 1).tolist():
                    g, th = match[b, k, t], c["thr"][cls, t]
                    for k2 in ks[(s == 0) & ~np.signbit(s) & (ks > k)].tolist():
                        v = vals[b, k2, g]
                        if (v < th) if dist else (v > th):
                            tags.add("pm0")
        same_row = {}                                                 # (class, the row's bytes) -> the boxes that hold it
        for g in np.flatnonzero((gl >= 0) & (gl < C) & ~ign).tolist():
            same_row.setdefault((int(gl[g]), c["gt_boxes"][b, g].tobytes()), []).append(g)
        for t in range(T):
            for k in np.flatnonzero(live).tolist():
                g, cd = match[b, k, t], code[b, k, t]
                th = c["thr"][dl[k], t]
                if cd == 1:
                    twins = [h for h in same_row[(int(gl[g]), c["gt_boxes"][b, g].tobytes())] if h > g]
                    if any(e["gt_det"][b, h, t] >= 0 for h in twins):
                        tags.add("identical_gt")
                    # an ignored box of the class was accepted with a better value
                    for h in np.flatnonzero(ign & (gl == dl[k])).tolist():
                        v, w = vals[b, k, h], vals[b, k, g]
                        if (v < th and v < w) if dist else (v > th and v > w):
                            tags.add("nonignored_preferred")
                if cd == 0:
                    # a box it would have matched better than the detection that holds it
                    for h in np.flatnonzero((gl == dl[k]) & ~ign).tolist():
                        o, v = e["gt_det"][b, h, t], vals[b, k, h]
                        if o >= 0 and ((v < th and v < vals[b, o, h]) if dist else (v > th and v > vals[b, o, h])):
                            tags.add("greedy_steal")
                    if (vals[b, k] == th).any() and (code[b, k] == 1).any():
                        tags.add("on_thr")
            for g in np.flatnonzero(ign).tolist():
                if int(((match[b, :, t] == g) & (code[b, :, t] == -1)).sum()) >= 3:
                    tags.add("ignore_absorbs3")
        gd = e["gt_det"][b]
        if T >= 2 and any((gd[g, t0] >= 0) and (gd[g, t1] >= 0) and gd[g, t0] != gd[g, t1] for g in range(G) for t0 in range(T) for t1 in range(t0)):
            tags.add("diverge")
    return tags


def threshold_margin(name):
    """The smallest |pair value - threshold| over the pairs and threshold columns the rule reads."""
    c, e = case(name), expected(name)
    m = np.inf
    for b in range(c["det_labels"].shape[0]):
        v = e["vals"][b].astype(np.float64)
        th = c["thr"].astype(np.float64)[np.clip(c["det_labels"][b], 0, c["thr"].shape[0] - 1)]      # [K,T]
        d = np.abs(v[:, :, None] - th[:, None, :])
        if np.isfinite(d).any():
            m = min(m, float(np.nanmin(d)))
    return m


# ---- AP cases -------------------------------------------------------------------------------------------------------------------
def _ap_rows(name, N, C=3, T=2, p_ign=0.2, p_tp=0.5, tied=False, n_gt=None, outside=True):
    rng = np.random.default_rng(_seed(name))
    scores = (rng.integers(0, 4, N) / 4 if tied else rng.permutation(N) / max(N, 1)).astype(F)
    if N > 8 and not tied:
        scores[rng.integers(0, N, N // 8)] = scores[rng.integers(0, N, N // 8)]              # some ties
        scores[:4] = np.array([0.0, -0.0, -1.0, 2.0], F)
    labels = rng.integers(-1 if outside else 0, C + (1 if outside else 0), N).astype(np.int32)
    u = rng.random((N, T))
    code = np.where(u < p_ign, -1, np.where(u < p_ign + (1 - p_ign) * p_tp, 1, 0)).astype(np.int32)
    if n_gt is None:
        n_gt = [(code[labels == c] == 1).sum(0).max(initial=0) + c for c in range(C)]    # class 0 reaches recall 1, the others do not
    return dict(scores=scores, labels=labels, code=code, n_gt=np.asarray(n_gt, np.int32), points=40, first=1, floor=0.0)


def _ap_with(c, **kw):
    c.update(kw)
    return c


AP_BUILDERS = {
    "n1": lambda: _ap_rows("n1", 1, C=1, p_ign=0.0, p_tp=1.0, outside=False),
    "n255": lambda: _ap_rows("n255", 255, C=1, outside=False),
    "n256": lambda: _ap_rows("n256", 256, C=1, outside=False),
    "n257": lambda: _ap_rows("n257", 257, C=1, outside=False),
    "n5000": lambda: _ap_rows("n5000", 5003),
    "r11": lambda: _ap_with(_ap_rows("r11", 700), points=10, first=0),
    "nuscenes": lambda: _ap_with(_ap_rows("nuscenes", 900, C=4, T=4), points=100, first=11, floor=0.1),
    "p128": lambda: _ap_with(_ap_rows("p128", 300, T=8), points=128, first=128),
    "all_ignored": lambda: _ap_rows("all_ignored", 300, p_ign=1.0, n_gt=[5, 0, 2]),
    "all_tied": lambda: _ap_rows("all_tied", 600, tied=True),
    "no_gt": lambda: _ap_rows("no_gt", 300, n_gt=[0, 7, 0]),
    "low_recall": lambda: _ap_rows("low_recall", 400, n_gt=[400, 300, 100]),
    "all_fp": lambda: _ap_rows("all_fp", 300, p_ign=0.0, p_tp=0.0, n_gt=[3, 3, 3]),
    "perfect": lambda: _ap_rows("perfect", 300, p_ign=0.0, p_tp=1.0, outside=False),
}
AP_CASES = list(AP_BUILDERS)


@functools.lru_cache(maxsize=None)
def ap_case(name):
    """-> dict(scores, labels, code, n_gt, points, first, floor).  Treat as read-only."""
    return _freeze(AP_BUILDERS[name]())


@functools.lru_cache(maxsize=None)
def ap_expected(name):
    c = ap_case(name)
    return _freeze(det_ap(c["scores"], c["labels"], c["code"], c["n_gt"], c["points"], c["first"], c["floor"]))
