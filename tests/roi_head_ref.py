"""Numpy float32 reference of SPEC.md §28 (RoI head: roi_targets, roi_decode), every operation written out in the section's
order and rounded on its own, in two forms that must agree bit for bit: `*_loop` (the kernels' structure: one RoI, one slot,
one row at a time) and `*_vec` (whole arrays).  Plus the named cases the CPU and GPU tests share:
tests/test_roi_head_cpu.py asserts on the reference the coverage the GPU cases rely on; tests/test_gpu_roi_head.py compares
the kernels with `expected(name)`.

The IoU is tests/box_ref.py's `boxes_iou(..., "3d")` (§19.3), computed once per case over the candidate rows only and shared by
both forms; sin / cos come from the oracle's §13 routine (`oracle.sincos_r`); the hash is §17's (`sad_amd.io._h`)."""
import functools

import numpy as np

import box_ref

F = np.float32
PI, TWO_PI, HALF_PI, THREE_HALF_PI = F(np.pi), F(2 * np.pi), F(np.pi / 2), F(3 * np.pi / 2)
EPS = F(1e-5)
DRAW_BASE = 0x80000000
OUTPUTS = ("index", "match", "labels", "iou", "cls_target", "reg_valid", "rois_s", "gt_local", "reg_target")
DEFAULTS = dict(S=32, fg_max=16, fg_thr=0.55, bg_lo=0.1, hard_ratio=0.8, reg_fg_thr=0.55, cls_fg_thr=0.75, cls_bg_thr=0.25,
                cls_mode="roi_iou", seed=0)


def h(seed, b, i):
    """§17 h(b, i) under `seed` for a scalar or an array of i -> uint32."""
    from sad_amd import io as sad_io
    return sad_io._h(int(seed), int(b), i)


def sincos(yaw):
    import oracle
    s, c = oracle.sincos_r(np.ascontiguousarray(np.asarray(yaw, F).reshape(-1)))
    return s.astype(F).reshape(np.shape(yaw)), c.astype(F).reshape(np.shape(yaw))


def counts_of(c):
    """n_b per scene."""
    B, R = c["rois"].shape[:2]
    return np.full(B, R, np.int64) if c["roi_count"] is None else np.clip(c["roi_count"].astype(np.int64), 0, R)


def iou_rows(c):
    """Per scene the [n_b, G] §19.3 3-D IoU of the candidate rows against the non-padding boxes (0 in a padding column): only
    rows r < n_b are read."""
    n, out = counts_of(c), []
    G = c["gt_labels"].shape[1]
    for b in range(len(n)):
        m = np.zeros((n[b], G), F)
        real = np.flatnonzero(c["gt_labels"][b] >= 0)
        if n[b] and real.size:
            m[:, real] = box_ref.boxes_iou(c["rois"][b:b + 1, :n[b], :7], c["gt_boxes"][b:b + 1, real, :7], "3d")[0]
        out.append(m)
    return out


def eligible(c, b, n):
    """[n, G] bool."""
    lab = c["gt_labels"][b]
    e = np.broadcast_to(lab >= 0, (n, lab.shape[0]))
    return e if c["roi_labels"] is None else e & (lab[None, :] == c["roi_labels"][b, :n, None])


# ---- matching ---------------------------------------------------------------------------------------------------------------
def match_loop(iou, elig):
    n, G = iou.shape
    m, j = np.zeros(n, F), np.full(n, -1, np.int32)
    for r in range(n):
        for g in range(G):
            if elig[r, g] and (j[r] < 0 or iou[r, g] > m[r]):       # strict: a tie stays with the lowest g
                m[r], j[r] = iou[r, g], g
    return m, j


def match_vec(iou, elig):
    n, G = iou.shape
    if G == 0:
        return np.zeros(n, F), np.full(n, -1, np.int32)
    masked = np.where(elig, iou, F(-1))
    j = np.where(elig.any(1), np.argmax(masked, 1), -1).astype(np.int32)    # first of the maxima: the lowest g
    return np.where(j >= 0, masked.max(1), F(0)).astype(F), j


# ---- sampling ---------------------------------------------------------------------------------------------------------------
def plan_of(m, kw):
    """The class lists (ascending r) and the slot counts of a scene with best IoUs m [n]."""
    fg_thr, bg_lo = F(kw["fg_thr"]), F(kw["bg_lo"])
    fg = np.flatnonzero(m >= fg_thr)
    hard = np.flatnonzero((m >= bg_lo) & (m < fg_thr))
    easy = np.flatnonzero(m < bg_lo)
    S, n_fg, n_bg = kw["S"], len(fg), len(hard) + len(easy)
    if len(m) == 0:
        nf = 0
    elif n_fg and n_bg:
        nf = min(kw["fg_max"], n_fg, S)
    else:
        nf = S if n_fg else 0
    nb = S - nf
    want = int(np.floor(F(nb) * F(kw["hard_ratio"])))
    if len(hard) and len(easy):
        nh = min(want, len(hard))
    else:
        nh = nb if len(hard) else 0
    return dict(fg=fg, hard=hard, easy=easy, nf=nf, nb=nb, nh=nh, want=want, ranked=bool(n_fg and n_bg))


def slots_loop(b, m, kw):
    """The candidate of every slot of scene b (-1: empty), one slot at a time."""
    p, S, seed = plan_of(m, kw), kw["S"], kw["seed"]
    pick = np.full(S, -1, np.int64)
    if len(m) == 0:
        return pick, p
    order = sorted((int(h(seed, b, int(r))), int(r)) for r in p["fg"]) if p["ranked"] else None
    for i in range(S):
        draw = int(h(seed, b, DRAW_BASE + i))
        if i < p["nf"]:
            pick[i] = order[i][1] if p["ranked"] else p["fg"][draw % len(p["fg"])]
        elif i - p["nf"] < p["nh"]:
            pick[i] = p["hard"][draw % len(p["hard"])]
        else:
            pick[i] = p["easy"][draw % len(p["easy"])]
    return pick, p


def slots_vec(b, m, kw):
    p, S, seed = plan_of(m, kw), kw["S"], kw["seed"]
    if len(m) == 0:
        return np.full(S, -1, np.int64), p
    i = np.arange(S)
    draw = h(seed, b, DRAW_BASE + i.astype(np.uint64)).astype(np.int64)
    pick = np.zeros(S, np.int64)
    fg, hard, easy, nf, nh = p["fg"], p["hard"], p["easy"], p["nf"], p["nh"]
    if p["ranked"]:
        key = h(seed, b, fg.astype(np.uint64)).astype(np.int64)
        pick[:nf] = fg[np.lexsort((fg, key))][:nf]
    elif nf:
        pick[:nf] = fg[draw[:nf] % len(fg)]
    if nh:
        pick[nf:nf + nh] = hard[draw[nf:nf + nh] % len(hard)]
    if S - nf - nh:
        pick[nf + nh:] = easy[draw[nf + nh:] % len(easy)]
    return pick, p


# ---- the outputs of a slot ----------------------------------------------------------------------------------------------------
def heading(gyaw, rr):
    """§28.1 heading; float32 scalars or arrays."""
    dr = gyaw - rr
    o = dr - (np.floor(dr / TWO_PI) * TWO_PI)
    flip = (o > HALF_PI) & (o < THREE_HALF_PI)
    o2 = o + PI
    o2 = o2 - (np.floor(o2 / TWO_PI) * TWO_PI)
    o = np.where(flip, o2, o)
    o = np.where(o > PI, o - TWO_PI, o)
    return np.minimum(np.maximum(o, -HALF_PI), HALF_PI).astype(F)


def cls_target_of(m, kw):
    fg, bg = F(kw["cls_fg_thr"]), F(kw["cls_bg_thr"])
    d = fg - bg
    mid = (m - bg) / d if kw["cls_mode"] == "roi_iou" else np.full(np.shape(m), -1, F)
    return np.where(m > fg, F(1), np.where(m < bg, F(0), mid)).astype(F)


def _empty_out(B, S):
    return dict(index=np.full((B, S), -1, np.int32), match=np.full((B, S), -1, np.int32), labels=np.full((B, S), -1, np.int32),
                iou=np.zeros((B, S), F), cls_target=np.full((B, S), -1, F), reg_valid=np.zeros((B, S), np.int32),
                rois_s=np.zeros((B, S, 7), F), gt_local=np.zeros((B, S, 7), F), reg_target=np.zeros((B, S, 7), F))


def fill_vec(out, b, c, pick, m, j, kw):
    """Slots of scene b from their candidates `pick` [S] (all >= 0), whole columns at a time."""
    roi = c["rois"][b, pick, :7]
    mm, jj = m[pick], j[pick]
    out["index"][b], out["match"][b], out["iou"][b], out["rois_s"][b] = pick, jj, mm, roi
    out["labels"][b] = np.where(jj >= 0, c["gt_labels"][b][np.maximum(jj, 0)], -1) if c["gt_labels"].shape[1] else -1
    out["reg_valid"][b] = (jj >= 0) & (mm > F(kw["reg_fg_thr"]))
    out["cls_target"][b] = cls_target_of(mm, kw)
    has = np.flatnonzero(jj >= 0)
    if not has.size:
        return
    r, g = roi[has], c["gt_boxes"][b, jj[has], :7]
    s, co = sincos(r[:, 6])
    dx, dy, dz = g[:, 0] - r[:, 0], g[:, 1] - r[:, 1], g[:, 2] - r[:, 2]
    lx = (dx * co) + (dy * s)
    ly = (dy * co) - (dx * s)
    o = heading(g[:, 6], r[:, 6])
    out["gt_local"][b, has] = np.stack([lx, ly, dz, g[:, 3], g[:, 4], g[:, 5], o], 1)
    la, wa, ha = np.maximum(r[:, 3], EPS), np.maximum(r[:, 4], EPS), np.maximum(r[:, 5], EPS)
    dg = np.sqrt((la * la) + (wa * wa))
    out["reg_target"][b, has] = np.stack([lx / dg, ly / dg, dz / ha, np.log(np.maximum(g[:, 3], EPS) / la),
                                          np.log(np.maximum(g[:, 4], EPS) / wa), np.log(np.maximum(g[:, 5], EPS) / ha), o], 1)


def fill_loop(out, b, c, pick, m, j, kw):
    """The same, one slot at a time on float32 scalars."""
    fg, bg, reg_thr = F(kw["cls_fg_thr"]), F(kw["cls_bg_thr"]), F(kw["reg_fg_thr"])
    d = fg - bg
    for i, r in enumerate(pick):
        roi, mm, jj = c["rois"][b, r, :7], m[r], int(j[r])
        out["index"][b, i], out["match"][b, i], out["iou"][b, i], out["rois_s"][b, i] = r, jj, mm, roi
        out["labels"][b, i] = c["gt_labels"][b, jj] if jj >= 0 else -1
        out["reg_valid"][b, i] = int(jj >= 0 and mm > reg_thr)
        if mm > fg:
            ct = F(1)
        elif mm < bg:
            ct = F(0)
        else:
            ct = (mm - bg) / d if kw["cls_mode"] == "roi_iou" else F(-1)
        out["cls_target"][b, i] = ct
        if jj < 0:
            continue
        g = c["gt_boxes"][b, jj, :7]
        s, co = (v[0] for v in sincos(roi[6:7]))
        dx, dy, dz = g[0] - roi[0], g[1] - roi[1], g[2] - roi[2]
        lx = (dx * co) + (dy * s)
        ly = (dy * co) - (dx * s)
        dr = g[6] - roi[6]
        o = dr - (np.floor(dr / TWO_PI) * TWO_PI)
        if o > HALF_PI and o < THREE_HALF_PI:
            o = o + PI
            o = o - (np.floor(o / TWO_PI) * TWO_PI)
        if o > PI:
            o = o - TWO_PI
        o = min(max(o, -HALF_PI), HALF_PI)
        out["gt_local"][b, i] = (lx, ly, dz, g[3], g[4], g[5], o)
        la, wa, ha = max(roi[3], EPS), max(roi[4], EPS), max(roi[5], EPS)
        dg = np.sqrt((la * la) + (wa * wa))
        out["reg_target"][b, i] = (lx / dg, ly / dg, dz / ha, np.log(max(g[3], EPS) / la), np.log(max(g[4], EPS) / wa),
                                   np.log(max(g[5], EPS) / ha), o)


def _roi_targets(form, c, iou=None):
    """-> the nine outputs and aux: m, j [B,R] (0 / -1 beyond n_b) and the per-scene plans."""
    with np.errstate(all="ignore"):
        kw = c["kw"]
        B, R = c["rois"].shape[:2]
        n = counts_of(c)
        iou = iou_rows(c) if iou is None else iou
        out = _empty_out(B, kw["S"])
        out["m"], out["j"], out["plans"] = np.zeros((B, R), F), np.full((B, R), -1, np.int32), []
        for b in range(B):
            m, j = (match_loop if form == "loop" else match_vec)(iou[b], eligible(c, b, n[b]))
            out["m"][b, :n[b]], out["j"][b, :n[b]] = m, j
            pick, plan = (slots_loop if form == "loop" else slots_vec)(b, m, kw)
            out["plans"].append(plan)
            if n[b]:
                (fill_loop if form == "loop" else fill_vec)(out, b, c, pick, m, j, kw)
        return out


roi_targets_loop = functools.partial(_roi_targets, "loop")
roi_targets_vec = functools.partial(_roi_targets, "vec")


# ---- §28.2 ------------------------------------------------------------------------------------------------------------------
def roi_decode_vec(rois, reg):
    with np.errstate(all="ignore"):
        r, t = np.asarray(rois, F)[..., :7], np.asarray(reg, F)
        la, wa, ha = np.maximum(r[..., 3], EPS), np.maximum(r[..., 4], EPS), np.maximum(r[..., 5], EPS)
        dg = np.sqrt((la * la) + (wa * wa))
        s, c = sincos(r[..., 6])
        lx, ly, lz = t[..., 0] * dg, t[..., 1] * dg, t[..., 2] * ha
        return np.stack([((lx * c) - (ly * s)) + r[..., 0], ((lx * s) + (ly * c)) + r[..., 1], lz + r[..., 2], np.exp(t[..., 3]) * la,
                         np.exp(t[..., 4]) * wa, np.exp(t[..., 5]) * ha, t[..., 6] + r[..., 6]], -1).astype(F)


def roi_decode_loop(rois, reg):
    with np.errstate(all="ignore"):
        rois, reg = np.asarray(rois, F), np.asarray(reg, F)
        out = np.zeros(reg.shape, F)
        for idx in np.ndindex(reg.shape[:-1]):
            r, t = rois[idx], reg[idx]
            la, wa, ha = max(r[3], EPS), max(r[4], EPS), max(r[5], EPS)
            dg = np.sqrt((la * la) + (wa * wa))
            s, c = (v[0] for v in sincos(r[6:7]))
            lx, ly, lz = t[0] * dg, t[1] * dg, t[2] * ha
            out[idx] = (((lx * c) - (ly * s)) + r[0], ((lx * s) + (ly * c)) + r[1], lz + r[2], np.exp(t[3]) * la, np.exp(t[4]) * wa,
                        np.exp(t[5]) * ha, t[6] + r[6])
        return out


# ---- cases --------------------------------------------------------------------------------------------------------------------
def _seed(name):
    return int.from_bytes(name.encode(), "little") % (2 ** 31)


def _gt(rng, G, ncls=3):
    """G boxes of car-like extents 12 m apart along x (no two overlap), any yaw; rows of 8 fields (the last one unread)."""
    gt = np.zeros((G, 8), np.float64)
    gt[:, 0] = 12.0 * np.arange(G) + rng.uniform(-1, 1, G)
    gt[:, 1] = rng.uniform(-3, 3, G)
    gt[:, 2] = rng.uniform(-1.5, 0.0, G)
    gt[:, 3:6] = np.array([3.9, 1.6, 1.56]) * rng.uniform(0.8, 1.25, (G, 3))
    gt[:, 6] = rng.uniform(-3.5, 3.5, G)
    gt[:, 7] = 77.0
    return gt, rng.integers(0, ncls, G).astype(np.int32)


def _rois_near(rng, gt, lab, kinds):
    """One RoI per entry of `kinds` around a random box: "fg" a small jitter (IoU about 0.7 and above), "hard" a shift of 0.35 .. 0.7
    lengths along the box (IoU about 0.15 .. 0.5), "easy" 0.93 lengths along it or 50 m to the side (IoU below 0.05 or 0)."""
    R, G = len(kinds), len(gt)
    rois, rl = np.zeros((R, 7), np.float64), np.zeros(R, np.int32)
    for r, kind in enumerate(kinds):
        g = int(rng.integers(0, G))
        box = gt[g, :7].copy()
        along = np.array([np.cos(box[6]), np.sin(box[6])])
        if kind == "fg":
            box[:3] += rng.uniform(-0.06, 0.06, 3)
            box[3:6] *= rng.uniform(0.97, 1.03, 3)
            box[6] += rng.uniform(-0.03, 0.03)
        elif kind == "hard":
            box[:2] += along * box[3] * rng.uniform(0.35, 0.7) * rng.choice([-1, 1])
            box[6] += rng.uniform(-0.02, 0.02)
        elif rng.random() < 0.5:
            box[:2] += along * box[3] * 0.93
        else:
            box[1] += 50.0 + rng.uniform(0, 20)
        box[6] += 2 * np.pi * int(rng.integers(-1, 2))            # the same box, a turn away
        rois[r], rl[r] = box, lab[g]
    return rois, rl


def _scenes(name, mixes, G=6, by_class=False, D=7, **kw):
    """One scene per entry of `mixes` = (n_fg, n_hard, n_easy), shuffled; R = the largest scene.  Where the scenes differ in size,
    roi_count holds their sizes and the rows beyond are far boxes."""
    rng = np.random.default_rng(_seed(name))
    B, R = len(mixes), max(sum(mx) for mx in mixes)
    rois, rl = np.zeros((B, R, D), np.float64), np.zeros((B, R), np.int32)
    gts, labs = np.zeros((B, G, 8), np.float64), np.zeros((B, G), np.int32)
    for b, (nf, nh, ne) in enumerate(mixes):
        gts[b], labs[b] = _gt(rng, G)
        kinds = np.array(["fg"] * nf + ["hard"] * nh + ["easy"] * ne)
        rng.shuffle(kinds)
        rois[b, :, :7], rl[b] = _rois_near(rng, gts[b], labs[b], list(kinds) + ["easy"] * (R - len(kinds)))
    rois[..., 7:] = -5.0
    sizes = np.array([sum(mx) for mx in mixes], np.int32)
    return dict(rois=rois.astype(F), roi_count=None if (sizes == R).all() else sizes, roi_labels=rl if by_class else None,
                gt_boxes=gts.astype(F), gt_labels=labs, kw=dict(DEFAULTS, **kw))


def _on_threshold(cls_mode):
    """Axis-aligned pairs whose IoU is a threshold exactly: l = 3 shifted by 1 gives 0.5, l = 5 shifted by 3 gives 0.25."""
    gt = np.array([[[0, 0, 0, 3, 1, 1, 0], [100, 0, 0, 5, 1, 1, 0]]], F)
    rois = np.array([[[1, 0, 0, 3, 1, 1, 0],          # 0.5  == fg_thr, reg_fg_thr, cls_fg_thr
                      [103, 0, 0, 5, 1, 1, 0],        # 0.25 == bg_lo, cls_bg_thr
                      [0, 0, 0, 3, 1, 1, 0],          # 1
                      [2, 0, 0, 3, 1, 1, 0],          # 0.2: easy
                      [-1, 0, 0, 3, 1, 1, 0],         # 0.5 from the other side
                      [97, 0, 0, 5, 1, 1, 0],         # 0.25 from the other side
                      [102, 0, 0, 5, 1, 1, 0],        # 3 / 7: between the thresholds
                      [50, 0, 0, 3, 1, 1, 0],         # 0
                      [0.5, 0, 0, 3, 1, 1, 0]]], F)   # 2.5 / 3.5: above
    return dict(rois=rois, roi_count=None, roi_labels=None, gt_boxes=gt, gt_labels=np.zeros((1, 2), np.int32),
                kw=dict(DEFAULTS, S=24, fg_max=12, fg_thr=0.5, bg_lo=0.25, reg_fg_thr=0.5, cls_fg_thr=0.5, cls_bg_thr=0.25, cls_mode=cls_mode,
                        seed=3))


HEADING_DR = [0.0, 0.4, -0.4, 7.0, -7.0, 2 * np.pi + 0.3, -2 * np.pi - 0.3, 12.9, -12.9] + [
    sgn * (base + e) for base in (np.pi / 2, np.pi, 3 * np.pi / 2, 2 * np.pi) for e in (-1e-3, 1e-3, -2e-6, 2e-6) for sgn in (1, -1)]


def _heading():
    """One box; RoIs on it whose yaw differs from the box's by HEADING_DR: either side of +-pi/2, +-pi, +-3pi/2, +-2pi, and beyond;
    and one RoI far away, so that the others are ranked and every one of them gets a slot."""
    box = np.array([2.0, -1.0, -0.5, 2.2, 2.0, 1.6, 0.3])
    rois = np.repeat(box[None], len(HEADING_DR) + 1, 0)
    rois[:-1, 6] = box[6] - np.array(HEADING_DR)
    rois[-1, 0] += 40.0
    return dict(rois=rois[None].astype(F), roi_count=None, roi_labels=None, gt_boxes=box[None, None].astype(F),
                gt_labels=np.zeros((1, 1), np.int32), kw=dict(DEFAULTS, S=128, fg_max=64, fg_thr=0.3, bg_lo=0.1, reg_fg_thr=0.3, seed=11))


def _no_gt(G):
    c = _scenes("no_gt", [(9, 7, 11), (9, 7, 11)], G=4, by_class=True)
    if G == 0:
        c["gt_boxes"], c["gt_labels"] = np.zeros((2, 0, 7), F), np.zeros((2, 0), np.int32)
    else:
        c["gt_labels"] = c["gt_labels"].copy()
        c["gt_labels"][0] = -1                                       # an all-padding scene next to a normal one
        c["gt_boxes"][0] = np.nan                                     # (a padding row is never read)
    return c


def _ragged():
    c = _scenes("ragged", [(20, 15, 35), (1, 0, 69), (8, 8, 54)], seed=5)
    c["roi_count"] = np.array([70, 1, 0], np.int32)
    c["rois"][1, 1:], c["rois"][2, :] = np.nan, np.nan           # the rows beyond the count are never read
    return c


def _by_class():
    """RoIs of `both`'s kind matched per class; the first fg RoIs of each scene carry another class than the box they stand on."""
    c = _scenes("by_class", [(40, 21, 30), (13, 9, 69)], G=8, by_class=True, seed=2)
    rl = c["roi_labels"].copy()
    rl[:, ::5] = (rl[:, ::5] + 1) % 3
    c["roi_labels"] = rl
    return c


def _cap():
    rng = np.random.default_rng(_seed("cap"))
    gt, lab = _gt(rng, 2)
    kinds = np.array(["fg"] * 1500 + ["hard"] * 1100 + ["easy"] * 1496)
    rng.shuffle(kinds)
    rois, _ = _rois_near(rng, gt, lab, kinds)
    return dict(rois=rois[None].astype(F), roi_count=None, roi_labels=None, gt_boxes=gt[None].astype(F), gt_labels=lab[None],
                kw=dict(DEFAULTS, S=1024, fg_max=512, seed=9))


BUILDERS = {
    "both": lambda: _scenes("both", [(50, 30, 40), (21, 45, 54)], seed=1),                       # n_fg > fg_max, both bg classes
    "few_fg": lambda: _scenes("few_fg", [(5, 7, 50), (3, 40, 19)], S=64, fg_max=32, seed=4),         # floor(nb * ratio) > n_hard in scene 0
    "fg_only": lambda: _scenes("fg_only", [(37, 0, 0), (11, 0, 0)], S=48, fg_max=24, seed=6),         # draws with replacement from fg
    "bg_only": lambda: _scenes("bg_only", [(0, 13, 29), (0, 5, 3)], seed=7),
    "hard_only": lambda: _scenes("hard_only", [(6, 23, 0), (0, 11, 0)], seed=8),
    "easy_only": lambda: _scenes("easy_only", [(6, 0, 21), (0, 0, 11)], seed=10),
    "no_gt": lambda: _no_gt(4),
    "no_gt:g0": lambda: _no_gt(0),
    "ragged": _ragged,
    "by_class": _by_class,
    "on_threshold": lambda: _on_threshold("roi_iou"),
    "on_threshold:cls": lambda: _on_threshold("cls"),
    "odd": lambda: _scenes("odd", [(30, 20, 15), (2, 3, 60)], S=1, fg_max=1, D=9, seed=12),           # R = 65, S = 1
    "odd:fg0": lambda: _scenes("odd", [(30, 20, 15), (2, 3, 60)], S=1, fg_max=0, D=9, seed=12),       # ... the one slot is a bg draw
    "odd:short": lambda: _scenes("odd:short", [(2, 2, 1)], S=16, fg_max=8, seed=13),                  # S > n_b
    "cap": _cap,
    "heading": _heading,
}
CASES = list(BUILDERS)


@functools.lru_cache(maxsize=None)
def case(name):
    """-> dict(rois, roi_count, roi_labels, gt_boxes, gt_labels, kw).  Treat as read-only."""
    c = BUILDERS[name]()
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def iou_of(name):
    """The candidate IoU rows of a case, computed once (the scalar clip of box_ref is slow) and shared by both forms."""
    return iou_rows(case(name))


@functools.lru_cache(maxsize=None)
def expected(name):
    """The outputs (and aux: m, j, plans) of a case, computed once.  Treat as read-only."""
    out = roi_targets_vec(case(name), iou_of(name))
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def close(got, want, what):
    """§9: 1e-4 absolute + relative."""
    err = np.abs(np.asarray(got, np.float64) - np.asarray(want, np.float64))
    ok = err <= 1e-4 + 1e-4 * np.abs(want)
    assert ok.all(), f"{what}: {int((~ok).sum())} of {ok.size} beyond 1e-4, worst {float(err.max()):.3g}"


def check_round_trip(c, out, boxes):
    """`boxes` [B,S,7] decoded from (rois_s, reg_target): a matched slot gives its ground-truth centre and size back."""
    b, i = np.nonzero(out["match"] >= 0)
    assert b.size
    want = c["gt_boxes"][b, out["match"][b, i], :6]
    close(boxes[b, i, :6], want, "round trip centre and size")
