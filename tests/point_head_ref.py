"""numpy reference of the point head targets and loss (SPEC.md §31) and the named cases of tests/test_point_head_cpu.py and
tests/test_gpu_point_head.py.

  targets  float32, one numpy operation per step of §31.1 in its order (the in-box predicate and the local coordinates are
           box_ref's, sin / cos the oracle's §13 routine behind them); what passes through cbrtf / logf (centerness,
           reg_target[..., 3:6]) is also evaluated in binary64 (`centerness64`, `reg64`), which is what the GPU test compares with
  loss     whole arrays; one function evaluates §31.2 in float32 (sin / cos: dense_loss_ref.sincos_r) and in binary64 (numpy's).
           The float32 regression / shift / size terms and gradients are the spec's bits; the classification terms pass through
           expf / log1pf and are compared in binary64

The cases are built, not drawn: every scene of a RICH case holds a yaw-0 box 0 with dyadic centre and extents, a box 1 that
overlaps it, a padding row in the middle of the list, and points placed exactly on an xy face, exactly on a z face, in the band
only, in both boxes and far away; candidates stay well inside their box (every ratio >= 0.1) or well outside it; predictions
sit below, at and above every clamp bound.  The EDGE cases (one point, no box, one box, no positive) hold what their shape allows."""
import functools
import zlib

import numpy as np

import box_ref
import dense_loss_ref

F = np.float32
D = np.float64
ANCHORS = ((3.9, 1.6, 1.56), (0.8, 0.6, 1.73), (1.76, 0.6, 1.73))          # SPEC.md §9
ANCHOR_CAR = (3.9, 1.6, 1.56)                                              # SPEC.md §8
SHIFT_MAX = 2.0
MARGIN = 1e-3                                                              # no |d| within this of the smooth-L1 kink beta
RATIO_MARGIN = 0.02                                                        # a positive's candidate: every ratio >= this, or centerness exactly 0
KW = dict(cls_loss="bce", alpha=0.25, beta=1.0 / 9.0, code_weights=tuple(float(F(v)) for v in (1.0, 1.0, 1.0, 0.7, 0.7, 0.7, 1.3)),
          shift_max=SHIFT_MAX, scale=(1.0, 2.0, 0.5, 0.25), normalize=True)
TARGET_OUTPUTS = ("labels", "match", "centerness", "shift_target", "size_target", "reg_target")
LOSS_INPUTS = ("o", "c", "labels", "centerness", "reg_target", "shift_target", "size_target")


def _seqsum(x):
    """Sum over the last axis, ascending, one rounding per addition, from +0."""
    acc = np.zeros(x.shape[:-1], x.dtype)
    for j in range(x.shape[-1]):
        acc = acc + x[..., j]
    return acc


# ---- §31.1 ---------------------------------------------------------------------------------------------------------------------
def _ratio(h, l, dt):
    f, bk = h + l, h - l
    mn, mx = np.maximum(np.minimum(f, bk), dt(0)), np.maximum(f, bk)
    with np.errstate(all="ignore"):
        return np.where(mx > 0, mn / np.where(mx > 0, mx, dt(1)), dt(0))


def size_code(size, size_anchor):
    """§31.1 size_target of float32 extents: the inverse of §8 step 3, three IEEE operations and two selections per element."""
    qd = np.asarray(size, F) / np.asarray(size_anchor, F)
    u = np.maximum((F(2) * qd) - F(1), F(0))
    return np.minimum(np.sqrt(u) - F(1), F(1))


def size_decode(s, size_anchor):
    """§8 step 3 on a float32 s: clamp, q = (1 + s) + 0.5 (s s), extents = size_anchor q."""
    s = np.clip(np.asarray(s, F), F(-1), F(1))
    q = (F(1) + s) + (F(0.5) * (s * s))
    return np.asarray(size_anchor, F) * q


def targets(c):
    """-> labels, match, centerness, shift_target, size_target, reg_target (float32 / int32) and centerness64, reg64, ratios64
    [B,M,3] (the three ratios of a positive in binary64, NaN elsewhere)."""
    xyz, cand, gt, gl, tk = c["xyz"], c["cand"], c["gt_boxes"], c["gt_labels"], c["tkw"]
    an, sa, sm = np.asarray(tk["anchors"], F), np.asarray(tk["size_anchor"], F), F(tk["shift_max"])
    C = an.shape[0]
    B, M = xyz.shape[:2]
    q = xyz if cand is None else cand
    out = dict(labels=np.full((B, M), -1, np.int32), match=np.full((B, M), -1, np.int32), centerness=np.zeros((B, M), F),
               shift_target=np.zeros((B, M, 3), F), size_target=np.zeros((B, M, 3), F), reg_target=np.zeros((B, M, 7), F),
               centerness64=np.zeros((B, M), D), reg64=np.zeros((B, M, 7), D), ratios64=np.full((B, M, 3), np.nan, D))
    rows = np.arange(M)
    for b in range(B):
        keep = np.flatnonzero((gl[b] >= 0) & (gl[b] < C) & (gt[b, :, 3:6] > 0).all(1)) if gt.shape[1] else np.zeros(0, np.int64)
        if keep.size == 0:
            continue
        bx = np.ascontiguousarray(gt[b, keep, :7])
        ins, band = box_ref.inside(xyz[b], bx, 0.0), box_ref.inside(xyz[b], bx, tk["extra_width"])
        hit, j = ins.any(1), np.argmax(ins, 1)
        cls = gl[b, keep[j]]
        out["labels"][b] = np.where(hit, cls, np.where(band.any(1), -2, -1))
        out["match"][b] = np.where(hit, keep[j], -1)
        lx, ly, dz, hl, hw, hh = box_ref.local_coords(q[b], bx, 0.0)
        r32 = [_ratio(h[j], l[rows, j], F) for h, l in ((hl, lx), (hw, ly), (hh, dz))]
        cent = np.cbrt((r32[0] * r32[1]) * r32[2])
        m = bx[j]                                                       # [M,7]: the matched box of every row (row 0 where none)
        b64 = m.astype(D)
        d64 = q[b].astype(D) - b64[:, :3]
        s64, c64 = np.sin(b64[:, 6]), np.cos(b64[:, 6])
        l64 = (d64[:, 0] * c64 + d64[:, 1] * s64, d64[:, 1] * c64 - d64[:, 0] * s64, d64[:, 2])
        r64 = np.stack([_ratio(0.5 * b64[:, 3 + a], l64[a], D) for a in range(3)], 1)
        with np.errstate(all="ignore"):
            reg = np.concatenate([m[:, :3] - q[b], np.clip(np.log(m[:, 3:6] / an[np.clip(cls, 0, C - 1)]), F(-2), F(2)), m[:, 6:7]], 1)
            reg64 = np.concatenate([b64[:, :3] - q[b].astype(D), np.clip(np.log(b64[:, 3:6] / an[np.clip(cls, 0, C - 1)].astype(D)), -2, 2), b64[:, 6:7]], 1)
            size = size_code(m[:, 3:6], sa)
        h1 = hit[:, None]
        out["centerness"][b] = np.where(hit, cent, F(0))
        out["centerness64"][b] = np.where(hit, np.cbrt(r64.prod(1)), 0.0)
        out["ratios64"][b] = np.where(h1, r64, np.nan)
        out["shift_target"][b] = np.where(h1, np.minimum(np.maximum(m[:, :3] - xyz[b], -sm), sm), F(0))
        out["size_target"][b] = np.where(h1, size, F(0))
        out["reg_target"][b] = np.where(h1, reg.astype(F), F(0))
        out["reg64"][b] = np.where(h1, reg64, 0.0)
    return out


# ---- §31.2 ---------------------------------------------------------------------------------------------------------------------
def _smooth_l1(d, beta, dt):
    a = np.abs(d)
    quad = a < beta
    return np.where(quad, ((dt(0.5) * a) * a) / beta, a - (dt(0.5) * beta)), np.where(quad, d / beta, np.sign(d))


def loss(c, dt=F):
    """-> num_pos [B], per_point [B,M,4], grad_o [B,M,C+7], grad_c [B,M,6] (when c["c"] is given), loss64 / loss [B,4] and
    resid [B,M,13] (|d| of the 7 + 3 + 3 smooth-L1 arguments of a positive row, NaN where a row or a component is off)."""
    kw = c["kw"]
    o = c["o"].astype(dt)
    labels = c["labels"]
    B, M, W = o.shape
    C = W - 7
    pos, live = labels >= 0, (labels != -2)[..., None]
    num_pos = pos.sum(1).astype(np.int32)
    s = np.asarray(kw["scale"], F).astype(dt)[None, :]
    wq = s / np.maximum(num_pos, 1).astype(F).astype(dt)[:, None] if kw["normalize"] else np.broadcast_to(s, (B, 4)).copy()
    wq0, wq1, wq2, wq3 = (wq[:, i][:, None, None] for i in range(4))
    beta, cw = dt(F(kw["beta"])), np.asarray((1.0,) * 7 if kw.get("code_weights") is None else kw["code_weights"], F).astype(dt)
    alpha, oma = dt(F(kw["alpha"])), dt(F(1.0) - F(kw["alpha"]))
    one, zero, two = dt(1), dt(0), dt(2)
    per = np.zeros((B, M, 4), dt)
    go = np.zeros((B, M, W), dt)
    resid = np.full((B, M, 13), np.nan, D)
    p1 = pos[..., None]
    with np.errstate(all="ignore"):
        # classification
        x = o[..., :C]
        hot = labels[..., None] == np.arange(C)
        e = np.exp(-np.abs(x))
        den = one + e
        big, small = one / den, e / den
        p, pc = np.where(x >= 0, big, small), np.where(x >= 0, small, big)
        if kw["cls_loss"] == "focal":
            bce = (np.maximum(x, zero) - np.where(hot, x, zero)) + np.log1p(e)
            pt, aw = np.where(hot, pc, p), np.where(hot, alpha, oma)
            term = ((aw * (pt * pt)) * bce) * wq0
            g = np.where(hot, ((-alpha) * (pc * pc)) * (((two * p) * bce) + pc), (oma * (p * p)) * (((two * pc) * bce) + p)) * wq0
        else:
            soft = one if c["centerness"] is None else c["centerness"].astype(dt)[..., None]
            t = np.where(hot & p1, soft, zero)
            bce = (np.maximum(x, zero) - (x * t)) + np.log1p(e)
            term, g = bce * wq0, (p - t) * wq0
        per[..., 0] = _seqsum(np.where(live, term, zero))
        go[..., :C] = np.where(live, g, zero)
        # box regression
        r, t = o[..., C:].copy(), c["reg_target"].astype(dt)
        ident = np.ones(r.shape, bool)
        ident[..., 3:6] = (r[..., 3:6] >= -two) & (r[..., 3:6] <= two)
        r[..., 3:6] = np.minimum(np.maximum(r[..., 3:6], -two), two)
        d = (r - t) * cw
        if dt is F:
            sp, cp = dense_loss_ref.sincos_r(r[..., 6])
            st, ct = dense_loss_ref.sincos_r(np.where(pos, t[..., 6], zero))
        else:
            sp, cp, st, ct = np.sin(r[..., 6]), np.cos(r[..., 6]), np.sin(t[..., 6]), np.cos(t[..., 6])
        d[..., 6] = ((sp * ct) - (cp * st)) * cw[6]
        l, sg = _smooth_l1(d, beta, dt)
        g = (sg * cw) * wq1
        g[..., 6] = g[..., 6] * ((cp * ct) + (sp * st))
        per[..., 1] = np.where(pos, _seqsum(l * wq1), zero)
        go[..., C:] = np.where(p1 & ident, g, zero)
        resid[..., :7] = np.where(p1, np.abs(d), np.nan)
        out = {"num_pos": num_pos, "grad_o": go}
        # shift and size
        if c["c"] is not None:
            cc = c["c"].astype(dt)
            gc = np.zeros((B, M, 6), dt)
            for k, (tg, lim, w, lo) in enumerate(((c["shift_target"], dt(F(kw["shift_max"] or 0)), wq2, 0), (c["size_target"], one, wq3, 3))):
                if tg is None:
                    continue
                xx = cc[..., lo:lo + 3]
                ident = (xx >= -lim) & (xx <= lim)
                d = np.minimum(np.maximum(xx, -lim), lim) - tg.astype(dt)
                l, sg = _smooth_l1(d, beta, dt)
                per[..., 2 + k] = np.where(pos, _seqsum(l * w), zero)
                gc[..., lo:lo + 3] = np.where(p1 & ident, sg * w, zero)
                resid[..., 7 + 3 * k:10 + 3 * k] = np.where(p1, np.abs(d), np.nan)
            out["grad_c"] = gc
    out["per_point"] = per
    out["resid"] = resid
    out["loss64"] = per.astype(D).sum(1)
    out["loss"] = out["loss64"].astype(F)
    return out


# ---- cases -----------------------------------------------------------------------------------------------------------------------
def _rng(*key):
    return np.random.default_rng([zlib.crc32(str(k).encode()) for k in key])


def _to_world(box, local):
    """A point given in a box's frame (binary64) -> the scene's frame."""
    s, c = np.sin(D(box[6])), np.cos(D(box[6]))
    return np.array([box[0] + local[0] * c - local[1] * s, box[1] + local[0] * s + local[1] * c, box[2] + local[2]])


def _scene(rng, M, G, C, rich, positives=True):
    """One scene: gt_boxes [G,8], gt_labels [G], xyz [M,3], cand [M,3]."""
    gt, gl = np.zeros((G, 8), F), np.full(G, -1, np.int32)
    for g in range(G):                                                       # a 20-column lattice, 8 m apart: no unplanned overlap
        gt[g, :3] = (8.0 + 8.0 * (g % 20), -4.0 + 8.0 * (g // 20), -1.0)
        k = (g - 1 if G >= 5 and g > 2 else g) % C                           # (row 2 of a list of five or more is padding)
        gt[g, 3:6] = np.asarray(ANCHORS[k]) * rng.uniform(0.8, 1.3, 3)
        gt[g, 6] = rng.uniform(-3.0, 3.0)
        gt[g, 7] = np.nan                                                    # column 7 of D = 8 is never read
        gl[g] = k
    if G >= 1:
        gt[0, :7] = (8.0, -4.0, -1.0, 4.0, 2.0, 1.5, 0.0)                     # dyadic, yaw 0: faces can be hit exactly
    if G >= 5:
        gt[1, :7] = (5.5, -3.0, -1.0, 4.0, 2.0, 1.5, 0.0)                     # overlaps box 0 in [6, 7.5] x [-4, -3]
        gl[1] = 1 % C
        gl[2] = -1                                                           # padding in the middle of the list
        gt[2, :7] = gt[3, :7]                                                # ... around box 3: it would win if it were not dropped
        gt[2, 3:6] *= F(1.25)
        if G >= 7:
            gl[5] = C                                                        # padding: a label beyond the classes
            gt[6, 4] = 0.0                                                   # padding: a non-positive extent
    valid = [g for g in range(G) if 0 <= gl[g] < C and (gt[g, 3:6] > 0).all()]
    if not positives:                                                        # every box far from every point
        gt[:, :2] += 1000.0
        valid = []
    xyz, cand = np.zeros((M, 3)), np.zeros((M, 3))
    special = []
    if rich:
        special = [((10.0, -4.0, -1.0), None),                               # exactly on the +x face of box 0: excluded, in the band
                   ((8.25, -4.25, -0.25), None),                             # exactly on the +z face of box 0: included
                   ((10.125, -4.0, -1.0), None),                             # the band only
                   ((7.0, -3.5, -1.0), None),                               # inside box 0 and box 1: box 0 wins
                   ((-100.0, -100.0, 0.0), None),                            # background
                   ((8.5, -4.5, -1.0), (18.0, -4.5, -1.0))]                  # inside box 0, candidate shifted far outside it
    for i in range(M):
        if i < len(special):
            xyz[i] = special[i][0]
            cand[i] = special[i][1] if special[i][1] is not None else special[i][0]
        elif valid and i % 5 != 4:                                           # inside a box, candidate well inside it too
            g = valid[(i - len(special)) % len(valid)]
            bx = gt[g].astype(D)
            lo = np.array([-0.6, -0.6, -0.6]), np.array([-0.8, -0.8, -0.8])
            hi = (np.array([-0.3, 0.6, 0.6]), np.array([-0.3, 0.8, 0.8])) if (g == 1 and G >= 5) else (-lo[0], -lo[1])   # box 1: its part outside box 0
            xyz[i] = _to_world(bx, rng.uniform(lo[0], hi[0]) * 0.5 * bx[3:6])
            cand[i] = _to_world(bx, rng.uniform(lo[1], hi[1]) * 0.5 * bx[3:6])
        else:                                                                # scattered: background, now and then a band
            xyz[i] = (rng.uniform(0, 170), rng.uniform(-10, 130), rng.uniform(-3, 1))
            cand[i] = xyz[i] + rng.uniform(-0.5, 0.5, 3)
    return gt, gl, xyz.astype(F), cand.astype(F)


def _predictions(name, c, t):
    """o and c around the targets `t`: noise of sigma 0.02 or 0.3 per row on the positives (|d| on both sides of beta), N(0, 0.5)
    elsewhere; in a rich case the first positives of scene 0 carry the clamp bounds.  Rows whose residuals come within MARGIN of
    beta are redrawn, deterministically, until none does."""
    rng = _rng(name, "pred")
    pos = t["labels"] >= 0
    B, M = pos.shape
    C = c["C"]
    sm = SHIFT_MAX

    def draw(r):
        sigma = np.where(pos, r.choice([0.02, 0.3], (B, M)), 0.5)[..., None]
        reg = np.where(pos[..., None], t["reg_target"], 0) + r.normal(0, 1, (B, M, 7)) * sigma
        cc = np.concatenate([np.where(pos[..., None], t["shift_target"], 0), np.where(pos[..., None], t["size_target"], 0)], -1)
        cc = cc + r.normal(0, 1, (B, M, 6)) * sigma
        cc[..., :3], cc[..., 3:] = np.clip(cc[..., :3], -0.9 * sm, 0.9 * sm), np.clip(cc[..., 3:], -0.9, 0.9)
        return np.concatenate([r.normal(0, 1.5, (B, M, C)), reg], -1).astype(F), cc.astype(F)

    o, cc = draw(rng)
    bounds = np.flatnonzero(pos[0])[:2] if c["rich"] else ()
    for attempt in range(1, 50):
        for k, m in enumerate(bounds):                                      # below / at / above, both signs
            o[0, m, C + 3:C + 6] = (-2.5, -2.0, 2.5) if k == 0 else (2.0, 1.0, -1.0)
            cc[0, m, :3] = (-2.5 * sm / 2, -sm, 2.5 * sm / 2) if k == 0 else (sm, 0.5, -0.5)
            cc[0, m, 3:] = (-1.5, -1.0, 1.5) if k == 0 else (1.0, 0.25, -0.25)
        c["o"], c["c"] = o, cc
        with np.errstate(all="ignore"):
            bad = (np.abs(loss(c, D)["resid"] - float(F(KW["beta"]))) < MARGIN).any(-1)
        if not bad.any():
            return
        o2, cc2 = draw(_rng(name, "pred", attempt))
        o, cc = np.where(bad[..., None], o2, o), np.where(bad[..., None], cc2, cc)
    raise AssertionError(f"{name}: rows within the margin after 50 draws")


#        name        B    M    G  C  rich
SHAPES = {
    "m70":        (1,  70,   5, 3, True),       # a partial workgroup
    "m257":       (3, 257,   5, 3, True),       # one workgroup and a row
    "m600_g300":  (3, 600, 300, 3, True),       # more boxes than threads in a staging pass; three workgroups, the last partial
    "m256_c1":    (1, 256,   5, 1, True),       # exactly one workgroup; one class
    "m1":         (1,   1,   1, 3, False),      # one point, one box
    "g0":         (3,  70,   0, 3, False),      # no boxes: the pointers are not read
    "g1_c1":      (1, 257,   1, 1, False),
    "no_pos":     (3, 257,   5, 3, False),      # scene 1 holds no positive
}
RICH = tuple(n for n, s in SHAPES.items() if s[4])
CASES = list(SHAPES)


def _case(name):
    B, M, G, C, rich = SHAPES[name]
    rng = _rng(name)
    scenes = [_scene(rng, M, G, C, rich, positives=not (name == "no_pos" and b == 1)) for b in range(B)]
    c = dict(name=name, C=C, rich=rich, gt_boxes=np.stack([s[0] for s in scenes]), gt_labels=np.stack([s[1] for s in scenes]),
             xyz=np.stack([s[2] for s in scenes]), cand=np.stack([s[3] for s in scenes]),
             tkw=dict(anchors=ANCHORS[:C], size_anchor=ANCHOR_CAR, shift_max=SHIFT_MAX, extra_width=0.2), kw=dict(KW))
    t = targets(c)
    # a scattered point that fell into a box with its candidate next to a face: the candidate moves to the box's centre
    close = (t["labels"] >= 0) & (np.nan_to_num(t["ratios64"], nan=1.0).min(-1) < 0.1) & (t["centerness64"] != 0)
    for b, m in np.argwhere(close):
        c["cand"][b, m] = c["gt_boxes"][b, t["match"][b, m], :3]
    t = targets(c)
    for k in TARGET_OUTPUTS:
        c[k] = t[k]
    _predictions(name, c, t)
    return c


@functools.lru_cache(maxsize=None)
def case(name):
    """-> dict(xyz, cand, gt_boxes, gt_labels, tkw; o, c, labels, centerness, reg_target, shift_target, size_target, kw; C, rich).
    The loss inputs are the reference's own float32 targets.  Treat as read-only."""
    c = _case(name)
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


def variant(c, **kw):
    """The case with other keywords of the loss (normalize=False, cls_loss="focal")."""
    return dict(c, kw=dict(c["kw"], **kw))


@functools.lru_cache(maxsize=None)
def expected_targets(name):
    t = targets(case(name))
    for v in t.values():
        v.setflags(write=False)
    return t


@functools.lru_cache(maxsize=None)
def expected(name, normalize=True, cls_loss="bce"):
    """{"f32": the float32 reference, "f64": the binary64 evaluation} of a named case under the given keywords, computed once.
    Treat as read-only."""
    c = variant(case(name), normalize=normalize, cls_loss=cls_loss)
    out = {"f32": loss(c), "f64": loss(c, D)}
    for r in out.values():
        for v in r.values():
            v.setflags(write=False)
    return out


def tolerance(want64):
    """§9: 1e-4 absolute + 1e-4 relative to |want64|."""
    return 1e-4 + 1e-4 * np.abs(want64)
