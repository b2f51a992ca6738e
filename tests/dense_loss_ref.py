"""numpy reference of the dense head losses (SPEC.md §27) in two independently written forms, a binary64 evaluation of the same
formulas, and the named cases of tests/test_dense_loss_cpu.py and tests/test_gpu_dense_loss.py.

  loop   one row / one element at a time, every operation a numpy float32 scalar operation in the order SPEC §27 writes it;
         sin / cos of the sine-difference from the oracle's §13 routine (`oracle.sincos_r`)
  vec    whole arrays; the same function evaluates the formulas in float32 (sin / cos: §13's routine written in numpy) and in
         float64 (numpy's sin / cos): what the GPU test compares the library-function parts against

Maps are nchw here; `to_nhwc` / `from_nhwc` permute them.  Every case has B = 3 different scenes."""
import functools
import zlib

import numpy as np

F = np.float32
D = np.float64
LO = F(1e-4)
HI = F(1.0) - F(1e-4)


# ---- §13's reproducible sin / cos in numpy float32 -----------------------------------------------------------------------------
def sincos_r(th):
    th = np.asarray(th, F)
    n = np.rint(th * F(0.63661975))
    r = th - n * F(1.5703125)
    r = r - n * F(4.8375129699707031e-4)
    r = r - n * F(7.5497899548918861e-8)
    q = n.astype(np.int64) & 3
    r2 = r * r
    ps = F(-1.9515295891e-4)
    ps = ps * r2; ps = ps + F(8.3321608736e-3)
    ps = ps * r2; ps = ps + F(-1.6666654611e-1)
    S = r * r2; S = S * ps; S = r + S
    pc = F(2.443315711809948e-5)
    pc = pc * r2; pc = pc + F(-1.388731625493765e-3)
    pc = pc * r2; pc = pc + F(4.166664568298827e-2)
    C = r2 * r2; C = C * pc
    one = F(1.0) - F(0.5) * r2
    C = one + C
    s = np.where(q == 0, S, np.where(q == 1, C, np.where(q == 2, -S, -C)))
    c = np.where(q == 0, C, np.where(q == 1, -S, np.where(q == 2, -C, S)))
    return s.astype(F), c.astype(F)


# ---- layouts -----------------------------------------------------------------------------------------------------------------
def to_nhwc(m):
    return None if m is None else np.ascontiguousarray(m.transpose(0, 2, 3, 1))


def from_nhwc(m):
    return None if m is None else np.ascontiguousarray(m.transpose(0, 3, 1, 2))


def rows_of(m, A):
    """nchw map [B, A*ch, H, W] -> rows [B, K, ch], k = (y*W + x)*A + a."""
    B, ch, H, W = m.shape
    return np.ascontiguousarray(m.reshape(B, A, ch // A, H, W).transpose(0, 3, 4, 1, 2).reshape(B, H * W * A, ch // A))


def map_of(r, A, H, W):
    """rows [B, K, ch] -> nchw map [B, A*ch, H, W]."""
    B, K, ch = r.shape
    return np.ascontiguousarray(r.reshape(B, H, W, A, ch).transpose(0, 3, 4, 1, 2).reshape(B, A * ch, H, W))


def _seqsum(x):
    """Sum over the last axis, ascending, one rounding per addition, from +0."""
    acc = np.zeros(x.shape[:-1], x.dtype)
    for j in range(x.shape[-1]):
        acc = acc + x[..., j]
    return acc


def _wq(scale, n, normalize, dt):
    """[B, len(scale)]: scale_i / (float)max(n_b, 1), or scale_i."""
    s = np.asarray(scale, F).astype(dt)[None, :]
    n = np.asarray(n).reshape(len(n), -1)
    return s / np.maximum(n, 1).astype(F).astype(dt) if normalize else np.broadcast_to(s, (n.shape[0], s.shape[1])).copy()


# ---- §27.1 ---------------------------------------------------------------------------------------------------------------------
def anchor_loss_vec(c, dt=F):
    kw = c["kw"]
    A, nb = c["A"], c["nb"]
    B, _, H, W = c["reg"].shape
    x = rows_of(c["cls"], A).astype(dt)
    reg = rows_of(c["reg"], A).astype(dt)
    labels, tgt = c["labels"], c["reg_target"].astype(dt)
    C = x.shape[-1]
    alpha, beta = dt(F(kw["alpha"])), dt(F(kw["beta"]))
    oma = dt(F(1.0) - F(kw["alpha"]))
    cw = np.asarray(kw["code_weights"], F).astype(dt)
    pos = labels >= 0
    num_pos = pos.sum(1).astype(np.int32)
    wq = _wq(kw["scale"], num_pos, kw["normalize"], dt)
    wq0, wq1, wq2 = (wq[:, i][:, None, None] for i in range(3))
    with np.errstate(all="ignore"):
        # classification
        t = labels[..., None] == np.arange(C)
        live = (labels != -2)[..., None]
        e = np.exp(-np.abs(x))
        den = dt(1) + e
        big, small = dt(1) / den, e / den
        p, pc = np.where(x >= 0, big, small), np.where(x >= 0, small, big)
        bce = (np.maximum(x, dt(0)) - np.where(t, x, dt(0))) + np.log1p(e)
        pt = np.where(t, pc, p)
        aw = np.where(t, alpha, oma)
        term0 = np.where(live, ((aw * (pt * pt)) * bce) * wq0, dt(0))
        gt_ = ((-alpha) * (pc * pc)) * (((dt(2) * p) * bce) + pc)
        gf_ = (oma * (p * p)) * (((dt(2) * pc) * bce) + p)
        gcls = np.where(live, np.where(t, gt_, gf_) * wq0, dt(0))
        # regression
        d = (reg - tgt) * cw
        extra = None
        if kw["sin_diff"]:
            if dt is F:
                sp, cp = sincos_r(reg[..., 6])
                st, ct = sincos_r(tgt[..., 6])
            else:
                sp, cp, st, ct = np.sin(reg[..., 6]), np.cos(reg[..., 6]), np.sin(tgt[..., 6]), np.cos(tgt[..., 6])
            d[..., 6] = ((sp * ct) - (cp * st)) * cw[6]
            extra = (cp * ct) + (sp * st)
        a = np.abs(d)
        quad = a < beta
        l = np.where(quad, ((dt(0.5) * a) * a) / beta, a - (dt(0.5) * beta))
        sg = np.where(quad, d / beta, np.sign(d))
        g = (sg * cw) * wq1
        if extra is not None:
            g[..., 6] = g[..., 6] * extra
        term1 = np.where(pos[..., None], l * wq1, dt(0))
        greg = np.where(pos[..., None], g, dt(0))
        per = np.zeros((B, labels.shape[1], 3), dt)
        per[..., 0], per[..., 1] = _seqsum(term0), _seqsum(term1)
        out = {"num_pos": num_pos, "grad_cls": map_of(gcls, A, H, W), "grad_reg": map_of(greg, A, H, W)}
        # direction
        if nb:
            z = rows_of(c["dir"], A).astype(dt)
            dirt = c["dir_target"]
            on = pos & (dirt >= 0) & (dirt < nb)
            tt = np.clip(dirt, 0, nb - 1)
            m = z.max(-1)
            u = np.exp(z - m[..., None])
            s = _seqsum(u)
            zt = np.take_along_axis(z, tt[..., None], -1)[..., 0]
            per[..., 2] = np.where(on, ((m + np.log(s)) - zt) * wq2[..., 0], dt(0))
            hot = (tt[..., None] == np.arange(nb)).astype(dt)
            out["grad_dir"] = map_of(np.where(on[..., None], ((u / s[..., None]) - hot) * wq2, dt(0)), A, H, W)
    out["per_anchor"] = per
    out["loss64"] = per.astype(D).sum(1)
    out["loss"] = out["loss64"].astype(F)
    return out


def anchor_loss_loop(c):
    """The per-row loop in binary32: every operation one numpy float32 scalar operation."""
    import oracle
    oracle.build()
    kw = c["kw"]
    A, nb = c["A"], c["nb"]
    B, _, H, W = c["reg"].shape
    cls, reg = rows_of(c["cls"], A), rows_of(c["reg"], A)
    dirm = rows_of(c["dir"], A) if nb else None
    labels, tgt, dirt = c["labels"], c["reg_target"], c["dir_target"]
    K, C = labels.shape[1], cls.shape[-1]
    alpha, beta, oma = F(kw["alpha"]), F(kw["beta"]), F(1.0) - F(kw["alpha"])
    cw = np.asarray(kw["code_weights"], F)
    with np.errstate(all="ignore"):
        yaw_p = np.clip(np.nan_to_num(reg[..., 6], posinf=0.0, neginf=0.0), -1e4, 1e4).astype(F)
        yaw_t = np.clip(np.nan_to_num(tgt[..., 6], posinf=0.0, neginf=0.0), -1e4, 1e4).astype(F)
    sp, cp = (v.reshape(B, K) for v in oracle.sincos_r(np.ascontiguousarray(yaw_p.reshape(-1))))
    st, ct = (v.reshape(B, K) for v in oracle.sincos_r(np.ascontiguousarray(yaw_t.reshape(-1))))
    per = np.zeros((B, K, 3), F)
    gcls, greg = np.zeros((B, K, C), F), np.zeros((B, K, 7), F)
    gdir = np.zeros((B, K, nb), F) if nb else None
    num_pos = np.zeros(B, np.int32)
    for b in range(B):
        n = int(sum(1 for k in range(K) if labels[b, k] >= 0))
        num_pos[b] = n
        w = [F(s) / F(max(n, 1)) if kw["normalize"] else F(s) for s in kw["scale"]]
        for k in range(K):
            lab = int(labels[b, k])
            acc = F(0)
            if lab != -2:
                for ci in range(C):
                    x = cls[b, k, ci]
                    e = np.exp(-np.abs(x))
                    den = F(1) + e
                    big, small = F(1) / den, e / den
                    p, pc = (big, small) if x >= 0 else (small, big)
                    bce = (np.maximum(x, F(0)) - (x if lab == ci else F(0))) + np.log1p(e)
                    if lab == ci:
                        l = (alpha * (pc * pc)) * bce
                        g = ((-alpha) * (pc * pc)) * (((F(2) * p) * bce) + pc)
                    else:
                        l = (oma * (p * p)) * bce
                        g = (oma * (p * p)) * (((F(2) * pc) * bce) + p)
                    acc = acc + l * w[0]
                    gcls[b, k, ci] = g * w[0]
            per[b, k, 0] = acc
            if lab < 0:
                continue
            acc = F(0)
            for j in range(7):
                if j == 6 and kw["sin_diff"]:
                    d = ((sp[b, k] * ct[b, k]) - (cp[b, k] * st[b, k])) * cw[6]
                else:
                    d = (reg[b, k, j] - tgt[b, k, j]) * cw[j]
                a = np.abs(d)
                if a < beta:
                    l, sg = ((F(0.5) * a) * a) / beta, d / beta
                else:
                    l, sg = a - (F(0.5) * beta), F(int(d > 0) - int(d < 0))
                g = (sg * cw[j]) * w[1]
                if j == 6 and kw["sin_diff"]:
                    g = g * ((cp[b, k] * ct[b, k]) + (sp[b, k] * st[b, k]))
                acc = acc + l * w[1]
                greg[b, k, j] = g
            per[b, k, 1] = acc
            if nb and 0 <= dirt[b, k] < nb:
                z = dirm[b, k]
                m = z[0]
                for dd in range(1, nb):
                    m = np.maximum(m, z[dd])
                u = [np.exp(z[dd] - m) for dd in range(nb)]
                s = F(0)
                for dd in range(nb):
                    s = s + u[dd]
                per[b, k, 2] = ((m + np.log(s)) - z[dirt[b, k]]) * w[2]
                for dd in range(nb):
                    gdir[b, k, dd] = ((u[dd] / s) - F(dd == dirt[b, k])) * w[2]
    out = {"num_pos": num_pos, "per_anchor": per, "grad_cls": map_of(gcls, A, H, W), "grad_reg": map_of(greg, A, H, W)}
    if nb:
        out["grad_dir"] = map_of(gdir, A, H, W)
    return out


# ---- §27.2 ---------------------------------------------------------------------------------------------------------------------
CENTER_MAPS = ("reg", "height", "dim", "rot", "vel")
CENTER_CH = (2, 1, 3, 2, 2)


def _center_cat(c):
    """The regression maps in anno's column order: [B, na, H*W]."""
    maps = [c[n] for n in CENTER_MAPS if c[n] is not None]
    B = maps[0].shape[0]
    return np.concatenate([m.reshape(B, m.shape[1], -1) for m in maps], 1)


def _center_split(g, c):
    """[B, na, H*W] -> {grad_<map>: nchw}."""
    B, _, H, W = c["hm"].shape
    out, j = {}, 0
    for n, ch in zip(CENTER_MAPS, CENTER_CH):
        if c[n] is not None:
            out["grad_" + n] = np.ascontiguousarray(g[:, j:j + ch].reshape(B, ch, H, W))
            j += ch
    return out


def center_loss_vec(c, dt=F, order=None):
    """`order`: the order in which the boxes of a scene add their gradients (default ascending g: the specified one)."""
    kw = c["kw"]
    x, t = c["hm"].astype(dt), c["heatmap"].astype(dt)
    B, C, H, W = x.shape
    HW = H * W
    ind, anno = c["ind"], c["anno"].astype(dt)
    G, na = ind.shape[1], anno.shape[-1]
    cw = np.asarray(kw["code_weights"], F).astype(dt)
    assigned = (ind >= 0) & (ind < HW)
    num_pos = np.stack([(c["heatmap"] == 1).reshape(B, -1).sum(1), assigned.sum(1)], 1).astype(np.int32)
    wq = _wq(kw["scale"], num_pos, kw["normalize"], dt)              # [B,2]: column i normalised by num_pos[:, i]
    wq0, wq1 = wq[:, 0][:, None, None, None], wq[:, 1][:, None, None]
    lo, hi = dt(LO), dt(HI)
    with np.errstate(all="ignore"):
        e = np.exp(-np.abs(x))
        den = dt(1) + e
        big, small = dt(1) / den, e / den
        ps = np.where(x >= 0, big, small)
        p = np.minimum(np.maximum(ps, lo), hi)
        inside = (ps >= lo) & (ps <= hi)
        q = dt(1) - p
        lgp, lgq = np.log(p), np.log(q)
        l1 = (-lgp) * (q * q)
        g1 = (q * q) * (((dt(2) * p) * lgp) - q)
        w1 = (dt(1) - t) * (dt(1) - t)
        w = w1 * w1
        l0 = ((-lgq) * (p * p)) * w
        g0 = (w * (p * p)) * (p - ((dt(2) * q) * lgq))
        one = t == 1
        terms_hm = np.where(one, l1, l0) * wq0
        ghm = np.where(inside, np.where(one, g1, g0) * wq0, dt(0))
        cat = _center_cat(c).astype(dt)
        cell = np.where(assigned, ind, 0)
        pred = np.take_along_axis(cat, np.broadcast_to(cell[:, None, :], (B, na, G)), 2).transpose(0, 2, 1) if G else np.zeros((B, 0, na), dt)
        d = pred - anno
        terms_reg = np.where(assigned[..., None], (np.abs(d) * cw) * wq1, dt(0))
        gbox = (np.sign(d) * cw) * wq1
    g = np.zeros((B, na, HW), dt)
    for b in range(B):
        seen = set()
        for gi in (range(G) if order is None else order):
            if not assigned[b, gi]:
                continue
            k = int(ind[b, gi])
            g[b, :, k] = gbox[b, gi] if k not in seen else g[b, :, k] + gbox[b, gi]
            seen.add(k)
    out = {"num_pos": num_pos, "grad_hm": ghm, "terms_hm": terms_hm, "terms_reg": terms_reg}
    out.update(_center_split(g, c))
    out["loss64"] = np.stack([terms_hm.astype(D).reshape(B, -1).sum(1), terms_reg.astype(D).reshape(B, -1).sum(1)], 1)
    out["loss"] = out["loss64"].astype(F)
    return out


def center_loss_loop(c):
    kw = c["kw"]
    x, t = c["hm"], c["heatmap"]
    B, C, H, W = x.shape
    HW = H * W
    ind, anno = c["ind"], c["anno"]
    G, na = ind.shape[1], anno.shape[-1]
    cw = np.asarray(kw["code_weights"], F)
    cat = _center_cat(c)
    num_pos = np.zeros((B, 2), np.int32)
    ghm, terms_hm = np.zeros((B, C, H, W), F), np.zeros((B, C, H, W), F)
    terms_reg = np.zeros((B, G, na), F)
    g = np.zeros((B, na, HW), F)
    for b in range(B):
        num_pos[b, 0] = int((t[b] == 1).sum())
        num_pos[b, 1] = sum(1 for gi in range(G) if 0 <= ind[b, gi] < HW)
        w = [F(kw["scale"][i]) / F(max(int(num_pos[b, i]), 1)) if kw["normalize"] else F(kw["scale"][i]) for i in range(2)]
        for idx in np.ndindex(C, H, W):
            xv, tv = x[(b,) + idx], t[(b,) + idx]
            e = np.exp(-np.abs(xv))
            den = F(1) + e
            ps = F(1) / den if xv >= 0 else e / den
            p = np.minimum(np.maximum(ps, LO), HI)
            q = F(1) - p
            if tv == 1:
                lg = np.log(p)
                l, gr = (-lg) * (q * q), (q * q) * (((F(2) * p) * lg) - q)
            else:
                lg = np.log(q)
                w1 = (F(1) - tv) * (F(1) - tv)
                ww = w1 * w1
                l, gr = ((-lg) * (p * p)) * ww, (ww * (p * p)) * (p - ((F(2) * q) * lg))
            terms_hm[(b,) + idx] = l * w[0]
            ghm[(b,) + idx] = gr * w[0] if LO <= ps <= HI else F(0)
        seen = set()
        for gi in range(G):
            k = int(ind[b, gi])
            if not 0 <= k < HW:
                continue
            for j in range(na):
                d = cat[b, j, k] - anno[b, gi, j]
                terms_reg[b, gi, j] = (np.abs(d) * cw[j]) * w[1]
                gj = (F(int(d > 0) - int(d < 0)) * cw[j]) * w[1]
                g[b, j, k] = gj if k not in seen else g[b, j, k] + gj
            seen.add(k)
    out = {"num_pos": num_pos, "grad_hm": ghm, "terms_hm": terms_hm, "terms_reg": terms_reg}
    out.update(_center_split(g, c))
    return out


# ---- cases -------------------------------------------------------------------------------------------------------------------
def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def _lattice(rng, shape, lo, hi, step=2.0 ** -10):
    """Random float32 values on a coarse lattice: differences of two of them are exact."""
    return (rng.integers(int(lo / step), int(hi / step) + 1, shape) * step).astype(F)


#                 name        H   W    A    C   nb
ANCHOR_SHAPES = {
    "l:1x1":     (1, 1, 1, 1, 0),
    "l:5x7":     (5, 7, 128, 3, 4),
    "l:3x67":    (3, 67, 6, 64, 2),
    "l:9x130":   (9, 130, 6, 3, 2),
    "l:5x7:c11": (5, 7, 6, 11, 2),         # a class chunk with a tail: 8 + 3
    "l:9x130:a32": (9, 130, 32, 1, 2),     # 19 tiles x 4 chunks = 76 workgroups per scene: the sum of the partials wraps its 64 lanes
    "l:edges":   (5, 7, 6, 3, 2),
    "l:exact":   (5, 7, 6, 3, 0),
    "l:3x67:a9": (3, 67, 9, 3, 2),         # a partial last chunk behind a full one: 8 + 1 anchors, the last tile 9 cells
    "l:5x7:a11": (5, 7, 11, 10, 2),        # 8 + 3 anchors, fewer cells than one tile
}
ANCHOR_CASES = list(ANCHOR_SHAPES)
ANCHOR_KW = dict(alpha=0.25, beta=1.0 / 9.0, code_weights=(1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0), sin_diff=True, scale=(1.0, 2.0, 0.2),
                 normalize=True)
BETA = F(1.0 / 9.0)


def _anchor_case(name):
    H, W, A, C, nb = ANCHOR_SHAPES[name]
    rng = _rng(name)
    B, HW = 3, H * W
    K = HW * A
    # scene 0: no positive (background and ignored rows), scene 1: all ignored, scene 2: mixed (a label >= C among the positives)
    labels = np.full((B, K), -1, np.int32)
    labels[0, rng.random(K) < 0.3] = -2
    labels[1] = -2
    kind = rng.random(K)
    labels[2] = np.where(kind < 0.3, rng.integers(0, C + 1, K), np.where(kind < 0.5, -2, -1)).astype(np.int32)
    labels[2, 0] = 0                                                    # (K = 1: the one row is a positive)
    pos = labels >= 0
    tgt = np.where(pos[..., None], _lattice(rng, (B, K, 7), -2.0, 2.0), F(0)).astype(F)
    tgt[..., 6] = np.where(pos, rng.uniform(-3.2, 3.2, (B, K)), 0).astype(F)
    reg_r = (tgt + rng.normal(0, 0.3, (B, K, 7))).astype(F)
    cls_r = rng.normal(0, 2.5, (B, K, C)).astype(F)
    dir_r = rng.normal(0, 2.0, (B, K, nb)).astype(F) if nb else None
    dirt = np.where(pos, rng.integers(0, max(nb, 1), (B, K)), -1).astype(np.int32) if nb else None
    kw = dict(ANCHOR_KW, code_weights=tuple(float(F(v)) for v in (1.0, 1.0, 1.0, 0.7, 0.7, 0.7, 1.3)))
    if name == "l:edges":
        pk = np.flatnonzero(pos[2])
        assert len(pk) >= 12
        # logits at 0, -0.0, +-100 on a positive's own class, on another class and on a background row
        cls_r[2, pk[0]] = (0.0, -0.0, 100.0)
        cls_r[2, pk[1]] = (-100.0, 100.0, 0.0)
        labels[2, pk[0]], labels[2, pk[1]] = 2, 0
        bg = np.flatnonzero(labels[2] == -1)
        cls_r[2, bg[0]] = (100.0, -100.0, -0.0)
        # |d| exactly at beta, just below, above, and d == 0 (code weight 1 in columns 0 .. 2)
        for i, dv in enumerate((BETA, np.nextafter(BETA, F(0)), F(0.5), F(0), -BETA, F(-2.0))):
            tgt[2, pk[2 + i], 0] = 0.0
            reg_r[2, pk[2 + i], 0] = dv
        # yaw predictions near +-1e3
        reg_r[2, pk[8], 6], reg_r[2, pk[9], 6] = F(999.7), F(-1000.2)
        # a dir_target out of range on a positive, on both sides
        dirt[2, pk[10]], dirt[2, pk[11]] = nb, -1
        # what a non-positive row holds in reg_target is never read into a result
        tgt[0, :, :6] = np.inf
        tgt[0, :, 6] = 7.0
    if name == "l:exact":
        # beta = 1/8, no sine difference, unit weights, 8 / 16 / 8 positives, differences multiples of 2^-4 with |d| <= 4
        kw = dict(ANCHOR_KW, beta=0.125, sin_diff=False, scale=(1.0, 1.0, 1.0))
        labels[:] = -1
        for b, npos in enumerate((8, 16, 8)):
            labels[b, rng.choice(K, npos, replace=False)] = rng.integers(0, C, npos)
        pos = labels >= 0
        tgt = np.where(pos[..., None], _lattice(rng, (B, K, 7), -2.0, 2.0, 2.0 ** -4), F(0)).astype(F)
        dmul = rng.integers(-64, 65, (B, K, 7))
        dmul[pos.nonzero()[0][:3], pos.nonzero()[1][:3], 0] = (0, 1, -1)   # d = 0 and |d| = 2^-4 < beta
        reg_r = (tgt + (dmul * 2.0 ** -4)).astype(F)
    c = dict(A=A, nb=nb, labels=labels, reg_target=tgt, dir_target=dirt, cls=map_of(cls_r, A, H, W), reg=map_of(reg_r, A, H, W),
             dir=map_of(dir_r, A, H, W) if nb else None, kw=kw)
    return c


#                 name        H   W    C   G     vel
CENTER_SHAPES = {
    "c:1x1":     (1, 1, 1, 0, False),
    "c:5x7":     (5, 7, 3, 3, True),
    "c:5x7:g1":  (5, 7, 1, 1, False),
    "c:3x67":    (3, 67, 64, 65, False),
    "c:5x7:c19": (5, 7, 19, 3, False),      # a class chunk with a tail: 16 + 3
    "c:9x130":   (9, 130, 3, 1024, True),
    "c:shared":  (5, 7, 1, 6, False),
}
CENTER_CASES = list(CENTER_SHAPES)
SHARED_CW = F(1.0) / F(3.0)


def _center_case(name):
    H, W, C, G, vel = CENTER_SHAPES[name]
    rng = _rng(name)
    B, HW = 3, H * W
    na = 10 if vel else 8
    # heat map targets: scene 0 has no cell equal to 1, scenes 1 and 2 have one to three; values in (0, 1) around, 0 elsewhere
    t = np.where(rng.random((B, C, H, W)) < 0.4, rng.uniform(0.01, 0.99, (B, C, H, W)), 0).astype(F)
    x = rng.normal(-2.0, 2.0, (B, C, H, W)).astype(F)
    flat_t, flat_x = t.reshape(B, -1), x.reshape(B, -1)
    n = flat_t.shape[1]
    for b in (1, 2):
        ones = rng.choice(n, min(n, b + 1), replace=False)
        flat_t[b, ones] = 1.0
        flat_x[b, ones] = rng.uniform(-9.0, -7.0, len(ones)).astype(F)     # a positive cell the head has not learnt yet
    if n >= 8:
        # sigmoids clamped on both sides: low on a positive cell, high on a cell with 0 < t < 1 and on one with t == 0
        flat_x[2, np.flatnonzero(flat_t[2] == 1)[0]] = -20.0
        mid, zero = np.flatnonzero((flat_t[2] > 0) & (flat_t[2] < 1)), np.flatnonzero(flat_t[2] == 0)
        flat_x[2, mid[0]], flat_x[2, zero[0]], flat_x[2, zero[1]] = 20.0, 20.0, -20.0
    ind = rng.integers(0, HW, (B, G)).astype(np.int32)
    ind[0] = -1                                                         # scene 0: no box assigned
    if G >= 3:
        ind[2, rng.random(G) < 0.3] = -1
        ind[2, 1], ind[2, 2] = -1, HW                                   # unassigned: -1 and an index past the map
    anno = np.where(((ind >= 0) & (ind < HW))[..., None], _lattice(rng, (B, G, na), -2.0, 2.0), F(0)).astype(F)
    maps = {nm: _lattice(rng, (B, ch, H, W), -2.0, 2.0) for nm, ch in zip(CENTER_MAPS, CENTER_CH)}
    if not vel:
        maps["vel"] = None
    kw = dict(code_weights=tuple(float(F(v)) for v in np.linspace(0.5, 1.5, na)), scale=(1.0, 0.25), normalize=True)
    if name == "c:shared":
        # scene 1: boxes 0, 1, 2, 4 share cell 9 with signs + + + - in column 0; the gradient there is +-(1/3)/4 * 0.75 ... per
        # box: partial sums that are odd multiples round, so the order of the additions shows (see test_dense_loss_cpu)
        kw = dict(code_weights=(float(SHARED_CW),) * 8, scale=(1.0, 1.0), normalize=False)
        ind[1] = (9, 9, 9, 3, 9, HW)
        ind[2] = (5, 5, 20, 20, 20, -1)
        anno[:] = 0
        maps["reg"][:] = 1.0                                           # pred - anno > 0 ...
        anno[1, 4, :] = 3.0                                            # ... except for box 4 of scene 1: < 0
        anno[2, 3, 0], anno[2, 4, 1] = 3.0, 1.0                        # signs + - + in column 0, + + 0 in column 1
        for nm in ("height", "dim", "rot"):
            maps[nm][:] = 1.0
    return dict(hm=x, heatmap=t, ind=ind, anno=anno, kw=kw, **maps)


@functools.lru_cache(maxsize=None)
def _case(name):
    c = _anchor_case(name) if name in ANCHOR_SHAPES else _center_case(name)
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


def case(name):
    """The inputs of a named case (read-only arrays, nchw)."""
    return _case(name)


def loss(c, form="vec"):
    anchor = "labels" in c
    if form == "loop":
        return anchor_loss_loop(c) if anchor else center_loss_loop(c)
    return (anchor_loss_vec if anchor else center_loss_vec)(c, D if form == "f64" else F)


def unnormalised(c):
    """The case with normalize = False (wq_i = scale_i): the library-function outputs keep their natural size, far above the
    absolute part of §9's tolerance, whatever the number of positives."""
    return dict(c, kw=dict(c["kw"], normalize=False))


@functools.lru_cache(maxsize=None)
def expected(name, normalize=True):
    """{"f32": the vectorised float32 reference, "f64": the binary64 evaluation} of a named case (normalize=False: of
    `unnormalised(case(name))`), computed once."""
    c = case(name) if normalize else unnormalised(case(name))
    out = {"f32": loss(c), "f64": loss(c, "f64")}
    for r in out.values():
        for v in r.values():
            v.setflags(write=False)
    return out
