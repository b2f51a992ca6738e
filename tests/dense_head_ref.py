"""Numpy float32 reference of SPEC.md §25 (dense head decode), every operation written out in the section's order and
rounded on its own, in two forms that must agree bit for bit: `*_loop` (one row at a time, np.float32 scalars) and `*_vec`
(whole arrays).  Plus the named cases the CPU and GPU tests share: tests/test_dense_head_cpu.py asserts on the reference
the coverage the GPU cases rely on; tests/test_gpu_dense_head.py compares the kernels with `expected(name)`.

Maps are kept in nchw; `to_nhwc` gives the permuted copy.  Results carry an `aux` dict (direction bin, q, v, ties, peak
masks) that only the coverage statements read."""
import functools

import numpy as np

F = np.float32
NINF = F(-np.inf)
DIR_OFFSET = 0.78539
KITTI_RANGE = (0.0, -40.0, -3.0, 70.4, 40.0, 1.0)


def period_of(nb):
    return F(2.0 * np.pi / nb)                   # in double, rounded once


def to_nhwc(m):
    return None if m is None else np.ascontiguousarray(m.transpose(0, 2, 3, 1))


def anchor_grid(point_range, H, W):
    """(origin, step) as dense_head.anchor_grid: corner aligned, computed in double, rounded once."""
    lo_x, lo_y, hi_x, hi_y = (float(point_range[i]) for i in (0, 1, 3, 4))
    sx = (hi_x - lo_x) / (W - 1) if W > 1 else 0.0
    sy = (hi_y - lo_y) / (H - 1) if H > 1 else 0.0
    return (float(F(lo_x)), float(F(lo_y))), (float(F(sx)), float(F(sy)))


def _gather(full, index, D):
    """Rows index[b, p] of the full decode; an entry outside [0, K) gives (0..., -inf, -1)."""
    boxes, scores, labels = full
    B, K = scores.shape
    index = np.asarray(index, np.int64)
    ok = (index >= 0) & (index < K)
    safe = np.where(ok, index, 0)
    bi = np.arange(B)[:, None]
    gb = np.where(ok[..., None], boxes[bi, safe], F(0)).astype(F)
    gs = np.where(ok, scores[bi, safe], NINF).astype(F)
    gl = np.where(ok, labels[bi, safe], -1).astype(np.int32)
    return gb, gs, gl


# ---- §25.1 ------------------------------------------------------------------------------------------------------------
def anchor_decode_vec(cls, reg, dir, sizes, z_center, rotations, origin, step, dir_offset=DIR_OFFSET, dir_limit_offset=0.0,
                      index=None, want_aux=False):
    with np.errstate(over="ignore", under="ignore"):
        sizes = np.asarray(sizes, F).reshape(-1, 3)
        zc, rots = np.asarray(z_center, F).reshape(-1), np.asarray(rotations, F).reshape(-1)
        ns, nr = len(sizes), len(rots)
        A = ns * nr
        B, _, H, W = cls.shape
        C = cls.shape[1] // A
        x0, y0, sx, sy = F(origin[0]), F(origin[1]), F(step[0]), F(step[1])
        doff, dlim = F(dir_offset), F(dir_limit_offset)
        c5 = cls.reshape(B, A, C, H, W).transpose(0, 3, 4, 1, 2)               # [B,H,W,A,C]
        t = reg.reshape(B, A, 7, H, W).transpose(0, 3, 4, 1, 2)                # [B,H,W,A,7]
        xa = (x0 + (np.arange(W).astype(F) * sx))[None, None, :, None]
        ya = (y0 + (np.arange(H).astype(F) * sy))[None, :, None, None]
        s_of = np.arange(A) // nr
        r_of = np.arange(A) % nr
        la, wa, ha = sizes[s_of, 0], sizes[s_of, 1], sizes[s_of, 2]
        za, ra = zc[s_of], rots[r_of]
        dg = np.sqrt((la * la) + (wa * wa))
        boxes = np.empty((B, H, W, A, 7), F)
        boxes[..., 0] = (t[..., 0] * dg) + xa
        boxes[..., 1] = (t[..., 1] * dg) + ya
        boxes[..., 2] = (t[..., 2] * ha) + za
        boxes[..., 3] = np.exp(t[..., 3]) * la
        boxes[..., 4] = np.exp(t[..., 4]) * wa
        boxes[..., 5] = np.exp(t[..., 5]) * ha
        r = t[..., 6] + ra
        aux = {}
        if dir is not None:
            nb = dir.shape[1] // A
            d5 = dir.reshape(B, A, nb, H, W).transpose(0, 3, 4, 1, 2)
            bins = np.argmax(d5, -1)                                           # first of the maxima; -0.0 == +0.0
            period = period_of(nb)
            v = r - doff
            q = np.floor((v / period) + dlim)
            rot = v - (q * period)
            yaw = (rot + doff) + (period * bins.astype(F))
            aux.update(bin=bins.reshape(B, -1), q=q.reshape(B, -1), v=v.reshape(B, -1),
                       dir_ties=((d5 == d5.max(-1, keepdims=True)).sum(-1) > 1).reshape(B, -1))
        else:
            yaw = r
        boxes[..., 6] = yaw
        m = c5.max(-1)
        labels = np.argmax(c5, -1).astype(np.int32)
        scores = F(1) / (F(1) + np.exp(-m))
        aux["cls_ties"] = ((c5 == m[..., None]).sum(-1) > 1).reshape(B, -1)
        out = boxes.reshape(B, -1, 7), scores.reshape(B, -1).astype(F), labels.reshape(B, -1)
        if index is not None:
            out = _gather(out, index, 7)
        return out + (aux,) if want_aux else out


def _anchor_row(cls, reg, dir, b, k, W, A, C, nb, nr, sizes, zc, rots, x0, y0, sx, sy, doff, dlim, period):
    cell, a = divmod(k, A)
    y, x = divmod(cell, W)
    s, r_ = divmod(a, nr)
    xa = x0 + (F(x) * sx)
    ya = y0 + (F(y) * sy)
    la, wa, ha = sizes[s]
    za, ra = zc[s], rots[r_]
    dg = np.sqrt((la * la) + (wa * wa))
    t = [reg[b, a * 7 + j, y, x] for j in range(7)]
    box = [(t[0] * dg) + xa, (t[1] * dg) + ya, (t[2] * ha) + za, np.exp(t[3]) * la, np.exp(t[4]) * wa, np.exp(t[5]) * ha]
    yaw = t[6] + ra
    if nb:
        bin_, best = 0, dir[b, a * nb, y, x]
        for d in range(1, nb):
            val = dir[b, a * nb + d, y, x]
            if val > best:
                best, bin_ = val, d
        v = yaw - doff
        q = np.floor((v / period) + dlim)
        rot = v - (q * period)
        yaw = (rot + doff) + (period * F(bin_))
    box.append(yaw)
    m, label = cls[b, a * C, y, x], 0
    for c in range(1, C):
        val = cls[b, a * C + c, y, x]
        if val > m:
            m, label = val, c
    return box, F(1) / (F(1) + np.exp(-m)), label


def anchor_decode_loop(cls, reg, dir, sizes, z_center, rotations, origin, step, dir_offset=DIR_OFFSET, dir_limit_offset=0.0,
                       index=None):
    with np.errstate(over="ignore", under="ignore"):
        sizes = np.asarray(sizes, F).reshape(-1, 3)
        zc, rots = np.asarray(z_center, F).reshape(-1), np.asarray(rotations, F).reshape(-1)
        ns, nr = len(sizes), len(rots)
        A = ns * nr
        B, _, H, W = cls.shape
        C = cls.shape[1] // A
        nb = 0 if dir is None else dir.shape[1] // A
        K = H * W * A
        rows = [list(range(K))] * B if index is None else [[int(k) for k in index[b]] for b in range(B)]
        R = len(rows[0])
        boxes, scores, labels = np.zeros((B, R, 7), F), np.full((B, R), NINF, F), np.full((B, R), -1, np.int32)
        args = (W, A, C, nb, nr, sizes, zc, rots, F(origin[0]), F(origin[1]), F(step[0]), F(step[1]), F(dir_offset),
                F(dir_limit_offset), period_of(nb) if nb else F(0))
        for b in range(B):
            for p, k in enumerate(rows[b]):
                if 0 <= k < K:
                    box, scores[b, p], labels[b, p] = _anchor_row(cls, reg, dir, b, k, *args)
                    boxes[b, p] = box
        return boxes, scores, labels


# ---- §25.2 ------------------------------------------------------------------------------------------------------------
def peak_mask(hm):
    """[B,C,H,W] bool: hm >= every in-image 8-neighbour (out-of-image neighbours do not exist)."""
    B, C, H, W = hm.shape
    ok = np.ones(hm.shape, bool)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if dy == 0 and dx == 0:
                continue
            ys, xs = slice(max(0, -dy), H - max(0, dy)), slice(max(0, -dx), W - max(0, dx))
            yn, xn = slice(max(0, dy), H - max(0, -dy)), slice(max(0, dx), W - max(0, -dx))
            ok[:, :, ys, xs] &= hm[:, :, ys, xs] >= hm[:, :, yn, xn]
    return ok


def center_decode_vec(hm, reg, height, dim, rot, vel, origin, cell, log_dim=True, peak=False, index=None, want_aux=False):
    with np.errstate(over="ignore", under="ignore"):
        B, C, H, W = hm.shape
        D = 9 if vel is not None else 7
        lo_x, lo_y, sx, sy = F(origin[0]), F(origin[1]), F(cell[0]), F(cell[1])
        boxes = np.empty((B, H, W, D), F)
        xs = np.arange(W).astype(F)[None, None, :]
        ys = np.arange(H).astype(F)[None, :, None]
        boxes[..., 0] = ((xs + reg[:, 0]) * sx) + lo_x
        boxes[..., 1] = ((ys + reg[:, 1]) * sy) + lo_y
        boxes[..., 2] = height[:, 0]
        d = dim.transpose(0, 2, 3, 1)
        boxes[..., 3:6] = np.exp(d) if log_dim else d
        boxes[..., 6] = np.arctan2(rot[:, 0], rot[:, 1])
        if vel is not None:
            boxes[..., 7:9] = vel.transpose(0, 2, 3, 1)
        h = hm.transpose(0, 2, 3, 1)                                           # [B,H,W,C]
        part = peak_mask(hm).transpose(0, 2, 3, 1) if peak else np.ones(h.shape, bool)
        masked = np.where(part, h, NINF)
        anyp = part.any(-1)
        m = masked.max(-1)
        # the lowest participating class that attains m (a participating -inf logit still counts)
        labels = np.where(anyp, np.argmax(part & (masked == m[..., None]), -1), -1).astype(np.int32)
        scores = np.where(anyp, F(1) / (F(1) + np.exp(-np.where(anyp, m, F(0)))), F(0)).astype(F)
        aux = dict(part=part.reshape(B, -1, C), none=(~anyp).reshape(B, -1))
        out = boxes.reshape(B, -1, D), scores.reshape(B, -1), labels.reshape(B, -1)
        if index is not None:
            out = _gather(out, index, D)
        return out + (aux,) if want_aux else out


def center_decode_loop(hm, reg, height, dim, rot, vel, origin, cell, log_dim=True, peak=False, index=None):
    with np.errstate(over="ignore", under="ignore"):
        B, C, H, W = hm.shape
        D = 9 if vel is not None else 7
        K = H * W
        lo_x, lo_y, sx, sy = F(origin[0]), F(origin[1]), F(cell[0]), F(cell[1])
        rows = [list(range(K))] * B if index is None else [[int(k) for k in index[b]] for b in range(B)]
        R = len(rows[0])
        boxes, scores, labels = np.zeros((B, R, D), F), np.full((B, R), NINF, F), np.full((B, R), -1, np.int32)
        for b in range(B):
            for p, k in enumerate(rows[b]):
                if not 0 <= k < K:
                    continue
                y, x = divmod(k, W)
                box = [((F(x) + reg[b, 0, y, x]) * sx) + lo_x, ((F(y) + reg[b, 1, y, x]) * sy) + lo_y, height[b, 0, y, x]]
                box += [np.exp(dim[b, j, y, x]) if log_dim else dim[b, j, y, x] for j in range(3)]
                box.append(np.arctan2(rot[b, 0, y, x], rot[b, 1, y, x]))
                if vel is not None:
                    box += [vel[b, 0, y, x], vel[b, 1, y, x]]
                m, label = F(0), -1
                for c in range(C):
                    v = hm[b, c, y, x]
                    part = True
                    if peak:
                        for dy in (-1, 0, 1):
                            for dx in (-1, 0, 1):
                                yy, xx = y + dy, x + dx
                                if (dy or dx) and 0 <= yy < H and 0 <= xx < W and not v >= hm[b, c, yy, xx]:
                                    part = False
                    if part and (label < 0 or v > m):
                        m, label = v, c
                boxes[b, p] = box
                scores[b, p] = F(0) if label < 0 else F(1) / (F(1) + np.exp(-m))
                labels[b, p] = label
        return boxes, scores, labels


# ---- cases --------------------------------------------------------------------------------------------------------------
def _anchor_cfg(ns, nr, rng):
    sizes = np.stack([rng.uniform(0.5, 5.0, ns), rng.uniform(0.4, 2.5, ns), rng.uniform(1.0, 3.0, ns)], 1).astype(F)
    if ns == 3:
        sizes = np.array([[3.9, 1.6, 1.56], [0.8, 0.6, 1.73], [1.76, 0.6, 1.73]], F)
    zc = rng.uniform(-1.5, 0.5, ns).astype(F)
    rots = (np.arange(nr) * (np.pi / nr)).astype(F) if nr > 1 else np.zeros(1, F)
    return sizes, zc, rots


#          name            H   W    B  ns nr  C   nb
ANCHOR_SHAPES = {
    "a:1x1":        (1, 1, 1, 1, 1, 1, 0),
    "a:5x7":        (5, 7, 3, 3, 2, 3, 2),
    "a:3x67:128":   (3, 67, 1, 16, 8, 10, 4),
    "a:9x130":      (9, 130, 3, 3, 2, 3, 2),
    "a:9x130:c10":  (9, 130, 1, 1, 1, 10, 0),
    "a:5x7:128":    (5, 7, 1, 16, 8, 1, 4),
    "a:3x67:c10":   (3, 67, 3, 3, 2, 10, 0),
    "a:1x1:b3":     (1, 1, 3, 3, 2, 3, 4),
    "a:5x7:a1":     (5, 7, 1, 1, 1, 3, 2),
    "a:3x67:a1":    (3, 67, 1, 1, 1, 1, 2),
    "a:3x67:a9":    (3, 67, 1, 3, 3, 10, 2),       # a partial last chunk behind a full one: 8 + 1 anchors, the last tile 9 cells
    "a:5x7:a11":    (5, 7, 3, 11, 1, 3, 2),        # 8 + 3 anchors, fewer cells than one tile
}
#          name            H   W    B  C  vel    log    peak
CENTER_SHAPES = {
    "c:1x1":        (1, 1, 1, 1, False, True, False),
    "c:5x7":        (5, 7, 3, 3, True, True, True),
    "c:3x67":       (3, 67, 1, 10, False, False, True),
    "c:9x130":      (9, 130, 3, 3, True, True, False),
    "c:9x130:peak": (9, 130, 1, 1, True, False, True),
    "c:1x1:peak":   (1, 1, 3, 3, False, True, True),
}
LATTICE = np.arange(-4.0, 4.0 + 1e-9, 0.25).astype(F)


def _seed(name):
    return int.from_bytes(name.encode(), "little") % (2 ** 31)


def _random_anchor(name, H, W, B, ns, nr, C, nb):
    rng = np.random.default_rng(_seed(name))
    A = ns * nr
    sizes, zc, rots = _anchor_cfg(ns, nr, rng)
    origin, step = anchor_grid(KITTI_RANGE, max(H, 2) * 8, max(W, 2) * 8)
    cls = rng.standard_normal((B, A * C, H, W)).astype(F) * F(2)
    reg = (rng.standard_normal((B, A * 7, H, W)) * 0.5).astype(F)
    reg[:, 6::7] = rng.uniform(-7.0, 7.0, (B, A, H, W)).astype(F)           # yaw residuals over several periods: q != 0
    dir_ = rng.standard_normal((B, A * nb, H, W)).astype(F) if nb else None
    return dict(cls=cls, reg=reg, dir=dir_, kw=dict(sizes=sizes, z_center=zc, rotations=rots, origin=origin, step=step,
                                                    dir_offset=DIR_OFFSET, dir_limit_offset=0.0))


def _find_t6(target_v, doff):
    """A float32 t6 with (t6 - doff) == target_v exactly (rotation 0), searched among the neighbours of target + doff."""
    t = F(target_v + doff)
    cands = [t]
    lo = hi = t
    for _ in range(16):
        lo, hi = np.nextafter(lo, F(-np.inf)), np.nextafter(hi, F(np.inf))
        cands += [lo, hi]
    for c in cands:
        if F(c - doff) == target_v:
            return c
    raise AssertionError(f"no float32 t6 gives v == {target_v!r}")


def _anchor_edges(dir_limit_offset):
    """(5,7), A = 6, C = 3, nb = 2, rotations (0, pi/2): the numeric edges of §25.1 planted in scene 0."""
    c = _random_anchor("a:edges", 5, 7, 2, 3, 2, 3, 2)
    c["kw"]["dir_limit_offset"] = dir_limit_offset
    # dir_offset 0.75 here: with 0.78539 (an odd number of quarter-ulps of [2, 4)) every r - dir_offset near pi is a rounding
    # tie that goes to the even neighbour, and float32 pi is odd: v == period could not occur at all
    c["kw"]["dir_offset"] = 0.75
    cls, reg, dir_ = c["cls"], c["reg"], c["dir"]
    doff, period = F(0.75), period_of(2)
    below = np.nextafter(period, F(0))
    # anchor 0 (rotation 0) of cells (0, 0..4): v = 0, period, one float below period, negative, -period
    for x, v in enumerate((F(0), period, below, F(-0.5), -period)):
        reg[0, 6, 0, x] = _find_t6(v, doff)
    # class ties: all equal; -0.0 vs +0.0 (both orders); the maximum twice
    cls[0, 0:3, 1, 0] = F(0.5)
    cls[0, 0:3, 1, 1] = (F(-0.0), F(0.0), F(-1.0))
    cls[0, 0:3, 1, 2] = (F(0.0), F(-0.0), F(-0.0))
    cls[0, 0:3, 1, 3] = (F(-1.0), F(2.0), F(2.0))
    # direction ties: equal, -0.0 vs +0.0 both ways
    dir_[0, 0:2, 2, 0] = F(1.25)
    dir_[0, 0:2, 2, 1] = (F(-0.0), F(0.0))
    dir_[0, 0:2, 2, 2] = (F(0.0), F(-0.0))
    # logits of +-200: score exactly 1 and exactly 0
    cls[0, 0:3, 3, 0] = (F(200.0), F(-200.0), F(0.0))
    cls[0, 0:3, 3, 1] = F(-200.0)
    # size residuals: 100 (+inf) and -110 (subnormal or zero)
    reg[0, 3:6, 3, 2] = F(100.0)
    reg[0, 3:6, 3, 3] = F(-110.0)
    return c


def _anchor_far():
    """Origins of 1e5: the anchor centre's rounding dominates."""
    c = _random_anchor("a:far", 5, 7, 1, 3, 2, 3, 2)
    c["kw"]["origin"] = (1e5, -1e5)
    return c


def _anchor_ties():
    """Logits on a coarse lattice: many class and direction ties, with both zeros."""
    c = _random_anchor("a:ties", 3, 67, 1, 3, 2, 3, 4)
    rng = np.random.default_rng(5)
    for key in ("cls", "dir"):
        q = rng.integers(-1, 2, c[key].shape).astype(F)
        q[(q == 0) & (rng.random(q.shape) < 0.5)] = F(-0.0)
        c[key] = q
    return c


def _random_center(name, H, W, B, C, vel, log_dim, peak):
    rng = np.random.default_rng(_seed(name))
    hm = rng.standard_normal((B, C, H, W)).astype(F) * F(2)
    if peak:
        hm = np.round(hm * 2) / 2                                             # a lattice: plateaus
        hm = hm.astype(F)
    c = dict(hm=hm, reg=rng.random((B, 2, H, W)).astype(F), height=rng.uniform(-2, 1, (B, 1, H, W)).astype(F),
             dim=(rng.standard_normal((B, 3, H, W)) * 0.5).astype(F) if log_dim else rng.uniform(0.3, 5, (B, 3, H, W)).astype(F),
             rot=rng.standard_normal((B, 2, H, W)).astype(F), vel=rng.standard_normal((B, 2, H, W)).astype(F) if vel else None,
             kw=dict(origin=(-54.0, -54.0), cell=(0.6, 0.6), log_dim=log_dim, peak=peak))
    return c


def _center_edges(vel, log_dim):
    """(5,7), C = 2, peak on: corner and edge peaks, a 2x2 plateau, a full-row plateau, a cell where no class is a peak,
    rot = (+-0, -1) and (0, 0)."""
    c = _random_center("c:edges", 5, 7, 2, 2, vel, log_dim, True)
    hm = c["hm"]
    hm[0] = F(-3.0)
    hm[0, 0, 0, 0] = hm[0, 0, 0, 6] = hm[0, 0, 4, 0] = hm[0, 0, 4, 6] = F(1.0)       # corners
    hm[0, 0, 0, 3] = hm[0, 0, 2, 0] = F(0.5)                                         # edges
    hm[0, 0, 2:4, 3:5] = F(2.0)                                                      # 2 x 2 plateau
    hm[0, 1, 2, :] = F(0.25)                                                         # full-row plateau of class 1
    hm[0, 1, 0, 1] = F(-2.5)                                                         # a lone peak of class 1 on the top edge
    hm[0, :, 1, 1] = F(-3.5)                                                         # below every neighbour in both classes: no peak
    c["rot"][0, :, 0, 0] = (F(0.0), F(-1.0))
    c["rot"][0, :, 0, 1] = (F(-0.0), F(-1.0))
    c["rot"][0, :, 0, 2] = (F(0.0), F(0.0))
    c["dim"][0, 0, 0, 3] = F(100.0) if log_dim else F(0.0)
    return c


@functools.lru_cache(maxsize=None)
def case(name):
    """-> dict(kind, maps..., kw).  Treat as read-only."""
    if name in ANCHOR_SHAPES:
        c = _random_anchor(name, *ANCHOR_SHAPES[name])
    elif name == "a:edges":
        c = _anchor_edges(0.0)
    elif name == "a:edges:half":
        c = _anchor_edges(0.5)
    elif name == "a:far":
        c = _anchor_far()
    elif name == "a:ties":
        c = _anchor_ties()
    elif name in CENTER_SHAPES:
        c = _random_center(name, *CENTER_SHAPES[name])
    elif name.startswith("c:edges"):
        c = _center_edges("vel" in name, "raw" not in name)
    elif name == "c:far":
        c = _random_center(name, 5, 7, 1, 3, True, True, False)
        c["kw"]["origin"] = (1e5, -1e5)
    else:
        raise KeyError(name)
    c["kind"] = "anchor" if name.startswith("a:") else "center"
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


ANCHOR_CASES = list(ANCHOR_SHAPES) + ["a:edges", "a:edges:half", "a:far", "a:ties"]
CENTER_CASES = list(CENTER_SHAPES) + ["c:edges", "c:edges:vel", "c:edges:raw", "c:far"]
ALL_CASES = ANCHOR_CASES + CENTER_CASES


def maps_of(c):
    return (c["cls"], c["reg"], c["dir"]) if c["kind"] == "anchor" else (c["hm"], c["reg"], c["height"], c["dim"], c["rot"], c["vel"])


def decode(c, form="vec", index=None, want_aux=False):
    fn = {("anchor", "vec"): anchor_decode_vec, ("anchor", "loop"): anchor_decode_loop,
          ("center", "vec"): center_decode_vec, ("center", "loop"): center_decode_loop}[c["kind"], form]
    extra = dict(want_aux=True) if want_aux else {}
    return fn(*maps_of(c), index=index, **c["kw"], **extra)


@functools.lru_cache(maxsize=None)
def expected(name):
    """(boxes, scores, labels, aux) of the full decode of a case, computed once.  Treat as read-only."""
    out = decode(case(name), want_aux=True)
    for v in out[:3]:
        v.setflags(write=False)
    return out


def rows_of_case(c):
    """K of a case."""
    if c["kind"] == "anchor":
        return c["cls"].shape[2] * c["cls"].shape[3] * len(c["kw"]["sizes"]) * len(c["kw"]["rotations"])
    return c["hm"].shape[2] * c["hm"].shape[3]


def rows_of(name):
    return rows_of_case(case(name))


def index_cases(name):
    """name -> {label: index[B,P] int32}: a permutation, duplicates, invalid entries (-1, K, 2^31 - 1) and P = 1."""
    K = rows_of(name)
    B = maps_of(case(name))[0].shape[0]
    rng = np.random.default_rng(K)
    perm = np.stack([rng.permutation(K) for _ in range(B)]).astype(np.int32)
    dup = rng.integers(0, K, (B, 300)).astype(np.int32)
    dup[:, 1::2] = dup[:, 0:-1:2]
    bad = rng.integers(0, K, (B, 257)).astype(np.int32)
    bad[:, 0], bad[:, 5], bad[:, 256], bad[:, 100] = -1, K, 2 ** 31 - 1, -(2 ** 31)
    one = np.full((B, 1), K - 1, np.int32)
    return dict(perm=perm, dup=dup, bad=bad, one=one)


# ---- the end-to-end case: AnchorHeadDecoder.predict ---------------------------------------------------------------
E2E_NMS = dict(iou_thr=0.3, score_thr=0.3, pre_max=400, post_max=150)


@functools.lru_cache(maxsize=None)
def e2e_case():
    """(3,67), A = 6, C = 3, nb = 2: class logits on LATTICE (neighbouring sigmoids differ by > 4e-3, so a 1e-4 error cannot
    reorder them and equal logits give equal scores), size residuals 0 (expf(0) = 1 exactly), anchors 0.4 m apart: crowded."""
    rng = np.random.default_rng(2025)
    B, H, W, ns, nr, C, nb = 2, 3, 67, 3, 2, 3, 2
    A = ns * nr
    sizes, zc, rots = _anchor_cfg(ns, nr, rng)
    cls = rng.choice(LATTICE, (B, A * C, H, W)).astype(F)
    reg = (rng.standard_normal((B, A * 7, H, W)) * 0.3).astype(F)
    for j in (3, 4, 5):
        reg[:, j::7] = F(0)
    reg[:, 6::7] = rng.uniform(-3.0, 3.0, (B, A, H, W)).astype(F)
    dir_ = rng.standard_normal((B, A * nb, H, W)).astype(F)
    kw = dict(sizes=sizes, z_center=zc, rotations=rots, origin=(0.0, -1.0), step=(0.4, 0.4), dir_offset=DIR_OFFSET,
              dir_limit_offset=0.0)
    return dict(kind="anchor", cls=cls, reg=reg, dir=dir_, kw=kw)
