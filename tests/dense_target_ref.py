"""Numpy float32 reference of SPEC.md §26 (dense head target assignment), every operation written out in the section's order
and rounded on its own, in two forms that must agree bit for bit: `*_loop` (the kernels' structure: one anchor row / one box
and one cell at a time, two passes for the anchor head) and `*_vec` (whole [K,G] arrays / slice maxima).  Plus the named
cases the CPU and GPU tests share: tests/test_dense_target_cpu.py asserts on the reference the coverage the GPU cases rely
on; tests/test_gpu_dense_target.py compares the kernels with `expected(name)`.

sin / cos of the centre head's anno come from the oracle's §13 routine (`oracle.sincos_r`), as tests/box_ref.py."""
import functools

import numpy as np

import dense_head_ref as dh

F = np.float32
PI, PI4, TWO_PI = F(np.pi), F(np.pi / 4), F(2 * np.pi)
MAXRAD = 64
DIR_OFFSET = dh.DIR_OFFSET


# ---- §26.1 ------------------------------------------------------------------------------------------------------------
def nearest_rect(cx, cy, l, w, yaw):
    """(x0, x1, y0, y1) of the nearest-BEV rectangle; float32 scalars or arrays."""
    n = np.floor((yaw / PI) + F(0.5))
    ang = np.abs(yaw - (n * PI))
    keep = ang < PI4
    ex, ey = np.where(keep, l, w), np.where(keep, w, l)
    hx, hy = ex * F(0.5), ey * F(0.5)
    return cx - hx, cx + hx, cy - hy, cy + hy


def rect_iou(a, g):
    ix = np.minimum(a[1], g[1]) - np.maximum(a[0], g[0])
    ix = np.where(ix > 0, ix, F(0))
    iy = np.minimum(a[3], g[3]) - np.maximum(a[2], g[2])
    iy = np.where(iy > 0, iy, F(0))
    inter = ix * iy
    area_a = (a[1] - a[0]) * (a[3] - a[2])
    area_g = (g[1] - g[0]) * (g[3] - g[2])
    den = np.maximum((area_a + area_g) - inter, F(1e-6))
    return inter / den


def _anchors(H, W, sizes, zc, rots, origin, step):
    """Per-row anchor columns [K] (xa, ya, za, la, wa, ha, ra) and the size index s [K], k = (y*W + x)*A + a."""
    ns, nr = len(sizes), len(rots)
    A = ns * nr
    x0, y0, sx, sy = F(origin[0]), F(origin[1]), F(step[0]), F(step[1])
    xa = (x0 + (np.arange(W).astype(F) * sx))
    ya = (y0 + (np.arange(H).astype(F) * sy))
    s_of, r_of = np.arange(A) // nr, np.arange(A) % nr
    K = H * W * A
    full = lambda v: np.broadcast_to(v, (H, W, A)).reshape(K).astype(v.dtype)      # noqa: E731
    return (full(xa[None, :, None]), full(ya[:, None, None]), full(zc[s_of][None, None]), full(sizes[s_of, 0][None, None]),
            full(sizes[s_of, 1][None, None]), full(sizes[s_of, 2][None, None]), full(rots[r_of][None, None]), full(s_of[None, None]))


def _cfg(sizes, z_center, rotations, pos_thr, neg_thr, size_class):
    sizes = np.asarray(sizes, F).reshape(-1, 3)
    ns = len(sizes)
    per = lambda v, dt: np.broadcast_to(np.asarray(v, dt).reshape(-1), (ns,)).copy()          # noqa: E731
    return (sizes, np.asarray(z_center, F).reshape(-1), np.asarray(rotations, F).reshape(-1), per(pos_thr, F), per(neg_thr, F),
            None if size_class is None else per(size_class, np.int32))


def _encode(out, b, k, box, anc, nb, doff, period):
    """Row k of scene b becomes a positive on `box` (float32 row): reg_target and dir_target."""
    xa, ya, za, la, wa, ha, ra = anc
    gx, gy, gz, gl, gw, gh, gyaw = (box[i] for i in range(7))
    dg = np.sqrt((la * la) + (wa * wa))
    t = out["reg_target"][b, k]
    t[0] = (gx - xa) / dg
    t[1] = (gy - ya) / dg
    t[2] = (gz - za) / ha
    t[3] = np.log(np.maximum(gl, F(1e-5)) / la)
    t[4] = np.log(np.maximum(gw, F(1e-5)) / wa)
    t[5] = np.log(np.maximum(gh, F(1e-5)) / ha)
    t[6] = gyaw - ra
    if nb:
        rg = t[6] + ra
        v = rg - doff
        o = v - (np.floor(v / TWO_PI) * TWO_PI)
        out["dir_target"][b, k] = min(max(int(np.floor(o / period)), 0), nb - 1)


def _anchor_out(B, K, G, nb):
    out = dict(labels=np.full((B, K), -1, np.int32), match=np.full((B, K), -1, np.int32), reg_target=np.zeros((B, K, 7), F),
               max_iou=np.zeros((B, K), F), best=np.zeros((B, G), F), forced=np.zeros((B, K), bool))
    if nb:
        out["dir_target"] = np.full((B, K), -1, np.int32)
    return out


def anchor_targets_vec(gt_boxes, gt_labels, H, W, sizes, z_center, rotations, origin, step, pos_thr, neg_thr, size_class=None, nb=0,
                       dir_offset=DIR_OFFSET):
    with np.errstate(all="ignore"):
        sizes, zc, rots, pos, neg, sc = _cfg(sizes, z_center, rotations, pos_thr, neg_thr, size_class)
        B, G = gt_labels.shape
        xa, ya, za, la, wa, ha, ra, s_of = _anchors(H, W, sizes, zc, rots, origin, step)
        K = len(xa)
        out = _anchor_out(B, K, G, nb)
        doff, period = F(dir_offset), dh.period_of(nb) if nb else F(0)
        arect = [v[:, None] for v in nearest_rect(xa, ya, la, wa, ra)]
        for b in range(B):
            gb, lab = gt_boxes[b], gt_labels[b]
            if G == 0:
                continue
            grect = [v[None, :] for v in nearest_rect(gb[:, 0], gb[:, 1], gb[:, 3], gb[:, 4], gb[:, 6])]
            iou = rect_iou(arect, grect).astype(F)                                      # [K,G]
            elig = (lab >= 0)[None, :] & (np.ones((K, G), bool) if sc is None else lab[None, :] == sc[s_of][:, None])
            masked = np.where(elig, iou, F(-1))
            j = np.where(elig.any(1), np.argmax(masked, 1), -1)                         # first of the maxima: the lowest g
            m = np.where(j >= 0, masked.max(1), F(0)).astype(F)
            best = np.where(elig, iou, F(0)).max(0)
            forced = (elig & (best[None, :] > 0) & (iou == best[None, :])).any(1)
            positive = forced | ((j >= 0) & (m >= pos[s_of]))
            back = ~positive & ((j < 0) | (m < neg[s_of]))
            out["max_iou"][b], out["best"][b], out["forced"][b] = m, best, forced
            out["labels"][b] = np.where(positive, lab[np.maximum(j, 0)], np.where(back, -1, -2))
            out["match"][b] = np.where(positive, j, -1)
            for k in np.nonzero(positive)[0]:
                _encode(out, b, k, gb[j[k]], (xa[k], ya[k], za[k], la[k], wa[k], ha[k], ra[k]), nb, doff, period)
        return out


def anchor_targets_loop(gt_boxes, gt_labels, H, W, sizes, z_center, rotations, origin, step, pos_thr, neg_thr, size_class=None, nb=0,
                        dir_offset=DIR_OFFSET):
    """The kernels' two passes, one anchor row at a time: pass 1 folds each row into a running best[g], pass 2 applies the rule."""
    with np.errstate(all="ignore"):
        sizes, zc, rots, pos, neg, sc = _cfg(sizes, z_center, rotations, pos_thr, neg_thr, size_class)
        B, G = gt_labels.shape
        ns, nr = len(sizes), len(rots)
        A = ns * nr
        K = H * W * A
        out = _anchor_out(B, K, G, nb)
        doff, period = F(dir_offset), dh.period_of(nb) if nb else F(0)
        x0, y0, sx, sy = F(origin[0]), F(origin[1]), F(step[0]), F(step[1])

        def anchor(k):
            cell, a = divmod(k, A)
            y, x = divmod(cell, W)
            s, r = divmod(a, nr)
            return s, (x0 + (F(x) * sx), y0 + (F(y) * sy), zc[s], sizes[s, 0], sizes[s, 1], sizes[s, 2], rots[r])

        for b in range(B):
            gb, lab = gt_boxes[b], gt_labels[b]
            grect = nearest_rect(gb[:, 0], gb[:, 1], gb[:, 3], gb[:, 4], gb[:, 6]) if G else None
            best = np.zeros(G, F)
            rows = []
            for k in range(K):                                                            # pass 1
                s, anc = anchor(k)
                if G == 0:
                    rows.append(None)
                    continue
                elig = (lab >= 0) if sc is None else (lab >= 0) & (lab == sc[s])
                iou = rect_iou(nearest_rect(anc[0], anc[1], anc[3], anc[4], anc[6]), grect).astype(F)
                best = np.maximum(best, np.where(elig, iou, F(0)))
                rows.append((elig, iou))
            out["best"][b] = best
            for k in range(K):                                                            # pass 2
                s, anc = anchor(k)
                m, j, forced = F(0), -1, False
                if G:
                    elig, iou = rows[k]
                    for g in np.nonzero(elig)[0]:
                        if j < 0 or iou[g] > m:
                            m, j = iou[g], int(g)
                        if best[g] > 0 and iou[g] == best[g]:
                            forced = True
                out["max_iou"][b, k], out["forced"][b, k] = m, forced
                if forced or (j >= 0 and m >= pos[s]):
                    out["labels"][b, k], out["match"][b, k] = lab[j], j
                    _encode(out, b, k, gb[j], anc, nb, doff, period)
                else:
                    out["labels"][b, k] = -1 if (j < 0 or m < neg[s]) else -2
        return out


# ---- §26.2 ------------------------------------------------------------------------------------------------------------
def gaussian_radius(hr, wr, mo):
    """CenterNet's gaussian_radius((height, width) = (hr, wr), min_overlap) in float32, its three roots in the source's order."""
    hw = hr + wr
    area = wr * hr
    c1 = (area * (F(1) - mo)) / (F(1) + mo)
    r1 = (hw + np.sqrt((hw * hw) - (F(4) * c1))) / F(2)
    b2 = F(2) * hw
    c2 = (F(1) - mo) * area
    r2 = (b2 + np.sqrt((b2 * b2) - (F(16) * c2))) / F(2)
    a3 = F(4) * mo
    b3 = (F(-2) * mo) * hw
    c3 = (mo - F(1)) * area
    r3 = (b3 + np.sqrt((b3 * b3) - ((F(4) * a3) * c3))) / F(2)
    return np.minimum(np.minimum(r1, r2), r3)


def _center_box(row, label, C, H, W, lo_x, lo_y, sx, sy, mo, min_radius):
    """None for an unassigned box, else (fx, fy, ix, iy, rad, den, r)."""
    if label < 0 or label >= C:
        return None
    fx, fy = (row[0] - lo_x) / sx, (row[1] - lo_y) / sy
    wr, hr = row[3] / sx, row[4] / sy
    if wr <= 0 or hr <= 0 or not (0 <= fx < F(W) and 0 <= fy < F(H)):
        return None
    ix, iy = int(np.floor(fx)), int(np.floor(fy))
    r = gaussian_radius(hr, wr, mo)
    rad = max(min_radius, int(np.minimum(r, F(MAXRAD))))
    sigma = F(2 * rad + 1) / F(6)
    return fx, fy, ix, iy, rad, (F(2) * sigma) * sigma, r


def _center_targets(form, gt_boxes, gt_labels, C, H, W, origin, cell, min_overlap=0.1, min_radius=2, vel=False):
    import oracle
    with np.errstate(all="ignore"):
        B, G = gt_labels.shape
        lo_x, lo_y, sx, sy, mo = F(origin[0]), F(origin[1]), F(cell[0]), F(cell[1]), F(min_overlap)
        na = 10 if vel else 8
        hm = np.zeros((B, C, H, W), F)
        ind, anno = np.full((B, G), -1, np.int32), np.zeros((B, G, na), F)
        rad_of, r_of = np.full((B, G), -1, np.int32), np.full((B, G), np.nan, F)
        sin, cos = oracle.sincos_r(np.ascontiguousarray(gt_boxes[..., 6].reshape(-1))) if G else (np.zeros(0, F), np.zeros(0, F))
        sin, cos = sin.reshape(B, G), cos.reshape(B, G)
        for b in range(B):
            for g in range(G):
                row, label = gt_boxes[b, g], int(gt_labels[b, g])
                bx = _center_box(row, label, C, H, W, lo_x, lo_y, sx, sy, mo, int(min_radius))
                if bx is None:
                    continue
                fx, fy, ix, iy, rad, den, r = bx
                ind[b, g], rad_of[b, g], r_of[b, g] = iy * W + ix, rad, r
                anno[b, g, :8] = (fx - F(ix), fy - F(iy), row[2], np.log(row[3]), np.log(row[4]), np.log(row[5]), sin[b, g], cos[b, g])
                if vel:
                    anno[b, g, 8:] = row[7:9]
                ys, xs = range(max(0, iy - rad), min(H, iy + rad + 1)), range(max(0, ix - rad), min(W, ix + rad + 1))
                if form == "loop":
                    for y in ys:
                        for x in xs:
                            d2 = (x - ix) * (x - ix) + (y - iy) * (y - iy)
                            v = np.exp(-F(d2) / den)
                            if v > hm[b, label, y, x]:
                                hm[b, label, y, x] = v
                else:
                    yy, xx = np.meshgrid(np.array(ys) - iy, np.array(xs) - ix, indexing="ij")
                    g2 = np.exp(-((xx * xx + yy * yy).astype(F)) / den).astype(F)
                    win = hm[b, label, ys.start:ys.stop, xs.start:xs.stop]
                    np.maximum(win, g2, out=win)
        return dict(heatmap=hm, ind=ind, anno=anno, rad=rad_of, r=r_of)


center_targets_loop = functools.partial(_center_targets, "loop")
center_targets_vec = functools.partial(_center_targets, "vec")


# ---- cases --------------------------------------------------------------------------------------------------------------
def _seed(name):
    return int.from_bytes(name.encode(), "little") % (2 ** 31)


def _pad(labels, rng):
    """A different number of padding rows per scene (scene b: its last ceil(b * G / 4) rows and a few scattered ones)."""
    B, G = labels.shape
    for b in range(B):
        if b and G:
            labels[b, G - (b * G + 3) // 4:] = -1
        if G > 8:
            labels[b, rng.integers(0, G, G // 8)] = -1
    return labels


#          name              H   W    B  ns nr  G    nb  size_class
ANCHOR_SHAPES = {
    "t:1x1":         (1, 1, 1, 1, 1, 1, 0, True),
    "t:5x7":         (5, 7, 3, 3, 2, 3, 2, True),
    "t:5x7:a1":      (5, 7, 1, 1, 1, 3, 2, True),
    "t:3x67:128":    (3, 67, 1, 16, 8, 65, 4, True),
    "t:9x130":       (9, 130, 3, 3, 2, 65, 2, True),
    "t:5x7:g1024":   (5, 7, 1, 3, 2, 1024, 0, True),
    "t:5x7:g0":      (5, 7, 2, 3, 2, 0, 2, True),
    "t:3x67:any":    (3, 67, 3, 3, 2, 65, 2, False),
    "t:3x67:a9":     (3, 67, 3, 3, 3, 65, 2, True),     # a partial last chunk behind a full one: 8 + 1 anchors, the last tile 9 cells
    "t:5x7:a11":     (5, 7, 1, 11, 1, 3, 2, True),      # 8 + 3 anchors, fewer cells than one tile
}


def _random_anchor(name, H, W, B, ns, nr, G, nb, per_class, origin_shift=(0.0, 0.0)):
    rng = np.random.default_rng(_seed(name))
    sizes, zc, rots = dh._anchor_cfg(ns, nr, rng)
    origin, step = dh.anchor_grid(dh.KITTI_RANGE, max(H, 2) * 8, max(W, 2) * 8)
    origin = (origin[0] + origin_shift[0], origin[1] + origin_shift[1])
    ncls = min(ns, 4)
    sc = (np.arange(ns) % ncls).astype(np.int32) if per_class else None
    # boxes near the anchors: the centre of a random cell plus a jitter, the extent of a random size of the class, any yaw
    lab = rng.integers(0, ncls, (B, G)).astype(np.int32)
    s_pick = lab if ns <= 4 else lab + ncls * rng.integers(0, ns // ncls, (B, G))
    gt = np.zeros((B, G, 7), np.float64)
    gt[..., 0] = origin[0] + (rng.integers(0, W, (B, G)) + rng.normal(0, 0.3, (B, G))) * step[0]
    gt[..., 1] = origin[1] + (rng.integers(0, H, (B, G)) + rng.normal(0, 0.3, (B, G))) * step[1]
    gt[..., 2] = rng.uniform(-2.0, 0.5, (B, G))
    gt[..., 3:6] = sizes[s_pick] * rng.uniform(0.7, 1.3, (B, G, 3))
    gt[..., 6] = rng.uniform(-7.0, 7.0, (B, G))
    # a quarter of the boxes stand exactly on an anchor with the anchor's extent and rotation: IoU 1
    on = rng.random((B, G)) < 0.25
    cx = (F(origin[0]) + (rng.integers(0, W, (B, G)).astype(F) * F(step[0]))).astype(F)
    cy = (F(origin[1]) + (rng.integers(0, H, (B, G)).astype(F) * F(step[1]))).astype(F)
    gt[..., 0], gt[..., 1] = np.where(on, cx, gt[..., 0]), np.where(on, cy, gt[..., 1])
    gt[..., 3:5] = np.where(on[..., None], sizes[s_pick][..., :2], gt[..., 3:5])
    gt[..., 6] = np.where(on, rots[rng.integers(0, nr, (B, G))], gt[..., 6])
    thr = rng.uniform(0.45, 0.7, ns).astype(F)
    return dict(gt_boxes=gt.astype(F), gt_labels=_pad(lab, rng),
                kw=dict(H=H, W=W, sizes=sizes, z_center=zc, rotations=rots, origin=origin, step=step, pos_thr=thr,
                        neg_thr=(thr - F(0.15)).astype(F), size_class=sc, nb=nb, dir_offset=DIR_OFFSET))


THIRD = float(F(4) / F(12))                      # the IoU of two 4 x 2 rectangles 2 apart along x: 4 / (8 + 8 - 4)


def _anchor_edges():
    """(5,7), steps of 2 from (0,0), sizes (4,2,1.5) for class 0 and (1.6,0.8,1.7) for class 1, rotations (0, pi/2), nb = 2."""
    up, dn = (lambda v: np.nextafter(F(v), F(np.inf))), (lambda v: np.nextafter(F(v), F(-np.inf)))
    q3 = F(PI - PI4)
    rows = [
        (4, 4, -1, 4, 2, 1.5, 0.0, 0),            # 0: equal to the anchor of cell (2,2), size 0, rotation 0; pos_thr = 1.0 (>=)
        (4, 4, -1, 4, 2, 1.5, 0.0, 0),            # 1: the same box again: a tie, the lowest g takes the anchor, both force it
        (10.5, 0.7, -1, 3.5, 1.8, 1.4, 0.1, 0),   # 2: its best anchor is below pos_thr: forced only
        (11.0, 7.3, -1, 0.5, 0.5, 1.0, 0.0, 0),   # 3: its best anchor is below neg_thr as well
        (100, 100, -1, 4, 2, 1.5, 0.0, 0),        # 4: far outside the grid: best = 0, forces nothing
        (0, 8, -1, 1.6, 0.8, 1.7, 0.0, 5),        # 5: a class no size takes
        (0, 0, -1, 1.6, 0.8, 1.7, dn(PI4), 1),    # 6, 7: yaw one float either side of PI4
        (2, 0, -1, 1.6, 0.8, 1.7, up(PI4), 1),
        (4, 0, -1, 1.6, 0.8, 1.7, dn(q3), 1),     # 8, 9: ... and of PI - PI4
        (6, 0, -1, 1.6, 0.8, 1.7, up(q3), 1),
        (8, 0, -1, 1.6, 0.8, 1.7, 0.3 + 6 * np.pi, 1),    # 10: several turns
        (10, 0.2, -1, 1.6, 0.8, 1.7, 0.3 - 8 * np.pi, 1), # 11: ... the other way
        (6, 6, -1, 4, 2, 1.5, 0.0, -1),           # 12: a padding row on an anchor
    ]
    a = np.array(rows, np.float64)
    sizes = np.array([[4, 2, 1.5], [1.6, 0.8, 1.7]], F)
    return dict(gt_boxes=a[None, :, :7].astype(F), gt_labels=a[None, :, 7].astype(np.int32),
                kw=dict(H=5, W=7, sizes=sizes, z_center=np.array([-1.0, -0.6], F), rotations=np.array([0, np.pi / 2], F),
                        origin=(0.0, 0.0), step=(2.0, 2.0), pos_thr=np.array([1.0, 0.6], F), neg_thr=np.array([THIRD, 0.45], F),
                        size_class=np.array([0, 1], np.int32), nb=2, dir_offset=DIR_OFFSET))


#          name              H   W    B  C  G    vel
CENTER_SHAPES = {
    "ct:1x1":        (1, 1, 1, 1, 1, False),
    "ct:5x7":        (5, 7, 3, 3, 3, True),
    "ct:3x67":       (3, 67, 1, 10, 65, False),
    "ct:9x130":      (9, 130, 3, 3, 65, True),
    "ct:40x37:g1024": (40, 37, 1, 2, 1024, False),
    "ct:5x7:g0":     (5, 7, 2, 3, 0, True),
}
CENTER_GEOM = dict(origin=(-54.0, -54.0), cell=(0.6, 0.6))


def _random_center(name, H, W, B, C, G, vel, origin=None, cell=None, inside=False):
    rng = np.random.default_rng(_seed(name))
    origin, cell = origin or CENTER_GEOM["origin"], cell or CENTER_GEOM["cell"]
    gt = np.zeros((B, G, 9 if vel else 7), np.float64)
    m = 0.0 if inside else 0.15                                             # some centres fall outside the map
    gt[..., 0] = origin[0] + rng.uniform(-m * W, (1 + m) * W, (B, G)) * cell[0]
    gt[..., 1] = origin[1] + rng.uniform(-m * H, (1 + m) * H, (B, G)) * cell[1]
    gt[..., 2] = rng.uniform(-2.0, 1.0, (B, G))
    gt[..., 3] = rng.uniform(0.4, 40.0, (B, G)) * cell[0]
    gt[..., 4] = rng.uniform(0.4, 20.0, (B, G)) * cell[1]
    gt[..., 5] = rng.uniform(1.0, 3.0, (B, G))
    gt[..., 6] = rng.uniform(-7.0, 7.0, (B, G))
    if vel:
        gt[..., 7:9] = rng.standard_normal((B, G, 2))
    lab = rng.integers(0 if inside else -1, C + (0 if inside else 1), (B, G)).astype(np.int32)      # -1 and C: padding
    return dict(gt_boxes=gt.astype(F), gt_labels=lab if inside else _pad(lab, rng),
                kw=dict(C=C, H=H, W=W, origin=origin, cell=cell, min_overlap=0.1, min_radius=2, vel=vel))


def _size_for_radius(target, side, cell):
    """A square box (in metres) whose float32 gaussian_radius is the float nearest to `target` from `side` (-1 below, +1 at or
    above), by bisection on the side length in cells: the radius grows with the size."""
    lo, hi = F(0.1), F(400.0)
    f = lambda n: gaussian_radius(F(n * F(cell)) / F(cell), F(n * F(cell)) / F(cell), F(0.1))      # noqa: E731
    for _ in range(80):
        mid = F((lo + hi) / F(2))
        if mid == lo or mid == hi:
            break
        if f(mid) < F(target):
            lo = mid
        else:
            hi = mid
    n = lo if side < 0 else hi
    assert (f(n) < F(target)) == (side < 0)
    return float(F(n * F(cell)))


def _center_edges():
    """(21,35): 2 x 3 tiles of 16 x 16.  origin (-4, 2), cells of 0.5: cell boundaries are exact."""
    H, W, C, cell = 21, 35, 2, 0.5
    lo_x, lo_y = -4.0, 2.0
    at = lambda ix, iy, dx=0.25, dy=0.25: (lo_x + (ix * cell) + dx, lo_y + (iy * cell) + dy)       # noqa: E731
    big = (3.0, 2.0)                                                          # 6 x 4 cells: radius above min_radius
    rows = []
    add = lambda xy, lw, label, yaw=0.3: rows.append((xy[0], xy[1], -0.5, lw[0], lw[1], 1.5, yaw, label))   # noqa: E731
    add(at(3, 0, 0.0, 0.0), big, 0)                                           # 0: exactly on a cell boundary and on lo_y
    add(at(W, 5, 0.0), big, 0)                                                # 1: exactly on hi_x: outside
    add(at(5, H, 0.25, 0.0), big, 1)                                          # 2: exactly on hi_y: outside
    s_lo, s_hi = _size_for_radius(4.0, -1, cell), _size_for_radius(4.0, +1, cell)
    add(at(8, 8), (s_lo, s_lo), 0)                                            # 3: radius one float below 4 -> 3
    add(at(24, 8), (s_hi, s_hi), 0)                                           # 4: radius at or above 4 -> 4
    add(at(17, 3), (0.5, 0.5), 1)                                             # 5: a one-cell box: min_radius takes over
    for ix, iy in ((0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1), (0, 10), (W - 1, 10), (17, 0), (17, H - 1)):
        add(at(ix, iy), big, 1)                                               # 6 - 13: windows clipped by corners and borders
    add(at(10, 15), big, 0)                                                   # 14, 15: one class, overlapping windows
    add(at(12, 15), (5.0, 4.0), 0)
    add(at(20, 5, 0.1, 0.1), big, 0)                                          # 16, 17: two boxes of a class in one cell
    add(at(20, 5, 0.4, 0.3), (6.0, 5.0), 0)
    add(at(28, 15), big, 0)                                                   # 18, 19: two classes in one cell
    add(at(28, 15, 0.3, 0.1), (1.0, 1.0), 1)
    add(at(15, 10), (0.0, 2.0), 0)                                            # 20, 21: l <= 0
    add(at(15, 10), (-1.0, 2.0), 0)
    add(at(15, 10), big, -1)                                                  # 22, 23: labels -1 and C
    add(at(15, 10), big, C)
    a = np.array(rows, np.float64)
    return dict(gt_boxes=a[None, :, :7].astype(F), gt_labels=a[None, :, 7].astype(np.int32),
                kw=dict(C=C, H=H, W=W, origin=(lo_x, lo_y), cell=(cell, cell), min_overlap=0.1, min_radius=2, vel=False))


def _center_round():
    """Round trip: every box inside the map, in a cell of its own (a map cell holds one box's anno)."""
    c = _random_center("ct:round", 40, 37, 2, 3, 40, True, inside=True)
    kw = c["kw"]
    gt, lab = c["gt_boxes"].copy(), c["gt_labels"].copy()
    for b in range(gt.shape[0]):
        seen = set()
        for g in range(gt.shape[1]):
            cellid = (int(np.floor((gt[b, g, 0] - F(kw["origin"][0])) / F(kw["cell"][0]))), int(np.floor((gt[b, g, 1] - F(kw["origin"][1])) / F(kw["cell"][1]))))
            if cellid in seen:
                lab[b, g] = -1
            seen.add(cellid)
    return dict(gt_boxes=gt, gt_labels=lab, kw=kw)


@functools.lru_cache(maxsize=None)
def case(name):
    """-> dict(kind, gt_boxes, gt_labels, kw).  Treat as read-only."""
    if name in ANCHOR_SHAPES:
        c = _random_anchor(name, *ANCHOR_SHAPES[name])
        if name == "t:1x1":                                                  # the one box overlaps the one anchor
            c["gt_boxes"][0, 0, :2] = (c["kw"]["origin"][0] + 0.3, c["kw"]["origin"][1] - 0.2)
    elif name == "t:edges":
        c = _anchor_edges()
    elif name == "t:far":
        c = _random_anchor(name, 5, 7, 1, 3, 2, 9, 2, True, origin_shift=(1e5, -1e5))
    elif name == "t:round":
        c = _random_anchor(name, 9, 11, 2, 3, 2, 12, 2, True)
    elif name in CENTER_SHAPES:
        c = _random_center(name, *CENTER_SHAPES[name], inside=name in ("ct:1x1", "ct:5x7"))
    elif name == "ct:edges":
        c = _center_edges()
    elif name == "ct:round":
        c = _center_round()
    else:
        raise KeyError(name)
    c["kind"] = "anchor" if name.startswith("t:") else "center"
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


ANCHOR_CASES = list(ANCHOR_SHAPES) + ["t:edges", "t:far", "t:round"]
CENTER_CASES = list(CENTER_SHAPES) + ["ct:edges", "ct:round"]
ALL_CASES = ANCHOR_CASES + CENTER_CASES


def targets(c, form="vec"):
    fn = {("anchor", "vec"): anchor_targets_vec, ("anchor", "loop"): anchor_targets_loop,
          ("center", "vec"): center_targets_vec, ("center", "loop"): center_targets_loop}[c["kind"], form]
    return fn(c["gt_boxes"], c["gt_labels"], **c["kw"])


@functools.lru_cache(maxsize=None)
def expected(name):
    """The outputs (and aux: best / forced, rad / r) of a case, computed once.  Treat as read-only."""
    out = targets(case(name))
    for v in out.values():
        v.setflags(write=False)
    return out


ANCHOR_OUTPUTS = ("labels", "match", "reg_target", "max_iou", "dir_target")
CENTER_OUTPUTS = ("heatmap", "ind", "anno")


def decode_maps(c, out):
    """The anchor head maps (cls zeros, reg, dir) in nchw that carry `reg_target` and a one-hot of `dir_target`."""
    kw = c["kw"]
    B = out["labels"].shape[0]
    H, W, nb = kw["H"], kw["W"], kw["nb"]
    A = len(kw["sizes"]) * len(kw["rotations"])
    reg = np.ascontiguousarray(out["reg_target"].reshape(B, H, W, A * 7).transpose(0, 3, 1, 2))
    onehot = (out["dir_target"][..., None] == np.arange(nb)).astype(F)          # [B,K,nb]; a non-positive row: all zero
    dir_ = np.ascontiguousarray(onehot.reshape(B, H, W, A * nb).transpose(0, 3, 1, 2))
    return np.zeros((B, A, H, W), F), reg, dir_


def center_maps(c, out):
    """The centre head maps (hm, reg, height, dim, rot, vel) in nchw with each assigned box's anno scattered to its cell."""
    kw = c["kw"]
    B, G = out["ind"].shape
    H, W = kw["H"], kw["W"]
    anno = out["anno"]
    maps = [np.zeros((B, ch, H * W), F) for ch in (2, 1, 3, 2, 2)]
    for b in range(B):
        for g in range(G):
            k = out["ind"][b, g]
            if k >= 0:
                for mp, cols in zip(maps, ((0, 1), (2,), (3, 4, 5), (6, 7), (8, 9))):
                    mp[b, :, k] = anno[b, g, list(cols)] if cols[-1] < anno.shape[-1] else 0
    reg, height, dim, rot, vel = (mp.reshape(B, -1, H, W) for mp in maps)
    hm = out["heatmap"] if out["heatmap"].shape[1] == kw["C"] else None
    return hm, reg, height, dim, rot, (vel if kw["vel"] else None)


# ---- the round trips through the §25 decoders (reference and device) ------------------------------------------------
def _close(got, want, what):
    err = np.abs(got.astype(np.float64) - want)
    assert (err <= 1e-4 + 1e-4 * np.abs(want)).all(), f"{what}: worst {float(err.max()):.3g}"


def check_anchor_round_trip(c, out, boxes):
    """`boxes` [B,K,7] decoded from decode_maps(c, out): every positive row is its matched ground-truth box."""
    pos = out["labels"] >= 0
    assert pos.sum() >= 10
    b, k = np.nonzero(pos)
    want = c["gt_boxes"][b, out["match"][b, k]].astype(np.float64)
    got = boxes[b, k]
    _close(got[:, :6], want[:, :6], "round trip box")
    d = (got[:, 6].astype(np.float64) - want[:, 6] + np.pi) % (2 * np.pi) - np.pi
    assert (np.abs(d) <= 1e-4 + 1e-4 * np.abs(want[:, 6])).all(), float(np.abs(d).max())


def check_center_round_trip(c, out, boxes):
    """`boxes` [B,P,D] decoded at index = ind from center_maps(c, out)."""
    ok = out["ind"] >= 0
    assert ok.sum() >= 30
    want, got = c["gt_boxes"][ok].astype(np.float64), boxes[ok]
    for j in (0, 1, 2, 3, 4, 5, 7, 8):
        _close(got[:, j], want[:, j], f"round trip column {j}")
    d = (got[:, 6].astype(np.float64) - want[:, 6] + np.pi) % (2 * np.pi) - np.pi
    assert (np.abs(d) <= 1e-4 + 1e-4 * np.abs(want[:, 6])).all(), float(np.abs(d).max())
