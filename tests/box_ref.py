"""float32 numpy reference of SPEC.md §19 (box operators), written in the spec's operation order.  numpy neither contracts
nor reorders elementwise float32 operations, and every scalar here is an np.float32, so these are the spec's bits.

sin / cos come from the oracle's §13 routine (``oracle.sincos_r``); the BEV IoU matrix is the oracle's ``iou_bev`` on the
expanded pairs; the 3-D IoU clips with the scalar ``clip_area`` below, whose BEV IoU equals the oracle's bit for bit
(tests/test_boxes_cpu.py)."""
import numpy as np

import oracle

F = np.float32
HALF, TWO, ZERO = F(0.5), F(2.0), F(0.0)


def box_consts(boxes, e=0.0):
    """§19.1 per-box constants of inside(p, box, e): (cx, cy, cz, hl, hw, hh, c, s), each [K] f32."""
    b = np.asarray(boxes, F)
    s, c = oracle.sincos_r(np.ascontiguousarray(b[:, 6]))
    e2 = TWO * F(e)
    L, W, H = b[:, 3] + e2, b[:, 4] + e2, b[:, 5] + e2
    return b[:, 0], b[:, 1], b[:, 2], HALF * L, HALF * W, HALF * H, c.astype(F), s.astype(F)


def local_coords(xyz, boxes, e=0.0):
    """(lx, ly, dz, hl, hw, hh) for every (point, box) pair: [N,K] arrays and [K] half extents."""
    cx, cy, cz, hl, hw, hh, c, s = box_consts(boxes, e)
    p = np.asarray(xyz, F)
    dx = p[:, None, 0] - cx[None]
    dy = p[:, None, 1] - cy[None]
    dz = p[:, None, 2] - cz[None]
    lx = dx * c[None] + dy * s[None]
    ly = dy * c[None] - dx * s[None]
    return lx, ly, dz, hl, hw, hh


def inside(xyz, boxes, e=0.0):
    """[N,K] bool: inside(xyz[n], boxes[k], e) of §19.1 (xy faces excluded, z faces included)."""
    lx, ly, dz, hl, hw, hh = local_coords(xyz, boxes, e)
    return (np.abs(dz) <= hh[None]) & (np.abs(lx) < hl[None]) & (np.abs(ly) < hw[None])


def face_hits(xyz, boxes, e=0.0):
    """(pairs exactly on an xy face, pairs exactly on a z face) of one scene: the boundary cases of the predicate."""
    lx, ly, dz, hl, hw, hh = local_coords(xyz, boxes, e)
    alx, aly, adz = np.abs(lx), np.abs(ly), np.abs(dz)
    xy = ((alx == hl) & (aly <= hw) | (aly == hw) & (alx <= hl)) & (adz <= hh)
    z = (adz == hh) & (alx < hl) & (aly < hw)
    return int(xy.sum()), int(z.sum())


def points_in_boxes(xyz, boxes, chunk=8192):
    """xyz [B,N,3], boxes [B,K,D] -> [B,N] int32: the lowest k containing the point, else -1."""
    B, N, _ = xyz.shape
    out = np.empty((B, N), np.int32)
    for b in range(B):
        for n0 in range(0, N, chunk):
            m = inside(xyz[b, n0:n0 + chunk], boxes[b])
            out[b, n0:n0 + chunk] = np.where(m.any(1), np.argmax(m, axis=1), -1)
    return out


def pool_counts(xyz, boxes, e, chunk=8192):
    """[B,K] number of points inside each enlarged box (all of them, not capped at S)."""
    B, N, _ = xyz.shape
    cnt = np.zeros(boxes.shape[:2], np.int64)
    for b in range(B):
        for n0 in range(0, N, chunk):
            cnt[b] += inside(xyz[b, n0:n0 + chunk], boxes[b], e).sum(0)
    return cnt


def roipoint_pool3d(xyz, feat, boxes, e, S):
    """xyz [B,N,3], feat [B,N,C] or None, boxes [B,K,D], extra width e (rounded to f32), S ->
    (pooled [B,K,S,3+C] f32, empty [B,K] int32, idx [B,K,S] int32)."""
    xyz = np.asarray(xyz, F)
    B, N, _ = xyz.shape
    K = boxes.shape[1]
    C = 0 if feat is None else feat.shape[2]
    rows = xyz if feat is None else np.concatenate([xyz, np.asarray(feat, F)], axis=2)
    pooled = np.zeros((B, K, S, 3 + C), F)
    empty = np.zeros((B, K), np.int32)
    idx = np.zeros((B, K, S), np.int32)
    e = F(e)
    for b in range(B):
        m = np.concatenate([inside(xyz[b, n0:n0 + 8192], boxes[b], e) for n0 in range(0, N, 8192)], axis=0)
        for k in range(K):
            sel = np.flatnonzero(m[:, k])[:S]
            if sel.size == 0:
                empty[b, k] = 1
                continue
            j = sel[np.arange(S) % sel.size]
            idx[b, k] = j
            pooled[b, k] = rows[b, j]
    return pooled, empty, idx


# ---- IoU ----------------------------------------------------------------------------------------------------
def corners(box, s, c):
    """§13 local corners (counter-clockwise) of one box row, the offsets from its own centre: ([4], [4]) lists of np.float32."""
    hl, hw = HALF * box[3], HALF * box[4]
    dx, dy = (hl, -hl, -hl, hl), (hw, hw, -hw, -hw)
    X, Y = [], []
    for k in range(4):
        X.append(c * dx[k] - s * dy[k])
        Y.append(s * dx[k] + c * dy[k])
    return X, Y


def pair_inter(a, ca, b, cb):
    """§13 clipped area of the pair (a, b) in b's frame: a's vertices are (a.centre - b.centre) + its local corners."""
    ddx, ddy = a[0] - b[0], a[1] - b[1]
    return clip_area([ddx + x for x in ca[0]], [ddy + y for y in ca[1]], cb[0], cb[1])


def clip_area(ax, ay, bx, by):
    """§13 Sutherland-Hodgman area of polygon a clipped against the four edges of b, scalar np.float32."""
    vx, vy = list(ax), list(ay)
    for e in range(4):
        if not vx:
            break
        q0x, q0y, q1x, q1y = bx[e], by[e], bx[(e + 1) & 3], by[(e + 1) & 3]
        ex, ey = q1x - q0x, q1y - q0y
        nx, ny = [], []
        ppx, ppy = vx[-1], vy[-1]
        cp = ex * (ppy - q0y) - ey * (ppx - q0x)
        for cx, cy in zip(vx, vy):
            cc = ex * (cy - q0y) - ey * (cx - q0x)
            ic, ip = cc >= ZERO, cp >= ZERO
            if ic != ip:
                t = cp / (cp - cc)
                nx.append(ppx + t * (cx - ppx))
                ny.append(ppy + t * (cy - ppy))
            if ic:
                nx.append(cx)
                ny.append(cy)
            ppx, ppy, cp = cx, cy, cc
        vx, vy = nx, ny
    n = len(vx)
    if n < 3:
        return ZERO
    sm = ZERO
    for i in range(n):
        j = (i + 1) % n
        sm = sm + (vx[i] * vy[j] - vx[j] * vy[i])
    return HALF * abs(sm)


def _corner_list(boxes):
    b = np.asarray(boxes, F)
    s, c = oracle.sincos_r(np.ascontiguousarray(b[:, 6]))
    return [corners(b[k], F(s[k]), F(c[k])) for k in range(b.shape[0])]


def iou_bev_pair(a, b):
    """§13 iou_bev of two box rows, scalar (the check of the clip the 3-D IoU uses)."""
    a, b = np.asarray(a, F), np.asarray(b, F)
    ca, cb = _corner_list(np.stack([a[:7], b[:7]]))
    inter = pair_inter(a, ca, b, cb)
    den = (F(a[3]) * F(a[4]) + F(b[3]) * F(b[4])) - inter
    return inter / den if den > ZERO else ZERO


def pad9(boxes):
    """[..., D] -> [..., 9] rows for the oracle (fields 7.. are not read by iou_bev)."""
    b = np.asarray(boxes, F)
    out = np.zeros(b.shape[:-1] + (9,), F)
    out[..., :7] = b[..., :7]
    return out


def iou_bev_matrix(a, b):
    """a [Ka,D], b [Kb,D] -> [Ka,Kb]: oracle.iou_bev(a_i, b_j) on the expanded pairs."""
    Ka, Kb = a.shape[0], b.shape[0]
    A = np.repeat(pad9(a), Kb, axis=0)
    Bm = np.tile(pad9(b), (Ka, 1))
    return oracle.iou_bev(A, Bm).reshape(Ka, Kb)


def iou3d_matrix(a, b):
    """a [Ka,D], b [Kb,D] -> [Ka,Kb]: §19.3 3-D IoU, in the spec's order (scalar clip: ~1e4 pairs per second)."""
    a, b = np.asarray(a, F), np.asarray(b, F)
    ca, cb = _corner_list(a), _corner_list(b)
    out = np.empty((a.shape[0], b.shape[0]), F)
    for i in range(a.shape[0]):
        A = a[i]
        ha = HALF * A[5]
        va = (A[3] * A[4]) * A[5]
        for j in range(b.shape[0]):
            Bx = b[j]
            inter = pair_inter(A, ca[i], Bx, cb[j])
            hb = HALF * Bx[5]
            top = min(A[2] + ha, Bx[2] + hb)
            bot = max(A[2] - ha, Bx[2] - hb)
            oh = top - bot
            oh = oh if oh > ZERO else ZERO
            i3 = inter * oh
            vb = (Bx[3] * Bx[4]) * Bx[5]
            den = (va + vb) - i3
            out[i, j] = i3 / den if den > ZERO else ZERO
    return out


def boxes_iou(a, b, mode):
    """a [B,Ka,Da], b [B,Kb,Db] -> [B,Ka,Kb] f32; mode "bev" or "3d"."""
    fn = iou_bev_matrix if mode == "bev" else iou3d_matrix
    return np.stack([fn(a[i], b[i]) for i in range(a.shape[0])])
