"""float32 numpy reference of SPEC.md §18 (three_nn, its weights, three_interpolate), written in the spec's operation
order.  numpy neither contracts nor reorders elementwise float32 operations, so these are the spec's bits."""
import numpy as np

F = np.float32


def d2_matrix(unknown, known):
    """[n,m] §1 squared distances, p = known[j], c = unknown[i]."""
    dx = known[None, :, 0] - unknown[:, None, 0]
    dy = known[None, :, 1] - unknown[:, None, 1]
    dz = known[None, :, 2] - unknown[:, None, 2]
    return (dx * dx + dy * dy) + dz * dz


def weights(dist2):
    """§18 weights from [.., 3] squared distances (+inf -> r = 0)."""
    with np.errstate(over="ignore"):
        r = F(1.0) / (np.sqrt(dist2) + F(1e-8))
    norm = (r[..., 0] + r[..., 1]) + r[..., 2]
    return (r / norm[..., None]).astype(F)


def three_nn(unknown, known, chunk=2048):
    """unknown [B,n,3], known [B,m,3] f32 -> (dist2 [B,n,3] f32, idx [B,n,3] int32, w [B,n,3] f32).
    Three passes of first-minimum argmin: ties go to the lowest j, the output is ascending in (d2, j)."""
    unknown = np.asarray(unknown, F)
    known = np.asarray(known, F)
    B, n, _ = unknown.shape
    m = known.shape[1]
    dist = np.full((B, n, 3), np.inf, F)
    idx = np.zeros((B, n, 3), np.int32)
    for b in range(B):
        for i0 in range(0, n, chunk):
            d = d2_matrix(unknown[b, i0:i0 + chunk], known[b])
            rows = np.arange(d.shape[0])
            for k in range(min(3, m)):
                j = np.argmin(d, axis=1)
                dist[b, i0:i0 + chunk, k] = d[rows, j]
                idx[b, i0:i0 + chunk, k] = j
                d[rows, j] = np.inf
    return dist, idx, weights(dist)


def three_nn_lexsort(unknown, known):
    """The same selection by a full lexicographic sort on (d2, j) (slow; the check of ``three_nn``)."""
    B, n, _ = unknown.shape
    m = known.shape[1]
    dist = np.full((B, n, 3), np.inf, F)
    idx = np.zeros((B, n, 3), np.int32)
    for b in range(B):
        d = d2_matrix(unknown[b], known[b])
        j = np.broadcast_to(np.arange(m), d.shape)
        for i in range(n):
            order = np.lexsort((j[i], d[i]))[:3]
            dist[b, i, :len(order)] = d[i, order]
            idx[b, i, :len(order)] = order
    return dist, idx


def in_range(idx, m):
    """[B,n,3] bool: the slots whose index names a known point; §18: any other slot reads a zero feature and gets no gradient."""
    return (idx >= 0) & (idx < m)


def three_interpolate_pm(feat_pm, idx, w):
    """feat [B,m,C], idx / w [B,n,3] -> [B,n,C]: (w0*f0 + w1*f1) + w2*f2, every operation rounded; a slot whose index lies
    outside [0, m) reads a zero feature (its product w * 0 is still formed)."""
    out = np.empty((idx.shape[0], idx.shape[1], feat_pm.shape[2]), F)
    ok = in_range(idx, feat_pm.shape[1])
    for b in range(idx.shape[0]):
        f = [np.where(ok[b, :, k:k + 1], feat_pm[b][np.where(ok[b, :, k], idx[b, :, k], 0)], F(0)) for k in range(3)]
        ww = [w[b, :, k:k + 1] for k in range(3)]
        out[b] = (ww[0] * f[0] + ww[1] * f[1]) + ww[2] * f[2]
    return out


def three_interpolate_grad_pm(grad_pm, idx, w, m):
    """binary64 sum of the terms w_k * grad (and of their magnitudes) over the slots whose index lies in [0, m):
    ([B,m,C], [B,m,C])."""
    B, n, C = grad_pm.shape
    ref = np.zeros((B, m, C), np.float64)
    mag = np.zeros((B, m, C), np.float64)
    ok = in_range(idx, m)
    for b in range(B):
        for k in range(3):
            t = (w[b, :, k:k + 1].astype(np.float64) * grad_pm[b].astype(np.float64))[ok[b, :, k]]
            np.add.at(ref[b], idx[b, ok[b, :, k], k], t)
            np.add.at(mag[b], idx[b, ok[b, :, k], k], np.abs(t))
    return ref, mag
