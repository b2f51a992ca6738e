"""Reference restatement of SPEC.md §21.4 (backward of the sparse convolution) in numpy.  Test infrastructure.

index   ``index_transpose_loop`` follows the definition literally; ``index_transpose_vec``, independent: a lexsort of the valid
        entries by (input row, offset, output row) and the first of every run.
values  ``grad_input``: the §21.2 fmaf chain over (g, nbrT, W^T) by ``spconv_ref.conv`` — bit for bit the definition.
        ``grad_weight``: float64 sums, with the sum of |terms| and the number of terms of every element (what the parity rule of
        §21.4 needs).  ``relu_mask``, ``to_dense_grad``: exact selections."""
import numpy as np

import spconv_ref as ref

F = np.float32


def index_transpose_loop(nbr, Nv):
    """-> (nbrT [Nv,Kvol] int32, collisions int)."""
    nbr = np.asarray(nbr, np.int32)
    No, Kvol = nbr.shape
    nbrT = np.full((Nv, Kvol), -1, np.int32)
    for o in range(No):
        for kk in range(Kvol):
            i = int(nbr[o, kk])
            if 0 <= i < Nv and nbrT[i, kk] < 0:                  # o ascending: the first one met is the lowest
                nbrT[i, kk] = o
    collisions = 0
    for o in range(No):
        for kk in range(Kvol):
            i = int(nbr[o, kk])
            if 0 <= i < Nv and nbrT[i, kk] != o:
                collisions += 1
    return nbrT, collisions


def index_transpose_vec(nbr, Nv):
    nbr = np.asarray(nbr, np.int64)
    No, Kvol = nbr.shape
    o, kk = np.nonzero((nbr >= 0) & (nbr < Nv))
    i = nbr[o, kk]
    order = np.lexsort((o, kk, i))                               # by i, then kk, then o
    i, kk, o = i[order], kk[order], o[order]
    key = i * Kvol + kk
    first = np.ones(len(key), bool)
    first[1:] = key[1:] != key[:-1]
    nbrT = np.full((Nv, Kvol), -1, np.int32)
    nbrT[i[first], kk[first]] = o[first]
    return nbrT, int(len(key) - first.sum())


def relu_mask(grad_out, out, relu):
    grad_out = np.asarray(grad_out, F)
    return np.where(np.asarray(out) > 0, grad_out, F(0)).astype(F) if relu else grad_out


def grad_input(g, nbrT, W):
    """§21.4: grad_feat [Nv,Cin] float32 = conv(g, nbrT, W^T), W [Kvol,Cout,Cin]."""
    return ref.conv(np.asarray(g, F), nbrT, np.ascontiguousarray(np.asarray(W, F).transpose(0, 2, 1)))


def grad_input_magnitude(g, nbrT, W):
    """float64 sum of |terms| of every element of ``grad_input`` (at most Kvol * Cout terms each)."""
    g, W = np.abs(np.asarray(g, np.float64)), np.abs(np.asarray(W, np.float64))
    gp = np.concatenate([g, np.zeros((1, g.shape[1]))])
    mag = np.zeros((len(nbrT), W.shape[2]))
    for kk in range(W.shape[0]):
        mag += gp[np.where(nbrT[:, kk] >= 0, nbrT[:, kk], len(g))] @ W[kk]
    return mag


def grad_weight(feat, nbr, g):
    """-> (grad_W [Kvol,Cout,Cin] float64, sum |terms| likewise, terms per kk [Kvol] int, grad_bias [Cout] float64,
    sum |g| [Cout] float64): every element of grad_W[kk] sums the same number of terms (the rows with a neighbour at kk),
    grad_bias sums No terms."""
    feat, g, nbr = np.asarray(feat, np.float64), np.asarray(g, np.float64), np.asarray(nbr)
    (No, Kvol), Cin, Cout = nbr.shape, feat.shape[1], g.shape[1]
    gw, mag, n = np.zeros((Kvol, Cout, Cin)), np.zeros((Kvol, Cout, Cin)), np.zeros(Kvol, np.int64)
    for kk in range(Kvol):
        o = np.flatnonzero((nbr[:, kk] >= 0) & (nbr[:, kk] < len(feat)))
        f = feat[nbr[o, kk]]
        gw[kk] = g[o].T @ f
        mag[kk] = np.abs(g[o]).T @ np.abs(f)
        n[kk] = len(o)
    return gw, mag, n, g.sum(0) if No else np.zeros(Cout), np.abs(g).sum(0) if No else np.zeros(Cout)


def grad_weight_bound(mag, n):
    """§21.4: |gpu - ref64| <= n * 2^-23 * sum |terms| per element; ``n`` per kk (or a scalar for grad_bias)."""
    n = np.asarray(n, np.float64)
    return (n.reshape((-1,) + (1,) * (mag.ndim - 1)) if n.ndim else n) * 2.0 ** -23 * mag


def lattice(shape, lim, seed):
    """Integers in [-lim, lim] as float32: with |g| <= 4 and |feat| <= 8 every partial sum of up to 2^19 products is an integer
    below 2^24, so binary32 sums them exactly in any order."""
    return np.random.default_rng(seed).integers(-lim, lim + 1, shape).astype(F)


def to_dense_grad(grad_dense, coors, offsets):
    """§21.4: grad_feat[o] = grad_dense[b,:,z,y,x] for the lowest row of a cell, zero for a shadowed duplicate."""
    grad_dense = np.asarray(grad_dense, F)
    sc = ref.scene_ids(offsets)
    out = np.zeros((len(coors), grad_dense.shape[1]), F)
    seen = set()
    for r in range(len(coors)):
        z, y, x = (int(v) for v in coors[r])
        key = (int(sc[r]), z, y, x)
        if key in seen:
            continue
        seen.add(key)
        out[r] = grad_dense[sc[r], :, z, y, x]
    return out
