"""Reference restatement of SPEC.md §22 (sparse max pool, its backward, inverse convolution) in numpy.  Test infrastructure.

pool      form A (``max_pool_loop``): §22.1 executed literally, row by row, channel by channel.  Form B (``max_pool_vec``),
          independent: the rows gathered from a table padded with one row of -inf, ``argmax`` over kk (the first maximum).
backward  ``max_pool_grad_loop``: §22.2 literally, a walk over nbrT with float32 additions in kk order.
          ``max_pool_grad_scatter``, independent: every g[o][c] scattered to row arg[o][c] and summed in float64 (exact, and
          equal to any float32 order, on exactly-summable inputs).
inverse   ``inverse_conv``: §22.3 is by definition ``spconv_ref.conv`` over the transposed rulebook; ``inverse_conv_check``:
          torch.nn.functional.conv_transpose3d on the densified input with the forward error bound ``conv3d_check`` uses."""
import numpy as np

import spconv_grad_ref as gref
import spconv_ref as ref

F = np.float32


def _valid(nbr, n):
    nbr = np.asarray(nbr)
    return (nbr >= 0) & (nbr < n)


def max_pool_loop(feat, nbr):
    """-> (out [No,C] float32, arg [No,C] int32)."""
    feat, nbr = np.asarray(feat, F), np.asarray(nbr, np.int32)
    (Nv, C), (No, Kvol) = feat.shape, nbr.shape
    out, arg = np.zeros((No, C), F), np.full((No, C), -1, np.int32)
    for o in range(No):
        for c in range(C):
            have = False
            for kk in range(Kvol):
                i = int(nbr[o, kk])
                if not 0 <= i < Nv:
                    continue
                if not have or feat[i, c] > out[o, c]:            # strictly greater: a tie (-0.0 against +0.0 too) keeps the first
                    out[o, c], arg[o, c], have = feat[i, c], i, True
    return out, arg


def max_pool_vec(feat, nbr):
    feat, nbr = np.asarray(feat, F), np.asarray(nbr, np.int64)
    (Nv, C), (No, Kvol) = feat.shape, nbr.shape
    ok = _valid(nbr, Nv)
    table = np.concatenate([feat, np.full((1, C), -np.inf, F)])
    rows = table[np.where(ok, nbr, Nv)]                            # [No,Kvol,C]
    kbest = rows.argmax(1)                                         # the first maximum along kk
    out = np.take_along_axis(rows, kbest[:, None, :], 1)[:, 0, :]
    arg = np.take_along_axis(np.where(ok, nbr, -1), kbest, 1).astype(np.int32)
    none = ~ok.any(1)
    out[none] = 0
    arg[none] = -1
    # (a row whose valid values are all -inf would pick a padded slot: the families hold finite values only)
    assert np.isfinite(out).all()
    return np.ascontiguousarray(out, F), arg


def max_pool_grad_loop(g, arg, nbrT):
    """-> grad_feat [Nv,C] float32."""
    g, arg, nbrT = np.asarray(g, F), np.asarray(arg, np.int32), np.asarray(nbrT, np.int32)
    (No, C), (Nv, Kvol) = g.shape, nbrT.shape
    out = np.zeros((Nv, C), F)
    for i in range(Nv):
        acc = np.zeros(C, F)
        for kk in range(Kvol):
            o = int(nbrT[i, kk])
            if 0 <= o < No:
                acc = np.where(arg[o] == i, (acc + g[o]).astype(F), acc)
        out[i] = acc
    return out


def max_pool_grad_scatter(g, arg, Nv):
    """float64 sums of g by arg -> [Nv,C] float64 (independent of nbrT: the true gradient when nothing collided)."""
    g, arg = np.asarray(g, np.float64), np.asarray(arg, np.int64)
    out = np.zeros((Nv, g.shape[1]))
    o, c = np.nonzero(arg >= 0)
    np.add.at(out, (arg[o, c], c), g[o, c])
    return out


def inverse_conv(feat, nbrT, W, bias=None, residual=None, relu=False):
    """§22.3: feat [No,Cin] on the rulebook's output rows, nbrT [Nv,Kvol], W [Kvol,Cout,Cin] -> out [Nv,Cout] float32."""
    return ref.conv(feat, nbrT, W, bias, residual, relu)


def inverse_grads(feat, nbr, nbrT, W, g):
    """§22.3 backward with the roles of §21.4 swapped: -> (grad_feat [No,Cin] float32, then ``grad_weight``'s five results)."""
    W = np.asarray(W, F)
    grad_feat = ref.conv(np.asarray(g, F), nbr, np.ascontiguousarray(W.transpose(0, 2, 1)))
    return (grad_feat,) + gref.grad_weight(feat, nbrT, g)


def inverse_conv_check(feat, out_coors, out_offsets, G, K, s, p, W, bias, out, coors, offsets):
    """``out`` [Nv,Cout] against conv_transpose3d(dense(feat on the output sites), w, stride, padding, output_padding) read at
    the input's active sites, w[ci,co,kz,ky,kx] = W[kk][co][ci]; within 2 * gamma(Kvol*Cin + 2) * sum |w.x|.  The input must be
    duplicate-free.  -> (largest err / bound, output_padding)."""
    import torch
    G, K, s, p, O = ref.geometry(G, K, s, p)
    W = np.asarray(W, F)
    Kvol, Cout, Cin = W.shape
    w5 = torch.from_numpy(np.ascontiguousarray(W.reshape(K[0], K[1], K[2], Cout, Cin).transpose(4, 3, 0, 1, 2)))     # [Cin,Cout,kz,ky,kx]
    opad = tuple(g - ((o - 1) * t - 2 * q + k) for g, o, t, q, k in zip(G, O, s, p, K))
    assert all(0 <= a < t for a, t in zip(opad, s)), opad
    x = torch.from_numpy(ref.to_dense(feat, out_coors, out_offsets, O))
    b = np.zeros(Cout, F) if bias is None else np.asarray(bias, F)
    y = torch.nn.functional.conv_transpose3d(x, w5, torch.from_numpy(b), stride=s, padding=p, output_padding=opad).numpy()
    mag = torch.nn.functional.conv_transpose3d(x.abs(), w5.abs(), torch.from_numpy(np.abs(b)), stride=s, padding=p, output_padding=opad).numpy()
    assert y.shape[2:] == G, (y.shape, G)
    sc = ref.scene_ids(offsets)
    z, yy, xx = coors[:, 0], coors[:, 1], coors[:, 2]
    want = y[sc, :, z, yy, xx]
    bound = 2.0 * ref.gamma(Kvol * Cin + 2) * mag[sc, :, z, yy, xx].astype(np.float64)
    err = np.abs(np.asarray(out, np.float64) - want.astype(np.float64))
    worst = float((err / np.maximum(bound, 1e-300)).max()) if err.size else 0.0
    assert (err <= bound).all(), f"conv_transpose3d cross-check: {int((err > bound).sum())} values outside the bound, worst {worst:.3g} x"
    return worst, opad


def dense_fill(feat, coors, offsets, shape, fill):
    """[B,C,z,y,x] holding ``fill`` where no voxel is (duplicate-free input)."""
    feat = np.asarray(feat, F)
    dense = np.full((len(offsets) - 1, feat.shape[1]) + tuple(shape), fill, F)
    sc = ref.scene_ids(offsets)
    dense[sc, :, coors[:, 0], coors[:, 1], coors[:, 2]] = feat
    return dense


def has_duplicates(coors, offsets):
    keys = np.concatenate([ref.scene_ids(offsets)[:, None], np.asarray(coors, np.int64)], 1)
    return len(np.unique(keys, axis=0)) < len(keys)


def strided_geometries():
    import spconv_cases as sc
    return [g for g in sc.GEOMETRIES if not g[4]]


def quantised_feat(n, c=4, seed=0, lo=-2, hi=2):
    """Integers in [lo, hi] as float32: many ties inside a window."""
    return np.random.default_rng(1000 + seed).integers(lo, hi + 1, (n, c)).astype(F)


def pool_coverage(feat, nbr, Nv):
    """What a pooling case exercises, from the reference alone -> dict of counts:
    ties = output elements whose maximum more than one valid neighbour attains; not_first = elements whose arg is not the row's
    first valid neighbour; uncovered = input rows no output row reads (nbrT[i,:] = -1); max_fanout = the most output elements of
    one channel that share an arg row (terms of the backward's in-order sum)."""
    feat, nbr = np.asarray(feat, F), np.asarray(nbr, np.int64)
    ok = _valid(nbr, Nv)
    out, arg = max_pool_vec(feat, nbr)
    table = np.concatenate([feat, np.full((1, feat.shape[1]), -np.inf, F)])
    rows = table[np.where(ok, nbr, Nv)]
    attained = (rows == out[:, None, :]) & ok[:, :, None]
    first_valid = np.where(ok.any(1), np.take_along_axis(nbr, ok.argmax(1)[:, None], 1)[:, 0], -1)
    nbrT, col = gref.index_transpose_vec(nbr, Nv)
    fan = np.zeros((Nv, feat.shape[1]), np.int64)
    o, c = np.nonzero(arg >= 0)
    np.add.at(fan, (arg[o, c], c), 1)
    return {"ties": int((attained.sum(1) > 1).sum()), "not_first": int(((arg != first_valid[:, None]) & (arg >= 0)).sum()),
            "uncovered": int((nbrT < 0).all(1).sum()), "max_fanout": int(fan.max()) if fan.size else 0, "collisions": col}
