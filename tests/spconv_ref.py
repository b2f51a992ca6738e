"""Reference restatement of SPEC.md §21 (sparse 3-D convolution) in numpy + the CPU oracle's §6 layer.  Test infrastructure.

index  form A (``index_loop``): a Python dict walk that follows §21.1 literally.  Form B (``index_vec``), independent: a dense
       lowest-row array per scene and array arithmetic.  ``active_sites``: the active output set a third way, as the sites whose
       window holds an active input (a strided OR over the padded occupancy = a dense max-pool).
values ``conv``: the plain rows of §21.2 built with numpy, one §6 layer by ``oracle.mlp_rows``, then residual and ReLU in
       float32: bit for bit the definition.  ``conv3d_check``: torch.nn.functional.conv3d on the densified input, with the
       derived forward error bound."""
import numpy as np

F = np.float32
INT_MAX = 2 ** 31 - 1


def geometry(G, K, s=(1, 1, 1), p=(0, 0, 0), subm=False):
    """-> (G, K, s, p, O) as tuples (z,y,x); subm fixes s = 1, p = K // 2."""
    G, K = tuple(int(x) for x in G), tuple(int(x) for x in K)
    if subm:
        assert all(k % 2 == 1 for k in K)
        s, p = (1, 1, 1), tuple(k // 2 for k in K)
    s, p = tuple(int(x) for x in s), tuple(int(x) for x in p)
    O = tuple((g + 2 * q - k) // t + 1 for g, q, k, t in zip(G, p, K, s))
    assert min(O) >= 1
    return G, K, s, p, O


def offsets_k(K):
    """[Kvol,3]: kernel offset kk = (kz*Ky + ky)*Kx + kx."""
    return np.array([(kz, ky, kx) for kz in range(K[0]) for ky in range(K[1]) for kx in range(K[2])], np.int64)


def index_loop(coors, offsets, G, K, s=(1, 1, 1), p=(0, 0, 0), subm=False):
    """§21.1 executed literally -> (out_coors [No,3] int32, out_offsets [B+1] int32, nbr [No,Kvol] int32)."""
    G, K, s, p, O = geometry(G, K, s, p, subm)
    ks = [tuple(int(v) for v in k) for k in offsets_k(K)]
    coors = np.asarray(coors, np.int64).reshape(-1, 3)
    offsets = [int(o) for o in offsets]
    out_coors, out_offsets, nbr = [], [0], []
    for b in range(len(offsets) - 1):
        first = {}
        for i in range(offsets[b], offsets[b + 1]):
            first.setdefault(tuple(int(v) for v in coors[i]), i)          # the lowest row owns a coordinate
        if subm:
            sites = [tuple(int(v) for v in coors[i]) for i in range(offsets[b], offsets[b + 1])]
        else:
            seen, sites = set(), []
            for i in range(offsets[b], offsets[b + 1]):
                for k in ks:
                    t = [int(coors[i][d]) + p[d] - k[d] for d in range(3)]
                    if any(t[d] < 0 or t[d] % s[d] for d in range(3)):
                        continue
                    o = tuple(t[d] // s[d] for d in range(3))
                    if any(o[d] >= O[d] for d in range(3)) or o in seen:
                        continue
                    seen.add(o)
                    sites.append(o)
        for o in sites:
            nbr.append([first.get(tuple(o[d] * s[d] - p[d] + k[d] for d in range(3)), -1) for k in ks])
        out_coors += sites
        out_offsets.append(len(out_coors))
    return (np.asarray(out_coors, np.int32).reshape(-1, 3), np.asarray(out_offsets, np.int32),
            np.asarray(nbr, np.int32).reshape(-1, len(ks)))


def row_grid(coors, G):
    """Dense lowest-row array of ONE scene's rows (local numbering), INT_MAX where empty."""
    grid = np.full(G, INT_MAX, np.int64)
    c = np.asarray(coors, np.int64).reshape(-1, 3)
    np.minimum.at(grid, (c[:, 0], c[:, 1], c[:, 2]), np.arange(len(c)))
    return grid


def index_vec(coors, offsets, G, K, s=(1, 1, 1), p=(0, 0, 0), subm=False):
    """The same by array arithmetic on a dense row array per scene."""
    G, K, s, p, O = geometry(G, K, s, p, subm)
    ks = offsets_k(K)
    sa, pa, Oa, Ga = (np.asarray(v, np.int64) for v in (s, p, O, G))
    coors = np.asarray(coors, np.int64).reshape(-1, 3)
    offsets = np.asarray(offsets, np.int64)
    oc, oo, nb = [], [0], []
    for b in range(len(offsets) - 1):
        c = coors[offsets[b]:offsets[b + 1]]
        if subm:
            sites = c
        else:
            t = c[:, None, :] + pa - ks[None, :, :]                               # [n,Kvol,3], walked in (row, kk) order
            ok = ((t >= 0) & (t % sa == 0) & (t // sa < Oa)).all(-1).reshape(-1)
            o = (t // sa).reshape(-1, 3)[ok]
            lin = (o[:, 0] * O[1] + o[:, 1]) * O[2] + o[:, 2]
            _, firsts = np.unique(lin, return_index=True)
            sites = o[np.sort(firsts)]
        grid = row_grid(c, G)
        q = sites[:, None, :] * sa - pa + ks[None, :, :]                          # [No,Kvol,3]
        inside = ((q >= 0) & (q < Ga)).all(-1)
        qc = np.clip(q, 0, Ga - 1)
        r = grid[qc[..., 0], qc[..., 1], qc[..., 2]]
        r = np.where(inside & (r != INT_MAX), r + offsets[b], -1)
        oc.append(sites)
        nb.append(r)
        oo.append(oo[-1] + len(sites))
    return (np.concatenate(oc).astype(np.int32).reshape(-1, 3), np.asarray(oo, np.int32),
            np.concatenate(nb).astype(np.int32).reshape(-1, len(ks)))


def active_sites(coors, G, K, s, p):
    """ONE scene: the sorted linear indices of the output sites whose window holds an active input."""
    G, K, s, p, O = geometry(G, K, s, p)
    occ = np.zeros(tuple(g + 2 * q for g, q in zip(G, p)), bool)
    c = np.asarray(coors, np.int64).reshape(-1, 3)
    occ[c[:, 0] + p[0], c[:, 1] + p[1], c[:, 2] + p[2]] = True
    act = np.zeros(O, bool)
    for k in offsets_k(K):
        act |= occ[k[0]:k[0] + s[0] * (O[0] - 1) + 1:s[0], k[1]:k[1] + s[1] * (O[1] - 1) + 1:s[1], k[2]:k[2] + s[2] * (O[2] - 1) + 1:s[2]]
    return np.flatnonzero(act.reshape(-1))


def plain_rows(feat, nbr):
    """[No, Kvol*Cin]: feat[nbr[o,0]] || ... || feat[nbr[o,Kvol-1]], zero rows for -1."""
    feat = np.asarray(feat, F)
    padded = np.concatenate([feat, np.zeros((1, feat.shape[1]), F)])
    return np.ascontiguousarray(padded[np.where(nbr >= 0, nbr, len(feat))].reshape(len(nbr), -1))


def conv(feat, nbr, W, bias=None, residual=None, relu=False):
    """§21.2: W [Kvol,Cout,Cin] -> out [No,Cout] float32."""
    import oracle
    W = np.asarray(W, F)
    Kvol, Cout, Cin = W.shape
    Wp = np.ascontiguousarray(W.transpose(1, 0, 2).reshape(Cout, Kvol * Cin))        # W'[co][kk*Cin + ci]
    b = np.zeros(Cout, F) if bias is None else np.asarray(bias, F)
    if len(nbr) == 0:
        return np.zeros((0, Cout), F)
    out = np.asarray(oracle.mlp_rows(plain_rows(feat, nbr), [(Wp, b)], relu_mask=0), F)
    if residual is not None:
        out = (out + np.asarray(residual, F)).astype(F)
    if relu:
        out = np.where(out > 0, out, F(0)).astype(F)
    return out


def scene_ids(offsets):
    offsets = np.asarray(offsets, np.int64)
    return np.repeat(np.arange(len(offsets) - 1), np.diff(offsets))


def to_dense(feat, coors, offsets, shape):
    """§21.3 -> [B,C,Oz,Oy,Ox]; the lowest row wins a duplicate (rows are written from the last to the first)."""
    feat = np.asarray(feat, F)
    B = len(offsets) - 1
    dense = np.zeros((B, feat.shape[1]) + tuple(shape), F)
    sc = scene_ids(offsets)
    for r in range(len(feat) - 1, -1, -1):
        z, y, x = (int(v) for v in coors[r])
        dense[sc[r], :, z, y, x] = feat[r]
    return dense


def from_voxels(feat, coors, voxel_num):
    """§20.3 outputs feat [B,V,C], coors [B,V,3], voxel_num [B] -> (feat [Nv,C], coors [Nv,3], offsets [B+1])."""
    B = feat.shape[0]
    f = np.concatenate([feat[b, :voxel_num[b]] for b in range(B)]).astype(F)
    c = np.concatenate([coors[b, :voxel_num[b]] for b in range(B)]).astype(np.int32)
    return f, c, np.concatenate([[0], np.cumsum(voxel_num)]).astype(np.int32)


def gamma(n):
    u = 2.0 ** -24
    return n * u / (1.0 - n * u)


def conv3d_check(feat, coors, offsets, G, K, s, p, W, bias, out, out_coors, out_offsets, subm=False):
    """Cross-check of ``out`` against torch.nn.functional.conv3d on the densified input (CPU): active sites within
    2 * gamma_n * sum |w.x| (the two forward error bounds added, n = Kvol*Cin + 2), inactive sites equal to the bias (not in
    the submanifold form, whose inactive sites are by definition sites the dense convolution would fill).
    -> (largest error / bound over the active sites, number of inactive sites checked)."""
    import torch
    G, K, s, p, O = geometry(G, K, s, p)
    W = np.asarray(W, F)
    Kvol, Cout, Cin = W.shape
    w5 = torch.from_numpy(np.ascontiguousarray(W.reshape(K[0], K[1], K[2], Cout, Cin).transpose(3, 4, 0, 1, 2)))
    x = torch.from_numpy(to_dense(feat, coors, offsets, G))
    b = np.zeros(Cout, F) if bias is None else np.asarray(bias, F)
    y = torch.nn.functional.conv3d(x, w5, torch.from_numpy(b), stride=s, padding=p).numpy()
    mag = torch.nn.functional.conv3d(x.abs(), w5.abs(), torch.from_numpy(np.abs(b)), stride=s, padding=p).numpy()
    assert y.shape[2:] == O
    sc = scene_ids(out_offsets)
    z, yy, xx = out_coors[:, 0], out_coors[:, 1], out_coors[:, 2]
    want = y[sc, :, z, yy, xx]
    bound = 2.0 * gamma(Kvol * Cin + 2) * mag[sc, :, z, yy, xx].astype(np.float64)
    err = np.abs(out.astype(np.float64) - want.astype(np.float64))
    assert (err <= bound).all(), f"conv3d cross-check: {int((err > bound).sum())} values outside the bound, worst {float((err / np.maximum(bound, 1e-300)).max()):.3g} x"
    inactive = np.ones(y.shape[:1] + y.shape[2:], bool)
    inactive[sc, z, yy, xx] = False
    yi = y.transpose(0, 2, 3, 4, 1)[inactive]
    assert subm or (yi == b[None, :]).all(), "conv3d cross-check: an inactive site differs from the bias"
    return (float((err / np.maximum(bound, 1e-300)).max()) if err.size else 0.0), int(inactive.sum())
