"""float32 numpy restatement of SPEC.md §24 (voxel feature encoder), the reference of tests/test_vfe_cpu.py and
tests/test_gpu_vfe.py.

Two forms: ``encode_loop`` executes the text voxel by voxel, ``encode`` is vectorised over the rows.  Both stand on
``voxel_ref.member_lists`` for the ordered members, float32 numpy for the decorations and ``oracle.mlp_rows`` for the layer (the
§6 fmaf chain).  ``backward`` is the float64 gradient with the sums of absolute terms the error bounds are stated in."""
import numpy as np

import voxel_ref as vr

F = np.float32


def clean(p2v, V):
    """Numbers outside [0, V) count as -1."""
    p2v = np.asarray(p2v, np.int32)
    return np.where((p2v >= 0) & (p2v < V), p2v, -1).astype(np.int32)


def members(p2v, offsets, V, T=None):
    """-> (rows, s_of, rank, start): list entry k is row rows[k] of voxel s_of[k] at position rank[k]; a member iff rank < T."""
    rows, start = vr.member_lists(clean(p2v, V), offsets, V)
    s_of = np.repeat(np.arange(len(start) - 1), np.diff(start))
    rank = np.arange(len(rows)) - start[s_of]
    return rows, s_of, rank, start


def member_p2v(p2v, offsets, V, T=None):
    """point2voxel with every row that is not a member set to -1."""
    out = clean(p2v, V)
    if T is not None:
        rows, s_of, rank, _ = members(p2v, offsets, V)
        out[rows[rank >= T]] = -1
    return out


def centres(coors, voxel_size, point_range):
    """ctr[B*V,3] (x,y,z) = ((float)g_d * v_d) + ((0.5f * v_d) + lo_d), every operation rounded to binary32."""
    v = np.asarray(voxel_size, F)
    lo = np.asarray(point_range, F)[:3]
    g = np.asarray(coors, np.int32).reshape(-1, 3)[:, ::-1].astype(F)       # (z,y,x) -> (x,y,z)
    ctr = (g * v) + ((F(0.5) * v) + lo)
    assert ctr.dtype == F
    return ctr


def decorate(points, p2v, offsets, V, coors=None, voxel_size=None, point_range=None, cluster_center=True, voxel_center=True,
             vox_feat=None, T=None):
    """-> (rows [total,Cin] f32 (zeros for rows that are not members), mp2v [total] (member_p2v), mean [B*V,3])."""
    points = np.asarray(points, F)
    total, C = points.shape
    mp = member_p2v(p2v, offsets, V, T)
    sid = vr.scene_ids(offsets, total).astype(np.int64)
    s = sid * V + mp
    live = mp >= 0
    B = len(offsets) - 1
    parts = [points]
    mean = np.zeros((B * V, 3), F)
    if cluster_center:
        mean = vr.voxel_reduce(points[:, :3], mp, offsets, V, "mean")[0].reshape(B * V, 3)
        parts.append(points[:, :3] - mean[np.where(live, s, 0)])
    if voxel_center:
        ctr = centres(coors, voxel_size, point_range)
        parts.append(points[:, :3] - ctr[np.where(live, s, 0)])
    if vox_feat is not None:
        vf = np.asarray(vox_feat, F).reshape(B * V, -1)
        parts.append(vf[np.where(live, s, 0)])
    rows = np.concatenate(parts, 1).astype(F)
    rows[~live] = 0
    return np.ascontiguousarray(rows), mp, mean


def encode(orc, points, p2v, offsets, V, W, b, relu=True, **kw):
    """Vectorised form -> (pooled [B,V,Cout], arg [B,V,Cout] int32, pointwise [total,Cout], rows [total,Cin])."""
    rows, mp, _ = decorate(points, p2v, offsets, V, **kw)
    W, b = np.asarray(W, F), np.asarray(b, F)
    live = np.flatnonzero(mp >= 0)
    y = np.zeros((rows.shape[0], W.shape[0]), F)
    if len(live):
        y[live] = orc.mlp_rows(np.ascontiguousarray(rows[live]), [(W, b)], 1 if relu else 0)
    pooled, arg, _ = vr.voxel_reduce(y, mp, offsets, V, "max")       # strict >: a tie stays with the lowest row, -0 == +0
    return pooled, arg, y, rows


def encode_loop(orc, points, p2v, offsets, V, W, b, relu=True, coors=None, voxel_size=None, point_range=None,
                cluster_center=True, voxel_center=True, vox_feat=None, T=None):
    """§24 executed voxel by voxel -> (pooled, arg, pointwise, rows, mean [B*V,3])."""
    points, W, b = np.asarray(points, F), np.asarray(W, F), np.asarray(b, F)
    total, C = points.shape
    B, Cout = len(offsets) - 1, W.shape[0]
    rows_l, s_of, rank, start = members(p2v, offsets, V)
    Cin = W.shape[1]
    pooled = np.zeros((B * V, Cout), F)
    arg = np.full((B * V, Cout), -1, np.int32)
    pw = np.zeros((total, Cout), F)
    rows = np.zeros((total, Cin), F)
    mean = np.zeros((B * V, 3), F)
    ctr = centres(coors, voxel_size, point_range) if voxel_center else None
    vf = None if vox_feat is None else np.asarray(vox_feat, F).reshape(B * V, -1)
    for s in range(B * V):
        m = rows_l[start[s]:start[s + 1]]
        if T is not None:
            m = m[:T]
        if len(m) == 0:
            continue
        if cluster_center:
            acc = points[m[0], :3].copy()
            for i in m[1:]:
                acc = acc + points[i, :3]
            mean[s] = acc / F(len(m))
        for i in m:
            parts = [points[i]]
            if cluster_center:
                parts.append(points[i, :3] - mean[s])
            if voxel_center:
                parts.append(points[i, :3] - ctr[s])
            if vf is not None:
                parts.append(vf[s])
            rows[i] = np.concatenate(parts)
        y = orc.mlp_rows(np.ascontiguousarray(rows[m]), [(W, b)], 1 if relu else 0)
        pw[m] = y
        mx = y.max(0)
        pooled[s] = mx
        arg[s] = m[(y == mx[None, :]).argmax(0)]                  # the lowest row with y == max
    return pooled.reshape(B, V, Cout), arg.reshape(B, V, Cout), pw, rows, mean


def pz(a):
    """+0.0 normalisation: -0.0 -> +0.0, everything else unchanged."""
    return np.asarray(a) + F(0)


def backward(rows, mp, offsets, V, W, y, arg, grad_pooled, grad_pointwise=None, relu=True, C=None, n_dec=0, Cv=0):
    """float64 gradients of §24 -> dict(grad_W, grad_bias, grad_points, grad_vox_feat) and, under the same keys + "_abs", the sums
    of the absolute values of the terms each entry adds up.  ``n_dec`` = number of decorations in the row, ``C`` = point columns."""
    total, Cin = rows.shape
    B = len(offsets) - 1
    Cout = W.shape[0]
    D = np.float64
    sid = vr.scene_ids(offsets, total).astype(np.int64)
    live = mp >= 0
    s = np.where(live, sid * V + mp, 0)
    gp = np.asarray(grad_pooled, D).reshape(B * V, Cout)
    a = np.asarray(arg).reshape(B * V, Cout)
    g = np.where(live[:, None] & (a[s] == np.arange(total)[:, None]), gp[s], 0.0)
    if grad_pointwise is not None:
        g = g + np.where(live[:, None], np.asarray(grad_pointwise, D), 0.0)
    if relu:
        g = np.where(y > 0, g, 0.0)
    r64, W64 = rows.astype(D), np.asarray(W, D)
    out = dict(g=g, grad_W=g.T @ r64, grad_W_abs=np.abs(g).T @ np.abs(r64), grad_bias=g.sum(0), grad_bias_abs=np.abs(g).sum(0))
    gr, gra = g @ W64, np.abs(g) @ np.abs(W64)
    gpts, gpts_a = gr[:, :C].copy(), gra[:, :C].copy()
    for k in range(n_dec):
        gpts[:, :3] += gr[:, C + 3 * k:C + 3 * k + 3]
        gpts_a[:, :3] += gra[:, C + 3 * k:C + 3 * k + 3]
    out.update(grad_points=gpts, grad_points_abs=gpts_a)
    if Cv:
        gv, gva = np.zeros((B * V, Cv)), np.zeros((B * V, Cv))
        np.add.at(gv, s[live], gr[live][:, Cin - Cv:])
        np.add.at(gva, s[live], gra[live][:, Cin - Cv:])
        out.update(grad_vox_feat=gv.reshape(B, V, Cv), grad_vox_feat_abs=gva.reshape(B, V, Cv))
    return out


def tiles_case(seed=0):
    """The hand-built family: two scenes on a 1-D row of voxels whose member counts are, in voxel order, the list below (voxel
    k of a scene is cell x = k), rows shuffled inside a scene so that list order and row order differ.  -> (points [total,4],
    offsets, params, counts per scene)."""
    rng = np.random.default_rng(100 + seed)
    counts = [[1, 31, 2, 32, 0, 33, 63, 200, 64, 65, 1, 0, 2], [65, 0, 31, 33, 1, 64, 200, 32, 63, 2, 0, 1]]
    pts, off = [], [0]
    for cs in counts:
        cell = np.repeat(np.arange(len(cs)), cs)
        n = len(cell)
        p = np.empty((n + 9, 4), F)
        p[:n, 0] = cell + rng.random(n).astype(F) * F(0.9) + F(0.05)
        p[:n, 1:3] = rng.random((n, 2)).astype(F) * F(0.9) + F(0.05)
        p[n:, :3] = F(-5)                                           # out of range
        p[:, 3] = rng.standard_normal(n + 9).astype(F)
        # the voxel NUMBER is the order of first appearance: keep the first point of every cell in cell order, shuffle the rest
        first = np.concatenate([[0], np.cumsum(cs)[:-1]])[np.asarray(cs) > 0]
        rest = np.setdiff1d(np.arange(n + 9), first)
        rng.shuffle(rest)
        order = np.concatenate([first, rest])
        pts.append(p[order])
        off.append(off[-1] + n + 9)
    V = 16
    par = dict(v=(1.0, 1.0, 1.0), r=(0, 0, 0, 14, 1, 1), T=8, V=V)
    return np.concatenate(pts), np.asarray(off, np.int32), par, counts


def signed_zero_case():
    """One scene, C = 1, no decorations, W = [[1],[-1]], bias -0.0: y = (x, -x) with the sign of a zero kept.  Voxel 0 holds
    x = -0.0 (row 0), +0.0, -1; voxel 1 holds only negative x (channel 0 has a negative maximum); voxel 2 holds +0.0 then -0.0
    and -2."""
    x = np.array([-0.0, 0.0, -1.0, -3.0, -0.5, -7.0, 0.0, -0.0, -2.0], F)
    pts = x.reshape(9, 1).copy()
    p2v = np.array([0, 0, 0, 1, 1, 1, 2, 2, 2], np.int32)
    off = np.array([0, 9], np.int32)
    W = np.array([[1], [-1]], F)
    return pts, off, dict(V=4), p2v, W, np.array([-0.0, -0.0], F)
