"""float32 numpy restatement of SPEC.md §20 (voxelization), the reference of tests/test_voxel_cpu.py and tests/test_gpu_voxel.py.

Two independent forms of the numbering of §20.2: ``number_loop`` executes the text literally (a per-point loop with a dict),
``number_vec`` uses ``np.unique(..., return_index=True)`` ordered by first index.  Everything else (coordinates, hard
voxelization, reductions, the backward gathers) is built on either; ``FORMS`` names both so a test can run one against the other.
Ragged input everywhere: ``points[total, C]`` + ``offsets[B+1]``; ``ragged(points[B,N,C])`` makes the pair for a batch."""
import numpy as np

F = np.float32
INT_MAX = 2 ** 31 - 1


def ragged(points):
    """points [B,N,C] -> (points [B*N,C], offsets [B+1] int32) with offsets[b] = b*N."""
    B, N, C = points.shape
    return np.ascontiguousarray(points.reshape(B * N, C)), (np.arange(B + 1, dtype=np.int64) * N).astype(np.int32)


def grid_size(voxel_size, point_range):
    """§20.1: G_d = (int)rintf((hi_d - lo_d) / v_d) in binary32 (np.rint rounds half to even, as rintf does)."""
    v = np.asarray(voxel_size, F)
    r = np.asarray(point_range, F)
    g = np.rint((r[3:] - r[:3]) / v)
    assert g.dtype == F
    return tuple(int(x) for x in g)


def check_grid(voxel_size, point_range):
    G = grid_size(voxel_size, point_range)
    if min(G) < 1:
        raise ValueError(f"grid dimension below 1: {G}")
    if G[0] * G[1] * G[2] > INT_MAX:
        raise ValueError(f"grid {G} exceeds 2^31 - 1 cells")
    return G


def point_cells(points, voxel_size, point_range):
    """-> (g [total,3] int64 (gx,gy,gz), valid [total] bool): one subtraction, one division, one floor, all binary32."""
    G = check_grid(voxel_size, point_range)
    v = np.asarray(voxel_size, F)
    lo = np.asarray(point_range, F)[:3]
    p = np.asarray(points, F)[:, :3]
    d = p - lo
    q = d / v
    f = np.floor(q)
    assert f.dtype == F
    Gf = np.asarray(G, F)                                  # compared as floats, before the conversion
    valid = ((f >= F(0)) & (f < Gf)).all(1)
    g = np.where(valid[:, None], f, F(-1)).astype(np.int64)
    return g, valid


def keys_of(points, voxel_size, point_range):
    """-> (key [total] int64, -1 for an invalid point; G)."""
    G = check_grid(voxel_size, point_range)
    g, valid = point_cells(points, voxel_size, point_range)
    key = (g[:, 2] * G[1] + g[:, 1]) * G[0] + g[:, 0]
    return np.where(valid, key, -1), G


def scene_ids(offsets, total):
    offsets = np.asarray(offsets, np.int64)
    return np.repeat(np.arange(len(offsets) - 1), np.diff(offsets)).astype(np.int32)[:total]


def voxel_coords(points, offsets, voxel_size, point_range):
    g, valid = point_cells(points, voxel_size, point_range)
    out = np.empty((points.shape[0], 4), np.int32)
    out[:, 0] = scene_ids(offsets, points.shape[0])
    out[:, 1], out[:, 2], out[:, 3] = g[:, 2], g[:, 1], g[:, 0]
    return out


def number_loop(key, V):
    """§20.2 executed literally for ONE scene: key [n] (-1 invalid) -> (p2v [n], first_rows of the voxels in number order)."""
    seen = {}
    p2v = np.full(len(key), -1, np.int32)
    firsts = []
    voxel_num = 0
    for i, k in enumerate(key.tolist()):
        if k < 0:
            continue
        if k not in seen:
            if voxel_num < V:
                seen[k] = voxel_num
                firsts.append(i)
                voxel_num += 1
            else:
                seen[k] = -1                                # dropped, and so is every later point of this key
        p2v[i] = seen[k]
    return p2v, np.asarray(firsts, np.int64)


def number_vec(key, V):
    """The same by np.unique: distinct keys ordered by the row of their first appearance; numbers >= V are dropped."""
    p2v = np.full(len(key), -1, np.int32)
    rows = np.flatnonzero(key >= 0)
    if len(rows) == 0:
        return p2v, np.zeros(0, np.int64)
    _, first, inv = np.unique(key[rows], return_index=True, return_inverse=True)
    order = np.argsort(first, kind="stable")               # unique keys by first appearance
    number = np.empty(len(order), np.int64)
    number[order] = np.arange(len(order))
    n = number[inv.reshape(-1)]
    p2v[rows] = np.where(n < V, n, -1)
    return p2v, rows[first[order][:V]]


FORMS = {"loop": number_loop, "vec": number_vec}


def voxel_index(points, offsets, voxel_size, point_range, V, form="vec"):
    """§20.3 -> (point2voxel [total] int32, coors [B,V,3] int32 (z,y,x), count [B,V] int32, voxel_num [B] int32)."""
    key, G = keys_of(points, voxel_size, point_range)
    offsets = np.asarray(offsets, np.int64)
    B = len(offsets) - 1
    p2v = np.full(points.shape[0], -1, np.int32)
    coors = np.full((B, V, 3), -1, np.int32)
    count = np.zeros((B, V), np.int32)
    voxel_num = np.zeros(B, np.int32)
    for b in range(B):
        o0, o1 = offsets[b], offsets[b + 1]
        pv, firsts = FORMS[form](key[o0:o1], V)
        p2v[o0:o1] = pv
        nv = len(firsts)
        voxel_num[b] = nv
        k = key[o0:o1][firsts]
        coors[b, :nv, 2] = k % G[0]
        coors[b, :nv, 1] = (k // G[0]) % G[1]
        coors[b, :nv, 0] = k // (G[0] * G[1])
        count[b] = np.bincount(pv[pv >= 0], minlength=V)[:V]
    return p2v, coors, count, voxel_num


def member_lists(p2v, offsets, V):
    """-> (rows sorted by (scene, voxel, row) for the taken points, start [B*V+1]): the members of voxel s = b*V+v in ascending
    row order are rows[start[s]:start[s+1]] (a stable argsort keeps the row order inside a voxel)."""
    offsets = np.asarray(offsets, np.int64)
    B = len(offsets) - 1
    sid = scene_ids(offsets, len(p2v)).astype(np.int64)
    rows = np.flatnonzero(p2v >= 0)
    s = sid[rows] * V + p2v[rows]
    order = np.argsort(s, kind="stable")
    start = np.zeros(B * V + 1, np.int64)
    np.cumsum(np.bincount(s, minlength=B * V), out=start[1:])
    return rows[order], start


def voxelize(points, offsets, voxel_size, point_range, T, V, form="vec"):
    """§20.4 -> (voxels [B,V,T,C] f32, coors [B,V,3], num_points [B,V], voxel_num [B])."""
    points = np.asarray(points, F)
    p2v, coors, count, voxel_num = voxel_index(points, offsets, voxel_size, point_range, V, form)
    B, C = len(offsets) - 1, points.shape[1]
    voxels = np.zeros((B * V, T, C), F)
    rows, start = member_lists(p2v, offsets, V)
    s_of = np.repeat(np.arange(B * V), np.diff(start))
    t_of = np.arange(len(rows)) - start[s_of]
    keep = t_of < T
    voxels[s_of[keep], t_of[keep]] = points[rows[keep]]
    return voxels.reshape(B, V, T, C), coors, np.minimum(count, T).astype(np.int32), voxel_num


def voxelize_loop(points, offsets, voxel_size, point_range, T, V):
    """§20.2 - §20.4 executed literally, point by point: -> (voxels, coors, num_points, voxel_num, point2voxel, count)."""
    points = np.asarray(points, F)
    key, G = keys_of(points, voxel_size, point_range)
    offsets = np.asarray(offsets, np.int64)
    B, C = len(offsets) - 1, points.shape[1]
    voxels = np.zeros((B, V, T, C), F)
    coors = np.full((B, V, 3), -1, np.int32)
    count = np.zeros((B, V), np.int32)
    voxel_num = np.zeros(B, np.int32)
    p2v = np.full(points.shape[0], -1, np.int32)
    for b in range(B):
        seen = {}
        for i in range(int(offsets[b]), int(offsets[b + 1])):
            k = int(key[i])
            if k < 0:
                continue
            v = seen.get(k)
            if v is None:
                if voxel_num[b] < V:
                    v = int(voxel_num[b])
                    voxel_num[b] += 1
                    coors[b, v] = (k // (G[0] * G[1]), (k // G[0]) % G[1], k % G[0])
                else:
                    v = -1
                seen[k] = v
            if v < 0:
                continue
            p2v[i] = v
            if count[b, v] < T:
                voxels[b, v, count[b, v]] = points[i]
            count[b, v] += 1
    return voxels, coors, np.minimum(count, T).astype(np.int32), voxel_num, p2v, count


def voxel_reduce_loop(feat, p2v, offsets, V, mode):
    """§20.5 executed literally (a Python loop over the points in row order)."""
    feat = np.asarray(feat, F)
    offsets = np.asarray(offsets, np.int64)
    B, Cf = len(offsets) - 1, feat.shape[1]
    out = np.zeros((B, V, Cf), F)
    arg = np.full((B, V, Cf), -1, np.int32)
    n = np.zeros((B, V), np.int32)
    for b in range(B):
        for i in range(int(offsets[b]), int(offsets[b + 1])):
            v = int(p2v[i])
            if v < 0:
                continue
            if n[b, v] == 0:
                out[b, v] = feat[i]
                arg[b, v] = i
            elif mode == "max":
                better = feat[i] > out[b, v]
                out[b, v][better] = feat[i][better]
                arg[b, v][better] = i
            else:
                out[b, v] = out[b, v] + feat[i]
            n[b, v] += 1
    if mode == "mean":
        nz = n > 0
        out[nz] = out[nz] / n[nz].astype(F)[:, None]
    return out, arg if mode == "max" else None, n


def voxel_reduce(feat, p2v, offsets, V, mode):
    """§20.5 -> (out [B,V,Cf] f32, arg [B,V,Cf] int32 or None, count [B,V] int32).  The sum adds the members one by one in
    ascending row order in float32 (step k adds the k-th member of every voxel that has one: one rounding per addition)."""
    feat = np.asarray(feat, F)
    B, Cf = len(offsets) - 1, feat.shape[1]
    rows, start = member_lists(p2v, offsets, V)
    n = np.diff(start)
    out = np.zeros((B * V, Cf), F)
    arg = np.full((B * V, Cf), -1, np.int32) if mode == "max" else None
    k = 0
    live = np.flatnonzero(n > 0)
    while len(live):
        r = rows[start[live] + k]
        x = feat[r]
        if k == 0:
            out[live] = x
            if arg is not None:
                arg[live] = r[:, None]
        elif mode == "max":
            better = x > out[live]                          # strict: ties stay with the lowest row
            out[live] = np.where(better, x, out[live])
            arg[live] = np.where(better, r[:, None], arg[live])
        else:
            out[live] = out[live] + x
        k += 1
        live = live[n[live] > k]
    assert out.dtype == F
    if mode == "mean":
        nz = n > 0
        out[nz] = out[nz] / n[nz].astype(F)[:, None]
    return out.reshape(B, V, Cf), None if arg is None else arg.reshape(B, V, Cf), n.astype(np.int32).reshape(B, V)


def voxel_reduce_grad(grad_out, p2v, offsets, aux, mode):
    """Backward of §20.5, a gather: grad_out [B,V,Cf] -> grad_feat [total,Cf].  aux = count [B,V] (mean) / arg [B,V,Cf] (max)."""
    grad_out = np.asarray(grad_out, F)
    B, V, Cf = grad_out.shape
    total = len(p2v)
    sid = scene_ids(offsets, total).astype(np.int64)
    g = np.zeros((total, Cf), F)
    rows = np.flatnonzero(p2v >= 0)
    b, v = sid[rows], p2v[rows]
    go = grad_out[b, v]
    if mode == "sum":
        g[rows] = go
    elif mode == "mean":
        g[rows] = go / aux[b, v].astype(F)[:, None]
    else:
        g[rows] = np.where(aux[b, v] == rows[:, None], go, F(0))
    return g
