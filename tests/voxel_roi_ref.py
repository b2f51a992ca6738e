"""float32 numpy restatement of SPEC.md §30 (voxel RoI pooling, the index side), the reference of tests/test_voxel_roi_cpu.py and
tests/test_gpu_voxel_roi.py, with the cases both run.

Two independent forms of ``voxel_query``: ``query_walk`` executes the text literally (a dict of coordinates, the candidate cells
walked dz slowest and dx fastest), ``query_brute`` tests every voxel of the scene against the query and sorts the accepted ones by
their rank in the walk.  ``FORMS`` names both.  ``roi_grid_points`` likewise (a scalar loop and whole arrays); sin / cos come from
the oracle's §13 routine (``oracle.sincos_r``), as in tests/box_ref.py.  ``pool_rows`` is §6 on the rows the module builds (the
oracle's fused group -> MLP -> max), zero where a group is empty."""
import functools

import numpy as np

import oracle

F = np.float32
NAN_BITS = 0x7FC00000                                    # the quiet NaN of an unread RoI's points
LIMIT = F(2.0 ** 30)


# ---- roi_grid_points ---------------------------------------------------------------------------------------------------------
def _sincos(yaw):
    s, c = oracle.sincos_r(np.ascontiguousarray(np.asarray(yaw, F).reshape(-1)))
    return np.asarray(s, F), np.asarray(c, F)


def _counts(rois, roi_count):
    B, R = rois.shape[:2]
    return np.full(B, R) if roi_count is None else np.clip(np.asarray(roi_count, np.int64), 0, R)


def grid_points_loop(rois, roi_count, G):
    B, R, _ = rois.shape
    n = _counts(rois, roi_count)
    out = np.full((B, R, G ** 3, 3), np.frombuffer(np.uint32(NAN_BITS).tobytes(), F)[0], F)
    for b in range(B):
        for r in range(int(n[b])):
            cx, cy, cz, l, w, h, yaw = (F(v) for v in rois[b, r, :7])
            s, c = (v[0] for v in _sincos([yaw]))
            for g in range(G ** 3):
                ix, iy, iz = g // (G * G), (g // G) % G, g % G
                lx = F(F(F(F(ix) + F(0.5)) / F(G)) * l) - F(F(0.5) * l)
                ly = F(F(F(F(iy) + F(0.5)) / F(G)) * w) - F(F(0.5) * w)
                lz = F(F(F(F(iz) + F(0.5)) / F(G)) * h) - F(F(0.5) * h)
                out[b, r, g, 0] = F(F(lx * c) - F(ly * s)) + cx
                out[b, r, g, 1] = F(F(lx * s) + F(ly * c)) + cy
                out[b, r, g, 2] = lz + cz
    return out


def grid_points_vec(rois, roi_count, G):
    B, R, _ = rois.shape
    n = _counts(rois, roi_count)
    r = np.asarray(rois, F)
    s, c = (v.reshape(B, R, 1) for v in _sincos(r[..., 6]))
    i = np.arange(G, dtype=F)
    frac = (i + F(0.5)) / F(G)
    ix, iy, iz = (v.reshape(1, 1, -1) for v in np.meshgrid(frac, frac, frac, indexing="ij"))
    with np.errstate(all="ignore"):
        lx = ix * r[..., 3:4] - F(0.5) * r[..., 3:4]
        ly = iy * r[..., 4:5] - F(0.5) * r[..., 4:5]
        lz = iz * r[..., 5:6] - F(0.5) * r[..., 5:6]
        out = np.stack([(lx * c - ly * s) + r[..., 0:1], (lx * s + ly * c) + r[..., 1:2], lz + r[..., 2:3]], -1).astype(F)
    out[np.arange(R)[None, :] >= n[:, None]] = np.frombuffer(np.uint32(NAN_BITS).tobytes(), F)[0]
    return out


# ---- voxel_query -------------------------------------------------------------------------------------------------------------
def query_cell(p, voxel_size, lo):
    """§20.1's cell of a query (x,y,z), or None for an empty query (NaN, Inf, beyond 2^30)."""
    with np.errstate(all="ignore"):
        f = np.floor((np.asarray(p, F) - np.asarray(lo, F)) / np.asarray(voxel_size, F))
    assert f.dtype == F
    if not (np.abs(f) < LIMIT).all():
        return None
    return tuple(int(v) for v in f)


def centres(cells_xyz, voxel_size, lo):
    """§24: ((float)g * v) + ((0.5 * v) + lo), cells (x,y,z) -> centres (x,y,z)."""
    v, lo = np.asarray(voxel_size, F), np.asarray(lo, F)
    return np.asarray(cells_xyz, F) * v + (F(0.5) * v + lo)


def d2(ctr, p):
    """§1 with point = voxel centre, centre = query."""
    d = np.asarray(ctr, F) - np.asarray(p, F)
    t = d * d
    return (t[..., 0] + t[..., 1]) + t[..., 2]


def _fill(rows, S):
    n = min(len(rows), S)
    out = np.zeros(S, np.int32)
    if n:
        out[:n] = rows[:n]
        out[n:] = rows[0]
    return out, n


def query_walk(coors, offsets, spatial_shape, voxel_size, lo, new_xyz, max_range, radius, S):
    B, M, _ = new_xyz.shape
    Gz, Gy, Gx = spatial_shape
    rz, ry, rx = max_range
    r2 = F(radius) * F(radius)
    idx, cnt = np.zeros((B, M, S), np.int32), np.zeros((B, M), np.int32)
    for b in range(B):
        table = {}
        for i in range(int(offsets[b]), int(offsets[b + 1])):
            table.setdefault(tuple(int(v) for v in coors[i]), i)
        for m in range(M):
            q = query_cell(new_xyz[b, m], voxel_size, lo)
            rows = []
            if q is not None:
                for dz in range(-rz, rz + 1):
                    for dy in range(-ry, ry + 1):
                        for dx in range(-rx, rx + 1):
                            x, y, z = q[0] + dx, q[1] + dy, q[2] + dz
                            if not (0 <= z < Gz and 0 <= y < Gy and 0 <= x < Gx) or (z, y, x) not in table:
                                continue
                            if d2(centres((x, y, z), voxel_size, lo), new_xyz[b, m]) < r2:
                                rows.append(table[(z, y, x)])
            idx[b, m], cnt[b, m] = _fill(rows, S)
    return idx, cnt


def query_brute(coors, offsets, spatial_shape, voxel_size, lo, new_xyz, max_range, radius, S):
    B, M, _ = new_xyz.shape
    rng = np.asarray(max_range, np.int64)                  # (z,y,x)
    r2 = F(radius) * F(radius)
    idx, cnt = np.zeros((B, M, S), np.int32), np.zeros((B, M), np.int32)
    shape = np.asarray(spatial_shape, np.int64)
    for b in range(B):
        o0, o1 = int(offsets[b]), int(offsets[b + 1])
        c = np.asarray(coors[o0:o1], np.int64)
        inside = ((c >= 0) & (c < shape)).all(1)
        key = (c[:, 0] * shape[1] + c[:, 1]) * shape[2] + c[:, 2]
        _, first = np.unique(key, return_index=True)       # the lowest row owns a duplicated coordinate
        owner = np.zeros(len(c), bool)
        owner[first] = True
        ctr = centres(c[:, ::-1], voxel_size, lo)
        for m in range(M):
            q = query_cell(new_xyz[b, m], voxel_size, lo)
            if q is None or not len(c):
                continue
            d = c - np.asarray(q[::-1], np.int64)
            ok = owner & inside & (np.abs(d) <= rng).all(1) & (d2(ctr, new_xyz[b, m]) < r2)
            rank = ((d[:, 0] + rng[0]) * (2 * rng[1] + 1) + (d[:, 1] + rng[1])) * (2 * rng[2] + 1) + (d[:, 2] + rng[2])
            rows = np.nonzero(ok)[0]
            rows = rows[np.argsort(rank[rows], kind="stable")] + o0
            idx[b, m], cnt[b, m] = _fill(list(rows), S)
    return idx, cnt


FORMS = {"walk": query_walk, "brute": query_brute}


def accepted_total(coors, offsets, spatial_shape, voxel_size, lo, new_xyz, max_range, radius):
    """[B,M]: the accepted candidates of every query without a cap (what S must exceed to be 'never filled')."""
    return query_brute(coors, offsets, spatial_shape, voxel_size, lo, new_xyz, max_range, radius, 1024)[1]


# ---- §6 on the module's rows -------------------------------------------------------------------------------------------------
def pool_rows(coors, feat, voxel_size, lo, pts, idx, cnt, layers):
    """coors [Nv,3], feat [Nv,C], pts [Q,3], idx [Q,S], cnt [Q] -> [Q,C_out]: §6 with the voxels as one scene, zero where cnt == 0."""
    xyz = centres(np.asarray(coors)[:, ::-1], voxel_size, lo)[None]
    with np.errstate(all="ignore"):
        out = oracle.sa_group_mlp_max(np.ascontiguousarray(xyz, F), np.ascontiguousarray(feat[None], F),
                                      np.ascontiguousarray(np.nan_to_num(pts, nan=0.0, posinf=0.0, neginf=0.0)[None], F),
                                      np.ascontiguousarray(idx[None], np.int32), layers)[0]
    out = np.array(out, F)
    out[np.asarray(cnt).reshape(-1) == 0] = 0
    return out


# ---- the cases ---------------------------------------------------------------------------------------------------------------
SHAPE = (5, 12, 12)                                      # (Gz,Gy,Gx)
RANGES = ((1, 2, 3), (0, 0, 0), (4, 4, 4))               # (rz,ry,rx); (1,2,3): 105 candidates, more than one 64-lane step
SIZES = (1, 4, 16, 128)                                  # 128: more than any ball of the cases holds
FAMILIES = {
    # name: (voxel_size (vx,vy,vz), point_range, radius)
    "exact": ((0.5, 0.5, 0.25), (-3.0, -3.0, -0.5, 3.0, 3.0, 0.75), 1.5),
    "general": ((0.05, 0.05, 0.1), (0.0, -40.0, -3.0, 0.6, -39.4, -2.5), 0.17),
}


@functools.lru_cache(maxsize=None)
def grid():
    """-> (coors [Nv,3] int32 (z,y,x), offsets [4] int32): B = 3, the middle scene empty, ~150 voxels in each of the others, every
    face of the grid touched, and scene 2 holding one coordinate twice (the copy is its LAST row: the lowest row owns the cell)."""
    rng = np.random.default_rng(30)
    scenes = []
    for _ in range(2):
        cells = rng.permutation(SHAPE[0] * SHAPE[1] * SHAPE[2])[:144]
        c = np.stack([cells // (SHAPE[1] * SHAPE[2]), (cells // SHAPE[2]) % SHAPE[1], cells % SHAPE[2]], 1)
        faces = np.array([[0, 5, 5], [4, 6, 6], [2, 0, 4], [2, 11, 7], [1, 3, 0], [3, 8, 11]])
        c = np.concatenate([c, faces])
        _, first = np.unique((c[:, 0] * SHAPE[1] + c[:, 1]) * SHAPE[2] + c[:, 2], return_index=True)
        scenes.append(c[np.sort(first)])
    scenes[1] = np.concatenate([scenes[1], scenes[1][7:8]])
    coors = np.concatenate(scenes).astype(np.int32)
    n0, n2 = len(scenes[0]), len(scenes[1])
    return coors, np.array([0, n0, n0, n0 + n2], np.int32)


@functools.lru_cache(maxsize=None)
def queries(family):
    """new_xyz [3,M,3] of a family (the same points asked of every scene; M = 67: the last workgroup is not full)."""
    vs, pr, radius = FAMILIES[family]
    v, lo, hi = np.asarray(vs, F), np.asarray(pr[:3], F), np.asarray(pr[3:], F)
    coors, offsets = grid()
    rng = np.random.default_rng(len(family))
    pts = []
    if family == "exact":
        r = F(radius)
        for i in (0, 3, 11, int(offsets[2]) + 2, int(offsets[2]) + 9):
            ctr = centres(coors[i, ::-1], vs, lo)
            for axis in range(3):
                on = ctr.copy()
                on[axis] = ctr[axis] + r                     # d2 == r2 exactly: rejected
                inside = on.copy()
                # one ulp inside: the first float below `on` whose difference from the centre is below r (where `on` is
                # smaller than r its own ulp is finer than the difference's, and the nearest floats still round onto r)
                while d2(ctr, inside) == r * r:
                    inside[axis] = np.nextafter(inside[axis], F(-np.inf))
                pts += [on, inside]
                assert d2(ctr, on) == r * r and d2(ctr, inside) < r * r
        pts += [lo + v * F(k) for k in (1, 2, 4)]            # on a cell face of all three axes
        pts += [np.array([-1.0, 0.5, 0.0], F), np.array([0.25, -1.5, 0.125], F)]     # on one face
    else:
        pts += [lo + v * F(k) for k in (1, 2, 4)]
    mid = (lo + hi) * F(0.5)
    for axis in range(3):                                    # outside the grid on each of the six sides, neighbours in range
        for side, edge in ((-1, lo), (1, hi)):
            p = mid.copy()
            p[axis] = edge[axis] + F(side) * F(0.6) * v[axis]
            pts.append(p)
            q = (lo + (hi - lo) * rng.uniform(0.2, 0.8, 3).astype(F)).astype(F)
            q[axis] = edge[axis] + F(side) * F(1.3) * v[axis]
            pts.append(q)
    pts += [np.array([np.nan, 0, 0], F), np.array([0, np.inf, 0], F), np.array([0, 0, -np.inf], F), np.array([1e30, 0, 0], F),
            np.array([0, -3e9, 0], F), mid + np.array([1e4, 0, 0], F)]
    n = 67 - len(pts)
    assert n > 10
    pts += list((lo - v + (hi - lo + F(2) * v) * rng.uniform(0, 1, (n, 3)).astype(F)).astype(F))
    one = np.stack(pts).astype(F)
    return np.ascontiguousarray(np.broadcast_to(one, (3,) + one.shape))


def query_args(family):
    """What both forms and the operator take: (coors, offsets, SHAPE, voxel_size, point_range, new_xyz, radius)."""
    vs, pr, radius = FAMILIES[family]
    coors, offsets = grid()
    return coors, offsets, SHAPE, vs, pr, queries(family), radius


@functools.lru_cache(maxsize=None)
def expected(family, max_range, S):
    """(idx, cnt) of a case: computed once, shared by the tests, never written to."""
    coors, offsets, shape, vs, pr, new_xyz, radius = query_args(family)
    idx, cnt = query_walk(coors, offsets, shape, vs, pr[:3], new_xyz, max_range, radius, S)
    idx.setflags(write=False)
    cnt.setflags(write=False)
    return idx, cnt


@functools.lru_cache(maxsize=None)
def extra_cases():
    """{name: (coors, offsets, shape, voxel_size, point_range, new_xyz, max_range, radius, S)}: what the families do not reach.
    widest      max_range (8,8,8): 4 913 candidates, 77 steps, on the exact family's grid and queries
    cell limit  a grid of 1290^3 = 2 146 689 000 cells (2^31 - 1 is the bound): voxels and queries at the far corner, where the
                cell number needs all 31 bits, and at the origin; one query in the empty middle"""
    coors, offsets, shape, vs, pr, new_xyz, _ = query_args("exact")
    cases = {"widest": (coors, offsets, shape, vs, pr, new_xyz, (8, 8, 8), 2.5, 16)}
    rng = np.random.default_rng(31)
    G = 1290
    far = G - 1 - rng.integers(0, 4, (40, 3))
    near = rng.integers(0, 4, (24, 3))
    c = np.unique(np.concatenate([far, near]), axis=0)
    c = c[rng.permutation(len(c))]
    half = len(c) // 2
    big = np.concatenate([c[:half], c[half:], c[:3]]).astype(np.int32)        # scene 1 ends with three cells scene 0 holds too
    off = np.array([0, half, len(c) + 3], np.int32)
    v = (0.5, 0.25, 0.125)
    hi = tuple(G * x for x in v)
    q = np.concatenate([(G - rng.uniform(0, 5, (10, 3))) * np.asarray(v), rng.uniform(-1, 4, (6, 3)) * np.asarray(v),
                        [[hi[0] + 0.2, hi[1] - 0.1, hi[2] - 0.1], [0.5 * hi[0], 0.5 * hi[1], 0.5 * hi[2]]]]).astype(F)
    cases["cell limit"] = (big, off, (G, G, G), v, (0.0, 0.0, 0.0) + hi, np.ascontiguousarray(np.broadcast_to(q, (2,) + q.shape)), (2, 2, 2), 0.9, 8)
    return cases


def rois_case(D, seed=0):
    """rois [2,9,D]: yaw across (-pi, pi] (both ends, 0, the quadrant boundaries), extents from 0.3 to 5, columns beyond 6 noise."""
    rng = np.random.default_rng(seed + D)
    rois = rng.uniform(-3, 3, (2, 9, D)).astype(F)
    rois[..., 3:6] = rng.uniform(0.3, 5.0, (2, 9, 3)).astype(F)
    yaw = np.array([np.pi, np.nextafter(F(-np.pi), F(0)), 0.0, np.pi / 2, -np.pi / 2, 0.3, -2.9, 1.9, 3.0], F)
    rois[0, :, 6] = yaw
    rois[1, :, 6] = rng.uniform(-np.pi, np.pi, 9).astype(F)
    return rois
