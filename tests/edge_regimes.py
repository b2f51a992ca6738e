"""Edge-regime scenes for the index kernels (fps, ball_query, knn_query, three_nn, ffps) and a float32 numpy model of the
ball-query grid.  Test helper: numpy only, no kernel code.

The index kernels must return the oracle's indices bit for bit (SPEC.md §1-§4, §15, §18), and two of them prune: the grid
ball query reads only the cells ix-1 .. ix+1 around a centroid, the bucketed FPS kernels keep cached keys of boxes.  Friendly
coordinates (U[0,1), lidar-shaped scenes, small lattices) never put those arguments under strain.  Every builder below makes
one regime where they get thin, deterministically, and every case carries statistics (`stats`) that tests/test_edge_regimes.py
asserts, so a case cannot quietly stop reaching its regime.

The grid model (`cell_coord`, `grid_geometry`, `reach`) restates csrc/ball_query_grid.hip's header comment and DESIGN.md §3.2
in float32 numpy: the cell of a coordinate, the growth loop of the build with the flat-z rule, the +-1-cell neighbourhood.
`grid_geometry(..., bounded=False)` is the geometry before the slack bound existed (cell edge 1.001 r_max whatever the cell
count), kept so that the `thin_line` counterexample stays demonstrable.  The model predicts which accepted pairs lie in which
cells; the expected answer of a kernel test is always the oracle (for three_nn: tests/interp_ref.py), never the model.
"""
import numpy as np

F = np.float32
GRID_MAXC = 32768
GRID_GROW = F(1.18920712)
GRID_MARGIN = F(1.001)
GRID_SLACK = F(2.0 ** -21)
GRID_MIN_POINTS = 2048         # ops.GRID_MIN_POINTS: the grid kernel runs from here on
SIZES = (1500, 4096, 20000)    # below GRID_MIN_POINTS (scan kernel only), the register build, N > 16 384


# ---------------------------------------------------------------- float32 references (SPEC.md §1-§4)
def d2_matrix(xyz, new_xyz):
    """[M,N] §1 squared distances, point minus centre."""
    with np.errstate(over="ignore"):
        dx = xyz[None, :, 0] - new_xyz[:, None, 0]
        dy = xyz[None, :, 1] - new_xyz[:, None, 1]
        dz = xyz[None, :, 2] - new_xyz[:, None, 2]
        return (dx * dx + dy * dy) + dz * dz


def rows_from_mask(acc, S):
    """§3 rows from an [M,N] accept mask: first S accepted indices ascending, padded with the first, all 0 when none."""
    out = np.zeros((acc.shape[0], S), np.int32)
    for m in range(acc.shape[0]):
        j = np.flatnonzero(acc[m])[:S]
        if j.size:
            out[m, :j.size] = j
            out[m, j.size:] = j[0]
    return out


def ball_query_np(r, S, xyz, new_xyz, mask=None):
    with np.errstate(over="ignore"):
        r2 = F(r) * F(r)
    acc = d2_matrix(xyz, new_xyz) < r2
    return rows_from_mask(acc if mask is None else acc & mask, S)


def knn_np(k, xyz, new_xyz):
    d = d2_matrix(xyz, new_xyz)
    j = np.arange(d.shape[1])
    return np.stack([np.lexsort((j, d[m]))[:k] for m in range(d.shape[0])]).astype(np.int32)


def fps_np(xyz, M):
    mind = np.full(xyz.shape[0], np.inf, F)
    idx = np.zeros(M, np.int32)
    for i in range(1, M):
        mind = np.minimum(mind, d2_matrix(xyz, xyz[idx[i - 1]][None])[0])
        idx[i] = np.argmax(mind)             # first maximum = lowest index
    return idx


# ---------------------------------------------------------------- the grid model
def cell_coord(x, x0, inv, g):
    """floor(clamp(fl(fl(x - x0) * inv), -2, g + 1)) as integers."""
    t = (np.asarray(x, F) - F(x0)) * F(inv)
    return np.floor(np.clip(t, F(-2), F(g + 1))).astype(np.int64)


def grid_geometry(lo, hi, r_max, bounded=True):
    """The build's geometry for a bounding box [lo, hi] (finite, float32) and the largest radius.  `bounded`: grow the edge
    while (edge - r_max) * inv < GRID_SLACK * (largest per-axis cell count + 2); False = the constant 1.001 margin alone."""
    lo, hi, r_max = np.asarray(lo, F), np.asarray(hi, F), F(r_max)
    cs, steps = F(r_max * GRID_MARGIN), 0
    while True:
        inv = F(1) / cs
        f = (hi - lo) * inv
        assert steps < 128 and (f < F(2.0e9)).all(), "outside the model: the build falls back to one cell here"
        g = [int(v) + 1 for v in f]
        fits, flat = g[0] * g[1] * g[2] <= GRID_MAXC, False
        if not fits and g[2] <= 4 and g[0] * g[1] <= GRID_MAXC:
            fits = flat = True
        if fits:
            gm = max(g[0], g[1], 1 if flat else g[2])
            if not bounded or F(cs - r_max) * inv >= GRID_SLACK * F(gm + 2):
                break
        cs, steps = F(cs * GRID_GROW), steps + 1
    if flat:
        g[2] = 1
    return dict(lo=lo, inv=inv, invz=F(0) if flat else inv, g=tuple(g), cs=cs, flat=flat, steps=steps)


def scene_geometry(xyz, r_max, bounded=True):
    return grid_geometry(xyz.min(0), xyz.max(0), r_max, bounded)


def cell_gaps(geo, xyz, new_xyz, pairs=None):
    """[M,N,3] cell of the point (clamped into the grid, as the build stores it) minus cell of the centroid (as the query
    computes it, in [-2, g+1]); with `pairs` = (m, n) index arrays, [len,3] for those pairs only."""
    out = []
    for a in range(3):
        inv = geo["invz"] if a == 2 else geo["inv"]
        pc = np.clip(cell_coord(xyz[:, a], geo["lo"][a], inv, geo["g"][a]), 0, geo["g"][a] - 1)
        cc = cell_coord(new_xyz[:, a], geo["lo"][a], inv, geo["g"][a])
        out.append(pc[None, :] - cc[:, None] if pairs is None else pc[pairs[1]] - cc[pairs[0]])
    return np.stack(out, -1)


def reach(geo, xyz, new_xyz):
    """[M,N] True where the query of centroid m reads the cell of point n (the +-1 neighbourhood)."""
    return (np.abs(cell_gaps(geo, xyz, new_xyz)) <= 1).all(-1)


def accepted_pairs(xyz, new_xyz, r):
    """(m, n) index arrays of the pairs that SPEC.md §3 accepts."""
    return np.nonzero(d2_matrix(xyz, new_xyz) < F(r) * F(r))


def gap_census(geo, xyz, new_xyz, pairs):
    """Accepted pairs by their largest per-axis cell gap: (gap 0, gap exactly 1, gap 2 or more)."""
    gap = np.abs(cell_gaps(geo, xyz, new_xyz, pairs)).max(-1)
    return int((gap == 0).sum()), int((gap == 1).sum()), int((gap >= 2).sum())


def shrink_until_accepted(p, c, r, axis):
    """Move p[:, axis] down the float lattice until d2(p, c) < r*r: the pair ends one step below r^2."""
    p, r2 = p.copy(), F(r) * F(r)
    for _ in range(8):
        d = c - p
        bad = ~(((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]) < r2)
        p[bad, axis] = np.nextafter(p[bad, axis], F(-np.inf))
    return p


# ---------------------------------------------------------------- cases
class Case:
    def __init__(self, name, xyz, new_xyz, radii, nsamples, npoint=None, **stats):
        self.name = name
        self.xyz = np.ascontiguousarray(xyz, F)[None]            # [1,N,3]
        self.new_xyz = np.ascontiguousarray(new_xyz, F)[None]    # [1,M,3]
        self.radii, self.nsamples = tuple(float(F(r)) for r in radii), tuple(nsamples)
        self.N, self.M = self.xyz.shape[1], self.new_xyz.shape[1]
        self.npoint = npoint or min(self.N, 256)
        self.stats = stats
        assert np.isfinite(self.xyz).all() and np.isfinite(self.new_xyz).all()

    def __repr__(self):
        return self.name


# the counterexample to the constant margin, float32 literals: at the 1.001 margin the centroid falls in cell 29590, the point in 29592
LINE_R, LINE_X0, LINE_C, LINE_P = F(1.1077702), F(-76.27446), F(32736.535), F(32737.643)


def thin_line(N, seed=0):
    """Points along x over ~29 600 cell edges of 1.001 r (y, z constant: gy = gz = 1).  Centroid / point pairs sit on the float
    lattice with d2 one step below r^2; those that the unbounded geometry puts two cells apart are chosen first."""
    rng = np.random.default_rng(seed)
    r, M = LINE_R, 384
    span = LINE_C - LINE_X0
    cx = (LINE_X0 + rng.uniform(0.5, 1.0, 200000) * span).astype(F)
    c = np.stack([cx, np.full_like(cx, 0.25), np.full_like(cx, -1.5)], 1)
    p = c.copy()
    p[:, 0] = cx + r
    p = shrink_until_accepted(p, c, r, 0)
    old = grid_geometry([LINE_X0, 0.25, -1.5], [LINE_P, 0.25, -1.5], r, bounded=False)
    gap = cell_coord(p[:, 0], LINE_X0, old["inv"], old["g"][0]) - cell_coord(cx, LINE_X0, old["inv"], old["g"][0])
    pick = np.concatenate([np.flatnonzero(gap >= 2)[:M // 2], np.flatnonzero(gap == 1)[:M // 4], np.flatnonzero(gap == 0)[:M // 4]])
    pick = pick[:M - 1]
    c = np.concatenate([[[LINE_C, 0.25, -1.5]], c[pick]]).astype(F)
    pp = np.concatenate([[[LINE_P, 0.25, -1.5]], p[pick]]).astype(F)
    fill = np.full((N - len(pp) - 1, 3), [0, 0.25, -1.5], F)
    fill[:, 0] = (LINE_X0 + rng.uniform(0, 1, len(fill)) * span).astype(F)
    xyz = np.concatenate([[[LINE_X0, 0.25, -1.5]], fill, pp[1:], pp[:1]])       # lo = x0 exactly; the counterexample's point is the last and largest
    xyz[1:-1] = xyz[1:-1][rng.permutation(N - 2)]
    assert xyz[:, 0].max() == LINE_P and xyz[:, 0].min() == LINE_X0
    old, new, acc = scene_geometry(xyz, r, False), scene_geometry(xyz, r), accepted_pairs(xyz, c, r)
    return Case(f"thin_line-N{N}", xyz, c, (r,), (32,), g_old=old["g"], g_new=new["g"],
                census_old=gap_census(old, xyz, c, acc), census_new=gap_census(new, xyz, c, acc))


def thin_plane(N, box, seed=1):
    """181 x 181 cells of 1.001 r in x and y.  `box` False: a z extent of a few cells, so the build gives the z split up (flat);
    True: gz = 5 just misses that rule and the growth loop runs.  Pairs one step below r^2 along x and along y."""
    rng = np.random.default_rng(seed)
    r, M = F(0.75), 384
    cs = F(r * GRID_MARGIN)
    ext = np.array([180.5 * cs, 180.5 * cs, (4.5 if box else 2.5) * cs], F)
    lo = np.array([-40.0, 13.0, -2.0], F)
    c = (lo + rng.uniform(0.02, 0.98, (M, 3)) * (ext - [r, r, 0])).astype(F)
    p = c.copy()
    axis = np.arange(M) % 2
    p[np.arange(M), axis] += r
    p = np.where((axis == 0)[:, None], shrink_until_accepted(p, c, r, 0), shrink_until_accepted(p, c, r, 1))
    fill = (lo + rng.uniform(0, 1, (N - M - 2, 3)) * ext).astype(F)
    xyz = np.concatenate([[lo], fill, p, [lo + ext]]).astype(F)
    old, new, acc = scene_geometry(xyz, r, False), scene_geometry(xyz, r), accepted_pairs(xyz, c, r)
    return Case(f"thin_plane-{'box' if box else 'flat'}-N{N}", xyz, c, (r, r * F(0.5)), (32, 16), g_old=old["g"], g_new=new["g"],
                flat=new["flat"], steps=new["steps"], census_old=gap_census(old, xyz, c, acc), census_new=gap_census(new, xyz, c, acc))


def offset(N, kind, shift, seed=2):
    """A lidar-shaped or unit-cube scene in a global frame: every coordinate translated by `shift` (|shift| = 1e5 or 1e6), so one
    ulp of a coordinate is 1-10 % of the smallest radius and the subtraction in d2 (and in every pruning box) sees few distinct
    values."""
    rng = np.random.default_rng(seed)
    if kind == "kitti":
        from sad_amd import synth
        base = synth.make_scene(900 + N, N)[:, :3]
        radii = (0.4, 0.8) if abs(shift) < 5e5 else (1.6, 4.8)
    else:
        base = rng.uniform(0, 1, (N, 3)).astype(F)
        radii = (0.2, 0.4) if abs(shift) < 5e5 else (0.7, 1.0)
    xyz = (base + F(shift)).astype(F)
    new_xyz = xyz[rng.choice(N, 256, replace=False)]
    d = d2_matrix(xyz, new_xyz[:32])
    distinct = float(np.mean([np.unique(row).size for row in d]))
    ulp = float(np.spacing(F(abs(shift))))
    return Case(f"offset-{kind}{shift:+.0e}-N{N}", xyz, new_xyz, radii, (32, 64), ulp_over_rmin=ulp / min(radii),
                distinct_d2=distinct, d2_ties=int(d.size - sum(np.unique(row).size for row in d)))


def shell(n_side, r_mult, seed=3):
    """n_side^3 lattice with spacing h = 2^-3 and r = r_mult * h (r^2 exact), centroids on lattice points (r_mult whole) or on
    half points (r_mult = 1.5): many points at d2 == r^2 exactly.  A share of the points has one coordinate moved by one float
    step, which puts pairs one step inside and one step outside the shell.  r_mult picks the candidate count of a centroid's 27
    cells (1: <= 64, 1.5: 65-128, 3: > 128), which decides the path inside the query."""
    rng = np.random.default_rng(seed)
    h = F(0.125)
    ax = np.arange(n_side, dtype=F) * h
    xyz = np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), -1).reshape(-1, 3).copy()
    N = len(xyz)
    xyz = xyz[rng.permutation(N)]
    moved = rng.choice(N, N // 3, replace=False)
    ax_m, up = rng.integers(0, 3, len(moved)), rng.integers(0, 2, len(moved)).astype(bool)
    xyz[moved, ax_m] = np.nextafter(xyz[moved, ax_m], np.where(up, F(np.inf), F(-np.inf)).astype(F))
    r = F(r_mult) * h
    inner = np.arange(2, n_side - 2, dtype=F)
    cen = (inner[rng.integers(0, len(inner), (256, 3))] * h).astype(F)
    if r_mult == 1.5:
        cen[:, 0] += h * F(0.5)          # (1.5 h, 0, 0) is then a lattice offset
    geo = scene_geometry(xyz, r)
    # a few centroids on both sides of a cell border of the model: the last float below the border and the border itself
    k = np.arange(2, 10)
    border = (geo["lo"][0] + k.astype(F) * geo["cs"]).astype(F)
    for _ in range(4):
        low = cell_coord(border, geo["lo"][0], geo["inv"], geo["g"][0]) < k
        border = np.where(low, np.nextafter(border, F(np.inf)), border).astype(F)
    below = np.nextafter(border, F(-np.inf))
    on_border = int((cell_coord(border, geo["lo"][0], geo["inv"], geo["g"][0]) - cell_coord(below, geo["lo"][0], geo["inv"], geo["g"][0]) == 1).sum())
    cen[:8, 0], cen[8:16, 0] = border, below
    d, r2 = d2_matrix(xyz, cen), r * r
    cand = reach(geo, xyz, cen).sum(1)
    eps = F(2.0 ** -20)
    return Case(f"shell-r{r_mult}h-N{N}", xyz, cen, (r,), (64,), at=int((d == r2).sum()),
                inside=int(((d < r2) & (d > r2 * (1 - eps))).sum()), outside=int(((d > r2) & (d < r2 * (1 + eps))).sum()),
                cand_le64=int((cand <= 64).sum()), cand_le128=int(((cand > 64) & (cand <= 128)).sum()),
                cand_gt128=int((cand > 128).sum()), on_border=on_border)


def outside(N, flat, seed=4):
    """Centroids outside the bounding box by 0.5, 1 - eps, 1, 1 + eps and 2.5 cell edges, off every face, edge and corner
    (`flat`: a wide thin scene whose z split the build gives up, so the z offsets lie in the given-up layer)."""
    rng = np.random.default_rng(seed)
    r = F(0.5)
    ext = np.array([60, 60, 1.2] if flat else [8, 8, 8], F)
    xyz = (rng.uniform(0, 1, (N, 3)) * ext).astype(F)
    xyz[:64] = (rng.integers(0, 2, (64, 3)) * ext).astype(F)          # points on the corners, so the faces are populated
    geo = scene_geometry(xyz, r)
    lo, hi, cs = xyz.min(0), xyz.max(0), geo["cs"]
    cen = []
    for d in np.ndindex(3, 3, 3):
        d = np.array(d) - 1
        if not d.any():
            continue
        for k in (0.5, 1 - 1e-6, 1.0, 1 + 1e-6, 2.5):
            anchor = xyz[rng.integers(0, N)]
            cen.append(np.where(d > 0, hi + F(k) * cs, np.where(d < 0, lo - F(k) * cs, anchor)))
    cen = np.array(cen, F)
    rr = reach(geo, xyz, cen)
    acc = d2_matrix(xyz, cen) < r * r
    return Case(f"outside-{'flat' if flat else 'box'}-N{N}", xyz, cen, (r, r * F(0.4)), (32, 8), flat=geo["flat"],
                with_candidates=int(rr.any(1).sum()), with_accepted=int(acc.any(1).sum()), missed=int((acc & ~rr).sum()),
                clamped=int(np.any([(cc == -2) | (cc == g + 1) for cc, g in
                                    ((cell_coord(cen[:, a], lo[a], geo["inv"], geo["g"][a]), geo["g"][a]) for a in range(2))], 0).sum()))


def tiny(N, e, seed=5):
    """A unit cube scaled by 2^-e (e = 60 .. 70): the terms of d2 are subnormal or zero, and so is r^2.  -0.0 mixed in."""
    rng = np.random.default_rng(seed)
    s = F(2.0 ** -e)
    xyz = (rng.integers(0, 1 << 12, (N, 3)).astype(F) * F(2.0 ** -12)) * s
    z = rng.choice(N, N // 16, replace=False)
    xyz[z, rng.integers(0, 3, len(z))] = F(-0.0)
    new_xyz = xyz[rng.choice(N, 192, replace=False)].copy()
    new_xyz[:16, 1] = F(-0.0)
    radii = (F(0.11) * s, F(0.3) * s)
    dx = xyz[None, :, 0] - new_xyz[:, None, 0]
    t = dx * dx
    d = d2_matrix(xyz, new_xyz)
    tinyf = float(np.finfo(F).tiny)
    return Case(f"tiny-2^-{e}-N{N}", xyz, new_xyz, radii, (32, 64), normal_terms=int((t >= tinyf).sum()),
                subnormal_terms=int(((t > 0) & (t < tinyf)).sum()), zero_terms=int(((t == 0) & (dx != 0)).sum()),
                r2_subnormal=bool(0 < radii[1] * radii[1] < tinyf), neg_zero=int(np.signbit(xyz[xyz == 0]).sum()),
                accepted=int((d < radii[0] * radii[0]).sum()))


def huge(N, seed=6):
    """Finite coordinates +-[1e19, 2e19]: d2 overflows to +inf between points of opposite sign and stays finite otherwise.
    The second radius squares to +inf, so it accepts exactly the finite d2."""
    rng = np.random.default_rng(seed)
    xyz = (rng.uniform(1e19, 2e19, (N, 3)) * rng.choice([-1.0, 1.0], (N, 3), p=[0.3, 0.7])).astype(F)
    new_xyz = xyz[rng.choice(N, 192, replace=False)]
    radii = (F(6e18), F(2e19))
    d = d2_matrix(xyz, new_xyz)
    with np.errstate(over="ignore"):
        r2 = [r * r for r in radii]
    return Case(f"huge-N{N}", xyz, new_xyz, radii, (32, 64), inf_d2=int(np.isinf(d).sum()), finite_d2=int(np.isfinite(d).sum()),
                r2_inf=bool(np.isinf(r2[1])), accepted=int((d < r2[0]).sum()))


def outlier(N, n_out, seed=7):
    """A unit cube plus 1-3 points at 1e6: the growth loop of the grid runs tens of steps, and almost every point shares one cell
    (of the grid, and of the Z-order the bucketed FPS kernels sort by)."""
    rng = np.random.default_rng(seed)
    xyz = rng.uniform(0, 1, (N, 3)).astype(F)
    where = rng.choice(N, n_out, replace=False)
    xyz[where] = [[1e6, 0.5, 0.5], [1e6, 1e6, 1e6], [-1e6, 0.25, 1e6]][:n_out]
    new_xyz = np.concatenate([xyz[where], xyz[rng.choice(N, 200, replace=False)]])
    r = F(0.05)
    geo = scene_geometry(xyz, r)
    pc = [np.clip(cell_coord(xyz[:, a], geo["lo"][a], geo["inv"], geo["g"][a]), 0, geo["g"][a] - 1) for a in range(3)]
    biggest = int(np.unique(np.stack(pc, 1), axis=0, return_counts=True)[1].max())
    return Case(f"outlier{n_out}-N{N}", xyz, new_xyz, (r, r * F(2)), (32, 64), steps=geo["steps"], g=geo["g"], biggest_cell=biggest)


def exhaust(N, seed=8):
    """K = 37 distinct points, each many times over, sampled with M = N: every min-distance reaches 0 after K picks and the
    argmax must fall back to index 0 from then on."""
    rng = np.random.default_rng(seed)
    K = 37
    src = rng.uniform(-3, 3, (K, 3)).astype(F)
    xyz = src[np.concatenate([np.arange(K), rng.integers(0, K, N - K)])][rng.permutation(N)]
    new_xyz = xyz[:128]
    return Case(f"exhaust-N{N}", xyz, new_xyz, (0.5,), (64,), npoint=N, distinct=int(np.unique(xyz, axis=0).shape[0]))


BUILDERS = {
    "thin_line": [(thin_line, (n,)) for n in SIZES],
    "thin_plane": [(thin_plane, (1500, False)), (thin_plane, (4096, False)), (thin_plane, (20000, False)), (thin_plane, (4096, True)),
                   (thin_plane, (20000, True))],
    "offset": [(offset, (1500, "cube", -1e5)), (offset, (4096, "cube", 1e6)), (offset, (4096, "kitti", -1e6)), (offset, (20000, "kitti", 1e5))],
    "shell": [(shell, (12, 1)), (shell, (16, 1)), (shell, (16, 1.5)), (shell, (16, 3)), (shell, (26, 1.5))],
    "outside": [(outside, (1500, False)), (outside, (4096, False)), (outside, (20000, True))],
    "tiny": [(tiny, (1500, 60)), (tiny, (4096, 65)), (tiny, (4096, 70))],
    "huge": [(huge, (1500,)), (huge, (4096,))],
    "outlier": [(outlier, (1500, 1)), (outlier, (4096, 3)), (outlier, (20000, 2))],
    "exhaust": [(exhaust, (5000,)), (exhaust, (16384,))],
}
CASE_IDS = [f"{reg}{i}" for reg, lst in BUILDERS.items() for i in range(len(lst))]
_cache = {}


def case(case_id):
    """Case by id (`<regime><n>`), built once per process."""
    if case_id not in _cache:
        reg = case_id.rstrip("0123456789")
        fn, args = BUILDERS[reg][int(case_id[len(reg):])]
        _cache[case_id] = fn(*args)
    return _cache[case_id]


def ids(*regimes):
    return [c for c in CASE_IDS if c.rstrip("0123456789") in regimes]


# ---------------------------------------------------------------- the randomized search that found the thin_line counterexample
def line_search(scenes, pairs, cells, bounded, seed=0):
    """`scenes` random line-like scenes (y, z constant) of 0.9-1.0 x `cells` cell edges of 1.001 r, `pairs` centroid / point pairs
    each one step below r^2.  Returns (accepted pairs two or more cells apart, largest gap seen, largest cell count)."""
    rng = np.random.default_rng(seed)
    bad = worst = gmax = 0
    for _ in range(scenes):
        r = F(rng.uniform(0.5, 2))
        E = F(rng.uniform(0.9, 1.0) * cells * F(r * GRID_MARGIN))
        x0 = F(rng.uniform(-1, 1) * rng.choice([1e-3, 1, 100]))
        c = (x0 + rng.uniform(0.5, 1, pairs) * E).astype(F)
        p = (c + r).astype(F)
        for _ in range(4):
            dx = p - c
            p = np.where(dx * dx < r * r, p, np.nextafter(p, F(-np.inf)))
        dx = p - c
        ok = dx * dx < r * r
        geo = grid_geometry([x0, 0, 0], [max(c.max(), p.max()), 0, 0], r, bounded)
        gap = cell_coord(p, x0, geo["inv"], geo["g"][0]) - cell_coord(c, x0, geo["inv"], geo["g"][0])
        bad += int((ok & (gap >= 2)).sum())
        worst, gmax = max(worst, int(gap[ok].max())), max(gmax, geo["g"][0])
    return bad, worst, gmax
