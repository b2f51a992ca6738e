"""Input families that take the integer-only kernels (csrc/voxel.hip, the rulebook half of csrc/spconv.hip, csrc/vox_hash.h) to
the edges of what the C ABI admits: geometries, grid sizes, scene counts, row counts and hash probe runs that the families of
spconv_cases.py / voxel_cases.py never reach.  Shared by test_index_space_cpu.py and test_gpu_index_space.py.

Every family is a builder plus a coverage condition asserted on the REFERENCE's output (spconv_ref.index_loop, voxel_ref) before
anything is compared, so a changed generator cannot silently lose what the family is for.  Builders print one coverage line.

A sparse-conv case is a ``SpCase``; its reference rulebooks come from ``reference(case, gi)`` (computed once, shared, read-only).
A voxel case is (name, points [total,C] f32, offsets [B+1] int32, dict(v, r, T, V)) as in voxel_cases.py."""
import functools
from typing import NamedTuple

import numpy as np

import spconv_ref as ref
import voxel_ref

F = np.float32
INT_MAX = 2 ** 31 - 1
HIGH = 2 ** 31 - 2 ** 24            # linear indices above this differ from a float32's neighbours by 128


class SpCase(NamedTuple):
    name: str
    coors: np.ndarray       # [Nv,3] int32 (z,y,x)
    off: np.ndarray         # [B+1] int32
    G: tuple
    geos: tuple             # ((name, K, s, p, subm), ...)
    small: bool             # the grid is small enough for spconv_ref.index_vec (a dense array per scene)


def gname(K, s, p, subm):
    j = lambda t: "".join(str(v) for v in t) if max(t) < 10 else "_".join(str(v) for v in t)
    return f"subm{j(K)}" if subm else f"k{j(K)}s{j(s)}p{j(p)}"


def geo(K, s=1, p=0, subm=False):
    t3 = lambda v: (int(v),) * 3 if isinstance(v, int) else tuple(int(x) for x in v)
    K, s, p = t3(K), t3(s), t3(p)
    if subm:
        s, p = (1, 1, 1), tuple(k // 2 for k in K)
    return (gname(K, s, p, subm), K, s, p, subm)


def fits(G, g):
    _, K, s, p, _ = g
    O = [(a + 2 * q - k) // t + 1 if a + 2 * q - k >= 0 else 0 for a, q, k, t in zip(G, p, K, s)]
    return min(O) >= 1 and O[0] * O[1] * O[2] <= INT_MAX


@functools.lru_cache(maxsize=None)
def _reference(key):
    case, gi = _CASES[key[0]], key[1]
    _, K, s, p, subm = case.geos[gi]
    out = ref.index_loop(case.coors, case.off, case.G, K, s, p, subm)
    for a in out:
        a.setflags(write=False)
    return out


_CASES = {}


def reference(case, gi):
    """(out_coors, out_offsets, nbr) of geometry ``gi`` of ``case`` by spconv_ref.index_loop: a dict walk that allocates nothing
    of the size of the grid.  Computed once per process; the arrays are read-only."""
    _CASES.setdefault(case.name, case)
    assert _CASES[case.name] is case, f"two cases named {case.name}"
    return _reference((case.name, gi))


def _join(scenes):
    off = np.concatenate([[0], np.cumsum([len(s) for s in scenes])]).astype(np.int32)
    rows = [np.asarray(s, np.int64).reshape(-1, 3) for s in scenes]
    return np.ascontiguousarray(np.concatenate(rows).astype(np.int32)), off


def linear(c, G):
    c = np.asarray(c, np.int64)
    return (c[:, 0] * G[1] + c[:, 1]) * G[2] + c[:, 2]


def nbr_by_key(case, gi, key):
    """A third form of nbr, through a LINEAR cell key as the kernels hold it: the lowest row of every (scene, key) by np.unique,
    one sorted lookup per (output row, kernel offset).  ``key(z, y, x)`` -> int64; with the right formula this is the
    reference's nbr, with a wrong one it shows what the wrong formula would give."""
    _, K, s, p, subm = case.geos[gi]
    G, K, s, p, O = ref.geometry(case.G, K, s, p, subm)
    oc, oo, _ = reference(case, gi)
    c = np.asarray(case.coors, np.int64)
    kin = ref.scene_ids(case.off) * 2 ** 32 + key(c[:, 0], c[:, 1], c[:, 2])
    uniq, first = np.unique(kin, return_index=True)                     # the first occurrence = the lowest row
    q = np.asarray(oc, np.int64)[:, None, :] * np.asarray(s) - np.asarray(p) + ref.offsets_k(K)[None, :, :]
    inside = ((q >= 0) & (q < np.asarray(G))).all(-1)
    kq = ref.scene_ids(oo)[:, None] * 2 ** 32 + key(q[..., 0], q[..., 1], q[..., 2])
    pos = np.minimum(np.searchsorted(uniq, kq), max(len(uniq) - 1, 0))
    hit = inside & (uniq[pos] == kq) if len(uniq) else np.zeros(kq.shape, bool)
    return np.where(hit, first[pos] if len(uniq) else 0, -1).astype(np.int32).reshape(len(oc), K[0] * K[1] * K[2])


def pool_grad_vec(g, arg, nbrT):
    """spconv_pool_ref.max_pool_grad_loop with the rows vectorised: the same float32 additions in the same kk order."""
    g, arg, nbrT = np.asarray(g, F), np.asarray(arg, np.int32), np.asarray(nbrT, np.int64)
    (No, C), (Nv, Kvol) = g.shape, nbrT.shape
    acc = np.zeros((Nv, C), F)
    if No == 0:
        return acc
    rows = np.arange(Nv)[:, None]
    for kk in range(Kvol):
        o = nbrT[:, kk]
        ok = (o >= 0) & (o < No)
        o = np.where(ok, o, 0)
        acc = np.where(ok[:, None] & (arg[o] == rows), (acc + g[o]).astype(F), acc)
    return acc


# ---- geometry sweep ---------------------------------------------------------------------------------------------------
SWEEP_WRITTEN = (
    geo(1, 2, 0), geo(2, 3, 0), geo(3, 1, 2), geo(3, 1, 0), geo((3, 2, 1), (1, 2, 3), (0, 1, 2)), geo(2, 1, 1), geo(3, 4, 3),
    geo((1, 3, 3), (3, 1, 2), (0, 1, 1)),
    geo((3, 1, 1), subm=True), geo((1, 3, 1), subm=True), geo((1, 1, 3), subm=True), geo((3, 3, 1), subm=True), geo((1, 3, 3), subm=True),
)
SWEEP_GRIDS = {"mixA": (4, 6, 9), "mixB": (5, 7, 9), "odd": (7, 9, 8)}
N_DRAWN = 40


def _density_cells(rng, G, density, lattice=None):
    z, y, x = np.meshgrid(*[np.arange(g) for g in G], indexing="ij")
    c = np.stack([z, y, x], -1).reshape(-1, 3)
    if lattice == "odd":
        c = c[(c % 2 == 1).all(1)]
    c = c[rng.random(len(c)) < density] if density < 1.0 else c
    return c[rng.permutation(len(c))]


def _sweep_inputs():
    """Three inputs of B = 3 on grids of at most 9 cells per axis; densities 0.05, 0.3 and 1.0 mixed, one empty scene in each.
    ``odd`` holds cells with three odd coordinates only (no output site at stride 2 without padding)."""
    rng = np.random.default_rng(4242)
    e = np.zeros((0, 3), np.int64)
    A, Bg, Og = SWEEP_GRIDS["mixA"], SWEEP_GRIDS["mixB"], SWEEP_GRIDS["odd"]
    return {"mixA": _join([_density_cells(rng, A, 0.05), e, _density_cells(rng, A, 1.0)]),
            "mixB": _join([_density_cells(rng, Bg, 0.3), e, _density_cells(rng, Bg, 1.0, "odd")]),
            "odd": _join([_density_cells(rng, Og, 1.0, "odd"), e, _density_cells(rng, Og, 0.3, "odd")])}


def _drawn_geometries():
    """N_DRAWN geometries drawn once from K in 1..3, s in 1..4, p in 0..3 per axis, dealt to the three inputs in turn; a draw
    that does not fit its input's grid is drawn again."""
    rng = np.random.default_rng(777)
    names = sorted(SWEEP_GRIDS)
    out = {n: [] for n in names}
    k = 0
    while k < N_DRAWN:
        g = geo(tuple(rng.integers(1, 4, 3)), tuple(rng.integers(1, 5, 3)), tuple(rng.integers(0, 4, 3)))
        n = names[k % 3]
        if fits(SWEEP_GRIDS[n], g) and g not in out[n] and g not in SWEEP_WRITTEN:
            out[n].append(g)
            k += 1
    return out


@functools.lru_cache(maxsize=None)
def family_sweep():
    inputs, drawn = _sweep_inputs(), _drawn_geometries()
    cases = tuple(SpCase(f"sweep_{n}", c, o, SWEEP_GRIDS[n], SWEEP_WRITTEN + tuple(drawn[n]), True) for n, (c, o) in sorted(inputs.items()))
    assert sum(len(c.geos) for c in cases) == 3 * len(SWEEP_WRITTEN) + N_DRAWN
    got = {"scene_no0": 0, "batch_no0": 0, "unread_rows": 0, "O_gt_G": 0, "O_is_1": 0, "full_row_k8": 0}
    for case in cases:
        assert max(case.G) <= 9 and len(case.off) == 4 and (np.diff(case.off) == 0).sum() == 1
        for gi, (_, K, s, p, subm) in enumerate(case.geos):
            oc, oo, nbr = reference(case, gi)
            O = ref.geometry(case.G, K, s, p, subm)[4]
            nv, no = np.diff(case.off), np.diff(oo)
            got["scene_no0"] += int(((nv > 0) & (no == 0)).sum())
            got["batch_no0"] += int(no.sum() == 0)
            got["unread_rows"] += len(case.coors) - len(np.unique(nbr[nbr >= 0]))
            got["O_gt_G"] += int(all(a >= b for a, b in zip(O, case.G)) and O != tuple(case.G))
            got["O_is_1"] += int(min(O) == 1)
            got["full_row_k8"] += int(nbr.shape[1] == 8 and bool((nbr >= 0).all(1).any()))
    print("sweep coverage:", got)
    assert all(v > 0 for v in got.values()), got
    return cases


# ---- stride and padding at the ABI limit -------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def family_limit():
    G = (1, 1, 200000)
    g = geo((1, 1, 3), (1, 1, 65535), (0, 0, 65535))
    rng = np.random.default_rng(5)
    xs = np.concatenate([[0, 1, 2], np.arange(65535, 65538), np.arange(131070, 131073), np.arange(196605, 196608)])
    decoys = rng.choice(np.setdiff1d(np.arange(200000), xs), 200, replace=False)

    def scene(x):
        return np.stack([np.zeros(len(x), np.int64), np.zeros(len(x), np.int64), x], -1)
    both = np.concatenate([xs, decoys])
    case = SpCase("limit", *_join([scene(rng.permutation(both)), scene(rng.permutation(decoys)), scene(xs[::-1])]), G, (g,), False)
    O = ref.geometry(G, *g[1:4])[4]
    oc, oo, nbr = reference(case, 0)
    assert O == (1, 1, 6), O
    no = np.diff(oo)
    print(f"limit coverage: O = {O}, No per scene = {no.tolist()}")
    # site o reads x = (o - 1) * 65535 + k: sites 1 .. 4 have their whole window in the grid, 0 and 5 none of it
    assert no.tolist() == [4, 0, 4] and sorted(oc[:4, 2].tolist()) == [1, 2, 3, 4] and (nbr >= 0).all()
    return (case,)


# ---- large grids ---------------------------------------------------------------------------------------------------------
LARGE_GRIDS = ((41, 1600, 1408), (1290, 1290, 1290), (1, 46340, 46340), (1, 1, 2 ** 31 - 1))
ANISO = LARGE_GRIDS[0]                  # Gy != Gx, both above 1
LARGE_GEOS = (geo(3, subm=True), geo(1, subm=True), geo(3, 2, 1), geo(2, 2, 0))


def _large_scene_cells(G, rng):
    """The eight corners and their in-grid neighbours, a full 3x3x3 block against the far corner, about 200 random cells."""
    Ga = np.asarray(G, np.int64)
    corners = np.array([[a, b, c] for a in (0, G[0] - 1) for b in (0, G[1] - 1) for c in (0, G[2] - 1)], np.int64)
    steps = np.array([[d if a == ax else 0 for a in range(3)] for ax in range(3) for d in (-1, 1)], np.int64)
    near = (corners[:, None, :] + steps[None, :, :]).reshape(-1, 3)
    blk = np.stack(np.meshgrid(*[np.arange(max(0, g - 3), g) for g in G], indexing="ij"), -1).reshape(-1, 3)
    rnd = np.stack([rng.integers(0, g, 200) for g in G], -1)
    c = np.concatenate([corners, near, blk, rnd])
    c = c[((c >= 0) & (c < Ga)).all(1)]
    return np.unique(c, axis=0)


@functools.lru_cache(maxsize=None)
def family_large():
    """Two scenes of the same few hundred cells (in different orders, each with duplicated rows) on grids up to 2^31 - 1 cells.
    A geometry that does not fit a grid (an even kernel on an axis of one cell) runs with its kernel clipped to the grid."""
    cases = []
    for G in LARGE_GRIDS:
        rng = np.random.default_rng(G[1])
        cells = _large_scene_cells(G, rng)
        if G == ANISO:
            # (z, Gx + 1, x) and (z + 1, 0, x): with Gy and Gx exchanged in the key, the second's +y neighbour IS the first
            assert G[1] > G[2] + 1
            cells = np.unique(np.concatenate([cells, [[5, G[2] + 1, 77], [6, 0, 77]]]), axis=0)
        scenes = []
        for _ in range(2):
            c = np.concatenate([cells, cells[rng.integers(0, len(cells), 40)]])
            scenes.append(c[rng.permutation(len(c))])
        geos = list(LARGE_GEOS) + ([geo(3, 1, 1)] if G == ANISO else [])
        geos = [g if fits(G, g) else geo(tuple(min(k, a) for k, a in zip(g[1], G)), g[2], g[3]) for g in geos]
        assert all(fits(G, g) for g in geos)
        case = SpCase("large_" + "x".join(str(g) for g in G), *_join(scenes), G, tuple(geos), False)
        lin = np.unique(linear(case.coors, G))
        assert lin.min() >= 0 and lin.max() < G[0] * G[1] * G[2] <= INT_MAX
        merged = int((np.diff(lin.astype(F)) == 0).sum())
        print(f"{case.name} coverage: {len(case.coors)} rows, largest linear index {lin.max()} (2^31 - 2^24 = {HIGH}), "
              f"{merged} neighbouring pairs of distinct cells equal as float32")
        assert merged > 0
        if G[0] * G[1] * G[2] > HIGH:
            assert lin.max() > HIGH
        if G == ANISO:
            right = nbr_by_key(case, 0, lambda z, y, x: (z * G[1] + y) * G[2] + x)
            wrong = nbr_by_key(case, 0, lambda z, y, x: (z * G[2] + y) * G[1] + x)
            assert np.array_equal(right, reference(case, 0)[2])
            diff = int((wrong != right).sum())
            print(f"{case.name} coverage: exchanging Gy and Gx in the key changes {diff} entries of nbr")
            assert diff > 0
        cases.append(case)
    assert sum(G[0] * G[1] * G[2] > HIGH for G in LARGE_GRIDS) == 3
    return tuple(cases)


# ---- many scenes -----------------------------------------------------------------------------------------------------------
# scene -> rows; every other scene is empty.  B = 1000 has runs of at least 20 empty scenes at the start, in the middle and at
# the end.  B = 40 has no room for three such runs beside its non-empty scenes: 20 at the start, shorter ones after.
MANY = {40: {20: 1, 21: 63, 23: 64, 29: 65, 30: 300, 33: 17},
        1000: {25: 1, 26: 63, 27: 64, 500: 65, 501: 300, 502: 1, 975: 200, 979: 64}}
MANY_GEOS = (geo(3, subm=True), geo(3, 2, 1), geo(2, 2, 0))


def _many_check(B, sizes):
    n = np.array([sizes.get(b, 0) for b in range(B)])
    assert any(b >= 16 and n[b] > 0 and n[b - 1] == 0 for b in range(1, B)), "no non-empty scene >= 16 after an empty one"
    assert {1, 63, 64, 65} <= set(n.tolist()) and n.max() >= 200 and (n == 0).sum() > B // 2
    runs = [len(r) for r in "".join("e" if v == 0 else " " for v in n).split()]
    assert n[0] == 0 and runs[0] >= 20 and len(runs) >= 3
    if B >= 100:
        assert n[-1] == 0 and runs[-1] >= 20 and max(runs[1:-1]) >= 20
    return n


@functools.lru_cache(maxsize=None)
def family_many_sp():
    G = (6, 10, 12)
    cases = []
    for B, sizes in MANY.items():
        n = _many_check(B, sizes)
        rng = np.random.default_rng(B)
        scenes = []
        for b in range(B):
            pick = rng.choice(G[0] * G[1] * G[2], n[b], replace=False)
            scenes.append(np.stack(np.unravel_index(pick, G), -1).reshape(-1, 3))
        cases.append(SpCase(f"many_B{B}", *_join(scenes), G, MANY_GEOS, True))
        print(f"many_B{B} coverage: non-empty scenes {sorted(sizes)} of {B}")
    return tuple(cases)


def family_many_voxel(C=4):
    par = dict(v=(0.5, 0.5, 0.5), r=(0, 0, 0, 8, 8, 4), T=4, V=64)
    cases = []
    for B, sizes in MANY.items():
        n = _many_check(B, sizes)
        rng = np.random.default_rng(B + 1)
        off = np.concatenate([[0], np.cumsum(n)]).astype(np.int32)
        pts = (rng.random((int(off[-1]), C)) * ([9, 9, 5] + [1] * (C - 3)) - 0.5).astype(F)       # some fall outside the range
        num = voxel_ref.voxel_index(pts, off, par["v"], par["r"], par["V"])[3]
        assert num.max() == par["V"] and (num[n == 0] == 0).all() and par["V"] <= 64
        cases.append((f"many_B{B}", pts, off, par))
    return cases


# ---- more than 65,536 rows: scan_in_place of vox_hash.h takes chunks of 2 and more --------------------------------------
@functools.lru_cache(maxsize=None)
def family_rows_sp():
    G = (12, 20, 24)
    rng = np.random.default_rng(65536)
    n0, n1 = 1200, 1301
    scenes = [np.stack(np.unravel_index(rng.choice(G[0] * G[1] * G[2], n, replace=False), G), -1) for n in (n0, n1)]
    case = SpCase("rows_2501", *_join(scenes), G, (geo(3, 2, 1), geo(3, 1, 1)), True)
    NC = len(case.coors) * 27
    nw = (NC + 63) // 64
    print(f"rows_2501 coverage: Nv * Kvol = {NC}, nw = {nw}")
    assert NC > 65536 and NC % 64 != 0 and nw > 1024
    return (case,)


def family_rows_voxel(C=4):
    rng = np.random.default_rng(70001)
    off = np.array([0, 30000, 30001, 70001], np.int32)
    par = dict(v=(0.4, 0.4, 4), r=(0, -40, -3, 70.4, 40, 1), T=4, V=2000)
    pts = (rng.random((70001, C)) * ([76, 86, 5] + [1] * (C - 3)) + ([-3, -43, -3.5] + [0] * (C - 3))).astype(F)
    nw = (len(pts) + 63) // 64
    num = voxel_ref.voxel_index(pts, off, par["v"], par["r"], par["V"])[3]
    print(f"rows_70001 coverage: nw = {nw}, voxel_num = {num.tolist()}")
    assert len(pts) == 70001 and nw > 1024
    return [("rows_70001", pts, off, par)]


# ---- probe runs that wrap: the one WHITE-BOX family ------------------------------------------------------------------------
# A Python model of CoordTable's constructor (capacity, shift) and slot0 of csrc/vox_hash.h.  If the hash there changes (the multiplier, the key layout
# scene << 32 | cell, the capacity rule), this model must change with it: the coverage assertions below are made on the model.
HASH_MULT = 0x9E3779B97F4A7C15
MASK64 = 2 ** 64 - 1


def hash_capacity(keys):
    """-> (cap, shift): the power of two >= 2 * keys (>= 2) and the shift that maps a 64-bit hash onto it."""
    cap, lg = 2, 1
    while cap < 2 * keys:
        cap, lg = cap << 1, lg + 1
    return cap, 64 - lg


def hash_key(scene, cell):
    return (int(scene) << 32) | int(cell)


def hash_slot0(k64, shift):
    return ((int(k64) * HASH_MULT) & MASK64) >> shift


def hash_slot0_vec(k64, shift):
    with np.errstate(over="ignore"):
        return (np.asarray(k64, np.uint64) * np.uint64(HASH_MULT)) >> np.uint64(shift)


def probe_model(keys, cap, shift):
    """Open-addressing insert (linear probing, ``(h + 1) & mask``) of ``keys`` in order -> (slot of every key, table).  The set
    of occupied slots does not depend on the order, so the runs are those of the kernel's table whatever order its atomics take."""
    table, slots = {}, []
    for k in keys:
        h = hash_slot0(k, shift)
        while h in table and table[h] != k:
            h = (h + 1) & (cap - 1)
        table[h] = k
        slots.append(h)
    return slots, table


def probe_runs(table, cap):
    """-> (longest circular run of occupied slots, True if a run crosses from slot cap - 1 to slot 0)."""
    occ = np.zeros(cap, bool)
    occ[list(table)] = True
    if occ.all():
        return cap, True
    start = int(np.flatnonzero(~occ)[0])
    rolled = np.roll(occ, -start)                         # now slot 0 of the roll is empty: no run wraps
    best = run = 0
    for v in rolled:
        run = run + 1 if v else 0
        best = max(best, run)
    return best, bool(occ[cap - 1] and occ[0])


PROBE_G = (1290, 1290, 1290)
PROBE_VOX = dict(v=(0.05, 0.05, 0.05), r=(0, 0, 0, 64.5, 64.5, 64.5), T=2, V=256)
PROBE_GEOS = (geo(3, subm=True), geo(1, subm=True), geo(1, 1, 0), geo(3, 2, 1))


def _centres(cells):
    """[n,3] (z,y,x) -> voxel centres (x,y,z) float32 of PROBE_VOX, and which of them the §20.1 arithmetic maps back."""
    c = np.asarray(cells, np.int64)
    pts = ((c[:, ::-1] + 0.5) * 0.05).astype(F)
    g, valid = voxel_ref.point_cells(pts, PROBE_VOX["v"], PROBE_VOX["r"])
    return pts, valid & (g[:, ::-1] == c).all(1)


@functools.lru_cache(maxsize=None)
def _probe_rows():
    per, dups = 110, 9
    rows = 2 * (per + dups)
    cap, shift = hash_capacity(rows)
    rng = np.random.default_rng(99)
    G = PROBE_G
    assert voxel_ref.grid_size(PROBE_VOX["v"], PROBE_VOX["r"]) == G[::-1]
    scenes = []
    for b in range(2):
        cand = np.unique(rng.integers(0, G[0] * G[1] * G[2], 400000))
        home = hash_slot0_vec((b << 32) | cand, shift)
        cand = cand[home >= cap - 3]
        cells = np.stack(np.unravel_index(cand, G), -1)
        cells = cells[_centres(cells)[1]][:per]
        assert len(cells) == per
        c = np.concatenate([cells, cells[rng.integers(0, per, dups)]])
        scenes.append(c[rng.permutation(len(c))])
    coors, off = _join(scenes)
    keys = [hash_key(b, k) for b, k in zip(ref.scene_ids(off), linear(coors, G))]
    slots, table = probe_model(keys, cap, shift)
    longest, wraps = probe_runs(table, cap)
    homes = [hash_slot0(k, shift) for k in keys]
    print(f"probe coverage: {len(keys)} rows, {len(table)} keys, capacity {cap}, longest probe run {longest}, crosses the last slot: {wraps}")
    assert 100 <= len(table) <= 300 and min(homes) >= cap - 3 and longest >= 64 and wraps
    assert any(s < h for s, h in zip(slots, homes)), "no key was placed past slot 0"
    assert len(set(keys)) < len(keys), "no duplicate rows"
    return coors, off


@functools.lru_cache(maxsize=None)
def family_probe_sp():
    coors, off = _probe_rows()
    one = SpCase("probe_one_key", np.array([[1289, 0, 645]], np.int32), np.array([0, 1], np.int32), PROBE_G, PROBE_GEOS, False)
    assert hash_capacity(len(one.coors))[0] == 2
    # K = 1, s = 1, p = 0 (strided): the second table is keyed by the output site = the input cell, and has the same size
    assert PROBE_GEOS[2][1:] == ((1, 1, 1), (1, 1, 1), (0, 0, 0), False)
    return (SpCase("probe_wrap", coors, off, PROBE_G, PROBE_GEOS, False), one)


def family_probe_voxel():
    coors, off = _probe_rows()
    pts, ok = _centres(coors)
    assert ok.all()
    want = linear(coors, PROBE_G)
    key, _ = voxel_ref.keys_of(pts, PROBE_VOX["v"], PROBE_VOX["r"])
    assert np.array_equal(key, want), "a voxel centre does not fall into its cell"
    p1, ok1 = _centres([[1289, 0, 645]])
    assert ok1.all() and hash_capacity(1)[0] == 2
    return [("probe_wrap", np.ascontiguousarray(pts), off, PROBE_VOX),
            ("probe_one_key", np.ascontiguousarray(p1), np.array([0, 1], np.int32), PROBE_VOX)]


# ---- voxel limit grid ---------------------------------------------------------------------------------------------------------
LIMIT_VOX = dict(v=(0.05, 0.05, 0.05), r=(0, 0, 0, 64.5, 64.5, 64.5), T=4, V=4096)
DENORM = float(np.float32(1e-45))                     # the smallest positive binary32 denormal


def limit_specials():
    """name -> xyz (float32) of the points §20.1's binary32 subtract, divide and floor decide at the edge."""
    hi, mid = F(64.5), F(30.0)
    sp = {}
    for d, ax in enumerate("xyz"):
        def at(v):
            p = np.full(3, mid, F)
            p[d] = v
            return p
        sp[f"hi_face_{ax}"] = at(hi)
        sp[f"lo_face_{ax}"] = at(F(0.0))
        sp[f"neg_zero_{ax}"] = at(F(-0.0))
        sp[f"neg_denormal_{ax}"] = at(F(-DENORM))
        sp[f"pos_denormal_{ax}"] = at(F(DENORM))
        sp[f"below_hi_{ax}"] = at(np.nextafter(hi, F(-np.inf), dtype=F))
        for v in (3e38, -3e38, 1e30, -1e30):
            sp[f"huge_{v:g}_{ax}"] = at(F(v))
    return sp


def family_limit_voxel(C=4):
    p = LIMIT_VOX
    G = voxel_ref.grid_size(p["v"], p["r"])
    assert G == (1290, 1290, 1290), G
    rng = np.random.default_rng(1290)
    sp = limit_specials()
    rnd = (rng.random((3000, 3)) * 64.5).astype(F)
    last = (64.45 + rng.random((60, 3)) * 0.049).astype(F)            # the last voxel of every axis at once ...
    for d in range(3):                                                # ... and of one axis at a time
        e = (rng.random((40, 3)) * 64.5).astype(F)
        e[:, d] = (64.45 + rng.random(40) * 0.049).astype(F)
        last = np.concatenate([last, e])
    special = np.stack(list(sp.values()))
    scenes = []
    for b in range(2):
        s = np.concatenate([rnd[b::2], last, special, special[::3]])
        scenes.append(s[rng.permutation(len(s))])
    off = np.concatenate([[0], np.cumsum([len(s) for s in scenes])]).astype(np.int32)
    xyz = np.concatenate(scenes)
    pts = np.ascontiguousarray(np.concatenate([xyz, rng.standard_normal((len(xyz), C - 3)).astype(F)], 1)) if C > 3 else np.ascontiguousarray(xyz)
    key, _ = voxel_ref.keys_of(pts, p["v"], p["r"])
    bits = pts[:, :3].view(np.uint32)
    verdict = {}
    for name, q in sp.items():
        rows = np.flatnonzero((bits == q.view(np.uint32)).all(1))         # bit patterns: -0.0 is not 0.0
        assert len(rows) >= 2, f"{name} is missing"
        v = set((key[rows] >= 0).tolist())
        assert len(v) == 1
        verdict[name] = v.pop()
    for name, ok in verdict.items():
        if name.startswith(("neg_denormal", "huge")):
            assert not ok, f"the reference takes {name} for a valid point"
        if name.startswith(("pos_denormal", "lo_face", "neg_zero", "below_hi")):
            assert ok, f"the reference takes {name} for an invalid point"
    print(f"limit_voxel coverage: {len(pts)} points, max_key {key.max()} (2^31 - 2^24 = {HIGH}), invalid {int((key < 0).sum())}, "
          f"hi faces valid: {[verdict[f'hi_face_{a}'] for a in 'xyz']}")
    assert key.max() > HIGH
    return [("limit_voxel", pts, off, p)]


# ---- padding on a grid at the cell limit: coors + p and o * s pass 2^31 - 1 --------------------------------------------------
PAD_EDGE_GEOS = (geo((1, 1, 3), (1, 1, 2), (0, 0, 2)), geo((1, 1, 3), (1, 1, 3), (0, 0, 65535)), geo((1, 1, 2), (1, 1, 4), (0, 0, 3)))


@functools.lru_cache(maxsize=None)
def family_pad_edge():
    """G = (1, 1, 2^31 - 1) with padding: an input at the far end has coors + p above 2^31 - 1, and the last output sites have
    o * s above it.  The sites that only such a sum reaches must be there, and their windows must read the far cells."""
    G = (1, 1, INT_MAX)
    rng = np.random.default_rng(31)
    far = INT_MAX - 1 - np.array([0, 1, 2, 3, 5, 8, 65535, 65536, 131071])
    xs = np.unique(np.concatenate([far, [0, 1, 2, 3, 65534, 65535], rng.integers(0, INT_MAX, 150)]))

    def scene(x):
        return np.stack([np.zeros(len(x), np.int64), np.zeros(len(x), np.int64), x], -1)
    case = SpCase("pad_edge", *_join([scene(rng.permutation(xs)), scene(far)]), G, PAD_EDGE_GEOS, False)
    over = 0
    for gi, (_, K, s, p, _) in enumerate(case.geos):
        assert fits(G, case.geos[gi])
        oc, oo, nbr = reference(case, gi)
        c = np.asarray(case.coors, np.int64)[:, 2]
        # sites reached from an input with coors + p - k above 2^31 - 1, for every k that reaches them
        t = c[:, None] + p[2] - np.arange(K[2])[None, :]
        hit = (t % s[2] == 0) & (t // s[2] < ref.geometry(G, K, s, p)[4][2])
        reach_hi, reach_lo = np.unique((t // s[2])[hit & (t > INT_MAX)]), np.unique((t // s[2])[hit & (t <= INT_MAX)])
        only_hi = np.setdiff1d(reach_hi, reach_lo)
        assert np.isin(only_hi, oc[:, 2]).all()
        over += len(only_hi) + int((oc[:, 2].astype(np.int64) * s[2] > INT_MAX).any())
        assert len(only_hi) > 0, case.geos[gi][0]
    print(f"pad_edge coverage: {over} output sites that only a sum above 2^31 - 1 reaches or that start above it")
    return (case,)


def sp_families():
    """name -> builder of a tuple of SpCase."""
    return {"sweep": family_sweep, "limit": family_limit, "large": family_large, "many": family_many_sp, "rows": family_rows_sp,
            "probe": family_probe_sp, "pad_edge": family_pad_edge}


def voxel_families():
    return {"many": family_many_voxel, "rows": family_rows_voxel, "probe": family_probe_voxel, "limit": family_limit_voxel}
