"""Input families of the sparse-convolution tests (SPEC.md §21), shared by the CPU and the GPU suite.  Every family states the
coverage it must reach (``need``); ``check_coverage`` asserts it on the REFERENCE's rulebook before anything is compared."""
import numpy as np

import spconv_ref as ref
import voxel_ref

F = np.float32
TILES = (64, 128)          # output rows per workgroup of the convolution kernel (csrc/spconv.hip)

# (name, kernel, stride, padding, subm)
GEOMETRIES = [
    ("subm333", (3, 3, 3), (1, 1, 1), (1, 1, 1), True),
    ("subm111", (1, 1, 1), (1, 1, 1), (0, 0, 0), True),
    ("k333s2p1", (3, 3, 3), (2, 2, 2), (1, 1, 1), False),
    ("k333s2p011", (3, 3, 3), (2, 2, 2), (0, 1, 1), False),
    ("k311s211p0", (3, 1, 1), (2, 1, 1), (0, 0, 0), False),
    ("k222s2p0", (2, 2, 2), (2, 2, 2), (0, 0, 0), False),
    ("k133s1p011", (1, 3, 3), (1, 1, 1), (0, 1, 1), False),
]

# every Cin of {1,3,4,5,16,32,64,128,256} and every Cout of {1,10,16,32,64,128,200,256} at least once, and the SECOND ladder
CHANNEL_PAIRS = [(4, 16), (5, 16), (16, 16), (16, 32), (32, 32), (32, 64), (64, 64), (64, 128), (128, 128),
                 (1, 1), (3, 10), (256, 200), (128, 256), (256, 64)]
assert {a for a, _ in CHANNEL_PAIRS} == {1, 3, 4, 5, 16, 32, 64, 128, 256}
assert {b for _, b in CHANNEL_PAIRS} == {1, 10, 16, 32, 64, 128, 200, 256}


def _scene_cells(rng, G, n=None, density=None):
    cells = np.prod(G)
    if n is None:
        pick = np.flatnonzero(rng.random(cells) < density)
    else:
        pick = rng.choice(cells, n, replace=False)
    pick = rng.permutation(pick)
    return np.stack(np.unravel_index(pick, G), -1).astype(np.int32).reshape(-1, 3)


def _join(scenes):
    off = np.concatenate([[0], np.cumsum([len(s) for s in scenes])]).astype(np.int32)
    return np.ascontiguousarray(np.concatenate(scenes).astype(np.int32).reshape(-1, 3)), off


def family_random(density, seed=0, G=(7, 9, 11), B=3):
    rng = np.random.default_rng(100 + seed)
    return _join([_scene_cells(rng, G, density=density) for _ in range(B)]) + (G,)


def family_empty_scene():
    rng = np.random.default_rng(7)
    G = (6, 7, 8)
    return _join([_scene_cells(rng, G, density=0.2), np.zeros((0, 3), np.int32), _scene_cells(rng, G, density=0.4)]) + (G,)


def family_one_voxel():
    return np.array([[2, 3, 1]], np.int32), np.array([0, 1], np.int32), (5, 5, 5)


def family_faces():
    """Every cell on a face, edge or corner of the grid, and nothing inside; two scenes in different orders."""
    G = (5, 6, 7)
    z, y, x = np.meshgrid(*[np.arange(g) for g in G], indexing="ij")
    edge = (z == 0) | (z == G[0] - 1) | (y == 0) | (y == G[1] - 1) | (x == 0) | (x == G[2] - 1)
    c = np.stack([z[edge], y[edge], x[edge]], -1).astype(np.int32)
    rng = np.random.default_rng(3)
    return _join([c, c[rng.permutation(len(c))]]) + (G,)


def family_duplicates():
    """Rows repeated inside a scene (the lowest row owns the coordinate), and the same coordinates in another scene."""
    rng = np.random.default_rng(11)
    G = (6, 6, 9)
    a = _scene_cells(rng, G, density=0.25)
    a = np.concatenate([a, a[rng.integers(0, len(a), len(a) // 2)]])
    a = a[rng.permutation(len(a))]
    return _join([a, a[::-1].copy()]) + (G,)


def family_tile_edge(nv):
    """Nv one below, at or above a multiple of the row tile."""
    rng = np.random.default_rng(nv)
    G = (8, 10, 12)
    n0 = nv // 3
    return _join([_scene_cells(rng, G, n=n0), _scene_cells(rng, G, n=nv - n0)]) + (G,)


def family_synth():
    """Voxels of two ``synth`` scenes through the §20 reference, on a cropped range (the CPU reference stays in seconds)."""
    from sad_amd import synth
    pts = np.stack([synth.make_scene(s, 16384) for s in (0, 1)])
    v, r = (0.4, 0.4, 0.5), (10.0, -8.0, -3.0, 26.0, 8.0, 1.0)
    p, off = voxel_ref.ragged(pts)
    V = 4096
    _, coors, _, num = voxel_ref.voxel_index(p, off, v, r, V)
    G = voxel_ref.grid_size(v, r)
    c, o = _join([coors[b, :num[b]] for b in range(2)])
    return c, o, (int(G[2]), int(G[1]), int(G[0]))


# name -> (builder, coverage that must be seen on the (3,3,3) submanifold rulebook of the family)
FAMILIES = {
    "random002": (lambda: family_random(0.02, 0), {"centre_only", "skip_column"}),
    "random030": (lambda: family_random(0.3, 1), {"skip_free_tile"}),
    "random100": (lambda: family_random(1.0, 2), {"full_row", "skip_free_tile"}),
    "empty_scene": (family_empty_scene, {"empty_scene"}),
    "one_voxel": (family_one_voxel, {"centre_only", "skip_column"}),
    "faces": (family_faces, {"skip_free_tile"}),
    "duplicates": (family_duplicates, {"duplicates"}),
    "tile63": (lambda: family_tile_edge(63), set()),
    "tile64": (lambda: family_tile_edge(64), set()),
    "tile65": (lambda: family_tile_edge(65), set()),
    "tile127": (lambda: family_tile_edge(127), set()),
    "tile128": (lambda: family_tile_edge(128), set()),
    "tile129": (lambda: family_tile_edge(129), set()),
    "synth": (family_synth, {"centre_only", "skip_free_tile"}),
}


def coverage(coors, offsets, nbr_subm333):
    """What the (3,3,3) submanifold rulebook of a case exercises."""
    got = set()
    has = nbr_subm333 >= 0
    n = has.sum(1)
    if len(n) and (n == 1).any():
        got.add("centre_only")
    if len(n) and (n == 27).any():
        got.add("full_row")
    for T in TILES:
        for r0 in range(0, len(has), T):
            col = has[r0:r0 + T].any(0)
            got.add("skip_column" if not col.all() else "skip_free_tile")
    if (np.diff(offsets) == 0).any():
        got.add("empty_scene")
    sc = ref.scene_ids(offsets)
    keys = np.concatenate([sc[:, None], np.asarray(coors, np.int64)], 1)
    if len(np.unique(keys, axis=0)) < len(keys):
        got.add("duplicates")
    return got


def check_coverage(name, coors, offsets, G):
    need = FAMILIES[name][1]
    _, _, nbr = ref.index_vec(coors, offsets, G, (3, 3, 3), subm=True)
    got = coverage(coors, offsets, nbr)
    assert need <= got, f"family {name}: coverage {sorted(need - got)} not reached"
    if name.startswith("tile"):
        nv = int(name[4:])
        assert len(coors) == nv and any(nv % T in (0, 1, T - 1) for T in TILES)


def make_layer(Kvol, cin, cout, seed, bias=True):
    rng = np.random.default_rng(seed)
    a = (Kvol * cin) ** -0.5
    W = rng.uniform(-a, a, (Kvol, cout, cin)).astype(F)
    return W, (rng.uniform(-0.1, 0.1, cout).astype(F) if bias else None)


def make_feat(n, c, seed):
    return np.random.default_rng(seed).standard_normal((n, c)).astype(F)
