"""Input families of the voxelization tests (SPEC.md §20) and the coverage each must reach, asserted on the REFERENCE's output
(tests/voxel_ref.py) so a changed generator cannot silently lose it.  Shared by test_voxel_cpu.py and test_gpu_voxel.py.

A case is (name, points [total,C] f32, offsets [B+1] int32, params) with params = dict(v, r, T, V)."""
import numpy as np

import voxel_ref as ref

F = np.float32

PILLARS = dict(v=(0.16, 0.16, 4), r=(0, -39.68, -3, 69.12, 39.68, 1), T=32, V=16000)
CAPPED = dict(v=(0.4, 0.4, 4), r=(0, -40, -3, 70.4, 40, 1), T=8, V=2000)
FINE = dict(v=(0.05, 0.05, 0.1), r=(0, -40, -3, 70.4, 40, 1), T=5, V=16000)
NUSC = dict(v=(0.2, 0.2, 8), r=(-51.2, -51.2, -5, 51.2, 51.2, 3), T=20, V=30000)


def with_channels(pts, C, seed=0):
    """[..., >=3] -> [..., C]: C = 3 keeps xyz, wider rows append seeded columns the index must not read."""
    xyz = np.asarray(pts, F)[..., :3]
    if C == 3:
        return np.ascontiguousarray(xyz)
    rng = np.random.default_rng(1000 + seed + C)
    extra = rng.standard_normal(xyz.shape[:-1] + (C - 3,)).astype(F)
    return np.ascontiguousarray(np.concatenate([xyz, extra], -1))


def kitti_scenes(C, sids=(0, 1)):
    from sad_amd import synth
    return with_channels(np.stack([synth.make_scene(s, 16384) for s in sids]), C)


def nuscenes_scene(C):
    from sad_amd import synth
    return with_channels(synth.make_nuscenes_batch(0, 1), C)


def dense_scenes(C):
    from sad_amd import synth
    return with_channels(synth.make_dense_batch(0, 2), C)


def stats(points, offsets, p):
    """What the coverage conditions are stated in, from the reference."""
    key, G = ref.keys_of(points, p["v"], p["r"])
    p2v, coors, count, voxel_num = ref.voxel_index(points, offsets, p["v"], p["r"], p["V"])
    B = len(offsets) - 1
    per_scene = []
    for b in range(B):
        o0, o1 = int(offsets[b]), int(offsets[b + 1])
        k, pv = key[o0:o1], p2v[o0:o1]
        dropped = np.flatnonzero((k >= 0) & (pv < 0))
        taken = np.flatnonzero(pv >= 0)
        per_scene.append(dict(
            n=o1 - o0, invalid=int((k < 0).sum()), voxel_num=int(voxel_num[b]), dropped=len(dropped),
            taken_after_drop=int((taken > dropped[0]).sum()) if len(dropped) else 0,
            t_overflow=int((count[b] > p["T"]).sum()), max_members=int(count[b].max()), max_key=int(k.max()) if len(k) else -1))
    return per_scene


def family_pillars(C=4):
    pts, off = ref.ragged(kitti_scenes(C))
    st = stats(pts, off, PILLARS)
    print("pillars:", st)
    for s in st:
        assert s["invalid"] >= 0.01 * s["n"] and s["voxel_num"] < PILLARS["V"] and s["dropped"] == 0 and s["max_members"] >= 2, s
    return [("pillars", pts, off, PILLARS)]


def family_capped(C=3):
    pts, off = ref.ragged(kitti_scenes(C))
    st = stats(pts, off, CAPPED)
    print("capped:", st)
    for s in st:
        assert s["voxel_num"] == CAPPED["V"] and s["t_overflow"] >= 1 and s["taken_after_drop"] >= 1, s
    return [("capped", pts, off, CAPPED)]


def family_fine(C=7):
    pts, off = ref.ragged(kitti_scenes(C))
    st = stats(pts, off, FINE)
    print("fine:", st)
    for s in st:
        assert s["max_key"] > 2 ** 24, s
    return [("fine", pts, off, FINE)]


def family_nuscenes(C=4):
    pts, off = ref.ragged(nuscenes_scene(C))
    st = stats(pts, off, NUSC)
    print("nuscenes:", st)
    assert pts.shape[0] == 65536
    return [("nuscenes", pts, off, NUSC)]


def family_dense(C=4):
    pts, off = ref.ragged(dense_scenes(C))
    st = stats(pts, off, CAPPED)
    print("dense:", st)
    for s in st:
        assert s["t_overflow"] >= 0.10 * s["voxel_num"] and s["voxel_num"] >= 1, s
    return [("dense", pts, off, CAPPED)]


def family_degenerate():
    """Lattice points on voxel faces with duplicates, one voxel holding every point, nothing in range, a ragged mix with an
    empty scene and wave-boundary sizes, V = 1."""
    rng = np.random.default_rng(20)
    cases = []
    lat = dict(v=(0.25, 0.25, 0.25), r=(-2, -2, -2, 2, 2, 2), T=4, V=3000)
    p = with_channels((rng.integers(-9, 10, (3000, 3)) * 0.25).astype(F), 4)       # -2.25 .. 2.25: faces, lo, hi and beyond
    p[100:200] = p[0:100]                                                       # duplicates
    off = np.array([0, 1700, 3000], np.int32)
    st = stats(p, off, lat)
    assert all(s["invalid"] >= 1 and s["max_members"] >= 2 for s in st), st
    assert (p[:, :3] == F(-2)).any() and (p[:, :3] == F(2)).any()
    cases.append(("lattice", p, off, lat))
    one = (rng.random((4096, 3)) * 0.3 + 0.05).astype(F)                         # all inside voxel (0,0,0) of a 0.4 grid
    box = (0, 0, 0, 4, 4, 0.4)
    for T in (1, 64):
        par = dict(v=(0.4, 0.4, 0.4), r=box, T=T, V=7)
        st = stats(with_channels(one, 3), np.array([0, 4096], np.int32), par)
        assert st[0]["max_members"] == 4096 and st[0]["voxel_num"] == 1
        cases.append((f"one_voxel_T{T}", with_channels(one, 3), np.array([0, 4096], np.int32), par))
    out = with_channels((rng.random((500, 3)) + 10).astype(F), 7)
    par = dict(v=(0.4, 0.4, 0.4), r=box, T=3, V=5)
    st = stats(out, np.array([0, 200, 500], np.int32), par)
    assert all(s["invalid"] == s["n"] and s["voxel_num"] == 0 for s in st)
    cases.append(("all_out_of_range", out, np.array([0, 200, 500], np.int32), par))
    from sad_amd import synth
    sizes = [0, 1, 63, 64, 65, 1000, 16384]
    sc = synth.make_scene(5, 16384)
    parts = [np.roll(sc, -7 * i, 0)[:n] for i, n in enumerate(sizes)]
    mix = with_channels(np.concatenate(parts), 4)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    st = stats(mix, off, CAPPED)
    assert [s["n"] for s in st] == sizes
    cases.append(("ragged_mix", mix, off, CAPPED))
    cases.append(("ragged_mix_pillars", mix, off, dict(PILLARS, V=600)))
    par = dict(CAPPED, V=1)
    st = stats(mix, off, par)
    assert st[-1]["voxel_num"] == 1 and st[-1]["dropped"] > 0
    cases.append(("V1", mix, off, par))
    return cases


FAMILIES = {"pillars": family_pillars, "capped": family_capped, "fine": family_fine, "nuscenes": family_nuscenes,
            "dense": family_dense, "degenerate": family_degenerate}
