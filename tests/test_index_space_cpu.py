"""The families of tests/index_space_cases.py on the CPU: every coverage condition holds, the two forms of the rulebook reference
agree wherever both can run, the hash model of the probe family is self-consistent, and ops.sparse_conv_geometry is the host
arithmetic of SPEC.md §21 on every geometry and grid of the families, with the refusals of the library's sp_geo."""
import numpy as np
import pytest

import index_space_cases as ic
import spconv_pool_ref as pref
import spconv_ref as ref
import voxel_ref

F = np.float32

# (the huge finite coordinates of the voxel limit family divide to inf in the reference, as §20.1 has it)
pytestmark = pytest.mark.filterwarnings("ignore:overflow encountered:RuntimeWarning")


@pytest.mark.parametrize("family", sorted(ic.sp_families()))
def test_sparse_family_coverage_and_reference_forms(orc, family):
    """The builder asserts its coverage; index_loop == index_vec on every small grid; the key form agrees on every grid."""
    cases = ic.sp_families()[family]()
    assert len(cases) >= 1
    for case in cases:
        for gi, (gname, K, s, p, subm) in enumerate(case.geos):
            want = ic.reference(case, gi)
            if case.small:
                got = ref.index_vec(case.coors, case.off, case.G, K, s, p, subm)
                for g, x, n in zip(got, want, ("out_coors", "out_offsets", "nbr")):
                    assert g.shape == x.shape and g.dtype == x.dtype and np.array_equal(g, x), f"{case.name}/{gname}: {n} of the two forms differ"
            G = case.G
            assert np.array_equal(ic.nbr_by_key(case, gi, lambda z, y, x: (z * G[1] + y) * G[2] + x), want[2]), f"{case.name}/{gname}: key form"


def test_sweep_active_sites_third_form(orc):
    """The active output set of every strided sweep geometry a third way (a strided OR over the padded occupancy)."""
    for case in ic.family_sweep():
        for gi, (gname, K, s, p, subm) in enumerate(case.geos):
            if subm:
                continue
            oc, oo, _ = ic.reference(case, gi)
            O = ref.geometry(case.G, K, s, p)[4]
            for b in range(len(case.off) - 1):
                want = ref.active_sites(case.coors[case.off[b]:case.off[b + 1]], case.G, K, s, p)
                o = oc[oo[b]:oo[b + 1]].astype(np.int64)
                got = np.sort((o[:, 0] * O[1] + o[:, 1]) * O[2] + o[:, 2])
                assert np.array_equal(got, want), f"{case.name}/{gname} scene {b}"


@pytest.mark.parametrize("family", sorted(ic.voxel_families()))
def test_voxel_family_coverage_and_reference_forms(sad, family):
    for name, pts, off, p in ic.voxel_families()[family]():
        a = voxel_ref.voxel_index(pts, off, p["v"], p["r"], p["V"], "vec")
        if len(pts) <= 8000:
            b = voxel_ref.voxel_index(pts, off, p["v"], p["r"], p["V"], "loop")
            for x, y in zip(a, b):
                assert np.array_equal(x, y), f"{name}: the two numbering forms differ"
        assert (np.diff(off) >= 0).all() and off[-1] == len(pts)


def test_many_scenes_reach_the_second_trip_of_the_scene_loop():
    for B, sizes in ic.MANY.items():
        n = ic._many_check(B, sizes)
        assert len(n) == B and B > 16 and max(sizes) >= 16
    for case in ic.family_many_sp():
        assert len(case.off) - 1 in ic.MANY
    for (name, pts, off, p), B in zip(ic.family_many_voxel(), ic.MANY):
        assert len(off) == B + 1 and p["V"] <= 64


def test_hash_model_is_self_consistent():
    """hash_capacity and hash_slot0 of the model, and the probe run the family asserts, by an insert of the chosen keys."""
    assert [ic.hash_capacity(n) for n in (0, 1, 2, 3, 238, 256, 257)] == [(2, 63), (2, 63), (4, 62), (8, 61), (512, 55), (512, 55), (1024, 54)]
    keys = np.array([0, 1, (1 << 32) | 5, (65534 << 32) | (2 ** 31 - 2)], np.uint64)
    for shift in (63, 55, 40):
        assert ic.hash_slot0_vec(keys, shift).tolist() == [ic.hash_slot0(int(k), shift) for k in keys]
        assert all(0 <= ic.hash_slot0(int(k), shift) < 1 << (64 - shift) for k in keys)
    wrap, one = ic.family_probe_sp()
    cap, shift = ic.hash_capacity(len(wrap.coors))
    keys = [ic.hash_key(b, k) for b, k in zip(ref.scene_ids(wrap.off), ic.linear(wrap.coors, wrap.G))]
    slots, table = ic.probe_model(keys, cap, shift)
    # every key sits at or (circularly) after its home slot with no empty slot between, and equal keys share a slot
    for k, sl in zip(keys, slots):
        h = ic.hash_slot0(k, shift)
        assert table[sl] == k
        while h != sl:
            assert h in table and table[h] != k
            h = (h + 1) & (cap - 1)
    assert len(table) == len(set(keys)) < len(keys) <= cap // 2
    longest, wraps = ic.probe_runs(table, cap)
    assert longest == len(table) >= 64 and wraps and set(table) == {(cap - 3 + j) % cap for j in range(len(table))}
    # the same run whatever the order of the inserts (the kernel's order is that of its atomics)
    _, t2 = ic.probe_model(keys[::-1], cap, shift)
    assert set(t2) == set(table)
    assert ic.hash_capacity(len(one.coors)) == (2, 63)
    # the strided K = 1 form keys its second table by the same cells, in a table of the same size
    _, K, s, p, subm = wrap.geos[2]
    oc, oo, nbr = ic.reference(wrap, 2)
    assert not subm and ref.geometry(wrap.G, K, s, p)[4] == wrap.G and len(oc) == len(table)
    assert ic.probe_runs({0: 1, 1: 2, 7: 3}, 8) == (3, True) and ic.probe_runs({2: 1, 3: 2}, 8) == (2, False)


def test_pool_grad_vec_is_the_loop(orc):
    import spconv_grad_ref as gref
    case = ic.family_sweep()[0]
    for gi in (1, 5, 8):
        _, _, nbr = ic.reference(case, gi)
        Nv = len(case.coors)
        feat = pref.quantised_feat(Nv, 3, gi)
        out, arg = pref.max_pool_vec(feat, nbr)
        nbrT, _ = gref.index_transpose_vec(nbr, Nv)
        g = np.random.default_rng(gi).standard_normal(out.shape).astype(F)
        a, b = ic.pool_grad_vec(g, arg, nbrT), pref.max_pool_grad_loop(g, arg, nbrT)
        assert a.dtype == b.dtype and np.array_equal(a, b)


def _all_geometries():
    for build in ic.sp_families().values():
        for case in build():
            for g in case.geos:
                yield case.G, g


def test_sparse_conv_geometry_is_the_reference(sad):
    from sad_amd import ops
    n = 0
    for G, (gname, K, s, p, subm) in _all_geometries():
        got = ops.sparse_conv_geometry(G, K, s, p, subm) if not subm else ops.sparse_conv_geometry(G, K, subm=True)
        assert got == ref.geometry(G, K, s, p, subm), (G, gname)
        n += 1
    assert n >= 3 * len(ic.SWEEP_WRITTEN) + ic.N_DRAWN + 20


def test_sparse_conv_geometry_refuses_what_the_library_refuses(sad):
    from sad_amd import ops
    with pytest.raises(ValueError, match=r"out_shape \(1292, 1292, 1292\) exceeds 2\^31 - 1 cells"):
        ops.sparse_conv_geometry((1290, 1290, 1290), 3, 1, 2)
    for bad in (65536, (1, 1, 65536), (70000, 1, 1)):
        with pytest.raises(ValueError, match="above 65535"):
            ops.sparse_conv_geometry((5, 5, 5), 1, bad, 0)
        with pytest.raises(ValueError, match="above 65535"):
            ops.sparse_conv_geometry((5, 5, 5), 1, 1, bad)
    # the limits themselves are accepted, and the earlier refusals keep their order and their text
    assert ops.sparse_conv_geometry((1, 1, 200000), (1, 1, 3), (1, 1, 65535), (0, 0, 65535))[4] == (1, 1, 6)
    assert ops.sparse_conv_geometry((1290, 1290, 1290), 3, 1, 1)[4] == (1290, 1290, 1290)
    assert ops.sparse_conv_geometry((1, 1, 2 ** 31 - 1), 1)[4] == (1, 1, 2 ** 31 - 1)
    with pytest.raises(ValueError, match=r"spatial_shape \(1291, 1291, 1291\) exceeds 2\^31 - 1 cells"):
        ops.sparse_conv_geometry((1291, 1291, 1291), 3, 65536, 0)
    with pytest.raises(ValueError, match="sizes 1 .. 3 are implemented"):
        ops.sparse_conv_geometry((1291, 1291, 1291), 4, 65536, 0)
    with pytest.raises(ValueError, match="does not fit the padded grid"):
        ops.sparse_conv_geometry((1, 5, 5), 2, 1, 0)
    with pytest.raises(ValueError, match="above 65535"):
        ops.sparse_conv_geometry((1, 5, 5), 2, 65536, 0)


# The workspace sizes of the three entry points whose layout is carved from the coordinate table and the numbering arrays, as
# the library returned them before the table and the carving moved into one place each (read from a build of that commit).
# Callers allocate by these numbers and the kernels index by the same layout, so a change here is a change of the C-ABI.
# (total, B, V)
WS_VOXEL = [
    ((0, 1, 1), 144),
    ((1, 1, 1), 208),
    ((1, 3, 2000), 72176),
    ((1000, 1, 2000), 64704),
    ((1000, 3, 2000), 112720),
    ((65537, 1, 1), 4198576),
    ((65537, 3, 2000), 4270544),
]
# (total, B, V, Cin, Cout)
WS_ENCODE = [
    ((0, 1, 1, 4, 0), 176),
    ((1, 3, 1, 256, 4), 33168),
    ((1000, 3, 2000, 4, 64), 187040),
    ((1000, 1, 2000, 64, 0), 88720),
    ((65537, 1, 2000, 64, 256), 4313104),
    ((65537, 3, 1, 256, 256), 4461808),
]
# (Nv, B, kernel, stride, subm)
WS_SPCONV = [
    ((0, 1, (3, 3, 3), None, 1), 48),
    ((1000, 3, (3, 3, 3), None, 1), 24592),
    ((65537, 1, (3, 1, 1), None, 1), 3145744),
    ((0, 1, (3, 3, 3), (2, 2, 2), 0), 96),
    ((1, 3, (2, 2, 2), (2, 2, 2), 0), 96),
    ((1000, 3, (3, 3, 3), (2, 2, 2), 0), 222896),
    ((1000, 1, (3, 3, 3), (1, 1, 1), 0), 812720),
    ((65537, 3, (3, 1, 1), (1, 1, 1), 0), 9449504),
    ((65537, 1, (2, 2, 2), (1, 1, 1), 0), 28344352),
    ((65537, 3, (3, 3, 3), (2, 2, 2), 0), 28422176),
]


def test_workspace_sizes_are_pinned(sad):
    import ctypes
    from sad_amd import _lib
    L = _lib.lib()
    n = ctypes.c_size_t(0)
    i3 = lambda t: None if t is None else (ctypes.c_int * 3)(*t)
    for a, want in WS_VOXEL:
        assert L.sad_voxel_workspace_bytes(*a, ctypes.byref(n)) == 0 and n.value == want, (a, n.value, want)
    for a, want in WS_ENCODE:
        assert L.sad_voxel_encode_workspace_bytes(*a, ctypes.byref(n)) == 0 and n.value == want, (a, n.value, want)
    for (Nv, B, K, s, subm), want in WS_SPCONV:
        assert L.sad_spconv_workspace_bytes(Nv, B, i3(K), i3(s), subm, ctypes.byref(n)) == 0 and n.value == want, ((Nv, B, K, s, subm), n.value, want)
