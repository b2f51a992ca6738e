"""CPU tests of the sparse-convolution reference (SPEC.md §21, tests/spconv_ref.py) and of the Python layer's checks that need
no GPU: the two index forms agree on every family x geometry, hand-worked cases, density 1.0 against the dense convolution,
the conv3d cross-check with its derived bound, shape / argument errors."""
import numpy as np
import pytest

import spconv_cases as sc
import spconv_ref as ref

F = np.float32


@pytest.mark.parametrize("name", sorted(sc.FAMILIES))
def test_index_forms_agree_and_coverage(name):
    coors, off, G = sc.FAMILIES[name][0]()
    sc.check_coverage(name, coors, off, G)
    for gname, K, s, p, subm in sc.GEOMETRIES:
        a = ref.index_loop(coors, off, G, K, s, p, subm)
        b = ref.index_vec(coors, off, G, K, s, p, subm)
        for x, y, what in zip(a, b, ("out_coors", "out_offsets", "nbr")):
            assert x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x, y), f"{name}/{gname}: {what} differs between the forms"
        out_coors, out_off, nbr = a
        O = ref.geometry(G, K, s, p, subm)[4]
        assert out_off[0] == 0 and out_off[-1] == len(out_coors) and nbr.shape == (len(out_coors), K[0] * K[1] * K[2])
        if subm:
            assert np.array_equal(out_coors, coors) and np.array_equal(out_off, off)
            continue
        for bb in range(len(off) - 1):             # the active set, a third way
            o = out_coors[out_off[bb]:out_off[bb + 1]].astype(np.int64)
            lin = (o[:, 0] * O[1] + o[:, 1]) * O[2] + o[:, 2]
            assert len(np.unique(lin)) == len(lin), f"{name}/{gname}: an output site twice"
            assert np.array_equal(np.sort(lin), ref.active_sites(coors[off[bb]:off[bb + 1]], G, K, s, p)), f"{name}/{gname}: active set"
            assert (nbr[out_off[bb]:out_off[bb + 1]] >= 0).any(1).all(), f"{name}/{gname}: an output row without a neighbour"


def test_all_families_together_reach_every_coverage():
    got = set()
    for name, (build, _) in sc.FAMILIES.items():
        coors, off, G = build()
        got |= sc.coverage(coors, off, ref.index_vec(coors, off, G, (3, 3, 3), subm=True)[2])
    assert got >= {"centre_only", "full_row", "skip_column", "skip_free_tile", "empty_scene", "duplicates"}


def test_hand_worked_line_stride_2():
    """A line of voxels along x, kernel (1,1,3), stride (1,1,2), padding (0,0,1): x = 4, 1, 2 in this row order.
    Row 0 (x=4): kk=0 -> t=5 odd; kk=1 -> t=4 -> o=2; kk=2 -> t=3 odd.             sites so far: 2
    Row 1 (x=1): kk=0 -> t=2 -> o=1; kk=1 -> t=1 odd; kk=2 -> t=0 -> o=0.           sites: 2, 1, 0
    Row 2 (x=2): kk=0 -> t=3 odd; kk=1 -> t=2 -> o=1 (seen); kk=2 -> odd.           sites: 2, 1, 0
    nbr[o] reads x = 2 o - 1 + k:  o=2 -> x 3,4,5 -> (-1, 0, -1);  o=1 -> x 1,2,3 -> (1, 2, -1);  o=0 -> x -1,0,1 -> (-1, -1, 1)."""
    coors = np.array([[0, 0, 4], [0, 0, 1], [0, 0, 2]], np.int32)
    off = np.array([0, 3], np.int32)
    for form in (ref.index_loop, ref.index_vec):
        oc, oo, nbr = form(coors, off, (1, 1, 6), (1, 1, 3), (1, 1, 2), (0, 0, 1))
        assert oc.tolist() == [[0, 0, 2], [0, 0, 1], [0, 0, 0]]
        assert oo.tolist() == [0, 3]
        assert nbr.tolist() == [[-1, 0, -1], [1, 2, -1], [-1, -1, 1]]


def test_hand_worked_duplicate_rule():
    """Rows 0 and 2 share (0,0,1): row 0 owns it; row 2 is nobody's neighbour but keeps its own output row (submanifold form),
    whose centre reads the owner."""
    coors = np.array([[0, 0, 1], [0, 0, 2], [0, 0, 1]], np.int32)
    off = np.array([0, 3], np.int32)
    for form in (ref.index_loop, ref.index_vec):
        oc, oo, nbr = form(coors, off, (1, 1, 4), (1, 1, 3), subm=True)
        assert np.array_equal(oc, coors) and np.array_equal(oo, off)
        assert nbr.tolist() == [[-1, 0, 1], [0, 1, -1], [-1, 0, 1]]
    d = ref.to_dense(np.array([[1.0], [2.0], [3.0]], F), coors, off, (1, 1, 4))
    assert d.reshape(-1).tolist() == [0.0, 1.0, 2.0, 0.0]


def test_conv_definition_by_hand(orc):
    """Two rows, Kvol = 2, Cin = 2, Cout = 1: the fmaf chain written out."""
    import math
    feat = np.array([[0.1, 0.2], [0.3, 0.4]], F)
    nbr = np.array([[1, 0], [-1, 1]], np.int32)
    W = np.array([[[0.5, -0.25]], [[1.5, 0.75]]], F)
    b = np.array([0.125], F)
    res = np.array([[-1.0], [0.5]], F)

    def fma(a, x, acc):
        return F(math.fma(float(a), float(x), float(acc))) if hasattr(math, "fma") else F(np.float64(a) * np.float64(x) + np.float64(acc))
    a0 = b[0]
    for w, x in ((W[0, 0, 0], feat[1, 0]), (W[0, 0, 1], feat[1, 1]), (W[1, 0, 0], feat[0, 0]), (W[1, 0, 1], feat[0, 1])):
        a0 = fma(w, x, a0)
    a1 = b[0]
    for w, x in ((W[1, 0, 0], feat[1, 0]), (W[1, 0, 1], feat[1, 1])):
        a1 = fma(w, x, a1)
    out = ref.conv(feat, nbr, W, b)
    assert out[0, 0] == a0 and out[1, 0] == a1
    out = ref.conv(feat, nbr, W, b, residual=res, relu=True)
    assert out[0, 0] == max(F(a0 + res[0, 0]), F(0)) and out[1, 0] == max(F(a1 + res[1, 0]), F(0))


@pytest.mark.parametrize("gname,K,s,p,subm", sc.GEOMETRIES)
def test_full_density_is_the_dense_convolution(orc, gname, K, s, p, subm):
    """Every cell active: the output set is the whole output grid and the values are conv3d's within the derived bound."""
    coors, off, G = sc.family_random(1.0, 2, G=(4, 5, 6), B=2)
    s, p = ref.geometry(G, K, s, p, subm)[2:4]
    oc, oo, nbr = ref.index_vec(coors, off, G, K, s, p, subm)
    O = ref.geometry(G, K, s, p)[4]
    assert len(oc) == 2 * O[0] * O[1] * O[2]
    W, b = sc.make_layer(K[0] * K[1] * K[2], 5, 10, 1)
    feat = sc.make_feat(len(coors), 5, 2)
    out = ref.conv(feat, nbr, W, b)
    worst, inactive = ref.conv3d_check(feat, coors, off, G, K, s, p, W, b, out, oc, oo, subm)
    assert inactive == 0 and worst <= 1.0


@pytest.mark.parametrize("name", ["random002", "random030", "empty_scene", "faces", "synth"])
def test_conv3d_cross_check(orc, name):
    coors, off, G = sc.FAMILIES[name][0]()
    for gi, (gname, K, s, p, subm) in enumerate(sc.GEOMETRIES):
        cin, cout = sc.CHANNEL_PAIRS[gi % 4]
        oc, oo, nbr = ref.index_vec(coors, off, G, K, s, p, subm)
        W, b = sc.make_layer(K[0] * K[1] * K[2], cin, cout, gi, bias=gi % 2 == 0)
        feat = sc.make_feat(len(coors), cin, gi + 5)
        out = ref.conv(feat, nbr, W, b)
        worst, _ = ref.conv3d_check(feat, coors, off, G, K, s, p, W, b, out, oc, oo, subm)
        assert worst <= 1.0, (name, gname, worst)


def test_to_dense_and_from_voxels():
    coors, off, G = sc.family_random(0.3, 1)
    feat = sc.make_feat(len(coors), 3, 0)
    d = ref.to_dense(feat, coors, off, G)
    assert d.shape == (3, 3) + G and np.count_nonzero(d.any(1)) == len(coors)
    s = ref.scene_ids(off)
    assert np.array_equal(d[s, :, coors[:, 0], coors[:, 1], coors[:, 2]], feat)
    f3 = np.arange(2 * 4 * 2, dtype=F).reshape(2, 4, 2)
    c3 = np.arange(2 * 4 * 3, dtype=np.int32).reshape(2, 4, 3)
    f, c, o = ref.from_voxels(f3, c3, np.array([3, 1], np.int32))
    assert o.tolist() == [0, 3, 4] and np.array_equal(f, np.concatenate([f3[0, :3], f3[1, :1]])) and np.array_equal(c[3], c3[1, 0])


def test_python_layer_argument_errors(sad):
    """The checks of ops / spconv that run before any GPU work."""
    import torch
    from sad_amd import ops, spconv
    g = ops.sparse_conv_geometry
    assert g((41, 1600, 1408), 3, 2, 1) == ((41, 1600, 1408), (3, 3, 3), (2, 2, 2), (1, 1, 1), (21, 800, 704))
    assert g((21, 800, 704), (3, 1, 1), (2, 1, 1), 0)[4] == (10, 800, 704)
    assert g((5, 800, 704), 3, 2, (0, 1, 1))[4] == (2, 400, 352)
    assert g((7, 9, 11), 3, subm=True)[2:] == ((1, 1, 1), (1, 1, 1), (7, 9, 11))
    for bad in (dict(kernel=4), dict(kernel=0), dict(kernel=2, subm=True), dict(kernel=3, stride=2, subm=True), dict(kernel=3, stride=0),
                dict(kernel=3, padding=-1), dict(kernel=(3, 3)), dict(kernel=3, padding=(1, 1, 1), subm=False, spatial_shape=(1, 1, 0))):
        kw = dict(spatial_shape=(7, 9, 11), kernel=3)
        kw.update(bad)
        with pytest.raises(ValueError):
            g(**kw)
    with pytest.raises(ValueError):
        g((2, 9, 11), 3, 1, 0)                         # the kernel does not fit
    with pytest.raises(ValueError):
        g((1 << 11, 1 << 11, 1 << 11), 3)              # more than 2^31 - 1 cells
    cpu = torch.zeros((4, 3), dtype=torch.int32)
    with pytest.raises(RuntimeError):
        ops.sparse_conv_index(cpu, torch.zeros((2,), dtype=torch.int32), (7, 9, 11), 3, subm=True)
    with pytest.raises(RuntimeError):
        ops.sparse_conv(torch.zeros((4, 3)), torch.zeros((4, 27), dtype=torch.int32), torch.zeros((27, 8, 3)))
    with pytest.raises(RuntimeError):
        ops.sparse_to_dense(torch.zeros((4, 3)), cpu, torch.zeros((2,), dtype=torch.int32), (7, 9, 11))
    with pytest.raises(ValueError):
        spconv.SparseTensor(torch.zeros((4, 3)), torch.zeros((5, 3), dtype=torch.int32), torch.zeros((2,), dtype=torch.int32), (7, 9, 11))
    with pytest.raises(ValueError):
        spconv.SparseTensor(torch.zeros((4, 3)), cpu, torch.zeros((2,), dtype=torch.int32), (7, 9))
    with pytest.raises(ValueError):
        spconv.SubMConv3d(4, 16, kernel_size=2)
    with pytest.raises(ValueError):
        spconv.SparseConv3d(4, 300, 3, 2, 1)
    m = spconv.SparseConv3d(4, 16, 3, 2, (0, 1, 1), indice_key="down1")
    assert m.weight.shape == (27, 16, 4) and m.stride == (2, 2, 2) and m.padding == (0, 1, 1)
    w = torch.arange(2 * 3 * 1 * 3 * 3, dtype=torch.float32).reshape(2, 3, 1, 3, 3)
    k = spconv.SubMConv3d.from_conv3d_weight(w)
    assert k.shape == (9, 2, 3) and k[5, 1, 2] == w[1, 2, 0, 1, 2]
    for name in ("sparse_conv_index", "sparse_conv", "sparse_to_dense", "SparseTensor", "SubMConv3d", "SparseConv3d", "SparseSequential"):
        assert getattr(sad, name) is not None
