"""GPU parity of the integer-only kernels (csrc/voxel.hip, the rulebook of csrc/spconv.hip, csrc/vox_hash.h) on the families of
tests/index_space_cases.py (-m gpu): geometries with stride above the kernel and padding above K // 2, grids up to 2^31 - 1
cells, up to 1000 scenes, more than 65,536 rows, hash probe runs that wrap past slot 0, denormal and huge finite coordinates.
Everything is EQUAL to the reference (np.array_equal, ``==`` for floats): no tolerance anywhere."""
import numpy as np
import pytest

import index_space_cases as ic
import spconv_cases as sc
import spconv_grad_ref as gref
import spconv_pool_ref as pref
import spconv_ref as ref
import voxel_ref

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:overflow encountered:RuntimeWarning")]

F = np.float32
MODES = ("sum", "mean", "max")


def _t(a, dev):
    import torch
    return torch.from_numpy(np.array(a, order="C")).to(dev)          # (a copy: the shared references are read-only)


def _eq_int(got, want, what):
    got = got.cpu().numpy()
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    assert np.array_equal(got, want), f"{what}: {int((got != want).sum())} of {want.size} entries differ"


def _eq_f(got, want, what):
    got = got.cpu().numpy()
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    bad = ~(got == want)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {want.size} values differ, first at {np.argwhere(bad)[0].tolist()}"


def _check_index(dev, case, gi, tc, to):
    """All three outputs of sparse_conv_index, both capacity forms of a strided geometry, and the transposed rulebook.
    -> (reference rulebook, reference nbrT)."""
    from sad_amd import ops
    gname, K, s, p, subm = case.geos[gi]
    w = f"{case.name}/{gname}"
    want = ic.reference(case, gi)
    oc, oo, nbr = want
    got = ops.sparse_conv_index(tc, to, case.G, K, s, p, subm)
    for g, x, n in zip(got, want, ("out_coors", "out_offsets", "nbr")):
        _eq_int(g, x, f"{w} {n}")
    if not subm:
        g2 = ops.sparse_conv_index(tc, to, case.G, K, s, p, False, capacity=len(oc) + 5)
        _eq_int(g2[1], oo, f"{w} out_offsets (capacity)")
        _eq_int(g2[0][:len(oc)], oc, f"{w} out_coors (capacity)")
        _eq_int(g2[2][:len(oc)], nbr, f"{w} nbr (capacity)")
        assert g2[0].shape[0] == len(oc) + 5 and bool((g2[0][len(oc):] == -1).all()) and bool((g2[2][len(oc):] == -1).all()), f"{w}: spare rows"
        if len(oc) > 3:
            g3 = ops.sparse_conv_index(tc, to, case.G, K, s, p, False, capacity=len(oc) - 3)
            _eq_int(g3[0], oc[:-3], f"{w} out_coors (short capacity)")
            _eq_int(g3[2], nbr[:-3], f"{w} nbr (short capacity)")
            _eq_int(g3[1], oo, f"{w} out_offsets (short capacity)")
    Nv = len(case.coors)
    nbrT, col = gref.index_transpose_vec(nbr, Nv)
    g_nbrT, g_col = ops.sparse_conv_index_transpose(_t(nbr, dev), Nv)
    _eq_int(g_nbrT, nbrT, f"{w} nbrT")
    assert int(g_col.item()) == col, f"{w}: collisions {int(g_col.item())}, reference {col}"
    return want, nbrT


def _check_values(dev, case, gi, want, nbrT):
    """Convolution, max pool with its gradient and the input gradient over the REFERENCE's rulebook (an index fault cannot hide
    behind a matching value).  No == 0 included: empty tensors of the right shape and dtype come back."""
    from sad_amd import ops
    gname, K = case.geos[gi][:2]
    w = f"{case.name}/{gname}"
    oc, oo, nbr = want
    Nv, No, Kvol = len(case.coors), len(oc), K[0] * K[1] * K[2]
    W, b = sc.make_layer(Kvol, 4, 16, gi)
    feat = sc.make_feat(Nv, 4, gi + 1)
    tn, tT, tw = _t(nbr, dev), _t(nbrT, dev), _t(W, dev)
    _eq_f(ops.sparse_conv(_t(feat, dev), tn, tw, _t(b, dev), None, True), ref.conv(feat, nbr, W, b, None, True), f"{w} sparse_conv 4->16")
    pf = pref.quantised_feat(Nv, 4, gi)
    w_out, w_arg = pref.max_pool_vec(pf, nbr)
    g_out, g_arg = ops.sparse_max_pool(_t(pf, dev), tn)
    _eq_f(g_out, w_out, f"{w} sparse_max_pool")
    _eq_int(g_arg, w_arg, f"{w} sparse_max_pool arg")
    go = sc.make_feat(No, 4, gi + 2)
    _eq_f(ops.sparse_max_pool_grad(_t(go, dev), _t(w_arg, dev), tT, Nv), ic.pool_grad_vec(go, w_arg, nbrT), f"{w} sparse_max_pool_grad")
    g = sc.make_feat(No, 16, gi + 3)
    _eq_f(ops.sparse_conv_grad_input(_t(g, dev), tT, tw), gref.grad_input(g, nbrT, W), f"{w} sparse_conv_grad_input")


def _run_sp_case(dev, case, values):
    tc, to = _t(case.coors, dev), _t(case.off, dev)
    for gi in range(len(case.geos)):
        want, nbrT = _check_index(dev, case, gi, tc, to)
        if values:
            _check_values(dev, case, gi, want, nbrT)


@pytest.mark.parametrize("k", range(3))
def test_sweep_rulebook_and_values(dev, orc, k):
    """13 written geometries and a third of the 40 drawn ones on one sweep input, the No == 0 rulebooks among them."""
    _run_sp_case(dev, ic.family_sweep()[k], True)


@pytest.mark.parametrize("k", range(len(ic.MANY)))
def test_many_scenes_rulebook_and_values(dev, orc, k):
    _run_sp_case(dev, ic.family_many_sp()[k], True)


def test_stride_and_padding_at_the_abi_limit(dev):
    _run_sp_case(dev, ic.family_limit()[0], False)


@pytest.mark.parametrize("k", range(len(ic.LARGE_GRIDS)))
def test_large_grid_rulebook(dev, k):
    _run_sp_case(dev, ic.family_large()[k], False)


def test_more_than_65536_candidates(dev):
    _run_sp_case(dev, ic.family_rows_sp()[0], False)


def test_padding_on_a_grid_at_the_cell_limit(dev):
    """coors + p and o * s above 2^31 - 1 (G = (1, 1, 2^31 - 1) with padding up to 65535)."""
    _run_sp_case(dev, ic.family_pad_edge()[0], False)


@pytest.mark.parametrize("k", range(2))
def test_probe_runs_that_wrap_rulebook(dev, k):
    _run_sp_case(dev, ic.family_probe_sp()[k], False)


def test_geometry_refusals_do_not_launch(dev):
    """What ops.sparse_conv_geometry refuses is refused before the workspace is made and before anything is launched."""
    import torch
    from sad_amd import ops
    case = ic.family_sweep()[1]
    tc, to = _t(case.coors, dev), _t(case.off, dev)
    torch.cuda.synchronize()
    with pytest.raises(ValueError, match="out_shape .* exceeds 2\\^31 - 1 cells"):
        ops.sparse_conv_index(tc, to, (1290, 1290, 1290), 3, 1, 2)
    for bad in (65536, (1, 65536, 1)):
        with pytest.raises(ValueError, match="above 65535"):
            ops.sparse_conv_index(tc, to, case.G, 1, bad, 0)
        with pytest.raises(ValueError, match="above 65535"):
            ops.sparse_conv_index(tc, to, case.G, 1, 1, bad)
        with pytest.raises(ValueError, match="above 65535"):
            ops.sparse_conv_index(tc, to, case.G, 1, 1, bad, capacity=10)
    torch.cuda.synchronize()                                                        # nothing faulted, nothing is pending
    got = ops.sparse_conv_index(tc, to, case.G, 3, 2, 1)                            # and the operator still works
    for g, x in zip(got, ref.index_vec(case.coors, case.off, case.G, (3, 3, 3), (2, 2, 2), (1, 1, 1))):
        _eq_int(g, x, "sparse_conv_index after the refused calls")


# ---- sparse_to_dense ------------------------------------------------------------------------------------------------------
def _dense_case(dev, case, gi, C=3):
    from sad_amd import ops
    gname, K, s, p, subm = case.geos[gi]
    oc, oo, _ = ic.reference(case, gi)
    O = ref.geometry(case.G, K, s, p, subm)[4]
    f = sc.make_feat(len(oc), C, gi)
    _eq_f(ops.sparse_to_dense(_t(f, dev), _t(oc, dev), _t(oo, dev), O), ref.to_dense(f, oc, oo, O), f"{case.name}/{gname} sparse_to_dense")


def test_sparse_to_dense_many_scenes(dev):
    case = ic.family_many_sp()[1]
    assert len(case.off) - 1 == 1000
    for gi in range(len(case.geos)):
        _dense_case(dev, case, gi)


def test_sparse_to_dense_kitti_strided_output(dev):
    case = ic.family_large()[0]
    gi = [g[0] for g in case.geos].index("k333s222p111")
    assert case.G == (41, 1600, 1408)
    _dense_case(dev, case, gi)


def test_sparse_to_dense_above_2_31_elements(dev):
    """B = 1, C = 17, O = (32, 2048, 2048): 2.28e9 output floats, checked on the device."""
    import torch
    from sad_amd import ops
    O, C = (32, 2048, 2048), 17
    assert C * O[0] * O[1] * O[2] > 2 ** 31
    free, total = torch.cuda.mem_get_info(dev)
    if free < 16 * 2 ** 30:
        pytest.skip(f"{free / 2 ** 30:.1f} GiB of {total / 2 ** 30:.1f} GiB free on the device, 16 GiB wanted (the output alone takes 9.1 GiB)")
    rng = np.random.default_rng(17)
    cells = np.unique(np.concatenate([np.stack([rng.integers(0, g, 180) for g in O], -1),
                                      [[0, 0, 0], [31, 2047, 2047], [31, 2047, 2046], [31, 0, 0], [16, 1024, 1024], [0, 2047, 2047]]]), axis=0)
    rows = np.concatenate([cells, cells[rng.integers(0, len(cells), 20)]])
    rows = rows[rng.permutation(len(rows))].astype(np.int32)
    feat = (rng.random((len(rows), C)) + 0.5).astype(F) * rng.choice([-1, 1], (len(rows), C)).astype(F)
    assert (feat != 0).all()
    _, lowest = np.unique(ic.linear(rows, O), return_index=True)
    assert len(lowest) == len(cells) < len(rows)
    dense = ops.sparse_to_dense(_t(feat, dev), _t(rows, dev), _t(np.array([0, len(rows)], np.int32), dev), O)
    assert tuple(dense.shape) == (1, C) + O and dense.dtype == torch.float32
    assert int(torch.count_nonzero(dense).item()) == len(cells) * C
    at = _t(rows[lowest].astype(np.int64), dev)
    got = dense[0][:, at[:, 0], at[:, 1], at[:, 2]].T.contiguous()
    _eq_f(got, feat[lowest], "sparse_to_dense above 2^31 elements: the lowest row of every cell")
    del dense
    torch.cuda.empty_cache()


# ---- voxel ----------------------------------------------------------------------------------------------------------------
def _check_voxel_case(dev, name, pts, off, p, reduce=False, dirty=False):
    from sad_amd import ops
    v, r, T, V = p["v"], p["r"], p["T"], p["V"]
    assert T <= 4
    tp, to = _t(pts, dev), _t(off, dev)
    ws = None
    if dirty:
        ws = ops.voxel_workspace(len(pts), len(off) - 1, V, dev)
        ws.fill_(0xA5)
    _eq_int(ops.voxel_coords(tp, to, v, r), voxel_ref.voxel_coords(pts, off, v, r), f"{name} voxel_coords")
    want_i = voxel_ref.voxel_index(pts, off, v, r, V)
    for g, x, n in zip(ops.voxel_index(tp, to, v, r, V, workspace=ws), want_i, ("point2voxel", "coors", "count", "voxel_num")):
        _eq_int(g, x, f"{name} voxel_index.{n}")
    for g, x, n in zip(ops.voxelize(tp, to, v, r, T, V, workspace=ws), voxel_ref.voxelize(pts, off, v, r, T, V),
                       ("voxels", "coors", "num_points", "voxel_num")):
        (_eq_f if n == "voxels" else _eq_int)(g, x, f"{name} voxelize.{n}")
    if reduce:
        p2v = want_i[0]                                # the reference's index: a numbering fault cannot hide behind the reduction
        tv = _t(p2v, dev)
        for mode in MODES:
            w_out, w_arg, w_cnt = voxel_ref.voxel_reduce(pts, p2v, off, V, mode)
            res = ops.voxel_reduce(tp, tv, to, V, mode, workspace=ws, return_count=True)
            _eq_f(res[0], w_out, f"{name} voxel_reduce({mode})")
            _eq_int(res[-1], w_cnt, f"{name} voxel_reduce({mode}).count")
            if mode == "max":
                _eq_int(res[1], w_arg, f"{name} voxel_reduce(max).arg")


@pytest.mark.parametrize("k", range(len(ic.MANY)))
def test_voxel_many_scenes(sad, dev, k):
    _check_voxel_case(dev, *ic.family_many_voxel()[k], reduce=True)


def test_voxel_more_than_65536_rows(sad, dev):
    _check_voxel_case(dev, *ic.family_rows_voxel()[0], reduce=True)


def test_voxel_probe_runs_that_wrap(sad, dev):
    """The cells of the probe family as voxel centres; the workspace (the hash table in it) is filled with 0xA5 first."""
    for case in ic.family_probe_voxel():
        _check_voxel_case(dev, *case, dirty=True)


def test_voxel_limit_grid(sad, dev):
    """1290^3 voxels; points on the faces, -0.0, one denormal either side of lo, the last float below hi, finite huge values."""
    _check_voxel_case(dev, *ic.family_limit_voxel()[0])


# ---- the numbering both share -----------------------------------------------------------------------------------------------
def test_voxel_and_rulebook_number_alike(sad, dev):
    """The two users of the first-appearance numbering (csrc/vox_hash.h) on one input: voxel_index over points at cell centres
    and the strided K = 1, s = 1, p = 0 rulebook over the cells give the same counts, the same coordinates in the same order
    and the lowest row of every voxel, and each equals its numpy reference.  Scenes of 0, 65, 64 and 129 rows: an empty scene,
    boundaries off and on a multiple of 64, a last partial wave."""
    from sad_amd import ops
    G = (6, 7, 8)                                                            # (z,y,x)
    sizes = (0, 65, 64, 129)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    N, B, V = int(off[-1]), len(sizes), int(off[-1])
    rng = np.random.default_rng(20)
    cells = np.stack([rng.integers(0, g, N) for g in G], -1).astype(np.int32)
    cells[128], cells[200] = cells[66], cells[130]                           # duplicates inside a scene, across a wave boundary
    pts = np.ascontiguousarray(cells[:, ::-1].astype(F) + F(0.5))            # (x,y,z) centres of a unit voxel grid
    v, r = (1.0, 1.0, 1.0), (0.0, 0.0, 0.0, float(G[2]), float(G[1]), float(G[0]))
    w_p2v, w_coors, w_count, w_num = voxel_ref.voxel_index(pts, off, v, r, V)
    w_oc, w_oo, w_nbr = ref.index_vec(cells, off, G, (1, 1, 1), (1, 1, 1), (0, 0, 0))
    # the input keeps what it is for
    assert any(w_num[b] < sizes[b] for b in range(B)), "no scene with fewer voxels than rows"
    assert any(sizes[b] > 0 and off[b] % 64 != 0 for b in range(B)), "no non-empty scene starts off a multiple of 64"
    assert (w_p2v >= 0).all() and w_nbr.shape == (len(w_oc), 1)

    tp, tc, to = _t(pts, dev), _t(cells, dev), _t(off, dev)
    g_vox = ops.voxel_index(tp, to, v, r, V)
    g_sp = ops.sparse_conv_index(tc, to, G, 1, 1, 0, False)
    for g, x, n in zip(g_vox, (w_p2v, w_coors, w_count, w_num), ("point2voxel", "coors", "count", "voxel_num")):
        _eq_int(g, x, f"voxel_index.{n}")
    for g, x, n in zip(g_sp, (w_oc, w_oo, w_nbr), ("out_coors", "out_offsets", "nbr")):
        _eq_int(g, x, f"sparse_conv_index.{n}")
    p2v, coors, _, num = (t.cpu().numpy() for t in g_vox)
    oc, oo, nbr = (t.cpu().numpy() for t in g_sp)
    assert np.array_equal(num, np.diff(oo)), "voxels per scene != output sites per scene"
    for b in range(B):
        assert np.array_equal(coors[b, :num[b]], oc[oo[b]:oo[b + 1]]), f"scene {b}: coordinates or their order differ"
        rows = np.arange(off[b], off[b + 1])
        lowest = np.array([rows[p2v[rows] == k].min() for k in range(num[b])], np.int32).reshape(-1)
        assert np.array_equal(nbr[oo[b]:oo[b + 1], 0], lowest), f"scene {b}: nbr[:, 0] is not the lowest row of each voxel"


# ---- modules ----------------------------------------------------------------------------------------------------------------
def test_sequential_of_sweep_geometries_layer_by_layer(dev, orc):
    import torch
    from sad_amd.spconv import SparseConv3d, SparseSequential, SparseTensor, SubMConv3d
    case = ic.family_sweep()[1]
    torch.manual_seed(1)
    net = SparseSequential(SubMConv3d(4, 16, (3, 1, 1), relu=True), SparseConv3d(16, 16, 2, 3, 0, relu=True),
                           SparseConv3d(16, 8, 3, 1, 2)).to(dev)
    feat = sc.make_feat(len(case.coors), 4, 5)
    x = SparseTensor(_t(feat, dev), _t(case.coors, dev), _t(case.off, dev), case.G)
    x0 = x
    f, c, o, g = feat, case.coors, case.off, case.G
    for li, m in enumerate(net):
        x = m(x)
        oc, oo, nbr = ref.index_loop(c, o, g, m.kernel_size, m.stride, m.padding, m.subm)
        f = ref.conv(f, nbr, m.weight.cpu().numpy(), m.bias.cpu().numpy(), None, m.relu)
        g = ref.geometry(g, m.kernel_size, m.stride, m.padding, m.subm)[4]
        c, o = oc, oo
        _eq_f(x.feat, f, f"layer {li} feat")
        _eq_int(x.coors, c, f"layer {li} coors")
        _eq_int(x.offsets, o, f"layer {li} offsets")
        assert x.spatial_shape == g
    assert len(c) > 0 and g == (4, 4, 5)
    _eq_f(net(x0).feat, f, "SparseSequential")
    _eq_f(x.dense(), ref.to_dense(f, c, o, g), "dense of the last layer")
