"""CPU checks of the reference restatement of SPEC.md §22 (tests/spconv_pool_ref.py): the two forms of the pool agree with each
other and with torch's dense max_pool3d, the two forms of its backward agree with each other and with torch.autograd, the inverse
convolution agrees with conv_transpose3d, and the coverage the GPU suite relies on is reached.  No GPU."""
import numpy as np
import pytest

import spconv_cases as sc
import spconv_grad_ref as gref
import spconv_pool_ref as pref
import spconv_ref as ref
from sad_amd.spconv import SparseInverseConv3d, SparseMaxPool3d, SparseTensor

F = np.float32
STRIDED = pref.strided_geometries()
DUP_FREE = [n for n in sorted(sc.FAMILIES) if n != "duplicates"]


def test_strided_geometries_are_the_five_of_the_cases():
    assert [g[0] for g in STRIDED] == ["k333s2p1", "k333s2p011", "k311s211p0", "k222s2p0", "k133s1p011"]


@pytest.mark.parametrize("name", sorted(sc.FAMILIES))
def test_pool_forms_agree_every_family_and_geometry(name):
    coors, off, G = sc.FAMILIES[name][0]()
    sc.check_coverage(name, coors, off, G)
    for gi, (gname, K, s, p, subm) in enumerate(STRIDED):
        nbr = ref.index_vec(coors, off, G, K, s, p, subm)[2]
        for feat in (sc.make_feat(len(coors), 3, gi), pref.quantised_feat(len(coors), 2, gi)):
            a, b = pref.max_pool_loop(feat, nbr), pref.max_pool_vec(feat, nbr)
            assert np.array_equal(a[0].view(np.int32), b[0].view(np.int32)), f"{name}/{gname}: out differs between the two forms"
            assert np.array_equal(a[1], b[1]), f"{name}/{gname}: arg differs between the two forms"
            assert (a[1] >= 0).all()                             # a strided rulebook has no empty row


def test_pool_edge_rules_of_the_reference():
    feat = np.array([[0.0, -1.0], [-0.0, -3.0], [5.0, -2.0]], F)
    nbr = np.array([[1, 0, -1], [0, 1, 7], [-1, -1, -1], [2, 2, 0]], np.int32)          # 7 >= Nv counts as -1
    for form in (pref.max_pool_loop, pref.max_pool_vec):
        out, arg = form(feat, nbr)
        assert np.signbit(out[0, 0]) and not np.signbit(out[1, 0])                      # -0.0 / +0.0 are a tie: the first stays
        assert arg.tolist() == [[1, 0], [0, 0], [-1, -1], [2, 0]]
        assert out[2].tolist() == [0.0, 0.0] and out[0, 1] == -1.0 and out[3].tolist() == [5.0, -1.0]


@pytest.mark.parametrize("name", DUP_FREE)
def test_pool_equals_dense_max_pool3d(name):
    import torch
    coors, off, G = sc.FAMILIES[name][0]()
    assert not pref.has_duplicates(coors, off)
    feat = sc.make_feat(len(coors), 3, 4)
    x = torch.from_numpy(pref.dense_fill(feat, coors, off, G, -np.inf))
    for gname, K, s, p, subm in STRIDED:
        oc, oo, nbr = ref.index_vec(coors, off, G, K, s, p, subm)
        out, _ = pref.max_pool_vec(feat, nbr)
        y = torch.nn.functional.max_pool3d(x, K, s, p).numpy()
        assert y.shape[2:] == ref.geometry(G, K, s, p)[4]
        scn = ref.scene_ids(oo)
        want = y[scn, :, oc[:, 0], oc[:, 1], oc[:, 2]]
        assert (out == want).all(), f"{name}/{gname}: {int((out != want).sum())} values differ from max_pool3d"
        # every other site of the dense result is empty (-inf): the active set is the set of windows that hold a voxel
        active = np.zeros(y.shape[:1] + y.shape[2:], bool)
        active[scn, oc[:, 0], oc[:, 1], oc[:, 2]] = True
        assert np.isneginf(y.transpose(0, 2, 3, 4, 1)[~active]).all()


@pytest.mark.parametrize("name", DUP_FREE)
def test_inverse_conv_equals_conv_transpose3d(name, orc):
    coors, off, G = sc.FAMILIES[name][0]()
    for gi, (gname, K, s, p, subm) in enumerate(STRIDED):
        oc, oo, nbr = ref.index_vec(coors, off, G, K, s, p, subm)
        nbrT, col = gref.index_transpose_vec(nbr, len(coors))
        assert col == 0, f"{name}/{gname}: a strided rulebook never collides"
        cin, cout = ((4, 5), (3, 2), (1, 4))[gi % 3]
        W, b = sc.make_layer(nbr.shape[1], cin, cout, gi, bias=bool(gi & 1))
        feat = sc.make_feat(len(oc), cin, gi + 2)
        out = pref.inverse_conv(feat, nbrT, W, b)
        assert out.shape == (len(coors), cout)
        worst, opad = pref.inverse_conv_check(feat, oc, oo, G, K, s, p, W, b, out, coors, off)
        print(f"{name}/{gname}: worst err / bound = {worst:.3g}, output_padding {opad}")
        dead = (nbrT < 0).all(1)
        assert (out[dead] == (np.zeros(cout, F) if b is None else b)[None, :]).all()


@pytest.mark.parametrize("name", DUP_FREE)
def test_pool_backward_forms_agree_and_match_autograd(name):
    import torch
    coors, off, G = sc.FAMILIES[name][0]()
    Nv = len(coors)
    for gi, (gname, K, s, p, subm) in enumerate(STRIDED):
        oc, oo, nbr = ref.index_vec(coors, off, G, K, s, p, subm)
        nbrT, col = gref.index_transpose_vec(nbr, Nv)
        assert col == 0
        g = gref.lattice((len(nbr), 3), 4, gi)
        # integer features (ties everywhere), integer gradients: the in-order float32 sum equals the float64 scatter
        _, arg = pref.max_pool_vec(pref.quantised_feat(Nv, 3, gi), nbr)
        got = pref.max_pool_grad_loop(g, arg, nbrT)
        assert (got.astype(np.float64) == pref.max_pool_grad_scatter(g, arg, Nv)).all(), f"{name}/{gname}: loop and scatter forms differ"
        # float features: no window has a tie, and torch.autograd through the dense max_pool3d agrees
        feat = sc.make_feat(Nv, 3, gi + 7)
        out, arg = pref.max_pool_vec(feat, nbr)
        assert pref.pool_coverage(feat, nbr, Nv)["ties"] == 0
        x = torch.from_numpy(pref.dense_fill(feat, coors, off, G, -np.inf)).requires_grad_(True)
        y = torch.nn.functional.max_pool3d(x, K, s, p)
        scn = torch.from_numpy(ref.scene_ids(oo))
        toc = torch.from_numpy(oc.astype(np.int64))
        (y[scn, :, toc[:, 0], toc[:, 1], toc[:, 2]] * torch.from_numpy(g)).sum().backward()
        sci = ref.scene_ids(off)
        want = x.grad.numpy()[sci, :, coors[:, 0], coors[:, 1], coors[:, 2]]
        assert (pref.max_pool_grad_loop(g, arg, nbrT) == want).all(), f"{name}/{gname}: differs from torch.autograd"


def test_coverage_conditions_on_random030():
    """Conditions of the GPU suite, asserted on the reference before anything is compared (SPEC.md §22 test plan)."""
    coors, off, G = sc.FAMILIES["random030"][0]()
    assert G == (7, 9, 11)
    Nv = len(coors)
    feat = pref.quantised_feat(Nv, 4, 0)
    cov = {}
    for gname, K, s, p, subm in STRIDED:
        nbr = ref.index_vec(coors, off, G, K, s, p, subm)[2]
        cov[gname] = c = pref.pool_coverage(feat, nbr, Nv)
        print(gname, c)
        assert c["ties"] >= 1 and c["not_first"] >= 1 and c["collisions"] == 0, (gname, c)       # (a), (b)
        a, b = pref.max_pool_loop(feat, nbr), pref.max_pool_vec(feat, nbr)
        assert np.array_equal(a[0].view(np.int32), b[0].view(np.int32)) and np.array_equal(a[1], b[1])
        nbrT = gref.index_transpose_vec(nbr, Nv)[0]
        g = gref.lattice((len(nbr), 4), 4, 3)
        assert (pref.max_pool_grad_loop(g, a[1], nbrT).astype(np.float64) == pref.max_pool_grad_scatter(g, a[1], Nv)).all()
        neg = -np.abs(sc.make_feat(Nv, 4, 5)) - F(0.5)                                             # (c): absent is not zero
        assert (pref.max_pool_vec(neg, nbr)[0] < 0).all()
    assert cov["k222s2p0"]["uncovered"] >= 1                                                       # (d): the odd grid's last planes
    assert cov["k333s2p1"]["max_fanout"] >= 2                                                      # (e): more than one term in a sum
    assert cov["k222s2p0"]["max_fanout"] <= 1                                                      # windows that do not overlap


def test_host_side_argument_errors_of_the_pool_entry_points(sad):
    """Refusals that need no GPU: the library's usual codes before any launch (SAD_EINVAL = -1, SAD_EUNSUPPORTED = -2)."""
    from sad_amd import _lib
    L = _lib.lib()
    p = 0x10000                                                  # never dereferenced: every call fails on the host
    assert L.sad_spconv_max_pool_f32(p, p, 4, 4, 28, 4, p, p, None) == -2 and b"Kvol" in L.sad_last_error()
    assert L.sad_spconv_max_pool_f32(p, p, 4, 4, 0, 4, p, p, None) == -1
    assert L.sad_spconv_max_pool_f32(p, p, 4, 4, 8, 0, p, p, None) == -1
    assert L.sad_spconv_max_pool_f32(p, p, 4, -1, 8, 4, p, p, None) == -1
    assert L.sad_spconv_max_pool_f32(p, p, 1 << 24, 4, 8, 128, p, p, None) == -2 and b"2^31" in L.sad_last_error()
    assert L.sad_spconv_max_pool_f32(p, None, 4, 4, 8, 4, p, p, None) == -1 and b"NULL" in L.sad_last_error()
    assert L.sad_spconv_max_pool_grad_f32(p, p, p, 4, 4, 28, 4, p, None) == -2
    assert L.sad_spconv_max_pool_grad_f32(p, p, p, 4, 1 << 24, 8, 128, p, None) == -2
    assert L.sad_spconv_max_pool_grad_f32(p, None, p, 4, 4, 8, 4, p, None) == -1 and b"NULL" in L.sad_last_error()
    # nothing to do is not an error, and launches nothing
    assert L.sad_spconv_max_pool_f32(None, None, 0, 0, 8, 4, None, None, None) == 0
    assert L.sad_spconv_max_pool_grad_f32(None, None, None, 0, 0, 8, 4, None, None) == 0


def test_layers_construct_and_refuse_without_a_gpu(sad):
    import torch
    from sad_amd import autograd, ops
    pool = SparseMaxPool3d(2, indice_key="p")
    assert pool.kernel_size == pool.stride == (2, 2, 2) and pool.padding == (0, 0, 0) and not list(pool.parameters())
    assert SparseMaxPool3d((3, 1, 1), (2, 1, 1), 0).stride == (2, 1, 1)
    with pytest.raises(ValueError):
        SparseMaxPool3d(4)
    inv = SparseInverseConv3d(32, 16, 3, "down1")
    assert tuple(inv.weight.shape) == (27, 16, 32) and tuple(inv.bias.shape) == (16,) and "down1" in repr(inv)
    with pytest.raises(ValueError, match="indice_key"):
        SparseInverseConv3d(32, 16, 3, None)
    with pytest.raises(ValueError):
        SparseInverseConv3d(32, 257, 3, "k")
    assert sad.SparseMaxPool3d is SparseMaxPool3d and sad.SparseInverseConv3d is SparseInverseConv3d and sad.sparse_max_pool is ops.sparse_max_pool
    assert callable(autograd.sparse_max_pool)
    x = SparseTensor(torch.zeros((2, 4)), torch.zeros((2, 3), dtype=torch.int32), torch.tensor([0, 2], dtype=torch.int32), (4, 4, 4))
    assert x.rulebooks == {} and x.replace_feature(x.feat).rulebooks is x.rulebooks
    for gone in ("transposed", "sources"):
        with pytest.raises(TypeError):
            SparseTensor(x.feat, x.coors, x.offsets, (4, 4, 4), {}, **{gone: {}})
    with pytest.raises(ValueError, match="no rulebook"):
        SparseInverseConv3d(4, 4, 3, "k")(x)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.sparse_max_pool(x.feat, torch.zeros((1, 8), dtype=torch.int32))
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.sparse_max_pool_grad(x.feat, torch.zeros((2, 4), dtype=torch.int32), torch.zeros((2, 8), dtype=torch.int32), 2)
