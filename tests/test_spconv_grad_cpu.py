"""CPU checks of SPEC.md §21.4 (backward of the sparse convolution): the reference restatement (tests/spconv_grad_ref.py) against
itself in two forms, against a hand-worked line, and against torch.nn.functional.conv3d double-precision autograd on the densified
input; the Python argument errors and the host-side refusals of the C-ABI (these need the built library, not a GPU)."""
import ctypes

import numpy as np
import pytest

import spconv_cases as sc
import spconv_grad_ref as gref
import spconv_ref as ref

F = np.float32


@pytest.mark.parametrize("name", sorted(sc.FAMILIES))
def test_index_transpose_two_forms_every_family_and_geometry(name):
    coors, off, G = sc.FAMILIES[name][0]()
    for gname, K, s, p, subm in sc.GEOMETRIES:
        nbr = ref.index_vec(coors, off, G, K, s, p, subm)[2]
        a, ca = gref.index_transpose_loop(nbr, len(coors))
        b, cb = gref.index_transpose_vec(nbr, len(coors))
        assert a.dtype == b.dtype == np.int32 and np.array_equal(a, b) and ca == cb, f"{name}/{gname}"
        assert (ca > 0) == (name == "duplicates" and subm), f"{name}/{gname}: {ca} collisions"
        if subm and name != "duplicates":
            assert np.array_equal(a, nbr[:, ::-1]), f"{name}/{gname}: a duplicate-free submanifold rulebook is its own mirror"
        # out-of-range entries count as -1
        if len(nbr):
            bad = nbr.copy()
            bad[0, 0] = len(coors) + 3
            cut = nbr.copy()
            cut[0, 0] = -1
            assert np.array_equal(gref.index_transpose_vec(bad, len(coors))[0], gref.index_transpose_vec(cut, len(coors))[0])


def test_hand_worked_line_stride_2(orc):
    """The line of test_spconv_cpu.test_hand_worked_line_stride_2: nbr = [[-1,0,-1],[1,2,-1],[-1,-1,1]] over 3 input rows.
    Entries: (o0,k1)->i0, (o1,k0)->i1, (o1,k1)->i2, (o2,k2)->i1, so nbrT = [[-1,0,-1],[1,-1,2],[-1,1,-1]], no collision.
    Cin = Cout = 1, W = (2,3,5), g = (1,10,100), feat = (7,11,13):
    grad_feat = (3*1, 2*10 + 5*100, 3*10) = (3, 520, 30); grad_W = (10*11, 1*7 + 10*13, 100*11) = (110, 137, 1100); grad_bias = 111."""
    coors = np.array([[0, 0, 4], [0, 0, 1], [0, 0, 2]], np.int32)
    nbr = ref.index_vec(coors, np.array([0, 3], np.int32), (1, 1, 6), (1, 1, 3), (1, 1, 2), (0, 0, 1))[2]
    for form in (gref.index_transpose_loop, gref.index_transpose_vec):
        nbrT, col = form(nbr, 3)
        assert nbrT.tolist() == [[-1, 0, -1], [1, -1, 2], [-1, 1, -1]] and col == 0
    W = np.array([2, 3, 5], F).reshape(3, 1, 1)
    g = np.array([[1], [10], [100]], F)
    feat = np.array([[7], [11], [13]], F)
    assert gref.grad_input(g, nbrT, W).reshape(-1).tolist() == [3.0, 520.0, 30.0]
    gw, mag, n, gb, magb = gref.grad_weight(feat, nbr, g)
    assert gw.reshape(-1).tolist() == [110.0, 137.0, 1100.0] and n.tolist() == [1, 2, 1] and gb.tolist() == [111.0]
    assert mag.reshape(-1).tolist() == [110.0, 137.0, 1100.0] and magb.tolist() == [111.0]


def test_hand_worked_collision():
    """test_spconv_cpu.test_hand_worked_duplicate_rule: rows 0 and 2 share a coordinate, nbr = [[-1,0,1],[0,1,-1],[-1,0,1]].
    Rows 0 and 2 have the same entries: row 2 loses both -> 2 collisions; nbrT = [[1,0,-1],[-1,1,0],[-1,-1,-1]]."""
    nbr = np.array([[-1, 0, 1], [0, 1, -1], [-1, 0, 1]], np.int32)
    for form in (gref.index_transpose_loop, gref.index_transpose_vec):
        nbrT, col = form(nbr, 3)
        assert nbrT.tolist() == [[1, 0, -1], [-1, 1, 0], [-1, -1, -1]] and col == 2
    gd = np.arange(4, dtype=F).reshape(1, 1, 1, 1, 4) + 1
    coors = np.array([[0, 0, 1], [0, 0, 2], [0, 0, 1]], np.int32)
    assert gref.to_dense_grad(gd, coors, np.array([0, 3], np.int32)).reshape(-1).tolist() == [2.0, 3.0, 0.0]


@pytest.mark.parametrize("name,gi", [("random030", 0), ("tile129", 2), ("faces", 4), ("empty_scene", 3)])
def test_reference_gradients_against_conv3d_autograd(orc, name, gi):
    """grad_W, grad_bias and grad_feat of the reference against float64 autograd through torch's dense conv3d (bias, residual and
    ReLU on; the ReLU mask is the reference's own, it is exact by definition): within 2 * gamma_n * sum |terms|, n = terms + 2."""
    import torch
    coors, off, G = sc.FAMILIES[name][0]()
    gname, K, s, p, subm = sc.GEOMETRIES[gi]
    G, K, s, p, O = ref.geometry(G, K, s, p, subm)
    oc, oo, nbr = ref.index_vec(coors, off, G, K, s, p, subm)
    Kvol, cin, cout = K[0] * K[1] * K[2], 5, 6
    W, b = sc.make_layer(Kvol, cin, cout, 3)
    feat, res, go = sc.make_feat(len(coors), cin, 4), sc.make_feat(len(oc), cout, 5), sc.make_feat(len(oc), cout, 6)
    out = ref.conv(feat, nbr, W, b, res, True)
    g = gref.relu_mask(go, out, True)
    assert (g == 0).any() and (g != 0).any()
    nbrT, col = gref.index_transpose_vec(nbr, len(coors))
    assert col == 0
    gf = gref.grad_input(g, nbrT, W)
    gw, mag, n, gb, magb = gref.grad_weight(feat, nbr, g)
    # torch, float64
    x = torch.from_numpy(ref.to_dense(feat, coors, off, G)).double().requires_grad_(True)
    w5 = torch.from_numpy(np.ascontiguousarray(W.reshape(K[0], K[1], K[2], cout, cin).transpose(3, 4, 0, 1, 2))).double().requires_grad_(True)
    tb = torch.from_numpy(b).double().requires_grad_(True)
    y = torch.nn.functional.conv3d(x, w5, tb, stride=s, padding=p)
    so, si = ref.scene_ids(oo), ref.scene_ids(off)
    ys = y[so, :, oc[:, 0], oc[:, 1], oc[:, 2]]
    (ys * torch.from_numpy(g).double()).sum().backward()
    want_w = w5.grad.numpy().transpose(2, 3, 4, 0, 1).reshape(Kvol, cout, cin)
    want_f = x.grad.numpy()[si, :, coors[:, 0], coors[:, 1], coors[:, 2]]
    worst = 0.0
    for got, want, m, terms in ((gw, want_w, mag, n.max()), (gb, tb.grad.numpy(), magb, len(oc)),
                                (gf.astype(np.float64), want_f, gref.grad_input_magnitude(g, nbrT, W), Kvol * cout)):
        bound = 2.0 * ref.gamma(int(terms) + 2) * m
        err = np.abs(got - want)
        assert (err <= bound).all(), f"{name}/{gname}: {int((err > bound).sum())} values outside the bound"
        worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
    print(f"{name}/{gname}: worst err / bound {worst:.3g}")


def test_python_argument_errors(sad):
    import torch
    from sad_amd import autograd, ops
    nbr = torch.zeros((4, 27), dtype=torch.int32)
    f = torch.zeros((4, 8))
    for call in (lambda: ops.sparse_conv_index_transpose(nbr, 4), lambda: ops.sparse_conv_grad_weight(f, nbr, f),
                 lambda: ops.sparse_conv_grad_input(f, nbr, torch.zeros((27, 8, 8)))):
        with pytest.raises(RuntimeError, match="no CPU path"):
            call()
    with pytest.raises(TypeError):
        ops.sparse_conv_index_transpose([[0]], 1)
    with pytest.raises(TypeError, match="no CPU path"):
        autograd.sparse_conv(f, torch.zeros((27, 8, 8)), None, None, nbr, False)
    import sad_amd
    for n in ("sparse_conv_index_transpose", "sparse_conv_grad_weight", "sparse_conv_grad_input"):
        assert getattr(sad_amd, n) is getattr(ops, n)


def test_abi_refusals_need_no_gpu(sad):
    """SAD_EINVAL / SAD_EUNSUPPORTED come back with a message before anything is launched."""
    from sad_amd import _lib
    L = _lib.lib()
    p = 0x10000                                               # never dereferenced: every call fails on the host
    n = ctypes.c_size_t(7)
    assert L.sad_spconv_index_transpose(None, 4, 4, 27, p, p, None) == -1 and b"NULL" in L.sad_last_error()
    assert L.sad_spconv_index_transpose(p, 4, 4, 27, p, None, None) == -1
    assert L.sad_spconv_index_transpose(p, -1, 4, 27, p, p, None) == -1
    assert L.sad_spconv_index_transpose(p, 4, 4, 28, p, p, None) == -2 and b"28" in L.sad_last_error()
    assert L.sad_spconv_index_transpose(p, 1 << 27, 4, 27, p, p, None) == -2 and b"2^31" in L.sad_last_error()
    assert L.sad_spconv_grad_weight_workspace_bytes(10, 27, 16, 16, None) == -1
    assert L.sad_spconv_grad_weight_workspace_bytes(10, 27, 257, 16, ctypes.byref(n)) == -2 and n.value == 0
    assert L.sad_spconv_grad_weight_workspace_bytes(10, 28, 16, 16, ctypes.byref(n)) == -2
    assert L.sad_spconv_grad_weight_workspace_bytes(10, 27, 256, 256, ctypes.byref(n)) == 0
    assert L.sad_spconv_grad_weight_f32(p, p, p, 4, 4, 27, 4, 4, None, None, None, None) == -1 and b"NULL" in L.sad_last_error()
    assert L.sad_spconv_grad_weight_f32(p, None, p, 4, 4, 27, 4, 4, p, None, None, None) == -1
    assert L.sad_spconv_grad_weight_f32(None, p, p, 4, 4, 27, 4, 4, p, None, None, None) == -1
    assert L.sad_spconv_grad_weight_f32(p, p, p, 4, 4, 27, 257, 4, p, None, None, None) == -2 and b"257" in L.sad_last_error()
    assert L.sad_spconv_grad_weight_f32(p, p, p, 4, 4, 27, 4, 257, p, None, None, None) == -2
    assert L.sad_spconv_grad_weight_f32(p, p, p, 4, 4, 28, 4, 4, p, None, None, None) == -2 and b"28" in L.sad_last_error()
    assert L.sad_spconv_grad_weight_f32(p, p, p, 4, 4, 0, 4, 4, p, None, None, None) == -1
    assert L.sad_spconv_grad_weight_f32(p, p, p, 4, 1 << 27, 27, 4, 4, p, None, None, None) == -2
    assert L.sad_spconv_grad_weight_f32(p, p, None, 4, 4, 27, 4, 4, None, p, None, None) == -1      # grad_bias alone still needs g
    assert L.sad_set_option(b"spconv_grad_ranges", 0) == 0
