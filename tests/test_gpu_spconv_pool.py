"""GPU parity of SPEC.md §22 (-m gpu) against tests/spconv_pool_ref.py: sparse max pool and its backward (``==``, ``out`` by bit
pattern, bit-equal from call to call), the inverse convolution (``==`` ``spconv_ref.conv`` over the transposed rulebook; its weight
gradients by the rules of §21.4), the pairing of an inverse layer with its partner through ``indice_key``, and a two-level sparse
U-Net end to end.  Families, geometries and channel pairs: tests/spconv_cases.py; the coverage the cases must reach is asserted on
the reference first (tests/test_spconv_pool_cpu.py holds the same conditions without a GPU)."""
import numpy as np
import pytest

import spconv_cases as sc
import spconv_grad_ref as gref
import spconv_pool_ref as pref
import spconv_ref as ref

pytestmark = pytest.mark.gpu

F = np.float32
CHANNELS = (1, 3, 4, 5, 16, 64, 128, 200, 256, 320)
STRIDED = pref.strided_geometries()


def _t(a, dev, grad=False):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return t.requires_grad_(True) if grad else t


def _eq_int(got, want, what):
    got = got.cpu().numpy()
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    assert np.array_equal(got, want), f"{what}: {int((got != want).sum())} of {want.size} entries differ"


def _eq_bits(got, want, what):
    got = got.detach().cpu().numpy()
    assert got.shape == want.shape and got.dtype == want.dtype == F, (what, got.shape, want.shape, got.dtype, want.dtype)
    bad = got.view(np.int32) != want.view(np.int32)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {want.size} values differ in their bits, first at {np.argwhere(bad)[0].tolist()}"


def _eq_f(got, want, what):
    got = got.detach().cpu().numpy()
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    bad = ~(got == want)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {want.size} values differ, first at {np.argwhere(bad)[0].tolist()}"


def _eq_exact_sum(got, want64, what):
    got = got.detach().cpu().numpy()
    assert got.shape == want64.shape and got.dtype == F, (what, got.shape, want64.shape, got.dtype)
    bad = ~(got.astype(np.float64) == want64)
    assert not bad.any(), f"{what} (lattice): {int(bad.sum())} of {want64.size} values differ, first at {np.argwhere(bad)[0].tolist()}"


def _within(got, want64, mag, n, what):
    """The §21.4 rule: |gpu - ref64| <= n * 2^-23 * sum |terms| per element."""
    got = got.detach().cpu().numpy()
    assert got.shape == want64.shape and got.dtype == F, (what, got.shape, want64.shape, got.dtype)
    bound = gref.grad_weight_bound(mag, n)
    err = np.abs(got.astype(np.float64) - want64)
    worst = float((err / np.maximum(bound, 1e-300)).max()) if err.size else 0.0
    print(f"{what}: worst err / bound = {worst:.4g}")
    assert (err <= bound).all(), f"{what}: {int((err > bound).sum())} of {err.size} values outside n * 2^-23 * sum|terms|, worst {worst:.4g} x"


def _mixed_feat(n, c, seed):
    """Even channels: integers in [-2, 2] (ties inside every window); odd channels: normal floats."""
    f = sc.make_feat(n, c, seed)
    f[:, ::2] = pref.quantised_feat(n, c, seed)[:, ::2]
    return f


# ---- max pool and its backward ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(sc.FAMILIES))
def test_max_pool_and_grad_every_family_geometry_and_width(dev, name):
    """Every geometry of the cases (the submanifold ones as a caller's nbr) x every channel count: channels are independent, so the
    reference is computed once at the largest width and sliced."""
    from sad_amd import ops
    coors, off, G = sc.FAMILIES[name][0]()
    sc.check_coverage(name, coors, off, G)
    Nv, cmax = len(coors), max(CHANNELS)
    feat = _mixed_feat(Nv, cmax, 1)
    for gi, (gname, K, s, p, subm) in enumerate(sc.GEOMETRIES):
        nbr = ref.index_vec(coors, off, G, K, s, p, subm)[2]
        nbrT, _ = gref.index_transpose_vec(nbr, Nv)
        want_out, want_arg = pref.max_pool_vec(feat, nbr)
        g = sc.make_feat(len(nbr), cmax, gi + 3)
        g[::5] = 0
        want_grad = pref.max_pool_grad_loop(g, want_arg, nbrT)
        tn, tnT = _t(nbr, dev), _t(nbrT, dev)
        for C in CHANNELS:
            w = f"{name}/{gname} C={C}"
            out, arg = ops.sparse_max_pool(_t(feat[:, :C], dev), tn)
            _eq_bits(out, np.ascontiguousarray(want_out[:, :C]), f"{w} out")
            _eq_int(arg, np.ascontiguousarray(want_arg[:, :C]), f"{w} arg")
            tg = _t(g[:, :C], dev)
            g1 = ops.sparse_max_pool_grad(tg, arg, tnT, Nv)
            g2 = ops.sparse_max_pool_grad(tg, arg, tnT, Nv)
            _eq_bits(g1, np.ascontiguousarray(want_grad[:, :C]), f"{w} grad_feat")
            _eq_bits(g2, g1.cpu().numpy(), f"{w} grad_feat, second call")


def test_max_pool_coverage_cases_on_random030(dev):
    """The conditions of the issue, asserted on the reference before anything is compared: ties, an arg that is not the first
    valid neighbour, all-negative features, uncovered input rows, an input row that is the arg of several outputs."""
    from sad_amd import ops
    coors, off, G = sc.FAMILIES["random030"][0]()
    Nv = len(coors)
    feat = pref.quantised_feat(Nv, 4, 0)
    neg = -np.abs(sc.make_feat(Nv, 4, 5)) - F(0.5)
    cov = {}
    for gname, K, s, p, subm in STRIDED:
        nbr = ref.index_vec(coors, off, G, K, s, p, subm)[2]
        nbrT, col = gref.index_transpose_vec(nbr, Nv)
        cov[gname] = c = pref.pool_coverage(feat, nbr, Nv)
        assert c["ties"] >= 1 and c["not_first"] >= 1 and col == 0, (gname, c)
        want_out, want_arg = pref.max_pool_loop(feat, nbr)
        out, arg = ops.sparse_max_pool(_t(feat, dev), _t(nbr, dev))
        _eq_bits(out, want_out, f"{gname} out (ties)")
        _eq_int(arg, want_arg, f"{gname} arg (ties)")
        g = gref.lattice((len(nbr), 4), 4, 3)
        got = ops.sparse_max_pool_grad(_t(g, dev), arg, _t(nbrT, dev), Nv)
        _eq_bits(got, pref.max_pool_grad_loop(g, want_arg, nbrT), f"{gname} grad_feat (ties)")
        _eq_exact_sum(got, pref.max_pool_grad_scatter(g, want_arg, Nv), f"{gname} grad_feat against the scatter form")
        want_neg = pref.max_pool_loop(neg, nbr)
        assert (want_neg[0] < 0).all()
        out, arg = ops.sparse_max_pool(_t(neg, dev), _t(nbr, dev))
        _eq_bits(out, want_neg[0], f"{gname} out (all negative)")
        _eq_int(arg, want_neg[1], f"{gname} arg (all negative)")
    assert cov["k222s2p0"]["uncovered"] >= 1 and cov["k333s2p1"]["max_fanout"] >= 2 and cov["k222s2p0"]["max_fanout"] <= 1


def test_max_pool_signed_zero_empty_rows_and_out_of_range_entries(dev):
    import torch
    from sad_amd import ops
    feat = np.array([[0.0, -1.0, -0.0, 2.0], [-0.0, -3.0, 0.0, 2.0], [5.0, -2.0, -7.0, 1.0]], F)
    nbr = np.array([[1, 0, -1], [0, 1, 7], [-1, -1, -1], [2, 2, 0], [3, -5, 2 ** 31 - 1], [-1, 2, 1]], np.int32)   # 3, 7, ... >= Nv count as -1
    want_out, want_arg = pref.max_pool_loop(feat, nbr)
    assert np.signbit(want_out[0, 0]) and not np.signbit(want_out[1, 0]) and not np.signbit(want_out[0, 2])
    assert want_arg[2].tolist() == [-1] * 4 and want_arg[4].tolist() == [-1] * 4 and want_out[0, 1] == -1.0
    for C in (4, 3, 1):                                          # the 16-byte form and the scalar one
        out, arg = ops.sparse_max_pool(_t(feat[:, :C], dev), _t(nbr, dev))
        _eq_bits(out, np.ascontiguousarray(want_out[:, :C]), f"edge rules C={C} out")
        _eq_int(arg, np.ascontiguousarray(want_arg[:, :C]), f"edge rules C={C} arg")
        # backward over a hand-made nbrT with entries outside [0, No) and an arg of -1
        nbrT, _ = gref.index_transpose_vec(nbr, 3)
        bad = nbrT.copy()
        bad[bad < 0] = 6 + 11
        g = sc.make_feat(len(nbr), C, 2)
        want = pref.max_pool_grad_loop(g, want_arg[:, :C], nbrT)
        _eq_bits(ops.sparse_max_pool_grad(_t(g, dev), arg, _t(bad, dev), 3), want, f"edge rules C={C} grad_feat")
    # a sum without a term is +0.0, whatever the gradients are
    z = ops.sparse_max_pool_grad(_t(-np.ones((6, 4), F), dev), torch.full((6, 4), -1, dtype=torch.int32, device=dev), _t(nbrT, dev), 3)
    assert not bool(z.view(torch.int32).any())
    # empty sides
    out, arg = ops.sparse_max_pool(torch.zeros((0, 4), device=dev), torch.full((5, 8), -1, dtype=torch.int32, device=dev))
    assert tuple(out.shape) == (5, 4) and not bool(out.view(torch.int32).any()) and bool((arg == -1).all())
    out, arg = ops.sparse_max_pool(torch.ones((5, 4), device=dev), torch.zeros((0, 8), dtype=torch.int32, device=dev))
    assert tuple(out.shape) == (0, 4) and tuple(arg.shape) == (0, 4)
    gz = ops.sparse_max_pool_grad(torch.zeros((0, 4), device=dev), torch.zeros((0, 4), dtype=torch.int32, device=dev),
                                  torch.full((5, 8), -1, dtype=torch.int32, device=dev), 5)
    assert tuple(gz.shape) == (5, 4) and not bool(gz.view(torch.int32).any())
    gz = ops.sparse_max_pool_grad(torch.ones((5, 4), device=dev), torch.zeros((5, 4), dtype=torch.int32, device=dev),
                                  torch.zeros((0, 8), dtype=torch.int32, device=dev), 0)
    assert tuple(gz.shape) == (0, 4)


def test_max_pool_argument_errors(dev):
    import torch
    from sad_amd import _lib, ops
    L = _lib.lib()
    p = 0x10000                                                  # never dereferenced: every call below fails on the host
    assert L.sad_spconv_max_pool_f32(p, p, 4, 4, 28, 4, p, p, None) == -2 and b"Kvol" in L.sad_last_error()
    assert L.sad_spconv_max_pool_f32(p, p, 4, 4, 0, 4, p, p, None) == -1
    assert L.sad_spconv_max_pool_f32(p, p, 4, 4, 8, 0, p, p, None) == -1
    assert L.sad_spconv_max_pool_f32(p, p, -1, 4, 8, 4, p, p, None) == -1
    assert L.sad_spconv_max_pool_f32(p, p, 1 << 24, 4, 8, 128, p, p, None) == -2 and b"2^31" in L.sad_last_error()
    assert L.sad_spconv_max_pool_f32(None, p, 4, 4, 8, 4, p, p, None) == -1 and b"NULL" in L.sad_last_error()
    assert L.sad_spconv_max_pool_grad_f32(p, p, p, 4, 4, 28, 4, p, None) == -2
    assert L.sad_spconv_max_pool_grad_f32(p, p, p, 4, 1 << 24, 8, 128, p, None) == -2
    assert L.sad_spconv_max_pool_grad_f32(p, p, p, 4, 4, 8, 4, None, None) == -1 and b"NULL" in L.sad_last_error()
    feat, nbr = torch.zeros((4, 4), device=dev), torch.zeros((3, 8), dtype=torch.int32, device=dev)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.sparse_max_pool(feat.cpu(), nbr)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.sparse_max_pool_grad(torch.zeros((3, 4)), torch.zeros((3, 4), dtype=torch.int32, device=dev), nbr, 3)
    with pytest.raises(TypeError):
        ops.sparse_max_pool(feat.double(), nbr)
    with pytest.raises(TypeError):
        ops.sparse_max_pool(feat, nbr.long())
    with pytest.raises(ValueError):
        ops.sparse_max_pool(feat, torch.zeros((3, 28), dtype=torch.int32, device=dev))
    with pytest.raises(ValueError):
        ops.sparse_max_pool_grad(torch.zeros((3, 4), device=dev), torch.zeros((3, 5), dtype=torch.int32, device=dev), nbr, 3)
    with pytest.raises(ValueError):
        ops.sparse_max_pool_grad(torch.zeros((3, 4), device=dev), torch.zeros((3, 4), dtype=torch.int32, device=dev), nbr, 4)
    # a strided view is made contiguous, not misread
    wide = torch.arange(32, dtype=torch.float32, device=dev).view(4, 8)
    out, arg = ops.sparse_max_pool(wide[:, ::2], torch.tensor([[0, 3, -1]], dtype=torch.int32, device=dev))
    assert out.tolist() == [[24.0, 26.0, 28.0, 30.0]] and arg.tolist() == [[3] * 4]


def test_collisions_refuse_backward_not_forward(dev):
    from sad_amd import autograd
    coors, off, G = sc.FAMILIES["duplicates"][0]()
    nbr = ref.index_vec(coors, off, G, (3, 3, 3), subm=True)[2]
    assert gref.index_transpose_vec(nbr, len(coors))[1] > 0
    feat = sc.make_feat(len(coors), 4, 0)
    tf = _t(feat, dev, True)
    out = autograd.sparse_max_pool(tf, _t(nbr, dev))
    _eq_bits(out, pref.max_pool_vec(feat, nbr)[0], "forward on duplicates")
    with pytest.raises(ValueError, match="duplicate coordinate"):
        out.sum().backward()
    # the strided rulebook of the same input never collides: the layer trains
    from sad_amd.spconv import SparseMaxPool3d, SparseTensor
    x = SparseTensor(_t(feat, dev, True), _t(coors, dev), _t(off, dev), G)
    y = SparseMaxPool3d(3, 2, 1, indice_key="p")(x)
    go = sc.make_feat(y.feat.shape[0], 4, 1)
    y.feat.backward(_t(go, dev))
    nbr = ref.index_vec(coors, off, G, (3, 3, 3), (2, 2, 2), (1, 1, 1))[2]
    nbrT, col = gref.index_transpose_vec(nbr, len(coors))
    assert col == 0 and x.rulebooks["p"].collisions == 0
    _eq_bits(x.feat.grad, pref.max_pool_grad_loop(go, pref.max_pool_vec(feat, nbr)[1], nbrT), "layer backward on duplicates (strided)")


# ---- inverse convolution ---------------------------------------------------------------------------------------------
def _check_inverse(dev, coors, off, G, geo, cin, cout, seed, use_b, use_r, relu, what, lattice=False):
    """Operator and autograd on one case: forward ``==``, uncovered rows = bias (+ residual), grad_feat ``==``, grad_W / grad_bias by §21.4."""
    from sad_amd import autograd, ops
    gname, K, s, p, subm = geo
    oc, oo, nbr = ref.index_vec(coors, off, G, K, s, p, subm)
    Nv, No = len(coors), len(oc)
    nbrT, col = gref.index_transpose_vec(nbr, Nv)
    assert col == 0
    W, b = sc.make_layer(nbr.shape[1], cin, cout, seed)
    if lattice:
        W, b = gref.lattice(W.shape, 2, seed), gref.lattice(b.shape, 2, seed + 1)
        feat, res, go = gref.lattice((No, cin), 8, seed + 2), gref.lattice((Nv, cout), 4, seed + 3), gref.lattice((Nv, cout), 4, seed + 4)
    else:
        feat, res, go = sc.make_feat(No, cin, seed + 2), sc.make_feat(Nv, cout, seed + 3), sc.make_feat(Nv, cout, seed + 4)
    b_, r_ = (b if use_b else None), (res if use_r else None)
    want = pref.inverse_conv(feat, nbrT, W, b_, r_, relu)
    tnT, tn = _t(nbrT, dev), _t(nbr, dev)
    got = ops.sparse_conv(_t(feat, dev), tnT, _t(W, dev), _t(b, dev) if use_b else None, _t(res, dev) if use_r else None, relu)
    _eq_f(got, want, f"{what} forward")
    dead = (nbrT < 0).all(1)
    if dead.any():
        alone = (np.zeros(cout, F) if b_ is None else b_)[None, :] + (0 if r_ is None else r_[dead])
        alone = np.where(alone > 0, alone, 0).astype(F) if relu else alone.astype(F)
        _eq_f(got[_t(dead, dev)], np.broadcast_to(alone, (int(dead.sum()), cout)).astype(F), f"{what} uncovered rows")
    tf, tw = _t(feat, dev, True), _t(W, dev, True)
    tb, tr = (_t(b, dev, True) if use_b else None), (_t(res, dev, True) if use_r else None)
    out = autograd.sparse_conv(tf, tw, tb, tr, tnT, relu, (tn, 0))
    _eq_f(out, want, f"{what} forward through autograd")
    out.backward(_t(go, dev))
    g = gref.relu_mask(go, want, relu)
    gfeat, gw, mag, n, gb, magb = pref.inverse_grads(feat, nbr, nbrT, W, g)
    _eq_f(tf.grad, gfeat, f"{what} grad_feat")
    if lattice:
        _eq_exact_sum(tw.grad, gw, f"{what} grad_W")
    else:
        _within(tw.grad, gw, mag, n, f"{what} grad_W")
    if use_b:
        (_eq_exact_sum(tb.grad, gb, f"{what} grad_bias") if lattice else _within(tb.grad, gb, magb, Nv, f"{what} grad_bias"))
    if use_r:
        _eq_f(tr.grad, g, f"{what} grad_residual")
    return int(dead.sum())


@pytest.mark.parametrize("name", sorted(sc.FAMILIES))
def test_inverse_conv_every_family_and_geometry(dev, orc, name):
    coors, off, G = sc.FAMILIES[name][0]()
    uncovered = {}
    for gi, geo in enumerate(STRIDED):
        cin, cout = sc.CHANNEL_PAIRS[gi % 6]
        w = f"{name}/{geo[0]} inverse {cin}->{cout}"
        uncovered[geo[0]] = _check_inverse(dev, coors, off, G, geo, cin, cout, gi, bool(gi & 1), bool(gi & 2), gi % 3 != 0, w)
        _check_inverse(dev, coors, off, G, geo, cin, cout, gi + 9, True, True, False, w + " (lattice)", lattice=True)
    if name == "random030":
        assert uncovered["k222s2p0"] >= 1, "the odd grid must leave input rows that no window covers"


@pytest.mark.parametrize("cin,cout", sc.CHANNEL_PAIRS)
def test_inverse_conv_every_channel_pair(dev, orc, cin, cout):
    for name, geo in (("random030", STRIDED[0]), ("random030", STRIDED[3]), ("tile129", STRIDED[0])):
        coors, off, G = sc.FAMILIES[name][0]()
        for use_b, use_r, relu in ((True, False, True), (False, True, False)):
            _check_inverse(dev, coors, off, G, geo, cin, cout, cin + cout, use_b, use_r, relu, f"{name}/{geo[0]} inverse {cin}->{cout}")


# ---- layers ----------------------------------------------------------------------------------------------------------
def _with_nbrT(x):
    """The keys whose record holds a transposed rulebook."""
    return sorted(k for k, v in x.rulebooks.items() if v.nbrT is not None)


def _count(monkeypatch, mod, fn, calls):
    real = getattr(mod, fn)
    monkeypatch.setattr(mod, fn, lambda *a, **k: (calls.__setitem__(fn, calls.get(fn, 0) + 1), real(*a, **k))[1])


def test_layer_pairing(dev, orc, monkeypatch):
    import torch
    from sad_amd import ops
    from sad_amd.spconv import Rulebook, SparseConv3d, SparseInverseConv3d, SparseMaxPool3d, SparseTensor, SubMConv3d
    coors, off, G = sc.FAMILIES["random030"][0]()
    Nv = len(coors)
    feat = sc.make_feat(Nv, 4, 0)
    torch.manual_seed(3)
    subm = SubMConv3d(4, 16, 3, relu=True, indice_key="subm1").to(dev)
    down = SparseConv3d(16, 32, 2, 2, 0, relu=True, indice_key="down1").to(dev)
    subm2 = SubMConv3d(32, 32, 3, indice_key="subm2").to(dev)
    inv = SparseInverseConv3d(32, 16, 2, "down1", relu=True).to(dev)
    again = SubMConv3d(16, 8, 3, indice_key="subm1").to(dev)
    x0 = SparseTensor(_t(feat, dev), _t(coors, dev), _t(off, dev), G)
    with pytest.raises(ValueError, match="indice_key"):
        SparseInverseConv3d(32, 16, 2, None)
    with pytest.raises(ValueError, match="no rulebook"):
        inv(x0.replace_feature(torch.zeros((Nv, 32), device=dev)))
    x1 = subm(x0)
    x2 = down(x1)
    x3 = subm2(x2).replace_feature(subm2(x2).feat * 0.5)
    with pytest.raises(ValueError, match="submanifold"):
        SparseInverseConv3d(32, 16, 3, "subm2").to(dev)(x3)
    with pytest.raises(ValueError, match="kernel_size"):
        SparseInverseConv3d(32, 16, 3, "down1").to(dev)(x3)
    with pytest.raises(ValueError, match="not the tensor"):
        inv(x1.replace_feature(torch.zeros((Nv, 32), device=dev)))
    with pytest.raises(ValueError, match="input channels"):
        inv(x2.replace_feature(torch.zeros((x2.feat.shape[0], 8), device=dev)))
    assert _with_nbrT(x0) == []
    calls = {}
    _count(monkeypatch, ops, "sparse_conv_index", calls)
    _count(monkeypatch, ops, "sparse_conv_index_transpose", calls)
    y = inv(x3)
    assert y.coors is x0.coors and y.offsets is x0.offsets and y.spatial_shape == x0.spatial_shape and y.feat.shape == (Nv, 16)
    assert y.rulebooks is x0.rulebooks
    z = again(y)
    assert calls == {"sparse_conv_index_transpose": 1}, calls    # no new rulebook: the submanifold key of this resolution is a hit
    assert sorted(x0.rulebooks) == ["down1", "subm1", "subm2"] and all(isinstance(v, Rulebook) for v in x0.rulebooks.values())
    assert _with_nbrT(x0) == ["down1"] and x0.rulebooks["down1"].collisions == 0
    # the values: the reference chain
    oc, oo, nbr_d = ref.index_vec(coors, off, G, (2, 2, 2), (2, 2, 2), (0, 0, 0))
    nbr_s = ref.index_vec(coors, off, G, (3, 3, 3), subm=True)[2]
    nbrT_d, col = gref.index_transpose_vec(nbr_d, Nv)
    assert col == 0 and (nbrT_d < 0).all(1).any()
    _eq_int(x0.rulebooks["down1"].nbrT, nbrT_d, "cached nbrT")
    np_ = lambda m: (m.weight.detach().cpu().numpy(), None if m.bias is None else m.bias.detach().cpu().numpy())
    want = pref.inverse_conv(x3.feat.cpu().numpy(), nbrT_d, *np_(inv), None, True)
    _eq_f(y.feat, want, "inverse layer")
    _eq_f(z.feat, ref.conv(want, nbr_s, *np_(again)), "submanifold layer behind the inverse layer")
    dead = (nbrT_d < 0).all(1)
    _eq_f(y.feat[_t(dead, dev)], np.broadcast_to(np.maximum(np_(inv)[1], 0), (int(dead.sum()), 16)).astype(F), "uncovered rows: relu(bias)")
    # encoder backward and decoder forward share ONE transposed rulebook per key
    for m in (subm, down, subm2, inv, again):
        m.requires_grad_(True)
    calls.clear()
    x0g = SparseTensor(_t(feat, dev, True), x0.coors, x0.offsets, G, x0.rulebooks)
    out = again(inv(subm2(down(subm(x0g)))))
    assert calls == {}, calls                                    # down1's nbrT is there already; the others wait for the backward
    out.feat.sum().backward()
    assert calls == {"sparse_conv_index_transpose": 2}, calls    # subm1, subm2; down1 reused by the encoder's backward
    assert _with_nbrT(x0) == ["down1", "subm1", "subm2"] and x0g.feat.grad is not None
    # a pool as the partner; a hand-built tensor that carries the cache goes through the inverse layer like the layer's own
    pool = SparseMaxPool3d(2, indice_key="pool1")
    assert pool.stride == (2, 2, 2) and pool.padding == (0, 0, 0) and not list(pool.parameters())
    xp = pool(x1)
    assert xp.feat.requires_grad is False and xp.spatial_shape == x2.spatial_shape
    _eq_bits(xp.feat, pref.max_pool_vec(x1.feat.cpu().numpy(), nbr_d)[0], "pool layer")
    invp = SparseInverseConv3d(16, 16, 2, "pool1", bias=False).to(dev)
    yp = invp(xp)
    assert yp.coors is x0.coors
    _eq_f(yp.feat, pref.inverse_conv(xp.feat.cpu().numpy(), nbrT_d, np_(invp)[0]), "inverse of a pool")
    yh = invp(SparseTensor(xp.feat, xp.coors, xp.offsets, xp.spatial_shape, xp.rulebooks))
    assert yh.coors is x0.coors and yh.offsets is x0.offsets
    _eq_bits(yh.feat, yp.feat.cpu().numpy(), "inverse of a pool, hand-built input")
    # a pool and a convolution of one geometry may share a key
    shared = SparseMaxPool3d(2, 2, 0, indice_key="down1")
    calls.clear()
    xs = shared(x1)
    assert calls == {} and xs.coors is x2.coors


def test_layers_without_a_key_build_each_table_once(dev, orc, monkeypatch):
    """indice_key=None: an uncached record per forward, one rulebook and one transposed rulebook per layer, nothing left in the cache."""
    import torch
    from sad_amd import ops
    from sad_amd.spconv import SparseConv3d, SparseTensor, SubMConv3d
    coors, off, G = sc.FAMILIES["random030"][0]()
    feat = sc.make_feat(len(coors), 4, 6)
    torch.manual_seed(4)
    calls = {}
    _count(monkeypatch, ops, "sparse_conv_index", calls)
    _count(monkeypatch, ops, "sparse_conv_index_transpose", calls)
    for layer in (SubMConv3d(4, 8, 3), SparseConv3d(4, 8, 2, 2, 0)):
        layer = layer.to(dev).requires_grad_(True)
        x = SparseTensor(_t(feat, dev, True), _t(coors, dev), _t(off, dev), G)
        calls.clear()
        y = layer(x)
        assert calls == {"sparse_conv_index": 1}, calls
        y.feat.sum().backward()
        assert calls == {"sparse_conv_index": 1, "sparse_conv_index_transpose": 1}, calls
        assert x.rulebooks == {} and y.rulebooks is x.rulebooks
        nbr = ref.index_vec(coors, off, G, layer.kernel_size, layer.stride, layer.padding, layer.subm)[2]
        W, b = _wb(layer)
        out = ref.conv(feat, nbr, W, b)
        _eq_f(y.feat, out, "layer without a key")
        nbrT, col = gref.index_transpose_vec(nbr, len(coors))
        assert col == 0
        _eq_f(x.feat.grad, gref.grad_input(np.ones(out.shape, F), nbrT, W), "input gradient without a key")


def _unet(dev):
    import torch
    from sad_amd.spconv import SparseConv3d, SparseInverseConv3d, SparseMaxPool3d, SubMConv3d
    torch.manual_seed(0)
    return torch.nn.ModuleList([
        SubMConv3d(4, 16, 3, relu=True, indice_key="subm1"), SparseConv3d(16, 32, 3, 2, 1, relu=True, indice_key="down1"),
        SubMConv3d(32, 32, 3, relu=True, indice_key="subm2"), SparseMaxPool3d(2, 2, indice_key="down2"),
        SubMConv3d(32, 32, 3, relu=True, indice_key="subm3"), SparseInverseConv3d(32, 32, 2, "down2", relu=True),
        SparseInverseConv3d(32, 16, 3, "down1", bias=False, relu=True), SubMConv3d(32, 8, 3, indice_key="subm1")]).to(dev)


def _unet_forward(net, x0):
    """Encoder, decoder and the skip connection (torch.cat on .feat with the first layer's output)."""
    import torch
    from sad_amd.spconv import SparseSequential
    x1 = net[0](x0)
    x7 = SparseSequential(*net[1:7])(x1)
    assert x7.coors is x1.coors
    return net[7](x7.replace_feature(torch.cat([x7.feat, x1.feat], 1)))


def _wb(m):
    return m.weight.detach().cpu().numpy(), None if m.bias is None else m.bias.detach().cpu().numpy()


def _unet_reference(net, feat, coors, off, G, lossw):
    """The reference chain forward and backward -> (output, input gradient, {layer: (grad_W64, mag, n, grad_b64, magb, rows)})."""
    Nv = len(coors)
    nbr_s1 = ref.index_vec(coors, off, G, (3, 3, 3), subm=True)[2]
    c1, o1, nbr_d1 = ref.index_vec(coors, off, G, (3, 3, 3), (2, 2, 2), (1, 1, 1))
    G1 = ref.geometry(G, (3, 3, 3), (2, 2, 2), (1, 1, 1))[4]
    nbr_s2 = ref.index_vec(c1, o1, G1, (3, 3, 3), subm=True)[2]
    c2, o2, nbr_d2 = ref.index_vec(c1, o1, G1, (2, 2, 2), (2, 2, 2), (0, 0, 0))
    G2 = ref.geometry(G1, (2, 2, 2), (2, 2, 2), (0, 0, 0))[4]
    nbr_s3 = ref.index_vec(c2, o2, G2, (3, 3, 3), subm=True)[2]
    T = lambda nbr, n: gref.index_transpose_vec(nbr, n)
    (t_s1, k1), (t_d1, k2), (t_s2, k3), (t_d2, k4), (t_s3, k5) = T(nbr_s1, Nv), T(nbr_d1, Nv), T(nbr_s2, len(c1)), T(nbr_d2, len(c1)), T(nbr_s3, len(c2))
    assert k1 == k2 == k3 == k4 == k5 == 0
    # forward
    x1 = ref.conv(feat, nbr_s1, *_wb(net[0]), None, True)
    x2 = ref.conv(x1, nbr_d1, *_wb(net[1]), None, True)
    x3 = ref.conv(x2, nbr_s2, *_wb(net[2]), None, True)
    x4, arg = pref.max_pool_vec(x3, nbr_d2)
    x5 = ref.conv(x4, nbr_s3, *_wb(net[4]), None, True)
    x6 = pref.inverse_conv(x5, t_d2, *_wb(net[5]), None, True)
    x7 = pref.inverse_conv(x6, t_d1, *_wb(net[6]), None, True)
    cat = np.ascontiguousarray(np.concatenate([x7, x1], 1))
    out = ref.conv(cat, nbr_s1, *_wb(net[7]))
    # backward
    grads = {}

    def conv_back(li, fin, nbr, nbrT_for_input, g, out_rows):
        """one convolution layer: records its weight gradients, returns the gradient of its input (the §21.2 chain over the other
        rulebook of the pair and W^T)."""
        grads[li] = gref.grad_weight(fin, nbr, g) + (out_rows,)
        return gref.grad_input(g, nbrT_for_input, _wb(net[li])[0])

    g_cat = conv_back(7, cat, nbr_s1, t_s1, np.asarray(lossw, F), Nv)
    g_x7, g_skip = np.ascontiguousarray(g_cat[:, :16]), np.ascontiguousarray(g_cat[:, 16:])
    g_x6 = conv_back(6, x6, t_d1, nbr_d1, gref.relu_mask(g_x7, x7, True), Nv)
    g_x5 = conv_back(5, x5, t_d2, nbr_d2, gref.relu_mask(g_x6, x6, True), len(c1))
    g_x4 = conv_back(4, x4, nbr_s3, t_s3, gref.relu_mask(g_x5, x5, True), len(c2))
    g_x3 = pref.max_pool_grad_loop(g_x4, arg, t_d2)
    g_x2 = conv_back(2, x2, nbr_s2, t_s2, gref.relu_mask(g_x3, x3, True), len(c1))
    g_x1 = conv_back(1, x1, nbr_d1, t_d1, gref.relu_mask(g_x2, x2, True), len(c1))
    g_x1 = (g_x1 + g_skip).astype(F)                            # the two uses of the first layer's output
    g_in = conv_back(0, feat, nbr_s1, t_s1, gref.relu_mask(g_x1, x1, True), Nv)
    return out, g_in, grads


def _run_unet(dev, coors, off, G, seed, stream=None):
    import torch
    from sad_amd.spconv import Rulebook, SparseTensor
    net = _unet(dev).requires_grad_(True)
    feat = sc.make_feat(len(coors), 4, seed)
    lossw = np.random.default_rng(seed).integers(-2, 3, (len(coors), 8)).astype(F)
    x0 = SparseTensor(_t(feat, dev, True), _t(coors, dev), _t(off, dev), G)
    tl = _t(lossw, dev)
    torch.cuda.synchronize()
    with torch.cuda.stream(stream) if stream is not None else torch.cuda.stream(torch.cuda.current_stream()):
        y = _unet_forward(net, x0)
        (y.feat * tl).sum().backward()
    if stream is not None:
        stream.synchronize()
    torch.cuda.synchronize()
    assert y.coors is x0.coors and y.offsets is x0.offsets and y.feat.shape == (len(coors), 8)
    want, g_in, grads = _unet_reference(net, feat, coors, off, G, lossw)
    _eq_f(y.feat, want, "U-Net forward")
    _eq_f(x0.feat.grad, g_in, "U-Net input gradient")
    for li, (gw, mag, n, gb, magb, rows) in grads.items():
        _within(net[li].weight.grad, gw, mag, n, f"U-Net layer {li} grad_W")
        if net[li].bias is not None:
            _within(net[li].bias.grad, gb, magb, rows, f"U-Net layer {li} grad_bias")
    assert sorted(x0.rulebooks) == ["down1", "down2", "subm1", "subm2", "subm3"] and all(isinstance(v, Rulebook) for v in x0.rulebooks.values())
    assert _with_nbrT(x0) == sorted(x0.rulebooks)
    return net, x0, y


def test_unet_end_to_end(dev, orc, monkeypatch):
    import torch
    from sad_amd import ops
    coors, off, G = sc.FAMILIES["synth"][0]()
    calls = {}
    _count(monkeypatch, ops, "sparse_conv_index", calls)
    _count(monkeypatch, ops, "sparse_conv_index_transpose", calls)
    net, x0, y = _run_unet(dev, coors, off, G, 9)
    assert calls == {"sparse_conv_index": 5, "sparse_conv_index_transpose": 5}, calls      # once per key, the second subm1 layer a hit
    # without gradients the same values, no graph
    with torch.no_grad():
        y2 = _unet_forward(net, x0)
    assert y2.feat.grad_fn is None and torch.equal(y2.feat, y.feat.detach())
    net.requires_grad_(False)
    x0.feat.requires_grad_(False)
    y3 = _unet_forward(net, x0)
    assert y3.feat.requires_grad is False and torch.equal(y3.feat, y.feat.detach())


def test_unet_non_default_stream_and_empty_scene(dev, orc):
    import torch
    coors, off, G = sc.FAMILIES["empty_scene"][0]()
    assert (np.diff(off) == 0).any()
    _run_unet(dev, coors, off, G, 4, stream=torch.cuda.Stream(device=dev))


def test_unet_without_voxels(dev):
    import torch
    from sad_amd.spconv import SparseTensor
    net = _unet(dev).requires_grad_(True)
    x0 = SparseTensor(torch.zeros((0, 4), device=dev, requires_grad=True), torch.zeros((0, 3), dtype=torch.int32, device=dev),
                      torch.zeros((3,), dtype=torch.int32, device=dev), (6, 7, 8))
    y = _unet_forward(net, x0)
    assert tuple(y.feat.shape) == (0, 8) and y.coors is x0.coors
    y.feat.sum().backward()
    assert tuple(x0.feat.grad.shape) == (0, 4)
    for m in net:
        for prm in m.parameters():
            assert prm.grad is not None and not bool(prm.grad.any())
