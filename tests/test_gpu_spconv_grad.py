"""GPU parity of the sparse-convolution backward (SPEC.md §21.4) (-m gpu) against tests/spconv_grad_ref.py.

Transposed rulebook: np.array_equal.  grad_feat: ``==`` (the §21.2 chain over the transposed operands; sign of a zero unspecified).
grad_W / grad_bias: the order of the additions is not specified, so (a) on lattice inputs (integers, |g| <= 4, |feat| <= 8: every
partial sum is representable) ``==`` in any order, and (b) on float inputs, per element whose sum has n terms,
|gpu - ref64| <= n * 2^-23 * sum |terms| (twice the first-order bound of n products each rounded or fused once, §21.4); the worst
err / bound of every case is printed.  Families and coverage: tests/spconv_cases.py."""
import numpy as np
import pytest

import spconv_cases as sc
import spconv_grad_ref as gref
import spconv_ref as ref

pytestmark = pytest.mark.gpu

F = np.float32
DUP_SKIPS = {("duplicates", "subm333"), ("duplicates", "subm111")}


def _t(a, dev, grad=False):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return t.requires_grad_(True) if grad else t


def _eq_int(got, want, what):
    got = got.cpu().numpy()
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    assert np.array_equal(got, want), f"{what}: {int((got != want).sum())} of {want.size} entries differ"


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
    """The §21.4 rule; -> worst err / bound (printed by the caller)."""
    got = got.detach().cpu().numpy()
    assert got.shape == want64.shape and got.dtype == F, (what, got.shape, want64.shape, got.dtype)
    bound = gref.grad_weight_bound(mag, n)
    err = np.abs(got.astype(np.float64) - want64)
    worst = float((err / np.maximum(bound, 1e-300)).max()) if err.size else 0.0
    print(f"{what}: worst err / bound = {worst:.4g}")
    assert (err <= bound).all(), f"{what}: {int((err > bound).sum())} of {err.size} values outside n * 2^-23 * sum|terms|, worst {worst:.4g} x"
    return worst


def _check_grad_weight(dev, feat, nbr, g, what, lattice):
    from sad_amd import ops
    gw, mag, n, gb, magb = gref.grad_weight(feat, nbr, g)
    got_w, got_b = ops.sparse_conv_grad_weight(_t(feat, dev), _t(nbr, dev), _t(g, dev))
    if lattice:
        _eq_exact_sum(got_w, gw, f"{what} grad_W")
        _eq_exact_sum(got_b, gb, f"{what} grad_bias")
    else:
        _within(got_w, gw, mag, n, f"{what} grad_W")
        _within(got_b, gb, magb, len(nbr), f"{what} grad_bias")
    w2, b2 = ops.sparse_conv_grad_weight(_t(feat, dev), _t(nbr, dev), _t(g, dev), bias=False)
    assert b2 is None
    (_eq_exact_sum if lattice else lambda a, b, c: _within(a, b, mag, n, c))(w2, gw, f"{what} grad_W (no bias)")


@pytest.mark.parametrize("name", sorted(sc.FAMILIES))
def test_index_transpose_every_family_and_geometry(dev, name):
    from sad_amd import ops
    coors, off, G = sc.FAMILIES[name][0]()
    sc.check_coverage(name, coors, off, G)
    for gname, K, s, p, subm in sc.GEOMETRIES:
        nbr = ref.index_vec(coors, off, G, K, s, p, subm)[2]
        want, col = gref.index_transpose_vec(nbr, len(coors))
        nbrT, c = ops.sparse_conv_index_transpose(_t(nbr, dev), len(coors))
        _eq_int(nbrT, want, f"{name}/{gname} nbrT")
        assert str(c.dtype) == "torch.int32" and int(c.item()) == col, f"{name}/{gname}: collisions {int(c.item())}, reference {col}"
        assert (col > 0) == ((name, gname) in DUP_SKIPS)
        if len(nbr):                                             # entries outside [0, Nv) count as -1
            bad = nbr.copy()
            bad[-1, :] = len(coors) + 7
            cut = nbr.copy()
            cut[-1, :] = -1
            w2, c2 = gref.index_transpose_vec(cut, len(coors))
            g2 = ops.sparse_conv_index_transpose(_t(bad, dev), len(coors))
            _eq_int(g2[0], w2, f"{name}/{gname} nbrT (out-of-range entries)")
            assert int(g2[1].item()) == c2
    # more input rows than any entry names: the extra rows are -1
    nbrT, c = ops.sparse_conv_index_transpose(_t(nbr, dev), len(coors) + 5)
    assert bool((nbrT[len(coors):] == -1).all()) and nbrT.shape[0] == len(coors) + 5


def test_grad_feat_every_family_and_geometry(dev, orc):
    from sad_amd import ops
    skipped = set()
    for name in sorted(sc.FAMILIES):
        coors, off, G = sc.FAMILIES[name][0]()
        for gi, (gname, K, s, p, subm) in enumerate(sc.GEOMETRIES):
            nbr = ref.index_vec(coors, off, G, K, s, p, subm)[2]
            nbrT, col = gref.index_transpose_vec(nbr, len(coors))
            if col > 0:
                skipped.add((name, gname))
                continue
            cin, cout = sc.CHANNEL_PAIRS[gi % 6]
            W, _ = sc.make_layer(nbr.shape[1], cin, cout, gi)
            g = sc.make_feat(len(nbr), cout, gi + 5)
            g[::3] = 0                                           # (rows a ReLU switched off)
            got = ops.sparse_conv_grad_input(_t(g, dev), _t(nbrT, dev), _t(W, dev))
            _eq_f(got, gref.grad_input(g, nbrT, W), f"{name}/{gname} grad_feat {cin}<-{cout}")
    assert skipped == DUP_SKIPS, f"left out: {sorted(skipped)}"


@pytest.mark.parametrize("cin,cout", sc.CHANNEL_PAIRS)
def test_grad_feat_every_channel_pair(dev, orc, cin, cout):
    from sad_amd import ops
    for name, (gname, K, s, p, subm) in (("random030", sc.GEOMETRIES[0]), ("tile129", sc.GEOMETRIES[2])):
        coors, off, G = sc.FAMILIES[name][0]()
        nbr = ref.index_vec(coors, off, G, K, s, p, subm)[2]
        nbrT, col = gref.index_transpose_vec(nbr, len(coors))
        assert col == 0
        W, _ = sc.make_layer(27, cin, cout, cin + cout)
        g = sc.make_feat(len(nbr), cout, cout + 1)
        tw = _t(W, dev)
        want = gref.grad_input(g, nbrT, W)
        _eq_f(ops.sparse_conv_grad_input(_t(g, dev), _t(nbrT, dev), tw), want, f"{name}/{gname} grad_feat {cin}<-{cout}")
        packed_t = ops.PackedSparseWeight(tw.transpose(1, 2).contiguous(), None)
        _eq_f(ops.sparse_conv_grad_input(_t(g, dev), _t(nbrT, dev), packed_t), want, f"{name}/{gname} grad_feat {cin}<-{cout} (packed)")


@pytest.mark.parametrize("name", sorted(sc.FAMILIES))
def test_grad_weight_every_family_and_geometry(dev, orc, name):
    """Operator on lattice and float inputs, then the same gradients through ``autograd.sparse_conv`` with bias / residual / ReLU
    switched on and off in turn (the duplicate-coordinate submanifold cases without a gradient for feat: it is not defined)."""
    from sad_amd import autograd
    coors, off, G = sc.FAMILIES[name][0]()
    for gi, (gname, K, s, p, subm) in enumerate(sc.GEOMETRIES):
        w = f"{name}/{gname}"
        nbr = ref.index_vec(coors, off, G, K, s, p, subm)[2]
        cin, cout = sc.CHANNEL_PAIRS[gi % 6]
        Kvol, Nv, No = nbr.shape[1], len(coors), len(nbr)
        _check_grad_weight(dev, gref.lattice((Nv, cin), 8, gi), nbr, gref.lattice((No, cout), 4, gi + 1), w, True)
        feat, go = sc.make_feat(Nv, cin, gi + 1), sc.make_feat(No, cout, gi + 4)
        _check_grad_weight(dev, feat, nbr, go, w, False)
        use_b, use_r, relu = bool(gi & 1), bool(gi & 2), gi % 3 != 0
        W, b = sc.make_layer(Kvol, cin, cout, gi)
        res = sc.make_feat(No, cout, gi + 2)
        dup = (name, gname) in DUP_SKIPS
        tf, tw, tb, tr = _t(feat, dev, not dup), _t(W, dev, True), _t(b, dev, True) if use_b else None, _t(res, dev, True) if use_r else None
        out = autograd.sparse_conv(tf, tw, tb, tr, _t(nbr, dev), relu)
        want = ref.conv(feat, nbr, W, b if use_b else None, res if use_r else None, relu)
        _eq_f(out, want, f"{w} forward through autograd")
        out.backward(_t(go, dev))
        g = gref.relu_mask(go, want, relu)
        gw, mag, n, gb, magb = gref.grad_weight(feat, nbr, g)
        _within(tw.grad, gw, mag, n, f"{w} autograd grad_W bias={use_b} residual={use_r} relu={relu}")
        if use_b:
            _within(tb.grad, gb, magb, No, f"{w} autograd grad_bias")
        if use_r:
            _eq_f(tr.grad, g, f"{w} autograd grad_residual")
        if not dup:
            _eq_f(tf.grad, gref.grad_input(g, gref.index_transpose_vec(nbr, Nv)[0], W), f"{w} autograd grad_feat")
        else:
            assert tf.grad is None


@pytest.mark.parametrize("cin,cout", sc.CHANNEL_PAIRS)
def test_grad_weight_every_channel_pair(dev, orc, cin, cout):
    from sad_amd import autograd
    for name, (gname, K, s, p, subm) in (("random030", sc.GEOMETRIES[0]), ("tile129", sc.GEOMETRIES[2]), ("random002", sc.GEOMETRIES[0])):
        coors, off, G = sc.FAMILIES[name][0]()
        nbr = ref.index_vec(coors, off, G, K, s, p, subm)[2]
        Nv, No, w = len(coors), len(nbr), f"{name}/{gname} {cin}->{cout}"
        _check_grad_weight(dev, gref.lattice((Nv, cin), 8, cin), nbr, gref.lattice((No, cout), 4, cout), w, True)
        feat, go, res = sc.make_feat(Nv, cin, cin), sc.make_feat(No, cout, cout + 3), sc.make_feat(No, cout, cout)
        _check_grad_weight(dev, feat, nbr, go, w, False)
        W, b = sc.make_layer(27, cin, cout, cin + cout)
        tn = _t(nbr, dev)
        for use_b, use_r, relu in ((False, False, False), (True, False, True), (False, True, False), (True, True, True)):
            tf, tw, tb, tr = _t(feat, dev), _t(W, dev, True), _t(b, dev, True) if use_b else None, _t(res, dev, True) if use_r else None
            autograd.sparse_conv(tf, tw, tb, tr, tn, relu).backward(_t(go, dev))
            g = gref.relu_mask(go, ref.conv(feat, nbr, W, b if use_b else None, res if use_r else None, relu), relu)
            gw, mag, n, gb, magb = gref.grad_weight(feat, nbr, g)
            _within(tw.grad, gw, mag, n, f"{w} grad_W bias={use_b} residual={use_r} relu={relu}")
            if use_b:
                _within(tb.grad, gb, magb, No, f"{w} grad_bias")
            if use_r:
                _eq_f(tr.grad, g, f"{w} grad_residual")
            assert tf.grad is None


def test_empty_inputs_give_zeros(dev):
    import torch
    from sad_amd import ops
    # an empty scene list: no output rows
    nbr = torch.zeros((0, 27), dtype=torch.int32, device=dev)
    gw, gb = ops.sparse_conv_grad_weight(torch.ones((5, 4), device=dev), nbr, torch.zeros((0, 8), device=dev))
    assert tuple(gw.shape) == (27, 8, 4) and tuple(gb.shape) == (8,) and not bool(gw.any()) and not bool(gb.any())
    nbrT, col = ops.sparse_conv_index_transpose(nbr, 5)
    assert tuple(nbrT.shape) == (5, 27) and bool((nbrT == -1).all()) and int(col.item()) == 0
    gf = ops.sparse_conv_grad_input(torch.zeros((0, 8), device=dev), nbrT, torch.ones((27, 8, 4), device=dev))
    assert tuple(gf.shape) == (5, 4) and not bool(gf.any())
    # no input rows: every entry is -1; grad_bias still sums g
    nbr = torch.full((3, 27), -1, dtype=torch.int32, device=dev)
    g = torch.arange(24, dtype=torch.float32, device=dev).view(3, 8)
    gw, gb = ops.sparse_conv_grad_weight(torch.zeros((0, 4), device=dev), nbr, g)
    assert not bool(gw.any()) and torch.equal(gb, g.sum(0))
    nbrT, col = ops.sparse_conv_index_transpose(nbr, 0)
    assert tuple(nbrT.shape) == (0, 27) and int(col.item()) == 0


def test_duplicate_coordinates_refuse_backward_not_forward(dev, orc):
    import torch
    from sad_amd.spconv import SparseTensor, SubMConv3d
    coors, off, G = sc.FAMILIES["duplicates"][0]()
    feat = sc.make_feat(len(coors), 4, 0)
    torch.manual_seed(1)
    m = SubMConv3d(4, 16, 3, relu=True, indice_key="k").to(dev).requires_grad_(True)
    x = SparseTensor(_t(feat, dev, True), _t(coors, dev), _t(off, dev), G)
    y = m(x)
    nbr = ref.index_vec(coors, off, G, (3, 3, 3), subm=True)[2]
    _eq_f(y.feat, ref.conv(feat, nbr, m.weight.detach().cpu().numpy(), m.bias.detach().cpu().numpy(), None, True), "forward on duplicates")
    with pytest.raises(ValueError, match="duplicate coordinate"):
        y.feat.sum().backward()
    # without a gradient for feat the layer trains: grad_W is defined
    x2 = SparseTensor(_t(feat, dev), _t(coors, dev), _t(off, dev), G)
    y2 = m(x2)
    y2.feat.sum().backward()
    g = gref.relu_mask(np.ones(y2.feat.shape, F), y2.feat.detach().cpu().numpy(), True)
    gw, mag, n, gb, magb = gref.grad_weight(feat, nbr, g)
    _within(m.weight.grad, gw, mag, n, "duplicates grad_W")


def _net(dev):
    import torch
    from sad_amd.spconv import SparseConv3d, SparseSequential, SubMConv3d
    torch.manual_seed(0)
    return SparseSequential(SubMConv3d(4, 16, 3, relu=True, indice_key="subm1"), SubMConv3d(16, 16, 3, relu=True, indice_key="subm1"),
                            SparseConv3d(16, 32, 3, 2, 1, relu=True, indice_key="down1"), SubMConv3d(32, 32, 3, bias=False, indice_key="subm2")).to(dev)


def test_autograd_sequential_end_to_end(dev, orc, monkeypatch):
    import torch
    from sad_amd import ops
    from sad_amd.spconv import Rulebook, SparseTensor
    coors, off, G = sc.FAMILIES["synth"][0]()
    net = _net(dev).requires_grad_(True)
    feat = sc.make_feat(len(coors), 4, 9)
    x0 = SparseTensor(_t(feat, dev, True), _t(coors, dev), _t(off, dev), G)
    y = net(x0)
    assert y.feat.requires_grad
    d = y.dense()
    lossw = np.random.default_rng(5).integers(-2, 3, tuple(d.shape)).astype(F)      # the fixed weights of the loss
    (d * _t(lossw, dev)).sum().backward()
    # the reference, forward then backward layer by layer
    f, c, o, g3 = feat, coors, off, G
    steps = []
    for m in net:
        oc, oo, nbr = ref.index_vec(c, o, g3, m.kernel_size, m.stride, m.padding, m.subm)
        W, b = m.weight.detach().cpu().numpy(), None if m.bias is None else m.bias.detach().cpu().numpy()
        out = ref.conv(f, nbr, W, b, None, m.relu)
        steps.append((m, f, nbr, W, out))
        g3 = ref.geometry(g3, m.kernel_size, m.stride, m.padding, m.subm)[4]
        f, c, o = out, oc, oo
    _eq_f(y.feat, f, "forward with gradients on")
    _eq_f(d, ref.to_dense(f, c, o, g3), "dense with gradients on")
    grad = gref.to_dense_grad(lossw, c, o)
    for li in range(len(steps) - 1, -1, -1):
        m, fin, nbr, W, out = steps[li]
        g = gref.relu_mask(grad, out, m.relu)
        gw, mag, n, gb, magb = gref.grad_weight(fin, nbr, g)
        _within(m.weight.grad, gw, mag, n, f"layer {li} grad_W")
        if m.bias is not None:
            _within(m.bias.grad, gb, magb, len(nbr), f"layer {li} grad_bias")
        nbrT, col = gref.index_transpose_vec(nbr, len(fin))
        assert col == 0
        grad = gref.grad_input(g, nbrT, W)
    _eq_f(x0.feat.grad, grad, "input gradient")
    # the transposed rulebooks sit on the records of the rulebooks, whose keys are what they were
    assert sorted(x0.rulebooks) == ["down1", "subm1", "subm2"]
    assert all(isinstance(v, Rulebook) and v.nbrT is not None for v in x0.rulebooks.values())
    cachedT = {k: v.nbrT for k, v in x0.rulebooks.items()}
    _eq_int(cachedT["subm1"], gref.index_transpose_vec(steps[0][2], len(coors))[0], "cached nbrT")
    # a second backward on a fresh forward reuses them; frozen parameters cost no weight-gradient call, an input without
    # requires_grad no input-gradient call for the first layer
    calls = {"w": 0, "i": 0, "t": 0}
    real_w, real_i, real_t = ops.sparse_conv_grad_weight, ops.sparse_conv_grad_input, ops.sparse_conv_index_transpose
    monkeypatch.setattr(ops, "sparse_conv_grad_weight", lambda *a, **k: (calls.__setitem__("w", calls["w"] + 1), real_w(*a, **k))[1])
    monkeypatch.setattr(ops, "sparse_conv_grad_input", lambda *a, **k: (calls.__setitem__("i", calls["i"] + 1), real_i(*a, **k))[1])
    monkeypatch.setattr(ops, "sparse_conv_index_transpose", lambda *a, **k: (calls.__setitem__("t", calls["t"] + 1), real_t(*a, **k))[1])
    net.zero_grad(set_to_none=True)
    net[1].requires_grad_(False)
    x0.feat.requires_grad_(False)
    net(x0).feat.sum().backward()
    assert calls == {"w": 3, "i": 3, "t": 0}, calls
    assert net[1].weight.grad is None and net[1].bias.grad is None and net[0].weight.grad is not None
    assert all(x0.rulebooks[k].nbrT is cachedT[k] for k in cachedT)
    # an in-place weight update between two forwards is seen (the packs are re-made), with and without gradients
    before = net(x0).feat.detach().clone()
    with torch.no_grad():
        net[0].weight.mul_(2.0)
        net[0].bias.add_(0.25)
    f1 = ref.conv(feat, steps[0][2], net[0].weight.detach().cpu().numpy(), net[0].bias.detach().cpu().numpy(), None, True)
    _eq_f(net[0](x0).feat, f1, "layer 0 after an in-place update")
    with torch.no_grad():
        _eq_f(net[0](x0).feat, f1, "layer 0 after an in-place update (no_grad)")
    assert not torch.equal(net(x0).feat.detach(), before)
    # ... and by the packed W^T of the input gradient
    xg = SparseTensor(_t(feat, dev, True), x0.coors, x0.offsets, G, x0.rulebooks)
    go = sc.make_feat(len(coors), 16, 3)
    net[0](xg).feat.backward(_t(go, dev))
    g = gref.relu_mask(go, f1, True)
    _eq_f(xg.feat.grad, gref.grad_input(g, gref.index_transpose_vec(steps[0][2], len(coors))[0], net[0].weight.detach().cpu().numpy()),
          "grad_feat after an in-place update")


def test_default_path_untouched_and_non_default_stream(dev, orc):
    import torch
    from sad_amd import autograd, ops
    from sad_amd.spconv import SparseTensor
    coors, off, G = sc.FAMILIES["random030"][0]()
    net = _net(dev)
    feat = sc.make_feat(len(coors), 4, 2)
    x = SparseTensor(_t(feat, dev), _t(coors, dev), _t(off, dev), G)
    y = net[0](x)
    assert y.feat.requires_grad is False and y.feat.grad_fn is None and all(v.nbrT is None for v in x.rulebooks.values())
    nbr = ref.index_vec(coors, off, G, (3, 3, 3), subm=True)[2]
    _eq_f(y.feat, ref.conv(feat, nbr, net[0].weight.cpu().numpy(), net[0].bias.cpu().numpy(), None, True), "default path")
    assert x.dense().requires_grad is False
    # dense() with a gradient: a gather, exact (duplicates: the lowest row owns the cell)
    dc, do, dG = sc.FAMILIES["duplicates"][0]()
    f2 = sc.make_feat(len(dc), 3, 1)
    xd = SparseTensor(_t(f2, dev, True), _t(dc, dev), _t(do, dev), dG)
    gd = sc.make_feat(2 * 3 * dG[0] * dG[1] * dG[2], 1, 8).reshape((2, 3) + tuple(dG))
    xd.bev().backward(_t(gd.reshape(2, 3 * dG[0], dG[1], dG[2]), dev))
    _eq_f(xd.feat.grad, gref.to_dense_grad(gd, dc, do), "sparse_to_dense backward")
    # everything on a non-default stream
    gname, K, s, p, subm = sc.GEOMETRIES[2]
    oc, oo, nbr = ref.index_vec(coors, off, G, K, s, p, subm)
    W, b = sc.make_layer(27, 16, 32, 0)
    feat, go = sc.make_feat(len(coors), 16, 1), sc.make_feat(len(oc), 32, 2)
    tf, tw, tb, tn, tg = _t(feat, dev, True), _t(W, dev, True), _t(b, dev, True), _t(nbr, dev), _t(go, dev)
    torch.cuda.synchronize()
    st = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(st):
        nbrT, col = ops.sparse_conv_index_transpose(tn, len(coors))
        out = autograd.sparse_conv(tf, tw, tb, None, tn, True, (nbrT, 0))
        out.backward(tg)
    st.synchronize()
    want = ref.conv(feat, nbr, W, b, None, True)
    g = gref.relu_mask(go, want, True)
    wantT, wcol = gref.index_transpose_vec(nbr, len(coors))
    _eq_int(nbrT, wantT, "nbrT (stream)")
    assert int(col.item()) == wcol == 0
    _eq_f(out, want, "forward (stream)")
    _eq_f(tf.grad, gref.grad_input(g, wantT, W), "grad_feat (stream)")
    gw, mag, n, gb, magb = gref.grad_weight(feat, nbr, g)
    _within(tw.grad, gw, mag, n, "grad_W (stream)")
    _within(tb.grad, gb, magb, len(oc), "grad_bias (stream)")


def _big_scenes(G, densities, seed):
    """Scenes of very different density, rows shuffled inside a scene: long runs of 64-row tiles whose offset masks differ."""
    rng = np.random.default_rng(seed)
    scenes = []
    for d in densities:
        pick = rng.permutation(np.flatnonzero(rng.random(int(np.prod(G))) < d))
        scenes.append(np.stack(np.unravel_index(pick, G), -1).astype(np.int32).reshape(-1, 3))
    off = np.concatenate([[0], np.cumsum([len(s) for s in scenes])]).astype(np.int32)
    return np.ascontiguousarray(np.concatenate(scenes)), off


def _ranges(No, cin, cout, cus, knob):
    """The host's sizing of the weight-gradient grid (csrc/spconv_grad.hip) -> (tiles, tiles per workgroup)."""
    ntiles = -(-No // 64)
    nblk = -(-(-(-cout // 32)) // 4) * -(-(-(-cin // 32)) // 4)
    target = knob if knob > 0 else max(1, 2 * cus // nblk)
    return ntiles, min(1024, max(1, -(-ntiles // target)))


@pytest.mark.parametrize("cin,cout,G,dens,knobs", [
    (4, 16, (16, 96, 96), (0.2, 0.004, 0.2, 0.06), (0, 1, 7)),          # ~68 k rows, one [Cout x Cin] block; knob 1: more than 1024 tiles, the cap
    (256, 200, (8, 64, 64), (0.25, 0.01, 0.3), (0, 3)),                  # ~18 k rows, four blocks of 128 x 128 (the second ones partial)
    (64, 64, (8, 64, 64), (0.01, 0.3, 0.02), (5, 2)),                    # two waves along Cout, two along the rows
])
def test_grad_weight_many_tiles_per_workgroup(dev, cin, cout, G, dens, knobs):
    """Workgroups that own SEVERAL 64-row tiles (no other test reaches that on a 256-CU device: it needs more than 8 192 .. 32 768
    rows): the accumulators carried over the tiles of a range and reset per offset, the per-tile masks and their skip, a partial
    last tile, the cap of 1024 tiles per workgroup.  The sizing is restated here and asserted, so the coverage cannot lapse
    silently; the knob ``spconv_grad_ranges`` forces other splits of the same rows.  Lattice inputs ``==``, floats by the §21.4 rule."""
    import torch
    from sad_amd import _lib
    coors, off = _big_scenes(G, dens, cin + cout)
    nbr = ref.index_vec(coors, off, G, (3, 3, 3), subm=True)[2]
    Nv = No = len(coors)
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    has = nbr >= 0
    pad = (-No) % 64
    tmask = np.concatenate([has, np.zeros((pad, 27), bool)]).reshape(-1, 64, 27).any(1)          # [tiles, 27]
    assert No % 64 != 0, "the last tile must be partial"
    lat_f, lat_g = gref.lattice((Nv, cin), 8, 1), gref.lattice((No, cout), 4, 2)
    flo_f, flo_g = sc.make_feat(Nv, cin, 3), sc.make_feat(No, cout, 4)
    try:
        for knob in knobs:
            ntiles, tpw = _ranges(No, cin, cout, cus, knob)
            assert tpw >= 3, f"knob {knob}: {ntiles} tiles on {cus} compute units give {tpw} tiles per workgroup: the case is too small"
            if knob == 1:
                assert ntiles > 1024 and tpw == 1024
            # some range holds, away from its ends, a tile that lacks an offset another tile of the range needs
            mixed = False
            for t0 in range(0, ntiles, tpw):
                r = tmask[t0:t0 + tpw]
                mixed = mixed or (len(r) >= 3 and bool((~r[1:-1] & r.any(0)[None, :]).any()))
            assert mixed, f"knob {knob}: no range with a mid-range tile that skips an offset"
            _lib.set_option("spconv_grad_ranges", knob)
            _check_grad_weight(dev, lat_f, nbr, lat_g, f"big {cin}->{cout} ranges={knob}", True)
            _check_grad_weight(dev, flo_f, nbr, flo_g, f"big {cin}->{cout} ranges={knob}", False)
    finally:
        _lib.set_option("spconv_grad_ranges", 0)


def test_frozen_weight_pays_for_the_bias_sums_only(dev, orc, monkeypatch):
    from sad_amd import autograd, ops
    coors, off, G = sc.FAMILIES["random030"][0]()
    nbr = ref.index_vec(coors, off, G, (3, 3, 3), subm=True)[2]
    W, b = sc.make_layer(27, 16, 32, 0)
    feat, go = sc.make_feat(len(coors), 16, 1), sc.make_feat(len(nbr), 32, 2)
    seen = []
    real = ops.sparse_conv_grad_weight
    monkeypatch.setattr(ops, "sparse_conv_grad_weight", lambda *a, **k: (seen.append(k), real(*a, **k))[1])
    tw, tb = _t(W, dev), _t(b, dev, True)
    autograd.sparse_conv(_t(feat, dev), tw, tb, None, _t(nbr, dev), True).backward(_t(go, dev))
    assert seen == [{"bias": True, "weight": False}] and tw.grad is None
    g = gref.relu_mask(go, ref.conv(feat, nbr, W, b, None, True), True)
    _, _, _, gb, magb = gref.grad_weight(feat, nbr, g)
    _within(tb.grad, gb, magb, len(nbr), "grad_bias alone")
    gw, gb2 = real(_t(feat, dev), _t(nbr, dev), _t(g, dev), bias=True, weight=False)
    assert gw is None
    _within(gb2, gb, magb, len(nbr), "grad_bias alone (operator)")
    with pytest.raises(ValueError):
        real(_t(feat, dev), _t(nbr, dev), _t(g, dev), bias=False, weight=False)


def test_sparse_to_dense_backward_rows_outside_and_double_backward(dev):
    import torch
    from sad_amd import autograd
    coors = np.array([[0, 1, 1], [0, 1, 1], [-1, -1, -1], [1, 0, 2], [0, 1, 1], [5, 0, 0]], np.int32)      # duplicates, a -1 row, one outside
    off = np.array([0, 3, 6], np.int32)
    f = _t(sc.make_feat(6, 2, 0), dev, True)
    d = autograd.sparse_to_dense(f, _t(coors, dev), _t(off, dev), (2, 2, 3))
    gd = sc.make_feat(2 * 2 * 12, 1, 1).reshape(2, 2, 2, 2, 3)
    (g,) = torch.autograd.grad(d, f, _t(gd, dev, True), create_graph=True)       # (a gradient that itself requires grad: double backward)
    want = np.zeros((6, 2), F)
    want[0], want[3], want[4] = gd[0, :, 0, 1, 1], gd[1, :, 1, 0, 2], gd[1, :, 0, 1, 1]
    _eq_f(g, want, "sparse_to_dense backward")
    with pytest.raises(RuntimeError, match="once_differentiable"):
        g.sum().backward()
