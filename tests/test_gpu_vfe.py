"""GPU parity of the voxel feature encoder (SPEC.md §24) (-m gpu): ops.voxel_decorate, ops.voxel_encode, autograd.voxel_encode
and PillarFeatureNet against tests/vfe_ref.py.  pooled and pointwise are EQUAL to the reference after +0.0 normalisation of
zeros (i.e. under ==), arg is equal exactly, the fused result equals the composition decorate -> PackedMLP.rows ->
voxel_reduce(max), and a second call is bit-equal to the first.  The operators are fed the REFERENCE's point2voxel.  Coverage
conditions are asserted on the reference (here and in tests/test_vfe_cpu.py); nothing is skipped."""
import numpy as np
import pytest

import vfe_ref as vfe
import voxel_cases as vc
import voxel_ref as vr

pytestmark = pytest.mark.gpu

F = np.float32


def _t(a, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _weights(cin, cout, seed=0):
    rng = np.random.default_rng(7000 + seed + 13 * cin + cout)
    return (rng.standard_normal((cout, cin)) / np.sqrt(cin)).astype(F), (rng.standard_normal(cout) * 0.1).astype(F)


def _eqz(got, want, what):
    got = got.cpu().numpy()
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape)
    assert np.array_equal(vfe.pz(got), vfe.pz(want)), f"{what}: {int((got != want).sum())} of {want.size} entries differ"


def _eq(got, want, what):
    got = got.cpu().numpy()
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape)
    assert np.array_equal(got, want), f"{what}: {int((got != want).sum())} of {want.size} entries differ"


def _check(dev, orc, pts, off, p2v, V, cout, relu=True, coors=None, v=None, r=None, cc=True, vc=True, vox_feat=None, T=None,
           batched=None, W=None, b=None, compose=True):
    """Every equality of the module docstring on one input.  -> the reference's (pooled, arg, pointwise, rows)."""
    import torch
    from sad_amd import ops
    C = pts.shape[1]
    cin = C + 3 * cc + 3 * vc + (0 if vox_feat is None else vox_feat.shape[-1])
    if W is None:
        W, b = _weights(cin, cout)
    want_p, want_a, want_y, want_r = vfe.encode(orc, pts, p2v, off, V, W, b, relu, coors=coors, voxel_size=v, point_range=r,
                                                cluster_center=cc, voxel_center=vc, vox_feat=vox_feat, T=T)
    tp, to, tv = _t(pts, dev), _t(off, dev), _t(p2v, dev)
    tc = None if coors is None else _t(coors, dev)
    tf = None if vox_feat is None else _t(vox_feat, dev)
    tW, tb = _t(W, dev), _t(b, dev)
    kw = dict(coors=tc, voxel_size=v, point_range=r, cluster_center=cc, voxel_center=vc, vox_feat=tf, max_points=T)
    rows = ops.voxel_decorate(tp, tv, to, V, **kw)
    _eq(rows, want_r, "rows")
    pooled, arg, pw = ops.voxel_encode(tp, tv, to, V, tW, tb, relu=relu, return_arg=True, return_pointwise=True, **kw)
    _eqz(pooled, want_p, "pooled")
    _eq(arg, want_a, "arg")
    _eqz(pw, want_y, "pointwise")
    ws = ops.voxel_encode_workspace(pts.shape[0], len(off) - 1, V, cin, W.shape[0], dev)
    for k in range(2):                                          # without arg / pointwise, on a workspace used twice
        alone = ops.voxel_encode(tp, tv, to, V, tW, tb, relu=relu, workspace=ws, **kw)
        assert torch.equal(alone.view(torch.int32), pooled.view(torch.int32)), "pooled differs without pointwise / from call to call"
    if batched:
        pb, ab = ops.voxel_encode(tp.view(batched[0], batched[1], C), tv, None, V, tW, tb, relu=relu, return_arg=True, **kw)
        assert torch.equal(pb.view(torch.int32), pooled.view(torch.int32)) and torch.equal(ab, arg)
    if compose:
        y = ops.PackedMLP([(W, b)], False, dev, 1 if relu else 0).rows(rows)
        comp, _ = ops.voxel_reduce(y, _t(vfe.member_p2v(p2v, off, V, T), dev), to, V, "max")
        _eqz(comp, vfe.pz(pooled.cpu().numpy()), "fused vs decorate -> PackedMLP.rows -> voxel_reduce(max)")
    return want_p, want_a, want_y, want_r


@pytest.fixture(scope="module")
def tiles():
    pts, off, par, counts = vfe.tiles_case()
    p2v, coors, count, _ = vr.voxel_index(pts, off, par["v"], par["r"], par["V"])
    have = set(count.reshape(-1).tolist())
    assert {0, 1, 2, 31, 32, 33, 63, 64, 65, 200} <= have
    rows, s_of, rank, start = vfe.members(p2v, off, par["V"])
    n = np.diff(start)
    assert ((n > 0) & (start[:-1] // 32 != (start[1:] - 1) // 32)).sum() >= 4        # voxels across a 32-row boundary
    assert ((n > 0) & (start[:-1] // 128 != (start[1:] - 1) // 128)).sum() >= 2      # ... and across a workgroup's four spans
    return pts, off, par, p2v, coors


def test_tiles(dev, orc, tiles):
    pts, off, par, p2v, coors = tiles
    for T in (None, 8):
        _check(dev, orc, pts, off, p2v, par["V"], 64, coors=coors, v=par["v"], r=par["r"], T=T)


@pytest.mark.parametrize("cout", [1, 31, 32, 33, 64, 128, 256])
def test_channels_out(dev, orc, tiles, cout):
    pts, off, par, p2v, coors = tiles
    _check(dev, orc, pts, off, p2v, par["V"], cout, coors=coors, v=par["v"], r=par["r"])


@pytest.mark.parametrize("C,cout", [(3, 33), (7, 33), (250, 32)])
def test_channels_in(dev, orc, tiles, C, cout):
    pts, off, par, p2v, coors = tiles
    _check(dev, orc, vc.with_channels(pts, C), off, p2v, par["V"], cout, coors=coors, v=par["v"], r=par["r"])


def test_one_column_no_decorations(dev, orc, tiles):
    pts, off, par, p2v, coors = tiles
    _check(dev, orc, np.ascontiguousarray(pts[:, 3:4]), off, p2v, par["V"], 33, cc=False, vc=False)


def test_cout_257_is_unsupported(dev, tiles):
    import torch
    from sad_amd import ops
    pts, off, par, p2v, coors = tiles
    W, b = _weights(4, 257)
    with pytest.raises(RuntimeError, match=r"\(-\d+\).*1 \.\. 256"):
        ops.voxel_encode(_t(pts, dev), _t(p2v, dev), _t(off, dev), par["V"], _t(W, dev), _t(b, dev), cluster_center=False,
                         voxel_center=False)
    torch.cuda.synchronize()


def test_flags(dev, orc, tiles):
    pts, off, par, p2v, coors = tiles
    V = par["V"]
    _check(dev, orc, pts, off, p2v, V, 33, cc=True, vc=False)
    _check(dev, orc, pts, off, p2v, V, 33, cc=False, vc=True, coors=coors, v=par["v"], r=par["r"])
    _check(dev, orc, pts, off, p2v, V, 33, relu=False, coors=coors, v=par["v"], r=par["r"])
    vf = np.random.default_rng(5).standard_normal((len(off) - 1, V, 16)).astype(F)
    _check(dev, orc, pts, off, p2v, V, 64, coors=coors, v=par["v"], r=par["r"], vox_feat=vf, T=8)
    _check(dev, orc, pts, off, p2v, V, 64, cc=False, vc=False, vox_feat=vf)


def test_negative_maxima_and_zero_tie(dev, orc):
    pts, off, par, p2v, W, b = vfe.signed_zero_case()
    pooled, arg, y, _ = _check(dev, orc, pts, off, p2v, par["V"], 2, relu=False, cc=False, vc=False, W=W, b=b)
    assert (pooled < 0).any() and np.signbit(y[y == 0]).any() and (~np.signbit(y[y == 0])).any()      # (see tests/test_vfe_cpu.py)


def test_family_pillars(dev, orc):
    (name, pts, off, par), = vc.family_pillars(4)
    p2v, coors, count, _ = vr.voxel_index(pts, off, par["v"], par["r"], par["V"])
    _check(dev, orc, pts, off, p2v, par["V"], 64, coors=coors, v=par["v"], r=par["r"], batched=(2, 16384))


def test_family_capped(dev, orc):
    (name, pts, off, par), = vc.family_capped(3)
    p2v, coors, count, _ = vr.voxel_index(pts, off, par["v"], par["r"], par["V"])
    assert (count > 8).any()
    _check(dev, orc, pts, off, p2v, par["V"], 64, coors=coors, v=par["v"], r=par["r"], T=8, batched=(2, 16384))


def test_family_degenerate(dev, orc):
    seen = set()
    for name, pts, off, par in vc.family_degenerate():
        p2v, coors, count, _ = vr.voxel_index(pts, off, par["v"], par["r"], par["V"])
        for T in (None, par["T"]):
            want_p, want_a, _, _ = _check(dev, orc, pts, off, p2v, par["V"], 32, coors=coors, v=par["v"], r=par["r"], T=T)
        if name.startswith("one_voxel"):
            assert count.max() == 4096
        if name == "all_out_of_range":
            assert (want_p == 0).all() and (want_a == -1).all()
        seen.add(name)
    assert {"one_voxel_T1", "one_voxel_T64", "all_out_of_range", "ragged_mix", "V1"} <= seen


def test_stack(dev, orc, tiles):
    import torch
    from sad_amd import PillarFeatureNet
    pts, off, par, p2v, coors = tiles
    V = par["V"]
    net = PillarFeatureNet(4, (32, 64), par["v"], par["r"]).to(dev)
    assert [tuple(w.shape) for w in net.weight] == [(16, 10), (64, 32)]
    with torch.no_grad():
        for l, w in enumerate(net.weight):
            W, b = _weights(w.shape[1], w.shape[0], l)
            w.copy_(_t(W, dev))
            net.bias[l].copy_(_t(b, dev))
        got = net(_t(pts, dev), _t(p2v, dev), _t(off, dev), _t(coors, dev))
    W0, b0 = net.weight[0].detach().cpu().numpy(), net.bias[0].detach().cpu().numpy()
    W1, b1 = net.weight[1].detach().cpu().numpy(), net.bias[1].detach().cpu().numpy()
    p0, _, y0, _ = vfe.encode(orc, pts, p2v, off, V, W0, b0, True, coors=coors, voxel_size=par["v"], point_range=par["r"])
    p1, _, _, rows1 = vfe.encode(orc, y0, p2v, off, V, W1, b1, True, cluster_center=False, voxel_center=False, vox_feat=p0)
    live = vfe.member_p2v(p2v, off, V) >= 0
    assert np.array_equal(rows1[live][:, :16], y0[live])                  # rows [y | max]
    _eqz(got, p1, "PillarFeatureNet(4, (32, 64))")


def _grads(dev, pts, off, p2v, V, W, b, gp, gpw, coors, v, r, cc, vc, vox_feat, T, relu=True):
    import torch
    from sad_amd import autograd
    tp = _t(pts, dev).requires_grad_(True)
    tW, tb = _t(W, dev).requires_grad_(True), _t(b, dev).requires_grad_(True)
    tf = None if vox_feat is None else _t(vox_feat, dev).requires_grad_(True)
    out = autograd.voxel_encode(tp, _t(p2v, dev), _t(off, dev), V, tW, tb, None if coors is None else _t(coors, dev), v, r, cc, vc, relu,
                                tf, T, gpw is not None)
    if gpw is not None:
        torch.autograd.backward(list(out), [_t(gp, dev), _t(gpw, dev)])
    else:
        out.backward(_t(gp, dev))
    g = dict(grad_points=tp.grad, grad_W=tW.grad, grad_bias=tb.grad)
    if tf is not None:
        g["grad_vox_feat"] = tf.grad
    return {k: x.cpu().numpy() for k, x in g.items()}


def _backward_case(dev, orc, pts, off, p2v, V, coors, v, r, T, seed):
    rng = np.random.default_rng(300 + seed)
    B, C, Cv, cout = len(off) - 1, pts.shape[1], 8, 33
    vox_feat = rng.standard_normal((B, V, Cv)).astype(F)
    W, b = _weights(C + 6 + Cv, cout, seed)
    pooled, arg, y, rows = vfe.encode(orc, pts, p2v, off, V, W, b, True, coors=coors, voxel_size=v, point_range=r, vox_feat=vox_feat, T=T)
    gp = rng.standard_normal(pooled.shape).astype(F)
    gpw = rng.standard_normal(y.shape).astype(F)
    mp = vfe.member_p2v(p2v, off, V, T)
    assert (y[mp >= 0] == 0).any() and (y[mp >= 0] > 0).any()               # the ReLU mask cuts some and passes some
    want = vfe.backward(rows, mp, off, V, W, y, arg, gp, gpw, True, C, 2, Cv)
    got = _grads(dev, pts, off, p2v, V, W, b, gp, gpw, coors, v, r, True, True, vox_feat, T)
    n_members = int(np.bincount(mp[mp >= 0]).max())
    terms = dict(grad_points=cout * 3 + 1, grad_vox_feat=(cout + 1) * n_members + 1, grad_W=len(pts) + 1, grad_bias=len(pts) + 1)
    for k, n in terms.items():
        err = np.abs(got[k].astype(np.float64) - want[k])
        bound = n * 2.0 ** -23 * want[k + "_abs"]
        print(k, "worst error / bound:", float((err / np.maximum(bound, 1e-300)).max()))
        assert (err <= bound).all(), f"{k}: {int((err > bound).sum())} entries outside n * 2^-23 * sum|terms| (n = {n})"


def test_backward_tiles(dev, orc, tiles):
    pts, off, par, p2v, coors = tiles
    for T in (None, 8):
        _backward_case(dev, orc, pts, off, p2v, par["V"], coors, par["v"], par["r"], T, 0)


def test_backward_pillars_scene(dev, orc):
    (name, pts, off, par), = vc.family_pillars(4)
    pts, off = pts[:16384], off[:2]
    p2v, coors, count, _ = vr.voxel_index(pts, off, par["v"], par["r"], par["V"])
    _backward_case(dev, orc, pts, off, p2v, par["V"], coors, par["v"], par["r"], None, 1)


def test_backward_exact_on_integers(dev, orc, tiles):
    """Exactly summable inputs (|g| <= 4, |row| <= 8, integer decorations): every gradient equals the float64 reference under
    ==.  The tiles family's point2voxel on a 4 x 4 grid of cells of size 2: all members of a voxel share one integer xyz (so the
    mean is that xyz and xyz - mean = 0), the centre of cell g is 2 g + 1, the fourth column and vox_feat are small integers."""
    _, off, par, p2v, _ = tiles
    rng = np.random.default_rng(9)
    V, B, total = par["V"], len(off) - 1, len(p2v)
    cell = np.arange(V)
    coors = np.stack([np.zeros(V, np.int32), cell // 4, cell % 4], 1).astype(np.int32)[None].repeat(B, 0)
    corner = rng.integers(0, 2, (B, V, 3))
    xyz_v = (2 * coors[..., ::-1] + corner).astype(F)
    sid = vr.scene_ids(off, total)
    pts = np.zeros((total, 4), F)
    live = p2v >= 0
    pts[live, :3] = xyz_v[sid[live], p2v[live]]
    pts[:, 3] = rng.integers(-8, 9, total)
    v, r = (2.0, 2.0, 2.0), (0, 0, 0, 8, 8, 2)
    Cv, cout = 4, 33
    vox_feat = rng.integers(-8, 9, (B, V, Cv)).astype(F)
    W = rng.integers(-2, 3, (cout, 14)).astype(F)
    b = rng.integers(-2, 3, cout).astype(F)
    pooled, arg, y, rows = vfe.encode(orc, pts, p2v, off, V, W, b, True, coors=coors, voxel_size=v, point_range=r, vox_feat=vox_feat)
    assert np.abs(rows).max() <= 8 and (rows == np.rint(rows)).all() and (rows[:, 4:7] == 0).all() and (rows[live][:, 7:10] != 0).any()
    gp = rng.integers(-4, 5, pooled.shape).astype(F)
    mp = vfe.member_p2v(p2v, off, V)
    want = vfe.backward(rows, mp, off, V, W, y, arg, gp, None, True, 4, 2, Cv)
    got = _grads(dev, pts, off, p2v, V, W, b, gp, None, coors, v, r, True, True, vox_feat, None)
    assert np.abs(want["g"]).max() <= 4 and (want["grad_W"] != 0).any()
    for k in ("grad_points", "grad_vox_feat", "grad_W", "grad_bias"):
        assert np.array_equal(got[k].astype(np.float64), want[k]), f"{k}: {int((got[k] != want[k]).sum())} entries differ"
