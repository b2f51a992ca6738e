"""GPU parity of feature propagation (SPEC.md §18) (-m gpu): three_nn (distances, indices and weights bit-equal to the numpy
reference, every kernel form), three_interpolate (bit-equal, both layouts, column slices), its backward (§16 tolerance) and
FPModule (bit-equal to the oracle's plain-row chain on the reference's concatenated rows)."""
import numpy as np
import pytest

import interp_ref as ref

pytestmark = pytest.mark.gpu


def _t(a, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _scene(kind, B, n, m, seed):
    rng = np.random.default_rng(seed)
    if kind == "lattice":
        unk = (rng.integers(0, 8, (B, n, 3)) * 0.5).astype(np.float32)
        kn = (rng.integers(0, 8, (B, m, 3)) * 0.5).astype(np.float32)
    else:
        unk = (rng.random((B, n, 3), dtype=np.float32) * 10).astype(np.float32)
        kn = (rng.random((B, m, 3), dtype=np.float32) * 10).astype(np.float32)
    if kind in ("lattice", "dups") and m > 4:
        kn[:, 3] = kn[:, 1]                                   # duplicate known points
        kn[:, m - 1] = kn[:, 0]
        k = min(n, m) // 2
        unk[:, :k] = kn[:, :k]                                # unknowns that coincide with known points
    return unk, kn


NN_CASES = [("random", 2, 1000, 300), ("lattice", 2, 777, 200), ("dups", 1, 513, 129), ("lattice", 1, 100, 1),
            ("lattice", 2, 65, 2), ("random", 1, 130, 3), ("lattice", 2, 1337, 1029), ("random", 3, 257, 2050),
            ("random", 2, 16384, 4096)]


@pytest.mark.parametrize("kind,B,n,m", NN_CASES)
def test_three_nn_bit_exact(sad, dev, kind, B, n, m):
    from sad_amd import _lib, ops
    unk, kn = _scene(kind, B, n, m, n + m)
    want_d, want_i, want_w = ref.three_nn(unk, kn)
    try:
        for variant in (0, 1, 2):                             # LDS, one point per lane (default); scalar loads; LDS, two points
            _lib.set_option("nn_variant", variant)
            d, i, w = ops.three_nn(_t(unk, dev), _t(kn, dev))
            np.testing.assert_array_equal(i.cpu().numpy(), want_i, err_msg=f"idx, nn_variant {variant}")
            np.testing.assert_array_equal(d.cpu().numpy(), want_d, err_msg=f"dist2, nn_variant {variant}")
            np.testing.assert_array_equal(w.cpu().numpy(), want_w, err_msg=f"w, nn_variant {variant}")
    finally:
        _lib.set_option("nn_variant", 0)


def _interp_inputs(B, n, m, C, seed):
    rng = np.random.default_rng(seed)
    feat_pm = rng.standard_normal((B, m, C)).astype(np.float32)
    idx = rng.integers(0, m, (B, n, 3)).astype(np.int32)
    w = rng.random((B, n, 3), dtype=np.float32)               # caller-made weights (not normalised)
    return feat_pm, idx, w


@pytest.mark.parametrize("B,n,m,C", [(2, 300, 77, 5), (2, 1000, 129, 64), (1, 4097, 1000, 128), (3, 33, 4, 1)])
def test_three_interpolate_bit_exact(sad, dev, B, n, m, C):
    from sad_amd import ops
    feat_pm, idx, w = _interp_inputs(B, n, m, C, n + C)
    want = ref.three_interpolate_pm(feat_pm, idx, w)
    got_pm = ops.three_interpolate(_t(feat_pm, dev), _t(idx, dev), _t(w, dev), point_major=True).cpu().numpy()
    np.testing.assert_array_equal(got_pm, want)
    got_cm = ops.three_interpolate(_t(feat_pm.transpose(0, 2, 1), dev), _t(idx, dev), _t(w, dev)).cpu().numpy()
    np.testing.assert_array_equal(got_cm, want.transpose(0, 2, 1))


@pytest.mark.parametrize("C,col_off,extra", [(64, 4, 8), (64, 3, 5), (7, 2, 3)])
def test_three_interpolate_column_slice(sad, dev, C, col_off, extra):
    from sad_amd import ops
    B, n, m = 2, 500, 90
    feat_pm, idx, w = _interp_inputs(B, n, m, C, C + col_off)
    want = ref.three_interpolate_pm(feat_pm, idx, w)
    ld = C + extra
    fill = np.random.default_rng(1).standard_normal((B, n, ld)).astype(np.float32)
    out = _t(fill, dev)
    r = ops.three_interpolate(_t(feat_pm, dev), _t(idx, dev), _t(w, dev), point_major=True, out=out, col_off=col_off)
    assert r is out
    got = out.cpu().numpy()
    np.testing.assert_array_equal(got[..., col_off:col_off + C], want)
    np.testing.assert_array_equal(got[..., :col_off], fill[..., :col_off])
    np.testing.assert_array_equal(got[..., col_off + C:], fill[..., col_off + C:])
    with pytest.raises(RuntimeError, match="col_off"):
        ops.three_interpolate(_t(feat_pm, dev), _t(idx, dev), _t(w, dev), point_major=True, out=out, col_off=extra + 1)


@pytest.mark.parametrize("B,n,m,C", [(2, 300, 77, 5), (1, 2000, 100, 128), (2, 4096, 1024, 64)])
def test_three_interpolate_grad(sad, dev, B, n, m, C):
    from sad_amd import autograd as ag
    rng = np.random.default_rng(B * n + C)
    unk, kn = _scene("random", B, n, m, C)
    _, idx, w = ref.three_nn(unk, kn)                         # realistic: many unknowns share known points
    g_pm = rng.standard_normal((B, n, C)).astype(np.float32)
    want, mag = ref.three_interpolate_grad_pm(g_pm, idx, w, m)
    tol = 1e-5 * mag + 1e-30
    got_pm = ag.three_interpolate_grad(_t(g_pm, dev), _t(idx, dev), _t(w, dev), m, point_major=True).cpu().numpy()
    assert np.all(np.abs(got_pm - want) <= tol)
    got_cm = ag.three_interpolate_grad(_t(g_pm.transpose(0, 2, 1), dev), _t(idx, dev), _t(w, dev), m).cpu().numpy()
    assert np.all(np.abs(got_cm.transpose(0, 2, 1) - want) <= tol)
    # autograd, both layouts: forward exact, gradient for the features only
    for pm in (False, True):
        f_pm = rng.standard_normal((B, m, C)).astype(np.float32)
        f = _t(f_pm if pm else f_pm.transpose(0, 2, 1), dev).requires_grad_(True)
        out = ag.three_interpolate(f, _t(idx, dev), _t(w, dev), pm)
        y = out.detach().cpu().numpy()
        np.testing.assert_array_equal(y if pm else y.transpose(0, 2, 1), ref.three_interpolate_pm(f_pm, idx, w))
        out.backward(_t(g_pm if pm else g_pm.transpose(0, 2, 1), dev))
        got = f.grad.cpu().numpy()
        assert np.all(np.abs((got if pm else got.transpose(0, 2, 1)) - want) <= tol), f"autograd point_major={pm}"


@pytest.mark.parametrize("B,n,m,C1,C2,mlp", [(2, 1024, 256, 64, 128, (128, 128)), (2, 700, 129, 0, 96, (64, 64, 32)),
                                              (1, 2048, 512, 3, 64, (128,))])
def test_fp_module_bit_exact(orc, sad, dev, B, n, m, C1, C2, mlp):
    from sad_amd.fp_module import FPModule
    rng = np.random.default_rng(n + C1)
    unk, kn = _scene("random", B, n, m, n)
    kf = rng.standard_normal((B, m, C2)).astype(np.float32)
    sk = rng.standard_normal((B, n, C1)).astype(np.float32) if C1 else None
    mod = FPModule(C2, C1, mlp, dev, seed=3)
    _, idx, w = ref.three_nn(unk, kn)
    rows = ref.three_interpolate_pm(kf, idx, w)
    if C1:
        rows = np.concatenate([rows, sk], axis=2)
    want = orc.mlp_rows(np.ascontiguousarray(rows.reshape(B * n, C1 + C2)), mod.weights).reshape(B, n, -1)
    got_pm = mod.forward_pm(_t(unk, dev), _t(kn, dev), _t(sk, dev) if C1 else None, _t(kf, dev)).cpu().numpy()
    np.testing.assert_array_equal(got_pm, want)
    got = mod(_t(unk, dev), _t(kn, dev), _t(sk.transpose(0, 2, 1), dev) if C1 else None,
              _t(kf.transpose(0, 2, 1), dev)).cpu().numpy()
    np.testing.assert_array_equal(got, want.transpose(0, 2, 1))


def _edge_inputs(B, n, m, C, seed):
    """Slots outside [0, m) (-1, m, 2^31 - 1; about a third, some points with all three), weights and gradient entries that are
    exactly 0, and one known point (0) that no valid slot names."""
    rng = np.random.default_rng(seed)
    feat_pm = rng.standard_normal((B, m, C)).astype(np.float32)
    idx = rng.integers(1, m, (B, n, 3)).astype(np.int32)
    bad = rng.random((B, n, 3)) < 0.3
    bad[:, ::9] = True
    idx[bad] = rng.choice(np.array([-1, m, 2 ** 31 - 1], np.int32), int(bad.sum()))
    w = rng.random((B, n, 3), dtype=np.float32)
    w[rng.random((B, n, 3)) < 0.2] = 0.0
    g_pm = rng.standard_normal((B, n, C)).astype(np.float32)
    g_pm[rng.random((B, n, C)) < 0.2] = 0.0
    ok = ref.in_range(idx, m)
    assert not ok.all(2).all() and ok.any() and (w[~ok] != 0).any() and (w[ok] == 0).any() and {-1, m, 2 ** 31 - 1} <= set(idx[~ok].tolist())
    return feat_pm, idx, w, g_pm


@pytest.mark.parametrize("C", [4, 5, 64, 65])                   # point-major: 16-byte chunks (C % 4 == 0) / one channel per thread
@pytest.mark.parametrize("n", [63, 64, 65])                     # around the 64-point tile of the channel-major gradient
def test_three_interpolate_out_of_range_slots(sad, dev, n, C):
    """An index outside [0, m) reads a zero feature and receives no gradient (interp.hip's ``(unsigned)j >= m`` branches), the
    gradient skips g == 0 and w * g == 0: forward bit-equal to the reference, gradient within the rule of
    test_three_interpolate_grad of the float64 sum without those slots, exactly 0 for known points no valid slot names."""
    from sad_amd import ops
    B, m = 2, 5
    feat_pm, idx, w, g_pm = _edge_inputs(B, n, m, C, 100 * n + C)
    want = ref.three_interpolate_pm(feat_pm, idx, w)
    ti, tw = _t(idx, dev), _t(w, dev)
    np.testing.assert_array_equal(ops.three_interpolate(_t(feat_pm, dev), ti, tw, point_major=True).cpu().numpy(), want)
    np.testing.assert_array_equal(ops.three_interpolate(_t(feat_pm.transpose(0, 2, 1), dev), ti, tw).cpu().numpy(), want.transpose(0, 2, 1))
    if C % 4 == 0:                                               # the same width through the one-channel form: a slice at an odd column
        out = _t(np.full((B, n, C + 3), np.nan, np.float32), dev)
        ops.three_interpolate(_t(feat_pm, dev), ti, tw, point_major=True, out=out, col_off=1)
        np.testing.assert_array_equal(out[..., 1:1 + C].cpu().numpy(), want)
    gwant, mag = ref.three_interpolate_grad_pm(g_pm, idx, w, m)
    tol = 1e-5 * mag + 1e-30
    named = np.zeros((B, m), bool)
    for b in range(B):
        named[b, idx[b][ref.in_range(idx[b], m)]] = True
    assert not named[:, 0].any() and named[:, 1:].all()
    got_pm = ops.three_interpolate_grad(_t(g_pm, dev), ti, tw, m, point_major=True).cpu().numpy()
    got_cm = ops.three_interpolate_grad(_t(g_pm.transpose(0, 2, 1), dev), ti, tw, m).cpu().numpy().transpose(0, 2, 1)
    for name, got in (("point-major", got_pm), ("channel-major", got_cm)):
        assert np.all(np.abs(got - gwant) <= tol), name
        assert (got[~named] == 0).all(), f"{name}: gradient at a known point that no valid slot names"
