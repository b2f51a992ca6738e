"""CPU checks of feature propagation (SPEC.md §18): the numpy reference the GPU tests use, and the host-side argument errors
of the three C entry points (nothing is launched)."""
import ctypes

import numpy as np
import pytest

import interp_ref as ref


def _scene(rng, B, n, m, lattice=False):
    if lattice:       # half-unit lattice: many exactly equal distances
        return (rng.integers(0, 6, (B, n, 3)) * 0.5).astype(np.float32), (rng.integers(0, 6, (B, m, 3)) * 0.5).astype(np.float32)
    return rng.random((B, n, 3), dtype=np.float32), rng.random((B, m, 3), dtype=np.float32)


def test_reference_distances_match_kdtree():
    from scipy.spatial import cKDTree
    rng = np.random.default_rng(0)
    unk, kn = _scene(rng, 2, 300, 77)
    dist, idx, w = ref.three_nn(unk, kn)
    for b in range(2):
        dd, _ = cKDTree(kn[b].astype(np.float64)).query(unk[b].astype(np.float64), k=3)
        np.testing.assert_allclose(np.sqrt(dist[b].astype(np.float64)), dd, rtol=1e-5, atol=1e-6)
    assert np.all(np.diff(dist, axis=2) >= 0)
    np.testing.assert_allclose(w.sum(-1), 1.0, rtol=1e-6)


@pytest.mark.parametrize("B,n,m,lattice", [(2, 200, 50, True), (1, 129, 3, True), (1, 64, 2, False), (2, 40, 1, True),
                                           (1, 150, 70, False)])
def test_reference_indices_match_lexsort(B, n, m, lattice):
    rng = np.random.default_rng(n + m)
    unk, kn = _scene(rng, B, n, m, lattice)
    if lattice and m > 3:
        kn[:, 1] = kn[:, 0]                       # duplicate known points
        unk[:, :5] = kn[:, :5]                    # unknowns that coincide with known points
    dist, idx, w = ref.three_nn(unk, kn)
    d2, i2 = ref.three_nn_lexsort(unk, kn)
    np.testing.assert_array_equal(idx, i2)
    np.testing.assert_array_equal(dist, d2)
    if m < 3:
        assert np.all(np.isinf(dist[..., m:])) and np.all(idx[..., m:] == 0) and np.all(w[..., m:] == 0)
    if m == 1:
        np.testing.assert_array_equal(w, np.broadcast_to(np.array([1, 0, 0], np.float32), w.shape))


def test_reference_weights_follow_the_spec_order():
    d = np.array([[[0.0, 1.0, 4.0], [2.25, np.inf, np.inf]]], np.float32)
    w = ref.weights(d)
    r = np.float32(1) / (np.sqrt(np.float32(0.0)) + np.float32(1e-8))
    r1, r2 = np.float32(1) / (np.float32(1) + np.float32(1e-8)), np.float32(1) / (np.float32(2) + np.float32(1e-8))
    norm = (r + r1) + r2
    np.testing.assert_array_equal(w[0, 0], np.array([r / norm, r1 / norm, r2 / norm], np.float32))
    np.testing.assert_array_equal(w[0, 1], np.array([1, 0, 0], np.float32))


def test_reference_out_of_range_slots_read_a_zero_feature():
    """A slot outside [0, m) is a slot that names an extra known point whose features are 0 (forward: the same bits; gradient:
    the same sums on the m real points); in range the reference is the plain gather it was."""
    rng = np.random.default_rng(3)
    B, n, m, C = 2, 65, 5, 5
    feat = rng.standard_normal((B, m, C)).astype(np.float32)
    idx = rng.integers(0, m, (B, n, 3)).astype(np.int32)
    w = rng.random((B, n, 3), dtype=np.float32)
    g = rng.standard_normal((B, n, C)).astype(np.float32)
    plain = np.stack([(w[b, :, 0:1] * feat[b][idx[b, :, 0]] + w[b, :, 1:2] * feat[b][idx[b, :, 1]]) + w[b, :, 2:3] * feat[b][idx[b, :, 2]]
                      for b in range(B)])
    np.testing.assert_array_equal(ref.three_interpolate_pm(feat, idx, w), plain)
    bad = idx.copy()
    sel = rng.random(idx.shape) < 0.3
    bad[sel] = rng.choice(np.array([-1, m, 2 ** 31 - 1, -2 ** 31], np.int32), int(sel.sum()))
    assert not ref.in_range(bad, m)[sel].any() and ref.in_range(bad, m)[~sel].all()
    ext = np.concatenate([feat, np.zeros((B, 1, C), np.float32)], 1)
    to_ext = np.where(sel, m, idx).astype(np.int32)
    np.testing.assert_array_equal(ref.three_interpolate_pm(feat, bad, w), ref.three_interpolate_pm(ext, to_ext, w))
    got, mag = ref.three_interpolate_grad_pm(g, bad, w, m)
    want, wmag = ref.three_interpolate_grad_pm(g, to_ext, w, m + 1)
    np.testing.assert_array_equal(got, want[:, :m])
    np.testing.assert_array_equal(mag, wmag[:, :m])


def test_host_side_argument_errors(sad):
    from sad_amd import _lib
    L = _lib.lib()
    p = 0x10000                                           # never dereferenced: every call below fails on the host
    assert L.sad_three_nn_f32(None, p, 1, 8, 4, p, p, None, None) == -1 and b"NULL" in L.sad_last_error()
    assert L.sad_three_nn_f32(p, p, 1, 8, 4, None, p, None, None) == -1 and b"NULL" in L.sad_last_error()
    assert L.sad_three_nn_f32(p, p, 1, 8, 0, p, p, None, None) == -1 and b"m must be >= 1" in L.sad_last_error()
    assert L.sad_three_interpolate_f32(p, None, p, 1, 4, 8, 16, 0, p, 16, 0, None) == -1 and b"NULL" in L.sad_last_error()
    assert L.sad_three_interpolate_f32(p, p, p, 1, 4, 0, 16, 0, p, 16, 0, None) == -1 and b"m must be >= 1" in L.sad_last_error()
    assert L.sad_three_interpolate_f32(p, p, p, 1, 4, 8, 16, 2, p, 16, 0, None) == -1 and b"layout" in L.sad_last_error()
    assert L.sad_three_interpolate_f32(p, p, p, 1, 4, 8, 16, 0, p, 16, 4, None) == -1 and b"col_off" in L.sad_last_error()
    assert L.sad_three_interpolate_f32(p, p, p, 1, 4, 8, 16, 0, p, 20, 0, None) == -1 and b"ld_out" in L.sad_last_error()
    assert L.sad_three_interpolate_f32(p, p, p, 1, 4, 8, 16, 1, p, 6, 4, None) == -1 and b"col_off" in L.sad_last_error()
    assert L.sad_three_interpolate_f32(p, p, p, 1, 4, 8, 16, 1, p, 8, -1, None) == -1 and b"col_off" in L.sad_last_error()
    assert L.sad_three_interpolate_grad_f32(p, p, None, 1, 4, 16, 8, 1, p, None) == -1 and b"NULL" in L.sad_last_error()
    assert L.sad_three_interpolate_grad_f32(p, p, p, 1, 4, 16, 0, 1, p, None) == -1 and b"m must be >= 1" in L.sad_last_error()
    assert L.sad_three_interpolate_grad_f32(p, p, p, 1, 4, 16, 8, -1, p, None) == -1 and b"layout" in L.sad_last_error()
    assert L.sad_set_option(b"nn_variant", 0) == 0


def test_python_surface_refuses_cpu_tensors(sad):
    import torch
    from sad_amd import ops
    x = torch.zeros(1, 16, 3)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.three_nn(x, x)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.three_interpolate(torch.zeros(1, 2, 16), torch.zeros(1, 16, 3, dtype=torch.int32), x)


def test_lazy_exports(sad):
    import sad_amd
    from sad_amd import fp_module, ops
    assert sad_amd.three_nn is ops.three_nn and sad_amd.three_interpolate is ops.three_interpolate
    assert sad_amd.FPModule is fp_module.FPModule
