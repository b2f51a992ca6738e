"""GPU parity of the index kernels on the edge regimes of tests/edge_regimes.py (-m gpu): every regime through every kernel
that takes a pruning or an ordering decision, exact equality with the oracle (three_nn: with tests/interp_ref.py as well).
The scenes are where the pruning arguments get thin — a grid of ~25 000 cells along one axis, coordinates whose ulp is a few
per cent of the radius, points exactly on, one step inside and one step outside a ball, centroids outside the grid, subnormal
and overflowing squared distances, outliers, exhausted samplers.  tests/test_edge_regimes.py shows on the CPU that the cases
reach those regimes and that the oracle agrees with float32 numpy there."""
import numpy as np
import pytest

import edge_regimes as er
import interp_ref as ref

pytestmark = pytest.mark.gpu

F = np.float32
_want = {}


def _t(a, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _oracle(key, fn):
    """Oracle results are shared by the tests of a case (kernel variants, forced kernels)."""
    if key not in _want:
        _want[key] = fn()
    return _want[key]


def _want_bq(orc, c, r, s):
    return _oracle((c.name, "bq", r, s), lambda: orc.ball_query(r, s, c.xyz, c.new_xyz))


def _counts(c, r, s):
    d2 = _oracle((c.name, "d2"), lambda: er.d2_matrix(c.xyz[0], c.new_xyz[0]))
    with np.errstate(over="ignore"):
        r2 = F(r) * F(r)
    return np.minimum((d2 < r2).sum(-1), s).astype(np.int32)[None]


def _radii(c, n):
    """n radii (1-4) whose largest is the case's largest, so the grid keeps the case's geometry."""
    pairs = sorted(zip(c.radii, c.nsamples), reverse=True) + [(float(F(max(c.radii) * f)), s) for f, s in ((0.75, 24), (0.4, 7), (0.9, 48))]
    pairs = sorted(pairs[:n])
    return [p[0] for p in pairs], [p[1] for p in pairs]


# ---------------------------------------------------------------- fps
@pytest.mark.parametrize("cid", er.CASE_IDS)
def test_fps(orc, sad, dev, cid):
    """Default dispatch (cell buckets from 2 048 points, sorted records above 16 384) and every fps_variant 1-7."""
    from sad_amd import _lib, ops
    c = er.case(cid)
    want = _oracle((c.name, "fps"), lambda: orc.fps(c.xyz, c.npoint))
    variants = (0, 3, 4, 5, 6, 7) if c.npoint > 8192 else range(8)     # (the unbucketed forms walk 16 384 x 16 384 pairs there)
    x = _t(c.xyz, dev)
    try:
        for v in variants:
            _lib.set_option("fps_variant", v)
            np.testing.assert_array_equal(ops.fps(x, c.npoint).cpu().numpy(), want, err_msg=f"{c.name}: fps_variant {v}")
    finally:
        _lib.set_option("fps_variant", 0)


@pytest.mark.parametrize("make", [lambda: er.offset(70000, "cube", 1e5), lambda: er.outlier(70000, 2)], ids=["offset", "outlier"])
def test_fps_above_65536(orc, sad, dev, make):
    """Beyond the record kernel's 65 536 points: the global-workspace kernel."""
    from sad_amd import ops
    c = make()
    np.testing.assert_array_equal(ops.fps(_t(c.xyz, dev), 200).cpu().numpy(), orc.fps(c.xyz, 200))


@pytest.mark.parametrize("cid", er.ids("offset")[:3] + er.ids("tiny", "huge"))
def test_ffps(orc, sad, dev, cid):
    """Feature-distance FPS, w_xyz = 1, features in the regime of the coordinates."""
    from sad_amd import ops
    c = er.case(cid)
    assert c.N <= 4096
    feat = np.concatenate([c.xyz[:, ::-1, :], c.xyz[:, np.arange(c.N) * 7 % c.N, :1]], -1).astype(F)
    want = orc.ffps(c.xyz, feat, 64, 1.0)
    np.testing.assert_array_equal(ops.ffps(_t(c.xyz, dev), _t(feat, dev), 64, 1.0).cpu().numpy(), want)


# ---------------------------------------------------------------- ball query
@pytest.mark.parametrize("variant", [0, 1, 2])
@pytest.mark.parametrize("cid", [c for c in er.CASE_IDS if not c.startswith("exhaust")])
def test_ball_query_grid(orc, sad, dev, cid, variant):
    """The grid kernel (N >= 2 048; below, the same call takes the scan kernel), 1-4 radii, indices and counts.  bq_variant 1 sends
    every centroid through the bitmap path, 2 is the one-bitmap-set layout."""
    from sad_amd import _lib, ops
    c = er.case(cid)
    x, q = _t(c.xyz, dev), _t(c.new_xyz, dev)
    _lib.set_option("bq_variant", variant)
    try:
        for n in ((1, 2, 3, 4) if variant == 0 else (len(c.radii), 4)):
            radii, ns = _radii(c, n)
            assert max(radii) == max(c.radii)
            idxs, cnts = ops.ball_query_multi(radii, ns, x, q, return_counts=True)
            for r, s, gi, gc in zip(radii, ns, idxs, cnts):
                want = _want_bq(orc, c, r, s)
                got = gi.cpu().numpy()
                if not np.array_equal(got, want):
                    m = int(np.flatnonzero((got != want).any(-1)[0])[0])
                    raise AssertionError(f"{c.name}, bq_variant {variant}, {n} radii, r = {r!r}, S = {s}: first differing centroid "
                                         f"{m} at {c.new_xyz[0, m].tolist()}\noracle {want[0, m].tolist()}\nkernel {got[0, m].tolist()}")
                np.testing.assert_array_equal(gc.cpu().numpy(), _oracle((c.name, "cnt", r, s), lambda: _counts(c, r, s)))
    finally:
        _lib.set_option("bq_variant", 0)


@pytest.mark.parametrize("cid", [c for c in er.CASE_IDS if not c.startswith("exhaust")])
def test_ball_query_scan_forced(orc, sad, dev, cid):
    from sad_amd import ops
    c = er.case(cid)
    radii, ns = _radii(c, 3)
    old, ops.GRID_MIN_POINTS = ops.GRID_MIN_POINTS, 1 << 30
    try:
        idxs, cnts = ops.ball_query_multi(radii, ns, _t(c.xyz, dev), _t(c.new_xyz, dev), return_counts=True)
    finally:
        ops.GRID_MIN_POINTS = old
    for r, s, gi, gc in zip(radii, ns, idxs, cnts):
        np.testing.assert_array_equal(gi.cpu().numpy(), _want_bq(orc, c, r, s), err_msg=f"{c.name}: r = {r!r}")
        np.testing.assert_array_equal(gc.cpu().numpy(), _oracle((c.name, "cnt", r, s), lambda: _counts(c, r, s)))


@pytest.mark.parametrize("cid", er.ids("offset", "tiny", "shell"))
def test_ball_query_per_centroid_radii(orc, sad, dev, cid):
    """radius[b,m] = radii[r] * pc[b,m] through the scan kernel; pc is a power of two, so `shell` keeps its exact r^2."""
    from sad_amd import ops
    c = er.case(cid)
    pc = np.array([0.5, 1.0, 2.0, 1.0], F)[np.arange(c.M) % 4][None]
    idxs = ops.ball_query_multi(c.radii, c.nsamples, _t(c.xyz, dev), _t(c.new_xyz, dev), _t(pc, dev))
    for r, s, gi in zip(c.radii, c.nsamples, idxs):
        rad = (F(r) * pc).astype(F)
        np.testing.assert_array_equal(gi.cpu().numpy(), orc.ball_query(rad, s, c.xyz, c.new_xyz), err_msg=f"{c.name}: r = {r!r}")
        got1 = ops.ball_query(_t(rad, dev), s, _t(c.xyz, dev), _t(c.new_xyz, dev)).cpu().numpy()
        np.testing.assert_array_equal(got1, orc.ball_query(rad, s, c.xyz, c.new_xyz))


# ---------------------------------------------------------------- nearest neighbours
@pytest.mark.parametrize("cid", er.CASE_IDS)
def test_knn(orc, sad, dev, cid):
    from sad_amd import ops
    c = er.case(cid)
    q = np.ascontiguousarray(c.new_xyz[:, :128])
    for k in (1, 3, 64):
        np.testing.assert_array_equal(ops.knn_query(k, _t(c.xyz, dev), _t(q, dev)).cpu().numpy(), orc.knn_query(k, c.xyz, q),
                                      err_msg=f"{c.name}: k = {k}")


@pytest.mark.parametrize("cid", er.CASE_IDS)
def test_three_nn(orc, sad, dev, cid):
    """Indices and squared distances bit for bit (the reference and the oracle's 3-NN agree first); the weights too, except on
    `tiny` and `huge`: there 1 / (sqrt(d2) + 1e-8) is 1e8 for every neighbour or 0 for an infinite d2, so the weights say
    nothing about the selection and only indices and distances are compared.  (SPEC §18 leaves an overflowing d2 undefined; every
    query point of `huge` has three neighbours at a finite d2, asserted below, and those are what is compared.)"""
    from sad_amd import _lib, ops
    c = er.case(cid)
    q = np.ascontiguousarray(c.new_xyz[:, :128])
    with np.errstate(over="ignore"):
        want_d, want_i, want_w = ref.three_nn(q, c.xyz)
    assert np.isfinite(want_d).all(), "three finite neighbours everywhere (the reference's masking needs them)"
    np.testing.assert_array_equal(want_i, orc.knn_query(3, c.xyz, q))
    try:
        for variant in (0, 1, 2):
            _lib.set_option("nn_variant", variant)
            d, i, w = ops.three_nn(_t(q, dev), _t(c.xyz, dev))
            np.testing.assert_array_equal(i.cpu().numpy(), want_i, err_msg=f"{c.name}: idx, nn_variant {variant}")
            np.testing.assert_array_equal(d.cpu().numpy(), want_d, err_msg=f"{c.name}: dist2, nn_variant {variant}")
            if not cid.startswith(("tiny", "huge")):
                np.testing.assert_array_equal(w.cpu().numpy(), want_w, err_msg=f"{c.name}: w, nn_variant {variant}")
    finally:
        _lib.set_option("nn_variant", 0)
