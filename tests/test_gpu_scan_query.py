"""GPU parity of the scan ball query `ball_query_kernel` (-m gpu): the LDS-staged form (N <= 2 048) at the sizes where its staging,
its chunk walk and its widest-radius gate can go wrong, and the global-memory form above.  Every case compares every slot of `idx`
(padding included) and `cnt` with the oracle for exact equality."""
import numpy as np
import pytest

import edge_regimes as er

pytestmark = pytest.mark.gpu

F = np.float32
UNSORTED = (3.2, 1.6, 4.8)


def _t(a, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _scene(seed, B, N, M, span=10.0):
    rng = np.random.default_rng(seed)
    xyz = (rng.random((B, N, 3)) * span).astype(F)
    new_xyz = (rng.random((B, M, 3)) * span).astype(F)
    return xyz, new_xyz


def _check(orc, dev, xyz, new_xyz, radii, ns, pc=None, tag=""):
    """The scan kernel (the grid kernel is switched off for the call) against the oracle: idx of every radius, and cnt."""
    from sad_amd import ops
    old, ops.GRID_MIN_POINTS = ops.GRID_MIN_POINTS, 1 << 30
    try:
        idxs, cnts = ops.ball_query_multi(radii, ns, _t(xyz, dev), _t(new_xyz, dev), None if pc is None else _t(pc, dev),
                                          return_counts=True)
    finally:
        ops.GRID_MIN_POINTS = old
    B, M = new_xyz.shape[:2]
    for r, s, gi, gc in zip(radii, ns, idxs, cnts):
        with np.errstate(over="ignore", invalid="ignore"):
            rad = np.full((B, M), F(r), F) if pc is None else (F(r) * pc).astype(F)
            r2 = rad * rad
        want = orc.ball_query(F(r) if pc is None else rad, s, xyz, new_xyz)
        got = gi.cpu().numpy()
        if not np.array_equal(got, want):
            b, m = np.argwhere((got != want).any(-1))[0]
            raise AssertionError(f"{tag} r = {r!r}, S = {s}: first differing centroid ({b}, {m})\noracle {want[b, m].tolist()}\n"
                                 f"kernel {got[b, m].tolist()}")
        with np.errstate(invalid="ignore"):
            n = np.stack([(er.d2_matrix(xyz[b], new_xyz[b]) < r2[b][:, None]).sum(-1) for b in range(B)])
        np.testing.assert_array_equal(gc.cpu().numpy(), np.minimum(n, s).astype(np.int32), err_msg=f"{tag} cnt, r = {r!r}, S = {s}")


@pytest.mark.parametrize("N,M", [(1, 1), (1, 5), (63, 5), (63, 33), (64, 31), (64, 1), (65, 33), (65, 5), (1000, 31), (1000, 33),
                                 (1024, 5), (1024, 33), (2047, 31), (2047, 1), (2048, 33), (2048, 5), (65, 15), (1000, 17), (64, 16), (2048, 17)])
def test_staged_sizes(orc, sad, dev, N, M):
    """N at the chunk edges and at the staging limit, M with a ragged last wave (two centroids per wave) and ragged 16-centroid
    workgroups (15, 16, 17 sit on that edge; 31 and 33 on the next), B = 2; unsorted radii, nsample 1 / 16 / 64; scalar radii
    and per-centroid radii."""
    xyz, new_xyz = _scene(N * 100 + M, 2, N, M)
    pc = np.array([0.5, 1.0, 2.0, 1.25, 0.75], F)[np.arange(2 * M) % 5].reshape(2, M)
    _check(orc, dev, xyz, new_xyz, UNSORTED, (16, 1, 64), tag=f"N={N} M={M}")
    _check(orc, dev, xyz, new_xyz, UNSORTED, (64, 16, 1), pc, tag=f"N={N} M={M} pc")


@pytest.mark.parametrize("n_radii", [1, 2, 3, 4])
def test_radius_counts(orc, sad, dev, n_radii):
    """Every instantiation of the staged form (1-4 radii) on one ragged scene."""
    xyz, new_xyz = _scene(7, 2, 333, 37)
    _check(orc, dev, xyz, new_xyz, (3.2, 1.6, 4.8, 2.4)[:n_radii], (16, 64, 1, 32)[:n_radii], tag=f"{n_radii} radii")


def test_fallback_above_staging_limit(orc, sad, dev):
    """N = 2 049 with per-centroid radii: the form that reads global memory."""
    xyz, new_xyz = _scene(11, 2, 2049, 33)
    pc = np.array([0.5, 1.0, 2.0], F)[np.arange(66) % 3].reshape(2, 33)
    _check(orc, dev, xyz, new_xyz, UNSORTED, (16, 1, 64), pc, tag="N=2049")
    _check(orc, dev, xyz, new_xyz, (1.6, 4.8), (64, 16), pc, tag="N=2049, two radii")


@pytest.mark.parametrize("pattern", ["all", "even", "63+1"])
@pytest.mark.parametrize("ns", [(1, 16, 64), (64, 64, 16), (16, 1, 1)])
def test_caps_and_empty_radius(orc, sad, dev, pattern, ns):
    """Near points at the origin, far points at 1 000.  `all`: the cap of 16 is reached inside chunk 0 and the cap of 64 exactly at
    its end; `even`: the 64th accepted point is index 126, the 16th is 30; `63+1`: 63 accepted in chunk 0, the 64th is the first
    lane of chunk 2.  Radii (2, 0, 2): two equal radii and one that accepts nothing.  Centroid 0 sits on the near points and
    fills while its wave neighbour 1 sits on the far points, 2 sees nothing, 3 is a copy of 0 (M = 6: three waves of two)."""
    N = 200
    j = np.arange(N)
    near = {"all": np.ones(N, bool), "even": j % 2 == 0, "63+1": (j < 63) | (j == 128) | (j > 190)}[pattern]
    xyz = np.repeat(np.where(near, 0.0, 1000.0).astype(F) + (j % 7).astype(F) * F(0.125), 3).reshape(N, 3)
    xyz = np.stack([xyz, xyz[::-1]])
    new_xyz = np.array([[0, 0, 0], [1000, 1000, 1000], [500, 500, 500], [0, 0, 0], [1000.5, 1000.5, 1000.5], [0.25, 0.25, 0.25]], F)
    new_xyz = np.stack([new_xyz, new_xyz[::-1]])
    _check(orc, dev, xyz, new_xyz, (2.0, 0.0, 2.0), ns, tag=f"{pattern} {ns}")


def test_radius_pc_zero_nan_huge(orc, sad, dev):
    """Single rows of radius_pc hold 0, a NaN and a value whose square overflows: nothing, nothing, everything."""
    xyz, new_xyz = _scene(3, 2, 300, 9)
    pc = np.ones((2, 9), F)
    pc[0, 1], pc[0, 2], pc[0, 6] = 0.0, np.nan, 1e30
    pc[1, 0], pc[1, 4], pc[1, 8] = 1e30, 0.0, np.nan
    _check(orc, dev, xyz, new_xyz, UNSORTED, (16, 64, 1), pc, tag="pc 0/NaN/huge")
    _check(orc, dev, xyz, new_xyz, (1.0,), (64,), pc, tag="pc 0/NaN/huge, one radius")


def test_duplicates_and_exact_ties(orc, sad, dev):
    """The integer lattice [-3, 3]^3, every point twice: d2 is an exact small integer, so points at d2 == r2 (9 and 25 from the
    centroids used) are exact ties and stay outside (strict test), and duplicates come in index order."""
    g = np.arange(-3, 4)
    lat = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3).astype(F)
    rng = np.random.default_rng(5)
    xyz = np.stack([np.concatenate([lat, lat])[rng.permutation(686)] for _ in range(2)])
    new_xyz = np.array([[0, 0, 0], [1, 0, 0], [-3, -3, -3], [0, 1, -1], [3, 3, 3]], F)
    new_xyz = np.stack([new_xyz, new_xyz[::-1]])
    d2 = er.d2_matrix(xyz[0], new_xyz[0])
    assert (d2 == 9).any() and (d2 == 25).any() and (d2 == 1).any()
    _check(orc, dev, xyz, new_xyz, (3.0, 5.0, 1.0), (64, 16, 64), tag="lattice")
    _check(orc, dev, xyz, new_xyz, (5.0, 3.0), (64, 64), np.ones((2, 5), F), tag="lattice pc")

