"""The reference of the voxel feature encoder (SPEC.md §24, tests/vfe_ref.py) against itself and against torch, on the CPU:
the loop form equals the vectorised form, the mean is §20.5's, the capped rows are the decoration of voxelize's filled slots,
the layer + maximum agree with torch.nn.functional.linear + amax within float32 rounding, and the coverage the GPU tests rely on
holds on the reference."""
import numpy as np
import pytest

import vfe_ref as vfe
import voxel_cases as vc
import voxel_ref as vr

F = np.float32


def gamma(n):
    u = 2.0 ** -24
    return n * u / (1.0 - n * u)


def _weights(cin, cout, seed=0):
    rng = np.random.default_rng(7000 + seed + 13 * cin + cout)
    return (rng.standard_normal((cout, cin)) / np.sqrt(cin)).astype(F), (rng.standard_normal(cout) * 0.1).astype(F)


def _tiles():
    pts, off, par, counts = vfe.tiles_case()
    p2v, coors, count, _ = vr.voxel_index(pts, off, par["v"], par["r"], par["V"])
    return pts, off, par, counts, p2v, coors, count


def test_tiles_coverage():
    pts, off, par, counts, p2v, coors, count = _tiles()
    for b, cs in enumerate(counts):
        nz = [c for c in cs if c > 0]
        assert count[b, :len(nz)].tolist() == nz and (count[b, len(nz):] == 0).all()
    have = set(count.reshape(-1).tolist())
    assert {0, 1, 2, 31, 32, 33, 63, 64, 65, 200} <= have
    rows, s_of, rank, start = vfe.members(p2v, off, par["V"])
    n = np.diff(start)
    straddle = (n > 0) & (start[:-1] // 32 != (start[1:] - 1) // 32)
    assert straddle.sum() >= 4                                         # voxels that cross a 32-row boundary of the lists
    assert ((n > 0) & (n <= 32) & straddle).any()                      # ... one of them shorter than a tile
    assert (np.diff(rows[start[0]:start[1]]) > 0).all() and not (np.diff(rows) > 0).all()   # list order is not row order
    assert (vfe.clean(p2v, par["V"]) < 0).sum() >= 18


@pytest.mark.parametrize("T", [None, 8])
def test_loop_equals_vectorised_and_mean(orc, T):
    pts, off, par, counts, p2v, coors, count = _tiles()
    V = par["V"]
    W, b = _weights(10, 33)
    kw = dict(coors=coors, voxel_size=par["v"], point_range=par["r"], T=T)
    pl, al, yl, rl, mean = vfe.encode_loop(orc, pts, p2v, off, V, W, b, **kw)
    pv, av, yv, rv = vfe.encode(orc, pts, p2v, off, V, W, b, **kw)
    assert np.array_equal(rl, rv) and np.array_equal(yl, yv) and np.array_equal(pl, pv) and np.array_equal(al, av)
    mp = vfe.member_p2v(p2v, off, V, T)
    want = vr.voxel_reduce(pts[:, :3], mp, off, V, "mean")[0].reshape(-1, 3)
    assert np.array_equal(mean, want)
    if T is not None:
        assert (count > T).any()


def test_capped_rows_are_the_filled_slots(orc):
    (name, pts, off, par), = vc.family_capped(3)
    T, V = 8, par["V"]
    p2v, coors, count, _ = vr.voxel_index(pts, off, par["v"], par["r"], V)
    assert (count > T).any()
    rows, mp, mean = vfe.decorate(pts, p2v, off, V, coors, par["v"], par["r"], True, True, None, T)
    voxels, _, num, _ = vr.voxelize(pts, off, par["v"], par["r"], T, V)
    B = len(off) - 1
    lst, s_of, rank, start = vfe.members(p2v, off, V)
    keep = rank < T
    # the decoration of slot (s, t) of the hard voxelization, from the slots alone
    vox = voxels.reshape(B * V, T, 3)
    nn = num.reshape(B * V)
    acc = vox[:, 0].copy()
    for t in range(1, T):
        acc = np.where((nn > t)[:, None], acc + vox[:, t], acc)
    m = np.where((nn > 0)[:, None], acc / np.maximum(nn, 1).astype(F)[:, None], F(0))
    ctr = vfe.centres(coors, par["v"], par["r"])
    slot = vox[s_of[keep], rank[keep]]
    want = np.concatenate([slot, slot - m[s_of[keep]], slot - ctr[s_of[keep]]], 1)
    assert np.array_equal(rows[lst[keep]], want)
    assert (rows[lst[~keep]] == 0).all() and (rows[mp < 0] == 0).all()


@pytest.mark.parametrize("relu", [True, False])
def test_against_torch_linear_amax(orc, relu):
    import torch
    pts, off, par, counts, p2v, coors, count = _tiles()
    V = par["V"]
    W, b = _weights(10, 64, 1)
    pooled, arg, y, rows = vfe.encode(orc, pts, p2v, off, V, W, b, relu, coors=coors, voxel_size=par["v"], point_range=par["r"])
    t = torch.nn.functional.linear(torch.from_numpy(rows), torch.from_numpy(W), torch.from_numpy(b))
    if relu:
        t = t.clamp_min(0)
    t = t.numpy().astype(np.float64)
    mag = np.abs(rows).astype(np.float64) @ np.abs(W).astype(np.float64).T + np.abs(b)
    bound = 2.0 * gamma(rows.shape[1] + 1) * mag
    mp = vfe.member_p2v(p2v, off, V)
    live = mp >= 0
    assert (np.abs(y.astype(np.float64) - t)[live] <= bound[live]).all()
    lst, s_of, rank, start = vfe.members(p2v, off, V)
    B = len(off) - 1
    for s in np.flatnonzero(np.diff(start) > 0):
        m = lst[start[s]:start[s + 1]]
        want = t[m].max(0)
        assert (np.abs(pooled.reshape(B * V, -1)[s] - want) <= bound[m].max(0)).all()
    assert (pooled.reshape(B * V, -1)[np.diff(start) == 0] == 0).all() and (arg.reshape(B * V, -1)[np.diff(start) == 0] == -1).all()


def test_negative_maxima_and_zero_tie(orc):
    """What the relu=False case of the GPU test relies on: negative maxima, and a voxel whose maximum is attained by -0.0 and
    +0.0 (a tie: arg is the lower row)."""
    pts, off, par, p2v, W, b = vfe.signed_zero_case()
    pooled, arg, y, rows = vfe.encode(orc, pts, p2v, off, par["V"], W, b, False, cluster_center=False, voxel_center=False)
    assert (pooled < 0).any()
    tie = [(np.signbit(y[m, 0]) & (y[m, 0] == 0)).any() and (~np.signbit(y[m, 0]) & (y[m, 0] == 0)).any() and pooled[0, v, 0] == 0
           for v in range(par["V"]) for m in [np.flatnonzero(p2v == v)] if len(m)]
    assert any(tie)
    v = tie.index(True)
    m = np.flatnonzero(p2v == v)
    assert arg[0, v, 0] == m[y[m, 0] == 0].min()
