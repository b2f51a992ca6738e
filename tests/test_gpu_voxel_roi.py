"""GPU parity of voxel RoI pooling (SPEC.md §30) (-m gpu): roi_grid_points and voxel_query equal tests/voxel_roi_ref.py under ==,
VoxelRoIPool's fused path against §6 under the comparison rule of tests/test_gpu_mlp.py, its training path against CPU autograd."""
import numpy as np
import pytest

import voxel_roi_ref as ref

pytestmark = pytest.mark.gpu
TOL = 1e-4                                              # tests/test_gpu_mlp.py's
CASES = [(f, r, S) for f in ref.FAMILIES for r in ref.RANGES for S in ref.SIZES]
EXACT_VS, EXACT_PR, _ = ref.FAMILIES["exact"]


def _t(a, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _close(got, want, what):
    """The rule tests/test_gpu_mlp.py applies to PackedMLP.grouped."""
    diff = np.abs(got.astype(np.float64) - want.astype(np.float64))
    rel = diff / (1.0 + np.abs(want))
    print(f"[parity] {what}: max|diff|={diff.max():.3e} bit-exact={np.array_equal(got, want)}")
    assert rel.max() <= TOL, f"{what}: max rel diff {rel.max():.3e} > {TOL}"


# ---- voxel_query -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family,max_range,S", CASES)
def test_voxel_query_parity(sad, dev, family, max_range, S):
    import torch
    from sad_amd import ops
    coors, offsets, shape, vs, pr, new_xyz, radius = ref.query_args(family)
    want_idx, want_cnt = ref.expected(family, max_range, S)
    args = (_t(coors, dev), _t(offsets, dev), shape, vs, pr, _t(new_xyz, dev))
    idx, cnt = ops.voxel_query(*args, max_range=max_range, radius=radius, S=S)
    assert np.array_equal(cnt.cpu().numpy(), want_cnt)
    assert np.array_equal(idx.cpu().numpy(), want_idx)
    # again, into the caller's buffers and workspace (both full of other bits): bit-equal
    out = (torch.full_like(idx, -7), torch.full_like(cnt, -7))
    ws = ops.voxel_query_workspace(len(coors), dev)
    ws.fill_(0x5A)
    got = ops.voxel_query(*args, max_range=max_range, radius=radius, S=S, out=out, workspace=ws)
    assert got[0] is out[0] and got[1] is out[1]
    assert torch.equal(out[0], idx) and torch.equal(out[1], cnt)


@pytest.mark.parametrize("name", ["widest", "cell limit"])
def test_voxel_query_extra_cases(sad, dev, name):
    """max_range (8,8,8), the widest walk; and a grid of 1290^3 cells, 794 647 below the bound, with voxels at its far corner."""
    from sad_amd import ops
    coors, offsets, shape, vs, pr, new_xyz, max_range, radius, S = ref.extra_cases()[name]
    form = ref.query_brute if name == "widest" else ref.query_walk
    want_idx, want_cnt = form(coors, offsets, shape, vs, pr[:3], new_xyz, max_range, radius, S)
    idx, cnt = ops.voxel_query(_t(coors, dev), _t(offsets, dev), shape, vs, pr, _t(new_xyz, dev), max_range=max_range, radius=radius, S=S)
    assert np.array_equal(cnt.cpu().numpy(), want_cnt)
    assert np.array_equal(idx.cpu().numpy(), want_idx)


def test_voxel_query_without_voxels_and_without_queries(sad, dev):
    import torch
    from sad_amd import ops
    _, _, shape, vs, pr, new_xyz, radius = ref.query_args("exact")
    none = torch.zeros((0, 3), dtype=torch.int32, device=dev)
    idx, cnt = ops.voxel_query(none, torch.zeros(4, dtype=torch.int32, device=dev), shape, vs, pr, _t(new_xyz, dev), max_range=(1, 2, 3),
                               radius=radius, S=4)
    assert tuple(idx.shape) == (3, 67, 4) and not idx.any() and not cnt.any()
    coors, offsets = ref.grid()
    idx, cnt = ops.voxel_query(_t(coors, dev), _t(offsets, dev), shape, vs, pr, torch.zeros((3, 0, 3), device=dev), max_range=(1, 2, 3),
                               radius=radius, S=4)
    torch.cuda.synchronize()
    assert tuple(idx.shape) == (3, 0, 4) and tuple(cnt.shape) == (3, 0)


# ---- roi_grid_points -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G", [1, 6])
@pytest.mark.parametrize("D", [7, 9])
def test_roi_grid_points_parity(sad, dev, G, D):
    import torch
    from sad_amd import ops
    rois = ref.rois_case(D)
    got = ops.roi_grid_points(_t(rois, dev), None, G)
    assert tuple(got.shape) == (2, 9, G ** 3, 3)
    assert np.array_equal(got.cpu().numpy().view(np.int32), ref.grid_points_loop(rois, None, G).view(np.int32))
    assert torch.equal(ops.roi_grid_points(_t(rois, dev), None, G), got), "two calls differ"
    for count in (np.array([4, 0], np.int32), np.array([-3, 99], np.int32), np.array([9, 1], np.int32)):
        want = ref.grid_points_loop(rois, count, G)
        n = np.clip(count, 0, 9)
        got = ops.roi_grid_points(_t(rois, dev), _t(count, dev), G).cpu().numpy()
        assert np.array_equal(got.view(np.int32), want.view(np.int32))
        for b in range(2):
            assert (got[b, n[b]:].view(np.uint32) == ref.NAN_BITS).all()
        poisoned = rois.copy()
        for b in range(2):
            poisoned[b, n[b]:] = np.array([np.nan, np.inf, -1e30, 1e38, 0, -np.inf, 1e30] + [np.nan] * (D - 7), np.float32)
        out = torch.full((2, 9, G ** 3, 3), 5.0, device=dev)
        assert ops.roi_grid_points(_t(poisoned, dev), _t(count, dev), G, out=out) is out
        assert np.array_equal(out.cpu().numpy().view(np.int32), want.view(np.int32)), "an unread RoI row reached the output"


# ---- VoxelRoIPool ----------------------------------------------------------------------------------------------------------------
def _coarse(coors, offsets):
    """The active set one stride-2 level down: cells // 2, per scene in order of first appearance."""
    out, offs = [], [0]
    for b in range(len(offsets) - 1):
        c = coors[offsets[b]:offsets[b + 1]] // 2
        if len(c):
            _, first = np.unique((c[:, 0] * 64 + c[:, 1]) * 64 + c[:, 2], return_index=True)
            c = c[np.sort(first)]
        out.append(c)
        offs.append(offs[-1] + len(c))
    return np.concatenate(out).astype(np.int32), np.array(offs, np.int32)


def _scene(C, seed, integer=False):
    """Two scales of the exact family's grid (B = 3, the middle scene empty) with features, and 5 RoIs per scene of which
    roi_count = (5, 3, 4) count: ([(coors, offsets, shape, voxel_size, feat)] * 2, rois, roi_count)."""
    rng = np.random.default_rng(seed)
    coors, offsets = ref.grid()
    c2, o2 = _coarse(coors, offsets)
    levels = []
    for c, o, shape, vs in ((coors, offsets, ref.SHAPE, EXACT_VS), (c2, o2, (3, 6, 6), tuple(2 * v for v in EXACT_VS))):
        feat = rng.integers(-8, 9, (len(c), C)).astype(np.float32) if integer else rng.normal(size=(len(c), C)).astype(np.float32)
        levels.append((c, o, shape, vs, feat))
    if integer:     # grid points on few-bit dyadic coordinates: centres on multiples of 0.5, extents 1 / 2 / 4, no rotation, G = 2
        rois = np.zeros((3, 5, 7), np.float32)
        rois[..., :3] = rng.integers(-4, 5, (3, 5, 3)) * 0.5
        rois[..., 2] = rng.integers(-1, 2, (3, 5)) * 0.5
        rois[..., 3:6] = 2.0 ** rng.integers(0, 3, (3, 5, 3))
    else:
        rois = rng.uniform(-2.5, 2.5, (3, 5, 8)).astype(np.float32)
        rois[..., 2] = rng.uniform(-0.4, 0.6, (3, 5))
        rois[..., 3:6] = rng.uniform(0.5, 3.0, (3, 5, 3))
        rois[..., 6] = rng.uniform(-np.pi, np.pi, (3, 5))
    return levels, rois.astype(np.float32), np.array([5, 3, 4], np.int32)


SCALES = (dict(max_range=(2, 2, 2), radius=1.2, nsample=16), dict(max_range=(1, 1, 1), radius=2.5, nsample=8))


def _module(sad, dev, levels, G, mlp, layers):
    """The module over `levels` with the given layers ([(W, b), ...] per scale) as its parameters."""
    import torch
    scales = [dict(s, in_channels=lv[4].shape[1], voxel_size=lv[3], mlp=mlp) for s, lv in zip(SCALES, levels)]
    m = sad.VoxelRoIPool(G, scales, EXACT_PR).to(dev)
    with torch.no_grad():
        for k, ls in enumerate(layers):
            for l, (W, b) in enumerate(ls):
                m.weight[k][l].copy_(_t(W, dev))
                m.bias[k][l].copy_(_t(b, dev))
    return m


def _tensors(sad, dev, levels, grad=False):
    out = []
    for c, o, shape, _, feat in levels:
        f = _t(feat, dev)
        f.requires_grad_(grad)
        out.append(sad.SparseTensor(f, _t(c, dev), _t(o, dev), shape))
    return out


def _reference_indices(levels, rois, count, G):
    """Per scale (idx [Q,S], cnt [Q]) of the reference, and the grid points [Q,3]; Q = B * R * G^3."""
    pts = ref.grid_points_loop(rois, count, G)
    B, R = rois.shape[:2]
    res = []
    for s, (c, o, shape, vs, _) in zip(SCALES, levels):
        idx, cnt = ref.query_walk(c, o, shape, vs, EXACT_PR[:3], pts.reshape(B, R * G ** 3, 3), s["max_range"], s["radius"], s["nsample"])
        res.append((idx.reshape(-1, s["nsample"]), cnt.reshape(-1)))
    return res, pts.reshape(-1, 3)


def test_fused_path_against_section_6(sad, dev):
    """Two scales, C = 16 -> [16, 16]: the pooled rows equal §6 on the reference's indices under test_gpu_mlp's rule; the rows of
    an empty group (the empty scene, the RoIs beyond roi_count, a grid point with nothing in reach) are exactly zero; two calls
    are bit-equal; and after a weight is written the chain is packed again."""
    import torch
    from sad_amd import synth
    G = 3
    levels, rois, count = _scene(16, 1)
    rng = np.random.default_rng(2)
    layers = [synth.make_mlp_weights([19, 16, 16], rng) for _ in levels]
    m = _module(sad, dev, levels, G, [16, 16], layers)
    tensors = _tensors(sad, dev, levels)
    with torch.no_grad():
        got_t = m(_t(rois, dev), _t(count, dev), tensors)
        again = m(_t(rois, dev), _t(count, dev), tensors)
    assert tuple(got_t.shape) == (3, 5, G ** 3, 32)
    assert torch.equal(got_t, again), "two calls differ"
    got = got_t.cpu().numpy().reshape(-1, 32)
    indices, pts = _reference_indices(levels, rois, count, G)
    for k, ((idx, cnt), (c, _, _, vs, feat)) in enumerate(zip(indices, levels)):
        want = ref.pool_rows(c, feat, vs, EXACT_PR[:3], pts, idx, cnt, layers[k])
        cols = got[:, 16 * k:16 * (k + 1)]
        _close(cols, want, f"scale {k}")
        assert 0 < (cnt == 0).sum() < len(cnt) and (cnt[135:270] == 0).all()
        assert (cols[cnt == 0] == 0).all(), "a row with cnt == 0 is not exactly zero"
        assert np.isfinite(cols).all() and (cols[cnt > 0] > 0).any()
    with torch.no_grad():
        m.weight[0][0].mul_(0.5)
        changed = m(_t(rois, dev), _t(count, dev), tensors).cpu().numpy().reshape(-1, 32)
    layers[0][0] = (layers[0][0][0] * np.float32(0.5), layers[0][0][1])
    idx, cnt = indices[0]
    _close(changed[:, :16], ref.pool_rows(levels[0][0], levels[0][4], levels[0][3], EXACT_PR[:3], pts, idx, cnt, layers[0]), "after a weight write")
    assert np.array_equal(changed[:, 16:], got[:, 16:])


def _compose_cpu(levels, pts, indices, weights, dtype):
    """The module's training composition in CPU torch: per scale gather -> [rel | feat] -> linear + ReLU layers -> max over the
    samples (the first of equal maxima, as MaxPoolS) -> zero where cnt == 0; -> (pooled [Q, sum C_out], the feature leaves)."""
    import torch
    cols, leaves = [], []
    p = torch.from_numpy(np.nan_to_num(pts, nan=0.0, posinf=0.0, neginf=0.0))
    for (c, _, _, vs, feat), (idx, cnt), ws in zip(levels, indices, weights):
        f = torch.tensor(feat, dtype=dtype, requires_grad=True)
        leaves.append(f)
        xyz = torch.from_numpy(ref.centres(c[:, ::-1], vs, EXACT_PR[:3]))
        i = torch.from_numpy(idx.astype(np.int64))
        rel = (xyz[i] - p[:, None, :]).to(dtype)          # (binary32 subtraction, as the module's)
        rel = torch.where(torch.from_numpy(np.isfinite(pts).all(1))[:, None, None], rel, torch.zeros((), dtype=dtype))
        x = torch.cat([rel, f[i]], -1)
        for W, b in ws:
            x = torch.relu(x @ W.t() + b)
        pooled = x.max(1).values
        cols.append(pooled.masked_fill(torch.from_numpy(cnt == 0)[:, None], 0.0))
    return torch.cat(cols, 1), leaves


def test_training_path_exact_on_summable_inputs(sad, dev):
    """Integer features (|feat| <= 8), integer weights and biases, grid points and voxel centres on multiples of 1/8: every
    partial sum of the forward and of the backward is representable (§21.4's condition), so pooled, the feature gradient and
    the weight gradients equal CPU torch autograd of the same composition under ==, whatever the order of the additions."""
    import torch
    G = 2
    levels, rois, count = _scene(4, 3, integer=True)
    rng = np.random.default_rng(4)
    layers = [[(rng.integers(-2, 3, (8, 7)).astype(np.float32), rng.integers(-2, 3, 8).astype(np.float32)),
               (rng.integers(-2, 3, (8, 8)).astype(np.float32), rng.integers(-2, 3, 8).astype(np.float32))] for _ in levels]
    m = _module(sad, dev, levels, G, [8, 8], layers)
    m.requires_grad_(True)
    tensors = _tensors(sad, dev, levels, grad=True)
    pooled = m(_t(rois, dev), _t(count, dev), tensors)
    pooled.sum().backward()
    indices, pts = _reference_indices(levels, rois, count, G)
    assert np.array_equal(pts[np.isfinite(pts).all(1)] * 8, np.round(pts[np.isfinite(pts).all(1)] * 8))
    weights = [[(torch.tensor(W, requires_grad=True), torch.tensor(b, requires_grad=True)) for W, b in ls] for ls in layers]
    want, leaves = _compose_cpu(levels, pts, indices, weights, torch.float32)
    want.sum().backward()
    assert (want.detach().numpy() > 0).any() and any((cnt == 0).any() for _, cnt in indices)
    assert np.array_equal(pooled.detach().cpu().numpy().reshape(want.shape), want.detach().numpy())
    for k in range(2):
        assert leaves[k].grad.abs().sum() > 0
        assert np.array_equal(tensors[k].feat.grad.cpu().numpy(), leaves[k].grad.numpy()), f"scale {k}: feature gradient"
        for l in range(2):
            assert np.array_equal(m.weight[k][l].grad.cpu().numpy(), weights[k][l][0].grad.numpy()), f"scale {k} layer {l}: weight gradient"
            assert np.array_equal(m.bias[k][l].grad.cpu().numpy(), weights[k][l][1].grad.numpy()), f"scale {k} layer {l}: bias gradient"


def test_training_path_gradient_bound_and_agreement_with_the_fused_path(sad, dev):
    """General inputs.  Forward: the training path and the fused path agree under test_gpu_mlp's rule, and both are exactly zero
    on the empty rows.  Backward of pooled.sum(): an element of the feature gradient is a sum of products of weights, one per
    (sample that reads the row, path through the layers that the ReLUs and the arg-max leave open); the masks are taken from a
    binary64 forward of the same rows, and the element must lie within §21.4's n * 2^-23 * sum|terms| of the binary64 sum, n = the
    number of its non-zero terms (an element without terms is exactly 0)."""
    import torch
    from sad_amd import synth
    G = 3
    levels, rois, count = _scene(16, 5)
    rng = np.random.default_rng(6)
    layers = [synth.make_mlp_weights([19, 16, 16], rng) for _ in levels]
    m = _module(sad, dev, levels, G, [16, 16], layers)
    tensors = _tensors(sad, dev, levels)
    with torch.no_grad():
        fused = m(_t(rois, dev), _t(count, dev), tensors).cpu().numpy().reshape(-1, 32)
    tensors = _tensors(sad, dev, levels, grad=True)
    pooled = m(_t(rois, dev), _t(count, dev), tensors)
    assert pooled.requires_grad
    pooled.sum().backward()
    train = pooled.detach().cpu().numpy().reshape(-1, 32)
    _close(train, fused, "training path against the fused path")
    indices, pts = _reference_indices(levels, rois, count, G)
    finite = np.isfinite(pts).all(1)
    for k, ((c, _, _, vs, feat), (idx, cnt)) in enumerate(zip(levels, indices)):
        empty = cnt == 0
        assert empty.any() and (train[empty, 16 * k:16 * (k + 1)] == 0).all() and (fused[empty, 16 * k:16 * (k + 1)] == 0).all()
        (W1, b1), (W2, b2) = [(np.asarray(W, np.float64), np.asarray(b, np.float64)) for W, b in layers[k]]
        xyz = ref.centres(c[:, ::-1], vs, EXACT_PR[:3])
        with np.errstate(all="ignore"):
            rel = np.where(finite[:, None, None], xyz[idx] - pts[:, None, :], np.float32(0))
        x0 = np.concatenate([rel, feat[idx]], -1).astype(np.float64)                     # [Q,S,19]
        a1 = x0 @ W1.T + b1
        a2 = np.maximum(a1, 0) @ W2.T + b2
        h2 = np.maximum(a2, 0)
        arg = h2.argmax(1)                                                              # [Q,16], the first of equal maxima
        g2 = (np.arange(idx.shape[1])[None, :, None] == arg[:, None, :]) & (a2 > 0) & ~empty[:, None, None]

        def back(m2, m1):
            g1 = (g2.astype(np.float64) @ m2) * (a1 > 0)
            g0 = g1 @ m1[:, 3:]
            out = np.zeros(feat.shape, np.float64)
            np.add.at(out, idx.reshape(-1), g0.reshape(-1, feat.shape[1]))
            return out
        want, mag, n = back(W2, W1), back(np.abs(W2), np.abs(W1)), back((W2 != 0).astype(np.float64), (W1 != 0).astype(np.float64))
        got = tensors[k].feat.grad.cpu().numpy().astype(np.float64)
        bound = n * 2.0 ** -23 * mag
        err = np.abs(got - want)
        print(f"[grad] scale {k}: max err {err.max():.3e}, max bound {bound.max():.3e}, max n {n.max():.0f}, "
              f"worst err / bound {np.max(err[bound > 0] / bound[bound > 0]):.3f}, rows without terms {(n.sum(1) == 0).sum()}")
        assert (n > 0).any() and (got[n == 0] == 0).all()
        assert (err <= bound).all(), f"scale {k}: {(err > bound).sum()} elements beyond n * 2^-23 * sum|terms|, worst {np.max(err - bound):.3e}"
