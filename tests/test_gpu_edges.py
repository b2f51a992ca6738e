"""GPU edge-case parity of the kernels around the hot path (-m gpu): backward (SPEC.md §16), candidates and
box decode (§8, §9), rotated NMS (§13), kNN (§4) and the pure copies (§5, §17).

Random inputs rarely reach the branches where these kernels can go wrong, so every input here is built to
sit on one: channel and row tiles that end part-way, out-of-range scatter indices, +-0 and exact ties, the
clamps of the head, the 64-rank chunks of the NMS walk, shells of equal d2 that straddle the k-th place,
and bit patterns (denormals, NaN payloads) that only a byte-faithful copy keeps.  Index results and copies
are compared bit for bit; scatter-adds use SPEC §16's 1e-5 * sum|terms| against a binary64 sum, boxes
SPEC §9's 1e-4."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TOL = 1e-4  # SPEC.md §9


def _t(a, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _bits(t):
    """Bit patterns of a float tensor (host copy) as int32 / int16."""
    import torch
    t = t.detach().cpu().contiguous()
    return (t.view(torch.int32) if t.element_size() == 4 else t.view(torch.int16)).numpy()


# ---------------------------------------------------------------- backward (SPEC.md §16)
def _scatter_ref(gout, idx, N):
    """binary64 scatter-add and sum|terms| per element; slots outside [0, N) contribute nothing."""
    B, C, M, S = gout.shape
    ref = np.zeros((B, N, C), np.float64)
    mag = np.zeros((B, N, C), np.float64)
    for b in range(B):
        j = idx[b].reshape(-1)
        ok = (j >= 0) & (j < N)
        g = gout[b].reshape(C, -1)[:, ok].T.astype(np.float64)
        np.add.at(ref[b], j[ok], g)
        np.add.at(mag[b], j[ok], np.abs(g))
    return ref.transpose(0, 2, 1), mag.transpose(0, 2, 1)


def _check_scatter_forms(ag, gout, idx, N, dev):
    """All three forms of group_points_grad: point-major + transpose (default), direct channel-major, point-major out."""
    ref, mag = _scatter_ref(gout, idx, N)
    for kw in (dict(via_point_major=True), dict(via_point_major=False), dict(point_major=True)):
        got = ag.group_points_grad(_t(gout, dev), _t(idx, dev), N, **kw).cpu().numpy()
        if kw.get("point_major"):
            got = got.transpose(0, 2, 1)
        bad = np.abs(got - ref) > 1e-5 * mag + 1e-30
        assert not bad.any(), f"{kw}: {int(bad.sum())} elements off, first at {np.argwhere(bad)[0]}"


@pytest.mark.parametrize("C", [63, 65, 128, 130, 257])
@pytest.mark.parametrize("M,S", [(7, 9), (29, 9)])
def test_group_points_grad_channel_and_row_tiles(sad, dev, C, M, S):
    """The point-major scatter tiles channels by 64 and (m,s) by 64: a second channel tile, a partial one, and an (m,s)
    range that is not a multiple of 64 (M*S = 63 and 261); N = 50 makes most points collect many terms."""
    from sad_amd import autograd as ag
    rng = np.random.default_rng(C * 100 + M)
    B, N = 2, 50
    idx = rng.integers(0, N, (B, M, S)).astype(np.int32)
    gout = rng.standard_normal((B, C, M, S)).astype(np.float32)
    _check_scatter_forms(ag, gout, idx, N, dev)


def test_group_points_grad_skips_out_of_range_slots(sad, dev):
    """backward.hip: an out-of-range or negative index contributes nothing, in both kernels."""
    from sad_amd import autograd as ag
    rng = np.random.default_rng(5)
    B, C, N, M, S = 2, 65, 40, 13, 11
    idx = rng.integers(0, N, (B, M, S)).astype(np.int32)
    bad = rng.random((B, M, S)) < 0.3
    idx[bad] = rng.choice(np.array([-1, N, N + 1, -N, 2 * N], np.int32), int(bad.sum()))
    idx[0, 0, :] = -1                                          # whole group of padding slots
    idx[1, -1, :] = N
    gout = rng.standard_normal((B, C, M, S)).astype(np.float32)
    _check_scatter_forms(ag, gout, idx, N, dev)


def test_group_points_grad_one_hot_point(sad, dev):
    """Every slot points at one point: 65 536 terms summed into one element per channel."""
    from sad_amd import autograd as ag
    rng = np.random.default_rng(6)
    B, C, N, M, S = 1, 3, 10, 1024, 64
    idx = np.full((B, M, S), 7, np.int32)
    gout = rng.standard_normal((B, C, M, S)).astype(np.float32)
    _check_scatter_forms(ag, gout, idx, N, dev)


@pytest.mark.parametrize("C", [5, 65])
def test_gather_points_autograd(sad, dev, C):
    """autograd.GatherPoints: forward == torch.gather bit for bit, backward == a binary64 index_add (SPEC §16 tolerance)."""
    import torch
    from sad_amd import autograd as ag
    rng = np.random.default_rng(C)
    B, N, M = 2, 90, 150                                       # M > N: repeated indices
    f0 = rng.standard_normal((B, C, N)).astype(np.float32)
    idx = rng.integers(0, N, (B, M)).astype(np.int32)
    idx[:, :20] = 3                                            # one point gathered many times
    g = rng.standard_normal((B, C, M)).astype(np.float32)
    feat = _t(f0, dev).requires_grad_(True)
    out = ag.gather_points(feat, _t(idx, dev))
    want = torch.gather(_t(f0, dev), 2, _t(idx, dev).long()[:, None, :].expand(B, C, M))
    np.testing.assert_array_equal(_bits(out), _bits(want))
    out.backward(_t(g, dev))
    ref = torch.zeros((B, C, N), dtype=torch.float64)
    mag = torch.zeros((B, C, N), dtype=torch.float64)
    for b in range(B):
        gb = torch.from_numpy(g[b]).double()
        ref[b].index_add_(1, torch.from_numpy(idx[b]).long(), gb)
        mag[b].index_add_(1, torch.from_numpy(idx[b]).long(), gb.abs())
    got = feat.grad.cpu().double()
    assert bool(((got - ref).abs() <= 1e-5 * mag + 1e-30).all())


def _pool_input(rng, B, C, M, S):
    """Rows of ordinary values, rows of one repeated value, rows of +-0, rows of very negative values, rows whose maximum
    occurs twice."""
    x = rng.standard_normal((B, C, M, S)).astype(np.float32)
    r = x.reshape(-1, S)
    kind = np.arange(r.shape[0]) % 5
    r[kind == 1] = rng.standard_normal((int((kind == 1).sum()), 1)).astype(np.float32)
    zs = rng.random((int((kind == 2).sum()), S)) < 0.5
    r[kind == 2] = np.where(zs, np.float32(-0.0), np.float32(0.0))
    r[kind == 3] = -rng.uniform(1e38, 3.4e38, (int((kind == 3).sum()), S)).astype(np.float32)
    if S > 1:
        rows3 = np.flatnonzero(kind == 3)
        r[rows3, S - 1] = r[rows3].max(axis=1)                  # the maximum of huge negatives twice
        rows4 = np.flatnonzero(kind == 4)
        hi = r[rows4].max(axis=1) + 1.0
        r[rows4, rng.integers(0, S, rows4.size)] = hi
        r[rows4, S - 1] = hi
    return x


@pytest.mark.parametrize("S", [1, 63, 64, 65])
def test_max_pool_s_ties_and_signed_zeros(sad, dev, S):
    """max over S with ties -> lowest s (SPEC §16): all-equal rows give arg 0, a +-0 row gives the FIRST zero with its
    sign bit, and the gradient lands on that slot only.  B*C*M = 303 rows: the last workgroup is partial."""
    from sad_amd import autograd as ag
    rng = np.random.default_rng(S)
    B, C, M = 1, 3, 101
    x = _pool_input(rng, B, C, M, S)
    out, arg = ag.max_pool_s_with_arg(_t(x, dev))
    want_arg = x.argmax(-1)                                     # numpy: first maximum; -0.0 == +0.0
    want_out = np.take_along_axis(x, want_arg[..., None], -1)[..., 0]
    np.testing.assert_array_equal(arg.cpu().numpy(), want_arg.astype(np.int32))
    np.testing.assert_array_equal(_bits(out), want_out.view(np.int32))
    rows = x.reshape(-1, S)
    if S > 1:
        assert (rows[1::5] == rows[1::5, :1]).all() and (arg.cpu().numpy().reshape(-1)[1::5] == 0).all()
        assert np.signbit(rows[2::5]).any() and (~np.signbit(rows[2::5])).any()
    g = rng.standard_normal((B, C, M)).astype(np.float32)
    xt = _t(x, dev).requires_grad_(True)
    ag.max_pool_s(xt).backward(_t(g, dev))
    want = np.zeros_like(x)
    np.put_along_axis(want, want_arg[..., None], g[..., None], axis=-1)
    np.testing.assert_array_equal(_bits(xt.grad), want.view(np.int32))


# ---------------------------------------------------------------- candidates + decode (SPEC.md §8 steps 2-4, §9)
def _f32(*v):
    return np.array(v, np.float32)


def _clamp_edges(lim, rng, n):
    """n float32 values: exactly +-lim, one ulp inside and past it, far past it, and ordinary ones inside."""
    lim = np.float32(lim)
    edge = _f32(lim, -lim, np.nextafter(lim, np.float32(0)), np.nextafter(-lim, np.float32(0)),
                np.nextafter(lim, np.float32(np.inf)), np.nextafter(-lim, np.float32(-np.inf)),
                4 * lim, -4 * lim, 0.0, -0.0)
    return np.where(np.arange(n) % 2 == 0, rng.choice(edge, n), rng.uniform(-1.5 * lim, 1.5 * lim, n)).astype(np.float32)


def _candidates_gpu(dev, xyz3, c, shift_max, r_min, r_max, anchor):
    import torch
    from sad_amd import _lib
    B, M3, _ = xyz3.shape
    K = c.shape[1]
    X, Cc = _t(xyz3, dev), _t(c, dev)
    cand = torch.empty((B, K, 3), dtype=torch.float32, device=dev)
    rad = torch.empty((B, K), dtype=torch.float32, device=dev)
    a = (ctypes.c_float * 3)(*anchor)
    _lib.check(_lib.lib().sad_candidates_f32(X.data_ptr(), Cc.data_ptr(), B, M3, K, shift_max, r_min, r_max, a,
                                             cand.data_ptr(), rad.data_ptr(), torch.cuda.current_stream().cuda_stream),
               "sad_candidates_f32")
    return cand.cpu().numpy(), rad.cpu().numpy()


def test_candidates_clamps(orc, sad, dev):
    """shift at +-shift_max, s at +-1 (and one ulp either side of both), radii clamped to r_min / r_max and radii that land
    exactly on them before the clamp: bit-exact vs the oracle.  B = 2, K = 300, M3 = 333 > K."""
    from sad_amd import config
    cfg = config.TINY
    rng = np.random.default_rng(8)
    B, K, M3 = 2, 300, 333
    xyz3 = rng.uniform(-40, 40, (B, M3, 3)).astype(np.float32)
    c = np.empty((B, K, 6), np.float32)
    c[..., :3] = _clamp_edges(cfg.shift_max, rng, B * K * 3).reshape(B, K, 3)
    c[..., 3:] = _clamp_edges(1.0, rng, B * K * 3).reshape(B, K, 3)
    anchor = tuple(cfg.anchor_car)
    # the unclamped radii: take two of them as r_min / r_max, so that some radii equal a bound exactly before the clamp
    # (with SPEC §8's own bounds r_min is never reached: q >= 0.5 keeps r above 1.12)
    _, raw = orc.candidates(xyz3, c, cfg.shift_max, 0.0, 3e38, anchor)
    lo, hi = np.quantile(raw, 0.25, method="lower"), np.quantile(raw, 0.75, method="lower")
    for r_min, r_max in ((cfg.r_min, cfg.r_max), (float(lo), float(hi))):
        want_c, want_r = orc.candidates(xyz3, c, cfg.shift_max, r_min, r_max, anchor)
        got_c, got_r = _candidates_gpu(dev, xyz3, c, cfg.shift_max, r_min, r_max, anchor)
        np.testing.assert_array_equal(got_c.view(np.int32), want_c.view(np.int32))
        np.testing.assert_array_equal(got_r.view(np.int32), want_r.view(np.int32))
        assert (want_r == np.float32(r_max)).sum() > 10
    assert (want_r == np.float32(lo)).sum() > 10 and (raw == lo).any() and (raw == hi).any()


def _decode_gpu(dev, cand, o, anchors):
    import torch
    from sad_amd import _lib
    B, K, _ = cand.shape
    boxes = torch.empty((B, K, 9), dtype=torch.float32, device=dev)
    a = (ctypes.c_float * 9)(*[v for an in anchors for v in an])
    Cd, O = _t(cand, dev), _t(o, dev)
    _lib.check(_lib.lib().sad_decode_boxes_f32(Cd.data_ptr(), O.data_ptr(), B, K, a, boxes.data_ptr(),
                                               torch.cuda.current_stream().cuda_stream), "sad_decode_boxes_f32")
    return boxes.cpu().numpy()


def test_decode_boxes_ties_clamps_saturation(orc, sad, dev):
    """label = argmax cls with ties -> lowest (two- and three-way, +-0), size residuals on and past +-2, and |cls| large
    enough that expf saturates (score exactly 0 or 1).  Labels exact, boxes within 1e-4.  B*K = 600 (partial workgroup)."""
    from sad_amd import config
    cfg = config.TINY
    rng = np.random.default_rng(9)
    B, K = 2, 300
    cand = rng.uniform(-40, 40, (B, K, 3)).astype(np.float32)
    o = rng.standard_normal((B, K, 10)).astype(np.float32)
    o[..., 6:9] = _clamp_edges(2.0, rng, B * K * 3).reshape(B, K, 3)
    o[..., 9] = rng.uniform(-7, 7, (B, K))
    cls = o[..., :3].reshape(-1, 3)
    kind = np.arange(cls.shape[0]) % 8
    v = rng.standard_normal(cls.shape[0]).astype(np.float32)
    lower = v - np.float32(1.0)
    cls[kind == 1] = np.stack([v, v, lower], 1)[kind == 1]      # labels 0 = 1 tie
    cls[kind == 2] = np.stack([lower, v, v], 1)[kind == 2]      # labels 1 = 2 tie
    cls[kind == 3] = np.stack([v, lower, v], 1)[kind == 3]      # labels 0 = 2 tie
    cls[kind == 4] = np.stack([v, v, v], 1)[kind == 4]          # three-way tie
    cls[kind == 5] = _f32(-0.0, 0.0, -1.0)                      # -0 and +0 tie
    cls[kind == 6] = (rng.choice(_f32(-1, 1), (int((kind == 6).sum()), 1)) *
                      rng.uniform(90, 200, (int((kind == 6).sum()), 3))).astype(np.float32)   # expf saturates
    cls[kind == 7] = _f32(-150.0, -150.0, -200.0)               # saturated and tied
    o[..., :3] = cls.reshape(B, K, 3)
    want = orc.decode_boxes(cand, o, cfg.anchors)
    got = _decode_gpu(dev, cand, o, cfg.anchors)
    np.testing.assert_array_equal(got[..., 8], want[..., 8])
    err = np.abs(got - want) / (1.0 + np.abs(want))
    assert err.max() <= TOL, f"boxes differ from the oracle: {err.max():.3e}"
    lab = want[..., 8].reshape(-1)
    assert (lab[kind == 4] == 0).all() and (lab[kind == 2] == 1).all() and (lab[kind == 5] == 0).all()
    assert (want[..., 7] == 0).any() and (want[..., 7] == 1).any()


# ---------------------------------------------------------------- rotated NMS (SPEC.md §13)
def _nms_all(orc, dev, bx, thr, sthr, out=None):
    """Both GPU paths (three kernels, one workgroup per scene) against the oracle; returns the oracle's result."""
    from sad_amd import ops
    want = orc.nms_bev(bx, thr, sthr)
    for single in (False, True):
        got = ops.nms_bev(_t(bx, dev), thr, sthr, single_kernel=single, out=out)
        for name, g, w in zip(("keep", "order", "count"), got, want):
            np.testing.assert_array_equal(g.cpu().numpy(), w, err_msg=f"{name}, single_kernel={single}")
    return want


def _boxes(seed, B, K, extent, size=(2.5, 5.0, 1.2, 2.2)):
    rng = np.random.default_rng(seed)
    bx = np.zeros((B, K, 9), np.float32)
    bx[..., 0:2] = rng.uniform(0, extent, (B, K, 2))
    bx[..., 2] = rng.uniform(-2, 0, (B, K))
    bx[..., 3] = rng.uniform(size[0], size[1], (B, K))
    bx[..., 4] = rng.uniform(size[2], size[3], (B, K))
    bx[..., 5] = 1.5
    bx[..., 6] = rng.uniform(-4, 4, (B, K))
    bx[..., 7] = rng.uniform(0, 1, (B, K))
    bx[..., 8] = rng.integers(0, 3, (B, K))
    return bx


@pytest.mark.parametrize("K", [63, 64, 65, 128, 511, 512])
def test_nms_chunk_edges(orc, sad, dev, K):
    """Crowded scenes with K at the edges of the walk's 64-rank chunks, and at the limit."""
    bx = _boxes(K, 2, K, extent=2.0 * np.sqrt(K))
    bx[1, ::3, 7] = bx[1, 0, 7]                                 # score ties across chunks
    _, _, cnt = _nms_all(orc, dev, bx, 0.1, 0.0)
    assert (cnt < K * 3 // 4).all()


def test_nms_score_threshold_edge(orc, sad, dev):
    """score == score_thr is a candidate (>=); a scene with every score below it keeps nothing."""
    K, sthr = 100, 0.3
    bx = _boxes(11, 2, K, extent=60.0)
    bx[0, :, 7] = np.random.default_rng(11).choice(_f32(0.1, sthr, np.nextafter(np.float32(sthr), np.float32(0)), 0.7), K)
    bx[1, :, 7] = np.nextafter(np.float32(sthr), np.float32(0))
    keep, order, cnt = _nms_all(orc, dev, bx, 0.2, sthr)
    assert ((keep[0] == 1) & (bx[0, :, 7] == np.float32(sthr))).any()
    assert cnt[1] == 0 and (order[1] == -1).all() and (keep[1] == 0).all()


@pytest.mark.parametrize("thr", [0.5, 1.0])
def test_nms_identical_boxes(orc, sad, dev, thr):
    """Exact duplicates: IoU ~1 suppresses the copy at thr = 0.5.  At thr = 1.0 the strict > keeps both copies exactly
    where the binary32 IoU of SPEC §13 does not round above 1 (it does for some: clipped area vs l*w)."""
    K = 80
    bx = _boxes(12, 2, K, extent=80.0)
    bx[:, :20, 6] = 0.0                                        # some axis-aligned
    bx[:, 1::2] = bx[:, 0::2]                                  # every box twice, same score
    bx[1, 1::2, 7] = bx[1, 0::2, 7] * np.float32(0.5)          # scene 1: the copy ranks lower
    _, _, cnt = _nms_all(orc, dev, bx, thr, 0.0)
    if thr == 1.0:
        self_iou = orc.iou_bev(bx[:, 0::2].reshape(-1, 9), bx[:, 1::2].reshape(-1, 9)).reshape(2, -1)
        np.testing.assert_array_equal(cnt, K - (self_iou > 1.0).sum(axis=1))
        assert (cnt > K // 2).all()
    else:
        assert (cnt <= K // 2).all()


def test_nms_degenerate_boxes(orc, sad, dev):
    """Zero-length and zero-width boxes (denominator <= 0 -> IoU 0), two of them at the same spot, next to ordinary
    boxes; at thr = 0."""
    K = 70
    bx = _boxes(13, 1, K, extent=8.0)
    bx[0, 0:10, 3] = 0.0
    bx[0, 10:20, 4] = 0.0
    bx[0, 20:24, 3:5] = 0.0
    bx[0, 30] = bx[0, 0]                                       # zero-length pair at one spot
    bx[0, 31] = bx[0, 10]                                      # zero-width pair
    bx[0, 32, :7] = bx[0, 20, :7]                              # zero-area pair
    for thr in (0.0, 0.3):
        _nms_all(orc, dev, bx, thr, 0.0)


def test_nms_shared_edges(orc, sad, dev):
    """Axis-aligned unit boxes on a grid: neighbours share an edge or a corner (intersection area 0); at thr = 0."""
    g = np.arange(8, dtype=np.float32)
    xx, yy = np.meshgrid(g, g, indexing="ij")
    K = xx.size
    bx = np.zeros((2, K, 9), np.float32)
    bx[..., 0], bx[..., 1] = xx.reshape(-1), yy.reshape(-1)
    bx[..., 3:6] = 1.0
    bx[..., 7] = np.random.default_rng(14).uniform(0, 1, (2, K))
    bx[1, :, 6] = np.float32(np.pi / 2)                        # rotated by a quarter turn: the same footprints
    bx[1, :, 3] = 2.0                                          # 2 x 1 boxes: overlaps
    _nms_all(orc, dev, bx, 0.0, 0.0)


def test_nms_yaw_edges(orc, sad, dev):
    """yaw at +-pi/2, pi, 3pi/2 (where the Cody-Waite quadrant switches) and around +-1e3."""
    K = 200
    bx = _boxes(15, 2, K, extent=20.0)
    rng = np.random.default_rng(15)
    quarter = _f32(np.pi / 2, -np.pi / 2, np.pi, 3 * np.pi / 2, -np.pi, 0.0)
    near = np.concatenate([quarter, np.nextafter(quarter, np.float32(10)), np.nextafter(quarter, np.float32(-10))])
    bx[0, :, 6] = rng.choice(near, K)
    bx[1, :, 6] = rng.choice(_f32(1, -1), K) * rng.uniform(999.0, 1001.0, K).astype(np.float32)
    for thr in (0.0, 0.2):
        _nms_all(orc, dev, bx, thr, 0.0)


def test_nms_workspace_reuse(orc, sad, dev):
    """out=nms_bev_buffers(...) reused on inputs A, B, A (pipeline.py reuses them every step): no result leaks into the next."""
    from sad_amd import ops
    B, K = 2, 300
    a = _boxes(16, B, K, extent=20.0)
    b = _boxes(17, B, K, extent=60.0)
    b[0, :, 7] *= np.float32(0.2)                              # far fewer candidates than A
    buf = ops.nms_bev_buffers(B, K, dev)
    for bx, sthr in ((a, 0.0), (b, 0.1), (a, 0.0)):
        _nms_all(orc, dev, bx, 0.1, sthr, out=buf)


def _boxes_few_candidates(B=2, K=200, n1=70):
    """Crowded scenes; in scene 1 only ``n1`` scattered boxes reach score 0.1: ceil(n/64) = 2 < ceil(K/64) = 4, last chunk partial."""
    bx = _boxes(19, B, K, extent=2.0 * np.sqrt(K))
    rng = np.random.default_rng(20)
    low = np.ones(K, bool)
    low[rng.permutation(K)[:n1]] = False
    bx[1, :, 7] = np.where(low, np.float32(0.09) * bx[1, :, 7], np.float32(0.1) + np.float32(0.9) * bx[1, :, 7])
    return bx


def test_nms_workspace_unwritten_words(orc, sad, dev):
    """The three-kernel nms_bev on a workspace whose every byte is 0xFF, twice on the same buffers: the mask kernel stores only
    the words k = p/64 .. ceil(n/64) - 1 of row p, so whatever the walk reads must have been written in this call.  Exact against
    the oracle; both scenes keep strictly between 0 and n boxes."""
    from sad_amd import ops
    B, K, thr, sthr = 2, 200, 0.1, 0.1
    bx = _boxes_few_candidates(B, K)
    n = (bx[..., 7] >= np.float32(sthr)).sum(1)
    assert n[1] == 70 and 128 < n[0] < K
    want = orc.nms_bev(bx, thr, sthr)
    assert (want[2] > 0).all() and (want[2] < n).all()
    buf = ops.nms_bev_buffers(B, K, dev)
    buf[3].fill_(0xFF)
    for call in (1, 2):
        got = ops.nms_bev(_t(bx, dev), thr, sthr, out=buf)
        for name, g, w in zip(("keep", "order", "count"), got, want):
            np.testing.assert_array_equal(g.cpu().numpy(), w, err_msg=f"{name}, call {call}")


def test_nms_out_buffers_checked(sad, dev):
    """A caller's ``out`` that a kernel would write past its end is refused before anything is launched: keep / order / count of
    a 2-byte dtype, keep / order as a ``[:, ::2]`` view of a twice-as-wide tensor (count [1] has no strided form: a view of one
    element is contiguous), a workspace one byte short (``single_kernel=True`` uses none).  The buffers keep their fill, and
    the untouched tuple then gives the result of the call without ``out``."""
    import torch
    from sad_amd import ops
    B, K = 1, 4
    boxes = _t(_boxes(18, B, K, extent=6.0), dev)
    scores = boxes[..., 7].contiguous()
    bev, big = ops.nms_bev_buffers(B, K, dev), ops.nms_boxes_buffers(B, K, dev)
    for name, buf, call, uses_ws in (
            ("nms_bev", bev, lambda out: ops.nms_bev(boxes, 0.1, 0.0, out=out), True),
            ("nms_bev single_kernel", bev, lambda out: ops.nms_bev(boxes, 0.1, 0.0, single_kernel=True, out=out), False),
            ("nms_boxes", big, lambda out: ops.nms_boxes(boxes, scores, None, 0.1, 0.0, out=out), True)):
        for t in buf[:3]:
            t.fill_(-7)
        bad = []
        for i, t in enumerate(buf[:3]):
            bad.append((i, torch.zeros(t.shape, dtype=torch.int16, device=dev)))
            if t.dim() == 2:
                bad.append((i, torch.zeros((B, 2 * t.shape[1]), dtype=torch.int32, device=dev)[:, ::2]))
        if uses_ws:
            assert buf[3].numel() > 1
            bad.append((3, buf[3][:-1]))
        for i, t in bad:
            with pytest.raises(ValueError, match="^(out|workspace): "):
                call(buf[:i] + (t,) + buf[i + 1:])
        torch.cuda.synchronize()
        assert all(bool((t == -7).all()) for t in buf[:3]), f"{name}: a refused call wrote into the buffers"
        for g, w in zip(call(buf), call(None)):
            assert torch.equal(g, w), name


# ---------------------------------------------------------------- kNN (SPEC.md §4)
def _lattice(seed, B, n):
    """B scenes of the n^3 integer lattice, each in its own point order (so index order is not spatial order)."""
    ax = np.arange(n, dtype=np.float32)
    g = np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), -1).reshape(-1, 3)
    rng = np.random.default_rng(seed)
    return np.stack([g[rng.permutation(len(g))] for _ in range(B)])


@pytest.mark.parametrize("k", [1, 6, 7, 26, 27, 64])
def test_knn_lattice_shells(orc, sad, dev, k):
    """Centroids on lattice points: shells of equal d2 (1, 6, 12, 8, 6, 24, ... points) straddle the k-th place; the lowest
    indices of the cut shell win.  M = 37 (not a multiple of 4 or 64)."""
    from sad_amd import ops
    xyz = _lattice(k, 2, 7)
    rng = np.random.default_rng(k)
    new_xyz = xyz[:, rng.integers(0, xyz.shape[1], 37)].copy()
    new_xyz[:, :5] = 3.0                                       # the lattice centre: complete shells around it
    got = ops.knn_query(k, _t(xyz, dev), _t(new_xyz, dev)).cpu().numpy()
    np.testing.assert_array_equal(got, orc.knn_query(k, xyz, new_xyz))


def test_knn_duplicates_beyond_k(orc, sad, dev):
    """A centroid with more than k exact duplicates at d2 = 0 (and more beyond them): the k lowest indices of them."""
    from sad_amd import ops
    xyz = _lattice(20, 2, 6)
    xyz[0, 30:130] = xyz[0, 200]                               # 101 copies of one point
    xyz[1, ::2] = xyz[1, 5]                                    # half the scene on one spot
    new_xyz = np.stack([xyz[0, [200, 31, 0, 150]], xyz[1, [5, 4, 7, 1]]])
    for k in (1, 33, 64):
        got = ops.knn_query(k, _t(xyz, dev), _t(new_xyz, dev)).cpu().numpy()
        np.testing.assert_array_equal(got, orc.knn_query(k, xyz, new_xyz), err_msg=f"k={k}")


@pytest.mark.parametrize("N", [37, 64])
def test_knn_k_equals_n(orc, sad, dev, N):
    """k == N <= 64: every point, sorted by (d2, index)."""
    from sad_amd import ops
    rng = np.random.default_rng(N)
    xyz = rng.integers(-2, 3, (2, N, 3)).astype(np.float32)   # small integers: many equal distances
    new_xyz = rng.integers(-3, 4, (2, 70, 3)).astype(np.float32)
    got = ops.knn_query(N, _t(xyz, dev), _t(new_xyz, dev)).cpu().numpy()
    np.testing.assert_array_equal(got, orc.knn_query(N, xyz, new_xyz))


def test_knn_far_centroids(orc, sad, dev):
    """Centroids far outside the cloud: d2 ~ 1e8 where neighbouring distances round to the same float."""
    from sad_amd import ops
    rng = np.random.default_rng(21)
    xyz = rng.uniform(0, 10, (2, 700, 3)).astype(np.float32)
    xyz[:, 600:] = xyz[:, :100]                                # and exact duplicates
    new_xyz = (rng.choice(_f32(-1, 1), (2, 45, 3)) * rng.uniform(5e3, 1e4, (2, 45, 3))).astype(np.float32)
    for k in (5, 64):
        got = ops.knn_query(k, _t(xyz, dev), _t(new_xyz, dev)).cpu().numpy()
        np.testing.assert_array_equal(got, orc.knn_query(k, xyz, new_xyz), err_msg=f"k={k}")


# ---------------------------------------------------------------- pure copies (SPEC.md §5, §17)
def _special_f32(rng, shape):
    """float32 bit patterns a copy through float arithmetic would change: +-denormals, -0.0, quiet and signalling NaNs with
    distinct payloads (either sign), among ordinary values."""
    n = int(np.prod(shape))
    k = np.arange(n, dtype=np.uint32)
    pats = [k % 0x7FFFFF + 1,                                  # denormals
            (k % 0x7FFFFF + 1) | 0x80000000,                   # negative denormals
            np.full(n, 0x80000000, np.uint32),                 # -0.0
            0x7FC00000 | (k % 0x3FFFFF + 1),                   # quiet NaN payloads
            0x7F800000 | (k % 0x3FFFFF + 1),                   # signalling NaN payloads
            0xFFC00000 | (k * 7 % 0x3FFFFF),                   # negative quiet NaNs
            rng.standard_normal(n).astype(np.float32).view(np.uint32)]
    u = np.choose(rng.integers(0, len(pats), n), pats).astype(np.uint32)
    return u.view(np.float32).reshape(shape)


def _special_16(rng, shape, kind):
    """float16 / bfloat16 bit patterns (as int16): +-denormals, -0, NaN payloads."""
    n = int(np.prod(shape))
    k = np.arange(n, dtype=np.uint16)
    if kind == "f16":
        pats = [k % 0x3FF + 1, (k % 0x3FF + 1) | 0x8000, 0x7C00 | (k % 0x1FF + 1), 0x7E00 | (k % 0x1FF), 0xFE00 | (k % 0x1FF)]
    else:
        pats = [k % 0x7F + 1, (k % 0x7F + 1) | 0x8000, 0x7F80 | (k % 0x3F + 1), 0x7FC0 | (k % 0x3F), 0xFFC0 | (k % 0x3F)]
    pats += [np.full(n, 0x8000, np.uint16), rng.integers(0x3000, 0x4400, n).astype(np.uint16)]
    return np.choose(rng.integers(0, len(pats), n), pats).astype(np.uint16).view(np.int16).reshape(shape)


_COPY_SHAPES = [(2, 3, 100, 64, 16),        # M*S = 1024: 16-byte vector path
                (2, 9, 100, 7, 9),          # M*S = 63: scalar path, a partial channel block of 8
                (1, 3, 500, 512, 16)]       # M*S = 8192 >= 4N: LDS-staged path


@pytest.mark.parametrize("B,C,N,M,S", _COPY_SHAPES)
@pytest.mark.parametrize("dtype", ["f32", "f16", "bf16"])
def test_copies_are_bit_faithful(orc, sad, dev, dtype, B, C, N, M, S):
    """group_points / gather_points (every element type) and gather_xyz keep every bit: denormals, -0.0, NaN payloads."""
    import torch
    from sad_amd import ops
    rng = np.random.default_rng(N + M + C)
    if dtype == "f32":
        feat = _special_f32(rng, (B, C, N))
        dev_feat = _t(feat, dev)
    else:
        feat = _special_16(rng, (B, C, N), dtype)
        dev_feat = _t(feat, dev).view(torch.float16 if dtype == "f16" else torch.bfloat16)
    ref_bits = feat.view(np.int32 if dtype == "f32" else np.int16)
    idx = rng.integers(0, N, (B, M, S)).astype(np.int32)
    got = ops.group_points(dev_feat, _t(idx, dev))
    np.testing.assert_array_equal(_bits(got), orc.group_points(ref_bits, idx))
    i2 = np.ascontiguousarray(idx[:, :, 0])
    got = ops.gather_points(dev_feat, _t(i2, dev))
    np.testing.assert_array_equal(_bits(got), orc.gather_points(ref_bits, i2))
    if dtype == "f32":
        xyz = _special_f32(rng, (B, N, 3))
        got = ops.gather_xyz(_t(xyz, dev), _t(i2, dev))
        want = orc.gather_xyz(xyz, i2)
        np.testing.assert_array_equal(_bits(got), want.view(np.int32))
        np.testing.assert_array_equal(want.view(np.int32), np.take_along_axis(xyz, i2[..., None], 1).view(np.int32))


@pytest.mark.parametrize("C", [1, 3, 4, 5])
@pytest.mark.parametrize("offset", [0, 1])
def test_subsample_pad_paths(orc, sad, dev, C, offset):
    """subsample_pad (SPEC §17) from / into views at a 4-byte offset (the scalar path for C = 4) and aligned ones: n_points =
    300 (partial workgroup), scenes with n > n_points, an empty one in the middle, n == n_points and n < n_points.  Rows
    are byte copies: equal to the oracle and io.fix_size bit for bit, special patterns included."""
    import torch
    from sad_amd import io, ops
    rng = np.random.default_rng(C * 10 + offset)
    n_points = 300
    sizes = [700, 0, 300, 41, 1]
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    pts = _special_f32(rng, (int(offs[-1]), C))
    pbuf = torch.empty(pts.size + offset, dtype=torch.float32, device=dev)
    pv = pbuf[offset:].view(pts.shape)
    pv.copy_(torch.from_numpy(pts))
    B = len(sizes)
    obuf = torch.full((B * n_points * C + offset,), float("nan"), dtype=torch.float32, device=dev)
    ov = obuf[offset:].view(B, n_points, C)
    assert pv.data_ptr() % 16 == 4 * offset and ov.data_ptr() % 16 == 4 * offset
    for seed in (0, 12345):
        got = ops.subsample_pad(pv, _t(offs, dev), n_points, seed, out=ov)
        want = orc.subsample_pad(pts, offs, n_points, seed)
        np.testing.assert_array_equal(_bits(got), want.view(np.int32))
        for b in range(B):
            fx = io.fix_size(pts[offs[b]:offs[b + 1]], n_points, seed, scene=b)
            np.testing.assert_array_equal(want[b].view(np.int32), fx.view(np.int32), err_msg=f"scene {b}")
