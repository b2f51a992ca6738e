"""numpy reference of the MLP chain backward (SPEC.md §32) and the input generators its tests share.

The activations come from the oracle's ``mlp_rows`` applied one layer at a time to the gathered rows, so they are §6's bits; the
arg-max and ReLU decisions are taken on them; the linear algebra runs in ``dtype`` (float64, or float32 to check that a lattice
generator is exactly summable).  Beside every output the same quantity is evaluated with every factor replaced by its absolute
value (``A``): |gpu - ref| <= n * 2^-23 * A is §21.4's bound carried through the chain, with n the number of roundings on the
longest path to the element (``depth``: the rows summed + the widths of the layers passed + L)."""
import numpy as np

EPS = 2.0 ** -23


def make_layers(rng, dims, lattice):
    """[(W [C_l, C_{l-1}], b [C_l])] float32.  lattice: sparse weights out of {-1, 0, 1} (about four per row) and integer biases."""
    layers = []
    for cin, cout in zip(dims[:-1], dims[1:]):
        if lattice:
            w = rng.integers(-1, 2, (cout, cin)) * (rng.random((cout, cin)) < min(1.0, 4.0 / cin))
            b = rng.integers(-1, 2, cout)
        else:
            w = rng.standard_normal((cout, cin)) * (2.0 / cin) ** 0.5
            b = 0.1 * rng.standard_normal(cout)
        layers.append((w.astype(np.float32), b.astype(np.float32)))
    return layers


def make_counts(rng, B, M, S, mode):
    """cnt [B,M] int32: "mixed" holds 0, 1, S and values between in one call, scene 1 is less populated than scene 0; "ones" /
    "zeros": every count 1 / 0 (rows far below the slots; nothing but empty groups); None: no counts."""
    if mode is None:
        return None
    if mode in ("ones", "zeros"):
        return np.full((B, M), int(mode == "ones"), np.int32)
    assert mode == "mixed", mode
    cnt = rng.integers(0, S + 1, (B, M))
    flat = cnt.reshape(-1)
    flat[0::7] = 0
    flat[1::7] = 1
    flat[2::7] = S
    if B > 1:
        cnt[1] = np.minimum(cnt[1], max(1, S // 3))
    return cnt.astype(np.int32)


def make_grouped(rng, B, N, M, S, C, cnt_mode, lattice):
    """(xyz [B,N,3], feat [B,N,C] | None, new_xyz [B,M,3], idx [B,M,S], cnt | None) following §3: slots beyond cnt repeat slot 0,
    an empty group holds point 0."""
    if lattice:
        xyz = rng.integers(-64, 65, (B, N, 3)) / 64.0
        new_xyz = rng.integers(-64, 65, (B, M, 3)) / 64.0
        feat = rng.integers(-2, 3, (B, N, C)) if C else None
    else:
        xyz = rng.standard_normal((B, N, 3))
        new_xyz = rng.standard_normal((B, M, 3))
        feat = rng.standard_normal((B, N, C)) if C else None
    idx = rng.integers(0, N, (B, M, S))
    cnt = make_counts(rng, B, M, S, cnt_mode)
    if cnt is not None:
        slot = np.arange(S)[None, None, :]
        idx = np.where(slot < cnt[..., None], idx, idx[..., :1])
        idx[cnt == 0] = 0
    f32 = lambda a: None if a is None else np.ascontiguousarray(a, np.float32)
    return f32(xyz), f32(feat), f32(new_xyz), idx.astype(np.int32), cnt


def make_grad(rng, shape, lattice):
    return (rng.integers(-2, 3, shape) if lattice else rng.standard_normal(shape)).astype(np.float32)


def _activations(orc, x0, layers, relu_mask):
    """X_0 .. X_L: the oracle's §6 bits, or (``orc`` None) the same formulas in float64."""
    xs = [x0]
    if orc is None:
        for l, (w, b) in enumerate(layers):
            y = xs[-1].astype(np.float64) @ w.astype(np.float64).T + b.astype(np.float64)
            xs.append(np.maximum(y, 0) if (relu_mask >> l) & 1 else y)
        return xs
    for l, layer in enumerate(layers):
        xs.append(orc.mlp_rows(xs[-1], [layer], relu_mask=(relu_mask >> l) & 1) if xs[-1].shape[0] else
                  np.zeros((0, layer[0].shape[0]), np.float32))
    return xs


def _chain_back(xs, layers, relu_mask, g, ga, dtype):
    """D_l, grad_W_l, grad_b_l and G_0 from G_L = g (``ga``: its absolute companion) -> (gW, gb, G_0), (gWA, gbA, GA_0)."""
    L = len(layers)
    gW, gb, gWA, gbA = [None] * L, [None] * L, [None] * L, [None] * L
    for l in range(L, 0, -1):
        if (relu_mask >> (l - 1)) & 1:
            live = xs[l] > 0
            g, ga = np.where(live, g, 0), np.where(live, ga, 0)
        xin, w = xs[l - 1].astype(dtype), layers[l - 1][0].astype(dtype)
        gb[l - 1], gbA[l - 1] = g.sum(0), ga.sum(0)
        gW[l - 1], gWA[l - 1] = g.T @ xin, ga.T @ np.abs(xin)
        g, ga = g @ w, ga @ np.abs(w)
    return (gW, gb, g), (gWA, gbA, ga)


def grouped_ref(orc, xyz, feat, new_xyz, idx, cnt, layers, grad_out, skip_empty=False, dtype=np.float64, grad_out_A=None):
    """``orc`` None: float64 activations (what a float64 evaluation of the unfused composition decides on).  ``grad_out_A``: the
    absolute companion of a ``grad_out`` that is itself a computed gradient (a stage composed with the next), else |grad_out|.
    -> dict: pooled (the reference's own forward), mismatch-free by construction; val / A: {grad_feat, grad_xyz, grad_new_xyz,
    grad_W, grad_b}; depth: {name: n}; rows: the number of rows that exist; relu_on: per layer (activations > 0, activations)."""
    B, N, _ = xyz.shape
    _, M, S = idx.shape
    C = 0 if feat is None else feat.shape[2]
    L = len(layers)
    nrow = np.full((B, M), S) if cnt is None else np.clip(cnt, 1, S)
    if skip_empty:
        nrow = np.where(cnt == 0, 0, nrow)
    bb, mm, ss = np.nonzero(np.arange(S)[None, None, :] < nrow[..., None])          # rows in (b, m, s) order
    src = idx[bb, mm, ss]
    x0 = xyz[bb, src] - new_xyz[bb, mm]                                              # float32: one rounding, as the kernels
    if C:
        x0 = np.concatenate([x0, feat[bb, src]], 1)
    x0 = np.ascontiguousarray(x0, np.float32)
    xs = _activations(orc, x0, layers, (1 << L) - 1)
    CL = layers[-1][0].shape[0]
    start = np.concatenate([[0], np.cumsum(nrow.reshape(-1))])
    pooled = np.zeros((B * M, CL), xs[L].dtype)
    g, ga = np.zeros((len(bb), CL), dtype), np.zeros((len(bb), CL), dtype)
    go = grad_out.reshape(B * M, CL).astype(dtype)
    goa = np.abs(go) if grad_out_A is None else grad_out_A.reshape(B * M, CL).astype(dtype)
    for gi in range(B * M):
        r0, r1 = start[gi], start[gi + 1]
        if r1 == r0:
            continue
        seg = xs[L][r0:r1]
        pooled[gi] = seg.max(0)
        arg = (seg == pooled[gi]).argmax(0)                                          # the lowest row that attains the maximum
        g[r0 + arg, np.arange(CL)] = go[gi]
        ga[r0 + arg, np.arange(CL)] = goa[gi]
    (gW, gb, g0), (gWA, gbA, g0A) = _chain_back(xs, layers, (1 << L) - 1, g, ga, dtype)
    val, A = {"grad_W": gW, "grad_b": gb}, {"grad_W": gWA, "grad_b": gbA}
    for d, src_g in ((val, g0), (A, g0A)):
        sign = -1.0 if d is val else 1.0
        gx = np.zeros((B, N, 3), dtype)
        np.add.at(gx, (bb, src), src_g[:, :3])
        gn = np.zeros((B, M, 3), dtype)
        np.add.at(gn, (bb, mm), sign * src_g[:, :3])
        d["grad_xyz"], d["grad_new_xyz"] = gx, gn
        if C:
            gf = np.zeros((B, N, C), dtype)
            np.add.at(gf, (bb, src), src_g[:, 3:])
            d["grad_feat"] = gf
    R = len(bb)
    widths = [w.shape[0] for w, _ in layers]
    depth = {"grad_W": [R + sum(widths[l + 1:]) + L for l in range(L)], "grad_feat": R + sum(widths) + L}
    depth["grad_b"] = depth["grad_W"]
    depth["grad_xyz"] = depth["grad_new_xyz"] = depth["grad_feat"]
    return {"pooled": pooled.reshape(B, M, CL), "val": val, "A": A, "depth": depth, "rows": R,
            "relu_on": [(int((x > 0).sum()), x.size) for x in xs[1:]]}


def rows_ref(orc, x, layers, relu_mask, grad_out, dtype=np.float64):
    """Plain rows: x [R, C_0], grad_out [R, C_L] -> the same dict with grad_x, grad_W, grad_b."""
    L = len(layers)
    xs = _activations(orc, np.ascontiguousarray(x, np.float32), layers, relu_mask)
    g = grad_out.astype(dtype)
    (gW, gb, g0), (gWA, gbA, g0A) = _chain_back(xs, layers, relu_mask, g, np.abs(g), dtype)
    R = x.shape[0]
    widths = [w.shape[0] for w, _ in layers]
    depth = {"grad_W": [R + sum(widths[l + 1:]) + L for l in range(L)], "grad_x": sum(widths) + L}
    depth["grad_b"] = depth["grad_W"]
    return {"out": xs[L], "val": {"grad_x": g0, "grad_W": gW, "grad_b": gb}, "A": {"grad_x": g0A, "grad_W": gWA, "grad_b": gbA},
            "depth": depth, "rows": R}


def check_close(name, got, want, A, n, exact=False):
    """|got - want| <= n 2^-23 A per element, exact zeros of the reference exact; ``exact``: equality."""
    got = np.asarray(got, np.float64)
    assert got.shape == want.shape, (name, got.shape, want.shape)
    assert np.isfinite(got).all(), f"{name}: non-finite values"
    if exact:
        bad = got != want
        assert not bad.any(), f"{name}: {int(bad.sum())} of {bad.size} elements differ on exactly summable inputs (max {np.abs(got - want).max():.3e})"
        return
    zero = A == 0
    assert (got[zero] == 0).all(), f"{name}: {int((got[zero] != 0).sum())} exact zeros of the reference are not zero"
    err, bound = np.abs(got - want), n * EPS * A
    worst = (err / np.maximum(bound, 1e-300))[~zero].max() if (~zero).any() else 0.0
    print(f"{name}: max |err| / bound = {worst:.3f} (n = {n})")
    assert (err <= bound).all(), f"{name}: {int((err > bound).sum())} elements beyond n 2^-23 A (n = {n}), worst ratio {worst:.3f}"


# The shapes the CPU and GPU tests share: the smallest at which the kernels take every path (a ragged last 32-channel tile, more
# than one 128-channel block, groups across 64-row tiles, S = 1 / 64, N = 3 points shared by every group, two scenes of
# different population, every kind of count in one call).
GROUPED_CASES = {
    "L1_C0_S1_nocnt_N3": dict(B=1, N=3, M=7, S=1, C=0, widths=[10], cnt_mode=None, skip=False),
    "L2_C1_S16_mixed": dict(B=1, N=50, M=13, S=16, C=1, widths=[33, 64], cnt_mode="mixed", skip=False),
    "L3_C5_S33_mixed_B2": dict(B=2, N=40, M=37, S=33, C=5, widths=[10, 33, 160], cnt_mode="mixed", skip=False),
    "L3_C5_S33_skip_B2": dict(B=2, N=40, M=37, S=33, C=5, widths=[10, 33, 160], cnt_mode="mixed", skip=True),
    "L4_C32_S64_mixed": dict(B=1, N=70, M=21, S=64, C=32, widths=[64, 33, 160, 10], cnt_mode="mixed", skip=False),
    "L2_C5_S16_nocnt_N3_B2": dict(B=2, N=3, M=9, S=16, C=5, widths=[33, 10], cnt_mode=None, skip=False),
}
ROWS_DIMS = [5, 33, 160, 10]
ROWS_MASKS = {"all": 7, "none": 0, "alternating": 5}
ROWS_R = (1, 63, 64, 65, 1000)


def grouped_case(name, lattice, seed=0):
    """-> (inputs dict, layers, grad_out [B,M,C_L]) of a named case."""
    c = GROUPED_CASES[name]
    rng = np.random.default_rng([seed, sorted(GROUPED_CASES).index(name), int(lattice)])
    xyz, feat, new_xyz, idx, cnt = make_grouped(rng, c["B"], c["N"], c["M"], c["S"], c["C"], c["cnt_mode"], lattice)
    layers = make_layers(rng, [3 + c["C"]] + c["widths"], lattice)
    grad_out = make_grad(rng, (c["B"], c["M"], c["widths"][-1]), lattice)
    return dict(xyz=xyz, feat=feat, new_xyz=new_xyz, idx=idx, cnt=cnt, skip_empty=c["skip"]), layers, grad_out


def rows_case(R, lattice, seed=0):
    rng = np.random.default_rng([seed, R, int(lattice)])
    x = (rng.integers(-2, 3, (R, ROWS_DIMS[0])) if lattice else rng.standard_normal((R, ROWS_DIMS[0]))).astype(np.float32)
    return x, make_layers(rng, ROWS_DIMS, lattice), make_grad(rng, (R, ROWS_DIMS[-1]), lattice)


# The contract edges and tile boundaries (tests/test_gpu_mlp_grad_edges.py), seeded apart from GROUPED_CASES so that neither
# table moves the other's inputs.  The GEMM tile is 128 channels x 64 rows x 32 k and a wave owns 32 channels: C_0 = 32 / 64 / 65,
# widths 1 / 32 / 128 / 129 / 257 (one logit, exact wave and block multiples, one channel into the next block, three blocks), K and
# the weight gradient's J at 64 / 65; chunks of exactly 64 and 128 rows; 100 rows in 6400 slots; nothing but empty groups;
# more than three chunks of the minimum workspace with and without counts (without: row = g S + s at a chunk base g0 > 0).
EDGE_CASES = {
    "w1_C29_S16_mixed": dict(B=1, N=40, M=9, S=16, C=29, widths=[32, 1], cnt_mode="mixed", skip=False),
    "w128_C61_S16_mixed": dict(B=1, N=40, M=9, S=16, C=61, widths=[128, 32], cnt_mode="mixed", skip=False),
    "w129_C62_S16_mixed": dict(B=1, N=40, M=9, S=16, C=62, widths=[129, 64, 65], cnt_mode="mixed", skip=False),
    "w257_C5_S16_mixed": dict(B=1, N=40, M=9, S=16, C=5, widths=[257, 10], cnt_mode="mixed", skip=False),
    "rows64_M4_S16_nocnt": dict(B=1, N=40, M=4, S=16, C=5, widths=[33, 10], cnt_mode=None, skip=False),
    "rows128_M2_S64_nocnt": dict(B=1, N=40, M=2, S=64, C=5, widths=[33, 10], cnt_mode=None, skip=False),
    "sparse_M100_S64_ones": dict(B=1, N=40, M=100, S=64, C=5, widths=[33, 10], cnt_mode="ones", skip=False),
    "empty_M100_S64_zeros_skip": dict(B=1, N=40, M=100, S=64, C=5, widths=[33, 10], cnt_mode="zeros", skip=True),
    "chunks_M100_S16_nocnt_B2": dict(B=2, N=60, M=100, S=16, C=5, widths=[33, 10], cnt_mode=None, skip=False),
    "chunks_M100_S16_mixed_B2": dict(B=2, N=60, M=100, S=16, C=5, widths=[33, 10], cnt_mode="mixed", skip=False),
}
EDGE_ROWS_DIMS = {"64_257_1": [64, 257, 1], "65_128_32": [65, 128, 32]}
EDGE_ROWS_MASKS = {"all": 3, "none": 0}
EDGE_ROWS_R = (64, 128)


def edge_case(name, lattice, seed=0):
    """-> (inputs dict, layers, grad_out [B,M,C_L]) of a named edge case (every coordinate finite; a test that wants NaN
    coordinates in skipped groups writes them itself)."""
    c = EDGE_CASES[name]
    rng = np.random.default_rng([seed, sorted(EDGE_CASES).index(name), int(lattice), 1])
    xyz, feat, new_xyz, idx, cnt = make_grouped(rng, c["B"], c["N"], c["M"], c["S"], c["C"], c["cnt_mode"], lattice)
    layers = make_layers(rng, [3 + c["C"]] + c["widths"], lattice)
    grad_out = make_grad(rng, (c["B"], c["M"], c["widths"][-1]), lattice)
    return dict(xyz=xyz, feat=feat, new_xyz=new_xyz, idx=idx, cnt=cnt, skip_empty=c["skip"]), layers, grad_out


def edge_rows_case(R, dims_name, lattice, seed=0):
    dims = EDGE_ROWS_DIMS[dims_name]
    rng = np.random.default_rng([seed, R, int(lattice), sorted(EDGE_ROWS_DIMS).index(dims_name), 1])
    x = (rng.integers(-2, 3, (R, dims[0])) if lattice else rng.standard_normal((R, dims[0]))).astype(np.float32)
    return x, make_layers(rng, dims, lattice), make_grad(rng, (R, dims[-1]), lattice)


LATTICE_UNIT = 2.0 ** -6     # every lattice input is a multiple of it (coordinates: k / 64; everything else: integers)


def order_free(res):
    """True when every sum of a lattice case is exact in float32 in ANY order: all terms are multiples of LATTICE_UNIT and
    the sum of their magnitudes (``A``) stays below 2^24 units, so no partial sum of any grouping needs more than 24 bits."""
    worst = 0.0
    for v in res["A"].values():
        for a in (v if isinstance(v, list) else [v]):
            worst = max(worst, float(np.max(a, initial=0.0)))
    return worst / LATTICE_UNIT < 2.0 ** 24, worst


def corrupt_pairs(cnt, grad_out, k_live, k_dead):
    """(group, channel) pairs whose pooled value a test overwrites: ``k_live`` in groups with cnt > 0 (``cnt`` None: any group)
    and ``k_dead`` in groups with cnt == 0, dealt in turn to the scenes and spread from the first to the last such group of
    each, at channels where grad_out is not 0 -> [(b, m, o)], no pair twice."""
    B, M, CL = grad_out.shape
    pairs = []
    for k, want in ((k_live, np.ones((B, M), bool) if cnt is None else cnt > 0), (k_dead, None if cnt is None else cnt == 0)):
        per = -(-k // B)
        for i in range(k):
            b, groups = i % B, np.nonzero(want[i % B])[0]
            m = int(groups[(i // B) * (len(groups) - 1) // max(1, per - 1)])
            o = next(o % CL for o in range(7 * i, 7 * i + CL) if grad_out[b, m, o % CL] != 0 and (b, m, o % CL) not in pairs)
            pairs.append((b, m, o))
    return pairs


def zero_pairs(grad_out, pairs):
    g = grad_out.copy()
    for b, m, o in pairs:
        g[b, m, o] = 0
    return g
