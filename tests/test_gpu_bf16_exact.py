"""Bit-exact parity of every bf16 MLP dispatch form with the SPEC §14 oracle, on lattice inputs (-m gpu).

On the inputs of tests/bf16_lattice.py every partial sum of every layer is exact in binary32 (the budget), so the order of the additions —
the one thing §14 leaves free — cannot change a bit, and the oracle's binary64 sum is THE answer.  Outputs behind a ReLU are compared by
their bits (SPEC: `acc > 0 ? acc : 0`, so a zero is +0); outputs of a layer without a ReLU by value (the sign of an exact zero there
depends on the order).  Every case asserts that it still reaches the kernel form it is named for, and prints its lattice statistics.

Stage level (test_detector_backbone_exact): SADDetector(dtype="bf16") on lattice points with sparse lattice weights (about three nonzero
weights of ±2^-s per output) in every sa* chain.  Each stage's output must equal the oracle chained from the raw points (fps -> ball query
-> branches -> aggregation, no GPU tensor fed back), and submit() with replayed plans and split pooling must give the eager boxes.  Cluster
layer and head stay under test_gpu_bf16's tolerance: their candidate centres are off the lattice.

Signed zeros.  The pooling of every grouped kernel is an unsigned atomicMax on the float's bits, correct only while no -0 reaches it
(0x80000000 beats every positive float).  test_signed_zero_probe first measures whether the matrix unit gives -0 at all for a sum of
-0 products on a -0 bias (one plain layer without ReLU, where the sign is visible) and prints the answer; the pooling cases that follow
feed such rows into every grouped kernel that takes a one-layer chain.  Measured on the MI355X: all three plain-row forms give +0 for
every such sum, so those cases pin the values and the +0 of the maxima, but a pooling that let -0 through (`m >= 0.f ? m : 0.f`) is
not reachable on this hardware and passes them.  The f32 chain is different: its pre-activations of such rows are -0 (measured and
printed by test_signed_zeros_into_pooling), so there the pooling cases do see a -0 reach the ReLU, at every forced geometry.
"""
import numpy as np
import pytest

import bf16_lattice as bl

pytestmark = pytest.mark.gpu


def _t(a, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _exact(got, want, what, by_bits=True):
    g = np.ascontiguousarray(got, dtype=np.float32)
    w = np.ascontiguousarray(want, dtype=np.float32)
    assert g.shape == w.shape, f"{what}: shape {g.shape} != {w.shape}"
    bad = (g.view(np.uint32) != w.view(np.uint32)) if by_bits else (g != w)
    n = int(bad.sum())
    print(f"[exact-bf16] {what}: {n} of {bad.size} differ ({'bits' if by_bits else 'values'})")
    if n:
        i = tuple(int(v) for v in np.argwhere(bad)[0])
        raise AssertionError(f"{what}: {n} of {bad.size} elements differ from the oracle; first at {i}: "
                             f"got {g[i]!r} ({g[i].view(np.uint32):#010x}) want {w[i]!r} ({w[i].view(np.uint32):#010x})")


def _cus(dev):
    import torch
    return torch.cuda.get_device_properties(dev).multi_processor_count


def _rows_form(rows, dims, x_bf16, cus, form1=False):
    """The kernel csrc/mlp_bf16_rows.hip launch_bf16_rows (one plain layer) or sad_mlp_chain_bf16 (more) picks for these rows."""
    if len(dims) > 2 or dims[0] % 8:
        return "tiled"
    ks = (dims[0] + 15) // 16
    ct = (dims[1] + 31) // 32
    nrb = (rows + 127) // 128
    if not form1 and x_bf16 and dims[0] == 16 * ks and ks % 4 == 0:
        return f"rows2 NTW{2 if ct > 2 else 1}" + (" many-blocks" if nrb > cus else "")
    nt = 4 if ct > 2 else 2
    grid = 8 * ((nrb + 7) // 8) * ((ct + nt - 1) // nt)
    deep = (ks + 3) // 4 > 2 and grid <= 2 * cus
    return f"rows1 NT{nt} " + ("deep" if deep else "single-ahead")


def _chain_limits(c, extra=()):
    keys = ["positive"] + (["rounded", "ties"] if len(c.recs) > 1 else []) + list(extra)
    return keys


# ---- plain rows (PackedMLPBf16.rows) ----------------------------------------------------------------------------------------------------
def test_smallest_plain_rows_case(sad, dev):
    """Run first: one plain layer, 37 rows — if the matrix unit were not exact within the budget this is where it shows."""
    from sad_amd import ops
    c = bl.plain_case(7, 37, [48, 40])
    bl.assert_stats("smallest plain rows", c.stats, ["positive"])
    assert _rows_form(37, [48, 40], True, _cus(dev)) == "rows1 NT2 single-ahead"
    mlp = ops.PackedMLPBf16(c.layers, False, dev)
    _exact(mlp.rows(_t(c.x, dev).bfloat16()).cpu().numpy(), c.want, "rows [48, 40] x 37")


PLAIN = [
    # (rows, dims, relu_mask, x dtype, form the launcher picks)
    (300, [64, 128], None, "f32", "rows1 NT4 single-ahead"),
    (129, [40, 72], None, "bf16", "rows1 NT4 single-ahead"),          # kin not a multiple of 16
    (500, [768, 96], None, "f32", "rows1 NT4 deep"),
    (66_000, [384, 128], None, "f32", "rows1 NT4 single-ahead"),      # a deep layer on a large grid
    (1000, [128, 64], None, "bf16", "rows2 NTW1"),
    (777, [256, 256], None, "bf16", "rows2 NTW2"),
    (40_000, [128, 64], None, "bf16", "rows2 NTW1 many-blocks"),
    (2000, [1536, 512], None, "bf16", "rows2 NTW2"),
    (256, [512, 256, 256, 10], 0b011, "bf16", "tiled"),              # head-like chain, last layer without ReLU
    (64, [33, 40, 50, 60, 70], None, "f32", "tiled"),
]


@pytest.mark.parametrize("rows,dims,mask,xdt,form", PLAIN)
def test_plain_rows_exact(sad, dev, rows, dims, mask, xdt, form):
    import torch
    from sad_amd import ops
    c = bl.plain_case(rows + sum(dims), rows, dims, relu_mask=mask)
    bl.assert_stats(f"rows {dims} x {rows}", c.stats, _chain_limits(c))
    assert _rows_form(rows, dims, xdt == "bf16", _cus(dev)) == form, "this case no longer reaches the form it is named for"
    last_relu = bool((c.relu_mask >> (len(dims) - 2)) & 1)
    mlp = ops.PackedMLPBf16(c.layers, False, dev, relu_mask=mask)
    x = _t(c.x, dev).bfloat16() if xdt == "bf16" else _t(c.x32, dev)
    _exact(mlp.rows(x).cpu().numpy(), c.want, f"{form} {dims} x {rows} f32 out", last_relu)
    w16 = bl.bf16(c.want)
    _exact(mlp.rows(x, out_dtype=torch.bfloat16).float().cpu().numpy(), w16, f"{form} bf16 out", last_relu)
    co = dims[-1]
    buf = torch.full((rows, co + 24), -7.0, device=dev, dtype=torch.bfloat16)
    mlp.rows(x, out=buf, col_off=8)
    b = buf.float().cpu().numpy()
    _exact(b[:, 8:8 + co], w16, f"{form} bf16 slice", last_relu)
    assert (b[:, :8] == -7).all() and (b[:, 8 + co:] == -7).all(), "written outside the slice"
    if form.startswith("rows2"):     # the first form forced on the same rows
        from sad_amd import _lib
        try:
            _lib.set_option("mlp_rows_form", 1)
            assert _rows_form(rows, dims, True, _cus(dev), form1=True).startswith("rows1")
            g1 = mlp.rows(x).cpu().numpy()
        finally:
            _lib.set_option("mlp_rows_form", 0)
        _exact(g1, c.want, f"forced first form {dims} x {rows}", last_relu)


# ---- grouped: the tiled kernel (geometry 0 and 32 .. 256 rows per tile) ---------------------------------------------------------------
TILED = [
    # (B, N, M, S, C, mlp, mode)
    (2, 600, 150, 32, 16, [32, 64], "any"),
    (1, 700, 90, 24, 8, [32, 48], "any"),             # nsample not a power of two
    (2, 400, 80, 64, 5, [24, 40], "full"),            # feature width not a multiple of 8
]


@pytest.mark.parametrize("B,N,M,S,C,mlp,mode", TILED)
def test_grouped_tiled_geometries_exact(sad, dev, B, N, M, S, C, mlp, mode):
    import ctypes
    import torch
    from sad_amd import ops, _lib
    c = bl.grouped_case(B * N + M + S + C, B, N, M, S, C, mlp, mode)
    bl.assert_stats(f"tiled {[C + 3] + mlp} S={S}", c.stats, _chain_limits(c, ["off_first"]))
    net = ops.PackedMLPBf16(c.layers, True, dev)
    X, Cn, I, K = _t(c.xyz, dev), _t(c.new_xyz, dev), _t(c.idx, dev), _t(c.cnt, dev)
    for fname, F in (("bf16", _t(c.feat, dev).bfloat16()), ("f32", _t(c.feat32, dev))):
        for geom in (0, 32, 64, 128, 256):
            for cnt in (None, K):
                a, out, keep = net._grouped_args(X, F, Cn, I, None, 0, cnt)
                a.geometry = geom
                rc = _lib.lib().sad_mlp_chain_bf16(ctypes.byref(a), torch.cuda.current_stream().cuda_stream)
                assert rc == 0, _lib.lib().sad_last_error()
                _exact(out.cpu().numpy(), c.want, f"tiled geometry {geom} {fname} features cnt={'yes' if cnt is not None else 'no'}")


# ---- grouped: the register-resident chain (geometry 2), all ten compiled shapes ------------------------------------------------------
REG = [
    # (shape id of kShapes, B, N, M, S, C, mlp, feat, mode)
    (0, 2, 800, 200, 32, 1, [16, 16, 32], "f32", "any"),       # SA1 narrow: one f32 channel of a strided point array
    (0, 2, 800, 150, 32, 4, [16, 16, 32], "f32", "few"),       # nuScenes SA1: four f32 channels, row stride 7
    (1, 2, 800, 100, 64, 1, [32, 32, 64], "f32", "full"),      # groups across three tiles
    (2, 2, 600, 120, 32, 64, [64, 64, 128], "bf16", "any"),
    (3, 2, 600, 80, 64, 64, [64, 96, 128], "bf16", "full"),
    (4, 2, 500, 80, 32, 128, [128, 128, 256], "bf16", "few"),
    (5, 2, 500, 70, 32, 128, [128, 192, 256], "bf16", "any"),
    (6, 1, 500, 90, 32, 128, [128, 256, 256], "bf16", "any"),
    (7, 2, 500, 120, 32, 0, [64, 64, 128], None, "any"),
    (7, 1, 500, 100, 16, 13, [64, 64, 128], "bf16", "any"),   # narrow bf16 features (element-wise loads)
    (8, 1, 400, 70, 16, 256, [256, 256, 512], "bf16", "any"),
    (9, 1, 400, 40, 32, 256, [256, 512, 1024], "bf16", "few"),
]


def _feat_tensor(c, fdt, dev):
    import torch
    if fdt is None:
        return None
    if fdt == "f32":        # a strided view of the point rows, as the detector's first stage reads them
        B, N, C = c.feat32.shape
        pts = np.zeros((B, N, 3 + C), np.float32)
        pts[:, :, :3] = c.xyz
        pts[:, :, 3:] = c.feat32
        return _t(pts, dev)[:, :, 3:]
    return _t(c.feat, dev).bfloat16()


@pytest.mark.parametrize("shape,B,N,M,S,C,mlp,fdt,mode", REG)
def test_register_chain_exact(sad, dev, shape, B, N, M, S, C, mlp, fdt, mode):
    import torch
    from sad_amd import ops
    c = bl.grouped_case(100 * shape + S + C + M, B, N, M, S, C, mlp, mode)
    keys = _chain_limits(c, ["off_first"] + (["straddle_only"] if mode != "full" or S == 64 else []))
    bl.assert_stats(f"register chain shape {shape} {[C + 3] + mlp} S={S} {mode}", c.stats, keys)
    net = ops.PackedMLPBf16(c.layers, True, dev)
    assert net.preferred_geometry == 2, "not a compiled shape of the register-resident chain"
    net.default_geometry = 2
    X, Cn, I, K = _t(c.xyz, dev), _t(c.new_xyz, dev), _t(c.idx, dev), _t(c.cnt, dev)
    F = _feat_tensor(c, fdt, dev)
    _exact(net.grouped(X, F, Cn, I, cnt=K).cpu().numpy(), c.want, f"register chain shape {shape} (own scan)")
    ws = ops.rowscan_multi([I], [K], N)[0]
    _exact(net.grouped(X, F, Cn, I, cnt=K, ws=ws).cpu().numpy(), c.want, f"register chain shape {shape} (rowscan_multi table)")
    if shape in (2, 4, 8, 9):      # an unaligned output slice: element-wise stores and per-channel atomics with their own bounds
        co, off = mlp[-1], 5
        buf = torch.full((B, M, co + 13), -7.0, device=dev, dtype=torch.float32)
        buf[:, :, off:off + co] = 0.0
        net.grouped(X, F, Cn, I, out=buf, col_off=off, cnt=K)
        b = buf.cpu().numpy()
        _exact(b[:, :, off:off + co], c.want, f"register chain shape {shape} unaligned slice")
        assert (b[:, :, :off] == -7).all() and (b[:, :, off + co:] == -7).all(), "written outside the slice"


SA3 = (2, 500, 100, 128, 32)        # B, N, M, C, S


def sa3_branches():
    """The three SA3 branches on one point set and one set of centres (one ball query): (base case, [(case, x0, pooled oracle)])."""
    B, N, M, C, S = SA3
    mlps = ([128, 128, 256], [128, 192, 256], [128, 256, 256])
    cases = [bl.grouped_case(900 + i, B, N, M, S, C, m, ("any", "few", "full")[i]) for i, m in enumerate(mlps)]
    base = cases[0]
    out = []
    for i, c in enumerate(cases):
        x0 = bl.layer0_rows(base.xyz, base.feat, base.new_xyz, c.idx)
        y, recs = bl.forward_exact(x0, c.layers)
        st = bl.chain_stats(recs)
        st.update(bl.group_stats(y, c.cnt, S))
        bl.assert_stats(f"SA3 branch {i}", st, ["rounded", "ties", "positive", "off_first", "straddle_only"])
        out.append((c, x0, y.reshape(B * M, S, -1).max(axis=1).reshape(B, M, -1) + np.float32(0)))
    return base, out


def test_grouped_multi_sa3_branches_exact(sad, dev):
    """The three SA3 branches as one register-resident dispatch (sad_mlp_chain_multi_bf16), each against the oracle."""
    import torch
    from sad_amd import ops
    B, N, M, C, S = SA3
    base, branches = sa3_branches()
    X, Cn, F = _t(base.xyz, dev), _t(base.new_xyz, dev), _t(base.feat, dev).bfloat16()
    idxs = [_t(c.idx, dev) for c, _, _ in branches]
    cnts = [_t(c.cnt, dev) for c, _, _ in branches]
    wss = ops.rowscan_multi(idxs, cnts, N)
    out = torch.zeros((B, M, 768), device=dev)
    calls, wants = [], []
    for i, (c, _, want) in enumerate(branches):
        wants.append(want)
        calls.append((ops.PackedMLPBf16(c.layers, True, dev), X, F, Cn, idxs[i], out, 256 * i, cnts[i], wss[i]))
    ops.grouped_multi(calls)
    got = out.cpu().numpy()
    for i in range(3):
        _exact(got[:, :, 256 * i:256 * (i + 1)], wants[i], f"merged SA3 dispatch, branch {i}")


# ---- split pooling (cont) and the layer that reads it --------------------------------------------------------------------------------
SPLIT = {
    # name: (B, N, M, [(S, C, mlp, mode)], agg out)
    "one chain, 64-row groups": (2, 500, 100, [(64, 64, [64, 64, 128], "full")], 64),
    "three chains": (2, 500, 120, [(32, 64, [64, 64, 128], "any"), (64, 64, [64, 96, 128], "full"), (16, 64, [64, 64, 128], "few")], 128),
    "four chains": (2, 600, 150, [(16, 0, [16, 16, 32], "any"), (32, 0, [32, 32, 64], "any"), (64, 0, [32, 32, 64], "full"),
                                  (32, 0, [16, 16, 32], "few")], 96),
    "many row blocks": (1, 4000, 33_000, [(8, 0, [16, 16, 32], "any"), (16, 0, [16, 16, 32], "any"), (16, 0, [32, 32, 64], "few")], 64),
}


def split_case(name):
    """The lattice data of one split-pooling case: points, per-chain (S, mlp, idx, cnt, layers, x0), the reading layer and its oracle
    on bf16(pooled); every chain's statistics are asserted."""
    B, N, M, specs, agg_out = SPLIT[name]
    rng = np.random.default_rng(len(name))
    xyz = bl.lattice_xyz(rng, (B, N, 3))
    new_xyz = bl.lattice_xyz(rng, (B, M, 3))
    C = specs[0][1]
    feat = bl.lattice_feat(rng, (B, N, C)) if C else None
    chains, pooled, two = [], [], 0
    for i, (S, C_, mlp, mode) in enumerate(specs):
        idx, cnt = bl.random_groups(rng, B, N, M, S, mode)
        x0 = bl.layer0_rows(xyz, feat, new_xyz, idx)
        layers, _ = bl.lattice_chain([C + 3] + mlp, x0, rng, nnz=4)      # (sparser: the reading layer adds a fourth layer to the budget)
        y, recs = bl.forward_exact(x0, layers)
        st = bl.chain_stats(recs)
        st.update(bl.group_stats(y, cnt, S))
        two += st["two_cont"]
        bl.assert_stats(f"split {name} chain {i} S={S} {mode}", st, ["rounded", "ties", "positive", "off_first", "straddle_only"])
        pooled.append(y.reshape(B * M, S, -1).max(axis=1))
        chains.append((S, mlp, idx, cnt, layers, x0))
    cat = bl.bf16(np.concatenate(pooled, axis=1))
    agg_layers, _ = bl.lattice_chain([cat.shape[1], agg_out], cat, rng, nnz=4, kmax=1)
    want, recs = bl.forward_exact(cat, agg_layers)
    st = bl.chain_stats(recs)
    st["groups_over_three_tiles"] = two
    bl.assert_stats(f"split {name} reading layer", st, ["positive"])
    if any(s[0] == 64 and s[3] == "full" for s in specs):
        assert two > 0, "no group spans three tiles: the second continuation row is not exercised"
    return xyz, feat, new_xyz, chains, cat, agg_layers, want


@pytest.mark.parametrize("name", list(SPLIT))
def test_split_pooling_and_reading_layer_exact(sad, dev, name):
    """Chains with split pooling (bf16 rows + continuation rows), then the aggregation layer that takes the maximum as it reads them
    (rows(..., pool=...)) — both forms of the reading layer — against the oracle chained through bf16(pooled)."""
    import torch
    from sad_amd import _lib, ops
    B, N, M, specs, agg_out = SPLIT[name]
    xyz, feat, new_xyz, chains, cat, agg_layers, want = split_case(name)
    X, Cn = _t(xyz, dev), _t(new_xyz, dev)
    F = _t(feat, dev).bfloat16() if feat is not None else None
    cat_c = cat.shape[1]
    cat16 = torch.full((B, M, cat_c), 9.0, device=dev, dtype=torch.bfloat16)
    calls, outs, idxs, cnts, conts, off = [], [], [], [], [], 0
    for S, mlp, idx, cnt, layers, _ in chains:
        net = ops.PackedMLPBf16(layers, True, dev)
        assert net.preferred_geometry == 2
        I, K = _t(idx, dev), _t(cnt, dev)
        cont = ops.cont_buffer(B, M, S, mlp[-1], dev)
        cont.fill_(0x7F)
        calls.append([net, X, F, Cn, I, cat16, off, K, None, cont])
        outs.append((cat16, off, mlp[-1], cont))
        idxs.append(I); cnts.append(K); conts.append(cont)
        off += mlp[-1]
    wss = ops.rowscan_multi(idxs, cnts, N, outs)
    for c, w in zip(calls, wss):
        c[8] = w
    if len(calls) > 1:
        ops.grouped_multi([tuple(c) for c in calls])
    else:
        c = calls[0]
        c[0].grouped(*c[1:5], out=cat16, col_off=0, cnt=c[7], ws=c[8], cont=c[9])
    agg = ops.PackedMLPBf16(agg_layers, False, dev)
    pool = [(w, k, s[0], s[2][-1]) for w, k, s in zip(wss, conts, specs)]
    rows = B * M
    form = _rows_form(rows, [cat_c, agg_out], True, _cus(dev))
    print(f"[exact-bf16] {name}: reading layer {form}")
    _exact(agg.rows(cat16, pool=pool).cpu().numpy().reshape(rows, -1), want, f"split {name}: reading layer ({form})")
    _exact(agg.rows(cat16, out_dtype=torch.bfloat16, pool=pool).float().cpu().numpy().reshape(rows, -1), bl.bf16(want),
           f"split {name}: reading layer, bf16 out")
    try:
        _lib.set_option("mlp_rows_form", 1)
        g1 = agg.rows(cat16, pool=pool).cpu().numpy().reshape(rows, -1)
    finally:
        _lib.set_option("mlp_rows_form", 0)
    _exact(g1, want, f"split {name}: reading layer, first form")
    if name == "many row blocks":
        assert (rows + 127) // 128 > _cus(dev)


# ---- signed zeros ------------------------------------------------------------------------------------------------------------------------
def _neg_zero_layer(cin, cout, rng, q=2.0 ** -8):
    """One layer whose even channels have a -0 bias, negative weights on the three xyz columns and positive weights on every
    feature column (so a row with rel_xyz = +0 and features -0 sums only -0 products there); odd channels are lattice values."""
    W = (rng.integers(1, 4, size=(cout, cin)) * q * 8).astype(np.float32)
    W[:, :3] *= -1
    qp = 2.0 ** -(bl.XYZ_BITS + 5)                          # the product quantum: rel_xyz 2^-10 times weights 2^-5
    b = (np.round(rng.uniform(-0.5, 0.5, cout) / qp) * qp).astype(np.float32)
    b[0::2] = -0.0
    W[1::2] *= rng.choice([-1, 1], size=(cout // 2, cin)).astype(np.float32)
    return W, b


def _probe(mlp, x, form):
    y = mlp.rows(x).cpu().numpy()
    neg = int(np.signbit(y[:, 0::2]).sum())
    print(f"[signed-zero probe] {form}: {neg} of {y[:, 0::2].size} sums of -0 products on a -0 bias came out as -0")
    return neg


def test_signed_zero_probe(sad, dev):
    """Does the matrix unit give -0 for a sum of -0 products on a -0 bias?  One plain layer without ReLU (the sign is visible),
    rows of +0 against negative weights, in the three plain-row forms.  The answer is printed; the sums' values must be zero."""
    import torch
    from sad_amd import ops
    rng = np.random.default_rng(0)
    res = {}
    for form, cin, xdt, geom in (("rows2", 64, "bf16", 0), ("rows1", 64, "f32", 0), ("tiled", 16, "bf16", 32)):
        W = -(rng.integers(1, 4, size=(32, cin)) * 2.0 ** -3).astype(np.float32)
        b = np.full(32, -0.0, np.float32)
        b[1::2] = 0.0
        x = np.zeros((64, cin), np.float32)
        mlp = ops.PackedMLPBf16([(W, b)], False, dev, relu_mask=0)
        mlp.default_geometry = geom
        xt = _t(x, dev).bfloat16() if xdt == "bf16" else _t(x, dev)
        assert _rows_form(64, [cin, 32], xdt == "bf16", _cus(dev)).startswith(form) or form == "tiled"
        res[form] = _probe(mlp, xt, form)
        y = mlp.rows(xt).cpu().numpy()
        assert (y == 0).all()
        relu = ops.PackedMLPBf16([(W, b)], False, dev)
        relu.default_geometry = geom
        r = relu.rows(xt).cpu().numpy()
        assert not np.signbit(r).any(), f"{form}: a ReLU let -0 through"
    print(f"[signed-zero probe] -0 reached: {res}" + ("" if any(res.values()) else
          "  -> the matrix unit never gives -0 here: a pooling that lets -0 through cannot be caught on this hardware"))


SZ = (2, 300, 120, 32, 13, 32)      # B, N, M, S, C, C_out   (C + 3 = 16: no padding column in the first k-step)


def signed_zero_case():
    """Lattice points where every even-numbered centre is a point with -0 features (its own row: rel_xyz = +0), groups of 1 .. S rows,
    and a `_neg_zero_layer`.  Returns (xyz, feat, new_xyz, idx, cnt, (W, b), x0 of SPEC §14, f32 rows of SPEC §6, rows_neg0)."""
    B, N, M, S, C, co = SZ
    rng = np.random.default_rng(5)
    xyz = bl.lattice_xyz(rng, (B, N, 3))
    feat = bl.lattice_feat(rng, (B, N, C))
    zero_pts = rng.choice(N, size=N // 3, replace=False)
    feat[:, zero_pts] = -0.0
    idx, cnt = bl.random_groups(rng, B, N, M, S, "any")
    for b in range(B):
        for m in range(0, M, 2):
            idx[b, m, 0] = zero_pts[rng.integers(len(zero_pts))]
            idx[b, m, cnt[b, m]:] = idx[b, m, 0]
    new_xyz = np.stack([xyz[b][idx[b, :, 0]] for b in range(B)])
    W, bias = _neg_zero_layer(C + 3, co, rng)
    x0 = bl.layer0_rows(xyz, feat, new_xyz, idx)
    rows32 = np.concatenate([np.concatenate([xyz[b][idx[b].reshape(-1)] - np.repeat(new_xyz[b], S, 0), feat[b][idx[b].reshape(-1)]], 1)
                             for b in range(B)], 0).astype(np.float32)
    # rows that sum only -0 products on a -0 bias (in IEEE order -0 + -0 stays -0)
    rows_neg0 = np.signbit(x0[:, 3:]).all(axis=1) & (x0[:, :3] == 0).all(axis=1) & ~np.signbit(x0[:, :3]).any(axis=1)
    return xyz, feat, new_xyz, idx, cnt, (W, bias), x0, rows32, rows_neg0


@pytest.mark.parametrize("kind", ["bf16", "f32"])
def test_signed_zeros_into_pooling(sad, dev, kind):
    """Rows whose every product on a channel is -0 (rel_xyz = +0 with negative weights, features -0 with positive weights) on a -0
    bias, in groups that straddle tiles where other rows give positive values on the same channel: the pooled maxima must equal the
    oracle's bits — no positive max lost to the unsigned atomicMax, every zero +0.  Every grouped kernel that takes a one-layer chain:
    the bf16 tiled kernel at every geometry, the f32 chain at every forced geometry code (mlp_force, as test_gpu_mlp)."""
    import ctypes
    import torch
    from sad_amd import _lib, ops
    B, N, M, S, C, co = SZ
    xyz, feat, new_xyz, idx, cnt, (W, bias), x0, rows32, rows_neg0 = signed_zero_case()
    rows = x0 if kind == "bf16" else rows32          # (SPEC §6: the f32 chain does not round rel_xyz)
    y, recs = bl.forward_exact(rows, [(W, bias)])
    bl.check_budget(recs)
    st = bl.group_stats(y, cnt, S)
    grp_mix = (rows_neg0.reshape(B * M, S) & (np.arange(S)[None, :] < cnt.reshape(-1, 1))).any(axis=1)
    pos = (y.reshape(B * M, S, -1)[:, :, 0::2].max(axis=1) > 0).any(axis=1)
    print(f"[signed zeros] {int(rows_neg0.sum())} all -0 rows, {int((grp_mix & pos).sum())} groups with such a row and a positive "
          f"max on a -0-bias channel, straddle_only={st['straddle_only']}")
    assert rows_neg0.sum() > 0 and (grp_mix & pos).sum() > 0 and st["straddle_only"] > 0
    want = y.reshape(B * M, S, -1).max(axis=1).reshape(B, M, -1) + np.float32(0)
    X, Cn, I, K = _t(xyz, dev), _t(new_xyz, dev), _t(idx, dev), _t(cnt, dev)
    if kind == "bf16":
        net = ops.PackedMLPBf16([(W, bias)], True, dev)
        F = _t(feat, dev).bfloat16()
        for geom in (0, 32, 64, 128, 256):
            for cn in (None, K):
                a, out, keep = net._grouped_args(X, F, Cn, I, None, 0, cn)
                a.geometry = geom
                rc = _lib.lib().sad_mlp_chain_bf16(ctypes.byref(a), torch.cuda.current_stream().cuda_stream)
                assert rc == 0, _lib.lib().sad_last_error()
                _exact(out.cpu().numpy(), want, f"bf16 tiled geometry {geom} cnt={'yes' if cn is not None else 'no'}")
        return
    # the f32 pre-activations of these rows, measured: one plain layer without ReLU on the same rows
    pre = ops.PackedMLP([(W, bias)], False, dev, relu_mask=0).rows(_t(rows32, dev)).cpu().numpy()
    neg0 = int((np.signbit(pre[:, 0::2]) & (pre[:, 0::2] == 0)).sum())
    print(f"[signed zeros] f32 chain: {neg0} of {int(rows_neg0.sum()) * (co // 2)} all -0 sums are -0 before the ReLU")
    net = ops.PackedMLP([(W, bias)], True, dev)
    F = _t(feat, dev)
    codes = [0] + list(ops.PackedMLP._CANDIDATES)
    codes += [c + 1000 * f for c in (801, 811, 100811) for f in ops.PackedMLP._F_CODES]
    codes += [c + 10000 * d for c in (801, 821, 100821, 5811) for d in (1, 2)]
    ran = 0
    try:
        for code in codes:
            _lib.set_option("mlp_force", code)
            for cn in (None, K):
                try:
                    got = net.grouped(X, F, Cn, I, cnt=cn).cpu().numpy()
                except RuntimeError as e:
                    assert "(-2)" in str(e), f"geometry {code}: {e}"      # SAD_EUNSUPPORTED only
                    continue
                _exact(got, want, f"f32 chain geometry {code} cnt={'yes' if cn is not None else 'no'}")
                ran += 1
    finally:
        _lib.set_option("mlp_force", 0)
    assert ran >= 20, f"only {ran} f32 geometries ran"


# ---- stage level: the detector backbone, no teacher forcing ------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg_name,batch,xyz_bits", [("TINY", 2, 10), ("KITTI", 2, 12), ("NUSCENES", 1, 12)])
def test_detector_backbone_exact(orc, sad, dev, cfg_name, batch, xyz_bits):
    """Lattice points (xyz on 2^-xyz_bits, extra channels binary32 stand-ins of bf16 values, ties included) and lattice weights for every
    sa* chain: tr["sa1..3"]["out"] of the traced eager path equal, bit for bit, the SPEC §14 oracle chained from the raw points.  Then the
    same batch through submit() with recorded and replayed plans and split pooling: the boxes of the traced eager run, bit for bit."""
    import torch
    from sad_amd import config, ops, synth
    from sad_amd.detector import SADDetector
    cfg = getattr(config, cfg_name)
    rng = np.random.default_rng(31)
    make = {"TINY": synth.make_tiny_batch, "KITTI": synth.make_batch, "NUSCENES": synth.make_nuscenes_batch}[cfg_name]
    pts = bl.snap_points(make(0, batch, cfg.n_points), xyz_bits, rng)
    w = synth.make_weights(cfg, 0)                # cand / cluster / head: off the lattice anyway
    want, stats = bl.backbone_lattice(orc, cfg, pts, rng, w)
    for name, st in stats.items():
        bl.assert_stats(f"{cfg_name} {name}", st, ["rounded", "ties", "positive"])
        # (ball-query groups of real scenes are mostly padding — a repeated first point — on the sparse KITTI scenes: a lower bar)
        assert st["off_first"] > 0.1, f"{cfg_name} {name}: off_first = {st['off_first']:.3f} (the case tests too little)"
    P = _t(pts, dev)
    det = SADDetector(cfg, w, dev, dtype="bf16")
    tr = {}
    boxes = det(P, tr)
    torch.cuda.synchronize()
    for name in want:
        assert tr[name]["out"].dtype == torch.bfloat16
        _exact(tr[name]["out"].float().cpu().numpy(), want[name], f"{cfg_name} B={batch} {name} out, chained from the raw points")
    assert ops.SPLIT_POOL, "split pooling is off in this environment"
    sub = SADDetector(cfg, w, dev, dtype="bf16", streams=(det._sides, det._mains))
    for _ in range(sub._plan_ring + 3):               # recorded and replayed steps
        out, ev = sub.submit(P)
    ev.synchronize()
    assert sub.plan_refused is None and sub.plan_replays >= 3
    n_in = [cfg.n_points] + [s.npoint for s in cfg.stages[:-1]]
    assert all(m.can_split(batch, n, m.stage.npoint, feat_dtype=torch.bfloat16 if i else torch.float32)
               for i, (m, n) in enumerate(zip(sub.stages, n_in))), "submit() no longer takes the split-pooling path"
    assert torch.equal(out, boxes), f"submit() boxes differ from the traced eager boxes: {(out - boxes).abs().max().item()}"
