"""The premise of the bit-exact bf16 tests (tests/bf16_lattice.py, tests/test_gpu_bf16_exact.py), shown on the CPU.

* Premise: on every lattice case the GPU file uses, binary32 accumulation in ANY order — sequential over random permutations of k,
  16-product blocks summed exactly and then rounded into the accumulator like a matrix unit, the same with truncation — gives the
  bits of the oracle (binary64 sum, one rounding).  On synth.make_mlp_weights data it does not: the emulation can see order at all.
* The gap: the bad kernel variants the exact tests are meant to catch, emulated here, differ from the oracle on lattice cases; whether
  SPEC §14's tolerance (test_gpu_bf16._close) would see them on random data is printed.
* The generator's invariants: the budget holds and every case's statistics are met.
"""
import functools

import numpy as np
import pytest

import bf16_lattice as bl
from test_gpu_bf16_exact import PLAIN, REG, SPLIT, TILED, _chain_limits, sa3_branches, signed_zero_case, split_case

SUB = 96          # rows per case for the accumulation emulations (exactness is per row)


@functools.lru_cache(maxsize=None)
def _plain(i):
    rows, dims, mask, _, _ = PLAIN[i]
    return bl.plain_case(rows + sum(dims), rows, dims, relu_mask=mask)


@functools.lru_cache(maxsize=None)
def _reg(i):
    shape, B, N, M, S, C, mlp, _, mode = REG[i]
    return bl.grouped_case(100 * shape + S + C + M, B, N, M, S, C, mlp, mode)


@functools.lru_cache(maxsize=None)
def _tiled(i):
    B, N, M, S, C, mlp, mode = TILED[i]
    return bl.grouped_case(B * N + M + S + C, B, N, M, S, C, mlp, mode)


def _f32_trunc(s):
    """binary64 -> binary32 rounded toward zero."""
    f = s.astype(np.float32)
    over = np.abs(f.astype(np.float64)) > np.abs(s)
    f[over] = np.nextafter(f[over], np.float32(0))
    return f


def _acc_layer(xb, Wb, b, mode, rng):
    """y = b + Σ_k Wb·xb accumulated in binary32 (xb, Wb: bf16 values, products exact).  mode: 'seq' — one addition at a time in a
    random order of k; 'block' / 'block_trunc' — 16 products summed exactly, the block rounded (to nearest / toward zero) into the
    accumulator, blocks in a random order."""
    R, K = xb.shape
    out = np.empty((R, Wb.shape[0]), np.float32)
    step = max(1, 4_000_000 // (Wb.size + 1))
    for r0 in range(0, R, step):
        P = xb[r0:r0 + step, None, :] * Wb[None, :, :]
        acc = np.broadcast_to(np.asarray(b, np.float32), P.shape[:2]).copy()
        if mode == "seq":
            for k in rng.permutation(K):
                acc = acc + P[:, :, k].astype(np.float32)
        else:
            blocks = list(range(0, K, 16))
            for i in rng.permutation(len(blocks)):
                s = acc.astype(np.float64) + P[:, :, blocks[i]:blocks[i] + 16].sum(axis=2)
                acc = s.astype(np.float32) if mode == "block" else _f32_trunc(s)
        out[r0:r0 + step] = acc
    return out


def _chain_emulated(x, layers, relu_mask, mode, rng):
    x = bl.bf16(np.asarray(x, np.float32)).astype(np.float64)
    L = len(layers)
    for l, (W, b) in enumerate(layers):
        y = _acc_layer(x, bl.bf16(np.asarray(W, np.float32)).astype(np.float64), b, mode, rng)
        if (relu_mask >> l) & 1:
            y = np.where(y > 0, y, np.float32(0))
        x = bl.bf16(y).astype(np.float64)
    return y


def _lattice_rows():
    """(name, rows, layers, relu_mask) of every lattice case the GPU file uses, SUB rows each."""
    out = []
    for i in range(len(PLAIN)):
        c = _plain(i)
        out.append((f"plain {PLAIN[i][1]}", c.x32[:SUB], c.layers, c.relu_mask))
    for i in range(len(REG)):
        c = _reg(i)
        out.append((f"register chain {REG[i][0]}", c.x0[::max(1, len(c.x0) // SUB)][:SUB], c.layers, 7))
    for i in range(len(TILED)):
        c = _tiled(i)
        out.append((f"tiled {TILED[i][5]}", c.x0[::max(1, len(c.x0) // SUB)][:SUB], c.layers, (1 << len(c.layers)) - 1))
    c = bl.plain_case(7, 37, [48, 40])                                     # test_smallest_plain_rows_case
    out.append(("smallest plain rows", c.x, c.layers, 1))
    _, branches = sa3_branches()
    for i, (c, x0, _) in enumerate(branches):
        out.append((f"SA3 branch {i}", _sub(x0), c.layers, 7))
    for name in SPLIT:
        _, _, _, chains, cat, agg_layers, _ = split_case(name)
        for S, mlp, _, _, layers, x0 in chains:
            out.append((f"split {name} chain S={S} {mlp}", _sub(x0), layers, 7))
        out.append((f"split {name} reading layer", _sub(cat), agg_layers, 1))
    _, _, _, _, _, layer, x0, rows32, _ = signed_zero_case()
    out.append(("signed zeros, bf16", _sub(x0), [layer], 1))
    return out


def _sub(x):
    return x[::max(1, len(x) // SUB)][:SUB]


@pytest.mark.parametrize("mode", ["seq", "block", "block_trunc"])
def test_every_summation_order_gives_the_oracle_bits_on_the_lattice(orc, mode):
    rng = np.random.default_rng(1)
    for name, x, layers, mask in _lattice_rows():
        want = orc.mlp_rows_bf16(x, layers, relu_mask=mask) + np.float32(0)
        for _ in range(2):
            got = _chain_emulated(x, layers, mask, mode, rng) + np.float32(0)
            last_relu = bool((mask >> (len(layers) - 1)) & 1)
            same = np.array_equal(got.view(np.uint32), want.view(np.uint32)) if last_relu else np.array_equal(got, want)
            assert same, f"{name}: {mode} accumulation differs from the oracle on a lattice case (the budget is not enough)"


def test_the_emulation_sees_order_on_random_data(orc):
    """Without the lattice the same emulations do not all give the oracle's bits."""
    from sad_amd import synth
    rng = np.random.default_rng(2)
    dims = [128, 128, 256]
    layers = synth.make_mlp_weights(dims, rng)
    x = rng.normal(size=(SUB, dims[0])).astype(np.float32)
    want = orc.mlp_rows_bf16(x, layers)
    differ = {m: int((_chain_emulated(x, layers, 3, m, rng) != want).sum()) for m in ("seq", "block", "block_trunc")}
    print(f"[lattice] random data, elements that differ from the oracle: {differ}")
    assert max(differ.values()) > 0


# ---- the mutants ------------------------------------------------------------------------------------------------------------------------
def _chain_variant(x, layers, relu_mask=None, bias_bf16=False, act=bl.bf16):
    """The oracle's chain (binary64 sums) with one deliberate fault."""
    L = len(layers)
    relu_mask = (1 << L) - 1 if relu_mask is None else relu_mask
    y = np.asarray(x, np.float32)
    for l, (W, b) in enumerate(layers):
        xb = (bl.bf16(y) if l == 0 else act(y)).astype(np.float64)
        Wb = bl.bf16(np.asarray(W, np.float32)).astype(np.float64)
        bb = bl.bf16(b) if bias_bf16 else np.asarray(b, np.float32)
        y = (xb @ Wb.T + bb.astype(np.float64)).astype(np.float32)
        if (relu_mask >> l) & 1:
            y = np.where(y > 0, y, np.float32(0))
    return y


def _rows_of(c, rel_fn=None, feat=None):
    B, M, S = c.idx.shape
    out = []
    for b in range(B):
        j = c.idx[b].reshape(-1)
        cen = np.repeat(c.new_xyz[b], S, 0)
        rel = (c.xyz[b][j] - cen) if rel_fn is None else rel_fn(c.xyz[b][j], cen)
        f = c.feat if feat is None else feat
        out.append(rel.astype(np.float32) if f is None else np.concatenate([rel.astype(np.float32), f[b][j]], 1))
    return np.concatenate(out, 0)


def _pool(y, c):
    B, M, S = c.idx.shape
    return y.reshape(B * M, S, -1).max(axis=1) + np.float32(0)


def _pool_two_tiles(y, c):
    """Split pooling that drops the second continuation row: a group's rows in its third 32-row tile are lost."""
    B, M, S = c.idx.shape
    cnt = np.maximum(c.cnt.reshape(-1), 1)
    gs = np.concatenate([[0], np.cumsum(cnt)])
    keep = np.arange(S)[None, :] < np.minimum(cnt, ((gs[:-1] >> 5) + 2) * 32 - gs[:-1])[:, None]
    yy = np.where(keep[:, :, None], y.reshape(B * M, S, -1), -np.inf)
    return yy.max(axis=1) + np.float32(0)


def _signed_zero_rows():
    """One-layer rows: some sum only -0 products on a -0 bias (rel_xyz +0 against negative weights, features -0 against positive)."""
    rng = np.random.default_rng(3)
    G, S, C = 64, 32, 13
    x = bl.lattice_feat(rng, (G, S, C + 3))
    x[:, :, :3] = bl.lattice_xyz(rng, (G, S, 3)) - 0.5
    x[:, 0, :3] = 0.0
    x[:, 0, 3:] = -0.0
    W = (rng.integers(1, 4, size=(32, C + 3)) * 2.0 ** -5).astype(np.float32)
    W[:, :3] *= -1
    b = np.round(rng.uniform(-0.5, 0.5, 32) * 2 ** 15) * 2.0 ** -15
    b[0::2] = -0.0
    return x.reshape(G * S, C + 3), W, b.astype(np.float32), G, S


def test_mutants_differ_from_the_oracle_on_the_lattice(orc):
    """Each bad variant of the kernels (tests/test_gpu_bf16_exact.py docstring) gives other bits than the oracle on lattice cases;
    printed: whether SPEC §14's tolerance would catch it on random data (it is not asserted)."""
    from sad_amd import synth
    plain = _plain(0)
    reg = _reg(2)            # three-layer register-chain case, 64-row groups across three tiles
    narrow = _reg(1)         # f32 features with ties
    want_reg = _pool(bl.forward_exact(bl.bf16(_rows_of(reg)), reg.layers)[0], reg)
    rng = np.random.default_rng(4)
    rdims = [67, 64, 64, 128]
    rl = synth.make_mlp_weights(rdims, rng)
    rx = rng.normal(size=(512, 67)).astype(np.float32)
    r_want = orc.mlp_rows_bf16(rx, rl)

    def tol(got, want):
        scale = max(float(np.abs(want).max()), 1e-6)
        d = np.abs(got.astype(np.float64) - want)
        return d.max() <= 1e-2 * scale and d.mean() <= 1e-5 * scale

    report = {}
    # 1. biases rounded to bf16 by the packer
    m1 = _chain_variant(plain.x32, plain.layers, plain.relu_mask, bias_bf16=True)
    assert not np.array_equal(m1, plain.want), "mutant 1 (bf16 bias) not visible on the lattice"
    report["1 bias rounded to bf16"] = tol(_chain_variant(rx, rl, bias_bf16=True), r_want)
    # 2. hidden activations truncated instead of rounded to nearest even
    m2 = _pool(_chain_variant(_rows_of(reg), reg.layers, act=bl.bf16_trunc), reg)
    assert not np.array_equal(m2, want_reg), "mutant 2 (truncated activations) not visible"
    report["2 activation truncated"] = tol(_chain_variant(rx, rl, act=bl.bf16_trunc), r_want)
    # 3. rel_xyz from bf16-rounded coordinates
    m3 = _pool(_chain_variant(_rows_of(reg, rel_fn=lambda p, c: bl.bf16(p) - bl.bf16(c)), reg.layers), reg)
    assert not np.array_equal(m3, want_reg), "mutant 3 (rel_xyz of rounded coordinates) not visible"
    rxyz = rng.uniform(-40, 40, size=(512, 3)).astype(np.float32)
    rcen = rxyz + rng.uniform(-0.5, 0.5, size=(512, 3)).astype(np.float32)
    ry = rng.normal(size=(512, 64)).astype(np.float32)
    r3_want = orc.mlp_rows_bf16(np.concatenate([rxyz - rcen, ry], 1), rl)
    report["3 rel_xyz of bf16 coordinates"] = tol(orc.mlp_rows_bf16(np.concatenate([bl.bf16(rxyz) - bl.bf16(rcen), ry], 1), rl), r3_want)
    # 4. f32 features truncated on load
    want_n = _pool(bl.forward_exact(bl.bf16(_rows_of(narrow, feat=narrow.feat32)), narrow.layers)[0], narrow)
    m4 = _pool(_chain_variant(_rows_of(narrow, feat=bl.bf16_trunc(narrow.feat32)), narrow.layers), narrow)
    assert not np.array_equal(m4, want_n), "mutant 4 (truncated f32 features) not visible"
    report["4 f32 features truncated"] = tol(orc.mlp_rows_bf16(np.concatenate([rx[:, :3], bl.bf16_trunc(rx[:, 3:])], 1), rl), r_want)
    # 5. the split-pooled reader drops the second continuation row
    y_reg = bl.forward_exact(bl.bf16(_rows_of(reg)), reg.layers)[0]
    assert not np.array_equal(_pool_two_tiles(y_reg, reg), want_reg), "mutant 5 (second continuation row) not visible"
    ry5 = orc.mlp_rows_bf16(rng.normal(size=(len(y_reg), 67)).astype(np.float32), rl)
    report["5 second continuation row dropped"] = tol(_pool_two_tiles(ry5, reg), _pool(ry5, reg))
    # 6. the pooling lets -0 through (needs a -0 out of the matrix unit: see test_gpu_bf16_exact.test_signed_zero_probe)
    x, W, b, G, S = _signed_zero_rows()
    xb = bl.bf16(x).astype(np.float64)
    acc = np.broadcast_to(b.astype(np.float64), (len(x), len(b))).copy()
    for k in range(x.shape[1]):                         # sequential IEEE additions: -0 + -0 = -0
        acc = acc + xb[:, k:k + 1] * W[None, :, k].astype(np.float64)
    y6 = np.where(acc >= 0, acc, 0.0).astype(np.float32)     # `m >= 0 ? m : 0` keeps -0
    m6 = y6.reshape(G, S, -1).view(np.uint32).max(axis=1).view(np.float32)     # unsigned atomicMax on the bits
    want6 = orc.mlp_rows_bf16(x, [(W, b)]).reshape(G, S, -1).max(axis=1) + np.float32(0)
    assert np.signbit(y6).any() and not np.array_equal(m6.view(np.uint32), want6.view(np.uint32)), "mutant 6 (-0 into the pooling) not visible"
    report["6 -0 into the pooling"] = None      # random data never sums only -0 products: nothing to see
    for k, v in report.items():
        print(f"[lattice] mutant {k}: within SPEC §14 tolerance on random data: "
              + ("not applicable: random data never sums only -0 products" if v is None else "yes (tolerance blind)" if v else "no"))


@pytest.mark.parametrize("kind,i", [("plain", i) for i in range(len(PLAIN))] + [("reg", i) for i in range(len(REG))]
                         + [("tiled", i) for i in range(len(TILED))])
def test_lattice_case_invariants(kind, i):
    """Every case the GPU file builds: within the budget (the generator would raise) and with the statistics it claims."""
    if kind == "plain":
        c = _plain(i)
        keys = _chain_limits(c)
    elif kind == "reg":
        c = _reg(i)
        mode, S = REG[i][8], REG[i][4]
        keys = _chain_limits(c, ["off_first"] + (["straddle_only"] if mode != "full" or S == 64 else []))
    else:
        c = _tiled(i)
        keys = _chain_limits(c, ["off_first"])
    assert bl.check_budget(c.recs) < bl.BUDGET_BITS
    bl.assert_stats(f"{kind} {i}", c.stats, keys)


def test_budget_is_enforced():
    """A chain that cannot stay exact is refused as a fixture."""
    rng = np.random.default_rng(9)
    x = bl.lattice_feat(rng, (64, 256))
    layers, _ = bl.lattice_chain([256, 256], x, rng, nnz=256, kmax=255, f32_ties=False)
    _, recs = bl.forward_exact(x, layers)
    with pytest.raises(ValueError, match="lattice budget"):
        bl.check_budget(recs)
