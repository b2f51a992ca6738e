"""Lattice cases for bit-exact tests of the bf16 MLP path (SPEC.md §14).  Test helper: numpy only, no kernel code.

SPEC §14 leaves one thing free: the ORDER of the binary32 additions of a layer (products of bf16 values are exact).  If every partial
sum of every layer is exactly representable in binary32, every order gives the same bits — and so does the oracle's binary64 sum
(oracle.mlp_rows_bf16).  On such inputs §14 has exactly one correct answer, and a test can demand it bit for bit, ties included.

Quantum.  All inputs of a layer are multiples of a power of two q (their quantum); weights are k·2^-s, so every product is a multiple of
q·2^-s (the product quantum), and so is the bias by construction.  A bf16 rounding of a multiple of q is again a multiple of q: the quantum
carries from layer to layer.

Budget.  For every layer, output channel and row, |b| + Σ|Wb·xb| < 2^22 × the layer's product quantum, checked on the exact intermediates
in binary64 (`check_budget`).  2^24 would already make every partial sum exact in binary32; the 2 spare bits keep it exact on a matrix unit
that aligns a 16-product block to its largest term and truncates inside it.  A case over budget is a wrong fixture, not a wrong kernel:
the generator raises.

Every case carries statistics (`stats`) that show it exercises what it is meant to — hidden activations that bf16 rounding changes,
exact round-to-nearest-even ties, a ReLU that is neither almost always open nor almost always shut, maxima away from a group's first
sample, and for ragged groups, maxima that live only in a later 32-row tile.
"""
import numpy as np

BUDGET_BITS = 22
XYZ_BITS = 10          # coordinates are multiples of 2^-10 in [0, 1): a rel_xyz of up to 10 significant bits (bf16 keeps 8)
FEAT_BITS = 7          # bf16 features k·2^-7, |k| < 256: every feature is a bf16 value, quantum 2^-7


def bf16(x):
    """Round-to-nearest-even binary32 -> bfloat16 (SPEC §14), as binary32 values."""
    u = np.array(x, dtype=np.float32).view(np.uint32)          # (a copy; no finite value overflows 32 bits below)
    lsb = u >> 16
    lsb &= 1
    lsb += 0x7FFF
    u += lsb
    u &= np.uint32(0xFFFF0000)
    return u.view(np.float32).reshape(np.shape(x))


def bf16_trunc(x):
    """Truncation to bfloat16 (a wrong rounding: for the mutants)."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32) & np.uint32(0xFFFF0000)
    return u.view(np.float32).reshape(np.shape(x))


def is_tie(x):
    """binary32 values exactly halfway between two bfloat16 values."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    return (u & 0xFFFF) == 0x8000


def quantum(a):
    """Largest power of two that divides every nonzero element of `a` (binary64-exact values); inf if all are zero."""
    a = np.asarray(a, dtype=np.float64).ravel()
    a = a[a != 0]
    if a.size == 0:
        return np.inf
    m, e = np.frexp(np.abs(a))
    mi = (m * 2.0 ** 53).astype(np.int64)
    low = mi & -mi
    return float(np.min(np.ldexp(low.astype(np.float64), e - 53)))


def _ulp_bf16(v):
    """bf16 ulp of nonzero binary32 values v."""
    _, e = np.frexp(np.abs(v).astype(np.float64))
    return np.ldexp(1.0, e - 8)


def perturb_f32(vals, rng, frac_tie=0.25, frac_noise=0.25):
    """binary32 stand-ins of bf16 values `vals` that round back to them under round-to-nearest-even only:
    exact ties (v + ulp/2 where v's last bf16 bit is even; v - ulp/2 where v is even and not a power of two — truncation then
    drops to the odd neighbour) and off-tie values below half an ulp.  Zeros stay zero."""
    v = np.asarray(vals, dtype=np.float32).copy()
    out = v.astype(np.float64)
    nz = v != 0
    u = np.zeros_like(out)
    u[nz] = _ulp_bf16(v[nz])
    even = nz & (((v.view(np.uint32) >> 16) & 1) == 0)
    pow2 = nz & ((v.view(np.uint32) & 0x007F0000) == 0)
    r = rng.random(v.shape)
    sgn = np.sign(out)
    up = even & (r < frac_tie / 2)
    dn = even & ~pow2 & (r >= frac_tie / 2) & (r < frac_tie)
    noise = nz & (r >= frac_tie) & (r < frac_tie + frac_noise)
    out[up] += sgn[up] * u[up] / 2
    out[dn] -= sgn[dn] * u[dn] / 2
    k = rng.integers(1, 116, size=int(noise.sum())) * rng.choice([-1, 1], size=int(noise.sum()))       # (|k| / 256 < 0.45 ulp)
    out[noise] += u[noise] * k / 256 * np.where(pow2[noise], 0.5, 1.0)
    w = out.astype(np.float32)
    assert np.array_equal(out, w.astype(np.float64)), "perturbed values not binary32"
    assert np.array_equal(bf16(w).view(np.uint32), v.view(np.uint32)), "perturbation does not round back"
    return w


# ---- points, features, groups -------------------------------------------------------------------------------------------------------
def lattice_xyz(rng, shape):
    return (rng.integers(0, 1 << XYZ_BITS, size=shape) * 2.0 ** -XYZ_BITS).astype(np.float32)


def lattice_feat(rng, shape, neg_zero=0.0):
    k = rng.integers(-255, 256, size=shape)
    f = (k * 2.0 ** -FEAT_BITS).astype(np.float32)
    if neg_zero:
        f[rng.random(shape) < neg_zero] = -0.0
    return f


def random_groups(rng, B, N, M, S, mode):
    """idx[B,M,S] with ball-query-style padding (the first index repeated) behind cnt[B,M] live rows.
    mode: 'any' — 1..S rows; 'few' — mostly 1..3 rows and some full groups; 'full' — every group full but every fifth
    (so that full groups start off the 32-row tile grid and straddle tiles)."""
    idx = rng.integers(0, N, size=(B, M, S)).astype(np.int32)
    if mode == "any":
        cnt = rng.integers(1, S + 1, size=(B, M))
    elif mode == "few":
        cnt = rng.choice([1, 1, 2, 3, S // 2, S], size=(B, M))
    else:
        cnt = np.full((B, M), S)
        cnt[:, ::5] = max(1, S - 19)      # (off the tile grid: full groups then straddle tiles)
    cnt = cnt.astype(np.int32)
    for b in range(B):
        for m in range(M):
            idx[b, m, cnt[b, m]:] = idx[b, m, 0]
    return idx, cnt


def layer0_rows(xyz, feat, new_xyz, idx):
    """Exact layer-0 rows [B*M*S, 3 + C] of SPEC §14 in the oracle's column order: bf16([rel_xyz ‖ feat])."""
    B, M, S = idx.shape
    rows = []
    for b in range(B):
        j = idx[b].reshape(-1)
        rel = (xyz[b][j] - np.repeat(new_xyz[b], S, axis=0)).astype(np.float32)
        rows.append(rel if feat is None else np.concatenate([rel, feat[b][j]], axis=1))
    return bf16(np.concatenate(rows, 0))


# ---- weights ------------------------------------------------------------------------------------------------------------------------
def lattice_chain(dims, x0, rng, relu_mask=None, nnz=6, kmax=3, f32_ties=True, neg_zero_bias=0.05, bias_scale=0.6):
    """Weights k·2^-s (|k| <= kmax, about `nnz` nonzero per output, mixed signs) and biases on the product quantum for a chain
    whose layer-0 inputs are the exact bf16 rows x0.  s is chosen per layer (on x0) so that activations stay O(1).  Returns
    (layers, layers_exact): binary32 weights — with exact bf16 ties and off-tie values that only round-to-nearest-even maps back
    when f32_ties — and the bf16 weights they round to; the biases are binary32 and the same in both."""
    L = len(dims) - 1
    if relu_mask is None:
        relu_mask = (1 << L) - 1
    x = np.asarray(x0, dtype=np.float64)
    q = quantum(x)
    layers, exact = [], []
    for l in range(L):
        cin, cout = dims[l], dims[l + 1]
        K = np.zeros((cout, cin))
        for o in range(cout):
            n = min(cin, nnz)
            cols = rng.choice(cin, size=n, replace=False)
            K[o, cols] = rng.integers(1, kmax + 1, size=n) * rng.choice([-1, 1], size=n)
        z = x @ K.T
        rms = float(np.sqrt(np.mean(z * z))) or 1.0
        s = int(np.round(np.log2(rms)))
        W = (K * 2.0 ** -s).astype(np.float32)
        qp = q * 2.0 ** -s
        b = np.round(rng.uniform(-bias_scale, bias_scale, size=cout) / qp) * qp
        b = b.astype(np.float32)
        b[rng.random(cout) < neg_zero_bias] = -0.0
        if (b == 0).sum() == 0 and cout > 1:
            b[rng.integers(cout)] = -0.0
        assert np.array_equal(b.astype(np.float64), np.round(b.astype(np.float64) / qp) * qp)
        Wf = perturb_f32(W, rng) if f32_ties else W
        layers.append((Wf, b))
        exact.append((W, b))
        y = x @ W.astype(np.float64).T + b.astype(np.float64)
        if (relu_mask >> l) & 1:
            y = np.maximum(y, 0.0)
        x = bf16(y.astype(np.float32)).astype(np.float64)
        q = qp
    return layers, exact


# ---- exact forward, budget and statistics -------------------------------------------------------------------------------------------
def forward_exact(x0, layers, relu_mask=None):
    """The chain on exact bf16 rows x0 in binary64, with everything the budget and the statistics need.  Returns
    (y_last binary32 with +0 for every zero of a ReLU layer, per-layer records)."""
    L = len(layers)
    if relu_mask is None:
        relu_mask = (1 << L) - 1
    x = np.asarray(x0, dtype=np.float64)
    q = quantum(x)
    recs = []
    for l, (W, b) in enumerate(layers):
        Wb = bf16(np.asarray(W, dtype=np.float32)).astype(np.float64)
        bd = np.asarray(b, dtype=np.float64)
        qw = quantum(Wb)
        qp = q * qw
        if np.isfinite(qp):
            assert np.array_equal(bd, np.round(bd / qp) * qp), f"layer {l}: a bias is not a multiple of the product quantum"
        mag = np.abs(x) @ np.abs(Wb).T + np.abs(bd)
        y = x @ Wb.T + bd
        y32 = y.astype(np.float32)
        assert np.array_equal(y32.astype(np.float64), y) or not np.isfinite(qp), f"layer {l}: a sum is not binary32"
        relu = bool((relu_mask >> l) & 1)
        if relu:
            y32 = np.where(y32 > 0, y32, np.float32(0))
        recs.append(dict(q=q, qp=qp, mag=mag, y=y32, relu=relu))
        x = bf16(y32).astype(np.float64)
        q = qp if np.isfinite(qp) else q
    return recs[-1]["y"], recs


def check_budget(recs, bits=BUDGET_BITS):
    """Raises if any layer's |b| + Σ|Wb·xb| reaches 2^bits product quanta: the case would not pin a single answer."""
    worst = 0.0
    for l, r in enumerate(recs):
        if not np.isfinite(r["qp"]):
            continue
        ratio = float(r["mag"].max()) / r["qp"]
        if ratio >= 2.0 ** bits:
            raise ValueError(f"lattice budget: layer {l} reaches 2^{np.log2(ratio):.2f} product quanta (limit 2^{bits})")
        worst = max(worst, ratio)
    return float(np.log2(worst)) if worst else 0.0


def chain_stats(recs):
    """Rounded fraction / ties over the hidden activations (inputs of the next layer), ReLU-open fraction over ReLU layers."""
    hid = [r["y"].ravel() for r in recs[:-1]]
    h = np.concatenate(hid) if hid else np.zeros(0, np.float32)
    relu = [r["y"].ravel() for r in recs if r["relu"]]
    rl = np.concatenate(relu) if relu else np.zeros(0, np.float32)
    return dict(rounded=float((bf16(h) != h).mean()) if h.size else 0.0, ties=int(is_tie(h).sum()),
                positive=float((rl > 0).mean()) if rl.size else 0.5, budget_bits=check_budget(recs))


def group_stats(y_last, cnt, S, dense=True):
    """(group, channel) statistics of the pooled rows y_last[G*S, C] (dense: S rows per group; only the first cnt[g] are live
    when cnt is given).  off_first: share of (group, channel) with a positive max not at sample 0; straddle_only: groups whose max
    on some channel lies only in a later 32-row tile of the packed order (group g's live rows at gstart[g] ..)."""
    G = y_last.shape[0] // S
    C = y_last.shape[1]
    y = y_last.reshape(G, S, C)
    c = np.full(G, S) if cnt is None else np.maximum(np.asarray(cnt).reshape(-1), 1)
    live = np.arange(S)[None, :] < c[:, None]
    yl = np.where(live[:, :, None], y, -np.inf)
    mx = yl.max(axis=1)
    off_first = float(((mx > y[:, 0, :]) & (mx > 0)).mean())
    gs = np.concatenate([[0], np.cumsum(c)])
    first_tile_rows = np.minimum(c, ((gs[:-1] >> 5) + 1) * 32 - gs[:-1])
    in_first = np.arange(S)[None, :] < first_tile_rows[:, None]
    m0 = np.where(in_first[:, :, None], yl, -np.inf).max(axis=1)
    straddle_only = int((mx > m0).any(axis=1).sum())
    n_cont = ((gs[1:] - 1) >> 5) - (gs[:-1] >> 5)
    return dict(off_first=off_first, straddle_only=straddle_only, two_cont=int((n_cont >= 2).sum()))


def print_stats(what, st, limits):
    print(f"[lattice] {what}: " + ", ".join(f"{k}={v:.3f}" if isinstance(v, float) else f"{k}={v}" for k, v in st.items())
          + "  (limits: " + ", ".join(f"{k} {v}" for k, v in limits.items()) + ")")


# Limits every case is held to (assert_stats); a case that only fills part of them names the ones that apply.
LIMITS = dict(rounded=("> 0.2", lambda v: v > 0.2), ties=("> 0", lambda v: v > 0), positive=("in [0.15, 0.85]", lambda v: 0.15 <= v <= 0.85),
              off_first=("> 0.2", lambda v: v > 0.2), straddle_only=("> 0", lambda v: v > 0))


def assert_stats(what, st, keys):
    print_stats(what, st, {k: LIMITS[k][0] for k in keys})
    for k in keys:
        assert LIMITS[k][1](st[k]), f"{what}: statistic {k} = {st[k]} outside {LIMITS[k][0]} (the case tests too little)"


# ---- whole cases --------------------------------------------------------------------------------------------------------------------
class Case:
    pass


def plain_case(seed, rows, dims, relu_mask=None, nnz=6, **kw):
    """Plain rows: x[rows, dims[0]] bf16 lattice values (x32: binary32 stand-ins with ties) and a lattice chain."""
    rng = np.random.default_rng(seed)
    c = Case()
    c.x = lattice_feat(rng, (rows, dims[0]))
    c.x32 = perturb_f32(c.x, rng)
    c.relu_mask = (1 << (len(dims) - 1)) - 1 if relu_mask is None else relu_mask
    c.layers, c.exact = lattice_chain(dims, c.x, rng, c.relu_mask, nnz=nnz, **kw)
    c.want, c.recs = forward_exact(c.x, c.layers, c.relu_mask)
    c.stats = chain_stats(c.recs)
    return c


def grouped_case(seed, B, N, M, S, C, mlp, mode="any", nnz=6, feat_neg_zero=0.0, **kw):
    """Grouped chain [C + 3] + mlp on lattice points: xyz, new_xyz (other lattice points), idx / cnt from `random_groups`,
    bf16 features (feat) and binary32 stand-ins (feat32).  want: the pooled oracle [B, M, C_out]."""
    rng = np.random.default_rng(seed)
    c = Case()
    c.xyz = lattice_xyz(rng, (B, N, 3))
    c.new_xyz = lattice_xyz(rng, (B, M, 3))
    c.feat = lattice_feat(rng, (B, N, C), feat_neg_zero) if C else None
    c.feat32 = perturb_f32(c.feat, rng) if C else None
    c.idx, c.cnt = random_groups(rng, B, N, M, S, mode)
    c.S = S
    x0 = layer0_rows(c.xyz, c.feat, c.new_xyz, c.idx)
    c.x0 = x0
    c.layers, c.exact = lattice_chain([C + 3] + list(mlp), x0, rng, nnz=nnz, **kw)
    y, c.recs = forward_exact(x0, c.layers)
    c.rows_out = y
    c.want = y.reshape(B * M, S, -1).max(axis=1).reshape(B, M, -1) + np.float32(0)
    st = chain_stats(c.recs)
    rel = np.concatenate([(c.xyz[b][c.idx[b].reshape(-1)] - np.repeat(c.new_xyz[b], S, 0)) for b in range(B)], 0).astype(np.float32)
    st["rel_rounded"] = float((bf16(rel) != rel).mean())
    st["rel_ties"] = int(is_tie(rel).sum())
    st.update(group_stats(y, c.cnt, S))
    c.stats = st
    return c


# ---- a whole detector backbone on the lattice -------------------------------------------------------------------------------------------
def snap_points(pts, xyz_bits, rng):
    """Raw points [B, N, 3 + F] on the lattice: xyz multiples of 2^-xyz_bits, extra channels bf16 lattice values as binary32
    stand-ins with ties (the first stage rounds them on load)."""
    p = np.array(pts, dtype=np.float32)
    p[:, :, :3] = (np.round(p[:, :, :3].astype(np.float64) * 2.0 ** xyz_bits) * 2.0 ** -xyz_bits).astype(np.float32)
    if p.shape[2] > 3:
        p[:, :, 3:] = perturb_f32(lattice_feat(rng, p[:, :, 3:].shape), rng)
    return p


def backbone_lattice(orc, cfg, pts, rng, weights, nnz=3, kmax=1):
    """Lattice weights for every sa* chain of `cfg` (written into `weights`), chosen stage by stage on the oracle's own inputs, and
    the SPEC §14 stage outputs chained from the raw points: fps -> ball query -> branches -> concat -> aggregation, no GPU tensor
    anywhere.  Returns ({name: out [B, M, C] as stored (bf16 values)}, {name: statistics}).  Raises if any layer leaves the budget."""
    xyz = np.ascontiguousarray(pts[:, :, :3])
    feat = bf16(np.ascontiguousarray(pts[:, :, 3:])) if pts.shape[2] > 3 else None
    B = pts.shape[0]
    outs, stats = {}, {}
    for si, st in enumerate(cfg.stages):
        name = f"sa{si + 1}"
        M = st.npoint
        new_xyz = orc.gather_xyz(xyz, orc.fps(xyz, M))
        C = 0 if feat is None else feat.shape[2]
        pooled, recs_all, st_all = [], [], []
        for bi, (r, s, mlp) in enumerate(zip(st.radii, st.nsamples, st.mlps)):
            idx = orc.ball_query(r, s, xyz, new_xyz)
            x0 = layer0_rows(xyz, feat, new_xyz, idx)
            layers, _ = lattice_chain([C + 3] + list(mlp), x0, rng, nnz=nnz, kmax=kmax)
            y, recs = forward_exact(x0, layers)
            check_budget(recs)
            weights[f"{name}.b{bi}"] = layers
            pooled.append(y.reshape(B * M, s, -1).max(axis=1))
            recs_all += recs
            st_all.append(group_stats(y, None, s))
        cat = bf16(np.concatenate(pooled, axis=1))
        agg, _ = lattice_chain([cat.shape[1], st.agg], cat, rng, nnz=nnz, kmax=kmax)
        y, recs = forward_exact(cat, agg)
        weights[f"{name}.agg"] = agg
        s_ = chain_stats(recs_all + recs)
        s_["off_first"] = float(np.mean([g["off_first"] for g in st_all]))
        stats[name] = s_
        outs[name] = bf16(y).reshape(B, M, -1)
        xyz, feat = new_xyz, outs[name]
    return outs, stats
