"""numpy reference of the candidate layer's backward (SPEC.md §33) and of the cluster section composed from it and the chain
references of tests/mlp_grad_ref.py, with the inputs their tests share.

``candidates_grad_ref`` / ``prefix_rows_grad_ref`` are the formulas of §33.1 / §33.2 as written: selections and copies, no
arithmetic, so the kernels are compared with ``==``.  ``cluster_ref`` is the float64 composition of §8-§9's backward on given
indices: head rows, cluster.agg rows, one ``grouped_ref`` per branch, the summed grad_new_xyz, ``candidates_grad``, the candidate
MLP's rows, the padded prefix plus the branches' grad_feat.  Beside every value runs its absolute companion ``A`` and the number
of roundings ``n`` on the longest path (mlp_grad_ref's bound): a stage that takes a computed gradient adds that gradient's n to
its own, a sum of k computed terms has the terms' n added up plus k - 1."""
import numpy as np

import mlp_grad_ref as ref


def step2(xyz_k, c, shift_max, dtype=np.float64):
    """§8 step 2 in ``dtype``: cand = xyz3[:, :K] + clamp(c[..., 0:3], -shift_max, shift_max)."""
    sh = np.asarray(c, dtype)[..., :3]
    return np.asarray(xyz_k, dtype) + np.minimum(np.maximum(sh, -dtype(shift_max)), dtype(shift_max))


def shift_passes(c, shift_max):
    """Where the clamp of §8 step 2 passes the gradient: -shift_max <= c_d <= shift_max, bounds included, NaN fails."""
    sh = np.asarray(c)[..., :3]
    sm = np.float32(shift_max)
    with np.errstate(invalid="ignore"):
        return (sh >= -sm) & (sh <= sm)


def candidates_grad_ref(c, grad_cand, shift_max):
    """c [B,K,6] f32, grad_cand [B,K,3] -> grad_c [B,K,6] of grad_cand's dtype: a selection in columns 0..2, +0 in 3..5."""
    g = np.asarray(grad_cand)
    out = np.zeros(g.shape[:-1] + (6,), g.dtype)
    out[..., :3] = np.where(shift_passes(c, shift_max), g, g.dtype.type(0))
    return out


def prefix_rows_grad_ref(g, M):
    """g [B,K,C] -> [B,M,C]: rows < K are g's, the rest +0."""
    g = np.asarray(g)
    B, K, C = g.shape
    assert 1 <= K <= M
    out = np.zeros((B, M, C), g.dtype)
    out[:, :K] = g
    return out


def edge_values(shift_max):
    """The values of c at which §33.1's selection can go wrong: both bounds (pass), the next float beyond each (blocked), both
    zeros, NaN, infinities."""
    sm = np.float32(shift_max)
    return np.array([-sm, sm, np.nextafter(sm, np.float32(np.inf)), np.nextafter(-sm, np.float32(-np.inf)), 0.0, -0.0, np.nan,
                     np.inf, -np.inf, np.nextafter(sm, np.float32(0)), np.nextafter(-sm, np.float32(0))], np.float32)


def edge_case(B, K, shift_max, seed=0):
    """(c [B,K,6], grad_cand [B,K,3]): edge values mixed with normals in c; normals and both zeros in grad_cand."""
    rng = np.random.default_rng([seed, B, K])
    c = (rng.standard_normal((B, K, 6)) * max(float(shift_max), 0.5)).astype(np.float32)
    ev = edge_values(shift_max)
    pick = rng.random((B, K, 6)) < 0.5
    c = np.where(pick, ev[rng.integers(0, len(ev), (B, K, 6))], c).astype(np.float32)
    flat = c.reshape(-1)
    flat[:min(len(ev), flat.size)] = ev[:min(len(ev), flat.size)]          # every edge value at least once where there is room
    g = rng.standard_normal((B, K, 3)).astype(np.float32)
    gz = rng.random((B, K, 3))
    g = np.where(gz < 0.1, np.float32(0.0), np.where(gz < 0.2, np.float32(-0.0), g)).astype(np.float32)
    return c, g


def rows_chain(orc, x, layers, relu_mask, g, gA=None, n_in=0, dtype=np.float64):
    """``mlp_grad_ref.rows_ref`` for a grad_out that is itself a computed gradient: ``gA`` its absolute companion (else |g|),
    ``n_in`` its depth, added to every depth of the result."""
    L = len(layers)
    xs = ref._activations(orc, np.ascontiguousarray(x, np.float32), layers, relu_mask)
    g = np.asarray(g, dtype)
    (gW, gb, g0), (gWA, gbA, g0A) = ref._chain_back(xs, layers, relu_mask, g, np.abs(g) if gA is None else np.asarray(gA, dtype), dtype)
    R = x.shape[0]
    widths = [w.shape[0] for w, _ in layers]
    dW = [R + sum(widths[l + 1:]) + L + n_in for l in range(L)]
    return {"out": xs[L], "val": {"grad_x": g0, "grad_W": gW, "grad_b": gb}, "A": {"grad_x": g0A, "grad_W": gWA, "grad_b": gbA},
            "depth": {"grad_x": sum(widths) + L + n_in, "grad_W": dW, "grad_b": dW}}


def _pooled(orc, inp, layers):
    z = np.zeros(inp["idx"].shape[:2] + (layers[-1][0].shape[0],), np.float32)
    return ref.grouped_ref(orc, layers=layers, grad_out=z, **inp)["pooled"]


def cluster_ref(orc, xyz3, feat3, weights, K, shift_max, idxs, cnts, w_o, w_c, c=None):
    """The cluster section (§8 + §9) forward and backward of ``(o * w_o).sum() + (c * w_c).sum()`` on the indices ``idxs`` /
    ``cnts`` (one [B,K,S] / [B,K] pair per branch).  ``orc``: the oracle (its §6 bits decide every ReLU, arg-max and clamp) or
    ``None`` (float64 activations).  ``c``: the candidate layer's rows to decide the clamp on and to place the candidates with,
    instead of the reference's own.  -> dict: c, cand, o (the reference's forward) and grads = {name: (val, A, n)} for
    "head.W<l>" / "head.b<l>", "cluster.agg.*", "cluster.b<k>.*", "cand.*", "feat3", "c" and "cand_xyz" (the gradient at cand)."""
    B, M3, C3 = feat3.shape
    nb = len(idxs)
    mask = lambda layers: (1 << (len(layers) - 1)) - 1
    # ---- forward
    xk = np.ascontiguousarray(feat3[:, :K]).reshape(B * K, C3)
    zero6 = np.zeros((B * K, 6))
    c_own = rows_chain(orc, xk, weights["cand"], mask(weights["cand"]), zero6)["out"].reshape(B, K, 6)
    c_use = c_own if c is None else c
    cand = step2(xyz3[:, :K], c_use, shift_max, np.float32 if c_use.dtype == np.float32 else np.float64).astype(np.float32)
    branch = [dict(xyz=xyz3, feat=feat3, new_xyz=cand, idx=i, cnt=n, skip_empty=False) for i, n in zip(idxs, cnts)]
    cat = np.concatenate([_pooled(orc, inp, weights[f"cluster.b{k}"]) for k, inp in enumerate(branch)], 2).reshape(B * K, -1)
    agg_out = rows_chain(orc, cat, weights["cluster.agg"], 1, np.zeros((B * K, weights["cluster.agg"][-1][0].shape[0])))["out"]
    # ---- backward
    grads = {}

    def put(name, r, layers):
        for l in range(len(layers)):
            grads[f"{name}.W{l}"] = (r["val"]["grad_W"][l], r["A"]["grad_W"][l], r["depth"]["grad_W"][l])
            grads[f"{name}.b{l}"] = (r["val"]["grad_b"][l], r["A"]["grad_b"][l], r["depth"]["grad_b"][l])

    Co = weights["head"][-1][0].shape[0]
    head = rows_chain(orc, agg_out, weights["head"], mask(weights["head"]), np.asarray(w_o).reshape(B * K, Co))
    put("head", head, weights["head"])
    agg = rows_chain(orc, cat, weights["cluster.agg"], 1, head["val"]["grad_x"], head["A"]["grad_x"], head["depth"]["grad_x"])
    put("cluster.agg", agg, weights["cluster.agg"])
    n_a = agg["depth"]["grad_x"]
    gf, gfA, gf_n = 0.0, 0.0, 0
    gn, gnA, gn_n = 0.0, 0.0, 0
    off = 0
    for k, inp in enumerate(branch):
        layers = weights[f"cluster.b{k}"]
        co = layers[-1][0].shape[0]
        go = agg["val"]["grad_x"][:, off:off + co].reshape(B, K, co)
        goA = agg["A"]["grad_x"][:, off:off + co].reshape(B, K, co)
        r = ref.grouped_ref(orc, layers=layers, grad_out=go, grad_out_A=goA, **inp)
        for l in range(len(layers)):
            grads[f"cluster.b{k}.W{l}"] = (r["val"]["grad_W"][l], r["A"]["grad_W"][l], r["depth"]["grad_W"][l] + n_a)
            grads[f"cluster.b{k}.b{l}"] = (r["val"]["grad_b"][l], r["A"]["grad_b"][l], r["depth"]["grad_b"][l] + n_a)
        gf, gfA, gf_n = gf + r["val"]["grad_feat"], gfA + r["A"]["grad_feat"], gf_n + r["depth"]["grad_feat"] + n_a
        gn, gnA, gn_n = gn + r["val"]["grad_new_xyz"], gnA + r["A"]["grad_new_xyz"], gn_n + r["depth"]["grad_new_xyz"] + n_a
        off += co
    gn_n += nb - 1
    grads["cand_xyz"] = (gn, gnA, gn_n)
    # candidates_grad (a selection on c) plus the direct gradient of (c * w_c).sum()
    wc = np.asarray(w_c, np.float64).reshape(B, K, 6)
    gc = candidates_grad_ref(c_use, gn, shift_max) + wc
    gcA = candidates_grad_ref(c_use, gnA, shift_max) + np.abs(wc)
    gc_n = gn_n + 1
    grads["c"] = (gc, gcA, gc_n)
    cm = rows_chain(orc, xk, weights["cand"], mask(weights["cand"]), gc.reshape(B * K, 6), gcA.reshape(B * K, 6), gc_n)
    put("cand", cm, weights["cand"])
    pad = prefix_rows_grad_ref(cm["val"]["grad_x"].reshape(B, K, C3), M3)
    padA = prefix_rows_grad_ref(cm["A"]["grad_x"].reshape(B, K, C3), M3)
    grads["feat3"] = (gf + pad, gfA + padA, gf_n + cm["depth"]["grad_x"] + nb)
    o = head["out"].reshape(B, K, Co)
    return {"c": c_own, "cand": cand, "o": o, "grads": grads}


def check(name, got, entry, extra_n=0):
    """``mlp_grad_ref.check_close`` on a (val, A, n) entry of ``cluster_ref``."""
    val, A, n = entry
    ref.check_close(name, got, np.asarray(val, np.float64), np.asarray(A, np.float64), n + extra_n)


def param_names(weights, chains=("head", "cluster.agg", "cluster.b0", "cluster.b1", "cand")):
    return [f"{ch}.{kind}{l}" for ch in chains for l in range(len(weights[ch])) for kind in ("W", "b")]


# ---- the small cluster section the CPU and GPU tests share -----------------------------------------------------------
# K < M3, a ragged 32-channel tile (33) in the cluster widths, S = 8 / 16; points in a slab of 4 x 4 x 1 with candidates
# shifted by up to shift_max = 1 out of it, radii within 0.3 .. 0.9 (a small size anchor): some candidates end up with no neighbour, many with a few.
def small_config():
    from sad_amd.config import DetectorConfig, SAStage
    return DetectorConfig(
        n_points=192, in_feat=1,
        stages=(SAStage(96, (0.5, 1.0), (8, 16), ((8, 16), (8, 16)), 16),
                SAStage(64, (1.0, 2.0), (8, 16), ((16, 16), (16, 33)), 24),
                SAStage(40, (1.5, 3.0), (8, 16), ((16, 32), (16, 33)), 20)),
        n_cand=24, cand_mlp=(16, 6), cluster_scales=(1.0, 2.0), cluster_nsamples=(8, 16),
        cluster_mlps=((16, 33), (10, 33, 40)), cluster_agg=33, head_mlp=(16, 10),
        anchor_car=(0.8, 0.6, 0.5), shift_max=1.0, r_min=0.3, r_max=0.9)


def small_weights(cfg, seed=0, shift_scale=30.0, size_scale=4.0):
    """``synth.make_weights`` with the shift rows of the candidate layer's last layer scaled up so that shift components fall on
    both sides of the clamp (make_weights scales that layer down by 0.05 to keep them inside), the size rows by less so that the
    radii spread between r_min and r_max."""
    from sad_amd import synth
    w = synth.make_weights(cfg, seed)
    W, b = w["cand"][-1]
    W = W.copy()
    W[:3] *= np.float32(shift_scale)
    W[3:] *= np.float32(size_scale)
    w["cand"][-1] = (np.ascontiguousarray(W), b)
    return w


def small_inputs(cfg, B=2, seed=0):
    """(xyz3 [B,M3,3], feat3 [B,M3,C3]) of the small section: what SA3 would hand over."""
    rng = np.random.default_rng([seed, 33])
    M3, C3 = cfg.stages[-1].npoint, cfg.stages[-1].agg
    xyz3 = (rng.uniform(-1.0, 1.0, (B, M3, 3)) * np.array([2.0, 2.0, 0.5])).astype(np.float32)
    feat3 = np.abs(rng.standard_normal((B, M3, C3))).astype(np.float32)          # (a stage output: behind a ReLU)
    return xyz3, feat3


def ball_counts(xyz3, cand, radius, scale, S):
    """Brute-force §3 on float32 values: (idx [B,K,S] int32, cnt [B,K] int32) — the first S points with d2 < r^2 in index order,
    slots beyond cnt repeat slot 0, an empty group holds point 0.  For the CPU test of the composition only (the GPU test takes
    the indices the module used)."""
    B, K, _ = cand.shape
    idx = np.zeros((B, K, S), np.int32)
    cnt = np.zeros((B, K), np.int32)
    r = (np.float32(scale) * radius).astype(np.float32)
    for b in range(B):
        for k in range(K):
            d = (xyz3[b] - cand[b, k]).astype(np.float32)
            d2 = (d * d).sum(1, dtype=np.float32)
            hit = np.nonzero(d2 < r[b, k] * r[b, k])[0][:S]
            cnt[b, k] = len(hit)
            if len(hit):
                idx[b, k, :len(hit)] = hit
                idx[b, k, len(hit):] = hit[0]
    return idx, cnt
