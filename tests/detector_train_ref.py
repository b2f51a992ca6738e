"""numpy reference of the candidate layer's backward (SPEC.md §33) and of the cluster section composed from it and the chain
references of tests/mlp_grad_ref.py, with the inputs their tests share.

``candidates_grad_ref`` / ``prefix_rows_grad_ref`` are the formulas of §33.1 / §33.2 as written: selections and copies, no
arithmetic, so the kernels are compared with ``==``.  ``cluster_ref`` is the float64 composition of §8-§9's backward on given
indices: head rows, cluster.agg rows, one ``grouped_ref`` per branch, the summed grad_new_xyz, ``candidates_grad``, the candidate
MLP's rows, the padded prefix plus the branches' grad_feat.  Beside every value runs its absolute companion ``A`` and the number
of roundings ``n`` on the longest path (mlp_grad_ref's bound): a stage that takes a computed gradient adds that gradient's n to
its own, a sum of k computed terms has the terms' n added up plus k - 1.  ``stack_ref`` carries the gradient at SA3's output on
through the SA stages (§7) the same way; both walk a multi-radius layer with ``_cat_backward``."""
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


def _put(grads, name, r, layers, extra_n=0):
    """The parameter gradients of a chain result ``r`` (``rows_chain`` / ``grouped_ref``) as (val, A, n) entries of ``grads``."""
    for l in range(len(layers)):
        grads[f"{name}.W{l}"] = (r["val"]["grad_W"][l], r["A"]["grad_W"][l], r["depth"]["grad_W"][l] + extra_n)
        grads[f"{name}.b{l}"] = (r["val"]["grad_b"][l], r["A"]["grad_b"][l], r["depth"]["grad_b"][l] + extra_n)


def _cat_forward(orc, branch, blayers, agg_layers):
    """The forward of a multi-radius layer: the branches' pooled rows side by side -> (cat [B*M, sum C_b], the aggregation
    layer's output [B*M, C'])."""
    B, M = branch[0]["idx"].shape[:2]
    cat = np.concatenate([_pooled(orc, inp, layers) for inp, layers in zip(branch, blayers)], 2).reshape(B * M, -1)
    return cat, rows_chain(orc, cat, agg_layers, 1, np.zeros((B * M, agg_layers[-1][0].shape[0])))["out"]


def _cat_backward(orc, grads, name, branch, blayers, cat, agg_layers, g, gA, n_in):
    """The backward of a multi-radius layer (branches -> cat -> aggregation layer with ReLU) from the gradient (g, gA, n_in) at
    the aggregation layer's output: ``rows_chain`` on the aggregation layer, one ``grouped_ref`` per branch with its column
    slice of grad_x as grad_out, the branches' input gradients summed.  Writes "<name>.agg.*" and "<name>.b<k>.*" into ``grads``
    -> {"grad_feat" (where the branches have input features), "grad_new_xyz": (val, A, n)}; n: every branch's depth plus the
    aggregation's grad_x depth, plus nb - 1 for the sum."""
    B, M = branch[0]["idx"].shape[:2]
    agg = rows_chain(orc, cat, agg_layers, 1, g, gA, n_in)
    _put(grads, f"{name}.agg", agg, agg_layers)
    n_a = agg["depth"]["grad_x"]
    keys = ("grad_feat", "grad_new_xyz") if branch[0]["feat"] is not None else ("grad_new_xyz",)
    tot = {k: [0.0, 0.0, len(branch) - 1] for k in keys}
    off = 0
    for k, (inp, layers) in enumerate(zip(branch, blayers)):
        co = layers[-1][0].shape[0]
        go = agg["val"]["grad_x"][:, off:off + co].reshape(B, M, co)
        goA = agg["A"]["grad_x"][:, off:off + co].reshape(B, M, co)
        r = ref.grouped_ref(orc, layers=layers, grad_out=go, grad_out_A=goA, **inp)
        _put(grads, f"{name}.b{k}", r, layers, n_a)
        for key, t in tot.items():
            t[0], t[1], t[2] = t[0] + r["val"][key], t[1] + r["A"][key], t[2] + r["depth"][key] + n_a
        off += co
    return {k: tuple(t) for k, t in tot.items()}


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
    blayers = [weights[f"cluster.b{k}"] for k in range(nb)]
    cat, agg_out = _cat_forward(orc, branch, blayers, weights["cluster.agg"])
    # ---- backward
    grads = {}
    Co = weights["head"][-1][0].shape[0]
    head = rows_chain(orc, agg_out, weights["head"], mask(weights["head"]), np.asarray(w_o).reshape(B * K, Co))
    _put(grads, "head", head, weights["head"])
    tot = _cat_backward(orc, grads, "cluster", branch, blayers, cat, weights["cluster.agg"], head["val"]["grad_x"], head["A"]["grad_x"],
                        head["depth"]["grad_x"])
    gf, gfA, gf_n = tot["grad_feat"]
    gn, gnA, gn_n = tot["grad_new_xyz"]
    grads["cand_xyz"] = (gn, gnA, gn_n)
    # candidates_grad (a selection on c) plus the direct gradient of (c * w_c).sum()
    wc = np.asarray(w_c, np.float64).reshape(B, K, 6)
    gc = candidates_grad_ref(c_use, gn, shift_max) + wc
    gcA = candidates_grad_ref(c_use, gnA, shift_max) + np.abs(wc)
    gc_n = gn_n + 1
    grads["c"] = (gc, gcA, gc_n)
    cm = rows_chain(orc, xk, weights["cand"], mask(weights["cand"]), gc.reshape(B * K, 6), gcA.reshape(B * K, 6), gc_n)
    _put(grads, "cand", cm, weights["cand"])
    pad = prefix_rows_grad_ref(cm["val"]["grad_x"].reshape(B, K, C3), M3)
    padA = prefix_rows_grad_ref(cm["A"]["grad_x"].reshape(B, K, C3), M3)
    grads["feat3"] = (gf + pad, gfA + padA, gf_n + cm["depth"]["grad_x"] + 1)
    o = head["out"].reshape(B, K, Co)
    return {"c": c_own, "cand": cand, "o": o, "grads": grads}


def _stage_branches(st):
    return [dict(xyz=st["xyz"], feat=st["feat"], new_xyz=st["new_xyz"], idx=i, cnt=n, skip_empty=False) for i, n in zip(st["idxs"], st["cnts"])]


def stage_forward(orc, st, weights, s):
    """The forward of SA stage ``s`` (1-based; SPEC.md §7) on a stage dict (see ``stack_ref``) -> (cat [B*M, sum C_b], out
    [B,M,C']): the oracle's §6 bits, or float64 activations with ``orc`` None."""
    nb = len(st["idxs"])
    cat, out = _cat_forward(orc, _stage_branches(st), [weights[f"sa{s}.b{k}"] for k in range(nb)], weights[f"sa{s}.agg"])
    return cat, out.reshape(st["new_xyz"].shape[:2] + (-1,))


def stack_ref(orc, stages, weights, grad_feat_last):
    """The SA stages' backward (§7 composed with §32) below a given gradient at the last stage's output.  ``stages``: first stage
    first, dicts of float32 arrays xyz [B,N,3], feat [B,N,C] | None, new_xyz [B,M,3] and one idx [B,M,S] / cnt [B,M] per branch
    in idxs / cnts: the bits and indices the module used (a stage's feat is the stage below's output).  ``weights``: the
    ``export()`` dict.  ``grad_feat_last``: (val, A, n) as ``cluster_ref`` returns for "feat3".  Walks from the last stage to the
    first: the aggregation layer's rows on the incoming gradient, each branch on its column slice of grad_x, the branches'
    grad_feat summed (a stage output's gradient is the sum over its consumers) and handed to the stage below.
    -> {"grads": {"sa<s>.b<k>.W<l>" / ".b<l>", "sa<s>.agg.W0" / ".b0", "feat<s>" (the gradient at stage s's INPUT features,
    where it has any): (val, A, n)}, "out<s>": the reference's own forward of stage s's output}."""
    res = {"grads": {}}
    cats = []
    for s, st in enumerate(stages, 1):
        cat, res[f"out{s}"] = stage_forward(orc, st, weights, s)
        cats.append(cat)
    g, gA, n = grad_feat_last
    for s in range(len(stages), 0, -1):
        st = stages[s - 1]
        B, M = st["new_xyz"].shape[:2]
        nb = len(st["idxs"])
        tot = _cat_backward(orc, res["grads"], f"sa{s}", _stage_branches(st), [weights[f"sa{s}.b{k}"] for k in range(nb)], cats[s - 1],
                            weights[f"sa{s}.agg"], np.asarray(g).reshape(B * M, -1), np.asarray(gA).reshape(B * M, -1), n)
        if st["feat"] is None:
            assert s == 1, "only the first stage can be without input features"
            break
        res["grads"][f"feat{s}"] = g, gA, n = tot["grad_feat"]
    return res


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


def small_points(cfg, B=2, seed=0):
    """points [B, n_points, 3 + in_feat] of the small detector: coordinates drawn as ``small_inputs`` draws xyz3 (a slab of
    4 x 4 x 1), the feature columns standard normal."""
    rng = np.random.default_rng([seed, 34])
    xyz = rng.uniform(-1.0, 1.0, (B, cfg.n_points, 3)) * np.array([2.0, 2.0, 0.5])
    return np.concatenate([xyz, rng.standard_normal((B, cfg.n_points, cfg.in_feat))], 2).astype(np.float32)


def stack_chains(cfg):
    """The names of the SA stages' chains, as ``param_names`` takes them."""
    return [f"sa{s}.{ch}" for s, st in enumerate(cfg.stages, 1) for ch in [f"b{k}" for k in range(len(st.mlps))] + ["agg"]]


def stack_populations(orc, stages, weights, cfg):
    """What a test of the SA stack must hold, asserted: in every stage no empty group (a centroid is one of the points) and, in
    at least one branch, both a partly filled group (0 < cnt < S) and a full one (cnt == S); in every layer of every chain at
    least one ReLU off and one on.  -> a line that says how many of each."""
    said = []
    for s, (st, cs) in enumerate(zip(stages, cfg.stages), 1):
        assert all((n >= 1).all() for n in st["cnts"]), f"sa{s}: an empty group"
        part = [int(((n > 0) & (n < S)).sum()) for n, S in zip(st["cnts"], cs.nsamples)]
        full = [int((n == S).sum()) for n, S in zip(st["cnts"], cs.nsamples)]
        assert any(p and f for p, f in zip(part, full)), f"sa{s}: no branch holds a partly filled and a full group ({part}, {full})"
        relu = []
        for k, inp in enumerate(_stage_branches(st)):
            layers = weights[f"sa{s}.b{k}"]
            z = np.zeros(inp["idx"].shape[:2] + (layers[-1][0].shape[0],), np.float32)
            relu += ref.grouped_ref(orc, layers=layers, grad_out=z, **inp)["relu_on"]
        out = stage_forward(orc, st, weights, s)[1]
        relu.append((int((out > 0).sum()), out.size))
        assert all(0 < on < size for on, size in relu), f"sa{s}: a layer whose ReLUs are all on or all off ({relu})"
        said.append(f"sa{s}: partly filled {part}, full {full}, ReLU on {[f'{on}/{size}' for on, size in relu]}")
    return "; ".join(said)


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
