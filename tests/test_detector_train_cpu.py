"""The candidate layer's backward without a GPU (SPEC.md §33): the numpy reference of tests/detector_train_ref.py against a float64
central difference of §8 step 2 and by enumeration at the clamp's edges; the refusals of ``ops.candidates`` /
``ops.candidates_grad`` / ``ops.prefix_rows_grad`` and of their C entry points that are decided before any device; the composed
float64 reference of the cluster section exercised against itself, and the whole composition (``stack_ref`` below ``cluster_ref``)
against torch autograd in float64."""
import numpy as np
import pytest

import detector_train_ref as dref


def test_reference_against_central_difference():
    """d/dc of sum(w * step2(xyz, c)) by central differences in float64, at c at least 0.1 away from +-shift_max: step 2 is
    linear on either side of a bound, so the quotient is the derivative up to float64 rounding (|w| * 2^-52 * |cand| / h)."""
    rng = np.random.default_rng(0)
    B, K, sm, h = 2, 40, 2.0, 1e-3
    c = rng.uniform(-4.0, 4.0, (B, K, 6))
    near = np.abs(np.abs(c[..., :3]) - sm) < 0.1
    c[..., :3] = np.where(near, c[..., :3] + np.sign(c[..., :3]) * 0.25, c[..., :3])
    assert (np.abs(np.abs(c[..., :3]) - sm) >= 0.1).all()
    assert (np.abs(c[..., :3]) > sm).any() and (np.abs(c[..., :3]) < sm).any()
    xyz = rng.standard_normal((B, K, 3))
    w = rng.standard_normal((B, K, 3))
    want = dref.candidates_grad_ref(c.astype(np.float32), w, sm)
    assert want.dtype == np.float64
    num = np.zeros((B, K, 6))
    for d in range(6):
        e = np.zeros(6)
        e[d] = h
        num[..., d] = ((dref.step2(xyz, c + e, sm) - dref.step2(xyz, c - e, sm)) * w).sum(-1) / (2 * h)
    assert np.abs(num - want).max() <= 1e-9
    assert (want[..., 3:] == 0).all()


@pytest.mark.parametrize("sm", [2.0, 0.0])
def test_reference_at_the_edges(sm):
    """Enumeration: a value on a bound passes the gradient, the next float beyond it gives +0, -0.0 passes, NaN gives +0;
    with shift_max = 0 exactly the two zeros pass.  The sign of a passed zero gradient is kept, a blocked one is +0."""
    smf = np.float32(sm)
    up, dn = np.nextafter(smf, np.float32(np.inf)), np.nextafter(-smf, np.float32(-np.inf))
    cases = [(-smf, True), (smf, True), (up, False), (dn, False), (np.float32(0.0), True), (np.float32(-0.0), True),
             (np.float32(np.nan), False), (np.float32(np.inf), False), (np.float32(-np.inf), False)]
    for g in (np.float32(1.5), np.float32(-0.0), np.float32(0.0)):
        for v, passes in cases:
            c = np.full((1, 1, 6), v, np.float32)
            out = dref.candidates_grad_ref(c, np.full((1, 1, 3), g, np.float32), sm)
            assert out.dtype == np.float32 and out.shape == (1, 1, 6)
            for d in range(3):
                if passes:
                    assert out[0, 0, d] == g and np.signbit(out[0, 0, d]) == np.signbit(g), (v, g)
                else:
                    assert out[0, 0, d] == 0 and not np.signbit(out[0, 0, d]), (v, g)
            assert (out[0, 0, 3:] == 0).all() and not np.signbit(out[0, 0, 3:]).any()
    assert set(np.abs(dref.edge_values(sm)[:2]).tolist()) == {float(smf)}


def test_prefix_rows_grad_reference_is_the_adjoint():
    """<x[:, :K], g> == <x, pad(g)> on integers (exact), rows K .. M-1 are +0, K == M is the identity."""
    rng = np.random.default_rng(1)
    for K, M, C in ((1, 1, 1), (5, 7, 3), (7, 7, 2)):
        x = rng.integers(-3, 4, (2, M, C)).astype(np.float32)
        g = rng.integers(-3, 4, (2, K, C)).astype(np.float32)
        p = dref.prefix_rows_grad_ref(g, M)
        assert p.shape == x.shape and (x[:, :K] * g).sum() == (x * p).sum()
        assert (p[:, K:] == 0).all() and not np.signbit(p[:, K:]).any()
        if K == M:
            assert np.array_equal(p, g)
    with pytest.raises(AssertionError):
        dref.prefix_rows_grad_ref(np.zeros((1, 3, 2), np.float32), 2)


def test_c_entry_points_refuse_on_the_host(sad):
    """NULL pointers, K < 1, B < 1, negative / NaN shift_max, K > M: SAD_EINVAL; B > 65535: SAD_EUNSUPPORTED.  The pointers are
    fake: nothing is dereferenced, no case reaches a launch."""
    from sad_amd import _lib
    L = _lib.lib()
    p = 0x10000
    f = L.sad_candidates_grad_f32
    for args in ((None, p, 2, 8, 1.0, p), (p, None, 2, 8, 1.0, p), (p, p, 2, 8, 1.0, None), (p, p, 2, 0, 1.0, p), (p, p, 0, 8, 1.0, p),
                 (p, p, 2, 8, -1.0, p), (p, p, 2, 8, float("nan"), p), (p, p, 2, 8, -0.5, p)):
        assert f(*args, None) == -1, args
        assert b"sad_candidates_grad_f32" in L.sad_last_error()
    assert f(p, p, 65536, 8, 1.0, p, None) == -2 and b"65535" in L.sad_last_error()
    assert f(None, p, 65536, 8, 1.0, p, None) == -1                       # (an invalid argument is named before a size)
    f = L.sad_prefix_rows_grad_f32
    for args in ((None, 2, 3, 4, 5, p), (p, 2, 3, 4, 5, None), (p, 0, 3, 4, 5, p), (p, 2, 0, 4, 5, p), (p, 2, 5, 4, 5, p), (p, 2, 3, 4, 0, p),
                 (p + 2, 2, 3, 4, 5, p)):
        assert f(*args, None) == -1, args
        assert b"sad_prefix_rows_grad_f32" in L.sad_last_error()


def test_operators_refuse_before_any_device(sad):
    """Wrong dtype, rank, shape, stride, K > M and a negative / NaN shift_max are judged before devices, so CPU tensors reach
    them; CPU tensors that are otherwise right are refused as such."""
    import torch
    from sad_amd import ops
    c, g = torch.zeros(2, 8, 6), torch.zeros(2, 8, 3)
    with pytest.raises(TypeError, match="c: expected dtype"):
        ops.candidates_grad(c.double(), g, 1.0)
    with pytest.raises(TypeError, match="grad_cand: expected dtype"):
        ops.candidates_grad(c, g.half(), 1.0)
    with pytest.raises(TypeError, match="c: expected a torch.Tensor"):
        ops.candidates_grad(c.numpy(), g, 1.0)
    with pytest.raises(ValueError, match=r"c: expected \[B,K,6\]"):
        ops.candidates_grad(c.view(16, 6), g, 1.0)
    with pytest.raises(ValueError, match=r"c: expected \[B,K,6\]"):
        ops.candidates_grad(torch.zeros(2, 8, 5), g, 1.0)
    with pytest.raises(ValueError, match="grad_cand: expected shape"):
        ops.candidates_grad(c, torch.zeros(2, 7, 3), 1.0)
    with pytest.raises(ValueError, match="grad_cand: must be contiguous"):
        ops.candidates_grad(c, torch.zeros(2, 3, 8).transpose(1, 2), 1.0)
    with pytest.raises(ValueError, match="c: expected 1 <= B"):
        ops.candidates_grad(torch.zeros(0, 8, 6), torch.zeros(0, 8, 3), 1.0)
    for bad in (-1.0, float("nan"), -1e-30):
        with pytest.raises(ValueError, match="shift_max"):
            ops.candidates_grad(c, g, bad)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.candidates_grad(c, g, 1.0)
    assert ops.candidates_grad_output_spec(2, 8) == (("grad_c", (2, 8, 6), torch.float32),)

    x = torch.zeros(2, 5, 3)
    with pytest.raises(TypeError, match="g: expected dtype"):
        ops.prefix_rows_grad(x.double(), 7)
    with pytest.raises(ValueError, match=r"g: expected \[B,K,C\]"):
        ops.prefix_rows_grad(x.view(10, 3), 7)
    with pytest.raises(ValueError, match=r"g: expected \[B,K,C\]"):
        ops.prefix_rows_grad(torch.zeros(2, 0, 3), 7)
    with pytest.raises(ValueError, match="g: must be contiguous"):
        ops.prefix_rows_grad(torch.zeros(2, 3, 5).transpose(1, 2), 7)
    with pytest.raises(ValueError, match="M: expected M >= K = 5"):
        ops.prefix_rows_grad(x, 4)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.prefix_rows_grad(x, 7)
    assert ops.prefix_rows_grad_output_spec(2, 7, 3) == (("out", (2, 7, 3), torch.float32),)

    xyz3 = torch.zeros(2, 10, 3)
    anchor = (3.9, 1.6, 1.56)
    with pytest.raises(TypeError, match="xyz3: expected dtype"):
        ops.candidates(xyz3.double(), c, 8, 1.0, 1.0, 4.8, anchor)
    with pytest.raises(ValueError, match=r"xyz3: expected \[B,M3,3\]"):
        ops.candidates(torch.zeros(2, 10, 4), c, 8, 1.0, 1.0, 4.8, anchor)
    with pytest.raises(ValueError, match="K: expected 1 <= K <= M3 = 10"):
        ops.candidates(xyz3, torch.zeros(2, 11, 6), 11, 1.0, 1.0, 4.8, anchor)
    with pytest.raises(ValueError, match="c: expected shape"):
        ops.candidates(xyz3, c, 7, 1.0, 1.0, 4.8, anchor)
    with pytest.raises(ValueError, match="shift_max"):
        ops.candidates(xyz3, c, 8, -1.0, 1.0, 4.8, anchor)
    with pytest.raises(ValueError, match="anchor: expected 3 values"):
        ops.candidates(xyz3, c, 8, 1.0, 1.0, 4.8, (1.0, 2.0))
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.candidates(xyz3, c, 8, 1.0, 1.0, 4.8, anchor)


def test_out_checks(sad):
    """The checker the operators hand their ``out=`` to, on the operators' own specs, with a CPU device standing in."""
    import torch
    from sad_amd import ops
    cpu = torch.device("cpu")
    for spec, good in ((ops.candidates_grad_output_spec(2, 8), torch.zeros(2, 8, 6)), (ops.prefix_rows_grad_output_spec(2, 7, 3), torch.zeros(2, 7, 3))):
        assert ops._outputs(spec, (good,), cpu, "c")[0] is good
        for bad in (good.double(), good[:, :-1], good.transpose(0, 1).contiguous().transpose(0, 1), good.view(-1)):
            with pytest.raises(ValueError, match="out: expected contiguous"):
                ops._outputs(spec, (bad,), cpu, "c")
        with pytest.raises(ValueError, match="out: expected contiguous"):
            ops._outputs(spec, (good, good), cpu, "c")


def _small_section(orc, seed=0, inputs=None):
    """``inputs``: (xyz3, feat3) to put in place of ``small_inputs`` (the SA stack's own output)."""
    cfg = dref.small_config()
    w = dref.small_weights(cfg, seed)
    xyz3, feat3 = dref.small_inputs(cfg, 2, seed) if inputs is None else inputs
    B, K = 2, cfg.n_cand
    L = len(w["cand"])
    xk = np.ascontiguousarray(feat3[:, :K]).reshape(B * K, -1)
    if orc is not None:
        c = orc.mlp_rows(xk, w["cand"], relu_mask=(1 << (L - 1)) - 1).reshape(B, K, 6)
        cand, radius = orc.candidates(xyz3, c, cfg.shift_max, cfg.r_min, cfg.r_max, cfg.anchor_car)
    else:
        c = dref.rows_chain(None, xk, w["cand"], (1 << (L - 1)) - 1, np.zeros((B * K, 6)))["out"].reshape(B, K, 6).astype(np.float32)
        cand = dref.step2(xyz3[:, :K], c, cfg.shift_max, np.float32)
        radius = np.full((B, K), 0.6, np.float32)
    pairs = [dref.ball_counts(xyz3, cand, radius, sc, S) for sc, S in zip(cfg.cluster_scales, cfg.cluster_nsamples)]
    return cfg, w, xyz3, feat3, c, cand, radius, [p[0] for p in pairs], [p[1] for p in pairs]


def test_small_section_holds_every_population(orc):
    """The shared small cluster section on the oracle's bits: clamped and unclamped shift components, empty and partly filled
    cluster groups all occur (what the GPU test asserts again on the module's own values), and K < M3."""
    cfg, w, xyz3, feat3, c, cand, radius, idxs, cnts = _small_section(orc)
    passes = dref.shift_passes(c, cfg.shift_max)
    print(f"unclamped {int(passes.sum())} of {passes.size}; cnt == 0: {[int((n == 0).sum()) for n in cnts]}; "
          f"0 < cnt < S: {[int(((n > 0) & (n < S)).sum()) for n, S in zip(cnts, cfg.cluster_nsamples)]}; "
          f"radius {radius.min():.2f} .. {radius.max():.2f}")
    assert cfg.n_cand < cfg.stages[-1].npoint
    assert passes.any() and (~passes).any()
    assert any((n == 0).any() for n in cnts) and all(((n > 0) & (n < S)).any() for n, S in zip(cnts, cfg.cluster_nsamples))


def test_composed_reference_against_itself():
    """``cluster_ref`` with float64 activations (``orc=None``): every entry has its shape, A >= |val|, the clamped components
    and the size columns of grad c carry the direct weights only, doubling both loss weights doubles every gradient exactly,
    and the directional derivative along the candidate layer's last bias meets a central difference of the reference's own
    forward (the new path: c -> cand -> relative coordinates -> o).  With the indices fixed the loss is continuous and piecewise
    linear along that direction, so the quotient differs from the slope by (a) the forward's float32 roundings of its rows,
    2^-24 of the summed |terms| (A) divided by h, and (b) the slope changes at the ReLU / arg-max / clamp kinks inside +-h, which
    shrink with h; at h = 2^-7 a tenth of the slope is allowed for them: a lost path, a wrong sign or a factor of two misses it
    by far.  This checks the reference, not the library."""
    cfg, w, xyz3, feat3, c, cand, radius, idxs, cnts = _small_section(None)
    B, K = 2, cfg.n_cand
    rng = np.random.default_rng(3)
    w_o = rng.standard_normal((B, K, cfg.head_mlp[-1]))
    w_c = rng.standard_normal((B, K, 6))
    res = dref.cluster_ref(None, xyz3, feat3, w, K, cfg.shift_max, idxs, cnts, w_o, w_c)
    g = res["grads"]
    for name in dref.param_names(w):
        ch, leaf = name.rsplit(".", 1)
        want = w[ch][int(leaf[1:])][0 if leaf[0] == "W" else 1].shape
        val, A, n = g[name]
        assert val.shape == want and A.shape == want and n > 0, name
        assert (A >= np.abs(val) * (1 - 1e-12)).all(), name
    assert g["feat3"][0].shape == feat3.shape
    passes = dref.shift_passes(res["c"], cfg.shift_max)
    assert passes.any() and (~passes).any()
    gc = g["c"][0]
    assert np.array_equal(gc[..., 3:], w_c[..., 3:]) and np.array_equal(gc[..., :3][~passes], w_c[..., :3][~passes])
    assert (gc[..., :3][passes] != w_c[..., :3][passes]).any()
    twice = dref.cluster_ref(None, xyz3, feat3, w, K, cfg.shift_max, idxs, cnts, 2 * w_o, 2 * w_c)["grads"]
    for name, (val, A, n) in g.items():
        assert np.array_equal(2 * np.asarray(val), twice[name][0]) and n == twice[name][2], name
    # central difference along the last bias of the candidate MLP, with w_c = 0: everything it measures went through cand
    v = rng.standard_normal(6)
    v[3:] = 0.0
    h = 2.0 ** -7
    zero_c = np.zeros_like(w_c)

    def loss(step):
        w2 = dict(w)
        Wl, bl = w["cand"][-1]
        w2["cand"] = list(w["cand"][:-1]) + [(Wl, (bl.astype(np.float64) + step * v))]
        return (dref.cluster_ref(None, xyz3, feat3, w2, K, cfg.shift_max, idxs, cnts, w_o, zero_c)["o"] * w_o).sum()
    last = len(w["cand"]) - 1
    gb = dref.cluster_ref(None, xyz3, feat3, w, K, cfg.shift_max, idxs, cnts, w_o, zero_c)["grads"][f"cand.b{last}"]
    num = (loss(h) - loss(-h)) / (2 * h)
    ana, scale = (gb[0] * v).sum(), (gb[1] * np.abs(v)).sum()
    print(f"directional derivative through cand: analytic {ana:.6f}, central difference {num:.6f}, A {scale:.3f}")
    assert ana != 0
    assert abs(num - ana) <= 0.1 * abs(ana) + 2.0 ** -24 * scale / h


def _small_stack(orc, act):
    """The three SA stages of ``small_config`` on ``small_points`` as ``stack_ref`` takes them: centroids from the oracle's FPS for
    stage 1 and the prefix of the stage before after that (what the detector takes), indices from the brute force
    ``ball_counts`` at the stage's constant radii, features from the reference's own forward on ``act`` (the oracle: §6's bits;
    ``None``: float64 activations, rounded to float32 where a chain hands over to the next, as every chain's input is).
    -> (cfg, weights, stage dicts)."""
    cfg = dref.small_config()
    w = dref.small_weights(cfg)
    pts = dref.small_points(cfg)
    xyz, feat = np.ascontiguousarray(pts[..., :3]), np.ascontiguousarray(pts[..., 3:])
    stages = []
    for s, st in enumerate(cfg.stages, 1):
        new_xyz = orc.gather_xyz(xyz, orc.fps(xyz, st.npoint)) if s == 1 else np.ascontiguousarray(xyz[:, :st.npoint])
        pairs = [dref.ball_counts(xyz, new_xyz, np.full(new_xyz.shape[:2], r, np.float32), 1.0, S) for r, S in zip(st.radii, st.nsamples)]
        stages.append(dict(xyz=xyz, feat=feat, new_xyz=new_xyz, idxs=[p[0] for p in pairs], cnts=[p[1] for p in pairs]))
        xyz, feat = new_xyz, dref.stage_forward(act, stages[-1], w, s)[1].astype(np.float32)
    return cfg, w, stages, (xyz, feat)


def test_small_stack_holds_every_population(orc):
    """The shared small SA stack on the oracle's bits: (192, 4) points in a slab of 4 x 4 x 1; in every stage no empty group, a
    partly filled and a full group in one branch at least, and in every layer of every chain ReLUs both on and off (what the
    GPU tests assert again on the module's own counts and bits)."""
    cfg, w, stages, _ = _small_stack(orc, orc)
    assert stages[0]["xyz"].shape == (2, 192, 3) and stages[0]["feat"].shape == (2, 192, 1)
    assert [st["new_xyz"].shape[1] for st in stages] == [96, 64, 40]
    for a, b in zip(stages[:-1], stages[1:]):
        assert b["xyz"] is a["new_xyz"] and np.array_equal(b["new_xyz"], a["new_xyz"][:, :b["new_xyz"].shape[1]])
    print(dref.stack_populations(orc, stages, w, cfg))


def _ste32(x):
    """x rounded to float32, with the identity as its derivative: a chain's input is a float32 tensor."""
    return x + (x.detach().float().double() - x.detach())


def _t_chain(x, layers, relu_mask):
    import torch
    for l, (W, b) in enumerate(layers):
        x = x @ W.T + b
        if (relu_mask >> l) & 1:
            x = torch.relu(x)
    return x


def _t_grouped(xyz, feat, new_xyz, idx, cnt, layers):
    """The unfused grouped chain in torch float64: index gather, relative coordinates, linear + ReLU layers, max over the slots
    that exist (slots < max(cnt, 1)).  xyz: numpy; feat [B,N,C] | None and new_xyz [B,M,3]: float64 tensors."""
    import torch
    B, M, S = idx.shape
    bb, mm, ss = np.nonzero(np.arange(S)[None, None, :] < np.clip(cnt, 1, S)[..., None])
    src = idx[bb, mm, ss]
    x0 = torch.from_numpy(xyz.astype(np.float64))[bb, src] - new_xyz[bb, mm]
    if feat is not None:
        x0 = torch.cat([x0, feat[bb, src]], 1)
    y = _t_chain(_ste32(x0), layers, (1 << len(layers)) - 1)
    slots = torch.full((B * M, S, y.shape[1]), -np.inf, dtype=torch.float64)
    slots = slots.index_put((torch.from_numpy(bb * M + mm), torch.from_numpy(ss)), y)
    return slots.max(1).values.reshape(B, M, -1)


def _torch_gradients(cfg, w, stages, xyz3, idxs, cnts, w_o, w_c):
    """d ((o * w_o).sum() + (c * w_c).sum()) by torch autograd in float64 on the unfused composition, on the fixed indices of
    ``stages`` (SA) and ``idxs`` / ``cnts`` (cluster) -> {name: array} under the names of ``stack_ref`` / ``cluster_ref``."""
    import torch
    tw = {n: [(torch.tensor(W, dtype=torch.float64, requires_grad=True), torch.tensor(b, dtype=torch.float64, requires_grad=True))
              for W, b in layers] for n, layers in w.items()}
    kept = {}
    feat = torch.tensor(stages[0]["feat"], dtype=torch.float64, requires_grad=True)
    kept["feat1"] = feat
    for s, st in enumerate(stages, 1):
        new_xyz = torch.from_numpy(st["new_xyz"].astype(np.float64))
        cat = torch.cat([_t_grouped(st["xyz"], feat, new_xyz, i, n, tw[f"sa{s}.b{k}"]) for k, (i, n) in enumerate(zip(st["idxs"], st["cnts"]))], 2)
        feat = _t_chain(_ste32(cat), tw[f"sa{s}.agg"], 1)
        feat.retain_grad()
        kept[f"feat{s + 1}" if s < len(stages) else "cluster.feat3"] = feat
    K, sm = cfg.n_cand, cfg.shift_max
    mask = lambda layers: (1 << (len(layers) - 1)) - 1
    c = _t_chain(_ste32(feat[:, :K]), tw["cand"], mask(tw["cand"]))
    cand = _ste32(torch.from_numpy(xyz3[:, :K].astype(np.float64)) + torch.clamp(c[..., :3], -sm, sm))
    for name, t in (("c", c), ("cand_xyz", cand)):
        t.retain_grad()
        kept[name] = t
    cat = torch.cat([_t_grouped(xyz3, feat, cand, i, n, tw[f"cluster.b{k}"]) for k, (i, n) in enumerate(zip(idxs, cnts))], 2)
    o = _t_chain(_ste32(_t_chain(_ste32(cat), tw["cluster.agg"], 1)), tw["head"], mask(tw["head"]))
    ((o * torch.from_numpy(w_o)).sum() + (c * torch.from_numpy(w_c)).sum()).backward()
    got = {n: t.grad.numpy() for n, t in kept.items()}
    for n, layers in tw.items():
        for l, (W, b) in enumerate(layers):
            got[f"{n}.W{l}"], got[f"{n}.b{l}"] = W.grad.numpy(), b.grad.numpy()
    return got, o.detach().numpy()


def test_stack_reference_against_autograd(orc):
    """``stack_ref`` below ``cluster_ref`` with float64 activations (``orc=None``; the oracle only samples stage 1's centroids)
    against torch autograd in float64 on the unfused composition on the same fixed indices: every parameter of every chain, the
    gradient at every stage's input features, at c and at cand agree within 1e-10 A (float64 sums in another order; a lost
    consumer, a wrong column slice or a wrong ReLU decision is of the order of A), A >= |val| everywhere, the depths grow from
    the last stage to the first, and doubling both loss weights doubles every value exactly.  This checks the reference, not
    the library."""
    cfg, w, stages, (xyz3, feat3) = _small_stack(orc, None)
    print(dref.stack_populations(None, stages, w, cfg))
    _, _, _, _, c, cand, radius, idxs, cnts = _small_section(None, inputs=(xyz3, feat3))
    B, K = 2, cfg.n_cand
    rng = np.random.default_rng(6)
    w_o = rng.standard_normal((B, K, cfg.head_mlp[-1]))
    w_c = rng.standard_normal((B, K, 6))

    def reference(scale):
        cl = dref.cluster_ref(None, xyz3, feat3, w, K, cfg.shift_max, idxs, cnts, scale * w_o, scale * w_c)
        st = dref.stack_ref(None, stages, w, cl["grads"]["feat3"])
        grads = {("cluster.feat3" if n == "feat3" else n): e for n, e in cl["grads"].items()}
        assert not set(grads) & set(st["grads"])
        grads.update(st["grads"])
        return cl, st, grads
    cl, st, grads = reference(1.0)
    assert np.array_equal(st["out3"].astype(np.float32), feat3)       # (the indices are fixed: that _small_section placed its candidates in float32 decides nothing)
    names = dref.param_names(w) + dref.param_names(w, dref.stack_chains(cfg)) + ["feat1", "feat2", "feat3", "cluster.feat3", "c", "cand_xyz"]
    assert sorted(names) == sorted(grads) and len(names) == len(set(names))
    got, o = _torch_gradients(cfg, w, stages, xyz3, idxs, cnts, w_o, w_c)
    assert np.abs(o - cl["o"]).max() <= 1e-12 * np.abs(o).max()
    worst = 0.0
    for name in names:
        val, A, n = grads[name]
        assert got[name].shape == np.shape(val) == np.shape(A), name
        assert (A >= np.abs(val) * (1 - 1e-12)).all() and (A > 0).any(), name
        err = np.abs(got[name] - val)
        assert (err <= 1e-10 * A).all(), f"{name}: {int((err > 1e-10 * A).sum())} elements differ from autograd, worst {np.max(err / np.maximum(A, 1e-300)):.3e} A"
        worst = max(worst, float(np.max(err[A > 0] / A[A > 0])))
    print(f"worst |reference - autograd| / A over {len(names)} entries: {worst:.3e}")
    depth = [grads[f"sa{s}.agg.W0"][2] for s in (3, 2, 1)]
    assert grads["cluster.feat3"][2] < depth[0] < depth[1] < depth[2], depth
    _, _, twice = reference(2.0)
    for name, (val, A, n) in grads.items():
        assert np.array_equal(2 * np.asarray(val), twice[name][0]) and np.array_equal(2 * np.asarray(A), twice[name][1]) and n == twice[name][2], name
