"""The MLP chain backward on the GPU (SPEC.md §32): ``ops.grouped_mlp_grad`` / ``ops.mlp_rows_grad`` against the numpy reference of
tests/mlp_grad_ref.py, and the autograd functions and modules built on them.

General inputs: every output within n * 2^-23 * A of the float64 reference (A: the same sum over absolute values, n: the rows
summed + the widths of the layers passed + L; derived, §21.4's bound carried through the chain), the reference's exact zeros exact,
``mismatch == 0``.  Lattice inputs (exactly summable, checked on the CPU in tests/test_mlp_grad_cpu.py): equality, and two calls
bit-equal.  The shapes are the smallest at which the kernels take every path (mlp_grad_ref.GROUPED_CASES)."""
import numpy as np
import pytest

import mlp_grad_ref as ref

pytestmark = pytest.mark.gpu


def _t(a, dev):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _layers(layers, dev):
    return [(_t(w, dev), _t(b, dev)) for w, b in layers]


def _forward(dev, inp, layers):
    """The library's own forward of the case: pooled [B,M,C_L]."""
    from sad_amd import ops
    mlp = ops.PackedMLP(layers, True, dev)
    return mlp.grouped(_t(inp["xyz"], dev), _t(inp["feat"], dev), _t(inp["new_xyz"], dev), _t(inp["idx"], dev), cnt=_t(inp["cnt"], dev))


def _grouped(dev, inp, layers, pooled, grad_out, **kw):
    from sad_amd import ops
    return ops.grouped_mlp_grad(_t(inp["xyz"], dev), _t(inp["feat"], dev), _t(inp["new_xyz"], dev), _t(inp["idx"], dev), _t(inp["cnt"], dev),
                                _layers(layers, dev), pooled, grad_out, skip_empty=inp["skip_empty"], **kw)


def _np(t):
    return None if t is None else t.detach().cpu().numpy()


def _check_grouped(res, got, exact, names=("grad_feat", "grad_xyz", "grad_new_xyz", "params")):
    gf, gx, gn, gW, gb, mismatch = got
    assert int(mismatch.item()) == 0, f"mismatch = {int(mismatch.item())}: the recompute does not meet the forward's pooled values"
    for name, g in (("grad_feat", gf), ("grad_xyz", gx), ("grad_new_xyz", gn)):
        if name in names and name in res["val"]:
            ref.check_close(name, _np(g), res["val"][name], res["A"][name], res["depth"][name], exact)
        else:
            assert g is None or name in res["val"], name
    if "params" in names:
        for l in range(len(gW)):
            ref.check_close(f"grad_W[{l}]", _np(gW[l]), res["val"]["grad_W"][l], res["A"]["grad_W"][l], res["depth"]["grad_W"][l], exact)
            ref.check_close(f"grad_b[{l}]", _np(gb[l]), res["val"]["grad_b"][l], res["A"]["grad_b"][l], res["depth"]["grad_b"][l], exact)


@pytest.mark.parametrize("lattice", [False, True], ids=["general", "lattice"])
@pytest.mark.parametrize("name", sorted(ref.GROUPED_CASES))
def test_grouped_against_reference(sad, dev, orc, name, lattice):
    import torch
    inp, layers, grad_out = ref.grouped_case(name, lattice)
    res = ref.grouped_ref(orc, layers=layers, grad_out=grad_out, **inp)
    pooled = _forward(dev, inp, layers)
    got = _grouped(dev, inp, layers, pooled, _t(grad_out, dev))
    _check_grouped(res, got, exact=lattice)
    print(f"{name}: {res['rows']} rows of {inp['idx'].size} slots, forward equals the oracle's bits: "
          f"{np.array_equal(np.where((inp['cnt'] == 0)[..., None], 0, _np(pooled)) if inp['skip_empty'] else _np(pooled), res['pooled'])}")
    if lattice:
        again = _grouped(dev, inp, layers, pooled, _t(grad_out, dev))
        for a, b in zip(got[:3] + tuple(got[3]) + tuple(got[4]), again[:3] + tuple(again[3]) + tuple(again[4])):
            assert (a is None and b is None) or torch.equal(a, b), "two calls differ on exactly summable inputs"


def test_grad_out_and_pooled_as_column_slices(sad, dev, orc):
    """grad_out / pooled read where they lie in wider buffers (a branch's slice of a stage's concatenated buffer)."""
    import torch
    inp, layers, grad_out = ref.grouped_case("L2_C1_S16_mixed", False)
    res = ref.grouped_ref(orc, layers=layers, grad_out=grad_out, **inp)
    pooled = _forward(dev, inp, layers)
    B, M, CL = grad_out.shape
    wide_g = torch.full((B, M, CL + 7), float("nan"), device=dev)
    wide_g[:, :, 5:5 + CL] = _t(grad_out, dev)
    wide_p = torch.full((B, M, CL + 3), float("nan"), device=dev)
    wide_p[:, :, 2:2 + CL] = pooled
    _check_grouped(res, _grouped(dev, inp, layers, wide_p, wide_g, col_off=5, pooled_off=2), exact=False)
    # a strided view (not rows at one stride) goes through a packed copy
    _check_grouped(res, _grouped(dev, inp, layers, pooled, _t(grad_out, dev).transpose(0, 1).contiguous().transpose(0, 1)), exact=False)


def test_every_need_combination(sad, dev, orc):
    """What is not asked for is not returned, what is asked for does not depend on the rest ("parameters only" included)."""
    inp, layers, grad_out = ref.grouped_case("L3_C5_S33_mixed_B2", True)
    res = ref.grouped_ref(orc, layers=layers, grad_out=grad_out, **inp)
    pooled, g = _forward(dev, inp, layers), _t(grad_out, dev)
    names = ("feat", "xyz", "new_xyz", "params")
    for mask in range(1, 16):
        need = [n for i, n in enumerate(names) if (mask >> i) & 1]
        got = _grouped(dev, inp, layers, pooled, g, need=need)
        for i, n in enumerate(names[:3]):
            assert (got[i] is not None) == (n in need), (need, n)
        assert (got[3] is not None) == (got[4] is not None) == ("params" in need)
        _check_grouped(res, got, exact=True, names=tuple("grad_" + n if n != "params" else n for n in need))


@pytest.mark.parametrize("lattice", [False, True], ids=["general", "lattice"])
def test_chunked_workspace(sad, dev, orc, lattice):
    """A workspace of the minimum size: 200 groups in chunks of 64 (four chunks); the same bound, and equality on the lattice."""
    from sad_amd import ops
    import torch
    rng = np.random.default_rng(11 + lattice)
    B, N, M, S, C, widths = 2, 60, 100, 16, 5, [33, 10]
    xyz, feat, new_xyz, idx, cnt = ref.make_grouped(rng, B, N, M, S, C, "mixed", lattice)
    inp = dict(xyz=xyz, feat=feat, new_xyz=new_xyz, idx=idx, cnt=cnt, skip_empty=False)
    layers = ref.make_layers(rng, [3 + C] + widths, lattice)
    grad_out = ref.make_grad(rng, (B, M, widths[-1]), lattice)
    res = ref.grouped_ref(orc, layers=layers, grad_out=grad_out, **inp)
    lo, hi = ops.mlp_grad_workspace_bytes(B, M, S, [3 + C] + widths, True, True)
    assert lo < hi and B * M > 3 * 64                            # (a chunk of the minimum workspace is 64 groups)
    pooled = _forward(dev, inp, layers)
    ws = torch.empty(lo, dtype=torch.uint8, device=dev)
    got = _grouped(dev, inp, layers, pooled, _t(grad_out, dev), workspace=ws)
    _check_grouped(res, got, exact=lattice)
    whole = _grouped(dev, inp, layers, pooled, _t(grad_out, dev), budget_bytes=hi)
    _check_grouped(res, whole, exact=lattice)
    with pytest.raises(ValueError, match="workspace"):
        _grouped(dev, inp, layers, pooled, _t(grad_out, dev), workspace=torch.empty(lo - 16, dtype=torch.uint8, device=dev))


@pytest.mark.parametrize("mask", sorted(ref.ROWS_MASKS))
@pytest.mark.parametrize("R", ref.ROWS_R)
def test_rows_against_reference(sad, dev, orc, R, mask):
    from sad_amd import ops
    import torch
    m = ref.ROWS_MASKS[mask]
    for lattice in (False, True):
        x, layers, grad_out = ref.rows_case(R, lattice)
        res = ref.rows_ref(orc, x, layers, m, grad_out)
        calls = [dict()]
        if R == 1000:                                            # the minimum workspace: chunks of 64 rows
            lo, _ = ops.mlp_grad_workspace_bytes(1, R, 1, ref.ROWS_DIMS, False, False)
            calls.append(dict(workspace=torch.empty(lo, dtype=torch.uint8, device=dev)))
        for kw in calls:
            gx, gW, gb = ops.mlp_rows_grad(_t(x, dev), _layers(layers, dev), _t(grad_out, dev), relu_mask=m, **kw)
            ref.check_close("grad_x", _np(gx), res["val"]["grad_x"], res["A"]["grad_x"], res["depth"]["grad_x"], lattice)
            for l in range(len(layers)):
                ref.check_close(f"grad_W[{l}]", _np(gW[l]), res["val"]["grad_W"][l], res["A"]["grad_W"][l], res["depth"]["grad_W"][l], lattice)
                ref.check_close(f"grad_b[{l}]", _np(gb[l]), res["val"]["grad_b"][l], res["A"]["grad_b"][l], res["depth"]["grad_b"][l], lattice)
        gx, gW, gb = ops.mlp_rows_grad(_t(x, dev), _layers(layers, dev), _t(grad_out, dev), relu_mask=m, need=("params",))
        assert gx is None and len(gW) == len(gb) == len(layers)
        gx, gW, gb = ops.mlp_rows_grad(_t(x, dev), _layers(layers, dev), _t(grad_out, dev), relu_mask=m, need=("feat",))
        assert gW is None and gb is None
        ref.check_close("grad_x alone", _np(gx), res["val"]["grad_x"], res["A"]["grad_x"], res["depth"]["grad_x"], lattice)


def test_nan_coordinates_of_skipped_groups(sad, dev, orc):
    """NaN new_xyz rows with cnt == 0 under skip_empty: every gradient finite (check_close asserts it), those groups' grad_new_xyz
    exactly 0, everything else as the reference, which never sees those rows."""
    inp, layers, grad_out = ref.grouped_case("L3_C5_S33_skip_B2", False)
    empty = inp["cnt"] == 0
    assert empty.any() and not empty.all()
    inp["new_xyz"] = inp["new_xyz"].copy()
    inp["new_xyz"][empty] = np.nan
    with np.errstate(all="ignore"):
        res = ref.grouped_ref(orc, layers=layers, grad_out=grad_out, **inp)
    pooled = _forward(dev, inp, layers)
    got = _grouped(dev, inp, layers, pooled, _t(grad_out, dev))
    _check_grouped(res, got, exact=False)
    assert (_np(got[2])[empty] == 0).all()


def test_shared_mlp_autograd(sad, dev, orc):
    """SharedMLP.grouped(...).square().sum().backward() is the reference at grad_out = 2 pooled; the training path's forward is the
    no_grad path's, bit for bit; parameters, features and both coordinate tensors receive their gradients."""
    import torch
    from sad_amd import autograd
    from sad_amd.shared_mlp import SharedMLP
    inp, layers, _ = ref.grouped_case("L3_C5_S33_mixed_B2", False)
    c = ref.GROUPED_CASES["L3_C5_S33_mixed_B2"]
    m = SharedMLP([3 + c["C"]] + c["widths"], True, layers=layers).to(dev)
    xyz, feat, new_xyz, idx, cnt = (_t(inp[k], dev) for k in ("xyz", "feat", "new_xyz", "idx", "cnt"))
    with torch.no_grad():
        plain = m.grouped(xyz, feat, new_xyz, idx, cnt)
    assert not plain.requires_grad and not m.grouped(xyz, feat, new_xyz, idx, cnt).requires_grad      # nothing requires grad
    m.requires_grad_(True)
    for t in (xyz, feat, new_xyz):
        t.requires_grad_(True)
    out = m.grouped(xyz, feat, new_xyz, idx, cnt)
    assert out.requires_grad and torch.equal(out.detach(), plain)
    out.square().sum().backward()
    res = ref.grouped_ref(orc, layers=layers, grad_out=2.0 * res_pooled(orc, inp, layers), **inp)
    print(f"forward equals the oracle's bits: {np.array_equal(res['pooled'], plain.cpu().numpy())}")
    got = (feat.grad, xyz.grad, new_xyz.grad, [w.grad for w in m.weight], [b.grad for b in m.bias], autograd.GroupedMLP.last_mismatch)
    _check_grouped(res, got, exact=False)
    # plain rows through the same module class
    x, rl, g = ref.rows_case(65, False)
    r = SharedMLP(ref.ROWS_DIMS, False, relu_mask=5, layers=rl).to(dev)
    xt = _t(x, dev)
    with torch.no_grad():
        plain = r.rows(xt)
    r.requires_grad_(True)
    xt.requires_grad_(True)
    y = r.rows(xt)
    assert torch.equal(y.detach(), plain)
    (y * _t(g, dev)).sum().backward()
    rr = ref.rows_ref(orc, x, rl, 5, g)
    ref.check_close("rows grad_x", _np(xt.grad), rr["val"]["grad_x"], rr["A"]["grad_x"], rr["depth"]["grad_x"])
    for l in range(3):
        ref.check_close(f"rows grad_W[{l}]", _np(r.weight[l].grad), rr["val"]["grad_W"][l], rr["A"]["grad_W"][l], rr["depth"]["grad_W"][l])
        ref.check_close(f"rows grad_b[{l}]", _np(r.bias[l].grad), rr["val"]["grad_b"][l], rr["A"]["grad_b"][l], rr["depth"]["grad_b"][l])


def res_pooled(orc, inp, layers):
    z = np.zeros(inp["idx"].shape[:2] + (layers[-1][0].shape[0],), np.float32)
    return ref.grouped_ref(orc, layers=layers, grad_out=z, **inp)["pooled"]


def test_sa_module_train(sad, dev, orc):
    """A two-branch stage with aggregation: without gradients the output equals SAModuleMSG's on the exported weights; with them
    every parameter and the input features get the gradient of the reference composed stage by stage (aggregation rows, then each
    branch with the aggregation's grad_x slice as its grad_out; n and A add up along the composition)."""
    import torch
    from sad_amd import ops
    from sad_amd.config import SAStage
    from sad_amd.sa_module import SAModuleMSG, SAModuleMSGTrain
    st = SAStage(24, (0.6, 1.2), (8, 16), ((16, 16), (16, 33)), 20)
    B, N, C = 2, 96, 4
    rng = np.random.default_rng(5)
    xyz = rng.uniform(-1.5, 1.5, (B, N, 3)).astype(np.float32)
    feat = rng.standard_normal((B, N, C)).astype(np.float32)
    m = SAModuleMSGTrain(C, st, dev, seed=3)
    xt, ft = _t(xyz, dev), _t(feat, dev)
    with torch.no_grad():
        new_xyz, plain = m.forward_pm(xt, ft)
        want_xyz, want = SAModuleMSG(C, st, dev, weights=m.export()).forward_pm(xt, ft)
    assert torch.equal(new_xyz, want_xyz) and torch.equal(plain, want)
    m.requires_grad_(True)
    ft.requires_grad_(True)
    _, out = m.forward_pm(xt, ft)
    assert torch.equal(out.detach(), plain)
    gw = rng.standard_normal(tuple(out.shape)).astype(np.float32)
    (out * _t(gw, dev)).sum().backward()
    # the reference, on the indices the stage used
    with torch.no_grad():
        idxs, cnts = ops.ball_query_multi(st.radii, st.nsamples, xt, new_xyz, None, return_counts=True)
    w = m.export()
    M = st.npoint
    branch = [dict(xyz=xyz, feat=feat, new_xyz=new_xyz.cpu().numpy(), idx=i.cpu().numpy(), cnt=c.cpu().numpy(), skip_empty=False)
              for i, c in zip(idxs, cnts)]
    cat = np.concatenate([res_pooled(orc, inp, w[f"b{k}"]) for k, inp in enumerate(branch)], 2)
    agg = ref.rows_ref(orc, cat.reshape(B * M, -1), w["agg"], 1, gw.reshape(B * M, -1))
    print(f"stage output equals the oracle's bits: {np.array_equal(agg['out'].reshape(B, M, -1), plain.cpu().numpy())}")
    ref.check_close("agg grad_W", _np(m.agg.weight[0].grad), agg["val"]["grad_W"][0], agg["A"]["grad_W"][0], agg["depth"]["grad_W"][0])
    ref.check_close("agg grad_b", _np(m.agg.bias[0].grad), agg["val"]["grad_b"][0], agg["A"]["grad_b"][0], agg["depth"]["grad_b"][0])
    gf, gfA, off = 0.0, 0.0, 0
    for k, inp in enumerate(branch):
        co = st.mlps[k][-1]
        go = agg["val"]["grad_x"][:, off:off + co].reshape(B, M, co)
        goA = agg["A"]["grad_x"][:, off:off + co].reshape(B, M, co)
        r = ref.grouped_ref(orc, layers=w[f"b{k}"], grad_out=go, grad_out_A=goA, **inp)
        extra = agg["depth"]["grad_x"]
        for l in range(len(w[f"b{k}"])):
            ref.check_close(f"b{k} grad_W[{l}]", _np(m.branches[k].weight[l].grad), r["val"]["grad_W"][l], r["A"]["grad_W"][l], r["depth"]["grad_W"][l] + extra)
            ref.check_close(f"b{k} grad_b[{l}]", _np(m.branches[k].bias[l].grad), r["val"]["grad_b"][l], r["A"]["grad_b"][l], r["depth"]["grad_b"][l] + extra)
        gf, gfA, depth = gf + r["val"]["grad_feat"], gfA + r["A"]["grad_feat"], r["depth"]["grad_feat"] + extra
        off += co
    ref.check_close("grad_feat", _np(ft.grad), gf, gfA, 2 * depth + 1)


def test_stage_without_input_features(sad, dev, orc):
    """The same stage on coordinates alone (``in_channels = 0``, ``feat_pm=None``, a leaf xyz that does not require grad) through
    the module class: the no_grad forward equals SAModuleMSG's on the exported weights; every parameter gradient lies within
    the composed bound (``detector_train_ref.stack_ref`` on the one stage: C = 0 in ``grouped_ref``, no grad_feat to hand on)."""
    import torch
    import detector_train_ref as dref
    from sad_amd import ops
    from sad_amd.config import SAStage
    from sad_amd.sa_module import SAModuleMSG, SAModuleMSGTrain
    st = SAStage(24, (0.6, 1.2), (8, 16), ((16, 16), (16, 33)), 20)
    B, N = 2, 96
    rng = np.random.default_rng(6)
    xyz = rng.uniform(-1.5, 1.5, (B, N, 3)).astype(np.float32)
    m = SAModuleMSGTrain(0, st, dev, seed=4)
    assert m.branches[0].dims[0] == 3
    xt = _t(xyz, dev)
    with torch.no_grad():
        new_xyz, plain = m.forward_pm(xt, None)
        want_xyz, want = SAModuleMSG(0, st, dev, weights=m.export()).forward_pm(xt, None)
        idxs, cnts = ops.ball_query_multi(st.radii, st.nsamples, xt, new_xyz, None, return_counts=True)
    assert torch.equal(new_xyz, want_xyz) and torch.equal(plain, want)
    assert any(((c > 0) & (c < S)).any() and (c == S).any() for c, S in zip(cnts, st.nsamples)), "partly filled and full groups are both needed"
    m.requires_grad_(True)
    assert xt.is_leaf and not xt.requires_grad
    _, out = m.forward_pm(xt, None)
    assert out.requires_grad and torch.equal(out.detach(), plain)
    gw = rng.standard_normal(tuple(out.shape)).astype(np.float32)
    (out * _t(gw, dev)).sum().backward()
    assert xt.grad is None
    w = {f"sa1.{k}": v for k, v in m.export().items()}
    stage = dict(xyz=xyz, feat=None, new_xyz=_np(new_xyz), idxs=[_np(i) for i in idxs], cnts=[_np(c) for c in cnts])
    res = dref.stack_ref(orc, [stage], w, (gw.astype(np.float64), np.abs(gw).astype(np.float64), 0))
    assert np.array_equal(res["out1"], _np(plain)), "the reference's forward is not the module's output"
    assert "feat1" not in res["grads"] and len(res["grads"]) == 10
    for name, chain in [("b0", m.branches[0]), ("b1", m.branches[1]), ("agg", m.agg)]:
        for l in range(len(chain.weight)):
            dref.check(f"{name} grad_W[{l}]", _np(chain.weight[l].grad), res["grads"][f"sa1.{name}.W{l}"])
            dref.check(f"{name} grad_b[{l}]", _np(chain.bias[l].grad), res["grads"][f"sa1.{name}.b{l}"])


def test_voxel_roi_pool_fused_grad(sad, dev):
    """VoxelRoIPool(fused_grad=True): its forward equals the inference path; at one small shape (2 scales, G = 2, a few hundred
    voxels, RoIs beyond roi_count and an empty scene) the parameter and feature gradients of BOTH training paths lie within the
    bound of a float64 evaluation of the unfused composition on the same indices (so no two float32 results are compared)."""
    import torch
    import test_gpu_voxel_roi as vr
    import voxel_roi_ref
    from sad_amd import synth
    G, C, mlp = 2, 16, [16, 33]
    levels, rois, count = vr._scene(C, 7)
    rng = np.random.default_rng(8)
    layers = [synth.make_mlp_weights([3 + C] + mlp, rng) for _ in levels]
    indices, pts = vr._reference_indices(levels, rois, count, G)
    gw = rng.standard_normal((len(pts), 2 * mlp[-1])).astype(np.float32)
    grads = {}
    for fused in (False, True):
        m = vr._module(sad, dev, levels, G, mlp, layers)
        m.fused_grad = fused
        with torch.no_grad():
            plain = m(_t(rois, dev), _t(count, dev), vr._tensors(sad, dev, levels))
        m.requires_grad_(True)
        tensors = vr._tensors(sad, dev, levels, grad=True)
        out = m(_t(rois, dev), _t(count, dev), tensors)
        if fused:
            assert torch.equal(out.detach(), plain), "the fused training path's forward is not the inference path's"
        (out.reshape(len(pts), -1) * _t(gw, dev)).sum().backward()
        grads[fused] = ([t.feat.grad for t in tensors], [[w.grad for w in ws] for ws in m.weight], [[b.grad for b in bs] for bs in m.bias])
    for k, ((c, _, _, vs, feat), (idx, cnt)) in enumerate(zip(levels, indices)):
        assert (cnt == 0).any() and not np.isfinite(pts).all()
        xyz = voxel_roi_ref.centres(c[:, ::-1], vs, vr.EXACT_PR[:3]).astype(np.float32)
        inp = dict(xyz=xyz[None], feat=feat[None], new_xyz=pts[None].astype(np.float32), idx=idx[None].astype(np.int32),
                   cnt=cnt[None].astype(np.int32), skip_empty=True)
        go = gw[None, :, mlp[-1] * k:mlp[-1] * (k + 1)]
        with np.errstate(all="ignore"):
            r = ref.grouped_ref(None, layers=layers[k], grad_out=go, **inp)          # float64 activations and decisions
        for fused in (False, True):
            gf, gW, gb = grads[fused]
            tag = f"scale {k} {'fused' if fused else 'unfused'}"
            ref.check_close(f"{tag} grad_feat", _np(gf[k])[None], r["val"]["grad_feat"], r["A"]["grad_feat"], r["depth"]["grad_feat"])
            for l in range(len(mlp)):
                ref.check_close(f"{tag} grad_W[{l}]", _np(gW[k][l]), r["val"]["grad_W"][l], r["A"]["grad_W"][l], r["depth"]["grad_W"][l])
                ref.check_close(f"{tag} grad_b[{l}]", _np(gb[k][l]), r["val"]["grad_b"][l], r["A"]["grad_b"][l], r["depth"]["grad_b"][l])
