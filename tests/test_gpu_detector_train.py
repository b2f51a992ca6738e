"""The candidate layer's backward and ``SADDetectorTrain`` on the GPU (SPEC.md §33).

``ops.candidates_grad`` / ``ops.prefix_rows_grad`` are selections and copies: compared with the numpy reference of
tests/detector_train_ref.py bit for bit.  The cluster section and the whole detector are compared with the float64 composition
``detector_train_ref.cluster_ref`` on the indices the module used, every parameter within n * 2^-23 * A (mlp_grad_ref's bound,
n and A added up along the composition), and with ``SADDetector`` on the exported weights under ``torch.equal``.  The SA stages'
gradients are compared with ``detector_train_ref.stack_ref`` below that: composed, with parts frozen, accumulated over two
passes, and link by link."""
import ctypes

import numpy as np
import pytest

import detector_train_ref as dref

pytestmark = pytest.mark.gpu


def _t(a, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _np(t):
    return t.detach().cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("K", [1, 255, 256, 257, 300])
def test_candidates_grad_equals_the_reference(sad, dev, K):
    """B = 2; c from the edge set (both bounds, the next float beyond, both zeros, NaN, infinities) mixed with normals, at
    shift_max = 2 and 0; the same bits as the reference, both signs of zero among them; a NaN-filled ``out`` comes back fully
    written; two calls are bit-equal."""
    import torch
    from sad_amd import ops
    for sm in (2.0, 0.0):
        c, g = dref.edge_case(2, K, sm)
        want = dref.candidates_grad_ref(c, g, sm)
        if K >= 255:
            zero = want[..., :3] == 0
            assert (zero & np.signbit(want[..., :3])).any() and (zero & ~np.signbit(want[..., :3])).any()
            assert np.isnan(c[..., :3]).any() and (c[..., :3] == np.float32(sm)).any() and (c[..., :3] == -np.float32(sm)).any()
        out = torch.full((2, K, 6), float("nan"), device=dev)
        got = ops.candidates_grad(_t(c, dev), _t(g, dev), sm, out=out)
        assert got is out
        res = _np(got)
        assert not np.isnan(res).any(), "an element of out was not written"
        assert np.array_equal(_bits(res), _bits(want)), f"K = {K}, shift_max = {sm}: {int((_bits(res) != _bits(want)).sum())} elements differ"
        again = ops.candidates_grad(_t(c, dev), _t(g, dev), sm)
        assert torch.equal(again.view(torch.int32), got.view(torch.int32))


def test_candidates_grad_refusals_on_the_device(sad, dev):
    import torch
    from sad_amd import ops
    c, g = torch.zeros(2, 8, 6, device=dev), torch.zeros(2, 8, 3, device=dev)
    for bad in (-1.0, float("nan")):
        with pytest.raises(ValueError, match="shift_max"):
            ops.candidates_grad(c, g, bad)
    with pytest.raises(ValueError, match="grad_cand: expected shape"):
        ops.candidates_grad(c, torch.zeros(2, 8, 4, device=dev), 1.0)
    with pytest.raises(TypeError, match="c: expected dtype"):
        ops.candidates_grad(c.half(), g, 1.0)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.candidates_grad(c, g.cpu(), 1.0)
    for bad in (torch.zeros(2, 8, 5, device=dev), torch.zeros(2, 8, 6, device=dev, dtype=torch.float64), torch.zeros(2, 8, 6),
                torch.zeros(2, 6, 8, device=dev).transpose(1, 2)):
        with pytest.raises(ValueError, match="out: expected contiguous"):
            ops.candidates_grad(c, g, 1.0, out=bad)
    with pytest.raises(ValueError, match="M: expected M >= K"):
        ops.prefix_rows_grad(g, 7)
    with pytest.raises(ValueError, match="out: expected contiguous"):
        ops.prefix_rows_grad(g, 9, out=torch.zeros(2, 8, 3, device=dev))
    L = sad._lib.lib()
    assert L.sad_candidates_grad_f32(c.data_ptr(), g.data_ptr(), 2, 8, -1.0, c.data_ptr(), None) == -1
    assert L.sad_prefix_rows_grad_f32(g.data_ptr(), 2, 8, 7, 3, c.data_ptr(), None) == -1


@pytest.mark.parametrize("K,M,C", [(1, 1, 1), (5, 7, 3), (64, 128, 256), (300, 300, 6)])
def test_prefix_rows_grad_equals_the_reference(sad, dev, K, M, C):
    """B = 2, a NaN-filled ``out``: rows < K are g's bits, rows K .. M-1 are +0; through ``autograd.PrefixRows`` the same lands in
    ``x.grad``, and K == M hands back the input's storage."""
    import torch
    from sad_amd import autograd, ops
    rng = np.random.default_rng([K, M, C])
    g = rng.standard_normal((2, K, C)).astype(np.float32)
    g.reshape(-1)[::5] = -0.0
    want = dref.prefix_rows_grad_ref(g, M)
    out = torch.full((2, M, C), float("nan"), device=dev)
    got = ops.prefix_rows_grad(_t(g, dev), M, out=out)
    assert got is out and np.array_equal(_bits(_np(got)), _bits(want))
    x = _t(rng.standard_normal((2, M, C)).astype(np.float32), dev).requires_grad_(True)
    y = autograd.PrefixRows.apply(x, K)
    assert torch.equal(y.detach(), x.detach()[:, :K])
    if K == M:
        assert y.data_ptr() == x.data_ptr(), "K == M: expected the identity, no copy"
    else:
        assert y.is_contiguous() and y.data_ptr() != x.data_ptr()
    y.backward(_t(g, dev))
    assert np.array_equal(_bits(_np(x.grad)), _bits(want))


def test_candidates_autograd(sad, dev):
    """``autograd.Candidates``: cand and radius are the bits of a direct sad_candidates_f32 call, radius does not require grad,
    and ``cand.backward(g)`` leaves exactly ``candidates_grad(c, g)`` in ``c.grad``."""
    import torch
    from sad_amd import _lib, autograd, ops
    B, M3, K, sm, r_min, r_max, anchor = 2, 300, 257, 2.0, 1.0, 4.8, (3.9, 1.6, 1.56)
    c_np, g_np = dref.edge_case(B, K, sm, seed=1)
    c_np[..., 3:] = np.nan_to_num(c_np[..., 3:], nan=0.3, posinf=3.0, neginf=-3.0)
    rng = np.random.default_rng(2)
    xyz3 = _t(rng.standard_normal((B, M3, 3)).astype(np.float32), dev)
    c = _t(c_np, dev).requires_grad_(True)
    cand, radius = autograd.Candidates.apply(xyz3, c, K, sm, r_min, r_max, anchor)
    want_c, want_r = torch.empty((B, K, 3), device=dev), torch.empty((B, K), device=dev)
    _lib.check(_lib.lib().sad_candidates_f32(xyz3.data_ptr(), c.data_ptr(), B, M3, K, sm, r_min, r_max, (ctypes.c_float * 3)(*anchor),
                                             want_c.data_ptr(), want_r.data_ptr(), torch.cuda.current_stream().cuda_stream), "sad_candidates_f32")
    assert torch.equal(cand.detach().view(torch.int32), want_c.view(torch.int32)) and torch.equal(radius.view(torch.int32), want_r.view(torch.int32))
    assert cand.requires_grad and radius.requires_grad is False
    plain = ops.candidates(xyz3, c.detach(), K, sm, r_min, r_max, anchor)
    assert torch.equal(plain[0].view(torch.int32), want_c.view(torch.int32)) and not plain[0].requires_grad
    g = _t(g_np, dev)
    cand.backward(g)
    want = ops.candidates_grad(c.detach(), g, sm)
    assert torch.equal(c.grad.view(torch.int32), want.view(torch.int32))
    assert np.array_equal(_bits(_np(c.grad)), _bits(dref.candidates_grad_ref(c_np, g_np, sm)))


def _cluster_indices(cfg, xyz3, out):
    import torch
    from sad_amd import ops
    with torch.no_grad():
        idxs, cnts = ops.ball_query_multi(cfg.cluster_scales, cfg.cluster_nsamples, xyz3, out.cand.detach(), out.radius, return_counts=True)
    return [_np(i) for i in idxs], [_np(n) for n in cnts]


def _check_section(det, res, feat_grad=None, chains=("head", "cluster.agg", "cluster.b0", "cluster.b1", "cand")):
    mods = {"head": det.head, "cluster.agg": det.cluster_agg, "cand": det.cand}
    mods.update({f"cluster.b{k}": m for k, m in enumerate(det.cluster_branches)})
    for ch in chains:
        m = mods[ch]
        for l in range(len(m.weight)):
            assert m.weight[l].grad is not None and m.bias[l].grad is not None, ch
            dref.check(f"{ch} grad_W[{l}]", _np(m.weight[l].grad), res["grads"][f"{ch}.W{l}"])
            dref.check(f"{ch} grad_b[{l}]", _np(m.bias[l].grad), res["grads"][f"{ch}.b{l}"])
    if feat_grad is not None:
        dref.check("grad_feat3", _np(feat_grad), res["grads"]["feat3"])


def test_cluster_section_composed_bound(sad, dev, orc):
    """The small cluster section of detector_train_ref (K = 24 < M3 = 40, widths 33 / 10 / 40, S = 8 / 16, the candidate layer
    scaled so that shifts fall on both sides of the clamp): (o * w_o).sum() + (c * w_c).sum() backpropagated; every parameter
    of head, cluster.agg, cluster.b* and cand and the gradient arriving at feat3 within n 2^-23 A of the float64 composition on
    the module's indices, the reference's exact zeros exact, mismatch == 0."""
    import torch
    from sad_amd import autograd
    from sad_amd.detector_train import SADDetectorTrain
    cfg = dref.small_config()
    w = dref.small_weights(cfg)
    xyz3_np, feat3_np = dref.small_inputs(cfg)
    B, K = 2, cfg.n_cand
    det = SADDetectorTrain(cfg, dev, w)
    xyz3, feat3 = _t(xyz3_np, dev), _t(feat3_np, dev)
    with torch.no_grad():
        plain = det.cluster_head(xyz3, feat3)
    det.requires_grad_(True)
    feat3.requires_grad_(True)
    out = det.cluster_head(xyz3, feat3)
    for a, b in zip(out[:5], plain[:5]):
        assert torch.equal(a.detach(), b), "the training path's forward is not the no_grad path's"
    assert out.radius.requires_grad is False and out.cand.requires_grad and K < xyz3.shape[1]
    idxs, cnts = _cluster_indices(cfg, xyz3, out)
    # the populations this test is about, before anything is compared
    passes = dref.shift_passes(_np(out.c), cfg.shift_max)
    assert passes.any() and (~passes).any(), "clamped and unclamped shift components are both needed"
    assert any((n == 0).any() for n in cnts), "no empty cluster group"
    assert all(((n > 0) & (n < S)).any() for n, S in zip(cnts, cfg.cluster_nsamples)), "no partly filled cluster group"
    rng = np.random.default_rng(4)
    w_o = rng.standard_normal(tuple(out.o.shape)).astype(np.float32)
    w_c = rng.standard_normal(tuple(out.c.shape)).astype(np.float32)
    ((out.o * _t(w_o, dev)).sum() + (out.c * _t(w_c, dev)).sum()).backward()
    assert int(autograd.GroupedMLP.last_mismatch.item()) == 0
    res = dref.cluster_ref(orc, xyz3_np, feat3_np, w, K, cfg.shift_max, idxs, cnts, w_o, w_c)
    print(f"forward equals the oracle's bits: c {np.array_equal(res['c'], _np(out.c))}, cand {np.array_equal(res['cand'], _np(out.cand))}, "
          f"o {np.array_equal(res['o'], _np(out.o))}; unclamped {int(passes.sum())} of {passes.size}, empty groups {[int((n == 0).sum()) for n in cnts]}")
    assert np.array_equal(res["c"], _np(out.c)) and np.array_equal(res["cand"], _np(out.cand)), \
        "the reference decides the clamp and places the candidates on other bits than the module"
    assert (res["grads"]["cand_xyz"][1] > 0).any(), "no gradient reached cand: the path under test is empty"
    _check_section(det, res, feat3.grad)


def _tiny(dev, B=2):
    from sad_amd import config, synth
    cfg = config.TINY
    pts = _t(synth.make_tiny_batch(0, B, cfg.n_points), dev)
    gt = np.stack([synth.scene_boxes(i, cfg.n_points, extent=(0.0, 20.0, -10.0, 10.0), n_boxes=6) for i in range(B)], 0)
    return cfg, pts, _t(gt, dev), _t(np.zeros(gt.shape[:2], np.int32), dev)


def test_whole_detector_on_tiny(sad, dev, orc):
    """TINY, B = 2.  Under no_grad the boxes equal SADDetector's on the exported weights; the training forward's o, c, cand equal
    the no_grad ones; after loss(...).sum().backward() every parameter of every stage has a finite gradient; with the SA stages
    frozen their gradients stay None and the cluster section's lie within the composed bound of the float64 reference fed with
    the loss's own grad_o / grad_c (so do the unfrozen run's: the section's gradients do not depend on what lies in front)."""
    import torch
    from sad_amd import ops
    from sad_amd.detector import SADDetector
    from sad_amd.detector_train import SADDetectorTrain
    cfg, pts, gt_boxes, gt_labels = _tiny(dev)
    det = SADDetectorTrain(cfg, dev, seed=0)
    with torch.no_grad():
        plain = det(pts)
        boxes = det.decode(plain)
        want = SADDetector(cfg, det.export(), dev)(pts)
    tg = det.targets(plain, gt_boxes, gt_labels)
    assert int((tg.labels >= 0).sum(1).max()) > 0, "no positive point in any scene: the test would train nothing"
    assert torch.equal(boxes, want), "decode(forward()) differs from SADDetector on the exported weights"
    grads = {}
    for frozen in (False, True):
        det.requires_grad_(True)
        det.stages.requires_grad_(not frozen)
        det.zero_grad(set_to_none=True)
        out = det(pts)
        for name in ("o", "c", "cand"):
            assert torch.equal(getattr(out, name).detach(), getattr(plain, name)), f"{name}: the training forward differs from the no_grad one"
        targets = det.targets(out, gt_boxes, gt_labels)
        loss = det.loss(out, targets)
        assert tuple(loss.shape) == (2, 4) and int(det.num_pos.max()) > 0
        loss.sum().backward()
        for name, p in det.named_parameters():
            if frozen and name.startswith("stages."):
                assert p.grad is None, f"{name}: a frozen stage received a gradient"
            else:
                assert p.grad is not None and bool(torch.isfinite(p.grad).all()), f"{name}: no finite gradient"
        grads[frozen] = {n: p.grad.clone() for n, p in det.named_parameters() if p.grad is not None}
        if not frozen:
            # the float64 reference of the section, on the module's indices and the loss's own gradients
            lo = ops.point_head_loss(out.o.detach(), out.c.detach(), targets.labels, targets.centerness, targets.reg_target,
                                     targets.shift_target, targets.size_target, shift_max=cfg.shift_max)
            xyz3 = _xyz3(det, pts)
            assert torch.equal(xyz3[:, :cfg.n_cand], out.xyz_k)
            idxs, cnts = _cluster_indices(cfg, xyz3, out)
            res = dref.cluster_ref(orc, _np(xyz3), _np(out.feat3), det.export(), cfg.n_cand, cfg.shift_max, idxs, cnts,
                                   _np(lo[2]), _np(lo[3]))
            assert np.array_equal(res["c"], _np(out.c)) and np.array_equal(res["cand"], _np(out.cand))
        _check_section(det, res)
    moved = [n for n in grads[True] if not torch.equal(grads[True][n], grads[False][n])]
    print(f"gradients that differ in bits between the frozen and the unfrozen run (float atomics, SPEC.md §32): {moved}")


def _xyz3(det, pts):
    """SA3's centroids as the detector samples them (coordinates only)."""
    import torch
    from sad_amd import ops
    with torch.no_grad():
        xyz, _ = ops.split_points(pts)
        cur = ops.gather_xyz(xyz, ops.fps(xyz, det.stages[0].stage.npoint))
        for m in list(det.stages)[1:]:
            cur = ops.prefix_rows(cur, m.stage.npoint)
    return cur


SGD_LR, SGD_STEPS = 5e-5, 5


def test_descent_and_export(sad, dev):
    """Plain SGD on one fixed TINY batch: SGD_STEPS = 5 steps at SGD_LR = 5e-5 (p -= lr * grad on every parameter).  The summed
    loss after the last step is below the first step's.  The rate is the largest of a 1e-3 .. 5e-5 sweep at which the loss fell
    at every one of eight steps (39.28, 25.21, 19.76, 16.98, 15.53, 14.71, ...); at 1e-4 and above it still ends lower but not
    monotonically.  Afterwards SADDetector on the exported weights still reproduces
    decode(forward()) bit for bit (the parameters were written in place: the packed chains were rebuilt)."""
    import torch
    from sad_amd.detector import SADDetector
    from sad_amd.detector_train import SADDetectorTrain
    cfg, pts, gt_boxes, gt_labels = _tiny(dev)
    det = SADDetectorTrain(cfg, dev, seed=0)
    det.requires_grad_(True)
    traj = []
    for step in range(SGD_STEPS + 1):
        det.zero_grad(set_to_none=True)
        out = det(pts)
        loss = det.loss(out, det.targets(out, gt_boxes, gt_labels)).sum()
        traj.append(float(loss.detach()))
        if step == SGD_STEPS:
            break
        loss.backward()
        with torch.no_grad():
            for p in det.parameters():
                p -= SGD_LR * p.grad
    print("summed loss per step: " + ", ".join(f"{v:.5f}" for v in traj))
    assert all(np.isfinite(traj)) and traj[-1] < traj[0], traj
    with torch.no_grad():
        boxes = det.decode(det(pts))
        want = SADDetector(cfg, det.export(), dev)(pts)
    assert torch.equal(boxes, want), "after training, SADDetector on the exported weights differs from decode(forward())"


# ---- the SA stages' gradients (detector_train_ref.stack_ref): small_config, B = 2, 192 points ---------------------------------
def _stage_io(det, pts, out):
    """The stage loop of ``SADDetectorTrain.forward`` replayed under no_grad (split_points, FPS for stage 1, prefix_rows after
    that, ball_query_multi per stage) -> (the per-stage dicts ``stack_ref`` takes, the stages' outputs, xyz3).  Its last
    features are ``out.feat3`` of the training forward, bit for bit."""
    import torch
    from sad_amd import ops
    stages, outs = [], []
    with torch.no_grad():
        xyz, feat = ops.split_points(pts.contiguous())
        for s, m in enumerate(det.stages):
            st = m.stage
            new_xyz = ops.gather_xyz(xyz, ops.fps(xyz, st.npoint)) if s == 0 else ops.prefix_rows(xyz, st.npoint)
            idxs, cnts = ops.ball_query_multi(st.radii, st.nsamples, xyz, new_xyz, None, return_counts=True)
            stages.append(dict(xyz=_np(xyz), feat=None if feat is None else _np(feat), new_xyz=_np(new_xyz), idxs=[_np(i) for i in idxs],
                               cnts=[_np(n) for n in cnts]))
            got_xyz, nxt = m.forward_pm(xyz, feat, new_xyz)
            assert got_xyz is new_xyz
            outs.append(nxt)
            xyz, feat = new_xyz, nxt
    assert torch.equal(feat, out.feat3.detach()), "the replayed stage loop does not end in the training forward's feat3"
    return stages, outs, xyz


_CASES = {}


def _case(dev, orc, n_cand=24):
    """The small detector with ``n_cand`` candidates, its inputs and loss weights, and the float64 reference of its gradients on
    the module's own indices (``cluster_ref`` then ``stack_ref``), computed once per ``n_cand`` and shared, never written to.
    The reference does not depend on what is frozen."""
    import dataclasses
    import torch
    from sad_amd.detector_train import SADDetectorTrain
    if n_cand in _CASES:
        return _CASES[n_cand]
    cfg = dataclasses.replace(dref.small_config(), n_cand=n_cand)
    w = dref.small_weights(cfg)
    det = SADDetectorTrain(cfg, dev, w)
    pts = _t(dref.small_points(cfg), dev)
    with torch.no_grad():
        plain = det(pts)
    stages, outs, xyz3 = _stage_io(det, pts, plain)
    idxs, cnts = _cluster_indices(cfg, xyz3, plain)
    rng = np.random.default_rng([7, n_cand])
    w_o = rng.standard_normal(tuple(plain.o.shape)).astype(np.float32)
    w_c = rng.standard_normal(tuple(plain.c.shape)).astype(np.float32)
    cl = dref.cluster_ref(orc, _np(xyz3), _np(plain.feat3), w, n_cand, cfg.shift_max, idxs, cnts, w_o, w_c)
    st = dref.stack_ref(orc, stages, w, cl["grads"]["feat3"])
    _CASES[n_cand] = dict(cfg=cfg, w=w, det=det, pts=pts, plain=plain, stages=stages, outs=outs, cnts=cnts, w_o=_t(w_o, dev), w_c=_t(w_c, dev), cl=cl, st=st)
    return _CASES[n_cand]


def _backward(case, before=None):
    """One training forward and the backward of (o * w_o).sum() + (c * w_c).sum() -> the forward's output.  ``before``: called
    between the two."""
    out = case["det"](case["pts"])
    loss = (out.o * case["w_o"]).sum() + (out.c * case["w_c"]).sum()
    if before is not None:
        before()
    loss.backward()
    return out


def _entries(case):
    """[(chain, parameter, its (val, A, n) entry)] over every parameter of the detector, the SA stages first."""
    det, res = case["det"], []
    chains = [(f"sa{s}.{'agg' if k is None else f'b{k}'}", m.agg if k is None else m.branches[k], case["st"]["grads"])
              for s, m in enumerate(det.stages, 1) for k in list(range(len(m.branches))) + [None]]
    chains += [(n, m, case["cl"]["grads"]) for n, m in [("head", det.head), ("cluster.agg", det.cluster_agg), ("cand", det.cand)]
               + [(f"cluster.b{k}", m) for k, m in enumerate(det.cluster_branches)]]
    for name, m, grads in chains:
        for l in range(len(m.weight)):
            res += [(name, f"W{l}", m.weight[l], grads[f"{name}.W{l}"]), (name, f"b{l}", m.bias[l], grads[f"{name}.b{l}"])]
    assert len(res) == len(list(det.parameters()))
    return res


def _check_params(case, times=1):
    """Every parameter that requires grad within the bound of ``times`` x its reference entry (a sum of ``times`` computed
    gradients: val and A times ``times``, n times ``times`` plus ``times`` - 1), the others without a gradient -> the worst
    |err| / bound per chain."""
    worst = {}
    for chain, leaf, p, (val, A, n) in _entries(case):
        if not p.requires_grad:
            assert p.grad is None, f"{chain}.{leaf}: a frozen parameter received a gradient"
            continue
        assert p.grad is not None, f"{chain}.{leaf}: no gradient"
        val, A, n = np.asarray(val, np.float64) * times, np.asarray(A, np.float64) * times, n * times + times - 1
        got = _np(p.grad).astype(np.float64)
        ratio = np.abs(got - val)[A > 0] / (n * dref.ref.EPS * A[A > 0])
        worst[chain] = max(worst.get(chain, 0.0), float(ratio.max()) if ratio.size else 0.0)
        dref.check(f"{chain} grad_{leaf}", got, (val, A, n))
    return worst


@pytest.mark.parametrize("n_cand", [24, 40])
def test_sa_stack_composed_bound(sad, dev, orc, n_cand):
    """The whole small detector, everything trainable: every parameter of sa1 .. sa3 and of the cluster section within
    n 2^-23 A of the float64 composition (``cluster_ref``'s gradient at feat3 handed to ``stack_ref``) on the module's indices;
    n_cand = 40 == M3 makes ``PrefixRows`` the identity.  This is the composition the detector uses: centroids handed in
    (``forward_pm(new_xyz=prefix)``), a stage's input features another stage's output (``need`` "feat" + "params"; "params"
    only at sa1), every stage output's gradient the sum over its consumers, ``torch.cat``'s backward handing each branch its
    column slice.  Each stage's output equals the reference's forward bit for bit, so a failure is the backward's.

    How tight the composed bound is, measured on an MI355X against this reference.  Worst |err| / bound per chain of the
    correct build (n_cand = 24 / 40): head 1.7e-2 / 7.6e-3, cluster.agg 5.5e-3 / 3.5e-3, cand 1.6e-3 / 4.3e-4, cluster.b0
    1.4e-3 / 8.2e-4, cluster.b1 3.3e-4 / 3.4e-4, sa3.agg 1.1e-5 / 3.6e-6, sa3.b0 2.8e-6 / 2.0e-6, sa3.b1 1.7e-6 / 5.7e-7,
    sa2.agg 1.9e-7 / 5.9e-8, sa2.b0 2.4e-7 / 6.2e-8, sa2.b1 5.0e-8 / 5.2e-8, sa1.agg 3.1e-9 / 1.3e-9, sa1.b0 6.3e-10 / 2.5e-10,
    sa1.b1 3.4e-10 / 3.4e-10.  With ``MLPRows.backward``'s grad_x scaled by 1 + 2^-k in every chain, the test as a whole fails
    from k = 15 (at cluster.agg, right below the head), 2^-12 included; the SA stages' own entries first fail at k = 6 (sa3),
    k = 2 (sa2) and k = -2 (sa1: a factor of 5 per chain).  n adds up to 10^4 and A, a product of absolute values, outgrows
    |val| with every chain: at sa1 and sa2 this bound is wider than the gradient.  It still catches a lost consumer or a stopped
    gradient, through sa3 and the cluster section; what it cannot see at sa1 / sa2 is ``test_sa_stack_link_by_link``'s."""
    import torch
    from sad_amd import autograd
    case = _case(dev, orc, n_cand)
    cfg, det, cl, st = case["cfg"], case["det"], case["cl"], case["st"]
    assert (n_cand == cfg.stages[-1].npoint) == (n_cand == 40)
    for s, got in enumerate(case["outs"], 1):
        assert np.array_equal(st[f"out{s}"], _np(got)), f"sa{s}: the reference's forward is not the module's output"
    assert np.array_equal(cl["c"], _np(case["plain"].c)) and np.array_equal(cl["cand"], _np(case["plain"].cand))
    print(dref.stack_populations(orc, case["stages"], case["w"], cfg))
    det.requires_grad_(True)
    det.zero_grad(set_to_none=True)
    out = _backward(case)
    for name in ("o", "c", "cand", "feat3"):
        assert torch.equal(getattr(out, name).detach(), getattr(case["plain"], name)), f"{name}: the training forward differs from the no_grad one"
    assert int(autograd.GroupedMLP.last_mismatch.item()) == 0
    worst = _check_params(case)
    print(f"n_cand = {n_cand}: worst |err| / bound per chain: " + ", ".join(f"{k} {v:.3e}" for k, v in worst.items()))
    assert len(worst) == 14


def test_partial_freezing_passes_gradients_through(sad, dev, orc):
    """The same inputs, loss and reference with parts frozen: only sa1 trainable (every chain above passes grad_feat down with
    ``need == ("feat",)``); everything but sa2 (a frozen middle stage passes the gradient through); only sa2's first branch (a
    trainable branch beside a frozen one in a ``BranchGroup``, below frozen stages); only ``cand`` (no stage runs its autograd
    form).  Frozen parameters keep ``grad is None``, trainable ones lie within the bound of the unfrozen reference."""
    import torch
    case = _case(dev, orc)
    det = case["det"]
    settings = {"sa1 alone": lambda: det.stages[0].requires_grad_(True),
                "all but sa2": lambda: (det.requires_grad_(True), det.stages[1].requires_grad_(False)),
                "sa2.b0 alone": lambda: det.stages[1].branches[0].requires_grad_(True),
                "cand alone": lambda: det.cand.requires_grad_(True)}
    for name, select in settings.items():
        det.requires_grad_(False)
        det.zero_grad(set_to_none=True)
        select()
        out = _backward(case)
        worst = _check_params(case)
        print(f"{name}: worst |err| / bound per chain: " + ", ".join(f"{k} {v:.3e}" for k, v in worst.items()))
        assert len(worst) == {"sa1 alone": 3, "all but sa2": 11, "sa2.b0 alone": 1, "cand alone": 1}[name]
        if name == "cand alone":
            assert out.feat3.requires_grad is False
            for m, st in zip(det.stages, case["stages"]):
                got = m.forward_pm(_t(st["xyz"], dev), _t(st["feat"], dev), _t(st["new_xyz"], dev))[1]
                assert got.requires_grad is False, "a frozen stage below nothing trainable ran its autograd form"
        else:
            assert out.feat3.requires_grad
    det.requires_grad_(False)


def test_gradients_accumulate(sad, dev, orc):
    """Two forward / backward passes without zero_grad: every ``p.grad`` within the bound of twice the reference (2 val, 2 A,
    2 n + 1).  The first pass's gradients, cloned before the second pass, are what the second pass added to: ``p.grad`` lies
    within (n + 1) 2^-23 (|clone| + A) of clone + val (the second contribution is within n 2^-23 A of val, the addition rounds
    once), in the tensor it lived in before (same ``data_ptr``).  A backward that hands out a view of a buffer it writes again
    would change the first pass's gradient underneath; the second forward alone must leave them bit for bit."""
    import torch
    case = _case(dev, orc)
    det = case["det"]
    det.requires_grad_(True)
    det.zero_grad(set_to_none=True)
    _backward(case)
    _check_params(case)
    first = [(p.grad.clone(), p.grad.data_ptr()) for _, _, p, _ in _entries(case)]

    def untouched():
        for (chain, leaf, p, _), (clone, _) in zip(_entries(case), first):
            assert torch.equal(p.grad, clone), f"{chain}.{leaf}: the second forward changed the first pass's gradient underneath"
    _backward(case, before=untouched)
    worst = _check_params(case, times=2)
    print("two passes: worst |err| / bound per chain: " + ", ".join(f"{k} {v:.3e}" for k, v in worst.items()))
    for (chain, leaf, p, (val, A, n)), (clone, ptr) in zip(_entries(case), first):
        assert p.grad.data_ptr() == ptr, f"{chain}.{leaf}: the second pass replaced .grad instead of adding to it"
        one = _np(clone).astype(np.float64)
        dref.check(f"{chain} grad_{leaf} after the second pass", _np(p.grad), (one + val, np.abs(one) + A, n + 1))
    det.requires_grad_(False)
    det.zero_grad(set_to_none=True)


def _links(case, orc):
    """One training backward with every stage's output gradient retained, then every stage judged on its own: from G_s, the
    float32 gradient that ARRIVED at stage s's output (the sum over its consumers, as the module computed it), the one-stage
    ``stack_ref`` with A = |G_s| and n = 0 gives the stage's parameter gradients and the gradient it hands down, which is
    G_{s-1}.  -> [(name, got, (val, A, n))]: the stages' parameters, G_2 and G_1 as stage 3's and 2's grad_feat, and G_3 as
    ``cluster_ref``'s "feat3"."""
    det, kept = case["det"], []
    for m in det.stages:
        def forward_pm(xyz, feat_pm, new_xyz=None, _orig=m.forward_pm):
            res = _orig(xyz, feat_pm, new_xyz)
            res[1].retain_grad()
            kept.append(res[1])
            return res
        m.forward_pm = forward_pm
    try:
        out = _backward(case)
    finally:
        for m in det.stages:
            del m.forward_pm
    assert len(kept) == len(det.stages) and kept[-1] is out.feat3
    links = [("G3 = grad_feat3", _np(kept[-1].grad), case["cl"]["grads"]["feat3"])]
    for s in range(len(det.stages), 0, -1):
        m, G = det.stages[s - 1], _np(kept[s - 1].grad).astype(np.float64)
        w = {f"sa1.{k}": v for k, v in m.export().items()}
        local = dref.stack_ref(orc, [case["stages"][s - 1]], w, (G, np.abs(G), 0))["grads"]
        for k, chain in [(f"b{k}", b) for k, b in enumerate(m.branches)] + [("agg", m.agg)]:
            for l in range(len(chain.weight)):
                links.append((f"sa{s}.{k} grad_W{l} from G{s}", _np(chain.weight[l].grad), local[f"sa1.{k}.W{l}"]))
                links.append((f"sa{s}.{k} grad_b{l} from G{s}", _np(chain.bias[l].grad), local[f"sa1.{k}.b{l}"]))
        if s > 1:
            links.append((f"G{s - 1} from G{s}", _np(kept[s - 2].grad), local["feat1"]))
    return links


def test_sa_stack_link_by_link(sad, dev, orc):
    """The composed bound of ``test_sa_stack_composed_bound`` grows with every chain it passes (n adds up, A is a product of
    absolute values) until, at sa1 and sa2, it is wider than the gradient itself.  This test judges every link on its own, with
    the same bound and nothing composed: the gradient that arrives at a stage's output is taken from the module as float32
    data (A = its absolute value, n = 0), and the stage's parameter gradients and the gradient it hands to the stage below must
    lie within n 2^-23 A of the one-stage reference on it; the topmost arriving gradient is ``cluster_ref``'s.  If every link
    holds, the chain holds, and a lost consumer, a wrong slice or a scaled grad_x shows at the link where it happens at the
    tightness of the single-chain tests (n of a few thousand instead of 10^4, no A carried over).  Measured on an MI355X: worst
    |err| / bound of the correct build 1.4e-2 (sa3), 1.0e-2 (sa2), 4.8e-3 (sa1), 3.8e-4 / 2.5e-4 for the gradients handed down;
    grad_x scaled by 1 + 2^-k fails from k = 13 at sa3 and from k = 12 at sa2 and sa1."""
    case = _case(dev, orc)
    det = case["det"]
    det.requires_grad_(True)
    det.zero_grad(set_to_none=True)
    links = _links(case, orc)
    det.requires_grad_(False)
    det.zero_grad(set_to_none=True)
    assert len(links) == 1 + 3 * 10 + 2
    for name, got, entry in links:
        assert (np.asarray(entry[1]) > 0).any(), f"{name}: the reference's gradient is empty"
        dref.check(name, got, entry)
