"""The candidate layer's backward and ``SADDetectorTrain`` on the GPU (SPEC.md §33).

``ops.candidates_grad`` / ``ops.prefix_rows_grad`` are selections and copies: compared with the numpy reference of
tests/detector_train_ref.py bit for bit.  The cluster section and the whole detector are compared with the float64 composition
``detector_train_ref.cluster_ref`` on the indices the module used, every parameter within n * 2^-23 * A (mlp_grad_ref's bound,
n and A added up along the composition), and with ``SADDetector`` on the exported weights under ``torch.equal``."""
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
