"""GPU parity of the point head targets and loss (SPEC.md §31) (-m gpu): ops.point_targets, ops.point_head_loss,
autograd.PointHeadLoss, point_head.PointTargetAssigner / PointHeadLoss and SADDetector.head_targets against
tests/point_head_ref.py.  Parity rules of §31: labels, match, shift_target, size_target, reg_target[..., 0:3] and [..., 6],
num_pos and the regression / shift / size terms with their gradients are EQUAL to the float32 reference under ==; what passes
through cbrtf / logf / expf / log1pf (centerness, reg_target[..., 3:6], the classification terms, the class columns of grad_o) is
within §9's 1e-4 (absolute + relative) of the binary64 evaluation; loss[b, i] is within n 2^-23 sum|terms| of the binary64 sum of
the device's own per_point[b, :, i] (§21.4's rule, n = M).  Outputs are pre-filled with NaN / a sentinel before every call; a
second call is bit-identical; every case runs with normalize=False and in both cls_loss modes.  The coverage the cases rely on is
asserted on the reference in tests/test_point_head_cpu.py; nothing is skipped."""
import numpy as np
import pytest

import point_head_ref as ref

pytestmark = pytest.mark.gpu

F = np.float32
D = np.float64
SENTINEL = -77777


def _t(a, dev):
    import torch
    return None if a is None else torch.from_numpy(np.array(a, order="C")).to(dev)       # (a copy: the cases are read-only)


def _poison(spec, dev):
    import torch
    return tuple(torch.full(shape, float("nan") if dt == torch.float32 else SENTINEL, dtype=dt, device=dev) for _, shape, dt in spec)


def _written(got, what):
    for n, v in got.items():
        assert not (np.isnan(v).any() if v.dtype == F else (v == SENTINEL).any()), f"{what}: {n} not fully written"


def _equal(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    bad = ~(got == want)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {want.size} differ under ==, first at {np.argwhere(bad)[0].tolist()}"


def _near(got, want64, what):
    assert got.shape == want64.shape, (what, got.shape, want64.shape)
    err = np.abs(got.astype(D) - want64)
    tol = ref.tolerance(want64)
    print(f"{what}: worst error {float(err.max()):.3g}, worst share of the tolerance {float((err / tol).max()):.3g}")
    assert (err <= tol).all(), f"{what}: {int((err > tol).sum())} of {err.size} beyond the tolerance, worst {float(err.max()):.3g}"


def _same_bits(a, b, what):
    assert set(a) == set(b)
    for n in a:
        bad = int((a[n].view(np.int32) != b[n].view(np.int32)).sum())
        assert bad == 0, f"{what}: {bad} of {a[n].size} words of {n} differ"


def _run_targets(c, dev, cand=True):
    from sad_amd import ops
    B, M = c["xyz"].shape[:2]
    out = _poison(ops.point_output_spec(B, M), dev)
    got = ops.point_targets(_t(c["xyz"], dev), _t(c["cand"], dev) if cand else None, _t(c["gt_boxes"], dev), _t(c["gt_labels"], dev),
                            out=out, **c["tkw"])
    assert len(got) == 6 and all(g is o for g, o in zip(got, out))
    return {n: g.cpu().numpy() for n, g in zip(ref.TARGET_OUTPUTS, got)}


def _targets_parity(got, want, what):
    _written(got, what)
    for n in ("labels", "match", "shift_target", "size_target"):
        _equal(got[n], want[n], f"{what} {n}")
    _equal(got["reg_target"][..., :3], want["reg_target"][..., :3], f"{what} reg_target[..., 0:3]")
    _equal(got["reg_target"][..., 6], want["reg_target"][..., 6], f"{what} reg_target[..., 6]")
    _near(got["centerness"], want["centerness64"], f"{what} centerness")
    _near(got["reg_target"][..., 3:6], want["reg64"][..., 3:6], f"{what} reg_target[..., 3:6]")


@pytest.mark.parametrize("name", ref.CASES)
def test_point_targets_parity_and_determinism(dev, name):
    c = ref.case(name)
    got = _run_targets(c, dev)
    _targets_parity(got, ref.expected_targets(name), name)
    _same_bits(_run_targets(c, dev), got, f"{name}: second call")
    nonpos = got["labels"] < 0
    assert (got["match"][nonpos] == -1).all() and (got["centerness"][nonpos] == 0).all()
    assert all((got[n][nonpos] == 0).all() for n in ("shift_target", "size_target", "reg_target"))


def test_point_targets_without_candidates(dev):
    """cand = None: the centre-ness and reg_target[..., 0:3] are taken at xyz; the assignment does not move."""
    c = ref.case("m257")
    got = _run_targets(c, dev, cand=False)
    want = ref.targets(dict(c, cand=None))
    _targets_parity(got, want, "m257 without cand")
    _equal(got["labels"], ref.expected_targets("m257")["labels"], "labels with and without cand")


def _names(with_c):
    return [n for n in ("loss", "num_pos", "grad_o", "grad_c", "per_point") if with_c or n != "grad_c"]


def _run_loss(c, dev, with_c=True):
    from sad_amd import ops
    B, M, W = c["o"].shape
    out = _poison(ops.point_loss_output_spec(B, M, W - 7, with_c, True), dev)
    a = [_t(c[k], dev) for k in ref.LOSS_INPUTS]
    if not with_c:
        a[1] = a[5] = a[6] = None
    got = ops.point_head_loss(*a, per_point=True, out=out, **c["kw"])
    assert len(got) == len(out) and all(g is o for g, o in zip(got, out))
    return {n: g.cpu().numpy() for n, g in zip(_names(with_c), got)}


def _loss_parity(got, want, w64, what):
    _written(got, what)
    C = got["grad_o"].shape[2] - 7
    _equal(got["num_pos"], want["num_pos"], f"{what} num_pos")
    for i, n in ((1, "regression"), (2, "shift"), (3, "size")):
        _equal(got["per_point"][..., i], want["per_point"][..., i], f"{what} {n} terms")
    _equal(got["grad_o"][..., C:], want["grad_o"][..., C:], f"{what} grad_o, box columns")
    if "grad_c" in got:
        _equal(got["grad_c"], want["grad_c"], f"{what} grad_c")
    _near(got["per_point"][..., 0], w64["per_point"][..., 0], f"{what} classification terms")
    _near(got["grad_o"][..., :C], w64["grad_o"][..., :C], f"{what} grad_o, class columns")
    terms = got["per_point"].astype(D)
    bound = terms.shape[1] * 2.0 ** -23 * np.abs(terms).sum(1)
    err = np.abs(got["loss"].astype(D) - terms.sum(1))
    print(f"{what}: loss error {err.max():.3g}, bound {bound.max():.3g}")
    assert (err <= bound).all(), f"{what}: loss off its terms' sum by {err.tolist()}, bound {bound.tolist()}"


@pytest.mark.parametrize("cls_loss", ("bce", "focal"))
@pytest.mark.parametrize("name", ref.CASES)
def test_point_head_loss_parity_and_determinism(dev, name, cls_loss):
    c = ref.variant(ref.case(name), cls_loss=cls_loss)
    got = _run_loss(c, dev)
    e = ref.expected(name, True, cls_loss)
    _loss_parity(got, e["f32"], e["f64"], f"{name} {cls_loss}")
    _same_bits(_run_loss(c, dev), got, f"{name} {cls_loss}: second call")
    un = _run_loss(ref.variant(c, normalize=False), dev)
    e = ref.expected(name, False, cls_loss)
    _loss_parity(un, e["f32"], e["f64"], f"{name} {cls_loss} unnormalised")
    _equal(un["num_pos"], got["num_pos"], f"{name} num_pos, unnormalised")


def test_scene_without_positives(dev):
    """num_pos = 0: the loss is finite, the classification still counts, the box / shift / size terms and gradients are exactly 0."""
    got = _run_loss(ref.case("no_pos"), dev)
    C = got["grad_o"].shape[2] - 7
    assert got["num_pos"].tolist() == ref.expected("no_pos")["f32"]["num_pos"].tolist() and got["num_pos"][1] == 0
    assert np.isfinite(got["loss"]).all() and got["loss"][1, 0] > 0 and (got["loss"][1, 1:] == 0).all()
    assert (got["grad_o"][1, :, C:] == 0).all() and (got["grad_c"][1] == 0).all() and (got["per_point"][1, :, 1:] == 0).all()
    assert (got["grad_o"][1, :, :C] != 0).any()
    g0 = _run_loss(ref.case("g0"), dev)
    assert (g0["num_pos"] == 0).all() and np.isfinite(g0["loss"]).all() and (g0["loss"][:, 1:] == 0).all()


def test_without_c_and_without_centerness(dev):
    """c = None: the tuple is one shorter, loss[:, 2:] == 0, the other components and grad_o are those of the full call;
    only one of the two targets: the other half of grad_c is 0; centerness = None trains the hot channel against 1."""
    import torch
    from sad_amd import ops
    c = ref.case("m257")
    full, bare = _run_loss(c, dev), _run_loss(c, dev, with_c=False)
    assert "grad_c" not in bare and (bare["loss"][:, 2:] == 0).all() and (bare["per_point"][..., 2:] == 0).all()
    _equal(bare["loss"][:, :2], full["loss"][:, :2], "loss without c")
    _equal(bare["grad_o"], full["grad_o"], "grad_o without c")
    a = [_t(c[k], dev) for k in ref.LOSS_INPUTS]
    only_shift = ops.point_head_loss(*a[:6], None, **c["kw"])
    only_size = ops.point_head_loss(*a[:5], None, a[6], **{k: v for k, v in c["kw"].items() if k != "shift_max"})
    both = ops.point_head_loss(*a, **c["kw"])
    assert torch.equal(only_shift[3][..., :3], both[3][..., :3]) and (only_shift[3][..., 3:] == 0).all() and (only_shift[0][:, 3] == 0).all()
    assert torch.equal(only_size[3][..., 3:], both[3][..., 3:]) and (only_size[3][..., :3] == 0).all() and (only_size[0][:, 2] == 0).all()
    hard = dict(c, centerness=None)
    got = _run_loss(hard, dev)
    _loss_parity(got, ref.loss(hard), ref.loss(hard, D), "m257 without centerness")


def test_out_workspace_and_refusals_on_the_device(dev):
    import torch
    from sad_amd import ops
    c = ref.case("m70")
    B, M, W = c["o"].shape
    a = [_t(c[k], dev) for k in ref.LOSS_INPUTS]
    ws = ops.point_head_loss_workspace(B, M, dev)
    assert ws.numel() == 16 * B * ((M + 255) // 256)
    want = ops.point_head_loss(*a, **c["kw"])
    got = ops.point_head_loss(*a, workspace=ws, **c["kw"])
    assert all(torch.equal(g, w) for g, w in zip(got, want))
    spec = ops.point_loss_output_spec(B, M, W - 7, True, False)
    for bad in (_poison(spec[:-1], dev), _poison(ops.point_loss_output_spec(B, M + 1, W - 7, True, False), dev),
                _poison(ops.point_loss_output_spec(B, M, W - 7, True, True), dev), tuple(t.cpu() for t in _poison(spec, dev))):
        with pytest.raises(ValueError, match="out"):
            ops.point_head_loss(*a, out=bad, **c["kw"])
    with pytest.raises(ValueError, match="workspace"):
        ops.point_head_loss(*a, workspace=ws[:-1], **c["kw"])
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.point_head_loss(a[0], a[1].cpu(), *a[2:], **c["kw"])
    with pytest.raises(ValueError, match="out"):
        ops.point_targets(_t(c["xyz"], dev), None, _t(c["gt_boxes"], dev), _t(c["gt_labels"], dev),
                          out=_poison(ops.point_output_spec(B, M)[:-1], dev), **c["tkw"])


def test_autograd(dev):
    """A non-uniform grad_loss [B,4]: the gradients of o and c are the saved gradients times the weights of their component, bit
    for bit; the targets get none."""
    import torch
    from sad_amd import autograd, ops
    c = ref.case("m257")
    a = [_t(c[k], dev) for k in ref.LOSS_INPUTS]
    C = a[0].shape[2] - 7
    want = ops.point_head_loss(*a, **c["kw"])
    up = torch.tensor([[0.5, -2.0, 3.0, 0.25], [1.25, 0.0, -1.0, 2.0], [-0.75, 4.0, 0.125, -3.0]], device=dev)
    for with_c in (True, False):
        o, cc = a[0].clone().requires_grad_(), a[1].clone().requires_grad_()
        tg = [t.clone().requires_grad_() if t.dtype == torch.float32 else t for t in a[2:]]
        if not with_c:
            tg[3] = tg[4] = None
        loss, num = autograd.PointHeadLoss.apply(o, cc if with_c else None, *tg, c["kw"])
        assert loss.requires_grad and not num.requires_grad and torch.equal(num, want[1])
        assert torch.equal(loss[:, :2], want[0][:, :2]) and (torch.equal(loss, want[0]) if with_c else (loss[:, 2:] == 0).all())
        (loss * up).sum().backward()
        assert torch.equal(o.grad[..., :C], want[2][..., :C] * up[:, 0].view(-1, 1, 1))
        assert torch.equal(o.grad[..., C:], want[2][..., C:] * up[:, 1].view(-1, 1, 1))
        if with_c:
            assert torch.equal(cc.grad[..., :3], want[3][..., :3] * up[:, 2].view(-1, 1, 1))
            assert torch.equal(cc.grad[..., 3:], want[3][..., 3:] * up[:, 3].view(-1, 1, 1))
        else:
            assert cc.grad is None
        assert all(t is None or t.grad is None for t in tg)


def test_round_trip_through_the_decode(dev):
    """reg_target placed in o with the class logit of the label set: sad_decode_boxes_f32 (§9) gives back the ground-truth box of
    every positive whose size code was not clamped, within the 1e-4 rule."""
    import ctypes
    import torch
    from sad_amd import _lib
    c = ref.case("m257")
    got = _run_targets(c, dev)
    B, M = got["labels"].shape
    pos = got["labels"] >= 0
    o = np.zeros((B, M, 10), F)
    o[..., 3:] = got["reg_target"]
    o[..., :3] = -5.0
    np.put_along_axis(o[..., :3], np.clip(got["labels"], 0, 2)[..., None], 5.0, -1)
    cand, ot = _t(c["cand"], dev), _t(o, dev)
    boxes = torch.full((B, M, 9), float("nan"), device=dev)
    anchors = (ctypes.c_float * 9)(*[v for a in ref.ANCHORS for v in a])
    _lib.check(_lib.lib().sad_decode_boxes_f32(cand.data_ptr(), ot.data_ptr(), B, M, anchors, boxes.data_ptr(),
                                               torch.cuda.current_stream().cuda_stream), "sad_decode_boxes_f32")
    bx = boxes.cpu().numpy()
    gt = np.take_along_axis(c["gt_boxes"][..., :7], np.clip(got["match"], 0, None)[..., None], 1)
    free = pos & (np.abs(got["reg_target"][..., 3:6]) < 2).all(-1)
    assert free.sum() > 100 and (bx[..., 8][pos] == got["labels"][pos]).all()
    _near(bx[free][:, :7], gt[free].astype(D), "decoded boxes")


def test_modules_behind_linear_heads(dev):
    """PointTargetAssigner -> two small linear heads on the device -> assigner.loss() -> backward: the weight gradients are finite
    and are those of the operator's grad_o / grad_c fed through the same layers by hand; num_pos is kept."""
    import torch
    from sad_amd import ops, point_head
    c = ref.case("m257")
    assigner = point_head.PointTargetAssigner(**c["tkw"])
    tg = assigner(_t(c["xyz"], dev), _t(c["cand"], dev), _t(c["gt_boxes"], dev), _t(c["gt_labels"], dev))
    B, M = tg.labels.shape
    torch.manual_seed(7)
    feat = (torch.randn(B * M, 16) * 0.5).to(dev)
    head, cl = torch.nn.Linear(16, 10).to(dev), torch.nn.Linear(16, 6).to(dev)
    mod = assigner.loss(code_weights=[1.0, 1.0, 1.0, 0.7, 0.7, 0.7, 1.3], reg_weight=2.0, shift_weight=0.5, size_weight=0.25)
    assert isinstance(mod, point_head.PointHeadLoss) and mod.num_pos is None
    loss = mod(head(feat), cl(feat), tg)                                   # [B*M,10] and [B*M,6]: views, never copied
    assert loss.shape == (B, 4) and loss.requires_grad
    loss.sum().backward()
    params = (*head.parameters(), *cl.parameters())
    mine = [p.grad.clone() for p in params]
    assert all(torch.isfinite(g).all() for g in mine) and all((g != 0).any() for g in mine)
    with torch.no_grad():
        o, cc = head(feat).view(B, M, 10), cl(feat).view(B, M, 6)
    want = ops.point_head_loss(o, cc, tg.labels, tg.centerness, tg.reg_target, tg.shift_target, tg.size_target, **mod.cfg)
    assert torch.equal(loss.detach(), want[0]) and torch.equal(mod.num_pos, want[1]) and int(mod.num_pos.sum()) > 0
    for p in params:
        p.grad = None
    head(feat).backward(want[2].view(B * M, 10))
    cl(feat).backward(want[3].view(B * M, 6))
    for g, p in zip(mine, params):
        assert torch.allclose(g, p.grad, rtol=1e-5, atol=1e-6), float((g - p.grad).abs().max())
    bare = mod(o, None, tg)
    assert torch.equal(bare[:, :2], want[0][:, :2]) and (bare[:, 2:] == 0).all()


def test_detector_head_targets_and_loss(sad, dev):
    """TINY detector, forward(trace=...) -> head_targets -> PointHeadLoss on trace["cluster"]: equal to the reference evaluated on
    the trace tensors copied to the host.  The ground truth is built around the detector's own SA3 points, so some are positive."""
    import torch
    from sad_amd import config, point_head, synth
    from sad_amd.detector import SADDetector
    cfg = config.TINY
    det = SADDetector(cfg, synth.make_weights(cfg, 0), dev)
    pts = _t(synth.make_tiny_batch(0, 2, cfg.n_points), dev)
    trace = {}
    det(pts, trace=trace)
    K = cfg.n_cand
    xyz = trace["sa3"]["new_xyz"][:, :K].contiguous()
    cand, cc, o = (trace["cluster"][k] for k in ("cand", "c", "head"))
    assert tuple(o.shape) == (2, K, 10) and tuple(cc.shape) == (2, K, 6)
    hx = xyz.cpu().numpy()
    B, G = 2, 6
    gt, gl = np.zeros((B, G, 7), F), np.zeros((B, G), np.int32)
    for b in range(B):
        for g in range(G):
            gt[b, g] = (*(hx[b, 5 * g] + F(0.125)), 3.9, 1.6, 1.56, 0.3 * g)
            gl[b, g] = g % 3 if g != 2 else -1
    tg = det.head_targets(trace, _t(gt, dev), _t(gl, dev))
    case = dict(xyz=hx, cand=cand.cpu().numpy(), gt_boxes=gt, gt_labels=gl,
                tkw=dict(anchors=cfg.anchors, size_anchor=cfg.anchor_car, shift_max=cfg.shift_max, extra_width=0.2))
    want = ref.targets(case)
    got = {n: t.cpu().numpy() for n, t in zip(ref.TARGET_OUTPUTS, tg)}
    _targets_parity(got, want, "detector targets")
    assert (got["labels"] >= 0).sum() >= 2 * (G - 1)
    mod = point_head.PointTargetAssigner.from_config(cfg).loss(reg_weight=2.0)
    o1, c1 = o.clone().requires_grad_(), cc.clone().requires_grad_()
    loss = mod(o1, c1, tg)
    loss.sum().backward()
    fed = dict(case, o=o.cpu().numpy(), c=cc.cpu().numpy(), kw=dict(mod.cfg), **{n: got[n] for n in ref.TARGET_OUTPUTS})
    w32, w64 = ref.loss(fed), ref.loss(fed, D)
    _equal(mod.num_pos.cpu().numpy(), w32["num_pos"], "detector num_pos")
    _equal(o1.grad.cpu().numpy()[..., 3:], w32["grad_o"][..., 3:], "detector grad_o, box columns")
    _equal(c1.grad.cpu().numpy(), w32["grad_c"], "detector grad_c")
    _near(o1.grad.cpu().numpy()[..., :3], w64["grad_o"][..., :3], "detector grad_o, class columns")
    _near(loss.detach().cpu().numpy(), w64["loss64"], "detector loss")
