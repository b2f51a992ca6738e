"""GPU parity of the RoI head loss (SPEC.md §29) (-m gpu): ops.roi_head_loss, autograd.RoIHeadLoss, roi_head.RoIHeadLoss and
ProposalTargetLayer.loss against tests/roi_loss_ref.py.  Parity rules of §29: num is exact; the regression terms and grad_reg
are EQUAL to the float32 reference under ==; what passes through expf / log1pf (the classification terms, grad_cls, the corner
terms) is within §9's 1e-4 (absolute + relative) of the binary64 evaluation, grad_corner within 1e-4 + 1e-4 mag, mag the sum
of the magnitudes of the element's eight addends; loss[b, i] is within n 2^-23 sum|terms| of the binary64 sum of the device's own
per_roi[b, :, i] (§21.4's rule).  Outputs are pre-filled with NaN / a sentinel before every call; a second call is bit-identical;
every case runs a second time with normalize=False.  The coverage the cases rely on, and that no row sits within the margin of
the flip or of the Huber kink, is asserted on the reference in tests/test_roi_loss_cpu.py; nothing is skipped."""
import numpy as np
import pytest

import roi_head_ref
import roi_loss_ref as ref

pytestmark = pytest.mark.gpu

F = np.float32
D = np.float64
SENTINEL = -77777
NAMES = ("loss", "num", "grad_cls", "grad_reg", "grad_corner", "per_roi")


def _t(a, dev):
    import torch
    return None if a is None else torch.from_numpy(np.array(a, order="C")).to(dev)       # (a copy: the cases are read-only)


def _poison(B, S, corner, dev, per_roi=True):
    import torch
    from sad_amd import ops
    return tuple(torch.full(shape, float("nan") if dt == torch.float32 else SENTINEL, dtype=dt, device=dev)
                 for _, shape, dt in ops.roi_loss_output_spec(B, S, corner, per_roi))


def _run(c, dev):
    """One call into poisoned outputs -> {name: numpy}."""
    from sad_amd import ops
    corner = c["rois"] is not None
    out = _poison(*c["rcnn_cls"].shape, corner, dev)
    got = ops.roi_head_loss(*[_t(c[k], dev) for k in ref.INPUTS], per_roi=True, out=out, **c["kw"])
    assert len(got) == len(out) == (6 if corner else 5) and all(g is o for g, o in zip(got, out))
    return {n: g.cpu().numpy() for n, g in zip([n for n in NAMES if corner or n != "grad_corner"], got)}


def _equal(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    bad = ~(got == want)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {want.size} differ under ==, first at {np.argwhere(bad)[0].tolist()}"


def _near(got, want64, what, scale=None):
    assert got.shape == want64.shape, (what, got.shape, want64.shape)
    err = np.abs(got.astype(D) - want64)
    ok = err <= ref.tolerance(want64, scale)
    print(f"{what}: worst error {float(err.max()):.3g}, worst share of the tolerance {float((err / ref.tolerance(want64, scale)).max()):.3g}")
    assert ok.all(), f"{what}: {int((~ok).sum())} of {ok.size} beyond the tolerance, worst {float(err.max()):.3g}"


def _same_bits(a, b, what):
    assert set(a) == set(b)
    for n in a:
        bad = int((a[n].view(np.int32) != b[n].view(np.int32)).sum())
        assert bad == 0, f"{what}: {bad} of {a[n].size} words of {n} differ"


def _parity(got, want, w64, what):
    for n, v in got.items():
        assert not (np.isnan(v).any() if v.dtype == F else (v == SENTINEL).any()), f"{what}: {n} not fully written"
    _equal(got["num"], want["num"], f"{what} num")
    _equal(got["per_roi"][..., 1], want["per_roi"][..., 1], f"{what} regression terms")
    _equal(got["grad_reg"], want["grad_reg"], f"{what} grad_reg")
    _near(got["per_roi"][..., 0], w64["per_roi"][..., 0], f"{what} classification terms")
    _near(got["grad_cls"], w64["grad_cls"], f"{what} grad_cls")
    assert ("grad_corner" in got) == ("grad_corner" in want)
    if "grad_corner" in got:
        _near(got["per_roi"][..., 2], w64["per_roi"][..., 2], f"{what} corner terms")
        _near(got["grad_corner"], w64["grad_corner"], f"{what} grad_corner", w64["mag"])
    else:
        assert (got["per_roi"][..., 2] == 0).all() and (got["loss"][:, 2] == 0).all()
    # the reduction on its own: against the binary64 sum of the device's own terms, §21.4's rule
    terms = got["per_roi"].astype(D)
    bound = terms.shape[1] * 2.0 ** -23 * np.abs(terms).sum(1)
    err = np.abs(got["loss"].astype(D) - terms.sum(1))
    print(f"{what}: loss error {err.max():.3g}, bound {bound.max():.3g}")
    assert (err <= bound).all(), f"{what}: loss off its terms' sum by {err.tolist()}, bound {bound.tolist()}"


@pytest.mark.parametrize("name", ref.CASES)
def test_roi_head_loss_parity_and_determinism(dev, name):
    c = ref.case(name)
    got = _run(c, dev)
    _parity(got, ref.expected(name)["f32"], ref.expected(name)["f64"], name)
    _same_bits(_run(c, dev), got, f"{name}: second call")
    # normalize=False: wq_i = scale_i, no output is scaled down towards the absolute part of the tolerance
    un = _run(ref.unnormalised(c), dev)
    _parity(un, ref.expected(name, False)["f32"], ref.expected(name, False)["f64"], f"{name} unnormalised")
    _equal(un["num"], got["num"], f"{name} num, unnormalised")


def test_coincident_boxes_give_exactly_zero(dev):
    """rcnn_reg = 0 on gt_local = (0, 0, 0, la, wa, ha, 0): every corner distance is 0, the corner term and its gradient are 0 under
    == (never 0 / 0) and nothing is NaN."""
    got = _run(ref.case("coincident"), dev)
    assert (got["per_roi"][..., 2] == 0).all() and (got["grad_corner"] == 0).all() and (got["loss"][:, 2] == 0).all()
    assert not any(np.isnan(v).any() for v in got.values())
    assert (got["per_roi"][..., 1] > 0).any()


def test_without_the_corner_component(dev):
    """rois = gt_local = None: the tuple is one shorter, loss[:, 2] == 0, the other two components are those of the full call."""
    import torch
    from sad_amd import ops
    c = ref.case("both")
    a = [_t(c[k], dev) for k in ref.INPUTS]
    full = ops.roi_head_loss(*a, **c["kw"])
    bare = ops.roi_head_loss(*a[:5], **c["kw"])
    assert len(full) == 5 and len(bare) == 4
    assert torch.equal(bare[0][:, :2], full[0][:, :2]) and (bare[0][:, 2] == 0).all()
    assert all(torch.equal(x, y) for x, y in zip(bare[1:], full[1:4]))
    assert len(ops.roi_head_loss(*a[:5], per_roi=True, **c["kw"])) == 5


def test_out_is_honoured_and_checked(dev):
    import torch
    from sad_amd import ops
    c = ref.case("both")
    B, S = c["rcnn_cls"].shape
    a = [_t(c[k], dev) for k in ref.INPUTS]
    out = _poison(B, S, True, dev, per_roi=False)
    got = ops.roi_head_loss(*a, out=out, **c["kw"])
    assert all(g is o for g, o in zip(got, out)) and all(torch.equal(g, w) for g, w in zip(got, ops.roi_head_loss(*a, **c["kw"])))
    for bad in (out[:-1], _poison(B, S + 1, True, dev, per_roi=False), _poison(B, S, True, dev), _poison(B, S, False, dev, per_roi=False),
                tuple(t.double() if t.dtype == torch.float32 else t for t in out), tuple(t.cpu() for t in out)):
        with pytest.raises(ValueError, match="out"):
            ops.roi_head_loss(*a, out=bad, **c["kw"])
    with pytest.raises(ValueError, match="together"):
        ops.roi_head_loss(*a[:6], **c["kw"])
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.roi_head_loss(a[0], a[1].cpu(), *a[2:], **c["kw"])


def test_autograd(dev):
    """A non-uniform grad_loss [B,3]: the gradients of the predictions are the saved gradients times the weights, bit for bit;
    the targets get none."""
    import torch
    from sad_amd import autograd, ops
    c = ref.case("ragged")
    a = [_t(c[k], dev) for k in ref.INPUTS]
    want = ops.roi_head_loss(*a, **c["kw"])
    up = torch.tensor([[0.5, -2.0, 3.0], [1.25, 0.0, -1.0], [-0.75, 4.0, 0.125]], device=dev)
    for corner in (True, False):
        x, r = a[0].clone().requires_grad_(), a[1].clone().requires_grad_()
        tg = [t.clone().requires_grad_() if t.dtype == torch.float32 else t for t in a[2:]]
        if not corner:
            tg[3] = tg[4] = None
        loss, num = autograd.RoIHeadLoss.apply(x, r, *tg, c["kw"])
        assert loss.requires_grad and not num.requires_grad and torch.equal(num, want[1])
        assert torch.equal(loss[:, :2], want[0][:, :2]) and (torch.equal(loss, want[0]) if corner else (loss[:, 2] == 0).all())
        (loss * up).sum().backward()
        assert torch.equal(x.grad, want[2] * up[:, 0].view(-1, 1))
        greg = want[3] * up[:, 1].view(-1, 1, 1)
        assert torch.equal(r.grad, greg + want[4] * up[:, 2].view(-1, 1, 1) if corner else greg)
        assert all(t is None or t.grad is None for t in tg)


def test_module_behind_a_linear_head(dev):
    """ProposalTargetLayer -> a small linear head on the device -> layer.loss() -> backward: the weight gradients are finite and
    are those of the operator's grad_* fed through the same layers by hand (up to the order of the GEMM's additions); num is kept."""
    import torch
    from sad_amd import ops, roi_head
    c = roi_head_ref.case("both")
    rois, gt, gl = _t(c["rois"], dev), _t(c["gt_boxes"], dev), _t(c["gt_labels"], dev)
    layer = roi_head.ProposalTargetLayer(roi_per_image=48, by_class=False, seed=5)
    tg = layer(rois, None, gt, gl)
    B, S = tg.cls_target.shape
    torch.manual_seed(7)
    feat = (torch.randn(B * S, 16) * 0.5).to(dev)
    cls_head, reg_head = torch.nn.Linear(16, 1).to(dev), torch.nn.Linear(16, 7).to(dev)
    mod = layer.loss(beta=1.0 / 9.0, code_weights=[1.0, 1.0, 1.0, 0.7, 0.7, 0.7, 1.3], cls_weight=1.0, reg_weight=2.0, corner_weight=0.5)
    assert isinstance(mod, roi_head.RoIHeadLoss) and mod.num is None
    loss = mod(cls_head(feat), reg_head(feat), tg)                        # [B*S,1] and [B*S,7]: views, never copied
    assert loss.shape == (B, 3) and loss.requires_grad
    loss.sum().backward()
    mine = [p.grad.clone() for p in (*cls_head.parameters(), *reg_head.parameters())]
    assert all(torch.isfinite(g).all() for g in mine) and all((g != 0).any() for g in mine)
    with torch.no_grad():
        x, r = cls_head(feat).view(B, S), reg_head(feat).view(B, S, 7)
    want = ops.roi_head_loss(x, r, tg.cls_target, tg.reg_valid, tg.reg_target, tg.rois_s, tg.gt_local, **mod.cfg)
    assert torch.equal(loss.detach(), want[0]) and torch.equal(mod.num, want[1]) and int(mod.num[:, 1].sum()) > 0
    for p in (*cls_head.parameters(), *reg_head.parameters()):
        p.grad = None
    cls_head(feat).backward(want[2].view(B * S, 1))
    reg_head(feat).backward((want[3] + want[4]).view(B * S, 7))
    for g, p in zip(mine, (*cls_head.parameters(), *reg_head.parameters())):
        assert torch.allclose(g, p.grad, rtol=1e-5, atol=1e-6), float((g - p.grad).abs().max())
    # the other accepted shapes give the same loss; without the corner component the module's loss[:, 2] is 0
    assert torch.equal(mod(x.view(B, S, 1), r.view(B * S, 7), tg), want[0])
    bare = roi_head.RoIHeadLoss(corner=False, **{k: v for k, v in zip(("cls_weight", "reg_weight", "corner_weight"), mod.cfg["scale"])},
                                beta=mod.cfg["beta"], code_weights=mod.cfg["code_weights"])(x, r, tg)
    assert torch.equal(bare[:, :2], want[0][:, :2]) and (bare[:, 2] == 0).all()


def test_chained_behind_roi_targets(dev):
    """The device's own roi_targets outputs go straight into roi_head_loss, nothing synchronised in between; the result against
    the reference fed the same arrays.  (rois_s and gt_local equal the reference's under ==, so the predictions of the case
    `both`, drawn around the reference's targets, keep their margins.)"""
    from sad_amd import ops
    tc, c = roi_head_ref.case("both"), ref.case("both")
    tg = ops.roi_targets(*[_t(tc[k], dev) for k in ("rois", "roi_count", "roi_labels", "gt_boxes", "gt_labels")], **tc["kw"])
    tg = dict(zip(roi_head_ref.OUTPUTS, tg))
    B, S = tg["cls_target"].shape
    out = _poison(B, S, True, dev)
    got = ops.roi_head_loss(_t(c["rcnn_cls"], dev), _t(c["rcnn_reg"], dev), tg["cls_target"], tg["reg_valid"], tg["reg_target"], tg["rois_s"],
                            tg["gt_local"], per_roi=True, out=out, **c["kw"])
    got = {n: g.cpu().numpy() for n, g in zip(NAMES, got)}                # (the first read-back)
    fed = dict(c, cls_target=tg["cls_target"].cpu().numpy(), reg_valid=tg["reg_valid"].cpu().numpy(), reg_target=tg["reg_target"].cpu().numpy(),
               rois=tg["rois_s"].cpu().numpy(), gt_local=tg["gt_local"].cpu().numpy())
    valid = fed["reg_valid"] != 0
    assert valid.any() and np.array_equal(fed["rois"][valid], c["rois"][valid]) and np.array_equal(fed["gt_local"][valid], c["gt_local"][valid])
    _parity(got, ref.loss_vec(fed), ref.loss_vec(fed, D), "chained")
