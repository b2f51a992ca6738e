"""GPU checks of the rotated IoU loss (SPEC.md §34): the kernel against the float32 reference under `==` wherever no library
function is involved, against `boxes_iou`'s diagonal, under exact translations, with weights, in the RoI code, and through
autograd and the modules.  Every output buffer is pre-filled with NaN, and every call is made twice: the second is bit-equal."""
import functools

import numpy as np
import pytest

import box_truth as bt
import iou_loss_ref as ref
import iou_loss_truth as truth

pytestmark = pytest.mark.gpu
F = np.float32
SIZES = sorted(bt.SIZE_FAMILIES)
NAN = float("nan")


@pytest.fixture(autouse=True)
def _oracle(orc):
    return orc


def _t(x, dev):
    import torch
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(dev)


def _widen(rows, D, fill=NAN):
    """[...,7] -> [...,D]: the columns beyond the seventh hold NaN (they are never read)."""
    rows = np.asarray(rows, F)
    return rows if D == 7 else np.concatenate([rows, np.full(rows.shape[:-1] + (D - 7,), fill, F)], -1)


def _call(dev, pred, target, weight=None, **kw):
    """ops.rotated_iou_loss into NaN-filled buffers, twice -> numpy results of the first call."""
    import torch
    from sad_amd import ops
    lead = pred.shape[:-1]
    spec = ops.rotated_iou_loss_output_spec(lead, kw.get("need_grad", True), kw.get("decoded", False))
    args = (_t(pred, dev), _t(target, dev), _t(weight, dev))
    kw = dict(kw, rois=_t(kw.get("rois"), dev))
    runs = []
    for _ in range(2):
        out = tuple(torch.full(shape, NAN, dtype=dt, device=dev) for _, shape, dt in spec)
        got = ops.rotated_iou_loss(*args, out=out, **kw)
        assert all(g is o for g, o in zip(got, out))
        runs.append([g.cpu().numpy() for g in got])
    for x, y in zip(*runs):
        np.testing.assert_array_equal(x.view(np.int32), y.view(np.int32), err_msg="a second call differs")
    return runs[0]


def _same(got, want, what):
    for name, g, w in zip(("loss", "iou", "grad"), got, want):
        assert not np.isnan(g).any(), f"{what}: {name} holds NaN (an element was not written)"
        np.testing.assert_array_equal(g, w.reshape(g.shape), err_msg=f"{what}: {name}")


# ---- 1: the float32 reference under == -------------------------------------------------------------------------------
@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("family", bt.PAIR_FAMILIES)
def test_equals_the_reference(sad, dev, family, size):
    a, b = bt.pair_family(family, size, 257, seed=2)
    for mode in ref.MODES:
        for kind in ref.KINDS:
            _same(_call(dev, a, b, mode=mode, kind=kind), ref.rotated_iou_loss(a, b, None, mode, kind)[:3], f"{family} {size} {mode} {kind}")


@functools.lru_cache(maxsize=None)
def _mixed(mode, kind):
    """1000 pairs whose index walks through the pair families, both size families: rows, weights and the reference."""
    a, b = bt.matrix_boxes(1000, 1000, seed=7)
    wt = np.random.default_rng(8).uniform(0.25, 4.0, 1000).astype(F)
    return a, b, wt, ref.rotated_iou_loss(a, b, wt, mode, kind)[:3]


@pytest.mark.parametrize("N", [1, 63, 64, 65, 255, 256, 257, 1000])
def test_wave_and_workgroup_edges(sad, dev, N):
    """N at the wave and workgroup edges; Dp and Dt each 7 or 9, chosen independently; leading shape [N] or [B,S]."""
    lead = {64: (2, 32), 256: (4, 64), 1000: (8, 125)}.get(N, (N,))
    for q, (Dp, Dt) in enumerate(((7, 7), (9, 7), (7, 9), (9, 9))):
        mode, kind = (("3d", "diou"), ("bev", "iou"), ("3d", "iou"), ("bev", "diou"))[(q + N) % 4]
        a, b, wt, want = _mixed(mode, kind)
        got = _call(dev, _widen(a[:N], Dp).reshape(lead + (Dp,)), _widen(b[:N], Dt).reshape(lead + (Dt,)), wt[:N].reshape(lead), mode=mode, kind=kind)
        assert got[0].shape == lead and got[2].shape == lead + (7,)
        _same(got, [w[:N] for w in want], f"N={N} Dp={Dp} Dt={Dt} {mode} {kind}")


# ---- 2: boxes_iou's diagonal -----------------------------------------------------------------------------------------
def test_iou_is_the_diagonal_of_boxes_iou(sad, dev):
    from sad_amd import ops
    a, b = bt.matrix_boxes(257, 257, seed=9)
    ta, tb = _t(a, dev), _t(b, dev)
    for mode, fn in (("bev", ops.boxes_iou_bev), ("3d", ops.boxes_iou3d)):
        want = fn(ta, tb).diagonal().cpu().numpy()
        np.testing.assert_array_equal(ops.boxes_iou_aligned(ta, tb, mode).cpu().numpy(), want, err_msg=mode)
        np.testing.assert_array_equal(_call(dev, a, b, mode=mode, kind="diou")[1], want, err_msg=mode)
    assert (want > 0.5).sum() >= 20 and (want == 0).sum() >= 20


# ---- 3: translation --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family,size", [("perturbed", "object"), ("nested", "thin"), ("edge", "object"), ("far", "thin")])
def test_exact_translation_keeps_every_bit(sad, dev, family, size):
    a, b = bt.pair_family(family, size, 257, seed=10)
    for mode, kind in (("3d", "diou"), ("bev", "iou")):
        first, moved = None, 0
        for off in bt.OFFSETS:
            if not (bt.is_exact_translation(a, off) and bt.is_exact_translation(b, off)):
                continue
            got = _call(dev, bt.translate(a, off), bt.translate(b, off), mode=mode, kind=kind)
            first = first or got
            moved += 1
            for name, g, f in zip(("loss", "iou", "grad"), got, first):
                np.testing.assert_array_equal(g.view(np.int32), f.view(np.int32), err_msg=f"{family} {mode} {kind}: {name} moved by {off}")
        assert moved >= 3


# ---- 4: weights ------------------------------------------------------------------------------------------------------
def test_weights_select_and_need_grad(sad, dev):
    import torch
    from sad_amd import ops
    a, b = bt.pair_family("perturbed", "object", 300, seed=4)
    for mode, kind in (("3d", "diou"), ("bev", "iou")):
        plain = _call(dev, a, b, mode=mode, kind=kind)
        ones = _call(dev, a, b, np.ones(300, F), mode=mode, kind=kind)
        for x, y in zip(plain, ones):
            np.testing.assert_array_equal(x.view(np.int32), y.view(np.int32), err_msg="weight = None against weight = 1")
        wt = np.where(np.arange(300) % 3 == 0, 0, np.linspace(0.5, 2, 300)).astype(F)
        an, bn = a.copy(), b.copy()
        an[::6], bn[3::6] = np.nan, np.nan                      # NaN boxes, in rows of weight 0 only
        loss, iou, grad = _call(dev, an, bn, wt, mode=mode, kind=kind)
        off = wt == 0
        assert (loss[off].view(np.int32) == 0).all() and (grad[off].view(np.int32) == 0).all(), "a row of weight 0 gives +0"
        _same((loss, iou[~off], grad), (np.where(off, 0, plain[0] * wt), plain[1][~off], np.where(off[:, None], 0, plain[2] * wt[:, None])), "weights")
        # need_grad = False: the same loss and iou, and no gradient buffer is touched
        guard = torch.full((300, 7), NAN, device=dev)
        l2, i2 = _call(dev, an, bn, wt, mode=mode, kind=kind, need_grad=False)
        np.testing.assert_array_equal(l2.view(np.int32), loss.view(np.int32))
        np.testing.assert_array_equal(i2.view(np.int32), iou.view(np.int32))
        assert torch.isnan(guard).all()
        with pytest.raises(ValueError, match="out: expected contiguous"):
            ops.rotated_iou_loss(_t(a, dev), _t(b, dev), need_grad=False, out=(guard[:, 0].contiguous(), guard[:, 1].contiguous(), guard))


# ---- 5: code = roi ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _roi_targets(S, dev):
    """ProposalTargetLayer's targets on two box_truth.roi_scene scenes, and seeded residuals near the regression target."""
    import torch
    from sad_amd import roi_head
    sc = [bt.roi_scene(130, 9, s) for s in range(2)]
    rois, gt = np.stack([x[0] for x in sc]), np.stack([x[1] for x in sc])
    layer = roi_head.ProposalTargetLayer(roi_per_image=S, by_class=False, seed=3)
    tg = layer(_t(rois, dev), None, _t(gt, dev), torch.zeros(2, 9, dtype=torch.int32, device=dev))
    noise = torch.from_numpy(np.random.default_rng(S).normal(0, 0.05, (2, S, 7)).astype(F)).to(dev)
    reg = torch.where(tg.reg_valid[..., None] != 0, tg.reg_target, torch.zeros_like(tg.reg_target)) + noise
    return layer, tg, reg.contiguous()


@pytest.mark.parametrize("S", [1, 128, 257])
def test_roi_code(sad, dev, S):
    import torch
    _, tg, reg = _roi_targets(S, dev)
    wt = (tg.reg_valid != 0).to(torch.float32)
    reg_n, gl_n, rois_n, wt_n = (t.cpu().numpy() for t in (reg, tg.gt_local, tg.rois_s, wt))
    flat = lambda x: x.reshape(2 * S, -1)
    for mode, kind in (("3d", "diou"), ("bev", "iou"), ("3d", "iou")):
        loss, iou, grad, dec = _call(dev, reg_n, gl_n, wt_n, mode=mode, kind=kind, code="roi", rois=rois_n, decoded=True)
        want = ref.decode(flat(reg_n), flat(rois_n))
        d = flat(dec)
        np.testing.assert_array_equal(d[:, [0, 1, 2, 6]], want[:, [0, 1, 2, 6]], err_msg="decoded, the columns without expf")
        assert (np.abs(d[:, 3:6] - want[:, 3:6]) <= 1e-4 + 1e-4 * np.abs(want[:, 3:6])).all(), "decoded extents beyond SPEC §9's rule"
        again = ref.rotated_iou_loss(flat(reg_n), flat(gl_n), wt_n.reshape(-1), mode, kind, "roi", flat(rois_n), decoded=d)
        _same((loss, iou, grad), again[:3], f"S={S} {mode} {kind} on the device's decoded boxes")
        if S > 1:
            assert (wt_n != 0).sum() >= 8 and np.abs(grad).max() > 0
        # rois of D = 9 columns: the same bits
        wide = _call(dev, reg_n, gl_n, wt_n, mode=mode, kind=kind, code="roi", rois=_widen(rois_n, 9), decoded=True)
        for x, y in zip((loss, iou, grad, dec), wide):
            np.testing.assert_array_equal(x.view(np.int32), y.view(np.int32))


# ---- 6: autograd and modules -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("Dp", [7, 9])
def test_module_backward_is_the_operators_gradient(sad, dev, Dp):
    import torch
    from sad_amd import RotatedIoULoss, ops
    a, b = bt.pair_family("perturbed", "object", 300, seed=12)
    wt = np.random.default_rng(13).uniform(0.5, 2, 300).astype(F)
    tb, tw = _t(b, dev), _t(wt, dev)
    for mode, kind in (("3d", "diou"), ("bev", "iou")):
        pred = _t(_widen(a, Dp, 0.0), dev).requires_grad_()
        loss, iou, grad = ops.rotated_iou_loss(pred.detach(), tb, tw, mode=mode, kind=kind)
        mod = RotatedIoULoss(mode, kind)
        out = mod(pred, tb, tw)
        assert out.shape == (300,) and torch.equal(out, loss) and torch.equal(mod.iou, iou) and not mod.iou.requires_grad
        out.sum().backward()
        assert pred.grad.shape == (300, Dp) and torch.equal(pred.grad[:, :7], grad) and (pred.grad[:, 7:] == 0).all()
        pred.grad = None
        total = RotatedIoULoss(mode, kind, reduction="sum")(pred, tb, tw)
        mean = RotatedIoULoss(mode, kind, reduction="mean")(pred, tb, tw)
        assert total.dim() == 0 and torch.equal(total, loss.sum()) and torch.equal(mean, loss.sum() / 300)
        (2.0 * total).backward()
        assert torch.equal(pred.grad[:, :7], grad * 2.0)


def test_roi_module(sad, dev):
    import torch
    from sad_amd import ops, roi_head
    S = 128
    layer, tg, reg = _roi_targets(S, dev)
    for mode, kind, normalize in (("3d", "diou", True), ("bev", "iou", False)):
        mod = layer.iou_loss(mode=mode, kind=kind, normalize=normalize)
        assert isinstance(mod, roi_head.RoIIoULoss) and mod.iou is None
        leaf = reg.reshape(2 * S, 7).clone().requires_grad_()                     # [B*S,7]: viewed, never copied
        out = mod(leaf, tg)
        wt = (tg.reg_valid != 0).to(torch.float32)
        loss, iou, grad, dec = ops.rotated_iou_loss(leaf.detach().view(2, S, 7), tg.gt_local, wt, mode=mode, kind=kind, code="roi",
                                                    rois=tg.rois_s, decoded=True)
        n = (tg.reg_valid != 0).sum(1).clamp(min=1).to(torch.float32)
        assert out.shape == (2,) and torch.equal(out, loss.sum(1) / n if normalize else loss.sum(1))
        assert torch.equal(mod.iou, iou) and torch.equal(mod.iou, ops.boxes_iou_aligned(dec, tg.gt_local, mode))
        out.sum().backward()
        scale = (torch.ones_like(n) / n if normalize else torch.ones_like(n))[:, None, None]
        assert leaf.grad.shape == (2 * S, 7) and torch.equal(leaf.grad, (grad * scale).view(2 * S, 7))
        assert (leaf.grad.view(2, S, 7)[tg.reg_valid == 0] == 0).all() and leaf.grad.abs().max() > 0
    with pytest.raises(ValueError, match="contiguous predictions"):
        mod(reg.transpose(0, 1), tg)


@pytest.mark.parametrize("size", SIZES)
def test_device_gradient_against_the_truth(sad, dev, size):
    """The device gradient, like the reference's, lies within G_TOL x gscale of the central differences of the binary64 loss on the
    well-conditioned pairs."""
    for family in truth.TRUTH_FAMILIES:
        a, b = bt.pair_family(family, size, 257, seed=1)
        keep = truth.well_conditioned(family, a, b)
        a, b = a[keep], b[keep]
        for mode, kind in (("3d", "diou"), ("bev", "iou")):
            loss, iou, grad = _call(dev, a, b, mode=mode, kind=kind)
            l64, g64, ill = truth.grad64(a, b, mode, kind)
            err = (np.abs(grad - g64) / truth.gscale(a, b))[~ill]
            print(f"{family} {size} {mode} {kind}: {len(a)} pairs, {int(ill.sum())} ill-conditioned, max err / gscale {err.max():.3f}")
            assert err.max() <= truth.G_TOL and ill.mean() < 0.02
            assert (np.abs(loss - l64) <= bt.tol(a, b) + 2.0 ** -20).all()
