"""GPU parity of the dense head losses (SPEC.md §27) (-m gpu): ops.anchor_head_loss, ops.center_head_loss, the autograd
Functions and the modules against tests/dense_loss_ref.py.  Parity rules of §27: num_pos is exact; the regression terms,
grad_reg and the centre head's regression gradients are EQUAL to the float32 reference under ==; what passes through expf /
logf / log1pf (classification, direction, heat map) is within §9's 1e-4 (absolute + relative) of the binary64 evaluation.  The
sums are checked on their own: loss[b, i] against the binary64 sum of the device's per_anchor[b, :, i] within n 2^-23 sum|terms|
(§21.4's rule); the centre head, which has no per-element output, against the reference's binary64 sum with the terms'
tolerance added.  Outputs are pre-filled with NaN / a sentinel before every call; a second call is bit-identical; nhwc gives the
same loss and num_pos and the permuted gradients bit for bit.  Every anchor case runs a second time with normalize=False,
where no output is scaled down towards the absolute part of the tolerance.  The coverage every case relies on is asserted on the reference
in tests/test_dense_loss_cpu.py; nothing is skipped."""
import numpy as np
import pytest

import dense_loss_ref as ref

pytestmark = pytest.mark.gpu

F = np.float32
D = np.float64
SENTINEL = -77777
ANCHOR_MAPS = ("cls", "reg", "dir")


def _t(a, dev):
    import torch
    return None if a is None else torch.from_numpy(np.array(a, order="C")).to(dev)       # (a copy: the cases are read-only)


def _poison(spec, dev):
    import torch
    return tuple(torch.full(shape, float("nan") if dt == torch.float32 else SENTINEL, dtype=dt, device=dev) for shape, dt in spec)


def _lay(m, layout):
    return ref.to_nhwc(m) if layout == "nhwc" else m


def _run_anchor(c, dev, layout="nchw", **over):
    """One call into poisoned outputs -> {name: numpy}, gradients back in nchw."""
    import torch
    from sad_amd import ops
    maps = [_t(_lay(c[n], layout), dev) for n in ANCHOR_MAPS]
    B, K = c["labels"].shape
    spec = [((B, 3), torch.float32), ((B,), torch.int32)] + [(tuple(m.shape), torch.float32) for m in maps if m is not None]
    spec.append(((B, K, 3), torch.float32))
    out = _poison(spec, dev)
    kw = dict(c["kw"], **over)
    got = ops.anchor_head_loss(*maps, _t(c["labels"], dev), _t(c["reg_target"], dev), _t(c["dir_target"], dev), layout=layout,
                               per_anchor=True, out=out, **kw)
    assert len(got) == len(out) and all(g is o for g, o in zip(got, out))
    names = ["loss", "num_pos", "grad_cls", "grad_reg"] + (["grad_dir"] if c["nb"] else []) + ["per_anchor"]
    res = {n: g.cpu().numpy() for n, g in zip(names, got)}
    if layout == "nhwc":
        res.update({n: ref.from_nhwc(v) for n, v in res.items() if n.startswith("grad_")})
    return res


def _run_center(c, dev, layout="nchw"):
    import torch
    from sad_amd import ops
    maps = [_t(_lay(c[n], layout), dev) for n in ("hm",) + ref.CENTER_MAPS]
    B = c["hm"].shape[0]
    spec = [((B, 2), torch.float32), ((B, 2), torch.int32)] + [(tuple(m.shape), torch.float32) for m in maps if m is not None]
    out = _poison(spec, dev)
    got = ops.center_head_loss(*maps, _t(_lay(c["heatmap"], layout), dev), _t(c["ind"], dev), _t(c["anno"], dev), layout=layout, out=out,
                               **c["kw"])
    assert len(got) == len(out) and all(g is o for g, o in zip(got, out))
    names = ["loss", "num_pos", "grad_hm"] + ["grad_" + n for n in ref.CENTER_MAPS if c[n] is not None]
    res = {n: g.cpu().numpy() for n, g in zip(names, got)}
    if layout == "nhwc":
        res.update({n: ref.from_nhwc(v) for n, v in res.items() if n.startswith("grad_")})
    return res


def _written(got, what):
    for n, v in got.items():
        assert not (np.isnan(v).any() if v.dtype == F else (v == SENTINEL).any()), f"{what}: {n} not fully written"


def _same_bits(a, b, what):
    assert set(a) == set(b)
    for n in a:
        assert a[n].shape == b[n].shape and a[n].dtype == b[n].dtype, (what, n)
        bad = int((a[n].view(np.int32) != b[n].view(np.int32)).sum())
        assert bad == 0, f"{what}: {bad} of {a[n].size} words of {n} differ"


def _equal(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    bad = ~(got == want)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {want.size} differ under ==, first at {np.argwhere(bad)[0].tolist()}"


def _near(got, want64, what):
    """§9: 1e-4 absolute + relative against the binary64 evaluation."""
    assert got.shape == want64.shape, (what, got.shape, want64.shape)
    err = np.abs(got.astype(D) - want64)
    ok = err <= 1e-4 + 1e-4 * np.abs(want64)
    print(f"{what}: worst error {float(err.max()) if err.size else 0:.3g}")
    assert ok.all(), f"{what}: {int((~ok).sum())} of {ok.size} beyond 1e-4, worst {float(err.max()):.3g}"


def _anchor_parity(got, name, normalize=True):
    want, w64 = ref.expected(name, normalize)["f32"], ref.expected(name, normalize)["f64"]
    name = name if normalize else name + " unnormalised"
    _written(got, name)
    _equal(got["num_pos"], want["num_pos"], f"{name} num_pos")
    _equal(got["per_anchor"][..., 1], want["per_anchor"][..., 1], f"{name} regression terms")
    _equal(got["grad_reg"], want["grad_reg"], f"{name} grad_reg")
    _near(got["per_anchor"][..., 0], w64["per_anchor"][..., 0], f"{name} classification terms")
    _near(got["per_anchor"][..., 2], w64["per_anchor"][..., 2], f"{name} direction terms")
    _near(got["grad_cls"], w64["grad_cls"], f"{name} grad_cls")
    assert ("grad_dir" in got) == ("grad_dir" in want)
    if "grad_dir" in got:
        _near(got["grad_dir"], w64["grad_dir"], f"{name} grad_dir")
    # the reduction on its own: against the binary64 sum of the device's own terms, §21.4's rule
    terms = got["per_anchor"].astype(D)
    n = terms.shape[1]
    bound = n * 2.0 ** -23 * np.abs(terms).sum(1)
    err = np.abs(got["loss"].astype(D) - terms.sum(1))
    print(f"{name}: loss error {err.max():.3g}, bound {bound.max():.3g}")
    assert (err <= bound).all(), f"{name}: loss off its terms' sum by {err.tolist()}, bound {bound.tolist()}"


def _center_parity(got, name):
    want, w64 = ref.expected(name)["f32"], ref.expected(name)["f64"]
    _written(got, name)
    _equal(got["num_pos"], want["num_pos"], f"{name} num_pos")
    for n in got:
        if n.startswith("grad_") and n != "grad_hm":
            _equal(got[n], want[n], f"{name} {n}")
    _near(got["grad_hm"], w64["grad_hm"], f"{name} grad_hm")
    B = got["loss"].shape[0]
    th, tr = w64["terms_hm"].reshape(B, -1), want["terms_reg"].astype(D).reshape(B, -1)
    b0 = (1e-4 + 1e-4 * np.abs(th)).sum(1) + th.shape[1] * 2.0 ** -23 * np.abs(th).sum(1)
    b1 = tr.shape[1] * 2.0 ** -23 * np.abs(tr).sum(1)              # (the regression terms pass through no library function)
    e0, e1 = np.abs(got["loss"][:, 0].astype(D) - th.sum(1)), np.abs(got["loss"][:, 1].astype(D) - tr.sum(1))
    print(f"{name}: loss errors {e0.tolist()} {e1.tolist()}, bounds {b0.tolist()} {b1.tolist()}")
    assert (e0 <= b0).all() and (e1 <= b1).all(), f"{name}: loss errors {e0.tolist()} {e1.tolist()}, bounds {b0.tolist()} {b1.tolist()}"


@pytest.mark.parametrize("name", ref.ANCHOR_CASES)
def test_anchor_head_loss_parity_layouts_and_determinism(dev, name):
    c = ref.case(name)
    got = _run_anchor(c, dev)
    _anchor_parity(got, name)
    _same_bits(_run_anchor(c, dev), got, f"{name}: second call")
    _same_bits(_run_anchor(c, dev, layout="nhwc"), got, f"{name}: nhwc against nchw")
    # normalize=False: wq_i = scale_i.  Normalised, a scene with a thousand positives shrinks its direction gradients and its
    # hot-class terms towards the absolute part of the tolerance; here they keep their natural size (asserted on the reference
    # in test_dense_loss_cpu), so the 1e-4 rule tests the softmax, the focal terms and their chunking at full strength
    un = _run_anchor(ref.unnormalised(c), dev)
    _anchor_parity(un, name, normalize=False)
    _same_bits(_run_anchor(ref.unnormalised(c), dev, layout="nhwc"), un, f"{name}: unnormalised nhwc against nchw")


def test_exactly_summable_loss_is_exact(dev):
    """l:exact: every term and every partial sum in any order is a binary32 number (asserted in test_dense_loss_cpu), so the
    regression loss equals the reference under == whatever the order of the additions."""
    for layout in ("nchw", "nhwc"):
        got = _run_anchor(ref.case("l:exact"), dev, layout=layout)
        _equal(got["loss"][:, 1], ref.expected("l:exact")["f32"]["loss"][:, 1], f"l:exact {layout} loss[:, 1]")


@pytest.mark.parametrize("name", ref.CENTER_CASES)
def test_center_head_loss_parity_layouts_and_determinism(dev, name):
    c = ref.case(name)
    got = _run_center(c, dev)
    _center_parity(got, name)
    _same_bits(_run_center(c, dev), got, f"{name}: second call")
    _same_bits(_run_center(c, dev, layout="nhwc"), got, f"{name}: nhwc against nchw")


def test_shared_cells_add_in_ascending_g(dev):
    """c:shared: four boxes of scene 1 share cell 9 with gradients + + + - of one magnitude: the ascending-g sum, which is not
    what another order gives (asserted in test_dense_loss_cpu)."""
    got = _run_center(ref.case("c:shared"), dev)
    m = ref.SHARED_CW
    assert got["grad_reg"][1, 0].reshape(-1)[9] == F(F(F(m + m) + m) - m) != F(F(F(-m + m) + m) + m)
    _equal(got["grad_reg"], ref.expected("c:shared")["f32"]["grad_reg"], "c:shared grad_reg")


def test_modules_and_autograd(dev):
    import torch
    from sad_amd import dense_head, ops
    # anchor head
    c = ref.case("l:9x130")
    kw = c["kw"]
    maps = [_t(c[n], dev).requires_grad_() for n in ANCHOR_MAPS]
    tg = (_t(c["labels"], dev), _t(c["reg_target"], dev), _t(c["dir_target"], dev))
    want = ops.anchor_head_loss(*[m.detach() for m in maps], *tg, **kw)
    dec = dense_head.AnchorHeadDecoder([[1.0, 1.0, 1.0]] * 3, [0.0] * 3, [0.0, 1.57], (0.0, 0.0), (1.0, 1.0))
    mod = dec.loss(**kw)
    assert isinstance(mod, dense_head.AnchorHeadLoss) and mod.cfg == dense_head.AnchorHeadLoss(**kw).cfg
    loss = mod(*maps, *tg)
    assert torch.equal(loss, want[0]) and torch.equal(mod.num_pos, want[1]) and loss.requires_grad
    loss.sum().backward()
    for m, g in zip(maps, want[2:5]):
        assert torch.equal(m.grad, g)
    # a non-trivial upstream gradient scales the saved gradients per scene and component
    up = torch.tensor([[0.5, -2.0, 3.0], [1.25, 0.0, -1.0], [-0.75, 4.0, 0.125]], device=dev)
    for m in maps:
        m.grad = None
    (mod(*maps, *tg) * up).sum().backward()
    for i, (m, g) in enumerate(zip(maps, want[2:5])):
        assert torch.equal(m.grad, g * up[:, i].view(-1, 1, 1, 1))
    # a kept workspace gives the same bits
    B, _, H, W = c["reg"].shape
    ws = ops.anchor_head_loss_workspace(B, H, W, c["A"], dev)
    for a, b in zip(want, ops.anchor_head_loss(*[m.detach() for m in maps], *tg, workspace=ws, **kw)):
        assert torch.equal(a, b)
    # without dir: loss[:, 2] = 0 and no grad_dir
    nodir = ops.anchor_head_loss(maps[0].detach(), maps[1].detach(), None, tg[0], tg[1], None, **kw)
    assert len(nodir) == 4 and torch.equal(nodir[0][:, :2], want[0][:, :2]) and (nodir[0][:, 2] == 0).all()
    # centre head, both layouts
    c = ref.case("c:9x130")
    kw = c["kw"]
    for layout in ("nchw", "nhwc"):
        maps = [_t(_lay(c[n], layout), dev).requires_grad_() for n in ("hm",) + ref.CENTER_MAPS]
        tg = (_t(_lay(c["heatmap"], layout), dev), _t(c["ind"], dev), _t(c["anno"], dev))
        want = ops.center_head_loss(*[m.detach() for m in maps], *tg, layout=layout, **kw)
        mod = dense_head.CenterHeadDecoder((0.0, 0.0), (1.0, 1.0), layout=layout).loss(**kw)
        assert isinstance(mod, dense_head.CenterHeadLoss) and mod.cfg == dense_head.CenterHeadLoss(layout=layout, **kw).cfg
        up = torch.tensor([[0.5, -2.0], [1.25, 0.0], [-0.75, 4.0]], device=dev)
        (mod(*maps, *tg) * up).sum().backward()
        assert torch.equal(mod.num_pos, want[1])
        for i, (m, g) in enumerate(zip(maps, want[2:])):
            assert torch.equal(m.grad, g * up[:, 0 if i == 0 else 1].view(-1, 1, 1, 1))
        ws = ops.center_head_loss_workspace(3, 9, 130, 1024, dev)
        for a, b in zip(want, ops.center_head_loss(*[m.detach() for m in maps], *tg, layout=layout, workspace=ws, **kw)):
            assert torch.equal(a, b)


def test_anchor_chain_on_the_device(dev):
    """ops.anchor_targets, then anchor_head_loss on its outputs where they are: maps that carry reg_target exactly give a
    regression loss and gradient of exactly 0; num_pos counts the assigner's positives."""
    import torch
    import dense_target_ref as tref
    from sad_amd import ops
    c = tref.case("t:9x130")
    kw = c["kw"]
    labels, _, reg_target, _, dir_target = ops.anchor_targets(_t(c["gt_boxes"], dev), _t(c["gt_labels"], dev), **kw)
    B, K = labels.shape
    H, W, nb = kw["H"], kw["W"], kw["nb"]
    A = K // (H * W)
    reg = reg_target.reshape(B, H, W, A * 7).permute(0, 3, 1, 2).contiguous()
    g = torch.Generator(device="cpu").manual_seed(3)
    cls = torch.randn((B, A * 3, H, W), generator=g).to(dev)
    dir_ = torch.randn((B, A * nb, H, W), generator=g).to(dev)
    loss, num_pos, gcls, greg, gdir = ops.anchor_head_loss(cls, reg, dir_, labels, reg_target, dir_target)
    assert torch.equal(num_pos, (labels >= 0).sum(1).int()) and int(num_pos.sum()) > 0
    assert (loss[:, 1] == 0).all() and (greg == 0).all()
    assert (loss[:, 0] > 0).all() and torch.isfinite(loss).all() and torch.isfinite(gcls).all() and torch.isfinite(gdir).all()
    assert (loss[:, 2] > 0).any()
    # nhwc: reg_target viewed [B,H,W,A*7] IS the nhwc map, read where it is
    loss2 = ops.anchor_head_loss(cls.permute(0, 2, 3, 1).contiguous(), reg_target.view(B, H, W, A * 7), dir_.permute(0, 2, 3, 1).contiguous(),
                                 labels, reg_target, dir_target, layout="nhwc")[0]
    assert torch.equal(loss2, loss)


def test_center_chain_on_the_device(dev):
    """ops.center_targets, then center_head_loss: maps that carry anno at ind give a regression loss and gradients of exactly 0."""
    import torch
    import dense_target_ref as tref
    from sad_amd import ops
    c = tref.case("ct:round")
    kw = c["kw"]
    heatmap, ind, anno = ops.center_targets(_t(c["gt_boxes"], dev), _t(c["gt_labels"], dev), **kw)
    out = {"heatmap": heatmap.cpu().numpy(), "ind": ind.cpu().numpy(), "anno": anno.cpu().numpy()}
    _, reg, height, dim, rot, vel = (_t(m, dev) for m in tref.center_maps(c, out))
    hm = torch.full_like(heatmap, -2.0)
    res = ops.center_head_loss(hm, reg, height, dim, rot, vel, heatmap, ind, anno)
    loss, num_pos = res[0], res[1]
    assert torch.equal(num_pos[:, 1], (ind >= 0).sum(1).int()) and int(num_pos[:, 1].sum()) > 0
    assert torch.equal(num_pos[:, 0], (heatmap == 1).flatten(1).sum(1).int())
    assert (loss[:, 1] == 0).all() and all((g == 0).all() for g in res[3:])
    assert (loss[:, 0] > 0).all() and torch.isfinite(res[2]).all()
