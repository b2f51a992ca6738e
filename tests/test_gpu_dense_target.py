"""GPU parity of the dense head target assignment (SPEC.md §26) (-m gpu): ops.anchor_targets, ops.center_targets and the
assigner modules against tests/dense_target_ref.py.  Parity rules of §26: labels, match, max_iou, dir_target and t0, t1, t2,
t6 of reg_target are EQUAL to the reference under ==, t3..t5 (logf) within §9's 1e-4 (absolute + relative); ind, the set of
non-zero heat-map cells, the cells equal to 1.0f and anno columns 0-2 and 6-9 are EQUAL, heat-map values and the logf columns
within 1e-4.  Outputs are pre-filled with NaN / a sentinel before every call; a second call is bit-identical to the first;
the nhwc heat map is the permuted nchw one bit for bit.  The coverage every case relies on is asserted on the reference in
tests/test_dense_target_cpu.py; nothing is skipped."""
import numpy as np
import pytest

import dense_target_ref as ref

pytestmark = pytest.mark.gpu

F = np.float32
SENTINEL = -77777


def _t(a, dev):
    import torch
    return None if a is None else torch.from_numpy(np.array(a, order="C")).to(dev)       # (a copy: the cases are read-only)


def _poison(spec, dev):
    import torch
    return tuple(torch.full(shape, float("nan") if dt == torch.float32 else SENTINEL, dtype=dt, device=dev) for shape, dt in spec)


def _run_anchor(c, dev):
    """One call into poisoned outputs -> {name: numpy}."""
    import torch
    from sad_amd import ops
    kw = c["kw"]
    B = c["gt_labels"].shape[0]
    K = kw["H"] * kw["W"] * len(kw["sizes"]) * len(kw["rotations"])
    spec = [((B, K), torch.int32), ((B, K), torch.int32), ((B, K, 7), torch.float32), ((B, K), torch.float32)]
    if kw["nb"]:
        spec.append(((B, K), torch.int32))
    out = _poison(spec, dev)
    got = ops.anchor_targets(_t(c["gt_boxes"], dev), _t(c["gt_labels"], dev), out=out, **kw)
    assert len(got) == len(out) and all(g is o for g, o in zip(got, out))
    return {n: g.cpu().numpy() for n, g in zip(ref.ANCHOR_OUTPUTS, got)}


def _run_center(c, dev, layout="nchw"):
    import torch
    from sad_amd import ops
    kw = c["kw"]
    B, G = c["gt_labels"].shape
    C, H, W = kw["C"], kw["H"], kw["W"]
    spec = [((B, C, H, W) if layout == "nchw" else (B, H, W, C), torch.float32), ((B, G), torch.int32),
            ((B, G, 10 if kw["vel"] else 8), torch.float32)]
    out = _poison(spec, dev)
    got = ops.center_targets(_t(c["gt_boxes"], dev), _t(c["gt_labels"], dev), layout=layout, out=out, **kw)
    assert all(g is o for g, o in zip(got, out))
    return {n: g.cpu().numpy() for n, g in zip(ref.CENTER_OUTPUTS, got)}


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
    assert not bad.any(), f"{what}: {int(bad.sum())} of {want.size} differ under =="


def _near(got, want, what):
    """§9: 1e-4 absolute + relative; infinities must match exactly."""
    inf = np.isinf(want)
    assert np.array_equal(got[inf], want[inf]), f"{what}: infinities differ"
    err = np.abs(got[~inf].astype(np.float64) - want[~inf])
    ok = err <= 1e-4 + 1e-4 * np.abs(want[~inf])
    assert ok.all(), f"{what}: {int((~ok).sum())} of {ok.size} beyond 1e-4, worst {float(err.max()):.3g}"


def _anchor_parity(got, want, what):
    _written(got, what)
    for n in ("labels", "match", "max_iou") + (("dir_target",) if "dir_target" in got else ()):
        _equal(got[n], want[n], f"{what} {n}")
    assert ("dir_target" in got) == ("dir_target" in want)
    for j in (0, 1, 2, 6):
        _equal(got["reg_target"][..., j], want["reg_target"][..., j], f"{what} t{j}")
    _near(got["reg_target"][..., 3:6], want["reg_target"][..., 3:6], f"{what} t3..t5")


def _center_parity(got, want, what):
    _written(got, what)
    _equal(got["ind"], want["ind"], f"{what} ind")
    hm, whm = got["heatmap"], want["heatmap"]
    assert hm.shape == whm.shape
    assert np.array_equal(hm != 0, whm != 0), f"{what}: the sets of non-zero cells differ"
    assert np.array_equal(hm == 1, whm == 1), f"{what}: the cells equal to 1.0 differ"
    _near(hm, whm, f"{what} heatmap")
    anno, wanno = got["anno"], want["anno"]
    for j in (0, 1, 2) + tuple(range(6, anno.shape[-1])):
        _equal(anno[..., j], wanno[..., j], f"{what} anno column {j}")
    _near(anno[..., 3:6], wanno[..., 3:6], f"{what} anno log columns")


@pytest.mark.parametrize("name", ref.ANCHOR_CASES)
def test_anchor_targets_parity_and_determinism(dev, name):
    c = ref.case(name)
    got = _run_anchor(c, dev)
    _anchor_parity(got, ref.expected(name), name)
    _same_bits(_run_anchor(c, dev), got, f"{name}: second call")


@pytest.mark.parametrize("name", ref.CENTER_CASES)
def test_center_targets_parity_layouts_and_determinism(dev, name):
    c = ref.case(name)
    got = _run_center(c, dev)
    _center_parity(got, ref.expected(name), name)
    _same_bits(_run_center(c, dev), got, f"{name}: second call")
    nhwc = _run_center(c, dev, layout="nhwc")
    nhwc["heatmap"] = np.ascontiguousarray(nhwc["heatmap"].transpose(0, 3, 1, 2))
    _same_bits(nhwc, got, f"{name}: nhwc against nchw")


def test_modules_forward_the_operators(dev):
    import torch
    from sad_amd import dense_head, ops
    c = ref.case("t:5x7")
    kw = c["kw"]
    gt, lab = _t(c["gt_boxes"], dev), _t(c["gt_labels"], dev)
    dec = dense_head.AnchorHeadDecoder(kw["sizes"], kw["z_center"], kw["rotations"], kw["origin"], kw["step"], kw["dir_offset"])
    asg = dec.assigner(kw["pos_thr"], kw["neg_thr"], kw["size_class"], nb=kw["nb"])
    got = asg(gt, lab, kw["H"], kw["W"])
    _anchor_parity({n: g.cpu().numpy() for n, g in zip(ref.ANCHOR_OUTPUTS, got)}, ref.expected("t:5x7"), "AnchorTargetAssigner")
    for a, b in zip(got, ops.anchor_targets(gt, lab, **kw)):
        assert torch.equal(a, b)
    # a kept workspace gives the same bits
    ws = ops.anchor_targets_workspace(*c["gt_labels"].shape, dev)
    for a, b in zip(got, ops.anchor_targets(gt, lab, workspace=ws, **kw)):
        assert torch.equal(a, b)
    c = ref.case("ct:9x130")
    kw = c["kw"]
    gt, lab = _t(c["gt_boxes"], dev), _t(c["gt_labels"], dev)
    for layout in ("nchw", "nhwc"):
        casg = dense_head.CenterHeadDecoder(kw["origin"], kw["cell"], layout=layout).assigner(kw["C"], kw["min_overlap"], kw["min_radius"], kw["vel"])
        got = casg(gt, lab, kw["H"], kw["W"])
        for a, b in zip(got, ops.center_targets(gt, lab, layout=layout, **kw)):
            assert torch.equal(a, b)
    _center_parity({n: g.cpu().numpy() for n, g in zip(ref.CENTER_OUTPUTS, (got[0].permute(0, 3, 1, 2).contiguous(),) + got[1:])},
                   ref.expected("ct:9x130"), "CenterTargetAssigner")


def test_anchor_round_trip_on_the_device(dev):
    """anchor_targets, then ops.anchor_decode on maps that carry reg_target and a one-hot of dir_target: every positive row
    decodes to its matched ground-truth box."""
    import torch
    from sad_amd import ops
    c = ref.case("t:round")
    kw = c["kw"]
    out = _run_anchor(c, dev)
    B, K = out["labels"].shape
    H, W, nb = kw["H"], kw["W"], kw["nb"]
    A = K // (H * W)
    reg = torch.from_numpy(out["reg_target"]).to(dev).reshape(B, H, W, A * 7).permute(0, 3, 1, 2).contiguous()
    onehot = (torch.from_numpy(out["dir_target"]).to(dev)[..., None] == torch.arange(nb, device=dev)).float()
    dir_ = onehot.reshape(B, H, W, A * nb).permute(0, 3, 1, 2).contiguous()
    cls = torch.zeros((B, A, H, W), device=dev)
    boxes, _, _ = ops.anchor_decode(cls, reg, dir_, sizes=kw["sizes"], z_center=kw["z_center"], rotations=kw["rotations"],
                                    origin=kw["origin"], step=kw["step"], dir_offset=kw["dir_offset"])
    ref.check_anchor_round_trip(c, out, boxes.cpu().numpy())


def test_center_round_trip_on_the_device(dev):
    """center_targets, anno scattered to maps at ind, then ops.center_decode at index = ind: the ground-truth boxes."""
    from sad_amd import ops
    c = ref.case("ct:round")
    kw = c["kw"]
    out = _run_center(c, dev)
    hm, reg, height, dim, rot, vel = (_t(m, dev) for m in ref.center_maps(c, out))
    index = _t(np.where(out["ind"] >= 0, out["ind"], 0).astype(np.int32), dev)
    boxes, _, _ = ops.center_decode(hm, reg, height, dim, rot, vel, origin=kw["origin"], cell=kw["cell"], index=index)
    ref.check_center_round_trip(c, out, boxes.cpu().numpy())
