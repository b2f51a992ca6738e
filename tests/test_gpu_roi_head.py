"""GPU parity of the RoI head (SPEC.md §28) (-m gpu): ops.roi_targets, ops.roi_decode and roi_head.ProposalTargetLayer against
tests/roi_head_ref.py.  Parity rule of §28: every output is EQUAL to the reference under ==, except t3..t5 of reg_target (logf)
and columns 3..5 of roi_decode (expf), which are within §9's 1e-4 (absolute + relative).  Outputs are pre-filled with NaN / a
sentinel before every call; a second call is bit-identical to the first.  The coverage every case relies on is asserted on the
reference in tests/test_roi_head_cpu.py; nothing is skipped."""
import numpy as np
import pytest

import nms_ref
import roi_head_ref as ref

pytestmark = pytest.mark.gpu

F = np.float32
SENTINEL = -77777


def _t(a, dev):
    import torch
    return None if a is None else torch.from_numpy(np.array(a, order="C")).to(dev)       # (a copy: the cases are read-only)


def _inputs(c, dev):
    return tuple(_t(c[k], dev) for k in ("rois", "roi_count", "roi_labels", "gt_boxes", "gt_labels"))


def _poison(B, S, dev):
    import torch
    spec = [((B, S), torch.int32)] * 3 + [((B, S), torch.float32)] * 2 + [((B, S), torch.int32)] + [((B, S, 7), torch.float32)] * 3
    return tuple(torch.full(shape, float("nan") if dt == torch.float32 else SENTINEL, dtype=dt, device=dev) for shape, dt in spec)


def _run(c, dev, **more):
    """One call into poisoned outputs -> {name: numpy}."""
    from sad_amd import ops
    out = _poison(c["rois"].shape[0], c["kw"]["S"], dev)
    got = ops.roi_targets(*_inputs(c, dev), out=out, **dict(c["kw"], **more))
    assert len(got) == len(out) and all(g is o for g, o in zip(got, out))
    return {n: g.cpu().numpy() for n, g in zip(ref.OUTPUTS, got)}


def _equal(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    bad = ~(got == want)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {want.size} differ under =="


def _parity(got, want, what):
    for n, v in got.items():
        assert not (np.isnan(v).any() if v.dtype == F else (v == SENTINEL).any()), f"{what}: {n} not fully written"
    for n in ref.OUTPUTS[:-1]:
        _equal(got[n], want[n], f"{what} {n}")
    for q in (0, 1, 2, 6):
        _equal(got["reg_target"][..., q], want["reg_target"][..., q], f"{what} t{q}")
    ref.close(got["reg_target"][..., 3:6], want["reg_target"][..., 3:6], f"{what} t3..t5")


def _same_bits(a, b, what):
    for n in a:
        bad = int((a[n].view(np.int32) != b[n].view(np.int32)).sum())
        assert bad == 0, f"{what}: {bad} of {a[n].size} words of {n} differ"


@pytest.mark.parametrize("name", ref.CASES)
def test_roi_targets_parity_and_determinism(dev, name):
    c = ref.case(name)
    got = _run(c, dev)
    _parity(got, ref.expected(name), name)
    _same_bits(_run(c, dev), got, f"{name}: second call")


def test_the_callers_workspace_is_accepted(dev):
    import torch
    from sad_amd import ops
    c = ref.case("by_class")
    B, R = c["rois"].shape[:2]
    ws = ops.roi_targets_workspace(B, R, dev)
    assert ws.numel() == 8 * B * R
    ws.fill_(0xA5)                                                       # its contents are irrelevant
    _parity(_run(c, dev, workspace=ws), ref.expected("by_class"), "a kept workspace")
    with pytest.raises(ValueError, match="workspace"):
        _run(c, dev, workspace=ws[:-8])
    with pytest.raises(ValueError, match="out"):
        ops.roi_targets(*_inputs(c, dev), out=_poison(B, c["kw"]["S"] + 1, dev), **c["kw"])
    with pytest.raises(ValueError, match="out"):
        ops.roi_targets(*_inputs(c, dev), out=_poison(B, c["kw"]["S"], dev)[:-1], **c["kw"])
    with pytest.raises(ValueError, match="out"):
        ops.roi_targets(*_inputs(c, dev), out=tuple(t.to(torch.float32) for t in _poison(B, c["kw"]["S"], dev)), **c["kw"])


def test_roi_decode_parity_and_round_trip(dev):
    import torch
    from sad_amd import ops
    for name in ("both", "heading", "odd"):
        c, e = ref.case(name), ref.expected(name)
        B, S = e["index"].shape
        # the reference's residuals, and random ones, on rows of D = 7 and of D = 9
        rng = np.random.default_rng(17)
        wide = np.concatenate([e["rois_s"], np.full((B, S, 2), np.nan, F)], -1)
        for rois, reg in ((e["rois_s"], e["reg_target"]), (wide, rng.normal(0, 0.4, (B, S, 7)).astype(F))):
            out = torch.full((B, S, 7), float("nan"), device=dev)
            got = ops.roi_decode(_t(rois, dev), _t(reg, dev), out=out)
            assert got is out
            got, want = got.cpu().numpy(), ref.roi_decode_vec(rois, reg)
            for q in (0, 1, 2, 6):
                _equal(got[..., q], want[..., q], f"{name} decode column {q}")
            ref.close(got[..., 3:6], want[..., 3:6], f"{name} decode sizes")
        # the device's own targets through the device's decoder: the matched ground truth
        mine = _run(c, dev)
        boxes = ops.roi_decode(_t(mine["rois_s"], dev), _t(mine["reg_target"], dev)).cpu().numpy()
        ref.check_round_trip(c, mine, boxes)


def test_module_against_the_operator(dev):
    import torch
    from sad_amd import ops, roi_head
    c = ref.case("by_class")
    rois, _, rl, gt, gl = _inputs(c, dev)
    cfg = dict(roi_per_image=48, fg_ratio=0.5, reg_fg_thresh=0.55, cls_fg_thresh=0.75, cls_bg_thresh=0.25, cls_bg_thresh_lo=0.1,
               hard_bg_ratio=0.8, cls_score_type="roi_iou", by_class=True, seed=21)
    layer = roi_head.ProposalTargetLayer(**cfg)
    first = layer(rois, rl, gt, gl)
    assert first._fields == ref.OUTPUTS and layer.step == 1
    want = ops.roi_targets(rois, None, rl, gt, gl, S=48, fg_max=24, fg_thr=0.55, bg_lo=0.1, hard_ratio=0.8, reg_fg_thr=0.55,
                           cls_fg_thr=0.75, cls_bg_thr=0.25, cls_mode="roi_iou", seed=layer.call_seed(0))
    assert all(torch.equal(a, b) for a, b in zip(first, want))
    # and against the reference under that seed
    kw = dict(c["kw"], S=48, fg_max=24, seed=layer.call_seed(0))
    e = ref.roi_targets_vec(dict(c, kw=kw), ref.iou_of("by_class"))
    _parity({n: t.cpu().numpy() for n, t in zip(ref.OUTPUTS, first)}, e, "ProposalTargetLayer")
    # the same seed gives the same result; the step counter changes the sample
    again = roi_head.ProposalTargetLayer(**cfg)
    assert all(torch.equal(a, b) for a, b in zip(first, again(rois, rl, gt, gl)))
    second = layer(rois, rl, gt, gl)
    assert layer.step == 2 and not torch.equal(first.index, second.index)
    assert all(torch.equal(a, b) for a, b in zip(second, again(rois, rl, gt, gl)))
    # by_class = False does not read the labels
    free = roi_head.ProposalTargetLayer(**dict(cfg, by_class=False))(rois, None, gt, gl)
    assert not torch.equal(free.match, first.match) or not torch.equal(free.index, first.index)
    # decode forwards roi_decode
    assert torch.equal(layer.decode(first.rois_s, first.reg_target), ops.roi_decode(first.rois_s, first.reg_target))


def test_chained_behind_nms_boxes(dev):
    """nms_boxes -> gather by `order` -> roi_targets with roi_count = count, nothing synchronised in between: equal to the reference
    fed the same rows.  The rows of the gathered tensor beyond count are whatever order holds there; they are never read."""
    import torch
    from sad_amd import ops
    c = ref.case("both")
    B, R = c["rois"].shape[:2]
    rng = np.random.default_rng(23)
    scores = rng.uniform(0.05, 1.0, (B, R)).astype(F)
    boxes, sc, gt, gl = _t(c["rois"], dev), _t(scores, dev), _t(c["gt_boxes"], dev), _t(c["gt_labels"], dev)
    keep, order, count = ops.nms_boxes(boxes, sc, None, 0.7, 0.3)
    P = order.shape[1]
    idx = order.clamp(0, R - 1).long()                                    # (order is undefined beyond count: any row will do)
    rois = torch.gather(boxes, 1, idx[..., None].expand(B, P, boxes.shape[2])).contiguous()
    kw = dict(c["kw"], seed=31)
    got = ops.roi_targets(rois, count, None, gt, gl, **kw)
    got = {n: t.cpu().numpy() for n, t in zip(ref.OUTPUTS, got)}          # (the first read-back)
    # the reference chain: the §23 reference's survivors in rank order, NaN beyond the count
    _, want_order, n = nms_ref.nms_boxes(c["rois"], scores, None, 0.7, 0.3)
    assert np.array_equal(count.cpu().numpy(), n) and (n > kw["S"]).all() and (n < R).all()
    fed = np.full((B, P, c["rois"].shape[2]), np.nan, F)
    for b in range(B):
        fed[b, :n[b]] = c["rois"][b, want_order[b, :n[b]]]
    e = ref.roi_targets_vec(dict(rois=fed, roi_count=n, roi_labels=None, gt_boxes=c["gt_boxes"], gt_labels=c["gt_labels"], kw=kw))
    assert all(len(p["fg"]) and len(p["hard"]) and len(p["easy"]) for p in e["plans"])
    _parity(got, e, "chained")
