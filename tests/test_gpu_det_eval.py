"""GPU parity of detection evaluation (SPEC.md §36) (-m gpu): ops.det_match, ops.det_ap and evaluate.DetectionEval against
tests/det_eval_ref.py.  Parity rule of §36: EVERY output equals the reference under ==.  Outputs are pre-filled with NaN / a
sentinel before every call; a second call is bit-identical to the first.  The coverage every case relies on is asserted on the
reference in tests/test_det_eval_cpu.py; nothing is skipped."""
import numpy as np
import pytest

import det_eval_ref as ref

pytestmark = pytest.mark.gpu

F = np.float32
SENTINEL = -77777


def _t(a, dev):
    import torch
    return None if a is None else torch.from_numpy(np.array(a, order="C")).to(dev)       # (a copy: the cases are read-only)


def _inputs(c, dev):
    return tuple(_t(c[k], dev) for k in ("det_boxes", "det_scores", "det_labels", "det_count", "gt_boxes", "gt_labels", "gt_ignore", "thr"))


def _poison(spec, dev):
    import torch
    return tuple(torch.full(shape, float("nan") if dt == torch.float32 else SENTINEL, dtype=dt, device=dev) for _, shape, dt in spec)


def _written(got, what):
    for n, v in got.items():
        assert not (np.isnan(v).any() if v.dtype == F else (v == SENTINEL).any()), f"{what}: {n} not fully written"


def _equal(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    bad = ~(got == want)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {want.size} differ under == (first at {np.argwhere(bad)[0].tolist()})"


def _same_bits(a, b, what):
    for n in a:
        bad = int((a[n].view(np.int32) != b[n].view(np.int32)).sum())
        assert bad == 0, f"{what}: {bad} of {a[n].size} words of {n} differ"


def _match(c, dev):
    """One call into poisoned outputs -> {name: numpy}."""
    from sad_amd import ops
    B, K = c["det_labels"].shape
    out = _poison(ops.det_match_output_spec(B, K, c["gt_labels"].shape[1], *c["thr"].shape), dev)
    got = ops.det_match(*_inputs(c, dev), metric=c["metric"], out=out)
    assert len(got) == len(out) and all(g is o for g, o in zip(got, out))
    return {n: g.cpu().numpy() for n, g in zip(ref.OUTPUTS, got)}


@pytest.mark.parametrize("name", ref.CASES)
def test_det_match_parity_and_determinism(dev, name):
    c, want = ref.case(name), ref.expected(name)
    got = _match(c, dev)
    _written(got, name)
    for n in ref.OUTPUTS:
        _equal(got[n], want[n], f"{name} {n}")
    _same_bits(_match(c, dev), got, f"{name}: second call")


@pytest.mark.parametrize("name,op", [("basic", "boxes_iou3d"), ("wide_rows", "boxes_iou3d"), ("basic:bev", "boxes_iou_bev")])
def test_value_is_the_entry_of_the_pairwise_matrix(dev, name, op):
    """Where a detection has a box, `value` is ops.boxes_iou3d(det, gt)[b, k, match] (boxes_iou_bev for that metric), bit for bit."""
    from sad_amd import ops
    c = ref.case(name)
    got = _match(c, dev)
    iou = getattr(ops, op)(_t(c["det_boxes"], dev), _t(c["gt_boxes"], dev)).cpu().numpy()
    b, k, t = np.nonzero(got["match"] >= 0)
    assert len(b) > 50 and (got["code"][b, k, t] != 0).all()
    _equal(got["value"][b, k, t], iou[b, k, got["match"][b, k, t]], f"{name} value")


def _ap(c, dev, **more):
    from sad_amd import ops
    out = _poison(ops.det_ap_output_spec(c["n_gt"].shape[0], c["code"].shape[1], c["points"], c["first"]), dev)
    got = ops.det_ap(*(_t(c[k], dev) for k in ("scores", "labels", "code", "n_gt")), points=c["points"], first=c["first"], floor=c["floor"],
                     out=out, **more)
    assert all(g is o for g, o in zip(got, out))
    return {n: g.cpu().numpy() for n, g in zip(ref.AP_OUTPUTS, got)}


@pytest.mark.parametrize("name", ref.AP_CASES)
def test_det_ap_parity_and_determinism(dev, name):
    c, want = ref.ap_case(name), ref.ap_expected(name)
    got = _ap(c, dev)
    _written(got, name)
    for n in ref.AP_OUTPUTS:
        _equal(got[n], want[n], f"{name} {n}")
    _same_bits(_ap(c, dev), got, f"{name}: second call")


def test_the_callers_workspace_is_accepted(dev):
    from sad_amd import ops
    c = ref.ap_case("n5000")
    ws = ops.det_ap_workspace(c["scores"].shape[0], dev)
    ws.fill_(0xA5)                                                       # its contents are irrelevant
    got = _ap(c, dev, workspace=ws)
    for n in ref.AP_OUTPUTS:
        _equal(got[n], ref.ap_expected("n5000")[n], f"a kept workspace: {n}")
    with pytest.raises(ValueError, match="workspace"):
        _ap(c, dev, workspace=ws[:-8])
    with pytest.raises(ValueError, match="out"):
        ops.det_ap(*(_t(c[k], dev) for k in ("scores", "labels", "code", "n_gt")), out=_poison(ops.det_ap_output_spec(3, 2, 41, 1), dev))


# ---- the module ---------------------------------------------------------------------------------------------------------------
def _evaluator(c, **kw):
    from sad_amd.evaluate import DetectionEval
    return DetectionEval(c["thr"].shape[0], c["thr"], c["metric"], **dict(dict(capacity=4096), **kw))


def _update(ev, c, dev, scenes=None):
    a = list(_inputs(c, dev))[:7]
    if scenes is not None:
        a = [None if t is None else t[scenes].contiguous() for t in a]
    return ev.update(*a)


def _result_equal(got, want, what):
    assert set(got) == set(want) | {"mean_ap"}
    for n, v in want.items():
        if n == "mean_ap":
            continue
        _equal(got[n], v, f"{what} {n}")


def test_three_updates_equal_the_reference_on_the_concatenation(dev):
    """Three cases of one configuration (C = 3, the IoU thresholds, iou3d), one update each, R11."""
    names = ("basic", "counts", "ties")
    cases = [ref.case(n) for n in names]
    ev = _evaluator(cases[0], points=10, first=0)
    for c in cases:
        _update(ev, c, dev)
    got = ev.compute()
    want = ref.evaluate(cases, 10, 0, 0.0)
    _result_equal(got, want, "three updates")
    valid = want["ap"] >= 0
    assert valid.all() and np.allclose(got["mean_ap"], want["ap"].mean(0))
    ev.reset()
    _update(ev, cases[0], dev)
    _result_equal(ev.compute(), ref.evaluate(cases[:1], 10, 0, 0.0), "after reset")


def test_batch_of_one_equals_batch_of_four_and_merge_equals_the_whole(dev):
    c = ref.case("counts")                                             # B = 4, det_count and ignored boxes
    whole = _evaluator(c)
    _update(whole, c, dev)
    want = whole.compute()
    _result_equal(want, ref.evaluate([c]), "batch of four")
    ones = _evaluator(c)
    for b in range(4):
        _update(ones, c, dev, slice(b, b + 1))
    got = ones.compute()
    _same_bits(got, want, "batch of one against batch of four")
    lo, hi = _evaluator(c), _evaluator(c)
    _update(lo, c, dev, slice(0, 2))
    _update(hi, c, dev, slice(2, 4))
    lo.merge(hi)
    _same_bits(lo.compute(), want, "merge of two halves")
    assert lo.rows == whole.rows == 4 * 33
    with pytest.raises(RuntimeError, match="capacity"):
        small = _evaluator(c, capacity=4 * 33 + 5)
        _update(small, c, dev)
        _update(small, c, dev, slice(0, 1))


def test_nms_gather_update_reads_nothing_back(dev):
    """nms_boxes -> gather -> update under torch.cuda.set_sync_debug_mode("error"): any synchronising call between the detector's
    boxes and the accumulated rows would raise.  (The mode is honoured by torch on ROCm: the .item() below is refused.)"""
    import torch
    from sad_amd import ops
    c = ref.case("basic")
    boxes, scores, labels, _, gt_boxes, gt_labels, gt_ignore, _ = _inputs(c, dev)
    ev = _evaluator(c)
    _update(ev, c, dev)                                                  # (buffers allocated, library loaded)
    ev.reset()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        keep, order, count = ops.nms_boxes(boxes, scores, labels, 0.1)
        idx = order.clamp(min=0).long()
        kept = torch.gather(boxes, 1, idx[..., None].expand(-1, -1, boxes.shape[2]))
        ev.update(kept, torch.gather(scores, 1, idx), torch.gather(labels, 1, idx), count, gt_boxes, gt_labels, gt_ignore)
        with pytest.raises(RuntimeError):
            count[0].item()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    got = ev.compute()
    # the same through the reference: the kept rows in rank order, count of them live
    o, n = order.cpu().numpy(), count.cpu().numpy()
    assert (n > 0).all() and (n < boxes.shape[1]).any()
    g = np.maximum(o, 0)
    k = dict(c, det_boxes=np.take_along_axis(c["det_boxes"], g[..., None], 1), det_scores=np.take_along_axis(c["det_scores"], g, 1),
             det_labels=np.take_along_axis(c["det_labels"], g, 1), det_count=n.astype(np.int32))
    _result_equal(got, ref.evaluate([k]), "nms -> gather -> update")
