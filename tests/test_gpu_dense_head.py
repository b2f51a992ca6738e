"""GPU parity of the dense head decode (SPEC.md §25) (-m gpu): ops.anchor_decode, ops.center_decode and the decoder modules
against tests/dense_head_ref.py.  Parity rules of §25: cx, cy, cz, yaw (anchor head), vel, raw dims and labels are EQUAL to
the reference under ==; expf outputs and scores are within §9's 1e-4 (absolute + relative) with inf == inf; the centre
head's yaw within 1e-4 after wrapping the difference into [-pi, pi).  Outputs are pre-filled with NaN before every call;
nhwc on the permuted copy of the maps is bit-identical to nchw; a second call is bit-identical to the first; index rows are
bit-identical to the rows of the full decode.  The coverage every case relies on is asserted on the reference in
tests/test_dense_head_cpu.py; nothing is skipped."""
import numpy as np
import pytest

import dense_head_ref as ref

pytestmark = pytest.mark.gpu

F = np.float32
SENTINEL = -77777


def _t(a, dev):
    import torch
    return None if a is None else torch.from_numpy(np.array(a, order="C")).to(dev)       # (a copy: the cases are read-only)


def _poisoned(B, rows, D, dev):
    import torch
    return (torch.full((B, rows, D), float("nan"), dtype=torch.float32, device=dev),
            torch.full((B, rows), float("nan"), dtype=torch.float32, device=dev),
            torch.full((B, rows), SENTINEL, dtype=torch.int32, device=dev))


def _run(c, dev, layout="nchw", index=None):
    """One call into NaN-filled outputs -> numpy (boxes, scores, labels)."""
    from sad_amd import ops
    maps = [_t(m if layout == "nchw" else ref.to_nhwc(m), dev) for m in ref.maps_of(c)]
    B = maps[0].shape[0]
    K = ref.rows_of_case(c) if index is None else index.shape[1]
    D = 9 if c["kind"] == "center" and c["vel"] is not None else 7
    out = _poisoned(B, K, D, dev)
    fn = ops.anchor_decode if c["kind"] == "anchor" else ops.center_decode
    got = fn(*maps, layout=layout, index=_t(index, dev), out=out, **c["kw"])
    assert all(g is o for g, o in zip(got, out))
    return tuple(g.cpu().numpy() for g in got)


def _same_bits(a, b, what):
    for name, x, y in zip(("boxes", "scores", "labels"), a, b):
        assert x.shape == y.shape and x.dtype == y.dtype, (what, name)
        n = int((x.view(np.int32) != y.view(np.int32)).sum())
        assert n == 0, f"{what}: {n} of {x.size} words of {name} differ"


def _near(got, want, what):
    """§9: 1e-4 absolute + relative; infinities must match exactly."""
    inf = np.isinf(want)
    assert np.array_equal(got[inf], want[inf]), f"{what}: infinities differ"
    err = np.abs(got[~inf].astype(np.float64) - want[~inf])
    ok = err <= 1e-4 + 1e-4 * np.abs(want[~inf])
    assert ok.all(), f"{what}: {int((~ok).sum())} of {ok.size} beyond 1e-4, worst {float(err.max()):.3g}"


def _equal(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    bad = ~(got == want)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {want.size} differ under =="


def _parity(got, want, c, what):
    boxes, scores, labels = got
    wb, ws, wl = want
    assert not np.isnan(boxes).any() and not np.isnan(scores).any() and not (labels == SENTINEL).any(), f"{what}: output not fully written"
    _equal(labels, wl, f"{what} labels")
    if c["kind"] == "anchor":
        for j, col in ((0, "cx"), (1, "cy"), (2, "cz"), (6, "yaw")):
            _equal(boxes[..., j], wb[..., j], f"{what} {col}")
        _near(boxes[..., 3:6], wb[..., 3:6], f"{what} l,w,h")
    else:
        for j in (0, 1, 2) + ((7, 8) if boxes.shape[-1] == 9 else ()):
            _equal(boxes[..., j], wb[..., j], f"{what} column {j}")
        if c["kw"]["log_dim"]:
            _near(boxes[..., 3:6], wb[..., 3:6], f"{what} l,w,h")
        else:
            _equal(boxes[..., 3:6], wb[..., 3:6], f"{what} l,w,h (raw)")
        d = boxes[..., 6].astype(np.float64) - wb[..., 6]
        d = (d + np.pi) % (2 * np.pi) - np.pi                     # atan2f(+-0, negative) may land on either side of the cut
        assert (np.abs(d) <= 1e-4 + 1e-4 * np.abs(wb[..., 6])).all(), f"{what} yaw: worst {float(np.abs(d).max()):.3g}"
    _near(scores, ws, f"{what} scores")


@pytest.mark.parametrize("name", ref.ALL_CASES)
def test_decode_parity_layouts_and_determinism(dev, name):
    c = ref.case(name)
    want = ref.expected(name)[:3]
    got = _run(c, dev)
    _parity(got, want, c, name)
    _same_bits(_run(c, dev), got, f"{name}: second call")
    _same_bits(_run(c, dev, layout="nhwc"), got, f"{name}: nhwc against nchw")


@pytest.mark.parametrize("name", ["a:5x7", "a:3x67:128", "a:9x130", "a:edges", "a:3x67:c10", "a:3x67:a9", "a:5x7:a11", "c:5x7", "c:9x130:peak", "c:3x67",
                                  "c:edges:vel"])
def test_index_rows_are_the_rows_of_the_full_decode(dev, name):
    c = ref.case(name)
    full = _run(c, dev)
    K = full[1].shape[1]
    for label, index in ref.index_cases(name).items():
        ok = (index >= 0) & (index < K)
        safe = np.where(ok, index, 0).astype(np.int64)
        bi = np.arange(index.shape[0])[:, None]
        want = (np.where(ok[..., None], full[0][bi, safe], F(0)).astype(F), np.where(ok, full[1][bi, safe], F(-np.inf)).astype(F),
                np.where(ok, full[2][bi, safe], -1).astype(np.int32))
        for layout in ("nchw", "nhwc"):
            got = _run(c, dev, layout=layout, index=index)
            assert not np.isnan(got[0]).any() and not np.isnan(got[1]).any() and not (got[2] == SENTINEL).any()
            _same_bits(got, want, f"{name} index:{label} {layout}")
        _parity(got, ref.decode(c, index=index), c, f"{name} index:{label}")
        if label == "bad":
            assert (~ok).sum() >= 4 and (got[0][~ok] == 0).all() and np.isneginf(got[1][~ok]).all() and (got[2][~ok] == -1).all()


def test_modules_forward_the_operators(dev):
    import torch
    from sad_amd import dense_head, ops
    c = ref.case("a:5x7")
    maps = [_t(m, dev) for m in ref.maps_of(c)]
    kw = c["kw"]
    dec = dense_head.AnchorHeadDecoder(kw["sizes"], kw["z_center"], kw["rotations"], kw["origin"], kw["step"])
    assert dec.num_anchors == 6 and not list(dec.parameters())
    _parity(tuple(t.cpu().numpy() for t in dec(*maps)), ref.expected("a:5x7")[:3], c, "AnchorHeadDecoder")
    idx = _t(ref.index_cases("a:5x7")["dup"], dev)
    for a, b in zip(dec(*maps, index=idx), ops.anchor_decode(*maps, index=idx, **kw)):
        assert torch.equal(a, b)
    c = ref.case("c:5x7")
    maps = [_t(m, dev) for m in ref.maps_of(c)]
    cdec = dense_head.CenterHeadDecoder(**c["kw"])
    _parity(tuple(t.cpu().numpy() for t in cdec(*maps)), ref.expected("c:5x7")[:3], c, "CenterHeadDecoder")
    out = cdec.predict(*maps, iou_thr=0.2, score_thr=0.1, pre_max=20, post_max=10)
    assert out[0].shape == (3, 35, 9) and out[3].shape == (3, 10) and out[4].shape == (3,)


def test_predict_equals_reference_decode_then_reference_nms(dev):
    """AnchorHeadDecoder.predict on the (3,67) map: lattice logits and zero size residuals make the ranking immune to expf,
    so keep / order / count equal tests/nms_ref.py run on the REFERENCE decode, array for array.  (Coverage, asserted in
    test_dense_head_cpu.py::test_coverage_e2e: both caps cut and at least a fifth of the pre-selected boxes are suppressed.)"""
    import nms_ref
    from sad_amd import dense_head
    c = ref.e2e_case()
    kw, nms = c["kw"], ref.E2E_NMS
    rb, rs, rl = ref.decode(c)
    want_keep, want_order, want_count = nms_ref.nms_boxes(rb, rs, rl, nms["iou_thr"], nms["score_thr"], nms["pre_max"], nms["post_max"])
    dec = dense_head.AnchorHeadDecoder(kw["sizes"], kw["z_center"], kw["rotations"], kw["origin"], kw["step"], kw["dir_offset"],
                                       kw["dir_limit_offset"])
    boxes, scores, labels, order, count = dec.predict(*[_t(m, dev) for m in ref.maps_of(c)], **nms)
    _parity((boxes.cpu().numpy(), scores.cpu().numpy(), labels.cpu().numpy()), (rb, rs, rl), c, "e2e decode")
    assert np.array_equal(boxes.cpu().numpy()[..., 3:6], rb[..., 3:6])           # expf(0) = 1 on both sides
    np.testing.assert_array_equal(count.cpu().numpy(), want_count)
    np.testing.assert_array_equal(order.cpu().numpy(), want_order)
    keep = np.zeros_like(want_keep)
    o = order.cpu().numpy()
    for b in range(o.shape[0]):
        keep[b, o[b, :want_count[b]]] = 1
    np.testing.assert_array_equal(keep, want_keep)
    # class-agnostic on the same decode: another result, the reference's
    _, _, _, order2, count2 = dec.predict(*[_t(m, dev) for m in ref.maps_of(c)], class_aware=False, **nms)
    w2 = nms_ref.nms_boxes(rb, rs, None, nms["iou_thr"], nms["score_thr"], nms["pre_max"], nms["post_max"])
    np.testing.assert_array_equal(order2.cpu().numpy(), w2[1])
    np.testing.assert_array_equal(count2.cpu().numpy(), w2[2])
    assert not np.array_equal(w2[1], want_order)
