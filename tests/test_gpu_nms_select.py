"""GPU parity of box selection and NMS at scale (SPEC.md §23, ops.nms_boxes) (-m gpu): keep, order and count equal the numpy
reference (tests/nms_ref.py) array for array; below the old operator's cap they also equal ops.nms_bev and, at any K,
oracle.nms_bev.  Cases and their references are shared with tests/test_nms_select_cpu.py, which checks the reference
against the oracle; each family here first asserts, on the REFERENCE's output, the coverage it exists for."""
import numpy as np
import pytest

import nms_ref as ref

pytestmark = pytest.mark.gpu

F = np.float32


def _t(a, dev):
    import torch
    return None if a is None else torch.from_numpy(np.array(a, order="C")).to(dev)    # (a copy: the cases are read-only)


def _run(sad, dev, boxes, scores, labels, out=None, **kw):
    got = sad.nms_boxes(_t(boxes, dev), _t(scores, dev), _t(labels, dev), out=out, **kw)
    return tuple(g.cpu().numpy() for g in got)


def _same(got, want, what=""):
    for name, g, w in zip(("keep", "order", "count"), got, want):
        assert g.dtype == np.int32 and g.shape == w.shape, f"{what} {name}: {g.dtype} {g.shape} vs {w.shape}"
        np.testing.assert_array_equal(g, w, err_msg=f"{what} {name}")


def _case(sad, dev, name, **override):
    c = ref.case(name)
    kw = dict(c["kw"])
    kw.update(override)
    return _run(sad, dev, c["boxes"], c["scores"], c["labels"], **kw)


@pytest.mark.parametrize("K", ref.IDENTITY_K)
def test_identity_with_nms_bev_and_oracle(sad, orc, dev, K):
    """labels=None, no limits: equal to oracle.nms_bev at every K, and to ops.nms_bev where that operator exists (K <= 512).
    K = 513 is the smallest size the library could not do before."""
    name = f"identity:{K}"
    c = ref.case(name)
    want = orc.nms_bev(c["boxes"], ref.IOU_THR, 0.0)
    if K >= 64:
        assert 0.2 < want[2].sum() / (2 * K) < 0.8                     # coverage: this NMS suppresses
    got = _run(sad, dev, c["boxes"], c["scores"], None, iou_thr=ref.IOU_THR)
    _same(got, want, f"K={K} vs oracle.nms_bev")
    _same(got, ref.expected(name), f"K={K} vs reference")
    if K <= 512:
        old = tuple(g.cpu().numpy() for g in sad.nms_bev(_t(c["boxes"], dev), ref.IOU_THR, 0.0))
        _same(got, old, f"K={K} vs ops.nms_bev")
    col7 = _run(sad, dev, c["boxes"], None, None, iou_thr=ref.IOU_THR)   # scores=None: column 7 of the rows
    _same(col7, want, f"K={K} scores=None")


def test_chains_across_chunks(sad, dev):
    """K = 200 crowded: a box whose only suppressors were themselves suppressed stays; suppression reaches over more than
    one 64-rank chunk."""
    want = ref.expected("chains")
    revived, far = ref.chain_coverage("chains")
    assert revived >= 1 and far >= 1                                      # coverage
    _same(_case(sad, dev, "chains"), want)


def test_ties_and_zeros(sad, dev):
    """Scores from {0.75, 0.5, +0.0, -0.0, -1.0}, score_thr = -0.0: both zeros are candidates and tie; the pre-selection cut
    inside a tie group takes the lowest indices."""
    cuts, inside, in_zero = ref.tie_cuts("ties")
    assert sum(inside) >= 2 and any(in_zero)                              # coverage
    for p in cuts:
        _same(_case(sad, dev, "ties", pre_max=p), ref.expected("ties", pre_max=p), f"pre_max={p}")


def test_post_max(sad, dev):
    kept = int(ref.expected("post")[2][0])
    assert 5 < kept < 595
    for post in (1, kept - 1, kept, kept + 5):
        want = ref.expected("post", post_max=post)
        got = _case(sad, dev, "post", post_max=post)
        assert got[1].shape == (2, min(600, post))
        np.testing.assert_array_equal(got[0].sum(1), got[2])
        assert (got[2] <= post).all()
        _same(got, want, f"post_max={post}")
    np.testing.assert_array_equal(ref.expected("post", post_max=kept - 1)[1][0], ref.expected("post")[1][0, :kept - 1])


def test_select_head_sized(sad, dev):
    """K = 70 400 (SECOND's KITTI grid x 2 anchors), pre_max = 1000 falling inside a group of 2000 equal scores, post_max = 100."""
    c = ref.case("head")
    for b in range(2):
        assert ref.cut_inside_tie(c["scores"][b], c["kw"]["score_thr"], 1000)   # coverage
    want = ref.expected("head")
    assert want[1].shape == (2, 100)
    _same(_case(sad, dev, "head"), want)
    want = ref.expected("head", post_max=None)                                    # the whole pre-selection walked
    assert (want[2] < 900).all() and (want[2] > 100).all()
    _same(_case(sad, dev, "head", post_max=None), want, "no post_max")


def test_select_at_the_cap(sad, dev):
    """K = 65 537, pre_max = 16 384 (the cap): rank, mask and walk at full width; boxes 10 m apart, so all 16 384 are kept."""
    want = ref.expected("cap")
    assert (want[2] == 16384).all() and want[1].shape == (2, 16384)
    _same(_case(sad, dev, "cap"), want)


@pytest.mark.parametrize("which", ["small", "big"])
def test_class_aware(sad, dev, which):
    """Suppression within a class only; any int32 is a class ({-5, 0, 2^30})."""
    name = f"classes:{which}"
    c = ref.case(name)
    want = ref.expected(name)
    agnostic = ref.nms_boxes(c["boxes"], c["scores"], None, **c["kw"])
    assert not np.array_equal(want[0], agnostic[0]) and want[2].sum() / 800 < 0.9      # coverage
    _same(_case(sad, dev, name), want)
    _same(_run(sad, dev, c["boxes"], c["scores"], None, **c["kw"]), agnostic, "class-agnostic")


def test_layout(sad, dev):
    """D = 7 and D = 9 rows give the same result; with D = 9 column 7 holds the scores reversed and is not read."""
    c7, c9 = ref.case("layout:7"), ref.case("layout:9")
    np.testing.assert_array_equal(c7["boxes"], c9["boxes"][..., :7])
    assert not np.array_equal(c9["boxes"][..., 7], c9["scores"])
    want = ref.expected("layout:7")
    other = ref.nms_boxes(c9["boxes"], c9["boxes"][..., 7], None, **c9["kw"])
    assert not np.array_equal(want[1], other[1])                                        # following column 7 would show
    _same(_case(sad, dev, "layout:7"), want, "D=7")
    _same(_case(sad, dev, "layout:9"), want, "D=9")


def test_degenerate(sad, dev):
    rng = np.random.default_rng(9)
    boxes = ref.crowded(rng, 2, 130)
    scores = rng.uniform(0.1, 0.9, (2, 130)).astype(F)
    kw = dict(iou_thr=ref.IOU_THR)
    got = _run(sad, dev, boxes, scores, None, score_thr=0.95, **kw)                     # no candidate
    assert (got[2] == 0).all() and (got[1] == -1).all() and (got[0] == 0).all() and got[1].shape == (2, 130)
    one = scores.copy()
    one[0, 77] = one[1, 3] = 0.99
    got = _run(sad, dev, boxes, one, None, score_thr=0.95, **kw)                        # one candidate
    _same(got, ref.nms_boxes(boxes, one, None, score_thr=0.95, **kw), "one candidate")
    assert got[1][0, 0] == 77 and got[1][1, 0] == 3 and (got[2] == 1).all()
    same = np.repeat(boxes[:, :1], 130, 1)                                              # all boxes identical
    for thr in (0.5, 1.0):
        want = ref.nms_boxes(same, scores, None, iou_thr=thr)
        _same(_run(sad, dev, same, scores, None, iou_thr=thr), want, f"identical boxes, iou_thr={thr}")
    assert (ref.nms_boxes(same, scores, None, iou_thr=0.5)[2] == 1).all()
    flat = boxes.copy()                                                                 # zero-area boxes: den <= 0 -> IoU 0
    flat[..., 3] = 0
    flat[:, ::2, 4] = 0
    want = ref.nms_boxes(flat, scores, None, iou_thr=0.0)
    _same(_run(sad, dev, flat, scores, None, iou_thr=0.0), want, "zero-area boxes")


def test_buffer_reuse_and_determinism(sad, dev):
    """out= buffers reused on inputs A, B, A with different candidate counts: nothing of an earlier call is left; two plain
    calls are bit-equal."""
    rng = np.random.default_rng(10)
    K = 700
    boxes = ref.crowded(rng, 2, K)
    sa = rng.uniform(0.0, 1.0, (2, K)).astype(F)
    sb = (sa * F(0.3)).astype(F)
    kw = dict(iou_thr=ref.IOU_THR, score_thr=0.25, pre_max=400, post_max=300)
    wa, wb = ref.nms_boxes(boxes, sa, None, **kw), ref.nms_boxes(boxes, sb, None, **kw)
    assert wa[2].min() > wb[2].max() + 50 > 50                                          # B leaves far fewer boxes than A
    buf = sad.nms_boxes_buffers(2, K, dev, pre_max=400, post_max=300)
    for s, w, tag in ((sa, wa, "A"), (sb, wb, "B"), (sa, wa, "A again")):
        got = _run(sad, dev, boxes, s, None, out=buf, **kw)
        _same(got, w, tag)
    _same(_run(sad, dev, boxes, sa, None, **kw), _run(sad, dev, boxes, sa, None, **kw), "two plain calls")
    import torch
    with pytest.raises(RuntimeError):
        sad.nms_boxes(torch.zeros((1, 4, 7)), torch.zeros((1, 4)), None, 0.5)      # CPU tensors


def test_refusals_through_the_c_abi(sad):
    """Host-side checks only (nothing is launched, the pointers are never dereferenced)."""
    from sad_amd import _lib
    L = _lib.lib()
    p = 0x10000
    assert L.sad_nms_boxes_f32(p, 7, p, None, 1, 20000, 0.5, 0.0, 16385, 100, p, p, p, p, None) == -2
    assert b"16385" in L.sad_last_error()
    assert L.sad_nms_boxes_f32(p, 7, p, None, 1, 16385, 0.5, 0.0, 16385, 100, p, p, p, p, None) == -2
    assert L.sad_nms_boxes_workspace_bytes(1, 20000, 16385) == 0
    assert L.sad_nms_boxes_workspace_bytes(1, 20000, 16384) > 0
    assert L.sad_nms_boxes_workspace_bytes(1, 513, 513) > 0
    assert L.sad_nms_boxes_f32(p, 7, p, None, 1, 100, 0.5, 0.0, 0, 100, p, p, p, p, None) == -1     # pre_max = 0
    assert L.sad_nms_boxes_f32(p, 7, p, None, 1, 100, 0.5, 0.0, 100, 0, p, p, p, p, None) == -1     # post_max = 0
    assert L.sad_nms_boxes_f32(p, 7, None, None, 1, 100, 0.5, 0.0, 100, 100, p, p, p, p, None) == -1  # NULL scores
    assert b"NULL" in L.sad_last_error()
    assert L.sad_nms_boxes_f32(p, 6, p, None, 1, 100, 0.5, 0.0, 100, 100, p, p, p, p, None) == -1   # D < 7
    assert L.sad_nms_boxes_workspace_bytes(0, 100, 100) == 0 and L.sad_nms_boxes_workspace_bytes(65536, 100, 100) == 0
    assert L.sad_nms_boxes_workspace_bytes(65535, 40000, 100) == 0                                  # B*K >= 2^31


def test_null_labels_accepted(sad, dev):
    """The C entry point with labels = NULL runs (class-agnostic); with labels it is class-aware (test_class_aware)."""
    import torch
    from sad_amd import _lib
    c = ref.case("layout:7")
    B, K = c["scores"].shape
    boxes, scores = _t(c["boxes"], dev), _t(c["scores"], dev)
    keep, order, count, ws = sad.nms_boxes_buffers(B, K, dev)
    rc = _lib.lib().sad_nms_boxes_f32(boxes.data_ptr(), 7, scores.data_ptr(), None, B, K, ref.IOU_THR, 0.0, K, K, keep.data_ptr(),
                                      order.data_ptr(), count.data_ptr(), ws.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    _same((keep.cpu().numpy(), order.cpu().numpy(), count.cpu().numpy()), ref.expected("layout:7"))


# ---- score regimes: selection over the whole float32 score line (small crowded scenes, so the NMS behind it shows) -----
def test_scores_logits(sad, dev):
    """All scores negative and distinct, pre_max cutting inside them: the negative branch of the key orders by value."""
    print(ref.cover_logits())                                                        # coverage
    _same(_case(sad, dev, "logits"), ref.expected("logits"))
    _same(_case(sad, dev, "logits", score_thr=-3.5, pre_max=None), ref.expected("logits", score_thr=-3.5, pre_max=None), "thr")


def test_scores_mixed(sad, dev):
    """Both signs and a block of +0.0 / -0.0: the cut among the positives, inside the zeros, among the negatives."""
    print(ref.cover_mixed())                                                         # coverage
    for p in ref.MIXED_CUTS:
        _same(_case(sad, dev, "mixed", pre_max=p), ref.expected("mixed", pre_max=p), f"pre_max={p}")


def test_scores_wide(sad, dev):
    """Every exponent in both signs, subnormals, +-FLT_MAX, FLT_MIN, +-Inf (ordinary scores): >= 200 top digits in use."""
    print(ref.cover_wide())                                                          # coverage
    for p in ref.wide_cuts():
        _same(_case(sad, dev, "wide", pre_max=p), ref.expected("wide", pre_max=p), f"pre_max={p}")


@pytest.mark.parametrize("q", sorted(ref.LADDER))
def test_scores_ladder(sad, dev, q):
    """Consecutive floats across the carry into radix digit q, positive (scene 0) and negative (scene 1): pass q is the
    first that separates the threshold from its neighbours; threshold keys end in 0x00 and 0xFF digits."""
    print(ref.cover_ladder())                                                        # coverage
    name = f"ladder:{q}"
    for p in ref.ladder_cuts(name):
        _same(_case(sad, dev, name, pre_max=p), ref.expected(name, pre_max=p), f"{name} pre_max={p}")


@pytest.mark.parametrize("pattern", ref.RUNS)
def test_scores_runs(sad, dev, pattern):
    """All equal / ascending / descending / two values alternating, K = 1500, pre_max = 700: one run per thread, or none."""
    print(ref.cover_runs())                                                          # coverage
    got = _case(sad, dev, f"runs:{pattern}")
    _same(got, ref.expected(f"runs:{pattern}"), pattern)
    if pattern == "equal":
        assert got[1].max() < 700                                                    # the lowest 700 indices went on


@pytest.mark.parametrize("pre_max", [None, 300])
def test_score_thresholds(sad, dev, pre_max):
    """score_thr above / at the maximum, at and one ulp either side of the 300-th score, negative, -Inf, +Inf with a +Inf
    score present (scene 1), +0.0 with -0.0 scores present."""
    print(ref.cover_thresholds())                                                    # coverage
    for tag, thr in ref.threshold_values():
        want = ref.expected("thresholds", score_thr=float(thr), pre_max=pre_max)
        _same(_case(sad, dev, "thresholds", score_thr=float(thr), pre_max=pre_max), want, tag)


# ---- stage boundaries ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", ref.STRIDE_K)
def test_select_strides(sad, dev, K):
    """K at the strides of the two select kernels (256, 1024) and at the switch between them (4096); no limits."""
    name = f"stride:{K}"
    assert ref.selected_n(ref.case(name)["scores"][0], 0.0) == K and 0.2 < ref.kept_fraction(name) < 0.8     # coverage
    _same(_case(sad, dev, name), ref.expected(name), name)


def test_selected_count_boundaries(sad, dev):
    """K = 5000, n at the rows-per-workgroup (16), chunk (64, 128), select-stride (256), rank-tile (2048) boundaries and
    at 4096: once through pre_max (P = n) and once through score_thr (P = K, so surplus workgroups exit on n)."""
    print(ref.cover_stages())                                                        # coverage
    for n, thr in zip(ref.N5000, ref.n5000_thresholds()):
        _same(_case(sad, dev, "n5000", pre_max=n), ref.expected("n5000", pre_max=n), f"pre_max={n}")
        _same(_case(sad, dev, "n5000", score_thr=thr), ref.expected("n5000", score_thr=thr), f"n={n} by score_thr")
    _same(_case(sad, dev, "n5000", pre_max=1), ref.expected("n5000", pre_max=1), "pre_max=1")
    _same(_case(sad, dev, "n5000", post_max=1), ref.expected("n5000", post_max=1), "post_max=1")


def test_post_cap_at_a_chunk_end(sad, dev):
    """post_max reached exactly on the last rank of a 64-rank chunk, and on the first rank of a chunk."""
    print(ref.cover_post_chunk())                                                    # coverage
    for post in ref.post_chunk_cuts():
        _same(_case(sad, dev, "post", post_max=post), ref.expected("post", post_max=post), f"post_max={post}")


def test_batch_of_37_on_a_dirty_workspace(sad, dev):
    """B = 37 in one launch, n = 0, 1, 17, 64, 65, 300 and P = 400 mixed over the scenes; every out= buffer filled with
    0xFF bytes before the first call and with 0xA5 before the second."""
    import torch
    print(ref.cover_stages()["batch37_n"])                                           # coverage
    c, want = ref.case("batch37"), ref.expected("batch37")
    buf = sad.nms_boxes_buffers(37, 600, dev, pre_max=400)
    for fill in (0xFF, 0xA5):
        for t in buf:
            t.view(torch.uint8).fill_(fill)
        _same(_run(sad, dev, c["boxes"], c["scores"], None, out=buf, **c["kw"]), want, f"workspace filled with {fill:#x}")


# ---- the walk at full reach ----------------------------------------------------------------------------------------------
def test_walk_far(sad, dev):
    """K = n = 16 384: copies planted 1 .. 16 000 ranks below their originals are suppressed from up to 250 chunks away;
    a box whose only suppressor was itself suppressed 17 chunks earlier is kept."""
    print(ref.cover_far())                                                           # coverage
    _same(_case(sad, dev, "far"), ref.expected("far"))


@pytest.mark.parametrize("name", ["crowded4k", "crowded4k:classes"])
def test_walk_crowded_4096(sad, dev, name):
    """K = n = 4096 crowded: suppression is dense across all 64 chunks, class-agnostic and with 3 labels."""
    print(ref.cover_crowded4k())                                                     # coverage
    _same(_case(sad, dev, name), ref.expected(name), name)
