"""Every refusal of detection evaluation's host code (SPEC.md §36), none of which needs a GPU.

The C entry points sad_det_match_f32, sad_det_ap_keys_f32 and sad_det_ap_f32: argument blocks hold fake non-null device pointers,
nothing is dereferenced, every case is refused before a launch: SAD_EUNSUPPORTED (-2) above the limits and only there,
SAD_EINVAL (-1) for the rest.

The operators ops.det_match / ops.det_ap and evaluate.DetectionEval: a wrong dtype, shape or stride and scalars out of range are
judged before any device, so CPU tensors reach them; a CPU tensor that is otherwise right is refused as such."""
import ctypes

import pytest

P = 0x10000                                           # a fake device pointer
NAN = float("nan")

MATCH = dict(det_boxes=P, det_scores=P, det_labels=P, det_count=P, gt_boxes=P, gt_labels=P, gt_ignore=P, thr=P, B=2, K=50, D=7, G=9, Dg=8,
             C=3, T=2, metric=1, code=P, match=P, value=P, gt_det=P, n_gt=P)
MATCH_CASES = [(f, {f: None}, -1) for f in ("det_boxes", "det_scores", "det_labels", "thr", "code", "match", "value", "n_gt", "gt_boxes",
                                             "gt_labels", "gt_det")] + [
    ("struct_size", dict(struct_size=-8), -1), ("B=0", dict(B=0), -1), ("K=0", dict(K=0), -1), ("G=-1", dict(G=-1), -1), ("D=6", dict(D=6), -1),
    ("Dg=6", dict(Dg=6), -1), ("C=0", dict(C=0), -1), ("T=0", dict(T=0), -1), ("metric=3", dict(metric=3), -1), ("metric=-1", dict(metric=-1), -1),
    ("K=1025", dict(K=1025), -2), ("G=1025", dict(G=1025), -2), ("C=65", dict(C=65), -2), ("T=9", dict(T=9), -2), ("B=65536", dict(B=65536), -2),
    ("D=6+K=1025", dict(D=6, K=1025), -1)]
AP = dict(keys=P, perm=P, code=P, n_gt=P, N=100, C=3, T=2, points=40, first=1, floor=0.0, ap=P, prec=P, max_recall=P, n_det=P)
AP_CASES = [(f, {f: None}, -1) for f in ("keys", "perm", "code", "n_gt", "ap", "prec", "max_recall", "n_det")] + [
    ("struct_size", dict(struct_size=8), -1), ("N=-1", dict(N=-1), -1), ("C=0", dict(C=0), -1), ("T=0", dict(T=0), -1),
    ("points=0", dict(points=0), -1), ("first=-1", dict(first=-1), -1), ("first>points", dict(first=41), -1), ("floor=1", dict(floor=1.0), -1),
    ("floor=1.5", dict(floor=1.5), -1), ("floor<0", dict(floor=-0.1), -1), ("floor nan", dict(floor=NAN), -1),
    ("points=129", dict(points=129), -2), ("C=65", dict(C=65), -2), ("T=9", dict(T=9), -2), ("N*T=2^31", dict(N=1 << 30, T=2), -2)]


def _block(cls, base, ov):
    f = dict(base, **ov)
    a = cls()
    a.struct_size = ctypes.sizeof(cls) + f.pop("struct_size", 0)
    for k, v in f.items():
        setattr(a, k, v)
    return a


def test_the_library_refuses_on_the_host(sad):
    from sad_amd import _lib
    L = _lib.lib()
    for cls, fn, base, cases in ((_lib.DetMatchArgs, L.sad_det_match_f32, MATCH, MATCH_CASES), (_lib.DetApArgs, L.sad_det_ap_f32, AP, AP_CASES)):
        assert fn(None, None) == -1 and b"NULL" in L.sad_last_error()
        for name, ov, want in cases:
            code = fn(ctypes.byref(_block(cls, base, ov)), None)
            assert code == want and L.sad_last_error(), f"{fn.__name__} {name}: returned {code}, expected {want}"
    a = _block(_lib.DetMatchArgs, MATCH, dict(struct_size=-8))
    assert L.sad_det_match_f32(ctypes.byref(a), None) == -1 and b"struct_size" in L.sad_last_error()
    # G = 0 comes with NULL ground truth: not refused for that (the fake pointers are never launched on: K = 0 stops it)
    a = _block(_lib.DetMatchArgs, MATCH, dict(G=0, gt_boxes=None, gt_labels=None, gt_ignore=None, gt_det=None, K=0))
    assert L.sad_det_match_f32(ctypes.byref(a), None) == -1 and b"K" in L.sad_last_error()
    for args, want in (((None, P, 10, 3, P), -1), ((P, None, 10, 3, P), -1), ((P, P, 10, 3, None), -1), ((P, P, -1, 3, P), -1),
                       ((P, P, 10, 0, P), -1), ((P, P, 10, 65, P), -2), ((P, P, 1 << 31, 3, P), -2)):
        assert L.sad_det_ap_keys_f32(*args, None) == want, args
    assert L.sad_det_ap_keys_f32(None, None, 0, 3, None, None) == 0          # no rows: nothing to do


def _match_inputs(B=2, K=9, D=7, G=3, C=3, T=2):
    import torch
    i32 = torch.int32
    return [torch.zeros(B, K, D), torch.zeros(B, K), torch.zeros(B, K, dtype=i32), torch.zeros(B, dtype=i32), torch.zeros(B, G, 7),
            torch.zeros(B, G, dtype=i32), torch.zeros(B, G, dtype=i32), torch.zeros(C, T)]


def test_det_match_argument_errors(sad):
    import torch
    from sad_amd import ops
    i32, i64 = torch.int32, torch.int64

    def call(i=None, t=None, **kw):
        a = _match_inputs()
        if i is not None:
            a[i] = t
        return ops.det_match(*a, **kw)

    for i, t in ((0, torch.zeros(2, 9, 7, dtype=torch.float64)), (1, torch.zeros(2, 9, dtype=torch.float16)), (2, torch.zeros(2, 9, dtype=i64)),
                 (3, torch.zeros(2, dtype=i64)), (4, torch.zeros(2, 3, 7, dtype=torch.float64)), (5, torch.zeros(2, 3)),
                 (6, torch.zeros(2, 3, dtype=torch.bool)), (7, torch.zeros(3, 2, dtype=torch.float64)), (0, None), (7, [[0.5, 0.25]] * 3)):
        with pytest.raises(TypeError):
            call(i, t)
    for i, t in ((0, torch.zeros(2, 9, 6)), (0, torch.zeros(18, 7)), (0, torch.zeros(2, 1025, 7)), (0, torch.zeros(2, 0, 7)),
                 (1, torch.zeros(2, 8)), (2, torch.zeros(3, 9, dtype=i32)), (3, torch.zeros(3, dtype=i32)), (4, torch.zeros(2, 3, 6)),
                 (4, torch.zeros(3, 3, 7)), (4, torch.zeros(2, 1025, 7)), (5, torch.zeros(2, 4, dtype=i32)), (6, torch.zeros(2, 4, dtype=i32)),
                 (7, torch.zeros(3, 9)), (7, torch.zeros(0, 2)), (7, torch.zeros(65, 2)), (7, torch.zeros(3, 0)), (7, torch.zeros(6)),
                 (0, torch.zeros(2, 9, 14)[..., ::2]), (1, torch.zeros(9, 2).t()), (7, torch.zeros(2, 3).t())):
        with pytest.raises(ValueError):
            call(i, t)
    with pytest.raises(ValueError, match="metric"):
        call(metric="iou")
    # everything right but the device
    for kw in (dict(), dict(metric="dist"), dict(metric="iou_bev")):
        with pytest.raises(RuntimeError, match="no CPU path"):
            call(**kw)
    with pytest.raises(RuntimeError, match="no CPU path"):
        a = _match_inputs()
        ops.det_match(a[0], a[1], a[2], None, torch.zeros(2, 0, 7), torch.zeros(2, 0, dtype=i32), None, a[7])


def test_det_ap_argument_errors(sad):
    import torch
    from sad_amd import ops
    i32 = torch.int32

    def call(i=None, t=None, **kw):
        a = [torch.zeros(50), torch.zeros(50, dtype=i32), torch.zeros(50, 2, dtype=i32), torch.ones(3, dtype=i32)]
        if i is not None:
            a[i] = t
        return ops.det_ap(*a, **kw)

    for i, t in ((0, torch.zeros(50, dtype=torch.float64)), (1, torch.zeros(50, dtype=torch.int64)), (2, torch.zeros(50, 2)),
                 (3, torch.ones(3, dtype=torch.int64)), (0, None)):
        with pytest.raises(TypeError):
            call(i, t)
    for i, t in ((0, torch.zeros(50, 1)), (1, torch.zeros(49, dtype=i32)), (2, torch.zeros(49, 2, dtype=i32)), (2, torch.zeros(50, 9, dtype=i32)),
                 (2, torch.zeros(50, 0, dtype=i32)), (2, torch.zeros(100, dtype=i32)), (3, torch.ones(0, dtype=i32)), (3, torch.ones(65, dtype=i32)),
                 (3, torch.ones(3, 1, dtype=i32)), (2, torch.zeros(2, 50, dtype=i32).t()), (0, torch.zeros(100)[::2])):
        with pytest.raises(ValueError):
            call(i, t)
    for kw in (dict(points=129), dict(points=0), dict(first=41), dict(first=-1), dict(points=10, first=11), dict(floor=1.0), dict(floor=1.5),
               dict(floor=-0.1), dict(floor=NAN)):
        with pytest.raises(ValueError):
            call(**kw)
    for kw in (dict(), dict(points=10, first=0), dict(points=100, first=11, floor=0.1), dict(points=128, first=128, floor=0.999)):
        with pytest.raises(RuntimeError, match="no CPU path"):
            call(**kw)


def test_out_and_workspace_checks(sad):
    """The two checkers det_match and det_ap hand their `out=` tuples and the workspace to, on the operators' own specs."""
    import torch
    from sad_amd import ops
    cpu = torch.device("cpu")
    for spec, names in ((ops.det_match_output_spec(2, 9, 3, 3, 2), ops.DET_MATCH_OUTPUTS), (ops.det_ap_output_spec(3, 2, 40, 1), ops.DET_AP_OUTPUTS)):
        assert tuple(n for n, _, _ in spec) == names
        good = tuple(torch.zeros(shape, dtype=dt) for _, shape, dt in spec)
        assert ops._outputs(spec, good, cpu, "x") == good
        for bad in (good[:-1], good[1:] + good[:1], tuple(t.to(torch.float64) for t in good), list(good)[:2]):
            with pytest.raises(ValueError, match="out: expected contiguous"):
                ops._outputs(spec, bad, cpu, "x")
    assert ops.det_ap_output_spec(3, 2, 100, 11)[1][1] == (3, 2, 90)
    with pytest.raises(ValueError, match="at least 400 bytes"):
        ops._workspace(400, torch.zeros(399, dtype=torch.uint8), cpu, "ops.det_ap_workspace", 8)


def test_detection_eval_refusals(sad):
    import torch
    from sad_amd.evaluate import DetectionEval
    for kw in (dict(num_classes=0), dict(num_classes=65), dict(thr=[[0.5], [0.5]]), dict(thr=[0.5] * 9), dict(thr=[]), dict(metric="iou"),
               dict(points=129), dict(points=0), dict(first=41), dict(first=-1), dict(floor=1.0), dict(floor=-0.5), dict(capacity=0),
               dict(capacity=1 << 30, thr=[0.5, 0.25])):
        with pytest.raises(ValueError):
            DetectionEval(**dict(dict(num_classes=3, thr=[0.7, 0.5]), **kw))
    ev = DetectionEval(3, [0.7, 0.5], "iou3d", 40, 1, 0.0, 20)
    assert (ev.C, ev.T, ev.capacity, ev.rows) == (3, 2, 20, 0) and ev.thr_host.shape == (3, 2)
    assert DetectionEval(2, 0.5).thr_host.tolist() == [[0.5], [0.5]]
    a = _match_inputs()[:7]
    with pytest.raises(RuntimeError, match="no CPU path"):                 # 18 rows fit: the device is judged
        ev.update(*a)
    with pytest.raises(RuntimeError, match="capacity 20 exceeded"):        # 2 x 11 rows do not: judged before anything else
        ev.update(*_match_inputs(K=11)[:7])
    with pytest.raises(RuntimeError, match="nothing was accumulated"):
        ev.compute()
    other = DetectionEval(3, [0.7, 0.25], "iou3d", 40, 1, 0.0, 20)
    with pytest.raises(ValueError, match="configuration"):
        ev.merge(other)
    other = DetectionEval(3, [0.7, 0.5], "iou3d", 40, 1, 0.0, 20)
    other.rows = 21                                                        # (as if it held more than this one can take)
    with pytest.raises(RuntimeError, match="capacity"):
        ev.merge(other)
