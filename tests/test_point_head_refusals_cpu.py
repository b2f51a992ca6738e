"""Every refusal of the point head's host code (SPEC.md §31), none of which needs a GPU.

The C entry points sad_point_targets_f32 and sad_point_head_loss_f32: argument blocks hold fake non-null device pointers, nothing is
dereferenced, every case is refused before the launch with the code §31 names (SAD_EINVAL -1, SAD_EUNSUPPORTED -2 above a cap)
and a message that names the cause.

The operators ops.point_targets / ops.point_head_loss: a wrong dtype, rank, shape or stride and scalars out of range are judged
before any device, so CPU tensors reach them; CPU tensors that are otherwise right are refused as such; the `out=` check is run
against the checker and the spec the operators use, with a CPU device standing in.  The module's view rules are checked the
same way."""
import ctypes

import pytest

P = 0x10000                                           # a fake device pointer
NAN = float("nan")

T_BASE = dict(xyz=P, cand=P, gt_boxes=P, gt_labels=P, B=2, M=300, G=5, D=7, C=3, shift_max=2.0, extra_width=0.2,
              labels=P, match=P, centerness=P, shift_target=P, size_target=P, reg_target=P)
L_BASE = dict(o=P, c=P, labels=P, centerness=P, reg_target=P, shift_target=P, size_target=P, B=2, M=300, C=3, cls_loss=0, normalize=1,
              alpha=0.25, beta=0.125, shift_max=2.0, loss=P, num_pos=P, grad_o=P, grad_c=P, per_point=P, workspace=P)
NO_C = dict(c=None, shift_target=None, size_target=None, grad_c=None)

#            name, overrides, code, a word of the message
T_CASES = [("struct_size", dict(struct_size=-8), -1, "struct_size"), ("struct_size+G", dict(struct_size=8, G=2000), -1, "struct_size")] + [
    (f, {f: None}, -1, "NULL") for f in ("xyz", "labels", "match", "centerness", "shift_target", "size_target", "reg_target", "gt_boxes", "gt_labels")] + [
    ("B=0", dict(B=0), -1, "B, M, C"), ("M=0", dict(M=0), -1, "B, M, C"), ("C=0", dict(C=0), -1, "B, M, C"), ("G=-1", dict(G=-1), -1, "G >= 0"),
    ("D=6", dict(D=6), -1, "D = 6"), ("anchor", dict(anchor=0.0), -1, "anchor"), ("size_anchor", dict(size_anchor=-1.0), -1, "size_anchor"),
    ("shift_max", dict(shift_max=-1.0), -1, "shift_max"), ("extra_width", dict(extra_width=NAN), -1, "extra_width"),
    ("C=17", dict(C=17), -2, "C = 17"), ("B=65536", dict(B=65536), -2, "65536"), ("G=1025", dict(G=1025), -2, "1025"),
    ("rows", dict(B=65535, M=40000), -2, "2^31")]
L_CASES = [("struct_size", dict(struct_size=-8), -1, "struct_size"), ("struct_size+C", dict(struct_size=8, C=17), -1, "struct_size")] + [
    (f, {f: None}, -1, "NULL") for f in ("o", "labels", "reg_target", "loss", "num_pos", "grad_o", "workspace")] + [
    ("targets without c", dict(c=None, grad_c=None), -1, "without c"), ("shift without c", dict(NO_C, shift_target=P), -1, "without c"),
    ("c without targets", dict(shift_target=None, size_target=None), -1, "without shift_target"),
    ("grad_c missing", dict(grad_c=None), -1, "grad_c"), ("grad_c without c", dict(NO_C, grad_c=P), -1, "grad_c"),
    ("cls_loss", dict(cls_loss=2), -1, "cls_loss"), ("beta=0", dict(beta=0.0), -1, "beta"), ("beta=-1", dict(beta=-1.0), -1, "beta"),
    ("beta nan", dict(beta=NAN), -1, "beta"), ("alpha", dict(alpha=1.5), -1, "alpha"), ("shift_max", dict(shift_max=-1.0), -1, "shift_max"),
    ("B=0", dict(B=0), -1, "B, M, C"), ("M=0", dict(M=0), -1, "B, M, C"), ("C=0", dict(C=0), -1, "B, M, C"),
    ("C=17", dict(C=17), -2, "C = 17"), ("B=65536", dict(B=65536), -2, "65536"), ("rows", dict(B=65535, M=40000), -2, "2^31"),
    ("C=17 no c", dict(NO_C, C=17), -2, "C = 17")]


def _block(cls, base, ov):
    f = dict(base, **ov)
    a = cls()
    a.struct_size = ctypes.sizeof(cls) + f.pop("struct_size", 0)
    anchor, size_anchor = f.pop("anchor", 1.5), f.pop("size_anchor", 2.0)
    if hasattr(a, "anchors"):
        a.anchors[:] = [1.0] * 47 + [anchor] if f["C"] > 16 else [1.0] * (3 * max(f["C"], 1) - 1) + [anchor] + [0.0] * (48 - 3 * max(f["C"], 1))
        a.size_anchor[:] = [1.0, size_anchor, 1.0]
    else:
        a.code_weights[:], a.scale[:] = [1.0] * 7, [1.0] * 4
    for k, v in f.items():
        setattr(a, k, v)
    return a


@pytest.mark.parametrize("which", ("targets", "loss"))
def test_c_entry_points_refuse_on_the_host(sad, which):
    from sad_amd import _lib
    L = _lib.lib()
    cls, fn, base, cases = ((_lib.PointTargetsArgs, L.sad_point_targets_f32, T_BASE, T_CASES) if which == "targets" else
                            (_lib.PointHeadLossArgs, L.sad_point_head_loss_f32, L_BASE, L_CASES))
    assert fn(None, None) == -1 and b"NULL args" in L.sad_last_error()
    assert len({n for n, *_ in cases}) == len(cases)
    for name, ov, code, word in cases:
        got = fn(ctypes.byref(_block(cls, base, ov)), None)
        msg = L.sad_last_error().decode()
        assert got == code and word in msg and msg.startswith(f"sad_point_{'targets' if which == 'targets' else 'head_loss'}_f32: "), (name, got, msg)
    # a right-sized block with everything NULL is refused for its pointers, not for its size
    a = cls()
    a.struct_size = ctypes.sizeof(cls)
    assert fn(ctypes.byref(a), None) == -1 and b"NULL pointer" in L.sad_last_error()
    # G = 0: the ground-truth pointers may be NULL; the call then fails on the next check, not on them
    if which == "targets":
        got = fn(ctypes.byref(_block(cls, base, dict(G=0, gt_boxes=None, gt_labels=None, C=17))), None)
        assert got == -2 and b"C = 17" in L.sad_last_error()


def test_workspace_size(sad):
    from sad_amd import _lib
    L = _lib.lib()
    assert L.sad_point_head_loss_workspace_bytes(32, 256) == 16 * 32 and L.sad_point_head_loss_workspace_bytes(3, 257) == 16 * 3 * 2
    assert L.sad_point_head_loss_workspace_bytes(1, 1) == 16 and L.sad_point_head_loss_workspace_bytes(32, 16384) == 16 * 32 * 64
    for B, M in ((0, 8), (8, 0), (65536, 8), (65535, 40000), (-1, -1)):
        assert L.sad_point_head_loss_workspace_bytes(B, M) == 0


# ---- the operators ----------------------------------------------------------------------------------------------------------
ANCHORS = ((3.9, 1.6, 1.56), (0.8, 0.6, 1.73), (1.76, 0.6, 1.73))
TKW = dict(anchors=ANCHORS, size_anchor=ANCHORS[0], shift_max=2.0)


def _target_inputs(B=2, M=8, G=4, D=7):
    import torch
    return [torch.zeros(B, M, 3), torch.zeros(B, M, 3), torch.zeros(B, G, D), torch.zeros(B, G, dtype=torch.int32)]


def _loss_inputs(B=2, M=8, C=3):
    import torch
    return [torch.zeros(B, M, C + 7), torch.zeros(B, M, 6), torch.zeros(B, M, dtype=torch.int32), torch.zeros(B, M), torch.zeros(B, M, 7),
            torch.zeros(B, M, 3), torch.zeros(B, M, 3)]


def _put(i, t):
    return lambda a: a.__setitem__(i, t)


def test_point_targets_argument_errors(sad):
    import torch
    from sad_amd import ops

    def call(change=None, **kw):
        a = _target_inputs()
        if change:
            change(a)
        return ops.point_targets(*a, **dict(TKW, **kw))

    for i, t in ((0, torch.zeros(2, 8, 3, dtype=torch.float64)), (1, torch.zeros(2, 8, 3, dtype=torch.float16)), (2, torch.zeros(2, 4, 7, dtype=torch.float64)),
                 (3, torch.zeros(2, 4, dtype=torch.int64)), (3, torch.zeros(2, 4)), (0, None)):
        with pytest.raises(TypeError):
            call(_put(i, t))
    for i, t in ((0, torch.zeros(2, 8, 4)), (0, torch.zeros(16, 3)), (0, torch.zeros(2, 0, 3)), (1, torch.zeros(2, 9, 3)), (1, torch.zeros(3, 8, 3)),
                 (2, torch.zeros(2, 4, 6)), (2, torch.zeros(3, 4, 7)), (2, torch.zeros(2, 1025, 7)), (3, torch.zeros(2, 5, dtype=torch.int32)),
                 (0, torch.zeros(2, 8, 6)[..., ::2]), (2, torch.zeros(2, 7, 4).transpose(1, 2))):
        with pytest.raises(ValueError):
            call(_put(i, t))
    for kw in (dict(anchors=[(1.0, 1.0, 1.0)] * 17), dict(anchors=[]), dict(anchors=[(1.0, 1.0)]), dict(anchors=[(1.0, 0.0, 1.0)]),
               dict(size_anchor=(1.0, 1.0)), dict(size_anchor=(1.0, -1.0, 1.0)), dict(shift_max=-1.0), dict(extra_width=-0.1), dict(extra_width=NAN)):
        with pytest.raises(ValueError):
            call(**kw)
    # everything right but the device: with and without candidates, without boxes, rows of D = 9
    with pytest.raises(RuntimeError, match="no CPU path"):
        call()
    with pytest.raises(RuntimeError, match="no CPU path"):
        call(_put(1, None))
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.point_targets(*_target_inputs(G=0, D=9), **TKW)


def test_point_head_loss_argument_errors(sad):
    import torch
    from sad_amd import ops

    def call(change=None, **kw):
        a = _loss_inputs()
        if change:
            change(a)
        return ops.point_head_loss(*a, **dict(dict(shift_max=2.0), **kw))

    for i, t in ((0, torch.zeros(2, 8, 10, dtype=torch.float64)), (1, torch.zeros(2, 8, 6, dtype=torch.float16)), (2, torch.zeros(2, 8)),
                 (2, torch.zeros(2, 8, dtype=torch.int64)), (3, torch.zeros(2, 8, dtype=torch.float64)), (4, torch.zeros(2, 8, 7, dtype=torch.int32)),
                 (5, torch.zeros(2, 8, 3, dtype=torch.float64)), (6, torch.zeros(2, 8, 3, dtype=torch.int32)), (0, None), (2, None), (4, None)):
        with pytest.raises(TypeError):
            call(_put(i, t))
    for i, t in ((0, torch.zeros(2, 8, 7)), (0, torch.zeros(2, 8, 24)), (0, torch.zeros(16, 10)), (0, torch.zeros(2, 0, 10)), (1, torch.zeros(2, 8, 7)),
                 (1, torch.zeros(16, 6)), (2, torch.zeros(2, 9, dtype=torch.int32)), (3, torch.zeros(2, 8, 1)), (4, torch.zeros(2, 8, 6)),
                 (5, torch.zeros(2, 8, 4)), (6, torch.zeros(3, 8, 3)),
                 (0, torch.zeros(2, 8, 20)[..., ::2]), (1, torch.zeros(2, 6, 8).transpose(1, 2)), (2, torch.zeros(8, 2, dtype=torch.int32).t())):
        with pytest.raises(ValueError):
            call(_put(i, t))
    # c without a target, a target without c
    with pytest.raises(ValueError, match="c needs"):
        ops.point_head_loss(*_loss_inputs()[:5], shift_max=2.0)
    for keep in (5, 6):
        a = _loss_inputs()
        a[1] = None
        a[11 - keep] = None
        with pytest.raises(ValueError, match="need c"):
            ops.point_head_loss(*a, shift_max=2.0)
    for kw in (dict(beta=0.0), dict(beta=-1.0), dict(beta=NAN), dict(beta=1e-60), dict(alpha=-0.1), dict(alpha=1.1), dict(cls_loss="ce"),
               dict(code_weights=[1.0] * 6), dict(scale=(1.0, 1.0, 1.0)), dict(shift_max=None), dict(shift_max=-1.0)):
        with pytest.raises(ValueError):
            call(**kw)
    # everything right but the device: the full call, without c, with one target, without the centre-ness, one class
    with pytest.raises(RuntimeError, match="no CPU path"):
        call()
    a = _loss_inputs()
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.point_head_loss(a[0], None, a[2], None, a[4], cls_loss="focal")
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.point_head_loss(*a[:5], None, a[6], per_point=True)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.point_head_loss(*_loss_inputs(C=1), shift_max=2.0)


def test_out_checks(sad):
    """The checker the two operators hand their `out=` tuple to, on the operators' own specs."""
    import torch
    from sad_amd import ops
    B, M, C = 2, 8, 3
    cpu = torch.device("cpu")
    assert tuple(n for n, _, _ in ops.point_output_spec(B, M)) == ops.POINT_OUTPUTS
    assert [n for n, _, _ in ops.point_loss_output_spec(B, M, C, True, True)] == ["loss", "num_pos", "grad_o", "grad_c", "per_point"]
    assert [n for n, _, _ in ops.point_loss_output_spec(B, M, C, False, False)] == ["loss", "num_pos", "grad_o"]
    assert [n for n, _, _ in ops.point_loss_output_spec(B, M, C, False, True)] == ["loss", "num_pos", "grad_o", "per_point"]
    for spec in (ops.point_output_spec(B, M), ops.point_loss_output_spec(B, M, C, True, True)):
        good = tuple(torch.zeros(shape, dtype=dt) for _, shape, dt in spec)
        assert ops._outputs(spec, good, cpu, "o") == good
        for bad in (good[:-1], good[1:] + good[:1], tuple(t.to(torch.float64) for t in good), good[:-1] + (torch.zeros(B, M, 5),),
                    good[:2] + (torch.zeros(tuple(good[2].shape) + (2,), dtype=good[2].dtype)[..., 0],) + good[3:], list(good)[:2]):
            with pytest.raises(ValueError, match="out: expected contiguous"):
                ops._outputs(spec, bad, cpu, "o")
    # the tuple with grad_c is the right one only with c
    full = tuple(torch.zeros(shape, dtype=dt) for _, shape, dt in ops.point_loss_output_spec(B, M, C, True, False))
    with pytest.raises(ValueError, match="out: expected contiguous"):
        ops._outputs(ops.point_loss_output_spec(B, M, C, False, False), full, cpu, "o")
    # a workspace that is not a GPU buffer of the size the library names is refused by the shared checker
    with pytest.raises(ValueError, match="workspace"):
        ops._workspace(64, torch.zeros(64, dtype=torch.uint8), cpu, "ops.point_head_loss_workspace")


def test_the_modules_take_views_and_refuse_copies(sad):
    import torch
    from sad_amd import PointHeadLoss, PointTargetAssigner, config, point_head
    B, M = 2, 8
    z = torch.zeros(B, M)
    tg = point_head.PointTargets(z.int(), z.int(), z, torch.zeros(B, M, 3), torch.zeros(B, M, 3), torch.zeros(B, M, 7))
    assigner = PointTargetAssigner.from_config(config.KITTI)
    assert assigner.anchors == tuple(tuple(float(v) for v in a) for a in config.KITTI.anchors) and assigner.size_anchor == tuple(config.KITTI.anchor_car)
    assert assigner.shift_max == config.KITTI.shift_max and assigner.extra_width == 0.2 and assigner.num_classes == 3
    mod = assigner.loss(beta=0.5, reg_weight=2.0, cls_loss="focal")
    assert isinstance(mod, PointHeadLoss) and mod.cfg["scale"] == (1.0, 2.0, 1.0, 1.0) and mod.cfg["shift_max"] == config.KITTI.shift_max
    assert mod.cfg["cls_loss"] == "focal" and mod.centerness and mod.num_pos is None
    for o, c in ((torch.zeros(B, M, 10), torch.zeros(B, M, 6)), (torch.zeros(B * M, 10), torch.zeros(B * M, 6)), (torch.zeros(B, M, 10), None)):
        with pytest.raises(RuntimeError, match="no CPU path"):             # the views are accepted: the operator is reached
            mod(o, c, tg)
    for o, c in ((torch.zeros(B, M + 1, 10)[:, :M], None), (torch.zeros(B, M, 10), torch.zeros(B, M, 7)), (torch.zeros(B, M, 10), torch.zeros(B, 6, M).transpose(1, 2)),
                 (torch.zeros(B * M * 10 + 1), None)):
        with pytest.raises(ValueError, match="contiguous rows"):
            mod(o, c, tg)
    with pytest.raises(ValueError, match="shift_max"):
        PointHeadLoss()(torch.zeros(B, M, 10), torch.zeros(B, M, 6), tg)
    with pytest.raises(RuntimeError, match="no CPU path"):
        assigner(torch.zeros(B, M, 3), None, torch.zeros(B, 0, 7), torch.zeros(B, 0, dtype=torch.int32))
