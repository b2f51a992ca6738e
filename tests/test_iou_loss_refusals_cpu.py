"""Every refusal of the rotated IoU loss' host code (SPEC.md §34), none of which needs a GPU.

The C entry point sad_rotated_iou_loss_f32: argument blocks hold fake non-null device pointers, nothing is dereferenced, every
case is refused with SAD_EINVAL before the launch and sad_last_error() names the reason; where several checks would fire, the
order of §34's list decides.  The operator ops.rotated_iou_loss: a wrong dtype, shape or stride and unknown names are judged
before any device, so CPU tensors reach them; CPU tensors that are otherwise right are refused as such; the `out=` check is run
against the checker and the spec the operator uses, with a CPU device standing in."""
import ctypes

import pytest

P = 0x10000                                           # a fake device pointer
BOX = dict(pred=P, target=P, weight=P, rois=None, N=256, Dp=7, Dt=9, Dr=0, mode=1, kind=1, code=0, need_grad=1, loss=P, iou=P, grad=P,
           decoded=None)
ROI = dict(BOX, rois=P, Dr=7, code=1, decoded=P)
CASES = [
    ("struct_size short", BOX, dict(struct_size=-8), "struct_size"),
    ("struct_size long + N=0", BOX, dict(struct_size=8, N=0), "struct_size"),
    ("pred", BOX, dict(pred=None), "NULL pointer"),
    ("target", BOX, dict(target=None), "NULL pointer"),
    ("loss", BOX, dict(loss=None), "NULL pointer"),
    ("iou", ROI, dict(iou=None), "NULL pointer"),
    ("pred + N=0", BOX, dict(pred=None, N=0), "NULL pointer"),
    ("N=0", BOX, dict(N=0), "N >= 1"),
    ("N=-5", ROI, dict(N=-5), "N >= 1"),
    ("N=0 + Dp=6", BOX, dict(N=0, Dp=6), "N >= 1"),
    ("Dp=6", BOX, dict(Dp=6), "D = 6, 9"),
    ("Dt=0", BOX, dict(Dt=0), "D = 7, 0"),
    ("Dp=6 + mode=2", BOX, dict(Dp=6, mode=2), "D = 6, 9"),
    ("mode=2", BOX, dict(mode=2), "mode"),
    ("mode=-1", ROI, dict(mode=-1), "mode"),
    ("kind=2", BOX, dict(kind=2), "kind"),
    ("kind=-1 + code=2", BOX, dict(kind=-1, code=2), "kind"),
    ("code=2", BOX, dict(code=2), "code"),
    ("code=2 with rois", ROI, dict(code=2), "code"),
    ("roi without rois", ROI, dict(rois=None), "rois must be given iff"),
    ("rois with box", BOX, dict(rois=P, Dr=7), "rois must be given iff"),
    ("rois Dr=6", ROI, dict(Dr=6), "rois rows have D = 6"),
    ("decoded with box", BOX, dict(decoded=P), "decoded"),
    ("grad missing", BOX, dict(grad=None), "grad must be given iff"),
    ("grad against need_grad=0", ROI, dict(need_grad=0), "grad must be given iff"),
]


def _block(cls, base, ov):
    f = dict(base, **ov)
    a = cls()
    a.struct_size = ctypes.sizeof(cls) + f.pop("struct_size", 0)
    for k, v in f.items():
        setattr(a, k, v)
    return a


@pytest.mark.parametrize("name,base,ov,needle", CASES, ids=[c[0] for c in CASES])
def test_refused_on_the_host(sad, name, base, ov, needle):
    from sad_amd import _lib
    L = _lib.lib()
    code = L.sad_rotated_iou_loss_f32(ctypes.byref(_block(_lib.RotatedIouLossArgs, base, ov)), None)
    msg = L.sad_last_error().decode()
    assert code == -1, f"{name}: not refused with SAD_EINVAL (code {code})"
    assert msg.startswith("sad_rotated_iou_loss_f32: ") and needle in msg, msg


def test_null_args_and_the_size_of_the_mirror(sad):
    from sad_amd import _lib
    L = _lib.lib()
    assert L.sad_rotated_iou_loss_f32(None, None) == -1 and b"NULL args" in L.sad_last_error()
    a = _lib.RotatedIouLossArgs()                     # a right-sized block with everything NULL is refused for its pointers
    a.struct_size = ctypes.sizeof(_lib.RotatedIouLossArgs)
    assert L.sad_rotated_iou_loss_f32(ctypes.byref(a), None) == -1 and b"NULL pointer" in L.sad_last_error()
    assert ctypes.sizeof(_lib.RotatedIouLossArgs) == 8 + 4 * 8 + 8 * 4 + 4 * 8
    assert L.sad_version() == _lib.ABI_VERSION == 4


# ---- the operator ---------------------------------------------------------------------------------------------------------
def test_operator_argument_errors(sad):
    import torch
    from sad_amd import ops
    z = torch.zeros
    for args, kw in (((z(8, 7, dtype=torch.float64), z(8, 7)), {}), ((z(8, 7), z(8, 7, dtype=torch.float16)), {}), ((None, z(8, 7)), {}),
                     ((z(8, 7), z(8, 7), z(8, dtype=torch.int32)), {}), ((z(8, 7), z(8, 7)), dict(code="roi", rois=z(8, 7, dtype=torch.float64)))):
        with pytest.raises(TypeError):
            ops.rotated_iou_loss(*args, **kw)
    for args, kw in (((z(8, 6), z(8, 7)), {}), ((z(8, 7), z(8, 6)), {}), ((z(7), z(7)), {}), ((z(0, 7), z(0, 7)), {}), ((z(8, 7), z(9, 7)), {}),
                     ((z(2, 4, 7), z(8, 7)), {}), ((z(8, 7), z(8, 7), z(8, 1)), {}), ((z(8, 7), z(8, 7), z(9)), {}),
                     ((z(8, 14)[:, ::2], z(8, 7)), {}), ((z(8, 7), z(7, 8).t()), {}), ((z(8, 7), z(8, 7), z(16)[::2]), {}),
                     ((z(8, 7), z(8, 7)), dict(mode="2d")), ((z(8, 7), z(8, 7)), dict(kind="giou")), ((z(8, 7), z(8, 7)), dict(code="anchor")),
                     ((z(8, 7), z(8, 7)), dict(code="roi")), ((z(8, 7), z(8, 7)), dict(rois=z(8, 7))), ((z(8, 7), z(8, 7)), dict(decoded=True)),
                     ((z(8, 7), z(8, 7)), dict(code="roi", rois=z(8, 6))), ((z(8, 7), z(8, 7)), dict(code="roi", rois=z(9, 7)))):
        with pytest.raises(ValueError):
            ops.rotated_iou_loss(*args, **kw)
    # everything right but the device
    for args, kw in (((z(8, 7), z(8, 9)), {}), ((z(2, 4, 9), z(2, 4, 7), z(2, 4)), dict(mode="bev", kind="diou", need_grad=False)),
                     ((z(2, 4, 7), z(2, 4, 7), z(2, 4)), dict(code="roi", rois=z(2, 4, 9), decoded=True))):
        with pytest.raises(RuntimeError, match="no CPU path"):
            ops.rotated_iou_loss(*args, **kw)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.boxes_iou_aligned(z(8, 7), z(8, 7), "bev")


def test_out_checks(sad):
    import torch
    from sad_amd import ops
    cpu = torch.device("cpu")
    assert [n for n, _, _ in ops.rotated_iou_loss_output_spec((2, 8), True, True)] == ["loss", "iou", "grad", "decoded"]
    assert [n for n, _, _ in ops.rotated_iou_loss_output_spec((8,), False, False)] == ["loss", "iou"]
    assert [n for n, _, _ in ops.rotated_iou_loss_output_spec((8,), False, True)] == ["loss", "iou", "decoded"]
    spec = ops.rotated_iou_loss_output_spec((2, 8), True, False)
    assert [tuple(s) for _, s, _ in spec] == [(2, 8), (2, 8), (2, 8, 7)]
    good = tuple(torch.zeros(shape, dtype=dt) for _, shape, dt in spec)
    assert ops._outputs(spec, good, cpu, "pred") == good
    for bad in (good[:-1], good[1:] + good[:1], tuple(t.to(torch.float64) for t in good), good[:2] + (torch.zeros(16, 7),),
                good[:2] + (torch.zeros(2, 7, 8).transpose(1, 2),)):
        with pytest.raises(ValueError, match="out: expected contiguous"):
            ops._outputs(spec, bad, cpu, "pred")


def test_the_modules_take_views_and_refuse_copies(sad):
    import torch
    import sad_amd
    from sad_amd import iou_loss, roi_head
    assert sad_amd.RotatedIoULoss is iou_loss.RotatedIoULoss and sad_amd.RoIIoULoss is roi_head.RoIIoULoss
    assert sad_amd.rotated_iou_loss is sad_amd.ops.rotated_iou_loss and sad_amd.boxes_iou_aligned is sad_amd.ops.boxes_iou_aligned
    with pytest.raises(ValueError, match="reduction"):
        iou_loss.RotatedIoULoss(reduction="batchmean")
    mod = iou_loss.RotatedIoULoss("bev", "diou", "mean")
    assert mod.cfg == dict(mode="bev", kind="diou", code="box") and mod.iou is None
    with pytest.raises(RuntimeError, match="no CPU path"):
        mod(torch.zeros(8, 7), torch.zeros(8, 7))
    B, S = 2, 8
    z = torch.zeros(B, S)
    tg = roi_head.RoiTargets(z.int(), z.int(), z.int(), z, z, z.int(), torch.zeros(B, S, 7), torch.zeros(B, S, 7), torch.zeros(B, S, 7))
    rmod = roi_head.ProposalTargetLayer(roi_per_image=S).iou_loss(mode="bev", kind="diou", normalize=False)
    assert isinstance(rmod, roi_head.RoIIoULoss) and rmod.cfg == dict(mode="bev", kind="diou", code="roi") and not rmod.normalize
    for reg in (torch.zeros(B, S, 7), torch.zeros(B * S, 7)):
        with pytest.raises(RuntimeError, match="no CPU path"):             # the views are accepted: the operator is reached
            rmod(reg, tg)
    for reg in (torch.zeros(B, S, 8), torch.zeros(B, S + 1, 7), torch.zeros(B, 7, S).transpose(1, 2), torch.zeros(B * S * 7)):
        with pytest.raises(ValueError, match="contiguous predictions"):
            rmod(reg, tg)
