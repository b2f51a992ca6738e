"""Every refusal of the RoI head loss' host code (SPEC.md §29), none of which needs a GPU.

The C entry point sad_roi_head_loss_f32: the return code AND the text of sad_last_error() are compared with
tests/golden/roi_loss_refusals.json, so which check fires first when several would is pinned too.  Argument blocks hold fake
non-null device pointers: nothing is dereferenced, every case is refused before the launch.
    python tests/test_roi_loss_refusals_cpu.py          (rewrites the fixture from the library that is built in the tree)

The operator ops.roi_head_loss: a wrong dtype, shape or stride and scalars out of range are judged before any device, so CPU
tensors reach them; CPU tensors that are otherwise right are refused as such; the `out=` check is run against the checker and
the spec the operator uses, with a CPU device standing in.  The module's view rules are checked the same way."""
import ctypes
import json
import os
import sys

import pytest

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "roi_loss_refusals.json")
P = 0x10000                                           # a fake device pointer
NAN = float("nan")

BASE = dict(rcnn_cls=P, rcnn_reg=P, cls_target=P, reg_valid=P, reg_target=P, rois=P, gt_local=P, B=2, S=128, D=7, normalize=1, beta=0.125,
            loss=P, num=P, grad_cls=P, grad_reg=P, grad_corner=P, per_roi=P)
NO_CORNER = dict(rois=None, gt_local=None, grad_corner=None)
CASES = [("null", None), ("struct_size", dict(struct_size=-8)), ("struct_size+S=1025", dict(struct_size=8, S=1025))] + [
    (f, {f: None}) for f in ("rcnn_cls", "rcnn_reg", "cls_target", "reg_valid", "reg_target", "loss", "num", "grad_cls", "grad_reg")] + [
    ("rcnn_cls+S=1025", dict(rcnn_cls=None, S=1025)),
    ("B=0", dict(B=0)), ("S=0", dict(S=0)), ("B=-1+D=6", dict(B=-1, D=6)), ("S=0+rois", dict(S=0, rois=None)),
    ("rois", dict(rois=None)), ("gt_local", dict(gt_local=None)), ("rois+grad_corner", dict(rois=None, grad_corner=None)),
    ("grad_corner", dict(grad_corner=None)), ("grad_corner without corner", dict(rois=None, gt_local=None)),
    ("gt_local+D=6", dict(gt_local=None, D=6)),
    ("D=6", dict(D=6)), ("D=0", dict(D=0)), ("D=6+beta=0", dict(D=6, beta=0.0)), ("D=6+B=65536", dict(D=6, B=65536)),
    ("beta=0", dict(beta=0.0)), ("beta=-1", dict(beta=-1.0)), ("beta nan", dict(beta=NAN)), ("beta=0+S=1025", dict(beta=0.0, S=1025)),
    ("beta=0 no corner", dict(NO_CORNER, beta=0.0)),
    ("S=1025", dict(S=1025)), ("B=65536", dict(B=65536)), ("B=65536+S=1025", dict(B=65536, S=1025)), ("S=1025 no corner", dict(NO_CORNER, S=1025)),
]
CAPS = {"S=1025", "B=65536", "B=65536+S=1025", "S=1025 no corner"}


def _block(cls, base, ov):
    if ov is None:
        return None
    f = dict(base, **ov)
    a = cls()
    a.struct_size = ctypes.sizeof(cls) + f.pop("struct_size", 0)
    for k, v in f.items():
        setattr(a, k, v)
    return a


def outcomes():
    """{case name: [return code, message]} of every case, from the library that is loaded."""
    from sad_amd import _lib
    L = _lib.lib()
    got = {}
    assert len({name for name, _ in CASES}) == len(CASES)
    for name, ov in CASES:
        a = _block(_lib.RoiHeadLossArgs, BASE, ov)
        code = L.sad_roi_head_loss_f32(ctypes.byref(a) if a is not None else None, None)
        assert code in (-1, -2), f"roi_head_loss: {name} was not refused on the host (code {code})"
        got[f"roi_head_loss: {name}"] = [code, L.sad_last_error().decode()]
    return got


def test_roi_loss_refusals_match_the_recorded_ones(sad):
    want = json.load(open(FIXTURE))
    got = outcomes()
    assert sorted(got) == sorted(want), "the cases of this file and of the fixture differ"
    wrong = {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    assert not wrong, f"{len(wrong)} refusals changed (got, recorded): {wrong}"


def test_the_recorded_codes_are_the_ones_the_section_names():
    """SAD_EUNSUPPORTED (-2) above the caps and only there; SAD_EINVAL (-1) for the rest."""
    want = json.load(open(FIXTURE))
    for k, v in want.items():
        assert v[0] == (-2 if k.split(": ", 1)[1] in CAPS else -1) and v[1].startswith("sad_roi_head_loss_f32: "), k
    assert "struct_size" in want["roi_head_loss: struct_size"][1] and "struct_size" in want["roi_head_loss: struct_size+S=1025"][1]
    for k in ("rois", "gt_local", "rois+grad_corner"):
        assert "together" in want[f"roi_head_loss: {k}"][1]
    for k in ("grad_corner", "grad_corner without corner"):
        assert "grad_corner" in want[f"roi_head_loss: {k}"][1]
    assert "beta" in want["roi_head_loss: beta nan"][1] and "D = 6" in want["roi_head_loss: D=6"][1]


def test_the_mirror_has_the_size_of_the_struct(sad):
    """A right-sized block with everything NULL is refused for its pointers, not for its size."""
    from sad_amd import _lib
    a = _lib.RoiHeadLossArgs()
    a.struct_size = ctypes.sizeof(_lib.RoiHeadLossArgs)
    assert _lib.lib().sad_roi_head_loss_f32(ctypes.byref(a), None) == -1
    assert b"NULL pointer" in _lib.lib().sad_last_error()


# ---- the operator ---------------------------------------------------------------------------------------------------------
def _cpu_inputs(B=2, S=8, D=7):
    import torch
    return [torch.zeros(B, S), torch.zeros(B, S, 7), torch.zeros(B, S), torch.zeros(B, S, dtype=torch.int32), torch.zeros(B, S, 7),
            torch.zeros(B, S, D), torch.zeros(B, S, 7)]


def test_roi_head_loss_argument_errors(sad):
    import torch
    from sad_amd import ops

    def call(change=None, **kw):
        a = _cpu_inputs()
        if change:
            change(a)
        return ops.roi_head_loss(*a, **kw)

    def put(i, t):
        return lambda a: a.__setitem__(i, t)

    for i, t in ((0, torch.zeros(2, 8, dtype=torch.float64)), (1, torch.zeros(2, 8, 7, dtype=torch.float16)), (2, torch.zeros(2, 8, dtype=torch.int32)),
                 (3, torch.zeros(2, 8)), (3, torch.zeros(2, 8, dtype=torch.int64)), (4, torch.zeros(2, 8, 7, dtype=torch.float64)),
                 (5, torch.zeros(2, 8, 7, dtype=torch.float64)), (6, torch.zeros(2, 8, 7, dtype=torch.int32)), (0, None)):
        with pytest.raises(TypeError):
            call(put(i, t))
    for i, t in ((0, torch.zeros(2, 8, 1)), (0, torch.zeros(16)), (0, torch.zeros(2, 0)), (0, torch.zeros(2, 1025)), (1, torch.zeros(2, 8, 8)),
                 (1, torch.zeros(16, 7)), (1, torch.zeros(2, 9, 7)), (2, torch.zeros(2, 9)), (3, torch.zeros(3, 8, dtype=torch.int32)),
                 (4, torch.zeros(2, 8, 6)), (5, torch.zeros(2, 8, 6)), (5, torch.zeros(2, 9, 7)), (5, torch.zeros(16, 7)), (6, torch.zeros(2, 8, 8)),
                 (5, None), (6, None),
                 (0, torch.zeros(2, 16)[:, ::2]), (1, torch.zeros(2, 7, 8).transpose(1, 2)), (5, torch.zeros(2, 8, 18)[..., ::2]),
                 (3, torch.zeros(8, 2, dtype=torch.int32).t())):
        with pytest.raises(ValueError):
            call(put(i, t))
    for kw in (dict(beta=0.0), dict(beta=-1.0), dict(beta=NAN), dict(beta=1e-60), dict(code_weights=[1.0] * 6), dict(scale=(1.0, 1.0))):
        with pytest.raises(ValueError):
            call(**kw)
    # everything right but the device: with and without the corner component, rows of D = 9
    with pytest.raises(RuntimeError, match="no CPU path"):
        call()
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.roi_head_loss(*_cpu_inputs()[:5])
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.roi_head_loss(*_cpu_inputs(D=9), per_roi=True)


def test_out_checks(sad):
    """The checker roi_head_loss hands its `out=` tuple to, on the operator's own spec."""
    import torch
    from sad_amd import ops
    B, S = 2, 8
    cpu = torch.device("cpu")
    assert [n for n, _, _ in ops.roi_loss_output_spec(B, S, True, True)] == ["loss", "num", "grad_cls", "grad_reg", "grad_corner", "per_roi"]
    assert [n for n, _, _ in ops.roi_loss_output_spec(B, S, False, False)] == ["loss", "num", "grad_cls", "grad_reg"]
    assert [n for n, _, _ in ops.roi_loss_output_spec(B, S, False, True)] == ["loss", "num", "grad_cls", "grad_reg", "per_roi"]
    spec = ops.roi_loss_output_spec(B, S, True, True)
    good = tuple(torch.zeros(shape, dtype=dt) for _, shape, dt in spec)
    assert ops._outputs(spec, good, cpu, "rcnn_cls") == good
    for bad in (good[:-1], good[1:] + good[:1], tuple(t.to(torch.float64) for t in good), good[:-1] + (torch.zeros(B, S, 4),),
                good[:3] + (torch.zeros(B, 7, S).transpose(1, 2),) + good[4:], list(good)[:4]):
        with pytest.raises(ValueError, match="out: expected contiguous"):
            ops._outputs(spec, bad, cpu, "rcnn_cls")
    # the tuple without grad_corner is the right one only without the corner component
    with pytest.raises(ValueError, match="out: expected contiguous"):
        ops._outputs(ops.roi_loss_output_spec(B, S, False, False), good[:5], cpu, "rcnn_cls")


def test_the_module_takes_views_and_refuses_copies(sad):
    import torch
    from sad_amd import roi_head
    B, S = 2, 8
    z = torch.zeros(B, S)
    tg = roi_head.RoiTargets(z.int(), z.int(), z.int(), z, z, z.int(), torch.zeros(B, S, 7), torch.zeros(B, S, 7), torch.zeros(B, S, 7))
    layer = roi_head.ProposalTargetLayer(roi_per_image=S)
    mod = layer.loss(beta=0.5, cls_weight=1.0, reg_weight=2.0, corner_weight=0.5)
    assert isinstance(mod, roi_head.RoIHeadLoss) and mod.cfg["scale"] == (1.0, 2.0, 0.5) and mod.cfg["beta"] == 0.5 and mod.corner and mod.num is None
    assert roi_head.RoIHeadLoss(corner=False).corner is False
    for cls, reg in ((torch.zeros(B, S), torch.zeros(B, S, 7)), (torch.zeros(B, S, 1), torch.zeros(B * S, 7)), (torch.zeros(B * S, 1), torch.zeros(B, S, 7))):
        with pytest.raises(RuntimeError, match="no CPU path"):             # the views are accepted: the operator is reached
            mod(cls, reg, tg)
    for cls, reg in ((torch.zeros(B, S + 1), torch.zeros(B, S, 7)), (torch.zeros(B, S), torch.zeros(B, S, 8)), (torch.zeros(B, 2 * S)[:, ::2], torch.zeros(B, S, 7)),
                     (torch.zeros(B, S), torch.zeros(B, 7, S).transpose(1, 2))):
        with pytest.raises(ValueError, match="contiguous predictions"):
            mod(cls, reg, tg)


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    res = outcomes()
    with open(FIXTURE, "w") as fh:
        json.dump(res, fh, indent=0, sort_keys=True)
        fh.write("\n")
    print(f"recorded {len(res)} refusals -> {FIXTURE}")
