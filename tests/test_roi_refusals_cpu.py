"""Every refusal of the RoI head's host code (SPEC.md §28), none of which needs a GPU.

The C entry points sad_roi_targets_f32, sad_roi_decode_f32 and sad_roi_targets_workspace_bytes: the return code AND the text of
sad_last_error() are compared with tests/golden/roi_refusals.json, so which check fires first when several would is pinned too;
of the size function the returned size is compared.  Argument blocks hold fake non-null device pointers: nothing is dereferenced,
every case is refused before a launch.
    python tests/test_roi_refusals_cpu.py          (rewrites the fixture from the library that is built in the tree)

The operators ops.roi_targets / ops.roi_decode: a wrong dtype, shape or stride and scalars out of range are judged before any
device, so CPU tensors reach them; a CPU tensor that is otherwise right is refused as such; the `out=` and workspace checks are
run against the checkers the operators use, with a CPU device standing in."""
import ctypes
import json
import os
import sys

import pytest

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "roi_refusals.json")
P = 0x10000                                           # a fake device pointer
NAN = float("nan")

TARGETS = dict(rois=P, roi_count=P, roi_labels=P, gt_boxes=P, gt_labels=P, B=2, R=70, D=7, G=5, Dg=8, S=32, fg_max=16, cls_mode=0, seed=1,
               fg_thr=0.55, bg_lo=0.1, hard_ratio=0.8, reg_fg_thr=0.55, cls_fg_thr=0.75, cls_bg_thr=0.25,
               index=P, match=P, labels=P, iou=P, cls_target=P, reg_valid=P, rois_s=P, gt_local=P, reg_target=P, workspace=P)
CASES = [("null", None), ("struct_size", dict(struct_size=-8)), ("struct_size+R=4097", dict(struct_size=8, R=4097))] + [
    (f, {f: None}) for f in ("rois", "index", "match", "labels", "iou", "cls_target", "reg_valid", "rois_s", "gt_local", "reg_target")] + [
    ("rois+R=4097", dict(rois=None, R=4097)),
    ("B=0", dict(B=0)), ("R=0", dict(R=0)), ("S=0", dict(S=0)), ("G=-1", dict(G=-1)), ("S=-3+D=6", dict(S=-3, D=6)),
    ("D=6", dict(D=6)), ("D=6+R=4097", dict(D=6, R=4097)), ("Dg=6", dict(Dg=6)), ("Dg=6+G=1025", dict(Dg=6, G=1025)),
    ("gt_boxes", dict(gt_boxes=None)), ("gt_labels", dict(gt_labels=None)), ("gt_boxes+G=1025", dict(gt_boxes=None, G=1025)),
    ("fg_max=-1", dict(fg_max=-1)), ("hard_ratio=-0.1", dict(hard_ratio=-0.1)), ("hard_ratio=1.5", dict(hard_ratio=1.5)),
    ("hard_ratio nan", dict(hard_ratio=NAN)),
    ("bg_lo<0", dict(bg_lo=-0.1)), ("bg_lo>fg_thr", dict(bg_lo=0.6)), ("fg_thr=0", dict(fg_thr=0.0, bg_lo=0.0)), ("fg_thr nan", dict(fg_thr=NAN)),
    ("cls thresholds equal", dict(cls_fg_thr=0.25)), ("cls thresholds reversed", dict(cls_fg_thr=0.25, cls_bg_thr=0.75)),
    ("cls_bg_thr nan", dict(cls_bg_thr=NAN)), ("reg_fg_thr nan", dict(reg_fg_thr=NAN)),
    ("thresholds+S=1025", dict(bg_lo=0.6, S=1025)),
    ("cls_mode=2", dict(cls_mode=2)), ("cls_mode=-1", dict(cls_mode=-1)),
    ("R=4097", dict(R=4097)), ("S=1025", dict(S=1025)), ("G=1025", dict(G=1025)), ("B=65536", dict(B=65536)),
    ("R=4097+S=1025+G=1025+B=65536", dict(R=4097, S=1025, G=1025, B=65536)), ("R=4097+workspace", dict(R=4097, workspace=None)),
    ("workspace", dict(workspace=None)), ("workspace align", dict(workspace=P + 2)),
]
# sad_roi_decode_f32(rois, D, reg, B, S, boxes, stream): (name, arguments)
DECODE = [("rois", (None, 7, P, 2, 8, P)), ("reg", (P, 7, None, 2, 8, P)), ("boxes", (P, 7, P, 2, 8, None)), ("B=0", (P, 7, P, 0, 8, P)),
          ("S=0", (P, 7, P, 2, 0, P)), ("D=6", (P, 6, P, 2, 8, P)), ("B=0+D=6", (P, 6, P, 0, 8, P)), ("B*S=2^31", (P, 7, P, 1 << 15, 1 << 16, P)),
          ("D=6+B*S=2^31", (P, 6, P, 1 << 15, 1 << 16, P))]
SIZES = [(2, 70), (1, 1), (65535, 4096), (0, 70), (-1, 70), (65536, 70), (2, 0), (2, -5), (2, 4097)]


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
    """{case name: [return code, message] or a size} of every case, from the library that is loaded."""
    from sad_amd import _lib
    L = _lib.lib()
    got = {}
    assert len({name for name, _ in CASES}) == len(CASES) and len({name for name, _ in DECODE}) == len(DECODE)
    for name, ov in CASES:
        a = _block(_lib.RoiTargetsArgs, TARGETS, ov)
        code = L.sad_roi_targets_f32(ctypes.byref(a) if a is not None else None, None)
        assert code in (-1, -2), f"roi_targets: {name} was not refused on the host (code {code})"
        got[f"roi_targets: {name}"] = [code, L.sad_last_error().decode()]
    for name, args in DECODE:
        code = L.sad_roi_decode_f32(*args, None)
        assert code in (-1, -2), f"roi_decode: {name} was not refused on the host (code {code})"
        got[f"roi_decode: {name}"] = [code, L.sad_last_error().decode()]
    for args in SIZES:
        got[f"roi_targets_workspace_bytes{args}"] = L.sad_roi_targets_workspace_bytes(*args)
    return got


def test_roi_refusals_match_the_recorded_ones(sad):
    want = json.load(open(FIXTURE))
    got = outcomes()
    assert sorted(got) == sorted(want), "the cases of this file and of the fixture differ"
    wrong = {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    assert not wrong, f"{len(wrong)} refusals changed (got, recorded): {wrong}"


def test_the_recorded_codes_are_the_ones_the_section_names():
    """SAD_EUNSUPPORTED (-2) above the caps and only there; SAD_EINVAL (-1) for the rest; the size function answers 8*B*R or 0."""
    want = json.load(open(FIXTURE))
    caps = {"roi_targets: R=4097", "roi_targets: S=1025", "roi_targets: G=1025", "roi_targets: B=65536",
            "roi_targets: R=4097+S=1025+G=1025+B=65536", "roi_targets: R=4097+workspace", "roi_decode: B*S=2^31"}
    for k, v in want.items():
        if isinstance(v, list):
            assert v[0] == (-2 if k in caps else -1) and v[1], k
    for B, R in SIZES:
        assert want[f"roi_targets_workspace_bytes{(B, R)}"] == (8 * B * R if 1 <= B <= 65535 and 1 <= R <= 4096 else 0)
    assert "struct_size" in want["roi_targets: struct_size"][1] and "struct_size" in want["roi_targets: struct_size+R=4097"][1]


# ---- the operators --------------------------------------------------------------------------------------------------------
KW = dict(S=32, fg_max=16, fg_thr=0.55, bg_lo=0.1, hard_ratio=0.8, reg_fg_thr=0.55, cls_fg_thr=0.75, cls_bg_thr=0.25)


def _cpu_inputs(B=2, R=9, D=7, G=3):
    import torch
    return [torch.zeros(B, R, D), torch.zeros(B, dtype=torch.int32), torch.zeros(B, R, dtype=torch.int32), torch.zeros(B, G, 7),
            torch.zeros(B, G, dtype=torch.int32)]


def test_roi_targets_argument_errors(sad):
    import torch
    from sad_amd import ops

    def call(change=None, **kw):
        a = _cpu_inputs()
        if change:
            change(a)
        return ops.roi_targets(*a, **dict(KW, **kw))

    def put(i, t):
        return lambda a: a.__setitem__(i, t)

    for i, t in ((0, torch.zeros(2, 9, 7, dtype=torch.float64)), (1, torch.zeros(2, dtype=torch.int64)), (2, torch.zeros(2, 9)),
                 (3, torch.zeros(2, 3, 7, dtype=torch.float16)), (4, torch.zeros(2, 3, dtype=torch.int64)), (0, None)):
        with pytest.raises(TypeError):
            call(put(i, t))
    for i, t in ((0, torch.zeros(2, 9, 6)), (0, torch.zeros(18, 7)), (0, torch.zeros(2, 4097, 7)), (0, torch.zeros(2, 0, 7)),
                 (1, torch.zeros(3, dtype=torch.int32)), (2, torch.zeros(2, 8, dtype=torch.int32)), (3, torch.zeros(2, 3, 6)),
                 (3, torch.zeros(3, 3, 7)), (4, torch.zeros(2, 4, dtype=torch.int32)), (3, torch.zeros(2, 1025, 7)),
                 (0, torch.zeros(2, 9, 14)[..., ::2]), (2, torch.zeros(2, 18, dtype=torch.int32)[:, ::2]),
                 (3, torch.zeros(2, 7, 3).transpose(1, 2))):
        with pytest.raises(ValueError):
            call(put(i, t))
    for kw in (dict(S=0), dict(S=1025), dict(fg_max=-1), dict(bg_lo=0.6), dict(bg_lo=-0.1), dict(fg_thr=0.0, bg_lo=0.0), dict(cls_fg_thr=0.25),
               dict(cls_fg_thr=0.2), dict(hard_ratio=1.5), dict(hard_ratio=-0.5), dict(reg_fg_thr=NAN), dict(cls_mode="iou")):
        with pytest.raises(ValueError):
            call(**kw)
    # thresholds are compared after rounding to binary32: 0.1 and the double next to it are the same threshold
    with pytest.raises(RuntimeError, match="no CPU path"):
        call(fg_thr=0.1, bg_lo=0.1 + 1e-12)
    # everything right but the device
    with pytest.raises(RuntimeError, match="no CPU path"):
        call()
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.roi_targets(_cpu_inputs()[0], None, None, torch.zeros(2, 0, 7), torch.zeros(2, 0, dtype=torch.int32), **KW)


def test_roi_decode_argument_errors(sad):
    import torch
    from sad_amd import ops
    with pytest.raises(TypeError):
        ops.roi_decode(torch.zeros(2, 8, 7, dtype=torch.float64), torch.zeros(2, 8, 7))
    with pytest.raises(TypeError):
        ops.roi_decode(torch.zeros(2, 8, 7), torch.zeros(2, 8, 7, dtype=torch.int32))
    for rois, reg in ((torch.zeros(2, 8, 6), torch.zeros(2, 8, 7)), (torch.zeros(2, 8, 7), torch.zeros(2, 8, 8)), (torch.zeros(2, 8, 7), torch.zeros(2, 9, 7)),
                      (torch.zeros(16, 7), torch.zeros(16, 7)), (torch.zeros(2, 0, 7), torch.zeros(2, 0, 7)),
                      (torch.zeros(2, 8, 14)[..., ::2], torch.zeros(2, 8, 7)), (torch.zeros(2, 8, 7), torch.zeros(2, 7, 8).transpose(1, 2))):
        with pytest.raises(ValueError):
            ops.roi_decode(rois, reg)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.roi_decode(torch.zeros(2, 8, 9), torch.zeros(2, 8, 7))


def test_out_and_workspace_checks(sad):
    """The two checkers roi_targets hands its `out=` tuple and its workspace to, on the operator's own spec."""
    import torch
    from sad_amd import ops, _lib
    B, R, S = 2, 9, 32
    cpu = torch.device("cpu")
    spec = ops.roi_output_spec(B, S)
    assert tuple(n for n, _, _ in spec) == ops.ROI_OUTPUTS
    good = tuple(torch.zeros(shape, dtype=dt) for _, shape, dt in spec)
    assert ops._outputs(spec, good, cpu, "rois") == good
    for bad in (good[:-1], good[1:] + good[:1], tuple(t.to(torch.float64) for t in good), good[:-1] + (torch.zeros(B, S, 8),),
                good[:-1] + (torch.zeros(B, 7, S).transpose(1, 2),), list(good)[:3]):
        with pytest.raises(ValueError, match="out: expected contiguous"):
            ops._outputs(spec, bad, cpu, "rois")
    nbytes = _lib.lib().sad_roi_targets_workspace_bytes(B, R)
    assert nbytes == 8 * B * R
    with pytest.raises(ValueError, match=f"at least {nbytes} bytes"):
        ops._workspace(nbytes, torch.zeros(nbytes - 1, dtype=torch.uint8), cpu, "ops.roi_targets_workspace", 4)
    with pytest.raises(ValueError, match="1 <= B <= 65535"):
        ops.roi_targets_workspace(2, 4097, cpu)


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    res = outcomes()
    with open(FIXTURE, "w") as fh:
        json.dump(res, fh, indent=0, sort_keys=True)
        fh.write("\n")
    print(f"recorded {len(res)} refusals -> {FIXTURE}")
