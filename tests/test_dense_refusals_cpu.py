"""Every refusal of the dense-head host code (SPEC.md §25 - §27): the six entry points sad_anchor_decode_f32, sad_center_decode_f32,
sad_anchor_targets_f32, sad_center_targets_f32, sad_anchor_head_loss_f32, sad_center_head_loss_f32 and the three *_workspace_bytes
functions.  The return code AND the text of sad_last_error() are compared with tests/golden/dense_refusals.json, so which check
fires first when several would is pinned too; of a size function the returned size is compared.  Argument blocks hold fake non-null
device pointers: nothing is dereferenced, and every case of an entry point is refused before a launch (needs no GPU).  Shapes
that are accepted are not in the tables: the 2^31 limits are met from above only (exactly 2^31 rows, the smallest refused count).

The fixture was recorded from the library as it was before the three files came to share csrc/dense_tile.h:
    python tests/test_dense_refusals_cpu.py          (rewrites the fixture from the library that is built in the tree)"""
import ctypes
import json
import os
import sys

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dense_refusals.json")
P = 0x10000                                           # a fake device pointer
SIZES3 = (3.9, 1.6, 1.56, 0.8, 0.6, 1.73, 1.76, 0.6, 1.73)
GRID = dict(x0=0.0, y0=-40.0, sx=0.4, sy=0.4)
BIG = 46341                                           # BIG * BIG = 2^31 + 4633: the smallest square grid that is refused
HALF = 1 << 15                                        # HALF * HALF = 2^30

ANCHOR_DECODE = dict(cls=P, reg=P, dir=P, boxes=P, scores=P, labels=P, B=2, H=5, W=7, C=3, nb=2, ns=3, nr=2, layout=0,
                     sizes=SIZES3, rotations=(0.0, 1.57), dir_offset=0.78, **GRID)
CENTER_DECODE = dict(hm=P, reg=P, height=P, dim=P, rot=P, vel=P, boxes=P, scores=P, labels=P, B=2, H=5, W=7, C=3, layout=0,
                     log_dim=1, peak=1, lo_x=0.0, lo_y=-40.0, sx=0.4, sy=0.4)
ANCHOR_TARGETS = dict(gt_boxes=P, gt_labels=P, B=2, G=5, D=7, H=5, W=7, ns=3, nr=2, nb=2, use_size_class=1, sizes=SIZES3,
                      rotations=(0.0, 1.57), pos_thr=(0.6, 0.5, 0.5), neg_thr=(0.45, 0.35, 0.35), size_class=(0, 1, 2), dir_offset=0.78,
                      labels=P, match=P, reg_target=P, max_iou=P, dir_target=P, workspace=P, **GRID)
CENTER_TARGETS = dict(gt_boxes=P, gt_labels=P, B=2, G=5, D=9, C=3, H=5, W=7, layout=0, min_radius=2, vel=1, lo_x=0.0, lo_y=-40.0,
                      sx=0.4, sy=0.4, min_overlap=0.1, heatmap=P, ind=P, anno=P)
ANCHOR_LOSS = dict(cls=P, reg=P, dir=P, labels=P, reg_target=P, dir_target=P, B=2, H=5, W=7, A=6, C=3, nb=2, layout=0, sin_diff=1,
                   normalize=1, alpha=0.25, beta=1.0 / 9.0, code_weights=(1.0,) * 7, scale=(1.0, 2.0, 0.2), loss=P, num_pos=P,
                   grad_cls=P, grad_reg=P, grad_dir=P, per_anchor=P, workspace=P)
CENTER_LOSS = dict(hm=P, reg=P, height=P, dim=P, rot=P, vel=P, heatmap=P, ind=P, anno=P, B=2, H=5, W=7, C=3, G=5, layout=0,
                   normalize=1, code_weights=(1.0,) * 10, scale=(1.0, 0.25), loss=P, num_pos=P, grad_hm=P, grad_reg=P, grad_height=P,
                   grad_dim=P, grad_rot=P, grad_vel=P, workspace=P)

# what the four entry points with a cell grid share: (name, overrides)
HEAD = [("null", None), ("struct_size", dict(struct_size=-8)), ("struct_size+layout", dict(struct_size=8, layout=2))]
LAYOUT = [("layout=2", dict(layout=2)), ("layout=-1", dict(layout=-1)), ("layout+B=0", dict(layout=7, B=0)),
          ("layout+B=65536+C=65", dict(layout=2, B=65536, C=65))]
ANCHOR_SET = [
    ("ns=0", dict(ns=0)), ("nr=0", dict(nr=0)), ("nr=-1+nb=1", dict(nr=-1, nb=1)),
    ("nb=1", dict(nb=1)), ("nb=-2", dict(nb=-2)), ("nb=1+ns=17", dict(nb=1, ns=17)),
    ("ns=17", dict(ns=17)), ("nr=9", dict(nr=9)), ("nb=9", dict(nb=9)), ("ns=17+nr=9+nb=9", dict(ns=17, nr=9, nb=9)),
    ("ns=17+H*W", dict(ns=17, H=BIG, W=BIG)), ("ns=17+B=65536", dict(ns=17, B=65536)),
]
# the ladder of an anchor grid, A = ns * nr = 6 in the base blocks: H * W, K = H * W * A and B * K at exactly 2^31 and above
LADDER_A = [
    ("H*W", dict(H=BIG, W=BIG)), ("H*W=2^31", dict(H=1 << 16, W=HALF)), ("H*W=2^40", dict(H=1 << 20, W=1 << 20)),
    ("H*W=2^60", dict(B=1, H=1 << 30, W=1 << 30)), ("K=2^31", dict(B=1, H=HALF, W=HALF, ns=1, nr=2)),
    ("K=3*2^30", dict(B=1, H=HALF, W=HALF)), ("B*K=2^31", dict(B=2, H=HALF, W=HALF, ns=1, nr=1)),
    ("B*K", dict(B=65535, H=64, W=65, ns=2, nr=4)), ("B*K=2^31, A=128", dict(B=1 << 10, H=128, W=128, ns=16, nr=8, sizes=(1.5,) * 48)),
]
LADDER_CELLS = [
    ("H*W", dict(H=BIG, W=BIG)), ("H*W=2^31", dict(H=1 << 16, W=HALF)), ("H*W=2^60", dict(B=1, H=1 << 30, W=1 << 30)),
    ("B*H*W=2^31", dict(B=2, H=HALF, W=HALF)), ("B*H*W", dict(B=65535, H=256, W=129)),
]
INDEX = [("index P=0", dict(index=P, P=0)), ("index P=-3", dict(index=P, P=-3)), ("index P=0+B=65536", dict(index=P, P=0, B=65536)),
         ("B*P=2^31", dict(index=P, B=HALF, P=1 << 16)), ("B*P", dict(index=P, B=65535, P=HALF + 1)),
         ("B*K+B*P", dict(index=P, B=65535, P=HALF + 1, H=256, W=128))]
GT = [("B=0", dict(B=0)), ("G=-1", dict(G=-1)), ("D=6", dict(D=6)), ("D=6+G=1025", dict(D=6, G=1025)),
      ("gt_boxes", dict(gt_boxes=None)), ("gt_labels", dict(gt_labels=None)), ("gt_boxes+G=1025", dict(gt_boxes=None, G=1025)),
      ("G=1025", dict(G=1025)), ("B=65536", dict(B=65536)), ("G=1025+B=65536", dict(G=1025, B=65536))]

CASES = {
    "anchor_decode": HEAD + LAYOUT + ANCHOR_SET + LADDER_A + INDEX + [
        (f, {f: None}) for f in ("cls", "reg", "boxes", "scores", "labels")] + [
        ("cls+layout", dict(cls=None, layout=2)), ("labels+ns=0", dict(labels=None, ns=0)),
        ("dir without nb", dict(nb=0)), ("nb without dir", dict(dir=None)), ("nb=9 without dir", dict(nb=9, dir=None)),
        ("ns=17+layout", dict(ns=17, layout=2)), ("nb=1+layout", dict(nb=1, layout=2)),
        ("B=0", dict(B=0)), ("H=0", dict(H=0)), ("W=-1", dict(W=-1)), ("C=0", dict(C=0)), ("C=0+index P=0", dict(C=0, index=P, P=0)),
        ("B=65536", dict(B=65536)), ("C=65", dict(C=65)), ("B=65536+C=65", dict(B=65536, C=65)), ("C=65+H*W", dict(C=65, H=BIG, W=BIG)),
        ("B=65536+H*W", dict(B=65536, H=BIG, W=BIG)),
    ],
    "center_decode": HEAD + LAYOUT + LADDER_CELLS + INDEX + [
        (f, {f: None}) for f in ("hm", "reg", "height", "dim", "rot", "boxes", "scores", "labels")] + [
        ("hm+layout", dict(hm=None, layout=2)),
        ("B=0", dict(B=0)), ("H=0", dict(H=0)), ("W=-1", dict(W=-1)), ("C=0", dict(C=0)), ("C=0+index P=0", dict(C=0, index=P, P=0)),
        ("B=65536", dict(B=65536)), ("C=65", dict(C=65)), ("B=65536+C=65", dict(B=65536, C=65)), ("C=65+H*W", dict(C=65, H=BIG, W=BIG)),
    ],
    "anchor_targets": HEAD[:2] + [("struct_size+H=0", dict(struct_size=8, H=0))] + ANCHOR_SET + LADDER_A + GT + [
        (f, {f: None}) for f in ("labels", "match", "reg_target", "max_iou")] + [
        ("labels+H=0", dict(labels=None, H=0)), ("H=0", dict(H=0)), ("W=-1", dict(W=-1)), ("H=0+ns=0", dict(H=0, ns=0)),
        ("dir_target without nb", dict(nb=0)), ("nb without dir_target", dict(dir_target=None)),
        ("nb=1+B=0", dict(nb=1, B=0)), ("B=0+ns=17", dict(B=0, ns=17)), ("G=1025+ns=17", dict(G=1025, ns=17)),
        ("size 0", dict(sizes=SIZES3[:4] + (0.0,) + SIZES3[5:])), ("size -1", dict(sizes=(-1.0,) + SIZES3[1:])),
        ("size nan", dict(sizes=SIZES3[:8] + (float("nan"),))), ("size 0+workspace", dict(sizes=(0.0,) + SIZES3[1:], workspace=None)),
        ("size 0+H*W", dict(sizes=(0.0,) + SIZES3[1:], H=BIG, W=BIG)), ("unused size", dict(ns=4)),
        ("workspace", dict(workspace=None)), ("workspace+H*W", dict(workspace=None, H=BIG, W=BIG)),
        ("G=1025+H*W", dict(G=1025, H=BIG, W=BIG)), ("B=65536+H*W", dict(B=65536, H=BIG, W=BIG)),
    ],
    "center_targets": HEAD + LAYOUT[:2] + LADDER_CELLS + GT + [
        ("heatmap", dict(heatmap=None)), ("heatmap+layout", dict(heatmap=None, layout=2)), ("layout+H=0", dict(layout=2, H=0)),
        ("H=0", dict(H=0)), ("W=-1", dict(W=-1)), ("C=0", dict(C=0)), ("C=0+B=0", dict(C=0, B=0)),
        ("ind", dict(ind=None)), ("anno", dict(anno=None)), ("G=1025+ind", dict(G=1025, ind=None)), ("ind+sx", dict(ind=None, sx=0.0)),
        ("sx=0", dict(sx=0.0)), ("sy<0", dict(sy=-0.4)), ("sx nan", dict(sx=float("nan"))), ("sx+min_overlap", dict(sx=0.0, min_overlap=1.0)),
        ("min_overlap=0", dict(min_overlap=0.0)), ("min_overlap=1", dict(min_overlap=1.0)), ("min_overlap+min_radius", dict(min_overlap=1.0, min_radius=65)),
        ("min_radius=-1", dict(min_radius=-1)), ("min_radius=65", dict(min_radius=65)), ("min_radius+vel", dict(min_radius=65, D=8)),
        ("vel D=8", dict(D=8)), ("vel D=8+C=65", dict(D=8, C=65)), ("C=65", dict(C=65)), ("C=65+H*W", dict(C=65, H=BIG, W=BIG)),
        ("B=65536+C=65", dict(B=65536, C=65)),
    ],
    "anchor_head_loss": HEAD + LAYOUT[:3] + [
        (f, {f: None}) for f in ("cls", "reg", "labels", "reg_target", "loss", "num_pos", "grad_cls", "grad_reg", "workspace")] + [
        ("cls+layout", dict(cls=None, layout=2)),
        ("B=0", dict(B=0)), ("H=0", dict(H=0)), ("W=-1", dict(W=-1)), ("A=0", dict(A=0)), ("C=0", dict(C=0)), ("A=0+nb=1", dict(A=0, nb=1)),
        ("nb=1", dict(nb=1)), ("nb=-2", dict(nb=-2)), ("nb=1+beta", dict(nb=1, beta=0.0)),
        ("dir without nb", dict(nb=0)), ("nb without dir", dict(dir=None)), ("nb without dir_target", dict(dir_target=None)),
        ("nb without grad_dir", dict(grad_dir=None)), ("nb=0 with grad_dir", dict(nb=0, dir=None, dir_target=None)),
        ("nb without dir+beta", dict(dir=None, beta=-1.0)),
        ("beta=0", dict(beta=0.0)), ("beta nan", dict(beta=float("nan"))), ("beta+alpha", dict(beta=0.0, alpha=2.0)),
        ("alpha<0", dict(alpha=-0.1)), ("alpha>1", dict(alpha=1.5)), ("alpha+B=65536", dict(alpha=1.5, B=65536)),
        ("B=65536", dict(B=65536)), ("C=65", dict(C=65)), ("B=65536+C=65", dict(B=65536, C=65)), ("C=65+A=129", dict(C=65, A=129)),
        ("A=129", dict(A=129)), ("nb=9", dict(nb=9)), ("A=129+H*W", dict(A=129, H=BIG, W=BIG)),
        ("H*W", dict(H=BIG, W=BIG)), ("H*W=2^31", dict(H=1 << 16, W=HALF)), ("H*W=2^60", dict(B=1, H=1 << 30, W=1 << 30)),
        ("K=2^31", dict(B=1, H=HALF, W=HALF, A=2)), ("K=3*2^30", dict(B=1, H=HALF, W=HALF)), ("B*K=2^31", dict(B=2, H=HALF, W=HALF, A=1)),
        ("B*K", dict(B=65535, H=64, W=65, A=8)), ("B*K=2^31, A=128", dict(B=1 << 10, H=128, W=128, A=128)),
    ],
    "center_head_loss": HEAD + LAYOUT[:3] + LADDER_CELLS + [
        (f, {f: None}) for f in ("hm", "reg", "height", "dim", "rot", "heatmap", "loss", "num_pos", "grad_hm", "grad_reg", "grad_height",
                                 "grad_dim", "grad_rot", "workspace")] + [
        ("hm+vel", dict(hm=None, vel=None)), ("vel without grad_vel", dict(grad_vel=None)), ("grad_vel without vel", dict(vel=None)),
        ("vel+layout", dict(vel=None, layout=2)),
        ("B=0", dict(B=0)), ("H=0", dict(H=0)), ("W=-1", dict(W=-1)), ("C=0", dict(C=0)), ("G=-1", dict(G=-1)), ("G=-1+ind", dict(G=-1, ind=None)),
        ("ind", dict(ind=None)), ("anno", dict(anno=None)), ("ind+B=65536", dict(ind=None, B=65536)),
        ("B=65536", dict(B=65536)), ("C=65", dict(C=65)), ("G=1025", dict(G=1025)), ("B=65536+C=65", dict(B=65536, C=65)),
        ("C=65+G=1025", dict(C=65, G=1025)), ("G=1025+H*W", dict(G=1025, H=BIG, W=BIG)),
    ],
}
# the size functions: (name, arguments).  0 is their refusal; the sizes of a few accepted shapes are recorded too (nothing is launched)
SIZES = {
    "anchor_targets_workspace_bytes": [(2, 5), (1, 0), (65535, 1024), (0, 5), (-1, 5), (2, -1), (2, 1025), (70000, 5)],
    "anchor_head_loss_workspace_bytes": [
        (2, 5, 7, 6), (1, 1, 1, 1), (3, 3, 67, 9), (3, 5, 7, 11), (3, 9, 130, 32), (1, 3, 67, 128), (2, 64, 64, 8), (65535, 8, 8, 1),
        (0, 5, 7, 6), (65536, 5, 7, 6), (2, 0, 7, 6), (2, 5, 0, 6), (2, 5, 7, 0), (2, 5, 7, 129), (2, BIG, BIG, 1), (1, 1 << 30, 1 << 30, 1),
        (1, HALF, HALF, 2), (2, HALF, HALF, 1), (65535, 64, 64, 8), (65535, 64, 65, 8), (1 << 10, 128, 128, 128)],
    "center_head_loss_workspace_bytes": [
        (2, 5, 7, 5), (1, 1, 1, 0), (3, 9, 130, 65), (3, 40, 37, 1024), (1, 16, 16, 256), (1, 16, 16, 257),
        (0, 5, 7, 5), (65536, 5, 7, 5), (2, 0, 7, 5), (2, 5, 0, 5), (2, 5, 7, -1), (2, 5, 7, 1025), (2, BIG, BIG, 5),
        (1, 1 << 30, 1 << 30, 5), (2, HALF, HALF, 5), (65535, 256, 128, 5), (65535, 256, 129, 5)],
}


def _block(cls, base, ov):
    if ov is None:
        return None
    f = dict(base, **ov)
    a = cls()
    a.struct_size = ctypes.sizeof(cls) + f.pop("struct_size", 0)
    for k, v in f.items():
        if isinstance(v, tuple):
            for i, x in enumerate(v):
                getattr(a, k)[i] = x
        else:
            setattr(a, k, v)
    return a


def outcomes():
    """{case name: [return code, message] or a size} of every case, from the library that is loaded."""
    from sad_amd import _lib
    L = _lib.lib()
    table = {"anchor_decode": (_lib.AnchorDecodeArgs, L.sad_anchor_decode_f32, ANCHOR_DECODE),
             "center_decode": (_lib.CenterDecodeArgs, L.sad_center_decode_f32, CENTER_DECODE),
             "anchor_targets": (_lib.AnchorTargetsArgs, L.sad_anchor_targets_f32, ANCHOR_TARGETS),
             "center_targets": (_lib.CenterTargetsArgs, L.sad_center_targets_f32, CENTER_TARGETS),
             "anchor_head_loss": (_lib.AnchorHeadLossArgs, L.sad_anchor_head_loss_f32, ANCHOR_LOSS),
             "center_head_loss": (_lib.CenterHeadLossArgs, L.sad_center_head_loss_f32, CENTER_LOSS)}
    got = {}
    for entry, cases in CASES.items():
        cls, fn, base = table[entry]
        assert len({name for name, _ in cases}) == len(cases), f"{entry}: a case name occurs twice"
        for name, ov in cases:
            a = _block(cls, base, ov)
            code = fn(ctypes.byref(a) if a is not None else None, None)
            assert code in (-1, -2), f"{entry}: {name} was not refused on the host (code {code})"
            got[f"{entry}: {name}"] = [code, L.sad_last_error().decode()]
    for entry, calls in SIZES.items():
        for args in calls:
            got[f"{entry}{args}"] = getattr(L, "sad_" + entry)(*args)
    return got


def test_every_entry_case_is_a_refusal():
    """No entry of the fixture can reach a launch: an entry-point case has a non-zero return code.  And the tables name no accepted
    shape: the smallest refused row counts are exactly 2^31."""
    want = json.load(open(FIXTURE))
    for k, v in want.items():
        if isinstance(v, list):
            assert v[0] in (-1, -2) and v[1], k
    assert BIG * BIG >= 1 << 31 > (BIG - 1) * (BIG - 1) and 2 * HALF * HALF == 1 << 31
    assert sum(isinstance(v, list) for v in want.values()) == sum(len(c) for c in CASES.values())


def test_dense_refusals_match_the_recorded_ones(sad):
    want = json.load(open(FIXTURE))
    got = outcomes()
    assert sorted(got) == sorted(want), "the cases of this file and of the fixture differ"
    wrong = {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    assert not wrong, f"{len(wrong)} refusals changed (got, recorded): {wrong}"


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    res = outcomes()
    with open(FIXTURE, "w") as fh:
        json.dump(res, fh, indent=0, sort_keys=True)
        fh.write("\n")
    print(f"recorded {len(res)} refusals -> {FIXTURE}")
