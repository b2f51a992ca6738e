"""SPEC.md §26 without a GPU: the two forms of the reference (tests/dense_target_ref.py) agree bit for bit, every coverage
condition the GPU cases of tests/test_gpu_dense_target.py rely on holds on the reference, the round trips through the §25
reference decoders hold on the reference, and the C-ABI refuses what §26 says it refuses before any launch.  If a case misses
its coverage, change its generator, never the assertion."""
import ctypes

import numpy as np
import pytest

import dense_head_ref as dh
import dense_target_ref as ref

F = np.float32


def _bits(a):
    return a if a.dtype == bool else a.view(np.int32)


@pytest.mark.parametrize("name", ref.ALL_CASES)
def test_loop_form_equals_vectorised_form(name):
    want = ref.expected(name)
    got = ref.targets(ref.case(name), "loop")
    assert set(got) == set(want)
    for k in want:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (name, k)
        assert np.array_equal(_bits(got[k]), _bits(want[k]), equal_nan=False) or k == "r", f"{name} {k}"
    if "r" in want:
        assert np.array_equal(got["r"], want["r"], equal_nan=True), name


# ---- the coverage the GPU cases rely on ----------------------------------------------------------------------------------
def test_coverage_shapes():
    """What the shapes are for: a single cell, a partial wave, cells no multiple of 64, several workgroups per scene (9 x 130:
    19 tiles, so best[] crosses workgroups), A = 1, 6 and 128 (one, one and sixteen anchor chunks), G = 0, 1, 3, 65 (> one
    wave) and 1024 (the limit), B = 3 with differing padding."""
    a, c = ref.ANCHOR_SHAPES, ref.CENTER_SHAPES
    assert {s[0] * s[1] for s in a.values()} == {1, 35, 201, 1170} and {s[0] * s[1] for s in c.values()} >= {1, 35, 201, 1170}
    assert {s[3] * s[4] for s in a.values()} == {1, 6, 9, 11, 128}      # (9, 11: a full anchor chunk and a partial one of 1 and of 3)
    assert {(s[0] * s[1], s[3] * s[4]) for s in a.values()} >= {(201, 9), (35, 11)}
    assert {s[5] for s in a.values()} == {0, 1, 3, 65, 1024} and {s[4] for s in c.values()} == {0, 1, 3, 65, 1024}
    assert {s[6] for s in a.values()} == {0, 2, 4} and {s[7] for s in a.values()} == {True, False}
    for name in ("t:5x7", "t:9x130", "ct:9x130"):
        lab = ref.case(name)["gt_labels"]
        assert lab.shape[0] == 3 and len({int((row < 0).sum()) for row in lab}) == 3, name
    assert ref.case("t:3x67:any")["kw"]["size_class"] is None
    # the centre head's 16 x 16 tiles: more than one tile in x and in y
    assert ref.CENTER_SHAPES["ct:40x37:g1024"][:2] == (40, 37)


@pytest.mark.parametrize("name", ["t:3x67:128", "t:9x130", "t:3x67:any"])
def test_coverage_anchor_outcomes(name):
    e, c = ref.expected(name), ref.case(name)
    lab, m = e["labels"], e["max_iou"]
    kw = c["kw"]
    nr = len(kw["rotations"])
    A = len(kw["sizes"]) * nr
    s_of = (np.arange(lab.shape[1]) % A) // nr
    pos = lab >= 0
    assert ((lab == -2).any() and (lab == -1).any() and pos.any()), name
    assert (pos & e["forced"] & (m < kw["pos_thr"][s_of])).any(), f"{name}: no forced-only positive"
    assert (pos & ~e["forced"]).any(), f"{name}: no positive by threshold alone"
    assert (m == 1).any() and ((m > 0) & (m < 1)).any()
    assert set(np.unique(e["dir_target"][pos])) == set(range(kw["nb"])), name
    assert (e["dir_target"][~pos] == -1).all() and (e["match"][~pos] == -1).all() and (e["reg_target"][~pos] == 0).all()
    assert (c["gt_labels"][np.arange(lab.shape[0])[:, None], np.maximum(e["match"], 0)][pos] == lab[pos]).all()
    assert (e["best"] > 0).any() and (e["best"][c["gt_labels"] < 0] == 0).all()


def test_coverage_anchor_small():
    assert (ref.expected("t:1x1")["labels"] >= 0).all()                     # the one anchor is forced by the one box
    e = ref.expected("t:5x7:g0")
    assert (e["labels"] == -1).all() and (e["max_iou"] == 0).all() and (e["dir_target"] == -1).all()
    e = ref.expected("t:5x7:g1024")
    assert "dir_target" not in e and (e["labels"] >= 0).sum() > 100 and (e["match"].max() > 64)
    far = ref.case("t:far")
    assert abs(far["kw"]["origin"][0]) >= 1e5 and (ref.expected("t:far")["labels"] >= 0).any() and (ref.expected("t:far")["labels"] == -2).any()


def test_coverage_anchor_edges():
    e, c = ref.expected("t:edges"), ref.case("t:edges")
    lab, match, m, best, forced = e["labels"][0], e["match"][0], e["max_iou"][0], e["best"][0], e["forced"][0]
    k = lambda y, x, s, r: ((y * 7 + x) * 2 + s) * 2 + r                    # noqa: E731
    # boxes 0 and 1 equal the anchor: IoU exactly 1 >= pos_thr = 1.0; the tie goes to the lowest g; both force the anchor
    k0 = k(2, 2, 0, 0)
    assert m[k0] == 1 and lab[k0] == 0 and match[k0] == 0 and forced[k0] and best[0] == 1 and best[1] == 1
    assert (e["reg_target"][0, k0, [0, 1, 3, 4, 5, 6]] == 0).all()
    # its neighbours along x see exactly neg_thr: not below it, so ignored
    for kn in (k(2, 1, 0, 0), k(2, 3, 0, 0)):
        assert m[kn] == F(ref.THIRD) == c["kw"]["neg_thr"][0] and lab[kn] == -2 and not forced[kn]
    # box 2: best anchor below pos_thr but above neg_thr; box 3: below neg_thr too; both forced positives
    for g, below_neg in ((2, False), (3, True)):
        rows = np.nonzero(match == g)[0]
        assert len(rows) >= 1 and forced[rows].all() and (m[rows] < 1).all() and 0 < best[g] < 1
        assert (best[g] < c["kw"]["neg_thr"][0]) == below_neg
    assert best[4] == 0 and not (match == 4).any()                          # far outside: forces nothing
    assert best[5] == 0 and not (match == 5).any() and best[12] == 0        # a class no size takes; a padding row
    # yaw either side of PI4 and of PI - PI4: the rectangle turns, so the anchor of rotation 0 / of rotation pi/2 is the equal one
    for g, x, r in ((6, 0, 0), (7, 1, 1), (8, 2, 1), (9, 3, 0)):
        kk = k(0, x, 1, r)
        assert m[kk] == 1 and match[kk] == g and m[k(0, x, 1, 1 - r)] < 1, g
    assert match[k(0, 4, 1, 0)] == 10 and (match == 11).any()               # several turns either way
    assert set(np.unique(e["dir_target"][0][lab >= 0])) == {0, 1}
    assert (lab == -1).any() and (lab == -2).any()


def test_coverage_center():
    for name in ("ct:3x67", "ct:9x130", "ct:40x37:g1024"):
        e, c = ref.expected(name), ref.case(name)
        ind, hm = e["ind"], e["heatmap"]
        lab, C = c["gt_labels"], c["kw"]["C"]
        assert (ind >= 0).any() and (ind[(lab >= 0) & (lab < C)] < 0).any(), f"{name}: no centre outside the map"
        assert (lab == -1).any() and (lab == C).any() and (ind[(lab < 0) | (lab >= C)] == -1).all()
        assert len(np.unique(e["rad"][ind >= 0])) >= 2 and (e["anno"][ind < 0] == 0).all()
        assert (hm == 1).sum() >= 1 and ((hm > 0) & (hm < 1)).any()
        assert (hm == 0).any() or name == "ct:40x37:g1024"                   # (268 windows cover that map completely)
    e = ref.expected("ct:40x37:g1024")
    assert (e["ind"] >= 0).sum() > 256 and (e["heatmap"] == 1).sum() < (e["ind"] >= 0).sum()     # shared cells
    assert (ref.expected("ct:1x1")["heatmap"] == 1).all() and (ref.expected("ct:5x7:g0")["heatmap"] == 0).all()
    assert ref.expected("ct:5x7")["anno"].shape[-1] == 10 and (ref.expected("ct:5x7")["ind"] >= 0).all()


def test_coverage_center_edges():
    e, c = ref.expected("ct:edges"), ref.case("ct:edges")
    ind, rad, r, hm = e["ind"][0], e["rad"][0], e["r"][0], e["heatmap"][0]
    H, W = 21, 35
    assert ind[0] == 3 and e["anno"][0, 0, 0] == 0 and e["anno"][0, 0, 1] == 0          # on a cell boundary and on lo_y
    assert ind[1] == -1 and ind[2] == -1                                                # on hi: outside, not clamped
    assert r[3] < 4 <= r[4] and np.nextafter(r[3], F(9)) >= F(4) - F(1e-5) and rad[3] == 3 and rad[4] == 4
    assert r[5] < 2 and rad[5] == 2                                                     # min_radius takes over
    for g, (ix, iy) in zip(range(6, 14), ((0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1), (0, 10), (W - 1, 10), (17, 0), (17, H - 1))):
        assert ind[g] == iy * W + ix and rad[g] >= 2 and hm[1, iy, ix] == 1             # windows cut by corners and borders
    assert abs(ind[14] - ind[15]) == 2 and rad[14] + rad[15] >= 2                       # overlapping windows of one class
    assert ind[16] == ind[17] and ind[18] == ind[19] and hm[0, 15, 28] == 1 and hm[1, 15, 28] == 1
    assert (ind[20:24] == -1).all() and (e["anno"][0, 20:24] == 0).all()                # l <= 0; labels -1 and C
    # between the two overlapping boxes the larger contribution wins: the map exceeds what box 14 alone would draw
    alone = ref.center_targets_vec(c["gt_boxes"][:, 14:15], c["gt_labels"][:, 14:15], **c["kw"])["heatmap"][0, 0]
    assert (hm[0] > alone).any() and (hm[0] >= alone).all()


# ---- round trips on the reference ----------------------------------------------------------------------------------------
def test_anchor_round_trip_on_the_reference():
    c, out = ref.case("t:round"), ref.expected("t:round")
    assert abs(c["kw"]["origin"][0]) < 100
    kw = {k: c["kw"][k] for k in ("sizes", "z_center", "rotations", "origin", "step", "dir_offset")}
    boxes, _, _ = dh.anchor_decode_vec(*ref.decode_maps(c, out), **kw)
    ref.check_anchor_round_trip(c, out, boxes)


def test_center_round_trip_on_the_reference():
    c, out = ref.case("ct:round"), ref.expected("ct:round")
    ok = out["ind"] >= 0
    assert all(len(set(row[o])) == o.sum() for row, o in zip(out["ind"], ok))                 # one box per cell
    hm, reg, height, dim, rot, vel = ref.center_maps(c, out)
    index = np.where(ok, out["ind"], 0)
    boxes, _, _ = dh.center_decode_vec(hm, reg, height, dim, rot, vel, c["kw"]["origin"], c["kw"]["cell"], index=index)
    ref.check_center_round_trip(c, out, boxes)


# ---- the C-ABI without a GPU --------------------------------------------------------------------------------------------
P_ = 0x10000                                                                    # never dereferenced: every call fails on the host
EINVAL, EUNSUPPORTED = -1, -2


def _anchor_args(_lib, **over):
    a = _lib.AnchorTargetsArgs()
    a.struct_size = ctypes.sizeof(_lib.AnchorTargetsArgs)
    a.gt_boxes = a.gt_labels = a.labels = a.match = a.reg_target = a.max_iou = a.dir_target = a.workspace = P_
    a.B, a.G, a.D, a.H, a.W, a.ns, a.nr, a.nb, a.use_size_class = 1, 4, 7, 4, 4, 3, 2, 2, 1
    for i in range(9):
        a.sizes[i] = 1.5
    for k, v in over.items():
        setattr(a, k, v)
    return a


def _center_args(_lib, **over):
    a = _lib.CenterTargetsArgs()
    a.struct_size = ctypes.sizeof(_lib.CenterTargetsArgs)
    a.gt_boxes = a.gt_labels = a.heatmap = a.ind = a.anno = P_
    a.B, a.G, a.D, a.C, a.H, a.W, a.layout, a.min_radius, a.vel = 1, 4, 7, 3, 4, 4, 0, 2, 0
    a.sx, a.sy, a.min_overlap = 0.5, 0.5, 0.1
    for k, v in over.items():
        setattr(a, k, v)
    return a


def test_c_abi_refusals(sad):
    from sad_amd import _lib
    L = _lib.lib()
    assert hasattr(L, "sad_anchor_targets_f32") and hasattr(L, "sad_center_targets_f32")
    assert L.sad_version() == 4
    for fn, make, ptrs in ((L.sad_anchor_targets_f32, _anchor_args, ("gt_boxes", "gt_labels", "labels", "match", "reg_target", "max_iou", "workspace")),
                           (L.sad_center_targets_f32, _center_args, ("gt_boxes", "gt_labels", "heatmap", "ind", "anno"))):
        def rc(**over):
            return fn(ctypes.byref(make(_lib, **over)), None)
        assert fn(None, None) == EINVAL and b"NULL" in L.sad_last_error()
        size = ctypes.sizeof(make(_lib))
        for wrong in (size - 8, size + 8, 0):
            assert rc(struct_size=wrong) == EINVAL and b"struct_size" in L.sad_last_error()
        for p in ptrs:
            assert rc(**{p: None}) == EINVAL and b"NULL" in L.sad_last_error(), p
        assert rc(G=1025) == EUNSUPPORTED and b"1024" in L.sad_last_error()
        assert rc(G=-1) == EINVAL and rc(D=6) == EINVAL
        for k in ("B", "H", "W"):
            assert rc(**{k: 0}) == EINVAL, k
        assert rc(B=65536) == EUNSUPPORTED and b"65535" in L.sad_last_error()
    a = lambda **over: L.sad_anchor_targets_f32(ctypes.byref(_anchor_args(_lib, **over)), None)    # noqa: E731
    assert a(nb=1) == EINVAL and a(nb=-2) == EINVAL and a(nb=9) == EUNSUPPORTED
    assert a(nb=0) == EINVAL and b"together" in L.sad_last_error()             # dir_target given, nb = 0
    assert a(dir_target=None) == EINVAL and b"together" in L.sad_last_error()  # nb = 2, no dir_target
    assert a(ns=0) == EINVAL and a(nr=0) == EINVAL and a(ns=17) == EUNSUPPORTED and a(nr=9) == EUNSUPPORTED
    for bad in (0.0, -1.0):
        args = _anchor_args(_lib)
        args.sizes[4] = bad
        assert L.sad_anchor_targets_f32(ctypes.byref(args), None) == EINVAL and b"anchor size 1" in L.sad_last_error()
    assert a(H=16384, W=16384, ns=1, nr=8) == EUNSUPPORTED and b"2^31" in L.sad_last_error()
    wb = L.sad_anchor_targets_workspace_bytes
    assert wb(3, 65) == 3 * 65 * 4 and wb(65535, 1024) == 65535 * 1024 * 4 and wb(2, 0) == 0
    assert wb(0, 4) == 0 and wb(1, 1025) == 0 and wb(1, -1) == 0
    c = lambda **over: L.sad_center_targets_f32(ctypes.byref(_center_args(_lib, **over)), None)    # noqa: E731
    assert c(C=0) == EINVAL and c(C=65) == EUNSUPPORTED
    assert c(layout=2) == EINVAL and b"layout" in L.sad_last_error()
    assert c(sx=0.0) == EINVAL and c(min_overlap=0.0) == EINVAL and c(min_overlap=1.0) == EINVAL
    assert c(min_radius=-1) == EINVAL and c(min_radius=65) == EINVAL
    assert c(vel=1) == EINVAL and b"D >= 9" in L.sad_last_error()
    assert c(B=32768, H=256, W=256) == EUNSUPPORTED and b"2^31" in L.sad_last_error()


def test_wrappers_name_the_wrong_argument(sad):
    import torch
    from sad_amd import dense_head, ops
    kw = dict(H=4, W=5, sizes=[[3.9, 1.6, 1.56]], z_center=[-1.0], rotations=[0.0, 1.57], origin=(0.0, -40.0), step=(0.4, 0.4),
              pos_thr=0.6, neg_thr=0.45)
    gt, lab = torch.zeros(1, 3, 7), torch.zeros(1, 3, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="gt_boxes: .*no CPU path"):
        ops.anchor_targets(gt, lab, **kw)
    with pytest.raises(TypeError, match="gt_labels: expected dtype torch.int32"):
        ops.anchor_targets(gt, lab.long(), **kw)
    with pytest.raises(ValueError, match="gt_boxes: expected \\[B,G,D\\]"):
        ops.anchor_targets(torch.zeros(1, 3, 6), lab, **kw)
    with pytest.raises(ValueError, match="gt_labels: expected shape"):
        ops.anchor_targets(gt, torch.zeros(1, 4, dtype=torch.int32), **kw)
    with pytest.raises(TypeError, match="gt_boxes: expected dtype torch.float32"):
        ops.anchor_targets(gt.double(), lab, **kw)
    with pytest.raises(TypeError, match="gt_boxes: expected a torch.Tensor"):
        ops.anchor_targets(gt.numpy(), lab, **kw)
    with pytest.raises(ValueError, match="gt_boxes / gt_labels: must be contiguous"):
        ops.anchor_targets(torch.zeros(1, 7, 3).transpose(1, 2), lab, **kw)
    with pytest.raises(ValueError, match="gt_boxes / gt_labels: must be contiguous"):
        ops.anchor_targets(gt, torch.zeros(1, 6, dtype=torch.int32)[:, ::2], **kw)
    with pytest.raises(TypeError, match="gt_labels: expected dtype"):         # both dtypes are judged before any shape
        ops.anchor_targets(torch.zeros(1, 3, 6), lab.long(), **kw)
    with pytest.raises(ValueError, match="at most 1024"):                      # G before contiguity
        ops.anchor_targets(torch.zeros(1, 7, 1025).transpose(1, 2), torch.zeros(1, 1025, dtype=torch.int32), **kw)
    with pytest.raises(ValueError, match="at most 1024"):
        ops.anchor_targets(torch.zeros(1, 1025, 7), torch.zeros(1, 1025, dtype=torch.int32), **kw)
    with pytest.raises(ValueError, match="sizes: every anchor extent"):
        ops.anchor_targets(gt, lab, **dict(kw, sizes=[[3.9, 0.0, 1.56]]))
    with pytest.raises(ValueError, match="pos_thr: expected one value per anchor size"):
        ops.anchor_targets(gt, lab, **dict(kw, pos_thr=[0.6, 0.5]))
    with pytest.raises(ValueError, match="nb: "):
        ops.anchor_targets(gt, lab, nb=1, **kw)
    ckw = dict(C=3, H=4, W=5, origin=(-54.0, -54.0), cell=(0.6, 0.6))
    with pytest.raises(RuntimeError, match="gt_boxes: .*no CPU path"):
        ops.center_targets(gt, lab, **ckw)
    with pytest.raises(ValueError, match="gt_boxes: expected \\[B,G,D\\] with B >= 1 and D >= 9"):
        ops.center_targets(gt, lab, vel=True, **ckw)
    with pytest.raises(ValueError, match="gt_labels: expected shape"):
        ops.center_targets(gt, torch.zeros(1, 4, dtype=torch.int32), **ckw)
    with pytest.raises(TypeError, match="gt_labels: expected dtype torch.int32"):
        ops.center_targets(gt, lab.short(), **ckw)
    with pytest.raises(ValueError, match="min_overlap"):
        ops.center_targets(gt, lab, min_overlap=1.0, **ckw)
    with pytest.raises(ValueError, match="layout"):
        ops.center_targets(gt, lab, layout="chwn", **ckw)
    assert sad.anchor_targets is ops.anchor_targets and sad.center_targets is ops.center_targets
    assert sad.AnchorTargetAssigner is dense_head.AnchorTargetAssigner and sad.CenterTargetAssigner is dense_head.CenterTargetAssigner
    dec = dense_head.AnchorHeadDecoder(kw["sizes"], kw["z_center"], kw["rotations"], kw["origin"], kw["step"])
    asg = dec.assigner(0.6, 0.45, [0], nb=2)
    assert asg.num_anchors == 2 and asg.origin == dec.origin and asg.step == dec.step and not list(asg.parameters())
    casg = dense_head.CenterHeadDecoder((-54.0, -54.0), (0.6, 0.6), layout="nhwc").assigner(3, vel=True)
    assert (casg.C, casg.cell, casg.layout, casg.vel) == (3, (0.6, 0.6), "nhwc", True)
