"""SPEC.md §25 without a GPU: the two forms of the reference (tests/dense_head_ref.py) agree bit for bit, the reference agrees
with an independent float64 restatement of the OpenPCDet formulas, anchor_grid is OpenPCDet's grid, the C-ABI refuses what
§25 says it refuses before any launch, the Python wrappers name a wrong argument, and every coverage condition the GPU cases
of tests/test_gpu_dense_head.py rely on holds on the reference.  If a case misses its coverage, change its generator, never
the assertion."""
import ctypes

import numpy as np
import pytest

import dense_head_ref as ref

F = np.float32


def _bits_equal(a, b, what):
    for name, x, y in zip(("boxes", "scores", "labels"), a, b):
        assert x.dtype == y.dtype and x.shape == y.shape, (what, name, x.dtype, y.dtype, x.shape, y.shape)
        assert np.array_equal(x.view(np.int32), y.view(np.int32)), f"{what} {name}: {int((x.view(np.int32) != y.view(np.int32)).sum())} words differ"


@pytest.mark.parametrize("name", ref.ALL_CASES)
def test_loop_form_equals_vectorised_form(name):
    c = ref.case(name)
    _bits_equal(ref.decode(c, "loop"), ref.expected(name)[:3], name)
    for label, index in ref.index_cases(name).items():
        _bits_equal(ref.decode(c, "loop", index=index), ref.decode(c, "vec", index=index), f"{name} index:{label}")


def test_e2e_case_forms_agree():
    c = ref.e2e_case()
    _bits_equal(ref.decode(c, "loop"), ref.decode(c, "vec"), "e2e")


# ---- an independent float64 restatement of the OpenPCDet formulas -----------------------------------------------------
def _limit_period(val, offset, period):
    return val - np.floor(val / period + offset) * period


def _pcdet_anchor(c):
    """AnchorGenerator (sizes outer, rotations inner) -> ResidualCoder.decode_torch -> the direction fix of
    AnchorHeadTemplate.generate_predicted_boxes -> sigmoid / max, all in float64 on the float32 inputs."""
    kw = c["kw"]
    cls, reg, dir_ = (None if m is None else m.astype(np.float64) for m in (c["cls"], c["reg"], c["dir"]))
    sizes, zc, rots = (np.asarray(kw[k], F).astype(np.float64) for k in ("sizes", "z_center", "rotations"))
    B, _, H, W = cls.shape
    ns, nr = len(sizes), len(rots)
    A = ns * nr
    xs = float(F(kw["origin"][0])) + np.arange(W) * float(F(kw["step"][0]))
    ys = float(F(kw["origin"][1])) + np.arange(H) * float(F(kw["step"][1]))
    anchors = np.zeros((H, W, ns, nr, 7))
    anchors[..., 0] = xs[None, :, None, None]
    anchors[..., 1] = ys[:, None, None, None]
    anchors[..., 2] = zc[None, None, :, None]
    anchors[..., 3:6] = sizes[None, None, :, None, :]
    anchors[..., 6] = rots[None, None, None, :]
    anchors = anchors.reshape(1, H * W * A, 7)
    t = reg.transpose(0, 2, 3, 1).reshape(B, -1, 7)                             # permute(0,2,3,1).view(B,-1,7)
    xa, ya, za, dxa, dya, dza, ra = (anchors[..., i] for i in range(7))
    diag = np.sqrt(dxa ** 2 + dya ** 2)
    with np.errstate(over="ignore"):
        box = np.stack([t[..., 0] * diag + xa, t[..., 1] * diag + ya, t[..., 2] * dza + za, np.exp(t[..., 3]) * dxa,
                        np.exp(t[..., 4]) * dya, np.exp(t[..., 5]) * dza, t[..., 6] + ra], -1)
    period = None
    if dir_ is not None:
        nb = dir_.shape[1] // A
        labels = np.argmax(dir_.transpose(0, 2, 3, 1).reshape(B, -1, nb), -1)
        period = 2 * np.pi / nb
        doff = float(F(kw["dir_offset"]))
        rot = _limit_period(box[..., 6] - doff, float(F(kw["dir_limit_offset"])), period)
        box[..., 6] = rot + doff + period * labels
    logits = cls.transpose(0, 2, 3, 1).reshape(B, -1, cls.shape[1] // A)
    score = 1.0 / (1.0 + np.exp(-logits))
    return box, score.max(-1), np.argmax(score, -1), period


def _pcdet_center(c):
    """CenterPoint's decode_bbox_from_heatmap without its top-k: every cell of every map, float64."""
    kw = c["kw"]
    hm, reg, height, dim, rot = (c[k].astype(np.float64) for k in ("hm", "reg", "height", "dim", "rot"))
    B, C, H, W = hm.shape
    xs = np.arange(W)[None, None, :] + reg[:, 0]
    ys = np.arange(H)[None, :, None] + reg[:, 1]
    with np.errstate(over="ignore"):
        d = np.exp(dim) if kw["log_dim"] else dim
    cols = [xs * float(F(kw["cell"][0])) + float(F(kw["origin"][0])), ys * float(F(kw["cell"][1])) + float(F(kw["origin"][1])),
            height[:, 0], d[:, 0], d[:, 1], d[:, 2], np.arctan2(rot[:, 0], rot[:, 1])]
    if c["vel"] is not None:
        cols += [c["vel"][:, 0].astype(np.float64), c["vel"][:, 1].astype(np.float64)]
    score = 1.0 / (1.0 + np.exp(-hm))
    return np.stack(cols, -1).reshape(B, H * W, -1), score.transpose(0, 2, 3, 1).reshape(B, H * W, C)


def _close(got, want, scale, what):
    """1e-5 relative, on the scale of the operands where a sum cancels; inf == inf; +-1e-30 where float32 underflows."""
    got, want = got.astype(np.float64), np.asarray(want, np.float64)
    fin = np.isfinite(want) & (np.abs(want) < 3e38)
    assert np.array_equal(got[~fin], np.where(np.isfinite(want[~fin]), np.inf * np.sign(want[~fin]), want[~fin])), what
    err = np.abs(got[fin] - want[fin])
    assert (err <= 1e-5 * np.maximum(np.abs(want[fin]), scale) + 1e-30).all(), (what, float(err.max()))


@pytest.mark.parametrize("name", ref.ANCHOR_CASES)
def test_anchor_reference_is_openpcdet(name):
    c = ref.case(name)
    boxes, scores, labels, aux = ref.expected(name)
    wbox, wscore, wlabel, period = _pcdet_anchor(c)
    scale = max(1.0, float(np.abs(np.asarray(c["kw"]["origin"])).max()))
    for j, col in enumerate("cx cy cz l w h".split()):
        _close(boxes[..., j], wbox[..., j], scale if j < 3 else 0.0, f"{name} {col}")
    d = boxes[..., 6].astype(np.float64) - wbox[..., 6]
    if period is not None:                                # a v within rounding of a multiple of the period may take the other q
        d = (d + period / 2) % period - period / 2
    assert (np.abs(d) <= 1e-5 * np.maximum(np.abs(wbox[..., 6]), 2 * np.pi)).all(), (name, float(np.abs(d).max()))
    _close(scores, wscore, 0.0, f"{name} score")
    # labels: equal wherever the float64 sigmoid still separates the classes (it saturates to 1.0 above ~37)
    sat = wscore >= 1.0
    assert np.array_equal(labels[~sat], wlabel[~sat]), name


@pytest.mark.parametrize("name", ref.CENTER_CASES)
def test_center_reference_is_centerpoint(name):
    c = ref.case(name)
    kw = dict(c["kw"], peak=False)
    boxes, scores, labels = ref.center_decode_vec(*ref.maps_of(c), **kw)
    wbox, wscore = _pcdet_center(c)
    scale = max(1.0, float(np.abs(np.asarray(c["kw"]["origin"])).max()))
    D = wbox.shape[-1]
    assert boxes.shape[-1] == D == (9 if c["vel"] is not None else 7)
    for j in range(D):
        if j == 6:
            d = boxes[..., 6].astype(np.float64) - wbox[..., 6]
            d = (d + np.pi) % (2 * np.pi) - np.pi
            assert (np.abs(d) <= 1e-5 * np.pi).all(), name
        else:
            _close(boxes[..., j], wbox[..., j], scale if j < 2 else 0.0, f"{name} column {j}")
    _close(scores, wscore.max(-1), 0.0, f"{name} score")
    assert np.array_equal(labels, np.argmax(wscore, -1)), name
    # peak = CenterNet's test: max_pool2d(3, stride 1, padding 1) == hm, padding with -inf
    hm = c["hm"]
    pad = np.full((hm.shape[0], hm.shape[1], hm.shape[2] + 2, hm.shape[3] + 2), -np.inf, F)
    pad[:, :, 1:-1, 1:-1] = hm
    pooled = np.max([pad[:, :, dy:dy + hm.shape[2], dx:dx + hm.shape[3]] for dy in range(3) for dx in range(3)], 0)
    assert np.array_equal(ref.peak_mask(hm), pooled == hm)


def test_anchor_grid_is_openpcdets():
    from sad_amd import dense_head
    H, W = 200, 176
    origin, step = dense_head.anchor_grid(ref.KITTI_RANGE, H, W)
    assert (origin, step) == ref.anchor_grid(ref.KITTI_RANGE, H, W)
    for n, lo, hi, o, s in ((W, 0.0, 70.4, origin[0], step[0]), (H, -40.0, 40.0, origin[1], step[1])):
        assert s == float(F((hi - lo) / (n - 1)))
        want = np.arange(lo, hi + 1e-5, (hi - lo) / (n - 1))                  # AnchorGenerator's x_shifts / y_shifts
        assert len(want) == n
        got = F(o) + (np.arange(n).astype(F) * F(s))                            # §25.1's xa / ya
        # "to float32": no float32 (origin, step) can do better than the roundings §25.1 prescribes: the step's own (half an ulp
        # of the step, n - 1 times at the far end), the product's (half an ulp of the span) and the sum's (half an ulp of the
        # larger end of the range).  That bound, from the number formats alone, is about two ulps of the range:
        half_ulp = lambda v: float(np.spacing(F(abs(v)))) / 2                   # noqa: E731
        bound = (n - 1) * half_ulp(s) + half_ulp(hi - lo) + half_ulp(max(abs(lo), abs(hi)))
        err = np.abs(got.astype(np.float64) - want)
        print(f"anchor_grid n={n}: max |error| {err.max():.3g} m, bound {bound:.3g} m, exact at {int((got == want.astype(F)).sum())} of {n}")
        assert (err <= bound).all() and bound < 3 * float(np.spacing(F(max(abs(lo), abs(hi)))))
        assert got[0] == F(lo) and abs(float(got[-1]) - hi) <= float(np.spacing(F(hi)))
    assert dense_head.anchor_grid(ref.KITTI_RANGE, 1, 1) == ((0.0, -40.0), (0.0, 0.0))
    with pytest.raises(ValueError):
        dense_head.anchor_grid(ref.KITTI_RANGE, 0, 4)


# ---- the C-ABI without a GPU --------------------------------------------------------------------------------------------
P_ = 0x10000                                                                    # never dereferenced: every call fails on the host
EINVAL, EUNSUPPORTED = -1, -2


def _anchor_args(_lib, **over):
    a = _lib.AnchorDecodeArgs()
    a.struct_size = ctypes.sizeof(_lib.AnchorDecodeArgs)
    a.cls = a.reg = a.dir = a.boxes = a.scores = a.labels = P_
    a.B, a.H, a.W, a.C, a.nb, a.ns, a.nr, a.layout, a.P = 1, 4, 4, 3, 2, 3, 2, 0, 0
    for k, v in over.items():
        setattr(a, k, v)
    return a


def _center_args(_lib, **over):
    a = _lib.CenterDecodeArgs()
    a.struct_size = ctypes.sizeof(_lib.CenterDecodeArgs)
    a.hm = a.reg = a.height = a.dim = a.rot = a.vel = a.boxes = a.scores = a.labels = P_
    a.B, a.H, a.W, a.C, a.layout, a.P = 1, 4, 4, 3, 0, 0
    for k, v in over.items():
        setattr(a, k, v)
    return a


def test_c_abi_refusals(sad):
    from sad_amd import _lib
    L = _lib.lib()
    assert hasattr(L, "sad_anchor_decode_f32") and hasattr(L, "sad_center_decode_f32")
    assert L.sad_version() == 4
    for fn, make, ptrs in ((L.sad_anchor_decode_f32, _anchor_args, ("cls", "reg", "boxes", "scores", "labels")),
                           (L.sad_center_decode_f32, _center_args, ("hm", "reg", "height", "dim", "rot", "boxes", "scores", "labels"))):
        def rc(**over):
            return fn(ctypes.byref(make(_lib, **over)), None)
        assert fn(None, None) == EINVAL
        size = ctypes.sizeof(make(_lib))
        for wrong in (size - 8, size + 8, 0):
            assert rc(struct_size=wrong) == EINVAL and b"struct_size" in L.sad_last_error()
        for p in ptrs:
            assert rc(**{p: None}) == EINVAL and b"NULL" in L.sad_last_error(), p
        for layout in (-1, 2):
            assert rc(layout=layout) == EINVAL and b"layout" in L.sad_last_error()
        for k in ("B", "H", "W", "C"):
            assert rc(**{k: 0}) == EINVAL, k
        assert rc(B=65536) == EUNSUPPORTED and b"65535" in L.sad_last_error()
        assert rc(C=65) == EUNSUPPORTED and b"64" in L.sad_last_error()
        assert rc(index=P_, P=0) == EINVAL
        assert rc(index=P_, P=2 ** 31 - 1, B=2) == EUNSUPPORTED
    a = lambda **over: L.sad_anchor_decode_f32(ctypes.byref(_anchor_args(_lib, **over)), None)    # noqa: E731
    assert a(ns=0) == EINVAL and a(nr=0) == EINVAL
    assert a(ns=17) == EUNSUPPORTED and a(nr=9) == EUNSUPPORTED
    assert a(nb=1) == EINVAL and a(nb=-2) == EINVAL
    assert a(nb=9) == EUNSUPPORTED
    assert a(nb=0) == EINVAL and b"together" in L.sad_last_error()             # dir given, nb = 0
    assert a(dir=None) == EINVAL and b"together" in L.sad_last_error()         # nb = 2, no dir
    # B * K < 2^31: K = H * W * A
    assert a(H=16384, W=16384, ns=1, nr=8) == EUNSUPPORTED and b"2^31" in L.sad_last_error()
    assert a(B=4, H=8192, W=8192, ns=4, nr=2) == EUNSUPPORTED
    c = lambda **over: L.sad_center_decode_f32(ctypes.byref(_center_args(_lib, **over)), None)    # noqa: E731
    assert c(H=65536, W=32768) == EUNSUPPORTED and b"2^31" in L.sad_last_error()
    assert c(B=32768, H=256, W=256) == EUNSUPPORTED


def test_wrappers_name_the_wrong_argument(sad):
    import torch
    from sad_amd import ops
    kw = dict(sizes=[[3.9, 1.6, 1.56]], z_center=[-1.0], rotations=[0.0, 1.57], origin=(0.0, -40.0), step=(0.4, 0.4))
    A, C, H, W = 2, 3, 4, 5
    cls, reg, dir_ = torch.zeros(1, A * C, H, W), torch.zeros(1, A * 7, H, W), torch.zeros(1, A * 2, H, W)
    with pytest.raises(RuntimeError, match="cls: .*no CPU path"):
        ops.anchor_decode(cls, reg, dir_, **kw)
    with pytest.raises(ValueError, match="cls: .*multiple of A"):
        ops.anchor_decode(torch.zeros(1, 7, H, W), reg, dir_, **kw)
    with pytest.raises(ValueError, match="reg: expected A \\* 7"):
        ops.anchor_decode(cls, torch.zeros(1, A * 6, H, W), dir_, **kw)
    with pytest.raises(ValueError, match="dir: "):
        ops.anchor_decode(cls, reg, torch.zeros(1, A, H, W), **kw)
    with pytest.raises(ValueError, match="reg: expected shape"):
        ops.anchor_decode(cls, torch.zeros(1, A * 7, H, W + 1), dir_, **kw)
    with pytest.raises(ValueError, match="reg: must be contiguous"):
        ops.anchor_decode(cls, torch.zeros(1, H, W, A * 7).permute(0, 3, 1, 2), dir_, **kw)
    with pytest.raises(ValueError, match="cls: must be contiguous"):
        ops.anchor_decode(torch.zeros(1, A * C, H, W).permute(0, 2, 3, 1), reg, dir_, layout="nhwc", **kw)
    with pytest.raises(TypeError, match="cls: expected dtype"):
        ops.anchor_decode(cls.double(), reg, dir_, **kw)
    with pytest.raises(TypeError, match="index: expected dtype torch.int32"):
        ops.anchor_decode(cls, reg, dir_, index=torch.zeros(1, 4, dtype=torch.int64), **kw)
    with pytest.raises(ValueError, match="index: expected \\[B,P\\]"):
        ops.anchor_decode(cls, reg, dir_, index=torch.zeros(2, 4, dtype=torch.int32), **kw)
    with pytest.raises(ValueError, match="index: must be contiguous"):
        ops.anchor_decode(cls, reg, dir_, index=torch.zeros(1, 8, dtype=torch.int32)[:, ::2], **kw)
    with pytest.raises(TypeError, match="reg: expected a torch.Tensor"):
        ops.anchor_decode(cls, reg.numpy(), dir_, **kw)
    with pytest.raises(TypeError, match="dir: expected dtype torch.float32"):
        ops.anchor_decode(cls, reg, dir_.half(), **kw)
    with pytest.raises(ValueError, match="cls: .*multiple of A"):          # channel count before dtype, cls before reg
        ops.anchor_decode(torch.zeros(1, 7, H, W).half(), torch.zeros(1, A * 6, H, W), dir_, **kw)
    with pytest.raises(ValueError, match="layout"):
        ops.anchor_decode(cls, reg, dir_, layout="chwn", **kw)
    with pytest.raises(ValueError, match="z_center"):
        ops.anchor_decode(cls, reg, dir_, **dict(kw, z_center=[0.0, 1.0]))
    ckw = dict(origin=(-54.0, -54.0), cell=(0.6, 0.6))
    hm, r2, h1, d3 = torch.zeros(1, 3, H, W), torch.zeros(1, 2, H, W), torch.zeros(1, 1, H, W), torch.zeros(1, 3, H, W)
    with pytest.raises(RuntimeError, match="hm: .*no CPU path"):
        ops.center_decode(hm, r2, h1, d3, r2, r2, **ckw)
    with pytest.raises(ValueError, match="dim: expected 3 channels"):
        ops.center_decode(hm, r2, h1, r2, r2, **ckw)
    with pytest.raises(ValueError, match="vel: expected 2 channels"):
        ops.center_decode(hm, r2, h1, d3, r2, d3, **ckw)
    with pytest.raises(ValueError, match="rot: must be contiguous"):
        ops.center_decode(hm, r2, h1, d3, torch.zeros(1, H, W, 2).permute(0, 3, 1, 2), **ckw)
    with pytest.raises(TypeError, match="index: expected dtype torch.int32"):
        ops.center_decode(hm, r2, h1, d3, r2, index=torch.zeros(1, 4), **ckw)
    with pytest.raises(TypeError, match="height: expected dtype"):
        ops.center_decode(hm, r2, h1.half(), d3, r2, **ckw)
    with pytest.raises(ValueError, match="reg: expected shape"):
        ops.center_decode(hm, torch.zeros(1, 2, H + 1, W), h1, d3, r2, **ckw)
    with pytest.raises(ValueError, match="hm: must be contiguous"):
        ops.center_decode(torch.zeros(1, H, W, 3).permute(0, 3, 1, 2), r2, h1, d3, r2, **ckw)
    with pytest.raises(ValueError, match="hm: needs at least one class channel"):      # before the other maps
        ops.center_decode(torch.zeros(1, 0, H, W), r2, h1.half(), d3, r2, **ckw)


def test_lazy_exports(sad):
    from sad_amd import dense_head, ops
    assert sad.anchor_decode is ops.anchor_decode and sad.center_decode is ops.center_decode
    assert sad.AnchorHeadDecoder is dense_head.AnchorHeadDecoder and sad.CenterHeadDecoder is dense_head.CenterHeadDecoder
    assert sad.anchor_grid is dense_head.anchor_grid


# ---- the coverage the GPU cases rely on ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n, s in ref.ANCHOR_SHAPES.items() if s[0] * s[1] * s[3] * s[4] >= 200])
def test_coverage_labels_and_bins(name):
    H, W, B, ns, nr, C, nb = ref.ANCHOR_SHAPES[name]
    _, _, labels, aux = ref.expected(name)
    assert set(np.unique(labels)) == set(range(C)), name
    if nb:
        assert set(np.unique(aux["bin"])) == set(range(nb)), name
        assert (aux["q"] != 0).any() and (aux["q"] > 0).any() and (aux["q"] < 0).any(), name


def test_coverage_tiles():
    """What the shapes are for: a partial wave, rows crossing one and two 64-lane boundaries, K no multiple of 256, more than
    8 anchors (sixteen full anchor chunks; 9 and 11: a full chunk and a partial one of 1 and of 3 anchors) and fewer than 4."""
    cells = {s[0] * s[1] for s in ref.ANCHOR_SHAPES.values()} | {s[0] * s[1] for s in ref.CENTER_SHAPES.values()}
    assert {1, 35, 201, 1170} <= cells and 67 > 64 and 130 > 128
    assert all(ref.rows_of(n) % 256 for n in ref.ALL_CASES)
    assert {s[3] * s[4] for s in ref.ANCHOR_SHAPES.values()} == {1, 6, 9, 11, 128}
    assert {(s[0] * s[1], s[3] * s[4]) for s in ref.ANCHOR_SHAPES.values()} >= {(201, 9), (35, 11)}
    assert {s[5] for s in ref.ANCHOR_SHAPES.values()} == {1, 3, 10} and {s[6] for s in ref.ANCHOR_SHAPES.values()} == {0, 2, 4}
    assert {s[2] for s in ref.ANCHOR_SHAPES.values()} == {1, 3}


def test_coverage_anchor_edges():
    period, below = ref.period_of(2), np.nextafter(ref.period_of(2), F(0))
    for name, q_want in (("a:edges", (0, 1, 0, -1, -1)), ("a:edges:half", (0, 1, 1, 0, -1))):
        boxes, scores, labels, aux = ref.expected(name)
        v, q = aux["v"][0, 0:30:6], aux["q"][0, 0:30:6]                    # anchor 0 of cells (0, 0..4)
        assert v[0] == 0 and v[1] == period and v[2] == below and v[3] == F(-0.5) and v[4] == -period
        assert tuple(q) == q_want, (name, q)
        K1 = 7 * 6                                                           # row 1 starts here
        assert aux["cls_ties"][0, [K1, K1 + 6, K1 + 12, K1 + 18]].all()
        assert tuple(labels[0, [K1, K1 + 6, K1 + 12, K1 + 18]]) == (0, 0, 0, 1)
        K2 = 2 * K1
        assert aux["dir_ties"][0, [K2, K2 + 6, K2 + 12]].all() and (aux["bin"][0, [K2, K2 + 6, K2 + 12]] == 0).all()
        K3 = 3 * K1
        assert scores[0, K3] == 1.0 and labels[0, K3] == 0 and scores[0, K3 + 6] == 0.0 and labels[0, K3 + 6] == 0
        assert np.isposinf(boxes[0, K3 + 12, 3:6]).all()
        assert (boxes[0, K3 + 18, 3:6] < 1e-37).all() and (boxes[0, K3 + 18, 3:6] >= 0).all()
    far = ref.expected("a:far")[0]
    assert (np.abs(far[..., 0]) > 9e4).all() and (np.abs(far[..., 1]) > 9e4).all()
    ties = ref.expected("a:ties")
    assert ties[3]["cls_ties"].mean() > 0.2 and ties[3]["dir_ties"].mean() > 0.2
    c = ref.case("a:ties")
    for key in ("cls", "dir"):
        assert (np.signbit(c[key]) & (c[key] == 0)).any() and (~np.signbit(c[key]) & (c[key] == 0)).any()


def test_coverage_center():
    for name in ("c:5x7", "c:3x67", "c:9x130:peak"):
        boxes, scores, labels, aux = ref.expected(name)
        C = ref.CENTER_SHAPES[name][3]
        assert aux["none"].any() and (~aux["none"]).any(), name             # all-masked cells and peaks
        assert ((labels == -1) == aux["none"]).all() and (scores[aux["none"]] == 0).all()
        assert set(np.unique(labels)) == set(range(-1, C)), name
        hm = ref.case(name)["hm"]
        pk = ref.peak_mask(hm)
        right = pk[:, :, :, :-1] & pk[:, :, :, 1:] & (hm[:, :, :, :-1] == hm[:, :, :, 1:])
        assert right.any(), f"{name}: no plateau peak"
    for name in ("c:9x130", "c:1x1"):
        assert not ref.expected(name)[3]["none"].any() and (ref.expected(name)[2] >= 0).all()
    boxes, scores, labels, aux = ref.expected("c:edges")
    part = aux["part"][0].reshape(5, 7, 2)
    assert part[0, 0, 0] and part[0, 6, 0] and part[4, 0, 0] and part[4, 6, 0]           # corners
    assert part[0, 3, 0] and part[2, 0, 0]                                              # edges
    assert part[2:4, 3:5, 0].all()                                                      # 2 x 2 plateau
    assert part[2, :, 1].all()                                                          # full-row plateau
    assert not part[1, 1].any() and labels[0, 1 * 7 + 1] == -1 and scores[0, 8] == 0    # no class is a peak
    assert part[0, 1, 1] and labels[0, 1] == 1
    assert abs(abs(boxes[0, 0, 6]) - np.pi) < 1e-6 and abs(abs(boxes[0, 1, 6]) - np.pi) < 1e-6 and boxes[0, 2, 6] == 0
    assert np.isposinf(boxes[0, 3, 3])
    assert ref.expected("c:edges:vel")[0].shape[-1] == 9 and ref.expected("c:edges:raw")[0][0, 3, 3] == 0


def test_coverage_index():
    for name in ("a:5x7", "c:5x7"):
        K = ref.rows_of(name)
        ix = ref.index_cases(name)
        assert ix["perm"].shape[1] == K and all(sorted(r) == list(range(K)) for r in ix["perm"])
        assert (ix["dup"][:, 1::2] == ix["dup"][:, 0:-1:2]).all()
        assert {-1, K, 2 ** 31 - 1} <= set(ix["bad"][0].tolist()) and ix["bad"].shape[1] > 256
        assert ix["one"].shape[1] == 1
        b, s, l = ref.decode(ref.case(name), index=ix["bad"])
        inv = (ix["bad"] < 0) | (ix["bad"] >= K)
        assert inv.sum() >= 4 and (b[inv] == 0).all() and np.isneginf(s[inv]).all() and (l[inv] == -1).all()


def test_coverage_e2e():
    """The end-to-end case: lattice logits, size residuals 0, and a crowded scene: at least a fifth of the pre-selected
    boxes are suppressed, and neither cap is idle."""
    import nms_ref
    c = ref.e2e_case()
    assert np.isin(c["cls"], ref.LATTICE).all()
    sig = 1.0 / (1.0 + np.exp(-ref.LATTICE.astype(np.float64)))
    assert np.diff(sig).min() > 4e-3 and np.abs(sig - ref.E2E_NMS["score_thr"]).min() > 4e-3
    boxes, scores, labels = ref.decode(c)
    A = 6
    assert (boxes[..., 3:6].reshape(2, -1, A, 3) == np.repeat(np.asarray(c["kw"]["sizes"], F), 2, 0)[None, None]).all()
    kw = dict(ref.E2E_NMS)
    keep, order, count = nms_ref.nms_boxes(boxes, scores, labels, kw["iou_thr"], kw["score_thr"], kw["pre_max"], None)
    for b in range(2):
        pre = min(kw["pre_max"], int((scores[b] >= F(kw["score_thr"])).sum()))
        assert pre == kw["pre_max"]                                         # the pre cap cuts
        assert count[b] <= 0.8 * pre, (int(count[b]), pre)                  # >= a fifth suppressed
        assert count[b] > kw["post_max"]                                    # the post cap cuts
