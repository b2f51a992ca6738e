"""GPU checks of the training augmentation (SPEC.md §35): ``ops.gt_paste`` and ``ops.global_augment`` against the float32 numpy
reference under ``==``, the fused form against the two calls in sequence, and the chain into ``SADDetectorTrain``.  Every output
buffer is pre-filled with NaN (integers with a sentinel), and every call is made twice: the second is bit-equal."""
import numpy as np
import pytest

import augment_ref as ref

pytestmark = pytest.mark.gpu
F = np.float32
NAN = float("nan")
SENTINEL = -77


@pytest.fixture(autouse=True)
def _oracle(orc):
    return orc


def _t(x, dev):
    import torch
    return None if x is None else torch.from_numpy(np.array(x)).to(dev)


def _filled(spec, dev):
    import torch
    return tuple(torch.full(shape, NAN if dt == torch.float32 else SENTINEL, dtype=dt, device=dev) for _, shape, dt in spec)


def _bits(a):
    return a.view(np.int32) if a.dtype == np.float32 else a


def _twice(fn):
    """fn() -> tuple of tensors, called twice into fresh sentinel-filled buffers; -> the first call's numpy results."""
    runs = [[g.cpu().numpy() for g in fn()] for _ in range(2)]
    for x, y in zip(*runs):
        np.testing.assert_array_equal(_bits(x), _bits(y), err_msg="a second call differs")
    return runs[0]


def _paste(dev, c, params=None, vel=False, slack=5):
    """ops.gt_paste on a case of the reference -> dict of numpy outputs; out_points keeps its unwritten tail."""
    from sad_amd import ops
    db = c["db"]
    B, G, D = c["gt_boxes"].shape
    Q, Cp, total = sum(c["sample_num"]), c["points"].shape[1], c["points"].shape[0]
    R = ops.gt_paste_rows(total, B, Q, c["Pmax"]) + slack
    args = [_t(c[k], dev) for k in ("points", "offsets", "gt_boxes", "gt_labels")] + [_t(db[k], dev) for k in ("points", "offsets", "boxes")]
    p = _t(params, dev)

    def run():
        out = _filled(ops.gt_paste_output_spec(B, G, D, Q, Cp, R), dev)
        got = ops.gt_paste(*args, db["class_offsets"], sample_num=c["sample_num"], max_obj_points=c["Pmax"], seed=c["seed_step"][0],
                           step=c["seed_step"][1], remove_extra_width=c["e"], params=p, with_velocity=vel, out=out)
        assert all(g is o for g, o in zip(got, out))
        return got
    return dict(zip(ops.PASTE_OUTPUTS, _twice(run)))


def _same_paste(got, want, what):
    for k in ("keep", "db_index", "labels_out", "num_pasted", "out_offsets", "boxes_out"):
        assert not (got[k] == SENTINEL).any() and not np.isnan(got[k]).any(), f"{what}: {k} was not fully written"
        np.testing.assert_array_equal(got[k], want[k], err_msg=f"{what}: {k}")
    n = int(want["out_offsets"][-1])
    np.testing.assert_array_equal(_bits(got["out_points"][:n]), _bits(want["out_points"]), err_msg=f"{what}: out_points")
    assert np.isnan(got["out_points"][n:]).all(), f"{what}: a row at or beyond out_offsets[B] was written"


# ---- 1: gt_paste == the reference ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ref.CASES)
def test_gt_paste_equals_reference(sad, dev, name):
    got = _paste(dev, ref.case(name))
    _same_paste(got, ref.expected(name), name)


def test_gt_paste_named_outcomes(sad, dev):
    """What the named cases are for, read from the kernel's outputs (the reference's side of it: test_augment_cpu.py)."""
    c = ref.case("all_collide")
    got = _paste(dev, c)
    assert not got["keep"].any() and (got["db_index"] >= 0).sum(1).tolist() == [4, 4, 4]
    np.testing.assert_array_equal(got["out_offsets"], c["offsets"])
    np.testing.assert_array_equal(_bits(got["out_points"][:c["points"].shape[0]]), _bits(c["points"]))
    assert _paste(dev, ref.case("none_collide"))["keep"].all()
    assert _paste(dev, ref.case("chain"))["keep"].tolist() == [[1, 0, 1]] * 3
    assert _paste(dev, ref.case("shared_edge"))["keep"][:, 0].all()
    assert _paste(dev, ref.case("twice"))["keep"].tolist() == [[1, 0, 1, 0]] * 3
    assert _paste(dev, ref.case("padding_gt"))["keep"].all()
    assert _paste(dev, ref.case("quota_met"))["db_index"].tolist() == [[-1, -1, 1, -1]] * 3
    assert _paste(dev, ref.case("empty_class"))["db_index"][:, 1:4].tolist() == [[-1] * 3] * 3


def test_gt_paste_kept_workspace_and_default_outputs(sad, dev):
    """The caller's workspace and no ``out``: the same results; out_points then has exactly the bound's rows."""
    import torch
    from sad_amd import ops
    name = "q70_c5_d7_g6"
    c, db = ref.case(name), ref.case(name)["db"]
    B, Q, total = 3, sum(c["sample_num"]), c["points"].shape[0]
    ws = ops.gt_paste_workspace(B, Q, total, dev)
    ws.fill_(0xAB)
    args = [_t(c[k], dev) for k in ("points", "offsets", "gt_boxes", "gt_labels")] + [_t(db[k], dev) for k in ("points", "offsets", "boxes")]
    got = ops.gt_paste(*args, db["class_offsets"], sample_num=c["sample_num"], max_obj_points=c["Pmax"], seed=c["seed_step"][0],
                       step=c["seed_step"][1], workspace=ws)
    torch.cuda.synchronize()
    got = dict(zip(ops.PASTE_OUTPUTS, [g.cpu().numpy() for g in got]))
    want = ref.expected(name)
    assert got["out_points"].shape[0] == ops.gt_paste_rows(total, B, Q, c["Pmax"])
    n = int(want["out_offsets"][-1])
    for k in ("keep", "db_index", "labels_out", "num_pasted", "out_offsets", "boxes_out"):
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)
    np.testing.assert_array_equal(_bits(got["out_points"][:n]), _bits(want["out_points"]))


# ---- 2: global_augment ---------------------------------------------------------------------------------------------------
def _global(dev, points, offsets, boxes, seed, step, vel=False, **cfg):
    from sad_amd import ops
    B, G, D = boxes.shape
    args = (_t(points, dev), _t(offsets, dev), _t(boxes, dev))

    def run():
        out = _filled(ops.global_augment_output_spec(points.shape, B, G, D), dev)
        got = ops.global_augment(*args, seed=seed, step=step, with_velocity=vel, out=out, **cfg)
        assert all(g is o for g, o in zip(got, out))
        return got
    return _twice(run)


@pytest.mark.parametrize("name,vel", [("q20_c4_d7_g6", False), ("q20_c5_d9_g1", True), ("q20_c4_d9_g0", False)])
def test_global_augment_equals_reference_ragged(sad, dev, name, vel):
    c = ref.case(name)
    for step in (0, 1, 2, 3):                            # four draws: both flips come up both ways
        got = _global(dev, c["points"], c["offsets"], c["gt_boxes"], 5, step, vel, **ref.GLOBAL)
        want = ref.global_augment(c["points"], c["offsets"], c["gt_boxes"], ref.call_seed(5, step), vel, **ref.GLOBAL)
        for g, w, what in zip(got, want, ("points", "boxes", "params")):
            assert not np.isnan(g).any(), f"{what} was not fully written"
            np.testing.assert_array_equal(_bits(g), _bits(w), err_msg=f"{name} step {step}: {what}")
    flips = {int(ref.draw_params(ref.call_seed(5, s), 3, **ref.GLOBAL)[b, 0]) for s in range(4) for b in range(3)}
    assert flips == {0, 1, 2, 3}, "the steps of this test do not draw every flip combination"


@pytest.mark.parametrize("Cp,D,vel", [(4, 7, False), (5, 9, True)])
def test_global_augment_padded_layout_and_copies(sad, dev, Cp, D, vel):
    """[B,N,Cp] with offsets=None; N = 300 crosses a workgroup inside every scene; the extra columns are bit copies, NaN included."""
    rng = np.random.default_rng(3)
    pts = rng.uniform(-30, 30, (3, 300, Cp)).astype(F)
    pts[:, ::7, 3:] = NAN
    boxes = rng.uniform(-5, 5, (3, 6, D)).astype(F)
    boxes[:, 2, 3:6] = 0
    got = _global(dev, pts, None, boxes, 9, 4, vel, **ref.GLOBAL)
    want = ref.global_augment(pts, None, boxes, ref.call_seed(9, 4), vel, **ref.GLOBAL)
    for g, w, what in zip(got, want, ("points", "boxes", "params")):
        np.testing.assert_array_equal(_bits(g), _bits(w), err_msg=what)
    np.testing.assert_array_equal(_bits(got[0][..., 3:]), _bits(pts[..., 3:]))
    np.testing.assert_array_equal(_bits(got[1][..., 9 if vel else 7:]), _bits(boxes[..., 9 if vel else 7:]))
    assert (got[1][:, 2, 3:6] == 0).all(), "a padding row stopped being padding"


def test_global_augment_identity(sad, dev):
    c = ref.case("q20_c5_d9_g1")
    pts, boxes, params = _global(dev, c["points"], c["offsets"], c["gt_boxes"], 1, 0, True, **ref.IDENTITY)
    np.testing.assert_array_equal(pts, c["points"])
    np.testing.assert_array_equal(boxes, c["gt_boxes"])
    np.testing.assert_array_equal(params, np.tile(np.array([0, 0, 1, 0, 1, 0, 0, 0], F), (3, 1)))


# ---- 3: the fused form ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,vel", [("q20_c4_d7_g6", False), ("q20_c5_d9_g1", True), ("q70_c5_d7_g6", False), ("faces", False)])
def test_fused_paste_equals_paste_then_global(sad, dev, name, vel):
    from sad_amd import ops
    c = ref.case(name)
    B = 3
    plain = _paste(dev, c, slack=0)
    n = int(plain["out_offsets"][-1])
    for step in (0, 2):
        P = ref.draw_params(ref.call_seed(5, step), B, **ref.GLOBAL)
        fused = _paste(dev, c, params=P, vel=vel, slack=0)
        pts, boxes, params = _global(dev, plain["out_points"], plain["out_offsets"], plain["boxes_out"], 5, step, vel, **ref.GLOBAL)
        np.testing.assert_array_equal(_bits(params), _bits(P))
        for k in ("keep", "db_index", "labels_out", "num_pasted", "out_offsets"):
            np.testing.assert_array_equal(fused[k], plain[k], err_msg=k)
        np.testing.assert_array_equal(_bits(fused["out_points"][:n]), _bits(pts[:n]), err_msg="points")
        assert np.isnan(fused["out_points"][n:]).all()
        np.testing.assert_array_equal(_bits(fused["boxes_out"]), _bits(boxes), err_msg="boxes")
        want = ref.gt_paste_vec(c, P, vel)
        np.testing.assert_array_equal(_bits(fused["out_points"][:n]), _bits(want["out_points"]), err_msg="points against the reference")
        np.testing.assert_array_equal(_bits(fused["boxes_out"]), _bits(want["boxes_out"]), err_msg="boxes against the reference")


# ---- 4: end to end ---------------------------------------------------------------------------------------------------------
def test_train_augment_feeds_detector(sad, dev):
    """TINY, B = 2, a database cut from two other synth scenes: TrainAugment -> SADDetectorTrain forward / targets / loss."""
    import torch
    from sad_amd import config, synth
    from sad_amd.augment import GTDatabase, GTSampler, GlobalAugment, TrainAugment
    from sad_amd.detector_train import SADDetectorTrain
    cfg, B = config.TINY, 2
    ext = dict(extent=(0.0, 20.0, -10.0, 10.0), n_boxes=6)

    def labelled(first):
        pts = synth.make_tiny_batch(first, B, cfg.n_points).reshape(-1, 4)
        gt = np.stack([synth.scene_boxes(first + i, cfg.n_points, **ext) for i in range(B)])
        return pts, np.arange(B + 1, dtype=np.int32) * cfg.n_points, gt, np.zeros(gt.shape[:2], np.int32)

    db = GTDatabase.from_scenes(*labelled(10), num_classes=1, device=dev, max_obj_points=256)
    assert len(db) > 0 and db.Pmax <= 256 and db.class_offsets == [0, len(db)]
    pts, off, gt, gl = labelled(0)
    args = (_t(pts, dev), _t(off, dev), _t(gt, dev), _t(gl, dev))
    det = SADDetectorTrain(cfg, dev, seed=0)

    def run(step):
        aug = TrainAugment(GTSampler(db, [12], remove_extra_width=0.1, seed=3), GlobalAugment(seed=4), cfg.n_points, seed=5)
        p, bx, lb = aug(*args, step=step)
        assert tuple(p.shape) == (B, cfg.n_points, 4) and tuple(bx.shape) == (B, 6 + 12, 7) and tuple(lb.shape) == (B, 6 + 12)
        with torch.no_grad():
            out = det(p)
            loss = det.loss(out, det.targets(out, bx, lb))
        return [x.cpu().numpy() for x in (p, bx, lb, loss)]

    a, again, other = run(0), run(0), run(1)
    assert np.isfinite(a[3]).all() and np.isfinite(a[0]).all()
    for x, y in zip(a, again):
        np.testing.assert_array_equal(_bits(x), _bits(y), err_msg="the same step is not bit-equal")
    assert not np.array_equal(a[0], other[0]) and not np.array_equal(a[1], other[1]), "another step gave the same batch"
    assert ((a[2] >= 0).sum(1) > (gl >= 0).sum(1)).any(), "nothing was pasted"
