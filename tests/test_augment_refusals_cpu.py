"""Every refusal of the augmentation's host code (SPEC.md §35), none of which needs a GPU.

The C entry points: argument blocks hold fake non-null device pointers, nothing is dereferenced, every case is refused before a
launch with the project's codes (SAD_EINVAL -1, SAD_EUNSUPPORTED -2) and sad_last_error() names the reason.  The operators: a
wrong dtype, shape or configuration is judged before any device, so CPU tensors reach those checks; CPU tensors that are
otherwise right are refused as such."""
import ctypes

import pytest

P = 0x10000                                           # a fake device pointer, 16-byte aligned
PASTE = dict(points=P, offsets=P, gt_boxes=P, gt_labels=P, db_points=P, db_offsets=P, db_boxes=P, params=None, B=2, total=1000, Cp=4, G=6,
             D=7, C=2, Ndb=10, max_obj_points=100, with_velocity=0, class_offsets=[0, 4, 10], sample_num=[8, 12], seed=1,
             remove_extra_width=0.0, R=1000 + 2 * 20 * 100, keep=P, db_index=P, boxes_out=P, labels_out=P, num_pasted=P, out_points=P,
             out_offsets=P, workspace=P)
GLOB = dict(points=P, offsets=P, gt_boxes=P, B=2, N=0, total=1000, Cp=4, G=6, D=7, seed=1, flip_x=1, flip_y=1, with_velocity=0, rot_lo=-0.5,
            rot_hi=0.5, scale_lo=0.9, scale_hi=1.1, translate=[0.0, 0.0, 0.0], points_out=P, boxes_out=P, params=P)
PASTE_CASES = [
    ("struct_size", dict(struct_size=-8), -1, "struct_size"),
    ("Q = 513", dict(sample_num=[500, 13], R=10 ** 9), -2, "Q=513"),
    ("Q = 0", dict(sample_num=[0, 0]), -1, "no candidate slot"),
    ("G = 1025", dict(G=1025), -1, "G <= 1024"),
    ("D = 6", dict(D=6), -1, "D = 6"),
    ("velocity with D = 8", dict(D=8, with_velocity=1), -1, "with_velocity needs D >= 9"),
    ("17 classes", dict(C=17), -1, "classes"),
    ("Cp = 2", dict(Cp=2), -1, "Cp >= 3"),
    ("class_offsets short of Ndb", dict(class_offsets=[0, 4, 9]), -1, "class_offsets"),
    ("class_offsets descending", dict(class_offsets=[0, 12, 10]), -1, "class_offsets"),
    ("out_points one row short", dict(R=1000 + 2 * 20 * 100 - 1), -1, "out_points has 4999 rows, needs"),
    ("negative extra width", dict(remove_extra_width=-0.1), -1, "remove_extra_width"),
    ("keep NULL", dict(keep=None), -1, "NULL pointer"),
    ("workspace NULL", dict(workspace=None), -1, "NULL pointer"),
    ("gt_labels NULL with G > 0", dict(gt_labels=None), -1, "NULL pointer"),
    ("workspace unaligned", dict(workspace=P + 4), -1, "16-byte aligned"),
    ("rows of 4 unaligned", dict(db_points=P + 4), -1, "16-byte aligned"),
    ("2^31 words", dict(total=2 ** 30, R=2 ** 31), -2, "2^31"),
]
GLOB_CASES = [
    ("struct_size", dict(struct_size=8), -1, "struct_size"),
    ("B = 0", dict(B=0), -1, "1 <= B"),
    ("G = 1025", dict(G=1025), -1, "G <= 1024"),
    ("D = 6", dict(D=6), -1, "D = 6"),
    ("velocity with D = 7", dict(with_velocity=1), -1, "with_velocity needs D >= 9"),
    ("padded, total != B * N", dict(offsets=None, N=400), -1, "B * N"),
    ("scale 0", dict(scale_lo=0.0), -1, "scale_lo"),
    ("rot descending", dict(rot_lo=1.0), -1, "rot_lo"),
    ("rot beyond 1e4", dict(rot_hi=2e4), -1, "1e4"),
    ("translate < 0", dict(translate=[0.0, -1.0, 0.0]), -1, "translate"),
    ("params NULL", dict(params=None), -1, "NULL pointer"),
    ("points_out NULL", dict(points_out=None), -1, "NULL pointer"),
]


def _block(cls, base, ov):
    f = dict(base, **ov)
    a = cls()
    a.struct_size = ctypes.sizeof(cls) + f.pop("struct_size", 0)
    for k, v in f.items():
        if isinstance(v, list):
            getattr(a, k)[:len(v)] = v
        else:
            setattr(a, k, v)
    return a


@pytest.mark.parametrize("name,ov,want,needle", PASTE_CASES, ids=[c[0] for c in PASTE_CASES])
def test_gt_paste_refused_on_the_host(sad, name, ov, want, needle):
    from sad_amd import _lib
    L = _lib.lib()
    code = L.sad_gt_paste_f32(ctypes.byref(_block(_lib.GtPasteArgs, PASTE, ov)), None)
    msg = L.sad_last_error().decode()
    assert code == want, f"{name}: code {code}, {msg}"
    assert msg.startswith("sad_gt_paste_f32: ") and needle in msg, msg


@pytest.mark.parametrize("name,ov,want,needle", GLOB_CASES, ids=[c[0] for c in GLOB_CASES])
def test_global_augment_refused_on_the_host(sad, name, ov, want, needle):
    from sad_amd import _lib
    L = _lib.lib()
    code = L.sad_global_augment_f32(ctypes.byref(_block(_lib.GlobalAugmentArgs, GLOB, ov)), None)
    msg = L.sad_last_error().decode()
    assert code == want, f"{name}: code {code}, {msg}"
    assert msg.startswith("sad_global_augment_f32: ") and needle in msg, msg


def test_null_args_workspace_sizes_and_mirrors(sad):
    from sad_amd import _lib
    L = _lib.lib()
    assert L.sad_gt_paste_f32(None, None) == -1 and b"NULL args" in L.sad_last_error()
    assert L.sad_global_augment_f32(None, None) == -1 and b"NULL args" in L.sad_last_error()
    assert L.sad_gt_paste_workspace_bytes(2, 513, 100) == 0 and L.sad_gt_paste_workspace_bytes(0, 20, 100) == 0
    assert L.sad_gt_paste_workspace_bytes(2, 20, -1) == 0
    small, large = L.sad_gt_paste_workspace_bytes(2, 20, 1000), L.sad_gt_paste_workspace_bytes(2, 512, 1000)
    assert 0 < small < large and small % 16 == 0
    assert L.sad_gt_paste_workspace_bytes(2, 20, 100000) > small
    assert ctypes.sizeof(_lib.GlobalAugmentArgs) == 128 and ctypes.sizeof(_lib.GtPasteArgs) == 320
    assert L.sad_version() == _lib.ABI_VERSION == 4


# ---- the operators ----------------------------------------------------------------------------------------------------------
def _paste_args(**ov):
    import torch
    z = torch.zeros
    a = dict(points=z(100, 4), offsets=z(3, dtype=torch.int32), gt_boxes=z(2, 6, 7), gt_labels=z(2, 6, dtype=torch.int32),
             db_points=z(50, 4), db_offsets=z(11, dtype=torch.int32), db_boxes=z(10, 7), class_offsets=[0, 4, 10])
    a.update(ov)
    return list(a.values())


def test_gt_paste_argument_errors(sad):
    import torch
    from sad_amd import ops
    z = torch.zeros
    kw = dict(sample_num=[8, 12], max_obj_points=10)
    for ov in (dict(points=z(100, 4, dtype=torch.float64)), dict(offsets=z(3, dtype=torch.int64)), dict(gt_labels=z(2, 6, dtype=torch.int64)),
               dict(gt_boxes=z(2, 6, 7, dtype=torch.float16)), dict(db_points=z(50, 4, dtype=torch.float64)),
               dict(db_offsets=z(11, dtype=torch.int64)), dict(db_boxes=z(10, 7, dtype=torch.float64)), dict(points=None)):
        with pytest.raises(TypeError):
            ops.gt_paste(*_paste_args(**ov), **kw)
    with pytest.raises(TypeError):
        ops.gt_paste(*_paste_args(), params=z(2, 8, dtype=torch.float64), **kw)
    for ov, k2 in ((dict(db_points=z(50, 5)), {}),                                      # a database with another Cp
                   (dict(db_boxes=z(10, 9)), {}),                                       # ... or another D
                   (dict(gt_boxes=z(2, 1025, 7), gt_labels=z(2, 1025, dtype=torch.int32)), {}),     # G > 1024
                   (dict(gt_boxes=z(3, 6, 7), gt_labels=z(3, 6, dtype=torch.int32)), {}),
                   (dict(gt_boxes=z(2, 6, 6)), {}),
                   (dict(points=z(100, 2)), {}),
                   (dict(db_offsets=z(12, dtype=torch.int32)), {}),
                   (dict(class_offsets=[0, 4, 9]), {}),
                   (dict(class_offsets=[0, 4]), {}),
                   ({}, dict(sample_num=[500, 13])),                                    # Q > 512
                   ({}, dict(sample_num=[0, 0])),
                   ({}, dict(sample_num=[-1, 3])),
                   ({}, dict(with_velocity=True)),                                      # D = 7
                   ({}, dict(params=z(3, 8))),
                   ({}, dict(remove_extra_width=-1.0)),
                   ({}, dict(max_obj_points=-1))):
        with pytest.raises(ValueError):
            ops.gt_paste(*_paste_args(**ov), **dict(kw, **k2))
    # out_points shorter than the bound: 100 + 2 * 20 * 10 rows are needed
    spec = ops.gt_paste_output_spec(2, 6, 7, 20, 4, ops.gt_paste_rows(100, 2, 20, 10) - 1)
    assert ops.gt_paste_rows(100, 2, 20, 10) == 500 and [n for n, _, _ in spec] == list(ops.PASTE_OUTPUTS)
    with pytest.raises(ValueError, match="out_points: 499 rows, needs"):
        ops.gt_paste(*_paste_args(), out=tuple(z(shape, dtype=dt) for _, shape, dt in spec), **kw)
    # everything right but the device
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.gt_paste(*_paste_args(), **kw)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.gt_paste(*_paste_args(), params=z(2, 8), **kw)


def test_global_augment_argument_errors(sad):
    import torch
    from sad_amd import ops
    z = torch.zeros
    off = z(3, dtype=torch.int32)
    for args in ((z(100, 4, dtype=torch.float64), off, z(2, 6, 7)), (z(100, 4), z(3, dtype=torch.int64), z(2, 6, 7)),
                 (z(100, 4), off, z(2, 6, 7, dtype=torch.float64)), (z(2, 50, 4), None, None)):
        with pytest.raises(TypeError):
            ops.global_augment(*args)
    for args, kw in (((z(100, 4), off, z(3, 6, 7)), {}), ((z(100, 4), off, z(2, 6, 6)), {}), ((z(100, 2), off, z(2, 6, 7)), {}),
                     ((z(2, 50, 4), off, z(2, 6, 7)), {}), ((z(100, 4), None, z(2, 6, 7)), {}), ((z(100, 4), off, z(2, 1025, 7)), {}),
                     ((z(100, 4), off, z(2, 6, 8)), dict(with_velocity=True)), ((z(100, 4), off, z(2, 6, 7)), dict(scale_range=(0.0, 1.0))),
                     ((z(100, 4), off, z(2, 6, 7)), dict(rot_range=(1.0, -1.0))), ((z(100, 4), off, z(2, 6, 7)), dict(rot_range=(0.0, 2e4))),
                     ((z(100, 4), off, z(2, 6, 7)), dict(translate_range=(0.0, -1.0, 0.0))),
                     ((z(100, 4), off, z(2, 6, 7)), dict(translate_range=(0.0, 1.0)))):
        with pytest.raises(ValueError):
            ops.global_augment(*args, **kw)
    for args in ((z(100, 4), off, z(2, 6, 7)), (z(2, 50, 5), None, z(2, 0, 9))):
        with pytest.raises(RuntimeError, match="no CPU path"):
            ops.global_augment(*args)


def test_out_checks_and_exports(sad):
    import torch
    import sad_amd
    from sad_amd import augment, ops
    cpu = torch.device("cpu")
    spec = ops.global_augment_output_spec((2, 50, 4), 2, 6, 9)
    assert [tuple(s) for _, s, _ in spec] == [(2, 50, 4), (2, 6, 9), (2, 8)]
    good = tuple(torch.zeros(shape, dtype=dt) for _, shape, dt in spec)
    assert ops._outputs(spec, good, cpu, "points") == good
    with pytest.raises(ValueError, match="out: expected contiguous"):
        ops._outputs(spec, good[:2] + (torch.zeros(2, 9),), cpu, "points")
    spec = ops.gt_paste_output_spec(2, 6, 7, 20, 4, 500)
    assert [tuple(s) for _, s, _ in spec] == [(2, 20), (2, 20), (2, 26, 7), (2, 26), (2,), (500, 4), (3,)]
    for n in ("global_augment", "gt_paste", "gt_paste_workspace", "gt_paste_rows"):
        assert getattr(sad_amd, n) is getattr(ops, n)
    for n in ("GTDatabase", "GTSampler", "GlobalAugment", "TrainAugment"):
        assert getattr(sad_amd, n) is getattr(augment, n)
