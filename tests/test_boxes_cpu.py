"""CPU checks of the box operators (SPEC.md §19): the numpy reference the GPU tests use (its BEV IoU against the oracle, its
in-box predicate against an independent float64 computation, hand-checked toy cases), the scene-box replay, and the
host-side argument errors of the three C entry points (nothing is launched)."""
import numpy as np
import pytest

import box_ref as ref

F = np.float32


def _pairs(rng, n):
    """n box pairs [n,7]: random, identical, edge-touching, lattice and yaw-offset-by-pi/2 pairs."""
    A = np.zeros((n, 7), F)
    B = np.zeros((n, 7), F)
    for X in (A, B):
        X[:, 0:2] = rng.uniform(-2, 2, (n, 2))
        X[:, 2] = rng.uniform(-1, 1, n)
        X[:, 3:6] = rng.uniform(0.5, 4, (n, 3))
        X[:, 6] = rng.uniform(-4, 4, n)
    q = n // 6
    B[:q] = A[:q]                                                     # identical
    s = slice(q, 2 * q)                                               # edge-touching: yaw 0, shifted by the length
    A[s, 6] = 0
    B[s] = A[s]
    B[s, 0] = A[s, 0] + A[s, 3]
    s = slice(2 * q, 3 * q)                                           # lattice
    A[s, 0:2] = rng.integers(-4, 5, (q, 2)) * 0.5
    B[s, 0:2] = rng.integers(-4, 5, (q, 2)) * 0.5
    A[s, 3:5] = 1
    B[s, 3:5] = 2
    A[s, 6] = 0
    B[s, 6] = 0
    s = slice(3 * q, 4 * q)                                           # the same box turned by pi/2
    B[s] = A[s]
    B[s, 6] = A[s, 6] + F(np.pi / 2)
    s = slice(4 * q, 5 * q)                                           # yaw near 1e3
    A[s, 6] += 1000
    B[s, 6] += 1000
    return A, B


def test_reference_bev_iou_equals_oracle():
    """The reference's scalar clip (used for the 3-D IoU) gives the oracle's iou_bev bit for bit on 3 000 pairs."""
    A, B = _pairs(np.random.default_rng(0), 3000)
    want = ref.iou_bev_matrix(A[:1], B[:1])[0]                        # (shape check of the matrix form)
    assert want.shape == (1,)
    import oracle
    want = oracle.iou_bev(ref.pad9(A), ref.pad9(B))
    got = np.array([ref.iou_bev_pair(A[i], B[i]) for i in range(len(A))], F)
    np.testing.assert_array_equal(got.view(np.int32), want.view(np.int32))
    assert (want > 0).sum() >= 1000 and (want == 0).sum() >= 300


def test_reference_inside_matches_float64():
    """§19.1 in float32 agrees with a float64 rotate-and-compare on every pair farther than 1e-4 from a face."""
    rng = np.random.default_rng(1)
    K, N = 64, 4000
    boxes = np.zeros((K, 7), F)
    boxes[:, 0:3] = rng.uniform(-3, 3, (K, 3))
    boxes[:, 3:6] = rng.uniform(0.5, 4, (K, 3))
    boxes[:, 6] = rng.uniform(-np.pi, np.pi, K)
    boxes[:8, 6] = rng.uniform(990, 1010, 8)
    pts = rng.uniform(-5, 5, (N, 3)).astype(F)
    for e in (0.0, 0.5):
        got = ref.inside(pts, boxes, e)
        b = boxes.astype(np.float64)
        c, s = np.cos(b[:, 6]), np.sin(b[:, 6])
        d = pts[:, None, :].astype(np.float64) - b[None, :, 0:3]
        lx = d[..., 0] * c + d[..., 1] * s
        ly = d[..., 1] * c - d[..., 0] * s
        hl, hw, hh = 0.5 * (b[:, 3] + 2 * e), 0.5 * (b[:, 4] + 2 * e), 0.5 * (b[:, 5] + 2 * e)
        want = (np.abs(d[..., 2]) <= hh) & (np.abs(lx) < hl) & (np.abs(ly) < hw)
        far = ((np.abs(np.abs(lx) - hl) > 1e-4) & (np.abs(np.abs(ly) - hw) > 1e-4) & (np.abs(np.abs(d[..., 2]) - hh) > 1e-4))
        assert far.mean() > 0.99 and want.sum() >= 1000 and (~want).sum() >= 1000
        np.testing.assert_array_equal(got[far], want[far])


def test_toy_lattice_faces():
    """A yaw-0 box 2 x 1 x 1 at the origin on a 0.25 lattice: the xy faces are outside, the z faces inside."""
    box = np.array([[[0, 0, 0, 2, 1, 1, 0]]], F)
    pts = np.array([[[1, 0, 0], [0.75, 0, 0], [-1, 0.25, 0], [0, 0.5, 0], [0, -0.25, 0], [0, 0, 0.5], [0.5, 0.25, -0.5],
                     [0, 0, 0.75], [0.75, 0.25, 0.5], [-0.75, -0.25, -0.5]]], F)
    got = ref.points_in_boxes(pts, box)[0]
    np.testing.assert_array_equal(got, [-1, 0, -1, -1, 0, 0, 0, -1, 0, 0])
    assert ref.face_hits(pts[0], box[0]) == (3, 4)


def test_toy_point_in_two_boxes_takes_the_lower_index():
    boxes = np.array([[[5, 5, 0, 1, 1, 1, 0], [0, 0, 0, 2, 2, 2, 0], [0.25, 0, 0, 1, 1, 1, 0.3]]], F)
    pts = np.array([[[0.25, 0, 0], [0.9, 0.9, 0], [5, 5, 0], [9, 9, 9]]], F)
    np.testing.assert_array_equal(ref.points_in_boxes(pts, boxes)[0], [1, 1, 0, -1])
    boxes2 = boxes[:, ::-1].copy()
    np.testing.assert_array_equal(ref.points_in_boxes(pts, boxes2)[0], [0, 1, 2, -1])


def test_toy_pool_cyclic_slots_and_empty_box():
    """Three points inside the first box, S = 7: slots repeat cyclically; the second box is empty: zeros, empty = 1."""
    pts = np.array([[[9, 9, 9], [0, 0, 0], [3, 3, 3], [0.25, 0, 0], [0, 0.25, 0.25], [8, 8, 8]]], F)
    feat = np.arange(12, dtype=F).reshape(1, 6, 2)
    boxes = np.array([[[0, 0, 0, 1, 1, 1, 0, 0.9, 1], [20, 20, 20, 1, 1, 1, 0, 0.1, 2]]], F)
    pooled, empty, idx = ref.roipoint_pool3d(pts, feat, boxes, 0.0, 7)
    np.testing.assert_array_equal(idx[0, 0], [1, 3, 4, 1, 3, 4, 1])
    np.testing.assert_array_equal(pooled[0, 0, 1], [0.25, 0, 0, 6, 7])
    np.testing.assert_array_equal(pooled[0, 0, 5], pooled[0, 0, 2])
    np.testing.assert_array_equal(empty[0], [0, 1])
    assert not pooled[0, 1].any() and not idx[0, 1].any()
    # extra width: the enlarged box reaches (3,3,3)? no (half extent 0.5 + 1 = 1.5); S = 2 keeps the first two
    pooled, empty, idx = ref.roipoint_pool3d(pts, None, boxes, 1.0, 2)
    np.testing.assert_array_equal(idx[0, 0], [1, 3])
    assert pooled.shape == (1, 2, 2, 3)


def test_toy_iou3d():
    """Stacked (touching in z), disjoint in z, half-overlapping in z and identical boxes."""
    a = np.array([[0, 0, 0, 2, 1, 1, 0]], F)
    b = np.array([[0, 0, 1, 2, 1, 1, 0], [0, 0, 5, 2, 1, 1, 0], [0, 0, 0.5, 2, 1, 1, 0], [0, 0, 0, 2, 1, 1, 0],
                  [0, 0, 0, 2, 1, 1, np.float32(0.7)]], F)
    got = ref.iou3d_matrix(a, b)[0]
    assert got[0] == 0 and got[1] == 0
    assert abs(got[2] - 1 / 3) < 1e-6 and abs(got[3] - 1) < 1e-6
    bev = ref.iou_bev_matrix(a, b)[0]
    assert abs(bev[0] - 1) < 1e-6 and 0 < got[4] == bev[4] < 1        # same height and z range: 3-D = BEV


def test_scene_boxes_replay_make_scene(sad):
    """synth.scene_boxes rebuilds the 40 ground-truth boxes of a scene: the scene's object points (30 %) fall inside them."""
    from sad_amd import synth
    for sid, n in ((0, 16384), (5, 4096)):
        pts = synth.make_scene(sid, n)[:, :3]
        bx = synth.scene_boxes(sid, n)
        assert bx.shape == (40, 7) and bx.dtype == np.float32
        share = (ref.points_in_boxes(pts[None], bx[None])[0] >= 0).mean()
        assert 0.29 < share < 0.33, share


def test_host_side_argument_errors(sad):
    from sad_amd import _lib
    L = _lib.lib()
    p = 0x10000                                           # never dereferenced: every call below fails on the host
    assert L.sad_boxes_iou_f32(None, p, 1, 4, 4, 7, 7, 0, p, None) == -1 and b"NULL" in L.sad_last_error()
    assert L.sad_boxes_iou_f32(p, p, 1, 4, 4, 6, 7, 0, p, None) == -1 and b"D >= 7" in L.sad_last_error()
    assert L.sad_boxes_iou_f32(p, p, 1, 4, 0, 7, 7, 0, p, None) == -1 and b">= 1" in L.sad_last_error()
    assert L.sad_boxes_iou_f32(p, p, 1, 4, 4, 7, 9, 2, p, None) == -1 and b"mode" in L.sad_last_error()
    assert L.sad_points_in_boxes_f32(p, p, 1, 8, 4, 7, None, None) == -1 and b"NULL" in L.sad_last_error()
    assert L.sad_points_in_boxes_f32(p, p, 1, 8, 4, 5, p, None) == -1 and b"D >= 7" in L.sad_last_error()
    assert L.sad_points_in_boxes_f32(p, p, 1, 0, 4, 7, p, None) == -1
    assert L.sad_roipoint_pool3d_f32(p, None, p, 1, 8, 4, 7, 2, 0.0, 4, p, p, None, None) == -1 and b"feature" in L.sad_last_error()
    assert L.sad_roipoint_pool3d_f32(p, None, p, 1, 8, 4, 7, 0, 0.0, 0, p, p, None, None) == -1 and b"S must be" in L.sad_last_error()
    assert L.sad_roipoint_pool3d_f32(p, None, p, 1, 8, 4, 7, 0, 0.0, 4, p, None, None, None) == -1 and b"NULL" in L.sad_last_error()
    assert L.sad_roipoint_pool3d_f32(p, None, p, 1, 8, 4, 7, 0, 0.0, 8193, p, p, None, None) == -2 and b"8193" in L.sad_last_error()


def test_python_surface(sad):
    import torch
    import sad_amd
    from sad_amd import ops
    x = torch.zeros(1, 16, 3)
    bx = torch.zeros(1, 4, 7)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.points_in_boxes(x, bx)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.roipoint_pool3d(x, None, bx, 1.0, 16)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.boxes_iou_bev(bx[0], bx[0])
    assert sad_amd.boxes_iou_bev is ops.boxes_iou_bev and sad_amd.boxes_iou3d is ops.boxes_iou3d
    assert sad_amd.points_in_boxes is ops.points_in_boxes and sad_amd.roipoint_pool3d is ops.roipoint_pool3d
