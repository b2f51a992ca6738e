"""CPU checks of the voxelization reference and boundary (SPEC.md §20), no GPU: the two forms of tests/voxel_ref.py agree on
every input family, hand-worked cases pin §20.1 / §20.2, the reductions are checked against float64 and torch.autograd, and the
C-ABI declares, binds and exports the six new entry points (argument errors come back before any launch)."""
import ctypes
import os
import re

import numpy as np
import pytest

import voxel_cases as vc
import voxel_ref as ref
from conftest import ROOT

F = np.float32
NAMES = ["sad_voxel_workspace_bytes", "sad_voxel_coords_f32", "sad_voxel_index_f32", "sad_voxelize_f32", "sad_voxel_reduce_f32",
         "sad_voxel_reduce_grad_f32"]


def _forms_agree(name, pts, off, p):
    v, r, T, V = p["v"], p["r"], p["T"], p["V"]
    a = ref.voxel_index(pts, off, v, r, V, "loop")
    b = ref.voxel_index(pts, off, v, r, V, "vec")
    for x, y, n in zip(a, b, ("point2voxel", "coors", "count", "voxel_num")):
        assert np.array_equal(x, y), f"{name}: loop and vec forms differ in {n}"
    lv = ref.voxelize_loop(pts, off, v, r, T, V)
    vv = ref.voxelize(pts, off, v, r, T, V)
    for x, y, n in zip(lv[:4], vv, ("voxels", "coors", "num_points", "voxel_num")):
        assert np.array_equal(x, y), f"{name}: literal and vectorised voxelize differ in {n}"
    assert np.array_equal(lv[4], b[0]) and np.array_equal(lv[5], b[2])
    return b


@pytest.mark.parametrize("family", ["pillars", "capped", "fine", "nuscenes", "dense", "degenerate"])
def test_reference_forms_agree(sad, family):
    for name, pts, off, p in vc.FAMILIES[family]():
        p2v = _forms_agree(name, pts, off, p)[0]
        if pts.shape[0] <= 40000:
            for mode in ("sum", "mean", "max"):
                a = ref.voxel_reduce_loop(pts, p2v, off, p["V"], mode)
                b = ref.voxel_reduce(pts, p2v, off, p["V"], mode)
                for x, y in zip(a, b):
                    assert (x is None and y is None) or np.array_equal(x, y), f"{name}: reduce forms differ ({mode})"


def test_grid_size_and_limits():
    assert ref.grid_size(vc.PILLARS["v"], vc.PILLARS["r"]) == (432, 496, 1)
    assert ref.grid_size(vc.FINE["v"], vc.FINE["r"]) == (1408, 1600, 40)
    assert ref.grid_size(vc.NUSC["v"], vc.NUSC["r"]) == (512, 512, 1)
    assert ref.grid_size((1, 1, 1), (0, 0, 0, 2.5, 3.5, 0.5)) == (2, 4, 0)         # round half to even
    with pytest.raises(ValueError):
        ref.check_grid((1, 1, 1), (0, 0, 0, 2.5, 3.5, 0.5))
    with pytest.raises(ValueError):
        ref.check_grid((0.001, 0.001, 0.001), (0, 0, 0, 4, 4, 4))


def test_faces_lo_hi_and_one_ulp():
    v, r = (F(0.16), F(0.16), F(4)), (0, -39.68, -3, 69.12, 39.68, 1)
    lo, hi = np.asarray(r, F)[:3], np.asarray(r, F)[3:]
    off = np.array([0, 2], np.int32)
    c = ref.voxel_coords(np.stack([lo, hi]), off, v, r)
    assert c[0].tolist() == [0, 0, 0, 0] and c[1].tolist() == [0, -1, -1, -1]       # on lo: valid; on hi: not
    for d in range(3):                                                              # on hi in ONE axis only is invalid too
        q = lo.copy()
        q[d] = hi[d]
        assert ref.voxel_coords(q[None], off[:1].tolist() + [1], v, r)[0, 1:].tolist() == [-1, -1, -1]
    # one ulp either side of an interior face: the face x = 1.0 of a 0.25 grid from 0 (exact in binary32)
    v2, r2 = (0.25, 0.25, 0.25), (0, 0, 0, 4, 4, 4)
    one = F(1.0)
    xs = np.array([np.nextafter(one, F(0)), one, np.nextafter(one, F(2))], F)
    pts = np.stack([xs, np.full(3, 0.1, F), np.full(3, 0.1, F)], 1)
    assert ref.voxel_coords(pts, [0, 3], v2, r2)[:, 3].tolist() == [3, 4, 4]
    assert ref.voxel_coords(np.array([[np.nextafter(F(0), F(-1)), 0.1, 0.1]], F), [0, 1], v2, r2)[0, 3] == -1


def test_lattice_points_all_k():
    """p = lo + k*v computed in binary32 for every k of the x axis of the pillar grid: the coordinate is whatever ONE correctly
    rounded division gives — stated here with exact rational arithmetic — and a reciprocal multiply would differ for some k."""
    from fractions import Fraction
    v, lo = F(0.16), F(0.0)
    G = 432
    k = np.arange(G + 1, dtype=F)
    p = lo + k * v
    assert p.dtype == F
    pts = np.stack([p, np.full(G + 1, -39.0, F), np.full(G + 1, 0, F)], 1)
    got = ref.voxel_coords(pts, [0, G + 1], vc.PILLARS["v"], vc.PILLARS["r"])[:, 3]
    want, recip = [], []
    inv = F(1) / v
    for x in p:
        q = Fraction(float(x)) / Fraction(float(v))                                 # exact quotient of the two binary32 numbers
        qf = F(float(q)) if q.denominator == 1 else None
        if qf is None:                                                              # round to nearest binary32 via float64 (53 > 2*24 + 2 bits)
            qf = F(np.float64(q.numerator) / np.float64(q.denominator))
        g = int(np.floor(qf))
        want.append(g if 0 <= g < G else -1)
        recip.append(int(np.floor(F(x * inv))))
    assert got.tolist() == want
    assert got[0] == 0 and got[1] in (0, 1)
    assert any(a != b for a, b in zip(recip, want) if b >= 0), "the case no longer separates division from reciprocal multiply"


def test_cap_reached_mid_scene_and_empty_scene():
    v, r = (1, 1, 1), (0, 0, 0, 4, 4, 4)
    xs = [0.5, 1.5, 0.6, 2.5, 1.6, 3.5, 0.7, 9.0, 2.6]                              # keys 0 1 0 2 1 3 0 - 2 ; V = 2
    pts = np.array([[x, 0.5, 0.5, i] for i, x in enumerate(xs)], F)
    off = np.array([0, 0, 9, 9], np.int32)                                           # scenes 0 and 2 are empty
    for form in ("loop", "vec"):
        p2v, coors, count, voxel_num = ref.voxel_index(pts, off, v, r, 2, form)
        assert p2v.tolist() == [0, 1, 0, -1, 1, -1, 0, -1, -1]
        assert voxel_num.tolist() == [0, 2, 0] and count.tolist() == [[0, 0], [3, 2], [0, 0]]
        assert coors[1].tolist() == [[0, 0, 0], [0, 0, 1]] and (coors[0] == -1).all() and (coors[2] == -1).all()
    voxels, coors, num, voxel_num = ref.voxelize(pts, off, v, r, 2, 2)
    assert num.tolist() == [[0, 0], [2, 2], [0, 0]]
    assert voxels[1, 0, :, 3].tolist() == [0, 2] and voxels[1, 1, :, 3].tolist() == [1, 4]      # rows 0, 2 (6 is beyond T) and 1, 4
    assert not voxels[0].any() and not voxels[2].any()
    p0 = np.zeros((0, 4), F)
    out = ref.voxelize(p0, np.array([0, 0], np.int32), v, r, 2, 2)
    assert out[0].shape == (1, 2, 2, 4) and out[3].tolist() == [0]


def test_reduce_against_float64_and_autograd():
    import torch
    name, pts, off, p = vc.family_dense(4)[0]
    V = p["V"]
    p2v, _, count, _ = ref.voxel_index(pts, off, p["v"], p["r"], V)
    feat = np.random.default_rng(1).standard_normal((pts.shape[0], 5)).astype(F)
    rows, start = ref.member_lists(p2v, off, V)
    s_of = np.repeat(np.arange(len(start) - 1), np.diff(start))
    sum64 = np.zeros((len(start) - 1, 5))
    np.add.at(sum64, s_of, feat[rows].astype(np.float64))
    abs64 = np.zeros_like(sum64)
    np.add.at(abs64, s_of, np.abs(feat[rows]).astype(np.float64))
    n = np.diff(start)[:, None]
    out = ref.voxel_reduce(feat, p2v, off, V, "sum")[0].reshape(-1, 5)
    # n - 1 additions of one rounding each: |err| <= (n - 1) * 2^-24 * sum|x| to first order (2x margin for the second order)
    bound = 2 * np.maximum(n - 1, 0) * 2.0 ** -24 * abs64
    assert (np.abs(out - sum64) <= bound).all()
    mean = ref.voxel_reduce(feat, p2v, off, V, "mean")[0].reshape(-1, 5)
    assert (np.abs(mean - sum64 / np.maximum(n, 1)) <= (bound + 2.0 ** -24 * abs64) / np.maximum(n, 1) + 1e-30).all()
    mx, arg, cnt = ref.voxel_reduce(feat, p2v, off, V, "max")
    assert np.array_equal(cnt, count)
    # torch restatement on the CPU: index_add / index_reduce-free, by the sorted member lists
    sid = ref.scene_ids(off, len(p2v)).astype(np.int64)
    seg = torch.from_numpy(np.where(p2v >= 0, sid * V + p2v, len(start) - 1))        # dropped rows -> a dummy segment
    keep = torch.from_numpy(p2v >= 0)
    go = np.random.default_rng(2).standard_normal((len(off) - 1, V, 5)).astype(F)
    tgo = torch.from_numpy(go).reshape(-1, 5)
    for mode in ("sum", "mean", "max"):
        f = torch.from_numpy(feat).clone().requires_grad_(True)
        fk = f * keep[:, None]
        if mode == "max":
            o = torch.full((len(start), 5), -np.inf).scatter_reduce(0, seg[:, None].expand(-1, 5), torch.where(keep[:, None], f, torch.tensor(-np.inf)), "amax")[:-1]
            o = torch.where(torch.isinf(o), torch.zeros(()), o)
            assert np.array_equal(o.detach().numpy().reshape(mx.shape), mx)
            aux = arg
        else:
            o = torch.zeros((len(start), 5)).index_add(0, seg, fk)[:-1]
            if mode == "mean":
                o = o / torch.from_numpy(np.maximum(n, 1).astype(F))
            aux = count if mode == "mean" else None
        (o * tgo).sum().backward()
        want = f.grad.numpy()
        got = ref.voxel_reduce_grad(go, p2v, off, aux, mode)
        if mode == "max":
            # autograd splits a tie's gradient evenly; §20.5 gives it to the lowest row: compare where the maximum is unique
            taken = np.flatnonzero(p2v >= 0)
            uniq = np.ones_like(got, bool)
            vals = mx.reshape(-1, 5)[(sid * V + p2v)[taken]]
            is_max = feat[taken] == vals
            ties = np.zeros((len(start) - 1, 5), int)
            np.add.at(ties, (sid * V + p2v)[taken], is_max.astype(int))
            uniq[taken] = ties[(sid * V + p2v)[taken]] == 1
            assert np.array_equal(got[uniq], want[uniq])
        else:
            assert np.array_equal(got, want), mode
        assert not got[p2v < 0].any()


def test_header_binding_and_exports(sad):
    from sad_amd import _lib
    text = open(os.path.join(ROOT, "include", "sad_amd.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(sad_[a-z0-9_]+)\s*\(", text))
    for n in NAMES:
        assert n in declared, f"{n} not declared in include/sad_amd.h"
        assert n in _lib.SIGNATURES, f"{n} not bound in _lib.py"
    for c, val in (("SAD_VOXEL_SUM", 0), ("SAD_VOXEL_MEAN", 1), ("SAD_VOXEL_MAX", 2)):
        assert re.search(rf"#define\s+{c}\s+{val}\b", text)
    _lib.build()
    handle = ctypes.CDLL(_lib.SO_PATH)
    for n in NAMES:
        assert hasattr(handle, n), f"{n} not exported"
    assert _lib.lib().sad_version() == 4
    import sad_amd
    from sad_amd import ops, voxel
    assert sad_amd.voxelize is ops.voxelize and sad_amd.voxel_index is ops.voxel_index and sad_amd.voxel_coords is ops.voxel_coords
    assert sad_amd.voxel_reduce is ops.voxel_reduce and sad_amd.Voxelization is voxel.Voxelization
    assert sad_amd.DynamicScatter is voxel.DynamicScatter


def test_host_side_argument_errors(sad):
    """Refusals that need no GPU: every call fails on the host, nothing is launched (the pointers are never dereferenced)."""
    from sad_amd import _lib
    L = _lib.lib()
    p = 0x10000
    vs = (ctypes.c_float * 3)(0.4, 0.4, 0.4)
    pr = (ctypes.c_float * 6)(0, 0, 0, 4, 4, 4)
    n = ctypes.c_size_t(0)
    assert L.sad_voxel_workspace_bytes(1000, 2, 100, ctypes.byref(n)) == 0 and n.value >= 2048 * 12 + 3 * 1000 * 4 and n.value % 16 == 0
    assert L.sad_voxel_workspace_bytes(0, 1, 1, ctypes.byref(n)) == 0 and n.value > 0
    assert L.sad_voxel_workspace_bytes(-1, 2, 100, ctypes.byref(n)) == -1 and n.value == 0
    assert L.sad_voxel_workspace_bytes(1000, 0, 100, ctypes.byref(n)) == -1
    assert L.sad_voxel_workspace_bytes(1000, 2, 0, ctypes.byref(n)) == -1
    assert L.sad_voxel_workspace_bytes(1000, 2, 100, None) == -1
    fine = (ctypes.c_float * 3)(0.001, 0.001, 0.001)
    flat = (ctypes.c_float * 3)(0.4, 0.4, 10.0)
    for vsz, code, needle in ((fine, -2, b"2^31 - 1"), (flat, -2, b"< 1")):
        assert L.sad_voxel_coords_f32(p, p, 64, 1, 4, vsz, pr, p, None) == code and needle in L.sad_last_error()
        assert L.sad_voxel_index_f32(p, p, 64, 1, 4, vsz, pr, 10, p, p, p, p, p, None) == code and needle in L.sad_last_error()
        assert L.sad_voxelize_f32(p, p, 64, 1, 4, vsz, pr, 4, 10, p, p, p, p, p, None) == code and needle in L.sad_last_error()
    assert L.sad_voxel_coords_f32(p, p, 64, 1, 2, vs, pr, p, None) == -1 and b"C >= 3" in L.sad_last_error()
    assert L.sad_voxel_index_f32(p, p, 64, 1, 2, vs, pr, 10, p, p, p, p, p, None) == -1 and b"C >= 3" in L.sad_last_error()
    assert L.sad_voxelize_f32(p, p, 64, 1, 2, vs, pr, 4, 10, p, p, p, p, p, None) == -1 and b"C >= 3" in L.sad_last_error()
    assert L.sad_voxelize_f32(p, p, 64, 1, 4, vs, pr, 0, 10, p, p, p, p, p, None) == -1 and b"max_points" in L.sad_last_error()
    assert L.sad_voxelize_f32(p, p, 64, 1, 4, vs, pr, 4, 0, p, p, p, p, p, None) == -1 and b"max_voxels" in L.sad_last_error()
    assert L.sad_voxelize_f32(p, p, 64, 1, 4, vs, pr, 4, 10, p, p, p, p, None, None) == -1 and b"NULL" in L.sad_last_error()
    assert L.sad_voxel_index_f32(p, None, 64, 1, 4, vs, pr, 10, p, p, p, p, p, None) == -1 and b"NULL" in L.sad_last_error()
    assert L.sad_voxel_reduce_f32(p, p, p, 64, 1, 4, 10, 3, p, p, None, p, None) == -1 and b"mode" in L.sad_last_error()
    assert L.sad_voxel_reduce_f32(p, p, p, 64, 1, 4, 10, 2, p, None, None, p, None) == -1 and b"arg" in L.sad_last_error()
    assert L.sad_voxel_reduce_f32(p, p, p, 64, 1, 0, 10, 0, p, None, None, p, None) == -1 and b"Cf" in L.sad_last_error()
    assert L.sad_voxel_reduce_grad_f32(p, p, p, 64, 1, 4, 10, 1, None, p, None) == -1 and b"count" in L.sad_last_error()
    assert L.sad_voxel_reduce_grad_f32(p, p, p, 64, 1, 4, 10, 5, p, p, None) == -1 and b"mode" in L.sad_last_error()


def test_ops_refuse_bad_inputs_without_a_gpu(sad):
    import torch
    from sad_amd import ops
    x = torch.zeros(64, 4)
    off = torch.tensor([0, 64], dtype=torch.int32)
    v, r = (0.4, 0.4, 0.4), (0, 0, 0, 4, 4, 4)
    for fn in (lambda: ops.voxel_coords(x, off, v, r), lambda: ops.voxel_index(x, off, v, r, 10), lambda: ops.voxelize(x, off, v, r, 4, 10),
               lambda: ops.voxel_reduce(x, torch.zeros(64, dtype=torch.int32), off, 10, "sum"),
               lambda: ops.voxelize(torch.zeros(2, 32, 4), None, v, r, 4, 10)):
        with pytest.raises(RuntimeError, match="no CPU path"):
            fn()
    with pytest.raises(ValueError, match="mode"):
        ops.voxel_reduce(x, torch.zeros(64, dtype=torch.int32), off, 10, "median")
    with pytest.raises(ValueError, match="3 entries"):
        ops.voxel_coords(x, off, (0.4, 0.4), r)
    import sad_amd
    with pytest.raises(ValueError):
        sad_amd.DynamicScatter("median")
    m = sad_amd.Voxelization(v, r, None, 10)
    assert m.max_points is None and "max_voxels=10" in repr(m)
