"""SPEC.md §30 without a GPU: the two forms of the reference agree on every case of tests/voxel_roi_ref.py, the cases hold what
their names say, and every refusal of the host code is pinned.

The C entry points sad_voxel_query_f32, sad_roi_grid_points_f32 and sad_voxel_query_workspace_bytes: the return code AND the
text of sad_last_error() are compared with tests/golden/voxel_roi_refusals.json; argument blocks hold fake non-null device
pointers, nothing is dereferenced, every case is refused before a launch.
    python tests/test_voxel_roi_cpu.py          (rewrites the fixture from the library that is built in the tree)"""
import ctypes
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))      # (run as a script: the package and the oracle)
import voxel_roi_ref as ref  # noqa: E402

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "voxel_roi_refusals.json")
P = 0x10000                                           # a fake device pointer
NAN = float("nan")
CASES = [(f, r, S) for f in ref.FAMILIES for r in ref.RANGES for S in ref.SIZES]


# ---- the reference -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family,max_range,S", CASES)
def test_the_two_forms_agree(family, max_range, S):
    coors, offsets, shape, vs, pr, new_xyz, radius = ref.query_args(family)
    idx, cnt = ref.expected(family, max_range, S)
    bidx, bcnt = ref.query_brute(coors, offsets, shape, vs, pr[:3], new_xyz, max_range, radius, S)
    assert np.array_equal(cnt, bcnt) and np.array_equal(idx, bidx)
    assert (cnt[1] == 0).all() and (idx[1] == 0).all(), "the middle scene is empty"
    assert ((idx >= 0) & (idx < len(coors))).all()
    scene = np.searchsorted(offsets, idx, side="right") - 1
    assert (scene[cnt > 0] == np.nonzero(cnt > 0)[0][:, None]).all(), "a row of another scene"


@pytest.mark.parametrize("name", ["widest", "cell limit"])
def test_the_two_forms_agree_on_the_extra_cases(name):
    coors, offsets, shape, vs, pr, new_xyz, max_range, radius, S = ref.extra_cases()[name]
    form = ref.query_brute if name == "widest" else ref.query_walk         # (the literal walk of 4 913 cells per query is slow)
    idx, cnt = form(coors, offsets, shape, vs, pr[:3], new_xyz, max_range, radius, S)
    assert (cnt == S).any() and (cnt == 0).any() and ((cnt > 0) & (cnt < S)).any()
    if name == "cell limit":
        bidx, bcnt = ref.query_brute(coors, offsets, shape, vs, pr[:3], new_xyz, max_range, radius, S)
        assert np.array_equal(cnt, bcnt) and np.array_equal(idx, bidx)
        key = (coors[:, 0].astype(np.int64) * shape[1] + coors[:, 1]) * shape[2] + coors[:, 2]
        assert key.max() > 2 ** 31 - 2 ** 24 and key.max() <= 2 ** 31 - 1 and shape[0] * shape[1] * shape[2] <= 2 ** 31 - 1
        assert key[idx[cnt > 0][:, 0]].max() > 2 ** 31 - 2 ** 24, "no accepted voxel at the far corner"
    else:
        some = [m for m in range(0, new_xyz.shape[1], 9)]
        widx, wcnt = ref.query_walk(coors, offsets, shape, vs, pr[:3], new_xyz[:, some], max_range, radius, S)
        assert np.array_equal(cnt[:, some], wcnt) and np.array_equal(idx[:, some], widx)


def test_the_cases_hold_what_they_name():
    coors, offsets = ref.grid()
    assert offsets[1] == offsets[2] and 280 <= len(coors) <= 320
    keys = [tuple(c) for c in coors[offsets[2]:]]
    assert len(set(keys)) == len(keys) - 1, "scene 2 holds one coordinate twice"
    assert len({tuple(c) for c in coors[:offsets[1]]}) == offsets[1]
    for family, (vs, pr, radius) in ref.FAMILIES.items():
        q = ref.queries(family)
        assert q.shape == (3, 67, 3)
        cells = [ref.query_cell(p, vs, pr[:3]) for p in q[0]]
        assert sum(c is None for c in cells) == 5, "NaN, +Inf, -Inf and the two absurd points are empty queries"
        for axis, G in enumerate(ref.SHAPE[::-1]):
            assert any(c is not None and c[axis] == -1 for c in cells) and any(c is not None and c[axis] == G for c in cells)
        total = ref.accepted_total(*ref.query_args(family)[:4], pr[:3], q, (4, 4, 4), radius)
        assert total.max() < 128, "S = 128 is larger than any ball holds"
        assert total.max() > 16, "S = 16 is filled by some ball"
        # outside the grid, yet with neighbours
        out = np.array([c is not None and not all(0 <= c[a] < G for a, G in enumerate(ref.SHAPE[::-1])) for c in cells])
        assert (total[0][out] > 0).any() and (total[2][out] > 0).any()
    # the exact family: a voxel at d2 == r2 is rejected, the query one ulp inside accepts it
    coors, offsets, shape, vs, pr, q, radius = ref.query_args("exact")
    all_idx, all_cnt = ref.query_brute(coors, offsets, shape, vs, pr[:3], q, (4, 4, 4), radius, 128)
    k = 0
    for i in (0, 3, 11, int(offsets[2]) + 2, int(offsets[2]) + 9):
        b = 0 if i < offsets[1] else 2
        for axis in range(3):
            on, inside = k, k + 1
            k += 2
            if axis == 2:
                continue                                # (1.5 along z is 6 cells: out of every range)
            assert i not in all_idx[b, on, :all_cnt[b, on]] and i in all_idx[b, inside, :all_cnt[b, inside]]


@pytest.mark.parametrize("G", [1, 2, 6])
def test_grid_points_forms_agree(G):
    for D in (7, 9):
        rois = ref.rois_case(D)
        for count in (None, np.array([4, 0], np.int32), np.array([-3, 99], np.int32)):
            a, b = ref.grid_points_loop(rois, count, G), ref.grid_points_vec(rois, count, G)
            assert np.array_equal(a.view(np.int32), b.view(np.int32))
            if count is not None:
                n = np.clip(count, 0, 9)
                assert all((a[s, n[s]:].view(np.uint32) == ref.NAN_BITS).all() and np.isfinite(a[s, :n[s]]).all() for s in range(2))
    # a box at the origin without rotation: the points are the centres of the G^3 sub-boxes, x slowest
    box = np.array([[[0, 0, 0, 2, 4, 8, 0]]], ref.F)
    pts = ref.grid_points_loop(box, None, 2)[0, 0]
    assert np.array_equal(pts, np.array([[x, y, z] for x in (-0.5, 0.5) for y in (-1, 1) for z in (-2, 2)], ref.F))


# ---- refusals of the host code -------------------------------------------------------------------------------------------------
QUERY = dict(coors=P, offsets=P, new_xyz=P, Nv=300, B=3, M=67, S=16, spatial_shape=(5, 12, 12), max_range=(1, 2, 3),
             voxel_size=(0.5, 0.5, 0.25), lo=(-3.0, -3.0, -0.5), radius=1.0, idx=P, cnt=P, workspace=P)
QUERY_CASES = [("null", None), ("struct_size", dict(struct_size=-8)), ("struct_size+S=129", dict(struct_size=8, S=129))] + [
    (f, {f: None}) for f in ("coors", "offsets", "new_xyz", "idx", "cnt", "workspace")] + [
    ("B=0", dict(B=0)), ("S=0", dict(S=0)), ("M=-1", dict(M=-1)), ("Nv=-1", dict(Nv=-1)),
    ("rz=-1", dict(max_range=(-1, 2, 3))), ("rx=-1", dict(max_range=(1, 2, -1))), ("rz=9", dict(max_range=(9, 2, 3))),
    ("ry=9", dict(max_range=(1, 9, 3))), ("rx=9", dict(max_range=(1, 2, 9))), ("rx=8", dict(max_range=(8, 8, 8), idx=None)),
    ("S=129", dict(S=129)), ("S=128", dict(S=128, idx=None)), ("B=65536", dict(B=65536)), ("B*M*S=2^31", dict(B=2, M=1 << 24, S=64)),
    ("Nv=2^30+1", dict(Nv=(1 << 30) + 1)), ("grid 2^31", dict(spatial_shape=(2, 1 << 15, 1 << 15))),
    ("grid 2^31-1", dict(spatial_shape=(1, 1, (1 << 31) - 1), idx=None)), ("Gz=0", dict(spatial_shape=(0, 12, 12))),
    ("radius=0", dict(radius=0.0)), ("radius<0", dict(radius=-1.0)), ("radius nan", dict(radius=NAN)),
    ("radius nan+S=129", dict(radius=NAN, S=129)),
    ("vx=0", dict(voxel_size=(0.0, 0.5, 0.25))), ("vz nan", dict(voxel_size=(0.5, 0.5, NAN))), ("lo inf", dict(lo=(-3.0, float("inf"), 0.0))),
    ("workspace align", dict(workspace=P + 4)), ("S=129+workspace", dict(S=129, workspace=None)),
]
POINTS = dict(rois=P, roi_count=P, B=2, R=9, D=7, G=6, pts=P)
POINTS_CASES = [("null", None), ("struct_size", dict(struct_size=8)), ("rois", dict(rois=None)), ("pts", dict(pts=None)),
                ("B=0", dict(B=0)), ("R=0", dict(R=0)), ("G=0", dict(G=0)), ("D=6", dict(D=6)), ("D=6+G=17", dict(D=6, G=17)),
                ("G=17", dict(G=17)), ("B=65536", dict(B=65536)), ("B*R*G^3=2^31", dict(B=128, R=4096, G=16))]
SIZES = [0, 1, 300, 1 << 30, -1, (1 << 30) + 1]


def _block(cls, base, ov):
    if ov is None:
        return None
    f = dict(base, **ov)
    a = cls()
    a.struct_size = ctypes.sizeof(cls) + f.pop("struct_size", 0)
    for k, v in f.items():
        if isinstance(v, tuple):
            getattr(a, k)[:] = v
        else:
            setattr(a, k, v)
    return a


def outcomes():
    """{case name: [return code, message] or a size} of every case, from the library that is loaded."""
    from sad_amd import _lib
    L = _lib.lib()
    got = {}
    for what, cls, fn, base, cases in (("voxel_query", _lib.VoxelQueryArgs, L.sad_voxel_query_f32, QUERY, QUERY_CASES),
                                       ("roi_grid_points", _lib.RoiGridPointsArgs, L.sad_roi_grid_points_f32, POINTS, POINTS_CASES)):
        assert len({name for name, _ in cases}) == len(cases)
        for name, ov in cases:
            a = _block(cls, base, ov)
            code = fn(ctypes.byref(a) if a is not None else None, None)
            assert code in (-1, -2), f"{what}: {name} was not refused on the host (code {code})"
            got[f"{what}: {name}"] = [code, L.sad_last_error().decode()]
    for n in SIZES:
        got[f"voxel_query_workspace_bytes({n})"] = L.sad_voxel_query_workspace_bytes(n)
    return got


def test_refusals_match_the_recorded_ones(sad):
    want = json.load(open(FIXTURE))
    got = outcomes()
    assert sorted(got) == sorted(want), "the cases of this file and of the fixture differ"
    wrong = {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    assert not wrong, f"{len(wrong)} refusals changed (got, recorded): {wrong}"


def test_the_recorded_codes_are_the_ones_the_section_names():
    """SAD_EUNSUPPORTED (-2) above the caps and only there, SAD_EINVAL (-1) for the rest.  The cases at a cap (rx=8, S=128, the
    grid of 2^31 - 1 cells) pass the caps and are refused for the NULL idx they carry.  The size is the table's: a power of two >= 2 Nv (>= 2)
    slots, 8 bytes of key and 4 of value each, either slice at least 16 bytes."""
    want = json.load(open(FIXTURE))
    caps = {"voxel_query: " + n for n in ("rz=9", "ry=9", "rx=9", "S=129", "B=65536", "B*M*S=2^31", "Nv=2^30+1", "grid 2^31", "S=129+workspace")}
    caps |= {"roi_grid_points: " + n for n in ("G=17", "B=65536", "B*R*G^3=2^31")}
    for k, v in want.items():
        if isinstance(v, list):
            assert v[0] == (-2 if k in caps else -1) and v[1], k
    for k in ("voxel_query: rx=8", "voxel_query: S=128", "voxel_query: grid 2^31-1"):
        assert "NULL pointer" in want[k][1], k
    assert "struct_size" in want["voxel_query: struct_size"][1] and "struct_size" in want["voxel_query: struct_size+S=129"][1]
    assert "radius" in want["voxel_query: radius nan"][1] and "radius" in want["voxel_query: radius nan+S=129"][1]
    for n in SIZES:
        slots = 2
        while slots < 2 * n:
            slots *= 2
        assert want[f"voxel_query_workspace_bytes({n})"] == (max(8 * slots, 16) + max(4 * slots, 16) if 0 <= n <= 1 << 30 else 0)


# ---- the operators -------------------------------------------------------------------------------------------------------------
def test_operator_argument_errors(sad):
    """A wrong dtype, shape or scalar is judged before any device, so CPU tensors reach the operators; a CPU tensor that is
    otherwise right is refused as such."""
    import torch
    from sad_amd import ops
    rois = torch.zeros(2, 9, 7)
    for bad in (torch.zeros(2, 9, 7, dtype=torch.float64), None):
        with pytest.raises(TypeError):
            ops.roi_grid_points(bad, None, 6)
    with pytest.raises(TypeError):
        ops.roi_grid_points(rois, torch.zeros(2, dtype=torch.int64), 6)
    for bad, count, G in ((torch.zeros(2, 9, 6), None, 6), (torch.zeros(18, 7), None, 6), (torch.zeros(2, 0, 7), None, 6),
                          (rois, torch.zeros(3, dtype=torch.int32), 6), (rois, None, 0), (rois, None, 17),
                          (torch.zeros(2, 9, 14)[..., ::2], None, 6)):
        with pytest.raises(ValueError):
            ops.roi_grid_points(bad, count, G)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.roi_grid_points(rois, torch.zeros(2, dtype=torch.int32), 6)

    coors, offsets, q = torch.zeros(10, 3, dtype=torch.int32), torch.zeros(4, dtype=torch.int32), torch.zeros(3, 5, 3)
    kw = dict(max_range=(1, 2, 3), radius=1.5, S=16)
    vs, pr = (0.5, 0.5, 0.25), (-3, -3, -0.5, 3, 3, 0.75)
    for change in (dict(max_range=(1, 2)), dict(max_range=2), dict(max_range=(1, 2, 9)), dict(max_range=(-1, 2, 3)), dict(S=0), dict(S=129),
                   dict(radius=0.0), dict(radius=NAN), dict(radius=-2.0)):
        with pytest.raises(ValueError):
            ops.voxel_query(coors, offsets, (5, 12, 12), vs, pr, q, **dict(kw, **change))
    for shape in ((5, 12), (0, 12, 12), (2, 1 << 15, 1 << 15)):
        with pytest.raises(ValueError):
            ops.voxel_query(coors, offsets, shape, vs, pr, q, **kw)
    with pytest.raises(ValueError):
        ops.voxel_query(coors, offsets, (5, 12, 12), (0.5, 0.5), pr, q, **kw)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.voxel_query(coors, offsets, (5, 12, 12), vs, pr, q, **kw)


def test_out_and_workspace_checks(sad):
    """The two checkers voxel_query hands its `out=` pair and its workspace to, with a CPU device standing in."""
    import torch
    from sad_amd import ops, _lib
    cpu = torch.device("cpu")
    spec = (("idx", (3, 5, 16), torch.int32), ("cnt", (3, 5), torch.int32))
    good = tuple(torch.zeros(shape, dtype=dt) for _, shape, dt in spec)
    assert ops._outputs(spec, good, cpu, "coors") == good
    for bad in (good[:1], good[::-1], (good[0].to(torch.int64), good[1]), (torch.zeros(3, 16, 5, dtype=torch.int32).transpose(1, 2), good[1])):
        with pytest.raises(ValueError, match="out: expected contiguous"):
            ops._outputs(spec, bad, cpu, "coors")
    nbytes = _lib.lib().sad_voxel_query_workspace_bytes(300)
    assert nbytes == 12 * 1024
    with pytest.raises(ValueError, match=f"at least {nbytes} bytes"):
        ops._workspace(nbytes, torch.zeros(nbytes - 1, dtype=torch.uint8), cpu, "ops.voxel_query_workspace", 16)
    with pytest.raises(ValueError, match="0 <= Nv <= 2\\^30"):
        ops.voxel_query_workspace(-1, cpu)


def test_module_construction(sad):
    from sad_amd import VoxelRoIPool
    scale = dict(in_channels=16, voxel_size=(0.1, 0.1, 0.2), max_range=(2, 2, 2), radius=0.4, nsample=16, mlp=[16, 16])
    m = VoxelRoIPool(6, [scale, dict(scale, in_channels=32, mlp=[32])], (0, -40, -3, 70.4, 40, 1))
    assert m.out_channels == 48 and len(m.weight) == 2
    assert tuple(m.weight[0][0].shape) == (16, 19) and tuple(m.weight[0][1].shape) == (16, 16) and tuple(m.weight[1][0].shape) == (32, 35)
    assert not any(p.requires_grad for p in m.parameters())
    for bad in (dict(scale, nsample=65), dict(scale, mlp=[]), dict(scale, max_range=(2, 2)), dict(scale, in_channels=0)):
        with pytest.raises(ValueError):
            VoxelRoIPool(6, [bad], (0, -40, -3, 70.4, 40, 1))
    with pytest.raises(ValueError):
        VoxelRoIPool(17, [scale], (0, -40, -3, 70.4, 40, 1))


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    res = outcomes()
    with open(FIXTURE, "w") as fh:
        json.dump(res, fh, indent=0, sort_keys=True)
        fh.write("\n")
    print(f"recorded {len(res)} refusals -> {FIXTURE}")
