"""CPU checks of tests/edge_regimes.py: every case reaches the regime it is named after (asserted statistics), the grid model is
trustworthy on friendly scenes, it shows the hole of the constant 1.001 margin on `thin_line` and its absence under the slack
bound of csrc/ball_query_grid.hip, lidar-shaped geometries are the same under both rules, and the oracle agrees with plain
float32 numpy on the small cases — so a disagreement on the GPU is not the oracle's."""
import numpy as np
import pytest

import edge_regimes as er

F = np.float32


def _regime(cid):
    return cid.rstrip("0123456789")


@pytest.mark.parametrize("cid", er.CASE_IDS)
def test_case_reaches_its_regime(cid):
    c, reg = er.case(cid), _regime(cid)
    s = c.stats
    if reg == "thin_line":
        assert s["g_old"] == (29593, 1, 1) and c.xyz[0, -1, 0] == er.LINE_P and c.new_xyz[0, 0, 0] == er.LINE_C
        assert s["census_old"][2] >= 1, "the 1.001 margin alone must leave an accepted pair two cells apart"
        assert s["census_old"][1] >= 100 and s["census_new"][1] >= 100, "pairs on both sides of a cell border"
        assert s["census_new"][2] == 0 and s["g_new"][0] < s["g_old"][0]
    elif reg == "thin_plane":
        assert s["flat"] and s["census_new"][2] == 0 and s["census_new"][1] >= 300
        if "box" in c.name:
            assert s["steps"] >= 1 and s["g_new"][0] * s["g_new"][1] <= er.GRID_MAXC < 181 * 181 * 5
        else:
            assert s["steps"] == 0 and s["g_new"] == (181, 181, 1)
    elif reg == "offset":
        assert 0.01 <= s["ulp_over_rmin"] <= 0.1
        assert s["d2_ties"] > 100 and s["distinct_d2"] < c.N
    elif reg == "shell":
        assert min(s["at"], s["inside"], s["outside"]) >= 10 and s["on_border"] >= 4
        want = {"r1h": "cand_le64", "r1.5h": "cand_le128", "r3h": "cand_gt128"}[c.name.split("-")[1]]
        assert s[want] >= 200, s
    elif reg == "outside":
        assert s["missed"] == 0 and s["flat"] == ("flat" in c.name)
        assert 0 < s["with_accepted"] < s["with_candidates"] < c.M and s["clamped"] >= 26
    elif reg == "tiny":
        assert s["neg_zero"] > 0 and s["accepted"] > c.M and s["subnormal_terms"] > 10000
        if "2^-60" in c.name:
            assert s["normal_terms"] > 10000 and not s["r2_subnormal"]
        else:
            assert s["normal_terms"] == 0 and s["zero_terms"] > 0 and s["r2_subnormal"]
    elif reg == "huge":
        assert s["inf_d2"] > 1000 and s["finite_d2"] > 1000 and s["r2_inf"] and 0 < s["accepted"] < s["finite_d2"]
    elif reg == "outlier":
        assert s["steps"] >= 30 and s["biggest_cell"] >= c.N - 3
    elif reg == "exhaust":
        assert s["distinct"] == 37 and c.npoint == c.N
    else:
        raise AssertionError(reg)


def test_every_regime_has_sizes_on_both_sides_of_the_grid_threshold():
    for reg in er.BUILDERS:
        n = [er.case(c).N for c in er.ids(reg)]
        if reg in ("tiny", "huge"):
            assert max(n) <= 4096
        if reg != "exhaust":
            assert min(n) < er.GRID_MIN_POINTS <= max(n), reg
    assert sum(er.case(c).N > 16384 for c in er.CASE_IDS) >= 5


def _friendly():
    from sad_amd import synth
    rng = np.random.default_rng(11)
    cube = rng.uniform(0, 1, (3000, 3)).astype(F)
    kitti = synth.make_scene(3, 4096)[:, :3]
    return [(cube, cube[::12], 0.1), (cube, cube[::12] + F(0.3), 0.25), (kitti, kitti[::16], 0.8), (kitti, kitti[::16], 4.8)]


@pytest.mark.parametrize("bounded", [False, True])
def test_model_equals_brute_force_on_friendly_scenes(bounded):
    for xyz, cen, r in _friendly():
        geo = er.scene_geometry(xyz, r, bounded)
        mask = er.reach(geo, xyz, cen)
        assert mask.sum() < 0.5 * mask.size or max(geo["g"]) <= 3, "the model prunes"
        np.testing.assert_array_equal(er.ball_query_np(r, 32, xyz, cen, mask), er.ball_query_np(r, 32, xyz, cen))


def test_model_loses_a_neighbour_on_thin_line_with_the_constant_margin():
    """The failing-before evidence that needs no GPU: with the 1.001 margin alone the +-1 neighbourhood of centroid 0 (the
    counterexample's pair) does not contain its accepted point N-1; with the slack bound it does, for every centroid."""
    c = er.case("thin_line1")
    xyz, cen, r = c.xyz[0], c.new_xyz[0], c.radii[0]
    want = er.ball_query_np(r, 32, xyz, cen)
    old = er.ball_query_np(r, 32, xyz, cen, er.reach(er.scene_geometry(xyz, r, False), xyz, cen))
    assert c.N - 1 in want[0] and c.N - 1 not in old[0]
    assert not np.array_equal(old, want)
    new = er.ball_query_np(r, 32, xyz, cen, er.reach(er.scene_geometry(xyz, r, True), xyz, cen))
    np.testing.assert_array_equal(new, want)


def test_counterexample_literals_fall_two_cells_apart():
    cs = F(er.LINE_R * er.GRID_MARGIN)
    inv = F(1) / cs
    assert cs == F(1.108878)
    assert er.cell_coord(er.LINE_C, er.LINE_X0, inv, 29593) == 29590 and er.cell_coord(er.LINE_P, er.LINE_X0, inv, 29593) == 29592
    dx = F(er.LINE_P - er.LINE_C)
    assert dx == F(1.1074219) and dx * dx < er.LINE_R * er.LINE_R


def test_randomized_line_search():
    """300 line-like scenes x 2*10^5 pairs one step below r^2.  Near the cap of 32 768 cells per axis the constant margin leaves
    accepted pairs two cells apart; the slack bound leaves none there, and none at ~2 080 cells, the largest count for which the
    bound still keeps the 1.001 edge (the thinnest slack per cell it ever allows)."""
    bad, worst, gmax = er.line_search(300, 200000, 32767, bounded=False)
    assert bad > 0 and worst == 2 and 29000 < gmax <= er.GRID_MAXC
    assert er.line_search(300, 200000, 32767, bounded=True)[:2] == (0, 1)
    bad, worst, gmax = er.line_search(300, 200000, 2080, bounded=True)
    assert (bad, worst) == (0, 1) and 2000 < gmax <= 2081, "the 1.001 edge must survive here"


@pytest.mark.parametrize("r", [0.8, 4.8])
def test_lidar_shaped_geometry_is_unchanged_by_the_slack_bound(r):
    """The timed path cannot move: KITTI-, nuScenes- and TINY-shaped scenes get the same cells under both rules."""
    from sad_amd import synth
    scenes = [synth.make_scene(0, 16384)[:, :3], synth.make_scene(5, 16384)[:, :3], synth.make_nuscenes_batch(0, 1)[0, :, :3],
              synth.make_tiny_batch(0, 1)[0, :, :3], synth.make_dense_batch(0, 1)[0, :, :3]]
    for xyz in scenes:
        a, b = er.scene_geometry(xyz, r, False), er.scene_geometry(xyz, r, True)
        assert a["g"] == b["g"] and a["cs"] == b["cs"] and a["flat"] == b["flat"] and a["steps"] == b["steps"]
        assert max(a["g"]) < 600


SMALL = [c for c in er.CASE_IDS if c in ("thin_line0", "thin_line1", "thin_plane0", "offset0", "offset1", "shell0", "shell2", "outside0",
                                         "tiny0", "tiny1", "tiny2", "huge0", "huge1", "outlier0", "outlier1")]


@pytest.mark.parametrize("cid", SMALL)
def test_oracle_equals_float32_numpy_on_small_cases(orc, cid):
    c = er.case(cid)
    xyz, cen = c.xyz[0], c.new_xyz[0, :64]
    for r, s in zip(c.radii, c.nsamples):
        np.testing.assert_array_equal(orc.ball_query(r, s, c.xyz, c.new_xyz[:, :64])[0], er.ball_query_np(r, s, xyz, cen))
    np.testing.assert_array_equal(orc.knn_query(16, c.xyz, c.new_xyz[:, :64])[0], er.knn_np(16, xyz, cen))
    np.testing.assert_array_equal(orc.fps(c.xyz, 96)[0], er.fps_np(xyz, 96))


def test_oracle_fps_falls_back_to_index_zero_when_exhausted(orc):
    c = er.case("exhaust0")
    got = orc.fps(c.xyz, c.N)[0]
    assert len(set(got[:37].tolist())) == 37 and not got[37:].any()
    np.testing.assert_array_equal(got[:64], er.fps_np(c.xyz[0], 64))
