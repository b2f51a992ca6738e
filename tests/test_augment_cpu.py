"""The numpy reference of SPEC.md §35 against itself (tests/augment_ref.py): the loop form equals the vectorised form, the
outputs have the properties the section promises, the cases stay inside the kernel's contract and every named case does what its
name says.  The host side of ``augment.GTDatabase`` is checked here too.  No GPU."""
import numpy as np
import pytest

import augment_ref as ref
import box_ref

F = np.float32


@pytest.fixture(autouse=True)
def _oracle(orc):
    return orc


def _scene(c, b):
    return c["points"][c["offsets"][b]:c["offsets"][b + 1]]


def _accepted(c, out, b):
    return c["db"]["boxes"][out["db_index"][b][out["keep"][b] == 1]]


@pytest.mark.parametrize("name", ref.CASES)
def test_loop_equals_vectorised(name):
    c = ref.case(name)
    vec, loop = ref.expected(name), ref.gt_paste_loop(c)
    for k in vec:
        np.testing.assert_array_equal(vec[k], loop[k], err_msg=f"{name}: {k}")
    P = ref.draw_params(ref.call_seed(5, 2), 3, **ref.GLOBAL)
    vel = c["gt_boxes"].shape[2] >= 9
    fv, fl = ref.gt_paste_vec(c, P, vel), ref.gt_paste_loop(c, P, vel)
    for k in fv:
        np.testing.assert_array_equal(fv[k], fl[k], err_msg=f"{name} fused: {k}")
    # the fused form is the transform of the plain form
    pts, boxes = ref.apply_params(vec["out_points"], vec["out_offsets"], vec["boxes_out"], P, vel)
    np.testing.assert_array_equal(fv["out_points"], pts)
    np.testing.assert_array_equal(fv["boxes_out"], boxes)


@pytest.mark.parametrize("name", ref.CASES)
def test_properties_and_contract(name):
    c, out = ref.case(name), ref.expected(name)
    B, G, D = c["gt_boxes"].shape
    Q, C = sum(c["sample_num"]), len(c["sample_num"])
    assert B == 3 and 1 <= Q <= ref.MAX_SLOTS and G <= 1024 and C <= 16
    assert np.abs(c["gt_boxes"][..., 6]).max(initial=0) < 1e4 and np.abs(c["db"]["boxes"][:, 6]).max() < 1e4
    assert c["db"]["class_offsets"][0] == 0 and c["db"]["class_offsets"][-1] == c["db"]["boxes"].shape[0]
    assert np.diff(c["db"]["offsets"]).max() <= c["Pmax"]
    R = c["points"].shape[0] + B * Q * c["Pmax"]
    assert out["out_offsets"][-1] <= R and R * c["points"].shape[1] < 2 ** 31
    for b in range(B):
        acc = _accepted(c, out, b)
        gt = c["gt_boxes"][b][ref.valid_gt(c["gt_boxes"][b], c["gt_labels"][b], C)]
        for i in range(acc.shape[0]):                    # pairwise disjoint, and disjoint from the ground truth
            assert all(box_ref.iou_bev_pair(acc[i], acc[j]) == 0 for j in range(i))
            assert all(box_ref.iou_bev_pair(acc[i], g) == 0 for g in gt)
        scene = _scene(c, b)
        rem = box_ref.inside(scene[:, :3], acc, c["e"]).any(1) if acc.shape[0] else np.zeros(scene.shape[0], bool)
        pasted = sum(int(c["db"]["offsets"][d + 1] - c["db"]["offsets"][d]) for d in out["db_index"][b][out["keep"][b] == 1])
        rows = out["out_points"][out["out_offsets"][b]:out["out_offsets"][b + 1]]
        assert rows.shape[0] == pasted + scene.shape[0] - int(rem.sum()), "point rows are not conserved"
        surv = rows[pasted:]
        np.testing.assert_array_equal(surv, scene[~rem], err_msg="the survivors are not the scene's rows in file order")
        if acc.shape[0]:
            assert not box_ref.inside(surv[:, :3], acc, c["e"]).any(), "a surviving scene point lies in an accepted box"
        n = int(out["num_pasted"][b])
        assert n == acc.shape[0] and (out["labels_out"][b, G + n:] == -1).all() and not out["boxes_out"][b, G + n:].any()
        assert (out["db_index"][b][out["keep"][b] == 1] >= 0).all()


def test_seed_and_step():
    name = "q20_c4_d7_g6"
    c = ref.case(name)
    again = ref.gt_paste_vec(dict(c))
    for k, v in ref.expected(name).items():
        np.testing.assert_array_equal(v, again[k])
    seed, step = c["seed_step"]
    assert c["seed"] == ref.call_seed(seed, step)
    other = ref.gt_paste_vec(dict(c, seed=ref.call_seed(seed, step + 1)))
    assert not np.array_equal(other["db_index"], again["db_index"])
    a, b = (ref.draw_params(ref.call_seed(5, s), 3, **ref.GLOBAL) for s in (0, 1))
    np.testing.assert_array_equal(a, ref.draw_params(ref.call_seed(5, 0), 3, **ref.GLOBAL))
    assert not np.array_equal(a, b)
    lo, hi = ref.GLOBAL["rot_range"]
    assert (a[:, 1] >= F(lo)).all() and (a[:, 1] <= F(hi)).all() and (a[:, 4] >= F(0.95)).all() and (a[:, 4] <= F(1.05)).all()
    assert (np.abs(a[:, 5:]) <= np.array(ref.GLOBAL["translate_range"], F)).all()
    # the draws of §35.1 and §35.2 never share a hash index
    assert ref.DRAW_GLOBAL + 7 <= ref.DRAW_PASTE and ref.DRAW_PASTE + ref.MAX_SLOTS < 2 ** 32 - 1


def test_identity_and_transform_order():
    c = ref.case("q20_c5_d9_g1")
    pts, boxes, P = ref.global_augment(c["points"], c["offsets"], c["gt_boxes"], ref.call_seed(1, 0), True, **ref.IDENTITY)
    np.testing.assert_array_equal(pts, c["points"])
    np.testing.assert_array_equal(boxes, c["gt_boxes"])
    np.testing.assert_array_equal(P, np.tile(np.array([0, 0, 1, 0, 1, 0, 0, 0], F), (3, 1)))
    # flip x, flip y, a quarter turn, scale 2, translate: (1, 2, 3) -> (1, -2) -> (-1, -2) -> (2, -1) -> (4, -2, 6) -> (14, 18, 36)
    s, cs = ref.sincos(np.array([np.pi / 2], F))
    p = np.array([3, F(np.pi / 2), cs[0], s[0], 2, 10, 20, 30], F)
    row = np.array([[1, 2, 3, 4, 5, 6, 0.25, 1, 0, 9]], F)
    out = ref.xform_boxes(row, p, vel=True)
    np.testing.assert_allclose(out[0, :3], [14, 18, 36], atol=1e-5)
    np.testing.assert_array_equal(out[0, 3:6], [8, 10, 12])
    assert out[0, 6] == (-(-F(0.25) + ref.PI_F)) + F(np.pi / 2)
    np.testing.assert_allclose(out[0, 7:9], [0, -2], atol=1e-6)      # (1, 0) -> (1, 0) -> (-1, 0) -> (0, -1) -> (0, -2), no translation
    assert out[0, 9] == 9
    np.testing.assert_array_equal(ref.xform_points(row, p)[0, 3:], row[0, 3:])


def test_named_cases_do_what_they_say():
    C = ref.case
    out = ref.expected("all_collide")
    assert not out["keep"].any() and (out["db_index"] >= 0).sum(1).tolist() == [4, 4, 4]
    np.testing.assert_array_equal(out["out_points"], C("all_collide")["points"])
    np.testing.assert_array_equal(out["out_offsets"], C("all_collide")["offsets"])
    assert ref.expected("none_collide")["keep"].all()
    # chain: three mutually chained boxes, the greedy rule keeps the ends (reject-both would keep none of a - b and b - c)
    a, b, c = C("chain")["db"]["boxes"]
    assert box_ref.iou_bev_pair(b, a) > 0 and box_ref.iou_bev_pair(c, b) > 0 and box_ref.iou_bev_pair(c, a) == 0
    assert ref.expected("chain")["keep"].tolist() == [[1, 0, 1]] * 3
    # shared edge: intersection exactly 0, accepted
    cand, gt = C("shared_edge")["db"]["boxes"][0], C("shared_edge")["gt_boxes"][1, 0]
    assert cand[0] + F(0.5) * cand[3] == gt[0] - F(0.5) * gt[3] and box_ref.iou_bev_pair(cand, gt) == 0
    assert box_ref.pair_inter(cand, box_ref._corner_list(cand[None])[0], gt, box_ref._corner_list(gt[None])[0]) == 0
    assert ref.expected("shared_edge")["keep"][:, 0].all()
    # the same entry twice: the second draw is rejected by its twin
    out = ref.expected("twice")
    assert (out["db_index"][:, 0] == out["db_index"][:, 1]).all() and out["keep"].tolist() == [[1, 0, 1, 0]] * 3
    # padding rows on the candidate: neither obstacles nor counted
    c = C("padding_gt")
    assert not ref.valid_gt(c["gt_boxes"][1], c["gt_labels"][1], 2).any() and (c["gt_boxes"][1, :, :2] == c["db"]["boxes"][0, :2]).all()
    assert ref.expected("padding_gt")["keep"].all() and (ref.expected("padding_gt")["db_index"] >= 0).all()
    # quota: class 0 holds its two boxes already, class 1 one of two
    assert ref.expected("quota_met")["db_index"].tolist() == [[-1, -1, 1, -1]] * 3
    # a class without entries
    coff = C("empty_class")["db"]["class_offsets"]
    assert coff[1] == coff[2] and ref.expected("empty_class")["db_index"][:, 1:4].tolist() == [[-1] * 3] * 3
    # faces: on an xy face kept, on a z face removed
    for name, e in (("faces", 0.0), ("extra_width", 0.5)):
        c, out = C(name), ref.expected(name)
        assert c["e"] == e and out["keep"][:, 0].all()
        bx = c["db"]["boxes"][:1]
        head = _scene(c, 2)[:11, :3]
        xy, z = box_ref.face_hits(head, bx, e)
        assert xy >= 2 and z >= 1, "the case has no point on a face"
        ins = box_ref.inside(head, bx, e)[:, 0]
        want = [0, 0, 0, 0, 1, 1, 1, 0, 0, 0, 0] if e == 0 else [1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 1]
        assert ins.astype(int).tolist() == want
    # the general cases: a second chunk of the walk with an accepted slot, padding rows in the middle, all object sizes
    out = ref.expected("q70_c5_d7_g6")
    assert out["keep"][:, 64:].any() and out["keep"][:, :64].any() and (out["db_index"][:, 64:] >= 0).any(1).all()
    gl = C("q20_c4_d7_g6")["gt_labels"][0]
    v = ref.valid_gt(C("q20_c4_d7_g6")["gt_boxes"][0], gl, 3)
    assert not v[1] and v[0] and v[2] and not v[4] and gl[1] == 1 and gl[4] == -1, "no padding row in the middle (one of them with a class label)"
    assert sorted(set(np.diff(C("q20_c4_d7_g6")["db"]["offsets"]).tolist())) == [0, 1, 64, 130]
    sizes = {n: np.diff(C(n)["offsets"]).tolist() for n in ref.GENERAL}
    assert {s[1] for s in sizes.values()} == {63, 64, 65} and all(s[0] == 0 and s[2] == 700 for s in sizes.values())


def test_gt_database_host_side(sad):
    from sad_amd import io as sio
    from sad_amd.augment import GTDatabase
    rng = np.random.default_rng(0)
    objs = [(rng.uniform(0, 1, (n, 4)).astype(F), ref.box(i, 0), lab) for i, (n, lab) in enumerate(((5, 2), (300, 0), (0, 2), (64, 0)))]
    db = GTDatabase(objs, num_classes=3, max_obj_points=100)
    assert len(db) == 4 and db.class_offsets == [0, 2, 2, 4] and db.Pmax == 100 and db.db_points is None
    assert db.offsets.tolist() == [0, 100, 164, 169, 169] and db.labels.tolist() == [0, 0, 2, 2]
    np.testing.assert_array_equal(db.points[:100], objs[1][0][sio.select_rows(300, 100, 0, 0)])
    np.testing.assert_array_equal(db.points[164:169], objs[0][0])
    np.testing.assert_array_equal(db.boxes[:, 0], [1, 3, 0, 2])
    for bad in (dict(objects=[]), dict(num_classes=17), dict(max_obj_points=0), dict(objects=objs + [(objs[0][0][:, :3], objs[0][1], 0)]),
                dict(objects=objs + [(objs[0][0], objs[0][1], 3)])):
        with pytest.raises(ValueError):
            GTDatabase(**dict(dict(objects=objs, num_classes=3, max_obj_points=100), **bad))


def test_gt_database_from_directory(sad, tmp_path):
    import json
    from sad_amd.augment import GTDatabase
    rng = np.random.default_rng(1)
    objs = [rng.uniform(0, 1, (n, 4)).astype(F) for n in (7, 3)]
    infos = []
    for i, (o, lab) in enumerate(zip(objs, (1, 0))):
        o.tofile(tmp_path / f"obj{i}.bin")
        infos.append(dict(path=f"obj{i}.bin", box=ref.box(i, 1).tolist(), label=lab))
    (tmp_path / "infos.json").write_text(json.dumps(infos))
    for given in ("infos.json", infos):
        db = GTDatabase.from_directory(str(tmp_path), given, num_classes=2, cols=4)
        assert db.class_offsets == [0, 1, 2] and db.offsets.tolist() == [0, 3, 10] and db.Pmax == 7
        np.testing.assert_array_equal(db.points, np.concatenate([objs[1], objs[0]]))
