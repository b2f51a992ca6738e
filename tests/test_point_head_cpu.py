"""CPU checks of the point head reference (tests/point_head_ref.py, SPEC.md §31): that the named cases hold what
tests/test_gpu_point_head.py relies on, that the reference gradient is the derivative of the reference loss, and that
size_target inverts §8 step 3.  No GPU, no library call."""
import numpy as np
import pytest

import box_ref
import point_head_ref as ref

F = np.float32
D = np.float64
EPS = 2.0 ** -24                   # the unit roundoff of binary32


@pytest.mark.parametrize("name", ref.RICH)
def test_rich_cases_cover_the_assignment(name):
    """Every scene of a rich case: a positive of every class, an ignored and a background point, a point inside two boxes (the
    lower index wins), a point exactly on an xy face (excluded) and one exactly on a z face (included), a point in the band only,
    a padding row in the middle of the list that would otherwise win, a candidate shifted out of its box (centerness 0)."""
    c, t = ref.case(name), ref.expected_targets(name)
    C = c["C"]
    B, M = t["labels"].shape
    for b in range(B):
        lab, gl, gt = t["labels"][b], c["gt_labels"][b], c["gt_boxes"][b]
        assert set(range(C)) <= set(lab.tolist()) and (lab == -2).any() and (lab == -1).any()
        valid = (gl >= 0) & (gl < C) & (gt[:, 3:6] > 0).all(1)
        G = len(gl)
        mid = [g for g in range(1, G - 1) if not valid[g] and valid[:g].any() and valid[g + 1:].any()]
        assert mid, "no padding row in the middle of the list"
        ins = box_ref.inside(c["xyz"][b], np.ascontiguousarray(gt[:, :7]), 0.0)                 # [M,G], padding rows included
        two = (ins & valid).sum(1) >= 2
        assert two.any() and (t["match"][b][two] == np.argmax(ins & valid, 1)[two]).all()
        # a padding row that contains a point and has a lower index than the point's match: dropped, not matched
        shadow = ins[:, ~valid].any(1) & (lab >= 0)
        assert shadow.any() and valid[t["match"][b][shadow]].all()
        assert any((ins[m, :g] & ~valid[:g]).any() for m in np.flatnonzero(shadow) for g in [t["match"][b, m]])
        xy, z = box_ref.face_hits(c["xyz"][b], np.ascontiguousarray(gt[:1, :7]), 0.0)
        assert xy >= 1 and z >= 1
        assert lab[0] == -2 and lab[1] == gl[0] and t["match"][b, 1] == 0                        # on the xy face / on the z face of box 0
        band = box_ref.inside(c["xyz"][b], np.ascontiguousarray(gt[valid, :7]), c["tkw"]["extra_width"]).any(1)
        assert lab[2] == -2 and band[2] and not ins[2].any()                                      # the band only
        assert (lab[band & ~(ins & valid).any(1)] == -2).all() and (lab[~band] == -1).all()
        out = (lab >= 0) & (t["centerness64"][b] == 0)
        assert out.any() and (t["centerness"][b][out] == 0).all()
        assert lab[5] >= 0 and t["centerness"][b, 5] == 0                                          # the shifted candidate
        pos = lab >= 0
        assert (t["centerness"][b][~pos] == 0).all() and (t["match"][b][~pos] == -1).all()
        assert ((t["centerness"][b][pos] >= 0) & (t["centerness"][b][pos] <= 1)).all() and (t["centerness"][b][pos] > 0.3).any()


@pytest.mark.parametrize("name", ref.CASES)
def test_margins(name):
    """What makes == and the 1e-4 rule safe: no smooth-L1 argument of a positive row within MARGIN of the kink beta (binary64 and
    float32 on the same side), and every positive's candidate either at least RATIO_MARGIN inside its box on every axis or with
    a centre-ness of exactly 0 in both precisions (cbrt has an infinite slope at 0)."""
    c, t = ref.case(name), ref.expected_targets(name)
    beta = float(F(ref.KW["beta"]))
    for cls_loss in ("bce", "focal"):
        e = ref.expected(name, True, cls_loss)
        with np.errstate(all="ignore"):
            r64, r32 = e["f64"]["resid"], e["f32"]["resid"]
            assert not (np.abs(r64 - beta) < ref.MARGIN).any()
            assert ((r64 < beta) == (r32 < beta))[~np.isnan(r64)].all()
    pos = t["labels"] >= 0
    inside = np.nan_to_num(t["ratios64"], nan=1.0).min(-1) >= ref.RATIO_MARGIN
    zero = (t["centerness64"] == 0) & (t["centerness"] == 0)
    assert (inside | zero)[pos].all()
    if pos.sum() > 10:
        r = e["f64"]["resid"][pos]
        assert (r[:, :7] < beta).any() and (r[:, :7] > beta).any()                               # both branches of the smooth-L1


def test_edge_cases_hold_what_their_shape_allows():
    assert ref.expected_targets("m1")["labels"].tolist() == [[0]]
    g0 = ref.expected_targets("g0")
    assert (g0["labels"] == -1).all() and (g0["match"] == -1).all() and not g0["reg_target"].any()
    n = ref.expected("no_pos")["f32"]
    assert n["num_pos"][1] == 0 and n["num_pos"][0] > 0 and not n["grad_o"][1, :, 3:].any() and not n["grad_c"][1].any()
    assert np.isfinite(n["loss64"]).all() and n["loss64"][1, 0] > 0 and not n["loss64"][1, 1:].any()
    assert sorted({ref.SHAPES[k][0] for k in ref.CASES}) == [1, 3] and sorted({ref.SHAPES[k][3] for k in ref.CASES}) == [1, 3]
    assert {ref.SHAPES[k][1] for k in ref.CASES} == {1, 70, 256, 257, 600} and {ref.SHAPES[k][2] for k in ref.CASES} == {0, 1, 5, 300}


@pytest.mark.parametrize("name", ref.RICH)
def test_predictions_sit_below_at_and_above_every_clamp_bound(name):
    """Over the positives of scene 0: for each of the bounds +-2 (o[C+3 .. C+5]), +-shift_max (c[0:3]) and +-1 (c[3:6]) a
    prediction beyond it, one exactly on it and one inside; the reference gradient is 0 beyond the bound and not 0 on it."""
    c = ref.case(name)
    e = ref.expected(name)["f32"]
    C = c["C"]
    pos = c["labels"][0] >= 0
    for x, g, lim in ((c["o"][0][pos][:, C + 3:C + 6], e["grad_o"][0][pos][:, C + 3:C + 6], 2.0), (c["c"][0][pos][:, :3], e["grad_c"][0][pos][:, :3], ref.SHIFT_MAX),
                      (c["c"][0][pos][:, 3:], e["grad_c"][0][pos][:, 3:], 1.0)):
        for sign in (-1.0, 1.0):
            beyond, on, within = sign * x > lim, sign * x == lim, (sign * x < lim) & (sign * x > 0)
            assert beyond.any() and on.any() and within.any(), (lim, sign)
            assert (g[beyond] == 0).all() and (g[on] != 0).all()


def test_reference_gradient_against_central_differences():
    """The binary64 gradient of the reference against central differences of its own binary64 loss, L = sum(loss * up) with a
    non-uniform up [B,4], in both classification modes, on every coordinate of o and c of twelve rows of `m70` (positives,
    ignored and background rows) that is not within two steps of a clamp bound; rows whose smooth-L1 arguments come within two
    steps of the kink are left out.  Steps h = 2^-10 and 2^-11.  Observed, the same in both modes (the yaw's sine dominates): on
    the curved coordinates (class logits, yaw) the worst error is 2.1e-8 at 2^-10 and 5.25e-9 at 2^-11: it falls 4.0x when the
    step halves, as a second-order formula must; on the other coordinates the loss is linear or quadratic in the coordinate and
    only roundoff is left (below 1e-12 at either step).  The tolerances are four times the worst error observed at the smaller
    step, 2.1e-8, on the curved coordinates and 1e-11 on the others."""
    c0 = ref.case("m70")
    up = np.array([[0.5, -2.0, 3.0, 0.25]])
    C = c0["C"]
    beta = float(F(ref.KW["beta"]))
    h1, h2 = 2.0 ** -10, 2.0 ** -11
    for cls_loss in ("bce", "focal"):
        c = ref.variant(c0, cls_loss=cls_loss)
        base = {"o": c["o"].astype(D), "c": c["c"].astype(D)}
        e = ref.loss(dict(c, **base), D)
        grad = {"o": e["grad_o"] * np.concatenate([np.repeat(up[:, :1], C, 1), np.repeat(up[:, 1:2], 7, 1)], 1)[:, None],
                "c": e["grad_c"] * np.repeat(up[:, 2:], 3, 1)[:, None]}
        with np.errstate(all="ignore"):
            calm = ~(np.abs(e["resid"][0] - beta) < 2 * 1.3 * h1).any(-1)
        rows = [m for m in range(c["o"].shape[1]) if calm[m]][:12]
        assert len(rows) == 12 and (c["labels"][0, rows] >= 0).sum() >= 4 and (c["labels"][0, rows] == -2).any() and (c["labels"][0, rows] == -1).any()

        def value(key, m, j, delta):
            x = base[key].copy()
            x[0, m, j] += delta
            return float((ref.loss(dict(c, **dict(base, **{key: x})), D)["loss64"] * up).sum())

        worst = {(k, h): 0.0 for k in ("curved", "flat") for h in (h1, h2)}
        for key, lims in (("o", [None] * (C + 3) + [2.0] * 3 + [None]), ("c", [ref.SHIFT_MAX] * 3 + [1.0] * 3)):
            for m in rows:
                for j, lim in enumerate(lims):
                    if lim is not None and abs(abs(base[key][0, m, j]) - lim) < 2 * h1:
                        continue
                    kind = "curved" if key == "o" and (j < C or j == C + 6) else "flat"
                    for h in (h1, h2):
                        fd = (value(key, m, j, h) - value(key, m, j, -h)) / (2 * h)
                        worst[kind, h] = max(worst[kind, h], abs(fd - grad[key][0, m, j]))
        print(cls_loss, {k: f"{v:.3g}" for k, v in worst.items()})
        assert 3.5 <= worst["curved", h1] / worst["curved", h2] <= 4.5
        assert worst["curved", h2] <= 2.1e-8 and worst["flat", h1] <= 1e-11 and worst["flat", h2] <= 1e-11


def test_size_target_inverts_step_3():
    """s -> §8 step 3 -> extents -> §31.1's size_target gives s back within a bound that follows from the roundings, eps = 2^-24,
    u = (1 + s)^2 = 2 q - 1:
      q' = fl(fl(1 + s) + 0.5 fl(s s))          |q' - q| <= q eps (2 + eps)             (1 + s >= 0: every addend is positive)
      qd = fl(fl(anchor q') / anchor)           |qd - q| <= 4.01 q eps                   (the multiplication and the division)
      u' = max(fl(2 qd - 1), 0)                 |u' - u| <= Du = eps (8.1 q + 1.01 u)    (2 qd is exact)
      r  = fl(sqrt(u'))                         |r - (1 + s)| <= A + eps (1 + s + sqrt(Du)),  A = min(Du / (1 + s), sqrt(Du))
      s' = min(fl(r - 1), 1)                    |s' - s| <= 1.01 (A + eps (1 + s + |s|)) + 2 eps sqrt(Du)
    The square root has an infinite slope at u = 0, so near s = -1 the bound is sqrt(Du), about 5e-4, not a few eps; at s = -1
    itself every step is exact.  Checked on 200 000 values of s over [-1, 1], the ends, 0 and values next to -1, for each of the
    three components of §8's anchor."""
    rng = np.random.default_rng(31)
    s = np.concatenate([rng.uniform(-1, 1, 200000), [-1.0, 1.0, 0.0, -0.0], -1 + 2.0 ** -np.arange(1, 24), 1 - 2.0 ** -np.arange(1, 24)]).astype(F)
    s = np.repeat(s[:, None], 3, 1)
    back = ref.size_code(ref.size_decode(s, ref.ANCHOR_CAR), ref.ANCHOR_CAR)
    s64 = s.astype(D)
    q, u = 1 + s64 + 0.5 * s64 * s64, (1 + s64) ** 2
    Du = EPS * (8.1 * q + 1.01 * u)
    with np.errstate(divide="ignore"):
        A = np.minimum(Du / (1 + s64), np.sqrt(Du))
    bound = 1.01 * (A + EPS * (1 + s64 + np.abs(s64))) + 2 * EPS * np.sqrt(Du)
    err = np.abs(back.astype(D) - s64)
    print(f"worst error {err.max():.3g}, worst share of the bound {(err / bound)[bound > 0].max():.3g}")
    assert (err <= bound).all()
    assert (back[s[:, 0] == -1] == -1).all() and (err[np.abs(s64) <= 0.5] <= 16 * EPS).all()
    # the clamps of the target: an extent below half the anchor gives -1, one beyond 2.5 anchors gives 1
    assert ref.size_code(np.asarray(ref.ANCHOR_CAR, F) * F(0.25), ref.ANCHOR_CAR).tolist() == [-1, -1, -1]
    assert ref.size_code(np.asarray(ref.ANCHOR_CAR, F) * F(4), ref.ANCHOR_CAR).tolist() == [1, 1, 1]
