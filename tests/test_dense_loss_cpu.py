"""CPU checks of the dense head losses (SPEC.md §27): the two forms of tests/dense_loss_ref.py agree, the reference's gradients
are torch.autograd's of the plain composition in float64, every condition the GPU cases of tests/test_gpu_dense_loss.py rely on
holds on the reference, and the C entry points refuse what §27 says they refuse before anything is launched."""
import ctypes

import numpy as np
import pytest

import dense_loss_ref as ref

F = np.float32
D = np.float64


def _bits(a, b, what):
    assert a.shape == b.shape and a.dtype == b.dtype, what
    bad = ~((a == b) | (np.isnan(a) & np.isnan(b)))
    assert not bad.any(), f"{what}: {int(bad.sum())} of {a.size} differ under =="


def _rel(a, b, what, tol=1e-6):
    err = np.abs(a.astype(D) - b.astype(D))
    ok = err <= tol * np.maximum(np.abs(a), np.abs(b))
    assert ok.all(), f"{what}: {int((~ok).sum())} beyond {tol} relative, worst {float(err.max()):.3g}"


@pytest.mark.parametrize("name", ref.ANCHOR_CASES)
def test_anchor_forms_agree(orc, name):
    c = ref.case(name)
    loop, vec = ref.loss(c, "loop"), ref.expected(name)["f32"]
    assert np.array_equal(loop["num_pos"], vec["num_pos"])
    _bits(loop["per_anchor"][..., 1], vec["per_anchor"][..., 1], f"{name} regression terms")
    _bits(loop["grad_reg"], vec["grad_reg"], f"{name} grad_reg")
    for i in (0, 2):
        _rel(loop["per_anchor"][..., i], vec["per_anchor"][..., i], f"{name} per_anchor[..., {i}]")
    _rel(loop["grad_cls"], vec["grad_cls"], f"{name} grad_cls")
    if c["nb"]:
        _rel(loop["grad_dir"], vec["grad_dir"], f"{name} grad_dir")


@pytest.mark.parametrize("name", ref.CENTER_CASES)
def test_center_forms_agree(name):
    loop, vec = ref.loss(ref.case(name), "loop"), ref.expected(name)["f32"]
    assert np.array_equal(loop["num_pos"], vec["num_pos"])
    for k in loop:
        if k.startswith("grad_") and k != "grad_hm" or k == "terms_reg":
            _bits(loop[k], vec[k], f"{name} {k}")
    _rel(loop["terms_hm"], vec["terms_hm"], f"{name} heat map terms")
    _rel(loop["grad_hm"], vec["grad_hm"], f"{name} grad_hm")


# ---- torch.autograd of the plain composition, float64 -----------------------------------------------------------------------------
def _torch_anchor(c):
    """OpenPCDet's composition: permuted copies, a one-hot tensor, the elementwise chain; loss [B,3], autograd for the gradients."""
    import torch
    kw, A, nb = c["kw"], c["A"], c["nb"]
    t64 = lambda a: torch.from_numpy(np.array(a, D))  # noqa: E731
    maps = {n: t64(c[n]).requires_grad_() for n in ("cls", "reg", "dir") if c[n] is not None}
    B, _, H, W = c["reg"].shape
    rows = lambda m: m.view(B, A, -1, H, W).permute(0, 3, 4, 1, 2).reshape(B, H * W * A, -1)  # noqa: E731
    labels = torch.from_numpy(np.array(c["labels"])).long()
    pos, live = labels >= 0, labels != -2
    n = pos.sum(1).clamp(min=1).to(torch.float64)
    scale = [float(F(s)) for s in kw["scale"]]
    alpha, beta = float(F(kw["alpha"])), float(F(kw["beta"]))
    x = rows(maps["cls"])
    C = x.shape[-1]
    onehot = (labels[..., None] == torch.arange(C)).to(torch.float64)
    p = torch.sigmoid(x)
    pt = onehot * (1 - p) + (1 - onehot) * p
    # max(x, 0) - x t + log1p(exp(-|x|)) as one torch function: the same values, and its derivative sigmoid(x) - t also AT x == 0,
    # where autograd of the clamp / abs spelling picks the subgradient 1 - t (the cases plant logits at 0 and -0.0)
    bce = torch.nn.functional.binary_cross_entropy_with_logits(x, onehot, reduction="none")
    lcls = ((onehot * alpha + (1 - onehot) * (1 - alpha)) * pt * pt * bce * live[..., None]).sum((1, 2)) * scale[0] / n
    r, tg = rows(maps["reg"]), torch.nan_to_num(t64(c["reg_target"]), posinf=0.0)
    cw = t64(np.asarray(kw["code_weights"], F))
    d = r - tg
    if kw["sin_diff"]:
        d = torch.cat([d[..., :6], (torch.sin(r[..., 6]) * torch.cos(tg[..., 6]) - torch.cos(r[..., 6]) * torch.sin(tg[..., 6]))[..., None]], -1)
    a = (d * cw).abs()
    lreg = (torch.where(a < beta, 0.5 * a * a / beta, a - 0.5 * beta) * pos[..., None]).sum((1, 2)) * scale[1] / n
    ldir = torch.zeros(B, dtype=torch.float64)
    if nb:
        dt = torch.from_numpy(np.array(c["dir_target"])).long()
        on = pos & (dt >= 0) & (dt < nb)
        ce = -torch.log_softmax(rows(maps["dir"]), -1).gather(-1, dt.clamp(0, nb - 1)[..., None])[..., 0]
        ldir = (ce * on).sum(1) * scale[2] / n
    loss = torch.stack([lcls, lreg, ldir], 1)
    loss.sum().backward()
    return loss.detach().numpy(), {"grad_" + k: v.grad.numpy() for k, v in maps.items()}


def _torch_center(c):
    import torch
    kw = c["kw"]
    t64 = lambda a: torch.from_numpy(np.array(a, D))  # noqa: E731
    names = ["hm"] + [n for n in ref.CENTER_MAPS if c[n] is not None]
    maps = {n: t64(c[n]).requires_grad_() for n in names}
    B, C, H, W = c["hm"].shape
    t = t64(c["heatmap"])
    one = t == 1
    scale = [float(F(s)) for s in kw["scale"]]
    p = torch.sigmoid(maps["hm"]).clamp(float(ref.LO), float(ref.HI))
    lpos = -torch.log(p) * (1 - p) ** 2 * one
    lneg = -torch.log(1 - p) * p ** 2 * (1 - t) ** 4 * (~one)
    lhm = (lpos + lneg).sum((1, 2, 3)) * scale[0] / (one.sum((1, 2, 3)).clamp(min=1) if kw["normalize"] else 1)
    ind = torch.from_numpy(np.array(c["ind"])).long()
    assigned = (ind >= 0) & (ind < H * W)
    cat = torch.cat([maps[n].view(B, -1, H * W) for n in names[1:]], 1)                       # [B,na,HW]
    na = cat.shape[1]
    pred = cat.gather(2, ind.clamp(0, H * W - 1)[:, None, :].expand(-1, na, -1)).transpose(1, 2)   # [B,G,na]
    l1 = (pred - t64(c["anno"])).abs() * t64(np.asarray(kw["code_weights"], F)) * assigned[..., None]
    lreg = l1.sum((1, 2)) * scale[1] / (assigned.sum(1).clamp(min=1) if kw["normalize"] else 1)
    loss = torch.stack([lhm, lreg], 1)
    loss.sum().backward()
    return loss.detach().numpy(), {"grad_" + k: v.grad.numpy() for k, v in maps.items()}


def _close(a, b, what):
    err = np.abs(a - b)
    assert (err <= 1e-9 * (1 + np.abs(b))).all(), f"{what}: worst {float(err.max()):.3g}"


@pytest.mark.parametrize("name", ref.ANCHOR_CASES + ref.CENTER_CASES)
def test_reference_gradients_are_autograds(name):
    c = ref.case(name)
    want = ref.expected(name)["f64"]
    loss, grads = (_torch_anchor if name in ref.ANCHOR_SHAPES else _torch_center)(c)
    _close(want["loss64"], loss, f"{name} loss")
    for k, g in grads.items():
        _close(want[k], g, f"{name} {k}")


# ---- coverage the GPU cases rely on ------------------------------------------------------------------------------------------------
def test_shapes_of_the_cases():
    """Every value of the issue's shape table occurs: H x W, A, C, nb, G; B = 3 everywhere."""
    hw = {s[:2] for s in ref.ANCHOR_SHAPES.values()}
    assert {(1, 1), (5, 7), (3, 67), (9, 130)} <= hw and hw == {s[:2] for s in ref.CENTER_SHAPES.values()}
    assert {1, 6, 9, 11, 128} <= {s[2] for s in ref.ANCHOR_SHAPES.values()}      # (9, 11: a full anchor chunk and a partial one)
    assert {1, 3, 64} <= {s[3] for s in ref.ANCHOR_SHAPES.values()} and {1, 3, 64} <= {s[2] for s in ref.CENTER_SHAPES.values()}
    assert {0, 2, 4} <= {s[4] for s in ref.ANCHOR_SHAPES.values()}
    assert {0, 1, 3, 65, 1024} <= {s[3] for s in ref.CENTER_SHAPES.values()}
    for n in ref.ANCHOR_CASES:
        assert ref.case(n)["labels"].shape[0] == 3
    for n in ref.CENTER_CASES:
        assert ref.case(n)["hm"].shape[0] == 3
    # 9 x 130: several workgroups per scene in both heads (tiles of 64 cells / of 256 cells)
    assert 9 * 130 > 4 * 256


@pytest.mark.parametrize("name", [n for n in ref.ANCHOR_CASES if n != "l:exact"])
def test_anchor_scenes_differ(name):
    lab = ref.case(name)["labels"]
    assert (lab[0] < 0).all() and (lab[0] == -1).any()                 # no positive: n = max(0, 1)
    assert (lab[1] == -2).all()                                        # all ignored
    assert (lab[2] >= 0).any()
    if lab.shape[1] >= 8:
        assert {-2, -1} <= set(lab[2].tolist()) and (lab[0] == -2).any()    # rows of all three kinds
        assert (lab[2] >= ref.rows_of(ref.case(name)["cls"], ref.case(name)["A"]).shape[-1]).any()    # a label >= C: no hot class
    want = ref.expected(name)["f32"]
    assert want["num_pos"][0] == 0 and want["num_pos"][1] == 0 and want["num_pos"][2] > 0
    assert (want["per_anchor"][1] == 0).all() and (want["grad_cls"][1] == 0).all()


@pytest.mark.parametrize("name", ref.ANCHOR_CASES)
def test_unnormalised_outputs_stand_clear_of_the_tolerance(name):
    """The GPU test holds the library-function outputs to 1e-4 + 1e-4 |ref|.  That rule only bites where |ref| is well above 1e-4,
    so every anchor case is also run with normalize=False, and here the reference of that run is shown to be of natural size:
    the median of the non-zero entries at least 100 x the absolute tolerance, three quarters of them at least 10 x."""
    c = ref.case(name)
    w64 = ref.expected(name, normalize=False)["f64"]
    hot = c["labels"][..., None] == np.arange(ref.rows_of(c["cls"], c["A"]).shape[-1])
    gcls = ref.rows_of(w64["grad_cls"], c["A"])
    groups = {"grad_cls": gcls, "grad_cls on the hot class": gcls[hot], "classification terms": w64["per_anchor"][..., 0]}
    if c["nb"]:
        groups["grad_dir"], groups["direction terms"] = w64["grad_dir"], w64["per_anchor"][..., 2]
    for what, v in groups.items():
        v = np.abs(v[v != 0])
        assert v.size > 0, (name, what)
        assert np.median(v) >= 1e-2 and np.mean(v >= 1e-3) >= 0.75, (name, what, float(np.median(v)), float(np.mean(v >= 1e-3)))
    # forms agree on this run too (the float32 reference the == comparisons of the GPU test use)
    w32 = ref.expected(name, normalize=False)["f32"]
    assert np.array_equal(w32["num_pos"], ref.expected(name)["f32"]["num_pos"])
    assert np.isfinite(w32["per_anchor"]).all() and np.isfinite(w32["grad_reg"]).all()


def test_finish_wraps_and_class_chunks_have_tails():
    """Cases the kernels' loops need: more than 64 workgroups per scene (the wave that adds the partial sums takes a second
    round), anchor classes 8 + tail, centre classes 16 + tail."""
    H, W, A, C, nb = ref.ANCHOR_SHAPES["l:9x130:a32"]
    assert -(-H * W // 64) * -(-A // 8) > 64
    assert any(C > 8 and C % 8 for _, _, _, C, _ in ref.ANCHOR_SHAPES.values())
    assert any(C > 16 and C % 16 for _, _, C, _, _ in ref.CENTER_SHAPES.values())


def test_anchor_edge_coverage():
    c = ref.case("l:edges")
    A, nb = c["A"], c["nb"]
    lab = c["labels"]
    x = ref.rows_of(c["cls"], A)
    live = lab != -2
    xs = x[live]
    assert (xs == 0).any() and (np.signbit(xs) & (xs == 0)).any() and (xs == 100).any() and (xs == -100).any()
    assert ((np.abs(xs) > 0.1) & (np.abs(xs) < 10)).any()
    # +-100 on a hot class and on a cold one: e underflows to nothing against 1, p == 1
    hot = lab[..., None] == np.arange(x.shape[-1])
    for v in (100.0, -100.0):
        assert ((x == v) & hot).any() and ((x == v) & ~hot & live[..., None]).any()
    assert F(1) / (F(1) + np.exp(F(-100))) == F(1)
    pos = lab >= 0
    d = ((ref.rows_of(c["reg"], A) - np.where(pos[..., None], c["reg_target"], 0)) * np.asarray(c["kw"]["code_weights"], F))[pos][:, :6]
    beta = F(c["kw"]["beta"])
    a = np.abs(d)
    assert (a == beta).any() and (a == np.nextafter(beta, F(0))).any() and (a > beta).any() and (d == 0).any()
    assert ((d == beta).any() and (d == -beta).any())
    yaw = ref.rows_of(c["reg"], A)[..., 6][pos]
    assert (yaw > 990).any() and (yaw < -990).any() and (np.abs(yaw) < 1e4).all()
    dt = c["dir_target"][pos]
    assert (dt == nb).any() and (dt == -1).any() and ((dt >= 0) & (dt < nb)).any()
    # garbage in reg_target of non-positive rows never reaches a result
    assert np.isinf(c["reg_target"][~pos]).any()
    want = ref.expected("l:edges")["f32"]
    assert np.isfinite(want["per_anchor"]).all() and np.isfinite(want["grad_reg"]).all()
    assert (want["per_anchor"][..., 1][~pos] == 0).all()


def test_exactly_summable_case():
    """l:exact: every regression term and every partial sum, in any order, is a binary32 number."""
    c = ref.case("l:exact")
    kw = c["kw"]
    assert kw["beta"] == 0.125 and not kw["sin_diff"] and set(kw["code_weights"]) == {1.0} and kw["scale"][1] == 1.0
    pos = c["labels"] >= 0
    assert pos.sum(1).tolist() == [8, 16, 8]
    d = (ref.rows_of(c["reg"], c["A"]).astype(D) - c["reg_target"])[pos]
    assert (d * 16 == np.round(d * 16)).all() and (np.abs(d) <= 4).all() and (d == 0).any() and (np.abs(d) == 2.0 ** -4).any()
    want, w64 = ref.expected("l:exact")["f32"], ref.expected("l:exact")["f64"]
    assert np.array_equal(want["per_anchor"][..., 1].astype(D), w64["per_anchor"][..., 1])       # the terms are exact
    rng = np.random.default_rng(5)
    for b in range(3):
        # the single terms of the scene, not only the row sums
        r = ref.rows_of(c["reg"], c["A"])[b][pos[b]].astype(D) - c["reg_target"][b][pos[b]]
        a = np.abs(r)
        terms = (np.where(a < 0.125, 0.5 * a * a / 0.125, a - 0.0625) / pos[b].sum()).reshape(-1)
        assert np.array_equal(terms.astype(F).astype(D), terms)
        for _ in range(8):
            acc = F(0)
            for v in rng.permutation(terms):
                acc = F(acc + F(v))
                assert D(acc) >= 0
            assert D(acc) == terms.sum() == want["loss64"][b, 1]
            part = np.cumsum(rng.permutation(terms))
            assert np.array_equal(part.astype(F).astype(D), part)
    assert np.array_equal(want["loss"][:, 1].astype(D), want["loss64"][:, 1])


@pytest.mark.parametrize("name", ref.CENTER_CASES)
def test_center_coverage_and_bound(name):
    c = ref.case(name)
    t, ind = c["heatmap"], c["ind"]
    B, C, H, W = t.shape
    want = ref.expected(name)
    npos = want["f32"]["num_pos"]
    assert npos[0, 0] == 0 and npos[0, 1] == 0 and (npos[1:, 0] > 0).all()                # scene 0: both normalisers max(0, 1)
    if C * H * W >= 8:
        assert ((t > 0) & (t < 1)).any() and (t == 0).any() and (t[2] == 1).any()
        e = np.exp(-np.abs(c["hm"][2]))
        ps = np.where(c["hm"][2] >= 0, 1 / (1 + e), e / (1 + e))
        assert (ps < ref.LO).any() and (ps > ref.HI).any()                                # clamped on both sides
        assert ((ps < ref.LO) & (t[2] == 1)).any() and ((ps > ref.HI) & (t[2] != 1)).any()
        assert (want["f32"]["grad_hm"][2][(ps < ref.LO) | (ps > ref.HI)] == 0).all()
    if ind.shape[1] >= 3:
        assert (ind == -1).any() and (ind >= H * W).any() and ((ind >= 0) & (ind < H * W)).any()
    if ind.shape[1] == 1024:
        assert len(np.unique(ind[1])) < 1024                                              # shared cells occur by themselves
    # the bound of the GPU test on loss[:, 0] is narrower than one missing positive cell
    th = want["f64"]["terms_hm"].reshape(B, -1)
    for b in range(B):
        one = t[b].reshape(-1) == 1
        if one.any():
            assert th[b][one].min() > hm_bound(th[b]), (name, b, th[b][one].min(), hm_bound(th[b]))


def hm_bound(terms):
    """Sum_k (1e-4 + 1e-4 |term_k|) + n 2^-23 Sum |terms|: the library-function tolerance of every term plus §21.4's rule."""
    return float((1e-4 + 1e-4 * np.abs(terms)).sum() + terms.size * 2.0 ** -23 * np.abs(terms).sum())


def test_shared_cells_order_shows():
    """c:shared: the gradient at a cell several boxes share depends on the order of the additions; ascending g is specified.
    (The gradients of one map element all have the magnitude cw_j * wq_1, so three boxes cannot show an order: every partial sum
    of up to three equal magnitudes is exact or is rounded last.  Four boxes with signs + + + - do: 3m rounds, then - m.)"""
    c = ref.case("c:shared")
    ind = c["ind"]
    assert (ind[1] == 9).sum() == 4 and (ind[2] == 20).sum() == 3 and (ind[2] == 5).sum() == 2
    asc = ref.loss(c)["grad_reg"]
    desc = ref.center_loss_vec(c, F, order=range(ind.shape[1] - 1, -1, -1))["grad_reg"]
    m = ref.SHARED_CW
    want = F(F(F(m + m) + m) - m)
    assert asc[1, 0].reshape(-1)[9] == want and desc[1, 0].reshape(-1)[9] == F(F(F(-m + m) + m) + m)
    assert asc[1, 0].reshape(-1)[9] != desc[1, 0].reshape(-1)[9]
    assert asc[2, 0].reshape(-1)[20] == m and asc[2, 1].reshape(-1)[20] == F(m + m)       # + - +, and + + 0
    assert asc[1, 0].reshape(-1)[3] == m                                                  # a cell of its own


# ---- the C ABI refuses before any launch ------------------------------------------------------------------------------------------
def _anchor_args(_lib, **over):
    a = _lib.AnchorHeadLossArgs()
    a.struct_size = ctypes.sizeof(_lib.AnchorHeadLossArgs)
    for f in ("cls", "reg", "dir", "labels", "reg_target", "dir_target", "loss", "num_pos", "grad_cls", "grad_reg", "grad_dir", "workspace"):
        setattr(a, f, 0x10000)                                         # never dereferenced: every call below fails on the host
    a.B, a.H, a.W, a.A, a.C, a.nb, a.layout, a.sin_diff, a.normalize = 2, 4, 4, 6, 3, 2, 0, 1, 1
    a.alpha, a.beta = 0.25, 1.0 / 9.0
    for k, v in over.items():
        setattr(a, k, v)
    return a


def _center_args(_lib, **over):
    a = _lib.CenterHeadLossArgs()
    a.struct_size = ctypes.sizeof(_lib.CenterHeadLossArgs)
    for f in ("hm", "reg", "height", "dim", "rot", "heatmap", "ind", "anno", "loss", "num_pos", "grad_hm", "grad_reg", "grad_height",
              "grad_dim", "grad_rot", "workspace"):
        setattr(a, f, 0x10000)
    a.B, a.H, a.W, a.C, a.G, a.layout, a.normalize = 2, 4, 4, 3, 5, 0, 1
    for k, v in over.items():
        setattr(a, k, v)
    return a


def test_c_abi_refusals(sad):
    from sad_amd import _lib
    L = _lib.lib()
    EINVAL, EUNSUPPORTED = -1, -2
    fa, fc = L.sad_anchor_head_loss_f32, L.sad_center_head_loss_f32
    assert fa(None, None) == EINVAL and fc(None, None) == EINVAL
    for over, code, needle in (
            (dict(struct_size=8), EINVAL, b"struct_size"), (dict(cls=None), EINVAL, b"NULL"), (dict(labels=None), EINVAL, b"NULL"),
            (dict(grad_reg=None), EINVAL, b"NULL"), (dict(workspace=None), EINVAL, b"NULL"), (dict(loss=None), EINVAL, b"NULL"),
            (dict(beta=0.0), EINVAL, b"beta"), (dict(beta=-1.0), EINVAL, b"beta"), (dict(alpha=-0.1), EINVAL, b"alpha"),
            (dict(alpha=1.5), EINVAL, b"alpha"), (dict(layout=2), EINVAL, b"layout"), (dict(dir=None), EINVAL, b"together"),
            (dict(nb=0), EINVAL, b"together"), (dict(dir_target=None), EINVAL, b"together"), (dict(grad_dir=None), EINVAL, b"together"),
            (dict(nb=1), EINVAL, b"nb"), (dict(B=0), EINVAL, b">= 1"), (dict(C=0), EINVAL, b">= 1"),
            (dict(B=65536), EUNSUPPORTED, b"65535"), (dict(C=65), EUNSUPPORTED, b"65"), (dict(A=129), EUNSUPPORTED, b"129"),
            (dict(nb=9), EUNSUPPORTED, b"nb = 9"), (dict(B=4, H=16384, W=16384, A=2), EUNSUPPORTED, b"2^31")):
        assert fa(ctypes.byref(_anchor_args(_lib, **over)), None) == code, over
        assert needle in L.sad_last_error(), (over, L.sad_last_error())
    for over, code, needle in (
            (dict(struct_size=8), EINVAL, b"struct_size"), (dict(hm=None), EINVAL, b"NULL"), (dict(heatmap=None), EINVAL, b"NULL"),
            (dict(grad_rot=None), EINVAL, b"NULL"), (dict(workspace=None), EINVAL, b"NULL"), (dict(ind=None), EINVAL, b"ind"),
            (dict(vel=0x10000), EINVAL, b"vel"), (dict(grad_vel=0x10000), EINVAL, b"vel"), (dict(layout=-1), EINVAL, b"layout"),
            (dict(H=0), EINVAL, b">= 1"), (dict(G=-1), EINVAL, b"G >= 0"),
            (dict(B=65536), EUNSUPPORTED, b"65535"), (dict(C=65), EUNSUPPORTED, b"65"), (dict(G=1025), EUNSUPPORTED, b"1025"),
            (dict(B=2, H=32768, W=32768), EUNSUPPORTED, b"2^31")):
        assert fc(ctypes.byref(_center_args(_lib, **over)), None) == code, over
        assert needle in L.sad_last_error(), (over, L.sad_last_error())
    # the workspace laws, and 0 outside the limits
    assert L.sad_anchor_head_loss_workspace_bytes(3, 9, 130, 6) == 3 * 19 * 1 * 12
    assert L.sad_anchor_head_loss_workspace_bytes(2, 5, 7, 128) == 2 * 1 * 16 * 12
    assert L.sad_anchor_head_loss_workspace_bytes(1, 5, 7, 129) == 0 and L.sad_anchor_head_loss_workspace_bytes(0, 5, 7, 1) == 0
    assert L.sad_center_head_loss_workspace_bytes(3, 9, 130, 1024) == 3 * (5 + 4) * 4
    assert L.sad_center_head_loss_workspace_bytes(3, 1, 1, 0) == 3 * 4
    assert L.sad_center_head_loss_workspace_bytes(3, 9, 130, 1025) == 0


def test_ops_refuse_cpu_tensors_and_bad_shapes(sad):
    import torch
    from sad_amd import dense_head, ops
    assert sad.anchor_head_loss is ops.anchor_head_loss and sad.center_head_loss is ops.center_head_loss
    assert sad.AnchorHeadLoss is dense_head.AnchorHeadLoss and sad.CenterHeadLoss is dense_head.CenterHeadLoss
    cls, reg = torch.zeros(1, 6, 2, 2), torch.zeros(1, 14, 2, 2)
    lab, tgt = torch.zeros(1, 8, dtype=torch.int32), torch.zeros(1, 8, 7)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.anchor_head_loss(cls, reg, None, lab, tgt)
    with pytest.raises(ValueError, match="A \\* 7"):
        ops.anchor_head_loss(cls, torch.zeros(1, 13, 2, 2), None, lab, tgt)
    with pytest.raises(ValueError, match="beta"):
        ops.anchor_head_loss(cls, reg, None, lab, tgt, beta=0.0)
    with pytest.raises(ValueError, match="together"):
        ops.anchor_head_loss(cls, reg, torch.zeros(1, 4, 2, 2), lab, tgt)
    with pytest.raises(TypeError, match="cls: expected dtype torch.float32"):
        ops.anchor_head_loss(cls.double(), reg, None, lab, tgt)
    with pytest.raises(TypeError, match="reg: expected a torch.Tensor"):
        ops.anchor_head_loss(cls, None, None, lab, tgt)
    with pytest.raises(ValueError, match="reg: expected shape"):
        ops.anchor_head_loss(cls, torch.zeros(1, 14, 2, 3), None, lab, tgt)
    with pytest.raises(ValueError, match="cls: must be contiguous"):
        ops.anchor_head_loss(torch.zeros(1, 2, 2, 6).permute(0, 3, 1, 2), reg, None, lab, tgt)
    with pytest.raises(ValueError, match="cls: 5 channels are not a multiple of A = 2"):
        ops.anchor_head_loss(torch.zeros(1, 5, 2, 2), reg, None, lab, tgt)
    with pytest.raises(ValueError, match="dir: 2 channels are not A \\* nb"):
        ops.anchor_head_loss(cls, reg, torch.zeros(1, 2, 2, 2), lab, tgt, lab)
    with pytest.raises(ValueError, match="dir: 18 channels are not A \\* nb with 2 <= nb <= 8"):
        ops.anchor_head_loss(cls, reg, torch.zeros(1, 18, 2, 2), lab, tgt, lab)
    with pytest.raises(ValueError, match="reg: at most 128 anchors"):         # the limits come before dtypes
        ops.anchor_head_loss(torch.zeros(1, 129, 1, 1).half(), torch.zeros(1, 129 * 7, 1, 1), None, lab, tgt)
    with pytest.raises(ValueError, match="cls: at most 64 classes"):
        ops.anchor_head_loss(torch.zeros(1, 130, 2, 2).half(), reg, None, lab, tgt)
    hm = torch.zeros(1, 3, 2, 2)
    m = [torch.zeros(1, ch, 2, 2) for ch in (2, 1, 3, 2)]
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.center_head_loss(hm, *m, None, hm, torch.zeros(1, 2, dtype=torch.int32), torch.zeros(1, 2, 8))
    ind, anno = torch.zeros(1, 2, dtype=torch.int32), torch.zeros(1, 2, 8)
    with pytest.raises(ValueError, match="dim: expected 3 channels, got 2"):
        ops.center_head_loss(hm, m[0], m[1], m[0], m[3], None, hm, ind, anno)
    with pytest.raises(TypeError, match="height: expected dtype torch.float32"):
        ops.center_head_loss(hm, m[0], m[1].half(), m[2], m[3], None, hm, ind, anno)
    with pytest.raises(ValueError, match="rot: must be contiguous"):
        ops.center_head_loss(hm, m[0], m[1], m[2], torch.zeros(1, 2, 2, 2).permute(0, 3, 1, 2), None, hm, ind, anno)
    with pytest.raises(ValueError, match="vel: expected shape"):
        ops.center_head_loss(hm, *m, torch.zeros(2, 2, 2, 2), hm, ind, anno)
    with pytest.raises(ValueError, match="hm: expected 1 .. 64 class channels, got 65"):
        ops.center_head_loss(torch.zeros(1, 65, 2, 2), m[0].half(), *m[1:], None, hm, ind, anno)
    loss = dense_head.AnchorHeadDecoder([[1, 1, 1]], [0], [0], (0, 0), (1, 1), layout="nhwc").loss(beta=0.2)
    assert isinstance(loss, dense_head.AnchorHeadLoss) and loss.cfg["layout"] == "nhwc" and loss.cfg["beta"] == 0.2
    closs = dense_head.CenterHeadDecoder((0, 0), (1, 1)).loss(scale=(1.0, 0.25))
    assert isinstance(closs, dense_head.CenterHeadLoss) and closs.cfg["scale"] == (1.0, 0.25)
