"""numpy reference of the RoI head loss (SPEC.md §29) and the named cases of tests/test_roi_loss_cpu.py and
tests/test_gpu_roi_loss.py.

  loop    one row at a time, every operation a numpy float32 scalar operation in the order §29 writes it; sin / cos from the
          oracle's §13 routine (`oracle.sincos_r`)
  vec     whole arrays; the same function evaluates the formulas in float32 (sin / cos: §13's routine written in numpy,
          dense_loss_ref.sincos_r) and in binary64 (numpy's sin / cos).  Both forms must agree bit for bit in float32.  The
          binary64 evaluation is what the GPU test compares the library-function parts against; with every element of
          grad_corner it returns `mag`, the binary64 sum of the absolute values of the element's eight addends (times the
          same 0.125 and |wq_2|): the scale §9's relative part is applied to, per addend
  torch   the replaced code bases' global-frame composition in binary64 under torch autograd (decode, boxes_to_corners_3d of
          the prediction, the box and the box turned by pi, min of the two norms, Huber with beta = 1), for the CPU test only

The cases take their targets from `roi_head_ref.expected(name)` (§28.1's outputs) and add seeded random predictions.  What a row
with reg_valid == 0 holds in reg_target / gt_local / rois is NaN in every case: it never reaches a result."""
import functools
import zlib

import numpy as np

import dense_loss_ref
import roi_head_ref

F = np.float32
D = np.float64
EPS = F(1e-5)
SX = (1, 1, -1, -1, 1, 1, -1, -1)
SY = (1, -1, -1, 1, 1, -1, -1, 1)
SZ = (-1, -1, -1, -1, 1, 1, 1, 1)
MARGIN = 1e-3
KW = dict(beta=1.0 / 9.0, code_weights=tuple(float(F(v)) for v in (1.0, 1.0, 1.0, 0.7, 0.7, 0.7, 1.3)), scale=(1.0, 2.0, 0.5), normalize=True)


def _seqsum(x):
    """Sum over the last axis, ascending, one rounding per addition, from +0."""
    acc = np.zeros(x.shape[:-1], x.dtype)
    for j in range(x.shape[-1]):
        acc = acc + x[..., j]
    return acc


def _weights(kw, num, dt):
    """[B,3]: scale_i / (float)max(n, 1) with n = (n_cls, n_reg, n_reg), or scale_i."""
    s = np.asarray(kw["scale"], F).astype(dt)[None, :]
    n = np.stack([num[:, 0], num[:, 1], num[:, 1]], 1)
    return s / np.maximum(n, 1).astype(F).astype(dt) if kw["normalize"] else np.broadcast_to(s, n.shape).copy()


# ---- vec: float32 and binary64 ----------------------------------------------------------------------------------------------
def loss_vec(c, dt=F):
    """-> num [B,2], per_roi [B,S,3], grad_cls, grad_reg (, grad_corner, mag), loss64 / loss [B,3], and per corner d0, d1, dist
    [B,S,8] (NaN outside the valid rows)."""
    kw = c["kw"]
    x, r, t, tg = (c[k].astype(dt) for k in ("rcnn_cls", "rcnn_reg", "cls_target", "reg_target"))
    live, valid = c["cls_target"] >= 0, c["reg_valid"] != 0
    B, S = x.shape
    num = np.stack([live.sum(1), valid.sum(1)], 1).astype(np.int32)
    wq = _weights(kw, num, dt)
    wq0, wq1, wq2 = (wq[:, i][:, None] for i in range(3))
    beta, cw = dt(F(kw["beta"])), np.asarray(kw["code_weights"], F).astype(dt)
    half, one, zero = dt(0.5), dt(1), dt(0)
    per = np.zeros((B, S, 3), dt)
    out = {"num": num}
    with np.errstate(all="ignore"):
        e = np.exp(-np.abs(x))
        den = one + e
        p = np.where(x >= 0, one / den, e / den)
        bce = (np.maximum(x, zero) - (x * t)) + np.log1p(e)
        per[..., 0] = np.where(live, bce * wq0, zero)
        out["grad_cls"] = np.where(live, (p - t) * wq0, zero)
        d = (r - tg) * cw
        a = np.abs(d)
        quad = a < beta
        l = np.where(quad, ((half * a) * a) / beta, a - (half * beta))
        sg = np.where(quad, d / beta, np.sign(d))
        per[..., 1] = np.where(valid, _seqsum(l) * wq1, zero)
        out["grad_reg"] = np.where(valid[..., None], (sg * cw) * wq1[..., None], zero)
        if c["rois"] is not None:
            roi, gt = c["rois"].astype(dt), c["gt_local"].astype(dt)
            la, wa, ha = (np.maximum(roi[..., q], dt(EPS)) for q in (3, 4, 5))
            dg = np.sqrt((la * la) + (wa * wa))
            px, py, pz = r[..., 0] * dg, r[..., 1] * dg, r[..., 2] * ha
            pl, pw, ph = np.exp(r[..., 3]) * la, np.exp(r[..., 4]) * wa, np.exp(r[..., 5]) * ha
            if dt is F:
                sp, cp = dense_loss_ref.sincos_r(r[..., 6])
                sgt, cgt = dense_loss_ref.sincos_r(gt[..., 6])
            else:
                sp, cp, sgt, cgt = np.sin(r[..., 6]), np.cos(r[..., 6]), np.sin(gt[..., 6]), np.cos(gt[..., 6])
            hl, hw, hh = half * pl, half * pw, half * ph
            ghl, ghw, ghh = half * gt[..., 3], half * gt[..., 4], half * gt[..., 5]
            total = np.zeros((B, S), dt)
            acc, mag = [np.zeros((B, S), dt) for _ in range(7)], [np.zeros((B, S), dt) for _ in range(7)]
            aux = {k: np.zeros((B, S, 8), dt) for k in ("d0", "d1", "dist")}
            for k in range(8):
                sx, sy, sz = dt(SX[k]), dt(SY[k]), dt(SZ[k])
                ox, oy, oz = sx * hl, sy * hw, sz * hh
                rx, ry = (ox * cp) - (oy * sp), (ox * sp) + (oy * cp)
                X, Y, Z = rx + px, ry + py, oz + pz
                gox, goy, goz = sx * ghl, sy * ghw, sz * ghh
                grx, gry = (gox * cgt) - (goy * sgt), (gox * sgt) + (goy * cgt)
                ex, ey, ez = X - (grx + gt[..., 0]), Y - (gry + gt[..., 1]), Z - (goz + gt[..., 2])
                fx, fy = X - (gt[..., 0] - grx), Y - (gt[..., 1] - gry)
                d0 = np.sqrt(((ex * ex) + (ey * ey)) + (ez * ez))
                d1 = np.sqrt(((fx * fx) + (fy * fy)) + (ez * ez))
                flip = d1 < d0
                dist, ux, uy = np.where(flip, d1, d0), np.where(flip, fx, ex), np.where(flip, fy, ey)
                q = dist < one
                total = total + np.where(q, (half * dist) * dist, dist - half)
                ax, ay, az = np.where(q, ux, ux / dist), np.where(q, uy, uy / dist), np.where(q, ez, ez / dist)
                add = (ax * dg, ay * dg, az * ha, ((ax * cp) + (ay * sp)) * ox, ((ay * cp) - (ax * sp)) * oy, az * oz, (ay * rx) - (ax * ry))
                for j in range(7):
                    acc[j] = acc[j] + add[j]
                    mag[j] = mag[j] + np.abs(add[j])
                aux["d0"][..., k], aux["d1"][..., k], aux["dist"][..., k] = d0, d1, dist
            eighth = dt(0.125)
            per[..., 2] = np.where(valid, (total * eighth) * wq2, zero)
            out["grad_corner"] = np.where(valid[..., None], np.stack([(v * eighth) * wq2 for v in acc], -1), zero)
            out["mag"] = np.where(valid[..., None], np.stack([(v * eighth) * np.abs(wq2) for v in mag], -1), zero)
            for k, v in aux.items():
                out[k] = np.where(valid[..., None], v, dt(np.nan))
    out["per_roi"] = per
    out["loss64"] = per.astype(D).sum(1)
    out["loss"] = out["loss64"].astype(F)
    return out


# ---- loop: float32 scalars ----------------------------------------------------------------------------------------------------
def _oracle_sincos(yaw):
    import oracle
    oracle.build()
    with np.errstate(all="ignore"):
        y = np.clip(np.nan_to_num(np.asarray(yaw, F), posinf=0.0, neginf=0.0), -1e4, 1e4).astype(F)
    s, c = oracle.sincos_r(np.ascontiguousarray(y.reshape(-1)))
    return s.astype(F).reshape(y.shape), c.astype(F).reshape(y.shape)


def loss_loop(c):
    kw = c["kw"]
    x, r, t, tg = c["rcnn_cls"], c["rcnn_reg"], c["cls_target"], c["reg_target"]
    B, S = x.shape
    corner = c["rois"] is not None
    beta, cw = F(kw["beta"]), np.asarray(kw["code_weights"], F)
    num, per = np.zeros((B, 2), np.int32), np.zeros((B, S, 3), F)
    gcls, greg, gcor = np.zeros((B, S), F), np.zeros((B, S, 7), F), np.zeros((B, S, 7), F)
    SP, CP = _oracle_sincos(r[..., 6])
    if corner:
        SG, CG = _oracle_sincos(c["gt_local"][..., 6])
    half, one = F(0.5), F(1)
    with np.errstate(all="ignore"):
        for b in range(B):
            num[b] = (sum(1 for i in range(S) if t[b, i] >= 0), sum(1 for i in range(S) if c["reg_valid"][b, i] != 0))
            n = (num[b, 0], num[b, 1], num[b, 1])
            w = [F(s) / F(max(int(n[i]), 1)) if kw["normalize"] else F(s) for i, s in enumerate(kw["scale"])]
            for i in range(S):
                xv, tv = x[b, i], t[b, i]
                if tv >= 0:
                    e = np.exp(-np.abs(xv))
                    den = one + e
                    p = one / den if xv >= 0 else e / den
                    bce = (np.maximum(xv, F(0)) - (xv * tv)) + np.log1p(e)
                    per[b, i, 0], gcls[b, i] = bce * w[0], (p - tv) * w[0]
                if c["reg_valid"][b, i] == 0:
                    continue
                acc = F(0)
                for j in range(7):
                    d = (r[b, i, j] - tg[b, i, j]) * cw[j]
                    a = np.abs(d)
                    if a < beta:
                        l, sg = ((half * a) * a) / beta, d / beta
                    else:
                        l, sg = a - (half * beta), F(int(d > 0) - int(d < 0))
                    acc = acc + l
                    greg[b, i, j] = (sg * cw[j]) * w[1]
                per[b, i, 1] = acc * w[1]
                if not corner:
                    continue
                roi, gt, tt = c["rois"][b, i], c["gt_local"][b, i], r[b, i]
                la, wa, ha = max(roi[3], EPS), max(roi[4], EPS), max(roi[5], EPS)
                dg = np.sqrt((la * la) + (wa * wa))
                px, py, pz = tt[0] * dg, tt[1] * dg, tt[2] * ha
                pl, pw, ph = np.exp(tt[3]) * la, np.exp(tt[4]) * wa, np.exp(tt[5]) * ha
                sp, cp, sgt, cgt = SP[b, i], CP[b, i], SG[b, i], CG[b, i]
                hl, hw, hh = half * pl, half * pw, half * ph
                ghl, ghw, ghh = half * gt[3], half * gt[4], half * gt[5]
                total, g = F(0), [F(0)] * 7
                for k in range(8):
                    sx, sy, sz = F(SX[k]), F(SY[k]), F(SZ[k])
                    ox, oy, oz = sx * hl, sy * hw, sz * hh
                    rx, ry = (ox * cp) - (oy * sp), (ox * sp) + (oy * cp)
                    X, Y, Z = rx + px, ry + py, oz + pz
                    gox, goy, goz = sx * ghl, sy * ghw, sz * ghh
                    grx, gry = (gox * cgt) - (goy * sgt), (gox * sgt) + (goy * cgt)
                    ex, ey, ez = X - (grx + gt[0]), Y - (gry + gt[1]), Z - (goz + gt[2])
                    fx, fy = X - (gt[0] - grx), Y - (gt[1] - gry)
                    d0 = np.sqrt(((ex * ex) + (ey * ey)) + (ez * ez))
                    d1 = np.sqrt(((fx * fx) + (fy * fy)) + (ez * ez))
                    dist, ux, uy = (d1, fx, fy) if d1 < d0 else (d0, ex, ey)
                    if dist < one:
                        total = total + (half * dist) * dist
                        ax, ay, az = ux, uy, ez
                    else:
                        total = total + (dist - half)
                        ax, ay, az = ux / dist, uy / dist, ez / dist
                    add = (ax * dg, ay * dg, az * ha, ((ax * cp) + (ay * sp)) * ox, ((ay * cp) - (ax * sp)) * oy, az * oz, (ay * rx) - (ax * ry))
                    g = [g[j] + add[j] for j in range(7)]
                per[b, i, 2] = (total * F(0.125)) * w[2]
                gcor[b, i] = [(v * F(0.125)) * w[2] for v in g]
    out = {"num": num, "per_roi": per, "grad_cls": gcls, "grad_reg": greg}
    if corner:
        out["grad_corner"] = gcor
    return out


# ---- the replaced code's global-frame form, binary64 under torch autograd ------------------------------------------------------
def global_boxes(c):
    """gt_local taken back into the scene's frame through rois (binary64): the boxes the global-frame form compares with.
    Rows with reg_valid == 0 come back as zeros."""
    valid = c["reg_valid"] != 0
    roi, gt = np.where(valid[..., None], c["rois"][..., :7], 0).astype(D), np.where(valid[..., None], c["gt_local"], 0).astype(D)
    s, co = np.sin(roi[..., 6]), np.cos(roi[..., 6])
    out = gt.copy()
    out[..., 0] = gt[..., 0] * co - gt[..., 1] * s + roi[..., 0]
    out[..., 1] = gt[..., 0] * s + gt[..., 1] * co + roi[..., 1]
    out[..., 2] = gt[..., 2] + roi[..., 2]
    out[..., 6] = gt[..., 6] + roi[..., 6]
    return out


def torch_composition(c):
    """-> loss [B,3], d(sum of loss)/d rcnn_cls, d(sum of loss)/d rcnn_reg: numpy binary64.  The normaliser is §29's (per scene)."""
    import torch
    kw = c["kw"]
    f64 = torch.float64
    valid = torch.from_numpy(np.array(c["reg_valid"] != 0))
    x = torch.tensor(c["rcnn_cls"], dtype=f64, requires_grad=True)
    reg = torch.tensor(c["rcnn_reg"], dtype=f64, requires_grad=True)
    t = torch.tensor(c["cls_target"], dtype=f64)
    live = t >= 0
    tgt = torch.tensor(np.where((c["reg_valid"] != 0)[..., None], c["reg_target"], 0), dtype=f64)
    cw = torch.tensor(np.asarray(kw["code_weights"], F), dtype=f64)
    scale = torch.tensor(np.asarray(kw["scale"], F), dtype=f64)
    beta = float(F(kw["beta"]))
    n_cls, n_reg = live.sum(1).clamp(min=1).to(f64), valid.sum(1).clamp(min=1).to(f64)
    if not kw["normalize"]:
        n_cls, n_reg = torch.ones_like(n_cls), torch.ones_like(n_reg)
    bce = torch.nn.functional.binary_cross_entropy_with_logits(x, t.clamp(min=0), reduction="none")
    l_cls = (bce * live).sum(1) / n_cls * scale[0]
    diff = (reg - tgt) * cw
    a = diff.abs()
    sl1 = torch.where(a < beta, 0.5 * a * a / beta, a - 0.5 * beta).sum(-1)
    l_reg = (sl1 * valid).sum(1) / n_reg * scale[1]
    l_cor = torch.zeros_like(l_reg)
    if c["rois"] is not None:
        roi = torch.tensor(np.where((c["reg_valid"] != 0)[..., None], c["rois"][..., :7], 1.0), dtype=f64)
        gt = torch.tensor(np.where((c["reg_valid"] != 0)[..., None], global_boxes(c), 1.0), dtype=f64)
        la, wa, ha = (roi[..., q].clamp(min=float(EPS)) for q in (3, 4, 5))
        dg = (la * la + wa * wa).sqrt()
        s, co = roi[..., 6].sin(), roi[..., 6].cos()
        lx, ly, lz = reg[..., 0] * dg, reg[..., 1] * dg, reg[..., 2] * ha
        pred = torch.stack([lx * co - ly * s + roi[..., 0], lx * s + ly * co + roi[..., 1], lz + roi[..., 2], reg[..., 3].exp() * la,
                            reg[..., 4].exp() * wa, reg[..., 5].exp() * ha, reg[..., 6] + roi[..., 6]], -1)

        def corners(bx):
            tpl = torch.tensor([SX, SY, SZ], dtype=f64).T / 2                     # [8,3]
            o = bx[..., None, 3:6] * tpl                                          # [B,S,8,3]
            sn, cs = bx[..., 6, None].sin(), bx[..., 6, None].cos()
            return torch.stack([o[..., 0] * cs - o[..., 1] * sn + bx[..., 0, None], o[..., 0] * sn + o[..., 1] * cs + bx[..., 1, None],
                                o[..., 2] + bx[..., 2, None]], -1)
        turned = gt.clone()
        turned[..., 6] = turned[..., 6] + np.pi
        pc = corners(pred)
        dist = torch.minimum((pc - corners(gt)).norm(dim=-1), (pc - corners(turned)).norm(dim=-1))
        hub = torch.where(dist < 1.0, 0.5 * dist * dist, dist - 0.5).mean(-1)
        l_cor = (hub * valid).sum(1) / n_reg * scale[2]
    loss = torch.stack([l_cls, l_reg, l_cor], 1)
    loss.sum().backward()
    return loss.detach().numpy(), x.grad.numpy(), reg.grad.numpy()


# ---- cases ----------------------------------------------------------------------------------------------------------------------
def _rng(*key):
    return np.random.default_rng([zlib.crc32(str(k).encode()) for k in key])


def margins(c):
    """Per valid row the smallest |d0 - d1| and |dist - 1| over its eight corners, in binary64 (inf elsewhere): [B,S] each."""
    e = loss_vec(c, D)
    with np.errstate(all="ignore"):
        flip = np.nan_to_num(np.abs(e["d0"] - e["d1"]).min(-1), nan=np.inf)
        kink = np.nan_to_num(np.abs(e["dist"] - 1.0).min(-1), nan=np.inf)
    return flip, kink


def _predictions(name, c):
    """Seeded predictions on the targets of `c`: rcnn_cls ~ N(0, 0.4); rcnn_reg = reg_target + noise of sigma 0.03, 0.15 or 0.4 per
    row (corner distances on both sides of 1, |d| on both sides of beta) on the valid rows, N(0, 0.4) elsewhere; every fifth valid
    row is turned by pi (the flipped box is the nearer one).  Rows that come within MARGIN of the flip or of the Huber kink are
    redrawn, deterministically, until none does."""
    rng = _rng(name)
    valid = c["reg_valid"] != 0
    B, S = valid.shape
    c["rcnn_cls"] = rng.normal(0, 0.4, (B, S)).astype(F)
    base = np.where(valid[..., None], c["reg_target"], 0).astype(D)
    turn = np.zeros((B, S, 7))
    turn[..., 6] = np.where((np.cumsum(valid.reshape(-1)).reshape(B, S) % 5 == 2) & valid, np.pi, 0.0)

    def draw(r, shape):
        sigma = np.where(valid, r.choice([0.03, 0.15, 0.4], valid.shape), 0.4)[..., None]
        return r.normal(0, 1, shape) * sigma

    reg = base + turn + draw(rng, (B, S, 7))
    c["rcnn_reg"] = reg.astype(F)
    if c["rois"] is None:
        return
    for attempt in range(1, 50):
        flip, kink = margins(c)
        bad = (flip < MARGIN) | (kink < MARGIN)
        if name in TIES:
            bad = kink < MARGIN
        if not bad.any():
            return
        again = base + turn + draw(_rng(name, attempt), (B, S, 7))
        c["rcnn_reg"] = np.where(bad[..., None], again, c["rcnn_reg"]).astype(F)
    raise AssertionError(f"{name}: rows within the margin after 50 draws")


def _poison(c):
    """NaN in reg_target, gt_local and the rois row wherever reg_valid == 0."""
    bad = (c["reg_valid"] == 0)[..., None]
    for k in ("reg_target", "gt_local", "rois"):
        if c[k] is not None:
            c[k] = np.where(bad, F(np.nan), c[k]).astype(F)


def _from_targets(name, src, S=None, wide=False, corner=True, **kw):
    e = roi_head_ref.expected(src)
    S = e["cls_target"].shape[1] if S is None else S
    c = {k: np.array(e[k][:, :S]) for k in ("cls_target", "reg_valid", "reg_target", "gt_local")}
    c["rois"] = np.array(e["rois_s"][:, :S])
    c["kw"] = dict(KW, **kw)
    _predictions(name, c)
    _poison(c)
    if wide:                                                        # rows of D = 9: two columns that are never read
        c["rois"] = np.concatenate([c["rois"], np.full(c["rois"].shape[:2] + (2,), np.nan, F)], -1)
    if not corner:
        c["rois"] = c["gt_local"] = None
    return c


def _built(name, S=40):
    """The two exact cases.  coincident: rcnn_reg = 0 on gt_local = (0, 0, 0, la, wa, ha, 0): the decoded box IS the ground truth,
    every corner distance is 0.  degenerate: gl = gw = 0, the box and the box turned by pi are one segment: d0 == d1 at every
    corner, the tie stays unflipped and either choice has the same value."""
    rng = _rng(name)
    B = 2
    rois = np.zeros((B, S, 7), F)
    rois[..., :3] = rng.uniform(-20, 20, (B, S, 3))
    rois[..., 3:6] = rng.uniform(0.6, 5.0, (B, S, 3))
    rois[..., 6] = rng.uniform(-3, 3, (B, S))
    valid = (rng.random((B, S)) < 0.7).astype(np.int32)
    valid[:, 0] = 1
    gl = np.zeros((B, S, 7), F)
    c = dict(cls_target=np.where(rng.random((B, S)) < 0.2, -1, rng.uniform(0, 1, (B, S))).astype(F), reg_valid=valid,
             reg_target=rng.normal(0, 0.3, (B, S, 7)).astype(F), rois=rois, gt_local=gl, kw=dict(KW))
    if name == "coincident":
        gl[..., 3:6] = rois[..., 3:6]
        c["rcnn_cls"] = rng.normal(0, 0.4, (B, S)).astype(F)
        c["rcnn_reg"] = np.zeros((B, S, 7), F)
    else:
        gl[..., :3] = rng.normal(0, 0.5, (B, S, 3))
        gl[..., 5] = rng.uniform(1.0, 2.0, (B, S))
        gl[..., 6] = rng.uniform(-1.5, 1.5, (B, S))
        c["reg_target"] = np.zeros((B, S, 7), F)
        _predictions(name, c)
    _poison(c)
    return c


TIES = ("degenerate",)                                               # d0 == d1 by construction: exempt from the flip margin
BUILDERS = {
    "both": lambda: _from_targets("both", "both"),                                       # B 2, S 32
    "no_gt": lambda: _from_targets("no_gt", "no_gt"),                                    # scene 0: n_reg = 0
    "ragged": lambda: _from_targets("ragged", "ragged"),                                 # B 3; scene 2: empty slots, n_cls = n_reg = 0
    "odd": lambda: _from_targets("odd", "odd", wide=True),                               # S 1, rois rows of D = 9
    "cap": lambda: _from_targets("cap", "cap"),                                          # S 1024: four passes
    "s257": lambda: _from_targets("s257", "cap", S=257, wide=True),                      # one slot into a second pass
    "heading": lambda: _from_targets("heading", "heading"),                              # S 128, headings at +-pi/2
    "on_threshold:cls": lambda: _from_targets("on_threshold:cls", "on_threshold:cls"),   # the ignored band (cls_target -1)
    "both:unit": lambda: _from_targets("both:unit", "both", beta=1.0, code_weights=(1.0,) * 7, scale=(1.0, 1.0, 1.0)),
    "both:nocorner": lambda: _from_targets("both:nocorner", "both", corner=False),
    "coincident": lambda: _built("coincident"),
    "degenerate": lambda: _built("degenerate"),
}
CASES = list(BUILDERS)
INPUTS = ("rcnn_cls", "rcnn_reg", "cls_target", "reg_valid", "reg_target", "rois", "gt_local")


@functools.lru_cache(maxsize=None)
def case(name):
    """-> dict(rcnn_cls, rcnn_reg, cls_target, reg_valid, reg_target, rois | None, gt_local | None, kw).  Treat as read-only."""
    c = BUILDERS[name]()
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


def unnormalised(c):
    """The case with normalize = False (wq_i = scale_i)."""
    return dict(c, kw=dict(c["kw"], normalize=False))


@functools.lru_cache(maxsize=None)
def expected(name, normalize=True):
    """{"f32": the vectorised float32 reference, "f64": the binary64 evaluation} of a named case (normalize=False: of
    `unnormalised(case(name))`), computed once.  Treat as read-only."""
    c = case(name) if normalize else unnormalised(case(name))
    out = {"f32": loss_vec(c), "f64": loss_vec(c, D)}
    for r in out.values():
        for v in r.values():
            v.setflags(write=False)
    return out


def tolerance(want64, scale=None):
    """§9: 1e-4 absolute + 1e-4 relative to |want64| (or to `scale`: the sum of the magnitudes of the addends)."""
    return 1e-4 + 1e-4 * np.abs(want64 if scale is None else scale)
