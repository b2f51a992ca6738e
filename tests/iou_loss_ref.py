"""float32 numpy reference of the rotated IoU loss (SPEC.md §34), operation for operation: every array here is float32, numpy
neither contracts nor reorders elementwise operations, so these are the section's bits.

sin / cos come from the oracle's §13 routine (``oracle.sincos_r``); the clipped area is ``box_ref``'s scalar
Sutherland-Hodgman clip on the vertices §34 names (the pair's centre difference plus the local corners), so ``iou`` is the
diagonal of ``box_ref.boxes_iou``.  The edge pass, the enclosing box, the quotient rules and the selections are whole-array
code; a selection is ``np.where`` (never a multiplication by a mask), a maximum with a tie rule is a strict comparison.

``rotated_iou_loss(..., decoded=boxes)`` with ``code="roi"`` evaluates the section on the given decoded boxes instead of its own
``expf`` (the GPU test hands it the device's, so that everything behind the library function compares under ``==``)."""
import numpy as np

import box_ref
import oracle

F = np.float32
ZERO, HALF, ONE, TWO = F(0.0), F(0.5), F(1.0), F(2.0)
EPS = F(1e-5)
SXH = (F(0.5), F(-0.5), F(-0.5), F(0.5))          # half the corner signs of §13's order (+,+), (-,+), (-,-), (+,-)
SYH = (F(0.5), F(0.5), F(-0.5), F(-0.5))
MODES, KINDS, CODES = ("bev", "3d"), ("iou", "diou"), ("box", "roi")
_INTER = {}


def roi_anchor(rois):
    """§28.1: (la, wa, ha, dg) of rois [N,D]."""
    la, wa, ha = (np.maximum(rois[:, q], EPS) for q in (3, 4, 5))
    return la, wa, ha, np.sqrt((la * la) + (wa * wa))


def decode(reg, rois):
    """§34 code="roi": reg [N,7], rois [N,D] -> the box in the RoI's frame [N,7] (numpy's float32 exp stands for expf)."""
    reg = np.asarray(reg, F)
    la, wa, ha, dg = roi_anchor(np.asarray(rois, F))
    with np.errstate(all="ignore"):
        return np.stack([reg[:, 0] * dg, reg[:, 1] * dg, reg[:, 2] * ha, np.exp(reg[:, 3]) * la, np.exp(reg[:, 4]) * wa,
                         np.exp(reg[:, 5]) * ha, reg[:, 6]], 1).astype(F)


def _clip_edge(X0, Y0, X1, Y1, ghl, ghw):
    """Liang-Barsky of the segment against |X| <= ghl, |Y| <= ghw (closed) -> (f, tm): the fraction inside and the
    parameter of its midpoint, (0, 0) when nothing is inside."""
    dX, dY = X1 - X0, Y1 - Y0
    t0, t1 = np.zeros_like(X0), np.ones_like(X0)
    ok = np.ones(X0.shape, bool)
    for p, q in ((-dX, X0 + ghl), (dX, ghl - X0), (-dY, Y0 + ghw), (dY, ghw - Y0)):
        par = p == ZERO
        ok = ok & ~(par & ~(q >= ZERO))
        r = q / p
        t0 = np.where(~par & (p < ZERO) & (r > t0), r, t0)
        t1 = np.where(~par & (p > ZERO) & (r < t1), r, t1)
    f = t1 - t0
    live = ok & (f > ZERO)
    return np.where(live, f, ZERO), np.where(live, HALF * (t0 + t1), ZERO)


def box_loss(P, T, mode, kind):
    """pred P [N,7], target T [N,7] f32 -> (loss, iou, grad [N,7]), unweighted."""
    N = P.shape[0]
    x, y, z, l, w, h, th = (np.ascontiguousarray(P[:, j]) for j in range(7))
    gx, gy, gz, gl, gw, gh, gth = (np.ascontiguousarray(T[:, j]) for j in range(7))
    with np.errstate(all="ignore"):
        sp, cp = oracle.sincos_r(th)
        st, ct = oracle.sincos_r(gth)
        sp, cp, st, ct = sp.astype(F), cp.astype(F), st.astype(F), ct.astype(F)
        hl, hw, ghl, ghw = HALF * l, HALF * w, HALF * gl, HALF * gw
        ddx, ddy = x - gx, y - gy
        # §13 local corners, the clip's vertices and the pred's corners in the target's frame
        cx, cy, tx, ty, X, Y = [], [], [], [], [], []
        for k in range(4):
            dxk, dyk = (hl, -hl, -hl, hl)[k], (hw, hw, -hw, -hw)[k]
            cx.append((cp * dxk) - (sp * dyk))
            cy.append((sp * dxk) + (cp * dyk))
            gdx, gdy = (ghl, -ghl, -ghl, ghl)[k], (ghw, ghw, -ghw, -ghw)[k]
            tx.append((ct * gdx) - (st * gdy))
            ty.append((st * gdx) + (ct * gdy))
            vx, vy = ddx + cx[k], ddy + cy[k]
            X.append((vx * ct) + (vy * st))
            Y.append((vy * ct) - (vx * st))
        key = (P[:, [0, 1, 3, 4, 6]].tobytes(), T[:, [0, 1, 3, 4, 6]].tobytes())          # the scalar clip is the slow part: once per set of pairs
        if key not in _INTER:
            _INTER[key] = np.array([box_ref.clip_area([ddx[i] + cx[k][i] for k in range(4)], [ddy[i] + cy[k][i] for k in range(4)],
                                                      [tx[k][i] for k in range(4)], [ty[k][i] for k in range(4)]) for i in range(N)], F).reshape(N)
        inter = _INTER[key]
        # edge pass
        ln, tm = [], []
        for k in range(4):
            f, t = _clip_edge(X[k], Y[k], X[(k + 1) & 3], Y[(k + 1) & 3], ghl, ghw)
            ln.append(f * (l if k % 2 == 0 else w))
            tm.append(t)
        a, b = ln[3] - ln[1], ln[0] - ln[2]
        dI = {"x": (cp * a) - (sp * b), "y": (cp * b) + (sp * a), "l": HALF * (ln[1] + ln[3]), "w": HALF * (ln[0] + ln[2])}
        u0, v1, u2, v3 = hl - (tm[0] * l), hw - (tm[1] * w), (tm[2] * l) - hl, (tm[3] * w) - hw
        dI["t"] = ((ln[0] * u0) + (ln[1] * v1)) - ((ln[2] * u2) + (ln[3] * v3))
        zero = np.zeros(N, F)
        if mode == "bev":
            S = (l * w) + (gl * gw)
            den = S - inter
            iou = np.where(den > ZERO, inter / den, ZERO)
            live = (inter > ZERO) & (den > ZERO)
            den2 = den * den
            num = {"x": dI["x"] * S, "y": dI["y"] * S, "z": zero, "l": (dI["l"] * S) - (inter * w), "w": (dI["w"] * S) - (inter * l),
                   "h": zero, "t": dI["t"] * S}
        else:
            ha, hb = HALF * h, HALF * gh
            topP, topT, botP, botT = z + ha, gz + hb, z - ha, gz - hb
            oh = np.minimum(topP, topT) - np.maximum(botP, botT)
            oh = np.where(oh > ZERO, oh, ZERO)
            i3 = inter * oh
            S = ((l * w) * h) + ((gl * gw) * gh)
            den = S - i3
            iou = np.where(den > ZERO, i3 / den, ZERO)
            live = (inter > ZERO) & (oh > ZERO) & (den > ZERO)
            den2 = den * den
            tp, bp = np.where(topP < topT, ONE, ZERO), np.where(botP > botT, ONE, ZERO)          # a tie is the target's
            num = {"x": (dI["x"] * oh) * S, "y": (dI["y"] * oh) * S, "z": (inter * (tp - bp)) * S,
                   "l": ((dI["l"] * oh) * S) - (i3 * (w * h)), "w": ((dI["w"] * oh) * S) - (i3 * (l * h)),
                   "h": ((inter * (HALF * (tp + bp))) * S) - (i3 * (l * w)), "t": (dI["t"] * oh) * S}
        g = {q: np.where(live, -(num[q] / den2), ZERO) for q in "xyzlwht"}
        loss = ONE - iou
        if kind == "diou":
            rho2 = (ddx * ddx) + (ddy * ddy)
            # the four extremes: value, and the winning corner's half signs (0, 0 while the target holds it)
            ext = [[ghl.copy(), zero, zero], [-ghl, zero, zero], [ghw.copy(), zero, zero], [-ghw, zero, zero]]
            for k in range(4):
                for e, (v, gt) in enumerate(((X[k], True), (X[k], False), (Y[k], True), (Y[k], False))):
                    won = (v > ext[e][0]) if gt else (v < ext[e][0])
                    ext[e] = [np.where(won, v, ext[e][0]), np.where(won, SXH[k], ext[e][1]), np.where(won, SYH[k], ext[e][2])]
            cw_, ch_ = ext[0][0] - ext[1][0], ext[2][0] - ext[3][0]
            c2 = (cw_ * cw_) + (ch_ * ch_)
            cd, sd = (cp * ct) + (sp * st), (sp * ct) - (cp * st)

            def dX(e):
                sx, sy = ext[e][1], ext[e][2]
                own = sx != ZERO
                a_, b_ = sx * l, sy * w
                d = {"x": ct, "y": st, "l": sx * cd, "w": -(sy * sd), "t": -((a_ * sd) + (b_ * cd))}
                return {q: np.where(own, d[q], ZERO) for q in d}

            def dY(e):
                sx, sy = ext[e][1], ext[e][2]
                own = sx != ZERO
                a_, b_ = sx * l, sy * w
                d = {"x": -st, "y": ct, "l": sx * sd, "w": sy * cd, "t": (a_ * cd) - (b_ * sd)}
                return {q: np.where(own, d[q], ZERO) for q in d}

            dx1, dx0, dy1, dy0 = dX(0), dX(1), dY(2), dY(3)
            dc2 = {q: TWO * ((cw_ * (dx1[q] - dx0[q])) + (ch_ * (dy1[q] - dy0[q]))) for q in "xylwt"}
            dr2 = {"x": TWO * ddx, "y": TWO * ddy, "z": zero, "l": zero, "w": zero, "h": zero, "t": zero}
            dc2["z"], dc2["h"] = zero, zero
            if mode == "3d":
                ddz = z - gz
                rho2 = rho2 + (ddz * ddz)
                cz = np.maximum(topP, topT) - np.minimum(botP, botT)
                c2 = c2 + (cz * cz)
                tpz, bpz = np.where(topP > topT, ONE, ZERO), np.where(botP < botT, ONE, ZERO)
                dc2["z"] = TWO * (cz * (tpz - bpz))
                dc2["h"] = TWO * (cz * (HALF * (tpz + bpz)))
                dr2["z"] = TWO * ddz
            okc = c2 > ZERO
            loss = loss + np.where(okc, rho2 / c2, ZERO)
            c4 = c2 * c2
            for q in "xyzlwht":
                g[q] = g[q] + np.where(okc, ((dr2[q] * c2) - (rho2 * dc2[q])) / c4, ZERO)
    return loss.astype(F), iou.astype(F), np.stack([g[q] for q in "xyzlwht"], 1).astype(F)


def rotated_iou_loss(pred, target, weight=None, mode="3d", kind="iou", code="box", rois=None, decoded=None):
    """§34 on rows: pred [N,Dp], target [N,Dt] (, weight [N]) (, rois [N,Dr]) -> (loss [N], iou [N], grad [N,7], decoded [N,7] or
    None).  ``decoded``: boxes to take for the decode's result (code="roi")."""
    assert mode in MODES and kind in KINDS and code in CODES and (rois is not None) == (code == "roi")
    pred, target = np.asarray(pred, F), np.asarray(target, F)
    P, T = pred[:, :7], target[:, :7]
    if code == "roi":
        la, wa, ha, dg = roi_anchor(np.asarray(rois, F))
        P = decode(pred, rois) if decoded is None else np.asarray(decoded, F)
        decoded = P
    loss, iou, grad = box_loss(P, T, mode, kind)
    with np.errstate(all="ignore"):
        on = None
        if weight is not None:
            wt = np.asarray(weight, F)
            on = wt != ZERO
            loss, grad = loss * wt, grad * wt[:, None]
        if code == "roi":
            jac = np.stack([dg, dg, ha, P[:, 3], P[:, 4], P[:, 5]], 1)
            grad = np.concatenate([grad[:, :6] * jac, grad[:, 6:]], 1)
        if on is not None:                              # selected last: what a row of weight 0 holds never reaches a result
            loss, grad = np.where(on, loss, ZERO), np.where(on[:, None], grad, ZERO)
    return loss.astype(F), iou, grad.astype(F), decoded
