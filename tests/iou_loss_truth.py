"""The truth of the rotated IoU loss (SPEC.md §34): plain Python / numpy binary64 on binary64 rows, no code shared with
tests/iou_loss_ref.py or the kernel.  Of tests/box_truth.py only the private clip (`_clip_area`) and the quotient (`_iou_of`) are
used: its entry points round their rows to float32, and a finite difference needs rows that move by 1e-5 of a box.

The loss is evaluated from its definition: the pair is moved by -target.centre, the intersection is the Sutherland-Hodgman area,
the DIoU term takes the pred's corners turned by -target.yaw as complex numbers.  **The true gradient is a central difference**
of that loss, per column, at a step h scaled to the pair (`steps`) and again at h / 2.  The loss is piecewise rational in every
column, so where no vertex crosses an edge within +-h the difference at h / 2 is off by about (h / 2)^2 f''' / 6, far below
TRUTH_ERR; where one does, the two steps disagree and the pair is reported as ill-conditioned (`grad64`'s second result).

The error scale of a float32 gradient, the counterpart of box_truth.tol():
    gscale(a, b)[j] = 2^-24 (D_a + D_b)^2 / min(l_a w_a, l_b w_b) / length_j,     D = hypot(l, w)
One float32 rounding of a coordinate of size D_a + D_b (the extent of the pair in b's frame) moves the clipped LENGTH of an
edge by about 2^-24 (D_a + D_b), and dIoU/dx = dI/dx S / den^2 by that over the smaller area: length_j = D_a + D_b for the
columns x and y.  dI/dyaw is a sum of length x lever arm, one more factor D_a + D_b: length_j = 1 for the yaw.  dIoU/dl =
(dI/dl S - I w) / den^2 carries the error of the clipped AREA itself, 2^-24 (D_a + D_b)^2, times w / den^2 <= 1 / (l min area):
length_j = min(l_a, l_b) for l and likewise min(w_a, w_b) for w.  dIoU/dz and dIoU/dh are at most about 1 / min(h_a, h_b) and
carry a relative rounding error, which 2^-24 (D_a + D_b)^2 / min area >= 8 x 2^-24 covers: length_j = min(h_a, h_b) for z and h.
The DIoU term's gradient is at most about 2 / c with c no smaller than any of these lengths, and carries a relative error too.

Ties.  §34 names which one-sided derivative the gradient is where the loss has a kink in z or h: an end of the height overlap
or of the height hull that both boxes share is the TARGET's, and intervals that only touch do not overlap.  The builders put z
and h on a lattice, so such ties are common; the truth therefore holds those choices fixed at the point where the gradient is
taken (`branches`) while it moves z and h, which makes the central difference the derivative §34 names and not the mean of the
two sides.  Everything in the plane (vertices crossing edges, the corner that holds an extreme of the enclosing box) is left
to the h against h / 2 comparison.
G_TOL = 4 x G_MEASURED, the margin C_TOL has over C_MEASURED; G_MEASURED is the largest err / gscale of the float32 reference
(tests/iou_loss_ref.py) over every well-conditioned pair of tests/test_iou_loss_cpu.py (every kind x mode x size family,
n = 600, seed 1), where the conditioning of the kept pairs (an edge pass divides by the sine of the angle between two edges,
at least about 0.1 there) is part of the constant.  test_gradient_tolerance_constant prints it and fails above G_TOL / 2.
For orientation, the reference's largest absolute errors over those pairs: 8.4e-7 (x, y, z), 1.6e-5 (l, w, h), 3.8e-6 (yaw) on
the object family and 2.2e-6, 6.2e-5, 2.5e-6 on thin, where a side of 0.05 m makes the derivative itself as large as 20 / m."""
import cmath
import math

import numpy as np

from box_truth import _clip_area, _iou_of

G_MEASURED = 6.53
G_TOL = 4.0 * G_MEASURED
TRUTH_ERR = 0.01          # the truth's own error, in units of gscale: the h and h / 2 differences agree to this, or the pair is ill-conditioned
H_REL = 1e-5


TRUTH_FAMILIES = ("perturbed", "yaw1e3", "nested", "far")      # held against the truth; the others have one-sided derivatives


def well_conditioned(family, a, b):
    """[N] bool, a condition on the rows and not a measurement: perturbed / yaw1e3 keep |sin 2(yaw_a - yaw_b)| >= 0.2 (no edge of a
    nearly parallel to an edge of b), nested keeps |l_b / l_a - 1| >= 0.02 (no edge of a on an edge of b), far keeps all."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    if family in ("perturbed", "yaw1e3"):
        return np.abs(np.sin(2.0 * (a[:, 6] - b[:, 6]))) >= 0.2
    if family == "nested":
        return np.abs(b[:, 3] / a[:, 3] - 1.0) >= 0.02
    assert family == "far"
    return np.ones(a.shape[0], bool)


def _corners(box):
    c, s = math.cos(box[6]), math.sin(box[6])
    hl, hw = box[3] / 2, box[4] / 2
    return [(c * dx - s * dy, s * dx + c * dy) for dx, dy in ((hl, hw), (-hl, hw), (-hl, -hw), (hl, -hw))]


def branches(p, t):
    """Which ends of the two height intervals are the pred's, at the point where the gradient is taken: (top of the overlap,
    bottom of the overlap, top of the hull, bottom of the hull), and whether the overlap is positive.  A tie is the target's, and
    intervals that only touch do not overlap (§34)."""
    tp, tt, bp, bt = p[2] + p[5] / 2, t[2] + t[5] / 2, p[2] - p[5] / 2, t[2] - t[5] / 2
    return tp < tt, bp > bt, tp > tt, bp < bt, min(tp, tt) - max(bp, bt) > 0


def iou64(p, t, mode, br=None):
    """True IoU of two binary64 rows, clipped in t's frame.  The height overlap takes the ends `br` names (default: p's own)."""
    dx, dy = p[0] - t[0], p[1] - t[1]
    inter = _clip_area([(dx + x, dy + y) for x, y in _corners(p)], _corners(t))
    if mode == "bev":
        return _iou_of(inter, p, t, mode)
    br = branches(p, t) if br is None else br
    top = p[2] + p[5] / 2 if br[0] else t[2] + t[5] / 2
    bot = p[2] - p[5] / 2 if br[1] else t[2] - t[5] / 2
    i3 = inter * (top - bot if br[4] else 0.0)
    den = p[3] * p[4] * p[5] + t[3] * t[4] * t[5] - i3
    return i3 / den if den > 0 else 0.0


def loss64(p, t, mode, kind, br=None):
    br = branches(p, t) if br is None else br
    v = 1.0 - iou64(p, t, mode, br)
    if kind == "diou":
        d = complex(p[0] - t[0], p[1] - t[1])
        rot = cmath.exp(-1j * t[6])
        pts = [(d + complex(sx * p[3] / 2, sy * p[4] / 2) * cmath.exp(1j * p[6])) * rot for sx, sy in ((1, 1), (-1, 1), (-1, -1), (1, -1))]
        xs, ys = [q.real for q in pts] + [t[3] / 2, -t[3] / 2], [q.imag for q in pts] + [t[4] / 2, -t[4] / 2]
        rho2, c2 = abs(d) ** 2, (max(xs) - min(xs)) ** 2 + (max(ys) - min(ys)) ** 2
        if mode == "3d":
            rho2 += (p[2] - t[2]) ** 2
            zt = p[2] + p[5] / 2 if br[2] else t[2] + t[5] / 2
            zb = p[2] - p[5] / 2 if br[3] else t[2] - t[5] / 2
            c2 += (zt - zb) ** 2
        v += rho2 / c2
    return v


def steps(p, t):
    """The seven steps of a pair: H_REL of the smallest BEV side for x, y, l, w, of the smaller height for z and h, and the
    angle that moves the pred's far corner by the first."""
    m = H_REL * min(p[3], p[4], t[3], t[4])
    hz = H_REL * min(p[5], t[5])
    return (m, m, hz, m, m, hz, m / (0.5 * math.hypot(p[3], p[4])))


def _central(p, t, mode, kind, hs):
    g, br = [], branches(p, t)
    for j in range(7):
        hi, lo = list(p), list(p)
        hi[j] += hs[j]
        lo[j] -= hs[j]
        g.append((loss64(hi, t, mode, kind, br) - loss64(lo, t, mode, kind, br)) / (hi[j] - lo[j]))
    return g


def gscale(a, b):
    """[..., 7] the float32 error scale of the gradient of one pair (see the module's text)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    d = np.hypot(a[..., 3], a[..., 4]) + np.hypot(b[..., 3], b[..., 4])
    base = 2.0 ** -24 * d * d / np.minimum(a[..., 3] * a[..., 4], b[..., 3] * b[..., 4])
    hz, ml, mw = np.minimum(a[..., 5], b[..., 5]), np.minimum(a[..., 3], b[..., 3]), np.minimum(a[..., 4], b[..., 4])
    return np.stack([base / d, base / d, base / hz, base / ml, base / mw, base / hz, base], -1)


def grad64(pred, target, mode, kind):
    """pred, target [N,>=7] (any float rows; widened, never rounded) -> (loss [N], grad [N,7] at h / 2, ill [N] bool: the
    differences at h and h / 2 disagree by more than TRUTH_ERR x gscale in some column)."""
    P, T = np.asarray(pred, np.float64)[:, :7], np.asarray(target, np.float64)[:, :7]
    sc = gscale(P, T)
    loss, grad, ill = np.empty(P.shape[0]), np.empty((P.shape[0], 7)), np.empty(P.shape[0], bool)
    for i in range(P.shape[0]):
        p, t = P[i].tolist(), T[i].tolist()
        hs = steps(p, t)
        g1 = _central(p, t, mode, kind, hs)
        g2 = _central(p, t, mode, kind, [0.5 * h for h in hs])
        loss[i], grad[i] = loss64(p, t, mode, kind), g2
        ill[i] = bool((np.abs(np.array(g1) - np.array(g2)) > TRUTH_ERR * sc[i]).any())
    return loss, grad, ill
