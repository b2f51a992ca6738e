"""Numpy float32 reference of SPEC.md §35 (training augmentation: global_augment, gt_paste), every operation written out in the
section's order on np.float32, so these are the spec's bits.  Two forms of gt_paste, as roi_head_ref.py has: ``loop`` tests a
slot against one box at a time with the scalar ``box_ref.iou_bev_pair``; ``vec`` takes the oracle's IoU on the expanded pairs
(``box_ref.iou_bev_matrix``) and ``box_ref.inside`` on all accepted boxes at once.  Built on box_ref, io._h and
roi_head_ref.sincos; none of them is modified.  The named cases of the tests are made here too (``case(name)``)."""
import functools

import numpy as np

import box_ref
from roi_head_ref import sincos
from sad_amd import io as _io

F = np.float32
PI_F = F(3.14159274)
DRAW_GLOBAL, DRAW_PASTE = 0xA0000000, 0xC0000000
MAX_SLOTS = 512
IDENTITY = dict(flip_x=False, flip_y=False, rot_range=(0.0, 0.0), scale_range=(1.0, 1.0), translate_range=(0.0, 0.0, 0.0))
GLOBAL = dict(flip_x=True, flip_y=True, rot_range=(-0.78539816, 0.78539816), scale_range=(0.95, 1.05), translate_range=(0.5, 0.25, 0.125))


def call_seed(seed, step):
    """§35: the seed of call number ``step``."""
    return int(_io._h(int(seed), int(step), np.zeros(1, np.int64))[0])


def uniform(h):
    return (np.asarray(h, np.uint32) >> np.uint32(8)).astype(F) * F(2.0 ** -24)


def draw_range(h, lo, hi):
    lo, hi = F(lo), F(hi)
    return lo + uniform(h) * (hi - lo)


def draw_params(seed, B, flip_x, flip_y, rot_range, scale_range, translate_range):
    """§35.1 params [B,8] = (flips, theta, cos, sin, scale, tx, ty, tz) of the call seed."""
    P = np.zeros((B, 8), F)
    for b in range(B):
        h = _io._h(seed, b, DRAW_GLOBAL + np.arange(7))
        fx = bool(flip_x) and bool(h[0] >> np.uint32(31))
        fy = bool(flip_y) and bool(h[1] >> np.uint32(31))
        th = draw_range(h[2], rot_range[0], rot_range[1])
        s, c = sincos(np.array([th], F))
        P[b] = (F(int(fx) + 2 * int(fy)), th, c[0], s[0], draw_range(h[3], scale_range[0], scale_range[1]),
                draw_range(h[4], -F(translate_range[0]), translate_range[0]), draw_range(h[5], -F(translate_range[1]), translate_range[1]),
                draw_range(h[6], -F(translate_range[2]), translate_range[2]))
    return P


def _vec(x, y, p):
    fx, fy = int(p[0]) & 1, (int(p[0]) >> 1) & 1
    c, s, sg = p[2], p[3], p[4]
    if fx:
        y = -y
    if fy:
        x = -x
    return ((x * c) - (y * s)) * sg, ((x * s) + (y * c)) * sg


def xform_points(rows, p):
    """rows [n,Cp] of one scene under params p [8]: columns 0..2 transformed, the others copied."""
    out = np.array(rows, F, copy=True)
    x, y = _vec(out[:, 0], out[:, 1], p)
    out[:, 0] = x + p[5]
    out[:, 1] = y + p[6]
    out[:, 2] = (out[:, 2] * p[4]) + p[7]
    return out


def xform_boxes(rows, p, vel=False):
    """box rows [n,D] of one scene under params p [8]."""
    out = xform_points(rows, p)
    fx, fy = int(p[0]) & 1, (int(p[0]) >> 1) & 1
    out[:, 3:6] = out[:, 3:6] * p[4]
    yaw = out[:, 6]
    if fx:
        yaw = -yaw
    if fy:
        yaw = -(yaw + PI_F)
    out[:, 6] = yaw + p[1]
    if vel:
        out[:, 7], out[:, 8] = _vec(out[:, 7], out[:, 8], p)
    return out


def apply_params(points, offsets, boxes, P, vel=False):
    """The transform of known params on ragged (offsets [B+1]) or padded (offsets None, points [B,N,Cp]) points and boxes [B,G,D]."""
    B = boxes.shape[0]
    pts = np.array(points, F, copy=True)
    for b in range(B):
        if offsets is None:
            pts[b] = xform_points(pts[b], P[b])
        else:
            pts[offsets[b]:offsets[b + 1]] = xform_points(pts[offsets[b]:offsets[b + 1]], P[b])
    bx = np.stack([xform_boxes(boxes[b], P[b], vel) for b in range(B)]) if boxes.shape[1] else np.array(boxes, F, copy=True)
    return pts, bx


def global_augment(points, offsets, boxes, seed, vel=False, **cfg):
    """§35.1 -> (points_out, boxes_out, params); ``seed`` is the call seed."""
    P = draw_params(seed, boxes.shape[0], **cfg)
    return apply_params(points, offsets, boxes, P, vel) + (P,)


# ---- §35.2 --------------------------------------------------------------------------------------------------------------
def valid_gt(boxes, labels, C):
    return (labels >= 0) & (labels < C) & (boxes[:, 3] > 0) & (boxes[:, 4] > 0) & (boxes[:, 5] > 0)


def slots(c, b, gt_boxes, gt_labels):
    """The Q candidate slots of scene b -> (class [Q], db entry [Q], -1 = inactive)."""
    coff, snum = c["db"]["class_offsets"], c["sample_num"]
    C = len(snum)
    ok = valid_gt(gt_boxes, gt_labels, C)
    cls = np.repeat(np.arange(C), snum)
    d = np.full(cls.shape[0], -1, np.int64)
    q = 0
    for k in range(C):
        nc = coff[k + 1] - coff[k]
        cnt = int((ok & (gt_labels == k)).sum())
        for j in range(snum[k]):
            if nc > 0 and j < snum[k] - cnt:
                d[q] = coff[k] + int(_io._h(c["seed"], b, np.array([DRAW_PASTE + q]))[0]) % nc
            q += 1
    return cls, d


def _accept_loop(cand, d, gt):
    keep = np.zeros(d.shape[0], bool)
    for q in range(d.shape[0]):
        if d[q] < 0:
            continue
        if any(box_ref.iou_bev_pair(cand[q], g) > 0 for g in gt):
            continue
        if any(keep[r] and box_ref.iou_bev_pair(cand[q], cand[r]) > 0 for r in range(q)):
            continue
        keep[q] = True
    return keep


def _accept_vec(cand, d, gt):
    act = np.flatnonzero(d >= 0)
    keep = np.zeros(d.shape[0], bool)
    if not act.size:
        return keep
    live = np.ones(act.size, bool)
    if gt.shape[0]:
        live &= ~(box_ref.iou_bev_matrix(cand[act], gt) > 0).any(1)
    hit = box_ref.iou_bev_matrix(cand[act], cand[act]) > 0          # [q, r]: q clipped in r's frame
    kept = []
    for i in range(act.size):
        if live[i] and not hit[i, kept].any():
            kept.append(i)
    keep[act[kept]] = True
    return keep


def _removed_loop(xyz, boxes, e):
    rem = np.zeros(xyz.shape[0], bool)
    for bx in boxes:
        rem |= box_ref.inside(xyz, bx[None], e)[:, 0]
    return rem


def _removed_vec(xyz, boxes, e):
    return box_ref.inside(xyz, boxes, e).any(1) if boxes.shape[0] else np.zeros(xyz.shape[0], bool)


def _gt_paste(form, c, params=None, vel=False):
    """-> dict of §35.2's outputs; out_points holds the rows below out_offsets[B] only."""
    pts, off, gtb, gtl, db = c["points"], c["offsets"], c["gt_boxes"], c["gt_labels"], c["db"]
    B, G, D = gtb.shape
    Q, C, Cp = int(sum(c["sample_num"])), len(c["sample_num"]), pts.shape[1]
    out = dict(keep=np.zeros((B, Q), np.int32), db_index=np.full((B, Q), -1, np.int32), boxes_out=np.zeros((B, G + Q, D), F),
               labels_out=np.full((B, G + Q), -1, np.int32), num_pasted=np.zeros(B, np.int32), out_offsets=np.zeros(B + 1, np.int32))
    rows = []
    e = F(c["e"])
    for b in range(B):
        cls, d = slots(c, b, gtb[b], gtl[b])
        cand = db["boxes"][np.maximum(d, 0)]
        gt = gtb[b][valid_gt(gtb[b], gtl[b], C)]
        keep = (_accept_loop if form == "loop" else _accept_vec)(cand, d, gt)
        acc = np.flatnonzero(keep)
        out["keep"][b], out["db_index"][b], out["num_pasted"][b] = keep, d, acc.size
        out["boxes_out"][b, :G], out["labels_out"][b, :G] = gtb[b], gtl[b]
        out["boxes_out"][b, G:G + acc.size], out["labels_out"][b, G:G + acc.size] = cand[acc], cls[acc]
        scene = pts[off[b]:off[b + 1]]
        rem = (_removed_loop if form == "loop" else _removed_vec)(scene[:, :3], cand[acc], e)
        objs = [db["points"][db["offsets"][k]:min(db["offsets"][k + 1], db["offsets"][k] + c["Pmax"])] for k in d[acc]]
        new = np.concatenate(objs + [scene[~rem]]) if objs else scene[~rem]
        if params is not None:
            new = xform_points(new, params[b])
            out["boxes_out"][b] = xform_boxes(out["boxes_out"][b], params[b], vel)
        rows.append(new)
        out["out_offsets"][b + 1] = out["out_offsets"][b] + new.shape[0]
    out["out_points"] = np.concatenate(rows).astype(F).reshape(-1, Cp)
    return out


gt_paste_loop = functools.partial(_gt_paste, "loop")
gt_paste_vec = functools.partial(_gt_paste, "vec")


@functools.lru_cache(maxsize=None)
def expected(name):
    """The vectorised reference of a named case, computed once and shared (read-only)."""
    out = gt_paste_vec(case(name))
    for v in out.values():
        v.setflags(write=False)
    return out


# ---- cases ----------------------------------------------------------------------------------------------------------------
def box(x, y, z=0.0, l=4.0, w=2.0, h=2.0, yaw=0.0, D=7, extra=0.0):
    r = np.full(D, extra, F)
    r[:7] = (x, y, z, l, w, h, yaw)
    return r


def object_points(rng, bx, n, Cp):
    """n rows strictly inside the box (local coordinates within 0.45 of the extents), extra columns random."""
    u = rng.uniform(-0.45, 0.45, (n, 3)).astype(F) * bx[3:6]
    s, c = np.sin(bx[6]), np.cos(bx[6])
    p = rng.uniform(0, 1, (n, Cp)).astype(F)
    p[:, 0] = bx[0] + u[:, 0] * c - u[:, 1] * s
    p[:, 1] = bx[1] + u[:, 0] * s + u[:, 1] * c
    p[:, 2] = bx[2] + u[:, 2]
    return p


def make_db(rng, entries, C, Cp):
    """entries: (box row, class, point count), any order -> the database of §35.2, sorted by class (stable)."""
    order = sorted(range(len(entries)), key=lambda i: entries[i][1])
    boxes = np.stack([entries[i][0] for i in order]).astype(F)
    labels = np.array([entries[i][1] for i in order])
    objs = [object_points(rng, entries[i][0], entries[i][2], Cp) for i in order]
    offsets = np.concatenate([[0], np.cumsum([o.shape[0] for o in objs])]).astype(np.int32)
    coff = [int((labels < k).sum()) for k in range(C + 1)]
    return dict(points=np.concatenate(objs).astype(F).reshape(-1, Cp), offsets=offsets, boxes=boxes, class_offsets=coff)


SCENE_N = (0, 64, 700)
OBJ_N = (0, 1, 64, 130)


def scenes(rng, Cp, sizes=SCENE_N, extra=()):
    """Ragged scenes in x 0..40, y -20..20, z -2..1; ``extra``: (scene, rows [k,3]) put at the head of that scene."""
    rows, off = [], [0]
    for b, n in enumerate(sizes):
        p = rng.uniform(0, 1, (n, Cp)).astype(F)
        p[:, 0] = p[:, 0] * F(40)
        p[:, 1] = p[:, 1] * F(40) - F(20)
        p[:, 2] = p[:, 2] * F(3) - F(2)
        for sb, xyz in extra:
            if sb == b:
                p[:len(xyz), :3] = np.asarray(xyz, F)
        rows.append(p)
        off.append(off[-1] + n)
    return np.concatenate(rows).reshape(-1, Cp), np.array(off, np.int32)


def pad_gt(rows, labels, G, D, B=3):
    """Per-scene lists of (box rows, labels) -> [B,G,D] / [B,G]; unused rows are zero with label -1."""
    gb, gl = np.zeros((B, G, D), F), np.full((B, G), -1, np.int32)
    for b in range(B):
        for i, (r, k) in enumerate(zip(rows[b], labels[b])):
            gb[b, i], gl[b, i] = r, k
    return gb, gl


def _general(Cp, D, G, snum, mid, seed):
    rng = np.random.default_rng(seed)
    pts, off = scenes(rng, Cp, (0, mid, 700))
    ent = []
    for i in range(12):                                  # a 4 x 3 grid of objects, 9 m apart; some turned, two overlapping neighbours
        bx = box(4 + 9 * (i % 4), -12 + 12 * (i // 4), -0.5, 3.5 + 0.25 * (i % 3), 1.6, 1.5, 0.3 * i, D, extra=0.1 * i)
        ent.append((bx, i % 3, OBJ_N[i % 4]))
    ent[5] = (box(ent[4][0][0] + 2.0, ent[4][0][1] + 0.5, -0.5, 4.0, 1.8, 1.5, 1.0, D, extra=0.7), 2, 64)
    db = make_db(rng, ent, 3, Cp)
    rows, labs = [[] for _ in range(3)], [[] for _ in range(3)]
    if G:
        for b in range(3):                               # valid rows with padding rows in the middle
            for i in range(G):
                valid = G == 1 or i % 3 != 1
                bx = box(6 + 9 * ((i + b) % 4), -11 + 12 * ((i + 2 * b) % 3), -0.4, 3.0, 1.5, 1.4, 0.5 * i + b, D, extra=1.0 + i)
                if not valid:
                    bx[3 + i % 3] = 0 if i % 2 else -1.0
                rows[b].append(bx)
                labs[b].append(i % 3 if valid or i % 2 else -1)
    gb, gl = pad_gt(rows, labs, G, D)
    return dict(points=pts, offsets=off, gt_boxes=gb, gt_labels=gl, db=db, sample_num=list(snum), Pmax=130, seed=call_seed(seed, 3), seed_step=(seed, 3), e=0.0)


def _special(name):
    """Scenes of 0, 64 and 700 points; every class has one entry, so the draw is known."""
    rng = np.random.default_rng(sum(map(ord, name)))
    Cp, D, e, extra = 4, 7, 0.0, ()
    far = [box(4 + 8 * i, -15.0) for i in range(4)]      # disjoint axis-aligned boxes
    gt_rows, gt_labs = [[], [], []], [[], [], []]
    snum = None
    if name == "all_collide":
        ent = [(far[i], i, OBJ_N[i]) for i in range(4)]
        for b in range(3):
            gt_rows[b], gt_labs[b] = [box(20, 0, 0, 1000.0, 1000.0, 4.0, 0.3)], [3]
        snum = [1, 1, 1, 2]                              # (class 3 holds one box already: one of its two slots is active)
    elif name == "none_collide":
        ent = [(far[i], i, OBJ_N[i]) for i in range(4)]
    elif name == "chain":                                # a - b - c: a and c are disjoint, b overlaps both
        ent = [(box(10, 0), 0, 64), (box(13, 0.5), 1, 130), (box(16, 0), 2, 1)]
    elif name == "shared_edge":                          # the candidate's x = 12 face is the ground-truth box's
        ent = [(box(10, 0), 0, 64), (far[3], 1, 1)]
        for b in range(3):
            gt_rows[b], gt_labs[b] = [box(14, 0)], [1]
        snum = [1, 2]
    elif name == "twice":                                # one entry, two slots
        ent = [(box(10, 0), 0, 64), (far[2], 1, 130)]
        snum = [2, 2]
    elif name == "padding_gt":                           # padding rows on top of the candidate: no obstacle, not counted
        ent = [(box(10, 0), 0, 64), (far[2], 1, 1)]
        for b in range(3):
            gt_rows[b] = [box(10, 0), box(10, 0, l=0.0), box(10, 0, h=-1.0)]
            gt_labs[b] = [-1, 0, 5]
        snum = [1, 1]
    elif name == "quota_met":                            # class 0 already has its two boxes, class 1 has one of two
        ent = [(box(10, 0), 0, 64), (far[2], 1, 130)]
        for b in range(3):
            gt_rows[b], gt_labs[b] = [box(30, 10), box(30, 15), box(20, 15)], [0, 0, 1]
        snum = [2, 2]
    elif name == "empty_class":                          # class 1 has no entry
        ent = [(box(10, 0), 0, 64), (far[2], 2, 1)]
        snum = [1, 3, 1]
    elif name in ("faces", "extra_width"):               # scene points on the faces of the accepted box at (20, 10, 0)
        ent = [(box(20, 10), 0, 64), (far[0], 1, 0)]
        snum = [1, 1]
        on = [(22, 10, 0), (18, 10.5, 0.5), (20, 11, 0), (20, 9, -1), (20, 10, 1), (21, 10.5, -1), (20, 10, 0), (22.25, 10, 0), (20, 11.5, 1.5),
              (22.5, 10, 0), (20, 10, 1.5)]
        extra = ((1, on), (2, on))
        e = 0.5 if name == "extra_width" else 0.0
    else:
        raise KeyError(name)
    C = max(k for _, k, _ in ent) + 1
    pts, off = scenes(rng, Cp, SCENE_N, extra)
    G = max(len(r) for r in gt_rows)
    gb, gl = pad_gt(gt_rows, gt_labs, G, D)
    return dict(points=pts, offsets=off, gt_boxes=gb, gt_labels=gl, db=make_db(rng, ent, C, Cp), sample_num=snum or [1] * C, Pmax=130,
                seed=call_seed(7, 0), seed_step=(7, 0), e=e)


GENERAL = {
    "q20_c4_d7_g6": (4, 7, 6, (8, 7, 5), 64, 11),
    "q20_c5_d9_g1": (5, 9, 1, (8, 7, 5), 63, 12),
    "q20_c4_d9_g0": (4, 9, 0, (8, 7, 5), 65, 13),
    "q70_c5_d7_g6": (5, 7, 6, (40, 26, 4), 64, 14),
}
SPECIAL = ("all_collide", "none_collide", "chain", "shared_edge", "twice", "padding_gt", "quota_met", "empty_class", "faces", "extra_width")
CASES = tuple(GENERAL) + SPECIAL


@functools.lru_cache(maxsize=None)
def case(name):
    c = _general(*GENERAL[name]) if name in GENERAL else _special(name)
    for v in (c["points"], c["offsets"], c["gt_boxes"], c["gt_labels"], *[a for a in c["db"].values() if isinstance(a, np.ndarray)]):
        v.setflags(write=False)
    return c
