"""Voxel RoI pooling timings (SPEC.md §30) at Voxel R-CNN's KITTI shape: B = 2 scenes, R = 128 RoIs, G = 6 (55 296 grid points),
three backbone scales (strides 2 / 4 / 8 of the 0.05 x 0.05 x 0.1 m grid) of a synthetic scene with about 60 k / 30 k / 12 k
voxels, max_range 4, S = 16, radii 0.4 / 0.8 / 1.6 m, channels 32 / 64 / 64 -> [32, 32].  Prints ONE JSON line.

    python tools/voxel_roi_bench.py [--out FILE] [--iters N]

Device-event timings after warm-up of `voxel_query` alone (per scale: table build + query, three launches) and of the whole
`VoxelRoIPool.forward` (inference path).  Next to them, what the query kernel issues, counted by a framework restatement of its
walk on the same inputs (a dense occupancy volume per scale, every candidate of every query, the 64-candidate steps that are
reached before S are accepted): the table probes (`find` calls: candidates inside the grid in the steps that are walked), the
probes a walk without the early exit would issue, and the bytes of idx written; the restatement's cnt is checked against the
kernel's.  These are the first numbers of their kind: nothing comparable existed before the operator."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, R, G, S, RANGE = 2, 128, 6, 16, (4, 4, 4)
POINT_RANGE = (0.0, -40.0, -3.0, 70.4, 40.0, 1.0)
BASE_VOXEL, BASE_SHAPE = (0.05, 0.05, 0.1), (41, 1600, 1408)
SCALES = [dict(stride=2, radius=0.4, channels=32), dict(stride=4, radius=0.8, channels=64), dict(stride=8, radius=1.6, channels=64)]


def scene(seed=0):
    """-> ([(coors [Nv,3] int32, offsets [B+1] int32, shape, voxel_size)] per scale, rois [B,R,7]).  The stride-8 scale is a rough
    ground sheet with 40 car-sized blobs per scene (about 6 k cells a scene); every finer scale keeps about 2.5 (stride 4) / 2 (stride 2) of the 8
    children of each of its parent's cells (at least one), so the scales nest as a backbone's do; the RoIs sit on the blobs."""
    import numpy as np
    rng = np.random.default_rng(seed)
    shapes = [BASE_SHAPE]
    for _ in range(3):
        shapes.append(tuple((g + 1) // 2 for g in shapes[-1]))
    shapes = shapes[1:]                                  # strides 2, 4, 8
    per_scale, rois = [[], [], []], []
    kids = np.array([[z, y, x] for z in (0, 1) for y in (0, 1) for x in (0, 1)])
    for b in range(B):
        shape, n = shapes[2], 6400
        gx, gy = rng.integers(0, shape[2], n), rng.integers(0, shape[1], n)
        gz = np.clip(rng.normal(1.6, 0.5, n).round().astype(np.int64), 0, shape[0] - 1)
        cars = rng.integers(0, 40, n // 3)
        cx, cy = rng.integers(10, shape[2] - 10, 40), rng.integers(10, shape[1] - 10, 40)
        gx[:n // 3] = np.clip(cx[cars] + rng.normal(0, 2.5, n // 3).round().astype(np.int64), 0, shape[2] - 1)
        gy[:n // 3] = np.clip(cy[cars] + rng.normal(0, 2.5, n // 3).round().astype(np.int64), 0, shape[1] - 1)
        gz[:n // 3] = rng.integers(1, 4, n // 3)
        c = np.stack([gz, gy, gx], 1)
        for k in (2, 1, 0):
            shape = shapes[k]
            if k < 2:
                keep = rng.uniform(size=(len(c), 8)) < (0.22, 0.15)[1 - k]
                keep[np.arange(len(c)), rng.integers(0, 8, len(c))] = True
                c = (2 * c[:, None, :] + kids[None])[keep]
                c = c[(c < np.asarray(shape)).all(1)]
            _, first = np.unique((c[:, 0] * shape[1] + c[:, 1]) * shape[2] + c[:, 2], return_index=True)
            c = c[np.sort(first)]
            per_scale[k].append(c)
        box = np.zeros((R, 7), np.float32)
        pick = rng.integers(0, 40, R)
        box[:, 0] = (cx[pick] + rng.normal(0, 2.0, R)) * 0.4
        box[:, 1] = (cy[pick] + rng.normal(0, 2.0, R)) * 0.4 - 40.0
        box[:, 2] = -1.0 + rng.normal(0, 0.2, R)
        box[:, 3:6] = (3.9, 1.6, 1.56)
        box[:, 6] = rng.uniform(-np.pi, np.pi, R)
        rois.append(box)
    levels = []
    for k, s in enumerate(SCALES):
        offsets = np.concatenate([[0], np.cumsum([len(c) for c in per_scale[k]])]).astype(np.int32)
        levels.append((np.concatenate(per_scale[k]).astype(np.int32), offsets, shapes[k], tuple(v * s["stride"] for v in BASE_VOXEL)))
    return levels, np.stack(rois)


def walk_counts(torch, coors, offsets, shape, vs, pts, radius, cnt):
    """The walk of voxel_query_kernel restated with framework operations -> (probes issued, probes without the early exit)."""
    dev = pts.device
    occ = torch.zeros((B,) + tuple(shape), dtype=torch.bool, device=dev)
    scene_of = torch.repeat_interleave(torch.arange(B, device=dev), (offsets[1:] - offsets[:-1]).long())
    occ[scene_of, coors[:, 0].long(), coors[:, 1].long(), coors[:, 2].long()] = True
    v = torch.tensor(vs, dtype=torch.float32, device=dev)
    lo = torch.tensor(POINT_RANGE[:3], dtype=torch.float32, device=dev)
    half = torch.tensor(0.5, device=dev) * v + lo
    p = pts.reshape(B, -1, 3)
    q = torch.floor((p - lo) / v)
    assert bool((q.abs() < 2.0 ** 30).all())
    q = q.long()
    n = 2 * RANGE[0] + 1
    d = torch.arange(n, device=dev) - RANGE[0]
    dz, dy, dx = torch.meshgrid(d, d, d, indexing="ij")
    off = torch.stack([dx.reshape(-1), dy.reshape(-1), dz.reshape(-1)], 1)           # [T,3] (x,y,z) in walk order
    r2 = torch.tensor(radius, dtype=torch.float32, device=dev) * torch.tensor(radius, dtype=torch.float32, device=dev)
    issued = total = 0
    lim = torch.tensor([shape[2], shape[1], shape[0]], device=dev)
    for b in range(B):
        cell = q[b][:, None, :] + off[None]                                           # [M,T,3]
        inside = ((cell >= 0) & (cell < lim)).all(-1)
        cc = torch.minimum(cell.clamp(min=0), lim - 1)
        ctr = cc.to(torch.float32) * v + half
        t = ctr - p[b][:, None, :]
        t = t * t
        ok = inside & occ[b][cc[..., 2], cc[..., 1], cc[..., 0]] & (((t[..., 0] + t[..., 1]) + t[..., 2]) < r2)
        T = off.shape[0]
        pad = (-T) % 64
        okp = torch.nn.functional.pad(ok, (0, pad)).reshape(ok.shape[0], -1, 64)
        inp = torch.nn.functional.pad(inside, (0, pad)).reshape(ok.shape[0], -1, 64)
        before = okp.sum(-1).cumsum(-1) - okp.sum(-1)                                 # accepted before each step
        walked = before < S
        issued += int((inp.sum(-1) * walked).sum())
        total += int(inside.sum())
        assert torch.equal(ok.sum(-1).clamp(max=S).to(torch.int32), cnt[b]), "the restatement and the kernel disagree on cnt"
    return issued, total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--iters", type=int, default=200)
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import numpy as np
    import sad_amd  # noqa: F401  (before torch: the package owns GPU_MAX_HW_QUEUES)
    import torch
    from sad_amd import ops, SparseTensor, VoxelRoIPool
    assert torch.cuda.is_available(), "this benchmark needs a GPU"
    dev = torch.device("cuda:0")
    levels, rois = scene()
    rng = np.random.default_rng(1)
    tensors = [SparseTensor(torch.from_numpy(rng.normal(size=(len(c), s["channels"])).astype(np.float32)).to(dev), torch.from_numpy(c).to(dev),
                            torch.from_numpy(o).to(dev), shape) for (c, o, shape, _), s in zip(levels, SCALES)]
    pool = VoxelRoIPool(G, [dict(in_channels=s["channels"], voxel_size=lv[3], max_range=RANGE, radius=s["radius"], nsample=S, mlp=[32, 32])
                            for s, lv in zip(SCALES, levels)], POINT_RANGE).to(dev)
    rois_t = torch.from_numpy(rois).to(dev)
    pts = ops.roi_grid_points(rois_t, None, G).view(B, R * G ** 3, 3)

    def timed(fn):
        for _ in range(20):
            fn()
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(a.iters):
            fn()
        t1.record()
        torch.cuda.synchronize()
        return round(t0.elapsed_time(t1) * 1000.0 / a.iters, 2)

    res = {"B": B, "R": R, "G": G, "S": S, "max_range": RANGE, "grid_points": B * R * G ** 3, "iters": a.iters, "scales": []}
    for t, s, lv in zip(tensors, SCALES, levels):
        kw = dict(max_range=RANGE, radius=s["radius"], S=S)
        out = ops.voxel_query(t.coors, t.offsets, t.spatial_shape, lv[3], POINT_RANGE, pts, **kw)
        ws = ops.voxel_query_workspace(t.coors.shape[0], dev)
        us = timed(lambda: ops.voxel_query(t.coors, t.offsets, t.spatial_shape, lv[3], POINT_RANGE, pts, out=out, workspace=ws, **kw))
        issued, total = walk_counts(torch, t.coors, t.offsets, t.spatial_shape, lv[3], pts, s["radius"], out[1])
        res["scales"].append({"stride": s["stride"], "voxels": int(t.coors.shape[0]), "spatial_shape": list(t.spatial_shape), "radius": s["radius"],
                              "voxel_query_us": us, "probes_issued": issued, "probes_without_early_exit": total,
                              "candidates": B * R * G ** 3 * (2 * RANGE[0] + 1) ** 3, "idx_bytes": B * R * G ** 3 * S * 4,
                              "mean_cnt": round(float(out[1].float().mean()), 2), "full_groups": round(float((out[1] == S).float().mean()), 3)})
    res["voxel_query_us_total"] = round(sum(s["voxel_query_us"] for s in res["scales"]), 2)
    res["roi_grid_points_us"] = timed(lambda: ops.roi_grid_points(rois_t, None, G))
    with torch.no_grad():
        res["forward_us"] = timed(lambda: pool(rois_t, None, tensors))
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
