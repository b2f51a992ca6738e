"""Box-operator timings (SPEC.md §19): points_in_boxes, roipoint_pool3d and the pairwise BEV / 3-D IoU at the detector's
K = 256 boxes per scene, B = 32, on KITTI-shaped (N = 16 384) and nuScenes-shaped (N = 65 536) synthetic scenes.  The boxes
of a scene are its 40 ground-truth boxes plus 216 detector-like car boxes centred on scene points.  Prints ONE JSON line.

    python tools/box_bench.py [--out FILE]

The parent process never touches the GPU.  It runs (each in a child process under its own `timeout`):
  1. `box_bench.py --child`: device-event timings after warm-up, and torch compositions of the same results for context;
  2. per shape, `rocprofv3 --kernel-trace --stats -- box_bench.py --child --shape i`: the kernel times;
  3. `rocprofv3 --pmc SQ_INSTS_VALU SQ_WAVES -- box_bench.py --child --iou-only`: VALU instructions per IoU pair.
Bounds: points_in_boxes at PIB_OPS VALU operations per point-box pair (the §19.1 predicate) and 78.65 T lane-ops/s;
roipoint_pool3d at the larger of that scan bound over all (box, point) pairs and its output bytes at 8.0 TB/s; the IoU at
its measured VALU instructions per pair (one pair per lane) at the same issue rate.
"""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [("kitti", 16384), ("nuscenes", 65536)]
B, K, E = 32, 256, 1.0
POOL = [(128, 1), (128, 128), (512, 1), (512, 128)]       # (S, C)
VALU_OPS_PER_S = 157.3e12 / 2          # wave-lane f32 operations per second (an FMA counts as two flops)
HBM_BPS = 8.0e12
PIB_OPS = 14                           # 3 differences, 4 products, 2 sums, 3 compares, 2 ands per (point, box) pair
KERNELS = {"points_in_boxes_kernel": "points_in_boxes", "roipoint_pool3d_kernel<1>": "roipoint_pool3d",
           "roipoint_pool3d_kernel<4>": "roipoint_pool3d_vec4", "boxes_iou_kernel": "boxes_iou"}


def scenes(n):
    """xyz [B,n,3], intensity [B,n,1], boxes [B,K,7] (numpy)."""
    import numpy as np
    from sad_amd import synth
    kw = {} if n == 16384 else {"extent": (-51.2, 51.2, -51.2, 51.2), "n_boxes": 160}
    rng = np.random.default_rng(n)
    pts, bxs = [], []
    for i in range(B):
        sc = synth.make_scene(i, n, **kw)
        gt = synth.scene_boxes(i, n, **kw)[:40]
        more = np.zeros((K - len(gt), 7), np.float32)
        more[:, 0:3] = sc[rng.integers(0, n, K - len(gt)), :3]
        more[:, 3:6] = (3.9, 1.6, 1.56)
        more[:, 6] = rng.uniform(-np.pi, np.pi, K - len(gt))
        pts.append(sc)
        bxs.append(np.concatenate([gt, more]))
    pts = np.stack(pts)
    return np.ascontiguousarray(pts[..., :3]), np.ascontiguousarray(pts[..., 3:]), np.stack(bxs).astype(np.float32)


def child(shape_ids, iters, with_torch, iou_only):
    sys.path.insert(0, ROOT)
    import sad_amd  # noqa: F401  (before torch: the package owns GPU_MAX_HW_QUEUES)
    import torch
    from sad_amd import ops
    dev = torch.device("cuda:0")

    def timed(fn, n=iters, warm=3):
        for _ in range(warm):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / n

    res = {}
    for si in shape_ids:
        name, n = SHAPES[si]
        xyz_np, inten_np, boxes_np = scenes(n)
        xyz, boxes = torch.from_numpy(xyz_np).to(dev), torch.from_numpy(boxes_np).to(dev)
        r = {}
        r["boxes_iou_bev"] = timed(lambda: ops.boxes_iou_bev(boxes, boxes))
        r["boxes_iou3d"] = timed(lambda: ops.boxes_iou3d(boxes, boxes))
        if iou_only:
            res[name] = r
            continue
        r["points_in_boxes"] = timed(lambda: ops.points_in_boxes(xyz, boxes))
        g = torch.Generator(device=dev).manual_seed(si)
        for S, C in POOL:
            feat = torch.from_numpy(inten_np).to(dev) if C == 1 else torch.randn((B, n, C), device=dev, generator=g)
            r[f"roipoint_pool3d_S{S}_C{C}"] = timed(lambda: ops.roipoint_pool3d(xyz, feat, boxes, E, S), n=max(3, iters // 4))
            if with_torch and S == 512 and C == 128:      # context: the composition a torch code base writes (mask + cumsum + gather)
                def torch_pool():
                    c, s_ = torch.cos(boxes[..., 6]), torch.sin(boxes[..., 6])
                    d = xyz[:, None, :, :] - boxes[:, :, None, 0:3]                          # [B,K,N,3]
                    lx = d[..., 0] * c[..., None] + d[..., 1] * s_[..., None]
                    ly = d[..., 1] * c[..., None] - d[..., 0] * s_[..., None]
                    m = ((d[..., 2].abs() <= 0.5 * (boxes[..., 5:6] + 2 * E)) & (lx.abs() < 0.5 * (boxes[..., 3:4] + 2 * E))
                         & (ly.abs() < 0.5 * (boxes[..., 4:5] + 2 * E)))
                    cnt = m.sum(-1)
                    order = torch.argsort((~m).to(torch.int8), dim=-1, stable=True)[..., :S]   # inside points first, ascending n
                    slot = torch.arange(S, device=dev) % cnt.clamp(min=1)[..., None]
                    j = torch.gather(order, 2, slot)
                    rows = torch.cat([xyz, feat], 2)
                    out = rows[torch.arange(B, device=dev)[:, None, None], j]
                    return out * (cnt > 0)[..., None, None]
                r["torch_mask_sort_gather_S512_C128"] = timed(torch_pool, n=2, warm=1)
            del feat
        if with_torch:
            def torch_pib():
                c, s_ = torch.cos(boxes[..., 6]), torch.sin(boxes[..., 6])
                d = xyz[:, :, None, :] - boxes[:, None, :, 0:3]                              # [B,N,K,3]
                lx = d[..., 0] * c[:, None] + d[..., 1] * s_[:, None]
                ly = d[..., 1] * c[:, None] - d[..., 0] * s_[:, None]
                m = (d[..., 2].abs() <= 0.5 * boxes[:, None, :, 5]) & (lx.abs() < 0.5 * boxes[:, None, :, 3]) & (ly.abs() < 0.5 * boxes[:, None, :, 4])
                first = torch.argmax(m.to(torch.int8), dim=2)
                return torch.where(m.any(2), first, -1)
            r["torch_points_in_boxes"] = timed(torch_pib, n=3, warm=1)
        res[name] = r
        del xyz, boxes
        torch.cuda.empty_cache()
    print("BOX_CHILD " + json.dumps(res), flush=True)


def _run(cmd, tmo):
    p = subprocess.run(["timeout", "-k", "10", str(tmo)] + cmd, cwd=ROOT, capture_output=True, text=True)
    if p.returncode != 0:
        sys.stderr.write(p.stdout[-2000:] + p.stderr[-2000:])
        raise SystemExit(f"step failed ({p.returncode}): {' '.join(cmd[:3])} ...")
    return p.stdout


def kernel_stats(si, workdir):
    d = os.path.join(workdir, f"prof{si}")
    _run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--",
          sys.executable, os.path.abspath(__file__), "--child", "--shape", str(si), "--iters", "8", "--no-torch"], 400)
    files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
    out = {}
    for f in files:
        for row in csv.DictReader(open(f)):
            for frag, label in KERNELS.items():
                if frag in row["Name"].replace(" ", ""):
                    out[label] = round(float(row["AverageNs"]) / 1e3, 2)
    return out


def iou_valu_per_pair(workdir):
    """VALU instructions per IoU pair (both modes), from SQ_INSTS_VALU / SQ_WAVES of boxes_iou_kernel (64 pairs per wave)."""
    d = os.path.join(workdir, "pmc")
    _run(["rocprofv3", "--pmc", "SQ_INSTS_VALU", "SQ_WAVES", "--output-format", "csv", "-d", d, "--",
          sys.executable, os.path.abspath(__file__), "--child", "--shape", "0", "--iters", "1", "--no-torch", "--iou-only"], 400)
    tot = {}
    for f in glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True):
        for row in csv.DictReader(open(f)):
            if "boxes_iou_kernel" in row.get("Kernel_Name", ""):
                tot[row["Counter_Name"]] = tot.get(row["Counter_Name"], 0.0) + float(row["Counter_Value"])
    if not tot.get("SQ_WAVES"):
        return None
    return round(tot["SQ_INSTS_VALU"] / tot["SQ_WAVES"], 1)     # per wave = per lane's pair (waves run 64 pairs in lockstep)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--shape", type=int, default=None)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--no-prof", action="store_true")
    ap.add_argument("--iou-only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.child:
        child([a.shape] if a.shape is not None else list(range(len(SHAPES))), a.iters, not a.no_torch, a.iou_only)
        return
    line = [ln for ln in _run([sys.executable, os.path.abspath(__file__), "--child"], 560).splitlines() if ln.startswith("BOX_CHILD ")]
    events = json.loads(line[-1][len("BOX_CHILD "):])
    kern, ipp = {}, None
    if not a.no_prof:
        with tempfile.TemporaryDirectory() as wd:
            for si, (name, _) in enumerate(SHAPES):
                kern[name] = kernel_stats(si, wd)
            ipp = iou_valu_per_pair(wd)
    result = {"B": B, "K": K, "extra_width": E,
              "bounds": {"points_in_boxes": f"VALU ({PIB_OPS} ops/pair at 78.65 T lane-ops/s)",
                         "roipoint_pool3d": "max(scan over all B*K*N pairs at the points_in_boxes rate, output bytes at 8.0 TB/s)",
                         "boxes_iou": "measured VALU instructions per pair (SQ_INSTS_VALU / SQ_WAVES) at 78.65 T lane-ops/s"},
              "iou_valu_instructions_per_pair": ipp, "shapes": {}}
    for name, n in SHAPES:
        ev, kt = events[name], kern.get(name, {})
        pairs = B * K * n
        bound = {"points_in_boxes": pairs * PIB_OPS / VALU_OPS_PER_S * 1e6}
        for S, C in POOL:
            bound[f"roipoint_pool3d_S{S}_C{C}"] = max(pairs * PIB_OPS / VALU_OPS_PER_S, B * K * S * (3 + C) * 4 / HBM_BPS) * 1e6
        if ipp:
            bound["boxes_iou_bev"] = bound["boxes_iou3d"] = B * K * K * ipp / VALU_OPS_PER_S * 1e6
        s = {"events_us": {k: round(v, 2) for k, v in ev.items()}, "kernel_us": kt,
             "bound_us": {k: round(v, 2) for k, v in bound.items()}, "fraction_of_bound": {}}
        for label, t in ev.items():
            if label in bound and t:
                # the kernel time where one kernel makes the op (points_in_boxes), else the event time
                kt_label = kt.get("points_in_boxes") if label == "points_in_boxes" else None
                s["fraction_of_bound"][label] = round(bound[label] / (kt_label or t), 3)
        result["shapes"][name] = s
    txt = json.dumps(result)
    if a.out:
        with open(a.out, "w") as f:
            f.write(txt + "\n")
    print(txt)


if __name__ == "__main__":
    main()
