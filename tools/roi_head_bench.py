"""RoI head timings (SPEC.md §28) -> profiles/roi_head_bench.json, at a training shape: B = 8 scenes, R = 512 RoIs, G = 64 boxes
per scene (the last 8 padding), S = 128 slots, roi_labels given (matching per class), roi_count given.

  (a) roi_targets  ops.roi_targets into kept outputs and a kept workspace (both launches)
  (b) roi_decode   ops.roi_decode on the sampled RoIs and their targets
  (c) copy         a plain device copy that moves (a)'s compulsory traffic (RoIs and ground truth read once + outputs written
                   once; the copy reads half of those bytes and writes half)

Method: as tools/dense_target_bench.py.  Warm-up, then REPEATS rounds in which the forms ALTERNATE, each timed by HIP events
around ITERS back-to-back calls; median and min..max per form.  call_us = the calls issued on an idle stream (the host's cost of a
call); us = the same calls queued BEHIND blocker copies that outlast the host's issuing (checked: host_ahead), so the events
bracket device time only.  The RoIs are jittered copies of the boxes: a third each near (fg), shifted (hard) and far (easy).
    python tools/roi_head_bench.py [--iters 50] [--repeats 9]"""
import argparse
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def scene(rng, B, R, G):
    gt = np.zeros((B, G, 7), np.float64)
    gt[..., 0], gt[..., 1] = rng.uniform(0, 70.4, (B, G)), rng.uniform(-40, 40, (B, G))
    gt[..., 2] = rng.uniform(-2, 0, (B, G))
    gt[..., 3:6] = np.array([3.9, 1.6, 1.56]) * rng.uniform(0.8, 1.2, (B, G, 3))
    gt[..., 6] = rng.uniform(-math.pi, math.pi, (B, G))
    lab = rng.integers(0, 3, (B, G)).astype(np.int32)
    lab[:, G - 8:] = -1
    src = rng.integers(0, G - 8, (B, R))
    rois = np.take_along_axis(gt, src[..., None], 1)
    kind = rng.integers(0, 3, (B, R))
    along = np.stack([np.cos(rois[..., 6]), np.sin(rois[..., 6])], -1)
    shift = np.where(kind == 0, rng.uniform(-0.03, 0.03, (B, R)), np.where(kind == 1, rng.uniform(0.35, 0.7, (B, R)), rng.uniform(0.9, 3.0, (B, R))))
    rois[..., :2] += along * (rois[..., 3] * shift)[..., None]
    rois[..., 6] += rng.uniform(-0.03, 0.03, (B, R))
    return rois.astype(np.float32), np.take_along_axis(lab, src, 1), gt.astype(np.float32), lab


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "roi_head_bench.json"))
    a = ap.parse_args()
    import sad_amd  # noqa: F401
    import torch
    from sad_amd import ops
    dev = torch.device("cuda:0")
    B, R, G, S = 8, 512, 64, 128
    rois_np, rl_np, gt_np, lab_np = scene(np.random.default_rng(0), B, R, G)
    rois, rl, gt, lab = (torch.from_numpy(v).to(dev) for v in (rois_np, rl_np, gt_np, lab_np))
    count = torch.full((B,), R - 12, dtype=torch.int32, device=dev)
    kw = dict(S=S, fg_max=S // 2, fg_thr=0.55, bg_lo=0.1, hard_ratio=0.8, reg_fg_thr=0.55, cls_fg_thr=0.75, cls_bg_thr=0.25, seed=1)
    out = ops.roi_targets(rois, count, rl, gt, lab, **kw)
    ws = ops.roi_targets_workspace(B, R, dev)
    boxes = torch.empty((B, S, 7), device=dev)

    blk_src = torch.empty(256 * 1024 * 1024, dtype=torch.float32, device=dev).normal_()      # 1 GiB
    blk_dst = torch.empty_like(blk_src)

    def span(fn, iters, head_start_us=0.0):
        """us per call of `iters` calls between two events; with a head start, behind that many us of blocker copies."""
        for _ in range(int(math.ceil(head_start_us / blk_us)) if head_start_us else 0):
            blk_dst.copy_(blk_src)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        ahead = not e0.query()                                # the device has not reached e0: the host was ahead throughout
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / iters, ahead

    for _ in range(2):
        blk_dst.copy_(blk_src)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(4):
        blk_dst.copy_(blk_src)
    e1.record()
    torch.cuda.synchronize()
    blk_us = e0.elapsed_time(e1) * 1e3 / 4

    traffic = B * R * 8 * 4 + B * 4 + B * G * 8 * 4 + B * S * (6 + 21) * 4
    src = torch.empty(max(traffic // 8, 1), dtype=torch.float32, device=dev).normal_()
    dst = torch.empty_like(src)
    forms = {"roi_targets": lambda: ops.roi_targets(rois, count, rl, gt, lab, out=out, workspace=ws, **kw),
             "roi_decode": lambda: ops.roi_decode(out[6], out[8], out=boxes),
             "copy": lambda: dst.copy_(src)}
    for fn in forms.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    call, devt, ok = {k: [] for k in forms}, {k: [] for k in forms}, {k: True for k in forms}
    for _ in range(a.repeats):
        for k, fn in forms.items():                           # alternate the forms
            call[k].append(span(fn, a.iters)[0])
        for k, fn in forms.items():
            t, ahead = span(fn, a.iters, 1.5 * call[k][-1] * a.iters + 500.0)
            devt[k].append(t)
            ok[k] = ok[k] and ahead
    index, match = out[0].cpu().numpy(), out[1].cpu().numpy()
    rec = dict(B=B, R=R, G=G, S=S, candidates=R - 12, traffic_bytes=traffic, pairs=int(B * (R - 12) * (G - 8)),
               matched_slots=int((match >= 0).sum()), distinct_rois=int(sum(len(set(r)) for r in index)))
    for k in forms:
        c, d = sorted(call[k]), sorted(devt[k])
        rec[k] = {"us": round(d[len(d) // 2], 1), "min_us": round(d[0], 1), "max_us": round(d[-1], 1), "host_ahead": ok[k],
                  "call_us": round(c[len(c) // 2], 1), "iters": a.iters}
    print(json.dumps(rec), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
