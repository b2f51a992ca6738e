"""Time of one training step of ``SADDetectorTrain`` (SPEC.md §33) on one GPU -> profiles/train_step_time.json

A step = ``zero_grad``, ``forward``, ``targets``, ``loss(...).sum()``, ``backward`` on one resident batch with every parameter
trainable (single stream, eager; no optimizer).  Measured for

  * KITTI  ``config.KITTI`` on ``synth.make_batch`` scenes with their ``synth.scene_boxes``, at the largest batch of
           ``--batches`` (tried from the largest down; the default starts at 32, the benchmark's batch) whose step runs
           without an out-of-memory error
  * TINY   ``config.TINY`` on ``synth.make_tiny_batch`` scenes, batch ``--tiny-batch``

Beside each step time: the inference forward of the same batch (``SADDetector`` on the exported weights, eager ``forward``,
``use_plans=False``) and ``torch.cuda.max_memory_allocated`` over the training steps.

Method: four warm-up steps of each form (the last three timed on the host to size the windows), then ``--repeats`` rounds in which the two forms alternate; each round times, with
device events, as many back-to-back calls as fill ``--seconds``; median and min..max per form.  The
host synchronises only at the end of a window.
    python tools/train_step_time.py [--batches 32,16,8,4,2,1] [--tiny-batch 8] [--seconds 1.5] [--repeats 5]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="32,16,8,4,2,1")
    ap.add_argument("--tiny-batch", type=int, default=8)
    ap.add_argument("--seconds", type=float, default=1.5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "train_step_time.json"))
    a = ap.parse_args()
    import sad_amd  # noqa: F401
    import torch
    from sad_amd import config, synth
    from sad_amd.detector import SADDetector
    from sad_amd.detector_train import SADDetectorTrain
    if not torch.cuda.is_available():
        raise SystemExit("train_step_time: needs a GPU (a time taken elsewhere says nothing)")
    dev = torch.device("cuda:0")

    def window(fn, iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / iters

    def measure(name, cfg, pts_np, gt_np):
        B = pts_np.shape[0]
        pts, gt = torch.from_numpy(pts_np).to(dev), torch.from_numpy(gt_np).to(dev)
        labels = torch.zeros(gt_np.shape[:2], dtype=torch.int32, device=dev)
        det = SADDetectorTrain(cfg, dev, seed=0)
        det.requires_grad_(True)
        state = {}

        def step():
            det.zero_grad(set_to_none=True)
            out = det(pts)
            loss = det.loss(out, det.targets(out, gt, labels)).sum()
            loss.backward()
            state["loss"] = loss.detach()

        torch.cuda.reset_peak_memory_stats(dev)
        step()                                     # (the first call loads code objects and fills the allocator: not counted)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(3):
            step()
        torch.cuda.synchronize()
        warm_s = (time.perf_counter() - t0) / 3
        inf = SADDetector(cfg, det.export(), dev)
        inf.use_plans = False

        def infer():
            with torch.no_grad():
                return inf(pts)

        infer()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(3):
            infer()
        torch.cuda.synchronize()
        warm_i = (time.perf_counter() - t0) / 3
        it_s, it_i = max(3, int(a.seconds / max(warm_s, 1e-4))), max(3, int(a.seconds / max(warm_i, 1e-4)))
        ts, ti = [], []
        for _ in range(a.repeats):
            ts.append(window(step, it_s))
            ti.append(window(infer, it_i))
        peak = torch.cuda.max_memory_allocated(dev)
        ts.sort()
        ti.sort()
        return {"config": name, "B": B, "n_points": cfg.n_points, "num_pos": int(det.num_pos.sum()), "loss": round(float(state["loss"]), 4),
                "train_step_ms": round(ts[len(ts) // 2], 3), "train_step_min_ms": round(ts[0], 3), "train_step_max_ms": round(ts[-1], 3),
                "train_iters_per_window": it_s,
                "infer_forward_ms": round(ti[len(ti) // 2], 3), "infer_forward_min_ms": round(ti[0], 3), "infer_forward_max_ms": round(ti[-1], 3),
                "infer_iters_per_window": it_i, "step_over_forward": round(ts[len(ts) // 2] / ti[len(ti) // 2], 2),
                "max_memory_allocated_MiB": round(peak / 2 ** 20, 1), "repeats": a.repeats}

    rows = []
    tried = []
    for B in [int(v) for v in a.batches.split(",")]:
        try:
            pts = synth.make_batch(0, B, config.KITTI.n_points)
            gt = np.stack([synth.scene_boxes(i, config.KITTI.n_points) for i in range(B)], 0)
            row = measure("KITTI", config.KITTI, pts, gt)
            row["batches_that_did_not_fit"] = tried
            rows.append(row)
            break
        except torch.cuda.OutOfMemoryError:
            tried.append(B)
            torch.cuda.empty_cache()
    else:
        rows.append({"config": "KITTI", "error": f"no batch of {a.batches} fits"})
    print(json.dumps(rows[-1]), flush=True)
    torch.cuda.empty_cache()
    cfg = config.TINY
    B = a.tiny_batch
    gt = np.stack([synth.scene_boxes(i, cfg.n_points, extent=(0.0, 20.0, -10.0, 10.0), n_boxes=6) for i in range(B)], 0)
    rows.append(measure("TINY", cfg, synth.make_tiny_batch(0, B, cfg.n_points), gt))
    print(json.dumps(rows[-1]), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(rows, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
