"""Rotated IoU loss timings (SPEC.md §34) -> profiles/iou_loss_bench.json, at N = 2 x 128 pairs (the RoI head's shape),
N = 32 x 256 and N = 65 536: perturbed copies of seeded boxes, mode "3d", kind "diou" (the form with the most arithmetic).

  (a) launch   ops.rotated_iou_loss into kept outputs: loss, iou AND the gradient, one launch
  (b) module   forward and backward through RotatedIoULoss(reduction="sum") on a leaf that requires a gradient: the launch, the
               sum, and autograd's multiply by the incoming gradient

There is no plain-torch differentiable rotated IoU here to compare with: the numbers are the first of their kind, no baseline.

Method: warm-up, then REPEATS rounds in which the forms ALTERNATE, each timed by HIP events around ITERS back-to-back steps that
end in a device synchronise; median and min..max of the time per step.  At these sizes the step is bound by launches and by the
host, not by the device: the figure is the time of a training step's loss, not a kernel's share of peak.
    python tools/iou_loss_bench.py [--iters 1000] [--repeats 9]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = ((2, 128), (32, 256), (256, 256))


def pairs(rng, B, S):
    """pred, target [B,S,7] f32: targets of everyday sizes, preds their perturbed copies (shift up to 0.5 m, yaw +-0.3, sizes +-10 %)."""
    t = np.zeros((B, S, 7), np.float64)
    t[..., 0:2] = rng.uniform(-40, 40, (B, S, 2))
    t[..., 2] = rng.uniform(-2, 1, (B, S))
    t[..., 3:6] = rng.uniform((1.5, 0.6, 1.0), (6.0, 2.5, 2.5), (B, S, 3))
    t[..., 6] = rng.uniform(-np.pi, np.pi, (B, S))
    p = t.copy()
    p[..., 0:3] += rng.uniform(-0.5, 0.5, (B, S, 3))
    p[..., 3:6] *= rng.uniform(0.9, 1.1, (B, S, 3))
    p[..., 6] += rng.uniform(-0.3, 0.3, (B, S))
    return p.astype(np.float32), t.astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=1000)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "iou_loss_bench.json"))
    a = ap.parse_args()
    import sad_amd  # noqa: F401
    import torch
    from sad_amd import RotatedIoULoss, ops
    dev = torch.device("cuda:0")

    def span(fn, iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / iters

    rec = dict(mode="3d", kind="diou", iters=a.iters, repeats=a.repeats, shapes=[])
    mod = RotatedIoULoss("3d", "diou", reduction="sum")
    for B, S in SHAPES:
        pred, tgt = (torch.from_numpy(v).to(dev) for v in pairs(np.random.default_rng(B * S), B, S))
        out = ops.rotated_iou_loss(pred, tgt, mode="3d", kind="diou")
        leaf = pred.clone().requires_grad_()

        def step():
            leaf.grad = None
            mod(leaf, tgt).backward()

        forms = {"launch": lambda: ops.rotated_iou_loss(pred, tgt, mode="3d", kind="diou", out=out), "module": step}
        step()
        agree = bool(torch.equal(leaf.grad, out[2]))
        for fn in forms.values():
            for _ in range(5):
                fn()
        torch.cuda.synchronize()
        times = {k: [] for k in forms}
        for _ in range(a.repeats):
            for k, fn in forms.items():                       # alternate the forms
                times[k].append(span(fn, a.iters))
        row = dict(B=B, S=S, N=B * S, mean_iou=round(float(out[1].mean()), 4), module_gradient_is_the_launch=agree)
        for k, v in times.items():
            v = sorted(v)
            row[k] = {"us": round(v[len(v) // 2], 1), "min_us": round(v[0], 1), "max_us": round(v[-1], 1)}
        rec["shapes"].append(row)
        print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
