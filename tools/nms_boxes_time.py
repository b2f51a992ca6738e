"""nms_boxes (SPEC.md §23) alone: us per call from events around back-to-back calls after warm-up.
(a) B = 32, K = 512, crowded and sparse scenes: nms_boxes next to the three-kernel nms_bev on the same rows (the old path
    is the yardstick), the two alternated over several rounds; (b) B = 32, K = 70 400, pre_max 1000 and 4096.
Under `rocprofv3 --kernel-trace --stats -- python tools/nms_boxes_time.py --split` only (b) runs, a few calls per shape:
the per-stage split is the trace's nmsx_select / nmsx_rank / nms_mask_kernel<NmsxLayout> / nmsx_walk rows.  Any error ends the process."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import numpy as np
import sad_amd  # noqa: F401
import torch
from sad_amd import ops
import nms_ref as ref

ap = argparse.ArgumentParser()
ap.add_argument("--split", action="store_true", help="only (b), 5 calls per shape: for a kernel trace")
ap.add_argument("--reps", type=int, default=200)
ap.add_argument("--rounds", type=int, default=5)
args = ap.parse_args()
dev = torch.device("cuda:0")
F = np.float32
IOU = ref.IOU_THR


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


def scene(B, K, density, seed, n_eff=None):
    rng = np.random.default_rng(seed)
    scores = rng.uniform(0.05, 1.0, (B, K)).astype(F)
    rows = ref.with_scores(ref.crowded(rng, B, K, density=density, n_eff=n_eff), scores)
    return torch.from_numpy(rows).to(dev), torch.from_numpy(scores).to(dev)


if not args.split:
    for tag, density in (("crowded", ref.DENSITY), ("sparse", 0.005)):
        rows, scores = scene(32, 512, density, 11)
        old_buf, new_buf = ops.nms_bev_buffers(32, 512, dev), ops.nms_boxes_buffers(32, 512, dev)
        old = lambda: ops.nms_bev(rows, IOU, 0.0, out=old_buf)
        new = lambda: ops.nms_boxes(rows, scores, None, IOU, 0.0, out=new_buf)
        ko, kn = old(), new()
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(ko, kn)), "nms_boxes differs from nms_bev"
        timed(old, 20), timed(new, 20)                                   # warm-up
        t_old, t_new = [], []
        for _ in range(args.rounds):                                     # alternate the two
            t_old.append(timed(old, args.reps))
            t_new.append(timed(new, args.reps))
        print(f"(a) B=32 K=512 {tag}: kept fraction {kn[2].float().mean().item() / 512:.3f}; nms_bev (three kernels) "
              f"{np.median(t_old):.1f} us [{min(t_old):.1f}, {max(t_old):.1f}], nms_boxes {np.median(t_new):.1f} us "
              f"[{min(t_new):.1f}, {max(t_new):.1f}] per call, {args.rounds} rounds x {args.reps} calls", flush=True)

for pre in (1000, 4096):
    rows, scores = scene(32, 70400, ref.DENSITY, 12, n_eff=pre)
    buf = ops.nms_boxes_buffers(32, 70400, dev, pre_max=pre)
    new = lambda: ops.nms_boxes(rows, scores, None, IOU, 0.3, pre_max=pre, out=buf)
    k = new()
    torch.cuda.synchronize()
    if args.split:
        timed(new, 5)
        print(f"(b) B=32 K=70400 pre_max={pre}: 6 calls traced, kept fraction of the pre-selection {k[2].float().mean().item() / pre:.3f}", flush=True)
        continue
    timed(new, 10)
    ts = [timed(new, max(args.reps // 4, 10)) for _ in range(args.rounds)]
    print(f"(b) B=32 K=70400 pre_max={pre}: kept fraction of the pre-selection {k[2].float().mean().item() / pre:.3f}; nms_boxes "
          f"{np.median(ts):.1f} us [{min(ts):.1f}, {max(ts):.1f}] per call, {args.rounds} rounds x {max(args.reps // 4, 10)} calls", flush=True)
