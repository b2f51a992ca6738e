"""Voxelization timings (SPEC.md §20) -> profiles/voxel_bench.json: voxelize, voxel_index and voxel_reduce(mean) at B = 32 on
the pillars, fine 3-D and nuScenes-shaped configurations, each next to

  * the HBM lower bound of its compulsory bytes (points read once, outputs written once) at 8.0 TB/s, and
  * the composition a user would write today without these operators, timed on the same GPU in the same run:
    torch.unique(key, return_inverse=True) + index_add_ for the dynamic path (order-agnostic, so not bit-comparable: timed
    only), plus a stable argsort and a per-voxel rank for hard voxelization.  It numbers voxels in key order, not in order
    of first appearance, and applies no voxel cap: it does LESS than the operators.

Method: warm-up, HIP events around ITERS back-to-back calls, REPEATS repeats, median and min..max reported.
    python tools/voxel_bench.py [--batch 32] [--iters 20] [--repeats 5]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_BPS = 8.0e12

CONFIGS = {
    "pillars": dict(v=(0.16, 0.16, 4), r=(0, -39.68, -3, 69.12, 39.68, 1), T=32, V=16000, scene="kitti"),
    "fine": dict(v=(0.05, 0.05, 0.1), r=(0, -40, -3, 70.4, 40, 1), T=5, V=16000, scene="kitti"),
    "nuscenes": dict(v=(0.2, 0.2, 8), r=(-51.2, -51.2, -5, 51.2, 51.2, 3), T=20, V=30000, scene="nuscenes"),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "voxel_bench.json"))
    a = ap.parse_args()
    import sad_amd  # noqa: F401
    import torch
    from sad_amd import ops, synth
    dev = torch.device("cuda:0")
    B = a.batch

    def timed(fn, iters=a.iters):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(a.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                fn()
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1) * 1e3 / iters)
        ts.sort()
        return {"us": round(ts[len(ts) // 2], 2), "min_us": round(ts[0], 2), "max_us": round(ts[-1], 2)}

    rows = []
    for name, c in CONFIGS.items():
        host = synth.make_batch(0, B) if c["scene"] == "kitti" else synth.make_nuscenes_batch(0, B)
        host = np.ascontiguousarray(host[..., :4], np.float32)
        N, C = host.shape[1], host.shape[2]
        pts = torch.from_numpy(host).to(dev)
        flat = pts.view(B * N, C)
        off = torch.arange(0, (B + 1) * N, N, dtype=torch.int32, device=dev)
        v, r, T, V = c["v"], c["r"], c["T"], c["V"]
        ws = ops.voxel_workspace(B * N, B, V, dev)
        p2v = ops.voxel_index(flat, off, v, r, V, workspace=ws)[0]
        vt = torch.tensor(v, dtype=torch.float32, device=dev)
        lo = torch.tensor(r[:3], dtype=torch.float32, device=dev)
        G = [int(x) for x in np.rint((np.asarray(r[3:], np.float32) - np.asarray(r[:3], np.float32)) / np.asarray(v, np.float32))]
        Gt = torch.tensor(G, dtype=torch.float32, device=dev)
        sid = torch.arange(B, device=dev).repeat_interleave(N)

        def torch_index():
            g = torch.floor((flat[:, :3] - lo) / vt)
            ok = ((g >= 0) & (g < Gt)).all(1)
            gi = g.long()
            key = ((sid * G[2] + gi[:, 2]) * G[1] + gi[:, 1]) * G[0] + gi[:, 0]
            key = torch.where(ok, key, torch.full_like(key, -1))
            uniq, inv = torch.unique(key, return_inverse=True)
            return uniq, inv, ok

        def torch_mean():
            uniq, inv, ok = torch_index()
            s = torch.zeros((uniq.shape[0], C), dtype=torch.float32, device=dev).index_add_(0, inv, flat)
            n = torch.zeros((uniq.shape[0],), dtype=torch.float32, device=dev).index_add_(0, inv, torch.ones_like(inv, dtype=torch.float32))
            return s / n[:, None]

        def torch_hard():
            uniq, inv, ok = torch_index()
            order = torch.argsort(inv, stable=True)
            sinv = inv[order]
            cnt = torch.bincount(inv, minlength=uniq.shape[0])
            start = torch.cumsum(cnt, 0) - cnt
            rank = torch.arange(inv.shape[0], device=dev) - start[sinv]
            keep = rank < T
            vox = torch.zeros((uniq.shape[0], T, C), dtype=torch.float32, device=dev)
            vox[sinv[keep], rank[keep]] = flat[order[keep]]
            return vox

        ours = {
            "voxelize": lambda: ops.voxelize(flat, off, v, r, T, V, workspace=ws),
            "voxel_index": lambda: ops.voxel_index(flat, off, v, r, V, workspace=ws),
            "voxel_reduce_mean": lambda: ops.voxel_reduce(flat, p2v, off, V, "mean", workspace=ws),
        }
        theirs = {"voxelize": torch_hard, "voxel_index": torch_index, "voxel_reduce_mean": torch_mean}
        nbytes = {
            "voxelize": B * N * C * 4 + B * V * T * C * 4 + B * V * 4 * 4 + B * 4,
            "voxel_index": B * N * C * 4 + B * N * 4 + B * V * 4 * 4 + B * 4,
            "voxel_reduce_mean": B * N * C * 4 + B * N * 4 + B * V * C * 4,
        }
        for op in ours:
            t = timed(ours[op])
            tt = timed(theirs[op], iters=max(2, a.iters // 4))
            bound = nbytes[op] / HBM_BPS * 1e6
            row = {"config": name, "op": op, "B": B, "N": N, "C": C, "T": T, "V": V, **t, "compulsory_bytes": nbytes[op],
                   "hbm_bound_us": round(bound, 2), "fraction_of_bound": round(bound / t["us"], 3),
                   "torch_us": tt["us"], "torch_min_us": tt["min_us"], "torch_max_us": tt["max_us"],
                   "ratio_torch_over_ours": round(tt["us"] / t["us"], 2),
                   "not_slower_outside_spread": tt["min_us"] >= t["max_us"]}
            rows.append(row)
            print(json.dumps(row), flush=True)
    doc = {"method": f"HIP events around {a.iters} back-to-back calls (torch composition: {max(2, a.iters // 4)}), {a.repeats} repeats, "
                     "median and min..max; 3 warm-up calls; workspace allocated once outside the timed region",
           "hbm_bps": HBM_BPS, "device": torch.cuda.get_device_name(0), "rows": rows}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()
