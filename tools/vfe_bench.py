"""Voxel feature encoder timings (SPEC.md §24) -> profiles/vfe_bench.json: the fused ``ops.voxel_encode`` against the composition
of operators that existed before it (torch decoration -> ``PackedMLP.rows`` -> ``ops.voxel_reduce(max)``), on

  * pillars   32 x 16 384 synthetic KITTI-shaped points, C = 4, Cin = 10, Cout = 64, V = 16 000 (tests/voxel_cases.py PILLARS)
  * dynamic   the same points on a 3-D grid (0.2, 0.2, 0.4), V = 16 000, Cout = 128

with the bytes each form moves.  The composition's decoration uses the per-voxel mean from ``ops.voxel_reduce(mean)`` and torch
indexing; its [total, Cin] rows and [total, Cout] layer output are written once and read once.

Method: warm-up, then REPEATS rounds in which the two forms ALTERNATE, each timed by HIP events around ITERS back-to-back calls;
median and min..max per form.
    python tools/vfe_bench.py [--batch 32] [--iters 20] [--repeats 7]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = {
    "pillars": dict(v=(0.16, 0.16, 4), r=(0, -39.68, -3, 69.12, 39.68, 1), V=16000, cout=64),
    "dynamic": dict(v=(0.2, 0.2, 0.4), r=(0, -39.68, -3, 69.12, 39.68, 1), V=16000, cout=128),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vfe_bench.json"))
    a = ap.parse_args()
    import sad_amd  # noqa: F401
    import torch
    from sad_amd import ops, synth
    dev = torch.device("cuda:0")
    B, N, C = a.batch, 16384, 4
    xyz = np.stack([synth.make_scene(s, N) for s in range(B)]).astype(np.float32)[..., :3]
    rng = np.random.default_rng(0)
    pts = torch.from_numpy(np.concatenate([xyz, rng.random((B, N, 1), dtype=np.float32)], -1).reshape(B * N, C)).to(dev)
    off = torch.arange(0, (B + 1) * N, N, dtype=torch.int32, device=dev)
    sid = torch.arange(B, device=dev).repeat_interleave(N)
    out = []
    for name, c in CONFIGS.items():
        V, cout, cin = c["V"], c["cout"], C + 6
        p2v, coors, count, voxel_num = ops.voxel_index(pts, off, c["v"], c["r"], V)
        W = torch.from_numpy((rng.standard_normal((cout, cin)) / np.sqrt(cin)).astype(np.float32)).to(dev)
        b = torch.from_numpy((rng.standard_normal(cout) * 0.1).astype(np.float32)).to(dev)
        mlp = ops.PackedMLP([(W, b)], False, dev)
        ws = ops.voxel_encode_workspace(B * N, B, V, cin, cout, dev)
        ws_r = ops.voxel_workspace(B * N, B, V, dev)
        vs = torch.tensor(c["v"], dtype=torch.float32, device=dev)
        lo = torch.tensor(c["r"][:3], dtype=torch.float32, device=dev)
        live = p2v >= 0
        s = (sid * V + p2v.clamp_min(0)).long()

        def fused():
            return ops.voxel_encode(pts, p2v, off, V, W, b, coors, c["v"], c["r"], workspace=ws)

        def composed():
            mean = ops.voxel_reduce(pts[:, :3].contiguous(), p2v, off, V, "mean", workspace=ws_r).view(B * V, 3)
            ctr = coors.view(B * V, 3).flip(1).float() * vs + (0.5 * vs + lo)
            rows = torch.cat([pts, pts[:, :3] - mean[s], pts[:, :3] - ctr[s]], 1)
            rows = torch.where(live[:, None], rows, torch.zeros_like(rows))
            return ops.voxel_reduce(mlp.rows(rows), p2v, off, V, "max", workspace=ws_r)[0]

        same = bool((fused() == composed()).all())
        forms = {"fused": fused, "composed": composed}
        for fn in forms.values():
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        ts = {k: [] for k in forms}
        for _ in range(a.repeats):
            for k, fn in forms.items():                       # alternate the two forms
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.iters):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                ts[k].append(e0.elapsed_time(e1) * 1e3 / a.iters)
        total, nvox = B * N, B * V
        # compulsory traffic of each form (bytes): reads + writes of every tensor that goes through memory
        by_f = total * C * 4 + total * 4 + nvox * cout * 4
        by_c = by_f + 2 * total * cin * 4 + 2 * total * cout * 4 + nvox * cout * 4 + 2 * nvox * 3 * 4 + 2 * total * 6 * 4
        rec = dict(case=name, B=B, N=N, V=V, cin=cin, cout=cout, voxels=int(voxel_num.sum()), taken=int(live.sum()), equal=same,
                   fused_bytes=by_f, composed_bytes=by_c)
        for k, v in ts.items():
            v.sort()
            rec[k] = {"us": round(v[len(v) // 2], 1), "min_us": round(v[0], 1), "max_us": round(v[-1], 1)}
        print(json.dumps(rec), flush=True)
        out.append(rec)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
