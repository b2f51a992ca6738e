"""Forward + backward of the fused training path (SharedMLP: the inference kernel forward, the backward of SPEC.md §32) against the
unfused composition it replaces (GroupPoints -> one einsum per layer -> MaxPoolS, VoxelRoIPool._train_rows generalised), in one
process, alternating, on synthetic scenes.

    python tools/probe/mlp_grad_time.py [--shape sa1|sa3|pool|all] [--batch B] [--reps R] [--out file.json]
    python tools/probe/mlp_grad_time.py --shape sa3 --loop 20          (the fused path alone: for a kernel trace of its own)

Shapes: sa1 = the three branches of the KITTI stage 1 (B scenes of 16 384 points, 4 096 groups, radii and nsample from config.py;
first stage: parameter gradients only); sa3 = one chain of the cluster widths 259 -> 256 -> 512 -> 1024, S = 32, on 512 points
and 256 groups per scene (feature and parameter gradients); pool = Voxel R-CNN's RoI grid pooling at the operator level: one ragged
scene of voxel centres, 2 x 128 RoIs x 6^3 grid points, S = 16, 32 -> 32 -> 32, empty groups skipped.  Reported per chain: ms per
forward + backward of either path (median of the repetitions, device events), torch.cuda.max_memory_allocated of either, the
executed-row fraction, and the flops of the weight-gradient products on executed rows.  If the composition does not fit in memory
the batch is halved until it does and the largest batch that fits is reported."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))


def composition(ws, bs, xyz, feat_pm, new_xyz, idx):
    """The parent path: dense [B,3+C,M,S] rows, every activation saved by autograd."""
    import torch
    from sad_amd import autograd, ops
    with torch.no_grad():
        rel = ops.group_points(xyz.transpose(1, 2).contiguous(), idx) - new_xyz.transpose(1, 2).unsqueeze(-1)
    x = rel if feat_pm is None else torch.cat([rel, autograd.GroupPoints.apply(feat_pm.transpose(1, 2).contiguous(), idx)], 1)
    for w, b in zip(ws, bs):
        x = torch.relu(torch.einsum("oc,bcms->boms", w, x) + b.view(1, -1, 1, 1))
    return autograd.MaxPoolS.apply(x.contiguous()).transpose(1, 2)


def chains_of(shape, B, dev, seed=0):
    """[(name, dims, xyz, feat_pm, new_xyz, idx, cnt, feat_grad, skip_empty)] of a shape, built by the library's own sampling and query."""
    import torch
    from sad_amd import config, ops, synth
    rng = np.random.default_rng(seed)
    out = []
    if shape == "sa1":
        st = config.KITTI.stages[0]
        pts = torch.from_numpy(synth.make_batch(0, B)).to(dev)
        xyz, feat = ops.split_points(pts)
        new_xyz = ops.gather_xyz(xyz, ops.fps(xyz, st.npoint))
        idxs, cnts = ops.ball_query_multi(st.radii, st.nsamples, xyz, new_xyz, None, return_counts=True)
        for k, (idx, cnt, mlp) in enumerate(zip(idxs, cnts, st.mlps)):
            out.append((f"sa1.b{k}", [4] + list(mlp), xyz, feat, new_xyz, idx, cnt, False, False))
    elif shape == "sa3":
        pts = torch.from_numpy(synth.make_batch(0, B)).to(dev)
        xyz0, _ = ops.split_points(pts)
        xyz = ops.gather_xyz(xyz0, ops.fps(xyz0, 512))
        new_xyz = ops.gather_xyz(xyz, ops.fps(xyz, 256))
        feat = torch.from_numpy(rng.standard_normal((B, 512, 256)).astype(np.float32)).to(dev)
        idxs, cnts = ops.ball_query_multi((4.8,), (32,), xyz, new_xyz, None, return_counts=True)
        out.append(("cluster 259-256-512-1024", [259, 256, 512, 1024], xyz, feat, new_xyz, idxs[0], cnts[0], True, False))
    elif shape == "pool":
        Nv, M = 40000, 2 * 128 * 216
        xyz = torch.from_numpy((rng.uniform(0, 1, (1, Nv, 3)) * np.array([70.4, 80.0, 4.0]) + np.array([0, -40.0, -3.0])).astype(np.float32)).to(dev)
        centre = xyz[0, torch.from_numpy(rng.integers(0, Nv, 256)).to(dev)]                        # RoIs around occupied places
        grid = torch.from_numpy(rng.uniform(-1, 1, (256, 216, 3)).astype(np.float32) * np.array([2.0, 1.0, 0.8], np.float32)).to(dev)
        new_xyz = (centre[:, None, :] + grid).reshape(1, M, 3).contiguous()
        feat = torch.from_numpy(rng.standard_normal((1, Nv, 32)).astype(np.float32)).to(dev)
        idxs, cnts = ops.ball_query_multi((0.8,), (16,), xyz, new_xyz, None, return_counts=True)
        out.append(("roi pool 35-32-32", [35, 32, 32], xyz, feat, new_xyz, idxs[0], cnts[0], True, True))
    else:
        raise ValueError(shape)
    return out


def run_chain(chain, reps, dev, loop=0):
    import torch
    from sad_amd import synth
    from sad_amd.shared_mlp import SharedMLP
    name, dims, xyz, feat, new_xyz, idx, cnt, feat_grad, skip = chain
    B, M, S = idx.shape
    layers = synth.make_mlp_weights(dims, np.random.default_rng(1))
    mod = SharedMLP(dims, True, layers=layers).to(dev).requires_grad_(True)
    f = None if feat is None else feat.clone().requires_grad_(feat_grad)
    empty = (cnt == 0).unsqueeze(-1)

    def fused():
        out = mod.grouped(xyz, f, new_xyz, idx, cnt, skip_empty=skip)
        (out.masked_fill(empty, 0.0) if skip else out).square().sum().backward()

    def unfused():
        out = composition(list(mod.weight), list(mod.bias), xyz, f, new_xyz, idx)
        (out.masked_fill(empty, 0.0) if skip else out).square().sum().backward()

    def clear():
        for p in list(mod.parameters()) + ([f] if f is not None else []):
            p.grad = None

    if loop:
        for _ in range(loop):
            fused()
            clear()
        torch.cuda.synchronize()
        return {"chain": name, "loop": loop}
    rows = int(torch.clamp(cnt, 1, S).sum().item()) - (int((cnt == 0).sum().item()) if skip else 0)
    res = {"chain": name, "dims": dims, "B": B, "M": M, "S": S, "rows_executed": rows, "rows_dense": B * M * S,
           "executed_fraction": rows / (B * M * S),
           "grad_w_flops_executed": 2 * rows * sum(a * b for a, b in zip(dims[:-1], dims[1:]))}
    times = {"fused": [], "unfused": []}
    fits = True
    for r in range(reps + 1):                                    # (the first repetition warms both paths up)
        for tag, fn in (("fused", fused), ("unfused", unfused)):
            if tag == "unfused" and not fits:
                continue
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            try:
                e0.record()
                fn()
                e1.record()
                torch.cuda.synchronize()
            except torch.cuda.OutOfMemoryError:
                fits = False
                res["unfused_out_of_memory"] = True
                clear()
                torch.cuda.empty_cache()
                continue
            if r:
                times[tag].append(e0.elapsed_time(e1))
            res[f"{tag}_peak_bytes"] = torch.cuda.max_memory_allocated() - base
            clear()
    from sad_amd import autograd
    res["mismatch"] = int(autograd.GroupedMLP.last_mismatch.item())
    for tag in times:
        if times[tag]:
            res[f"{tag}_ms"] = float(np.median(times[tag]))
            res[f"{tag}_ms_min_max"] = [float(min(times[tag])), float(max(times[tag]))]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="all", choices=["sa1", "sa3", "pool", "all"])
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--loop", type=int, default=0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import sad_amd  # noqa: F401
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("mlp_grad_time.py needs a GPU (a timing on the CPU says nothing)")
    dev = torch.device("cuda:0")
    results = []
    for shape in (["sa1", "sa3", "pool"] if a.shape == "all" else [a.shape]):
        B = 1 if shape == "pool" else a.batch
        while True:
            rs = [run_chain(c, a.reps, dev, a.loop) for c in chains_of(shape, B, dev)]
            if a.loop or B == 1 or not any(r.get("unfused_out_of_memory") for r in rs):
                break
            for r in rs:
                r["note"] = f"the composition does not fit at B = {B}"
                print(json.dumps(r), flush=True)
            B //= 2
            torch.cuda.empty_cache()
        for r in rs:
            print(json.dumps(r), flush=True)
        results += rs
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(results, fh, indent=1)


if __name__ == "__main__":
    main()
