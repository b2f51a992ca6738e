"""Sparse-convolution timings (SPEC.md §21) -> profiles/spconv_bench.json: B = 32 ``synth`` KITTI-shaped scenes voxelized at
0.05 x 0.05 x 0.1 m, then the layers of the SECOND ladder and their rulebook builds.  Per layer: time, rows, mean neighbours per
row, useful and executed flops (the kernel skips a kernel offset per 32-row subtile, csrc/spconv.hip), compulsory bytes (feat
once + nbr + out + W), the fraction of the f32 MFMA peak and of HBM reached and which of the two bounds the layer; next to it, in
the same process on the same inputs, the composition a user would write without the operator: per kernel offset
index_select -> torch.mm -> index_add_ over pair lists made from the same nbr outside the timed region.

Method: warm-up, HIP events around ITERS back-to-back calls, REPEATS repeats, median and min..max reported.
    python tools/spconv_bench.py [--batch 32] [--iters 10] [--repeats 5]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_BPS = 8.0e12
F32_MFMA_FLOPS = 256 * 4 * 64 * 2.4e9          # 256 CUs x 4 SIMDs x 64 FLOP / clock x 2.4 GHz = 157 TFLOP/s

# (name, Cin, Cout, kernel, stride, padding, subm, rulebook key)
LADDER = [
    ("subm1a 4->16", 4, 16, 3, 1, 1, True, "subm1"),
    ("subm1b 16->16", 16, 16, 3, 1, 1, True, "subm1"),
    ("down1 16->32 s2", 16, 32, 3, 2, 1, False, "down1"),
    ("subm2 32->32", 32, 32, 3, 1, 1, True, "subm2"),
    ("down2 32->64 s2", 32, 64, 3, 2, 1, False, "down2"),
    ("subm3 64->64", 64, 64, 3, 1, 1, True, "subm3"),
    ("down3 64->64 s2 p(0,1,1)", 64, 64, 3, 2, (0, 1, 1), False, "down3"),
    ("out 64->128 (3,1,1) s(2,1,1)", 64, 128, (3, 1, 1), (2, 1, 1), 0, False, "out"),
]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spconv_bench.json"))
    a = ap.parse_args()
    import sad_amd  # noqa: F401
    import torch
    from sad_amd import ops, synth
    from sad_amd.spconv import SparseTensor
    dev = torch.device("cuda:0")
    B = a.batch

    def timed(fn, iters=a.iters):
        for _ in range(2):
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

    host = np.ascontiguousarray(synth.make_batch(0, B)[..., :4], np.float32)
    N = host.shape[1]
    flat = torch.from_numpy(host).to(dev).view(B * N, 4)
    off = torch.arange(0, (B + 1) * N, N, dtype=torch.int32, device=dev)
    v, r, V = (0.05, 0.05, 0.1), (0, -40, -3, 70.4, 40, 1), N
    p2v, vcoors, _, vnum = ops.voxel_index(flat, off, v, r, V)
    x = SparseTensor.from_voxels(ops.voxel_reduce(flat, p2v, off, V, "mean"), vcoors, vnum, (40, 1600, 1408))
    torch.manual_seed(0)
    rows, books = [], {}
    for name, cin, cout, K, s, p, subm, key in LADDER:
        G, Kt, st, pt, O = ops.sparse_conv_geometry(x.spatial_shape, K, s, p, subm)
        Kvol = Kt[0] * Kt[1] * Kt[2]
        if key not in books:
            build = lambda: ops.sparse_conv_index(x.coors, x.offsets, G, Kt, st, pt, subm)       # noqa: E731
            books[key] = build()
            tb = timed(build, iters=max(2, a.iters // 2))
            row = {"op": "rulebook", "layer": key, "subm": subm, "Nv": x.coors.shape[0], "No": books[key][0].shape[0], "Kvol": Kvol,
                   "spatial_shape": list(G), "out_shape": list(O), **tb,
                   "note": "strided: includes the one read-back of the row count" if not subm else ""}
            rows.append(row)
            print(json.dumps(row), flush=True)
        oc, oo, nbr = books[key]
        Nv, No = x.feat.shape[0], nbr.shape[0]
        W = (torch.rand((Kvol, cout, cin), device=dev) * 2 - 1) * (Kvol * cin) ** -0.5
        bias = torch.rand((cout,), device=dev) * 0.1
        pw = ops.PackedSparseWeight(W, bias)
        has = nbr >= 0
        nnz = int(has.sum().item())
        padr = (-No) % 32
        sub = torch.cat([has, torch.zeros((padr, Kvol), dtype=torch.bool, device=dev)]).view(-1, 32, Kvol).any(1)
        cinp, coutp = (cin + 7) // 8 * 8, (cout + 31) // 32 * 32
        useful = 2.0 * nnz * cin * cout
        executed = 2.0 * int(sub.sum().item()) * 32 * cinp * coutp
        nbytes = Nv * cin * 4 + No * Kvol * 4 + No * cout * 4 + Kvol * cout * cin * 4
        t = timed(lambda: ops.sparse_conv(x.feat, nbr, pw, None, None, True))
        pairs = []
        for kk in range(Kvol):
            o = torch.nonzero(has[:, kk]).squeeze(1)
            pairs.append((o, nbr[o, kk].long(), W[kk].t().contiguous()))

        def composed():
            out = bias.repeat(No, 1)
            for o, i, wt in pairs:
                if o.numel():
                    out.index_add_(0, o, torch.mm(x.feat.index_select(0, i), wt))
            return torch.relu_(out)

        tt = timed(composed, iters=max(2, a.iters // 4))
        got, ref = ops.sparse_conv(x.feat, nbr, pw, None, None, True), composed()
        mfma_us, hbm_us = executed / F32_MFMA_FLOPS * 1e6, nbytes / HBM_BPS * 1e6
        row = {"op": "sparse_conv", "layer": name, "Nv": Nv, "No": No, "Kvol": Kvol, "Cin": cin, "Cout": cout,
               "mean_neighbours": round(nnz / max(No, 1), 3), **t, "useful_flops": useful, "executed_flops": executed,
               "useful_over_executed": round(useful / executed, 4), "compulsory_bytes": nbytes,
               "useful_tflops": round(useful / t["us"] / 1e6, 3), "executed_tflops": round(executed / t["us"] / 1e6, 3),
               "fraction_of_f32_mfma_peak_executed": round(mfma_us / t["us"], 4), "fraction_of_f32_mfma_peak_useful": round(useful / F32_MFMA_FLOPS * 1e6 / t["us"], 4),
               "fraction_of_hbm": round(hbm_us / t["us"], 4), "nearer_bound": "mfma" if mfma_us > hbm_us else "hbm",
               "torch_us": tt["us"], "torch_min_us": tt["min_us"], "torch_max_us": tt["max_us"],
               "ratio_torch_over_ours": round(tt["us"] / t["us"], 2),
               "max_abs_diff_vs_composition": float((got - ref).abs().max().item())}
        rows.append(row)
        print(json.dumps(row), flush=True)
        x = SparseTensor(got, oc, oo, O)
    d = timed(lambda: x.dense())
    rows.append({"op": "sparse_to_dense", "No": x.feat.shape[0], "C": x.feat.shape[1], "shape": list(x.spatial_shape), **d})
    print(json.dumps(rows[-1]), flush=True)
    doc = {"method": f"HIP events around {a.iters} back-to-back calls (composition: {max(2, a.iters // 4)}, rulebooks: {max(2, a.iters // 2)}), "
                     f"{a.repeats} repeats, median and min..max; 2 warm-up calls; weights packed and pair lists built outside the timed region; "
                     "output and workspace allocation (framework caching allocator) inside it on both sides",
           "f32_mfma_peak_flops": F32_MFMA_FLOPS, "hbm_bps": HBM_BPS, "device": torch.cuda.get_device_name(0), "batch": B,
           "voxel_size": list(v), "point_range": list(r), "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()
