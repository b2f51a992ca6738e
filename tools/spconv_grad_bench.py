"""Timings of the sparse-convolution backward (SPEC.md §21.4) -> profiles/spconv_grad_bench.json: the scenes, layers, timing
method and roofline conventions of tools/spconv_bench.py (B = 32 ``synth`` KITTI-shaped scenes voxelized at 0.05 x 0.05 x 0.1 m,
the layers of the SECOND ladder).  Per layer: the transposed-rulebook build (once per rulebook), grad_feat (the forward kernel
over nbrT and the packed W^T) and grad_W + grad_bias (csrc/spconv_grad.hip), each with useful and executed flops, compulsory
bytes, the fractions of the f32 MFMA peak and of HBM and the nearer bound; next to each, in the same process on the same inputs,
the composition a user would write without the operator, over pair lists made from the same nbr outside the timed region:
grad_feat = per offset index_select -> mm -> index_add_, grad_W = per offset index_select -> mm(g^T, f).  Last: forward +
backward of the four-layer sequential of the tests under one timer.

Method: warm-up, HIP events around ITERS back-to-back calls, REPEATS repeats, median and min..max reported.
    python tools/spconv_grad_bench.py [--batch 32] [--iters 10] [--repeats 5]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from spconv_bench import F32_MFMA_FLOPS, HBM_BPS, LADDER  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spconv_grad_bench.json"))
    a = ap.parse_args()
    import sad_amd  # noqa: F401
    import torch
    from sad_amd import ops, synth
    from sad_amd.spconv import SparseConv3d, SparseSequential, SparseTensor, SubMConv3d
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

    def roof(t_us, executed, nbytes):
        mfma_us, hbm_us = executed / F32_MFMA_FLOPS * 1e6, nbytes / HBM_BPS * 1e6
        return {"fraction_of_f32_mfma_peak_executed": round(mfma_us / t_us, 4), "fraction_of_hbm": round(hbm_us / t_us, 4),
                "nearer_bound": "mfma" if mfma_us > hbm_us else "hbm"}

    def subtiles(has, rows):
        """32-row subtiles x offsets that hold at least one entry (what the forward kernel executes)."""
        pad = (-has.shape[0]) % rows
        return int(torch.cat([has, torch.zeros((pad, has.shape[1]), dtype=torch.bool, device=dev)]).view(-1, rows, has.shape[1]).any(1).sum().item())

    host = np.ascontiguousarray(synth.make_batch(0, B)[..., :4], np.float32)
    N = host.shape[1]
    flat = torch.from_numpy(host).to(dev).view(B * N, 4)
    off = torch.arange(0, (B + 1) * N, N, dtype=torch.int32, device=dev)
    v, r, V = (0.05, 0.05, 0.1), (0, -40, -3, 70.4, 40, 1), N
    p2v, vcoors, _, vnum = ops.voxel_index(flat, off, v, r, V)
    x = SparseTensor.from_voxels(ops.voxel_reduce(flat, p2v, off, V, "mean"), vcoors, vnum, (40, 1600, 1408))
    x0 = x
    torch.manual_seed(0)
    rows, books, booksT = [], {}, {}
    small = max(2, a.iters // 4)
    for name, cin, cout, K, s, p, subm, key in LADDER:
        G, Kt, st, pt, O = ops.sparse_conv_geometry(x.spatial_shape, K, s, p, subm)
        Kvol = Kt[0] * Kt[1] * Kt[2]
        if key not in books:
            books[key] = ops.sparse_conv_index(x.coors, x.offsets, G, Kt, st, pt, subm)
        oc, oo, nbr = books[key]
        Nv, No = x.feat.shape[0], nbr.shape[0]
        if key not in booksT:
            build = lambda: ops.sparse_conv_index_transpose(nbr, Nv)       # noqa: E731
            booksT[key] = build()
            row = {"op": "index_transpose", "layer": key, "Nv": Nv, "No": No, "Kvol": Kvol, "collisions": int(booksT[key][1].item()),
                   **timed(build, iters=max(2, a.iters // 2)), "note": "without the read-back of the collision count"}
            rows.append(row)
            print(json.dumps(row), flush=True)
        nbrT = booksT[key][0]
        W = (torch.rand((Kvol, cout, cin), device=dev) * 2 - 1) * (Kvol * cin) ** -0.5
        bias = torch.rand((cout,), device=dev) * 0.1
        pw, pwt = ops.PackedSparseWeight(W, bias), ops.PackedSparseWeight(W.transpose(1, 2).contiguous(), None)
        out = ops.sparse_conv(x.feat, nbr, pw, None, None, True)
        g = torch.randn((No, cout), device=dev) * (out > 0)
        has, hasT = nbr >= 0, nbrT >= 0
        nnz = int(has.sum().item())
        useful = 2.0 * nnz * cin * cout
        pairs = []
        for kk in range(Kvol):
            o = torch.nonzero(has[:, kk]).squeeze(1)
            pairs.append((o, nbr[o, kk].long(), W[kk].contiguous()))
        # ---- grad_feat ----
        coutp8, cinp32 = (cout + 7) // 8 * 8, (cin + 31) // 32 * 32
        ex_f = 2.0 * subtiles(hasT, 32) * 32 * coutp8 * cinp32
        by_f = No * cout * 4 + Nv * Kvol * 4 + Nv * cin * 4 + Kvol * cout * cin * 4
        tf = timed(lambda: ops.sparse_conv_grad_input(g, nbrT, pwt))

        def composed_f():
            gf = torch.zeros((Nv, cin), device=dev)
            for o, i, w in pairs:
                if o.numel():
                    gf.index_add_(0, i, torch.mm(g.index_select(0, o), w))
            return gf

        tcf = timed(composed_f, iters=small)
        df = float((ops.sparse_conv_grad_input(g, nbrT, pwt) - composed_f()).abs().max().item())
        row = {"op": "grad_feat", "layer": name, "Nv": Nv, "No": No, "Kvol": Kvol, "Cin": cin, "Cout": cout, **tf, "useful_flops": useful,
               "executed_flops": ex_f, "useful_over_executed": round(useful / ex_f, 4), "compulsory_bytes": by_f, **roof(tf["us"], ex_f, by_f),
               "torch_us": tcf["us"], "torch_min_us": tcf["min_us"], "torch_max_us": tcf["max_us"], "ratio_torch_over_ours": round(tcf["us"] / tf["us"], 2),
               "max_abs_diff_vs_composition": df}
        rows.append(row)
        print(json.dumps(row), flush=True)
        # ---- grad_W + grad_bias: the kernel runs every (64-row tile, offset) that holds an entry, all 64 rows of it, for every
        # 128 x 128 block of [Cout x Cin], channels padded to 32 ----
        coutp32 = (cout + 31) // 32 * 32
        ex_w = 2.0 * subtiles(has, 64) * 64 * coutp32 * cinp32
        by_w = Nv * cin * 4 + No * Kvol * 4 + No * cout * 4 + Kvol * cout * cin * 4
        tw = timed(lambda: ops.sparse_conv_grad_weight(x.feat, nbr, g))

        def composed_w():
            gw = torch.zeros((Kvol, cout, cin), device=dev)
            for kk, (o, i, _) in enumerate(pairs):
                if o.numel():
                    torch.mm(g.index_select(0, o).t(), x.feat.index_select(0, i), out=gw[kk])
            return gw, g.sum(0)

        tcw = timed(composed_w, iters=small)
        dw = float((ops.sparse_conv_grad_weight(x.feat, nbr, g)[0] - composed_w()[0]).abs().max().item())
        row = {"op": "grad_weight", "layer": name, "Nv": Nv, "No": No, "Kvol": Kvol, "Cin": cin, "Cout": cout, **tw, "useful_flops": useful,
               "executed_flops": ex_w, "useful_over_executed": round(useful / ex_w, 4), "compulsory_bytes": by_w, **roof(tw["us"], ex_w, by_w),
               "torch_us": tcw["us"], "torch_min_us": tcw["min_us"], "torch_max_us": tcw["max_us"], "ratio_torch_over_ours": round(tcw["us"] / tw["us"], 2),
               "max_abs_diff_vs_composition": dw}
        rows.append(row)
        print(json.dumps(row), flush=True)
        x = SparseTensor(out, oc, oo, O)
    # ---- forward + backward of the four-layer sequential under one timer (rulebooks and transposed rulebooks cached) ----
    net = SparseSequential(SubMConv3d(4, 16, 3, relu=True, indice_key="subm1"), SubMConv3d(16, 16, 3, relu=True, indice_key="subm1"),
                           SparseConv3d(16, 32, 3, 2, 1, relu=True, indice_key="down1"), SubMConv3d(32, 32, 3, bias=False, indice_key="subm2")).to(dev)
    tfwd = timed(lambda: net(x0), iters=small)
    net.requires_grad_(True)

    def step():
        net.zero_grad(set_to_none=True)
        net(x0).feat.sum().backward()

    tstep = timed(step, iters=small)
    rows.append({"op": "sequential4", "forward_no_grad": tfwd, "forward_backward": tstep,
                 "note": "4 -> 16 -> 16 -> (s2) 32 -> 32 on the first-level voxels; parameters require grad, the input does not"})
    print(json.dumps(rows[-1]), flush=True)
    doc = {"method": f"HIP events around {a.iters} back-to-back calls (compositions and the sequential: {small}, index_transpose: {max(2, a.iters // 2)}), "
                     f"{a.repeats} repeats, median and min..max; 2 warm-up calls; weights packed and pair lists built outside the timed region; "
                     "output allocation (framework caching allocator) and the zero-fill of the accumulated outputs inside it on both sides",
           "f32_mfma_peak_flops": F32_MFMA_FLOPS, "hbm_bps": HBM_BPS, "device": torch.cuda.get_device_name(0), "batch": B,
           "voxel_size": list(v), "point_range": list(r), "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()
