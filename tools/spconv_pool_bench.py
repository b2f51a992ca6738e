"""Timings of the sparse max pool, its backward and the inverse convolution (SPEC.md §22) -> profiles/spconv_pool_bench.json: the
scenes, timing method and roofline conventions of tools/spconv_bench.py (B = 32 ``synth`` KITTI-shaped scenes voxelized at
0.05 x 0.05 x 0.1 m; the pooled tensor is the first-level voxel set), the strided rulebooks k333s2p1 and k222s2p0, C = 16 .. 128.

pool / pool backward   time against the COMPULSORY bytes at 8 TB/s: the index rows (nbr / nbrT), the valid feature rows (or g and
                       arg rows) once per use, the outputs.  Next to each, in the same process on the same rulebook, what a user
                       writes without the operator: index_select on a table padded with a row of -inf + max over kk (in chunks of
                       2^18 output rows, to bound the [rows,Kvol,C] intermediate), and scatter_add_ of g by arg for the backward.
inverse convolution    ``sad_spconv_f32`` over nbrT against the partner layer's forward (the same kernel over nbr) at the same
                       channel pair; the ratio is reported beside Nv / No.

Method: warm-up, HIP events around ITERS back-to-back calls, REPEATS repeats, median and min..max reported.
    python tools/spconv_pool_bench.py [--batch 32] [--iters 10] [--repeats 5]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from spconv_bench import HBM_BPS  # noqa: E402

GEOMETRIES = [("k333s2p1", 3, 2, 1), ("k222s2p0", 2, 2, 0)]
CHANNELS = (16, 32, 64, 128)
PAIRS = ((16, 32), (32, 64), (64, 64))
CHUNK = 1 << 18


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spconv_pool_bench.json"))
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
    Nv = x.feat.shape[0]
    small = max(2, a.iters // 4)
    rows = []
    torch.manual_seed(0)
    for gname, K, s, p in GEOMETRIES:
        G, Kt, st, pt, O = ops.sparse_conv_geometry(x.spatial_shape, K, s, p, False)
        Kvol = Kt[0] * Kt[1] * Kt[2]
        _, _, nbr = ops.sparse_conv_index(x.coors, x.offsets, G, Kt, st, pt, False)
        nbrT, col = ops.sparse_conv_index_transpose(nbr, Nv)
        No = nbr.shape[0]
        nnz, nnzT = int((nbr >= 0).sum().item()), int((nbrT >= 0).sum().item())
        base = {"geometry": gname, "Nv": Nv, "No": No, "Kvol": Kvol, "nbrs_per_out_row": round(nnz / No, 3), "collisions": int(col.item())}
        idx = torch.where(nbr >= 0, nbr, Nv).long()
        for C in CHANNELS:
            feat = torch.randn((Nv, C), device=dev)
            out, arg = ops.sparse_max_pool(feat, nbr)
            g = torch.randn((No, C), device=dev)
            table = torch.cat([feat, torch.full((1, C), float("-inf"), device=dev)])

            def composed():
                outs, args = [], []
                for r0 in range(0, No, CHUNK):
                    ix = idx[r0:r0 + CHUNK]
                    val, kk = table.index_select(0, ix.reshape(-1)).view(ix.shape[0], Kvol, C).max(1)
                    outs.append(val)
                    args.append(torch.gather(ix, 1, kk))
                return torch.cat(outs), torch.cat(args)

            co, ca = composed()
            assert torch.equal(co, out) and torch.equal(ca.int(), arg), "the composition and the operator disagree"      # (normal floats: no ties)
            by = No * Kvol * 4 + nnz * C * 4 + 2 * No * C * 4
            t, tc = timed(lambda: ops.sparse_max_pool(feat, nbr)), timed(composed, iters=small)
            row = {"op": "max_pool", **base, "C": C, **t, "compulsory_bytes": by, "fraction_of_hbm": round(by / HBM_BPS * 1e6 / t["us"], 4),
                   "torch_us": tc["us"], "torch_min_us": tc["min_us"], "torch_max_us": tc["max_us"], "ratio_torch_over_ours": round(tc["us"] / t["us"], 2)}
            rows.append(row)
            print(json.dumps(row), flush=True)
            del table, co, ca
            arg64 = arg.long()

            def composed_b():
                return torch.zeros((Nv, C), device=dev).scatter_add_(0, arg64, g)

            ours = ops.sparse_max_pool_grad(g, arg, nbrT, Nv)
            db = float((ours - composed_b()).abs().max().item())
            by = Nv * Kvol * 4 + nnzT * C * 8 + Nv * C * 4
            t, tc = timed(lambda: ops.sparse_max_pool_grad(g, arg, nbrT, Nv)), timed(composed_b, iters=small)
            row = {"op": "max_pool_grad", **base, "C": C, **t, "compulsory_bytes": by, "fraction_of_hbm": round(by / HBM_BPS * 1e6 / t["us"], 4),
                   "torch_us": tc["us"], "torch_min_us": tc["min_us"], "torch_max_us": tc["max_us"], "ratio_torch_over_ours": round(tc["us"] / t["us"], 2),
                   "max_abs_diff_vs_composition": db}
            rows.append(row)
            print(json.dumps(row), flush=True)
            del feat, out, arg, arg64, g, ours
        for cin, cout in PAIRS:
            W = (torch.rand((Kvol, cout, cin), device=dev) * 2 - 1) * (Kvol * cin) ** -0.5
            pw = ops.PackedSparseWeight(W, torch.rand((cout,), device=dev) * 0.1)
            pwi = ops.PackedSparseWeight((torch.rand((Kvol, cin, cout), device=dev) * 2 - 1) * (Kvol * cout) ** -0.5, torch.rand((cin,), device=dev) * 0.1)
            f_in, f_out = torch.randn((Nv, cin), device=dev), torch.randn((No, cout), device=dev)
            tf = timed(lambda: ops.sparse_conv(f_in, nbr, pw, None, None, True))
            ti = timed(lambda: ops.sparse_conv(f_out, nbrT, pwi, None, None, True))
            row = {"op": "inverse_conv", **base, "partner": f"{cin}->{cout}", "inverse": f"{cout}->{cin}", "partner_forward": tf, "inverse_forward": ti,
                   "ratio_inverse_over_partner": round(ti["us"] / tf["us"], 3), "Nv_over_No": round(Nv / No, 3)}
            rows.append(row)
            print(json.dumps(row), flush=True)
        del nbr, nbrT, idx
        torch.cuda.empty_cache()
    doc = {"method": f"HIP events around {a.iters} back-to-back calls (compositions: {small}), {a.repeats} repeats, median and min..max; 2 warm-up "
                     "calls; rulebooks, transposed rulebooks, packs and the padded table built outside the timed region; output allocation "
                     "(framework caching allocator) inside it on both sides",
           "hbm_bps": HBM_BPS, "device": torch.cuda.get_device_name(0), "batch": B, "voxel_size": list(v), "point_range": list(r), "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()
