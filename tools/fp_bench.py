"""Feature-propagation timings (SPEC.md §18): three_nn (every kernel form), three_interpolate in both layouts, its backward
and an FPModule at B = 32, (n, m) = (16384, 4096) and (4096, 1024), C = 128.  Prints ONE JSON line.

    python tools/fp_bench.py [--out FILE]

The parent process never touches the GPU.  It runs (each in a child process under its own `timeout`):
  1. `fp_bench.py --child`: device-event timings after warm-up, and a torch composition (cdist + topk + gather) for context;
  2. per shape, `rocprofv3 --kernel-trace --stats -- fp_bench.py --child --shape i`: the kernel times.
Bounds: three_nn against the f32 vector rate (9 VALU operations per pair, 157.3 TF counting an FMA as two);
three_interpolate against HBM (8.0 TB/s spec peak; compulsory bytes = output written once + known table read once);
the backward against the memory-side float-atomic rate (1.3 TB/s of added bytes, MI355X measurement).
"""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(16384, 4096), (4096, 1024)]
B, C = 32, 128
VALU_OPS_PER_S = 157.3e12 / 2          # wave-lane f32 operations per second (an FMA counts as two flops)
HBM_BPS = 8.0e12
ATOMIC_BPS = 1.3e12
KERNELS = {                            # rocprofv3 kernel-name fragment -> label
    "three_nn_lds_kernel<2>": "three_nn_lds2", "three_nn_lds_kernel<1>": "three_nn_lds1", "three_nn_scalar_kernel": "three_nn_scalar",
    "interp_cm_kernel": "interp_cm", "interp_pm_kernel<4>": "interp_pm", "interp_grad_pm_kernel": "grad_pm",
    "interp_grad_cm_kernel": "grad_cm",
}


def child(shape_ids, iters, with_torch):
    sys.path.insert(0, ROOT)
    import sad_amd  # noqa: F401  (before torch: the package owns GPU_MAX_HW_QUEUES)
    import torch
    from sad_amd import _lib, ops
    from sad_amd.fp_module import FPModule
    dev = torch.device("cuda:0")
    L = _lib.lib()
    st = lambda: torch.cuda.current_stream().cuda_stream  # noqa: E731

    def timed(fn, n=iters, warm=3):
        for _ in range(warm):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / n

    res = {}
    for si in shape_ids:
        n, m = SHAPES[si]
        g = torch.Generator(device=dev).manual_seed(si)
        unk = torch.rand((B, n, 3), device=dev, generator=g) * 50
        kn = torch.rand((B, m, 3), device=dev, generator=g) * 50
        feat_cm = torch.randn((B, C, m), device=dev, generator=g)
        feat_pm = feat_cm.transpose(1, 2).contiguous()
        r = {}
        for v, name in ((0, "three_nn_lds1"), (1, "three_nn_scalar"), (2, "three_nn_lds2")):
            _lib.set_option("nn_variant", v)
            r[name] = timed(lambda: ops.three_nn(unk, kn))
        _lib.set_option("nn_variant", 0)
        _, idx, w = ops.three_nn(unk, kn)
        r["interp_cm"] = timed(lambda: ops.three_interpolate(feat_cm, idx, w))
        r["interp_pm"] = timed(lambda: ops.three_interpolate(feat_pm, idx, w, point_major=True))
        gout_cm = torch.randn((B, C, n), device=dev, generator=g)
        gout_pm = gout_cm.transpose(1, 2).contiguous()
        gbuf = torch.zeros((B, m, C), device=dev)       # accumulates over the repeats: the values do not matter here
        r["grad_cm"] = timed(lambda: _lib.check(L.sad_three_interpolate_grad_f32(gout_cm.data_ptr(), idx.data_ptr(), w.data_ptr(), B, C, n, m, 0,
                                                                                 gbuf.data_ptr(), st()), "grad"))
        r["grad_pm"] = timed(lambda: _lib.check(L.sad_three_interpolate_grad_f32(gout_pm.data_ptr(), idx.data_ptr(), w.data_ptr(), B, C, n, m, 1,
                                                                                 gbuf.data_ptr(), st()), "grad"))
        fp = FPModule(C, C, (C, C), dev, seed=0)
        skip_pm = torch.randn((B, n, C), device=dev, generator=g)
        r["fp_module_pm"] = timed(lambda: fp.forward_pm(unk, kn, skip_pm, feat_pm))
        if with_torch:          # context only: the composition a torch code base writes (cdist + topk + gather)
            def torch_fp():
                d, j = torch.topk(torch.cdist(unk, kn), 3, dim=2, largest=False)
                rr = 1.0 / (d + 1e-8)
                ww = rr / rr.sum(2, keepdim=True)
                f = feat_pm[torch.arange(B, device=dev)[:, None, None], j]          # gather: [B,n,3,C]
                return (f * ww.unsqueeze(-1)).sum(2)
            r["torch_cdist_topk_gather"] = timed(torch_fp, n=3, warm=1)
        res[f"n{n}_m{m}"] = r
        del fp, unk, kn, feat_cm, feat_pm, gout_cm, gout_pm, gbuf, skip_pm, idx, w
        torch.cuda.empty_cache()
    print("FP_CHILD " + json.dumps(res), flush=True)


def _run(cmd, tmo):
    p = subprocess.run(["timeout", "-k", "10", str(tmo)] + cmd, cwd=ROOT, capture_output=True, text=True)
    if p.returncode != 0:
        sys.stderr.write(p.stdout[-2000:] + p.stderr[-2000:])
        raise SystemExit(f"step failed ({p.returncode}): {' '.join(cmd[:3])} ...")
    return p.stdout


def kernel_stats(si, workdir):
    d = os.path.join(workdir, f"prof{si}")
    _run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--",
          sys.executable, os.path.abspath(__file__), "--child", "--shape", str(si), "--iters", "5", "--no-torch"], 400)
    files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
    out = {}
    for f in files:
        for row in csv.DictReader(open(f)):
            for frag, label in KERNELS.items():
                if frag in row["Name"].replace(" ", ""):
                    out[label] = round(float(row["AverageNs"]) / 1e3, 2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--shape", type=int, default=None)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--no-prof", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.child:
        child([a.shape] if a.shape is not None else list(range(len(SHAPES))), a.iters, not a.no_torch)
        return
    line = [ln for ln in _run([sys.executable, os.path.abspath(__file__), "--child"], 500).splitlines() if ln.startswith("FP_CHILD ")]
    events = json.loads(line[-1][len("FP_CHILD "):])
    kern = {}
    if not a.no_prof:
        with tempfile.TemporaryDirectory() as wd:
            for si, (n, m) in enumerate(SHAPES):
                kern[f"n{n}_m{m}"] = kernel_stats(si, wd)
    result = {"B": B, "C": C, "bounds": {"three_nn": "VALU (9 ops/pair at 78.65 T lane-ops/s)",
                                         "interp": "HBM 8.0 TB/s (output + known table)", "grad": "float atomics 1.3 TB/s of added bytes"},
              "shapes": {}}
    for n, m in SHAPES:
        key = f"n{n}_m{m}"
        bound = {"three_nn": B * n * m * 9 / VALU_OPS_PER_S * 1e6,
                 "interp": B * C * (n + m) * 4 / HBM_BPS * 1e6,
                 "grad": B * n * C * 3 * 4 / ATOMIC_BPS * 1e6}
        ev, kt = events[key], kern.get(key, {})
        s = {"events_us": {k: round(v, 2) for k, v in ev.items()}, "kernel_us": kt,
             "bound_us": {k: round(v, 2) for k, v in bound.items()}, "fraction_of_bound": {}}
        for label, kind in (("three_nn_lds2", "three_nn"), ("three_nn_scalar", "three_nn"), ("three_nn_lds1", "three_nn"),
                            ("interp_cm", "interp"), ("interp_pm", "interp"), ("grad_cm", "grad"), ("grad_pm", "grad")):
            t = kt.get(label, ev.get(label))
            if t:
                s["fraction_of_bound"][label] = round(bound[kind] / t, 3)
        result["shapes"][key] = s
    txt = json.dumps(result)
    if a.out:
        with open(a.out, "w") as f:
            f.write(txt + "\n")
    print(txt)


if __name__ == "__main__":
    main()
