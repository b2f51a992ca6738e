"""Point head timings (SPEC.md §31) -> profiles/point_head_bench.json, at two shapes

  * detector   B = 32, M = 256,    G = 40, C = 3: the size-adaptive layer's candidates (K = 256)
  * per_point  B = 32, M = 16 384, G = 40, C = 3: a per-point head on the raw scene

each timed two ways in the same process, back to back:
  (a) fused     ops.point_targets, then ops.point_head_loss (the four losses AND grad_o, grad_c): 1 + 3 launches and a memset
  (b) torch     the composition they replace, written here: the [B,M,G] point-in-box test in both widths, first-hit argmax,
                gathers of the matched box, centre-ness, the three targets; then BCE against the centre-ness, smooth-L1 with the
                sine difference and the clamps, masks instead of nonzero() so that nothing synchronises, forward + backward
                through autograd.  Its kernel launches are counted with torch.profiler on one call (null if that fails)

Method: as tools/dense_loss_bench.py.  Warm-up, then REPEATS rounds in which the forms ALTERNATE, each timed by HIP events
around ITERS back-to-back calls; median and min..max per form.  call_us = the calls issued on an idle stream (the host's cost
of a call); us = the same calls queued BEHIND blocker copies that outlast the host's issuing (checked: host_ahead), so the
events bracket device time only.  Nothing but the package and torch is read.
    python tools/point_head_bench.py [--batch 32] [--iters 20] [--repeats 7]"""
import argparse
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ANCHORS = ((3.9, 1.6, 1.56), (0.8, 0.6, 1.73), (1.76, 0.6, 1.73))
SHIFT_MAX, EXTRA, BETA = 2.0, 0.2, 1.0 / 9.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "point_head_bench.json"))
    a = ap.parse_args()
    import sad_amd  # noqa: F401
    import torch
    import torch.nn.functional as tf
    from sad_amd import ops
    dev = torch.device("cuda:0")
    B, G, C = a.batch, 40, 3

    blk_src = torch.empty(128 * 1024 * 1024, dtype=torch.float32, device=dev).normal_()      # 512 MiB
    blk_dst = torch.empty_like(blk_src)

    def span(fn, iters, head_start_us=0.0):
        """us per call of `iters` calls between two events; with a head start, behind that many us of blocker copies."""
        for _ in range(int(math.ceil(head_start_us / blk_us)) if head_start_us else 0):
            blk_dst.copy_(blk_src)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        ahead = not e0.query()                                # the device has not reached e0: the host was ahead throughout
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / iters, ahead

    for _ in range(2):
        blk_dst.copy_(blk_src)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(4):
        blk_dst.copy_(blk_src)
    e1.record()
    torch.cuda.synchronize()
    blk_us = e0.elapsed_time(e1) * 1e3 / 4

    def timed(forms, iters):
        for fn in forms.values():
            for _ in range(2):
                fn()
        torch.cuda.synchronize()
        call, devt, ok = {k: [] for k in forms}, {k: [] for k in forms}, {k: True for k in forms}
        for _ in range(a.repeats):
            for k, fn in forms.items():                       # alternate the forms
                call[k].append(span(fn, iters)[0])
            for k, fn in forms.items():
                t, ahead = span(fn, iters, 1.5 * call[k][-1] * iters + 500.0)
                devt[k].append(t)
                ok[k] = ok[k] and ahead
        out = {}
        for k in forms:
            c, d = sorted(call[k]), sorted(devt[k])
            out[k] = {"us": round(d[len(d) // 2], 1), "min_us": round(d[0], 1), "max_us": round(d[-1], 1), "host_ahead": ok[k],
                      "call_us": round(c[len(c) // 2], 1), "iters": iters}
        return out

    def launches(fn):
        try:
            from torch.profiler import ProfilerActivity, profile
            fn()
            torch.cuda.synchronize()
            with profile(activities=[ProfilerActivity.CUDA]) as prof:
                fn()
                torch.cuda.synchronize()
            return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA)
        except Exception:                                      # the count is a side figure: the timings do not depend on it
            return None

    an = torch.tensor(ANCHORS, device=dev)
    sa = an[0]

    def torch_targets(xyz, cand, gt, gl):
        valid = (gl >= 0) & (gl < C) & (gt[..., 3:6] > 0).all(-1)
        ctr, ext, yaw = gt[..., :3], gt[..., 3:6], gt[..., 6]
        s, c = yaw.sin()[:, None], yaw.cos()[:, None]
        d = xyz[:, :, None, :] - ctr[:, None]
        lx, ly, dz = d[..., 0] * c + d[..., 1] * s, d[..., 1] * c - d[..., 0] * s, d[..., 2]

        def inside(e):
            h = (0.5 * (ext + 2 * e))[:, None]
            return (lx.abs() < h[..., 0]) & (ly.abs() < h[..., 1]) & (dz.abs() <= h[..., 2]) & valid[:, None]

        in0, band = inside(0.0), inside(EXTRA)
        hit, j = in0.any(-1), in0.to(torch.uint8).argmax(-1)
        cls = gl.gather(1, j)
        labels = torch.where(hit, cls, torch.where(band.any(-1), -2, -1).to(gl.dtype))
        m = gt.gather(1, j[..., None].expand(-1, -1, gt.shape[-1]))
        dq = cand - m[..., :3]
        sm, cm = m[..., 6].sin(), m[..., 6].cos()
        loc = torch.stack([dq[..., 0] * cm + dq[..., 1] * sm, dq[..., 1] * cm - dq[..., 0] * sm, dq[..., 2]], -1)
        half = 0.5 * m[..., 3:6]
        f, bk = half + loc, half - loc
        mn, mx = torch.minimum(f, bk).clamp(min=0), torch.maximum(f, bk)
        ratio = torch.where(mx > 0, mn / mx.clamp(min=1e-12), torch.zeros_like(mn))
        h1 = hit[..., None]
        cent = torch.where(hit, ratio.prod(-1).pow(1.0 / 3.0), torch.zeros_like(lx[..., 0]))
        shift = torch.where(h1, (m[..., :3] - xyz).clamp(-SHIFT_MAX, SHIFT_MAX), torch.zeros_like(xyz))
        size = torch.where(h1, ((2 * m[..., 3:6] / sa - 1).clamp(min=0).sqrt() - 1).clamp(max=1), torch.zeros_like(xyz))
        reg = torch.cat([-dq, (m[..., 3:6] / an[cls.clamp(0, C - 1).long()]).log().clamp(-2, 2), m[..., 6:7]], -1)
        return labels, torch.where(hit, j, -1), cent, shift, size, torch.where(h1, reg, torch.zeros_like(reg))

    def smooth_l1(d):
        ad = d.abs()
        return torch.where(ad < BETA, 0.5 * ad * ad / BETA, ad - 0.5 * BETA)

    def torch_loss(o, cc, labels, cent, reg_t, shift_t, size_t):
        pos, live = labels >= 0, labels != -2
        n = pos.sum(1).clamp(min=1).to(o.dtype)
        hot = tf.one_hot(labels.clamp(min=0).long(), C).to(o.dtype) * (pos.to(o.dtype) * cent)[..., None]
        l_cls = (tf.binary_cross_entropy_with_logits(o[..., :C], hot, reduction="none").sum(-1) * live).sum(1) / n
        r = o[..., C:]
        d = torch.cat([r[..., :3] - reg_t[..., :3], r[..., 3:6].clamp(-2, 2) - reg_t[..., 3:6], torch.sin(r[..., 6:] - reg_t[..., 6:])], -1)
        l_reg = (smooth_l1(d).sum(-1) * pos).sum(1) / n
        l_shift = (smooth_l1(cc[..., :3].clamp(-SHIFT_MAX, SHIFT_MAX) - shift_t).sum(-1) * pos).sum(1) / n
        l_size = (smooth_l1(cc[..., 3:].clamp(-1, 1) - size_t).sum(-1) * pos).sum(1) / n
        return torch.stack([l_cls, l_reg, l_shift, l_size], 1)

    out = []
    for name, M, iters in (("detector", 256, a.iters * 5), ("per_point", 16384, a.iters)):
        rng = np.random.default_rng(M)
        gt = np.zeros((B, G, 7), np.float32)
        gt[..., 0], gt[..., 1], gt[..., 2] = rng.uniform(0, 70.4, (B, G)), rng.uniform(-40, 40, (B, G)), rng.normal(-1.0, 0.1, (B, G))
        gl = rng.integers(0, C, (B, G)).astype(np.int32)
        gl[:, -4:] = -1                                                              # padded lists
        gt[..., 3:6] = np.asarray(ANCHORS, np.float32)[np.clip(gl, 0, C - 1)] * rng.uniform(0.8, 1.25, (B, G, 3))
        gt[..., 6] = rng.uniform(-3.14, 3.14, (B, G))
        # 30 % of the points in the boxes (SPEC.md §12's scenes), the rest on the ground
        near = rng.integers(0, G - 4, (B, M))
        ctr = np.take_along_axis(gt[..., :3], near[..., None], 1)
        pts = np.where(rng.random((B, M, 1)) < 0.3, ctr + rng.normal(0, 0.7, (B, M, 3)),
                       np.stack([rng.uniform(0, 70.4, (B, M)), rng.uniform(-40, 40, (B, M)), rng.normal(-1.6, 0.1, (B, M))], -1)).astype(np.float32)
        xyz = torch.from_numpy(pts).to(dev)
        cand = xyz + (torch.randn(B, M, 3, device=dev) * 0.3).clamp(-SHIFT_MAX, SHIFT_MAX)
        gtt, glt = torch.from_numpy(gt).to(dev), torch.from_numpy(gl).to(dev)
        o = torch.randn(B, M, C + 7, device=dev)
        cc = torch.randn(B, M, 6, device=dev) * 0.5
        tbuf = tuple(torch.empty(shape, dtype=dt, device=dev) for _, shape, dt in ops.point_output_spec(B, M))
        lbuf = tuple(torch.empty(shape, dtype=dt, device=dev) for _, shape, dt in ops.point_loss_output_spec(B, M, C, True, False))
        ws = ops.point_head_loss_workspace(B, M, dev)

        def fused():
            t = ops.point_targets(xyz, cand, gtt, glt, anchors=ANCHORS, size_anchor=ANCHORS[0], shift_max=SHIFT_MAX, extra_width=EXTRA, out=tbuf)
            return ops.point_head_loss(o, cc, t[0], t[2], t[5], t[3], t[4], beta=BETA, shift_max=SHIFT_MAX, out=lbuf, workspace=ws)

        o_t, c_t = o.clone().requires_grad_(), cc.clone().requires_grad_()

        def plain():
            with torch.no_grad():
                t = torch_targets(xyz, cand, gtt, glt)
            o_t.grad = c_t.grad = None
            loss = torch_loss(o_t, c_t, t[0], t[2], t[5], t[3], t[4])
            loss.sum().backward()
            return loss

        # the two forms agree (a sanity check of the composition, not a parity test: tests/test_gpu_point_head.py is that)
        lf, lt = fused()[0], plain()
        torch.cuda.synchronize()
        agree = bool(torch.allclose(lf, lt.detach(), rtol=1e-3, atol=1e-4))
        npos = int(fused()[1].sum())
        res = timed({"fused": fused, "torch": plain}, iters)
        res["fused"]["launches"] = "1 + 3 and a memset"
        res["torch"]["launches"] = launches(plain)
        row = {"shape": name, "B": B, "M": M, "G": G, "C": C, "positives": npos, "forms_agree": agree, **res,
               "speedup": round(res["torch"]["us"] / res["fused"]["us"], 1)}
        print(json.dumps(row))
        out.append(row)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
