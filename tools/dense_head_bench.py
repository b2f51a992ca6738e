"""Dense head decode timings (SPEC.md §25) -> profiles/dense_head_bench.json, on

  * second    SECOND's KITTI head: B = 4, 200 x 176 cells, 3 sizes x 2 rotations, C = 3, nb = 2 (K = 211 200 per scene)
  * center    a CenterPoint map:   B = 4, 468 x 468 cells, C = 3, with vel (K = 219 024 per scene)

each timed three ways in the same process, back to back:
  (a) fused     ops.anchor_decode / ops.center_decode on the maps as the convolution left them (nchw)
  (b) torch     the composition it replaces, written here: permute + contiguous of every map, materialised anchors,
                sigmoid / max / decode / direction fix, concatenation into rows
  (c) copy      a plain device copy that moves the call's compulsory traffic (maps read once + outputs written once; the copy
                reads half of those bytes and writes half): the streaming bound achievable here
plus one line for the index path (P = 4 096 of K = 211 200).

Method: warm-up, then REPEATS rounds in which the forms ALTERNATE, each timed by HIP events around ITERS back-to-back calls;
median and min..max per form.  Two figures per form:
  call_us     the calls issued back to back on an idle stream: what a loop around the call costs, which for a 20 us kernel
              is the HOST's time to issue it (argument checks, three output allocations, the launch)
  us          the same ITERS calls queued BEHIND a blocker (device copies sized to outlast the host's issuing, checked: the
              first event must not have been reached when the last call is issued), so the events bracket device time only:
              the kernels and the gaps between dependent launches.  The ratios of DESIGN.md are taken from these.
    python tools/dense_head_bench.py [--batch 4] [--iters 50] [--repeats 9]"""
import argparse
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KITTI_RANGE = (0.0, -40.0, -3.0, 70.4, 40.0, 1.0)
SIZES = [[3.9, 1.6, 1.56], [0.8, 0.6, 1.73], [1.76, 0.6, 1.73]]
Z_CENTER = [-1.0, -0.6, -0.6]
ROTATIONS = [0.0, 1.57]
DIR_OFFSET = 0.78539


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dense_head_bench.json"))
    a = ap.parse_args()
    import sad_amd  # noqa: F401
    import torch
    from sad_amd import dense_head, ops
    dev = torch.device("cuda:0")
    g = torch.Generator(device="cpu").manual_seed(0)
    B = a.batch

    def rnd(*shape, scale=1.0):
        return (torch.randn(*shape, generator=g) * scale).to(dev)

    blk_src = torch.empty(256 * 1024 * 1024, dtype=torch.float32, device=dev).normal_()      # 1 GiB
    blk_dst = torch.empty_like(blk_src)

    def span(fn, head_start_us=0.0):
        """us per call of ITERS calls between two events; with a head start, behind that many us of blocker copies."""
        for _ in range(int(math.ceil(head_start_us / blk_us)) if head_start_us else 0):
            blk_dst.copy_(blk_src)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.iters):
            fn()
        ahead = not e0.query()                                # the device has not reached e0: the host was ahead throughout
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / a.iters, ahead

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

    def timed(forms):
        for fn in forms.values():
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        call, devt, ok = {k: [] for k in forms}, {k: [] for k in forms}, {k: True for k in forms}
        for _ in range(a.repeats):
            for k, fn in forms.items():                       # alternate the forms
                call[k].append(span(fn)[0])
            for k, fn in forms.items():
                t, ahead = span(fn, 1.5 * call[k][-1] * a.iters + 500.0)
                devt[k].append(t)
                ok[k] = ok[k] and ahead
        out = {}
        for k in forms:
            c, d = sorted(call[k]), sorted(devt[k])
            out[k] = {"us": round(d[len(d) // 2], 1), "min_us": round(d[0], 1), "max_us": round(d[-1], 1), "host_ahead": ok[k],
                      "call_us": round(c[len(c) // 2], 1)}
        return out

    def copier(nbytes):
        src = torch.empty(nbytes // 8, dtype=torch.float32, device=dev).normal_()
        dst = torch.empty_like(src)
        return lambda: dst.copy_(src)

    def close(x, y):
        return bool(torch.allclose(x, y, rtol=1e-4, atol=1e-4, equal_nan=True))

    out = []
    # ---- SECOND's KITTI head ------------------------------------------------------------------------------------------
    H, W, ns, nr, C, nb = 200, 176, 3, 2, 3, 2
    A, K = ns * nr, 200 * 176 * 6
    cls, reg, dirm = rnd(B, A * C, H, W, scale=2.0), rnd(B, A * 7, H, W, scale=0.5), rnd(B, A * nb, H, W)
    origin, step = dense_head.anchor_grid(KITTI_RANGE, H, W)
    dec = dense_head.AnchorHeadDecoder(SIZES, Z_CENTER, ROTATIONS, origin, step)
    # the anchors OpenPCDet keeps on the device: [K, 7], sizes outer, rotations inner
    xs = origin[0] + torch.arange(W, dtype=torch.float32, device=dev) * step[0]
    ys = origin[1] + torch.arange(H, dtype=torch.float32, device=dev) * step[1]
    anc = torch.zeros(H, W, ns, nr, 7, device=dev)
    anc[..., 0], anc[..., 1] = xs[None, :, None, None], ys[:, None, None, None]
    anc[..., 2] = torch.tensor(Z_CENTER, device=dev)[None, None, :, None]
    anc[..., 3:6] = torch.tensor(SIZES, device=dev)[None, None, :, None, :]
    anc[..., 6] = torch.tensor(ROTATIONS, device=dev)[None, None, None, :]
    anc = anc.view(1, K, 7)
    period = 2 * math.pi / nb

    def fused():
        return dec(cls, reg, dirm)

    def composed():
        c = cls.permute(0, 2, 3, 1).contiguous().view(B, K, C)
        t = reg.permute(0, 2, 3, 1).contiguous().view(B, K, 7)
        d = dirm.permute(0, 2, 3, 1).contiguous().view(B, K, nb)
        xa, ya, za, la, wa, ha, ra = torch.split(anc, 1, dim=-1)
        xt, yt, zt, lt, wt, ht, rt = torch.split(t, 1, dim=-1)
        diag = torch.sqrt(la ** 2 + wa ** 2)
        boxes = torch.cat([xt * diag + xa, yt * diag + ya, zt * ha + za, torch.exp(lt) * la, torch.exp(wt) * wa, torch.exp(ht) * ha,
                           rt + ra], dim=-1)
        bins = torch.max(d, dim=-1)[1]
        v = boxes[..., 6] - DIR_OFFSET
        rot = v - torch.floor(v / period + 0.0) * period
        boxes[..., 6] = rot + DIR_OFFSET + period * bins.to(boxes.dtype)
        scores, labels = torch.max(torch.sigmoid(c), dim=-1)
        return boxes, scores, labels.int()

    fb, fs, fl = fused()
    cb, cs, cl = composed()
    traffic = B * K * (C + 7 + nb) * 4 + B * K * 9 * 4
    idx = torch.randint(0, K, (B, 4096), generator=g, dtype=torch.int32).to(dev)
    rec = dict(case="second", B=B, H=H, W=W, A=A, C=C, nb=nb, K=K, traffic_bytes=traffic,
               agree=close(fb, cb) and close(fs, cs) and bool((fl == cl).float().mean() > 0.9999))
    rec.update(timed({"fused": fused, "torch": composed, "copy": copier(traffic), "index4096": lambda: dec(cls, reg, dirm, index=idx)}))
    out.append(rec)
    print(json.dumps(rec), flush=True)
    del cls, reg, dirm, anc, fb, cb

    # ---- a CenterPoint map ----------------------------------------------------------------------------------------------
    H = W = 468
    C, K = 3, 468 * 468
    hm, r2, hg = rnd(B, C, H, W, scale=2.0), torch.rand(B, 2, H, W, generator=g).to(dev), rnd(B, 1, H, W)
    dm, rt, vl = rnd(B, 3, H, W, scale=0.5), rnd(B, 2, H, W), rnd(B, 2, H, W)
    cdec = dense_head.CenterHeadDecoder(origin=(-54.0, -54.0), cell=(0.6, 0.6))
    pdec = dense_head.CenterHeadDecoder(origin=(-54.0, -54.0), cell=(0.6, 0.6), peak=True)
    gx = torch.arange(W, dtype=torch.float32, device=dev).view(1, 1, W).expand(B, H, W)
    gy = torch.arange(H, dtype=torch.float32, device=dev).view(1, H, 1).expand(B, H, W)

    def cfused():
        return cdec(hm, r2, hg, dm, rt, vl)

    def cpeak():
        return pdec(hm, r2, hg, dm, rt, vl)

    def ccomposed():
        h = torch.sigmoid(hm).permute(0, 2, 3, 1).contiguous().view(B, K, C)
        scores, labels = torch.max(h, dim=-1)
        rg = r2.permute(0, 2, 3, 1).contiguous().view(B, K, 2)
        hh = hg.permute(0, 2, 3, 1).contiguous().view(B, K, 1)
        dd = torch.exp(dm.permute(0, 2, 3, 1).contiguous().view(B, K, 3))
        rr = rt.permute(0, 2, 3, 1).contiguous().view(B, K, 2)
        vv = vl.permute(0, 2, 3, 1).contiguous().view(B, K, 2)
        x = (gx.reshape(B, K, 1) + rg[..., 0:1]) * 0.6 + -54.0
        y = (gy.reshape(B, K, 1) + rg[..., 1:2]) * 0.6 + -54.0
        yaw = torch.atan2(rr[..., 0:1], rr[..., 1:2])
        return torch.cat([x, y, hh, dd, yaw, vv], dim=-1), scores, labels.int()

    fb, fs, fl = cfused()
    cb, cs, cl = ccomposed()
    traffic = B * K * (C + 10) * 4 + B * K * 11 * 4
    rec = dict(case="center", B=B, H=H, W=W, C=C, K=K, traffic_bytes=traffic,
               agree=close(fb, cb) and close(fs, cs) and bool((fl == cl).float().mean() > 0.9999))
    rec.update(timed({"fused": cfused, "torch": ccomposed, "copy": copier(traffic), "fused_peak": cpeak}))
    out.append(rec)
    print(json.dumps(rec), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
