"""Dense head loss timings (SPEC.md §27) -> profiles/dense_loss_bench.json, on the shapes of tools/dense_target_bench.py

  * second    SECOND's KITTI shape: B = 4, 200 x 176 cells, A = 6 anchors, C = 3, nb = 2 (K = 211 200 rows per scene)
  * center    a CenterPoint map:    B = 4, 468 x 468 cells, C = 3, G = 200 boxes per scene

each timed three ways in the same process, back to back:
  (a) fused     ops.anchor_head_loss / ops.center_head_loss: the losses AND the gradient of every map
  (b) torch     the composition it replaces, written here, forward + backward through autograd.  Anchor head: the three maps
                permuted to [B,K,.] copies, a one-hot [B,K,C], OpenPCDet's sigmoid focal loss, smooth-L1 with the sine
                difference, cross-entropy of the direction bins, masks instead of nonzero() so that nothing synchronises.
                Centre head: the clamped-sigmoid focal loss of CenterNet and a gather + L1 at ind
  (c) copy      a plain device copy that moves the call's compulsory traffic (maps and targets read once, gradients written
                once; the copy reads half of those bytes and writes half): the streaming bound achievable here

Method: as tools/dense_target_bench.py.  Warm-up, then REPEATS rounds in which the forms ALTERNATE, each timed by HIP events
around ITERS back-to-back calls; median and min..max per form.  call_us = the calls issued on an idle stream (the host's cost
of a call); us = the same calls queued BEHIND blocker copies that outlast the host's issuing (checked: host_ahead), so the
events bracket device time only.
    python tools/dense_loss_bench.py [--batch 4] [--iters 50] [--repeats 9]"""
import argparse
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dense_loss_bench.json"))
    a = ap.parse_args()
    import sad_amd  # noqa: F401
    import torch
    import torch.nn.functional as tf
    from sad_amd import ops
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    B = a.batch

    blk_src = torch.empty(256 * 1024 * 1024, dtype=torch.float32, device=dev).normal_()      # 1 GiB
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

    def timed(forms):
        for fn in forms.values():
            for _ in range(2):
                fn()
        torch.cuda.synchronize()
        call, devt, ok = {k: [] for k in forms}, {k: [] for k in forms}, {k: True for k in forms}
        for _ in range(a.repeats):
            for k, fn in forms.items():                       # alternate the forms
                call[k].append(span(fn, a.iters)[0])
            for k, fn in forms.items():
                t, ahead = span(fn, a.iters, 1.5 * call[k][-1] * a.iters + 500.0)
                devt[k].append(t)
                ok[k] = ok[k] and ahead
        out = {}
        for k in forms:
            c, d = sorted(call[k]), sorted(devt[k])
            out[k] = {"us": round(d[len(d) // 2], 1), "min_us": round(d[0], 1), "max_us": round(d[-1], 1), "host_ahead": ok[k],
                      "call_us": round(c[len(c) // 2], 1), "iters": a.iters}
        return out

    def copier(nbytes):
        src = torch.empty(max(nbytes // 8, 1), dtype=torch.float32, device=dev).normal_()
        dst = torch.empty_like(src)
        return lambda: dst.copy_(src)

    out = []
    # ---- SECOND's KITTI shape -------------------------------------------------------------------------------------------
    H, W, A, C, nb = 200, 176, 6, 3, 2
    K = H * W * A
    alpha, beta = 0.25, 1.0 / 9.0
    kind = rng.random((B, K))
    lab_np = np.where(kind < 0.002, rng.integers(0, C, (B, K)), np.where(kind < 0.01, -2, -1)).astype(np.int32)   # ~400 positives per scene
    pos_np = lab_np >= 0
    tgt_np = np.where(pos_np[..., None], rng.normal(0, 0.5, (B, K, 7)), 0).astype(np.float32)
    dirt_np = np.where(pos_np, rng.integers(0, nb, (B, K)), -1).astype(np.int32)
    labels, tgt, dirt = (torch.from_numpy(v).to(dev) for v in (lab_np, tgt_np, dirt_np))
    cls = torch.randn(B, A * C, H, W, device=dev) * 2 - 3
    reg = torch.randn(B, A * 7, H, W, device=dev) * 0.5
    dir_ = torch.randn(B, A * nb, H, W, device=dev)
    outs = tuple(torch.empty(s, dtype=dt, device=dev) for s, dt in (((B, 3), torch.float32), ((B,), torch.int32), (tuple(cls.shape), torch.float32),
                                                                     (tuple(reg.shape), torch.float32), (tuple(dir_.shape), torch.float32)))
    ws = ops.anchor_head_loss_workspace(B, H, W, A, dev)

    def fused():
        return ops.anchor_head_loss(cls, reg, dir_, labels, tgt, dirt, alpha=alpha, beta=beta, out=outs, workspace=ws)

    tcls, treg, tdir = (m.clone().requires_grad_() for m in (cls, reg, dir_))
    lab64, dirt64 = labels.long(), dirt.long()
    pos, live = lab64 >= 0, lab64 != -2
    norm = pos.sum(1).clamp(min=1).float()

    def composed():
        for m in (tcls, treg, tdir):
            m.grad = None
        rows = lambda m: m.view(B, A, -1, H, W).permute(0, 3, 4, 1, 2).reshape(B, K, -1)  # noqa: E731
        x, r, z = rows(tcls), rows(treg), rows(tdir)
        onehot = (lab64[..., None] == torch.arange(C, device=dev)).float()
        p = torch.sigmoid(x)
        pt = onehot * (1 - p) + (1 - onehot) * p
        bce = x.clamp(min=0) - x * onehot + torch.log1p(torch.exp(-x.abs()))
        lcls = ((onehot * alpha + (1 - onehot) * (1 - alpha)) * pt * pt * bce * live[..., None]).sum((1, 2)) / norm
        sd = torch.sin(r[..., 6:]) * torch.cos(tgt[..., 6:]) - torch.cos(r[..., 6:]) * torch.sin(tgt[..., 6:])
        d = torch.cat([r[..., :6] - tgt[..., :6], sd], -1).abs()
        lreg = (torch.where(d < beta, 0.5 * d * d / beta, d - 0.5 * beta) * pos[..., None]).sum((1, 2)) / norm
        ce = tf.cross_entropy(z.reshape(-1, nb), dirt64.clamp(min=0).reshape(-1), reduction="none").view(B, K)
        ldir = (ce * pos).sum(1) / norm
        loss = torch.stack([lcls, lreg, ldir], 1)
        loss.sum().backward()
        return loss

    f, c = fused(), composed()
    agree = bool(torch.allclose(f[0], c, rtol=1e-4, atol=1e-5) and torch.allclose(f[2], tcls.grad, atol=1e-6)
                 and torch.allclose(f[3], treg.grad, atol=1e-6) and torch.allclose(f[4], tdir.grad, atol=1e-6))
    nmap = B * H * W * A * (C + 7 + nb)
    traffic = 2 * nmap * 4 + B * K * (1 + 7 + 1) * 4
    rec = dict(case="second", B=B, H=H, W=W, A=A, C=C, nb=nb, K=K, traffic_bytes=traffic, positives=int(pos.sum()), agree=agree,
               loss=[round(float(v), 6) for v in f[0][0]])
    rec.update(timed({"fused": fused, "torch": composed, "copy": copier(traffic)}))
    out.append(rec)
    print(json.dumps(rec), flush=True)
    del tcls, treg, tdir, f, c

    # ---- a CenterPoint map ----------------------------------------------------------------------------------------------
    H = W = 468
    C, G = 3, 200
    HW = H * W
    ind_np = rng.integers(0, HW, (B, G)).astype(np.int32)
    ind_np[:, G - 20:] = -1
    ind = torch.from_numpy(ind_np).to(dev)
    anno = torch.randn(B, G, 8, device=dev) * (ind >= 0)[..., None]
    heat = torch.rand(B, C, H, W, device=dev) * (torch.rand(B, C, H, W, device=dev) < 0.02)
    heat.view(B, -1)[:, rng.integers(0, C * HW, 180)] = 1.0
    hm = torch.randn(B, C, H, W, device=dev) - 3
    maps = [torch.randn(B, ch, H, W, device=dev) for ch in (2, 1, 3, 2)]
    couts = tuple(torch.empty(s, dtype=dt, device=dev) for s, dt in
                  [((B, 2), torch.float32), ((B, 2), torch.int32), (tuple(hm.shape), torch.float32)] + [(tuple(m.shape), torch.float32) for m in maps])
    cws = ops.center_head_loss_workspace(B, H, W, G, dev)

    def cfused():
        return ops.center_head_loss(hm, *maps, None, heat, ind, anno, out=couts, workspace=cws)

    thm = hm.clone().requires_grad_()
    tmaps = [m.clone().requires_grad_() for m in maps]
    one = heat == 1
    npos = one.sum((1, 2, 3)).clamp(min=1).float()
    assigned = ind >= 0
    nbox = assigned.sum(1).clamp(min=1).float()
    gidx = ind.clamp(min=0).long()[:, None, :].expand(-1, 8, -1)
    negw = (1 - heat) ** 4 * (~one)

    def ccomposed():
        for m in [thm] + tmaps:
            m.grad = None
        p = torch.sigmoid(thm).clamp(1e-4, 1 - 1e-4)
        lhm = (-torch.log(p) * (1 - p) ** 2 * one - torch.log(1 - p) * p ** 2 * negw).sum((1, 2, 3)) / npos
        pred = torch.cat([m.view(B, -1, HW) for m in tmaps], 1).gather(2, gidx).transpose(1, 2)
        lreg = ((pred - anno).abs() * assigned[..., None]).sum((1, 2)) / nbox
        loss = torch.stack([lhm, lreg], 1)
        loss.sum().backward()
        return loss

    f, c = cfused(), ccomposed()
    agree = bool(torch.allclose(f[0], c, rtol=1e-4, atol=1e-5) and torch.allclose(f[2], thm.grad, atol=1e-6)
                 and all(torch.allclose(g, m.grad, atol=1e-6) for g, m in zip(f[3:], tmaps)))
    traffic = B * C * HW * 4 * 3 + B * 8 * HW * 4 + B * G * (8 * 3 + 1) * 4       # hm, heatmap, grad_hm; the zero fill; the boxes
    rec = dict(case="center", B=B, H=H, W=W, C=C, G=G, traffic_bytes=traffic, assigned=int(assigned.sum()), ones=int(one.sum()), agree=agree,
               loss=[round(float(v), 6) for v in f[0][0]])
    rec.update(timed({"fused": cfused, "torch": ccomposed, "copy": copier(traffic)}))
    out.append(rec)
    print(json.dumps(rec), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
