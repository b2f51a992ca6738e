"""Dense head target assignment timings (SPEC.md §26) -> profiles/dense_target_bench.json, on

  * second    SECOND's KITTI shape: B = 4, 200 x 176 cells, 3 sizes x 2 rotations, G = 32 boxes per scene, nb = 2
  * center    a CenterPoint map:    B = 4, 468 x 468 cells, C = 3, G = 200 boxes per scene

each timed three ways in the same process, back to back:
  (a) fused     ops.anchor_targets / ops.center_targets
  (b) torch     the composition it replaces, written here.  Anchor head: materialised anchors, a [K_c, G] nearest-BEV IoU
                matrix per class (the per-class loop of SECOND's assigner, batched over the scenes, masks instead of
                nonzero() so that nothing synchronises), max / argmax / forced test / gather / residual encoding.  Centre
                head: the radii on the host (numpy), then one Gaussian patch per box drawn into the device map with
                torch.maximum, box by box
  (c) copy      a plain device copy that moves the call's compulsory traffic (ground truth read once + outputs written
                once; the copy reads half of those bytes and writes half): the streaming bound achievable here

Method: as tools/dense_head_bench.py.  Warm-up, then REPEATS rounds in which the forms ALTERNATE, each timed by HIP events
around ITERS back-to-back calls (the per-box loop: ITERS / 10); median and min..max per form.  call_us = the calls issued on an
idle stream (the host's cost of a call); us = the same calls queued BEHIND blocker copies that outlast the host's issuing
(checked: host_ahead), so the events bracket device time only.
    python tools/dense_target_bench.py [--batch 4] [--iters 50] [--repeats 9]"""
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
POS_THR, NEG_THR = [0.6, 0.5, 0.5], [0.45, 0.35, 0.35]
DIR_OFFSET = 0.78539


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dense_target_bench.json"))
    a = ap.parse_args()
    import sad_amd  # noqa: F401
    import torch
    from sad_amd import dense_head, ops
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

    def timed(forms, slow=()):
        for fn in forms.values():
            for _ in range(2):
                fn()
        torch.cuda.synchronize()
        call, devt, ok = {k: [] for k in forms}, {k: [] for k in forms}, {k: True for k in forms}
        its = {k: max(2, a.iters // 10) if k in slow else a.iters for k in forms}
        for _ in range(a.repeats):
            for k, fn in forms.items():                       # alternate the forms
                call[k].append(span(fn, its[k])[0])
            for k, fn in forms.items():
                t, ahead = span(fn, its[k], 1.5 * call[k][-1] * its[k] + 500.0)
                devt[k].append(t)
                ok[k] = ok[k] and ahead
        out = {}
        for k in forms:
            c, d = sorted(call[k]), sorted(devt[k])
            out[k] = {"us": round(d[len(d) // 2], 1), "min_us": round(d[0], 1), "max_us": round(d[-1], 1), "host_ahead": ok[k],
                      "call_us": round(c[len(c) // 2], 1), "iters": its[k]}
        return out

    def copier(nbytes):
        src = torch.empty(max(nbytes // 8, 1), dtype=torch.float32, device=dev).normal_()
        dst = torch.empty_like(src)
        return lambda: dst.copy_(src)

    out = []
    # ---- SECOND's KITTI shape -------------------------------------------------------------------------------------------
    H, W, ns, nr, G, nb = 200, 176, 3, 2, 32, 2
    A, HW = ns * nr, 200 * 176
    K = HW * A
    origin, step = dense_head.anchor_grid(KITTI_RANGE, H, W)
    lab_np = rng.integers(0, ns, (B, G)).astype(np.int32)
    lab_np[:, G - 4:] = -1                                                    # padding rows
    gt_np = np.zeros((B, G, 7), np.float32)
    gt_np[..., 0], gt_np[..., 1] = rng.uniform(0, 70.4, (B, G)), rng.uniform(-40, 40, (B, G))
    gt_np[..., 2] = rng.uniform(-2, 0, (B, G))
    gt_np[..., 3:6] = np.asarray(SIZES, np.float32)[np.maximum(lab_np, 0)] * rng.uniform(0.8, 1.2, (B, G, 3))
    gt_np[..., 6] = rng.uniform(-math.pi, math.pi, (B, G))
    gt, lab = torch.from_numpy(gt_np).to(dev), torch.from_numpy(lab_np).to(dev)
    asg = dense_head.AnchorHeadDecoder(SIZES, Z_CENTER, ROTATIONS, origin, step).assigner(POS_THR, NEG_THR, [0, 1, 2], nb=nb)
    xs = origin[0] + torch.arange(W, dtype=torch.float32, device=dev) * step[0]
    ys = origin[1] + torch.arange(H, dtype=torch.float32, device=dev) * step[1]
    anc = torch.zeros(H, W, ns, nr, 7, device=dev)
    anc[..., 0], anc[..., 1] = xs[None, :, None, None], ys[:, None, None, None]
    anc[..., 2] = torch.tensor(Z_CENTER, device=dev)[None, None, :, None]
    anc[..., 3:6] = torch.tensor(SIZES, device=dev)[None, None, :, None, :]
    anc[..., 6] = torch.tensor(ROTATIONS, device=dev)[None, None, None, :]
    anc = anc.view(HW, ns, nr, 7)
    period = 2 * math.pi / nb

    def rect(b):
        yaw = b[..., 6]
        ang = torch.abs(yaw - torch.floor(yaw / math.pi + 0.5) * math.pi)
        keep = ang < math.pi / 4
        ex, ey = torch.where(keep, b[..., 3], b[..., 4]), torch.where(keep, b[..., 4], b[..., 3])
        return b[..., 0] - ex * 0.5, b[..., 0] + ex * 0.5, b[..., 1] - ey * 0.5, b[..., 1] + ey * 0.5

    def fused():
        return asg(gt, lab, H, W)

    def composed():
        labels = torch.empty(B, HW, ns, nr, dtype=torch.int32, device=dev)
        match, dirt = torch.empty_like(labels), torch.empty_like(labels)
        regt = torch.empty(B, HW, ns, nr, 7, device=dev)
        miou = torch.empty(B, HW, ns, nr, device=dev)
        gx0, gx1, gy0, gy1 = (v[:, None, :] for v in rect(gt))                 # [B,1,G]
        garea = (gx1 - gx0) * (gy1 - gy0)
        for s in range(ns):                                                   # the per-class loop
            an = anc[:, s].reshape(HW * nr, 7)                                # this class's anchors [K_c,7]
            ax0, ax1, ay0, ay1 = (v[None, :, None] for v in rect(an))         # [1,K_c,1]
            ix = (torch.minimum(ax1, gx1) - torch.maximum(ax0, gx0)).clamp_(min=0)
            iy = (torch.minimum(ay1, gy1) - torch.maximum(ay0, gy0)).clamp_(min=0)
            inter = ix * iy
            iou = inter / ((ax1 - ax0) * (ay1 - ay0) + garea - inter).clamp_(min=1e-6)      # [B,K_c,G]
            elig = (lab == s)[:, None, :]
            has = elig.any(-1)
            m, j = torch.where(elig, iou, -1.0).max(-1)
            m = torch.where(has, m, 0.0)
            best = torch.where(elig, iou, 0.0).amax(1, keepdim=True)
            forced = (elig & (best > 0) & (iou == best)).any(-1)
            pos = forced | (has & (m >= POS_THR[s]))
            lb = torch.where(pos, torch.gather(lab, 1, j), torch.where(~has | (m < NEG_THR[s]), -1, -2).int())
            g = torch.gather(gt, 1, j[..., None].expand(-1, -1, 7))
            av = an[None]
            dg = torch.sqrt(av[..., 3] ** 2 + av[..., 4] ** 2)
            t = torch.stack([(g[..., 0] - av[..., 0]) / dg, (g[..., 1] - av[..., 1]) / dg, (g[..., 2] - av[..., 2]) / av[..., 5],
                             torch.log(g[..., 3].clamp(min=1e-5) / av[..., 3]), torch.log(g[..., 4].clamp(min=1e-5) / av[..., 4]),
                             torch.log(g[..., 5].clamp(min=1e-5) / av[..., 5]), g[..., 6] - av[..., 6]], -1)
            v = g[..., 6] - DIR_OFFSET
            o = v - torch.floor(v / (2 * math.pi)) * (2 * math.pi)
            d = torch.floor(o / period).clamp_(0, nb - 1).int()
            labels[:, :, s] = lb.view(B, HW, nr)
            match[:, :, s] = torch.where(pos, j.int(), -1).view(B, HW, nr)
            dirt[:, :, s] = torch.where(pos, d, -1).view(B, HW, nr)
            regt[:, :, s] = torch.where(pos[..., None], t, 0.0).view(B, HW, nr, 7)
            miou[:, :, s] = m.view(B, HW, nr)
        return labels.view(B, K), match.view(B, K), regt.view(B, K, 7), miou.view(B, K), dirt.view(B, K)

    f, c = fused(), composed()
    same = [float((x == y).float().mean()) for x, y in ((f[0], c[0]), (f[1], c[1]), (f[4], c[4]))]
    traffic = B * G * 8 * 4 + B * K * 11 * 4
    rec = dict(case="second", B=B, H=H, W=W, A=A, G=G, nb=nb, K=K, traffic_bytes=traffic, positives=int((f[0] >= 0).sum()),
               ignored=int((f[0] == -2).sum()), labels_match_dir_equal_fraction=[round(v, 6) for v in same],
               agree=bool(min(same) > 0.9999 and torch.allclose(f[3], c[3], atol=1e-5) and torch.allclose(f[2], c[2], atol=1e-3)))
    rec.update(timed({"fused": fused, "torch": composed, "copy": copier(traffic)}))
    out.append(rec)
    print(json.dumps(rec), flush=True)
    del anc, f, c

    # ---- a CenterPoint map ----------------------------------------------------------------------------------------------
    H = W = 468
    C, G = 3, 200
    lo, cell = (-54.0, -54.0), (0.24, 0.24)                                    # 468 cells of 0.24 m: +-56.16 m
    lab_np = rng.integers(0, C, (B, G)).astype(np.int32)
    lab_np[:, G - 20:] = -1
    gt_np = np.zeros((B, G, 7), np.float32)
    gt_np[..., 0:2] = rng.uniform(-54.0, -54.0 + 468 * 0.24, (B, G, 2))
    gt_np[..., 2] = rng.uniform(-2, 0, (B, G))
    gt_np[..., 3], gt_np[..., 4], gt_np[..., 5] = rng.uniform(0.5, 12.0, (B, G)), rng.uniform(0.5, 3.0, (B, G)), rng.uniform(1, 3, (B, G))
    gt_np[..., 6] = rng.uniform(-math.pi, math.pi, (B, G))
    gt, lab = torch.from_numpy(gt_np).to(dev), torch.from_numpy(lab_np).to(dev)
    casg = dense_head.CenterHeadDecoder(lo, cell).assigner(C)

    def cfused():
        return casg(gt, lab, H, W)

    def radius(h, w, mo=0.1):
        r1 = ((h + w) + np.sqrt((h + w) ** 2 - 4 * w * h * (1 - mo) / (1 + mo))) / 2
        r2 = (2 * (h + w) + np.sqrt(4 * (h + w) ** 2 - 16 * (1 - mo) * w * h)) / 2
        r3 = (-2 * mo * (h + w) + np.sqrt((2 * mo * (h + w)) ** 2 - 16 * mo * (mo - 1) * w * h)) / 2
        return np.minimum(np.minimum(r1, r2), r3)

    ar = torch.arange(-64, 65, dtype=torch.float32, device=dev)
    d2 = ar[:, None] ** 2 + ar[None, :] ** 2                                    # squared distances of a 129 x 129 patch

    def ccomposed():
        hm = torch.zeros(B, C, H, W, device=dev)
        fx, fy = (gt_np[..., 0] - lo[0]) / cell[0], (gt_np[..., 1] - lo[1]) / cell[1]
        rad = np.maximum(2, radius(gt_np[..., 4] / cell[1], gt_np[..., 3] / cell[0]).astype(np.int64))
        for b in range(B):
            for g in range(G):                                                # the per-box loop
                if lab_np[b, g] < 0 or not (0 <= fx[b, g] < W and 0 <= fy[b, g] < H):
                    continue
                ix, iy, r = int(fx[b, g]), int(fy[b, g]), int(min(rad[b, g], 64))
                x0, x1, y0, y1 = max(0, ix - r), min(W, ix + r + 1), max(0, iy - r), min(H, iy + r + 1)
                sigma = (2 * r + 1) / 6.0
                patch = torch.exp(d2[64 + y0 - iy:64 + y1 - iy, 64 + x0 - ix:64 + x1 - ix] * (-1.0 / (2 * sigma * sigma)))
                win = hm[b, lab_np[b, g], y0:y1, x0:x1]
                torch.maximum(win, patch, out=win)
        return hm

    fh, fi, fa = cfused()
    ch = ccomposed()
    traffic = B * G * 8 * 4 + B * C * H * W * 4 + B * G * 9 * 4
    rec = dict(case="center", B=B, H=H, W=W, C=C, G=G, traffic_bytes=traffic, assigned=int((fi >= 0).sum()),
               nonzero_cells=int((fh > 0).sum()), agree=bool(torch.allclose(fh, ch, atol=1e-4) and torch.equal(fh > 0, ch > 0)))
    rec.update(timed({"fused": cfused, "torch": ccomposed, "copy": copier(traffic)}, slow=("torch",)))
    out.append(rec)
    print(json.dumps(rec), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
