"""RoI head loss timings (SPEC.md §29) -> profiles/roi_loss_bench.json, at a training shape: B = 32 scenes x S = 128 sampled RoIs
(4 096 rows), the targets made by ops.roi_targets from R = 512 RoIs and G = 64 boxes per scene (tools/roi_head_bench.py's scene),
the predictions drawn around the targets.

  (a) roi_head_loss   ops.roi_head_loss into kept outputs: the three losses AND the gradients of both predictions, one launch
  (b) torch           the replaced code's form on the same inputs in float32: binary cross-entropy, the two [fg_mask] gathers,
                      fg_sum.item(), smooth-L1, a second decode, three boxes_to_corners_3d, min of two norms, Huber; then
                      autograd's backward to the two predictions.  It normalises over the batch (what that code does); the
                      arithmetic per row is the same

Method: warm-up, then REPEATS rounds in which the two forms ALTERNATE, each timed by HIP events around ITERS back-to-back steps
that end in a device synchronise; median and min..max of the time per step.  At 4 096 rows both forms are bound by launches and
by the host, not by the device: the figure is the time of a training step's loss, not a kernel's share of peak.
    python tools/roi_loss_bench.py [--iters 50] [--repeats 9]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def corners(torch, bx):
    tpl = torch.tensor([[1, 1, -1, -1, 1, 1, -1, -1], [1, -1, -1, 1, 1, -1, -1, 1], [-1, -1, -1, -1, 1, 1, 1, 1]], dtype=bx.dtype,
                       device=bx.device).T / 2
    o = bx[:, None, 3:6] * tpl
    sn, cs = bx[:, 6, None].sin(), bx[:, 6, None].cos()
    return torch.stack([o[..., 0] * cs - o[..., 1] * sn + bx[:, 0, None], o[..., 0] * sn + o[..., 1] * cs + bx[:, 1, None],
                        o[..., 2] + bx[:, 2, None]], -1)


def torch_step(torch, x, reg, tg, gt_global, beta, cw, scale):
    """Forward and backward of the replaced code's losses; returns the two gradients."""
    x, reg = x.detach().requires_grad_(), reg.detach().requires_grad_()
    t = tg.cls_target.view(-1)
    live = (t >= 0).float()
    bce = torch.nn.functional.binary_cross_entropy_with_logits(x.view(-1), t.clamp(min=0), reduction="none")
    l_cls = (bce * live).sum() / live.sum().clamp(min=1.0) * scale[0]
    fg = tg.reg_valid.view(-1) > 0
    fg_sum = int(fg.long().sum().item())
    loss = l_cls
    if fg_sum:
        diff = (reg.view(-1, 7)[fg] - tg.reg_target.view(-1, 7)[fg]) * cw
        a = diff.abs()
        loss = loss + torch.where(a < beta, 0.5 * a * a / beta, a - 0.5 * beta).sum() / fg_sum * scale[1]
        roi, r = tg.rois_s.view(-1, 7)[fg], reg.view(-1, 7)[fg]
        la, wa, ha = roi[:, 3].clamp(min=1e-5), roi[:, 4].clamp(min=1e-5), roi[:, 5].clamp(min=1e-5)
        dg = (la * la + wa * wa).sqrt()
        s, co = roi[:, 6].sin(), roi[:, 6].cos()
        lx, ly = r[:, 0] * dg, r[:, 1] * dg
        pred = torch.stack([lx * co - ly * s + roi[:, 0], lx * s + ly * co + roi[:, 1], r[:, 2] * ha + roi[:, 2], r[:, 3].exp() * la,
                            r[:, 4].exp() * wa, r[:, 5].exp() * ha, r[:, 6] + roi[:, 6]], -1)
        gt = gt_global.view(-1, 7)[fg]
        turned = gt.clone()
        turned[:, 6] += np.pi
        pc = corners(torch, pred)
        dist = torch.minimum((pc - corners(torch, gt)).norm(dim=-1), (pc - corners(torch, turned)).norm(dim=-1))
        loss = loss + torch.where(dist < 1.0, 0.5 * dist * dist, dist - 0.5).mean(-1).sum() / fg_sum * scale[2]
    loss.backward()
    return x.grad, reg.grad


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "roi_loss_bench.json"))
    a = ap.parse_args()
    import sad_amd  # noqa: F401
    import torch
    from roi_head_bench import scene
    from sad_amd import ops, roi_head
    dev = torch.device("cuda:0")
    B, R, G, S = 32, 512, 64, 128
    rois, rl, gt, lab = (torch.from_numpy(v).to(dev) for v in scene(np.random.default_rng(0), B, R, G))
    tg = roi_head.RoiTargets(*ops.roi_targets(rois, None, rl, gt, lab, S=S, fg_max=S // 2, fg_thr=0.55, bg_lo=0.1, hard_ratio=0.8, reg_fg_thr=0.55,
                                              cls_fg_thr=0.75, cls_bg_thr=0.25, seed=1))
    g = torch.Generator(device="cpu").manual_seed(1)
    x = (torch.randn((B, S), generator=g) * 0.4).to(dev)
    reg = tg.reg_target + (torch.randn((B, S, 7), generator=g) * 0.15).to(dev)
    gt_global = torch.gather(gt, 1, tg.match.clamp(min=0).long()[..., None].expand(B, S, 7)).contiguous()
    beta, cwl, scale = 1.0 / 9.0, [1.0, 1.0, 1.0, 0.7, 0.7, 0.7, 1.3], (1.0, 2.0, 0.5)
    cw = torch.tensor(cwl, device=dev)
    out = ops.roi_head_loss(x, reg, tg.cls_target, tg.reg_valid, tg.reg_target, tg.rois_s, tg.gt_local, beta=beta, code_weights=cwl, scale=scale)
    forms = {"roi_head_loss": lambda: ops.roi_head_loss(x, reg, tg.cls_target, tg.reg_valid, tg.reg_target, tg.rois_s, tg.gt_local, beta=beta,
                                                        code_weights=cwl, scale=scale, out=out),
             "torch": lambda: torch_step(torch, x, reg, tg, gt_global, beta, cw, scale)}
    # the two forms compute the same thing: per scene against over the batch, so compare unnormalised sums
    raw = ops.roi_head_loss(x, reg, tg.cls_target, tg.reg_valid, tg.reg_target, tg.rois_s, tg.gt_local, beta=beta, code_weights=cwl, scale=scale,
                            normalize=False)
    n_cls, n_reg = int(raw[1][:, 0].sum()), int(raw[1][:, 1].sum())
    gx, gr = forms["torch"]()
    mine_x, mine_r = raw[2] / max(n_cls, 1), (raw[3] + raw[4]) / max(n_reg, 1)
    agree = max(float((gx - mine_x).abs().max()), float((gr - mine_r).abs().max()))

    def span(fn, iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / iters

    for fn in forms.values():
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in forms}
    for _ in range(a.repeats):
        for k, fn in forms.items():                           # alternate the forms
            times[k].append(span(fn, a.iters))
    rec = dict(B=B, S=S, rows=B * S, n_cls=n_cls, n_reg=n_reg, max_gradient_difference=agree, iters=a.iters, repeats=a.repeats)
    for k, v in times.items():
        v = sorted(v)
        rec[k] = {"us": round(v[len(v) // 2], 1), "min_us": round(v[0], 1), "max_us": round(v[-1], 1)}
    print(json.dumps(rec), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
