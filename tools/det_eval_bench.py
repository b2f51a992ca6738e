"""Detection evaluation timings (SPEC.md §36) -> profiles/det_eval_bench.json, at KITTI-val scale (3769 scenes in batches of 32,
G = 24 boxes, three classes, two IoU thresholds, "iou3d") with K = 100 and K = 500 detections per scene, and at a nuScenes-like
shape (K = 500, G = 64, ten classes, four distance thresholds, "dist").  Seeded scenes: boxes on a grid, three detections in
four on a box (jittered), the rest far away.  ONE batch of 32 scenes is made and reused for every batch of a pass: 117 updates of
32 scenes and one of its first 25, 3769 scenes in all.

  (a) det_match   one batch into kept outputs: one launch
  (b) det_ap      the rows of the whole pass (scenes x K): the key kernel, torch.sort, the AP kernel
  (c) pass        a DetectionEval over the whole split: 118 updates and compute(), host wall time including the one synchronisation
                  (MEASURED as a whole)
  (d) torch       the plain-torch composition of one batch: ops.boxes_iou3d matrix (a broadcast distance for "dist"), the matrix to
                  the host, a per-scene greedy loop in numpy; and of the whole pass's AP: sort + cumsum + cummax per (class,
                  threshold) on the device.  torch_pass_extrapolated_s is NOT a measured pass: it is the one batch's time times 3769 / 32,
                  plus the AP.

Method: warm-up, then REPEATS rounds; (a), (b) and the AP of (d) timed by HIP events around ITERS back-to-back calls that end in a
device synchronise, (c) and the matching of (d) by the host clock around a synchronised region; median and min..max.
    python tools/det_eval_bench.py [--iters 20] [--repeats 5]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SCENES, BATCH = 3769, 32
SHAPES = (dict(name="kitti_k100", K=100, G=24, C=3, metric="iou3d", thr=[[0.7, 0.5], [0.5, 0.25], [0.5, 0.25]]),
          dict(name="kitti_k500", K=500, G=24, C=3, metric="iou3d", thr=[[0.7, 0.5], [0.5, 0.25], [0.5, 0.25]]),
          dict(name="nuscenes_k500", K=500, G=64, C=10, metric="dist", thr=[[0.5, 1.0, 2.0, 4.0]] * 10))


def batch(rng, B, K, G, C):
    """det [B,K,7], scores [B,K], labels [B,K] i32, gt [B,G,7], gt_labels [B,G] i32, ignore [B,G] i32."""
    gt = np.zeros((B, G, 7))
    i = np.arange(G)
    gt[..., 0] = 10.0 * (i % 8) + rng.uniform(-1, 1, (B, G))
    gt[..., 1] = 10.0 * (i // 8) + rng.uniform(-1, 1, (B, G))
    gt[..., 2] = rng.uniform(-1.5, 0, (B, G))
    gt[..., 3:6] = np.array([3.9, 1.6, 1.56]) * rng.uniform(0.8, 1.25, (B, G, 3))
    gt[..., 6] = rng.uniform(-np.pi, np.pi, (B, G))
    gl = rng.integers(0, C, (B, G)).astype(np.int32)
    on = rng.integers(0, G, (B, K))
    det = np.take_along_axis(gt, on[..., None], 1)
    det[..., 0:3] += rng.uniform(-0.4, 0.4, (B, K, 3))
    det[..., 3:6] *= rng.uniform(0.9, 1.1, (B, K, 3))
    det[..., 6] += rng.uniform(-0.2, 0.2, (B, K))
    det[..., 1] += np.where(rng.random((B, K)) < 0.25, 500.0, 0.0)
    dl = np.take_along_axis(gl, on, 1)
    sc = rng.random((B, K))
    ign = (rng.random((B, G)) < 0.2).astype(np.int32)
    return det.astype(np.float32), sc.astype(np.float32), dl, gt.astype(np.float32), gl, ign


def host_match(val, scores, dl, gl, ign, thr, dist):
    """The per-scene greedy loop the replaced evaluators run on the host: val [B,K,G], everything numpy -> code [B,K,T]."""
    B, K, G = val.shape
    T = thr.shape[1]
    code = np.zeros((B, K, T), np.int32)
    for b in range(B):
        order = np.argsort(-scores[b], kind="stable")
        same = dl[b][:, None] == gl[b][None]
        for t in range(T):
            th = thr[dl[b], t][:, None]
            ok = same & ((val[b] < th) if dist else (val[b] > th))
            free = ign[b] == 0
            for k in order:
                v = np.where(ok[k] & free, -val[b, k] if dist else val[b, k], -np.inf)
                g = int(np.argmax(v))
                if v[g] > -np.inf:
                    code[b, k, t] = 1
                    free[g] = False
                elif (ok[k] & (ign[b] != 0)).any():
                    code[b, k, t] = -1
    return code


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "det_eval_bench.json"))
    a = ap.parse_args()
    import sad_amd  # noqa: F401
    import torch
    from sad_amd import ops
    from sad_amd.evaluate import DetectionEval
    dev = torch.device("cuda:0")

    def span(fn, iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / iters

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e6

    def stat(v, unit="us", scale=1.0):
        v = sorted(x * scale for x in v)
        return {unit: round(v[len(v) // 2], 3 if unit == "s" else 1), f"min_{unit}": round(v[0], 3 if unit == "s" else 1),
                f"max_{unit}": round(v[-1], 3 if unit == "s" else 1)}

    nb = -(-SCENES // BATCH)
    rec = dict(scenes=SCENES, batch=BATCH, batches=nb, iters=a.iters, repeats=a.repeats, shapes=[])
    for s in SHAPES:
        K, G, C, metric = s["K"], s["G"], s["C"], s["metric"]
        host = batch(np.random.default_rng(K + G), BATCH, K, G, C)
        det, sc, dl, gt, gl, ign = (torch.from_numpy(v).to(dev) for v in host)
        thr_np = np.asarray(s["thr"], np.float32)
        thr = torch.from_numpy(thr_np).to(dev)
        T = thr.shape[1]
        out = ops.det_match(det, sc, dl, None, gt, gl, ign, thr, metric=metric)
        ev = DetectionEval(C, thr_np, metric, capacity=SCENES * K)

        last = SCENES - (nb - 1) * BATCH                            # the scenes of the last, shorter batch
        tail = tuple(t[:last].contiguous() for t in (det, sc, dl, gt, gl, ign))

        def one_pass():
            ev.reset()
            for _ in range(nb - 1):
                ev.update(det, sc, dl, None, gt, gl, ign)
            ev.update(tail[0], tail[1], tail[2], None, tail[3], tail[4], tail[5])
            return ev.compute()

        res = one_pass()
        n = ev.rows
        rows = (ev.scores[:n], ev.labels[:n], ev.code[:n], ev.n_gt)
        ap_out = ops.det_ap(*rows)
        ws = ops.det_ap_workspace(n, dev)

        def torch_values():
            if metric == "dist":
                d = det[:, :, None, :2] - gt[:, None, :, :2]
                return torch.sqrt(d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1])
            return ops.boxes_iou3d(det, gt)

        def torch_match():
            return host_match(torch_values().cpu().numpy(), host[1], host[2], host[4], host[5], thr_np, metric == "dist")

        def torch_ap():
            scores, labels, code, n_gt = rows
            order = torch.argsort(scores, descending=True, stable=True)
            aps = []
            for c in range(C):
                sel = order[labels[order] == c]
                for t in range(T):
                    cd = code[sel, t]
                    cd = cd[cd != -1]
                    tp = torch.cumsum(cd == 1, 0).float()
                    prec = tp / torch.arange(1, cd.shape[0] + 1, device=dev)
                    env = torch.flip(torch.cummax(torch.flip(prec, (0,)), 0)[0], (0,))
                    rec_ = tp / n_gt[c]
                    pos = torch.searchsorted(rec_, torch.arange(1, 41, device=dev) / 40.0)
                    aps.append(torch.where(pos < env.shape[0], env[pos.clamp(max=max(env.shape[0] - 1, 0))], 0.0).mean())
            return torch.stack(aps)

        agree = bool((torch_match() == out[0].cpu().numpy()).all())
        for fn in (lambda: ops.det_match(det, sc, dl, None, gt, gl, ign, thr, metric=metric, out=out),
                   lambda: ops.det_ap(*rows, out=ap_out, workspace=ws), torch_ap):
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        times = dict(det_match=[], det_ap=[], passes=[], torch_match=[], torch_ap=[])
        for _ in range(a.repeats):                                    # alternate the forms
            times["det_match"].append(span(lambda: ops.det_match(det, sc, dl, None, gt, gl, ign, thr, metric=metric, out=out), a.iters))
            times["det_ap"].append(span(lambda: ops.det_ap(*rows, out=ap_out, workspace=ws), max(a.iters // 4, 1)))
            times["passes"].append(wall(one_pass))
            times["torch_match"].append(wall(torch_match))
            times["torch_ap"].append(span(torch_ap, 1))
        row = dict(name=s["name"], K=K, G=G, C=C, T=T, metric=metric, scenes=n // K, rows=n, mean_ap=[round(float(x), 4) for x in res["mean_ap"]],
                   host_loop_codes_equal_det_match=agree,
                   det_match_batch=stat(times["det_match"]), det_ap=stat(times["det_ap"]), pass_=stat(times["passes"], "s", 1e-6),
                   torch_match_batch=stat(times["torch_match"]), torch_ap=stat(times["torch_ap"]))
        row["pass"] = row.pop("pass_")
        row["torch_pass_extrapolated_s"] = round((row["torch_match_batch"]["us"] * SCENES / BATCH + row["torch_ap"]["us"]) * 1e-6, 3)
        rec["shapes"].append(row)
        print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
