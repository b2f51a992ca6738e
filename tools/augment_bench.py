"""Training augmentation timings (SPEC.md §35) -> profiles/augment_bench.json: B = 32 ``synth`` scenes at their raw size (16 384
rows of 4 columns), G = 40 labelled boxes per scene in three classes, Q = 45 candidate slots, a database cut from eight other
scenes with ``GTDatabase.from_scenes``.

  (a) gt_paste       ``GTSampler`` into kept outputs and a kept workspace: the four launches
  (b) train_augment  ``TrainAugment``: params, paste with the transform fused, ``subsample_pad`` to 16 384 rows: six launches
  (c) composition    what a user writes from the operators that existed before: ``boxes_iou_bev`` of the candidates against the
                     ground truth and against themselves, both matrices read back, the greedy walk as a host loop,
                     ``points_in_boxes`` on the accepted boxes, a boolean mask and ``torch.cat`` per scene.  It is given the
                     candidate draw of (a) and must accept the same slots (``composition_agrees``); it applies no transform.

``--step-json``: a file written by tools/train_step_time.py in the same visit; its KITTI step time is copied in and the
augmentation's share of it is reported.  No threshold: these are first numbers of their kind.

Method: warm-up, then REPEATS rounds in which the forms ALTERNATE, each timed by HIP events around ITERS back-to-back calls that
end in a device synchronise (the composition, which synchronises by itself, gets ITERS / 50 calls per window); median and
min..max of the time per call.
    python tools/augment_bench.py [--iters 2000] [--repeats 9] [--step-json FILE]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B, G, SAMPLE_NUM, DB_SCENES, N = 32, 40, (20, 15, 10), 8, 16384


def labelled(first, count):
    from sad_amd import synth
    pts = synth.make_batch(first, count, N).reshape(-1, 4)
    gt = np.stack([synth.scene_boxes(first + i, N) for i in range(count)])
    labels = (np.arange(gt.shape[1], dtype=np.int32) % 3)[None].repeat(count, 0)
    return pts, np.arange(count + 1, dtype=np.int32) * N, gt, np.ascontiguousarray(labels)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=2000)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--step-json", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "augment_bench.json"))
    a = ap.parse_args()
    import sad_amd  # noqa: F401
    import torch
    from sad_amd import ops
    from sad_amd.augment import GTDatabase, GTSampler, GlobalAugment, TrainAugment
    if not torch.cuda.is_available():
        raise SystemExit("augment_bench: needs a GPU")
    dev = torch.device("cuda:0")
    db = GTDatabase.from_scenes(*labelled(1000, DB_SCENES), num_classes=3, device=dev, max_obj_points=512)
    pts, off, gt, gl = (torch.from_numpy(v).to(dev) for v in labelled(0, B))
    Q = sum(SAMPLE_NUM)
    sampler = GTSampler(db, SAMPLE_NUM, remove_extra_width=0.2, seed=1)
    out = sampler(pts, off, gt, gl, step=0)
    ws = ops.gt_paste_workspace(B, Q, pts.shape[0], dev)
    aug = TrainAugment(GTSampler(db, SAMPLE_NUM, remove_extra_width=0.2, seed=1), GlobalAugment(seed=2), N, seed=3)
    keep, dbi = out[0].cpu().numpy(), out[1].cpu().numpy()
    cand = db.db_boxes[torch.from_numpy(np.maximum(dbi, 0)).to(dev).long()].contiguous()            # [B,Q,7]: the draw of (a)
    gt_valid = ((gl >= 0) & (gt[..., 3:6] > 0).all(-1)).cpu().numpy()
    xyz = pts.view(B, N, 4)[..., :3].contiguous()
    e2 = 2 * 0.2
    state = {}

    def composition():
        m_gt = (ops.boxes_iou_bev(cand, gt) > 0).cpu().numpy()                  # synchronises
        m_cc = (ops.boxes_iou_bev(cand, cand) > 0).cpu().numpy()                # [q, r]: q clipped in r's frame
        acc = np.zeros((B, Q), bool)
        for b in range(B):
            kept = []
            for q in np.flatnonzero(dbi[b] >= 0):
                if not m_gt[b, q][gt_valid[b]].any() and not m_cc[b, q, kept].any():
                    kept.append(q)
            acc[b, kept] = True
        sel = torch.from_numpy(acc).to(dev)
        wide = cand.clone()
        wide[..., 3:6] = torch.where(sel[..., None], wide[..., 3:6] + e2, torch.zeros_like(wide[..., 3:6]))      # rejected: nothing inside
        inside = ops.points_in_boxes(xyz, wide) >= 0
        rows = []
        for b in range(B):
            objs = [db.db_points[db.offsets[d]:db.offsets[d + 1]] for d in dbi[b][acc[b]]]
            rows.append(torch.cat(objs + [pts[b * N:(b + 1) * N][~inside[b]]]))
        state["acc"], state["rows"] = acc, rows
        return rows

    forms = {"gt_paste": lambda: sampler(pts, off, gt, gl, step=0, out=out, workspace=ws),
             "train_augment": lambda: aug(pts, off, gt, gl, step=0),
             "composition": composition}
    composition()
    torch.cuda.synchronize()
    oo = out[6].cpu().numpy()
    agrees = bool(np.array_equal(state["acc"], keep == 1)) and all(
        torch.equal(state["rows"][b], out[5][oo[b]:oo[b + 1]]) for b in range(B))

    def span(fn, iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / iters

    for fn in forms.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in forms}
    for _ in range(a.repeats):
        for k, fn in forms.items():                           # alternate the forms
            times[k].append(span(fn, a.iters if k != "composition" else max(3, a.iters // 50)))
    rec = dict(B=B, rows_per_scene=N, Cp=4, G=G, Q=Q, sample_num=list(SAMPLE_NUM), db_objects=len(db), db_points=int(db.points.shape[0]),
               Pmax=db.Pmax, pasted_per_scene=round(float(keep.sum(1).mean()), 2), rows_out=int(oo[-1]), rows_in=int(pts.shape[0]),
               bytes_moved_MB=round((int(pts.shape[0]) + int(oo[-1])) * 16 / 1e6, 1), composition_agrees=agrees, iters=a.iters, composition_iters=max(3, a.iters // 50),
               repeats=a.repeats)
    for k, v in times.items():
        v = sorted(v)
        rec[k] = {"ms": round(v[len(v) // 2], 4), "min_ms": round(v[0], 4), "max_ms": round(v[-1], 4)}
    rec["composition_over_gt_paste"] = round(rec["composition"]["ms"] / rec["gt_paste"]["ms"], 1)
    if a.step_json:
        with open(a.step_json) as f:
            step = next(r for r in json.load(f) if r.get("config") == "KITTI")
        rec["train_step"] = {k: step[k] for k in ("B", "train_step_ms", "train_step_min_ms", "train_step_max_ms")}
        rec["train_augment_share_of_step"] = round(rec["train_augment"]["ms"] / step["train_step_ms"], 4)
    print(json.dumps(rec), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
