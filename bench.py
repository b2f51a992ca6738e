#!/usr/bin/env python3
"""bench.py — scenes/sec of the SA + size-adaptive-cluster + head path on N MI355X (one node).

    python bench.py --gpus N --steps K --warmup W        (N > 1: starts its own N ranks with torch.distributed.run)
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...

Workload (BASELINE.json metric / configs[1..3]): per GPU resident batches of 32 synthetic KITTI-shaped
16 384-point scenes -> 3-stage multi-radius SA backbone (fp32) -> size-adaptive cluster layer -> box/cls head
-> boxes[32,256,9]; with N > 1 every rank processes its own scenes (weak scaling) and ONE RCCL all_gather of the
boxes closes each step.  A step = one such pass over one batch.  Inputs are already in HBM when the timed region
starts.  The timed region ROTATES over several distinct resident batches (``--batches``, default 4): consecutive
steps never see the same scenes, the MLP geometry is tuned on batch 0 only, and the parity check is made on the
LAST batch the timed region submitted.

One JSON line on rank 0.  A plain run sets up, warms up, times the steps and prints the contract fields (metric, value,
unit, higher_is_better, dtype, ms_per_step) with the run's configuration and step-time tail.  ``--dump-outputs DIR``
writes the boxes of the last timed step to DIR/boxes.npy (float32; inputs are seeded, so two builds compare output for
output).  ``--full`` adds everything else, each a pass of its own after the timed region:
  parity_check — the boxes of the last timed step against the CPU spec-oracle on the same scenes (<= 1e-4, labels
                 exact); a failure makes the exit code non-zero;
  roofline     — the dominant kernel (the fused gather+MLP+max / MLP launches of a step) against the dense MFMA
                 peak of the dtype on EXECUTED flops, timed with HIP events on the launching stream in a
                 non-overlapped pass (one stream, no sibling batch) and corrected for the measured cost of an empty
                 event pair, so that every interval is a kernel duration;
  kernels      — fps / ball_query (HBM roofline on algorithmic bytes) from the same serial pass;
  dense_leg    — the same detector with the padding skip switched off (every grouped row computed);
  bf16_leg     — the same KITTI-shaped batches through the bf16 MFMA mode (SPEC.md §14);
  configs4_leg — BASELINE.json configs[4] on its own shape: 65 536-point nuScenes-shaped scenes, bf16, 32 per batch;
  cpu_baseline — this repository's CPU spec-oracle (the upstream reference ships no CPU path) on a bounded sample of
                 the same scenes, same host: dense SPEC path and padding-skipped.
Parity is against this repo's spec-oracle; the reference (README-only) ships no implementation.
"""
import argparse
import hashlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
# HIP multiplexes streams onto 4 hardware queues by default; this pipeline uses two main streams, up to eight
# sampling streams and the gather stream, and a 3 - 16 ms FPS kernel sharing a queue with MLP launches (or with
# another FPS chain) would serialise them (measured: six FPS chains side by side keep their single-stream time,
# eight on 8 queues take twice as long - tools/fps_concurrency.py).  Must be set before the runtime initialises;
# `import sad_amd` does the same for any other caller (3dsad-main_amd/_runtime.py).
HW_QUEUES_AT_START = os.environ.get("GPU_MAX_HW_QUEUES")      # what the process was started with (None: unset; recorded in the line)
os.environ.setdefault("GPU_MAX_HW_QUEUES", "24")

PEAK_MFMA_F32_TFLOPS = 157.3   # /opt/skills/guides/MI355X_MICROARCH.md: dense f32 MFMA
PEAK_MFMA_BF16_TFLOPS = 2500.0 # same guide: dense bf16 MFMA (not the 2:1-sparsity headline)
PEAK_HBM_GBPS = 8000.0         # HBM3E spec
PARITY_TOL = 1e-4              # BASELINE.json north_star: fp32 boxes within 1e-4
# profiles/: HBM bytes of the MLP dispatches of one step (rocprofv3 --pmc passes, tools/pmc_traffic.py), per workload;
# the first file that exists is used
TRAFFIC_FILES = {("kitti", "f32"): ("r05_pmc_traffic.json", "r04_pmc_traffic.json", "r03_pmc_traffic.json"),
                 ("kitti", "bf16"): ("r05_bf16_pmc_traffic.json", "r04_bf16_pmc_traffic.json"),
                 ("nuscenes", "bf16"): ("r05_nuscenes_bf16_pmc_traffic.json", "r04_nuscenes_bf16_pmc_traffic.json")}


def usable_cores() -> int:
    n = len(os.sched_getaffinity(0))
    try:
        q, p = open("/sys/fs/cgroup/cpu.max").read().split()
        if q != "max":
            n = max(1, min(n, int(float(q) / float(p) + 0.5)))
    except Exception:
        pass
    return n


def cpu_baseline(cfg, weights, pts, repeats: int = 2):
    """Oracle forward on the scenes ``pts``; best of ``repeats`` for the dense SPEC path and for the
    padding-skipped variant (same boxes; the arithmetic the HIP path executes).  Returns
    (record, boxes)."""
    import oracle
    cores = usable_cores()
    os.environ["OMP_NUM_THREADS"] = str(cores)
    oracle.build()
    scenes = pts.shape[0]
    best = {}
    boxes = None
    for skip in (False, True):
        for _ in range(repeats):
            t0 = time.perf_counter()
            out = oracle.detector_forward(pts, cfg, weights, skip_padding=skip)
            dt = time.perf_counter() - t0
            best[skip] = dt if skip not in best else min(best[skip], dt)
        if boxes is None:
            boxes = out
        else:
            assert (boxes == out).all(), "oracle: padding-skipped boxes differ from the dense path"
    rec = {"value": round(scenes / best[False], 4), "unit": "scenes/s", "cores": cores,
           "kind": "port (self-authored spec-oracle: the upstream reference is a 2-line README with no CPU path)",
           "value_padding_skipped": round(scenes / best[True], 4),
           "sample": f"{scenes} scenes of the last timed batch through oracle.detector_forward (C + AVX2 fmaf chains + "
                     f"OpenMP, {cores} threads, brute-force FPS / ball query), best of {repeats}.  `value` computes "
                     "every grouped row (dense SPEC path, ~13x the MLP rows the HIP path executes on these sparse "
                     "scenes); `value_padding_skipped` skips the ball-query padding rows exactly as the HIP kernels do "
                     "(identical boxes) - that is the like-for-like CPU figure"}
    return rec, boxes


def parity_check(got, want):
    """Boxes of the timed configuration vs the oracle: max relative difference and label equality."""
    import numpy as np
    n = min(got.shape[0], want.shape[0])
    g, w = got[:n].astype(np.float64), want[:n].astype(np.float64)
    rel = float((np.abs(g - w) / (1.0 + np.abs(w))).max())
    labels = bool(np.array_equal(got[:n, :, 8], want[:n, :, 8]))
    return {"scenes": int(n), "max_rel": float(f"{rel:.3e}"), "tol": PARITY_TOL, "labels_equal": labels,
            "ok": bool(rel <= PARITY_TOL and labels),
            "against": "CPU spec-oracle (oracle/sad_oracle.c) on the same scenes; parity with the upstream "
                       "reference is unpinned (README-only, no implementation)"}


DUMP_MAX_BYTES = 64 << 20


def dump_boxes(out_dir: str, boxes) -> str:
    """Write the boxes a caller of the timed path received in its last step as ``out_dir/boxes.npy`` (float32).  Above
    DUMP_MAX_BYTES a fixed, seeded sample of whole scenes is kept, in scene order, so the same arguments write the same
    rows."""
    import numpy as np
    b = np.ascontiguousarray(boxes, dtype=np.float32)
    if b.nbytes > DUMP_MAX_BYTES:
        keep = DUMP_MAX_BYTES // b[0].nbytes
        b = b[np.sort(np.random.default_rng(0).choice(b.shape[0], keep, replace=False))]
    os.makedirs(out_dir, exist_ok=True)
    path = os.path.join(out_dir, "boxes.npy")
    np.save(path, b)
    return path


def step_tail(gaps) -> dict:
    """Tail record of a timed region from its per-step completion intervals (ms): how many steps took more than twice the
    median, and the extremes — so that a run with a few very long steps (three boxes of round 4 read configs4_leg 8 - 17 % low
    under a NORMAL median) shows up in the line itself."""
    g = sorted(float(x) for x in gaps)
    if not g:
        return {}
    p50 = g[len(g) // 2]
    return {"p50": round(p50, 3), "min": round(g[0], 3), "p99": round(g[(len(g) * 99) // 100], 3), "max": round(g[-1], 3),
            "over_2x_p50": sum(1 for x in g if x > 2 * p50), "mean": round(sum(g) / len(g), 3)}


def bf16_quality(boxes_bf16, boxes_f32, idx_bf16, idx_f32) -> dict:
    """How far the bf16 mode's boxes sit from the f32 detector's on the SAME scenes (numpy arrays: boxes [B,K,9] =
    x y z l w h yaw score label; idx_* = the adaptive cluster query's index sets, one [B,K,S] array per branch).
    The bf16 mode is narrower arithmetic than the f32 path north_star specifies: this is its quality figure."""
    import numpy as np
    b, f = np.asarray(boxes_bf16, np.float64), np.asarray(boxes_f32, np.float64)
    n = b.shape[0] * b.shape[1]
    centre = np.sqrt(((b[..., 0:3] - f[..., 0:3]) ** 2).sum(-1)).ravel()
    size_abs = np.abs(b[..., 3:6] - f[..., 3:6]).max(-1).ravel()
    size_rel = (np.abs(b[..., 3:6] - f[..., 3:6]) / np.maximum(np.abs(f[..., 3:6]), 1e-6)).max(-1).ravel()
    dyaw = np.abs(np.arctan2(np.sin(b[..., 6] - f[..., 6]), np.cos(b[..., 6] - f[..., 6]))).ravel()
    dscore = np.abs(b[..., 7] - f[..., 7]).ravel()

    def q(v, p):
        return float(np.sort(v)[min(len(v) - 1, (len(v) * p) // 100)])

    differ = np.zeros(b.shape[:2], bool)
    per_branch = []
    for ib, i32 in zip(idx_bf16, idx_f32):
        d = (np.asarray(ib) != np.asarray(i32)).any(-1)
        per_branch.append(round(float(d.mean()), 5))
        differ |= d
    return {"candidates": int(n), "label_agreement": round(float((b[..., 8] == f[..., 8]).mean()), 5),
            "centre_delta_m": {"max": round(float(centre.max()), 5), "p99": round(q(centre, 99), 5), "p50": round(q(centre, 50), 6)},
            "size_delta_m": {"max": round(float(size_abs.max()), 5), "p99": round(q(size_abs, 99), 5), "p50": round(q(size_abs, 50), 6)},
            "size_delta_rel": {"max": round(float(size_rel.max()), 5), "p99": round(q(size_rel, 99), 5)},
            "yaw_delta_rad": {"max": round(float(dyaw.max()), 5), "p99": round(q(dyaw, 99), 5)},
            "score_delta": {"max": round(float(dscore.max()), 5), "p99": round(q(dscore, 99), 5)},
            "adaptive_index_sets_differ": {"share_of_candidates": round(float(differ.mean()), 5), "per_branch": per_branch},
            "against": "the f32 detector (same weights, same scenes: the last batch of the leg's timed region), both with trace on; "
                       "an index set differs when any of its nsample slots differs (a rounding flip of the predicted size moves the "
                       "adaptive radius)"}


def pipeline_parity(got, want_boxes, oracle_nms) -> dict:
    """Boxes + NMS result of the pipeline's last step vs the oracle chain on the same staged files.  ``got`` = (boxes, order,
    count) from the device, ``want_boxes`` = oracle boxes [n,K,9], ``oracle_nms(boxes) -> (keep, order, count)``."""
    import numpy as np
    boxes, order, count = got
    n = want_boxes.shape[0]
    g, w = boxes[:n].astype(np.float64), want_boxes.astype(np.float64)
    rel = float((np.abs(g - w) / (1.0 + np.abs(w))).max())
    _, o_same, c_same = oracle_nms(np.ascontiguousarray(boxes[:n]))        # the NMS kernel alone: same input, exact output
    _, o_e2e, c_e2e = oracle_nms(want_boxes)                               # end to end (boxes differ by <= 1e-4: a flip needs an IoU within that of the threshold)
    same = bool(np.array_equal(o_same, order[:n]) and np.array_equal(c_same, count[:n]))
    e2e = bool(np.array_equal(o_e2e, order[:n]) and np.array_equal(c_e2e, count[:n]))
    return {"scenes": int(n), "boxes_max_rel": float(f"{rel:.3e}"), "tol": PARITY_TOL,
            "nms_equal_on_device_boxes": same, "nms_equal_end_to_end": e2e, "kept_per_scene_mean": round(float(count[:n].mean()), 2),
            "ok": bool(rel <= PARITY_TOL and same),
            "against": "oracle.subsample_pad -> oracle.detector_forward -> oracle.nms_bev on the same staged point files"}


def executed_flops(det, points, cfg, dense=False):
    """Flops the MLP kernels execute on this batch: per grouped launch only the leading rows of each
    group up to the last sample that differs from the first (the kernel's own rule); plain launches
    (aggregation, candidate MLP, head) execute every row."""
    import torch
    from sad_amd import config as _c
    tr = {}
    det.overlap_fps, ov = False, det.overlap_fps
    try:
        det(points, trace=tr)
        torch.cuda.synchronize()
    finally:
        det.overlap_fps = ov
    B = points.shape[0]
    dims = dict(_c.mlp_layers(cfg))

    def chain(d):
        return 2 * sum(a * b for a, b in zip(d[:-1], d[1:]))

    def rows_of(idx):
        if dense:                 # every row of every group
            return idx.numel()
        diff = idx != idx[..., :1]
        pos = torch.arange(1, idx.shape[-1] + 1, device=idx.device)
        return int(torch.clamp((diff * pos).amax(-1), min=1).sum().item())

    dense_rows, exec_rows = 0, 0
    per = {}
    # algorithmic HBM bytes per chain (what a dispatch must move at least: every executed row's inputs once, every output once,
    # the weights once): a grouped chain reads per packed row its row-map entry (8 B), the point's coordinates (12 B) and
    # feature row, per group the centroid (12 B), and writes the pooled row; a plain chain reads and writes its rows
    bf = getattr(det, "dtype", "f32") == "bf16"
    per_bytes = {}

    def wbytes(d):
        return (2 if bf else 4) * sum(a * b for a, b in zip(d[:-1], d[1:]))

    feat_esz = 4                                   # the scene's own feature channels are float32 in both modes
    pool_esz = 2 if bf else 4                      # pooled rows between the branches and the aggregation layer (bf16 mode: split pooling)
    for si, st in enumerate(cfg.stages):
        name = f"sa{si + 1}"
        for bi, idx in enumerate(tr[name]["ball_idx"]):
            r = rows_of(idx)
            d = dims[f"{name}.b{bi}"]
            per[f"{name}.b{bi}"] = r * chain(d)
            per_bytes[f"{name}.b{bi}"] = r * (8 + 12 + (d[0] - 3) * feat_esz) + B * st.npoint * (12 + d[-1] * pool_esz) + wbytes(d)
            exec_rows += r
            dense_rows += idx.numel()
        if st.agg:
            d = dims[f"{name}.agg"]
            per[f"{name}.agg"] = B * st.npoint * chain(d)
            per_bytes[f"{name}.agg"] = B * st.npoint * (d[0] * pool_esz + d[-1] * (2 if bf else 4)) + wbytes(d)
            feat_esz = 2 if bf else 4              # a bf16 aggregation layer hands bf16 rows to the next stage (SPEC 14)
    for bi, idx in enumerate(tr["cluster"]["ball_idx"]):
        r = rows_of(idx)
        d = dims[f"cluster.b{bi}"]
        per[f"cluster.b{bi}"] = r * chain(d)
        per_bytes[f"cluster.b{bi}"] = r * (8 + 12 + (d[0] - 3) * feat_esz) + B * cfg.n_cand * (12 + d[-1] * pool_esz) + wbytes(d)
        exec_rows += r
        dense_rows += idx.numel()
    K = cfg.n_cand
    for n in ("cand", "cluster.agg", "head"):
        d = dims[n]
        per[n] = B * K * chain(d)
        # (bf16 mode: cluster.agg reads split-pooled rows and hands bf16 cluster features to the head)
        in_esz = feat_esz if n == "cand" else pool_esz
        out_esz = pool_esz if n == "cluster.agg" else 4
        per_bytes[n] = B * K * (d[0] * in_esz + d[-1] * out_esz) + wbytes(d)
    executed_flops.last_bytes = per_bytes          # (kept beside the return value: the callers unpack three values)
    return sum(per.values()), exec_rows / max(1, dense_rows), per


def flops_of(name, per_flops):
    """A merged dispatch is named "a+b+c" (fused chain: "cluster.agg+head")."""
    return sum(per_flops.get(x, 0) for x in name.split("+"))


def bytes_of(name, per_bytes):
    """Algorithmic bytes of a dispatch = the sum over its chains (a fused chain's intermediate rows are counted: an upper
    bound on its compulsory traffic, so its `frac_of_bound` is not flattered)."""
    return sum(per_bytes.get(x, 0) for x in name.split("+"))


def dispatch_bound(flops, nbytes, ms, peak_tflops):
    """Which roofline bounds a dispatch and how close it runs to it: the time its flops need at the dense MFMA peak of the
    dtype against the time its algorithmic bytes need at the HBM peak — the larger of the two is the bound (four of
    the bf16 dispatches are byte-bound launches that were graded against 2.5 PFLOP/s)."""
    t_mfma = flops / (peak_tflops * 1e12) * 1e3
    t_hbm = nbytes / (PEAK_HBM_GBPS * 1e9) * 1e3
    bound_ms = max(t_mfma, t_hbm)
    return {"bound": "mfma" if t_mfma >= t_hbm else "hbm", "mfma_ms": round(t_mfma, 5), "hbm_ms": round(t_hbm, 5),
            "algorithmic_mb": round(nbytes / 1e6, 2), "frac_of_bound": round(bound_ms / ms, 4) if ms > 0 else None}


def launch_command(argv, n, port):
    """The command a parent `python bench.py --gpus N` (N > 1, no WORLD_SIZE in the environment) runs as a CHILD process:
    one rank per GPU under torch.distributed.run, same bench.py arguments."""
    return [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}", "--master-addr", "127.0.0.1",
            "--master-port", str(port), os.path.abspath(__file__)] + list(argv)


def free_port():
    import socket
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def self_launch(cmd, env=None):
    """Run `cmd` (the torchrun command of launch_command) as a child, relay rank 0's JSON line to stdout (everything else
    the ranks print goes to stderr) and return the child's exit code.  The parent never touches the GPU: it starts a child
    process instead of exec'ing, so nothing that initialised HIP is ever replaced."""
    import subprocess
    proc = subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=None, text=True, env=env)
    line_out = None
    for line in proc.stdout:
        t = line.strip()
        rec = None
        if t.startswith("{") and t.endswith("}"):
            try:
                rec = json.loads(t)
            except ValueError:
                rec = None
        if isinstance(rec, dict) and "metric" in rec and "value" in rec:
            line_out = t                      # (the last one wins; rank 0 prints exactly one)
        else:
            sys.stderr.write(line)
    rc = proc.wait()
    if line_out is not None:
        print(line_out, flush=True)
    elif rc == 0:
        sys.stderr.write("bench.py: the ranks exited 0 but printed no result line\n")
        rc = 1
    return rc


# The device serves 24 mapped hardware queues at full speed (tools/probe/queue_budget.sh: the pipeline's 19 + the null stream + up to
# 3 more; one more -10 %, four more -24 %).  A process group brings queues of its own (RCCL's internal streams, the backend's stream
# for barriers and reductions: 3 in the one-rank rehearsal, unknown for 8 ranks), so a distributed run maps a smaller set:
# six sampling streams, no ingest stream = 13 queues.  Set by main() once the process group exists.
DISTRIBUTED = False


def default_fps_streams(dtype: str) -> int:
    """The serial FPS chain of a batch (2.0 ms KITTI, 11.9 ms nuScenes) must not bound the step, and at the start of a timed
    region the chains of the first steps should all run at once.  With the streams placed (sad_amd._runtime.placed_streams: main
    streams alone on their dispatch pipes) eight sampling streams are best everywhere (profiles/r05_stream_placement.txt):
    f32 14.5 k at the driver's setting against 14.2 - 14.3 k with 2 - 4, bf16 47.7 k against 46.8 k with 6, nuScenes-shaped
    7.05 k against 6.97 k; ten or more need more hardware queues than the device serves at full speed (37 k / 7 k).
    Six under a process group (queue budget: above): f32 15.15 against 15.2 k."""
    return 6 if DISTRIBUTED else 8


def batch_first_scene(k: int, rank: int, world: int, B: int) -> int:
    """First scene id of resident batch k on this rank: batches of different ranks and rotation slots never share a scene."""
    return (k * world + rank) * B


class Workload:
    """What one measurement runs: topology, scene generator, arithmetic, batch size and stream plan."""

    def __init__(self, config: str, scene: str, dtype: str, batch: int, fps_streams=None, main_streams: int = 2,
                 queue_depth=None, n_batches: int = 4, overlap: bool = True, first_batch: int = 0):
        self.config, self.scene, self.dtype, self.B = config, scene, dtype, batch
        self.first_batch = first_batch
        self.fps_streams = default_fps_streams(dtype) if fps_streams is None else fps_streams
        self.main_streams = main_streams
        self.queue_depth = max(6, self.fps_streams + 2) if queue_depth is None else queue_depth
        self.n_batches = max(1, n_batches)
        self.overlap = overlap

    def cfg(self):
        from sad_amd import config
        return config.KITTI if self.config == "kitti" else config.NUSCENES

    def maker(self):
        from sad_amd import synth
        if self.config == "nuscenes":
            return synth.make_nuscenes_batch
        return synth.make_batch if self.scene == "kitti" else synth.make_dense_batch

    def peak(self):
        return PEAK_MFMA_F32_TFLOPS if self.dtype == "f32" else PEAK_MFMA_BF16_TFLOPS

    def describe(self):
        cfg = self.cfg()
        return (f"{'configs[1-2]' if self.config == 'kitti' else 'configs[4]'}: batch {self.B} x {cfg.n_points}-pt "
                f"{'KITTI' if self.config == 'kitti' else 'nuScenes'}-shaped scenes per GPU"
                f"{' (DENSE variant: 20 m x 20 m extents)' if self.scene == 'dense' else ''}, "
                f"3-stage multi-radius SA backbone {'fp32' if self.dtype == 'f32' else 'bf16 (SPEC 14)'} + size-adaptive cluster layer + box head; "
                f"{self.n_batches} distinct resident batches in rotation")


def event_overhead_ms(stream, n: int = 31) -> float:
    """What an EMPTY pair of timing events measures on this stream (median of n): every per-launch interval of the serial
    pass contains it once.  On 14 - 130 us bf16 dispatches it was 17 % of the summed intervals (round 3: 0.1205 by events
    against 0.1416 from the rocprofv3 trace of the same launches)."""
    import torch
    stream.synchronize()
    vals = []
    for _ in range(n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        e1.record(stream)
        stream.synchronize()
        vals.append(e0.elapsed_time(e1))
    vals.sort()
    return vals[len(vals) // 2]


_STREAMS = {}


def shared_streams(dev, n_side: int, n_main: int):
    """ONE set of sampling / main streams (and one gather stream) for every detector this process builds: each stream
    ever created keeps a place among the GPU_MAX_HW_QUEUES hardware queues, and the three detectors of a default run
    would otherwise create 24 (the last one then ran its FPS chains two to a queue: 3.1 k instead of 5.4 k scenes/s).
    The whole set (eight sampling streams, six under a process group: `DISTRIBUTED`) is made at the first call, in the order that keeps the
    main streams alone on their dispatch pipes (sad_amd._runtime.placed_streams)."""
    from sad_amd import _runtime
    from sad_amd.dist import AsyncBoxGather
    st = _STREAMS.get(str(dev))
    if st is None or len(st["side"]) < n_side or len(st["main"]) < n_main:
        if st is not None:
            raise SystemExit(f"shared_streams: {n_side} sampling / {n_main} main streams asked for after the set was made "
                             f"with {len(st['side'])} / {len(st['main'])}")
        if n_main >= 3:       # (three main streams: every other stream shares ONE pipe, four queue numbers apiece: only what this run needs)
            side, main, extra = _runtime.placed_streams(dev, n_side, n_main, 1)
        else:
            side, main, extra = _runtime.placed_streams(dev, max(n_side, default_fps_streams("f32")), max(n_main, 2), 1 if DISTRIBUTED else 2)
        st = _STREAMS[str(dev)] = {"side": side, "main": main, "gather": AsyncBoxGather(dev, stream=extra[0]),
                                   "ingest": extra[1] if len(extra) > 1 else None}
    return (st["side"][:n_side], st["main"][:n_main]), st["gather"]


def measure(w: Workload, steps: int, warmup: int, rank: int, world: int, dev, args, detail: bool):
    """Build the detector of workload ``w``, run ``warmup`` untimed and exactly ``steps`` timed steps between device
    synchronisations (and barriers for world > 1), then the per-launch passes.  Returns (record, exit code, context) on
    rank 0 and (None, 0, None) on the others.  ``detail``: the headline record (every field); otherwise a leg record
    (value, ms/step, MLP roofline, FPS / ball-query ms)."""
    import gc
    from collections import deque
    import numpy as np
    import torch
    import torch.distributed as dist
    from sad_amd import _lib, config, ops, synth
    from sad_amd.detector import SADDetector

    cfg = w.cfg()
    B = w.B
    weights = synth.make_weights(cfg, 0)
    streams, gather = shared_streams(dev, w.fps_streams if w.overlap else 0, w.main_streams)   # (gather: the step's one collective, off the compute streams)
    det = SADDetector(cfg, weights, dev, overlap_fps=w.overlap, n_fps_streams=w.fps_streams,
                      n_main_streams=w.main_streams, dtype=w.dtype, streams=streams)
    PEAK = w.peak()
    make = w.maker()
    batches_np = [make(batch_first_scene(w.first_batch + k, rank, world, B), B, cfg.n_points) for k in range(w.n_batches)]
    batches = [torch.from_numpy(p).to(dev) for p in batches_np]
    torch.cuda.synchronize()

    if args.geometry_file and detail:
        det.set_geometry(json.load(open(args.geometry_file)))
        tuned = det.geometry()
        geometry_source = f"file:{os.path.basename(args.geometry_file)}"
    elif args.no_autotune:
        tuned, geometry_source = {}, "heuristic"
    else:
        tuned, geometry_source = det.autotune(batches[0]), "autotuned on batch 0 of the rotation"
    if args.save_geometry and rank == 0 and detail:
        json.dump(tuned, open(args.save_geometry, "w"), indent=1, sort_keys=True)
    geom_hash = hashlib.sha256(json.dumps(tuned, sort_keys=True).encode()).hexdigest()[:12]

    # Bounded run-ahead: the host enqueues a step in ~0.5 ms, the GPU needs ~2.4 ms, so an unbounded loop queues
    # hundreds of steps whose workspaces (~0.3 GB each) cannot be recycled until they have run — the caching
    # allocator then grows until it has to free and re-allocate, which stalls the device for 0.4-0.6 s (measured).
    # A serving loop bounds its queue the same way: at most `queue_depth` steps in flight.
    inflight = deque()
    submitted = [0]

    def step():
        if len(inflight) >= w.queue_depth:
            inflight.popleft().synchronize()
        k = submitted[0] % len(batches)
        submitted[0] += 1
        out, ev = det.submit(batches[k], post=gather)
        inflight.append(ev)
        return out, k

    # Setup, like the autotune pass above: every slot of the detector's step-plan ring records its launches (and allocates the
    # ~0.3 GB of buffers it keeps) once — a recording step is an eager step plus fresh allocations, and with fewer warm-up steps
    # than ring slots (the driver's --warmup 5 against 12 slots) up to seven of them would fall into the timed region
    primed = 0
    if getattr(det, "use_plans", False):
        for _ in range(det._plan_ring):
            step()
            primed += 1
        torch.cuda.synchronize()
        inflight.clear()
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    if dist.is_initialized():
        dist.barrier()
        torch.cuda.synchronize()
    # The timed region carries no per-launch events (creating ~40 timing events per sampled step stalled the
    # queue for 15-30 ms once per run: measured); per-launch intervals under overlap are sampled in a few extra
    # steps AFTER the timed region, the roofline figures come from the serial pass further down.
    step_marks = [torch.cuda.Event(enable_timing=True) for _ in range(steps)]   # one per step, created up front
    # (no cyclic-GC passes of the interpreter inside the timed region: the 1 ms steps of the bf16 mode empty an eight-deep queue
    # during one multi-millisecond pause of the enqueuing thread; one evidence run showed 14 of 200 steps stalled ~5 ms)
    gc.collect()
    gc.disable()
    out, last = None, 0
    try:                                          # (a failure inside must not leave the collector off for the later legs)
        t0 = time.perf_counter()
        for i in range(steps):
            out, last = step()
            step_marks[i].record(det.last_stream)
        torch.cuda.synchronize()
        if dist.is_initialized():
            dist.barrier()
            torch.cuda.synchronize()
        elapsed_local = time.perf_counter() - t0
    finally:
        gc.enable()
    # (SAD_BENCH_WHATIF: measurement builds that skip work on purpose produce garbage boxes; never set for a reported line)
    assert out.shape == (world * B, cfg.n_cand, 9) and (bool(torch.isfinite(out).all()) or bool(os.environ.get("SAD_BENCH_WHATIF")))
    got_boxes = out[:B].cpu().numpy()          # rank 0's own scenes come first in the gathered tensor; batch `last`
    points, points_np = batches[last], batches_np[last]
    if detail and rank == 0 and args.dump_outputs:
        dump_boxes(args.dump_outputs, out.cpu().numpy())

    quality = None
    if args.full and w.dtype == "bf16" and rank == 0 and not getattr(args, "no_bf16_quality", False):
        # the bf16 mode against the f32 detector on the batch the timed region ended with (same weights; serial, traced passes)
        det32 = SADDetector(cfg, weights, dev, overlap_fps=False, n_main_streams=w.main_streams, dtype="f32", streams=streams)
        det.overlap_fps, ov = False, det.overlap_fps
        try:
            tr_b, tr_f = {}, {}
            b_bf = det(points, trace=tr_b)
            b_32 = det32(points, trace=tr_f)
            torch.cuda.synchronize()
            quality = bf16_quality(b_bf.cpu().numpy(), b_32.cpu().numpy(),
                                   [t.cpu().numpy() for t in tr_b["cluster"]["ball_idx"]],
                                   [t.cpu().numpy() for t in tr_f["cluster"]["ball_idx"]])
            quality["timed_region_boxes_equal_traced_pass"] = bool(np.array_equal(b_bf.cpu().numpy(), got_boxes))
        finally:
            det.overlap_fps = ov
        del det32, tr_b, tr_f, b_bf, b_32
        torch.cuda.empty_cache()

    log = [] if args.full and not args.no_launch_timing else None
    timed_steps = 0
    if log is not None and detail:
        for i in range(16):
            sample = i % 4 == 2
            ops.LAUNCH_LOG = log if sample else None
            timed_steps += int(sample)
            step()
            ops.LAUNCH_LOG = None
        torch.cuda.synchronize()
    inflight.clear()
    elapsed = elapsed_local
    rank_info = None
    if dist.is_initialized():
        t = torch.tensor([elapsed], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
        # per-rank view (who is the straggler, which device, which geometry): one small all_gather
        mine = torch.tensor([B * steps / elapsed_local, float(torch.cuda.current_device()),
                             float(int(geom_hash[:6], 16))], dtype=torch.float64, device=dev)
        allr = [torch.zeros_like(mine) for _ in range(world)]
        dist.all_gather(allr, mine)
        per_rank = [r.cpu().tolist() for r in allr]
        rank_info = {"backend": dist.get_backend(), "ranks_seen": dist.get_world_size(),
                     "scenes_per_s_per_rank": {"min": round(min(p[0] for p in per_rank), 1),
                                               "max": round(max(p[0] for p in per_rank), 1),
                                               "all": [round(p[0], 1) for p in per_rank]},
                     "device_index_per_rank": [int(p[1]) for p in per_rank],
                     "geometry_hash_per_rank": [f"{int(p[2]):06x}" for p in per_rank],
                     "gpu_max_hw_queues": os.environ.get("GPU_MAX_HW_QUEUES"),
                     "one_rank_rehearsal": bool(os.environ.get("SAD_DIST_FORCE_COLLECTIVE")) and world == 1,
                     "note": "each rank autotunes its own geometry (same kernels, same bits; picks may differ "
                             "by a few per cent in speed); elapsed is the MAX over ranks between two barriers"}
    if rank != 0:
        return None, 0, None

    rc = 0
    work = config.work_per_scene(cfg)
    # completion-to-completion intervals of consecutive steps (steps alternate between the main
    # streams; an interval between steps on different streams can be ~0 or ~2 steps: use pairs)
    nm = max(1, w.main_streams)
    gaps = [step_marks[i].elapsed_time(step_marks[i + nm]) / nm for i in range(0, len(step_marks) - nm)]
    slow_at = [i for i, g in enumerate(gaps) if g > 2 * sorted(gaps)[len(gaps) // 2]]
    gaps.sort()
    res = {
        "metric": ("scenes/sec (16384-pt KITTI-shaped) through SA+cluster path" if w.config == "kitti" else
                   "scenes/sec (65536-pt nuScenes-shaped, configs[4]) through SA+cluster path"),
        "value": round(world * B * steps / elapsed, 2),
        "unit": "scenes/s",
        "n_gpus": world, "steps": steps, "warmup": warmup,
        "ms_per_step": round(1e3 * elapsed / steps, 3),
        "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
        "dtype": w.dtype, "data": "synthetic",
        "config": {"workload": w.describe(),
                   "scenes_per_gpu": B, "global_batch": world * B, "n_points": cfg.n_points, "scene": w.scene,
                   "resident_batches": len(batches), "parity_batch": w.first_batch + last,
                   "parallelism": f"batch-sharded x{world}, one all_gather of boxes",
                   "fps_overlap": w.overlap, "fps_streams": w.fps_streams, "main_streams": w.main_streams, "opts": args.opt,
                   "queue_depth": w.queue_depth,
                   "step_plans": {"enabled": bool(getattr(det, "use_plans", False)), "ring_slots": getattr(det, "_plan_ring", None),
                                  "priming_steps_before_warmup": primed, "replays": getattr(det, "plan_replays", None),
                                  "refused": getattr(det, "plan_refused", None)},
                   # (bf16 mode: pooled rows as bf16 + continuation rows, which stages took it — DESIGN.md 3.4; f32: n/a)
                   "split_pooling": split_pooling_state(det, B),
                   "gpu_max_hw_queues": os.environ.get("GPU_MAX_HW_QUEUES"), "gpu_max_hw_queues_at_process_start": HW_QUEUES_AT_START,
                   "mlp_geometry": tuned if tuned else "heuristic", "mlp_geometry_source": geometry_source,
                   "mlp_geometry_hash": geom_hash},
    }
    if gaps:
        res["step_ms"] = dict(step_tail(gaps), over_2x_p50_at_steps=slow_at[:8],
                              note=f"completion-to-completion over {nm} consecutive steps / {nm} (HIP events on the main streams)")
    if quality is not None:
        res["bf16_quality"] = quality
    if rank_info is not None:
        res["ranks"] = rank_info
    elif world == 1 and detail:
        res["ranks"] = {"backend": None, "ranks_seen": 1, "note": "N = 1: no process group, no collective; "
                        "the RCCL path (N > 1) is unmeasured until the driver has a multi-GPU node"}

    if log is not None:
        tsteps = max(1, timed_steps)
        per_kind, per_name = {}, {}
        for kind, name, e0, e1 in log:
            ms = e0.elapsed_time(e1)
            per_kind[kind] = per_kind.get(kind, 0.0) + ms
            per_name[(kind, name)] = per_name.get((kind, name), 0.0) + ms
        exec_flops, row_frac, per_flops = executed_flops(det, points, cfg)
        # ---- serial pass: ONE stream, sampling not overlapped, no sibling batch: every event
        # interval is the duration of that launch's kernels (plus the cost of the event pair itself, measured and
        # subtracted) (a pass is synchronised before the next starts and the per-launch MEDIAN over the passes is
        # used: an interval also contains any time the stream waited for the host, e.g. one allocator miss)
        NSER = 7
        det.overlap_fps, ov = False, det.overlap_fps
        passes = []
        try:
            det(points)
            torch.cuda.synchronize()
            for _ in range(NSER):
                ops.LAUNCH_LOG = []
                det(points)
                torch.cuda.synchronize()
                passes.append(ops.LAUNCH_LOG)
                ops.LAUNCH_LOG = None
        finally:
            det.overlap_fps = ov
            ops.LAUNCH_LOG = None
        empty_pair_ms = event_overhead_ms(torch.cuda.current_stream())
        # What a pair of events adds to the interval around a dispatch, calibrated on the step's own dispatches: one more
        # serial step with re-launchable closures; for each of the three shortest dispatches T1 (one launch between a pair)
        # and T6 (six in a row): the launch itself costs (T6 - T1) / 5, the bracket T1 - that.  (An EMPTY pair measures ~4 us,
        # the bracket around a real launch ~9 us: the first kernel also waits for the start event's timestamp write.)
        det.overlap_fps, ov = False, det.overlap_fps
        try:
            ops.RERUN_LOG = []
            det(points)
            torch.cuda.synchronize()
            reruns, ops.RERUN_LOG = ops.RERUN_LOG, None
        finally:
            det.overlap_fps = ov
            ops.RERUN_LOG = None
        cur = torch.cuda.current_stream()

        def timed_runs(fn, k, reps=7):
            vals = []
            for _ in range(reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(cur)
                for _ in range(k):
                    fn()
                e1.record(cur)
                torch.cuda.synchronize()
                vals.append(e0.elapsed_time(e1))
            vals.sort()
            return vals[len(vals) // 2]

        cal = []
        for name, fn in reruns:
            fn()
            torch.cuda.synchronize()
            cal.append((timed_runs(fn, 1, 5), name, fn))
        cal.sort(key=lambda t: t[0])
        brackets = []
        for t1, name, fn in cal[:3]:
            t1 = timed_runs(fn, 1)
            t6 = timed_runs(fn, 6)
            brackets.append(max(0.0, t1 - (t6 - t1) / 5.0))
        brackets.sort()
        ev_ms = brackets[len(brackets) // 2] if brackets else empty_pair_ms
        ser_log = passes[0]
        n_mlp = sum(1 for k, _, _, _ in ser_log if k == "mlp")
        ser_kind, ser_name, raw_kind = {}, {}, {}
        for li, (k, n, _, _) in enumerate(ser_log):
            raw = sorted(p[li][2].elapsed_time(p[li][3]) for p in passes)[NSER // 2]
            ms = max(0.0, raw - ev_ms)
            raw_kind[k] = raw_kind.get(k, 0.0) + raw
            ser_kind[k] = ser_kind.get(k, 0.0) + ms
            ser_name[(k, n)] = ser_name.get((k, n), 0.0) + ms
        mlp_ms = ser_kind.get("mlp", 0.0)
        ach = exec_flops / (mlp_ms * 1e-3) / 1e12 if mlp_ms > 0 else 0.0
        traffic, traffic_file = None, None
        if w.scene == "kitti":
            for fn in TRAFFIC_FILES.get((w.config, w.dtype), ()):
                tpath = os.path.join(ROOT, "profiles", fn)
                if os.path.exists(tpath):
                    # HBM bytes of the same launches from the committed rocprofv3 --pmc passes (bench.py cannot
                    # collect PMC counters itself): corrected FETCH_SIZE + WRITE_SIZE, per step like `achieved`
                    tj = json.load(open(tpath))
                    traffic, traffic_file = tj["fetch_bytes_per_step"] + tj["write_bytes_per_step"], fn
                    break
        ov_ms = per_kind.get("mlp", 0.0) / tsteps
        kname = ("mlp_reg / mlp_coop / mlp_layer / mlp_rows / mlp_chain kernels" if w.dtype == "f32"
                 else "mlp_bf16_reg / bf16_rows / mlp_bf16 kernels")
        res["roofline"] = {
            "kernel": f"{kname} ({n_mlp} dispatches per step, summed)",
            "bound": "mfma", "achieved": round(ach, 2), "peak": PEAK,
            "unit": "TFLOP/s", "frac": round(ach / PEAK, 4), "traffic": traffic,
            "traffic_note": (f"HBM bytes per step of the step's MLP dispatches from profiles/{traffic_file} (rocprofv3 --pmc, "
                             "FETCH_SIZE and WRITE_SIZE in separate passes, gfx950 corrections of MI355X_MICROARCH.md); "
                             "the kernels are MFMA-bound, not HBM-bound") if traffic else None,
            "flop_per_step": exec_flops, "ms_per_step": round(mlp_ms, 4),
            "ms_per_step_uncorrected": round(raw_kind.get("mlp", 0.0), 4), "event_pair_ms": round(ev_ms, 5),
            "empty_event_pair_ms": round(empty_pair_ms, 5),
            "note": "achieved = flops the kernels EXECUTE per step / the summed duration of the step's MLP dispatches, "
                    "HIP events on the launching stream in a serial pass (one stream, nothing overlapped) on the batch the parity "
                    f"check uses, per-dispatch median of {NSER} passes right after the timed region, minus what the event pair around a "
                    "dispatch adds (`event_pair_ms`: calibrated on the three shortest dispatches of the step as T1 - (T6 - T1) / 5, one launch "
                    "against six in a row between one pair; `ms_per_step_uncorrected` keeps the raw sum).  Grouped rows "
                    "that only repeat a group's first neighbour (ball-query padding) are skipped exactly (a duplicate row cannot change "
                    "the max-pool), so executed flops < SPEC-dense flops; tools/roofline_from_profiles.py recomputes the same fraction "
                    "from the committed rocprofv3 kernel trace",
            "executed_row_fraction": round(row_frac, 4), "spec_dense_flop_per_step": work["mlp_flops"] * B}
        if detail:
            res["roofline"]["under_overlap"] = {
                "ms_per_step_summed": round(ov_ms, 3), "sampled_steps": tsteps,
                "note": "the same launches in extra steps run exactly like the timed region (two main streams run "
                        "consecutive batches side by side): intervals stretch (kernels share the chip) and their "
                        "sum may exceed ms_per_step; not a kernel-quality figure"}
        # ---- the same dispatches back to back: each dispatch of one serial step is enqueued again, 1 + 5 times in a row,
        # and timed with one pair of events.  Two uses.  (a) f32: in the serial pass every step begins with ~2 ms of FPS on 32
        # of 256 CUs, the chip clocks down meanwhile and the MLP launches behind it run several % slower than the same
        # launches at the clock the timed region holds (tools/insitu_probe.py): `steady_clock` is that second figure, `frac`
        # stays the in-step one (it is what the committed serial rocprofv3 trace reproduces: 0.566 vs 0.562).  (b) bf16: the
        # dispatches are 14 - 130 us long and the bracket around each in-step dispatch also holds the launch gap and the
        # end-of-kernel write-back of its predecessor (~6 us per dispatch, 10 % of the summed intervals; kernel DURATIONS in
        # the rocprofv3 trace of the same launches do not): there `frac` is the back-to-back figure (0.145 vs 0.142 from
        # the trace) and the in-step sum is kept as `in_step`.  (bf16 on nuScenes-shaped batches: dispatches of 60 - 850 us, in-step
        # like f32: 0.190 by events vs 0.191 from the trace; back to back they run 7 % faster.)
        if True:
            steady = {}
            for name, fn in reruns:
                fn()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(cur)
                for _ in range(5):
                    fn()
                e1.record(cur)
                torch.cuda.synchronize()
                steady[name] = steady.get(name, 0.0) + e0.elapsed_time(e1) / 5
            reruns = None
            st_ms = sum(steady.values())
            st = {"ms_per_step": round(st_ms, 4), "achieved": round(exec_flops / (st_ms * 1e-3) / 1e12, 2),
                  "frac": round(exec_flops / (st_ms * 1e-3) / 1e12 / PEAK, 4),
                  "per_launch_ms": {n: round(v, 4) for n, v in sorted(steady.items())},
                  "note": "the same dispatches (same arguments, from one more serial step), each enqueued 5 times in a row between "
                          "one pair of events"}
            r = res["roofline"]
            # short dispatches (mean below 100 us: the bf16 mode on KITTI-shaped batches): back to back; long ones (f32; bf16 on the
            # nuScenes-shaped batches, 272 us on average): in the step — each choice is the one the committed traces reproduce
            if mlp_ms / max(1, n_mlp) < 0.1:
                r["in_step"] = {"ms_per_step": r["ms_per_step"], "achieved": r["achieved"], "frac": r["frac"],
                                "note": "summed event intervals of the serial pass (each also holds a launch gap and the predecessor's "
                                        "write-back: ~6 us per dispatch)"}
                r["ms_per_step"], r["achieved"], r["frac"] = st["ms_per_step"], st["achieved"], st["frac"]
                r["frac_source"] = "back_to_back"
                r["back_to_back"] = st
                for n, v in ser_name.items():          # per-dispatch table: the same source as `frac`
                    if n[0] == "mlp" and n[1] in steady:
                        ser_name[n] = steady[n[1]]
            else:
                r["frac_source"] = "in_step_events"
                st["note"] += ": durations at the clock a continuously busy chip holds.  In the serial pass every step starts with ~2 ms of FPS " \
                              "on 32 CUs and the MLP launches behind it run at a lower clock; the timed region (two main streams, FPS " \
                              "overlapped) is continuously busy.  `frac` stays the in-step figure"
                r["steady_clock"] = st
        kern = []
        fps_ms = ser_kind.get("fps", 0.0)
        if fps_ms > 0:
            nested = getattr(det, "nested_fps_shortcut", True)
            serial = cfg.stages[0].npoint if nested else work["fps_steps"]
            kern.append({"kernel": "fps_sort_kernel + fps_cell_kernel / fps_cellg_kernel ("
                                   + ("stage 1 only: stages 2-3 reuse its prefix, proven identical)" if nested else "3 stages)"),
                         "ms_per_step": round(fps_ms, 3),
                         "cu_ms_per_step": round(fps_ms * B, 1),
                         "updates_per_s": round(work["fps_updates"] * B / (fps_ms * 1e-3) / 1e9, 2),
                         "unit": "G distance-updates/s (plain-scan equivalent; most are skipped exactly)",
                         "serial_steps": serial,
                         "us_per_serial_step": round(1e3 * fps_ms / serial, 3),
                         "bound": "serial latency (neither HBM nor MFMA); one workgroup (one CU) per scene: cu_ms_per_step = CUs held x ms; "
                                  "in the timed region it runs on sampling streams under the MLP kernels"})
        bq_ms = ser_kind.get("ball_query", 0.0)
        if bq_ms > 0:
            gbps = work["ball_query_bytes"] * B / (bq_ms * 1e-3) / 1e9
            kern.append({"kernel": "ball query: grid_build/grid_query (SA1, SA2) + ball_query_kernel scan (SA3, adaptive cluster query)",
                         "ms_per_step": round(bq_ms, 3),
                         "per_launch_ms": {n: round(v, 4) for (k, n), v in sorted(ser_name.items()) if k == "ball_query"},
                         "bound": "hbm", "achieved": round(gbps, 1), "peak": PEAK_HBM_GBPS, "unit": "GB/s",
                         "frac": round(gbps / PEAK_HBM_GBPS, 5), "algorithmic_bytes_per_step": work["ball_query_bytes"] * B,
                         "pair_tests_per_s": round(work["pair_tests"] * B / (bq_ms * 1e-3) / 1e12, 3),
                         "note": "serial pass, HIP events per launch.  BASELINE's >= 70 % of HBM peak is not reachable: the "
                                 "PMC traffic equals the algorithmic bytes (nothing is re-read), the kernels are bound by the "
                                 "per-centroid instruction chain that restores index order (~300 vector instructions for ~20 "
                                 "candidates), not by bytes"})
        if detail:
            # the unfused group_points operator (not on the fused path; part of the drop-in surface):
            # an HBM-bound gather, timed here on the SA2 branch shape with its own HIP events
            gC, gN, gM, gS = 64, 4096, 1024, 32
            gfeat = torch.randn(B, gC, gN, device=dev)
            gidx = torch.randint(0, gN, (B, gM, gS), device=dev, dtype=torch.int32)
            ops.group_points(gfeat, gidx)
            torch.cuda.synchronize()
            ge0, ge1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ge0.record()
            for _ in range(10):
                ops.group_points(gfeat, gidx)
            ge1.record()
            torch.cuda.synchronize()
            g_ms = ge0.elapsed_time(ge1) / 10
            g_bytes = B * (gM * gS * 4 + gC * gM * gS * 4 + gC * gN * 4)     # idx + grouped out + source once
            kern.append({"kernel": "group_lds_kernel (unfused group_points, SA2 branch shape, outside the timed region)",
                         "ms_per_launch": round(g_ms, 4), "bound": "hbm",
                         "achieved": round(g_bytes / (g_ms * 1e-3) / 1e9, 1), "peak": PEAK_HBM_GBPS, "unit": "GB/s",
                         "frac": round(g_bytes / (g_ms * 1e-3) / 1e9 / PEAK_HBM_GBPS, 4),
                         "algorithmic_bytes": g_bytes})
            del gfeat, gidx
        res["kernels"] = kern
        per_bytes = getattr(executed_flops, "last_bytes", {})
        res["mlp_launches"] = {n: {"ms": round(v, 4), "executed_gflop": round(flops_of(n, per_flops) / 1e9, 2),
                                   "tflops": round(flops_of(n, per_flops) / (v * 1e-3) / 1e12, 1) if v > 0 else None,
                                   "frac": round(flops_of(n, per_flops) / (v * 1e-3) / 1e12 / PEAK, 3) if v > 0 else None,
                                   **dispatch_bound(flops_of(n, per_flops), bytes_of(n, per_bytes), v, PEAK),
                                   **({"ms_under_overlap": round(per_name.get(("mlp", n), 0.0) / tsteps, 4)} if detail else {})}
                               for (k, n), v in sorted(ser_name.items()) if k == "mlp"}
        # every dispatch against ITS bound: sum of the bound times / sum of the measured times
        bt = sum(max(d["mfma_ms"], d["hbm_ms"]) for d in res["mlp_launches"].values())
        mt = sum(d["ms"] for d in res["mlp_launches"].values())
        res["roofline"]["per_dispatch_bound"] = {
            "frac": round(bt / mt, 4) if mt > 0 else None, "bound_ms": round(bt, 4),
            "hbm_bound_dispatches": sorted(n for n, d in res["mlp_launches"].items() if d["bound"] == "hbm"),
            "algorithmic_mb_per_step": round(sum(d["algorithmic_mb"] for d in res["mlp_launches"].values()), 1),
            "note": "each dispatch graded against max(flops / MFMA peak, algorithmic bytes / 8 TB/s); `frac` above keeps the MFMA-only "
                    "definition of the earlier rounds"}
        if detail:
            res["mlp_launch_order"] = [n for k, n, _, _ in ser_log if k == "mlp"]

    # ---- dense leg: the same kernels with the padding skip off (every grouped row computed) ----
    if args.full and detail and not args.no_dense_leg and w.dtype == "f32" and world == 1:
        _lib.set_option("mlp_nodedup", 1)
        try:
            for _ in range(2):
                det.submit(points)
            torch.cuda.synchronize()
            nd = 8
            td = time.perf_counter()
            for _ in range(nd):
                dout, _ = det.submit(points)
            torch.cuda.synchronize()
            dd = time.perf_counter() - td
        finally:
            _lib.set_option("mlp_nodedup", 0)
        res["dense_leg"] = {"value": round(B * nd / dd, 1), "unit": "scenes/s", "steps": nd,
                            "tflops_spec_dense": round(work["mlp_flops"] * B * nd / dd / 1e12, 1),
                            "same_boxes": bool(np.array_equal(dout.cpu().numpy(), got_boxes)),
                            "note": "sad_set_option(mlp_nodedup=1): every padded grouped row is computed (SPEC-dense flops, "
                                    "geometry tuned for the sparse rows) - the floor for scenes whose neighbourhoods are all "
                                    "full; the headline's 13x fewer rows are a property of the KITTI-shaped scene density "
                                    "(~3 points per square metre), not of the kernels"}
    ctx = {"cfg": cfg, "weights": weights, "points_np": points_np, "got_boxes": got_boxes}
    del det, batches
    torch.cuda.empty_cache()
    return res, rc, ctx


def ragged_scenes(first_scene: int, B: int, n_points: int, lo: float = 0.55, hi: float = 1.75):
    """B KITTI-shaped scenes with DIFFERENT point counts (uniform in [lo, hi] x n_points, seeded by the scene id): what a
    loader hands over after reading and range-cropping the files of a batch."""
    import numpy as np
    from sad_amd import synth
    out = []
    for i in range(B):
        sid = first_scene + i
        n = int(np.random.default_rng(777 + sid).integers(int(lo * n_points), int(hi * n_points) + 1))
        out.append(synth.make_scene(sid, n))
    return out


def pipeline_leg(args, dev, geometry, headline_value: float, rank: int, world: int) -> dict:
    """SURVEY 8(f) rows 1 + 2 on the step: ragged point files in pinned host memory -> async H2D -> ops.subsample_pad ->
    SADDetector.submit -> ops.nms_bev -> D2H (boxes, rank order, kept count), `sad_amd.pipeline.IngestPipeline`.  Scenes/s beside
    the resident-input headline, per-stage ms from a serial pass, and a parity check of the last step against the oracle chain."""
    import gc
    import numpy as np
    import torch
    import oracle
    from sad_amd import config, synth
    from sad_amd.detector import SADDetector
    from sad_amd.pipeline import IngestPipeline

    cfg, B = config.KITTI, args.batch
    weights = synth.make_weights(cfg, 0)
    w = Workload("kitti", "kitti", "f32", B, None, args.main_streams, None, args.batches)
    streams, _ = shared_streams(dev, w.fps_streams, w.main_streams)
    ing = _STREAMS[str(dev)]["ingest"]              # (made with the other streams: not on a main stream's dispatch pipe)
    det = SADDetector(cfg, weights, dev, n_fps_streams=w.fps_streams, n_main_streams=w.main_streams, dtype="f32", streams=streams)
    if isinstance(geometry, dict):
        det.set_geometry(geometry)
    nb = max(1, args.batches)
    scenes = [ragged_scenes(batch_first_scene(100 + k, rank, world, B), B, cfg.n_points) for k in range(nb)]
    pipe = IngestPipeline(det, B, cols=4, max_points_per_scene=int(1.75 * cfg.n_points) + 1, in_slots=nb, out_slots=w.queue_depth,
                          ingest_stream=ing)
    staged_bytes = [pipe.stage(k, scenes[k]) for k in range(nb)]
    steps, warm = args.pipeline_steps, 14
    kept_total, last = 0, None
    for i in range(warm):
        last = pipe.submit(i % nb)
    torch.cuda.synchronize()
    gc.collect()
    gc.disable()
    marks = [torch.cuda.Event(enable_timing=True) for _ in range(steps)]
    try:
        t0 = time.perf_counter()
        for i in range(steps):
            last = pipe.submit(i % nb)
            marks[i].record(det.last_stream)
            if i >= w.queue_depth - 1:                   # the host consumes a finished step: kept boxes of its scenes
                _, _, cnt = pipe.result((last + 1) % w.queue_depth)
                kept_total += int(cnt.sum())
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
    finally:
        gc.enable()
    last_in = (steps - 1) % nb
    got = tuple(np.array(a) for a in pipe.result(last))
    nm = max(1, w.main_streams)
    gaps = [marks[i].elapsed_time(marks[i + nm]) / nm for i in range(0, steps - nm)]
    stage_ms = {}
    for _ in range(5):
        for k, v in pipe.timed_serial_step(last_in).items():
            stage_ms.setdefault(k, []).append(v)
    stage_ms = {k: round(sorted(v)[len(v) // 2], 4) for k, v in stage_ms.items()}
    # parity: the oracle chain on the same staged files (first n scenes of the last step's batch)
    oracle.build()
    n_par = max(1, min(B, args.cpu_scenes)) if not args.no_cpu else min(B, 4)
    pts, offs = pipe.staged(last_in)
    padded = oracle.subsample_pad(pts[:offs[n_par]], offs[:n_par + 1], cfg.n_points, 0)
    want = oracle.detector_forward(padded, cfg, weights, skip_padding=True)
    par = pipeline_parity(got, want, lambda b: oracle.nms_bev(b, pipe.iou_thr, pipe.score_thr))
    value = B * steps / dt
    rec = {"value": round(value, 1), "unit": "scenes/s", "steps": steps, "warmup": warm, "ms_per_step": round(1e3 * dt / steps, 3),
           "vs_resident_headline": round(value / headline_value, 4) if headline_value else None,
           "step_ms": step_tail(gaps),
           "stages_ms_serial": stage_ms,
           "bytes_per_step": {"h2d": int(sum(staged_bytes) / nb), "d2h": int(B * cfg.n_cand * (9 * 4 + 4) + B * 4)},
           "h2d_gbps_serial": round(sum(staged_bytes) / nb / (stage_ms["h2d"] * 1e-3) / 1e9, 1) if stage_ms.get("h2d") else None,
           "points_per_scene": {"min": int(min(s_.shape[0] for b_ in scenes for s_ in b_)), "max": int(max(s_.shape[0] for b_ in scenes for s_ in b_))},
           "nms": {"iou_thr": pipe.iou_thr, "score_thr": pipe.score_thr, "kept_boxes_consumed": kept_total},
           "parity_check": par,
           "workload": (f"{nb} batches of {B} RAGGED KITTI-shaped scenes ({int(0.55 * cfg.n_points)} - {int(1.75 * cfg.n_points)} points each, "
                        "raw N x 4 float32 file bytes staged in pinned host memory) in rotation -> H2D copy + ops.subsample_pad on an ingest "
                        "stream -> SADDetector.submit (f32, the headline's geometry and streams) -> ops.nms_bev -> D2H of boxes, rank order and "
                        f"kept count into pinned slots; {w.queue_depth} steps in flight, the host reads every finished step's counts"),
           "note": "inputs are NOT resident: this is the PCIe-inclusive rate of the same detector; `value` of the headline stays the "
                   "resident-input figure (contract)"}
    del pipe, det
    torch.cuda.empty_cache()
    return rec


def split_pooling_state(det, B: int):
    """Which stages of a bf16 detector pool split (None for f32 or a detector without the hooks): the SA stages, then the cluster layer."""
    if getattr(det, "dtype", "f32") != "bf16" or not hasattr(det, "_cluster_can_split"):
        return None
    import torch
    cfg = det.cfg
    n_in = [cfg.n_points] + [st.npoint for st in cfg.stages[:-1]]
    out = []
    for si, m in enumerate(det.stages):
        prev_agg = si > 0 and det.stages[si - 1].agg is not None
        out.append(bool(m.can_split(B, n_in[si], m.stage.npoint, feat_dtype=torch.bfloat16 if prev_agg else torch.float32)))
    out.append(bool(det._cluster_can_split(B)))
    return out


def leg_record(res: dict) -> dict:
    """The part of a measurement that a secondary leg reports inside the headline line."""
    out = {k: res[k] for k in ("metric", "value", "unit", "steps", "warmup", "ms_per_step", "dtype") if k in res}
    out["workload"] = res["config"]["workload"]
    # (which kernels ran and whether the steps were replayed: a tiled pick for one chain turns the plans off and costs 7 - 8 %)
    out["mlp_geometry"] = res["config"].get("mlp_geometry")
    out["step_plans"] = res["config"].get("step_plans")
    out["split_pooling"] = res["config"].get("split_pooling")
    out["fps_streams"] = res["config"]["fps_streams"]
    out["scenes_per_gpu"] = res["config"]["scenes_per_gpu"]
    if "step_ms" in res:
        out["step_ms_p50"] = res["step_ms"]["p50"]
        out["step_ms"] = {k: res["step_ms"][k] for k in ("p50", "p99", "max", "over_2x_p50", "over_2x_p50_at_steps") if k in res["step_ms"]}
    if "bf16_quality" in res:
        out["bf16_quality"] = res["bf16_quality"]
    if "roofline" in res:
        r = res["roofline"]
        out["roofline"] = {k: r[k] for k in ("bound", "achieved", "peak", "unit", "frac", "traffic", "flop_per_step",
                                             "ms_per_step", "ms_per_step_uncorrected", "event_pair_ms", "frac_source")
                           if k in r}
        if "in_step" in r:
            out["roofline"]["in_step_frac"] = r["in_step"]["frac"]
        out["mlp_ms_per_step"] = r["ms_per_step"]
    for k in res.get("kernels", []):
        if k["kernel"].startswith("fps"):
            out["fps_ms_per_step"] = k["ms_per_step"]
            out["fps_cu_ms_per_step"] = k["cu_ms_per_step"]
            out["fps_us_per_serial_step"] = k["us_per_serial_step"]
        elif k["kernel"].startswith("ball query"):
            out["ball_query_ms_per_step"] = k["ms_per_step"]
            out["ball_query_hbm_frac"] = k["frac"]
    if "mlp_launches" in res:
        out["mlp_launches"] = {n: {"ms": v["ms"], "frac": v["frac"], "bound": v.get("bound"), "frac_of_bound": v.get("frac_of_bound")}
                               for n, v in res["mlp_launches"].items()}
        if "per_dispatch_bound" in res.get("roofline", {}):
            out["roofline"]["per_dispatch_bound"] = {k: res["roofline"]["per_dispatch_bound"][k] for k in ("frac", "hbm_bound_dispatches", "algorithmic_mb_per_step")}
    out["parity_check"] = res.get("parity_check")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--batch", type=int, default=32, help="scenes per GPU per step")
    ap.add_argument("--batches", type=int, default=4, help="distinct resident batches the timed region rotates over")
    ap.add_argument("--first-batch", type=int, default=0,
                    help="rotation slot of the first resident batch (profiling: --batches 1 --first-batch K runs exactly the batch a "
                         "default run reports as config.parity_batch, whose executed flops its roofline uses)")
    ap.add_argument("--no-overlap", action="store_true", help="run FPS on the main stream")
    ap.add_argument("--fps-streams", type=int, default=None,
                    help="sampling streams used round-robin (default: 3 for f32, 6 for bf16 - the bf16 MLP "
                         "dispatches are short enough that the serial FPS chain of a batch bounds the step otherwise)")
    ap.add_argument("--main-streams", type=int, default=2, help="main streams used round-robin by consecutive steps")
    ap.add_argument("--queue-depth", type=int, default=None,
                    help="steps in flight before the host waits for the oldest (default: max(6, sampling streams + 2))")
    ap.add_argument("--no-cpu", action="store_true", help="--full: skip the cpu_baseline leg (parity_check then uses 4 scenes)")
    ap.add_argument("--cpu-scenes", type=int, default=32, help="--full: scenes of the cpu_baseline sample")
    ap.add_argument("--no-launch-timing", action="store_true", help="--full: skip the per-launch event passes (roofline / kernels)")
    ap.add_argument("--no-dense-leg", action="store_true", help="--full: skip the dense_leg")
    ap.add_argument("--no-legs", action="store_true", help="--full: skip the secondary bf16_leg / configs4_leg / pipeline_leg of the default run")
    ap.add_argument("--no-bf16-quality", action="store_true", help="--full, bf16 runs: skip the comparison with the f32 detector on the last batch")
    ap.add_argument("--pipeline-steps", type=int, default=150, help="--full: timed steps of the pipeline_leg (files -> H2D -> subsample_pad -> detector -> NMS -> D2H)")
    ap.add_argument("--leg-steps", type=int, nargs=2, default=(300, 80), metavar=("BF16", "CONFIGS4"),
                    help="--full: timed steps of the two secondary legs")
    ap.add_argument("--no-autotune", action="store_true", help="use the built-in geometry heuristic")
    ap.add_argument("--geometry-file", default=None,
                    help="JSON {launch name: geometry code} from --save-geometry: no autotune launches (rocprof runs)")
    ap.add_argument("--save-geometry", default=None, help="write the geometry in use to this JSON file")
    ap.add_argument("--config", choices=("kitti", "nuscenes"), default="kitti",
                    help="nuscenes = BASELINE configs[4] shape (65536-pt scenes, 4 extra channels); secondary, "
                         "use with --dtype bf16 --no-cpu; the headline metric is the kitti default")
    ap.add_argument("--scene", choices=("kitti", "dense"), default="kitti",
                    help="dense = the same 16384 points on 20 m x 20 m (most neighbourhoods full): the dense-occupancy "
                         "floor of the same kernels; secondary, the headline is the KITTI-shaped default")
    ap.add_argument("--dtype", choices=("f32", "bf16"), default="f32",
                    help="bf16 = SPEC.md 14 mode (configs[4]): MLPs on the bf16 matrix cores; "
                         "the headline metric is the f32 default")
    ap.add_argument("--opt", action="append", default=[], help="tuning knob key=value (sad_set_option)")
    ap.add_argument("--full", action="store_true",
                    help="after the headline also run the per-launch roofline / kernel passes, dense_leg, parity_check against the "
                         "CPU oracle, cpu_baseline, bf16_quality and the secondary legs (the --no-* options above trim this)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the boxes of the last timed step to DIR/boxes.npy (float32)")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # `python bench.py --gpus N` as the driver runs it: start the N ranks ourselves (as a child process, before
        # anything here has imported torch or touched the GPU), relay rank 0's line and exit with the child's code
        raise SystemExit(self_launch(launch_command(sys.argv[1:], args.gpus, free_port())))

    import torch
    import torch.distributed as dist
    import sad_amd  # noqa: F401
    from sad_amd import ops

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}: launch `python bench.py --gpus N` (it starts its own "
                         "ranks) or torch.distributed.run with --nproc-per-node N")
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU: the HIP path is the only path (no CPU fallback)")
    if os.environ.get("SAD_BENCH_ONE_DEVICE"):      # rehearsal of the N>1 path on a one-GPU box
        local_rank = 0
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    if world == 1 and os.environ.get("SAD_BENCH_FORCE_DIST"):
        # rehearsal of the N > 1 path on a one-GPU box with the REAL backend: a one-rank RCCL communicator, the step's
        # all_gather, the barriers and the max-over-ranks reduction all run (sad_amd.dist: SAD_DIST_FORCE_COLLECTIVE)
        os.environ["SAD_DIST_FORCE_COLLECTIVE"] = "1"
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", str(free_port()))
        os.environ.setdefault("RANK", "0")
        os.environ.setdefault("WORLD_SIZE", "1")
        dist.init_process_group("nccl", device_id=dev)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        backend = os.environ.get("SAD_BENCH_BACKEND", "nccl")       # "nccl" is RCCL on ROCm
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=dev)
        else:                                                        # rehearsal on a one-GPU box
            dist.init_process_group(backend)

    global DISTRIBUTED
    DISTRIBUTED = dist.is_initialized()

    from sad_amd import _lib
    for kv in args.opt:
        k, v = kv.split("=")
        _lib.set_option(k, int(v))
    if os.environ.get("SAD_NO_MERGE_BF16"):
        ops.MERGE_BF16 = False

    head = Workload(args.config, args.scene, args.dtype, args.batch, args.fps_streams, args.main_streams,
                    args.queue_depth, args.batches, overlap=not args.no_overlap, first_batch=args.first_batch)
    res, rc, ctx = measure(head, args.steps, args.warmup, rank, world, dev, args, detail=True)

    if rank == 0 and args.full:
        cfg, weights, points_np = ctx["cfg"], ctx["weights"], ctx["points_np"]
        want = None
        if not args.no_cpu and world == 1:
            n_cpu = max(1, min(args.batch, args.cpu_scenes))
            res["cpu_baseline"], want = cpu_baseline(cfg, weights, points_np[:n_cpu])
        else:
            import oracle
            oracle.build()
            want = oracle.detector_forward(points_np[:min(args.batch, 4)], cfg, weights, skip_padding=True)
        if args.dtype == "f32":
            res["parity_check"] = parity_check(ctx["got_boxes"], want)
            res["parity_check"]["batch"] = res["config"]["parity_batch"]
            if not res["parity_check"]["ok"]:
                rc = 1
        else:
            res["parity_check"] = {"ok": None, "note": "bf16 mode (SPEC 14) is verified stage by stage with teacher forcing in "
                                                       "tests/test_gpu_bf16.py; an end-to-end box comparison is not meaningful "
                                                       "(one rounding flip may move an index decision)"}
        del ctx

    # ---- secondary legs of the default run (one GPU, the headline workload): the bf16 mode on the same scenes, and
    # BASELINE configs[4] on its own shape; short, after the headline, each a full measurement of its own detector
    default_run = (args.full and world == 1 and args.config == "kitti" and args.scene == "kitti" and args.dtype == "f32"
                   and not args.no_legs and not args.no_overlap and not args.opt)
    if default_run:
        import copy
        largs = copy.copy(args)
        largs.geometry_file, largs.save_geometry = None, None
        bf_note = {"ok": None, "note": "bf16 mode (SPEC 14): verified stage by stage in tests/test_gpu_bf16.py; its distance from the f32 "
                                       "detector on the leg's last batch is `bf16_quality`"}
        t_leg = time.perf_counter()
        try:
            res["pipeline_leg"] = pipeline_leg(args, dev, res["config"]["mlp_geometry"], res["value"], rank, world)
            res["pipeline_leg"]["wall_s"] = round(time.perf_counter() - t_leg, 1)
            if not res["pipeline_leg"]["parity_check"]["ok"]:
                rc = rc or 1
        except Exception as e:
            import traceback
            res["pipeline_leg"] = {"error": f"{type(e).__name__}: {e}", "trace": traceback.format_exc()[-600:]}
            rc = rc or 1
        for key, wl, nsteps in (("bf16_leg", Workload("kitti", "kitti", "bf16", args.batch, None, 2, None, args.batches), args.leg_steps[0]),
                                ("configs4_leg", Workload("nuscenes", "kitti", "bf16", 32, None, 2, None, 2), args.leg_steps[1])):
            t_leg = time.perf_counter()
            try:
                lres, _, lctx = measure(wl, nsteps, max(wl.fps_streams + 2, 14), rank, world, dev, largs, detail=False)   # (warm-up covers the 12 slots of the step-plan ring)
                del lctx
                lres["parity_check"] = bf_note
                res[key] = leg_record(lres)
                res[key]["wall_s"] = round(time.perf_counter() - t_leg, 1)
            except Exception as e:          # a leg must never take the headline line down with it
                res[key] = {"error": f"{type(e).__name__}: {e}"}
                rc = rc or 1
    if rank == 0:
        print(json.dumps(res), flush=True)
    if dist.is_initialized():
        dist.barrier()
        dist.destroy_process_group()
    if rc:
        raise SystemExit(rc)


if __name__ == "__main__":
    main()
