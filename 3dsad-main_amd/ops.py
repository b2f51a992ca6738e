"""Python operator surface: ``fps / ball_query / knn_query / group_points / gather_points`` and the other families,
each a thin validated wrapper over one C-ABI call.  The fused grouped-MLP (``PackedMLP`` / ``PackedMLPBf16`` / ``grouped_multi`` /
``rowscan_multi`` / ``mlp_chain`` and the autotuner) lives in ``mlp.py`` and is re-exported at the end of this module; its
switches (``AUTOTUNE``, ``LAUNCH_LOG``, ``RERUN_LOG``, ``MERGE_BF16``, ``SPLIT_POOL``) are set HERE, as ``ops.NAME = ...``.

Names and argument order are the ones BASELINE.json ``north_star`` fixes ("keeps the reference's
Python operator surface (fps / ball_query / group_points / sa_module)"); the upstream reference
itself (``/root/reference/README.md:1-2``) defines none, so semantics are SPEC.md §2-§6.

Every function takes CUDA(=HIP) tensors, enqueues hand-written gfx950 kernels on the current torch
stream through the C-ABI (``include/sad_amd.h``) and returns without synchronising.  There is no CPU
path: a CPU tensor raises ``RuntimeError``.  torch is used for device memory and streams only.
"""
import ctypes
import os
from typing import Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import _lib
from ._lib import check, lib, vp


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _empty(*a, **k) -> torch.Tensor:
    """torch.empty; while a step plan is recorded (plan.py) the plan keeps the buffer, so its address stays valid for replays."""
    rec = _lib.recorder()
    return torch.empty(*a, **k) if rec is None else rec.empty(*a, **k)


def _unrecordable(what: str) -> None:
    """In front of any framework kernel on the step path (fill, strided copy): an error while a plan records, nothing otherwise."""
    if _lib.recorder() is not None:
        from .plan import PlanUnsupported
        raise PlanUnsupported(what)


def copy_rows(src: torch.Tensor, src_off_words: int, src_stride_words: int, n_rows: int, row_words: int,
              out: torch.Tensor, dst_stride_words: Optional[int] = None) -> torch.Tensor:
    """Strided row copy in 4-byte words through the library (``sad_copy_rows_u32``): row r of ``out`` = words
    [0, row_words) of row r of ``src`` starting at word ``src_off_words``, rows ``src_stride_words`` apart.  ``out`` must be
    contiguous.  The host side's replacement for framework copies on the step (recordable: plan.py)."""
    check(lib().sad_copy_rows_u32(src.data_ptr() + 4 * int(src_off_words), int(src_stride_words), out.data_ptr(),
                                  int(row_words if dst_stride_words is None else dst_stride_words), int(n_rows), int(row_words),
                                  _stream()), "sad_copy_rows_u32")
    return out


def copy_to_host(src: torch.Tensor, dst_pinned: torch.Tensor) -> None:
    """Device tensor -> PINNED host tensor of the same byte size, written by a kernel of the library over the bus (pinned
    memory is device-addressable; visible to the host once the launching stream has reached an event behind this call).
    For the few hundred KB a step hands back (boxes, NMS order and counts): a copy-engine transfer per tensor shared its
    queue with the step's H2D transfer and a few steps in a hundred stalled for milliseconds (tools/probe/pipeline_probe.py)."""
    if not src.is_cuda or not src.is_contiguous() or dst_pinned.is_cuda or not dst_pinned.is_pinned() or not dst_pinned.is_contiguous():
        raise TypeError("copy_to_host: expected a contiguous GPU source and a contiguous pinned host destination")
    nbytes = src.numel() * src.element_size()
    if nbytes != dst_pinned.numel() * dst_pinned.element_size() or nbytes % 4 != 0:
        raise ValueError("copy_to_host: sizes differ (or are not whole 4-byte words)")
    check(lib().sad_copy_rows_u32(src.data_ptr(), nbytes // 4, dst_pinned.data_ptr(), nbytes // 4, 1, nbytes // 4, _stream()),
          "sad_copy_rows_u32")


def split_points(points: torch.Tensor):
    """points [B,N,3+C] f32 contiguous -> (xyz [B,N,3], feat [B,N,C] or None), both packed (two library launches)."""
    B, N, D = points.shape
    xyz = _empty((B, N, 3), dtype=torch.float32, device=points.device)
    copy_rows(points, 0, D, B * N, 3, xyz)
    feat = None
    if D > 3:
        feat = _empty((B, N, D - 3), dtype=torch.float32, device=points.device)
        copy_rows(points, 3, D, B * N, D - 3, feat)
    return xyz, feat


def prefix_rows(x: torch.Tensor, m: int) -> torch.Tensor:
    """x [B,M,C] contiguous (C * element size a multiple of 4 bytes) -> packed copy of x[:, :m, :] (one library launch)."""
    B, M, C = x.shape
    rb = C * x.element_size()
    if rb % 4 != 0 or not x.is_contiguous() or not x.is_cuda:
        raise TypeError("prefix_rows: expected a contiguous GPU tensor whose rows are whole 4-byte words")
    out = _empty((B, m, C), dtype=x.dtype, device=x.device)
    return copy_rows(x, 0, M * rb // 4, B, m * rb // 4, out)


# Optional per-launch timing for bench.py: when LAUNCH_LOG is a list, every operator brackets its
# C-ABI call with HIP events recorded on the stream the kernel is launched on and appends
# (kind, name, start_event, end_event).  None (the default) adds nothing to the launch path.
LAUNCH_LOG: Optional[list] = None
# When a list, every MLP dispatch appends (name, fn): fn() enqueues the SAME dispatch again (same arguments; the
# tensors it reads are kept alive by the entry).  bench.py re-times the dispatches of a step back to back with it.
RERUN_LOG: Optional[list] = None

# ball_query_multi uses the grid-pruned kernel for scenes with at least this many points (scalar
# radii only); below it the brute-force scan is already cheap.  Set very large to force brute force.
GRID_MIN_POINTS: int = 2048

# When True, PackedMLP measures the workgroup geometries of mlp_chain_kernel on the first call for
# each shape and keeps the fastest (SADDetector.autotune() switches it on for one forward pass).
AUTOTUNE: bool = False
# bf16 chains: merge the branches of a stage into one dispatch (sad_mlp_chain_multi_bf16)?
MERGE_BF16: bool = True
# bf16 stages with an aggregation layer: split pooling (bf16 pooled rows + continuation rows, no atomics, no zero fill; sa_module.can_split)?
SPLIT_POOL: bool = not os.environ.get("SAD_NO_SPLIT_POOL")


class _timed:
    __slots__ = ("kind", "name", "ev")

    def __init__(self, kind: str, name: str = ""):
        self.kind, self.name, self.ev = kind, name, None

    def __enter__(self):
        if LAUNCH_LOG is not None:
            self.ev = torch.cuda.Event(enable_timing=True)
            self.ev.record(torch.cuda.current_stream())
        return self

    def __exit__(self, *exc):
        if self.ev is not None:
            end = torch.cuda.Event(enable_timing=True)
            end.record(torch.cuda.current_stream())
            LAUNCH_LOG.append((self.kind, self.name, self.ev, end))
        return False


def _on_current_device(t: torch.Tensor, name: str) -> None:
    """The C-ABI launches on the CURRENT device's stream ("device chosen by caller"):
    a tensor that lives on another GPU would be dereferenced by a kernel running on the wrong one."""
    cur = torch.cuda.current_device()
    if t.device.index != cur:
        raise RuntimeError(f"{name}: tensor is on {t.device} but the current device is cuda:{cur}; "
                           f"wrap the call in `with torch.cuda.device({t.device.index}):`")


def _need(t: torch.Tensor, name: str, dtype, ndim: int) -> torch.Tensor:
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name}: expected a torch.Tensor")
    if not t.is_cuda:
        raise RuntimeError(f"{name}: expected a GPU tensor (sad_amd has no CPU path)")
    _on_current_device(t, name)
    if dtype is not None and t.dtype != dtype:
        raise TypeError(f"{name}: expected dtype {dtype}, got {t.dtype}")
    if t.dim() != ndim:
        raise ValueError(f"{name}: expected {ndim} dims, got shape {tuple(t.shape)}")
    if not t.is_contiguous():
        _unrecordable(f"{name}: strided copy")
    return t.contiguous()


def _f32(v) -> float:
    return float(np.float32(v))


def _ptr(t: Optional[torch.Tensor]):
    return t.data_ptr() if t is not None else None


def _results(*ts):
    """The results that were asked for (the others are ``None``): the only one alone, several as a tuple."""
    res = tuple(t for t in ts if t is not None)
    return res[0] if len(res) == 1 else res


def _offsets(offsets: torch.Tensor, dev, of: str) -> int:
    """B of offsets [B+1] (already through ``_need``), which live on ``dev``, the device of ``of``."""
    if offsets.device != dev:
        raise ValueError(f"offsets must be on the device of {of}")
    B = offsets.shape[0] - 1
    if B < 1:
        raise ValueError("offsets must have B + 1 >= 2 entries")
    return B


def _outputs(spec, out: Optional[tuple], dev, of: str) -> tuple:
    """The buffers a call writes.  ``spec`` = ((name, shape, dtype), ...); ``out`` checked against it, or new buffers."""
    if out is None:
        return tuple(_empty(shape, dtype=dt, device=dev) for _, shape, dt in spec)
    ok = len(out) == len(spec) and all(isinstance(t, torch.Tensor) and tuple(t.shape) == tuple(shape) and t.dtype == dt
                                       and t.is_contiguous() and t.device == dev for t, (_, shape, dt) in zip(out, spec))
    if not ok:
        want = ", ".join(f"{n} {list(shape)} {str(dt).replace('torch.', '')}" for n, shape, dt in spec)
        raise ValueError(f"out: expected contiguous ({want}) on the device of {of}")
    return tuple(out)


def _bytes(fn_name: str, *args) -> int:
    """The byte count of a workspace query of the library that answers through a size_t (and refuses sizes it does not support)."""
    n = ctypes.c_size_t(0)
    check(getattr(lib(), fn_name)(*args, ctypes.byref(n)), fn_name)
    return n.value


def _workspace(nbytes: int, given: Optional[torch.Tensor], dev, maker: str, align: int = 1) -> torch.Tensor:
    """Scratch of ``nbytes`` bytes on ``dev``: a new buffer, or the caller's (from ``maker``), which a kernel will write over its
    whole length: a tensor, on that GPU, contiguous, long enough and aligned, or the call is refused."""
    if given is None:
        return _empty((nbytes,), dtype=torch.uint8, device=dev)
    if (not isinstance(given, torch.Tensor) or not given.is_cuda or given.device != dev or not given.is_contiguous()
            or given.numel() * given.element_size() < nbytes or given.data_ptr() % align):
        raise ValueError(f"workspace: expected a contiguous GPU buffer of at least {nbytes} bytes on {dev}"
                         + (f", {align}-byte aligned" if align > 1 else "") + f" ({maker})")
    return given


def fps(xyz: torch.Tensor, npoint: int) -> torch.Tensor:
    """Farthest point sampling (SPEC.md §2).  xyz [B,N,3] f32 -> idx [B,npoint] int32."""
    xyz = _need(xyz, "xyz", torch.float32, 3)
    B, N, three = xyz.shape
    if three != 3:
        raise ValueError("xyz: last dim must be 3")
    if not 1 <= npoint <= N:
        raise ValueError(f"npoint={npoint} must be in 1..N={N}")
    idx = _empty((B, npoint), dtype=torch.int32, device=xyz.device)
    ws_bytes = lib().sad_fps_workspace_bytes(B, N)
    ws = _empty((ws_bytes,), dtype=torch.uint8, device=xyz.device) if ws_bytes else None
    with _timed("fps", f"N{N}"):
        check(lib().sad_fps_f32(xyz.data_ptr(), B, N, npoint, idx.data_ptr(), _ptr(ws), _stream()), "sad_fps_f32")
    return idx


def ffps(xyz: torch.Tensor, feat_pm: torch.Tensor, npoint: int, w_xyz: float = 1.0) -> torch.Tensor:
    """Feature-distance FPS (SPEC.md §15).  xyz [B,N,3] f32, feat_pm [B,N,C] f32 point-major ->
    idx [B,npoint] int32.  Allocates the B*N*N distance matrix the two-phase kernel needs."""
    xyz = _need(xyz, "xyz", torch.float32, 3)
    feat_pm = _need(feat_pm, "feat_pm", torch.float32, 3)
    B, N, _ = xyz.shape
    if feat_pm.shape[0] != B or feat_pm.shape[1] != N:
        raise ValueError("feat_pm must be [B,N,C]")
    if feat_pm.stride(2) != 1 or feat_pm.stride(0) != N * feat_pm.stride(1):
        feat_pm = feat_pm.contiguous()
    if not 1 <= npoint <= N:
        raise ValueError(f"npoint={npoint} must be in 1..N={N}")
    idx = _empty((B, npoint), dtype=torch.int32, device=xyz.device)
    ws = _empty((lib().sad_ffps_workspace_bytes(B, N),), dtype=torch.uint8, device=xyz.device)
    with _timed("fps", f"F{N}"):
        check(lib().sad_ffps_f32(xyz.data_ptr(), feat_pm.data_ptr(), feat_pm.stride(1), B, N,
                                 feat_pm.shape[2], npoint, float(w_xyz), idx.data_ptr(), ws.data_ptr(),
                                 _stream()), "sad_ffps_f32")
    return idx


def dfps_ffps(xyz: torch.Tensor, feat_pm: torch.Tensor, npoint: int, w_xyz: float = 1.0) -> torch.Tensor:
    """Fused D+F sampling (SPEC.md §15): npoint//2 picks by distance FPS, the rest by F-FPS."""
    half = npoint // 2
    parts = ([fps(xyz, half)] if half else []) + [ffps(xyz, feat_pm, npoint - half, w_xyz)]
    return torch.cat(parts, dim=1)


def gather_xyz(xyz: torch.Tensor, idx: torch.Tensor) -> torch.Tensor:
    """xyz [B,N,3], idx [B,M] -> [B,M,3] (SPEC.md §5)."""
    xyz = _need(xyz, "xyz", torch.float32, 3)
    idx = _need(idx, "idx", torch.int32, 2)
    B, N, _ = xyz.shape
    M = idx.shape[1]
    out = _empty((B, M, 3), dtype=torch.float32, device=xyz.device)
    check(lib().sad_gather_xyz_f32(xyz.data_ptr(), idx.data_ptr(), B, N, M, out.data_ptr(), _stream()),
          "sad_gather_xyz_f32")
    return out


def gather_points(features: torch.Tensor, idx: torch.Tensor) -> torch.Tensor:
    """features [B,C,N] (f32/bf16/f16), idx [B,M] -> [B,C,M] (SPEC.md §5)."""
    features = _need(features, "features", None, 3)
    idx = _need(idx, "idx", torch.int32, 2)
    esz = features.element_size()
    if esz not in (2, 4):
        raise TypeError("features: element size must be 2 or 4 bytes")
    B, C, N = features.shape
    M = idx.shape[1]
    out = _empty((B, C, M), dtype=features.dtype, device=features.device)
    check(lib().sad_gather_points(features.data_ptr(), idx.data_ptr(), B, C, N, M, esz,
                                  out.data_ptr(), _stream()), "sad_gather_points")
    return out


def group_points(features: torch.Tensor, idx: torch.Tensor) -> torch.Tensor:
    """features [B,C,N] (f32/bf16/f16), idx [B,M,S] -> [B,C,M,S] (SPEC.md §5)."""
    features = _need(features, "features", None, 3)
    idx = _need(idx, "idx", torch.int32, 3)
    esz = features.element_size()
    if esz not in (2, 4):
        raise TypeError("features: element size must be 2 or 4 bytes")
    B, C, N = features.shape
    _, M, S = idx.shape
    out = _empty((B, C, M, S), dtype=features.dtype, device=features.device)
    with _timed("group_points", f"C{C}N{N}M{M}S{S}"):
        check(lib().sad_group_points(features.data_ptr(), idx.data_ptr(), B, C, N, M, S, esz,
                                     out.data_ptr(), _stream()), "sad_group_points")
    return out


def group_points_grad(grad_out: torch.Tensor, idx: torch.Tensor, N: int, point_major: bool = False,
                      via_point_major: bool = True) -> torch.Tensor:
    """Backward of ``group_points`` / ``gather_points`` (SPEC.md §16): grad_out [B,C,M,S] f32 (or [B,C,M] with idx [B,M]) ->
    grad_feat [B,C,N] (scatter-add), or [B,N,C] with ``point_major=True``.  By default the sum is formed point-major (contiguous
    float atomics, ~10x faster) and transposed at the end; ``via_point_major=False`` uses the direct channel-major scatter."""
    if isinstance(grad_out, torch.Tensor) and grad_out.dim() == 3 and isinstance(idx, torch.Tensor):
        grad_out, idx = grad_out.unsqueeze(-1), idx.unsqueeze(-1)
    grad_out = _need(grad_out, "grad_out", torch.float32, 4)
    idx = _need(idx, "idx", torch.int32, 3)
    B, C, M, S = grad_out.shape
    if tuple(idx.shape) != (B, M, S):
        raise ValueError("idx must be [B,M,S]")
    pm = bool(point_major or via_point_major)
    _unrecordable("group_points_grad: zero fill")
    g = torch.zeros((B, N, C) if pm else (B, C, N), dtype=torch.float32, device=grad_out.device)      # the kernels add (float atomics)
    name = "sad_group_points_grad_pm_f32" if pm else "sad_group_points_grad_f32"
    with _timed("group_points_grad", f"C{C}N{N}M{M}S{S}" + ("pm" if pm else "cm")):
        check(getattr(lib(), name)(grad_out.data_ptr(), idx.data_ptr(), B, C, N, M, S, g.data_ptr(), _stream()), name)
    return g.transpose(1, 2).contiguous() if pm and not point_major else g


def max_pool_s_with_arg(x: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """x [B,C,M,S] f32 -> (out [B,C,M], arg [B,C,M] int32): the maximum over S and its position, ties -> lowest s (SPEC.md §16)."""
    x = _need(x, "x", torch.float32, 4)
    B, C, M, S = x.shape
    out = _empty((B, C, M), dtype=torch.float32, device=x.device)
    arg = _empty((B, C, M), dtype=torch.int32, device=x.device)
    with _timed("max_pool_s", f"C{C}M{M}S{S}"):
        check(lib().sad_max_pool_s_f32(x.data_ptr(), B, C, M, S, out.data_ptr(), arg.data_ptr(), _stream()), "sad_max_pool_s_f32")
    return out, arg


def max_pool_s_grad(grad_out: torch.Tensor, arg: torch.Tensor, S: int) -> torch.Tensor:
    """Backward of ``max_pool_s_with_arg``: grad_out [B,C,M] f32, arg [B,C,M] int32 -> grad_x [B,C,M,S], grad_out in the arg-max
    slot and 0 elsewhere (every element written: no zero fill)."""
    grad_out = _need(grad_out, "grad_out", torch.float32, 3)
    arg = _need(arg, "arg", torch.int32, 3)
    B, C, M = grad_out.shape
    if tuple(arg.shape) != (B, C, M):
        raise ValueError("arg must have the shape of grad_out")
    gx = _empty((B, C, M, int(S)), dtype=torch.float32, device=grad_out.device)
    with _timed("max_pool_s_grad", f"C{C}M{M}S{S}"):
        check(lib().sad_max_pool_s_grad_f32(grad_out.data_ptr(), arg.data_ptr(), B, C, M, int(S), gx.data_ptr(), _stream()),
              "sad_max_pool_s_grad_f32")
    return gx


def subsample_pad(points: torch.Tensor, offsets: torch.Tensor, n_points: int, seed: int = 0,
                  out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Ragged scenes -> a fixed point count on the GPU (SPEC.md §17; the step before the path).
    points [total, C] f32 (all scenes concatenated), offsets [B+1] int32 on the GPU -> [B, n_points, C]:
    more points than needed = an evenly spread subset in file order, fewer = all points then hashed
    repeats, empty = zeros.  Same rows as the host loader ``io.fix_size(points_b, n_points, seed, scene=b)``."""
    points = _need(points, "points", torch.float32, 2)
    offsets = _need(offsets, "offsets", torch.int32, 1)
    B = _offsets(offsets, points.device, "points")
    C = points.shape[1]
    out, = _outputs((("out", (B, n_points, C), torch.float32),), None if out is None else (out,), points.device, "points")
    check(lib().sad_subsample_pad_f32(points.data_ptr(), offsets.data_ptr(), B, C, int(n_points),
                                      int(seed) & 0xFFFFFFFF, out.data_ptr(), _stream()), "sad_subsample_pad_f32")
    return out


def ball_query(radius: Union[float, torch.Tensor], nsample: int, xyz: torch.Tensor,
               new_xyz: torch.Tensor) -> torch.Tensor:
    """Ball query (SPEC.md §3).  ``radius``: Python float (fixed) or [B,M] f32 tensor (adaptive,
    per centroid).  xyz [B,N,3], new_xyz [B,M,3] -> idx [B,M,nsample] int32."""
    xyz = _need(xyz, "xyz", torch.float32, 3)
    new_xyz = _need(new_xyz, "new_xyz", torch.float32, 3)
    B, N, _ = xyz.shape
    M = new_xyz.shape[1]
    if new_xyz.shape[0] != B:
        raise ValueError("xyz / new_xyz batch mismatch")
    idx = _empty((B, M, nsample), dtype=torch.int32, device=xyz.device)
    if isinstance(radius, torch.Tensor):
        rad = _need(radius, "radius", torch.float32, 2)
        if tuple(rad.shape) != (B, M):
            raise ValueError(f"radius tensor must be [B,M]=({B},{M})")
        check(lib().sad_ball_query_f32(xyz.data_ptr(), new_xyz.data_ptr(), 0.0, rad.data_ptr(), B, N, M,
                                       nsample, idx.data_ptr(), _stream()), "sad_ball_query_f32")
    else:
        check(lib().sad_ball_query_f32(xyz.data_ptr(), new_xyz.data_ptr(), _f32(radius), None, B, N, M, nsample, idx.data_ptr(), _stream()),
              "sad_ball_query_f32")
    return idx


def ball_query_multi(radii: Sequence[float], nsamples: Sequence[int], xyz: torch.Tensor,
                     new_xyz: torch.Tensor, radius_pc: Optional[torch.Tensor] = None,
                     return_counts: bool = False):
    """Several radii over the same (xyz, new_xyz): d2 is evaluated once per pair.  With
    ``radius_pc`` [B,M] the radius of branch r for centroid (b,m) is radii[r]*radius_pc[b,m]
    (SPEC.md §8 step 5).  Returns one idx [B,M,nsamples[r]] per radius; with ``return_counts`` also
    one int32 [B,M] per radius = accepted points capped at nsample (the non-padding rows of each
    group, which lets the fused MLP skip the padding without scanning idx)."""
    xyz = _need(xyz, "xyz", torch.float32, 3)
    new_xyz = _need(new_xyz, "new_xyz", torch.float32, 3)
    B, N, _ = xyz.shape
    M = new_xyz.shape[1]
    n = len(radii)
    if n != len(nsamples) or not 1 <= n <= _lib.MAX_RADII:
        raise ValueError(f"need 1..{_lib.MAX_RADII} radii with matching nsamples")
    outs = [_empty((B, M, s), dtype=torch.int32, device=xyz.device) for s in nsamples]
    r_arr = (ctypes.c_float * n)(*[_f32(r) for r in radii])
    s_arr = (ctypes.c_int * n)(*[int(s) for s in nsamples])
    p_arr = (vp * n)(*[o.data_ptr() for o in outs])
    cnts = [_empty((B, M), dtype=torch.int32, device=xyz.device) for _ in nsamples] if return_counts else None
    c_arr = (vp * n)(*[c.data_ptr() for c in cnts]) if return_counts else None
    pc = None
    if radius_pc is not None:
        radius_pc = _need(radius_pc, "radius_pc", torch.float32, 2)
        if tuple(radius_pc.shape) != (B, M):
            raise ValueError(f"radius_pc must be [B,M]=({B},{M})")
        pc = radius_pc.data_ptr()
    if pc is None and N >= GRID_MIN_POINTS and N <= 65536 and min(radii) > 0:
        # grid-pruned kernel: same indices, ~100x fewer pair tests (csrc/ball_query_grid.hip)
        ws = _empty((lib().sad_ball_query_grid_workspace_bytes(B, N),), dtype=torch.uint8,
                         device=xyz.device)
        with _timed("ball_query", f"N{N}M{M}x{n}"):
            check(lib().sad_ball_query_grid_f32(xyz.data_ptr(), new_xyz.data_ptr(), n, r_arr, s_arr, p_arr,
                                                c_arr, B, N, M, ws.data_ptr(), _stream()),
                  "sad_ball_query_grid_f32")
        return (outs, cnts) if return_counts else outs
    with _timed("ball_query", f"N{N}M{M}x{n}"):
        check(lib().sad_ball_query_multi_f32(xyz.data_ptr(), new_xyz.data_ptr(), n, r_arr, pc, s_arr,
                                             p_arr, c_arr, B, N, M, _stream()), "sad_ball_query_multi_f32")
    return (outs, cnts) if return_counts else outs


def knn_query(k: int, xyz: torch.Tensor, new_xyz: torch.Tensor) -> torch.Tensor:
    """k nearest neighbours sorted by (d2, index) (SPEC.md §4).  -> idx [B,M,k] int32."""
    xyz = _need(xyz, "xyz", torch.float32, 3)
    new_xyz = _need(new_xyz, "new_xyz", torch.float32, 3)
    B, N, _ = xyz.shape
    M = new_xyz.shape[1]
    idx = _empty((B, M, k), dtype=torch.int32, device=xyz.device)
    check(lib().sad_knn_f32(xyz.data_ptr(), new_xyz.data_ptr(), B, N, M, k, idx.data_ptr(), _stream()),
          "sad_knn_f32")
    return idx


def three_nn(unknown: torch.Tensor, known: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """The three nearest known points of every unknown point (SPEC.md §18).  unknown [B,n,3], known [B,m,3] f32, m >= 1 ->
    (dist2 [B,n,3] f32 squared distances, idx [B,n,3] int32, w [B,n,3] f32 interpolation weights), ascending by (d2, j);
    slots beyond m hold d2 = +inf, idx = 0, w = 0."""
    unknown = _need(unknown, "unknown", torch.float32, 3)
    known = _need(known, "known", torch.float32, 3)
    B, n, three = unknown.shape
    if three != 3 or known.shape[2] != 3 or known.shape[0] != B:
        raise ValueError("unknown [B,n,3] and known [B,m,3] expected")
    m = known.shape[1]
    dist2 = _empty((B, n, 3), dtype=torch.float32, device=unknown.device)
    idx = _empty((B, n, 3), dtype=torch.int32, device=unknown.device)
    w = _empty((B, n, 3), dtype=torch.float32, device=unknown.device)
    with _timed("three_nn", f"n{n}m{m}"):
        check(lib().sad_three_nn_f32(unknown.data_ptr(), known.data_ptr(), B, n, m, dist2.data_ptr(), idx.data_ptr(),
                                     w.data_ptr(), _stream()), "sad_three_nn_f32")
    return dist2, idx, w


def three_interpolate(feat: torch.Tensor, idx: torch.Tensor, w: torch.Tensor, point_major: bool = False,
                      out: Optional[torch.Tensor] = None, col_off: int = 0) -> torch.Tensor:
    """Weighted sum of three known features per unknown point (SPEC.md §18), exact.  idx [B,n,3] int32 in [0,m), w [B,n,3] f32
    (from ``three_nn`` or computed by the caller).  Channel-major: feat [B,C,m] -> [B,C,n].  ``point_major``: feat [B,m,C] ->
    [B,n,C], or written into columns [col_off, col_off + C) of a contiguous ``out`` [B,n,ld] (the other columns untouched)."""
    feat = _need(feat, "feat", torch.float32, 3)
    idx = _need(idx, "idx", torch.int32, 3)
    w = _need(w, "w", torch.float32, 3)
    B, n = idx.shape[0], idx.shape[1]
    if idx.shape[2] != 3 or tuple(w.shape) != tuple(idx.shape) or feat.shape[0] != B:
        raise ValueError("idx and w must be [B,n,3] and feat must have the same B")
    C, m = (feat.shape[2], feat.shape[1]) if point_major else (feat.shape[1], feat.shape[2])
    if point_major:
        if out is None:
            if col_off != 0:
                raise ValueError("col_off needs an out buffer")
            out = _empty((B, n, C), dtype=torch.float32, device=feat.device)
        if (not out.is_cuda or out.dtype != torch.float32 or not out.is_contiguous() or out.dim() != 3
                or tuple(out.shape[:2]) != (B, n) or out.device != feat.device):
            raise ValueError("out: expected a contiguous float32 [B,n,ld] tensor on the device of feat")
        ld = out.shape[2]
    else:
        if out is not None or col_off != 0:
            raise ValueError("out / col_off apply to the point-major layout only")
        out = _empty((B, C, n), dtype=torch.float32, device=feat.device)
        ld = n
    with _timed("three_interpolate", f"C{C}" + ("pm" if point_major else "cm")):
        check(lib().sad_three_interpolate_f32(feat.data_ptr(), idx.data_ptr(), w.data_ptr(), B, C, m, n, int(bool(point_major)),
                                              out.data_ptr(), ld, int(col_off), _stream()), "sad_three_interpolate_f32")
    return out


def three_interpolate_grad(grad_out: torch.Tensor, idx: torch.Tensor, w: torch.Tensor, m: int,
                           point_major: bool = False) -> torch.Tensor:
    """Backward of ``three_interpolate`` (SPEC.md §18): grad_out [B,C,n] (or [B,n,C] with ``point_major=True``), idx / w [B,n,3] ->
    grad_feat [B,C,m] (or [B,m,C]): ``grad_feat[.., idx_k] += w_k * grad_out``.  The sum is formed point-major (contiguous float
    atomics) and transposed at the end for the channel-major layout.  idx and w get no gradient."""
    grad_out = _need(grad_out, "grad_out", torch.float32, 3)
    idx = _need(idx, "idx", torch.int32, 3)
    w = _need(w, "w", torch.float32, 3)
    (B, n, C) = grad_out.shape if point_major else (grad_out.shape[0], grad_out.shape[2], grad_out.shape[1])
    if tuple(idx.shape) != (B, n, 3) or tuple(w.shape) != (B, n, 3):
        raise ValueError("idx and w must be [B,n,3]")
    _unrecordable("three_interpolate_grad: zero fill")
    g = torch.zeros((B, int(m), C), dtype=torch.float32, device=grad_out.device)      # the kernel adds (float atomics)
    with _timed("three_interpolate_grad", f"C{C}" + ("pm" if point_major else "cm")):
        check(lib().sad_three_interpolate_grad_f32(grad_out.data_ptr(), idx.data_ptr(), w.data_ptr(), B, C, n, int(m), int(bool(point_major)),
                                                   g.data_ptr(), _stream()), "sad_three_interpolate_grad_f32")
    return g if point_major else g.transpose(1, 2).contiguous()


def _boxes(t: torch.Tensor, name: str, batched: bool = True) -> torch.Tensor:
    """boxes [B,K,D] (or [K,D] when not ``batched``) f32 with D >= 7 fields (cx,cy,cz,l,w,h,yaw,...) (SPEC.md §19)."""
    t = _need(t, name, torch.float32, 3 if batched else 2)
    if t.shape[-1] < 7:
        raise ValueError(f"{name}: box rows need at least 7 fields (cx,cy,cz,l,w,h,yaw), got {t.shape[-1]}")
    return t


def _boxes_iou(a: torch.Tensor, b: torch.Tensor, mode: int, kind: str) -> torch.Tensor:
    batched = isinstance(a, torch.Tensor) and a.dim() == 3
    a = _boxes(a, "a", batched)
    b = _boxes(b, "b", batched)
    if not batched:
        a, b = a.unsqueeze(0), b.unsqueeze(0)
    B, Ka, Da = a.shape
    if b.shape[0] != B or b.device != a.device:
        raise ValueError("a and b must have the same batch size and device")
    Kb, Db = b.shape[1], b.shape[2]
    iou = _empty((B, Ka, Kb), dtype=torch.float32, device=a.device)
    with _timed("boxes_iou", f"{kind}Ka{Ka}Kb{Kb}"):
        check(lib().sad_boxes_iou_f32(a.data_ptr(), b.data_ptr(), B, Ka, Kb, Da, Db, mode, iou.data_ptr(), _stream()),
              "sad_boxes_iou_f32")
    return iou if batched else iou[0]


def boxes_iou_bev(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """Pairwise rotated BEV IoU (SPEC.md §19.3, = §13 ``iou_bev(a_i, b_j)``).  a [B,Ka,Da], b [B,Kb,Db] -> [B,Ka,Kb], or
    unbatched a [Ka,Da], b [Kb,Db] -> [Ka,Kb]; rows of D >= 7 floats (cx,cy,cz,l,w,h,yaw,...).  No gradient."""
    return _boxes_iou(a, b, 0, "bev")


def boxes_iou3d(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """Pairwise rotated 3-D IoU (SPEC.md §19.3: the §13 BEV intersection times the z overlap over the union of the
    volumes).  Shapes as ``boxes_iou_bev``.  No gradient."""
    return _boxes_iou(a, b, 1, "3d")


def _xyz_boxes(xyz: torch.Tensor, boxes: torch.Tensor):
    """xyz [B,N,3] and boxes [B,K,D] of one batch on one device -> (xyz, boxes, B, N, K, D)."""
    xyz = _need(xyz, "xyz", torch.float32, 3)
    boxes = _boxes(boxes, "boxes")
    B, N, three = xyz.shape
    if three != 3 or boxes.shape[0] != B or boxes.device != xyz.device:
        raise ValueError("xyz [B,N,3] and boxes [B,K,D] on one device expected")
    return xyz, boxes, B, N, boxes.shape[1], boxes.shape[2]


def points_in_boxes(xyz: torch.Tensor, boxes: torch.Tensor) -> torch.Tensor:
    """For each point the lowest index of a box that contains it, else -1 (SPEC.md §19.1).  xyz [B,N,3] f32,
    boxes [B,K,D] f32 (D >= 7, centre / size / yaw) -> box_idx [B,N] int32."""
    xyz, boxes, B, N, K, D = _xyz_boxes(xyz, boxes)
    box_idx = _empty((B, N), dtype=torch.int32, device=xyz.device)
    with _timed("points_in_boxes", f"N{N}K{K}"):
        check(lib().sad_points_in_boxes_f32(xyz.data_ptr(), boxes.data_ptr(), B, N, K, D, box_idx.data_ptr(), _stream()),
              "sad_points_in_boxes_f32")
    return box_idx


def roipoint_pool3d(xyz: torch.Tensor, feat_pm: Optional[torch.Tensor], boxes: torch.Tensor, extra_width: float,
                    num_sampled_points: int, return_idx: bool = False):
    """RoI point pooling (SPEC.md §19.2).  Per box (enlarged by ``extra_width`` on every side) the first
    ``num_sampled_points`` = S points in ascending index order, repeated cyclically when fewer fall inside.
    xyz [B,N,3], feat_pm [B,N,C] point-major or None, boxes [B,K,D] -> (pooled [B,K,S,3+C] rows [xyz || feat],
    empty [B,K] int32 1 = no point inside (rows zero)[, idx [B,K,S] int32]).  1 <= S <= 8192.  No gradient."""
    xyz, boxes, B, N, K, D = _xyz_boxes(xyz, boxes)
    C = 0
    if feat_pm is not None:
        feat_pm = _need(feat_pm, "feat_pm", torch.float32, 3)
        if tuple(feat_pm.shape[:2]) != (B, N) or feat_pm.device != xyz.device:
            raise ValueError("feat_pm: expected [B,N,C] on the device of xyz")
        C = feat_pm.shape[2]
    S = int(num_sampled_points)
    if S < 1:
        raise ValueError(f"num_sampled_points={S} must be >= 1")
    pooled = _empty((B, K, S, 3 + C), dtype=torch.float32, device=xyz.device)
    empty = _empty((B, K), dtype=torch.int32, device=xyz.device)
    idx = _empty((B, K, S), dtype=torch.int32, device=xyz.device) if return_idx else None
    with _timed("roipoint_pool3d", f"N{N}K{K}S{S}C{C}"):
        check(lib().sad_roipoint_pool3d_f32(xyz.data_ptr(), feat_pm.data_ptr() if C else None, boxes.data_ptr(), B, N, K, D, C,
                                            _f32(extra_width), S, pooled.data_ptr(), empty.data_ptr(), _ptr(idx), _stream()),
              "sad_roipoint_pool3d_f32")
    return (pooled, empty, idx) if return_idx else (pooled, empty)


VOXEL_MODES = {"sum": 0, "mean": 1, "max": 2}


def _voxel_points(points: torch.Tensor, offsets: Optional[torch.Tensor], name: str = "points", min_c: int = 3):
    """Ragged ``points [total,C]`` + ``offsets [B+1]`` int32 on the GPU, or a batch ``points [B,N,C]`` with ``offsets=None``
    (offsets[b] = b*N) -> (rows [total,C] contiguous, offsets, B) (SPEC.md §20)."""
    if offsets is None:
        points = _need(points, name, torch.float32, 3)
        B, N, C = points.shape
        if B < 1:
            raise ValueError(f"{name}: empty batch")
        if B * N >= 1 << 30:
            raise ValueError(f"{name}: too many points")
        offsets = torch.arange(0, (B + 1) * N, N, dtype=torch.int32, device=points.device) if N else \
            torch.zeros((B + 1,), dtype=torch.int32, device=points.device)
        points = points.view(B * N, C)
    else:
        points = _need(points, name, torch.float32, 2)
        offsets = _need(offsets, "offsets", torch.int32, 1)
        B = _offsets(offsets, points.device, name)
    if points.shape[1] < min_c:
        raise ValueError(f"{name}: rows need at least {min_c} columns, got {points.shape[1]}")
    return points, offsets, B


def _voxel_grid(voxel_size, point_range):
    """(vx,vy,vz), (x0,y0,z0,x1,y1,z1) -> two host float arrays, Python floats rounded to binary32."""
    if len(voxel_size) != 3 or len(point_range) != 6:
        raise ValueError("voxel_size must have 3 entries (vx,vy,vz) and point_range 6 (x0,y0,z0,x1,y1,z1)")
    return (ctypes.c_float * 3)(*[_f32(v) for v in voxel_size]), (ctypes.c_float * 6)(*[_f32(v) for v in point_range])


def voxel_workspace(total_points: int, B: int, max_voxels: int, device) -> torch.Tensor:
    """Scratch of the §20 operators for (total_points, B, max_voxels); contents arbitrary, reusable call after call on one stream."""
    return _workspace(_bytes("sad_voxel_workspace_bytes", int(total_points), int(B), int(max_voxels)), None, device, "ops.voxel_workspace")


def voxel_coords(points: torch.Tensor, offsets: Optional[torch.Tensor], voxel_size, point_range) -> torch.Tensor:
    """Voxel coordinate of every point (SPEC.md §20.1).  points [total,C] f32 + offsets [B+1] int32, or points [B,N,C] with
    ``offsets=None`` -> coors [total,4] int32 = (b, z, y, x), or (b,-1,-1,-1) for a point outside ``point_range``."""
    vs, pr = _voxel_grid(voxel_size, point_range)
    points, offsets, B = _voxel_points(points, offsets)
    total, C = points.shape
    coors = _empty((total, 4), dtype=torch.int32, device=points.device)
    with _timed("voxel_coords", f"n{total}"):
        check(lib().sad_voxel_coords_f32(points.data_ptr(), offsets.data_ptr(), total, B, C, vs, pr, coors.data_ptr(), _stream()),
              "sad_voxel_coords_f32")
    return coors


def voxel_index(points: torch.Tensor, offsets: Optional[torch.Tensor], voxel_size, point_range, max_voxels: int,
                workspace: Optional[torch.Tensor] = None):
    """Dynamic voxel index (SPEC.md §20.3): voxels numbered per scene in order of first appearance, at most ``max_voxels``.
    -> (point2voxel [total] int32 (scene-local number, -1 = out of range or dropped), coors [B,V,3] int32 (z,y,x),
    count [B,V] int32 (all members), voxel_num [B] int32).  Deterministic, bit-equal to the reference.  No gradient."""
    vs, pr = _voxel_grid(voxel_size, point_range)
    points, offsets, B = _voxel_points(points, offsets)
    V = int(max_voxels)
    if V < 1:
        raise ValueError(f"max_voxels={V} must be >= 1")
    total, C = points.shape
    dev = points.device
    ws = _workspace(_bytes("sad_voxel_workspace_bytes", total, B, V), workspace, dev, "ops.voxel_workspace", 16)
    p2v = _empty((total,), dtype=torch.int32, device=dev)
    coors = _empty((B, V, 3), dtype=torch.int32, device=dev)
    count = _empty((B, V), dtype=torch.int32, device=dev)
    voxel_num = _empty((B,), dtype=torch.int32, device=dev)
    with _timed("voxel_index", f"n{total}V{V}"):
        check(lib().sad_voxel_index_f32(points.data_ptr(), offsets.data_ptr(), total, B, C, vs, pr, V, p2v.data_ptr(), coors.data_ptr(),
                                        count.data_ptr(), voxel_num.data_ptr(), ws.data_ptr(), _stream()), "sad_voxel_index_f32")
    return p2v, coors, count, voxel_num


def voxelize(points: torch.Tensor, offsets: Optional[torch.Tensor], voxel_size, point_range, max_points: int, max_voxels: int,
             workspace: Optional[torch.Tensor] = None):
    """Hard voxelization (SPEC.md §20.4): the first ``max_voxels`` voxels of each scene in order of first appearance, the
    first ``max_points`` points of each in row order.  -> (voxels [B,V,T,C] f32 (unused slots 0), coors [B,V,3] int32 (z,y,x),
    num_points [B,V] int32, voxel_num [B] int32).  Deterministic, bit-equal to the reference.  No gradient."""
    vs, pr = _voxel_grid(voxel_size, point_range)
    points, offsets, B = _voxel_points(points, offsets)
    T, V = int(max_points), int(max_voxels)
    if T < 1 or V < 1:
        raise ValueError(f"max_points={T} and max_voxels={V} must be >= 1")
    total, C = points.shape
    dev = points.device
    ws = _workspace(_bytes("sad_voxel_workspace_bytes", total, B, V), workspace, dev, "ops.voxel_workspace", 16)
    voxels = _empty((B, V, T, C), dtype=torch.float32, device=dev)
    coors = _empty((B, V, 3), dtype=torch.int32, device=dev)
    num_points = _empty((B, V), dtype=torch.int32, device=dev)
    voxel_num = _empty((B,), dtype=torch.int32, device=dev)
    with _timed("voxelize", f"n{total}T{T}V{V}"):
        check(lib().sad_voxelize_f32(points.data_ptr(), offsets.data_ptr(), total, B, C, vs, pr, T, V, voxels.data_ptr(), coors.data_ptr(),
                                     num_points.data_ptr(), voxel_num.data_ptr(), ws.data_ptr(), _stream()), "sad_voxelize_f32")
    return voxels, coors, num_points, voxel_num


def voxel_reduce(feat: torch.Tensor, point2voxel: torch.Tensor, offsets: Optional[torch.Tensor], max_voxels: int, mode: str = "mean",
                 workspace: Optional[torch.Tensor] = None, return_count: bool = False):
    """Reduction of point features over voxels (SPEC.md §20.5).  feat [total,Cf] f32 + offsets, or feat [B,N,Cf] with
    ``offsets=None``; point2voxel [total] int32 from ``voxel_index``.  ``mode`` "sum" / "mean" -> out [B,V,Cf]; "max" ->
    (out, arg [B,V,Cf] int32 = row of the first member that attains the maximum, -1 for an empty voxel).  The sum runs over
    the members in ascending row order (exact against the reference, unlike a float-atomic scatter).  ``return_count`` appends
    count [B,V] int32.  No gradient here: ``autograd.voxel_reduce``."""
    if mode not in VOXEL_MODES:
        raise ValueError(f"mode must be one of {sorted(VOXEL_MODES)}, got {mode!r}")
    feat, offsets, B = _voxel_points(feat, offsets, "feat", 1)
    point2voxel = _need(point2voxel, "point2voxel", torch.int32, 1)
    total, Cf = feat.shape
    if point2voxel.shape[0] != total or point2voxel.device != feat.device:
        raise ValueError("point2voxel must have one entry per row of feat, on its device")
    V = int(max_voxels)
    if V < 1:
        raise ValueError(f"max_voxels={V} must be >= 1")
    dev = feat.device
    ws = _workspace(_bytes("sad_voxel_workspace_bytes", total, B, V), workspace, dev, "ops.voxel_workspace", 16)
    out = _empty((B, V, Cf), dtype=torch.float32, device=dev)
    arg = _empty((B, V, Cf), dtype=torch.int32, device=dev) if mode == "max" else None
    count = _empty((B, V), dtype=torch.int32, device=dev) if return_count else None
    with _timed("voxel_reduce", f"{mode}n{total}V{V}C{Cf}"):
        check(lib().sad_voxel_reduce_f32(feat.data_ptr(), point2voxel.data_ptr(), offsets.data_ptr(), total, B, Cf, V, VOXEL_MODES[mode],
                                         out.data_ptr(), _ptr(arg), _ptr(count), ws.data_ptr(), _stream()), "sad_voxel_reduce_f32")
    return _results(out, arg, count)


def voxel_reduce_grad(grad_out: torch.Tensor, point2voxel: torch.Tensor, offsets: torch.Tensor, mode: str,
                      aux: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Backward of ``voxel_reduce`` (SPEC.md §20.5), a gather: grad_out [B,V,Cf] -> grad_feat [total,Cf].  ``aux``: count [B,V]
    for "mean", arg [B,V,Cf] for "max".  Rows with point2voxel = -1 get 0."""
    if mode not in VOXEL_MODES:
        raise ValueError(f"mode must be one of {sorted(VOXEL_MODES)}, got {mode!r}")
    grad_out = _need(grad_out, "grad_out", torch.float32, 3)
    point2voxel = _need(point2voxel, "point2voxel", torch.int32, 1)
    offsets = _need(offsets, "offsets", torch.int32, 1)
    B, V, Cf = grad_out.shape
    total = point2voxel.shape[0]
    if offsets.shape[0] != B + 1:
        raise ValueError("offsets must have B + 1 entries")
    if mode != "sum":
        aux = _need(aux, "aux", torch.int32, 2 if mode == "mean" else 3)
        if tuple(aux.shape) != ((B, V) if mode == "mean" else (B, V, Cf)):
            raise ValueError("aux: count [B,V] for mean, arg [B,V,Cf] for max")
    grad_feat = _empty((total, Cf), dtype=torch.float32, device=grad_out.device)
    check(lib().sad_voxel_reduce_grad_f32(grad_out.data_ptr(), point2voxel.data_ptr(), offsets.data_ptr(), total, B, Cf, V, VOXEL_MODES[mode],
                                          aux.data_ptr() if mode != "sum" else None, grad_feat.data_ptr(), _stream()),
          "sad_voxel_reduce_grad_f32")
    return grad_feat


VFE_CLUSTER_CENTER, VFE_VOXEL_CENTER, VFE_RELU = 1, 2, 4


def voxel_encode_workspace(total_points: int, B: int, max_voxels: int, cin: int, cout: int, device) -> torch.Tensor:
    """Scratch of ``voxel_encode`` / ``voxel_decorate`` (``cout=0``) for these sizes; contents arbitrary, reusable call after call
    on one stream."""
    return _workspace(_bytes("sad_voxel_encode_workspace_bytes", int(total_points), int(B), int(max_voxels), int(cin), int(cout)), None, device,
                      "ops.voxel_encode_workspace")


def _vfe_args(points, point2voxel, offsets, max_voxels, coors, voxel_size, point_range, cluster_center, voxel_center, vox_feat,
              max_points, cout, workspace):
    """The arguments ``voxel_decorate`` and ``voxel_encode`` share -> (points, p2v, offsets, coors, vox_feat, total, B, C, V, Cv, vs,
    pr, flags, T, Cin, workspace)."""
    cc, vc = bool(cluster_center), bool(voxel_center)
    points, offsets, B = _voxel_points(points, offsets, "points", 3 if (cc or vc) else 1)
    point2voxel = _need(point2voxel, "point2voxel", torch.int32, 1)
    total, C = points.shape
    dev = points.device
    if point2voxel.shape[0] != total or point2voxel.device != dev:
        raise ValueError("point2voxel must have one entry per row of points, on its device")
    V = int(max_voxels)
    if V < 1:
        raise ValueError(f"max_voxels={V} must be >= 1")
    vs = pr = None
    if vc:
        if coors is None or voxel_size is None or point_range is None:
            raise ValueError("voxel_center needs coors [B,V,3], voxel_size and point_range")
        vs, pr = _voxel_grid(voxel_size, point_range)
        coors = _need(coors, "coors", torch.int32, 3)
        if tuple(coors.shape) != (B, V, 3) or coors.device != dev:
            raise ValueError(f"coors: [{B},{V},3] on the device of points expected")
    else:
        coors = None
    Cv = 0
    if vox_feat is not None:
        vox_feat = _need(vox_feat, "vox_feat", torch.float32, 3)
        if tuple(vox_feat.shape[:2]) != (B, V) or vox_feat.shape[2] < 1 or vox_feat.device != dev:
            raise ValueError(f"vox_feat: [{B},{V},Cv >= 1] on the device of points expected")
        Cv = vox_feat.shape[2]
    T = 0
    if max_points is not None:
        T = int(max_points)
        if T < 1:
            raise ValueError(f"max_points={T} must be >= 1 (None: no cap)")
    cin = C + 3 * cc + 3 * vc + Cv
    # (Cin or Cout outside 1 .. 256: SAD_EUNSUPPORTED from the size query, before anything is launched)
    workspace = _workspace(_bytes("sad_voxel_encode_workspace_bytes", total, B, V, cin, cout), workspace, dev, "ops.voxel_encode_workspace", 16)
    flags = (VFE_CLUSTER_CENTER if cc else 0) | (VFE_VOXEL_CENTER if vc else 0)
    return points, point2voxel, offsets, coors, vox_feat, total, B, C, V, Cv, vs, pr, flags, T, cin, workspace


def voxel_decorate(points: torch.Tensor, point2voxel: torch.Tensor, offsets: Optional[torch.Tensor], max_voxels: int,
                   coors: Optional[torch.Tensor] = None, voxel_size=None, point_range=None, cluster_center: bool = True,
                   voxel_center: bool = True, vox_feat: Optional[torch.Tensor] = None, max_points: Optional[int] = None,
                   workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The decorated rows of the voxel feature encoder (SPEC.md §24), unfused: points [total,C] f32 + offsets (or [B,N,C] with
    ``offsets=None``), point2voxel [total] int32 -> rows [total,Cin] = [points | xyz - mean of the voxel's members | xyz - voxel
    centre | vox_feat[b,v]] as asked for; rows that are not members (point2voxel outside [0,V), or past the first ``max_points`` of
    their voxel) are zero.  ``voxel_center`` needs coors [B,V,3] (z,y,x), ``voxel_size`` and ``point_range``.  No gradient."""
    (points, point2voxel, offsets, coors, vox_feat, total, B, C, V, Cv, vs, pr, flags, T, cin, ws) = _vfe_args(
        points, point2voxel, offsets, max_voxels, coors, voxel_size, point_range, cluster_center, voxel_center, vox_feat, max_points, 0,
        workspace)
    rows = _empty((total, cin), dtype=torch.float32, device=points.device)
    with _timed("voxel_decorate", f"n{total}V{V}C{cin}"):
        check(lib().sad_voxel_decorate_f32(points.data_ptr(), point2voxel.data_ptr(), offsets.data_ptr(), _ptr(coors), _ptr(vox_feat), total, B,
                                           C, V, Cv, vs, pr, flags, T, rows.data_ptr(), ws.data_ptr(), _stream()), "sad_voxel_decorate_f32")
    return rows


def voxel_encode(points: torch.Tensor, point2voxel: torch.Tensor, offsets: Optional[torch.Tensor], max_voxels: int,
                 weight: torch.Tensor, bias: torch.Tensor, coors: Optional[torch.Tensor] = None, voxel_size=None, point_range=None,
                 cluster_center: bool = True, voxel_center: bool = True, relu: bool = True, vox_feat: Optional[torch.Tensor] = None,
                 max_points: Optional[int] = None, return_arg: bool = False, return_pointwise: bool = False,
                 workspace: Optional[torch.Tensor] = None):
    """Voxel feature encoder (SPEC.md §24), fused: the rows of ``voxel_decorate``, one layer ``weight [Cout,Cin]``, ``bias [Cout]``
    (+ ReLU) and the maximum over each voxel's members in one kernel, without the [total,Cout] intermediate.  -> pooled [B,V,Cout]
    (0 for a voxel without members); ``return_arg`` appends arg [B,V,Cout] int32 (lowest member row that attains the maximum, -1
    without members); ``return_pointwise`` appends pointwise [total,Cout] (the layer output of every member row, 0 elsewhere: what
    the next layer of a stack reads).  Equal to the reference under ``==``, bit-equal from call to call.  No gradient here:
    ``autograd.voxel_encode``."""
    weight = _need(weight, "weight", torch.float32, 2)
    bias = _need(bias, "bias", torch.float32, 1)
    cout = weight.shape[0]
    (points, point2voxel, offsets, coors, vox_feat, total, B, C, V, Cv, vs, pr, flags, T, cin, ws) = _vfe_args(
        points, point2voxel, offsets, max_voxels, coors, voxel_size, point_range, cluster_center, voxel_center, vox_feat, max_points, cout,
        workspace)
    dev = points.device
    if weight.shape[1] != cin or bias.shape[0] != cout or weight.device != dev or bias.device != dev:
        raise ValueError(f"weight [Cout,{cin}] and bias [Cout] on the device of points expected, got {tuple(weight.shape)}, {tuple(bias.shape)}")
    pooled = _empty((B, V, cout), dtype=torch.float32, device=dev)
    arg = _empty((B, V, cout), dtype=torch.int32, device=dev) if return_arg else None
    pointwise = _empty((total, cout), dtype=torch.float32, device=dev) if return_pointwise else None
    with _timed("voxel_encode", f"n{total}V{V}C{cin}x{cout}"):
        check(lib().sad_voxel_encode_f32(points.data_ptr(), point2voxel.data_ptr(), offsets.data_ptr(), _ptr(coors), _ptr(vox_feat), total, B, C,
                                         V, Cv, vs, pr, weight.data_ptr(), bias.data_ptr(), cout, flags | (VFE_RELU if relu else 0), T,
                                         pooled.data_ptr(), _ptr(arg), _ptr(pointwise), ws.data_ptr(), _stream()), "sad_voxel_encode_f32")
    return _results(pooled, arg, pointwise)


def _int3(v, name: str, lo: int):
    """int or 3 ints (z,y,x) -> (tuple of 3 Python ints, host int array)."""
    t = (int(v),) * 3 if isinstance(v, (int, np.integer)) else tuple(int(x) for x in v)
    if len(t) != 3:
        raise ValueError(f"{name}: an int or 3 ints (z,y,x) expected, got {v!r}")
    if min(t) < lo:
        raise ValueError(f"{name}: entries must be >= {lo}, got {t}")
    return t, (ctypes.c_int * 3)(*t)


def sparse_conv_geometry(spatial_shape, kernel, stride=1, padding=0, subm: bool = False):
    """Host arithmetic of SPEC.md §21: -> (spatial_shape, kernel, stride, padding, out_shape), tuples of 3 ints (z,y,x).
    ``subm`` demands odd kernel sizes and fixes stride 1 and padding K // 2.  Refuses what the library refuses (sp_geo in
    csrc/spconv.hip): more than 2^31 - 1 cells in either shape, a stride or padding above 65535.  Needs no GPU."""
    G, _ = _int3(spatial_shape, "spatial_shape", 1)
    K, _ = _int3(kernel, "kernel", 1)
    if max(K) > 3:
        raise ValueError(f"kernel: sizes 1 .. 3 are implemented, got {K}")
    if G[0] * G[1] * G[2] > 2 ** 31 - 1:
        raise ValueError(f"spatial_shape {G} exceeds 2^31 - 1 cells")
    if subm:
        if any(k % 2 == 0 for k in K):
            raise ValueError(f"a submanifold convolution needs odd kernel sizes, got {K}")
        s, p = (1, 1, 1), tuple(k // 2 for k in K)
        if _int3(stride, "stride", 1)[0] != s:
            raise ValueError("a submanifold convolution has stride 1")
        if padding not in (0, None) and _int3(padding, "padding", 0)[0] != p:
            raise ValueError("a submanifold convolution has padding K // 2")
    else:
        s, _ = _int3(stride, "stride", 1)
        p, _ = _int3(padding, "padding", 0)
        if max(s) > 65535 or max(p) > 65535:
            raise ValueError(f"stride {s} / padding {p} above 65535")
    if any(g + 2 * q - k < 0 for g, q, k in zip(G, p, K)):
        raise ValueError(f"kernel {K} does not fit the padded grid {G} + 2 * {p}")
    O = tuple((g + 2 * q - k) // t + 1 for g, q, k, t in zip(G, p, K, s))
    if O[0] * O[1] * O[2] > 2 ** 31 - 1:
        raise ValueError(f"out_shape {O} exceeds 2^31 - 1 cells")
    return G, K, s, p, O


def _sparse_coors(coors: torch.Tensor, offsets: torch.Tensor):
    coors = _need(coors, "coors", torch.int32, 2)
    offsets = _need(offsets, "offsets", torch.int32, 1)
    if coors.shape[1] != 3:
        raise ValueError(f"coors: [Nv,3] (z,y,x) expected, got {tuple(coors.shape)}")
    return coors, offsets, _offsets(offsets, coors.device, "coors")


def sparse_conv_index(coors: torch.Tensor, offsets: torch.Tensor, spatial_shape, kernel, stride=1, padding=0, subm: bool = False,
                      capacity: Optional[int] = None):
    """Rulebook of a sparse 3-D convolution (SPEC.md §21.1).  coors [Nv,3] int32 (z,y,x), offsets [B+1] int32, both on the GPU ->
    (out_coors [No,3], out_offsets [B+1], nbr [No,Kvol] int32): nbr[o,kk] = the input row that output row o reads at kernel offset
    kk, or -1.  ``subm``: out_coors / out_offsets ARE coors / offsets (the same tensors).  Otherwise the number of output rows is
    known only on the device: with ``capacity=None`` it is read back once (ONE synchronisation of the current stream, as in the
    libraries this replaces); with a ``capacity`` the call stays asynchronous, returns ``capacity`` rows (-1 beyond the true
    total, which is out_offsets[B]) and drops the rows that do not fit.  Integer work, equal to the reference.  No gradient."""
    _unrecordable("sparse_conv_index")
    G, K, s, p, _ = sparse_conv_geometry(spatial_shape, kernel, stride, padding, subm)
    coors, offsets, B = _sparse_coors(coors, offsets)
    Nv, Kvol, dev = coors.shape[0], K[0] * K[1] * K[2], coors.device
    cG, cK, cs, cp = [(ctypes.c_int * 3)(*t) for t in (G, K, s, p)]
    ws = torch.empty((_bytes("sad_spconv_workspace_bytes", Nv, B, cK, cs, int(subm)),), dtype=torch.uint8, device=dev)
    if subm:
        nbr = torch.empty((Nv, Kvol), dtype=torch.int32, device=dev)
        with _timed("spconv_index", f"subm n{Nv}k{Kvol}"):
            check(lib().sad_spconv_index_subm(coors.data_ptr(), offsets.data_ptr(), Nv, B, cG, cK, nbr.data_ptr(), ws.data_ptr(), _stream()),
                  "sad_spconv_index_subm")
        return coors, offsets, nbr
    out_offsets = torch.empty((B + 1,), dtype=torch.int32, device=dev)
    with _timed("spconv_index", f"count n{Nv}k{Kvol}"):
        check(lib().sad_spconv_index_count(coors.data_ptr(), offsets.data_ptr(), Nv, B, cG, cK, cs, cp, out_offsets.data_ptr(), ws.data_ptr(),
                                           _stream()), "sad_spconv_index_count")
    No = int(out_offsets[B].item()) if capacity is None else int(capacity)
    if No < 0:
        raise ValueError(f"capacity={No} must be >= 0")
    out_coors = torch.empty((No, 3), dtype=torch.int32, device=dev)
    nbr = torch.empty((No, Kvol), dtype=torch.int32, device=dev)
    with _timed("spconv_index", f"fill n{Nv}k{Kvol}"):
        check(lib().sad_spconv_index_fill(coors.data_ptr(), offsets.data_ptr(), Nv, B, cG, cK, cs, cp, out_offsets.data_ptr(), No,
                                          out_coors.data_ptr(), nbr.data_ptr(), ws.data_ptr(), _stream()), "sad_spconv_index_fill")
    return out_coors, out_offsets, nbr


# the limits of the sparse-convolution family (csrc/spconv_limits.h): 1 <= Kvol <= 27 (3 x 3 x 3), 1 <= Cin, Cout <= 256
SPARSE_MAX_KVOL, SPARSE_MAX_C = 27, 256


def _sparse_limits(what: str, kvol: int, cin: Optional[int] = None, cout: Optional[int] = None) -> None:
    if not 1 <= kvol <= SPARSE_MAX_KVOL:
        raise ValueError(f"{what}: Kvol = {kvol} must be in 1 .. {SPARSE_MAX_KVOL}")
    if cin is not None and not (1 <= cin <= SPARSE_MAX_C and 1 <= cout <= SPARSE_MAX_C):
        raise ValueError(f"{what}: channels must be in 1 .. {SPARSE_MAX_C}, got {cin} -> {cout}")


class PackedSparseWeight:
    """``W [Kvol,Cout,Cin]`` (+ ``bias [Cout]``) in the fragment layout the convolution kernel reads (``sad_spconv_pack_f32``);
    BatchNorm is folded into W and bias beforehand, as for ``PackedMLP``."""

    def __init__(self, weight: torch.Tensor, bias: Optional[torch.Tensor] = None):
        weight = _need(weight, "weight", torch.float32, 3)
        self.kvol, self.cout, self.cin = (int(x) for x in weight.shape)
        if bias is not None:
            bias = _need(bias, "bias", torch.float32, 1)
            if bias.shape[0] != self.cout or bias.device != weight.device:
                raise ValueError("bias: [Cout] on the device of weight expected")
        _sparse_limits("weight", self.kvol)
        n = lib().sad_spconv_packed_floats(self.kvol, self.cin, self.cout)
        if n == 0:
            raise RuntimeError(f"sparse_conv: Cin = {self.cin}, Cout = {self.cout} unsupported (1 .. {SPARSE_MAX_C} each)")
        self.has_bias = bias is not None
        self.packed = torch.empty((n,), dtype=torch.float32, device=weight.device)
        check(lib().sad_spconv_pack_f32(weight.data_ptr(), _ptr(bias), self.kvol, self.cin, self.cout,
                                        self.packed.data_ptr(), _stream()), "sad_spconv_pack_f32")


def sparse_conv(feat: torch.Tensor, nbr: torch.Tensor, weight, bias: Optional[torch.Tensor] = None,
                residual: Optional[torch.Tensor] = None, relu: bool = False) -> torch.Tensor:
    """Sparse convolution over a rulebook (SPEC.md §21.2).  feat [Nv,Cin] f32, nbr [No,Kvol] int32 (``sparse_conv_index``),
    ``weight`` [Kvol,Cout,Cin] f32 (packed on every call) or a ``PackedSparseWeight`` (then ``bias`` must be None: it is in the
    pack) -> out [No,Cout] = act(bias + sum_kk W[kk] . feat[nbr[:,kk]] (+ residual [No,Cout])).  One accumulator per output
    element, kk then ci ascending: equal to the CPU reference under ``==``.  No gradient."""
    _unrecordable("sparse_conv")
    feat = _need(feat, "feat", torch.float32, 2)
    nbr = _need(nbr, "nbr", torch.int32, 2)
    if isinstance(weight, PackedSparseWeight):
        if bias is not None:
            raise ValueError("bias: already part of the PackedSparseWeight")
        pw = weight
    else:
        pw = PackedSparseWeight(weight, bias)
    Nv, No, dev = feat.shape[0], nbr.shape[0], feat.device
    if feat.shape[1] != pw.cin or nbr.shape[1] != pw.kvol:
        raise ValueError(f"feat {tuple(feat.shape)} / nbr {tuple(nbr.shape)} do not fit weight [Kvol={pw.kvol},Cout={pw.cout},Cin={pw.cin}]")
    if nbr.device != dev or pw.packed.device != dev:
        raise ValueError("feat, nbr and weight must be on one device")
    if residual is not None:
        residual = _need(residual, "residual", torch.float32, 2)
        if tuple(residual.shape) != (No, pw.cout) or residual.device != dev:
            raise ValueError(f"residual: [{No},{pw.cout}] on the device of feat expected, got {tuple(residual.shape)}")
    out = torch.empty((No, pw.cout), dtype=torch.float32, device=dev)
    with _timed("spconv", f"n{No}k{pw.kvol}c{pw.cin}x{pw.cout}"):
        check(lib().sad_spconv_f32(feat.data_ptr(), nbr.data_ptr(), pw.packed.data_ptr(), _ptr(residual), int(bool(relu)), Nv, No, pw.kvol,
                                   pw.cin, pw.cout, out.data_ptr(), _stream()), "sad_spconv_f32")
    return out


def sparse_conv_index_transpose(nbr: torch.Tensor, Nv: int):
    """Transposed rulebook (SPEC.md §21.4).  nbr [No,Kvol] int32, ``Nv`` input rows -> (nbrT [Nv,Kvol] int32, collisions: int32
    scalar tensor on the device): nbrT[i,kk] = the lowest o with nbr[o,kk] == i, -1 if none; collisions = the entries (o,kk) that
    another, lower row shadows.  ``sparse_conv_grad_input`` over nbrT is the true gradient iff collisions == 0.  Integer work,
    equal to the reference.  No gradient."""
    _unrecordable("sparse_conv_index_transpose")
    nbr = _need(nbr, "nbr", torch.int32, 2)
    Nv = int(Nv)
    No, Kvol = nbr.shape
    if Nv < 0:
        raise ValueError(f"Nv={Nv} must be >= 0")
    _sparse_limits("nbr", Kvol)
    nbrT = torch.empty((Nv, Kvol), dtype=torch.int32, device=nbr.device)
    collisions = torch.empty((), dtype=torch.int32, device=nbr.device)
    with _timed("spconv_index", f"transpose n{No}k{Kvol}"):
        check(lib().sad_spconv_index_transpose(nbr.data_ptr(), No, Nv, Kvol, nbrT.data_ptr(), collisions.data_ptr(), _stream()),
              "sad_spconv_index_transpose")
    return nbrT, collisions


def sparse_conv_grad_weight(feat: torch.Tensor, nbr: torch.Tensor, g: torch.Tensor, bias: bool = True, weight: bool = True):
    """Weight gradient of ``sparse_conv`` (SPEC.md §21.4).  feat [Nv,Cin] f32 (the forward's input), nbr [No,Kvol] int32,
    g [No,Cout] f32 (the output gradient AFTER the ReLU mask) -> (grad_W [Kvol,Cout,Cin], grad_bias [Cout] or None with
    ``bias=False``; ``weight=False`` -> (None, grad_bias): the column sums only, no GEMM): grad_W[kk] = sum over the rows o with nbr[o,kk] >= 0 of g[o] (x) feat[nbr[o,kk]].  binary32 sums in an
    order that is not specified (float atomics): within n * 2^-23 * sum |terms| of the exact sum, exact where every partial
    sum is representable, not bit-equal from call to call."""
    _unrecordable("sparse_conv_grad_weight")
    feat = _need(feat, "feat", torch.float32, 2)
    nbr = _need(nbr, "nbr", torch.int32, 2)
    g = _need(g, "g", torch.float32, 2)
    (Nv, cin), (No, kvol), cout, dev = feat.shape, nbr.shape, g.shape[1], feat.device
    if g.shape[0] != No:
        raise ValueError(f"g: one row per row of nbr expected, got {tuple(g.shape)} for nbr {tuple(nbr.shape)}")
    if nbr.device != dev or g.device != dev:
        raise ValueError("feat, nbr and g must be on one device")
    _sparse_limits("sparse_conv_grad_weight", kvol, cin, cout)
    if not (bias or weight):
        raise ValueError("sparse_conv_grad_weight: nothing asked for (bias=False, weight=False)")
    nbytes = _bytes("sad_spconv_grad_weight_workspace_bytes", No, kvol, cin, cout)
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev) if nbytes else None
    grad_w = torch.empty((kvol, cout, cin), dtype=torch.float32, device=dev) if weight else None
    grad_b = torch.empty((cout,), dtype=torch.float32, device=dev) if bias else None
    with _timed("spconv_grad_w", f"n{No}k{kvol}c{cin}x{cout}"):
        check(lib().sad_spconv_grad_weight_f32(feat.data_ptr(), nbr.data_ptr(), g.data_ptr(), Nv, No, kvol, cin, cout, _ptr(grad_w), _ptr(grad_b),
                                               _ptr(ws), _stream()), "sad_spconv_grad_weight_f32")
    return grad_w, grad_b


def sparse_conv_grad_input(g: torch.Tensor, nbrT: torch.Tensor, weight) -> torch.Tensor:
    """Input gradient of ``sparse_conv`` (SPEC.md §21.4).  g [No,Cout] f32 (after the ReLU mask), nbrT [Nv,Kvol] int32
    (``sparse_conv_index_transpose``), ``weight`` = the forward's W [Kvol,Cout,Cin] (transposed and packed on every call) or a
    ``PackedSparseWeight`` made from W.transpose(1, 2) without a bias -> grad_feat [Nv,Cin]: the §21.2 chain over
    (g, nbrT, W^T) on the forward kernel, equal to the reference under ``==``.  The true gradient iff the transposed rulebook
    has no collisions."""
    if isinstance(weight, PackedSparseWeight):
        if weight.has_bias:
            raise ValueError("weight: the packed W^T of a gradient carries no bias")
        pw = weight
    else:
        pw = PackedSparseWeight(_need(weight, "weight", torch.float32, 3).transpose(1, 2).contiguous(), None)
    return sparse_conv(g, nbrT, pw, None, None, False)


def _pool_sizes(Nv: int, No: int, Kvol: int, C: int, what: str) -> None:
    _sparse_limits(what, Kvol)
    if C < 1:
        raise ValueError(f"{what}: at least one channel expected")
    if Nv * C >= 2 ** 31 or No * C >= 2 ** 31:
        raise ValueError(f"{what}: Nv * C and No * C must be below 2^31, got {Nv} and {No} rows of {C}")


def sparse_max_pool(feat: torch.Tensor, nbr: torch.Tensor):
    """Sparse max pool over a rulebook (SPEC.md §22.1).  feat [Nv,C] f32, nbr [No,Kvol] int32 (``sparse_conv_index``, or a
    caller's: entries outside [0, Nv) count as -1) -> (out [No,C] f32, arg [No,C] int32): per channel the maximum over the valid
    entries, ties to the lowest kk, and the global input row it came from; 0.0 and -1 for a row without a valid entry (an absent
    neighbour is absent, not a zero).  Exact: ``out`` is a bit copy of one input element.  No gradient
    (``autograd.sparse_max_pool``)."""
    _unrecordable("sparse_max_pool")
    feat = _need(feat, "feat", torch.float32, 2)
    nbr = _need(nbr, "nbr", torch.int32, 2)
    (Nv, C), (No, Kvol), dev = feat.shape, nbr.shape, feat.device
    if nbr.device != dev:
        raise ValueError("feat and nbr must be on one device")
    _pool_sizes(Nv, No, Kvol, C, "sparse_max_pool")
    out = torch.empty((No, C), dtype=torch.float32, device=dev)
    arg = torch.empty((No, C), dtype=torch.int32, device=dev)
    with _timed("spconv_pool", f"n{No}k{Kvol}c{C}"):
        check(lib().sad_spconv_max_pool_f32(feat.data_ptr(), nbr.data_ptr(), Nv, No, Kvol, C, out.data_ptr(), arg.data_ptr(), _stream()),
              "sad_spconv_max_pool_f32")
    return out, arg


def sparse_max_pool_grad(g: torch.Tensor, arg: torch.Tensor, nbrT: torch.Tensor, Nv: int) -> torch.Tensor:
    """Backward of ``sparse_max_pool`` (SPEC.md §22.2).  g [No,C] f32, arg [No,C] int32 (the forward's), nbrT [Nv,Kvol] int32
    (``sparse_conv_index_transpose`` of the forward's nbr) -> grad_feat [Nv,C]: per element the sum, kk ascending, of g[o][c] over
    o = nbrT[i,kk] with arg[o][c] == i.  A gather: no atomics, bit-equal from call to call, equal to the reference under ``==``.
    The true gradient iff the transposed rulebook has no collisions."""
    _unrecordable("sparse_max_pool_grad")
    g = _need(g, "g", torch.float32, 2)
    arg = _need(arg, "arg", torch.int32, 2)
    nbrT = _need(nbrT, "nbrT", torch.int32, 2)
    (No, C), Kvol, dev, Nv = g.shape, nbrT.shape[1], g.device, int(Nv)
    if tuple(arg.shape) != (No, C):
        raise ValueError(f"arg: the shape of g expected, got {tuple(arg.shape)} for g {tuple(g.shape)}")
    if nbrT.shape[0] != Nv:
        raise ValueError(f"nbrT: {Nv} rows expected, got {tuple(nbrT.shape)}")
    if arg.device != dev or nbrT.device != dev:
        raise ValueError("g, arg and nbrT must be on one device")
    _pool_sizes(Nv, No, Kvol, C, "sparse_max_pool_grad")
    grad_feat = torch.empty((Nv, C), dtype=torch.float32, device=dev)
    with _timed("spconv_pool_grad", f"n{Nv}k{Kvol}c{C}"):
        check(lib().sad_spconv_max_pool_grad_f32(g.data_ptr(), arg.data_ptr(), nbrT.data_ptr(), Nv, No, Kvol, C, grad_feat.data_ptr(), _stream()),
              "sad_spconv_max_pool_grad_f32")
    return grad_feat


def sparse_to_dense(feat: torch.Tensor, out_coors: torch.Tensor, out_offsets: torch.Tensor, out_shape) -> torch.Tensor:
    """SPEC.md §21.3: feat [No,C] f32, out_coors [No,3] int32 (z,y,x), out_offsets [B+1] int32 -> dense [B,C,Oz,Oy,Ox] f32, zero
    where no voxel is and an exact copy elsewhere (the lowest row on a duplicate; rows with a coordinate outside ``out_shape``,
    such as the -1 rows of a fill with spare capacity, are skipped)."""
    _unrecordable("sparse_to_dense")
    feat = _need(feat, "feat", torch.float32, 2)
    out_coors, out_offsets, B = _sparse_coors(out_coors, out_offsets)
    O, cO = _int3(out_shape, "out_shape", 1)
    No, C = feat.shape
    if out_coors.shape[0] != No or out_coors.device != feat.device:
        raise ValueError("out_coors must have one row per row of feat, on its device")
    if C < 1:
        raise ValueError("feat: at least one channel expected")
    ws = torch.empty((_bytes("sad_sparse_to_dense_workspace_bytes", B, cO),), dtype=torch.uint8, device=feat.device)
    dense = torch.empty((B, C) + O, dtype=torch.float32, device=feat.device)
    with _timed("sparse_to_dense", f"n{No}c{C}"):
        check(lib().sad_sparse_to_dense_f32(feat.data_ptr(), out_coors.data_ptr(), out_offsets.data_ptr(), No, B, C, cO, dense.data_ptr(),
                                            ws.data_ptr(), _stream()), "sad_sparse_to_dense_f32")
    return dense


def _nms_outputs(B: int, K: int, P: int, out: Optional[tuple], dev) -> tuple:
    """(keep [B,K], order [B,P], count [B], the caller's workspace or ``None``) of an NMS call; ``out`` = (keep, order, count,
    workspace): the three through ``_outputs``, the fourth is for ``_workspace``."""
    spec = (("keep", (B, K), torch.int32), ("order", (B, P), torch.int32), ("count", (B,), torch.int32))
    if out is not None and len(out) != 4:
        raise ValueError("out: expected (keep, order, count, workspace)")
    return _outputs(spec, None if out is None else out[:3], dev, "boxes") + (None if out is None else out[3],)


def nms_bev_buffers(B: int, K: int, device) -> tuple:
    """(keep [B,K], order [B,K], count [B], workspace) for ``nms_bev(..., out=...)``: a caller that runs NMS every step
    allocates them once (pipeline.py)."""
    return (torch.empty((B, K), dtype=torch.int32, device=device), torch.empty((B, K), dtype=torch.int32, device=device),
            torch.empty((B,), dtype=torch.int32, device=device),
            torch.empty((lib().sad_nms_bev_workspace_bytes(B, K),), dtype=torch.uint8, device=device))


def nms_bev(boxes: torch.Tensor, iou_thr: float, score_thr: float = 0.0, single_kernel: bool = False, out: Optional[tuple] = None
            ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Rotated-box NMS in bird's-eye view (SPEC.md §13).  boxes [B,K,9] f32, K <= 512 ->
    (keep [B,K] int32 0/1, order [B,K] int32 kept indices in rank order (-1 padded), count [B]).
    Default: the three-kernel variant (suppression matrix spread over the chip, workspace allocated
    here); ``single_kernel=True``: one workgroup per scene, no workspace.  Same keep decisions."""
    boxes = _need(boxes, "boxes", torch.float32, 3)
    B, K, nine = boxes.shape
    if nine != 9:
        raise ValueError("boxes: last dim must be 9 (x,y,z,l,w,h,yaw,score,label)")
    keep, order, count, ws = _nms_outputs(B, K, K, out, boxes.device)   # out: buffers from nms_bev_buffers(B, K, device)
    if not single_kernel:
        ws = _workspace(lib().sad_nms_bev_workspace_bytes(B, K), ws, boxes.device, "ops.nms_bev_buffers")
    with _timed("nms", f"K{K}"):
        if single_kernel:
            check(lib().sad_nms_bev_f32(boxes.data_ptr(), B, K, _f32(iou_thr), _f32(score_thr), keep.data_ptr(), order.data_ptr(),
                                        count.data_ptr(), _stream()), "sad_nms_bev_f32")
        else:
            check(lib().sad_nms_bev_ws_f32(boxes.data_ptr(), B, K, _f32(iou_thr), _f32(score_thr), keep.data_ptr(), order.data_ptr(),
                                           count.data_ptr(), ws.data_ptr(), _stream()), "sad_nms_bev_ws_f32")
    return keep, order, count


def _nms_boxes_limits(K: int, pre_max: Optional[int], post_max: Optional[int]) -> Tuple[int, int, int]:
    """(pre_max, post_max, P) as the C-ABI wants them: ``None`` = K; P = min(K, pre_max, post_max) = columns of ``order``."""
    pre = K if pre_max is None else int(pre_max)
    post = K if post_max is None else int(post_max)
    if pre < 1 or post < 1:
        raise ValueError(f"pre_max={pre_max} and post_max={post_max} must be >= 1 (or None)")
    pre, post = min(pre, 2 ** 31 - 1), min(post, 2 ** 31 - 1)
    return pre, post, min(K, pre, post)


def nms_boxes_buffers(B: int, K: int, device, pre_max: Optional[int] = None, post_max: Optional[int] = None) -> tuple:
    """(keep [B,K], order [B,P], count [B], workspace) for ``nms_boxes(..., out=...)`` with the same limits."""
    pre, post, P = _nms_boxes_limits(K, pre_max, post_max)
    nbytes = lib().sad_nms_boxes_workspace_bytes(B, K, pre)
    if nbytes == 0:
        raise ValueError(f"nms_boxes: unsupported shape B={B}, K={K}, pre_max={pre_max} (min(K, pre_max) <= 16384, B <= 65535, B*K < 2^31)")
    return (torch.empty((B, K), dtype=torch.int32, device=device), torch.empty((B, P), dtype=torch.int32, device=device),
            torch.empty((B,), dtype=torch.int32, device=device), torch.empty((nbytes,), dtype=torch.uint8, device=device))


def nms_boxes(boxes: torch.Tensor, scores: Optional[torch.Tensor], labels: Optional[torch.Tensor], iou_thr: float,
              score_thr: float = 0.0, pre_max: Optional[int] = None, post_max: Optional[int] = None,
              out: Optional[tuple] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Box selection and rotated BEV NMS at scale (SPEC.md §23).  boxes [B,K,D] f32 (D >= 7: cx,cy,cz,l,w,h,yaw,...),
    scores [B,K] f32 (``None`` with D >= 8: column 7 of the rows), labels [B,K] int32 or ``None`` (class-agnostic) ->
    (keep [B,K] int32 0/1, order [B,P] int32 kept indices in rank order (-1 padded), count [B]), P = min(K, pre_max,
    post_max).  Candidates (score >= score_thr) are ranked by (score desc, index asc); the best ``pre_max`` are walked
    greedily with §13's IoU, suppressing within a class only, until ``post_max`` are kept.  min(K, pre_max) <= 16384.
    No synchronisation; ``out`` = buffers from ``nms_boxes_buffers`` with the same limits."""
    boxes = _boxes(boxes, "boxes")
    B, K, D = boxes.shape
    if scores is None:
        if D < 8:
            raise ValueError("scores=None needs box rows with a score column (D >= 8)")
        scores = _empty((B, K), dtype=torch.float32, device=boxes.device)
        copy_rows(boxes, 7, D, B * K, 1, scores)
    else:
        scores = _need(scores, "scores", torch.float32, 2)
    if tuple(scores.shape) != (B, K) or scores.device != boxes.device:
        raise ValueError("scores: expected [B,K] on the device of boxes")
    if labels is not None:
        labels = _need(labels, "labels", torch.int32, 2)
        if tuple(labels.shape) != (B, K) or labels.device != boxes.device:
            raise ValueError("labels: expected [B,K] on the device of boxes")
    pre, post, P = _nms_boxes_limits(K, pre_max, post_max)
    keep, order, count, ws = _nms_outputs(B, K, P, out, boxes.device)   # out: buffers from nms_boxes_buffers(B, K, device, pre_max, post_max)
    # 0 bytes = unsupported shape: the call below refuses it and says why, so a caller's workspace of any length passes here,
    # and a new buffer gets 16 bytes so that it has an address
    nbytes = lib().sad_nms_boxes_workspace_bytes(B, K, pre)
    ws = _workspace(nbytes if ws is not None else max(nbytes, 16), ws, boxes.device, "ops.nms_boxes_buffers")
    with _timed("nms_boxes", f"K{K}P{min(K, pre)}"):
        check(lib().sad_nms_boxes_f32(boxes.data_ptr(), D, scores.data_ptr(), _ptr(labels), B, K, _f32(iou_thr), _f32(score_thr), pre, post,
                                      keep.data_ptr(), order.data_ptr(), count.data_ptr(), ws.data_ptr(), _stream()),
              "sad_nms_boxes_f32")
    return keep, order, count


def _strict(t: torch.Tensor, name: str, dtype, shape, want: Optional[str] = None, how: str = "", dev=None) -> torch.Tensor:
    """The strict policy of the dense family: a tensor of ``dtype`` and ``shape`` (``None``: any extent; ``want`` says it in the
    caller's words), contiguous, read where it is (no copy is ever made).  Shapes and dtypes are judged before devices
    (``_head_devices``; for a target, ``dev``: the maps' device), so a wrong tensor is named whatever it lives on."""
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name}: expected a torch.Tensor")
    if t.dtype != dtype:
        raise TypeError(f"{name}: expected dtype {dtype}, got {t.dtype}")
    if t.dim() != len(shape) or any(w is not None and w != n for w, n in zip(shape, t.shape)):
        raise ValueError(f"{name}: expected {want or f'shape {tuple(shape)}'}, got {tuple(t.shape)}")
    if not t.is_contiguous():
        raise ValueError(f"{name}: must be contiguous{how}")
    if dev is not None and (not t.is_cuda or t.device != dev):
        raise RuntimeError(f"{name}: expected a tensor on {dev} (sad_amd has no CPU path)")
    return t


def _head_map(t: torch.Tensor, name: str, B: int, ch: int, H: int, W: int, layout: str) -> torch.Tensor:
    """A head map [B,ch,H,W] (nchw) / [B,H,W,ch] (nhwc): contiguous f32."""
    want = (B, ch, H, W) if layout == "nchw" else (B, H, W, ch)
    return _strict(t, name, torch.float32, want, f"shape {want} for layout {layout!r} ({ch} channels)",
                   f" in layout {layout!r} (the kernel reads the map where it is)")


def _head_devices(named) -> torch.device:
    """Every tensor of (name, tensor-or-None) pairs on the current GPU."""
    dev = None
    for name, t in named:
        if t is None:
            continue
        if not t.is_cuda:
            raise RuntimeError(f"{name}: expected a GPU tensor (sad_amd has no CPU path)")
        _on_current_device(t, name)
        dev = t.device
    return dev


def _head_index(index: Optional[torch.Tensor], B: int) -> int:
    """P of index [B,P] int32 (0 without one)."""
    if index is None:
        return 0
    want = f"[B,P] with B = {B} and P >= 1"
    _strict(index, "index", torch.int32, (B, None), want)
    if index.shape[1] < 1:      # (an empty tensor is contiguous: still judged before contiguity)
        raise ValueError(f"index: expected {want}, got {tuple(index.shape)}")
    return index.shape[1]


def _head_grid(first: torch.Tensor, name: str, layout: str) -> Tuple[int, int, int, int]:
    """(B, channels, H, W) of the first map of a head."""
    if layout not in _lib.LAYOUTS:
        raise ValueError(f"layout: expected 'nchw' or 'nhwc', got {layout!r}")
    if not isinstance(first, torch.Tensor):
        raise TypeError(f"{name}: expected a torch.Tensor")
    if first.dim() != 4:
        raise ValueError(f"{name}: expected 4 dims, got shape {tuple(first.shape)}")
    B, d1, d2, d3 = first.shape
    return (B, d1, d2, d3) if layout == "nchw" else (B, d3, d1, d2)


def _center_maps(hm: torch.Tensor, reg: torch.Tensor, height: torch.Tensor, dim: torch.Tensor, rot: torch.Tensor,
                 vel: Optional[torch.Tensor], B: int, C: int, H: int, W: int, layout: str) -> None:
    """The maps of a centre head against the grid (B, C, H, W) of hm, whose class count the caller has judged; ``vel`` may be
    ``None``."""
    _head_map(hm, "hm", B, C, H, W, layout)
    for t, name, ch in ((reg, "reg", 2), (height, "height", 1), (dim, "dim", 3), (rot, "rot", 2), (vel, "vel", 2)):
        if t is None and name == "vel":
            continue
        if isinstance(t, torch.Tensor) and t.dim() == 4 and _head_grid(t, name, layout)[1] != ch:
            raise ValueError(f"{name}: expected {ch} channels, got {_head_grid(t, name, layout)[1]}")
        _head_map(t, name, B, ch, H, W, layout)


def _anchor_arrays(sizes, z_center, rotations):
    """``sizes`` [ns,3], ``z_center`` [ns], ``rotations`` [nr] as float32 arrays (what the dense_head modules keep; not judged)."""
    return (np.asarray(sizes, dtype=np.float32).reshape(-1, 3), np.asarray(z_center, dtype=np.float32).reshape(-1),
            np.asarray(rotations, dtype=np.float32).reshape(-1))


def _anchor_scalars(sizes, z_center, rotations):
    """The anchor scalars of an operator call, judged -> (sizes, z_center, rotations as float32 arrays, ns, nr)."""
    sizes_np, zc, rots = _anchor_arrays(sizes, z_center, rotations)
    ns, nr = sizes_np.shape[0], rots.shape[0]
    if ns < 1 or nr < 1 or zc.shape[0] != ns:
        raise ValueError(f"sizes [ns,3], z_center [ns], rotations [nr]: need ns, nr >= 1 and one z_center per size (ns = {ns}, "
                         f"z_center: {zc.shape[0]}, nr = {nr})")
    if ns > 16 or nr > 8:
        raise ValueError(f"sizes / rotations: at most 16 sizes and 8 rotations (got {ns}, {nr})")
    return sizes_np, zc, rots, ns, nr


def _fill_anchors(a, sizes_np: np.ndarray, zc: np.ndarray, rots: np.ndarray, origin, step) -> None:
    """The anchor fields of an argument block: the scalars of ``_anchor_scalars`` and the grid (``dense_head.anchor_grid``)."""
    a.ns, a.nr = sizes_np.shape[0], rots.shape[0]
    a.sizes[:3 * a.ns] = sizes_np.reshape(-1).tolist()
    a.z_center[:a.ns] = zc.tolist()
    a.rotations[:a.nr] = rots.tolist()
    a.x0, a.y0, a.sx, a.sy = _f32(origin[0]), _f32(origin[1]), _f32(step[0]), _f32(step[1])


def anchor_decode(cls: torch.Tensor, reg: torch.Tensor, dir: Optional[torch.Tensor] = None, *, sizes, z_center, rotations,
                  origin, step, dir_offset: float = 0.78539, dir_limit_offset: float = 0.0, layout: str = "nchw",
                  index: Optional[torch.Tensor] = None, out: Optional[tuple] = None
                  ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Anchor head decode (SPEC.md §25.1).  cls [B,A*C,H,W], reg [B,A*7,H,W], dir [B,A*nb,H,W] or ``None`` (``layout="nhwc"``:
    channels last), contiguous f32, read where they are.  A = ns * nr anchors per cell from ``sizes`` [ns,3] (l,w,h),
    ``z_center`` [ns], ``rotations`` [nr] (sizes outer, rotations inner); the anchor of cell (y, x) stands at
    ``origin + (x, y) * step`` (``dense_head.anchor_grid``).  -> (boxes [B,K,7], scores [B,K], labels [B,K] int32), K = H*W*A,
    k = (y*W + x)*A + a: ResidualCoder.decode, the direction bin applied when ``dir`` is given, score = sigmoid(max class
    logit).  ``index`` [B,P] int32: only those rows, outputs [B,P,...]; an entry outside [0, K) gives (0..., -inf, -1).
    One launch, no synchronisation, no gradients.  ``out`` = (boxes, scores, labels) to write into."""
    sizes_np, zc, rots, ns, nr = _anchor_scalars(sizes, z_center, rotations)
    A = ns * nr
    B, chc, H, W = _head_grid(cls, "cls", layout)
    if chc < A or chc % A:
        raise ValueError(f"cls: {chc} channels are not a multiple of A = ns * nr = {A}")
    C = chc // A
    cls = _head_map(cls, "cls", B, A * C, H, W, layout)
    _, chr_, _, _ = _head_grid(reg, "reg", layout)
    if chr_ != A * 7:
        raise ValueError(f"reg: expected A * 7 = {A * 7} channels, got {chr_}")
    reg = _head_map(reg, "reg", B, A * 7, H, W, layout)
    nb = 0
    if dir is not None:
        _, chd, _, _ = _head_grid(dir, "dir", layout)
        if chd < 2 * A or chd % A:
            raise ValueError(f"dir: {chd} channels are not A * nb with nb >= 2 (A = {A})")
        nb = chd // A
        dir = _head_map(dir, "dir", B, chd, H, W, layout)
    K = H * W * A
    P = _head_index(index, B)
    dev = _head_devices((("cls", cls), ("reg", reg), ("dir", dir), ("index", index)))
    rows = P if index is not None else K
    boxes, scores, labels = _outputs((("boxes", (B, rows, 7), torch.float32), ("scores", (B, rows), torch.float32),
                                      ("labels", (B, rows), torch.int32)), out, dev, "the maps")
    a = _lib.AnchorDecodeArgs()
    a.struct_size = ctypes.sizeof(_lib.AnchorDecodeArgs)
    a.cls, a.reg, a.dir, a.index = cls.data_ptr(), reg.data_ptr(), _ptr(dir), _ptr(index)
    a.B, a.H, a.W, a.C, a.nb, a.layout, a.P = B, H, W, C, nb, _lib.LAYOUTS[layout], P
    _fill_anchors(a, sizes_np, zc, rots, origin, step)
    a.dir_offset, a.dir_limit_offset = _f32(dir_offset), _f32(dir_limit_offset)
    a.boxes, a.scores, a.labels = boxes.data_ptr(), scores.data_ptr(), labels.data_ptr()
    with _timed("anchor_decode", f"K{K}R{rows}"):
        check(lib().sad_anchor_decode_f32(ctypes.byref(a), _stream()), "sad_anchor_decode_f32")
    return boxes, scores, labels


def center_decode(hm: torch.Tensor, reg: torch.Tensor, height: torch.Tensor, dim: torch.Tensor, rot: torch.Tensor,
                  vel: Optional[torch.Tensor] = None, *, origin, cell, log_dim: bool = True, peak: bool = False,
                  layout: str = "nchw", index: Optional[torch.Tensor] = None, out: Optional[tuple] = None
                  ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Centre head decode (SPEC.md §25.2, one CenterPoint task).  hm [B,C,H,W], reg [B,2,H,W], height [B,1,H,W], dim [B,3,H,W],
    rot [B,2,H,W] (sine, cosine), vel [B,2,H,W] or ``None`` (``layout="nhwc"``: channels last), contiguous f32 ->
    (boxes [B,K,D], scores [B,K], labels [B,K] int32), K = H*W, k = y*W + x, D = 9 with ``vel`` else 7:
    cx = (x + reg0) * cell[0] + origin[0], cy likewise, cz = height, (l,w,h) = exp(dim) if ``log_dim`` else dim,
    yaw = atan2(rot0, rot1), score = sigmoid(max class logit).  ``peak``: only the classes that are a 3x3 local maximum at the
    cell take part; a cell without one gets score 0 and label -1.  ``index`` / ``out`` as in ``anchor_decode``."""
    B, C, H, W = _head_grid(hm, "hm", layout)
    if C < 1:
        raise ValueError("hm: needs at least one class channel")
    _center_maps(hm, reg, height, dim, rot, vel, B, C, H, W, layout)
    D = 9 if vel is not None else 7
    K = H * W
    P = _head_index(index, B)
    dev = _head_devices((("hm", hm), ("reg", reg), ("height", height), ("dim", dim), ("rot", rot), ("vel", vel), ("index", index)))
    rows = P if index is not None else K
    boxes, scores, labels = _outputs((("boxes", (B, rows, D), torch.float32), ("scores", (B, rows), torch.float32),
                                      ("labels", (B, rows), torch.int32)), out, dev, "the maps")
    a = _lib.CenterDecodeArgs()
    a.struct_size = ctypes.sizeof(_lib.CenterDecodeArgs)
    a.hm, a.reg, a.height, a.dim, a.rot = hm.data_ptr(), reg.data_ptr(), height.data_ptr(), dim.data_ptr(), rot.data_ptr()
    a.vel, a.index = _ptr(vel), _ptr(index)
    a.B, a.H, a.W, a.C, a.layout, a.P, a.log_dim, a.peak = B, H, W, C, _lib.LAYOUTS[layout], P, int(bool(log_dim)), int(bool(peak))
    a.lo_x, a.lo_y, a.sx, a.sy = _f32(origin[0]), _f32(origin[1]), _f32(cell[0]), _f32(cell[1])
    a.boxes, a.scores, a.labels = boxes.data_ptr(), scores.data_ptr(), labels.data_ptr()
    with _timed("center_decode", f"K{K}R{rows}"):
        check(lib().sad_center_decode_f32(ctypes.byref(a), _stream()), "sad_center_decode_f32")
    return boxes, scores, labels


def _gt_shapes(gt_boxes: torch.Tensor, gt_labels: torch.Tensor, min_d: int = 7) -> Tuple[int, int, int]:
    """(B, G, D) of gt_boxes [B,G,D] f32 / gt_labels [B,G] int32, both contiguous; judged before any device."""
    for t, name, dt in ((gt_boxes, "gt_boxes", torch.float32), (gt_labels, "gt_labels", torch.int32)):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name}: expected a torch.Tensor")
        if t.dtype != dt:
            raise TypeError(f"{name}: expected dtype {dt}, got {t.dtype}")
    if gt_boxes.dim() != 3 or gt_boxes.shape[0] < 1 or gt_boxes.shape[2] < min_d:
        raise ValueError(f"gt_boxes: expected [B,G,D] with B >= 1 and D >= {min_d}, got {tuple(gt_boxes.shape)}")
    B, G, D = gt_boxes.shape
    if tuple(gt_labels.shape) != (B, G):
        raise ValueError(f"gt_labels: expected shape {(B, G)}, got {tuple(gt_labels.shape)}")
    if G > 1024:
        raise ValueError(f"gt_boxes: at most 1024 boxes per scene (got G = {G})")
    if not gt_boxes.is_contiguous() or not gt_labels.is_contiguous():
        raise ValueError("gt_boxes / gt_labels: must be contiguous")
    return B, G, D


def _gt_inputs(gt_boxes: torch.Tensor, gt_labels: torch.Tensor, min_d: int = 7) -> Tuple[int, int, int, torch.device]:
    """(B, G, D, device) of gt_boxes [B,G,D] f32 / gt_labels [B,G] int32, both contiguous on the current GPU."""
    B, G, D = _gt_shapes(gt_boxes, gt_labels, min_d)
    return B, G, D, _head_devices((("gt_boxes", gt_boxes), ("gt_labels", gt_labels)))


def _per_size(v, ns: int, name: str, dtype) -> np.ndarray:
    a = np.asarray(v, dtype=dtype).reshape(-1)
    if a.shape[0] == 1 and ns > 1:
        a = np.repeat(a, ns)
    if a.shape[0] != ns:
        raise ValueError(f"{name}: expected one value per anchor size (ns = {ns}), got {a.shape[0]}")
    return a


def anchor_targets_workspace(B: int, G: int, device) -> Optional[torch.Tensor]:
    """The workspace of ``anchor_targets(..., workspace=...)`` for a caller that keeps it (``None`` when G = 0)."""
    nbytes = lib().sad_anchor_targets_workspace_bytes(B, G)
    return torch.empty(nbytes, dtype=torch.uint8, device=device) if nbytes else None


def anchor_targets(gt_boxes: torch.Tensor, gt_labels: torch.Tensor, *, H: int, W: int, sizes, z_center, rotations, origin, step,
                   pos_thr, neg_thr, size_class=None, nb: int = 0, dir_offset: float = 0.78539, out: Optional[tuple] = None,
                   workspace: Optional[torch.Tensor] = None) -> tuple:
    """Anchor head target assignment (SPEC.md §26.1), the inverse of ``anchor_decode`` on the same anchor scalars.
    gt_boxes [B,G,D>=7] f32 rows (cx,cy,cz,l,w,h,yaw,...), gt_labels [B,G] int32 (negative: padding row), G <= 1024 ->
    (labels [B,K] int32, match [B,K] int32, reg_target [B,K,7], max_iou [B,K][, dir_target [B,K] int32 when nb >= 2]),
    K = H*W*A, k = (y*W + x)*A + a.  The max-IoU assigner of SECOND / PointPillars on the nearest-BEV IoU: anchor k of size s
    is positive when its best IoU over the boxes of class ``size_class[s]`` (``None``: of any class) reaches ``pos_thr[s]``, or
    when it attains some box's best IoU over the scene; background (-1) below ``neg_thr[s]``, else ignored (-2).  A positive
    gets the class, the index and the residual encoding of its own best box.  Two launches and a memset, no anchor tensor, no
    IoU matrix, no synchronisation, no gradients, bit-identical from call to call.  ``out``: the tuple to write into."""
    sizes_np, zc, rots, ns, nr = _anchor_scalars(sizes, z_center, rotations)
    if not (sizes_np > 0).all():
        raise ValueError("sizes: every anchor extent must be > 0")
    if H < 1 or W < 1:
        raise ValueError(f"H, W: need >= 1 (got {H}, {W})")
    if nb != 0 and not 2 <= nb <= 8:
        raise ValueError(f"nb: 0 (no direction target) or 2 .. 8 (got {nb})")
    pos, neg = _per_size(pos_thr, ns, "pos_thr", np.float32), _per_size(neg_thr, ns, "neg_thr", np.float32)
    sc = None if size_class is None else _per_size(size_class, ns, "size_class", np.int32)
    B, G, D, dev = _gt_inputs(gt_boxes, gt_labels)
    A = ns * nr
    K = H * W * A
    spec = [("labels", (B, K), torch.int32), ("match", (B, K), torch.int32), ("reg_target", (B, K, 7), torch.float32),
            ("max_iou", (B, K), torch.float32)]
    if nb:
        spec.append(("dir_target", (B, K), torch.int32))
    outs = _outputs(spec, out, dev, "gt_boxes")
    nbytes = lib().sad_anchor_targets_workspace_bytes(B, G)     # (0 with G = 0: nothing is matched, no workspace is read)
    workspace = _workspace(nbytes, workspace, dev, "ops.anchor_targets_workspace") if nbytes else None
    a = _lib.AnchorTargetsArgs()
    a.struct_size = ctypes.sizeof(_lib.AnchorTargetsArgs)
    a.gt_boxes, a.gt_labels = (gt_boxes.data_ptr(), gt_labels.data_ptr()) if G else (None, None)
    a.B, a.G, a.D, a.H, a.W, a.nb, a.use_size_class = B, G, D, H, W, nb, int(sc is not None)
    _fill_anchors(a, sizes_np, zc, rots, origin, step)
    a.pos_thr[:ns] = pos.tolist()
    a.neg_thr[:ns] = neg.tolist()
    if sc is not None:
        a.size_class[:ns] = sc.tolist()
    a.dir_offset = _f32(dir_offset)
    a.labels, a.match, a.reg_target, a.max_iou = (t.data_ptr() for t in outs[:4])
    a.dir_target = outs[4].data_ptr() if nb else None
    a.workspace = _ptr(workspace)
    with _timed("anchor_targets", f"K{K}G{G}"):
        check(lib().sad_anchor_targets_f32(ctypes.byref(a), _stream()), "sad_anchor_targets_f32")
    return outs


def center_targets(gt_boxes: torch.Tensor, gt_labels: torch.Tensor, *, C: int, H: int, W: int, origin, cell,
                   min_overlap: float = 0.1, min_radius: int = 2, vel: bool = False, layout: str = "nchw",
                   out: Optional[tuple] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Centre head target assignment (SPEC.md §26.2, one CenterPoint task), the inverse of ``center_decode``.
    gt_boxes [B,G,D>=7] f32, gt_labels [B,G] int32 (outside [0, C): padding), G <= 1024 -> (heatmap [B,C,H,W] f32 (``nhwc``:
    [B,H,W,C]), ind [B,G] int32, anno [B,G,8 | 10] f32).  A box whose centre falls into cell (iy, ix) of the map draws
    CenterNet's Gaussian of radius max(min_radius, int(gaussian_radius((w, l) in cells, min_overlap))) into the plane of its
    class (maximum where boxes overlap, centre cell exactly 1); ind = iy*W + ix, anno = (dx, dy, z, log l, log w, log h,
    sin yaw, cos yaw[, vx, vy]).  A box whose centre lies outside the map, whose l or w is <= 0 or whose label is padding is
    unassigned: ind -1, anno 0, nothing drawn.  Two launches, every element stored once, no synchronisation, no gradients."""
    if layout not in _lib.LAYOUTS:
        raise ValueError(f"layout: expected 'nchw' or 'nhwc', got {layout!r}")
    if C < 1 or C > 64 or H < 1 or W < 1:
        raise ValueError(f"C, H, W: need 1 <= C <= 64 and H, W >= 1 (got {C}, {H}, {W})")
    if not 0.0 < float(min_overlap) < 1.0:
        raise ValueError(f"min_overlap: expected a value in (0, 1), got {min_overlap}")
    if not 0 <= int(min_radius) <= 64:
        raise ValueError(f"min_radius: expected 0 .. 64, got {min_radius}")
    if not (float(cell[0]) > 0 and float(cell[1]) > 0):
        raise ValueError(f"cell: must be positive, got {tuple(cell)}")
    B, G, D, dev = _gt_inputs(gt_boxes, gt_labels, 9 if vel else 7)
    na = 10 if vel else 8
    spec = (("heatmap", (B, C, H, W) if layout == "nchw" else (B, H, W, C), torch.float32), ("ind", (B, G), torch.int32),
            ("anno", (B, G, na), torch.float32))
    heatmap, ind, anno = _outputs(spec, out, dev, "gt_boxes")
    a = _lib.CenterTargetsArgs()
    a.struct_size = ctypes.sizeof(_lib.CenterTargetsArgs)
    a.gt_boxes, a.gt_labels = (gt_boxes.data_ptr(), gt_labels.data_ptr()) if G else (None, None)
    a.B, a.G, a.D, a.C, a.H, a.W, a.layout, a.min_radius, a.vel = B, G, D, C, H, W, _lib.LAYOUTS[layout], int(min_radius), int(bool(vel))
    a.lo_x, a.lo_y, a.sx, a.sy = _f32(origin[0]), _f32(origin[1]), _f32(cell[0]), _f32(cell[1])
    a.min_overlap = _f32(min_overlap)
    a.heatmap = heatmap.data_ptr()
    a.ind, a.anno = (ind.data_ptr(), anno.data_ptr()) if G else (None, None)
    with _timed("center_targets", f"K{H * W}G{G}"):
        check(lib().sad_center_targets_f32(ctypes.byref(a), _stream()), "sad_center_targets_f32")
    return heatmap, ind, anno


ROI_OUTPUTS = ("index", "match", "labels", "iou", "cls_target", "reg_valid", "rois_s", "gt_local", "reg_target")


def roi_output_spec(B: int, S: int) -> tuple:
    """((name, shape, dtype), ...) of ``roi_targets``' outputs, what its ``out=`` tuple is checked against."""
    i32, f32 = torch.int32, torch.float32
    return (("index", (B, S), i32), ("match", (B, S), i32), ("labels", (B, S), i32), ("iou", (B, S), f32), ("cls_target", (B, S), f32),
            ("reg_valid", (B, S), i32), ("rois_s", (B, S, 7), f32), ("gt_local", (B, S, 7), f32), ("reg_target", (B, S, 7), f32))


def roi_targets_workspace(B: int, R: int, device) -> torch.Tensor:
    """The workspace of ``roi_targets(..., workspace=...)`` for a caller that keeps it."""
    nbytes = lib().sad_roi_targets_workspace_bytes(B, R)
    if not nbytes:
        raise ValueError(f"roi_targets_workspace: need 1 <= B <= 65535 and 1 <= R <= 4096 (got {B}, {R})")
    return torch.empty(nbytes, dtype=torch.uint8, device=device)


def roi_targets(rois: torch.Tensor, roi_count: Optional[torch.Tensor], roi_labels: Optional[torch.Tensor], gt_boxes: torch.Tensor,
                gt_labels: torch.Tensor, *, S: int, fg_max: int, fg_thr: float, bg_lo: float, hard_ratio: float, reg_fg_thr: float,
                cls_fg_thr: float, cls_bg_thr: float, cls_mode: str = "roi_iou", seed: int = 0, out: Optional[tuple] = None,
                workspace: Optional[torch.Tensor] = None) -> tuple:
    """RoI head proposal sampling and targets (SPEC.md §28.1).  rois [B,R,D>=7] f32 rows (cx,cy,cz,l,w,h,yaw,...), roi_count [B]
    int32 or ``None`` (the candidates of scene b are its first ``roi_count[b]`` rows; the rows beyond are never read, so the
    gathered output of ``nms_boxes`` goes in as it is), roi_labels [B,R] int32 or ``None`` (given: a RoI is matched against the
    boxes of its own class only), gt_boxes [B,G,Dg>=7] / gt_labels [B,G] int32 as in ``anchor_targets`` ->
    (index [B,S] int32, match, labels, iou [B,S] f32, cls_target [B,S] f32, reg_valid [B,S] int32, rois_s [B,S,7], gt_local
    [B,S,7], reg_target [B,S,7]).  A candidate's best 3-D IoU m makes it fg (m >= fg_thr), hard (bg_lo <= m < fg_thr) or easy;
    the first min(fg_max, n_fg, S) slots hold fg candidates without replacement, the others draw from hard (``hard_ratio`` of
    them) and easy with replacement, all from an integer hash of (seed, scene, row or slot).  ``index`` gathers whatever was
    pooled per RoI.  Two launches, no IoU matrix, no synchronisation, no gradients, bit-identical from call to call."""
    if cls_mode not in _lib.ROI_CLS_MODES:
        raise ValueError(f"cls_mode: expected 'roi_iou' or 'cls', got {cls_mode!r}")
    _strict(rois, "rois", torch.float32, (None, None, None), "[B,R,D] with B, R >= 1 and D >= 7")
    B, R, D = rois.shape
    if B < 1 or R < 1 or D < 7:
        raise ValueError(f"rois: expected [B,R,D] with B, R >= 1 and D >= 7, got {tuple(rois.shape)}")
    if R > 4096:
        raise ValueError(f"rois: at most 4096 RoIs per scene (got R = {R})")
    if roi_count is not None:
        _strict(roi_count, "roi_count", torch.int32, (B,))
    if roi_labels is not None:
        _strict(roi_labels, "roi_labels", torch.int32, (B, R))
    S, fg_max = int(S), int(fg_max)
    if not 1 <= S <= 1024:
        raise ValueError(f"S: expected 1 .. 1024, got {S}")
    if fg_max < 0:
        raise ValueError(f"fg_max: expected >= 0, got {fg_max}")
    fg_thr, bg_lo, hard_ratio, reg_fg_thr = _f32(fg_thr), _f32(bg_lo), _f32(hard_ratio), _f32(reg_fg_thr)
    cls_fg_thr, cls_bg_thr = _f32(cls_fg_thr), _f32(cls_bg_thr)
    if not (0.0 <= bg_lo <= fg_thr and fg_thr > 0.0):
        raise ValueError(f"fg_thr, bg_lo: need 0 <= bg_lo <= fg_thr and fg_thr > 0 (got {fg_thr}, {bg_lo})")
    if not cls_bg_thr < cls_fg_thr:
        raise ValueError(f"cls_fg_thr, cls_bg_thr: need cls_bg_thr < cls_fg_thr (got {cls_fg_thr}, {cls_bg_thr})")
    if not 0.0 <= hard_ratio <= 1.0:
        raise ValueError(f"hard_ratio: expected a value in [0, 1], got {hard_ratio}")
    if reg_fg_thr != reg_fg_thr:
        raise ValueError("reg_fg_thr: NaN")
    if isinstance(gt_boxes, torch.Tensor) and gt_boxes.dim() == 3 and gt_boxes.shape[0] != B:
        raise ValueError(f"gt_boxes: expected {B} scenes like rois, got {gt_boxes.shape[0]}")
    _, G, Dg, _ = _gt_inputs(gt_boxes, gt_labels)
    dev = _head_devices((("rois", rois), ("roi_count", roi_count), ("roi_labels", roi_labels), ("gt_boxes", gt_boxes)))
    outs = _outputs(roi_output_spec(B, S), out, dev, "rois")
    workspace = _workspace(lib().sad_roi_targets_workspace_bytes(B, R), workspace, dev, "ops.roi_targets_workspace", 4)
    a = _lib.RoiTargetsArgs()
    a.struct_size = ctypes.sizeof(_lib.RoiTargetsArgs)
    a.rois, a.roi_count, a.roi_labels = rois.data_ptr(), _ptr(roi_count), _ptr(roi_labels)
    a.gt_boxes, a.gt_labels = (gt_boxes.data_ptr(), gt_labels.data_ptr()) if G else (None, None)
    a.B, a.R, a.D, a.G, a.Dg, a.S, a.fg_max, a.cls_mode = B, R, D, G, Dg, S, fg_max, _lib.ROI_CLS_MODES[cls_mode]
    a.seed = int(seed) & 0xFFFFFFFF
    a.fg_thr, a.bg_lo, a.hard_ratio, a.reg_fg_thr, a.cls_fg_thr, a.cls_bg_thr = fg_thr, bg_lo, hard_ratio, reg_fg_thr, cls_fg_thr, cls_bg_thr
    for n, t in zip(ROI_OUTPUTS, outs):
        setattr(a, n, t.data_ptr())
    a.workspace = workspace.data_ptr()
    with _timed("roi_targets", f"R{R}G{G}S{S}"):
        check(lib().sad_roi_targets_f32(ctypes.byref(a), _stream()), "sad_roi_targets_f32")
    return outs


def roi_decode(rois: torch.Tensor, reg: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The inverse of ``roi_targets``' residual code (SPEC.md §28.2), what a RoI head runs at inference: rois [B,S,D>=7] f32,
    reg [B,S,7] f32 -> boxes [B,S,7]: the residuals scaled by the RoI's diagonal and height, rotated out of the RoI's frame and
    moved to its centre, exp of the size residuals times the RoI's extents, yaw = reg6 + the RoI's.  One launch."""
    _strict(rois, "rois", torch.float32, (None, None, None), "[B,S,D] with B, S >= 1 and D >= 7")
    B, S, D = rois.shape
    if B < 1 or S < 1 or D < 7:
        raise ValueError(f"rois: expected [B,S,D] with B, S >= 1 and D >= 7, got {tuple(rois.shape)}")
    _strict(reg, "reg", torch.float32, (B, S, 7))
    dev = _head_devices((("rois", rois), ("reg", reg)))
    boxes, = _outputs((("boxes", (B, S, 7), torch.float32),), None if out is None else (out,), dev, "rois")
    with _timed("roi_decode", f"R{B * S}"):
        check(lib().sad_roi_decode_f32(rois.data_ptr(), D, reg.data_ptr(), B, S, boxes.data_ptr(), _stream()), "sad_roi_decode_f32")
    return boxes


def _weights(v, n: int, name: str) -> list:
    a = np.ones(n, np.float32) if v is None else np.asarray(v, dtype=np.float32).reshape(-1)
    if a.shape[0] != n:
        raise ValueError(f"{name}: expected {n} values, got {a.shape[0]}")
    return a.tolist()


def anchor_head_loss_workspace(B: int, H: int, W: int, A: int, device) -> torch.Tensor:
    """The workspace of ``anchor_head_loss(..., workspace=...)`` for a caller that keeps it."""
    nbytes = lib().sad_anchor_head_loss_workspace_bytes(B, H, W, A)
    if not nbytes:
        raise ValueError(f"anchor_head_loss_workspace: unsupported shape B = {B}, H = {H}, W = {W}, A = {A}")
    return torch.empty(nbytes, dtype=torch.uint8, device=device)


def anchor_head_loss(cls: torch.Tensor, reg: torch.Tensor, dir: Optional[torch.Tensor], labels: torch.Tensor,
                     reg_target: torch.Tensor, dir_target: Optional[torch.Tensor] = None, *, alpha: float = 0.25,
                     beta: float = 1.0 / 9.0, code_weights=None, sin_diff: bool = True, scale=(1.0, 1.0, 1.0), normalize: bool = True,
                     layout: str = "nchw", per_anchor: bool = False, out: Optional[tuple] = None,
                     workspace: Optional[torch.Tensor] = None) -> tuple:
    """Anchor head losses with their gradients (SPEC.md §27.1).  cls [B,A*C,H,W], reg [B,A*7,H,W], dir [B,A*nb,H,W] or ``None``
    (``layout="nhwc"``: channels last), contiguous f32; labels [B,K] int32 (>= 0 class, -1 background, -2 ignored), reg_target
    [B,K,7] f32 and dir_target [B,K] int32 as ``anchor_targets`` makes them, K = H*W*A ->
    (loss [B,3] = (cls, reg, dir), num_pos [B] int32, grad_cls, grad_reg[, grad_dir][, per_anchor [B,K,3]]): OpenPCDet's sigmoid
    focal loss (gamma = 2) over the rows that are not ignored, smooth-L1 with the sine-difference yaw and softmax cross-entropy
    of the direction bins over the positives, each scaled by ``scale[i] / max(num_pos[b], 1)`` per scene (``normalize=False``:
    by ``scale[i]``); the gradients are those of ``loss[b, i]`` summed over i, in the shape and layout of the maps.  Two small
    launches around one pass over the maps, no synchronisation, bit-identical from call to call.  ``out``: the tuple to write into."""
    B, chc, H, W = _head_grid(cls, "cls", layout)
    _, chr_, _, _ = _head_grid(reg, "reg", layout)
    if chr_ < 7 or chr_ % 7:
        raise ValueError(f"reg: {chr_} channels are not A * 7")
    A = chr_ // 7
    if A > 128:
        raise ValueError(f"reg: at most 128 anchors per cell (got A = {A})")
    if chc < A or chc % A:
        raise ValueError(f"cls: {chc} channels are not a multiple of A = {A}")
    C = chc // A
    if C > 64:
        raise ValueError(f"cls: at most 64 classes (got C = {C})")
    cls = _head_map(cls, "cls", B, A * C, H, W, layout)
    reg = _head_map(reg, "reg", B, A * 7, H, W, layout)
    nb = 0
    if dir is not None:
        _, chd, _, _ = _head_grid(dir, "dir", layout)
        if chd < 2 * A or chd % A or chd // A > 8:
            raise ValueError(f"dir: {chd} channels are not A * nb with 2 <= nb <= 8 (A = {A})")
        nb = chd // A
        dir = _head_map(dir, "dir", B, chd, H, W, layout)
    if (dir is None) != (dir_target is None):
        raise ValueError("dir and dir_target must be given together")
    if not float(beta) > 0.0:
        raise ValueError(f"beta: must be > 0, got {beta}")
    if not 0.0 <= float(alpha) <= 1.0:
        raise ValueError(f"alpha: expected a value in [0, 1], got {alpha}")
    cw, sc = _weights(code_weights, 7, "code_weights"), _weights(scale, 3, "scale")
    K = H * W * A
    dev = _head_devices((("cls", cls), ("reg", reg), ("dir", dir)))
    for name, t, shape, dt in ([("labels", labels, (B, K), torch.int32), ("reg_target", reg_target, (B, K, 7), torch.float32)]
                               + ([("dir_target", dir_target, (B, K), torch.int32)] if nb else [])):
        _strict(t, name, dt, shape, dev=dev)
    spec = [("loss", (B, 3), torch.float32), ("num_pos", (B,), torch.int32), ("grad_cls", tuple(cls.shape), torch.float32),
            ("grad_reg", tuple(reg.shape), torch.float32)]
    if nb:
        spec.append(("grad_dir", tuple(dir.shape), torch.float32))
    if per_anchor:
        spec.append(("per_anchor", (B, K, 3), torch.float32))
    outs = _outputs(spec, out, dev, "the maps")
    nbytes = lib().sad_anchor_head_loss_workspace_bytes(B, H, W, A)
    if not nbytes:
        raise ValueError(f"anchor_head_loss: unsupported shape (B = {B}, K = {K}: B <= 65535 and B * K < 2^31)")
    workspace = _workspace(nbytes, workspace, dev, "ops.anchor_head_loss_workspace")
    a = _lib.AnchorHeadLossArgs()
    a.struct_size = ctypes.sizeof(_lib.AnchorHeadLossArgs)
    a.cls, a.reg, a.dir = cls.data_ptr(), reg.data_ptr(), _ptr(dir)
    a.labels, a.reg_target, a.dir_target = labels.data_ptr(), reg_target.data_ptr(), _ptr(dir_target)
    a.B, a.H, a.W, a.A, a.C, a.nb, a.layout = B, H, W, A, C, nb, _lib.LAYOUTS[layout]
    a.sin_diff, a.normalize = int(bool(sin_diff)), int(bool(normalize))
    a.alpha, a.beta = _f32(alpha), _f32(beta)
    a.code_weights[:], a.scale[:] = cw, sc
    a.loss, a.num_pos, a.grad_cls, a.grad_reg = (t.data_ptr() for t in outs[:4])
    a.grad_dir = outs[4].data_ptr() if nb else None
    a.per_anchor = outs[-1].data_ptr() if per_anchor else None
    a.workspace = workspace.data_ptr()
    with _timed("anchor_head_loss", f"K{K}C{C}"):
        check(lib().sad_anchor_head_loss_f32(ctypes.byref(a), _stream()), "sad_anchor_head_loss_f32")
    return outs


def center_head_loss_workspace(B: int, H: int, W: int, G: int, device) -> torch.Tensor:
    """The workspace of ``center_head_loss(..., workspace=...)`` for a caller that keeps it."""
    nbytes = lib().sad_center_head_loss_workspace_bytes(B, H, W, G)
    if not nbytes:
        raise ValueError(f"center_head_loss_workspace: unsupported shape B = {B}, H = {H}, W = {W}, G = {G}")
    return torch.empty(nbytes, dtype=torch.uint8, device=device)


def center_head_loss(hm: torch.Tensor, reg: torch.Tensor, height: torch.Tensor, dim: torch.Tensor, rot: torch.Tensor,
                     vel: Optional[torch.Tensor], heatmap: torch.Tensor, ind: torch.Tensor, anno: torch.Tensor, *, code_weights=None,
                     scale=(1.0, 1.0), normalize: bool = True, layout: str = "nchw", out: Optional[tuple] = None,
                     workspace: Optional[torch.Tensor] = None) -> tuple:
    """Centre head losses with their gradients (SPEC.md §27.2, one CenterPoint task).  The maps of ``center_decode`` and the
    (heatmap, ind, anno) of ``center_targets`` (heatmap in the maps' layout) ->
    (loss [B,2] = (hm, reg), num_pos [B,2] int32 = (cells with heatmap == 1, assigned boxes), grad_hm, grad_reg, grad_height,
    grad_dim, grad_rot[, grad_vel]): CenterNet's penalty-reduced focal loss of the clamped sigmoid over every cell and class,
    and L1 of the regression channels at the boxes' cells against anno, weighted by ``code_weights`` (one per anno column);
    component i of scene b is scaled by ``scale[i] / max(num_pos[b, i], 1)`` (``normalize=False``: by ``scale[i]``).  Boxes
    that share a cell add their gradients in ascending g.  No synchronisation, bit-identical from call to call."""
    B, C, H, W = _head_grid(hm, "hm", layout)
    if C < 1 or C > 64:
        raise ValueError(f"hm: expected 1 .. 64 class channels, got {C}")
    _center_maps(hm, reg, height, dim, rot, vel, B, C, H, W, layout)
    na = 10 if vel is not None else 8
    dev = _head_devices((("hm", hm), ("reg", reg), ("height", height), ("dim", dim), ("rot", rot), ("vel", vel)))
    if not isinstance(ind, torch.Tensor) or ind.dim() != 2 or ind.shape[0] != B:
        raise ValueError(f"ind: expected [B,G] with B = {B}")
    G = ind.shape[1]
    if G > 1024:
        raise ValueError(f"ind: at most 1024 boxes per scene (got G = {G})")
    for name, t, shape, dt in (("heatmap", heatmap, tuple(hm.shape), torch.float32), ("ind", ind, (B, G), torch.int32),
                               ("anno", anno, (B, G, na), torch.float32)):
        _strict(t, name, dt, shape, dev=dev)
    cw, sc = _weights(code_weights, na, "code_weights"), _weights(scale, 2, "scale")
    spec = [("loss", (B, 2), torch.float32), ("num_pos", (B, 2), torch.int32), ("grad_hm", tuple(hm.shape), torch.float32)]
    spec += [(f"grad_{n}", tuple(t.shape), torch.float32) for n, t in (("reg", reg), ("height", height), ("dim", dim), ("rot", rot), ("vel", vel))
             if t is not None]
    outs = _outputs(spec, out, dev, "the maps")
    nbytes = lib().sad_center_head_loss_workspace_bytes(B, H, W, G)
    if not nbytes:
        raise ValueError(f"center_head_loss: unsupported shape (B = {B}, H * W = {H * W}: B <= 65535 and B * H * W < 2^31)")
    workspace = _workspace(nbytes, workspace, dev, "ops.center_head_loss_workspace")
    a = _lib.CenterHeadLossArgs()
    a.struct_size = ctypes.sizeof(_lib.CenterHeadLossArgs)
    a.hm, a.reg, a.height, a.dim, a.rot = hm.data_ptr(), reg.data_ptr(), height.data_ptr(), dim.data_ptr(), rot.data_ptr()
    a.vel = _ptr(vel)
    a.heatmap = heatmap.data_ptr()
    a.ind, a.anno = (ind.data_ptr(), anno.data_ptr()) if G else (None, None)
    a.B, a.H, a.W, a.C, a.G, a.layout, a.normalize = B, H, W, C, G, _lib.LAYOUTS[layout], int(bool(normalize))
    a.code_weights[:na], a.scale[:] = cw, sc
    a.loss, a.num_pos, a.grad_hm, a.grad_reg, a.grad_height, a.grad_dim, a.grad_rot = (t.data_ptr() for t in outs[:7])
    a.grad_vel = outs[7].data_ptr() if vel is not None else None
    a.workspace = workspace.data_ptr()
    with _timed("center_head_loss", f"K{H * W}G{G}"):
        check(lib().sad_center_head_loss_f32(ctypes.byref(a), _stream()), "sad_center_head_loss_f32")
    return outs


def roi_loss_output_spec(B: int, S: int, corner: bool, per_roi: bool) -> tuple:
    """((name, shape, dtype), ...) of ``roi_head_loss``' outputs, what its ``out=`` tuple is checked against."""
    f32 = torch.float32
    spec = [("loss", (B, 3), f32), ("num", (B, 2), torch.int32), ("grad_cls", (B, S), f32), ("grad_reg", (B, S, 7), f32)]
    if corner:
        spec.append(("grad_corner", (B, S, 7), f32))
    if per_roi:
        spec.append(("per_roi", (B, S, 3), f32))
    return tuple(spec)


def roi_head_loss(rcnn_cls: torch.Tensor, rcnn_reg: torch.Tensor, cls_target: torch.Tensor, reg_valid: torch.Tensor,
                  reg_target: torch.Tensor, rois: Optional[torch.Tensor] = None, gt_local: Optional[torch.Tensor] = None, *,
                  beta: float = 1.0 / 9.0, code_weights=None, scale=(1.0, 1.0, 1.0), normalize: bool = True, per_roi: bool = False,
                  out: Optional[tuple] = None) -> tuple:
    """RoI head losses with their gradients (SPEC.md §29).  rcnn_cls [B,S] f32 (one logit per RoI), rcnn_reg [B,S,7] f32, and the
    targets ``roi_targets`` makes, read where they are: cls_target [B,S] f32 (-1: ignored), reg_valid [B,S] int32, reg_target
    [B,S,7]; with rois [B,S,D>=7] (``rois_s``; only the extents are read) and gt_local [B,S,7] the corner loss is on (both or
    neither) -> (loss [B,3] = (cls, reg, corner), num [B,2] int32 = (n_cls, n_reg), grad_cls [B,S], grad_reg [B,S,7]
    [, grad_corner [B,S,7]][, per_roi [B,S,3]]): binary cross-entropy on the soft target over the rows with cls_target >= 0,
    smooth-L1 over the rows with reg_valid != 0, and the replaced code bases' ``get_corner_loss_lidar`` on the decoded box over
    the same rows, each scaled by ``scale[i] / max(n, 1)`` per scene (``normalize=False``: by ``scale[i]``).  grad_reg and
    grad_corner are the gradients of loss[:, 1] and loss[:, 2] with respect to rcnn_reg.  One launch, no workspace, no
    synchronisation, bit-identical from call to call.  ``out``: the tuple to write into."""
    _strict(rcnn_cls, "rcnn_cls", torch.float32, (None, None), "[B,S] with 1 <= B <= 65535 and 1 <= S <= 1024")
    B, S = rcnn_cls.shape
    if not (1 <= B <= 65535 and 1 <= S <= 1024):
        raise ValueError(f"rcnn_cls: expected [B,S] with 1 <= B <= 65535 and 1 <= S <= 1024, got {tuple(rcnn_cls.shape)}")
    _strict(rcnn_reg, "rcnn_reg", torch.float32, (B, S, 7))
    _strict(cls_target, "cls_target", torch.float32, (B, S))
    _strict(reg_valid, "reg_valid", torch.int32, (B, S))
    _strict(reg_target, "reg_target", torch.float32, (B, S, 7))
    if (rois is None) != (gt_local is None):
        raise ValueError("rois and gt_local must be given together (the corner component)")
    corner, D = rois is not None, 0
    if corner:
        _strict(rois, "rois", torch.float32, (B, S, None), f"[B,S,D] with B = {B}, S = {S} and D >= 7")
        D = rois.shape[2]
        if D < 7:
            raise ValueError(f"rois: expected [B,S,D] with B = {B}, S = {S} and D >= 7, got {tuple(rois.shape)}")
        _strict(gt_local, "gt_local", torch.float32, (B, S, 7))
    beta = _f32(beta)
    if not beta > 0.0:
        raise ValueError(f"beta: must be > 0, got {beta}")
    cw, sc = _weights(code_weights, 7, "code_weights"), _weights(scale, 3, "scale")
    dev = _head_devices((("rcnn_cls", rcnn_cls), ("rcnn_reg", rcnn_reg), ("cls_target", cls_target), ("reg_valid", reg_valid),
                         ("reg_target", reg_target), ("rois", rois), ("gt_local", gt_local)))
    outs = _outputs(roi_loss_output_spec(B, S, corner, bool(per_roi)), out, dev, "rcnn_cls")
    a = _lib.RoiHeadLossArgs()
    a.struct_size = ctypes.sizeof(_lib.RoiHeadLossArgs)
    a.rcnn_cls, a.rcnn_reg, a.cls_target, a.reg_valid, a.reg_target = (t.data_ptr() for t in (rcnn_cls, rcnn_reg, cls_target, reg_valid, reg_target))
    a.rois, a.gt_local = _ptr(rois), _ptr(gt_local)
    a.B, a.S, a.D, a.normalize, a.beta = B, S, D, int(bool(normalize)), beta
    a.code_weights[:], a.scale[:] = cw, sc
    a.loss, a.num, a.grad_cls, a.grad_reg = (t.data_ptr() for t in outs[:4])
    a.grad_corner = outs[4].data_ptr() if corner else None
    a.per_roi = outs[-1].data_ptr() if per_roi else None
    with _timed("roi_head_loss", f"S{S}"):
        check(lib().sad_roi_head_loss_f32(ctypes.byref(a), _stream()), "sad_roi_head_loss_f32")
    return outs


def rotated_iou_loss_output_spec(lead: tuple, need_grad: bool, decoded: bool) -> tuple:
    """((name, shape, dtype), ...) of ``rotated_iou_loss``' outputs for pairs of leading shape ``lead``, what its ``out=`` tuple
    is checked against."""
    f32, lead = torch.float32, tuple(lead)
    spec = [("loss", lead, f32), ("iou", lead, f32)]
    if need_grad:
        spec.append(("grad", lead + (7,), f32))
    if decoded:
        spec.append(("decoded", lead + (7,), f32))
    return tuple(spec)


def _box_rows(t: torch.Tensor, name: str, lead: Optional[tuple] = None) -> torch.Tensor:
    """Box rows [..., D >= 7] of the strict policy (at least one leading axis; ``lead``: the leading shape they must have)."""
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name}: expected a torch.Tensor")
    want = "[..., D] with D >= 7 and at least one leading axis" if lead is None else f"[..., D] with leading shape {tuple(lead)} and D >= 7"
    shape = (None,) * max(t.dim(), 2) if lead is None else tuple(lead) + (None,)
    _strict(t, name, torch.float32, shape, want)
    if t.shape[-1] < 7 or t.numel() == 0:
        raise ValueError(f"{name}: expected {want}, got {tuple(t.shape)}")
    return t


def rotated_iou_loss(pred: torch.Tensor, target: torch.Tensor, weight: Optional[torch.Tensor] = None, *, mode: str = "3d",
                     kind: str = "iou", code: str = "box", rois: Optional[torch.Tensor] = None, need_grad: bool = True,
                     decoded: bool = False, out: Optional[tuple] = None) -> tuple:
    """Rotated IoU loss of aligned pairs with its analytic gradient (SPEC.md §34).  pred [...,Dp], target [...,Dt] f32 box rows
    (D >= 7, seven columns read) of one leading shape, weight [...] f32 or None -> (loss [...], iou [...] [, grad [...,7]]
    [, decoded [...,7]]).  ``iou`` is the rotated IoU of the pair (``mode`` "bev" or "3d"), bit-equal to the diagonal of
    ``boxes_iou_bev`` / ``boxes_iou3d``; ``loss = weight * (1 - iou)``, ``kind="diou"`` adds the squared centre distance over the
    squared diagonal of the box aligned with the target's axes around both boxes; ``grad`` is d loss / d pred, the target is a
    constant.  A row of weight 0 gives loss = grad = 0 whatever its boxes hold.  ``code="roi"``: pred is a RoI head's
    ``rcnn_reg``, target ``roi_targets``' ``gt_local`` and ``rois`` [...,D] (``rois_s``) is required; the box is decoded in the
    RoI's frame, ``grad`` is with respect to the residuals and ``decoded=True`` returns the box.  One launch, no workspace, no
    synchronisation, bit-identical from call to call.  ``out``: the tuple to write into."""
    _box_rows(pred, "pred")
    lead = tuple(pred.shape[:-1])
    if pred.numel() // pred.shape[-1] >= 2 ** 31:
        raise ValueError(f"pred: {pred.numel() // pred.shape[-1]} pairs (fewer than 2^31 supported)")
    _box_rows(target, "target", lead)
    if weight is not None:
        _strict(weight, "weight", torch.float32, lead)
    for name, v, table in (("mode", mode, _lib.IOU_MODES), ("kind", kind, _lib.IOU_LOSS_KINDS), ("code", code, _lib.IOU_CODES)):
        if v not in table:
            raise ValueError(f"{name}: expected one of {sorted(table)}, got {v!r}")
    if (rois is not None) != (code == "roi"):
        raise ValueError('rois must be given with code="roi" and only then')
    if decoded and code != "roi":
        raise ValueError('decoded: the decoded box is an output of code="roi" only')
    if rois is not None:
        _box_rows(rois, "rois", lead)
    dev = _head_devices((("pred", pred), ("target", target), ("weight", weight), ("rois", rois)))
    outs = _outputs(rotated_iou_loss_output_spec(lead, bool(need_grad), bool(decoded)), out, dev, "pred")
    a = _lib.RotatedIouLossArgs()
    a.struct_size = ctypes.sizeof(_lib.RotatedIouLossArgs)
    a.pred, a.target, a.weight, a.rois = pred.data_ptr(), target.data_ptr(), _ptr(weight), _ptr(rois)
    a.N, a.Dp, a.Dt, a.Dr = pred.numel() // pred.shape[-1], pred.shape[-1], target.shape[-1], rois.shape[-1] if rois is not None else 0
    a.mode, a.kind, a.code, a.need_grad = _lib.IOU_MODES[mode], _lib.IOU_LOSS_KINDS[kind], _lib.IOU_CODES[code], int(bool(need_grad))
    a.loss, a.iou = outs[0].data_ptr(), outs[1].data_ptr()
    a.grad = outs[2].data_ptr() if need_grad else None
    a.decoded = outs[-1].data_ptr() if decoded else None
    with _timed("rotated_iou_loss", f"{mode}{kind}N{a.N}"):
        check(lib().sad_rotated_iou_loss_f32(ctypes.byref(a), _stream()), "sad_rotated_iou_loss_f32")
    return outs


def boxes_iou_aligned(a: torch.Tensor, b: torch.Tensor, mode: str = "3d") -> torch.Tensor:
    """Rotated IoU of the aligned pairs (a_i, b_i) (SPEC.md §34): a [...,Da], b [...,Db] -> iou [...], the diagonal of
    ``boxes_iou_bev`` / ``boxes_iou3d`` without the matrix.  ``rotated_iou_loss``' launch with ``need_grad=False``."""
    return rotated_iou_loss(a, b, mode=mode, need_grad=False)[1]


POINT_OUTPUTS = ("labels", "match", "centerness", "shift_target", "size_target", "reg_target")


def point_output_spec(B: int, M: int) -> tuple:
    """((name, shape, dtype), ...) of ``point_targets``' outputs, what its ``out=`` tuple is checked against."""
    i32, f32 = torch.int32, torch.float32
    return (("labels", (B, M), i32), ("match", (B, M), i32), ("centerness", (B, M), f32), ("shift_target", (B, M, 3), f32),
            ("size_target", (B, M, 3), f32), ("reg_target", (B, M, 7), f32))


def _point_rows(t: torch.Tensor, name: str, what: str = "B * M < 2^31") -> Tuple[int, int]:
    """(B, M) of a point-major tensor [B,M,...] whose dtype and rank were judged already."""
    B, M = t.shape[:2]
    if not (1 <= B <= 65535 and M >= 1 and B * M < 2 ** 31):
        raise ValueError(f"{name}: expected 1 <= B <= 65535, M >= 1 and {what}, got {tuple(t.shape)}")
    return B, M


def point_targets(xyz: torch.Tensor, cand: Optional[torch.Tensor], gt_boxes: torch.Tensor, gt_labels: torch.Tensor, *, anchors,
                  size_anchor, shift_max: float, extra_width: float = 0.2, out: Optional[tuple] = None) -> tuple:
    """Point head target assignment (SPEC.md §31.1).  xyz [B,M,3] f32: the origin points (the detector: the first K SA3 points);
    cand [B,M,3] f32 or ``None`` (= xyz): where the head predicts from (§8 step 2's shifted candidates); gt_boxes [B,G,D>=7] f32,
    gt_labels [B,G] int32 (outside [0, C): padding; so is a box with a non-positive extent), G <= 1024; anchors [C,3]: §9's class
    anchors; size_anchor [3]: §8's ``anchor_car`` -> (labels [B,M] int32, match [B,M] int32, centerness [B,M], shift_target
    [B,M,3], size_target [B,M,3], reg_target [B,M,7]).  A point is assigned by its ORIGIN (3DSSD's rule): the lowest box that
    contains xyz gives the class and the index; a point in no box but within ``extra_width`` of one is ignored (-2), any other
    is background (-1).  centerness and reg_target (centre - cand, clamp(log(size / anchors[class]), +-2), yaw) are taken at
    cand; shift_target = clamp(centre - xyz, +-shift_max) and size_target invert §8 steps 2 and 3.  One launch, no workspace,
    no synchronisation, no gradients, bit-identical from call to call.  ``out``: the tuple to write into."""
    _strict(xyz, "xyz", torch.float32, (None, None, 3), "[B,M,3]")
    B, M = _point_rows(xyz, "xyz")
    if cand is not None:
        _strict(cand, "cand", torch.float32, (B, M, 3))
    an = np.asarray(anchors, dtype=np.float32)
    if an.ndim != 2 or an.shape[1] != 3 or not 1 <= an.shape[0] <= 16:
        raise ValueError(f"anchors: expected [C,3] with 1 <= C <= 16, got {an.shape}")
    sa = np.asarray(size_anchor, dtype=np.float32).reshape(-1)
    if sa.shape[0] != 3:
        raise ValueError(f"size_anchor: expected 3 values, got {sa.shape[0]}")
    if not (an > 0).all() or not (sa > 0).all():
        raise ValueError("anchors / size_anchor: every extent must be > 0")
    if not (float(shift_max) >= 0.0 and float(extra_width) >= 0.0):
        raise ValueError(f"shift_max, extra_width: need >= 0 (got {shift_max}, {extra_width})")
    C = an.shape[0]
    Bg, G, D, dev = _gt_inputs(gt_boxes, gt_labels)
    if Bg != B:
        raise ValueError(f"gt_boxes: expected B = {B} scenes, got {Bg}")
    if _head_devices((("xyz", xyz), ("cand", cand))) != dev:
        raise ValueError("xyz / cand: must be on the device of gt_boxes")
    outs = _outputs(point_output_spec(B, M), out, dev, "xyz")
    a = _lib.PointTargetsArgs()
    a.struct_size = ctypes.sizeof(_lib.PointTargetsArgs)
    a.xyz, a.cand = xyz.data_ptr(), _ptr(cand)
    a.gt_boxes, a.gt_labels = (gt_boxes.data_ptr(), gt_labels.data_ptr()) if G else (None, None)
    a.B, a.M, a.G, a.D, a.C = B, M, G, D, C
    a.anchors[:3 * C] = an.reshape(-1).tolist()
    a.size_anchor[:] = sa.tolist()
    a.shift_max, a.extra_width = _f32(shift_max), _f32(extra_width)
    a.labels, a.match, a.centerness, a.shift_target, a.size_target, a.reg_target = (t.data_ptr() for t in outs)
    with _timed("point_targets", f"M{M}G{G}"):
        check(lib().sad_point_targets_f32(ctypes.byref(a), _stream()), "sad_point_targets_f32")
    return outs


def point_loss_output_spec(B: int, M: int, C: int, with_c: bool, per_point: bool) -> tuple:
    """((name, shape, dtype), ...) of ``point_head_loss``' outputs, what its ``out=`` tuple is checked against."""
    f32 = torch.float32
    spec = [("loss", (B, 4), f32), ("num_pos", (B,), torch.int32), ("grad_o", (B, M, C + 7), f32)]
    if with_c:
        spec.append(("grad_c", (B, M, 6), f32))
    if per_point:
        spec.append(("per_point", (B, M, 4), f32))
    return tuple(spec)


def point_head_loss_workspace(B: int, M: int, device) -> torch.Tensor:
    """The workspace of ``point_head_loss(..., workspace=...)`` for a caller that keeps it."""
    nbytes = lib().sad_point_head_loss_workspace_bytes(B, M)
    if not nbytes:
        raise ValueError(f"point_head_loss_workspace: unsupported shape B = {B}, M = {M}")
    return torch.empty(nbytes, dtype=torch.uint8, device=device)


def point_head_loss(o: torch.Tensor, c: Optional[torch.Tensor], labels: torch.Tensor, centerness: Optional[torch.Tensor],
                    reg_target: torch.Tensor, shift_target: Optional[torch.Tensor] = None, size_target: Optional[torch.Tensor] = None, *,
                    cls_loss: str = "bce", alpha: float = 0.25, beta: float = 1.0 / 9.0, code_weights=None,
                    shift_max: Optional[float] = None, scale=(1.0, 1.0, 1.0, 1.0), normalize: bool = True, per_point: bool = False,
                    workspace: Optional[torch.Tensor] = None, out: Optional[tuple] = None) -> tuple:
    """Point head losses with their gradients (SPEC.md §31.2).  o [B,M,C+7] f32 (the head's rows: C class logits, then §9's box
    code), c [B,M,6] f32 or ``None`` (the cluster layer's rows: shift, size), and the targets ``point_targets`` makes, read where
    they are: labels [B,M] int32, centerness [B,M] or ``None``, reg_target [B,M,7], shift_target / size_target [B,M,3] or
    ``None`` -> (loss [B,4] = (cls, reg, shift, size), num_pos [B] int32, grad_o [B,M,C+7][, grad_c [B,M,6]][, per_point
    [B,M,4]]).  Classification over the rows that are not ignored: ``"bce"``, binary cross-entropy against the centre-ness at
    the label's channel (3DSSD), or ``"focal"``, the sigmoid focal loss of ``anchor_head_loss``; smooth-L1 with the
    sine-difference yaw of the box code (sizes clamped to +-2 as the decode does), of clamp(c[0:3], +-shift_max) and of
    clamp(c[3:6], +-1) over the positives; each scaled by ``scale[i] / max(num_pos[b], 1)`` per scene (``normalize=False``: by
    ``scale[i]``).  The shift / size components are on iff c and their target are given.  grad_o holds d loss[:, 0] in its
    first C columns and d loss[:, 1] in the last 7; grad_c d loss[:, 2] in columns 0..2 and d loss[:, 3] in 3..5.  Two small
    launches around one pass over the rows, no synchronisation, bit-identical from call to call.  ``out``: the tuple to write into."""
    _strict(o, "o", torch.float32, (None, None, None), "[B,M,C+7] with 1 <= C <= 16")
    B, M = _point_rows(o, "o")
    C = o.shape[2] - 7
    if not 1 <= C <= 16:
        raise ValueError(f"o: expected [B,M,C+7] with 1 <= C <= 16, got {tuple(o.shape)}")
    if cls_loss not in _lib.POINT_CLS_LOSSES:
        raise ValueError(f"cls_loss: expected 'bce' or 'focal', got {cls_loss!r}")
    if c is None and (shift_target is not None or size_target is not None):
        raise ValueError("shift_target / size_target need c (the cluster layer's rows)")
    if c is not None and shift_target is None and size_target is None:
        raise ValueError("c needs shift_target or size_target (without either it has no loss)")
    for name, t, shape, dt in (("c", c, (B, M, 6), torch.float32), ("labels", labels, (B, M), torch.int32),
                               ("centerness", centerness, (B, M), torch.float32), ("reg_target", reg_target, (B, M, 7), torch.float32),
                               ("shift_target", shift_target, (B, M, 3), torch.float32), ("size_target", size_target, (B, M, 3), torch.float32)):
        if t is not None or name in ("labels", "reg_target"):
            _strict(t, name, dt, shape)
    beta = _f32(beta)
    if not beta > 0.0:
        raise ValueError(f"beta: must be > 0, got {beta}")
    if not 0.0 <= float(alpha) <= 1.0:
        raise ValueError(f"alpha: expected a value in [0, 1], got {alpha}")
    if shift_target is not None and not (shift_max is not None and float(shift_max) >= 0.0):
        raise ValueError(f"shift_max: the shift component needs shift_max >= 0 (got {shift_max})")
    cw, sc = _weights(code_weights, 7, "code_weights"), _weights(scale, 4, "scale")
    dev = _head_devices((("o", o), ("c", c), ("labels", labels), ("centerness", centerness), ("reg_target", reg_target),
                         ("shift_target", shift_target), ("size_target", size_target)))
    outs = _outputs(point_loss_output_spec(B, M, C, c is not None, bool(per_point)), out, dev, "o")
    workspace = _workspace(lib().sad_point_head_loss_workspace_bytes(B, M), workspace, dev, "ops.point_head_loss_workspace")
    a = _lib.PointHeadLossArgs()
    a.struct_size = ctypes.sizeof(_lib.PointHeadLossArgs)
    a.o, a.c, a.labels, a.centerness, a.reg_target = o.data_ptr(), _ptr(c), labels.data_ptr(), _ptr(centerness), reg_target.data_ptr()
    a.shift_target, a.size_target = _ptr(shift_target), _ptr(size_target)
    a.B, a.M, a.C, a.cls_loss, a.normalize = B, M, C, _lib.POINT_CLS_LOSSES[cls_loss], int(bool(normalize))
    a.alpha, a.beta, a.shift_max = _f32(alpha), beta, _f32(0.0 if shift_max is None else shift_max)
    a.code_weights[:], a.scale[:] = cw, sc
    a.loss, a.num_pos, a.grad_o = (t.data_ptr() for t in outs[:3])
    a.grad_c = outs[3].data_ptr() if c is not None else None
    a.per_point = outs[-1].data_ptr() if per_point else None
    a.workspace = workspace.data_ptr()
    with _timed("point_head_loss", f"M{M}C{C}"):
        check(lib().sad_point_head_loss_f32(ctypes.byref(a), _stream()), "sad_point_head_loss_f32")
    return outs


def candidates_grad_output_spec(B: int, K: int) -> tuple:
    """((name, shape, dtype),) of ``candidates_grad``'s output, what its ``out=`` is checked against."""
    return (("grad_c", (B, K, 6), torch.float32),)


def prefix_rows_grad_output_spec(B: int, M: int, C: int) -> tuple:
    """((name, shape, dtype),) of ``prefix_rows_grad``'s output, what its ``out=`` is checked against."""
    return (("out", (B, M, C), torch.float32),)


def _shift_max(shift_max) -> float:
    """§8 step 2's clamp bound as the float32 the kernels get: >= 0, not NaN."""
    if not float(shift_max) >= 0.0:
        raise ValueError(f"shift_max: need >= 0 (got {shift_max})")
    return _f32(shift_max)


def candidates(xyz3: torch.Tensor, c: torch.Tensor, K: int, shift_max: float, r_min: float, r_max: float, anchor,
               out: Optional[tuple] = None) -> tuple:
    """Candidate centres and adaptive radius (SPEC.md §8 steps 2-4).  xyz3 [B,M3,3] f32 (SA3's centroids), c [B,K,6] f32 (the
    candidate layer's rows: shift, size), 1 <= K <= M3, anchor [3] (§8's ``anchor_car``) -> (cand [B,K,3] = xyz3[:, :K] +
    clamp(c[..., 0:3], +-shift_max), radius [B,K]).  One launch.  ``out``: the tuple to write into."""
    _strict(xyz3, "xyz3", torch.float32, (None, None, 3), "[B,M3,3]")
    B, M3 = _point_rows(xyz3, "xyz3")
    K = int(K)
    if not 1 <= K <= M3:
        raise ValueError(f"K: expected 1 <= K <= M3 = {M3}, got {K}")
    _strict(c, "c", torch.float32, (B, K, 6))
    sm = _shift_max(shift_max)
    an = np.asarray(anchor, dtype=np.float32).reshape(-1)
    if an.shape[0] != 3:
        raise ValueError(f"anchor: expected 3 values, got {an.shape[0]}")
    dev = _head_devices((("xyz3", xyz3), ("c", c)))
    if xyz3.device != c.device:
        raise ValueError("c: must be on the device of xyz3")
    cand, radius = _outputs((("cand", (B, K, 3), torch.float32), ("radius", (B, K), torch.float32)), out, dev, "xyz3")
    with _timed("candidates", f"K{K}"):
        check(lib().sad_candidates_f32(xyz3.data_ptr(), c.data_ptr(), B, M3, K, sm, _f32(r_min), _f32(r_max),
                                       (ctypes.c_float * 3)(*an.tolist()), cand.data_ptr(), radius.data_ptr(), _stream()),
              "sad_candidates_f32")
    return cand, radius


def candidates_grad(c: torch.Tensor, grad_cand: torch.Tensor, shift_max: float, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The backward of ``candidates`` with respect to c (SPEC.md §33.1).  c [B,K,6] f32, grad_cand [B,K,3] f32 -> grad_c [B,K,6]:
    column d < 3 is grad_cand's where -shift_max <= c[..., d] <= shift_max (bounds included, §31.2's convention; a selection, so a
    NaN c gives +0), else +0; columns 3..5 are +0: the size columns reach the forward only through the radius of an index
    decision and are trained by ``size_target`` alone.  One launch, every element written, bit-identical from call to call.
    ``out``: the tensor to write into."""
    _strict(c, "c", torch.float32, (None, None, 6), "[B,K,6]")
    B, K = _point_rows(c, "c", "B * K < 2^31")
    _strict(grad_cand, "grad_cand", torch.float32, (B, K, 3))
    sm = _shift_max(shift_max)
    dev = _head_devices((("c", c), ("grad_cand", grad_cand)))
    if c.device != grad_cand.device:
        raise ValueError("grad_cand: must be on the device of c")
    (grad_c,) = _outputs(candidates_grad_output_spec(B, K), None if out is None else (out,), dev, "c")
    with _timed("candidates_grad", f"K{K}"):
        check(lib().sad_candidates_grad_f32(c.data_ptr(), grad_cand.data_ptr(), B, K, sm, grad_c.data_ptr(), _stream()),
              "sad_candidates_grad_f32")
    return grad_c


def prefix_rows_grad(g: torch.Tensor, M: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The backward of ``prefix_rows`` (SPEC.md §33.2).  g [B,K,C] f32, M >= K -> [B,M,C]: rows < K of every scene are g's, rows
    K .. M-1 are +0.  One launch writes every element exactly once (no zero fill in front).  ``out``: the tensor to write into."""
    _strict(g, "g", torch.float32, (None, None, None), "[B,K,C] with B, K, C >= 1")
    B, K, C = g.shape
    if min(B, K, C) < 1:
        raise ValueError(f"g: expected [B,K,C] with B, K, C >= 1, got {tuple(g.shape)}")
    M = int(M)
    if M < K:
        raise ValueError(f"M: expected M >= K = {K}, got {M}")
    dev = _head_devices((("g", g),))
    (res,) = _outputs(prefix_rows_grad_output_spec(B, M, C), None if out is None else (out,), dev, "g")
    with _timed("prefix_rows_grad", f"K{K}M{M}"):
        check(lib().sad_prefix_rows_grad_f32(g.data_ptr(), B, K, M, C, res.data_ptr(), _stream()), "sad_prefix_rows_grad_f32")
    return res


def roi_grid_points(rois: torch.Tensor, roi_count: Optional[torch.Tensor], grid_size: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The grid points of every RoI (SPEC.md §30): rois [B,R,D>=7] f32 rows (cx,cy,cz,l,w,h,yaw,...), roi_count [B] int32 or
    ``None`` (as in ``roi_targets``: the rows beyond it are never read) -> pts [B,R,G^3,3] with G = ``grid_size`` (1 .. 16): point
    g = (ix*G + iy)*G + iz sits at ((i + 0.5) / G - 0.5) * extent on each axis of the RoI's frame, rotated by its yaw and moved to
    its centre.  The points of a row beyond ``roi_count`` are NaN, which ``voxel_query`` answers with an empty neighbourhood, so the
    output of ``nms_boxes`` is pooled with nothing synchronised in between.  One launch."""
    _strict(rois, "rois", torch.float32, (None, None, None), "[B,R,D] with B, R >= 1 and D >= 7")
    B, R, D = rois.shape
    if B < 1 or R < 1 or D < 7:
        raise ValueError(f"rois: expected [B,R,D] with B, R >= 1 and D >= 7, got {tuple(rois.shape)}")
    if roi_count is not None:
        _strict(roi_count, "roi_count", torch.int32, (B,))
    G = int(grid_size)
    if not 1 <= G <= 16:
        raise ValueError(f"grid_size: expected 1 .. 16, got {G}")
    if B > 65535 or B * R * G ** 3 >= 2 ** 31:
        raise ValueError(f"rois: B <= 65535 and B * R * G^3 < 2^31 supported (got B = {B}, R = {R}, G = {G})")
    dev = _head_devices((("rois", rois), ("roi_count", roi_count)))
    pts, = _outputs((("pts", (B, R, G ** 3, 3), torch.float32),), None if out is None else (out,), dev, "rois")
    a = _lib.RoiGridPointsArgs()
    a.struct_size = ctypes.sizeof(_lib.RoiGridPointsArgs)
    a.rois, a.roi_count, a.pts = rois.data_ptr(), _ptr(roi_count), pts.data_ptr()
    a.B, a.R, a.D, a.G = B, R, D, G
    with _timed("roi_grid_points", f"R{B * R}G{G}"):
        check(lib().sad_roi_grid_points_f32(ctypes.byref(a), _stream()), "sad_roi_grid_points_f32")
    return pts


def voxel_query_workspace(Nv: int, device) -> torch.Tensor:
    """The workspace of ``voxel_query(..., workspace=...)`` (the coordinate table of ``Nv`` voxels) for a caller that keeps it."""
    nbytes = lib().sad_voxel_query_workspace_bytes(int(Nv))
    if not nbytes:
        raise ValueError(f"voxel_query_workspace: need 0 <= Nv <= 2^30 (got {Nv})")
    return torch.empty(nbytes, dtype=torch.uint8, device=device)


def voxel_query(coors: torch.Tensor, offsets: torch.Tensor, spatial_shape, voxel_size, point_range, new_xyz: torch.Tensor, *,
                max_range, radius: float, S: int, out: Optional[tuple] = None, workspace: Optional[torch.Tensor] = None) -> tuple:
    """The non-empty voxels around every query point, in walk order (SPEC.md §30).  coors [Nv,3] int32 (z,y,x), offsets [B+1] int32
    and ``spatial_shape`` (Gz,Gy,Gx): a sparse tensor of §21; ``voxel_size`` (vx,vy,vz): the size of a voxel AT THAT SCALE (base
    size x stride); ``point_range`` (x0,y0,z0,x1,y1,z1), of which the low corner is read; new_xyz [B,M,3] f32 ->
    (idx [B,M,S] int32, cnt [B,M] int32).  The candidates of a query are the cells within ``max_range`` = (rz,ry,rx) cells of its
    own, walked dz slowest and dx fastest; one counts if the query's scene holds a voxel there whose centre is closer than
    ``radius`` (strict).  idx holds the GLOBAL rows (into Nv) of the first S in walk order, padded with the first; cnt =
    min(accepted, S); a NaN / Inf query, and one with nothing in reach, gives cnt 0 and idx 0: what ``PackedMLP.grouped`` takes as
    (idx, cnt) with the voxels as one scene.  Three launches, no synchronisation, no gradients, bit-identical from call to call."""
    vs, pr = _voxel_grid(voxel_size, point_range)
    G, _ = _int3(spatial_shape, "spatial_shape", 1)
    if isinstance(max_range, (int, np.integer)):
        raise ValueError("max_range: 3 ints (rz,ry,rx) expected")
    rng, _ = _int3(max_range, "max_range", 0)
    if max(rng) > 8:
        raise ValueError(f"max_range: entries 0 .. 8 are implemented, got {rng}")
    S, radius = int(S), _f32(radius)
    if not 1 <= S <= 128:
        raise ValueError(f"S: expected 1 .. 128, got {S}")
    if not radius > 0.0:
        raise ValueError(f"radius: must be > 0, got {radius}")
    if G[0] * G[1] * G[2] > 2 ** 31 - 1:
        raise ValueError(f"spatial_shape {G} exceeds 2^31 - 1 cells")
    coors, offsets, B = _sparse_coors(coors, offsets)
    new_xyz = _need(new_xyz, "new_xyz", torch.float32, 3)
    if new_xyz.shape[0] != B or new_xyz.shape[2] != 3:
        raise ValueError(f"new_xyz: expected [B,M,3] with B = {B}, got {tuple(new_xyz.shape)}")
    if new_xyz.device != coors.device:
        raise ValueError("new_xyz must be on the device of coors")
    Nv, M, dev = coors.shape[0], new_xyz.shape[1], coors.device
    if B > 65535 or B * M * S >= 2 ** 31 or Nv > 2 ** 30:
        raise ValueError(f"voxel_query: B <= 65535, B * M * S < 2^31 and Nv <= 2^30 supported (got B = {B}, M = {M}, S = {S}, Nv = {Nv})")
    idx, cnt = _outputs((("idx", (B, M, S), torch.int32), ("cnt", (B, M), torch.int32)), out, dev, "coors")
    workspace = _workspace(lib().sad_voxel_query_workspace_bytes(Nv), workspace, dev, "ops.voxel_query_workspace", 16)
    a = _lib.VoxelQueryArgs()
    a.struct_size = ctypes.sizeof(_lib.VoxelQueryArgs)
    a.coors, a.offsets, a.new_xyz = coors.data_ptr(), offsets.data_ptr(), new_xyz.data_ptr()
    a.Nv, a.B, a.M, a.S = Nv, B, M, S
    a.spatial_shape[:], a.max_range[:], a.voxel_size[:], a.lo[:], a.radius = G, rng, list(vs), list(pr)[:3], radius
    a.idx, a.cnt, a.workspace = idx.data_ptr(), cnt.data_ptr(), workspace.data_ptr()
    with _timed("voxel_query", f"n{Nv}m{B * M}s{S}"):
        check(lib().sad_voxel_query_f32(ctypes.byref(a), _stream()), "sad_voxel_query_f32")
    return idx, cnt


PASTE_MAX_SLOTS = 512          # Q of SPEC.md §35.2


def augment_seed(seed: int, step: int) -> int:
    """The seed of call number ``step`` (SPEC.md §35): §17's hash of (seed, step), as ``ProposalTargetLayer.call_seed``."""
    from . import io as _io
    return int(_io._h(int(seed), int(step), 0))


def _range2(v, name: str) -> Tuple[float, float]:
    lo, hi = (v if isinstance(v, (tuple, list)) else (-v, v))
    lo, hi = _f32(lo), _f32(hi)
    if not lo <= hi:
        raise ValueError(f"{name}: expected (lo, hi) with lo <= hi, got {v!r}")
    return lo, hi


def _aug_points(points: torch.Tensor, offsets: Optional[torch.Tensor]):
    """Ragged ``points [total,Cp]`` + ``offsets [B+1]`` int32, or padded ``points [B,N,Cp]`` with ``offsets=None`` ->
    (shape, B, N, total, Cp): contiguous f32, judged before any device."""
    if offsets is None:
        _strict(points, "points", torch.float32, (None, None, None), "[B,N,Cp] (or [total,Cp] with offsets)")
        B, N, Cp = points.shape
        total = B * N
    else:
        _strict(points, "points", torch.float32, (None, None), "[total,Cp] with offsets")
        _strict(offsets, "offsets", torch.int32, (None,), "[B+1]")
        (total, Cp), B, N = points.shape, offsets.shape[0] - 1, 0
    if B < 1 or Cp < 3:
        raise ValueError(f"points: expected at least one scene and Cp >= 3 columns, got {tuple(points.shape)}")
    if total * Cp >= 1 << 31:
        raise ValueError("points: too many rows")
    return tuple(points.shape), B, N, total, Cp


def global_augment_output_spec(points_shape: tuple, B: int, G: int, D: int) -> tuple:
    """((name, shape, dtype), ...) of ``global_augment``'s outputs, what its ``out=`` tuple is checked against."""
    f32 = torch.float32
    return (("points_out", tuple(points_shape), f32), ("boxes_out", (B, G, D), f32), ("params", (B, 8), f32))


def global_augment(points: torch.Tensor, offsets: Optional[torch.Tensor], gt_boxes: torch.Tensor, *, seed: int = 0, step: int = 0,
                   flip_x: bool = True, flip_y: bool = False, rot_range=(-0.78539816, 0.78539816), scale_range=(0.95, 1.05),
                   translate_range=(0.0, 0.0, 0.0), with_velocity: bool = False, out: Optional[tuple] = None) -> tuple:
    """One random flip / rotation / scale / translation per scene, on points and boxes (SPEC.md §35.1).  points [total,Cp] +
    offsets [B+1] int32, or points [B,N,Cp] with ``offsets=None``; gt_boxes [B,G,D>=7] ->
    (points_out, boxes_out [B,G,D], params [B,8] = (flips, theta, cos, sin, scale, tx, ty, tz)).  The draws are §17's hash of
    (seed mixed with step, scene); ``flip_x`` / ``flip_y`` allow the flip, which one hash bit decides.  Order: flip about x
    (y = -y), flip about y, rotate, scale, translate; ``with_velocity`` (D >= 9) carries columns 7, 8 as a vector.  Every other
    column is a bit copy; every box row is transformed, padding included.  One launch, no synchronisation."""
    shape, B, N, total, Cp = _aug_points(points, offsets)
    _strict(gt_boxes, "gt_boxes", torch.float32, (B, None, None), f"[{B},G,D] with D >= 7")
    G, D = gt_boxes.shape[1:]
    if D < 7:
        raise ValueError(f"gt_boxes: box rows need at least 7 fields, got {D}")
    if G > 1024:
        raise ValueError(f"gt_boxes: at most 1024 boxes per scene (got G = {G})")
    if with_velocity and D < 9:
        raise ValueError(f"with_velocity: needs box rows of D >= 9 columns (got {D})")
    rot, sc = _range2(rot_range, "rot_range"), _range2(scale_range, "scale_range")
    tr = [_f32(v) for v in translate_range]
    if len(tr) != 3 or min(tr) < 0.0:
        raise ValueError(f"translate_range: expected three values >= 0, got {translate_range!r}")
    if not sc[0] > 0.0:
        raise ValueError(f"scale_range: expected 0 < lo <= hi, got {scale_range!r}")
    if max(abs(rot[0]), abs(rot[1])) >= 1e4:
        raise ValueError("rot_range: |angle| must be below 1e4")
    dev = _head_devices((("points", points), ("offsets", offsets), ("gt_boxes", gt_boxes)))
    outs = _outputs(global_augment_output_spec(shape, B, G, D), out, dev, "points")
    a = _lib.GlobalAugmentArgs()
    a.struct_size = ctypes.sizeof(_lib.GlobalAugmentArgs)
    a.points, a.offsets, a.gt_boxes = points.data_ptr(), _ptr(offsets), gt_boxes.data_ptr() if G else None
    a.B, a.N, a.total, a.Cp, a.G, a.D = B, N, total, Cp, G, D
    a.seed = augment_seed(seed, step)
    a.flip_x, a.flip_y, a.with_velocity = int(bool(flip_x)), int(bool(flip_y)), int(bool(with_velocity))
    a.rot_lo, a.rot_hi, a.scale_lo, a.scale_hi = rot[0], rot[1], sc[0], sc[1]
    a.translate[:] = tr
    a.points_out, a.boxes_out, a.params = outs[0].data_ptr(), outs[1].data_ptr() if G else None, outs[2].data_ptr()
    with _timed("global_augment", f"n{total}G{G}"):
        check(lib().sad_global_augment_f32(ctypes.byref(a), _stream()), "sad_global_augment_f32")
    return outs


PASTE_OUTPUTS = ("keep", "db_index", "boxes_out", "labels_out", "num_pasted", "out_points", "out_offsets")


def gt_paste_rows(total: int, B: int, Q: int, max_obj_points: int) -> int:
    """The least row count of ``gt_paste``'s ``out_points``: total + B * Q * max_obj_points (SPEC.md §35.2)."""
    return int(total) + int(B) * int(Q) * int(max_obj_points)


def gt_paste_output_spec(B: int, G: int, D: int, Q: int, Cp: int, R: int) -> tuple:
    """((name, shape, dtype), ...) of ``gt_paste``'s outputs, what its ``out=`` tuple is checked against."""
    i32, f32 = torch.int32, torch.float32
    return (("keep", (B, Q), i32), ("db_index", (B, Q), i32), ("boxes_out", (B, G + Q, D), f32), ("labels_out", (B, G + Q), i32),
            ("num_pasted", (B,), i32), ("out_points", (R, Cp), f32), ("out_offsets", (B + 1,), i32))


def gt_paste_workspace(B: int, Q: int, total: int, device) -> torch.Tensor:
    """The workspace of ``gt_paste(..., workspace=...)`` for a caller that keeps it."""
    nbytes = lib().sad_gt_paste_workspace_bytes(int(B), int(Q), int(total))
    if not nbytes:
        raise ValueError(f"gt_paste_workspace: need 1 <= B <= 65535, 1 <= Q <= {PASTE_MAX_SLOTS} and total >= 0 (got {B}, {Q}, {total})")
    return torch.empty(nbytes, dtype=torch.uint8, device=device)


def gt_paste(points: torch.Tensor, offsets: torch.Tensor, gt_boxes: torch.Tensor, gt_labels: torch.Tensor, db_points: torch.Tensor,
             db_offsets: torch.Tensor, db_boxes: torch.Tensor, class_offsets: Sequence[int], *, sample_num: Sequence[int],
             max_obj_points: int, seed: int = 0, step: int = 0, remove_extra_width: float = 0.0, params: Optional[torch.Tensor] = None,
             with_velocity: bool = False, out: Optional[tuple] = None, workspace: Optional[torch.Tensor] = None) -> tuple:
    """Ground-truth database sampling (SPEC.md §35.2).  points [total,Cp] + offsets [B+1] int32, padded gt_boxes [B,G,D] /
    gt_labels [B,G] int32; the database on the device: db_points [.,Cp], db_offsets [Ndb+1] int32, db_boxes [Ndb,D], entries
    sorted by class with the host list ``class_offsets`` [C+1]; ``sample_num`` [C] = the "fill up to" count per class, Q = its sum
    (<= 512).  -> (keep [B,Q], db_index [B,Q], boxes_out [B,G+Q,D], labels_out [B,G+Q], num_pasted [B], out_points [R,Cp],
    out_offsets [B+1]): accepted greedily in slot order where the candidate overlaps no valid ground-truth box and no accepted
    earlier slot in bird's-eye view; the scene points inside an accepted box (enlarged by ``remove_extra_width``) are dropped,
    the objects' points come first, then the survivors in file order.  ``out_points`` has R >= total + B*Q*max_obj_points rows,
    those at or beyond out_offsets[B] are not written.  ``params`` [B,8] (from ``global_augment``): that transform is applied
    as the rows are stored.  Four launches, no synchronisation, bit-identical from call to call."""
    _, B, _, total, Cp = _aug_points(points, offsets)
    if isinstance(gt_boxes, torch.Tensor) and gt_boxes.dim() == 3 and gt_boxes.shape[0] != B:
        raise ValueError(f"gt_boxes: expected {B} scenes like offsets, got {gt_boxes.shape[0]}")
    _, G, D = _gt_shapes(gt_boxes, gt_labels)
    class_offsets, sample_num = [int(v) for v in class_offsets], [int(v) for v in sample_num]
    C = len(sample_num)
    if not 1 <= C <= _lib.PASTE_MAX_CLASSES or len(class_offsets) != C + 1:
        raise ValueError(f"sample_num / class_offsets: expected C and C + 1 entries with 1 <= C <= {_lib.PASTE_MAX_CLASSES}")
    if min(sample_num) < 0 or sum(sample_num) < 1:
        raise ValueError(f"sample_num: expected counts >= 0 with a sum >= 1, got {sample_num}")
    Q = sum(sample_num)
    if Q > PASTE_MAX_SLOTS:
        raise ValueError(f"sample_num: Q = {Q} candidate slots per scene, at most {PASTE_MAX_SLOTS} are supported")
    _strict(db_points, "db_points", torch.float32, (None, Cp), f"[.,{Cp}]: the database must have the scene's {Cp} point columns")
    _strict(db_boxes, "db_boxes", torch.float32, (None, D), f"[Ndb,{D}]: the database must have the ground truth's {D} box columns")
    Ndb = db_boxes.shape[0]
    _strict(db_offsets, "db_offsets", torch.int32, (Ndb + 1,))
    if Ndb < 1 or class_offsets[0] != 0 or class_offsets[-1] != Ndb or any(a > b for a, b in zip(class_offsets, class_offsets[1:])):
        raise ValueError(f"class_offsets: expected an ascending list from 0 to Ndb = {Ndb}, got {class_offsets}")
    if with_velocity and D < 9:
        raise ValueError(f"with_velocity: needs box rows of D >= 9 columns (got {D})")
    if params is not None:
        _strict(params, "params", torch.float32, (B, 8))
    Pmax, e = int(max_obj_points), _f32(remove_extra_width)
    if Pmax < 0 or not e >= 0.0:
        raise ValueError("max_obj_points and remove_extra_width must be >= 0")
    need = gt_paste_rows(total, B, Q, Pmax)
    R = need
    if out is not None and len(out) == len(PASTE_OUTPUTS) and isinstance(out[5], torch.Tensor) and out[5].dim() == 2:
        R = out[5].shape[0]
        if R < need:
            raise ValueError(f"out_points: {R} rows, needs total + B*Q*max_obj_points = {need}")
    if need * Cp >= 1 << 31:
        raise ValueError("out_points: too many rows")
    dev = _head_devices((("points", points), ("offsets", offsets), ("gt_boxes", gt_boxes), ("gt_labels", gt_labels), ("db_points", db_points),
                         ("db_offsets", db_offsets), ("db_boxes", db_boxes), ("params", params)))
    outs = _outputs(gt_paste_output_spec(B, G, D, Q, Cp, R), out, dev, "points")
    workspace = _workspace(lib().sad_gt_paste_workspace_bytes(B, Q, total), workspace, dev, "ops.gt_paste_workspace", 16)
    a = _lib.GtPasteArgs()
    a.struct_size = ctypes.sizeof(_lib.GtPasteArgs)
    a.points, a.offsets = points.data_ptr(), offsets.data_ptr()
    a.gt_boxes, a.gt_labels = (gt_boxes.data_ptr(), gt_labels.data_ptr()) if G else (None, None)
    a.db_points, a.db_offsets, a.db_boxes, a.params = db_points.data_ptr(), db_offsets.data_ptr(), db_boxes.data_ptr(), _ptr(params)
    a.B, a.total, a.Cp, a.G, a.D, a.C, a.Ndb, a.max_obj_points, a.with_velocity = B, total, Cp, G, D, C, Ndb, Pmax, int(bool(with_velocity))
    a.class_offsets[:C + 1], a.sample_num[:C] = class_offsets, sample_num
    a.seed, a.remove_extra_width, a.R = augment_seed(seed, step), e, R
    for n, t in zip(PASTE_OUTPUTS, outs):
        setattr(a, n, t.data_ptr())
    a.workspace = workspace.data_ptr()
    with _timed("gt_paste", f"n{total}G{G}Q{Q}"):
        check(lib().sad_gt_paste_f32(ctypes.byref(a), _stream()), "sad_gt_paste_f32")
    return outs


DET_MATCH_OUTPUTS = ("code", "match", "value", "gt_det", "n_gt")
DET_AP_OUTPUTS = ("ap", "prec", "max_recall", "n_det")


def det_match_output_spec(B: int, K: int, G: int, C: int, T: int) -> tuple:
    """((name, shape, dtype), ...) of ``det_match``'s outputs, what its ``out=`` tuple is checked against."""
    i32, f32 = torch.int32, torch.float32
    return (("code", (B, K, T), i32), ("match", (B, K, T), i32), ("value", (B, K, T), f32), ("gt_det", (B, G, T), i32), ("n_gt", (B, C), i32))


def det_match(det_boxes: torch.Tensor, det_scores: torch.Tensor, det_labels: torch.Tensor, det_count: Optional[torch.Tensor],
              gt_boxes: torch.Tensor, gt_labels: torch.Tensor, gt_ignore: Optional[torch.Tensor], thr: torch.Tensor, *,
              metric: str = "iou3d", out: Optional[tuple] = None) -> tuple:
    """Score-ordered assignment of detections to ground truth, per scene (SPEC.md §36.1).  det_boxes [B,K,D>=7] f32 rows
    (cx,cy,cz,l,w,h,yaw,...), det_scores [B,K] f32, det_labels [B,K] int32, det_count [B] int32 or ``None`` (the rows beyond
    ``det_count[b]`` are never read: the gathered output of ``nms_boxes`` goes in as it is), gt_boxes [B,G,Dg>=7] / gt_labels
    [B,G] int32 (outside [0, C): padding), gt_ignore [B,G] int32 or ``None``, thr [C,T] f32 on the device ->
    (code [B,K,T] int32, match [B,K,T] int32, value [B,K,T] f32, gt_det [B,G,T] int32, n_gt [B,C] int32).
    Live detections (k < det_count, 0 <= label < C) are walked in §23's rank order, independently per threshold column: the best
    accepted box of the class that is neither ignored nor taken wins (code 1); else the best accepted ignored box absorbs the
    detection (code -1, never taken); else a false positive (code 0, match -1, value 0).  ``metric``: ``"iou3d"`` / ``"iou_bev"``
    (§19.3's bits, accepted iff v > thr) or ``"dist"`` (centre distance, accepted iff v < thr).  A row that is not live gets
    (-1, -1, 0).  K, G <= 1024, C <= 64, T <= 8.  One launch, no workspace, no synchronisation; two calls are bit-equal."""
    if metric not in _lib.DET_METRICS:
        raise ValueError(f"metric: expected 'iou3d', 'iou_bev' or 'dist', got {metric!r}")
    _strict(det_boxes, "det_boxes", torch.float32, (None, None, None), "[B,K,D] with B, K >= 1 and D >= 7")
    B, K, D = det_boxes.shape
    if B < 1 or K < 1 or D < 7:
        raise ValueError(f"det_boxes: expected [B,K,D] with B, K >= 1 and D >= 7, got {tuple(det_boxes.shape)}")
    if K > 1024:
        raise ValueError(f"det_boxes: at most 1024 detections per scene (got K = {K})")
    if B > 65535:
        raise ValueError(f"det_boxes: at most 65535 scenes (got B = {B})")
    _strict(det_scores, "det_scores", torch.float32, (B, K))
    _strict(det_labels, "det_labels", torch.int32, (B, K))
    if det_count is not None:
        _strict(det_count, "det_count", torch.int32, (B,))
    if isinstance(gt_boxes, torch.Tensor) and gt_boxes.dim() == 3 and gt_boxes.shape[0] != B:
        raise ValueError(f"gt_boxes: expected {B} scenes like det_boxes, got {gt_boxes.shape[0]}")
    _, G, Dg = _gt_shapes(gt_boxes, gt_labels)
    if gt_ignore is not None:
        _strict(gt_ignore, "gt_ignore", torch.int32, (B, G))
    _strict(thr, "thr", torch.float32, (None, None), "[C,T] with 1 <= C <= 64 and 1 <= T <= 8")
    C, T = thr.shape
    if not (1 <= C <= 64 and 1 <= T <= 8):
        raise ValueError(f"thr: expected [C,T] with 1 <= C <= 64 and 1 <= T <= 8, got {tuple(thr.shape)}")
    dev = _head_devices((("det_boxes", det_boxes), ("det_scores", det_scores), ("det_labels", det_labels), ("det_count", det_count),
                         ("gt_boxes", gt_boxes), ("gt_labels", gt_labels), ("gt_ignore", gt_ignore), ("thr", thr)))
    outs = _outputs(det_match_output_spec(B, K, G, C, T), out, dev, "det_boxes")
    a = _lib.DetMatchArgs()
    a.struct_size = ctypes.sizeof(_lib.DetMatchArgs)
    a.det_boxes, a.det_scores, a.det_labels, a.det_count = det_boxes.data_ptr(), det_scores.data_ptr(), det_labels.data_ptr(), _ptr(det_count)
    a.gt_boxes, a.gt_labels, a.gt_ignore = (gt_boxes.data_ptr(), gt_labels.data_ptr(), _ptr(gt_ignore)) if G else (None, None, None)
    a.thr = thr.data_ptr()
    a.B, a.K, a.D, a.G, a.Dg, a.C, a.T, a.metric = B, K, D, G, Dg, C, T, _lib.DET_METRICS[metric]
    for n, t in zip(DET_MATCH_OUTPUTS, outs):
        setattr(a, n, t.data_ptr() if t.numel() else None)
    with _timed("det_match", f"{metric}K{K}G{G}C{C}T{T}"):
        check(lib().sad_det_match_f32(ctypes.byref(a), _stream()), "sad_det_match_f32")
    return outs


def det_ap_output_spec(C: int, T: int, points: int = 40, first: int = 1) -> tuple:
    """((name, shape, dtype), ...) of ``det_ap``'s outputs, what its ``out=`` tuple is checked against."""
    f32 = torch.float32
    return (("ap", (C, T), f32), ("prec", (C, T, points - first + 1), f32), ("max_recall", (C, T), f32), ("n_det", (C, T), torch.int32))


def det_ap_workspace(N: int, device) -> torch.Tensor:
    """The workspace of ``det_ap(..., workspace=...)`` for a caller that keeps it: the N sort keys."""
    return torch.empty(max(8 * int(N), 8), dtype=torch.uint8, device=device)


def det_ap(scores: torch.Tensor, labels: torch.Tensor, code: torch.Tensor, n_gt: torch.Tensor, *, points: int = 40, first: int = 1,
           floor: float = 0.0, out: Optional[tuple] = None, workspace: Optional[torch.Tensor] = None) -> tuple:
    """Precision / recall and AP over accumulated rows (SPEC.md §36.2).  scores [N] f32, labels [N] int32, code [N,T] int32
    (``det_match``'s, rows flattened), n_gt [C] int32 -> (ap [C,T] f32, prec [C,T,points-first+1] f32, max_recall [C,T] f32, n_det
    [C,T] int32).  For (c, t) the rows of class c with code != -1, by (score descending, row ascending), give the running
    precision and recall; ``prec[c,t,k-first]`` is the precision envelope at the first row whose recall reaches k / points
    (0 when none does), ``ap`` the mean of max(prec - floor, 0) over k = first .. points, divided by 1 - floor; -1 for a class
    without ground truth.  (40, 1, 0) is KITTI R40, (10, 0, 0) R11, (100, 11, 0.1) nuScenes' recall and precision floors.  The
    order comes from one stable ``torch.sort`` on a key the library writes; everything else is two launches.  N * T < 2^31,
    points <= 128.  No synchronisation; two calls are bit-equal."""
    points, first, floor = int(points), int(first), _f32(floor)
    if not 1 <= points <= 128:
        raise ValueError(f"points: expected 1 .. 128, got {points}")
    if not 0 <= first <= points:
        raise ValueError(f"first: expected 0 .. points, got {first}")
    if not 0.0 <= floor < 1.0:
        raise ValueError(f"floor: expected a value in [0, 1), got {floor}")
    _strict(scores, "scores", torch.float32, (None,), "[N]")
    N = scores.shape[0]
    _strict(labels, "labels", torch.int32, (N,))
    _strict(code, "code", torch.int32, (N, None), f"[N,T] with N = {N} and 1 <= T <= 8")
    T = code.shape[1]
    if not 1 <= T <= 8:
        raise ValueError(f"code: expected [N,T] with 1 <= T <= 8, got {tuple(code.shape)}")
    _strict(n_gt, "n_gt", torch.int32, (None,), "[C] with 1 <= C <= 64")
    C = n_gt.shape[0]
    if not 1 <= C <= 64:
        raise ValueError(f"n_gt: expected [C] with 1 <= C <= 64, got {tuple(n_gt.shape)}")
    if N * T >= 1 << 31:
        raise ValueError(f"code: N * T must stay below 2^31 (got {N} x {T})")
    dev = _head_devices((("scores", scores), ("labels", labels), ("code", code), ("n_gt", n_gt)))
    outs = _outputs(det_ap_output_spec(C, T, points, first), out, dev, "scores")
    workspace = _workspace(max(8 * N, 8), workspace, dev, "ops.det_ap_workspace", 8)
    keys = workspace[:8 * N].view(torch.int64)
    with _timed("det_ap", f"N{N}C{C}T{T}"):
        check(lib().sad_det_ap_keys_f32(scores.data_ptr(), labels.data_ptr(), N, C, keys.data_ptr(), _stream()), "sad_det_ap_keys_f32")
        _unrecordable("det_ap: torch.sort")
        skeys, perm = torch.sort(keys, stable=True)
        a = _lib.DetApArgs()
        a.struct_size = ctypes.sizeof(_lib.DetApArgs)
        a.keys, a.perm, a.code = (skeys.data_ptr(), perm.data_ptr(), code.data_ptr()) if N else (None, None, None)
        a.n_gt = n_gt.data_ptr()
        a.N, a.C, a.T, a.points, a.first, a.floor = N, C, T, points, first, floor
        for n, t in zip(DET_AP_OUTPUTS, outs):
            setattr(a, n, t.data_ptr())
        check(lib().sad_det_ap_f32(ctypes.byref(a), _stream()), "sad_det_ap_f32")
    return outs


# The fused MLP chains (PackedMLP / PackedMLPBf16, grouped_multi, rowscan_multi, the autotuner) live in mlp.py; they belong
# to this operator surface, so their public names are re-exported here (the same objects).
from .mlp import (GroupedCall, PackedMLP, PackedMLPBf16, check_workspace, choose_stage_assignment, cont_buffer,  # noqa: E402,F401
                  grouped_mlp_grad, grouped_multi, mlp_chain, mlp_grad_workspace_bytes, mlp_rows_grad, rowscan_multi, workspace_status)
