"""Host side of the fused MLP chains: ``PackedMLP`` (f32) / ``PackedMLPBf16``, the merged stage dispatch
(``grouped_multi``), the row-packing scan (``rowscan_multi``), split-pooling buffers and the autotuner.

Unlike the operator families of ``ops.py`` (one validated C-ABI call each) this module decides: which kernel runs a
chain, who prepares its pooling buffer, what a recorded step plan (plan.py) must keep alive.  Each mechanism exists once:
``_time_launch`` times a candidate, ``_dispatch`` enqueues and logs a chain dispatch, ``GroupedCall`` is one branch of a
merged dispatch, ``_PackedChain`` holds what the two classes share; each class keeps its kernel choice and tuning policy.
The switches (``AUTOTUNE``, ``LAUNCH_LOG``, ``RERUN_LOG``, ``MERGE_BF16``, ``SPLIT_POOL``) stay in ``ops.py``, where callers
assign them, and are read as ``ops.NAME`` at call time.  ``ops.py`` re-exports the public names of this module.
The backward of the chains (``grouped_mlp_grad`` / ``mlp_rows_grad``, SPEC.md §32) closes the module: one validated C-ABI call
each, on the unpacked layers.
"""
import ctypes
import os
import sys
from typing import Callable, List, NamedTuple, Optional, Sequence, Tuple

import torch

from . import _lib
from ._lib import MlpArgs, check, lib, vp


def rowscan_multi(idxs: Sequence[torch.Tensor], cnts: Sequence[torch.Tensor], N: int,
                  outs: Optional[Sequence[Tuple[torch.Tensor, int, int]]] = None) -> List[torch.Tensor]:
    """Row-packing tables (prefix sum of the per-group counts + row map) of up to four branches of one ball
    query, two launches for all of them.  Needs only what the ball query produced, so it can run on the stream
    that ran the query (the sampling stream), off the MLP stream's critical path; pass table i as the last
    element of branch i's ``grouped_multi`` call (``PackedMLP.grouped(..., ws=table)``).
    ``outs`` = [(out [B,M,ld_out] float32, col_off, C_out)] per branch: the scan also zero-fills the output slice of the
    groups the chain kernels combine with an atomic max, so ``out`` may be UNINITIALISED (``sad_mlp_rowscan_init``).
    Split pooling (bf16 mode): ``outs`` = [(out [B,M,ld_out] bfloat16, col_off, C_out, cont)] with ``cont`` from
    ``cont_buffer`` — nothing is filled, the tables carry what a split-pooled chain and the layer that reads its rows need
    (``sad_mlp_rowscan_split``)."""
    n = len(idxs)
    if n != len(cnts) or not 1 <= n <= _lib.MAX_RADII:
        raise ValueError(f"need 1..{_lib.MAX_RADII} (idx, cnt) pairs")
    B, M = cnts[0].shape
    wss = []
    for idx, cnt in zip(idxs, cnts):
        idx = ops._need(idx, "idx", torch.int32, 3)
        cnt = ops._need(cnt, "cnt", torch.int32, 2)
        if tuple(idx.shape[:2]) != (B, M) or tuple(cnt.shape) != (B, M):
            raise ValueError("idx / cnt shapes do not match")
        wss.append(ops._empty((lib().sad_mlp_workspace_bytes(B, M, idx.shape[2]),), dtype=torch.uint8, device=idx.device))
    c_arr = (vp * n)(*[c.data_ptr() for c in cnts])
    i_arr = (vp * n)(*[i.data_ptr() for i in idxs])
    s_arr = (ctypes.c_int * n)(*[int(i.shape[2]) for i in idxs])
    w_arr = (vp * n)(*[w.data_ptr() for w in wss])
    if outs is None:
        check(lib().sad_mlp_rowscan(n, c_arr, i_arr, s_arr, B, int(N), M, w_arr, ops._stream()), "sad_mlp_rowscan")
        return wss
    if len(outs) != n:
        raise ValueError("outs: one (out, col_off, C_out) per branch")
    if any(len(o) > 3 for o in outs):
        if not all(len(o) == 4 and o[3] is not None and o[0].dtype == torch.bfloat16 for o in outs):
            raise ValueError("outs: split pooling needs (bfloat16 out, col_off, C_out, cont) for EVERY branch of the scan")
        for (o, off, co, cont), idx in zip(outs, idxs):
            if tuple(o.shape[:2]) != (B, M) or not o.is_contiguous() or off < 0 or off + co > o.shape[2]:
                raise ValueError("outs: need contiguous [B,M,ld_out] buffers with col_off + C_out <= ld_out")
            if cont.numel() * cont.element_size() < lib().sad_mlp_cont_bytes(B, M, int(idx.shape[2]), int(co)):
                raise ValueError("outs: continuation buffer too small (ops.cont_buffer)")
        k_arr = (vp * n)(*[o[3].data_ptr() for o in outs])
        co_arr = (ctypes.c_int * n)(*[int(o[2]) for o in outs])
        check(lib().sad_mlp_rowscan_split(n, c_arr, i_arr, s_arr, B, int(N), M, w_arr, k_arr, co_arr, ops._stream()), "sad_mlp_rowscan_split")
        for w in wss:
            w._sad_split = True
        return wss
    for o, off, co in outs:
        o = ops._need(o, "out", torch.float32, 3)
        if tuple(o.shape[:2]) != (B, M) or not o.is_contiguous() or off < 0 or off + co > o.shape[2]:
            raise ValueError("outs: need contiguous [B,M,ld_out] float32 buffers with col_off + C_out <= ld_out")
    o_arr = (vp * n)(*[o.data_ptr() for o, _, _ in outs])
    ld_arr = (ctypes.c_int * n)(*[int(o.shape[2]) for o, _, _ in outs])
    off_arr = (ctypes.c_int * n)(*[int(off) for _, off, _ in outs])
    co_arr = (ctypes.c_int * n)(*[int(co) for _, _, co in outs])
    check(lib().sad_mlp_rowscan_init(n, c_arr, i_arr, s_arr, B, int(N), M, w_arr, o_arr, ld_arr, off_arr, co_arr, ops._stream()),
          "sad_mlp_rowscan_init")
    return wss


def cont_buffer(B: int, M: int, S: int, cout: int, device) -> torch.Tensor:
    """Continuation rows of one split-pooled bf16 chain (``sad_mlp_cont_bytes``; include/sad_amd.h ``sad_mlp_bf16_args.cont``)."""
    return ops._empty((lib().sad_mlp_cont_bytes(int(B), int(M), int(S), int(cout)),), dtype=torch.uint8, device=device)


_ITEMQ_INTS = 2 + 32 * 8      # csrc/common.h: a table carries the per-XCD item queues (and these ints) only when it has this many row starts


def workspace_status(ws: torch.Tensor, n_groups: Optional[int] = None) -> dict:
    """Instrumentation ints of a row-packing table (include/sad_amd.h, SAD_WS_*): weight-ring refills of the
    cooperative chain kernel, the id of the dispatch that owns the item queues right now and the conflict flag of the
    ``mlp_check_inuse`` knob.  Synchronises the device (a test / debugging helper, never on the measured path).
    ``n_groups`` = B * M of the table: a table with fewer than 258 row starts has no item queues (the kernels deal such
    launches statically) and ints 5..7 hold row starts there, so zeros are reported; pass it whenever the table may be small."""
    if n_groups is not None and n_groups + 1 < _ITEMQ_INTS:
        return {"refills": 0, "in_use": 0, "conflict": 0}
    torch.cuda.synchronize(ws.device)
    hdr = ws[:32].view(torch.int32).cpu()
    return {"refills": int(hdr[_lib.WS_REFILLS]), "in_use": int(hdr[_lib.WS_INUSE]), "conflict": int(hdr[_lib.WS_CONFLICT])}


def check_workspace(ws: torch.Tensor, n_groups: Optional[int] = None) -> None:
    """Raises if two dispatches were seen sharing ``ws`` at the same time (needs ``mlp_check_inuse=1``)."""
    st = workspace_status(ws, n_groups)
    if st["conflict"]:
        raise RuntimeError("row-packing workspace was used by two dispatches at the same time (one dispatch at a time per "
                           "workspace: sad_mlp_args.workspace in include/sad_amd.h)")


def _time_launch(enqueue: Callable[[], int], stream) -> Optional[float]:
    """ms per launch of ``enqueue`` (enqueues the dispatch once, returns the library's code) on ``stream``; None if the
    library refuses it (does not fit LDS / not valid for this nsample).  One warm launch, then the faster of two timed
    batches of four — single batches of three picked different winners from run to run."""
    if enqueue() != 0:
        return None
    stream.synchronize()
    times = []
    for _ in range(2):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(4):
            enqueue()
        e1.record(stream)
        stream.synchronize()
        times.append(e0.elapsed_time(e1) / 4)
    return min(times)


def _dispatch(label: str, fn_name: str, enqueue: Callable[[], int], alive, retry: Optional[Callable[[], bool]] = None) -> None:
    """One chain dispatch: ``enqueue`` inside the ``LAUNCH_LOG`` bracket, its code checked under ``fn_name``, and one ``RERUN_LOG``
    entry (label, fn): fn() enqueues the SAME dispatch again; the entry keeps ``alive`` (tensors the dispatch reads or writes)
    and what ``enqueue`` closes over (argument blocks, pointer array).  ``retry``: asked when the library answers -2
    (unsupported); True = it adjusted the argument blocks, enqueue again (inside the same bracket)."""
    with ops._timed("mlp", label):
        rc = enqueue()
        if rc == -2 and retry is not None and retry():
            rc = enqueue()
        check(rc, fn_name)
    if ops.RERUN_LOG is not None:
        ops.RERUN_LOG.append((label, lambda alive=alive: check(enqueue(), fn_name)))


class _PackedChain:
    """What ``PackedMLP`` and ``PackedMLPBf16`` share: the uploaded layers, the argument block, the shape key of the
    autotuner, and the validation of a grouped call / of plain rows.  A subclass names its argument block (``_ARGS``), the
    C-ABI function of a chain (``_CHAIN``), those that size and pack the weights (``_PACK``, into ``_PACK_DTYPE``), and has
    ``_takes_table(geometry)``: does this kernel consume a caller-made row-packing table?  ``_feat_fits(feat_pm)``: can those
    kernels read the feature rows?  ``_fresh_fits(C, dtype)``: the same for a fresh contiguous [B,N,C] tensor."""

    def _upload(self, layers, first_has_xyz: bool, device, relu_mask: Optional[int], name: str):
        """-> the layers' (weights, biases) as float32 GPU tensors."""
        self.name = name
        self._geom = {}              # shape key (_key) -> geometry picked by the autotuner (bf16: rows per tile, or 2)
        # used for shapes never tuned (0 = built-in heuristic of the tiled kernel); see SADDetector.set_geometry
        self.default_geometry = 0
        if not 1 <= len(layers) <= _lib.MAX_LAYERS:
            raise ValueError(f"1..{_lib.MAX_LAYERS} layers supported")
        self.device = torch.device(device)
        ws = [torch.as_tensor(w, dtype=torch.float32).to(self.device).contiguous() for w, _ in layers]
        bs = [torch.as_tensor(b, dtype=torch.float32).to(self.device).contiguous() for _, b in layers]
        self.dims = [ws[0].shape[1]] + [w.shape[0] for w in ws]
        for a, b in zip(ws[:-1], ws[1:]):
            if b.shape[1] != a.shape[0]:
                raise ValueError("layer shapes do not chain")
        self.L = len(ws)
        self.first_has_xyz = bool(first_has_xyz)
        self.relu_mask = (1 << self.L) - 1 if relu_mask is None else int(relu_mask)
        self.pack_dims = list(self.dims)     # the dims the library sees (PackedMLP may pad them)
        self.out_channels = self.dims[-1]
        return ws, bs

    def _pack(self, ws, bs):
        """Repack the layers into ``self.packed`` (MFMA fragment order); -> ``pack_dims`` as a C array."""
        dims_c = (ctypes.c_int * (self.L + 1))(*self.pack_dims)
        size_fn, pack_fn = self._PACK
        n = getattr(lib(), size_fn)(self.L, dims_c, int(self.first_has_xyz))
        self.packed = ops._empty((n,), dtype=self._PACK_DTYPE, device=self.device)
        w_arr = (vp * self.L)(*[w.data_ptr() for w in ws])
        b_arr = (vp * self.L)(*[b.data_ptr() for b in bs])
        with torch.cuda.device(self.device):
            check(getattr(lib(), pack_fn)(self.L, dims_c, int(self.first_has_xyz), w_arr, b_arr,
                                          self.packed.data_ptr(), ops._stream()), pack_fn)
            torch.cuda.current_stream().synchronize()  # ws/bs may be freed after this returns
        return dims_c

    def _args(self):
        a = self._ARGS()
        a.struct_size = ctypes.sizeof(self._ARGS)
        a.L = self.L
        for i, d in enumerate(self.pack_dims):
            a.dims[i] = d
        a.packed = self.packed.data_ptr()
        a.relu_mask = self.relu_mask
        return a

    @staticmethod
    def _key(a) -> tuple:        # the shape a geometry is tuned for
        return (bool(a.idx), a.B, a.N, a.M, a.S, a.ld_out)

    def _enqueue(self, a) -> Callable[[], int]:
        return lambda: getattr(lib(), self._CHAIN)(ctypes.byref(a), ops._stream())

    def _grouped_prologue(self, xyz, feat_pm, new_xyz, idx):
        """The operands of a grouped call, validated, in a fresh argument block -> (a, keep, xyz, feat_pm) with
        ``keep`` the tensors the block points into.  ``_feat_arg`` is the class's own rule for the feature tensor."""
        if not self.first_has_xyz:
            raise RuntimeError(f"this {type(self).__name__} was packed without the xyz prefix")
        xyz = ops._need(xyz, "xyz", torch.float32, 3)
        new_xyz = ops._need(new_xyz, "new_xyz", torch.float32, 3)
        idx = ops._need(idx, "idx", torch.int32, 3)
        B, N, _ = xyz.shape
        _, M, S = idx.shape
        a = self._args()
        keep = [xyz, new_xyz, idx]
        C = 0
        if feat_pm is not None:
            self._feat_arg(a, feat_pm)
            if feat_pm.stride(2) != 1 or feat_pm.stride(0) != N * feat_pm.stride(1):
                ops._unrecordable("feat_pm: strided copy")
                feat_pm = feat_pm.contiguous()
            C = feat_pm.shape[2]
            a.feat, a.ld_feat = feat_pm.data_ptr(), feat_pm.stride(1)
            keep.append(feat_pm)
        if self.dims[0] != C + 3:
            raise ValueError(f"MLP expects {self.dims[0] - 3} feature channels, got {C}")
        a.xyz, a.new_xyz, a.idx = xyz.data_ptr(), new_xyz.data_ptr(), idx.data_ptr()
        a.B, a.N, a.M, a.S, a.C = B, N, M, S, C
        return a, keep, xyz, feat_pm

    def _zero_out(self, a, device) -> torch.Tensor:   # (the kernel max-combines into the buffer: it must start at zero)
        ops._unrecordable("grouped: zero-filled output")
        return torch.zeros((a.B, a.M, self.out_channels), dtype=torch.float32, device=device)

    def _counts_and_table(self, a, keep, cnt, ws, device) -> None:
        """``cnt`` [B,M] int32 from ball_query_multi(return_counts=True); ``ws``: a fresh table (the chain scans the counts itself)
        or the caller's, already filled by ``rowscan_multi`` (the table kernels then launch no scan)."""
        cnt = ops._need(cnt, "cnt", torch.int32, 2)
        if tuple(cnt.shape) != (a.B, a.M):
            raise ValueError("cnt must be [B,M]")
        nbytes = lib().sad_mlp_workspace_bytes(a.B, a.M, a.S)
        if ws is None:
            ws = ops._empty((nbytes,), dtype=torch.uint8, device=device)
        else:
            if ws.numel() < nbytes:
                raise ValueError("ws: too small for this (B, M, S)")
            a.prescanned = 1
        a.cnt, a.workspace = cnt.data_ptr(), ws.data_ptr()   # global row packing
        keep += [cnt, ws]

    def _pick_geometry(self, a, prefer: bool, forced: int = 0) -> None:
        """``forced``, else the tuned geometry of the shape, else the default; an un-tuned call gets the kernel the library
        prefers when it comes with counts and features the table kernels can read (``prefer``).
        Backstop: a caller-made table means the caller's scan prepared `out` for a table kernel (only the groups those
        kernels combine atomically were zeroed); the tiled kernel packs for itself and max-combines into memory it
        expects to be zero — never run it on such a buffer."""
        a.geometry = forced or self._geom.get(self._key(a)) or self.default_geometry
        if not a.geometry and prefer and not ops.AUTOTUNE:
            a.geometry = self.preferred_geometry
        if a.prescanned and not self._takes_table(a.geometry):
            raise RuntimeError(f"{self.name or type(self).__name__}: a row-packing table (ws) was passed but geometry {a.geometry} packs for "
                               "itself; ask wants_prescan(..., feat=<the feature tensor>) before making the table")

    def wants_prescan(self, B: int, N: int, M: int, S: int, ld_out: int, C: int, feat: Optional[torch.Tensor] = None,
                      feat_dtype=None) -> bool:
        """Will a grouped call of this shape (with counts) run a kernel that consumes a caller-made row-packing table
        (f32: geometries 2 / 3 / 4, bf16: 2)?  The tiled kernel packs with its own tile height: a table made for it would be
        wasted — and it expects a ZERO pooling buffer, which the scan does not give it.  ``feat``: the feature tensor the call
        will get ([B,N,C] point-major, any stride); None = a fresh contiguous [B,N,C] tensor (a stage output) of ``feat_dtype``
        (default: the chain's own, float32 / bfloat16).  The same ``_feat_fits`` rule decides in ``_grouped_args``."""
        geom = self._geom.get((True, B, N, M, S, ld_out)) or self.default_geometry
        if feat is None:
            fits = self._fresh_fits(C, feat_dtype)
        else:
            fits = feat.dim() == 3 and feat.stride(2) == 1 and feat.stride(0) == N * feat.stride(1) and self._feat_fits(feat)
        if not geom and not ops.AUTOTUNE and fits:
            geom = self.preferred_geometry
        return self._takes_table(geom)

    def _rows_input(self, x: torch.Tensor):
        """x [..., C] of plain rows -> (x2 [R, C] with unit last-dim stride, R, C)."""
        C = x.shape[-1]
        if C != self.dims[0]:
            raise ValueError(f"MLP expects {self.dims[0]} channels, got {C}")
        if not x.is_contiguous():
            ops._unrecordable("rows: strided input")
        x2 = x.reshape(-1, C)
        if x2.stride(1) != 1:
            x2 = x2.contiguous()
        return x2, x2.shape[0], C

    @staticmethod
    def _rows_args(a, x2, out, col_off) -> None:
        a.feat, a.ld_feat = x2.data_ptr(), x2.stride(0)
        a.B, a.N, a.M, a.S, a.C = 1, 0, x2.shape[0], 1, x2.shape[1]
        a.out, a.ld_out, a.col_off = out.data_ptr(), out.stride(-2), col_off


class PackedMLP(_PackedChain):
    """A shared-MLP chain (SPEC.md §6) with weights repacked once into MFMA A-fragment order.

    ``layers`` = [(W [C_out,C_in], b [C_out]), ...] as numpy arrays or tensors (BatchNorm already
    folded).  ``first_has_xyz``: the first layer's input is [rel_xyz(3) ‖ features(C_in-3)].
    ``relu_mask`` bit l = ReLU after layer l (default: all layers).
    """
    _ARGS, _CHAIN = MlpArgs, "sad_mlp_chain_f32"
    _PACK, _PACK_DTYPE = ("sad_mlp_packed_floats", "sad_mlp_pack_f32"), torch.float32

    def __init__(self, layers, first_has_xyz: bool, device, relu_mask: Optional[int] = None,
                 name: str = ""):
        # grouped calls that come with counts (cnt) and are not tuned use the kernel the library prefers for the shape
        # (register-resident / cooperative / layer-streamed chain; 0 = tiled): the un-tuned path is then within a few per
        # cent of the tuned one on the benchmark shapes
        self.preferred_geometry = 0
        ws, bs = self._upload(layers, first_has_xyz, device, relu_mask, name)
        # A grouped 3-layer chain that is not a compiled shape of the register-resident kernels but is DOMINATED by one (every
        # width <= the shape's, at most 1.6 x the flops) is packed zero-padded onto that shape and runs there: `pack_dims` are the
        # dims the library sees, `dims` stay the chain's own (sad_mlp_args.c_out, ABI 3; DESIGN.md 6, generality table)
        if self.first_has_xyz and self.L == 3 and self.relu_mask == (1 << self.L) - 1:
            pad_c = (ctypes.c_int * (self.L + 1))()
            if lib().sad_mlp_padded_dims(self.L, (ctypes.c_int * (self.L + 1))(*self.dims), pad_c):
                self.pack_dims = [int(v) for v in pad_c]
                for l in range(self.L):
                    w2 = torch.zeros((self.pack_dims[l + 1], self.pack_dims[l]), dtype=torch.float32, device=self.device)
                    w2[:ws[l].shape[0], :ws[l].shape[1]] = ws[l]
                    b2 = torch.zeros((self.pack_dims[l + 1],), dtype=torch.float32, device=self.device)
                    b2[:bs[l].shape[0]] = bs[l]
                    ws[l], bs[l] = w2.contiguous(), b2
        self.padded = self.pack_dims != self.dims
        dims_c = self._pack(ws, bs)
        if self.first_has_xyz:
            self.preferred_geometry = int(lib().sad_mlp_preferred_geometry(self.L, dims_c))
        # geometry 3 (layer-streamed chain, csrc/mlp_layer.hip) applies when every layer's padded width is a
        # multiple of 128 channels; it needs scratch for the activations between layers
        # (plain rows: also C % 8 == 0 and an unpadded C_out, whole 128-channel blocks are stored)
        wide = all(((d + 31) // 32 * 32) % 128 == 0 for d in self.dims[1:])
        self._layered_ok = (not self.padded) and wide and (self.first_has_xyz or (self.dims[0] % 8 == 0 and self.dims[-1] % 128 == 0))

    # Geometries tried by the autotuner: W*100 + log2(WN)*10 + RW (include/sad_amd.h, sad_mlp_args).
    _CANDIDATES = [w * 100 + n * 10 + r for w in (8, 4) for n in range(4) if (1 << n) <= w
                   for r in (1, 2, 4)] + [1600 + n * 10 + r for n in (3, 4) for r in (1, 2)] \
        + [100000 + w * 100 + n * 10 + 1 for w in (8, 4) for n in range(3) if (2 << n) <= w] \
        + [200000 + w * 100 + n * 10 + 1 for w in (8, 4) for n in range(4) if (1 << n) <= w] \
        + [300000 + w * 100 + n * 10 + 1 for w in (8, 4) for n in range(3) if (2 << n) <= w]
    # +100000 flexible item distribution, +200000 two output tiles per wave, +300000 both
    _F_CODES = (2, 4, 5, 6)      # grouped mode: 2^f * R / S groups per workgroup (default f = 3)

    @staticmethod
    def _takes_table(geom: int) -> bool:     # register-resident (2), layer-streamed (3) and cooperative (4) chains
        return geom % 1000 in (2, 3, 4)

    def _launch(self, a: MlpArgs, keep=None) -> None:
        """Enqueue the chain.  With AUTOTUNE on, the first call for a shape times every workgroup
        geometry that fits (a few ms, synchronous) and the fastest one is reused afterwards."""
        key = self._key(a)
        geom = self._geom.get(key)
        if geom is None and ops.AUTOTUNE:
            geom = self._tune(a)
            self._geom[key] = geom
        a.geometry = geom or self.default_geometry or a.geometry      # (a.geometry: the preferred kernel of an un-tuned grouped call)
        _dispatch(self.name, self._CHAIN, self._enqueue(a), keep, retry=lambda: self._drop_untuned_pick(a, geom))

    def _drop_untuned_pick(self, a: MlpArgs, tuned) -> bool:
        """After a refusal: the library's un-tuned pick for the tiled kernel does not fit LDS for this (S, widths): its built-in heuristic."""
        if tuned or self.default_geometry or a.geometry <= 5:
            return False
        self.preferred_geometry = 0
        a.geometry = 0
        return True

    def _tune(self, a: MlpArgs) -> int:
        stream = torch.cuda.current_stream()
        enqueue = self._enqueue(a)

        def time(code: int) -> Optional[float]:
            a.geometry = code
            return _time_launch(enqueue, stream)
        best, best_ms = 0, None
        # 1 = VALU row-per-lane kernel (narrow chains), 2 = register-resident chain kernel (csrc/mlp_reg.hip),
        # 3 = layer-streamed chain (csrc/mlp_layer.hip), 4 = cooperative register-resident chain (csrc/mlp_coop.hip)
        # ... 5 = row-streaming plain layer (csrc/mlp_rows.hip)
        plain_extra = ([3] if self._layered_ok else []) + ([5] if self.L == 1 and self.dims[0] % 8 == 0 else [])
        for code in self._CANDIDATES + ([1] if a.idx else plain_extra):
            ms = time(code)
            if ms is not None and (best_ms is None or ms < best_ms * 0.98):   # prefer earlier entries on ties
                best, best_ms = code, ms
        # The kernels that consume a row-packing table (2 / 3 / 4) are timed apart and WIN unless the tiled kernel is more than
        # 10 % faster: a tiled pick for one chain of a stage costs what this timing does not see — its pooling buffer must be
        # zero-filled (a framework kernel: the step cannot be recorded into a plan any more, plan.py), its branch leaves the
        # stage's merged dispatch and its scan.  The cluster branch 259 -> 256 -> 256 -> 512 is within 2 - 3 % either way:
        # two of eleven runs of round 5 picked the tiled kernel for it and lost 7 % (f32), 8 % (the pipeline leg that shares
        # the geometry) of the step — very likely also the low readings round 4 could not explain.
        if a.idx and a.cnt and a.workspace:
            t_best, t_ms = 0, None
            for code in (2, 3, 4):
                ms = time(code)
                if ms is not None and (t_ms is None or ms < t_ms * 0.98):
                    t_best, t_ms = code, ms
            if os.environ.get("SAD_TUNE_DEBUG"):
                print(f"[tune] {self.name}: tiled {best} {best_ms}, table {t_best} {t_ms}", file=sys.stderr, flush=True)
            if t_ms is not None and (best_ms is None or t_ms <= best_ms * 1.10):
                return t_best
        if a.idx and best > 4:   # second sweep: groups per workgroup (how much padding is expected)
            base = best
            for f in self._F_CODES:
                ms = time(base + 1000 * f)
                if ms is not None and ms < best_ms * 0.98:
                    best, best_ms = base + 1000 * f, ms
            if a.cnt and a.workspace:   # third sweep: global row packing (1) vs per-workgroup packing (2)
                base, found = best, None
                for d in (1, 2):
                    ms = time(base + 10000 * d)
                    if ms is not None and (found is None or ms < found[1]):
                        found = (base + 10000 * d, ms)
                if found is not None:
                    best = found[0]
        return best

    def _args(self) -> MlpArgs:
        a = super()._args()
        a.c_out = self.dims[-1] if self.padded else 0       # (a zero-padded chain stores only its own output channels)
        return a

    @staticmethod
    def feat_fits_table_kernels(C: int, ld_feat: int, ptr: int) -> bool:
        """Can the register-resident / layer-streamed / cooperative kernels read feature rows of this layout?  They fetch
        16-byte chunks (C % 4 == 0, row stride % 4 == 0, 16-byte aligned base); a single strided channel (or none) is the
        other layout they take.  The ONE predicate behind ``wants_prescan`` and ``_grouped_args``: the first decides who
        prepares the pooling buffer, the second which kernel runs, and they must agree."""
        return C <= 1 or (C % 4 == 0 and ld_feat % 4 == 0 and ptr % 16 == 0)

    def _feat_fits(self, feat_pm) -> bool:
        return feat_pm is None or self.feat_fits_table_kernels(feat_pm.shape[2], feat_pm.stride(1), feat_pm.data_ptr())

    def _fresh_fits(self, C: int, dtype) -> bool:
        return self.feat_fits_table_kernels(C, C, 0)

    def grouped(self, xyz: torch.Tensor, feat_pm: Optional[torch.Tensor], new_xyz: torch.Tensor,
                idx: torch.Tensor, out: Optional[torch.Tensor] = None, col_off: int = 0,
                cnt: Optional[torch.Tensor] = None, ws: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Fused group -> MLP -> max over nsample.  xyz [B,N,3]; feat_pm point-major [B,N,C] (or
        None); new_xyz [B,M,3]; idx [B,M,S].  Writes out[:, :, col_off:col_off+C_out] of a
        point-major [B,M,ld_out] buffer (allocated [B,M,C_out] when ``out`` is None).  A caller-
        provided ``out`` slice must be ZERO on entry (groups spanning two row tiles are combined
        with an atomic max).  Samples that repeat a group's first index are skipped.  ``ws``: the
        row-packing table of (idx, cnt) from ``rowscan_multi`` (else the chain scans the counts itself)."""
        a, out, _keep = self._grouped_args(xyz, feat_pm, new_xyz, idx, out, col_off, cnt, ws)
        self._launch(a, _keep + [out])
        return out

    @staticmethod
    def _feat_arg(a, feat_pm) -> None:
        if not feat_pm.is_cuda or feat_pm.dtype != torch.float32 or feat_pm.dim() != 3:
            raise TypeError("feat_pm: expected a GPU float32 [B,N,C] tensor")

    def _grouped_args(self, xyz, feat_pm, new_xyz, idx, out, col_off, cnt, ws=None):
        """Validated ``MlpArgs`` of a grouped call + the output tensor + tensors to keep alive."""
        a, keep, xyz, feat_pm = self._grouped_prologue(xyz, feat_pm, new_xyz, idx)
        # (the register-resident / layer-streamed kernels read feature rows as 16-byte chunks; a single strided
        # channel is the other layout they take)
        feat_ok16 = self._feat_fits(feat_pm)
        if self.padded:
            # a zero-padded chain runs on the register-resident kernels only: they take counts and 16-byte feature rows
            if cnt is None:
                ops._unrecordable("padded chain: counts derived from idx")
                pos = torch.arange(1, a.S + 1, device=idx.device, dtype=torch.int32)
                cnt = torch.clamp(((idx != idx[..., :1]).to(torch.int32) * pos).amax(-1), min=1).to(torch.int32).contiguous()
            if not feat_ok16:
                ops._unrecordable("padded chain: packed copy of the features")
                feat_pm = feat_pm.contiguous()
                a.feat, a.ld_feat = feat_pm.data_ptr(), feat_pm.stride(1)
                keep.append(feat_pm)
                feat_ok16 = self._feat_fits(feat_pm)
        out = self._zero_out(a, xyz.device) if out is None else out
        if self.relu_mask != (1 << self.L) - 1:
            raise RuntimeError("grouped chains need a ReLU after every layer (max-pool combine)")
        self._check_out(out, a.B * a.M, col_off)
        if cnt is not None:
            self._counts_and_table(a, keep, cnt, ws, xyz.device)
        a.out, a.ld_out, a.col_off = out.data_ptr(), out.stride(-2), col_off
        self._pick_geometry(a, cnt is not None and feat_ok16)
        if self._layered_ok and cnt is not None and (a.geometry == 3 or ops.AUTOTUNE):
            self._scratch(a, keep, xyz.device)
        return a, out, keep

    def _scratch(self, a: MlpArgs, keep: list, device) -> None:
        """Scratch of the layer-streamed chain: the activations between the layer launches (``_layered_ok``: dims are not padded)."""
        nbytes = lib().sad_mlp_scratch_bytes(a.B, a.M, a.S, self.L, (ctypes.c_int * (self.L + 1))(*self.dims))
        sc = ops._empty((nbytes,), dtype=torch.uint8, device=device)
        a.scratch, a.scratch_bytes = sc.data_ptr(), nbytes
        keep.append(sc)

    def rows(self, x: torch.Tensor, out: Optional[torch.Tensor] = None, col_off: int = 0
             ) -> torch.Tensor:
        """Plain rows.  x [..., C] point-major (last-dim stride 1) -> [..., C_out]."""
        if self.first_has_xyz:
            raise RuntimeError("this PackedMLP was packed with the xyz prefix")
        if not x.is_cuda or x.dtype != torch.float32:
            raise TypeError("x: expected a GPU float32 tensor")
        ops._on_current_device(x, "x")
        x2, R, C = self._rows_input(x)
        if out is None:
            out = ops._empty(tuple(x.shape[:-1]) + (self.out_channels,), dtype=torch.float32,
                             device=x.device)
        self._check_out(out, R, col_off)
        a = self._args()
        self._rows_args(a, x2, out, col_off)
        geom = self._geom.get(self._key(a)) or self.default_geometry
        keep = [x2, out]
        if self._layered_ok and self.L > 1 and (geom == 3 or ops.AUTOTUNE):
            self._scratch(a, keep, x.device)
        self._launch(a, keep)
        return out

    def _check_out(self, out: torch.Tensor, rows: int, col_off: int) -> None:
        if not out.is_cuda or out.dtype != torch.float32 or out.stride(-1) != 1:
            raise TypeError("out: expected a GPU float32 tensor with unit last-dim stride")
        if out.numel() // out.shape[-1] != rows or not out.is_contiguous():
            raise ValueError("out: expected a contiguous [rows, ld_out] buffer")
        if col_off < 0 or col_off + self.out_channels > out.shape[-1]:
            raise ValueError("out: col_off + C_out exceeds the buffer width")


class GroupedCall(NamedTuple):
    """One branch of a ``grouped_multi`` dispatch: the chain and the arguments of its ``grouped`` call.  ``ws``: row-packing
    table from ``rowscan_multi``; ``cont``: continuation rows of a split-pooled bf16 chain (``cont_buffer``)."""
    mlp: _PackedChain
    xyz: torch.Tensor
    feat_pm: Optional[torch.Tensor]
    new_xyz: torch.Tensor
    idx: torch.Tensor
    out: torch.Tensor
    col_off: int
    cnt: Optional[torch.Tensor]
    ws: Optional[torch.Tensor] = None
    cont: Optional[torch.Tensor] = None

    def args(self, table: bool = True):
        """``mlp._grouped_args`` of this call (``table`` False: without the caller's table — the chain scans for itself).
        ``cont`` is handed on only when set: split pooling is for bf16 chains, an f32 chain refuses the argument."""
        more = {} if self.cont is None or not table else {"cont": self.cont}
        return self.mlp._grouped_args(self.xyz, self.feat_pm, self.new_xyz, self.idx, self.out, self.col_off, self.cnt,
                                      self.ws if table else None, **more)


def _multi(calls, args):
    """(C-ABI function name, enqueue) of ONE dispatch of the argument blocks ``args`` of ``calls`` (all f32 or all bf16)."""
    bf16 = isinstance(calls[0].mlp, PackedMLPBf16)
    fn_name = "sad_mlp_chain_multi_bf16" if bf16 else "sad_mlp_chain_multi_f32"
    arr = (ctypes.POINTER(_lib.MlpBf16Args if bf16 else MlpArgs) * len(args))(*[ctypes.pointer(a) for a in args])
    return fn_name, lambda: getattr(lib(), fn_name)(arr, len(args), ops._stream())


def grouped_multi(calls) -> None:
    """Several independent fused group -> MLP -> max launches (the branches of one multi-radius
    stage) as ONE dispatch (``sad_mlp_chain_multi_f32``): the light chains fill the tail of the
    heavy one.  ``calls`` = [GroupedCall(mlp, xyz, feat_pm, new_xyz, idx, out, col_off, cnt[, ws[, cont]]), ...] (or plain
    tuples in that order) with caller-provided zero ``out`` buffers (``ws``: row-packing table from ``rowscan_multi``).
    While autotuning, or for a single call, each chain is launched (and tuned) on its own."""
    calls = [GroupedCall(*c) for c in calls]
    if ops.AUTOTUNE or len(calls) < 2 or (not ops.MERGE_BF16 and isinstance(calls[0].mlp, PackedMLPBf16)):
        for c in calls:
            more = {} if c.cont is None else {"ws": c.ws, "cont": c.cont}
            c.mlp.grouped(c.xyz, c.feat_pm, c.new_xyz, c.idx, out=c.out, col_off=c.col_off, cnt=c.cnt, **more)
        if ops.AUTOTUNE and len(calls) >= 2:
            _tune_stage(calls)
        return
    args, keep = [], []
    for c in calls:
        a, _, k = c.args()
        args.append(a)
        keep.append(k)
    bf16 = isinstance(calls[0].mlp, PackedMLPBf16)
    if any(isinstance(c.mlp, PackedMLPBf16) != bf16 for c in calls):
        raise TypeError("grouped_multi: all chains must be of the same class (f32 or bf16)")
    _rec = _lib.recorder()
    if _rec is not None:             # (a recorded step replays this dispatch: its argument blocks live as long as the plan)
        _rec.keep.append((args, keep))
    fn_name, enqueue = _multi(calls, args)
    _dispatch("+".join(c.mlp.name for c in calls), fn_name, enqueue, (keep, [c.out for c in calls]),
              retry=None if bf16 else lambda: any([c.mlp._drop_untuned_pick(a, c.mlp._geom) for a, c in zip(args, calls)]))


def choose_stage_assignment(picked, t_picked, uniform_times, table=(2, 3, 4)):
    """The stage-level decision of the autotuner as a pure function (CPU-testable).  ``picked`` = per-chain codes with the measured
    time ``t_picked`` of their merged dispatch; ``uniform_times`` = {table code: time of the dispatch with every chain on it, or
    None when refused}.  Among the uniform assignments the fastest wins (an earlier code keeps a tie within 2 %).  It replaces
    per-chain picks that are all table kernels when it is 2 % faster — and picks with a TILED kernel among them unless those are
    more than 10 % faster: a tiled branch needs its pooling slice zero-filled by a framework kernel (the step can no longer be
    replayed from a plan), leaves the stage's scan and its merged dispatch, none of which this timing sees."""
    u_best, u_t = None, None
    for code in table:
        t = uniform_times.get(code)
        if t is not None and (u_t is None or t < u_t * 0.98):
            u_best, u_t = code, t
    all_table = all(p in table for p in picked)
    if u_t is not None:
        if (all_table and (t_picked is None or u_t < t_picked * 0.98)) or (not all_table and (t_picked is None or u_t <= t_picked * 1.10)):
            return [u_best] * len(picked), u_t
    return list(picked), t_picked


def _tune_stage(calls) -> None:
    """Stage-level autotune step: the branches of a stage go out as ONE dispatch, and register-resident
    (geometry 2) / layer-streamed (geometry 3) chains share their launches and work lists, so a branch
    that is slower on its own (few tiles) may still be best inside the merged dispatch.  Times the merged
    dispatch with the per-chain picks against all-2 and all-3 and keeps the fastest assignment.  (The chains scan
    for themselves here: the callers' tables and continuation rows are not used.)"""
    calls = [GroupedCall(*c) for c in calls]
    stream = torch.cuda.current_stream()
    bf16 = isinstance(calls[0].mlp, PackedMLPBf16)
    keys = [c.mlp._key(c.args(table=False)[0]) for c in calls]

    def run(codes):
        args, keep = [], []
        for c, code in zip(calls, codes):
            a, _, k = c.args(table=False)
            a.geometry = code
            args.append(a)
            keep.append(k)
        return _time_launch(_multi(calls, args)[1], stream)

    picked = [c.mlp._geom.get(k) or 0 for c, k in zip(calls, keys)]
    table = (2,) if bf16 else (2, 3, 4)          # the kernels whose chains share launches (f32: register-resident, layer-streamed, cooperative)
    all_table = all(p in table for p in picked)
    t_picked = run(picked)
    uniform = {}
    for code in table:
        uniform[code] = t_picked if (all_table and all(p == code for p in picked)) else run([code] * len(calls))
    best, t_best = choose_stage_assignment(picked, t_picked, uniform, table)
    if os.environ.get("SAD_TUNE_DEBUG"):
        print(f"[tune-stage] {'+'.join(c.mlp.name for c in calls)}: picked {picked} {t_picked}, uniform {uniform}, final {best} {t_best}", file=sys.stderr, flush=True)
    for c, k, code in zip(calls, keys, best):
        c.mlp._geom[k] = code


class PackedMLPBf16(_PackedChain):
    """The same chain in bfloat16 on the matrix cores (SPEC.md §14, BASELINE.json configs[4]).

    Weights are rounded to bf16 once and stored in MFMA fragment order; features are bf16 tensors
    (float32 accepted and rounded on load); accumulation is float32.  Grouped output is float32
    (pooled), plain output float32 or bfloat16.  Dense rows — ball-query padding is computed."""
    _ARGS, _CHAIN = _lib.MlpBf16Args, "sad_mlp_chain_bf16"
    _PACK, _PACK_DTYPE = ("sad_mlp_packed_bytes_bf16", "sad_mlp_pack_bf16"), torch.uint8

    def __init__(self, layers, first_has_xyz: bool, device, relu_mask: Optional[int] = None,
                 name: str = ""):
        dims_c = self._pack(*self._upload(layers, first_has_xyz, device, relu_mask, name))
        # grouped calls that come with counts use the register-resident chain kernel (geometry 2, csrc/mlp_bf16_reg.hip)
        # where the library has the shape compiled
        self.preferred_geometry = int(lib().sad_mlp_preferred_geometry_bf16(self.L, dims_c)) if self.first_has_xyz else 0

    @staticmethod
    def _takes_table(geom: int) -> bool:     # the register-resident chain
        return geom == 2

    def _feat_ok_reg(self, feat_pm) -> bool:
        if feat_pm is None:
            return True
        C = feat_pm.shape[2]
        if C <= 13:
            return True
        return (feat_pm.dtype == torch.bfloat16 and C % 8 == 0 and feat_pm.stride(1) % 8 == 0 and feat_pm.data_ptr() % 16 == 0)

    _feat_fits = _feat_ok_reg

    def _fresh_fits(self, C: int, dtype) -> bool:
        return C <= 13 or (dtype in (None, torch.bfloat16) and C % 8 == 0)

    @staticmethod
    def _feat(t: torch.Tensor, name: str):
        if not t.is_cuda or t.dtype not in (torch.bfloat16, torch.float32):
            raise TypeError(f"{name}: expected a GPU bfloat16 or float32 tensor")
        return 1 if t.dtype == torch.bfloat16 else 0

    def grouped(self, xyz: torch.Tensor, feat_pm: Optional[torch.Tensor], new_xyz: torch.Tensor,
                idx: torch.Tensor, out: Optional[torch.Tensor] = None, col_off: int = 0,
                cnt: Optional[torch.Tensor] = None, ws: Optional[torch.Tensor] = None,
                cont: Optional[torch.Tensor] = None) -> torch.Tensor:
        """xyz [B,N,3] f32; feat_pm point-major [B,N,C] bf16/f32 (or None); new_xyz [B,M,3]; idx
        [B,M,S] -> out[:, :, col_off:col_off+C_out] of a ZERO-initialised float32 [B,M,ld] buffer.
        With ``cnt`` ([B,M] int32 from ball_query_multi(return_counts=True)) only the leading cnt
        rows of each group are computed — the ball query's padding rows cannot change the max.
        ``ws``: the row-packing table of (idx, cnt) from ``rowscan_multi`` (geometry 2 then launches no scan).
        Split pooling: ``out`` an UNINITIALISED bfloat16 [B,M,ld] buffer and ``cont`` from ``cont_buffer`` (needs ``cnt`` and the
        register-resident chain) — the true pooled row is the maximum of out[g] and the group's continuation rows, which
        ``rows(..., pool=...)`` takes while it reads them (include/sad_amd.h ``sad_mlp_bf16_args.cont``)."""
        a, out, _keep = self._grouped_args(xyz, feat_pm, new_xyz, idx, out, col_off, cnt, ws, cont)
        self._launch(a, _keep + [out])
        return out

    def _feat_arg(self, a, feat_pm) -> None:
        a.feat_bf16 = self._feat(feat_pm, "feat_pm")
        if feat_pm.dim() != 3:
            raise ValueError("feat_pm: expected [B,N,C]")

    def _grouped_args(self, xyz, feat_pm, new_xyz, idx, out, col_off, cnt, ws=None, cont=None):
        """Validated ``MlpBf16Args`` of a grouped call + the output tensor + tensors to keep alive."""
        a, keep, xyz, feat_pm = self._grouped_prologue(xyz, feat_pm, new_xyz, idx)
        out = self._zero_out(a, xyz.device) if out is None else out
        split = out.dtype == torch.bfloat16
        if (not split and out.dtype != torch.float32) or not out.is_contiguous() or col_off + self.out_channels > out.shape[-1]:
            raise ValueError("out: expected a contiguous float32 (or, split pooling, bfloat16) [B,M,ld_out] buffer wide enough")
        if split != (cont is not None):
            raise ValueError("split pooling needs both a bfloat16 out and a continuation buffer (ops.cont_buffer)")
        a.out, a.out_bf16, a.ld_out, a.col_off = out.data_ptr(), int(split), out.stride(-2), col_off
        if split:
            if cnt is None or self.preferred_geometry != 2 or not self._feat_ok_reg(feat_pm):
                raise RuntimeError(f"{self.name or 'PackedMLPBf16'}: split pooling runs on the register-resident chain only (cnt, a compiled shape, 16-byte bf16 feature rows)")
            if cont.numel() * cont.element_size() < lib().sad_mlp_cont_bytes(a.B, a.M, a.S, self.out_channels):
                raise ValueError("cont: too small (ops.cont_buffer)")
            if ws is not None and not getattr(ws, "_sad_split", False):
                raise RuntimeError("split pooling: the row-packing table must come from rowscan_multi with split-pooling outs")
            a.cont = cont.data_ptr()
            keep.append(cont)
        if cnt is not None:
            self._counts_and_table(a, keep, cnt, ws, xyz.device)
        self._pick_geometry(a, cnt is not None and self._feat_fits(feat_pm), forced=2 if split else 0)
        return a, out, keep

    def _launch(self, a, keep=None) -> None:
        """Enqueue; with AUTOTUNE on, the first call for a shape times 64 / 128 / 256 rows per tile.  ``keep``: tensors the
        launch reads or writes (kept alive by a RERUN_LOG entry)."""
        key = self._key(a)
        geom = self._geom.get(key)
        preferred = a.geometry          # the un-tuned choice of _grouped_args (0 while autotuning)
        if not (a.idx and a.out_bf16):  # (split pooling: the register-resident chain, nothing to tune)
            if geom is None and ops.AUTOTUNE:
                geom = self._geom[key] = self._tune(a)
                preferred = 0
            a.geometry = geom or self.default_geometry or preferred
        _dispatch(self.name, self._CHAIN, self._enqueue(a), keep)

    def _tune(self, a) -> int:
        stream = torch.cuda.current_stream()
        enqueue = self._enqueue(a)
        best, best_ms, reg_ms = 0, None, None
        for code in (0, 32, 64, 128, 256) + ((2,) if a.cnt and a.workspace and not a.prescanned else ()):
            a.geometry = code
            ms = _time_launch(enqueue, stream)
            if ms is None:
                continue
            if code == 2:
                reg_ms = ms
            elif best_ms is None or ms < best_ms * 0.98:
                best, best_ms = code, ms
        # (the register-resident chain wins unless the tiled kernel is more than 10 % faster: see PackedMLP._tune)
        if reg_ms is not None and (best_ms is None or reg_ms <= best_ms * 1.10):
            best = 2
        return best

    def takes_pooled(self, rows: int, ld_out: int) -> bool:
        """Can ``rows(..., pool=...)`` read split-pooled rows: one layer on the row-streaming kernel (the autotuner may have picked a
        tiled kernel for this layer: then not)."""
        geom = self._geom.get((False, 1, 0, rows, 1, ld_out)) or self.default_geometry
        return self.L == 1 and not self.first_has_xyz and self.dims[0] % 8 == 0 and geom in (0, 3)

    def rows(self, x: torch.Tensor, out: Optional[torch.Tensor] = None, col_off: int = 0,
             out_dtype=torch.float32, pool=None) -> torch.Tensor:
        """Plain rows.  x [..., C] bf16/f32 (last-dim stride 1) -> [..., C_out] f32 or bf16.
        ``pool`` = [(ws, cont, S, cols)] per chain, in column order: ``x`` holds SPLIT-POOLED rows (``grouped(..., cont=...)``)
        of these chains side by side; the layer takes the maximum with their continuation rows while it reads them."""
        if self.first_has_xyz:
            raise RuntimeError("this PackedMLPBf16 was packed with the xyz prefix")
        a = self._args()
        a.feat_bf16 = self._feat(x, "x")
        keep_pool = []
        if pool:
            if len(pool) > _lib.MAX_RADII or x.dtype != torch.bfloat16 or not x.is_contiguous():
                raise ValueError(f"pool: at most {_lib.MAX_RADII} chains behind contiguous bfloat16 rows")
            a.n_pool = len(pool)
            for i, (ws, cont, S, cols) in enumerate(pool):
                a.pool_ws[i], a.pool_cont[i], a.pool_S[i], a.pool_cols[i] = ws.data_ptr(), cont.data_ptr(), int(S), int(cols)
                keep_pool += [ws, cont]
        x2, R, C = self._rows_input(x)
        if out is None:
            out = ops._empty(tuple(x.shape[:-1]) + (self.out_channels,), dtype=out_dtype, device=x.device)
        if out.dtype not in (torch.float32, torch.bfloat16) or not out.is_contiguous() \
                or out.numel() // out.shape[-1] != R or col_off + self.out_channels > out.shape[-1]:
            raise ValueError("out: expected a contiguous f32/bf16 [rows, ld_out] buffer wide enough")
        self._rows_args(a, x2, out, col_off)
        a.out_bf16 = int(out.dtype == torch.bfloat16)
        if pool:
            a.geometry = 0                # (the row-streaming layer: the only reader of split-pooled rows)
            _dispatch(self.name, self._CHAIN, self._enqueue(a), [x2, out] + keep_pool)
            _rec = _lib.recorder()
            if _rec is not None:
                _rec.keep.append((a, keep_pool))
            return out
        self._launch(a, [x2, out])
        return out


def mlp_chain(x: torch.Tensor, layers, relu_mask: Optional[int] = None) -> torch.Tensor:
    """One-shot convenience: pack ``layers`` and apply them to rows x [..., C]."""
    return PackedMLP(layers, False, x.device, relu_mask).rows(x)


# ---- backward of the chains (SPEC.md §32, csrc/mlp_grad.hip) -------------------------------------------------------------
NEED_BITS = {"feat": _lib.GRAD_FEAT, "xyz": _lib.GRAD_XYZ, "new_xyz": _lib.GRAD_NEW_XYZ, "params": _lib.GRAD_PARAMS}
GRAD_WS_BUDGET: int = 1 << 30      # bytes of workspace a call allocates at most when it is given none (it then works in chunks)


def _need_mask(need, allowed: int, default: int) -> int:
    if need is None:
        return default
    if isinstance(need, str):
        need = (need,)
    m = 0
    for n in need:
        if n not in NEED_BITS:
            raise ValueError(f"need: unknown gradient '{n}' (one of {sorted(NEED_BITS)})")
        m |= NEED_BITS[n]
    if m == 0 or m & ~allowed:
        raise ValueError("need: empty, or asks for a gradient this call does not have")
    return m


def _grad_layers(layers) -> Tuple[list, list, list]:
    """Unpacked layers [(W [C_l, C_{l-1}], b [C_l])] checked -> (Ws, bs, dims)."""
    if not 1 <= len(layers) <= _lib.MAX_LAYERS:
        raise ValueError(f"1..{_lib.MAX_LAYERS} layers supported")
    Ws, bs = [], []
    for l, (w, b) in enumerate(layers):
        if not isinstance(w, torch.Tensor) or not isinstance(b, torch.Tensor):
            raise TypeError("layers: expected (W, b) pairs of tensors")
        w = ops._strict(w.detach(), f"W[{l}]", torch.float32, (None, None))
        b = ops._strict(b.detach(), f"b[{l}]", torch.float32, (None,))
        if b.shape[0] != w.shape[0] or (Ws and w.shape[1] != Ws[-1].shape[0]) or min(w.shape) < 1:
            raise ValueError("layer shapes do not chain")
        Ws.append(w)
        bs.append(b)
    return Ws, bs, [Ws[0].shape[1]] + [w.shape[0] for w in Ws]


def _grad_rows_check(t: torch.Tensor, name: str, rows_shape: tuple, width: int, col_off: int) -> None:
    """A gradient / pooled tensor [*rows_shape, ld] that is read as rows of ``width`` columns from ``col_off``: float32 and wide
    enough (judged before any device)."""
    if not isinstance(t, torch.Tensor) or t.dtype != torch.float32:
        raise TypeError(f"{name}: expected a float32 tensor")
    if t.dim() != len(rows_shape) + 1 or tuple(t.shape[:-1]) != tuple(rows_shape):
        raise ValueError(f"{name}: expected shape {list(rows_shape)} + [ld], got {list(t.shape)}")
    if col_off < 0 or col_off + width > t.shape[-1]:
        raise ValueError(f"{name}: col_off + C_L = {col_off + width} exceeds its width {t.shape[-1]}")


def _grad_rows_read(t: torch.Tensor, name: str) -> torch.Tensor:
    """Rows at one stride with unit column stride are read where they lie, anything else through a packed copy."""
    uniform = t.stride(-1) == 1 and t.stride(-2) >= t.shape[-1] and all(t.stride(i) == t.stride(i + 1) * t.shape[i + 1]
                                                                          for i in range(t.dim() - 2))
    if not uniform:
        ops._unrecordable(f"{name}: strided copy")
        t = t.contiguous()
    return t


def _grad_on_gpu(named) -> None:
    for name, t in named:
        if t is not None:
            if not t.is_cuda:
                raise RuntimeError(f"{name}: expected a GPU tensor (sad_amd has no CPU path)")
            ops._on_current_device(t, name)


def mlp_grad_workspace_bytes(B: int, M: int, S: int, dims: Sequence[int], grouped: bool = True, has_cnt: bool = True) -> Tuple[int, int]:
    """(minimum, no-chunking size) in bytes of the workspace of ``grouped_mlp_grad`` (``grouped``) / ``mlp_rows_grad`` (B = 1, M = rows)."""
    lo, hi = ctypes.c_size_t(0), ctypes.c_size_t(0)
    check(lib().sad_mlp_grad_workspace_bytes(int(B), int(M), int(S), int(grouped), int(has_cnt), len(dims) - 1,
                                             (ctypes.c_int * len(dims))(*[int(d) for d in dims]), ctypes.byref(lo), ctypes.byref(hi)),
          "sad_mlp_grad_workspace_bytes")
    return lo.value, hi.value


def _grad_budget(sizes, workspace, budget) -> int:
    """Bytes to allocate when no workspace is given: the no-chunking size, capped by the budget, which may not be below the minimum."""
    lo, hi = sizes
    cap = GRAD_WS_BUDGET if budget is None else int(budget)
    if workspace is None and cap < lo:
        raise ValueError(f"workspace budget of {cap} bytes is below the minimum of {lo} (mlp_grad_workspace_bytes)")
    return min(hi, cap)


def _grad_call(a, Ws, bs, dims, need: int, spec, out, workspace, nbytes: int, lo: int, dev, maker: str):
    """Fills the layer / output / workspace fields of ``a`` -> ({name: output tensor}, workspace)."""
    L = len(Ws)
    a.struct_size = ctypes.sizeof(_lib.MlpGradArgs)
    a.L, a.need = L, need
    for i, d in enumerate(dims):
        a.dims[i] = d
    for l in range(L):
        a.W[l], a.b[l] = Ws[l].data_ptr(), bs[l].data_ptr()
    if need & _lib.GRAD_PARAMS:
        spec = list(spec) + [(f"grad_W{l}", tuple(Ws[l].shape), torch.float32) for l in range(L)] \
            + [(f"grad_b{l}", tuple(bs[l].shape), torch.float32) for l in range(L)]
    outs = dict(zip([n for n, _, _ in spec], ops._outputs(spec, out, dev, maker)))
    workspace = ops._workspace(nbytes if workspace is None else lo, workspace, dev, "mlp_grad_workspace_bytes", align=16)
    a.workspace, a.workspace_bytes = workspace.data_ptr(), workspace.numel() * workspace.element_size()
    if need & _lib.GRAD_PARAMS:
        for l in range(L):
            a.grad_W[l], a.grad_b[l] = outs[f"grad_W{l}"].data_ptr(), outs[f"grad_b{l}"].data_ptr()
    return outs, workspace


def _param_lists(outs: dict, L: int, need: int):
    if not need & _lib.GRAD_PARAMS:
        return None, None
    return [outs[f"grad_W{l}"] for l in range(L)], [outs[f"grad_b{l}"] for l in range(L)]


def grouped_mlp_grad(xyz: torch.Tensor, feat_pm: Optional[torch.Tensor], new_xyz: torch.Tensor, idx: torch.Tensor,
                     cnt: Optional[torch.Tensor], layers, pooled: torch.Tensor, grad_out: torch.Tensor, col_off: int = 0,
                     pooled_off: int = 0, skip_empty: bool = False, need=None, out: Optional[tuple] = None,
                     workspace: Optional[torch.Tensor] = None, budget_bytes: Optional[int] = None):
    """Backward of ``PackedMLP.grouped`` (SPEC.md §32).  Inputs as the forward's, ``layers`` = the UNPACKED [(W_l, b_l)] GPU tensors,
    ``pooled`` [B,M,ldp] the forward's output (columns pooled_off .. + C_L), ``grad_out`` [B,M,ld] read at columns col_off .. + C_L.
    ``need``: names out of ("feat", "xyz", "new_xyz", "params"), default all that exist; ``out``: the buffers to write, in the order
    (grad_feat, grad_xyz, grad_new_xyz, grad_W..., grad_b...) restricted to what is needed.  ``workspace``: at least the minimum of
    ``mlp_grad_workspace_bytes``; else one of at most ``budget_bytes`` (default ``GRAD_WS_BUDGET``) is allocated and the groups
    are processed in chunks.  -> (grad_feat [B,N,C], grad_xyz [B,N,3], grad_new_xyz [B,M,3], [grad_W], [grad_b], mismatch) with
    None for what was not asked; ``mismatch`` is a 1-element int32 GPU tensor (a view of the workspace: reading it synchronises,
    the call does not): 0 whenever ``pooled`` is the forward's.  Shapes and dtypes are judged before devices."""
    xyz = ops._strict(xyz, "xyz", torch.float32, (None, None, 3), "[B,N,3]")
    B, N, _ = xyz.shape
    idx = ops._strict(idx, "idx", torch.int32, (B, None, None), "[B,M,S]")
    _, M, S = idx.shape
    new_xyz = ops._strict(new_xyz, "new_xyz", torch.float32, (B, M, 3), "[B,M,3]")
    if min(B, N, M) < 1:
        raise ValueError("B, N and M must be >= 1")
    if not 1 <= S <= 64:
        raise ValueError(f"S = {S}: the grouped chain takes 1 .. 64 samples")
    Ws, bs, dims = _grad_layers(layers)
    C = 0
    if feat_pm is not None:
        if not isinstance(feat_pm, torch.Tensor) or feat_pm.dtype != torch.float32:
            raise TypeError("feat_pm: expected a float32 tensor")
        if feat_pm.dim() != 3 or feat_pm.shape[0] != B or feat_pm.shape[1] != N or feat_pm.shape[2] < 1:
            raise ValueError("feat_pm: expected [B,N,C]")
        C = feat_pm.shape[2]
    if dims[0] != C + 3:
        raise ValueError(f"MLP expects {dims[0] - 3} feature channels, got {C}")
    if cnt is not None:
        cnt = ops._strict(cnt, "cnt", torch.int32, (B, M), "[B,M]")
    elif skip_empty:
        raise ValueError("skip_empty needs cnt")
    _grad_rows_check(pooled, "pooled", (B, M), dims[-1], pooled_off)
    _grad_rows_check(grad_out, "grad_out", (B, M), dims[-1], col_off)
    allowed = _lib.GRAD_XYZ | _lib.GRAD_NEW_XYZ | _lib.GRAD_PARAMS | (_lib.GRAD_FEAT if C else 0)
    need = _need_mask(need, allowed, allowed)
    sizes = mlp_grad_workspace_bytes(B, M, S, dims, True, cnt is not None)
    nbytes = _grad_budget(sizes, workspace, budget_bytes)
    _grad_on_gpu([("xyz", xyz), ("new_xyz", new_xyz), ("idx", idx), ("cnt", cnt), ("feat_pm", feat_pm), ("pooled", pooled), ("grad_out", grad_out)]
                 + [(f"W[{l}]", w) for l, w in enumerate(Ws)] + [(f"b[{l}]", b) for l, b in enumerate(bs)])
    a = _lib.MlpGradArgs()
    if feat_pm is not None:
        if feat_pm.stride(2) != 1 or feat_pm.stride(0) != N * feat_pm.stride(1) or feat_pm.stride(1) < C:
            ops._unrecordable("feat_pm: strided copy")
            feat_pm = feat_pm.contiguous()
        a.feat, a.ld_feat = feat_pm.data_ptr(), feat_pm.stride(1)
    pooled, grad_out = _grad_rows_read(pooled, "pooled"), _grad_rows_read(grad_out, "grad_out")
    spec = [(n, s, torch.float32) for n, s, bit in (("grad_feat", (B, N, C), _lib.GRAD_FEAT), ("grad_xyz", (B, N, 3), _lib.GRAD_XYZ),
                                                    ("grad_new_xyz", (B, M, 3), _lib.GRAD_NEW_XYZ)) if need & bit]
    a.xyz, a.new_xyz, a.idx, a.cnt = xyz.data_ptr(), new_xyz.data_ptr(), idx.data_ptr(), ops._ptr(cnt)
    a.B, a.N, a.M, a.S, a.C = B, N, M, S, C
    a.relu_mask, a.skip_empty = (1 << len(Ws)) - 1, int(bool(skip_empty))
    a.pooled, a.ld_pooled, a.pooled_off = pooled.data_ptr(), pooled.stride(-2), int(pooled_off)
    a.grad_out, a.ld_grad, a.col_off = grad_out.data_ptr(), grad_out.stride(-2), int(col_off)
    outs, workspace = _grad_call(a, Ws, bs, dims, need, spec, out, workspace, nbytes, sizes[0], xyz.device, "grouped_mlp_grad")
    a.grad_feat, a.grad_xyz, a.grad_new_xyz = ops._ptr(outs.get("grad_feat")), ops._ptr(outs.get("grad_xyz")), ops._ptr(outs.get("grad_new_xyz"))
    with ops._timed("mlp_grad", f"g{B * M}s{S}"):
        check(lib().sad_mlp_grad_f32(ctypes.byref(a), ops._stream()), "sad_mlp_grad_f32")
    return (outs.get("grad_feat"), outs.get("grad_xyz"), outs.get("grad_new_xyz")) + _param_lists(outs, len(Ws), need) \
        + (workspace[:4].view(torch.int32),)


def mlp_rows_grad(x: torch.Tensor, layers, grad_out: torch.Tensor, relu_mask: Optional[int] = None, col_off: int = 0, need=None,
                  out: Optional[tuple] = None, workspace: Optional[torch.Tensor] = None, budget_bytes: Optional[int] = None):
    """Backward of ``PackedMLP.rows`` (SPEC.md §32): x [..., C_0] (unit last-dim stride), ``layers`` unpacked, ``relu_mask`` bit l = ReLU
    after layer l (default: all), ``grad_out`` [..., ld] read at columns col_off .. + C_L.  ``need`` out of ("feat", "params"):
    "feat" is the gradient of x.  ``out`` / ``workspace`` / ``budget_bytes`` as for ``grouped_mlp_grad`` (grad_x as [rows, C_0]).
    -> (grad_x [..., C_0], [grad_W], [grad_b]), None for what was not asked."""
    if not isinstance(x, torch.Tensor) or x.dtype != torch.float32:
        raise TypeError("x: expected a float32 tensor")
    Ws, bs, dims = _grad_layers(layers)
    L = len(Ws)
    if x.dim() < 1 or x.shape[-1] != dims[0]:
        raise ValueError(f"MLP expects {dims[0]} channels, got x of shape {list(x.shape)}")
    R = x.numel() // dims[0]
    if R < 1:
        raise ValueError("x: at least one row")
    relu_mask = (1 << L) - 1 if relu_mask is None else int(relu_mask)
    if relu_mask & ~((1 << L) - 1):
        raise ValueError("relu_mask: a bit beyond the last layer")
    _grad_rows_check(grad_out, "grad_out", tuple(x.shape[:-1]), dims[-1], col_off)
    allowed = _lib.GRAD_FEAT | _lib.GRAD_PARAMS
    need = _need_mask(need, allowed, allowed)
    sizes = mlp_grad_workspace_bytes(1, R, 1, dims, False, False)
    nbytes = _grad_budget(sizes, workspace, budget_bytes)
    _grad_on_gpu([("x", x), ("grad_out", grad_out)] + [(f"W[{l}]", w) for l, w in enumerate(Ws)] + [(f"b[{l}]", b) for l, b in enumerate(bs)])
    x2 = _grad_rows_read(x if x.dim() > 1 else x.unsqueeze(0), "x")
    x2 = x2.view(-1, dims[0]) if x2.dim() != 2 else x2
    g2 = _grad_rows_read(grad_out if grad_out.dim() > 1 else grad_out.unsqueeze(0), "grad_out")
    g2 = g2.view(-1, g2.shape[-1]) if g2.dim() != 2 else g2
    spec = [("grad_feat", (R, dims[0]), torch.float32)] if need & _lib.GRAD_FEAT else []
    a = _lib.MlpGradArgs()
    a.feat, a.ld_feat = x2.data_ptr(), x2.stride(0)
    a.B, a.N, a.M, a.S, a.C = 1, 0, R, 1, dims[0]
    a.relu_mask = relu_mask
    a.grad_out, a.ld_grad, a.col_off = g2.data_ptr(), g2.stride(0), int(col_off)
    outs, workspace = _grad_call(a, Ws, bs, dims, need, spec, out, workspace, nbytes, sizes[0], x.device, "mlp_rows_grad")
    a.grad_feat = ops._ptr(outs.get("grad_feat"))
    with ops._timed("mlp_grad", f"r{R}"):
        check(lib().sad_mlp_grad_f32(ctypes.byref(a), ops._stream()), "sad_mlp_grad_f32")
    gx = outs.get("grad_feat")
    return (gx.view(tuple(x.shape)) if gx is not None else None,) + _param_lists(outs, L, need)


# Last, because ops.py closes with a re-export of the names above: whichever of the two modules is imported first, the other
# then finds what it needs at import time already defined (ops is used at call time only).
from . import ops  # noqa: E402
