"""Every refusal of the MLP chain host code that is decided before the first HIP call: sad_mlp_chain_f32 / _bf16 (validation and the
per-kernel preparers up to a scan or VALU launch), the three sad_mlp_rowscan* entry points and the two *_multi entry points.  The return
code AND the text of sad_last_error() are compared with tests/golden/mlp_refusals.json, so which check fires first when several would is
pinned too.  Argument blocks hold fake non-null device pointers: nothing is dereferenced, no case reaches a launch (needs no GPU).

The fixture was recorded from the library as it was before the dispatch code was split into one preparer per kernel:
    python tests/test_mlp_refusals_cpu.py          (rewrites the fixture from the library that is built in the tree)"""
import ctypes
import json
import os
import sys

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mlp_refusals.json")
PTRS_F32 = ("xyz", "new_xyz", "idx", "cnt", "workspace", "feat", "packed", "out", "scratch")
PTRS_BF16 = ("xyz", "new_xyz", "idx", "feat", "packed", "out", "cnt", "workspace")
# plain base blocks: one layer of 64 (f32) / 128 (bf16) channels; grouped base blocks: a 3-layer chain with a compiled register-resident shape
F32_PLAIN = dict(feat=0x10000, packed=0x20000, out=0x30000, L=1, S=1, B=1, M=64, C=64, ld_feat=64, dims=(64, 128), ld_out=128, relu_mask=1)
F32_GROUPED = dict({f: 0x10000 for f in PTRS_F32}, L=3, B=1, N=64, M=16, S=32, C=64, ld_feat=64, dims=(67, 64, 64, 128), relu_mask=7,
                   ld_out=128, geometry=2)
F32_WIDE = dict(F32_GROUPED, C=256, ld_feat=256, dims=(259, 256, 512, 1024), ld_out=1024, geometry=3, scratch_bytes=1 << 62)
BF_PLAIN = dict(feat=0x10000, packed=0x20000, out=0x30000, L=1, S=1, B=1, M=256, C=128, ld_feat=128, feat_bf16=1, dims=(128, 32),
                ld_out=32, relu_mask=1)
BF_POOL = dict(BF_PLAIN, n_pool=1, pool_ws=(0x40000,), pool_cont=(0x50000,), pool_S=(32,), pool_cols=(128,))
BF_GROUPED = dict({f: 0x10000 for f in PTRS_BF16}, L=3, B=1, N=64, M=16, S=32, C=64, ld_feat=64, feat_bf16=1, dims=(67, 64, 64, 128),
                  relu_mask=7, ld_out=128, geometry=2)
MANY = dict(B=1 << 15, M=1 << 15, S=1, N=1)        # 2^30 groups of one row

# (name, base block, overrides); "struct_size" is relative to the right size; a base of None is a NULL argument block
CHAIN_F32 = [
    ("null", None, {}),
    ("struct_size", F32_PLAIN, dict(struct_size=-8)),
    ("struct_size+L", F32_PLAIN, dict(struct_size=8, L=0)),
    ("L=0", F32_PLAIN, dict(L=0)),
    ("L=5", F32_PLAIN, dict(L=5)),
    ("L=0+packed", F32_PLAIN, dict(L=0, packed=None)),
    ("dims[0]=0", F32_PLAIN, dict(dims=(0, 128))),
    ("dims[1]=5000", F32_PLAIN, dict(dims=(64, 5000))),
    ("packed", F32_PLAIN, dict(packed=None)),
    ("out", F32_PLAIN, dict(out=None)),
    ("packed+B", F32_PLAIN, dict(packed=None, B=0)),
    ("B=0", F32_PLAIN, dict(B=0)),
    ("M=0", F32_PLAIN, dict(M=0)),
    ("C=-1", F32_PLAIN, dict(C=-1)),
    ("feat", F32_PLAIN, dict(feat=None)),
    ("ld_feat", F32_PLAIN, dict(ld_feat=32)),
    ("feat+ld_feat", F32_PLAIN, dict(feat=None, ld_feat=32)),
    ("grouped xyz", F32_GROUPED, dict(xyz=None)),
    ("grouped new_xyz", F32_GROUPED, dict(new_xyz=None)),
    ("grouped N=0", F32_GROUPED, dict(N=0)),
    ("grouped S=0", F32_GROUPED, dict(S=0)),
    ("grouped S=65", F32_GROUPED, dict(S=65)),
    ("grouped xyz+S", F32_GROUPED, dict(xyz=None, S=65)),
    ("c_out too wide", F32_GROUPED, dict(c_out=200)),
    ("c_out C too wide", F32_GROUPED, dict(c_out=64, C=128, ld_feat=128)),
    ("grouped dims[0]", F32_GROUPED, dict(C=32)),
    ("B*N", F32_GROUPED, dict(B=1 << 16, N=1 << 15, M=1, S=1)),
    ("B*N+B*M*S", F32_GROUPED, dict(B=1 << 16, N=1 << 15, M=1 << 15, S=1)),
    ("B*M*S", F32_GROUPED, dict(B=1 << 16, N=1, M=1 << 15, S=1)),
    ("grouped relu", F32_GROUPED, dict(relu_mask=3)),
    ("grouped relu+ld_out", F32_GROUPED, dict(relu_mask=3, ld_out=64)),
    ("plain S=2", F32_PLAIN, dict(S=2)),
    ("plain c_out", F32_PLAIN, dict(c_out=8)),
    ("plain dims[0]", F32_PLAIN, dict(dims=(32, 128))),
    ("plain C=0", F32_PLAIN, dict(C=0)),
    ("plain rows", F32_PLAIN, dict(B=1 << 16, M=1 << 15)),
    ("ld_out", F32_PLAIN, dict(ld_out=64)),
    ("col_off<0", F32_PLAIN, dict(col_off=-4)),
    ("ld_out c_out", F32_GROUPED, dict(c_out=64, ld_out=32)),
    ("c_out geometry 0", F32_GROUPED, dict(c_out=64, geometry=0)),
    ("c_out geometry 3", F32_GROUPED, dict(c_out=64, geometry=3)),
    ("c_out mlp_force=5", F32_GROUPED, dict(c_out=64, mlp_force=5)),
    ("geometry 4 plain", F32_PLAIN, dict(geometry=4)),
    ("geometry 4 shape", F32_GROUPED, dict(geometry=4, C=1, ld_feat=1, dims=(4, 16, 16, 32), ld_out=32)),
    ("geometry 4 rows", F32_GROUPED, dict(geometry=4, ld_feat=66)),
    ("geometry 4 rows+workspace", F32_GROUPED, dict(geometry=4, ld_feat=66, workspace=0x10004)),
    ("geometry 2 plain", F32_PLAIN, dict(geometry=2)),
    ("geometry 2 shape", F32_GROUPED, dict(dims=(67, 64, 96, 96), ld_out=96)),
    ("geometry 2 cnt", F32_GROUPED, dict(cnt=None)),
    ("geometry 2 workspace", F32_GROUPED, dict(workspace=None)),
    ("geometry 2 feat", F32_GROUPED, dict(feat=0x10004)),
    ("geometry 2 align", F32_GROUPED, dict(workspace=0x10004)),
    ("geometry 2 groups", F32_GROUPED, MANY),
    ("geometry 2 align+groups", F32_GROUPED, dict(MANY, workspace=0x10004)),
    ("geometry 4 groups", F32_GROUPED, dict(MANY, geometry=4)),
    ("mlp_force=2 groups", F32_GROUPED, dict(MANY, geometry=0, mlp_force=2)),
    ("geometry 5 grouped", F32_GROUPED, dict(geometry=5)),
    ("geometry 5 L=2", F32_PLAIN, dict(geometry=5, L=2, dims=(64, 128, 128), relu_mask=3)),
    ("geometry 5 C=60", F32_PLAIN, dict(geometry=5, C=60, ld_feat=60, dims=(60, 128))),
    ("geometry 5 feat", F32_PLAIN, dict(geometry=5, feat=0x10004)),
    ("geometry 3 plain width", F32_PLAIN, dict(geometry=3, dims=(64, 64), ld_out=64)),
    ("geometry 3 plain cout", F32_PLAIN, dict(geometry=3, dims=(64, 100))),
    ("geometry 3 plain vec_out", F32_PLAIN, dict(geometry=3, out=0x30004)),
    ("geometry 3 plain no scratch", F32_PLAIN, dict(geometry=3, L=2, dims=(64, 128, 128), relu_mask=3)),
    ("geometry 3 plain small scratch", F32_PLAIN, dict(geometry=3, L=2, dims=(64, 128, 128), relu_mask=3, scratch=0x40000, scratch_bytes=64)),
    ("geometry 3 plain scratch align", F32_PLAIN, dict(geometry=3, L=2, dims=(64, 128, 128), relu_mask=3, scratch=0x40004, scratch_bytes=1 << 62)),
    ("geometry 3 plain 4 GiB", F32_PLAIN, dict(geometry=3, C=512, ld_feat=512, dims=(512, 128), M=2 * 1024 * 1024 + 128)),
    ("geometry 3 plain 4 GiB hidden", F32_PLAIN, dict(geometry=3, L=2, dims=(64, 1024, 128), relu_mask=3, M=1 << 20, scratch=0x40000, scratch_bytes=1 << 62)),
    ("geometry 3 plain align+4 GiB", F32_PLAIN, dict(geometry=3, L=2, dims=(64, 1024, 128), relu_mask=3, M=1 << 20, scratch=0x40004, scratch_bytes=1 << 62)),
    ("geometry 3 grouped width", F32_GROUPED, dict(geometry=3)),
    ("geometry 3 grouped cnt", F32_WIDE, dict(cnt=None)),
    ("geometry 3 grouped no scratch", F32_WIDE, dict(scratch=None)),
    ("geometry 3 grouped small scratch", F32_WIDE, dict(scratch_bytes=4096)),
    ("geometry 3 grouped workspace align", F32_WIDE, dict(workspace=0x10004)),
    ("geometry 3 grouped scratch align", F32_WIDE, dict(scratch=0x10004)),
    ("geometry 3 grouped groups", F32_WIDE, MANY),
    ("geometry 3 grouped align+groups", F32_WIDE, dict(MANY, scratch=0x10004)),
    ("geometry 3 grouped 4 GiB", F32_WIDE, dict(B=64, N=2048, M=1024)),
    ("geometry 3 grouped 4 GiB feat", F32_WIDE, dict(B=1 << 12, N=1 << 10, M=1)),
    ("geometry 3 grouped groups+4 GiB", F32_WIDE, dict(B=1 << 15, N=1 << 10, M=1 << 15, S=1)),
    ("geometry 1 plain", F32_PLAIN, dict(geometry=1)),
    ("geometry 1 grouped", F32_GROUPED, dict(geometry=1)),
    ("geometry 999", F32_PLAIN, dict(geometry=999)),
    ("geometry 830", F32_PLAIN, dict(geometry=830)),
    ("geometry 844", F32_PLAIN, dict(geometry=844)),
    ("geometry 804 LDS", F32_PLAIN, dict(geometry=804)),
    ("geometry 804 LDS chunked", F32_PLAIN, dict(geometry=804, C=512, ld_feat=512, dims=(512, 128))),
    ("heuristic LDS", F32_PLAIN, dict(L=2, C=4096, ld_feat=4096, dims=(4096, 4096, 128), relu_mask=3)),
    ("flex RW=2", F32_PLAIN, dict(geometry=100802)),
    ("flex 4", F32_PLAIN, dict(geometry=400000)),
    ("geometry 201601", F32_PLAIN, dict(geometry=201601)),      # (the forced geometry is read modulo 1000: 16 waves cannot be asked for)
    ("geometry 101644", F32_PLAIN, dict(geometry=101644, C=8, ld_feat=8, dims=(8, 32), ld_out=32)),
    ("geometry 1644", F32_PLAIN, dict(geometry=1644, C=8, ld_feat=8, dims=(8, 32), ld_out=32)),
    ("packing workspace align", F32_GROUPED, dict(geometry=10000, workspace=0x10004)),
    ("packing groups", F32_GROUPED, dict(MANY, geometry=10000)),
    ("packing align+groups", F32_GROUPED, dict(MANY, geometry=10000, workspace=0x10004)),
]
CHAIN_BF16 = [
    ("null", None, {}),
    ("struct_size", BF_PLAIN, dict(struct_size=-8)),
    ("struct_size+L", BF_PLAIN, dict(struct_size=8, L=0)),
    ("L=0", BF_PLAIN, dict(L=0)),
    ("L=5", BF_PLAIN, dict(L=5)),
    ("packed", BF_PLAIN, dict(packed=None)),
    ("out", BF_PLAIN, dict(out=None)),
    ("packed align", BF_PLAIN, dict(packed=0x20004)),
    ("out+packed align", BF_PLAIN, dict(packed=0x20004, out=None)),
    ("B=0", BF_PLAIN, dict(B=0)),
    ("C=-1", BF_PLAIN, dict(C=-1)),
    ("grouped xyz", BF_GROUPED, dict(xyz=None)),
    ("grouped N=0", BF_GROUPED, dict(N=0)),
    ("grouped S=0", BF_GROUPED, dict(S=0)),
    ("grouped dims[0]", BF_GROUPED, dict(C=32)),
    ("grouped relu", BF_GROUPED, dict(relu_mask=3)),
    ("grouped dims[0]+relu", BF_GROUPED, dict(C=32, relu_mask=3)),
    ("out_bf16 no cont", BF_GROUPED, dict(out_bf16=1)),
    ("out_bf16 tiled", BF_GROUPED, dict(out_bf16=1, cont=0x60000, geometry=128)),
    ("grouped n_pool", BF_GROUPED, dict(n_pool=1)),
    ("plain dims[0]", BF_PLAIN, dict(dims=(64, 32))),
    ("plain S=2", BF_PLAIN, dict(S=2)),
    ("plain C=0", BF_PLAIN, dict(C=0, dims=(0, 32))),
    ("feat", BF_PLAIN, dict(feat=None)),
    ("grouped feat", BF_GROUPED, dict(feat=None)),
    ("plain rows", BF_PLAIN, dict(B=1 << 16, M=1 << 15)),
    ("grouped rows", BF_GROUPED, dict(B=1 << 16, M=1 << 15, S=1)),
    ("feat+rows", BF_PLAIN, dict(feat=None, B=1 << 16, M=1 << 15)),
    ("feat align", BF_PLAIN, dict(feat=0x10008)),
    ("n_pool=5", BF_POOL, dict(n_pool=5)),
    ("n_pool=-1", BF_POOL, dict(n_pool=-1)),
    ("n_pool L=2", BF_POOL, dict(L=2, dims=(128, 64, 32))),
    ("n_pool f32 rows", BF_POOL, dict(feat_bf16=0)),
    ("n_pool geometry 32", BF_POOL, dict(geometry=32)),
    ("n_pool=5+L=2", BF_POOL, dict(n_pool=5, L=2, dims=(128, 64, 32))),
    ("pool_ws", BF_POOL, dict(pool_ws=(None,))),
    ("pool_cont align", BF_POOL, dict(pool_cont=(0x50008,))),
    ("pool_S=0", BF_POOL, dict(pool_S=(0,))),
    ("pool_S=65", BF_POOL, dict(pool_S=(65,))),
    ("pool_cols=24", BF_POOL, dict(pool_cols=(24,), C=24, ld_feat=24, dims=(24, 32))),
    ("pool_cols sum", BF_POOL, dict(pool_cols=(64,))),
    ("pool second chain", BF_POOL, dict(n_pool=2, pool_ws=(0x40000, None), pool_cont=(0x50000, 0x50000), pool_S=(32, 32), pool_cols=(64, 64))),
    ("pool cont bytes", BF_POOL, dict(B=1 << 10, M=1 << 13, pool_S=(64,))),
    ("pool rows", BF_POOL, dict(ld_feat=132)),
    ("geometry 3 rows", BF_PLAIN, dict(geometry=3, C=12, ld_feat=12, dims=(12, 32))),
    ("geometry 2 plain", BF_PLAIN, dict(geometry=2)),
    ("geometry 2 shape", BF_GROUPED, dict(dims=(67, 64, 64, 96), ld_out=96)),
    ("geometry 2 cnt", BF_GROUPED, dict(cnt=None)),
    ("geometry 2 workspace", BF_GROUPED, dict(workspace=None)),
    ("geometry 2 f32 rows", BF_GROUPED, dict(feat_bf16=0)),
    ("geometry 2 align", BF_GROUPED, dict(workspace=0x10004)),
    ("geometry 2 groups", BF_GROUPED, dict(B=1 << 14, M=1 << 15, S=1, N=1)),
    ("geometry 2 align+groups", BF_GROUPED, dict(B=1 << 14, M=1 << 15, S=1, N=1, workspace=0x10004)),
    ("geometry 2 B*N", BF_GROUPED, dict(B=1 << 16, N=1 << 15, M=1)),
    ("split multiples", BF_GROUPED, dict(out_bf16=1, cont=0x60000, ld_out=132)),
    ("split cont align", BF_GROUPED, dict(out_bf16=1, cont=0x60008)),
    ("split cont bytes", BF_GROUPED, dict(out_bf16=1, cont=0x60000, B=1 << 12, M=1 << 12)),
    ("split multiples+cont bytes", BF_GROUPED, dict(out_bf16=1, cont=0x60000, B=1 << 12, M=1 << 12, col_off=4)),
    ("tiled workspace align", BF_GROUPED, dict(geometry=0, workspace=0x10004)),
    ("tiled groups", BF_GROUPED, dict(MANY, geometry=0)),
    ("tiled geometry 48", BF_PLAIN, dict(geometry=48, L=2, dims=(128, 64, 32), relu_mask=3)),
    ("tiled geometry 5 grouped", BF_GROUPED, dict(geometry=5, cnt=None)),
    ("tiled align+geometry 5", BF_GROUPED, dict(geometry=5, workspace=0x10004)),
    ("tiled geometry 256 LDS", BF_PLAIN, dict(geometry=256, L=2, C=4096, ld_feat=4096, dims=(4096, 64, 32), relu_mask=3)),
    ("tiled LDS", BF_PLAIN, dict(L=2, C=4096, ld_feat=4096, dims=(4096, 64, 32), relu_mask=3)),
]
# sad_mlp_rowscan*: (name, entry point, overrides of the call below); per-chain arrays are given whole
SCAN = dict(n=2, cnt=(0x10000, 0x10000), idx=(0x20000, 0x20000), S=(32, 16), B=2, N=64, M=16, workspace=(0x30000, 0x40000),
            out=(0x50000, 0x50000), ld_out=(128, 128), col_off=(0, 64), cout=(64, 64), cont=(0x60000, 0x70000))
ROWSCAN = [(name, entry, ov) for entry in ("", "_init", "_split") for name, ov in [
    ("n=0", dict(n=0)),
    ("n=5", dict(n=5)),
    ("cnt array", dict(cnt=None)),
    ("workspace array", dict(workspace=None)),
    ("n=0+B=0", dict(n=0, B=0)),
    ("B=0", dict(B=0)),
    ("N=0", dict(N=0)),
    ("2^30 groups", dict(B=1 << 15, M=1 << 15, S=(1, 1))),
    ("cnt[0]", dict(cnt=(None, 0x10000))),
    ("idx[1]", dict(idx=(0x20000, None))),
    ("S[1]=0", dict(S=(32, 0))),
    ("S[0]=65", dict(S=(65, 16))),
    ("workspace[1] align", dict(workspace=(0x30000, 0x40004))),
    ("cnt[0]+workspace[0] align", dict(cnt=(None, 0x10000), workspace=(0x30004, 0x40000))),
    ("B*M*S", dict(B=1 << 13, M=1 << 13, S=(16, 32))),
    ("workspace[0] align+B*M*S", dict(B=1 << 13, M=1 << 13, S=(32, 32), workspace=(0x30004, 0x40000))),
]] + [
    ("out array", "_init", dict(out=None)),
    ("cout array", "_init", dict(cout=None)),
    ("out[1]", "_init", dict(out=(0x50000, None))),
    ("cout[0]=0", "_init", dict(cout=(0, 64))),
    ("col_off[0]<0", "_init", dict(col_off=(-4, 64))),
    ("ld_out[1]", "_init", dict(ld_out=(128, 96))),
    ("out[0]+cnt[1]", "_init", dict(out=(None, 0x50000), cnt=(0x10000, None))),
    ("2^29 groups", "_split", dict(B=1 << 14, M=1 << 15, S=(1, 1))),      # (the group number shares its int with one more flag)
    ("cont array", "_split", dict(cont=None)),
    ("cout array", "_split", dict(cout=None)),
    ("cont[1]", "_split", dict(cont=(0x60000, None))),
    ("cont[0] align", "_split", dict(cont=(0x60008, 0x70000))),
    ("cout[1]=4", "_split", dict(cout=(64, 4))),
    ("cout[0]=12", "_split", dict(cout=(12, 64))),
    ("cont[0]+workspace[1] align", "_split", dict(cont=(None, 0x70000), workspace=(0x30000, 0x40004))),
]


def _block(cls, base, ov):
    """An argument block of `cls` from a base dict and overrides; also returns the mlp_force knob the case asks for."""
    if base is None:
        return None, 0
    f = dict(base, **ov)
    a = cls()
    a.struct_size = ctypes.sizeof(cls) + f.pop("struct_size", 0)
    force = f.pop("mlp_force", 0)
    for k, v in f.items():
        if isinstance(v, tuple):
            for i, x in enumerate(v):
                getattr(a, k)[i] = x
        else:
            setattr(a, k, v)
    return a, force


def _outcome(L, code):
    assert code in (-1, -2), f"a case was not refused on the host (code {code})"
    return [code, L.sad_last_error().decode()]


def _chain(L, cls, fn, base, ov):
    a, force = _block(cls, base, ov)
    L.sad_set_option(b"mlp_force", force)
    try:
        return _outcome(L, fn(ctypes.byref(a) if a is not None else None, None))
    finally:
        L.sad_set_option(b"mlp_force", 0)


def _multi(L, cls, fn, blocks, n):
    """`blocks`: (base, overrides) pairs; None instead of the list = a NULL array."""
    if blocks is None:
        return _outcome(L, fn(None, n, None))
    keep = [_block(cls, b, ov)[0] for b, ov in blocks]
    arr = (ctypes.POINTER(cls) * len(keep))(*[ctypes.pointer(a) for a in keep])
    return _outcome(L, fn(arr, n, None))


def _rowscan(L, entry, ov):
    f = dict(SCAN, **ov)
    vp = ctypes.c_void_p

    def arr(key, ctype):
        return None if f[key] is None else (ctype * 4)(*f[key])       # (n = 5 is refused before an array is read)
    head = [f["n"], arr("cnt", vp), arr("idx", vp), arr("S", ctypes.c_int), f["B"], f["N"], f["M"], arr("workspace", vp)]
    tail = {"": [], "_init": [arr("out", vp), arr("ld_out", ctypes.c_int), arr("col_off", ctypes.c_int), arr("cout", ctypes.c_int)],
            "_split": [arr("cont", vp), arr("cout", ctypes.c_int)]}[entry]
    return _outcome(L, getattr(L, "sad_mlp_rowscan" + entry)(*head, *tail, None))


def outcomes():
    """{case name: [return code, message]} of every case, from the library that is loaded."""
    from sad_amd import _lib
    L = _lib.lib()
    got = {}
    for prefix, cls, fn, cases in (("f32", _lib.MlpArgs, L.sad_mlp_chain_f32, CHAIN_F32), ("bf16", _lib.MlpBf16Args, L.sad_mlp_chain_bf16, CHAIN_BF16)):
        for name, base, ov in cases:
            got[f"chain_{prefix}: {name}"] = _chain(L, cls, fn, base, ov)
    for prefix, cls, fn, plain in (("f32", _lib.MlpArgs, L.sad_mlp_chain_multi_f32, F32_PLAIN), ("bf16", _lib.MlpBf16Args, L.sad_mlp_chain_multi_bf16, BF_PLAIN)):
        bad, worse = (plain, dict(B=0)), (plain, dict(packed=None))
        got[f"multi_{prefix}: NULL array"] = _multi(L, cls, fn, None, 1)
        got[f"multi_{prefix}: n=0"] = _multi(L, cls, fn, [bad], 0)
        got[f"multi_{prefix}: n=-1"] = _multi(L, cls, fn, [bad], -1)
        got[f"multi_{prefix}: one bad chain"] = _multi(L, cls, fn, [bad], 1)
        got[f"multi_{prefix}: first bad chain of two"] = _multi(L, cls, fn, [bad, worse], 2)
        got[f"multi_{prefix}: first bad chain of six"] = _multi(L, cls, fn, [worse] + [bad] * 5, 6)     # (more than one dispatch carries)
    for name, entry, ov in ROWSCAN:
        got[f"rowscan{entry}: {name}"] = _rowscan(L, entry, ov)
    return got


def test_mlp_refusals_match_the_recorded_ones(sad):
    want = json.load(open(FIXTURE))
    got = outcomes()
    assert sorted(got) == sorted(want), "the cases of this file and of the fixture differ"
    wrong = {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    assert not wrong, f"{len(wrong)} refusals changed (got, recorded): {wrong}"


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    res = outcomes()
    with open(FIXTURE, "w") as fh:
        json.dump(res, fh, indent=0, sort_keys=True)
        fh.write("\n")
    print(f"recorded {len(res)} refusals -> {FIXTURE}")
