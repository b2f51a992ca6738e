"""The MLP chain backward (SPEC.md §32) without a GPU: the numpy reference against torch.autograd in float64 on lattice inputs
(where both forwards are exact and so decide alike), the exact summability of the lattice generator at every shape the GPU tests
use, the Python refusals of ``ops.grouped_mlp_grad`` / ``ops.mlp_rows_grad`` (judged before any device, so CPU tensors reach
them) and the repacking rule of ``SharedMLP.packed``."""
import numpy as np
import pytest
import torch

import mlp_grad_ref as ref


def _torch_grouped(inp, layers, grad_out):
    """The same chain in float64 torch: gather, layers, ReLU, max over the rows that exist (ties to the lowest slot), autograd."""
    t = lambda a: torch.from_numpy(np.asarray(a, np.float64))
    xyz, new_xyz = t(inp["xyz"]).requires_grad_(), t(inp["new_xyz"]).requires_grad_()
    feat = None if inp["feat"] is None else t(inp["feat"]).requires_grad_()
    Ws = [t(w).requires_grad_() for w, _ in layers]
    bs = [t(b).requires_grad_() for _, b in layers]
    idx = torch.from_numpy(inp["idx"].astype(np.int64))
    B, M, S = idx.shape
    bsel = torch.arange(B)[:, None, None].expand(B, M, S)
    x = xyz[bsel, idx] - new_xyz[:, :, None, :]
    if feat is not None:
        x = torch.cat([x, feat[bsel, idx]], -1)
    for w, b in zip(Ws, bs):
        x = torch.relu(x @ w.t() + b)
    nrow = torch.full((B, M), S) if inp["cnt"] is None else torch.from_numpy(np.clip(inp["cnt"], 1, S).astype(np.int64))
    live = torch.arange(S)[None, None, :, None] < nrow[..., None, None]
    xm = torch.where(live, x.detach(), torch.full_like(x, -1.0))                    # (activations are >= 0)
    arg = (xm == xm.amax(2, keepdim=True)).to(torch.int64).argmax(2, keepdim=True)  # the lowest slot that attains the maximum
    pooled = x.gather(2, arg).squeeze(2)
    if inp["skip_empty"]:
        pooled = torch.where(torch.from_numpy(inp["cnt"] == 0)[..., None], torch.zeros_like(pooled), pooled)
    (pooled * t(grad_out)).sum().backward()
    g = lambda v: None if v is None else v.grad.numpy()
    return {"grad_xyz": g(xyz), "grad_new_xyz": g(new_xyz), "grad_feat": g(feat), "grad_W": [g(w) for w in Ws], "grad_b": [g(b) for b in bs]}


def _same(name, a, b):
    assert a.shape == b.shape and (a == b).all(), f"{name}: max diff {np.abs(a - b).max():.3e}"


def _compare(got, want):
    for k, v in want.items():
        if v is None:
            continue
        if isinstance(v, list):
            for l, (a, b) in enumerate(zip(got[k], v)):
                _same(f"{k}[{l}]", np.asarray(a, np.float64), np.asarray(b, np.float64))
        else:
            _same(k, np.asarray(got[k], np.float64), np.asarray(v, np.float64))


@pytest.mark.parametrize("name", sorted(ref.GROUPED_CASES))
def test_reference_matches_torch_autograd_and_lattice_is_exact(orc, name):
    inp, layers, grad_out = ref.grouped_case(name, lattice=True)
    r64 = ref.grouped_ref(orc, layers=layers, grad_out=grad_out, **inp)
    assert r64["rows"] > 0
    _compare(r64["val"], _torch_grouped(inp, layers, grad_out))
    # the generator is exactly summable at this shape: float32 linear algebra gives the float64 values
    r32 = ref.grouped_ref(orc, layers=layers, grad_out=grad_out, dtype=np.float32, **inp)
    _compare(r32["val"], r64["val"])
    # every padding slot is dead: the reference over all S slots of every group gives the same gradients as over the rows that exist
    if inp["cnt"] is not None and not inp["skip_empty"]:
        dense = ref.grouped_ref(orc, layers=layers, grad_out=grad_out, **dict(inp, cnt=None))
        _compare(dense["val"], r64["val"])


@pytest.mark.parametrize("mask", sorted(ref.ROWS_MASKS))
@pytest.mark.parametrize("R", ref.ROWS_R)
def test_rows_reference_matches_torch_autograd_and_lattice_is_exact(orc, R, mask):
    x, layers, grad_out = ref.rows_case(R, lattice=True)
    m = ref.ROWS_MASKS[mask]
    r64 = ref.rows_ref(orc, x, layers, m, grad_out)
    t = lambda a: torch.from_numpy(np.asarray(a, np.float64))
    xt = t(x).requires_grad_()
    Ws, bs = [t(w).requires_grad_() for w, _ in layers], [t(b).requires_grad_() for _, b in layers]
    y = xt
    for l, (w, b) in enumerate(zip(Ws, bs)):
        y = y @ w.t() + b
        if (m >> l) & 1:
            y = torch.relu(y)
    assert (y.detach().numpy() == r64["out"]).all()
    (y * t(grad_out)).sum().backward()
    _compare(r64["val"], {"grad_x": xt.grad.numpy(), "grad_W": [w.grad.numpy() for w in Ws], "grad_b": [b.grad.numpy() for b in bs]})
    _compare(ref.rows_ref(orc, x, layers, m, grad_out, dtype=np.float32)["val"], r64["val"])


@pytest.mark.parametrize("name", sorted(ref.EDGE_CASES))
def test_edge_reference_matches_torch_autograd_and_lattice_is_exact(orc, name):
    """The same two checks for every case of EDGE_CASES (tests/test_gpu_mlp_grad_edges.py asserts equality on them), and the
    stronger form of the second: the sums are exact in float32 in any order, which is what the kernels' atomics need."""
    inp, layers, grad_out = ref.edge_case(name, lattice=True)
    r64 = ref.grouped_ref(orc, layers=layers, grad_out=grad_out, **inp)
    c = ref.EDGE_CASES[name]
    slots = c["B"] * c["M"] * c["S"]
    want_rows = {None: slots, "ones": c["B"] * c["M"], "zeros": 0}.get(c["cnt_mode"])
    assert r64["rows"] == want_rows if want_rows is not None else 0 < r64["rows"] < slots
    _compare(r64["val"], _torch_grouped(inp, layers, grad_out))
    r32 = ref.grouped_ref(orc, layers=layers, grad_out=grad_out, dtype=np.float32, **inp)
    _compare(r32["val"], r64["val"])
    ok, worst = ref.order_free(r64)
    assert ok, f"{name}: sum of magnitudes {worst} reaches 2^24 lattice units"
    if inp["cnt"] is not None and not inp["skip_empty"]:
        dense = ref.grouped_ref(orc, layers=layers, grad_out=grad_out, **dict(inp, cnt=None))
        _compare(dense["val"], r64["val"])
    if c["cnt_mode"] == "zeros":                                                     # nothing but empty groups: every gradient is 0
        for v in r64["val"].values():
            assert all((a == 0).all() for a in (v if isinstance(v, list) else [v]))


def test_grouped_reference_with_masked_pairs_is_autograd_of_a_masked_output(orc):
    """What the counter test of the GPU file compares against: zeroing grad_out at chosen (group, channel) pairs is the gradient
    of an output from which those pairs were removed, so a pair that route gives no row contributes to no gradient."""
    inp, layers, grad_out = ref.grouped_case("L3_C5_S33_skip_B2", lattice=True)
    pairs = ref.corrupt_pairs(inp["cnt"], grad_out, 12, 4)
    masked = ref.zero_pairs(grad_out, pairs)
    assert sum(inp["cnt"][b, m] == 0 for b, m, _ in pairs) >= 3 and {b for b, _, _ in pairs} == {0, 1}
    assert all(grad_out[b, m, o] != 0 for b, m, o in pairs) and (masked != grad_out).sum() == len(pairs)
    r = ref.grouped_ref(orc, layers=layers, grad_out=masked, **inp)
    _compare(r["val"], _torch_grouped(inp, layers, masked))
    full = ref.grouped_ref(orc, layers=layers, grad_out=grad_out, **inp)
    assert any((a != b).any() for a, b in zip(r["val"]["grad_W"], full["val"]["grad_W"])), "the live pairs chosen carry no gradient"
    assert ref.order_free(r)[0]


@pytest.mark.parametrize("mask", sorted(ref.EDGE_ROWS_MASKS))
@pytest.mark.parametrize("dims", sorted(ref.EDGE_ROWS_DIMS))
@pytest.mark.parametrize("R", ref.EDGE_ROWS_R)
def test_edge_rows_reference_matches_torch_autograd_and_lattice_is_exact(orc, R, dims, mask):
    x, layers, grad_out = ref.edge_rows_case(R, dims, lattice=True)
    m = ref.EDGE_ROWS_MASKS[mask]
    r64 = ref.rows_ref(orc, x, layers, m, grad_out)
    t = lambda a: torch.from_numpy(np.asarray(a, np.float64))
    xt = t(x).requires_grad_()
    Ws, bs = [t(w).requires_grad_() for w, _ in layers], [t(b).requires_grad_() for _, b in layers]
    y = xt
    for l, (w, b) in enumerate(zip(Ws, bs)):
        y = y @ w.t() + b
        if (m >> l) & 1:
            y = torch.relu(y)
    assert (y.detach().numpy() == r64["out"]).all()
    (y * t(grad_out)).sum().backward()
    _compare(r64["val"], {"grad_x": xt.grad.numpy(), "grad_W": [w.grad.numpy() for w in Ws], "grad_b": [b.grad.numpy() for b in bs]})
    _compare(ref.rows_ref(orc, x, layers, m, grad_out, dtype=np.float32)["val"], r64["val"])
    ok, worst = ref.order_free(r64)
    assert ok, f"R = {R}, {dims}: sum of magnitudes {worst} reaches 2^24 lattice units"


def _cpu_call(**over):
    """Arguments of a well-formed grouped call on CPU tensors (refused as such at the very end), with overrides."""
    B, N, M, S, C = 1, 8, 4, 2, 2
    a = dict(xyz=torch.zeros(B, N, 3), feat_pm=torch.zeros(B, N, C), new_xyz=torch.zeros(B, M, 3), idx=torch.zeros(B, M, S, dtype=torch.int32),
             cnt=torch.ones(B, M, dtype=torch.int32), layers=[(torch.zeros(6, 5), torch.zeros(6))], pooled=torch.zeros(B, M, 6),
             grad_out=torch.zeros(B, M, 6))
    a.update(over)
    return a


def test_grouped_refusals(sad):
    from sad_amd import ops
    g = ops.grouped_mlp_grad
    with pytest.raises(RuntimeError, match="GPU tensor"):                            # right in everything but the device
        g(**_cpu_call())
    with pytest.raises(TypeError, match="idx"):
        g(**_cpu_call(idx=torch.zeros(1, 4, 2, dtype=torch.int64)))
    with pytest.raises(TypeError, match="xyz"):
        g(**_cpu_call(xyz=torch.zeros(1, 8, 3, dtype=torch.float64)))
    with pytest.raises(TypeError, match="grad_out"):
        g(**_cpu_call(grad_out=torch.zeros(1, 4, 6, dtype=torch.float16)))
    with pytest.raises(ValueError, match="contiguous"):
        g(**_cpu_call(idx=torch.zeros(1, 2, 4, dtype=torch.int32).transpose(1, 2)))
    with pytest.raises(ValueError, match="new_xyz"):
        g(**_cpu_call(new_xyz=torch.zeros(1, 5, 3)))
    with pytest.raises(ValueError, match="cnt"):
        g(**_cpu_call(cnt=torch.ones(1, 5, dtype=torch.int32)))
    with pytest.raises(ValueError, match="layers"):                                  # L > 4
        g(**_cpu_call(layers=[(torch.zeros(5, 5), torch.zeros(5))] * 5))
    with pytest.raises(ValueError, match="chain"):
        g(**_cpu_call(layers=[(torch.zeros(6, 5), torch.zeros(6)), (torch.zeros(6, 7), torch.zeros(6))]))
    with pytest.raises(ValueError, match="1 .. 64"):                                 # S > 64
        g(**_cpu_call(idx=torch.zeros(1, 4, 65, dtype=torch.int32)))
    with pytest.raises(ValueError, match="feature channels"):
        g(**_cpu_call(feat_pm=None))
    with pytest.raises(ValueError, match="col_off"):                                 # grad_out too narrow for col_off
        g(**_cpu_call(col_off=1))
    g_wide = _cpu_call(grad_out=torch.zeros(1, 4, 10), col_off=4)                    # (a slice that fits passes this check)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        g(**g_wide)
    with pytest.raises(ValueError, match="pooled"):
        g(**_cpu_call(pooled=torch.zeros(1, 4, 5)))
    with pytest.raises(ValueError, match="skip_empty"):
        g(**_cpu_call(cnt=None, skip_empty=True))
    with pytest.raises(ValueError, match="need"):
        g(**_cpu_call(need=("feat", "weights")))
    with pytest.raises(ValueError, match="need"):
        g(**_cpu_call(feat_pm=None, layers=[(torch.zeros(6, 3), torch.zeros(6))], need=("feat",)))
    lo, hi = ops.mlp_grad_workspace_bytes(1, 4, 2, [5, 6])
    assert 0 < lo <= hi
    with pytest.raises(ValueError, match="below the minimum"):                       # workspace budget below the minimum
        g(**_cpu_call(budget_bytes=lo - 1))
    with pytest.raises(ValueError, match="workspace"):                               # the checker the operator uses on a given workspace
        ops._workspace(lo, torch.empty(lo - 1, dtype=torch.uint8), torch.device("cpu"), "mlp_grad_workspace_bytes", align=16)


def test_rows_refusals(sad):
    from sad_amd import ops
    r = ops.mlp_rows_grad
    layers = [(torch.zeros(6, 5), torch.zeros(6)), (torch.zeros(4, 6), torch.zeros(4))]
    with pytest.raises(RuntimeError, match="GPU tensor"):
        r(torch.zeros(9, 5), layers, torch.zeros(9, 4))
    with pytest.raises(TypeError, match="x"):
        r(torch.zeros(9, 5, dtype=torch.float64), layers, torch.zeros(9, 4))
    with pytest.raises(ValueError, match="channels"):
        r(torch.zeros(9, 4), layers, torch.zeros(9, 4))
    with pytest.raises(ValueError, match="col_off"):
        r(torch.zeros(9, 5), layers, torch.zeros(9, 4), col_off=2)
    with pytest.raises(ValueError, match="grad_out"):
        r(torch.zeros(9, 5), layers, torch.zeros(8, 4))
    with pytest.raises(ValueError, match="relu_mask"):
        r(torch.zeros(9, 5), layers, torch.zeros(9, 4), relu_mask=4)
    with pytest.raises(ValueError, match="need"):
        r(torch.zeros(9, 5), layers, torch.zeros(9, 4), need=("xyz",))
    with pytest.raises(ValueError, match="below the minimum"):
        r(torch.zeros(9, 5), layers, torch.zeros(9, 4), budget_bytes=8)


def test_c_entry_refusals(sad):
    """The C entry refuses what it cannot run before any launch (fake device pointers, nothing is dereferenced)."""
    import ctypes
    from sad_amd import _lib
    L = _lib.lib()
    P = 0x10000

    def block(**over):
        a = _lib.MlpGradArgs()
        a.struct_size = ctypes.sizeof(_lib.MlpGradArgs)
        for f in ("xyz", "new_xyz", "feat", "idx", "cnt", "pooled", "grad_out", "grad_feat", "grad_xyz", "grad_new_xyz", "workspace"):
            setattr(a, f, P)
        a.B, a.N, a.M, a.S, a.C, a.L, a.ld_feat = 1, 8, 4, 2, 2, 1, 2
        a.dims[0], a.dims[1] = 5, 6
        a.W[0] = a.b[0] = a.grad_W[0] = a.grad_b[0] = P
        a.relu_mask, a.need, a.ld_pooled, a.ld_grad, a.workspace_bytes = 1, 15, 6, 6, 1 << 20
        for k, v in over.items():
            setattr(a, k, v)
        return a

    def refused(a, text, code=-1):
        assert L.sad_mlp_grad_f32(ctypes.byref(a), None) == code
        assert text in L.sad_last_error(), L.sad_last_error()

    assert L.sad_mlp_grad_f32(None, None) == -1
    refused(block(struct_size=8), b"struct_size")
    refused(block(L=5), b"layers")
    refused(block(S=65), b"samples")
    refused(block(col_off=1), b"col_off")
    refused(block(pooled_off=1), b"pooled")
    refused(block(need=0), b"need")
    refused(block(need=16), b"need")
    refused(block(relu_mask=0), b"ReLU")
    refused(block(C=3), b"dims[0]")
    refused(block(workspace=P + 4), b"aligned")
    refused(block(workspace_bytes=64), b"minimum")
    refused(block(grad_xyz=None), b"grad_xyz")
    refused(block(B=1 << 14, M=1 << 14, S=4), b"2^29", code=-2)
    refused(block(idx=None, need=2, C=5, ld_feat=5), b"coordinate")
    lo, hi = ctypes.c_size_t(0), ctypes.c_size_t(0)
    dims = (ctypes.c_int * 2)(5, 6)
    assert L.sad_mlp_grad_workspace_bytes(1, 4, 2, 1, 1, 1, dims, ctypes.byref(lo), ctypes.byref(hi)) == 0
    assert lo.value == hi.value == 64 + ((L.sad_mlp_workspace_bytes(1, 4, 2) + 15) & ~15) + 4 * 11 * 8     # 4 groups x 2 rows, X_0 + X_1
    assert L.sad_mlp_grad_workspace_bytes(1, 1000, 1, 0, 0, 1, dims, ctypes.byref(lo), ctypes.byref(hi)) == 0
    assert (lo.value, hi.value) == (64 + 4 * 6 * 64, 64 + 4 * 6 * 1000)                                     # plain rows: X_1 only
    assert L.sad_mlp_grad_workspace_bytes(1, 4, 65, 1, 1, 1, dims, ctypes.byref(lo), ctypes.byref(hi)) == -1


def test_shared_mlp_repacks_after_an_in_place_update(sad, monkeypatch):
    from sad_amd import ops, shared_mlp
    made = []

    class FakePacked:
        def __init__(self, layers, first_has_xyz, device, relu_mask=None, name=""):
            made.append([w.clone() for w, _ in layers])

    monkeypatch.setattr(ops, "PackedMLP", FakePacked)
    m = shared_mlp.SharedMLP([7, 16, 8], True)
    assert all(not p.requires_grad for p in m.parameters())
    p0 = m.packed()
    assert m.packed() is p0 and len(made) == 1                                       # nothing changed: the same chain
    with torch.no_grad():
        m.weight[1].add_(1.0)                                                        # an optimiser step
    p1 = m.packed()
    assert p1 is not p0 and len(made) == 2 and (made[1][1] == made[0][1] + 1.0).all()
    m.bias[0] = torch.nn.Parameter(torch.ones(16), requires_grad=False)              # a replaced parameter
    assert m.packed() is not p1 and len(made) == 3
    assert m.packed() is m.packed() and len(made) == 3
    layers = m.export()
    assert [w.shape for w, _ in layers] == [(16, 7), (8, 16)] and (layers[0][1] == 1.0).all()
