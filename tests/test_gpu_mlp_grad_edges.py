"""The MLP chain backward (SPEC.md §32) at its contract edges and tile boundaries: what tests/test_gpu_mlp_grad.py leaves open.

1. the mismatch counter counts (test_counter_*): pooled values no row attains are counted, pair by pair, over chunks and through
   autograd, and the pairs that miss get no gradient;
2. unwritten memory (test_dirty_*): NaN-filled ``out=`` buffers and 0xFF-filled workspaces give the bits of fresh ones;
3. a non-default current stream (test_non_default_stream);
4. operand strides (test_strided_*): ``feat_pm`` / ``x`` read in place at a row stride above their width, non-uniform views copied,
   ``col_off`` of plain rows;
5. GEMM tile edges, 6. chunks without counts, 7. row counts far below the slots and nothing but empty groups
   (test_edge_grouped_against_reference / test_edge_rows_against_reference over mlp_grad_ref.EDGE_CASES / EDGE_ROWS_*).

The judges are those of test_gpu_mlp_grad.py: general inputs within n * 2^-23 * A of the float64 reference with its exact zeros
exact (``check_close``), lattice inputs equal (they are exactly summable in any order: tests/test_mlp_grad_cpu.py) and two calls
bit-equal."""
import numpy as np
import pytest

import mlp_grad_ref as ref
from test_gpu_mlp_grad import _forward, _grouped, _layers, _np, _t

pytestmark = pytest.mark.gpu

NAN = float("nan")
NEEDS = (None, ("params",))                                      # the default need mask, parameters only


def _flat(got):
    """The gradient tensors of a grouped (6 entries, the last the mismatch view) or plain-rows (3) result, in the order of ``out=``."""
    head, (gW, gb) = (got[:3], got[3:5]) if len(got) == 6 else (got[:1], got[1:3])
    return [t for t in head if t is not None] + list(gW or []) + list(gb or [])


def _bits_equal(a, b, what):
    import torch
    fa, fb = _flat(a), _flat(b)
    assert len(fa) == len(fb) and len(fa) > 0, what
    for i, (x, y) in enumerate(zip(fa, fb)):
        assert x.shape == y.shape and torch.equal(x.contiguous().view(torch.int32), y.contiguous().view(torch.int32)), f"{what}: output {i} differs"


def _check_grouped(res, got, exact, mismatch=0):
    gf, gx, gn, gW, gb, mm = got
    assert int(mm.item()) == mismatch, f"mismatch = {int(mm.item())}, expected {mismatch}"
    for name, g in (("grad_feat", gf), ("grad_xyz", gx), ("grad_new_xyz", gn)):
        if g is not None:
            ref.check_close(name, _np(g), res["val"][name], res["A"][name], res["depth"][name], exact)
    for l in range(len(gW or [])):
        ref.check_close(f"grad_W[{l}]", _np(gW[l]), res["val"]["grad_W"][l], res["A"]["grad_W"][l], res["depth"]["grad_W"][l], exact)
        ref.check_close(f"grad_b[{l}]", _np(gb[l]), res["val"]["grad_b"][l], res["A"]["grad_b"][l], res["depth"]["grad_b"][l], exact)


def _check_rows(res, got, exact):
    gx, gW, gb = got
    if gx is not None:
        ref.check_close("grad_x", _np(gx), res["val"]["grad_x"], res["A"]["grad_x"], res["depth"]["grad_x"], exact)
    for l in range(len(gW or [])):
        ref.check_close(f"grad_W[{l}]", _np(gW[l]), res["val"]["grad_W"][l], res["A"]["grad_W"][l], res["depth"]["grad_W"][l], exact)
        ref.check_close(f"grad_b[{l}]", _np(gb[l]), res["val"]["grad_b"][l], res["A"]["grad_b"][l], res["depth"]["grad_b"][l], exact)


def _ws_bytes(inp, layers):
    """(minimum, no-chunking size) of the grouped workspace of a case."""
    from sad_amd import ops
    B, M, S = inp["idx"].shape
    return ops.mlp_grad_workspace_bytes(B, M, S, [layers[0][0].shape[1]] + [w.shape[0] for w, _ in layers], True, inp["cnt"] is not None)


def _min_workspace(dev, inp, layers):
    """A workspace of the minimum size (chunks of 64 groups) -> (workspace, minimum, no-chunking size)."""
    import torch
    lo, hi = _ws_bytes(inp, layers)
    return torch.empty(lo, dtype=torch.uint8, device=dev), lo, hi


# ---- gaps 5, 6, 7: tile edges, chunks without counts, rows far below the slots, nothing but empty groups ----
@pytest.mark.parametrize("lattice", [False, True], ids=["general", "lattice"])
@pytest.mark.parametrize("name", sorted(ref.EDGE_CASES))
def test_edge_grouped_against_reference(sad, dev, orc, name, lattice):
    inp, layers, grad_out = ref.edge_case(name, lattice)
    c = ref.EDGE_CASES[name]
    all_empty = c["cnt_mode"] == "zeros"
    if all_empty:                                                # skipped groups may carry any coordinates
        assert c["skip"] and (inp["cnt"] == 0).all()
        inp["new_xyz"] = np.full_like(inp["new_xyz"], np.nan)
    with np.errstate(all="ignore"):
        res = ref.grouped_ref(orc, layers=layers, grad_out=grad_out, **inp)
    pooled, g = _forward(dev, inp, layers), _t(grad_out, dev)
    kw = {}
    if name.startswith("chunks"):                                # the minimum workspace: 200 groups in four chunks of 64
        kw["workspace"], lo, hi = _min_workspace(dev, inp, layers)
        assert lo < hi and c["B"] * c["M"] > 3 * 64
    print(f"{name} ({'lattice' if lattice else 'general'}): {res['rows']} rows of {inp['idx'].size} slots")
    for need in NEEDS:
        got = _grouped(dev, inp, layers, pooled, g, need=need, **kw)
        assert (got[0] is not None) == (got[1] is not None) == (got[2] is not None) == (need is None) and got[3] is not None
        _check_grouped(res, got, exact=lattice)
        if lattice:
            _bits_equal(got, _grouped(dev, inp, layers, pooled, g, need=need, **kw), f"{name}: two calls")
        if all_empty:
            for t in _flat(got):
                assert (_np(t).view(np.int32) == 0).all(), f"{name}: an output that is not +0 everywhere"


@pytest.mark.parametrize("mask", sorted(ref.EDGE_ROWS_MASKS))
@pytest.mark.parametrize("dims", sorted(ref.EDGE_ROWS_DIMS))
@pytest.mark.parametrize("R", ref.EDGE_ROWS_R)
def test_edge_rows_against_reference(sad, dev, orc, R, dims, mask):
    from sad_amd import ops
    m = ref.EDGE_ROWS_MASKS[mask]
    for lattice in (False, True):
        x, layers, grad_out = ref.edge_rows_case(R, dims, lattice)
        res = ref.rows_ref(orc, x, layers, m, grad_out)
        print(f"R = {R}, dims {dims}, mask {mask} ({'lattice' if lattice else 'general'})")
        for need in NEEDS + (("feat",),):
            got = ops.mlp_rows_grad(_t(x, dev), _layers(layers, dev), _t(grad_out, dev), relu_mask=m, need=need)
            assert (got[0] is None) == (need == ("params",)) and (got[1] is None) == (got[2] is None) == (need == ("feat",))
            _check_rows(res, got, exact=lattice)
            if lattice:
                _bits_equal(got, ops.mlp_rows_grad(_t(x, dev), _layers(layers, dev), _t(grad_out, dev), relu_mask=m, need=need), "two calls")


# ---- gap 1: the counter counts ----
def _tamper(pooled, pairs):
    """pooled with the chosen pairs replaced by values no row can attain: above the maximum, below any ReLU output, NaN."""
    p = _np(pooled).copy()
    for i, (b, m, o) in enumerate(pairs):
        p[b, m, o] = (p[b, m, o] + 1.0, -1.0, np.nan)[i % 3]
    return _t(p, pooled.device)


def test_counter_counts_the_pairs_that_miss(sad, dev, orc):
    """16 corrupted pairs of L3_C5_S33_skip_B2, 4 of them in groups that skip_empty leaves out: mismatch == 12, and every gradient
    is the reference's with grad_out zeroed at the corrupted pairs (route gives them no row).  A clean call into the same
    workspace counts 0 again (the header is cleared by every call)."""
    import torch
    inp, layers, grad_out = ref.grouped_case("L3_C5_S33_skip_B2", True)
    k_live, k_dead = 12, 4
    pairs = ref.corrupt_pairs(inp["cnt"], grad_out, k_live, k_dead)
    assert len(set(pairs)) == k_live + k_dead and {b for b, _, _ in pairs} == {0, 1}
    assert sum(inp["cnt"][b, m] == 0 for b, m, _ in pairs) == k_dead >= 3
    res = ref.grouped_ref(orc, layers=layers, grad_out=ref.zero_pairs(grad_out, pairs), **inp)
    pooled, g = _forward(dev, inp, layers), _t(grad_out, dev)
    bad = _tamper(pooled, pairs)
    ws = torch.empty(_ws_bytes(inp, layers)[1], dtype=torch.uint8, device=dev)
    for need in NEEDS:
        got = _grouped(dev, inp, layers, bad, g, need=need, workspace=ws)
        print(f"need {need}: expected mismatch {k_live}, observed {int(got[5].item())}")
        _check_grouped(res, got, exact=True, mismatch=k_live)
        clean = _grouped(dev, inp, layers, pooled, g, need=need, workspace=ws)
        assert int(clean[5].item()) == 0, "the counter of an earlier call survives in the workspace"


def test_counter_accumulates_over_chunks(sad, dev, orc):
    """The shape of test_chunked_workspace (200 groups, four chunks of the minimum workspace), 14 corrupted pairs from the first
    to the last group, some in every chunk: the count is the sum over the chunks, with the minimum workspace and without chunking."""
    inp, layers, grad_out = ref.edge_case("chunks_M100_S16_mixed_B2", True)
    k = 14
    pairs = ref.corrupt_pairs(None, grad_out, k, 0)                  # no skip_empty: every group is live
    M = grad_out.shape[1]
    assert len(set(pairs)) == k and {(b * M + m) // 64 for b, m, _ in pairs} == {0, 1, 2, 3}
    res = ref.grouped_ref(orc, layers=layers, grad_out=ref.zero_pairs(grad_out, pairs), **inp)
    pooled, g = _forward(dev, inp, layers), _t(grad_out, dev)
    bad = _tamper(pooled, pairs)
    ws, lo, hi = _min_workspace(dev, inp, layers)
    for kw in (dict(workspace=ws), dict(budget_bytes=hi)):
        got = _grouped(dev, inp, layers, bad, g, **kw)
        print(f"{'chunked' if 'workspace' in kw else 'whole'}: expected mismatch {k}, observed {int(got[5].item())}")
        _check_grouped(res, got, exact=True, mismatch=k)


def test_counter_through_autograd(sad, dev, orc):
    """SharedMLP.grouped(...).backward() with the saved output overwritten between forward and backward (through ``.data``, which
    autograd's version check does not see): ``autograd.GroupedMLP.last_mismatch`` is the count of a direct call, the gradients
    are the direct call's."""
    import torch
    from sad_amd import autograd
    from sad_amd.shared_mlp import SharedMLP
    name = "L3_C5_S33_skip_B2"
    inp, layers, grad_out = ref.grouped_case(name, True)
    c = ref.GROUPED_CASES[name]
    pairs = ref.corrupt_pairs(inp["cnt"], grad_out, 12, 4)
    res = ref.grouped_ref(orc, layers=layers, grad_out=ref.zero_pairs(grad_out, pairs), **inp)
    m = SharedMLP([3 + c["C"]] + c["widths"], True, layers=layers).to(dev)
    m.requires_grad_(True)
    xyz, feat, new_xyz, idx, cnt = (_t(inp[k], dev) for k in ("xyz", "feat", "new_xyz", "idx", "cnt"))
    for t in (xyz, feat, new_xyz):
        t.requires_grad_(True)
    out = m.grouped(xyz, feat, new_xyz, idx, cnt, skip_empty=True)
    bad = _tamper(out.detach(), pairs)
    out.data.copy_(bad)
    out.backward(_t(grad_out, dev))
    got = (feat.grad, xyz.grad, new_xyz.grad, [w.grad for w in m.weight], [b.grad for b in m.bias], autograd.GroupedMLP.last_mismatch)
    direct = _grouped(dev, inp, layers, bad, _t(grad_out, dev))
    print(f"autograd: expected mismatch 12, direct call {int(direct[5].item())}, last_mismatch {int(got[5].item())}")
    assert int(got[5].item()) == int(direct[5].item())
    _check_grouped(res, got, exact=True, mismatch=12)
    _bits_equal(got, direct, "autograd against the direct call")


# ---- gap 2: unwritten memory ----
def test_dirty_buffers_grouped(sad, dev, orc):
    """NaN-filled ``out=`` buffers and a 0xFF-filled workspace (of the no-chunking size and of the minimum size): the bits of a call
    with fresh buffers, for the default need mask and every single-bit mask, and again on a second call into the same, now used,
    buffers.  The fresh result itself is the reference's (lattice inputs)."""
    import torch
    inp, layers, grad_out = ref.edge_case("chunks_M100_S16_mixed_B2", True)
    res = ref.grouped_ref(orc, layers=layers, grad_out=grad_out, **inp)
    pooled, g = _forward(dev, inp, layers), _t(grad_out, dev)
    lo, hi = _ws_bytes(inp, layers)
    assert lo < hi
    for need in (None, ("feat",), ("xyz",), ("new_xyz",), ("params",)):
        fresh = _grouped(dev, inp, layers, pooled, g, need=need)
        _check_grouped(res, fresh, exact=True)
        for size in (hi, lo):
            ws = torch.full((size,), 0xFF, dtype=torch.uint8, device=dev)
            out = tuple(torch.full_like(t, NAN) for t in _flat(fresh))
            for call in ("first", "second"):
                got = _grouped(dev, inp, layers, pooled, g, need=need, out=out, workspace=ws)
                assert [t.data_ptr() for t in _flat(got)] == [t.data_ptr() for t in out], "the results are not the out= buffers"
                assert int(got[5].item()) == 0
                _bits_equal(got, fresh, f"need {need}, workspace of {size} bytes, {call} call")


def test_dirty_buffers_rows(sad, dev, orc):
    import torch
    from sad_amd import ops
    R, m = 1000, ref.ROWS_MASKS["alternating"]
    x, layers, grad_out = ref.rows_case(R, True)
    res = ref.rows_ref(orc, x, layers, m, grad_out)
    tx, tl, tg = _t(x, dev), _layers(layers, dev), _t(grad_out, dev)
    lo, hi = ops.mlp_grad_workspace_bytes(1, R, 1, ref.ROWS_DIMS, False, False)
    assert lo < hi
    for need in (None, ("feat",), ("params",)):
        fresh = ops.mlp_rows_grad(tx, tl, tg, relu_mask=m, need=need)
        _check_rows(res, fresh, exact=True)
        for size in (hi, lo):
            ws = torch.full((size,), 0xFF, dtype=torch.uint8, device=dev)
            out = tuple(torch.full_like(t, NAN) for t in _flat(fresh))
            for call in ("first", "second"):
                got = ops.mlp_rows_grad(tx, tl, tg, relu_mask=m, need=need, out=out, workspace=ws)
                assert [t.data_ptr() for t in _flat(got)] == [t.data_ptr() for t in out], "the results are not the out= buffers"
                _bits_equal(got, fresh, f"need {need}, workspace of {size} bytes, {call} call")


# ---- gap 3: a non-default current stream ----
def test_non_default_stream(sad, dev, orc):
    """Inputs produced on a side stream, the default stream busy, the calls (grouped whole and chunked, plain rows) on the side
    stream: the bits of the default-stream results (lattice inputs), mismatch == 0."""
    import torch
    from sad_amd import ops
    inp, layers, grad_out = ref.edge_case("chunks_M100_S16_mixed_B2", True)
    x, rl, rg = ref.rows_case(1000, True)
    mask = ref.ROWS_MASKS["alternating"]
    lo, hi = _ws_bytes(inp, layers)
    rlo, _ = ops.mlp_grad_workspace_bytes(1, 1000, 1, ref.ROWS_DIMS, False, False)

    def run():
        ti = {k: (None if v is None or isinstance(v, bool) else _t(v, dev).clone()) for k, v in inp.items()}
        tl, g = [(w.clone(), b.clone()) for w, b in _layers(layers, dev)], _t(grad_out, dev).clone()
        pooled = ops.PackedMLP(tl, True, dev).grouped(ti["xyz"], ti["feat"], ti["new_xyz"], ti["idx"], cnt=ti["cnt"])
        call = lambda **kw: ops.grouped_mlp_grad(ti["xyz"], ti["feat"], ti["new_xyz"], ti["idx"], ti["cnt"], tl, pooled, g, **kw)
        whole = call(budget_bytes=hi)
        chunked = call(workspace=torch.empty(lo, dtype=torch.uint8, device=dev))
        rows = ops.mlp_rows_grad(_t(x, dev).clone(), [(w.clone(), b.clone()) for w, b in _layers(rl, dev)], _t(rg, dev).clone(), relu_mask=mask,
                                 workspace=torch.empty(rlo, dtype=torch.uint8, device=dev))
        return whole, chunked, rows

    want = run()
    torch.cuda.synchronize()
    busy = torch.zeros(1 << 25, device=dev)
    st = torch.cuda.Stream(device=dev)
    for _ in range(16):                                          # work queued on the default stream while the side stream runs
        busy.add_(1.0)
    with torch.cuda.stream(st):
        got = run()
    st.synchronize()
    for name, a, b in zip(("whole", "chunked", "rows"), got, want):
        _bits_equal(a, b, f"{name} on a side stream")
    assert int(got[0][5].item()) == 0 and int(got[1][5].item()) == 0
    res = ref.grouped_ref(orc, layers=layers, grad_out=grad_out, **inp)
    _check_grouped(res, got[0], exact=True)
    _check_grouped(res, got[1], exact=True)
    _check_rows(ref.rows_ref(orc, x, rl, mask, rg), got[2], exact=True)
    torch.cuda.synchronize()
    assert bool((busy == 16.0).all())


# ---- gap 4: operand strides ----
@pytest.mark.parametrize("lattice", [False, True], ids=["general", "lattice"])
def test_strided_feat(sad, dev, orc, lattice, monkeypatch):
    """feat_pm as columns 2 .. 2 + C of NaN-filled rows of C + 5 floats: read in place (no strided-copy note), ld_feat = C + 5;
    as a transposed view: copied (the note is made).  Both give the packed call's result."""
    import torch
    from sad_amd import ops
    inp, layers, grad_out = ref.grouped_case("L3_C5_S33_mixed_B2", lattice)
    res = ref.grouped_ref(orc, layers=layers, grad_out=grad_out, **inp)
    pooled, g = _forward(dev, inp, layers), _t(grad_out, dev)
    packed = _grouped(dev, inp, layers, pooled, g)
    _check_grouped(res, packed, exact=lattice)
    notes = []
    monkeypatch.setattr(ops, "_unrecordable", notes.append)
    feat = _t(inp["feat"], dev)
    B, N, C = feat.shape
    wide = torch.full((B, N, C + 5), NAN, device=dev)
    wide[:, :, 2:2 + C] = feat
    view = feat.transpose(1, 2).contiguous().transpose(1, 2)
    assert view.stride(2) != 1 and torch.equal(view, feat)
    args = (_t(inp["xyz"], dev), _t(inp["new_xyz"], dev), _t(inp["idx"], dev), _t(inp["cnt"], dev), _layers(layers, dev))
    for f, copied in ((wide[:, :, 2:2 + C], False), (view, True)):
        del notes[:]
        for need in NEEDS:
            got = ops.grouped_mlp_grad(args[0], f, *args[1:], pooled, g, skip_empty=inp["skip_empty"], need=need)
            _check_grouped(res, got, exact=lattice)
            if lattice and need is None:
                _bits_equal(got, packed, "strided feat_pm against the packed call")
        assert ("feat_pm: strided copy" in notes) == copied, notes


@pytest.mark.parametrize("lattice", [False, True], ids=["general", "lattice"])
def test_strided_rows(sad, dev, orc, lattice, monkeypatch):
    """x of mlp_rows_grad as a column slice of wider NaN-filled rows (read in place at its row stride), grad_out in a wider
    NaN-filled buffer at col_off = 5, and both at once; with the minimum workspace too (chunks of 64 rows advance by the strides)."""
    import torch
    from sad_amd import ops
    R, m = 1000, ref.ROWS_MASKS["alternating"]
    x, layers, grad_out = ref.rows_case(R, lattice)
    res = ref.rows_ref(orc, x, layers, m, grad_out)
    tl = _layers(layers, dev)
    packed = ops.mlp_rows_grad(_t(x, dev), tl, _t(grad_out, dev), relu_mask=m)
    _check_rows(res, packed, exact=lattice)
    notes = []
    monkeypatch.setattr(ops, "_unrecordable", notes.append)
    C0, CL = x.shape[1], grad_out.shape[1]
    wide_x = torch.full((R, C0 + 5), NAN, device=dev)
    wide_x[:, 2:2 + C0] = _t(x, dev)
    wide_g = torch.full((R, CL + 7), NAN, device=dev)
    wide_g[:, 5:5 + CL] = _t(grad_out, dev)
    lo, _ = ops.mlp_grad_workspace_bytes(1, R, 1, ref.ROWS_DIMS, False, False)
    for xs, gs, off in ((wide_x[:, 2:2 + C0], _t(grad_out, dev), 0), (_t(x, dev), wide_g, 5), (wide_x[:, 2:2 + C0], wide_g, 5)):
        for kw in (dict(), dict(workspace=torch.empty(lo, dtype=torch.uint8, device=dev))):
            got = ops.mlp_rows_grad(xs, tl, gs, relu_mask=m, col_off=off, **kw)
            assert tuple(got[0].shape) == (R, C0) and got[0].is_contiguous()
            _check_rows(res, got, exact=lattice)
            if lattice:
                _bits_equal(got, packed, "strided rows against the packed call")
    assert notes == [], notes
