"""Oracle parity of the exact configuration bench.py times (BASELINE.json configs[2]): batch 32 x
16 384-point KITTI-shaped scenes, autotuned geometries, ``SADDetector.submit()`` on alternating main
streams with sampling streams, merged ``grouped_multi`` dispatches and the fused ``cluster.agg+head``
chain (no trace).  Parity is against this repository's spec-oracle; the upstream reference
(``/root/reference/README.md:1-2``) ships no implementation to compare with.  (-m gpu)"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
TOL = 1e-4


def _t(a, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _rel(got, want):
    return float((np.abs(got.astype(np.float64) - want.astype(np.float64)) / (1.0 + np.abs(want))).max())


def _agg_head_layers(w):
    return list(w["cluster.agg"]) + list(w["head"])


@pytest.mark.parametrize("rows", [1000, 8192])
def test_fused_agg_head_chain_every_geometry(orc, sad, dev, rows):
    """The fused cluster aggregation + head chain (1536 -> 512 -> 256 -> 256 -> 10, last layer
    linear, layer 0 staged in k-chunks) on plain rows, for EVERY geometry code the autotuner may pick
    — including +100000 (flexible items), +200000 (two output tiles per wave, the code the round-1
    bench picked) and +300000 — bit-exact against the oracle's fmaf chains.  8192 rows = the 32 x 256
    candidates of the timed batch; 1000 rows leaves a ragged last tile."""
    from sad_amd import _lib, config, ops, synth
    w = synth.make_weights(config.KITTI, 0)
    layers = _agg_head_layers(w)
    L = len(layers)
    mask = (1 << (L - 1)) - 1
    rng = np.random.default_rng(rows)
    # post-ReLU pooled features are >= 0 with many exact zeros: mimic that
    x = np.maximum(rng.normal(size=(rows, layers[0][0].shape[1])).astype(np.float32), 0.0)
    want = orc.mlp_rows(x, layers, relu_mask=mask)
    net = ops.PackedMLP(layers, False, dev, relu_mask=mask, name="cluster.agg+head")
    X = _t(x, dev)
    ran, refused = [], []
    try:
        for code in [0] + list(ops.PackedMLP._CANDIDATES):
            _lib.set_option("mlp_force", code)
            try:
                got = net.rows(X).cpu().numpy()
            except RuntimeError as e:
                assert "(-2)" in str(e), f"geometry {code}: {e}"      # SAD_EUNSUPPORTED only
                refused.append(code)
                continue
            assert np.array_equal(got, want), f"plain geometry {code}: max diff {np.abs(got - want).max():.3e}"
            ran.append(code)
    finally:
        _lib.set_option("mlp_force", 0)
    print(f"[parity] fused agg+head rows={rows}: {len(ran)} geometries bit-exact, {len(refused)} refused (LDS)")
    # +200000 (two output tiles per wave) is the family the autotuner picks for this chain; codes whose
    # LDS image of the 1536-channel input does not fit are refused with SAD_EUNSUPPORTED (never wrong)
    assert any(c // 100000 == 2 for c in ran), f"no +200000 geometry ran: {ran}"
    assert 200831 in ran, "the geometry the benchmark's autotuner picks was refused"
    assert len(ran) >= 4, f"only {len(ran)} geometries ran: {ran}"   # a 1536-channel input leaves few wave grids that fit LDS
    print(f"[parity] ran: {ran}")


@pytest.mark.parametrize("dims,mask", [([128, 64], None), ([384, 128], None), ([768, 256], None),
                                       ([256, 128, 6], 0b01), ([512, 256, 256, 10], 0b011)])
def test_plain_chains_of_the_detector_every_geometry(orc, sad, dev, dims, mask):
    """The other plain-row chains of the timed step (stage aggregations, candidate MLP, unfused
    head) under every geometry code including the flag codes."""
    from sad_amd import _lib, ops, synth
    rng = np.random.default_rng(sum(dims))
    layers = synth.make_mlp_weights(dims, rng)
    x = rng.normal(size=(777, dims[0])).astype(np.float32)
    want = orc.mlp_rows(x, layers, relu_mask=mask)
    net = ops.PackedMLP(layers, False, dev, relu_mask=mask)
    X = _t(x, dev)
    ran = 0
    try:
        for code in ops.PackedMLP._CANDIDATES:
            _lib.set_option("mlp_force", code)
            try:
                got = net.rows(X).cpu().numpy()
            except RuntimeError as e:
                assert "(-2)" in str(e), f"geometry {code}: {e}"
                continue
            assert np.array_equal(got, want), f"plain {dims} geometry {code}"
            ran += 1
    finally:
        _lib.set_option("mlp_force", 0)
    assert ran >= 10, f"only {ran} geometries ran"


def test_detector_kitti_f32_cluster_head_boxes(orc, sad, dev):
    """f32 twin of test_detector_bf16_stagewise at full KITTI size: SA1-SA3, then the candidate MLP,
    candidates + adaptive radius (exact), BOTH adaptive ball-query index sets (exact), pooled
    cluster features, aggregation, head (<= 1e-4) and boxes, each stage fed with the GPU's own
    upstream tensors; plus the fused (trace-free) path's boxes against the unfused ones."""
    import torch
    from sad_amd import config, synth
    from sad_amd.detector import SADDetector
    cfg = config.KITTI
    B = 2
    w = synth.make_weights(cfg, 0)
    pts = synth.make_batch(40, B)
    det = SADDetector(cfg, w, dev)
    tr = {}
    P = _t(pts, dev)
    boxes = det(P, tr)
    torch.cuda.synchronize()
    xyz = np.ascontiguousarray(pts[:, :, :3])
    feat = np.ascontiguousarray(pts[:, :, 3:])
    for si, st in enumerate(cfg.stages):
        name = f"sa{si + 1}"
        onx, onf = orc.sa_module(xyz, feat, st, w, name)
        np.testing.assert_array_equal(tr[name]["new_xyz"].cpu().numpy(), onx)
        got = tr[name]["out"].cpu().numpy()
        assert _rel(got, onf) <= TOL, name
        xyz, feat = onx, got
    c = tr["cluster"]
    K = cfg.n_cand
    want_c = orc.mlp_rows(np.ascontiguousarray(feat[:, :K]).reshape(B * K, -1), w["cand"],
                          relu_mask=(1 << (len(w["cand"]) - 1)) - 1).reshape(B, K, -1)
    gc = c["c"].cpu().numpy()
    assert _rel(gc, want_c) <= TOL
    cand, rad = orc.candidates(xyz, gc, cfg.shift_max, cfg.r_min, cfg.r_max, cfg.anchor_car)
    np.testing.assert_array_equal(c["cand"].cpu().numpy(), cand)
    np.testing.assert_array_equal(c["radius"].cpu().numpy(), rad)
    assert rad.min() < rad.max(), "adaptive radius is constant: the size-adaptive path is not exercised"
    idxs = [i.cpu().numpy() for i in c["ball_idx"]]
    cat = np.empty((B, K, sum(m[-1] for m in cfg.cluster_mlps)), np.float32)
    off = 0
    for bi, (sc, s, got) in enumerate(zip(cfg.cluster_scales, cfg.cluster_nsamples, idxs)):
        np.testing.assert_array_equal(got, orc.ball_query((np.float32(sc) * rad).astype(np.float32), s, xyz, cand))
        orc.sa_group_mlp_max(xyz, feat, cand, got, w[f"cluster.b{bi}"], out=cat, col_off=off)
        off += cfg.cluster_mlps[bi][-1]
    gcat = c["cat"].cpu().numpy()
    assert _rel(gcat, cat) <= TOL
    print(f"[parity] KITTI f32 cluster pooled bit-exact={np.array_equal(gcat, cat)}")
    want_cf = orc.mlp_rows(gcat.reshape(B * K, -1), w["cluster.agg"])
    gcf = c["cfeat"].cpu().numpy().reshape(B * K, -1)
    assert _rel(gcf, want_cf) <= TOL
    want_h = orc.mlp_rows(gcf, w["head"], relu_mask=(1 << (len(w["head"]) - 1)) - 1).reshape(B, K, -1)
    gh = c["head"].cpu().numpy()
    assert _rel(gh, want_h) <= TOL
    print(f"[parity] KITTI f32 head bit-exact={np.array_equal(gh, want_h)}")
    want_b = orc.decode_boxes(cand, gh, [v for a in cfg.anchors for v in a])
    b = boxes.cpu().numpy()
    np.testing.assert_array_equal(b[..., 8], want_b[..., 8])
    assert _rel(b, want_b) <= TOL
    # the product default (no trace): fused cluster.agg+head chain -> same boxes, bit for bit
    fused = det(P)
    torch.cuda.synchronize()
    assert det.agg_head is not None
    assert torch.equal(fused, boxes), "fused cluster.agg+head chain differs from the unfused pair"
    # ... and end to end against the oracle run from the raw points
    full = orc.detector_forward(pts, cfg, w)
    np.testing.assert_array_equal(b[..., 8], full[..., 8])
    assert _rel(b, full) <= TOL


def test_bench_configuration_b32_submit_autotuned(orc, sad, dev):
    """BASELINE configs[2] exactly as bench.py runs it: B = 32 KITTI scenes, det.autotune(), then
    det.submit() several times with NO trace (fused agg+head chain, merged branch dispatches, two
    main streams, four sampling streams).  Every submitted batch must give the oracle's boxes
    (<= 1e-4, labels exact) — the oracle runs the dense SPEC path from the raw points."""
    import torch
    from sad_amd import config, synth
    from sad_amd.detector import SADDetector
    cfg = config.KITTI
    B = 32
    w = synth.make_weights(cfg, 0)
    pts = synth.make_batch(0, B)
    want = orc.detector_forward(pts, cfg, w)
    det = SADDetector(cfg, w, dev, overlap_fps=True, n_fps_streams=4, n_main_streams=2)
    P = _t(pts, dev)
    torch.cuda.synchronize()
    tuned = det.autotune(P)
    assert "cluster.agg+head" in tuned, f"the fused chain was not tuned: {sorted(tuned)}"
    print(f"[parity] tuned geometry: {tuned}")
    # the pooling buffers of the overlapped path are never zero-filled (the row-packing scans prepare the few groups that are
    # combined with an atomic max): NaN in everything the kernels do not write must not reach the boxes
    det.poison_buffers = True
    import os
    stress = int(os.environ.get("SAD_STRESS", "1"))     # SAD_STRESS=10: soak (the kernels that pull work from queues,
    outs = []                                           # overlap of batches on two main + four sampling streams)
    for _ in range(4 * stress):
        outs.append(det.submit(P)[0])
        if len(outs) % 6 == 0:
            torch.cuda.synchronize()                    # (bounded queue depth, as bench.py)
    torch.cuda.synchronize()
    for i, out in enumerate(outs):
        got = out.cpu().numpy()
        assert got.shape == (B, cfg.n_cand, 9)
        np.testing.assert_array_equal(got[..., 8], want[..., 8], err_msg=f"labels, submit {i}")
        r = _rel(got, want)
        print(f"[parity] B=32 submit {i}: max rel diff vs oracle {r:.3e}")
        assert r <= TOL, f"submit {i}: boxes differ from the oracle: {r:.3e}"
    assert all(torch.equal(outs[0], o) for o in outs[1:]), "consecutive submits differ"
    # a second shard (other scenes), heuristic geometry on the same detector shapes
    pts2 = synth.make_batch(32, B)
    want2 = orc.detector_forward(pts2, cfg, w)
    out2, ev = det.submit(_t(pts2, dev))
    ev.synchronize()
    got2 = out2.cpu().numpy()
    np.testing.assert_array_equal(got2[..., 8], want2[..., 8])
    assert _rel(got2, want2) <= TOL


@pytest.mark.parametrize("pack_features", [True, False])
def test_unaligned_feature_view_with_poisoned_buffers(orc, sad, dev, pack_features):
    """Regression (round-3 advisor finding): with 4 extra channels the SA1 feature view of [B,N,7] points has row stride 7
    and a 12-byte offset, so the register-resident kernels cannot fetch it in 16-byte chunks.  The row-packing scan used to
    prepare the pooling buffer for them anyway while the tiled kernel ran (it max-combines into memory it expects to be
    ZERO) — silently wrong or NaN results on the default submit() path.  Now ``wants_prescan`` and ``_grouped_args``
    share one layout predicate and the detector packs the features once; both routes (packed copy -> table kernels;
    strided view handed straight to a stage -> tiled kernel on a zero-filled slice) must give the oracle's results with
    every uninitialised buffer poisoned with NaN.  TINY topology with ``in_feat = 4``: the SA1 chains are the nuScenes
    shapes (7 -> 16 -> 16 -> 32), sizes the oracle finishes in a second."""
    import dataclasses
    import torch
    from sad_amd import config, ops, synth
    from sad_amd.detector import SADDetector
    cfg = dataclasses.replace(config.TINY, in_feat=4)
    B = 3
    w = synth.make_weights(cfg, 0)
    base = synth.make_tiny_batch(40, B, cfg.n_points)
    extra = np.random.default_rng(7).uniform(0.0, 1.0, (B, cfg.n_points, 3)).astype(np.float32)
    pts = np.ascontiguousarray(np.concatenate([base, extra], 2))           # [B,N,7]
    otr = {}
    want = orc.detector_forward(pts, cfg, w, otr)
    P = _t(pts, dev)
    if pack_features:
        det = SADDetector(cfg, w, dev, overlap_fps=True, n_fps_streams=2, n_main_streams=2)
        det.poison_buffers = True
        assert det.stages[0].branches[0].preferred_geometry % 1000 in (2, 3, 4), "the SA1 shape is expected to be a compiled one"
        outs = [det.submit(P)[0] for _ in range(3)]
        torch.cuda.synchronize()
        for i, out in enumerate(outs):
            got = out.cpu().numpy()
            assert np.isfinite(got).all(), f"submit {i}: non-finite boxes"
            np.testing.assert_array_equal(got[..., 8], want[..., 8], err_msg=f"labels, submit {i}")
            assert _rel(got, want) <= TOL, f"submit {i}: {_rel(got, want):.3e}"
    else:
        # the stage on its own, fed the strided view: query(prescan=True, cat=<NaN buffer>, feat=view) must not prepare the
        # buffer for a table kernel that will not run
        m = SADDetector(cfg, w, dev).stages[0]
        xyz = P[:, :, :3].contiguous()
        view = P[:, :, 3:]
        assert not ops.PackedMLP.feat_fits_table_kernels(view.shape[2], view.stride(1), view.data_ptr())
        _, new_xyz = m.sample(xyz)
        cat = torch.full((B, m.stage.npoint, m.cat_channels), float("nan"), dtype=torch.float32, device=dev)
        q = m.query(xyz, new_xyz, prescan=True, cat=cat, feat=view)
        assert all(t is None for t in q[2]), "a row-packing table was made for a layout the table kernels cannot read"
        out = m.group_and_pool(xyz, view, new_xyz, query=q, cat=cat)
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy(), otr["sa1"]["out"]), "SA1 features differ from the oracle"
        # and the backstop: a table handed to a chain whose kernel packs for itself is refused, not run
        idxs, cnts = q[0], q[1]
        ws = ops.rowscan_multi(idxs[:1], cnts[:1], xyz.shape[1])[0]
        with pytest.raises(RuntimeError, match="packs for itself"):
            m.branches[0].grouped(xyz, view, new_xyz, idxs[0], out=torch.zeros_like(cat), cnt=cnts[0], ws=ws)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_one_log_entry_per_dispatch_and_rerun_reproduces(sad, dev, dtype):
    """The bookkeeping of an MLP dispatch, with the switches set through ``ops``: a single ``grouped`` call and a merged
    ``grouped_multi`` each append exactly ONE entry to ``ops.LAUNCH_LOG`` and to ``ops.RERUN_LOG``, named ``name`` / ``"a+b"``,
    and the RERUN_LOG entry's fn() enqueues the same dispatch again: onto a re-zeroed ``out`` it reproduces the result bit for
    bit.  One scene of 128 points, 16 groups of up to 8 samples (some short), two 3-layer chains: what can go wrong here is
    bookkeeping (a switch read from the wrong module, a closure that lost an object, a double append), not arithmetic."""
    import torch
    from sad_amd import ops, synth
    rng = np.random.default_rng(128)
    B, N, M, S, C = 1, 128, 16, 8, 4
    xyz = rng.random((B, N, 3), dtype=np.float32)
    X, F, Cn = _t(xyz, dev), _t(rng.normal(size=(B, N, C)).astype(np.float32), dev), _t(xyz[:, :M], dev)
    (idx,), (cnt,) = ops.ball_query_multi([0.25], [S], X, Cn, return_counts=True)
    assert bool((cnt < S).any()) and bool((cnt == S).any()), "want groups short of S beside full ones"
    cls = ops.PackedMLP if dtype == "f32" else ops.PackedMLPBf16
    nets = [cls(synth.make_mlp_weights([C + 3] + m, rng), True, dev, name=n) for n, m in (("a", [16, 16, 32]), ("b", [32, 32, 64]))]
    one = torch.zeros(B, M, 32, device=dev)
    both = torch.zeros(B, M, 96, device=dev)
    assert ops.RERUN_LOG is None and ops.LAUNCH_LOG is None
    try:
        ops.RERUN_LOG, ops.LAUNCH_LOG = [], []
        nets[0].grouped(X, F, Cn, idx, out=one, col_off=0, cnt=cnt)
        assert [e[0] for e in ops.RERUN_LOG] == ["a"] and [e[:2] for e in ops.LAUNCH_LOG] == [("mlp", "a")]
        ops.grouped_multi([(nets[0], X, F, Cn, idx, both, 0, cnt), (nets[1], X, F, Cn, idx, both, 32, cnt)])
        assert [e[0] for e in ops.RERUN_LOG] == ["a", "a+b"]
        assert [e[:2] for e in ops.LAUNCH_LOG] == [("mlp", "a"), ("mlp", "a+b")]
        reruns, ops.RERUN_LOG, ops.LAUNCH_LOG = ops.RERUN_LOG, None, None
        for (name, fn), out in zip(reruns, (one, both)):
            first = out.clone()
            assert bool((first > 0).any()), name
            out.zero_()
            fn()
            torch.cuda.synchronize()
            assert torch.equal(out, first), f"{dtype} {name}: the re-enqueued dispatch differs"
        if dtype == "f32":      # (the merged dispatch writes the single launch's bits: test_multi_chain_dispatch_matches_single_launches)
            assert torch.equal(both[:, :, :32], one)
    finally:
        ops.RERUN_LOG, ops.LAUNCH_LOG = None, None
