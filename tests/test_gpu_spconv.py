"""GPU parity of sparse 3-D convolution (SPEC.md §21) (-m gpu): the rulebook, the convolution, the dense scatter and the modules,
every output EQUAL to the reference (tests/spconv_ref.py) — integer arrays with np.array_equal, float arrays under ``==`` (the
sign of a zero is not specified, §21.2).  No tolerance anywhere.  Families and coverage: tests/spconv_cases.py."""
import numpy as np
import pytest

import spconv_cases as sc
import spconv_ref as ref
import voxel_ref

pytestmark = pytest.mark.gpu

F = np.float32


def _t(a, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _eq_int(got, want, what):
    got = got.cpu().numpy()
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    assert np.array_equal(got, want), f"{what}: {int((got != want).sum())} of {want.size} entries differ"


def _eq_f(got, want, what):
    got = got.cpu().numpy()
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    bad = ~(got == want)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {want.size} values differ, first at {np.argwhere(bad)[0].tolist()}"


@pytest.mark.parametrize("name", sorted(sc.FAMILIES))
def test_rulebook_conv_dense_every_family_and_geometry(dev, orc, name):
    from sad_amd import ops
    coors, off, G = sc.FAMILIES[name][0]()
    sc.check_coverage(name, coors, off, G)
    tc, to = _t(coors, dev), _t(off, dev)
    for gi, (gname, K, s, p, subm) in enumerate(sc.GEOMETRIES):
        w = f"{name}/{gname}"
        want = ref.index_vec(coors, off, G, K, s, p, subm)
        got = ops.sparse_conv_index(tc, to, G, K, s, p, subm)
        for g, x, n in zip(got, want, ("out_coors", "out_offsets", "nbr")):
            _eq_int(g, x, f"{w} {n}")
        oc, oo, nbr = want
        # with spare capacity (asynchronous form): the same rows, then -1
        if not subm:
            cap = len(oc) + 5
            g2 = ops.sparse_conv_index(tc, to, G, K, s, p, False, capacity=cap)
            _eq_int(g2[1], oo, f"{w} out_offsets (capacity)")
            _eq_int(g2[0][:len(oc)], oc, f"{w} out_coors (capacity)")
            _eq_int(g2[2][:len(oc)], nbr, f"{w} nbr (capacity)")
            assert bool((g2[0][len(oc):] == -1).all()) and bool((g2[2][len(oc):] == -1).all())
            if len(oc) > 3:
                g3 = ops.sparse_conv_index(tc, to, G, K, s, p, False, capacity=len(oc) - 3)
                _eq_int(g3[0], oc[:-3], f"{w} out_coors (short capacity)")
                _eq_int(g3[2], nbr[:-3], f"{w} nbr (short capacity)")
        # values over the REFERENCE's rulebook (an index fault cannot hide behind a matching convolution)
        cin, cout = sc.CHANNEL_PAIRS[gi % 6]
        Kvol = K[0] * K[1] * K[2]
        W, b = sc.make_layer(Kvol, cin, cout, gi)
        feat = sc.make_feat(len(coors), cin, gi + 1)
        res = sc.make_feat(len(oc), cout, gi + 2)
        out = ops.sparse_conv(_t(feat, dev), _t(nbr, dev), _t(W, dev), _t(b, dev), _t(res, dev), True)
        _eq_f(out, ref.conv(feat, nbr, W, b, res, True), f"{w} sparse_conv {cin}->{cout}")
        O = ref.geometry(G, K, s, p, subm)[4]
        f2 = sc.make_feat(len(oc), 3, gi + 3)
        _eq_f(ops.sparse_to_dense(_t(f2, dev), _t(oc, dev), _t(oo, dev), O), ref.to_dense(f2, oc, oo, O), f"{w} sparse_to_dense")


@pytest.mark.parametrize("cin,cout", sc.CHANNEL_PAIRS)
def test_conv_every_channel_pair(dev, orc, cin, cout):
    """Every channel pair on a submanifold and a strided rulebook, with and without bias, residual and ReLU."""
    from sad_amd import ops
    for name, (gname, K, s, p, subm) in (("random030", sc.GEOMETRIES[0]), ("tile129", sc.GEOMETRIES[2]), ("random002", sc.GEOMETRIES[0])):
        coors, off, G = sc.FAMILIES[name][0]()
        oc, oo, nbr = ref.index_vec(coors, off, G, K, s, p, subm)
        W, b = sc.make_layer(27, cin, cout, cin + cout)
        feat = sc.make_feat(len(coors), cin, cin)
        res = sc.make_feat(len(oc), cout, cout)
        tf, tn, tw, tb, tr = _t(feat, dev), _t(nbr, dev), _t(W, dev), _t(b, dev), _t(res, dev)
        packed = ops.PackedSparseWeight(tw, tb)
        for use_b, use_r, relu in ((False, False, False), (True, False, True), (False, True, False), (True, True, True)):
            want = ref.conv(feat, nbr, W, b if use_b else None, res if use_r else None, relu)
            got = ops.sparse_conv(tf, tn, tw, tb if use_b else None, tr if use_r else None, relu)
            _eq_f(got, want, f"{name}/{gname} {cin}->{cout} bias={use_b} residual={use_r} relu={relu}")
            if use_b:
                _eq_f(ops.sparse_conv(tf, tn, packed, None, tr if use_r else None, relu), want, f"{name}/{gname} {cin}->{cout} (packed)")


def test_from_voxels_after_voxel_index_and_reduce(dev, orc):
    import torch
    from sad_amd import ops, synth
    from sad_amd.spconv import SparseTensor, SubMConv3d
    pts = np.stack([synth.make_scene(s, 16384) for s in (0, 1, 2)])
    v, r, V = (0.4, 0.4, 0.5), (10.0, -8.0, -3.0, 26.0, 8.0, 1.0), 2048
    p, off = voxel_ref.ragged(pts)
    p2v, coors, count, num = voxel_ref.voxel_index(p, off, v, r, V)
    mean = voxel_ref.voxel_reduce(p, p2v, off, V, "mean")[0]
    wf, wc, wo = ref.from_voxels(mean, coors, num)
    G = tuple(int(g) for g in voxel_ref.grid_size(v, r)[::-1])
    tp, to = _t(p, dev), _t(off, dev)
    g_p2v, g_coors, g_count, g_num = ops.voxel_index(tp, to, v, r, V)
    g_mean = ops.voxel_reduce(tp, g_p2v, to, V, "mean")
    x = SparseTensor.from_voxels(g_mean, g_coors, g_num, G)
    _eq_f(x.feat, wf, "from_voxels feat")
    _eq_int(x.coors, wc, "from_voxels coors")
    _eq_int(x.offsets, wo, "from_voxels offsets")
    assert x.spatial_shape == G and x.batch_size == 3
    _eq_f(x.dense(), ref.to_dense(wf, wc, wo, G), "dense")
    assert tuple(x.bev().shape) == (3, wf.shape[1] * G[0], G[1], G[2]) and torch.equal(x.bev().reshape(x.dense().shape), x.dense())
    m = SubMConv3d(4, 16, 3, relu=True).to(dev)
    y = m(x)
    nbr = ref.index_vec(wc, wo, G, (3, 3, 3), subm=True)[2]
    _eq_f(y.feat, ref.conv(wf, nbr, m.weight.cpu().numpy(), m.bias.cpu().numpy(), None, True), "SubMConv3d on from_voxels")


def test_sequential_layer_by_layer_and_rulebook_cache(dev, orc):
    import torch
    from sad_amd import ops
    from sad_amd.spconv import SparseConv3d, SparseSequential, SparseTensor, SubMConv3d
    coors, off, G = sc.FAMILIES["synth"][0]()
    torch.manual_seed(0)
    net = SparseSequential(SubMConv3d(4, 16, 3, relu=True, indice_key="subm1"), SubMConv3d(16, 16, 3, relu=True, indice_key="subm1"),
                           SparseConv3d(16, 32, 3, 2, 1, relu=True, indice_key="down1"), SubMConv3d(32, 32, 3, bias=False, indice_key="subm2")).to(dev)
    feat = sc.make_feat(len(coors), 4, 9)
    x = SparseTensor(_t(feat, dev), _t(coors, dev), _t(off, dev), G)
    f, c, o, g = feat, coors, off, G
    for li, m in enumerate(net):
        x = m(x)
        oc, oo, nbr = ref.index_vec(c, o, g, m.kernel_size, m.stride, m.padding, m.subm)
        f = ref.conv(f, nbr, m.weight.cpu().numpy(), None if m.bias is None else m.bias.cpu().numpy(), None, m.relu)
        g = ref.geometry(g, m.kernel_size, m.stride, m.padding, m.subm)[4]
        c, o = oc, oo
        _eq_f(x.feat, f, f"layer {li} feat")
        _eq_int(x.coors, c, f"layer {li} coors")
        _eq_int(x.offsets, o, f"layer {li} offsets")
        assert x.spatial_shape == g
    assert sorted(x.rulebooks) == ["down1", "subm1", "subm2"]
    # the whole chain again through forward(): the cache is hit (same tensors come back) and equals a rebuilt rulebook
    x0 = SparseTensor(_t(feat, dev), _t(coors, dev), _t(off, dev), G)
    y = net(x0)
    _eq_f(y.feat, f, "SparseSequential")
    cached = x0.rulebooks["subm1"]
    rebuilt = ops.sparse_conv_index(x0.coors, x0.offsets, G, 3, subm=True)
    assert torch.equal(cached.nbr, rebuilt[2]) and cached.out_coors is x0.coors
    y1 = net[1](net[0](x0))
    assert x0.rulebooks["subm1"] is cached and y1.coors is x0.coors
    d = x0.rulebooks["down1"]
    r2 = ops.sparse_conv_index(x0.coors, x0.offsets, G, 3, 2, 1)
    assert torch.equal(d.out_coors, r2[0]) and torch.equal(d.out_offsets, r2[1]) and torch.equal(d.nbr, r2[2])
    with pytest.raises(ValueError):
        SubMConv3d(16, 16, (1, 3, 3), indice_key="subm1").to(dev)(net[0](x0))          # the key belongs to another geometry
    # residual input of a layer
    res = sc.make_feat(len(coors), 16, 4)
    y2 = net[1](net[0](x0), residual=_t(res, dev))
    nbr = ref.index_vec(coors, off, G, (3, 3, 3), subm=True)[2]
    f1 = ref.conv(feat, nbr, net[0].weight.cpu().numpy(), net[0].bias.cpu().numpy(), None, True)
    _eq_f(y2.feat, ref.conv(f1, nbr, net[1].weight.cpu().numpy(), net[1].bias.cpu().numpy(), res, True), "residual layer")


def test_non_default_stream(dev, orc):
    import torch
    from sad_amd import ops
    coors, off, G = sc.FAMILIES["random030"][0]()
    gname, K, s, p, subm = sc.GEOMETRIES[2]
    oc, oo, nbr = ref.index_vec(coors, off, G, K, s, p, subm)
    W, b = sc.make_layer(27, 16, 32, 0)
    feat = sc.make_feat(len(coors), 16, 1)
    tc, to, tf, tw, tb = _t(coors, dev), _t(off, dev), _t(feat, dev), _t(W, dev), _t(b, dev)
    torch.cuda.synchronize()
    st = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(st):
        g = ops.sparse_conv_index(tc, to, G, K, s, p, subm)
        out = ops.sparse_conv(tf, g[2], tw, tb, None, True)
        O = ref.geometry(G, K, s, p)[4]
        dense = ops.sparse_to_dense(out, g[0], g[1], O)
    st.synchronize()
    _eq_int(g[0], oc, "out_coors (stream)")
    _eq_int(g[2], nbr, "nbr (stream)")
    want = ref.conv(feat, nbr, W, b, None, True)
    _eq_f(out, want, "sparse_conv (stream)")
    _eq_f(dense, ref.to_dense(want, oc, oo, O), "sparse_to_dense (stream)")


def test_abi_argument_errors(dev):
    """SAD_EINVAL / SAD_EUNSUPPORTED of the C-ABI that the Python layer cannot reach (it checks first)."""
    import ctypes
    import torch
    from sad_amd import _lib
    L = _lib.lib()
    i3 = lambda *a: (ctypes.c_int * 3)(*a)
    n = ctypes.c_size_t(0)
    assert L.sad_spconv_workspace_bytes(10, 1, i3(3, 3, 3), i3(1, 1, 1), 1, ctypes.byref(n)) == 0 and n.value > 0
    assert L.sad_spconv_workspace_bytes(10, 1, i3(4, 3, 3), i3(1, 1, 1), 0, ctypes.byref(n)) == -2 and b"kernel size" in L.sad_last_error()
    assert L.sad_spconv_workspace_bytes(10, 1, i3(2, 3, 3), None, 1, ctypes.byref(n)) == -1
    assert L.sad_spconv_workspace_bytes(10, 0, i3(3, 3, 3), None, 1, ctypes.byref(n)) == -1
    assert L.sad_spconv_workspace_bytes(1 << 30, 1, i3(3, 3, 3), None, 1, ctypes.byref(n)) == -2
    assert L.sad_spconv_packed_floats(27, 257, 16) == 0 and L.sad_spconv_packed_floats(27, 4, 16) == 32 + 27 * 256
    buf = torch.zeros((1024,), dtype=torch.float32, device=dev)
    assert L.sad_spconv_pack_f32(buf.data_ptr(), None, 27, 300, 16, buf.data_ptr(), None) == -2
    assert L.sad_spconv_f32(buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), None, 0, 4, 4, 28, 4, 4, buf.data_ptr(), None) == -2
    assert L.sad_spconv_f32(buf.data_ptr(), buf.data_ptr(), None, None, 0, 4, 4, 27, 4, 4, buf.data_ptr(), None) == -1
    assert L.sad_spconv_index_subm(buf.data_ptr(), buf.data_ptr(), 4, 1, i3(1 << 11, 1 << 11, 1 << 11), i3(3, 3, 3), buf.data_ptr(), buf.data_ptr(),
                                   None) == -2
    assert L.sad_sparse_to_dense_workspace_bytes(2, i3(1 << 11, 1 << 11, 1 << 10), ctypes.byref(n)) == -2
