"""``shared_mlp.BranchGroup`` on the GPU (-m gpu): the two forms of the branches' forward agree bit for bit."""
import pytest


@pytest.mark.gpu
def test_branch_group_forms_agree(sad, dev, monkeypatch):
    """Two branches, S = (4, 8), widths (8, 16) and (8, 33) (33 crosses a 32-channel tile), groups with no member and full groups:
    the sliced buffer of the ``no_grad`` form equals the concatenation of each branch's own ``grouped``, the training form
    equals the ``no_grad`` form and its backward reaches every parameter; one branch returns its own tensor."""
    import torch
    from sad_amd import ops
    from sad_amd.shared_mlp import BranchGroup, SharedMLP
    B, N, M, C, S = 2, 64, 8, 3, (4, 8)
    torch.manual_seed(0)
    xyz = torch.rand(B, N, 3).to(dev)
    feat = torch.randn(B, N, C).to(dev)
    new_xyz = xyz[:, :M].clone()
    new_xyz[0, 0] = 10.0                                                  # a centroid with nothing in reach
    idxs, cnts = ops.ball_query_multi((0.3, 0.6), S, xyz, new_xyz, None, return_counts=True)
    for cnt, s in zip(cnts, S):
        assert int(cnt.min()) == 0 and int(cnt.max()) == s
    group = BranchGroup([SharedMLP([C + 3, 8, 16], True), SharedMLP([C + 3, 8, 33], True)]).to(dev)
    assert group.cat_channels == 49
    with torch.no_grad():
        got = group(xyz, feat, new_xyz, idxs, cnts)
        want = torch.cat([mlp.grouped(xyz, feat, new_xyz, idx, cnt) for mlp, idx, cnt in zip(group, idxs, cnts)], 2)
    assert tuple(got.shape) == (B, M, 49) and got.dtype == torch.float32 and not got.requires_grad
    assert torch.equal(got, want) and bool(got.abs().sum() > 0)
    assert torch.equal(group(xyz, feat, new_xyz, idxs, cnts), got)        # grad mode on, nothing requires grad: the same form
    group.requires_grad_(True)
    out = group(xyz, feat, new_xyz, idxs, cnts)
    assert out.requires_grad and torch.equal(out, got)
    out.backward(torch.randn(B, M, 49).to(dev))
    for name, p in group.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), name
    # one branch: its own pooled tensor, no concatenation and no copy
    one = BranchGroup([SharedMLP([C + 3, 8, 16], True)]).to(dev).requires_grad_(True)
    seen, real = [], one[0].grouped
    monkeypatch.setattr(one[0], "grouped", lambda *a, **k: (seen.append(real(*a, **k)), seen[-1])[1])
    out1 = one(xyz, feat, new_xyz, idxs[:1], cnts[:1])
    assert len(seen) == 1 and out1.data_ptr() == seen[0].data_ptr() and out1.requires_grad
    with torch.no_grad():
        assert torch.equal(one(xyz, feat, new_xyz, idxs[:1], cnts[:1]), out1)
