"""The Python training layer without a GPU: the parameter names of the trainable modules (a checkpoint's keys), the one
"does this call train?" predicate, the default weights of a stage, the scaling of the loss Functions' saved gradients against
the expressions it replaced, and the refusals of the backward operators that moved into ``ops``."""
import numpy as np
import pytest

import detector_train_ref as dref

# (name, shape) of every parameter, as printed by ``named_parameters()`` before the branch lists became ``BranchGroup``s
DETECTOR_PARAMS = [
    ("stages.0.branches.0.weight.0", (8, 4)), ("stages.0.branches.0.weight.1", (16, 8)),
    ("stages.0.branches.0.bias.0", (8,)), ("stages.0.branches.0.bias.1", (16,)),
    ("stages.0.branches.1.weight.0", (8, 4)), ("stages.0.branches.1.weight.1", (16, 8)),
    ("stages.0.branches.1.bias.0", (8,)), ("stages.0.branches.1.bias.1", (16,)),
    ("stages.0.agg.weight.0", (16, 32)), ("stages.0.agg.bias.0", (16,)),
    ("stages.1.branches.0.weight.0", (16, 19)), ("stages.1.branches.0.weight.1", (16, 16)),
    ("stages.1.branches.0.bias.0", (16,)), ("stages.1.branches.0.bias.1", (16,)),
    ("stages.1.branches.1.weight.0", (16, 19)), ("stages.1.branches.1.weight.1", (33, 16)),
    ("stages.1.branches.1.bias.0", (16,)), ("stages.1.branches.1.bias.1", (33,)),
    ("stages.1.agg.weight.0", (24, 49)), ("stages.1.agg.bias.0", (24,)),
    ("stages.2.branches.0.weight.0", (16, 27)), ("stages.2.branches.0.weight.1", (32, 16)),
    ("stages.2.branches.0.bias.0", (16,)), ("stages.2.branches.0.bias.1", (32,)),
    ("stages.2.branches.1.weight.0", (16, 27)), ("stages.2.branches.1.weight.1", (33, 16)),
    ("stages.2.branches.1.bias.0", (16,)), ("stages.2.branches.1.bias.1", (33,)),
    ("stages.2.agg.weight.0", (20, 65)), ("stages.2.agg.bias.0", (20,)),
    ("cand.weight.0", (16, 20)), ("cand.weight.1", (6, 16)), ("cand.bias.0", (16,)), ("cand.bias.1", (6,)),
    ("cluster_branches.0.weight.0", (16, 23)), ("cluster_branches.0.weight.1", (33, 16)),
    ("cluster_branches.0.bias.0", (16,)), ("cluster_branches.0.bias.1", (33,)),
    ("cluster_branches.1.weight.0", (10, 23)), ("cluster_branches.1.weight.1", (33, 10)), ("cluster_branches.1.weight.2", (40, 33)),
    ("cluster_branches.1.bias.0", (10,)), ("cluster_branches.1.bias.1", (33,)), ("cluster_branches.1.bias.2", (40,)),
    ("cluster_agg.weight.0", (33, 73)), ("cluster_agg.bias.0", (33,)),
    ("head.weight.0", (16, 33)), ("head.weight.1", (10, 16)), ("head.bias.0", (16,)), ("head.bias.1", (10,)),
]
# SAModuleMSGTrain(4, SAStage(16, (0.5, 1.0), (4, 8), ((8, 16), (8, 12, 33)), 24), "cpu")
STAGE_PARAMS = [
    ("branches.0.weight.0", (8, 7)), ("branches.0.weight.1", (16, 8)), ("branches.0.bias.0", (8,)), ("branches.0.bias.1", (16,)),
    ("branches.1.weight.0", (8, 7)), ("branches.1.weight.1", (12, 8)), ("branches.1.weight.2", (33, 12)),
    ("branches.1.bias.0", (8,)), ("branches.1.bias.1", (12,)), ("branches.1.bias.2", (33,)),
    ("agg.weight.0", (24, 49)), ("agg.bias.0", (24,)),
]


def _named(module):
    return {(n, tuple(p.shape)) for n, p in module.named_parameters()}


def test_parameter_names_are_the_checkpoint_keys(sad):
    from sad_amd.config import SAStage
    from sad_amd.detector_train import SADDetectorTrain
    from sad_amd.sa_module import SAModuleMSGTrain
    from sad_amd.shared_mlp import BranchGroup
    det = SADDetectorTrain(dref.small_config(), "cpu")
    assert _named(det) == set(DETECTOR_PARAMS) and len(list(det.parameters())) == len(DETECTOR_PARAMS)
    assert isinstance(det.cluster_branches, BranchGroup) and det.cluster_branches.cat_channels == 33 + 40
    sa = SAModuleMSGTrain(4, SAStage(16, (0.5, 1.0), (4, 8), ((8, 16), (8, 12, 33)), 24), "cpu")
    assert _named(sa) == set(STAGE_PARAMS) and len(list(sa.parameters())) == len(STAGE_PARAMS)
    assert isinstance(sa.branches, BranchGroup) and sa.branches.cat_channels == sa.cat_channels == 49 and sa.out_channels == 24
    assert not any(p.requires_grad for p in det.parameters())


def test_wants_grad_truth_table(sad):
    import torch
    from torch import nn
    from sad_amd.shared_mlp import wants_grad
    plain, live = torch.zeros(2), torch.zeros(2, requires_grad=True)
    frozen, trained = nn.Linear(2, 2).requires_grad_(False), nn.Linear(2, 2).requires_grad_(False)
    trained.bias.requires_grad_(True)
    assert not wants_grad() and not wants_grad(plain) and not wants_grad(None, plain, None)
    assert not wants_grad(plain, module=frozen) and not wants_grad(module=frozen)
    assert wants_grad(live) and wants_grad(None, plain, live) and wants_grad(live, module=frozen)
    assert wants_grad(module=trained) and wants_grad(plain, None, module=trained)
    with torch.no_grad():
        assert not wants_grad(live) and not wants_grad(module=trained) and not wants_grad(live, None, module=trained)


def test_stage_weights_are_the_inline_draws(sad):
    """``default_rng(seed)``, the branches in order, then the aggregation layer: the lines both constructors carried."""
    from sad_amd.config import SAStage
    from sad_amd.sa_module import stage_weights
    from sad_amd.synth import make_mlp_weights
    for c, stage in ((4, SAStage(16, (0.5, 1.0), (4, 8), ((8, 16), (8, 12, 33)), 24)), (0, SAStage(8, (0.5,), (4,), ((8, 9),), 0))):
        rng = np.random.default_rng(0)
        want = {f"b{i}": make_mlp_weights([c + 3] + list(m), rng) for i, m in enumerate(stage.mlps)}
        if stage.agg:
            want["agg"] = make_mlp_weights([sum(m[-1] for m in stage.mlps), stage.agg], rng)
        got = stage_weights(c, stage, 0)
        assert list(got) == list(want) and ("agg" in got) == bool(stage.agg)
        for k in want:
            assert len(got[k]) == len(want[k])
            for (gw, gb), (ww, wb) in zip(got[k], want[k]):
                assert gw.dtype == ww.dtype and np.array_equal(gw, ww) and np.array_equal(gb, wb)
        assert not np.array_equal(stage_weights(c, stage, 1)["b0"][0][0], want["b0"][0][0])


def _rand(gen, *shape):
    import torch
    return torch.randn(*shape, generator=gen, dtype=torch.float32)


def _scaled(grad, w):
    """The helper the four backwards used: grad [B,...] times w [B], broadcast per scene."""
    return grad * w.view(-1, *([1] * (grad.dim() - 1)))


@pytest.mark.parametrize("optional", [False, True])
def test_scale_saved_equals_the_four_backwards(sad, optional):
    """``autograd._scale_saved`` with each Function's table against that Function's former backward, written out."""
    import torch
    from sad_amd import autograd
    gen = torch.Generator().manual_seed(5)
    B = 2
    # anchor head: saved map i scales with column i; dir is optional
    saved = [_rand(gen, B, 6, 3, 2) for _ in range(3 if optional else 2)]
    gl = _rand(gen, B, 3)
    got = autograd._scale_saved(saved, gl, autograd.AnchorHeadLoss.table)
    assert sorted(got) == list(range(len(saved)))
    for i, g in enumerate(saved):
        assert torch.equal(got[i], _scaled(g, gl[:, i]))
    # centre head: the heat map with column 0, every regression map with column 1; vel is optional
    saved = [_rand(gen, B, ch, 3, 2) for ch in (3, 2, 1, 3, 2) + ((2,) if optional else ())]
    gl = _rand(gen, B, 2)
    got = autograd._scale_saved(saved, gl, autograd.CenterHeadLoss.table)
    assert sorted(got) == list(range(len(saved)))
    for i, g in enumerate(saved):
        assert torch.equal(got[i], _scaled(g, gl[:, 0 if i == 0 else 1]))
    # RoI head: grad_cls with column 0; grad_reg * g1 (+ grad_corner * g2, in this order)
    S = 5
    saved = [_rand(gen, B, S), _rand(gen, B, S, 7)] + ([_rand(gen, B, S, 7)] if optional else [])
    gl = _rand(gen, B, 3)
    got = autograd._scale_saved(saved, gl, autograd.RoIHeadLoss.table)
    greg = _scaled(saved[1], gl[:, 1])
    if optional:
        greg = greg + _scaled(saved[2], gl[:, 2])
    assert sorted(got) == [0, 1] and torch.equal(got[0], _scaled(saved[0], gl[:, 0])) and torch.equal(got[1], greg)
    # point head: column blocks (C -> 0, 7 -> 1) of grad_o and (3 -> 2, 3 -> 3) of grad_c; c is optional
    M, C = 5, 3
    saved = [_rand(gen, B, M, C + 7)] + ([_rand(gen, B, M, 6)] if optional else [])
    gl = _rand(gen, B, 4)
    got = autograd._scale_saved(saved, gl, autograd.PointHeadLoss.table)
    w = torch.cat([gl[:, 0:1].expand(-1, C), gl[:, 1:2].expand(-1, 7)], 1)
    assert sorted(got) == list(range(len(saved))) and torch.equal(got[0], saved[0] * w.unsqueeze(1))
    if optional:
        assert torch.equal(got[1], saved[1] * torch.cat([gl[:, 2:3].expand(-1, 3), gl[:, 3:4].expand(-1, 3)], 1).unsqueeze(1))


def test_moved_backward_operators_refuse_cpu_tensors(sad):
    """The four wrappers live in ``ops`` and go through its checks: a CPU tensor is refused as everywhere else."""
    import torch
    from sad_amd import autograd, ops
    for n in ("group_points_grad", "max_pool_s_with_arg", "three_interpolate_grad"):
        assert getattr(autograd, n) is getattr(ops, n)
    assert not hasattr(autograd, "_f32") and not hasattr(autograd, "_stream")
    idx3 = torch.zeros((1, 4, 3), dtype=torch.int32)
    for call in (lambda: ops.group_points_grad(torch.zeros(1, 2, 4, 3), idx3, 8),
                 lambda: ops.group_points_grad(torch.zeros(1, 2, 4), torch.zeros((1, 4), dtype=torch.int32), 8),
                 lambda: ops.max_pool_s_with_arg(torch.zeros(1, 2, 4, 3)),
                 lambda: ops.max_pool_s_grad(torch.zeros(1, 2, 4), torch.zeros((1, 2, 4), dtype=torch.int32), 3),
                 lambda: ops.three_interpolate_grad(torch.zeros(1, 2, 4), idx3, torch.zeros(1, 4, 3), 8),
                 lambda: autograd.max_pool_s(torch.zeros(1, 2, 4, 3, requires_grad=True)),
                 lambda: autograd.group_points(torch.zeros(1, 2, 8, requires_grad=True), idx3),
                 lambda: autograd.three_interpolate(torch.zeros(1, 2, 8, requires_grad=True), idx3, torch.zeros(1, 4, 3))):
        with pytest.raises(RuntimeError, match="no CPU path"):
            call()
    with pytest.raises(TypeError):
        ops.group_points_grad([[0.0]], idx3, 8)
