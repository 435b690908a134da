"""CPU tests of the host side of the chunk-table optimizers: the table
builder, the `fused` switch, and the reference `_optim_refs.opt_ref` pinned
to the eager path the project already ships."""

import pytest
import torch

import _optim_refs as O
from config import Config
from sat_amd.optim import MT_CHUNK, Optimizer, build_chunk_table

C = MT_CHUNK
SCALAR_SHAPES = [(5,), (3, 7), (64, 33), (1,), (1000,)]
VEC4_SHAPES = [(8,), (4, 3), (64, 32), (1000,), (4,)]
EDGE_SHAPES = [(C,), (C + 1,), (2 * C - 3,), (1,), (3,)]


def _numel(shape):
    n = 1
    for d in shape:
        n *= d
    return n


NUMELS = [
    [_numel(s) for s in SCALAR_SHAPES],
    [_numel(s) for s in VEC4_SHAPES],
    [_numel(s) for s in EDGE_SHAPES],
    [1], [C], [C + 1],
    [3, C - 1, 4 * C, 7, 2 * C + 2, 1],
    [C, C, C],
]


def test_mt_chunk_is_a_multiple_of_4():
    assert MT_CHUNK > 0 and MT_CHUNK % 4 == 0


@pytest.mark.parametrize('chunk', [4, 8, C])
@pytest.mark.parametrize('numels', NUMELS)
def test_chunk_table_covers_every_element_once(numels, chunk):
    table = build_chunk_table(numels, chunk)
    seen = [[0] * n for n in numels]
    for t, start, count in table:
        assert 0 <= t < len(numels)
        assert 0 < count <= chunk                 # no chunk longer
        assert start % 4 == 0
        assert 0 <= start and start + count <= numels[t]   # one tensor
        for i in range(start, start + count):
            seen[t][i] += 1
    assert all(c == 1 for row in seen for c in row)
    # tensor order, and ascending inside a tensor
    assert [(t, s) for t, s, _ in table] == sorted((t, s)
                                                   for t, s, _ in table)
    # only a tensor's last chunk is short
    for t, start, count in table:
        assert count == chunk or start + count == numels[t]


def test_chunk_table_default_chunk_and_bad_chunk():
    assert build_chunk_table([C + 1]) == [(0, 0, C), (0, C, 1)]
    assert build_chunk_table([]) == []
    for bad in (0, 6, -4):
        with pytest.raises(ValueError):
            build_chunk_table([10], bad)


@pytest.mark.parametrize('kind', ['Adam', 'RMSProp', 'Momentum', 'SGD'])
def test_fused_is_false_on_cpu(kind):
    cfg = Config()
    cfg.optimizer = kind
    assert cfg.use_fused_optimizer is True
    opt = Optimizer(cfg, [torch.nn.Parameter(torch.ones(3))])
    assert opt.fused is False


def _hp(cfg):
    return dict(lr0=cfg.initial_learning_rate,
                decay=cfg.learning_rate_decay_factor,
                spd=cfg.num_steps_per_decay, clip=cfg.clip_gradients,
                momentum=cfg.momentum, rho=cfg.decay, eps=cfg.epsilon,
                nesterov=cfg.use_nesterov, centered=cfg.centered)


@pytest.mark.parametrize('kind,flag', [
    ('SGD', None), ('Momentum', False), ('Momentum', True),
    ('RMSProp', False), ('RMSProp', True)])
def test_opt_ref_fp32_matches_eager_step(kind, flag):
    """5 steps, clip active on the odd ones, the staircase crossed at 3;
    atol 1e-6 is the bound of test_adam_matches_torch"""
    cfg = Config()
    cfg.optimizer = kind
    cfg.momentum = 0.9
    cfg.initial_learning_rate = 1e-2
    cfg.learning_rate_decay_factor = 0.5
    cfg.num_steps_per_decay = 3
    cfg.use_nesterov = bool(flag)
    cfg.centered = bool(flag)
    hp = _hp(cfg)
    gen = torch.Generator().manual_seed(7)
    shapes = [(5,), (3, 7), (40,)]
    params = [torch.nn.Parameter(torch.rand(s, generator=gen) * 2 - 1)
              for s in shapes]
    opt = Optimizer(cfg, params)
    names = O.slot_names(kind, hp)
    ps = [p.detach().clone() for p in params]
    slots = {k: [torch.zeros(s) for s in shapes] for k in names}
    clipped = set()
    for t in range(1, 6):
        gs = [torch.randn(s, generator=gen) * (3.0 if t % 2 else 0.01)
              for s in shapes]
        for p, g in zip(params, gs):
            p.grad = g.clone()
        opt.step()
        ps, slots, lr, scale = O.opt_ref(kind, ps, gs, slots, t, hp,
                                         torch.float32)
        clipped.add(scale < 1.0)
        assert abs(lr - opt.learning_rate()) < 1e-9
        for i, p in enumerate(params):
            assert torch.allclose(p.detach(), ps[i], atol=1e-6), (t, i)
            for k in names:
                assert torch.allclose(opt.state[p][k], slots[k][i],
                                      atol=1e-6), (t, i, k)
    assert clipped == {True, False}
