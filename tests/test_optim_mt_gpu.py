"""GPU tests of the chunk-table optimizers (optim_mt.hip: SGD, Momentum,
Momentum-Nesterov, RMSProp, RMSProp-centered) through Optimizer.step(), the
model and the engine, against `_optim_refs.opt_ref`.

Tolerance policy, as in test_tail_ops_gpu.py (no bound is taken from the
code under test):

1. bitwise wherever the arithmetic allows it: bf16 shadows, zeroed grads,
   guard gaps, the step counter, and two runs of the same step;
2. slots against the formula in fp64, with the noise floor
   `floor = max|fp32_cpu - fp64|` of the same formula evaluated by torch on
   the CPU in fp32 on the same inputs, taken at run time:
   max|got - ref| <= 8 floor;
3. updates as max|d - d_ref| / max|d_ref| per tensor and step, with
   d = p_after - p_before in fp64, the reference step taken from the
   device's own (p, slots) before the step, and the floor from an fp32 CPU
   step the same way, <= 8 floors.

Each non-bitwise assertion prints a MEASURE line.
"""

import math

import numpy as np
import pytest
import torch

import _fp64_refs as R
import _optim_refs as O

pytestmark = pytest.mark.gpu

DEV = 'cuda'
F64, F32, BF = torch.float64, torch.float32, torch.bfloat16

SCALAR_SHAPES = [(5,), (3, 7), (64, 33), (1,), (1000,)]
VEC4_SHAPES = [(8,), (4, 3), (64, 32), (1000,), (4,)]
GAP = 8

# (config.optimizer, use_nesterov / centered)
KINDS = [('SGD', None), ('Momentum', False), ('Momentum', True),
         ('RMSProp', False), ('RMSProp', True)]
KIND_IDS = ['sgd', 'momentum', 'nesterov', 'rmsprop', 'rmsprop_centered']


def _chunk():
    from sat_amd.optim import MT_CHUNK
    return MT_CHUNK


def _edge_shapes():
    C = _chunk()
    return [(C,), (C + 1,), (2 * C - 3,), (1,), (3,)]


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _cfg(kind, flag):
    from config import Config
    cfg = Config()
    cfg.optimizer = kind
    cfg.use_nesterov = bool(flag)
    cfg.centered = bool(flag)
    cfg.momentum = 0.9
    cfg.decay = 0.9
    cfg.initial_learning_rate = 1e-2
    cfg.learning_rate_decay_factor = 0.5
    cfg.num_steps_per_decay = 3
    cfg.clip_gradients = 5.0
    return cfg


def _hp(cfg):
    return dict(lr0=cfg.initial_learning_rate,
                decay=cfg.learning_rate_decay_factor,
                spd=cfg.num_steps_per_decay, clip=cfg.clip_gradients,
                momentum=cfg.momentum, rho=cfg.decay, eps=cfg.epsilon,
                nesterov=cfg.use_nesterov, centered=cfg.centered)


class _ParamSet(object):
    """Parameters, their grads and their bf16 shadows as views into three
    flat buffers with NaN guard gaps between and around them, so a write
    next to any tensor shows.  shift = 1 starts every view one element
    further in: 4-byte but not 16-byte aligned (2-byte for the shadows)."""

    def __init__(self, shapes, shadowed, kind, flag, nograd=None, seed=0,
                 shift=0):
        from sat_amd.optim import Optimizer
        self.shapes, self.nograd = shapes, nograd
        offs, o = [], GAP
        for s in shapes:
            offs.append(o + shift)
            o += (int(np.prod(s)) + shift + 3) // 4 * 4 + GAP
        nan = float('nan')
        self.pflat = torch.full((o,), nan, device=DEV)
        self.gflat = torch.full((o,), nan, device=DEV)
        self.sflat = torch.full((o,), nan, dtype=BF, device=DEV)
        assert self.pflat.data_ptr() % 16 == 0
        assert self.gflat.data_ptr() % 16 == 0
        assert self.sflat.data_ptr() % 16 == 0
        self.used = torch.zeros(o, dtype=torch.bool, device=DEV)
        self.sused = torch.zeros(o, dtype=torch.bool, device=DEV)
        gen = _gen(seed)
        self.params, self.grads, shadows = [], [], {}
        for i, (s, off) in enumerate(zip(shapes, offs)):
            n = int(np.prod(s))
            self.used[off:off + n] = True
            pv = self.pflat[off:off + n].view(s)
            pv.copy_(torch.rand(s, generator=gen) * 2 - 1)
            p = torch.nn.Parameter(pv)
            assert p.data_ptr() == pv.data_ptr()
            assert p.data_ptr() % 16 == 4 * shift
            gv = self.gflat[off:off + n].view(s)
            gv.zero_()
            if i != nograd:
                p.grad = gv
            if i in shadowed:
                self.sused[off:off + n] = True
                shadows[p] = self.sflat[off:off + n].view(s)
            self.params.append(p)
            self.grads.append(gv)
        self.cfg = _cfg(kind, flag)
        self.hp = _hp(self.cfg)
        self.names = O.slot_names(kind, self.hp)
        self.kind = kind
        self.opt = Optimizer(self.cfg, self.params)
        assert self.opt.fused is True
        self.shadows = shadows
        self.opt.register_shadows(shadows)

    def fill_grads(self, scale, gen):
        """in place (the addresses a graph captured stay valid); returns
        the fp32 values handed in, on the CPU"""
        out = []
        for i, g in enumerate(self.grads):
            if i != self.nograd:
                g.copy_(torch.randn(g.shape, generator=gen) * scale)
            out.append(g.detach().cpu().clone())
        return out

    def state(self):
        st = self.opt.state
        return ([p.detach().cpu().clone() for p in self.params],
                {k: [st[p][k].cpu().clone() for p in self.params]
                 for k in self.names})

    def assert_guards(self):
        for flat, used in ((self.pflat, self.used), (self.gflat, self.used),
                           (self.sflat, self.sused)):
            assert torch.isnan(flat[~used]).all()      # gaps untouched
            assert not torch.isnan(flat[used]).any()

    def assert_route(self, vec):
        """the 16-byte route is a per-tensor host decision"""
        assert self.opt._ck_vec.cpu().tolist() == [int(vec)] * len(
            self.params)
        assert self.opt._ck_any_vec is bool(vec)


def _compare(tag, t, kind, names, hp, p0, s0, g0, p1, s1):
    """policy 2 (slots) and 3 (dp) for one step on CPU copies"""
    r64 = O.opt_ref(kind, p0, g0, s0, t, hp, F64)
    r32 = O.opt_ref(kind, p0, g0, s0, t, hp, F32)
    # The floor is the maximum over every element of the set: the tensors
    # share one formula and one input distribution, and a maximum over the
    # 1 or 5 elements of the small ones is a draw, not a floor.  The error
    # is taken per tensor.
    fl_d = 0.0
    fl_s = {k: 0.0 for k in names}
    for i in range(len(p0)):
        dref = r64[0][i] - p0[i].double()
        if dref.abs().max() > 0:
            fl_d = max(fl_d, ((r32[0][i].double() - p0[i].double()) - dref)
                       .abs().max().item() / dref.abs().max().item())
        for k in names:
            fl_s[k] = max(fl_s[k], R.noise_floor(r32[1][k][i],
                                                 r64[1][k][i]))
    worst_d = 0.0
    worst_s = {k: 0.0 for k in names}
    for i in range(len(p0)):
        d = p1[i].double() - p0[i].double()
        dref = r64[0][i] - p0[i].double()
        if dref.abs().max() == 0:          # no grad, zero slots: no update
            assert (d == 0).all(), (tag, t, i)
        else:
            e = ((d - dref).abs().max() / dref.abs().max()).item()
            worst_d = max(worst_d, e)
            assert e <= R.SLACK * fl_d, (tag, t, i, e, fl_d)
        for k in names:
            e = R.fp32_err(s1[k][i], r64[1][k][i])
            worst_s[k] = max(worst_s[k], e)
            assert e <= R.SLACK * fl_s[k], (tag, t, i, k, e, fl_s[k])
    print('MEASURE %s %-8s t=%d scale %.4f lr %.5f | dp err %.2e floor %.2e'
          % (kind, tag, t, r64[3], r64[2], worst_d, fl_d)
          + ''.join(' | %s err %.2e floor %.2e' % (k, worst_s[k], fl_s[k])
                    for k in names))
    return r64[2], r64[3]


def _checked_step(S, run, t, gscale, gen, tag):
    """hand in grads, run one step (eager or a replay), and compare
    everything it wrote with the fp64 step from the state before it"""
    g0 = S.fill_grads(gscale, gen)
    p0, s0 = S.state()
    run()
    torch.cuda.synchronize()
    p1, s1 = S.state()
    lr, scale = _compare(tag, t, S.kind, S.names, S.hp, p0, s0, g0, p1, s1)
    for g in S.grads:                      # zeroed in the update pass
        assert (g == 0).all()
    for p, sh in S.shadows.items():        # bf16 write-through
        assert torch.equal(R.bits(sh), R.bits(p.detach().to(BF)))
    S.assert_guards()
    assert S.opt.step_dev.item() == t
    return lr, scale


# =====================================================================
# 1. seven steps
# =====================================================================

# first MI355X run, both sets, per step: dp err equal to the floor to three
# digits at nearly every step, at most 1.08 floors (SGD 2.0e-5..1.1e-3,
# Momentum 9.2e-6..1.1e-4, RMSProp 8.6e-7..2.1e-6); Momentum's mom err
# 1.4e-8..4.5e-8 at floors 1.5e-8..5.6e-8 (at most 1.25 floors); RMSProp's
# ms err 5.5e-10..4.9e-9 (at most 3.2 floors: 3.96e-9 at 1.24e-9, step 7),
# mom 3.4e-9..1.0e-8 (1.16 floors), mg 1.9e-9..1.3e-8 (1.8 floors)
@pytest.mark.parametrize('shapes', ['scalar', 'vec4'])
@pytest.mark.parametrize('kind,flag', KINDS, ids=KIND_IDS)
def test_opt_mt_seven_steps(kind, flag, shapes):
    """7 steps of Optimizer.step(): grads alternate between 3 randn (clip
    active) and 0.01 randn (inactive), the staircase is crossed at steps 3
    and 6.  The first set has a parameter without grad and two of five
    shadowed; the second has every tensor shadowed."""
    if shapes == 'scalar':
        S = _ParamSet(SCALAR_SHAPES, (1, 4), kind, flag, nograd=3, seed=1)
    else:
        S = _ParamSet(VEC4_SHAPES, (0, 1, 2, 3, 4), kind, flag, seed=2)
    gen = _gen(10)
    scales = set()
    for t in range(1, 8):
        lr, scale = _checked_step(S, S.opt.step, t,
                                  3.0 if t % 2 else 0.01, gen, shapes)
        scales.add(scale < 1.0)
        assert S.opt.learning_rate() == lr      # the host formula
        assert lr == 1e-2 * 0.5 ** (t // 3)
    assert scales == {True, False}              # both clip branches ran
    # every view starts on 16 bytes (8 for a shadow): all on the float4 route
    S.assert_route(True)


# =====================================================================
# 2. chunk edges
# =====================================================================

# first run: every err equal to its floor to three digits or below it, on
# both routes (RMSProp dp 1.0e-6..2.0e-6, ms 3.9e-10..2.5e-9, mom
# 9.0e-9..1.1e-8, mg 1.6e-9..8.2e-9; SGD dp 1.3e-5..1.6e-4)
@pytest.mark.parametrize('shift', [0, 1], ids=['aligned', 'misaligned'])
@pytest.mark.parametrize('kind,flag', [('RMSProp', True), ('SGD', None)],
                         ids=['rmsprop_centered', 'sgd'])
def test_opt_mt_chunk_edges(kind, flag, shift):
    """tensors of C, C+1, 2C-3, 1 and 3 elements: a full chunk, a
    one-element last chunk, a last chunk with a scalar tail, and tensors
    below one float4.  Shifted by one element every pointer is 4-byte but
    not 16-byte aligned: the element-by-element route, and nothing written
    on either side."""
    from sat_amd.optim import build_chunk_table
    shapes = _edge_shapes()
    S = _ParamSet(shapes, (0, 2, 3), kind, flag, seed=20 + shift,
                  shift=shift)
    gen = _gen(21)
    for t in (1, 2):
        _checked_step(S, S.opt.step, t, 3.0 if t % 2 else 0.01, gen,
                      'edge%d' % shift)
    S.assert_route(shift == 0)
    want = build_chunk_table([int(np.prod(s)) for s in shapes], _chunk())
    assert len(want) == 1 + 2 + 2 + 1 + 1
    assert S.opt._ck_chunks.cpu().tolist() == [list(r) for r in want]


# =====================================================================
# 3. graph replay
# =====================================================================

# first run, warm-up and replays: dp err equal to the floor (at most 1.00);
# slots at most 2.7 floors (RMSProp ms 3.60e-9 at 1.34e-9, replay t=3), mg
# 1.5, Momentum's mom 1.4
@pytest.mark.parametrize('kind,flag', KINDS, ids=KIND_IDS)
def test_opt_mt_graph_replay(kind, flag):
    """opt.step() captured once and replayed 5 times with grads refilled
    in place: each replay is the fp64 step of its own t (2..6, across the
    decay boundaries at 3 and 6), which only the device counter gives"""
    S = _ParamSet(VEC4_SHAPES, (0, 2), kind, flag, seed=3)
    gen = _gen(11)
    # eager warm-up: the table build copies host to device
    _checked_step(S, S.opt.step, 1, 3.0, gen, 'warmup')
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        S.opt.step()
    torch.cuda.synchronize()
    assert S.opt.step_dev.item() == 1           # capture ran nothing
    lrs = []
    for t in range(2, 7):
        lr, _ = _checked_step(S, graph.replay, t,
                              3.0 if t % 2 else 0.01, gen, 'replay')
        lrs.append(lr)
    assert lrs == [1e-2, 5e-3, 5e-3, 5e-3, 2.5e-3]


# =====================================================================
# 4. reproducibility
# =====================================================================

def test_opt_mt_step_is_bitwise_reproducible():
    """two sets from one seed, the same grads, one clipped step: the norm
    is a fixed-order sum of per-block partials, so parameters and slots
    are equal bit for bit"""
    C = _chunk()
    out = []
    for _ in range(2):
        S = _ParamSet([(2 * C - 3,)], (0,), 'RMSProp', True, seed=30)
        S.fill_grads(3.0, _gen(31))
        S.opt.step()
        torch.cuda.synchronize()
        p, s = S.state()
        out.append((p, s, S.sflat.cpu().view(torch.int16)))
        S.assert_guards()
    (pa, sa, ha), (pb, sb, hb) = out
    assert torch.equal(pa[0].view(torch.int32), pb[0].view(torch.int32))
    for k in ('ms', 'mom', 'mg'):
        assert sa[k][0].abs().max() > 0
        assert torch.equal(sa[k][0].view(torch.int32),
                           sb[k][0].view(torch.int32))
    assert torch.equal(ha, hb)


# =====================================================================
# 5. clip boundary
# =====================================================================

@pytest.mark.parametrize('extra,clipped', [(0.0, False), (1.0, True)])
def test_opt_mt_clip_boundary(extra, clipped):
    """SGD, sum g^2 = 25 exactly with clip = 5: norm > clip is false, scale
    1, dp = -lr g; sum g^2 = 26: scale 5 / sqrt(26).  The parameters start
    at 0, so p after the step is the fp32 product chain itself."""
    S = _ParamSet([(5,), (3, 7)], (), 'SGD', None, seed=5)
    for p in S.params:
        p.data.zero_()
    S.grads[0][0] = 3.0
    S.grads[1][1, 2] = 4.0
    S.grads[1][2, 6] = extra
    g0 = [g.cpu().double() for g in S.grads]
    assert sum((g * g).sum().item() for g in g0) == 25.0 + extra
    S.opt.step()
    torch.cuda.synchronize()
    scale = 5.0 / math.sqrt(26.0) if clipped else 1.0
    lr = float(np.float32(1e-2))
    for p, g in zip(S.params, g0):
        got = p.detach().cpu().double()
        want = -lr * g * scale
        err = (got - want).abs().max().item()
        print('MEASURE sgd clip boundary extra=%g err %.3e bound %.3e'
              % (extra, err, 8 * 2.0 ** -24 * 0.04))
        # one fp32 product chain: a few 2^-24 relative of |dp| <= 0.04
        # (first run: err 0 unclipped, 1.7e-9 clipped, bound 1.9e-8)
        assert err <= 8 * 2.0 ** -24 * 0.04
        assert (got[g == 0] == 0).all()
    # the two scales differ by 2 %: the boundary case is not clipped
    p00 = S.params[0][0].item()
    assert (abs(p00 + 0.03) < 1e-7) is (not clipped)
    S.assert_guards()


# =====================================================================
# 6. channels_last
# =====================================================================

@pytest.mark.parametrize('grad_layout', ['channels_last', 'contiguous'])
def test_opt_mt_channels_last_param(grad_layout):
    """a channels_last 4-D parameter with a grad in either layout, two
    Momentum steps: p, g and mom pair by LOGICAL index (the second step
    shows a mispaired mom), and mom has the parameter's strides"""
    from sat_amd.optim import Optimizer
    gen = _gen(13)
    w = torch.randn(8, 4, 3, 3, generator=gen)
    p = torch.nn.Parameter(
        w.to(DEV).contiguous(memory_format=torch.channels_last))
    assert not p.is_contiguous()
    cfg = _cfg('Momentum', False)
    hp = _hp(cfg)
    opt = Optimizer(cfg, [p])
    for t in (1, 2):
        g = torch.randn(8, 4, 3, 3, generator=gen) * 0.01
        gd = g.to(DEV)
        if grad_layout == 'channels_last':
            gd = gd.contiguous(memory_format=torch.channels_last)
        p.grad = gd
        p0 = [p.detach().cpu().contiguous()]
        s0 = {'mom': [opt.state[p]['mom'].cpu().contiguous()]}
        opt.step()
        torch.cuda.synchronize()
        p1 = [p.detach().cpu().contiguous()]
        s1 = {'mom': [opt.state[p]['mom'].cpu().contiguous()]}
        # first run, either layout: dp err 3.62e-4 / 2.94e-4 (steps 1 / 2)
        # and mom err 0 / 1.49e-9, all equal to their floors
        _compare('CL/' + grad_layout[:4], t, 'Momentum', ('mom',), hp,
                 p0, s0, [g], p1, s1)
        assert opt.state[p]['mom'].stride() == p.stride()
        # the grad now has the parameter's layout, and it is the tensor
        # the kernel zeroed
        assert p.grad.stride() == p.stride()
        assert (p.grad == 0).all()
        assert (p.grad is gd) is (grad_layout == 'channels_last')
    assert opt.state[p]['mom'].abs().max() > 0


# =====================================================================
# 7. the model's own parameter list
# =====================================================================

def _model_cfg(tiny_config, kind, **kw):
    cfg = tiny_config
    cfg.device = 'cuda'
    cfg.vocabulary_size = 500
    cfg.dim_embedding = 512
    cfg.num_lstm_units = 512
    cfg.dim_initalize_layer = 512
    cfg.dim_attend_layer = 512
    cfg.dim_decode_layer = 1024
    cfg.fc_drop_rate = 0.0
    cfg.lstm_drop_rate = 0.0
    cfg.batch_size = 2
    cfg.optimizer = kind
    # the hyper-parameters of every case of this file.  At the default
    # lr0 = 1e-4 an SGD update of the least-driven tensors (weight decay
    # only, |g| ~ 1e-5) is below half an ulp of the weight and fp32 rounds
    # it away, on the eager path too: "every tensor moved" needs 1e-2.
    cfg.momentum = 0.9
    cfg.decay = 0.9
    cfg.initial_learning_rate = 1e-2
    cfg.learning_rate_decay_factor = 0.5
    cfg.num_steps_per_decay = 3
    cfg.clip_gradients = 5.0
    for k, v in kw.items():
        setattr(cfg, k, v)
    return cfg


def _batch(cfg, B=2):
    torch.manual_seed(1)
    T = cfg.max_caption_length
    return (torch.randn(B, 3, 224, 224, device='cuda') * 50.0,
            torch.randint(1, cfg.vocabulary_size, (B, T), device='cuda'),
            torch.ones(B, T, device='cuda'))


def _assert_shadows(m):
    d = m.model.decoder
    assert getattr(d, '_shadows_active', False)
    assert len(d._shadow_map) > 0
    for p, sh in d._shadow_map.items():
        assert torch.equal(R.bits(sh), R.bits(p.detach().to(BF))), \
            'stale shadow for %s' % (tuple(p.shape),)


@pytest.mark.parametrize('kind', ['RMSProp', 'Momentum', 'SGD'])
def test_opt_mt_model_parameters(tiny_config, kind):
    """one hand-made forward and backward of the tiny model, then
    optimizer.step() on its own parameter list (config defaults: centered,
    nesterov) against the fp64 step, policy 3"""
    from sat_amd.models.base_model import BaseModel
    cfg = _model_cfg(tiny_config, kind, use_hip_graph=False)
    torch.manual_seed(cfg.seed)
    m = BaseModel(cfg)
    opt = m.optimizer
    assert opt.fused is True
    m.model.train()
    out = m.model(*_batch(cfg))
    out['total_loss'].backward()
    hp = _hp(cfg)
    names = O.slot_names(kind, hp)
    g0 = [(p.grad if p.grad is not None else torch.zeros_like(p))
          .detach().float().cpu().clone() for p in opt.params]
    assert sum(g.abs().max() > 0 for g in g0) > len(g0) // 2
    p0 = [p.detach().cpu().clone() for p in opt.params]
    s0 = {k: [opt.state[p][k].cpu().clone() for p in opt.params]
          for k in names}
    opt.step()
    torch.cuda.synchronize()
    p1 = [p.detach().cpu().clone() for p in opt.params]
    s1 = {k: [opt.state[p][k].cpu().clone() for p in opt.params]
          for k in names}
    _compare('model', 1, kind, names, hp, p0, s0, g0, p1, s1)
    for p in opt.params:
        assert p.grad is None or (p.grad == 0).all()
    assert opt.step_dev.item() == 1
    _assert_shadows(m)


# =====================================================================
# 8. engine
# =====================================================================

@pytest.mark.parametrize('kind', ['RMSProp', 'Momentum', 'SGD'])
def test_opt_mt_engine_captures_full_graph(tiny_config, kind):
    from sat_amd.models.base_model import BaseModel
    cfg = _model_cfg(tiny_config, kind, use_hip_graph=True)
    torch.manual_seed(cfg.seed)
    m = BaseModel(cfg)
    assert m.optimizer.fused is True
    before = [p.detach().clone() for p in m.optimizer.params]
    b = _batch(cfg)
    losses = [m.train_step(*b)['total_loss'].item() for _ in range(5)]
    torch.cuda.synchronize()
    assert m._engine.mode == 'full' and m._engine.failed is False
    assert m.global_step == 5
    assert m.optimizer.step_count == 5
    assert int(m.optimizer.step_dev.item()) == 5
    assert all(math.isfinite(x) for x in losses), losses
    for p, q in zip(m.optimizer.params, before):
        assert torch.isfinite(p).all()
        assert (p.detach() != q).any(), tuple(p.shape)
    _assert_shadows(m)


@pytest.mark.parametrize('kind', ['RMSProp', 'Momentum', 'SGD'])
def test_opt_mt_engine_unfused_falls_back_to_eager(tiny_config, kind):
    from sat_amd.models.base_model import BaseModel
    cfg = _model_cfg(tiny_config, kind, use_hip_graph=True,
                     use_fused_optimizer=False)
    torch.manual_seed(cfg.seed)
    m = BaseModel(cfg)
    assert m.optimizer.fused is False
    before = [p.detach().clone() for p in m.optimizer.params]
    b = _batch(cfg)
    losses = [m.train_step(*b)['total_loss'].item() for _ in range(5)]
    torch.cuda.synchronize()
    assert m._engine.failed is True and m._engine.mode is None
    assert m.optimizer.step_count == 5
    assert all(math.isfinite(x) for x in losses), losses
    for p, q in zip(m.optimizer.params, before):
        assert (p.detach() != q).any(), tuple(p.shape)
    _assert_shadows(m)
