"""GPU tests of the kernels the fused chains share or sit next to: the
dropout hash family, the live multi-tensor Adam, masked CE, embedding, the
LSTM pointwise pair, the attention pool and the frozen-BatchNorm epilogue,
each against an independent reference from `_fp64_refs`.

Tolerance policy (no bound is taken from the code under test):

1. bitwise wherever the arithmetic allows it: masks, gathers, bf16
   shadows, zeroed grads, and sums of small integers (exact in fp32 in any
   order);
2. otherwise against the formula in fp64, with the noise floor
   `floor = max|fp32_cpu - fp64|` of the same formula evaluated by torch on
   the CPU in fp32 on the same inputs, taken at run time:
     fp32 outputs   max|got - ref| <= 8 floor
     bf16 outputs   |got - ref| <= 2^-8 |ref| + 8 floor, elementwise
   (8: the device's __expf / __logf / powf / division are a few ulp looser
   than libm, and it sums in another order);
3. Adam updates as max|d - d_ref| / max|d_ref| per tensor and step, with
   d = p_after - p_before in fp64, the reference step taken from the
   device's own (p, m, v) before the step, and the floor from an fp32 CPU
   step the same way.

Each non-bitwise assertion prints `name err floor bound`; the figures of
the first MI355X run stand next to the assertions.
"""

import json
import math
import os

import numpy as np
import pytest
import torch

import _fp64_refs as R

pytestmark = pytest.mark.gpu

DEV = 'cuda'
F64, F32, BF = torch.float64, torch.float32, torch.bfloat16
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)),
                      'golden', 'dropout_hash.json')


def _C():
    from sat_amd import _C as ext
    return ext


def _bf(x):
    return x.to(DEV, BF)


def _seed(v=12345):
    return torch.tensor(v, dtype=torch.int64, device=DEV)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _check_fp32(name, got, ref64, ref32):
    floor = R.noise_floor(ref32, ref64)
    err = R.fp32_err(got, ref64)
    print('MEASURE %-34s err %.3e floor %.3e bound %.3e'
          % (name, err, floor, R.SLACK * floor))
    assert err <= R.SLACK * floor, (name, err, floor)


def _check_bf16(name, got, ref64, ref32, sel=None):
    got = got.detach().cpu()
    if sel is not None:
        got, ref64, ref32 = got[sel], ref64[sel], ref32[sel]
    floor = R.noise_floor(ref32, ref64)
    ratio = R.bf16_excess(got, ref64, floor)
    print('MEASURE %-34s err/bound %.3f floor %.3e max|ref| %.3e'
          % (name, ratio, floor, ref64.abs().max().item()))
    assert ratio <= 1.0, (name, ratio, floor)


# =====================================================================
# 1. dropout hash: every kernel bitwise against the numpy oracle
# =====================================================================

SEED = 12345
PS = [0.3, 0.5]


def _x_nonzero(shape, seed):
    x = torch.randn(shape, generator=_gen(seed))
    x[x.abs() < 1e-3] = 1.0           # a dropped element is told by its 0
    return x.to(BF)


def _assert_dropout(got, x_cpu, scale):
    """kept/dropped pattern and values, both bitwise"""
    got = got.detach().cpu()
    keep = torch.from_numpy(np.ascontiguousarray(scale != 0))
    assert torch.equal(got.reshape(-1) != 0, keep.reshape(-1))
    ref = R.dropout_ref(x_cpu, scale)
    assert torch.equal(R.bits(got), R.bits(ref))


# 8 / 120 / 16640: less than a block, and a ragged last block; 13 and
# 2051 end in the scalar tail of the 8-wide kernel
@pytest.mark.parametrize('n', [8, 120, 16640, 13, 2051])
@pytest.mark.parametrize('p', PS)
def test_hash_dropout_and_out_match_oracle(p, n):
    C = _C()
    x = _x_nonzero((n,), n)
    xd = x.to(DEV)
    scale = R.drop_scale(SEED, 9, np.arange(n), p)
    assert 0 < (scale != 0).sum() < n or n <= 13
    y = C.hash_dropout(xd, _seed(), p, 9)
    _assert_dropout(y, x, scale)
    buf = torch.full((n + 32,), 7.0, dtype=BF, device=DEV)
    C.hash_dropout_out(xd, _seed(), p, 9, buf[16:16 + n])
    _assert_dropout(buf[16:16 + n], x, scale)
    assert (buf[:16] == 7).all() and (buf[16 + n:] == 7).all()
    assert torch.equal(xd.cpu(), x)                  # input untouched


@pytest.mark.parametrize('B,N', [(3, 40), (33, 72)])
@pytest.mark.parametrize('p', PS)
def test_hash_dropout_steps_and_slabs_match_oracle(p, B, N):
    """T = 3 slabs, salt = base + 16 t, indices LOCAL to the slab"""
    C = _C()
    T, base, stride = 3, 5, 16
    idx = np.arange(B * N)
    scale = np.stack([R.drop_scale(SEED, base + stride * t, idx, p)
                      for t in range(T)])            # [T, B*N]
    # steps: one [B, N] input, T outputs
    x = _x_nonzero((B, N), B)
    y = C.hash_dropout_steps(x.to(DEV), _seed(), p, base, stride, T)
    assert y.shape == (T, B, N)
    _assert_dropout(y, x.expand(T, B, N).contiguous(),
                    scale.reshape(T, B, N))
    # slabs: a step-major [T*B, N] input
    xs = _x_nonzero((T * B, N), B + 1)
    ys = C.hash_dropout_slabs(xs.to(DEV), _seed(), p, base, stride, T)
    assert ys.shape == (T * B, N)
    _assert_dropout(ys, xs, scale.reshape(T * B, N))


@pytest.mark.parametrize('B,D,E,H,V', [(3, 16, 24, 8, 11),
                                       (33, 64, 40, 72, 50)])
@pytest.mark.parametrize('p', PS + [0.0])
def test_lstm_in_tail_matches_oracle(p, B, D, E, H, V):
    """columns [D, D+E) = dropout(table[ids]) at index b*(D+E) + column,
    [D+E, D+E+H) = state copy, [0, D) not written"""
    C = _C()
    I = D + E
    table = _x_nonzero((V, E), 1)
    sth = _x_nonzero((B, H), 2)
    ids = torch.randint(0, V, (B,), generator=_gen(3))
    ids[0], ids[-1] = 0, V - 1
    xh = torch.full((B, I + H), 7.0, dtype=BF, device=DEV)
    C.lstm_in_tail(table.to(DEV), ids.to(DEV), sth.to(DEV), _seed(),
                   p, 51, xh, D)
    idx = (np.arange(B)[:, None] * I + np.arange(D, I)[None, :])
    scale = R.drop_scale(SEED, 51, idx, p)
    _assert_dropout(xh[:, D:I], table[ids], scale)
    assert torch.equal(xh[:, I:].cpu(), sth)
    assert (xh[:, :D] == 7).all()


def _scores_ref(t1, t2, v, L, p, salt, dtype):
    """(scale [B*L, A], t = (t1 + t2) * scale, logits = t . v)"""
    rows, A = t1.shape
    sc = R.drop_scale8(SEED, salt, np.arange(rows * A // 8), p)
    sc = torch.from_numpy(sc.reshape(rows, A))
    s = t1.float() + t2.float().repeat_interleave(L, 0)   # exact in fp32
    t = s.to(dtype) * sc.to(dtype)
    return sc, s, (t * v.to(dtype)).sum(1)


@pytest.mark.parametrize('B,L,A', [(2, 5, 512), (3, 49, 512)])
@pytest.mark.parametrize('p', PS + [0.0])
def test_attn_scores_fused_matches_oracle(p, B, L, A):
    """tdrop bitwise against the 8-wide oracle (group index = flat index
    / 8); the fp32 logits by policy 2"""
    C = _C()
    t1 = _x_nonzero((B * L, A), 4)
    t2 = _x_nonzero((B, A), 5)
    s_chk = t1.float() + t2.float().repeat_interleave(L, 0)
    t1[s_chk == 0] += 1.0                       # keep t1 + t2 nonzero
    v = (torch.randn(A, generator=_gen(6)) * 0.05).to(BF)
    tdrop, logits = C.attn_scores_fused(t1.to(DEV), t2.to(DEV), v.to(DEV),
                                        _seed(), p, 2, L)
    sc, s, ref64 = _scores_ref(t1, t2, v, L, p, 2, F64)
    _, _, ref32 = _scores_ref(t1, t2, v, L, p, 2, F32)
    got = tdrop.cpu()
    assert torch.equal(got != 0, sc != 0)
    assert torch.equal(R.bits(got), R.bits((s * sc).to(BF)))
    # first run: err 1.8e-7..4.3e-7 at floors 1.1e-7..6.8e-7 (at most
    # 1.7 floors)
    _check_fp32('attn_scores logits p=%s L=%d' % (p, L),
                logits.reshape(-1), ref64, ref32)


@pytest.mark.parametrize('p', PS)
def test_attn_scores_dropout_scale_is_unbiased(p):
    """mean(tdrop / t) with t == 1 over 2^19 elements is within 4.5 sigma
    of 1.  With kept values scaled by 1/(1-p) while the byte compare
    drops floor(256p)/256 of them, p = 0.3 gives 180/256 * bf16(1/0.7) =
    1.0053, 5.8 sigma off."""
    C = _C()
    B, L, A = 8, 128, 512
    n = B * L * A
    assert n >= 2 ** 19
    t1 = torch.ones(B * L, A, dtype=BF, device=DEV)
    t2 = torch.zeros(B, A, dtype=BF, device=DEV)
    v = torch.zeros(A, dtype=BF, device=DEV)
    tdrop, _ = C.attn_scores_fused(t1, t2, v, _seed(), p, 2, L)
    mean = tdrop.double().mean().item()
    q = 1.0 - R.drop_pq(p) / 256.0
    sigma = float(R.drop_inv8(p)) * math.sqrt(q * (1 - q) / n)
    z = abs(mean - 1.0) / sigma
    print('MEASURE drop_scale8 mean p=%s: %.6f z %.2f' % (p, mean, z))
    assert z < 4.5, (mean, z)       # first run: z 1.12 (0.3), 0.65 (0.5)
    sc = R.drop_scale8(SEED, 2, np.arange(n // 8), p).reshape(B * L, A)
    assert torch.equal(R.bits(tdrop),
                       R.bits(torch.from_numpy(sc).to(BF)))


def test_dropout_p0_is_identity():
    """p = 0: hash_dropout and _slabs return their input itself, _out and
    _steps fill copies"""
    C = _C()
    x = _x_nonzero((6, 40), 7).to(DEV)
    assert C.hash_dropout(x, _seed(), 0.0, 9).data_ptr() == x.data_ptr()
    assert C.hash_dropout_slabs(x, _seed(), 0.0, 5, 16, 3).data_ptr() \
        == x.data_ptr()
    out = torch.full_like(x, 7.0)
    C.hash_dropout_out(x, _seed(), 0.0, 9, out)
    assert torch.equal(R.bits(out), R.bits(x))
    y = C.hash_dropout_steps(x, _seed(), 0.0, 5, 16, 3)
    assert y.data_ptr() != x.data_ptr()
    assert torch.equal(R.bits(y), R.bits(x.expand(3, 6, 40).contiguous()))


def test_golden_vectors_on_device():
    """the first 64 pinned hash words against the device: hash_dropout of
    x = 1 at a pinned (seed, salt) shows the keep decision of each pinned
    index, and that decision is a function of the pinned word alone"""
    C = _C()
    with open(GOLDEN) as f:
        vec = json.load(f)['vectors'][:64]
    groups = {}
    for seed, salt, idx, h in vec:
        groups.setdefault((seed, salt), []).append((idx, h))
    assert len(groups) == 4
    x = torch.ones(4096, dtype=BF, device=DEV)
    for (seed, salt), items in groups.items():
        idx = torch.tensor([i for i, _ in items])
        h = np.array([w for _, w in items], dtype=np.uint32)
        u = (h >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)
        for p in PS:
            y = C.hash_dropout(x, _seed(seed), p, salt).cpu()
            want = torch.from_numpy(u >= np.float32(p))
            assert torch.equal(y[idx] != 0, want), (seed, salt, p)


# =====================================================================
# 2. the live multi-tensor Adam, through Optimizer.step()
# =====================================================================

SCALAR_SHAPES = [(5,), (3, 7), (64, 33), (1,), (1000,)]   # cum not all % 4
VEC4_SHAPES = [(8,), (4, 3), (64, 32), (1000,), (4,)]     # cum all % 4
GAP = 8


def _cfg():
    from config import Config
    cfg = Config()
    cfg.initial_learning_rate = 1e-2
    cfg.learning_rate_decay_factor = 0.5
    cfg.num_steps_per_decay = 3
    return cfg


def _hp(cfg):
    return dict(lr0=cfg.initial_learning_rate,
                decay=cfg.learning_rate_decay_factor,
                spd=cfg.num_steps_per_decay, b1=cfg.beta1, b2=cfg.beta2,
                eps=cfg.epsilon, clip=cfg.clip_gradients)


class _ParamSet(object):
    """Parameters, their grads and their bf16 shadows as views into three
    flat buffers with NaN guard gaps between and around them, so a write
    next to any tensor shows."""

    def __init__(self, shapes, shadowed, nograd=None, seed=0):
        from sat_amd.optim import Optimizer
        self.shapes, self.nograd = shapes, nograd
        offs, o = [], GAP
        for s in shapes:
            offs.append(o)
            o += (int(np.prod(s)) + 3) // 4 * 4 + GAP
        nan = float('nan')
        self.pflat = torch.full((o,), nan, device=DEV)
        self.gflat = torch.full((o,), nan, device=DEV)
        self.sflat = torch.full((o,), nan, dtype=BF, device=DEV)
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
            gv = self.gflat[off:off + n].view(s)
            gv.zero_()
            if i != nograd:
                p.grad = gv
            if i in shadowed:
                self.sused[off:off + n] = True
                shadows[p] = self.sflat[off:off + n].view(s)
            self.params.append(p)
            self.grads.append(gv)
        self.cfg = _cfg()
        self.opt = Optimizer(self.cfg, self.params)
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
                [st[p]['m'].cpu().clone() for p in self.params],
                [st[p]['v'].cpu().clone() for p in self.params])

    def assert_guards(self):
        for flat, used in ((self.pflat, self.used), (self.gflat, self.used),
                           (self.sflat, self.sused)):
            assert torch.isnan(flat[~used]).all()      # gaps untouched
            assert not torch.isnan(flat[used]).any()


def _checked_step(S, run, t, gscale, gen, tag):
    """hand in grads, run one step (eager or a replay), and compare
    everything it wrote with the fp64 step from the state before it"""
    hp = _hp(S.cfg)
    g0 = S.fill_grads(gscale, gen)
    p0, m0, v0 = S.state()
    run()
    torch.cuda.synchronize()
    p1, m1, v1 = S.state()
    r64 = R.adam_ref(p0, g0, m0, v0, t, hp, F64)
    r32 = R.adam_ref(p0, g0, m0, v0, t, hp, F32)
    # The floor is the maximum over every element of the set: the tensors
    # share one formula and one input distribution, and a maximum over the
    # 1 or 5 elements of the small ones is a draw, not a floor.  The error
    # is taken per tensor.
    fl_d = fl_m = fl_v = 0.0
    for i in range(len(p0)):
        dref = r64[0][i] - p0[i].double()
        if dref.abs().max() > 0:
            fl_d = max(fl_d, ((r32[0][i].double() - p0[i].double()) - dref)
                       .abs().max().item() / dref.abs().max().item())
        fl_m = max(fl_m, R.noise_floor(r32[1][i], r64[1][i]))
        fl_v = max(fl_v, R.noise_floor(r32[2][i], r64[2][i]))
    worst = [0.0, 0.0, 0.0]
    for i in range(len(p0)):
        d = p1[i].double() - p0[i].double()
        dref = r64[0][i] - p0[i].double()
        if dref.abs().max() == 0:          # no grad, m = v = 0: no update
            assert (d == 0).all()
        else:
            e = ((d - dref).abs().max() / dref.abs().max()).item()
            worst[0] = max(worst[0], e)
            assert e <= R.SLACK * fl_d, (tag, t, i, e, fl_d)
        em = R.fp32_err(m1[i], r64[1][i])
        ev = R.fp32_err(v1[i], r64[2][i])
        worst[1], worst[2] = max(worst[1], em), max(worst[2], ev)
        assert em <= R.SLACK * fl_m, (tag, t, i, em, fl_m)
        assert ev <= R.SLACK * fl_v, (tag, t, i, ev, fl_v)
    print('MEASURE adam %-8s t=%d scale %.4f lr %.5f | dp err %.2e floor '
          '%.2e | m err %.2e floor %.2e | v err %.2e floor %.2e'
          % (tag, t, r64[4], r64[3], worst[0], fl_d, worst[1], fl_m,
             worst[2], fl_v))
    for i, g in enumerate(S.grads):        # zeroed in the update pass
        assert (g == 0).all()
    for p, sh in S.shadows.items():        # bf16 write-through
        assert torch.equal(R.bits(sh), R.bits(p.detach().to(BF)))
    S.assert_guards()
    assert S.opt.step_dev.item() == t
    return r64[3], r64[4]


# first run, both sets and the replays, per step: dp err 5.7e-6..3.3e-5,
# equal to the floor to three digits at every step; m err 1.8e-9..1.4e-8 at
# floors 2.3e-9..1.3e-8 (at most 1.8 floors); v err 1.4e-11..1.8e-9 at
# floors 1.4e-11..1.8e-9 (at most 1.2 floors)
@pytest.mark.parametrize('kind', ['scalar', 'vec4'])
def test_adam_mt_seven_steps(kind):
    """7 steps of Optimizer.step(): grads alternate between 3 randn (clip
    active) and 0.01 randn (inactive), the staircase is crossed at steps 3
    and 6.  The scalar set has a parameter without grad and two of five
    shadowed; the float4 set has every boundary a multiple of 4."""
    if kind == 'scalar':
        S = _ParamSet(SCALAR_SHAPES, shadowed=(1, 4), nograd=3, seed=1)
    else:
        S = _ParamSet(VEC4_SHAPES, shadowed=(0, 1, 2, 3, 4), seed=2)
    gen = _gen(10)
    scales = set()
    for t in range(1, 8):
        lr, scale = _checked_step(S, S.opt.step, t,
                                  3.0 if t % 2 else 0.01, gen, kind)
        scales.add(scale < 1.0)
        assert S.opt.learning_rate() == lr      # the host formula
        assert lr == 1e-2 * 0.5 ** (t // 3)
    assert scales == {True, False}              # both clip branches ran
    assert S.opt._mt_vec4 is (kind == 'vec4')


def test_adam_mt_graph_replay():
    """opt.step() captured once and replayed 5 times with grads refilled
    in place: each replay is the fp64 step of its own t (2..6, across the
    decay boundaries at 3 and 6), which only the device counter gives"""
    S = _ParamSet(VEC4_SHAPES, shadowed=(0, 2), seed=3)
    gen = _gen(11)
    # eager warm-up: the descriptor build copies host to device
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


def _int_grads(S, gen, lo=-8, hi=8):
    out = []
    for g in S.grads:
        g.copy_(torch.randint(lo, hi + 1, g.shape, generator=gen).float())
        out.append(g.cpu().double())
    return out


def test_sq_norm_mt_exact():
    """integer grads, |g| <= 8, 63267 elements: the sum of squares is an
    integer below 2^24, exact in fp32 in any order -> bitwise"""
    C = _C()
    S = _ParamSet([(1000,), (257,), (64, 33), (5,), (59893,)],
                  shadowed=(), seed=4)
    S.opt.step()                                # builds the descriptors
    gs = _int_grads(S, _gen(12))
    want = sum((g * g).sum().item() for g in gs)
    assert want < 2 ** 24 and want == int(want)
    got = C.sq_norm_mt(S.opt._mt_desc, S.opt._mt_cum, len(S.params),
                       S.opt._mt_total)
    assert got.item() == want
    S.assert_guards()


@pytest.mark.parametrize('extra,clipped', [(0.0, False), (1.0, True)])
def test_adam_mt_clip_boundary(extra, clipped):
    """sum g^2 = 25 exactly with clip = 5: norm > clip is false, scale 1;
    sum g^2 = 26: scale 5 / sqrt(26).  Both show in m after one step."""
    S = _ParamSet([(5,), (3, 7)], shadowed=(), seed=5)
    S.grads[0][0] = 3.0
    S.grads[1][1, 2] = 4.0
    S.grads[1][2, 6] = extra
    g0 = [g.cpu().double() for g in S.grads]
    assert sum((g * g).sum().item() for g in g0) == 25.0 + extra
    S.opt.step()
    scale = 5.0 / math.sqrt(26.0) if clipped else 1.0
    for p, g in zip(S.params, g0):
        m = S.opt.state[p]['m'].cpu().double()
        want = (1.0 - float(np.float32(0.9))) * g * scale
        # one fp32 product chain: a few 2^-24 relative
        assert (m - want).abs().max().item() <= 8 * 2.0 ** -24 * 0.4
        assert (m[g == 0] == 0).all()
    # the two scales differ by 2 %: the boundary case is not clipped
    m00 = S.opt.state[S.params[0]]['m'][0].item()
    assert (abs(m00 - 0.3) < 1e-6) is (not clipped)


@pytest.mark.parametrize('grad_layout', ['channels_last', 'contiguous'])
def test_adam_mt_channels_last_param(grad_layout):
    """a channels_last 4-D parameter with a grad in either layout: the
    update pairs p, g, m, v by LOGICAL index.  The kernel walks flat
    storage, so the optimizer lays a grad out like its parameter first."""
    from sat_amd.optim import Optimizer
    gen = _gen(13)
    w = torch.randn(8, 4, 3, 3, generator=gen)
    g = torch.randn(8, 4, 3, 3, generator=gen) * 0.01
    p = torch.nn.Parameter(
        w.to(DEV).contiguous(memory_format=torch.channels_last))
    assert not p.is_contiguous()
    gd = g.to(DEV)
    if grad_layout == 'channels_last':
        gd = gd.contiguous(memory_format=torch.channels_last)
    p.grad = gd
    cfg = _cfg()
    opt = Optimizer(cfg, [p])
    opt.step()
    torch.cuda.synchronize()
    z = [torch.zeros(8, 4, 3, 3)]
    r64 = R.adam_ref([w], [g], z, z, 1, _hp(cfg), F64)
    r32 = R.adam_ref([w], [g], z, z, 1, _hp(cfg), F32)
    dref = r64[0][0] - w.double()
    floor = (((r32[0][0].double() - w.double()) - dref).abs().max()
             / dref.abs().max()).item()
    d = p.detach().cpu().double() - w.double()
    err = ((d - dref).abs().max() / dref.abs().max()).item()
    print('MEASURE adam CL param, %s grad: dp err %.2e floor %.2e'
          % (grad_layout, err, floor))
    assert err <= R.SLACK * floor           # first run: 1.16e-5 at 1.16e-5;
    #                                         m 7.0e-10, v 1.3e-11, = floors
    for k, j in (('m', 1), ('v', 2)):
        got = opt.state[p][k]
        assert got.stride() == p.stride()
        _check_fp32('adam CL param, %s grad: %s' % (grad_layout, k),
                    got, r64[j][0], r32[j][0])
    # the chosen behaviour: the grad now has the parameter's layout, and
    # it is the tensor the kernel zeroed
    assert p.grad.stride() == p.stride()
    assert (p.grad == 0).all()
    assert (p.grad is gd) is (grad_layout == 'channels_last')


# =====================================================================
# 3. masked cross-entropy and embedding
# =====================================================================

def _ce_case(B, V):
    gen = _gen(B * 10000 + V)
    x = torch.randn(B, V, generator=gen) * 3
    labels = torch.randint(0, V, (B,), generator=gen)
    mask = torch.ones(B)
    x[0, V // 2] = 40.0                 # one +40 outlier
    labels[0] = 0                       # a label at index 0
    x[1] = x[1, 0].item()               # a constant row
    labels[1] = V - 1                   # a label at V-1
    mask[2] = 0.0                       # a masked row
    if B > 3:
        mask[3] = 0.5
    dloss = torch.linspace(0.5, 2.0, B)
    return x.to(BF), labels, mask, dloss


@pytest.mark.parametrize('B,V', [(3, 7), (5, 300), (4, 5000)])
def test_ce_fwd_bwd_fp64(B, V):
    C = _C()
    x, labels, mask, dloss = _ce_case(B, V)
    xd, ld, md = x.to(DEV), labels.to(DEV), mask.to(DEV)
    losses, lse = C.ce_fwd(xd, ld, md)
    dlog = C.ce_bwd(xd, ld, md, lse, dloss.to(DEV))
    l64, s64, d64 = R.ce_ref(x, labels, mask, dloss, F64)
    l32, s32, d32 = R.ce_ref(x, labels, mask, dloss, F32)
    tag = 'ce V=%d ' % V
    # first run: lse err 3.0e-7 (V=7), 1.3e-6 (300), 6.0e-7 (5000) at
    # floors 3.0e-7, 5.6e-7, 5.2e-7; losses the same errors at floors
    # 3.0e-7, 5.6e-7, 3.5e-7 (at most 2.4 floors)
    _check_fp32(tag + 'lse', lse, s64, s32)
    _check_fp32(tag + 'losses', losses, l64, l32)
    assert losses[2].item() == 0.0
    # label and non-label entries apart: the label entry is ~ -1, the
    # other V-1 of a row ~ 1/V, and a maximum over both sees only the first
    lab = torch.zeros(B, V, dtype=torch.bool)
    lab[torch.arange(B), labels] = True
    # first run, V = 7 / 300 / 5000: err/bound 0.27 / 0.29 / 0.05 (label),
    # 0.20 / 0.78 / 0.86 (non-label); floors 2.6e-8..2.1e-7
    _check_bf16(tag + 'dlogits label', dlog, d64, d32, lab)
    _check_bf16(tag + 'dlogits non-label', dlog, d64, d32, ~lab)
    assert (dlog[2] == 0).all()                     # masked row
    assert d64[~lab].abs().max() > 0


@pytest.mark.parametrize('V,E,B', [(7, 8, 1), (50, 72, 33)])
def test_embedding_fwd_bwd_exact(V, E, B):
    C = _C()
    gen = _gen(V)
    table = torch.randn(V, E, generator=gen).to(BF)
    ids = torch.randint(0, min(V, 9), (B,), generator=gen)   # repeats
    ids[0] = 0
    ids[-1] = V - 1 if B > 1 else 0
    if B > 2:
        ids[1] = V - 1
    out = C.embedding_fwd(ids.to(DEV), table.to(DEV))
    assert torch.equal(R.bits(out), R.bits(table[ids]))
    # small integers: the atomic scatter-add is exact in any order
    dy = torch.randint(-4, 5, (B, E), generator=gen).to(BF)
    dt = C.embedding_bwd(ids.to(DEV), dy.to(DEV), V)
    want = torch.zeros(V, E, dtype=F64).index_add_(0, ids, dy.double())
    assert dt.dtype == F32 and torch.equal(dt.cpu().double(), want)
    unused = torch.ones(V, dtype=torch.bool)
    unused[ids] = False
    assert unused.any() and (dt.cpu()[unused] == 0).all()


def test_int32_labels_and_ids_raise():
    """ce_fwd, ce_bwd and embedding_bwd read their indices as int64"""
    C = _C()
    x, labels, mask, dloss = _ce_case(3, 7)
    xd, md = x.to(DEV), mask.to(DEV)
    l32 = labels.to(DEV, torch.int32)
    with pytest.raises(RuntimeError, match='int64'):
        C.ce_fwd(xd, l32, md)
    _, lse = C.ce_fwd(xd, labels.to(DEV), md)
    with pytest.raises(RuntimeError, match='int64'):
        C.ce_bwd(xd, l32, md, lse, dloss.to(DEV))
    dy = torch.ones(3, 8, dtype=BF, device=DEV)
    with pytest.raises(RuntimeError, match='int64'):
        C.embedding_bwd(torch.zeros(3, dtype=torch.int32, device=DEV),
                        dy, 7)


# =====================================================================
# 4. LSTM pointwise forward and backward
# =====================================================================

def _lstm_case(B, H):
    gen = _gen(B * 1000 + H)
    gates = torch.randn(B, 4 * H, generator=gen) * 2
    g4 = gates.view(B, 4, H)
    g4[:, :, 0:4] = 20.0                # saturated bands, both signs
    g4[:, :, 4:8] = -20.0
    g4[0, :, 8:12] = torch.tensor([20.0, -20.0, -20.0, 20.0])[:, None]
    g4[:, :, 12:16] = 0.0               # exact zeros
    c = torch.randn(B, H, generator=gen)
    dh = torch.randn(B, H, generator=gen)
    dc = torch.randn(B, H, generator=gen)
    return gates.to(BF), c.to(BF), dh.to(BF), dc.to(BF)


@pytest.mark.parametrize('fb', [0.0, 1.0])
@pytest.mark.parametrize('B,H', [(3, 40), (5, 104), (32, 64)])
def test_lstm_pointwise_fwd_bwd_fp64(B, H, fb):
    C = _C()
    gates, c, dh, dc = _lstm_case(B, H)
    gd, cd, dhd, dcd = (t.to(DEV) for t in (gates, c, dh, dc))
    tag = 'lstm %dx%d fb=%g ' % (B, H, fb)
    h1, c1 = C.lstm_pointwise_fwd(gd, cd, fb)
    h64, c64 = R.lstm_fwd_ref(gates, c, fb, F64)
    h32, c32 = R.lstm_fwd_ref(gates, c, fb, F32)
    # first run, maxima over the 12 cases: err/bound 0.97 (h), 0.99 (c),
    # 0.98 / 0.99 / 0.98 / 0.98 (di, dj, df, do), 0.99 (dc_prev), all one
    # bf16 rounding; floors 6e-8..4e-7
    _check_bf16(tag + 'h', h1, h64, h32)
    _check_bf16(tag + 'c', c1, c64, c32)
    empty = torch.empty(0, dtype=BF, device=DEV)
    for name, dc_dev, dc_cpu in (('dc', dcd, dc), ('nodc', empty, None)):
        dg, dcp = C.lstm_pointwise_bwd(gd, cd, dhd, dc_dev, fb)
        g64, p64 = R.lstm_bwd_ref(gates, c, dh, dc_cpu, fb, F64)
        g32, p32 = R.lstm_bwd_ref(gates, c, dh, dc_cpu, fb, F32)
        dg4 = dg.view(B, 4, H).cpu()
        for q, gate in enumerate('ijfo'):       # one gate cannot hide
            _check_bf16(tag + name + ' d' + gate, dg4[:, q],
                        g64[:, q], g32[:, q])
        _check_bf16(tag + name + ' dc_prev', dcp, p64, p32)
        # _out writes into the buffer it is given, same bits
        buf = torch.full((B, 4 * H), 7.0, dtype=BF, device=DEV)
        dg2, dcp2 = C.lstm_pointwise_bwd_out(gd, cd, dhd, dc_dev, fb, buf)
        assert dg2.data_ptr() == buf.data_ptr()
        assert torch.equal(R.bits(buf), R.bits(dg))
        assert torch.equal(R.bits(dcp2), R.bits(dcp))


# =====================================================================
# 5. attention pool and the NHWC scale/shift epilogue
# =====================================================================

def _pool_case(B, L, D):
    gen = _gen(B * 100000 + L * 10 + D)
    ctx = torch.randn(B, L, D, generator=gen).to(BF)
    logits = torch.randn(B, L, generator=gen)
    if B > 1:                           # (a single row stays generic)
        logits[0, L // 2] += 80.0       # a row with a +80 spike
        logits[B - 1] = 0.25            # a row all equal
    dalpha = torch.randn(B, L, generator=gen)
    dpooled = torch.randn(B, D, generator=gen).to(BF)
    return ctx, logits, dalpha, dpooled


# the spike and the flat row sit in the three shapes with B > 1; the one
# row of the D = 2048 shape is generic, so that shape checks the pooling
@pytest.mark.parametrize('B,L,D', [(2, 1, 8), (3, 5, 136), (2, 196, 512),
                                   (1, 49, 2048)])
def test_attn_pool_fwd_bwd_fp64(B, L, D):
    C = _C()
    ctx, logits, dalpha, dpooled = _pool_case(B, L, D)
    cd, ld = ctx.to(DEV), logits.to(DEV)
    tag = 'pool %dx%dx%d ' % (B, L, D)
    alpha, pooled = C.attn_pool_fwd(cd, ld)
    a64, p64 = R.attn_pool_ref(ctx, logits, F64)
    a32, p32 = R.attn_pool_ref(ctx, logits, F32)
    # first run, in the order of the shapes: alpha err 0 / 1.0e-8 /
    # 1.0e-10 / 5.4e-9 at floors 0 / 1.0e-8 / 1.0e-10 / 3.0e-9; pooled and
    # dctx err/bound <= 0.994; dlogits err 0 and 3.3e-8..6.5e-7 at floors 0
    # and 7.0e-8..6.6e-7 (at most 2.2 floors)
    _check_fp32(tag + 'alpha', alpha, a64, a32)
    # sum alpha = 1: every alpha_l carries one rounding, the tree sum of z
    # at most L/256 + 10 more, 1/z one -> below 16 * 2^-24 for L <= 1024
    srow = alpha.double().sum(1).cpu()
    esum = (srow - 1).abs().max().item()
    print('MEASURE %-34s err %.3e bound %.3e'
          % (tag + 'sum alpha', esum, 16 * 2.0 ** -24))
    assert esum <= 16 * 2.0 ** -24          # first run: at most 2.0e-8
    _check_bf16(tag + 'pooled', pooled, p64, p32)
    empty = torch.empty(0, device=DEV)
    for name, da_dev, da_cpu in (('da', dalpha.to(DEV), dalpha),
                                 ('noda', empty, None)):
        dl, dctx = C.attn_pool_bwd(cd, alpha, da_dev, dpooled.to(DEV), True)
        l64, c64 = R.attn_pool_bwd_ref(ctx, logits, da_cpu, dpooled, F64)
        l32, c32 = R.attn_pool_bwd_ref(ctx, logits, da_cpu, dpooled, F32)
        _check_fp32(tag + name + ' dlogits', dl, l64, l32)
        _check_bf16(tag + name + ' dctx', dctx, c64, c32)
        dl2, none = C.attn_pool_bwd(cd, alpha, da_dev, dpooled.to(DEV),
                                    False)
        assert none.numel() == 0
        assert torch.equal(dl2, dl)


def test_attn_pool_fwd_rejects_ragged_d():
    """the kernel reads ctx 8 columns at a time, as its backward does"""
    C = _C()
    ctx = torch.zeros(1, 2, 20, dtype=BF, device=DEV)
    with pytest.raises(RuntimeError, match='D % 8'):
        C.attn_pool_fwd(ctx, torch.zeros(1, 2, device=DEV))


@pytest.mark.parametrize('relu', [True, False])
@pytest.mark.parametrize('shape', [(2, 16, 7, 9), (1, 72, 5, 5)])
def test_scale_bias_act_nhwc_fp64(shape, relu):
    C = _C()
    gen = _gen(shape[1])
    x = torch.randn(shape, generator=gen).to(BF)
    scale = (torch.rand(shape[1], generator=gen) * 1.5 + 0.25).to(BF)
    shift = torch.randn(shape[1], generator=gen).to(BF)
    y = x.to(DEV).contiguous(memory_format=torch.channels_last)
    C.scale_bias_act_nhwc(y, scale.to(DEV), shift.to(DEV), relu)
    r64 = R.scale_shift_ref(x, scale, shift, relu, F64)
    r32 = R.scale_shift_ref(x, scale, shift, relu, F32)
    assert y.is_contiguous(memory_format=torch.channels_last)
    # first run: err/bound 0.93..0.98, floor 6.0e-8
    _check_bf16('scale_bias_act %s relu=%s' % (shape, relu), y, r64, r32)
    if relu:
        assert (y.cpu()[r64 == 0] == 0).all()
