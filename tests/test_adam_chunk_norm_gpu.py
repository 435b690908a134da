"""GPU tests of Adam on the chunk table (sq_norm_chunks + opt_step_mt):
with a norm that is exact in any order, Optimizer.step() must leave the
bits that the per-element-search pair sq_norm_mt + adam_step_mt leaves."""

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = 'cuda'
BF = torch.bfloat16
# the parameter shapes of test_sq_norm_mt_exact (tests/test_tail_ops_gpu.py)
SHAPES = [(1000,), (257,), (64, 33), (5,), (59893,)]
SHADOWED = (1, 4)


def _cfg(clip):
    from config import Config
    cfg = Config()
    cfg.initial_learning_rate = 1e-2
    cfg.learning_rate_decay_factor = 0.5
    cfg.num_steps_per_decay = 3
    cfg.clip_gradients = clip
    return cfg


class _Set(object):
    def __init__(self, clip, seed=0, offset=()):
        """`offset`: indices of the parameters that start one element into
        their storage; such a tensor takes the element route of the chunk
        kernels (all of them: the build without the 16-byte route)"""
        from sat_amd.optim import Optimizer
        gen = torch.Generator().manual_seed(seed)
        self.params = []
        for i, s in enumerate(SHAPES):
            v = (torch.rand(s, generator=gen) * 2 - 1).to(DEV)
            if i in offset:
                buf = torch.empty(v.numel() + 1, device=DEV)
                buf[1:].copy_(v.reshape(-1))
                v = buf[1:].view(s)
                assert v.data_ptr() % 16 == 4
            self.params.append(torch.nn.Parameter(v))
        for p in self.params:
            p.grad = torch.zeros_like(p)
        self.cfg = _cfg(clip)
        self.opt = Optimizer(self.cfg, self.params)
        self.shadows = {self.params[i]: torch.empty_like(self.params[i],
                                                         dtype=BF)
                        for i in SHADOWED}
        self.opt.register_shadows(self.shadows)

    def fill(self, grads):
        for p, g in zip(self.params, grads):
            p.grad.copy_(g)

    def state(self):
        st = self.opt.state
        return ([p.detach().clone() for p in self.params]
                + [st[p]['m'].clone() for p in self.params]
                + [st[p]['v'].clone() for p in self.params]
                + [self.shadows[self.params[i]].clone() for i in SHADOWED])


def _int_grads(seed):
    """integers, |g| <= 8, sum of squares below 2^24: every partial sum of
    squares and their total are exact in fp32, in any order"""
    gen = torch.Generator().manual_seed(seed)
    gs = [torch.randint(-8, 9, s, generator=gen).float() for s in SHAPES]
    total = sum((g * g).sum().item() for g in gs)
    assert 0 < total < 2 ** 24 and total == int(total)
    return gs, total


def _old_route_step(S):
    """one step through _C.sq_norm_mt + _C.adam_step_mt, with the
    descriptors Optimizer.step() keeps building"""
    from sat_amd import _C
    cfg, opt = S.cfg, S.opt
    opt.step_count += 1
    opt.step_dev.add_(1.0)
    gsq = _C.sq_norm_mt(opt._mt_desc, opt._mt_cum, len(opt.params),
                        opt._mt_total)
    _C.adam_step_mt(opt._mt_desc, opt._mt_cum, len(opt.params),
                    opt._mt_total, opt.step_dev, cfg.initial_learning_rate,
                    cfg.learning_rate_decay_factor, cfg.num_steps_per_decay,
                    cfg.beta1, cfg.beta2, cfg.epsilon, cfg.clip_gradients,
                    gsq, True, opt._mt_vec4)


OFFSETS = {'vec': (), 'mixed': (0, 2), 'element': tuple(range(len(SHAPES)))}


@pytest.mark.parametrize('route', sorted(OFFSETS))
@pytest.mark.parametrize('clipped', [True, False])
def test_chunk_route_matches_search_route(clipped, route):
    gs, total = _int_grads(21)
    norm = total ** 0.5
    clip = norm / 4 if clipped else norm * 4
    off = OFFSETS[route]
    A, B = _Set(clip, seed=3, offset=off), _Set(clip, seed=3, offset=off)
    assert getattr(A.cfg, 'use_adam_chunk_norm', True)
    # step 1 on both through step(): it builds the descriptors of both
    # routes; zero grads leave p, m, v as they are
    A.opt.step()
    B.opt.step()
    for a, b in zip(A.state(), B.state()):
        assert torch.equal(a, b)
    for t in range(2):
        A.fill(gs)
        B.fill(gs)
        A.opt.step()
        _old_route_step(B)
        torch.cuda.synchronize()
        for k, (a, b) in enumerate(zip(A.state(), B.state())):
            assert torch.equal(a, b), (t, k)
        for S in (A, B):
            for p in S.params:
                assert not bool((p.grad != 0).any())
    assert A.opt.step_dev.item() == B.opt.step_dev.item() == 3
    assert A.opt._ck_any_vec is (route != 'element')
    assert A.opt._ck_vec.tolist() == [int(i not in off)
                                      for i in range(len(SHAPES))]
    # the update did move the parameters, and the clip branch is the one
    # this case names
    fresh = _Set(clip, seed=3, offset=off)
    assert not torch.equal(fresh.params[0], A.params[0])
    assert (norm > clip) is clipped


def test_chunk_route_graph_replay():
    """step() captured once, replayed three times with grads refilled in
    place: the device counter advances and the bits are those of eager
    steps"""
    sets = [_int_grads(30 + k)[0] for k in range(3)]
    clip = 40.0
    G, E = _Set(clip, seed=5), _Set(clip, seed=5)
    G.opt.step()                                # builds the tables
    E.opt.step()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        G.opt.step()
    torch.cuda.synchronize()
    assert G.opt.step_dev.item() == 1           # capture ran nothing
    for k, gs in enumerate(sets):
        G.fill(gs)
        E.fill(gs)
        graph.replay()
        E.opt.step()
        torch.cuda.synchronize()
        assert G.opt.step_dev.item() == 2 + k
        for j, (a, b) in enumerate(zip(G.state(), E.state())):
            assert torch.equal(a, b), (k, j)
