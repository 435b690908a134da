"""Fused beam-search decoder on the GPU: the two kernels against their
references, the engine graph against eager, its step numerics against the
existing decode_step and an fp32 CPU model, cache invalidation and the
public entry points."""

import copy

import pytest
import torch

from sat_amd.ops import functional as F

from _beam_refs import (beam_inputs, fresh_state, rand_bf16_logits,
                        stable_topk_ref)

pytestmark = pytest.mark.gpu

DEV = 'cuda'


# ---- 5. softmax_topk kernel against the fp64 softmax ----

@pytest.mark.parametrize('R,V,K', [(4, 40, 4), (6, 1000, 4), (5, 1001, 3),
                                   (3, 16, 9), (195, 5000, 4),
                                   (1, 5000, 9)])
def test_softmax_topk_kernel(R, V, K):
    from sat_amd import ops
    logits = rand_bf16_logits(R, V, K, seed=R + V + K) if R > 1 else \
        (torch.randn(1, V, generator=torch.Generator().manual_seed(V))
         * 3.0).bfloat16().float()
    # one row with logits spanning +-80
    span = torch.linspace(-80.0, 80.0, V)[
        torch.randperm(V, generator=torch.Generator().manual_seed(1))]
    logits[R - 1] = span.bfloat16().float()
    p_ref, idx_ref = stable_topk_ref(logits, K)
    p, idx = ops.softmax_topk(logits.to(DEV).bfloat16(), K)
    assert p.dtype == torch.float32 and idx.dtype == torch.int64
    assert torch.equal(idx.cpu(), idx_ref)
    rel = ((p.cpu().double() - p_ref).abs() / p_ref).max().item()
    print('softmax_topk R=%d V=%d K=%d: max rel err %.3g' % (R, V, K, rel))
    assert rel <= 1e-5


# ---- 6. beam_advance kernel against F.beam_advance ----

@pytest.mark.parametrize('HE', [32, 512])
@pytest.mark.parametrize('B,W,K,T', [(1, 1, 2, 4), (2, 3, 4, 8),
                                     (5, 8, 9, 20)])
def test_beam_advance_kernel(B, W, K, T, HE):
    from sat_amd import ops
    H = E = D = HE
    V, period = 50, 7
    g = torch.Generator().manual_seed(B * 100 + W + HE)
    table = torch.randn(V, E, generator=g).bfloat16()
    table_d = table.to(DEV)
    N = B * W
    cur, nxt = fresh_state(B, W, T), fresh_state(B, W, T)

    def outs(device, dtype=torch.bfloat16):
        z = dict(device=device)
        return (torch.zeros(N, H, dtype=dtype, **z),
                torch.zeros(N, D + E + H, dtype=dtype, **z),
                torch.zeros(N, H + D + E, dtype=dtype, **z),
                torch.zeros(N, dtype=torch.int64, **z),
                torch.zeros(B, W, dtype=torch.int64, **z))

    for t in range(T):
        top_p, top_w = beam_inputs(B, W, K, V, period, g)
        mem_new = torch.randn(N, H, generator=g).bfloat16()
        h_new = torch.randn(N, H, generator=g).bfloat16()
        o_ref = outs('cpu')
        F.beam_advance(cur, nxt, top_p, top_w, period, mem_new, h_new,
                       table, *o_ref)
        o_gpu = outs(DEV)
        nxt_d = fresh_state(B, W, T, DEV)
        ops.beam_advance(tuple(x.to(DEV) for x in cur), nxt_d,
                         top_p.to(DEV), top_w.to(DEV), period,
                         mem_new.to(DEV), h_new.to(DEV), table_d, *o_gpu)
        got = [x.cpu() for x in nxt_d]
        mem_g, xh_g, exp_g, word_g, par_g = [x.cpu() for x in o_gpu]
        mem_r, xh_r, exp_r, word_r, par_r = o_ref
        assert torch.equal(got[0], nxt[0])        # fp64, bitwise
        assert torch.equal(got[3], nxt[3])
        live, done = nxt[0] > 0, nxt[3] > 0
        assert torch.equal(par_g[live], par_r[live])
        assert torch.equal(word_g.reshape(B, W)[live],
                           word_r.reshape(B, W)[live])
        assert torch.equal(got[1][live], nxt[1][live])
        assert torch.equal(got[2][live], nxt[2][live])
        assert torch.equal(got[4][done], nxt[4][done])
        assert torch.equal(got[5][done], nxt[5][done])
        rows = live.reshape(-1)

        def same(a, b):
            return torch.equal(a[rows].view(torch.int16),
                               b[rows].view(torch.int16))
        assert same(mem_g, mem_r) and same(xh_g, xh_r)
        assert same(exp_g, exp_r)
        cur, nxt = nxt, cur


# ---- the engine ----

def _model(V=1000, T=20, H=512, E=512, Dd=1024, cnn='vgg16', seed=11,
           period_bias=0.0, period=5):
    from config import Config
    from sat_amd.models.caption_generator import CaptionGenerator
    cfg = Config()
    cfg.phase = 'eval'
    cfg.train_cnn = False
    cfg.cnn = cnn
    cfg.vocabulary_size = V
    cfg.max_caption_length = T
    cfg.num_lstm_units = H
    cfg.dim_embedding = E
    cfg.dim_initalize_layer = H
    cfg.dim_decode_layer = Dd
    torch.manual_seed(seed)
    model = CaptionGenerator(cfg)
    if period_bias:
        with torch.no_grad():
            model.decoder.dec_fc_2.bias[period] += period_bias
    return model.to(DEV).eval()


def _contexts(B, L, D, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, L, D, generator=g).abs().to(DEV).bfloat16()


def _caps(res):
    return [[(list(c.sentence), c.score) for c in caps] for caps in res]


@pytest.mark.parametrize('case', ['flagship_2x3', 'flagship_1x1',
                                  'resnet_grid', 'unfused_lstm_130'])
def test_engine_graph_matches_eager(case):
    from sat_amd.beam import FusedBeamDecoder
    if case == 'flagship_2x3':
        model, B, W = _model(), 2, 3
    elif case == 'flagship_1x1':
        model, B, W = _model(), 1, 1
    elif case == 'resnet_grid':
        model, B, W = _model(V=100, T=6, H=64, E=64, Dd=64,
                             cnn='resnet50'), 2, 3
    else:
        model, B, W = _model(V=100, T=4), 26, 5
    L, D = model.num_ctx, model.dim_ctx
    if case == 'resnet_grid':
        assert (L, D) == (49, 2048)
    ctx1, ctx2 = _contexts(B, L, D, 1), _contexts(B, L, D, 2)
    eng = FusedBeamDecoder(model)
    assert eng.mode(True, torch.bfloat16, W) == 'hip'
    graphed = _caps(eng.search(ctx1, 5, W, graph=True))
    assert (B, W, model.config.max_caption_length) in eng._graphs
    eager = _caps(eng.search(ctx1, 5, W, graph=False))
    assert graphed == eager                 # captions and scores, bitwise
    assert len(graphed) == B and all(1 <= len(c) <= W for c in graphed)
    # a second replay, on new contexts, against a fresh engine
    replay = _caps(eng.search(ctx2, 5, W, graph=True))
    fresh = _caps(FusedBeamDecoder(model).search(ctx2, 5, W, graph=False))
    assert replay == fresh
    assert replay != graphed


@pytest.fixture(scope='module')
def traced():
    """The (2,3) flagship case with its trace, plus per step the
    probabilities of (a) the existing GPU decode_step and (b) decode_step
    of an fp32 CPU copy of the model, on the trace's own input state."""
    from sat_amd.beam import FusedBeamDecoder
    B, W, period = 2, 3, 5
    # the untrained model's logits spread over about +-4: a bias of 5 puts
    # the period among every row's top K, so each step merges completed
    # candidates (checked on the CPU twin: none at +1 or +3)
    model = _model(period_bias=5.0, period=period)
    cpu = copy.deepcopy(model).float().cpu()
    ctx = _contexts(B, model.num_ctx, model.dim_ctx, 3)
    ctx_rep = ctx.repeat_interleave(W, dim=0)
    ctx_rep_cpu = ctx_rep.float().cpu()
    res, trace = FusedBeamDecoder(model).search(ctx, period, W,
                                                return_trace=True)
    pa, pb = [], []
    for rec in trace:
        _m, _o, p = model.decode_step(ctx_rep, rec['last_word'],
                                      rec['memory'], rec['output'])
        pa.append(p.double().cpu())
        _m, _o, p = cpu.decode_step(ctx_rep_cpu, rec['last_word'].cpu(),
                                    rec['memory'].float().cpu(),
                                    rec['output'].float().cpu())
        pb.append(p.double())
    d_eng = d_gpu = 0.0
    for rec, a, b in zip(trace, pa, pb):
        idx = rec['top_w'].cpu()
        ref = b.gather(1, idx)
        d_eng = max(d_eng, ((rec['top_p'].cpu().double() - ref).abs()
                            / ref).max().item())
        d_gpu = max(d_gpu, ((a.gather(1, idx) - ref).abs()
                            / ref).max().item())
    return dict(B=B, W=W, K=W + 1, period=period, res=res, trace=trace,
                pa=pa, d_eng=d_eng, d_gpu=d_gpu,
                eps=2.0 * d_gpu + 2.0 ** -7)


def test_step_numerics(traced):
    """d(x): largest relative deviation from the fp32 CPU model over the
    engine's top-K entries of every step."""
    print('step numerics: d(engine) = %.4g, d(existing GPU path) = %.4g, '
          'bound = %.4g' % (traced['d_eng'], traced['d_gpu'],
                            traced['eps']))
    assert traced['d_eng'] <= 2.0 * traced['d_gpu'] + 2.0 ** -7


def test_selections_valid_under_existing_probs(traced):
    """Every selection of every step is a valid one under the existing
    path's probabilities (a), up to eps = the bound of test_step_numerics.
    Candidates are all V words of every live parent: a word outside its
    parent's top K has K better siblings, at most one of them the period,
    so it cannot be among the best W anyway."""
    B, W, K = traced['B'], traced['W'], traced['K']
    period, eps = traced['period'], traced['eps']
    n_completed = 0
    for rec, pa in zip(traced['trace'], traced['pa']):
        V = pa.shape[1]
        s_in = rec['scores_in'].cpu()
        cand = (s_in.unsqueeze(2) * pa.reshape(B, W, V))     # [B,W,V]
        parent, word = rec['parent'].cpu(), rec['word'].cpu()
        score = rec['score'].cpu()
        top_w = rec['top_w'].cpu().reshape(B, W, K)
        top_p = rec['top_p'].cpu().double().reshape(B, W, K)
        c_in, c_out = rec['c_scores_in'].cpu(), rec['c_scores'].cpu()
        for b in range(B):
            # ---- live set ----
            sel = score[b] > 0
            assert sel.any()
            mask = torch.ones(W, V, dtype=torch.bool)
            mask[:, period] = False
            for w in torch.nonzero(sel).flatten().tolist():
                p, v = int(parent[b, w]), int(word[b, w])
                assert v != period
                ref = cand[b, p, v].item()
                assert abs(score[b, w].item() - ref) <= eps * ref
                mask[p, v] = False
            weakest = score[b][sel].min().item()
            rest = cand[b][mask]
            if not sel.all():
                # a dead slot: no positive candidate may be left over
                assert rest.max().item() <= 0.0
            assert rest.max().item() <= weakest * (1.0 + 2.0 * eps)

            # ---- completed merge ----
            e_per = top_w[b] == period                       # [W,K]
            e_score = (s_in[b].unsqueeze(1) * top_p[b])[e_per]
            a_score = (s_in[b].unsqueeze(1)
                       * pa.reshape(B, W, V)[b, :, period].unsqueeze(1)
                       .expand(W, K))[e_per]
            pool_e = torch.cat([c_in[b], e_score])
            pool_a = torch.cat([c_in[b], a_score])
            # a period clearly inside a parent's top K under (a) must be
            # among the engine's candidates
            kth = pa.reshape(B, W, V)[b].topk(K, dim=1)[0][:, K - 1]
            clear = (pa.reshape(B, W, V)[b, :, period]
                     > kth * (1.0 + 2.0 * eps)) & (s_in[b] > 0)
            assert bool((e_per.any(dim=1) | ~clear).all())
            # the engine keeps the best W of its own pool, exactly
            best = pool_e.sort(descending=True)[0][:W]
            assert torch.equal(c_out[b], best)
            kept = c_out[b] > 0
            n_completed += int(kept.sum())
            if kept.any():
                order = pool_e.sort(descending=True, stable=True)[1]
                for j in order[:W][kept].tolist():
                    ref = pool_a[j].item()
                    assert abs(pool_e[j].item() - ref) <= eps * ref
                weakest = c_out[b][kept].min().item()
                left = pool_a[order[W:]]
                if left.numel():
                    if not kept.all():
                        assert left.max().item() <= 0.0
                    assert left.max().item() <= weakest * (1 + 2 * eps)
    assert n_completed > 0          # the completed merge was exercised
    for caps in traced['res']:
        assert caps[0].sentence[-1] == period


# ---- 10. cache invalidation ----

def test_weight_cache_invalidation():
    from sat_amd.beam import FusedBeamDecoder
    model = _model(V=1000, T=8)
    B, W = 2, 3
    ctx = _contexts(B, model.num_ctx, model.dim_ctx, 4)
    eng = FusedBeamDecoder(model)
    first = _caps(eng.search(ctx, 5, W))
    g = torch.Generator().manual_seed(9)
    with torch.no_grad():
        for p in model.decoder.parameters():
            new = torch.rand(p.shape, generator=g) * 0.16 - 0.08
            p.copy_(new.to(DEV))
    second = _caps(eng.search(ctx, 5, W))
    fresh = _caps(FusedBeamDecoder(model).search(ctx, 5, W))
    assert second == fresh
    assert second != first


# ---- 11. through the front door ----

def test_front_door(tiny_config):
    from sat_amd.data.dataset import prepare_eval_data
    from sat_amd.models.base_model import BaseModel
    cfg = tiny_config
    cfg.device = 'cuda'
    cfg.phase = 'eval'
    cfg.vocabulary_size = 1000
    cfg.dim_embedding = 512
    cfg.num_lstm_units = 512
    cfg.dim_initalize_layer = 512
    cfg.dim_attend_layer = 512
    cfg.dim_decode_layer = 1024
    cfg.beam_size = 3
    cfg.batch_size = 2
    cfg.use_fused_beam = True
    coco, data, vocab = prepare_eval_data(cfg)
    m = BaseModel(cfg)
    assert m._fused_beam_mode() == 'hip'
    calls = []
    orig = m.beam_search_fused

    def fused(files, vocabulary):
        calls.append(len(files))
        return orig(files, vocabulary)
    m.beam_search_fused = fused
    scores = m.eval(coco, data, vocab)
    assert set(scores) >= {'Bleu_1', 'Bleu_4', 'CIDEr'}
    assert calls and all(n == 2 for n in calls)
    res = m.beam_search(['synthetic://0', 'synthetic://1'], vocab)
    assert len(res) == 2
    for caps in res:
        assert 1 <= len(caps) <= 3
        s = [c.score for c in caps]
        assert s == sorted(s, reverse=True)
