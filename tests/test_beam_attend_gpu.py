"""In-loop 1-layer attention of the fused beam decoder on the GPU: the
beam_attend kernel against fp64, the engine graph against eager for the
1-layer architectures, its step numerics and selections against the
existing decode_step, cache invalidation and the front door."""

import copy

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = 'cuda'
FC_SCALE = 0.08     # Config.fc_kernel_initializer_scale: uniform +-0.08


# ---- 4. the kernel against fp64 ----

def _attend_inputs(B, W, L, D, E, H, seed):
    g = torch.Generator().manual_seed(seed)

    def uni(*shape):
        return torch.rand(*shape, generator=g) * 2.0 - 1.0
    ctx = torch.randn(B, L, D, generator=g).abs().bfloat16()
    wa = (uni(D) * FC_SCALE).bfloat16()
    wb = (uni(L, H) * FC_SCALE).bfloat16()
    l1 = ctx.float().matmul(wa.float())                 # [B,L] fp32
    xh = torch.randn(B * W, D + E + H, generator=g).bfloat16()
    xh[:, D + E:] = uni(B * W, H).bfloat16()
    return ctx, l1, wb, xh


def _attend_ref(ctx, l1, wb, xh, W):
    """The three formulas in fp64 on the bf16 inputs."""
    H = wb.shape[1]
    h = xh[:, xh.shape[1] - H:].double()
    logit = l1.double().repeat_interleave(W, dim=0) \
        + h.matmul(wb.double().t())
    alpha = torch.softmax(logit, dim=1)
    B, L, D = ctx.shape
    pooled = torch.bmm(alpha.reshape(B, W, L), ctx.double()) \
        .reshape(B * W, D)
    return alpha, pooled


def _bits(t):
    return t.contiguous().view(torch.int16)


def _max_ctx():
    from sat_amd.beam import MAX_CTX
    return MAX_CTX


@pytest.mark.parametrize('case', ['flagship_1x1', 'flagship_2x3',
                                  'resnet_grid_w8', 'tiny_l7',
                                  'odd_dims', 'l_limit'])
def test_beam_attend_kernel(case):
    from sat_amd import ops
    B, W, L, D, E, H = {
        'flagship_1x1': (1, 1, 196, 512, 512, 512),
        'flagship_2x3': (2, 3, 196, 512, 512, 512),
        'resnet_grid_w8': (3, 8, 49, 2048, 16, 64),
        'tiny_l7': (2, 5, 7, 8, 8, 8),
        'odd_dims': (2, 3, 50, 40, 24, 72),
        'l_limit': (1, 2, _max_ctx(), 16, 8, 24),
    }[case]
    ctx, l1, wb, xh = _attend_inputs(B, W, L, D, E, H, seed=B + W + L + D)
    a_ref, p_ref = _attend_ref(ctx, l1, wb, xh, W)
    N = B * W
    ctx_d, l1_d, wb_d = ctx.to(DEV), l1.to(DEV), wb.to(DEV)

    def launch():
        xh_d = xh.to(DEV)
        pool = torch.zeros(N, D, dtype=torch.bfloat16, device=DEV)
        alpha = torch.zeros(N, L, dtype=torch.float32, device=DEV)
        ops.beam_attend(ctx_d, l1_d, wb_d, xh_d, pool, alpha)
        return xh_d.cpu(), pool.cpu(), alpha.cpu()
    xh_g, pool_g, alpha_g = launch()

    # the existing path on the same inputs, as Decoder.attend computes it
    ctx_rep = ctx_d.repeat_interleave(W, dim=0)
    l2 = xh[:, D + E:].to(DEV).matmul(wb_d.t())                  # bf16
    logits = (l1_d.repeat_interleave(W, dim=0) + l2.float()).bfloat16()
    a_old, _p_old = ops.attention_pool(ctx_rep, logits)

    err = (pool_g.double() - p_ref).abs()
    rel = (err / p_ref.abs().clamp_min(1e-300)).max().item()
    d_new = (alpha_g.double() - a_ref).abs().max().item()
    d_old = (a_old.cpu().double() - a_ref).abs().max().item()
    print('beam_attend %s: pooled max rel err %.4g (bound %.4g); '
          'max|alpha - ref| = %.4g, existing path %.4g'
          % (case, rel, 2.0 ** -8, d_new, d_old))
    assert bool((err <= 2.0 ** -8 * p_ref.abs()).all())
    assert (alpha_g.sum(dim=1) - 1.0).abs().max().item() <= 1e-5
    assert d_new <= d_old

    # in-place contract
    assert torch.equal(_bits(xh_g[:, :D]), _bits(pool_g))
    assert torch.equal(_bits(xh_g[:, D:]), _bits(xh[:, D:]))
    # alpha is optional: without it the same pooled bits
    xh_e = xh.to(DEV)
    pool_e = torch.zeros(N, D, dtype=torch.bfloat16, device=DEV)
    ops.beam_attend(ctx_d, l1_d, wb_d, xh_e, pool_e)
    assert torch.equal(_bits(pool_e.cpu()), _bits(pool_g))
    # a second launch gives identical bits
    xh_2, pool_2, alpha_2 = launch()
    assert torch.equal(_bits(pool_2), _bits(pool_g))
    assert torch.equal(_bits(xh_2), _bits(xh_g))
    assert torch.equal(alpha_2, alpha_g)


@pytest.mark.parametrize('split', [1, 2, 4, 5])
def test_beam_attend_explicit_split(split):
    """Blocks per image, set by hand on the 5 column vectors of the odd
    shape: even and uneven slices, and with 4 a block left without one.
    Same bound as above."""
    from sat_amd.ops import hip
    B, W, L, D, E, H = 2, 3, 50, 40, 24, 72
    ctx, l1, wb, xh = _attend_inputs(B, W, L, D, E, H, seed=split)
    a_ref, p_ref = _attend_ref(ctx, l1, wb, xh, W)
    xh_d = xh.to(DEV)
    pool = torch.zeros(B * W, D, dtype=torch.bfloat16, device=DEV)
    alpha = torch.zeros(B * W, L, dtype=torch.float32, device=DEV)
    hip.beam_attend(ctx.to(DEV), l1.to(DEV), wb.to(DEV), xh_d, pool,
                    alpha, split=split)
    err = (pool.cpu().double() - p_ref).abs()
    assert bool((err <= 2.0 ** -8 * p_ref.abs()).all())
    assert (alpha.cpu().double() - a_ref).abs().max().item() <= 1e-5
    assert torch.equal(_bits(xh_d[:, :D]).cpu(), _bits(pool).cpu())
    assert torch.equal(_bits(xh_d[:, D:]).cpu(), _bits(xh[:, D:]))
    with pytest.raises(RuntimeError):
        hip.beam_attend(ctx.to(DEV), l1.to(DEV), wb.to(DEV), xh_d, pool,
                        alpha, split=D // 8 + 1)


def test_beam_attend_rejects_bad_arguments():
    from sat_amd import ops
    B, W, L, D, E, H = 1, 2, 16, 16, 8, 24
    ctx, l1, wb, xh = [t.to(DEV) for t in
                       _attend_inputs(B, W, L, D, E, H, seed=1)]

    def pool(n=B * W):
        return torch.zeros(n, D, dtype=torch.bfloat16, device=DEV)
    p = pool()
    ops.beam_attend(ctx, l1, wb, xh, p)                 # the valid call
    assert p.any()

    # W = 9
    xh9 = torch.zeros(9, D + E + H, dtype=torch.bfloat16, device=DEV)
    p9 = pool(9)
    with pytest.raises(RuntimeError):
        ops.beam_attend(ctx, l1, wb, xh9, p9)
    assert not p9.any()
    # xh off the 16-byte grid
    flat = torch.zeros(B * W * (D + E + H) + 8, dtype=torch.bfloat16,
                       device=DEV)
    xh_off = flat[4:4 + B * W * (D + E + H)].view(B * W, D + E + H)
    assert xh_off.is_contiguous() and xh_off.data_ptr() % 16 == 8
    p = pool()
    with pytest.raises(RuntimeError):
        ops.beam_attend(ctx, l1, wb, xh_off, p)
    assert not p.any()
    # L above the limit
    L2 = _max_ctx() + 1
    ctx2, l12, wb2, xh2 = [t.to(DEV) for t in
                           _attend_inputs(B, W, L2, D, E, H, seed=2)]
    p = pool()
    with pytest.raises(RuntimeError):
        ops.beam_attend(ctx2, l12, wb2, xh2, p)
    assert not p.any()


# ---- the engine with 1-layer attention ----

_MODELS = {}


def _model(decode=2, V=1000, T=20, H=512, E=512, Dd=1024, cnn='vgg16',
           seed=11, period_bias=0.0, period=5):
    """An eval CaptionGenerator with num_attend_layers = 1 on the GPU
    (cached per argument set; tests that write weights pass a seed of
    their own)."""
    key = (decode, V, T, H, E, Dd, cnn, seed, period_bias, period)
    if key in _MODELS:
        return _MODELS[key]
    from config import Config
    from sat_amd.models.caption_generator import CaptionGenerator
    cfg = Config()
    cfg.phase = 'eval'
    cfg.train_cnn = False
    cfg.cnn = cnn
    cfg.num_attend_layers = 1
    cfg.num_decode_layers = decode
    cfg.vocabulary_size = V
    cfg.max_caption_length = T
    cfg.num_lstm_units = H
    cfg.dim_embedding = E
    cfg.dim_initalize_layer = H
    cfg.dim_decode_layer = Dd
    torch.manual_seed(seed)
    model = CaptionGenerator(cfg)
    if period_bias:
        fc = model.decoder.dec_fc if decode == 1 \
            else model.decoder.dec_fc_2
        with torch.no_grad():
            fc.bias[period] += period_bias
    _MODELS[key] = model.to(DEV).eval()
    return _MODELS[key]


def _contexts(B, L, D, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, L, D, generator=g).abs().to(DEV).bfloat16()


def _caps(res):
    return [[(list(c.sentence), c.score) for c in caps] for caps in res]


# ---- 5. graph against eager ----

@pytest.mark.parametrize('decode', [2, 1])
@pytest.mark.parametrize('case', ['flagship_2x3', 'flagship_1x1',
                                  'resnet_grid', 'unfused_lstm_130'])
def test_engine_graph_matches_eager(case, decode):
    from sat_amd.beam import FusedBeamDecoder
    if case == 'flagship_2x3':
        model, B, W = _model(decode), 2, 3
    elif case == 'flagship_1x1':
        model, B, W = _model(decode), 1, 1
    elif case == 'resnet_grid':
        model, B, W = _model(decode, V=100, T=6, H=64, E=64, Dd=64,
                             cnn='resnet50'), 2, 3
    else:
        model, B, W = _model(decode, V=100, T=4), 26, 5
    L, D = model.num_ctx, model.dim_ctx
    if case == 'resnet_grid':
        assert (L, D) == (49, 2048)
    ctx1, ctx2 = _contexts(B, L, D, 1), _contexts(B, L, D, 2)
    eng = FusedBeamDecoder(model)
    assert eng.inloop and eng.mode(True, torch.bfloat16, W) == 'hip'
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


# ---- 6. step numerics and selections ----

@pytest.fixture(scope='module')
def traced():
    """The (2,3) flagship case of the 1-layer-attention model with its
    trace, plus per step the probabilities of (a) the existing GPU
    decode_step and (b) decode_step of an fp32 CPU copy of the model, on
    the trace's own input state."""
    from sat_amd.beam import FusedBeamDecoder
    B, W, period = 2, 3, 5
    # the decode MLP is the one of the 2-layer model, its logits spread
    # over about +-4, and a bias of 5 puts the period among every live
    # row's top K at every step, so each step merges completed candidates
    # (checked on the CPU twin with search(mode='twin') on an fp32 copy of
    # this model and these contexts: the period is in top_w of every row
    # with a positive score at all 20 steps, and both best captions end
    # with it)
    model = _model(2, seed=11, period_bias=5.0, period=period)
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
    print('in-loop step numerics: d(engine) = %.4g, d(existing GPU path) '
          '= %.4g, bound = %.4g' % (traced['d_eng'], traced['d_gpu'],
                                    traced['eps']))
    assert traced['d_eng'] <= 2.0 * traced['d_gpu'] + 2.0 ** -7


def test_trace_alpha(traced):
    B, W = traced['B'], traced['W']
    trace = traced['trace']
    for rec in trace:
        a = rec['alpha']
        assert a.shape[0] == B * W and a.dtype == torch.float32
        assert (a.sum(dim=1) - 1.0).abs().max().item() <= 1e-5
    assert not torch.equal(trace[0]['alpha'], trace[1]['alpha'])


def test_selections_valid_under_existing_probs(traced):
    import test_fused_beam_gpu as existing
    existing.test_selections_valid_under_existing_probs(traced)


# ---- 7. cache invalidation ----

def test_weight_cache_invalidation():
    from sat_amd.beam import FusedBeamDecoder
    model = _model(2, V=1000, T=8, seed=12)     # written below: own model
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


# ---- 8. through the front door ----

def test_front_door(tiny_config):
    from sat_amd.data.dataset import prepare_eval_data
    from sat_amd.models.base_model import BaseModel
    cfg = tiny_config
    cfg.device = 'cuda'
    cfg.phase = 'eval'
    cfg.num_attend_layers = 1
    cfg.vocabulary_size = 1000
    cfg.dim_embedding = 512
    cfg.num_lstm_units = 512
    cfg.dim_initalize_layer = 512
    cfg.dim_decode_layer = 1024
    cfg.beam_size = 3
    cfg.batch_size = 2
    cfg.use_fused_beam = True
    coco, data, vocab = prepare_eval_data(cfg)
    m = BaseModel(cfg)
    assert m._fused_beam_mode() == 'hip'
    calls, fallbacks = [], []
    orig, orig_dev = m.beam_search_fused, m.beam_search_device

    def fused(files, vocabulary):
        calls.append(len(files))
        return orig(files, vocabulary)

    def device(files, vocabulary):
        fallbacks.append(len(files))
        return orig_dev(files, vocabulary)
    m.beam_search_fused = fused
    m.beam_search_device = device
    scores = m.eval(coco, data, vocab)
    assert set(scores) >= {'Bleu_1', 'Bleu_4', 'CIDEr'}
    assert calls and all(n == 2 for n in calls)
    assert not fallbacks
