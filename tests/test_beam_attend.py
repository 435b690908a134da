"""In-loop 1-layer attention of the fused beam decoder, CPU side: the
PyTorch twin of beam_attend against the model's own attend, the engine's
in-loop and 1-layer-decode structure end to end, and the trace."""

import pytest
import torch

from sat_amd.ops import functional as F

from _beam_refs import tiny_beam_model


# ---- 1. F.beam_attend against Decoder.attend ----

def test_beam_attend_twin_matches_model_attend():
    m, _vocab = tiny_beam_model(seed=3, num_attend_layers=1)
    model = m.model.eval()
    dec = model.decoder
    B, W = 2, 3
    L, D = model.num_ctx, model.dim_ctx
    E, H = m.config.dim_embedding, m.config.num_lstm_units
    g = torch.Generator().manual_seed(5)
    ctx = torch.randn(B, L, D, generator=g).abs()
    xh = torch.randn(B * W, D + E + H, generator=g)
    xh0 = xh.clone()
    h = xh[:, D + E:].clone()
    wa, wb = dec.att_fc_a.weight.detach(), dec.att_fc_b.weight.detach()
    assert wa.shape == (1, D) and wb.shape == (L, H)
    l1 = ctx.matmul(wa.reshape(-1))
    pool = torch.zeros(B * W, D)
    alpha = torch.zeros(B * W, L)
    F.beam_attend(ctx, l1, wb, xh, pool, alpha)

    ctx_rep = ctx.repeat_interleave(W, dim=0)
    with torch.no_grad():
        a_ref, p_ref = dec.attend(ctx_rep, ctx_rep.reshape(-1, D), h)
    torch.testing.assert_close(alpha, a_ref, rtol=1e-5, atol=0)
    torch.testing.assert_close(pool, p_ref, rtol=1e-5, atol=0)
    assert torch.equal(xh[:, :D], pool)
    assert torch.equal(xh[:, D:], xh0[:, D:])
    # an empty alpha is not written, the rest is the same
    xh2, pool2 = xh0.clone(), torch.zeros(B * W, D)
    F.beam_attend(ctx, l1, wb, xh2, pool2, torch.empty(0))
    assert torch.equal(pool2, pool) and torch.equal(xh2, xh)


# ---- 2. the engine end to end through the twins ----

def _caps(res):
    return [[(list(map(int, c.sentence)), c.score) for c in caps]
            for caps in res]


def _bias_period(m, period, bias):
    dec = m.model.decoder
    fc = dec.dec_fc if m.config.num_decode_layers == 1 else dec.dec_fc_2
    with torch.no_grad():
        fc.bias[period] += bias


# seed 3 for every architecture: the device and host paths agree with each
# other (sentences equal, scores within 1e-5) on all 8 images for each of
# the six (architecture, bias) cases, which the test itself asserts; a
# bias of 1.0 completes captions and 0.0 completes none, also asserted
@pytest.mark.parametrize('period_bias', [0.0, 1.0])
@pytest.mark.parametrize('attend,decode', [(1, 2), (1, 1), (2, 1)])
def test_engine_twin_matches_device_and_host(attend, decode, period_bias):
    from sat_amd.beam import FusedBeamDecoder
    m, vocab = tiny_beam_model(seed=3, num_attend_layers=attend,
                               num_decode_layers=decode)
    period = vocab.words.index('.')
    if period_bias:
        _bias_period(m, period, period_bias)
    files = ['synthetic://%d' % i for i in range(8)]
    m.model.eval()
    with torch.no_grad():
        contexts = m.model.compute_contexts(m._load_batch(files))
    eng = FusedBeamDecoder(m.model)
    assert eng.mode(False, torch.float32, 3) == (None if attend == 1
                                                 else 'twin')
    fused = _caps(eng.search(contexts, period, 3, mode='twin'))
    dev = _caps(m.beam_search_device(files, vocab))
    host = _caps(m.beam_search_host(files, vocab))
    assert len(fused) == len(dev) == len(host) == 8

    completed = 0
    for k in range(8):
        for other in (dev[k], host[k]):
            assert len(fused[k]) == len(other), (k, fused[k], other)
            for (s1, p1), (s2, p2) in zip(fused[k], other):
                assert s1 == s2, (k, s1, s2)
                assert abs(p1 - p2) <= 1e-5 * abs(p2), (k, p1, p2)
        completed += bool(fused[k][0][0]) and fused[k][0][0][-1] == period
    if period_bias:
        assert completed >= 1
    else:
        assert completed == 0

    if attend == 2:
        # 1-layer decode alone is offered on the CPU: the front door's
        # fused entry runs the engine, not the fallback
        assert m._fused_beam_mode() == 'twin'
        calls = []
        orig = m.beam_search_device
        m.beam_search_device = lambda *a: calls.append(1) or orig(*a)
        assert _caps(m.beam_search_fused(files, vocab)) == fused
        assert not calls
    else:
        assert m._fused_beam_mode() is None


def test_search_mode_argument_is_checked():
    from sat_amd.beam import FusedBeamDecoder
    m, _vocab = tiny_beam_model(seed=3, num_attend_layers=1)
    contexts = torch.rand(1, m.model.num_ctx, m.model.dim_ctx)
    eng = FusedBeamDecoder(m.model)
    with pytest.raises(ValueError):
        eng.search(contexts, 5, 3)              # mode() is None on the CPU
    with pytest.raises(ValueError):
        eng.search(contexts, 5, 3, mode='eager')


# ---- 3. the trace of the in-loop form ----

def test_trace_carries_state_dependent_alpha():
    from sat_amd.beam import FusedBeamDecoder
    m, vocab = tiny_beam_model(seed=3, num_attend_layers=1)
    B, W = 2, 3
    L, D = m.model.num_ctx, m.model.dim_ctx
    g = torch.Generator().manual_seed(7)
    contexts = torch.randn(B, L, D, generator=g).abs()
    T = m.config.max_caption_length
    res, trace = FusedBeamDecoder(m.model).search(
        contexts, vocab.words.index('.'), W, return_trace=True,
        mode='twin')
    assert len(res) == B and len(trace) == T
    for rec in trace:
        assert {'last_word', 'memory', 'output', 'scores_in', 'top_p',
                'top_w', 'parent', 'word', 'score', 'alpha'} <= set(rec)
        a = rec['alpha']
        assert a.shape == (B * W, L) and a.dtype == torch.float32
        torch.testing.assert_close(a.sum(dim=1), torch.ones(B * W),
                                   rtol=1e-5, atol=0)
    # not hoisted: the weights follow the LSTM state from step to step
    assert not torch.equal(trace[0]['alpha'], trace[1]['alpha'])
    assert not torch.equal(trace[1]['alpha'], trace[2]['alpha'])
    # the 2-layer form keeps its keys
    m2, _ = tiny_beam_model(seed=3)
    _res, trace2 = FusedBeamDecoder(m2.model).search(
        contexts, 5, W, return_trace=True)
    assert 'alpha' not in trace2[0]
