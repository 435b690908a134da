"""Fused beam-search decoder, CPU side: the PyTorch twins of the two
kernels, the engine's structure end to end, and the dispatch."""

import pytest
import torch

from sat_amd.ops import functional as F

from _beam_refs import (beam_inputs, fresh_state, rand_bf16_logits,
                        ref_beam_step, stable_topk_ref, tiny_beam_model)


# ---- 1. F.softmax_topk against the stable-sort reference ----

@pytest.mark.parametrize('R,V,K', [(4, 40, 4), (6, 1000, 4), (5, 1001, 3),
                                   (3, 16, 9)])
def test_softmax_topk_twin(R, V, K):
    logits = rand_bf16_logits(R, V, K, seed=R * 7 + K)
    p, idx = F.softmax_topk(logits, K)
    p_ref, idx_ref = stable_topk_ref(logits, K)
    assert p.dtype == torch.float32 and idx.dtype == torch.int64
    assert torch.equal(idx, idx_ref)
    # row 0 is all-equal: indices 0..K-1; row 1 has a planted tie across
    # the K boundary, whose lower index must win
    assert idx[0].tolist() == list(range(K))
    assert logits[1, idx[1, K - 1]] == logits[1].float().sort(
        descending=True)[0][K]
    torch.testing.assert_close(p.double(), p_ref, rtol=1e-5, atol=0)


# ---- 2. end to end on the CPU ----

def _caps(res):
    return [[(list(map(int, c.sentence)), c.score) for c in caps]
            for caps in res]


@pytest.mark.parametrize('period_bias', [0.0, 1.0])
def test_fused_beam_matches_device_and_host_cpu(period_bias):
    m, vocab = tiny_beam_model(seed=3)
    if period_bias:
        with torch.no_grad():
            m.model.decoder.dec_fc_2.bias[vocab.words.index('.')] += \
                period_bias
    files = ['synthetic://%d' % i for i in range(8)]
    assert m._fused_beam_mode() == 'twin'
    fused = _caps(m.beam_search_fused(files, vocab))
    dev = _caps(m.beam_search_device(files, vocab))
    host = _caps(m.beam_search_host(files, vocab))
    assert len(fused) == len(dev) == len(host) == 8

    period = vocab.words.index('.')
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


# ---- 3. F.beam_advance against a transcription of beam_search_device ----

@pytest.mark.parametrize('B,W,K,T', [(1, 1, 2, 4), (2, 3, 4, 8),
                                     (5, 8, 9, 20)])
def test_beam_advance_twin(B, W, K, T):
    H = E = D = 8
    V, period = 50, 7
    g = torch.Generator().manual_seed(B * 100 + W)
    table = torch.randn(V, E, generator=g)
    ref = fresh_state(B, W, T)
    cur = fresh_state(B, W, T)
    nxt = fresh_state(B, W, T)
    for t in range(T):
        top_p, top_w = beam_inputs(B, W, K, V, period, g)
        mem_new = torch.randn(B * W, H, generator=g)
        h_new = torch.randn(B * W, H, generator=g)
        cand = (ref[0].unsqueeze(2)
                * top_p.double().reshape(B, W, K)).reshape(B, -1)
        for b in range(B):
            pos = cand[b][cand[b] > 0]
            assert pos.unique().numel() == pos.numel()
        ref, r_parent, r_word = ref_beam_step(ref, top_p, top_w, period)

        mem_next = torch.zeros(B * W, H)
        xh_next = torch.zeros(B * W, D + E + H)
        exp_next = torch.zeros(B * W, H + D + E)
        last_word = torch.zeros(B * W, dtype=torch.int64)
        parent = torch.zeros(B, W, dtype=torch.int64)
        F.beam_advance(cur, nxt, top_p, top_w, period, mem_new, h_new,
                       table, mem_next, xh_next, exp_next, last_word,
                       parent)
        assert torch.equal(nxt[0], ref[0])            # fp64, bitwise
        live = ref[0] > 0
        assert torch.equal(parent[live], r_parent[live])
        assert torch.equal(last_word.reshape(B, W)[live], r_word[live])
        assert torch.equal(nxt[1][live], ref[1][live])
        assert torch.equal(nxt[2][live], ref[2][live])
        assert torch.equal(nxt[3], ref[3])
        done = ref[3] > 0
        assert torch.equal(nxt[4][done], ref[4][done])
        assert torch.equal(nxt[5][done], ref[5][done])
        # gathers
        rows = (parent + torch.arange(B).unsqueeze(1) * W).reshape(-1)
        assert torch.equal(mem_next, mem_new[rows])
        assert torch.equal(xh_next[:, D + E:], h_new[rows])
        assert torch.equal(xh_next[:, D:D + E], table[last_word])
        assert torch.equal(exp_next[:, H + D:], table[last_word])
        assert not xh_next[:, :D].any() and not exp_next[:, :H + D].any()
        cur, nxt = nxt, cur
    if W > 1:       # the inputs exercised both sets (W = 1 may just die)
        assert (ref[3] > 0).any() and (ref[0] > 0).any()


# ---- 4. dispatch ----

def _record(m, monkeypatch):
    calls = []
    for name in ('beam_search_device', 'beam_search_fused'):
        orig = getattr(m, name)

        def wrapped(files, vocab, _o=orig, _n=name):
            calls.append(_n)
            return _o(files, vocab)
        monkeypatch.setattr(m, name, wrapped)
    return calls


def test_knob_off_uses_device_path(monkeypatch):
    from config import Config
    assert Config().use_fused_beam is False
    m, vocab = tiny_beam_model(seed=3)
    calls = _record(m, monkeypatch)
    res = m.beam_search(['synthetic://0'], vocab)
    assert calls == ['beam_search_device'] and len(res) == 1


@pytest.mark.parametrize('case', ['cpu', 'one_attend_layer', 'beam9'])
def test_knob_on_but_ineligible_falls_back(case, monkeypatch):
    over = {'use_fused_beam': True}
    if case == 'one_attend_layer':
        over['num_attend_layers'] = 1
    if case == 'beam9':
        over['beam_size'] = 9
    m, vocab = tiny_beam_model(seed=3, **over)
    assert m._fused_beam_mode() == ('twin' if case == 'cpu' else None)
    calls = _record(m, monkeypatch)
    files = ['synthetic://0', 'synthetic://1']
    res = m.beam_search(files, vocab)
    assert calls == ['beam_search_device']
    assert len(res) == 2 and all(len(c) >= 1 for c in res)
    if case != 'cpu':
        # asked for directly, the fused entry point falls back as well
        res = m.beam_search_fused(files, vocab)
        assert calls[-1] == 'beam_search_device' and len(res) == 2


def test_cli_flags_reach_config():
    import main
    args = main.build_parser().parse_args(
        ['--phase', 'eval', '--fused_beam', '--eval_batch_size', '4'])
    cfg = main.build_config(args)
    assert cfg.use_fused_beam is True and cfg.batch_size == 4
    cfg = main.build_config(main.build_parser().parse_args(
        ['--phase', 'eval']))
    assert cfg.use_fused_beam is False and cfg.batch_size == 1
