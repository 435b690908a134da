"""Shared references of the fused-beam tests (CPU and GPU files)."""

import torch


def rand_bf16_logits(R, V, K, seed, scale=3.0):
    """[R,V] fp32 holding bf16-rounded random logits.  Row 0 is all-equal;
    row 1 has a tie planted across the top-K boundary (its K-th and
    (K+1)-th largest values are equal)."""
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(R, V, generator=g) * scale).bfloat16().float()
    x[0] = 0.5
    if V > K:
        order = x[1].sort(descending=True, stable=True)[1]
        x[1, order[K]] = x[1, order[K - 1]]
    return x


def stable_topk_ref(logits, K):
    """fp64 softmax of the given logits at the K stably-sorted best
    indices (descending, ties by ascending index)."""
    x = logits.double()
    idx = torch.sort(logits.float(), dim=1, descending=True,
                     stable=True)[1][:, :K]
    return torch.softmax(x, dim=1).gather(1, idx), idx


def fresh_state(B, W, T, device='cpu'):
    """(scores, seqs, lens, c_scores, c_seqs, c_lens) at step 0."""
    scores = torch.zeros(B, W, dtype=torch.float64, device=device)
    scores[:, 0] = 1.0
    z = dict(dtype=torch.int64, device=device)
    return (scores, torch.zeros(B, W, T, **z), torch.zeros(B, W, **z),
            torch.zeros(B, W, dtype=torch.float64, device=device),
            torch.zeros(B, W, T, **z), torch.zeros(B, W, **z))


def beam_inputs(B, W, K, V, period, g):
    """top_p [B*W,K] fp32, pairwise distinct and positive; top_w random
    words with the period planted in about 30 % of the entries."""
    n = B * W * K
    # a jittered permutation of n levels: distinct by construction
    level = torch.randperm(n, generator=g).double() \
        + torch.rand(n, generator=g).double() * 0.5
    top_p = (0.05 + 0.9 * level / n).float().reshape(B * W, K)
    assert top_p.unique().numel() == n
    top_w = torch.randint(0, V - 1, (B * W, K), generator=g)
    top_w = top_w + (top_w >= period).long()          # never the period
    plant = torch.rand(B * W, K, generator=g) < 0.3
    return top_p, torch.where(plant, torch.full_like(top_w, period), top_w)


def ref_beam_step(state, top_p, top_w, period):
    """The torch bookkeeping lines of BaseModel.beam_search_device between
    two decode_step calls, with stable sorts in place of topk.
    -> (new state, selected parents [B,W], selected words [B,W])."""
    scores, seqs, lens, c_scores, c_seqs, c_lens = state
    B, W = scores.shape
    T = seqs.shape[2]
    K = top_p.shape[1]
    dev = scores.device
    NEG = float('-inf')

    def topk(x, k):
        s, i = torch.sort(x, dim=1, descending=True, stable=True)
        return s[:, :k], i[:, :k]

    cand = (scores.unsqueeze(2)
            * top_p.double().reshape(B, W, -1)).reshape(B, -1)
    cand_w = top_w.reshape(B, -1)
    is_period = cand_w == period
    comp_cand = torch.where(is_period, cand, torch.zeros_like(cand))
    merged_s = torch.cat([c_scores, comp_cand], dim=1)
    parent = torch.arange(W * K, device=dev).reshape(1, -1) \
        .expand(B, -1) // K
    new_seq = seqs.gather(
        1, parent.unsqueeze(2).expand(B, W * K, T)).clone()
    new_len = lens.gather(1, parent)
    step_seq = new_seq.scatter(
        2, new_len.clamp(max=T - 1).reshape(B, W * K, 1),
        cand_w.reshape(B, W * K, 1))
    step_len = (new_len + 1).clamp(max=T)
    merged_seq = torch.cat([c_seqs, step_seq], dim=1)
    merged_len = torch.cat([c_lens, step_len], dim=1)
    keep_s, keep_i = topk(merged_s, W)
    c_scores = keep_s
    c_seqs = merged_seq.gather(1, keep_i.unsqueeze(2).expand(B, W, T))
    c_lens = merged_len.gather(1, keep_i)

    part = torch.where(is_period, torch.full_like(cand, NEG), cand)
    part = torch.nan_to_num(part, nan=NEG, neginf=NEG)
    sel_s, sel_i = topk(part, W)
    scores = sel_s.clamp_min(0.0)
    sel_parent = sel_i // K
    seqs = step_seq.gather(1, sel_i.unsqueeze(2).expand(B, W, T))
    lens = step_len.gather(1, sel_i)
    last_word = cand_w.gather(1, sel_i)
    return ((scores, seqs, lens, c_scores, c_seqs, c_lens), sel_parent,
            last_word)


def tiny_beam_model(seed=3, **overrides):
    """BaseModel + vocabulary of test_device_beam_matches_host_beam:
    V=40, dims 16, T=8, beam 3, CPU, synthetic images."""
    from config import Config
    from sat_amd.data.vocabulary import Vocabulary
    from sat_amd.models.base_model import BaseModel

    cfg = Config()
    cfg.phase = 'eval'
    cfg.train_cnn = False
    cfg.synthetic_data = True
    cfg.device = 'cpu'
    cfg.beam_size = 3
    cfg.vocabulary_size = 40
    cfg.dim_embedding = 16
    cfg.num_lstm_units = 16
    cfg.dim_initalize_layer = 16
    cfg.dim_attend_layer = 16
    cfg.dim_decode_layer = 16
    cfg.max_caption_length = 8
    for k, v in overrides.items():
        setattr(cfg, k, v)

    vocab = Vocabulary(40)
    vocab.build(['a man rides a horse down the street .',
                 'a dog sits on the beach sand .',
                 'the cat sleeps near a window ledge .'])
    torch.manual_seed(seed)
    return BaseModel(cfg), vocab
