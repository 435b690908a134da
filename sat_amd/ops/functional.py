"""Reference (plain PyTorch) implementations of the op layer.

These are the CPU path and the numerics ground truth for the HIP kernels.
Semantics mirror the TF ops the reference launches:

  * dense           — tf.layers.dense semantics; kernels are stored [out,in]
                      (torch Linear layout) so the GPU MFMA kernel reads a
                      [N,K]-contiguous B operand with no transpose
  * lstm_cell       — tf.nn.rnn_cell.LSTMCell (gate order i,j,f,o; forget
                      bias added pre-sigmoid; no peepholes)
  * attention_pool  — softmax over locations + Σ_l α_l·ctx_l
                      (reference model.py:435, :263-264)
  * embedding       — tf.nn.embedding_lookup (model.py:273)
  * masked_softmax_ce — tf.nn.sparse_softmax_cross_entropy_with_logits ×
                      mask (model.py:294-297)
  * softmax_topk / beam_advance — the beam-search inference pair
                      (sat_amd/beam.py); no reference analog
  * resize_normalize_u8 — Pillow's 8-bit bilinear resize in integers, mean
                      subtraction and the cast (sat_amd/data/pipeline.py)
"""

import torch
import torch.nn.functional as tF


def dense(x, weight, bias=None, activation=None):
    """act(x @ weight.T + bias); weight: [out, in]."""
    y = x.matmul(weight.t())
    if bias is not None:
        y = y + bias
    if activation == 'tanh':
        y = torch.tanh(y)
    elif activation == 'relu':
        y = torch.relu(y)
    elif activation not in (None, 'none'):
        raise ValueError('unknown activation %r' % (activation,))
    return y


def lstm_cell(x, h, c, weight, bias, forget_bias=1.0):
    """TF LSTMCell step.

    x: [B, I], h/c: [B, H], weight: [4H, I+H] with gate order (i, j, f, o),
    bias: [4H].  Returns (new_h, new_c).
    """
    gates = torch.cat([x, h], dim=1).matmul(weight.t()) + bias
    i, j, f, o = gates.chunk(4, dim=1)
    new_c = c * torch.sigmoid(f + forget_bias) + \
        torch.sigmoid(i) * torch.tanh(j)
    new_h = torch.tanh(new_c) * torch.sigmoid(o)
    return new_h, new_c


def attention_pool(contexts, logits):
    """contexts: [B, L, D], logits: [B, L] -> (alpha [B,L], context [B,D])."""
    alpha = torch.softmax(logits, dim=1)
    context = (contexts * alpha.unsqueeze(2)).sum(dim=1)
    return alpha, context


def attention_tail(t1, t2, v, contexts, p, training):
    """Attention tail (reference model.py:425-435 + :263-264):
    t = dropout(t1 + tiled t2); logits = t @ v; alpha = softmax over L;
    context = Σ_l α_l·ctx_l.  Returns (alpha [B,L], context [B,D])."""
    B, L = contexts.shape[0], contexts.shape[1]
    t = t1 + t2.repeat_interleave(L, dim=0)
    t = dropout(t, p, training)
    logits = t.matmul(v).reshape(B, L)
    return attention_pool(contexts, logits)


def embedding(ids, table):
    return table[ids]


def masked_softmax_ce(logits, labels, mask):
    """logits: [B, V], labels: [B] int64, mask: [B] -> masked CE [B]."""
    ce = tF.cross_entropy(logits.float(), labels, reduction='none')
    return ce * mask


def dropout(x, rate, training):
    if not training or rate <= 0.0:
        return x
    return tF.dropout(x, p=rate, training=True)


# ---- beam-search inference (twins of csrc/beam.hip) ----

def softmax_topk(logits, k):
    """The k largest softmax probabilities of each row -> (p [R,k] fp32,
    idx [R,k] int64).  Ranked on the logits, descending; equal logits by
    ascending index (torch.topk promises no order among ties, and bf16
    logits tie often)."""
    x = logits.float()
    v, idx = torch.sort(x, dim=1, descending=True, stable=True)
    v, idx = v[:, :k], idx[:, :k]
    mx = v[:, :1]
    denom = torch.exp(x - mx).sum(dim=1, keepdim=True)
    return torch.exp(v - mx) / denom, idx


def beam_advance(state_in, state_out, top_p, top_w, period, mem_new, h_new,
                 table, mem_next, xh_next, exp_next, last_word, parent):
    """One beam-search bookkeeping step (semantics of
    BaseModel.beam_search_device between two decode_step calls) plus the
    next step's inputs.

    state_* = (scores [B,W] fp64, seqs [B,W,T], lens [B,W], c_scores,
    c_seqs, c_lens); state_out and every tensor after `table` are written
    in place.  Candidate parent*K + k scores scores[parent] * top_p in
    fp64; period candidates merge into the completed set (best W of
    [completed..., candidates...]), the best W others become the live
    beams (dead slots: score 0).  Every selection is by score descending,
    then position ascending.  The selected parents' rows of mem_new / h_new
    go to mem_next and the state columns of xh_next [B*W, D+E+H]; the
    selected words' embeddings to the E columns of xh_next and (when given)
    of exp_next [B*W, H+D+E]; the words to last_word, the parents to
    `parent`."""
    scores, seqs, lens, c_scores, c_seqs, c_lens = state_in
    B, W = scores.shape
    T = seqs.shape[2]
    K = top_p.shape[1]
    H, E = mem_new.shape[1], table.shape[1]
    D = xh_next.shape[1] - E - H
    dev = scores.device
    neg = float('-inf')

    cand = (scores.unsqueeze(2)
            * top_p.double().reshape(B, W, K)).reshape(B, W * K)
    cand = torch.nan_to_num(cand, nan=0.0)
    cand_w = top_w.reshape(B, W * K)
    is_period = cand_w == period
    par = (torch.arange(W * K, device=dev) // K).reshape(1, -1) \
        .expand(B, -1)
    par_len = lens.gather(1, par)
    step_seq = seqs.gather(1, par.unsqueeze(2).expand(B, W * K, T)) \
        .scatter(2, par_len.clamp(max=T - 1).unsqueeze(2),
                 cand_w.unsqueeze(2))
    step_len = (par_len + 1).clamp(max=T)

    # completed: best W of [completed..., period candidates...]
    merged_s = torch.cat(
        [c_scores, torch.where(is_period, cand, torch.zeros_like(cand))],
        dim=1)
    keep = torch.sort(merged_s, dim=1, descending=True,
                      stable=True)[1][:, :W]
    merged_seq = torch.cat([c_seqs, step_seq], dim=1)
    merged_len = torch.cat([c_lens, step_len], dim=1)
    new_c = (merged_s.gather(1, keep),
             merged_seq.gather(1, keep.unsqueeze(2).expand(B, W, T)),
             merged_len.gather(1, keep))

    # live: best W non-period candidates
    part = torch.where(is_period, torch.full_like(cand, neg), cand)
    sel = torch.sort(part, dim=1, descending=True, stable=True)[1][:, :W]
    sel_parent = sel // K
    words = cand_w.gather(1, sel)
    new_live = (part.gather(1, sel).clamp_min(0.0),
                step_seq.gather(1, sel.unsqueeze(2).expand(B, W, T)),
                step_len.gather(1, sel))

    for dst, src in zip(state_out, new_live + new_c):
        dst.copy_(src)
    rows = (sel_parent
            + torch.arange(B, device=dev).unsqueeze(1) * W).reshape(-1)
    mem_next.copy_(mem_new[rows])
    xh_next[:, D + E:] = h_new[rows]
    emb = table[words.reshape(-1).clamp(0, table.shape[0] - 1)]
    xh_next[:, D:D + E] = emb
    if exp_next is not None and exp_next.numel() > 0:
        exp_next[:, H + D:] = emb
    last_word.copy_(words.reshape(-1))
    parent.copy_(sel_parent.reshape(parent.shape))


def beam_attend(contexts, l1, wb, xh, pool, alpha=None):
    """1-layer attention (Decoder.attend with num_attend_layers == 1) of
    one beam-search step, for all beams at once.  Row n = b*W + w is beam
    w of image b; W = xh.shape[0] // B.

    contexts [B,L,D] (not repeated per beam); l1 [B,L] fp32, the
    per-image constant contexts · att_fc_a.weight; wb [L,H] =
    att_fc_b.weight; xh [B*W, D+E+H], the step's LSTM-input rows, whose
    last H columns hold h.

        logit[n,l]  = l1[b,l] + sum_k h[n,k] * wb[l,k]
        alpha[n,:]  = softmax over l of logit[n,:]
        pooled[n,d] = sum_l alpha[n,l] * contexts[b,l,d]

    all in fp32, pooled rounded once to pool's dtype.  Written in place:
    pool [B*W,D] and xh[:, :D] receive the same values; alpha [B*W,L]
    fp32 receives the weights unless it is None or empty.  The other
    columns of xh are read (h) or left alone."""
    B, L, D = contexts.shape
    W = xh.shape[0] // B
    H = wb.shape[1]
    h = xh[:, xh.shape[1] - H:].float()
    logits = l1.float().repeat_interleave(W, dim=0) \
        + h.matmul(wb.float().t())
    a, pooled = attention_pool(
        contexts.float().repeat_interleave(W, dim=0), logits)
    pool.copy_(pooled)
    xh[:, :D] = pool
    if alpha is not None and alpha.numel() > 0:
        alpha.copy_(a)


def _resample_u8(src, table, out_size, ksize, dim):
    """One pass of Pillow's 8-bit resample along `dim` of src [H,W,3]
    uint8.  `table` is an axis table of ImagePrep: first source index and
    tap count per output, then out_size x ksize Q22 coefficients (zero
    past the tap count)."""
    first = table[:out_size].long()
    coef = table[2 * out_size:].reshape(out_size, ksize)
    last = src.shape[dim] - 1
    shape = [1, 1, 1]
    shape[dim] = out_size
    acc = None
    for k in range(ksize):
        px = src.index_select(dim, (first + k).clamp(max=last))
        term = px.to(torch.int32) * coef[:, k].reshape(shape)
        acc = term if acc is None else acc + term
    return ((acc + (1 << 21)) >> 22).clamp(0, 255).to(torch.uint8)


def resize_normalize_u8(packed, desc, tables, mean, out_h, out_w,
                        dtype=torch.float32):
    """N packed uint8 HWC images -> [N,3,out_h,out_w] channels_last:
    Pillow's resize(..., BILINEAR) bit for bit (horizontal pass, then
    vertical, each rounded to 8 bits), then float(u8) - mean[c] in fp32,
    then the cast to `dtype`.

    packed: 1-D uint8; desc: [N,8] int64 rows (byte offset, H, W,
    horizontal table offset, its taps, vertical table offset, its taps,
    0); tables: 1-D int32 holding the axis tables (ImagePrep builds
    them); mean: [3] fp32."""
    N = desc.shape[0]
    out = torch.empty((N, 3, out_h, out_w), dtype=dtype,
                      device=packed.device,
                      memory_format=torch.channels_last)
    nhwc = out.permute(0, 2, 3, 1)
    mean = mean.to(torch.float32)
    for n, (off, H, W, ht, hk, vt, vk, _) in enumerate(desc.tolist()):
        src = packed[off:off + H * W * 3].reshape(H, W, 3)
        htab = tables[ht:ht + out_w * (2 + hk)]
        vtab = tables[vt:vt + out_h * (2 + vk)]
        px = _resample_u8(src, htab, out_w, hk, 1)
        px = _resample_u8(px, vtab, out_h, vk, 0)
        nhwc[n] = (px.to(torch.float32) - mean).to(dtype)
    return out
