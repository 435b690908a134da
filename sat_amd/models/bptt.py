"""Hand-written BPTT for the attention-LSTM decoder (GPU bf16 path).

The reference gets its training step as one static TF graph executed by the
C++ runtime; autograd-per-op in a Python loop pays ~1500
kernel dispatches and ~300 gradient-accumulation adds per step instead.
This module runs the whole T-step decoder as TWO torch.autograd.Functions:

  * DecoderCoreBPTT — the recurrent part (attention MLP + LSTM + expand),
    forward as direct _C kernel calls over the T teacher-forced steps,
    backward as the fused reverse-time loop with hand-carried recurrent
    gradients;
  * DecodeHeadBPTT — the decode MLP + cross-entropy, batched over
    [T·B, ·]: two chip-filling MFMA GEMMs + slab dropout + one fused CE
    instead of 3 skinny launches × T steps.

The split is load-bearing for data-parallel overlap: the head's backward
runs FIRST and takes the fp32 leaf weights directly, so its weight
gradients (decode fc_1/fc_2 — 6.7M of the ~14M trainable params)
accumulate and fire the DDP bucket hooks while the recurrent reverse loop
is still executing; their RCCL all-reduce then overlaps the bulk of
backward (VERDICT r01 Weak #2 fix).

Numerics are identical to the per-op path (reference model.py:259-334):
same gate order, same dropout sites and counter-hash masks (slab salt
t*16+k matches the per-step calls bit-for-bit), same doubly-stochastic
attention-loss wiring through masked alphas.

Supported shape: the reference default architecture (2-layer attend MLP,
2-layer decode MLP).  Other configs use the per-op autograd loop.
"""

import torch

from sat_amd import _C

ACT_NONE, ACT_TANH, ACT_RELU = 0, 1, 2

# The B <= 128 step chain with its epilogue / elementwise launches folded
# into their producers and consumers (docs/KERNELS.md).  False runs the
# same steps launch by launch; tests compare the two.
CHAIN_FUSION = True


def _drop(x, seed, p, salt):
    if p <= 0.0:
        return x
    return _C.hash_dropout(x, seed, p, salt)


class DecoderCoreBPTT(torch.autograd.Function):
    """Recurrent core: T steps of attention + LSTM + expand.

    Outputs EXPD [T·B, H+D+E] (the concat[output, context, embedding]
    rows the decode MLP consumes, step-major) and the mask-weighted
    attention accumulation [B, L] for the doubly-stochastic loss.
    """

    @staticmethod
    def forward(ctx_ag, contexts, init_memory, init_output, sentences,
                masks, emb, w1a, b1a, w1b, b1b, v, wl, bl, seed,
                p_fc, p_lstm, train_cnn, shadows=None):
        # shadow mode: the weight INPUTS are the fp32 leaves (grads
        # return straight to AccumulateGrad) while the COMPUTE tensors
        # are the Adam-refreshed bf16 shadows — no per-forward casts
        # and no cast-node backwards.
        if shadows is not None:
            emb_c = shadows['emb']
            w1a_c, b1a_c = shadows['w1a'], shadows['b1a']
            w1b_c, b1b_c = shadows['w1b'], shadows['b1b']
            v_c = shadows['v'].reshape(-1)
            wl_c, bl_c = shadows['wl'], shadows['bl']
        else:
            emb_c, w1a_c, b1a_c = emb, w1a, b1a
            w1b_c, b1b_c, v_c = w1b, b1b, v
            wl_c, bl_c = wl, bl
        B, L, D = contexts.shape
        T = sentences.shape[1]
        A = w1a_c.shape[0]
        H = init_memory.shape[1]
        E = emb_c.shape[1]
        I = D + E
        dev = contexts.device

        ctx_flat = contexts.reshape(B * L, D)
        # all T context-dropout slabs in one kernel (salt t*16+0); the
        # buffer also feeds the batched dW_1a GEMM in backward.  fc_1a
        # (the attention context projection) does not depend on the
        # recurrence, so ALL T steps run as ONE batched MFMA GEMM here
        # instead of 20 per-step launches.
        if p_fc > 0.0:
            CDROP = _C.hash_dropout_steps(ctx_flat, seed, p_fc, 0, 16, T)
            T1 = _C.dense_fwd(CDROP.reshape(T * B * L, D), w1a_c,
                              b1a_c, 1)
        else:
            CDROP = None
            T1 = _C.dense_fwd(ctx_flat, w1a_c, b1a_c, 1)  # shared

        # forward-side batched buffers (consumed by backward's batched dW)
        XH = torch.empty(T * B, I + H, dtype=torch.bfloat16, device=dev)
        EXPD = torch.empty(T * B, H + D + E, dtype=torch.bfloat16,
                           device=dev)
        ODROP = torch.empty(T * B, H, dtype=torch.bfloat16, device=dev)

        t1s, t2s, tdrops, alphas = [], [], [], []
        gates_l, cprev_l = [], []

        labels_cat = sentences.t().reshape(-1)          # [T·B] step-major

        memory = init_memory
        state_h = init_output
        last_word = torch.zeros(B, dtype=torch.int64, device=dev)
        empty_b = _EMPTY_B(dev)
        fuse_small = (B <= 128 and (I + H) % 32 == 0
                      and (H + D + E) % 32 == 0)
        chain = fuse_small and CHAIN_FUSION

        # attend input for step 0 (later steps' come fused out of
        # expand_fuse at step t-1)
        _C.hash_dropout_out(init_output, seed, p_fc, 1, ODROP[0:B])
        if chain:
            # embedding + state columns of XH[0]; inside the loop step t's
            # gates epilogue writes them for step t+1, and the pooled
            # columns come straight out of the attention pool
            _C.lstm_in_tail(emb_c, last_word, state_h, seed, p_lstm, 3,
                            XH[0:B], D)

        for t in range(T):
            s = t * 16
            sl = slice(t * B, (t + 1) * B)

            t1 = T1.reshape(-1, A)[t * B * L:(t + 1) * B * L] \
                if CDROP is not None else T1
            t2 = _C.dense_fwd(ODROP[sl], w1b_c, b1b_c, ACT_TANH)
            tdrop, att_logits = _C.attn_scores_fused(
                t1, t2, v_c, seed, p_fc, s + 2, L)
            if chain:
                alpha, pooled = _C.attn_pool_fwd_xh(
                    contexts, att_logits, seed, p_lstm, s + 3, XH[sl], I)
            else:
                alpha, pooled = _C.attn_pool_fwd(contexts, att_logits)
                _C.lstm_in_fuse(pooled, emb_c, last_word, state_h, seed,
                                p_lstm, s + 3, XH[sl])
            od_next = ODROP[(t + 1) * B:(t + 2) * B] if t + 1 < T \
                else empty_b
            if chain:
                xh_next = XH[(t + 1) * B:(t + 2) * B] if t + 1 < T \
                    else empty_b
                gates, c_new, sth_t = _C.dense_lstm_expand_xh_fwd(
                    XH[sl], wl_c, bl_c, memory, pooled, emb_c,
                    last_word, seed, EXPD[sl], od_next,
                    1.0, p_lstm, p_fc, s, labels_cat[sl], xh_next)
            elif fuse_small:
                # gates GEMM -> gate math + expand scatter in ONE
                # epilogue (h_raw / out_t never touch HBM)
                gates, c_new, sth_t = _C.dense_lstm_expand_fwd(
                    XH[sl], wl_c, bl_c, memory, pooled, emb_c,
                    last_word, seed, EXPD[sl], od_next,
                    1.0, p_lstm, p_fc, s)
            else:
                gates = _C.dense_fwd(XH[sl], wl_c, bl_c, ACT_NONE)
                h_raw, c_new = _C.lstm_pointwise_fwd(gates, memory, 1.0)
                out_t, sth_t = _C.expand_fuse(
                    h_raw, pooled, emb_c, last_word, seed, EXPD[sl],
                    od_next, p_lstm, p_fc, s)

            t1s.append(t1)
            t2s.append(t2)
            tdrops.append(tdrop)
            alphas.append(alpha)
            gates_l.append(gates)
            cprev_l.append(memory)

            memory = c_new
            state_h = sth_t
            last_word = labels_cat[sl]

        alpha_stack = torch.stack(alphas)                # [T,B,L]
        attn_acc = (alpha_stack
                    * masks.t().reshape(T, B, 1)).sum(dim=0)

        ctx_ag.save_for_backward(
            contexts, emb_c, w1a_c, b1a_c, w1b_c, b1b_c, v_c, wl_c,
            bl_c, seed, XH, ODROP, labels_cat, masks)
        ctx_ag.leaf_mode = shadows is not None
        ctx_ag.cdrop = CDROP
        ctx_ag.saved_lists = (t1s, t2s, tdrops, alphas, gates_l, cprev_l)
        ctx_ag.dims = (B, L, D, T, A, H, E, I)
        ctx_ag.p_fc = p_fc
        ctx_ag.p_lstm = p_lstm
        ctx_ag.train_cnn = train_cnn
        ctx_ag.chain = chain
        return EXPD, attn_acc

    @staticmethod
    def backward(ctx_ag, d_expd, d_attn):
        (contexts, emb, w1a, b1a, w1b, b1b, v, wl, bl, seed, XH,
         ODROP, labels_cat, masks) = ctx_ag.saved_tensors
        (t1s, t2s, tdrops, alphas, gates_l,
         cprev_l) = ctx_ag.saved_lists
        B, L, D, T, A, H, E, I = ctx_ag.dims
        p_fc = ctx_ag.p_fc
        p_lstm = ctx_ag.p_lstm
        dev = contexts.device
        need_dctx = ctx_ag.train_cnn and ctx_ag.needs_input_grad[0]

        ctx_flat = contexts.reshape(B * L, D)
        if not d_expd.is_contiguous():
            d_expd = d_expd.contiguous()

        # transposed weights for the per-step skinny GEMMs (x @ W forms)
        wl_t = wl.t().contiguous()
        w1b_t = w1b.t().contiguous()

        DG = torch.empty(T * B, 4 * H, dtype=torch.bfloat16, device=dev)
        DEMB = torch.empty(T * B, E, dtype=torch.bfloat16, device=dev)
        DPRE1B = torch.empty(T * B, A, dtype=torch.bfloat16, device=dev)
        DPRE1A = torch.empty(T * B * L, A, dtype=torch.bfloat16,
                             device=dev)
        CDROP = ctx_ag.cdrop

        dv_acc = torch.zeros_like(v, dtype=torch.float32)
        dctx_acc = torch.zeros_like(contexts) if need_dctx else None

        chain = ctx_ag.chain
        # one zeroed dt2 accumulator for all T steps (the scores kernel
        # atomically adds into its step's slice)
        DT2 = torch.zeros(T, B, A, dtype=torch.float32, device=dev) \
            if chain else None
        carry_slabs, carry_salt = None, 0

        d_out_carry = torch.zeros(B, H, dtype=torch.bfloat16, device=dev)
        d_sth_carry = torch.zeros(B, H, dtype=torch.bfloat16, device=dev)
        dc_carry = torch.zeros(B, H, dtype=torch.bfloat16, device=dev)

        for t in range(T - 1, -1, -1):
            s = t * 16
            sl = slice(t * B, (t + 1) * B)
            # dexp scatter + LSTM pointwise backward fused: dh_raw
            # stays in registers inside the one kernel
            if carry_slabs is not None:
                # d_out_carry still as the dodrop GEMM's split-K slabs:
                # their epilogue (sum, ODROP mask of the producing step,
                # bf16 rounding) runs inside this kernel
                dc_prev, dpool_dec, demb_dec = _C.dexp_lstm_bwd_slabs(
                    d_expd[sl], carry_slabs, carry_salt, d_sth_carry,
                    seed, gates_l[t], cprev_l[t], dc_carry, DG[sl],
                    p_fc, p_lstm, s, D, E, 1.0)
            else:
                dc_prev, dpool_dec, demb_dec = _C.dexp_lstm_bwd(
                    d_expd[sl], d_out_carry, d_sth_carry, seed,
                    gates_l[t], cprev_l[t], dc_carry, DG[sl],
                    p_fc, p_lstm, s, D, E, 1.0)
            dgates = DG[sl]
            if B <= 128:
                # dxh GEMM + the dx scatter in one epilogue
                dpooled, d_sth_carry = _C.dense_dx_fuse(
                    dgates, wl_t, dpool_dec, demb_dec, seed, DEMB[sl],
                    p_lstm, s + 3, D, E, H)
            else:
                dxh = _C.dense_fwd(dgates, wl_t, _EMPTY_B(dev),
                                   ACT_NONE)
                dpooled, d_sth_carry = _C.dx_fuse(
                    dxh, dpool_dec, demb_dec, seed, DEMB[sl], p_lstm,
                    s + 3, H)
            dc_carry = dc_prev

            dalpha_t = d_attn * masks[:, t].unsqueeze(1)
            dlog_att, dctx_t = _C.attn_pool_bwd(
                contexts, alphas[t], dalpha_t.contiguous(),
                dpooled, need_dctx)
            if need_dctx:
                dctx_acc += dctx_t
            sl_a = slice(t * B * L, (t + 1) * B * L)
            # dt1 tanh-backward fused into the scores kernel, written
            # straight into the DPRE1A slab (one launch + no dt1
            # round-trip instead of scores_bwd + act_bwd_out)
            if chain:
                _dt1, dt2f, _dv = _C.attn_scores_bwd_step(
                    tdrops[t], v, dlog_att, seed, p_fc, s + 2, L, dv_acc,
                    t1s[t], DPRE1A[sl_a], DT2[t])
            else:
                _dt1, dt2f, _dv = _C.attn_scores_bwd_tanh(
                    tdrops[t], v, dlog_att, seed, p_fc, s + 2, L, dv_acc,
                    t1s[t], DPRE1A[sl_a])

            if chain:
                # dodrop GEMM with the tanh backward of dt2 built in its
                # A-operand load (DPRE1B[t] stored on the side); its
                # split-K slabs go to the next iteration as they are
                carry_slabs = _C.dense_tanhbwd_slabs(dt2f, t2s[t], w1b_t,
                                                     DPRE1B[sl])
                carry_salt = s + 1
            else:
                _C.act_bwd_f32_out(dt2f, t2s[t], ACT_TANH, DPRE1B[sl])
                # dodrop GEMM with the ODROP mask (salt s+1) regenerated
                # in the split-K epilogue — one launch instead of
                # GEMM+dropout
                d_out_carry = _C.dense_fwd_drop(DPRE1B[sl], w1b_t, seed,
                                                p_fc, s + 1)

            if need_dctx:
                dcd = DPRE1A[sl_a].matmul(w1a)
                dctx_acc += _drop(dcd, seed, p_fc, s + 0) \
                    .reshape(B, L, D)

        if carry_slabs is not None:
            # the last carry is needed as a tensor (d_init_output)
            d_out_carry = _C.slab_epilogue_drop(carry_slabs, seed, p_fc,
                                                carry_salt)

        # ---- batched weight grads ----
        if CDROP is not None:
            # hipBLASLt schedules this K=T*B*L GEMM on ~32 blocks (163 TF
            # measured); as a T-chunk bmm + sum it fills the chip
            dW1a = torch.bmm(
                DPRE1A.reshape(T, B * L, A).transpose(1, 2),
                CDROP.reshape(T, B * L, D)).sum(dim=0)
        else:
            # p_fc == 0: every step saw the same ctx_flat
            dW1a = DPRE1A.reshape(T, B * L, A).sum(0).t() \
                .matmul(ctx_flat)
        db1a = DPRE1A.sum(0, dtype=torch.float32)
        dWl = DG.t().matmul(XH)
        dbl = DG.sum(0, dtype=torch.float32)
        dW1b = DPRE1B.t().matmul(ODROP)
        db1b = DPRE1B.sum(0, dtype=torch.float32)
        demb_table = _C.embedding_bwd(
            torch.cat([torch.zeros(B, dtype=torch.int64, device=dev),
                       labels_cat[:-B]]),
            DEMB, emb.shape[0])

        d_init_output = (d_out_carry.float()
                         + d_sth_carry.float()).to(torch.bfloat16)
        d_init_memory = dc_carry

        if ctx_ag.leaf_mode:
            # fp32 grads straight to the leaves' AccumulateGrad (the
            # fp32 sums are already fp32 — only the bf16 GEMM outputs
            # need one cast each); dv keeps the leaf's [1, A] shape
            return (dctx_acc, d_init_memory, d_init_output, None, None,
                    demb_table.float(), dW1a.float(), db1a,
                    dW1b.float(), db1b, dv_acc.reshape(1, -1),
                    dWl.float(), dbl, None, None, None, None, None)
        bf = torch.bfloat16
        return (dctx_acc, d_init_memory, d_init_output, None, None,
                demb_table.to(bf), dW1a.to(bf), db1a.to(bf),
                dW1b.to(bf), db1b.to(bf), dv_acc.to(bf),
                dWl.to(bf), dbl.to(bf), None, None, None, None, None)


class DecodeHeadBPTT(torch.autograd.Function):
    """Decode MLP + CE, batched over [T·B, ·].

    Takes the fp32 LEAF weights (not the precast bf16 views) and casts
    inside: its backward then returns fp32 grads straight to the leaves,
    whose AccumulateGrad nodes run at top autograd priority — the DDP
    post-accumulate hooks fire (and the bucket all-reduce launches)
    BEFORE DecoderCoreBPTT.backward executes, overlapping communication
    with the recurrent reverse loop.
    """

    @staticmethod
    def forward(ctx_ag, expd, wd1, bd1, wd2, bd2, sentences, masks,
                seed, p_fc, shadows=None):
        B, T = sentences.shape
        V = wd2.shape[0]
        bf = torch.bfloat16

        if shadows is not None:
            wd1c, bd1c = shadows['wd1'], shadows['bd1']
            wd2c, bd2c = shadows['wd2'], shadows['bd2']
        else:
            wd1c = wd1.to(bf)
            bd1c = bd1.to(bf)
            wd2c = wd2.to(bf)
            bd2c = bd2.to(bf)

        HID = _C.dense_fwd(expd, wd1c, bd1c, ACT_TANH)   # [T·B, Dd]
        HD = _C.hash_dropout_slabs(HID, seed, p_fc, 7, 16, T) \
            if p_fc > 0.0 else HID
        LOGITS = _C.dense_fwd(HD, wd2c, bd2c, ACT_NONE)  # [T·B, V]

        labels_cat = sentences.t().reshape(-1)           # [T·B]
        masks_cat = masks.t().reshape(-1).contiguous()
        CE, LSE = _C.ce_fwd(LOGITS, labels_cat, masks_cat)
        ce = CE.reshape(T, B).t().contiguous()           # [B,T]
        predictions = LOGITS.reshape(T, B, V).argmax(dim=2) \
            .t().contiguous()                            # [B,T]

        ctx_ag.save_for_backward(expd, wd1c, wd2c, HID, HD, LOGITS,
                                 LSE, labels_cat, masks_cat, seed)
        ctx_ag.T = T
        ctx_ag.p_fc = p_fc
        ctx_ag.mark_non_differentiable(predictions)
        return ce, predictions

    @staticmethod
    def backward(ctx_ag, d_ce, _d_pred):
        (expd, wd1c, wd2c, HID, HD, LOGITS, LSE, labels_cat,
         masks_cat, seed) = ctx_ag.saved_tensors
        T = ctx_ag.T
        p_fc = ctx_ag.p_fc

        # batched CE backward over [T·B, V]
        dce_cat = d_ce.t().reshape(-1).contiguous().float()
        DL = _C.ce_bwd(LOGITS, labels_cat, masks_cat, LSE, dce_cat)

        # dX GEMMs through the in-tree split-K tiled kernel (hipBLASLt
        # ran these M=640 shapes at 28-42 TF on ~40 blocks); the
        # transposed-weight copies are ~13 us against ~200 us saved.
        # K must be bf16x8-aligned for the kernel (always true at the
        # flagship dims; tiny test configs fall back to matmul).
        fast_dx = wd2c.shape[0] % 8 == 0 and wd1c.shape[0] % 8 == 0
        if fast_dx:
            wd2_t = wd2c.t().contiguous()
            wd1_t = wd1c.t().contiguous()
            eb = torch.empty(0, dtype=torch.bfloat16, device=DL.device)
            DHD = _C.dense_fwd(DL, wd2_t, eb, 0)  # [T·B, Dd]
        else:
            DHD = DL.matmul(wd2c)
        DHID = _C.hash_dropout_slabs(DHD, seed, p_fc, 7, 16, T) \
            if p_fc > 0.0 else DHD
        DP1 = _C.act_bwd(DHID, HID, ACT_TANH)     # dpre of dec fc_1

        # weight grads first: their AccumulateGrad + DDP hooks are what
        # the core's backward overlaps with.  dWd2 through the in-tree
        # tiled kernel: hipBLASLt ran this [V,TB]x[TB,Dd] shape at
        # 43 TF / 152 us (r02e profile); two small transposes + the
        # MFMA tile land at ~25 us.
        # (here K is T·B: odd batches, e.g. B=1, take the matmul too)
        if fast_dx and DL.shape[0] % 8 == 0:
            dWd2 = _C.dense_fwd(DL.t().contiguous(),
                                HD.t().contiguous(), eb, 0).float()
        else:
            dWd2 = DL.t().matmul(HD).float()
        dbd2 = DL.sum(0, dtype=torch.float32)
        dWd1 = DP1.t().matmul(expd).float()
        dbd1 = DP1.sum(0, dtype=torch.float32)
        d_expd = _C.dense_fwd(DP1, wd1_t, eb, 0) if fast_dx \
            else DP1.matmul(wd1c)                 # [T·B, H+D+E]

        return (d_expd, dWd1, dbd1, dWd2, dbd2, None, None, None, None,
                None)


_EMPTY = {}


def _EMPTY_B(device):
    key = str(device)
    if key not in _EMPTY:
        _EMPTY[key] = torch.empty(0, device=device, dtype=torch.bfloat16)
    return _EMPTY[key]


def run_decoder_bptt(decoder, contexts, init_memory, init_output,
                     sentences, masks):
    """Run the fused BPTT decoder (core + head Functions). Returns
    (ce [B,T], attentions [B,L], predictions [B,T])."""
    d = decoder
    sh = getattr(d, '_shadows', None) \
        if getattr(d, '_shadows_active', False) else None
    if sh:
        # shadow mode: fp32 leaves as autograd inputs, Adam-refreshed
        # bf16 shadows as compute tensors
        expd, attn_acc = DecoderCoreBPTT.apply(
            contexts, init_memory, init_output, sentences, masks,
            d.embedding, d.att_fc_1a.weight, d.att_fc_1a.bias,
            d.att_fc_1b.weight, d.att_fc_1b.bias, d.att_fc_2.weight,
            d.lstm_w, d.lstm_b,
            d._rng, d.nn.fc_drop_rate, d.nn.lstm_drop_rate,
            d.nn.train_cnn, sh)
        ce, predictions = DecodeHeadBPTT.apply(
            expd, d.dec_fc_1.weight, d.dec_fc_1.bias,
            d.dec_fc_2.weight, d.dec_fc_2.bias,
            sentences, masks, d._rng, d.nn.fc_drop_rate, sh)
        return ce, attn_acc, predictions
    expd, attn_acc = DecoderCoreBPTT.apply(
        contexts, init_memory, init_output, sentences, masks,
        d._emb_c, d.att_fc_1a._wc, d.att_fc_1a._bc,
        d.att_fc_1b._wc, d.att_fc_1b._bc, d._att_vc,
        d._lstm_wc, d._lstm_bc,
        d._rng, d.nn.fc_drop_rate, d.nn.lstm_drop_rate,
        d.nn.train_cnn, None)
    ce, predictions = DecodeHeadBPTT.apply(
        expd, d.dec_fc_1.weight, d.dec_fc_1.bias,
        d.dec_fc_2.weight, d.dec_fc_2.bias,
        sentences, masks, d._rng, d.nn.fc_drop_rate, None)
    return ce, attn_acc, predictions
