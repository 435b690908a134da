"""FusedBeamDecoder — the inference engine: beam search with the per-image
work done once and the T decoder steps as project kernels in one hipGraph.

What makes the loop small (default architecture, 2-layer attend MLP):

  * the attention logits are (tanh(fc_1a ctx) + tanh(fc_1b h))·v = t1·v +
    t2·v and the second term is the same for every location, so without
    dropout the softmax over locations does not depend on the LSTM state:
    alpha and the pooled context are per-image constants.  They are
    computed once per batch on B rows (not B·W) through the existing
    attention_tail path with t2 = 0, and the loop has no attention kernel;
  * the pooled context therefore fills fixed columns of the LSTM-input and
    decode-input rows, written once per batch;
  * bf16 weight copies are cached, keyed on the parameters' `_version`
    (load() and the checkpoint loader write with copy_, which bumps it) and
    refreshed in place so captured graphs keep valid addresses.

Per step, GPU: gates GEMM + gate math + expand (`dense_lstm_expand_fwd`
where B·W <= 128, else `dense_fwd` + `lstm_pointwise_fwd` + `expand_fuse`),
decode fc_1, decode fc_2 (or the one dec_fc), `softmax_topk`,
`beam_advance` — all at drop rate 0.  `beam_advance` writes the next
step's state and input rows into
the other half of a double buffer.  The T steps are captured once per
(B, W, T) on one stream as one linear chain and replayed; the loop holds no
host copy and no synchronisation, its state buffers are owned by the
engine, and the temporaries the existing GEMM entry points allocate come
from the graph's private pool.  At most MAX_GRAPHS shapes are captured;
further shapes run the same launches eagerly.

With the 1-layer attention (num_attend_layers == 1) the logits are
att_fc_a(ctx)[b,l] + att_fc_b(h)[n,l]: the second term differs per
location, the softmax follows the LSTM state and nothing can be hoisted
but the first term, l1 [B,L] fp32, computed once per batch.  Each step
then starts with `beam_attend`, one more launch on the same linear chain
(7 instead of 6): it reads h from the step's LSTM-input rows, reads each
image's [L,D] context block once for all its W beams and writes the pooled
context into `pool` and the context columns of those rows.  The contexts
and l1 are copied into engine-owned buffers so a captured graph keeps valid
addresses.  num_decode_layers == 1 is one `dense_fwd` on dec_fc instead
of two.

On the CPU the same structure runs through the op layer's PyTorch twins
(hoisted or in-loop attention, stable top-k, the beam_advance twin),
without a graph.  mode() offers the CPU form for the 2-layer attention
only; search(mode='twin') runs the in-loop form there as well.

Beam semantics are those of BaseModel.beam_search_device: beam_size + 1
expansion, '.'-termination, probability-product scores in fp64, completed
set bounded at beam_size, partial fallback when nothing completed.
"""

import torch

from . import ops
from .ops import functional as F  # noqa: N812
from .utils.topn import CaptionData

MAX_BEAM = 8
MAX_CTX = 1024              # locations: attention_tail and beam_attend
MAX_ATTEND_UNITS = 2048     # LSTM units beam_attend stages in LDS


class _Buffers(object):
    """Static per-(B, W, T) state: everything the loop reads or writes."""

    def __init__(self, B, W, T, K, H, D, E, dtype, dev, L=0, alpha=False):
        """L > 0: the in-loop attention's inputs (contexts, l1) and, for
        a trace, its alpha."""
        N = B * W
        z = dict(device=dev)
        if L:
            self.ctx = torch.zeros(B, L, D, dtype=dtype, **z)
            self.l1 = torch.zeros(B, L, dtype=torch.float32, **z)
        self.alpha = torch.zeros(N, L, dtype=torch.float32, **z) \
            if L and alpha else None
        self.xh = [torch.zeros(N, D + E + H, dtype=dtype, **z)
                   for _ in range(2)]
        self.mem = [torch.zeros(N, H, dtype=dtype, **z) for _ in range(2)]
        self.expd = torch.zeros(N, H + D + E, dtype=dtype, **z)
        self.pool = torch.zeros(N, D, dtype=dtype, **z)
        self.word = [torch.zeros(N, dtype=torch.int64, **z)
                     for _ in range(2)]
        self.state = [(torch.zeros(B, W, dtype=torch.float64, **z),
                       torch.zeros(B, W, T, dtype=torch.int64, **z),
                       torch.zeros(B, W, dtype=torch.int64, **z),
                       torch.zeros(B, W, dtype=torch.float64, **z),
                       torch.zeros(B, W, T, dtype=torch.int64, **z),
                       torch.zeros(B, W, dtype=torch.int64, **z))
                      for _ in range(2)]
        self.top_p = torch.zeros(N, K, dtype=torch.float32, **z)
        self.top_w = torch.zeros(N, K, dtype=torch.int64, **z)
        self.parent = torch.zeros(B, W, dtype=torch.int64, **z)
        self.dims = (B, W, T, K, H, D, E)


class FusedBeamDecoder(object):
    MAX_GRAPHS = 4

    def __init__(self, model):
        self.model = model                  # CaptionGenerator
        self.dec = model.decoder
        self.cfg = model.config
        # 1-layer attention runs inside the loop, 1-layer decode is one GEMM
        self.inloop = self.cfg.num_attend_layers == 1
        self.dec1 = self.cfg.num_decode_layers == 1
        self._w = None                      # cached compute-dtype weights
        self._w_key = None
        self._bufs = {}                     # (B,W,T) -> _Buffers (graphed)
        self._graphs = {}                   # (B,W,T) -> CUDAGraph
        self._seed = None
        self._empty = None

    # ---- what the engine covers ----

    def mode(self, is_cuda, dtype, beam_size):
        """For contexts of that device kind and dtype: 'hip' (GPU
        kernels), 'twin' (CPU, PyTorch twins) or None (the caller falls
        back to beam_search_device)."""
        cfg = self.cfg
        if not (1 <= beam_size <= MAX_BEAM
                and cfg.num_attend_layers in (1, 2)
                and cfg.num_decode_layers in (1, 2)
                and cfg.vocabulary_size >= beam_size + 1):
            return None
        if not is_cuda:
            # the in-loop form is reachable on the CPU through
            # search(mode='twin') only
            if self.inloop:
                return None
            return 'twin' if dtype == torch.float32 else None
        ok = (dtype == torch.bfloat16
              and getattr(cfg, 'use_hip_kernels', True)
              and self.model.dim_ctx % 8 == 0
              and cfg.dim_embedding % 8 == 0
              and cfg.num_lstm_units % 8 == 0
              and self.model.num_ctx <= MAX_CTX)
        if self.inloop:
            ok = ok and cfg.num_lstm_units <= MAX_ATTEND_UNITS
        else:
            # the shape contracts of CaptionGenerator._use_bptt
            ok = (ok and cfg.dim_attend_layer % 512 == 0
                  and cfg.dim_attend_layer <= 2048)
        if not self.dec1:
            ok = ok and cfg.dim_decode_layer % 8 == 0
        if not ok:
            return None
        from .ops import hip
        hip.require()       # a missing extension is an error, not a fallback
        return 'hip'

    # ---- weight cache ----

    def _params(self):
        d = self.dec
        named = [('emb', d.embedding), ('wl', d.lstm_w), ('bl', d.lstm_b)]
        if self.inloop:
            named += [('wa', d.att_fc_a.weight), ('wb', d.att_fc_b.weight)]
        else:
            named += [('w1a', d.att_fc_1a.weight),
                      ('b1a', d.att_fc_1a.bias), ('v', d.att_fc_2.weight)]
        if self.dec1:
            named += [('wd', d.dec_fc.weight), ('bd', d.dec_fc.bias)]
        else:
            named += [('wd1', d.dec_fc_1.weight), ('bd1', d.dec_fc_1.bias),
                      ('wd2', d.dec_fc_2.weight), ('bd2', d.dec_fc_2.bias)]
        if self.cfg.num_initalize_layers == 1:
            init = [('a', d.init_fc_a), ('b', d.init_fc_b)]
        else:
            init = [('a1', d.init_fc_a1), ('a2', d.init_fc_a2),
                    ('b1', d.init_fc_b1), ('b2', d.init_fc_b2)]
        for k, m in init:
            named.append(('wi' + k, m.weight))
            named.append(('bi' + k, m.bias))
        return named

    def weights(self, dtype):
        """Compute-dtype copies of the decoder weights, made once and
        refreshed in place when a parameter was written since."""
        named = self._params()
        key = (dtype,) + tuple((id(p), p._version, p.device)
                               for _, p in named)
        if key != self._w_key:
            if (self._w is not None and self._w_key[0] == dtype
                    and all(self._w[k].device == p.device
                            and self._w[k].shape == p.shape
                            for k, p in named)):
                for k, p in named:
                    self._w[k].copy_(p.detach())
            else:
                self._w = {k: p.detach().to(dtype).contiguous().clone()
                           for k, p in named}
                self._graphs.clear()        # they hold the old addresses
                self._bufs.clear()
            self._w_key = key
        return self._w

    # ---- once per batch, on B rows ----

    def _initial_state(self, w, mean):
        if self.cfg.num_initalize_layers == 1:
            return (ops.dense(mean, w['wia'], w['bia'], None),
                    ops.dense(mean, w['wib'], w['bib'], None))
        ta = ops.dense(mean, w['wia1'], w['bia1'], 'tanh')
        tb = ops.dense(mean, w['wib1'], w['bib1'], 'tanh')
        return (ops.dense(ta, w['wia2'], w['bia2'], None),
                ops.dense(tb, w['wib2'], w['bib2'], None))

    def _per_image(self, w, contexts):
        """-> (memory0, output0, attention constant), each on B rows:
        the pooled context [B,D], or for the in-loop attention l1 [B,L]
        fp32, the state-independent term of its logits."""
        B, L, D = contexts.shape
        mean = contexts.float().mean(dim=1).to(contexts.dtype)
        mem0, out0 = self._initial_state(w, mean)
        if self._seed is None or self._seed.device != contexts.device:
            self._seed = torch.zeros((), dtype=torch.int64,
                                     device=contexts.device)
            self._empty = torch.empty(0, dtype=contexts.dtype,
                                      device=contexts.device)
        if self.inloop:
            l1 = contexts.float().matmul(w['wa'].float().reshape(-1))
            return mem0, out0, l1
        t1 = ops.dense(contexts.reshape(B * L, D), w['w1a'], w['b1a'],
                       'tanh')
        t2 = torch.zeros(B, t1.shape[1], dtype=t1.dtype,
                         device=t1.device)
        _alpha, pooled = ops.attention_tail(
            t1, t2, w['v'].reshape(-1), contexts, 0.0, False, self._seed,
            0)
        return mem0, out0, pooled.to(contexts.dtype)

    def _setup(self, bufs, w, mem0, out0, att, contexts):
        B, W, T, K, H, D, E = bufs.dims
        emb0 = w['emb'][0]
        if self.inloop:
            # beam_attend fills the context columns every step
            bufs.ctx.copy_(contexts)
            bufs.l1.copy_(att)
        else:
            bufs.pool.copy_(att.repeat_interleave(W, dim=0))
            for xh in bufs.xh:
                xh[:, :D] = bufs.pool
            bufs.expd[:, H:H + D] = bufs.pool
        bufs.xh[0][:, D:D + E] = emb0
        bufs.xh[0][:, D + E:] = out0.repeat_interleave(W, dim=0)
        bufs.expd[:, H + D:] = emb0
        bufs.mem[0].copy_(mem0.repeat_interleave(W, dim=0))
        bufs.word[0].zero_()
        for t in bufs.state[0]:
            t.zero_()
        bufs.state[0][0][:, 0] = 1.0        # live scores: 1, 0, 0, ...

    # ---- one step ----

    def _step(self, bufs, w, t, hip, period):
        B, W, T, K, H, D, E = bufs.dims
        cur, nxt = t % 2, (t + 1) % 2
        xh, mem, ids = bufs.xh[cur], bufs.mem[cur], bufs.word[cur]
        if self.inloop:
            # reads h from xh's state columns, writes pool and xh[:, :D]
            ops.beam_attend(bufs.ctx, bufs.l1, w['wb'], xh, bufs.pool,
                            bufs.alpha)
        if hip:
            from sat_amd import _C
            # the existing expand epilogues write the whole decode-input
            # row (output, pooled and embedding columns) from `pool` and
            # `ids`; the CPU form below relies on the columns _setup and
            # beam_advance laid down
            if B * W <= 128 and (D + E + H) % 32 == 0:
                _g, c_new, h_new = _C.dense_lstm_expand_fwd(
                    xh, w['wl'], w['bl'], mem, bufs.pool, w['emb'], ids,
                    self._seed, bufs.expd, self._empty, 1.0, 0.0, 0.0, 0)
            else:
                gates = _C.dense_fwd(xh, w['wl'], w['bl'], 0)
                h_new, c_new = _C.lstm_pointwise_fwd(gates, mem, 1.0)
                _C.expand_fuse(h_new, bufs.pool, w['emb'], ids, self._seed,
                               bufs.expd, self._empty, 0.0, 0.0, 0)
            if self.dec1:
                logits = _C.dense_fwd(bufs.expd, w['wd'], w['bd'], 0)
            else:
                hid = _C.dense_fwd(bufs.expd, w['wd1'], w['bd1'], 1)
                logits = _C.dense_fwd(hid, w['wd2'], w['bd2'], 0)
        else:
            h_new, c_new = F.lstm_cell(xh[:, :D + E], xh[:, D + E:], mem,
                                       w['wl'], w['bl'])
            bufs.expd[:, :H] = h_new
            if self.inloop:
                bufs.expd[:, H:H + D] = bufs.pool
            if self.dec1:
                logits = F.dense(bufs.expd, w['wd'], w['bd'], None)
            else:
                hid = F.dense(bufs.expd, w['wd1'], w['bd1'], 'tanh')
                logits = F.dense(hid, w['wd2'], w['bd2'], None)
        ops.softmax_topk(logits, K, out=(bufs.top_p, bufs.top_w))
        ops.beam_advance(bufs.state[cur], bufs.state[nxt], bufs.top_p,
                         bufs.top_w, period, c_new, h_new, w['emb'],
                         bufs.mem[nxt], bufs.xh[nxt], bufs.expd,
                         bufs.word[nxt], bufs.parent)

    def _run(self, bufs, w, hip, period, trace=None):
        B, W, T, K, H, D, E = bufs.dims
        for t in range(T):
            cur, nxt = t % 2, (t + 1) % 2
            if trace is not None:
                rec = {'last_word': bufs.word[cur].clone(),
                       'memory': bufs.mem[cur].clone(),
                       'output': bufs.xh[cur][:, D + E:].clone(),
                       'scores_in': bufs.state[cur][0].clone(),
                       'c_scores_in': bufs.state[cur][3].clone()}
            self._step(bufs, w, t, hip, period)
            if trace is not None:
                rec.update(top_p=bufs.top_p.clone(),
                           top_w=bufs.top_w.clone(),
                           parent=bufs.parent.clone(),
                           word=bufs.word[nxt].reshape(B, W).clone(),
                           score=bufs.state[nxt][0].clone(),
                           c_scores=bufs.state[nxt][3].clone())
                if self.inloop:
                    rec['alpha'] = bufs.alpha.clone()
                trace.append(rec)

    # ---- public ----

    @torch.no_grad()
    def search(self, contexts, period_id, beam_size, graph=True,
               return_trace=False, mode=None):
        """contexts [B,L,D] -> per image a list of CaptionData (best
        first), as BaseModel.beam_search_device returns it.  With
        return_trace also a per-step list of dicts: the state fed to the
        step (last_word, memory, output, scores_in), the top_p / top_w it
        produced, the selected (parent, word, score) and, with the
        in-loop attention, its alpha [B*W,L]; a traced search runs
        eagerly.  mode='twin' or 'hip' runs that form without asking
        mode() (the CPU twin of the in-loop attention is offered this way
        only)."""
        if mode is None:
            mode = self.mode(contexts.is_cuda, contexts.dtype, beam_size)
            if mode is None:
                raise ValueError('FusedBeamDecoder does not cover this '
                                 'configuration')
        elif mode not in ('twin', 'hip'):
            raise ValueError("mode must be 'twin', 'hip' or None")
        hip = mode == 'hip'
        cfg = self.cfg
        B, L, D = contexts.shape
        W, K, T = beam_size, beam_size + 1, cfg.max_caption_length
        H, E = cfg.num_lstm_units, cfg.dim_embedding
        contexts = contexts.contiguous()
        w = self.weights(contexts.dtype)
        mem0, out0, att = self._per_image(w, contexts)

        key = (B, W, T)
        trace = [] if return_trace else None
        graphed = hip and graph and not return_trace
        bufs = self._bufs.get(key) if graphed else None
        if bufs is None:
            bufs = _Buffers(B, W, T, K, H, D, E, contexts.dtype,
                            contexts.device, L if self.inloop else 0,
                            return_trace)
        period = int(period_id)
        if graphed and key not in self._graphs \
                and len(self._graphs) < self.MAX_GRAPHS:
            self._capture(key, bufs, w, period, mem0, out0, att, contexts)
        self._setup(bufs, w, mem0, out0, att, contexts)
        g = self._graphs.get(key) if graphed else None
        if g is not None and g[1] == period:
            g[0].replay()
        else:
            self._run(bufs, w, hip, period, trace)
        results = self._readout(bufs)
        return (results, trace) if return_trace else results

    def _capture(self, key, bufs, w, period, mem0, out0, att, contexts):
        """Warm the launches up on a side stream, then capture the T steps
        on one stream as one linear chain."""
        self._setup(bufs, w, mem0, out0, att, contexts)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            self._run(bufs, w, True, period)
        torch.cuda.current_stream().wait_stream(side)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            self._run(bufs, w, True, period)
        self._bufs[key] = bufs
        self._graphs[key] = (g, period)

    def _readout(self, bufs):
        """The one host readout; completed-else-partial rule and result
        structure of BaseModel.beam_search_device."""
        B, W, T, K, H, D, E = bufs.dims
        live = bufs.state[T % 2]
        p_scores, p_seqs, p_lens, c_scores, c_seqs, c_lens = [
            x.cpu().numpy() for x in live]
        results = []
        for k in range(B):
            use_partial = float(c_scores[k].max()) <= 0.0
            ss = p_scores[k] if use_partial else c_scores[k]
            qq = p_seqs[k] if use_partial else c_seqs[k]
            ll = p_lens[k] if use_partial else c_lens[k]
            order = ss.argsort()[::-1][:W]
            caps = [CaptionData([int(v) for v in qq[i][:ll[i]]],
                                None, None, float(ss[i]))
                    for i in order if ss[i] > 0.0 or use_partial]
            if not caps:
                caps = [CaptionData([], None, None, 0.0)]
            results.append(caps)
        return results
