"""Optimizers + global-norm gradient clipping (parity with reference
`model.py:461-513` build_optimizer).

Supports 'Adam' (default; β1/β2/ε from config, config.py:41-43), 'RMSProp',
'Momentum' (with use_nesterov) and 'SGD', all behind global-norm clipping at
config.clip_gradients (model.py:510) and the optional staircase exponential
LR decay (model.py:466-474, inactive at the default decay factor 1.0).

On GPU every kind runs two hand-written CDNA4 kernels per step, a
multi-tensor grad-norm² reduction and a multi-tensor clip+update — one
launch each over all ~14M decoder params instead of per-tensor eager ops,
with the step counter, the LR staircase and the clip scale on the device,
so the step has no host sync and is hipGraph-capturable:

  * every kind: sq_norm_chunks + opt_step_mt
    (sat_amd/ops/csrc/optim_mt.hip), over a host-built table of chunks of
    MT_CHUNK elements that never cross a tensor; the norm is one partial
    per block summed in a fixed order, so a step is bitwise reproducible.
    `use_fused_optimizer = False` sends RMSProp, Momentum and SGD down the
    eager path instead; Adam is always fused on the GPU.
  * `use_adam_chunk_norm = False` keeps Adam on its earlier pair
    sq_norm_mt + adam_step_mt (sat_amd/ops/csrc/kernels.hip): one search
    per element over the concatenation of all tensors, atomics in the norm.

The eager path (PyTorch math, one host sync per tensor for the norm) serves
the CPU.
"""

import math

import torch

# elements per chunk of the chunk-table kernels: one float4 per thread of a
# 256-thread block, and small enough that the ~14M flagship elements give
# each of the 2048 blocks 6 or 7 chunks (an uneven last round costs 1/7)
MT_CHUNK = 1024

FUSED_KINDS = ('Adam', 'RMSProp', 'Momentum', 'SGD')
# kernel codes of optim_mt.hip
_K_SGD, _K_MOM, _K_NAG, _K_RMS, _K_RMSC, _K_ADAM = range(6)


def build_chunk_table(numels, chunk=MT_CHUNK):
    """Cut tensors of `numels` elements into (tensor, start, count) chunks
    of at most `chunk` elements, in tensor order.  No chunk crosses a
    tensor, every start is a multiple of 4 (chunk is), and only the last
    chunk of a tensor may be short."""
    if chunk <= 0 or chunk % 4:
        raise ValueError('chunk must be a positive multiple of 4')
    table = []
    for t, n in enumerate(numels):
        for start in range(0, n, chunk):
            table.append((t, start, min(chunk, n - start)))
    return table


class Optimizer(object):
    def __init__(self, config, params):
        self.config = config
        self.params = [p for p in params if p.requires_grad]
        self.kind = config.optimizer
        self.step_count = 0
        self.state = {}
        for p in self.params:
            s = {}
            if self.kind == 'Adam':
                s['m'] = torch.zeros_like(p, dtype=torch.float32)
                s['v'] = torch.zeros_like(p, dtype=torch.float32)
            elif self.kind == 'RMSProp':
                s['ms'] = torch.zeros_like(p, dtype=torch.float32)
                s['mom'] = torch.zeros_like(p, dtype=torch.float32)
                if config.centered:
                    s['mg'] = torch.zeros_like(p, dtype=torch.float32)
            elif self.kind == 'Momentum':
                s['mom'] = torch.zeros_like(p, dtype=torch.float32)
            self.state[p] = s

    def learning_rate(self):
        cfg = self.config
        lr = cfg.initial_learning_rate
        if cfg.learning_rate_decay_factor < 1.0:
            # staircase exponential decay (model.py:466-474)
            lr = lr * cfg.learning_rate_decay_factor ** (
                self.step_count // cfg.num_steps_per_decay)
        return lr

    @property
    def fused(self):
        """step() runs the fused HIP kernels (and zeroes grads itself)"""
        if not self.params or not self.params[0].is_cuda:
            return False
        if self.kind == 'Adam':
            return True
        return (self.kind in FUSED_KINDS and bool(
            getattr(self.config, 'use_fused_optimizer', True)))

    def zero_grad(self):
        for p in self.params:
            p.grad = None

    # ---- bf16 shadow weights ----
    # The fused kernels refresh persistent bf16 copies of registered
    # params in its own update pass (free — the new value is already in
    # a register), so the compute path reads shadows instead of casting
    # weights every forward.  Non-fused/eager steps fall back to an
    # explicit sync so shadows can never go stale.

    def register_shadows(self, mapping):
        """mapping: {param: bf16 tensor of the same shape}."""
        self._shadows = dict(mapping)
        self._mt_ptrs = None  # force desc rebuild
        self._ck_ptrs = None
        self.sync_shadows()

    def sync_shadows(self):
        for p, sh in getattr(self, '_shadows', {}).items():
            with torch.no_grad():
                sh.copy_(p.detach().to(sh.dtype))

    @torch.no_grad()
    def step(self):
        cfg = self.config
        self.step_count += 1
        lr = self.learning_rate()
        fused = self.fused
        use_hip = fused and self.kind == 'Adam'
        if fused:
            # the fused kernel walks p/g/m/v in flat storage order and m/v
            # are laid out like p, so a grad in another layout (a
            # contiguous grad assigned to a channels_last weight) would
            # pair the wrong elements: lay it out like its parameter, once
            # (autograd then accumulates into that tensor in place)
            for p in self.params:
                g = p.grad
                if g is not None and g.stride() != p.stride():
                    p.grad = torch.empty_like(p, dtype=g.dtype).copy_(g)
        if fused and not use_hip:
            return self._step_chunks()
        if use_hip:
            grads = self._dense_grads()
        else:
            grads = [p.grad if p.grad is not None else torch.zeros_like(p)
                     for p in self.params]

        if use_hip:
            from sat_amd import _C
            from .ops import hip
            hip.require()
            # Everything stays on-device (grad-norm², clip scale, step
            # counter, bias correction, LR decay): zero host syncs, so the
            # whole optimizer step is hipGraph-capturable.  All tensors go
            # through ONE multi-tensor kernel via a device pointer table,
            # rebuilt only when any data pointer changes.
            if not hasattr(self, 'step_dev') or self.step_dev is None:
                self.step_dev = torch.zeros(
                    (), dtype=torch.float32,
                    device=self.params[0].device)
                self.step_dev.fill_(float(self.step_count - 1))
            self.step_dev.add_(1.0)
            shadows = getattr(self, '_shadows', {})
            ptrs = tuple(
                (p.data.data_ptr(), g.data_ptr(),
                 self.state[p]['m'].data_ptr(),
                 self.state[p]['v'].data_ptr(),
                 shadows[p].data_ptr() if p in shadows else 0)
                for p, g in zip(self.params, grads))
            if getattr(self, '_mt_ptrs', None) != ptrs:
                dev = self.params[0].device
                self._mt_ptrs = ptrs
                self._mt_desc = torch.tensor(
                    [list(row) for row in ptrs],
                    dtype=torch.int64).to(dev)
                numels = [p.numel() for p in self.params]
                cum = [0]
                for n in numels:
                    cum.append(cum[-1] + n)
                self._mt_cum = torch.tensor(
                    cum, dtype=torch.int64).to(dev)
                self._mt_total = cum[-1]
                # float4 path needs every tensor boundary 16B-aligned
                self._mt_vec4 = all(c % 4 == 0 for c in cum)
                for g, p0 in zip(grads, self.params):
                    # dense storage in either layout (channels_last conv
                    # grads included) is fine: g has p's strides by now,
                    # m/v were allocated like p, and the kernel iterates
                    # flat storage order
                    if g.dtype != torch.float32 or not (
                            g.is_contiguous()
                            or g.is_contiguous(
                                memory_format=torch.channels_last)):
                        raise RuntimeError(
                            'fused Adam needs dense fp32 grads; got '
                            '%s for a %s param' % (g.dtype,
                                                   tuple(p0.shape)))
            if getattr(cfg, 'use_adam_chunk_norm', True):
                # the norm as one partial per block over the chunk table,
                # summed in a fixed order by every block of the update
                # (the _mt_* tables above are kept for the earlier route
                # below and for the tests that read them)
                return self._launch_chunks(
                    grads, ('m', 'v'), _K_ADAM, cfg.beta1, cfg.beta2)
            gsq = _C.sq_norm_mt(self._mt_desc, self._mt_cum,
                                len(self.params), self._mt_total)
            # zero_grads=True: the update kernel clears p.grad in the
            # same pass, so the engine skips its per-tensor fill
            # launches and autograd accumulates into stable addresses
            _C.adam_step_mt(
                self._mt_desc, self._mt_cum, len(self.params),
                self._mt_total, self.step_dev,
                cfg.initial_learning_rate,
                cfg.learning_rate_decay_factor, cfg.num_steps_per_decay,
                cfg.beta1, cfg.beta2, cfg.epsilon,
                cfg.clip_gradients, gsq, True,
                getattr(self, '_mt_vec4', False))
            return

        # ---- eager path (CPU, or use_fused_optimizer = False) ----
        gnorm = math.sqrt(sum(float((g.float() ** 2).sum()) for g in grads))
        scale = 1.0
        if cfg.clip_gradients and gnorm > cfg.clip_gradients:
            scale = cfg.clip_gradients / (gnorm + 1e-12)

        for p, g in zip(self.params, grads):
            g = g.float() * scale
            s = self.state[p]
            if self.kind == 'Adam':
                s['m'].mul_(cfg.beta1).add_(g, alpha=1 - cfg.beta1)
                s['v'].mul_(cfg.beta2).addcmul_(g, g, value=1 - cfg.beta2)
                mhat = s['m'] / (1 - cfg.beta1 ** self.step_count)
                vhat = s['v'] / (1 - cfg.beta2 ** self.step_count)
                upd = mhat / (vhat.sqrt() + cfg.epsilon)
            elif self.kind == 'RMSProp':
                # TF RMSPropOptimizer: mom = m*mom + lr*g/sqrt(ms[-mg^2]+eps)
                # and var -= mom (epsilon inside the sqrt)
                s['ms'].mul_(cfg.decay).addcmul_(g, g, value=1 - cfg.decay)
                denom = s['ms']
                if cfg.centered:
                    s['mg'].mul_(cfg.decay).add_(g, alpha=1 - cfg.decay)
                    denom = denom - s['mg'] ** 2
                s['mom'].mul_(cfg.momentum).add_(
                    lr * g / (denom + cfg.epsilon).sqrt())
                p.data.add_(-s['mom'].to(p.dtype))
                continue
            elif self.kind == 'Momentum':
                s['mom'].mul_(cfg.momentum).add_(g)
                if cfg.use_nesterov:
                    upd = g + cfg.momentum * s['mom']
                else:
                    upd = s['mom']
            elif self.kind == 'SGD':
                upd = g
            else:
                raise ValueError('unknown optimizer %r' % (self.kind,))
            p.data.add_(upd.to(p.dtype), alpha=-lr)
        self.sync_shadows()

    def _dense_grads(self):
        """p.grad per parameter; one without grad takes a zero gradient
        from a persistent buffer, so that the pointer tables stay valid"""
        zeros = getattr(self, '_ck_zero', None)
        if zeros is None:
            zeros = self._ck_zero = {}
        grads = []
        for p in self.params:
            g = p.grad
            if g is None:
                g = zeros.get(p)
                if g is None:
                    g = zeros[p] = torch.zeros_like(p)
            grads.append(g)
        return grads

    def _step_chunks(self):
        """RMSProp / Momentum / SGD through optim_mt.hip: two launches (one
        without clipping) and the counter's add_, no host sync, nothing
        allocated after the first call.  The slots are the tensors of
        self.state, so checkpoints move freely between this route and the
        eager one."""
        cfg = self.config
        from .ops import hip
        hip.require()
        dev = self.params[0].device
        if getattr(self, 'step_dev', None) is None:
            self.step_dev = torch.zeros((), dtype=torch.float32, device=dev)
            self.step_dev.fill_(float(self.step_count - 1))
        self.step_dev.add_(1.0)
        if self.kind == 'RMSProp':
            names = ('ms', 'mom', 'mg') if cfg.centered else ('ms', 'mom')
            kind = _K_RMSC if cfg.centered else _K_RMS
        elif self.kind == 'Momentum':
            names = ('mom',)
            kind = _K_NAG if cfg.use_nesterov else _K_MOM
        else:
            names, kind = (), _K_SGD
        self._launch_chunks(self._dense_grads(), names, kind,
                            cfg.momentum, cfg.decay)

    def _launch_chunks(self, grads, names, kind, momentum, decay):
        """sq_norm_chunks (with clipping) + opt_step_mt over the chunk
        table of `grads` and the state slots `names`; step_dev is already
        advanced.  Adam passes beta1 / beta2 as momentum / decay."""
        cfg = self.config
        from sat_amd import _C
        dev = self.params[0].device
        shadows = getattr(self, '_shadows', {})
        ptrs = tuple(
            (p.data.data_ptr(), g.data_ptr())
            + tuple(self.state[p][k].data_ptr() for k in names)
            + (0,) * (3 - len(names))
            + (shadows[p].data_ptr() if p in shadows else 0,)
            for p, g in zip(self.params, grads))
        if getattr(self, '_ck_ptrs', None) != ptrs:
            for g, p0 in zip(grads, self.params):
                # dense storage in either layout: g has p's strides by now,
                # the slots were allocated like p, and the kernel walks
                # flat storage order
                if g.dtype != torch.float32 or not (
                        g.is_contiguous()
                        or g.is_contiguous(
                            memory_format=torch.channels_last)):
                    raise RuntimeError(
                        'fused %s needs dense fp32 grads; got '
                        '%s for a %s param' % (self.kind, g.dtype,
                                               tuple(p0.shape)))
            numels = [p.numel() for p in self.params]
            if max(numels) >= 2 ** 31:
                raise RuntimeError('fused %s: a tensor of 2^31 or more '
                                   'elements' % (self.kind,))
            table = build_chunk_table(numels, MT_CHUNK)
            # 16-byte route: float4 traffic on p, g and the slots, 8-byte
            # stores of 4 bf16 to the shadow
            vec = [int(all(a % 16 == 0 for a in row[:5])
                       and row[5] % 8 == 0) for row in ptrs]
            self._ck_ptrs = ptrs
            self._ck_chunks = torch.tensor(
                table, dtype=torch.int32).reshape(len(table), 3).to(dev)
            self._ck_desc = torch.tensor(
                [list(row) for row in ptrs], dtype=torch.int64).to(dev)
            self._ck_vec = torch.tensor(vec, dtype=torch.int32).to(dev)
            self._ck_any_vec = any(vec)
            if getattr(self, '_ck_partials', None) is None:
                # one partial of sum g^2 per block of the norm kernel
                self._ck_partials = torch.zeros(
                    2048, dtype=torch.float32, device=dev)
        clip = float(cfg.clip_gradients or 0.0)
        if clip > 0.0:
            _C.sq_norm_chunks(self._ck_chunks, self._ck_desc, self._ck_vec,
                              self._ck_partials)
        # zero_grads=True: the update kernel clears p.grad in the same
        # pass, so the engine skips its per-tensor fill launches and
        # autograd accumulates into stable addresses
        _C.opt_step_mt(
            self._ck_chunks, self._ck_desc, self._ck_vec, self._ck_any_vec,
            self.step_dev, cfg.initial_learning_rate,
            cfg.learning_rate_decay_factor, cfg.num_steps_per_decay,
            momentum, decay, cfg.epsilon, clip, kind, True,
            self._ck_partials)

    # ---- checkpoint support: optimizer slots are saved like TF's ----

    def state_arrays(self):
        out = {}
        for i, p in enumerate(self.params):
            for k, t in self.state[p].items():
                out['optimizer/%d/%s' % (i, k)] = t
        out['optimizer/step_count'] = torch.tensor(
            float(self.step_count))
        return out

    def load_state_arrays(self, arrays):
        for i, p in enumerate(self.params):
            for k in self.state[p]:
                key = 'optimizer/%d/%s' % (i, k)
                if key in arrays:
                    self.state[p][k].copy_(
                        torch.as_tensor(arrays[key]).to(
                            self.state[p][k].device))
        if 'optimizer/step_count' in arrays:
            self.step_count = int(float(arrays['optimizer/step_count']))
            if getattr(self, 'step_dev', None) is not None:
                self.step_dev.fill_(float(self.step_count))
        self.sync_shadows()
