#!/usr/bin/env python3
"""Optimizer benchmark: the chunk-table kernels (optim_mt.hip) against the
eager path they replace, on the flagship's trainable set (default Config,
frozen VGG16, B = 32).

    python tools/bench_optim.py [--kinds SGD,Momentum,RMSProp]
                                [--opt-steps 200] [--steps 30] [--warmup 10]
                                [--repeats 3] [--no-train] [--out FILE]
    python tools/bench_optim.py --trace-loop 20     # under a kernel trace

For each kind (Momentum with Nesterov, RMSProp centered, momentum 0.9) it
times with device events over a warm loop, fused and
`use_fused_optimizer = False` alternating:

  1. Optimizer.step() alone;
  2. the update kernel alone, launched back to back (fused only), with its
     byte count and the share of the 6.29 TB/s copy rate it reaches;
  3. the whole train_step: one captured graph for the fused route, the
     engine's eager fallback for the other.

One JSON line per figure.  --trace-loop N only runs N fused steps of every
kind and of Adam, for a kernel trace taken in a run of its own.
"""
import argparse
import copy
import json
import statistics
import sys

sys.path.insert(0, '.')

import torch  # noqa: E402

COPY_RATE = 6.29e12        # measured float4 copy, bytes/s

# bytes per element the update kernel moves: (read, write); +2 per
# shadowed element
TRAFFIC = {'SGD': (8, 8), 'Momentum': (12, 12), 'RMSProp': (20, 20),
           'Adam': (16, 16)}


def _emit(fh, **kw):
    line = json.dumps(kw)
    print(line, flush=True)
    if fh is not None:
        fh.write(line + '\n')
        fh.flush()


def _event_ms(fn, iters, warm):
    """mean ms per call of fn over `iters` calls after `warm` warm ones"""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0 = torch.cuda.Event(enable_timing=True)
    e1 = torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--kinds', default='SGD,Momentum,RMSProp')
    ap.add_argument('--opt-steps', type=int, default=200)
    ap.add_argument('--steps', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--no-train', action='store_true')
    ap.add_argument('--trace-loop', type=int, default=0)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_optim.py measures on the GPU; none found')

    from config import Config
    from sat_amd.models.base_model import BaseModel
    from sat_amd.optim import MT_CHUNK, Optimizer
    from sat_amd import _C

    fh = open(args.out, 'w') if args.out else None
    cfg = Config()
    cfg.phase = 'train'
    cfg.train_cnn = False
    cfg.synthetic_data = True
    cfg.batch_size = args.batch
    cfg.device = 'cuda'
    cfg.use_hip_graph = True
    torch.manual_seed(cfg.seed)
    m = BaseModel(cfg)
    params = m.optimizer.params
    smap = dict(getattr(m.optimizer, '_shadows', {}))
    numel = sum(p.numel() for p in params)
    shadowed = sum(p.numel() for p in smap)
    _emit(fh, what='trainable set', tensors=len(params), elements=numel,
          shadowed_elements=shadowed, mt_chunk=MT_CHUNK)

    g = torch.Generator().manual_seed(cfg.seed)
    T = cfg.max_caption_length
    batch = (
        (torch.randn(args.batch, 3, 224, 224, generator=g) * 50.0).cuda(),
        torch.randint(1, cfg.vocabulary_size, (args.batch, T),
                      generator=g).cuda(),
        torch.ones(args.batch, T).cuda())
    snap = [p.detach().clone() for p in params]

    def restore(opt):
        with torch.no_grad():
            for p, s in zip(params, snap):
                p.copy_(s)
            for st in opt.state.values():
                for t in st.values():
                    t.zero_()
        opt.step_count = 0
        if getattr(opt, 'step_dev', None) is not None:
            opt.step_dev.zero_()
        opt.sync_shadows()

    def make_opt(kind, fused):
        c = copy.copy(cfg)
        c.optimizer = kind
        c.momentum = 0.9
        c.use_fused_optimizer = fused
        opt = Optimizer(c, params)
        if smap:
            opt.register_shadows(smap)
        return opt

    def backward_once():
        m.model.train()
        for p in params:
            if p.grad is not None:
                p.grad.zero_()
        m.model(*batch)['total_loss'].backward()
        torch.cuda.synchronize()

    kinds = [k for k in args.kinds.split(',') if k]

    if args.trace_loop:
        backward_once()
        for kind in kinds + ['Adam']:
            opt = make_opt(kind, True)
            for _ in range(args.trace_loop):
                opt.step()
            torch.cuda.synchronize()
            restore(opt)
        return

    opts = {}
    for kind in kinds:
        of, oe = make_opt(kind, True), make_opt(kind, False)
        assert of.fused and not oe.fused
        # 1. Optimizer.step() alone (the values do not change the work)
        backward_once()
        res = {'fused': [], 'eager': []}
        for _ in range(args.repeats):
            for name, opt in (('fused', of), ('eager', oe)):
                restore(opt)
                res[name].append(_event_ms(opt.step, args.opt_steps, 10))
        f, e = (statistics.median(res[k]) for k in ('fused', 'eager'))
        _emit(fh, what='Optimizer.step()', kind=kind, fused_ms=round(f, 4),
              eager_ms=round(e, 4), speedup=round(e / f, 2),
              fused_all=[round(x, 4) for x in res['fused']],
              eager_all=[round(x, 4) for x in res['eager']])

        # 2. the update kernel alone, back to back
        restore(of)
        of.step()
        c = of.config
        code = {'SGD': 0, 'Momentum': 2 if c.use_nesterov else 1,
                'RMSProp': 4 if c.centered else 3}[kind]

        def update():
            _C.opt_step_mt(of._ck_chunks, of._ck_desc, of._ck_vec,
                           of._ck_any_vec, of.step_dev,
                           c.initial_learning_rate,
                           c.learning_rate_decay_factor,
                           c.num_steps_per_decay, c.momentum, c.decay,
                           c.epsilon, float(c.clip_gradients), code, True,
                           of._ck_partials)

        def norm():
            _C.sq_norm_chunks(of._ck_chunks, of._ck_desc, of._ck_vec,
                              of._ck_partials)

        rd, wr = TRAFFIC[kind]
        if kind == 'RMSProp' and not c.centered:
            rd, wr = rd - 4, wr - 4
        for name, fn, nbytes in (
                ('update kernel', update, numel * (rd + wr) + 2 * shadowed),
                ('norm kernel', norm, numel * 4)):
            ts = [_event_ms(fn, args.opt_steps, 10)
                  for _ in range(args.repeats)]
            t = statistics.median(ts)
            _emit(fh, what=name, kind=kind, us=round(t * 1e3, 2),
                  bytes=nbytes, floor_us=round(nbytes / COPY_RATE * 1e6, 2),
                  share_of_copy_rate=round(nbytes / COPY_RATE / (t * 1e-3),
                                           3),
                  ns_per_kib=round(t * 1e6 / (nbytes / 1024.0), 4),
                  vec_route=bool(of._ck_any_vec),
                  chunks=int(of._ck_chunks.shape[0]))

        opts[kind] = (of, oe)

    # 3. the whole train_step: every captured run before the first eager
    # fallback, whose failed capture attempt comes first in its warm-up
    out = {k: {} for k in kinds}
    for name in (() if args.no_train else ('fused', 'eager')):
        for kind in kinds:
            opt = opts[kind][0 if name == 'fused' else 1]
            restore(opt)
            for p in params:
                p.grad = None
            m.optimizer, m._engine = opt, None
            out[kind][name] = _event_ms(lambda: m.train_step(*batch),
                                        args.steps, args.warmup)
            out[kind][name + '_mode'] = (
                'full graph' if m._engine.mode == 'full' else
                'eager fallback' if m._engine.failed else m._engine.mode)
            _emit(fh, what='train_step ' + name, kind=kind,
                  ms=round(out[kind][name], 3),
                  mode=out[kind][name + '_mode'])
            if name == 'eager':
                o = out[kind]
                _emit(fh, what='train_step', kind=kind, batch=args.batch,
                      fused_ms=round(o['fused'], 3),
                      eager_ms=round(o['eager'], 3),
                      speedup=round(o['eager'] / o['fused'], 2),
                      fused_mode=o['fused_mode'], eager_mode=o['eager_mode'])
    if fh is not None:
        fh.close()


if __name__ == '__main__':
    main()
