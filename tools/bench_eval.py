#!/usr/bin/env python3
"""Eval (beam search) throughput: captions/sec at beam=3, batched.

    python tools/bench_eval.py [--batch 64] [--batches 5] [--beam 3]
                               [--host-beam | --fused] [--repeats 1]
                               [--attend-layers {1,2}] [--decode-layers {1,2}]

Measures the device-resident beam path (or the host-heap reference path
with --host-beam, or the fused graph-captured engine with --fused) on the
flagship eval model shape: VGG16 frozen,
LSTM-512, vocab 5000, synthetic images.  --attend-layers / --decode-layers
select the 1-layer forms of the attention and decode MLPs.
"""
import argparse
import sys
import time

sys.path.insert(0, '.')

import torch  # noqa: E402


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--batch', type=int, default=64)
    p.add_argument('--batches', type=int, default=5)
    p.add_argument('--beam', type=int, default=3)
    p.add_argument('--host-beam', action='store_true')
    p.add_argument('--fused', action='store_true',
                   help='config.use_fused_beam (sat_amd/beam.py)')
    p.add_argument('--repeats', type=int, default=1,
                   help='timed windows of --batches batches each')
    p.add_argument('--attend-layers', type=int, choices=(1, 2), default=2,
                   help='config.num_attend_layers')
    p.add_argument('--decode-layers', type=int, choices=(1, 2), default=2,
                   help='config.num_decode_layers')
    args = p.parse_args()

    from config import Config
    from sat_amd.models.base_model import BaseModel
    from sat_amd.data.vocabulary import Vocabulary

    cfg = Config()
    cfg.phase = 'eval'
    cfg.train_cnn = False
    cfg.synthetic_data = True
    cfg.beam_size = args.beam
    cfg.use_device_beam = not args.host_beam
    cfg.use_fused_beam = args.fused
    cfg.num_attend_layers = args.attend_layers
    cfg.num_decode_layers = args.decode_layers
    torch.manual_seed(cfg.seed)

    vocab = Vocabulary(cfg.vocabulary_size)
    vocab.build(['a man rides a horse down the street .',
                 'a dog sits on the beach sand .'])
    m = BaseModel(cfg)
    files = ['synthetic://%d' % i for i in range(args.batch)]

    m.beam_search(files, vocab)  # warmup
    if torch.cuda.is_available():
        torch.cuda.synchronize()
    name = 'fused' if args.fused else 'host' if args.host_beam else 'device'
    if args.fused and m._fused_beam_mode() != 'hip':
        name = 'fused->device fallback'
    if (args.attend_layers, args.decode_layers) != (2, 2):
        name += ' attend=%d decode=%d' % (args.attend_layers,
                                          args.decode_layers)
    for _ in range(args.repeats):
        t0 = time.perf_counter()
        for _ in range(args.batches):
            m.beam_search(files, vocab)
        if torch.cuda.is_available():
            torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        n = args.batch * args.batches
        print('%s beam=%d batch=%d: %.1f captions/sec (%.1f ms/batch)'
              % (name, args.beam, args.batch, n / dt,
                 dt / args.batches * 1000), flush=True)


if __name__ == '__main__':
    main()
