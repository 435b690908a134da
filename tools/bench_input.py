#!/usr/bin/env python3
"""Input-pipeline throughput on real files (sat_amd/data/pipeline.py).

    python tools/bench_input.py [--images 512] [--batch 32]
                                [--threads 4,8,16] [--repeats 3]
                                [--out FILE.md]

Writes --images synthetic 640x480 JPEGs to a temporary directory and
times, in this one process:

  1. the synchronous host path per batch: ImageLoader.load_images (PIL
     decode + resize + mean), the NCHW permute + copy to the device, the
     cast to bf16 channels_last, ending in a device synchronise;
  2. the pipeline alone (BatchPrefetcher + ImagePrep, no model) at each
     thread count: batches/s over an epoch after a warm-up epoch;
  3. the resize kernel alone on one batch, by device events, warmed up,
     median of 25 launches;
  4. real-file training (the body of BaseModel.train: _batches,
     _load_batch, train_step; no summaries or checkpoints) in images/s
     with the knobs off and on, alternating, --repeats times each.

Needs a GPU; prints the figures and, with --out, writes them as a
markdown table.
"""
import argparse
import os
import statistics
import sys
import tempfile
import time

sys.path.insert(0, '.')

import numpy as np  # noqa: E402
import torch  # noqa: E402
from PIL import Image  # noqa: E402


def write_jpegs(root, n, h=480, w=640):
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    files = []
    for i in range(n):
        rng = np.random.RandomState(i)
        img = np.zeros((h, w, 3))
        for c in range(3):
            fy, fx, ph = rng.uniform(0.01, 0.2, 3)
            img[:, :, c] = 127 + 110 * np.sin(fy * yy + ph) * np.cos(fx * xx)
        img += rng.uniform(-12, 12, (h, w, 3))
        f = os.path.join(root, 'bench_%05d.jpg' % i)
        Image.fromarray(np.clip(img, 0, 255).astype(np.uint8)).save(
            f, quality=90)
        files.append(f)
    return files


def make_dataset(files, batch, T, vocab, seed):
    from sat_amd.data.dataset import DataSet
    rng = np.random.RandomState(seed)
    n = len(files)
    words = rng.randint(1, vocab, (n, T)).astype(np.int32)
    masks = np.ones((n, T), dtype=np.float32)
    return DataSet(list(range(n)), files, batch, words, masks, True, True)


def sync():
    torch.cuda.synchronize()


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--images', type=int, default=512)
    p.add_argument('--batch', type=int, default=32)
    p.add_argument('--threads', default='4,8,16')
    p.add_argument('--repeats', type=int, default=3)
    p.add_argument('--out', default=None)
    args = p.parse_args()
    if not torch.cuda.is_available():
        sys.exit('bench_input.py measures on the GPU; none found')
    thread_counts = [int(t) for t in args.threads.split(',')]

    from config import Config
    from sat_amd import ops
    from sat_amd.data.pipeline import BatchPrefetcher, ImagePrep, decode_u8
    from sat_amd.models.base_model import BaseModel

    cfg = Config()
    cfg.phase = 'train'
    cfg.train_cnn = False
    cfg.synthetic_data = False
    cfg.batch_size = args.batch
    cfg.device = 'cuda'
    torch.manual_seed(cfg.seed)
    np.random.seed(cfg.seed)
    rows = []

    def report(name, value):
        rows.append((name, value))
        print('%-58s %s' % (name, value), flush=True)

    with tempfile.TemporaryDirectory() as root:
        files = write_jpegs(root, args.images)
        data = make_dataset(files, args.batch, cfg.max_caption_length,
                            cfg.vocabulary_size, 0)
        model = BaseModel(cfg)
        loader = model.image_loader
        nb = data.num_batches

        # 1. the synchronous host path, per batch
        def host_batch(fs):
            x = model._images_to_device(loader.load_images(fs))
            return x.to(torch.bfloat16).contiguous(
                memory_format=torch.channels_last)
        host_batch(files[:args.batch])
        sync()
        times = []
        for b in range(min(nb, 8)):
            fs = files[b * args.batch:(b + 1) * args.batch]
            t0 = time.perf_counter()
            host_batch(fs)
            sync()
            times.append(time.perf_counter() - t0)
        report('host path, ms per batch of %d (median of %d)'
               % (args.batch, len(times)),
               '%.1f' % (statistics.median(times) * 1e3))

        # 2. the pipeline alone
        prep = ImagePrep(loader.mean, loader.image_shape, model.device,
                         torch.bfloat16)
        for threads in thread_counts:
            pre = BatchPrefetcher(data, loader, prep, threads,
                                  cfg.prefetch_batches)
            for _ in pre:           # warm-up epoch
                pass
            data.reset()
            sync()
            t0 = time.perf_counter()
            for _ in pre:
                pass
            sync()
            dt = time.perf_counter() - t0
            data.reset()
            report('pipeline alone, %2d threads: batches/s (images/s)'
                   % threads, '%.1f (%.0f)' % (nb / dt,
                                               nb * args.batch / dt))

        # 3. the kernel alone, one batch
        arrays = [decode_u8(f) for f in files[:args.batch]]
        packed, desc, tables = prep._layout(arrays)
        dev = [torch.from_numpy(a).to(model.device)
               for a in (packed, desc, tables)]
        for _ in range(5):
            ops.resize_normalize_u8(dev[0], dev[1], dev[2], prep.mean, 224,
                                    224, torch.bfloat16)
        sync()
        kt = []
        for _ in range(25):
            e0, e1 = torch.cuda.Event(True), torch.cuda.Event(True)
            e0.record()
            ops.resize_normalize_u8(dev[0], dev[1], dev[2], prep.mean, 224,
                                    224, torch.bfloat16)
            e1.record()
            e1.synchronize()
            kt.append(e0.elapsed_time(e1))
        report('resize kernel, batch of %d 640x480 -> 224x224 bf16: '
               'us (median of 25)' % args.batch,
               '%.1f' % (statistics.median(kt) * 1e3))

        # 4. real-file training, knobs off and on
        # (a model of its own per setting: the captured step keeps the
        # input form of the first batch it saw)
        import copy
        cfg_on = copy.copy(cfg)
        best = max(thread_counts)
        cfg_on.num_loader_threads = best
        cfg_on.device_image_prep = True
        torch.manual_seed(cfg.seed)
        model_on = BaseModel(cfg_on)

        def train_epoch(model):
            sync()
            t0 = time.perf_counter()
            for fs, sent, mask in model._batches(data):
                images = model._load_batch(fs)
                sent = torch.as_tensor(sent, dtype=torch.int64).to(
                    model.device)
                mask = torch.as_tensor(mask, dtype=torch.float32).to(
                    model.device)
                model.train_step(images, sent, mask)
            sync()
            dt = time.perf_counter() - t0
            data.reset()
            return nb * args.batch / dt

        train_epoch(model)          # capture + warm-up
        train_epoch(model_on)
        off, on = [], []
        for _ in range(args.repeats):
            off.append(train_epoch(model))
            on.append(train_epoch(model_on))
        report('train, knobs off: images/s (each of %d runs)'
               % args.repeats, ', '.join('%.0f' % v for v in off))
        report('train, %d threads + device prep: images/s (each run)'
               % best, ', '.join('%.0f' % v for v in on))

    if args.out:
        with open(args.out, 'w') as f:
            f.write('| measurement | value |\n|---|---|\n')
            for name, value in rows:
                f.write('| %s | %s |\n' % (name, value))


if __name__ == '__main__':
    main()
