"""Opt-in input pipeline: threaded decode, on-device resize + normalise.

Two pieces, both off by default (config.num_loader_threads,
config.device_image_prep):

  * `ImagePrep` turns a list of decoded uint8 HWC images of any sizes into
    the [N,3,OH,OW] channels_last tensor the encoder reads, on the model's
    device and in its compute dtype.  The images are packed into a pinned
    staging buffer together with a descriptor table and Pillow's
    resampling coefficients (built here in float64, cached per axis
    size), copied in one non-blocking transfer and resized, mean-
    subtracted and cast by one kernel (ops.resize_normalize_u8).  The
    result has the bits of `ImageLoader.load_images` followed by the
    model's cast, so a model fed this way computes what it computed
    before.
  * `BatchPrefetcher` walks a DataSet up to `depth` batches ahead of the
    consumer and decodes the files of those batches on worker threads.

The coefficient arithmetic is Pillow's (`precompute_coeffs` and
`normalize_coeffs_8bpc` of its Resample.c) for the bilinear filter.  Very
long thin images, where Pillow's result follows another pass order, and
images a Pillow of different arithmetic would resize differently are
resized on the host and pass through the kernel as the identity case.
"""

import warnings
from collections import deque
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch
from PIL import Image

from .. import ops

MAX_THREADS = 16
MAX_SIDE = 8192         # larger images are resized on the host
MAX_ASPECT = 16         # so are images longer than this times their width
PRECISION_BITS = 22     # Pillow: 32 - 8 - 2

_DESC_COLS = 8


def axis_table(in_size, out_size):
    """Pillow's bilinear coefficients for one axis -> (int32 table, ksize).

    table = first source index [out_size], tap count [out_size], then
    out_size x ksize coefficients in Q22, zero past the tap count."""
    scale = float(in_size) / float(out_size)
    filterscale = max(scale, 1.0)
    support = 1.0 * filterscale
    ksize = int(np.ceil(support)) * 2 + 1
    ss = 1.0 / filterscale
    center = (np.arange(out_size, dtype=np.float64) + 0.5) * scale
    xmin = np.maximum((center - support + 0.5).astype(np.int64), 0)
    xmax = np.minimum((center + support + 0.5).astype(np.int64), in_size)
    count = xmax - xmin
    w = np.zeros((out_size, ksize), dtype=np.float64)
    ww = np.zeros(out_size, dtype=np.float64)
    for k in range(ksize):          # summed tap by tap, as Pillow does
        x = np.abs((k + xmin - center + 0.5) * ss)
        wk = np.where((x < 1.0) & (k < count), 1.0 - x, 0.0)
        w[:, k] = wk
        ww += wk
    ww[ww == 0.0] = 1.0
    w /= ww[:, None]
    q = w * float(1 << PRECISION_BITS)
    coef = np.where(q < 0, -0.5 + q, 0.5 + q).astype(np.int32)
    table = np.concatenate([xmin.astype(np.int32), count.astype(np.int32),
                            coef.reshape(-1)])
    return table, ksize


def decode_u8(image_file):
    """File -> uint8 [H,W,3] RGB, the decode half of ImageLoader."""
    return np.asarray(Image.open(image_file).convert('RGB'))


class _Slot(object):
    """One pinned staging buffer, its device twin and the event after
    which the host side may be written again."""

    def __init__(self):
        self.host = None
        self.dev = None
        self.event = None


class ImagePrep(object):
    def __init__(self, mean, image_shape=(224, 224, 3), device='cpu',
                 dtype=torch.float32):
        mean = np.asarray(mean, dtype=np.float32)
        if mean.shape != (3,):
            raise ValueError('ImagePrep takes a per-channel mean')
        self.out_h, self.out_w = int(image_shape[0]), int(image_shape[1])
        self.device = torch.device(device)
        self.dtype = dtype
        self.mean = torch.from_numpy(mean.copy()).to(self.device)
        self._axis = {}                 # (in, out) -> (table, ksize)
        self._slots = [_Slot(), _Slot()]
        self._turn = 0
        self.device_tables = None       # set by the self-check

    # ---- tables ----

    def _axis_table(self, in_size, out_size):
        key = (in_size, out_size)
        if key not in self._axis:
            self._axis[key] = axis_table(in_size, out_size)
        return self._axis[key]

    def _pil_resize(self, arr):
        return np.asarray(Image.fromarray(arr).resize(
            (self.out_w, self.out_h), Image.BILINEAR))

    def _self_check(self):
        """The twin against the installed Pillow on one fixed image; a
        Pillow of other arithmetic sends every image through the host
        resize."""
        arr = np.random.RandomState(0).randint(
            0, 256, (37, 53, 3)).astype(np.uint8)
        packed, desc, tables = self._layout([arr])
        got = ops.F.resize_normalize_u8(
            torch.from_numpy(packed), torch.from_numpy(desc),
            torch.from_numpy(tables), torch.zeros(3), self.out_h,
            self.out_w)
        got = got.permute(0, 2, 3, 1)[0].numpy().astype(np.uint8)
        self.device_tables = bool(np.array_equal(got, self._pil_resize(arr)))
        if not self.device_tables:
            warnings.warn('ImagePrep: the installed Pillow resizes '
                          'differently from the device tables; images '
                          'are resized on the host')

    def _takes(self, h, w):
        return (self.device_tables and max(h, w) <= MAX_SIDE
                and max(h, w) <= MAX_ASPECT * min(h, w))

    def _layout(self, arrays, pack=True):
        """-> (packed uint8, desc [N,8] int64, tables int32); without
        `pack`, the number of pixel bytes in place of the packed
        buffer, for `_pack_into`."""
        desc = np.zeros((len(arrays), _DESC_COLS), dtype=np.int64)
        parts, where, size, off = [], {}, 0, 0
        for n, a in enumerate(arrays):
            h, w = a.shape[0], a.shape[1]
            row = [off, h, w]
            for key in ((w, self.out_w), (h, self.out_h)):
                if key not in where:
                    table, ksize = self._axis_table(*key)
                    where[key] = (size, ksize)
                    parts.append(table)
                    size += table.size
                row.extend(where[key])
            desc[n, :7] = row
            off += h * w * 3
        tables = np.concatenate(parts)
        if not pack:
            return off, desc, tables
        packed = np.empty(off, dtype=np.uint8)
        self._pack_into(packed, arrays, desc)
        return packed, desc, tables

    @staticmethod
    def _pack_into(packed, arrays, desc):
        for n, a in enumerate(arrays):
            packed[desc[n, 0]:desc[n, 0] + a.size] = a.reshape(-1)

    # ---- the batch ----

    def __call__(self, arrays):
        """uint8 [H,W,3] arrays -> [N,3,OH,OW] channels_last on the
        device, in the compute dtype."""
        if self.device_tables is None:
            self._self_check()
        arrays = [np.ascontiguousarray(a, dtype=np.uint8) for a in arrays]
        for a in arrays:
            if a.ndim != 3 or a.shape[2] != 3 or a.size == 0:
                raise ValueError('ImagePrep takes uint8 [H,W,3] images')
        arrays = [a if self._takes(a.shape[0], a.shape[1])
                  else self._pil_resize(a) for a in arrays]
        if self.device.type != 'cuda':
            packed, desc, tables = self._layout(arrays)
            return ops.resize_normalize_u8(
                torch.from_numpy(packed), torch.from_numpy(desc),
                torch.from_numpy(tables), self.mean, self.out_h,
                self.out_w, self.dtype)

        # one staging buffer: descriptors, tables, pixels (packed in
        # place: one pass over the pixels on the host)
        n_pix, desc, tables = self._layout(arrays, pack=False)
        n_desc = desc.nbytes
        n_tab = tables.nbytes
        pix0 = (n_desc + n_tab + 15) // 16 * 16
        total = pix0 + n_pix
        slot = self._slots[self._turn]
        self._turn ^= 1
        if slot.event is not None:
            slot.event.synchronize()    # its last copy has left the host
        if slot.host is None or slot.host.numel() < total:
            cap = max(total * 5 // 4, 1 << 20)
            slot.host = torch.empty(cap, dtype=torch.uint8,
                                    pin_memory=True)
            slot.dev = torch.empty(cap, dtype=torch.uint8,
                                   device=self.device)
            slot.event = torch.cuda.Event()
        host = slot.host.numpy()
        host[:n_desc] = desc.reshape(-1).view(np.uint8)
        host[n_desc:n_desc + n_tab] = tables.view(np.uint8)
        self._pack_into(host[pix0:total], arrays, desc)
        slot.dev[:total].copy_(slot.host[:total], non_blocking=True)
        slot.event.record()
        dev = slot.dev
        return ops.resize_normalize_u8(
            dev[pix0:total],
            dev[:n_desc].view(torch.int64).reshape(-1, _DESC_COLS),
            dev[n_desc:n_desc + n_tab].view(torch.int32),
            self.mean, self.out_h, self.out_w, self.dtype)


class BatchPrefetcher(object):
    """One epoch of `dataset` per iteration: yields (batch, images) with
    `batch` what `dataset.next_batch()` returned and `images` what the
    model's loader would have made of its files: the tensor of
    `prep(decoded files)`, or without `prep` the float32 [N,H,W,3] array
    of `image_loader.load_images`.

    `next_batch()` runs on the consuming thread, in order, at most `depth`
    batches ahead and never past the end of the epoch, so the dataset and
    the global numpy random stream advance exactly as in a plain loop; the
    caller still calls `reset()`.  Worker threads only turn files into
    arrays.  A file that fails raises at its own batch.  The threads are
    gone when the iteration ends, however it ends, and after `close()`."""

    def __init__(self, dataset, image_loader, prep=None, threads=1,
                 depth=2):
        self.dataset = dataset
        self.image_loader = image_loader
        self.prep = prep
        self.threads = max(1, min(int(threads), MAX_THREADS))
        self.depth = max(0, int(depth))
        self._pool = None

    def _load(self, image_file):
        if self.prep is not None:
            return decode_u8(image_file)
        return self.image_loader.load_image(image_file)

    def _submit(self, pool):
        batch = self.dataset.next_batch()
        files = batch[0] if self.dataset.is_train else batch
        return batch, [pool.submit(self._load, f) for f in files]

    def __iter__(self):
        self.close()
        pool = ThreadPoolExecutor(max_workers=self.threads,
                                  thread_name_prefix='sat-loader')
        self._pool = pool
        try:
            total = self.dataset.num_batches
            ahead = deque()
            taken = 0
            for _ in range(total):
                while taken < total and len(ahead) <= self.depth:
                    ahead.append(self._submit(pool))
                    taken += 1
                batch, futures = ahead.popleft()
                arrays = [f.result() for f in futures]
                if self.prep is not None:
                    yield batch, self.prep(arrays)
                else:
                    yield batch, np.stack(arrays, axis=0)
        finally:
            self._shutdown(pool)

    def _shutdown(self, pool):
        pool.shutdown(wait=True, cancel_futures=True)
        if self._pool is pool:
            self._pool = None

    def close(self):
        if self._pool is not None:
            self._shutdown(self._pool)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
