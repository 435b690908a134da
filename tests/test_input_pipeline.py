"""BatchPrefetcher and the pipeline knobs through BaseModel, on the CPU:
same batches, same image bits, same losses, no thread left behind."""

import threading

import numpy as np
import pytest
import torch

from _pipeline_files import Recorder, file_config, write_images
from sat_amd.data.dataset import (DataSet, prepare_eval_data,
                                  prepare_train_data)
from sat_amd.data.image_loader import ImageLoader
from sat_amd.data.pipeline import BatchPrefetcher, ImagePrep
from sat_amd.models.base_model import BaseModel

SIZES = [(48, 64), (37, 53), (60, 40), (30, 30), (64, 48), (33, 71),
         (50, 50)]


def _dataset(files, batch_size, is_train=True):
    n = len(files)
    if not is_train:
        return DataSet(list(range(n)), files, batch_size)
    words = np.arange(n * 5, dtype=np.int32).reshape(n, 5)
    masks = np.ones((n, 5), dtype=np.float32)
    return DataSet(list(range(n)), files, batch_size, words, masks,
                   True, True)


def _plain_epochs(files, batch_size, epochs, seed):
    np.random.seed(seed)
    data = _dataset(files, batch_size)
    seen = []
    for _ in range(epochs):
        for _ in range(data.num_batches):
            seen.append(data.next_batch())
        data.reset()
    return seen


@pytest.fixture
def files(tmp_path):
    return write_images(str(tmp_path / 'img'), SIZES, ext='png')


@pytest.mark.parametrize('with_prep', [False, True])
def test_same_batches_as_the_plain_loop(files, with_prep):
    loader = ImageLoader(None, (32, 40, 3))
    want = _plain_epochs(files, 3, 2, seed=5)       # 7 files: 3 + 3 + 1(+2)
    np.random.seed(5)
    data = _dataset(files, 3)
    prep = ImagePrep(loader.mean, loader.image_shape) if with_prep else None
    pre = BatchPrefetcher(data, loader, prep, threads=3, depth=2)
    got = []
    for _ in range(2):
        for batch, images in pre:
            got.append(batch)
            ref = loader.load_images(batch[0])
            if with_prep:
                assert torch.is_tensor(images)
                images = images.permute(0, 2, 3, 1).numpy()
            assert images.dtype == np.float32
            assert np.array_equal(images, ref)
        data.reset()
    assert len(got) == len(want) == 6
    for (f1, s1, m1), (f2, s2, m2) in zip(got, want):
        assert list(f1) == list(f2)
        assert np.array_equal(s1, s2) and np.array_equal(m1, m2)
    # the random stream stands where the plain loop leaves it
    state = np.random.get_state()[1].copy()
    _plain_epochs(files, 3, 2, seed=5)
    assert np.array_equal(state, np.random.get_state()[1])


def test_never_further_ahead_than_depth(files):
    loader = ImageLoader(None, (8, 8, 3))
    data = _dataset(files, 1, is_train=False)       # 7 batches
    pre = BatchPrefetcher(data, loader, None, threads=2, depth=2)
    for i, (batch, _) in enumerate(pre):
        assert list(batch) == [files[i]]
        assert data.current_idx == min(i + 1 + 2, 7)
    assert not data.has_next_batch()


def test_unreadable_file_raises_at_its_own_batch(files, tmp_path):
    bad = str(tmp_path / 'broken.jpg')
    with open(bad, 'wb') as f:
        f.write(b'not an image')
    listed = files[:4] + [bad] + files[4:6]          # batch 2 of 0..3
    before = set(threading.enumerate())
    data = _dataset(listed, 2, is_train=False)
    loader = ImageLoader(None, (8, 8, 3))
    pre = BatchPrefetcher(data, loader, ImagePrep(loader.mean, (8, 8, 3)),
                          threads=2, depth=3)
    done = []
    with pytest.raises(Exception) as err:
        for batch, _ in pre:
            done.append(list(batch))
    assert done == [listed[0:2], listed[2:4]]
    assert 'broken.jpg' in str(err.value) or 'identify' in str(err.value)
    assert set(threading.enumerate()) <= before


@pytest.mark.parametrize('how', ['exhaust', 'break', 'close'])
def test_no_thread_survives(files, how):
    before = set(threading.enumerate())
    loader = ImageLoader(None, (8, 8, 3))
    data = _dataset(files, 2, is_train=False)
    pre = BatchPrefetcher(data, loader, None, threads=4, depth=2)
    if how == 'exhaust':
        assert len(list(pre)) == data.num_batches
    elif how == 'break':
        for _ in pre:
            assert len(set(threading.enumerate()) - before) >= 1
            break
    else:
        it = iter(pre)
        next(it)
        assert len(set(threading.enumerate()) - before) >= 1
        pre.close()
    assert set(threading.enumerate()) <= before


def test_thread_count_is_capped(files):
    data = _dataset(files, 2, is_train=False)
    pre = BatchPrefetcher(data, ImageLoader(None, (8, 8, 3)), None,
                          threads=1000, depth=1)
    assert pre.threads == 16


def _train_and_eval(cfg_factory, tmp_path, threads, prep):
    """Two train steps and one eval batch on JPEG files -> (images that
    reached compute_contexts, losses, eval results)."""
    cfg = file_config(cfg_factory, tmp_path, SIZES[:4], SIZES[4:6])
    cfg.num_epochs = 1
    cfg.batch_size = 2
    cfg.save_dir = str(tmp_path / 'models') + '/'
    cfg.num_loader_threads = threads
    cfg.device_image_prep = prep
    np.random.seed(11)
    torch.manual_seed(11)
    data = prepare_train_data(cfg)
    m = BaseModel(cfg)
    rec = Recorder(m.model)
    losses = []
    step = m.train_step

    def train_step(images, sentences, masks):
        out = step(images, sentences, masks)
        losses.append(out['total_loss'].detach().item())
        return out
    m.train_step = train_step
    m.train(data)
    assert m.global_step == 2

    cfg.phase = 'eval'
    coco, ds, vocab = prepare_eval_data(cfg)
    ev = BaseModel(cfg)
    ev.load()
    rec_eval = Recorder(ev.model)
    ev.eval(coco, ds, vocab)
    assert len(rec_eval.images) == 1
    return rec.images + rec_eval.images, losses, m, ev


def test_knobs_change_no_bit(tiny_config, tmp_path):
    import copy
    before = set(threading.enumerate())
    off = _train_and_eval(copy.copy(tiny_config), tmp_path / 'off', 0,
                          False)
    on = _train_and_eval(copy.copy(tiny_config), tmp_path / 'on', 2, True)
    assert on[2]._prep is not None and on[3]._prep is not None
    assert off[2]._prep is None
    assert len(off[0]) == len(on[0]) == 3
    for a, b in zip(off[0], on[0]):
        assert a.shape == b.shape and a.dtype == b.dtype
        assert torch.equal(a, b)
    assert off[1] == on[1] and len(on[1]) == 2
    # (tqdm keeps a monitor thread of its own)
    assert not [t for t in set(threading.enumerate()) - before
                if t.name.startswith('sat-loader')]


def test_threads_without_prep_and_synthetic(tiny_config):
    """Threads alone overlap the float path; the synthetic loader has no
    uint8 source and never gets an ImagePrep."""
    cfg = tiny_config
    cfg.num_loader_threads = 2
    cfg.device_image_prep = True
    np.random.seed(3)
    torch.manual_seed(3)
    data = prepare_train_data(cfg)
    m = BaseModel(cfg)
    rec = Recorder(m.model)
    m.train(data)
    assert m._image_prep() is None
    assert m.global_step == data.num_batches == len(rec.images)


def test_mean_image_keeps_the_pipeline_off(tiny_config):
    cfg = tiny_config
    cfg.synthetic_data = False
    cfg.device_image_prep = True
    m = BaseModel(cfg)
    assert m._image_prep() is not None
    m._prep = None
    m.image_loader.mean = np.zeros((224, 224, 3), np.float32)
    assert m._image_prep() is None


def test_flags_reach_the_config():
    from config import Config
    from main import build_config, build_parser
    cfg = Config()
    assert cfg.num_loader_threads == 0
    assert cfg.prefetch_batches == 2
    assert cfg.device_image_prep is False
    cfg = build_config(build_parser().parse_args([]))
    assert cfg.num_loader_threads == 0 and cfg.device_image_prep is False
    cfg = build_config(build_parser().parse_args(
        ['--loader_threads', '8', '--device_image_prep']))
    assert cfg.num_loader_threads == 8 and cfg.device_image_prep is True
