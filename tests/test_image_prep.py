"""The integer twin of the resize kernel and ImagePrep's tables against
Pillow and ImageLoader, on the CPU: every byte equal."""

import warnings

import numpy as np
import pytest
import torch
from PIL import Image

from sat_amd.data import pipeline
from sat_amd.data.image_loader import ILSVRC_2012_MEAN, ImageLoader
from sat_amd.data.pipeline import ImagePrep

# (H, W): down, up, identity, one tap, many taps, thin but inside the gate
SHAPES = [(480, 640), (427, 640), (640, 427), (224, 224), (448, 448),
          (100, 150), (150, 100), (300, 200), (37, 53), (1, 1), (2, 3),
          (223, 225), (225, 223), (1200, 1600), (3000, 4000), (7, 3000),
          (9, 2000), (500, 9), (3000, 100)]
OUT_SIZES = [(224, 224), (16, 24), (7, 5)]


def _rand(h, w, seed=0):
    return np.random.RandomState(seed + 7 * h + w).randint(
        0, 256, (h, w, 3)).astype(np.uint8)


def _pil(a, oh, ow):
    return np.asarray(Image.fromarray(a).resize((ow, oh), Image.BILINEAR))


def _resized_u8(arrays, oh, ow):
    """ImagePrep with a zero mean -> the resized bytes, [N,OH,OW,3]."""
    prep = ImagePrep(np.zeros(3, np.float32), (oh, ow, 3))
    out = prep(arrays)
    assert out.shape == (len(arrays), 3, oh, ow)
    assert out.is_contiguous(memory_format=torch.channels_last)
    vals = out.permute(0, 2, 3, 1).numpy()
    assert np.array_equal(vals, np.round(vals))
    return vals.astype(np.uint8), prep


@pytest.fixture(scope='module')
def images():
    return [_rand(h, w) for h, w in SHAPES]


@pytest.mark.parametrize('oh,ow', OUT_SIZES)
def test_twin_equals_pillow_mixed_batch(images, oh, ow):
    got, prep = _resized_u8(images, oh, ow)
    assert prep.device_tables is True
    for n, a in enumerate(images):
        want = _pil(a, oh, ow)
        assert np.array_equal(got[n], want), \
            '%dx%d -> %dx%d: %d bytes differ' % (
                a.shape[0], a.shape[1], oh, ow, int((got[n] != want).sum()))


@pytest.mark.parametrize('value', [0, 255])
def test_twin_constant_images(value):
    arrays = [np.full((h, w, 3), value, np.uint8)
              for h, w in [(480, 640), (37, 53), (1, 1)]]
    got, _ = _resized_u8(arrays, 224, 224)
    assert (got == value).all()


def test_float_output_equals_image_loader(tmp_path):
    files = []
    for i, (h, w) in enumerate([(48, 64), (37, 53), (224, 224), (300, 200)]):
        f = str(tmp_path / ('im%d.png' % i))
        Image.fromarray(_rand(h, w)).save(f)
        files.append(f)
    f = str(tmp_path / 'im.jpg')
    Image.fromarray(_rand(120, 160)).save(f)
    files.append(f)
    loader = ImageLoader(None, (224, 224, 3))
    want = loader.load_images(files)
    prep = ImagePrep(loader.mean, loader.image_shape)
    got = prep([pipeline.decode_u8(f) for f in files])
    assert got.dtype == torch.float32
    assert np.array_equal(got.permute(0, 2, 3, 1).numpy(), want)


def test_images_outside_the_gate_take_the_host_resize(monkeypatch):
    thin = _rand(2000, 16)
    huge_side = _rand(3, 8200)          # aspect and size both outside
    inside = _rand(37, 53)
    calls = []
    real = ImagePrep._pil_resize

    def spy(self, arr):
        calls.append(arr.shape[:2])
        return real(self, arr)

    got, prep = _resized_u8([inside], 224, 224)     # runs the self-check
    monkeypatch.setattr(ImagePrep, '_pil_resize', spy)
    out = prep([thin, inside, huge_side]).permute(0, 2, 3, 1).numpy()
    assert calls == [(2000, 16), (3, 8200)]
    for n, a in enumerate([thin, inside, huge_side]):
        assert np.array_equal(out[n].astype(np.uint8), _pil(a, 224, 224))


def test_self_check_disables_device_tables(monkeypatch):
    real = Image.Image.resize

    def other_pillow(self, size, *args, **kw):
        out = np.asarray(real(self, size, *args, **kw)).copy()
        out[0, 0, 0] ^= 1
        return Image.fromarray(out)

    monkeypatch.setattr(Image.Image, 'resize', other_pillow)
    prep = ImagePrep(ILSVRC_2012_MEAN, (224, 224, 3))
    a = _rand(100, 150)
    with pytest.warns(UserWarning, match='Pillow'):
        got = prep([a])
    assert prep.device_tables is False
    with warnings.catch_warnings():
        warnings.simplefilter('error')              # it warns once
        got2 = prep([a])
    want = np.asarray(Image.fromarray(a).resize((224, 224), Image.BILINEAR),
                      dtype=np.float32) - ILSVRC_2012_MEAN
    assert np.array_equal(got.permute(0, 2, 3, 1).numpy()[0], want)
    assert torch.equal(got, got2)


def test_mean_image_is_rejected():
    with pytest.raises(ValueError):
        ImagePrep(np.zeros((224, 224, 3), np.float32))


def test_axis_tables_are_cached_per_size(images):
    prep = ImagePrep(ILSVRC_2012_MEAN, (16, 24, 3))
    prep([images[0], images[0], images[1]])          # 480x640, 427x640
    keys = set(prep._axis) - {(53, 24), (37, 16)}    # the self-check's
    assert keys == {(640, 24), (480, 16), (427, 16)}
