"""Conv2d keeps the cast weight and bias of a frozen layer across forwards
(sat_amd/models/nn.py, Conv2d._cast_operands)."""

import pytest
import torch

from config import Config
from sat_amd.models.nn import NN, Conv2d


def _dtypes():
    out = [torch.float32]
    try:
        torch.nn.functional.conv2d(
            torch.zeros(1, 3, 4, 4, dtype=torch.bfloat16),
            torch.zeros(2, 3, 3, 3, dtype=torch.bfloat16), padding=1)
        out.append(torch.bfloat16)
    except RuntimeError:
        pass
    return out


def _layer(frozen=True, cache=True):
    cfg = Config()
    cfg.phase = 'train'
    cfg.cache_frozen_conv_cast = cache
    torch.manual_seed(0)
    conv = Conv2d(NN(cfg), 3, 8)
    with torch.no_grad():
        conv.bias.copy_(torch.randn(8))
    for p in conv.parameters():
        p.requires_grad_(not frozen)
    return conv


@pytest.mark.parametrize('dtype', _dtypes())
def test_cached_operands_are_reused(dtype):
    conv = _layer()
    with torch.no_grad():
        w1, b1 = conv._cast_operands(dtype)
        w2, b2 = conv._cast_operands(dtype)
    assert w1.dtype == dtype and b1.dtype == dtype
    assert w1.data_ptr() == w2.data_ptr()
    assert b1.data_ptr() == b2.data_ptr()
    x = torch.randn(2, 3, 6, 6).to(dtype)
    with torch.no_grad():
        conv(x)
        w3, _ = conv._cast_operands(dtype)
        conv(x)
        w4, _ = conv._cast_operands(dtype)
    assert w3.data_ptr() == w4.data_ptr() == w1.data_ptr()


@pytest.mark.parametrize('dtype', _dtypes())
def test_cache_refreshed_after_in_place_write(dtype):
    conv = _layer()
    with torch.no_grad():
        w1, b1 = conv._cast_operands(dtype)
        w1, b1 = w1.clone(), b1.clone()
        new_w = torch.randn_like(conv.weight)
        # a write through .data leaves weight._version where it was
        conv.weight.data.copy_(new_w)
        w2, b2 = conv._cast_operands(dtype)
        assert torch.equal(w2, new_w.to(dtype))
        assert not torch.equal(w2, w1)
        assert torch.equal(b2, b1)
        new_b = torch.randn_like(conv.bias)
        conv.bias.data.copy_(new_b)
        _, b3 = conv._cast_operands(dtype)
        assert torch.equal(b3, new_b.to(dtype))
        # another dtype is another entry
        other = torch.float64
        w4, _ = conv._cast_operands(other)
        assert w4.dtype == other


def test_cache_not_used_when_trainable_or_grad_enabled():
    dtype = torch.float64           # a real cast on every platform
    conv = _layer(frozen=False)
    with torch.no_grad():
        w1, _ = conv._cast_operands(dtype)
        w2, _ = conv._cast_operands(dtype)
    assert w1.data_ptr() != w2.data_ptr()
    assert getattr(conv, '_cast_cache', None) is None
    w3, _ = conv._cast_operands(dtype)          # grad mode: in the graph
    assert w3.requires_grad and w3.grad_fn is not None
    frozen = _layer(frozen=True)
    a, _ = frozen._cast_operands(dtype)         # grad mode, frozen layer
    b, _ = frozen._cast_operands(dtype)
    assert a.data_ptr() != b.data_ptr()
    assert getattr(frozen, '_cast_cache', None) is None


@pytest.mark.parametrize('dtype', _dtypes())
def test_outputs_equal_uncached_path(dtype):
    cached, plain = _layer(cache=True), _layer(cache=False)
    assert torch.equal(cached.weight, plain.weight)
    x = torch.randn(2, 3, 9, 7).to(dtype)
    with torch.no_grad():
        y0 = plain(x)
        y1 = cached(x)
        y2 = cached(x)                          # from the cache
        assert getattr(plain, '_cast_cache', None) is None
        assert getattr(cached, '_cast_cache', None) is not None
        assert torch.equal(y0, y1) and torch.equal(y0, y2)
        cached.weight.data.mul_(2.0)
        plain.weight.data.mul_(2.0)
        assert torch.equal(plain(x), cached(x))
