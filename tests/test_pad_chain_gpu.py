"""GPU tests: the "emit padded" mode of the frozen-VGG producers.

Each producer (conv3_fwd, glds, glds64, 8-phase single pass, 8-phase
split-K + combine, maxpool) is run twice on the same input: unpadded, and
with emit_pad into a caller buffer pre-filled with a bf16 NaN sentinel.
The interior of the padded output must equal the unpadded output BITWISE
(same kernel, same accumulation order: no tolerance), the 1-px border must
be +0 in every bit, and no sentinel may survive.

Shapes are the smallest that can still go wrong: H != W (a swap shows),
B >= 2 with M = B*H*W no multiple of the 128- / 256-row tile (a tile spans
an image boundary and has a clamped tail), a Cout that is no multiple of
the 128-column tile for glds, odd H and W for the pool.
"""

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = 'cuda'
CL = torch.channels_last

# (B, H, W): M = 280 (two 128-row tiles + 24, image boundary at row 140
# inside tile 1); M = 288 (the 256-row tile's case: boundary at 144, 32
# rows in tile 1); M = 105 (three images inside one tile, clamped tail)
_SHAPES = [(2, 10, 14), (2, 12, 12), (3, 5, 7)]


def _nhwc(*shape, scale=1.0):
    return (torch.randn(*shape) * scale).to(DEV, torch.bfloat16) \
        .contiguous(memory_format=CL)


def _sentinel(B, C, H, W):
    """[B,C,H+2,W+2] channels-last buffer, every element a bf16 NaN"""
    buf = torch.empty(B, C, H + 2, W + 2, dtype=torch.bfloat16,
                      device=DEV, memory_format=CL)
    buf.fill_(float('nan'))
    assert torch.isnan(buf).all()
    return buf


def _bits(t):
    return t.view(torch.int16)


def _check_padded(yp, buf, y0):
    """yp: padded result, buf: the sentinel buffer handed in, y0: the
    same kernel's unpadded result"""
    assert yp.data_ptr() == buf.data_ptr()          # written in place
    B, C, H, W = y0.shape
    assert tuple(yp.shape) == (B, C, H + 2, W + 2)
    assert yp.is_contiguous(memory_format=CL)
    assert not torch.isnan(yp).any(), 'sentinel left in the output'
    assert torch.equal(_bits(yp[:, :, 1:-1, 1:-1]), _bits(y0)), \
        'interior differs from the unpadded output'
    border = _bits(yp).clone()
    border[:, :, 1:-1, 1:-1] = 0
    assert not border.any(), 'border is not +0 everywhere'


def _conv_inputs(B, H, W, Cin, Cout, seed):
    from sat_amd import _C
    torch.manual_seed(seed)
    x = _nhwc(B, Cin, H, W)
    w = (torch.randn(Cout, Cin, 3, 3) * 0.05).to(DEV, torch.bfloat16)
    w_ohwi = w.permute(0, 2, 3, 1).contiguous().reshape(Cout, -1)
    b = (torch.randn(Cout) * 0.5).to(DEV, torch.bfloat16)
    return _C.pad1_nhwc(x), w_ohwi, b


@pytest.mark.parametrize('B,H,W', _SHAPES)
@pytest.mark.parametrize('Cout', [128, 136])
def test_glds_emit_pad(B, H, W, Cout):
    from sat_amd import _C
    xp, w, b = _conv_inputs(B, H, W, 64, Cout, 11)
    y0 = _C.conv_igemm_glds_fwd(xp, w, b, H, W, True)
    buf = _sentinel(B, Cout, H, W)
    yp = _C.conv_igemm_glds_fwd(xp, w, b, H, W, True, True, buf)
    _check_padded(yp, buf, y0)


@pytest.mark.parametrize('B,H,W', _SHAPES)
def test_glds64_emit_pad(B, H, W):
    from sat_amd import _C
    xp, w, b = _conv_inputs(B, H, W, 64, 64, 12)
    y0 = _C.conv_igemm_glds64_fwd(xp, w, b, H, W, True)
    buf = _sentinel(B, 64, H, W)
    yp = _C.conv_igemm_glds64_fwd(xp, w, b, H, W, True, True, buf)
    _check_padded(yp, buf, y0)


# split 0: the SPLIT=0 instantiation (the shape heuristic alone would
# pick split-K at these M).  split 2: the SPLIT=1 instantiation + the
# combine kernel, with two K slices — each scratch element is then
# 0 + a + b by fp32 atomics, which is the same value in either order, so
# the split route too is deterministic and compared bitwise.
@pytest.mark.parametrize('B,H,W', _SHAPES)
@pytest.mark.parametrize('split', [0, 2])
def test_8p_emit_pad(B, H, W, split):
    from sat_amd import _C
    xp, w, b = _conv_inputs(B, H, W, 64, 256, 13)
    y0 = _C.conv_igemm_8p_fwd(xp, w, b, H, W, True, False, None, split)
    buf = _sentinel(B, 256, H, W)
    yp = _C.conv_igemm_8p_fwd(xp, w, b, H, W, True, True, buf, split)
    _check_padded(yp, buf, y0)


def test_8p_split_override_matches_default_route():
    """the override only picks the instantiation: single pass, forced
    2-slice split-K and the default heuristic agree to bf16 rounding of
    the same fp32 sums (one bf16 ulp of the output range)"""
    from sat_amd import _C
    B, H, W = 2, 12, 12
    xp, w, b = _conv_inputs(B, H, W, 64, 256, 14)
    y_auto = _C.conv_igemm_8p_fwd(xp, w, b, H, W, True).float()
    for split in (0, 2):
        y = _C.conv_igemm_8p_fwd(xp, w, b, H, W, True, False, None,
                                 split).float()
        tol = y_auto.abs().max().item() * 2.0 ** -7
        assert (y - y_auto).abs().max().item() <= tol


@pytest.mark.parametrize('B,H,W', [(2, 7, 9), (2, 10, 14), (3, 5, 7)])
def test_maxpool_emit_pad(B, H, W):
    from sat_amd import _C
    torch.manual_seed(15)
    x = _nhwc(B, 64, H, W)
    y0 = _C.maxpool2x2_nhwc(x)
    Ho, Wo = (H + 1) // 2, (W + 1) // 2
    assert tuple(y0.shape) == (B, 64, Ho, Wo)
    buf = _sentinel(B, 64, Ho, Wo)
    yp = _C.maxpool2x2_nhwc(x, True, buf)
    _check_padded(yp, buf, y0)


@pytest.mark.parametrize('B,H,W', _SHAPES)
def test_conv3_fwd_emit_pad_writes_own_border(B, H, W):
    from sat_amd import _C
    torch.manual_seed(16)
    x = _nhwc(B, 3, H, W, scale=2.0)
    w = (torch.randn(64, 3, 3, 3) * 0.2).to(DEV, torch.bfloat16)
    b = (torch.randn(64) * 0.5).to(DEV, torch.bfloat16)
    y0 = _C.conv3_fwd(x, w, b, True, False)
    buf = _sentinel(B, 64, H, W)
    yp = _C.conv3_fwd(x, w, b, True, True, buf)
    _check_padded(yp, buf, y0)


def test_caller_output_is_checked():
    from sat_amd import _C
    B, H, W = 2, 10, 14
    xp, w, b = _conv_inputs(B, H, W, 64, 128, 17)
    swapped = torch.empty(B, 128, W + 2, H + 2, dtype=torch.bfloat16,
                          device=DEV, memory_format=CL)
    with pytest.raises(RuntimeError):
        _C.conv_igemm_glds_fwd(xp, w, b, H, W, True, True, swapped)
    unpadded = torch.empty(B, 128, H, W, dtype=torch.bfloat16,
                           device=DEV, memory_format=CL)
    with pytest.raises(RuntimeError):
        _C.conv_igemm_glds_fwd(xp, w, b, H, W, True, True, unpadded)
    nchw = torch.empty(B, 128, H + 2, W + 2, dtype=torch.bfloat16,
                       device=DEV)
    with pytest.raises(RuntimeError):
        _C.conv_igemm_glds_fwd(xp, w, b, H, W, True, True, nchw)
    f32 = torch.empty(B, 128, H + 2, W + 2, device=DEV,
                      memory_format=CL)
    with pytest.raises(RuntimeError):
        _C.maxpool2x2_nhwc(xp, True, f32)


# ---- model level ----

def _vgg(seed):
    from config import Config
    from sat_amd.models.encoders import VGG16
    from sat_amd.models.nn import NN
    cfg = Config()
    cfg.phase = 'train'
    cfg.train_cnn = False
    torch.manual_seed(seed)
    return VGG16(NN(cfg)).to(DEV).to(memory_format=CL)


def _count_calls(monkeypatch, names):
    """count calls of extension entry points (one kernel launch each)"""
    from sat_amd import _C
    counts = dict.fromkeys(names, 0)

    def wrap(name, fn):
        def counted(*a, **k):
            counts[name] += 1
            return fn(*a, **k)
        return counted
    for name in names:
        monkeypatch.setattr(_C, name, wrap(name, getattr(_C, name)))
    return counts


# (PAD_CHAIN, PAD_CHAIN_8P): the pad1_nhwc routing; the default chain,
# in which the single-pass 8-phase kernel still emits unpadded; the full
# chain, in which every producer emits padded
_OFF, _DEFAULT, _FULL = (False, False), (True, False), (True, True)


def _set_chain(monkeypatch, mode):
    from sat_amd.models import nn
    monkeypatch.setattr(nn, 'PAD_CHAIN', mode[0])
    monkeypatch.setattr(nn, 'PAD_CHAIN_8P', mode[1])


def test_vgg_forward_chain_on_equals_chain_off(monkeypatch):
    """VGG16.forward in bf16 at batch 16, 224^2 (conv4: M = 12544, exactly
    the 8-phase threshold; conv5: M = 3136, below the in-tree route, so the
    chain must end at conv4_3 without an unpad copy): contexts with the
    padded chain, default and full, bitwise equal to the pad1_nhwc
    routing."""
    # conv5 runs in the library at this batch, and its default split-K
    # solver sums with atomics: two runs of the SAME routing differ
    # there (measured 7.8e-3 on outputs up to 2.6, chain off against
    # chain off, while every layer up to pool4 was bitwise equal).  A
    # bitwise comparison needs the library's deterministic solvers, in
    # all arms alike.
    monkeypatch.setattr(torch.backends.cudnn, 'deterministic', True)
    vgg = _vgg(31)
    torch.manual_seed(32)
    images = _nhwc(16, 3, 224, 224, scale=50.0)
    counts = _count_calls(monkeypatch, ['pad1_nhwc'])
    pool4 = {}
    out, pads = {}, {}
    for mode in (_OFF, _DEFAULT, _FULL):
        hook = vgg._layers[-4].register_forward_hook(
            lambda mod, inp, y, mode=mode: pool4.__setitem__(mode, y.clone()))
        _set_chain(monkeypatch, mode)
        counts['pad1_nhwc'] = 0
        with torch.no_grad():
            out[mode] = vgg(images)
        pads[mode] = counts['pad1_nhwc']
        hook.remove()
    assert out[_OFF].shape == (16, 196, 512)
    assert torch.isfinite(out[_OFF].float()).all()
    assert tuple(pool4[_OFF].shape) == (16, 512, 14, 14)
    for mode in (_DEFAULT, _FULL):
        # the in-tree part of the forward, conv1_1 .. pool4
        assert torch.equal(_bits(pool4[mode]), _bits(pool4[_OFF])), mode
        same = torch.equal(_bits(out[mode]), _bits(out[_OFF]))
        ndiff = (_bits(out[mode]) != _bits(out[_OFF])).sum().item()
        maxd = (out[mode].float() - out[_OFF].float()).abs().max().item()
        print('contexts %s: %d of %d elements differ, max abs diff %.3e'
              % (mode, ndiff, out[mode].numel(), maxd))
        assert same, 'contexts differ between chain on and chain off'
    # chain off: the 8 pad passes of conv2_1..conv4_3.  Default chain: the
    # two behind the single-pass 8-phase conv3_1 / conv3_2 stay (conv4 at
    # M = 12544 runs split-K, whose combine kernel emits padded).  Full
    # chain: none.
    assert pads[_OFF] == 8
    assert pads[_DEFAULT] == 2
    assert pads[_FULL] == 0


def test_vgg_flagship_forward_pad_passes(monkeypatch):
    """Flagship batch 32.  Full chain: no pad1_nhwc launch in the frozen
    forward, whichever way conv5 is routed (the border launch that
    conv3_fwd used to make no longer exists in the extension at all), and
    with conv5 in-tree no library conv either.  Default chain: only the
    four passes behind the single-pass 8-phase convs (conv3_1, conv3_2,
    conv4_1, conv4_2) are left."""
    from sat_amd.models import nn
    vgg = _vgg(33)
    torch.manual_seed(34)
    images = _nhwc(32, 3, 224, 224, scale=50.0)
    counts = _count_calls(monkeypatch, [
        'pad1_nhwc', 'conv_igemm_8p_fwd', 'bias_act_nhwc'])
    ctx = {}
    for mode, npad in ((_FULL, 0), (_DEFAULT, 4)):
        _set_chain(monkeypatch, mode)
        for route, n8p, nlib in (('intree', 9, 0), ('miopen', 6, 3)):
            monkeypatch.setattr(nn, 'CONV5_ROUTE', route)
            for k in counts:
                counts[k] = 0
            with torch.no_grad():
                ctx[route] = vgg(images)
            assert counts['pad1_nhwc'] == npad, (mode, route)
            assert counts['conv_igemm_8p_fwd'] == n8p, (mode, route)
            assert counts['bias_act_nhwc'] == nlib, (mode, route)
    # two implementations of the same three convs: bf16 outputs of
    # fp32-accumulated K = 4608 sums, three layers deep.  Each layer
    # rounds to bf16 (2^-8 relative), so the routes may differ by a few
    # ulps of the largest activation; 2^-5 of it bounds three layers of
    # one-ulp disagreement amplified by the next layer with margin for
    # neither route being the reference.
    a, b = ctx['intree'].float(), ctx['miopen'].float()
    assert (a - b).abs().max().item() <= a.abs().max().item() * 2.0 ** -5
