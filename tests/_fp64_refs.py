"""Independent references for the kernel tests, written from the maths.

Two kinds live here:

* a numpy re-implementation of the counter dropout hash (`mix3`,
  `drop_scale`, `drop_scale8`) in exact uint32 / float32 arithmetic, so a
  mask can be compared bitwise with the device's;
* plain torch formulas (Adam with global-norm clip and staircase decay,
  masked softmax cross-entropy, the LSTM cell, the attention pool, the
  frozen-BatchNorm epilogue) that take a dtype: evaluated in float64 they
  are the reference, evaluated in float32 on the CPU they give the noise
  floor `max|fp32_cpu - fp64|` the tolerances are built from.

Nothing here imports the extension or looks at a kernel's memory layout.
"""

import numpy as np
import torch

# ---------------------------------------------------------------------
# tolerance policy
# ---------------------------------------------------------------------

BF16_EPS = 2.0 ** -8       # one bf16 rounding, relative (half an ulp)
SLACK = 8.0                # device fast-math + summation order allowance


def f64(t):
    return t.detach().to('cpu', torch.float64)


def noise_floor(fp32_cpu, ref64):
    """max|fp32_cpu - fp64| of the same formula on the same inputs"""
    return (fp32_cpu.double() - ref64).abs().max().item()


def fp32_err(got, ref64):
    return (f64(got) - ref64).abs().max().item()


def bf16_excess(got, ref64, floor):
    """max over elements of |got - ref| / (2^-8 |ref| + 8 floor); the
    policy holds when this is <= 1.  Where the bound is 0 (ref == 0 and
    floor == 0) the element must be exactly 0."""
    err = (f64(got) - ref64).abs()
    bound = BF16_EPS * ref64.abs() + SLACK * floor
    inf = torch.full_like(err, float('inf'))
    ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300),
                        torch.where(err > 0, inf, torch.zeros_like(err)))
    return ratio.max().item()


# ---------------------------------------------------------------------
# dropout hash oracle (numpy uint32 / float32)
# ---------------------------------------------------------------------

_M32 = np.uint64(0xFFFFFFFF)


def _u64(x):
    return np.asarray(x).astype(np.int64).astype(np.uint64) & _M32


def _mul(a, k):
    return (a * np.uint64(k)) & _M32


def mix3(a, b, c):
    """h(a, b, c) on uint32 words (arrays broadcast); returns uint32."""
    a, b, c = _u64(a), _u64(b), _u64(c)
    h = _mul(a, 0x9E3779B1) ^ _mul(b, 0x85EBCA77) ^ _mul(c, 0xC2B2AE3D)
    h ^= h >> np.uint64(16)
    h = _mul(h, 0x7FEB352D)
    h ^= h >> np.uint64(15)
    h = _mul(h, 0x846CA68B)
    h ^= h >> np.uint64(16)
    return h.astype(np.uint32)


def drop_keep(seed, salt, idx, p):
    """keep decision of drop_scale: u = (h >> 8) * 2^-24 >= p in float32"""
    h = mix3(seed, salt, idx)
    u = (h >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)
    return u >= np.float32(p)


def drop_inv(p):
    """1 / (1 - p) in float32 arithmetic"""
    return np.float32(1.0) / (np.float32(1.0) - np.float32(p))


def drop_scale(seed, salt, idx, p):
    if p <= 0.0:
        return np.ones(np.shape(idx), np.float32)
    return np.where(drop_keep(seed, salt, idx, p), drop_inv(p),
                    np.float32(0.0)).astype(np.float32)


def drop_pq(p):
    return int(np.float32(p) * np.float32(256.0))


def drop_keep8(seed, salt, idx8, p):
    """[..., 8] keep decisions of drop_scale8 for 8-element group idx8:
    lane e < 4 is byte e of h1, lane 4 + e is byte e of h2."""
    idx8 = np.asarray(idx8)
    h1 = mix3(seed, salt, idx8)
    h2 = mix3(h1, _u64(salt) ^ np.uint64(0xA5A5A5A5), idx8)
    pq = np.uint32(drop_pq(p))
    lanes = []
    for h in (h1, h2):
        for e in range(4):
            lanes.append(((h >> np.uint32(8 * e)) & np.uint32(0xFF)) >= pq)
    return np.stack(lanes, axis=-1)


def drop_inv8(p):
    """the inverse of the rate drop_scale8 really applies, floor(256p)/256"""
    return np.float32(256.0) / np.float32(256 - drop_pq(p))


def drop_scale8(seed, salt, idx8, p):
    idx8 = np.asarray(idx8)
    if p <= 0.0:
        return np.ones(idx8.shape + (8,), np.float32)
    return np.where(drop_keep8(seed, salt, idx8, p), drop_inv8(p),
                    np.float32(0.0)).astype(np.float32)


def dropout_ref(x_bf16, scale):
    """bf16(float32(x) * scale); x a CPU bf16 tensor, scale a float32
    numpy array of x's shape.  One fp32 multiply, one rounding."""
    s = torch.from_numpy(np.ascontiguousarray(scale, dtype=np.float32))
    return (x_bf16.float() * s.reshape(x_bf16.shape)).to(torch.bfloat16)


def bits(t):
    """bit pattern of a bf16 tensor, for exact comparison (-0 != +0)"""
    return t.detach().cpu().contiguous().view(torch.int16)


# ---------------------------------------------------------------------
# Adam with global-norm clip and staircase decay
# ---------------------------------------------------------------------

def adam_ref(ps, gs, ms, vs, t, hp, dtype):
    """One step on lists of CPU tensors, all arithmetic in `dtype`.
    hp: dict(lr0, decay, spd, b1, b2, eps, clip).  Returns
    (new ps, new ms, new vs, lr, scale) without touching the inputs."""
    def S(x):
        return torch.tensor(float(x), dtype=dtype)
    ps = [x.to(dtype) for x in ps]
    gs = [x.to(dtype) for x in gs]
    ms = [x.to(dtype) for x in ms]
    vs = [x.to(dtype) for x in vs]
    gsq = sum((g * g).sum() for g in gs)
    norm = gsq.sqrt()
    scale = S(1.0)
    if hp['clip'] > 0 and norm > S(hp['clip']):
        scale = S(hp['clip']) / norm
    lr = S(hp['lr0'])
    if hp['decay'] < 1.0:
        lr = lr * S(hp['decay']) ** torch.floor(S(t) / S(hp['spd']))
    b1, b2, eps = S(hp['b1']), S(hp['b2']), S(hp['eps'])
    bc1 = 1 - b1 ** S(t)
    bc2 = 1 - b2 ** S(t)
    pn, mn, vn = [], [], []
    for p, g, m, v in zip(ps, gs, ms, vs):
        g = g * scale
        m1 = b1 * m + (1 - b1) * g
        v1 = b2 * v + (1 - b2) * g * g
        pn.append(p - lr * (m1 / bc1) / ((v1 / bc2).sqrt() + eps))
        mn.append(m1)
        vn.append(v1)
    return pn, mn, vn, lr.item(), scale.item()


# ---------------------------------------------------------------------
# masked softmax cross-entropy
# ---------------------------------------------------------------------

def ce_ref(logits, labels, mask, dloss, dtype):
    """(losses, lse, dlogits) for logits [B,V], labels [B], mask [B],
    dloss [B]; CPU tensors, arithmetic in `dtype`."""
    x = logits.to(dtype)
    lse = torch.logsumexp(x, dim=1)
    picked = x.gather(1, labels.view(-1, 1)).squeeze(1)
    mk, dl = mask.to(dtype), dloss.to(dtype)
    losses = (lse - picked) * mk
    onehot = torch.zeros_like(x)
    onehot.scatter_(1, labels.view(-1, 1), 1.0)
    dlogits = (torch.exp(x - lse[:, None]) - onehot) * (mk * dl)[:, None]
    return losses, lse, dlogits


# ---------------------------------------------------------------------
# LSTM cell (gate order i, j, f, o; forget bias before the sigmoid)
# ---------------------------------------------------------------------

def lstm_fwd_ref(gates, c, fb, dtype):
    B, H = c.shape
    g = gates.to(dtype).view(B, 4, H)
    gi, gj = torch.sigmoid(g[:, 0]), torch.tanh(g[:, 1])
    gf, go = torch.sigmoid(g[:, 2] + fb), torch.sigmoid(g[:, 3])
    cn = c.to(dtype) * gf + gi * gj
    return torch.tanh(cn) * go, cn


def lstm_bwd_ref(gates, c, dh, dc, fb, dtype):
    """(dgates [B,4,H], dc_prev [B,H]); dc may be None"""
    B, H = c.shape
    g = gates.to(dtype).view(B, 4, H)
    cp, dh = c.to(dtype), dh.to(dtype)
    gi, gj = torch.sigmoid(g[:, 0]), torch.tanh(g[:, 1])
    gf, go = torch.sigmoid(g[:, 2] + fb), torch.sigmoid(g[:, 3])
    tc = torch.tanh(cp * gf + gi * gj)
    dct = dh * go * (1 - tc * tc)
    if dc is not None:
        dct = dct + dc.to(dtype)
    dg = torch.stack([dct * gj * gi * (1 - gi),
                      dct * gi * (1 - gj * gj),
                      dct * cp * gf * (1 - gf),
                      dh * tc * go * (1 - go)], dim=1)
    return dg, dct * gf


# ---------------------------------------------------------------------
# attention pool: alpha = softmax_L(logits), pooled = sum_l alpha ctx
# ---------------------------------------------------------------------

def attn_pool_ref(ctx, logits, dtype):
    a = torch.softmax(logits.to(dtype), dim=1)
    return a, torch.einsum('bl,bld->bd', a, ctx.to(dtype))


def attn_pool_bwd_ref(ctx, logits, dalpha, dpooled, dtype):
    """(dlogits [B,L], dctx [B,L,D]); dalpha may be None"""
    a = torch.softmax(logits.to(dtype), dim=1)
    dp = dpooled.to(dtype)
    da = torch.einsum('bld,bd->bl', ctx.to(dtype), dp)
    if dalpha is not None:
        da = da + dalpha.to(dtype)
    dlogits = a * (da - (a * da).sum(1, keepdim=True))
    return dlogits, a[:, :, None] * dp[:, None, :]


# ---------------------------------------------------------------------
# frozen BatchNorm epilogue: relu(x * scale + shift), per channel
# ---------------------------------------------------------------------

def scale_shift_ref(x, scale, shift, relu, dtype):
    y = x.to(dtype) * scale.to(dtype).view(1, -1, 1, 1) \
        + shift.to(dtype).view(1, -1, 1, 1)
    return torch.relu(y) if relu else y
