"""The counter dropout hash, checked on the CPU against a numpy oracle.

The oracle (`_fp64_refs.mix3` / `drop_scale` / `drop_scale8`) is written
from the formulas of `common.h` in exact uint32 / float32 arithmetic.  This
file pins it (golden vectors, a second pure-int implementation) and asserts
the statistical properties dropout needs from it; `test_tail_ops_gpu.py`
then compares every dropout kernel with it bitwise, and the first golden
vectors with the device.

Every statistic is a z-score: under independence a sample correlation of n
pairs has standard deviation 1/sqrt(n), a sample rate sqrt(p(1-p)/n).
Bounds are 4.5 sigma for rates and 5 for correlations (a few thousand
statistics are taken; P(|z| > 4.5) = 7e-6, P(|z| > 5) = 6e-7).
"""

import json
import os

import numpy as np
import pytest

from _fp64_refs import (drop_inv, drop_inv8, drop_keep, drop_keep8,
                        drop_pq, drop_scale, drop_scale8, mix3)

N = 65536
IDX = np.arange(N, dtype=np.int64)
SEEDS = (0, 1, 777, 12345, 12346)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)),
                      'golden', 'dropout_hash.json')


def _golden():
    with open(GOLDEN) as f:
        return json.load(f)['vectors']


def _mix3_int(a, b, c):
    """mix3 again, on Python ints (no numpy): pins the oracle itself"""
    m = 0xFFFFFFFF
    a, b, c = a & m, b & m, c & m
    h = (a * 0x9E3779B1 & m) ^ (b * 0x85EBCA77 & m) ^ (c * 0xC2B2AE3D & m)
    h ^= h >> 16
    h = h * 0x7FEB352D & m
    h ^= h >> 15
    h = h * 0x846CA68B & m
    h ^= h >> 16
    return h


def _u(seed, salt, idx):
    """the uniform drop_scale thresholds, exact in float64"""
    return (mix3(seed, salt, idx) >> np.uint32(8)).astype(np.float64) \
        * 2.0 ** -24


def _zcorr(rows):
    """|rho| sqrt(n) for every pair of rows of a [k, n] array"""
    x = np.asarray(rows, dtype=np.float64)
    x = x - x.mean(axis=1, keepdims=True)
    x /= np.sqrt((x * x).sum(axis=1, keepdims=True))
    z = np.abs(x @ x.T) * np.sqrt(x.shape[1])
    return z[np.triu_indices(x.shape[0], k=1)]


# ---- the oracle is pinned ----

def test_golden_vectors_match_oracle():
    vec = _golden()
    assert len(vec) >= 300
    a = np.array(vec, dtype=np.int64)
    got = mix3(a[:, 0], a[:, 1], a[:, 2])
    assert np.array_equal(got, a[:, 3].astype(np.uint32))
    for seed, salt, idx, h in vec:
        assert _mix3_int(seed, salt, idx) == h
    # the vectors exercise the wrap-arounds: a negative salt, an index
    # and a seed past 2^31
    assert (a[:, 1] < 0).any() and (a[:, 2] >= 2 ** 31).any() \
        and (a[:, 0] >= 2 ** 31).any()


def test_salt_and_seed_enter_as_uint32():
    """(uint32)salt of a negative int, (uint32)seed of an int64"""
    i = IDX[:64]
    assert np.array_equal(mix3(5, -1, i), mix3(5, 0xFFFFFFFF, i))
    assert np.array_equal(mix3(2 ** 32 + 5, 3, i), mix3(5, 3, i))


def test_drop_scale_threshold_is_float32():
    """u = (h >> 8) 2^-24 is compared with float32(p), and u == p is
    kept: the boundary hash words on either side of p = 0.3 and 0.5"""
    for p in (0.3, 0.5):
        k = int(np.ceil(float(np.float32(p)) * 2 ** 24))    # first kept u
        for word, kept in ((k << 8, True), (((k - 1) << 8) | 0xFF, False)):
            u = np.float32(word >> 8) * np.float32(2.0 ** -24)
            assert bool(u >= np.float32(p)) is kept
    # the oracle's values: 0 or 1/(1-p) in float32, 1 at p = 0
    s = drop_scale(777, 7, IDX[:4096], 0.3)
    assert set(np.unique(s).tolist()) == {0.0, float(drop_inv(0.3))}
    assert float(drop_inv(0.5)) == 2.0
    assert (drop_scale(777, 7, IDX[:64], 0.0) == 1.0).all()
    assert (drop_scale8(777, 7, IDX[:64], 0.0) == 1.0).all()


# ---- statistics of the per-element hash ----

@pytest.mark.parametrize('p', [0.3, 0.5])
def test_keep_rate(p):
    sigma = np.sqrt(p * (1 - p) / N)
    salts = np.arange(64, dtype=np.int64)[:, None]
    worst = 0.0
    for seed in SEEDS:
        keep = drop_keep(seed, salts, IDX[None, :], p)      # [64, N]
        z = np.abs(keep.mean(axis=1) - (1 - p)) / sigma
        worst = max(worst, z.max())
    assert worst < 4.5, worst                   # measured 2.96 / 3.07


@pytest.mark.parametrize('seed', [0, 777, 12345])
def test_salt_streams_uncorrelated(seed):
    """every pair of salts below 40, same seed, same index: the uniform
    thresholds and the keep bits at both rates"""
    salts = np.arange(40, dtype=np.int64)[:, None]
    u = _u(seed, salts, IDX[None, :])
    for rows in (u, u >= np.float32(0.3), u >= 0.5):
        z = _zcorr(rows)
        assert z.size == 780
        assert z.max() < 5, z.max()             # measured max 4.09


@pytest.mark.parametrize('seed', [0, 777, 12345])
def test_consecutive_seeds_uncorrelated(seed):
    """seed vs seed+1, +2, +3 (the model advances the seed by one per
    step) at the same salt and index"""
    for salt in (0, 1, 7, 48):
        u = np.stack([_u(seed + d, salt, IDX) for d in range(4)])
        for rows in (u, u >= np.float32(0.3), u >= 0.5):
            assert _zcorr(rows).max() < 5       # measured max 3.05


def test_lag1_autocorrelation():
    salts = np.arange(64, dtype=np.int64)[:, None]
    worst = 0.0
    for seed in SEEDS:
        u = _u(seed, salts, IDX[None, :])
        for x in (u, (u >= 0.5).astype(np.float64)):
            a = x[:, :-1] - x[:, :-1].mean(axis=1, keepdims=True)
            b = x[:, 1:] - x[:, 1:].mean(axis=1, keepdims=True)
            rho = (a * b).sum(1) / np.sqrt((a * a).sum(1) * (b * b).sum(1))
            worst = max(worst, np.abs(rho).max() * np.sqrt(N - 1))
    assert worst < 5, worst                     # measured 3.8


# ---- the 8-wide variant ----

@pytest.mark.parametrize('p', [0.3, 0.5])
def test_drop_scale8_lanes(p):
    """the eight lanes of one group are pairwise uncorrelated, each keeps
    at the quantised rate 1 - floor(256p)/256, and two salts do not
    correlate lane by lane"""
    q = 1.0 - drop_pq(p) / 256.0
    sigma = np.sqrt(q * (1 - q) / N)
    for seed in (0, 777, 12345):
        for salt in (2, 50):
            keep = drop_keep8(seed, salt, IDX, p)           # [N, 8]
            assert _zcorr(keep.T).max() < 5                 # measured 2.8
            z = np.abs(keep.mean(axis=0) - q) / sigma
            assert z.max() < 4.5, z.max()                   # measured 2.5
        a = drop_keep8(seed, 2, IDX, p).reshape(-1)
        b = drop_keep8(seed, 18, IDX, p).reshape(-1)
        c = drop_keep8(seed + 1, 2, IDX, p).reshape(-1)
        assert _zcorr(np.stack([a, b, c])).max() < 5


@pytest.mark.parametrize('p', [0.3, 0.5])
def test_drop_scale8_scale_is_unbiased(p):
    """E[scale] = 1: kept values are scaled by the inverse of the rate the
    byte compare really applies.  Scaling by 1/(1-p) instead is exact at
    p = 0.5 and 0.45 % high at p = 0.3 (180/256 kept, times 1/0.7)."""
    n8 = 2 ** 16                                # 2^19 elements
    sc = drop_scale8(12345, 2, np.arange(n8, dtype=np.int64), p)
    q = 1.0 - drop_pq(p) / 256.0
    assert abs(float(drop_inv8(p)) * q - 1.0) < 2.0 ** -23
    sigma = float(drop_inv8(p)) * np.sqrt(q * (1 - q) / sc.size)
    z = abs(sc.astype(np.float64).mean() - 1.0) / sigma
    assert z < 4.5, z                           # measured 1.4 / 0.65; with the
    #                                             1/(1-p) scale: 6.4 / 0.65
    # what the 1/(1-p) scale would have given
    biased = q * float(drop_inv(p))
    if p == 0.5:
        assert biased == 1.0 and drop_inv8(p) == drop_inv(p)
    else:
        assert abs(biased - 1.0045) < 1e-4
