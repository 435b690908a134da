"""GPU tests for the decoder chain kernels that issue their loads ahead of
their waits: the split-K slab sums and the skinny GEMM's batched K loop;
and for the scores backward, pinned to its fp32 reference at the shapes
where a row-batched form of it would go wrong.

Moving loads must not move a bit: slab sums keep the order
((0 + s0) + s1) + ..., each MFMA accumulator still sums k-ascending, and
dt1 is a per-element function of its own row.  So the checks are
torch.equal wherever the output is deterministic, and the accumulation
tolerance of tests/test_chain_fusion_gpu.py for the atomically summed
dt2 / dv.
"""

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = 'cuda'
_P_FC, _P_LSTM, _SALT = 0.5, 0.3, 48


def _bf(x):
    return x.to(DEV, torch.bfloat16)


def _seed():
    return torch.tensor(777, dtype=torch.int64, device=DEV)


def _empty_bf(*shape):
    return torch.empty(*shape, dtype=torch.bfloat16, device=DEV)


def _skinny_plan(N, K):
    """split count of the skinny GEMM (gemm.hip skinny_plan)"""
    nblocks = -(-N // 64)
    splitk = 1
    while nblocks * splitk < 192 and splitk < 8 and K // 32 >= 2 * splitk:
        splitk *= 2
    return splitk


# ---- slab sum order ----

def _slab_fixture(S, M, N):
    """fp32 slabs [S, M, N] on the CPU with a wide magnitude spread.

    A different summation order changes an fp32 sum in its last bits, and
    a bf16 cast hides that unless the terms nearly cancel.  So on every
    other element the last slab is set to minus the sequential sum of the
    others, plus a term 2^-20 of their size: what is left after the last
    add are the rounding errors of the partial sums, which depend on the
    order, at full relative size."""
    g = torch.Generator().manual_seed(1000 + 100 * S + M)
    x = torch.randn(S, M, N, generator=g) * 10.0 ** torch.randint(
        -3, 4, (S, M, N), generator=g).float()
    if S >= 3:
        part = torch.zeros(M, N)
        for k in range(S - 1):
            part = part + x[k]
        cancel = -part + part.abs() * 2.0 ** -20 * torch.randn(
            M, N, generator=g)
        x[S - 1].view(-1)[::2] = cancel.view(-1)[::2]
    return x


def _seq_sum(x):
    v = torch.zeros_like(x[0])
    for k in range(x.shape[0]):
        v = v + x[k]
    return v


def _tree_sum(xs):
    if len(xs) == 1:
        return xs[0]
    mid = len(xs) // 2
    return _tree_sum(xs[:mid]) + _tree_sum(xs[mid:])


@pytest.mark.parametrize('M,N', [(3, 40), (32, 520)])
@pytest.mark.parametrize('S', [1, 2, 3, 4, 5, 7, 8, 11])
def test_slab_sum_is_sequential(S, M, N):
    """slab_epilogue_drop(p = 0) == bf16 of the sequential fp32 sum, for
    the compile-time counts 1..8 and the runtime-count path (11); 120
    elements (less than a block) and 16640 (ragged last block).  For
    S >= 3 the fixture tells a pairwise tree from the sequential order
    (S <= 2 has one order only)."""
    from sat_amd import _C
    x = _slab_fixture(S, M, N)
    ref = _seq_sum(x).to(torch.bfloat16)
    if S >= 3:
        tree = _tree_sum(list(x)).to(torch.bfloat16)
        assert not torch.equal(tree, ref), 'fixture cannot tell the orders'
    y = _C.slab_epilogue_drop(x.to(DEV), _seed(), 0.0, _SALT)
    assert y.shape == (M, N)
    assert torch.equal(y.cpu(), ref)


# ---- fused slab consumers at every split count ----

# (B, H, D, E) -> gates GEMM N = 4H, K = D+E+H, splitk 1 / 2 / 4 / 8
_split_shapes = pytest.mark.parametrize('B,H,D,E,splitk', [
    (2, 16, 8, 8, 1), (3, 32, 32, 32, 2), (32, 64, 64, 64, 4),
    (5, 128, 128, 128, 8)])


@_split_shapes
def test_lstm_expand_xh_every_split_bitwise(B, H, D, E, splitk):
    """dense_lstm_expand_xh_fwd == dense_lstm_expand_fwd + the next step's
    lstm_in_fuse, with and without the next row"""
    from sat_amd import _C
    torch.manual_seed(61)
    assert _skinny_plan(4 * H, D + E + H) == splitk
    V_ = 50
    I, W = D + E, H + D + E
    seed = _seed()
    xh = _bf(torch.randn(B, I + H) * 0.1)
    wl = _bf(torch.randn(4 * H, I + H) * 0.05)
    bl = _bf(torch.randn(4 * H) * 0.1)
    cprev = _bf(torch.randn(B, H))
    pooled = _bf(torch.randn(B, D))
    table = _bf(torch.randn(V_, E))
    ids = torch.randint(0, V_, (B,), device=DEV)
    nids = torch.randint(0, V_, (B,), device=DEV)
    e1, e3 = _empty_bf(B, W), _empty_bf(B, W)
    od1, od3 = _empty_bf(B, H), _empty_bf(B, H)
    xn1 = torch.full((B, W), 7.0, dtype=torch.bfloat16, device=DEV)
    g1, c1, s1 = _C.dense_lstm_expand_xh_fwd(
        xh, wl, bl, cprev, pooled, table, ids, seed, e1, od1,
        1.0, _P_LSTM, _P_FC, _SALT, nids, xn1)
    e2, od2 = _empty_bf(B, W), _empty_bf(B, H)
    g2, c2, s2 = _C.dense_lstm_expand_fwd(
        xh, wl, bl, cprev, pooled, table, ids, seed, e2, od2,
        1.0, _P_LSTM, _P_FC, _SALT)
    xn2 = _empty_bf(B, W)
    _C.lstm_in_fuse(pooled, table, nids, s2, seed, _P_LSTM,
                    _SALT + 16 + 3, xn2)
    for a, b in ((g1, g2), (c1, c2), (s1, s2), (e1, e2), (od1, od2)):
        assert torch.equal(a, b)
    # gates and c also against the plain gates epilogue (its h_raw is
    # rounded to bf16 before the expand, so only these two are bitwise)
    g4, _h4, c4 = _C.dense_lstm_fwd(xh, wl, bl, cprev, 1.0)
    assert torch.equal(g1, g4) and torch.equal(c1, c4)
    assert torch.equal(xn1[:, D:], xn2[:, D:])
    assert (xn1[:, :D] == 7.0).all()               # the pool's columns
    # last step: no next row
    g3, c3, s3 = _C.dense_lstm_expand_xh_fwd(
        xh, wl, bl, cprev, pooled, table, ids, seed, e3, od3,
        1.0, _P_LSTM, _P_FC, _SALT, nids, _empty_bf(0))
    for a, b in ((g3, g2), (c3, c2), (s3, s2), (e3, e2), (od3, od2)):
        assert torch.equal(a, b)


@_split_shapes
def test_dense_dx_fuse_every_split_bitwise(B, H, D, E, splitk):
    """dense_dx_fuse == dense_fwd + dx_fuse.  The pair rounds dxh to bf16
    between its launches; with small-integer operands (dxh an integer of
    at most 256 in size, exact in bf16) and p = 0.5 (keep scale 2.0,
    exact) that rounding changes nothing, and the pair is bitwise."""
    from sat_amd import _C
    torch.manual_seed(62)
    I = D + E
    seed = _seed()
    dgates = _bf(torch.randint(-2, 3, (B, 4 * H)).float())
    wl_t = _bf(torch.randint(-1, 2, (I + H, 4 * H)).float())
    dpool_dec = _bf(torch.randn(B, D))
    demb_dec = _bf(torch.randn(B, E))
    demb1, demb2 = _empty_bf(B, E), _empty_bf(B, E)
    dp1, ds1 = _C.dense_dx_fuse(dgates, wl_t, dpool_dec, demb_dec,
                                seed, demb1, 0.5, _SALT + 3, D, E, H)
    dxh = _C.dense_fwd(dgates, wl_t, _empty_bf(0), 0)
    assert dxh.float().abs().max().item() <= 256.0
    assert torch.equal(dxh.float(), dgates.float() @ wl_t.float().t())
    dp2, ds2 = _C.dx_fuse(dxh, dpool_dec, demb_dec, seed, demb2,
                          0.5, _SALT + 3, H)
    assert torch.equal(dp1, dp2)
    assert torch.equal(ds1, ds2)
    assert torch.equal(demb1, demb2)


@_split_shapes
def test_dexp_lstm_bwd_slabs_every_split_bitwise(B, H, D, E, splitk):
    """dexp_lstm_bwd_slabs(dense_tanhbwd_slabs) ==
    act_bwd_f32_out + dense_fwd_drop + dexp_lstm_bwd; the carry GEMM is
    [B, K] x [H, K]^T with K = D+E+H, with and without dc"""
    from sat_amd import _C
    torch.manual_seed(63)
    W = K = H + D + E
    seed = _seed()
    w = _bf(torch.randn(H, K) * 0.05)
    dsc = _bf(torch.randn(B, H) * 0.1)
    gates = _bf(torch.randn(B, 4 * H))
    cprev = _bf(torch.randn(B, H))
    dexpd = _bf(torch.randn(B, W) * 0.1)
    dy = torch.randn(B, K, device=DEV) * 0.1
    y = _bf(torch.tanh(torch.randn(B, K)))
    for dcc in (_bf(torch.randn(B, H) * 0.1), _empty_bf(0)):
        DG1, DG2 = _empty_bf(B, 4 * H), _empty_bf(B, 4 * H)
        pre1, pre2 = _empty_bf(B, K), _empty_bf(B, K)
        slabs = _C.dense_tanhbwd_slabs(dy, y, w, pre1)
        assert slabs.shape[0] == _skinny_plan(H, K)
        o1 = _C.dexp_lstm_bwd_slabs(
            dexpd, slabs, _SALT + 17, dsc, seed, gates, cprev, dcc, DG1,
            _P_FC, _P_LSTM, _SALT, D, E, 1.0)
        _C.act_bwd_f32_out(dy, y, 1, pre2)
        doc = _C.dense_fwd_drop(pre2, w, seed, _P_FC, _SALT + 17)
        o2 = _C.dexp_lstm_bwd(
            dexpd, doc, dsc, seed, gates, cprev, dcc, DG2,
            _P_FC, _P_LSTM, _SALT, D, E, 1.0)
        assert torch.equal(pre1, pre2) and torch.equal(DG1, DG2)
        for a, b in zip(o1, o2):
            assert torch.equal(a, b)


# ---- skinny GEMM exactness ----

_INT_REF = {}


def _int_case(M, N, K):
    """small-integer operands in [-4, 4]: every partial sum is an integer
    below 2^24, exact in fp32 in any order"""
    key = (M, N, K)
    if key not in _INT_REF:
        g = torch.Generator().manual_seed(7000 + M + 3 * N + 5 * K)
        x = torch.randint(-4, 5, (M, K), generator=g).float()
        w = torch.randint(-4, 5, (N, K), generator=g).float()
        b = torch.randint(-4, 5, (N,), generator=g).float()
        _INT_REF[key] = (_bf(x), _bf(w), _bf(b), (x @ w.t()).to(DEV),
                         b.to(DEV))
    return _INT_REF[key]


@pytest.mark.parametrize('K', [32, 64, 192, 1536])
@pytest.mark.parametrize('N', [40, 72, 512])
@pytest.mark.parametrize('M', [1, 17, 32, 33, 64, 100, 128])
def test_skinny_gemm_exact_on_integers(M, N, K):
    """dense_fwd == bf16(fp32 matmul) on integer operands, bias off and
    on; with tanh on, the tolerance of test_ops_gpu.test_dense_fwd"""
    from sat_amd import _C
    x, w, b, xw, bias = _int_case(M, N, K)
    y0 = _C.dense_fwd(x, w, _empty_bf(0), 0)
    assert torch.equal(y0, xw.to(torch.bfloat16))
    y1 = _C.dense_fwd(x, w, b, 0)
    assert torch.equal(y1, (xw + bias).to(torch.bfloat16))
    for bb, ref in ((_empty_bf(0), xw), (b, xw + bias)):
        # tanh of an integer is +-1 almost everywhere; scale the product
        # down so the comparison sees the curve
        ws = (w.float() / 64.0).to(torch.bfloat16)     # exact: power of 2
        yt = _C.dense_fwd(x, ws, bb, 1)
        rt = torch.tanh(xw / 64.0 + (ref - xw))
        denom = rt.abs().max().clamp_min(1e-6)
        assert ((yt.float() - rt).abs().max() / denom).item() < 2e-2


@pytest.mark.parametrize('K', [32, 512])          # 1 and 8 splits at N = 72
@pytest.mark.parametrize('M', [3, 32, 100])
def test_dense_tanhbwd_slabs_matches_pair(M, K):
    """dense_tanhbwd_slabs + slab_epilogue_drop ==
    act_bwd_f32_out + dense_fwd_drop, bitwise, and the side store"""
    from sat_amd import _C
    torch.manual_seed(64)
    N = 72
    seed = _seed()
    dy = torch.randn(M, K, device=DEV) * 0.1
    y = _bf(torch.tanh(torch.randn(M, K)))
    w = _bf(torch.randn(N, K) * 0.05)
    pre1 = torch.full((M, K), 7.0, dtype=torch.bfloat16, device=DEV)
    pre2 = _empty_bf(M, K)
    slabs = _C.dense_tanhbwd_slabs(dy, y, w, pre1)
    assert slabs.shape[0] == _skinny_plan(N, K) == (1 if K == 32 else 8)
    y1 = _C.slab_epilogue_drop(slabs, seed, _P_FC, _SALT + 1)
    _C.act_bwd_f32_out(dy, y, 1, pre2)
    y2 = _C.dense_fwd_drop(pre2, w, seed, _P_FC, _SALT + 1)
    assert torch.equal(pre1, pre2)
    assert torch.equal(y1, y2)


# ---- scores backward ----

@pytest.mark.parametrize('with_y', [False, True])
@pytest.mark.parametrize('B,L,A', [
    (2, 5, 512),        # fewer rows than chunks and waves
    (3, 196, 512),      # flagship L, short last chunk
    (1, 33, 1024),      # NCH = 2
    (1, 9, 1536),       # NCH = 3
])
def test_attn_scores_bwd_against_reference(B, L, A, with_y):
    """attn_scores_bwd_step (caller-zeroed dt2) and attn_scores_bwd_tanh
    against the fp32 reference built from the mask the forward kernel
    applies (p = 0.5: keep scale 2.0, exact).

    dt1: equal between the two launches, zero exactly where the mask is,
    and within one bf16 ulp of the reference, |a - b| <= 2^-7 |ref| (8-bit
    significand; 1 - y*y is contracted to one FMA).  dt2 / dv: atomically
    accumulated, rtol = atol = 1e-4 at unit-scale inputs."""
    from sat_amd import _C
    torch.manual_seed(65)
    p, salt = 0.5, _SALT + 2
    seed = _seed()
    ones = torch.ones(B * L, A, dtype=torch.bfloat16, device=DEV)
    zeros = torch.zeros(B, A, dtype=torch.bfloat16, device=DEV)
    v1 = torch.ones(A, dtype=torch.bfloat16, device=DEV)
    sc = _C.attn_scores_fused(ones, zeros, v1, seed, p, salt, L)[0].float()
    assert set(sc.unique().tolist()) == {0.0, 2.0}

    tdrop = _bf(torch.randn(B * L, A))
    v = _bf(torch.randn(A))
    dlog = torch.randn(B, L, device=DEV)
    t1y = _bf(torch.tanh(torch.randn(B * L, A))) if with_y \
        else _empty_bf(0)

    dt = dlog.reshape(-1, 1) * v.float() * sc
    ref2 = dt.reshape(B, L, A).sum(1)
    refv = (tdrop.float() * dlog.reshape(-1, 1)).sum(0)
    ref1 = dt * (1.0 - t1y.float() ** 2) if with_y else dt

    dva = torch.zeros(A, dtype=torch.float32, device=DEV)
    dvb = torch.zeros(A, dtype=torch.float32, device=DEV)
    out_a, out_b = _empty_bf(B * L, A), _empty_bf(B * L, A)
    DT2 = torch.zeros(3, B, A, dtype=torch.float32, device=DEV)
    _d, dt2a, _ = _C.attn_scores_bwd_step(
        tdrop, v, dlog, seed, p, salt, L, dva, t1y, out_a, DT2[1])
    _d, dt2b, _ = _C.attn_scores_bwd_tanh(
        tdrop, v, dlog, seed, p, salt, L, dvb, t1y, out_b)
    assert torch.equal(out_a, out_b)
    assert torch.equal(out_a == 0, ref1 == 0)
    assert ((out_a.float() - ref1).abs() <= 2.0 ** -7 * ref1.abs()).all()
    assert dt2a.data_ptr() == DT2[1].data_ptr()
    assert not DT2[0].any() and not DT2[2].any()   # neighbours untouched
    for got, ref in ((dt2a, ref2), (dt2b, ref2), (dva, refv), (dvb, refv)):
        assert torch.allclose(got, ref, rtol=1e-4, atol=1e-4)
