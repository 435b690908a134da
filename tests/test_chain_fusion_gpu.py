"""GPU tests: each decoder chain fusion against the launch pair it
replaces, on the same seed (p_fc 0.5, p_lstm 0.3).

The fusions reproduce the pair's roundings, so every deterministic output
must match BITWISE (torch.equal).  Outputs accumulated with fp32 atomics
(dt2, dv) are compared at the accumulation-order tolerance that
test_ops_gpu.test_attn_scores_bwd_tanh_matches_pair uses: two identical
launches already differ in the last ulps there.
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


def _atomics_close(a, b):
    assert torch.allclose(a, b, rtol=1e-4, atol=1e-4)


# (B,H,D,E): the flagship step; then H=D=E=64, where the K=192 GEMMs split
# into four 64-wide K-chunks of which the last is empty — at B=33 (RF=4,
# 31 masked rows) and B=128 (RF=8 full)
_fuse_shapes = pytest.mark.parametrize('B,H,D,E', [
    (32, 512, 512, 512), (33, 64, 64, 64), (128, 64, 64, 64)])

# (B,L,A) of the scores backward: L below its 8 chunks per image; the
# flagship L; two 512-column chunks
_scores_shapes = pytest.mark.parametrize('B,L,A', [
    (3, 5, 512), (2, 196, 512), (4, 196, 1024)])


# ---- dt2 accumulated into a slice of one buffer zeroed once ----

@_scores_shapes
def test_attn_scores_bwd_step_matches_own_fill(B, L, A):
    """attn_scores_bwd_step into a slice of a zeroed [T,B,A] buffer ==
    attn_scores_bwd_tanh (which fills its own dt2)"""
    from sat_amd import _C
    torch.manual_seed(52)
    seed = _seed()
    t1 = _bf(torch.tanh(torch.randn(B * L, A)))
    tdrop = _bf(torch.randn(B * L, A))
    v = _bf(torch.randn(A) * 0.05)
    dlog = torch.randn(B, L, device=DEV)
    dv1 = torch.zeros(A, dtype=torch.float32, device=DEV)
    dv2 = torch.zeros(A, dtype=torch.float32, device=DEV)
    out1, out2 = _empty_bf(B * L, A), _empty_bf(B * L, A)
    DT2 = torch.zeros(3, B, A, dtype=torch.float32, device=DEV)
    _d, dt2a, _ = _C.attn_scores_bwd_step(
        tdrop, v, dlog, seed, _P_FC, _SALT + 2, L, dv1, t1, out1, DT2[1])
    _d, dt2b, _ = _C.attn_scores_bwd_tanh(
        tdrop, v, dlog, seed, _P_FC, _SALT + 2, L, dv2, t1, out2)
    assert torch.equal(out1, out2)
    assert dt2a.data_ptr() == DT2[1].data_ptr()
    _atomics_close(dt2a, dt2b)
    _atomics_close(dv1, dv2)
    assert not DT2[0].any() and not DT2[2].any()   # neighbours untouched


# ---- lstm_in_fuse's columns written by the producers ----

@pytest.mark.parametrize('L', [196, 5])
def test_attn_pool_fwd_xh_matches_pair_bitwise(L):
    """attn_pool_fwd_xh == attn_pool_fwd + lstm_in_fuse (pooled columns)"""
    from sat_amd import _C
    torch.manual_seed(53)
    B, D, E, H, V_ = 3, 512, 64, 64, 100
    I = D + E
    seed = _seed()
    ctx = _bf(torch.randn(B, L, D))
    logits = torch.randn(B, L, device=DEV)
    table = _bf(torch.randn(V_, E))
    ids = torch.randint(0, V_, (B,), device=DEV)
    sth = _bf(torch.randn(B, H))
    xh1 = torch.full((B, I + H), 7.0, dtype=torch.bfloat16, device=DEV)
    xh2 = _empty_bf(B, I + H)
    al1, po1 = _C.attn_pool_fwd_xh(ctx, logits, seed, _P_LSTM, _SALT + 3,
                                   xh1, I)
    al2, po2 = _C.attn_pool_fwd(ctx, logits)
    _C.lstm_in_fuse(po2, table, ids, sth, seed, _P_LSTM, _SALT + 3, xh2)
    assert torch.equal(al1, al2)
    assert torch.equal(po1, po2)
    assert torch.equal(xh1[:, :D], xh2[:, :D])
    assert (xh1[:, D:] == 7.0).all()               # others' columns
    # and the rest of the row from the step-0 launch
    _C.lstm_in_tail(table, ids, sth, seed, _P_LSTM, _SALT + 3, xh1, D)
    assert torch.equal(xh1, xh2)


@_fuse_shapes
def test_dense_lstm_expand_xh_matches_pair_bitwise(B, H, D, E):
    """dense_lstm_expand_xh_fwd == dense_lstm_expand_fwd + the next
    step's lstm_in_fuse (embedding and state columns)"""
    from sat_amd import _C
    torch.manual_seed(54)
    V_ = 1000
    I = D + E
    W = H + D + E
    seed = _seed()
    xh = _bf(torch.randn(B, I + H) * 0.1)
    wl = _bf(torch.randn(4 * H, I + H) * 0.05)
    bl = _bf(torch.randn(4 * H) * 0.1)
    cprev = _bf(torch.randn(B, H))
    pooled = _bf(torch.randn(B, D))
    table = _bf(torch.randn(V_, E))
    ids = torch.randint(0, V_, (B,), device=DEV)
    nids = torch.randint(0, V_, (B,), device=DEV)
    e1, e2 = _empty_bf(B, W), _empty_bf(B, W)
    od1, od2 = _empty_bf(B, H), _empty_bf(B, H)
    xn1 = torch.full((B, W), 7.0, dtype=torch.bfloat16, device=DEV)
    xn2 = _empty_bf(B, W)
    g1, c1, s1 = _C.dense_lstm_expand_xh_fwd(
        xh, wl, bl, cprev, pooled, table, ids, seed, e1, od1,
        1.0, _P_LSTM, _P_FC, _SALT, nids, xn1)
    g2, c2, s2 = _C.dense_lstm_expand_fwd(
        xh, wl, bl, cprev, pooled, table, ids, seed, e2, od2,
        1.0, _P_LSTM, _P_FC, _SALT)
    _C.lstm_in_fuse(pooled, table, nids, s2, seed, _P_LSTM,
                    _SALT + 16 + 3, xn2)
    for a, b in ((g1, g2), (c1, c2), (s1, s2), (e1, e2), (od1, od2)):
        assert torch.equal(a, b)
    assert torch.equal(xn1[:, D:], xn2[:, D:])
    assert (xn1[:, :D] == 7.0).all()               # the pool's columns
    # last step: no next row
    g3, c3, s3 = _C.dense_lstm_expand_xh_fwd(
        xh, wl, bl, cprev, pooled, table, ids, seed, e1, _empty_bf(0),
        1.0, _P_LSTM, _P_FC, _SALT, nids, _empty_bf(0))
    assert torch.equal(g3, g2) and torch.equal(s3, s2)


# ---- tanh backward in the dodrop GEMM's A-operand load ----

def _tanhbwd_case(B, N, K):
    from sat_amd import _C
    seed = _seed()
    dy = torch.randn(B, K, device=DEV) * 0.1
    y = _bf(torch.tanh(torch.randn(B, K)))
    w = _bf(torch.randn(N, K) * 0.05)
    pre1 = torch.full((B, K), 7.0, dtype=torch.bfloat16, device=DEV)
    pre2 = _empty_bf(B, K)
    slabs = _C.dense_tanhbwd_slabs(dy, y, w, pre1)
    y1 = _C.slab_epilogue_drop(slabs, seed, _P_FC, _SALT + 1)
    _C.act_bwd_f32_out(dy, y, 1, pre2)
    y2 = _C.dense_fwd_drop(pre2, w, seed, _P_FC, _SALT + 1)
    assert torch.equal(pre1, pre2)
    assert torch.equal(y1, y2)
    return slabs


@_fuse_shapes
def test_dense_tanhbwd_slabs_matches_pair_bitwise(B, H, D, E):
    """dense_tanhbwd_slabs + slab_epilogue_drop ==
    act_bwd_f32_out + dense_fwd_drop"""
    torch.manual_seed(56)
    K = 512 if H == 512 else H + D + E     # 192: empty 4th K-chunk
    slabs = _tanhbwd_case(B, H, K)
    assert slabs.shape[0] == (8 if H == 512 else 4)


def test_dense_tanhbwd_slabs_single_split_bitwise():
    """K=32 leaves the skinny plan at splitk == 1 (one slab)"""
    torch.manual_seed(57)
    slabs = _tanhbwd_case(32, 72, 32)
    assert slabs.shape[0] == 1


# ---- the drop epilogue inside the next dexp_lstm_bwd ----

@_fuse_shapes
def test_dexp_lstm_bwd_slabs_two_chained_steps_bitwise(B, H, D, E):
    """Two chained reverse steps, d_out_carry handed over as split-K slabs
    vs materialised in bf16 by dense_fwd_drop.  The second step's GEMM
    input is derived from the first step's result, so a difference in
    the first hand-over would also surface in the second."""
    from sat_amd import _C
    torch.manual_seed(58)
    W = H + D + E
    K = 512 if H == 512 else 192
    seed = _seed()
    w = _bf(torch.randn(H, K) * 0.05)
    dsc = _bf(torch.randn(B, H) * 0.1)
    dcc = _bf(torch.randn(B, H) * 0.1)
    steps = [(_bf(torch.randn(B, 4 * H)), _bf(torch.randn(B, H)),
              _bf(torch.randn(B, W) * 0.1),
              _bf(torch.tanh(torch.randn(B, K)))) for _ in range(2)]
    dy0 = torch.randn(B, K, device=DEV) * 0.1

    def run(slab_mode):
        outs = []
        dy = dy0
        y_prod = _bf(torch.tanh(dy0))
        for k, (gates, cprev, dexpd, y_next) in enumerate(steps):
            salt_prod = _SALT + 16 * (2 - k) + 1
            s = _SALT + 16 * (1 - k)
            DG = _empty_bf(B, 4 * H)
            pre = _empty_bf(B, K)
            if slab_mode:
                slabs = _C.dense_tanhbwd_slabs(dy, y_prod, w, pre)
                dcp, dpd, ded = _C.dexp_lstm_bwd_slabs(
                    dexpd, slabs, salt_prod, dsc, seed, gates, cprev, dcc,
                    DG, _P_FC, _P_LSTM, s, D, E, 1.0)
            else:
                _C.act_bwd_f32_out(dy, y_prod, 1, pre)
                doc = _C.dense_fwd_drop(pre, w, seed, _P_FC, salt_prod)
                dcp, dpd, ded = _C.dexp_lstm_bwd(
                    dexpd, doc, dsc, seed, gates, cprev, dcc, DG,
                    _P_FC, _P_LSTM, s, D, E, 1.0)
            outs += [DG, dcp, dpd, ded, pre]
            dy = DG[:, :K].float().contiguous()
            y_prod = y_next
        return outs

    for a, b in zip(run(True), run(False)):
        assert torch.equal(a, b)


# ---- end to end ----

def test_train_steps_fused_chain_matches_per_launch_chain(tiny_config):
    """A B=4 train_step sequence from one seed with dropout on, run twice:
    with the fused chain and with bptt.CHAIN_FUSION off (the launch-by-
    launch chain the fusions replace).  Losses finite and equal to the
    atomics tolerance.

    Parameters: the two runs' gradients differ by fp32 accumulation order
    (dt2 / dv atomics), and Adam's first steps move an element by about
    lr * g/|g| whatever the size of g, so an element whose gradient is
    itself rounding residue may step either way: bounded by 2 * lr per
    step, not by the atomics tolerance.  That bound is what is asserted
    for them."""
    from sat_amd.models import bptt
    from sat_amd.models.base_model import BaseModel
    cfg = tiny_config
    cfg.device = 'cuda'
    cfg.batch_size = 4
    cfg.vocabulary_size = 1000
    cfg.dim_embedding = 512
    cfg.num_lstm_units = 512
    cfg.dim_initalize_layer = 512
    cfg.dim_attend_layer = 512
    cfg.dim_decode_layer = 1024
    cfg.fc_drop_rate = _P_FC
    cfg.lstm_drop_rate = _P_LSTM
    steps = 3

    def run(fused):
        bptt.CHAIN_FUSION = fused
        try:
            torch.manual_seed(cfg.seed)
            m = BaseModel(cfg)
            torch.manual_seed(0)
            images = torch.randn(4, 3, 224, 224, device=DEV) * 50.0
            T = cfg.max_caption_length
            sentences = torch.randint(1, cfg.vocabulary_size, (4, T),
                                      device=DEV)
            masks = torch.zeros(4, T, device=DEV)
            masks[:, :14] = 1.0
            masks[1, 9:] = 0.0
            losses = [m.train_step(images, sentences, masks)['total_loss']
                      .item() for _ in range(steps)]
            params = {n: p.detach().float().clone()
                      for n, p in m.model.named_parameters()
                      if p.requires_grad}
        finally:
            bptt.CHAIN_FUSION = True
        return losses, params

    la, pa = run(True)
    lb, pb = run(False)
    print('losses', la, lb)
    assert all(x == x and abs(x) != float('inf') for x in la + lb)
    _atomics_close(torch.tensor(la), torch.tensor(lb))
    bound = 2.0 * steps * cfg.initial_learning_rate * 1.01
    assert set(pa) == set(pb)
    for n in pa:
        assert float((pa[n] - pb[n]).abs().max()) <= bound, n
