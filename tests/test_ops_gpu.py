"""GPU numerics tests: every HIP kernel vs the plain-PyTorch fp32 reference
(sat_amd.ops.functional).  bf16 kernels are compared against the fp32
reference computed on bf16-rounded inputs, with tolerances sized for one
bf16 rounding on inputs + fp32 accumulation in the kernel."""

import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from sat_amd.ops import functional as F
    from sat_amd.ops import hip

DEV = 'cuda'


def _bf(x):
    return x.to(DEV, torch.bfloat16)


def _rel_err(a, b):
    denom = b.float().abs().max().clamp_min(1e-6)
    return ((a.float() - b.float()).abs().max() / denom).item()


@pytest.mark.parametrize('M,N,K', [
    (128, 128, 64),      # single tile
    (6272, 512, 512),    # attention projection (B=32, L=196)
    (32, 2048, 1536),    # LSTM gates
    (32, 5000, 1024),    # decode logits (N edge: 5000 % 128 != 0)
    (100, 130, 72),      # everything-edge
    (1, 16, 8),          # degenerate
    (48, 320, 96),       # skinny RF=4 (16 masked rows), splitk 2
    (48, 296, 96),       # same, last block: partial wave + idle wave
    (128, 200, 160),     # skinny RF=8, partial last 16-column slab,
                         # splitk 4 with an empty fourth K-chunk
    (32, 64, 32),        # skinny splitk == 1 direct-store branch
])
@pytest.mark.parametrize('act', [None, 'tanh', 'relu'])
def test_dense_fwd(M, N, K, act):
    torch.manual_seed(0)
    x = _bf(torch.randn(M, K))
    w = _bf(torch.randn(N, K) * 0.05)
    b = _bf(torch.randn(N))
    y = hip.dense(x, w, b, act)
    ref = F.dense(x.float(), w.float(), b.float(), act)
    assert y.shape == (M, N)
    assert _rel_err(y, ref) < 2e-2


def test_dense_asymmetric_layout():
    """Catches transposed C-write / swapped operands (asymmetric B)."""
    M, N, K = 64, 48, 32
    x = torch.zeros(M, K)
    x[3, 5] = 1.0
    w = torch.zeros(N, K)
    w[7, 5] = 2.0
    w[7, 6] = 99.0  # must not contribute
    y = hip.dense(_bf(x), _bf(w), None, None).float().cpu()
    assert abs(y[3, 7].item() - 2.0) < 1e-3
    assert y.abs().sum().item() == pytest.approx(2.0, abs=1e-2)


def test_dense_backward():
    torch.manual_seed(1)
    M, N, K = 96, 64, 40
    x = _bf(torch.randn(M, K)).requires_grad_(True)
    w = _bf(torch.randn(N, K) * 0.1).requires_grad_(True)
    b = _bf(torch.randn(N)).requires_grad_(True)
    y = hip.dense(x, w, b, 'tanh')
    g = torch.randn_like(y)
    y.backward(g)

    xr = x.detach().float().requires_grad_(True)
    wr = w.detach().float().requires_grad_(True)
    br = b.detach().float().requires_grad_(True)
    F.dense(xr, wr, br, 'tanh').backward(g.float())
    assert _rel_err(x.grad, xr.grad) < 5e-2
    assert _rel_err(w.grad, wr.grad) < 5e-2
    assert _rel_err(b.grad, br.grad) < 5e-2


def test_lstm_cell_fwd_bwd():
    torch.manual_seed(2)
    B, I, H = 32, 1024, 512
    x = _bf(torch.randn(B, I)).requires_grad_(True)
    h = _bf(torch.randn(B, H)).requires_grad_(True)
    c = _bf(torch.randn(B, H)).requires_grad_(True)
    w = _bf(torch.randn(4 * H, I + H) * 0.02).requires_grad_(True)
    b = _bf(torch.zeros(4 * H)).requires_grad_(True)

    nh, nc = hip.lstm_cell(x, h, c, w, b)
    refs = [t.detach().float().requires_grad_(True)
            for t in (x, h, c, w, b)]
    rh, rc = F.lstm_cell(*refs)
    assert _rel_err(nh, rh) < 2e-2
    assert _rel_err(nc, rc) < 2e-2

    gh = torch.randn_like(nh)
    gc = torch.randn_like(nc)
    (nh.float() * gh.float()).sum().backward(retain_graph=True)
    (nc.float() * gc.float()).sum().backward()
    (rh * gh.float()).sum().backward(retain_graph=True)
    (rc * gc.float()).sum().backward()
    for t, r in zip((x, h, c, w), refs[:4]):
        assert _rel_err(t.grad, r.grad) < 5e-2


def _seed_dev():
    return torch.tensor(12345, dtype=torch.int64, device=DEV)


def test_attention_tail_fwd_bwd_nodrop():
    """p=0: exact comparison against the fp32 reference chain."""
    torch.manual_seed(3)
    B, L, A, D = 32, 196, 512, 512
    t1 = _bf(torch.randn(B * L, A)).requires_grad_(True)
    t2 = _bf(torch.randn(B, A)).requires_grad_(True)
    v = _bf(torch.randn(A) * 0.05).requires_grad_(True)
    ctx = _bf(torch.randn(B, L, D)).requires_grad_(True)

    alpha, pooled = hip.attention_tail(t1, t2, v, ctx, 0.0, _seed_dev(), 7)
    refs = [t.detach().float().requires_grad_(True)
            for t in (t1, t2, v, ctx)]
    ra, rp = F.attention_tail(*refs, 0.0, False)
    assert alpha.shape == (B, L)
    assert torch.allclose(alpha.sum(1),
                          torch.ones(B, device=DEV), atol=1e-4)
    assert _rel_err(alpha, ra) < 2e-2
    assert _rel_err(pooled, rp) < 2e-2

    ga = torch.randn_like(alpha)
    gp = torch.randn_like(pooled)
    (alpha * ga).sum().backward(retain_graph=True)
    (pooled.float() * gp.float()).sum().backward()
    (ra * ga).sum().backward(retain_graph=True)
    (rp * gp.float()).sum().backward()
    for t, r in zip((t1, v, ctx), (refs[0], refs[2], refs[3])):
        assert _rel_err(t.grad, r.grad) < 5e-2
    # t2's true gradient is ~0 at p=0 (softmax is shift-invariant in the
    # broadcast t2), so compare absolutely against the dt1 scale instead
    scale = t1.grad.float().abs().max().item()
    assert (t2.grad.float() - refs[1].grad).abs().max().item() \
        < 5e-2 * scale


def test_attention_tail_dropout_semantics():
    """p=0.5: mask statistics + fwd/bwd mask consistency."""
    torch.manual_seed(4)
    B, L, A, D = 8, 49, 512, 512
    p = 0.5
    t1 = _bf(torch.randn(B * L, A) + 3.0).requires_grad_(True)  # no 0s
    t2 = _bf(torch.randn(B, A)).requires_grad_(True)
    v = _bf(torch.ones(A) * 0.01).requires_grad_(True)
    ctx = _bf(torch.randn(B, L, D))
    seed = _seed_dev()

    alpha, pooled = hip.attention_tail(t1, t2, v, ctx, p, seed, 3)
    # recover tdrop from the saved forward by rerunning the scores kernel
    from sat_amd import _C
    tdrop, logits = _C.attn_scores_fused(
        t1.detach(), t2.detach(), v.detach(), seed, p, 3, L)
    kept = (tdrop != 0).float().mean().item()
    assert 0.45 < kept < 0.55
    # kept elements are scaled by 1/(1-p)
    full = (t1.detach().float().view(B * L, A)
            + t2.detach().float().repeat_interleave(L, dim=0))
    nz = tdrop != 0
    ratio = tdrop.float()[nz] / full[nz]
    assert (ratio - 2.0).abs().max().item() < 0.05

    # determinism: same seed+salt -> same mask; different salt -> different
    tdrop2, _ = _C.attn_scores_fused(
        t1.detach(), t2.detach(), v.detach(), seed, p, 3, L)
    assert torch.equal(tdrop, tdrop2)
    tdrop3, _ = _C.attn_scores_fused(
        t1.detach(), t2.detach(), v.detach(), seed, p, 4, L)
    assert not torch.equal(tdrop, tdrop3)

    # fwd/bwd mask consistency, with exactly recoverable masks:
    # t = 1 everywhere -> tdrop ∈ {0, 2}; dlogits = 1, v = 1 -> dt1 ∈ {0, 2}
    ones1 = torch.ones(B * L, A, device=DEV, dtype=torch.bfloat16)
    zeros2 = torch.zeros(B, A, device=DEV, dtype=torch.bfloat16)
    vones = torch.ones(A, device=DEV, dtype=torch.bfloat16)
    td, _ = _C.attn_scores_fused(ones1, zeros2, vones, seed, p, 9, L)
    dl = torch.ones(B, L, device=DEV)
    dt1b, _, _ = _C.attn_scores_bwd(td, vones, dl, seed, p, 9, L)
    assert torch.equal(td != 0, dt1b != 0)


def test_attention_pool_small_l():
    """ResNet50 grid: L=49."""
    B, L, D = 4, 49, 2048
    ctx = _bf(torch.randn(B, L, D))
    logits = torch.randn(B, L, device=DEV)
    alpha, pooled = hip.attention_pool(ctx, logits)
    ra, rp = F.attention_pool(ctx.float(), logits)
    assert _rel_err(alpha, ra) < 1e-2
    assert _rel_err(pooled, rp) < 2e-2


def test_embedding_fwd_bwd():
    torch.manual_seed(4)
    V, E, B = 5000, 512, 64
    table = _bf(torch.randn(V, E)).requires_grad_(True)
    ids = torch.randint(0, V, (B,), device=DEV)
    ids[0] = ids[1]  # duplicate: scatter-add must accumulate
    out = hip.embedding(ids, table)
    assert torch.equal(out[0], out[1])
    g = torch.randn_like(out)
    out.backward(g)
    ref = torch.zeros(V, E, device=DEV)
    ref.index_add_(0, ids, g.float())
    assert _rel_err(table.grad, ref) < 2e-2


def test_masked_ce_fwd_bwd():
    torch.manual_seed(5)
    B, V = 640, 5000
    logits = _bf(torch.randn(B, V)).requires_grad_(True)
    labels = torch.randint(0, V, (B,), device=DEV)
    mask = (torch.rand(B, device=DEV) > 0.3).float()
    ce = hip.masked_softmax_ce(logits, labels, mask)
    lr = logits.detach().float().requires_grad_(True)
    ref = F.masked_softmax_ce(lr, labels, mask)
    assert _rel_err(ce, ref) < 1e-2
    assert (ce[mask == 0].abs() < 1e-6).all()

    ce.sum().backward()
    ref.sum().backward()
    assert _rel_err(logits.grad, lr.grad) < 5e-2


def test_adam_fused_matches_eager():
    torch.manual_seed(6)
    shapes = [(1000,), (64, 32), (5000, 16)]
    params = [torch.randn(s, device=DEV) for s in shapes]
    grads = [torch.randn(s, device=DEV) * 3 for s in shapes]
    ms = [torch.zeros(s, device=DEV) for s in shapes]
    vs = [torch.zeros(s, device=DEV) for s in shapes]
    p_ref = [p.clone() for p in params]

    lr, b1, b2, eps, clip = 1e-3, 0.9, 0.999, 1e-6, 5.0
    gsq = hip.grad_sq_norm(grads)
    norm_ref = torch.sqrt(sum((g ** 2).sum() for g in grads))
    assert _rel_err(gsq.sqrt(), norm_ref) < 1e-4

    step_dev = torch.ones((), device=DEV)
    hip.adam_step(params, grads, ms, vs, step_dev, lr, 1.0, 1e5,
                  b1, b2, eps, clip, gsq)

    scale = min(1.0, clip / norm_ref.item())
    for p, g in zip(p_ref, grads):
        gc = g * scale
        m = (1 - b1) * gc
        v = (1 - b2) * gc * gc
        mh = m / (1 - b1)
        vh = v / (1 - b2)
        p -= lr * mh / (vh.sqrt() + eps)
    for p, r in zip(params, p_ref):
        assert _rel_err(p, r) < 1e-4


def test_fused_optimizer_in_training(tiny_config):
    """Full Optimizer.step on GPU uses the fused kernels end-to-end."""
    from sat_amd.optim import Optimizer
    from config import Config
    cfg = Config()
    p = torch.nn.Parameter(torch.randn(100, device=DEV))
    opt = Optimizer(cfg, [p])
    p.grad = torch.randn(100, device=DEV)
    before = p.detach().clone()
    opt.step()
    torch.cuda.synchronize()
    assert not torch.equal(before, p.detach())
    assert torch.isfinite(p).all()


def test_conv3_fwd_matches_torch():
    """Direct NHWC conv1_1 kernel vs torch.conv2d (fp32 reference)."""
    from sat_amd import _C
    torch.manual_seed(7)
    B, H, W, C = 4, 57, 61, 64  # odd sizes exercise the halo guards
    x = torch.randn(B, 3, H, W).to(DEV, torch.bfloat16) \
        .contiguous(memory_format=torch.channels_last)
    w = (torch.randn(C, 3, 3, 3) * 0.2).to(DEV, torch.bfloat16)
    b = torch.randn(C).to(DEV, torch.bfloat16)
    y = _C.conv3_fwd(x, w, b, True, False)
    ref = torch.relu(torch.nn.functional.conv2d(
        x.float(), w.float(), b.float(), padding=1))
    assert y.shape == ref.shape
    assert _rel_err(y, ref) < 2e-2


def test_conv3_fwd_no_bias_no_relu():
    from sat_amd import _C
    x = torch.randn(2, 3, 16, 16).to(DEV, torch.bfloat16) \
        .contiguous(memory_format=torch.channels_last)
    w = (torch.randn(8, 3, 3, 3) * 0.2).to(DEV, torch.bfloat16)
    y = _C.conv3_fwd(x, w, torch.empty(0, dtype=torch.bfloat16,
                                       device=DEV), False, False)
    ref = torch.nn.functional.conv2d(x.float(), w.float(), padding=1)
    assert _rel_err(y, ref) < 2e-2


def test_bias_act_nhwc():
    from sat_amd import _C
    torch.manual_seed(8)
    y = torch.randn(2, 16, 7, 9).to(DEV, torch.bfloat16) \
        .contiguous(memory_format=torch.channels_last)
    b = torch.randn(16).to(DEV, torch.bfloat16)
    ref = torch.relu(y.float() + b.float().reshape(1, -1, 1, 1))
    _C.bias_act_nhwc(y, b, True)
    assert _rel_err(y, ref) < 1e-2


def test_maxpool2x2_nhwc():
    from sat_amd import _C
    for H, W in [(8, 8), (7, 9)]:
        x = torch.randn(2, 16, H, W).to(DEV, torch.bfloat16) \
            .contiguous(memory_format=torch.channels_last)
        y = _C.maxpool2x2_nhwc(x)
        ref = torch.nn.functional.max_pool2d(
            x.float(), 2, 2, ceil_mode=True)
        assert y.shape == ref.shape
        assert _rel_err(y, ref) < 1e-3


def test_conv_igemm_matches_torch():
    from sat_amd import _C
    torch.manual_seed(9)
    for Cin, Cout, H in [(64, 64, 30), (64, 128, 17), (128, 64, 9)]:
        x = torch.randn(2, Cin, H, H).to(DEV, torch.bfloat16) \
            .contiguous(memory_format=torch.channels_last)
        w = (torch.randn(Cout, Cin, 3, 3) * 0.05).to(DEV, torch.bfloat16)
        b = torch.randn(Cout).to(DEV, torch.bfloat16)
        w_ohwi = w.permute(0, 2, 3, 1).contiguous().reshape(Cout, -1)
        y = _C.conv_igemm_fwd(x, w_ohwi, b, True)
        ref = torch.relu(torch.nn.functional.conv2d(
            x.float(), w.float(), b.float(), padding=1))
        assert _rel_err(y, ref) < 2e-2, (Cin, Cout, H)


def test_conv_igemm_glds_matches_torch():
    from sat_amd import _C
    torch.manual_seed(10)
    for Cin, Cout, H, W in [(64, 128, 19, 23), (128, 128, 14, 14),
                            (128, 256, 9, 31)]:
        x = torch.randn(2, Cin, H, W).to(DEV, torch.bfloat16) \
            .contiguous(memory_format=torch.channels_last)
        w = (torch.randn(Cout, Cin, 3, 3) * 0.05).to(DEV, torch.bfloat16)
        b = torch.randn(Cout).to(DEV, torch.bfloat16)
        w_ohwi = w.permute(0, 2, 3, 1).contiguous().reshape(Cout, -1)
        xp = _C.pad1_nhwc(x)
        y = _C.conv_igemm_glds_fwd(xp, w_ohwi, b, H, W, True)
        ref = torch.relu(torch.nn.functional.conv2d(
            x.float(), w.float(), b.float(), padding=1))
        assert _rel_err(y, ref) < 2e-2, (Cin, Cout, H, W)


def test_conv_igemm_8p_matches_torch():
    """8-phase pipelined igemm (conv8p.hip) vs fp32 torch conv.  Shapes
    cover: M % 256 != 0 (edge-clamp rows), Cout 256 and 512, Cin 64..512,
    and non-square H/W."""
    from sat_amd import _C
    torch.manual_seed(11)
    for Cin, Cout, B, H, W in [(64, 256, 2, 17, 19), (128, 256, 3, 16, 16),
                               (256, 512, 2, 14, 14), (512, 512, 1, 28, 28)]:
        x = torch.randn(B, Cin, H, W).to(DEV, torch.bfloat16) \
            .contiguous(memory_format=torch.channels_last)
        w = (torch.randn(Cout, Cin, 3, 3) * 0.05).to(DEV, torch.bfloat16)
        b = torch.randn(Cout).to(DEV, torch.bfloat16)
        w_ohwi = w.permute(0, 2, 3, 1).contiguous().reshape(Cout, -1)
        xp = _C.pad1_nhwc(x)
        y = _C.conv_igemm_8p_fwd(xp, w_ohwi, b, H, W, True)
        ref = torch.relu(torch.nn.functional.conv2d(
            x.float(), w.float(), b.float(), padding=1))
        assert _rel_err(y, ref) < 2e-2, (Cin, Cout, B, H, W)


def test_conv_igemm_8p_race_screen():
    """Sync-structure discipline (CDNA4 guide §5.4): a new pipelined
    schedule needs a multi-run race screen — same inputs, repeated
    launches, every run must agree with the fp32 reference."""
    from sat_amd import _C
    torch.manual_seed(12)
    Cin, Cout, B, H, W = (256, 256, 2, 23, 29)
    x = torch.randn(B, Cin, H, W).to(DEV, torch.bfloat16) \
        .contiguous(memory_format=torch.channels_last)
    w = (torch.randn(Cout, Cin, 3, 3) * 0.05).to(DEV, torch.bfloat16)
    b = torch.randn(Cout).to(DEV, torch.bfloat16)
    w_ohwi = w.permute(0, 2, 3, 1).contiguous().reshape(Cout, -1)
    ref = torch.relu(torch.nn.functional.conv2d(
        x.float(), w.float(), b.float(), padding=1))
    xp = _C.pad1_nhwc(x)
    for run in range(6):
        y = _C.conv_igemm_8p_fwd(xp, w_ohwi, b, H, W, True)
        assert _rel_err(y, ref) < 2e-2, 'race screen run %d' % run


def test_conv3x3_wgrad_matches_torch():
    from sat_amd import _C
    torch.manual_seed(13)
    for Cin, Cout, B, H, W in [(64, 64, 2, 14, 14), (128, 256, 2, 9, 11),
                               (64, 128, 3, 16, 16)]:
        x = torch.randn(B, Cin, H, W).to(DEV, torch.bfloat16) \
            .contiguous(memory_format=torch.channels_last)
        dy = torch.randn(B, Cout, H, W).to(DEV, torch.bfloat16) \
            .contiguous(memory_format=torch.channels_last)
        xpad = _C.pad1_nhwc(x)
        dy_rows = dy.permute(0, 2, 3, 1).reshape(B * H * W, Cout)
        dwf = _C.conv3x3_wgrad(xpad, dy_rows, H, W)
        got = dwf.reshape(Cout, 3, 3, Cin).permute(0, 3, 1, 2)
        xr = x.float().detach().requires_grad_(True)
        wr = torch.zeros(Cout, Cin, 3, 3, device=DEV,
                         requires_grad=True)
        torch.nn.functional.conv2d(xr, wr, padding=1) \
            .backward(dy.float())
        assert _rel_err(got, wr.grad) < 2e-2, (Cin, Cout, B, H, W)


def test_conv3x3_train_function_grads():
    """Full autograd triple (fwd + dgrad + wgrad + dbias + fused ReLU)
    vs fp32 torch reference."""
    from sat_amd.ops.convgrad import Conv3x3Train
    torch.manual_seed(14)
    for Cin, Cout, B, H, W, relu in [(64, 128, 2, 14, 14, True),
                                     (128, 256, 2, 16, 16, True),
                                     (256, 512, 1, 14, 14, False)]:
        x0 = torch.randn(B, Cin, H, W) * 0.5
        w0 = torch.randn(Cout, Cin, 3, 3) * 0.05
        b0 = torch.randn(Cout) * 0.1
        dy0 = torch.randn(B, Cout, H, W)

        x = x0.to(DEV, torch.bfloat16) \
            .contiguous(memory_format=torch.channels_last) \
            .requires_grad_(True)
        w = w0.to(DEV, torch.bfloat16) \
            .contiguous(memory_format=torch.channels_last) \
            .requires_grad_(True)
        b = b0.to(DEV, torch.bfloat16).requires_grad_(True)
        y = Conv3x3Train.apply(x, w, b, relu)
        y.backward(dy0.to(DEV, torch.bfloat16)
                   .contiguous(memory_format=torch.channels_last))

        xr = x0.to(DEV).requires_grad_(True)
        wr = w0.to(DEV).requires_grad_(True)
        br = b0.to(DEV).requires_grad_(True)
        yr = torch.nn.functional.conv2d(xr, wr, br, padding=1)
        dy_ref = dy0.to(DEV)
        if relu:
            # use OUR kernel's bf16 ReLU mask in the fp32 reference:
            # elements with y ~ 0 flip sides of the threshold under bf16
            # rounding, which is a representation artifact, not a grad
            # bug — a mask-consistent reference isolates the real math
            dy_ref = dy_ref * (y.float() > 0)
            assert _rel_err(y, torch.relu(yr)) < 2e-2
        else:
            assert _rel_err(y, yr) < 2e-2
        yr.backward(dy_ref)

        assert _rel_err(x.grad, xr.grad) < 3e-2, (Cin, Cout, relu)
        assert _rel_err(w.grad, wr.grad) < 3e-2, (Cin, Cout, relu)
        assert _rel_err(b.grad, br.grad) < 3e-2, (Cin, Cout, relu)


def test_conv_igemm_glds64_matches_torch():
    from sat_amd import _C
    torch.manual_seed(15)
    for Cin, Cout, B, H, W in [(64, 64, 2, 19, 17), (128, 64, 2, 14, 14),
                               (64, 128, 1, 23, 23)]:
        x = torch.randn(B, Cin, H, W).to(DEV, torch.bfloat16) \
            .contiguous(memory_format=torch.channels_last)
        w = (torch.randn(Cout, Cin, 3, 3) * 0.05).to(DEV, torch.bfloat16)
        b = torch.randn(Cout).to(DEV, torch.bfloat16)
        w_ohwi = w.permute(0, 2, 3, 1).contiguous().reshape(Cout, -1)
        xp = _C.pad1_nhwc(x)
        y = _C.conv_igemm_glds64_fwd(xp, w_ohwi, b, H, W, True)
        ref = torch.relu(torch.nn.functional.conv2d(
            x.float(), w.float(), b.float(), padding=1))
        assert _rel_err(y, ref) < 2e-2, (Cin, Cout, B, H, W)


def test_conv3_fwd_emit_pad_and_glds64_chain():
    """conv1_1 emitting a zero-bordered padded output that conv1_2
    (glds64) consumes directly — the chained-pad fast path."""
    from sat_amd import _C
    torch.manual_seed(16)
    B, H, W = 2, 20, 24
    x = torch.randn(B, 3, H, W).to(DEV, torch.bfloat16) \
        .contiguous(memory_format=torch.channels_last)
    w1 = (torch.randn(64, 3, 3, 3) * 0.2).to(DEV, torch.bfloat16)
    b1 = torch.randn(64).to(DEV, torch.bfloat16)
    w2 = (torch.randn(64, 64, 3, 3) * 0.05).to(DEV, torch.bfloat16)
    b2 = torch.randn(64).to(DEV, torch.bfloat16)

    yp = _C.conv3_fwd(x, w1, b1, True, True)
    assert yp.shape == (B, 64, H + 2, W + 2)
    # border must be exactly zero
    assert float(yp[:, :, 0, :].float().abs().max()) == 0.0
    assert float(yp[:, :, :, -1].float().abs().max()) == 0.0
    # interior equals the unpadded conv
    y0 = _C.conv3_fwd(x, w1, b1, True, False)
    assert torch.equal(yp[:, :, 1:H + 1, 1:W + 1], y0)

    w2_ohwi = w2.permute(0, 2, 3, 1).contiguous().reshape(64, -1)
    y2 = _C.conv_igemm_glds64_fwd(yp, w2_ohwi, b2, H, W, True)
    ref = torch.relu(torch.nn.functional.conv2d(
        y0.float(), w2.float(), b2.float(), padding=1))
    assert _rel_err(y2, ref) < 2e-2


def test_conv1x1_as_gemm_route():
    """ResNet bottleneck 1x1 convs route through the tiled MFMA GEMM."""
    import torch.nn as tnn
    from config import Config
    from sat_amd.models.nn import NN, Conv2d
    cfg = Config()
    cfg.phase = 'eval'
    pol = NN(cfg)
    torch.manual_seed(17)
    for Cin, Cout, relu in [(64, 256, True), (256, 64, False)]:
        conv = Conv2d(pol, Cin, Cout, 1, 1,
                      'relu' if relu else None, use_bias=False)
        conv = conv.to(DEV)
        x = torch.randn(2, Cin, 14, 14).to(DEV, torch.bfloat16) \
            .contiguous(memory_format=torch.channels_last)
        with torch.no_grad():
            y = conv(x)
            ref = torch.nn.functional.conv2d(
                x.float(), conv.weight.float())
            if relu:
                ref = torch.relu(ref)
        assert _rel_err(y, ref) < 2e-2, (Cin, Cout)


# ---- every r02 fusion vs the kernel pair it replaced ----
# Outputs whose math is identical must match BITWISE (dropout masks
# especially — backward regenerates them from the same counter hash).
# Outputs where the fusion keeps fp32 through a stage the pair rounds to
# bf16 (e.g. dxh, h_raw, dt1 intermediates) may differ by ONE bf16
# rounding — the fused value is the more accurate one.

def _one_ulp(a, b):
    # bounded by one bf16 rounding of the pair's intermediate, scaled to
    # the tensor's magnitude (a relative bound would be wrong under
    # cancellation: x*scale + y with y ~ -x*scale keeps the
    # intermediate's absolute rounding while the result is ~0)
    fa, fb = a.float(), b.float()
    tol = float(fb.abs().max()) * (2.0 ** -7) + 1e-6
    assert float((fa - fb).abs().max()) <= tol


def _fuse_seed():
    return torch.tensor(777, dtype=torch.int64, device=DEV)


def _empty_bf(*shape):
    return torch.empty(*shape, dtype=torch.bfloat16, device=DEV)


_P_FC, _P_LSTM, _SALT = 0.5, 0.3, 48

# (B,H,D,E): the flagship step; then H=D=E=64, where the gates GEMM has
# K=192, N=256 -> splitk 4 with a 64-wide chunk, so the fourth K-chunk is
# empty and its slab must come out as zeros — at B=33 (RF=4, 31 masked
# rows) and B=128 (RF=8 full)
_fuse_shapes = pytest.mark.parametrize('B,H,D,E', [
    (32, 512, 512, 512), (33, 64, 64, 64), (128, 64, 64, 64)])


@_fuse_shapes
def test_dense_fwd_drop_matches_pair_bitwise(B, H, D, E):
    """dense_fwd_drop == dense_fwd + hash_dropout"""
    from sat_amd import _C
    torch.manual_seed(33)
    A = 512
    seed = _fuse_seed()
    x = _bf(torch.randn(B, A))
    w = _bf(torch.randn(H, A) * 0.05)
    y1 = _C.dense_fwd_drop(x, w, seed, _P_FC, _SALT + 1)
    y2 = _C.hash_dropout(_C.dense_fwd(x, w, _empty_bf(0), 0), seed,
                         _P_FC, _SALT + 1)
    assert torch.equal(y1, y2)


def test_dense_fwd_drop_single_split_bitwise():
    """K=32 leaves the skinny plan at splitk == 1: the fused entry point
    still runs the GEMM in slab mode (one slab) under its own epilogue."""
    from sat_amd import _C
    torch.manual_seed(34)
    seed = _fuse_seed()
    x = _bf(torch.randn(32, 32))
    w = _bf(torch.randn(72, 32) * 0.05)
    y1 = _C.dense_fwd_drop(x, w, seed, _P_FC, _SALT + 1)
    y2 = _C.hash_dropout(_C.dense_fwd(x, w, _empty_bf(0), 0), seed,
                         _P_FC, _SALT + 1)
    assert torch.equal(y1, y2)


@_fuse_shapes
def test_dense_dx_fuse_matches_pair(B, H, D, E):
    """dense_dx_fuse == dense_fwd + dx_fuse"""
    from sat_amd import _C
    torch.manual_seed(35)
    I = D + E
    seed = _fuse_seed()
    dgates = _bf(torch.randn(B, 4 * H) * 0.1)
    wl_t = _bf(torch.randn(I + H, 4 * H) * 0.05)
    dpool_dec = _bf(torch.randn(B, D))
    demb_dec = _bf(torch.randn(B, E))
    demb1 = _empty_bf(B, E)
    demb2 = _empty_bf(B, E)
    dp1, ds1 = _C.dense_dx_fuse(dgates, wl_t, dpool_dec, demb_dec,
                                seed, demb1, _P_LSTM, _SALT + 3, D, E, H)
    dxh = _C.dense_fwd(dgates, wl_t, _empty_bf(0), 0)
    dp2, ds2 = _C.dx_fuse(dxh, dpool_dec, demb_dec, seed, demb2,
                          _P_LSTM, _SALT + 3, H)
    _one_ulp(dp1, dp2)       # pair rounds dxh to bf16 first
    _one_ulp(ds1, ds2)
    _one_ulp(demb1, demb2)


@_fuse_shapes
def test_dense_lstm_expand_fwd_matches_pair(B, H, D, E):
    """dense_lstm_expand_fwd == dense_lstm_fwd + expand_fuse"""
    from sat_amd import _C
    torch.manual_seed(36)
    V_ = 1000
    I = D + E
    W = H + D + E
    seed = _fuse_seed()
    xh = _bf(torch.randn(B, I + H) * 0.1)
    wl = _bf(torch.randn(4 * H, I + H) * 0.05)
    bl = _bf(torch.zeros(4 * H))
    cprev = _bf(torch.randn(B, H))
    pooled = _bf(torch.randn(B, D))
    table = _bf(torch.randn(V_, E))
    ids = torch.randint(0, V_, (B,), device=DEV)
    e1, e2 = _empty_bf(B, W), _empty_bf(B, W)
    od1, od2 = _empty_bf(B, H), _empty_bf(B, H)
    g1, c1, sth1 = _C.dense_lstm_expand_fwd(
        xh, wl, bl, cprev, pooled, table, ids, seed, e1, od1,
        1.0, _P_LSTM, _P_FC, _SALT)
    g2, h2, c2 = _C.dense_lstm_fwd(xh, wl, bl, cprev, 1.0)
    _out2, sth2 = _C.expand_fuse(h2, pooled, table, ids, seed, e2, od2,
                                 _P_LSTM, _P_FC, _SALT)
    assert torch.equal(g1, g2)   # identical fp32 math, rounded once
    assert torch.equal(c1, c2)
    _one_ulp(sth1, sth2)         # pair rounds h_raw to bf16 first
    _one_ulp(e1, e2)
    _one_ulp(od1, od2)


@_fuse_shapes
def test_dexp_lstm_bwd_matches_pair(B, H, D, E):
    """dexp_lstm_bwd == dexp_fuse + lstm_pointwise_bwd_out"""
    from sat_amd import _C
    torch.manual_seed(37)
    W = H + D + E
    seed = _fuse_seed()
    gates = _bf(torch.randn(B, 4 * H))
    cprev = _bf(torch.randn(B, H))
    dexpd = _bf(torch.randn(B, W) * 0.1)
    doc = _bf(torch.randn(B, H) * 0.1)
    dsc = _bf(torch.randn(B, H) * 0.1)
    dcc = _bf(torch.randn(B, H) * 0.1)
    DG1 = _empty_bf(B, 4 * H)
    DG2 = _empty_bf(B, 4 * H)
    dcp1, dpd1, ded1 = _C.dexp_lstm_bwd(
        dexpd, doc, dsc, seed, gates, cprev, dcc, DG1,
        _P_FC, _P_LSTM, _SALT, D, E, 1.0)
    dh2, dpd2, ded2 = _C.dexp_fuse(dexpd, doc, dsc, seed, _P_FC, _P_LSTM,
                                   _SALT, D, E)
    dg2, dcp2 = _C.lstm_pointwise_bwd_out(gates, cprev, dh2, dcc, 1.0, DG2)
    _one_ulp(DG1, DG2)           # pair rounds dh_raw to bf16 first
    _one_ulp(dcp1, dcp2)
    assert torch.equal(dpd1, dpd2)   # same single-rounding math
    assert torch.equal(ded1, ded2)


def test_attn_scores_bwd_tanh_matches_pair():
    """attn_scores_bwd_tanh == attn_scores_bwd_acc + act_bwd_out"""
    from sat_amd import _C
    torch.manual_seed(38)
    B, A, L = 32, 512, 196
    seed = _fuse_seed()
    t1y = _bf(torch.tanh(torch.randn(B * L, A)))
    tdrop = _bf(torch.randn(B * L, A))
    dlog = torch.randn(B, L, device=DEV)
    vvec = _bf(torch.randn(A) * 0.05)
    dv1 = torch.zeros(A, dtype=torch.float32, device=DEV)
    dv2 = torch.zeros(A, dtype=torch.float32, device=DEV)
    out1 = _empty_bf(B * L, A)
    _d1, dt2a, _ = _C.attn_scores_bwd_tanh(
        tdrop, vvec, dlog, seed, _P_FC, _SALT + 2, L, dv1, t1y, out1)
    dt1b, dt2b, _ = _C.attn_scores_bwd_acc(
        tdrop, vvec, dlog, seed, _P_FC, _SALT + 2, L, dv2)
    out2 = torch.empty_like(out1)
    _C.act_bwd_out(dt1b, t1y, 1, out2)
    _one_ulp(out1, out2)         # pair rounds dt1 to bf16 first
    # dt2/dv are fp32 atomicAdd accumulations across l-chunk blocks:
    # summation order is nondeterministic between runs, so two
    # IDENTICAL kernels differ in the last ulps — compare to fp32
    # accumulation-order tolerance
    assert torch.allclose(dt2a, dt2b, rtol=1e-4, atol=1e-4)
    assert torch.allclose(dv1, dv2, rtol=1e-4, atol=1e-4)


def test_dense_8p_matches_torch_and_is_race_stable():
    """8-phase dense GEMM (gemm8p.hip): numerics vs fp32 torch on edge
    shapes + repeated-launch race screen (new-template discipline)."""
    from sat_amd import _C
    torch.manual_seed(44)
    for M, N, K, act in [(300, 512, 512, 0), (257, 256, 128, 1),
                         (1024, 520, 192, 2)]:
        x = _bf(torch.randn(M, K))
        w = _bf(torch.randn(N, K) * 0.05)
        b = _bf(torch.randn(N))
        ref = x.float() @ w.float().t() + b.float()
        if act == 1:
            ref = torch.tanh(ref)
        elif act == 2:
            ref = torch.relu(ref)
        for run in range(5):
            y = _C.dense_8p_fwd(x, w, b, act)
            assert _rel_err(y, ref) < 2e-2, (M, N, K, act, run)
