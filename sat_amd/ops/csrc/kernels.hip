// Fused pointwise / reduction kernels of the decoder hot path (gfx950).
//
// Covers the non-GEMM rows of the reference's implicit kernel surface
// (SURVEY.md §2.3): LSTM gate fusion, the LDS-staged 196-location attention
// softmax + weighted context sum, embedding gather/scatter-grad, fused
// masked softmax cross-entropy, and the fused global-norm-clipped Adam.

#include "common.h"

// ======================================================================
// LSTM gate fusion (TF LSTMCell semantics: gate order i,j,f,o; forget
// bias added pre-sigmoid; no peepholes).  gates: [B,4H] from the GEMM.
// ======================================================================

__global__ void lstm_pw_fwd_kernel(const bf16* __restrict__ gates,
                                   const bf16* __restrict__ c,
                                   bf16* __restrict__ h_out,
                                   bf16* __restrict__ c_out,
                                   int B, int H, float fb) {
    int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= B * H) return;
    int b = idx / H, hh = idx % H;
    const bf16* gp = gates + (int64_t)b * 4 * H + hh;
    float g[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) g[q] = bf2f(gp[q * H]);
    float cn, h;
    lstm_cell_fwd(g, bf2f(c[idx]), fb, cn, h);
    h_out[idx] = f2bf(h);
    c_out[idx] = f2bf(cn);
}

__global__ void lstm_pw_bwd_kernel(const bf16* __restrict__ gates,
                                   const bf16* __restrict__ c,
                                   const bf16* __restrict__ dh,
                                   const bf16* __restrict__ dc,
                                   bf16* __restrict__ dgates,
                                   bf16* __restrict__ dc_prev,
                                   int B, int H, float fb) {
    int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= B * H) return;
    int b = idx / H, hh = idx % H;
    const bf16* gp = gates + (int64_t)b * 4 * H + hh;
    float g[4], dg[4], dcp;
#pragma unroll
    for (int q = 0; q < 4; ++q) g[q] = bf2f(gp[q * H]);
    float dcv = (dc != nullptr) ? bf2f(dc[idx]) : 0.f;
    lstm_cell_bwd(g, bf2f(c[idx]), bf2f(dh[idx]), dcv, fb, dg, dcp);
    bf16* dgp = dgates + (int64_t)b * 4 * H + hh;
#pragma unroll
    for (int q = 0; q < 4; ++q) dgp[q * H] = f2bf(dg[q]);
    dc_prev[idx] = f2bf(dcp);
}

std::vector<at::Tensor> lstm_pointwise_fwd(at::Tensor gates, at::Tensor c,
                                           double fb) {
    CHECK_GPU(gates); CHECK_CONTIG(gates); CHECK_BF16(gates);
    CHECK_GPU(c); CHECK_CONTIG(c); CHECK_BF16(c);
    int B = c.size(0), H = c.size(1);
    TORCH_CHECK(gates.size(0) == B && gates.size(1) == 4 * H);
    auto h_out = at::empty_like(c);
    auto c_out = at::empty_like(c);
    int n = B * H;
    hipStream_t s = at::cuda::getCurrentCUDAStream();
    hipLaunchKernelGGL(lstm_pw_fwd_kernel, dim3(cdiv(n, 256)), dim3(256), 0, s,
                       (const bf16*)gates.data_ptr(), (const bf16*)c.data_ptr(),
                       (bf16*)h_out.data_ptr(), (bf16*)c_out.data_ptr(),
                       B, H, (float)fb);
    HIP_OK(hipGetLastError());
    return {h_out, c_out};
}

std::vector<at::Tensor> lstm_pointwise_bwd_out(at::Tensor gates,
                                               at::Tensor c, at::Tensor dh,
                                               at::Tensor dc, double fb,
                                               at::Tensor dgates_out) {
    CHECK_GPU(gates); CHECK_CONTIG(gates); CHECK_BF16(gates);
    int B = c.size(0), H = c.size(1);
    at::Tensor dgates;
    if (dgates_out.defined() && dgates_out.numel() > 0)
        dgates = dgates_out;
    else
        dgates = at::empty_like(gates);
    auto dc_prev = at::empty_like(c);
    const bf16* dc_ptr = nullptr;
    if (dc.defined() && dc.numel() > 0) dc_ptr = (const bf16*)dc.data_ptr();
    int n = B * H;
    hipStream_t s = at::cuda::getCurrentCUDAStream();
    hipLaunchKernelGGL(lstm_pw_bwd_kernel, dim3(cdiv(n, 256)), dim3(256), 0, s,
                       (const bf16*)gates.data_ptr(), (const bf16*)c.data_ptr(),
                       (const bf16*)dh.data_ptr(), dc_ptr,
                       (bf16*)dgates.data_ptr(), (bf16*)dc_prev.data_ptr(),
                       B, H, (float)fb);
    HIP_OK(hipGetLastError());
    return {dgates, dc_prev};
}

std::vector<at::Tensor> lstm_pointwise_bwd(at::Tensor gates, at::Tensor c,
                                           at::Tensor dh, at::Tensor dc,
                                           double fb) {
    return lstm_pointwise_bwd_out(gates, c, dh, dc, fb, at::Tensor());
}

// ======================================================================
// Activation backward: dpre = dy * act'(y) in ONE kernel (the eager chain
// y.float / 1-y^2 / mul / cast is 4 launches per dense backward).
// ======================================================================

__global__ void act_bwd_kernel(const bf16* __restrict__ dy,
                               const bf16* __restrict__ y,
                               bf16* __restrict__ dpre,
                               int64_t n, int act) {
    int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n) return;
    float g = bf2f(dy[idx]);
    float yv = bf2f(y[idx]);
    if (act == 1) g *= (1.f - yv * yv);        // tanh'
    else if (act == 2) g *= (yv > 0.f ? 1.f : 0.f);  // relu'
    dpre[idx] = f2bf(g);
}

at::Tensor act_bwd(at::Tensor dy, at::Tensor y, int64_t act) {
    CHECK_GPU(dy); CHECK_CONTIG(dy); CHECK_BF16(dy);
    CHECK_GPU(y); CHECK_CONTIG(y); CHECK_BF16(y);
    auto dpre = at::empty_like(dy);
    int64_t n = dy.numel();
    hipStream_t s = at::cuda::getCurrentCUDAStream();
    hipLaunchKernelGGL(act_bwd_kernel, dim3(cdiv(n, 256)), dim3(256), 0, s,
                       (const bf16*)dy.data_ptr(), (const bf16*)y.data_ptr(),
                       (bf16*)dpre.data_ptr(), n, (int)act);
    HIP_OK(hipGetLastError());
    return dpre;
}

// ======================================================================
// Attention: scores GEMV (temp[M,A] @ v[A] -> logits[M]) and the fused
// LDS-staged softmax-over-L + weighted context sum (model.py:435,263-264).
// ======================================================================

#define MAX_L 1024

// ---- generic counter-based dropout (used by the hand-written BPTT) ----
// The counter hash of common.h: y = x * mask(seed,salt,idx)/(1-p).
// Forward and backward are the same kernel (masks regenerate exactly).

__global__ void hash_dropout_kernel(const bf16* __restrict__ x,
                                    const int64_t* __restrict__ seed_p,
                                    bf16* __restrict__ y,
                                    int64_t n, float p, int salt) {
    const uint32_t seed = (uint32_t)(*seed_p);
    int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = idx * 8; i < n; i += stride * 8) {
        if (i + 8 <= n) {
            bf16x8 v = *(const bf16x8*)(x + i);
            bf16x8 o;
#pragma unroll
            for (int e = 0; e < 8; ++e)
                o[e] = f2bf(bf2f(v[e]) *
                            drop_scale(seed, salt, (uint32_t)(i + e), p));
            *(bf16x8*)(y + i) = o;
        } else {
            for (int64_t j = i; j < n; ++j)
                y[j] = f2bf(bf2f(x[j]) *
                            drop_scale(seed, salt, (uint32_t)j, p));
        }
    }
}

at::Tensor hash_dropout(at::Tensor x, at::Tensor seed, double p,
                        int64_t salt) {
    CHECK_GPU(x); CHECK_CONTIG(x); CHECK_BF16(x);
    if (p <= 0.0) return x;
    auto y = at::empty_like(x);
    int64_t n = x.numel();
    int blocks = (int)std::min<int64_t>(cdiv(n, 256 * 8), 4096);
    hipStream_t s = at::cuda::getCurrentCUDAStream();
    hipLaunchKernelGGL(hash_dropout_kernel, dim3(blocks), dim3(256), 0, s,
                       (const bf16*)x.data_ptr(),
                       (const int64_t*)seed.data_ptr(),
                       (bf16*)y.data_ptr(), n, (float)p, (int)salt);
    HIP_OK(hipGetLastError());
    return y;
}

// ---- fused attention scores: t = dropout(t1 + t2), logits = t·v ----
// t1: [B·L, A], t2: [B, A], v: [A]; writes tdrop (saved for dv in bwd)
// and logits [B·L] fp32.  One wave per row.

__global__ void attn_scores_fused_kernel(
        const bf16* __restrict__ t1, const bf16* __restrict__ t2,
        const bf16* __restrict__ v, const int64_t* __restrict__ seed_p,
        bf16* __restrict__ tdrop, float* __restrict__ logits,
        int B, int L, int A, float p, int salt) {
    const uint32_t seed = (uint32_t)(*seed_p);
    int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= B * L) return;
    int lane = threadIdx.x & 63;
    int b = row / L;
    const bf16* t1r = t1 + (int64_t)row * A;
    const bf16* t2r = t2 + (int64_t)b * A;
    bf16* tdr = tdrop + (int64_t)row * A;
    float acc = 0.f;
    for (int a0 = lane * 8; a0 + 8 <= A; a0 += 64 * 8) {
        bf16x8 x1 = *(const bf16x8*)(t1r + a0);
        bf16x8 x2 = *(const bf16x8*)(t2r + a0);
        bf16x8 vv = *(const bf16x8*)(v + a0);
        bf16x8 out;
        float sc[8];
        drop_scale8(seed, salt, (uint32_t)((row * A + a0) >> 3), p, sc);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            float t = (bf2f(x1[e]) + bf2f(x2[e])) * sc[e];
            out[e] = f2bf(t);
            acc += t * bf2f(vv[e]);
        }
        *(bf16x8*)(tdr + a0) = out;
    }
    acc = wave_sum(acc);
    if (lane == 0) logits[row] = acc;
}

std::vector<at::Tensor> attn_scores_fused(at::Tensor t1, at::Tensor t2,
                                          at::Tensor v, at::Tensor seed,
                                          double p, int64_t salt,
                                          int64_t L) {
    CHECK_GPU(t1); CHECK_CONTIG(t1); CHECK_BF16(t1);
    CHECK_GPU(t2); CHECK_CONTIG(t2); CHECK_BF16(t2);
    CHECK_GPU(v); CHECK_CONTIG(v); CHECK_BF16(v);
    int A = t1.size(1);
    int rows = t1.size(0);
    int B = rows / (int)L;
    TORCH_CHECK(A % 8 == 0 && rows % L == 0);
    auto tdrop = at::empty_like(t1);
    auto logits = at::empty({B, (int)L},
                            t1.options().dtype(at::kFloat));
    hipStream_t s = at::cuda::getCurrentCUDAStream();
    hipLaunchKernelGGL(attn_scores_fused_kernel, dim3(cdiv(rows, 4)),
                       dim3(256), 0, s,
                       (const bf16*)t1.data_ptr(),
                       (const bf16*)t2.data_ptr(),
                       (const bf16*)v.data_ptr(),
                       (const int64_t*)seed.data_ptr(),
                       (bf16*)tdrop.data_ptr(), (float*)logits.data_ptr(),
                       B, (int)L, A, (float)p, (int)salt);
    HIP_OK(hipGetLastError());
    return {tdrop, logits};
}

// ---- attention pool backward ----
// phase 1, grid (B, 4): s_l = Σ_d dpooled·ctx[l,d] for an l-chunk (wave
// per row, coalesced), plus dctx = α ⊗ dpooled for the same rows.
// phase 2, grid (B): dlogits = α (dα_ext + s − Σ_l α·(dα_ext + s)).

//
// A wave takes its rows (l0 + wid, step 4) in batches of 8 with the alpha
// and ctx loads of the whole batch issued before the first use (one row
// at a time was two dependent round trips per row).  A row past the chunk
// end loads the chunk's last row, is computed and not stored: a branch
// around the whole row would let the compiler move the row's loads down
// into it, one wait per row again.  DCTX: dctx is wanted.

template <bool DCTX>
__global__ __launch_bounds__(256)
void attn_pool_bwd_p1_kernel(
        const bf16* __restrict__ ctx, const float* __restrict__ alpha,
        const bf16* __restrict__ dpooled,
        float* __restrict__ sbuf, bf16* __restrict__ dctx,
        int L, int D) {
    constexpr int R = 8;
    int b = blockIdx.x;
    int nchunk = gridDim.y;
    int lchunk = (L + nchunk - 1) / nchunk;
    int l0 = blockIdx.y * lchunk;
    int l1 = min(L, l0 + lchunk);
    int wid = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const bf16* cb = ctx + (int64_t)b * L * D;
    const bf16* dp = dpooled + (int64_t)b * D;

    for (int lb = l0 + wid; lb < l1; lb += 4 * R) {
        float a[R], acc[R];
        const bf16* cr[R];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            int l = min(lb + 4 * r, l1 - 1);
            a[r] = alpha[(int64_t)b * L + l];
            cr[r] = cb + (int64_t)l * D;
            acc[r] = 0.f;
        }
        for (int d0 = lane * 8; d0 + 8 <= D; d0 += 64 * 8) {
            bf16x8 cv[R];
#pragma unroll
            for (int r = 0; r < R; ++r)
                cv[r] = *(const bf16x8*)(cr[r] + d0);
            bf16x8 dv = *(const bf16x8*)(dp + d0);
#pragma unroll
            for (int r = 0; r < R; ++r) {
                bf16x8 out;
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    float dpe = bf2f(dv[e]);
                    acc[r] += bf2f(cv[r][e]) * dpe;
                    if constexpr (DCTX) out[e] = f2bf(a[r] * dpe);
                }
                if constexpr (DCTX) {
                    if (lb + 4 * r < l1)
                        *(bf16x8*)(dctx + (cr[r] - ctx) + d0) = out;
                }
            }
        }
#pragma unroll
        for (int r = 0; r < R; ++r) {
            float s = wave_sum(acc[r]);
            if (lane == 0 && lb + 4 * r < l1)
                sbuf[(int64_t)b * L + lb + 4 * r] = s;
        }
    }
}

__global__ void attn_pool_bwd_p2_kernel(
        const float* __restrict__ alpha, const float* __restrict__ dalpha,
        const float* __restrict__ sbuf, float* __restrict__ dlogits,
        int L) {
    __shared__ float red[4];
    int b = blockIdx.x;
    int tid = threadIdx.x;
    // the dalpha load goes out with the other two: its address is valid
    // with or without a dalpha (the value is dropped without one)
    const float* dap = dalpha != nullptr ? dalpha : sbuf;
    float part = 0.f;
    for (int l = tid; l < L; l += blockDim.x) {
        float da = sbuf[(int64_t)b * L + l];
        float dx = dap[(int64_t)b * L + l];
        float al = alpha[(int64_t)b * L + l];
        if (dalpha != nullptr) da += dx;
        part += al * da;
    }
    part = wave_sum(part);
    if ((tid & 63) == 0) red[tid >> 6] = part;
    __syncthreads();
    float dot = red[0] + red[1] + red[2] + red[3];
    for (int l = tid; l < L; l += blockDim.x) {
        float da = sbuf[(int64_t)b * L + l];
        float dx = dap[(int64_t)b * L + l];
        float al = alpha[(int64_t)b * L + l];
        if (dalpha != nullptr) da += dx;
        dlogits[(int64_t)b * L + l] = al * (da - dot);
    }
}

std::vector<at::Tensor> attn_pool_bwd(at::Tensor ctx, at::Tensor alpha,
                                      at::Tensor dalpha, at::Tensor dpooled,
                                      bool need_dctx) {
    CHECK_GPU(ctx); CHECK_CONTIG(ctx); CHECK_BF16(ctx);
    CHECK_GPU(alpha); CHECK_CONTIG(alpha); CHECK_F32(alpha);
    int B = ctx.size(0), L = ctx.size(1), D = ctx.size(2);
    TORCH_CHECK(L <= MAX_L && D % 8 == 0);
    auto dlogits = at::empty({B, L}, alpha.options());
    auto sbuf = at::empty({B, L}, alpha.options());
    at::Tensor dctx;
    bf16* dctx_ptr = nullptr;
    if (need_dctx) {
        dctx = at::empty_like(ctx);
        dctx_ptr = (bf16*)dctx.data_ptr();
    } else {
        dctx = at::empty({0}, ctx.options());
    }
    const float* dalpha_ptr = nullptr;
    if (dalpha.defined() && dalpha.numel() > 0)
        dalpha_ptr = (const float*)dalpha.data_ptr();
    hipStream_t s = at::cuda::getCurrentCUDAStream();
    // NOTE: a one-block-per-image fused p1+p2 variant measured SLOWER at
    // batch 32 — it cuts the p1 grid from B*4 to B blocks on a
    // latency-bound chain; the two-launch form stays (r02 A/B evidence).
    hipLaunchKernelGGL((need_dctx ? attn_pool_bwd_p1_kernel<true>
                                  : attn_pool_bwd_p1_kernel<false>),
                       dim3(B, 8), dim3(256), 0, s,
                       (const bf16*)ctx.data_ptr(),
                       (const float*)alpha.data_ptr(),
                       (const bf16*)dpooled.data_ptr(),
                       (float*)sbuf.data_ptr(), dctx_ptr, L, D);
    hipLaunchKernelGGL(attn_pool_bwd_p2_kernel, dim3(B), dim3(256), 0, s,
                       (const float*)alpha.data_ptr(), dalpha_ptr,
                       (const float*)sbuf.data_ptr(),
                       (float*)dlogits.data_ptr(), L);
    HIP_OK(hipGetLastError());
    return {dlogits, dctx};
}

// ---- attention scores backward ----
// dt1 = dlogit ⊗ v ⊙ mask/(1-p) (mask regenerated); dt2 = Σ_l dt1;
// dv = Σ_rows tdrop·dlogit.  Blocks cover l-chunks within one image.

template <int NCH>
__global__ void attn_scores_bwd_kernel(
        const bf16* __restrict__ tdrop, const bf16* __restrict__ v,
        const float* __restrict__ dlogits,
        const int64_t* __restrict__ seed_p,
        bf16* __restrict__ dt1, float* __restrict__ dt2,
        float* __restrict__ dvf,
        const bf16* __restrict__ t1y,  // when set: dt1 <- dt * (1-y^2)
        int B, int L, int A, int lchunk, float p, int salt) {
    // wave-per-row bf16x8 streaming; per-wave column partials are combined
    // through LDS and flushed with ONE atomic per thread-column — a lane
    // issuing 8 consecutive atomics serializes ~40x (measured 420us vs
    // 10us for this shape).
    __shared__ float sdv[4][NCH * 512];
    __shared__ float sd2[4][NCH * 512];
    const uint32_t seed = (uint32_t)(*seed_p);
    int nchunk = (L + lchunk - 1) / lchunk;
    int b = blockIdx.x / nchunk;
    int l0 = (blockIdx.x % nchunk) * lchunk;
    int l1 = min(L, l0 + lchunk);
    int wid = threadIdx.x >> 6, lane = threadIdx.x & 63;

    float dv_acc[NCH][8] = {};
    float dt2_acc[NCH][8] = {};

    for (int l = l0 + wid; l < l1; l += 4) {
        int64_t row = (int64_t)b * L + l;
        float dl = dlogits[row];
#pragma unroll
        for (int ch = 0; ch < NCH; ++ch) {
            int a0 = ch * 512 + lane * 8;
            bf16x8 td = *(const bf16x8*)(tdrop + row * A + a0);
            bf16x8 vv = *(const bf16x8*)(v + a0);
            bf16x8 o;
            float sc[8];
            drop_scale8(seed, salt, (uint32_t)((row * A + a0) >> 3), p, sc);
            bf16x8 yv = {};
            if (t1y != nullptr)
                yv = *(const bf16x8*)(t1y + row * A + a0);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                dv_acc[ch][e] += bf2f(td[e]) * dl;
                float dt = dl * bf2f(vv[e]) * sc[e];
                dt2_acc[ch][e] += dt;
                if (t1y != nullptr) {
                    // fused tanh backward: dt1 is dpre of att fc_1a
                    float y = bf2f(yv[e]);
                    dt *= (1.f - y * y);
                }
                o[e] = f2bf(dt);
            }
            *(bf16x8*)(dt1 + row * A + a0) = o;
        }
    }
#pragma unroll
    for (int ch = 0; ch < NCH; ++ch) {
        int a0 = ch * 512 + lane * 8;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            sdv[wid][a0 + e] = dv_acc[ch][e];
            sd2[wid][a0 + e] = dt2_acc[ch][e];
        }
    }
    __syncthreads();
    for (int a = threadIdx.x; a < A; a += (int)blockDim.x) {
        float dv_s = sdv[0][a] + sdv[1][a] + sdv[2][a] + sdv[3][a];
        float d2_s = sd2[0][a] + sd2[1][a] + sd2[2][a] + sd2[3][a];
        atomicAdd(dvf + a, dv_s);
        atomicAdd(dt2 + (int64_t)b * A + a, d2_s);
    }
}

// One host path for every scores-backward entry point.  dt2_out, when
// given, is a caller-ZEROED [B, A] fp32 slice the atomics accumulate into
// (saves the per-call fill launch); otherwise dt2 is allocated and zeroed
// here.
static std::vector<at::Tensor> attn_scores_bwd_impl(
        at::Tensor tdrop, at::Tensor v, at::Tensor dlogits,
        at::Tensor seed, double p, int64_t salt, int64_t L,
        at::Tensor dv_acc, at::Tensor t1y, at::Tensor dt1_out,
        at::Tensor dt2_out) {
    CHECK_GPU(tdrop); CHECK_CONTIG(tdrop); CHECK_BF16(tdrop);
    int rows = tdrop.size(0), A = tdrop.size(1);
    TORCH_CHECK(A % 512 == 0 && A <= 2048,
                "attn_scores_bwd requires A % 512 == 0, A <= 2048");
    int B = rows / (int)L;
    at::Tensor dt1;
    if (dt1_out.defined() && dt1_out.numel() > 0) {
        TORCH_CHECK(dt1_out.numel() == tdrop.numel());
        dt1 = dt1_out;
    } else {
        dt1 = at::empty_like(tdrop);
    }
    const bf16* t1y_ptr = nullptr;
    if (t1y.defined() && t1y.numel() > 0) {
        TORCH_CHECK(t1y.numel() == tdrop.numel());
        t1y_ptr = (const bf16*)t1y.data_ptr();
    }
    at::Tensor dt2;
    if (dt2_out.defined() && dt2_out.numel() > 0) {
        CHECK_GPU(dt2_out); CHECK_CONTIG(dt2_out); CHECK_F32(dt2_out);
        TORCH_CHECK(dt2_out.numel() == (int64_t)B * A);
        dt2 = dt2_out;
    } else {
        dt2 = at::zeros({B, A}, tdrop.options().dtype(at::kFloat));
    }
    at::Tensor dvf;
    if (dv_acc.defined() && dv_acc.numel() > 0)
        dvf = dv_acc;   // caller-owned accumulator (atomicAdd accumulates)
    else
        dvf = at::zeros({A}, tdrop.options().dtype(at::kFloat));
    int lchunk = ((int)L + 7) / 8;     // 8 chunks/image
    // (4 -> 8 chunks: 256 blocks at batch 32 — the kernel is
    // latency-bound at 12us, more blocks shorten the chain)
    int nchunk = ((int)L + lchunk - 1) / lchunk;
    hipStream_t s = at::cuda::getCurrentCUDAStream();
#define LAUNCH_SB(NCH) \
    hipLaunchKernelGGL((attn_scores_bwd_kernel<NCH>), dim3(B * nchunk), \
                       dim3(256), 0, s, \
                       (const bf16*)tdrop.data_ptr(), \
                       (const bf16*)v.data_ptr(), \
                       (const float*)dlogits.data_ptr(), \
                       (const int64_t*)seed.data_ptr(), \
                       (bf16*)dt1.data_ptr(), (float*)dt2.data_ptr(), \
                       (float*)dvf.data_ptr(), t1y_ptr, \
                       B, (int)L, A, lchunk, (float)p, (int)salt)
    switch (A / 512) {
        case 1: LAUNCH_SB(1); break;
        case 2: LAUNCH_SB(2); break;
        case 3: LAUNCH_SB(3); break;
        default: LAUNCH_SB(4); break;
    }
#undef LAUNCH_SB
    HIP_OK(hipGetLastError());
    return {dt1, dt2, dvf};
}

std::vector<at::Tensor> attn_scores_bwd_tanh(
        at::Tensor tdrop, at::Tensor v, at::Tensor dlogits,
        at::Tensor seed, double p, int64_t salt, int64_t L,
        at::Tensor dv_acc, at::Tensor t1y, at::Tensor dt1_out) {
    return attn_scores_bwd_impl(tdrop, v, dlogits, seed, p, salt, L,
                                dv_acc, t1y, dt1_out, at::Tensor());
}

std::vector<at::Tensor> attn_scores_bwd_acc(at::Tensor tdrop, at::Tensor v,
                                            at::Tensor dlogits,
                                            at::Tensor seed, double p,
                                            int64_t salt, int64_t L,
                                            at::Tensor dv_acc) {
    return attn_scores_bwd_tanh(tdrop, v, dlogits, seed, p, salt, L,
                                dv_acc, at::Tensor(), at::Tensor());
}

// the decoder reverse loop's form: dt2 accumulates into a caller-zeroed
// slice of one [T, B, A] buffer
std::vector<at::Tensor> attn_scores_bwd_step(
        at::Tensor tdrop, at::Tensor v, at::Tensor dlogits,
        at::Tensor seed, double p, int64_t salt, int64_t L,
        at::Tensor dv_acc, at::Tensor t1y, at::Tensor dt1_out,
        at::Tensor dt2_out) {
    return attn_scores_bwd_impl(tdrop, v, dlogits, seed, p, salt, L,
                                dv_acc, t1y, dt1_out, dt2_out);
}

std::vector<at::Tensor> attn_scores_bwd(at::Tensor tdrop, at::Tensor v,
                                        at::Tensor dlogits, at::Tensor seed,
                                        double p, int64_t salt, int64_t L) {
    return attn_scores_bwd_acc(tdrop, v, dlogits, seed, p, salt, L,
                               at::Tensor());
}

__global__ void attn_softmax_kernel(const float* __restrict__ logits,
                                    float* __restrict__ alpha, int L) {
    __shared__ float sa[MAX_L];
    __shared__ float red[8];
    int b = blockIdx.x;
    int tid = threadIdx.x;
    float lmax = -1e30f;
    for (int l = tid; l < L; l += blockDim.x) {
        float x = logits[(int64_t)b * L + l];
        sa[l] = x;
        lmax = fmaxf(lmax, x);
    }
    lmax = wave_max(lmax);
    if ((tid & 63) == 0) red[tid >> 6] = lmax;
    __syncthreads();
    float m = -1e30f;
    for (int w = 0; w < (int)(blockDim.x >> 6); ++w) m = fmaxf(m, red[w]);
    __syncthreads();
    float lsum = 0.f;
    for (int l = tid; l < L; l += blockDim.x) {
        float e = __expf(sa[l] - m);
        sa[l] = e;
        lsum += e;
    }
    lsum = wave_sum(lsum);
    if ((tid & 63) == 0) red[tid >> 6] = lsum;
    __syncthreads();
    float z = 0.f;
    for (int w = 0; w < (int)(blockDim.x >> 6); ++w) z += red[w];
    float inv = 1.0f / z;
    for (int l = tid; l < L; l += blockDim.x)
        alpha[(int64_t)b * L + l] = sa[l] * inv;
}

// pooled[b, d] = sum_l alpha[b,l] * ctx[b,l,d]; grid (B, ceil(D/128));
// 256 threads sweep two l-rows x 128 columns per iteration (coalesced).
__global__ void attn_pool_sum_kernel(const bf16* __restrict__ ctx,
                                     const float* __restrict__ alpha,
                                     bf16* __restrict__ pooled,
                                     int L, int D) {
    // grid (B, ceil(D/128)); 256 threads = 16 l-streams x (16 threads x
    // bf16x8) covering 128 columns; partials combined through LDS.
    __shared__ float sa[MAX_L];
    __shared__ float part[16][128 + 4];
    int b = blockIdx.x;
    int d0 = blockIdx.y * 128;
    int tid = threadIdx.x;
    for (int l = tid; l < L; l += blockDim.x)
        sa[l] = alpha[(int64_t)b * L + l];
    __syncthreads();
    int dg = tid & 15;               // column-chunk within the 128
    int lg = tid >> 4;               // l-stream 0..15
    int d = d0 + dg * 8;
    float acc[8] = {};
    if (d < D) {
        const bf16* cb = ctx + (int64_t)b * L * D;
        for (int l = lg; l < L; l += 16) {
            bf16x8 cv = *(const bf16x8*)(cb + (int64_t)l * D + d);
            float a = sa[l];
#pragma unroll
            for (int e = 0; e < 8; ++e) acc[e] += a * bf2f(cv[e]);
        }
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) part[lg][dg * 8 + e] = acc[e];
    __syncthreads();
    // threads 0..127 finalize one column each
    if (tid < 128 && d0 + tid < D) {
        float s = 0.f;
#pragma unroll
        for (int g = 0; g < 16; ++g) s += part[g][tid];
        pooled[(int64_t)b * D + d0 + tid] = f2bf(s);
    }
}

// fused softmax + weighted pool: each (b, d-chunk) block recomputes the
// L-wide softmax in LDS (cheap: L <= 1024 floats) and pools its 128
// columns — one launch instead of softmax + pool, no alpha round-trip
// on the forward critical path (alpha is still written once, by the
// chunk-0 block, for backward/attention-loss use).
__global__ void attn_pool_fused_kernel(const bf16* __restrict__ ctx,
                                       const float* __restrict__ logits,
                                       float* __restrict__ alpha,
                                       bf16* __restrict__ pooled,
                                       int L, int D,
                                       bf16* __restrict__ xh,
                                       const int64_t* __restrict__ seed_p,
                                       int xh_stride, int I, float p,
                                       int salt) {
    // xh != null: the bf16 pooled columns also go, input-dropped (index
    // b*I + d, as lstm_in_fuse does), into the step's LSTM input row
    __shared__ float sa[MAX_L];
    __shared__ float red[8];
    __shared__ float part[16][128 + 4];
    int b = blockIdx.x;
    int d0 = blockIdx.y * 128;
    int tid = threadIdx.x;

    // softmax over L into sa (same math as attn_softmax_kernel)
    float lmax = -1e30f;
    for (int l = tid; l < L; l += blockDim.x) {
        float x = logits[(int64_t)b * L + l];
        sa[l] = x;
        lmax = fmaxf(lmax, x);
    }
    lmax = wave_max(lmax);
    if ((tid & 63) == 0) red[tid >> 6] = lmax;
    __syncthreads();
    float m = -1e30f;
    for (int w = 0; w < (int)(blockDim.x >> 6); ++w)
        m = fmaxf(m, red[w]);
    __syncthreads();
    float lsum = 0.f;
    for (int l = tid; l < L; l += blockDim.x) {
        float e = __expf(sa[l] - m);
        sa[l] = e;
        lsum += e;
    }
    lsum = wave_sum(lsum);
    if ((tid & 63) == 0) red[tid >> 6] = lsum;
    __syncthreads();
    float z = 0.f;
    for (int w = 0; w < (int)(blockDim.x >> 6); ++w) z += red[w];
    float inv = 1.0f / z;
    __syncthreads();
    for (int l = tid; l < L; l += blockDim.x) {
        sa[l] *= inv;
        if (blockIdx.y == 0)
            alpha[(int64_t)b * L + l] = sa[l];
    }
    __syncthreads();

    // pool this block's 128 columns
    int dg = tid & 15;
    int lg = tid >> 4;
    int d = d0 + dg * 8;
    float acc[8] = {};
    if (d < D) {
        const bf16* cb = ctx + (int64_t)b * L * D;
        for (int l = lg; l < L; l += 16) {
            bf16x8 cv = *(const bf16x8*)(cb + (int64_t)l * D + d);
            float a = sa[l];
#pragma unroll
            for (int e = 0; e < 8; ++e) acc[e] += a * bf2f(cv[e]);
        }
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) part[lg][dg * 8 + e] = acc[e];
    __syncthreads();
    if (tid < 128 && d0 + tid < D) {
        float ssum = 0.f;
#pragma unroll
        for (int g = 0; g < 16; ++g) ssum += part[g][tid];
        bf16 pv = f2bf(ssum);
        pooled[(int64_t)b * D + d0 + tid] = pv;
        if (xh != nullptr) {
            int d = d0 + tid;
            xh[(int64_t)b * xh_stride + d] =
                f2bf(bf2f(pv) * drop_scale((uint32_t)(*seed_p), salt,
                                           (uint32_t)(b * I + d), p));
        }
    }
}

static std::vector<at::Tensor> attn_pool_fwd_impl(
        at::Tensor ctx, at::Tensor logits, bf16* xh_ptr,
        const int64_t* seed_ptr, int xh_stride, int I, double p,
        int64_t salt) {
    CHECK_GPU(ctx); CHECK_CONTIG(ctx); CHECK_BF16(ctx);
    CHECK_GPU(logits); CHECK_CONTIG(logits); CHECK_F32(logits);
    int B = ctx.size(0), L = ctx.size(1), D = ctx.size(2);
    TORCH_CHECK(L <= MAX_L, "attention locations exceed LDS stage");
    TORCH_CHECK(D % 8 == 0, "attn_pool_fwd requires D % 8 == 0");
    TORCH_CHECK(logits.numel() == (int64_t)B * L);
    auto alpha = at::empty({B, L}, ctx.options().dtype(at::kFloat));
    auto pooled = at::empty({B, D}, ctx.options());
    hipStream_t s = at::cuda::getCurrentCUDAStream();
    hipLaunchKernelGGL(attn_pool_fused_kernel, dim3(B, cdiv(D, 128)),
                       dim3(256), 0, s,
                       (const bf16*)ctx.data_ptr(),
                       (const float*)logits.data_ptr(),
                       (float*)alpha.data_ptr(),
                       (bf16*)pooled.data_ptr(), L, D,
                       xh_ptr, seed_ptr, xh_stride, I, (float)p,
                       (int)salt);
    HIP_OK(hipGetLastError());
    return {alpha, pooled};
}

std::vector<at::Tensor> attn_pool_fwd(at::Tensor ctx, at::Tensor logits) {
    return attn_pool_fwd_impl(ctx, logits, nullptr, nullptr, 0, 0, 0.0, 0);
}

// attn_pool_fwd that also writes dropout(pooled, p, salt) into columns
// [0, D) of the step's LSTM input rows xh [B, I + H] (I = D + E)
std::vector<at::Tensor> attn_pool_fwd_xh(at::Tensor ctx, at::Tensor logits,
                                         at::Tensor seed, double p,
                                         int64_t salt, at::Tensor xh,
                                         int64_t I) {
    CHECK_GPU(xh); CHECK_CONTIG(xh); CHECK_BF16(xh);
    CHECK_GPU(seed);
    TORCH_CHECK(xh.dim() == 2 && xh.size(0) == ctx.size(0)
                && I >= ctx.size(2) && xh.size(1) >= I,
                "xh must be [B, I + H] with I >= D");
    return attn_pool_fwd_impl(ctx, logits, (bf16*)xh.data_ptr(),
                              (const int64_t*)seed.data_ptr(),
                              (int)xh.size(1), (int)I, p, salt);
}

// ======================================================================
// Embedding gather / scatter-add grad (model.py:273; table [V,E] bf16).
// ======================================================================

__global__ void embedding_fwd_kernel(const int64_t* __restrict__ ids,
                                     const bf16* __restrict__ table,
                                     bf16* __restrict__ out,
                                     int B, int E) {
    int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= B * E) return;
    int b = idx / E, e = idx % E;
    out[idx] = table[ids[b] * E + e];
}

__global__ void embedding_bwd_kernel(const int64_t* __restrict__ ids,
                                     const bf16* __restrict__ dy,
                                     float* __restrict__ dtable,
                                     int B, int E) {
    int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= B * E) return;
    int b = idx / E, e = idx % E;
    atomicAdd(dtable + ids[b] * E + e, bf2f(dy[idx]));
}

at::Tensor embedding_fwd(at::Tensor ids, at::Tensor table) {
    CHECK_GPU(ids); CHECK_CONTIG(ids);
    CHECK_GPU(table); CHECK_CONTIG(table); CHECK_BF16(table);
    TORCH_CHECK(ids.scalar_type() == at::kLong, "ids must be int64");
    int B = ids.numel(), E = table.size(1);
    auto out = at::empty({B, E}, table.options());
    hipStream_t s = at::cuda::getCurrentCUDAStream();
    hipLaunchKernelGGL(embedding_fwd_kernel, dim3(cdiv(B * E, 256)),
                       dim3(256), 0, s,
                       (const int64_t*)ids.data_ptr(),
                       (const bf16*)table.data_ptr(),
                       (bf16*)out.data_ptr(), B, E);
    HIP_OK(hipGetLastError());
    return out;
}

at::Tensor embedding_bwd(at::Tensor ids, at::Tensor dy, int64_t rows) {
    CHECK_GPU(ids); CHECK_GPU(dy); CHECK_CONTIG(dy); CHECK_BF16(dy);
    TORCH_CHECK(ids.scalar_type() == at::kLong, "ids must be int64");
    int B = ids.numel(), E = dy.size(1);
    auto dtable = at::zeros({rows, E}, dy.options().dtype(at::kFloat));
    hipStream_t s = at::cuda::getCurrentCUDAStream();
    hipLaunchKernelGGL(embedding_bwd_kernel, dim3(cdiv(B * E, 256)),
                       dim3(256), 0, s,
                       (const int64_t*)ids.data_ptr(),
                       (const bf16*)dy.data_ptr(),
                       (float*)dtable.data_ptr(), B, E);
    HIP_OK(hipGetLastError());
    return dtable;
}

// ======================================================================
// Fused masked softmax cross-entropy over the vocabulary (model.py:294-297)
// ======================================================================

__global__ void ce_fwd_kernel(const bf16* __restrict__ logits, // [B,V]
                              const int64_t* __restrict__ labels,
                              const float* __restrict__ mask,
                              float* __restrict__ losses,
                              float* __restrict__ lse,
                              int V) {
    __shared__ float red[8];
    int b = blockIdx.x;
    int tid = threadIdx.x;
    const bf16* row = logits + (int64_t)b * V;

    float lmax = -1e30f;
    for (int v = tid; v < V; v += blockDim.x)
        lmax = fmaxf(lmax, bf2f(row[v]));
    lmax = wave_max(lmax);
    if ((tid & 63) == 0) red[tid >> 6] = lmax;
    __syncthreads();
    float m = -1e30f;
    for (int w = 0; w < (int)(blockDim.x >> 6); ++w) m = fmaxf(m, red[w]);
    __syncthreads();

    float lsum = 0.f;
    for (int v = tid; v < V; v += blockDim.x)
        lsum += __expf(bf2f(row[v]) - m);
    lsum = wave_sum(lsum);
    if ((tid & 63) == 0) red[tid >> 6] = lsum;
    __syncthreads();
    if (tid == 0) {
        float z = 0.f;
        for (int w = 0; w < (int)(blockDim.x >> 6); ++w) z += red[w];
        float l = m + __logf(z);
        lse[b] = l;
        losses[b] = (l - bf2f(row[labels[b]])) * mask[b];
    }
}

__global__ void ce_bwd_kernel(const bf16* __restrict__ logits,
                              const int64_t* __restrict__ labels,
                              const float* __restrict__ mask,
                              const float* __restrict__ lse,
                              const float* __restrict__ dloss,
                              bf16* __restrict__ dlogits,
                              int B, int V) {
    int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (int64_t)B * V) return;
    int b = idx / V, v = idx % V;
    float p = __expf(bf2f(logits[idx]) - lse[b]);
    float g = (p - (labels[b] == v ? 1.f : 0.f)) * mask[b] * dloss[b];
    dlogits[idx] = f2bf(g);
}

std::vector<at::Tensor> ce_fwd(at::Tensor logits, at::Tensor labels,
                               at::Tensor mask) {
    CHECK_GPU(logits); CHECK_CONTIG(logits); CHECK_BF16(logits);
    CHECK_GPU(labels); CHECK_GPU(mask); CHECK_F32(mask);
    TORCH_CHECK(labels.scalar_type() == at::kLong, "labels must be int64");
    int B = logits.size(0), V = logits.size(1);
    auto losses = at::empty({B}, logits.options().dtype(at::kFloat));
    auto lse = at::empty({B}, logits.options().dtype(at::kFloat));
    hipStream_t s = at::cuda::getCurrentCUDAStream();
    hipLaunchKernelGGL(ce_fwd_kernel, dim3(B), dim3(256), 0, s,
                       (const bf16*)logits.data_ptr(),
                       (const int64_t*)labels.data_ptr(),
                       (const float*)mask.data_ptr(),
                       (float*)losses.data_ptr(), (float*)lse.data_ptr(), V);
    HIP_OK(hipGetLastError());
    return {losses, lse};
}

at::Tensor ce_bwd(at::Tensor logits, at::Tensor labels, at::Tensor mask,
                  at::Tensor lse, at::Tensor dloss) {
    CHECK_GPU(logits); CHECK_CONTIG(logits); CHECK_BF16(logits);
    TORCH_CHECK(labels.scalar_type() == at::kLong, "labels must be int64");
    int B = logits.size(0), V = logits.size(1);
    auto dlogits = at::empty_like(logits);
    hipStream_t s = at::cuda::getCurrentCUDAStream();
    hipLaunchKernelGGL(ce_bwd_kernel,
                       dim3(cdiv((int64_t)B * V, 256)), dim3(256), 0, s,
                       (const bf16*)logits.data_ptr(),
                       (const int64_t*)labels.data_ptr(),
                       (const float*)mask.data_ptr(),
                       (const float*)lse.data_ptr(),
                       (const float*)dloss.data_ptr(),
                       (bf16*)dlogits.data_ptr(), B, V);
    HIP_OK(hipGetLastError());
    return dlogits;
}

// ======================================================================
// Fused global-norm-clipped Adam (model.py:461-513 + optimize_loss clip).
// Two phases: grad_sq_norm accumulates Σ‖g‖² across all tensors into one
// device scalar; adam_step applies clip scale + bias-corrected Adam.
// ======================================================================

__global__ void sq_norm_kernel(const float* __restrict__ g, int64_t n,
                               float* __restrict__ out) {
    int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    float acc = 0.f;
    for (int64_t i = idx; i < n; i += (int64_t)gridDim.x * blockDim.x)
        acc += g[i] * g[i];
    acc = wave_sum(acc);
    __shared__ float red[8];
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        float t = 0.f;
        for (int w = 0; w < (int)(blockDim.x >> 6); ++w) t += red[w];
        atomicAdd(out, t);
    }
}

// step (and with it bias correction + staircase LR decay) comes from a
// DEVICE scalar so the whole optimizer is hipGraph-capturable: replays see
// the advancing counter, no host scalar is baked in at capture time.
__global__ void adam_kernel(float* __restrict__ p, const float* __restrict__ g,
                            float* __restrict__ m, float* __restrict__ v,
                            const float* __restrict__ gsq,
                            const float* __restrict__ step_dev,
                            int64_t n, float lr0, float decay_factor,
                            float steps_per_decay, float b1, float b2,
                            float eps, float clip) {
    float step = *step_dev;
    float bc1 = 1.f - powf(b1, step);
    float bc2 = 1.f - powf(b2, step);
    float lr = lr0;
    if (decay_factor < 1.f)
        lr = lr0 * powf(decay_factor, floorf(step / steps_per_decay));
    float scale = 1.f;
    if (clip > 0.f) {
        float norm = sqrtf(*gsq);
        if (norm > clip) scale = clip / norm;
    }
    int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (int64_t i = idx; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        float gi = g[i] * scale;
        float mi = b1 * m[i] + (1.f - b1) * gi;
        float vi = b2 * v[i] + (1.f - b2) * gi * gi;
        m[i] = mi;
        v[i] = vi;
        float mhat = mi / bc1;
        float vhat = vi / bc2;
        p[i] -= lr * mhat / (sqrtf(vhat) + eps);
    }
}

at::Tensor grad_sq_norm(std::vector<at::Tensor> grads) {
    TORCH_CHECK(!grads.empty());
    auto out = at::zeros({1}, grads[0].options().dtype(at::kFloat));
    hipStream_t s = at::cuda::getCurrentCUDAStream();
    for (auto& g : grads) {
        CHECK_GPU(g); CHECK_CONTIG(g); CHECK_F32(g);
        int64_t n = g.numel();
        int blocks = (int)std::min<int64_t>(cdiv(n, 256), 1024);
        hipLaunchKernelGGL(sq_norm_kernel, dim3(blocks), dim3(256), 0, s,
                           (const float*)g.data_ptr(), n,
                           (float*)out.data_ptr());
    }
    HIP_OK(hipGetLastError());
    return out;
}

void adam_step(std::vector<at::Tensor> params, std::vector<at::Tensor> grads,
               std::vector<at::Tensor> ms, std::vector<at::Tensor> vs,
               at::Tensor step_dev, double lr0, double decay_factor,
               double steps_per_decay, double b1, double b2, double eps,
               double clip, at::Tensor gsq) {
    CHECK_GPU(step_dev); CHECK_F32(step_dev);
    hipStream_t s = at::cuda::getCurrentCUDAStream();
    for (size_t i = 0; i < params.size(); ++i) {
        auto& p = params[i];
        CHECK_GPU(p); CHECK_CONTIG(p); CHECK_F32(p);
        int64_t n = p.numel();
        int blocks = (int)std::min<int64_t>(cdiv(n, 256), 2048);
        hipLaunchKernelGGL(adam_kernel, dim3(blocks), dim3(256), 0, s,
                           (float*)p.data_ptr(),
                           (const float*)grads[i].data_ptr(),
                           (float*)ms[i].data_ptr(), (float*)vs[i].data_ptr(),
                           (const float*)gsq.data_ptr(),
                           (const float*)step_dev.data_ptr(), n,
                           (float)lr0, (float)decay_factor,
                           (float)steps_per_decay, (float)b1, (float)b2,
                           (float)eps, (float)clip);
    }
    HIP_OK(hipGetLastError());
}

// ======================================================================
// Multi-tensor Adam / grad-norm: ONE launch over the concatenation of all
// parameter tensors.  desc: [n,4] int64 device pointers (p,g,m,v); cum:
// [n+1] int64 cumulative numels.  Tensor lookup = binary search in LDS.
// ======================================================================

__global__ void sq_norm_mt_kernel(const int64_t* __restrict__ desc,
                                  const int64_t* __restrict__ cum,
                                  int n_tensors, int64_t total,
                                  float* __restrict__ out) {
    extern __shared__ int64_t scum[];
    for (int i = threadIdx.x; i <= n_tensors; i += blockDim.x)
        scum[i] = cum[i];
    __syncthreads();
    float acc = 0.f;
    int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = idx; i < total; i += stride) {
        int lo = 0, hi = n_tensors;
        while (hi - lo > 1) {
            int mid = (lo + hi) >> 1;
            if (i >= scum[mid]) lo = mid; else hi = mid;
        }
        const float* g = (const float*)desc[lo * 5 + 1];
        float gv = g[i - scum[lo]];
        acc += gv * gv;
    }
    acc = wave_sum(acc);
    __shared__ float red[4];
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0)
        atomicAdd(out, red[0] + red[1] + red[2] + red[3]);
}

at::Tensor sq_norm_mt(at::Tensor desc, at::Tensor cum, int64_t n_tensors,
                      int64_t total) {
    auto out = at::zeros({1}, at::TensorOptions()
                                  .dtype(at::kFloat)
                                  .device(desc.device()));
    hipStream_t s = at::cuda::getCurrentCUDAStream();
    int blocks = (int)std::min<int64_t>(cdiv(total, 256 * 8), 2048);
    size_t shm = (n_tensors + 1) * sizeof(int64_t);
    hipLaunchKernelGGL(sq_norm_mt_kernel, dim3(blocks), dim3(256), shm, s,
                       (const int64_t*)desc.data_ptr(),
                       (const int64_t*)cum.data_ptr(),
                       (int)n_tensors, total, (float*)out.data_ptr());
    HIP_OK(hipGetLastError());
    return out;
}

typedef __attribute__((ext_vector_type(4))) float floatx4v;

// VEC4 = all tensor boundaries 16B-aligned (host-checked): 4 elements
// per thread iteration with float4 traffic — the scalar form ran ~3x
// over the ~35 us p/g/m/v streaming floor
template <int VEC4>
__global__ void adam_mt_kernel(const int64_t* __restrict__ desc,
                               const int64_t* __restrict__ cum,
                               int n_tensors, int64_t total,
                               const float* __restrict__ gsq,
                               const float* __restrict__ step_dev,
                               float lr0, float decay_factor,
                               float steps_per_decay, float b1, float b2,
                               float eps, float clip, int zero_g) {
    extern __shared__ int64_t scum[];
    for (int i = threadIdx.x; i <= n_tensors; i += blockDim.x)
        scum[i] = cum[i];
    __syncthreads();
    float step = *step_dev;
    float bc1 = 1.f - powf(b1, step);
    float bc2 = 1.f - powf(b2, step);
    float lr = lr0;
    if (decay_factor < 1.f)
        lr = lr0 * powf(decay_factor, floorf(step / steps_per_decay));
    float scale = 1.f;
    if (clip > 0.f) {
        float norm = sqrtf(*gsq);
        if (norm > clip) scale = clip / norm;
    }
    constexpr int V = VEC4 ? 4 : 1;
    int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    int64_t niter = (total + V - 1) / V;
    for (int64_t it = idx; it < niter; it += stride) {
        int64_t i = it * V;
        int lo = 0, hi = n_tensors;
        while (hi - lo > 1) {
            int mid = (lo + hi) >> 1;
            if (i >= scum[mid]) lo = mid; else hi = mid;
        }
        int64_t off = i - scum[lo];
        float* p = (float*)desc[lo * 5 + 0];
        float* g = (float*)desc[lo * 5 + 1];
        float* m = (float*)desc[lo * 5 + 2];
        float* v = (float*)desc[lo * 5 + 3];
        bf16* sh = (bf16*)desc[lo * 5 + 4];
        if (VEC4) {
            // boundaries are %4 (host-checked): the 4-span never
            // crosses a tensor; tail guarded by niter
            floatx4v g4 = *(floatx4v*)(g + off);
            floatx4v m4 = *(floatx4v*)(m + off);
            floatx4v v4 = *(floatx4v*)(v + off);
            floatx4v p4 = *(floatx4v*)(p + off);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float gi = g4[e] * scale;
                float mi = b1 * m4[e] + (1.f - b1) * gi;
                float vi = b2 * v4[e] + (1.f - b2) * gi * gi;
                m4[e] = mi;
                v4[e] = vi;
                p4[e] -= lr * (mi / bc1) / (sqrtf(vi / bc2) + eps);
            }
            *(floatx4v*)(m + off) = m4;
            *(floatx4v*)(v + off) = v4;
            *(floatx4v*)(p + off) = p4;
            if (sh != nullptr) {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    sh[off + e] = f2bf(p4[e]);
            }
            if (zero_g)
                *(floatx4v*)(g + off) = floatx4v{0.f, 0.f, 0.f, 0.f};
        } else {
            float gi = g[off] * scale;
            float mi = b1 * m[off] + (1.f - b1) * gi;
            float vi = b2 * v[off] + (1.f - b2) * gi * gi;
            m[off] = mi;
            v[off] = vi;
            float pn = p[off]
                - lr * (mi / bc1) / (sqrtf(vi / bc2) + eps);
            p[off] = pn;
            // write-through bf16 shadow (see optim.py)
            if (sh != nullptr) sh[off] = f2bf(pn);
            // fold next step's grad zeroing into the update pass
            if (zero_g) g[off] = 0.f;
        }
    }
}

void adam_step_mt(at::Tensor desc, at::Tensor cum, int64_t n_tensors,
                  int64_t total, at::Tensor step_dev, double lr0,
                  double decay_factor, double steps_per_decay, double b1,
                  double b2, double eps, double clip, at::Tensor gsq,
                  bool zero_grads, bool vec4) {
    hipStream_t s = at::cuda::getCurrentCUDAStream();
    int blocks = (int)std::min<int64_t>(cdiv(total, 256 * 4), 4096);
    size_t shm = (n_tensors + 1) * sizeof(int64_t);
    // vec4 = caller guarantees every tensor boundary is 16B-aligned
    // (hoisted to the desc build: a device->host check here would sync
    // inside graph capture)
    if (vec4)
        hipLaunchKernelGGL((adam_mt_kernel<1>), dim3(blocks), dim3(256),
                           shm, s,
                           (const int64_t*)desc.data_ptr(),
                           (const int64_t*)cum.data_ptr(),
                           (int)n_tensors, total,
                           (const float*)gsq.data_ptr(),
                           (const float*)step_dev.data_ptr(),
                           (float)lr0, (float)decay_factor,
                           (float)steps_per_decay, (float)b1, (float)b2,
                           (float)eps, (float)clip, zero_grads ? 1 : 0);
    else
        hipLaunchKernelGGL((adam_mt_kernel<0>), dim3(blocks), dim3(256),
                           shm, s,
                           (const int64_t*)desc.data_ptr(),
                           (const int64_t*)cum.data_ptr(),
                           (int)n_tensors, total,
                           (const float*)gsq.data_ptr(),
                           (const float*)step_dev.data_ptr(),
                           (float)lr0, (float)decay_factor,
                           (float)steps_per_decay, (float)b1, (float)b2,
                           (float)eps, (float)clip, zero_grads ? 1 : 0);
    HIP_OK(hipGetLastError());
}
