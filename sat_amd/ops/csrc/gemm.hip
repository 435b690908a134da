// dense_fwd: Y[M,N] = act(X[M,K] @ W[N,K]^T + bias), bf16 in/out, fp32 acc.
//
// The hand-written MFMA GEMM family behind every fc layer of the decoder
// (reference op surface SURVEY.md §2.3: init/attend/decode MLPs, LSTM gate
// GEMM).  Three shapes of work, three kernels:
//
//   * tiled_gemm<2,2,4,4>  — 128x128 tile, the large-M path (attention
//     projection [B·196,512]x[512,512]);
//   * tiled_gemm<4,1,2,4>  — 128x64 tile for N <= 512: twice the blocks,
//     fills the 256-CU / 8-XCD chip at the flagship shapes;
//   * skinny split-K       — M <= 128 (decode/LSTM GEMMs at per-GPU
//     batch 32..128): one RF*16-row tile (RF = 2/4/8), 16-column wave
//     slabs, K split across blocks into per-split fp32 slabs that a
//     separate epilogue kernel sums and finishes (bias/act, dropout,
//     LSTM gate math, dx scatter).  The 128x128 kernel runs these
//     shapes at 8-40 blocks (latency-bound, measured 40-60us each); the
//     skinny kernel runs 128-316 blocks.
//
// CDNA4 structure per the gfx950 playbook: v_mfma_f32_16x16x32_bf16,
// fp32 AGPR accumulation, LDS staging with +8 bf16 row padding (bank
// spread for ds_read_b128 fragment reads), bf16x8 (16 B) global loads,
// guarded edges so any K%8==0 shape works.

#include "common.h"

at::Tensor dense_8p_fwd(at::Tensor x, at::Tensor w, at::Tensor bias,
                        int64_t act);                      // gemm8p.hip
at::Tensor hash_dropout(at::Tensor x, at::Tensor seed, double p,
                        int64_t salt);                     // kernels.hip

#define BK 64
#define LDS_STRIDE (BK + 8)   // row stride 144 B (16 B aligned)

#define ACT_NONE 0
#define ACT_TANH 1
#define ACT_RELU 2

__device__ __forceinline__ float apply_act(float v, int act) {
    if (act == ACT_TANH) return tanhf(v);
    if (act == ACT_RELU) return fmaxf(v, 0.f);
    return v;
}

// ---------------------------------------------------------------------
// tiled kernel: BM = WR*FM*16, BN = WC*FN*16; 4 waves (WR*WC == 4)
// ---------------------------------------------------------------------

template <int WR, int WC, int FM, int FN>
__global__ __launch_bounds__(256)
void tiled_gemm_kernel(const bf16* __restrict__ A,    // [M,K]
                       const bf16* __restrict__ W,    // [N,K]
                       const bf16* __restrict__ bias, // [N] or null
                       bf16* __restrict__ Y,          // [M,N]
                       int M, int N, int K, int act,
                       // split-K: when Yf != null, block z covers
                       // K-range [kq*kchunk, ...) and stores an fp32
                       // slab; skinny_epilogue_kernel combines
                       float* __restrict__ Yf, int kchunk) {
    constexpr int BM = WR * FM * 16;
    constexpr int BN = WC * FN * 16;
    __shared__ bf16 As[BM * LDS_STRIDE];
    __shared__ bf16 Bs[BN * LDS_STRIDE];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int wr = wave / WC;
    const int wc = wave % WC;

    const int bm = blockIdx.y * BM;
    const int bn = blockIdx.x * BN;

    floatx4 acc[FM][FN];
#pragma unroll
    for (int i = 0; i < FM; ++i)
#pragma unroll
        for (int j = 0; j < FN; ++j)
            acc[i][j] = floatx4{0.f, 0.f, 0.f, 0.f};

    const int lrow = lane & 15;
    const int kgrp = lane >> 4;

    constexpr int A_CHUNKS = BM * BK / 8 / 256;  // bf16x8 chunks per thread
    constexpr int B_CHUNKS = BN * BK / 8 / 256;

    int kbeg = 0, kend = K;
    if (Yf != nullptr) {
        kbeg = blockIdx.z * kchunk;
        kend = min(K, kbeg + kchunk);
    }
    for (int k0 = kbeg; k0 < kend; k0 += BK) {
#pragma unroll
        for (int i = 0; i < A_CHUNKS; ++i) {
            int q = tid + 256 * i;
            int row = q >> 3;
            int c8 = (q & 7) * 8;
            int gk = k0 + c8;
            bf16x8 v = {};
            int ga = bm + row;
            if (ga < M && gk + 8 <= K) {
                v = *(const bf16x8*)(A + (int64_t)ga * K + gk);
            } else if (ga < M) {
                for (int e = 0; e < 8; ++e)
                    if (gk + e < K) v[e] = A[(int64_t)ga * K + gk + e];
            }
            *(bf16x8*)(As + row * LDS_STRIDE + c8) = v;
        }
#pragma unroll
        for (int i = 0; i < B_CHUNKS; ++i) {
            int q = tid + 256 * i;
            int row = q >> 3;
            int c8 = (q & 7) * 8;
            int gk = k0 + c8;
            bf16x8 v = {};
            int gb = bn + row;
            if (gb < N && gk + 8 <= K) {
                v = *(const bf16x8*)(W + (int64_t)gb * K + gk);
            } else if (gb < N) {
                for (int e = 0; e < 8; ++e)
                    if (gk + e < K) v[e] = W[(int64_t)gb * K + gk + e];
            }
            *(bf16x8*)(Bs + row * LDS_STRIDE + c8) = v;
        }
        __syncthreads();

#pragma unroll
        for (int kk = 0; kk < BK / 32; ++kk) {
            bf16x8 a_frag[FM], b_frag[FN];
            const int kof = kk * 32 + kgrp * 8;
#pragma unroll
            for (int mi = 0; mi < FM; ++mi)
                a_frag[mi] = *(const bf16x8*)(
                    As + (wr * FM * 16 + mi * 16 + lrow) * LDS_STRIDE + kof);
#pragma unroll
            for (int ni = 0; ni < FN; ++ni)
                b_frag[ni] = *(const bf16x8*)(
                    Bs + (wc * FN * 16 + ni * 16 + lrow) * LDS_STRIDE + kof);
#pragma unroll
            for (int mi = 0; mi < FM; ++mi)
#pragma unroll
                for (int ni = 0; ni < FN; ++ni)
                    acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                        a_frag[mi], b_frag[ni], acc[mi][ni], 0, 0, 0);
        }
        __syncthreads();
    }

    // epilogue (C/D map: col = lane&15, row = (lane>>4)*4 + reg)
    float* slab = (Yf != nullptr)
        ? Yf + (int64_t)blockIdx.z * M * N : nullptr;
#pragma unroll
    for (int ni = 0; ni < FN; ++ni) {
        int col = bn + wc * FN * 16 + ni * 16 + (lane & 15);
        float bv = (bias != nullptr && col < N) ? bf2f(bias[col]) : 0.f;
#pragma unroll
        for (int mi = 0; mi < FM; ++mi) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                int row = bm + wr * FM * 16 + mi * 16 + (lane >> 4) * 4 + r;
                if (row < M && col < N) {
                    if (slab != nullptr)
                        slab[(int64_t)row * N + col] = acc[mi][ni][r];
                    else
                        Y[(int64_t)row * N + col] =
                            f2bf(apply_act(acc[mi][ni][r] + bv, act));
                }
            }
        }
    }
}

// ---------------------------------------------------------------------
// skinny kernel: M <= RF*16; grid (ceil(N/64), splitk); 4 waves of 16
// cols; A fragments straight from global (x is L2-resident and tiny), W
// fragments streamed from global.  Yf == null stores the final bf16
// (needs splitk == 1); otherwise block row kq stores its K-chunk's
// partial sums into fp32 slab kq and a separate epilogue kernel combines
// (an empty trailing chunk stores zeros).
//
// K % 32 == 0 (launch_skinny checks it), so no K tail exists; ragged M
// and N are handled by clamped load rows and guarded stores, and the K
// loop carries no edge test.
//
// TANHA (slab mode): the A operand is not read but built as
// it loads, a = f2bf(Af * (1 - Ay^2)) from an fp32 gradient Af and the
// bf16 tanh output Ay (what act_bwd_f32_out computes, same rounding);
// wave 0 of the blockIdx.x == 0 blocks stores its K-chunk of it to Apre.
// ---------------------------------------------------------------------

template <int RF, bool TANHA>
__global__ __launch_bounds__(256)
void skinny_gemm_kernel(const bf16* __restrict__ A,   // [M,K], M <= RF*16
                        const bf16* __restrict__ W,   // [N,K]
                        const bf16* __restrict__ bias,
                        bf16* __restrict__ Y,         // [M,N]
                        float* __restrict__ Yf,       // [splitk,M,N] slabs
                        int M, int N, int K, int act, int splitk,
                        const float* __restrict__ Af,   // [M,K]
                        const bf16* __restrict__ Ay,    // [M,K]
                        bf16* __restrict__ Apre) {      // [M,K]
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int n0 = blockIdx.x * 64 + wave * 16;
    const bool active = (n0 < N);

    const int kq = blockIdx.y;
    const int kchunk = ((K / 32 + splitk - 1) / splitk) * 32;
    const int kbeg = kq * kchunk;
    const int kend = min(K, kbeg + kchunk);

    const int lrow = lane & 15;
    const int kgrp = lane >> 4;

    floatx4 acc[RF];
#pragma unroll
    for (int i = 0; i < RF; ++i)
        acc[i] = floatx4{0.f, 0.f, 0.f, 0.f};

    if (active) {
        // Rows past M / N are clamped onto the last valid one, not
        // branched around: an MFMA output row depends on its own A row
        // only (a column on its own W row), and the stores below drop
        // them.  With no edge test left, the loads of a whole batch of
        // K steps are issued before the first MFMA waits for one.
        const bf16* wp = W + (int64_t)min(n0 + lrow, N - 1) * K + kgrp * 8;
        int64_t aoff[RF];
#pragma unroll
        for (int mi = 0; mi < RF; ++mi)
            aoff[mi] = (int64_t)min(mi * 16 + lrow, M - 1) * K + kgrp * 8;
        const bool pre = TANHA && blockIdx.x == 0 && wave == 0;

        // U consecutive 32-wide K steps from k: all loads, then the MFMAs
        // in k order (each accumulator sums k-ascending, as one step at a
        // time does)
        auto steps = [&](auto uc, int k) {
            constexpr int U = decltype(uc)::value;
            bf16x8 bw[U], a[U][RF];
            floatx4 g0[TANHA ? U : 1][RF], g1[TANHA ? U : 1][RF];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                bw[u] = *(const bf16x8*)(wp + k + u * 32);
#pragma unroll
                for (int mi = 0; mi < RF; ++mi) {
                    const int64_t ao = aoff[mi] + k + u * 32;
                    if constexpr (TANHA) {
                        g0[u][mi] = *(const floatx4*)(Af + ao);
                        g1[u][mi] = *(const floatx4*)(Af + ao + 4);
                        a[u][mi] = *(const bf16x8*)(Ay + ao);
                    } else {
                        a[u][mi] = *(const bf16x8*)(A + ao);
                    }
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int mi = 0; mi < RF; ++mi) {
                    if constexpr (TANHA) {
                        bf16x8 yv = a[u][mi];
#pragma unroll
                        for (int e = 0; e < 8; ++e) {
                            float y = bf2f(yv[e]);
                            float g = e < 4 ? g0[u][mi][e]
                                            : g1[u][mi][e - 4];
                            // y*y is exact in fp32 (bf16 operand), so
                            // contraction cannot move this result
                            a[u][mi][e] = f2bf(g * (1.f - y * y));
                        }
                        if (pre && mi * 16 + lrow < M)
                            *(bf16x8*)(Apre + aoff[mi] + k + u * 32)
                                = a[u][mi];
                    }
                    acc[mi] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                        a[u][mi], bw[u], acc[mi], 0, 0, 0);
                }
        };

        // batch depth: ~12 fragments in flight (8 for TANHA, whose A
        // operand is three loads), so registers stay bounded at any K;
        // a flagship split (2-6 steps) is one batch
        constexpr int U = TANHA ? (RF >= 8 ? 1 : 8 / RF)
                                : (RF >= 8 ? 2 : 12 / RF);
        int k = kbeg;
        for (; k + U * 32 <= kend; k += U * 32)
            steps(std::integral_constant<int, U>{}, k);
        if constexpr (U > 2)
            for (; k + 64 <= kend; k += 64)
                steps(std::integral_constant<int, 2>{}, k);
        if constexpr (U > 1)
            for (; k < kend; k += 32)
                steps(std::integral_constant<int, 1>{}, k);
    }

    const int col = n0 + (lane & 15);
    if (!active || col >= N) return;
    if (Yf == nullptr) {
        float bv = (bias != nullptr) ? bf2f(bias[col]) : 0.f;
#pragma unroll
        for (int mi = 0; mi < RF; ++mi)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                int row = mi * 16 + (lane >> 4) * 4 + r;
                if (row < M)
                    Y[(int64_t)row * N + col] =
                        f2bf(apply_act(acc[mi][r] + bv, act));
            }
        return;
    }

    // split-K slab store; the caller's epilogue kernel reduces
    float* slab = Yf + (int64_t)kq * M * N;
#pragma unroll
    for (int mi = 0; mi < RF; ++mi)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            int row = mi * 16 + (lane >> 4) * 4 + r;
            if (row < M)
                slab[(int64_t)row * N + col] = acc[mi][r];
        }
}

// split-K combine + bias/act for both GEMM kernels' fp32 slabs
template <int S>
__global__ void skinny_epilogue_kernel(const float* __restrict__ Yf,
                                       const bf16* __restrict__ bias,
                                       bf16* __restrict__ Y,
                                       int64_t n, int N, int act,
                                       int splitk) {
    int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n) return;
    // the bias load goes out with the slab loads: always a valid address,
    // the value is dropped when there is no bias
    const bf16* bp = bias != nullptr ? bias + idx % N : (const bf16*)Yf;
    float bv = bf2f(*bp);
    float v = sum_slabs<S>(Yf, n, idx, splitk);
    if (bias != nullptr) v += bv;
    Y[idx] = f2bf(apply_act(v, act));
}

__global__ void dense_glds_kernel(const bf16* __restrict__ A,
                                  const bf16* __restrict__ W,
                                  const bf16* __restrict__ bias,
                                  bf16* __restrict__ Y,
                                  int M, int N, int K, int act);

// ---------------------------------------------------------------------
// host side: one launch function per kernel family
// ---------------------------------------------------------------------

static bool is_skinny(int64_t M, int64_t K) {
    return M <= 128 && K % 32 == 0;
}

// skinny grid: 64-column blocks, K split across blocks until ~3/4 of the
// 256 CUs have one (every split keeps at least two 32-wide MFMA steps)
struct SkinnyPlan { int nblocks, splitk; };

static SkinnyPlan skinny_plan(int64_t N, int64_t K) {
    int nblocks = cdiv(N, 64);
    int splitk = 1;
    while (nblocks * splitk < 192 && splitk < 8 &&
           (int)(K / 32) >= 2 * splitk)
        splitk *= 2;
    return {nblocks, splitk};
}

// the one skinny launch (RF by M).  yf == null: bias/act and the final
// bf16 into y, plan.splitk must be 1; otherwise fp32 partial sums into
// the yf slabs and bias / y / act are unused.
static void launch_skinny(hipStream_t stream, const at::Tensor& x,
                          const at::Tensor& w, const bf16* bias, bf16* y,
                          float* yf, int act, SkinnyPlan plan) {
    const int M = x.size(0), K = x.size(1), N = w.size(0);
    TORCH_CHECK(is_skinny(M, K),
                "skinny GEMM: M <= 128 and K % 32 == 0 only");
    auto kernel = M <= 32 ? skinny_gemm_kernel<2, false>
                : M <= 64 ? skinny_gemm_kernel<4, false>
                          : skinny_gemm_kernel<8, false>;
    hipLaunchKernelGGL(kernel, dim3(plan.nblocks, plan.splitk), dim3(256),
                       0, stream, (const bf16*)x.data_ptr(),
                       (const bf16*)w.data_ptr(), bias, y, yf, M, N, K,
                       act, plan.splitk, (const float*)nullptr,
                       (const bf16*)nullptr, (bf16*)nullptr);
}

// dense_fwd_drop's GEMM with act_bwd_f32_out folded into the A-operand
// load: slabs of (dy * (1 - y^2)) @ w^T, dy [M,K] fp32, y [M,K] bf16 the
// tanh output; dpre_out [M,K] receives the bf16 A operand (the batched
// weight/bias gradients still read it).  The consumer finishes the slabs
// (dexp_lstm_bwd_slabs, or slab_epilogue_drop after the loop).
at::Tensor dense_tanhbwd_slabs(at::Tensor dy, at::Tensor y, at::Tensor w,
                               at::Tensor dpre_out) {
    CHECK_GPU(dy); CHECK_CONTIG(dy); CHECK_F32(dy);
    CHECK_GPU(y); CHECK_CONTIG(y); CHECK_BF16(y);
    CHECK_GPU(w); CHECK_CONTIG(w); CHECK_BF16(w);
    CHECK_GPU(dpre_out); CHECK_CONTIG(dpre_out); CHECK_BF16(dpre_out);
    TORCH_CHECK(dy.dim() == 2 && w.dim() == 2);
    const int M = dy.size(0), K = dy.size(1), N = w.size(0);
    TORCH_CHECK(w.size(1) == K && y.numel() == dy.numel()
                && dpre_out.numel() == dy.numel(), "shape mismatch");
    TORCH_CHECK(is_skinny(M, K),
                "skinny GEMM: M <= 128 and K % 32 == 0 only");
    SkinnyPlan plan = skinny_plan(N, K);
    auto yf = at::empty({plan.splitk, M, N}, dy.options());
    auto kernel = M <= 32 ? skinny_gemm_kernel<2, true>
                : M <= 64 ? skinny_gemm_kernel<4, true>
                          : skinny_gemm_kernel<8, true>;
    hipStream_t stream = at::cuda::getCurrentCUDAStream();
    hipLaunchKernelGGL(kernel, dim3(plan.nblocks, plan.splitk), dim3(256),
                       0, stream, (const bf16*)nullptr,
                       (const bf16*)w.data_ptr(), (const bf16*)nullptr,
                       (bf16*)nullptr, (float*)yf.data_ptr(), M, N, K,
                       ACT_NONE, plan.splitk,
                       (const float*)dy.data_ptr(),
                       (const bf16*)y.data_ptr(),
                       (bf16*)dpre_out.data_ptr());
    HIP_OK(hipGetLastError());
    return yf;
}

// slab-mode skinny GEMM for entry points that bring their own epilogue:
// returns the [splitk, M, N] fp32 partial sums of x @ w^T
static at::Tensor skinny_slabs(hipStream_t stream, const at::Tensor& x,
                               const at::Tensor& w) {
    SkinnyPlan plan = skinny_plan(w.size(0), x.size(1));
    auto yf = at::empty({plan.splitk, x.size(0), w.size(0)},
                        x.options().dtype(at::kFloat));
    launch_skinny(stream, x, w, nullptr, nullptr, (float*)yf.data_ptr(),
                  ACT_NONE, plan);
    return yf;
}

// the one tiled launch: 128x64 tile for N <= 512, else 128x128.
// yf != null: split-K slab mode (grid z = splitk, kchunk of K each)
static void launch_tiled(hipStream_t stream, const at::Tensor& x,
                         const at::Tensor& w, const bf16* bias, bf16* y,
                         float* yf, int act, int splitk, int kchunk) {
    const int M = x.size(0), K = x.size(1), N = w.size(0);
    const bool narrow = N <= 512;
    auto kernel = narrow ? tiled_gemm_kernel<4, 1, 2, 4>
                         : tiled_gemm_kernel<2, 2, 4, 4>;
    dim3 grid(cdiv(N, narrow ? 64 : 128), cdiv(M, 128), splitk);
    hipLaunchKernelGGL(kernel, grid, dim3(256), 0, stream,
                       (const bf16*)x.data_ptr(),
                       (const bf16*)w.data_ptr(), bias, y, M, N, K, act,
                       yf, kchunk);
}

// y[M,N] = act(sum of the yf slabs + bias)
static void launch_epilogue(hipStream_t stream, const at::Tensor& yf,
                            const bf16* bias, at::Tensor& y, int act) {
    int64_t n = y.numel();
    const int splitk = (int)yf.size(0);
#define LAUNCH_EPI(S) \
    hipLaunchKernelGGL(skinny_epilogue_kernel<S>, dim3(cdiv(n, 256)), \
                       dim3(256), 0, stream, (const float*)yf.data_ptr(), \
                       bias, (bf16*)y.data_ptr(), n, (int)y.size(1), act, \
                       splitk)
    SLAB_DISPATCH(splitk, LAUNCH_EPI)
#undef LAUNCH_EPI
}

at::Tensor dense_fwd(at::Tensor x, at::Tensor w, at::Tensor bias,
                     int64_t act) {
    CHECK_GPU(x); CHECK_CONTIG(x); CHECK_BF16(x);
    CHECK_GPU(w); CHECK_CONTIG(w); CHECK_BF16(w);
    TORCH_CHECK(x.dim() == 2 && w.dim() == 2, "dense_fwd expects 2-D inputs");
    const int64_t M = x.size(0), K = x.size(1), N = w.size(0);
    TORCH_CHECK(w.size(1) == K, "weight inner dim mismatch");
    TORCH_CHECK(K % 8 == 0, "K must be a multiple of 8 (bf16x8 loads)");
    const bf16* bias_ptr = nullptr;
    if (bias.defined() && bias.numel() > 0) {
        CHECK_GPU(bias); CHECK_CONTIG(bias); CHECK_BF16(bias);
        TORCH_CHECK(bias.numel() == N, "bias size mismatch");
        bias_ptr = (const bf16*)bias.data_ptr();
    }
    const bool skinny = is_skinny(M, K);
    if (!skinny && M >= 16384 && N >= 256 && N % 8 == 0 && K % 64 == 0
        && K >= 128) {
        // big-M dense shapes: the 8-phase deep-pipelined 256^2 tile
        // (gemm8p.hip; the 2-barrier glds tile measured only ~190 TF
        // here — short K leaves it prologue-bound)
        return dense_8p_fwd(x, w, bias_ptr != nullptr ? bias : at::Tensor(),
                            act);
    }
    auto y = at::empty({M, N}, x.options());
    hipStream_t stream = at::cuda::getCurrentCUDAStream();

    if (skinny) {
        SkinnyPlan plan = skinny_plan(N, K);
        if (plan.splitk == 1) {
            launch_skinny(stream, x, w, bias_ptr, (bf16*)y.data_ptr(),
                          nullptr, (int)act, plan);
        } else {
            auto yf = skinny_slabs(stream, x, w);
            launch_epilogue(stream, yf, bias_ptr, y, (int)act);
        }
    } else if (M >= 16384 && N % 128 == 0 && K % 64 == 0) {
        // (retained) glds-staged 128^2 tile: the big-M shapes the
        // 8-phase kernel does not take (N < 256 or K < 128)
        dim3 grid(cdiv(N, 128), cdiv(M, 128));
        hipLaunchKernelGGL(dense_glds_kernel, grid, dim3(256), 0,
                           stream,
                           (const bf16*)x.data_ptr(),
                           (const bf16*)w.data_ptr(), bias_ptr,
                           (bf16*)y.data_ptr(), (int)M, (int)N, (int)K,
                           (int)act);
    } else {
        // mid-M shapes (the decode-head GEMMs: M=640, N=1024..1536)
        // leave the 2-barrier tile grid at 40-60 blocks on 256 CUs;
        // split K until ~2/3 of the chip has a block (measured 28-42 TF
        // -> the slab+epilogue pair more than doubles it)
        int tiles = cdiv(N, N <= 512 ? 64 : 128) * cdiv(M, 128);
        int splitk = 1;
        while (tiles * splitk < 160 && splitk < 8
               && K >= 128 * 2 * splitk)
            splitk *= 2;
        int kchunk = cdiv(cdiv(K, splitk), 64) * 64;
        splitk = cdiv(K, kchunk);
        if (splitk == 1) {
            launch_tiled(stream, x, w, bias_ptr, (bf16*)y.data_ptr(),
                         nullptr, (int)act, 1, kchunk);
        } else {
            auto yf = at::empty({splitk, M, N},
                                x.options().dtype(at::kFloat));
            launch_tiled(stream, x, w, bias_ptr, (bf16*)y.data_ptr(),
                         (float*)yf.data_ptr(), (int)act, splitk, kchunk);
            launch_epilogue(stream, yf, bias_ptr, y, (int)act);
        }
    }
    HIP_OK(hipGetLastError());
    return y;
}

// ---- GEMM + counter-hash dropout fused into the split-K epilogue ----

template <int S>
__global__ void skinny_epilogue_drop_kernel(
        const float* __restrict__ Yf, bf16* __restrict__ Y,
        const int64_t* __restrict__ seed_p, int64_t n, int splitk,
        float p, int salt) {
    int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n) return;
    float v = sum_slabs<S>(Yf, n, idx, splitk);
    v *= drop_scale((uint32_t)(*seed_p), salt, (uint32_t)idx, p);
    Y[idx] = f2bf(v);
}

// y = bf16(sum of the yf slabs * dropout mask(salt))
static void launch_epilogue_drop(hipStream_t stream, const at::Tensor& yf,
                                 at::Tensor& y, const at::Tensor& seed,
                                 double p, int64_t salt) {
    int64_t n = y.numel();
    const int splitk = (int)yf.size(0);
#define LAUNCH_EPI(S) \
    hipLaunchKernelGGL(skinny_epilogue_drop_kernel<S>, \
                       dim3(cdiv(n, 256)), dim3(256), 0, stream, \
                       (const float*)yf.data_ptr(), (bf16*)y.data_ptr(), \
                       (const int64_t*)seed.data_ptr(), n, splitk, \
                       (float)p, (int)salt)
    SLAB_DISPATCH(splitk, LAUNCH_EPI)
#undef LAUNCH_EPI
}

at::Tensor dense_fwd_drop(at::Tensor x, at::Tensor w, at::Tensor seed,
                          double p, int64_t salt) {
    // bias-free, activation-free skinny GEMM whose split-K epilogue
    // applies hash dropout (salt/index convention of hash_dropout) —
    // removes one elementwise launch per decoder reverse step
    CHECK_GPU(x); CHECK_CONTIG(x); CHECK_BF16(x);
    CHECK_GPU(w); CHECK_CONTIG(w); CHECK_BF16(w);
    int64_t M = x.size(0), K = x.size(1), N = w.size(0);
    if (p <= 0.0 || !is_skinny(M, K)) {
        // non-skinny shapes: plain GEMM + the separate dropout pass
        auto y = dense_fwd(x, w, at::Tensor(), ACT_NONE);
        return p > 0.0 ? hash_dropout(y, seed, p, salt) : y;
    }
    auto y = at::empty({M, N}, x.options());
    hipStream_t stream = at::cuda::getCurrentCUDAStream();
    auto yf = skinny_slabs(stream, x, w);
    launch_epilogue_drop(stream, yf, y, seed, p, salt);
    HIP_OK(hipGetLastError());
    return y;
}

// the drop epilogue alone, over slabs some other entry point produced:
// y = bf16(sum_slabs * dropout mask(salt))
at::Tensor slab_epilogue_drop(at::Tensor yf, at::Tensor seed, double p,
                              int64_t salt) {
    CHECK_GPU(yf); CHECK_CONTIG(yf); CHECK_F32(yf);
    TORCH_CHECK(yf.dim() == 3, "slabs must be [splitk, M, N]");
    auto y = at::empty({yf.size(1), yf.size(2)},
                       yf.options().dtype(at::kBFloat16));
    hipStream_t stream = at::cuda::getCurrentCUDAStream();
    launch_epilogue_drop(stream, yf, y, seed, p, salt);
    HIP_OK(hipGetLastError());
    return y;
}

// ---- fused skinny epilogues for the BPTT step chain (B <= 128) ----

// the four pre-activation gates of (b, hh): split-K sum + bias, written
// to gates[] as bf16 (saved for backward) and returned in fp32
//
// The 4*S slab loads, the 4 bias loads and c_prev[b, hh] (returned in
// cp) all go out before the first add.  The bias address is valid with
// or without a bias (the value is dropped without one), so no load sits
// behind a branch.  4*B*H < 2^31 (the hosts check it).
template <int S>
__device__ __forceinline__ void sum_gates(const float* __restrict__ Yf,
                                          const bf16* __restrict__ bias,
                                          const bf16* __restrict__ c_prev,
                                          bf16* __restrict__ gates,
                                          int B, int H, int b, int hh,
                                          int splitk, float g[4],
                                          float& cp) {
    const int n = B * 4 * H;
    const int off0 = b * 4 * H + hh;
    const bf16* bp = bias != nullptr ? bias + hh : c_prev;
    const int bstride = bias != nullptr ? H : 0;
    float s[4][S > 0 ? S : 1];
    bf16 bv[4];
    if constexpr (S > 0) {
#pragma unroll
        for (int q = 0; q < 4; ++q) load_slabs<S>(Yf, n, off0 + q * H, s[q]);
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) bv[q] = bp[q * bstride];
    cp = bf2f(c_prev[b * H + hh]);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        float acc;
        if constexpr (S > 0) acc = add_slabs<S>(s[q]);
        else acc = sum_slabs<0>(Yf, n, off0 + q * H, splitk);
        if (bias != nullptr) acc += bf2f(bv[q]);
        gates[off0 + q * H] = f2bf(acc);
        g[q] = acc;
    }
}

// gates epilogue + LSTM pointwise: thread per (b,h) sums the 4 gate
// elements across split-K slabs, applies the LSTM gate math, writes the
// bf16 gates plus h_raw and c_new.
template <int S>
__global__ void skinny_epi_lstm_kernel(const float* __restrict__ Yf,
                                       const bf16* __restrict__ bias,
                                       const bf16* __restrict__ c_prev,
                                       bf16* __restrict__ gates,
                                       bf16* __restrict__ h_out,
                                       bf16* __restrict__ c_out,
                                       int B, int H, int splitk,
                                       float fb) {
    int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= B * H) return;
    float g[4], cp, cn, h;
    sum_gates<S>(Yf, bias, c_prev, gates, B, H, idx / H, idx % H, splitk,
                 g, cp);
    lstm_cell_fwd(g, cp, fb, cn, h);
    h_out[idx] = f2bf(h);
    c_out[idx] = f2bf(cn);
}

std::vector<at::Tensor> dense_lstm_fwd(at::Tensor xh, at::Tensor wl,
                                       at::Tensor bl, at::Tensor c_prev,
                                       double fb) {
    // gates = xh @ wl^T + bl ; (h_raw, c_new) = LSTM(gates, c_prev)
    int64_t M = xh.size(0), N = wl.size(0);
    int B = c_prev.size(0), H = c_prev.size(1);
    TORCH_CHECK(M == B && N == 4 * H);
    auto gates = at::empty({M, N}, xh.options());
    auto h_out = at::empty_like(c_prev);
    auto c_out = at::empty_like(c_prev);
    hipStream_t s = at::cuda::getCurrentCUDAStream();
    TORCH_CHECK(M * N < (1LL << 31), "gates have >= 2^31 elements");
    auto yf = skinny_slabs(s, xh, wl);
    const int splitk = (int)yf.size(0);
#define LAUNCH_EPI(S) \
    hipLaunchKernelGGL(skinny_epi_lstm_kernel<S>, \
                       dim3(cdiv(B * H, 256)), dim3(256), 0, s, \
                       (const float*)yf.data_ptr(), \
                       (const bf16*)bl.data_ptr(), \
                       (const bf16*)c_prev.data_ptr(), \
                       (bf16*)gates.data_ptr(), (bf16*)h_out.data_ptr(), \
                       (bf16*)c_out.data_ptr(), B, H, splitk, (float)fb)
    SLAB_DISPATCH(splitk, LAUNCH_EPI)
#undef LAUNCH_EPI
    HIP_OK(hipGetLastError());
    return {gates, h_out, c_out};
}


// ---------------------------------------------------------------------
// glds-staged 128x128 dense GEMM for big-M shapes (the attention
// projection T1: [T*B*L, 512] x [512, 512] ran at 148 TF on the
// register-staged 2-barrier tile; the glds + XOR-swizzle structure
// measured 536-658 TF on the conv igemm with identical geometry).
// Same discipline as conv_igemm_glds_kernel: global_load_lds width 16,
// lane-linear LDS, st_16x32 swizzle pre-applied to the per-lane GLOBAL
// source address and XOR'd on the fragment reads.  K % 64 == 0.
// ---------------------------------------------------------------------

__global__ __launch_bounds__(256)
void dense_glds_kernel(const bf16* __restrict__ A,   // [M,K]
                       const bf16* __restrict__ W,   // [N,K]
                       const bf16* __restrict__ bias,
                       bf16* __restrict__ Y,
                       int M, int N, int K, int act) {
    constexpr int BM = 128, BN = 128, BKc = 64;
    __shared__ bf16 lds[2 * BM * BKc];
    bf16* As = lds;
    bf16* Bs = lds + BM * BKc;

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int wr = wave >> 1, wc = wave & 1;
    const int bm = blockIdx.y * BM;
    const int bn = blockIdx.x * BN;

    // per-lane staged rows (4 per wave for each operand) + source swz
    const bf16* aSrc[4];
    const bf16* wSrc[4];
    const int ci8 = (lane & 7) * 8;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        int r = wave * 32 + i * 8 + (lane >> 3);
        int swz = (r & 4) ? 16 : 0;
        int ga = bm + r;
        if (ga >= M) ga = M - 1;
        aSrc[i] = A + (int64_t)ga * K + (ci8 ^ swz);
        int gb = bn + r;
        if (gb >= N) gb = N - 1;
        wSrc[i] = W + (int64_t)gb * K + (ci8 ^ swz);
    }

    floatx4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
            acc[i][j] = floatx4{0.f, 0.f, 0.f, 0.f};

    const int lrow = lane & 15;
    const int kgrp = lane >> 4;

    for (int k0 = 0; k0 < K; k0 += BKc) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            __builtin_amdgcn_global_load_lds(
                (const __attribute__((address_space(1))) uint32_t*)
                    (aSrc[i] + k0),
                (__attribute__((address_space(3))) uint32_t*)
                    (As + (wave * 32 + i * 8) * BKc),
                16, 0, 0);
            __builtin_amdgcn_global_load_lds(
                (const __attribute__((address_space(1))) uint32_t*)
                    (wSrc[i] + k0),
                (__attribute__((address_space(3))) uint32_t*)
                    (Bs + (wave * 32 + i * 8) * BKc),
                16, 0, 0);
        }
        __syncthreads();

#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
            bf16x8 a_frag[4], b_frag[4];
            const int kof = kk * 32 + kgrp * 8;
#pragma unroll
            for (int mi = 0; mi < 4; ++mi) {
                int r = wr * 64 + mi * 16 + lrow;
                a_frag[mi] = *(const bf16x8*)(
                    As + r * BKc + (kof ^ ((r & 4) ? 16 : 0)));
            }
#pragma unroll
            for (int ni = 0; ni < 4; ++ni) {
                int r = wc * 64 + ni * 16 + lrow;
                b_frag[ni] = *(const bf16x8*)(
                    Bs + r * BKc + (kof ^ ((r & 4) ? 16 : 0)));
            }
#pragma unroll
            for (int mi = 0; mi < 4; ++mi)
#pragma unroll
                for (int ni = 0; ni < 4; ++ni)
                    acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                        a_frag[mi], b_frag[ni], acc[mi][ni], 0, 0, 0);
        }
        __syncthreads();
    }

#pragma unroll
    for (int ni = 0; ni < 4; ++ni) {
        int col = bn + wc * 64 + ni * 16 + (lane & 15);
        float bv = (bias != nullptr && col < N) ? bf2f(bias[col]) : 0.f;
#pragma unroll
        for (int mi = 0; mi < 4; ++mi) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                int row = bm + wr * 64 + mi * 16 + (lane >> 4) * 4 + r;
                if (row < M && col < N) {
                    float vv = acc[mi][ni][r] + bv;
                    Y[(int64_t)row * N + col] = f2bf(apply_act(vv, act));
                }
            }
        }
    }
}

// ---------------------------------------------------------------------
// dxh GEMM with the dx_fuse scatter folded into the split-K epilogue:
// dxh = dgates @ wl^T, then per element: input-dropout mask regen and
// the split into dpooled (+dpool_dec), DEMB slab (+demb_dec), dsth.
// Removes one launch + the dxh round trip per decoder reverse step.
// ---------------------------------------------------------------------

template <int S>
__global__ void skinny_epi_dx_kernel(const float* __restrict__ Yf,
                                     const bf16* __restrict__ dpool_dec,
                                     const bf16* __restrict__ demb_dec,
                                     const int64_t* __restrict__ seed_p,
                                     bf16* __restrict__ dpooled,
                                     bf16* __restrict__ demb_out,
                                     bf16* __restrict__ dsth,
                                     int n, int splitk,
                                     int B, int D, int E, int H,
                                     float p, int salt) {
    const uint32_t seed = (uint32_t)(*seed_p);
    const int I = D + E;
    const int W = I + H;
    int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n) return;
    int b = idx / W, j = idx - b * W;
    // the decoder-side addend goes out with the slab loads, selected by
    // address (the H range reads a valid element it does not use)
    const bf16* addp = j < D ? dpool_dec + b * D + j
                     : j < I ? demb_dec + b * E + (j - D)
                             : (const bf16*)Yf;
    float add = bf2f(*addp);
    float g = sum_slabs<S>(Yf, n, idx, splitk);
    if (j < I) {
        // the mask multiply and the add each round on their own, as they
        // did while the addend was loaded after the multiply; with it
        // already in a register the compiler would fuse them into an FMA
#pragma clang fp contract(off)
        g *= drop_scale(seed, salt, (uint32_t)(b * I + j), p);
        if (j < D)
            dpooled[b * D + j] = f2bf(g + add);
        else
            demb_out[b * E + (j - D)] = f2bf(g + add);
    } else {
        dsth[b * H + (j - I)] = f2bf(g);
    }
}

std::vector<at::Tensor> dense_dx_fuse(at::Tensor dgates, at::Tensor wl_t,
                                      at::Tensor dpool_dec,
                                      at::Tensor demb_dec,
                                      at::Tensor seed,
                                      at::Tensor demb_out,
                                      double p, int64_t salt,
                                      int64_t D, int64_t E, int64_t H) {
    CHECK_GPU(dgates); CHECK_CONTIG(dgates); CHECK_BF16(dgates);
    CHECK_GPU(wl_t); CHECK_CONTIG(wl_t); CHECK_BF16(wl_t);
    int64_t M = dgates.size(0), N = wl_t.size(0);
    TORCH_CHECK(N == D + E + H);
    auto dpooled = at::empty({M, D}, dgates.options());
    auto dsth = at::empty({M, H}, dgates.options());
    hipStream_t stream = at::cuda::getCurrentCUDAStream();
    auto yf = skinny_slabs(stream, dgates, wl_t);
    int64_t n = M * N;
    TORCH_CHECK(n < (1LL << 31), "dxh has >= 2^31 elements");
    const int splitk = (int)yf.size(0);
#define LAUNCH_EPI(S) \
    hipLaunchKernelGGL(skinny_epi_dx_kernel<S>, dim3(cdiv(n, 256)), \
                       dim3(256), 0, stream, \
                       (const float*)yf.data_ptr(), \
                       (const bf16*)dpool_dec.data_ptr(), \
                       (const bf16*)demb_dec.data_ptr(), \
                       (const int64_t*)seed.data_ptr(), \
                       (bf16*)dpooled.data_ptr(), \
                       (bf16*)demb_out.data_ptr(), \
                       (bf16*)dsth.data_ptr(), \
                       (int)n, splitk, (int)M, (int)D, (int)E, (int)H, \
                       (float)p, (int)salt)
    SLAB_DISPATCH(splitk, LAUNCH_EPI)
#undef LAUNCH_EPI
    HIP_OK(hipGetLastError());
    return {dpooled, dsth};
}

// ---------------------------------------------------------------------
// LSTM gates epilogue + the expand scatter in ONE launch: the H-range
// threads finish the gate math and write sth / EXPD-h / od_next
// directly (h_raw and out_t never touch HBM); D/E threads do the
// pooled / embedding-gather parts of the expand row.  Replaces
// skinny_epi_lstm + expand_fuse.  Dropout salts identical to the pair
// it replaces (s+4 out, s+5 state, s+6 expand, s+17 next attend).
//
// xh_next != null: the threads also lay down the NEXT step's LSTM input
// row where they already hold its values — H-range threads the state_h
// columns [I, I+H), E-range threads dropout(table[next_ids], salt s+16+3)
// into [D, I) — so no lstm_in_fuse launch sits between the steps (the
// pooled columns [0, D) come from the next step's attn_pool_fwd_xh).
// ---------------------------------------------------------------------

template <int S, bool XN>   // S: slab count (common.h); XN: xh_next given
__global__ void skinny_epi_lstm_expand_kernel(
        const float* __restrict__ Yf, const bf16* __restrict__ bias,
        const bf16* __restrict__ c_prev,
        const bf16* __restrict__ pooled,
        const bf16* __restrict__ table,
        const int64_t* __restrict__ ids,
        const int64_t* __restrict__ seed_p,
        bf16* __restrict__ gates, bf16* __restrict__ c_out,
        bf16* __restrict__ sth_t, bf16* __restrict__ expdrop,
        bf16* __restrict__ od_next,
        int B, int H, int D, int E, int splitk,
        float fb, float p_lstm, float p_fc, int s,
        const int64_t* __restrict__ next_ids,
        bf16* __restrict__ xh_next) {
    const uint32_t seed = (uint32_t)(*seed_p);
    const int W = H + D + E;
    const int I = D + E;
    // B * W and 4 * B * H < 2^31 (the host checks it)
    int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= B * W) return;
    int b = idx / W, j = idx - b * W;
    float val;
    if (j < H) {
        float g[4], cp, cn, h;
        sum_gates<S>(Yf, bias, c_prev, gates, B, H, b, j, splitk, g, cp);
        lstm_cell_fwd(g, cp, fb, cn, h);
        c_out[b * H + j] = f2bf(cn);
        uint32_t hidx = (uint32_t)(b * H + j);
        float ot = h * drop_scale(seed, s + 4, hidx, p_lstm);
        bf16 sth = f2bf(h * drop_scale(seed, s + 5, hidx, p_lstm));
        sth_t[b * H + j] = sth;
        if constexpr (XN)
            xh_next[b * W + I + j] = sth;
        if (od_next != nullptr)
            od_next[b * H + j] =
                f2bf(ot * drop_scale(seed, s + 16 + 1, hidx, p_fc));
        val = ot;
    } else if (j < H + D) {
        val = bf2f(pooled[b * D + (j - H)]);
    } else {
        // both id loads first, then both table gathers: two round trips,
        // not four (XN is a template parameter so that no load waits
        // behind a test of xh_next)
        int e = j - H - D;
        int64_t id = ids[b], nid = 0;
        if constexpr (XN) nid = next_ids[b];
        bf16 tv = table[id * E + e];
        if constexpr (XN) {
            bf16 tn = table[nid * E + e];
            xh_next[b * W + D + e] =
                f2bf(bf2f(tn)
                     * drop_scale(seed, s + 16 + 3,
                                  (uint32_t)(b * I + D + e), p_lstm));
        }
        val = bf2f(tv);
    }
    expdrop[idx] = f2bf(val * drop_scale(seed, s + 6,
                                         (uint32_t)(b * W + j), p_fc));
}

static std::vector<at::Tensor> dense_lstm_expand_impl(
        at::Tensor xh, at::Tensor wl, at::Tensor bl, at::Tensor c_prev,
        at::Tensor pooled, at::Tensor table, at::Tensor ids,
        at::Tensor seed, at::Tensor expdrop, at::Tensor od_next,
        double fb, double p_lstm, double p_fc, int64_t s,
        const int64_t* next_ids_ptr, bf16* xh_next_ptr) {
    int64_t M = xh.size(0), N = wl.size(0);
    int B = c_prev.size(0), H = c_prev.size(1);
    int D = pooled.size(1), E = table.size(1);
    TORCH_CHECK(M == B && N == 4 * H);
    auto gates = at::empty({M, N}, xh.options());
    auto c_out = at::empty({B, H}, xh.options());
    auto sth_t = at::empty({B, H}, xh.options());
    hipStream_t stream = at::cuda::getCurrentCUDAStream();
    auto yf = skinny_slabs(stream, xh, wl);
    const bf16* bias_ptr = nullptr;
    if (bl.defined() && bl.numel() > 0)
        bias_ptr = (const bf16*)bl.data_ptr();
    bf16* od_ptr = nullptr;
    if (od_next.defined() && od_next.numel() > 0)
        od_ptr = (bf16*)od_next.data_ptr();
    int64_t n = (int64_t)B * (H + D + E);
    TORCH_CHECK(n < (1LL << 31) && M * N < (1LL << 31),
                "expand row or gates have >= 2^31 elements");
    const int splitk = (int)yf.size(0);
#define LAUNCH_EPI(S) \
    hipLaunchKernelGGL((xh_next_ptr != nullptr \
                            ? skinny_epi_lstm_expand_kernel<S, true> \
                            : skinny_epi_lstm_expand_kernel<S, false>), \
                       dim3(cdiv(n, 256)), dim3(256), 0, stream, \
                       (const float*)yf.data_ptr(), bias_ptr, \
                       (const bf16*)c_prev.data_ptr(), \
                       (const bf16*)pooled.data_ptr(), \
                       (const bf16*)table.data_ptr(), \
                       (const int64_t*)ids.data_ptr(), \
                       (const int64_t*)seed.data_ptr(), \
                       (bf16*)gates.data_ptr(), \
                       (bf16*)c_out.data_ptr(), \
                       (bf16*)sth_t.data_ptr(), \
                       (bf16*)expdrop.data_ptr(), od_ptr, \
                       B, H, D, E, splitk, \
                       (float)fb, (float)p_lstm, (float)p_fc, (int)s, \
                       next_ids_ptr, xh_next_ptr)
    SLAB_DISPATCH(splitk, LAUNCH_EPI)
#undef LAUNCH_EPI
    HIP_OK(hipGetLastError());
    return {gates, c_out, sth_t};
}

std::vector<at::Tensor> dense_lstm_expand_fwd(
        at::Tensor xh, at::Tensor wl, at::Tensor bl, at::Tensor c_prev,
        at::Tensor pooled, at::Tensor table, at::Tensor ids,
        at::Tensor seed, at::Tensor expdrop, at::Tensor od_next,
        double fb, double p_lstm, double p_fc, int64_t s) {
    return dense_lstm_expand_impl(xh, wl, bl, c_prev, pooled, table, ids,
                                  seed, expdrop, od_next, fb, p_lstm, p_fc,
                                  s, nullptr, nullptr);
}

// dense_lstm_expand_fwd that also writes the embedding (next_ids) and
// state columns of the next step's LSTM input rows xh_next [B, D+E+H];
// an empty xh_next (the last step) writes none
std::vector<at::Tensor> dense_lstm_expand_xh_fwd(
        at::Tensor xh, at::Tensor wl, at::Tensor bl, at::Tensor c_prev,
        at::Tensor pooled, at::Tensor table, at::Tensor ids,
        at::Tensor seed, at::Tensor expdrop, at::Tensor od_next,
        double fb, double p_lstm, double p_fc, int64_t s,
        at::Tensor next_ids, at::Tensor xh_next) {
    const int64_t* nid = nullptr;
    bf16* xn = nullptr;
    if (xh_next.defined() && xh_next.numel() > 0) {
        CHECK_GPU(xh_next); CHECK_CONTIG(xh_next); CHECK_BF16(xh_next);
        CHECK_GPU(next_ids); CHECK_CONTIG(next_ids);
        TORCH_CHECK(next_ids.scalar_type() == at::kLong
                    && next_ids.numel() == c_prev.size(0));
        TORCH_CHECK(xh_next.numel() == c_prev.size(0)
                    * (c_prev.size(1) + pooled.size(1) + table.size(1)));
        nid = (const int64_t*)next_ids.data_ptr();
        xn = (bf16*)xh_next.data_ptr();
    }
    return dense_lstm_expand_impl(xh, wl, bl, c_prev, pooled, table, ids,
                                  seed, expdrop, od_next, fb, p_lstm, p_fc,
                                  s, nid, xn);
}
