// Common helpers for the sat_amd CDNA4 (gfx950) kernel layer.
// MI355X-only: wave64, MFMA bf16, 160 KiB LDS/CU. No CUDA paths.
#pragma once

#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>

#define CHECK_GPU(x) TORCH_CHECK((x).is_cuda(), #x " must be on GPU")
#define CHECK_CONTIG(x) TORCH_CHECK((x).is_contiguous(), #x " must be contiguous")
#define CHECK_BF16(x) TORCH_CHECK((x).scalar_type() == at::kBFloat16, #x " must be bf16")
#define CHECK_F32(x) TORCH_CHECK((x).scalar_type() == at::kFloat, #x " must be fp32")

#define HIP_OK(expr) do { hipError_t _e = (expr); \
    TORCH_CHECK(_e == hipSuccess, "HIP error: ", hipGetErrorString(_e)); } while (0)

using bf16 = __bf16;
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) float floatx4;

static inline int cdiv(int64_t a, int64_t b) { return (int)((a + b - 1) / b); }

__device__ __forceinline__ float bf2f(bf16 v) { return (float)v; }
__device__ __forceinline__ bf16 f2bf(float v) { return (bf16)v; }

// wave-level sum over 64 lanes
__device__ __forceinline__ float wave_sum(float v) {
    for (int off = 32; off > 0; off >>= 1)
        v += __shfl_down(v, off, 64);
    return v;
}

__device__ __forceinline__ float wave_max(float v) {
    for (int off = 32; off > 0; off >>= 1)
        v = fmaxf(v, __shfl_down(v, off, 64));
    return v;
}

__device__ __forceinline__ float sigmoidf(float x) {
    return 1.0f / (1.0f + __expf(-x));
}

// counter-based dropout hash: deterministic in (seed, salt, index), so the
// backward regenerates the mask with zero storage, and the seed lives in a
// DEVICE scalar the model advances once per step (hipGraph-safe: replays
// see fresh masks, unlike a host-baked philox offset).  Every forward /
// backward mask pair in the extension goes through these three functions.
__device__ __forceinline__ uint32_t mix3(uint32_t a, uint32_t b, uint32_t c) {
    uint32_t h = a * 0x9E3779B1u ^ b * 0x85EBCA77u ^ c * 0xC2B2AE3Du;
    h ^= h >> 16; h *= 0x7FEB352Du;
    h ^= h >> 15; h *= 0x846CA68Bu;
    h ^= h >> 16;
    return h;
}

__device__ __forceinline__ float drop_scale(uint32_t seed, int salt,
                                            uint32_t idx, float p) {
    if (p <= 0.f) return 1.f;
    uint32_t h = mix3(seed, (uint32_t)salt, idx);
    float u = (h >> 8) * (1.0f / 16777216.0f);
    return u >= p ? 1.0f / (1.0f - p) : 0.0f;
}

// 8 masks from two hashes (one per 4 bytes): ~4x less ALU than 8
// per-element hashes.  Used by the attention scores fwd/bwd PAIR only —
// both sides must derive masks identically.  The byte compare quantises
// the drop rate to pq/256 with pq = floor(256 p), so the kept values are
// scaled by 256/(256 - pq), the inverse of the rate actually applied
// (1/(1-p) left E[scale] = 1.0045 at p = 0.3; the two agree at p = 0.5).
__device__ __forceinline__ void drop_scale8(uint32_t seed, int salt,
                                            uint32_t idx8, float p,
                                            float* sc) {
    if (p <= 0.f) {
#pragma unroll
        for (int e = 0; e < 8; ++e) sc[e] = 1.f;
        return;
    }
    uint32_t pq = (uint32_t)(p * 256.0f);
    float inv = 256.0f / (float)(256u - pq);
    uint32_t h1 = mix3(seed, (uint32_t)salt, idx8);
    uint32_t h2 = mix3(h1, (uint32_t)salt ^ 0xA5A5A5A5u, idx8);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        sc[e] = ((h1 >> (e * 8)) & 0xFFu) >= pq ? inv : 0.f;
        sc[4 + e] = ((h2 >> (e * 8)) & 0xFFu) >= pq ? inv : 0.f;
    }
}

// TF LSTMCell gate math in fp32: gate order i,j,f,o; forget bias added
// pre-sigmoid; no peepholes.  g[] are the four pre-activation gates.
//
// Contraction is OFF inside these helpers and every FMA is spelled out:
// left to -ffp-contract=fast the compiler fuses cp*gf + gi*gj on either
// product, and 1 - tc*tc or not, depending on the surrounding kernel, so
// kernels that must agree bitwise (each fusion and the pair it replaces,
// forward and recomputing backward) would drift apart by an fp32 ulp.
struct LstmAct { float gi, gj, gf, go, cn; };

__device__ __forceinline__ LstmAct lstm_act(const float g[4], float cp,
                                            float fb) {
#pragma clang fp contract(off)
    LstmAct a;
    a.gi = sigmoidf(g[0]);
    a.gj = tanhf(g[1]);
    a.gf = sigmoidf(g[2] + fb);
    a.go = sigmoidf(g[3]);
    a.cn = fmaf(a.gi, a.gj, cp * a.gf);
    return a;
}

__device__ __forceinline__ void lstm_cell_fwd(const float g[4], float cp,
                                              float fb, float& cn,
                                              float& h) {
    LstmAct a = lstm_act(g, cp, fb);
    cn = a.cn;
    h = tanhf(a.cn) * a.go;
}

// backward from the SAVED pre-activation gates (activations are
// recomputed, not stored): dg[] in gate order, dcp = dL/dc_prev.
__device__ __forceinline__ void lstm_cell_bwd(const float g[4], float cp,
                                              float dhv, float dcv,
                                              float fb, float dg[4],
                                              float& dcp) {
#pragma clang fp contract(off)
    LstmAct a = lstm_act(g, cp, fb);
    float tc = tanhf(a.cn);
    float dct = fmaf(dhv * a.go, 1.f - tc * tc, dcv);
    dg[0] = dct * a.gj * a.gi * (1.f - a.gi);             // di
    dg[1] = dct * a.gi * fmaf(-a.gj, a.gj, 1.f);          // dj
    dg[2] = dct * cp * a.gf * (1.f - a.gf);               // df
    dg[3] = dhv * tc * a.go * (1.f - a.go);               // do
    dcp = dct * a.gf;
}

// ---- "emit padded" output mode of the frozen-VGG producers ----
// A producer may write its [B,H,W,C] result into the interior of a
// [B,H+2,W+2,C] buffer and zero the 1-px border itself, so the next 3x3
// conv's glds staging reads it without a pad1_nhwc pass.  The thread that
// stores pixel (y,x) also zeroes the border pixels next to it, which
// covers every border pixel exactly once and needs no state or launch.

// Pixel row m of the [B,H,W] grid: (y,x) and the index of its interior
// slot in the padded buffer, in pixels (below 2^31 whenever the padded
// buffer has fewer than 2^31 pixels; the hosts check it).
struct PadPix { int pix, y, x; };

__device__ __forceinline__ PadPix pad_pix(int m, int H, int W) {
    int b = m / (H * W);
    int yx = m - b * (H * W);
    PadPix p;
    p.y = yx / W;
    p.x = yx - p.y * W;
    p.pix = (b * (H + 2) + p.y + 1) * (W + 2) + p.x + 1;
    return p;
}

// step to pixel row m+1 without dividing again (a lane of an MFMA
// epilogue owns runs of 4 consecutive rows); branch-free
__device__ __forceinline__ void pad_pix_next(PadPix& p, int H, int W) {
    const bool wx = (p.x + 1 == W);           // next image row
    const bool wy = wx && (p.y + 1 == H);     // next image
    p.pix += 1 + (wx ? 2 : 0) + (wy ? 2 * (W + 2) : 0);
    p.y = wy ? 0 : (wx ? p.y + 1 : p.y);
    p.x = wx ? 0 : p.x + 1;
}

// p = address of this thread's T-wide (bf16 or bf16x8) store at interior
// pixel (y,x): zero the same channels of the adjacent border pixels.
template <typename T>
__device__ __forceinline__ void pad_border_zero(bf16* p, int y, int x,
                                                int H, int W, int C) {
    const bool l = (x == 0), r = (x == W - 1);
    if (!(l || r || y == 0 || y == H - 1)) return;
    const int64_t rs = (int64_t)(W + 2) * C;   // padded row stride
    const T z = {};
    if (l) *(T*)(p - C) = z;
    if (r) *(T*)(p + C) = z;
    if (y == 0) {
        *(T*)(p - rs) = z;
        if (l) *(T*)(p - rs - C) = z;
        if (r) *(T*)(p - rs + C) = z;
    }
    if (y == H - 1) {
        *(T*)(p + rs) = z;
        if (l) *(T*)(p + rs - C) = z;
        if (r) *(T*)(p + rs + C) = z;
    }
}

// MFMA epilogues keep the border out of their unrolled store loops (128
// inlined copies of the edge tests made the 8-phase epilogue ~60 KB of
// straight-line code): after the stores, this compact loop walks a
// lane's run of 4 rows from row0 and zeroes the border next to its edge
// pixels in the lane's (up to 4) columns.
__device__ __forceinline__ void pad_border_run(bf16* out, int row0, int M,
                                               int H, int W, int C,
                                               const int (&cols)[4]) {
    if (row0 >= M) return;
    PadPix p = pad_pix(row0, H, W);
#pragma unroll 1
    for (int r = 0; r < 4 && row0 + r < M; ++r) {
        if (r) pad_pix_next(p, H, W);
        if (p.x == 0 || p.x == W - 1 || p.y == 0 || p.y == H - 1) {
            bf16* q = out + (int64_t)p.pix * C;
#pragma unroll 1
            for (int j = 0; j < 4; ++j)
                if (cols[j] < C)
                    pad_border_zero<bf16>(q + cols[j], p.y, p.x, H, W, C);
        }
    }
}

// Output of a producer: [B,C,H,W] channels-last, or [B,C,H+2,W+2] with
// emit_pad.  A caller-supplied `out` is used in place of a fresh
// allocation after its shape, dtype and layout are checked.
static inline at::Tensor nhwc_out(const at::Tensor& like, int64_t B,
                                  int64_t C, int64_t H, int64_t W,
                                  bool emit_pad,
                                  const c10::optional<at::Tensor>& out) {
    const int64_t Ho = emit_pad ? H + 2 : H, Wo = emit_pad ? W + 2 : W;
    TORCH_CHECK(B * Ho * Wo < (1LL << 31), "output has >= 2^31 pixels");
    if (out.has_value() && out->defined()) {
        CHECK_GPU(*out); CHECK_BF16(*out);
        TORCH_CHECK(out->dim() == 4 && out->size(0) == B
                    && out->size(1) == C && out->size(2) == Ho
                    && out->size(3) == Wo,
                    "out: expected [", B, ",", C, ",", Ho, ",", Wo, "]");
        TORCH_CHECK(out->is_contiguous(at::MemoryFormat::ChannelsLast),
                    "out must be channels_last");
        TORCH_CHECK(out->device() == like.device(),
                    "out must be on the input's device");
        return *out;
    }
    return at::empty({B, C, Ho, Wo},
                     like.options()
                         .memory_format(at::MemoryFormat::ChannelsLast));
}

// split-K combine: element `off` summed over the fp32 slabs of n.
//
// S > 0 is the slab count at compile time: all S loads are issued before
// the first add, so a thread pays one memory round trip, not S dependent
// ones (the runtime-count loop compiles to load, wait, add per slab).
// S == 0 is that runtime loop, for counts no planner produces.  Both add
// in the order ((0 + s0) + s1) + ..., so every count gives the same bits
// on either path.  Hosts pick S with SLAB_DISPATCH.
constexpr int MAX_SLABS = 8;

template <int S>
__device__ __forceinline__ void load_slabs(const float* __restrict__ Yf,
                                           int64_t n, int64_t off,
                                           float (&s)[S > 0 ? S : 1]) {
#pragma unroll
    for (int k = 0; k < S; ++k) s[k] = Yf[k * n + off];
}

template <int S>
__device__ __forceinline__ float add_slabs(const float (&s)[S > 0 ? S : 1]) {
    float v = 0.f;
#pragma unroll
    for (int k = 0; k < S; ++k) v += s[k];
    return v;
}

template <int S>
__device__ __forceinline__ float sum_slabs(const float* __restrict__ Yf,
                                           int64_t n, int64_t off,
                                           int splitk) {
    if constexpr (S > 0) {
        float s[S];
        load_slabs<S>(Yf, n, off, s);
        return add_slabs<S>(s);
    } else {
        float v = 0.f;
        for (int k = 0; k < splitk; ++k) v += Yf[k * n + off];
        return v;
    }
}

// CALL(S) with S = splitk for 1..MAX_SLABS, CALL(0) for any other count
#define SLAB_DISPATCH(splitk, CALL) \
    switch (splitk) { \
        case 1: CALL(1); break; case 2: CALL(2); break; \
        case 3: CALL(3); break; case 4: CALL(4); break; \
        case 5: CALL(5); break; case 6: CALL(6); break; \
        case 7: CALL(7); break; case 8: CALL(8); break; \
        default: CALL(0); break; \
    }
