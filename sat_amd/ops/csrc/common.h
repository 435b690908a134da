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
// both sides must derive masks identically.
__device__ __forceinline__ void drop_scale8(uint32_t seed, int salt,
                                            uint32_t idx8, float p,
                                            float* sc) {
    if (p <= 0.f) {
#pragma unroll
        for (int e = 0; e < 8; ++e) sc[e] = 1.f;
        return;
    }
    uint32_t pq = (uint32_t)(p * 256.0f);
    float inv = 1.0f / (1.0f - p);
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

// split-K combine: element `off` summed over `splitk` fp32 slabs of n
__device__ __forceinline__ float sum_slabs(const float* __restrict__ Yf,
                                           int64_t n, int64_t off,
                                           int splitk) {
    float v = 0.f;
    for (int k = 0; k < splitk; ++k) v += Yf[k * n + off];
    return v;
}
