// sat_amd — chunk-table multi-tensor optimizers for gfx950: SGD, Momentum
// (plain / Nesterov) and RMSProp (plain / centered) behind global-norm
// clipping, with the LR staircase, the clip scale and the step counter all
// on the device, so the whole step is hipGraph-capturable (sat_amd/optim.py).
//
// Layout.  The host cuts every tensor into chunks of at most MT_CHUNK
// elements that never cross a tensor boundary:
//   chunks [n_chunks, 3] int32  (tensor, start, count), starts % 4 == 0
//   ptrs   [n_tensors, 6] int64 (p, g, slot0, slot1, slot2, bf16 shadow | 0)
//   vec    [n_tensors]    int32 1 = every pointer of the tensor allows the
//                               16-byte route (decided on the host)
// A block takes whole chunks, so the tensor and its pointers are uniform
// over the block: no per-element search (adam_mt_kernel does one binary
// search per element group).  Blocks stride over the chunks.
//
// Norm without atomics.  sq_norm_chunks writes ONE fp32 partial per block;
// every block of the update kernel sums those <= 2048 partials in a fixed
// order.  No zero-fill launch, and the step is bitwise reproducible.
//
// Slots per kind:  SGD none | Momentum mom | RMSProp ms, mom, (mg) | Adam m, v
#include "common.h"

namespace {

enum { OPT_SGD = 0, OPT_MOM = 1, OPT_NAG = 2, OPT_RMS = 3, OPT_RMSC = 4,
       OPT_ADAM = 5 };

constexpr int MT_BLOCK = 256;
constexpr int MT_MAX_GRID = 2048;   // 256 CUs x 8 blocks

typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;

template <int KIND> struct NSlots {
    static constexpr int value =
        KIND == OPT_SGD ? 0 : (KIND <= OPT_NAG ? 1 :
                               (KIND == OPT_RMSC ? 3 : 2));
};

// sum over the 256 threads of a block in a fixed order; every thread gets it
__device__ __forceinline__ float block_sum(float v, float* red) {
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    float s = (red[0] + red[1]) + (red[2] + red[3]);
    __syncthreads();
    return s;
}

__global__ __launch_bounds__(MT_BLOCK) void sq_norm_chunks_kernel(
        const int* __restrict__ chunks, const int64_t* __restrict__ ptrs,
        const int* __restrict__ vec, int n_chunks,
        float* __restrict__ partials) {
    __shared__ float red[4];
    const int tid = threadIdx.x;
    float acc = 0.f;
    for (int c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        const int t = chunks[c * 3 + 0];
        const int start = chunks[c * 3 + 1];
        const int count = chunks[c * 3 + 2];
        const float* g = (const float*)ptrs[(int64_t)t * 6 + 1] + start;
        if (vec[t]) {
            const int n4 = count >> 2;
            for (int i = tid; i < n4; i += MT_BLOCK) {
                floatx4 v = ((const floatx4*)g)[i];
                acc += (v[0] * v[0] + v[1] * v[1])
                     + (v[2] * v[2] + v[3] * v[3]);
            }
            const int j = n4 * 4 + tid;         // <= 3 elements, last chunk
            if (j < count) acc += g[j] * g[j];
        } else {
            for (int i = tid; i < count; i += MT_BLOCK) acc += g[i] * g[i];
        }
    }
    float s = block_sum(acc, red);
    if (tid == 0) partials[blockIdx.x] = s;
}

// Adam reads beta1 from `momentum`, beta2 from `decay`; bc1 / bc2 are its
// bias corrections 1 - beta^step
struct OptHyper {
    float lr, scale, momentum, decay, eps, bc1, bc2;
};

// m = b1 m + (1 - b1) g, v = b2 v + (1 - b2) g g with the first product
// of each sum fused, as adam_mt_kernel has them; g is already scaled.
// adam_mt_kernel (kernels.hip) leaves that choice to the compiler's
// contraction, so the bit equality of the two routes that
// tests/test_adam_chunk_norm_gpu.py asserts holds for the compiler that
// fuses it this way; should another one not, spell the same fmaf calls out
// there.
__device__ __forceinline__ void adam_update(float& p, float g, float& m,
                                            float& v, const OptHyper& h) {
#pragma clang fp contract(off)
    const float mi = fmaf(h.momentum, m, (1.f - h.momentum) * g);
    const float vi = fmaf(h.decay, v, (1.f - h.decay) * g * g);
    m = mi;
    v = vi;
    p -= h.lr * (mi / h.bc1) / (sqrtf(vi / h.bc2) + h.eps);
}

// one element; g is the raw gradient, s[] the slots of KIND
template <int KIND>
__device__ __forceinline__ void opt_update(float& p, float g, float* s,
                                           const OptHyper& h) {
    g *= h.scale;
    if (KIND == OPT_SGD) {
        p -= h.lr * g;
    } else if (KIND == OPT_MOM) {
        s[0] = h.momentum * s[0] + g;
        p -= h.lr * s[0];
    } else if (KIND == OPT_NAG) {
        s[0] = h.momentum * s[0] + g;
        p -= h.lr * (g + h.momentum * s[0]);
    } else if (KIND == OPT_ADAM) {
        // the expressions of adam_mt_kernel (kernels.hip) with the FMAs
        // it compiles to spelled out (contraction is off in adam_update):
        // left to the compiler, this kernel fused the other product
        adam_update(p, g, s[0], s[1], h);
    } else {
        // TF RMSProp: epsilon inside the sqrt, var -= mom
        s[0] = h.decay * s[0] + (1.f - h.decay) * g * g;
        float den = s[0];
        if (KIND == OPT_RMSC) {
            s[2] = h.decay * s[2] + (1.f - h.decay) * g;
            den -= s[2] * s[2];
        }
        s[1] = h.momentum * s[1] + h.lr * g / sqrtf(den + h.eps);
        p -= s[1];
    }
}

// VEC = 0: no tensor of the table takes the 16-byte route (host-known), the
// route is compiled out.  8 waves per SIMD (<= 64 VGPRs) keep all 2048
// blocks resident: centered RMSProp took 70 without the bound.
template <int KIND, int VEC>
__global__ __launch_bounds__(MT_BLOCK, 8) void opt_mt_kernel(
        const int* __restrict__ chunks, const int64_t* __restrict__ ptrs,
        const int* __restrict__ vec, int n_chunks,
        const float* __restrict__ partials, int n_parts,
        const float* __restrict__ step_dev, float lr0, float decay_factor,
        float steps_per_decay, float momentum, float decay, float eps,
        float clip, int zero_g) {
    constexpr int NS = NSlots<KIND>::value;
    __shared__ float red[4];
    const int tid = threadIdx.x;

    OptHyper h;
    h.momentum = momentum;
    h.decay = decay;
    h.eps = eps;
    const float step = *step_dev;
    h.lr = lr0;
    if (decay_factor < 1.f)
        h.lr = lr0 * powf(decay_factor, floorf(step / steps_per_decay));
    h.bc1 = h.bc2 = 1.f;
    if (KIND == OPT_ADAM) {
        h.bc1 = 1.f - powf(momentum, step);
        h.bc2 = 1.f - powf(decay, step);
    }
    h.scale = 1.f;
    if (clip > 0.f) {
        // the same fixed-order sum in every block: one scale for all
        float a = 0.f;
        for (int i = tid; i < n_parts; i += MT_BLOCK) a += partials[i];
        const float norm = sqrtf(block_sum(a, red));
        if (norm > clip) h.scale = clip / norm;
    }

    for (int c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        const int t = chunks[c * 3 + 0];
        const int start = chunks[c * 3 + 1];
        const int count = chunks[c * 3 + 2];
        const int64_t* row = ptrs + (int64_t)t * 6;
        float* p = (float*)row[0] + start;
        float* g = (float*)row[1] + start;
        float* sl[3] = {nullptr, nullptr, nullptr};
#pragma unroll
        for (int k = 0; k < NS; ++k) sl[k] = (float*)row[2 + k] + start;
        bf16* sh = (bf16*)row[5];
        if (sh != nullptr) sh += start;

        int done = 0;                      // elements the 16-byte route took
        if (VEC && vec[t]) {
            const int n4 = count >> 2;
            for (int i = tid; i < n4; i += MT_BLOCK) {
                // every load of the iteration before the first use
                floatx4 g4 = ((floatx4*)g)[i];
                floatx4 p4 = ((floatx4*)p)[i];
                floatx4 s4[3];
#pragma unroll
                for (int k = 0; k < NS; ++k) s4[k] = ((floatx4*)sl[k])[i];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    float pe = p4[e], se[3] = {0.f, 0.f, 0.f};
#pragma unroll
                    for (int k = 0; k < NS; ++k) se[k] = s4[k][e];
                    opt_update<KIND>(pe, g4[e], se, h);
                    p4[e] = pe;
#pragma unroll
                    for (int k = 0; k < NS; ++k) s4[k][e] = se[k];
                }
                ((floatx4*)p)[i] = p4;
#pragma unroll
                for (int k = 0; k < NS; ++k) ((floatx4*)sl[k])[i] = s4[k];
                if (sh != nullptr) {
                    bf16x4 b;
#pragma unroll
                    for (int e = 0; e < 4; ++e) b[e] = f2bf(p4[e]);
                    ((bf16x4*)sh)[i] = b;
                }
                if (zero_g) ((floatx4*)g)[i] = floatx4{0.f, 0.f, 0.f, 0.f};
            }
            done = n4 * 4;                 // <= 3 left, a tensor's last chunk
        }
        for (int i = done + tid; i < count; i += MT_BLOCK) {
            float ge = g[i], pe = p[i], se[3] = {0.f, 0.f, 0.f};
#pragma unroll
            for (int k = 0; k < NS; ++k) se[k] = sl[k][i];
            opt_update<KIND>(pe, ge, se, h);
            p[i] = pe;
#pragma unroll
            for (int k = 0; k < NS; ++k) sl[k][i] = se[k];
            if (sh != nullptr) sh[i] = f2bf(pe);
            if (zero_g) g[i] = 0.f;
        }
    }
}

struct Tables {
    const int* chunks;
    const int64_t* ptrs;
    const int* vec;
    int n_chunks, grid;
};

Tables check_tables(const at::Tensor& chunks, const at::Tensor& ptrs,
                    const at::Tensor& vec, const at::Tensor& partials) {
    CHECK_GPU(chunks); CHECK_CONTIG(chunks);
    CHECK_GPU(ptrs); CHECK_CONTIG(ptrs);
    CHECK_GPU(vec); CHECK_CONTIG(vec);
    CHECK_GPU(partials); CHECK_CONTIG(partials); CHECK_F32(partials);
    TORCH_CHECK(chunks.scalar_type() == at::kInt && chunks.dim() == 2
                && chunks.size(1) == 3, "chunks must be int32 [n_chunks, 3]");
    TORCH_CHECK(ptrs.scalar_type() == at::kLong && ptrs.dim() == 2
                && ptrs.size(1) == 6, "ptrs must be int64 [n_tensors, 6]");
    TORCH_CHECK(vec.scalar_type() == at::kInt && vec.dim() == 1
                && vec.size(0) == ptrs.size(0),
                "vec must be int32 [n_tensors]");
    TORCH_CHECK(chunks.size(0) < (1LL << 31) / 3, "too many chunks");
    Tables T;
    T.chunks = (const int*)chunks.data_ptr();
    T.ptrs = (const int64_t*)ptrs.data_ptr();
    T.vec = (const int*)vec.data_ptr();
    T.n_chunks = (int)chunks.size(0);
    T.grid = std::min(T.n_chunks, MT_MAX_GRID);
    TORCH_CHECK(partials.numel() >= T.grid,
                "partials needs one float per block (", T.grid, ")");
    return T;
}

}  // namespace

// one partial sum of g^2 per block into partials[0 .. min(n_chunks, 2048))
void sq_norm_chunks(at::Tensor chunks, at::Tensor ptrs, at::Tensor vec,
                    at::Tensor partials) {
    Tables T = check_tables(chunks, ptrs, vec, partials);
    if (T.n_chunks == 0) return;
    hipStream_t s = at::cuda::getCurrentCUDAStream();
    hipLaunchKernelGGL(sq_norm_chunks_kernel, dim3(T.grid), dim3(MT_BLOCK),
                       0, s, T.chunks, T.ptrs, T.vec, T.n_chunks,
                       (float*)partials.data_ptr());
    HIP_OK(hipGetLastError());
}

// kind: 0 SGD, 1 Momentum, 2 Momentum-Nesterov, 3 RMSProp, 4 RMSProp
// centered, 5 Adam (momentum = beta1, decay = beta2).  any_vec: some
// vec[t] is set (host-known; reading it back here would sync inside a
// graph capture).  With clip > 0, partials holds what sq_norm_chunks wrote
// for the same tables.
void opt_step_mt(at::Tensor chunks, at::Tensor ptrs, at::Tensor vec,
                 bool any_vec, at::Tensor step_dev, double lr0,
                 double decay_factor, double steps_per_decay,
                 double momentum, double decay, double eps, double clip,
                 int64_t kind, bool zero_grads, at::Tensor partials) {
    Tables T = check_tables(chunks, ptrs, vec, partials);
    CHECK_GPU(step_dev); CHECK_F32(step_dev);
    TORCH_CHECK(kind >= OPT_SGD && kind <= OPT_ADAM, "unknown kind ", kind);
    if (T.n_chunks == 0) return;
    hipStream_t s = at::cuda::getCurrentCUDAStream();
#define OPT_LAUNCH(K, V) \
    hipLaunchKernelGGL((opt_mt_kernel<K, V>), dim3(T.grid), dim3(MT_BLOCK), \
                       0, s, T.chunks, T.ptrs, T.vec, T.n_chunks, \
                       (const float*)partials.data_ptr(), T.grid, \
                       (const float*)step_dev.data_ptr(), (float)lr0, \
                       (float)decay_factor, (float)steps_per_decay, \
                       (float)momentum, (float)decay, (float)eps, \
                       (float)clip, zero_grads ? 1 : 0)
#define OPT_KIND(K) \
    case K: if (any_vec) OPT_LAUNCH(K, 1); else OPT_LAUNCH(K, 0); break
    switch (kind) {
        OPT_KIND(OPT_SGD);
        OPT_KIND(OPT_MOM);
        OPT_KIND(OPT_NAG);
        OPT_KIND(OPT_RMS);
        OPT_KIND(OPT_RMSC);
        OPT_KIND(OPT_ADAM);
    }
#undef OPT_KIND
#undef OPT_LAUNCH
    HIP_OK(hipGetLastError());
}
