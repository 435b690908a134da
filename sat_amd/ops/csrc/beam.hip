// Beam-search inference kernels (sat_amd/beam.py, docs/KERNELS.md):
//
//   softmax_topk   the K largest softmax probabilities of each logits row,
//                  without writing the [R,V] probabilities anywhere
//   beam_advance   everything beam search does between two decoder steps,
//                  plus the next step's inputs, in one launch
//   beam_attend    1-layer attention of one decoder step for all beams:
//                  logits, softmax over locations and the pooled context,
//                  each image's contexts read once for its W beams
//
// The first two order their selections by (value descending, position
// ascending): random bf16 logits tie often, and torch.topk promises no
// order among ties, so the tie rule is part of the contract here.
#include "common.h"

#include <climits>

namespace {

constexpr int TOPK_THREADS = 256;
constexpr int TOPK_WAVES = TOPK_THREADS / 64;
constexpr int MAX_TOPK = 9;
constexpr int MAX_BEAM = 8;
constexpr int MAX_CAND = MAX_BEAM * MAX_TOPK;

// (av, ai) ranks strictly before (bv, bi)
__device__ __forceinline__ bool before(float av, int ai, float bv, int bi) {
    return av > bv || (av == bv && ai < bi);
}

// NaN logits rank as -inf so that every one of the V entries has a rank
// and the K results are always real indices below V
__device__ __forceinline__ float clean(bf16 x) {
    float v = bf2f(x);
    return v != v ? -INFINITY : v;
}

// sorted insert into a thread's K best (all indices static: registers)
template <int K>
__device__ __forceinline__ void topk_insert(float (&tv)[K], int (&ti)[K],
                                            float v, int i) {
    if (!before(v, i, tv[K - 1], ti[K - 1])) return;
    tv[K - 1] = v;
    ti[K - 1] = i;
#pragma unroll
    for (int k = K - 1; k > 0; --k) {
        if (before(tv[k], ti[k], tv[k - 1], ti[k - 1])) {
            float fv = tv[k]; tv[k] = tv[k - 1]; tv[k - 1] = fv;
            int fi = ti[k]; ti[k] = ti[k - 1]; ti[k - 1] = fi;
        }
    }
}

// A row of V bf16 starts 16-byte aligned only when its offset is a
// multiple of 8 elements: `head` scalar elements up to the first aligned
// address, then bf16x8 loads, then fewer than 8 scalar elements.
struct RowSplit { int head, nvec, tail0; };

__device__ __forceinline__ RowSplit row_split(const bf16* row, int V) {
    RowSplit s;
    s.head = (int)(((16u - (unsigned)((uintptr_t)row & 15u)) & 15u) >> 1);
    if (s.head > V) s.head = V;
    s.nvec = (V - s.head) / 8;
    s.tail0 = s.head + s.nvec * 8;
    return s;
}

// One block per row.  Pass 1: every thread keeps the K best of its share
// of the row; K rounds of a block-wide arg-best over the threads' heads
// merge them (the winner pops its head).  Pass 2: sum of exp(x - max) in
// fp32, per thread then wave tree then the waves in fixed order.
template <int K>
__global__ __launch_bounds__(TOPK_THREADS)
void softmax_topk_kernel(const bf16* __restrict__ logits,
                         float* __restrict__ p_out,
                         int64_t* __restrict__ idx_out, int V) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const bf16* row = logits + (int64_t)blockIdx.x * V;
    const RowSplit sp = row_split(row, V);

    float tv[K];
    int ti[K];
#pragma unroll
    for (int k = 0; k < K; ++k) { tv[k] = -INFINITY; ti[k] = INT_MAX; }

    if (tid < sp.head) topk_insert<K>(tv, ti, clean(row[tid]), tid);
    for (int j = tid; j < sp.nvec; j += TOPK_THREADS) {
        const int e0 = sp.head + j * 8;
        bf16x8 x = *(const bf16x8*)(row + e0);
#pragma unroll
        for (int e = 0; e < 8; ++e)
            topk_insert<K>(tv, ti, clean(x[e]), e0 + e);
    }
    if (sp.tail0 + tid < V)
        topk_insert<K>(tv, ti, clean(row[sp.tail0 + tid]), sp.tail0 + tid);

    // round k writes buffer k & 1; a thread can only reach round k + 2
    // after every thread has passed the barrier of round k + 1, i.e. has
    // finished reading round k's buffer
    __shared__ float s_v[2][TOPK_WAVES];
    __shared__ int s_i[2][TOPK_WAVES];
    float wv[K];
    int wi[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
        float v = tv[0];
        int i = ti[0];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            float ov = __shfl_xor(v, off, 64);
            int oi = __shfl_xor(i, off, 64);
            if (before(ov, oi, v, i)) { v = ov; i = oi; }
        }
        if (lane == 0) { s_v[k & 1][wave] = v; s_i[k & 1][wave] = i; }
        __syncthreads();
        v = s_v[k & 1][0];
        i = s_i[k & 1][0];
#pragma unroll
        for (int w = 1; w < TOPK_WAVES; ++w) {
            float ov = s_v[k & 1][w];
            int oi = s_i[k & 1][w];
            if (before(ov, oi, v, i)) { v = ov; i = oi; }
        }
        wv[k] = v;
        wi[k] = i;
        if (ti[0] == i) {       // indices are unique: one thread pops
#pragma unroll
            for (int j = 0; j + 1 < K; ++j) {
                tv[j] = tv[j + 1];
                ti[j] = ti[j + 1];
            }
            tv[K - 1] = -INFINITY;
            ti[K - 1] = INT_MAX;
        }
    }

    const float mx = wv[0];
    float sum = 0.f;
    if (tid < sp.head) sum += expf(clean(row[tid]) - mx);
    for (int j = tid; j < sp.nvec; j += TOPK_THREADS) {
        bf16x8 x = *(const bf16x8*)(row + sp.head + j * 8);
#pragma unroll
        for (int e = 0; e < 8; ++e) sum += expf(clean(x[e]) - mx);
    }
    if (sp.tail0 + tid < V) sum += expf(clean(row[sp.tail0 + tid]) - mx);
    sum = wave_sum(sum);
    __shared__ float s_sum[TOPK_WAVES];
    if (lane == 0) s_sum[wave] = sum;
    __syncthreads();
    if (tid == 0) {
        float tot = 0.f;
#pragma unroll
        for (int w = 0; w < TOPK_WAVES; ++w) tot += s_sum[w];
#pragma unroll
        for (int k = 0; k < K; ++k) {
            p_out[(int64_t)blockIdx.x * K + k] = expf(wv[k] - mx) / tot;
            idx_out[(int64_t)blockIdx.x * K + k] = wi[k];
        }
    }
}

// ---------------------------------------------------------------------
// beam_advance: one block per image.
//
// Candidates c = parent * K + k score scores[parent] * p[parent, k] in
// fp64.  Period candidates merge into the completed set (best W of
// [completed..., candidates...]); the best W others become the live beams
// (dead slots carry score 0).  Both selections rank by counting: the rank
// of an entry is the number of entries with a larger score, or an equal
// score and a smaller position, so rank r < W is slot r and no sort runs.
// The selected parents' LSTM rows and the selected words' embedding rows
// are then gathered into the NEXT step's buffers: the state it reads and
// the state it writes are different buffers, an in-place reorder would
// race between slots.
// ---------------------------------------------------------------------

struct BeamState {
    double* scores;        // [B,W]
    int64_t* seqs;         // [B,W,T]
    int64_t* lens;         // [B,W]
    double* c_scores;      // [B,W]  completed set
    int64_t* c_seqs;       // [B,W,T]
    int64_t* c_lens;       // [B,W]
};

__global__ __launch_bounds__(256)
void beam_advance_kernel(BeamState in, BeamState out,
                         const float* __restrict__ top_p,     // [B*W,K]
                         const int64_t* __restrict__ top_w,   // [B*W,K]
                         const bf16* __restrict__ mem_new,    // [B*W,H]
                         const bf16* __restrict__ h_new,      // [B*W,H]
                         const bf16* __restrict__ table,      // [V,E]
                         bf16* __restrict__ mem_next,         // [B*W,H]
                         bf16* __restrict__ xh_next,          // [B*W,D+E+H]
                         bf16* __restrict__ exp_next,         // [B*W,H+D+E]
                         int64_t* __restrict__ last_word,     // [B*W]
                         int64_t* __restrict__ parent_out,    // [B*W]
                         int W, int K, int T, int H, int D, int E, int V,
                         int64_t period) {
    const int b = blockIdx.x, tid = threadIdx.x;
    const int WK = W * K;
    const int row0 = b * W;

    __shared__ double s_part[MAX_CAND];              // live ranking key
    __shared__ double s_merged[MAX_BEAM + MAX_CAND]; // completed ranking key
    __shared__ int64_t s_word[MAX_CAND];
    __shared__ int s_sel[MAX_BEAM];
    __shared__ int s_keep[MAX_BEAM];

    if (tid < WK) {
        const int parent = tid / K;
        double s = in.scores[row0 + parent]
            * (double)top_p[(int64_t)row0 * K + tid];
        if (s != s) s = 0.0;
        const int64_t w = top_w[(int64_t)row0 * K + tid];
        const bool is_period = (w == period);
        s_word[tid] = w;
        s_part[tid] = is_period ? -INFINITY : s;
        s_merged[W + tid] = is_period ? s : 0.0;
    }
    if (tid < W) {
        const double cs = in.c_scores[row0 + tid];
        s_merged[tid] = cs != cs ? 0.0 : cs;
        // without NaN the ranks below are a permutation and fill every
        // slot; the zeros only keep a slot's index in range regardless
        s_sel[tid] = 0;
        s_keep[tid] = 0;
    }
    __syncthreads();

    if (tid < W + WK) {
        const double m = s_merged[tid];
        int rank = 0;
        for (int i = 0; i < W + WK; ++i) {
            const double o = s_merged[i];
            rank += (o > m || (o == m && i < tid)) ? 1 : 0;
        }
        if (rank < W) s_keep[rank] = tid;
    }
    if (tid < WK) {
        const double m = s_part[tid];
        int rank = 0;
        for (int i = 0; i < WK; ++i) {
            const double o = s_part[i];
            rank += (o > m || (o == m && i < tid)) ? 1 : 0;
        }
        if (rank < W) s_sel[rank] = tid;
    }
    __syncthreads();

    // ---- scalar state of the W live and W completed slots ----
    if (tid < W) {
        const int c = s_sel[tid];
        const int parent = c / K;
        const double s = s_part[c];
        out.scores[row0 + tid] = s > 0.0 ? s : 0.0;
        int64_t len = in.lens[row0 + parent] + 1;
        out.lens[row0 + tid] = len < T ? len : T;
        last_word[row0 + tid] = s_word[c];
        parent_out[row0 + tid] = parent;

        const int j = s_keep[tid];
        if (j < W) {
            out.c_scores[row0 + tid] = in.c_scores[row0 + j];
            out.c_lens[row0 + tid] = in.c_lens[row0 + j];
        } else {
            const int cp = (j - W) / K;
            out.c_scores[row0 + tid] = s_merged[j];
            int64_t cl = in.lens[row0 + cp] + 1;
            out.c_lens[row0 + tid] = cl < T ? cl : T;
        }
    }

    // ---- sequences: parent's row with the word written at its length ----
    for (int idx = tid; idx < W * T; idx += blockDim.x) {
        const int w = idx / T, t = idx - w * T;
        {
            const int c = s_sel[w];
            const int parent = c / K;
            int64_t pos = in.lens[row0 + parent];
            if (pos > T - 1) pos = T - 1;
            out.seqs[(int64_t)(row0 + w) * T + t] = (t == pos)
                ? s_word[c] : in.seqs[(int64_t)(row0 + parent) * T + t];
        }
        {
            const int j = s_keep[w];
            int64_t val;
            if (j < W) {
                val = in.c_seqs[(int64_t)(row0 + j) * T + t];
            } else {
                const int c = j - W;
                const int parent = c / K;
                int64_t pos = in.lens[row0 + parent];
                if (pos > T - 1) pos = T - 1;
                val = (t == pos)
                    ? s_word[c] : in.seqs[(int64_t)(row0 + parent) * T + t];
            }
            out.c_seqs[(int64_t)(row0 + w) * T + t] = val;
        }
    }

    // ---- row gathers, 16 bytes per thread (H, D, E multiples of 8) ----
    const int H8 = H / 8, E8 = E / 8;
    const int nv = 2 * H8 + E8;
    const int XS = D + E + H;
    for (int idx = tid; idx < W * nv; idx += blockDim.x) {
        const int w = idx / nv, r = idx - w * nv;
        const int c = s_sel[w];
        const int64_t dst = row0 + w, src = row0 + c / K;
        if (r < H8) {
            *(uint4*)(mem_next + dst * H + r * 8) =
                *(const uint4*)(mem_new + src * H + r * 8);
        } else if (r < 2 * H8) {
            const int q = r - H8;
            *(uint4*)(xh_next + dst * XS + D + E + q * 8) =
                *(const uint4*)(h_new + src * H + q * 8);
        } else {
            const int q = r - 2 * H8;
            int64_t word = s_word[c];
            // ids from softmax_topk are below V; anything else reads row 0
            if (word < 0 || word >= V) word = 0;
            const uint4 v = *(const uint4*)(table + word * E + q * 8);
            *(uint4*)(xh_next + dst * XS + D + q * 8) = v;
            if (exp_next != nullptr)
                *(uint4*)(exp_next + dst * XS + H + D + q * 8) = v;
        }
    }
}

BeamState beam_state(const std::vector<at::Tensor>& st, int64_t B,
                     int64_t W, int64_t T, const char* name) {
    TORCH_CHECK(st.size() == 6, name,
                ": (scores, seqs, lens, c_scores, c_seqs, c_lens)");
    for (int i = 0; i < 6; ++i) {
        const at::Tensor& t = st[i];
        CHECK_GPU(t); CHECK_CONTIG(t);
        const bool is_score = (i % 3 == 0), is_seq = (i % 3 == 1);
        TORCH_CHECK(t.scalar_type() == (is_score ? at::kDouble : at::kLong),
                    name, ": scores are fp64, seqs / lens int64");
        TORCH_CHECK(t.dim() == (is_seq ? 3 : 2) && t.size(0) == B
                    && t.size(1) == W && (!is_seq || t.size(2) == T),
                    name, ": tensor ", i, " has the wrong shape");
    }
    return {(double*)st[0].data_ptr(), (int64_t*)st[1].data_ptr(),
            (int64_t*)st[2].data_ptr(), (double*)st[3].data_ptr(),
            (int64_t*)st[4].data_ptr(), (int64_t*)st[5].data_ptr()};
}

void check_rows(const at::Tensor& t, int64_t rows, int64_t cols,
                const char* name) {
    CHECK_GPU(t); CHECK_CONTIG(t); CHECK_BF16(t);
    TORCH_CHECK(t.dim() == 2 && t.size(0) == rows && t.size(1) == cols,
                name, ": expected [", rows, ",", cols, "]");
    TORCH_CHECK(((uintptr_t)t.data_ptr() & 15) == 0, name,
                " must be 16-byte aligned");
}

// ---------------------------------------------------------------------
// beam_attend: grid (B, S), block (b, s) serves the W beams of image b and
// the s-th slice of the D/8 column vectors.  Row n = b*W + w.
//
//   logit[n,l]  = l1[b,l] + sum_k h[n,k] * wb[l,k]     fp32
//   alpha[n,:]  = softmax_l(logit[n,:])                fp32, max-subtracted
//   pooled[n,d] = sum_l alpha[n,l] * ctx[b,l,d]        fp32, one rounding
//
// Phase 1 stages the image's W rows of h in LDS.  Phase 2: 8 lanes per
// location (8 locations per wave, 32 per block and pass) walk wb[l,:] in
// 16-byte loads against the W staged rows with the 2-element bf16 dot
// instruction (fp32 accumulator) and meet in a 3-level xor tree.
// Phase 3: one wave per row does the softmax in LDS.  Phase 4: thread
// (tl, tc) keeps W x 8 fp32 accumulators for column vector tc over the
// locations tl, tl + LG, ...: a context vector is loaded once and used by
// all W beams.  The LG partial sums meet through LDS in index order.
// Every block repeats phases 1-3 (cheap next to phase 4 at small B·S, and
// what lets S > 1 spread one image over several CUs); block s == 0 writes
// alpha.  No atomics and no order that depends on timing: two launches on
// the same inputs give the same bits.
//
// The kernel reads columns [D+E, D+E+H) of xh (h, where beam_advance and
// the engine's setup put it) and writes columns [0, D) of the same rows.
// The two ranges are disjoint and no block reads what another writes, so
// unlike beam_advance, whose slots read their PARENTS' rows and would race
// an in-place reorder, it needs no second buffer.
// ---------------------------------------------------------------------

constexpr int ATT_THREADS = 256;
constexpr int ATT_WAVES = ATT_THREADS / 64;
constexpr int ATT_MAX_L = 1024;     // W*L fp32 logits: 32 KiB at W = 8
constexpr int ATT_MAX_H = 2048;     // W*H bf16 staged h: 32 KiB at W = 8
constexpr int ATT_GRID = 256;       // one block per CU
constexpr int ATT_UNROLL = 8;       // 16-byte loads in flight per lane
constexpr int ATT_MIN_VEC = 16;     // profiles/beam_attend_perf_log.md

// beams whose partial sums cross the waves through LDS in one pass
template <int W> struct AttChunk { static constexpr int n = W < 4 ? W : 4; };

// bytes of the region shared by the staged h (phases 1-2) and the
// partial sums (phase 4)
static inline size_t att_union_bytes(int W, int H) {
    const size_t h_bytes = (size_t)W * H * sizeof(bf16);
    const size_t part = (size_t)ATT_THREADS * (W < 4 ? W : 4) * 8
        * sizeof(float);
    return h_bytes > part ? h_bytes : part;
}

// S, the blocks per image: the largest power of two that keeps B*S within
// ATT_GRID blocks and leaves a block at least ATT_MIN_VEC column vectors
static inline int att_split(int B, int nvec) {
    int S = 1;
    while (B * S * 2 <= ATT_GRID && nvec / (S * 2) >= ATT_MIN_VEC) S *= 2;
    return S;
}

__device__ __forceinline__ float xor_sum(float v, int from) {
    for (int off = from; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

__device__ __forceinline__ int cdiv_dev(int a, int b) {
    return a > 0 ? (a + b - 1) / b : 0;
}

// acc + sum of 8 bf16 products, fp32: four 2-element bf16 dot instructions
__device__ __forceinline__ float dot8(bf16x8 a, bf16x8 b, float acc) {
    acc = __builtin_amdgcn_fdot2_f32_bf16(
        __builtin_shufflevector(a, a, 0, 1),
        __builtin_shufflevector(b, b, 0, 1), acc, false);
    acc = __builtin_amdgcn_fdot2_f32_bf16(
        __builtin_shufflevector(a, a, 2, 3),
        __builtin_shufflevector(b, b, 2, 3), acc, false);
    acc = __builtin_amdgcn_fdot2_f32_bf16(
        __builtin_shufflevector(a, a, 4, 5),
        __builtin_shufflevector(b, b, 4, 5), acc, false);
    return __builtin_amdgcn_fdot2_f32_bf16(
        __builtin_shufflevector(a, a, 6, 7),
        __builtin_shufflevector(b, b, 6, 7), acc, false);
}

// pass `it` of a wave's logits phase: location l = l_first + p * 32 and
// the vectors (c * ATT_UNROLL + u) * 8 + sub of wb[l,:], with
// (p, c) = divmod(it, nchunk); what lies past L or H loads as zero
__device__ __forceinline__ void att_load_wb(bf16x8 (&buf)[ATT_UNROLL],
                                            const bf16* __restrict__ wb,
                                            int it, int nchunk, int l_first,
                                            int sub, int L, int H) {
    const int p = it / nchunk, c = it - p * nchunk;
    const int l = l_first + p * ATT_WAVES * 8;
    const bf16* wr = wb + (int64_t)l * H;
#pragma unroll
    for (int u = 0; u < ATT_UNROLL; ++u) {
        const int jv = (c * ATT_UNROLL + u) * 8 + sub;
        bf16x8 v = {};
        if (l < L && jv < H / 8) v = *(const bf16x8*)(wr + jv * 8);
        buf[u] = v;
    }
}

template <int W>
__global__ __launch_bounds__(ATT_THREADS)
void beam_attend_kernel(const bf16* __restrict__ ctx,     // [B,L,D]
                        const float* __restrict__ l1,     // [B,L]
                        const bf16* __restrict__ wb,      // [L,H]
                        bf16* xh,                         // [B*W,D+E+H]
                        bf16* __restrict__ pool,          // [B*W,D]
                        float* __restrict__ alpha,        // [B*W,L] or null
                        int L, int D, int E, int H,
                        int cv,        // column vectors per block
                        int CW,        // power of two, min(cv, 256) <= CW
                        int union_bytes) {
    constexpr int WC = AttChunk<W>::n;
    const int b = blockIdx.x, tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int nvec = D / 8, v0 = blockIdx.y * cv;
    const int NC = (nvec - v0 < cv) ? nvec - v0 : cv;
    if (NC <= 0) return;                // whole block, before any barrier
    const int XS = D + E + H;
    const int64_t row0 = (int64_t)b * W;

    extern __shared__ __attribute__((aligned(16))) unsigned char att_lds[];
    bf16* s_h = (bf16*)att_lds;                         // [W,H]
    float* s_part = (float*)att_lds;                    // [LG,WC,CW*8]
    float* s_a = (float*)(att_lds + union_bytes);       // [W,L]

    // ---- 1. h rows of this image ----
    const int H8 = H / 8;
    for (int idx = tid; idx < W * H8; idx += ATT_THREADS) {
        const int w = idx / H8, q = idx - w * H8;
        *(uint4*)(s_h + w * H + q * 8) =
            *(const uint4*)(xh + (row0 + w) * XS + D + E + q * 8);
    }
    __syncthreads();

    // ---- 2. logits: 8 lanes per location ----
    // A pass is 8 locations per wave and ATT_UNROLL*8 vectors of H per
    // location: its loads are issued together, and the next pass's before
    // this pass's arithmetic, so a wave waits for memory once per pass and
    // not once per load.
    {
        const int sub = lane & 7, grp = lane >> 3;
        const int nchunk = cdiv_dev(H8, ATT_UNROLL * 8);
        const int npass = cdiv_dev(L - wave * 8, ATT_WAVES * 8) * nchunk;
        bf16x8 cur[ATT_UNROLL], nxt[ATT_UNROLL] = {};
        att_load_wb(cur, wb, 0, nchunk, wave * 8 + grp, sub, L, H);
        float acc[W];
        for (int it = 0; it < npass; ++it) {
            if (it + 1 < npass)
                att_load_wb(nxt, wb, it + 1, nchunk, wave * 8 + grp, sub,
                            L, H);
            const int p = it / nchunk, c = it - p * nchunk;
            if (c == 0) {
#pragma unroll
                for (int w = 0; w < W; ++w) acc[w] = 0.f;
            }
#pragma unroll
            for (int u = 0; u < ATT_UNROLL; ++u) {
                const int jv = (c * ATT_UNROLL + u) * 8 + sub;
                if (jv < H8) {
#pragma unroll
                    for (int w = 0; w < W; ++w)
                        acc[w] = dot8(*(const bf16x8*)(s_h + w * H + jv * 8),
                                      cur[u], acc[w]);
                }
            }
            if (c == nchunk - 1) {          // wave-uniform
                const int l = wave * 8 + p * ATT_WAVES * 8 + grp;
#pragma unroll
                for (int w = 0; w < W; ++w) acc[w] = xor_sum(acc[w], 4);
                if (l < L && sub == 0) {
                    const float base = l1[(int64_t)b * L + l];
#pragma unroll
                    for (int w = 0; w < W; ++w)
                        s_a[w * L + l] = base + acc[w];
                }
            }
#pragma unroll
            for (int u = 0; u < ATT_UNROLL; ++u) cur[u] = nxt[u];
        }
    }
    __syncthreads();

    // ---- 3. softmax, one wave per row (xor trees: every lane ends with
    // the same bits) ----
    for (int w = wave; w < W; w += ATT_WAVES) {
        float* row = s_a + w * L;
        float m = -INFINITY;
        for (int l = lane; l < L; l += 64) m = fmaxf(m, row[l]);
        for (int off = 32; off > 0; off >>= 1)
            m = fmaxf(m, __shfl_xor(m, off, 64));
        float s = 0.f;
        for (int l = lane; l < L; l += 64) {
            const float e = __expf(row[l] - m);
            row[l] = e;
            s += e;
        }
        s = xor_sum(s, 32);
        const float inv = 1.0f / s;
        for (int l = lane; l < L; l += 64) {
            const float a = row[l] * inv;
            row[l] = a;
            if (alpha != nullptr && blockIdx.y == 0)
                alpha[(row0 + w) * L + l] = a;
        }
    }
    __syncthreads();    // s_a complete; s_h is dead from here (s_part)

    // ---- 4. pooled columns [v0, v0 + NC) ----
    const int LG = ATT_THREADS / CW;
    const int tc = tid & (CW - 1), tl = tid / CW;
    const bf16* cb = ctx + (int64_t)b * L * D;
    for (int c0 = 0; c0 < NC; c0 += CW) {       // once unless cv > 256
        const int c = c0 + tc;
        float acc[W][8];
#pragma unroll
        for (int w = 0; w < W; ++w)
#pragma unroll
            for (int e = 0; e < 8; ++e) acc[w][e] = 0.f;
        if (c < NC) {
            const bf16* cp = cb + (int64_t)(v0 + c) * 8;
#pragma unroll 4
            for (int l = tl; l < L; l += LG) {
                const bf16x8 x = *(const bf16x8*)(cp + (int64_t)l * D);
#pragma unroll
                for (int w = 0; w < W; ++w) {
                    const float a = s_a[w * L + l];
#pragma unroll
                    for (int e = 0; e < 8; ++e)
                        acc[w][e] += a * bf2f(x[e]);
                }
            }
        }
#pragma unroll
        for (int w0 = 0; w0 < W; w0 += WC) {
            __syncthreads();            // s_part (or s_h) no longer read
#pragma unroll
            for (int wi = 0; wi < WC; ++wi) {
                if (w0 + wi < W) {
                    float* dst = s_part + ((tl * WC + wi) * CW + tc) * 8;
                    *(floatx4*)dst = floatx4{acc[w0 + wi][0],
                                             acc[w0 + wi][1],
                                             acc[w0 + wi][2],
                                             acc[w0 + wi][3]};
                    *(floatx4*)(dst + 4) = floatx4{acc[w0 + wi][4],
                                                   acc[w0 + wi][5],
                                                   acc[w0 + wi][6],
                                                   acc[w0 + wi][7]};
                }
            }
            __syncthreads();
            // (beam, column vector) per thread: the LG partial sums in
            // index order, one rounding, the same 16 bytes to pool and xh
            for (int idx = tid; idx < WC * CW; idx += ATT_THREADS) {
                const int wi = idx / CW, ci = idx - wi * CW;
                const int w = w0 + wi;
                if (w >= W || c0 + ci >= NC) continue;
                float s[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) s[e] = 0.f;
                for (int g = 0; g < LG; ++g) {
                    const float* src = s_part + ((g * WC + wi) * CW + ci) * 8;
                    const floatx4 lo = *(const floatx4*)src;
                    const floatx4 hi = *(const floatx4*)(src + 4);
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        s[e] += lo[e];
                        s[4 + e] += hi[e];
                    }
                }
                bf16x8 o;
#pragma unroll
                for (int e = 0; e < 8; ++e) o[e] = f2bf(s[e]);
                const int64_t col = (int64_t)(v0 + c0 + ci) * 8;
                *(bf16x8*)(pool + (row0 + w) * D + col) = o;
                *(bf16x8*)(xh + (row0 + w) * XS + col) = o;
            }
        }
    }
}

}  // namespace

// p [R,K] fp32 and idx [R,K] int64 are written in place
void softmax_topk(at::Tensor logits, int64_t K, at::Tensor p,
                  at::Tensor idx) {
    CHECK_GPU(logits); CHECK_CONTIG(logits); CHECK_BF16(logits);
    CHECK_GPU(p); CHECK_CONTIG(p); CHECK_F32(p);
    CHECK_GPU(idx); CHECK_CONTIG(idx);
    TORCH_CHECK(idx.scalar_type() == at::kLong, "idx must be int64");
    TORCH_CHECK(logits.dim() == 2, "logits must be [R,V]");
    const int64_t R = logits.size(0), V = logits.size(1);
    TORCH_CHECK(K >= 1 && K <= MAX_TOPK, "softmax_topk: 1 <= K <= 9");
    TORCH_CHECK(V >= K && V < INT_MAX, "softmax_topk: K <= V < 2^31");
    TORCH_CHECK(R < INT_MAX, "softmax_topk: too many rows");
    TORCH_CHECK(p.dim() == 2 && p.size(0) == R && p.size(1) == K
                && idx.dim() == 2 && idx.size(0) == R && idx.size(1) == K,
                "softmax_topk: p and idx must be [R,K]");
    if (R == 0) return;
    hipStream_t stream = at::cuda::getCurrentCUDAStream();
#define LAUNCH_TOPK(KK) \
    case KK: \
        hipLaunchKernelGGL(softmax_topk_kernel<KK>, dim3((unsigned)R), \
                           dim3(TOPK_THREADS), 0, stream, \
                           (const bf16*)logits.data_ptr(), \
                           (float*)p.data_ptr(), \
                           (int64_t*)idx.data_ptr(), (int)V); \
        break;
    switch (K) {
        LAUNCH_TOPK(1) LAUNCH_TOPK(2) LAUNCH_TOPK(3) LAUNCH_TOPK(4)
        LAUNCH_TOPK(5) LAUNCH_TOPK(6) LAUNCH_TOPK(7) LAUNCH_TOPK(8)
        LAUNCH_TOPK(9)
    }
#undef LAUNCH_TOPK
    HIP_OK(hipGetLastError());
}

// state_in -> state_out (distinct tensors), plus the next step's inputs;
// exp_next may be empty (no decode-input row to fill)
void beam_advance(std::vector<at::Tensor> state_in,
                  std::vector<at::Tensor> state_out, at::Tensor top_p,
                  at::Tensor top_w, int64_t period, at::Tensor mem_new,
                  at::Tensor h_new, at::Tensor table, at::Tensor mem_next,
                  at::Tensor xh_next, at::Tensor exp_next,
                  at::Tensor last_word, at::Tensor parent) {
    TORCH_CHECK(state_in.size() == 6 && state_in[1].dim() == 3,
                "beam_advance: bad state_in");
    const int64_t B = state_in[1].size(0), W = state_in[1].size(1),
                  T = state_in[1].size(2);
    CHECK_GPU(top_p); CHECK_CONTIG(top_p); CHECK_F32(top_p);
    CHECK_GPU(top_w); CHECK_CONTIG(top_w);
    TORCH_CHECK(top_w.scalar_type() == at::kLong, "top_w must be int64");
    TORCH_CHECK(top_p.dim() == 2 && top_p.size(0) == B * W,
                "top_p must be [B*W,K]");
    const int64_t K = top_p.size(1);
    TORCH_CHECK(top_w.dim() == 2 && top_w.size(0) == B * W
                && top_w.size(1) == K, "top_w must be [B*W,K]");
    TORCH_CHECK(W >= 1 && W <= MAX_BEAM && K >= 1 && K <= MAX_TOPK
                && T >= 1, "beam_advance: 1 <= W <= 8, 1 <= K <= 9");
    TORCH_CHECK(B >= 1 && B * W * std::max(T, K) < INT_MAX,
                "beam_advance: batch out of range");
    BeamState in = beam_state(state_in, B, W, T, "state_in");
    BeamState out = beam_state(state_out, B, W, T, "state_out");
    for (int i = 0; i < 6; ++i)
        TORCH_CHECK(state_in[i].data_ptr() != state_out[i].data_ptr(),
                    "beam_advance: state_in and state_out must differ");

    TORCH_CHECK(mem_new.dim() == 2 && table.dim() == 2
                && xh_next.dim() == 2, "beam_advance: 2-D rows expected");
    const int64_t H = mem_new.size(1), E = table.size(1),
                  V = table.size(0);
    const int64_t D = xh_next.size(1) - E - H;
    TORCH_CHECK(D >= 0 && H % 8 == 0 && E % 8 == 0 && D % 8 == 0
                && H >= 8 && E >= 8,
                "beam_advance: H, E, D must be multiples of 8");
    check_rows(mem_new, B * W, H, "mem_new");
    check_rows(h_new, B * W, H, "h_new");
    check_rows(table, V, E, "table");
    check_rows(mem_next, B * W, H, "mem_next");
    check_rows(xh_next, B * W, D + E + H, "xh_next");
    TORCH_CHECK(V >= 1 && V < INT_MAX && (H + D + E) * B * W < INT_MAX);
    TORCH_CHECK(mem_new.data_ptr() != mem_next.data_ptr(),
                "beam_advance: mem_new and mem_next must differ");
    bf16* exp_ptr = nullptr;
    if (exp_next.defined() && exp_next.numel() > 0) {
        check_rows(exp_next, B * W, H + D + E, "exp_next");
        exp_ptr = (bf16*)exp_next.data_ptr();
    }
    CHECK_GPU(last_word); CHECK_CONTIG(last_word);
    CHECK_GPU(parent); CHECK_CONTIG(parent);
    TORCH_CHECK(last_word.scalar_type() == at::kLong
                && parent.scalar_type() == at::kLong
                && last_word.numel() == B * W && parent.numel() == B * W,
                "last_word and parent must be int64 with B*W entries");

    hipStream_t stream = at::cuda::getCurrentCUDAStream();
    hipLaunchKernelGGL(beam_advance_kernel, dim3((unsigned)B), dim3(256), 0,
                       stream, in, out, (const float*)top_p.data_ptr(),
                       (const int64_t*)top_w.data_ptr(),
                       (const bf16*)mem_new.data_ptr(),
                       (const bf16*)h_new.data_ptr(),
                       (const bf16*)table.data_ptr(),
                       (bf16*)mem_next.data_ptr(),
                       (bf16*)xh_next.data_ptr(), exp_ptr,
                       (int64_t*)last_word.data_ptr(),
                       (int64_t*)parent.data_ptr(), (int)W, (int)K, (int)T,
                       (int)H, (int)D, (int)E, (int)V, period);
    HIP_OK(hipGetLastError());
}

// contexts [B,L,D], l1 [B,L] fp32, wb [L,H], xh [B*W,D+E+H]: pooled
// contexts into pool [B*W,D] and xh[:, :D] (the same bits), softmax
// weights into alpha [B*W,L] fp32 unless it is empty.  split = S, the
// number of blocks per image (0: chosen here).
void beam_attend(at::Tensor contexts, at::Tensor l1, at::Tensor wb,
                 at::Tensor xh, at::Tensor pool, at::Tensor alpha,
                 int64_t split) {
    CHECK_GPU(contexts); CHECK_CONTIG(contexts); CHECK_BF16(contexts);
    CHECK_GPU(l1); CHECK_CONTIG(l1); CHECK_F32(l1);
    TORCH_CHECK(contexts.dim() == 3 && wb.dim() == 2 && xh.dim() == 2,
                "beam_attend: contexts [B,L,D], wb [L,H], xh [B*W,D+E+H]");
    const int64_t B = contexts.size(0), L = contexts.size(1),
                  D = contexts.size(2), H = wb.size(1);
    TORCH_CHECK(B >= 1 && xh.size(0) % B == 0,
                "beam_attend: xh rows must be B*W");
    const int64_t W = xh.size(0) / B, E = xh.size(1) - D - H;
    TORCH_CHECK(W >= 1 && W <= MAX_BEAM, "beam_attend: 1 <= W <= 8");
    TORCH_CHECK(L >= 1 && L <= ATT_MAX_L, "beam_attend: 1 <= L <= ",
                ATT_MAX_L);
    TORCH_CHECK(H >= 8 && H <= ATT_MAX_H && H % 8 == 0 && D >= 8
                && D % 8 == 0 && E >= 0 && E % 8 == 0,
                "beam_attend: D, E, H multiples of 8, 8 <= H <= ",
                ATT_MAX_H);
    TORCH_CHECK(((uintptr_t)contexts.data_ptr() & 15) == 0,
                "contexts must be 16-byte aligned");
    TORCH_CHECK(l1.dim() == 2 && l1.size(0) == B && l1.size(1) == L,
                "l1 must be [B,L]");
    check_rows(wb, L, H, "wb");
    check_rows(xh, B * W, D + E + H, "xh");
    check_rows(pool, B * W, D, "pool");
    TORCH_CHECK(B * L * D < INT_MAX && B * W * (D + E + H) < INT_MAX
                && B * W * L < INT_MAX && L * H < INT_MAX,
                "beam_attend: batch out of range");
    float* alpha_ptr = nullptr;
    if (alpha.defined() && alpha.numel() > 0) {
        CHECK_GPU(alpha); CHECK_CONTIG(alpha); CHECK_F32(alpha);
        TORCH_CHECK(alpha.dim() == 2 && alpha.size(0) == B * W
                    && alpha.size(1) == L, "alpha must be [B*W,L]");
        alpha_ptr = (float*)alpha.data_ptr();
    }

    const int nvec = (int)(D / 8);
    TORCH_CHECK(split >= 0 && split <= nvec,
                "beam_attend: 0 <= split <= D / 8");
    int S = (int)split;
    if (S == 0) S = att_split((int)B, nvec);
    const int cv = cdiv(nvec, S);
    int CW = 1;
    while (CW < cv && CW < ATT_THREADS) CW <<= 1;
    const size_t ub = att_union_bytes((int)W, (int)H);
    const size_t lds = ub + (size_t)W * L * sizeof(float);

    hipStream_t stream = at::cuda::getCurrentCUDAStream();
#define LAUNCH_ATTEND(WW) \
    case WW: \
        hipLaunchKernelGGL(beam_attend_kernel<WW>, \
                           dim3((unsigned)B, (unsigned)S), \
                           dim3(ATT_THREADS), lds, stream, \
                           (const bf16*)contexts.data_ptr(), \
                           (const float*)l1.data_ptr(), \
                           (const bf16*)wb.data_ptr(), \
                           (bf16*)xh.data_ptr(), (bf16*)pool.data_ptr(), \
                           alpha_ptr, (int)L, (int)D, (int)E, (int)H, cv, \
                           CW, (int)ub); \
        break;
    switch (W) {
        LAUNCH_ATTEND(1) LAUNCH_ATTEND(2) LAUNCH_ATTEND(3) LAUNCH_ATTEND(4)
        LAUNCH_ATTEND(5) LAUNCH_ATTEND(6) LAUNCH_ATTEND(7) LAUNCH_ATTEND(8)
    }
#undef LAUNCH_ATTEND
    HIP_OK(hipGetLastError());
}
