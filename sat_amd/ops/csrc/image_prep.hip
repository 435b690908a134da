// resize_normalize_u8: the device half of the input pipeline
// (sat_amd/data/pipeline.py).  N uint8 RGB images of different sizes,
// packed HWC one after the other, become the [N,3,OH,OW] channels_last
// tensor the first conv reads: Pillow's 8-bit bilinear resize (horizontal
// pass, rounded to 8 bits, then vertical pass, rounded again; integer
// arithmetic on Q22 coefficients the host built in float64), minus the
// per-channel mean in fp32, cast to bf16 or fp32.  Integer sums are exact
// in any order, so the result has Pillow's bytes whatever the tiling.
//
// One block per (image, tile of TILE_ROWS output rows).  The source rows
// the tile needs are taken in chunks of `rch`: the block runs the
// horizontal pass of a chunk into LDS as uint8 rows, then every lane adds
// the chunk's share of the vertical sums of its own 4-byte groups to
// accumulators it alone owns (LDS too: their number depends on OW).  A
// 640x480 -> 224x224 tile needs 20 source rows and takes one chunk; a
// tall image takes more chunks in the same LDS.  Tap counts are per image
// and looped over.  Everything read is checked against the buffer sizes
// (the tables live on the device, the host cannot check them): an image
// whose descriptor does not fit is written as zeros minus the mean.

#include "common.h"

#include <climits>

namespace {

constexpr int TILE_ROWS = 8;
constexpr int MAX_CHUNK = 32;
constexpr int THREADS = 256;
constexpr int LDS_BYTES = 64 * 1024;
constexpr uint32_t HALF = 1u << 21;      // Pillow: 1 << (PRECISION_BITS-1)
constexpr int SHIFT = 22;

__device__ __forceinline__ uint32_t clip8(uint32_t acc) {
    return min(acc >> SHIFT, 255u);
}

template <typename T> struct alignas(sizeof(T) * 4) Quad { T v[4]; };

struct AxisTable {
    const int32_t* first;   // [out]
    const int32_t* count;   // [out]
    const int32_t* coef;    // [out, taps]
    int taps;
};

// the table of `out` outputs at tables[off], or taps = 0 when it does
// not lie inside the buffer
__device__ __forceinline__ AxisTable axis_table(
        const int32_t* __restrict__ tables, int64_t n_tables, int64_t off,
        int64_t taps, int out) {
    AxisTable t;
    const bool ok = off >= 0 && taps >= 1 && taps <= INT_MAX / 4
        && off + (int64_t)out * (2 + taps) <= n_tables;
    t.first = tables + (ok ? off : 0);
    t.count = t.first + out;
    t.coef = t.count + out;
    t.taps = ok ? (int)taps : 0;
    return t;
}

template <typename T>
__global__ __launch_bounds__(THREADS)
void resize_normalize_u8_kernel(const uint8_t* __restrict__ packed,
                                int64_t n_packed,
                                const int64_t* __restrict__ desc,
                                const int32_t* __restrict__ tables,
                                int64_t n_tables,
                                const float* __restrict__ mean,
                                T* __restrict__ out, int OH, int OW,
                                int tiles, int rch, int rowb) {
    extern __shared__ __align__(16) unsigned char smem[];
    uint32_t* acc = (uint32_t*)smem;                    // [TILE_ROWS][rowb]
    uint8_t* hrow = smem + (size_t)TILE_ROWS * rowb * 4;    // [rch][rowb]

    const int tid = threadIdx.x;
    const int n = blockIdx.x / tiles;
    const int r0 = (blockIdx.x - n * tiles) * TILE_ROWS;
    const int nr = min(TILE_ROWS, OH - r0);
    const int rowd = rowb >> 2;             // 4-byte groups per row
    const int items = nr * rowd;

    const int64_t* d = desc + (int64_t)n * 8;
    const int64_t off = d[0], H64 = d[1], W64 = d[2];
    const AxisTable ht = axis_table(tables, n_tables, d[3], d[4], OW);
    const AxisTable vt = axis_table(tables, n_tables, d[5], d[6], OH);
    // H*W*3 <= 2^31 * 3 for sides below 2^16: no overflow in int64
    const bool fits = H64 >= 1 && W64 >= 1 && H64 < 65536 && W64 < 65536
        && off >= 0 && off <= n_packed
        && H64 * W64 * 3 <= n_packed - off && ht.taps && vt.taps;
    const int H = fits ? (int)H64 : 0, W = fits ? (int)W64 : 0;
    const uint8_t* src = packed + (fits ? off : 0);

    for (int i = tid; i < items; i += THREADS) {
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i * 4 + j] = 0;
    }

    // source rows of this tile: first of its first output row to last of
    // its last (both grow with the row), clamped to the image
    int y0 = 0, y1 = 0;
    if (fits) {
        y0 = min(max(vt.first[r0], 0), H);
        const int rl = r0 + nr - 1;
        y1 = min(max(vt.first[rl] + min(vt.count[rl], vt.taps), y0), H);
    }

    for (int c0 = y0; c0 < y1; c0 += rch) {
        const int c1 = min(c0 + rch, y1);
        __syncthreads();        // the last chunk's rows have been read

        // horizontal pass: source rows [c0, c1) -> uint8 rows of 3*OW
        for (int i = tid; i < (c1 - c0) * OW; i += THREADS) {
            const int yy = i / OW, x = i - yy * OW;
            const int first = min(max(ht.first[x], 0), W);
            const int cnt = min(min(ht.count[x], ht.taps), W - first);
            const int32_t* cf = ht.coef + (int64_t)x * ht.taps;
            const uint8_t* p = src + ((int64_t)(c0 + yy) * W + first) * 3;
            uint32_t s0 = HALF, s1 = HALF, s2 = HALF;
            for (int k = 0; k < cnt; ++k) {
                const uint32_t c = (uint32_t)cf[k];
                s0 += c * p[0];
                s1 += c * p[1];
                s2 += c * p[2];
                p += 3;
            }
            uint8_t* q = hrow + yy * rowb + 3 * x;
            q[0] = (uint8_t)clip8(s0);
            q[1] = (uint8_t)clip8(s1);
            q[2] = (uint8_t)clip8(s2);
        }
        __syncthreads();

        // this chunk's share of the vertical sums, 4 bytes per item
        for (int i = tid; i < items; i += THREADS) {
            const int r = i / rowd, g = i - r * rowd;
            const int first = vt.first[r0 + r];
            const int cnt = min(vt.count[r0 + r], vt.taps);
            const int ka = max(first, c0), kb = min(first + cnt, c1);
            if (ka >= kb) continue;
            const int32_t* cf = vt.coef + (int64_t)(r0 + r) * vt.taps
                                - first;
            uint32_t a0 = 0, a1 = 0, a2 = 0, a3 = 0;
            for (int y = ka; y < kb; ++y) {
                const uint32_t v =
                    *(const uint32_t*)(hrow + (y - c0) * rowb + 4 * g);
                const uint32_t c = (uint32_t)cf[y];
                a0 += c * (v & 255u);
                a1 += c * ((v >> 8) & 255u);
                a2 += c * ((v >> 16) & 255u);
                a3 += c * (v >> 24);
            }
            acc[i * 4 + 0] += a0;
            acc[i * 4 + 1] += a1;
            acc[i * 4 + 2] += a2;
            acc[i * 4 + 3] += a3;
        }
    }

    // round to 8 bits, subtract the mean, cast, store NHWC.  Each lane
    // reads back only accumulators it wrote itself.
    const float m0 = mean[0], m1 = mean[1], m2 = mean[2];
    const int rowlen = 3 * OW;
    const bool vec = (rowlen & 3) == 0;
    for (int i = tid; i < items; i += THREADS) {
        const int r = i / rowd, g = i - r * rowd;
        T* o = out + ((int64_t)n * OH + r0 + r) * rowlen;
        Quad<T> q;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int ch = (4 * g + j) % 3;
            const float px = (float)clip8(acc[i * 4 + j] + HALF);
            q.v[j] = (T)(px - (ch == 0 ? m0 : ch == 1 ? m1 : m2));
        }
        if (vec) {
            *(Quad<T>*)(o + 4 * g) = q;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (4 * g + j < rowlen) o[4 * g + j] = q.v[j];
        }
    }
}

}  // namespace

at::Tensor resize_normalize_u8(at::Tensor packed, at::Tensor desc,
                               at::Tensor tables, at::Tensor mean,
                               int64_t OH, int64_t OW, bool bf16_out) {
    CHECK_GPU(packed); CHECK_CONTIG(packed);
    CHECK_GPU(desc); CHECK_CONTIG(desc);
    CHECK_GPU(tables); CHECK_CONTIG(tables);
    CHECK_GPU(mean); CHECK_CONTIG(mean); CHECK_F32(mean);
    TORCH_CHECK(packed.scalar_type() == at::kByte && packed.dim() == 1,
                "packed must be 1-D uint8");
    TORCH_CHECK(desc.scalar_type() == at::kLong && desc.dim() == 2
                && desc.size(1) == 8, "desc must be [N,8] int64");
    TORCH_CHECK(tables.scalar_type() == at::kInt && tables.dim() == 1,
                "tables must be 1-D int32");
    TORCH_CHECK(mean.numel() == 3, "mean must hold 3 values");
    TORCH_CHECK(desc.device() == packed.device()
                && tables.device() == packed.device()
                && mean.device() == packed.device(),
                "all inputs must be on one device");
    const int64_t N = desc.size(0);
    TORCH_CHECK(OH >= 1 && OW >= 1 && OH < INT_MAX, "bad output size");
    const int64_t rowb = (3 * OW + 3) / 4 * 4;
    // LDS: TILE_ROWS rows of uint32 accumulators + rch uint8 rows
    const int64_t room = (LDS_BYTES - TILE_ROWS * rowb * 4) / rowb;
    TORCH_CHECK(room >= 1, "resize_normalize_u8: output rows of ", OW,
                " pixels do not fit the LDS tile");
    const int rch = (int)std::min<int64_t>(room, MAX_CHUNK);
    const int64_t tiles = (OH + TILE_ROWS - 1) / TILE_ROWS;
    TORCH_CHECK(N * tiles < INT_MAX && N * OH * OW < INT_MAX,
                "resize_normalize_u8: batch too large");

    at::Tensor out = at::empty(
        {N, 3, OH, OW},
        packed.options()
            .dtype(bf16_out ? at::kBFloat16 : at::kFloat)
            .memory_format(at::MemoryFormat::ChannelsLast));
    if (N == 0) return out;
    const size_t lds = (size_t)(TILE_ROWS * 4 + rch) * rowb;
    hipStream_t stream = at::cuda::getCurrentCUDAStream();
#define LAUNCH(T) \
    hipLaunchKernelGGL(resize_normalize_u8_kernel<T>, \
                       dim3((unsigned)(N * tiles)), dim3(THREADS), lds, \
                       stream, (const uint8_t*)packed.data_ptr(), \
                       packed.numel(), (const int64_t*)desc.data_ptr(), \
                       (const int32_t*)tables.data_ptr(), tables.numel(), \
                       (const float*)mean.data_ptr(), (T*)out.data_ptr(), \
                       (int)OH, (int)OW, (int)tiles, rch, (int)rowb)
    if (bf16_out) LAUNCH(bf16); else LAUNCH(float);
#undef LAUNCH
    HIP_OK(hipGetLastError());
    return out;
}
