// nearest.hip - nearest training images of generated samples in pixel space: the memorisation check of neighbours.py.
//
//   pack        image batch [B,S,S,C] fp32 or bf16 -> search descriptors bf16 [B, (S/f)(S/f)C]: f x f box mean in fp32,
//               rounded to nearest even; optionally of the horizontally flipped image
//   distances   out[i,n] = sum_j (q[i,j] - set[n,j])^2 over bf16 rows, computed as differences in fp32
//   topk        the k <= 16 smallest (value, index) pairs of every fp32 row, ascending, ties to the lower index
//
// The distance kernel.  A block owns 16 set rows and walks the queries in tiles of 8 with the row walker of rowdist.h,
// which describes the arithmetic, the tiling and the order of summation; the even lane of each lane pair stores its tile's
// d(i, n).  Every (i, n) sum is made by one wave in one fixed order: no atomics, no partials across blocks, and two
// launches give the same bits.
//
// The selection.  A thread scans its part of a row with a stride of 256 and keeps its K best in registers (an unrolled
// insertion, so that the list is never indexed by a variable); the 256 lists are merged pairwise through LDS.  Rows longer
// than NN_TK_SEG are split over blocks, whose lists go through a workspace into a second pass of the same kernel.  The
// order on (value, index) is total, so the result does not depend on how the row was split.
#include "common.h"
#include "rowdist.h"

#include <math.h>

namespace bg {

#define NN_BLOCK 256                 // the pack and selection kernels
#define NN_TK_SEG 16384              // elements of a row per block of the first selection pass
#define NN_TK_MAX_SPLITS 256

__device__ __forceinline__ float nn_widen(float v) { return v; }
__device__ __forceinline__ float nn_widen(uint16_t bits) { return __uint_as_float((uint32_t)bits << 16); }   // bf16, exact

__device__ __forceinline__ uint16_t nn_bf16_rne(float v) {       // finite input
    const uint32_t b = __float_as_uint(v);
    return (uint16_t)((b + 0x7fffu + ((b >> 16) & 1u)) >> 16);
}

// ---------------------------------------------------------------------------------------------------- pack
template <typename T>
__global__ __launch_bounds__(NN_BLOCK) void nn_pack_kernel(const T* __restrict__ x, int B, int S, int C, int f, int mirror,
                                                           uint16_t* __restrict__ out) {
    const int s = S / f;
    const int64_t total = (int64_t)B * s * s * C;
    const float scale = 1.0f / (float)(f * f);
    for (int64_t e = (int64_t)blockIdx.x * NN_BLOCK + threadIdx.x; e < total; e += (int64_t)gridDim.x * NN_BLOCK) {
        const int c = (int)(e % C);
        int64_t r = e / C;
        const int ox = (int)(r % s);
        r /= s;
        const int oy = (int)(r % s);
        const int64_t b = r / s;
        const int sx = mirror ? s - 1 - ox : ox;         // a box of the flipped image is the flipped box: the sum is kept in
        const T* src = x + ((b * S + (int64_t)oy * f) * S + (int64_t)sx * f) * C + c;       // its own column order
        float acc = 0.0f;
        for (int dy = 0; dy < f; ++dy)
            for (int dx = 0; dx < f; ++dx) acc += nn_widen(src[((int64_t)dy * S + (mirror ? f - 1 - dx : dx)) * C]);
        out[e] = nn_bf16_rne(acc * scale);
    }
}

// ---------------------------------------------------------------------------------------------------- distances
__global__ __launch_bounds__(RD_BLOCK) void nn_distances_kernel(const uint16_t* __restrict__ q, const uint16_t* __restrict__ set,
                                                                int Q, int64_t N, int D, float* __restrict__ out) {
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int64_t row0 = (int64_t)blockIdx.x * RD_ROWS + wave * RD_RW;
    const uint16_t* rows[RD_RW];
    rd_rows(set, N, D, row0, rows);
    const int i = lane >> 3;                                         // the lane pair's query slot and row (rd_tile)
    const int64_t n = row0 + ((lane >> 1) & 3);
    RowsAhead ahead;
    rd_prologue(ahead, rows, D, lane);
    for (int q0 = 0; q0 < Q; q0 += RD_QT) {
        const float d = rd_tile(ahead, q, q0, Q, rows, D, t, lane);
        if ((lane & 1) == 0 && q0 + i < Q && n < N) out[(int64_t)(q0 + i) * N + n] = d;
    }
}

// ---------------------------------------------------------------------------------------------------- top-k
__device__ __forceinline__ bool nn_before(float va, int ia, float vb, int ib) { return va < vb || (va == vb && ia < ib); }

template <int K>
__device__ __forceinline__ void nn_insert(float (&bv)[K], int (&bi)[K], float v, int i) {
    if (!nn_before(v, i, bv[K - 1], bi[K - 1])) return;
#pragma unroll
    for (int j = 0; j < K; ++j) {
        if (nn_before(v, i, bv[j], bi[j])) {
            const float tv = bv[j];
            const int ti = bi[j];
            bv[j] = v;
            bi[j] = i;
            v = tv;
            i = ti;
        }
    }
}

// grid (splits, Q).  PAIRS = false: the block scans elements [split * seg, min(n, (split + 1) * seg)) of row blockIdx.y of
// ``val`` [Q, n]; their index is their position.  PAIRS = true: it scans the n (value, index) pairs of row blockIdx.y of
// ``val`` / ``idx``.  The block's K best go to ov / oi + (blockIdx.y * gridDim.x + blockIdx.x) * out_k, the first out_k.
template <int K, bool PAIRS>
__global__ __launch_bounds__(NN_BLOCK) void nn_topk_kernel(const float* __restrict__ val, const int* __restrict__ idx, int64_t n,
                                                           int64_t seg, float* __restrict__ ov, int* __restrict__ oi,
                                                           int out_k) {
    __shared__ float lv[NN_BLOCK * K];
    __shared__ int li[NN_BLOCK * K];
    const int t = threadIdx.x;
    float bv[K];
    int bi[K];
#pragma unroll
    for (int j = 0; j < K; ++j) {
        bv[j] = INFINITY;
        bi[j] = 0x7fffffff;                    // an empty place sorts after every element; written out as -1
    }
    const float* row = val + (int64_t)blockIdx.y * n;
    const int64_t lo = (int64_t)blockIdx.x * seg;
    const int64_t hi = lo + seg < n ? lo + seg : n;
    for (int64_t e = lo + t; e < hi; e += NN_BLOCK) {
        const int i = PAIRS ? idx[(int64_t)blockIdx.y * n + e] : (int)e;
        if (!PAIRS || i >= 0) nn_insert<K>(bv, bi, row[e], i);
    }
#pragma unroll
    for (int j = 0; j < K; ++j) {
        lv[t * K + j] = bv[j];
        li[t * K + j] = bi[j];
    }
    for (int st = 1; st < NN_BLOCK; st <<= 1) {
        __syncthreads();
        if ((t & (2 * st - 1)) == 0) {
            int a = t * K, b = (t + st) * K;                   // two ascending lists -> the first K of their merge
#pragma unroll
            for (int j = 0; j < K; ++j) {
                const bool take_a = nn_before(lv[a], li[a], lv[b], li[b]);
                bv[j] = take_a ? lv[a] : lv[b];
                bi[j] = take_a ? li[a] : li[b];
                a += take_a ? 1 : 0;                           // neither runs past its list: at most K steps in all, and
                b += take_a ? 0 : 1;                           // place K - 1 is the last one read
            }
#pragma unroll
            for (int j = 0; j < K; ++j) {
                lv[t * K + j] = bv[j];
                li[t * K + j] = bi[j];
            }
        }
    }
    if (t == 0) {
        const int64_t o = ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * out_k;
#pragma unroll
        for (int j = 0; j < K; ++j)
            if (j < out_k) {
                ov[o + j] = bv[j];
                oi[o + j] = bi[j] == 0x7fffffff ? -1 : bi[j];
            }
    }
}

static int nn_topk_splits(int64_t N) {
    const int64_t s = (N + NN_TK_SEG - 1) / NN_TK_SEG;
    return (int)(s < 1 ? 1 : (s > NN_TK_MAX_SPLITS ? NN_TK_MAX_SPLITS : s));
}

static inline bool nn_pow2(int v) { return v > 0 && (v & (v - 1)) == 0; }

template <int K>
static void nn_topk_launch(const float* dist, int Q, int64_t N, int k, float* out_dist, int32_t* out_idx, void* ws,
                           hipStream_t s) {
    const int splits = nn_topk_splits(N);
    if (splits == 1) {
        hipLaunchKernelGGL((nn_topk_kernel<K, false>), dim3(1, Q), dim3(NN_BLOCK), 0, s, dist, (const int*)nullptr, N, N,
                           out_dist, out_idx, k);
        return;
    }
    const int64_t seg = (N + splits - 1) / splits;
    float* wv = static_cast<float*>(ws);
    int* wi = reinterpret_cast<int*>(wv + (size_t)Q * splits * K);
    hipLaunchKernelGGL((nn_topk_kernel<K, false>), dim3(splits, Q), dim3(NN_BLOCK), 0, s, dist, (const int*)nullptr, N, seg, wv,
                       wi, K);
    hipLaunchKernelGGL((nn_topk_kernel<K, true>), dim3(1, Q), dim3(NN_BLOCK), 0, s, (const float*)wv, (const int*)wi,
                       (int64_t)splits * K, (int64_t)splits * K, out_dist, out_idx, k);
}

}  // namespace bg

using namespace bg;

extern "C" {

int bg_nn_pack(const void* x, int x_dtype, int B, int S, int C, int f, int mirror, void* out, void* stream) {
    BG_REQUIRE(x && out, "bg_nn_pack: NULL pointer");
    BG_REQUIRE(x_dtype == BG_F32 || x_dtype == BG_BF16, "bg_nn_pack: x_dtype=%d (BG_F32 or BG_BF16)", x_dtype);
    BG_REQUIRE(B > 0 && (C == 1 || C == 3 || C == 4), "bg_nn_pack: B=%d C=%d (C is 1, 3 or 4)", B, C);
    BG_REQUIRE(S > 0 && S <= 16384 && nn_pow2(f) && f <= S && S % f == 0 && S / f >= 8,
               "bg_nn_pack: S=%d f=%d (f a power of two, S / f >= 8)", S, f);
    const int64_t total = (int64_t)B * (S / f) * (S / f) * C;
    const int64_t blocks = (total + NN_BLOCK - 1) / NN_BLOCK;
    const unsigned grid = (unsigned)(blocks > 4096 ? 4096 : blocks);
    if (x_dtype == BG_F32)
        hipLaunchKernelGGL(nn_pack_kernel<float>, dim3(grid), dim3(NN_BLOCK), 0, as_stream(stream),
                           static_cast<const float*>(x), B, S, C, f, mirror != 0, static_cast<uint16_t*>(out));
    else
        hipLaunchKernelGGL(nn_pack_kernel<uint16_t>, dim3(grid), dim3(NN_BLOCK), 0, as_stream(stream),
                           static_cast<const uint16_t*>(x), B, S, C, f, mirror != 0, static_cast<uint16_t*>(out));
    BG_LAUNCH_CHECK();
    return BG_OK;
}

int bg_nn_distances(const void* q, const void* set, int Q, int64_t N, int D, float* out, void* stream) {
    BG_REQUIRE(q && set && out, "bg_nn_distances: NULL pointer");
    BG_REQUIRE(Q > 0 && N > 0 && (N + RD_ROWS - 1) / RD_ROWS <= 0x7fffffffLL, "bg_nn_distances: Q=%d N=%lld", Q, (long long)N);
    BG_REQUIRE(D >= 64 && D % 64 == 0, "bg_nn_distances: D=%d (a multiple of 64)", D);
    BG_REQUIRE((((uintptr_t)q | (uintptr_t)set) & 15) == 0 && ((uintptr_t)out & 3) == 0,
               "bg_nn_distances: q and set must be 16-byte aligned");
    hipLaunchKernelGGL(nn_distances_kernel, dim3((unsigned)((N + RD_ROWS - 1) / RD_ROWS)), dim3(RD_BLOCK), 0, as_stream(stream),
                       static_cast<const uint16_t*>(q), static_cast<const uint16_t*>(set), Q, N, D, out);
    BG_LAUNCH_CHECK();
    return BG_OK;
}

size_t bg_nn_topk_workspace_bytes(int Q, int64_t N, int k) {
    if (Q < 1 || N < 1 || k < 1 || k > 16) return 0;
    const int splits = nn_topk_splits(N);
    return splits == 1 ? 0 : (size_t)Q * splits * (k <= 8 ? 8 : 16) * 8;
}

int bg_nn_topk(const float* dist, int Q, int64_t N, int k, float* out_dist, int32_t* out_idx, void* ws, size_t ws_bytes,
               void* stream) {
    BG_REQUIRE(dist && out_dist && out_idx, "bg_nn_topk: NULL pointer");
    BG_REQUIRE(Q > 0 && Q <= 65535 && N > 0 && N <= 0x7fffffffLL, "bg_nn_topk: Q=%d N=%lld", Q, (long long)N);
    BG_REQUIRE(k >= 1 && k <= 16, "bg_nn_topk: k=%d (1..16)", k);
    const size_t need = bg_nn_topk_workspace_bytes(Q, N, k);
    BG_REQUIRE(need == 0 || (ws && ws_bytes >= need && ((uintptr_t)ws & 3) == 0),
               "bg_nn_topk: workspace of %zu bytes, bg_nn_topk_workspace_bytes(%d, %lld, %d) = %zu needed", ws_bytes, Q,
               (long long)N, k, need);
    if (k <= 8)
        nn_topk_launch<8>(dist, Q, N, k, out_dist, out_idx, ws, as_stream(stream));
    else
        nn_topk_launch<16>(dist, Q, N, k, out_dist, out_idx, ws, as_stream(stream));
    BG_LAUNCH_CHECK();
    return BG_OK;
}

}  // extern "C"
