// prdc.hip - improved precision / recall (Kynkaanniemi et al. 2019) and density / coverage (Naeem et al. 2020) of a
// generated set against a real set, on the bf16 search descriptors of nearest.hip (bg_nn_pack): the kernels of
// metrics.Prdc.
//
//   radii    radius[n] = the k-th smallest squared distance of row n to the other rows of its own set (k <= 8)
//   cover    count[n] = #{i : d(q_i, set_n) <= radius_q[i]} and dmin[n] = min_i d(q_i, set_n) over all queries
//   reduce   the four integers behind the four scores, as int64, so that an event ends with one 32-byte copy
//
// All pairs of two sets of thousands of rows are needed, and of each [Q, N] matrix one or two numbers per row: the matrix
// is never written.  The distance is that of nn_distances_kernel, restated here so that nearest.hip keeps its bits: fp32
// differences of exactly widened bf16, one fma per term, no |q|^2 + |s|^2 - 2 q.s expansion and no MFMA, so equal rows
// give 0.0f.  A block of 256 threads owns PR_ROWS = 16 set rows, four per wave, and walks ALL queries in tiles of PR_QT = 8,
// staged in LDS in chunks of PR_DC = 2048 elements (rows of 4 KiB: lane-contiguous 16-byte reads, so every 16-lane group
// of a ds_read_b128 covers the 64 banks once).  Lane l holds elements [8 l, 8 l + 8) of its four rows and 8 x 4 packed
// accumulators; after the last chunk the transposing butterfly leaves d(query slot i, row r) in the lane pair
// l >> 1 = 4 i + r.  The order of summation depends on the element index alone (elements of one lane in sequence, then a
// balanced tree over lanes whose additions commute), so d(a, b) and d(b, a) are the same bits, and the radii and the
// membership tests use one function, prdc_tile.  With 16 rows a block, a few thousand rows leave one or two waves per
// SIMD, so the loop itself keeps loads in flight: the eight staging loads of a chunk are issued before the first LDS store,
// and a lane loads its rows' next 16 bytes while it computes on the current ones (PrdcAhead).
//
// The lane pair keeps its own running state across the query tiles: a K-long ascending list in registers (an unrolled
// insertion: the list is never indexed by a variable), or an integer count against radius_q[i], read once per tile, and a
// running minimum.  After the last tile the 8 lane pairs of a row (lane bits 3..5) merge through shuffles.  Every
// reduction is local to the block that owns the row: no second pass, no workspace, no atomics, and a repeated launch is
// bit-identical.  Pseudo-queries past Q (staged as zeros) and rows past N (which repeat the last row) do not contribute;
// in the radii kernel the pair with the row's own index is left out by index, so a different row of equal content counts.
#include "common.h"

#include <math.h>

namespace bg {

#define PR_BLOCK 256
#define PR_QT 8
#define PR_RW 4                      // set rows per wave
#define PR_ROWS (4 * PR_RW)          // set rows per block
#define PR_DC 2048                   // elements of a query row staged per pass
#define PR_MAX_K 8

typedef float pr_f2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ void pr_unpack(const uint4& w, pr_f2 (&v)[4]) {       // bf16 pairs, widened exactly
    v[0] = pr_f2{__uint_as_float(w.x << 16), __uint_as_float(w.x & 0xffff0000u)};
    v[1] = pr_f2{__uint_as_float(w.y << 16), __uint_as_float(w.y & 0xffff0000u)};
    v[2] = pr_f2{__uint_as_float(w.z << 16), __uint_as_float(w.z & 0xffff0000u)};
    v[3] = pr_f2{__uint_as_float(w.w << 16), __uint_as_float(w.w & 0xffff0000u)};
}

// one step of the transposing butterfly: HALF values stay, each plus the partner lane's counterpart of the other half
template <int HALF>
__device__ __forceinline__ void pr_fold(float (&v)[PR_QT * PR_RW], int lane) {
    constexpr int dist = HALF == 16 ? 32 : HALF == 8 ? 16 : HALF == 4 ? 8 : HALF == 2 ? 4 : 2;
    const bool hi = (lane & dist) != 0;
#pragma unroll
    for (int i = 0; i < HALF; ++i) {
        const float keep = hi ? v[i + HALF] : v[i];
        const float send = hi ? v[i] : v[i + HALF];
        v[i] = keep + __shfl_xor(send, dist, 64);
    }
}

// What a lane holds ahead of its use: the 16 bytes of its four rows for the NEXT turn of the walk, loaded while this turn
// is computed, so that the walk does not wait for a global load per turn.  The chain runs on across chunks and tiles; the
// rows are the same for every tile, so it wraps to their first chunk.  16 registers: the kernels stay at two waves per
// SIMD (holding the next chunk of the queries as well costs 32 more and the second wave; measured slower at 8192 rows).
// Prefetching changes no arithmetic and no order.
struct PrdcAhead {
    uint4 s[PR_RW];
};

// the wave's rows at elements [c0 + o, c0 + o + 8); zeros past the end of the chunk
__device__ __forceinline__ void prdc_fetch_rows(PrdcAhead& a, const uint16_t* const (&rows)[PR_RW], int D, int c0, int o) {
    const int len = D - c0 < PR_DC ? D - c0 : PR_DC;
#pragma unroll
    for (int r = 0; r < PR_RW; ++r) {
        a.s[r] = uint4{0u, 0u, 0u, 0u};
        if (o < len) a.s[r] = *reinterpret_cast<const uint4*>(rows[r] + c0 + o);
    }
}

__device__ __forceinline__ void prdc_prologue(PrdcAhead& a, const uint16_t* const (&rows)[PR_RW], int D, int lane) {
    prdc_fetch_rows(a, rows, D, 0, lane * 8);
}

// The squared distances of the query tile [q0, q0 + PR_QT) to the wave's four rows.  Every thread of the block calls it
// (it holds the barriers of the staging).  Returns d(q0 + i, rows[r]) for i = lane >> 3, r = (lane >> 1) & 3; the two
// lanes of a pair hold the same value.  Queries past Q are zeros.  ``a`` holds this tile's first turn on entry
// (prdc_prologue, or the previous call) and the next tile's on return.
__device__ __forceinline__ float prdc_tile(PrdcAhead& a, const uint16_t* __restrict__ q, int64_t q0, int64_t Q,
                                           const uint16_t* const (&rows)[PR_RW], int D, int t, int lane) {
    __shared__ __attribute__((aligned(16))) uint16_t qs[PR_QT * PR_DC];      // the tile's chunk of the queries, rows of 4 KiB
    pr_f2 acc[PR_QT][PR_RW];
#pragma unroll
    for (int i = 0; i < PR_QT; ++i)
#pragma unroll
        for (int r = 0; r < PR_RW; ++r) acc[i][r] = pr_f2{0.0f, 0.0f};
    for (int c0 = 0; c0 < D; c0 += PR_DC) {
        const int len = D - c0 < PR_DC ? D - c0 : PR_DC;        // a multiple of 8
        __syncthreads();                                        // the previous chunk has been read
        if (t * 8 < len) {                                      // PR_DC = 8 PR_BLOCK: one piece of every query per thread
            uint4 w[PR_QT];                                     // all eight loads are in flight before the first store
#pragma unroll
            for (int i = 0; i < PR_QT; ++i)
                w[i] = *reinterpret_cast<const uint4*>(q + (q0 + i < Q ? q0 + i : 0) * (int64_t)D + c0 + t * 8);
            __builtin_amdgcn_sched_barrier(0);                  // (or the scheduler waits for the first before the fourth)
#pragma unroll
            for (int i = 0; i < PR_QT; ++i)                     // queries past the end are zeros
                *reinterpret_cast<uint4*>(&qs[i * PR_DC + t * 8]) = q0 + i < Q ? w[i] : uint4{0u, 0u, 0u, 0u};
        }
        __syncthreads();
        for (int o = lane * 8; o < len + lane * 8; o += 512) {  // every lane of the wave makes the same number of turns
            const bool in = o < len;
            pr_f2 sv[PR_RW][4];
#pragma unroll
            for (int r = 0; r < PR_RW; ++r) pr_unpack(a.s[r], sv[r]);
            if (o + 512 < len + lane * 8)                       // the next turn; after the last, the next chunk's first
                prdc_fetch_rows(a, rows, D, c0, o + 512);
            else
                prdc_fetch_rows(a, rows, D, c0 + PR_DC < D ? c0 + PR_DC : 0, lane * 8);
#pragma unroll
            for (int i = 0; i < PR_QT; ++i) {
                uint4 w = uint4{0u, 0u, 0u, 0u};
                if (in) w = *reinterpret_cast<const uint4*>(&qs[i * PR_DC + o]);
                pr_f2 qv[4];
                pr_unpack(w, qv);
#pragma unroll
                for (int r = 0; r < PR_RW; ++r)
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const pr_f2 d = qv[j] - sv[r][j];
                        acc[i][r] = __builtin_elementwise_fma(d, d, acc[i][r]);
                    }
            }
        }
    }
    float v[PR_QT * PR_RW];
#pragma unroll
    for (int i = 0; i < PR_QT; ++i)
#pragma unroll
        for (int r = 0; r < PR_RW; ++r) v[i * PR_RW + r] = acc[i][r].x + acc[i][r].y;
    pr_fold<16>(v, lane);
    pr_fold<8>(v, lane);
    pr_fold<4>(v, lane);
    pr_fold<2>(v, lane);
    pr_fold<1>(v, lane);
    return v[0] + __shfl_xor(v[0], 1, 64);
}

__device__ __forceinline__ void prdc_rows(const uint16_t* set, int64_t N, int D, int64_t row0,
                                          const uint16_t* (&rows)[PR_RW]) {
#pragma unroll
    for (int r = 0; r < PR_RW; ++r) {
        const int64_t n = row0 + r < N ? row0 + r : N - 1;      // rows past the end repeat the last one; not stored
        rows[r] = set + n * D;
    }
}

// an ascending list of the K smallest values seen, equal values kept with multiplicity
template <int K>
__device__ __forceinline__ void pr_insert(float (&bv)[K], float v) {
    if (!(v < bv[K - 1])) return;
#pragma unroll
    for (int j = 0; j < K; ++j) {
        if (v < bv[j]) {
            const float tv = bv[j];
            bv[j] = v;
            v = tv;
        }
    }
}

// ---------------------------------------------------------------------------------------------------- radii
template <int K>
__global__ __launch_bounds__(PR_BLOCK) void prdc_radii_kernel(const uint16_t* __restrict__ x, int64_t N, int D, int k,
                                                              float* __restrict__ radius) {
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int64_t row0 = (int64_t)blockIdx.x * PR_ROWS + wave * PR_RW;
    const uint16_t* rows[PR_RW];
    prdc_rows(x, N, D, row0, rows);
    const int i = lane >> 3;
    const int64_t n = row0 + ((lane >> 1) & 3);
    float bv[K];
#pragma unroll
    for (int j = 0; j < K; ++j) bv[j] = INFINITY;
    PrdcAhead ahead;
    prdc_prologue(ahead, rows, D, lane);
    for (int64_t q0 = 0; q0 < N; q0 += PR_QT) {
        const float d = prdc_tile(ahead, x, q0, N, rows, D, t, lane);
        if (q0 + i < N && q0 + i != n) pr_insert<K>(bv, d);
    }
#pragma unroll
    for (int dist = 8; dist <= 32; dist <<= 1) {                // the 8 query slots of a row: lane bits 3..5
        float other[K];
#pragma unroll
        for (int j = 0; j < K; ++j) other[j] = __shfl_xor(bv[j], dist, 64);
#pragma unroll
        for (int j = 0; j < K; ++j) pr_insert<K>(bv, other[j]);
    }
    float out = bv[0];
#pragma unroll
    for (int j = 1; j < K; ++j)
        if (j == k - 1) out = bv[j];
    if ((lane & 57) == 0 && n < N) radius[n] = out;              // query slot 0, the even lane of the pair
}

// ---------------------------------------------------------------------------------------------------- cover
__global__ __launch_bounds__(PR_BLOCK) void prdc_cover_kernel(const uint16_t* __restrict__ q, const float* __restrict__ radius_q,
                                                              int64_t Q, const uint16_t* __restrict__ set, int64_t N, int D,
                                                              int32_t* __restrict__ count, float* __restrict__ dmin) {
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int64_t row0 = (int64_t)blockIdx.x * PR_ROWS + wave * PR_RW;
    const uint16_t* rows[PR_RW];
    prdc_rows(set, N, D, row0, rows);
    const int i = lane >> 3;
    const int64_t n = row0 + ((lane >> 1) & 3);
    int cnt = 0;
    float mn = INFINITY;
    PrdcAhead ahead;
    prdc_prologue(ahead, rows, D, lane);
    for (int64_t q0 = 0; q0 < Q; q0 += PR_QT) {
        const bool valid = q0 + i < Q;
        const float rad = valid && radius_q ? radius_q[q0 + i] : 0.0f;
        const float d = prdc_tile(ahead, q, q0, Q, rows, D, t, lane);
        if (valid) {
            cnt += d <= rad ? 1 : 0;
            mn = fminf(mn, d);
        }
    }
#pragma unroll
    for (int dist = 8; dist <= 32; dist <<= 1) {
        cnt += __shfl_xor(cnt, dist, 64);
        mn = fminf(mn, __shfl_xor(mn, dist, 64));
    }
    if ((lane & 57) == 0 && n < N) {
        if (count) count[n] = cnt;
        if (dmin) dmin[n] = mn;
    }
}

// ---------------------------------------------------------------------------------------------------- reduce
__global__ __launch_bounds__(PR_BLOCK) void prdc_reduce_kernel(const int32_t* __restrict__ count_f, int64_t M,
                                                               const int32_t* __restrict__ count_r,
                                                               const float* __restrict__ dmin_r,
                                                               const float* __restrict__ radius_r, int64_t N,
                                                               int64_t* __restrict__ out4) {
    __shared__ long long part[4][PR_BLOCK];
    const int t = threadIdx.x;
    long long a[4] = {0, 0, 0, 0};
    for (int64_t j = t; j < M; j += PR_BLOCK) {
        const int32_t c = count_f[j];
        a[0] += c > 0 ? 1 : 0;
        a[1] += c;
    }
    for (int64_t n = t; n < N; n += PR_BLOCK) {
        a[2] += count_r[n] > 0 ? 1 : 0;
        a[3] += dmin_r[n] <= radius_r[n] ? 1 : 0;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) part[j][t] = a[j];
    for (int st = PR_BLOCK / 2; st > 0; st >>= 1) {
        __syncthreads();
        if (t < st)
#pragma unroll
            for (int j = 0; j < 4; ++j) part[j][t] += part[j][t + st];
    }
    if (t == 0)
#pragma unroll
        for (int j = 0; j < 4; ++j) out4[j] = part[j][0];
}

static inline bool prdc_rows_fit(int64_t N) { return N > 0 && (N + PR_ROWS - 1) / PR_ROWS <= 0x7fffffffLL; }

}  // namespace bg

using namespace bg;

extern "C" {

int bg_prdc_radii(const void* x, int64_t N, int D, int k, float* radius, void* stream) {
    BG_REQUIRE(x && radius, "bg_prdc_radii: NULL pointer");
    BG_REQUIRE(k >= 1 && k <= PR_MAX_K, "bg_prdc_radii: k=%d (1..%d)", k, PR_MAX_K);
    BG_REQUIRE(prdc_rows_fit(N) && N >= (int64_t)k + 1, "bg_prdc_radii: N=%lld (at least k + 1 = %d rows)", (long long)N, k + 1);
    BG_REQUIRE(D >= 64 && D % 64 == 0, "bg_prdc_radii: D=%d (a multiple of 64)", D);
    BG_REQUIRE(((uintptr_t)x & 15) == 0 && ((uintptr_t)radius & 3) == 0, "bg_prdc_radii: x must be 16-byte aligned");
    const dim3 grid((unsigned)((N + PR_ROWS - 1) / PR_ROWS));
    if (k <= 4)
        hipLaunchKernelGGL(prdc_radii_kernel<4>, grid, dim3(PR_BLOCK), 0, as_stream(stream), static_cast<const uint16_t*>(x), N,
                           D, k, radius);
    else
        hipLaunchKernelGGL(prdc_radii_kernel<8>, grid, dim3(PR_BLOCK), 0, as_stream(stream), static_cast<const uint16_t*>(x), N,
                           D, k, radius);
    BG_LAUNCH_CHECK();
    return BG_OK;
}

int bg_prdc_cover(const void* q, const float* radius_q, int64_t Q, const void* set, int64_t N, int D, int32_t* count,
                  float* dmin, void* stream) {
    BG_REQUIRE(q && set, "bg_prdc_cover: NULL pointer");
    BG_REQUIRE(count || dmin, "bg_prdc_cover: count and dmin are both NULL");
    BG_REQUIRE(!count || radius_q, "bg_prdc_cover: count needs radius_q");
    BG_REQUIRE(Q > 0 && Q <= 0x7fffffffLL && prdc_rows_fit(N), "bg_prdc_cover: Q=%lld N=%lld", (long long)Q, (long long)N);
    BG_REQUIRE(D >= 64 && D % 64 == 0, "bg_prdc_cover: D=%d (a multiple of 64)", D);
    BG_REQUIRE((((uintptr_t)q | (uintptr_t)set) & 15) == 0 &&
                   (((uintptr_t)radius_q | (uintptr_t)count | (uintptr_t)dmin) & 3) == 0,
               "bg_prdc_cover: q and set must be 16-byte aligned");
    hipLaunchKernelGGL(prdc_cover_kernel, dim3((unsigned)((N + PR_ROWS - 1) / PR_ROWS)), dim3(PR_BLOCK), 0, as_stream(stream),
                       static_cast<const uint16_t*>(q), radius_q, Q, static_cast<const uint16_t*>(set), N, D, count, dmin);
    BG_LAUNCH_CHECK();
    return BG_OK;
}

int bg_prdc_reduce(const int32_t* count_f, int64_t M, const int32_t* count_r, const float* dmin_r, const float* radius_r,
                   int64_t N, int64_t* out4, void* stream) {
    BG_REQUIRE(count_f && count_r && dmin_r && radius_r && out4, "bg_prdc_reduce: NULL pointer");
    BG_REQUIRE(M > 0 && N > 0, "bg_prdc_reduce: M=%lld N=%lld", (long long)M, (long long)N);
    BG_REQUIRE((((uintptr_t)count_f | (uintptr_t)count_r | (uintptr_t)dmin_r | (uintptr_t)radius_r) & 3) == 0 &&
                   ((uintptr_t)out4 & 7) == 0,
               "bg_prdc_reduce: misaligned pointer");
    hipLaunchKernelGGL(prdc_reduce_kernel, dim3(1), dim3(PR_BLOCK), 0, as_stream(stream), count_f, M, count_r, dmin_r, radius_r,
                       N, out4);
    BG_LAUNCH_CHECK();
    return BG_OK;
}

}  // extern "C"
