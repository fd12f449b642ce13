// prdc.hip - improved precision / recall (Kynkaanniemi et al. 2019) and density / coverage (Naeem et al. 2020) of a
// generated set against a real set, on the bf16 search descriptors of nearest.hip (bg_nn_pack): the kernels of
// metrics.Prdc.
//
//   radii    radius[n] = the k-th smallest squared distance of row n to the other rows of its own set (k <= 8)
//   cover    count[n] = #{i : d(q_i, set_n) <= radius_q[i]} and dmin[n] = min_i d(q_i, set_n) over all queries
//   reduce   the four integers behind the four scores, as int64, so that an event ends with one 32-byte copy
//
// All pairs of two sets of thousands of rows are needed, and of each [Q, N] matrix one or two numbers per row: the matrix
// is never written.  The distance is the search kernel's, by the same function: a block owns 16 set rows and walks ALL
// queries in tiles of 8 with the row walker of rowdist.h, which describes the arithmetic, the tiling and the order of
// summation.  rd_tile leaves d(query slot i, row r) in the lane pair l >> 1 = 4 i + r, and d(a, b) and d(b, a) are the
// same bits, so the radii, the membership tests and the search kernel's matrix agree bit for bit.
//
// The lane pair keeps its own running state across the query tiles: a K-long ascending list in registers (an unrolled
// insertion: the list is never indexed by a variable), or an integer count against radius_q[i], read once per tile, and a
// running minimum.  After the last tile the 8 lane pairs of a row (lane bits 3..5) merge through shuffles.  Every
// reduction is local to the block that owns the row: no second pass, no workspace, no atomics, and a repeated launch is
// bit-identical.  Pseudo-queries past Q (staged as zeros) and rows past N (which repeat the last row) do not contribute;
// in the radii kernel the pair with the row's own index is left out by index, so a different row of equal content counts.
#include "common.h"
#include "rowdist.h"

#include <math.h>

namespace bg {

#define PR_BLOCK 256                 // the reduce kernel
#define PR_MAX_K 8

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
__global__ __launch_bounds__(RD_BLOCK) void prdc_radii_kernel(const uint16_t* __restrict__ x, int64_t N, int D, int k,
                                                              float* __restrict__ radius) {
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int64_t row0 = (int64_t)blockIdx.x * RD_ROWS + wave * RD_RW;
    const uint16_t* rows[RD_RW];
    rd_rows(x, N, D, row0, rows);
    const int i = lane >> 3;
    const int64_t n = row0 + ((lane >> 1) & 3);
    float bv[K];
#pragma unroll
    for (int j = 0; j < K; ++j) bv[j] = INFINITY;
    RowsAhead ahead;
    rd_prologue(ahead, rows, D, lane);
    for (int64_t q0 = 0; q0 < N; q0 += RD_QT) {
        const float d = rd_tile(ahead, x, q0, N, rows, D, t, lane);
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
__global__ __launch_bounds__(RD_BLOCK) void prdc_cover_kernel(const uint16_t* __restrict__ q, const float* __restrict__ radius_q,
                                                              int64_t Q, const uint16_t* __restrict__ set, int64_t N, int D,
                                                              int32_t* __restrict__ count, float* __restrict__ dmin) {
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int64_t row0 = (int64_t)blockIdx.x * RD_ROWS + wave * RD_RW;
    const uint16_t* rows[RD_RW];
    rd_rows(set, N, D, row0, rows);
    const int i = lane >> 3;
    const int64_t n = row0 + ((lane >> 1) & 3);
    int cnt = 0;
    float mn = INFINITY;
    RowsAhead ahead;
    rd_prologue(ahead, rows, D, lane);
    for (int64_t q0 = 0; q0 < Q; q0 += RD_QT) {
        const bool valid = q0 + i < Q;
        const float rad = valid && radius_q ? radius_q[q0 + i] : 0.0f;
        const float d = rd_tile(ahead, q, q0, Q, rows, D, t, lane);
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

static inline bool prdc_rows_fit(int64_t N) { return N > 0 && (N + RD_ROWS - 1) / RD_ROWS <= 0x7fffffffLL; }

}  // namespace bg

using namespace bg;

extern "C" {

int bg_prdc_radii(const void* x, int64_t N, int D, int k, float* radius, void* stream) {
    BG_REQUIRE(x && radius, "bg_prdc_radii: NULL pointer");
    BG_REQUIRE(k >= 1 && k <= PR_MAX_K, "bg_prdc_radii: k=%d (1..%d)", k, PR_MAX_K);
    BG_REQUIRE(prdc_rows_fit(N) && N >= (int64_t)k + 1, "bg_prdc_radii: N=%lld (at least k + 1 = %d rows)", (long long)N, k + 1);
    BG_REQUIRE(D >= 64 && D % 64 == 0, "bg_prdc_radii: D=%d (a multiple of 64)", D);
    BG_REQUIRE(((uintptr_t)x & 15) == 0 && ((uintptr_t)radius & 3) == 0, "bg_prdc_radii: x must be 16-byte aligned");
    const dim3 grid((unsigned)((N + RD_ROWS - 1) / RD_ROWS));
    if (k <= 4)
        hipLaunchKernelGGL(prdc_radii_kernel<4>, grid, dim3(RD_BLOCK), 0, as_stream(stream), static_cast<const uint16_t*>(x), N,
                           D, k, radius);
    else
        hipLaunchKernelGGL(prdc_radii_kernel<8>, grid, dim3(RD_BLOCK), 0, as_stream(stream), static_cast<const uint16_t*>(x), N,
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
    hipLaunchKernelGGL(prdc_cover_kernel, dim3((unsigned)((N + RD_ROWS - 1) / RD_ROWS)), dim3(RD_BLOCK), 0, as_stream(stream),
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
