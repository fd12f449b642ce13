// swd.hip - sliced Wasserstein distance on Laplacian-pyramid patches (Karras et al. 2018, "Progressive Growing of GANs",
// section 5): the in-training quality score of metrics.py.  NHWC images, H = W a power of two.
//
//   pyr_down     g(i+1) = conv(g(i), f x f / 256)[::2, ::2], f = [1 4 6 4 1], mirror boundary without the edge
//                (d c b | a b c d | c b a); input fp32 or bf16, output fp32
//   pyr_lap      g(i) - up(g(i+1)): up puts g(i+1) on the even grid points of a zero image and convolves with 4 x the filter
//   descriptors  128 patches of 7 x 7 per image -> rows [c, dy, dx] of an fp32 [N, 49 C] buffer, plus per-image partial sums
//                and sums of squares per channel in fp64; stats_finish adds them in a fixed order
//   project      out[s][n] = sum_k ((desc[n,k] - mean_c) * rstd_c) * dir[k,s], fp32, k ascending, segment-major output
//   sort         batched bitonic network over segments of 2^m floats
//   l1           sum |a - b| in fp64 through per-block partials, added in a fixed order
//
// Every reduction goes through partial rows that a second kernel adds in index order: no float atomics, so a repeated
// launch is bit-identical.
//
// The sort.  A tile of SW_TILE = 4096 floats lives in LDS (16 KiB, 512 threads).  A thread owns 8 elements at a stride JL
// in {512, 64, 8, 1} and runs the three exchange distances 4 JL, 2 JL, JL on them in registers, so the twelve distances
// below a tile take four LDS round trips instead of twelve, and the three smallest (4, 2, 1) are two 16-byte reads of
// 8 consecutive floats with no exchange between lanes at all.  At JL = 8 the eight loads of a 32-lane group would fall
// on 8 banks (4-way); the tile is therefore stored XOR-swizzled, element i at i ^ (((i >> 6) & 3) << 3), which sends the
// four 64-element rows a group touches to four different bank octets and leaves every aligned run of 8 floats
// contiguous, so the JL = 1 vector reads and the JL >= 64 lane-consecutive reads stay conflict-free.  Distances of a
// tile or more are global passes: a thread holds 2, 4 or 8 float4 at the smallest distance of the pass and runs up to
// three distances per sweep over HBM.
#include "common.h"

namespace bg {

#define SW_BLOCK 256
#define SW_PATCHES 128
#define SW_TAPS 49

__device__ __forceinline__ float sw_widen(float v) { return v; }
__device__ __forceinline__ float sw_widen(uint16_t bits) { return __uint_as_float((uint32_t)bits << 16); }   // bf16, exact

__device__ __forceinline__ int sw_mirror(int i, int n) { return i < 0 ? -i : (i >= n ? 2 * n - 2 - i : i); }

__device__ __forceinline__ float sw_f(int i) { return i == 2 ? 6.0f : ((i == 1 || i == 3) ? 4.0f : 1.0f); }

// ---------------------------------------------------------------------------------------------------- pyramid
template <typename T>
__global__ __launch_bounds__(SW_BLOCK) void swd_pyr_down_kernel(const T* __restrict__ x, float* __restrict__ y, int B, int H,
                                                                int C) {
    const int Ho = H >> 1;
    const int64_t total = (int64_t)B * Ho * Ho * C;
    for (int64_t e = (int64_t)blockIdx.x * SW_BLOCK + threadIdx.x; e < total; e += (int64_t)gridDim.x * SW_BLOCK) {
        const int c = (int)(e % C);
        int64_t r = e / C;
        const int j = (int)(r % Ho);
        r /= Ho;
        const int i = (int)(r % Ho);
        const int64_t b = r / Ho;
        const T* img = x + b * H * H * C;
        float acc = 0.0f;
#pragma unroll
        for (int dy = 0; dy < 5; ++dy) {
            const int yy = sw_mirror(2 * i + dy - 2, H);
#pragma unroll
            for (int dx = 0; dx < 5; ++dx) {
                const int xx = sw_mirror(2 * j + dx - 2, H);
                acc = fmaf(sw_f(dy) * sw_f(dx) * (1.0f / 256.0f), sw_widen(img[((int64_t)yy * H + xx) * C + c]), acc);
            }
        }
        y[e] = acc;
    }
}

template <typename T>
__global__ __launch_bounds__(SW_BLOCK) void swd_pyr_lap_kernel(const T* __restrict__ g, const float* __restrict__ g1,
                                                               float* __restrict__ y, int B, int H, int C) {
    const int Hc = H >> 1;
    const int64_t total = (int64_t)B * H * H * C;
    for (int64_t e = (int64_t)blockIdx.x * SW_BLOCK + threadIdx.x; e < total; e += (int64_t)gridDim.x * SW_BLOCK) {
        const int c = (int)(e % C);
        int64_t r = e / C;
        const int j = (int)(r % H);
        r /= H;
        const int i = (int)(r % H);
        const int64_t b = r / H;
        const float* coarse = g1 + b * Hc * Hc * C;
        float up = 0.0f;
#pragma unroll
        for (int dy = 0; dy < 5; ++dy) {
            const int yy = sw_mirror(i + dy - 2, H);
#pragma unroll
            for (int dx = 0; dx < 5; ++dx) {
                const int xx = sw_mirror(j + dx - 2, H);
                if (((yy | xx) & 1) == 0)          // the zero-stuffed image is non-zero on the even grid only
                    up = fmaf(sw_f(dy) * sw_f(dx) * (1.0f / 64.0f),
                              coarse[((int64_t)(yy >> 1) * Hc + (xx >> 1)) * C + c], up);
            }
        }
        y[e] = sw_widen(g[e]) - up;
    }
}

// ---------------------------------------------------------------------------------------------------- descriptors
// fixed-order block sum of a double over 256 threads (xor butterflies inside a wave, then the four waves in order)
__device__ __forceinline__ double sw_block_sum(double v, double* sh) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((sh[0] + sh[1]) + sh[2]) + sh[3];
}

// One block per image.  partials[(row_offset / 128 + b)][c][0..1] = sum, sum of squares of the image's values of channel c.
__global__ __launch_bounds__(SW_BLOCK) void swd_descriptors_kernel(const float* __restrict__ x, const int32_t* __restrict__ pos,
                                                                   int H, int C, float* __restrict__ desc,
                                                                   int64_t row_offset, double* __restrict__ partials) {
    __shared__ int cy[SW_PATCHES], cx[SW_PATCHES];
    __shared__ double red[4];
    const int b = blockIdx.x, t = threadIdx.x;
    const int K = SW_TAPS * C;
    if (t < SW_PATCHES) {
        const int py = pos[((int64_t)b * SW_PATCHES + t) * 2], px = pos[((int64_t)b * SW_PATCHES + t) * 2 + 1];
        const bool ok = py >= 3 && py <= H - 4 && px >= 3 && px <= H - 4;
        cy[t] = ok ? py : -1;          // a position that does not fit gives a zero row
        cx[t] = px;
    }
    __syncthreads();
    const float* img = x + (int64_t)b * H * H * C;
    float* rows = desc + (row_offset + (int64_t)b * SW_PATCHES) * K;
    double* part = partials + (row_offset / SW_PATCHES + b) * (int64_t)(2 * C);
    for (int c = 0; c < C; ++c) {
        double s = 0.0, ss = 0.0;
        for (int e = t; e < SW_PATCHES * SW_TAPS; e += SW_BLOCK) {
            const int p = e / SW_TAPS, tap = e - p * SW_TAPS;
            const int dy = tap / 7, dx = tap - dy * 7;
            float v = 0.0f;
            if (cy[p] >= 0) v = img[((int64_t)(cy[p] + dy - 3) * H + (cx[p] + dx - 3)) * C + c];
            rows[(int64_t)p * K + c * SW_TAPS + tap] = v;
            s += (double)v;
            ss += (double)v * (double)v;
        }
        s = sw_block_sum(s, red);
        ss = sw_block_sum(ss, red);
        if (t == 0) {
            part[2 * c] = s;
            part[2 * c + 1] = ss;
        }
    }
}

// stats[c] = (mean, 1 / biased deviation; 0 for a channel without deviation) over n_images * 128 * 49 values.
__global__ __launch_bounds__(SW_BLOCK) void swd_stats_finish_kernel(const double* __restrict__ partials, int n_images, int C,
                                                                    double* __restrict__ stats) {
    __shared__ double red[4];
    const double count = (double)n_images * (double)(SW_PATCHES * SW_TAPS);
    for (int c = 0; c < C; ++c) {
        double s = 0.0, ss = 0.0;
        for (int i = threadIdx.x; i < n_images; i += SW_BLOCK) {
            s += partials[(int64_t)i * 2 * C + 2 * c];
            ss += partials[(int64_t)i * 2 * C + 2 * c + 1];
        }
        s = sw_block_sum(s, red);
        ss = sw_block_sum(ss, red);
        if (threadIdx.x == 0) {
            const double mean = s / count;
            const double var = ss / count - mean * mean;
            stats[2 * c] = mean;
            stats[2 * c + 1] = var > 0.0 ? 1.0 / sqrt(var) : 0.0;
        }
    }
}

// ---------------------------------------------------------------------------------------------------- projection
#define SW_PN 64          // rows (n) of a block's output tile
#define SW_PS 64          // directions (s) of it
#define SW_PLD 68         // leading dimension of the transposed descriptor tile: 16-byte aligned rows

// One channel (49 values of k) per staging round, so the normalisation constants are scalars of the round.  A thread owns
// 4 n x 4 s outputs; n is the fast index of the output, so its four n go out as one 16-byte store.
__global__ __launch_bounds__(SW_BLOCK) void swd_project_kernel(const float* __restrict__ desc_a, const double* __restrict__ stats_a,
                                                               const float* __restrict__ desc_b, const double* __restrict__ stats_b,
                                                               const float* __restrict__ dirs, float* __restrict__ out,
                                                               int64_t N, int C, int S) {
    __shared__ __attribute__((aligned(16))) float A[SW_TAPS][SW_PLD];
    __shared__ __attribute__((aligned(16))) float D[SW_TAPS][SW_PS];
    const int set = blockIdx.z, t = threadIdx.x;
    const float* desc = set ? desc_b : desc_a;
    const double* stats = set ? stats_b : stats_a;
    const int64_t n0 = (int64_t)blockIdx.x * SW_PN;
    const int s0 = blockIdx.y * SW_PS;
    const int K = SW_TAPS * C;
    const int tn = t & 15, ts = t >> 4;
    float acc[4][4];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[j][i] = 0.0f;
    for (int c = 0; c < C; ++c) {
        const double mean = stats[2 * c], rstd = stats[2 * c + 1];
        __syncthreads();
        for (int e = t; e < SW_PN * SW_TAPS; e += SW_BLOCK) {
            const int nl = e / SW_TAPS, kk = e - nl * SW_TAPS;
            const float v = desc[(n0 + nl) * K + c * SW_TAPS + kk];
            A[kk][nl] = (float)(((double)v - mean) * rstd);
        }
        for (int e = t; e < SW_TAPS * SW_PS; e += SW_BLOCK) {
            const int kk = e / SW_PS, sl = e - kk * SW_PS;
            D[kk][sl] = (s0 + sl < S) ? dirs[(int64_t)(c * SW_TAPS + kk) * S + s0 + sl] : 0.0f;
        }
        __syncthreads();
#pragma unroll 7
        for (int kk = 0; kk < SW_TAPS; ++kk) {
            const float4 a4 = *reinterpret_cast<const float4*>(&A[kk][tn * 4]);
            const float4 d4 = *reinterpret_cast<const float4*>(&D[kk][ts * 4]);
            const float a[4] = {a4.x, a4.y, a4.z, a4.w}, d[4] = {d4.x, d4.y, d4.z, d4.w};
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int i = 0; i < 4; ++i) acc[j][i] = fmaf(a[i], d[j], acc[j][i]);
        }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int s = s0 + ts * 4 + j;
        if (s < S)
            *reinterpret_cast<float4*>(out + ((int64_t)set * S + s) * N + n0 + tn * 4) =
                make_float4(acc[j][0], acc[j][1], acc[j][2], acc[j][3]);
    }
}

// ---------------------------------------------------------------------------------------------------- sort
#define SW_TILE 4096
#define SW_SORT_THREADS 512

__device__ __forceinline__ int sw_phys(int i) { return i ^ (((i >> 6) & 3) << 3); }

__device__ __forceinline__ void sw_cmpx(float& a, float& b, bool asc) {
    const bool swap = asc ? (a > b) : (a < b);
    const float lo = swap ? b : a, hi = swap ? a : b;
    a = lo;
    b = hi;
}

// The exchange distances 4 JL, 2 JL, JL (those below k) of merge size k on the 8 elements base + r JL of this thread.
template <int JL>
__device__ __forceinline__ void sw_local_pass(float* sh, int t, int k, int64_t g0, int seg_mask) {
    const int base = (t / JL) * (8 * JL) + (t % JL);
    float v[8];
    if (JL == 1) {
        const float4 lo = *reinterpret_cast<const float4*>(sh + sw_phys(base));
        const float4 hi = *reinterpret_cast<const float4*>(sh + sw_phys(base) + 4);
        v[0] = lo.x; v[1] = lo.y; v[2] = lo.z; v[3] = lo.w;
        v[4] = hi.x; v[5] = hi.y; v[6] = hi.z; v[7] = hi.w;
    } else {
#pragma unroll
        for (int r = 0; r < 8; ++r) v[r] = sh[sw_phys(base + r * JL)];
    }
#pragma unroll
    for (int h = 4; h >= 1; h >>= 1) {
        if (h * JL < k) {
#pragma unroll
            for (int r = 0; r < 8; ++r) {
                if ((r & h) == 0) {
                    const bool asc = ((int)((g0 + base + r * JL) & seg_mask) & k) == 0;
                    sw_cmpx(v[r], v[r + h], asc);
                }
            }
        }
    }
    if (JL == 1) {
        *reinterpret_cast<float4*>(sh + sw_phys(base)) = make_float4(v[0], v[1], v[2], v[3]);
        *reinterpret_cast<float4*>(sh + sw_phys(base) + 4) = make_float4(v[4], v[5], v[6], v[7]);
    } else {
#pragma unroll
        for (int r = 0; r < 8; ++r) sh[sw_phys(base + r * JL)] = v[r];
    }
}

// Every exchange distance below a tile of the merge sizes k_first .. k_last (powers of two, k_first <= k_last), on one
// tile per block.  total is the number of floats of all segments; a last, partial tile (segments shorter than a tile
// only) is padded with +inf, which stays in segments of its own.
__global__ __launch_bounds__(SW_SORT_THREADS) void swd_sort_tile_kernel(float* __restrict__ data, int64_t total, int seg_mask,
                                                                        int k_first, int k_last, int vec) {
    __shared__ __attribute__((aligned(16))) float sh[SW_TILE];
    const int t = threadIdx.x;
    const int64_t g0 = (int64_t)blockIdx.x * SW_TILE;
    const bool full = vec && g0 + SW_TILE <= total;
    if (full) {
#pragma unroll
        for (int q = 0; q < SW_TILE / (4 * SW_SORT_THREADS); ++q) {
            const int i = (q * SW_SORT_THREADS + t) * 4;
            *reinterpret_cast<float4*>(sh + sw_phys(i)) = *reinterpret_cast<const float4*>(data + g0 + i);
        }
    } else {
        for (int i = t; i < SW_TILE; i += SW_SORT_THREADS) sh[sw_phys(i)] = g0 + i < total ? data[g0 + i] : INFINITY;
    }
    __syncthreads();
    for (int k = k_first; k <= k_last && k > 0; k <<= 1) {
        if (k > 512) {
            sw_local_pass<512>(sh, t, k, g0, seg_mask);
            __syncthreads();
        }
        if (k > 64) {
            sw_local_pass<64>(sh, t, k, g0, seg_mask);
            __syncthreads();
        }
        if (k > 8) {
            sw_local_pass<8>(sh, t, k, g0, seg_mask);
            __syncthreads();
        }
        sw_local_pass<1>(sh, t, k, g0, seg_mask);
        __syncthreads();
    }
    if (full) {
#pragma unroll
        for (int q = 0; q < SW_TILE / (4 * SW_SORT_THREADS); ++q) {
            const int i = (q * SW_SORT_THREADS + t) * 4;
            *reinterpret_cast<float4*>(data + g0 + i) = *reinterpret_cast<const float4*>(sh + sw_phys(i));
        }
    } else {
        for (int i = t; i < SW_TILE; i += SW_SORT_THREADS)
            if (g0 + i < total) data[g0 + i] = sh[sw_phys(i)];
    }
}

// The NS exchange distances jl << (NS-1) .. jl (jl >= SW_TILE) of merge size k, one sweep over the data: a thread holds
// E = 2^NS float4 at distance jl.  total is a multiple of E * jl.
template <int NS>
__global__ __launch_bounds__(SW_BLOCK) void swd_sort_global_kernel(float* __restrict__ data, int64_t total, int seg_mask,
                                                                   int k, int jl) {
    constexpr int E = 1 << NS;
    const int64_t work = total / (4 * E);
    for (int64_t w = (int64_t)blockIdx.x * SW_BLOCK + threadIdx.x; w < work; w += (int64_t)gridDim.x * SW_BLOCK) {
        const int64_t w4 = w * 4;
        const int64_t base = (w4 / jl) * ((int64_t)E * jl) + (w4 % jl);
        float4 v[E];
#pragma unroll
        for (int e = 0; e < E; ++e) v[e] = *reinterpret_cast<const float4*>(data + base + (int64_t)e * jl);
#pragma unroll
        for (int h = E / 2; h >= 1; h >>= 1) {
#pragma unroll
            for (int e = 0; e < E; ++e) {
                if ((e & h) == 0) {
                    const bool asc = ((int)((base + (int64_t)e * jl) & seg_mask) & k) == 0;
                    sw_cmpx(v[e].x, v[e + h].x, asc);
                    sw_cmpx(v[e].y, v[e + h].y, asc);
                    sw_cmpx(v[e].z, v[e + h].z, asc);
                    sw_cmpx(v[e].w, v[e + h].w, asc);
                }
            }
        }
#pragma unroll
        for (int e = 0; e < E; ++e) *reinterpret_cast<float4*>(data + base + (int64_t)e * jl) = v[e];
    }
}

// ---------------------------------------------------------------------------------------------------- L1
#define SW_L1_CHUNK 4096
#define SW_L1_MAX_BLOCKS 1024

static inline int sw_l1_blocks(int64_t n_per_out) {
    int64_t b = (n_per_out + SW_L1_CHUNK - 1) / SW_L1_CHUNK;
    if (b > SW_L1_MAX_BLOCKS) b = SW_L1_MAX_BLOCKS;
    if (b < 1) b = 1;
    return (int)b;
}

// grid (blocks, n_out): ws[out][block] = the block's share of sum |a - b| over elements [out * n, (out + 1) * n)
template <int VEC>
__global__ __launch_bounds__(SW_BLOCK) void swd_l1_partial_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                                  int64_t n, double* __restrict__ ws) {
    __shared__ double red[4];
    const float* pa = a + (int64_t)blockIdx.y * n;
    const float* pb = b + (int64_t)blockIdx.y * n;
    double s = 0.0;
    const int64_t items = n / VEC;
    for (int64_t i = (int64_t)blockIdx.x * SW_BLOCK + threadIdx.x; i < items; i += (int64_t)gridDim.x * SW_BLOCK) {
        if (VEC == 4) {
            const float4 u = *reinterpret_cast<const float4*>(pa + i * 4), v = *reinterpret_cast<const float4*>(pb + i * 4);
            s += fabs((double)u.x - (double)v.x);
            s += fabs((double)u.y - (double)v.y);
            s += fabs((double)u.z - (double)v.z);
            s += fabs((double)u.w - (double)v.w);
        } else {
            s += fabs((double)pa[i] - (double)pb[i]);
        }
    }
    s = sw_block_sum(s, red);
    if (threadIdx.x == 0) ws[(int64_t)blockIdx.y * gridDim.x + blockIdx.x] = s;
}

__global__ __launch_bounds__(SW_BLOCK) void swd_l1_finish_kernel(const double* __restrict__ ws, int blocks,
                                                                 double* __restrict__ out) {
    __shared__ double red[4];
    double s = 0.0;
    for (int i = threadIdx.x; i < blocks; i += SW_BLOCK) s += ws[(int64_t)blockIdx.x * blocks + i];
    s = sw_block_sum(s, red);
    if (threadIdx.x == 0) out[blockIdx.x] = s;
}

static inline int sw_grid(int64_t work) {
    int64_t b = (work + SW_BLOCK - 1) / SW_BLOCK;
    if (b > 65536) b = 65536;
    if (b < 1) b = 1;
    return (int)b;
}

static inline bool sw_pow2(int64_t v) { return v > 0 && (v & (v - 1)) == 0; }

}  // namespace bg

using namespace bg;

extern "C" {

int bg_swd_pyr_down(const void* x, int x_dtype, float* y, int B, int H, int C, void* stream) {
    BG_REQUIRE(x && y, "bg_swd_pyr_down: NULL pointer");
    BG_REQUIRE(x_dtype == BG_F32 || x_dtype == BG_BF16, "bg_swd_pyr_down: x_dtype=%d (BG_F32 or BG_BF16)", x_dtype);
    BG_REQUIRE(B > 0 && (C == 1 || C == 3 || C == 4), "bg_swd_pyr_down: B=%d C=%d (C is 1, 3 or 4)", B, C);
    BG_REQUIRE(H >= 32 && H <= 16384 && sw_pow2(H), "bg_swd_pyr_down: H=%d (a power of two >= 32)", H);
    const int64_t total = (int64_t)B * (H / 2) * (H / 2) * C;
    if (x_dtype == BG_F32)
        hipLaunchKernelGGL(swd_pyr_down_kernel<float>, dim3(sw_grid(total)), dim3(SW_BLOCK), 0, as_stream(stream),
                           static_cast<const float*>(x), y, B, H, C);
    else
        hipLaunchKernelGGL(swd_pyr_down_kernel<uint16_t>, dim3(sw_grid(total)), dim3(SW_BLOCK), 0, as_stream(stream),
                           static_cast<const uint16_t*>(x), y, B, H, C);
    BG_LAUNCH_CHECK();
    return BG_OK;
}

int bg_swd_pyr_lap(const void* g, int g_dtype, const float* g1, float* y, int B, int H, int C, void* stream) {
    BG_REQUIRE(g && g1 && y, "bg_swd_pyr_lap: NULL pointer");
    BG_REQUIRE(g_dtype == BG_F32 || g_dtype == BG_BF16, "bg_swd_pyr_lap: g_dtype=%d (BG_F32 or BG_BF16)", g_dtype);
    BG_REQUIRE(B > 0 && (C == 1 || C == 3 || C == 4), "bg_swd_pyr_lap: B=%d C=%d (C is 1, 3 or 4)", B, C);
    BG_REQUIRE(H >= 32 && H <= 16384 && sw_pow2(H), "bg_swd_pyr_lap: H=%d (a power of two >= 32)", H);
    const int64_t total = (int64_t)B * H * H * C;
    if (g_dtype == BG_F32)
        hipLaunchKernelGGL(swd_pyr_lap_kernel<float>, dim3(sw_grid(total)), dim3(SW_BLOCK), 0, as_stream(stream),
                           static_cast<const float*>(g), g1, y, B, H, C);
    else
        hipLaunchKernelGGL(swd_pyr_lap_kernel<uint16_t>, dim3(sw_grid(total)), dim3(SW_BLOCK), 0, as_stream(stream),
                           static_cast<const uint16_t*>(g), g1, y, B, H, C);
    BG_LAUNCH_CHECK();
    return BG_OK;
}

size_t bg_swd_stats_workspace_bytes(int n_images, int C) {
    if (n_images < 1 || C < 1) return 0;
    return (size_t)n_images * 2 * (size_t)C * sizeof(double);
}

int bg_swd_descriptors(const float* x, const int32_t* pos, int B, int H, int C, float* desc, int64_t n_rows,
                       int64_t row_offset, double* partials, size_t partials_bytes, void* stream) {
    BG_REQUIRE(x && pos && desc && partials, "bg_swd_descriptors: NULL pointer");
    BG_REQUIRE(B > 0 && B <= 65535 && (C == 1 || C == 3 || C == 4), "bg_swd_descriptors: B=%d C=%d (C is 1, 3 or 4)", B, C);
    BG_REQUIRE(H >= 8 && H <= 16384, "bg_swd_descriptors: H=%d (8..16384)", H);
    BG_REQUIRE(n_rows > 0 && n_rows % SW_PATCHES == 0 && row_offset >= 0 && row_offset % SW_PATCHES == 0 &&
                   row_offset + (int64_t)B * SW_PATCHES <= n_rows,
               "bg_swd_descriptors: rows %lld + %d x 128 do not fit the %lld rows of the buffer (multiples of 128)",
               (long long)row_offset, B, (long long)n_rows);
    BG_REQUIRE(partials_bytes >= bg_swd_stats_workspace_bytes((int)(n_rows / SW_PATCHES), C) &&
                   ((uintptr_t)partials & 7) == 0,
               "bg_swd_descriptors: partials of %zu bytes, bg_swd_stats_workspace_bytes(%lld, %d) needed, 8-byte aligned",
               partials_bytes, (long long)(n_rows / SW_PATCHES), C);
    hipLaunchKernelGGL(swd_descriptors_kernel, dim3(B), dim3(SW_BLOCK), 0, as_stream(stream), x, pos, H, C, desc, row_offset,
                       partials);
    BG_LAUNCH_CHECK();
    return BG_OK;
}

int bg_swd_stats_finish(const double* partials, size_t partials_bytes, int n_images, int C, double* stats, void* stream) {
    BG_REQUIRE(partials && stats, "bg_swd_stats_finish: NULL pointer");
    BG_REQUIRE(n_images > 0 && (C == 1 || C == 3 || C == 4), "bg_swd_stats_finish: n_images=%d C=%d", n_images, C);
    BG_REQUIRE(partials_bytes >= bg_swd_stats_workspace_bytes(n_images, C) && ((uintptr_t)partials & 7) == 0 &&
                   ((uintptr_t)stats & 7) == 0,
               "bg_swd_stats_finish: partials of %zu bytes, bg_swd_stats_workspace_bytes(%d, %d) needed, 8-byte aligned",
               partials_bytes, n_images, C);
    hipLaunchKernelGGL(swd_stats_finish_kernel, dim3(1), dim3(SW_BLOCK), 0, as_stream(stream), partials, n_images, C, stats);
    BG_LAUNCH_CHECK();
    return BG_OK;
}

int bg_swd_project(const float* desc_a, const double* stats_a, const float* desc_b, const double* stats_b, const float* dirs,
                   float* out, int64_t N, int C, int S, void* stream) {
    BG_REQUIRE(desc_a && stats_a && dirs && out, "bg_swd_project: NULL pointer");
    BG_REQUIRE((desc_b == nullptr) == (stats_b == nullptr), "bg_swd_project: the second set needs desc_b and stats_b");
    BG_REQUIRE(C == 1 || C == 3 || C == 4, "bg_swd_project: C=%d (1, 3 or 4)", C);
    BG_REQUIRE(N > 0 && N % SW_PN == 0 && N / SW_PN <= 0x7fffffffLL, "bg_swd_project: N=%lld (a multiple of %d)",
               (long long)N, SW_PN);
    BG_REQUIRE(S > 0 && S <= 65535 * SW_PS, "bg_swd_project: S=%d", S);
    BG_REQUIRE(((uintptr_t)out & 15) == 0 && ((uintptr_t)stats_a & 7) == 0 && ((uintptr_t)stats_b & 7) == 0,
               "bg_swd_project: out must be 16-byte and the statistics 8-byte aligned");
    hipLaunchKernelGGL(swd_project_kernel, dim3((unsigned)(N / SW_PN), (S + SW_PS - 1) / SW_PS, desc_b ? 2 : 1),
                       dim3(SW_BLOCK), 0, as_stream(stream), desc_a, stats_a, desc_b, stats_b, dirs, out, N, C, S);
    BG_LAUNCH_CHECK();
    return BG_OK;
}

size_t bg_swd_sort_tile(void) { return SW_TILE; }

int bg_swd_sort_segments(float* data, int n_seg, int seg_len, void* stream) {
    BG_REQUIRE(data, "bg_swd_sort_segments: NULL pointer");
    BG_REQUIRE(n_seg > 0, "bg_swd_sort_segments: n_seg=%d", n_seg);
    BG_REQUIRE(seg_len >= 2 && seg_len <= (1 << 24) && sw_pow2(seg_len),
               "bg_swd_sort_segments: seg_len=%d (a power of two from 2 to 2^24)", seg_len);
    BG_REQUIRE(((uintptr_t)data & 3) == 0, "bg_swd_sort_segments: data must be 4-byte aligned");
    const int64_t total = (int64_t)n_seg * seg_len;
    const int64_t tiles = (total + SW_TILE - 1) / SW_TILE;
    BG_REQUIRE(tiles <= 0x7fffffffLL, "bg_swd_sort_segments: %lld floats are too many", (long long)total);
    const int vec = ((uintptr_t)data & 15) == 0;
    BG_REQUIRE(vec || seg_len < SW_TILE, "bg_swd_sort_segments: segments of a tile (%d) or more need 16-byte aligned data",
               SW_TILE);
    hipStream_t s = as_stream(stream);
    const int seg_mask = seg_len - 1;
    hipLaunchKernelGGL(swd_sort_tile_kernel, dim3((unsigned)tiles), dim3(SW_SORT_THREADS), 0, s, data, total, seg_mask, 2,
                       seg_len < SW_TILE ? seg_len : SW_TILE, vec);
    for (int64_t k = 2 * SW_TILE; k <= seg_len; k <<= 1) {
        int64_t j = k >> 1;                              // the largest distance still to run
        while (j >= SW_TILE) {
            int ns = 1;
            while (ns < 3 && (j >> ns) >= SW_TILE) ++ns;
            const int jl = (int)(j >> (ns - 1));
            const int grid = sw_grid(total / (4 << ns));
            if (ns == 3)
                hipLaunchKernelGGL(swd_sort_global_kernel<3>, dim3(grid), dim3(SW_BLOCK), 0, s, data, total, seg_mask, (int)k, jl);
            else if (ns == 2)
                hipLaunchKernelGGL(swd_sort_global_kernel<2>, dim3(grid), dim3(SW_BLOCK), 0, s, data, total, seg_mask, (int)k, jl);
            else
                hipLaunchKernelGGL(swd_sort_global_kernel<1>, dim3(grid), dim3(SW_BLOCK), 0, s, data, total, seg_mask, (int)k, jl);
            j = jl >> 1;
        }
        hipLaunchKernelGGL(swd_sort_tile_kernel, dim3((unsigned)tiles), dim3(SW_SORT_THREADS), 0, s, data, total, seg_mask,
                           (int)k, (int)k, vec);
    }
    BG_LAUNCH_CHECK();
    return BG_OK;
}

size_t bg_swd_l1_workspace_bytes(int64_t n_per_out, int n_out) {
    if (n_per_out < 1 || n_out < 1) return 0;
    return (size_t)n_out * (size_t)sw_l1_blocks(n_per_out) * sizeof(double);
}

int bg_swd_l1(const float* a, const float* b, int64_t n_per_out, int n_out, double* out, void* ws, size_t ws_bytes,
              void* stream) {
    BG_REQUIRE(a && b && out && ws, "bg_swd_l1: NULL pointer");
    BG_REQUIRE(n_per_out > 0 && n_out > 0 && n_out <= 65535, "bg_swd_l1: n_per_out=%lld n_out=%d", (long long)n_per_out,
               n_out);
    BG_REQUIRE(ws_bytes >= bg_swd_l1_workspace_bytes(n_per_out, n_out) && ((uintptr_t)ws & 7) == 0 && ((uintptr_t)out & 7) == 0,
               "bg_swd_l1: workspace of %zu bytes, %zu needed, 8-byte aligned", ws_bytes,
               bg_swd_l1_workspace_bytes(n_per_out, n_out));
    const int blocks = sw_l1_blocks(n_per_out);
    const bool vec = (n_per_out & 3) == 0 && (((uintptr_t)a | (uintptr_t)b) & 15) == 0;
    if (vec)
        hipLaunchKernelGGL(swd_l1_partial_kernel<4>, dim3(blocks, n_out), dim3(SW_BLOCK), 0, as_stream(stream), a, b, n_per_out,
                           static_cast<double*>(ws));
    else
        hipLaunchKernelGGL(swd_l1_partial_kernel<1>, dim3(blocks, n_out), dim3(SW_BLOCK), 0, as_stream(stream), a, b, n_per_out,
                           static_cast<double*>(ws));
    hipLaunchKernelGGL(swd_l1_finish_kernel, dim3(n_out), dim3(SW_BLOCK), 0, as_stream(stream), static_cast<const double*>(ws),
                       blocks, out);
    BG_LAUNCH_CHECK();
    return BG_OK;
}

}  // extern "C"
