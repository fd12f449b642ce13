// msssim.hip - multi-scale structural similarity (Wang, Simoncelli and Bovik 2003) of image pairs: the in-training
// diversity score of metrics.py (Odena et al. 2017 use it per class).  NHWC images in [-1, 1], H = W a power of two >= 16,
// C in {1, 3, 4}; DESIGN.md gives the definition, tests/msssim_ref.py restates it in float64.
//
//   level    one launch per pyramid level: every image of both sets is read once; out go the per-(pair, tile, channel)
//            sums of cs and ssim over the tile's window positions in fp64 and, unless the level is the last, the 2 x 2
//            means of both images (the next level's input, fp32)
//   finish   adds the tiles of every level in index order, divides by the (side - 10)^2 positions, clamps at 0, raises to
//            the level weights, multiplies over levels, averages over channels: one fp64 score per pair
//
// Every reduction goes through partial rows that the finish launch adds in index order: no float atomics, so a repeated
// launch is bit-identical.
//
// The level kernel.  A block of 256 threads owns MS_T x MS_T = 16 x 16 window positions of one pair, so it needs a
// 26 x 26 pixel tile (10-pixel apron of the 11-tap window) of both images.  H is a multiple of 16 and H - 10 = 16 k + 6, so
// there are (H / 16)^2 tiles, the last one of a row or column holds 6 positions, its tile is cut at the image edge (the
// rest is zero and feeds no valid position), and the top-left 16 x 16 pixels of every tile partition the image: the block
// pools exactly those, 8 x 8 outputs per image and channel.  16 was chosen over 32 because the moment rows would grow to
// 27 KiB and the tile to 56 KiB at C = 4 (one block per CU), and because a 16 or 32 px level would leave most of a 32-wide
// block idle; the price is that a pixel is staged into LDS (26 / 16)^2 = 2.6 times, out of L2 after its first read.
//
// LDS per block: the tile, 2 images x C planes of 26 rows x 27 floats (plane stride 702, 715, 712 floats for C = 1, 3, 4),
// and the five moment rows of ONE channel, 5 x 16 columns x 26 floats = 8320 B; the channels take turns.  With the 32 B of
// the block sum: 13968 B (C = 1), 25520 B (C = 3), 31136 B (C = 4), i.e. 8 (wave cap), 6 and 5 blocks per CU.
//
// Banks (ds_read_b32 / ds_write_b32: 32 banks of 4 B, lanes 0-31 and 32-63 served separately):
//   staging     lanes run along a pixel row's C-interleaved floats; the plane strides are 11 (C = 3) and 8 (C = 4) mod 32, so
//               the 32 floats of a lane group, 11 or 8 pixels of every channel, fall on 32 different banks
//   horizontal  a lane group is the 26 rows (6 lanes idle) of one output column: word row * 27 + x + tap, 27 is odd, so
//               the rows sit on different banks; the five results go to M[m][x][row], consecutive words
//   vertical    a lane group is 16 positions y of column x and 16 of column x + 8: words x * 26 + y + tap and
//               (x + 8) * 26 + y + tap, 208 = 16 mod 32 apart, so the two runs of 16 consecutive words cover all 32 banks once
// All three are conflict-free.
#include <cmath>

#include "common.h"

namespace bg {

#define MS_BLOCK 256
#define MS_T 16                     // window positions per tile side
#define MS_TAPS 11
#define MS_IN (MS_T + MS_TAPS - 1)  // 26: pixels per tile side
#define MS_RS 27                    // row stride of a tile plane (odd)
#define MS_MAX_LEVELS 5

struct MsWindow {
    float g[MS_TAPS];
};

__device__ __forceinline__ float ms_widen(float v) { return v; }
__device__ __forceinline__ float ms_widen(uint16_t bits) { return __uint_as_float((uint32_t)bits << 16); }   // bf16, exact

template <int C>
struct MsPlane {
    static constexpr int stride = MS_IN * MS_RS + (C == 3 ? 13 : (C == 4 ? 10 : 0));   // 702, 715, 712
};

// fixed-order block sum of a double over 256 threads (xor butterflies inside a wave, then the four waves in order)
__device__ __forceinline__ double ms_block_sum(double v, double* sh) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((sh[0] + sh[1]) + sh[2]) + sh[3];
}

// grid (tiles, P).  a, b: the level's images, pair p at p * pair_stride images; pool_a, pool_b: fp32 [P, H/2, H/2, C] or
// NULL; part: fp64 [P][tiles][C][2] = (sum of cs, sum of ssim).
template <typename T, int C>
__global__ __launch_bounds__(MS_BLOCK) void msssim_level_kernel(const T* __restrict__ a, const T* __restrict__ b,
                                                                int64_t pair_stride, int H, MsWindow win,
                                                                float* __restrict__ pool_a, float* __restrict__ pool_b,
                                                                double* __restrict__ part) {
    constexpr int PS = MsPlane<C>::stride;
    __shared__ float tile[2][C * PS];
    __shared__ float mom[5][MS_T * MS_IN];
    __shared__ double red[4];
    const int t = threadIdx.x;
    const int nt = H / MS_T;
    const int ty = blockIdx.x / nt, tx = blockIdx.x - ty * nt;
    const int y0 = ty * MS_T, x0 = tx * MS_T;
    const int64_t p = blockIdx.y;
    const int64_t img_elems = (int64_t)H * H * C;

    // ---- stage both tiles (raw values; what lies past the image edge is zero)
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const T* img = (s ? b : a) + p * pair_stride * img_elems;
        for (int e = t; e < MS_IN * MS_IN * C; e += MS_BLOCK) {
            const int row = e / (MS_IN * C), j = e - row * (MS_IN * C);
            const int col = j / C, c = j - col * C;
            const int gy = y0 + row, gx = x0 + col;
            float v = 0.0f;
            if (gy < H && gx < H) v = ms_widen(img[((int64_t)gy * H + gx) * C + c]);
            tile[s][c * PS + row * MS_RS + col] = v;
        }
    }
    __syncthreads();

    // ---- the next level: 2 x 2 means of the tile's first 16 x 16 pixels, three additions and an exact scaling
    if (pool_a != nullptr) {
        const int h2 = H >> 1;
        for (int e = t; e < 2 * 64 * C; e += MS_BLOCK) {
            const int s = e / (64 * C), r = e - s * (64 * C);
            const int py = r / (8 * C), q = r - py * (8 * C);
            const int px = q / C, c = q - px * C;
            const float* src = &tile[s][c * PS + (2 * py) * MS_RS + 2 * px];
            const float v = ((src[0] + src[1]) + (src[MS_RS] + src[MS_RS + 1])) * 0.25f;
            float* dst = s ? pool_b : pool_a;
            dst[((p * h2 + (y0 / 2 + py)) * h2 + (x0 / 2 + px)) * C + c] = v;
        }
    }

    const int vy = t & 15, vx = (t >> 5) + 8 * ((t >> 4) & 1);
    const bool valid = (y0 + vy < H - (MS_TAPS - 1)) && (x0 + vx < H - (MS_TAPS - 1));
    const float C1 = 0.01f * 0.01f, C2 = 0.03f * 0.03f;
    double* out = part + ((p * gridDim.x + blockIdx.x) * C) * 2;

    for (int c = 0; c < C; ++c) {
        // ---- horizontal pass: the five moment rows of channel c, u = (x + 1) / 2
#pragma unroll
        for (int it = 0; it < 2; ++it) {
            const int i = t + it * MS_BLOCK;
            const int row = i & 31, x = i >> 5;
            if (row < MS_IN) {
                const float* ra = &tile[0][c * PS + row * MS_RS + x];
                const float* rb = &tile[1][c * PS + row * MS_RS + x];
                float m0 = 0.0f, m1 = 0.0f, m2 = 0.0f, m3 = 0.0f, m4 = 0.0f;
#pragma unroll
                for (int k = 0; k < MS_TAPS; ++k) {
                    const float ua = fmaf(ra[k], 0.5f, 0.5f), ub = fmaf(rb[k], 0.5f, 0.5f);
                    const float g = win.g[k];
                    m0 = fmaf(g, ua, m0);
                    m1 = fmaf(g, ub, m1);
                    m2 = fmaf(g, ua * ua, m2);
                    m3 = fmaf(g, ub * ub, m3);
                    m4 = fmaf(g, ua * ub, m4);
                }
                const int o = x * MS_IN + row;
                mom[0][o] = m0;
                mom[1][o] = m1;
                mom[2][o] = m2;
                mom[3][o] = m3;
                mom[4][o] = m4;
            }
        }
        __syncthreads();
        // ---- vertical pass and the cs / ssim arithmetic of one window position
        float acc[5];
#pragma unroll
        for (int m = 0; m < 5; ++m) {
            const float* col = &mom[m][vx * MS_IN + vy];
            float s = 0.0f;
#pragma unroll
            for (int k = 0; k < MS_TAPS; ++k) s = fmaf(win.g[k], col[k], s);
            acc[m] = s;
        }
        const float mua = acc[0], mub = acc[1];
        const float va = acc[2] - mua * mua, vb = acc[3] - mub * mub, cab = acc[4] - mua * mub;
        const float cs = (2.0f * cab + C2) / (va + vb + C2);
        const float l = (2.0f * mua * mub + C1) / (mua * mua + mub * mub + C1);
        const double s_cs = ms_block_sum(valid ? (double)cs : 0.0, red);
        const double s_ss = ms_block_sum(valid ? (double)(l * cs) : 0.0, red);   // (its barriers also release mom)
        if (t == 0) {
            out[2 * c] = s_cs;
            out[2 * c + 1] = s_ss;
        }
    }
}

struct MsPlan {
    int levels;
    int side[MS_MAX_LEVELS];
    int64_t tiles[MS_MAX_LEVELS];      // per pair
    int64_t offset[MS_MAX_LEVELS];     // of the level's partials, in tiles per pair, before it
    int64_t total_tiles;               // per pair, all levels
    double weight[MS_MAX_LEVELS];
};

// One block of 64 threads per pair: thread (level, c, which) adds its tiles in index order; thread 0 combines.
__global__ __launch_bounds__(64) void msssim_finish_kernel(const double* __restrict__ part, int P, int C, MsPlan plan,
                                                           double* __restrict__ scores) {
    __shared__ double mean[MS_MAX_LEVELS * 4 * 2];
    const int t = threadIdx.x;
    const int64_t p = blockIdx.x;
    if (t < plan.levels * C * 2) {
        const int level = t / (2 * C), r = t - level * (2 * C);
        const double* src = part + (plan.offset[level] * P + p * plan.tiles[level]) * (2 * C) + r;
        double s = 0.0;
        for (int64_t i = 0; i < plan.tiles[level]; ++i) s += src[i * (2 * C)];
        const double n = (double)(plan.side[level] - (MS_TAPS - 1));
        mean[t] = s / (n * n);
    }
    __syncthreads();
    if (t == 0) {
        double total = 0.0;
        for (int c = 0; c < C; ++c) {
            double prod = 1.0;
            for (int level = 0; level < plan.levels; ++level) {
                const double m = mean[(level * C + c) * 2 + (level + 1 == plan.levels ? 1 : 0)];
                prod *= pow(m > 0.0 ? m : 0.0, plan.weight[level]);
            }
            total += prod;
        }
        scores[p] = total / (double)C;
    }
}

static inline bool ms_side_ok(int H) { return H >= 16 && H <= 16384 && (H & (H - 1)) == 0; }

static inline MsPlan ms_plan(int H) {
    static const double W5[MS_MAX_LEVELS] = {0.0448, 0.2856, 0.3001, 0.2363, 0.1333};
    MsPlan pl;
    int log2 = 0;
    while ((1 << log2) < H) ++log2;
    pl.levels = log2 - 3 < MS_MAX_LEVELS ? log2 - 3 : MS_MAX_LEVELS;
    double wsum = 0.0;
    for (int i = 0; i < pl.levels; ++i) wsum += W5[i];
    int64_t off = 0;
    for (int i = 0; i < MS_MAX_LEVELS; ++i) {
        const bool live = i < pl.levels;
        pl.side[i] = live ? H >> i : 0;
        pl.tiles[i] = live ? (int64_t)(pl.side[i] / MS_T) * (pl.side[i] / MS_T) : 0;
        pl.offset[i] = off;
        pl.weight[i] = live ? W5[i] / wsum : 0.0;
        off += pl.tiles[i];
    }
    pl.total_tiles = off;
    return pl;
}

static inline MsWindow ms_window() {
    double g[MS_TAPS], sum = 0.0;
    for (int k = 0; k < MS_TAPS; ++k) {
        const double d = (double)(k - MS_TAPS / 2);
        g[k] = std::exp(-d * d / (2.0 * 1.5 * 1.5));
        sum += g[k];
    }
    MsWindow w;
    for (int k = 0; k < MS_TAPS; ++k) w.g[k] = (float)(g[k] / sum);
    return w;
}

template <typename T>
static void ms_launch_level(int C, dim3 grid, hipStream_t s, const T* a, const T* b, int64_t pair_stride, int h, float* pool_a,
                            float* pool_b, double* part) {
    const MsWindow w = ms_window();
    if (C == 1)
        hipLaunchKernelGGL((msssim_level_kernel<T, 1>), grid, dim3(MS_BLOCK), 0, s, a, b, pair_stride, h, w, pool_a, pool_b, part);
    else if (C == 3)
        hipLaunchKernelGGL((msssim_level_kernel<T, 3>), grid, dim3(MS_BLOCK), 0, s, a, b, pair_stride, h, w, pool_a, pool_b, part);
    else
        hipLaunchKernelGGL((msssim_level_kernel<T, 4>), grid, dim3(MS_BLOCK), 0, s, a, b, pair_stride, h, w, pool_a, pool_b, part);
}

}  // namespace bg

using namespace bg;

extern "C" {

size_t bg_msssim_workspace_bytes(int P, int H, int C) {
    if (P < 1 || !ms_side_ok(H) || !(C == 1 || C == 3 || C == 4)) return 0;
    return (size_t)P * (size_t)ms_plan(H).total_tiles * (size_t)C * 2 * sizeof(double);
}

int bg_msssim_level(const void* a, const void* b, int dtype, int64_t pair_stride, int P, int H, int level, int C,
                    float* pool_a, float* pool_b, double* ws, size_t ws_bytes, void* stream) {
    BG_REQUIRE(a && b && ws, "bg_msssim_level: NULL pointer");
    BG_REQUIRE(dtype == BG_F32 || dtype == BG_BF16, "bg_msssim_level: dtype=%d (BG_F32 or BG_BF16)", dtype);
    BG_REQUIRE(ms_side_ok(H), "bg_msssim_level: H=%d (a power of two from 16 to 16384)", H);
    BG_REQUIRE(C == 1 || C == 3 || C == 4, "bg_msssim_level: C=%d (1, 3 or 4)", C);
    BG_REQUIRE(P > 0 && P <= 65535, "bg_msssim_level: P=%d (1..65535 pairs a launch)", P);
    BG_REQUIRE(pair_stride >= 1, "bg_msssim_level: pair_stride=%lld (images from one pair to the next, >= 1)",
               (long long)pair_stride);
    const MsPlan pl = ms_plan(H);
    BG_REQUIRE(level >= 0 && level < pl.levels, "bg_msssim_level: level=%d, H=%d has %d levels", level, H, pl.levels);
    BG_REQUIRE(level == 0 || dtype == BG_F32, "bg_msssim_level: level %d reads the fp32 images of the level above", level);
    const bool last = level + 1 == pl.levels;
    BG_REQUIRE(last || (pool_a && pool_b), "bg_msssim_level: level %d of %d needs pool_a and pool_b", level, pl.levels);
    BG_REQUIRE(last || ((((uintptr_t)pool_a | (uintptr_t)pool_b) & 3) == 0), "bg_msssim_level: pooled outputs must be 4-byte aligned");
    BG_REQUIRE(ws_bytes >= bg_msssim_workspace_bytes(P, H, C) && ((uintptr_t)ws & 7) == 0,
               "bg_msssim_level: workspace of %zu bytes, bg_msssim_workspace_bytes(%d, %d, %d) = %zu needed, 8-byte aligned",
               ws_bytes, P, H, C, bg_msssim_workspace_bytes(P, H, C));
    const int h = pl.side[level];
    double* part = ws + pl.offset[level] * (int64_t)P * (2 * C);
    float* pa = last ? nullptr : pool_a;
    float* pb = last ? nullptr : pool_b;
    const dim3 grid((unsigned)pl.tiles[level], (unsigned)P);
    if (dtype == BG_F32)
        ms_launch_level<float>(C, grid, as_stream(stream), static_cast<const float*>(a), static_cast<const float*>(b),
                               pair_stride, h, pa, pb, part);
    else
        ms_launch_level<uint16_t>(C, grid, as_stream(stream), static_cast<const uint16_t*>(a), static_cast<const uint16_t*>(b),
                                  pair_stride, h, pa, pb, part);
    BG_LAUNCH_CHECK();
    return BG_OK;
}

int bg_msssim_finish(const double* ws, size_t ws_bytes, int P, int H, int C, double* scores, int64_t n_scores,
                     int64_t row_offset, void* stream) {
    BG_REQUIRE(ws && scores, "bg_msssim_finish: NULL pointer");
    BG_REQUIRE(ms_side_ok(H), "bg_msssim_finish: H=%d (a power of two from 16 to 16384)", H);
    BG_REQUIRE(C == 1 || C == 3 || C == 4, "bg_msssim_finish: C=%d (1, 3 or 4)", C);
    BG_REQUIRE(P > 0 && P <= 65535, "bg_msssim_finish: P=%d (1..65535 pairs a launch)", P);
    BG_REQUIRE(row_offset >= 0 && n_scores > 0 && row_offset + P <= n_scores,
               "bg_msssim_finish: rows %lld + %d do not fit the %lld scores", (long long)row_offset, P, (long long)n_scores);
    BG_REQUIRE(ws_bytes >= bg_msssim_workspace_bytes(P, H, C) && ((uintptr_t)ws & 7) == 0 && ((uintptr_t)scores & 7) == 0,
               "bg_msssim_finish: workspace of %zu bytes, bg_msssim_workspace_bytes(%d, %d, %d) = %zu needed, 8-byte aligned",
               ws_bytes, P, H, C, bg_msssim_workspace_bytes(P, H, C));
    hipLaunchKernelGGL(msssim_finish_kernel, dim3((unsigned)P), dim3(64), 0, as_stream(stream), ws, P, C, ms_plan(H),
                       scores + row_offset);
    BG_LAUNCH_CHECK();
    return BG_OK;
}

}  // extern "C"
