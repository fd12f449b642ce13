// powerspec.hip - radial power spectrum of image sets (metrics.py, --ps_freq): batched 2-D real-to-complex FFTs of sides
// 16 to 512 in fp32, the power of every coefficient of the half plane, its azimuthal average and the fp64 mean 2-D spectrum.
// NHWC images in [-1, 1], C in {1, 3, 4}; DESIGN.md gives the definition, tests/ps_ref.py restates it in float64.
//
//   twiddle   exp(-2 pi i k / 512), k < 512, evaluated in fp64 and rounded once to fp32, at the head of the workspace
//   rows      luminance, then the row transforms: rows 2 j and 2 j + 1 of an image are the real and the imaginary part of
//             ONE complex transform Z; A_k = (Z_k + conj Z_{S-k}) / 2 and B_k = (Z_k - conj Z_{S-k}) / 2i are the
//             transforms of the two rows, kept for k = 0 .. S/2 in the workspace, fp32 complex [n, S, S/2 + 1]
//   columns   groups of G columns of one image staged through LDS, transformed along ky, and
//             P = (re^2 + im^2) / S^4 written to power fp32 [n, S, S/2 + 1], row ky in DFT order
//   profile   one thread per radial bin walks the rows of an image in order; the bin's columns of a row are an interval
//             found in integers; columns 0 < kx < S/2 count twice; fp64 sums in a fixed order
//   sum2d     one thread per coefficient adds the images in order in fp64
// No atomics anywhere: a repeated launch is bit-identical.  powerspec_fft.h holds the pass schedule, the butterflies and
// the bank analysis of the padded LDS layouts.
#include <cmath>

#include "common.h"
#include "powerspec_fft.h"

namespace bg {

#define PS_BLOCK 256
#define PS_TW 512                     // twiddle table entries at the head of the workspace
#define PS_TW_BYTES (PS_TW * 8)
#define PS_ROW_POINTS 1024            // complex points of one block of the row kernel: 1024 / S row pairs
#define PS_PROFILE_BLOCK 384          // >= NB(512) = 363 bins

__device__ __forceinline__ float ps_widen(float v) { return v; }
__device__ __forceinline__ float ps_widen(uint16_t bits) { return __uint_as_float((uint32_t)bits << 16); }   // bf16, exact

template <typename T, int C>
__device__ __forceinline__ float ps_luminance(const T* px) {
    if (C == 1) return ps_widen(px[0]);
    return fmaf(0.114f, ps_widen(px[2]), fmaf(0.587f, ps_widen(px[1]), 0.299f * ps_widen(px[0])));   // alpha is ignored
}

__global__ __launch_bounds__(PS_BLOCK) void ps_twiddle_kernel(float2* __restrict__ tw) {
    const int k = blockIdx.x * PS_BLOCK + threadIdx.x;
    if (k < PS_TW) {
        double s, c;
        sincospi(-(double)k / (double)(PS_TW / 2), &s, &c);
        tw[k] = make_float2((float)c, (float)s);
    }
}

// All passes over the two LDS buffers (plane 0 real, plane 1 imaginary).  Returns the index of the buffer that holds the
// result; *mode_out is its layout.  Every thread of the block calls it.
template <int POINTS>
__device__ __forceinline__ int ps_fft(float (*buf)[2][POINTS + POINTS / 4], const float* twr, const float* twi, int lg,
                                      int mode_in, int final_mode, int sk, int* mode_out) {
    PsPass ps = ps_first_pass(lg, mode_in, final_mode);
    int cur = 0;
    bool more = true;
    while (more) {
        if (ps.radix == 4) {
            for (int b = threadIdx.x; b < POINTS / 4; b += PS_BLOCK)
                ps_radix4(buf[cur][0], buf[cur][1], buf[cur ^ 1][0], buf[cur ^ 1][1], twr, twi, b, lg, ps, sk);
        } else {
            for (int b = threadIdx.x; b < POINTS / 2; b += PS_BLOCK)
                ps_radix2(buf[cur][0], buf[cur][1], buf[cur ^ 1][0], buf[cur ^ 1][1], b, lg, ps, sk);
        }
        cur ^= 1;
        __syncthreads();
        *mode_out = ps.wmode;
        more = ps_next_pass(&ps, final_mode);
    }
    return cur;
}

__device__ __forceinline__ void ps_load_twiddles(const float2* __restrict__ tw, float* twr, float* twi, int lg) {
    for (int k = threadIdx.x; k < (1 << lg); k += PS_BLOCK) {
        const float2 w = tw[k << (9 - lg)];
        twr[k] = w.x;
        twi[k] = w.y;
    }
}

// grid: ceil(n * S / 2 row pairs / (1024 / S)).  spec: fp32 complex [n, S, S/2 + 1].
template <typename T, int C>
__global__ __launch_bounds__(PS_BLOCK) void ps_rows_kernel(const T* __restrict__ x, int64_t pairs, int lg,
                                                           const float2* __restrict__ tw, float2* __restrict__ spec) {
    __shared__ float buf[2][2][PS_ROW_POINTS + PS_ROW_POINTS / 4];
    __shared__ float twr[PS_TW], twi[PS_TW];
    const int S = 1 << lg, half = S >> 1, W = half + 1;
    const int per_block = PS_ROW_POINTS >> lg;
    const int64_t pair0 = (int64_t)blockIdx.x * per_block;
    ps_load_twiddles(tw, twr, twi, lg);
    for (int e = threadIdx.x; e < PS_ROW_POINTS; e += PS_BLOCK) {
        const int64_t pr = pair0 + (e >> lg);
        const int col = e & (S - 1);
        float re = 0.0f, im = 0.0f;
        if (pr < pairs) {
            const int64_t img = pr >> (lg - 1), row = (pr & (half - 1)) * 2;
            const T* px = x + (((img << lg) + row) * S + col) * C;
            re = ps_luminance<T, C>(px);
            im = ps_luminance<T, C>(px + (int64_t)S * C);
        }
        buf[0][0][e] = re;
        buf[0][1][e] = im;
    }
    __syncthreads();
    int mode;
    const int cur = ps_fft<PS_ROW_POINTS>(buf, twr, twi, lg, 0, 0, 0, &mode);
    const float* zr = buf[cur][0];
    const float* zi = buf[cur][1];
    for (int o = threadIdx.x; o < per_block * W; o += PS_BLOCK) {
        const int q = o / W, k = o - q * W;
        const int64_t pr = pair0 + q;
        if (pr >= pairs) break;
        const int ik = ps_phys((q << lg) + k, mode, lg, 0), im_ = ps_phys((q << lg) + ((S - k) & (S - 1)), mode, lg, 0);
        const float ar = zr[ik], ai = zi[ik], mr = zr[im_], mi = -zi[im_];          // Z_k and conj Z_{S-k}
        const int64_t img = pr >> (lg - 1), row = (pr & (half - 1)) * 2;
        float2* dst = spec + ((img << lg) + row) * W + k;
        dst[0] = make_float2(0.5f * (ar + mr), 0.5f * (ai + mi));
        dst[W] = make_float2(0.5f * (ai - mi), -0.5f * (ar - mr));                 // (Z_k - conj Z_{S-k}) / 2i
    }
}

// grid: n * ceil((S/2 + 1) / G); G = POINTS / S columns a block.
template <int POINTS>
__global__ __launch_bounds__(PS_BLOCK) void ps_cols_kernel(const float2* __restrict__ spec, int lg, int groups, float scale,
                                                           const float2* __restrict__ tw, float* __restrict__ power) {
    __shared__ float buf[2][2][POINTS + POINTS / 4];
    __shared__ float twr[PS_TW], twi[PS_TW];
    const int S = 1 << lg, W = (S >> 1) + 1;
    const int G = POINTS >> lg, sk = G >= 32 ? 1 : 32 / G;
    const int64_t img = blockIdx.x / groups;
    const int col0 = (blockIdx.x - (int)img * groups) * G;
    const float2* src = spec + (img << lg) * W;
    ps_load_twiddles(tw, twr, twi, lg);
    for (int i = threadIdx.x; i < POINTS; i += PS_BLOCK) {
        const int c = i & (G - 1), ky = i / G, col = col0 + c;
        float2 v = make_float2(0.0f, 0.0f);
        if (col < W) v = src[(int64_t)ky * W + col];
        const int e = ps_phys((c << lg) + ky, 4, lg, sk);
        buf[0][0][e] = v.x;
        buf[0][1][e] = v.y;
    }
    __syncthreads();
    int mode;
    const int cur = ps_fft<POINTS>(buf, twr, twi, lg, 4, 4, sk, &mode);
    float* dst = power + (img << lg) * W;
    for (int i = threadIdx.x; i < POINTS; i += PS_BLOCK) {
        const int c = i & (G - 1), ky = i / G, col = col0 + c;
        if (col < W) {
            const int e = ps_phys((c << lg) + ky, mode, lg, sk);
            const float re = buf[cur][0][e], im = buf[cur][1][e];
            dst[(int64_t)ky * W + col] = fmaf(re, re, im * im) * scale;
        }
    }
}

__device__ __forceinline__ int ps_isqrt(int v) {        // floor(sqrt(v)), v >= 0: a float estimate corrected in integers
    int s = (int)sqrtf((float)v);
    while (s * s > v) --s;
    while ((s + 1) * (s + 1) <= v) ++s;
    return s;
}

// grid n, one thread per bin r < NB.  Bin r holds the coefficients with r^2 - r + 1 <= ky^2 + kx^2 <= r^2 + r (bin 0: DC
// alone), which is r = (isqrt(4 m) + 1) / 2 solved for m; within row ky that is an interval of kx.
__global__ __launch_bounds__(PS_PROFILE_BLOCK) void ps_profile_kernel(const float* __restrict__ power, int S, int NB,
                                                                      double* __restrict__ profiles) {
    const int r = threadIdx.x;
    if (r >= NB) return;
    const int half = S >> 1, W = half + 1;
    const float* P = power + (int64_t)blockIdx.x * S * W;
    const int lo_m = r == 0 ? 0 : r * r - r + 1, hi_m = r * r + r;
    double acc = 0.0;
    long long count = 0;
    for (int i = 0; i < S; ++i) {
        const int fy = i < half ? i : S - i, a = fy * fy;
        if (a > hi_m) continue;
        int lo = 0;
        if (lo_m > a) {
            lo = ps_isqrt(lo_m - a);
            if (lo * lo < lo_m - a) ++lo;
        }
        int hi = ps_isqrt(hi_m - a);
        if (hi > half) hi = half;
        for (int kx = lo; kx <= hi; ++kx) {
            const int w = (kx == 0 || kx == half) ? 1 : 2;
            acc += (double)w * (double)P[i * W + kx];
            count += w;
        }
    }
    profiles[(int64_t)blockIdx.x * NB + r] = count ? acc / (double)count : 0.0;
}

__global__ __launch_bounds__(PS_BLOCK) void ps_sum2d_kernel(const float* __restrict__ power, int n, int plane,
                                                            double* __restrict__ sum2d) {
    const int idx = blockIdx.x * PS_BLOCK + threadIdx.x;
    if (idx >= plane) return;
    double acc = sum2d[idx];
    for (int i = 0; i < n; ++i) acc += (double)power[(int64_t)i * plane + idx];
    sum2d[idx] = acc;
}

static inline int ps_log2_side(int S) {                 // log2 of a power of two in [16, 512], else 0
    for (int lg = 4; lg <= 9; ++lg)
        if (S == (1 << lg)) return lg;
    return 0;
}

static inline int ps_bins(int S) {                      // (isqrt(2 S^2) + 1) / 2 + 1: the corner (S/2, S/2) is the last bin
    const long long v = 2LL * S * S;
    long long s = (long long)std::sqrt((double)v);
    while (s * s > v) --s;
    while ((s + 1) * (s + 1) <= v) ++s;
    return (int)((s + 1) / 2 + 1);
}

template <typename T>
static void ps_launch_rows(int C, unsigned grid, hipStream_t s, const T* x, int64_t pairs, int lg, const float2* tw,
                           float2* spec) {
    if (C == 1)
        hipLaunchKernelGGL((ps_rows_kernel<T, 1>), dim3(grid), dim3(PS_BLOCK), 0, s, x, pairs, lg, tw, spec);
    else if (C == 3)
        hipLaunchKernelGGL((ps_rows_kernel<T, 3>), dim3(grid), dim3(PS_BLOCK), 0, s, x, pairs, lg, tw, spec);
    else
        hipLaunchKernelGGL((ps_rows_kernel<T, 4>), dim3(grid), dim3(PS_BLOCK), 0, s, x, pairs, lg, tw, spec);
}

}  // namespace bg

using namespace bg;

extern "C" {

size_t bg_ps_workspace_bytes(int n, int S) {
    if (n < 1 || !ps_log2_side(S)) return 0;
    return (size_t)PS_TW_BYTES + (size_t)n * (size_t)S * (size_t)(S / 2 + 1) * sizeof(float2);
}

int bg_ps_power(const void* x, int dtype, int n, int S, int C, float* power, void* ws, size_t ws_bytes, void* stream) {
    BG_REQUIRE(x && power && ws, "bg_ps_power: NULL pointer");
    BG_REQUIRE(dtype == BG_F32 || dtype == BG_BF16, "bg_ps_power: dtype=%d (BG_F32 or BG_BF16)", dtype);
    const int lg = ps_log2_side(S);
    BG_REQUIRE(lg, "bg_ps_power: S=%d (a power of two from 16 to 512)", S);
    BG_REQUIRE(C == 1 || C == 3 || C == 4, "bg_ps_power: C=%d (1, 3 or 4)", C);
    BG_REQUIRE(n >= 1 && n <= (1 << 20), "bg_ps_power: n=%d (1..1048576 images a launch)", n);
    BG_REQUIRE(ws_bytes >= bg_ps_workspace_bytes(n, S), "bg_ps_power: workspace of %zu bytes, bg_ps_workspace_bytes(%d, %d) = %zu needed",
               ws_bytes, n, S, bg_ps_workspace_bytes(n, S));
    BG_REQUIRE(((uintptr_t)x & (dtype == BG_F32 ? 3 : 1)) == 0 && ((uintptr_t)power & 3) == 0 && ((uintptr_t)ws & 7) == 0,
               "bg_ps_power: buffers must be aligned (images to their element, power to 4 bytes, workspace to 8)");
    hipStream_t s = as_stream(stream);
    float2* tw = static_cast<float2*>(ws);
    float2* spec = tw + PS_TW;
    hipLaunchKernelGGL(ps_twiddle_kernel, dim3(PS_TW / PS_BLOCK), dim3(PS_BLOCK), 0, s, tw);
    const int64_t pairs = (int64_t)n * (S / 2);
    const int per_block = PS_ROW_POINTS >> lg;
    const unsigned row_grid = (unsigned)((pairs + per_block - 1) / per_block);
    if (dtype == BG_F32)
        ps_launch_rows<float>(C, row_grid, s, static_cast<const float*>(x), pairs, lg, tw, spec);
    else
        ps_launch_rows<uint16_t>(C, row_grid, s, static_cast<const uint16_t*>(x), pairs, lg, tw, spec);
    BG_LAUNCH_CHECK();
    const float scale = 1.0f / ((float)S * (float)S * (float)S * (float)S);       // a power of two: exact
    const int W = S / 2 + 1;
    if (S <= 128) {                                                               // 1024 / S columns a block
        const int G = 1024 >> lg, groups = (W + G - 1) / G;
        hipLaunchKernelGGL((ps_cols_kernel<1024>), dim3((unsigned)(n * groups)), dim3(PS_BLOCK), 0, s, spec, lg, groups, scale,
                           tw, power);
    } else {                                                                      // 8 columns at 256, 4 at 512
        const int G = 2048 >> lg, groups = (W + G - 1) / G;
        hipLaunchKernelGGL((ps_cols_kernel<2048>), dim3((unsigned)(n * groups)), dim3(PS_BLOCK), 0, s, spec, lg, groups, scale,
                           tw, power);
    }
    BG_LAUNCH_CHECK();
    return BG_OK;
}

int bg_ps_profile(const float* power, int n, int S, double* profiles, double* sum2d, void* stream) {
    BG_REQUIRE(power && profiles, "bg_ps_profile: NULL pointer");
    BG_REQUIRE(ps_log2_side(S), "bg_ps_profile: S=%d (a power of two from 16 to 512)", S);
    BG_REQUIRE(n >= 1 && n <= (1 << 20), "bg_ps_profile: n=%d (1..1048576 images a launch)", n);
    BG_REQUIRE(((uintptr_t)power & 3) == 0 && ((uintptr_t)profiles & 7) == 0 && ((uintptr_t)sum2d & 7) == 0,
               "bg_ps_profile: buffers must be aligned (power to 4 bytes, profiles and sum2d to 8)");
    hipStream_t s = as_stream(stream);
    hipLaunchKernelGGL(ps_profile_kernel, dim3((unsigned)n), dim3(PS_PROFILE_BLOCK), 0, s, power, S, ps_bins(S), profiles);
    BG_LAUNCH_CHECK();
    if (sum2d) {
        const int plane = S * (S / 2 + 1);
        hipLaunchKernelGGL(ps_sum2d_kernel, dim3((unsigned)((plane + PS_BLOCK - 1) / PS_BLOCK)), dim3(PS_BLOCK), 0, s, power, n,
                           plane, sum2d);
        BG_LAUNCH_CHECK();
    }
    return BG_OK;
}

}  // extern "C"
