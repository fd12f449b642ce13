// alpha.hip - the two RGBA image ops of --c_dim 4 (BigGAN.py:572-579, 616-619), on fp32 NHWC [rows][4] tensors:
// one pixel per thread, one 16-byte load per pixel and operand.  Both sit on the image (a 4-channel fp32 tensor in
// every precision: G_logit's result and DiffAugment's output are never bf16-resident), so they are HBM-bound passes.
//
//   alpha helper (generator head):  a' = a + w (r + g + b + a), then tanh over all four channels.  The sum includes the
//                                   alpha logit itself (tf.reduce_sum(x, -1) over every channel).  w is one fp32 in
//                                   device memory (generator/alphahelper_w), read by the kernels: graph capture works.
//   alpha mask (discriminator input): rgb' = (rgb + 1)(a + 1)/2 - 1, alpha unchanged.
//
// The helper's weight gradient is a sum over every pixel: each block stores one fp64 partial in the deterministic
// reduction workspace and alpha_dw_finalize_kernel adds them in a fixed order (no atomics: reruns are bit-identical).
#include "common.h"

namespace bg {

#define ALPHA_BLOCK 256
#define ALPHA_MAX_BLOCKS 2048

static inline int alpha_grid(int64_t rows) {
    int64_t b = (rows + ALPHA_BLOCK - 1) / ALPHA_BLOCK;
    return (int)(b < ALPHA_MAX_BLOCKS ? b : ALPHA_MAX_BLOCKS);
}

static inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

__device__ __forceinline__ float4 ld4(const float* p, int64_t i) { return reinterpret_cast<const float4*>(p)[i]; }
__device__ __forceinline__ void st4(float* p, int64_t i, float4 v) { reinterpret_cast<float4*>(p)[i] = v; }

__device__ __forceinline__ float alpha_logit(float4 v, float w) { return v.w + w * (((v.x + v.y) + v.z) + v.w); }

__global__ __launch_bounds__(ALPHA_BLOCK) void alpha_head_fwd_kernel(const float* __restrict__ x,
                                                                     const float* __restrict__ w,
                                                                     float* __restrict__ y, int64_t rows) {
    const float wv = w[0];
    for (int64_t i = (int64_t)blockIdx.x * ALPHA_BLOCK + threadIdx.x; i < rows; i += (int64_t)gridDim.x * ALPHA_BLOCK) {
        const float4 v = ld4(x, i);
        st4(y, i, make_float4(tanhf(v.x), tanhf(v.y), tanhf(v.z), tanhf(alpha_logit(v, wv))));
    }
}

// g = dy (1 - y^2) with y recomputed from x as the forward computed it;
// dx_c = g_c + w g_a (colour), dx_a = g_a (1 + w), dw = sum over pixels of g_a (r + g + b + a)
__global__ __launch_bounds__(ALPHA_BLOCK) void alpha_head_bwd_kernel(const float* __restrict__ x,
                                                                     const float* __restrict__ w,
                                                                     const float* __restrict__ dy,
                                                                     float* __restrict__ dx, double* __restrict__ part,
                                                                     int64_t rows) {
    __shared__ double sh[ALPHA_BLOCK / 64];
    const float wv = w[0];
    double acc = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * ALPHA_BLOCK + threadIdx.x; i < rows; i += (int64_t)gridDim.x * ALPHA_BLOCK) {
        const float4 v = ld4(x, i), d = ld4(dy, i);
        const float yr = tanhf(v.x), yg = tanhf(v.y), yb = tanhf(v.z), ya = tanhf(alpha_logit(v, wv));
        const float gr = d.x * (1.f - yr * yr), gg = d.y * (1.f - yg * yg), gb = d.z * (1.f - yb * yb);
        const float ga = d.w * (1.f - ya * ya);
        st4(dx, i, make_float4(gr + wv * ga, gg + wv * ga, gb + wv * ga, ga * (1.f + wv)));
        acc += (double)ga * (double)(((v.x + v.y) + v.z) + v.w);
    }
    if (!part) return;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    if (lane == 0) sh[wid] = acc;
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.x] = ((sh[0] + sh[1]) + sh[2]) + sh[3];
}

// dw[0] += sum of the per-block partials in a fixed order: lane l adds blocks l, l + 64, ... in turn, then a fixed
// butterfly over the wave (one serial thread over 2048 partials took 0.1 ms)
__global__ __launch_bounds__(64) void alpha_dw_finalize_kernel(const double* __restrict__ part, float* dw, int nb) {
    double s = 0.0;
    for (int b = threadIdx.x; b < nb; b += 64) s += part[b];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if (threadIdx.x == 0) dw[0] += (float)s;
}

__global__ __launch_bounds__(ALPHA_BLOCK) void alpha_mask_fwd_kernel(const float* __restrict__ x,
                                                                     float* __restrict__ y, int64_t rows) {
    for (int64_t i = (int64_t)blockIdx.x * ALPHA_BLOCK + threadIdx.x; i < rows; i += (int64_t)gridDim.x * ALPHA_BLOCK) {
        const float4 v = ld4(x, i);
        const float h = 0.5f * (v.w + 1.f);
        st4(y, i, make_float4((v.x + 1.f) * h - 1.f, (v.y + 1.f) * h - 1.f, (v.z + 1.f) * h - 1.f, v.w));
    }
}

// dx_rgb = dy_rgb (a + 1) / 2, dx_a = dy_a + sum_c dy_c (rgb_c + 1) / 2
__global__ __launch_bounds__(ALPHA_BLOCK) void alpha_mask_bwd_kernel(const float* __restrict__ x,
                                                                     const float* __restrict__ dy,
                                                                     float* __restrict__ dx, int64_t rows) {
    for (int64_t i = (int64_t)blockIdx.x * ALPHA_BLOCK + threadIdx.x; i < rows; i += (int64_t)gridDim.x * ALPHA_BLOCK) {
        const float4 v = ld4(x, i), d = ld4(dy, i);
        const float h = 0.5f * (v.w + 1.f);
        const float s = (d.x * (v.x + 1.f) + d.y * (v.y + 1.f)) + d.z * (v.z + 1.f);
        st4(dx, i, make_float4(d.x * h, d.y * h, d.z * h, d.w + 0.5f * s));
    }
}

// forward-mode tangent at x: ydot_rgb = (xdot_rgb (a + 1) + (rgb + 1) xdot_a) / 2, ydot_a = xdot_a
__global__ __launch_bounds__(ALPHA_BLOCK) void alpha_mask_tangent_kernel(const float* __restrict__ x,
                                                                         const float* __restrict__ xdot,
                                                                         float* __restrict__ ydot, int64_t rows) {
    for (int64_t i = (int64_t)blockIdx.x * ALPHA_BLOCK + threadIdx.x; i < rows; i += (int64_t)gridDim.x * ALPHA_BLOCK) {
        const float4 v = ld4(x, i), t = ld4(xdot, i);
        const float a1 = v.w + 1.f;
        st4(ydot, i, make_float4(0.5f * (t.x * a1 + (v.x + 1.f) * t.w), 0.5f * (t.y * a1 + (v.y + 1.f) * t.w),
                                 0.5f * (t.z * a1 + (v.z + 1.f) * t.w), t.w));
    }
}

}  // namespace bg

using namespace bg;

#define ALPHA_REQUIRE_ROWS(name, rows) BG_REQUIRE((rows) > 0, name ": rows must be positive")
#define ALPHA_REQUIRE_ALIGNED(name, ...)                                                          \
    do {                                                                                          \
        const void* ps__[] = {__VA_ARGS__};                                                       \
        for (const void* p__ : ps__) BG_REQUIRE(aligned16(p__), name ": tensors must be 16-byte aligned"); \
    } while (0)

extern "C" {

int bg_alpha_head_fwd(const float* x, const float* w, float* y, int64_t rows, void* stream) {
    BG_REQUIRE(x && w && y, "bg_alpha_head_fwd: NULL tensor");
    ALPHA_REQUIRE_ROWS("bg_alpha_head_fwd", rows);
    ALPHA_REQUIRE_ALIGNED("bg_alpha_head_fwd", x, y);
    hipLaunchKernelGGL(alpha_head_fwd_kernel, dim3(alpha_grid(rows)), dim3(ALPHA_BLOCK), 0, as_stream(stream), x, w, y,
                       rows);
    BG_LAUNCH_CHECK();
    return BG_OK;
}

int bg_alpha_head_bwd(const float* x, const float* w, const float* dy, float* dx, float* dw_accum, int64_t rows,
                      void* stream) {
    BG_REQUIRE(x && w && dy && dx, "bg_alpha_head_bwd: NULL tensor");
    ALPHA_REQUIRE_ROWS("bg_alpha_head_bwd", rows);
    ALPHA_REQUIRE_ALIGNED("bg_alpha_head_bwd", x, dy, dx);
    hipStream_t s = as_stream(stream);
    const int grid = alpha_grid(rows);
    double* part = nullptr;
    if (dw_accum) {
        // (the per-device partial-sum workspace holds floats: two per fp64 partial)
        part = reinterpret_cast<double*>(colreduce_workspace((size_t)grid * 2, s));
        if (!part) return BG_ERR_LAUNCH;
    }
    hipLaunchKernelGGL(alpha_head_bwd_kernel, dim3(grid), dim3(ALPHA_BLOCK), 0, s, x, w, dy, dx, part, rows);
    if (dw_accum) hipLaunchKernelGGL(alpha_dw_finalize_kernel, dim3(1), dim3(64), 0, s, part, dw_accum, grid);
    BG_LAUNCH_CHECK();
    return BG_OK;
}

int bg_alpha_mask_fwd(const float* x, float* y, int64_t rows, void* stream) {
    BG_REQUIRE(x && y, "bg_alpha_mask_fwd: NULL tensor");
    ALPHA_REQUIRE_ROWS("bg_alpha_mask_fwd", rows);
    ALPHA_REQUIRE_ALIGNED("bg_alpha_mask_fwd", x, y);
    hipLaunchKernelGGL(alpha_mask_fwd_kernel, dim3(alpha_grid(rows)), dim3(ALPHA_BLOCK), 0, as_stream(stream), x, y,
                       rows);
    BG_LAUNCH_CHECK();
    return BG_OK;
}

int bg_alpha_mask_bwd(const float* x, const float* dy, float* dx, int64_t rows, void* stream) {
    BG_REQUIRE(x && dy && dx, "bg_alpha_mask_bwd: NULL tensor");
    ALPHA_REQUIRE_ROWS("bg_alpha_mask_bwd", rows);
    ALPHA_REQUIRE_ALIGNED("bg_alpha_mask_bwd", x, dy, dx);
    hipLaunchKernelGGL(alpha_mask_bwd_kernel, dim3(alpha_grid(rows)), dim3(ALPHA_BLOCK), 0, as_stream(stream), x, dy,
                       dx, rows);
    BG_LAUNCH_CHECK();
    return BG_OK;
}

int bg_alpha_mask_tangent(const float* x, const float* xdot, float* ydot, int64_t rows, void* stream) {
    BG_REQUIRE(x && xdot && ydot, "bg_alpha_mask_tangent: NULL tensor");
    ALPHA_REQUIRE_ROWS("bg_alpha_mask_tangent", rows);
    ALPHA_REQUIRE_ALIGNED("bg_alpha_mask_tangent", x, xdot, ydot);
    hipLaunchKernelGGL(alpha_mask_tangent_kernel, dim3(alpha_grid(rows)), dim3(ALPHA_BLOCK), 0, as_stream(stream), x,
                       xdot, ydot, rows);
    BG_LAUNCH_CHECK();
    return BG_OK;
}

}  // extern "C"
