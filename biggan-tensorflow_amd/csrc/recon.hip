// recon.hip - the arithmetic of the discriminator's reconstruction heads (BigGAN.py:639-661 simple_upscaler on a
// feature map, 810-836 the L2-norm losses; --d_reconstruction / --d_reconstruction_halfres / --d_reconstruction_texture).
//
//   glu             ops.py:842-845   y[r, c] = x[r, c] * sigmoid(x[r, C + c]),  x [rows, 2C]
//   upsample2 (_t)  ops.py:516-519   nearest-neighbour 2x on fp32 or bf16 tensors; the backward is the 2x2 box sum
//   crop_at         BigGAN.py:657    y[N,p,p,C] = x[N, oy:oy+p, ox:ox+p, C] with (oy, ox) read from DEVICE memory, so a
//                                    captured graph replays with fresh draws; the backward writes the whole dx (dy inside
//                                    the window, zero outside) in one pass
//   recon_loss      BigGAN.py:817    ||tanh(y) - target||_2 * scale, target = the image itself, its 2x2 average
//                                    (halfres) or its crop at (oy * f, ox * f) (texture)
//
// The feature-map kernels (glu, bn + glu, upsample2, crop_at) are HBM-bound: one 16-byte piece per thread per step
// wherever the channel count allows it (C % 4 == 0 in fp32, C % 8 == 0 in bf16), a scalar form otherwise; arithmetic in
// fp32 registers, one rounding per stored bf16 element.  The loss kernels work on c_dim-channel fp32 images (1, 3 or 4
// channels, a few hundred KB per sample): one element per thread step, scalar accesses.  Offsets are clamped to the
// valid range on the device: no draw can address outside the tensors.
#include "common.h"

namespace bg {

#define RC_BLOCK 256
#define RC_MAX_BLOCKS 8192

static inline int rc_blocks(int64_t work) {
    int64_t b = (work + RC_BLOCK - 1) / RC_BLOCK;
    if (b > RC_MAX_BLOCKS) b = RC_MAX_BLOCKS;
    if (b < 1) b = 1;
    return (int)b;
}

template <typename T, int VEC>
struct Piece;      // VEC elements of T moved as one access, widened to fp32 registers

template <>
struct Piece<float, 4> {
    static __device__ __forceinline__ void load(const float* p, float (&v)[4]) {
        const float4 t = *reinterpret_cast<const float4*>(p);
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    }
    static __device__ __forceinline__ void store(float* p, const float (&v)[4]) {
        *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
    }
};
template <>
struct Piece<float, 1> {
    static __device__ __forceinline__ void load(const float* p, float (&v)[1]) { v[0] = p[0]; }
    static __device__ __forceinline__ void store(float* p, const float (&v)[1]) { p[0] = v[0]; }
};
template <>
struct Piece<__bf16, 8> {
    typedef __bf16 bf16x8v __attribute__((ext_vector_type(8)));
    static __device__ __forceinline__ void load(const __bf16* p, float (&v)[8]) {
        const bf16x8v t = *reinterpret_cast<const bf16x8v*>(p);
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = (float)t[j];
    }
    static __device__ __forceinline__ void store(__bf16* p, const float (&v)[8]) {
        bf16x8v t;
#pragma unroll
        for (int j = 0; j < 8; ++j) t[j] = (__bf16)v[j];
        *reinterpret_cast<bf16x8v*>(p) = t;
    }
};
template <>
struct Piece<__bf16, 1> {
    static __device__ __forceinline__ void load(const __bf16* p, float (&v)[1]) { v[0] = (float)p[0]; }
    static __device__ __forceinline__ void store(__bf16* p, const float (&v)[1]) { p[0] = (__bf16)v[0]; }
};

__device__ __forceinline__ float sigmoid_f(float g) { return 1.f / (1.f + expf(-g)); }

// ---- GLU ------------------------------------------------------------------------------------------------------
template <typename T, int VEC>
__global__ __launch_bounds__(RC_BLOCK) void glu_fwd_kernel(const T* __restrict__ x, T* __restrict__ y, int64_t rows,
                                                           int C) {
    const int CV = C / VEC;
    const int64_t total = rows * CV;
    for (int64_t i = (int64_t)blockIdx.x * RC_BLOCK + threadIdx.x; i < total; i += (int64_t)gridDim.x * RC_BLOCK) {
        const int64_t r = i / CV;
        const int c = (int)(i - r * CV) * VEC;
        float a[VEC], g[VEC], o[VEC];
        Piece<T, VEC>::load(x + r * 2 * C + c, a);
        Piece<T, VEC>::load(x + r * 2 * C + C + c, g);
#pragma unroll
        for (int j = 0; j < VEC; ++j) o[j] = a[j] * sigmoid_f(g[j]);
        Piece<T, VEC>::store(y + r * C + c, o);
    }
}

template <typename T, int VEC>
__global__ __launch_bounds__(RC_BLOCK) void glu_bwd_kernel(const T* __restrict__ x, const T* __restrict__ dy,
                                                           T* __restrict__ dx, int64_t rows, int C) {
    const int CV = C / VEC;
    const int64_t total = rows * CV;
    for (int64_t i = (int64_t)blockIdx.x * RC_BLOCK + threadIdx.x; i < total; i += (int64_t)gridDim.x * RC_BLOCK) {
        const int64_t r = i / CV;
        const int c = (int)(i - r * CV) * VEC;
        float a[VEC], g[VEC], d[VEC], da[VEC], dg[VEC];
        Piece<T, VEC>::load(x + r * 2 * C + c, a);
        Piece<T, VEC>::load(x + r * 2 * C + C + c, g);
        Piece<T, VEC>::load(dy + r * C + c, d);
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
            const float s = sigmoid_f(g[j]);
            da[j] = d[j] * s;
            dg[j] = d[j] * a[j] * s * (1.f - s);
        }
        Piece<T, VEC>::store(dx + r * 2 * C + c, da);
        Piece<T, VEC>::store(dx + r * 2 * C + C + c, dg);
    }
}

// ---- batch-norm apply + GLU (the default order of simple_upscale: conv, bn, glu) -------------------------------------
// x [rows, 2C] is read once: both halves are normalised with the per-channel affine of bg_bn_apply_act_* and the first
// is gated by the sigmoid of the second.  The backward mirrors the reduce / finalize / dx split of batch norm: the
// reduce pass leaves, per row segment and channel, sum g and sum g xh (g = the gradient at the batch-norm output, i.e.
// the GLU backward recomputed on the fly) in the layout bg_bn_bwd_finalize reads; the dx pass gets the all-reduced means.
struct BnGluParams {
    const float *mean, *rstd, *gamma, *beta;      // [2C]
};

template <int VEC>
__device__ __forceinline__ void ldf(const float* p, float (&v)[VEC]) {
#pragma unroll
    for (int j = 0; j < VEC; ++j) v[j] = p[j];
}

// pre-activations of both halves (tf.nn.batch_normalization: x inv + (offset - mean inv)) and xh = (x - mean) rstd
template <typename T, int VEC>
__device__ __forceinline__ void bn_glu_load(const T* xrow, const BnGluParams& p, int c, int C, float (&pre)[2][VEC],
                                            float (&xh)[2][VEC], float (&rs)[2][VEC], float (&ga)[2][VEC]) {
#pragma unroll
    for (int hf = 0; hf < 2; ++hf) {
        float xv[VEC], mu[VEC], be[VEC];
        Piece<T, VEC>::load(xrow + hf * C + c, xv);
        ldf<VEC>(p.mean + hf * C + c, mu);
        ldf<VEC>(p.rstd + hf * C + c, rs[hf]);
        ldf<VEC>(p.gamma + hf * C + c, ga[hf]);
        ldf<VEC>(p.beta + hf * C + c, be);
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
            const float inv = rs[hf][j] * ga[hf][j];
            pre[hf][j] = xv[j] * inv + (be[j] - mu[j] * inv);
            xh[hf][j] = (xv[j] - mu[j]) * rs[hf][j];
        }
    }
}

template <typename T, int VEC>
__global__ __launch_bounds__(RC_BLOCK) void bn_glu_fwd_kernel(const T* __restrict__ x, BnGluParams p, T* __restrict__ y,
                                                              int64_t rows, int C) {
    const int CV = C / VEC;
    const int64_t total = rows * CV;
    for (int64_t i = (int64_t)blockIdx.x * RC_BLOCK + threadIdx.x; i < total; i += (int64_t)gridDim.x * RC_BLOCK) {
        const int64_t r = i / CV;
        const int c = (int)(i - r * CV) * VEC;
        float pre[2][VEC], xh[2][VEC], rs[2][VEC], ga[2][VEC], o[VEC];
        bn_glu_load<T, VEC>(x + r * 2 * C, p, c, C, pre, xh, rs, ga);
#pragma unroll
        for (int j = 0; j < VEC; ++j) o[j] = pre[0][j] * sigmoid_f(pre[1][j]);
        Piece<T, VEC>::store(y + r * C + c, o);
    }
}

// grid (channel tiles, row segments); a block is LC channel lanes x RL row lanes; part [3][nseg][2C] (plane 2 unused)
template <typename T, int VEC>
__global__ __launch_bounds__(RC_BLOCK) void bn_glu_bwd_reduce_kernel(const T* __restrict__ x, const T* __restrict__ dy,
                                                                     BnGluParams p, float* __restrict__ part, int64_t rows,
                                                                     int64_t rps, int C, int LC, int RL, int nseg) {
    __shared__ float red[4 * VEC][RC_BLOCK];
    const int CV = C / VEC;
    const int cx = threadIdx.x % LC, ry = threadIdx.x / LC;
    const int cv = blockIdx.x * LC + cx;
    const bool live = ry < RL && cv < CV;
    const int c = cv * VEC;
    float acc[4][VEC];
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int j = 0; j < VEC; ++j) acc[q][j] = 0.f;
    if (live) {
        const int64_t r0 = (int64_t)blockIdx.y * rps;
        const int64_t r1 = r0 + rps < rows ? r0 + rps : rows;
        for (int64_t r = r0 + ry; r < r1; r += RL) {
            float pre[2][VEC], xh[2][VEC], rs[2][VEC], ga[2][VEC], d[VEC];
            bn_glu_load<T, VEC>(x + r * 2 * C, p, c, C, pre, xh, rs, ga);
            Piece<T, VEC>::load(dy + r * C + c, d);
#pragma unroll
            for (int j = 0; j < VEC; ++j) {
                const float s = sigmoid_f(pre[1][j]);
                const float gm = d[j] * s, gg = d[j] * pre[0][j] * s * (1.f - s);
                acc[0][j] += gm;
                acc[1][j] += gm * xh[0][j];
                acc[2][j] += gg;
                acc[3][j] += gg * xh[1][j];
            }
        }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int j = 0; j < VEC; ++j) red[q * VEC + j][threadIdx.x] = acc[q][j];
    __syncthreads();
    if (!live || ry != 0) return;
    const int64_t plane = (int64_t)nseg * 2 * C;
    float* out = part + (int64_t)blockIdx.y * 2 * C;
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
            float sum = 0.f;
            for (int k = 0; k < RL; ++k) sum += red[q * VEC + j][k * LC + cx];
            // q: 0 sum g (main), 1 sum g xh (main), 2 sum g (gate), 3 sum g xh (gate)
            out[(q & 1) * plane + (q >> 1) * C + c + j] = sum;
        }
}

// dx = rstd (g gamma - m1 - xh m2), cm = {m1 [2C], m2 [2C]} from bg_bn_bwd_finalize (all-reduced by the caller)
template <typename T, int VEC>
__global__ __launch_bounds__(RC_BLOCK) void bn_glu_bwd_dx_kernel(const T* __restrict__ x, const T* __restrict__ dy,
                                                                 BnGluParams p, const float* __restrict__ cm,
                                                                 T* __restrict__ dx, int64_t rows, int C) {
    const int CV = C / VEC;
    const int64_t total = rows * CV;
    for (int64_t i = (int64_t)blockIdx.x * RC_BLOCK + threadIdx.x; i < total; i += (int64_t)gridDim.x * RC_BLOCK) {
        const int64_t r = i / CV;
        const int c = (int)(i - r * CV) * VEC;
        float pre[2][VEC], xh[2][VEC], rs[2][VEC], ga[2][VEC], d[VEC], g[2][VEC];
        bn_glu_load<T, VEC>(x + r * 2 * C, p, c, C, pre, xh, rs, ga);
        Piece<T, VEC>::load(dy + r * C + c, d);
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
            const float s = sigmoid_f(pre[1][j]);
            g[0][j] = d[j] * s;
            g[1][j] = d[j] * pre[0][j] * s * (1.f - s);
        }
#pragma unroll
        for (int hf = 0; hf < 2; ++hf) {
            float m1[VEC], m2[VEC], o[VEC];
            ldf<VEC>(cm + hf * C + c, m1);
            ldf<VEC>(cm + 2 * C + hf * C + c, m2);
#pragma unroll
            for (int j = 0; j < VEC; ++j) o[j] = rs[hf][j] * (g[hf][j] * ga[hf][j] - m1[j] - xh[hf][j] * m2[j]);
            Piece<T, VEC>::store(dx + r * 2 * C + hf * C + c, o);
        }
    }
}

// ---- nearest 2x ------------------------------------------------------------------------------------------------
// one OUTPUT piece per thread step (stores coalesced; each input piece is read four times, three of them from cache)
template <typename T, int VEC>
__global__ __launch_bounds__(RC_BLOCK) void upsample2_fwd_kernel(const T* __restrict__ x, T* __restrict__ y, int64_t NH2,
                                                                 int H, int W, int C) {
    const int CV = C / VEC;
    const int64_t rowp = (int64_t)2 * W * CV;          // pieces per output row
    const int64_t total = NH2 * rowp;
    for (int64_t i = (int64_t)blockIdx.x * RC_BLOCK + threadIdx.x; i < total; i += (int64_t)gridDim.x * RC_BLOCK) {
        const int64_t q = i / rowp;                    // n * 2H + ho
        const int rem = (int)(i - q * rowp);
        const int wo = rem / CV;
        const int c = (rem - wo * CV) * VEC;
        const int64_t n = q / (2 * H);
        const int ho = (int)(q - n * 2 * H);
        float v[VEC];
        Piece<T, VEC>::load(x + ((n * H + (ho >> 1)) * W + (wo >> 1)) * C + c, v);
        Piece<T, VEC>::store(y + (q * 2 * W + wo) * C + c, v);
    }
}

// dx[n,h,w,c] = sum of the 2x2 window of dy, summed in fp32, rounded once
template <typename T, int VEC>
__global__ __launch_bounds__(RC_BLOCK) void upsample2_bwd_kernel(const T* __restrict__ dy, T* __restrict__ dx, int64_t NH,
                                                                 int H, int W, int C) {
    const int CV = C / VEC;
    const int64_t rowp = (int64_t)W * CV;
    const int64_t total = NH * rowp;
    for (int64_t i = (int64_t)blockIdx.x * RC_BLOCK + threadIdx.x; i < total; i += (int64_t)gridDim.x * RC_BLOCK) {
        const int64_t q = i / rowp;                    // n * H + h
        const int rem = (int)(i - q * rowp);
        const int w = rem / CV;
        const int c = (rem - w * CV) * VEC;
        const T* top = dy + ((q * 2) * (int64_t)(2 * W) + 2 * w) * C + c;
        const T* bot = top + (int64_t)2 * W * C;
        float a[VEC], b[VEC], e[VEC], f[VEC], o[VEC];
        Piece<T, VEC>::load(top, a);
        Piece<T, VEC>::load(top + C, b);
        Piece<T, VEC>::load(bot, e);
        Piece<T, VEC>::load(bot + C, f);
#pragma unroll
        for (int j = 0; j < VEC; ++j) o[j] = (a[j] + b[j]) + (e[j] + f[j]);
        Piece<T, VEC>::store(dx + (q * W + w) * C + c, o);
    }
}

// ---- crop at a device-resident offset --------------------------------------------------------------------------
__device__ __forceinline__ int clamp_off(const int32_t* p, int hi) {
    const int v = p[0];
    return v < 0 ? 0 : (v > hi ? hi : v);
}

template <typename T, int VEC>
__global__ __launch_bounds__(RC_BLOCK) void crop_at_fwd_kernel(const T* __restrict__ x, T* __restrict__ y,
                                                               const int32_t* __restrict__ off_y,
                                                               const int32_t* __restrict__ off_x, int N, int H, int W,
                                                               int p, int C) {
    const int oy = clamp_off(off_y, H - p), ox = clamp_off(off_x, W - p);
    const int CV = C / VEC;
    const int64_t rowp = (int64_t)p * CV;
    const int64_t total = (int64_t)N * p * rowp;
    for (int64_t i = (int64_t)blockIdx.x * RC_BLOCK + threadIdx.x; i < total; i += (int64_t)gridDim.x * RC_BLOCK) {
        const int64_t q = i / rowp;                    // n * p + a
        const int rem = (int)(i - q * rowp);           // b * CV + piece: the window's row is contiguous in x
        const int64_t n = q / p;
        const int a = (int)(q - n * p);
        float v[VEC];
        Piece<T, VEC>::load(x + ((n * H + oy + a) * W + ox) * C + (int64_t)rem * VEC, v);
        Piece<T, VEC>::store(y + i * VEC, v);
    }
}

template <typename T, int VEC>
__global__ __launch_bounds__(RC_BLOCK) void crop_at_bwd_kernel(const T* __restrict__ dy, T* __restrict__ dx,
                                                               const int32_t* __restrict__ off_y,
                                                               const int32_t* __restrict__ off_x, int N, int H, int W,
                                                               int p, int C) {
    const int oy = clamp_off(off_y, H - p), ox = clamp_off(off_x, W - p);
    const int CV = C / VEC;
    const int64_t rowp = (int64_t)W * CV;
    const int64_t total = (int64_t)N * H * rowp;
    for (int64_t i = (int64_t)blockIdx.x * RC_BLOCK + threadIdx.x; i < total; i += (int64_t)gridDim.x * RC_BLOCK) {
        const int64_t q = i / rowp;                    // n * H + h
        const int rem = (int)(i - q * rowp);
        const int w = rem / CV;
        const int64_t n = q / H;
        const int a = (int)(q - n * H) - oy, b = w - ox;
        float v[VEC];
        if (a >= 0 && a < p && b >= 0 && b < p) {
            Piece<T, VEC>::load(dy + ((n * p + a) * p + b) * C + (rem - w * CV) * VEC, v);
        } else {
#pragma unroll
            for (int j = 0; j < VEC; ++j) v[j] = 0.f;
        }
        Piece<T, VEC>::store(dx + i * VEC, v);
    }
}

// ---- reconstruction loss ---------------------------------------------------------------------------------------
struct ReconGeom {
    int h, w, S, C, mode, f;      // y [N,h,w,C], target [N,S,S,C]
};

// target value for output element (n, i, j, c); oy / ox: the clamped FEATURE offsets (mode 2)
__device__ __forceinline__ float recon_target(const float* __restrict__ t, const ReconGeom& g, int64_t n, int i, int j,
                                              int c, int oy, int ox) {
    const int64_t base = n * g.S * (int64_t)g.S;
    if (g.mode == 0) return t[(base + (int64_t)i * g.S + j) * g.C + c];
    if (g.mode == 1) {
        const float* p = t + (base + (int64_t)(2 * i) * g.S + 2 * j) * g.C + c;
        const float* q = p + (int64_t)g.S * g.C;
        return 0.25f * ((p[0] + p[g.C]) + (q[0] + q[g.C]));
    }
    return t[(base + (int64_t)(oy * g.f + i) * g.S + (ox * g.f + j)) * g.C + c];
}

__device__ __forceinline__ void recon_offsets(const ReconGeom& g, const int32_t* off_y, const int32_t* off_x, int& oy,
                                              int& ox) {
    oy = ox = 0;
    if (g.mode == 2) {
        const int hi = (g.S - g.h) / g.f;            // largest feature offset whose patch stays inside the image
        oy = clamp_off(off_y, hi);
        ox = clamp_off(off_x, hi);
    }
}

__global__ __launch_bounds__(RC_BLOCK) void recon_loss_sums_kernel(const float* __restrict__ y, const float* __restrict__ t,
                                                                   float* __restrict__ img, const int32_t* off_y,
                                                                   const int32_t* off_x, ReconGeom g, int64_t total,
                                                                   double* sum) {
    __shared__ float sh[4];
    int oy, ox;
    recon_offsets(g, off_y, off_x, oy, ox);
    const int64_t row = (int64_t)g.w * g.C;
    float acc = 0.f;
    for (int64_t e = (int64_t)blockIdx.x * RC_BLOCK + threadIdx.x; e < total; e += (int64_t)gridDim.x * RC_BLOCK) {
        const int64_t q = e / row;                     // n * h + i
        const int rem = (int)(e - q * row);
        const int j = rem / g.C, c = rem - j * g.C;
        const int64_t n = q / g.h;
        const int i = (int)(q - n * g.h);
        const float v = tanhf(y[e]);
        if (img) img[e] = v;
        const float d = v - recon_target(t, g, n, i, j, c, oy, ox);
        acc = fmaf(d, d, acc);
    }
    const float s = block_sum_256(acc, sh);
    if (threadIdx.x == 0 && s != 0.f) atomicAdd(sum, (double)s);
}

__global__ void recon_loss_finalize_kernel(const double* sum, double scale, float* loss) {
    if (threadIdx.x == 0 && blockIdx.x == 0) loss[0] = (float)(sqrt(sum[0]) * scale);
}

// dy = dloss * scale * (tanh(y) - t) / sqrt(sum) * (1 - tanh(y)^2); zero at the norm's singular point sum == 0
__global__ __launch_bounds__(RC_BLOCK) void recon_loss_bwd_kernel(const float* __restrict__ y, const float* __restrict__ t,
                                                                  const int32_t* off_y, const int32_t* off_x, ReconGeom g,
                                                                  int64_t total, const double* __restrict__ sum,
                                                                  double scale, const float* __restrict__ dloss,
                                                                  float* __restrict__ dy) {
    int oy, ox;
    recon_offsets(g, off_y, off_x, oy, ox);
    const double ss = sum[0];
    const float k = ss > 0.0 ? (float)(scale / sqrt(ss)) * (dloss ? dloss[0] : 1.f) : 0.f;
    const int64_t row = (int64_t)g.w * g.C;
    for (int64_t e = (int64_t)blockIdx.x * RC_BLOCK + threadIdx.x; e < total; e += (int64_t)gridDim.x * RC_BLOCK) {
        const int64_t q = e / row;
        const int rem = (int)(e - q * row);
        const int j = rem / g.C, c = rem - j * g.C;
        const int64_t n = q / g.h;
        const int i = (int)(q - n * g.h);
        const float v = tanhf(y[e]);
        dy[e] = k * (v - recon_target(t, g, n, i, j, c, oy, ox)) * (1.f - v * v);
    }
}

// ---- launch helpers --------------------------------------------------------------------------------------------
static bool wide_ok(int dtype, int C, const void* a, const void* b, const void* c = nullptr) {
    const int per16 = dtype == BG_BF16 ? 8 : 4;
    return C % per16 == 0 && (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c) & 15) == 0;
}

}  // namespace bg

using namespace bg;

#define RC_DTYPE_OK(name) BG_REQUIRE(dtype == BG_F32 || dtype == BG_BF16, "%s: dtype %d (BG_F32 / BG_BF16)", name, dtype)

extern "C" {

// One launch of KERNEL<T, VEC> for the call's element type and access width: T is __bf16 or float, VEC the 16-byte piece
// (8 / 4) when ``wide`` and 1 otherwise; GW / GS are the grids of the two forms; the arguments may name T.
#define RC_LAUNCH(KERNEL, GW, GS, ...)                                                                 \
    do {                                                                                               \
        hipStream_t s__ = as_stream(stream);                                                           \
        if (dtype == BG_BF16) {                                                                        \
            typedef __bf16 T;                                                                          \
            if (wide) hipLaunchKernelGGL((KERNEL<T, 8>), GW, dim3(RC_BLOCK), 0, s__, __VA_ARGS__);     \
            else hipLaunchKernelGGL((KERNEL<T, 1>), GS, dim3(RC_BLOCK), 0, s__, __VA_ARGS__);          \
        } else {                                                                                       \
            typedef float T;                                                                           \
            if (wide) hipLaunchKernelGGL((KERNEL<T, 4>), GW, dim3(RC_BLOCK), 0, s__, __VA_ARGS__);     \
            else hipLaunchKernelGGL((KERNEL<T, 1>), GS, dim3(RC_BLOCK), 0, s__, __VA_ARGS__);          \
        }                                                                                              \
    } while (0)
// the same for an elementwise kernel over ``elems`` elements (wide: one thread step per 16-byte piece)
#define RC_LAUNCH_EW(KERNEL, elems, ...) \
    RC_LAUNCH(KERNEL, dim3(rc_blocks((elems) / (dtype == BG_BF16 ? 8 : 4))), dim3(rc_blocks(elems)), __VA_ARGS__)

static int rows_args(const char* name, bool ptrs, int dtype, int64_t rows, int C) {
    BG_REQUIRE(ptrs, "%s: NULL tensor", name);
    RC_DTYPE_OK(name);
    BG_REQUIRE(rows > 0 && C > 0 && rows * C < (int64_t(1) << 40), "%s: rows=%lld C=%d", name, (long long)rows, C);
    return BG_OK;
}

int bg_glu_fwd(const void* x, void* y, int dtype, int64_t rows, int C, void* stream) {
    if (int rc = rows_args("bg_glu_fwd", x && y, dtype, rows, C)) return rc;
    const bool wide = wide_ok(dtype, C, x, y);
    RC_LAUNCH_EW(glu_fwd_kernel, rows * C, (const T*)x, (T*)y, rows, C);
    BG_LAUNCH_CHECK();
    return BG_OK;
}

int bg_glu_bwd(const void* x, const void* dy, void* dx, int dtype, int64_t rows, int C, void* stream) {
    if (int rc = rows_args("bg_glu_bwd", x && dy && dx, dtype, rows, C)) return rc;
    const bool wide = wide_ok(dtype, C, x, dy, dx);
    RC_LAUNCH_EW(glu_bwd_kernel, rows * C, (const T*)x, (const T*)dy, (T*)dx, rows, C);
    BG_LAUNCH_CHECK();
    return BG_OK;
}

int bg_bn_glu_fwd(const void* x, const float* mean, const float* rstd, const float* gamma, const float* beta, void* y,
                  int dtype, int64_t rows, int C, void* stream) {
    if (int rc = rows_args("bg_bn_glu_fwd", x && y && mean && rstd && gamma && beta, dtype, rows, C)) return rc;
    const bool wide = wide_ok(dtype, C, x, y);
    const BnGluParams p{mean, rstd, gamma, beta};
    RC_LAUNCH_EW(bn_glu_fwd_kernel, rows * C, (const T*)x, p, (T*)y, rows, C);
    BG_LAUNCH_CHECK();
    return BG_OK;
}

int bg_bn_glu_bwd_reduce(const void* x, const void* dy, const float* mean, const float* rstd, const float* gamma,
                         const float* beta, float* part, int dtype, int64_t rows, int C, int nseg, void* stream) {
    if (int rc = rows_args("bg_bn_glu_bwd_reduce", x && dy && mean && rstd && gamma && beta && part, dtype, rows, C))
        return rc;
    BG_REQUIRE(nseg >= 1 && nseg <= rows && nseg <= 65535, "bg_bn_glu_bwd_reduce: nseg %d for %lld rows", nseg,
               (long long)rows);
    const bool wide = wide_ok(dtype, C, x, dy);
    const int vec = wide ? (dtype == BG_BF16 ? 8 : 4) : 1;
    const int CV = C / vec;
    const int LC = CV < RC_BLOCK ? CV : RC_BLOCK;
    const int RL = RC_BLOCK / LC;
    const int64_t rps = (rows + nseg - 1) / nseg;
    const dim3 grid((unsigned)((CV + LC - 1) / LC), (unsigned)nseg);
    const BnGluParams p{mean, rstd, gamma, beta};
    RC_LAUNCH(bn_glu_bwd_reduce_kernel, grid, grid, (const T*)x, (const T*)dy, p, part, rows, rps, C, LC, RL, nseg);
    BG_LAUNCH_CHECK();
    return BG_OK;
}

int bg_bn_glu_bwd_dx(const void* x, const void* dy, const float* mean, const float* rstd, const float* gamma,
                     const float* beta, const float* cm, void* dx, int dtype, int64_t rows, int C, void* stream) {
    if (int rc = rows_args("bg_bn_glu_bwd_dx", x && dy && mean && rstd && gamma && beta && cm && dx, dtype, rows, C))
        return rc;
    const bool wide = wide_ok(dtype, C, x, dy, dx);
    const BnGluParams p{mean, rstd, gamma, beta};
    RC_LAUNCH_EW(bn_glu_bwd_dx_kernel, rows * C, (const T*)x, (const T*)dy, p, cm, (T*)dx, rows, C);
    BG_LAUNCH_CHECK();
    return BG_OK;
}

static int map_args(const char* name, bool ptrs, int dtype, int N, int H, int W, int C) {
    BG_REQUIRE(ptrs, "%s: NULL tensor", name);
    RC_DTYPE_OK(name);
    BG_REQUIRE(N > 0 && H > 0 && W > 0 && C > 0 && (int64_t)N * H * W * C < (int64_t(1) << 38),
               "%s: N=%d H=%d W=%d C=%d", name, N, H, W, C);
    return BG_OK;
}

/* x [N,H,W,C] -> y [N,2H,2W,C] */
int bg_upsample2_fwd_t(const void* x, void* y, int dtype, int N, int H, int W, int C, void* stream) {
    if (int rc = map_args("bg_upsample2_fwd_t", x && y, dtype, N, H, W, C)) return rc;
    const bool wide = wide_ok(dtype, C, x, y);
    const int64_t NH2 = (int64_t)N * 2 * H;
    RC_LAUNCH_EW(upsample2_fwd_kernel, NH2 * 2 * W * C, (const T*)x, (T*)y, NH2, H, W, C);
    BG_LAUNCH_CHECK();
    return BG_OK;
}

/* dy [N,2H,2W,C] -> dx [N,H,W,C] (2x2 box sum) */
int bg_upsample2_bwd_t(const void* dy, void* dx, int dtype, int N, int H, int W, int C, void* stream) {
    if (int rc = map_args("bg_upsample2_bwd_t", dy && dx, dtype, N, H, W, C)) return rc;
    const bool wide = wide_ok(dtype, C, dy, dx);
    const int64_t NH = (int64_t)N * H;
    RC_LAUNCH_EW(upsample2_bwd_kernel, NH * W * C, (const T*)dy, (T*)dx, NH, H, W, C);
    BG_LAUNCH_CHECK();
    return BG_OK;
}

static int crop_args(const char* name, bool ptrs, int dtype, int N, int H, int W, int p, int C) {
    if (int rc = map_args(name, ptrs, dtype, N, H, W, C)) return rc;
    BG_REQUIRE(p > 0 && p <= H && p <= W, "%s: window p=%d on a %d x %d map", name, p, H, W);
    return BG_OK;
}

int bg_crop_at_fwd(const void* x, void* y, int dtype, const int32_t* off_y, const int32_t* off_x, int N, int H, int W,
                   int p, int C, void* stream) {
    if (int rc = crop_args("bg_crop_at_fwd", x && y && off_y && off_x, dtype, N, H, W, p, C)) return rc;
    const bool wide = wide_ok(dtype, C, x, y);
    RC_LAUNCH_EW(crop_at_fwd_kernel, (int64_t)N * p * p * C, (const T*)x, (T*)y, off_y, off_x, N, H, W, p, C);
    BG_LAUNCH_CHECK();
    return BG_OK;
}

int bg_crop_at_bwd(const void* dy, void* dx, int dtype, const int32_t* off_y, const int32_t* off_x, int N, int H, int W,
                   int p, int C, void* stream) {
    if (int rc = crop_args("bg_crop_at_bwd", dy && dx && off_y && off_x, dtype, N, H, W, p, C)) return rc;
    const bool wide = wide_ok(dtype, C, dy, dx);
    RC_LAUNCH_EW(crop_at_bwd_kernel, (int64_t)N * H * W * C, (const T*)dy, (T*)dx, off_y, off_x, N, H, W, p, C);
    BG_LAUNCH_CHECK();
    return BG_OK;
}

static int recon_args(const char* name, const void* y, const void* t, const void* acc, const int32_t* oy,
                      const int32_t* ox, int mode, int f, int N, int h, int w, int S, int C, ReconGeom* g) {
    BG_REQUIRE(y && t && acc, "%s: NULL tensor", name);
    BG_REQUIRE(mode >= 0 && mode <= 2, "%s: mode %d (0 identity, 1 2x2 average, 2 crop at offset * f)", name, mode);
    BG_REQUIRE(N > 0 && h > 0 && w > 0 && h == w && S > 0 && C > 0 && (int64_t)N * S * S * C < (int64_t(1) << 38),
               "%s: N=%d h=%d w=%d S=%d C=%d", name, N, h, w, S, C);
    if (mode == 0) BG_REQUIRE(S == h, "%s: identity target needs S == h (%d vs %d)", name, S, h);
    if (mode == 1) BG_REQUIRE(S == 2 * h, "%s: 2x2-average target needs S == 2 h (%d vs %d)", name, S, h);
    if (mode == 2) {
        BG_REQUIRE(oy && ox, "%s: crop target needs the offsets", name);
        BG_REQUIRE(f >= 1 && h <= S, "%s: crop target with f=%d h=%d S=%d", name, f, h, S);
    }
    g->h = h; g->w = w; g->S = S; g->C = C; g->mode = mode; g->f = f;
    return BG_OK;
}

int bg_recon_loss_sums(const float* y, const float* target, float* tanh_out, const int32_t* off_y, const int32_t* off_x,
                       int mode, int f, double* sum, int N, int h, int w, int S, int C, void* stream) {
    ReconGeom g;
    if (int rc = recon_args("bg_recon_loss_sums", y, target, sum, off_y, off_x, mode, f, N, h, w, S, C, &g)) return rc;
    const int64_t total = (int64_t)N * h * w * C;
    hipLaunchKernelGGL(recon_loss_sums_kernel, dim3(rc_blocks(total)), dim3(RC_BLOCK), 0, as_stream(stream), y, target,
                       tanh_out, off_y, off_x, g, total, sum);
    BG_LAUNCH_CHECK();
    return BG_OK;
}

int bg_recon_loss_finalize(const double* sum, double scale, float* loss, void* stream) {
    BG_REQUIRE(sum && loss, "bg_recon_loss_finalize: NULL tensor");
    hipLaunchKernelGGL(recon_loss_finalize_kernel, dim3(1), dim3(64), 0, as_stream(stream), sum, scale, loss);
    BG_LAUNCH_CHECK();
    return BG_OK;
}

int bg_recon_loss_bwd(const float* y, const float* target, const int32_t* off_y, const int32_t* off_x, int mode, int f,
                      const double* sum, double scale, const float* dloss, float* dy, int N, int h, int w, int S, int C,
                      void* stream) {
    ReconGeom g;
    if (int rc = recon_args("bg_recon_loss_bwd", y, target, sum, off_y, off_x, mode, f, N, h, w, S, C, &g)) return rc;
    BG_REQUIRE(dy, "bg_recon_loss_bwd: NULL dy");
    const int64_t total = (int64_t)N * h * w * C;
    hipLaunchKernelGGL(recon_loss_bwd_kernel, dim3(rc_blocks(total)), dim3(RC_BLOCK), 0, as_stream(stream), y, target,
                       off_y, off_x, g, total, sum, scale, dloss, dy);
    BG_LAUNCH_CHECK();
    return BG_OK;
}

}  // extern "C"
