// mixconv.hip - multi-branch stride-1 convolution driven by a branch table (include/biggan_hip.h, BgMixBranch).
//
// Reference call sites: clown_conv (ops.py:403-436: transposed 4x4 / 3x3 / 2x2, conv 3x3 / 5x5 and a dilated 5x5 on
// one input, concatenated along the channels), the string-kernel form of conv (ops.py:52-59) and conv(dilation=d)
// (ops.py:95).  Every branch writes its own channel slice of one output row, so the concatenation never exists as a
// separate pass; the input gradient sums all branches in registers; the weight gradient reduces split-K slabs in a
// fixed order.  bf16-resident calls (bf16 x and y, Cin % 32 == 0) run as implicit GEMMs on the bf16 MFMA; every other
// call is a direct convolution on the vector ALU with fp32 accumulation: one thread per output element (forward,
// input gradient) or per weight element and pixel slab (weight gradient).  Any branch width; no atomics.
#include "common.h"

namespace bg {

constexpr int MX_BLOCK = 256;

struct MixArgs {
    BgMixBranch br[BG_MIX_MAX_BRANCHES];
    int32_t ch_start[BG_MIX_MAX_BRANCHES + 1];     // forward: thread channel index -> branch (prefix sums of cb)
    int64_t e_start[BG_MIX_MAX_BRANCHES + 1];      // weight gradient: prefix sums of the branches' weight elements
    int32_t blk_start[BG_MIX_MAX_BRANCHES + 1];    // MFMA kernels: prefix sums of each branch's block tiles
    int32_t n, N, H, W, Cin, ldy, Ct, slabs;
    int64_t E;
};

__device__ __forceinline__ float mx_ld(const float* p, int64_t i) { return p[i]; }
__device__ __forceinline__ float mx_ld(const __bf16* p, int64_t i) { return (float)p[i]; }
__device__ __forceinline__ void mx_st(float* p, int64_t i, float v) { p[i] = v; }
__device__ __forceinline__ void mx_st(__bf16* p, int64_t i, float v) { p[i] = (__bf16)v; }
template <bool RND>
__device__ __forceinline__ float mx_r(float v) { return RND ? (float)(__bf16)v : v; }

// index of padded coordinate u in [0, n), or -1 for a zero tap (tf.pad REFLECT mirrors without repeating the border)
__device__ __forceinline__ int mx_pad(int u, int n, int mode) {
    if (u >= 0 && u < n) return u;
    if (mode == BG_PAD_ZERO) return -1;
    return u < 0 ? -u : 2 * (n - 1) - u;
}

// the padded coordinates that read input coordinate p (the adjoint of mx_pad)
__device__ __forceinline__ int mx_sources(int p, int n, int mode, int (&u)[3]) {
    int m = 0;
    u[m++] = p;
    if (mode == BG_PAD_REFLECT) {
        if (p > 0) u[m++] = -p;
        if (p < n - 1) u[m++] = 2 * (n - 1) - p;
    }
    return m;
}

// y[pix, c_off + c] = bias[c] + sum_taps sum_ci x * W;  one thread per (pixel, channel of the union of the branches)
template <typename XT, typename YT, bool RND>
__global__ __launch_bounds__(MX_BLOCK) void mix_fwd_kernel(const MixArgs a, const XT* __restrict__ x,
                                                            YT* __restrict__ y) {
    const int64_t t = (int64_t)blockIdx.x * MX_BLOCK + threadIdx.x;
    const int64_t P = (int64_t)a.N * a.H * a.W;
    if (t >= P * a.Ct) return;
    const int64_t pix = t / a.Ct;
    const int cc = (int)(t - pix * a.Ct);
    int b = 0;
    while (b + 1 < a.n && a.ch_start[b + 1] <= cc) ++b;
    const BgMixBranch& br = a.br[b];
    const int c = cc - a.ch_start[b];
    const int q = (int)(pix % a.W);
    const int64_t np = pix / a.W;
    const int p = (int)(np % a.H);
    const int n = (int)(np / a.H);
    const int k = br.k, cb = br.cb, Cin = a.Cin;
    float acc = br.bias ? br.bias[c] : 0.f;
    for (int i = 0; i < k; ++i) {
        const int r = mx_pad(p - br.lo + i * br.dil, a.H, br.pad_mode);
        if (r < 0) continue;
        for (int j = 0; j < k; ++j) {
            const int s = mx_pad(q - br.lo + j * br.dil, a.W, br.pad_mode);
            if (s < 0) continue;
            const XT* xp = x + ((int64_t)(n * a.H + r) * a.W + s) * Cin;
            if (!br.transposed) {
                const float* wp = br.w + (int64_t)(i * k + j) * Cin * cb + c;
                for (int ci = 0; ci < Cin; ++ci)
                    acc = fmaf(mx_r<RND>(mx_ld(xp, ci)), mx_r<RND>(wp[(int64_t)ci * cb]), acc);
            } else {
                const float* wp = br.w + ((int64_t)((k - 1 - i) * k + (k - 1 - j)) * cb + c) * Cin;
                for (int ci = 0; ci < Cin; ++ci)
                    acc = fmaf(mx_r<RND>(mx_ld(xp, ci)), mx_r<RND>(wp[ci]), acc);
            }
        }
    }
    mx_st(y, pix * a.ldy + br.c_off + c, acc);
}

// dx[pix, ci] (+)= sum_branches sum_taps sum over the outputs that read (pix, ci) of dy * W;  one thread per element
template <typename XT, typename YT, bool RND>
__global__ __launch_bounds__(MX_BLOCK) void mix_dgrad_kernel(const MixArgs a, const YT* __restrict__ dy,
                                                              XT* __restrict__ dx, int accumulate) {
    const int64_t t = (int64_t)blockIdx.x * MX_BLOCK + threadIdx.x;
    const int Cin = a.Cin;
    const int64_t P = (int64_t)a.N * a.H * a.W;
    if (t >= P * Cin) return;
    const int64_t pix = t / Cin;
    const int ci = (int)(t - pix * Cin);
    const int q = (int)(pix % a.W);
    const int64_t np = pix / a.W;
    const int p = (int)(np % a.H);
    const int n = (int)(np / a.H);
    float acc = 0.f;
    for (int b = 0; b < a.n; ++b) {
        const BgMixBranch& br = a.br[b];
        const int k = br.k, cb = br.cb;
        int us[3], vs[3];
        const int nu = mx_sources(p, a.H, br.pad_mode, us);
        const int nv = mx_sources(q, a.W, br.pad_mode, vs);
        for (int i = 0; i < k; ++i) {
            for (int iu = 0; iu < nu; ++iu) {
                const int orow = us[iu] + br.lo - i * br.dil;
                if (orow < 0 || orow >= a.H) continue;
                for (int j = 0; j < k; ++j) {
                    for (int iv = 0; iv < nv; ++iv) {
                        const int ocol = vs[iv] + br.lo - j * br.dil;
                        if (ocol < 0 || ocol >= a.W) continue;
                        const YT* dp = dy + ((int64_t)(n * a.H + orow) * a.W + ocol) * a.ldy + br.c_off;
                        if (!br.transposed) {
                            const float* wp = br.w + ((int64_t)(i * k + j) * Cin + ci) * cb;
                            for (int c = 0; c < cb; ++c)
                                acc = fmaf(mx_r<RND>(mx_ld(dp, c)), mx_r<RND>(wp[c]), acc);
                        } else {
                            const float* wp = br.w + (int64_t)((k - 1 - i) * k + (k - 1 - j)) * cb * Cin + ci;
                            for (int c = 0; c < cb; ++c)
                                acc = fmaf(mx_r<RND>(mx_ld(dp, c)), mx_r<RND>(wp[(int64_t)c * Cin]), acc);
                        }
                    }
                }
            }
        }
    }
    if (accumulate) acc = mx_ld(dx, t) + acc;
    mx_st(dx, t, acc);
}

// ws[slab, e] = sum over the slab's image rows of x * dy for weight element e (branch order, [k,k,Cin,cb] inside a
// branch);  blockIdx.y = slab of whole image rows
template <typename XT, typename YT, bool RND>
__global__ __launch_bounds__(MX_BLOCK) void mix_wgrad_kernel(const MixArgs a, const XT* __restrict__ x,
                                                              const YT* __restrict__ dy, float* __restrict__ ws) {
    const int64_t e = (int64_t)blockIdx.x * MX_BLOCK + threadIdx.x;
    if (e >= a.E) return;
    int b = 0;
    while (b + 1 < a.n && a.e_start[b + 1] <= e) ++b;
    const BgMixBranch& br = a.br[b];
    if (!br.dw) return;
    const int64_t el = e - a.e_start[b];
    const int cb = br.cb, Cin = a.Cin, k = br.k;
    const int c = (int)(el % cb);
    const int64_t rest = el / cb;
    const int ci = (int)(rest % Cin);
    const int tap = (int)(rest / Cin);
    const int i = tap / k, j = tap - (tap / k) * k;
    const int64_t rows = (int64_t)a.N * a.H;
    const int64_t r0 = rows * blockIdx.y / a.slabs, r1 = rows * (blockIdx.y + 1) / a.slabs;
    float acc = 0.f;
    for (int64_t row = r0; row < r1; ++row) {
        const int n = (int)(row / a.H), p = (int)(row - (int64_t)n * a.H);
        const int r = mx_pad(p - br.lo + i * br.dil, a.H, br.pad_mode);
        if (r < 0) continue;
        const XT* xr = x + (int64_t)(n * a.H + r) * a.W * Cin + ci;
        const YT* dr = dy + row * a.W * a.ldy + br.c_off + c;
        for (int q = 0; q < a.W; ++q) {
            const int s = mx_pad(q - br.lo + j * br.dil, a.W, br.pad_mode);
            if (s < 0) continue;
            acc = fmaf(mx_r<RND>(mx_ld(xr, (int64_t)s * Cin)), mx_r<RND>(mx_ld(dr, (int64_t)q * a.ldy)), acc);
        }
    }
    ws[(int64_t)blockIdx.y * a.E + e] = acc;
}

// dw (+)= sum over the slabs in slab order, written in the variable's layout ([k,k,cb,Cin] flipped for transposed)
__global__ __launch_bounds__(MX_BLOCK) void mix_wgrad_finish_kernel(const MixArgs a, const float* __restrict__ ws) {
    const int64_t e = (int64_t)blockIdx.x * MX_BLOCK + threadIdx.x;
    if (e >= a.E) return;
    int b = 0;
    while (b + 1 < a.n && a.e_start[b + 1] <= e) ++b;
    const BgMixBranch& br = a.br[b];
    if (!br.dw) return;
    float v = 0.f;
    for (int s = 0; s < a.slabs; ++s) v += ws[(int64_t)s * a.E + e];
    int64_t el = e - a.e_start[b];
    if (br.transposed) {
        const int cb = br.cb, Cin = a.Cin, k = br.k;
        const int c = (int)(el % cb);
        const int64_t rest = el / cb;
        const int ci = (int)(rest % Cin);
        const int tap = (int)(rest / Cin);
        const int i = tap / k, j = tap - (tap / k) * k;
        el = ((int64_t)((k - 1 - i) * k + (k - 1 - j)) * cb + c) * Cin + ci;
    }
    if (br.acc_w) v = br.dw[el] + v;
    br.dw[el] = v;
}


// ---- bf16-resident path: implicit GEMM on v_mfma_f32_16x16x32_bf16 ----------------------------------------------
// Taken when x and y / dy are bf16 and Cin % 32 == 0 (every generator level).  Each wave owns a 64 x 16 output tile:
// four 16 x 16 MFMA accumulators that share the B fragment of every K step; a block is 4 waves side by side along N.
// Lane l holds A[row l&15][k = 8(l>>4) + j] and B[k = 8(l>>4) + j][col l&15] (j < 8); the accumulator holds
// C[row (l>>4)*4 + r][col l&15].  Operands are gathered straight from global memory (no LDS): x rows are 16-byte bf16
// vectors, the fp32 branch kernels are rounded to bf16 (RNE) as they are read.  fp32 accumulation; every output
// element is written by one lane, so results do not depend on timing.
typedef short mx_v8s __attribute__((ext_vector_type(8)));
typedef float mx_v4f __attribute__((ext_vector_type(4)));

__device__ __forceinline__ short mx_bits(float v) { return __builtin_bit_cast(short, (__bf16)v); }
__device__ __forceinline__ int mx_find_blk(const MixArgs& a, int blk) {
    int b = 0;
    while (b + 1 < a.n && a.blk_start[b + 1] <= blk) ++b;
    return b;
}
__device__ __forceinline__ mx_v4f mx_mfma(const mx_v8s& A, const mx_v8s& B, const mx_v4f& C) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(A, B, C, 0, 0, 0);
}

// forward: rows = 64 output pixels (blockIdx.x), cols = 16 channels per wave (blockIdx.y: branch, 64-channel block)
__global__ __launch_bounds__(MX_BLOCK) void mix_fwd_mfma_kernel(const MixArgs a, const __bf16* __restrict__ x,
                                                                 __bf16* __restrict__ y) {
    const int b = mx_find_blk(a, blockIdx.y);
    const BgMixBranch& br = a.br[b];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, r = lane & 15, kh = lane >> 4;
    const int c0 = ((blockIdx.y - a.blk_start[b]) * 4 + wave) * 16;
    if (c0 >= br.cb) return;
    const int64_t P = (int64_t)a.N * a.H * a.W;
    const int k = br.k, cb = br.cb, Cin = a.Cin, HW = a.H * a.W;
    int64_t pix[4];
    int n[4], p[4], q[4];
    for (int t = 0; t < 4; ++t) {
        pix[t] = (int64_t)blockIdx.x * 64 + t * 16 + r;
        const int64_t pc = pix[t] < P ? pix[t] : P - 1;
        n[t] = (int)(pc / HW);
        const int rem = (int)(pc - (int64_t)n[t] * HW);
        p[t] = rem / a.W;
        q[t] = rem - p[t] * a.W;
    }
    const int c = c0 + r;
    mx_v4f acc[4];
    for (int t = 0; t < 4; ++t) acc[t] = mx_v4f{0.f, 0.f, 0.f, 0.f};
    const mx_v8s zero = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int i = 0; i < k; ++i)
        for (int j = 0; j < k; ++j) {
            int64_t src[4];
            for (int t = 0; t < 4; ++t) {
                const int rr = mx_pad(p[t] - br.lo + i * br.dil, a.H, br.pad_mode);
                const int ss = mx_pad(q[t] - br.lo + j * br.dil, a.W, br.pad_mode);
                src[t] = (pix[t] < P && rr >= 0 && ss >= 0) ? ((int64_t)(n[t] * a.H + rr) * a.W + ss) * Cin : -1;
            }
            const float* wt = br.transposed ? br.w + ((int64_t)((k - 1 - i) * k + (k - 1 - j)) * cb + c) * Cin
                                            : br.w + (int64_t)(i * k + j) * Cin * cb + c;
            for (int ci0 = 0; ci0 < Cin; ci0 += 32) {
                const int ci = ci0 + 8 * kh;
                mx_v8s B = zero;
                if (c < cb) {
                    const int64_t st = br.transposed ? 1 : cb;
                    for (int e = 0; e < 8; ++e) B[e] = mx_bits(wt[(int64_t)(ci + e) * st]);
                }
                for (int t = 0; t < 4; ++t) {
                    const mx_v8s A = src[t] >= 0 ? *reinterpret_cast<const mx_v8s*>(x + src[t] + ci) : zero;
                    acc[t] = mx_mfma(A, B, acc[t]);
                }
            }
        }
    const int cw = c0 + r;
    if (cw >= cb) return;
    const float bv = br.bias ? br.bias[cw] : 0.f;
    for (int t = 0; t < 4; ++t)
        for (int e = 0; e < 4; ++e) {
            const int64_t m = (int64_t)blockIdx.x * 64 + t * 16 + kh * 4 + e;
            if (m < P) y[m * a.ldy + br.c_off + cw] = (__bf16)(acc[t][e] + bv);
        }
}

// input gradient: rows = 64 input pixels (blockIdx.x), cols = 16 input channels per wave (blockIdx.y: 64-channel
// block); K = branches x taps x padded sources x branch channels.  The padded sources (reflect: up to three per axis)
// of a row are visited only when some lane of the wave has one.
__global__ __launch_bounds__(MX_BLOCK) void mix_dgrad_mfma_kernel(const MixArgs a, const __bf16* __restrict__ dy,
                                                                   __bf16* __restrict__ dx, int accumulate) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, r = lane & 15, kh = lane >> 4;
    const int ci0 = (blockIdx.y * 4 + wave) * 16;
    const int Cin = a.Cin;
    if (ci0 >= Cin) return;
    const int64_t P = (int64_t)a.N * a.H * a.W;
    const int HW = a.H * a.W;
    int64_t pix[4];
    int n[4], p[4], q[4];
    for (int t = 0; t < 4; ++t) {
        pix[t] = (int64_t)blockIdx.x * 64 + t * 16 + r;
        const int64_t pc = pix[t] < P ? pix[t] : P - 1;
        n[t] = (int)(pc / HW);
        const int rem = (int)(pc - (int64_t)n[t] * HW);
        p[t] = rem / a.W;
        q[t] = rem - p[t] * a.W;
    }
    const int ci = ci0 + r;
    mx_v4f acc[4];
    for (int t = 0; t < 4; ++t) acc[t] = mx_v4f{0.f, 0.f, 0.f, 0.f};
    const mx_v8s zero = {0, 0, 0, 0, 0, 0, 0, 0};
    const short* dys = reinterpret_cast<const short*>(dy);
    for (int b = 0; b < a.n; ++b) {
        const BgMixBranch& br = a.br[b];
        const int k = br.k, cb = br.cb;
        int us[4][3], vs[4][3], nu[4], nv[4];
        for (int t = 0; t < 4; ++t) {
            nu[t] = mx_sources(p[t], a.H, br.pad_mode, us[t]);
            nv[t] = mx_sources(q[t], a.W, br.pad_mode, vs[t]);
        }
        for (int i = 0; i < k; ++i)
            for (int iu = 0; iu < 3; ++iu)
                for (int j = 0; j < k; ++j)
                    for (int iv = 0; iv < 3; ++iv) {
                        int64_t off[4];
                        bool any = false;
                        for (int t = 0; t < 4; ++t) {
                            off[t] = -1;
                            if (pix[t] < P && iu < nu[t] && iv < nv[t]) {
                                const int orow = us[t][iu] + br.lo - i * br.dil;
                                const int ocol = vs[t][iv] + br.lo - j * br.dil;
                                if (orow >= 0 && orow < a.H && ocol >= 0 && ocol < a.W)
                                    off[t] = ((int64_t)(n[t] * a.H + orow) * a.W + ocol) * a.ldy + br.c_off;
                            }
                            any |= off[t] >= 0;
                        }
                        if (!__any(any)) continue;
                        const float* wt = br.transposed ? br.w + (int64_t)((k - 1 - i) * k + (k - 1 - j)) * cb * Cin + ci
                                                        : br.w + ((int64_t)(i * k + j) * Cin + ci) * cb;
                        for (int cc = 0; cc < cb; cc += 32) {
                            const int c = cc + 8 * kh;
                            mx_v8s B = zero;
                            if (ci < Cin)
                                for (int e = 0; e < 8; ++e)
                                    if (c + e < cb) B[e] = mx_bits(br.transposed ? wt[(int64_t)(c + e) * Cin] : wt[c + e]);
                            for (int t = 0; t < 4; ++t) {
                                mx_v8s A = zero;
                                if (off[t] >= 0)
                                    for (int e = 0; e < 8; ++e)
                                        if (c + e < cb) A[e] = dys[off[t] + c + e];
                                acc[t] = mx_mfma(A, B, acc[t]);
                            }
                        }
                    }
    }
    if (ci >= Cin) return;
    for (int t = 0; t < 4; ++t)
        for (int e = 0; e < 4; ++e) {
            const int64_t m = (int64_t)blockIdx.x * 64 + t * 16 + kh * 4 + e;
            if (m >= P) continue;
            float v = acc[t][e];
            if (accumulate) v = (float)dx[m * Cin + ci] + v;
            dx[m * Cin + ci] = (__bf16)v;
        }
}

// weight gradient: rows = 64 input channels, cols = 16 branch channels per wave, K = the pixels of one slab
// (blockIdx.y); blockIdx.x = (branch, tap, 64-channel block of Cin, 64-channel block of cb).  Partial sums go to
// ws[slab][e] like mix_wgrad_kernel's, reduced in slab order by mix_wgrad_finish_kernel.
__global__ __launch_bounds__(MX_BLOCK) void mix_wgrad_mfma_kernel(const MixArgs a, const __bf16* __restrict__ x,
                                                                   const __bf16* __restrict__ dy, float* __restrict__ ws) {
    const int b = mx_find_blk(a, blockIdx.x);
    const BgMixBranch& br = a.br[b];
    if (!br.dw) return;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, r = lane & 15, kh = lane >> 4;
    const int Cin = a.Cin, k = br.k, cb = br.cb;
    const int nci = (Cin + 63) / 64, ncb = (cb + 63) / 64;
    int rest = blockIdx.x - a.blk_start[b];
    const int cbk = rest % ncb;
    rest /= ncb;
    const int cik = rest % nci;
    const int tap = rest / nci;
    const int i = tap / k, j = tap - (tap / k) * k;
    const int c0 = (cbk * 4 + wave) * 16;
    if (c0 >= cb) return;
    const int c = c0 + r;
    const int64_t P = (int64_t)a.N * a.H * a.W;
    const int64_t p0 = P * blockIdx.y / a.slabs, p1 = P * (blockIdx.y + 1) / a.slabs;
    const int HW = a.H * a.W;
    const short* xs = reinterpret_cast<const short*>(x);
    const short* dys = reinterpret_cast<const short*>(dy);
    mx_v4f acc[4];
    for (int t = 0; t < 4; ++t) acc[t] = mx_v4f{0.f, 0.f, 0.f, 0.f};
    for (int64_t pk = p0; pk < p1; pk += 32) {
        int64_t xo[8], yo[8];
        int64_t m = pk + 8 * kh;
        int nn = (int)(m / HW);
        int rem = (int)(m - (int64_t)nn * HW);
        int pp = rem / a.W, qq = rem - (rem / a.W) * a.W;
        for (int e = 0; e < 8; ++e) {
            xo[e] = yo[e] = -1;
            if (m + e < p1) {
                const int rr = mx_pad(pp - br.lo + i * br.dil, a.H, br.pad_mode);
                const int ss = mx_pad(qq - br.lo + j * br.dil, a.W, br.pad_mode);
                if (rr >= 0 && ss >= 0) {
                    xo[e] = ((int64_t)(nn * a.H + rr) * a.W + ss) * Cin;
                    yo[e] = (m + e) * a.ldy + br.c_off;
                }
            }
            if (++qq == a.W) {
                qq = 0;
                if (++pp == a.H) { pp = 0; ++nn; }
            }
        }
        mx_v8s B;
        for (int e = 0; e < 8; ++e) B[e] = (yo[e] >= 0 && c < cb) ? dys[yo[e] + c] : (short)0;
        for (int t = 0; t < 4; ++t) {
            const int ci = cik * 64 + t * 16 + r;
            mx_v8s A;
            for (int e = 0; e < 8; ++e) A[e] = (xo[e] >= 0 && ci < Cin) ? xs[xo[e] + ci] : (short)0;
            acc[t] = mx_mfma(A, B, acc[t]);
        }
    }
    if (c >= cb) return;
    float* out = ws + (int64_t)blockIdx.y * a.E + a.e_start[b];
    for (int t = 0; t < 4; ++t)
        for (int e = 0; e < 4; ++e) {
            const int ci = cik * 64 + t * 16 + kh * 4 + e;
            if (ci < Cin) out[((int64_t)tap * Cin + ci) * cb + c] = acc[t][e];
        }
}

// ---- host side ------------------------------------------------------------------------------------------------
static int mix_prepare(const BgConvDesc* d, const void* table, int nb, int ldy, MixArgs& a, const char* who) {
    BG_REQUIRE(d && table, "%s: NULL descriptor or branch table", who);
    BG_REQUIRE(nb >= 1 && nb <= BG_MIX_MAX_BRANCHES, "%s: %d branches (1 ... %d)", who, nb, BG_MIX_MAX_BRANCHES);
    BG_REQUIRE(d->N > 0 && d->H > 0 && d->W > 0 && d->Cin > 0 && d->stride == 1 && d->Ho == d->H && d->Wo == d->W,
               "%s: stride-1 geometry with Ho = H, Wo = W expected", who);
    BG_REQUIRE((d->x_dtype == BG_F32 || d->x_dtype == BG_BF16) && (d->y_dtype == BG_F32 || d->y_dtype == BG_BF16) &&
                   (d->compute == BG_COMPUTE_F32 || d->compute == BG_COMPUTE_BF16),
               "%s: bad dtype / compute field", who);
    const BgMixBranch* t = static_cast<const BgMixBranch*>(table);
    memset(&a, 0, sizeof(a));
    a.n = nb;
    a.N = d->N; a.H = d->H; a.W = d->W; a.Cin = d->Cin; a.ldy = ldy;
    int64_t E = 0;
    int Ct = 0;
    for (int b = 0; b < nb; ++b) {
        const BgMixBranch& br = t[b];
        BG_REQUIRE(br.w && br.cb > 0 && br.k >= 1 && br.dil >= 1 && br.lo >= 0 && br.c_off >= 0 &&
                       br.c_off + br.cb <= ldy && (br.pad_mode == BG_PAD_REFLECT || br.pad_mode == BG_PAD_ZERO),
                   "%s: bad branch %d (w, cb, k, dil, lo, c_off + cb <= ldy %d, pad_mode)", who, b, ldy);
        if (br.pad_mode == BG_PAD_REFLECT) {
            const int hi = (br.k - 1) * br.dil - br.lo;
            BG_REQUIRE(br.lo <= d->H - 1 && br.lo <= d->W - 1 && hi <= d->H - 1 && hi <= d->W - 1,
                       "%s: branch %d: reflect padding wider than the image minus one (%dx%d, lo %d, hi %d)", who, b,
                       d->H, d->W, br.lo, hi);
        }
        a.br[b] = br;
        a.ch_start[b] = Ct;
        a.e_start[b] = E;
        Ct += br.cb;
        E += (int64_t)br.k * br.k * d->Cin * br.cb;
    }
    a.ch_start[nb] = Ct;
    a.e_start[nb] = E;
    a.Ct = Ct;
    a.E = E;
    return BG_OK;
}

// the bf16-resident MFMA kernels serve a call whose x and y / dy are bf16 with Cin % 32 == 0 and a 16-byte aligned x
static bool mx_mfma_ok(const BgConvDesc* d, const void* x) {
    return d->x_dtype == BG_BF16 && d->y_dtype == BG_BF16 && d->Cin % 32 == 0 && ((uintptr_t)x & 15) == 0;
}

// blocks per branch of the MFMA weight gradient: taps x 64-channel blocks of Cin x 64-channel blocks of cb
static void mx_wgrad_blocks(MixArgs& a) {
    int s = 0;
    for (int b = 0; b < a.n; ++b) {
        a.blk_start[b] = s;
        s += a.br[b].k * a.br[b].k * ((a.Cin + 63) / 64) * ((a.br[b].cb + 63) / 64);
    }
    a.blk_start[a.n] = s;
}

static int mix_slabs(const MixArgs& a, bool mfma) {
    if (mfma) {              // >= 2048 blocks in all, >= 256 pixels per slab
        const int64_t P = (int64_t)a.N * a.H * a.W;
        const int64_t blocks = a.blk_start[a.n] > 0 ? a.blk_start[a.n] : 1;
        int64_t s = (2048 + blocks - 1) / blocks;
        if (s > P / 256) s = P / 256;
        if (s > 1024) s = 1024;
        return (int)(s < 1 ? 1 : s);
    }
    const int64_t rows = (int64_t)a.N * a.H;
    int64_t s = ((int64_t)1 << 21) / (a.E > 0 ? a.E : 1);
    if (s < 1) s = 1;
    if (s > rows) s = rows;
    if (s > 1024) s = 1024;
    return (int)s;
}

static inline unsigned mx_blocks(int64_t n) { return (unsigned)((n + MX_BLOCK - 1) / MX_BLOCK); }

// picks the <x type, y type, rounding> instantiation of a host launcher template
#define MX_DISPATCH(d, LAUNCHER, ...)                                                                                  \
    do {                                                                                                               \
        if (d->x_dtype == BG_F32 && d->y_dtype == BG_F32) {                                                            \
            if (d->compute == BG_COMPUTE_BF16) LAUNCHER<float, float, true>(__VA_ARGS__);                              \
            else LAUNCHER<float, float, false>(__VA_ARGS__);                                                           \
        } else if (d->x_dtype == BG_F32) {                                                                             \
            LAUNCHER<float, __bf16, true>(__VA_ARGS__);                                                                \
        } else if (d->y_dtype == BG_F32) {                                                                             \
            LAUNCHER<__bf16, float, true>(__VA_ARGS__);                                                                \
        } else {                                                                                                       \
            LAUNCHER<__bf16, __bf16, true>(__VA_ARGS__);                                                               \
        }                                                                                                              \
    } while (0)

// (a bf16 tensor on either side, or compute = BG_COMPUTE_BF16: both factors of every product are rounded to bf16)
template <typename XT, typename YT, bool RND>
static void mix_fwd_launch(const MixArgs& a, const void* x, void* y, hipStream_t s) {
    const int64_t total = (int64_t)a.N * a.H * a.W * a.Ct;
    hipLaunchKernelGGL((mix_fwd_kernel<XT, YT, RND>), dim3(mx_blocks(total)), dim3(MX_BLOCK), 0, s, a,
                       static_cast<const XT*>(x), static_cast<YT*>(y));
}

template <typename XT, typename YT, bool RND>
static void mix_dgrad_launch(const MixArgs& a, const void* dy, void* dx, int accumulate, hipStream_t s) {
    const int64_t total = (int64_t)a.N * a.H * a.W * a.Cin;
    hipLaunchKernelGGL((mix_dgrad_kernel<XT, YT, RND>), dim3(mx_blocks(total)), dim3(MX_BLOCK), 0, s, a,
                       static_cast<const YT*>(dy), static_cast<XT*>(dx), accumulate);
}

template <typename XT, typename YT, bool RND>
static void mix_wgrad_launch(const MixArgs& a, const void* x, const void* dy, float* ws, hipStream_t s) {
    hipLaunchKernelGGL((mix_wgrad_kernel<XT, YT, RND>), dim3(mx_blocks(a.E), a.slabs), dim3(MX_BLOCK), 0, s, a,
                       static_cast<const XT*>(x), static_cast<const YT*>(dy), ws);
}

}  // namespace bg

using namespace bg;

extern "C" {

int bg_mixconv_fwd(const BgConvDesc* d, const void* table, int nb, const void* x, void* y, int ldy, void* stream) {
    MixArgs a;
    const int rc = mix_prepare(d, table, nb, ldy, a, "bg_mixconv_fwd");
    if (rc) return rc;
    BG_REQUIRE(x && y, "bg_mixconv_fwd: NULL tensor");
    if (mx_mfma_ok(d, x)) {
        int s = 0;
        for (int b = 0; b < nb; ++b) {
            a.blk_start[b] = s;
            s += (a.br[b].cb + 63) / 64;
        }
        a.blk_start[nb] = s;
        const int64_t P = (int64_t)a.N * a.H * a.W;
        hipLaunchKernelGGL(mix_fwd_mfma_kernel, dim3((unsigned)((P + 63) / 64), s), dim3(MX_BLOCK), 0,
                           as_stream(stream), a, static_cast<const __bf16*>(x), static_cast<__bf16*>(y));
        BG_LAUNCH_CHECK();
        return BG_OK;
    }
    MX_DISPATCH(d, mix_fwd_launch, a, x, y, as_stream(stream));
    BG_LAUNCH_CHECK();
    return BG_OK;
}

int bg_mixconv_dgrad(const BgConvDesc* d, const void* table, int nb, const void* dy, int ldy, void* dx, int accumulate,
                     void* stream) {
    MixArgs a;
    const int rc = mix_prepare(d, table, nb, ldy, a, "bg_mixconv_dgrad");
    if (rc) return rc;
    BG_REQUIRE(dy && dx, "bg_mixconv_dgrad: NULL tensor");
    if (mx_mfma_ok(d, dx)) {
        const int64_t P = (int64_t)a.N * a.H * a.W;
        hipLaunchKernelGGL(mix_dgrad_mfma_kernel, dim3((unsigned)((P + 63) / 64), (unsigned)((a.Cin + 63) / 64)),
                           dim3(MX_BLOCK), 0, as_stream(stream), a, static_cast<const __bf16*>(dy),
                           static_cast<__bf16*>(dx), accumulate);
        BG_LAUNCH_CHECK();
        return BG_OK;
    }
    MX_DISPATCH(d, mix_dgrad_launch, a, dy, dx, accumulate, as_stream(stream));
    BG_LAUNCH_CHECK();
    return BG_OK;
}

size_t bg_mixconv_wgrad_workspace_bytes(const BgConvDesc* d, const void* table, int nb) {
    MixArgs a;
    if (mix_prepare(d, table, nb, 1 << 30, a, "bg_mixconv_wgrad_workspace_bytes")) return 0;
    const bool mfma = d->x_dtype == BG_BF16 && d->y_dtype == BG_BF16 && d->Cin % 32 == 0;
    if (mfma) mx_wgrad_blocks(a);
    return (size_t)mix_slabs(a, mfma) * (size_t)a.E * sizeof(float);
}

int bg_mixconv_wgrad(const BgConvDesc* d, const void* table, int nb, const void* x, const void* dy, int ldy, void* ws,
                     size_t ws_bytes, void* stream) {
    MixArgs a;
    const int rc = mix_prepare(d, table, nb, ldy, a, "bg_mixconv_wgrad");
    if (rc) return rc;
    BG_REQUIRE(x && dy && ws, "bg_mixconv_wgrad: NULL tensor or workspace");
    bool any_dw = false;
    for (int b = 0; b < nb; ++b) any_dw |= a.br[b].dw != nullptr;
    BG_REQUIRE(any_dw, "bg_mixconv_wgrad: no branch has a dw");
    // (the slab count follows the dtypes alone, as in bg_mixconv_wgrad_workspace_bytes; x alignment picks the kernel)
    const bool mfma_shape = d->x_dtype == BG_BF16 && d->y_dtype == BG_BF16 && d->Cin % 32 == 0;
    if (mfma_shape) mx_wgrad_blocks(a);
    a.slabs = mix_slabs(a, mfma_shape);
    BG_REQUIRE(ws_bytes >= (size_t)a.slabs * (size_t)a.E * sizeof(float),
               "bg_mixconv_wgrad: workspace of %zu bytes < bg_mixconv_wgrad_workspace_bytes", ws_bytes);
    hipStream_t s = as_stream(stream);
    if (mfma_shape)
        hipLaunchKernelGGL(mix_wgrad_mfma_kernel, dim3(a.blk_start[nb], a.slabs), dim3(MX_BLOCK), 0, s, a,
                           static_cast<const __bf16*>(x), static_cast<const __bf16*>(dy), static_cast<float*>(ws));
    else
        MX_DISPATCH(d, mix_wgrad_launch, a, x, dy, static_cast<float*>(ws), s);
    hipLaunchKernelGGL(mix_wgrad_finish_kernel, dim3(mx_blocks(a.E)), dim3(MX_BLOCK), 0, s, a,
                       static_cast<const float*>(ws));
    BG_LAUNCH_CHECK();
    return BG_OK;
}

}  // extern "C"
