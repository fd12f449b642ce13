// subpixel.hip - tf.nn.depth_to_space and its inverse (ops.py:23-27 subpixel_conv: --upsampling_method subpixel2 /
// subpixel3), NHWC, fp32 or bf16.
//
//   depth_to_space: x[N,H,W,r*r*C] -> y[N,r*H,r*W,C],  y[n, h*r+i, w*r+j, c] = x[n, h, w, (i*r+j)*C + c]
//   space_to_depth: the inverse permutation, which is also its adjoint (the backward pass gathers dy with it).
//
// Both are one batched transpose.  Row (n, h*r+i) of the high-resolution tensor is the concatenation over w of the
// CONTIGUOUS runs x[n, h, w, i*r*C .. (i+1)*r*C): with L = the 16-byte pieces of such a run and q = n*H + h,
//   low-resolution  piece index = ((q*W + w)*r + i)*L + l        high-resolution piece index = ((q*r + i)*W + w)*L + l
// so one kernel serves both directions: dst = ((q*RA + a)*RB + b)*L + l, src = ((q*RB + b)*RA + a)*L + l with
// (RA, RB) = (r, W) for depth_to_space and (W, r) for space_to_depth.  Pure HBM-bound copies: every thread moves
// 16-byte pieces in destination order (stores fully coalesced, loads in runs of L pieces >= 32 bytes), the grid is sized
// by bytes, and the mixed-radix digits (q, a, b, l) of a thread's piece advance by the digits of the grid stride with
// compare-and-subtract carries - the only integer divisions are the three that split a thread's FIRST piece (the same
// reasoning as the row decomposition of igemm16.hip's nn16_row: a division is ~40 VALU instructions, a piece is one load
// and one store).
#include "common.h"

namespace bg {

#define SHUF_BLOCK 256
#define SHUF_UNROLL 4
#define SHUF_MAX_BLOCKS 4096

struct ShufParams {
    const uint4* src;
    uint4* dst;
    int64_t total;          // 16-byte pieces
    int32_t RA, RB, L;      // radices of the two transposed digits, pieces per run
    int64_t sq;             // digits of the grid stride (gridDim.x * SHUF_BLOCK pieces)
    int32_t sa, sb, sl;
};

__global__ __launch_bounds__(SHUF_BLOCK) void subpixel_shuffle_kernel(const ShufParams p) {
    const int64_t S = (int64_t)gridDim.x * SHUF_BLOCK;
    int64_t u = (int64_t)blockIdx.x * SHUF_BLOCK + threadIdx.x;
    if (u >= p.total) return;
    int l, a, b;
    int64_t q;
    {
        int64_t t = u / p.L;
        l = (int)(u - t * p.L);
        const int64_t t2 = t / p.RB;
        b = (int)(t - t2 * p.RB);
        q = t2 / p.RA;
        a = (int)(t2 - q * p.RA);
    }
    for (; u < p.total; u += SHUF_UNROLL * S) {
        uint4 v[SHUF_UNROLL];
        bool live[SHUF_UNROLL];
#pragma unroll
        for (int k = 0; k < SHUF_UNROLL; ++k) {
            live[k] = u + k * S < p.total;
            if (live[k]) v[k] = p.src[((q * p.RB + b) * p.RA + a) * (int64_t)p.L + l];
            // digits of the next piece (every addend is below its radix: one conditional subtraction per digit)
            l += p.sl;
            int c = l >= p.L;
            l -= c ? p.L : 0;
            b += p.sb + c;
            c = b >= p.RB;
            b -= c ? p.RB : 0;
            a += p.sa + c;
            c = a >= p.RA;
            a -= c ? p.RA : 0;
            q += p.sq + c;
        }
#pragma unroll
        for (int k = 0; k < SHUF_UNROLL; ++k)
            if (live[k]) p.dst[u + k * S] = v[k];
    }
}

// x, y: the source and destination of the permutation; low-resolution map H x W, C channels per sub-pixel
static int launch_shuffle(const char* name, const void* x, void* y, int dtype, int N, int H, int W, int C, int r,
                          bool to_space, void* stream) {
    BG_REQUIRE(x && y, "%s: NULL tensor", name);
    BG_REQUIRE(dtype == BG_F32 || dtype == BG_BF16, "%s: dtype %d (BG_F32 / BG_BF16)", name, dtype);
    BG_REQUIRE(N > 0 && H > 0 && W > 0 && C > 0 && r >= 1 && r <= 8, "%s: N=%d H=%d W=%d C=%d r=%d", name, N, H, W, C, r);
    const int per16 = dtype == BG_BF16 ? 8 : 4;
    BG_REQUIRE(C % per16 == 0, "%s: C = %d must be a multiple of %d (16-byte runs)", name, C, per16);
    BG_REQUIRE(((uintptr_t)x & 15) == 0 && ((uintptr_t)y & 15) == 0, "%s: tensors must be 16-byte aligned", name);
    BG_REQUIRE((int64_t)N * H < (int64_t(1) << 31) && (int64_t)W * r * r * C < (int64_t(1) << 31), "%s: tensor too large",
               name);
    ShufParams p;
    p.src = reinterpret_cast<const uint4*>(x);
    p.dst = reinterpret_cast<uint4*>(y);
    p.L = r * (C / per16);
    p.RA = to_space ? r : W;
    p.RB = to_space ? W : r;
    p.total = (int64_t)N * H * W * r * p.L;
    int64_t blocks = (p.total + SHUF_BLOCK * SHUF_UNROLL - 1) / (SHUF_BLOCK * SHUF_UNROLL);
    if (blocks > SHUF_MAX_BLOCKS) blocks = SHUF_MAX_BLOCKS;
    const int64_t S = blocks * SHUF_BLOCK;
    p.sl = (int)(S % p.L);
    int64_t t = S / p.L;
    p.sb = (int)(t % p.RB);
    t /= p.RB;
    p.sa = (int)(t % p.RA);
    p.sq = t / p.RA;
    hipLaunchKernelGGL(subpixel_shuffle_kernel, dim3((int)blocks), dim3(SHUF_BLOCK), 0, as_stream(stream), p);
    BG_LAUNCH_CHECK();
    return BG_OK;
}

}  // namespace bg

using namespace bg;

extern "C" {

int bg_depth_to_space(const void* x, void* y, int dtype, int N, int H, int W, int C, int r, void* stream) {
    return launch_shuffle("bg_depth_to_space", x, y, dtype, N, H, W, C, r, true, stream);
}

int bg_space_to_depth(const void* x, void* y, int dtype, int N, int H, int W, int C, int r, void* stream) {
    return launch_shuffle("bg_space_to_depth", x, y, dtype, N, H, W, C, r, false, stream);
}

}  // extern "C"
