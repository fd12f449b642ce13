// input.hip - decoded uint8 images -> the training batch (utils.py:12-38 image_processing: tf.image.resize_images of
// TF 1.x, random_flip_left_right, x / 127.5 - 1), so that the host only decodes and the batch crosses the bus as one byte
// per element instead of four.
//
//   image_batch_u8   raw: the pixels of n images, each [h,w,C] row-major at a 16-byte aligned offset of one buffer;
//                    table: one BgImageEntry per image (offset, h, w, flip, the two fp32 scales)
//                    ->  out [n,S,S,C] fp32 in [-1,1]
//
// Arithmetic, bit-identical to the host path (data.resize_bilinear_legacy, [:, ::-1], (img / 127.5 - 1) in numpy fp32);
// every step below is one correctly rounded fp32 operation, nothing is fused:
//   src = i * scale (scale = (float)((double)n_in / S), from the table), lo = floor(src), hi = min(lo + 1, n_in - 1),
//   f = src - lo;  top = a * (1 - fx) + b * fx, bot likewise;  v = top * (1 - fy) + bot * fy;  out = v / 127.5f - 1.
// The flip mirrors the OUTPUT columns (legacy bilinear is not flip-symmetric).  hipcc contracts a * b + c into an fma by
// default, and __fmul_rn / __fadd_rn are plain operators in its headers, so contraction is switched off for this file.
//
// HBM-bound, one pass.  One thread = one output pixel, all C channels: four source taps (one 32-bit load each for C = 4,
// byte loads otherwise), one 16-byte store for C = 4; adjacent lanes walk along the output row.  The library cannot see
// the table, so the kernel checks each entry against raw_bytes itself: an entry that does not fit (or has h or w < 1, or
// a misaligned offset) fills its image with NaN and reads nothing.
#include "common.h"

#pragma clang fp contract(off)

#include "input_resize.h"      // InAxis, in_axis, in_pixel: shared with dataset.hip

namespace bg {

#define IN_BLOCK 256
#define IN_MAX_BLOCKS 4096

static_assert(sizeof(BgImageEntry) == 32, "BgImageEntry is 32 bytes (data.pack_batch builds it as 8 int32)");

struct InGeom {
    int64_t total;      // output pixels: n * S * S
    int64_t raw_bytes;
    int S;
};

// VEC (C = 4 only): raw 4-byte aligned and out 16-byte aligned.
template <int C, bool VEC>
__global__ __launch_bounds__(IN_BLOCK) void image_batch_u8_kernel(const uint8_t* __restrict__ raw,
                                                                  const BgImageEntry* __restrict__ table,
                                                                  float* __restrict__ out, InGeom g) {
    const int64_t SS = (int64_t)g.S * g.S;
    for (int64_t i = (int64_t)blockIdx.x * IN_BLOCK + threadIdx.x; i < g.total; i += (int64_t)gridDim.x * IN_BLOCK) {
        const int64_t img = i / SS;
        const int r = (int)(i - img * SS);                    // < S * S <= 16384^2
        const int oy = r / g.S, ox = r - oy * g.S;
        const BgImageEntry e = table[img];
        float* dst = out + i * C;
        const bool fits = e.h >= 1 && e.w >= 1 && e.offset >= 0 && (e.offset & 15) == 0 && e.offset <= g.raw_bytes &&
                          (int64_t)e.h * e.w <= (g.raw_bytes - e.offset) / C;
        if (!fits) {
            const float nan = __uint_as_float(0x7fc00000u);
            if constexpr (VEC) {
                *reinterpret_cast<float4*>(dst) = make_float4(nan, nan, nan, nan);
            } else {
#pragma unroll
                for (int c = 0; c < C; ++c) dst[c] = nan;
            }
            continue;
        }
        const InAxis ay = in_axis(oy, e.scale_y, e.h);
        const InAxis ax = in_axis(e.flip ? g.S - 1 - ox : ox, e.scale_x, e.w);
        const uint8_t* base = raw + e.offset;
        const uint8_t* pa = base + ((int64_t)ay.lo * e.w + ax.lo) * C;
        const uint8_t* pb = base + ((int64_t)ay.lo * e.w + ax.hi) * C;
        const uint8_t* pc = base + ((int64_t)ay.hi * e.w + ax.lo) * C;
        const uint8_t* pd = base + ((int64_t)ay.hi * e.w + ax.hi) * C;
        if constexpr (VEC) {
            const uint32_t a = *reinterpret_cast<const uint32_t*>(pa), b = *reinterpret_cast<const uint32_t*>(pb);
            const uint32_t c = *reinterpret_cast<const uint32_t*>(pc), d = *reinterpret_cast<const uint32_t*>(pd);
            float v[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int sh = 8 * k;
                v[k] = in_pixel((float)((a >> sh) & 255u), (float)((b >> sh) & 255u), (float)((c >> sh) & 255u),
                                (float)((d >> sh) & 255u), ax, ay);
            }
            *reinterpret_cast<float4*>(dst) = make_float4(v[0], v[1], v[2], v[3]);
        } else {
#pragma unroll
            for (int k = 0; k < C; ++k) dst[k] = in_pixel((float)pa[k], (float)pb[k], (float)pc[k], (float)pd[k], ax, ay);
        }
    }
}

}  // namespace bg

using namespace bg;

extern "C" {

int bg_image_batch_u8(const uint8_t* raw, int64_t raw_bytes, const BgImageEntry* table, int n, int S, int C, float* out,
                      void* stream) {
    BG_REQUIRE(raw && table && out, "bg_image_batch_u8: NULL tensor");
    BG_REQUIRE(C == 1 || C == 3 || C == 4, "bg_image_batch_u8: C=%d (1, 3 or 4 channels)", C);
    BG_REQUIRE(n > 0 && S > 0 && raw_bytes > 0, "bg_image_batch_u8: n=%d S=%d raw_bytes=%lld", n, S, (long long)raw_bytes);
    BG_REQUIRE(S <= 16384, "bg_image_batch_u8: S=%d too large", S);
    BG_REQUIRE(((uintptr_t)table & 7) == 0 && ((uintptr_t)out & 3) == 0, "bg_image_batch_u8: table must be 8-byte, out "
               "4-byte aligned");
    InGeom g;
    g.total = (int64_t)n * S * S;
    g.raw_bytes = raw_bytes;
    g.S = S;
    int64_t nb = (g.total + IN_BLOCK - 1) / IN_BLOCK;
    if (nb > IN_MAX_BLOCKS) nb = IN_MAX_BLOCKS;
    hipStream_t s = as_stream(stream);
    const dim3 blocks((unsigned)nb), block(IN_BLOCK);
    if (C == 4) {
        const bool vec = ((uintptr_t)raw & 3) == 0 && ((uintptr_t)out & 15) == 0;
        if (vec) hipLaunchKernelGGL((image_batch_u8_kernel<4, true>), blocks, block, 0, s, raw, table, out, g);
        else hipLaunchKernelGGL((image_batch_u8_kernel<4, false>), blocks, block, 0, s, raw, table, out, g);
    } else if (C == 3) {
        hipLaunchKernelGGL((image_batch_u8_kernel<3, false>), blocks, block, 0, s, raw, table, out, g);
    } else {
        hipLaunchKernelGGL((image_batch_u8_kernel<1, false>), blocks, block, 0, s, raw, table, out, g);
    }
    BG_LAUNCH_CHECK();
    return BG_OK;
}

}  // extern "C"
