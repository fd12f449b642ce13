// input_resize.h - the per-pixel arithmetic of the TF1 legacy-bilinear resize and the normalisation x / 127.5 - 1, shared
// by input.hip (bg_image_batch_u8) and dataset.hip (bg_dataset_batch, kind 0) so that one copy exists.  Every step is one
// correctly rounded fp32 operation, bit-identical to data.resize_bilinear_legacy and (img / 127.5 - 1) in numpy fp32:
//   src = i * scale (scale = (float)((double)n_in / S), from the table), lo = floor(src), hi = min(lo + 1, n_in - 1),
//   f = src - lo;  top = a * (1 - fx) + b * fx, bot likewise;  v = top * (1 - fy) + bot * fy;  out = v / 127.5f - 1.
// hipcc contracts a * b + c into an fma by default, and __fmul_rn / __fadd_rn are plain operators in its headers, so
// contraction is switched off here and in both translation units.
#pragma once

#pragma clang fp contract(off)

namespace bg {

struct InAxis {
    int lo, hi;
    float f, g;         // weight of hi, weight of lo = fl32(1 - f)
};

__device__ __forceinline__ InAxis in_axis(int i, float scale, int n_in) {
    const float src = (float)i * scale;
    const float fl = floorf(src);
    int lo = (int)fl;
    lo = lo < 0 ? 0 : (lo > n_in - 1 ? n_in - 1 : lo);      // (never fires where the host path succeeds: bounds only)
    InAxis a;
    a.lo = lo;
    a.hi = lo + 1 < n_in ? lo + 1 : n_in - 1;
    a.f = src - fl;
    a.g = 1.0f - a.f;
    return a;
}

__device__ __forceinline__ float in_pixel(float a, float b, float c, float d, const InAxis& ax, const InAxis& ay) {
    const float top = a * ax.g + b * ax.f;
    const float bot = c * ax.g + d * ax.f;
    const float v = top * ay.g + bot * ay.f;
    return v / 127.5f - 1.0f;
}

}  // namespace bg
