// sample.hip - generator output -> the bytes of a sample grid (utils.py:133-161 save_images: inverse_transform, merge,
// imageio's 8-bit conversion), so that an in-training sample grid (BigGAN.py:1125-1230) leaves the device as one byte
// per element instead of four.
//
//   image_tiles_u8   x [n,H,W,C] fp32 or bf16, nominally in [-1,1]  ->  grid [gh*H, gw*W, C] uint8
//                    image i goes to tile t = tile0 + i at grid row t / gw, column t % gw (the row-major placement of
//                    utils.merge); images whose tile is >= gh*gw are skipped, tiles without an image are not touched.
//
// Arithmetic, bit-identical to the host path (numpy): t = (x + 1) * 0.5 in fp32 (inverse_transform on an fp32 array),
// then in DOUBLE v = t * 255 (merge copies into a float64 grid), rint (nearest even), clamp to [0,255].  The widening
// matters: an fp32 product rounds values next to a k + 0.5 tie to the other side.  NaN writes 0.
//
//   image_place_u8   the same bytes, but every image of the batch goes to a destination of its own: a device table gives
//                    each image the byte offset of its first row in an arena and the pitch between its rows (the
//                    sampling service packs the images of one generator batch into the response strips of several
//                    request files).  The host cannot read the table, so the kernel checks every entry against the
//                    arena and writes nothing at all for one that does not fit.
//
// HBM-bound, one pass.  With tw = W*C bytes per tile row and tw % 4 == 0, every tile row starts 4-element aligned in the
// image and in the grid: one thread takes 4 consecutive elements of one tile row (one 16-byte fp32 / 8-byte bf16 load,
// one 32-bit store of the packed bytes), adjacent lanes walk along the row.  Otherwise one element per thread.
#include "common.h"

namespace bg {

#define SM_BLOCK 256
#define SM_MAX_BLOCKS 16384

static inline int sm_blocks(int64_t work) {
    int64_t b = (work + SM_BLOCK - 1) / SM_BLOCK;
    if (b > SM_MAX_BLOCKS) b = SM_MAX_BLOCKS;
    if (b < 1) b = 1;
    return (int)b;
}

__device__ __forceinline__ float sm_widen(float v) { return v; }
__device__ __forceinline__ float sm_widen(uint16_t bits) { return __uint_as_float((uint32_t)bits << 16); }   // bf16 -> fp32, exact

__device__ __forceinline__ uint32_t sm_byte(float x) {
    const float t = (x + 1.0f) * 0.5f;
    const double r = rint((double)t * 255.0);
    // (NaN fails the first comparison: 0)
    return r >= 0.0 ? (r <= 255.0 ? (uint32_t)r : 255u) : 0u;
}

template <typename T>
struct SmVec4;
template <>
struct SmVec4<float> {
    static __device__ __forceinline__ void load(const float* p, float (&v)[4]) {
        const float4 t = *reinterpret_cast<const float4*>(p);
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    }
};
template <>
struct SmVec4<uint16_t> {
    static __device__ __forceinline__ void load(const uint16_t* p, float (&v)[4]) {
        const uint2 t = *reinterpret_cast<const uint2*>(p);
        v[0] = __uint_as_float(t.x << 16); v[1] = __uint_as_float(t.x & 0xffff0000u);
        v[2] = __uint_as_float(t.y << 16); v[3] = __uint_as_float(t.y & 0xffff0000u);
    }
};

// 4 consecutive elements -> their 4 bytes, lowest address in the low byte
template <typename T>
__device__ __forceinline__ uint32_t sm_word(const T* src) {
    float v[4];
    SmVec4<T>::load(src, v);
    return sm_byte(v[0]) | (sm_byte(v[1]) << 8) | (sm_byte(v[2]) << 16) | (sm_byte(v[3]) << 24);
}

struct SmGeom {
    int64_t total;      // work items: images placed * H * (tw / VEC)
    int H, tw, gw, tile0;
};

// VEC = 4: tw % 4 == 0, x 16-byte (fp32) / 8-byte (bf16) aligned, grid 4-byte aligned.
template <typename T, int VEC>
__global__ __launch_bounds__(SM_BLOCK) void image_tiles_u8_kernel(const T* __restrict__ x, uint8_t* __restrict__ grid,
                                                                  SmGeom g) {
    const int64_t per_row = g.tw / VEC;
    const int64_t row_bytes = (int64_t)g.gw * g.tw;           // one grid row
    for (int64_t i = (int64_t)blockIdx.x * SM_BLOCK + threadIdx.x; i < g.total; i += (int64_t)gridDim.x * SM_BLOCK) {
        const int64_t r = i / per_row;                        // tile row over all placed images: img * H + row
        const int64_t q = i - r * per_row;
        const int64_t img = r / g.H;
        const int64_t row = r - img * g.H;
        const int64_t t = g.tile0 + img;
        const int64_t gr = t / g.gw, gc = t - gr * g.gw;
        uint8_t* dst = grid + (gr * g.H + row) * row_bytes + gc * g.tw + q * VEC;
        const T* src = x + i * VEC;                           // the placed images are a contiguous prefix of x
        if constexpr (VEC == 4) {
            *reinterpret_cast<uint32_t*>(dst) = sm_word<T>(src);
        } else {
            dst[0] = (uint8_t)sm_byte(sm_widen(src[0]));
        }
    }
}

// One work item = VEC consecutive elements of one image row.  An entry is used only if the whole image fits:
// 0 <= offset, tw <= pitch, offset + (H-1)*pitch + tw <= arena_bytes (H <= 16384 and pitch < 2^31: no overflow once
// the extent itself is known to be <= arena_bytes).  VEC = 4 needs tw % 4 == 0, x 16-byte (fp32) / 8-byte (bf16) aligned
// and a 4-byte aligned arena; an entry whose offset or pitch is off the 4-byte grid then stores its 4 bytes one by one.
template <typename T, int VEC>
__global__ __launch_bounds__(SM_BLOCK) void image_place_u8_kernel(const T* __restrict__ x,
                                                                  const BgPlaceEntry* __restrict__ table,
                                                                  uint8_t* __restrict__ arena, int64_t arena_bytes,
                                                                  int64_t total, int H, int tw) {
    const int64_t per_row = tw / VEC;
    for (int64_t i = (int64_t)blockIdx.x * SM_BLOCK + threadIdx.x; i < total; i += (int64_t)gridDim.x * SM_BLOCK) {
        const int64_t r = i / per_row;                        // img * H + row
        const int64_t q = i - r * per_row;
        const int64_t img = r / H;
        const int64_t row = r - img * H;
        const BgPlaceEntry e = table[img];
        if (e.skip != 0 || e.offset < 0 || e.pitch < tw) continue;
        const int64_t extent = (int64_t)(H - 1) * e.pitch + tw;
        if (extent > arena_bytes || e.offset > arena_bytes - extent) continue;
        uint8_t* dst = arena + e.offset + row * (int64_t)e.pitch + q * VEC;
        const T* src = x + i * VEC;
        if constexpr (VEC == 4) {
            const uint32_t word = sm_word<T>(src);
            if (((e.offset | (int64_t)e.pitch) & 3) == 0) {
                *reinterpret_cast<uint32_t*>(dst) = word;
            } else {
                dst[0] = (uint8_t)word; dst[1] = (uint8_t)(word >> 8); dst[2] = (uint8_t)(word >> 16);
                dst[3] = (uint8_t)(word >> 24);
            }
        } else {
            dst[0] = (uint8_t)sm_byte(sm_widen(src[0]));
        }
    }
}

}  // namespace bg

using namespace bg;

extern "C" {

int bg_image_tiles_u8(const void* x, int x_dtype, int n, int H, int W, int C, uint8_t* grid, int gh, int gw, int tile0,
                      void* stream) {
    BG_REQUIRE(x && grid, "bg_image_tiles_u8: NULL tensor");
    BG_REQUIRE(x_dtype == BG_F32 || x_dtype == BG_BF16, "bg_image_tiles_u8: dtype %d (BG_F32 / BG_BF16)", x_dtype);
    BG_REQUIRE(C == 1 || C == 3 || C == 4, "bg_image_tiles_u8: C=%d (1, 3 or 4 channels)", C);
    BG_REQUIRE(n > 0 && H > 0 && W > 0 && gh > 0 && gw > 0, "bg_image_tiles_u8: n=%d H=%d W=%d gh=%d gw=%d", n, H, W, gh, gw);
    BG_REQUIRE(H <= 16384 && W <= 16384 && gh <= 4096 && gw <= 4096, "bg_image_tiles_u8: H=%d W=%d gh=%d gw=%d too large",
               H, W, gh, gw);
    BG_REQUIRE(tile0 >= 0, "bg_image_tiles_u8: tile0=%d", tile0);
    const int64_t tiles = (int64_t)gh * gw;
    if (tile0 >= tiles) return BG_OK;                         // every image falls past the grid
    const int64_t placed = (tiles - tile0 < n) ? tiles - tile0 : n;
    const int tw = W * C;
    const size_t esz = x_dtype == BG_BF16 ? 2 : 4;
    const bool wide = tw % 4 == 0 && ((uintptr_t)x & (4 * esz - 1)) == 0 && ((uintptr_t)grid & 3) == 0;
    SmGeom g;
    g.total = placed * H * (wide ? tw / 4 : tw);
    g.H = H; g.tw = tw; g.gw = gw; g.tile0 = tile0;
    hipStream_t s = as_stream(stream);
    const dim3 blocks(sm_blocks(g.total)), block(SM_BLOCK);
    if (x_dtype == BG_BF16) {
        if (wide) hipLaunchKernelGGL((image_tiles_u8_kernel<uint16_t, 4>), blocks, block, 0, s, (const uint16_t*)x, grid, g);
        else hipLaunchKernelGGL((image_tiles_u8_kernel<uint16_t, 1>), blocks, block, 0, s, (const uint16_t*)x, grid, g);
    } else {
        if (wide) hipLaunchKernelGGL((image_tiles_u8_kernel<float, 4>), blocks, block, 0, s, (const float*)x, grid, g);
        else hipLaunchKernelGGL((image_tiles_u8_kernel<float, 1>), blocks, block, 0, s, (const float*)x, grid, g);
    }
    BG_LAUNCH_CHECK();
    return BG_OK;
}

int bg_image_place_u8(const void* x, int x_dtype, int n, int H, int W, int C, const BgPlaceEntry* table, uint8_t* arena,
                      int64_t arena_bytes, void* stream) {
    BG_REQUIRE(x && table && arena, "bg_image_place_u8: NULL tensor");
    BG_REQUIRE(x_dtype == BG_F32 || x_dtype == BG_BF16, "bg_image_place_u8: dtype %d (BG_F32 / BG_BF16)", x_dtype);
    BG_REQUIRE(C == 1 || C == 3 || C == 4, "bg_image_place_u8: C=%d (1, 3 or 4 channels)", C);
    BG_REQUIRE(n > 0 && H > 0 && W > 0, "bg_image_place_u8: n=%d H=%d W=%d", n, H, W);
    BG_REQUIRE(H <= 16384 && W <= 16384, "bg_image_place_u8: H=%d W=%d too large", H, W);
    BG_REQUIRE(arena_bytes > 0, "bg_image_place_u8: arena_bytes=%lld", (long long)arena_bytes);
    BG_REQUIRE(((uintptr_t)table & 7) == 0, "bg_image_place_u8: table must be 8-byte aligned");
    const int tw = W * C;
    const size_t esz = x_dtype == BG_BF16 ? 2 : 4;
    BG_REQUIRE(((uintptr_t)x & (esz - 1)) == 0, "bg_image_place_u8: x is not aligned to its element size");
    const bool wide = tw % 4 == 0 && ((uintptr_t)x & (4 * esz - 1)) == 0 && ((uintptr_t)arena & 3) == 0;
    const int64_t total = (int64_t)n * H * (wide ? tw / 4 : tw);
    hipStream_t s = as_stream(stream);
    const dim3 blocks(sm_blocks(total)), block(SM_BLOCK);
    if (x_dtype == BG_BF16) {
        if (wide) hipLaunchKernelGGL((image_place_u8_kernel<uint16_t, 4>), blocks, block, 0, s, (const uint16_t*)x, table,
                                     arena, arena_bytes, total, H, tw);
        else hipLaunchKernelGGL((image_place_u8_kernel<uint16_t, 1>), blocks, block, 0, s, (const uint16_t*)x, table, arena,
                                arena_bytes, total, H, tw);
    } else {
        if (wide) hipLaunchKernelGGL((image_place_u8_kernel<float, 4>), blocks, block, 0, s, (const float*)x, table, arena,
                                     arena_bytes, total, H, tw);
        else hipLaunchKernelGGL((image_place_u8_kernel<float, 1>), blocks, block, 0, s, (const float*)x, table, arena,
                                arena_bytes, total, H, tw);
    }
    BG_LAUNCH_CHECK();
    return BG_OK;
}

}  // extern "C"
