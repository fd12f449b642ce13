// dataset.hip - the device-resident dataset cache (data.DatasetCache): every file is decoded once, kept in one arena on
// the GPU in its cached form, and every later batch is one gather launch from an index list.
//
//   dataset_store   src: a staged buffer (packed uint8 pixels, or finished fp32 images); segs: one BgCopySeg per image
//                   ->  the bytes of each segment at its slot of the arena.  A guarded batched copy, nothing else.
//   dataset_batch   arena + one BgDatasetEntry per cached image + sel int32 [n,2] (entry index, flip)
//                   ->  out [n,S,S,C] fp32 in [-1,1]
//
// The two cached forms of an image:
//   kind 0  the decoded uint8 pixels [h,w,C]: resize, flip and normalise happen here, with the arithmetic of
//           bg_image_batch_u8 step for step (input_resize.h: one copy of it exists; no fma, contraction is off);
//   kind 1  the finished fp32 image [S,S,C], not flipped: out[y][x][:] = cached[y][flip ? S-1-x : x][:], pixels mirrored,
//           channels in order.  The normalisation is elementwise, so this is the host path's flip bit for bit.
//
// HBM-bound, one pass, laid out as input.hip: one thread = one output pixel, all C channels; 16-byte accesses for C = 4
// where aligned; a grid capped at 4096 blocks of 256 with a grid-stride loop; 64-bit indices.  Mixed kinds in one launch
// are the normal case: the branch is uniform per image, so a wave diverges only where it straddles two images.
//
// The library cannot read the device tables, so the kernels check every entry themselves.  dataset_batch fills the image
// of a sel row with NaN, reading nothing, when the index is outside [0, n_entries), the kind is neither 0 nor 1, h or
// w < 1, kind 1 with h or w != S, the offset is negative or no multiple of 16, or the extent ends past arena_bytes.
// dataset_store skips a segment whole when src, dst or bytes is negative or no multiple of 4, or an extent lies outside
// src_bytes / arena_bytes.  data.plan_entries validates first, so neither guard fires in normal use.
#include "common.h"

#pragma clang fp contract(off)

#include "input_resize.h"      // InAxis, in_axis, in_pixel: shared with input.hip

namespace bg {

#define DS_BLOCK 256
#define DS_MAX_BLOCKS 4096

static_assert(sizeof(BgDatasetEntry) == 32, "BgDatasetEntry is 32 bytes (data.plan_entries builds it as 8 int32)");
static_assert(sizeof(BgCopySeg) == 32, "BgCopySeg is 32 bytes (data.DatasetCache builds it as 4 int64)");

struct DsGeom {
    int64_t total;      // output pixels: n * S * S
    int64_t arena_bytes;
    int S;
    int n_entries;
};

// VEC (C = 4 only): arena and out 16-byte aligned (entry offsets are multiples of 16, checked per entry).
template <int C, bool VEC>
__global__ __launch_bounds__(DS_BLOCK) void dataset_batch_kernel(const uint8_t* __restrict__ arena,
                                                                 const BgDatasetEntry* __restrict__ entries,
                                                                 const int32_t* __restrict__ sel, float* __restrict__ out,
                                                                 DsGeom g) {
    const int64_t SS = (int64_t)g.S * g.S;
    for (int64_t i = (int64_t)blockIdx.x * DS_BLOCK + threadIdx.x; i < g.total; i += (int64_t)gridDim.x * DS_BLOCK) {
        const int64_t img = i / SS;
        const int r = (int)(i - img * SS);                    // < S * S <= 16384^2
        const int oy = r / g.S, ox = r - oy * g.S;
        const int idx = sel[2 * img], flip = sel[2 * img + 1];
        float* dst = out + i * C;
        bool fits = idx >= 0 && idx < g.n_entries;
        BgDatasetEntry e;
        e.offset = 0, e.h = 0, e.w = 0, e.kind = -1, e.scale_y = 0.0f, e.scale_x = 0.0f, e.reserved = 0;
        if (fits) e = entries[idx];
        const int64_t elem = e.kind == 1 ? (int64_t)C * 4 : (int64_t)C;          // bytes per pixel of the cached form
        fits = fits && (e.kind == 0 || e.kind == 1) && e.h >= 1 && e.w >= 1 && (e.kind == 0 || (e.h == g.S && e.w == g.S)) &&
               e.offset >= 0 && (e.offset & 15) == 0 && e.offset <= g.arena_bytes &&
               (int64_t)e.h * e.w <= (g.arena_bytes - e.offset) / elem;
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
        const uint8_t* base = arena + e.offset;
        if (e.kind == 1) {
            const int sx = flip ? g.S - 1 - ox : ox;
            const float* src = reinterpret_cast<const float*>(base) + ((int64_t)oy * g.S + sx) * C;
            if constexpr (VEC) {
                *reinterpret_cast<float4*>(dst) = *reinterpret_cast<const float4*>(src);
            } else {
#pragma unroll
                for (int c = 0; c < C; ++c) dst[c] = src[c];
            }
            continue;
        }
        const InAxis ay = in_axis(oy, e.scale_y, e.h);
        const InAxis ax = in_axis(flip ? g.S - 1 - ox : ox, e.scale_x, e.w);
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

// blockIdx.y walks the segments, blockIdx.x the words of one segment; both with a stride loop.  ALIGNED: src and arena
// are 16-byte aligned, so a segment whose src, dst and bytes are multiples of 16 moves as 16-byte words.
template <bool ALIGNED>
__global__ __launch_bounds__(DS_BLOCK) void dataset_store_kernel(const uint8_t* __restrict__ src, int64_t src_bytes,
                                                                 const BgCopySeg* __restrict__ segs, int n_segs,
                                                                 uint8_t* __restrict__ arena, int64_t arena_bytes) {
    for (int s = blockIdx.y; s < n_segs; s += gridDim.y) {
        const BgCopySeg g = segs[s];
        const bool fits = g.src >= 0 && g.dst >= 0 && g.bytes >= 0 && ((g.src | g.dst | g.bytes) & 3) == 0 &&
                          g.src <= src_bytes && g.bytes <= src_bytes - g.src &&
                          g.dst <= arena_bytes && g.bytes <= arena_bytes - g.dst;
        if (!fits) continue;
        const int64_t first = (int64_t)blockIdx.x * DS_BLOCK + threadIdx.x, step = (int64_t)gridDim.x * DS_BLOCK;
        if (ALIGNED && ((g.src | g.dst | g.bytes) & 15) == 0) {
            const uint4* from = reinterpret_cast<const uint4*>(src + g.src);
            uint4* to = reinterpret_cast<uint4*>(arena + g.dst);
            const int64_t n = g.bytes >> 4;
            for (int64_t i = first; i < n; i += step) to[i] = from[i];
        } else {
            const uint32_t* from = reinterpret_cast<const uint32_t*>(src + g.src);
            uint32_t* to = reinterpret_cast<uint32_t*>(arena + g.dst);
            const int64_t n = g.bytes >> 2;
            for (int64_t i = first; i < n; i += step) to[i] = from[i];
        }
    }
}

}  // namespace bg

using namespace bg;

extern "C" {

int bg_dataset_store(const void* src, int64_t src_bytes, const BgCopySeg* segs, int n_segs, uint8_t* arena,
                     int64_t arena_bytes, void* stream) {
    BG_REQUIRE(src && segs && arena, "bg_dataset_store: NULL tensor");
    BG_REQUIRE(n_segs > 0 && src_bytes > 0 && arena_bytes > 0, "bg_dataset_store: n_segs=%d src_bytes=%lld arena_bytes=%lld",
               n_segs, (long long)src_bytes, (long long)arena_bytes);
    BG_REQUIRE(((uintptr_t)src & 3) == 0 && ((uintptr_t)arena & 3) == 0 && ((uintptr_t)segs & 7) == 0,
               "bg_dataset_store: src and arena must be 4-byte, segs 8-byte aligned");
    // the library cannot see the segment sizes: a fixed number of blocks per segment, at most DS_MAX_BLOCKS in all
    const int gy = n_segs < DS_MAX_BLOCKS ? n_segs : DS_MAX_BLOCKS;
    int gx = DS_MAX_BLOCKS / gy;
    gx = gx > 64 ? 64 : gx;
    const dim3 blocks((unsigned)gx, (unsigned)gy), block(DS_BLOCK);
    hipStream_t s = as_stream(stream);
    const uint8_t* from = static_cast<const uint8_t*>(src);
    const bool aligned = (((uintptr_t)src | (uintptr_t)arena) & 15) == 0;
    if (aligned) hipLaunchKernelGGL((dataset_store_kernel<true>), blocks, block, 0, s, from, src_bytes, segs, n_segs, arena,
                                    arena_bytes);
    else hipLaunchKernelGGL((dataset_store_kernel<false>), blocks, block, 0, s, from, src_bytes, segs, n_segs, arena,
                            arena_bytes);
    BG_LAUNCH_CHECK();
    return BG_OK;
}

int bg_dataset_batch(const uint8_t* arena, int64_t arena_bytes, const BgDatasetEntry* entries, int n_entries,
                     const int32_t* sel, int n, int S, int C, float* out, void* stream) {
    BG_REQUIRE(arena && entries && sel && out, "bg_dataset_batch: NULL tensor");
    BG_REQUIRE(C == 1 || C == 3 || C == 4, "bg_dataset_batch: C=%d (1, 3 or 4 channels)", C);
    BG_REQUIRE(n > 0 && S > 0 && n_entries > 0 && arena_bytes > 0, "bg_dataset_batch: n=%d S=%d n_entries=%d arena_bytes=%lld",
               n, S, n_entries, (long long)arena_bytes);
    BG_REQUIRE(S <= 16384, "bg_dataset_batch: S=%d too large", S);
    BG_REQUIRE(((uintptr_t)arena & 15) == 0 && ((uintptr_t)entries & 7) == 0 && ((uintptr_t)sel & 3) == 0 &&
               ((uintptr_t)out & 3) == 0, "bg_dataset_batch: arena must be 16-byte, entries 8-byte, sel and out 4-byte aligned");
    DsGeom g;
    g.total = (int64_t)n * S * S;
    g.arena_bytes = arena_bytes;
    g.S = S;
    g.n_entries = n_entries;
    int64_t nb = (g.total + DS_BLOCK - 1) / DS_BLOCK;
    if (nb > DS_MAX_BLOCKS) nb = DS_MAX_BLOCKS;
    hipStream_t s = as_stream(stream);
    const dim3 blocks((unsigned)nb), block(DS_BLOCK);
    if (C == 4) {
        if (((uintptr_t)out & 15) == 0) hipLaunchKernelGGL((dataset_batch_kernel<4, true>), blocks, block, 0, s, arena, entries, sel, out, g);
        else hipLaunchKernelGGL((dataset_batch_kernel<4, false>), blocks, block, 0, s, arena, entries, sel, out, g);
    } else if (C == 3) {
        hipLaunchKernelGGL((dataset_batch_kernel<3, false>), blocks, block, 0, s, arena, entries, sel, out, g);
    } else {
        hipLaunchKernelGGL((dataset_batch_kernel<1, false>), blocks, block, 0, s, arena, entries, sel, out, g);
    }
    BG_LAUNCH_CHECK();
    return BG_OK;
}

}  // extern "C"
