// jpeg.hip - the dense part of a JPEG decode for every JPEG image of a packed batch (data.pack_batch): entropy-decoded
// coefficients -> the uint8 pixels of the images' slots in `raw`, after which bg_image_batch_u8 (input.hip) resizes,
// flips and normalises as for any other decoded image.  The serial part (marker walk, Huffman decode) is host code:
// csrc/jpeg_entropy.hip.
//
//   jpeg_batch_u8   coef: int16 coefficients, de-zigzagged, not dequantised, 64 per block;
//                   jpegs: one BgJpegEntry per JPEG image (slot, size, channels, sampling, per component the coefficient
//                          offset and the block grid, the quantisation tables, the image's first block index)
//                   ->  raw[slot : slot + h*w*channels] = the pixels [h, w, channels]
//
// Integer arithmetic, bit-identical to data.decode_jpeg (libjpeg's slow-integer IDCT, "fancy" upsampling, 16-bit
// fixed-point colour); products and sums wrap in 32 bits as numpy's int32 does, shifts are arithmetic.
//
// Three launches:
//   0. jpeg_validate_kernel    one workgroup.  The library cannot trust the table, so every extent is checked here,
//                              once: status[j] in the workspace, and an entry that fails has the height of its image's
//                              BgImageEntry set to 0, which bg_image_batch_u8 turns into a NaN image.  One thread walks
//                              each chunk of 256 verdicts in LDS in order, refuses block ranges that do not ascend, and
//                              gives start[j], a monotone copy of the block0 prefix for the search of the next kernel.  The other two
//                              kernels touch nothing of an entry without status 1.
//   1. jpeg_idct_kernel        one 8x8 block per 8 lanes, 32 blocks per workgroup.  The batch's blocks are numbered
//                              through the start[] prefix (binary search), so one grid covers images of any sizes.
//                              Lane r loads row r of the coefficients and of the quantisation table (16 bytes each),
//                              multiplies, and the block is transposed through LDS (padded to 9 words a row) so that the
//                              lane owns column r for pass 1; a second transpose gives it row r for pass 2; it stores its 8
//                              bytes.  Component planes are kept as 8x8 tiles of 64 bytes, block g at 64 * g, so a wave
//                              stores 512 contiguous bytes.
//   2. jpeg_colour_kernel      one thread per output pixel, grid.y = entry: crop to the component's size, triangle
//                              upsampling with the edge rules at the cropped size, YCbCr -> RGB, channels; [h, w, C].
// Bandwidth- and integer-bound at a few bytes per pixel; no atomics, no communication between workgroups.
#include "common.h"

namespace bg {

#define JP_BLOCK 256
#define JP_BLOCKS_PER_WG (JP_BLOCK / 8)
#define JP_MAX_GRID_X 1024

static_assert(sizeof(BgJpegEntry) == 480, "BgJpegEntry is 480 bytes (data.pack_batch builds it as 120 int32)");
static_assert(offsetof(BgJpegEntry, q) == 96, "the quantisation tables are loaded 16 bytes at a time");

struct JpGeom {
    int64_t coef_count;     // int16 elements
    int64_t total_blocks;
    int64_t raw_bytes;
    int n_jpeg, n;
};

__device__ __forceinline__ int64_t jp_entry_blocks(const BgJpegEntry& e) {      // of a valid entry
    int64_t nb = 0;
    for (int c = 0; c < e.ncomp; ++c) nb += (int64_t)e.comp[c].bw * e.comp[c].bh;
    return nb;
}

__device__ __forceinline__ bool jp_entry_ok(const BgJpegEntry& e, const JpGeom& g) {
    if (e.image < 0 || e.image >= g.n) return false;
    if (e.ncomp != 1 && e.ncomp != 3) return false;
    if (e.channels != 1 && e.channels != 3) return false;
    const bool s11 = e.hs == 1 && e.vs == 1, s21 = e.hs == 2 && e.vs == 1, s22 = e.hs == 2 && e.vs == 2;
    if (!(s11 || s21 || s22) || (e.ncomp == 1 && !s11)) return false;
    if (e.w < 1 || e.h < 1 || e.w > 65535 || e.h > 65535) return false;
    const int mx = (e.w + 8 * e.hs - 1) / (8 * e.hs), my = (e.h + 8 * e.vs - 1) / (8 * e.vs);
    int64_t nb = 0;
    for (int c = 0; c < e.ncomp; ++c) {
        const int bw = c == 0 ? mx * e.hs : mx, bh = c == 0 ? my * e.vs : my;       // <= 8192 each
        if (e.comp[c].bw != bw || e.comp[c].bh != bh) return false;
        const int64_t cnt = (int64_t)64 * bw * bh;
        if (e.comp[c].coef < 0 || (e.comp[c].coef & 7) || e.comp[c].coef > g.coef_count ||
            cnt > g.coef_count - e.comp[c].coef)
            return false;
        nb += (int64_t)bw * bh;
    }
    if (e.block0 < 0 || e.block0 > g.total_blocks || nb > g.total_blocks - e.block0) return false;
    if (e.slot < 0 || (e.slot & 15) || e.slot > g.raw_bytes) return false;
    return (int64_t)e.w * e.h <= (g.raw_bytes - e.slot) / e.channels;
}

__global__ __launch_bounds__(JP_BLOCK) void jpeg_validate_kernel(const BgJpegEntry* __restrict__ jpegs,
                                                                 BgImageEntry* table, int32_t* __restrict__ status,
                                                                 int32_t* __restrict__ start, JpGeom g) {
    __shared__ int32_t s_ok[JP_BLOCK], s_block0[JP_BLOCK], s_blocks[JP_BLOCK];
    __shared__ int64_t s_end;                       // one past the last block of the valid entries so far
    if (threadIdx.x == 0) s_end = 0;
    for (int base = 0; base < g.n_jpeg; base += JP_BLOCK) {        // uniform: every thread takes every turn
        const int j = base + threadIdx.x;
        int image = -1;
        s_ok[threadIdx.x] = 0;
        if (j < g.n_jpeg) {
            const BgJpegEntry& e = jpegs[j];
            bool ok = jp_entry_ok(e, g);
            if (e.image >= 0 && e.image < g.n) image = e.image;
            if (ok) {                               // the image entry that bg_image_batch_u8 will read describes this slot
                const BgImageEntry t = table[e.image];
                ok = t.offset == e.slot && t.h == e.h && t.w == e.w;
            }
            s_ok[threadIdx.x] = ok ? 1 : 0;
            s_block0[threadIdx.x] = e.block0;
            s_blocks[threadIdx.x] = ok ? (int32_t)jp_entry_blocks(e) : 0;      // <= total_blocks < 2^31
        }
        __syncthreads();
        if (threadIdx.x == 0) {                     // in order: block ranges must ascend, start[] ascends whatever they do
            int64_t end = s_end;
            const int m = g.n_jpeg - base < JP_BLOCK ? g.n_jpeg - base : JP_BLOCK;
            for (int k = 0; k < m; ++k) {
                const bool ok = s_ok[k] == 1 && s_block0[k] >= end;
                s_ok[k] = ok ? 1 : 0;
                if (ok) end = (int64_t)s_block0[k] + s_blocks[k];
                else s_block0[k] = (int32_t)end;    // a refused entry owns no block
            }
            s_end = end;
        }
        __syncthreads();
        if (j < g.n_jpeg) {
            status[j] = s_ok[threadIdx.x];
            start[j] = s_block0[threadIdx.x];
            if (!s_ok[threadIdx.x] && image >= 0) table[image].h = 0;      // bg_image_batch_u8: h < 1 -> NaN
        }
        __syncthreads();
    }
}

// libjpeg's jidctint.c butterfly (CONST_BITS = 13) on eight values, in place; wrapping 32-bit arithmetic.
#define JP_FIX_0_298631336 2446u
#define JP_FIX_0_390180644 3196u
#define JP_FIX_0_541196100 4433u
#define JP_FIX_0_765366865 6270u
#define JP_FIX_0_899976223 7373u
#define JP_FIX_1_175875602 9633u
#define JP_FIX_1_501321110 12299u
#define JP_FIX_1_847759065 15137u
#define JP_FIX_1_961570560 16069u
#define JP_FIX_2_053119869 16819u
#define JP_FIX_2_562915447 20995u
#define JP_FIX_3_072711026 25172u

template <int SHIFT>
__device__ __forceinline__ void jp_idct8(int32_t (&v)[8]) {
    uint32_t in[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) in[k] = (uint32_t)v[k];
    uint32_t z1 = (in[2] + in[6]) * JP_FIX_0_541196100;
    const uint32_t t2 = z1 - in[6] * JP_FIX_1_847759065;
    const uint32_t t3 = z1 + in[2] * JP_FIX_0_765366865;
    const uint32_t t0 = (in[0] + in[4]) << 13;
    const uint32_t t1 = (in[0] - in[4]) << 13;
    const uint32_t t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    uint32_t a = in[7], b = in[5], c = in[3], d = in[1];
    z1 = a + d;
    uint32_t z2 = b + c, z3 = a + c, z4 = b + d;
    const uint32_t z5 = (z3 + z4) * JP_FIX_1_175875602;
    a *= JP_FIX_0_298631336;
    b *= JP_FIX_2_053119869;
    c *= JP_FIX_3_072711026;
    d *= JP_FIX_1_501321110;
    z1 *= 0u - JP_FIX_0_899976223;
    z2 *= 0u - JP_FIX_2_562915447;
    z3 = z3 * (0u - JP_FIX_1_961570560) + z5;
    z4 = z4 * (0u - JP_FIX_0_390180644) + z5;
    a += z1 + z3;
    b += z2 + z4;
    c += z2 + z3;
    d += z1 + z4;
    const uint32_t r = 1u << (SHIFT - 1);
    v[0] = (int32_t)(t10 + d + r) >> SHIFT;
    v[1] = (int32_t)(t11 + c + r) >> SHIFT;
    v[2] = (int32_t)(t12 + b + r) >> SHIFT;
    v[3] = (int32_t)(t13 + a + r) >> SHIFT;
    v[4] = (int32_t)(t13 - a + r) >> SHIFT;
    v[5] = (int32_t)(t12 - b + r) >> SHIFT;
    v[6] = (int32_t)(t11 - c + r) >> SHIFT;
    v[7] = (int32_t)(t10 - d + r) >> SHIFT;
}

__global__ __launch_bounds__(JP_BLOCK) void jpeg_idct_kernel(const int16_t* __restrict__ coef,
                                                             const BgJpegEntry* __restrict__ jpegs,
                                                             const int32_t* __restrict__ status,
                                                             const int32_t* __restrict__ start,
                                                             uint8_t* __restrict__ planes, JpGeom g) {
    __shared__ int32_t tile[JP_BLOCKS_PER_WG][8][9];
    const int slot = threadIdx.x >> 3, r = threadIdx.x & 7;
    const int64_t blk = (int64_t)blockIdx.x * JP_BLOCKS_PER_WG + slot;      // the block's number in the batch
    // the last entry with start <= blk (start ascends; a refused entry shares its start with its successor)
    int lo = 0, hi = g.n_jpeg - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if ((int64_t)start[mid] <= blk) lo = mid;
        else hi = mid - 1;
    }
    bool live = blk < g.total_blocks && status[lo] == 1;
    int32_t v[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = 0;
    if (live) {
        const BgJpegEntry& e = jpegs[lo];
        int64_t b = blk - e.block0;                 // the block's number in the image; the entry is valid, so its
        int c = 0;                                  // components' blocks add up to at most total_blocks - block0
        live = b >= 0;
        while (live) {
            const int64_t nb = (int64_t)e.comp[c].bw * e.comp[c].bh;
            if (b < nb) break;
            b -= nb;
            if (++c == e.ncomp) live = false;       // past the image's last block: a hole of the prefix table
        }
        if (live) {
            const int4 cw = *reinterpret_cast<const int4*>(coef + e.comp[c].coef + 64 * b + 8 * r);
            const int4 qw = *reinterpret_cast<const int4*>(&e.q[c][8 * r]);
            const uint32_t cs[4] = {(uint32_t)cw.x, (uint32_t)cw.y, (uint32_t)cw.z, (uint32_t)cw.w};
            const uint32_t qs[4] = {(uint32_t)qw.x, (uint32_t)qw.y, (uint32_t)qw.z, (uint32_t)qw.w};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                v[2 * k] = (int32_t)(int16_t)(cs[k] & 0xffffu) * (int32_t)(qs[k] & 0xffffu);
                v[2 * k + 1] = (int32_t)(int16_t)(cs[k] >> 16) * (int32_t)(qs[k] >> 16);
            }
        }
    }
    // row r of the dequantised block -> column r
#pragma unroll
    for (int k = 0; k < 8; ++k) tile[slot][r][k] = v[k];
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = tile[slot][k][r];
    __syncthreads();
    jp_idct8<11>(v);                                // pass 1: v[k] = workspace[k][r]
#pragma unroll
    for (int k = 0; k < 8; ++k) tile[slot][k][r] = v[k];
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = tile[slot][r][k];
    jp_idct8<18>(v);                                // pass 2: v[k] = pixel[r][k] - 128
    if (live) {
        uint32_t w[2] = {0u, 0u};
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            int32_t p = v[k] + 128;
            p = p < 0 ? 0 : (p > 255 ? 255 : p);
            w[k >> 2] |= (uint32_t)p << (8 * (k & 3));
        }
        *reinterpret_cast<uint2*>(planes + 64 * blk + 8 * r) = make_uint2(w[0], w[1]);
    }
}

// sample (x, y) of a component plane kept as 8x8 tiles, bw tiles a row
__device__ __forceinline__ int32_t jp_sample(const uint8_t* __restrict__ plane, int bw, int x, int y) {
    return plane[((int64_t)(y >> 3) * bw + (x >> 3)) * 64 + (y & 7) * 8 + (x & 7)];
}

// chroma sample (x, y) of the full-size image: libjpeg's h2v1 / h2v2 "fancy" upsampling of the plane cropped to cw x ch.
// The neighbour of an edge sample is the sample itself, which is what libjpeg's edge rules amount to.
__device__ __forceinline__ int32_t jp_chroma(const uint8_t* __restrict__ plane, int bw, int cw, int ch, int hs, int vs,
                                             int x, int y) {
    if (hs == 1) return jp_sample(plane, bw, x, y);
    const int i = x >> 1;
    const int in = (x & 1) ? (i + 1 < cw ? i + 1 : cw - 1) : (i > 0 ? i - 1 : 0);
    if (vs == 1) return (3 * jp_sample(plane, bw, i, y) + jp_sample(plane, bw, in, y) + 1 + (x & 1)) >> 2;
    const int j = y >> 1;
    const int jn = (y & 1) ? (j + 1 < ch ? j + 1 : ch - 1) : (j > 0 ? j - 1 : 0);
    const int32_t r0 = 3 * jp_sample(plane, bw, i, j) + jp_sample(plane, bw, i, jn);
    const int32_t r1 = 3 * jp_sample(plane, bw, in, j) + jp_sample(plane, bw, in, jn);
    return (3 * r0 + r1 + 8 - (x & 1)) >> 4;
}

__global__ __launch_bounds__(JP_BLOCK) void jpeg_colour_kernel(const BgJpegEntry* __restrict__ jpegs,
                                                               const int32_t* __restrict__ status,
                                                               const uint8_t* __restrict__ planes,
                                                               uint8_t* __restrict__ raw) {
    const int j = blockIdx.y;
    if (status[j] != 1) return;
    const BgJpegEntry& e = jpegs[j];
    const int w = e.w, h = e.h, C = e.channels, hs = e.hs, vs = e.vs;
    const bool colour = C == 3 && e.ncomp == 3;
    const int bw0 = e.comp[0].bw, bw1 = e.comp[1].bw;
    const uint8_t* py = planes + 64 * (int64_t)e.block0;
    const uint8_t* pcb = py + 64 * (int64_t)bw0 * e.comp[0].bh;
    const uint8_t* pcr = pcb + 64 * (int64_t)bw1 * e.comp[1].bh;
    const int cw = (w + hs - 1) / hs, ch = (h + vs - 1) / vs;
    uint8_t* dst = raw + e.slot;
    const int64_t total = (int64_t)w * h;
    for (int64_t i = (int64_t)blockIdx.x * JP_BLOCK + threadIdx.x; i < total; i += (int64_t)gridDim.x * JP_BLOCK) {
        const int y = (int)(i / w), x = (int)(i - (int64_t)y * w);
        const int32_t Y = jp_sample(py, bw0, x, y);
        if (!colour) {
            if (C == 1) {
                dst[i] = (uint8_t)Y;
            } else {
                dst[3 * i] = (uint8_t)Y;
                dst[3 * i + 1] = (uint8_t)Y;
                dst[3 * i + 2] = (uint8_t)Y;
            }
            continue;
        }
        const int32_t cb = jp_chroma(pcb, bw1, cw, ch, hs, vs, x, y) - 128;
        const int32_t cr = jp_chroma(pcr, bw1, cw, ch, hs, vs, x, y) - 128;
        int32_t R = Y + ((91881 * cr + 32768) >> 16);                       // F(1.402)
        int32_t B = Y + ((116130 * cb + 32768) >> 16);                      // F(1.772)
        int32_t G = Y + ((-22554 * cb + 32768 - 46802 * cr) >> 16);         // F(0.34414), F(0.71414)
        R = R < 0 ? 0 : (R > 255 ? 255 : R);
        G = G < 0 ? 0 : (G > 255 ? 255 : G);
        B = B < 0 ? 0 : (B > 255 ? 255 : B);
        dst[3 * i] = (uint8_t)R;
        dst[3 * i + 1] = (uint8_t)G;
        dst[3 * i + 2] = (uint8_t)B;
    }
}

// status[n_jpeg] and start[n_jpeg], int32 each, ahead of the planes
static inline size_t jp_status_bytes(int n_jpeg) { return ((size_t)n_jpeg * 8 + 15) & ~(size_t)15; }

}  // namespace bg

using namespace bg;

extern "C" {

size_t bg_jpeg_batch_workspace_bytes(int n_jpeg, int64_t total_blocks) {
    if (n_jpeg < 1 || total_blocks < 1) return 0;
    return jp_status_bytes(n_jpeg) + 64 * (size_t)total_blocks;
}

int bg_jpeg_batch_u8(const int16_t* coef, int64_t coef_count, const BgJpegEntry* jpegs, int n_jpeg, int64_t total_blocks,
                     int max_pixels, uint8_t* raw, int64_t raw_bytes, BgImageEntry* table, int n, void* ws,
                     size_t ws_bytes, void* stream) {
    BG_REQUIRE(coef && jpegs && raw && table && ws, "bg_jpeg_batch_u8: NULL tensor");
    BG_REQUIRE(n_jpeg > 0 && n_jpeg <= 65535 && n >= n_jpeg, "bg_jpeg_batch_u8: n_jpeg=%d of n=%d images (1 .. 65535)",
               n_jpeg, n);
    BG_REQUIRE(coef_count > 0 && total_blocks > 0 && total_blocks <= (int64_t)0x7fffffff - JP_BLOCKS_PER_WG &&
               raw_bytes > 0 && max_pixels > 0,
               "bg_jpeg_batch_u8: coef_count=%lld total_blocks=%lld raw_bytes=%lld max_pixels=%d", (long long)coef_count,
               (long long)total_blocks, (long long)raw_bytes, max_pixels);
    BG_REQUIRE(((uintptr_t)coef & 15) == 0 && ((uintptr_t)jpegs & 15) == 0 && ((uintptr_t)table & 7) == 0 &&
               ((uintptr_t)ws & 15) == 0, "bg_jpeg_batch_u8: coef, jpegs and ws must be 16-byte, table 8-byte aligned");
    BG_REQUIRE(ws_bytes >= bg_jpeg_batch_workspace_bytes(n_jpeg, total_blocks),
               "bg_jpeg_batch_u8: workspace of %zu bytes, %zu needed", ws_bytes,
               bg_jpeg_batch_workspace_bytes(n_jpeg, total_blocks));
    JpGeom g;
    g.coef_count = coef_count;
    g.total_blocks = total_blocks;
    g.raw_bytes = raw_bytes;
    g.n_jpeg = n_jpeg;
    g.n = n;
    int32_t* status = static_cast<int32_t*>(ws);
    uint8_t* planes = static_cast<uint8_t*>(ws) + jp_status_bytes(n_jpeg);
    hipStream_t s = as_stream(stream);
    int32_t* start = status + n_jpeg;
    hipLaunchKernelGGL(jpeg_validate_kernel, dim3(1), dim3(JP_BLOCK), 0, s, jpegs, table, status, start, g);
    BG_LAUNCH_CHECK();
    const unsigned idct_blocks = (unsigned)((total_blocks + JP_BLOCKS_PER_WG - 1) / JP_BLOCKS_PER_WG);
    hipLaunchKernelGGL(jpeg_idct_kernel, dim3(idct_blocks), dim3(JP_BLOCK), 0, s, coef, jpegs, status, start, planes, g);
    BG_LAUNCH_CHECK();
    int gx = (max_pixels + JP_BLOCK - 1) / JP_BLOCK;        // the pixel loop strides, so a small max_pixels is only slow
    if (gx > JP_MAX_GRID_X) gx = JP_MAX_GRID_X;
    hipLaunchKernelGGL(jpeg_colour_kernel, dim3((unsigned)gx, (unsigned)n_jpeg), dim3(JP_BLOCK), 0, s, jpegs, status,
                       planes, raw);
    BG_LAUNCH_CHECK();
    return BG_OK;
}

}  // extern "C"
