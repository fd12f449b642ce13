// igemm16.hip - bf16-RESIDENT implicit-GEMM kernels for conv / transposed conv and their gradients (gfx950).
//
// Reference call sites replaced: tf.pad + tf.nn.conv2d (ops.py:82,94-98), tf.nn.conv2d_transpose (ops.py:127-132)
// and the gradients TensorFlow derives for them, in the bf16 configurations of BASELINE.json (configs 3-5).
//
// Why a second family next to igemm.hip / igemm_bf16.h: those kernels read fp32 tensors and round to bf16 while
// staging through VGPRs, which left the bf16 MFMA pipe 80-90 % idle.  Here every operand is
// ALREADY bf16 in HBM, so a tile goes global -> LDS with global_load_lds_dwordx4 (16 bytes per lane, no VGPRs, no
// VALU conversion), the gather of the implicit GEMM is just the per-lane SOURCE address of that instruction, and the
// K loop is {issue next tile's LDS-DMA ; ds_read_b128 fragments ; MFMA ; barrier}.
//
//   nn16_kernel  out[m, n] = sum_tap sum_c A(pixel(m), tap)[c] * B[tap][n][c]        (forward, input gradients)
//       block tile 128 x (32*TN) x 64, 4 waves (2 x 2), v_mfma_f32_16x16x32_bf16, fp32 accumulate (this is the two-stage
//       form; SLOTS = 3: a ring of 32-channel stages under the same or a 256-row tile; SLOTS = 2 with WM = 4: the phased
//       form, a 256 x 32 TN tile (TN = 4, 6, 8) on 8 waves at one block per CU whose LDS-DMA prefetch stays in flight across
//       raw barriers - the C >= 384 launches; see the kernel's header).
//       LDS image: rows of 64 bf16 (128 B); 16-byte chunk c of row r is stored at chunk position c ^ ((r >> 1) & 7):
//       LDS-DMA writes are lane-linear, so the swizzle is applied to the SOURCE chunk each lane fetches, and the
//       ds_read_b128 operand reads (lane -> row lane & 15, chunk lane >> 4) are bank-conflict free.
//       K is flattened over (tap, channel chunk): a 64-wide K step may straddle taps (C = 96), every lane keeps its
//       own (tap, channel) cursor.  Out-of-image taps, rows >= M, columns >= N and the K tail fetch a zero page.
//       The epilogue transposes the accumulators through LDS and stores whole 16-byte row segments
//       (bias, alpha, residual accumulate, bf16 or fp32 output).
//       PM = true (NN16Params::posmajor): rows enumerate (position, image) and a tile walks only the taps that have a
//       source at its positions - the frame of a reflect-padded gradient grid, the borders of 4 x 4 / 8 x 8 maps.
//   nn16h_kernel  the same product for 3 x 3 stride-1 gathers and the phases of 4 x 4 stride-2 transposed gathers on maps
//       whose sides are multiples of 16: a block owns a 16 x 16 pixel patch, loads its (16 + NT - 1)^2 source pixels per
//       64-channel chunk ONCE (pixel rows swizzled so that every tap shift reads conflict-free) and streams only the
//       weight tiles; 8 waves, two blocks per CU.
//   tn16_kernel  out[(tap, ca)][cb] = sum_pixels A(pixel, tap)[ca] * Bv(pixel)[cb]   (weight gradients)
//       both tiles stay PIXEL-major in LDS ([64 pixels][128 channels] bf16, chunk-swizzled) and the MFMA operands
//       are read transposed with ds_read_b64_tr_b16; fp32 split-K slabs over pixel ranges.
//   tn16x_kernel  the wide form of it: 256 x 128 output tile, 8 waves, v_mfma_f32_32x32x16_bf16, 3-stage LDS ring of
//       32-pixel stages filled by hand-counted LDS-DMA (s_waitcnt vmcnt(N)), two blocks per CU.
//   tn16x_phased_kernel  the same product on a 256 x 192 / 256 x 256 tile at ONE block per CU: a ring of 16-pixel K blocks,
//       operand reads one block ahead of the MFMAs, one raw barrier per block (launches chosen by tn16x_phased_bn).
#include <stdlib.h>

#include "common.h"
#include "igemm.h"
#include "igemm16.h"
#include "igemm16_plan.h"
#include <type_traits>
#include "igemm_dev.h"

namespace bg {

typedef float f32x4_t __attribute__((ext_vector_type(4)));
typedef float f32x16_t __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
typedef short s16x4v __attribute__((ext_vector_type(4)));
typedef short s16x8v __attribute__((ext_vector_type(8)));
typedef __attribute__((address_space(3))) void lds_void_t;
typedef __attribute__((address_space(1))) const void gbl_void_t;
typedef __attribute__((address_space(3))) s16x4v lds_s16x4v;

// the source of every out-of-range 16-byte chunk (zero-initialised device memory of the code object)
// 16 KB: a gather row without a source reads zeros at any channel offset (C <= 8192: the input gradient of the first
// level's sub-pixel convolution at config 3 reduces over 4 x 1536 channels per tap)
__device__ uint4 g_zero_page[1024];

__device__ __forceinline__ void glds16(const void* src, unsigned char* lds_wave_base) {
    // LDS destination = wave-uniform base + lane * 16 ; the global source address is per lane
    __builtin_amdgcn_global_load_lds((gbl_void_t*)src, (lds_void_t*)lds_wave_base, 16, 0, 0);
}

// The same LDS-DMA in inline assembly (MI355X guide 5.7: M0 written in the statement that reads it).  hipcc does not
// model it: it neither counts it in vmcnt nor knows that LDS is written, so the kernel owns the counted
// s_waitcnt vmcnt(N) + barrier before the ds_reads of that tile - and the compiler does NOT drain the queue with a
// vmcnt(0) in front of every ds_read that follows an LDS-DMA in program order, which it does for the builtin
// (SIInsertWaitcnts treats an in-flight LDS-DMA as a store that any LDS read may alias).  That drain is what caps a
// ring with more than one tile in flight; the 2-stage kernels, which wait for everything at their barrier anyway,
// keep the builtin.  lds_byte_addr must be wave-uniform.
__device__ __forceinline__ void glds16_asm(const void* src, uint32_t lds_byte_addr) {
    unsigned keep;
    const uint32_t dst = __builtin_amdgcn_readfirstlane(lds_byte_addr);
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep)
                 : "v"(src), "s"(dst)
                 : "memory");
}

__device__ __forceinline__ uint32_t pack_bf16x2(float a, float b) {
    typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
    bf16x2_t v;
    v[0] = (__bf16)a;
    v[1] = (__bf16)b;
    return __builtin_bit_cast(uint32_t, v);
}
__device__ __forceinline__ float bf16_lo(uint32_t u) { return __builtin_bit_cast(float, u << 16); }
__device__ __forceinline__ float bf16_hi(uint32_t u) { return __builtin_bit_cast(float, u & 0xffff0000u); }

// ------------------------------------------------------------------------------------------
// NN kernel
// ------------------------------------------------------------------------------------------
constexpr int NN16_BM = 128;      // block tile rows; the K step is 64 bf16 = one 128-byte LDS row
constexpr int NN16_TAPS = 4;      // taps per axis one block walks (kernel sizes 1, 3, 4)
constexpr int NN16_RING_TAPS = 8; // per-axis tap slots of a ring launch (NN16Params::ring): k real + k mirrored, k <= 4
constexpr int nn16_lds_bytes(int TN, int TAPS = NN16_TAPS) {
    const int stage = (NN16_BM + 32 * TN) * 128;
    const int epi = NN16_BM * (32 * TN + 4) * 4;
    const int tab = 2 * TAPS * NN16_BM * 4;                    // gather tables [axis][tap][row] of int32 behind the stages
    // + output pixel of every row + the tile's tap flags (in the dynamic block on purpose: a static __shared__ variable
    // moves the stages off their 1 KB alignment, which costs the LDS-DMA writes of the HBM-bound layers ~25 %)
    return (2 * stage + tab > epi ? 2 * stage + tab : epi) + NN16_BM * 4 + 16;
}
// ring forms (SLOTS = 3): three stages of 32 channels (64-byte rows), row tables [axis 0: int32 | axis 1: int16], the
// epilogue passes through the ring area in parts of 64 rows
constexpr int nn16_pipe_lds_bytes(int TN, int WM, int TAPS = NN16_TAPS) {
    const int bm = 64 * WM;
    return 3 * (bm + 32 * TN) * 64 + TAPS * bm * (4 + 2) + bm * 4 + 16;
}
// phased form (SLOTS = 2, WM = 4): two 64-channel stages of a 256 x 32 TN tile, int32 row tables, tabo, the tap flags; the
// epilogue passes through the front in two parts of 128 rows
constexpr int nn16x_lds_bytes(int TN) {
    return 2 * (256 + 32 * TN) * 128 + 2 * NN16_TAPS * 256 * 4 + 256 * 4 + 16;
}
constexpr int NN16_NOSRC = -(1 << 30);                         // table entry of a tap without a source pixel

// element offset of the source pixel of row r under tap (kh, kw), or -1 (selects, no divergent branches)
template <int MODE>
__device__ __forceinline__ int64_t nn16_src_off(const Gather& g, const RowPos& r, int kh, int kw) {
    int h, w;
    if (MODE == GATHER_CONV) {
        h = conv_src(r.ho, kh, g.stride, g.pad, g.reflect, g.Hs);
        w = conv_src(r.wo, kw, g.stride, g.pad, g.reflect, g.Ws);
    } else {
        h = tconv_src_from_num(r.ho + g.pad - kh, g.stride, g.Hs);
        w = tconv_src_from_num(r.wo + g.pad - kw, g.stride, g.Ws);
    }
    const bool ok = r.valid && h >= 0 && w >= 0;
    const int pix = (r.b * g.Hs + h) * g.Ws + w;          // < 2^31 (checked on the host)
    return ok ? (int64_t)pix * g.ld : (int64_t)-1;
}

// row of the implicit GEMM -> output pixel of this stride phase (shifts when the phase grid is a power of two: the
// divisions of decompose_row cost ~90 VALU instructions per row, as much as several K steps of a C = 96 layer)
// padded position that tf.pad(REFLECT) (pad 1) fills from pixel o of an axis of n pixels, beyond o itself: -1 for o = 1,
// n for o = n - 2 (when the high border is padded at all); NN16_NOMIRROR otherwise
constexpr int NN16_NOMIRROR = -(1 << 20);
__device__ __forceinline__ int nn16_mirror_pos(int o, int n, bool hi) {
    return o == 1 ? -1 : ((hi && o == n - 2) ? n : NN16_NOMIRROR);
}

template <int MODE, bool PM, bool RING = false>
__device__ __forceinline__ RowPos nn16_row(const NN16Params& p, int m, int ph, int pw) {
    RowPos r;
    if (PM) {                                      // image fastest: every row of a tile sits at (nearly) the same position
        r.valid = m < p.M;
        const int pos = m / p.g.Nb;
        r.b = m - pos * p.g.Nb;
        if (RING) {
            // the pixels that receive mirrored taps, each once: rows {1, Ho - 2} in full, then columns {1, Wo - 2} without
            // those rows (ring_lines == 1: row 1 and column 1 only)
            const int L = p.ring_lines, first = L * p.g.Wo;
            if (pos < first) {
                const int line = pos / p.g.Wo;
                r.ho = line == 0 ? 1 : p.g.Ho - 2;
                r.wo = pos - line * p.g.Wo;
            } else {
                const int per = p.g.Ho - L, q = pos - first;
                const int line = q / per, idx = q - line * per;
                r.wo = line == 0 ? 1 : p.g.Wo - 2;
                r.ho = idx == 0 ? 0 : ((L == 2 && idx > p.g.Ho - 4) ? p.g.Ho - 1 : idx + 1);
            }
            return r;
        }
        const int hq = pos / p.g.Wq;
        r.ho = hq * p.g.pstep + ph;
        r.wo = (pos - hq * p.g.Wq) * p.g.pstep + pw;
        return r;
    }
    if (MODE == GATHER_PLAIN || !p.pow2) return decompose_row<MODE>(p.g, m, p.M, ph, pw);
    r.valid = m < p.M;
    const int wq = m & (p.g.Wq - 1);
    const int t = m >> p.wq_shift;
    const int hq = t & (p.g.Hq - 1);
    r.b = t >> p.hq_shift;
    r.ho = hq * p.g.pstep + ph;
    r.wo = wq * p.g.pstep + pw;
    return r;
}

// PM: position-major rows and a K walk over the tile's own taps (NN16Params::posmajor); the image-major form is its own
// instantiation because the tap bookkeeping costs the short-K launches (1 x 1 convolutions: 3 K steps) 25 %.
// RING (NN16Params::ring; PM launches of transposed gathers only): 8 tap slots per axis = real taps followed by the taps
// of the mirrored padded position.
//
// SLOTS / WM - how deep the operand pipeline of a block is (chosen per launch by nn16_form):
//   SLOTS = 2, WM = 2  two 64-channel stages, ONE tile in flight: stage(next) ; 8 TN MFMAs per wave ; vmcnt(0) ; barrier.
//       At TN = 4 the MFMAs of a step take ~0.21 us and the tile they wait for was issued that long ago, while an LDS-DMA
//       takes on the order of a microsecond from issue to landing: a block is parked for most of a step and only the CU's
//       second block (70 KB of LDS each) fills the matrix pipe - mfma_busy 0.50, 39 % of wave cycles waiting (r02 counters,
//       384 -> 384 at 32^2).
//   SLOTS = 3, WM = 2  the same 128 x 32 TN tile on a 3-slot ring of 32-channel stages (64-byte LDS rows, chunk c of row r at
//       c ^ ((r >> 1) & 2)): tile s + 2 is issued right after the barrier of step s and the wait in front of that barrier is
//       a counted vmcnt that leaves the newest tile in flight (tn16x_kernel's kstep).  Two tiles in flight per block, and
//       52.7 KB of LDS (the epilogue goes through LDS in halves) let three blocks share a CU.
//   SLOTS = 3, WM = 4  the same ring under a 256 x 32 TN tile on 8 waves (2 A + <= 1 B LDS-DMA per wave and stage): a quarter
//       fewer L2 -> LDS bytes per FLOP; two blocks per CU, <= 128 VGPRs.
//   SLOTS = 2, WM = 4  the phased form: a 256 x 32 TN tile (TN = 4, 6, 8) on 8 waves, ONE block per CU (<= 250 VGPRs, 107 -
//       140 KB of LDS), two 64-channel stages that keep whole 128-byte lines (the two-stage form's chunk swizzle), filled
//       half by half (A rows 0 - 127 / 128 - 255, B columns below / from BN / 2) by LDS-DMA that stays in flight across raw
//       barriers.  A K tile is four phases, one accumulator quadrant each: {ds_read_b128 fragments ; one half of prefetch ;
//       s_barrier ; lgkmcnt(0) ; s_setprio(1) ; MFMAs ; s_setprio(0) ; s_barrier}, with ONE counted vmcnt per tile - the
//       schedule and its read-after-write / write-after-read argument stand at the loop.  Row tables, K cursor (set_tap /
//       advance), zero page, tap mask and the epilogue in parts are the two-stage form's own code.
// Every form feeds an accumulator the same sequence of 32-channel MFMA K blocks (the split-K partition stays in 64-channel
// steps = two stages), so their results are bit-identical.
// Measured (profiles/nn16_pipe_ab.txt; 384 -> 384 at 32^2 on this kernel, 256 images): mfma_busy 0.495 with two stages, 0.414
// with the 128-row ring, 0.530 with the wide form; no LDS bank conflicts in any.  The 64-byte rows cost more than the deeper
// pipeline buys wherever weights stream (each 128-byte line is requested twice, a step apart: the CU's L2 read requests
// double), so the 128-row ring is a default nowhere and the wide form takes the image-major launches with C <= 192; the
// phased form takes the C >= 384 launches whose one-block-per-CU grid comes out in whole rounds (profiles/nn16x_phase_ab.txt:
// 1536 -> 768 k4 s2 at 8^2 0.64 -> 0.47 ms at BN = 256, 1536 -> 1536 k3 at 8^2 0.617 -> 0.566 at BN = 192) - see nn16_form for
// the per-layer numbers.
template <int TN, int MODE, bool PM, bool RING = false, int SLOTS = 2, int WM = 2>
__global__ __launch_bounds__(128 * WM, SLOTS == 2 ? 2 : (WM == 4 ? 4 : 3)) void nn16_kernel(const NN16Params p) {
    static_assert(!RING || (PM && MODE == GATHER_TCONV), "ring launches are position-major transposed gathers");
    static_assert((SLOTS == 2 && (WM == 2 || WM == 4)) || (SLOTS == 3 && (WM == 2 || WM == 4)),
                  "two stages (WM = 4: the phased form), or a 3-slot ring on 4 / 8 waves");
    constexpr bool PIPE = SLOTS == 3;
    constexpr bool PHASED = SLOTS == 2 && WM == 4;
    static_assert(!PHASED || (!RING && (TN == 4 || TN == 6 || TN == 8)), "phased form: 128, 192 or 256 columns, no mirrored taps");
    static_assert(PHASED || TN <= 4, "tiles of at most 128 columns");
    constexpr int TAPS = RING ? NN16_RING_TAPS : NN16_TAPS;
    constexpr int LDS_BYTES = PIPE ? nn16_pipe_lds_bytes(TN, WM, TAPS) : (PHASED ? nn16x_lds_bytes(TN) : nn16_lds_bytes(TN, TAPS));
    typedef typename std::conditional<RING, uint64_t, unsigned>::type mask_t;
    typedef typename std::conditional<PIPE, int16_t, int>::type tabw_t;     // column table entries (source column, < 0: none)
    constexpr int BM = 64 * WM, BN = 32 * TN, NTHR = 128 * WM, NWV = 2 * WM;
    constexpr int CPS = PIPE ? 4 : 8;              // 16-byte chunks of K per stage = per LDS row
    constexpr int ROWB = 16 * CPS;                 // bytes of an LDS row
    constexpr int RSTR = PIPE ? 16 * NWV : 8 * NWV;     // rows between the LDS-DMA instructions of a wave (1 KB = 1024 / ROWB rows each)
    // LDS-DMA instructions per wave and stage; PIPE: wave w stages the 16-row groups w, w + NWV, ... below BN / 16
    constexpr int JA = BM / RSTR, JB = PIPE ? (BN / 16 + NWV - 1) / NWV : (PHASED ? 2 * ((BN / 2 + 63) / 64) : BN / RSTR);
    constexpr int A_BYTES = BM * ROWB, STAGE = (BM + BN) * ROWB;
    static_assert(BM == NN16_BM || PIPE || PHASED, "the two-stage form has 128-row tiles");
    static_assert(!PHASED || (LDS_BYTES <= 160 * 1024 && 128 * (BN + 4) * 4 <= LDS_BYTES - 16 - BM * 4),
                  "phased form: one block per CU; a 128-row part of the epilogue ends in front of tabo");
    static_assert(A_BYTES % 1024 == 0 && STAGE % 1024 == 0 && (RSTR * ROWB) % 1024 == 0,
                  "every LDS-DMA destination is 1 KB aligned");
    static_assert(!PIPE || 64 * (BN + 4) * 4 <= SLOTS * STAGE, "a 64-row part of the epilogue fits in front of the tables");
    static_assert(!PIPE || RING || LDS_BYTES * (WM == 4 ? 2 : 3) <= 160 * 1024, "ring forms: 3 (8 waves: 2) blocks per CU");
    static_assert(!PIPE || LDS_BYTES * 2 <= 160 * 1024, "mirrored-tap ring launches: 2 blocks per CU");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];

    const int t = threadIdx.x;
    const int lane = t & 63, w = (PIPE || PHASED) ? __builtin_amdgcn_readfirstlane(t >> 6) : t >> 6;
    const int wm = w >> 1, wn = w & 1;
    const Gather& g = p.g;

    // Tile order inside an XCD's contiguous share of the grid (NN16Params::mfast): N-tiles fastest keeps an M-tile's gathered
    // rows in that L2 while the weight slabs stream past (right when the activations are the big operand); M-tiles fastest
    // keeps ONE weight slab (one phase, one N-column: <= 1.5 MB) resident while the rows stream (right for the 4 x 4 ...
    // 16 x 16 layers, whose weights are 5 - 20 x their activations and were re-fetched once per M-tile: 1.9 GB per launch
    // in round 2's counters).
    int tile_m, tile_n, bz = blockIdx.z;
    if (p.zfold > 0) {
        const int lin = xcd_remap(blockIdx.x, p.tiles_m * p.tiles_n * p.zfold);
        if (p.mfast) {
            tile_m = lin % p.tiles_m;
            const int r_ = lin / p.tiles_m;
            bz = r_ % p.zfold;
            tile_n = r_ / p.zfold;
        } else {
            bz = lin % p.zfold;
            const int tile = lin / p.zfold;
            tile_n = tile % p.tiles_n;
            tile_m = tile / p.tiles_n;
        }
    } else {
        const int tile = xcd_remap(blockIdx.x, p.tiles_m * p.tiles_n);
        if (p.mfast) {
            tile_m = tile % p.tiles_m;
            tile_n = tile / p.tiles_m;
        } else {
            tile_n = tile % p.tiles_n;
            tile_m = tile / p.tiles_n;
        }
    }
    const int m0 = tile_m * BM, n0 = tile_n * BN;
    const int zs = bz % p.splitk, zo = bz / p.splitk;

    int ph = 0, pw = 0;
    if (MODE == GATHER_TCONV) {
        ph = g.pstep - 1 - zo / g.pstep;           // heaviest stride phase first
        pw = g.pstep - 1 - zo % g.pstep;
    }
    int kh0 = 0, kw0 = 0, kstep = 1, nkh = g.k, nkw = g.k;
    if (MODE == GATHER_TCONV && g.pstep > 1) {
        kstep = g.stride;
        kh0 = (ph + g.pad) % g.stride;
        kw0 = (pw + g.pad) % g.stride;
        nkh = (g.k - kh0 + g.stride - 1) / g.stride;
        nkw = (g.k - kw0 + g.stride - 1) / g.stride;
    }
    // ring launches: per axis g.k real taps (kk = i) followed by g.k taps of the mirrored position (kk = i - g.k); the
    // (real, real) pairs belong to the plain launch and are left out of the walk
    int nrh = 0, nrw = 0;
    if (RING) {
        nrh = nrw = g.k;
        nkh = nkw = 2 * g.k;
    }
    const int C8 = p.C >> 3;
    const int ntap = nkh * nkw;

    // ---- gather tables ----
    // The source pixel of (row, tap) separates into a row part and a column part: tabh[ih][row] = (b Hs + h) Ws and
    // tabw[iw][row] = w (NN16_NOSRC where the tap has no source).  Built once per block; a tap change in the K walk
    // then costs two LDS reads and an add per row instead of the whole gather arithmetic (which made the C = 96
    // layers, where the tap changes every 1.5 K steps, VALU-bound at ~11 VALU instructions per MFMA).
    // s_any: bit (axis * NN16_TAPS + i) = some row of this tile has a source under tap i of that axis.  Taps without
    // any are left out of the K walk: the border tiles of a position-major launch (p.posmajor) then cost what their
    // sources cost, not k x k zero-page tiles.
    unsigned& s_any = *reinterpret_cast<unsigned*>(smem + LDS_BYTES - 16);
    if (PM) {
        if (t == 0) s_any = 0;
        __syncthreads();
    }
    unsigned any_local = 0;
    int* tabh = reinterpret_cast<int*>(smem + SLOTS * STAGE);
    tabw_t* tabw = reinterpret_cast<tabw_t*>(tabh + TAPS * BM);
    for (int e = t; e < 2 * TAPS * BM; e += NTHR) {
        const int axis = e / (TAPS * BM), i = (e / BM) % TAPS, row = e % BM;
        const RowPos r = nn16_row<MODE, PM, RING>(p, m0 + row, ph, pw);
        int v = NN16_NOSRC;
        if (r.valid && i < (axis ? nkw : nkh)) {
            int kk = (axis ? kw0 : kh0) + i * kstep;
            int o = axis ? r.wo : r.ho;
            const int n = axis ? g.Ws : g.Hs;
            if (RING) {
                const int nr = axis ? nrw : nrh;
                if (i >= nr) {                         // tap of the mirrored padded position
                    kk = i - nr;
                    o = nn16_mirror_pos(o, axis ? g.Wo : g.Ho, p.ring_lines == 2);
                }
            }
            const int src = MODE == GATHER_CONV ? conv_src(o, kk, g.stride, g.pad, g.reflect, n)
                                                : (o == NN16_NOMIRROR ? -1 : tconv_src_from_num(o + g.pad - kk, g.stride, n));
            if (src >= 0) {
                v = axis ? src : (r.b * g.Hs + src) * g.Ws;
                any_local |= 1u << (axis * TAPS + i);
            }
        }
        if (PIPE && axis) tabw[e - TAPS * BM] = (tabw_t)(v < 0 ? -1 : v);      // (source columns < 2^15: nn16_form)
        else tabh[e] = v;
    }
    if (PM && any_local) atomicOr(&s_any, any_local);
    // output pixel of every row (transposed gathers: rows enumerate a stride phase, possibly of a padded grid), behind
    // everything the epilogue overlays; 0xffffffff = no output
    unsigned* tabo = reinterpret_cast<unsigned*>(smem + LDS_BYTES - 16 - BM * 4);
    constexpr bool use_tabo = MODE == GATHER_TCONV || PM;
    if (use_tabo && t < BM) {
        const RowPos r = nn16_row<MODE, PM, RING>(p, m0 + t, ph, pw);
        tabo[t] = (r.valid && r.ho < g.Ho && r.wo < g.Wo) ? (unsigned)((r.b * g.Ho + r.ho) * g.Wo + r.wo) : 0xffffffffu;
    }

    // ---- staging role of this lane: 16-byte chunk `cch` of the K step, rows 32 j + rsub of both tiles ----
    // (PIPE: 4 chunks per row, an instruction covers 16 rows; chunk c of row r sits at c ^ ((r >> 1) & 2))
    const int cch = PIPE ? (lane & 3) ^ ((lane >> 3) & 2) : (lane & 7) ^ ((((w & 1) << 2) | (lane >> 4)) & 7);
    const int rsub = PIPE ? 16 * w + (lane >> 2) : 8 * w + (lane >> 3);
    // PIPE: B instructions of this wave per stage (wave-uniform; the counted waits need it as a constant per branch)
    constexpr int NB_HI = JB, NB_LO = (BN / 16) / NWV;
    const int nbw = (PIPE && NB_HI != NB_LO) ? (BN / 16 - w + NWV - 1) / NWV : JB;
    const unsigned char* abase = reinterpret_cast<const unsigned char*>(p.A);
    const unsigned char* bbase = reinterpret_cast<const unsigned char*>(p.B);
    const unsigned char* zero = reinterpret_cast<const unsigned char*>(g_zero_page);
    const unsigned ald2 = 2u * (unsigned)g.ld;
    const uint32_t lds0 = static_cast<uint32_t>(
        reinterpret_cast<uintptr_t>((__attribute__((address_space(3))) unsigned char*)smem));

    __syncthreads();                     // tables (and s_any) complete
    // PM: taps this tile walks, bit (ih * NN16_TAPS + iw), in the (ih, iw) order of the packed weights
    mask_t tapmask = 0;
    if (PM) {
        const unsigned any = __builtin_amdgcn_readfirstlane(s_any);      // block-uniform: the K loop stays scalar
        for (int i = 0; i < nkh; ++i)
            for (int j = 0; j < nkw; ++j)
                if (((any >> i) & (any >> (TAPS + j)) & 1u) != 0 && !(RING && i < nrh && j < nrw))
                    tapmask |= (mask_t)1 << (i * TAPS + j);
    }
    const int nsteps_all = ((PM ? __builtin_popcountll((uint64_t)tapmask) : ntap) * C8 + 7) >> 3;
    const int sps = (nsteps_all + p.splitk - 1) / p.splitk;
    const int it0 = zs * sps;
    const int nsteps = max(0, min(nsteps_all, it0 + sps) - it0);

    // K cursor of this lane.  Image-major: tap index tidx = (ih, iw).  PM: rem = the taps from the current one on
    // (lowest set bit = current).
    mask_t rem = tapmask;
    int tidx = 0, c8, ih = 0, iw = 0;
    {
        const int kk = it0 * 8 + cch;
        tidx = kk / C8;
        c8 = kk - tidx * C8;
        if (PM) {
            for (int i = 0; i < tidx && rem; ++i) rem &= rem - 1;
        } else {
            ih = tidx / nkw;
            iw = tidx - ih * nkw;
        }
    }
    const unsigned char* asrc[JA];       // source of this lane's chunk at channel 0 of the current tap (or the zero page)
    const unsigned char* wsrc[JB];
    auto set_tap = [&]() {
        bool kvalid;
        if (PM) {
            kvalid = rem != 0;
            const int bit = kvalid ? __builtin_ctzll((uint64_t)rem) : 0;
            ih = bit / TAPS;
            iw = bit % TAPS;
        } else {
            kvalid = tidx < ntap;
        }
        const int* th = tabh + (ih & (TAPS - 1)) * BM + rsub;
        const tabw_t* tw = tabw + (iw & (TAPS - 1)) * BM + rsub;
#pragma unroll
        for (int j = 0; j < JA; ++j) {
            int col = tw[RSTR * j];
            if (PIPE) col = col < 0 ? NN16_NOSRC : col;
            const int pix = th[RSTR * j] + col;
            asrc[j] = (kvalid & (pix >= 0)) ? abase + (uint64_t)(unsigned)pix * ald2 : zero;
        }
        const int kh = RING ? (ih >= nrh ? ih - nrh : ih) : kh0 + ih * kstep;
        const int kw = RING ? (iw >= nrw ? iw - nrw : iw) : kw0 + iw * kstep;
        const unsigned char* wt = bbase + 2 * (int64_t)(kh * g.k + kw) * p.tap_stride;
#pragma unroll
        for (int j = 0; j < JB; ++j) {
            // (phased form: the B halves of BN / 2 rows are staged apart, JB / 2 instructions of 64 rows each; at BN = 192 the
            //  second one of a half covers 32 rows and the waves 4 - 7 have no part in it)
            const int brow = PHASED ? (BN / 2) * (j / (JB / 2)) + 64 * (j % (JB / 2)) + rsub : RSTR * j + rsub;
            const bool inside = !PHASED || 64 * (j % (JB / 2)) + rsub < BN / 2;
            const int n = n0 + brow;
            wsrc[j] = (kvalid & inside & (n < p.N)) ? wt + 2 * (uint64_t)((unsigned)n * (unsigned)p.C) : zero;
        }
    };
    set_tap();
    auto advance = [&]() {               // the K cursor moves on by one stage
        c8 += CPS;
        if (c8 >= C8) {
            do {
                c8 -= C8;
                if (PM) {
                    rem &= rem - 1;
                } else {
                    ++tidx;
                    if (++iw == nkw) {
                        iw = 0;
                        ++ih;
                    }
                }
            } while (c8 >= C8);
            set_tap();
        }
    };

    // LDS-DMA through glds16_asm: the table reads of set_tap follow the DMA issue in program order, and behind the
    // builtin the compiler would drain the queue (vmcnt(0)) in front of them; the wait before the barrier is explicit
    auto stage = [&](int buf) {
        const uint32_t sa = lds0 + buf * STAGE + w * 1024;       // (1 KB = the rows of one instruction)
        const uint32_t sb = sa + A_BYTES;
        const unsigned cbyte = 16u * (unsigned)c8;
#pragma unroll
        for (int j = 0; j < JA; ++j) glds16_asm(asrc[j] + cbyte, sa + j * RSTR * ROWB);
#pragma unroll
        for (int j = 0; j < JB; ++j)
            if (!PIPE || j < nbw) glds16_asm(wsrc[j] + cbyte, sb + j * RSTR * ROWB);
        advance();
    };

    // ONE accumulator array per instantiation, shaped by the form and named by it: acc[16-row fragment][16-column fragment]
    // of the wave's tile, or (phased form) accx by quadrant, [A half][16-row fragment][B half][16-column fragment].  Each
    // name is used only inside the `if constexpr` branches of its form.
    constexpr int XMI = PHASED ? (TN == 8 ? 4 : 2) : 1, XNJ = PHASED ? (TN == 6 ? 3 : 2) : 1;
    typedef f32x4_t acc_plain_t[4][TN];
    typedef f32x4_t acc_quad_t[2][XMI][2][XNJ];
    typename std::conditional<PHASED, acc_quad_t, acc_plain_t>::type accv;
    auto& acc = accv;
    auto& accx = accv;
    if constexpr (PHASED) {
#pragma unroll
        for (int i = 0; i < 2 * XMI; ++i)
#pragma unroll
            for (int j = 0; j < 2 * XNJ; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r) accx[i / XMI][i % XMI][j / XNJ][j % XNJ][r] = 0.f;
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r) acc[i][j][r] = 0.f;
    }

    if constexpr (PIPE) {
        // operand reads: lane -> row (lane & 15) of a 16-row fragment, chunk (lane >> 4) of the stage's one K block
        const int frag = (lane & 15) * ROWB + 16 * ((lane >> 4) ^ (((lane & 15) >> 1) & 2));
        const unsigned char* a_ad = smem + wm * 64 * ROWB + frag;
        const unsigned char* b_ad = smem + A_BYTES + wn * 16 * TN * ROWB + frag;
        const int nst = 2 * nsteps;                // a 64-channel K step = two stages
        if (nst > 0) stage(0);
        if (nst > 1) stage(1);
        // one stage on ring slot SLOT (a compile-time constant: operand addresses = base + immediate)
        auto kstep = [&](int it, auto slot_c) {
            constexpr int SLOT = decltype(slot_c)::value;
            // tile `it` has landed (this wave's part; the barrier extends that to every wave), tile it + 1 stays in flight:
            // JA + nbw LDS-DMA instructions of this wave
            if (it + 1 < nst) {
                if (NB_HI == NB_LO || nbw == NB_HI) asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(JA + NB_HI) : "memory");
                else asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(JA + NB_LO) : "memory");
            } else
                asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            if (it + 2 < nst) stage((SLOT + 2) % 3);    // the slot every wave finished reading before this barrier
            bf16x8_t a[4], b[TN];
#pragma unroll
            for (int i = 0; i < 4; ++i) a[i] = *reinterpret_cast<const bf16x8_t*>(a_ad + SLOT * STAGE + i * 16 * ROWB);
#pragma unroll
            for (int j = 0; j < TN; ++j) b[j] = *reinterpret_cast<const bf16x8_t*>(b_ad + SLOT * STAGE + j * 16 * ROWB);
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(b[j], a[i], acc[i][j], 0, 0, 0);
        };
        for (int it = 0; it < nst; it += 3) {
            kstep(it, std::integral_constant<int, 0>());
            if (it + 1 < nst) kstep(it + 1, std::integral_constant<int, 1>());
            if (it + 2 < nst) kstep(it + 2, std::integral_constant<int, 2>());
        }
        __syncthreads();                           // every wave has read its last stage: the epilogue overlays the ring
    } else if constexpr (PHASED) {
        // Two K tiles per loop trip, four phases per tile, one accumulator quadrant per phase.  Waves: 2 (rows) x 4 at BN = 256,
        // 4 x 2 at BN = 192 and 128.  Wave (wmx, wnx) owns the rows 128 h + 16 XMI wmx + 16 i (i < XMI) and the columns
        // (BN / 2) hn + 16 XNJ wnx + 16 j (j < XNJ) of the tile (h, hn = 0, 1), so quadrant (h, hn)
        // reads only the A half h and the B half hn of a stage, and a half is free for the tile after next as soon as its
        // quadrants are read.  Tile u sits in buffer u & 1; its phases q = 0 .. 3 are
        //   q  quadrant  ds_read_b128        LDS-DMA issued (2 A / JBH B instructions per wave)
        //   0  (0, 0)    B half 0, A half 0  A half 1 of tile u + 1, then the K cursor moves on to tile u + 2
        //   1  (0, 1)    B half 1            A half 0 of tile u + 2   (last read: phase 0)
        //   2  (1, 1)    A half 1            B half 0 of tile u + 2   (last read: phase 0, kept in registers for phase 3)
        //   3  (1, 0)    -                   B half 1 of tile u + 2   (last read: phase 1) ; s_waitcnt vmcnt(NFLY)
        // and every phase is {reads ; issue ; s_barrier ; lgkmcnt(0) ; MFMAs ; s_barrier}.  Write after read: a half is
        // restaged one phase after its last read, and those reads were retired by the lgkmcnt(0) every wave passes before
        // the closing barrier of the reading phase.  Read after write: the one counted wait of a tile, in front of the first
        // barrier of phase 3, leaves the three halves of tile u + 2 in flight (2 + 2 x the B instructions of this wave per
        // half: JBH, at BN = 192 one fewer in the waves 4 - 7) and so retires everything of tile u + 1, whose first read is a
        // phase later, behind that barrier.
        constexpr int WNX = TN == 8 ? 4 : 2, JBH = JB / 2;
        static_assert(JA == 4 && (8 / WNX) * XMI * 16 == 128 && WNX * XNJ * 16 == BN / 2, "halves of 128 rows / BN / 2 columns");
        const int wmx = w / WNX, wnx = w % WNX;
        const bool b_short = TN == 6 && w >= 4;        // (wave-uniform: w is scalar)
        const int fsw = (lane & 15) >> 1;
        const int a_row = (wmx * 16 * XMI + (lane & 15)) * 128;
        const int b_row = A_BYTES + (wnx * 16 * XNJ + (lane & 15)) * 128;
        int koff[2];
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2) koff[s2] = 16 * ((4 * s2 + (lane >> 4)) ^ fsw);
        // LDS-DMA of one half of the K cursor's tile into buffer `buf` (h: a compile-time constant)
        auto piece_a = [&](int buf, auto h_c) {
            constexpr int H = decltype(h_c)::value;
            const uint32_t sa = lds0 + buf * STAGE + w * 1024;
            const unsigned cbyte = 16u * (unsigned)c8;
#pragma unroll
            for (int j = 2 * H; j < 2 * H + 2; ++j) glds16_asm(asrc[j] + cbyte, sa + j * RSTR * ROWB);
        };
        auto piece_b = [&](int buf, auto h_c) {
            constexpr int H = decltype(h_c)::value;
            const uint32_t sb = lds0 + buf * STAGE + w * 1024 + A_BYTES;
            const unsigned cbyte = 16u * (unsigned)c8;
#pragma unroll
            for (int jj = 0; jj < JBH; ++jj)
                if (jj == 0 || !b_short) glds16_asm(wsrc[JBH * H + jj] + cbyte, sb + ((BN / 2) * H + 64 * jj) * ROWB);
        };
        auto wait_fly = [&]() {            // everything but this wave's part of the newest three halves has landed
            if (b_short) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * JBH) : "memory");
            else asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 + 2 * JBH) : "memory");
        };
        const std::integral_constant<int, 0> c0;
        const std::integral_constant<int, 1> c1;
        auto read_a = [&](bf16x8_t (&a)[2][XMI], const unsigned char* sbuf, int h) {
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
                for (int i = 0; i < XMI; ++i)
                    a[s2][i] = *reinterpret_cast<const bf16x8_t*>(sbuf + a_row + (128 * h + 16 * i) * 128 + koff[s2]);
        };
        auto read_b = [&](bf16x8_t (&b)[2][XNJ], const unsigned char* sbuf, int hn) {
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
                for (int j = 0; j < XNJ; ++j)
                    b[s2][j] = *reinterpret_cast<const bf16x8_t*>(sbuf + b_row + ((BN / 2) * hn + 16 * j) * 128 + koff[s2]);
        };
        auto mid = [&]() {                 // the phase's reads and LDS-DMA are issued: meet, then wait for the reads alone
            __builtin_amdgcn_s_barrier();
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_sched_barrier(0);
            __builtin_amdgcn_s_setprio(1);
        };
        auto close = [&]() {
            __builtin_amdgcn_s_setprio(0);
            __builtin_amdgcn_sched_barrier(0);
            __builtin_amdgcn_s_barrier();
        };
        // weights as the MFMA's first operand; every accumulator takes K block 0, then K block 1 of the tile
        auto quad = [&](auto h_c, auto hn_c, const bf16x8_t (&a)[2][XMI], const bf16x8_t (&b)[2][XNJ]) {
            constexpr int H = decltype(h_c)::value, HN = decltype(hn_c)::value;
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
                for (int i = 0; i < XMI; ++i)
#pragma unroll
                    for (int j = 0; j < XNJ; ++j)
                        accx[H][i][HN][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(b[s2][j], a[s2][i], accx[H][i][HN][j], 0, 0, 0);
        };
        // TAIL: one of the last two tiles of the range - the issues are conditional and the wait drains the queue
        auto ktile = [&](int u, auto buf_c, auto tail_c) {
            constexpr int BUF = decltype(buf_c)::value;
            constexpr bool TAIL = decltype(tail_c)::value;
            const unsigned char* sbuf = smem + BUF * STAGE;
            const bool n1 = !TAIL || u + 1 < nsteps, n2 = !TAIL || u + 2 < nsteps;
            bf16x8_t a[2][XMI], b0[2][XNJ], b1[2][XNJ];
            read_b(b0, sbuf, 0);
            __builtin_amdgcn_sched_barrier(0);
            read_a(a, sbuf, 0);
            if (n1) {
                piece_a(BUF ^ 1, c1);
                advance();
            }
            mid();
            quad(c0, c0, a, b0);
            close();
            read_b(b1, sbuf, 1);
            if (n2) piece_a(BUF, c0);
            mid();
            quad(c0, c1, a, b1);
            close();
            read_a(a, sbuf, 1);
            if (n2) piece_b(BUF, c0);
            mid();
            quad(c1, c1, a, b1);
            close();
            if (n2) {
                piece_b(BUF, c1);
                wait_fly();
            } else {
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            }
            mid();
            quad(c1, c0, a, b0);
            close();
        };
        // prologue: tile 0 whole, tile 1 without its A half 1 (phase 0 of tile 0 issues it) - the state every tile starts from
        if (nsteps > 0) {
            piece_a(0, c0);
            piece_b(0, c0);
            piece_b(0, c1);
            piece_a(0, c1);
            advance();
        }
        if (nsteps > 1) {
            piece_a(1, c0);
            piece_b(1, c0);
            piece_b(1, c1);
            wait_fly();
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        } else {
            asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        }
        __builtin_amdgcn_s_barrier();
        const std::integral_constant<bool, false> steady;
        const std::integral_constant<bool, true> tail;
        int u = 0;
        for (; u + 4 <= nsteps; u += 2) {          // (tile u + 3 exists: both tiles prefetch unconditionally)
            ktile(u, c0, steady);
            ktile(u + 1, c1, steady);
        }
        if (u < nsteps) ktile(u, c0, tail);
        if (u + 1 < nsteps) ktile(u + 1, c1, tail);
        if (u + 2 < nsteps) ktile(u + 2, c0, tail);
        // (the closing barrier of the last phase, or the prologue's: every read and LDS-DMA is done, the epilogue overlays)
    } else {
    // operand reads: lane -> row (lane & 15) of a 16-row fragment, chunk 4 s + (lane >> 4), swizzled by (row >> 1) & 7
    const int fsw = (lane & 15) >> 1;
    const int a_row = (wm * 64 + (lane & 15)) * 128;
    const int b_row = A_BYTES + (wn * 16 * TN + (lane & 15)) * 128;
    int koff[2];
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2) koff[s2] = 16 * ((4 * s2 + (lane >> 4)) ^ fsw);

    if (nsteps > 0) stage(0);
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();

    for (int it = 0; it < nsteps; ++it) {
        const int cur = it & 1;
        if (it + 1 < nsteps) stage(cur ^ 1);
        const unsigned char* sbuf = smem + cur * STAGE;
        // all operand reads of the K step are issued up front (the second half lands behind the first half's MFMAs)
        bf16x8_t a[2][4], b[2][TN];
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2) {
#pragma unroll
            for (int i = 0; i < 4; ++i)
                a[s2][i] = *reinterpret_cast<const bf16x8_t*>(sbuf + a_row + i * 16 * 128 + koff[s2]);
#pragma unroll
            for (int j = 0; j < TN; ++j)
                b[s2][j] = *reinterpret_cast<const bf16x8_t*>(sbuf + b_row + j * 16 * 128 + koff[s2]);
        }
        // weights as the MFMA's first operand: D rows = output channels (4 per lane), D columns = pixels
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(b[s2][j], a[s2][i], acc[i][j], 0, 0, 0);
        // the next tile has landed (this wave's part; the barrier extends it to all) and this one is read out
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
    }
    }

    // ---- epilogue: accumulators -> LDS [PR][BN + 4] fp32 -> whole 16-byte row segments ----
    // (two stages: all 128 rows at once; ring forms: the 64 rows of wave row `part` at a time, in front of the tables;
    //  phased form: the 128 rows of A half `part` at a time, every wave its quadrants of that half)
    constexpr int PARTS = PIPE ? WM : (PHASED ? 2 : 1), PR = BM / PARTS;
    constexpr int ELD = BN + 4;
    float* est = reinterpret_cast<float*>(smem);
    const bool partial = p.splitk > 1;
    const float alpha = (!partial && p.alpha) ? *p.alpha : 1.0f;
    constexpr int CPR = BN / 8;                     // 8-column chunks per row
    float* slab = partial ? p.slabs + (int64_t)zs * p.slab_stride : nullptr;
#pragma unroll
    for (int part = 0; part < PARTS; ++part) {
    if (part > 0) __syncthreads();                  // (the previous part is stored)
    if constexpr (PHASED) {
        constexpr int WNX = TN == 8 ? 4 : 2;
        const int wmx = w / WNX, wnx = w % WNX;
#pragma unroll
        for (int i = 0; i < XMI; ++i)
#pragma unroll
            for (int hj = 0; hj < 2 * XNJ; ++hj) {
                const int row = wmx * 16 * XMI + 16 * i + (lane & 15);
                const int col = (BN / 2) * (hj / XNJ) + wnx * 16 * XNJ + 16 * (hj % XNJ) + 4 * (lane >> 4);
                f32x4_t v = accx[part][i][hj / XNJ][hj % XNJ];
                v[0] *= alpha; v[1] *= alpha; v[2] *= alpha; v[3] *= alpha;
                *reinterpret_cast<f32x4_t*>(est + row * ELD + col) = v;
            }
    } else if (!PIPE || wm == part) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                const int row = (PIPE ? 0 : wm * 64) + 16 * i + (lane & 15);
                const int col = wn * 16 * TN + 16 * j + 4 * (lane >> 4);
                f32x4_t v = acc[i][j];
                v[0] *= alpha; v[1] *= alpha; v[2] *= alpha; v[3] *= alpha;
                *reinterpret_cast<f32x4_t*>(est + row * ELD + col) = v;
            }
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < (PR * CPR + NTHR - 1) / NTHR; ++q) {
        const int idx = t + NTHR * q;
        if ((PR * CPR) % NTHR != 0 && idx >= PR * CPR) continue;
        const int erow = idx / CPR, cc = idx - erow * CPR;
        const int row = part * PR + erow;
        const int m = m0 + row, col = n0 + cc * 8;
        if (m >= p.M || col >= p.N) continue;
        int64_t ooff;
        if (use_tabo) {
            const unsigned op = tabo[row];
            if (op == 0xffffffffu) continue;
            ooff = (int64_t)op * p.out_ld + col;
        } else if (p.d2s_c) {
            // depth-to-space store (image-major forward gathers only): this 16-byte segment lies inside one sub-pixel
            int b, ho, wo;
            if (p.pow2) {
                wo = m & (g.Wo - 1);
                const int t2 = m >> p.wq_shift;
                ho = t2 & (g.Ho - 1);
                b = t2 >> p.hq_shift;
            } else {
                const int t2 = m / g.Wo;
                wo = m - t2 * g.Wo;
                b = t2 / g.Ho;
                ho = t2 - b * g.Ho;
            }
            const int sub = col / p.d2s_c, c = col - sub * p.d2s_c;
            ooff = (((int64_t)b * (2 * g.Ho) + 2 * ho + (sub >> 1)) * (2 * g.Wo) + 2 * wo + (sub & 1)) * p.d2s_c + c;
        } else {
            ooff = (int64_t)m * p.out_ld + col;
        }
        f32x4_t v0 = *reinterpret_cast<const f32x4_t*>(est + erow * ELD + cc * 8);
        f32x4_t v1 = *reinterpret_cast<const f32x4_t*>(est + erow * ELD + cc * 8 + 4);
        if (partial) {
            *reinterpret_cast<f32x4_t*>(slab + ooff) = v0;
            *reinterpret_cast<f32x4_t*>(slab + ooff + 4) = v1;
            continue;
        }
        if (p.bias) {
            const f32x4_t b0 = *reinterpret_cast<const f32x4_t*>(p.bias + col);
            const f32x4_t b1 = *reinterpret_cast<const f32x4_t*>(p.bias + col + 4);
            v0 += b0;
            v1 += b1;
        }
        if (p.out_f32) {
            float* o = reinterpret_cast<float*>(p.out) + ooff;
            if (p.accumulate) {
                v0 += *reinterpret_cast<const f32x4_t*>(o);
                v1 += *reinterpret_cast<const f32x4_t*>(o + 4);
            }
            *reinterpret_cast<f32x4_t*>(o) = v0;
            *reinterpret_cast<f32x4_t*>(o + 4) = v1;
        } else {
            __bf16* o = reinterpret_cast<__bf16*>(p.out) + ooff;
            if (p.accumulate) {
                const uint4 r = *reinterpret_cast<const uint4*>(o);
                v0[0] += bf16_lo(r.x); v0[1] += bf16_hi(r.x); v0[2] += bf16_lo(r.y); v0[3] += bf16_hi(r.y);
                v1[0] += bf16_lo(r.z); v1[1] += bf16_hi(r.z); v1[2] += bf16_lo(r.w); v1[3] += bf16_hi(r.w);
            }
            uint4 r;
            r.x = pack_bf16x2(v0[0], v0[1]);
            r.y = pack_bf16x2(v0[2], v0[3]);
            r.z = pack_bf16x2(v1[0], v1[1]);
            r.w = pack_bf16x2(v1[2], v1[3]);
            *reinterpret_cast<uint4*>(o) = r;
        }
    }
    }
}

// out = alpha * sum_z slabs[z] (+ bias) (+ out), 8 elements per thread; n8 = elements / 8, N % 8 == 0
__global__ __launch_bounds__(256) void nn16_slab_reduce_kernel(const float* __restrict__ slabs, void* __restrict__ out,
                                                               const float* __restrict__ bias,
                                                               const float* __restrict__ alpha_dev, int64_t n8, int N,
                                                               int splitk, int64_t slab_stride, int accumulate,
                                                               int out_f32) {
    const float alpha = alpha_dev ? *alpha_dev : 1.0f;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n8; i += (int64_t)gridDim.x * 256) {
        f32x4_t s0 = {0.f, 0.f, 0.f, 0.f}, s1 = s0;
        for (int z = 0; z < splitk; ++z) {
            const float* sp = slabs + (int64_t)z * slab_stride + i * 8;
            s0 += *reinterpret_cast<const f32x4_t*>(sp);
            s1 += *reinterpret_cast<const f32x4_t*>(sp + 4);
        }
        s0 *= alpha;
        s1 *= alpha;
        if (bias) {
            const int col = (int)((i * 8) % N);
            s0 += *reinterpret_cast<const f32x4_t*>(bias + col);
            s1 += *reinterpret_cast<const f32x4_t*>(bias + col + 4);
        }
        if (out_f32) {
            float* o = reinterpret_cast<float*>(out) + i * 8;
            if (accumulate) {
                s0 += *reinterpret_cast<const f32x4_t*>(o);
                s1 += *reinterpret_cast<const f32x4_t*>(o + 4);
            }
            *reinterpret_cast<f32x4_t*>(o) = s0;
            *reinterpret_cast<f32x4_t*>(o + 4) = s1;
        } else {
            __bf16* o = reinterpret_cast<__bf16*>(out) + i * 8;
            if (accumulate) {
                const uint4 r = *reinterpret_cast<const uint4*>(o);
                s0[0] += bf16_lo(r.x); s0[1] += bf16_hi(r.x); s0[2] += bf16_lo(r.y); s0[3] += bf16_hi(r.y);
                s1[0] += bf16_lo(r.z); s1[1] += bf16_hi(r.z); s1[2] += bf16_lo(r.w); s1[3] += bf16_hi(r.w);
            }
            uint4 r;
            r.x = pack_bf16x2(s0[0], s0[1]);
            r.y = pack_bf16x2(s0[2], s0[3]);
            r.z = pack_bf16x2(s1[0], s1[1]);
            r.w = pack_bf16x2(s1[2], s1[3]);
            *reinterpret_cast<uint4*>(o) = r;
        }
    }
}

// ------------------------------------------------------------------------------------------
// NN kernel, halo-tile form: stride-1 window gathers (3 x 3 convolutions forward, 3 x 3 transposed convolutions in
// both directions, each stride phase of a 4 x 4 stride-2 transposed convolution = a 2 x 2 window on the input grid).
//   nn16_kernel re-reads the source pixels once per tap: on the C <= 192 layers (the high-resolution end of every
//   generator / discriminator, most of the FLOPs of the 256^2 / 512^2 models) it is bound by L2 -> LDS bandwidth on
//   that 9-fold im2col re-read (measured r02: ~7 TB/s of TCC traffic at 0.24 - 0.30 MFMA busy).  Here a block owns a
//   16 x 16 patch of output pixels of one image and a slice of BN output channels; per 64-channel chunk it loads the
//   (16 + NT - 1)^2 source pixels ONCE into LDS (128-byte pixel rows, 16-byte chunks XOR-swizzled by (pixel & 6): found by
//   brute force to be conflict-free for a 16-lane fragment starting at ANY pixel, i.e. for every tap shift), and the
//   NT^2 taps read their operands from that ONE halo buffer at shifted pixel indices while only the weight tile of each
//   (chunk, tap) step streams in through a ring of two slots: the tile of step s + 1 is issued behind the barrier of
//   step s, and every step opens with vmcnt(0) + barrier.  L2 -> LDS bytes per MAC: 0.0098 against 0.031.
//   8 waves = 4 (pixel rows) x 2 (channels), wave tile 64 pixels x 16 NF channels, v_mfma_f32_16x16x32_bf16.
//   LDS (halo | 2 weight slots) is sized in 1 KB wave-instructions, not in 8 KB rounds of the whole block: the waves whose
//   index lies beyond a tile's last round skip that DMA instruction (wave-uniform branch) instead of fetching the zero
//   page into padding - 41 instead of 48 instructions per halo tile at NT = 3 (37 / 40 at NT = 2), 4 NF instead of 8 or
//   16 per weight tile (12 / 16 at NF = 3, 4 / 8 at NF = 1).  Every destination stays 1 KB aligned; 45 - 73 KB per block,
//   two blocks per CU.
//   Measured and rejected (profiles/halo_ring_ab.txt): a THREE-slot ring in this layout (41 + 3 x 12 = 77 KB at NF = 3:
//   it fits beside a second block), weight tile s + 2 issued behind the barrier of step s, counted vmcnt per wave in
//   front of each barrier so that the newest tile stays in flight across it and across the halo reload.  Bit-identical;
//   per layer within +- 1 % of the two-slot instantiation of the same kernel on every halo shape of config 3 (2.5 %
//   SLOWER on 96 -> 96 at 128^2 and 384 -> 192 at 32^2 k4s2): the second co-resident block already covers a block's weight
//   latency, a deeper ring per block adds nothing.
// ------------------------------------------------------------------------------------------
constexpr int NH_T = 16;                                   // patch edge
constexpr int NH_LDS_MAX = 81920;                          // two blocks per CU
template <int NT> struct NHGeom {
    static constexpr int HW = NH_T + NT - 1;               // halo edge
    static constexpr int NPIX = HW * HW;
    static constexpr int A_ROUNDS = (NPIX * 8 + 63) / 64;  // LDS-DMA wave-instructions (1 KB = 8 pixel rows) per chunk
    static constexpr int A_INSTR = (A_ROUNDS + 7) / 8;     // ... per wave at most (wave w issues rounds w, w + 8, ...)
    static constexpr int A_BYTES = A_ROUNDS * 1024;
};
constexpr int nh_w_rounds(int NF) { return 32 * NF * 8 / 64; }          // wave-instructions per weight tile [32 NF][64]
constexpr int nh_w_instr(int NF) { return (nh_w_rounds(NF) + 7) / 8; }
// Two blocks per CU: ONE halo buffer and a 2-tile weight ring.  A block alone on its CU (two halo
// buffers, 3- or 4-tile ring, 147 - 160 KB) was measured 10 - 20 % slower than nn16_kernel: nothing runs while it computes
// its per-lane halo addresses, waits for its first 77 KB or stores its epilogue (~7 of 21 us per block at C = 96).
constexpr int NH_WS = 2;
template <int NT, int NF> constexpr int nn16h_lds_bytes() {
    const int ring = NHGeom<NT>::A_BYTES + NH_WS * nh_w_rounds(NF) * 1024;
    const int epi = 128 * (32 * NF + 4) * 4;               // the epilogue goes through LDS in two halves of 128 pixels
    return ring > epi ? ring : epi;
}

// Epilogue of the halo-tile kernels (both forms): accumulators -> LDS [128][BN + 4] fp32 (two halves of the patch) ->
// 16-byte row segments.
// p.stats_part (batch-norm statistics of the OUTPUT, fused: ops.py:630 tf.nn.moments of the tensor this launch writes):
// every stored value, as rounded to its stored type, is written back into the staging tile; the block then reduces the
// tile's columns to one row of per-channel partial sums [sum | sum of squares] - summed over blocks in a fixed order by
// bn_partial_finalize, no atomics.
struct NHTile {                     // which patch / column tile / phase a block owns
    int b, y0, x0, n0, ph, pw, phase, nph, tx, ty, tiles_x, tiles_y;
};
template <int NF, int THIN>
__device__ __forceinline__ void nn16h_epilogue(const NN16Params& p, const NHTile& tl, f32x4_t (&acc)[4][NF],
                                               unsigned char* smem) {
    constexpr int BN = 32 * NF;
    const Gather& g = p.g;
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int wm = w >> 1, wn = w & 1;
    const int px = lane & 15, kb = lane >> 4;
    const int b = tl.b, y0 = tl.y0, x0 = tl.x0, n0 = tl.n0, ph = tl.ph, pw = tl.pw, phase = tl.phase, nph = tl.nph;
    const int tx = tl.tx, ty = tl.ty, tiles_x = tl.tiles_x, tiles_y = tl.tiles_y;
    constexpr int ELD = BN + 4;
    float* est = reinterpret_cast<float*>(smem);
    const float alpha = p.alpha ? *p.alpha : 1.0f;
    constexpr int CPR = BN / 8;
    constexpr int RG = 512 / BN;                        // row groups of the column reduction (threads RG * BN .. 511 idle)
    for (int half = 0; half < 2; ++half) {
        if ((wm >> 1) == half) {                        // waves of pixel rows 8 half .. 8 half + 7
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < NF; ++j) {
                    const int row = ((wm & 1) * 4 + i) * 16 + px;
                    const int col = wn * 16 * NF + 16 * j + 4 * kb;
                    f32x4_t v = acc[i][j];
                    v[0] *= alpha; v[1] *= alpha; v[2] *= alpha; v[3] *= alpha;
                    *reinterpret_cast<f32x4_t*>(est + row * ELD + col) = v;
                }
        }
        __syncthreads();
        for (int idx = t; idx < 128 * CPR; idx += 512) {
            const int row = idx / CPR, cc = idx - row * CPR;
            const int gy = y0 + 8 * half + (row >> 4), gx = x0 + (row & 15);
            const int col = THIN == 1 ? 0 : n0 + cc * 8;
            const int oy = THIN == 1 ? 2 * gy + (cc >> 1) : gy * g.pstep + ph;
            const int ox = THIN == 1 ? 2 * gx + (cc & 1) : gx * g.pstep + pw;
            f32x4_t v0 = *reinterpret_cast<const f32x4_t*>(est + row * ELD + cc * 8);
            f32x4_t v1 = *reinterpret_cast<const f32x4_t*>(est + row * ELD + cc * 8 + 4);
            const bool live = gy < g.Hq && gx < g.Wq && col < p.N && oy < g.Ho && ox < g.Wo;
            if (live) {
                int64_t ooff = ((int64_t)(b * g.Ho + oy) * g.Wo + ox) * p.out_ld + col;
                if (THIN == 0 && p.d2s_c) {             // depth-to-space store: the segment lies inside one sub-pixel
                    const int sub = col / p.d2s_c, c = col - sub * p.d2s_c;
                    ooff = (((int64_t)b * (2 * g.Ho) + 2 * oy + (sub >> 1)) * (2 * g.Wo) + 2 * ox + (sub & 1)) * p.d2s_c + c;
                }
                if (p.bias) {
                    v0 += *reinterpret_cast<const f32x4_t*>(p.bias + col);
                    v1 += *reinterpret_cast<const f32x4_t*>(p.bias + col + 4);
                }
                if (p.out_f32) {
                    float* o = reinterpret_cast<float*>(p.out) + ooff;
                    if (p.accumulate) {
                        v0 += *reinterpret_cast<const f32x4_t*>(o);
                        v1 += *reinterpret_cast<const f32x4_t*>(o + 4);
                    }
                    *reinterpret_cast<f32x4_t*>(o) = v0;
                    *reinterpret_cast<f32x4_t*>(o + 4) = v1;
                } else {
                    __bf16* o = reinterpret_cast<__bf16*>(p.out) + ooff;
                    if (p.accumulate) {
                        const uint4 rr = *reinterpret_cast<const uint4*>(o);
                        v0[0] += bf16_lo(rr.x); v0[1] += bf16_hi(rr.x); v0[2] += bf16_lo(rr.y); v0[3] += bf16_hi(rr.y);
                        v1[0] += bf16_lo(rr.z); v1[1] += bf16_hi(rr.z); v1[2] += bf16_lo(rr.w); v1[3] += bf16_hi(rr.w);
                    }
                    uint4 rr;
                    rr.x = pack_bf16x2(v0[0], v0[1]);
                    rr.y = pack_bf16x2(v0[2], v0[3]);
                    rr.z = pack_bf16x2(v1[0], v1[1]);
                    rr.w = pack_bf16x2(v1[2], v1[3]);
                    *reinterpret_cast<uint4*>(o) = rr;
                    if (p.stats_part) {                 // the values as stored
                        v0[0] = bf16_lo(rr.x); v0[1] = bf16_hi(rr.x); v0[2] = bf16_lo(rr.y); v0[3] = bf16_hi(rr.y);
                        v1[0] = bf16_lo(rr.z); v1[1] = bf16_hi(rr.z); v1[2] = bf16_lo(rr.w); v1[3] = bf16_hi(rr.w);
                    }
                }
            } else if (p.stats_part) {
                v0 = f32x4_t{0.f, 0.f, 0.f, 0.f};
                v1 = v0;
            }
            if (p.stats_part) {
                *reinterpret_cast<f32x4_t*>(est + row * ELD + cc * 8) = v0;
                *reinterpret_cast<f32x4_t*>(est + row * ELD + cc * 8 + 4) = v1;
            }
        }
        __syncthreads();
        if (p.stats_part) {                             // (block-uniform)
            // column sums of this half's 128 stored rows -> partial row 2 * block + half
            float st_s = 0.f, st_q = 0.f;
            if (t < RG * BN) {
                const int colr = t % BN;
                for (int row = t / BN; row < 128; row += RG) {
                    const float v = est[row * ELD + colr];
                    st_s += v;
                    st_q = fmaf(v, v, st_q);
                }
            }
            __syncthreads();                            // every read of the tile is done: reuse its first rows
            if (t < RG * BN) {
                est[t] = st_s;
                est[RG * BN + t] = st_q;
            }
            __syncthreads();
            if (t < BN && n0 + t < p.N) {
                float s = 0.f, q = 0.f;
#pragma unroll
                for (int r2 = 0; r2 < RG; ++r2) {
                    s += est[r2 * BN + t];
                    q += est[RG * BN + r2 * BN + t];
                }
                const int64_t prow = 2 * ((((int64_t)b * tiles_y + ty) * tiles_x + tx) * nph + phase) + half;
                p.stats_part[prow * (2 * (int64_t)p.N) + n0 + t] = s;
                p.stats_part[prow * (2 * (int64_t)p.N) + p.N + n0 + t] = q;
            }
            __syncthreads();                            // (the next half overwrites the tile)
        }
    }
}

// THIN = 1 (r03): the input gradient of a 3 x 3 stride-2 (pad 1) convolution whose INPUT has 8 channels (the image layers of
// the discriminator) as ONE stride-1 2 x 2-window launch: the 2 x 2 output pixels (2 y + py, 2 x + px) of source pixel
// window (y .. y + 1, x .. x + 1) are the 4 x 8 = 32 output columns of a tile (tap k = p + 1 - 2 w per axis, a zero weight
// tile where that falls outside 0 .. 2), stored depth-to-space.  The four stride phases of the generic path each walked
// their own taps over 32 padded columns: 0.63 ms per call at 46 TF/s for 170 MB of tensors.
template <int NT, int NF, int MODE, int THIN = 0>
__global__ __launch_bounds__(512, 4) void nn16h_kernel(const NN16Params p) {       // 4 waves per SIMD: <= 128 VGPRs
    using G = NHGeom<NT>;
    constexpr int WW = G::HW, NPIX = G::NPIX, A_ROUNDS = G::A_ROUNDS, A_INSTR = G::A_INSTR, A_BYTES = G::A_BYTES;
    constexpr int BN = 32 * NF, W_ROUNDS = nh_w_rounds(NF), W_INSTR = nh_w_instr(NF), W_BYTES = W_ROUNDS * 1024;
    constexpr int NTAPS = NT * NT;
    static_assert(NH_WS == 2, "the step loop below alternates between two slots");
    static_assert(nn16h_lds_bytes<NT, NF>() <= NH_LDS_MAX, "two blocks per CU");
    static_assert(128 * (BN + 4) * 4 <= nn16h_lds_bytes<NT, NF>(), "the epilogue's staging tile overlays the ring");
    static_assert(A_BYTES % 1024 == 0 && W_BYTES % 1024 == 0, "every LDS-DMA destination is 1 KB aligned");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];   // halo tile | W ring (NH_WS tiles)

    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int wu = __builtin_amdgcn_readfirstlane(w);   // (scalar: the branches on it below are wave-uniform by construction)
    const int wm = w >> 1, wn = w & 1;
    const Gather& g = p.g;

    // ---- which patch ----
    const int nph = g.pstep * g.pstep;
    const int tiles_x = (g.Wq + NH_T - 1) / NH_T, tiles_y = (g.Hq + NH_T - 1) / NH_T;
    const int nt = (p.N + BN - 1) / BN;
    int r = xcd_remap(blockIdx.x, gridDim.x);
    int phase, tile_n, tx, ty, b;
    if (p.mfast) {              // patches fastest: one (phase, N-column) weight slab stays in the XCD's L2 (see nn16_kernel)
        tx = r % tiles_x; r /= tiles_x;
        ty = r % tiles_y; r /= tiles_y;
        b = r % g.Nb; r /= g.Nb;
        phase = r % nph;
        tile_n = r / nph;
    } else {
        phase = r % nph; r /= nph;
        tile_n = r % nt; r /= nt;
        tx = r % tiles_x; r /= tiles_x;
        ty = r % tiles_y;
        b = r / tiles_y;
    }
    const int y0 = ty * NH_T, x0 = tx * NH_T, n0 = tile_n * BN;
    int ph = 0, pw = 0;
    if (MODE == GATHER_TCONV && g.pstep > 1) {
        ph = g.pstep - 1 - phase / g.pstep;
        pw = g.pstep - 1 - phase % g.pstep;
    }
    // window geometry per axis: halo index hi in [0, NT) <-> weight tap, source = q + base + hi
    //   CONV  (stride 1): source = q + kh - pad                    -> base = -pad,            tap(hi) = hi
    //   TCONV (stride 1): source = q + pad - kh                    -> base = pad - (NT - 1),  tap(hi) = NT - 1 - hi
    //   TCONV phase     : kh = kh0 + 2 i, source = q + d - i       -> base = d - (NT - 1),    tap(hi) = kh0 + 2 (NT - 1 - hi)
    int base_h, base_w, kh0 = 0, kw0 = 0, kstep = 1;
    if (MODE == GATHER_CONV) {
        base_h = base_w = -g.pad;
    } else if (g.pstep > 1) {
        kstep = g.stride;
        kh0 = (ph + g.pad) % g.stride;
        kw0 = (pw + g.pad) % g.stride;
        base_h = (ph + g.pad - kh0) / g.stride - (NT - 1);
        base_w = (pw + g.pad - kw0) / g.stride - (NT - 1);
    } else {
        base_h = base_w = g.pad - (NT - 1);
    }
    // taps this block walks: all NT x NT, except in the stride phases of a kernel with k < NT * stride (3 x 3 stride 2, r03:
    // 1 / 2 / 2 / 4 taps) - there only the window rows / columns hy >= NT - nkh (hx >= NT - nkw) carry a tap
    int nkh = NT, nkw = NT;
    if (MODE == GATHER_TCONV && NT == 2 && g.pstep > 1) {
        nkh = (g.k - kh0 + kstep - 1) / kstep;
        nkw = (g.k - kw0 + kstep - 1) / kstep;
    }
    const int ntaps = (MODE == GATHER_TCONV && NT == 2) ? nkh * nkw : NTAPS;

    const unsigned char* abase = reinterpret_cast<const unsigned char*>(p.A);
    const unsigned char* bbase = reinterpret_cast<const unsigned char*>(p.B);
    const unsigned char* zero = reinterpret_cast<const unsigned char*>(g_zero_page);
    const uint32_t lds0 = static_cast<uint32_t>(
        reinterpret_cast<uintptr_t>((__attribute__((address_space(3))) unsigned char*)smem));
    const uint32_t ldsw = lds0 + A_BYTES;

    // ---- per-lane sources of the halo tile (fixed for the whole block) ----
    // byte offset of this lane's 8 channels inside a 64-channel chunk: pixel 8 (8 i + w) + (lane >> 3), chunk (lane & 7)
    // swizzled by (pixel & 6) - the same for every instruction i (one register, not A_INSTR)
    const int acb = 16 * ((lane & 7) ^ ((lane >> 3) & 6));
    const unsigned char* asrc[A_INSTR];
#pragma unroll
    for (int i = 0; i < A_INSTR; ++i) {
        const int pp = (i * 8 + w) * 64 + lane;
        const int q = pp >> 3;
        const int hy = q / WW, hx = q - hy * WW;
        int sy = y0 + hy + base_h, sx = x0 + hx + base_w;
        bool ok = q < NPIX;
        if (MODE == GATHER_CONV && g.reflect) {
            sy = sy < 0 ? -sy : sy;
            sy = sy >= g.Hs ? 2 * (g.Hs - 1) - sy : sy;
            sx = sx < 0 ? -sx : sx;
            sx = sx >= g.Ws ? 2 * (g.Ws - 1) - sx : sx;
        }
        ok = ok && sy >= 0 && sy < g.Hs && sx >= 0 && sx < g.Ws;
        asrc[i] = ok ? abase + 2 * ((int64_t)((b * g.Hs + sy) * g.Ws + sx) * g.ld) : zero;
    }
    // (weight row n = 8 (8 i + w) + (lane >> 3): its swizzle (n >> 1) & 7 = 4 (w & 1) + (lane >> 4) does not depend on i)
    const int wcb = 16 * ((lane & 7) ^ (4 * (w & 1) + (lane >> 4)));
    const unsigned char* wsrc[W_INSTR];
    bool wok[W_INSTR];
    int wrow[W_INSTR];
#pragma unroll
    for (int i = 0; i < W_INSTR; ++i) {
        const int pp = (i * 8 + w) * 64 + lane;
        const int n = pp >> 3;
        wok[i] = n < BN && n0 + n < p.N;
        wrow[i] = n;
        wsrc[i] = bbase + 2 * ((int64_t)(THIN == 1 ? (n & 7) : n0 + n) * p.C);      // THIN 1: column = (py, px, channel)
    }
    const uint32_t dma_a = __builtin_amdgcn_readfirstlane(lds0 + w * 1024);
    const uint32_t dma_w = __builtin_amdgcn_readfirstlane(ldsw + w * 1024);

    // Round r = 8 i + (wave index) of a tile is one instruction of one wave (1 KB); the waves beyond the tile's last round
    // skip instruction i as a whole (EXEC stays full in the issued ones: surplus lanes of the last halo round fetch the
    // zero page into the padding behind pixel NPIX - 1).
    auto issue_a = [&](int chunk) {                     // the (NT + 15)^2 source pixels of 64 channels
        const uint32_t dst = dma_a;
        const int cb = chunk * 128;
        const bool cv = (cb + acb) < 2 * p.C;
#pragma unroll
        for (int i = 0; i < A_INSTR; ++i) {
            if (8 * (i + 1) > A_ROUNDS && 8 * i + wu >= A_ROUNDS) continue;
            glds16_asm(cv ? asrc[i] + (cb + acb) : zero, dst + i * 8192);
        }
    };
    // weight tile [BN][64 channels] of chunk `chunk` and tap (ty_, tx_) of the nkh x nkw taps this block walks
    auto issue_w = [&](int chunk, int ty_, int tx_, int slot) {
        const int hy = NT - nkh + ty_, hx = NT - nkw + tx_;
        const int kh = MODE == GATHER_CONV ? hy : kh0 + kstep * (NT - 1 - hy);
        const int kw = MODE == GATHER_CONV ? hx : kw0 + kstep * (NT - 1 - hx);
        const int64_t toff = 2 * ((int64_t)(kh * g.k + kw) * p.tap_stride);
        const uint32_t dst = dma_w + slot * W_BYTES;
        const int cb = chunk * 128;
#pragma unroll
        for (int i = 0; i < W_INSTR; ++i) {
            if (8 * (i + 1) > W_ROUNDS && 8 * i + wu >= W_ROUNDS) continue;
            bool cv = wok[i] && (cb + wcb) < 2 * p.C;
            int64_t to = toff;
            if (THIN == 1) {                            // window position (hy, hx), output parity (py, px) -> tap
                const int kty = ((wrow[i] >> 4) & 1) + 1 - 2 * hy, ktx = ((wrow[i] >> 3) & 1) + 1 - 2 * hx;
                cv = cv && kty >= 0 && ktx >= 0;
                to = 2 * ((int64_t)(kty * 3 + ktx) * p.tap_stride);
            }
            glds16_asm(cv ? wsrc[i] + to + (cb + wcb) : zero, dst + i * 8192);
        }
    };

    // ---- operand addresses ----
    const int px = lane & 15, kb = lane >> 4;
    int qb[4];                                          // halo pixel of this lane's output pixel at tap (0, 0)
#pragma unroll
    for (int i = 0; i < 4; ++i) qb[i] = (wm * 4 + i) * WW + px;
    uint32_t boff[NF];
#pragma unroll
    for (int j = 0; j < NF; ++j) {
        const int n = wn * 16 * NF + 16 * j + px;
        boff[j] = A_BYTES + n * 128 + 16 * (kb ^ ((n >> 1) & 7));          // (byte offset into smem)
    }

    f32x4_t acc[4][NF];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < NF; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[i][j][e] = 0.f;

    const int nchunks = (p.C + 63) >> 6;
    const int T = nchunks * ntaps;
    // Cursors over the (chunk, tap) steps - the step that computes and the next weight tile to issue, one step in front -
    // instead of a division by the (run-time) tap counts per step.
    // DMA order per wave: W(0), halo(0) | W(s + 1) behind the barrier of step s | and at a chunk's last tap, whose
    // successor needs the ONE halo buffer this step still reads: compute, barrier, halo(next chunk), W(s + 1).
    int c_chunk = 0, c_ty = 0, c_tx = 0;
    int w_chunk = 0, w_ty = 0, w_tx = 0, w_step = 0;
    auto issue_next_w = [&](int slot) {
        if (w_step < T) {
            issue_w(w_chunk, w_ty, w_tx, slot);
            ++w_step;
            if (++w_tx == nkw) {
                w_tx = 0;
                if (++w_ty == nkh) {
                    w_ty = 0;
                    ++w_chunk;
                }
            }
        }
    };
    issue_next_w(0);
    issue_a(0);

    // one (chunk, tap) step on ring slot SLOT (a compile-time constant: the operand addresses are base + immediate)
    auto hstep = [&](int step, auto slot_c) {
        constexpr int SLOT = decltype(slot_c)::value;
        constexpr int NEXT = SLOT ^ 1;                  // the slot step - 1 read
        // W(step) (and at a chunk's first tap its halo tile, issued in front of it) has landed - this wave's part; the
        // barrier extends that to every wave: nothing else is in flight
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        // the next step starts a chunk: its halo tile goes into the ONE buffer this step still reads - so this step
        // computes first and issues after a barrier of its own
        const bool reload = c_ty == nkh - 1 && c_tx == nkw - 1 && step + 1 < T;
        if (!reload) issue_next_w(NEXT);

        const int hy = NT - nkh + c_ty, hx = NT - nkw + c_tx;
        constexpr uint32_t wslot = (uint32_t)SLOT * W_BYTES;
        const int tq = hy * WW + hx;
        const int ksteps = (p.C - c_chunk * 64) >= 64 ? 2 : 1;         // 32-channel MFMA steps in this chunk
        uint32_t aaddr[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int q = qb[i] + tq;
            aaddr[i] = q * 128 + 16 * (kb ^ (q & 6));
        }
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2) {
            if (s2 < ksteps) {                          // (one 32-channel half at a time: 128 VGPRs at 4 waves per SIMD)
                bf16x8_t a[4], bw[NF];
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    a[i] = *reinterpret_cast<const bf16x8_t*>(smem + (aaddr[i] ^ (s2 ? 64u : 0u)));
#pragma unroll
                for (int j = 0; j < NF; ++j)
                    bw[j] = *reinterpret_cast<const bf16x8_t*>(smem + ((boff[j] ^ (s2 ? 64u : 0u)) + wslot));
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < NF; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bw[j], a[i], acc[i][j], 0, 0, 0);
            }
        }
        if (reload) {
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");       // every wave has read the halo tile of this chunk
            __builtin_amdgcn_s_barrier();
            issue_a(c_chunk + 1);
            issue_next_w(NEXT);
        }
        if (++c_tx == nkw) {
            c_tx = 0;
            if (++c_ty == nkh) {
                c_ty = 0;
                ++c_chunk;
            }
        }
    };
    for (int step = 0; step < T; step += NH_WS) {
        hstep(step, std::integral_constant<int, 0>());
        if (step + 1 < T) hstep(step + 1, std::integral_constant<int, 1>());
    }
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();

    NHTile tl;
    tl.b = b; tl.y0 = y0; tl.x0 = x0; tl.n0 = n0; tl.ph = ph; tl.pw = pw; tl.phase = phase; tl.nph = nph;
    tl.tx = tx; tl.ty = ty; tl.tiles_x = tiles_x; tl.tiles_y = tiles_y;
    nn16h_epilogue<NF, THIN>(p, tl, acc, smem);
}

// ------------------------------------------------------------------------------------------
// Measured and rejected (r03): a second form of the halo kernel - 32-channel chunks (64-byte pixel rows), TWO halo buffers so
// that the next chunk streams in during the current one, two K items per step with their weight tiles issued two steps
// ahead through a 3-slot ring, counted waits (s_waitcnt vmcnt(issued - needed) per wave, nothing drained), 74 - 78 KB of LDS.
// Bit-identical results, config 3 at batch 256: 101.6 -> 106.9 ms per iteration; transposed conv 192 -> 96 at 128^2:
// 3.1 -> 4.4 ms.  A block computes a 32-channel chunk of a 2 x 2 window in ~0.6 us and a halo tile takes ~2 us to arrive: one
// chunk of look-ahead hides less than the single 64-channel buffer of the first form loses, and the 64-byte rows halve the
// coalescing of the DMA's global reads.  (Three WEIGHT tiles in flight per block beside the one 64-channel halo buffer do
// fit two blocks per CU and were measured as well - no gain, see the kernel's header.)  (The 64-byte-row swizzle that is
// conflict-free for ds_read_b128's lane groups, should it be needed again: chunk c of row r at c ^ ((r >> 1) & 2).)
// ------------------------------------------------------------------------------------------
// TN kernel (weight gradients): K = pixels, both operands pixel-major in LDS, transposed operand reads
// ------------------------------------------------------------------------------------------
constexpr int TN16_BK = 64;
constexpr int TN16_TILE = TN16_BK * 256;            // bytes of one [64 pixels][128 channels] bf16 image

__device__ __forceinline__ s16x4v lds_tr16(uint32_t lds_byte_addr) {
    return __builtin_amdgcn_ds_read_tr16_b64_v4i16(reinterpret_cast<lds_s16x4v*>(lds_byte_addr));
}
__device__ __forceinline__ int tr16_swz(int row, int chunk) {
    return 256 * row + 16 * (chunk ^ (((row & 3) << 2) | ((row >> 2) & 3)));
}

template <int MODE>
__global__ __launch_bounds__(256, 2) void tn16_kernel(const TN16Params p) {
    constexpr int BM = 128, BN = 128;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];   // [2][A image | B image]

    const int t = threadIdx.x;
    const int lane = t & 63, w = t >> 6;
    const int wm = w >> 1, wn = w & 1;
    const Gather& g = p.g;

    // split-major logical order inside each XCD: the (M, N) tiles of one pixel range run together on ONE XCD, so the
    // x / dy rows of that range are fetched into that L2 once and shared (the kernel is otherwise bound by L2 misses:
    // every tile streams the whole pixel range)
    const int ntile = p.tiles_m * p.tiles_n;
    const int lin = xcd_remap(blockIdx.x, ntile * p.splitk);
    const int zs = lin / ntile;
    const int tile = lin - zs * ntile;
    const int tile_n = tile % p.tiles_n, tile_m = tile / p.tiles_n;
    const int mf0 = tile_m * BM, cb0 = tile_n * BN;
    const int row_begin = zs * p.rows_per_split;
    const int row_end = min(p.M, row_begin + p.rows_per_split);
    const int nsteps = max(0, (row_end - row_begin + TN16_BK - 1) / TN16_BK);

    // staging role: pixel rows 16 j + 4 w + prow of the K tile, channel chunk `ch` (fixed: the swizzle of those rows
    // depends on prow and w only)
    const int prow = lane >> 4;
    const int ch = (lane & 15) ^ ((prow << 2) | w);
    const int mf = mf0 + 8 * ch;
    int a_kh = 0, a_kw = 0, a_c = mf;
    if (MODE != GATHER_PLAIN) {
        const int tap = mf / p.Ca;
        a_c = mf - tap * p.Ca;
        a_kh = tap / g.k;
        a_kw = tap - a_kh * g.k;
    }
    const bool a_ok = mf < p.Mf;
    const int cb = cb0 + 8 * ch;
    const bool b_ok = cb < p.Cb;
    const __bf16* Ab = reinterpret_cast<const __bf16*>(p.A);
    const __bf16* Bb = reinterpret_cast<const __bf16*>(p.Bv);
    const void* zero = reinterpret_cast<const void*>(g_zero_page);
    int m_next = row_begin + 4 * w + prow;          // pixel of instruction j = 0 of the next K tile

    auto stage = [&](int buf) {
        unsigned char* sa = smem + buf * (2 * TN16_TILE) + (4 * w) * 256;
        unsigned char* sb = sa + TN16_TILE;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int m = m_next + 16 * j;
            const void* srca = zero;
            const void* srcb = zero;
            if (m < row_end) {
                if (a_ok) {
                    int64_t pix;
                    if (MODE == GATHER_PLAIN) {
                        pix = m;
                    } else {
                        int b, ho, wo;
                        if (p.pow2) {
                            wo = m & (g.Wq - 1);
                            const int r = m >> p.wq_shift;
                            ho = r & (g.Hq - 1);
                            b = r >> p.hq_shift;
                        } else {
                            wo = m % g.Wq;
                            const int r = m / g.Wq;
                            ho = r % g.Hq;
                            b = r / g.Hq;
                        }
                        const int hs = conv_src(ho, a_kh, g.stride, g.pad, g.reflect, g.Hs);
                        const int ws = conv_src(wo, a_kw, g.stride, g.pad, g.reflect, g.Ws);
                        pix = (hs >= 0 && ws >= 0) ? ((int64_t)b * g.Hs + hs) * g.Ws + ws : -1;
                    }
                    if (pix >= 0) srca = Ab + pix * g.ld + a_c;
                }
                if (b_ok) srcb = Bb + (int64_t)m * p.b_ld + cb;
            }
            glds16(srca, sa + j * 16 * 256);
            glds16(srcb, sb + j * 16 * 256);
        }
        m_next += TN16_BK;
    };

    f32x16_t acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    // transposed-read addresses (buffer 0, k-step 0): lane -> k block lane >> 5, 16-channel group (lane >> 4) & 1,
    // block row q = (lane & 15) >> 2, column quad pq = lane & 3; read jj covers pixels 8 kblk + 4 jj .. + 3
    const int kblk = lane >> 5, g16 = (lane >> 4) & 1, q = (lane & 15) >> 2, pq = lane & 3;
    const uint32_t lds0 = static_cast<uint32_t>(
        reinterpret_cast<uintptr_t>((__attribute__((address_space(3))) unsigned char*)smem));
    uint32_t a_ad[2][2], b_ad[2][2];
#pragma unroll
    for (int jj = 0; jj < 2; ++jj) {
        const int row = 8 * kblk + 4 * jj + q;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            a_ad[i][jj] = lds0 + tr16_swz(row, 4 * (wm * 2 + i) + 2 * g16 + (pq >> 1)) + 8 * (pq & 1);
            b_ad[i][jj] = lds0 + TN16_TILE + tr16_swz(row, 4 * (wn * 2 + i) + 2 * g16 + (pq >> 1)) + 8 * (pq & 1);
        }
    }
    auto operand = [&](uint32_t lo_addr, uint32_t hi_addr) {
        const s16x4v lo = lds_tr16(lo_addr), hi = lds_tr16(hi_addr);
        const s16x8v v = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
        return __builtin_bit_cast(bf16x8_t, v);
    };

    if (nsteps > 0) stage(0);
    __syncthreads();
    for (int it = 0; it < nsteps; ++it) {
        const int cur = it & 1;
        if (it + 1 < nsteps) stage(cur ^ 1);
        const uint32_t bufoff = (uint32_t)cur * (2u * TN16_TILE);
#pragma unroll
        for (int s = 0; s < TN16_BK / 16; ++s) {
            bf16x8_t a[2], b[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) a[i] = operand(a_ad[i][0] + bufoff + 4096 * s, a_ad[i][1] + bufoff + 4096 * s);
#pragma unroll
            for (int j = 0; j < 2; ++j) b[j] = operand(b_ad[j][0] + bufoff + 4096 * s, b_ad[j][1] + bufoff + 4096 * s);
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[i], b[j], acc[i][j], 0, 0, 0);
        }
        __syncthreads();
    }

    float* obase = p.out + (int64_t)zs * p.slab_stride;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = mf0 + wm * 64 + 32 * i + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
            if (row >= p.Mf) continue;
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int col = cb0 + wn * 64 + 32 * j + (lane & 31);
                if (col < p.Cb) obase[(int64_t)row * p.out_ld + col] = acc[i][j][r];
            }
        }
    }
}


// ------------------------------------------------------------------------------------------
// TN kernel, wide form: 256 x 128 tile, 8 waves, 3-stage LDS ring with counted vmcnt.
//   The 128 x 128 kernel above keeps one 32 KB tile in flight per block (64 KB per CU) and moves 64 FLOP per loaded
//   byte; measured (PMC, r02): 47 % of its wave cycles parked in s_waitcnt / barrier, MFMA busy 22 %, L2 -> LDS traffic
//   6.9 TB/s - throughput = bytes in flight x FLOP per byte / latency.  Here a tile is 48 KB for 1.5x the FLOPs per byte
//   (87), two tiles (96 KB) are in flight behind the one being computed, and the barrier no longer drains the queue:
//   tile t + 2 is issued right after the barrier of iteration t, the wait before that barrier leaves tile t + 1 in
//   flight (s_waitcnt vmcnt(6): 6 LDS-DMA instructions per wave and tile).  One block per CU (144 KB of LDS).
// ------------------------------------------------------------------------------------------
// BK = 32 pixels per stage: a stage is 24 KB, the ring 72 KB, and TWO blocks share a CU (the halo-tile NN kernel's lesson: an
// 8-wave block alone on its CU leaves the matrix pipe idle at every barrier and in its epilogue); BK = 64 is the first form
// (one block per CU, 144 KB), kept for A/B (BG_TN16X_BK=64).
// NBI = 2 (r03): TWO B images, a 256 x 256 output tile, wave tile 64 x 128.  The 256 x 128 form moves 87 FLOP per byte
// from L2 into LDS and reads 64 B of LDS per lane for 4 MFMAs - on the C >= 768 layers (tiny maps, everything comes from
// L2) it sat at the L2 -> LDS limit (~8 TB/s) with the LDS pipe as busy as the matrix pipe; the wider tile is 131 FLOP per
// byte and 96 B per 8 MFMAs.  96 KB of ring: one block per CU, 2 waves per SIMD, 256 VGPRs each.
template <int MODE, int BK, int NBI = 1>
__global__ __launch_bounds__(512, (BK == 32 && NBI == 1) ? 4 : 2) void tn16x_kernel(const TN16Params p) {
    constexpr int TILE = BK * 256;                      // bytes of one [BK pixels][128 channels] bf16 image
    constexpr int TNX_STAGE = (2 + NBI) * TILE;         // A image 0 | A image 1 | B image(s)
    constexpr int NJ = BK / 16;                         // LDS-DMA instructions per wave and A image
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];   // 3 stages

    const int t = threadIdx.x;
    const int lane = t & 63, w = t >> 6;
    const int wm = w >> 1, wn = w & 1;
    const Gather& g = p.g;

    const int ntile = p.tiles_m * p.tiles_n;
    const int lin = xcd_remap(blockIdx.x, ntile * p.splitk);
    const int zs = lin / ntile;
    const int tile = lin - zs * ntile;
    const int tile_n = tile % p.tiles_n, tile_m = tile / p.tiles_n;
    const int mf0 = tile_m * 256, cb0 = tile_n * 128 * NBI;
    const int row_begin = zs * p.rows_per_split;
    const int row_end = min(p.M, row_begin + p.rows_per_split);
    const int nsteps = max(0, (row_end - row_begin + BK - 1) / BK);

    // staging role: A image (w >> 2), pixel rows 16 j + 4 (w & 3) + prow (j < BK / 16), channel chunk `ch` of that image;
    // B: the same rows for the j's of half (w >> 2)
    const int prow = lane >> 4;
    const int wq = w & 3, ia = w >> 2;
    const int ch = (lane & 15) ^ ((prow << 2) | wq);
    const int mf = mf0 + 128 * ia + 8 * ch;
    int a_kh = 0, a_kw = 0, a_c = mf;
    if (MODE != GATHER_PLAIN) {
        const int tap = mf / p.Ca;
        a_c = mf - tap * p.Ca;
        a_kh = tap / g.k;
        a_kw = tap - a_kh * g.k;
    }
    const int cb = cb0 + (NBI == 2 ? 128 * ia : 0) + 8 * ch;       // NBI = 2: this wave stages rows of B image `ia`
    const void* zero = reinterpret_cast<const void*>(g_zero_page);
    int m_next = row_begin + 4 * wq + prow;
    const uint32_t lds0 = static_cast<uint32_t>(
        reinterpret_cast<uintptr_t>((__attribute__((address_space(3))) unsigned char*)smem));

    // The pixel row changes with every K step here (in the NN kernels it is fixed per block), so the row -> source
    // address arithmetic is in the steady-state loop: straight-line integer code without divisions or branches
    // (power-of-two pixel grid: plan_tn16x), about 25 VALU instructions per LDS-DMA.  The first form of this kernel
    // reused the generic gather helpers and spent ~700 instructions per K step for 16 MFMAs - issue-bound at 23 %
    // MFMA busy with the data already in LDS.
    const int dh = a_kh - g.pad, dw = a_kw - g.pad;                   // tap displacement of this lane's channel chunk
    const unsigned hmax = g.reflect ? 0xffffffffu : (unsigned)g.Hs - 1u;   // zero padding: out-of-range sources are zeros
    const unsigned wmax = g.reflect ? 0xffffffffu : (unsigned)g.Ws - 1u;
    const int h2 = 2 * (g.Hs - 1), w2 = 2 * (g.Ws - 1);
    const int wmask = g.Wq - 1, hmask = g.Hq - 1, bsh = p.wq_shift + p.hq_shift;
    const int a_lim = mf < p.Mf ? row_end : 0, b_lim = cb < p.Cb ? row_end : 0;
    const unsigned char* abase = reinterpret_cast<const unsigned char*>(reinterpret_cast<const __bf16*>(p.A) + a_c);
    const unsigned char* bbase = reinterpret_cast<const unsigned char*>(reinterpret_cast<const __bf16*>(p.Bv) + cb);
    const unsigned ald2 = 2u * (unsigned)g.ld, bld2 = 2u * (unsigned)p.b_ld;

    // wave-uniform LDS destinations as scalars (SALU adds per LDS-DMA instead of VALU + readfirstlane)
    const uint32_t sa0 = __builtin_amdgcn_readfirstlane(lds0 + ia * TILE + (4 * wq) * 256);
    const uint32_t sb0 = __builtin_amdgcn_readfirstlane(lds0 + (2 + (NBI == 2 ? ia : 0)) * TILE + (4 * wq) * 256);
    auto stage = [&](int slot) {
        const uint32_t sa = sa0 + slot * TNX_STAGE;
        const uint32_t sb = sb0 + slot * TNX_STAGE;
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int m = m_next + 16 * j;
            unsigned pix = (unsigned)m;
            bool ok = m < a_lim;
            if (MODE != GATHER_PLAIN) {
                const int wo = m & wmask, ho = (m >> p.wq_shift) & hmask, b = m >> bsh;
                const int h = __mul24(ho, g.stride) + dh, wsrc = __mul24(wo, g.stride) + dw;
                const int ha = h < 0 ? -h : h, wa = wsrc < 0 ? -wsrc : wsrc;          // tf.pad(REFLECT): -1 -> 1, n -> n - 2
                const int hr = min(ha, h2 - ha), wr = min(wa, w2 - wa);
                ok = ok & ((unsigned)h <= hmax) & ((unsigned)wsrc <= wmax);
                pix = __umul24(__umul24((unsigned)b, (unsigned)g.Hs) + (unsigned)hr, (unsigned)g.Ws) + (unsigned)wr;
            }
            const void* srca = ok ? static_cast<const void*>(abase + (uint64_t)pix * ald2) : zero;
            glds16_asm(srca, sa + j * 16 * 256);
            if (NBI == 2 || j / (NJ / 2) == ia) {      // (wave-uniform) this wave's share of the B image's rows
                const void* srcb = m < b_lim ? static_cast<const void*>(bbase + (uint64_t)(unsigned)m * bld2) : zero;
                glds16_asm(srcb, sb + j * 16 * 256);
            }
        }
        m_next += BK;
    };

    constexpr int NBJ = 2 * NBI;                       // 32-column MFMA tiles per wave
    f32x16_t acc[2][NBJ];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < NBJ; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    const int kblk = lane >> 5, g16 = (lane >> 4) & 1, q = (lane & 15) >> 2, pq = lane & 3;
    uint32_t a_ad[2][2], b_ad[NBJ][2];
#pragma unroll
    for (int jj = 0; jj < 2; ++jj) {
        const int row = 8 * kblk + 4 * jj + q;
#pragma unroll
        for (int i = 0; i < 2; ++i)
            a_ad[i][jj] = lds0 + (wm >> 1) * TILE +
                          tr16_swz(row, 4 * ((wm & 1) * 2 + i) + 2 * g16 + (pq >> 1)) + 8 * (pq & 1);
#pragma unroll
        for (int j = 0; j < NBJ; ++j)      // NBI = 1: 32-column blocks 2 wn, 2 wn + 1 of the one image; NBI = 2: all four of image wn
            b_ad[j][jj] = lds0 + (2 + (NBI == 2 ? wn : 0)) * TILE +
                          tr16_swz(row, 4 * (NBI == 2 ? j : wn * 2 + j) + 2 * g16 + (pq >> 1)) + 8 * (pq & 1);
    }
    auto operand = [&](uint32_t lo_addr, uint32_t hi_addr) {
        const s16x4v lo = lds_tr16(lo_addr), hi = lds_tr16(hi_addr);
        const s16x8v v = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
        return __builtin_bit_cast(bf16x8_t, v);
    };

    if (nsteps > 0) stage(0);
    if (nsteps > 1) stage(1);
    // one K step on ring slot SLOT (a compile-time constant: the operand addresses are base + immediate)
    auto kstep = [&](int it, auto slot_c) {
        constexpr int SLOT = decltype(slot_c)::value;
        // tile `it` has landed (this wave's part; the barrier extends that to every wave); tile it + 1 stays in flight
        if (it + 1 < nsteps) {                              // DMA per wave and tile: NJ (A) + NJ / 2 (B), or NJ + NJ with two B images
            if (BK == 64 && NBI == 2) asm volatile("s_waitcnt vmcnt(8) lgkmcnt(0)" ::: "memory");
            else if (BK == 64) asm volatile("s_waitcnt vmcnt(6) lgkmcnt(0)" ::: "memory");
            else if (NBI == 2) asm volatile("s_waitcnt vmcnt(4) lgkmcnt(0)" ::: "memory");
            else asm volatile("s_waitcnt vmcnt(3) lgkmcnt(0)" ::: "memory");
        } else
            asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        if (it + 2 < nsteps) stage((SLOT + 2) % 3);      // the slot every wave finished reading before this barrier
        constexpr uint32_t bufoff = (uint32_t)SLOT * (uint32_t)TNX_STAGE;
#pragma unroll
        for (int s = 0; s < BK / 16; ++s) {
            bf16x8_t a[2], b[NBJ];
#pragma unroll
            for (int i = 0; i < 2; ++i) a[i] = operand(a_ad[i][0] + (bufoff + 4096 * s), a_ad[i][1] + (bufoff + 4096 * s));
#pragma unroll
            for (int j = 0; j < NBJ; ++j) b[j] = operand(b_ad[j][0] + (bufoff + 4096 * s), b_ad[j][1] + (bufoff + 4096 * s));
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < NBJ; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[i], b[j], acc[i][j], 0, 0, 0);
        }
    };
    for (int it = 0; it < nsteps; it += 3) {
        kstep(it, std::integral_constant<int, 0>());
        if (it + 1 < nsteps) kstep(it + 1, std::integral_constant<int, 1>());
        if (it + 2 < nsteps) kstep(it + 2, std::integral_constant<int, 2>());
    }

    float* obase = p.out + (int64_t)zs * p.slab_stride;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = mf0 + wm * 64 + 32 * i + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
            if (row >= p.Mf) continue;
#pragma unroll
            for (int j = 0; j < NBJ; ++j) {
                const int col = cb0 + wn * 32 * NBJ + 32 * j + (lane & 31);
                if (col < p.Cb) obase[(int64_t)row * p.out_ld + col] = acc[i][j][r];
            }
        }
    }
}

// ------------------------------------------------------------------------------------------
// TN kernel, phased form: 256 x BN tile (BN = 192, 256), 8 waves as 4 (rows) x 2 (columns), ONE block per CU.
//   tn16x_kernel<.., 32, 2> already had the 256 x 256 tile and bought nothing with it: alone on its CU, two waves per SIMD,
//   a ring schedule idles the matrix pipe at every barrier.  This is that tile under nn16_kernel's phased schedule, and a
//   192-column tile beside it (Cb = 192, 384, 768, 1536 are whole multiples of 192: no padding columns, 110 FLOP per staged
//   byte; 256 columns: 131).  Wave (wm, wn) owns rows 64 wm .. + 63 and the 32-column fragments NBJ wn + j (j < NBJ = BN / 64);
//   fragment f is 32-column block f & 3 of B image f >> 2.  At BN = 192 only chunks 0 - 7 of B image 1 are staged (the
//   other lanes of those LDS-DMA instructions are masked) and read.
//   LDS is a ring of NKB K BLOCKS of 16 pixels: [A image 0 | A image 1 | B image 0 | B image 1], 4 KB each ([16 pixels][128
//   channels] bf16, tr16_swz as in the kernels above) = 16 KB per block, NKB = 6 (96 KB) or 8 (128 KB: measured, no faster).
//   A K block is one phase and moves as 16 LDS-DMA instructions, two per wave (one A, one B): pixel rows
//   4 (w & 3) + (lane >> 4) of image w >> 2.  The operands of a block are read into registers one phase ahead, so the
//   transposed LDS reads of block n + 1 run under the MFMAs of block n.  Phase n (K block n, ring slot n % NKB):
//     {s_waitcnt vmcnt(2 (NKB - 2)) lgkmcnt(0) ; s_barrier ; ds_read_tr16_b64 operands of block n + 1 ;
//      s_setprio(1) ; NBJ MFMAs of block n ; s_setprio(0) ; LDS-DMA of block n + NKB into slot n % NKB ;
//      s_setprio(1) ; NBJ MFMAs of block n ; s_setprio(0)}
//   ONE barrier per phase.  The row -> source arithmetic and the two LDS-DMA of a phase sit between the halves of its MFMAs,
//   where the matrix pipe has the first half queued (measured against the issue in front of the barrier, the pipe idle
//   behind it: 1 - 4 % per launch; and against waves 0 - 3 issuing before and waves 4 - 7 after their MFMAs: that lost 7 %).
//   Write after read: slot n % NKB was last read for block n, in phase n - 1; every wave retires those reads with the
//   lgkmcnt(0) in front of the barrier of phase n, and the LDS-DMA into the slot is issued behind that barrier.  Read after
//   write: at the wait of phase n a wave has issued the blocks up to n + NKB - 1, two instructions each, so
//   vmcnt(2 (NKB - 2)) leaves the NKB - 2 youngest in flight and retires its part of block n + 1; the barrier extends that
//   to every wave, and block n + 1 is read behind it.  The blocks n + 2 ... stay in flight across the barrier.  The last
//   NKB phases have nothing to issue; there the wait drains the queue (vmcnt(0)), outside the steady loop.
//   Sums: every accumulator takes the 16-pixel K blocks of its split in increasing pixel order, the same MFMA on the same
//   operands as tn16x_kernel, over the same (zero-padded to 32 pixels) range - bit-identical to it under the same split.
// ------------------------------------------------------------------------------------------
constexpr int tn16xp_lds_bytes(int NKB) { return NKB * 4 * 16 * 256; }

template <int MODE, int BN, int NKB>
__global__ __launch_bounds__(512, 2) void tn16x_phased_kernel(const TN16Params p) {
    static_assert(BN == 192 || BN == 256, "column tile: B image 0 and half or all of B image 1");
    static_assert(NKB >= 3, "ring: the block being read, the block that lands next, at least one more in flight");
    constexpr int NBJ = BN / 64;                        // 32-column MFMA tiles per wave
    constexpr int IMG = 16 * 256;                       // bytes of one [16 pixels][128 channels] bf16 image
    constexpr int KBLK = 4 * IMG;                       // A image 0 | A image 1 | B image 0 | B image 1
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];   // NKB K blocks

    const int t = threadIdx.x;
    const int lane = t & 63, w = t >> 6;
    const int wm = w >> 1, wn = w & 1;
    const Gather& g = p.g;

    const int ntile = p.tiles_m * p.tiles_n;
    const int lin = xcd_remap(blockIdx.x, ntile * p.splitk);
    const int zs = lin / ntile;
    const int tile = lin - zs * ntile;
    const int tile_n = tile % p.tiles_n, tile_m = tile / p.tiles_n;
    const int mf0 = tile_m * 256, cb0 = tile_n * BN;
    const int row_begin = zs * p.rows_per_split;
    const int row_end = min(p.M, row_begin + p.rows_per_split);
    const int nkb = 2 * max(0, (row_end - row_begin + 31) / 32);      // (tn16x_kernel's range: whole 32-pixel tiles)

    // staging role: pixel row 4 wq + prow of the K block, channel chunk `ch` of A image ia and of B image ia
    const int prow = lane >> 4;
    const int wq = w & 3, ia = w >> 2;
    const int ch = (lane & 15) ^ ((prow << 2) | wq);
    const int mf = mf0 + 128 * ia + 8 * ch;
    int a_kh = 0, a_kw = 0, a_c = mf;
    if (MODE != GATHER_PLAIN) {
        const int tap = mf / p.Ca;
        a_c = mf - tap * p.Ca;
        a_kh = tap / g.k;
        a_kw = tap - a_kh * g.k;
    }
    const int cb = cb0 + 128 * ia + 8 * ch;
    const bool b_lane = BN == 256 || ia == 0 || ch < 8;           // BN = 192: the next tile's columns are not staged
    const void* zero = reinterpret_cast<const void*>(g_zero_page);
    int m_next = row_begin + 4 * wq + prow;
    const uint32_t lds0 = static_cast<uint32_t>(
        reinterpret_cast<uintptr_t>((__attribute__((address_space(3))) unsigned char*)smem));

    // row -> source address as in tn16x_kernel: shifts on a power-of-two pixel grid, no divisions or branches
    const int dh = a_kh - g.pad, dw = a_kw - g.pad;
    const unsigned hmax = g.reflect ? 0xffffffffu : (unsigned)g.Hs - 1u;
    const unsigned wmax = g.reflect ? 0xffffffffu : (unsigned)g.Ws - 1u;
    const int h2 = 2 * (g.Hs - 1), w2 = 2 * (g.Ws - 1);
    const int wmask = g.Wq - 1, hmask = g.Hq - 1, bsh = p.wq_shift + p.hq_shift;
    const int a_lim = mf < p.Mf ? row_end : 0, b_lim = cb < p.Cb ? row_end : 0;
    const unsigned char* abase = reinterpret_cast<const unsigned char*>(reinterpret_cast<const __bf16*>(p.A) + a_c);
    const unsigned char* bbase = reinterpret_cast<const unsigned char*>(reinterpret_cast<const __bf16*>(p.Bv) + cb);
    const unsigned ald2 = 2u * (unsigned)g.ld, bld2 = 2u * (unsigned)p.b_ld;

    const uint32_t sa0 = __builtin_amdgcn_readfirstlane(lds0 + ia * IMG + (4 * wq) * 256);
    const uint32_t sb0 = __builtin_amdgcn_readfirstlane(lds0 + (2 + ia) * IMG + (4 * wq) * 256);
    // LDS-DMA of the K cursor's block into ring slot `slot`: two instructions per wave, always (the counted waits rely on it)
    auto issue = [&](int slot) __attribute__((always_inline)) {
        const int m = m_next;
        unsigned pix = (unsigned)m;
        bool ok = m < a_lim;
        if (MODE != GATHER_PLAIN) {
            const int wo = m & wmask, ho = (m >> p.wq_shift) & hmask, b = m >> bsh;
            const int h = __mul24(ho, g.stride) + dh, wsrc = __mul24(wo, g.stride) + dw;
            const int ha = h < 0 ? -h : h, wa = wsrc < 0 ? -wsrc : wsrc;          // tf.pad(REFLECT): -1 -> 1, n -> n - 2
            const int hr = min(ha, h2 - ha), wr = min(wa, w2 - wa);
            ok = ok & ((unsigned)h <= hmax) & ((unsigned)wsrc <= wmax);
            pix = __umul24(__umul24((unsigned)b, (unsigned)g.Hs) + (unsigned)hr, (unsigned)g.Ws) + (unsigned)wr;
        }
        const void* srca = ok ? static_cast<const void*>(abase + (uint64_t)pix * ald2) : zero;
        glds16_asm(srca, sa0 + slot * KBLK);
        const void* srcb = m < b_lim ? static_cast<const void*>(bbase + (uint64_t)(unsigned)m * bld2) : zero;
        if (b_lane) glds16_asm(srcb, sb0 + slot * KBLK);
        m_next += 16;
    };

    f32x16_t acc[2][NBJ];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < NBJ; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    // transposed-read addresses (slot 0): as in tn16x_kernel, rows 0 .. 15 of the K block
    const int kblk = lane >> 5, g16 = (lane >> 4) & 1, q = (lane & 15) >> 2, pq = lane & 3;
    uint32_t a_ad[2][2], b_ad[NBJ][2];
#pragma unroll
    for (int jj = 0; jj < 2; ++jj) {
        const int row = 8 * kblk + 4 * jj + q;
#pragma unroll
        for (int i = 0; i < 2; ++i)
            a_ad[i][jj] = lds0 + (wm >> 1) * IMG +
                          tr16_swz(row, 4 * ((wm & 1) * 2 + i) + 2 * g16 + (pq >> 1)) + 8 * (pq & 1);
#pragma unroll
        for (int j = 0; j < NBJ; ++j) {
            const int f = NBJ * wn + j;
            b_ad[j][jj] = lds0 + (2 + (f >> 2)) * IMG + tr16_swz(row, 4 * (f & 3) + 2 * g16 + (pq >> 1)) + 8 * (pq & 1);
        }
    }
    auto operand = [&](uint32_t lo_addr, uint32_t hi_addr) __attribute__((always_inline)) {
        const s16x4v lo = lds_tr16(lo_addr), hi = lds_tr16(hi_addr);
        const s16x8v v = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
        return __builtin_bit_cast(bf16x8_t, v);
    };

    // operands of block n in registers of parity n & 1: block n + 1 is read from LDS while block n is multiplied
    bf16x8_t ra[2][2], rb[2][NBJ];
    auto read_block = [&](auto slot_c) __attribute__((always_inline)) {
        constexpr int SLOT = decltype(slot_c)::value;
        constexpr uint32_t off = (uint32_t)SLOT * (uint32_t)KBLK;
#pragma unroll
        for (int i = 0; i < 2; ++i) ra[SLOT & 1][i] = operand(a_ad[i][0] + off, a_ad[i][1] + off);
#pragma unroll
        for (int j = 0; j < NBJ; ++j) rb[SLOT & 1][j] = operand(b_ad[j][0] + off, b_ad[j][1] + off);
    };
    // one phase on ring slot SLOT (a compile-time constant); TAIL: one of the phases at the end of the range, where the issue
    // may be past it and the queue drains
    auto phase = [&](int n, auto slot_c, auto tail_c) __attribute__((always_inline)) {
        constexpr int SLOT = decltype(slot_c)::value;
        constexpr bool TAIL = decltype(tail_c)::value;
        if (!TAIL || n + NKB <= nkb) asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(2 * (NKB - 2)) : "memory");
        else asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_waitcnt(0xC07F);          // lgkmcnt(0) once more, where the compiler's own wait counting sees it
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_sched_barrier(0);
        if (!TAIL || n + 1 < nkb) read_block(std::integral_constant<int, (SLOT + 1) % NKB>());
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int j = 0; j < NBJ; ++j)
            acc[0][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ra[SLOT & 1][0], rb[SLOT & 1][j], acc[0][j], 0, 0, 0);
        __builtin_amdgcn_s_setprio(0);
        __builtin_amdgcn_sched_barrier(0);
        if (!TAIL || n + NKB < nkb) issue(SLOT);
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int j = 0; j < NBJ; ++j)
            acc[1][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ra[SLOT & 1][1], rb[SLOT & 1][j], acc[1][j], 0, 0, 0);
        __builtin_amdgcn_s_setprio(0);
        __builtin_amdgcn_sched_barrier(0);
    };
    auto round = [&](int n, auto tail_c) __attribute__((always_inline)) {            // NKB phases from block n (n % NKB == 0), as far as the range goes
        phase(n, std::integral_constant<int, 0>(), tail_c);
        if (n + 1 < nkb) phase(n + 1, std::integral_constant<int, 1>(), tail_c);
        if (n + 2 < nkb) phase(n + 2, std::integral_constant<int, 2>(), tail_c);
        if (n + 3 < nkb) phase(n + 3, std::integral_constant<int, 3>(), tail_c);
        if (n + 4 < nkb) phase(n + 4, std::integral_constant<int, 4>(), tail_c);
        if (n + 5 < nkb) phase(n + 5, std::integral_constant<int, 5>(), tail_c);
        if constexpr (NKB == 8) {
            if (n + 6 < nkb) phase(n + 6, std::integral_constant<int, 6>(), tail_c);
            if (n + 7 < nkb) phase(n + 7, std::integral_constant<int, 7>(), tail_c);
        }
    };
    static_assert(NKB == 6 || NKB == 8, "round() spells the phases out");

    // prologue: blocks 0 .. NKB - 1 issued, block 0 landed and read - the state every phase starts from
#pragma unroll
    for (int k = 0; k < NKB; ++k)
        if (k < nkb) issue(k);
    if (nkb >= NKB) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * (NKB - 1)) : "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    if (nkb > 0) read_block(std::integral_constant<int, 0>());
    const std::integral_constant<bool, false> steady;
    const std::integral_constant<bool, true> tail;
    int n = 0;
    for (; n + 2 * NKB <= nkb; n += NKB) round(n, steady);            // (the round's last phase still has a block to issue)
    if (n < nkb) round(n, tail);
    if (n + NKB < nkb) round(n + NKB, tail);

    float* obase = p.out + (int64_t)zs * p.slab_stride;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = mf0 + wm * 64 + 32 * i + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
            if (row >= p.Mf) continue;
#pragma unroll
            for (int j = 0; j < NBJ; ++j) {
                const int col = cb0 + 32 * (NBJ * wn + j) + (lane & 31);
                if (col < p.Cb) obase[(int64_t)row * p.out_ld + col] = acc[i][j][r];
            }
        }
    }
}

// ------------------------------------------------------------------------------------------
// transpose of tf.pad(REFLECT) (ops.py:82): fold the gradient on the padded grid back onto the image
// ------------------------------------------------------------------------------------------
template <bool F32>
__global__ __launch_bounds__(256) void reflect_fold_kernel(const void* __restrict__ dxp_, void* __restrict__ dx_, int N,
                                                           int H, int W, int C8, int Hp, int Wp, int pad,
                                                           int accumulate) {
    const int64_t total = (int64_t)N * H * W * C8;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int c8 = (int)(i % C8);
        int64_t t = i / C8;
        const int w = (int)(t % W);
        t /= W;
        const int h = (int)(t % H);
        const int n = (int)(t / H);
        // padded positions that mirror onto h: h + pad, pad - h (h >= 1), 2 (H - 1) - h + pad (h <= H - 2)
        int hs[3], ws[3], nh = 0, nw = 0;
        hs[nh++] = h + pad;
        if (h >= 1 && pad - h >= 0) hs[nh++] = pad - h;
        if (h <= H - 2 && 2 * (H - 1) - h + pad < Hp && H > 1) hs[nh++] = 2 * (H - 1) - h + pad;
        ws[nw++] = w + pad;
        if (w >= 1 && pad - w >= 0) ws[nw++] = pad - w;
        if (w <= W - 2 && 2 * (W - 1) - w + pad < Wp && W > 1) ws[nw++] = 2 * (W - 1) - w + pad;
        float acc[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] = 0.f;
        for (int a = 0; a < nh; ++a)
            for (int b = 0; b < nw; ++b) {
                if (hs[a] >= Hp || ws[b] >= Wp) continue;
                const int64_t off = ((((int64_t)n * Hp + hs[a]) * Wp + ws[b]) * C8 + c8) * 8;
                if (F32) {
                    const float* sp = reinterpret_cast<const float*>(dxp_) + off;
                    const f32x4_t v0 = *reinterpret_cast<const f32x4_t*>(sp), v1 = *reinterpret_cast<const f32x4_t*>(sp + 4);
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        acc[j] += v0[j];
                        acc[4 + j] += v1[j];
                    }
                } else {
                    const uint4 r = *reinterpret_cast<const uint4*>(reinterpret_cast<const __bf16*>(dxp_) + off);
                    acc[0] += bf16_lo(r.x); acc[1] += bf16_hi(r.x); acc[2] += bf16_lo(r.y); acc[3] += bf16_hi(r.y);
                    acc[4] += bf16_lo(r.z); acc[5] += bf16_hi(r.z); acc[6] += bf16_lo(r.w); acc[7] += bf16_hi(r.w);
                }
            }
        if (F32) {
            float* o = reinterpret_cast<float*>(dx_) + i * 8;
            f32x4_t v0 = {acc[0], acc[1], acc[2], acc[3]}, v1 = {acc[4], acc[5], acc[6], acc[7]};
            if (accumulate) {
                v0 += *reinterpret_cast<const f32x4_t*>(o);
                v1 += *reinterpret_cast<const f32x4_t*>(o + 4);
            }
            *reinterpret_cast<f32x4_t*>(o) = v0;
            *reinterpret_cast<f32x4_t*>(o + 4) = v1;
        } else {
            __bf16* o = reinterpret_cast<__bf16*>(dx_) + i * 8;
            if (accumulate) {
                const uint4 r = *reinterpret_cast<const uint4*>(o);
                acc[0] += bf16_lo(r.x); acc[1] += bf16_hi(r.x); acc[2] += bf16_lo(r.y); acc[3] += bf16_hi(r.y);
                acc[4] += bf16_lo(r.z); acc[5] += bf16_hi(r.z); acc[6] += bf16_lo(r.w); acc[7] += bf16_hi(r.w);
            }
            uint4 r;
            r.x = pack_bf16x2(acc[0], acc[1]);
            r.y = pack_bf16x2(acc[2], acc[3]);
            r.z = pack_bf16x2(acc[4], acc[5]);
            r.w = pack_bf16x2(acc[6], acc[7]);
            *reinterpret_cast<uint4*>(o) = r;
        }
    }
}

// the same fold, one fp32 element per thread: channel counts that are no multiple of 8 (fp32 tensors only)
__global__ __launch_bounds__(256) void reflect_fold_scalar_kernel(const float* __restrict__ dxp, float* __restrict__ dx,
                                                                  int N, int H, int W, int C, int Hp, int Wp, int pad,
                                                                  int accumulate) {
    const int64_t total = (int64_t)N * H * W * C;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int c = (int)(i % C);
        int64_t t = i / C;
        const int w = (int)(t % W);
        t /= W;
        const int h = (int)(t % H);
        const int n = (int)(t / H);
        int hs[3], ws[3], nh = 0, nw = 0;
        hs[nh++] = h + pad;
        if (h >= 1 && pad - h >= 0) hs[nh++] = pad - h;
        if (h <= H - 2 && 2 * (H - 1) - h + pad < Hp) hs[nh++] = 2 * (H - 1) - h + pad;
        ws[nw++] = w + pad;
        if (w >= 1 && pad - w >= 0) ws[nw++] = pad - w;
        if (w <= W - 2 && 2 * (W - 1) - w + pad < Wp) ws[nw++] = 2 * (W - 1) - w + pad;
        float acc = 0.f;
        for (int a = 0; a < nh; ++a)
            for (int b = 0; b < nw; ++b) {
                if (hs[a] >= Hp || ws[b] >= Wp) continue;
                acc += dxp[(((int64_t)n * Hp + hs[a]) * Wp + ws[b]) * C + c];
            }
        dx[i] = accumulate ? dx[i] + acc : acc;
    }
}

int launch_reflect_fold(const void* dxp, void* dx, int f32, int N, int H, int W, int C, int Hp, int Wp, int pad_lo,
                        int accumulate, hipStream_t s) {
    if (C % 8 != 0) {
        BG_REQUIRE(f32, "reflect fold: bf16 tensors need C %% 8 == 0");
        const int64_t n = (int64_t)N * H * W * C;
        int64_t nb = (n + 255) / 256;
        if (nb > 4096) nb = 4096;
        hipLaunchKernelGGL(reflect_fold_scalar_kernel, dim3((unsigned)nb), dim3(256), 0, s, (const float*)dxp, (float*)dx, N,
                           H, W, C, Hp, Wp, pad_lo, accumulate);
        BG_LAUNCH_CHECK();
        return BG_OK;
    }
    const int64_t total = (int64_t)N * H * W * (C / 8);
    int64_t blocks = (total + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    if (f32)
        hipLaunchKernelGGL((reflect_fold_kernel<true>), dim3((unsigned)blocks), dim3(256), 0, s, dxp, dx, N, H, W, C / 8, Hp,
                           Wp, pad_lo, accumulate);
    else
        hipLaunchKernelGGL((reflect_fold_kernel<false>), dim3((unsigned)blocks), dim3(256), 0, s, dxp, dx, N, H, W, C / 8,
                           Hp, Wp, pad_lo, accumulate);
    BG_LAUNCH_CHECK();
    return BG_OK;
}

// ------------------------------------------------------------------------------------------
// host side: the launchers run the plans of igemm16_plan.h
// ------------------------------------------------------------------------------------------
static_assert(P16_BM == NN16_BM && P16_HALO_T == NH_T && P16_TN_BK == TN16_BK, "igemm16_plan.h counts with other tiles");

// An instantiation: the kernel and its dynamic LDS bytes.
struct NN16Inst { void (*fn)(NN16Params); int lds; };
struct TN16Inst { void (*fn)(TN16Params); int lds; };

// nn16_kernel<TN, MODE, PM, RING, SLOTS, WM> by pipeline form.  RING: a mirrored-tap launch (position-major, two stages or
// the 128-row ring); the wide form has image-major rows only (nn16_form).
template <int TN, int MODE, bool PM, bool RING>
static NN16Inst nn16_inst_form(int form) {
    constexpr int TAPS = RING ? NN16_RING_TAPS : NN16_TAPS;
    if (form == NN16_FORM_RING) return {&nn16_kernel<TN, MODE, PM, RING, 3, 2>, nn16_pipe_lds_bytes(TN, 2, TAPS)};
    if constexpr (!PM)
        if (form == NN16_FORM_WIDE) return {&nn16_kernel<TN, MODE, PM, false, 3, 4>, nn16_pipe_lds_bytes(TN, 4)};
    return {&nn16_kernel<TN, MODE, PM, RING, 2, 2>, nn16_lds_bytes(TN, TAPS)};
}

template <int MODE, bool PM, bool RING = false>
static NN16Inst nn16_inst_tn(const NN16Launch& l) {
    if constexpr (!RING)
        if (l.form == NN16_FORM_PHASED)                // (tn: the form's own column tile, 4, 6 or 8)
            return l.tn == 8   ? NN16Inst{&nn16_kernel<8, MODE, PM, false, 2, 4>, nn16x_lds_bytes(8)}
                   : l.tn == 6 ? NN16Inst{&nn16_kernel<6, MODE, PM, false, 2, 4>, nn16x_lds_bytes(6)}
                               : NN16Inst{&nn16_kernel<4, MODE, PM, false, 2, 4>, nn16x_lds_bytes(4)};
    switch (l.tn) {
        case 1: return nn16_inst_form<1, MODE, PM, RING>(l.form);
        case 2: return nn16_inst_form<2, MODE, PM, RING>(l.form);
        case 3: return nn16_inst_form<3, MODE, PM, RING>(l.form);
        default: return nn16_inst_form<4, MODE, PM, RING>(l.form);
    }
}

template <int NT, int MODE>
static NN16Inst nn16h_inst_nf(int nf) {
    switch (nf) {
        case 1: return {&nn16h_kernel<NT, 1, MODE>, nn16h_lds_bytes<NT, 1>()};
        case 2: return {&nn16h_kernel<NT, 2, MODE>, nn16h_lds_bytes<NT, 2>()};
        case 3: return {&nn16h_kernel<NT, 3, MODE>, nn16h_lds_bytes<NT, 3>()};
        default: return {&nn16h_kernel<NT, 4, MODE>, nn16h_lds_bytes<NT, 4>()};
    }
}

// THE dispatch of the forward / input-gradient launches: plan fields -> instantiation
static NN16Inst nn16_inst(const NN16Launch& l) {
    switch (l.family) {
        case NN16_HALO_D2S: return {&nn16h_kernel<2, 1, GATHER_CONV, 1>, nn16h_lds_bytes<2, 1>()};
        case NN16_HALO:
            if (l.mode == GATHER_CONV) return nn16h_inst_nf<3, GATHER_CONV>(l.nf);
            return l.nt == 3 ? nn16h_inst_nf<3, GATHER_TCONV>(l.nf) : nn16h_inst_nf<2, GATHER_TCONV>(l.nf);
        case NN16_MIRROR_RING: return nn16_inst_tn<GATHER_TCONV, true, true>(l);
        default:
            if (l.mode == GATHER_CONV)
                return l.posmajor ? nn16_inst_tn<GATHER_CONV, true>(l) : nn16_inst_tn<GATHER_CONV, false>(l);
            return l.posmajor ? nn16_inst_tn<GATHER_TCONV, true>(l) : nn16_inst_tn<GATHER_TCONV, false>(l);
    }
}
int nn16_launch_lds(const NN16Launch& l) { return nn16_inst(l).lds; }

// The shared tail: the plan's fields into the parameter block, the launch, its check, the slab reduce of a split launch.
// record: name the instantiation for bg_prof (the mirrored-tap launch leaves the plain launch's name in place).
static int nn16_run(NN16Params& p, const NN16Launch& l, bool record, hipStream_t s) {
    BG_REQUIRE(l.grid_x > 0 && l.grid_x < (int64_t(1) << 31), "bf16-resident conv: grid out of range");
    p.splitk = l.splitk; p.posmajor = l.posmajor; p.mfast = l.mfast; p.zfold = l.zfold;
    p.pow2 = l.pow2; p.wq_shift = l.wq_shift; p.hq_shift = l.hq_shift;
    p.tiles_m = l.tiles_m; p.tiles_n = l.tiles_n;
    const NN16Inst k = nn16_inst(l);
    // > 48 KB of dynamic LDS needs the opt-in once per kernel and device
    if (!lds_opt_in(reinterpret_cast<const void*>(k.fn), k.lds)) return BG_ERR_LAUNCH;
    if (record && prof_on()) {
        char name[48];
        nn16_launch_name(l, name, sizeof(name));
        prof_kernel("%s", name);
    }
    hipLaunchKernelGGL(k.fn, dim3((unsigned)l.grid_x, 1, l.grid_z), dim3(l.block), k.lds, s, p);
    BG_LAUNCH_CHECK();
    if (l.splitk > 1) {
        const int64_t n8 = p.slab_stride / 8;
        int blocks = (int)((n8 + 255) / 256);
        if (blocks > 2048) blocks = 2048;
        hipLaunchKernelGGL(nn16_slab_reduce_kernel, dim3(blocks), dim3(256), 0, s, p.slabs, p.out, p.bias, p.alpha, n8,
                           p.N, l.splitk, p.slab_stride, p.accumulate, p.out_f32);
        BG_LAUNCH_CHECK();
    }
    return BG_OK;
}

int launch_nn16(NN16Params& p, const NN16Launch& l, int64_t out_elems, void* ws, hipStream_t s) {
    BG_REQUIRE(p.C % 8 == 0 && p.N % 8 == 0 && p.g.ld % 8 == 0 && p.out_ld % 8 == 0,
               "bf16-resident conv: channel counts must be multiples of 8 (C=%d N=%d)", p.C, p.N);
    BG_REQUIRE((reinterpret_cast<uintptr_t>(p.A) & 15) == 0 && (reinterpret_cast<uintptr_t>(p.B) & 15) == 0 &&
                   (reinterpret_cast<uintptr_t>(p.out) & 15) == 0,
               "bf16-resident conv: tensors must be 16-byte aligned");
    BG_REQUIRE(p.g.k >= 1 && p.g.k <= NN16_TAPS && p.C <= 8192 && p.g.stride >= 1 && p.g.stride <= 2,
               "bf16-resident conv: kernel size %d / stride %d / %d channels not supported", p.g.k, p.g.stride, p.C);
    BG_REQUIRE((int64_t)p.g.Nb * p.g.Hs * p.g.Ws < (int64_t(1) << 30) && (int64_t)p.g.Nb * p.g.Ho * p.g.Wo < (int64_t(1) << 31),
               "bf16-resident conv: more than 2^30 source / 2^31 output pixels");
    BG_REQUIRE(p.d2s_c == 0 || (l.d2s_store && ws == nullptr),
               "bf16-resident conv: this launch has no depth-to-space store (bg_conv2d_fwd_d2s_supported)");
    BG_REQUIRE(l.family == NN16_HALO || p.stats_part == nullptr,
               "bf16-resident conv: fused statistics need the halo-tile form (bg_deconv2d_fwd_stats_workspace_bytes)");
    BG_REQUIRE((l.family == NN16_HALO || l.family == NN16_TAP) && (l.splitk == 1 || ws != nullptr),
               "bf16-resident conv: not a plan of this launch");
    p.slabs = reinterpret_cast<float*>(ws);
    p.slab_stride = out_elems;
    return nn16_run(p, l, true, s);
}

int launch_nn16_ring(NN16Params& p, const NN16Launch& l, hipStream_t s) {
    BG_REQUIRE(p.ring == 1 && (p.ring_lines == 1 || p.ring_lines == 2), "nn16 ring launch: ring = 1, ring_lines 1 or 2");
    BG_REQUIRE(l.family == NN16_MIRROR_RING && p.g.k >= 1 && p.g.k <= NN16_RING_TAPS / 2 && p.g.Ho >= 4 && p.g.Wo >= 4 &&
                   p.accumulate == 1,
               "nn16 ring launch: kernel size %d / map %d x %d not supported", p.g.k, p.g.Ho, p.g.Wo);
    BG_REQUIRE(p.C % 8 == 0 && p.N % 8 == 0 && p.g.ld % 8 == 0 && p.out_ld % 8 == 0, "nn16 ring launch: channels %% 8");
    const int npos = p.ring_lines * p.g.Wo + p.ring_lines * (p.g.Ho - p.ring_lines);
    p.g.pstep = 1;
    p.g.Hq = 1;
    p.g.Wq = npos;
    p.M = p.g.Nb * npos;
    p.slabs = nullptr;
    return nn16_run(p, l, false, s);
}

// The THIN = 1 form of nn16h_kernel (see there): plain describes the plain transposed gather (nn16h_d2s_ok).
int launch_nn16h_d2s(const NN16Params& plain, const NN16Launch& l, hipStream_t s) {
    BG_REQUIRE(l.family == NN16_HALO_D2S, "nn16h depth-to-space form: not a plan of this launch");
    NN16Params p = plain;
    Gather& g = p.g;
    g.Hq = g.Hs; g.Wq = g.Ws; g.pstep = 1; g.pad = 0; g.stride = 1;
    p.N = 32;
    p.ring = 0;
    return nn16_run(p, l, true, s);
}

// THE dispatch of the weight-gradient launches
static TN16Inst tn16_inst(const TN16Launch& l) {
    const bool conv = l.mode == GATHER_CONV;
    if (l.kernel == TN16_PHASED) {                     // (gathered operands only: tn16x_phased_bn)
        const int lds = tn16xp_lds_bytes(l.nkb);
        if (l.bn == 256)
            return {l.nkb == 8 ? &tn16x_phased_kernel<GATHER_CONV, 256, 8> : &tn16x_phased_kernel<GATHER_CONV, 256, 6>, lds};
        return {l.nkb == 8 ? &tn16x_phased_kernel<GATHER_CONV, 192, 8> : &tn16x_phased_kernel<GATHER_CONV, 192, 6>, lds};
    }
    if (l.kernel == TN16_NARROW) return {conv ? &tn16_kernel<GATHER_CONV> : &tn16_kernel<GATHER_PLAIN>, 4 * TN16_TILE};
    if (l.nbi == 2) return {conv ? &tn16x_kernel<GATHER_CONV, 32, 2> : &tn16x_kernel<GATHER_PLAIN, 32, 2>, 3 * 4 * 32 * 256};
    if (l.bk == 64) return {conv ? &tn16x_kernel<GATHER_CONV, 64> : &tn16x_kernel<GATHER_PLAIN, 64>, 3 * 3 * l.bk * 256};
    return {conv ? &tn16x_kernel<GATHER_CONV, 32> : &tn16x_kernel<GATHER_PLAIN, 32>, 3 * 3 * l.bk * 256};
}
int tn16_launch_lds(const TN16Launch& l) { return tn16_inst(l).lds; }

int launch_tn16(TN16Params& p, const TN16Launch& l, float* final_out, void* ws, hipStream_t s) {
    BG_REQUIRE(p.Ca % 8 == 0 && p.Cb % 8 == 0 && p.g.ld % 8 == 0 && p.b_ld % 8 == 0,
               "bf16-resident wgrad: channel counts must be multiples of 8 (Ca=%d Cb=%d)", p.Ca, p.Cb);
    BG_REQUIRE((reinterpret_cast<uintptr_t>(p.A) & 15) == 0 && (reinterpret_cast<uintptr_t>(p.Bv) & 15) == 0,
               "bf16-resident wgrad: tensors must be 16-byte aligned");
    BG_REQUIRE(l.splitk == 1 || ws != nullptr, "bf16-resident wgrad: not a plan of this launch");
    BG_REQUIRE(l.grid_x > 0 && l.grid_x < (int64_t(1) << 31), "bf16-resident wgrad: grid out of range");
    const int64_t total = (int64_t)p.Mf * p.Cb;
    p.splitk = l.splitk; p.rows_per_split = l.rows_per_split;
    p.out = l.splitk > 1 ? reinterpret_cast<float*>(ws) : final_out;
    p.slab_stride = l.splitk > 1 ? total : 0;
    p.tiles_m = l.tiles_m; p.tiles_n = l.tiles_n;
    p.pow2 = l.pow2; p.wq_shift = l.wq_shift; p.hq_shift = l.hq_shift;
    const TN16Inst k = tn16_inst(l);
    if (!lds_opt_in(reinterpret_cast<const void*>(k.fn), k.lds)) return BG_ERR_LAUNCH;
    if (prof_on()) {
        char name[48];
        tn16_launch_name(l, name, sizeof(name));
        prof_kernel("%s", name);
    }
    hipLaunchKernelGGL(k.fn, dim3((unsigned)l.grid_x), dim3(l.block), k.lds, s, p);
    BG_LAUNCH_CHECK();
    if (l.splitk > 1) {
        launch_slab_reduce(reinterpret_cast<const float*>(ws), final_out, total, l.splitk, total, s);
        BG_LAUNCH_CHECK();
    }
    return BG_OK;
}

}  // namespace bg
