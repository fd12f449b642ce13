// rowdist.h - the squared distances of a tile of queries to the set rows of a block: the one row walker of the search
// kernel (nearest.hip, which writes the [Q, N] matrix) and of the precision / recall / density / coverage kernels
// (prdc.hip, which keep one or two numbers per set row and never write it).  d(q, s) = sum_j (q_j - s_j)^2 over bf16 rows
// of D elements, D a multiple of 64.
//
// Arithmetic.  bf16 is widened exactly, the difference is taken in fp32 and one fma per term adds its square.  The
// distance is not expanded into |q|^2 + |s|^2 - 2 q.s and there is no MFMA: for a near-copy d << |q|^2, and the expansion
// cancels exactly where the answer matters.  Equal rows give 0.0f.
//
// Tiling.  A block of RD_BLOCK = 256 threads owns RD_ROWS = 16 set rows, RD_RW = 4 per wave (rd_rows: rows past N repeat
// row N - 1; the caller does not store them).  Per tile of RD_QT = 8 queries and per chunk of RD_DC = 2048 elements the
// block stages the queries' chunk in LDS (32 KiB, rows of 4 KiB), a query past Q as zeros read from row 0 (not stored
// either); the eight staging loads of a thread are issued before its first LDS store.  Every wave then walks the chunk 512
// elements a turn: lane l holds elements [8 l, 8 l + 8) of its four rows from one 16-byte global load each, reads the
// same 16 bytes of each query from LDS (lane-contiguous, so every 16-lane group of a ds_read_b128 covers the 64 banks
// once) and adds into 8 x 4 accumulators of two floats (even and odd elements: v_pk_add_f32 / v_pk_fma_f32).  LDS bytes
// are RD_QT / RD_RW = 2 x the HBM bytes.  Lanes past the end of a chunk (D is a multiple of 64, not of 512) take zeros for
// both operands.  The rows' 16 bytes of the NEXT turn are loaded while this turn is computed (RowsAhead): with 16 rows a
// block a few thousand rows leave one or two waves per SIMD, and nothing else hides a global load per turn.
//
// Order.  After the last chunk the 32 sums of a lane go through a transposing butterfly: at lane distance 32, 16, 8, 4, 2 a
// lane keeps one half of its values and adds to each the partner's counterpart of the other half, and one step at
// distance 1 finishes: 32 shuffles, d(query slot i, row r) in the lane pair l >> 1 = 4 i + r.  The order of summation
// depends on the element index alone (the elements of one lane in sequence, then a balanced tree over lanes whose
// additions commute), so d(a, b) and d(b, a) are the same bits, whichever kernel made them.  Every sum is made by one
// wave in one order: no atomics, no partial sums across blocks, and a repeated launch gives the same bits.
#pragma once
#include "common.h"

namespace bg {

#define RD_BLOCK 256
#define RD_QT 8                      // queries per tile
#define RD_RW 4                      // set rows per wave
#define RD_ROWS (4 * RD_RW)          // set rows per block
#define RD_DC 2048                   // elements of a query row staged per pass

typedef float rd_f2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ void rd_unpack(const uint4& w, rd_f2 (&v)[4]) {       // bf16 pairs, widened exactly
    v[0] = rd_f2{__uint_as_float(w.x << 16), __uint_as_float(w.x & 0xffff0000u)};
    v[1] = rd_f2{__uint_as_float(w.y << 16), __uint_as_float(w.y & 0xffff0000u)};
    v[2] = rd_f2{__uint_as_float(w.z << 16), __uint_as_float(w.z & 0xffff0000u)};
    v[3] = rd_f2{__uint_as_float(w.w << 16), __uint_as_float(w.w & 0xffff0000u)};
}

// one step of the transposing butterfly: HALF values stay, each plus the partner lane's counterpart of the other half
template <int HALF>
__device__ __forceinline__ void rd_fold(float (&v)[RD_QT * RD_RW], int lane) {
    constexpr int dist = HALF == 16 ? 32 : HALF == 8 ? 16 : HALF == 4 ? 8 : HALF == 2 ? 4 : 2;
    const bool hi = (lane & dist) != 0;
#pragma unroll
    for (int i = 0; i < HALF; ++i) {
        const float keep = hi ? v[i + HALF] : v[i];
        const float send = hi ? v[i] : v[i + HALF];
        v[i] = keep + __shfl_xor(send, dist, 64);
    }
}

// the wave's rows of the block whose first row is row0
__device__ __forceinline__ void rd_rows(const uint16_t* set, int64_t N, int D, int64_t row0, const uint16_t* (&rows)[RD_RW]) {
#pragma unroll
    for (int r = 0; r < RD_RW; ++r) {
        const int64_t n = row0 + r < N ? row0 + r : N - 1;      // rows past the end repeat the last one; not stored
        rows[r] = set + n * D;
    }
}

// What a lane holds ahead of its use: the 16 bytes of its four rows for the NEXT turn of the walk.  The chain runs on
// across chunks and tiles; the rows are the same for every tile, so after the last chunk it wraps to their first.  16
// registers: the kernels stay at two waves per SIMD (holding the next chunk of the queries as well costs 32 more and the
// second wave; measured slower at 8192 rows).  Prefetching changes no arithmetic and no order.
struct RowsAhead {
    uint4 s[RD_RW];
};

// the wave's rows at elements [c0 + o, c0 + o + 8); zeros past the end of the chunk
__device__ __forceinline__ void rd_fetch_rows(RowsAhead& a, const uint16_t* const (&rows)[RD_RW], int D, int c0, int o) {
    const int len = D - c0 < RD_DC ? D - c0 : RD_DC;
#pragma unroll
    for (int r = 0; r < RD_RW; ++r) {
        a.s[r] = uint4{0u, 0u, 0u, 0u};
        if (o < len) a.s[r] = *reinterpret_cast<const uint4*>(rows[r] + c0 + o);
    }
}

__device__ __forceinline__ void rd_prologue(RowsAhead& a, const uint16_t* const (&rows)[RD_RW], int D, int lane) {
    rd_fetch_rows(a, rows, D, 0, lane * 8);
}

// The squared distances of the query tile [q0, q0 + RD_QT) to the wave's four rows.  Every thread of the block calls it
// (it holds the barriers of the staging).  Returns d(q0 + i, rows[r]) for i = lane >> 3, r = (lane >> 1) & 3; the two
// lanes of a pair hold the same value.  Queries past Q are zeros.  ``a`` holds this tile's first turn on entry
// (rd_prologue, or the previous call) and the next tile's on return.
__device__ __forceinline__ float rd_tile(RowsAhead& a, const uint16_t* __restrict__ q, int64_t q0, int64_t Q,
                                         const uint16_t* const (&rows)[RD_RW], int D, int t, int lane) {
    __shared__ __attribute__((aligned(16))) uint16_t qs[RD_QT * RD_DC];      // the tile's chunk of the queries, rows of 4 KiB
    rd_f2 acc[RD_QT][RD_RW];
#pragma unroll
    for (int i = 0; i < RD_QT; ++i)
#pragma unroll
        for (int r = 0; r < RD_RW; ++r) acc[i][r] = rd_f2{0.0f, 0.0f};
    for (int c0 = 0; c0 < D; c0 += RD_DC) {
        const int len = D - c0 < RD_DC ? D - c0 : RD_DC;        // a multiple of 8
        __syncthreads();                                        // the previous chunk has been read
        if (t * 8 < len) {                                      // RD_DC = 8 RD_BLOCK: one piece of every query per thread
            uint4 w[RD_QT];                                     // all eight loads are in flight before the first store
#pragma unroll
            for (int i = 0; i < RD_QT; ++i)
                w[i] = *reinterpret_cast<const uint4*>(q + (q0 + i < Q ? q0 + i : 0) * (int64_t)D + c0 + t * 8);
            __builtin_amdgcn_sched_barrier(0);                  // (or the scheduler waits for the first before the fourth)
#pragma unroll
            for (int i = 0; i < RD_QT; ++i)                     // queries past the end are zeros
                *reinterpret_cast<uint4*>(&qs[i * RD_DC + t * 8]) = q0 + i < Q ? w[i] : uint4{0u, 0u, 0u, 0u};
        }
        __syncthreads();
        for (int o = lane * 8; o < len + lane * 8; o += 512) {  // every lane of the wave makes the same number of turns
            const bool in = o < len;
            rd_f2 sv[RD_RW][4];
#pragma unroll
            for (int r = 0; r < RD_RW; ++r) rd_unpack(a.s[r], sv[r]);
            if (o + 512 < len + lane * 8)                       // the next turn; after the last, the next chunk's first
                rd_fetch_rows(a, rows, D, c0, o + 512);
            else
                rd_fetch_rows(a, rows, D, c0 + RD_DC < D ? c0 + RD_DC : 0, lane * 8);
#pragma unroll
            for (int i = 0; i < RD_QT; ++i) {
                uint4 w = uint4{0u, 0u, 0u, 0u};
                if (in) w = *reinterpret_cast<const uint4*>(&qs[i * RD_DC + o]);
                rd_f2 qv[4];
                rd_unpack(w, qv);
#pragma unroll
                for (int r = 0; r < RD_RW; ++r)
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const rd_f2 d = qv[j] - sv[r][j];
                        acc[i][r] = __builtin_elementwise_fma(d, d, acc[i][r]);
                    }
            }
        }
    }
    float v[RD_QT * RD_RW];
#pragma unroll
    for (int i = 0; i < RD_QT; ++i)
#pragma unroll
        for (int r = 0; r < RD_RW; ++r) v[i * RD_RW + r] = acc[i][r].x + acc[i][r].y;
    rd_fold<16>(v, lane);
    rd_fold<8>(v, lane);
    rd_fold<4>(v, lane);
    rd_fold<2>(v, lane);
    rd_fold<1>(v, lane);
    return v[0] + __shfl_xor(v[0], 1, 64);
}

}  // namespace bg
