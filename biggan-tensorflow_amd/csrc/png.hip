// png.hip - PNG row filtering and DEFLATE on the device, so that a sample grid (BigGAN.py:1125-1230) or a strip of the
// sampling service (BigGAN.py:1298-1369) leaves the device as the compressed bytes of its IDAT chunk instead of as pixels
// for zlib on the host.  Opt-in (BG_DEVICE_PNG=1, png.py); the format is in DESIGN.md "Device-side PNG encoding".
//
//   png_filter        one workgroup per image row: the five filter costs sum |(int8)residual| are block reductions, the
//                     lowest type with the smallest cost wins, the row is written as 1 + row_bytes bytes.
//   deflate_segments  one workgroup per segment (<= 32 KiB, staged in LDS), no match reaches outside the segment:
//                       tokens   literals and distance-1 matches of 3..258 bytes.  A run of equal bytes [s, e) is its
//                                first byte as a literal and the other R = e-s-1 bytes cut into pieces of 258; a run or a
//                                piece shorter than 3 is literals.  A position's token is a function of (s, e) alone, so
//                                every thread derives the tokens of its own chunk of positions: s and e across chunk borders
//                                come from two block scans of the per-chunk first / last run break.
//                       code     histogram by LDS integer atomics, rank sort by (count, symbol) in parallel, then lane 0:
//                                two-queue Huffman, depth counts clamped to 15 (7 for the code-length code) and repaired to
//                                a complete code by Kraft sum, lengths handed out in sorted order, canonical codes.
//                       bits     per-thread bit totals -> exclusive block scan -> every token is OR-ed into the LDS image
//                                of the block at its own bit offset (32-bit LDS atomicOr: order-free, so the bytes do not
//                                depend on scheduling).
//                       a stored block is written instead whenever it is not larger.
//   deflate_compact   one block scans the segment sizes, one block per segment gathers its slot into the contiguous
//                     output; per-stream (offset, bytes) pairs are written for the host.
// Three walks over the chunk (histogram, bit count, emission) recompute the tokens instead of keeping them: the LDS holds
// the segment, the block image and small tables only.  Chunks are 4 * odd bytes long, so that the 64 lanes of a wave read
// their chunks from different LDS banks.
#include "common.h"

namespace bg {

#define PF_BLOCK 256
#define PF_MAX_ROW (1 << 24)          // cost <= 128 * row_bytes stays inside int32
#define DF_BLOCK 256
#define DF_MAX_SEG 32768
#define DF_NLL 286                    // literal/length symbols
#define DF_NCL 19
#define DF_SLACK 16                   // bytes of the LDS block image past seg_bytes (trailer of a barely smaller block)
#define DF_ADLER 65521u

// ---------------------------------------------------------------------------------------------------------------------
// filter
// ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int pf_abs8(int r) {
    const int s = (int)(int8_t)(r & 255);
    return s < 0 ? -s : s;
}
__device__ __forceinline__ int pf_paeth(int a, int b, int c) {
    const int p = a + b - c;
    const int pa = abs(p - a), pb = abs(p - b), pc = abs(p - c);
    return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}
__device__ __forceinline__ int pf_residual(int type, int x, int a, int b, int c) {
    switch (type) {
        case 0: return x;
        case 1: return x - a;
        case 2: return x - b;
        case 3: return x - ((a + b) >> 1);
        default: return x - pf_paeth(a, b, c);
    }
}

// grid (max_h, n): block (row, image).  An entry is used only if the whole image fits both arenas.
__global__ __launch_bounds__(PF_BLOCK) void png_filter_kernel(const uint8_t* __restrict__ src, int64_t src_bytes,
                                                              const BgPngImage* __restrict__ table, int bpp,
                                                              uint8_t* __restrict__ dst, int64_t dst_bytes) {
    __shared__ int sh_cost[5][PF_BLOCK / 64];
    const BgPngImage e = table[blockIdx.y];
    const int row = blockIdx.x;
    if (e.h < 1 || e.h > (int)gridDim.x || e.row_bytes < 1 || e.row_bytes > PF_MAX_ROW || e.src_offset < 0 ||
        e.dst_offset < 0)
        return;
    const int64_t in_ext = (int64_t)e.h * e.row_bytes, out_ext = (int64_t)e.h * ((int64_t)e.row_bytes + 1);
    if (in_ext > src_bytes || e.src_offset > src_bytes - in_ext || out_ext > dst_bytes || e.dst_offset > dst_bytes - out_ext)
        return;
    if (row >= e.h) return;
    const int rb = e.row_bytes;
    const uint8_t* cur = src + e.src_offset + (int64_t)row * rb;
    const uint8_t* up = cur - rb;
    const bool has_up = row > 0;
    int cost[5] = {0, 0, 0, 0, 0};
    for (int i = threadIdx.x; i < rb; i += PF_BLOCK) {
        const int x = cur[i];
        const int a = i >= bpp ? cur[i - bpp] : 0;
        const int b = has_up ? up[i] : 0;
        const int c = (has_up && i >= bpp) ? up[i - bpp] : 0;
#pragma unroll
        for (int t = 0; t < 5; ++t) cost[t] += pf_abs8(pf_residual(t, x, a, b, c));
    }
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int t = 0; t < 5; ++t) {
        int v = cost[t];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
        if (lane == 0) sh_cost[t][w] = v;
    }
    __syncthreads();
    int best = 0, best_cost = 0;
#pragma unroll
    for (int t = 0; t < 5; ++t) {
        int v = 0;
#pragma unroll
        for (int k = 0; k < PF_BLOCK / 64; ++k) v += sh_cost[t][k];
        if (t == 0 || v < best_cost) {                        // ties go to the lowest type
            best = t;
            best_cost = v;
        }
    }
    uint8_t* out = dst + e.dst_offset + (int64_t)row * ((int64_t)rb + 1);
    if (threadIdx.x == 0) out[0] = (uint8_t)best;
    for (int i = threadIdx.x; i < rb; i += PF_BLOCK) {
        const int x = cur[i];
        const int a = i >= bpp ? cur[i - bpp] : 0;
        const int b = has_up ? up[i] : 0;
        const int c = (has_up && i >= bpp) ? up[i - bpp] : 0;
        out[1 + i] = (uint8_t)pf_residual(best, x, a, b, c);
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// deflate
// ---------------------------------------------------------------------------------------------------------------------
struct DfShared {
    uint32_t freq[288];               // literal/length counts
    uint32_t w[2 * 288];              // Huffman node weights (lane 0)
    uint16_t parent[2 * 288];         // Huffman parents, then depths (lane 0)
    uint16_t order[288];              // used symbols by ascending (count, symbol)
    uint16_t code[288];               // bit-reversed canonical codes
    uint16_t seq[320];                // code-length symbols of the header: symbol | extra << 5
    uint8_t len[288];                 // code lengths
    uint8_t cl_len[DF_NCL + 1];
    uint16_t cl_code[DF_NCL + 1];
    int scan[2][DF_BLOCK];
    int carry[DF_BLOCK];              // run start handed to each chunk
    int next_break[DF_BLOCK];         // first run break behind each chunk
    uint32_t n_used, dfreq, adler_a, adler_b;
    uint32_t hdr_bits, n_seq, hlit, hclen, body_bits;
};

struct DfMax { __device__ int operator()(int a, int b) const { return a > b ? a : b; } };
struct DfMin { __device__ int operator()(int a, int b) const { return a < b ? a : b; } };
struct DfAdd { __device__ int operator()(int a, int b) const { return a + b; } };

// inclusive scan over the block's threads; every thread gets its value.  Ends with the scan buffers free for reuse.
template <typename Op>
__device__ int df_scan_incl(int v, int (*sh)[DF_BLOCK], Op op) {
    const int t = threadIdx.x;
    int cur = 0;
    __syncthreads();
    sh[0][t] = v;
    __syncthreads();
    for (int o = 1; o < DF_BLOCK; o <<= 1) {
        int a = sh[cur][t];
        if (t >= o) a = op(sh[cur][t - o], a);
        sh[cur ^ 1][t] = a;
        cur ^= 1;
        __syncthreads();
    }
    const int r = sh[cur][t];
    __syncthreads();
    return r;
}

// length 3..258 -> length code 0..28 and its extra bits
__device__ __forceinline__ void df_len_code(int L, int& code, int& nextra, int& extra) {
    if (L == 258) {
        code = 28; nextra = 0; extra = 0;
        return;
    }
    const int v = L - 3;
    if (v < 8) {
        code = v; nextra = 0; extra = 0;
        return;
    }
    const int e = 29 - __clz(v);                              // floor(log2 v) - 2
    code = 4 * e + 4 + ((v >> e) & 3);
    nextra = e;
    extra = v & ((1 << e) - 1);
}

// The tokens of positions [lo, hi) of x[0:len].  s0: start of the run that holds lo (used when lo is no run break);
// next_break: the first run break at or behind hi (len if none).  lit(byte), match(length) are called in stream order.
template <typename Lit, typename Match>
__device__ __forceinline__ void df_walk(const uint8_t* x, int lo, int hi, int s0, int next_break, Lit lit, Match match) {
    if (lo >= hi) return;
    int i = lo;
    int s = (lo == 0 || x[lo] != x[lo - 1]) ? lo : s0;
    while (i < hi) {
        int j = i + 1;
        while (j < hi && x[j] == x[j - 1]) ++j;
        const int e = j < hi ? j : next_break;                // the run is [s, e)
        const int stop = e < hi ? e : hi;
        const int R = e - s - 1;
        const int byte = x[i];
        int p = i;
        while (p < stop) {
            const int k = p - s;
            if (k == 0 || R < 3) {
                lit(byte);
                ++p;
                continue;
            }
            const int m = k - 1, q = m / 258, r = m - q * 258;
            const int rest = R - q * 258;
            const int L = rest < 258 ? rest : 258;
            if (L < 3) {
                lit(byte);
                ++p;
            } else if (r == 0) {
                match(L);
                p += L;
            } else {
                p += L - r;                                   // inside a match that an earlier chunk started
            }
        }
        i = stop;
        s = e;
    }
}

// OR nbits (<= 32) of value into the little-endian bit image at bit position pos
__device__ __forceinline__ void df_put(uint32_t* img, uint32_t pos, uint32_t value, int nbits) {
    if (nbits == 0) return;
    const uint64_t v = (uint64_t)value << (pos & 31);
    const uint32_t lo = (uint32_t)v, hi = (uint32_t)(v >> 32);
    if (lo) atomicOr(&img[pos >> 5], lo);
    if (hi) atomicOr(&img[(pos >> 5) + 1], hi);
}

__device__ __forceinline__ uint32_t df_reverse(uint32_t code, int nbits) { return __brev(code) >> (32 - nbits); }

// Lane 0.  order[0:n] (n >= 2): the used symbols by ascending (count, symbol); count(order[i]) in sh.w[i].  Writes
// len_out[symbol] <= maxbits for them: a complete prefix code, optimal when no depth exceeds maxbits.
__device__ void df_build_lengths(DfShared& sh, const uint16_t* order, int n, int maxbits, uint8_t* len_out) {
    int leaf = 0, inner = n;
    for (int next = n; next < 2 * n - 1; ++next) {
        int pick[2];
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            if (leaf < n && (inner >= next || sh.w[leaf] <= sh.w[inner])) pick[k] = leaf++;
            else pick[k] = inner++;
        }
        sh.w[next] = sh.w[pick[0]] + sh.w[pick[1]];
        sh.parent[pick[0]] = sh.parent[pick[1]] = (uint16_t)next;
    }
    int count[16];
#pragma unroll
    for (int b = 0; b < 16; ++b) count[b] = 0;
    sh.parent[2 * n - 2] = 0;                                 // parents become depths, root first
    for (int node = 2 * n - 3; node >= 0; --node) {
        const int d = sh.parent[sh.parent[node]] + 1;
        sh.parent[node] = (uint16_t)d;
        if (node < n) count[d < maxbits ? d : maxbits]++;
    }
    // Kraft sum in units of 2^-maxbits: clamping made it too large; lengthen the deepest codes below maxbits until it
    // is not, then shorten from the deepest level while the code is incomplete.
    int64_t kraft = 0;
    for (int b = 1; b <= maxbits; ++b) kraft += (int64_t)count[b] << (maxbits - b);
    const int64_t full = (int64_t)1 << maxbits;
    while (kraft > full) {
        int b = maxbits - 1;
        while (count[b] == 0) --b;
        count[b]--;
        count[b + 1]++;
        kraft -= (int64_t)1 << (maxbits - b - 1);
    }
    while (kraft < full) {
        int b = maxbits;
        while (count[b] == 0) --b;                            // nothing deeper: the deficit is a multiple of 2^(maxbits-b)
        count[b]--;
        count[b - 1]++;
        kraft += (int64_t)1 << (maxbits - b);
    }
    int idx = 0;
    for (int b = maxbits; b >= 1; --b)
        for (int c = 0; c < count[b]; ++c) len_out[order[idx++]] = (uint8_t)b;
}

// Lane 0: canonical codes of len[0:nsym], bit-reversed for LSB-first output.
template <typename CodeT>
__device__ void df_assign_codes(const uint8_t* len, int nsym, CodeT* code) {
    int count[16], next[16];
#pragma unroll
    for (int b = 0; b < 16; ++b) count[b] = 0;
    for (int s = 0; s < nsym; ++s) count[len[s]]++;
    count[0] = 0;
    int c = 0;
    next[0] = 0;
    for (int b = 1; b < 16; ++b) {
        c = (c + count[b - 1]) << 1;
        next[b] = c;
    }
    for (int s = 0; s < nsym; ++s) {
        const int b = len[s];
        code[s] = b ? (CodeT)df_reverse((uint32_t)next[b]++, b) : (CodeT)0;
    }
}

__constant__ uint8_t df_cl_order[DF_NCL] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

// Lane 0: literal/length code, the header's code-length sequence and its code; everything the bit count needs.
__device__ void df_build_codes(DfShared& sh) {
    const int n = (int)sh.n_used;
    for (int i = 0; i < n; ++i) sh.w[i] = sh.freq[sh.order[i]];
    df_build_lengths(sh, sh.order, n, 15, sh.len);            // n >= 2: a byte and the end-of-block symbol
    df_assign_codes(sh.len, DF_NLL, sh.code);
    int hlit = DF_NLL;
    while (hlit > 257 && sh.len[hlit - 1] == 0) --hlit;
    const int dlen = sh.dfreq ? 1 : 0;                        // one distance code: 1 bit when used, length zero when not
    const int total = hlit + 1;
    auto length_at = [&](int i) { return i < hlit ? (int)sh.len[i] : dlen; };
    uint32_t cl_freq[DF_NCL];
#pragma unroll
    for (int s = 0; s < DF_NCL; ++s) cl_freq[s] = 0;
    int n_seq = 0;
    auto emit = [&](int sym, int extra) {
        sh.seq[n_seq++] = (uint16_t)(sym | (extra << 5));
        cl_freq[sym]++;
    };
    for (int i = 0; i < total;) {
        const int v = length_at(i);
        int run = 1;
        while (i + run < total && length_at(i + run) == v) ++run;
        int r = run;
        if (v == 0) {
            while (r >= 3) {
                const int t = r > 138 ? 138 : r;
                if (t >= 11) emit(18, t - 11);
                else emit(17, t - 3);
                r -= t;
            }
            while (r-- > 0) emit(0, 0);
        } else {
            emit(v, 0);
            --r;
            while (r >= 3) {
                const int t = r > 6 ? 6 : r;
                emit(16, t - 3);
                r -= t;
            }
            while (r-- > 0) emit(v, 0);
        }
        i += run;
    }
    // code-length code: insertion sort of the used symbols by (count, symbol), at least two of them
    uint16_t* cl_order = sh.order;                            // the literal/length order is no longer needed
    int cn = 0;
    for (int s = 0; s < DF_NCL; ++s) {
        sh.cl_len[s] = 0;
        if (cl_freq[s] == 0) continue;
        int k = cn++;
        while (k > 0 && cl_freq[cl_order[k - 1]] > cl_freq[s]) {
            cl_order[k] = cl_order[k - 1];
            --k;
        }
        cl_order[k] = (uint16_t)s;
    }
    if (cn == 1) {                                            // a code of one symbol must still be complete
        const uint16_t other = cl_order[0] == 0 ? 1 : 0;
        cl_order[1] = cl_order[0];
        cl_order[0] = other;
        cn = 2;
    }
    for (int i = 0; i < cn; ++i) sh.w[i] = cl_freq[cl_order[i]];
    df_build_lengths(sh, cl_order, cn, 7, sh.cl_len);
    df_assign_codes(sh.cl_len, DF_NCL, sh.cl_code);
    int hclen = DF_NCL;
    while (hclen > 4 && sh.cl_len[df_cl_order[hclen - 1]] == 0) --hclen;
    uint32_t bits = 5 + 5 + 4 + 3 * hclen;
    for (int i = 0; i < n_seq; ++i) {
        const int sym = sh.seq[i] & 31;
        bits += sh.cl_len[sym] + (sym == 16 ? 2 : sym == 17 ? 3 : sym == 18 ? 7 : 0);
    }
    sh.hdr_bits = bits;
    sh.n_seq = (uint32_t)n_seq;
    sh.hlit = (uint32_t)hlit;
    sh.hclen = (uint32_t)hclen;
}

// Lane 0: the dynamic block's header behind the 3 block bits.
__device__ void df_emit_header(DfShared& sh, uint32_t* img, uint32_t pos) {
    df_put(img, pos, sh.hlit - 257, 5); pos += 5;
    df_put(img, pos, 0, 5); pos += 5;                         // HDIST = 1 code
    df_put(img, pos, sh.hclen - 4, 4); pos += 4;
    for (uint32_t i = 0; i < sh.hclen; ++i) {
        df_put(img, pos, sh.cl_len[df_cl_order[i]], 3);
        pos += 3;
    }
    for (uint32_t i = 0; i < sh.n_seq; ++i) {
        const int sym = sh.seq[i] & 31, extra = sh.seq[i] >> 5;
        df_put(img, pos, sh.cl_code[sym], sh.cl_len[sym]);
        pos += sh.cl_len[sym];
        const int nx = sym == 16 ? 2 : sym == 17 ? 3 : sym == 18 ? 7 : 0;
        df_put(img, pos, (uint32_t)extra, nx);
        pos += nx;
    }
}

// One workgroup per segment.  Dynamic LDS: the segment (seg_bytes), then the block image (seg_bytes + DF_SLACK).
__global__ __launch_bounds__(DF_BLOCK) void deflate_segments_kernel(const uint8_t* __restrict__ src, int64_t src_bytes,
                                                                    const BgDeflateSeg* __restrict__ table, int seg_bytes,
                                                                    uint8_t* __restrict__ dst, int64_t dst_bytes,
                                                                    int32_t* __restrict__ records) {
    extern __shared__ __attribute__((aligned(16))) uint8_t df_lds[];
    __shared__ DfShared sh;
    uint8_t* x = df_lds;
    uint32_t* img = reinterpret_cast<uint32_t*>(df_lds + seg_bytes);
    const int t = threadIdx.x;
    const BgDeflateSeg g = table[blockIdx.x];
    int32_t* rec = records + 4 * (int64_t)blockIdx.x;
    const int len = g.len;
    const int64_t bound = (int64_t)len + 16;                  // bg_deflate_bound
    if (len < 1 || len > seg_bytes || g.src_offset < 0 || g.src_offset > src_bytes - len || g.dst_offset < 0 ||
        bound > dst_bytes || g.dst_offset > dst_bytes - bound) {
        if (t == 0) {
            rec[0] = 0; rec[1] = 1; rec[2] = 0; rec[3] = -1;
        }
        return;
    }
    const uint8_t* in = src + g.src_offset;
    uint8_t* out = dst + g.dst_offset;
    const bool last = g.last != 0;

    // stage the segment; clear the tables
    if ((reinterpret_cast<uintptr_t>(in) & 3) == 0) {
        const uint32_t* in4 = reinterpret_cast<const uint32_t*>(in);
        uint32_t* x4 = reinterpret_cast<uint32_t*>(x);
        for (int i = t; i < len / 4; i += DF_BLOCK) x4[i] = in4[i];
        for (int i = (len & ~3) + t; i < len; i += DF_BLOCK) x[i] = in[i];
    } else {
        for (int i = t; i < len; i += DF_BLOCK) x[i] = in[i];
    }
    for (int i = t; i < 288; i += DF_BLOCK) {
        sh.freq[i] = 0;
        sh.len[i] = 0;
    }
    if (t == 0) sh.n_used = sh.dfreq = sh.adler_a = sh.adler_b = 0;
    __syncthreads();

    // chunk of this thread: 4 * odd bytes (bank-conflict-free byte walks)
    int c4 = (len + 4 * DF_BLOCK - 1) / (4 * DF_BLOCK);
    c4 |= 1;
    const int chunk = 4 * c4;
    const int lo = (int64_t)t * chunk < len ? t * chunk : len;
    const int hi = lo + chunk < len ? lo + chunk : len;

    // Adler-32 of the segment on its own, and the first / last run break of the chunk
    {
        uint32_t s1 = 0, s2 = 0;                              // s2 <= 132 * 32768 * 255 < 2^31
        int first = len, lastb = -1;
        for (int p = lo; p < hi; ++p) {
            const uint32_t v = x[p];
            s1 += v;
            s2 += (uint32_t)(len - p) * v;
            if (p == 0 || x[p] != x[p - 1]) {
                if (first == len) first = p;
                lastb = p;
            }
        }
        if (lo < hi) {
            atomicAdd(&sh.adler_a, s1);
            atomicAdd(&sh.adler_b, s2 % DF_ADLER);
        }
        const int incl = df_scan_incl(lastb, sh.scan, DfMax());
        sh.carry[t] = incl;
        // suffix minimum: scan over the reversed thread order
        sh.next_break[t] = first;
        __syncthreads();
        const int rmin = df_scan_incl(sh.next_break[DF_BLOCK - 1 - t], sh.scan, DfMin());
        __syncthreads();
        sh.next_break[DF_BLOCK - 1 - t] = rmin;               // inclusive: min over threads >= this one
        __syncthreads();
    }
    const int s0 = t > 0 ? sh.carry[t - 1] : 0;
    const int nb = t + 1 < DF_BLOCK ? sh.next_break[t + 1] : len;

    // walk 1: histogram
    df_walk(x, lo, hi, s0, nb,
            [&](int byte) { atomicAdd(&sh.freq[byte], 1u); },
            [&](int L) {
                int code, nx, ex;
                df_len_code(L, code, nx, ex);
                atomicAdd(&sh.freq[257 + code], 1u);
                atomicAdd(&sh.dfreq, 1u);
            });
    if (t == 0) atomicAdd(&sh.freq[256], 1u);
    __syncthreads();

    // rank sort of the used symbols by (count, symbol)
    for (int s = t; s < DF_NLL; s += DF_BLOCK) {
        const uint32_t f = sh.freq[s];
        if (f == 0) continue;
        int rank = 0;
        for (int j = 0; j < DF_NLL; ++j) {
            const uint32_t fj = sh.freq[j];
            rank += (fj != 0 && (fj < f || (fj == f && j < s))) ? 1 : 0;
        }
        sh.order[rank] = (uint16_t)s;
        atomicAdd(&sh.n_used, 1u);
    }
    __syncthreads();
    if (t == 0) df_build_codes(sh);
    __syncthreads();

    // walk 2: bits of this chunk's tokens
    uint32_t my_bits = 0;
    df_walk(x, lo, hi, s0, nb,
            [&](int byte) { my_bits += sh.len[byte]; },
            [&](int L) {
                int code, nx, ex;
                df_len_code(L, code, nx, ex);
                my_bits += sh.len[257 + code] + nx + 1;
            });
    const uint32_t incl_bits = (uint32_t)df_scan_incl((int)my_bits, sh.scan, DfAdd());
    if (t == DF_BLOCK - 1) sh.body_bits = incl_bits;
    __syncthreads();
    const uint32_t body_bits = sh.body_bits;
    const uint32_t block_bits = 3 + sh.hdr_bits + body_bits + sh.len[256];
    const uint32_t dyn_bytes = (block_bits + 7) >> 3, stored_bytes = 5 + (uint32_t)len;
    const uint32_t adler_a = (1u + sh.adler_a) % DF_ADLER;
    const uint32_t adler_b = ((uint32_t)len + sh.adler_b) % DF_ADLER;

    if (dyn_bytes >= stored_bytes) {
        // stored block: header, the bytes, and on every segment but the last the empty stored block
        for (int i = t; i < len; i += DF_BLOCK) out[5 + i] = x[i];
        if (t == 0) {
            out[0] = last ? 1 : 0;
            out[1] = (uint8_t)(len & 255);
            out[2] = (uint8_t)(len >> 8);
            out[3] = (uint8_t)(~len & 255);
            out[4] = (uint8_t)((~len >> 8) & 255);
            int n = 5 + len;
            if (!last) {
                out[n] = 0; out[n + 1] = 0; out[n + 2] = 0; out[n + 3] = 0xFF; out[n + 4] = 0xFF;
                n += 5;
            }
            rec[0] = n; rec[1] = (int32_t)adler_a; rec[2] = (int32_t)adler_b; rec[3] = 0;
        }
        return;
    }

    // dynamic block into the LDS image
    const int img_words = (seg_bytes + DF_SLACK) / 4;
    for (int i = t; i < img_words; i += DF_BLOCK) img[i] = 0;
    __syncthreads();
    const uint32_t body0 = 3 + sh.hdr_bits;
    uint32_t pos = body0 + incl_bits - my_bits;
    df_walk(x, lo, hi, s0, nb,
            [&](int byte) {
                df_put(img, pos, sh.code[byte], sh.len[byte]);
                pos += sh.len[byte];
            },
            [&](int L) {
                int code, nx, ex;
                df_len_code(L, code, nx, ex);
                const int sym = 257 + code;
                df_put(img, pos, sh.code[sym], sh.len[sym]);
                pos += sh.len[sym];
                df_put(img, pos, (uint32_t)ex, nx);
                pos += nx + 1;                                // the distance code of distance 1 is one 0 bit
            });
    // end of block, then BFINAL's padding or the empty stored block 000 + padding + 00 00 FF FF
    uint32_t end_bits = block_bits;
    if (!last) end_bits = ((end_bits + 3 + 7) & ~7u) + 32;
    const uint32_t nbytes = (end_bits + 7) >> 3;
    if (t == 0) {
        df_put(img, 0, (last ? 1u : 0u) | (2u << 1), 3);
        df_emit_header(sh, img, 3);
        df_put(img, body0 + body_bits, sh.code[256], sh.len[256]);
        if (!last) df_put(img, end_bits - 16, 0xFFFFu, 16);
        rec[0] = (int32_t)nbytes; rec[1] = (int32_t)adler_a; rec[2] = (int32_t)adler_b; rec[3] = 1;
    }
    __syncthreads();
    if ((reinterpret_cast<uintptr_t>(out) & 3) == 0) {
        uint32_t* out4 = reinterpret_cast<uint32_t*>(out);
        for (uint32_t i = t; i < nbytes / 4; i += DF_BLOCK) out4[i] = img[i];
        const uint8_t* img8 = reinterpret_cast<const uint8_t*>(img);
        for (uint32_t i = (nbytes & ~3u) + t; i < nbytes; i += DF_BLOCK) out[i] = img8[i];
    } else {
        const uint8_t* img8 = reinterpret_cast<const uint8_t*>(img);
        for (uint32_t i = t; i < nbytes; i += DF_BLOCK) out[i] = img8[i];
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// compaction
// ---------------------------------------------------------------------------------------------------------------------
// One block: seg_off[i] = sum of the sizes before segment i (seg_off[n] the total); totals[k] = (offset, bytes) of stream
// k, a stream ending at every segment with last != 0.
__global__ __launch_bounds__(DF_BLOCK) void deflate_scan_kernel(const BgDeflateSeg* __restrict__ table,
                                                                const int32_t* __restrict__ records, int n,
                                                                int64_t* __restrict__ seg_off, int64_t* __restrict__ totals,
                                                                int n_streams) {
    __shared__ int scan[2][DF_BLOCK];
    const int t = threadIdx.x;
    int64_t carry = 0;
    int streams = 0;
    for (int base = 0; base < n; base += DF_BLOCK) {
        const int i = base + t;
        int v = 0, l = 0;
        if (i < n) {
            v = records[4 * (int64_t)i];
            v = v > 0 ? v : 0;
            l = table[i].last != 0 ? 1 : 0;
        }
        const int incl = df_scan_incl(v, scan, DfAdd());      // <= 256 * (32768 + 16)
        const int lincl = df_scan_incl(l, scan, DfAdd());
        if (i < n) {
            seg_off[i] = carry + incl - v;
            const int k = streams + lincl - 1;
            if (l && k < n_streams) totals[2 * (int64_t)k + 1] = carry + incl;       // the stream's end, for now
        }
        scan[0][t] = incl;
        scan[1][t] = lincl;
        __syncthreads();
        carry += scan[0][DF_BLOCK - 1];
        streams += scan[1][DF_BLOCK - 1];
        __syncthreads();
    }
    if (t == 0) seg_off[n] = carry;
    __syncthreads();
    // ends -> (offset, bytes), highest streams first: a pass reads only ends that no earlier pass rewrote
    const int have = streams < n_streams ? streams : n_streams;
    for (int top = have; top > 0; top -= DF_BLOCK) {
        const int k = top - 1 - t;
        int64_t end = 0, begin = 0;
        if (k >= 0) {
            end = totals[2 * (int64_t)k + 1];
            begin = k > 0 ? totals[2 * (int64_t)(k - 1) + 1] : 0;
        }
        __syncthreads();
        if (k >= 0) {
            totals[2 * (int64_t)k] = begin;
            totals[2 * (int64_t)k + 1] = end - begin;
        }
        __syncthreads();
    }
    for (int k = have + t; k < n_streams; k += DF_BLOCK) {
        totals[2 * (int64_t)k] = carry;
        totals[2 * (int64_t)k + 1] = 0;
    }
}

__global__ __launch_bounds__(DF_BLOCK) void deflate_gather_kernel(const uint8_t* __restrict__ slots, int64_t slots_bytes,
                                                                  const BgDeflateSeg* __restrict__ table,
                                                                  const int32_t* __restrict__ records,
                                                                  const int64_t* __restrict__ seg_off,
                                                                  uint8_t* __restrict__ out, int64_t out_bytes) {
    const int i = blockIdx.x;
    const int64_t n = records[4 * (int64_t)i];
    const int64_t from = table[i].dst_offset, to = seg_off[i];
    if (n <= 0 || from < 0 || n > slots_bytes || from > slots_bytes - n || to < 0 || n > out_bytes || to > out_bytes - n)
        return;
    const uint8_t* s = slots + from;
    uint8_t* d = out + to;
    for (int64_t b = threadIdx.x; b < n; b += DF_BLOCK) d[b] = s[b];
}

}  // namespace bg

using namespace bg;

extern "C" {

size_t bg_deflate_bound(int len) { return len > 0 ? (size_t)len + 16 : 16; }

int bg_png_filter(const uint8_t* src, int64_t src_bytes, const BgPngImage* table, int n, int max_h, int bpp, uint8_t* dst,
                  int64_t dst_bytes, void* stream) {
    BG_REQUIRE(src && table && dst, "bg_png_filter: NULL pointer");
    BG_REQUIRE(n > 0 && n <= 65535, "bg_png_filter: n=%d (1..65535 images)", n);
    BG_REQUIRE(max_h > 0 && max_h <= (1 << 20), "bg_png_filter: max_h=%d", max_h);
    BG_REQUIRE(bpp == 1 || bpp == 3 || bpp == 4, "bg_png_filter: bpp=%d (1, 3 or 4)", bpp);
    BG_REQUIRE(src_bytes > 0 && dst_bytes > 0, "bg_png_filter: src_bytes=%lld dst_bytes=%lld", (long long)src_bytes,
               (long long)dst_bytes);
    BG_REQUIRE(((uintptr_t)table & 7) == 0, "bg_png_filter: table must be 8-byte aligned");
    hipLaunchKernelGGL(png_filter_kernel, dim3(max_h, n), dim3(PF_BLOCK), 0, as_stream(stream), src, src_bytes, table, bpp,
                       dst, dst_bytes);
    BG_LAUNCH_CHECK();
    return BG_OK;
}

int bg_deflate_segments(const uint8_t* src, int64_t src_bytes, const BgDeflateSeg* table, int n_segs, int seg_bytes,
                        uint8_t* dst, int64_t dst_bytes, int32_t* records, void* stream) {
    BG_REQUIRE(src && table && dst && records, "bg_deflate_segments: NULL pointer");
    BG_REQUIRE(n_segs > 0, "bg_deflate_segments: n_segs=%d", n_segs);
    BG_REQUIRE(seg_bytes >= 256 && seg_bytes <= DF_MAX_SEG && (seg_bytes & (seg_bytes - 1)) == 0,
               "bg_deflate_segments: seg_bytes=%d (a power of two from 256 to 32768)", seg_bytes);
    BG_REQUIRE(src_bytes > 0 && dst_bytes > 0, "bg_deflate_segments: src_bytes=%lld dst_bytes=%lld", (long long)src_bytes,
               (long long)dst_bytes);
    BG_REQUIRE(((uintptr_t)table & 7) == 0 && ((uintptr_t)records & 3) == 0,
               "bg_deflate_segments: table must be 8-byte and records 4-byte aligned");
    if (!lds_opt_in((const void*)deflate_segments_kernel, 2 * DF_MAX_SEG + DF_SLACK)) return BG_ERR_LAUNCH;
    const size_t lds = (size_t)2 * seg_bytes + DF_SLACK;
    hipLaunchKernelGGL(deflate_segments_kernel, dim3(n_segs), dim3(DF_BLOCK), lds, as_stream(stream), src, src_bytes, table,
                       seg_bytes, dst, dst_bytes, records);
    BG_LAUNCH_CHECK();
    return BG_OK;
}

int bg_deflate_compact(const uint8_t* slots, int64_t slots_bytes, const BgDeflateSeg* table, const int32_t* records,
                       int n_segs, uint8_t* out, int64_t out_bytes, int64_t* seg_off, int64_t* totals, int n_streams,
                       void* stream) {
    BG_REQUIRE(slots && table && records && out && seg_off && totals, "bg_deflate_compact: NULL pointer");
    BG_REQUIRE(n_segs > 0 && n_streams > 0 && n_streams <= n_segs, "bg_deflate_compact: n_segs=%d n_streams=%d", n_segs,
               n_streams);
    BG_REQUIRE(slots_bytes > 0 && out_bytes > 0, "bg_deflate_compact: slots_bytes=%lld out_bytes=%lld",
               (long long)slots_bytes, (long long)out_bytes);
    BG_REQUIRE(((uintptr_t)table & 7) == 0 && ((uintptr_t)records & 3) == 0 && ((uintptr_t)seg_off & 7) == 0 &&
                   ((uintptr_t)totals & 7) == 0,
               "bg_deflate_compact: table, seg_off and totals must be 8-byte and records 4-byte aligned");
    hipStream_t s = as_stream(stream);
    hipLaunchKernelGGL(deflate_scan_kernel, dim3(1), dim3(DF_BLOCK), 0, s, table, records, n_segs, seg_off, totals,
                       n_streams);
    hipLaunchKernelGGL(deflate_gather_kernel, dim3(n_segs), dim3(DF_BLOCK), 0, s, slots, slots_bytes, table, records,
                       (const int64_t*)seg_off, out, out_bytes);
    BG_LAUNCH_CHECK();
    return BG_OK;
}

}  // extern "C"
