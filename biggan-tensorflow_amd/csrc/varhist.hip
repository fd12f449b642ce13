// varhist.hip - TensorBoard-style histograms of every variable of the model in one launch (utils.py:322-333
// tf.summary.histogram over tf.global_variables(); the bucket rule is TF 1.x core/lib/histogram/histogram.cc).
//
//   items    several hundred fp32 views (arena segments and stand-alone tensors), 1 element to tens of millions each
//   limits   the 1551 bucket limits as doubles, built once on the host and uploaded: the kernel never recomputes one
//   ->  counts [n_items][n_limits] uint32: counts[i][b] = #{ finite x of item i : upper_bound(limits, (double)x) == b }
//       stats  [n_items][6] double: min, max, num, sum, sum_squares over the finite elements, and the non-finite count
//
// Plan (bg_var_hist_plan, host): every item is cut into chunks of at most VH_CHUNK elements, so that no chunk crosses an
// item boundary; the caller uploads the plan once and passes the device copy to every call.
//
// Kernel 1 (var_hist_kernel): a block owns a contiguous range of chunks.  The limits sit in LDS as doubles (12.4 KB) next
// to the block's histogram (6.2 KB).  Per element: a bucket guess from log2|x| (the limits grow by 1.1 per bucket), then
// the guess is walked against the table in double until limits[b-1] <= x < limits[b] holds, which is upper_bound exactly,
// whatever the guess was.  Counts go to the LDS histogram with integer atomics (one add per wave when every lane of the
// wave hits the same bucket: all-zero biases and gammas) and leave the block as global uint32 adds of its non-empty bins
// when the block moves to another item: integer sums do not depend on arrival order.  sum / sum_squares / min / max / num
// are NOT merged with atomics: each chunk writes one partial row, reduced inside the block in a fixed order.
// Kernel 2 (var_hist_finalize_kernel): one wave per item adds the item's partial rows in a fixed order.
// Both are therefore bit-identical from run to run.
//
// Loads: a chunk starts at any 4-byte offset (views of a flat arena), so the block peels scalars up to the first 16-byte
// boundary, reads float4 from there and finishes with scalars; nothing outside [start, start + count) is read.
#include <float.h>

#include "common.h"

namespace bg {

#define VH_BLOCK 256
#define VH_CHUNK 16384            // elements per chunk (64 KB of fp32)
#define VH_MAX_LIMITS 2048
#define VH_MAX_BLOCKS 2048
#define VH_PART 6                 // doubles per partial row: min, max, num, sum, sum_squares, nonfinite

struct VhItem {                   // 24 bytes, plan part 1
    const float* x;
    uint32_t n, chunk0, n_chunks, reserved;
};
struct VhChunk {                  // 16 bytes, plan part 2
    uint32_t item, start, count, reserved;
};
static_assert(sizeof(VhItem) == 24 && sizeof(VhChunk) == 16, "plan layout");

struct VhAcc {
    double sum, sq;
    float mn, mx;
    uint32_t fin, bad;
};

// upper_bound(limits, x) for a finite x: the first index whose limit is strictly greater, in double, against the table.
__device__ __forceinline__ int vh_bucket(float xf, const double* lim, int n_limits, int zero) {
    const double x = (double)xf;
    const float ax = fabsf(xf);
    // limits[zero + 1 + k] = 1e-12 * 1.1^k: k ~ (log2|x| - log2(1e-12)) / log2(1.1); only a starting point
    float t = (__log2f(ax) + 39.863137f) * 7.2725406f;
    t = fminf(fmaxf(t, -1.0f), (float)(zero - 1));
    const int k = (int)floorf(t);
    int b = xf < 0.0f ? zero - 1 - k : zero + 2 + k;
    b = b < 1 ? 1 : (b > n_limits - 1 ? n_limits - 1 : b);
    while (b < n_limits - 1 && lim[b] <= x) ++b;
    while (b > 0 && lim[b - 1] > x) --b;
    return b;
}

__device__ __forceinline__ bool vh_finite(float x) { return (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u; }

// one element of one lane: statistics, and the bucket (or -1 for a non-finite value)
__device__ __forceinline__ int vh_take(float x, VhAcc& a, const double* lim, int n_limits, int zero) {
    if (!vh_finite(x)) {
        ++a.bad;
        return -1;
    }
    const double d = (double)x;
    a.sum += d;
    a.sq += d * d;
    a.mn = fminf(a.mn, x);
    a.mx = fmaxf(a.mx, x);
    ++a.fin;
    return vh_bucket(x, lim, n_limits, zero);
}

__device__ __forceinline__ double vh_wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__global__ __launch_bounds__(VH_BLOCK) void var_hist_kernel(const VhItem* __restrict__ items,
                                                            const VhChunk* __restrict__ chunks, int n_items, int n_chunks,
                                                            int per_block, const double* __restrict__ limits,
                                                            int n_limits, uint32_t* __restrict__ counts,
                                                            double* __restrict__ part) {
    __shared__ double lim[VH_MAX_LIMITS];
    __shared__ uint32_t hist[VH_MAX_LIMITS];
    __shared__ double red[4][VH_PART];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int zero = (n_limits - 1) >> 1;
    for (int i = tid; i < n_limits; i += VH_BLOCK) {
        lim[i] = limits[i];
        hist[i] = 0u;
    }
    __syncthreads();
    const int c0 = blockIdx.x * per_block;
    const int c1 = c0 + per_block < n_chunks ? c0 + per_block : n_chunks;
    for (int c = c0; c < c1; ++c) {
        const VhChunk ch = chunks[c];
        if (ch.item >= (uint32_t)n_items) continue;           // (a plan of another model: count nothing)
        const VhItem it = items[ch.item];
        const float* p = it.x + ch.start;
        const uint32_t count = ch.count;
        VhAcc a;
        a.sum = 0.0; a.sq = 0.0;
        a.mn = __uint_as_float(0x7f800000u);
        a.mx = __uint_as_float(0xff800000u);
        a.fin = 0u; a.bad = 0u;
        // scalars up to the first 16-byte boundary
        uint32_t head = (uint32_t)(((16u - (uint32_t)((uintptr_t)p & 15u)) & 15u) >> 2);
        if (head > count) head = count;
        if ((uint32_t)tid < head) {
            const int b = vh_take(p[tid], a, lim, n_limits, zero);
            if (b >= 0) atomicAdd(&hist[b], 1u);
        }
        // float4 body: trip count uniform over the block, so that the wave-wide votes below are convergent
        const uint32_t nvec = (count - head) >> 2;
        const float4* pv = reinterpret_cast<const float4*>(p + head);
        for (uint32_t base = 0; base < nvec; base += VH_BLOCK) {
            const uint32_t i = base + tid;
            const bool valid = i < nvec;
            int b0 = -1, b1 = -1, b2 = -1, b3 = -1;
            if (valid) {
                const float4 v = pv[i];
                b0 = vh_take(v.x, a, lim, n_limits, zero);
                b1 = vh_take(v.y, a, lim, n_limits, zero);
                b2 = vh_take(v.z, a, lim, n_limits, zero);
                b3 = vh_take(v.w, a, lim, n_limits, zero);
            }
            // every lane of the wave in one and the same bucket (a constant tensor): one add for the wave
            const int first = __shfl(b0, 0, 64);
            const bool same = valid && b0 >= 0 && b0 == first && b1 == first && b2 == first && b3 == first;
            if (__all(same)) {
                if (lane == 0) atomicAdd(&hist[first], 256u);
            } else {
                if (b0 >= 0) atomicAdd(&hist[b0], 1u);
                if (b1 >= 0) atomicAdd(&hist[b1], 1u);
                if (b2 >= 0) atomicAdd(&hist[b2], 1u);
                if (b3 >= 0) atomicAdd(&hist[b3], 1u);
            }
        }
        // scalar tail
        const uint32_t done = head + (nvec << 2);
        if (done + (uint32_t)tid < count) {
            const int b = vh_take(p[done + tid], a, lim, n_limits, zero);
            if (b >= 0) atomicAdd(&hist[b], 1u);
        }
        // the chunk's partial row, reduced in a fixed order: lanes by xor shuffles, then waves 0..3
        double r[VH_PART];
        r[0] = (double)a.mn; r[1] = (double)a.mx; r[2] = (double)a.fin; r[3] = a.sum; r[4] = a.sq; r[5] = (double)a.bad;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            r[0] = fmin(r[0], __shfl_xor(r[0], o, 64));
            r[1] = fmax(r[1], __shfl_xor(r[1], o, 64));
        }
        r[2] = vh_wave_sum(r[2]);
        r[3] = vh_wave_sum(r[3]);
        r[4] = vh_wave_sum(r[4]);
        r[5] = vh_wave_sum(r[5]);
        if (lane == 0) {
#pragma unroll
            for (int j = 0; j < VH_PART; ++j) red[wave][j] = r[j];
        }
        __syncthreads();                                       // (also: every LDS histogram add of this chunk is done)
        if (tid == 0) {
            double* o = part + (size_t)c * VH_PART;
            o[0] = fmin(fmin(red[0][0], red[1][0]), fmin(red[2][0], red[3][0]));
            o[1] = fmax(fmax(red[0][1], red[1][1]), fmax(red[2][1], red[3][1]));
#pragma unroll
            for (int j = 2; j < VH_PART; ++j) o[j] = ((red[0][j] + red[1][j]) + red[2][j]) + red[3][j];
        }
        // leave the block's counts when the next chunk belongs to another item (or to another block)
        const bool flush = c + 1 >= c1 || chunks[c + 1].item != ch.item;
        if (flush) {
            uint32_t* dst = counts + (size_t)ch.item * n_limits;
            for (int i = tid; i < n_limits; i += VH_BLOCK) {
                const uint32_t v = hist[i];
                if (v) {
                    atomicAdd(&dst[i], v);
                    hist[i] = 0u;
                }
            }
        }
        __syncthreads();                                       // red[] and hist[] are free for the next chunk
    }
}

// one wave per item: lane l adds the partial rows chunk0 + l, chunk0 + l + 64, ... in that order, then an xor tree
__global__ __launch_bounds__(64) void var_hist_finalize_kernel(const VhItem* __restrict__ items, int n_items,
                                                               const double* __restrict__ part,
                                                               double* __restrict__ stats) {
    const int item = blockIdx.x;
    if (item >= n_items) return;
    const VhItem it = items[item];
    double mn = __longlong_as_double(0x7ff0000000000000LL), mx = -mn, num = 0.0, sum = 0.0, sq = 0.0, bad = 0.0;
    for (uint32_t c = threadIdx.x; c < it.n_chunks; c += 64) {
        const double* r = part + (size_t)(it.chunk0 + c) * VH_PART;
        mn = fmin(mn, r[0]);
        mx = fmax(mx, r[1]);
        num += r[2];
        sum += r[3];
        sq += r[4];
        bad += r[5];
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        mn = fmin(mn, __shfl_xor(mn, o, 64));
        mx = fmax(mx, __shfl_xor(mx, o, 64));
    }
    num = vh_wave_sum(num);
    sum = vh_wave_sum(sum);
    sq = vh_wave_sum(sq);
    bad = vh_wave_sum(bad);
    if (threadIdx.x == 0) {
        double* o = stats + (size_t)item * VH_PART;
        o[0] = num > 0.0 ? mn : DBL_MAX;                       // TF's Histogram::Clear(): min = DBL_MAX, max = -DBL_MAX
        o[1] = num > 0.0 ? mx : -DBL_MAX;
        o[2] = num;
        o[3] = sum;
        o[4] = sq;
        o[5] = bad;
    }
}

static int64_t vh_chunks_of(int64_t n) { return (n + VH_CHUNK - 1) / VH_CHUNK; }

// total chunks, or -1 (with the error set)
static int64_t vh_count_chunks(const BgHistItem* items, int n_items, const char* who) {
    if (!items || n_items <= 0) {
        set_error("%s: items=%p n_items=%d", who, (const void*)items, n_items);
        return -1;
    }
    int64_t total = 0;
    for (int i = 0; i < n_items; ++i) {
        const int64_t n = items[i].n;
        if (n < 0 || n >= ((int64_t)1 << 32)) {
            set_error("%s: item %d has n=%lld (0 <= n < 2^32 per item)", who, i, (long long)n);
            return -1;
        }
        if (n > 0 && (!items[i].x || ((uintptr_t)items[i].x & 3) != 0)) {
            set_error("%s: item %d: pointer %p is NULL or not 4-byte aligned", who, i, (const void*)items[i].x);
            return -1;
        }
        total += vh_chunks_of(n);
    }
    if (total > 0x7fffffff) {
        set_error("%s: %lld chunks", who, (long long)total);
        return -1;
    }
    return total;
}

}  // namespace bg

using namespace bg;

extern "C" {

int bg_var_hist_plan_chunks(const BgHistItem* items, int n_items, int* n_chunks) {
    BG_REQUIRE(n_chunks, "bg_var_hist_plan_chunks: NULL n_chunks");
    const int64_t total = vh_count_chunks(items, n_items, "bg_var_hist_plan_chunks");
    if (total < 0) return BG_ERR_ARG;
    *n_chunks = (int)total;
    return BG_OK;
}

size_t bg_var_hist_plan_bytes(int n_items, int n_chunks) {
    if (n_items <= 0 || n_chunks < 0) return 0;
    return (size_t)n_items * sizeof(VhItem) + (size_t)n_chunks * sizeof(VhChunk);
}

int bg_var_hist_plan(const BgHistItem* items, int n_items, void* plan, size_t plan_bytes) {
    const int64_t total = vh_count_chunks(items, n_items, "bg_var_hist_plan");
    if (total < 0) return BG_ERR_ARG;
    BG_REQUIRE(plan && ((uintptr_t)plan & 7) == 0, "bg_var_hist_plan: plan must be a non-NULL 8-byte aligned host buffer");
    BG_REQUIRE(plan_bytes >= bg_var_hist_plan_bytes(n_items, (int)total), "bg_var_hist_plan: plan_bytes=%zu < %zu",
               plan_bytes, bg_var_hist_plan_bytes(n_items, (int)total));
    VhItem* pi = reinterpret_cast<VhItem*>(plan);
    VhChunk* pc = reinterpret_cast<VhChunk*>(pi + n_items);
    uint32_t c = 0;
    for (int i = 0; i < n_items; ++i) {
        const int64_t n = items[i].n;
        pi[i].x = items[i].x;
        pi[i].n = (uint32_t)n;
        pi[i].chunk0 = c;
        pi[i].n_chunks = (uint32_t)vh_chunks_of(n);
        pi[i].reserved = 0;
        for (int64_t s = 0; s < n; s += VH_CHUNK, ++c) {
            pc[c].item = (uint32_t)i;
            pc[c].start = (uint32_t)s;
            pc[c].count = (uint32_t)(n - s < VH_CHUNK ? n - s : VH_CHUNK);
            pc[c].reserved = 0;
        }
    }
    return BG_OK;
}

size_t bg_var_hist_workspace_bytes(int n_items, int n_chunks) {
    if (n_items <= 0 || n_chunks < 0) return 0;
    return ((size_t)n_chunks + 1) * VH_PART * sizeof(double);
}

int bg_var_hist(const void* plan, int n_items, int n_chunks, const double* limits, int n_limits, uint32_t* counts,
                double* stats, void* ws, size_t ws_bytes, void* stream) {
    BG_REQUIRE(n_items > 0 && n_chunks >= 0, "bg_var_hist: n_items=%d n_chunks=%d", n_items, n_chunks);
    BG_REQUIRE(plan && limits && counts && stats && ws, "bg_var_hist: NULL plan, limits, counts, stats or workspace");
    BG_REQUIRE(n_limits >= 3 && n_limits <= VH_MAX_LIMITS && (n_limits & 1) == 1,
               "bg_var_hist: n_limits=%d (odd, 3 to %d: negative limits, 0, positive limits)", n_limits, VH_MAX_LIMITS);
    BG_REQUIRE(((uintptr_t)plan & 7) == 0 && ((uintptr_t)limits & 7) == 0 && ((uintptr_t)stats & 7) == 0 &&
               ((uintptr_t)ws & 7) == 0 && ((uintptr_t)counts & 3) == 0, "bg_var_hist: misaligned buffer");
    BG_REQUIRE(ws_bytes >= bg_var_hist_workspace_bytes(n_items, n_chunks), "bg_var_hist: ws_bytes=%zu < %zu", ws_bytes,
               bg_var_hist_workspace_bytes(n_items, n_chunks));
    hipStream_t s = as_stream(stream);
    const VhItem* items = reinterpret_cast<const VhItem*>(plan);
    const VhChunk* chunks = reinterpret_cast<const VhChunk*>(items + n_items);
    double* part = reinterpret_cast<double*>(ws);
    if (zero_async(counts, (size_t)n_items * n_limits * sizeof(uint32_t), s) != hipSuccess) {
        set_error("bg_var_hist: cannot zero counts");
        (void)hipGetLastError();
        return BG_ERR_LAUNCH;
    }
    if (n_chunks > 0) {
        int blocks = n_chunks < VH_MAX_BLOCKS ? n_chunks : VH_MAX_BLOCKS;
        const int per_block = (n_chunks + blocks - 1) / blocks;
        blocks = (n_chunks + per_block - 1) / per_block;
        hipLaunchKernelGGL(var_hist_kernel, dim3(blocks), dim3(VH_BLOCK), 0, s, items, chunks, n_items, n_chunks,
                           per_block, limits, n_limits, counts, part);
        BG_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(var_hist_finalize_kernel, dim3(n_items), dim3(64), 0, s, items, n_items, part, stats);
    BG_LAUNCH_CHECK();
    return BG_OK;
}

}  // extern "C"
