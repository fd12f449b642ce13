// dense_group.hip - grouped launch for small dense projections that share their batch rows.
//
// Reference call site: condition_batch_norm's beta / gamma projections (ops.py:623-624: two fully_connected(z -> C)
// per conditional batch norm, ops.py:163-165 each).  A generator block has two conditional batch norms on the SAME z
// chunk, i.e. four [B, 32 (+ n_labels)] x [K, C] products of ~10 MFLOP: as separate GEMM launches they cost a launch
// each (forward) and three each backward (weight gradient, bias gradient, split-K reduce) - ~190 launches of ~6 us
// per training iteration (round 2 kernel statistics), pure launch and host overhead under strong scaling.
// Here the projections of one block are ONE launch per direction.  fp32 FMA on the vector ALU: the work is far too
// small for a matrix tile to matter; no atomics (each output element is produced by one thread, batch order fixed),
// so the result is reproducible.
#include "common.h"

namespace bg {

constexpr int DG_COLS = 256;      // threads per block = output columns per block
constexpr int DG_ROWS = 8;        // batch rows (forward) / K rows (weight gradient) per block

struct DenseGroupArgs {
    BgDenseItem item[BG_DENSE_GROUP_MAX];
    int32_t tile_start[BG_DENSE_GROUP_MAX + 1];     // first column tile of every item in blockIdx.x
    int32_t n, B;
};

__device__ __forceinline__ int dg_find(const DenseGroupArgs& a, int tile) {
    int j = 0;
    while (j + 1 < a.n && a.tile_start[j + 1] <= tile) ++j;
    return j;
}

// y[b, c] = bias[c] + sum_k x[b, k] w[k, c];  blockIdx.x = (item, column tile), blockIdx.y = strip of DG_ROWS rows
__global__ __launch_bounds__(DG_COLS) void dense_group_fwd_kernel(const DenseGroupArgs a) {
    extern __shared__ float xs[];                      // [DG_ROWS][K]
    const int j = dg_find(a, blockIdx.x);
    const BgDenseItem it = a.item[j];
    const int c = (blockIdx.x - a.tile_start[j]) * DG_COLS + threadIdx.x;
    const int b0 = blockIdx.y * DG_ROWS;
    const int K = it.K;
    for (int e = threadIdx.x; e < DG_ROWS * K; e += DG_COLS) {
        const int r = e / K, k = e - r * K;
        xs[e] = (b0 + r < a.B) ? it.x[(int64_t)(b0 + r) * it.ldx + k] : 0.f;
    }
    __syncthreads();
    if (c >= it.N) return;
    float acc[DG_ROWS];
    const float bv = it.bias ? it.bias[c] : 0.f;
#pragma unroll
    for (int r = 0; r < DG_ROWS; ++r) acc[r] = bv;
    const float* wp = it.w + c;
    for (int k = 0; k < K; ++k) {
        const float wv = wp[(int64_t)k * it.N];
#pragma unroll
        for (int r = 0; r < DG_ROWS; ++r) acc[r] = fmaf(xs[r * K + k], wv, acc[r]);
    }
#pragma unroll
    for (int r = 0; r < DG_ROWS; ++r)
        if (b0 + r < a.B) it.y[(int64_t)(b0 + r) * it.N + c] = acc[r];
}

// dw[k, c] (+)= sum_b x[b, k] dy[b, c]  (blockIdx.y = strip of DG_ROWS values of k);  the strip that holds k = 0 also
// produces db[c] (+)= sum_b dy[b, c].  The batch is walked in chunks of DG_BCH rows staged in LDS.
constexpr int DG_BCH = 64;
__global__ __launch_bounds__(DG_COLS) void dense_group_wgrad_kernel(const DenseGroupArgs a) {
    __shared__ float xs[DG_BCH][DG_ROWS];
    const int j = dg_find(a, blockIdx.x);
    const BgDenseItem it = a.item[j];
    const int c = (blockIdx.x - a.tile_start[j]) * DG_COLS + threadIdx.x;
    const int k0 = blockIdx.y * DG_ROWS;
    if (k0 >= it.K) return;                            // (block-uniform: items of a group may differ in K)
    float acc[DG_ROWS], sb = 0.f;
#pragma unroll
    for (int r = 0; r < DG_ROWS; ++r) acc[r] = 0.f;
    const bool live = c < it.N;
    for (int bb = 0; bb < a.B; bb += DG_BCH) {
        __syncthreads();
        for (int e = threadIdx.x; e < DG_BCH * DG_ROWS; e += DG_COLS) {
            const int b = e / DG_ROWS, r = e - b * DG_ROWS;
            xs[b][r] = (bb + b < a.B && k0 + r < it.K) ? it.x[(int64_t)(bb + b) * it.ldx + k0 + r] : 0.f;
        }
        __syncthreads();
        if (live) {
            const int nb = min(DG_BCH, a.B - bb);
            for (int b = 0; b < nb; ++b) {
                const float g = it.y[(int64_t)(bb + b) * it.N + c];        // (y holds dy in this direction)
                sb += g;
#pragma unroll
                for (int r = 0; r < DG_ROWS; ++r) acc[r] = fmaf(xs[b][r], g, acc[r]);
            }
        }
    }
    if (!live) return;
#pragma unroll
    for (int r = 0; r < DG_ROWS; ++r)
        if (k0 + r < it.K) {
            float* o = it.dw + (int64_t)(k0 + r) * it.N + c;
            *o = it.acc_w ? *o + acc[r] : acc[r];
        }
    if (k0 == 0 && it.db) it.db[c] = it.acc_b ? it.db[c] + sb : sb;
}

// dx[b, k] (+)= sum_i sum_c dy_i[b, c] w_i[k, c] over items that share their input rows (same K).  blockIdx.x = tile of
// DD_K values of k, blockIdx.y = strip of DG_ROWS rows; thread (kk, r) owns one output element and walks the items and
// their columns in a fixed order.  Chunks of DD_C columns of w (padded row: no bank conflicts across kk) and of dy are
// staged in LDS with coalesced loads.
constexpr int DD_K = 32, DD_C = 64;
static_assert(DD_K * DG_ROWS == DG_COLS, "one thread per (k, row) of the tile");
__global__ __launch_bounds__(DG_COLS) void dense_group_dgrad_kernel(const DenseGroupArgs a, float* dx, int64_t lddx,
                                                                    int acc) {
    __shared__ float ws[DD_K][DD_C + 1];
    __shared__ float gs[DG_ROWS][DD_C];
    const int k0 = blockIdx.x * DD_K, b0 = blockIdx.y * DG_ROWS;
    const int kk = threadIdx.x % DD_K, r = threadIdx.x / DD_K;
    const int K = a.item[0].K;
    float s = 0.f;
    for (int i = 0; i < a.n; ++i) {
        const BgDenseItem it = a.item[i];
        const int N = it.N;
        for (int c0 = 0; c0 < N; c0 += DD_C) {
            __syncthreads();
            for (int e = threadIdx.x; e < DD_K * DD_C; e += DG_COLS) {
                const int rr = e / DD_C, cc = e - rr * DD_C;
                ws[rr][cc] = (k0 + rr < K && c0 + cc < N) ? it.w[(int64_t)(k0 + rr) * N + c0 + cc] : 0.f;
            }
            for (int e = threadIdx.x; e < DG_ROWS * DD_C; e += DG_COLS) {
                const int rr = e / DD_C, cc = e - rr * DD_C;
                gs[rr][cc] = (b0 + rr < a.B && c0 + cc < N) ? it.y[(int64_t)(b0 + rr) * N + c0 + cc] : 0.f;
            }
            __syncthreads();
#pragma unroll 16
            for (int cc = 0; cc < DD_C; ++cc) s = fmaf(gs[r][cc], ws[kk][cc], s);
        }
    }
    if (k0 + kk < K && b0 + r < a.B) {
        float* o = dx + (int64_t)(b0 + r) * lddx + k0 + kk;
        *o = acc ? *o + s : s;
    }
}

// ---- latent fan-out / fan-in ----------------------------------------------------------------------------------------
// target t, element (b, c) = sum over the segments routed to t that cover column c (in segment order) of
// src[b, src_col + c - dst_col]; accumulate adds to the old value.  One thread per output element, no atomics.
struct LatentArgs {
    BgLatentTarget tgt[BG_LATENT_MAX_TARGETS];
    BgLatentSeg seg[BG_LATENT_MAX_SEGS];
    int32_t n_tgt, n_seg, B;
};

__global__ __launch_bounds__(256) void latent_route_kernel(const LatentArgs a) {
    const int t = blockIdx.y;
    const BgLatentTarget tg = a.tgt[t];
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (int64_t)a.B * tg.width) return;
    const int b = (int)(e / tg.width), c = (int)(e - (int64_t)b * tg.width);
    float s = 0.f;
    for (int i = 0; i < a.n_seg; ++i) {
        const BgLatentSeg sg = a.seg[i];
        if (sg.target == t && c >= sg.dst_col && c < sg.dst_col + sg.width)
            s += sg.src[(int64_t)b * sg.lds + sg.src_col + (c - sg.dst_col)];
    }
    float* o = tg.dst + (int64_t)b * tg.ldd + c;
    *o = tg.accumulate ? *o + s : s;
}

static int latent_prepare(const void* targets, int n_tgt, const void* segs, int n_seg, int B, LatentArgs& a,
                          const char* who, bool exact_cover) {
    BG_REQUIRE(targets && segs && n_tgt >= 1 && n_tgt <= BG_LATENT_MAX_TARGETS && n_seg >= 1 &&
               n_seg <= BG_LATENT_MAX_SEGS && B >= 1, "%s: 1..%d targets, 1..%d segments and a positive batch", who,
               BG_LATENT_MAX_TARGETS, BG_LATENT_MAX_SEGS);
    memset(&a, 0, sizeof(a));
    const BgLatentTarget* tg = static_cast<const BgLatentTarget*>(targets);
    const BgLatentSeg* sg = static_cast<const BgLatentSeg*>(segs);
    for (int t = 0; t < n_tgt; ++t) {
        BG_REQUIRE(tg[t].dst && tg[t].width >= 1 && tg[t].ldd >= tg[t].width, "%s: target %d: bad operand", who, t);
        a.tgt[t] = tg[t];
    }
    for (int i = 0; i < n_seg; ++i) {
        const BgLatentSeg& s = sg[i];
        BG_REQUIRE(s.src && s.target >= 0 && s.target < n_tgt && s.width >= 1 && s.src_col >= 0 && s.dst_col >= 0 &&
                   s.dst_col + s.width <= tg[s.target].width && s.lds >= s.src_col + s.width,
                   "%s: segment %d: bad operand", who, i);
        a.seg[i] = s;
    }
    if (exact_cover) {          // fan-out: every output column is written by exactly one segment
        for (int t = 0; t < n_tgt; ++t) {
            int64_t cover = 0;
            for (int i = 0; i < n_seg; ++i)
                if (sg[i].target == t) cover += sg[i].width;
            BG_REQUIRE(cover == tg[t].width, "%s: target %d: segments cover %lld of %d columns", who, t,
                       (long long)cover, tg[t].width);
            for (int i = 0; i < n_seg; ++i)
                for (int j = i + 1; j < n_seg; ++j)
                    BG_REQUIRE(sg[i].target != t || sg[j].target != t || sg[i].dst_col + sg[i].width <= sg[j].dst_col ||
                               sg[j].dst_col + sg[j].width <= sg[i].dst_col, "%s: segments %d and %d overlap", who, i, j);
        }
    }
    a.n_tgt = n_tgt;
    a.n_seg = n_seg;
    a.B = B;
    return BG_OK;
}

static int latent_launch(const LatentArgs& a, void* stream) {
    int wmax = 0;
    for (int t = 0; t < a.n_tgt; ++t) wmax = a.tgt[t].width > wmax ? a.tgt[t].width : wmax;
    const int64_t blocks = ((int64_t)a.B * wmax + 255) / 256;
    hipLaunchKernelGGL(latent_route_kernel, dim3((unsigned)blocks, a.n_tgt), dim3(256), 0, as_stream(stream), a);
    BG_LAUNCH_CHECK();
    return BG_OK;
}

static int dg_prepare(const BgDenseItem* items, int n, int B, DenseGroupArgs& a, int* kmax, const char* who, bool bwd) {
    BG_REQUIRE(items && n >= 1 && n <= BG_DENSE_GROUP_MAX && B >= 1, "%s: 1..%d items and a positive batch", who,
               BG_DENSE_GROUP_MAX);
    memset(&a, 0, sizeof(a));
    a.n = n;
    a.B = B;
    int tiles = 0, km = 0;
    for (int i = 0; i < n; ++i) {
        const BgDenseItem& it = items[i];
        BG_REQUIRE(it.x && it.y && it.K >= 1 && it.N >= 1 && it.ldx >= it.K, "%s: item %d: bad operand", who, i);
        BG_REQUIRE(bwd ? it.dw != nullptr : it.w != nullptr, "%s: item %d: null weight operand", who, i);
        a.item[i] = it;
        a.tile_start[i] = tiles;
        tiles += (it.N + DG_COLS - 1) / DG_COLS;
        km = it.K > km ? it.K : km;
    }
    a.tile_start[n] = tiles;
    *kmax = km;
    return BG_OK;
}

}  // namespace bg

using namespace bg;

extern "C" {

int bg_dense_group_fwd(const BgDenseItem* items, int n_items, int B, void* stream) {
    DenseGroupArgs a;
    int kmax = 0;
    int rc = dg_prepare(items, n_items, B, a, &kmax, "bg_dense_group_fwd", false);
    if (rc) return rc;
    const size_t lds = (size_t)DG_ROWS * kmax * sizeof(float);
    BG_REQUIRE(lds <= 48 * 1024, "bg_dense_group_fwd: K = %d is too long for the row strip in LDS", kmax);
    dim3 grid(a.tile_start[a.n], (B + DG_ROWS - 1) / DG_ROWS);
    hipLaunchKernelGGL(dense_group_fwd_kernel, grid, dim3(DG_COLS), lds, as_stream(stream), a);
    BG_LAUNCH_CHECK();
    return BG_OK;
}

int bg_dense_group_wgrad(const BgDenseItem* items, int n_items, int B, void* stream) {
    DenseGroupArgs a;
    int kmax = 0;
    int rc = dg_prepare(items, n_items, B, a, &kmax, "bg_dense_group_wgrad", true);
    if (rc) return rc;
    dim3 grid(a.tile_start[a.n], (kmax + DG_ROWS - 1) / DG_ROWS);
    hipLaunchKernelGGL(dense_group_wgrad_kernel, grid, dim3(DG_COLS), 0, as_stream(stream), a);
    BG_LAUNCH_CHECK();
    return BG_OK;
}

int bg_dense_group_dgrad(const BgDenseItem* items, int n_items, int B, void* dx, int lddx, int accumulate,
                         void* stream) {
    BG_REQUIRE(items && n_items >= 1 && n_items <= BG_DENSE_GROUP_MAX && B >= 1 && dx,
               "bg_dense_group_dgrad: 1..%d items, a positive batch and an output", BG_DENSE_GROUP_MAX);
    DenseGroupArgs a;
    memset(&a, 0, sizeof(a));
    a.n = n_items;
    a.B = B;
    const int K = items[0].K;
    for (int i = 0; i < n_items; ++i) {
        const BgDenseItem& it = items[i];
        BG_REQUIRE(it.w && it.y && it.K == K && K >= 1 && it.N >= 1, "bg_dense_group_dgrad: item %d: bad operand "
                   "(every item needs w, dy in y and the same K)", i);
        a.item[i] = it;
    }
    BG_REQUIRE(lddx >= K, "bg_dense_group_dgrad: lddx %d < K %d", lddx, K);
    dim3 grid((K + DD_K - 1) / DD_K, (B + DG_ROWS - 1) / DG_ROWS);
    hipLaunchKernelGGL(dense_group_dgrad_kernel, grid, dim3(DG_COLS), 0, as_stream(stream), a, static_cast<float*>(dx),
                       (int64_t)lddx, accumulate);
    BG_LAUNCH_CHECK();
    return BG_OK;
}

int bg_latent_fanout(const void* targets, int n_targets, const void* segs, int n_segs, int B, void* stream) {
    LatentArgs a;
    int rc = latent_prepare(targets, n_targets, segs, n_segs, B, a, "bg_latent_fanout", true);
    if (rc) return rc;
    return latent_launch(a, stream);
}

int bg_latent_fanin(const void* targets, int n_targets, const void* segs, int n_segs, int B, void* stream) {
    LatentArgs a;
    int rc = latent_prepare(targets, n_targets, segs, n_segs, B, a, "bg_latent_fanin", false);
    if (rc) return rc;
    return latent_launch(a, stream);
}

}  // extern "C"
