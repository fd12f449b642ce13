// labels.hip - labelled datasets: the sliced label loss of --cls_loss_type (utils.py:339-375) and the row gather that
// draws the generator's fake labels from the dataset's label table (BigGAN.py:1447-1455).  gfx950 only.
//
// The tensors are tiny ([256, 1000] at most in a BASELINE-like run), so the work is launch-bound: the loss is two
// launches (per-slice sums, then loss + dlogits) with the cross-rank all-reduce of the per-slice sums between them, and
// nothing is read back.  The slice description lives in device memory (uploaded once when the loss is built): no
// kernel reads host memory after its launcher returns.
#include "common.h"

namespace bg {

constexpr int LB_BLOCK = 256;
constexpr int LB_ROW_CHUNKS = 8;       // pass 1: row chunks per column tile (blockIdx.y)
constexpr int LB_KIND_LOGISTIC = 0, LB_KIND_EUCLIDEAN = 1;

__device__ __forceinline__ int clamp_slice(int s, int n_slices) { return s < 0 ? 0 : (s >= n_slices ? n_slices - 1 : s); }

// ------------------------------------------------------------------------------------------
// pass 1: sums[s] += sum over this rank's rows and the columns of slice s of
//   logistic : sigmoid_cross_entropy_with_logits(t, x) * w = (max(x,0) - x t + log1p(exp(-|x|))) * w
//   euclidean: ((x - t) * w)^2
// One thread per column (coalesced rows), fp32 terms accumulated in fp64.  The columns of a slice are contiguous, so
// a wave reduces each run of equal slice indices with a segmented shuffle scan and its first lane adds the run's sum:
// at most one fp64 atomic per (wave, slice) in each of the up to LB_ROW_CHUNKS row chunks.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(LB_BLOCK) void label_loss_sums_kernel(const float* __restrict__ x, const float* __restrict__ t,
                                                                   const float* __restrict__ w,
                                                                   const int32_t* __restrict__ slices,
                                                                   const int32_t* __restrict__ col_slice,
                                                                   double* __restrict__ sums, int B, int n, int n_slices) {
    const int j = blockIdx.x * LB_BLOCK + threadIdx.x;
    int s = -1;
    double acc = 0.0;
    if (j < n) {
        s = clamp_slice(col_slice[j], n_slices);
        const int kind = slices[2 * s];
        const float wj = w[j];
        for (int b = blockIdx.y; b < B; b += gridDim.y) {
            const int64_t i = (int64_t)b * n + j;
            const float xi = x[i], ti = t[i];
            if (kind == LB_KIND_EUCLIDEAN) {
                const float d = (xi - ti) * wj;
                acc += (double)d * (double)d;
            } else {
                const float e = expf(-fabsf(xi));
                acc += (double)((fmaxf(xi, 0.f) - xi * ti + log1pf(e)) * wj);
            }
        }
    }
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const double v = __shfl_down(acc, o, 64);
        const int so = __shfl_down(s, o, 64);
        if (lane + o < 64 && so == s) acc += v;
    }
    const int sp = __shfl_up(s, 1, 64);
    if (s >= 0 && (lane == 0 || sp != s)) atomicAdd(&sums[s], acc);
}

// ------------------------------------------------------------------------------------------
// pass 2 (sums now hold the GLOBAL batch): block 0 writes
//   loss = loss_weight * sum_s (logistic: sums[s] / (rows_global * size_s); euclidean: sqrt(sums[s]))
// and every block writes its share of
//   dlogits[b,j] = loss_weight * w_j * (sigmoid(x) - t) / (rows_global * size_s)     logistic
//                = loss_weight * w_j^2 * (x - t) / sqrt(sums[s])                     euclidean, 0 where sums[s] == 0
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(LB_BLOCK) void label_loss_finish_kernel(const float* __restrict__ x, const float* __restrict__ t,
                                                                     const float* __restrict__ w,
                                                                     const int32_t* __restrict__ slices,
                                                                     const int32_t* __restrict__ col_slice,
                                                                     const double* __restrict__ sums, double rows_global,
                                                                     float loss_weight, float* __restrict__ loss_out,
                                                                     float* __restrict__ dx, int B, int n, int n_slices) {
    if (blockIdx.x == 0) {
        __shared__ double sh[LB_BLOCK];
        double acc = 0.0;
        for (int s = threadIdx.x; s < n_slices; s += LB_BLOCK) {
            const double v = sums[s];
            if (slices[2 * s] == LB_KIND_EUCLIDEAN)
                acc += sqrt(v);
            else
                acc += v / (rows_global * (double)max(slices[2 * s + 1], 1));
        }
        sh[threadIdx.x] = acc;
        __syncthreads();
        for (int o = LB_BLOCK / 2; o > 0; o >>= 1) {          // fixed tree: the same value on every run
            if (threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
            __syncthreads();
        }
        if (threadIdx.x == 0) *loss_out = (float)((double)loss_weight * sh[0]);
    }
    const int64_t total = (int64_t)B * n;
    for (int64_t i = (int64_t)blockIdx.x * LB_BLOCK + threadIdx.x; i < total; i += (int64_t)gridDim.x * LB_BLOCK) {
        const int j = (int)(i % n);
        const int s = clamp_slice(col_slice[j], n_slices);
        const float xi = x[i], ti = t[i], wj = w[j];
        if (slices[2 * s] == LB_KIND_EUCLIDEAN) {
            const double ss = sums[s];
            const float c = ss > 0.0 ? (float)((double)loss_weight / sqrt(ss)) : 0.f;
            dx[i] = ((xi - ti) * wj) * wj * c;
        } else {
            const float c = (float)((double)loss_weight / (rows_global * (double)max(slices[2 * s + 1], 1)));
            const float e = expf(-fabsf(xi));
            const float sig = xi >= 0.f ? 1.f / (1.f + e) : e / (1.f + e);
            dx[i] = (sig - ti) * (wj * c);
        }
    }
}

// out[b, :] = table[idx[b], :] (32-bit words moved as they are); an index outside the table is clamped into it
__global__ __launch_bounds__(LB_BLOCK) void gather_rows_kernel(const uint32_t* __restrict__ table,
                                                               const int64_t* __restrict__ idx, uint32_t* __restrict__ out,
                                                               int rows, int n, int B) {
    const int64_t total = (int64_t)B * n;
    for (int64_t i = (int64_t)blockIdx.x * LB_BLOCK + threadIdx.x; i < total; i += (int64_t)gridDim.x * LB_BLOCK) {
        const int64_t b = i / n;
        const int c = (int)(i - b * n);
        int64_t r = idx[b];
        r = r < 0 ? 0 : (r >= rows ? rows - 1 : r);
        out[i] = table[r * n + c];
    }
}

static inline unsigned elementwise_blocks(int64_t total) {
    int64_t blocks = (total + LB_BLOCK - 1) / LB_BLOCK;
    return (unsigned)(blocks > 2048 ? 2048 : blocks);
}

}  // namespace bg

using namespace bg;

extern "C" {

int bg_label_loss_sums(const float* logits, const float* truth, const float* weights, const int32_t* slices,
                       const int32_t* col_slice, double* sums, int B, int n, int n_slices, void* stream) {
    BG_REQUIRE(logits && truth && weights && slices && col_slice && sums, "bg_label_loss_sums: NULL tensor");
    BG_REQUIRE(B > 0 && n > 0 && n_slices > 0 && n_slices <= n, "bg_label_loss_sums: bad argument");
    // col_slice is trusted to be non-decreasing (utils.cls_loss_fn builds it from the slice sizes): the kernel clamps an
    // index into range, which keeps every access in bounds, but a map out of order would give wrong sums
    const dim3 grid((n + LB_BLOCK - 1) / LB_BLOCK, B < LB_ROW_CHUNKS ? B : LB_ROW_CHUNKS);
    hipLaunchKernelGGL(label_loss_sums_kernel, grid, dim3(LB_BLOCK), 0, as_stream(stream), logits, truth, weights, slices,
                       col_slice, sums, B, n, n_slices);
    BG_LAUNCH_CHECK();
    return BG_OK;
}

int bg_label_loss_finish(const float* logits, const float* truth, const float* weights, const int32_t* slices,
                         const int32_t* col_slice, const double* sums, double rows_global, float loss_weight,
                         float* loss_out, float* dlogits, int B, int n, int n_slices, void* stream) {
    BG_REQUIRE(logits && truth && weights && slices && col_slice && sums && loss_out && dlogits,
               "bg_label_loss_finish: NULL tensor");
    BG_REQUIRE(B > 0 && n > 0 && n_slices > 0 && n_slices <= n && rows_global >= (double)B,
               "bg_label_loss_finish: bad argument");
    hipLaunchKernelGGL(label_loss_finish_kernel, dim3(elementwise_blocks((int64_t)B * n)), dim3(LB_BLOCK), 0,
                       as_stream(stream), logits, truth, weights, slices, col_slice, sums, rows_global, loss_weight,
                       loss_out, dlogits, B, n, n_slices);
    BG_LAUNCH_CHECK();
    return BG_OK;
}

int bg_gather_rows(const float* table, const int64_t* idx, float* out, int rows, int n, int B, void* stream) {
    BG_REQUIRE(table && idx && out, "bg_gather_rows: NULL tensor");
    BG_REQUIRE(rows > 0 && n > 0 && B > 0, "bg_gather_rows: bad argument");
    hipLaunchKernelGGL(gather_rows_kernel, dim3(elementwise_blocks((int64_t)B * n)), dim3(LB_BLOCK), 0,
                       as_stream(stream), reinterpret_cast<const uint32_t*>(table), idx,
                       reinterpret_cast<uint32_t*>(out), rows, n, B);
    BG_LAUNCH_CHECK();
    return BG_OK;
}

}  // extern "C"
