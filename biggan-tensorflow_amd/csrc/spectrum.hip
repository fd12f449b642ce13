// spectrum.hip - the top singular values of every weight of a network at once (spectrum.py, --sv_freq): the diagnostic
// of Brock et al. 2019 (sigma_0, sigma_1, sigma_2 of each weight over training).  Block (subspace) power iteration on
// W^T W with a basis of BG_SV_BLOCK = 8 vectors per weight, then a Rayleigh-Ritz step; DESIGN.md has the derivation,
// tests/sv_ref.py restates the algorithm in float64.
//
// An item is a weight W[rows][cols] (fp32, row-major) with its basis Q[cols][8] (fp32, orthonormal columns, in / out).
// b_eff = min(8, rows, cols); basis columns >= b_eff are zero and their outputs are 0.  Launches per call, whatever the
// number of items: 3 * iters + 5.
//
//   begin        one block per item: zeroes the item's header and Z, and the basis columns >= b_eff
//   project   A  Y[rows][8] = W Q: W read once, 8 fp32 accumulators per row (the spectral-norm row-dot widened to 8
//                vectors, 8 rows per wave so that the basis is read once per 8 rows); Y is kept as fp64 holding the fp32 sums, so that the second pass multiplies exactly
//   backproj  B  Z[cols][8] += W^T Y: the second read of W, units of 256 rows x 256 columns spread over the items by
//                size, the unit's rows of Y staged in LDS, fp64 products and sums, one fp64 atomic per (column, vector)
//                and unit
//   orth      C  one block per item: Z -> Q in fp64.  Where the 8 x 8 Gram matrix is well conditioned, Cholesky QR twice (three
//                passes over Z); otherwise classical Gram-Schmidt with one re-orthogonalisation (three passes
//                per column: dots; subtract + dots of the result; subtract + remaining norm).  A column whose remaining
//                squared norm is at most 2^-80 of its squared norm before the projections, or that is zero or not
//                finite, becomes a zero column: no NaN or Inf is ever written.  Leaves Z zeroed for the next pass B.
//   ritz         after the last iteration and one more pass A: H = Y^T Y (8 x 8, fp64, summed in a fixed order), cyclic
//                Jacobi in fp64 on its leading b_eff x b_eff block, eigenvalues sorted descending, sv = sqrt(max(l, 0));
//                Q and Y are rotated to the Ritz vectors
//   resid        after one more pass B: resid[i] = || W^T (W q_i) - l_i q_i ||_2 / l_0 (0 when l_0 = 0)
//
// Pass B's unit is 256 rows tall (the spectral-norm column sum uses 64): per 256 x 256 elements of W (256 KB read) it
// adds 256 x 8 fp64 values (16 KB), a sixteenth of the bytes it reads, so the atomics stay well under the streaming time
// at the ~1.3 TB/s measured for float atomics.  The alternative, a two-stage reduce, needs a second launch and a partial
// buffer of rows / 64 x cols x 8 doubles per item.
//
// NOT bit-reproducible: the arrival order of pass B's fp64 atomics differs from launch to launch, so Z, Q, sv and resid
// can differ in their last bits between two calls on the same inputs.
#include <cmath>

#include "common.h"

namespace bg {

#define SV_BLOCK 256
#define SV_GRID 2048
#define SV_TAIL 512           // threads of the orthonormalisation, one block per item (up to 88 fp64 values per thread)
#define SV_RITZ 512           // threads of the Ritz and residual kernels, one block per item (36 fp64 sums per thread)
#define SV_ROWS_B 256         // rows per unit of pass B
#define SV_UNIT_ELEMS_A 65536 // 256 KB of W per block of pass A
#define SV_HDR 80             // doubles ahead of Z: [0, 64) the Ritz rotation, [64, 72) lambda, [72, 80) unused
#define SV_B BG_SV_BLOCK
#define SV_NH 36                // upper triangle of an 8 x 8 Gram matrix

static_assert(BG_SV_BLOCK == 8, "the kernels are written for a basis of 8 vectors");

__host__ __device__ inline size_t sv_need(int rows, int cols) {
    return 8 * ((size_t)SV_HDR + (size_t)SV_B * (size_t)cols + (size_t)SV_B * (size_t)rows);
}

struct SvView {
    double* hdr;   // [SV_HDR]
    double* z;     // [cols][8]
    double* y;     // [rows][8]
    int beff;
};

// false: the item's geometry or scratch does not fit; every kernel then leaves the item alone
__device__ __forceinline__ bool sv_view(const BgSvItem& it, char* ws, size_t ws_bytes, SvView* v) {
    if (it.rows < 1 || it.cols < 1 || it.ws_offset < 0 || (it.ws_offset & 15) || !it.w || !it.q || !it.sv || !it.resid)
        return false;
    if ((size_t)it.ws_offset > ws_bytes || sv_need(it.rows, it.cols) > ws_bytes - (size_t)it.ws_offset) return false;
    v->hdr = reinterpret_cast<double*>(ws + it.ws_offset);
    v->z = v->hdr + SV_HDR;
    v->y = v->z + (size_t)SV_B * it.cols;
    v->beff = min(SV_B, min(it.rows, it.cols));
    return true;
}

// a pointer read from the item table is generic to the compiler (flat loads); it always points into device memory, and
// the streaming passes say so
#define SV_GF const __attribute__((address_space(1))) float
__device__ __forceinline__ float4 sv_ld4(SV_GF* p) {
    typedef float f4 __attribute__((ext_vector_type(4)));
    const f4 t = *reinterpret_cast<const __attribute__((address_space(1))) f4*>(p);
    return make_float4(t.x, t.y, t.z, t.w);
}

__device__ __forceinline__ float4 sv_ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ double2 sv_ld2(const double* p) { return *reinterpret_cast<const double2*>(p); }

__device__ __forceinline__ double sv_wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// block-wide sums of N doubles per thread over THREADS threads; every thread gets the same results (thread i adds the
// partials of the waves of sum i in wave order, then all read them).  sh holds (THREADS / 64 + 1) * N doubles.
template <int N, int THREADS>
__device__ __forceinline__ void sv_block_sum(double (&v)[N], double* sh) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int i = 0; i < N; ++i) v[i] = sv_wave_sum(v[i]);
    __syncthreads();
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < N; ++i) sh[w * N + i] = v[i];
    }
    __syncthreads();
    double* tot = sh + (THREADS / 64) * N;
    if (threadIdx.x < N) {
        double t = 0.0;
        for (int k = 0; k < THREADS / 64; ++k) t += sh[k * N + threadIdx.x];
        tot[threadIdx.x] = t;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < N; ++i) v[i] = tot[i];
}

// ---- work schedule of the two streaming passes (as the multi-tensor spectral norm: a flat grid strides over units) ----
__device__ __forceinline__ int sv_units_of(const BgSvItem& it, int pass_b, char* ws, size_t ws_bytes) {
    SvView v;
    if (!sv_view(it, ws, ws_bytes, &v)) return 0;
    if (pass_b) return ((it.cols + SV_BLOCK - 1) / SV_BLOCK) * ((it.rows + SV_ROWS_B - 1) / SV_ROWS_B);
    const int64_t n = (int64_t)it.rows * it.cols;
    int64_t u = (n + SV_UNIT_ELEMS_A - 1) / SV_UNIT_ELEMS_A;
    const int64_t cap = (it.rows + 31) / 32;        // a block takes 32 rows per trip: more blocks than that would idle
    if (u > cap) u = cap;
    return u < 1 ? 1 : (int)u;
}
__device__ __forceinline__ int sv_sched_build(int* start, const BgSvItem* __restrict__ items, int n_items, int pass_b,
                                              char* ws, size_t ws_bytes) {
    for (int i = threadIdx.x; i < n_items; i += SV_BLOCK) start[i + 1] = sv_units_of(items[i], pass_b, ws, ws_bytes);
    if (threadIdx.x == 0) start[0] = 0;
    __syncthreads();
    if (threadIdx.x == 0)
        for (int i = 1; i <= n_items; ++i) start[i] += start[i - 1];
    __syncthreads();
    return start[n_items];
}
__device__ __forceinline__ int sv_sched_find(const int* start, int n_items, int unit) {
    int lo = 0, hi = n_items;            // largest i with start[i] <= unit
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (start[mid] <= unit) lo = mid; else hi = mid;
    }
    return lo;
}

// ---- begin -------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SV_BLOCK) void sv_begin_kernel(const BgSvItem* __restrict__ items, char* ws,
                                                             size_t ws_bytes) {
    const BgSvItem it = items[blockIdx.x];
    SvView v;
    if (!sv_view(it, ws, ws_bytes, &v)) return;
    const int64_t nz = SV_HDR + (int64_t)SV_B * it.cols;
    for (int64_t i = threadIdx.x; i < nz; i += SV_BLOCK) v.hdr[i] = 0.0;
    if (v.beff < SV_B) {
        const int64_t nq = (int64_t)SV_B * it.cols;
        for (int64_t i = threadIdx.x; i < nq; i += SV_BLOCK)
            if ((int)(i & (SV_B - 1)) >= v.beff) it.q[i] = 0.f;
    }
}

// ---- pass A: Y = W Q -----------------------------------------------------------------------------------------------
#define SV_FMA8(S, A, Q0, Q1)                                                                    \
    do {                                                                                         \
        S[0] += (A) * (Q0).x; S[1] += (A) * (Q0).y; S[2] += (A) * (Q0).z; S[3] += (A) * (Q0).w;  \
        S[4] += (A) * (Q1).x; S[5] += (A) * (Q1).y; S[6] += (A) * (Q1).z; S[7] += (A) * (Q1).w;  \
    } while (0)

#define SV_ROWS_A 8      // rows per wave and trip: the basis is read once per 8 rows of W

__device__ __forceinline__ void sv_project_body(SV_GF* __restrict__ w, SV_GF* __restrict__ q,
                                                double* __restrict__ y, int rows, int cols, int bid, int nblocks) {
    const int lane = threadIdx.x & 63;
    const int wave = bid * 4 + (threadIdx.x >> 6);
    const int nwaves = nblocks * 4;
    // eight rows per wave at a time: eight independent 16-byte loads of W in flight per lane, 64 accumulators
    for (int r0 = wave; r0 < rows; r0 += SV_ROWS_A * nwaves) {      // (second trip: rows > 32 * blocks of the item)
        SV_GF* wr[SV_ROWS_A];
#pragma unroll
        for (int k = 0; k < SV_ROWS_A; ++k) {
            const int rk = r0 + k * nwaves;
            wr[k] = w + (int64_t)(rk < rows ? rk : r0) * cols;
        }
        float s[SV_ROWS_A * SV_B];                                  // s[k * 8 + i]: row k, vector i
#pragma unroll
        for (int k = 0; k < SV_ROWS_A * SV_B; ++k) s[k] = 0.f;
        if ((cols & 3) == 0) {
            for (int c = lane * 4; c < cols; c += 256) {
                float4 a[SV_ROWS_A];
#pragma unroll
                for (int k = 0; k < SV_ROWS_A; ++k) a[k] = sv_ld4(wr[k] + c);
                SV_GF* qc = q + (int64_t)c * SV_B;
                {
                    const float4 q0 = sv_ld4(qc), q1 = sv_ld4(qc + 4);
#pragma unroll
                    for (int k = 0; k < SV_ROWS_A; ++k) SV_FMA8((s + k * SV_B), a[k].x, q0, q1);
                }
                {
                    const float4 q0 = sv_ld4(qc + 8), q1 = sv_ld4(qc + 12);
#pragma unroll
                    for (int k = 0; k < SV_ROWS_A; ++k) SV_FMA8((s + k * SV_B), a[k].y, q0, q1);
                }
                {
                    const float4 q0 = sv_ld4(qc + 16), q1 = sv_ld4(qc + 20);
#pragma unroll
                    for (int k = 0; k < SV_ROWS_A; ++k) SV_FMA8((s + k * SV_B), a[k].z, q0, q1);
                }
                {
                    const float4 q0 = sv_ld4(qc + 24), q1 = sv_ld4(qc + 28);
#pragma unroll
                    for (int k = 0; k < SV_ROWS_A; ++k) SV_FMA8((s + k * SV_B), a[k].w, q0, q1);
                }
            }
        } else {
            for (int c = lane; c < cols; c += 64) {
                SV_GF* qc = q + (int64_t)c * SV_B;
                const float4 q0 = sv_ld4(qc), q1 = sv_ld4(qc + 4);
#pragma unroll
                for (int k = 0; k < SV_ROWS_A; ++k) {
                    const float a = wr[k][c];
                    SV_FMA8((s + k * SV_B), a, q0, q1);
                }
            }
        }
        // the 64 sums of the wave, each over the 64 lanes, by halving: at distance h a lane keeps the half of its values
        // that its bit h selects and receives the other lanes' partials of them; after the six steps lane l holds the
        // total of s[l] (63 shuffles instead of 64 x 6)
#pragma unroll
        for (int h = 32; h >= 1; h >>= 1) {
            const bool up = (lane & h) != 0;
#pragma unroll
            for (int i = 0; i < h; ++i) {
                const float keep = up ? s[i + h] : s[i];
                const float send = up ? s[i] : s[i + h];
                s[i] = keep + __shfl_xor(send, h, 64);
            }
        }
        const int rk = r0 + (lane >> 3) * nwaves;                    // lane l: row l / 8 of the group, vector l % 8
        if (rk < rows) y[(int64_t)rk * SV_B + (lane & 7)] = (double)s[0];
    }
}

__global__ __launch_bounds__(SV_BLOCK) void sv_project_kernel(const BgSvItem* __restrict__ items, int n_items,
                                                               char* ws, size_t ws_bytes) {
    __shared__ int start[257];
    const int total = sv_sched_build(start, items, n_items, 0, ws, ws_bytes);
    for (int unit = blockIdx.x; unit < total; unit += gridDim.x) {      // (second trip: more than SV_GRID units)
        const int j = __builtin_amdgcn_readfirstlane(sv_sched_find(start, n_items, unit));   // (block-uniform: scalar loads)
        const BgSvItem it = items[j];
        SvView v;
        if (!sv_view(it, ws, ws_bytes, &v)) continue;
        sv_project_body((SV_GF*)it.w, (SV_GF*)it.q, v.y, it.rows, it.cols, unit - start[j], start[j + 1] - start[j]);
    }
}

// ---- pass B: Z += W^T Y ----------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SV_BLOCK) void sv_backproject_kernel(const BgSvItem* __restrict__ items, int n_items,
                                                                   char* ws, size_t ws_bytes) {
    __shared__ int start[257];
    __shared__ double2 ys[SV_ROWS_B * (SV_B / 2)];       // Y of the unit's rows: 16 KB
    const int total = sv_sched_build(start, items, n_items, 1, ws, ws_bytes);
    for (int unit = blockIdx.x; unit < total; unit += gridDim.x) {      // (second trip: more than SV_GRID units)
        const int j = __builtin_amdgcn_readfirstlane(sv_sched_find(start, n_items, unit));   // (block-uniform: scalar loads)
        const BgSvItem it = items[j];
        SvView v;
        if (!sv_view(it, ws, ws_bytes, &v)) continue;
        const int cblocks = (it.cols + SV_BLOCK - 1) / SV_BLOCK;
        const int u = unit - start[j];
        const int c = (u % cblocks) * SV_BLOCK + threadIdx.x;
        const int r0 = (u / cblocks) * SV_ROWS_B;
        const int nr = min(it.rows - r0, SV_ROWS_B);
        // the unit's rows of Y go through LDS: every lane needs the same 64 bytes per row, and as global loads they
        // cost the load path four 16-byte instructions per 4-byte load of W
        __syncthreads();                                  // (the readers of the previous unit are done)
        const double2* ysrc = reinterpret_cast<const double2*>(v.y + (int64_t)r0 * SV_B);
        for (int i = threadIdx.x; i < nr * (SV_B / 2); i += SV_BLOCK) ys[i] = ysrc[i];
        __syncthreads();
        if (c < it.cols) {
            double acc[SV_B];
#pragma unroll
            for (int i = 0; i < SV_B; ++i) acc[i] = 0.0;
            SV_GF* wp = (SV_GF*)it.w + (int64_t)r0 * it.cols + c;
            const int64_t cols = it.cols;
            int r = 0;
            for (; r + 8 <= nr; r += 8) {                 // 8 rows' loads in flight per thread
                float a[8];
#pragma unroll
                for (int k = 0; k < 8; ++k) a[k] = wp[(int64_t)(r + k) * cols];
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    const double av = (double)a[k];
#pragma unroll
                    for (int i = 0; i < SV_B / 2; ++i) {
                        const double2 yv = ys[(r + k) * (SV_B / 2) + i];     // (the same address in every lane)
                        acc[2 * i] = fma(av, yv.x, acc[2 * i]);
                        acc[2 * i + 1] = fma(av, yv.y, acc[2 * i + 1]);
                    }
                }
            }
            for (; r < nr; ++r) {
                const double av = (double)wp[(int64_t)r * cols];
#pragma unroll
                for (int i = 0; i < SV_B / 2; ++i) {
                    const double2 yv = ys[r * (SV_B / 2) + i];
                    acc[2 * i] = fma(av, yv.x, acc[2 * i]);
                    acc[2 * i + 1] = fma(av, yv.y, acc[2 * i + 1]);
                }
            }
            double* zc = v.z + (int64_t)c * SV_B;
#pragma unroll
            for (int i = 0; i < SV_B; ++i)
                if (i < v.beff) atomicAdd(zc + i, acc[i]);
        }
    }
}

// ---- pass C: orthonormalise Z into Q ----------------------------------------------------------------------------------
__device__ __forceinline__ void sv_load_row(const double* p, double (&row)[SV_B]) {
#pragma unroll
    for (int i = 0; i < SV_B; i += 2) {
        const double2 t = sv_ld2(p + i);
        row[i] = t.x;
        row[i + 1] = t.y;
    }
}

// o = row R^-1 for the upper triangular R^-1 held as ri[e], e running over (i, k >= i) row by row
__device__ __forceinline__ void sv_apply_upper(const double (&row)[SV_B], const double (&ri)[SV_NH], double (&o)[SV_B]) {
#pragma unroll
    for (int k = 0; k < SV_B; ++k) o[k] = 0.0;
    int e = 0;
#pragma unroll
    for (int i = 0; i < SV_B; ++i)
#pragma unroll
        for (int k = i; k < SV_B; ++k) o[k] = fma(row[i], ri[e], o[k]), ++e;
}

// Cholesky G = R^T R of the leading n x n block of the Gram matrix h (upper triangle, row by row) and R^-1 into ri (zero
// beyond the block); false (for every thread) if a pivot does not keep more than tol of its diagonal entry.  Thread 0
// computes in LDS (gm, rr, rinv: 8 x 8 each), all threads read the result.
__device__ __forceinline__ bool sv_chol_step(const double (&h)[SV_NH], double (&ri)[SV_NH], int n, double tol, double* gm,
                                             double* rr, double* rinv, int* flag) {
    if (threadIdx.x == 0) {
        int e = 0;
#pragma unroll
        for (int i = 0; i < SV_B; ++i)
#pragma unroll
            for (int k = i; k < SV_B; ++k) gm[i * SV_B + k] = h[e], ++e;
        bool ok = true;
        for (int i = 0; i < SV_B * SV_B; ++i) rr[i] = rinv[i] = 0.0;
        for (int j = 0; j < n && ok; ++j) {
            const double gjj = gm[j * SV_B + j];
            double d = gjj;
            for (int k = 0; k < j; ++k) d -= rr[k * SV_B + j] * rr[k * SV_B + j];
            if (!(gjj > 0.0) || !(gjj < INFINITY) || !(d > tol * gjj)) {
                ok = false;
                break;
            }
            const double rjj = sqrt(d);
            rr[j * SV_B + j] = rjj;
            for (int i = j + 1; i < n; ++i) {
                double t = gm[j * SV_B + i];
                for (int k = 0; k < j; ++k) t -= rr[k * SV_B + j] * rr[k * SV_B + i];
                rr[j * SV_B + i] = t / rjj;
            }
        }
        if (ok) {
            for (int i = 0; i < n; ++i) {              // row i of X = R^-1 from X R = I
                rinv[i * SV_B + i] = 1.0 / rr[i * SV_B + i];
                for (int j = i + 1; j < n; ++j) {
                    double t = 0.0;
                    for (int k = i; k < j; ++k) t += rinv[i * SV_B + k] * rr[k * SV_B + j];
                    rinv[i * SV_B + j] = -t / rr[j * SV_B + j];
                }
            }
            for (int i = 0; i < SV_B * SV_B; ++i) ok = ok && rinv[i] == rinv[i] && fabs(rinv[i]) < INFINITY;
        }
        *flag = ok ? 1 : 0;
    }
    __syncthreads();
    const bool ok = *flag != 0;
    int e = 0;
#pragma unroll
    for (int i = 0; i < SV_B; ++i)
#pragma unroll
        for (int k = i; k < SV_B; ++k) ri[e] = rinv[i * SV_B + k], ++e;
    __syncthreads();                                   // (thread 0 may write flag and rinv again)
    return ok;
}

__global__ __launch_bounds__(SV_TAIL) void sv_orth_kernel(const BgSvItem* __restrict__ items, char* ws,
                                                           size_t ws_bytes) {
    __shared__ double sh[(SV_TAIL / 64 + 1) * SV_NH];
    __shared__ double gm[SV_B * SV_B], rr[SV_B * SV_B], rinv[SV_B * SV_B];
    __shared__ int flag;
    const BgSvItem it = items[blockIdx.x];
    SvView v;
    if (!sv_view(it, ws, ws_bytes, &v)) return;
    double* z = v.z;
    const int cols = it.cols;
    // The fast path, Cholesky QR twice: G = Z^T Z = R^T R, Z1 = Z R^-1, and once more on Z1, three passes over Z instead
    // of three per column.  The same Q as Gram-Schmidt yields (the QR factorisation with a positive diagonal is unique);
    // the second round takes the orthonormality from cond(Z)^2 2^-53 to 2^-53.  It is taken only where every pivot keeps
    // more than 2^-26 of its column's squared norm; otherwise (dependent, zero or non-finite columns) the Gram-Schmidt
    // passes below decide with their 2^-80 rule.
    {
        double ri[SV_NH], h[SV_NH];
#pragma unroll
        for (int e = 0; e < SV_NH; ++e) h[e] = 0.0;
        for (int c = threadIdx.x; c < cols; c += SV_TAIL) {
            double row[SV_B];
            sv_load_row(z + (int64_t)c * SV_B, row);
            int e = 0;
#pragma unroll
            for (int i = 0; i < SV_B; ++i)
#pragma unroll
                for (int k = i; k < SV_B; ++k) h[e] = fma(row[i], row[k], h[e]), ++e;
        }
        sv_block_sum<SV_NH, SV_TAIL>(h, sh);
        bool fast = sv_chol_step(h, ri, v.beff, ldexp(1.0, -26), gm, rr, rinv, &flag);
        if (fast) {
#pragma unroll
            for (int e = 0; e < SV_NH; ++e) h[e] = 0.0;
            for (int c = threadIdx.x; c < cols; c += SV_TAIL) {
                double row[SV_B], o[SV_B];
                double* zr = z + (int64_t)c * SV_B;
                sv_load_row(zr, row);
                sv_apply_upper(row, ri, o);
                int e = 0;
#pragma unroll
                for (int i = 0; i < SV_B; ++i) {
                    zr[i] = o[i];
#pragma unroll
                    for (int k = i; k < SV_B; ++k) h[e] = fma(o[i], o[k], h[e]), ++e;
                }
            }
            sv_block_sum<SV_NH, SV_TAIL>(h, sh);
            fast = sv_chol_step(h, ri, v.beff, 0.5, gm, rr, rinv, &flag);
        }
        if (fast) {
            for (int c = threadIdx.x; c < cols; c += SV_TAIL) {
                double row[SV_B], o[SV_B];
                double* zr = z + (int64_t)c * SV_B;
                sv_load_row(zr, row);
                sv_apply_upper(row, ri, o);
                float* qr = it.q + (int64_t)c * SV_B;
#pragma unroll
                for (int k = 0; k < SV_B; ++k) {
                    qr[k] = (float)o[k];
                    zr[k] = 0.0;                           // the next pass B adds into zeros
                }
            }
            return;
        }
    }
    // rn[k]: squared norm of the finished column k as it stands in Z (columns stay unnormalised until the last pass);
    // 0 marks a zero column
    double rn[SV_B];
#pragma unroll
    for (int k = 0; k < SV_B; ++k) rn[k] = 0.0;
    for (int j = 0; j < SV_B; ++j) {
        double d[SV_B];
#pragma unroll
        for (int k = 0; k < SV_B; ++k) d[k] = 0.0;
        for (int c = threadIdx.x; c < cols; c += SV_TAIL) {          // (second trip: cols > 512)
            double row[SV_B];
            sv_load_row(z + (int64_t)c * SV_B, row);
            const double zj = z[(int64_t)c * SV_B + j];
#pragma unroll
            for (int k = 0; k < SV_B; ++k) d[k] = fma(row[k], zj, d[k]);
        }
        sv_block_sum<SV_B, SV_TAIL>(d, sh);
        double orig = 0.0;
#pragma unroll
        for (int k = 0; k < SV_B; ++k) orig = k == j ? d[k] : orig;
        bool keep = j < v.beff && orig > 0.0 && orig < INFINITY;          // (false for NaN as well)
        double rem = orig;
        if (keep && j > 0) {
            double cf[SV_B], d2[SV_B];
#pragma unroll
            for (int k = 0; k < SV_B; ++k) {
                cf[k] = (k < j && rn[k] > 0.0) ? d[k] / rn[k] : 0.0;
                d2[k] = 0.0;
            }
            for (int c = threadIdx.x; c < cols; c += SV_TAIL) {
                double row[SV_B];
                sv_load_row(z + (int64_t)c * SV_B, row);
                double zj = z[(int64_t)c * SV_B + j];
#pragma unroll
                for (int k = 0; k < SV_B; ++k) zj = fma(-cf[k], row[k], zj);
                z[(int64_t)c * SV_B + j] = zj;
#pragma unroll
                for (int k = 0; k < SV_B; ++k) d2[k] = fma(row[k], zj, d2[k]);
            }
            sv_block_sum<SV_B, SV_TAIL>(d2, sh);
            double nrm[1] = {0.0};
#pragma unroll
            for (int k = 0; k < SV_B; ++k) cf[k] = (k < j && rn[k] > 0.0) ? d2[k] / rn[k] : 0.0;
            for (int c = threadIdx.x; c < cols; c += SV_TAIL) {
                double row[SV_B];
                sv_load_row(z + (int64_t)c * SV_B, row);
                double zj = z[(int64_t)c * SV_B + j];
#pragma unroll
                for (int k = 0; k < SV_B; ++k) zj = fma(-cf[k], row[k], zj);
                z[(int64_t)c * SV_B + j] = zj;
                nrm[0] = fma(zj, zj, nrm[0]);
            }
            sv_block_sum<1, SV_TAIL>(nrm, sh);
            rem = nrm[0];
            keep = rem > ldexp(orig, -80) && rem < INFINITY;
        }
        if (!keep) {
            rem = 0.0;
            for (int c = threadIdx.x; c < cols; c += SV_TAIL) z[(int64_t)c * SV_B + j] = 0.0;
        }
#pragma unroll
        for (int k = 0; k < SV_B; ++k) rn[k] = k == j ? rem : rn[k];
    }
    double sc[SV_B];
#pragma unroll
    for (int k = 0; k < SV_B; ++k) sc[k] = rn[k] > 0.0 ? 1.0 / sqrt(rn[k]) : 0.0;
    for (int c = threadIdx.x; c < cols; c += SV_TAIL) {
        double row[SV_B];
        double* zr = z + (int64_t)c * SV_B;
        sv_load_row(zr, row);
        float o[SV_B];
#pragma unroll
        for (int k = 0; k < SV_B; ++k) o[k] = sc[k] > 0.0 ? (float)(row[k] * sc[k]) : 0.f;
        float* qr = it.q + (int64_t)c * SV_B;
#pragma unroll
        for (int k = 0; k < SV_B; ++k) {
            qr[k] = o[k];
            zr[k] = 0.0;                                   // the next pass B adds into zeros
        }
    }
}

// ---- Rayleigh-Ritz -----------------------------------------------------------------------------------------------------
// cyclic Jacobi on the leading n x n block of the symmetric a[8][8]; vm receives the eigenvectors as columns (identity
// outside the block).  One thread.
__device__ void sv_jacobi(double* a, double* vm, int n) {
    for (int i = 0; i < SV_B * SV_B; ++i) vm[i] = (i / SV_B == i % SV_B) ? 1.0 : 0.0;
    for (int sweep = 0; sweep < 40; ++sweep) {
        double off = 0.0, dia = 0.0;
        for (int p = 0; p < n; ++p)
            for (int q = 0; q < n; ++q) {
                const double t = a[p * SV_B + q];
                if (p == q) dia += t * t; else off += t * t;
            }
        if (!(off > 1e-36 * dia)) break;                   // (also leaves on NaN)
        for (int p = 0; p < n - 1; ++p)
            for (int q = p + 1; q < n; ++q) {
                const double apq = a[p * SV_B + q];
                if (apq == 0.0) continue;
                const double theta = (a[q * SV_B + q] - a[p * SV_B + p]) / (2.0 * apq);
                const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double cs = 1.0 / sqrt(t * t + 1.0), sn = t * cs;
                for (int k = 0; k < n; ++k) {              // columns p, q
                    const double akp = a[k * SV_B + p], akq = a[k * SV_B + q];
                    a[k * SV_B + p] = cs * akp - sn * akq;
                    a[k * SV_B + q] = sn * akp + cs * akq;
                }
                for (int k = 0; k < n; ++k) {              // rows p, q
                    const double apk = a[p * SV_B + k], aqk = a[q * SV_B + k];
                    a[p * SV_B + k] = cs * apk - sn * aqk;
                    a[q * SV_B + k] = sn * apk + cs * aqk;
                }
                for (int k = 0; k < SV_B; ++k) {
                    const double vkp = vm[k * SV_B + p], vkq = vm[k * SV_B + q];
                    vm[k * SV_B + p] = cs * vkp - sn * vkq;
                    vm[k * SV_B + q] = sn * vkp + cs * vkq;
                }
            }
    }
    for (int i = 0; i < n - 1; ++i) {                      // descending, by selection
        int m = i;
        for (int k = i + 1; k < n; ++k)
            if (a[k * SV_B + k] > a[m * SV_B + m]) m = k;
        if (m != i) {
            const double t = a[i * SV_B + i];
            a[i * SV_B + i] = a[m * SV_B + m];
            a[m * SV_B + m] = t;
            for (int k = 0; k < SV_B; ++k) {
                const double u = vm[k * SV_B + i];
                vm[k * SV_B + i] = vm[k * SV_B + m];
                vm[k * SV_B + m] = u;
            }
        }
    }
}


__global__ __launch_bounds__(SV_RITZ) void sv_ritz_kernel(const BgSvItem* __restrict__ items, char* ws,
                                                           size_t ws_bytes) {
    __shared__ double sh[(SV_RITZ / 64 + 1) * SV_NH];
    __shared__ double am[SV_B * SV_B], vm[SV_B * SV_B];
    const BgSvItem it = items[blockIdx.x];
    SvView v;
    if (!sv_view(it, ws, ws_bytes, &v)) return;
    double h[SV_NH];
#pragma unroll
    for (int e = 0; e < SV_NH; ++e) h[e] = 0.0;
    for (int r = threadIdx.x; r < it.rows; r += SV_RITZ) {             // (second trip: rows > 512)
        double row[SV_B];
        sv_load_row(v.y + (int64_t)r * SV_B, row);
        int e = 0;
#pragma unroll
        for (int i = 0; i < SV_B; ++i)
#pragma unroll
            for (int k = i; k < SV_B; ++k) h[e] = fma(row[i], row[k], h[e]), ++e;
    }
    sv_block_sum<SV_NH, SV_RITZ>(h, sh);
    if (threadIdx.x == 0) {
        int e = 0;
#pragma unroll
        for (int i = 0; i < SV_B; ++i)
#pragma unroll
            for (int k = i; k < SV_B; ++k) {
                am[i * SV_B + k] = h[e];
                am[k * SV_B + i] = h[e];
                ++e;
            }
        sv_jacobi(am, vm, v.beff);
        for (int i = 0; i < SV_B; ++i) {
            double lam = i < v.beff ? am[i * SV_B + i] : 0.0;
            if (!(lam > 0.0) || !(lam < INFINITY)) lam = 0.0;
            v.hdr[64 + i] = lam;
            it.sv[i] = (float)sqrt(lam);
        }
        for (int i = 0; i < SV_B * SV_B; ++i) v.hdr[i] = vm[i];
    }
    __syncthreads();
    // rotate the basis and Y to the Ritz vectors (columns >= b_eff are zero and stay so: vm is the identity there)
    for (int c = threadIdx.x; c < it.cols; c += SV_RITZ) {
        float* qr = it.q + (int64_t)c * SV_B;
        const float4 q0 = sv_ld4(qr), q1 = sv_ld4(qr + 4);
        const double in[SV_B] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w};
#pragma unroll
        for (int i = 0; i < SV_B; ++i) {
            double s = 0.0;
#pragma unroll
            for (int k = 0; k < SV_B; ++k) s = fma(in[k], vm[k * SV_B + i], s);
            qr[i] = (float)s;
        }
    }
    for (int r = threadIdx.x; r < it.rows; r += SV_RITZ) {
        double* yr = v.y + (int64_t)r * SV_B;
        double in[SV_B];
        sv_load_row(yr, in);
#pragma unroll
        for (int i = 0; i < SV_B; ++i) {
            double s = 0.0;
#pragma unroll
            for (int k = 0; k < SV_B; ++k) s = fma(in[k], vm[k * SV_B + i], s);
            yr[i] = s;
        }
    }
}

__global__ __launch_bounds__(SV_RITZ) void sv_resid_kernel(const BgSvItem* __restrict__ items, char* ws,
                                                            size_t ws_bytes) {
    __shared__ double sh[(SV_RITZ / 64 + 1) * SV_B];
    const BgSvItem it = items[blockIdx.x];
    SvView v;
    if (!sv_view(it, ws, ws_bytes, &v)) return;
    double lam[SV_B], acc[SV_B];
#pragma unroll
    for (int i = 0; i < SV_B; ++i) {
        lam[i] = v.hdr[64 + i];
        acc[i] = 0.0;
    }
    for (int c = threadIdx.x; c < it.cols; c += SV_RITZ) {
        double row[SV_B];
        sv_load_row(v.z + (int64_t)c * SV_B, row);
        const float* qr = it.q + (int64_t)c * SV_B;
        const float4 q0 = sv_ld4(qr), q1 = sv_ld4(qr + 4);
        const double qv[SV_B] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w};
#pragma unroll
        for (int i = 0; i < SV_B; ++i) {
            const double dlt = fma(-lam[i], qv[i], row[i]);
            acc[i] = fma(dlt, dlt, acc[i]);
        }
    }
    sv_block_sum<SV_B, SV_RITZ>(acc, sh);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int i = 0; i < SV_B; ++i) {
            float r = 0.f;
            if (i < v.beff && lam[0] > 0.0) {
                const double t = sqrt(acc[i]) / lam[0];
                r = t < 3.0e38 ? (float)t : 3.0e38f;          // (never Inf or NaN)
                if (!(t == t)) r = 3.0e38f;
            }
            it.resid[i] = r;
        }
    }
}

}  // namespace bg

using namespace bg;

extern "C" {

size_t bg_sv_workspace_bytes(int rows, int cols) {
    if (rows < 1 || cols < 1) return 0;
    return sv_need(rows, cols);
}

int bg_sv_batch(const BgSvItem* items_dev, int n_items, int iters, void* ws, size_t ws_bytes, void* stream) {
    BG_REQUIRE(items_dev, "bg_sv_batch: NULL item table");
    BG_REQUIRE(ws, "bg_sv_batch: NULL workspace");
    BG_REQUIRE(n_items >= 1 && n_items <= 256, "bg_sv_batch: n_items=%d (1..256 items per call)", n_items);
    BG_REQUIRE(iters >= 0 && iters <= 256, "bg_sv_batch: iters=%d (0..256)", iters);
    BG_REQUIRE(((uintptr_t)ws & 15) == 0, "bg_sv_batch: workspace must be 16-byte aligned");
    // the table is in device memory: the host can only hold the workspace against the smallest items there are; the
    // kernels check every item's own range against ws_bytes and leave an item that does not fit alone
    BG_REQUIRE(ws_bytes >= (size_t)n_items * sv_need(1, 1), "bg_sv_batch: workspace of %zu bytes too small for %d items",
               ws_bytes, n_items);
    hipStream_t s = as_stream(stream);
    char* w8 = reinterpret_cast<char*>(ws);
    hipLaunchKernelGGL(sv_begin_kernel, dim3(n_items), dim3(SV_BLOCK), 0, s, items_dev, w8, ws_bytes);
    BG_LAUNCH_CHECK();
    for (int t = 0; t <= iters; ++t) {
        hipLaunchKernelGGL(sv_project_kernel, dim3(SV_GRID), dim3(SV_BLOCK), 0, s, items_dev, n_items, w8, ws_bytes);
        BG_LAUNCH_CHECK();
        if (t == iters) {
            hipLaunchKernelGGL(sv_ritz_kernel, dim3(n_items), dim3(SV_RITZ), 0, s, items_dev, w8, ws_bytes);
            BG_LAUNCH_CHECK();
        }
        hipLaunchKernelGGL(sv_backproject_kernel, dim3(SV_GRID), dim3(SV_BLOCK), 0, s, items_dev, n_items, w8, ws_bytes);
        BG_LAUNCH_CHECK();
        if (t == iters)
            hipLaunchKernelGGL(sv_resid_kernel, dim3(n_items), dim3(SV_RITZ), 0, s, items_dev, w8, ws_bytes);
        else
            hipLaunchKernelGGL(sv_orth_kernel, dim3(n_items), dim3(SV_TAIL), 0, s, items_dev, w8, ws_bytes);
        BG_LAUNCH_CHECK();
    }
    return BG_OK;
}

}  // extern "C"
