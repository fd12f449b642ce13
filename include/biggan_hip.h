/* biggan_hip.h - C ABI of libbiggan_hip.so: the MI355X (gfx950) kernels behind the BigGAN
 * training-step hot path of david-jk/BigGAN-Tensorflow.
 *
 * The reference has no FFI: its operator layer (ops.py, DiffAugment_tf.py) lowers to stock
 * TensorFlow ops.  Each entry point below names the reference call site whose arithmetic it
 * replaces (file:line relative to the reference repository).
 *
 * Conventions
 *   - every pointer is a DEVICE pointer owned by the caller (PyTorch tensor storage); the library
 *     never allocates, frees or retains memory and never synchronises the device;
 *   - every call is asynchronous on the caller-supplied HIP stream (void* = hipStream_t) and is
 *     safe to capture into a hipGraph;
 *   - tensors are NHWC fp32, conv kernels HWIO [k,k,Cin,Cout], transposed-conv kernels
 *     [k,k,Cout,Cin] (the reference's variable layouts, ops.py:88,127);
 *   - return value 0 = success; non-zero = error, message in bg_last_error() (thread-local);
 *   - scratch memory is passed in by the caller, sized by the matching *_workspace_bytes();
 *   - sub-pixel up-sampling (ops.py:23-27 subpixel_conv = conv to r*r*C channels + tf.nn.depth_to_space) is
 *     bg_depth_to_space / bg_space_to_depth, and bg_conv2d_fwd_d2s where the bf16-resident convolution can store
 *     its output at the shuffled address itself.
 */
#ifndef BIGGAN_HIP_H
#define BIGGAN_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BG_ABI_VERSION 10

enum { BG_OK = 0, BG_ERR_ARG = 1, BG_ERR_LAUNCH = 2, BG_ERR_UNSUPPORTED = 3 };
enum { BG_PAD_REFLECT = 0, BG_PAD_ZERO = 1 };
/* element types of activation tensors (the "_t" entry points and the dtype fields of BgConvDesc) */
enum { BG_F32 = 0, BG_BF16 = 1 };
/* arithmetic of a GEMM-shaped launch, chosen PER CALL in its descriptor (no process-wide state):
 *   BG_COMPUTE_F32  : v_mfma_f32_32x32x2_f32, exact fp32 FMA chain (the reference's precision, ops.py:14)
 *   BG_COMPUTE_BF16 : bf16 MFMA with fp32 accumulation; fp32 operands are rounded to bf16 (RNE) while staged */
enum { BG_COMPUTE_F32 = 0, BG_COMPUTE_BF16 = 1 };

int         bg_abi_version(void);
const char* bg_last_error(void);
/* "gfx950" - the only code object in the library */
const char* bg_target_arch(void);

/* Host-side helper of the input pipeline (utils.py:12-38 decode_png): reverse the PNG row filters of an 8-bit
 * image on the CPU.  raw: h rows of 1 filter byte + stride bytes (the inflated IDAT stream); out: h * stride. */
int bg_png_unfilter(const unsigned char* raw, int h, int stride, int bpp, unsigned char* out);

/* Host-side helpers of the input pipeline (tf.image.decode_jpeg behind utils.py:27; csrc/jpeg_entropy.hip): the serial
 * part of decoding an 8-bit Huffman sequential JPEG (SOF0 / SOF1; 1 or 3 components; luma sampling 1x1, 2x1 or 2x2 with
 * chroma 1x1; one interleaved scan; restart intervals) on the CPU.  data[0:n] is untrusted: nothing outside it is read.
 *   bg_jpeg_info          the headers: size, components, luma sampling hs x vs (1 x 1 for one component), per component
 *                         the block grid bw x bh (whole MCUs) and its quantisation table in natural (row-major) order,
 *                         blocks = sum of bw * bh
 *   bg_jpeg_coefficients  the Huffman decode with DC prediction: coef[64 * blocks] int16, de-zigzagged, NOT dequantised;
 *                         component by component, each block-row major, 64 values a block; coef_count must be 64 * blocks
 * BG_ERR_ARG: truncated or corrupt data (or a NULL argument); BG_ERR_UNSUPPORTED: progressive, arithmetic-coded, 12-bit,
 * two- or four-component files, other samplings, non-interleaved scans. */
typedef struct BgJpegInfo {
    int32_t  width, height, ncomp, hs, vs, restart;
    int32_t  bw[3], bh[3];
    int64_t  blocks;
    uint16_t q[3][64];
} BgJpegInfo;
int bg_jpeg_info(const unsigned char* data, size_t n, BgJpegInfo* info);
int bg_jpeg_coefficients(const unsigned char* data, size_t n, int16_t* coef, size_t coef_count);

/* Host-side helper of the event-file writer (trainlog.py; TF's lib/io/record_writer.cc frames every record with two
 * of these): CRC-32C (Castagnoli, reflected polynomial 0x82F63B78, initial value and final xor 0xFFFFFFFF) of n bytes.
 * crc is the CRC of the bytes before them (0 to start), so that a buffer can be fed in pieces. */
uint32_t bg_crc32c(const void* data, size_t n, uint32_t crc);

/* --------------------------------------------------------------------------------------------
 * Convolution geometry shared by conv / transposed conv (ops.py:49-139).
 *   conv   : x[N,H,W,Cin]  -> y[N,Ho,Wo,Cout],  Ho = (H + pad_lo + pad_hi - k)/stride + 1
 *   deconv : x[N,H,W,Cin]  -> y[N,Ho,Wo,Cout],  Ho = stride*H ('SAME'), pad_lo = TF's low crop
 * ------------------------------------------------------------------------------------------ */
typedef struct BgConvDesc {
    int32_t N, H, W, Cin;      /* input  */
    int32_t Ho, Wo, Cout;      /* output */
    int32_t k, stride;
    int32_t pad_lo;            /* low padding (conv) / low crop (deconv)            */
    int32_t pad_mode;          /* BG_PAD_REFLECT (tf.pad REFLECT + VALID, ops.py:82) or BG_PAD_ZERO */
    int32_t compute;           /* BG_COMPUTE_F32 / BG_COMPUTE_BF16 (fp32 tensors)                  */
    int32_t x_dtype;           /* element type of the layer's INPUT-side tensor  (x, dx): BG_F32 / BG_BF16 */
    int32_t y_dtype;           /* element type of the layer's OUTPUT-side tensor (y, dy)                    */
    int32_t w_packed;          /* 1: w is a bf16 K-contiguous packed copy (see below), 0: the fp32 variable */
} BgConvDesc;

/* The bf16-RESIDENT data path (BASELINE configs 3-5).  When the tensor a launch GATHERS from (x for the forward
 * and the weight gradient, dy for the input gradient) is BG_BF16, the launch runs on the global_load_lds kernels
 * of csrc/igemm16.hip: tiles go HBM -> LDS without passing through registers, so the weights must already be bf16
 * with the reduction dimension contiguous (w_packed = 1):
 *     forward of conv  : [k*k][Cout][Cin]      input gradient of conv  : [k*k][Cin][Cout]
 *     forward of deconv: [k*k][Cout][Cin]      input gradient of deconv: [k*k][Cin][Cout]
 * i.e. for each op one of the two copies bg_spectral_norm_batch_fwd writes next to w / sigma (BgSnItem::pack_p =
 * the variable's own order, pack_t = the two inner axes swapped).  Channel counts must be multiples of 8.  The
 * forward and the input gradient take kernels of at most 4 x 4 taps (k <= 4): with a larger k bg_conv2d_fwd /
 * bg_conv2d_dgrad / bg_deconv2d_fwd / bg_deconv2d_dgrad return BG_ERR_ARG and a message, and callers run the layer
 * on the fp32-tensor kernels (functional._resident_ok).  The
 * other tensor of the call may be bf16 or fp32 (its dtype field); weight gradients are always fp32.  With
 * BG_PAD_REFLECT the input gradient is computed on the padded grid and folded back (scratch from ws), or, for
 * 3 x 3 windows with one row of padding on maps of at least 4 x 4, by mirrored-tap launches on the map itself.
 *
 * Geometry every conv entry point accepts (check_conv): 1 <= k <= 7, stride 1 or 2, 0 <= pad_lo < k, pad_lo < H,
 * the last window starting inside the input, and for BG_PAD_REFLECT tf.pad's rule pad_lo, pad_hi <= H - 1, W - 1
 * (pad_hi = (Ho - 1) stride + k - 1 - pad_lo - (H - 1)); the input gradient also needs H, W multiples of the
 * stride.  Within that, every map size (down to 2 x 2, non-square), both splits of an odd total padding and maps
 * on which one row mirrors both borders (H <= pad_lo + pad_hi + 1) are computed. */

/* Every MFMA GEMM entry point takes caller-provided scratch (ws, ws_bytes) sized by the matching
 * *_workspace_bytes(): it holds split-K partial slabs for layers whose output is too small to fill
 * the chip (4x4 / 8x8 feature maps, weight gradients).  ws may be NULL: the kernel then runs
 * un-split (same result up to fp32 summation order). */

/* tf.nn.conv2d (+ reflect tf.pad, + bias_add)                       ops.py:82,94-98
 *   y = alpha * conv(x, w) [+ bias] [+ y if accumulate]; alpha_dev (nullable) is a device scalar.
 *   x, y: fp32, or the dtypes named by d->x_dtype / d->y_dtype; w: fp32 [k,k,Cin,Cout] or the packed bf16 copy. */
size_t bg_conv2d_fwd_workspace_bytes(const BgConvDesc*);
int bg_conv2d_fwd  (const BgConvDesc*, const void* x, const void* w, const float* bias,
                    const float* alpha_dev, void* y, int accumulate,
                    void* ws, size_t ws_bytes, void* stream);
/* The same convolution with tf.nn.depth_to_space(block) of its output fused into the store (ops.py:23-27
 * subpixel_conv): d describes the convolution (Cout = block * block * C, stride 1, Ho x Wo = H x W) and y is the shuffled
 * tensor [N, block * Ho, block * Wo, C]: y[n, h * block + i, w * block + j, c] = conv[n, h, w, (i * block + j) * C + c].
 * The epilogue writes each 16-byte row segment (8 channels, C % 8 == 0: a segment never straddles a sub-pixel) at its
 * shuffled address, so [N, Ho, Wo, Cout] is never materialised; the accumulators are those of bg_conv2d_fwd, so the
 * result is bit-identical to bg_conv2d_fwd + bg_depth_to_space.  bg_conv2d_fwd_d2s_supported returns 1 for the launches
 * whose kernel form has the fused store (bf16-resident, block = 2: the halo-tile form, and the tap kernel without
 * split-K and without position-major rows); elsewhere callers run the pair.  No workspace: supported launches never
 * split K. */
int bg_conv2d_fwd_d2s_supported(const BgConvDesc*, int block);
int bg_conv2d_fwd_d2s(const BgConvDesc*, const void* x, const void* w, const float* bias, const float* alpha_dev,
                      void* y, int block, void* ws, size_t ws_bytes, void* stream);
/* gradient of the above w.r.t. x (reflect padding folded back)      autodiff of ops.py:82,94
 *   dy has d->y_dtype, dx has d->x_dtype */
size_t bg_conv2d_dgrad_workspace_bytes(const BgConvDesc*);
int bg_conv2d_dgrad(const BgConvDesc*, const void* dy, const void* w, const float* alpha_dev,
                    void* dx, int accumulate, void* ws, size_t ws_bytes, void* stream);
/* gradient w.r.t. w: dw[k,k,Cin,Cout], always fp32 */
size_t bg_conv2d_wgrad_workspace_bytes(const BgConvDesc*);
int bg_conv2d_wgrad(const BgConvDesc*, const void* x, const void* dy, float* dw,
                    void* ws, size_t ws_bytes, void* stream);

/* tf.nn.conv2d_transpose(SAME) (+ bias_add)                          ops.py:127-132 */
size_t bg_deconv2d_fwd_workspace_bytes(const BgConvDesc*);
int bg_deconv2d_fwd  (const BgConvDesc*, const void* x, const void* w, const float* bias,
                      const float* alpha_dev, void* y, int accumulate,
                      void* ws, size_t ws_bytes, void* stream);
/* Transposed-conv forward with the batch-norm statistics of its OUTPUT fused into the epilogue (ops.py:630
 * tf.nn.moments of the tensor the following condition_batch_norm / batch_norm normalises): sums[0..Cout) = sum of the
 * stored (bf16-rounded) outputs per channel over (N, Ho, Wo), sums[Cout..2 Cout) = sum of their squares, fp64, zeroed by
 * the call - what bg_bn_stats_t would compute by reading y again.  Available for the bf16-resident launches that take the
 * halo-tile form (bf16 y): bg_deconv2d_fwd_stats_workspace_bytes returns the bytes of per-block partial sums the call
 * needs (stats_ws), 0 when the launch has no fused statistics (callers then use bg_bn_stats_t).  Deterministic: one
 * partial row per block, summed in fp64. */
size_t bg_deconv2d_fwd_stats_workspace_bytes(const BgConvDesc*);
int bg_deconv2d_fwd_stats(const BgConvDesc*, const void* x, const void* w, const float* bias, const float* alpha_dev,
                          void* y, int accumulate, double* sums, void* stats_ws, size_t stats_ws_bytes, void* ws,
                          size_t ws_bytes, void* stream);
size_t bg_deconv2d_dgrad_workspace_bytes(const BgConvDesc*);
int bg_deconv2d_dgrad(const BgConvDesc*, const void* dy, const void* w, const float* alpha_dev,
                      void* dx, int accumulate, void* ws, size_t ws_bytes, void* stream);
size_t bg_deconv2d_wgrad_workspace_bytes(const BgConvDesc*);
int bg_deconv2d_wgrad(const BgConvDesc*, const void* x, const void* dy, float* dw,
                      void* ws, size_t ws_bytes, void* stream);

/* What a conv / transposed-conv call would launch, as text, without launching it (no GPU needed): one line of
 * "key=value" pairs separated by "; " in buf.  pass: BG_PASS_* - the six passes above and the forward with the fused
 * depth-to-space store (block 2).  ws_bytes: the workspace the caller would hand the call ((size_t)-1: what the pass's
 * *_workspace_bytes returns; 0: a null pointer).  The line is made from the same plan the call and its queries read:
 *   every route     route (the form of the call: F32_TAP ... TN_BF16), ws (bytes of workspace: with ws_bytes = -1 the
 *                   query's answer, else what the launches use of ws_bytes)
 *   bf16 routes     kernel (the instantiation, as bg_prof_dump names it), grid (x * y * z), block, lds (dynamic bytes),
 *                   tile (rows x columns), form (two | ring | wide | phased; halo; narrow | wide | phased for weight
 *                   gradients), splitk, posmajor, mfast, zfold, stats_rows, d2s (the launch stores depth-to-space)
 *   halo-tile       nt, nf            weight gradients   rows_per_split
 *   ring routes     ring_kernel, ring_grid, ring_tile, ring_form, ring_lds (the mirrored-tap launch)
 *   padded grid     fold_grid_bytes (the padded gradient at the head of the workspace), fold_grid (Hp x Wp)
 * BG_ERR_ARG (nothing written) for a null descriptor or buffer, a buffer too small for the line, an unknown pass, a
 * descriptor the pass rejects, or a ws_bytes smaller than the padded grid of a call that needs one. */
enum { BG_PASS_CONV_FWD = 0, BG_PASS_CONV_DGRAD = 1, BG_PASS_CONV_WGRAD = 2, BG_PASS_DECONV_FWD = 3,
       BG_PASS_DECONV_DGRAD = 4, BG_PASS_DECONV_WGRAD = 5, BG_PASS_CONV_FWD_D2S = 6 };
int bg_conv_plan_describe(const BgConvDesc* d, int pass, size_t ws_bytes, char* buf, size_t buf_bytes);

/* Direct (vector-ALU, HBM-bound) path for k x k stride-1 convolutions with <= 3 output channels:
 * the generator's RGB head G_logit (BigGAN.py:570 -> ops.py:49-113).  Same arithmetic as
 * bg_conv2d_*; bg_rgbconv_supported tells whether a geometry qualifies.
 * bg_rgbconv_supported(d) == 1 means that ALL THREE passes (fwd, dgrad, wgrad) compute d, so a caller decides once per
 * layer: fp32 tensors, 1 <= Cout <= 3, Cin % 4 == 0, stride 1, Ho x Wo = H x W, k = 1 or 3, any 0 <= pad_lo < k
 * (pad_hi = k - 1 - pad_lo, the two may differ), k * k * Cin * 16 bytes <= 60 KB of LDS, and for BG_PAD_REFLECT
 * pad_lo, pad_hi <= min(H, W) - 1.  That includes maps on which a row mirrors both borders (H <= pad_lo + pad_hi + 1:
 * the input gradient takes both mirrors).  Every other geometry runs on bg_conv2d_*. */
int bg_rgbconv_supported(const BgConvDesc*);
int bg_rgbconv_fwd  (const BgConvDesc*, const float* x, const float* w, const float* bias, float* y,
                     int accumulate, void* stream);
int bg_rgbconv_dgrad(const BgConvDesc*, const float* dy, const float* w, float* dx, int accumulate, void* stream);
size_t bg_rgbconv_wgrad_workspace_bytes(const BgConvDesc*);
int bg_rgbconv_wgrad(const BgConvDesc*, const float* x, const float* dy, float* dw,
                     void* ws, size_t ws_bytes, void* stream);

/* --------------------------------------------------------------------------------------------
 * Plain (batched) matrix products: tf.matmul call sites ops.py:163-165 (dense), 481,485
 * (attention), utils.py:198,222 (Gram matrix of the regulariser).
 *   C[b] = alpha * op(A[b]) * op(B[b]) (+ bias[n]) (+ C[b] if accumulate), row-major, fp32.
 *   transA: A stored [K,M] (lda = M-stride), transB: B stored [N,K].
 * ------------------------------------------------------------------------------------------ */
typedef struct BgGemmDesc {
    int32_t M, N, K;
    int32_t transA, transB;
    int32_t lda, ldb, ldc;
    int32_t batch;
    int64_t strideA, strideB, strideC;   /* elements between batch items */
    int32_t compute;                     /* BG_COMPUTE_F32 / BG_COMPUTE_BF16 */
    int32_t reserved;
} BgGemmDesc;
size_t bg_gemm_workspace_bytes(const BgGemmDesc*);
int bg_gemm(const BgGemmDesc*, const float* A, const float* B, const float* bias,
            const float* alpha_dev, float* C, int accumulate, void* ws, size_t ws_bytes, void* stream);

/* Grouped small dense projections on shared batch rows: the beta / gamma fully_connected(z -> C) pairs of the two
 * conditional batch norms of a generator block (ops.py:623-624 -> ops.py:163-165) as ONE launch per direction.
 *   fwd  : y_i[b, :] = x_i[b, :K_i] w_i + bias_i             (x_i rows ldx_i floats apart, w_i [K_i, N_i], y_i [B, N_i])
 *   wgrad: dw_i (+)= x_i^T dy_i, db_i (+)= column sums of dy_i  (y = dy_i; acc_w / acc_b select add vs overwrite; db
 *          may be NULL).  The items array is HOST memory (copied into the launch), all other pointers device fp32.
 * No atomics: every output element is produced by one thread in a fixed batch order. */
#define BG_DENSE_GROUP_MAX 8
typedef struct BgDenseItem {
    const float* x;
    int64_t ldx;
    const float* w;        /* fwd */
    const float* bias;     /* fwd, nullable */
    float* y;              /* fwd: output; wgrad: dy (read) */
    float* dw;             /* wgrad */
    float* db;             /* wgrad, nullable */
    int32_t K, N;
    int32_t acc_w, acc_b;
} BgDenseItem;
int bg_dense_group_fwd(const BgDenseItem* items_host, int n_items, int B, void* stream);
int bg_dense_group_wgrad(const BgDenseItem* items_host, int n_items, int B, void* stream);
/* Input gradient of a group whose items all read the SAME input rows (a latent that needs a gradient):
 *   dx[b, :K] (+)= sum_i dy_i[b, :] w_i^T      (dy_i in y, w_i [K, N_i]; every item has the same K; dx rows lddx floats
 *   apart; accumulate selects add vs overwrite).  One thread per element of dx, items and columns in a fixed order. */
int bg_dense_group_dgrad(const BgDenseItem* items_host, int n_items, int B, void* dx, int lddx, int accumulate,
                         void* stream);

/* Latent fan-out / fan-in of the generator's shared class embedding and shared z (BigGAN.py:338-424): every level's
 * vector [z_i | class vector | shared vector] is a column range of one packed buffer, written by ONE launch, and the
 * gradients of the shared sources are reduced over all levels by ONE launch.  Both calls route column segments:
 *   target t, element (b, c) (+)= sum over the segments with target == t that cover c, in array order, of
 *                                 src[b * lds + src_col + c - dst_col]
 *   fan-out: every column of every target is covered by exactly one segment (checked);
 *   fan-in : any number of segments per column; a column no segment covers becomes 0 (or keeps its value).
 * ``targets`` / ``segs`` are HOST arrays of BgLatentTarget / BgLatentSeg (copied into the launch), declared void* so
 * that the ABI gains no new pointer types.  No atomics: one thread per output element. */
#define BG_LATENT_MAX_TARGETS 8
#define BG_LATENT_MAX_SEGS 48
typedef struct BgLatentTarget {
    float* dst;
    int64_t ldd;
    int32_t width, accumulate;
} BgLatentTarget;
typedef struct BgLatentSeg {
    const float* src;
    int64_t lds;
    int32_t src_col, dst_col, width, target;
} BgLatentSeg;
int bg_latent_fanout(const void* targets_host, int n_targets, const void* segs_host, int n_segs, int B, void* stream);
int bg_latent_fanin(const void* targets_host, int n_targets, const void* segs_host, int n_segs, int B, void* stream);

/* --------------------------------------------------------------------------------------------
 * Multi-branch stride-1 convolution (ops.py:403-436 clown_conv, ops.py:52-59 string kernels, ops.py:95 dilation):
 * several convolutions of ONE input x[N,H,W,Cin], each writing its own channel slice of one output row.
 * ``table`` is a HOST array of n BgMixBranch (copied into the launch by value, so it may die after the call and a
 * captured graph keeps it), declared void* so that the ABI gains no new pointer types.  Per branch:
 *   y[n,p,q,c_off+c] = bias[c] + sum_{i,j<k} sum_ci x[n, P(p - lo + i*dil), P(q - lo + j*dil), ci] * W(i,j,ci,c)
 * with P the padding (BG_PAD_REFLECT: tf.pad REFLECT, the index mirrored at the border without repeating it;
 * BG_PAD_ZERO: taps outside the image read 0) and W the branch kernel:
 *   transposed = 0: w [k,k,Cin,cb] (conv, ops.py:88),              W(i,j,ci,c) = w[i][j][ci][c]
 *   transposed = 1: w [k,k,cb,Cin] (stride-1 conv2d_transpose SAME, ops.py:127), stored as a correlation with the
 *                   flipped kernel: W(i,j,ci,c) = w[k-1-i][k-1-j][c][ci], lo = k - 1 - TF's low crop.
 * Geometry from the descriptor: N, H, W, Cin, Ho = H, Wo = W, stride 1; x_dtype names x / dx, y_dtype y / dy
 * (BG_F32 or BG_BF16); with fp32 x and y, compute = BG_COMPUTE_BF16 rounds x and w to bf16 as they are read,
 * BG_COMPUTE_F32 is an exact fp32 FMA chain.  bf16 tensors are multiplied as bf16 x bf16 (w rounded to bf16) with
 * fp32 accumulation; with bf16 x and y / dy and Cin % 32 == 0 the three passes are implicit GEMMs on
 * v_mfma_f32_16x16x32_bf16.  y / dy rows are ldy elements apart (the branches' slices may sit inside a wider tensor whose
 * other channels are left untouched); x / dx rows are Cin apart.  Any branch width; at most BG_MIX_MAX_BRANCHES.
 * Reflect padding needs lo <= H-1, W-1 and the high overhang (k-1)*dil - lo <= H-1, W-1 (TF's rule).
 * Deterministic: no atomics; the weight gradient's split-K slabs (ws) are reduced in a fixed order.
 * ------------------------------------------------------------------------------------------ */
#define BG_MIX_MAX_BRANCHES 8
typedef struct BgMixBranch {
    int32_t c_off;         /* first channel of the branch in a row of y / dy                              */
    int32_t cb;            /* branch width (output channels)                                             */
    int32_t k, dil, lo;    /* taps per axis, dilation, low tap offset                                    */
    int32_t pad_mode;      /* BG_PAD_REFLECT / BG_PAD_ZERO                                               */
    int32_t transposed;    /* 0: conv kernel [k,k,Cin,cb]; 1: transposed-conv kernel [k,k,cb,Cin]         */
    int32_t acc_w;         /* weight gradient: 1 adds into dw, 0 overwrites                               */
    const float* w;        /* fp32 kernel in the variable's layout                                       */
    const float* bias;     /* forward, nullable: [cb]                                                    */
    float* dw;             /* weight gradient (same layout as w), NULL: none for this branch; bias gradients
                              come from bg_bias_grad_t */
} BgMixBranch;
/* forward: y[..., c_off : c_off + cb] = branch(x) for every branch */
int bg_mixconv_fwd(const BgConvDesc* d, const void* table_host, int n_branches, const void* x, void* y, int ldy,
                   void* stream);
/* input gradient: dx (+)= sum over branches of the adjoint of the branch (reflect padding folded back at the border),
 * summed in registers; one thread per element of dx */
int bg_mixconv_dgrad(const BgConvDesc* d, const void* table_host, int n_branches, const void* dy, int ldy, void* dx,
                     int accumulate, void* stream);
/* weight gradients of every branch (dw of each table entry, fp32, (+)= per acc_w) */
size_t bg_mixconv_wgrad_workspace_bytes(const BgConvDesc* d, const void* table_host, int n_branches);
int bg_mixconv_wgrad(const BgConvDesc* d, const void* table_host, int n_branches, const void* x, const void* dy,
                     int ldy, void* ws, size_t ws_bytes, void* stream);

/* --------------------------------------------------------------------------------------------
 * Fused attention of self_attention_2 (ops.py:481-485): o = softmax(q k^T) v, no 1/sqrt(d) scale.
 *   q [B,N,d], k [B,Nk,d], v [B,Nk,dv], o [B,N,dv], lse [B,N] (= max + log sum exp of each query's
 *   logits, kept for backward).  The [N,Nk] logits/probabilities are never written to memory; backward
 *   recomputes them (delta_ws: B*N floats of scratch).  fp32 MFMA, deterministic (no atomics).
 *   Supported when N % 128 == 0, Nk % 128 == 0, d % 4 == 0, dv % 4 == 0, d <= 32, dv <= 128
 *   (bg_attention2_supported); other shapes use bg_gemm + bg_softmax_* (materialised form).
 * ------------------------------------------------------------------------------------------ */
int bg_attention2_supported(int N, int Nk, int d, int dv);
int bg_attention2_fwd(const float* q, const float* k, const float* v, float* o, float* lse,
                      int B, int N, int Nk, int d, int dv, void* stream);
int bg_attention2_bwd(const float* q, const float* k, const float* v, const float* o, const float* dout,
                      const float* lse, float* dq, float* dk, float* dv_out, float* delta_ws,
                      int B, int N, int Nk, int d, int dv, void* stream);

/* --------------------------------------------------------------------------------------------
 * Fused attention on the bf16 MFMA for the bf16-resident path (csrc/attention16.hip): same function as
 * bg_attention2_* (ops.py:481-485, o = softmax(q k^T) v, no scale) with bf16 tensors that may be COLUMN SLICES of wider
 * tensors (the fused f|g|h projection of self_attention_2 and its max-pooled copy): every tensor has a row stride ld*
 * and a batch stride s* in elements.  d <= 64, dv <= 256 (all BASELINE topologies; BigGAN.py:292-293 puts d = 48 / 64,
 * dv = 192 / 256 in the 256^2 / 512^2 generators), d and dv multiples of 4, N and Nk multiples of 128, pointers 8-byte
 * aligned.  lse [B,N] fp32 (contiguous) is written by fwd and read by bwd; delta_ws: B*N floats of scratch.
 * Probabilities are rounded to bf16 before the P V product (fp32 accumulation); deterministic, no atomics.
 * bwd: dq may be NULL, or dk and dv_out may both be NULL (the two gradient kernels are independent); delta_ws is
 * (re)computed by a call that produces dk / dv and reused as it stands by a dq-only call.
 * bg_attention16_supported(N, Nk, d, dv) == 1 means that fwd and both bwd calls compute EVERY column of every output
 * for that shape: each (d, dv) with d % 4 == 0, d <= 64, dv % 4 == 0, dv <= 256 in any combination (d <= 16 with
 * dv > 128 included), N and Nk any multiples of 128, equal or not.
 * ------------------------------------------------------------------------------------------ */
typedef struct BgAttn16Desc {
    int32_t B, N, Nk, d, dv;
    int32_t reserved;
    int64_t ldq, sq, ldk, sk, ldv, sv, ldo, so;          /* q, k, v, o                                  */
    int64_t ldg, sg, lddq, sdq, lddk, sdk, lddv, sdv;    /* backward: dout (layout of o), dq, dk, dv    */
} BgAttn16Desc;
int bg_attention16_supported(int N, int Nk, int d, int dv);
int bg_attention16_fwd(const BgAttn16Desc*, const void* q, const void* k, const void* v, void* o, float* lse,
                       void* stream);
int bg_attention16_bwd(const BgAttn16Desc*, const void* q, const void* k, const void* v, const void* o,
                       const void* dout, const float* lse, void* dq, void* dk, void* dv_out, float* delta_ws,
                       void* stream);

/* --------------------------------------------------------------------------------------------
 * Spectral norm, one power iteration (ops.py:718-747).  W is [rows, cols] (= reshape(w,[-1,last])).
 *   v = l2n(u W^T), u_out = l2n(v W), sigma = |v W|, w_norm = W / sigma.
 *   l2n(t) = t * rsqrt(max(sum t^2, 1e-12)).  scratch: bg_spectral_norm_workspace_bytes (fp64 accumulators).
 * bwd: dW = (G - <G, w_norm> v^T u_out) / sigma  (u_out, v stop-gradient, ops.py:738-739).
 * ------------------------------------------------------------------------------------------ */
size_t bg_spectral_norm_workspace_bytes(int rows, int cols);
int bg_spectral_norm_fwd(const float* w, const float* u_in, float* u_out, float* v_out,
                         float* sigma_out, float* w_norm, int rows, int cols,
                         void* ws, size_t ws_bytes, void* stream);
int bg_spectral_norm_bwd(const float* g_wnorm, const float* w_norm, const float* u_hat,
                         const float* v_hat, const float* sigma, float* dw, int rows, int cols,
                         void* ws, size_t ws_bytes, void* stream);

/* Multi-tensor form: every spectrally-normalised weight of one network in 4 (fwd) / 2 (bwd) launches.
 * The BgSnItem table lives in device memory (pointers are stable: flat arenas); ws_offset is the byte
 * offset (16-byte aligned) of the item's scratch of bg_spectral_norm_workspace_bytes(rows, cols) bytes
 * inside ws; fwd zeroes ws[0, ws_bytes).  u is updated in place.  bwd: bit i of enable_mask /
 * accumulate_mask (host arrays of ceil(n/64) words; NULL = all / none) selects whether item i is
 * processed and whether dw is added to instead of overwritten; ws >= 8 * n_items bytes. */
typedef struct BgSnItem {
    const float* w;        /* [rows, cols] */
    float* u;              /* [cols], in/out */
    float* v;              /* [rows], out */
    float* sigma;          /* [1], out */
    float* w_norm;         /* [rows, cols], out */
    const float* g_wnorm;  /* bwd in: dL/d(w_norm) */
    float* dw;             /* bwd out: dL/dw */
    int64_t ws_offset;
    int32_t rows, cols;
    /* bf16-resident path (optional, NULL otherwise): the weight seen as [taps][rows / taps][cols];
     * pack_p[tap][r][c] = pack_t[tap][c][r] = bf16(w[tap][r][c] / sigma).  rows / taps and cols must be even. */
    void* pack_p;
    void* pack_t;
    int32_t taps;
    int32_t pack_p_ld;     /* elements between rows of pack_p (0 = cols): kernels that share one GEMM (the f|g|h 1x1
                            * projections of self_attention_2) write column slices of a common [rows][sum cols] copy;
                            * their pack_t copies are row blocks of a common [sum cols][rows] matrix (plain offsets) */
} BgSnItem;
int bg_spectral_norm_batch_fwd(const BgSnItem* items_dev, int n_items, void* ws, size_t ws_bytes, void* stream);
/* The same in two halves, for data parallelism (last row: the batch-independent power iteration is
 * SHARDED by weight instead of repeated on every rank):
 *   BG_SN_POWER      the two GEMV passes + finalisation of the items given (a rank's OWN weights: a sub-table): writes
 *                    u (in place), sigma and v_hat of those items - nothing else
 *   BG_SN_NORMALIZE  w / sigma (+ packed bf16 copies) of the items given (ALL weights), sigma read from each item's
 *                    sigma slot - filled for the other ranks' weights by an all-gather of sigma | u | v_hat in between
 *   BG_SN_ALL        both, = bg_spectral_norm_batch_fwd */
#define BG_SN_ALL 0
#define BG_SN_POWER 1
#define BG_SN_NORMALIZE 2
int bg_spectral_norm_batch_phase(const BgSnItem* items_dev, int n_items, void* ws, size_t ws_bytes, int phase,
                                 void* stream);
int bg_spectral_norm_batch_bwd(const BgSnItem* items_dev, int n_items, const uint64_t* enable_mask,
                               const uint64_t* accumulate_mask, void* ws, size_t ws_bytes, void* stream);

/* Forward-mode tangent of TRAINING-mode batch norm and its backward: the gradient penalty (BigGAN.py:717-742) through a
 * discriminator with --bn_in_d (ops.py:546-561).  x, xd, s are [rows, C] fp32.
 *   bg_chan_dots3            sums[0:C] = sum p, [C:2C] = sum p q, [2C:3C] = sum p r (r may be NULL: zeros) in fp64; the
 *                            call zeroes sums itself and overwrites all 3C entries (the caller all-reduces them under
 *                            data parallelism)
 *   bg_bn_tangent_fwd_coefs  from sums(p = xd, q = x): coefs[3C] with yd = coefs[0] xd + coefs[1] x + coefs[2] and m12[2C] =
 *                            (mean(xd) | mean(xd xhat)), kept for the backward
 *   bg_bn_tangent_bwd_coefs  from sums(p = s, q = x, r = xd), s = dL/dyd: coefs_dxd[3C] (d_xd = . s + . x + .), coefs_dx[4C]
 *                            (d_x = . s + . x + . xd + .) and dgamma[C]
 *   bg_chan_lincomb3         out = cp[c] p + cq[c] q (+ cr[c] r) + c0[c] */
int bg_chan_dots3(const float* p, const float* q, const float* r, double* sums, int64_t rows, int C, void* stream);
int bg_bn_tangent_fwd_coefs(const double* sums, double count, const float* mean, const float* rstd, const float* gamma,
                            float* coefs, float* m12, int C, void* stream);
int bg_bn_tangent_bwd_coefs(const double* sums, double count, const float* mean, const float* rstd, const float* gamma,
                            const float* m12, float* coefs_dxd, float* coefs_dx, float* dgamma, int C, void* stream);
int bg_chan_lincomb3(const float* p, const float* cp, const float* q, const float* cq, const float* r, const float* cr,
                     const float* c0, float* out, int64_t rows, int C, void* stream);

/* Gram matrix out[c1][c2] = sum_r a[r][c1] * a[r][c2] (fp32, [cols][cols]) of a bf16 row-major matrix a[rows][ld]:
 * the ortho-cosine regulariser's W^T W (utils.py:198) from the packed bf16 copy of w / sigma (BgSnItem.pack_p); the caller
 * rescales by sigma^2.  cols % 8 == ld % 8 == 0; ws from bg_gram16_workspace_bytes (split-K slabs). */
size_t bg_gram16_workspace_bytes(int rows, int cols);
int bg_gram16(const void* a, int rows, int cols, int ld, float* out, void* ws, size_t ws_bytes, void* stream);

/* --------------------------------------------------------------------------------------------
 * Batch statistics + (conditional) batch-norm + PReLU (ops.py:532-537, 580-585, 611-643).
 *   x [N,HW,C].  stats: sums[0:C] = sum x, sums[C:2C] = sum x^2 over N*HW (fp64 accumulators, so the
 *   result does not depend on the arrival order of the blocks' atomics; caller zeroes or
 *   all-reduces them for cross-replica BN), then bg_bn_finalize turns sums into mean / rstd
 *   (biased variance, eps) and updates the moving statistics.
 *   apply: y = act((x - mean) * rstd * gamma + beta), gamma/beta per sample [N,C] (per_sample=1,
 *   condition_batch_norm) or per channel [C] (tf.layers.batch_normalization);
 *   act = PReLU with per-channel alpha when alpha != NULL (ops.py:535-537), identity otherwise.
 *   The entries that take activation tensors (here and below: PReLU, pooling, bg_bias_grad) forward to their "_t"
 *   forms with BG_F32 - see "bf16-resident data path".
 * ------------------------------------------------------------------------------------------ */
int bg_bn_stats(const float* x, double* sums, int64_t rows, int C, void* stream);
/* mean = sums[0:C] / count and var = sums[C:2C] / count - mean^2 are formed in fp64 (a negative var is clamped to 0),
 *   rstd = 1/sqrt((float) var + eps).  moving_mean / moving_var are nullable, each on its own: a non-NULL one moves to
 *   moving * momentum + new * (1 - momentum), new = mean | var (times count / (count - 1) when unbiased_moving_var and
 *   count > 1). */
int bg_bn_finalize(const double* sums, double count, float eps, float momentum, int unbiased_moving_var,
                   float* mean, float* rstd, float* moving_mean, float* moving_var, int C, void* stream);
/* inference (ops.py:640-643): mean = pop_mean, rstd = 1/sqrt(pop_var + eps) for the apply kernel below */
int bg_bn_population(const float* pop_mean, const float* pop_var, float eps, float* mean, float* rstd, int C,
                     void* stream);
int bg_bn_apply_act_fwd(const float* x, const float* mean, const float* rstd,
                        const float* gamma, const float* beta, int per_sample,
                        const float* alpha, float* y, int N, int HW, int C, void* stream);
/* backward, pass 1: per-(sample,channel) reductions
 *   part[0][n][c] = sum_hw g, part[1][n][c] = sum_hw g * xhat, part[2][n][c] = sum_hw dy * min(pre,0)
 *   where pre = xhat*gamma+beta, g = dy * act'(pre).            part is [3,N,C] fp32 */
int bg_bn_apply_act_bwd_reduce(const float* x, const float* dy, const float* mean, const float* rstd,
                               const float* gamma, const float* beta, int per_sample,
                               const float* alpha, float* part, int N, int HW, int C, void* stream);
/* backward, pass 2: dx = rstd * (g*gamma - m1 - xhat * m2), m1 = mean(g*gamma), m2 = mean(g*gamma*xhat)
 *   given as per-channel device vectors cm[0:C] = m1, cm[C:2C] = m2 (caller reduces part over N,
 *   and across ranks for cross-replica BN). */
int bg_bn_apply_act_bwd_dx(const float* x, const float* dy, const float* mean, const float* rstd,
                           const float* gamma, const float* beta, int per_sample,
                           const float* alpha, const float* cm, float* dx,
                           int N, int HW, int C, void* stream);
/* reduce part[3,N,C] -> dgamma/dbeta (per sample: [N,C] copies of part1 / part0; per channel: [C] sums over N),
 *   dalpha[C] = sum_n part2_n (nullable: plane 2 is then not summed into anything),
 *   cm[2C] = (sum_n gamma_n * part0_n, sum_n gamma_n * part1_n) / count; sums in fp64, rounded once */
int bg_bn_bwd_finalize(const float* part, const float* gamma, int per_sample, double count,
                       float* dgamma, float* dbeta, float* dalpha, float* cm, int N, int C, void* stream);

/* Batch renormalisation (ops.py:600-609 tf.layers.batch_normalization(renorm=True); ops.py:645-715
 * condition_batch_renorm).  The normalisation itself is the batch-norm above with the affine pair replaced by
 *   gamma_eff = r * gamma ,  beta_eff = beta + d * gamma        (r, d per channel, constants for the gradient)
 * bg_renorm_coeffs turns the batch sums of bg_bn_stats into the clipped corrections, measured against running
 * statistics that are read BEFORE any update of this run:
 *   sigma = sqrt(var + eps) ; sigma_ref = sqrt(ref_scale + eps)            (scale_is_var = 1, ops.py:688-689)
 *                             sigma_ref = max(ref_scale, sqrt(eps))        (scale_is_var = 0, Keras renorm_stddev)
 *   sigma_w = w * sigma_ref + (1-w) * sigma ;  mean_w = w * ref_mean + (1-w) * mean     (ops.py:690-691;
 *             w = *weight, or 1 when weight == NULL: --bn_renorm_shared / Keras)
 *   r = clip(sigma / sigma_w, rmin, rmax) ;  d = clip((mean - mean_w) / sigma_w, -dmax, dmax)   (ops.py:692-693)
 * update = 1 also moves the running statistics (ops.py:701-703):
 *   ref_mean  <- ref_mean  * decay + mean * (1-decay)
 *   ref_scale <- ref_scale * decay + (scale_is_var ? var : sigma) * (1-decay)
 *   *weight   <- *weight * fadein_decay + (1 - fadein_decay)
 * bg_renorm_affine_fwd/bwd: the [rows, C] (conditional, rows = batch) or [1, C] affine pair and the gradient
 *   dgamma = r * dgamma_eff + d * dbeta_eff   (dbeta = dbeta_eff). */
int bg_renorm_coeffs(const double* sums, double count, float* ref_mean, float* ref_scale, int scale_is_var,
                     float* weight, float eps, float rmin, float rmax, float dmax, float decay, float fadein_decay,
                     int update, float* r, float* d, int C, void* stream);
int bg_renorm_affine_fwd(const float* gamma, const float* beta, const float* r, const float* d,
                         float* gamma_eff, float* beta_eff, int64_t rows, int C, void* stream);
int bg_renorm_affine_bwd(const float* dgamma_eff, const float* dbeta_eff, const float* r, const float* d,
                         float* dgamma, int64_t rows, int C, void* stream);

/* stand-alone PReLU (ops.py:532-537): y = x>0 ? x : alpha_c*x ; bwd returns dx and per-channel
 * partial dalpha accumulated with atomics into dalpha[C] (caller zeroes). */
int bg_prelu_fwd(const float* x, const float* alpha, float* y, int64_t rows, int C, void* stream);
int bg_prelu_bwd(const float* x, const float* dy, const float* alpha, float* dx, float* dalpha,
                 int64_t rows, int C, void* stream);

/* tf.layers.max_pooling2d(2,2,'SAME') on even H,W (ops.py:508-510); bwd routes to the first max */
int bg_maxpool2_fwd(const float* x, float* y, int N, int H, int W, int C, void* stream);
int bg_maxpool2_bwd(const float* x, const float* dy, float* dx, int N, int H, int W, int C, void* stream);
/* 2x2 stride-2 box kernels (x is [N,H,W,C] for both): bg_box2_down: y[N,H/2,W/2,C] = scale * sum of each 2x2
 * block (avg_pooling forward with scale 1/4, ops.py:512-514; up_sample backward with scale 1);
 * bg_box2_up: y[N,2H,2W,C] = scale * x replicated 2x2 (up_sample = resize_nearest_neighbor x2 forward with
 * scale 1, ops.py:516-519; avg_pooling backward with scale 1/4). */
/* C % 4 == 0 takes 16-byte accesses: x and y must then be 16-byte aligned (BG_ERR_ARG otherwise; any other C: 4). */
int bg_box2_down(const float* x, float* y, int N, int H, int W, int C, float scale, void* stream);
int bg_box2_up(const float* x, float* y, int N, int H, int W, int C, float scale, void* stream);

/* tf.nn.softmax over the last axis (ops.py:483): rows x cols, cols <= 1024 (more: BG_ERR_UNSUPPORTED, nothing is launched;
 * the same holds for bg_softmax_tangent_bwd), in place allowed (p == s); bwd: ds = p*(dp - sum(dp*p)) */
int bg_softmax_fwd(const float* s, float* p, int64_t rows, int cols, void* stream);
int bg_softmax_bwd(const float* p, const float* dp, float* ds, int64_t rows, int cols, void* stream);

/* tf.reduce_sum(x,[1,2]) (ops.py:503-506) and its gradient (broadcast) */
int bg_sum_pool_fwd(const float* x, float* y, int N, int HW, int C, void* stream);
int bg_sum_pool_bwd(const float* dy, float* dx, int N, int HW, int C, void* stream);

/* y = a*x + b*y elementwise family used by residual adds, gamma*o + x (ops.py:490), tanh (ops.py:539).
 * bg_axpby reads y only when b != 0; in place allowed: x == y of bg_axpby (y = (a + b) y), a == y of bg_add, y == x
 * of bg_scale_dev.  Every other pair of arguments must not overlap.  bg_axpby / bg_add / bg_scale_add take 16-byte
 * aligned pointers (BG_ERR_ARG otherwise). */
int bg_axpby(const float* x, float a, float* y, float b, int64_t n, void* stream);
int bg_add(const float* a, const float* b, float* y, int64_t n, void* stream);            /* y = a + b */
int bg_scale_add(const float* o, const float* gamma_dev, const float* x, float* y, int64_t n, void* stream);
int bg_dot(const float* a, const float* b, float* out_accum, int64_t n, void* stream);   /* out += <a,b> */
int bg_scale_dev(const float* x, const float* s_dev, float* y, int64_t n, void* stream);  /* y = s*x, s a device scalar; in place allowed (y == x) */
int bg_tanh_fwd(const float* x, float* y, int64_t n, void* stream);
int bg_tanh_bwd(const float* y, const float* dy, float* dx, int64_t n, void* stream);
int bg_bias_grad(const float* dy, float* db, int64_t rows, int C, void* stream);         /* db[c] = sum_rows dy */

/* --------------------------------------------------------------------------------------------
 * RGBA images (--c_dim 4; alpha.hip).  fp32 NHWC tensors of `rows` pixels x 4 channels (r, g, b, a), 16-byte aligned.
 *   alpha helper (BigGAN.py:572-580), between G_logit and tanh, with w = generator/alphahelper_w ([] in device memory):
 *     y = tanh(r, g, b, a + w (r + g + b + a))   (the sum includes the alpha logit itself)
 *   bwd, one pass with g = dy (1 - y^2) (y recomputed from x): dx_c = g_c + w g_a (colour), dx_a = g_a (1 + w);
 *     dw_accum[0] += sum over pixels of g_a (r + g + b + a): per-block fp64 partials added in a fixed order, no
 *     atomics (dw_accum NULL: no weight gradient).
 *   alpha mask (BigGAN.py:616-619), D's input: rgb' = (rgb + 1)(a + 1)/2 - 1, alpha unchanged;
 *     bwd: dx_rgb = dy_rgb (a + 1)/2, dx_a = dy_a + sum_c dy_c (rgb_c + 1)/2;
 *     tangent (forward mode, the gradient penalty's pass): ydot_rgb = (xdot_rgb (a + 1) + (rgb + 1) xdot_a)/2,
 *     ydot_a = xdot_a.
 * ------------------------------------------------------------------------------------------ */
int bg_alpha_head_fwd(const float* x, const float* w, float* y, int64_t rows, void* stream);
int bg_alpha_head_bwd(const float* x, const float* w, const float* dy, float* dx, float* dw_accum, int64_t rows,
                      void* stream);
int bg_alpha_mask_fwd(const float* x, float* y, int64_t rows, void* stream);
int bg_alpha_mask_bwd(const float* x, const float* dy, float* dx, int64_t rows, void* stream);
int bg_alpha_mask_tangent(const float* x, const float* xdot, float* ydot, int64_t rows, void* stream);

/* --------------------------------------------------------------------------------------------
 * bf16-resident data path (BASELINE configs 3-5): "_t" forms of the bandwidth-bound kernels above.  Activation
 * tensors are fp32 or bf16 in HBM (dtype arguments: BG_F32 / BG_BF16), arithmetic is fp32 in registers, parameters,
 * statistics and reductions stay fp32 / fp64.  x_dtype names the op's INPUT-side tensors (x, dx), y_dtype its
 * OUTPUT-side tensors (y, dy).  Any C > 0: with C % 8 == 0 and every activation pointer on a 16-byte boundary the
 * all-bf16 calls move 16 bytes per access; with C % 4 == 0 a bf16 tensor needs 8-byte alignment only (8-byte
 * accesses) - except column reductions (statistics, backward reduce, dalpha, bias gradient) over 16 Mi elements or
 * more, which read 16 bytes at C % 8 == 0 and need 16-byte alignment; any other C (the image layers' 3 and 6) goes one
 * element per thread.  fp32 tensors: 16-byte aligned when C % 4 == 0.  bg_lincomb_t / bg_dot_t: n % 4 == 0, bf16
 * tensors 8-byte aligned.  tests/test_gpu_elementwise16.py holds every one of these forms to a float64 reference.
 * These ARE the implementation of the fp32 entry points of the same name (bg_bn_stats, bg_bn_apply_act_fwd /
 * _bwd_reduce / _bwd_dx, bg_prelu_fwd / _bwd, bg_bias_grad, bg_maxpool2_fwd / _bwd, bg_sum_pool_fwd / _bwd): each of
 * those calls its "_t" entry with BG_F32 and dx_add = NULL, so a call it rejects names the "_t" entry in
 * bg_last_error.  bg_dot runs bg_dot_t's kernel too but keeps its own check: it takes any n.  An fp32 / fp32
 * bg_prelu_bwd(_t) with C <= 4 and rows >= 65536 (the PReLU of the image) sums dalpha with whole pixels per thread.
 * ------------------------------------------------------------------------------------------ */
int bg_cast(const void* x, int x_dtype, void* y, int y_dtype, int64_t n, void* stream);
/* tf.nn.depth_to_space (ops.py:27) and its inverse / adjoint, NHWC, block size r (csrc/subpixel.hip):
 *   bg_depth_to_space: x[N,H,W,r*r*C] -> y[N,r*H,r*W,C],  y[n, h*r+i, w*r+j, c] = x[n, h, w, (i*r+j)*C + c]
 *   bg_space_to_depth: x[N,r*H,r*W,C] -> y[N,H,W,r*r*C]   (H, W: the LOW-resolution map in both calls)
 * Pure permutations of BG_F32 or BG_BF16 tensors (bit-exact); C * element size must be a multiple of 16 bytes
 * (C % 8 == 0 for bf16, C % 4 == 0 for fp32): a run of C channels stays contiguous and moves in 16-byte pieces. */
int bg_depth_to_space(const void* x, void* y, int dtype, int N, int H, int W, int C, int r, void* stream);
int bg_space_to_depth(const void* x, void* y, int dtype, int N, int H, int W, int C, int r, void* stream);
/* Widen or narrow the middle dimension of an [outer][C][inner] view from Cs to Cd entries, converting between fp32 and
 * bf16: the 3-channel image layers (ops.py:49 with Cin = 3, BigGAN.py:570 with Cout = 3) run on the bf16-resident GEMMs
 * with the thin side widened to 8 channels.  mode BG_PAD_ZERO_FILL (0): dst[c] = c < Cs ? src[c] : 0;
 * BG_PAD_SPLIT (1, Cd >= 2 Cs): dst[c] = bf16(src[c]), dst[Cs + c] = src[c] - bf16(src[c]) - the idle padding channels
 * carry the rounding residual, so the MFMA sees the thin operand to ~16 mantissa bits; BG_PAD_DUP (2): dst[c] =
 * dst[Cs + c] = src[c] (the partner operand of a split one); BG_PAD_FOLD (3, Cs >= 2 Cd): dst[c] = src[c] + src[Cd + c]. */
enum { BG_PAD_ZERO_FILL = 0, BG_PAD_SPLIT = 1, BG_PAD_DUP = 2, BG_PAD_FOLD = 3 };
int bg_pad_channels(const void* src, int src_dtype, void* dst, int dst_dtype, int64_t outer, int Cs, int Cd,
                    int64_t inner, int mode, void* stream);
/* the two packed bf16 copies of a conv kernel that is NOT spectrally normalised (see BgSnItem::pack_p / pack_t) */
int bg_weight_pack(const float* w, int taps, int rows_per_tap, int cols, void* pack_p, void* pack_t, void* stream);
int bg_bn_stats_t(const void* x, int x_dtype, double* sums, int64_t rows, int C, void* stream);
int bg_bn_apply_act_fwd_t(const void* x, int x_dtype, const float* mean, const float* rstd, const float* gamma,
                          const float* beta, int per_sample, const float* alpha, void* y, int y_dtype,
                          int N, int HW, int C, void* stream);
int bg_bn_apply_act_bwd_reduce_t(const void* x, int x_dtype, const void* dy, int y_dtype, const float* mean,
                                 const float* rstd, const float* gamma, const float* beta, int per_sample,
                                 const float* alpha, float* part, int N, int HW, int C, void* stream);
int bg_bn_apply_act_bwd_dx_t(const void* x, int x_dtype, const void* dy, int y_dtype, const float* mean,
                             const float* rstd, const float* gamma, const float* beta, int per_sample,
                             const float* alpha, const float* cm, void* dx, const void* dx_add, int N, int HW, int C,
                             void* stream);      /* dx_add (x_dtype, nullable, may alias dx): dx = dx_add + gradient - the
                                                    sum of the two branch gradients of a forked tensor, fused */
int bg_prelu_fwd_t(const void* x, int x_dtype, const float* alpha, void* y, int y_dtype, int64_t rows, int C,
                   void* stream);
/* dx (x_dtype, nullable) and / or dalpha (fp32 [C], accumulated: caller zeroes; nullable); dx_add as above */
int bg_prelu_bwd_t(const void* x, int x_dtype, const void* dy, int y_dtype, const float* alpha, void* dx,
                   float* dalpha, const void* dx_add, int64_t rows, int C, void* stream);
int bg_bias_grad_t(const void* dy, int dtype, float* db, int64_t rows, int C, void* stream);
int bg_maxpool2_fwd_t(const void* x, void* y, int dtype, int N, int H, int W, int C, void* stream);
int bg_maxpool2_bwd_t(const void* x, const void* dy, void* dx, int dtype, int N, int H, int W, int C, void* stream);
int bg_sum_pool_fwd_t(const void* x, int x_dtype, float* y, int N, int HW, int C, void* stream);
int bg_sum_pool_bwd_t(const float* dy, void* dx, int x_dtype, int N, int HW, int C, void* stream);
/* y = s * a + sb * b with s = *sa_dev (device scalar) when sa_dev != NULL, else sa; b may be NULL (y = s * a):
 * residual adds, gamma * o + x (ops.py:490), scaling by a device scalar.  n % 4 == 0. */
int bg_lincomb_t(const void* a, const float* sa_dev, float sa, const void* b, float sb, void* y, int dtype,
                 int64_t n, void* stream);
int bg_dot_t(const void* a, const void* b, int dtype, float* out_accum, int64_t n, void* stream);  /* out += <a,b> */

/* --------------------------------------------------------------------------------------------
 * DiffAugment 'color,translation,cutout' (DiffAugment_tf.py:8-73), x [N,S,S,C] fp32.
 *   policy bit 0 = color, 1 = translation, 2 = cutout.  Draws are explicit device arrays:
 *   u_b,u_s,u_c float[N] in [0,1); t_x,t_y int32[N] in [-shift,shift]; o_x,o_y int32[N].
 *   mean_ws: N doubles scratch (per-sample sums for rand_contrast).  Integer index math is
 *   bit-exact with DiffAugment_tf.py:40-66.
 * ------------------------------------------------------------------------------------------ */
int bg_diffaugment_fwd(const float* x, float* y, const float* u_b, const float* u_s, const float* u_c,
                       const int32_t* t_x, const int32_t* t_y, const int32_t* o_x, const int32_t* o_y,
                       int N, int S, int C, int policy, double* mean_ws, void* stream);
int bg_diffaugment_bwd(const float* dy, float* dx, const float* u_s, const float* u_c,
                       const int32_t* t_x, const int32_t* t_y, const int32_t* o_x, const int32_t* o_y,
                       int N, int S, int C, int policy, double* mean_ws, void* stream);

/* --------------------------------------------------------------------------------------------
 * Hinge losses with flood (ops.py:788-797, 832-840, 847-848).
 *   sums: device float accumulators (caller zeroes; all-reduced across ranks for DP):
 *     D (float[2]): sums[0] += sum relu(1-real), sums[1] += sum relu(1+fake);   G (float[1]): sums[0] += sum fake
 *   grad kernels read the (global) sums, n_global = global batch, and write the flooded loss
 *   (loss_out[0], nullable) and d(loss)/d(logit); where the loss equals flood exactly the gradient is +-0.
 * ------------------------------------------------------------------------------------------ */
int bg_hinge_d_sums(const float* real, const float* fake, float* sums, int n, void* stream);
int bg_hinge_d_grad(const float* real, const float* fake, const float* sums, double n_global, float flood,
                    float* d_real, float* d_fake, float* loss_out, int n, void* stream);
int bg_hinge_g_sums(const float* fake, float* sums, int n, void* stream);
int bg_hinge_g_grad(const float* sums, double n_global, float flood, float* d_fake, float* loss_out,
                    int n, void* stream);

/* General GAN losses (ops.py:753-840): kind 0 hinge, 1 lsgan, 2 gan (also 'dragan'), 3 ra-lsgan, 4 ra-gan (also
 * 'ra-dragan'), 5 ra-hinge, 6 wgan (wgan-gp / wgan-lp); generator = 0 for discriminator_loss, 1 for generator_loss.  Three steps so that data-parallel
 * ranks can exchange the sums in between:  bg_gan_loss_means -> sums = {sum real, sum fake} (OVERWRITTEN - the hinge
 * pair above accumulates, this one does not; sum real = 0 for nr = 0; tsums below is overwritten as well);
 * bg_gan_loss_terms (given the GLOBAL sums / counts) -> tsums = {sum phi_r, sum phi_f, sum phi_r', sum phi_f'};
 * bg_gan_loss_grad (given the GLOBAL tsums) -> loss (flooded), d_real, d_fake (incl. the coupling through the
 * batch means of the relativistic kinds).  real may be NULL with nr = 0 (non-relativistic generator losses; d_real is
 * then not written).  loss_out may be NULL. */
int bg_gan_loss_means(const float* real, const float* fake, float* sums, int nr, int nf, void* stream);
int bg_gan_loss_terms(int kind, int generator, const float* real, const float* fake, const float* sums,
                      double n_real_global, double n_fake_global, float* tsums, int nr, int nf, void* stream);
int bg_gan_loss_grad(int kind, int generator, const float* real, const float* fake, const float* sums,
                     const float* tsums, double n_real_global, double n_fake_global, float flood, float* d_real,
                     float* d_fake, float* loss_out, int nr, int nf, void* stream);

/* --------------------------------------------------------------------------------------------
 * Gradient penalty (BigGAN.py:717-742) and the second-order pieces it needs.
 *   GP = ld * mean_n phi(||g_n||),  g = d sum(D(aug(x^)))/d x^,  phi = (n-1)^2 (wgan-gp, dragan) or max(0,n-1)^2 (wgan-lp).
 *   Its parameter gradient is taken as the gradient of the directional derivative of D along the constant
 *   direction v_n = ld * phi'(||g_n||) / count * g_n / ||g_n||  (d GP/d theta = d <g(theta), v>/d theta), i.e. by
 *   differentiating a forward-mode (tangent) pass of the discriminator; the entries below are the tangent maps that
 *   are not already linear kernels of this library, and their derivatives.
 * bg_gp_interpolate: x^ = real + alpha_n (other - real)           (sums == NULL; other = fake: BigGAN.py:726-727)
 *                    x^ = real + alpha_n * 0.5 * std(real) * other (sums = {sum real, sum real^2} in fp64 from
 *                         bg_bn_stats with C = 1, count = numel: BigGAN.py:719-724, other = eps ~ U[0,1))
 * bg_gp_penalty: g [N, per] -> *loss = ld * sum_n phi(||g_n||) / count_global (this rank's share of the mean),
 *                v = the direction above (a row of norm 0 gets v = 0); ws: 2*N doubles, zeroed by the call: on return
 *                ws[0:N] = ||g_n||^2 and ws[N:2N] = the factor of g_n in v_n; lp = 1 selects wgan-lp.
 * bg_maxpool2_gather: tangent of the 2x2 max pool, y = t at the first maximum of x's window (its transpose is
 *                bg_maxpool2_bwd).
 * bg_prelu_tangent_dalpha: the PReLU tangent is ydot = xdot * prelu'(x) (computed by bg_prelu_bwd with dy := xdot);
 *                its derivative w.r.t. alpha is dalpha[c] = sum_rows dy * xdot * [x < 0]  (1/2 at x == 0); dalpha is
 *                overwritten (the call zeroes it; bg_prelu_bwd_t's dalpha accumulates).
 * bg_softmax_tangent_bwd: the softmax tangent is pdot = p * (sdot - sum p sdot) (computed by bg_softmax_bwd with
 *                dp := sdot); given g = dL/dpdot:  dsdot = p * (g - u), dp = g * (sdot - t) - u * sdot,
 *                t = sum p sdot, u = sum g p (row sums).
 * ------------------------------------------------------------------------------------------ */
int bg_gp_interpolate(const float* real, const float* other, const float* alpha, const double* sums, double count,
                      float* out, int N, int64_t per, void* stream);
int bg_gp_penalty(const float* g, int N, int64_t per, double count_global, float ld, int lp, double* ws, float* loss,
                  float* v, void* stream);
int bg_maxpool2_gather(const float* x, const float* t, float* y, int N, int H, int W, int C, void* stream);
int bg_prelu_tangent_dalpha(const float* x, const float* xdot, const float* dy, float* dalpha, int64_t rows, int C,
                            void* stream);
int bg_softmax_tangent_bwd(const float* p, const float* sdot, const float* g, float* dp, float* dsdot, int64_t rows,
                           int cols, void* stream);

/* Class-label loss of the conditional model (utils.py:366-369, BigGAN.py:853,894), 'logistic' type:
 *   loss = scale * sum_{b,j} sigmoid_cross_entropy_with_logits(truth, logits)[b,j] * weights[j]
 *   dlogits = scale * weights[j] * (sigmoid(logits) - truth);  scale = loss_weight / (global_batch * n).
 *   weights may be NULL (all ones).  logits/truth/dlogits are [B, n]. */
int bg_sigmoid_ce(const float* logits, const float* truth, const float* weights, float scale, float* loss_out,
                  float* dlogits, int B, int n, void* stream);

/* --------------------------------------------------------------------------------------------
 * Labelled datasets (csrc/labels.hip): the sliced label loss of --cls_loss_type (utils.py:339-375) and the draw of the
 * generator's fake labels from the dataset's label table (BigGAN.py:1447-1455).
 *   A spec "N-type,M-type,..." (or a plain 'logistic' / 'euclidean' = one slice of all n columns) splits the columns of
 *   logits / truth [B, n] and weights [n] into n_slices contiguous slices.  Device-resident description, uploaded once:
 *     slices    int32 [n_slices, 2] = (kind, size), kind 0 = logistic, 1 = euclidean;
 *     col_slice int32 [n]           = slice index of every column, non-decreasing.
 *   With rows_global = the batch of all ranks, the loss is loss_weight * sum_s L_s,
 *     logistic : L_s = sum_{b,j in s} sigmoid_cross_entropy_with_logits(t, x)[b,j] * w_j / (rows_global * size_s)
 *     euclidean: L_s = sqrt(sum_{b,j in s} ((x[b,j] - t[b,j]) * w_j)^2)                 (one norm, not a mean)
 * bg_label_loss_sums: sums[s] += this rank's share of the weighted cross-entropy sum (logistic) or of the sum of squares
 *   (euclidean): fp32 terms, fp64 accumulators.  sums [n_slices] fp64 must be zero on entry; a data-parallel run
 *   all-reduces it (SUM) between the two calls, so the square root is taken of the global sum of squares.
 * bg_label_loss_finish: *loss_out = loss_weight * sum_s L_s (the same value on every rank) and the derivative of that
 *   global loss with respect to the local logits,
 *     dlogits[b,j] = loss_weight * w_j * (sigmoid(x) - t) / (rows_global * size_s)        logistic
 *                  = loss_weight * w_j^2 * (x - t) / sqrt(sums[s])                        euclidean,
 *   0 where sums[s] == 0 (TensorFlow's sqrt gradient gives NaN there).
 * Neither call synchronises or reads anything back; both can be captured.
 * bg_gather_rows: out[b, :] = table[idx[b], :], bit-exact; table fp32 [rows, n], idx int64 [B] on the device, any
 *   n >= 1 and rows >= 1.  An index outside [0, rows) is clamped into the table.
 * ------------------------------------------------------------------------------------------ */
int bg_label_loss_sums(const float* logits, const float* truth, const float* weights, const int32_t* slices,
                       const int32_t* col_slice, double* sums, int B, int n, int n_slices, void* stream);
int bg_label_loss_finish(const float* logits, const float* truth, const float* weights, const int32_t* slices,
                         const int32_t* col_slice, const double* sums, double rows_global, float loss_weight,
                         float* loss_out, float* dlogits, int B, int n, int n_slices, void* stream);
int bg_gather_rows(const float* table, const int64_t* idx, float* out, int rows, int n, int B, void* stream);

/* --------------------------------------------------------------------------------------------
 * Orthogonal-cosine regulariser (utils.py:180-235) from the Gram matrix A = W^T W [c,c]
 * (computed with bg_gemm), using R[i,j] = (sum_k Ahat[i,k] - Ahat[i,j]) / sqrt(c-1):
 *   fwd: loss_accum[0] += scale/2 * sum R^2 ; bwd: dA (so that dW = W (dA + dA^T), via bg_gemm).
 * ------------------------------------------------------------------------------------------ */
int bg_ortho_cosine_fwd_bwd(const float* A, float scale, float* loss_accum, float* dA, int c, void* stream);
/* type 'ortho' (utils.py:199-200): loss_accum += scale/2 * sum (A - I)^2, dA = scale * (A - I). */
/* S = A + A^T (c x c, out of place): d(loss)/dW = W dA + W dA^T = W S, one GEMM instead of two (utils.py:197-203) */
int bg_symmetrize(const float* A, float* S, int c, void* stream);
int bg_ortho_identity_fwd_bwd(const float* A, float scale, float* loss_accum, float* dA, int c, void* stream);
/* Low-rank form of the same function for wide kernels W[rows, c] with rows < c (first/dense2 is
 * [184, 16*16*ch]): with G = W W^T, s = W 1, P = G W (bg_gemm) the c x c Gram matrix is never formed.
 *   cols:   alpha_beta[0:c] = alpha, [c:2c] = beta, Wb = W diag(beta), loss_accum[0] += loss
 *   finish: dW = 2*dW_in + s alpha^T + (W alpha) 1^T + 2 P diag(beta), dW_in = (Wb W^T) W */
/* out[r] = sum_c W[r,c] * v[c] (v == NULL: row sums) - the s = W 1 and W alpha vectors of the low-rank form */
int bg_gemv_rows(const float* w, const float* v, float* out, int rows, int cols, void* stream);
int bg_ortho_lowrank_cols(const float* W, const float* P, const float* s, float scale, float* alpha_beta,
                          float* Wb, float* loss_accum, int rows, int c, void* stream);
int bg_ortho_lowrank_finish(float* dW, const float* P, const float* s, const float* Walpha,
                            const float* alpha_beta, int rows, int c, void* stream);

/* --------------------------------------------------------------------------------------------
 * TF AdamOptimizer (+ MovingAverageOptimizer shadow) over a flat parameter arena (BigGAN.py:923-927):
 *   m = b1 m + (1-b1) g; v = b2 v + (1-b2) g^2; p -= lr_t * m / (sqrt(v) + eps);
 *   lr_t = lr sqrt(1-b2^t)/(1-b1^t) computed by the caller; ema (nullable) = d*ema + (1-d)*p.
 *   grad_scale multiplies g first (1/world_size for summed all-reduce).
 * ------------------------------------------------------------------------------------------ */
int bg_adam_tf_ema_step(float* p, const float* g, float* m, float* v, float* ema,
                        float lr_t, float b1, float b2, float eps, float ema_decay, float grad_scale,
                        int64_t n, void* stream);
/* Same update with the bias-corrected step size read from device memory (lr_t_dev[0]): the launch carries no
 * per-step host scalar, so a captured HIP graph of the training step can be replayed. */
int bg_adam_tf_ema_step_dev(float* p, const float* g, float* m, float* v, float* ema, const float* lr_t_dev,
                            float b1, float b2, float eps, float ema_decay, float grad_scale, int64_t n,
                            void* stream);

/* --------------------------------------------------------------------------------------------
 * Discriminator reconstruction heads (BigGAN.py:639-661, 744-762, 810-836; csrc/recon.hip).  dtype = BG_F32 / BG_BF16;
 * 16-byte accesses when C is a multiple of 4 (fp32) / 8 (bf16) and the tensors are 16-byte aligned, scalar otherwise.
 * bg_glu_*: ops.py:842-845, x[rows, 2C] -> y[rows, C] = x[:, :C] * sigmoid(x[:, C:]); bwd writes dx for both halves.
 * bg_upsample2_*_t: nearest-neighbour 2x (ops.py:516-519), x[N,H,W,C] -> y[N,2H,2W,C]; bwd = 2x2 box sum (fp32 sum,
 *   one rounding).
 * bg_crop_at_*: y[N,p,p,C] = x[N, oy:oy+p, ox:ox+p, C] with oy = off_y[0], ox = off_x[0] read on the DEVICE (clamped to
 *   [0, H-p] / [0, W-p]); bwd writes all of dx (zero outside the window).
 * bg_recon_loss_*: y[N,h,w,C] pre-tanh, target[N,S,S,C] fp32; mode 0: target itself (S == h), 1: its 2x2 average
 *   (S == 2h), 2: its crop at (off_y[0]*f, off_x[0]*f).  sums: sum[0] += sum (tanh(y) - t)^2 (fp64, caller zeroes;
 *   all-reduced under data parallelism), tanh_out (nullable) receives tanh(y).  finalize: loss = sqrt(sum) * scale.
 *   bwd: dy = dloss[0] * scale * (tanh(y) - t) / sqrt(sum) * (1 - tanh(y)^2)  (dloss NULL: 1; sum == 0: dy = 0).
 * ------------------------------------------------------------------------------------------ */
/* bg_bn_glu_*: batch-norm apply on x[rows, 2C] (mean, rstd, gamma, beta: float[2C], the affine of bg_bn_apply_act_*)
 *   fused with the GLU that follows: y[rows, C].  Backward in the reduce / finalize / dx split of batch norm:
 *   bwd_reduce writes part = float[3][nseg][2C] (plane 0: sum g, plane 1: sum g xh over the rows of a segment, g = the
 *   gradient at the batch-norm output; plane 2 unused), which bg_bn_bwd_finalize(part, gamma, 0, count, dgamma, dbeta,
 *   NULL, cm, nseg, 2C) turns into dgamma, dbeta and cm = {m1, m2}; after the caller's all-reduce of cm,
 *   bwd_dx writes dx[rows, 2C].  nseg: any split of the rows, 1 <= nseg <= min(rows, 65535). */
int bg_bn_glu_fwd(const void* x, const float* mean, const float* rstd, const float* gamma, const float* beta, void* y,
                  int dtype, int64_t rows, int C, void* stream);
int bg_bn_glu_bwd_reduce(const void* x, const void* dy, const float* mean, const float* rstd, const float* gamma,
                         const float* beta, float* part, int dtype, int64_t rows, int C, int nseg, void* stream);
int bg_bn_glu_bwd_dx(const void* x, const void* dy, const float* mean, const float* rstd, const float* gamma,
                     const float* beta, const float* cm, void* dx, int dtype, int64_t rows, int C, void* stream);
int bg_glu_fwd(const void* x, void* y, int dtype, int64_t rows, int C, void* stream);
int bg_glu_bwd(const void* x, const void* dy, void* dx, int dtype, int64_t rows, int C, void* stream);
int bg_upsample2_fwd_t(const void* x, void* y, int dtype, int N, int H, int W, int C, void* stream);
int bg_upsample2_bwd_t(const void* dy, void* dx, int dtype, int N, int H, int W, int C, void* stream);
int bg_crop_at_fwd(const void* x, void* y, int dtype, const int32_t* off_y, const int32_t* off_x, int N, int H, int W,
                   int p, int C, void* stream);
int bg_crop_at_bwd(const void* dy, void* dx, int dtype, const int32_t* off_y, const int32_t* off_x, int N, int H, int W,
                   int p, int C, void* stream);
int bg_recon_loss_sums(const float* y, const float* target, float* tanh_out, const int32_t* off_y, const int32_t* off_x,
                       int mode, int f, double* sum, int N, int h, int w, int S, int C, void* stream);
int bg_recon_loss_finalize(const double* sum, double scale, float* loss, void* stream);
int bg_recon_loss_bwd(const float* y, const float* target, const int32_t* off_y, const int32_t* off_x, int mode, int f,
                      const double* sum, double scale, const float* dloss, float* dy, int N, int h, int w, int S, int C,
                      void* stream);

/* --------------------------------------------------------------------------------------------
 * Sample grids (utils.py:133-161 save_images; csrc/sample.hip).
 * bg_image_tiles_u8: x [n,H,W,C] (BG_F32 / BG_BF16, NHWC, nominally in [-1,1], C in {1,3,4}) -> bytes of the image grid
 *   grid [gh*H, gw*W, C] uint8, row-major.  Image i goes to tile t = tile0 + i at grid row t / gw, column t % gw; images
 *   whose tile is >= gh*gw are skipped; tiles without an image are left untouched (the caller zero-fills the grid once
 *   and may fill it one generator batch at a time).  byte = clamp(rint((double)((x + 1.0f) * 0.5f) * 255.0), 0, 255),
 *   bit-identical to the numpy host path; +-inf clamp, NaN writes 0.
 * ------------------------------------------------------------------------------------------ */
int bg_image_tiles_u8(const void* x, int x_dtype, int n, int H, int W, int C, uint8_t* grid, int gh, int gw, int tile0,
                      void* stream);

/* bg_image_place_u8: the same bytes, every image to a destination of its own inside one uint8 arena (the sampling service
 *   packs the images of a generator batch into the response strips of several request files).
 *   table  n entries of 16 bytes on the device (int32 [n,4], little-endian):
 *            word 0-1 offset (int64) of the image's first byte in arena   2 pitch (bytes per row)   3 skip (0 / 1)
 *   Row r of image i goes to arena + offset + r * pitch.  skip != 0 is a padding slot and writes nothing.
 *   The library cannot read the table: an entry with offset < 0, pitch < W*C or offset + (H-1)*pitch + W*C > arena_bytes
 *   writes nothing at all.  Overlapping destinations are the caller's error.
 *   When W*C, offset and pitch are multiples of 4 (and x and arena are aligned for it) a thread converts 4 consecutive
 *   elements and stores one 32-bit word; otherwise the stores are single bytes. */
typedef struct BgPlaceEntry {
    int64_t offset;
    int32_t pitch, skip;
} BgPlaceEntry;
int bg_image_place_u8(const void* x, int x_dtype, int n, int H, int W, int C, const BgPlaceEntry* table, uint8_t* arena,
                      int64_t arena_bytes, void* stream);

/* --------------------------------------------------------------------------------------------
 * Device-side PNG encoding (csrc/png.hip; an addition to ABI 10: new symbols only, nothing existing changes).  The bytes of
 * bg_image_tiles_u8 / bg_image_place_u8 are filtered and DEFLATE-compressed where they lie; the host adds the zlib and PNG
 * framing (png.py).  All three launchers are stream-ordered, allocate nothing, and cannot read their device tables: a
 * kernel checks every entry against the arena sizes it was given and writes nothing for one that does not fit.
 *
 * bg_png_filter: images inside the uint8 arena src -> their filtered streams inside dst.  Image i is h rows of row_bytes
 *   bytes at src + src_offset; its stream is h rows of 1 + row_bytes bytes at dst + dst_offset: the filter type, then the
 *   filtered bytes.  The type of a row is the type 0-4 with the smallest sum of abs((int8)residual), ties to the lowest
 *   type; the row above the first is zeros; bpp (1, 3 or 4) is common to the launch.  max_h >= every h (an entry with
 *   h > max_h writes nothing).  One workgroup per row.
 * bg_deflate_segments: segment j, len bytes (1 <= len <= seg_bytes) at src + src_offset, is compressed on its own - no match
 *   reaches outside it - into its slot of bg_deflate_bound(len) bytes at dst + dst_offset, byte-aligned: one dynamic-Huffman
 *   block (literals and distance-1 matches of 3..258 bytes, code lengths <= 15, code-length code <= 7) or, when that is not
 *   smaller, one stored block; with last == 0 an empty stored block follows (000, zero padding, 00 00 FF FF), with last != 0
 *   the block carries BFINAL and is zero-padded to a byte.  The slots of one stream, end to end, are a raw DEFLATE stream.
 *   records[4*j .. 4*j+3] = nbytes, adler_a, adler_b (the Adler-32 halves of the segment on its own), kind (1 dynamic,
 *   0 stored, -1 the entry did not fit: nbytes 0, nothing written).  seg_bytes: a power of two from 256 to 32768.
 *   Same input, same bytes: on every call, whatever else shares the launch.
 * bg_deflate_bound: what a slot must hold (a true upper bound of nbytes); host function.
 * bg_deflate_compact: seg_off[j] = sum of nbytes before segment j (seg_off[n_segs] = the total), the slots gathered into
 *   out at those offsets, and totals[2*k], totals[2*k+1] = (offset in out, bytes) of stream k, a stream ending at every
 *   segment with last != 0.  seg_off: int64 [n_segs + 1]; totals: int64 [2 * n_streams].
 * ------------------------------------------------------------------------------------------ */
typedef struct BgPngImage {
    int64_t src_offset;
    int32_t h, row_bytes;
    int64_t dst_offset;
} BgPngImage;
typedef struct BgDeflateSeg {
    int64_t src_offset;
    int32_t len, last;
    int64_t dst_offset;
} BgDeflateSeg;
size_t bg_deflate_bound(int len);
int bg_png_filter(const uint8_t* src, int64_t src_bytes, const BgPngImage* table, int n, int max_h, int bpp, uint8_t* dst,
                  int64_t dst_bytes, void* stream);
int bg_deflate_segments(const uint8_t* src, int64_t src_bytes, const BgDeflateSeg* table, int n_segs, int seg_bytes,
                        uint8_t* dst, int64_t dst_bytes, int32_t* records, void* stream);
int bg_deflate_compact(const uint8_t* slots, int64_t slots_bytes, const BgDeflateSeg* table, const int32_t* records,
                       int n_segs, uint8_t* out, int64_t out_bytes, int64_t* seg_off, int64_t* totals, int n_streams,
                       void* stream);

/* --------------------------------------------------------------------------------------------
 * Input batches (utils.py:12-38 image_processing, BigGAN.py:768-787; csrc/input.hip).
 * bg_image_batch_u8: the decoded pixels of n images -> the training batch out [n,S,S,C] fp32 in [-1,1], C in {1,3,4}.
 *   raw    one packed uint8 buffer of raw_bytes bytes; image i is [h,w,C] row-major at table[i].offset, a multiple of 16
 *   table  n entries of 32 bytes on the device (data.pack_batch builds them as int32 [n,8], little-endian):
 *            word 0-1 offset (int64)   2 h   3 w   4 flip (0 / 1)   5 scale_y   6 scale_x (fp32 bits)   7 reserved (0)
 *          with scale = (float)((double)n_in / (double)S), computed on the host
 *   Per element, each step one correctly rounded fp32 operation (bit-identical to the numpy host path, no fma):
 *     src = i * scale, lo = floor(src), hi = min(lo + 1, n_in - 1), f = src - lo;
 *     top = a * (1 - fx) + b * fx, bot likewise; v = top * (1 - fy) + bot * fy; out = v / 127.5f - 1.0f.
 *   flip mirrors the output columns: out[:, x] = resized[:, S - 1 - x].
 *   The library cannot read the table: an entry with h or w < 1, an offset that is negative or no multiple of 16, or an
 *   extent offset + h*w*C > raw_bytes reads nothing and fills its image with NaN.
 * ------------------------------------------------------------------------------------------ */
typedef struct BgImageEntry {
    int64_t offset;
    int32_t h, w;
    int32_t flip;
    float   scale_y, scale_x;
    int32_t reserved;
} BgImageEntry;
int bg_image_batch_u8(const uint8_t* raw, int64_t raw_bytes, const BgImageEntry* table, int n, int S, int C, float* out,
                      void* stream);

/* --------------------------------------------------------------------------------------------
 * JPEG images of an input batch (tf.image.decode_jpeg with its defaults behind utils.py:27; csrc/jpeg.hip).
 * bg_jpeg_batch_u8: entropy-decoded coefficients (bg_jpeg_coefficients) -> the uint8 pixels [h,w,channels] of the JPEG
 *   images' slots in raw, the buffer that bg_image_batch_u8 reads next.  Slots of other images are not touched.
 *   coef    int16 [coef_count], 16-byte aligned; 64 values a block, de-zigzagged, not dequantised
 *   jpegs   n_jpeg entries of 480 bytes on the device, 16-byte aligned, in ascending block0 (data.pack_batch builds them
 *           as int32 [n_jpeg,120]):
 *             slot      byte offset of the image in raw (a multiple of 16)
 *             w, h      image size; channels 1 or 3 = what the slot holds; ncomp 1 or 3; hs x vs the luma sampling
 *             block0    number of the image's first block among the batch's blocks (sum of its predecessors' blocks);
 *                       the image's component planes live at 64 * block0 of the workspace's plane area
 *             image     index of the image's BgImageEntry in table, whose offset, h and w must be slot, h and w
 *             comp[c]   coef = first int16 of the component in coef (a multiple of 8), bw x bh = its block grid, which
 *                       must be the one of w, h, hs, vs: whole MCUs of hs x vs luma blocks and one block per chroma
 *             q[c]      the component's quantisation table in natural order
 *   total_blocks  blocks of all entries; max_pixels  the largest w * h (sizes the grid only)
 *   table   the n BgImageEntry of the batch: see below
 *   ws      bg_jpeg_batch_workspace_bytes(n_jpeg, total_blocks) bytes, 16-byte aligned
 *   Integer arithmetic, bit-identical to data.decode_jpeg: coefficient * q; libjpeg's slow-integer inverse DCT (13-bit
 *   constants; columns, (v + 2^10) >> 11; rows, (v + 2^17) >> 18; + 128; clamp); the planes cropped to
 *   ceil(w / hs) x ceil(h / vs); "fancy" upsampling, 2x1: (3 p[i] + p[i-1] + 1) >> 2, (3 p[i] + p[i+1] + 2) >> 2, 2x2:
 *   r = 3 p[j] + p[j-1 | j+1], then (3 r[i] + r[i-1] + 8) >> 4, (3 r[i] + r[i+1] + 7) >> 4, an edge sample being its own
 *   neighbour; R = Y + ((91881 Cr + 32768) >> 16), B = Y + ((116130 Cb + 32768) >> 16),
 *   G = Y + ((-22554 Cb + 32768 - 46802 Cr) >> 16) with Cb, Cr less 128; clamp.  channels = 1 stores Y, one component at
 *   channels = 3 stores Y three times.
 *   The library cannot read the tables: an entry whose sampling, block grid, coefficient extent, block range (inside
 *   total_blocks and not below the end of an earlier entry's) or slot extent is not as described reads and writes
 *   nothing for that image, and table[image] gets h = 0, so that bg_image_batch_u8 fills that image with NaN.
 * ------------------------------------------------------------------------------------------ */
typedef struct BgJpegComp {
    int64_t coef;
    int32_t bw, bh;
} BgJpegComp;
typedef struct BgJpegEntry {
    int64_t    slot;
    int32_t    w, h, channels, ncomp, hs, vs;
    int32_t    block0, image, reserved[2];
    BgJpegComp comp[3];
    uint16_t   q[3][64];
} BgJpegEntry;
size_t bg_jpeg_batch_workspace_bytes(int n_jpeg, int64_t total_blocks);
int    bg_jpeg_batch_u8(const int16_t* coef, int64_t coef_count, const BgJpegEntry* jpegs, int n_jpeg, int64_t total_blocks,
                        int max_pixels, uint8_t* raw, int64_t raw_bytes, BgImageEntry* table, int n, void* ws,
                        size_t ws_bytes, void* stream);

/* --------------------------------------------------------------------------------------------
 * Device-resident dataset (data.DatasetCache; csrc/dataset.hip): every file is decoded once and kept in one arena on the
 * GPU; every later batch is one gather launch from an index list.  The cached form of an image is one of two kinds:
 *   kind 0  the decoded uint8 pixels [h,w,C], exactly the bytes of its slot in bg_image_batch_u8's raw buffer;
 *   kind 1  the finished fp32 image [S,S,C]: resized and normalised, NOT flipped.
 * bg_dataset_store: a guarded batched copy of n_segs segments from src (src_bytes bytes, staged on the device) into the
 *   arena.  segs: n_segs entries of 32 bytes on the device (int64 [n_segs,4]: src, dst, bytes, reserved).  A segment whose
 *   src, dst and bytes are all multiples of 16 moves in 16-byte words (where src and arena are so aligned), any other in
 *   4-byte words.  A segment with a negative src, dst or bytes, one that is no multiple of 4, or an extent outside
 *   src_bytes / arena_bytes is skipped whole: nothing of it is copied.  Segments must not overlap in the arena.
 * bg_dataset_batch: out [n,S,S,C] fp32, C in {1,3,4}, from sel int32 [n,2] (entry index, flip) and entries, n_entries
 *   entries of 32 bytes on the device (int32 [n_entries,8], little-endian):
 *     word 0-1 offset (int64)   2 h   3 w   4 kind   5 scale_y   6 scale_x (fp32 bits, kind 0)   7 reserved (0)
 *   kind 0: the arithmetic of bg_image_batch_u8 step for step, scale = (float)((double)n_in / (double)S), the flip
 *   mirroring the output columns.  kind 1: out[y][x][:] = cached[y][flip ? S-1-x : x][:] (pixels mirrored, channels in
 *   order).  Both are bit-identical to data.ImageData.image_processing.
 *   The library cannot read the tables: a sel index outside [0, n_entries), a kind other than 0 or 1, h or w < 1, kind 1
 *   with h or w != S, an offset that is negative or no multiple of 16, or an extent past arena_bytes reads nothing and
 *   fills that image with NaN; other images are unaffected.
 * ------------------------------------------------------------------------------------------ */
typedef struct BgDatasetEntry {
    int64_t offset;               /* in the arena, multiple of 16 */
    int32_t h, w;                 /* kind 1: both must equal S */
    int32_t kind;                 /* 0 u8 source, 1 finished fp32 */
    float   scale_y, scale_x;     /* kind 0: (float)((double)n_in / S) */
    int32_t reserved;
} BgDatasetEntry;
typedef struct BgCopySeg {
    int64_t src, dst, bytes, reserved;   /* multiples of 4 */
} BgCopySeg;
int bg_dataset_store(const void* src, int64_t src_bytes, const BgCopySeg* segs, int n_segs, uint8_t* arena,
                     int64_t arena_bytes, void* stream);
int bg_dataset_batch(const uint8_t* arena, int64_t arena_bytes, const BgDatasetEntry* entries, int n_entries,
                     const int32_t* sel, int n, int S, int C, float* out, void* stream);

/* --------------------------------------------------------------------------------------------
 * Variable histograms (utils.py:322-333 tf.summary.histogram of every global variable; csrc/varhist.hip).
 * One call histograms every variable of the model by the rule of TF 1.x's histogram.cc:
 *   counts[i][b] = number of finite elements x of item i with upper_bound(limits, (double)x) == b, i.e. b is the first
 *                  index whose limit is strictly greater than x, compared in double against the uploaded table;
 *   stats[i]     = min, max, num, sum, sum_squares over the finite elements (sums in double) and, in stats[i][5], the
 *                  number of non-finite elements (NaN, +-Inf), which enter neither the buckets nor the statistics;
 *                  without a finite element min = DBL_MAX and max = -DBL_MAX (Histogram::Clear()).
 *   counts, min, max and num are exact; everything is bit-identical from run to run (bucket counts are merged with
 *   integer atomics, the sums through per-chunk partial rows in the workspace, added in a fixed order).
 * The item table does not change after VariableStore.pack(), so it is compiled once, on the host, into a plan that the
 * caller uploads and keeps (no allocation and no host-to-device copy inside bg_var_hist):
 *   bg_var_hist_plan_chunks  number of chunks of the plan (no chunk crosses an item boundary); BG_ERR_ARG for
 *                            n_items < 1, an item with n < 0 or n >= 2^32, a NULL or not 4-byte aligned pointer
 *   bg_var_hist_plan_bytes   size of the plan
 *   bg_var_hist_plan         writes the plan into a HOST buffer (8-byte aligned); items are device views at any 4-byte
 *                            offset, adjacent arena segments included
 *   bg_var_hist              plan: the DEVICE copy; limits: n_limits doubles on the device, ascending, odd count with
 *                            0.0 in the middle (TF's table has 1551), n_limits <= 2048; counts [n_items][n_limits] uint32
 *                            (zeroed by the call); stats [n_items][6] double; ws of bg_var_hist_workspace_bytes
 * ------------------------------------------------------------------------------------------ */
typedef struct BgHistItem {
    const float* x;
    int64_t      n;
} BgHistItem;
int    bg_var_hist_plan_chunks(const BgHistItem* items, int n_items, int* n_chunks);
size_t bg_var_hist_plan_bytes(int n_items, int n_chunks);
int    bg_var_hist_plan(const BgHistItem* items, int n_items, void* plan, size_t plan_bytes);
size_t bg_var_hist_workspace_bytes(int n_items, int n_chunks);
int    bg_var_hist(const void* plan, int n_items, int n_chunks, const double* limits, int n_limits, uint32_t* counts,
                   double* stats, void* ws, size_t ws_bytes, void* stream);

/* --------------------------------------------------------------------------------------------
 * Sliced Wasserstein distance on Laplacian-pyramid patches (Karras et al. 2018, section 5; csrc/swd.hip, metrics.py; an
 * addition to ABI 10: new symbols only).  NHWC images with H = W a power of two, C in {1, 3, 4}.  Every launcher is
 * stream-ordered and allocates nothing; every sum goes through partial rows added in index order (no float atomics), so
 * a repeated launch is bit-identical.  BG_ERR_ARG with a message for a NULL pointer, a bad dtype or a bad size.
 *
 * bg_swd_pyr_down: x [B,H,H,C] (BG_F32 / BG_BF16) -> y fp32 [B,H/2,H/2,C] = conv(x, f (x) f / 256)[::2, ::2] with
 *   f = [1 4 6 4 1] and the mirror boundary that does not repeat the edge (d c b | a b c d | c b a); H >= 32.
 * bg_swd_pyr_lap: y fp32 [B,H,H,C] = g - up(g1), g [B,H,H,C] (BG_F32 / BG_BF16), g1 fp32 [B,H/2,H/2,C]; up puts g1 on the
 *   even points of a zero [2h,2h] image and convolves it with 4 x the filter, mirror boundary on the 2h grid.  Both
 *   kernels add their 25 taps in row-major tap order, each term one fp32 fma.
 * bg_swd_descriptors: 128 patches of 7 x 7 per image of x fp32 [B,H,H,C], centres pos int32 [B,128,2] = (y, x) on the
 *   device -> rows row_offset + b * 128 + k of desc fp32 [n_rows, 49 C], a row holding the patch in [c, dy, dx] order, and
 *   partials[row_offset / 128 + b][c] = (sum, sum of squares) of the image's values of channel c in fp64.  partials:
 *   bg_swd_stats_workspace_bytes(n_rows / 128, C) bytes.  n_rows and row_offset are multiples of 128.  The library cannot
 *   read the table: a centre outside [3, H-4] writes a zero row.
 * bg_swd_stats_finish: stats[c] = (mean, 1 / biased standard deviation) in fp64 over the n_images * 128 * 49 values of
 *   channel c; a channel without deviation gets 0 for the reciprocal, which makes its normalised descriptors zero.
 * bg_swd_project: out[set * S + s][n] = sum over k ascending of fp32(((double)desc[n][k] - mean) * rstd) * dirs[k][s] in
 *   fp32 fma; dirs fp32 [49 C, S]; out fp32 [sets * S][N], one contiguous segment per direction.  desc_b / stats_b NULL:
 *   one set; otherwise set 1 follows set 0 in out.  N is a multiple of 64; out is 16-byte aligned.
 * bg_swd_sort_segments: sorts n_seg adjacent segments of seg_len floats (a power of two from 2 to 2^24) ascending, in
 *   place, by a bitonic network: the exchange distances below bg_swd_sort_tile() floats run inside LDS, one launch per
 *   merge size past the tile, the longer distances as passes over global memory, up to three distances a pass.  +-inf sort
 *   correctly; NaN is not handled.  Segments of a tile or more need 16-byte aligned data.
 * bg_swd_l1: out[i] = sum over j < n_per_out of |a[i * n_per_out + j] - b[i * n_per_out + j]|, differences and sums in
 *   fp64; ws of bg_swd_l1_workspace_bytes(n_per_out, n_out) bytes, 8-byte aligned.
 * ------------------------------------------------------------------------------------------ */
int    bg_swd_pyr_down(const void* x, int x_dtype, float* y, int B, int H, int C, void* stream);
int    bg_swd_pyr_lap(const void* g, int g_dtype, const float* g1, float* y, int B, int H, int C, void* stream);
size_t bg_swd_stats_workspace_bytes(int n_images, int C);
int    bg_swd_descriptors(const float* x, const int32_t* pos, int B, int H, int C, float* desc, int64_t n_rows,
                          int64_t row_offset, double* partials, size_t partials_bytes, void* stream);
int    bg_swd_stats_finish(const double* partials, size_t partials_bytes, int n_images, int C, double* stats, void* stream);
int    bg_swd_project(const float* desc_a, const double* stats_a, const float* desc_b, const double* stats_b,
                      const float* dirs, float* out, int64_t N, int C, int S, void* stream);
size_t bg_swd_sort_tile(void);
int    bg_swd_sort_segments(float* data, int n_seg, int seg_len, void* stream);
size_t bg_swd_l1_workspace_bytes(int64_t n_per_out, int n_out);
int    bg_swd_l1(const float* a, const float* b, int64_t n_per_out, int n_out, double* out, void* ws, size_t ws_bytes,
                 void* stream);

/* --------------------------------------------------------------------------------------------
 * Nearest training images of generated samples, in pixel space (csrc/nearest.hip, neighbours.py; an addition to ABI 10:
 * new symbols only).  Every launcher is stream-ordered and allocates nothing; no float atomics anywhere, so a repeated
 * launch is bit-identical.  BG_ERR_ARG with a message for a NULL pointer, a bad dtype or a bad size.
 *
 * bg_nn_pack: x [B,S,S,C] (BG_F32 / BG_BF16), C in {1, 3, 4} -> out bf16 [B, (S/f)(S/f)C], the search descriptors: the
 *   f x f box sum in fp32 (row-major order), times 1 / f^2, rounded to nearest even.  f is a power of two (1: a plain
 *   convert), S / f >= 8.  mirror != 0: the descriptor of the horizontally flipped image (columns reversed, channel order
 *   kept), bit-identical to packing the flipped batch.
 * bg_nn_distances: q bf16 [Q,D], set bf16 [N,D], both 16-byte aligned, D a multiple of 64 -> out fp32 [Q,N],
 *   out[i][n] = sum_j (q[i][j] - set[n][j])^2.  Every term is an fp32 difference squared into an fp32 sum (one fma); the
 *   expansion |q|^2 + |s|^2 - 2 q.s is not used, so a set row equal to a query gives 0.0f exactly.  One wave makes each sum
 *   in a fixed order.  Relative error at most (D + 2) u / (1 - (D + 2) u), u = 2^-24.
 * bg_nn_topk: for each of the Q rows of dist fp32 [Q,N] (finite values) the k <= 16 smallest entries as (value, index),
 *   ascending, ties to the lower index, into out_dist fp32 [Q,k] and out_idx int32 [Q,k]; places past N hold (+inf, -1).
 *   Exact.  ws: bg_nn_topk_workspace_bytes(Q, N, k) bytes, 4-byte aligned (0 bytes, and then ws may be NULL, for rows that
 *   one block scans).
 * ------------------------------------------------------------------------------------------ */
int    bg_nn_pack(const void* x, int x_dtype, int B, int S, int C, int f, int mirror, void* out, void* stream);
int    bg_nn_distances(const void* q, const void* set, int Q, int64_t N, int D, float* out, void* stream);
size_t bg_nn_topk_workspace_bytes(int Q, int64_t N, int k);
int    bg_nn_topk(const float* dist, int Q, int64_t N, int k, float* out_dist, int32_t* out_idx, void* ws, size_t ws_bytes,
                  void* stream);

/* --------------------------------------------------------------------------------------------
 * Multi-scale structural similarity of image pairs (Wang, Simoncelli and Bovik 2003; csrc/msssim.hip, metrics.py; an
 * addition to ABI 10: new symbols only).  NHWC images in [-1, 1] with H = W a power of two >= 16, C in {1, 3, 4}; the
 * arithmetic runs on u = (x + 1) / 2 with C1 = 0.01^2, C2 = 0.03^2, an 11-tap Gaussian window (sigma 1.5, no padding) and
 * L = min(5, log2(H) - 3) levels, level i of side H >> i, weighted by the first L of (0.0448, 0.2856, 0.3001, 0.2363,
 * 0.1333) over their sum.  Every launcher is stream-ordered and allocates nothing; every sum goes through partial rows
 * added in index order (no float atomics), so a repeated launch is bit-identical.  BG_ERR_ARG with a message for a NULL
 * pointer, a bad dtype or a bad size.
 *
 * bg_msssim_workspace_bytes: bytes of the fp64 partial sums of all L levels of P pairs of side H (0 for sizes that the
 *   launches reject); level and finish of one batch of pairs share one such workspace, 8-byte aligned.  It holds, level
 *   after level, fp64 [P][tiles][C][2] = (sum of cs, sum of ssim), tiles = ((H >> level) / 16)^2 in row-major tile order.
 * bg_msssim_level: level `level` (0 .. L-1) of P pairs.  a, b: the level's images [*, h, h, C], h = H >> level, BG_F32 or
 *   BG_BF16 at level 0 and BG_F32 below; pair p is image p * pair_stride of a and of b (pair_stride 1: two buffers of P
 *   images; pair_stride 2 with b = a + one image: rows 2p and 2p + 1 of one batch).  Each image is read once.  Written:
 *   the level's rows of ws, per (pair, 16 x 16 tile of window positions, channel) the sums of cs and of ssim = l * cs over
 *   the tile's positions, each position evaluated in fp32 (separable window, horizontal pass first) and added in fp64;
 *   and, unless the level is the last, pool_a and pool_b fp32 [P, h/2, h/2, C], the 2 x 2 means of the images,
 *   ((p00 + p01) + (p10 + p11)) * 0.25 in fp32.  At the last level pool_a and pool_b are not written and may be NULL.
 * bg_msssim_finish: scores[row_offset + p] for p < P, fp64: per channel the product over levels of
 *   max(mean cs_i, 0)^w_i (the last level: mean ssim), means over the (h - 10)^2 positions, then the mean over channels.
 *   scores holds n_scores doubles; row_offset + P <= n_scores.
 * ------------------------------------------------------------------------------------------ */
size_t bg_msssim_workspace_bytes(int P, int H, int C);
int    bg_msssim_level(const void* a, const void* b, int dtype, int64_t pair_stride, int P, int H, int level, int C,
                       float* pool_a, float* pool_b, double* ws, size_t ws_bytes, void* stream);
int    bg_msssim_finish(const double* ws, size_t ws_bytes, int P, int H, int C, double* scores, int64_t n_scores,
                        int64_t row_offset, void* stream);

/* --------------------------------------------------------------------------------------------
 * Singular-value monitor: the top singular values of every weight of a network at once (csrc/spectrum.hip, spectrum.py;
 * an addition to ABI 10: new symbols only).  Block power iteration on W^T W with a basis of BG_SV_BLOCK vectors per weight,
 * then a Rayleigh-Ritz step.  An item is a weight w[rows][cols] (fp32, row-major; the reshape of BgSnItem) with
 *   q      [cols][BG_SV_BLOCK] fp32, the basis: orthonormal columns, in and out (it warm-starts the next call)
 *   sv     [BG_SV_BLOCK] out: the Ritz values sqrt(max(lambda_i, 0)), descending
 *   resid  [BG_SV_BLOCK] out: || W^T (W q_i) - lambda_i q_i ||_2 / lambda_0 (0 when lambda_0 = 0): some singular value
 *          squared of W lies within resid[i] * sv[0]^2 of sv[i]^2
 * b_eff = min(BG_SV_BLOCK, rows, cols): basis columns >= b_eff are set to zero and sv, resid are 0 there.  A direction
 * that is numerically dependent on the earlier ones (remaining squared norm <= 2^-80 of its squared norm) becomes a zero
 * column of q; no NaN or Inf is written.  The table lives in device memory; ws_offset is the byte offset (16-byte
 * aligned) of the item's scratch of bg_sv_workspace_bytes(rows, cols) bytes inside ws, and the call zeroes the part of ws
 * that it uses.  iters (0..256) iterations of [Y = W Q; Z = W^T Y; Q = orth(Z)], then the Ritz step: 3 * iters + 5
 * launches for any n_items (1..256); iters = 0 is the Ritz step on the basis as given.  BG_ERR_ARG with a message, before
 * any launch, for a NULL table, a NULL or misaligned ws, a count out of range or ws_bytes below n_items times the
 * smallest item's scratch; an item whose own scratch range does not lie inside ws_bytes is left alone by every kernel.
 * Not bit-reproducible: the second pass adds with fp64 atomics, whose arrival order differs between launches.
 * ------------------------------------------------------------------------------------------ */
#define BG_SV_BLOCK 8
typedef struct BgSvItem {
    const float* w;        /* [rows, cols] */
    float* q;              /* [cols, BG_SV_BLOCK], in/out */
    float* sv;             /* [BG_SV_BLOCK], out */
    float* resid;          /* [BG_SV_BLOCK], out */
    int64_t ws_offset;
    int32_t rows, cols;
} BgSvItem;
size_t bg_sv_workspace_bytes(int rows, int cols);
int    bg_sv_batch(const BgSvItem* items_dev, int n_items, int iters, void* ws, size_t ws_bytes, void* stream);

/* --------------------------------------------------------------------------------------------
 * Radial power spectrum of image sets (Durall et al. 2020; csrc/powerspec.hip, metrics.py; an addition to ABI 10: new
 * symbols only).  NHWC images in [-1, 1], contiguous, side S a power of two from 16 to 512, C in {1, 3, 4}: C = 1 is used as
 * it is, C = 3 and 4 go through Y = 0.299 R + 0.587 G + 0.114 B (alpha is ignored).  F = DFT2(Y), unnormalised, and
 * P = |F|^2 / S^4, so that the sum of P over the full plane is mean(Y^2); no window, no mean subtraction.  Only the columns
 * kx = 0 .. S/2 are kept; 0 < kx < S/2 stand for their mirror images as well.  The transforms are fp32 radix-4 / radix-2
 * passes in LDS with twiddles rounded once from fp64; two real rows share one complex transform.  Every launcher is
 * stream-ordered and allocates nothing; there are no atomics, so a repeated launch is bit-identical.  BG_ERR_ARG with a
 * message for a NULL pointer, a bad dtype, side, channel count or image count, a short workspace, a misaligned buffer.
 *
 * bg_ps_workspace_bytes: bytes of the workspace of n images of side S (0 for sizes that the launches reject): the
 *   twiddle table and the row transforms, fp32 complex [n, S, S/2 + 1]; 8-byte aligned.
 * bg_ps_power: power fp32 [n, S, S/2 + 1] = P; row ky in DFT order (0 .. S/2 - 1, then -S/2 .. -1), unshifted.  x is
 *   BG_F32 or BG_BF16 [n, S, S, C].
 * bg_ps_profile: profiles fp64 [n, NB], NB = (isqrt(2 S^2) + 1) / 2 + 1 (12 / 24 / 46 / 92 / 182 / 363 for S = 16 .. 512):
 *   the mean of P over the coefficients of the full plane whose radius rounds to r, r = (isqrt(4 (ky^2 + kx^2)) + 1) / 2
 *   with signed frequencies, in integers; bin 0 is DC, bin NB - 1 holds the corner (S/2, S/2).  With sum2d, fp64
 *   [S, S/2 + 1], P of image 0, then image 1, ... is added to what sum2d holds; sum2d may be NULL.
 * ------------------------------------------------------------------------------------------ */
size_t bg_ps_workspace_bytes(int n, int S);
int    bg_ps_power(const void* x, int dtype, int n, int S, int C, float* power, void* ws, size_t ws_bytes, void* stream);
int    bg_ps_profile(const float* power, int n, int S, double* profiles, double* sum2d, void* stream);

/* --------------------------------------------------------------------------------------------
 * Precision / recall (Kynkaanniemi et al. 2019) and density / coverage (Naeem et al. 2020) of a generated set against a
 * real set, on the bf16 search descriptors of bg_nn_pack (csrc/prdc.hip, metrics.py; an addition to ABI 10: new symbols
 * only).  All on squared distances d(a, b) = sum_j (a_j - b_j)^2 over bf16 rows [., D], D a multiple of 64, rows 16-byte
 * aligned: the arithmetic of bg_nn_distances (fp32 differences of exactly widened bf16, one fma per term, no
 * |a|^2 + |b|^2 - 2 a.b expansion, no MFMA), so equal rows give 0.0f exactly and the relative error is at most
 * (D + 2) u / (1 - (D + 2) u), u = 2^-24.  The order of summation depends on the element index alone: d(a, b) and d(b, a)
 * are the same bits, and the radii and the membership tests come from one function.  The [Q, N] matrix is never written: a
 * block owns 16 set rows, walks all queries and keeps per row what is asked for.  Every launcher is stream-ordered and
 * allocates nothing; there are no atomics, so a repeated launch is bit-identical.  BG_ERR_ARG with a message, before
 * anything is launched, for a NULL pointer, a bad size or a misaligned pointer.
 *
 * bg_prdc_radii: x bf16 [N, D], 1 <= k <= 8, N >= k + 1 -> radius fp32 [N]: radius[n] is the k-th smallest d(x_n, x_m) over
 *   m != n.  "Itself" is the row with the same index: a different row of equal content counts (and gives 0); ties count
 *   with multiplicity.
 * bg_prdc_cover: q bf16 [Q, D] with radius_q fp32 [Q], set bf16 [N, D] -> count int32 [N], count[n] = #{i < Q :
 *   d(q_i, set_n) <= radius_q[i]} (inclusive; radius_q may hold 0 and +inf), and dmin fp32 [N], dmin[n] = min_i
 *   d(q_i, set_n).  Either output may be NULL, not both; radius_q may be NULL when count is.
 * bg_prdc_reduce: count_f int32 [M], count_r int32 [N], dmin_r and radius_r fp32 [N] -> out4 int64 [4], 8-byte aligned:
 *   (#{count_f > 0}, sum count_f, #{count_r > 0}, #{dmin_r <= radius_r}).  With k and the sizes: precision = out4[0] / M,
 *   density = out4[1] / (k M), recall = out4[2] / N, coverage = out4[3] / N, for count_f = cover(q = real with its radii,
 *   set = fake), count_r = cover(q = fake with its radii, set = real) and dmin_r of the latter.
 * ------------------------------------------------------------------------------------------ */
int    bg_prdc_radii(const void* x, int64_t N, int D, int k, float* radius, void* stream);
int    bg_prdc_cover(const void* q, const float* radius_q, int64_t Q, const void* set, int64_t N, int D, int32_t* count,
                     float* dmin, void* stream);
int    bg_prdc_reduce(const int32_t* count_f, int64_t M, const int32_t* count_r, const float* dmin_r, const float* radius_r,
                      int64_t N, int64_t* out4, void* stream);

/* --------------------------------------------------------------------------------------------
 * Optional per-kernel timing for bench.py's roofline leg: when enabled, every MFMA GEMM launch
 * (conv / deconv / gemm families) is bracketed by hipEvents on its stream.
 * bg_prof_collect synchronises the events and returns totals since the last reset.
 * ------------------------------------------------------------------------------------------ */
void bg_prof_enable(int on);
void bg_prof_reset(void);
int  bg_prof_collect(double* total_ms, double* total_flops, int64_t* launches);
/* write one CSV line (tag,flops,ms) per recorded launch; does not clear the records */
int  bg_prof_dump(const char* path);

#ifdef __cplusplus
}
#endif
#endif /* BIGGAN_HIP_H */
