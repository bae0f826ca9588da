/*
 * p3hip — C-ABI of the MI355X-native (gfx950) Pix2Poly / FFL encoder-fusion-decoder path.
 *
 * The reference (raphaelsulzer/PixelsPointsPolygons) has NO FFI / plugin boundary for this path:
 * it is a Python nn.Module API whose arithmetic runs inside third-party binaries (ATen/cuDNN/
 * cuBLAS kernels behind timm + torch.nn, and Open3D's compiled `voxelize` / `ragged_to_dense`
 * ops).  This header is the boundary this project introduces one level below those nn.Modules:
 * each entry point names the reference call it replaces (paths relative to the reference root).
 *
 * Conventions
 *   - plain C types only; every pointer is a DEVICE pointer owned by the caller (PyTorch);
 *     the library allocates nothing persistent and keeps no pointer after return.
 *   - `stream` is a hipStream_t passed as void*; all calls are asynchronous on that stream,
 *     never synchronise, and are safe to capture into a hipGraph.
 *   - return 0 on success; negative P3_E* for argument errors (p3_last_error_string() has text);
 *     positive values are hipError_t codes from a failed launch.
 *   - dtype codes: P3_F32 = 0 (exact fp32 path, fp32 MFMA), P3_BF16 = 1 (bf16 storage, fp32 accumulate), P3_F32X3 = 2 (fp32 storage, products as
 *     bf16 x 3 on the bf16 MFMA: accepted wherever a descriptor's dtype names the operands of a PRODUCT - p3_gemm_desc.dtype_in, p3_gemm_tn's dtype,
 *     p3_attn_desc.dtype, p3_pillar_desc.dtype - and chosen per call, so two models of different precision share one process).
 *   - matrices are row-major with explicit element strides.
 */
#ifndef P3HIP_H
#define P3HIP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define P3_OK 0
#define P3_EINVAL (-1)
#define P3_ESHAPE (-2)
#define P3_EALIGN (-3)
#define P3_EUNSUP (-4)

#define P3_F32 0
#define P3_BF16 1
#define P3_F32X3 2 /* operands stored as fp32 exactly like P3_F32; every value is split into hi = bf16(x) and lo = bf16(x - hi) while it is staged and the product
                    * accumulates a_lo b_hi + a_hi b_lo + a_hi b_hi in fp32 on the bf16 MFMA (2^-17 relative per product instead of the exact fp32 MFMA's 2^-24;
                    * outputs, epilogues and every non-product kernel stay fp32).  The "fp32x3" precision of the Python host; tests hold it to the north star's 1e-3. */

#define P3_ACT_NONE 0
#define P3_ACT_GELU 1 /* exact erf GELU (timm Mlp act_layer=nn.GELU) */
#define P3_ACT_RELU 2
#define P3_ACT_MUL 3  /* p3_gemm_desc.bwd_act only: the saved tensor already holds act'(pre) (aux_mode = 1): plain multiply */
#define P3_ACT_BN_RELU 4 /* p3_gemm_desc.bwd_act only: bwd_saved = H, the input of a train-mode BatchNorm + ReLU whose OUTPUT this GEMM's product is the gradient
                          * of: C = [H*bn[0] + bn[1] > 0] * (A'W^T) * bn[0] + bn[2] + bn[3] * H  with bwd_bn = four rows of N floats (scale, shift, and the a / b
                          * of p3_bn_bwd_coeffs) - the whole BatchNorm backward of the layer in front, no [M,N] gradient stored in between */

#define P3_A_PLAIN 0
#define P3_A_CONV3X3 1 /* A is an NHWC map [B,H,W,lda]; K = 9*C, zero padding 1 (implicit GEMM) */
#define P3_A_AFFINE_RELU 2 /* A'[m,k] = relu(A[m,k]*a_scale[k] + a_shift[k])  (BN+ReLU folded into the load) */
#define P3_A_PAIR_AFFINE_RELU 3 /* A'[(b,i,j),k] = relu((U[b,i,k]+V[b,j,k])*a_scale[k]+a_shift[k]) ScoreNet conv1 */
#define P3_A_AFFINE_MASK2 5 /* p3_gemm_tn_ex only: B'[m, k] = [y > 0] for k < K and [y > 0] * B[m, k - K] for K <= k < 2K, y = B[m, k]*b_scale[k]+b_shift[k]:
                              * ONE pass over (A, B) gives G = A^T [y > 0] and G2 = A^T ([y > 0] B) - a BatchNorm/ReLU layer's weight gradient AND the sums
                              * of its input gradient's BatchNorm backward (p3_bn_sums_from_g); C is [N, 2K] */
#define P3_A_CONV3X3_AFFINE_RELU 4 /* CONV3X3 over relu(A*a_scale[c]+a_shift[c]) (a_scale/a_shift indexed by input channel): FFL heads */

int p3_version(void);
const char* p3_last_error_string(void);
/* Measurement hook: after p3_trace_kernels(1), p3_last_kernel() names the device kernel the calling thread's last p3_gemm launched, spelled as
 * rocprofv3 --kernel-trace prints it after tools/kstats.py's bf16 rewrite ("gemm_dma_kernel<bf16, 32, 2>"); "" when tracing is off.  The other entries
 * that choose between kernels record theirs too: p3_gemm_x3, p3_gemm_tn_ex ("gemm_tn_kernel<bf16, 0>" or its dedicated kernels), p3_gemm_tn_x3,
 * p3_attention ("attn_fwd_kernel<bf16_t, 64, false>" / "attn_decode_kernel<64>") and the LayerNorm entries ("ln_fwd_kernel",
 * "ln_fwd_half_planes_kernel", "ln_bwd_half_kernel", "ln_bwd_kernel").  p3_trace_kernels() itself forgets the last name. */
void p3_trace_kernels(int on);
const char* p3_last_kernel(void);

/* Deterministic reductions.  The reference seeds everything and sets cudnn.deterministic (misc/shared_utils.py:120-126, trainer.py:214);
 * here the kernels that would finish in fp32 atomicAdd's over workgroup partials (BatchNorm sums of the ScoreNet, split-M weight
 * gradients, bias-gradient column sums) store the partials into `scratch` instead and add them in workgroup order in float64: the same
 * bits every run.  scratch: device memory owned by the caller (16-byte aligned, >= 8 MB for the shapes of this path; a launch whose
 * partials do not fit falls back to atomics), used launch by launch in stream order on ONE stream; NULL / 0 switches the mode off.
 * all_dtypes = 0: only fp32 (parity-mode) launches take the path; 1: bf16 launches too.  p3_get_deterministic: 0 off, 1 fp32, 2 all. */
int p3_set_deterministic(void* scratch, int64_t bytes, int all_dtypes);
int p3_get_deterministic(void);
/* More than one launch stream (r04: the independent branches of model_pix2poly.py:256-264 - scorenet1 || scorenet2 - the weight-gradient
 * GEMMs and the pillar stem beside the patch embedding, early_fusion_vit.py:99-100, may be enqueued on side streams): the scratch is cut
 * into `n` equal regions (p3_scratch_regions, before or after p3_set_deterministic).  Region 0 serves every stream that is not registered
 * (default stream, hipGraph capture streams); p3_scratch_side_stream registers a side stream (returns its region 1 .. 15) and
 * p3_scratch_stream names the stream of the launches that follow (returns the region, -1 = a side stream beyond the region count: those
 * launches take their atomics path).  Single-threaded like the rest of the library. */
int p3_scratch_regions(int n);
int p3_scratch_side_stream(void* stream);
/* Deferred parameter-gradient reduces (r04).  p3_reduce_defer(arena, floats): from now on a launch whose workgroup partials only feed parameter gradients (the
 * LayerNorm backward's dgamma / dbeta: 42 launches per Pix2Poly train step) parks them in `arena` while p3_reduce_defer_enable(1) is in force (device memory, caller-owned; NULL switches the mode off) instead
 * of launching its own reduce; p3_reduce_flush(stream) adds every parked set to its outputs in ONE launch, in the same fixed float64 order (bit-identical
 * gradients) - call it after the backward pass, before anything reads the gradients.  p3_reduce_pending(): sets parked since the last flush.  A full arena or
 * table (48 sets) falls back to the immediate reduce. */
int p3_reduce_defer(float* arena, int64_t floats);
int p3_reduce_defer_enable(int on);    /* parking happens only between enable(1) and enable(0): the host brackets exactly the launches whose outputs are
                                         * accumulation targets that stay valid until the flush (gradient arena views), returns the previous setting */
int p3_reduce_flush(void* stream);
int p3_reduce_pending(void);
int p3_reduce_drop(void);              /* forget the parked sets without adding them (after a backward pass that raised); returns how many */
int p3_scratch_stream(void* stream);
/* Deferred weight-gradient reduces (r05), the same idea for the split-M weight-gradient GEMMs (p3_gemm_tn / p3_gemm_tn_ex / p3_gemm_tn_x3) in the deterministic mode:
 * between p3_tn_defer_enable(1) and (0) a launch that would store its partial tiles in the caller's `slabs` and add them to C with a reduce launch of its own
 * (109 launches of ~16 us per fp32x3 train step) parks them in `arena` instead (p3_tn_defer: device memory, caller-owned; a full arena / table falls back to the
 * immediate reduce); p3_tn_flush(stream) adds every parked set to its C - float64, split order: bit-identical gradients - in ceil(sets / 96) launches.  Only for
 * C that stays valid and unread until the flush (views of the optimizer's gradient arena); call the flush after the backward pass. */
int p3_tn_defer(float* arena, int64_t floats);
int p3_tn_defer_enable(int on);
int p3_tn_flush(void* stream);
int p3_tn_pending(void);
int p3_tn_drop(void);

/* ------------------------------------------------------------------------------------------
 * GEMM with fused epilogue:  C[M,N] = act(A'[M,K] * W[N,K]^T + bias) + residual
 * Replaces every nn.Linear / 1x1 / kxk(stride k) conv on the path:
 *   timm PatchEmbed.proj            models/fusion_layers/early_fusion_vit.py:69-70,99  (im2col'd by p3_patchify)
 *   timm Attention.qkv/.proj, Mlp   models/vision_transformer/vit.py:48 (timm Block x12)
 *   fusion Conv3x3                  models/fusion_layers/early_fusion_vit.py:75-79     (P3_A_CONV3X3)
 *   nn.MultiheadAttention in/out proj, linear1/2, output   models/pix2poly/model_pix2poly.py:138-139,185
 *   ScoreNet conv1..3               models/pix2poly/model_pix2poly.py:74-80            (P3_A_PAIR_AFFINE_RELU / P3_A_AFFINE_RELU)
 * K must be a multiple of 64 (bf16) / 16 (f32); M, N arbitrary.
 * ------------------------------------------------------------------------------------------ */
/* Counter-based dropout (nn.Dropout / the attention-probability dropout of nn.MultiheadAttention in training mode, reference
 * Decoder: model_pix2poly.py:136,139,143): element (row, col) of site `site` is kept iff 16 bits of hash(seed, site, row, col) are
 * >= round(p * 65536), and scaled by 1/(1-p); the mask is never stored, backward kernels regenerate it.  `seed` points to a DEVICE counter (advance it once per
 * training step with p3_rng_advance, inside the captured graph).  seed == NULL disables dropout. */
typedef struct {
    const unsigned long long* seed;
    unsigned int site;
    float p;
} p3_dropout;
int p3_rng_advance(unsigned long long* seed, void* stream);
/* Batched 2-D bf16 transposes inside one arena (the W^T copies the dX GEMMs read, refreshed after the optimizer step in one launch).
 * table: device array of n_entries records {int64 src_off, int64 dst_off, int32 rows, int32 cols, int32 first_tile, int32 tiles_c}
 * (element offsets; 32x32 tiles, tiles_c = ceil(cols / 32), first_tile = running sum of tile counts); grid = total_tiles blocks. */
int p3_transpose_many(const void* src, void* dst, const void* table, int n_entries, int total_tiles, void* stream);
/* out[i] = keep(i / ncols, i % ncols) ? in[i] / (1-p) : 0   (elementwise dropout forward, and its backward applied to the gradient) */
int p3_dropout_apply(const void* in, int dtype_in, void* out, int dtype_out, int64_t n, int64_t ncols, const p3_dropout* drop, void* stream);

typedef struct {
    int M, N, K;
    int lda, ldb, ldc;
    int dtype_in;  /* dtype of A and W */
    int dtype_out; /* dtype of C and aux */
    int act;
    int a_mode;
    const float* bias;    /* [N] or NULL */
    const void* residual; /* [M,N] (ldr) or NULL; added after the activation */
    int ldr;
    int dtype_res;        /* dtype of residual (may differ from dtype_out: bf16 stream + fp32 pre-LayerNorm sum) */
    void* aux;            /* optional [M,N] (ldc): pre-activation values (for backward) */
    int conv_H, conv_W, conv_C; /* P3_A_CONV3X3 */
    const float* a_scale; /* [K] for the AFFINE modes */
    const float* a_shift; /* [K] */
    const void* pair_V;   /* P3_A_PAIR_AFFINE_RELU: V [B*n, K] (A is U [B*n, K]); M = B*n*n */
    int pair_n;
    float* colsum;        /* optional [N]: += sum over rows of (A'W^T + bias)   (train-mode BatchNorm statistics) */
    float* colsumsq;      /* optional [N]: += sum of squares */
    p3_dropout drop;      /* dropout of act(A'W^T + bias) before the residual add; element = (row, col) */
    /* backward of an upstream activation fused into this (dX) GEMM's epilogue: C = (A'W^T) * act'(bwd_saved) * bwd_scale, with
     * bwd_saved [M,N] (ldc, dtype_out) = the pre-activation (P3_ACT_GELU) or the activation output (P3_ACT_RELU) saved by forward */
    const void* bwd_saved;
    int bwd_act;
    float bwd_scale;
    int aux_mode;         /* what `aux` receives: 0 = the pre-activation, 1 = act'(pre) (GELU: cdf + x*pdf, computed with the
                           * activation from the same erf / exp), so that backward is a multiply with no transcendental */
    int conv_pad;         /* P3_A_CONV3X3: 1 = A is a zero-bordered image [B, conv_H+2, conv_W+2, lda] (p3_pad_nhwc): taps are read
                           * without bounds checks; conv_H / conv_W stay the OUTPUT size */
    const float* bwd_bn;  /* bwd_act = P3_ACT_BN_RELU: [4, N] floats (scale | shift | a | b) */
    const void* w_lo;     /* dtype_in = P3_F32X3 with a plain / 3x3-gathered A only: non-NULL = the weight comes as PLANES - W addresses hi = bf16(w) [N, K], w_lo the
                           * matching lo = bf16(w - hi), both with row stride ldb (bf16 elements, % 8 == 0, 16-byte aligned) - what the optimizer keeps fresh for every
                           * 2-D master (training.FlatAdamW).  The kernel then stages W with plain 16-byte copies instead of splitting it in every tile (r06: MFMA and VALU
                           * work do not overlap on a SIMD - tools/probe/coissue_probe.hip - so the split of an operand that never changes was pure added time);
                           * the bits of the result are those of the fp32 weight's split */
} p3_gemm_desc;
int p3_gemm(const void* A, const void* W, void* C, const p3_gemm_desc* d, void* stream);
/* The LDS-DMA kernels behind p3_gemm for the plain bf16 products (csrc/gemm_dma.hip), callable directly for A/B measurements and parity tests: same
 * descriptor, P3_EUNSUP when the problem is not eligible (plain bf16 A, K % 64 == 0, N % 8 == 0, 16-byte aligned rows, no column sums).  variant 4: 128 x 128
 * tile, 64-deep slices, two in LDS; 6: 32-deep, two = 4 workgroups / CU; 9: 128 x 384 tile with 8 waves.  p3_gemm itself picks them from M = 2048 on (N = 384
 * and K >= 1024: 9; other K >= 1024: 4; K <= 512 and N >= 1024: 6; P3_GEMM_DMA=0 switches that off).  All of them add the same 16-deep MFMA blocks in
 * ascending k order as the register-staged kernel: bit-identical outputs. */
int p3_gemm_dma(const void* A, const void* W, void* C, const p3_gemm_desc* d, int variant, void* stream);

/* ------------------------------------------------------------------------------------------
 * "Planes" - the operand format of the fp32x3 ViT block (r05).  A value x of an fp32 tensor travels between the kernels of one timm Block
 * (models/vision_transformer/vit.py:48) as TWO bf16 numbers, hi = bf16(x) and lo = bf16(x - hi) (16 significant bits, the same 4 bytes as the fp32 value), stored
 * as two row-major bf16 matrices with one leading dimension (typically the two halves [:, :K] and [:, K:] of one [M, 2K] buffer).  The PRODUCER writes the
 * split (LayerNorm output, GELU output, attention output, the gradients between the backward GEMMs), so that the consuming GEMM stages all four operand
 * images global -> LDS by LDS-DMA with no conversion pass and multiplies a_lo b_hi + a_hi b_lo + a_hi b_hi on the bf16 MFMA - the arithmetic of P3_F32X3
 * (2^-17 per product) at the memory path of the bf16 kernels.  Weights: the optimizer keeps hi / lo bf16 arenas beside the fp32 master (p3_adamw, shadow_lo).
 *
 * p3_gemm_x3:  C = epilogue(A W^T),  A = a_hi + a_lo [M, K], W = w_hi + w_lo [N, K]
 *   v = A W^T + bias;  act == P3_ACT_GELU: aux <- GELU'(v) (fp32 [M, N], ldaux), v <- GELU(v);  mul != NULL: v *= mul[m, n] (fp32, ldmul: the backward of
 *   that GELU);  residual != NULL: v += residual[m, n] (fp32, ldr);  then C <- v as fp32 (c, ldc; c_lo == NULL) or as planes (c = hi, c_lo = lo, ldc).
 * Shapes: K % 32 == 0, N % 8 == 0, 16-byte aligned rows.  Kernels: K = 256 / 384 with 1024 <= N <= 4096, N % 32 == 0 - the A-stationary persistent kernel
 * (gemm_x3_as.hip: the A rows of a wave live in registers, the weights stream through LDS, one workgroup per CU walks (row block, column block) units);
 * otherwise tiles of 128 x 128 (4 waves) or, for N == 384 and K >= 1024, 128 x 384 (8 waves).
 * ------------------------------------------------------------------------------------------ */
typedef struct {
    int M, N, K;
    const void* a_hi; const void* a_lo; int lda;
    const void* w_hi; const void* w_lo; int ldb;
    void* c; void* c_lo; int ldc;
    const float* bias;
    const float* residual; int ldr;
    int act;
    float* aux; int ldaux;
    const float* mul; int ldmul;
    int tile;             /* 0: the library picks the kernel (measured rule); 1: the 128 x 128 tile kernel, 2: the 128 x 384 tile kernel, 3: the A-stationary kernel -
                           * for THIS call (the host splits a launch with a ragged last round of 128 x 384 tiles into a head on tile 2 and a remainder on tile 1);
                           * the process-wide p3_gemm_x3_tile hook is for measurement tools only and loses against this field */
    /* 3 x 3 convolution as a GEMM over a zero-bordered planes image (conv_ci > 0; the two tile kernels only, P3_EUNSUP on the A-stationary one): A is the image [conv_B, conv_H + 2, conv_W + 2, lda] (p3_pad_nhwc_planes), K = 9 * conv_ci, W is laid out [N, (ky, kx, ci)].  Output row m is
     * interior pixel (b, y, x) = unravel(conv_row0 + m) of the UNPADDED [conv_B, conv_H, conv_W] grid, its A row b P_h P_w + (y + 1) P_w + (x + 1) with
     * P_h = conv_H + 2, P_w = conv_W + 2; the 32-deep slice kt belongs to tap t = kt * 32 / conv_ci and reads A at row + (ky - 1) P_w + (kx - 1), column
     * kt * 32 - t * conv_ci: an interior row +- one pixel never leaves its own padded image.  conv_ci % 32 == 0.  conv_row0: first output pixel of this launch
     * (c, residual, ... address ITS row 0) - the second half of a launch the host splits over the two tile kernels. */
    int conv_B, conv_H, conv_W, conv_ci, conv_row0;
} p3_gemm_x3_desc;
int p3_gemm_x3(const p3_gemm_x3_desc* d, void* stream);
/* measurement hook (tools/mb_x3.py, tools/mb_as.py): 0 = the library's rule, 1 = every product on the 128 x 128 tile, 2 = on the 128 x 384 tile, 3 = on the
 * A-stationary persistent kernel (csrc/gemm_x3_as.hip; P3_EUNSUP unless K = 256 / 384, N % 32 == 0, N <= 4096); returns the previous mode */
int p3_gemm_x3_tile(int mode);
/* weight gradient from planes:  C[N, K] (+)= (a_hi + a_lo)[M, N]^T (b_hi + b_lo)[M, K]  (fp32 C, split over M: fp32 atomics, or - `slabs` given - partial
 * tiles + a fixed-order reduce like p3_gemm_tn_ex); colsum (optional, [N]) += column sums of A (the bias gradient).  M % 64 == 0, N % 128 == 0, K % 128 == 0. */
int p3_gemm_tn_x3(const void* a_hi, const void* a_lo, int lda, const void* b_hi, const void* b_lo, int ldb, float* C, int ldc, int M, int N, int K,
                  float* colsum, float* slabs, int max_slabs, void* stream);
/* weight gradient of a 3 x 3 convolution from planes in ONE launch:  C[N, 9 * Ci] (+)= sum_m (a_hi + a_lo)[m, n] (b_hi + b_lo)[m + s_t, c]  for column
 * t * Ci + c, s_t = (t / 3 - 1) * Pw + (t % 3 - 1).  A: the output gradient in the zero-bordered row space [M, N] (rows outside the interior are zero), B: the
 * zero-bordered input image [M, Ci] in the same row space; b_hi / b_lo address ITS row 0 and the buffer holds Pw + 1 readable (zero) guard rows in front of it
 * and behind row M - 1: the shifted rows of the first and last padded image rows are READ (and multiplied by zero).  M % 64 == 0, N % 128 == 0, Ci % 128 == 0;
 * column tiles never straddle a tap (the 128 x 384 tile needs Ci % 384 == 0).  Splits, slabs, parking and the fixed-order reduce as in p3_gemm_tn_x3. */
int p3_gemm_tn_x3_conv(const void* a_hi, const void* a_lo, int lda, const void* b_hi, const void* b_lo, int ldb, float* C, int ldc, int M, int N, int Ci, int Pw,
                       float* slabs, int max_slabs, void* stream);
/* fp32 [B*H*W, C] (ld_src) -> zero-bordered PLANES image [B, H+2, W+2, C] (hi, lo address padded row 0; ld_dst) for the convolution forms of p3_gemm_x3 /
 * p3_gemm_tn_x3_conv: border pixels, the `guard` rows in front of row 0 and the rows B (H+2) (W+2) .. rows_total + guard - 1 behind the image are written as
 * zeros in the same pass.  pre != NULL: the value split is src + a[c] + b[c] * pre[m, c] (ld_pre) - p3_affine_fix_ld's arithmetic, the BatchNorm statistics term
 * of a gradient, without writing the fp32 gradient back.  The image has Cp >= C columns, columns C .. Cp - 1 zero (a 64-channel gradient as the 128-column operand
 * of the weight-gradient kernel).  C % 8 == 0, Cp % 8 == 0. */
int p3_pad_nhwc_planes(const float* src, int ld_src, const float* pre, int ld_pre, const float* a, const float* b, void* hi, void* lo, int ld_dst, int B, int H,
                       int W, int C, int Cp, int guard, int64_t rows_total, void* stream);
/* sums[0 .. N) = column sums, sums[N .. 2N) = column sums of squares of fp32 x [M, N] (ld): workgroup partials in `scratch` (scratch_floats >= 2 N; as many
 * workgroups as fit, at most 1024) added in workgroup order in float64 - the same bits on every run (the BatchNorm batch statistics of a planes GEMM's output).
 * N % 4 == 0, N <= 1024. */
int p3_col_stats(const float* x, int ld, int64_t M, int N, float* sums, float* scratch, int64_t scratch_floats, void* stream);
/* measurement hook: 0 keeps every weight gradient on the 128 x 128 tile (the 128 x 384 tile is the default where K % 384 == 0 and it has >= 8 tiles); returns the previous setting */
int p3_gemm_tn_x3_wide(int on);
/* fp32 [rows, cols] (ld_src) -> planes (hi, lo; ld_dst), and back (x = hi + lo): the seams of the planes region (attention outputs, tests) */
int p3_to_planes(const float* src, int ld_src, void* hi, void* lo, int ld_dst, int64_t rows, int cols, void* stream);
int p3_from_planes(const void* hi, const void* lo, int ld_src, float* dst, int ld_dst, int64_t rows, int cols, void* stream);

/* ------------------------------------------------------------------------------------------
 * LayerNorm over the last dim:  y = (x - mean) / sqrt(var + eps) * gamma + beta
 * timm Block.norm1/norm2/VisionTransformer.norm (eps 1e-6); nn.TransformerDecoderLayer.norm1..3
 * (eps 1e-5, models/pix2poly/model_pix2poly.py:138).  x dtype_in, y dtype_out; optional save of
 * mean / rstd (float[rows]) for the backward pass.
 * ------------------------------------------------------------------------------------------ */
int p3_layernorm(const void* x, const float* gamma, const float* beta, void* y, int64_t rows, int cols, int ldx, int ldy,
                 float eps, int dtype_in, int dtype_out, float* save_mean, float* save_rstd, void* stream);
/* dres (optional, dtype_dx, [rows, cols]): gradient arriving at x through a residual connection; added to dx in the same pass */
int p3_layernorm_bwd_res(const void* dy, const void* x, const float* gamma, const float* mean, const float* rstd, const void* dres,
                         void* dx, float* dgamma, float* dbeta, int64_t rows, int cols, int dtype_dy, int dtype_x, int dtype_dx,
                         void* stream);
/* dx_lo (optional, bf16 [rows, cols], needs cols % 128 == 0 and an fp32 dx): a bf16 copy of dx written in the same pass - what the
 * GEMMs of the sublayer below read, instead of a separate cast pass over the fp32 residual-gradient stream */
int p3_layernorm_bwd_lo(const void* dy, const void* x, const float* gamma, const float* mean, const float* rstd, const void* dres,
                        void* dx, void* dx_lo, float* dgamma, float* dbeta, int64_t rows, int cols, int dtype_dy, int dtype_x, int dtype_dx,
                        void* stream);
/* lo_drop (optional; needs dx_lo, no dres, bf16 dy, fp32 x / dx, cols 256 / 384 / 768): dx_lo = mask(dx) / (1-p) with the mask of
 * dropout site lo_drop at element (row, col) - the gradient the nn.Dropout in front of this LayerNorm's residual add
 * (nn.TransformerDecoderLayer.dropout1..3, model_pix2poly.py:136) passes down, so that sublayer's backward needs no p3_dropout_apply pass.
 * dx (the residual path) is not masked. */
int p3_layernorm_bwd_lo_drop(const void* dy, const void* x, const float* gamma, const float* mean, const float* rstd, const void* dres,
                             void* dx, void* dx_lo, const p3_dropout* lo_drop, float* dgamma, float* dbeta, int64_t rows, int cols,
                             int dtype_dy, int dtype_x, int dtype_dx, void* stream);
/* planes forms (fp32x3 ViT block, see p3_gemm_x3): LayerNorm of the fp32 stream written as planes (y_hi, y_lo, row stride ldy) - the qkv / fc1 operand;
 * and the backward whose fp32 dx (the residual-gradient stream, + dres) is ALSO written as planes from the same registers (dx_hi, dx_lo, ld_planes): the
 * operand of the dX / dW GEMMs of the sublayer below. */
int p3_layernorm_planes(const float* x, const float* gamma, const float* beta, void* y_hi, void* y_lo, int64_t rows, int cols, int ldx, int ldy, float eps,
                        float* save_mean, float* save_rstd, void* stream);
int p3_layernorm_bwd_planes(const float* dy, const float* x, const float* gamma, const float* mean, const float* rstd, const float* dres, float* dx,
                            void* dx_hi, void* dx_lo, int ld_planes, float* dgamma, float* dbeta, int64_t rows, int cols, void* stream);
int p3_layernorm_bwd(const void* dy, const void* x, const float* gamma, const float* mean, const float* rstd, void* dx,
                     float* dgamma, float* dbeta, int64_t rows, int cols, int dtype_dy, int dtype_x, int dtype_dx,
                     void* stream);

/* ------------------------------------------------------------------------------------------
 * Fused scaled-dot-product attention (flash style, MFMA):  O = softmax(Q K^T * scale + bias) V
 * Replaces F.scaled_dot_product_attention in timm Attention (785x785, 6 heads x 64) and the three
 * attention products of nn.TransformerDecoderLayer (models/pix2poly/model_pix2poly.py:177-182):
 *   causal != 0   : tgt_mask of create_mask (model_pix2poly.py:12-19), keys j > i masked to -inf
 *   key_bias      : float [B, Lk] ADDED to the scores - the reference passes (tgt == PAD).float() as
 *                   tgt_key_padding_mask, which torch treats as an additive +1.0 bias (model_pix2poly.py:28-29)
 * Q/K/V/O are addressed as  ptr + b*batch_stride + t*row_stride + h*head_dim  (elements).
 * lse (optional, float [B,H,Lq]) receives log-sum-exp rows for the backward pass.
 * head_dim in {32, 64}.
 * ------------------------------------------------------------------------------------------ */
typedef struct {
    int B, H, Lq, Lk, head_dim;
    int64_t q_bs, k_bs, v_bs, o_bs; /* batch strides */
    int q_rs, k_rs, v_rs, o_rs;     /* row (token) strides */
    float scale;
    int causal;
    const float* key_bias; /* [B, Lk] or NULL */
    int dtype;             /* Q,K,V,O dtype */
    float* lse;            /* [B,H,Lq] or NULL */
    p3_dropout drop;       /* dropout of the attention probabilities; element = (row (b*H + h)*Lq + q, col k) */
    unsigned int* drop_rows; /* optional keep-bit words, B*H*ceil(Lk/32)*Lq of them laid out [B*H][ceil(Lk/32)][Lq] (bit k%32 of word k/32
                              * of query q = element kept; q innermost so that a wave's 32 queries touch 128 contiguous bytes): WRITTEN
                              * by p3_attention when given, READ by p3_attention_bwd instead of re-hashing (NULL: hash again) */
    int grad_planes;        /* p3_attention_bwd with dtype P3_F32X3 only: 1 = dQ / dK / dV are written as PLANES (see p3_gemm_x3): the pointers address the bf16 hi
                             * plane with batch stride g_bs and row stride g_rs (bf16 elements), the lo plane lies g_lo elements behind - the packed qkv gradient
                             * leaves as the operand of the projection's dX / dW GEMMs, no fp32 tensor and no conversion pass.  0: dtype / strides of Q, K, V */
    int g_rs;
    int64_t g_bs, g_lo;
    void* o_planes;         /* p3_attention with dtype P3_F32X3 only, optional: the output ALSO as planes - the bf16 hi plane of O at o_planes + b*op_bs + t*op_rs + h*head_dim
                             * (bf16 elements), the lo plane op_lo elements behind it: the operand of the output projection's planes GEMM, written from the registers that
                             * hold the fp32 row (r06: replaces a p3_to_planes pass over O per ViT block).  O itself is written as before (the backward reads it) */
    int op_rs;
    int64_t op_bs, op_lo;
} p3_attn_desc;
int p3_attention(const void* Q, const void* K, const void* V, void* O, const p3_attn_desc* d, void* stream);



/* ------------------------------------------------------------------------------------------
 * LiDAR pillar stem = PointPillarsEncoder.forward (models/pointpillars/pointpillars_o3d.py:85-107):
 * Open3D-ML PointPillars.voxelize (hard voxelisation: inclusive range test, <= max_points lowest point
 * indices per pillar, <= max_voxels pillars per sample in ascending hash order) -> PillarFeatureNet
 * (decorate to 8 ch; Linear(8,32,no bias)+BatchNorm1d(eps 1e-3, momentum 0.01)+ReLU+max+concat;
 * Linear(64,C)+BN+ReLU+max; padded slots are zeros and take part in BN statistics and in the max) ->
 * PointPillarsScatter.  Input is the jagged layout of datasets/collate_funcs.py:108:
 * values [sumN,3] f32 + offsets [B+1] int64.  Output: token-major canvas out[b, y*nx+x, col_off + c]
 * (row stride out_ld) = NHWC of the reference's [B,C,ny,nx]; empty pillars are exact zeros.
 * training != 0: BatchNorm batch statistics + running-stat update, else running statistics.
 * ------------------------------------------------------------------------------------------ */
typedef struct {
    int B;
    int64_t total_points; /* offsets[B] (rows of `values`) */
    int nx, ny;           /* pillar grid (patch_feature_width/height) */
    float vx, vy, vz;     /* in_voxel_size */
    float zmax;           /* point_cloud_range z max (range min is 0) */
    int max_points;       /* max_num_points_per_voxel (1..4096; > 64 = the lidar_density_ablation{128,256,512} configs) */
    int max_voxels;       /* max_num_voxels.{train,test} */
    int C;                /* patch_feature_dim */
    int training;
    float bn_eps, bn_momentum;
    int dtype;            /* dtype of w2, of the internal X2/H2 matrices and of `out` */
    int out_ld, out_col_off;
    int no_backward;      /* != 0: no p3_pillar_stem_bwd will follow on this workspace - the layer-1 activation matrix need not be kept (C = 128 / 384, bf16 / P3_F32X3: never written) */
} p3_pillar_desc;
int64_t p3_pillar_stem_workspace_bytes(const p3_pillar_desc* d);
int p3_pillar_stem(const float* values, const int64_t* offsets, const float* w1, const float* bn1_gamma,
                   const float* bn1_beta, float* bn1_rmean, float* bn1_rvar, const void* w2, const float* bn2_gamma,
                   const float* bn2_beta, float* bn2_rmean, float* bn2_rvar, void* out, void* workspace,
                   const p3_pillar_desc* d, void* stream);
/* byte offsets (18 int64) of the workspace sections: sorted, vox_xy, vox_start, vox_cnt, vox_row, nvox, X2, H2, hmax, hmin, F8 (decorated
 * point features per X2 row), row_vox (pillar slot per row, -1 unused), row_w, then the statistics SyncBatchNorm all-reduces between the
 * phases: totals (int32: kept pillars of the batch), sums1 (fp32 [2*32]), sums2 (fp32 [2*C]), acc1 (fp32 [584]: layer-0 backward sums),
 * acc1_stat (inside acc1: fp32 [2*32] = dbeta1 | dgamma1, acc1[520:584]) */
int p3_pillar_stem_layout(const p3_pillar_desc* d, int64_t* offsets);
/* p3_pillar_stem split at its two BatchNorm statistics (nn.SyncBatchNorm.convert_sync_batchnorm, model_pix2poly.py:326): phases is a
 * bit mask, 1 = pillarize + layer-0 sums, 2 = layer-0 apply + layer-1 GEMM + sums, 4 = finalize + scatter; all-reduce totals / sums1
 * after phase 1 and sums2 after phase 2.  p3_pillar_stem == phases 7. */
int p3_pillar_stem_phased(const float* values, const int64_t* offsets, const float* w1, const float* bn1_gamma,
                          const float* bn1_beta, float* bn1_rmean, float* bn1_rvar, const void* w2, const float* bn2_gamma,
                          const float* bn2_beta, float* bn2_rmean, float* bn2_rvar, void* out, void* workspace,
                          const p3_pillar_desc* d, int phases, void* stream);
/* Backward of p3_pillar_stem w.r.t. the PillarFeatureNet parameters (what autograd produces for
 * PointPillarsEncoder.forward, pointpillars_o3d.py:85-107: voxel_encoder.pfn_layers.{0,1}.{linear.weight, norm.weight, norm.bias};
 * the point coordinates carry no gradient).  dcanvas: gradient of the token-major canvas the forward wrote (same dtype, row stride
 * dcanvas_ld; columns d->out_col_off .. +C are read).  w2t = pfn_layers.1.linear.weight transposed, [64, C] in the compute dtype.
 * `workspace` must be the buffer the matching forward call filled (pillar tables, layer inputs / outputs, BatchNorm statistics) and
 * is consumed.  Outputs (fp32, overwritten): dw1 [32,8], dg1/db1 [32], dw2 [C,64], dg2/db2 [C]. */
int p3_pillar_stem_bwd(const void* dcanvas, int dcanvas_ld, const float* w1, const float* bn1_gamma, const void* w2t,
                       const float* bn2_gamma, void* workspace, const p3_pillar_desc* d, float* dw1, float* dg1, float* db1,
                       float* dw2, float* dg2, float* db2, void* stream);
/* The same in phases (1 = layer-1 arg-max gradients + local dg2/db2, 2 = dH2 rows + GEMMs + layer-0 sums, 4 = layer-0 finalize) for
 * SyncBatchNorm: stat2 = all-reduced [db2 (C) | dg2 (C)], stat1 = all-reduced [dbeta1 (32) | dgamma1 (32)] (acc1[520:584]) feed the
 * input-gradient terms; NULL = this rank's own sums.  The parameter gradients written to dg*, db* stay per-rank, as in torch. */
int p3_pillar_stem_bwd_phased(const void* dcanvas, int dcanvas_ld, const float* w1, const float* bn1_gamma, const void* w2t,
                              const float* bn2_gamma, void* workspace, const p3_pillar_desc* d, float* dw1, float* dg1, float* db1,
                              float* dw2, float* dg2, float* db2, const float* stat2, const float* stat1, int phases, void* stream);

/* ------------------------------------------------------------------------------------------
 * HBM-bound glue of the encoders / decoder (each replaces a chain of ATen elementwise kernels)
 * ------------------------------------------------------------------------------------------ */
/* im2col of timm PatchEmbed.proj (Conv2d k=P, s=P): img NCHW f32 -> rows [B*(H/P)*(W/P), Cin*P*P], k = c*P*P + py*P + px */
int p3_patchify(const float* img, void* out, int B, int Cin, int H, int W, int P, int dtype_out, void* stream);
/* the same rows with a leading dimension ldk >= Cin*P*P (<= 1024): columns [Cin*P*P, ldk) are written as zeros, so that a K that no GEMM
 * kernel takes (patch 14: K = 588) runs as K = ldk against a weight zero-padded in the same way */
int p3_patchify_ld(const float* img, void* out, int B, int Cin, int H, int W, int P, int ldk, int dtype_out, void* stream);
/* DINOv2 (vit_dinov2.py: the hub model's interpolate_pos_encoding): bicubic (A = -0.75, align_corners = False, no antialias, clamped border)
 * resampling of the trained position table [1 + n_in*n_in, D] to [1 + n_out*n_out, D]; row 0 (CLS) passes through.  The operator is separable
 * and linear: out[y, x, :] = sum_i sum_j wy[y, i] wx[x, j] table[i, j, :] with host-built tap tables wy, wx [n_out, n_in] (device fp32).
 * _bwd is the transposed gather (one workgroup per source cell, fixed order, no atomics): dtable[i, j, :] = sum_y sum_x wy[y, i] wx[x, j] dout[y, x, :].
 * D % 4 == 0, D <= 4096, 16-byte aligned tensors. */
int p3_posembed_resample(const float* table, const float* wy, const float* wx, float* out, int n_in, int n_out, int D, void* stream);
int p3_posembed_resample_bwd(const float* dout, const float* wy, const float* wx, float* dtable, int n_in, int n_out, int D, void* stream);
/* DINOv2 LayerScale folded into the branch's last Linear: res + gamma * (W a + b) = res + (diag(gamma) W) a + gamma * b.
 *   fold:  Wf[n, :] = gamma[n] W[n, :],  bf[n] = gamma[n] b[n]                      (W [N, K] fp32, K % 4 == 0; b / bf may be NULL)
 *   bwd:   dW = gamma[:, None] dWf,  db = gamma dbf,  dgamma[n] = sum_k dWf[n, k] W[n, k] + dbf[n] b[n]   (one wave per row, fixed order;
 *          dgamma never divides by gamma) */
int p3_layerscale_fold(const float* gamma, const float* W, const float* b, float* Wf, float* bf, int N, int K, void* stream);
int p3_layerscale_fold_bwd(const float* gamma, const float* W, const float* b, const float* dWf, const float* dbf, float* dW, float* db,
                           float* dgamma, int N, int K, void* stream);
/* timm VisionTransformer._pos_embed (+ fusion BN2d+ReLU, early_fusion_vit.py:75-79,123 when scale/shift given):
 *   x[b,0,:] = cls + pos[0];  x[b,1+p,:] = f(src[b,p,:]) + pos[1+p];  x is the fp32 residual stream [B, np+1, D] */
int p3_tokens_assemble(const void* src, int src_ld, int dtype_src, const float* scale, const float* shift, const float* cls,
                       const float* pos, float* x, int B, int np, int D, void* stream);
/* drop CLS + nn.AdaptiveAvgPool1d(Dout) over channels (vit.py:41,49; early_fusion_vit.py:94,125) (+ Decoder's
 * `encoder_out + encoder_pos_embed`, model_pix2poly.py:171-173, when pos != NULL).  y: [B, np+1, Din] */
int p3_pool_pos(const void* y, int dtype_in, const float* pos, void* out, void* out_nopos, int dtype_out, int B, int np, int Din,
                int Dout, void* stream);
/* Decoder.forward head (model_pix2poly.py:164-168 + create_mask :21-31): x = embedding[tgt] + decoder_pos_embed,
 * key_bias = (tgt == pad).float() */
int p3_embed_tokens(const int64_t* tokens, const float* emb, const float* pos, void* x, float* key_bias, int B, int L, int D,
                    int pad_idx, int dtype_out, void* stream);
/* ScoreNet.forward (model_pix2poly.py:86-112), never materialising the [B,512,N,N] pair tensor:
 *   p3_pair_mean   feats[:,1:] -> mean of token pairs [B,N,D]
 *   p3_gemm x2     U = F W1[:, :D]^T + b1, V = F W1[:, D:]^T              (conv1 is separable over (i, j))
 *   p3_pair_stats  closed-form BatchNorm2d batch statistics of U_i + V_j  (sums[0:C] = sum, sums[C:2C] = sum of squares)
 *   p3_bn_finalize scale/shift (+ running stats update, torch momentum semantics)
 *   p3_gemm        conv2 with P3_A_PAIR_AFFINE_RELU, conv3 with P3_A_AFFINE_RELU (colsum -> next BN)
 *   p3_score_out   BN3+ReLU+conv4 -> scores [B,N,N]; transpose_accumulate adds s2^T (perm = s1 + s2^T, :257-259) */
int p3_pair_mean(const void* feats, void* out, int B, int L, int N, int D, int dtype, void* stream);
int p3_pair_stats(const void* U, const void* V, int B, int N, int C, int dtype, float* sums, void* stream);
int p3_bn_finalize(const float* sums, int C, float count, const float* gamma, const float* beta, float* running_mean,
                   float* running_var, float eps, float momentum, int training, float* scale, float* shift, float* save_mean,
                   float* save_rstd, void* stream);
int p3_score_out(const void* H3, int dtype, const float* scale, const float* shift, const float* w4, const float* b4, float* out,
                 int B, int N, int C, int transpose_accumulate, void* stream);
/* log_optimal_transport (model_pix2poly.py:44-66) + [:, :m, :n] + softmax(-1) (:261-264) in one launch.
 * perm [B,m,n] (may be NULL), z_full [B,m+1,n+1] = log_optimal_transport's return value (may be NULL),
 * uv_hist [B,iters,(m+1)+(n+1)] optional dual iterates for the backward pass. */
int p3_sinkhorn(const float* scores, const float* alpha, int B, int m, int n, int iters, float* perm, float* z_full,
                float* uv_hist, void* stream);
/* scores_to_permutations (predictor_pix2poly.py:307-319): per tile scipy.optimize.linear_sum_assignment(-scores[b]) (maximize = 1),
 * the float64 shortest-augmenting-path solver with scipy's tie rule, one wave per tile.  scores [B,N,N] fp32;
 * col4row [B,N] (column assigned to row r; -1 if the tile failed); perm [B,N,N] 0/1 fp32 (may be NULL);
 * status [B]: 0 ok, 1 NaN / -inf cost (scipy: ValueError "invalid numeric entries"), 2 infeasible. */
int p3_assignment(const float* scores, int B, int N, int maximize, int32_t* col4row, float* perm, int32_t* status, void* stream);
/* greedy decode step (predictor_pix2poly.py:165,196-197): argmax over the last dim, first maximum wins */
int p3_argmax(const float* x, int64_t* out, int rows, int cols, int ld, void* stream);

/* One nn.TransformerDecoderLayer (post-norm, ReLU, eval mode) applied to ONE new position per sample with key/value caches: the body
 * of Decoder.predict's loop (model_pix2poly.py:187-219, layer built at :138-141) as a single launch.  bf16 activations / weights, fp32
 * biases and LayerNorm parameters; D = 256, 8 heads, FF = 2048.  Weights are row-major [out, in] like nn.Linear.weight. */
typedef struct {
    int B, t, steps, Lmem;       /* batch, index of the new position, cache length (positions), memory tokens */
    int D, H, FF;
    const void* x_in;  long long x_in_stride;    /* [B] rows of D bf16 */
    void* x_out;       long long x_out_stride;   /* [B] rows of D bf16: norm3 output */
    void* kv_self;               /* [B, steps, 3D] bf16: row t is WRITTEN (q|k|v of the new position), rows < t are read */
    const void* kv_mem;          /* [B, Lmem, 2D] bf16: k|v of the memory tokens (multihead_attn.in_proj rows D..3D applied once) */
    const float* key_bias; long long key_bias_stride;   /* [B] rows of >= t+1 floats added to the self-attention scores, or NULL */
    const void* w_in;  const float* b_in;        /* self_attn.in_proj   [3D, D] */
    const void* w_so;  const float* b_so;        /* self_attn.out_proj  [D, D] */
    const void* w_q;   const float* b_q;         /* multihead_attn.in_proj rows 0..D (query)  [D, D] */
    const void* w_co;  const float* b_co;        /* multihead_attn.out_proj [D, D] */
    const void* w1;    const float* b1;          /* linear1 [FF, D] */
    const void* w2;    const float* b2;          /* linear2 [D, FF] */
    const float *g1, *be1, *g2, *be2, *g3, *be3; /* norm1..3 weight / bias */
    float eps, scale;            /* LayerNorm eps; 1/sqrt(D/H) */
    int cluster;                 /* workgroups per sample: 1, or 4 (heads / hidden units split over the cluster; needs the three below) */
    float* exch;                 /* [B, 3, cluster, D] fp32 scratch: the partial projections the cluster members exchange */
    unsigned int* sync;          /* [B, 2] {arrival count, generation}: zero before the FIRST launch, never touched by the host afterwards */
    int* err;                    /* optional: set to 1 if a cluster barrier gave up (spin limit) - the outputs are then invalid */
    int fp32;                    /* 0 (a zeroed descriptor, the r02 layout's meaning): x_in / x_out / kv_self / kv_mem and the six weight matrices are
                                  * bf16 as the comments above say; 1 (r03): all of them fp32 - the parity mode's decode step as one launch per
                                  * layer too, nothing rounded between the stages */
} p3_decode_layer_desc;
int p3_decode_layer(const p3_decode_layer_desc* d, void* stream);
int p3_cast(const void* a, int dtype_a, void* b, int dtype_b, int64_t n, void* stream);
/* out[b,t,:] = x[b,t,:] + pos[t,:]  (Decoder: encoder_out + encoder_pos_embed, model_pix2poly.py:171-173) */
int p3_add_pos(const void* x, const float* pos, void* out, int B, int L, int D, int dtype, void* stream);

/* ------------------------------------------------------------------------------------------
 * Training step (a-11: trainer_pix2poly.py:284-351 = forward, CE + 10*BCE, backward, AdamW)
 * ------------------------------------------------------------------------------------------ */
/* attention backward (recompute, no atomics): delta_ws float [B,H,Lq] scratch; dQ/dK/dV use the q/k/v strides, dO the o strides */
int p3_attention_bwd(const void* Q, const void* K, const void* V, const void* O, const void* dO, const float* lse, void* dQ,
                     void* dK, void* dV, float* delta_ws, const p3_attn_desc* d, void* stream);
/* weight gradient: C[N,K] += A[M,N]^T B[M,K] (fp32 C, split over M with fp32 atomics) ; column sums (bias gradients) */
int p3_gemm_tn(const void* A, const void* B, float* C, int M, int N, int K, int lda, int ldb, int ldc, int dtype, void* stream);
int p3_colsum(const void* x, float* out, int64_t M, int N, int ld, int dtype, void* stream);
/* dpre = dy * act'(.)  (GELU: saved = pre-activation; ReLU: saved = output) */
/* scale: extra factor on dy (1/(1-p) when a dropout followed the activation: the saved ReLU output is already masked) */
int p3_act_bwd(const void* dy, int dtype_dy, const void* saved, int dtype_saved, void* out, int dtype_out, int64_t n, int act, float scale,
               void* stream);
/* dpos may be NULL (then take it as the column sums of dx viewed as [B, L*D]: no atomics) */
int p3_embed_tokens_bwd(const void* dx, int dtype, const int64_t* tokens, float* demb, float* dpos, int B, int L, int D, void* stream);
/* the embedding part alone for a vocabulary of V rows (nn.Embedding backward of model_pix2poly.py:135,164): tokens outside [0, V) are ignored;
 * V * 256 bytes of LDS per workgroup (falls back to the atomics form above beyond 64 KiB) */
int p3_embed_tokens_bwd_v(const void* dx, int dtype, const int64_t* tokens, float* demb, int B, int L, int D, int V, void* stream);
/* dscale is the centred sum  sum dz*(src - mean)  when mean != NULL (feeds p3_bn_bwd_coeffs) */
int p3_tokens_assemble_bwd(const float* dx, const void* src, int src_ld, int dtype_src, const float* scale, const float* shift, const float* mean,
                           void* dsrc, float* dscale, float* dshift, int B, int np, int D, void* stream);
int p3_pool_pos_bwd(const void* dout, int dtype_dout, void* dy, int dtype_dy, int B, int np, int Din, int Dout, void* stream);
int p3_pair_mean_bwd(const float* dF, void* dfeats, int dtype, int B, int L, int N, int D, int accumulate, void* stream);
/* reverse-mode through all Sinkhorn iterations + slice + softmax in one launch (uv_hist from p3_sinkhorn) */
/* workspace: p3_sinkhorn_bwd_workspace_bytes(B, m, n, iters) bytes of device scratch (per-tile path flags + the per-iteration
 * row / column factor vectors of the linear-domain sweep) */
int p3_sinkhorn_bwd(const float* scores, const float* alpha, int B, int m, int n, int iters, const float* perm,
                    const float* uv_hist, const float* dperm, float* dscores, float* dalpha, void* workspace, void* stream);
int64_t p3_sinkhorn_bwd_workspace_bytes(int B, int m, int n, int iters);
/* nn.CrossEntropyLoss(ignore_index) / nn.BCELoss (trainer_pix2poly.py:91-93): acc[0] = loss sum, acc[1] = #valid rows;
 * backward kernels read the upstream gradient x loss weight from the device scalar `gscale` (no host sync) */
int p3_ce_loss_fwd(const float* logits, int ld, const int64_t* targets, int R, int V, int ignore_index, float* row_lse, float* acc, void* stream);
int p3_ce_loss_bwd(const float* logits, int ld, const int64_t* targets, int R, int V, int ignore_index, const float* row_lse,
                   const float* acc, const float* gscale, void* dlogits, int dtype_out, int ld_out, int Vpad, void* stream);
int p3_bce_loss_fwd(const float* p, const float* y, int64_t n, float* acc, void* stream);
int p3_bce_loss_bwd(const float* p, const float* y, int64_t n, const float* gscale, float* dp, void* stream);
/* Device-side step counter + learning-rate schedule of the optimizer (torch.optim.AdamW bias corrections, and the reference's
 * transformers.get_linear_schedule_with_warmup, train/trainer_pix2poly.py:62-77): reads step[0] = s (optimizer steps done), writes
 * hyper = {base_lr * lambda(s), 1 - beta1^(s+1), 1 - beta2^(s+1)} and step[0] = s + 1.  kind 0 = constant, 1 = linear warm-up / decay.
 * Launch it right before p3_adamw on the same stream (inside the captured step graph). */
int p3_adamw_schedule(long long* step, float* hyper, float base_lr, int kind, int warmup_steps, int total_steps, float beta1, float beta2,
                      void* stream);
/* the same with sched = device float[4] {base_lr, kind, warm-up steps, total steps} (all < 2^24: exact in fp32) read by the kernel: a captured
 * step follows a learning rate / schedule the host rewrites after the capture */
int p3_adamw_schedule_dev(long long* step, float* hyper, const float* sched, float beta1, float beta2, void* stream);
/* torch.optim.AdamW step over a flat parameter arena; hyper = {lr, 1-beta1^t, 1-beta2^t} on the device; optional bf16 shadow */
int p3_adamw(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, const float* hyper, float beta1,
             float beta2, float eps, float weight_decay, float grad_scale, void* bf16_shadow, void* stream);

/* ScoreNet backward (model_pix2poly.py:69-112) without the [B,512,N,N] pair tensor; see csrc/scorenet_bwd.hip.
 * p3_gemm_tn_ex: weight gradient with a generated B operand  B' = relu((B (+V)) * b_scale + b_shift)  (b_mode = P3_A_*). */
int p3_gemm_tn_ex(const void* A, const void* B, float* C, int M, int N, int K, int lda, int ldb, int ldc, int dtype, int b_mode,
                  const float* b_scale, const float* b_shift, const void* pair_V, int pair_n, float* colsum /* optional [N]: += column sums of A */,
                  float* slabs /* optional scratch [max_slabs][N][K] fp32: split-M partials stored + reduced instead of fp32 atomics */,
                  int max_slabs, void* stream);
/* tail (dS != NULL, C = 64): dS [B,N,N] (read transposed if transpose) -> dHd = dz*scale, acc = [dscale(C) | dshift(C) | dw4(C) | db4]
 * matrix (dA != NULL, C = 128): dA [R,C] -> dHd = dA*(z>0)*scale (may alias dA), acc = [dscale(C) | dshift(C)] */
int p3_row_affine_bwd(const void* dA, const float* dS, const void* H, const float* scale, const float* shift, const float* mean, const float* w4,
                      void* dHd, float* acc, int64_t R, int C, int N, int transpose, int dtype, void* stream);
/* Two-pass form for train-mode BatchNorm: call once with dHd = NULL (sums only, nothing stored), derive (a, b) with
 * p3_bn_bwd_coeffs, call again with acc = NULL and fix_a / fix_b to write the final gradient dz*scale + a + b*H directly. */
int p3_row_affine_bwd2(const void* dA, const float* dS, const void* H, const float* scale, const float* shift, const float* mean,
                       const float* w4, void* dHd, float* acc, const float* fix_a, const float* fix_b, int64_t R, int C, int N,
                       int transpose, int dtype, void* stream);
/* BatchNorm backward through scale/shift and (train mode) the batch statistics: d(pre) = direct + a[c] + b[c]*pre.
 * `dscale` is the CENTRED sum  sum dz*(pre - mean)  as accumulated by p3_row_affine_bwd / p3_pair_bwd (acc[0:C]).
 * training: bit 0 = batch statistics (a, b non-zero), bit 1 = dgamma / dbeta are accumulated (+=) instead of stored */
int p3_bn_bwd_coeffs(const float* dscale, const float* dshift, const float* gamma, const float* mean, const float* rstd, float count,
                     int training, int C, float* dgamma, float* dbeta, float* a, float* b, void* stream);
int p3_affine_fix(void* dH, const void* H, const float* a, const float* b, int64_t R, int C, int dtype, void* stream);
/* same with a row stride on H (dH stays dense [R, C]) */
int p3_affine_fix_ld(void* dH, const void* H, int ldh, const float* a, const float* b, int64_t R, int C, int dtype, void* stream);
/* pair grid: dA [B*N*N, C] -> dU (written), dV (+=, zero-filled by the caller) [B*N, C] fp32, acc = [dscale(C) | dshift(C)] */
int p3_pair_bwd(const void* dA, const void* U, const void* V, const float* scale, const float* shift, const float* mean, float* dU, float* dV, float* acc,
                int B, int N, int C, int dtype, void* stream);
/* same with a scratch of p3_pair_bwd_workspace_bytes(B, N, C) bytes: the per-block dV partial rows are stored there and summed by a second
 * kernel instead of being added with global fp32 atomics (bf16 path; other dtypes ignore the workspace) */
int64_t p3_pair_bwd_workspace_bytes(int B, int N, int C);
int64_t p3_pair_bwd_workspace_bytes_dt(int B, int N, int C, int dtype);   /* per dtype: the fp32 form takes smaller row chunks (more slabs) */
int p3_pair_bwd_ws(const void* dA, const void* U, const void* V, const float* scale, const float* shift, const float* mean, float* dU, float* dV,
                   float* acc, int B, int N, int C, int dtype, void* workspace, void* stream);
/* p3_gemm (dA2 = dH2 . W2, the input gradient of ScoreNet.conv2, model_pix2poly.py:76) and p3_pair_bwd in ONE launch (bf16; csrc/pair_bwd_mma.hip): a
 * workgroup owns (tile, 8 rows i, all j), the 128 x 256 product tiles of dA2 stay in its MFMA accumulators and are masked / summed there - the
 * [B N^2, 256] gradient (1.2 GB per net at B = 64, N = 192) is neither written nor read.  dH2 [B N^2, 128] bf16 (dense), W2t = conv2.weight transposed
 * [256, 128] bf16, U / V [B N, 256] bf16, scale / shift / mean [256] fp32; outputs as p3_pair_bwd: dU (=), dV (+=, zero it first), acc[0:256] += centred
 * scale sums, acc[256:512] += shift sums.  workspace: p3_pair_bwd_fused_workspace_bytes(B, N) bytes (dV partial rows of the N / 8 row blocks). */
/* From G [N, 2K] = p3_gemm_tn_ex(dH [M, N], H [M, K], P3_A_AFFINE_MASK2) (G | G2 side by side, row stride ldg) and W [N, K] fp32 (the weight of the layer
 * dH belongs to, e.g. ScoreNet.conv3.weight, model_pix2poly.py:78): dW [N, K] += scale G2 + shift G (that layer's weight gradient over relu(bn(H))), and
 * acc[0:K] += sum dz (H - mean), acc[K:2K] += sum dz for dz = [bn(H) > 0] (dH W) - the BatchNorm backward sums of the layer below, WITHOUT a pass over
 * the [M, K] input gradient (r01 - r03: p3_row_affine_bwd pass 1, 290 us per ScoreNet at B = 64). */
int p3_bn_sums_from_g(const float* G, int ldg, const float* W, const float* scale, const float* shift, const float* mean, float* dW, float* acc,
                      int N, int K, void* stream);
int64_t p3_pair_bwd_fused_workspace_bytes(int B, int N);
int p3_pair_bwd_fused(const void* dH2, const void* W2t, const void* U, const void* V, const float* scale, const float* shift, const float* mean,
                      float* dU, float* dV, float* acc, int B, int N, void* workspace, void* stream);
int p3_pair_stats_bwd(const void* U, const void* V, const float* a, const float* b, float* dU, float* dV, int B, int N, int C, int dtype,
                      void* stream);
/* the same launch for P3_F32X3 (csrc/pair_bwd_x3.hip): everything fp32 in memory (dH2 [B N^2, 128], W2t [256, 128], U / V [B N, 256]), the products as
 * three bf16 MFMA terms with fp32 accumulation; W2t's hi / lo split lives in registers.  Same outputs, same workspace size. */
int p3_pair_bwd_fused_x3(const float* dH2, const float* W2t, const float* U, const float* V, const float* scale, const float* shift, const float* mean,
                         float* dU, float* dV, float* acc, int B, int N, void* workspace, void* stream);

/* ------------------------------------------------------------------------------------------
 * FFL / *CNN encoder tails (models/fusion_layers/early_fusion_vit_cnn.py:87-104, models/vision_transformer/vit_cnn.py:45-57,
 * models/ffl/model_ffl.py:53-96).  The 3x3 convolutions are p3_gemm with P3_A_CONV3X3 / P3_A_CONV3X3_AFFINE_RELU.
 * ------------------------------------------------------------------------------------------ */
/* nn.Upsample(size=(H,W), mode='bilinear', align_corners=False) of the token map: src tokens [B, src_tok_per_img, C] starting at token
 * src_tok_off (1 = CLS dropped) viewed as [h, w] -> NHWC dst [B, H, W, ld] */
int p3_upsample_bilinear(const void* src, int dtype_src, void* dst, int dtype_dst, int B, int h, int w, int C, int H, int W, int ld,
                         int src_tok_off, int src_tok_per_img, void* stream);
/* Conv1x1(256 -> n_out) on relu(x*scale+shift) + Sigmoid (act 0) | post_mul*Tanh (act 1); out NCHW fp32 [B, n_out, H*W]; optionally the
 * first output is also written to copy_dst[r*copy_ld] (the seg channel concatenated to the features, model_ffl.py:87-89) */
int p3_head1x1(const void* X, int ld, int dtype, const float* scale, const float* shift, const float* W, const float* bias, int n_out,
               int act, float post_mul, float* out_nchw, void* copy_dst, int copy_ld, int64_t R, int64_t HW, void* stream);
int p3_nhwc_to_nchw(const void* X, int ld, int dtype, const float* scale, const float* shift, float* out, int B, int C, int64_t HW, void* stream);

/* ---- backward of the FFL / *CNN tail (autograd of models/ffl/model_ffl.py:71-96 and of the *CNN encoders' `proj`) ----
 * p3_head1x1_bwd: through Conv1x1 + Sigmoid | post_mul*Tanh and the BatchNorm + ReLU in front of it.  out_nchw / dout_nchw are the
 *   forward output and its gradient [B, n_out, HW] fp32.  dHd [R,256] = dy*scale (add the batch-statistics term with p3_affine_fix).
 *   acc (zeroed by the caller) += [dscale centred (256) | dshift (256) | dW (n_out*256) | db (n_out)].
 * p3_affine_relu_bwd256: dA = gradient w.r.t. relu(bn(H)) -> dHd = dA*[bn(H) > 0]*scale, acc += [dscale centred | dshift].
 * p3_pad_nhwc: [B*H*W, ld_src] -> zero-bordered [B, H+2, W+2, Cp] image (channels < c_aff through relu(x*scale+shift) when scale is
 *   given) that the shifted-row weight-gradient GEMMs (p3_gemm_tn) read.
 * p3_upsample_bilinear_bwd: adjoint of p3_upsample_bilinear (separable, gather form, deterministic); tmp = fp32 [B, H, w, C]. */
int p3_head1x1_bwd(const void* H, int dtype, const float* scale, const float* shift, const float* mean, const float* W, int n_out,
                   const float* out_nchw, const float* dout_nchw, int act, float post_mul, void* dHd, float* acc, int64_t R, int64_t HW,
                   void* stream);
int p3_affine_relu_bwd256(const void* dA, const void* H, int ldh, int dtype, const float* scale, const float* shift, const float* mean,
                          void* dHd, float* acc, int64_t R, void* stream);
int p3_pad_nhwc(const void* src, int ld_src, int dtype, const float* scale, const float* shift, int c_aff, int C, int Cp, void* dst, int B, int H,
                int W, void* stream);

/* ---- HiSup head set (models/hisup/model_hisup.py:38-64 `ECA`, :122-226 `EncoderDecoder.forward_common` after the encoder).
 * The 3x3 / 1x1 convolutions, BatchNorm statistics and zero-bordered images are p3_gemm (P3_A_CONV3X3 + conv_pad, column sums), p3_bn_finalize
 * and p3_pad_nhwc; these three entries are the rest.  Maps are token-major [B*H*W, ld] in `dtype`, a producer's BatchNorm + ReLU travels as
 * per-channel (scale, shift) and is applied where the map is read.
 * p3_nchw_to_nhwc:    the encoder's NCHW fp32 feature map (what the reference hands to the heads, model_hisup.py:205) -> token-major.
 * p3_eca_gate:        pooled[b,c] = mean_hw(relu(bn(a1)) + relu(bn(a2)))  (ECA.avg_pool(x1 + x2)), gate = sigmoid(conv1d_k(pooled) over c)
 *                     (Conv1d(1, 1, k, padding k/2, no bias), model_hisup.py:47,59-61); k odd.
 * p3_affine_relu_mix: out = f(a) * gate[b, c] + g(b)  with f / g = relu(x*scale + shift) when scale is given, identity otherwise; gate and the
 *                     second source are optional: x2 * y (ECA.forward, :63), feature + attention feature (:217-218), the channel halves of
 *                     torch.cat((features, afm_conv)) (:222). */
int p3_nchw_to_nhwc(const float* X, void* out, int ld, int dtype, int B, int C, int64_t HW, void* stream);
int p3_eca_gate(const void* a1, int ld1, const float* scale1, const float* shift1, const void* a2, int ld2, const float* scale2,
                const float* shift2, const float* conv_w, int k, float* pooled, float* gate, int B, int64_t HW, int C, int dtype, void* stream);
int p3_affine_relu_mix(void* out, int ld_out, const void* a, int ld_a, const float* scale_a, const float* shift_a, const float* gate,
                       const void* b, int ld_b, const float* scale_b, const float* shift_b, int64_t R, int C, int64_t HW, int dtype,
                       void* stream);
int p3_upsample_bilinear_bwd(const void* dUp, int dtype, float* tmp, void* dtok, int B, int h, int w, int C, int H, int W, int tok_off,
                             int tok_per_img, void* stream);


/* ------------------------------------------------------------------------------------------
 * Input pipeline on the device.  The reference augments per sample on CPU workers: albumentations
 * D4(p=1) + Normalize + ToTensorV2 (datasets/build_datasets.py:53-75) and apply_d4_augmentations_to_lidar (datasets/p3_coco.py:115-164).
 * group[b] in 0..7 = albumentations' D4 element of tile b: e, r90, r180, r270, v, hvt, h, t.
 * ------------------------------------------------------------------------------------------ */
/* src u8 [B,H,W,C] (HWC as rasterio/albumentations hold it) -> dst f32 [B,C,H,W] = ToTensorV2(Normalize(D4_g(img))):
 * dst = ((float)px - sub[c]) * mul[c] with the HOST-side constants sub = mean*max_pixel_value, mul = 1/(std*max_pixel_value) (fp32).
 * group may be NULL (no augmentation: validation / prediction). */
int p3_image_prepare(const uint8_t* src, const int32_t* group, float* dst, int B, int H, int W, int C, const float* sub, const float* mul,
                     void* stream);
/* in-place D4 of the jagged point list values [total,3] (x, y, z) / offsets [B+1] around the centre (cx, cy) = (in_width // 2,
 * in_height // 2): subtract centre, swap / negate as p3_coco.py:135-158, add centre - fp32, same operation order */
int p3_points_d4(float* values, const int64_t* offsets, const int32_t* group, int B, int64_t total, float cx, float cy, void* stream);
/* FFL ground truth of a batch (datasets/p3_coco.py:254-296 + apply_augmentations_to_ffl_crossfield_angle :166-205), every input optional:
 * gt_polygons_u8 [B,H,W,3] -> out_gt f32 [B,3,H,W] = clamp(u8 / 255, 0, 1); crossfield_angle_u8 [B,H,W] -> out_angle f32 [B,1,H,W] =
 * ((u8 * pi / 255 + pi/2) % pi) rotated / mirrored with the tile; distances / sizes f32 [B,H,W] -> [B,1,H,W] permuted only.
 * group[b] = the tile's D4 element (NULL: none). */
int p3_ffl_targets_prepare(const uint8_t* gt_polygons_u8, const uint8_t* crossfield_angle_u8, const float* distances, const float* sizes,
                           const int32_t* group, int B, int H, int W, float* out_gt, float* out_angle, float* out_distances, float* out_sizes,
                           void* stream);

/* ------------------------------------------------------------------------------------------
 * FFL frame-field loss, forward + gradients: build_combined_loss / MultiLoss of models/ffl/losses.py:84-141,237-316 with
 * the shipped config/model/ffl.yaml (seg = interior channel only, crossfield on, no freq / dist / size weights, seg.type "bool"):
 *   0 seg (bce_coef * BCE(seg, gt0 > 0.98) + dice_coef * dice(seg, gt0), :318-365)   1 crossfield_align (:368-386)
 *   2 crossfield_align90 (:389-406)   3 crossfield_smooth (:409-419)   4 seg_interior_crossfield (:220-235, :422-444)
 * seg [B,1,H,W], crossfield [B,4,H,W], gt_polygons_image [B,3,H,W] (interior, edge, vertex), gt_crossfield_angle [B,1,H,W]: fp32 NCHW.
 * seg_weights [B,1,H,W] or NULL: the per-pixel BCE weights of compute_seg_loss_weigths (:150-205; all ones in the shipped config).
 * coef[5] (host) = weight_i(epoch) / norm_i.  losses[6] (device) = the five RAW losses and total = sum coef_i * loss_i.
 * dseg / dcrossfield (both or neither): d total / d input.  workspace: p3_ffl_loss_workspace_bytes(B, H, W) bytes of device scratch.
 * ------------------------------------------------------------------------------------------ */
int p3_ffl_loss(const float* seg, const float* crossfield, const float* gt_polygons_image, const float* gt_crossfield_angle,
                const float* seg_weights, int B, int H, int W, const float* coef, float bce_coef, float dice_coef, float* losses, float* dseg,
                float* dcrossfield, void* workspace, void* stream);
int64_t p3_ffl_loss_workspace_bytes(int B, int H, int W);

/* ------------------------------------------------------------------------------------------
 * HiSup attraction field map (the reference's only native kernel: models/hisup/afm_module/afm_op/cuda/afm.cu:29-112,
 * bound as afm(lines, shape_info, height, width) in models/hisup/model_hisup.py:95).
 * lines [L,4] fp32 (x1, y1, x2, y2 in source pixels), shape_info [B,4] int32 = (first line, one past the last line, source height,
 * source width) per tile -> afmap [B,2,height,width] fp32 = -sgn(a) log(|a| / size + 1e-6) of the offset a to the closest segment
 * point, aflabel [B,1,height,width] int32 = index of that segment inside the tile (first of equally close ones); tiles without
 * segments get zeros.
 * ------------------------------------------------------------------------------------------ */
int p3_afm(const float* lines, const int32_t* shape_info, int B, int height, int width, float* afmap, int32_t* aflabel, void* stream);

/* ------------------------------------------------------------------------------------------
 * HiSup inference after the heads (models/hisup/model_hisup.py:229-293 `EncoderDecoder.forward_val`).  Forward only; every output
 * repeats bit for bit from run to run.  A logit map is given as base pointer + (batch, channel, pixel) strides in ELEMENTS, element
 * (b, c, pix) = base[b*sb + c*sc + pix*sp]: NCHW fp32 is (C*H*W, H*W, 1), token-major fp32 rows [B*H*W, ld] are (H*W*ld, 1, ld).
 * H * W <= 2^22.  workspace: p3_*_workspace_bytes(...) bytes of device scratch, contents irrelevant on entry.
 *
 * p3_hisup_junctions - model_hisup.py:251-253,266-268 + models/hisup/polygon.py:8-38 (softmax, max_pool2d NMS, two .item() counts, two
 *   topk, four gathers per image) for the whole batch without host synchronisation.  jloc: 3 classes, joff: 2 channels.
 *   p = softmax(jloc); per class a pixel is a candidate when p equals the maximum of its (border-clipped) 3x3 neighbourhood and p > 0.008;
 *   plateaus survive whole.  The 300 candidates with the highest p are kept in descending order of p; EQUAL p: LOWER FLAT INDEX FIRST
 *   (torch.topk leaves that order open).  Class 2 first, then class 1 (forward_val's argument order into get_pred_junctions):
 *   counts[b] = (n_class2, n_class1), class-1 entries start at juncs[b, n_class2].  x = ((idx % W) + (sigmoid(joff0) - 0.5) + 0.5) * scale_x,
 *   y likewise with idx / W, joff1, scale_y.  juncs fp32 [B,600,2], scores fp32 [B,600] (= p), index int32 [B,600] (flat source pixel),
 *   counts int32 [B,2]; entries past the count are 0 (index: -1).
 *
 * p3_hisup_regions - model_hisup.py:254,265,271 (`remask.softmax(1)[:, 1:]`, skimage `label(mask > 0.5)`, the `regionprops` fields
 *   forward_val and polygon.py:139-142 read).  remask: 2 classes.  mask fp32 [B,H,W] = class-1 probability; labels int32 [B,H,W]:
 *   8-connected components of mask > 0.5 numbered 1..n in raster order of each component's first pixel (the numbering of
 *   skimage.measure.label / scipy.ndimage.label), 0 = background; n_regions int32 [B]; for the first max_regions regions area int32
 *   [B,max_regions], bbox int32 [B,max_regions,4] = (min_row, min_col, max_row + 1, max_col + 1), score fp32 [B,max_regions] = mean of
 *   mask over the region (summed as 32.32 fixed point: order independent).  status int32 [B] = 1 where n_regions > max_regions: labels
 *   and n_regions are still complete, the statistics hold the first max_regions regions, nothing is written past the arrays.
 *
 * p3_hisup_val_loss - model_hisup.py:241-245 with sigmoid_l1_loss (:27-37): NCHW fp32 contiguous logits jloc [B,3,H,W], joff / mask / afm /
 *   remask [B,2,H,W]; targets as AnnotationEncoder (:66-120) makes them: t_jloc int64 [B,1,H,W] in {0,1,2}, t_joff fp32 [B,2,H,W], t_mask fp32
 *   [B,1,H,W] in {0,1}, t_afm fp32 [B,2,H,W].  losses fp32 [5] = loss_jloc (3-class cross-entropy), loss_joff (mean of |sigmoid(joff) - 0.5 -
 *   t_joff| * t / w, t = junction pixel, w = the image's share of junction pixels, 1 where there is none), loss_mask, loss_afm (L1),
 *   loss_remask - un-weighted means.  Workgroup partials are summed in a fixed order in float64.
 * ------------------------------------------------------------------------------------------ */
int p3_hisup_junctions(const float* jloc, int64_t jloc_sb, int64_t jloc_sc, int64_t jloc_sp, const float* joff, int64_t joff_sb,
                       int64_t joff_sc, int64_t joff_sp, int B, int H, int W, float scale_x, float scale_y, float* juncs, float* scores,
                       int32_t* index, int32_t* counts, void* workspace, void* stream);
int64_t p3_hisup_junctions_workspace_bytes(int B, int H, int W);
int p3_hisup_regions(const float* remask, int64_t sb, int64_t sc, int64_t sp, int B, int H, int W, int max_regions, float* mask,
                     int32_t* labels, int32_t* n_regions, int32_t* area, int32_t* bbox, float* score, int32_t* status, void* workspace,
                     void* stream);
int64_t p3_hisup_regions_workspace_bytes(int B, int H, int W, int max_regions);
int p3_hisup_val_loss(const float* jloc, const float* joff, const float* mask, const float* afm, const float* remask, const int64_t* t_jloc,
                      const float* t_joff, const float* t_mask, const float* t_afm, int B, int H, int W, float* losses, void* workspace,
                      void* stream);
int64_t p3_hisup_val_loss_workspace_bytes(int B, int H, int W);

/* ------------------------------------------------------------------------------------------
 * HiSup training losses with their gradients: the five lines of `EncoderDecoder.forward_train` (models/hisup/model_hisup.py:302-306, sigmoid_l1_loss
 * :27-37) weighted as `LossReducer` does (train/trainer_hisup.py:31-39), forward and backward in one call.  The five prediction maps are fp32, each
 * given as base pointer + (batch, channel, pixel) strides in elements as in the block above (NCHW and token-major rows, in any mix): jloc 3 channels,
 * joff / mask / afm / remask 2.  Targets as p3_hisup_val_loss reads them (contiguous): t_jloc int64 [B,1,H,W], t_joff fp32 [B,2,H,W], t_mask fp32
 * [B,1,H,W], t_afm fp32 [B,2,H,W].  weights[5] (host) in the order loss_jloc, loss_joff, loss_mask, loss_afm, loss_remask.
 * losses fp32 [6] (device) = the five un-weighted losses in that order, then total = sum w_k * loss_k.
 * d_jloc .. d_remask: d total / d map, each written with the strides of its prediction from a base pointer of its own; only the map's valid
 * channels of the B * H * W pixels are written (the padding of token-major rows keeps its contents).  All five or none: without them only the
 * values are computed, bit for bit the same values.  With N = B * H * W, pixel p of image b:
 *   jloc, mask, remask (cross-entropy; mask classes = (int64) t_mask):  w_k / N * (softmax(l)_c - [c == t])
 *   afm (L1 over 2N elements):                                            w_afm / 2N * sign(afm - t_afm), sign(0) = 0
 *   joff: on junction pixels (t_jloc in {1, 2})                            w_joff / 2N * (H * W / c_b) * sign(s - 0.5 - t_joff) * s * (1 - s),
 *         s = sigmoid(joff), c_b = junction pixels of image b (the reference's t / w with w == 0 -> 1); zero elsewhere and in an image without junctions.
 * Targets select by comparison only, so any target value is safe: a t_jloc outside {0, 1} is class 2 of the cross-entropy, a truncated t_mask other
 * than 0 is class 1.  No host synchronisation, no floating-point atomics: workgroup partials are summed in one fixed order in float64 and every
 * output repeats bit for bit.  Three launches with gradients (junction count, pixel pass, final sum), two without.  H * W <= 2^22, B <= 65535.
 * workspace: p3_hisup_train_loss_workspace_bytes(B, H, W) bytes of device scratch, contents irrelevant on entry.
 * ------------------------------------------------------------------------------------------ */
int p3_hisup_train_loss(const float* jloc, int64_t jloc_sb, int64_t jloc_sc, int64_t jloc_sp, const float* joff, int64_t joff_sb, int64_t joff_sc,
                        int64_t joff_sp, const float* mask, int64_t mask_sb, int64_t mask_sc, int64_t mask_sp, const float* afm, int64_t afm_sb,
                        int64_t afm_sc, int64_t afm_sp, const float* remask, int64_t remask_sb, int64_t remask_sc, int64_t remask_sp,
                        const int64_t* t_jloc, const float* t_joff, const float* t_mask, const float* t_afm, int B, int H, int W,
                        const float* weights, float* losses, float* d_jloc, float* d_joff, float* d_mask, float* d_afm, float* d_remask,
                        void* workspace, void* stream);
int64_t p3_hisup_train_loss_workspace_bytes(int B, int H, int W);

/* ------------------------------------------------------------------------------------------
 * FFL active-contour (ACM) polygon optimiser: predict/ffl/polygonize_acm.py:77-220 (`PolygonAlignLoss`, `TensorPolyOptimizer`), `steps` plain-SGD
 * iterations of every contour vertex in one call, with the analytic gradient of the reference's loss instead of an autograd graph.
 * pos fp32 [N,2] (row, col), updated in place.  poly_slice int32 [P,2] = [first vertex, one past the last) of each polygon, poly_batch int32 [P] its
 * image, is_endpoint uint8 [N] (a vertex that never moves), indicator fp32 [B,H,W], c0c2 fp32 [B,4,H,W] (c0 re, c0 im, c2 re, c2 im).
 * A polygon p_0..p_{n-1}, open or closed, has the n edges e_i = p_{(i+1) mod n} - p_i (the reference pads every polygon with its first vertex).
 *   edge:    mid = round_half_even((p_i + p_{i+1}) / 2) clamped into the map; norm = |e|, mask = norm < 0.1 ? 0 : 1; z = e / (norm + 1e-3) as re + i im;
 *            align = mask |z^4 + c2(mid) z^2 + c0(mid)|^2, length = (norm mask)^2
 *   vertex:  level = (bilinear(indicator, p) - data_level)^2, weights from the unclamped floor, the four fetches clamped
 *   total = (data_coef sum level + length_coef sum length + crossfield_coef sum align) / (data_coef + length_coef + crossfield_coef)
 *   round, floor, the clamps and the mask are constants of the gradient; d norm / d e = 0 at norm = 0, so a masked edge contributes exactly 0.
 *   p <- p - lr_i grad for every vertex that is no endpoint, lr_i = poly_lr * (i < warmup_iters ? 1 + (warmup_factor - 1)(warmup_iters - i) / warmup_iters : 1),
 *   i = first_iter .. first_iter + steps - 1 (evaluated in double, as torch's LambdaLR does).
 * Polygons of up to 4096 vertices run all steps in ONE launch, one workgroup each, positions in LDS; longer ones (or all, force_fallback != 0) take one
 * launch per step over `workspace`.  Both paths, any split of the steps into calls, any polygon order and any two runs give the same bits; no atomics, no
 * host synchronisation.  max_len: an upper bound of the vertices of one polygon that the HOST knows (sizes the LDS and decides whether the fallback is
 * launched at all; a longer polygon is left as it is), <= 0: unknown, both paths are launched.  poly_losses (NULL or fp32 [P,3]): each polygon's
 * (align, level, length) sums of the LAST executed step, evaluated before its update.  workspace: p3_acm_workspace_bytes(N) bytes, needed (non-NULL)
 * only when the fallback can run.  P == 0, N == 0 or steps == 0: returns 0 without a launch.
 * ------------------------------------------------------------------------------------------ */
int p3_acm_optimize(float* pos, int64_t N, const int32_t* poly_slice, const int32_t* poly_batch, int P, const uint8_t* is_endpoint,
                    const float* indicator, const float* c0c2, int B, int H, int W, float data_coef, float length_coef, float crossfield_coef,
                    float data_level, double poly_lr, int warmup_iters, double warmup_factor, int first_iter, int steps, int max_len,
                    int force_fallback, float* poly_losses, void* workspace, void* stream);
int64_t p3_acm_workspace_bytes(int64_t N);

/* ------------------------------------------------------------------------------------------
 * FFL active-skeleton (ASM) optimiser: predict/ffl/polygonize_asm.py:133-421 (`AlignLoss`, `TensorSkeletonOptimizer`) over the containers of
 * torch_lydorn/torchvision/transforms/tensorskeleton.py, `steps` RMSprop iterations of every skeleton node in one call, with the analytic gradient
 * of the reference's total_loss instead of an autograd graph.  Line 353 keeps three terms in the loss that is differentiated,
 *     total_loss = data_coef * level_loss + length_coef * total_length_loss + crossfield_coef * total_align_loss,
 * so the positions depend on level, length and align alone; the curvature, corner and junction terms (reported, never differentiated) are not built.
 *
 * Containers (tensorskeleton.py:44-68): pos [N,2] (row, col) fp32, degrees [N], path_index [M] node ids, path_delim [P+1] delimiting paths inside
 * path_index, batch [N] each node's image.  A junction node appears in path_index once per incident path end; a closed contour repeats its first
 * node id as its last entry.  k is a position in path_index; "path start" / "path end" come from path_delim.
 *
 * Terms of one step (polygonize_asm.py:177-235):
 *   level   (:205-216) every node, on a path or not: (bilinear(indicator, pos) - data_level)^2, the interpolation of functionnal.py:4-42 (weights from
 *           the unclamped floor, fetches clamped).
 *   align   (:179-202) every edge (k, k+1), k no path end: t = p[k+1] - p[k], mask 0 where |t| < 0.1, z = t / (|t| + 1e-6), c0 and c2 read at the
 *           rounded (half to even), clamped midpoint; the term is |z^4 + c2 z^2 + c0|^2 * mask and its gradient flows to both end nodes (torch.norm's
 *           subgradient at 0 is 0).  The maps are read in the image of the node that evaluates the edge: a path lies in one image.
 *   length  (:219-235) every k that is neither a path start nor a path end: |p[k] - p[k-1]|^2 + |p[k+1] - p[k]|^2 with both neighbours detached, so the
 *           gradient 2 (p[k] - p[k-1]) - 2 (p[k+1] - p[k]) goes to node path_index[k] only.
 *   Nothing is divided by a coefficient sum.
 * Schedules (:151-156, 342-344, 380-381, 411-412), evaluated in double and rounded to float: the three coefficients at integer iteration i are
 * scipy interp1d's linear form over `knots` (slope = (y_hi - y_lo) / (x_hi - x_lo); y = slope * (i - x_lo) + y_lo on the segment x_lo <= i < x_hi
 * that numpy.interp, to which scipy hands 1-d tables, picks: a knot gives its own value; beyond the last knot the last segment is extended); lr_i = lr * gamma^i by repeated multiplication, as ExponentialLR chains it.
 * Update (:380, 404-409): torch.optim.RMSprop(alpha = 0.9, eps = 1e-8, no momentum, not centred): sq = 0.9 sq + 0.1 g^2,
 * pos -= lr_i * g / (sqrt(sq) + eps).  A node with is_tip (degree 1) keeps its position; its sq is still updated.
 *
 * The work unit is a connected component of the skeleton graph, described by a plan built once per skeleton, on the host or by p3_asm_plan below (csrc/asm.hip explains it):
 * comp_ptr int32 [C+1] delimits components inside cn_node int32 [CN] (node ids; an entry's index inside its component is its local index);
 * cn_occ int32 [CN+1] delimits each entry's occurrences, ascending in k, inside slot_nb int32 [S,2] = local index of the node at k-1 (-1 at a path
 * start) and at k+1 (-1 at a path end).  is_tip uint8 [N], node_batch int32 [N].  Every index is clamped on the device.
 * Components of at most 4096 nodes run all steps in ONE launch (positions in LDS, one barrier per step); larger ones, or all with force_fallback,
 * take one launch per step over `workspace` (p3_asm_workspace_bytes(N, CN), needed only then).  Both paths, any split of the steps into calls
 * (first_iter, sq carried) and any two runs give the same bits; no atomics, no host synchronisation.  max_comp: an upper bound of the nodes of one
 * component that the HOST knows, <= 0: unknown.  knots: HOST double [4, nk] = step_thresholds, data, length, crossfield (2 <= nk <= 8).
 * pos and sq fp32 [N,2] are updated in place (sq zeros on a first call).  grad_out (NULL or fp32 [N,2]): the gradient of the LAST executed step.
 * comp_losses (NULL or fp32 [C,3]): each component's (align, level, length) sums of the last executed step before its update, each edge counted
 * once by its tail.  C == 0, N == 0, CN == 0 or steps == 0: returns 0 without a launch.
 * p3_asm_schedule (host only): out[4] = (data, length, crossfield, lr) of iteration `iter`, the floats the kernel uses, from the same functions.
 * ------------------------------------------------------------------------------------------ */
int p3_asm_optimize(float* pos, float* sq, int64_t N, const int32_t* comp_ptr, int C, const int32_t* cn_node, const int32_t* cn_occ, int64_t CN,
                    const int32_t* slot_nb, int64_t S, const uint8_t* is_tip, const int32_t* node_batch, const float* indicator, const float* c0c2,
                    int B, int H, int W, float data_level, const double* knots, int nk, double lr, double gamma, int first_iter, int steps,
                    int max_comp, int force_fallback, float* grad_out, float* comp_losses, void* workspace, void* stream);
int64_t p3_asm_workspace_bytes(int64_t N, int64_t CN);
int p3_asm_schedule(int iter, const double* knots, int nk, double lr, double gamma, double* out);

/* ------------------------------------------------------------------------------------------
 * FFL initial contours: predict/ffl/polygonize_utils.py:15-44 (`compute_init_contours_batch`, i.e. skimage.measure.find_contours(indicator, level,
 * fully_connected='low', positive_orientation='high') per image) on the device, with the contour container of p3_acm_optimize as its output.
 * indicator fp32 [B,H,W] read through element strides (stride_b, stride_r, stride_c: channel 0 of a [B,C,H,W] map needs no copy); level is a double.
 *   cell (r, c), 0 <= r < H-1, 0 <= c < W-1, corners ul = I[r,c], ur = I[r,c+1], ll = I[r+1,c], lr = I[r+1,c+1] taken as double; a NaN corner: nothing;
 *   case = (ul > level) + 2 (ur > level) + 4 (ll > level) + 8 (lr > level); with f(a, b) = (level - a) / (b - a) in double (0 if a == b) the crossing
 *   points are T = (r, c + f(ul, ur)), B = (r+1, c + f(ll, lr)), L = (r + f(ul, ll), c), R = (r + f(ur, lr), c+1), rounded to fp32 once;
 *   segments from -> to in slot order: 1 T-L | 2 R-T | 3 R-L | 4 L-B | 5 T-B | 6 R-T, L-B | 7 R-B | 8 B-R | 9 T-L, B-R | 10 B-T | 11 B-L | 12 L-R |
 *   13 T-R | 14 L-T; key of a segment = 2 (r (W-1) + c) + slot.
 *   A vertex is a crossed grid edge; linking is by edge identity, never by coordinates; the successor of a segment's `to` vertex is its `from` vertex.
 *   A contour with a vertex that is the `from` of no segment is open and starts there; any other is closed, starts at the `to` vertex of its
 *   largest-key segment and does not repeat its first point.  Contours are ordered by image, then by their smallest segment key.
 * Outputs: pos fp32 [max_vertices,2] (row, col); poly_slice int64 [max_contours,2] = [first vertex, one past the last); poly_batch int32 [max_contours];
 * batch int64 [max_vertices] the image of each vertex; is_endpoint uint8 [max_vertices] = 1 on both ends of an open contour; counts int32 [3] =
 * (N vertices, P contours, vertices of the longest contour); n_contours, n_vertices int32 [B]; status int32 [1] = 1 when N > max_vertices or
 * P > max_contours: counts still hold the true totals and nothing is written past the capacities (B (H (W-1) + (H-1) W) vertices and half as many
 * contours can never overflow).  H < 2 or W < 2: no contour.
 * No atomics and one writer per element: two runs give the same bits, an image alone gives the contours it gives inside a batch.  No host
 * synchronisation; the number of launches depends on B, H, W only.  workspace: p3_init_contours_workspace_bytes(B, H, W) bytes.
 * ------------------------------------------------------------------------------------------ */
int p3_init_contours(const float* indicator, int64_t stride_b, int64_t stride_r, int64_t stride_c, int B, int H, int W, double level,
                     int max_vertices, int max_contours, float* pos, int64_t* poly_slice, int32_t* poly_batch, int64_t* batch, uint8_t* is_endpoint,
                     int32_t* counts, int32_t* n_contours, int32_t* n_vertices, int32_t* status, void* workspace, void* stream);
int64_t p3_init_contours_workspace_bytes(int B, int H, int W);

/* ------------------------------------------------------------------------------------------
 * FFL corner-aware contour simplification: the array half of `post_process` (predict/ffl/polygonize_acm.py:277-284 and polygonize_asm.py:498-504:
 * skimage.measure.approximate_polygon, frame_field_utils.detect_corners :71-114 over math_utils.compute_crossfield_uv, polygonize_utils.split_polylines_corner
 * :47-61, LineString.simplify per piece) on the device.  The planar-graph half (unary_union, polygonize_full, the area / probability filters) is p3_ffl_polygons below.
 * Polyline i is the EXPLICIT point sequence q_0 .. q_{n-1} = pos[index[slice[i,0] .. slice[i,1])] (pos[slice ...] when index is NULL), the first point
 * appended once more when closed[i] is set; coordinates are (row, col).  A polyline with fewer than 2 explicit points gives no piece.
 *   DP(points, tol): Douglas-Peucker.  The first and last point are kept; in a section (s, e) the distance of point k is |cross(q_k - q_s, d)| / |d| with
 *      d = q_e - q_s when (q_k - q_s).d > 0 and (q_e - q_k).d > 0, else min(|q_k - q_s|, |q_k - q_e|); if any distance is > tol the point with the largest
 *      one, the lowest index among equal maxima, is kept and both halves are searched, otherwise the interior is dropped.  tol <= 0 keeps every point.
 *   A  tol_pre > 0: the polyline becomes DP(explicit points, tol_pre)  (ACM: min(1, tolerance); ASM: 0).
 *   B  corner mask (detect_corners).  Closed (max |q_0 - q_last| < 1e-6): vertex i < last has the left edge predecessor - q_i (the predecessor of vertex 0 is
 *      the second-to-last point) and the right edge q_{i+1} - q_i, mask[last] = mask[0].  Open: both ends are corners, interior vertices use q_{i-1} - q_i and
 *      q_{i+1} - q_i.  At the vertex's pixel (round half to even, clipped into the map) c0 = c0c2[0] + i c0c2[1], c2 = c0c2[2] + i c0c2[3],
 *      s = sqrt(c2^2 - 4 c0), u = sqrt((c2 + s) / 2), v = sqrt((c2 - s) / 2) (principal roots, computed at the vertices only);
 *      score(e, w) = |e_row Re w + e_col Im w|, is_u(e) = score(e, v) < score(e, u), corner = is_u(left) != is_u(right).
 *   C  pieces (split_polylines_corner): without a corner the polyline is one piece; else one piece per pair of consecutive corners, both included, and, when
 *      neither mask[0] nor mask[last] is set, the merged piece polyline[last corner:] + polyline[:first corner + 1] last.
 *   D  tol > 0: every piece becomes DP(piece, tol).
 * Distances and the frame field are evaluated in double.  Outputs, polylines in input order and pieces in the order of C: out_pos fp32 [max_vertices,2] (bit
 * copies of input positions), out_src int32 [max_vertices] (the point's position inside its explicit polyline), piece_slice int64 [max_pieces,2] = [first,
 * one past the last) inside out_pos, piece_poly / piece_batch int32 [max_pieces]; stage_flags (NULL or uint8 [E], E = (index ? K : N) + P, the polylines'
 * explicit points one after the other): bit 0 kept by A, bit 1 corner, bit 2 kept by D in some piece; counts int32 [3] = (vertices, pieces, longest piece);
 * status int32 [1]: bit 0 = more vertices than max_vertices or more pieces than max_pieces (counts still hold the true totals and nothing is written past
 * the capacities; 2 E' vertices and E' pieces for E' explicit points can never overflow), bit 1 = overlapping slices hold more than E explicit points (the
 * polylines past E give no piece).  Every index read from index / slice / poly_batch is clamped.
 * Polylines of up to 4096 explicit points run in one workgroup each with all working arrays in LDS; longer ones (or all, force_fallback != 0) run the same
 * device functions over `workspace`.  max_len: an upper bound of slice[i,1] - slice[i,0] that the HOST knows (decides whether the second form is launched
 * at all; a longer polyline gives no piece), <= 0: unknown.  Two runs, either form, a polyline alone or inside a batch give the same bits; no host
 * synchronisation.  workspace: p3_corner_split_workspace_bytes(E, P) bytes.  P == 0, N == 0 or an empty index: zero counts without a kernel launch.
 * ------------------------------------------------------------------------------------------ */
int p3_corner_split(const float* pos, int64_t N, const int64_t* index, int64_t K, const int64_t* slice, const uint8_t* closed, const int32_t* poly_batch,
                    int P, const float* c0c2, int B, int H, int W, double tol_pre, double tol, int max_len, int force_fallback, int max_vertices,
                    int max_pieces, float* out_pos, int32_t* out_src, int64_t* piece_slice, int32_t* piece_poly, int32_t* piece_batch,
                    uint8_t* stage_flags, int32_t* counts, int32_t* status, void* workspace, void* stream);
int64_t p3_corner_split_workspace_bytes(int64_t E, int P);

/* ------------------------------------------------------------------------------------------
 * FFL active-skeleton initialisation from marching squares: the conversion half of get_marching_squares_skeleton (predict/ffl/polygonize_asm.py:581-638)
 * and tensorskeleton.py:87-159 on the device, behind p3_init_contours (csrc/skeleton_init.hip).
 * Input, the contour container exactly as p3_init_contours leaves it: pos fp32 [N,2], poly_slice int64 [P,2], poly_batch int32 [P], is_endpoint uint8 [N]; a
 * closed contour does not repeat its first point, an open one has is_endpoint = 1 on both ends; contours ordered by image.  Every slice and image is clamped.
 * A contour of n stored points is CLOSED when its first point is no endpoint.  The reference tests max|c[0] - c[-1]| < 1e-6 on skimage's points instead; the
 * two agree whenever no pixel equals the level (an open contour's two ends lie on different border edges, which can only share a point at a grid vertex whose
 * value is the level).  filter != 0 keeps a contour when vertices >= 3 - a closed contour counts its repeated point: n + 1 - and
 * min_area < |sum_i x_i y_(i+1) - y_i x_(i+1)| / 2 (cyclic over the n points, evaluated in double from the fp32 positions; the order of the sum is fixed per
 * build but not that of numpy: a contour within rounding of min_area may be decided differently).  filter == 0 keeps every contour with a point (min_area=None).
 * Output, kept contours in container order, nodes numbered in that order (the fields of skeletons_to_tensorskeleton([contours_to_skeleton(c_b, min_area)])):
 * out_pos fp32 [max_nodes,2] (bit copies); degrees int64 [max_nodes] = 2, and 1 on the two ends of an open contour; path_index int64 [max_slots]: a path's
 * node ids, a closed one's first id once more; path_delim int64 [max_paths+1], entry P' = M'; batch int64 [max_nodes]; batch_delim int64 [B+1] = kept paths
 * in front of each image; counts int32 [4] = (N' nodes, M' slots, P' paths, nodes of the longest kept path); status int32 [1] bit 0 = a capacity was too
 * small: counts hold the true totals and nothing is written past a capacity.  N nodes, N + P slots and P paths can never overflow.
 * One writer per element, no atomics: two runs give the same bits and an image alone gives the rows it gives inside a batch.  Three launches and one memset
 * whatever the data, no host synchronisation.  P == 0 or N == 0: zero counts and batch_delim, nothing else is touched.
 * workspace: p3_skeleton_from_contours_workspace_bytes(P) bytes.
 *
 * p3_asm_plan: the plan of p3_asm_optimize (above) from path_index int64 [M] and path_delim int64 [D] (D = paths + 1, or 0) for N nodes, entry for entry
 * what polygonize_asm.AsmPlan builds on the host.  Path boundaries are the INTERIOR entries path_delim[1 .. D-2] that lie in 1 .. M-1 (the first path starts
 * at 0, the last ends at M, a repeated delimiter is an empty path and changes nothing); an edge is (k, k+1) for every k that is no path end; components are
 * ordered by their smallest node id and list their nodes in ascending id; a node on no path is a component of its own.  Outputs, all int32: comp_ptr [N+1]
 * (C + 1 entries used), cn_node [N], cn_occ [N+1], slot_nb [M,2] = local index of the node at k-1 and k+1, -1 at a path start / end, node_local [N],
 * slot_k [M] (a node's slots ascending in k); counts [2] = (C, nodes of the largest component); status [1]: bit 1 = a node id outside [0, N) (it is
 * clamped before any use as an index; the outputs are then no plan).  No float arithmetic; integer atomics only where their order cannot show (minimum,
 * maximum, or); two runs give the same bits.  The component search (labels over PATHS, lowered along shared nodes until a round changes nothing) has no
 * round cap: labels never rise and every round but the last lowers one (csrc/skeleton_init.hip).  It runs inside one launch, so the number of launches
 * depends on N and M only; no host synchronisation.  N == 0: C = 0, comp_ptr[0] = cn_occ[0] = 0 (status bit 1 when M > 0).
 * workspace: p3_asm_plan_workspace_bytes(N, M) bytes.
 * ------------------------------------------------------------------------------------------ */
int p3_skeleton_from_contours(const float* pos, int64_t N, const int64_t* poly_slice, const int32_t* poly_batch, const uint8_t* is_endpoint, int P, int B,
                              int filter, double min_area, int max_nodes, int max_slots, int max_paths, float* out_pos, int64_t* degrees,
                              int64_t* path_index, int64_t* path_delim, int64_t* batch, int64_t* batch_delim, int32_t* counts, int32_t* status,
                              void* workspace, void* stream);
int64_t p3_skeleton_from_contours_workspace_bytes(int P);
int p3_asm_plan(const int64_t* path_index, int64_t M, const int64_t* path_delim, int64_t D, int64_t N, int32_t* comp_ptr, int32_t* cn_node, int32_t* cn_occ,
                int32_t* slot_nb, int32_t* node_local, int32_t* slot_k, int32_t* counts, int32_t* status, void* workspace, void* stream);
int64_t p3_asm_plan_workspace_bytes(int64_t N, int64_t M);

/* ------------------------------------------------------------------------------------------
 * FFL active-skeleton initialisation from the segmentation map: init_method "skeleton_device" (csrc/skeleton_thin.hip).  The reference's
 * init_method "skeleton" (predict/ffl/polygonize_asm.py:655-675 compute_skeletons, then skimage binary_closing, skimage skeletonize and skan.Skeleton) restated
 * with a written definition; it is NOT those libraries bit for bit (Zhang-Suen instead of skimage's table, the diagonal rule instead of skan's junctions).
 * Input: seg fp32, image b at seg + b stride_b, channel c at + c stride_c (strides in elements), each channel H x W with contiguous rows.  Channel 0 is the
 * interior probability, channel 1, read only when C >= 2, the edge probability.  level is rounded to fp32 (as torch compares a Python number with an fp32 map).
 *   1 Edge mask.  m = (level < seg[0]) as fp32.  gx, gy = the 3 x 3 Sobel responses of m, replicate padding, divided by 8 (kornia's normalised kernel).
 *     g = sqrt((2 gx)^2 + (2 gy)^2) in fp32; with C >= 2, g = clamp(seg[1] + g, 0, 1).  edge = (level < g).  Both comparisons are strict.  2 gx and 2 gy are
 *     multiples of 1/4, the sum of squares is exact, the root is correctly rounded, nothing is contracted: the mask is torch's on the CPU bit for bit.
 *   2 Pad by 2 on every side, edge replication: the working image is (H+4) x (W+4).
 *   3 Closing: dilation, then erosion, by the 3 x 3 cross.  Outside the working image is background for the dilation, foreground for the erosion
 *     (scipy.ndimage.binary_dilation(border_value=0), binary_erosion(border_value=1), what skimage's binary_closing does).
 *   4 Thinning: Zhang-Suen on the working image, outside = background.  P2 .. P9 = N, NE, E, SE, S, SW, W, NW; B = their sum; A = the 0 -> 1 steps in the cyclic
 *     sequence P2, P3, ..., P9, P2.  Sub-iteration 1 deletes a foreground pixel when 2 <= B <= 6, A == 1, P2 P4 P6 == 0 and P4 P6 P8 == 0; sub-iteration 2 when
 *     2 <= B <= 6, A == 1, P2 P4 P8 == 0 and P2 P6 P8 == 0.  A sub-iteration decides every pixel from the image as it stood when it began.  A round is 1 then
 *     2; rounds repeat until one deletes nothing.  No round cap: every round but the last deletes a pixel, at most (foreground + 1) rounds.
 *   5 Crop the pad: the skeleton image is H x W.
 *   6 Graph.  Two skeleton pixels are linked when they are 4-neighbours, or diagonal neighbours with neither of the two pixels 4-adjacent to both a skeleton
 *     pixel (no triangles at staircase corners; nothing is disconnected, the two 4-links through the shared pixel remain).  degree = links of a pixel (at most
 *     4).  A pixel without a link is no node.  Nodes are numbered in raster order (row, then column), image after image.  pos = (row, col) as fp32.
 *   7 Paths.  A path is a maximal chain of links whose interior nodes all have degree 2; its two ends have degree != 2; a loop from a junction back to it is
 *     [u, ..., u].  Of a chain's two directed readings the one with the lexicographically smaller (first node, second node) is kept.  A connected set of
 *     degree-2 nodes without an end is a cycle: it starts at its smallest node, goes to the smaller of that node's two neighbours first, and repeats the
 *     first id at its end.  Paths are ordered by (first node, second node), ascending; node ids are image-major, so paths are too.
 * Output, the fields of p3_skeleton_from_contours: out_pos fp32 [max_nodes,2]; degrees int64 [max_nodes]; path_index int64 [max_slots]; path_delim int64
 * [max_paths+1], entry P = M; batch int64 [max_nodes]; batch_delim int64 [B+1] = the paths in front of each image; counts int32 [4] = (N nodes, M slots,
 * P paths, nodes of the longest path, a repeated end counted once); status int32 [1] bit 0 = a capacity was too small: counts hold the true totals and
 * nothing is written past a capacity.
 * Capacities that can never overflow: N <= B H W.  A node has at most 4 links (a diagonal link needs both 4-neighbours beside it empty), so there are at
 * most 2 N links; every link lies on exactly one path and a path has one slot more than links: P <= links <= 2 N and M = links + P <= 4 N.
 *   max_nodes = B H W, max_paths = 2 B H W, max_slots = 4 B H W.
 * Size limit: H + 4 <= 512 and W + 4 <= 512 (one workgroup per image keeps two bit planes of the working image in 64 KB of LDS); a larger image, C < 1 or a
 * negative capacity is P3_ESHAPE before any launch.  Three launches whatever the data, no memset, no host synchronisation.  One writer per output element;
 * the one atomic is an or in LDS and no workspace word is written by two workgroups: two runs give the same bits, an image alone gives the rows it gives inside a batch, re-based.
 * B == 0 or a batch without a skeleton pixel: zero counts, status and batch_delim, nothing else is touched.
 * workspace: p3_skeleton_from_seg_workspace_bytes(B, H, W) bytes (0 for B <= 0).
 * ------------------------------------------------------------------------------------------ */
int p3_skeleton_from_seg(const float* seg, int B, int C, int H, int W, int64_t stride_b, int64_t stride_c, double level, int max_nodes, int max_slots,
                         int max_paths, float* out_pos, int64_t* degrees, int64_t* path_index, int64_t* path_delim, int64_t* batch, int64_t* batch_delim,
                         int32_t* counts, int32_t* status, void* workspace, void* stream);
int64_t p3_skeleton_from_seg_workspace_bytes(int B, int H, int W);

/* ------------------------------------------------------------------------------------------
 * HiSup polygons: models/hisup/polygon.py:56-93,111-169 (`ext_c_to_poly_coco`, `diagonal_to_square`, `simple_polygon`, `get_poly_crowdai` with
 * test_inria = False) on the device: the OUTER polygon of every region of p3_hisup_regions, what `forward_val` returns as `polys_pred`.
 * Inputs as the two kernels above write them: labels int32 [B,H,W], n_regions int32 [B], bbox int32 [B,max_regions,4], juncs fp32 [B,600,2] (x, y),
 * junc_counts int32 [B,2]; an image has n = min(600, counts[b,0] + counts[b,1]) junctions.  Every count and box read is clamped.  H, W <= 32766.
 * Region (b, l), l <= min(n_regions[b], max_regions), pixel set M, coordinates (x, y) = (column, row):
 *   A  F = M and every background pixel that no 4-connected background path joins to the outside of the bounding box; hole_pixels = |F| - |M|.
 *   B  corner grid T [(H+1),(W+1)]: T[y,x] = F[y,x] | F[y-1,x] | F[y,x-1] | F[y-1,x-1], pixels outside the image are 0.
 *   C  outer border of T, 8-connected border following.  Directions s = 0 E (+x), 1 NE (+x,-y), 2 N, 3 NW, 4 W, 5 SW, 6 S, 7 SE.  p0 = first set cell in
 *      raster order; from s = 4, s = (s - 1) mod 8 until the neighbour p1 of p0 in direction s is set.  p = p0; repeat: s = (s + 1) mod 8 until the
 *      neighbour q of p in direction s is set; emit p; stop when q == p0 and p == p1; else p = q, s = (s + 4) mod 8.
 *   D  after every emitted p whose step to its cyclic successor is diagonal one point is inserted: (+1,+1): (p.x+1, p.y), (-1,-1): (p.x-1, p.y),
 *      (+1,-1): (p.x, p.y-1), (-1,+1): (p.x, p.y+1).  The ring r_0 .. r_{m-1} has unit axis steps only.
 *   E  (n > 0) every ring point takes d_j = sqrt(dx dx + dy dy) in float64 (correctly rounded products, sum and root, no fused multiply-add) to every
 *      junction; j* = the lowest index among the minima; the point votes for j* when d_j* < 5; first[j] = the smallest ring index that votes for j.
 *      More than two junctions with a vote: the polygon is those junctions in ascending `first` (flag bit 0); otherwise it is the ring.
 *   F  of the sequence q_0 .. q_{k-1}: e_i = q_{(i+1) mod k} - q_i, a_i = atan2(e.y, e.x) 180 / pi in float64, t_i = |a_i - a_{(i+1) mod k}|; vertex
 *      (i+1) mod k is kept when 10 < t_i < 350; output = the kept vertices in ascending index, then the first kept one once more.  Nothing kept: the
 *      region gives no polygon (flag bit 2; the reference raises there).
 * p3_hisup_polygons: inner rings are NOT built: a region with holes gets its outer polygon, flag bit 1 and hole_pixels; p3_hisup_polygons_rings (below)
 * builds them in the same call.
 * Outputs, polygons packed in the order (image, label): pos fp32 [max_vertices,2] (x, y; ring corners are integers, junctions bit copies of juncs); src
 * int32 [max_vertices] the ring index or junction index of each vertex; poly_slice int64 [B,max_regions,2] = [first, one past the last) in pos (empty
 * for a region without polygon and for labels past n_regions); poly_flags int32 [B,max_regions] bit 0 junction polygon, bit 1 hole_pixels > 0, bit 2 no
 * polygon; hole_pixels int32 [B,max_regions]; n_vertices int32 [B]; counts int32 [2] = (vertices, vertices of the longest polygon); status int32 [1]:
 * bit 0 = more vertices than max_vertices: counts, poly_slice, flags, hole_pixels and n_vertices still hold the true values, pos and src are left
 * untouched and nothing is written past a capacity; bit 1 = a ring was longer than the bound below (never seen; that region gives no polygon); bit 2 = the run was cut short by the measurement
 * switch P3_HISUP_POLY_STOP of tools/bench_hisup_polygons.py and its outputs are no result.
 * Ring bound: every visit of the border follower to a cell uses up a side of that cell that faces the outer background, so it emits at most c(T) cells,
 * c = the number of such sides; a diagonal step adds one point: m <= 2 c(T).  Dilating by the 2 x 2 block adds at most 4 sides, and a pixel side
 * belongs to one region only, so m <= 2 (c(M) + 4) <= 2 (H (W+1) + W (H+1)) + 8 for one region, and the regions of an image together have at most
 * 2 (H (W+1) + W (H+1)) + 8 n_regions ring points.  A polygon has at most m + 1 vertices (junctions with a vote have distinct `first`), so
 * max_vertices = B (2 (H (W+1) + W (H+1)) + 9 min(max_regions, ceil(H/2) ceil(W/2))) can never overflow.
 * Execution: a region whose padded box (h + 3) (w + 3) has at most 16384 cells and whose ring has at most 5120 points runs with its bitmaps and ring in
 * LDS, one workgroup per region; the others (all of them with force_fallback != 0) run the same device function over slabs of `workspace`.  Four launches
 * whatever the data; no host synchronisation; two runs, either form, an image alone or inside a batch give the same bits.  B == 0 or max_regions == 0:
 * returns 0 without a launch.  workspace: p3_hisup_polygons_workspace_bytes(B, H, W, max_regions, max_vertices) bytes.
 * ------------------------------------------------------------------------------------------ */
int p3_hisup_polygons(const int32_t* labels, const int32_t* n_regions, const int32_t* bbox, const float* juncs, const int32_t* junc_counts, int B,
                      int H, int W, int max_regions, int max_vertices, int force_fallback, float* pos, int32_t* src, int64_t* poly_slice,
                      int32_t* poly_flags, int32_t* hole_pixels, int32_t* n_vertices, int32_t* counts, int32_t* status, void* workspace,
                      void* stream);
int64_t p3_hisup_polygons_workspace_bytes(int B, int H, int W, int max_regions, int max_vertices);

/* ------------------------------------------------------------------------------------------
 * HiSup polygons with their inner rings: the hole branch of `get_poly_crowdai` (models/hisup/polygon.py:95-109,152-154, `inn_c_to_poly_coco`) next to
 * the outer polygons.  p3_hisup_polygons_rings takes the inputs of p3_hisup_polygons, writes its eight outputs with the same bits, and in the same call
 * the ring of every hole of every region whose border encloses an area of at least 50.  Steps A to F are those above; for region (b, l) with pixel set M
 * (everything else, other labels included, is background):
 *   G  a hole is a 4-connected component of the background that step A leaves unfilled.  The holes of a region are numbered in raster order of their
 *      first cell (x_h, y_h).  OpenCV's own order of sibling contours is NOT reproduced: this is the one deviation from the reference's output.
 *   H  the hole border: the follower of step C on M (not on T) from p0 = (x_h - 1, y_h), a region pixel, with the start direction s = 0 in place of 4
 *      (s = (s - 1) mod 8 until the neighbour p1 is set); the loop and the stop condition are unchanged.  This is Suzuki and Abe's hole border for
 *      8-connected foreground, it cuts corners diagonally.  a2 = |sum (x_i y_{i+1} - x_{i+1} y_i)| over the cyclic border; the hole gives a ring iff
 *      a2 >= 100 (area >= 50), decided in integers.  A 6 x 7 rectangular hole has area 54, 6 x 6 has 47, 3 x 3 has 14.
 *   I  K = the border's cells and every cell that no 4-connected path avoiding them joins to the outside of the box (the flood of step A; it stands for
 *      drawContours(thickness = -1)).  K' = K without the cells of its lowest row index and of its lowest column index.  K' holds the whole hole and
 *      otherwise border pixels 8-adjacent to it, so it is one 8-connected component.  The ring: the outer border of K' by step C as it stands (first set
 *      cell, s = 4), the point sequence REVERSED, then step D on the reversed cyclic sequence.  No corner grid: the coordinates are K''s pixel coordinates.
 *   E and F as above on that ring.  A ring in which nothing is kept gets ring flag bit 2 and no vertices.
 * Further arguments: max_rings, max_ring_vertices.  Further outputs, rings in (image, label, hole) order: ring_pos fp32 [max_ring_vertices,2] and ring_src
 * int32 [max_ring_vertices], closed rings as pos / src; ring_slice int64 [max_rings,2] = [first, one past the last) in ring_pos; ring_region int32
 * [max_rings] = b max_regions + l - 1; ring_flags int32 [max_rings] bit 0 junction ring, bit 2 nothing kept; ring_area2 int32 [max_rings] the a2 of step
 * H; region_rings int32 [B,max_regions,2] = [first, one past the last) ring of the region; n_holes int32 [B,max_regions] all holes, kept or not;
 * ring_counts int32 [3] = (rings, ring vertices, vertices of the longest ring).  status, further bits: bit 3 = more rings than max_rings: region_rings,
 * n_holes and ring_counts hold the true values, no other ring output is written; bit 4 = more ring vertices than max_ring_vertices: all of them hold the
 * true values, ring_pos and ring_src are left untouched.  Nothing is written past a capacity.  Bit 1 covers an inner ring past the bound as well.
 * Ring bound: the kept rings of an image number at most floor(H W / 50), because the border polygons of distinct holes have disjoint interiors of area
 * >= 50 each.  A ring has m <= 2 c(K') points as above, c = the sides of K' that face the outside.  Cutting the first row (column) takes away the upper
 * (left) sides of its cells and lays open at most as many below (right of) them: c(K') <= c(K).  K is the hole grown by its 4-neighbours and filled, and
 * its outline is the hole's outer outline moved outwards by one pixel: every side of the hole has one parallel side of K, a convex corner adds two sides,
 * a concave one takes two away, and a rectilinear outline has four more convex corners than concave ones; where the moved outline meets itself sides
 * only drop out.  So c(K) <= p + 8 with p the sides between the hole and M, and m <= 2 p + 16.  A pixel side lies between one region and one hole, and
 * no side on the image border faces a hole, so the p of an image add up to at most H (W-1) + W (H-1), and one ring stays below the single-region bound
 * 2 (H (W+1) + W (H+1)) + 8 the workspace slabs are sized for.  A ring has at most m + 1 vertices:
 * max_rings = max(1, B floor(H W / 50)) and max_ring_vertices = B (2 (H (W-1) + W (H-1)) + 17 floor(H W / 50)), at least 1, can never overflow.
 * Execution: as above, one workgroup per region in either form; after the outer polygon is staged the holes are taken one after another (seed by an
 * integer atomicMin over the cells still unfilled, flood, border walk of one lane) with K / K' in the bitmap of T and the ring in the ring buffer, so the
 * first form keeps its static LDS.  A region one of whose rings does not fit the 5120 LDS ring points goes on in the second form from that hole.  Six
 * launches whatever the data; no host synchronisation; two runs, either form, an image alone or inside a batch give the same bits.  B == 0 or
 * max_regions == 0: returns 0 without a launch.  workspace: p3_hisup_polygons_rings_workspace_bytes(B, H, W, max_regions, max_vertices, max_rings,
 * max_ring_vertices) bytes.  Hand values (no junctions, (x, y)): a 15 x 14 block at rows 2..15, cols 3..17 with a hole at rows 4..9, cols 5..11: area 54,
 * ring [[12,4],[12,10],[5,10],[5,4],[12,4]] from 26 ring points; two 8-row holes at cols 4..11 and 13..21 with the one-pixel wall at col 12 between them:
 * areas 79 and 88, rings [[12,4],[12,12],[4,12],[4,4],[12,4]] and [[22,4],[22,12],[13,12],[13,4],[22,4]].
 * ------------------------------------------------------------------------------------------ */
int p3_hisup_polygons_rings(const int32_t* labels, const int32_t* n_regions, const int32_t* bbox, const float* juncs, const int32_t* junc_counts, int B,
                            int H, int W, int max_regions, int max_vertices, int max_rings, int max_ring_vertices, int force_fallback, float* pos,
                            int32_t* src, int64_t* poly_slice, int32_t* poly_flags, int32_t* hole_pixels, int32_t* n_vertices, int32_t* counts,
                            float* ring_pos, int32_t* ring_src, int64_t* ring_slice, int32_t* ring_region, int32_t* ring_flags, int32_t* ring_area2,
                            int32_t* region_rings, int32_t* n_holes, int32_t* ring_counts, int32_t* status, void* workspace, void* stream);
int64_t p3_hisup_polygons_rings_workspace_bytes(int B, int H, int W, int max_regions, int max_vertices, int max_rings, int max_ring_vertices);

/* ------------------------------------------------------------------------------------------
 * FFL polygons: the planar-graph half of shapely_postprocess (predict/ffl/polygonize_acm.py:281-324, polygonize_asm.py:438-494: LineString per piece and
 * the border ring, shapely.ops.unary_union, polygonize_full / polygonize, the min_area filter, polygonize_utils.compute_geom_prob :64-101 and the
 * seg_threshold filter) on the device, behind p3_corner_split (csrc/ffl_polygons.hip).  DESIGN.md section 19 holds the definition in full.
 * Input: the pieces as p3_corner_split leaves them - out_pos fp32 [V,2] (row, col), piece_slice int64 [Q,2], piece_batch int32 [Q] - and the indicator map
 * fp32 [B,H,W].  x = col, y = row.  Per image b:
 *   1  segments: the consecutive vertex pairs of the image's pieces, zero-length pairs dropped (-0 counts as +0), and the border ring (0,0), (0,H-1),
 *      (W-1,H-1), (W-1,0).
 *   2  a segment end that lies exactly on a border side splits that side there.
 *   3  nodes: the distinct end points; edges: the distinct unordered node pairs.
 *   4  two edges without a common node that share a point, or two edges with one common node that overlap collinearly (this covers a node inside an
 *      edge): image_status bit 0 and the image gives no polygon.  Predicates are signs of (b-a) x (c-a) in double.  A coordinate that is not finite:
 *      image_status bit 1, no polygon.
 *   5  dangles: edges with an end of degree 1 are deleted until none is left; then every edge whose two half-edges lie on one traced ring (a cut).
 *   6  faces: next(u->v) is the half-edge that comes before v->u in counter-clockwise order (half-plane, then cross product) among those leaving v, so that
 *      bounded faces have a positive S = sum(x_i y_{i+1} - x_{i+1} y_i).
 *   7  a ring starts at its half-edge of smallest key (origin (x, y), destination (x, y)); S is summed in double from there.  S > 0: a shell.  S < 0:
 *      a hole of the smallest-area shell of another component that contains its start node (crossing number), else the unbounded face, dropped.
 *      S == 0: image_status bit 2, no polygon.
 *   8  a polygon: a shell and its holes in key order; the polygons of an image in key order of their shells, images in order.  area = S(shell) / 2 -
 *      sum |S(hole) / 2|.  poly_flags bit 0: not (min_area < area).
 *   9  probability, compute_geom_prob: the shell's bounds minx = int(min x), maxx = int(max x) + 1 (int() truncates towards zero), the same in y; prob = 0
 *      when minx < 0 or miny < 0 or maxx > W or maxy > H.  Else every vertex becomes rint(x - minx) + minx (half to even, in the cropped window as the
 *      reference rounds it), a pixel of the window [minx, maxx) x [miny, maxy) is covered by a ring set when it lies on an edge of a rounded ring or
 *      inside by the even-odd rule over the whole set, raster = covered(shell) and not covered(holes), prob = sum(indicator[raster]) / count(raster) in
 *      double, 0 without a pixel.  poly_flags bit 1: not (seg_threshold < prob).
 * Outputs: ring_pos fp32 [max_vertices,2] (row, col; closed rings, the first vertex again at the end), ring_slice int64 [max_rings,2], poly_rings int64
 * [max_polygons,2] = [first, one past the last) ring, the shell first; poly_batch int32, poly_area fp32, poly_prob fp32, poly_flags int32 [max_polygons];
 * image_status int32 [B]; counts int32 [3] = (polygons, rings, vertices); status int32 [1]: bit 0 = a capacity was too small (counts hold the true totals,
 * nothing is written past a capacity), bit 1 = a piece with piece_batch outside [0, B) or a piece_slice row outside [0, V] was left out.  With E = 2 V +
 * 4 B (an image of n piece vertices has at most 2 n + 4 edges) E polygons, E rings and 3 E vertices can never overflow: a ring has 3 half-edges at least.
 * Errors before any launch, P3_EINVAL with a message: negative counts, H or W < 2, NaN thresholds, null pointers, and piece_slice / piece_batch in host
 * memory - the values are then checked right there (piece_batch out of [0, B), a piece_slice row outside out_pos), and the call is refused either way.
 * An image of up to 1024 edge slots (its segments + its segment ends on the border + 4) runs in one workgroup with every working array in LDS, a larger
 * one (or all, force_fallback != 0) runs the same device function over `workspace`; the probability takes one workgroup per polygon.  No floating-point
 * atomics, no host synchronisation; two runs, either form, an image alone or inside a batch give the same bits.
 * workspace: p3_ffl_polygons_workspace_bytes(V, B) bytes.
 * ------------------------------------------------------------------------------------------ */
int p3_ffl_polygons(const float* out_pos, int64_t V, const int64_t* piece_slice, const int32_t* piece_batch, int Q, const float* indicator, int B, int H,
                    int W, double min_area, double seg_threshold, int force_fallback, int max_polygons, int max_rings, int max_vertices,
                    float* ring_pos, int64_t* ring_slice, int64_t* poly_rings, int32_t* poly_batch, float* poly_area, float* poly_prob,
                    int32_t* poly_flags, int32_t* image_status, int32_t* counts, int32_t* status, void* workspace, void* stream);
int64_t p3_ffl_polygons_workspace_bytes(int64_t V, int B);

/* ------------------------------------------------------------------------------------------
 * Polygon metrics: the figures of the reference's Evaluator.evaluate that depend only on two polygon sets and the image size - IoU, C-IoU and NR
 * (eval/cIoU.py compute_IoU_cIoU) and POLIS, chamfer and Hausdorff (eval/polis_chamfer_hausdorff.py PointBasedMetrics, IoU threshold 0.5, sampling distance
 * 0.1) - on the device (csrc/poly_metrics.hip).  pycocotools and shapely are not linked: the text below and its float64 restatement
 * tests/poly_metrics_ref.py are the contract, DESIGN.md section 21 says where the text knowingly differs from those libraries.
 * Input: two ring sets, ground truth (gt) and predictions (dt).  A ring set: pos fp32 [V,2] in (x, y) order, ring_slice int64 [R,2] = [first vertex, one
 * past the last), ring_image int32 [R], non-decreasing.  Rings are open (n distinct vertices, the closing edge implied) and exterior rings only.  A ring
 * with fewer than 3 vertices, or with a coordinate that is not finite or lies beyond +-32768, is invalid: it takes part in nothing, is counted in
 * invalid_rings[image] and sets status bit 0.  A ring with ring_image outside [0, B) or a slice outside [0, V] is left out and sets status bit 1.
 * All arithmetic is in double on the fp32 coordinates converted once, every product and sum rounded on its own (no fused multiply-add).
 *   1  mask of an image: pixel (r, c), 0 <= r < H, 0 <= c < W, has centre p = (c + 0.5, r + 0.5) and lies in a ring by the even-odd rule: an edge (a, b),
 *      the closing one included, is crossed when (a.y <= p.y) != (b.y <= p.y), and the crossing lies to the right of p when the sign of
 *      (b.x - a.x)(p.y - a.y) - (p.x - a.x)(b.y - a.y) equals the sign of b.y - a.y.  The mask of a set is the union of the parities of its valid rings.
 *   2  per image: I = |gt and dt|, U = |gt or dt| as integers; iou = 1 when U == 0, else I / (U + 1e-9); N_gt, N_dt the vertex counts of the valid
 *      rings; nr = 1 - |N_dt - N_gt| / (N_dt + N_gt + 1e-9); ciou = iou nr.  IoU, C-IoU and NR are the means over all B images, summed in image order.
 *   3  matching per image: the box of a ring is [min x, min y, max x - min x, max y - min y]; box IoU with iw = min(x0 + w0, x1 + w1) - max(x0, x1), ih
 *      likewise, 0 when iw <= 0 or ih <= 0, else i = iw ih and iou = i / (w0 h0 + w1 h1 - i).  For every valid gt ring in order the matched prediction is
 *      the first argmax over the image's valid predictions; the pair counts when that box IoU is > 0.5.
 *   4  POLIS of a pair (A = gt, B = prediction): side(A, B) = (sum over the n vertices a of A of d(a, ring B)) / (2 (n + 1)), d the least point-to-segment
 *      distance over B's n_B edges, the closing one included (t = clamp(((a - p).(q - p)) / |q - p|^2, 0, 1), d = |a - (p + t (q - p))|; a zero-length
 *      edge is the point p); polis = side(A, B) + side(B, A).
 *   5  samples of a ring: for each edge (p, q) in order, the closing edge last, L = sqrt(dx dx + dy dy), m = max(1, ceil(L / 0.1)) and the samples
 *      p + ((j (L / m)) / L) (q - p), j = 0 .. m-1 (p once when L == 0); behind the last edge the first vertex once more.
 *   6  chamfer and Hausdorff of a pair: S_A, S_B the samples, d1[i] = min_j |S_A[i] - S_B[j]|, d2 the other way round; chamfer = (mean d1 + mean d2) / 2,
 *      hausdorff = max(max d1, max d2).
 *   7  an image without a counted pair is not valid; else its three figures are the means over its counted pairs in gt order.  POLIS, chamfer and
 *      hausdorff are the means over the valid images in image order, NaN when there is none.
 * modes: P3_PM_IOU (steps 1-2), P3_PM_POLIS (step 4), P3_PM_SAMPLES (steps 5-6), any non-empty set; what a mode that is off would give is NaN (image_iou, image_nr
 * and metrics[0..2]; pair_polis, image_polis and metrics[3]; the chamfer and hausdorff outputs; image_counts: 0).  match, image_valid and invalid_rings do not depend on modes.
 * Outputs: metrics fp64 [6] = (IoU, C-IoU, NR, POLIS, chamfer, hausdorff); image_iou, image_nr, image_polis, image_chamfer, image_hausdorff fp64 [B] (NaN
 * for the last three where the image is not valid); image_valid int32 [B]; image_counts int32 [B,2] = (I, U); match int32 [R_gt]: the index of the matched
 * ring in the prediction set, -1 when the gt ring has no counted pair; pair_polis, pair_chamfer, pair_hausdorff fp64 [R_gt], NaN where match is -1;
 * invalid_rings int32 [B,2] = (gt, dt); status int32 [1].
 * Errors before any launch, P3_EINVAL with a message: negative counts, B, H or W < 1, H W above 2^18 (both bit-packed masks of an image are held in LDS),
 * an empty or unknown modes, null pointers, and ring_slice / ring_image in host memory.
 * Launches depend on the shapes and modes only; no floating-point atomics, no host synchronisation; two runs, an image alone or inside a batch give the
 * same bits.  workspace: p3_polygon_metrics_workspace_bytes(R_gt, R_dt, B) bytes (0 for B < 1 or a negative count).
 * ------------------------------------------------------------------------------------------ */
#define P3_PM_IOU 1
#define P3_PM_POLIS 2
#define P3_PM_SAMPLES 4
int p3_polygon_metrics(const float* gt_pos, int64_t V_gt, const int64_t* gt_slice, const int32_t* gt_image, int R_gt, const float* dt_pos, int64_t V_dt,
                       const int64_t* dt_slice, const int32_t* dt_image, int R_dt, int B, int H, int W, int modes, double* metrics, double* image_iou,
                       double* image_nr, double* image_polis, double* image_chamfer, double* image_hausdorff, int32_t* image_valid, int32_t* image_counts,
                       int32_t* match, double* pair_polis, double* pair_chamfer, double* pair_hausdorff, int32_t* invalid_rings, int32_t* status,
                       void* workspace, void* stream);
int64_t p3_polygon_metrics_workspace_bytes(int R_gt, int R_dt, int B);

/* ------------------------------------------------------------------------------------------
 * COCO AP / AR of a predicted ring set against a ground-truth ring set, on instance masks (segm) and on their boundaries (boundary): the reference's
 * Evaluator.compute_coco_metrics (pycocotools COCOeval, iouType 'segm', one category) and compute_boundary_coco_metrics (boundary-iou-api), on the device
 * (csrc/coco_metrics.hip).  Neither library is linked: the text below and its float64 / integer restatement tests/coco_metrics_ref.py are the contract,
 * DESIGN.md section 22 says where the text knowingly differs from those libraries.
 * Input: two ring sets as for p3_polygon_metrics (pos, ring_slice, ring_image non-decreasing; open exterior rings), with one optional fp32 [R] field each:
 * dt_score, the prediction's score (null: every score is 1.0), and gt_area, the annotation's area that sorts a gt ring into the size buckets (null: the
 * ring's own pixel count).  Ring validity, status bits 0 and 1 and the bound H W <= 2^18 are those of p3_polygon_metrics; a prediction whose score is NaN
 * is invalid (bit 0).  Counts are integers, quotients are doubles of those integers, every operation rounded on its own.
 *   1  instance mask: the pixels (r, c) of the H x W image whose centre (c + 0.5, r + 0.5) lies in the ring by the even-odd crossing rule of
 *      p3_polygon_metrics step 1, for this ring alone; area_px is its pixel count.  The area of a prediction is area_px, that of a gt ring gt_area or area_px.
 *   2  boundary mask: d = max(1, (int)rint(0.02 sqrt(H H + W W))), rint rounding half to even; the eroded mask keeps a pixel when every pixel of the
 *      (2d+1) x (2d+1) square around it is in the mask, pixels outside the image counting as not in it; the boundary is the mask minus the eroded mask.
 *   3  pair IoU, per image, between every valid gt ring and the image's kept predictions - its valid predictions in stable order of descending score, the
 *      first 100: I the common pixels, U = a + b - I, iou = 0 when U == 0, else (double)I / (double)U.  For boundary the IoU of a pair is the smaller of
 *      its mask IoU and the IoU of the two boundary masks.
 *   4  tables: iouThrs = linspace(0.5, 0.95, 10) and recThrs = linspace(0, 1, 101) as numpy's doubles (p3_coco_thresholds); area ranges [0, 1e10],
 *      [0, 1024], [1024, 9216], [9216, 1e10]; maxDets 1, 10, 100.
 *   5  matching (evaluateImg, no crowd) per image, area range a and threshold t: a gt ring is ignored when its area is < lo or > hi; the gt rings are
 *      visited in stable order of that flag, not-ignored first.  The kept predictions are visited in order; for each the running best starts at
 *      min(t, 1 - 1e-10) with no match; walking the gt rings, one already matched at this (a, t) is skipped, the walk stops at the first ignored gt ring
 *      once a not-ignored match is held, a gt ring whose IoU is less than the running best is skipped (equality matches), any other is taken and raises the
 *      running best to its IoU.  A matched prediction inherits the ignore flag of its gt ring; an unmatched one is ignored when its own area lies outside
 *      the range.  The matching for maxDets 1 and 10 is the prefix of the one for 100.
 *   6  accumulation (accumulate) per (a, m): the first m kept predictions of every image, in image order, ordered stably by descending score; npig the
 *      number of not-ignored gt rings - 0 leaves -1 in the (a, m) entries of precision and recall; tp, fp the integer prefix counts of the not-ignored
 *      matched and unmatched predictions; per t, with nd predictions: rc = tp / npig, pr = tp / (fp + tp + 2^-52), recall[t, a, m] = rc[nd-1] (0 when
 *      nd == 0), pr made non-increasing from the right, precision[t, r, a, m] = pr[first i with rc[i] >= recThrs[r]] (0 when there is none).
 *   7  stats (summarize), 12 per type in pycocotools' order - AP, AP50, AP75, AP small, medium, large (maxDets 100), AR at maxDets 1, 10, 100 (all areas),
 *      AR small, medium, large (maxDets 100): the mean, summed in index order, over the entries > -1; -1 when there is none.
 * iou_types: P3_COCO_SEGM | P3_COCO_BOUNDARY, any non-empty set.  A type that is off leaves NaN in its row of stats, precision and recall, -1 in its rows of
 * dt_match and gt_match and 0 in its rows of dt_ignore; without P3_COCO_BOUNDARY no boundary is built: gt_boundary_px, dt_boundary_px and row 1 of
 * pair_inter hold 0.  The areas, dt_rank and row 0 of pair_inter do not depend on iou_types.
 * Outputs: stats fp64 [2,12] (row 0 segm, row 1 boundary); precision fp64 [2,10,101,4,3]; recall fp64 [2,10,4,3]; gt_area_px, gt_boundary_px int32 [R_gt],
 * dt_area_px, dt_boundary_px int32 [R_dt] (0 for a ring that is not valid); dt_rank int32 [R_dt]: the position among its image's kept predictions, -1 when
 * not kept; pair_inter int32 [2, 100 R_gt]: I of gt ring g and the prediction of rank k at 100 g + k (0 where no kept prediction has that rank, and where
 * the masks do not overlap); dt_match int32 [2,4,10,R_dt]: the gt ring index or -1; dt_ignore uint8 of that shape; gt_match int32 [2,4,10,R_gt]: the
 * prediction's ring index or -1; status int32 [1].
 * Errors before any launch, P3_EINVAL with a message: those of p3_polygon_metrics, an empty or unknown iou_types, dt_score / gt_area in host memory.
 * Launches depend on the shapes and iou_types only; no floating-point atomics, no host synchronisation; two runs, an image alone or inside a batch give the
 * same bits in every per-ring and per-pair output.  workspace: p3_coco_metrics_workspace_bytes(R_gt, R_dt, B, H, W, iou_types) bytes (0 for arguments
 * the entry refuses).  p3_coco_thresholds (host only) copies the two threshold tables out; either pointer may be null.
 * ------------------------------------------------------------------------------------------ */
#define P3_COCO_SEGM 1
#define P3_COCO_BOUNDARY 2
int p3_coco_metrics(const float* gt_pos, int64_t V_gt, const int64_t* gt_slice, const int32_t* gt_image, const float* gt_area, int R_gt,
                    const float* dt_pos, int64_t V_dt, const int64_t* dt_slice, const int32_t* dt_image, const float* dt_score, int R_dt, int B, int H, int W,
                    int iou_types, double* stats, double* precision, double* recall, int32_t* gt_area_px, int32_t* dt_area_px, int32_t* gt_boundary_px,
                    int32_t* dt_boundary_px, int32_t* dt_rank, int32_t* pair_inter, int32_t* dt_match, uint8_t* dt_ignore, int32_t* gt_match, int32_t* status,
                    void* workspace, void* stream);
int64_t p3_coco_metrics_workspace_bytes(int R_gt, int R_dt, int B, int H, int W, int iou_types);
void p3_coco_thresholds(double* iou10, double* rec101);

/* ------------------------------------------------------------------------------------------
 * Max tangent angle error (MTA): the mean over the predicted polygons of the largest angle between a polygon's contour and the ground-truth contour it
 * projects onto - the reference's eval/angle_eval.py (the Frame Field Learning contour measure), on the device (csrc/mta_metrics.hip).  shapely is not
 * linked: the text below and its float64 restatement tests/mta_ref.py are the contract, DESIGN.md section 23 says where the text knowingly differs from
 * angle_eval.py.
 * Input: two ring sets exactly as for p3_polygon_metrics (pos fp32 [V,2] in (x, y), ring_slice int64 [R,2], ring_image int32 [R] non-decreasing; open
 * exterior rings).  Ring validity, status bits 0 and 1 and the bound H W <= 2^18 are those of p3_polygon_metrics.  Parameters: sampling_spacing (the
 * reference: 2.0), min_precision (0.5), max_stretch (2.0).  All arithmetic is in double on the fp32 coordinates converted once, every product and sum
 * rounded on its own (no fused multiply-add).
 *   1  masks: the instance mask of a valid prediction ring is p3_coco_metrics step 1 (the even-odd crossing rule at pixel centres, the ring alone), A its
 *      pixel count; the gt mask of an image is p3_polygon_metrics step 1 (the union of the parities of its valid gt rings); I = the pixels of the
 *      prediction's mask that are in the gt mask.
 *   2  precision filter: A == 0: the ring is empty (the reference drops zero-area polygons); else it is kept when (double)I / (double)A > min_precision,
 *      else it is below precision.
 *   3  samples of a kept prediction ring: for each edge (p, q) in order, the closing edge last, L = sqrt(dx dx + dy dy) and
 *      m = max(1, (int)rint(L / sampling_spacing)), rint rounding half to even; the points of the edge are
 *      p + j ((q - p) / m), j = 0 .. m-1, the step computed per component, and the end point q itself (the last point of a linspace); the first point of
 *      every edge but the first is skipped, so that the sample line starts at vertex 0 and ends at vertex 0 again: 1 + sum m samples.
 *   4  projection of a sample s: its nearest point on the edges of all valid gt rings of the same image, closing edges included, rings in set order and
 *      edges in ring order.  Per edge (p, q): t = ((s - p).(q - p)) / |q - p|^2; the point is p when t <= 0 or the edge has zero length, q when t >= 1,
 *      else p + t (q - p); the squared distance is e = dx dx + dy dy; the first edge with the strictly smallest e wins.
 *   5  edges of a ring: for consecutive samples k, k+1: u = s[k+1] - s[k], v = proj[k+1] - proj[k], |u| = sqrt(ux ux + uy uy), |v| likewise; the edge is
 *      valid when |u| |v| > 0 and 1 / max_stretch < |u| / |v| < max_stretch, both strict; c = fabs((ux vx + uy vy) / (|u| |v|)); ring_cos is the least c
 *      over the valid edges; a ring without a valid edge has no valid edge (the reference's None).
 *   6  ring_angle = acos(min(1, ring_cos)) in radians; MTA is the mean of (ring_angle 180) / pi over the counted rings of the whole call, summed in ring
 *      order, NaN when nothing is counted.
 *   7  overlap report: per image, image_overlap_px = (sum of A over its valid predictions) - (pixel count of the union of their masks); status bit 2
 *      (value 4) is set when it is non-zero anywhere: in such an image the reference would have merged the overlapping predictions before measuring.
 * Outputs: mta fp64 [1] in degrees; counted int32 [1]; ring_angle, ring_cos fp64 [R_dt], NaN unless the ring is counted; ring_state int32 [R_dt]:
 * P3_MTA_COUNTED, P3_MTA_INVALID (invalid or left out), P3_MTA_EMPTY, P3_MTA_BELOW_PRECISION, P3_MTA_NO_EDGE; ring_px int32 [R_dt,2] = (A, I), both 0 for
 * P3_MTA_INVALID; image_overlap_px int32 [B]; invalid_rings int32 [B,2] = (gt, dt); status int32 [1].
 * Errors before any launch, P3_EINVAL with a message: those of p3_polygon_metrics (negative counts, B, H or W < 1, H W above 2^18, null pointers,
 * ring_slice / ring_image in host memory); sampling_spacing not finite, <= 0 or below 1 / 64 (with coordinates within 2^15 an edge then has fewer than 2^23 samples); min_precision outside [0, 1); max_stretch not finite or <= 1.
 * Launches depend on the shapes only; no floating-point atomics, no host synchronisation; two runs give the same bits in every per-ring and per-image
 * output, and so does an image alone or inside a batch.  workspace: p3_max_tangent_angle_workspace_bytes(R_gt, R_dt, B) bytes (0 for B < 1 or a negative
 * count).
 * ------------------------------------------------------------------------------------------ */
#define P3_MTA_COUNTED 0
#define P3_MTA_INVALID 1
#define P3_MTA_EMPTY 2
#define P3_MTA_BELOW_PRECISION 3
#define P3_MTA_NO_EDGE 4
int p3_max_tangent_angle(const float* gt_pos, int64_t V_gt, const int64_t* gt_slice, const int32_t* gt_image, int R_gt, const float* dt_pos, int64_t V_dt,
                         const int64_t* dt_slice, const int32_t* dt_image, int R_dt, int B, int H, int W, double sampling_spacing, double min_precision,
                         double max_stretch, double* mta, int32_t* counted, double* ring_angle, double* ring_cos, int32_t* ring_state, int32_t* ring_px,
                         int32_t* image_overlap_px, int32_t* invalid_rings, int32_t* status, void* workspace, void* stream);
int64_t p3_max_tangent_angle_workspace_bytes(int R_gt, int R_dt, int B);

/* ------------------------------------------------------------------------------------------
 * Mask and topology metrics, subset IoU and annotation counts: the modes `topdig` (eval/topdig_metrics.py compute_mask_metrics: pixel accuracy, F1 and IoU
 * of the filled union masks and of the "topology" masks, the polygon outlines stroked buffer_thickness pixels thick), `subset_iou`
 * (compute_IoU_cIoU(subset=True): IoU, C-IoU and NR over the images that have a prediction) and `stats` (compute_coco_stats) of the reference's
 * Evaluator.evaluate, on the device (csrc/mask_metrics.hip).  Neither OpenCV, pycocotools nor torchmetrics is linked: the text below and its
 * float64 / Python-integer restatement tests/mask_metrics_ref.py are the contract, DESIGN.md section 24 says where the text knowingly differs from them.
 * Input: two ring sets exactly as for p3_polygon_metrics (pos fp32 [V,2] in (x, y), ring_slice int64 [R,2], ring_image int32 [R] non-decreasing; open
 * exterior rings).  Ring validity, status bits 0 and 1 and the bound H W <= 2^18 are those of p3_polygon_metrics.  buffer_thickness = T (the reference: 5).
 *   1  filled mask of a set in image b: p3_polygon_metrics step 1 (the even-odd rule at the pixel centres (c + 0.5, r + 0.5), the union of the parities of
 *      the valid rings).
 *   2  stroked mask of a set in image b: each vertex of a valid ring becomes the integer point q = (rint(x), rint(y)), rint of the double made of the fp32
 *      coordinate, half to even (with |x| <= 2^15 it fits int32).  Pixel (r, c) is the integer point p = (c, r), not its centre (OpenCV's convention).
 *      For every edge (a, b) of the ring, the closing one included: d = b - a, u = p - a, L2 = d.d, t = u.d; the pixel is set when the first matching
 *      condition holds:  L2 == 0 or t <= 0: 4 u.u <= T T;  t >= L2: 4 |p - b|^2 <= T T;  otherwise 4 (u.x d.y - u.y d.x)^2 <= T T L2  - the pixel lies
 *      within T / 2 of the segment, decided in exact integer arithmetic.  The mask is the union over the edges of all valid rings of the set in image b.
 *   3  confusion counts per image and mask kind, p the prediction mask and g the gt mask: TP = |p & g|, FP = |p & ~g|, FN = |~p & g|,
 *      TN = H W - TP - FP - FN, int32.  TP + FP + FN == 0: acc = f1 = iou = 1.0; else acc = (double)(TP + TN) / (double)(H W),
 *      f1 = (double)(2 TP) / (double)(2 TP + FP + FN), iou = (double)TP / ((double)(TP + FP + FN) + 1e-9): one correctly rounded division each, the
 *      iou one addition before it.
 *   4  TopDiG means: IoU_, P-Acc, F1-Score from the filled masks, IoU-Topo, P-Acc-Topo, F1-Score-Topo from the stroked masks, each the sum over the B
 *      images in image order divided by B.
 *   5  subset: image b is in the subset when the prediction set has at least one ring with ring_image == b, whatever its state.  Per image iou is step 3
 *      on the filled masks and nr is p3_polygon_metrics step 2 (the vertex counts of the valid rings).  sIoU, sC-IoU (the products iou nr) and sNR are the
 *      means over the subset, summed in image order; NaN when the subset is empty.
 *   6  stats int64 [7] = (B, images with at least one counted gt ring, images with at least one counted prediction ring, gt rings, prediction rings, gt
 *      vertices, prediction vertices).  A ring is counted unless it is left out (status bit 1); its vertices are its slice length, valid or not.
 * modes: P3_MM_TOPDIG (steps 1-4), P3_MM_SUBSET (steps 1, 3, 5), P3_MM_STATS (step 6), any non-empty set.  A mode that is off leaves NaN in its
 * floating-point outputs and 0 in its integer outputs: without P3_MM_TOPDIG metrics[0..5] and image_scores are NaN and the stroked row of image_conf is 0;
 * without P3_MM_SUBSET metrics[6..8] and image_nr are NaN and image_subset is 0; without both the filled row of image_conf is 0 too; without P3_MM_STATS
 * stats is 0.  invalid_rings and status do not depend on modes.
 * Outputs: metrics fp64 [9] = (IoU_, P-Acc, F1-Score, IoU-Topo, P-Acc-Topo, F1-Score-Topo, sIoU, sC-IoU, sNR); stats int64 [7]; image_conf int32 [B,2,4]
 * = (filled, stroked) x (TP, FP, FN, TN); image_scores fp64 [B,6], per image in the order of metrics[0..5]; image_nr fp64 [B]; image_subset int32 [B];
 * invalid_rings int32 [B,2] = (gt, dt); status int32 [1].
 * Errors before any launch, P3_EINVAL with a message: those of p3_polygon_metrics (negative counts, B, H or W < 1, H W above 2^18, null pointers,
 * ring_slice / ring_image in host memory); buffer_thickness outside [1, 64]; an empty or unknown modes.
 * Launches depend on the shapes and modes only; no floating-point atomics, no host synchronisation; two runs, an image alone or inside a batch give the
 * same bits.  workspace: p3_mask_metrics_workspace_bytes(R_gt, R_dt, B) bytes (0 for B < 1 or a negative count).
 * ------------------------------------------------------------------------------------------ */
#define P3_MM_TOPDIG 1
#define P3_MM_SUBSET 2
#define P3_MM_STATS 4
int p3_mask_metrics(const float* gt_pos, int64_t V_gt, const int64_t* gt_slice, const int32_t* gt_image, int R_gt, const float* dt_pos, int64_t V_dt,
                    const int64_t* dt_slice, const int32_t* dt_image, int R_dt, int B, int H, int W, int buffer_thickness, int modes, double* metrics,
                    int64_t* stats, int32_t* image_conf, double* image_scores, double* image_nr, int32_t* image_subset, int32_t* invalid_rings,
                    int32_t* status, void* workspace, void* stream);
int64_t p3_mask_metrics_workspace_bytes(int R_gt, int R_dt, int B);

#ifdef __cplusplus
}
#endif
#endif
