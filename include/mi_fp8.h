/*
 * mi_fp8.h -- C ABI of libmi_fp8.so: the MI355X (gfx950) FP8 Linear hot path.
 *
 * This is the drop-in boundary of the build.  The reference
 * (xuanvinh1997/llm-fp8) has no FFI of its own: its FP8 arithmetic is reached
 * through Python calls into transformer_engine.pytorch modules
 *   te_llama.py:45-63,76-80      MultiheadAttention / LayerNormMLP under fp8_autocast
 *   te_llama_hybrid.py:39,75,78  single HYBRID recipe
 *   te_llama_mxfp8.py:28-29,86,93  MXFP8BlockScaling recipe
 *   accelerate utils/transformer_engine.py:52-59  nn.Linear -> te.Linear
 * Each entry point below names the TE-internal kernel
 * it replaces on that path.  INTEGRATION.md shows the ctypes stub that binds
 * them (llm_fp8_amd/_lib.py is that stub).
 *
 * Conventions
 *   - plain C, device pointers are `void*` / `float*` into HBM owned by the caller
 *     (PyTorch caching allocator); the library allocates nothing persistent.
 *   - `stream` is a hipStream_t passed as void*; all work is enqueued on it, no
 *     internal synchronisation, no global mutable state besides the thread-local
 *     error string -- with ONE documented exception: mi_gemm_set_workspace binds a
 *     caller-owned stream-K workspace to the current device (per-device table, used
 *     only by the explicit algo 44; never touched by the automatic choice).
 *   - return 0 on success, <0 on error: -1 invalid argument, -2 unsupported shape,
 *     -3 HIP runtime error.  mi_last_error() gives the message (thread-local).
 *   - matrices are row-major; `fmt`: 0 = OCP E4M3FN, 1 = OCP E5M2.
 *   - all GEMMs are "TN": D[M,N] = A[M,K] . B[N,K]^T with K contiguous in both
 *     operands; dgrad / wgrad use the transposed fp8 copies the cast kernels emit.
 */
#ifndef MI_FP8_H
#define MI_FP8_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MI_FMT_E4M3 0
#define MI_FMT_E5M2 1

#define MI_OK 0
#define MI_ERR_ARG (-1)
#define MI_ERR_SHAPE (-2)
#define MI_ERR_HIP (-3)

#define MI_OUT_BF16 0
#define MI_OUT_F32 1

#define MI_AMAX_ALGO_MAX 0
#define MI_AMAX_ALGO_MOST_RECENT 1

/* ABI version and revision.  The VERSION changes when an existing entry point changes its signature or the meaning of an
 * argument, or goes away: a binding written against another version must not call the library (llm_fp8_amd/_lib.py compares at
 * load time).  The REVISION counts the entry points added since that version: every caller of revision r works unchanged with a
 * library of the same version and a revision >= r, and a binding that finds a lower revision knows which entry points are missing.
 * mi_abi_version() / mi_abi_revision() return the values the library was built with.  (Up to version 5 an added entry point
 * bumped the version; the history below records that.)
 *   1  round 1 (the surface of SURVEY.md 8b + fused neighbours)
 *   2  round 2: mi_gemm_fp8 algo values 20-30, 46 (diagnostic builds), mi_adamw_cast_bf16_multi, mi_transpose_u8,
 *      mi_gemm_fp8_grouped
 *   3  round 2: mi_adamw_mxcast_bf16_multi
 *   4  round 3: diagnostic algo values and mi_attn_fwd_diag moved out (lab build, -DMI_DIAG); mi_gemm_fp8 algos 6, 9, 47 and
 *      mi_gemm_fp8_grouped tile_cfg 4 (four-wave kernel); mi_gemm_fp8_clock; mi_swiglu_cast_bias, mi_dswiglu_cast_bias,
 *      mi_add_bias_rmsnorm_stats (bias fused into the consumer of the GEMM output)
 *   5  mi_gemm_mxfp8_grouped (a Linear's block-scaled dgrad + wgrad in one persistent launch)
 * Revisions of version 5:
 *   1  mi_adamw_f32_multi (fp32 master weights and moments in the fused AdamW + FP8 cast pass), mi_abi_revision
 *   2  mi_amax_bf16, mi_amax_norm, mi_amax_swiglu, mi_amax_dswiglu, mi_current_scale (Float8CurrentScaling: the amax of a tensor
 *      before its cast, and the scale from it)
 *   3  mi_blockfp8_quantize_ex, mi_blockfp8_norm_quantize, mi_blockfp8_swiglu_quantize, mi_blockfp8_dswiglu_quantize
 *      (Float8BlockScaling: 1 x 128 and 128 x 128 power-of-two block scales in the MX operand layout)
 *   4  mi_adamw_sr_bf16_multi (stochastic rounding of the bf16 weight and moments in the fused AdamW + FP8 cast pass)
 *   5  no new entry point: every mi_adamw_* call reads a NON-FINITE *grad_scale as "skip the step" (THE STEP GUARD below, at
 *      mi_sumsq_bf16).  A caller that sends NaN to drop a step needs a library of this revision; finite values and NULL are unchanged.
 *   6  mi_qknorm_rope_qkv, mi_qknorm_rope_qkv_bwd (per-head QK RMSNorm fused into the RoPE split: Qwen3 attention)
 *   7  mi_grad_accum_multi (fp32 gradient accumulation over a window of micro-batches, rounded to bf16 once)
 */
#define MI_ABI_VERSION 5
#define MI_ABI_REVISION 7
int mi_abi_version(void);
int mi_abi_revision(void);
/* Thread-local message of the last failing call on this thread ("" if none). */
const char* mi_last_error(void);
/* 1 if the current HIP device is gfx950 (MI355X), else 0; <0 on HIP error. */
int mi_device_supported(void);

/*
 * K1/K2  cast (+transpose) + amax, delayed scaling  [replaces TE quantize / cast_transpose].
 *   y[r*ld_y + c]   = sat_cast_fmt(float(x[r*cols+c]) * *scale)          (RNE, NaN -> 0x7F)
 *   yT[c*ld_yT + r] = same byte                                           (if yT != NULL)
 *   *amax           = max(*amax, max|x|)   atomically (fmaxf semantics: NaN ignored)
 * x: bf16 [rows, cols] contiguous.  rows, cols multiples of 8.  ld_y >= cols, ld_yT >= rows.
 * y may be NULL when only the transposed copy is wanted.  amax may be NULL.
 */
int mi_cast_amax(const void* x_bf16, void* y_fp8, void* yT_fp8, const float* scale, float* amax,
                 int64_t rows, int64_t cols, int64_t ld_y, int64_t ld_yT, int fmt, void* stream);
/* yT[c * ld_yT + r] = y[r * ld_y + c] on FP8 bytes (rows, cols multiples of 8): the transposed copy of an operand that was
 * quantised elsewhere -- after an FP8 all-gather of row shards (llm_fp8_amd.distributed.ShardedFP8DP). */
int mi_transpose_u8(const void* y, void* yT, int64_t rows, int64_t cols, int64_t ld_y, int64_t ld_yT, void* stream);
/*
 * mi_cast_amax that also returns the column sums of x (the bias gradient when x = grad_output of a Linear,
 * `db = sum_M dy`): colsum_partial [ceil(rows/64), cols] fp32, one row per 64-row tile, to be reduced by
 * mi_colsum_finish.  Fixed summation order: reproducible.
 */
int mi_cast_amax_colsum(const void* x_bf16, void* y_fp8, void* yT_fp8, const float* scale, float* amax,
                        float* colsum_partial, int64_t rows, int64_t cols, int64_t ld_y, int64_t ld_yT, int fmt, void* stream);
/* out[c] = sum_p partial[p, c]; out bf16 (MI_OUT_BF16) or fp32 (MI_OUT_F32).  Second stage of every partial column sum
 * the library emits (mi_cast_amax_colsum, mi_dswiglu_cast, mi_mxfp8_dswiglu_quantize, mi_rmsnorm_bwd). */
int mi_colsum_finish(const float* partial, int64_t P, int64_t C, void* out, int out_dtype, void* stream);
/* Up to 4 mi_colsum_finish in one launch (host arrays of length n; same arithmetic and summation order per output). */
int mi_colsum_finish_multi(const void* const* partials, const int64_t* P, const int64_t* C, void* const* outs,
                           const int* out_dtypes, int n, void* stream);

/*
 * K3  amax-history roll + scale update for S slots in ONE launch
 *     [replaces TE fused_amax_and_scale_update_after_reduction].
 *   amax = max_h hist[h][s] (algo MAX) | hist[0][s] (MOST_RECENT)
 *   hist = roll(hist, -1, dim 0); hist[0][s] = 0
 *   sf = (fp8_max[s] / amax) / 2^margin ; keep old scale if !(amax > 0) or !isfinite(amax);
 *   sf = FLT_MAX if isinf(sf) ; scale[s] = sf ; scale_inv[s] = 1 / sf
 * amax_history: [H, S] fp32, row stride `ld` >= S floats (a used prefix of a larger arena).  H <= 4096.
 */
int mi_scale_update(float* amax_history, float* scale, float* scale_inv, const float* fp8_max,
                    int H, int S, int64_t ld, int margin, int algo, void* stream);

/*
 * K4/K5/K6  FP8 x FP8 -> bf16 GEMM on gfx950 MFMA (v_mfma_scale_f32_16x16x128_f8f6f4, unit scales)
 *           [replaces TE's cuBLASLt FP8 GEMM: fprop, dgrad, wgrad].
 *   D[m*ldd + n] = bf16( (sum_k A[m*lda+k] * B[n*ldb+k]) * (*sa_inv * *sb_inv) + bias[n] )
 * A: fp8 [M,K] fmt_a, B: fp8 [N,K] fmt_b, D: bf16 [M,N] (out_dtype 0) or fp32 (out_dtype 1).
 * bias: bf16 [N] or NULL.  M, N multiples of 16 (8 for the generic path), K multiple of 16.
 * algo: 0 = auto, 1 = generic 64x64 tile, 2 = 256x256 two-phase, 3 = 256x256 eight-phase ping-pong (eight waves),
 *       4 = persistent eight-phase (one workgroup per CU, epilogue overlapped with the next tile),
 *       5 = the kernel of 4 launched with one workgroup per tile (hardware-balanced: for use while collectives hold part of
 *           the chip), 6 = four-wave kernel (128x128 wave tiles, one wave per SIMD; mi_gemm_w4.hip), one tile per workgroup,
 *       9 = persistent four-wave kernel, 40-43 force one tile shape of 4, 44 = stream-K form of 4 (see mi_gemm_set_workspace),
 *       45 = 4, 47 = auto that takes the persistent four-wave kernel where it is the faster one (256-multiples, K >= 512, and
 *       256 x 256 is the eight-wave kernel's own tile choice; with or without a bias), else as 0.  Of the four-wave kernels
 *       only 9 takes a bias: 6 with one is MI_ERR_ARG.
 * 2/3/6 need M,N % 256 == 0 and K % 128 == 0 (6, 9: K % 256 == 0); 4 additionally K % 256 == 0, bf16 output and operands
 * below 2 GiB (M, N may also be multiples of 192: workgroup tiles of 256/192 rows x 256/192 columns are picked per shape).
 * auto picks a persistent kernel when the shape allows, else 3, else 1.  Every algo listed here gives the SAME bits for the
 * same inputs (one fp32 summation order per output element), tests/test_kernels_gpu.py.
 * Not part of this library: the timing / ablation / stamp builds (algos 7, 8, 10-30, 46, 50-73) live in the lab build
 * (tools/bin/libmi_fp8_lab.so, `make -C llm_fp8_amd/csrc lab`, compiled with -DMI_DIAG; see tools/README.md); the product
 * library returns MI_ERR_ARG for them.
 * Leading dimensions and pointers (every algo; pinned by tests/test_gemm_contract_gpu.py): A, B and D may be views into larger
 * buffers.  lda, ldb >= K and multiples of 16 (bytes); ldd >= N and a multiple of 4 (elements: a bf16 row may then be only 8-byte
 * aligned, the kernels' 16-byte stores take that); A, B and D 16-byte aligned.  Anything else is MI_ERR_ARG and nothing is
 * launched.  Only the K bytes of each operand row are read and only the N elements of each output row are written: padding
 * columns and neighbouring rows are never touched.  The persistent algos (4, 5, 6, 9, 40-45) use 32-bit buffer offsets over
 * rows * ld bytes: M * lda, N * ldb and 2 * M * ldd must stay below 2^31 (MI_ERR_SHAPE when asked for explicitly; 0 / 47 fall
 * back to 3 or 1).
 * Non-finite values propagate, they are never scrubbed: a NaN byte (0x7F / 0xFF in E4M3, 0x7D-0x7F / 0xFD-0xFF in E5M2; the casts
 * emit 0x7F for a NaN input on purpose) makes exactly its output row (byte in A) or column (byte in B) NaN, an E5M2 +-Inf byte makes
 * it non-finite, a NaN / +-Inf bias element gives a NaN / +-Inf column, and every other output keeps the bits it has without the
 * poison; nothing carries over into a later launch (stream-K workspace included).  *sa_inv or *sb_inv NaN -> all NaN, Inf ->
 * nothing finite, 0 -> +-0 (exactly the bias, with one).  A product with alpha beyond FLT_MAX is +-Inf in both output types; a
 * finite fp32 value beyond the bf16 range rounds to +-Inf (round-to-nearest-even), it does not saturate.
 */
int mi_gemm_fp8(const void* A, const void* B, void* D, const float* sa_inv, const float* sb_inv,
                const void* bias_bf16, int64_t M, int64_t N, int64_t K, int64_t lda, int64_t ldb,
                int64_t ldd, int fmt_a, int fmt_b, int out_dtype, int algo, void* stream);

/*
 * Measurement aid (bench.py `roofline.clock_ghz`): the persistent production kernel (algo 0 / 4 / 9 as mi_gemm_fp8 would run
 * it, E4M3 x E4M3, no bias) with two clock reads around each workgroup's whole tile walk.  stamps: u64 [4 * workgroups] =
 * {shader cycles (s_memtime), 100 MHz ticks (s_memrealtime), K-tile steps walked, XCC id} per workgroup; the output D is
 * written as usual.  In-kernel clock = cycles / ticks x 100 MHz.
 */
int mi_gemm_fp8_clock(const void* A, const void* B, void* D, const float* sa_inv, const float* sb_inv, int64_t M, int64_t N,
                      int64_t K, int64_t lda, int64_t ldb, int64_t ldd, int algo, unsigned long long* stamps, void* stream);

/*
 * Grouped form of mi_gemm_fp8: up to 4 independent problems D_p = (A_p . B_p^T) * (*sa_inv_p * *sb_inv_p), bf16 outputs, no
 * bias, in ONE persistent launch whose workgroups walk a shared tile list (longest tiles first) -- a Linear's dgrad + wgrad
 * (both consume the same grad_output) pay one ramp and one exposed epilogue, and the short problem's tiles fill
 * the idle part of the long one's last round of tiles.  All problems share fmt_a / fmt_b and the tile shape: tile_cfg
 * 0 = 256x256, 1 = 256x192, 2 = 192x256, 3 = 192x192, 4 = 256x256 on the four-wave kernel (every K_p >= 512), -1 = choose among 0-3 (M_p, N_p must be multiples of the tile, K_p of 256;
 * operands below 2 GiB; at most 64 tiles per workgroup).  Results are bitwise those of mi_gemm_fp8(algo 4) per problem.
 * Each problem has its own leading dimensions and pointers under the rules of mi_gemm_fp8 (lda, ldb >= K, multiples of 16; ldd >= N,
 * multiple of 4; 16-byte aligned A, B, D; M * lda, N * ldb, 2 * M * ldd < 2^31), checked per problem: MI_ERR_ARG names the
 * offending one and nothing is launched.  NaN / Inf bytes and scales propagate as in mi_gemm_fp8 and stay inside their own
 * problem.
 */
typedef struct mi_gemm_problem {
  const void* A;        /* fp8 [M, K], row stride lda */
  const void* B;        /* fp8 [N, K], row stride ldb */
  void* D;              /* bf16 [M, N], row stride ldd */
  const float* sa_inv;  /* device scalars */
  const float* sb_inv;
  int64_t M, N, K, lda, ldb, ldd;
} mi_gemm_problem;
int mi_gemm_fp8_grouped(const mi_gemm_problem* problems, int n, int fmt_a, int fmt_b, int tile_cfg, void* stream);

/*
 * Stream-K workspace for the persistent GEMM, used only by the explicit algo 44: when the 256x256 tile count is not a
 * multiple of the CU count, the (tile, K-tile) steps are cut into equal ranges and a tile split between two workgroups is
 * summed through this buffer (fp32 partial accumulators + one flag per workgroup).  The caller owns the memory: at least
 * mi_gemm_workspace_bytes(), 256-byte aligned, its first 4 KiB zeroed once; it is bound to the CURRENT device until replaced
 * (NULL unregisters) and must only be used by GEMMs of one stream at a time.
 */
int64_t mi_gemm_workspace_bytes(void);
int mi_gemm_set_workspace(void* workspace, int64_t bytes);

/*
 * K7  MXFP8 block quantise  [replaces TE's MXFP8 quantize, row-wise and column-wise].
 *   Row-wise: one E8M0 scale per 32 consecutive elements of a row:
 *     e = roundup_e8m0(amax_blk * (1/fp8_max)); y = sat_cast(x * 2^(127-e))
 *     y_row [rows, cols] fp8, s_row [cols/32, rows] u8 (BLOCK-MAJOR: the scales of one 32-block of every row are contiguous).
 *   Column-wise (blocks of 32 along rows), emitted TRANSPOSED so it is a TN GEMM operand:
 *     y_colT [cols, rows] fp8, s_colT [rows/32, cols] u8 (block-major w.r.t. the transposed operand).
 * Either pair may be NULL.  rows, cols multiples of 32.
 */
int mi_mxfp8_quantize(const void* x_bf16, void* y_row, void* s_row, void* y_colT, void* s_colT,
                      int64_t rows, int64_t cols, int fmt, void* stream);

/*
 * mi_mxfp8_quantize for a tensor that is a ROW-BLOCK of a larger operand (query | key | value weights forming one GEMM
 * operand, te_llama.py:200-217): y_row / s_colT point at the block's first row inside the larger [R_total, cols] buffers
 * (contiguous); s_row / y_colT point at the block's first column and use ld_rows (= R_total, >= rows) as their leading
 * dimension.  colsum (optional): fp32 [ceil(rows/128), cols] partial column sums of x, one row per 128-row tile, for
 * mi_colsum_finish (bias gradient riding on the quantisation of grad_output).
 */
int mi_mxfp8_quantize_ex(const void* x_bf16, void* y_row, void* s_row, void* y_colT, void* s_colT, float* colsum,
                         int64_t rows, int64_t cols, int64_t ld_rows, int fmt, void* stream);
/*
 * K7 fused with the GEMM neighbours (MXFP8 counterparts of K9 / K10; same output layout as mi_mxfp8_quantize):
 *   mi_mxfp8_norm_quantize     quantises (x * rstd[r]) * gamma[c]                      (RMSNorm -> MXFP8)
 *   mi_mxfp8_swiglu_quantize   quantises silu(h[:, :F]) * h[:, F:]                     (outputs have F columns)
 *   mi_mxfp8_dswiglu_quantize  quantises [dact*dsilu(g)*u | dact*silu(g)] ([rows, 2F]) and writes the per-128-row
 *                              column sums (fp32 [ceil(rows/128), 2F], nullable) for the fc1 bias gradient
 */
int mi_mxfp8_norm_quantize(const void* x_bf16, const float* rstd, const void* gamma_bf16, void* y_row, void* s_row,
                           void* y_colT, void* s_colT, int64_t rows, int64_t cols, int fmt, void* stream);
int mi_mxfp8_swiglu_quantize(const void* h_bf16, void* y_row, void* s_row, void* y_colT, void* s_colT, int64_t rows,
                             int64_t F, int fmt, void* stream);
int mi_mxfp8_dswiglu_quantize(const void* h_bf16, const void* dact_bf16, void* y_row, void* s_row, void* y_colT,
                              void* s_colT, float* colsum, int64_t rows, int64_t F, int fmt, void* stream);
/*
 * RoPE backward (mi_rope_qkv, backward = 1) fused with mi_mxfp8_quantize of its result: the MXFP8 grad_output of the q|k|v
 * projection under MXFP8BlockScaling (te_llama_mxfp8.py:28-29,86), straight from the attention gradients dq / dk / dv; the
 * bf16 d(qkv) [rows, W] is never written.  Outputs as mi_mxfp8_quantize for a [rows, W] tensor, W = (n_q + 2 n_kv) * 128;
 * equal to the two-kernel sequence bit for bit.
 */
int mi_mxfp8_rope_bwd_quantize(const void* dq_bf16, const void* dk_bf16, const void* dv_bf16, const float* cos_tab,
                               const float* sin_tab, void* y_row, void* s_row, void* y_colT, void* s_colT, int64_t rows,
                               int64_t seq, int n_q_heads, int n_kv_heads, int head_dim, int fmt, void* stream);

/*
 * Float8BlockScaling quantise (revision 3): the K7 kernel with one POWER-OF-TWO scale per 1 x 128 block along the contraction
 * axis (block_dim 1: 128 consecutive elements of a row for the row-wise copy, of a column for the column-wise one) or per
 * 128 x 128 block (block_dim 2: both copies share the block's scale, so y_colT is the byte transpose of y_row).  Per block B of
 * the fp32 values v the cast sees:
 *     amax  = max |v|                        (fmaxf semantics: a NaN element is ignored, Inf gives Inf)
 *     a     = max(amax, amax_epsilon)
 *     scale = 1 if a is 0 or Inf, else fp8_max / a (IEEE fp32; Inf -> FLT_MAX) with the mantissa cleared   (mi_current_scale, pow2)
 *     y     = sat_cast(v * scale)            (NaN -> the NaN byte, +-Inf and over-range -> +-max)
 *     byte  = 254 - biased_exponent(scale)   (E8M0 of 1 / scale, exactly; 0..247)
 * Outputs in the layout of mi_mxfp8_quantize(_ex), the block's byte stored at EVERY 32-group position the block covers, so that
 * mi_gemm_mxfp8 / mi_gemm_mxfp8_grouped take these operands unchanged.  rows, cols multiples of 32; a trailing block shorter than
 * 128 is a block over the elements that exist.  Blocks start at the tensor's first row and column: with block_dim 2 a row-block
 * destination (ld_rows > rows) must start on a multiple of 128 rows of its operand (the operand's buffers 128-byte aligned).
 * The argument lists are those of the mi_mxfp8_* counterparts plus (block_dim, amax_epsilon >= 0) in front of the stream.
 */
int mi_blockfp8_quantize_ex(const void* x_bf16, void* y_row, void* s_row, void* y_colT, void* s_colT, float* colsum,
                            int64_t rows, int64_t cols, int64_t ld_rows, int fmt, int block_dim, float amax_epsilon, void* stream);
int mi_blockfp8_norm_quantize(const void* x_bf16, const float* rstd, const void* gamma_bf16, void* y_row, void* s_row,
                              void* y_colT, void* s_colT, int64_t rows, int64_t cols, int fmt, int block_dim, float amax_epsilon,
                              void* stream);
int mi_blockfp8_swiglu_quantize(const void* h_bf16, void* y_row, void* s_row, void* y_colT, void* s_colT, int64_t rows,
                                int64_t F, int fmt, int block_dim, float amax_epsilon, void* stream);
int mi_blockfp8_dswiglu_quantize(const void* h_bf16, const void* dact_bf16, void* y_row, void* s_row, void* y_colT,
                                 void* s_colT, float* colsum, int64_t rows, int64_t F, int fmt, int block_dim, float amax_epsilon,
                                 void* stream);

/*
 * K8  block-scaled MXFP8 GEMM (v_mfma_scale_f32_16x16x128_f8f6f4 with per-32 E8M0 scales)
 *   D[m,n] = bf16( sum_blk 2^(sa[m,blk]+sb[n,blk]-254) * sum_{k in blk} A[m,k] B[n,k] + bias[n] )
 * A [M,K] fp8 + SA [K/32, M] u8; B [N,K] fp8 + SB [K/32, N] u8 (block-major, as mi_mxfp8_quantize emits); K multiple of 32.
 * algo: 0 = auto (persistent 256x256 kernel when M,N,K % 256 == 0 and bf16 output; else generic), 1 = generic; 4, 5, 40-45 as in
 * mi_gemm_fp8 (bf16 output, K % 256 == 0).  fmt_a / fmt_b are independent: all four pairs are built (HYBRID backward = E5M2 x E4M3).
 * No leading dimensions: A, B, D and the scale arrays are tight (lda = ldb = K, ldd = N) and 16-byte aligned.
 * A NaN data byte makes its output row / column NaN, as in mi_gemm_fp8.  An E8M0 scale byte of 0xFF is NaN (OCP MX): measured on
 * MI355X, the scaled MFMA turns every output that block feeds into NaN -- the whole row (scale of A) or column (scale of B) -- in
 * every algo alike (1, 4, 5, 41-43, 44), which is what the oracle computes; mi_mxfp8_quantize never emits 0xFF.  A block whose 32
 * data bytes are all zero contributes exactly nothing under any scale byte 0 .. 0xFE: the output bits do not depend on it.
 */
int mi_gemm_mxfp8(const void* A, const void* SA, const void* B, const void* SB, void* D,
                  const void* bias_bf16, int64_t M, int64_t N, int64_t K, int fmt_a, int fmt_b,
                  int out_dtype, int algo, void* stream);

/*
 * Grouped form of mi_gemm_mxfp8 (ABI 5): 1 to 4 independent block-scaled problems, bf16 outputs, no bias, in ONE persistent
 * launch whose workgroups walk a shared tile list, longest tiles first -- what mi_gemm_fp8_grouped is to mi_gemm_fp8: a Linear's
 * MXFP8 dgrad + wgrad pay one ramp and one exposed epilogue, and the short problem's tiles fill the long one's last round.
 * All problems share fmt_a / fmt_b (all four pairs are built: HYBRID backward = E5M2 x E4M3) and the tile shape: tile_cfg
 * 0 = 256x256, 1 = 256x192, 2 = 192x256, 3 = 192x192 (the shapes of mi_gemm_mxfp8 algos 40-43; all four are built), -1 = choose
 * among those that divide every problem.  tile_cfg 4 is MI_ERR_ARG: the four-wave kernel has no block-scaled main loop.
 * Operands as in mi_gemm_mxfp8: tight (lda = ldb = K, ldd = N), scales block-major; A, SA, B, SB, D 16-byte aligned.  Every M_p,
 * N_p a multiple of the tile, every K_p of 256, M K, N K and 2 M N below 2^31, at most 64 tiles per workgroup.
 * Each problem's output is bit for bit what mi_gemm_mxfp8(algo 4) writes for that problem alone, whatever the tile shape (one
 * fp32 summation order per output element).  A NaN data byte or a 0xFF scale byte poisons exactly its row (A side) or column
 * (B side) of its own problem, as documented for mi_gemm_mxfp8; nothing crosses a problem boundary.
 * Everything refused is refused on the host before anything is launched or dereferenced, and mi_last_error() names the
 * offending problem: MI_ERR_ARG for n outside 1..4, a null or misaligned pointer, a bad fmt or tile_cfg; MI_ERR_SHAPE for
 * K % 256 != 0, a shape the tile (or, with -1, any tile) does not divide, an operand of 2 GiB or more, more than 64 tiles per
 * workgroup.
 */
typedef struct mi_gemm_mx_problem {
  const void* A;   /* fp8 [M, K] tight */
  const void* SA;  /* E8M0 [K/32, M] block-major */
  const void* B;   /* fp8 [N, K] tight */
  const void* SB;  /* E8M0 [K/32, N] block-major */
  void* D;         /* bf16 [M, N] tight */
  int64_t M, N, K;
} mi_gemm_mx_problem;
int mi_gemm_mxfp8_grouped(const mi_gemm_mx_problem* problems, int n, int fmt_a, int fmt_b, int tile_cfg, void* stream);

/*
 * RoPE fused with the q/k/v split of the QKV projection output  [TE applies a fused RoPE kernel between
 * layernorm_qkv and the attention core on the reference path, te_llama.py:65-66,77].
 *   forward  (backward = 0): q, k, v <- fused [rows, (nq + 2 nkv) * D]; q, k heads rotated by +theta(row % seq)
 *   backward (backward = 1): fused gradient <- dq, dk, dv with the conjugate rotation
 * out1 = x1 cos - x2 sin, out2 = x2 cos + x1 sin over the two halves of a head (non-interleaved);
 * cos_tab / sin_tab: fp32 [>= seq, D/2]; math in fp32, one bf16 rounding.
 */
int mi_rope_qkv(void* fused_bf16, void* q_bf16, void* k_bf16, void* v_bf16, const float* cos_tab,
                const float* sin_tab, int64_t rows, int64_t seq, int n_q_heads, int n_kv_heads, int head_dim,
                int backward, void* stream);
/*
 * RoPE backward (mi_rope_qkv with backward = 1) fused with mi_cast_amax of its result: dq [rows, n_q*D], dk, dv
 * [rows, n_kv*D] bf16 -> the FP8 copies y [rows, W] / yT [W, rows] (W = (n_q + 2 n_kv) * D) of the fused gradient d(qkv),
 * which is grad_output of the q|k|v projection (te_llama.py:45-56: `layernorm_qkv` feeding the rotary attention core), plus
 * its amax.  The bf16 gradient is never written.  Bytes and amax equal the two-kernel sequence bit for bit.  head_dim 128.
 */
int mi_rope_qkv_bwd_cast(const void* dq_bf16, const void* dk_bf16, const void* dv_bf16, const float* cos_tab, const float* sin_tab,
                         void* y_fp8, void* yT_fp8, const float* scale, float* amax, int64_t rows, int64_t seq, int n_q_heads,
                         int n_kv_heads, int head_dim, int fmt, void* stream);
/*
 * Per-head QK RMSNorm fused into the RoPE split (revision 6; HF Qwen3 `self_attn.q_norm` / `k_norm`, TE MultiheadAttention with
 * qk_norm_type="RMSNorm", qk_norm_before_rope=True).  Layout as mi_rope_qkv: fused bf16 [rows, (n_q + 2 n_kv) * D], q / k / v
 * separate and contiguous, cos_tab / sin_tab fp32 [>= seq, D/2], row r at position r % seq.  head_dim 64 or 128.
 *   mi_qknorm_rope_qkv: per q / k head vector x (bf16 -> fp32): rstd = rsqrt(mean_D(x^2) + eps), n = (x * rstd) * gamma with gamma =
 *     gamma_q / gamma_k (bf16 [D]); then the rotation out1 = n1 cos - n2 sin, out2 = n2 cos + n1 sin.  All arithmetic in fp32, one
 *     round-to-nearest-even to bf16 at the store; v is copied.  rstd_out: fp32 [rows, n_q + n_kv] (q heads first), for backward.
 *   mi_qknorm_rope_qkv_bwd: dn = conjugate rotation of the incoming head gradient (dn1 = d1 cos + d2 sin, dn2 = d2 cos - d1 sin),
 *     g = gamma * dn, xhat = x * rstd (x from fused_x, the forward's input), dx = rstd * (g - xhat * mean_D(g * xhat)) into the
 *     q | k columns of dfused; dv copied into its v columns.  dgamma_partial: fp32 [n_partials, 2 D]; the launch has n_partials
 *     workgroups, workgroup p owns rows [p * ceil(rows / n_partials), ...) and writes row p = the sums of dn * xhat over its rows
 *     and all q heads (columns 0 .. D-1) resp. all k heads (D .. 2D-1), zeros if it owns no row.  Fixed summation order, no
 *     atomics: a given n_partials gives the same bits every run.  The caller finishes with mi_colsum_finish.
 * MI_ERR_ARG before any launch: a null pointer, head_dim outside {64, 128}, rows < 0 or >= 2^31, seq <= 0, head counts < 1,
 * n_partials < 1, a pointer that is not 16-byte aligned, eps negative or not finite.
 */
int mi_qknorm_rope_qkv(const void* fused_bf16, void* q_bf16, void* k_bf16, void* v_bf16, const void* gamma_q_bf16,
                       const void* gamma_k_bf16, float* rstd_out, const float* cos_tab, const float* sin_tab, int64_t rows,
                       int64_t seq, int n_q_heads, int n_kv_heads, int head_dim, float eps, void* stream);
int mi_qknorm_rope_qkv_bwd(const void* dq_bf16, const void* dk_bf16, const void* dv_bf16, const void* fused_x_bf16,
                           const float* rstd, const void* gamma_q_bf16, const void* gamma_k_bf16, const float* cos_tab,
                           const float* sin_tab, void* dfused_bf16, float* dgamma_partial, int n_partials, int64_t rows,
                           int64_t seq, int n_q_heads, int n_kv_heads, int head_dim, void* stream);

/*
 * K10  SwiGLU fused with the FP8 cast of fc2's input  [TE LayerNormMLP activation="swiglu", te_llama.py:58-63].
 *   act[r,c] = silu(h[r,c]) * h[r,F+c] in fp32, c in [0,F);  y = sat_cast(act * *scale), yT its transpose,
 *   *amax = max(*amax, max|act|).  h: bf16 [rows, 2F] (gate | up).  rows, F multiples of 8.
 */
int mi_swiglu_cast(const void* h_bf16, void* y_fp8, void* yT_fp8, const float* scale, float* amax,
                   int64_t rows, int64_t F, int fmt, void* stream);

/*
 * K10 backward: dh = [dact * dsilu(g) * u | dact * silu(g)] in fp32 -> FP8 [rows, 2F] (+ transpose) + amax.
 * colsum (nullable): fp32 [ceil(rows/128), 2F] per-row-block column sums of dh in a fixed order (the caller adds
 * the row blocks to get the fc1 bias gradient bitwise reproducibly).
 */
int mi_dswiglu_cast(const void* h_bf16, const void* dact_bf16, void* y_fp8, void* yT_fp8, const float* scale,
                    float* amax, float* colsum, int64_t rows, int64_t F, int fmt, void* stream);
/* The two SwiGLU kernels with the fc1 bias (bf16 [2F], 16-byte aligned) added to `h` INSIDE the kernel, in fp32, before the
 * activation: `h` is then the fc1 GEMM's output WITHOUT its bias.  TE's bias + activation fusion (LayerNormMLP keeps TE's default
 * bias=True on the reference path, te_llama.py:58-63): the add rides in an HBM-bound kernel instead of in the GEMM epilogue. */
int mi_swiglu_cast_bias(const void* h_bf16, const void* bias_bf16, void* y_fp8, void* yT_fp8, const float* scale, float* amax,
                        int64_t rows, int64_t F, int fmt, void* stream);
int mi_dswiglu_cast_bias(const void* h_bf16, const void* bias_bf16, const void* dact_bf16, void* y_fp8, void* yT_fp8,
                         const float* scale, float* amax, float* colsum, int64_t rows, int64_t F, int fmt, void* stream);

/*
 * K9  RMSNorm fused with the FP8 cast of the following GEMM's input  [TE LayerNormLinear / LayerNormMLP with
 *     normalization="RMSNorm", te_llama.py:45-63: the normalised bf16 activation is never materialised].
 *   mi_rmsnorm_stats: rstd[r] = rsqrt(mean_c x[r,c]^2 + eps)                                   (fp32, one wave per row)
 *   mi_norm_cast:     v = (x[r,c] * rstd[r]) * gamma[c] in fp32; y = sat_cast(v * *scale), yT, *amax = max(*amax, max|v|)
 *   mi_rmsnorm_bwd:   dx = rstd * (dy*gamma - xhat * mean_c(dy*gamma*xhat)) (+ dres), xhat = x*rstd;
 *                     dgamma_partial[b, c] = sum over block b's rows of dy*xhat (fp32, fixed order; caller adds the blocks).
 *                     cols % 512 == 0, cols <= 8192.
 */
int mi_rmsnorm_stats(const void* x_bf16, float* rstd, int64_t rows, int64_t cols, float eps, void* stream);
/* out = a + b (bf16, one rounding of the fp32 sum) and rstd[r] of the rounded sum in one pass: the residual add of a decoder
 * layer (te_llama.py:78,81) fused with the statistics pass of the RMSNorm that consumes it. */
int mi_add_rmsnorm_stats(const void* a_bf16, const void* b_bf16, void* out_bf16, float* rstd, int64_t rows, int64_t cols,
                         float eps, void* stream);
/* mi_add_rmsnorm_stats with a bias (bf16 [cols]) on the second addend: out = a + (b + bias) -- `b` is the fc2 GEMM's output without
 * its bias, which joins the residual add it feeds anyway. */
int mi_add_bias_rmsnorm_stats(const void* a_bf16, const void* b_bf16, const void* bias_bf16, void* out_bf16, float* rstd,
                              int64_t rows, int64_t cols, float eps, void* stream);
int mi_norm_cast(const void* x_bf16, const float* rstd, const void* gamma_bf16, void* y_fp8, void* yT_fp8,
                 const float* scale, float* amax, int64_t rows, int64_t cols, int fmt, void* stream);
int mi_rmsnorm_bwd(const void* dy_bf16, const void* x_bf16, const float* rstd, const void* gamma_bf16,
                   const void* dres_bf16, void* dx_bf16, float* dgamma_partial, int n_partials, int64_t rows,
                   int64_t cols, void* stream);

/*
 * Current scaling (ABI 5 revision 2; TE's Float8CurrentScaling): a tensor is quantised with a scale computed from its OWN amax, so
 * the amax exists before the cast.  An amax pass reads what the matching cast kernel reads and reduces |v|, v being the fp32 value
 * that kernel multiplies by *scale (same device code, so the same bits):
 *   mi_amax_bf16     v of mi_cast_amax:                  x[r,c]
 *   mi_amax_norm     v of mi_norm_cast:                  (x[r,c] * rstd[r]) * gamma[c]
 *   mi_amax_swiglu   v of mi_swiglu_cast(_bias):         silu(g) * u, g | u = h[r,c] | h[r,F+c] (+ bias, fp32, if bias != NULL)
 *   mi_amax_dswiglu  v of mi_dswiglu_cast(_bias):        both halves, dact * dsilu(g) * u and dact * silu(g)
 * The launch has exactly n_partial workgroups (1..1024, the caller's choice) and workgroup i stores partial[i] = max |v| over the
 * elements it walked, 0 if it walked none: all n_partial entries are written, nothing has to be zeroed first and there are no
 * atomics.  NaN elements are ignored, an Inf gives Inf (the cast kernels' own amax).  Shapes and alignment as for the matching cast
 * kernel (rows, cols / F multiples of 8; bf16 inputs, rstd, gamma and bias 16-byte aligned); a violation is MI_ERR_ARG and nothing is
 * launched.  An empty tensor still launches and writes zeros.
 *   mi_current_scale (one workgroup): amax = max_i partial[i]; a = amax < amax_epsilon ? amax_epsilon : amax;
 *     scale = 1 if a == 0 or a is infinite, else fp8_max / a (one IEEE division), FLT_MAX if that is infinite, 1 if it is NaN;
 *     pow2 != 0 clears the scale's mantissa bits (rounds it down to a power of two); out3 = {amax, scale, 1 / scale}.
 *   Several amax passes may fill segments of one partial buffer (query | key | value weights forming one operand) and one
 *   mi_current_scale then covers the whole buffer (n_partial up to 2^20 there).
 * The casts themselves are the kernels above with `scale` = out3 + 1.
 */
int mi_amax_bf16(const void* x_bf16, float* partial, int n_partial, int64_t rows, int64_t cols, void* stream);
int mi_amax_norm(const void* x_bf16, const float* rstd, const void* gamma_bf16, float* partial, int n_partial, int64_t rows,
                 int64_t cols, void* stream);
int mi_amax_swiglu(const void* h_bf16, const void* bias_bf16, float* partial, int n_partial, int64_t rows, int64_t F, void* stream);
int mi_amax_dswiglu(const void* h_bf16, const void* bias_bf16, const void* dact_bf16, float* partial, int n_partial, int64_t rows,
                    int64_t F, void* stream);
int mi_current_scale(const float* partial, int n_partial, float fp8_max, float amax_epsilon, int pow2, float* out3, void* stream);

/*
 * Token cross-entropy on the bf16 logits of the FP8 lm_head (the loss of the reference loop, HF ForCausalLMLoss:
 * mean over tokens whose label != -100; train_fp8.py:278-279 `outputs.loss`), without an fp32 copy of the logits.
 *   mi_ce_forward : lse[r] = log sum_c exp(x[r,c]); loss_rows[r] = lse[r] - x[r, labels[r]] (0 where the label is ignored)
 *   mi_ce_backward: dlogits[r,c] = (exp(x[r,c] - lse[r]) - [c == labels[r]]) * *gscale (0 on ignored rows);
 *                   *gscale = upstream gradient / number of valid tokens (device scalar).  cols % 8 == 0.
 */
int mi_ce_forward(const void* logits_bf16, const int64_t* labels, float* lse, float* loss_rows, int64_t rows,
                  int64_t cols, void* stream);
int mi_ce_backward(const void* logits_bf16, const int64_t* labels, const float* lse, const float* gscale,
                   void* dlogits_bf16, int64_t rows, int64_t cols, void* stream);
/*
 * mi_ce_backward fused with mi_cast_amax of its result: d(logits) leaves as the FP8 copies y [rows, cols] / yT [cols, rows]
 * (+ amax) that the lm_head Linear's backward quantises its grad_output into (train_fp8.py:276-280: `outputs.loss` of the
 * FP8 lm_head); the bf16 d(logits) is never written.  Bytes and amax equal the two-kernel sequence bit for bit.
 */
int mi_ce_backward_cast(const void* logits_bf16, const int64_t* labels, const float* lse, const float* gscale, void* y_fp8,
                        void* yT_fp8, const float* scale, float* amax, int64_t rows, int64_t cols, int fmt, void* stream);

/*
 * Optimiser step of the reference loop (train_fp8.py:288-291: clip_grad_norm_(model.parameters(), 1.0) then
 * AdamW(fused=True).step()), used by llm_fp8_amd.train on the single-GPU path.
 *   mi_sumsq_bf16: partial[b] = sum of g^2 over block b's grid-stride share, b < n_partials (fixed order: reproducible).
 *   mi_adamw_bf16: torch.optim.AdamW update on bf16 p / exp_avg / exp_avg_sq with fp32 math; the gradient is
 *                  multiplied by *grad_scale (device scalar, NULL = 1) -- the clip coefficient, so the gradients are
 *                  not rescaled in a separate pass.  `step` is the 1-based step count for the bias corrections.
 * THE STEP GUARD (ABI 5 revision 5), the same for mi_adamw_bf16 and every mi_adamw_*_multi call below.  A NON-FINITE *grad_scale
 * (NaN, +Inf, -Inf: all exponent bits set) means "skip": the launch behaves as after an update of exactly zero.  p, exp_avg,
 * exp_avg_sq and the fp32 master are not written, not even with their own values; the gradient and the moments are not loaded; no
 * random bits are drawn.  A tensor without an FP8 sink (and every flat chunk) is left alone.  A tensor WITH a sink still gets its
 * copies: a tile loads p only and emits what mi_cast_amax (per-tensor sink: y, yT from the stored weight with the current
 * *scale, its amax published) or mi_mxfp8_quantize (MXFP8 sink: all four buffers) would emit from the stored weight -- the
 * sink may never have been filled, and under delayed scaling *scale has moved since the last emission.  The test is made once per
 * workgroup, on the bits of the value, before anything else is loaded.  NULL and every finite value: the update, as before.
 * A caller makes the decision on the device: a clip coefficient formed from a non-finite gradient norm is sent as NaN.
 */
int mi_sumsq_bf16(const void* g_bf16, int64_t n, float* partial, int n_partials, void* stream);
/*
 * Multi-tensor forms: one launch for every tensor of a parameter group.  table [5, n_tensors] int64 ON THE DEVICE = rows of
 * p / g / exp_avg / exp_avg_sq addresses and element counts; chunks [n_chunks, 2] int32 on the device = (tensor index, chunk
 * index inside the tensor); each workgroup handles one chunk of chunk_elems (multiple of 8) elements.
 * mi_sumsq_bf16_multi writes partial[n_chunks] in FLOAT64 (exact fp32 squares accumulated in fp64: the total is independent of the
 * chunking and of how a caller groups or shards the tensors, to 2^-52); mi_adamw_bf16_multi = mi_adamw_bf16 on every tensor.
 * Non-finite *grad_scale: the step guard above -- the launch returns at once, nothing is read or written.
 */
int mi_sumsq_bf16_multi(const int64_t* table, int n_tensors, const int32_t* chunks, int n_chunks, int chunk_elems,
                        double* partial, void* stream);
int mi_adamw_bf16_multi(const int64_t* table, int n_tensors, const int32_t* chunks, int n_chunks, int chunk_elems,
                        const float* grad_scale, float lr, float beta1, float beta2, float eps, float weight_decay,
                        int64_t step, void* stream);
/*
 * mi_adamw_bf16_multi that ALSO emits the FP8 copies the next forward would cast (K1/K2 folded into the optimiser pass).
 * table: int64 [12, n_tensors]: rows 0-4 as above (p, g, exp_avg, exp_avg_sq, numel), then per tensor
 *   5 cols (0 = no FP8 sink: flat chunks of chunk_elems; > 0: the tensor is a [numel / cols, cols] weight and its chunks are
 *     128 x 128 tiles, chunk index = tile_row * ceil(cols / 128) + tile_col),
 *   6 y (fp8 [rows, ld_y] or 0), 7 yT (fp8 [cols, ld_yT] or 0), 8 ld_y, 9 ld_yT, 10 const float* scale, 11 float* amax (or 0).
 * For a sink tensor every element is updated, rounded to bf16 and stored, and that rounded value is quantised exactly as
 * mi_cast_amax would: y = sat_cast_e4m3(float(bf16) * *scale), *amax = max(*amax, |bf16|) -- bitwise the bytes of a
 * mi_cast_amax call on the updated weight.  rows and cols multiples of 8.
 * Non-finite *grad_scale: the step guard above -- tensors with cols == 0 are left alone; a sink tensor's p, exp_avg and exp_avg_sq
 * are not written, and y / yT / *amax are those of mi_cast_amax on p as it stands, with *scale as it is now.
 */
int mi_adamw_cast_bf16_multi(const int64_t* table, int n_tensors, const int32_t* chunks, int n_chunks, int chunk_elems,
                             const float* grad_scale, float lr, float beta1, float beta2, float eps, float weight_decay,
                             int64_t step, void* stream);
/*
 * The MXFP8 form of mi_adamw_cast_bf16_multi (ABI 3): block scaling has no state, so the copies the next forward would
 * quantise (K7 on every weight: row-wise blocks for fprop, column-wise blocks stored transposed for dgrad) leave with the update.
 * table: int64 [12, n_tensors]: rows 0-5 as above (cols > 0: a [numel / cols, cols] weight walked in 128 x 128 tiles), then
 *   6 y_row (fp8 e4m3 [rows, cols]), 7 s_row (E8M0 [cols/32, ldr]), 8 y_colT (fp8 [cols, ldr]), 9 s_colT (E8M0 [rows/32, cols]),
 *   10 ldr (row count of the operand the tensor is a row-block of: query | key | value form one operand), 11 unused.
 * Rows 6-9 point at the tensor's first row inside the operand's buffers.  Bitwise the bytes of mi_mxfp8_quantize(_ex) on the
 * updated, bf16-rounded weight.  rows and cols multiples of 32; the row offset of a part a multiple of 32.
 * Non-finite *grad_scale: the step guard above -- tensors with cols == 0 are left alone; a sink tensor's p, exp_avg and exp_avg_sq
 * are not written, and y_row / s_row / y_colT / s_colT are those of mi_mxfp8_quantize on p as it stands.
 */
int mi_adamw_mxcast_bf16_multi(const int64_t* table, int n_tensors, const int32_t* chunks, int n_chunks, int chunk_elems,
                               const float* grad_scale, float lr, float beta1, float beta2, float eps, float weight_decay,
                               int64_t step, void* stream);

/*
 * The two calls above with fp32 optimiser state (ABI 5 revision 1): the update is carried by an fp32 MASTER weight and fp32
 * exp_avg / exp_avg_sq, so a step smaller than half a bf16 ulp of the weight is kept instead of rounded away.
 * table: int64 [13, n_tensors].  Rows 0-11 as for mi_adamw_cast_bf16_multi (sink_kind 0) or mi_adamw_mxcast_bf16_multi
 * (sink_kind 1), except that rows 2 and 3 point at FP32 exp_avg / exp_avg_sq and row 0 (p, bf16) is OUTPUT ONLY; row 12 is the
 * fp32 master weight.  Per element: w = master[i]; the AdamW update of the bf16 calls (one formula) runs on w, evaluated in fp64 --
 * fp32 evaluation loses exp_avg where its two terms cancel, which would show in fp32 state -- and master, exp_avg and exp_avg_sq
 * are each rounded once to fp32 and stored; p[i] = RNE_bf16(master[i]); the FP8 copies (y / yT / amax, or y_row / s_row / y_colT / s_colT) are
 * quantised from that ROUNDED bf16 value, exactly as the bf16 calls do -- bitwise the bytes of mi_cast_amax / mi_mxfp8_quantize
 * on the updated p.  Non-finite values follow from the arithmetic.  A tensor with cols == 0 takes the flat chunks (16-byte
 * accesses where p, g and the three fp32 arrays are all 16-byte aligned, element-wise otherwise); a tensor with cols > 0 is walked
 * in 128 x 128 tiles and needs all five arrays 16-byte aligned (the caller sends anything else down the flat chunks).
 * MI_ERR_ARG before any launch: null table / chunks, n_tensors < 1, chunk_elems not a positive multiple of 8, sink_kind outside
 * {0, 1}, step < 1.  n_chunks == 0 is MI_OK (nothing to do).
 * Non-finite *grad_scale, both sink kinds: the step guard above -- master, exp_avg, exp_avg_sq and p are not written; the copies of a
 * sink tensor are quantised from the bf16 p as it stands (the master is not read).
 */
int mi_adamw_f32_multi(const int64_t* table, int n_tensors, const int32_t* chunks, int n_chunks, int chunk_elems,
                       const float* grad_scale, float lr, float beta1, float beta2, float eps, float weight_decay,
                       int64_t step, int sink_kind, void* stream);

/*
 * mi_adamw_cast_bf16_multi (sink_kind 0) / mi_adamw_mxcast_bf16_multi (sink_kind 1) with STOCHASTIC ROUNDING of every bf16 result
 * (ABI 5 revision 4): the same bf16 state, walks and fp32 arithmetic; only the rounding of the updated weight, exp_avg and
 * exp_avg_sq to bf16 differs.  An update below half a bf16 ulp then moves the weight with the matching probability instead of
 * never, and exp_avg_sq decays (beta2 = 0.999 is a relative change below half an ulp: under RNE it does not).
 * Rounding rule, for an fp32 result x with bits b: finite x -> bf16 bits (b + r) >> 16 with r = 16 uniform random bits, i.e. x goes
 * to its upper neighbour (in magnitude) with probability (b & 0xFFFF) / 65536 and a bf16 value never moves; the largest finite
 * magnitudes may become Inf, as under RNE.  NaN and Inf take the RNE conversion of the other calls and use no random bits.
 * Generator: Philox4x32-10 (Salmon et al., SC'11; multipliers D2511F53 / CD9E8D57, key increments 9E3779B9 / BB67AE85), stateless.
 *   key     = (seed & 0xFFFFFFFF, seed >> 32)
 *   counter = (v & 0xFFFFFFFF, v >> 32, step & 0xFFFFFFFF, tensor_key << 2 | stream)
 *   v = e >> 3 for the GLOBAL element index e = table row 12 + the element's index inside the tensor; stream 0 = weight,
 *   1 = exp_avg, 2 = exp_avg_sq.  Element e takes r = bits [16 (j & 1), + 16) of output word j >> 1, j = e & 7: one call per
 *   stream serves 8 consecutive elements.  The bits of an element depend on (seed, step, tensor key, stream, e) and on nothing
 *   else: not on the walk (128 x 128 tile, 8-wide flat vector, element-wise tail), the chunking, the sink, or on whether the
 *   tensor is a whole weight or a row shard of it (row 12 = first row x cols).
 * table: int64 [14, n_tensors].  Rows 0-11 as for mi_adamw_cast_bf16_multi (sink_kind 0) or mi_adamw_mxcast_bf16_multi
 * (sink_kind 1); 12 the global index of the tensor's first element (>= 0; the 8-wide walks need a multiple of 8, which the caller
 * guarantees for tensors with cols > 0 -- a flat tensor with another base is walked element-wise); 13 the tensor key, < 2^30.
 * The FP8 / MXFP8 copies are quantised from the stochastically rounded bf16 weight as stored: bitwise mi_cast_amax /
 * mi_mxfp8_quantize of the updated p.  Alignment rules and refusals as for mi_adamw_f32_multi: MI_ERR_ARG before any launch for a
 * null table / chunks, n_tensors < 1, chunk_elems not a positive multiple of 8, sink_kind outside {0, 1}, step < 1; n_chunks == 0
 * is MI_OK.
 * Non-finite *grad_scale, both sink kinds: the step guard above -- nothing of the state is written and NO random bits are drawn (the
 * stream is counted by `step`, which the caller advances all the same); the copies of a sink tensor are quantised from p as it stands.
 */
int mi_adamw_sr_bf16_multi(const int64_t* table, int n_tensors, const int32_t* chunks, int n_chunks, int chunk_elems,
                           const float* grad_scale, float lr, float beta1, float beta2, float eps, float weight_decay,
                           int64_t step, int sink_kind, uint64_t seed, void* stream);

/*
 * fp32 gradient accumulation over a window of micro-batches (ABI 5 revision 7): ONE launch per micro-batch folds the bf16
 * gradients of every tensor into fp32 window sums, and the last launch of the window rounds each sum to bf16 ONCE.  (Autograd's
 * accumulation into a bf16 `.grad` rounds the running sum to bf16 after every micro-batch but the first.)
 * table: int64 [5, n_tensors] ON THE DEVICE, one column per tensor; chunks [n_chunks, 2] int32 = (tensor, chunk) as for
 * mi_sumsq_bf16_multi, one workgroup per chunk of chunk_elems elements.
 *   0 g     bf16 gradient of this micro-batch; may be 0 in mode 2
 *   1 acc   fp32 window sum
 *   2 numel element count
 *   3 mode  per tensor, may be mixed in one launch:
 *           0 ADD     acc[i] = fl32(acc[i] + float(g[i])); g is not written
 *           1 SET     acc[i] = float(g[i]); acc is not read (starts a window without a zeroing pass); g is not written
 *           2 FINISH  out[i] = RNE_bf16(fl32(acc[i] + float(g[i]))), or RNE_bf16(acc[i]) when g is 0; acc is NOT written: its
 *                     contents are dead afterwards and the next window starts with SET
 *           any other value: the tensor is left alone (the host cannot read a device table).  So is a tensor with acc == 0,
 *           with g == 0 in mode 0 or 1, or with out == 0 in mode 2.
 *   4 out   bf16, mode 2 only; may equal g (each element is read before it is written, by the same lane)
 * Arithmetic: exactly one IEEE fp32 add (round to nearest even) per element and launch, so a window is the micro-batches added
 * in launch order; no FMA, no scaling (a caller's loss / N is already in the gradients).  fp32 denormals are kept, in the sums
 * and in the conversion.  NaN and +-Inf propagate, Inf + (-Inf) = NaN.  The conversion to bf16 is round-to-nearest-even and
 * keeps NaN; an fp32 sum beyond the bf16 range rounds to +-Inf, it does not saturate (the GEMMs' convention for bf16 output).
 * The result is therefore bit for bit a numpy float32 restatement (NaN payloads aside).
 * Accesses: 16 bytes per lane (8 elements: one bf16 load, two fp32 loads, two fp32 stores or one bf16 store) where g, acc and
 * (mode 2) out are 16-byte aligned, element-wise otherwise and on the tail; 64-bit element indices.
 * Bytes moved per element: SET 6, ADD 10, FINISH 8.
 * MI_ERR_ARG before any launch: null table / chunks, n_tensors < 1, n_chunks < 0, chunk_elems not a positive multiple of 8.
 * n_chunks == 0 is MI_OK (nothing to do).
 */
int mi_grad_accum_multi(const int64_t* table, int n_tensors, const int32_t* chunks, int n_chunks, int chunk_elems, void* stream);

/*
 * Embedding weight gradient added in place: grad[id, :] += alpha * sum_{tokens t with ids[t] == id} dY[t, :]   (bf16, fp32
 * sums).  The tied lm_head / embedding table of the reference's Llama models (te_llama.py: `tie_word_embeddings`) already
 * holds the lm_head wgrad when the embedding's backward runs; this replaces a dense [vocab, hidden] scatter + add by a pass
 * over the touched rows.  sorted_ids / perm: the token ids sorted ascending (stable) and the permutation that sorts them
 * (row perm[i] of dY belongs to sorted_ids[i]); ids outside [0, vocab) and padding_idx (-1: none) are skipped.
 * Deterministic (fixed summation order, one writer per row).
 */
int mi_embedding_grad_add(void* grad_bf16, const void* dy_bf16, const int64_t* sorted_ids, const int64_t* perm, int64_t tokens,
                          int64_t hidden, int64_t vocab, float alpha, int64_t padding_idx, void* stream);
/* mi_adamw_bf16 (stated at mi_sumsq_bf16 above).  Non-finite *grad_scale: the step guard -- the launch returns at once. */
int mi_adamw_bf16(void* p_bf16, const void* g_bf16, void* exp_avg_bf16, void* exp_avg_sq_bf16, int64_t n,
                  const float* grad_scale, float lr, float beta1, float beta2, float eps, float weight_decay,
                  int64_t step, void* stream);

/*
 * Attention core of te.pytorch.MultiheadAttention as the reference configures it (te_llama.py:45-56: causal mask type,
 * num_gqa_groups, qkv_format="bshd", attention_dropout 0; TE dispatches to flash-attn, README.md:27-28).  bf16 in/out,
 * fp32 softmax statistics, scores never written to memory.
 *   q, o [B, S, H, D]; k, v [B, S, G, D] (H % G == 0), D contiguous, `*_ts` = token stride in elements (multiple of 8), so
 *   the operands may be column slices of one fused [tokens, (H + 2G) * D] buffer.  D in {64, 128}, S >= 128 and S % 16 == 0
 *   (the reference's collator pads to a multiple of 16; S % 128 != 0 launches the TAIL instantiations, whose last 128-row
 *   block is partial: rows at or past S are neither read nor written).  Every
 *   bf16 pointer (here and in mi_attn_bwd) must be 16-byte aligned; other shapes, strides or alignments are refused.
 *   lse [B, H, S] fp32 = log2-domain log-sum-exp (max * c + log2(sum), c = scale * log2(e)); kept for the backward.
 */
int mi_attn_fwd(const void* q, const void* k, const void* v, void* o, float* lse, int B, int S, int H, int G, int D,
                int64_t q_ts, int64_t k_ts, int64_t v_ts, int64_t o_ts, float scale, int causal, void* stream);
/* What the library launches for one mi_gemm_fp8 / mi_gemm_mxfp8 / mi_gemm_fp8_clock call.  No entry point of this library returns
 * it; the lab library's mi_gemm_plan_diag (below) does.  family 0 = nothing to launch (M or N is 0), 1 = generic, 2 = two-phase,
 * 3 = eight-phase, 4 = persistent eight-wave, 5 = stream-K, 6 = four-wave, one tile per workgroup, 7 = four-wave persistent;
 * build / sched = the kernel's ABL / S template values; mx = block-scaled; tile_cfg as in mi_gemm_fp8_grouped (-1: no tile shape to
 * choose), tiles_m x tiles_n tiles of it (the generic kernel has none and ignores them); bias_use 0 = unused, 1 = added, 2 = a stamp buffer. */
typedef struct mi_gemm_plan {
  int algo, family, build, sched, mx, tile_cfg, tiles_m, tiles_n, grid_x, grid_y, block, one_tile_per_wg, sk_units, bias_use;
} mi_gemm_plan;
#ifdef MI_DIAG
/* LAB BUILD ONLY (-DMI_DIAG).  Timing-only diagnostic build of the forward kernel (causal, D = 128): per wave, shader cycles spent in {S^T MFMAs + K fragment
 * reads, softmax arithmetic, P.V MFMAs + V fragment reads, stage stores incl. the wait for the next tile's loads, barrier};
 * dbg [B, H, S/128, 4 waves, 8] u64 (slot 5 = tiles walked).  Shares only: the stamps forbid overlaps the real kernel has. */
int mi_attn_fwd_diag(const void* q, const void* k, const void* v, void* o, float* lse, unsigned long long* dbg, int B, int S,
                     int H, int G, int D, int64_t q_ts, int64_t k_ts, int64_t v_ts, int64_t o_ts, float scale, void* stream);
/* LAB BUILD ONLY (-DMI_DIAG).  What mi_gemm_fp8 (entry 0), mi_gemm_mxfp8 (1) or mi_gemm_fp8_clock (2) would launch for a call: the
 * shape and leading-dimension checks and every algo / shape refusal of that entry point, with its return code and mi_last_error
 * text, and no launch; it takes no operands.  mi_gemm_mxfp8 passes lda = ldb = K, ldd = N.  On MI_OK `out` holds the plan. */
int mi_gemm_plan_diag(int entry, int64_t M, int64_t N, int64_t K, int64_t lda, int64_t ldb, int64_t ldd, int fmt_a, int fmt_b,
                      int out_dtype, int has_bias, int algo, mi_gemm_plan* out);
#endif
/*
 * Backward of mi_attn_fwd: P is recomputed from q, k and `lse`; two launches (dQ pass, which also writes
 * delta[B, H, S] = rowsum(dO * O), then the dK/dV pass), no sums across workgroups: results are bitwise reproducible.
 * dq [B, S, H, D], dk / dv [B, S, G, D] bf16 with their own token strides (they may be slices of one fused buffer).
 * Shapes as mi_attn_fwd (S >= 128, S % 16 == 0); `delta`, like `lse`, is written for rows below S only.
 */
int mi_attn_bwd(const void* q, const void* k, const void* v, const void* o, const void* dout, const float* lse,
                float* delta, void* dq, void* dk, void* dv, int B, int S, int H, int G, int D, int64_t q_ts,
                int64_t k_ts, int64_t v_ts, int64_t o_ts, int64_t do_ts, int64_t dq_ts, int64_t dk_ts, int64_t dv_ts,
                float scale, int causal, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MI_FP8_H */
