// K7: MXFP8 block quantise -- one E8M0 (power-of-two) scale per 32 consecutive elements along the
// GEMM contraction axis.  Both orientations in ONE pass over the bf16 input (2 B read, 2 B + 2/32 B
// written per element): the row-wise copy (blocks along the last dim) feeds fprop, the column-wise
// copy (blocks along the first dim, emitted transposed) feeds dgrad / wgrad.
// Scales are stored BLOCK-MAJOR ([K/32, rows]: all rows' scales of one 32-block are contiguous): the quantiser
// writes 8 bytes per lane instead of 8 single bytes and the GEMM stages one K-tile's scales of a 256-row tile as
// four 256-byte runs.
// Same tiling as the delayed-scaling cast: 128x128 tile per workgroup, 8x8 block per lane; a
// 32-element block spans 4 neighbouring lanes, reduced with two DPP shuffles.
// Replaces TE's MXFP8 quantise under MXFP8BlockScaling(fp8_format=E4M3)
// (te_llama_mxfp8.py:28-29,86,93; SURVEY.md 2.3 K7, Appendix A "MXFP8").
// The same kernel quantises for Float8BlockScaling (template parameter GRAN below): one power-of-two scale per 1 x 128 or 128 x 128
// block, whose inverse is stored as an E8M0 byte at every 32-block position the block covers -- the layout above, so the MX GEMMs
// read such operands unchanged.
// Host side: ONE argument check (quant_check), ONE launcher (launch_mx) and one body per producer (quant_plain / _norm / _swiglu /
// _dswiglu / _rope_bwd) serve both families; the mi_mxfp8_* and mi_blockfp8_* entry points only say which granularity they mean.
#include "mi_common.h"

namespace mi {

// PRE selects what is quantised (the value block f[8][8] of this lane), so the neighbours of the GEMMs fuse into
// the quantiser exactly as they do on the delayed-scaling path (K9 / K10):
//   0  x[r,c]                                               x: [rows, cols]
//   1  (x[r,c] * rstd[r]) * gamma[c]          (RMSNorm)     x: [rows, cols], aux32 = rstd, aux16 = gamma
//   2  silu(h[r,c]) * h[r,F+c]                (SwiGLU)      x = h: [rows, 2*cols]
//   3  dSwiGLU: [d*dsilu(g)*u | d*silu(g)]                  x = h: [rows, cols] (cols = 2F), aux16 = d: [rows, F];
//      colsum[tile_r, c] = per-128-row column sums (fc1 bias gradient, fixed order)
// The per-element values of 1 .. 3 are those of the delayed-scaling casts: norm_value2, swiglu_value2 and sigmoidf_ (mi_common.h).

// GRAN selects the scaling granularity of the quantise stage; the value block, the producers, the column sums and the NaN handling
// above it are the same code for all three:
//   0  MX: one E8M0 scale per 32 elements (mx_quant_rows / mx_quant_cols, mi_common.h)
//   1  Float8BlockScaling, scaling dim 1: one power-of-two scale per 1 x 128 block along the contraction axis -- a row's 128 columns
//      of the tile for the row-wise copy, a column's 128 rows for the column-wise one (two waves share either)
//   2  Float8BlockScaling, scaling dim 2: one power-of-two scale for the whole 128 x 128 tile, shared by both copies
// GRAN 1 / 2 store the scale-inverse as an E8M0 byte at every 32-group position the block covers, in the MX layout, so the MX GEMMs
// read these operands unchanged.  A trailing block shorter than 128 is a block over the elements that exist (the lanes outside
// the tensor carry zeros).

// one block's scale: TE's compute_scale_from_amax with power-of-two forcing
template <int FMT>
__device__ __forceinline__ float blk_scale(float amax, float eps) { return scale_from_amax(amax, fp8_max_of<FMT>(), eps, true); }
// the E8M0 byte of 1 / scale for a power-of-two scale: 2^(byte - 127) * scale == 1 (0..247, never 0xFF)
__device__ __forceinline__ u32 blk_scale_byte(float scale) { return 254u - ((__float_as_uint(scale) >> 23) & 0xFFu); }

template <int FMT, bool ROWWISE, bool COLWISE, int PRE, int GRAN>
__global__ __launch_bounds__(256) void mxfp8_quant_kernel(const uint16_t* __restrict__ x, const uint16_t* __restrict__ aux16,
                                                          const float* __restrict__ aux32, uint8_t* __restrict__ y_row,
                                                          uint8_t* __restrict__ s_row, uint8_t* __restrict__ y_colT,
                                                          uint8_t* __restrict__ s_colT, float* __restrict__ colsum, int rows,
                                                          int cols, int tiles_c, int ldr, const uint16_t* __restrict__ e0 = nullptr,
                                                          const float* __restrict__ e1 = nullptr, int i0 = 0, int i1 = 0,
                                                          int i2 = 0, float eps = 0.0f) {
  // ldr: leading dimension of s_row / y_colT (= rows, or the row count of a larger operand this tensor is a row-block of)
  __shared__ float s_col[2][128];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int tile_r = blockIdx.x / tiles_c, tile_c = blockIdx.x % tiles_c;
  const int r0 = tile_r * 128 + (wave >> 1) * 64 + (lane >> 3) * 8;
  const int c0 = tile_c * 128 + (wave & 1) * 64 + (lane & 7) * 8;
  const bool active = (r0 < rows) && (c0 < cols);
  float f[8][8];  // values as cast; a NaN is replaced by 0 and recorded in `nanmask` (mx_take_nans, mi_common.h)
  unsigned long long nanmask = 0;
  bool any_nan = false;
  if (PRE == 0) {
    u32 screen = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      v4i raw = {0, 0, 0, 0};
      if (active) raw = *reinterpret_cast<const v4i*>(x + (int64_t)(r0 + i) * cols + c0);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        u32 w = (u32)raw[j];
        screen = nan_screen(screen, w);
        f[i][2 * j] = __uint_as_float(w << 16);
        f[i][2 * j + 1] = __uint_as_float(w & 0xFFFF0000u);
      }
    }
    any_nan = nan_seen(screen);
  } else if (PRE == 1) {
    float gm[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (active) {
      const v4i gv = *reinterpret_cast<const v4i*>(aux16 + c0);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        gm[2 * j] = __uint_as_float((u32)gv[j] << 16);
        gm[2 * j + 1] = __uint_as_float((u32)gv[j] & 0xFFFF0000u);
      }
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      v4i raw = {0, 0, 0, 0};
      float rs = 0.0f;
      if (active) {
        raw = *reinterpret_cast<const v4i*>(x + (int64_t)(r0 + i) * cols + c0);
        rs = aux32[r0 + i];
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) norm_value2((u32)raw[j], rs, gm[2 * j], gm[2 * j + 1], f[i][2 * j], f[i][2 * j + 1]);
    }
    any_nan = true;  // computed values: take the explicit NaN test below
  } else if (PRE == 4) {
    // RoPE backward of the attention gradients, quantised as the fused d(qkv) [rows, W] they merge into (grad_output of the
    // q|k|v projection): x = dq [rows, nq*128], aux16 = dk, e0 = dv [rows, nk*128], aux32 / e1 = cos / sin [seq, 64] fp32,
    // i0 = nq, i1 = nk, i2 = seq; head_dim 128.  Same expressions and bf16 rounding as rope_qkv_kernel<1> (mi_fused.hip), so
    // the result equals mi_rope_qkv(backward) + mi_mxfp8_quantize bit for bit; the bf16 d(qkv) is never written.
    constexpr int HD = 128, HALF = 64;
    const int nq = i0, nk = i1, seq = i2;
    const int hd = c0 / HD, within = c0 % HD;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
#pragma unroll
      for (int j = 0; j < 8; ++j) f[i][j] = 0.0f;
      if (!active) continue;
      const int64_t r = r0 + i;
      if (hd < nq + nk) {
        const uint16_t* src = hd < nq ? x + (r * nq + hd) * HD : aux16 + (r * nk + (hd - nq)) * HD;
        const bool upper = within >= HALF;
        const int cc = upper ? within - HALF : within;
        const v4i a = *reinterpret_cast<const v4i*>(src + cc), b = *reinterpret_cast<const v4i*>(src + HALF + cc);
        const int pos = (int)(r % seq);
        float c[8], sn[8];
        *reinterpret_cast<v4f*>(c) = *reinterpret_cast<const v4f*>(aux32 + (int64_t)pos * HALF + cc);
        *reinterpret_cast<v4f*>(c + 4) = *reinterpret_cast<const v4f*>(aux32 + (int64_t)pos * HALF + cc + 4);
        *reinterpret_cast<v4f*>(sn) = *reinterpret_cast<const v4f*>(e1 + (int64_t)pos * HALF + cc);
        *reinterpret_cast<v4f*>(sn + 4) = *reinterpret_cast<const v4f*>(e1 + (int64_t)pos * HALF + cc + 4);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const u32 wa = (u32)a[j], wb = (u32)b[j];
          const float x1l = __uint_as_float(wa << 16), x1h = __uint_as_float(wa & 0xFFFF0000u);
          const float x2l = __uint_as_float(wb << 16), x2h = __uint_as_float(wb & 0xFFFF0000u);
          const float cl = c[2 * j], ch = c[2 * j + 1], sl = -1.0f * sn[2 * j], sh = -1.0f * sn[2 * j + 1];
          const float ol = upper ? x2l * cl + x1l * sl : x1l * cl - x2l * sl;
          const float oh = upper ? x2h * ch + x1h * sh : x1h * ch - x2h * sh;
          f[i][2 * j] = __uint_as_float(float_to_bf16_bits(ol) << 16);
          f[i][2 * j + 1] = __uint_as_float(float_to_bf16_bits(oh) << 16);
        }
      } else {
        const v4i a = *reinterpret_cast<const v4i*>(e0 + r * (int64_t)(nk * HD) + (c0 - (nq + nk) * HD));
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          f[i][2 * j] = __uint_as_float((u32)a[j] << 16);
          f[i][2 * j + 1] = __uint_as_float((u32)a[j] & 0xFFFF0000u);
        }
      }
    }
    any_nan = true;
  } else {
    const int F = PRE == 2 ? cols : cols / 2;
    const bool up_half = (PRE == 3) && (c0 >= F);
    const int cg = up_half ? c0 - F : c0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      v4i gv = {0, 0, 0, 0}, uv = {0, 0, 0, 0}, dv = {0, 0, 0, 0};
      if (active) {
        const int64_t r = r0 + i;
        gv = *reinterpret_cast<const v4i*>(x + r * 2 * F + cg);
        uv = *reinterpret_cast<const v4i*>(x + r * 2 * F + F + cg);
        if (PRE == 3) dv = *reinterpret_cast<const v4i*>(aux16 + r * F + cg);
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const u32 wg = (u32)gv[j], wu = (u32)uv[j], wd = (u32)dv[j];
        if (PRE == 2) {
          swiglu_value2<0>(wg, wu, wd, false, nullptr, nullptr, &f[i][2 * j], nullptr);
          continue;
        }
        // a lane is in one half of dh: it takes that half's expression of swiglu_value2<1> alone
        const float g2[2] = {__uint_as_float(wg << 16), __uint_as_float(wg & 0xFFFF0000u)};
        const float u2[2] = {__uint_as_float(wu << 16), __uint_as_float(wu & 0xFFFF0000u)};
        const float d2[2] = {__uint_as_float(wd << 16), __uint_as_float(wd & 0xFFFF0000u)};
#pragma unroll
        for (int e = 0; e < 2; ++e) {
          const float sg = sigmoidf_(g2[e]);
          f[i][2 * j + e] = !up_half ? d2[e] * u2[e] * (sg * (1.0f + g2[e] * (1.0f - sg))) : d2[e] * (g2[e] * sg);
        }
      }
    }
    any_nan = true;
  }
  if ((PRE == 3 || PRE == 0) && colsum != nullptr) {  // column sums of the values being quantised (bias gradients)
    float csum[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float v = 0.0f;
#pragma unroll
      for (int i = 0; i < 8; ++i) v += f[i][j];
      v += __shfl_xor(v, 8);
      v += __shfl_xor(v, 16);
      v += __shfl_xor(v, 32);
      csum[j] = v;
    }
    if ((lane >> 3) == 0) {
#pragma unroll
      for (int j = 0; j < 8; ++j) s_col[wave >> 1][(wave & 1) * 64 + (lane & 7) * 8 + j] = csum[j];
    }
    __syncthreads();
    if (tid < 128) {
      const int c = tile_c * 128 + tid;
      if (c < cols) colsum[(int64_t)tile_r * cols + c] = s_col[0][tid] + s_col[1][tid];
    }
  }
  if (__builtin_expect(any_nan, PRE != 0)) nanmask = mx_take_nans(f);  // PRE == 0: only threads whose packed screen saw a NaN come here
  // NOTE: the quantisers' shuffles are executed by every lane (inactive lanes carry zeros); rows/cols are
  // multiples of 32 so a 4-lane block group is all-active or all-inactive.
  u32 lo[8], hi[8], sbytes[8];
  if (GRAN == 0) {
    if (ROWWISE) {
      mx_quant_rows<FMT>(f, nanmask, lo, hi, sbytes);
      if (active) {
        store_rows8<MI_NT_Y>(y_row + (int64_t)r0 * cols + c0, cols, lo, hi);
        // block-major scales [cols/32, rows]: this lane's 8 rows are 8 contiguous bytes
        if ((lane & 3) == 0) store_scales8(s_row + (int64_t)(c0 / 32) * ldr + r0, sbytes);
      }
    }
    if (COLWISE) {
      mx_quant_cols<FMT>(f, nanmask, lo, hi, sbytes);
      if (active) {
        store_cols8<MI_NT_YT>(y_colT + (int64_t)c0 * ldr + r0, ldr, lo, hi);
        // block-major scales [rows/32, cols]: 8 contiguous bytes for this lane's 8 columns
        if (((lane >> 3) & 3) == 0) store_scales8(s_colT + (int64_t)(r0 / 32) * cols + c0, sbytes);
      }
    }
  } else if (GRAN == 1) {
    // 1 x 128 blocks: a row of the tile spans 8 lanes of each of the two waves (wave & 1) that hold its 128 columns, a column the 8
    // row groups of each of the two waves (wave >> 1) that hold its 128 rows.  The partial maxima meet in LDS (entries 0..127: the
    // tile's rows, 128..255: its columns); then every thread turns ONE pair into its block's scale -- one IEEE division per thread
    // instead of one per row and column of every lane -- and the lanes read the scales back.
    __shared__ float s_blk[256][2];
    const int lr = (wave >> 1) * 64 + (lane >> 3) * 8, lc = (wave & 1) * 64 + (lane & 7) * 8;
    if (ROWWISE) {
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        float a = 0.0f;
#pragma unroll
        for (int j = 0; j < 8; ++j) a = fmaxf(a, fabsf(f[i][j]));
        a = fmaxf(a, __shfl_xor(a, 1));
        a = fmaxf(a, __shfl_xor(a, 2));
        a = fmaxf(a, __shfl_xor(a, 4));
        if ((lane & 7) == 0) s_blk[lr + i][wave & 1] = a;
      }
    }
    if (COLWISE) {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        float a = 0.0f;
#pragma unroll
        for (int i = 0; i < 8; ++i) a = fmaxf(a, fabsf(f[i][j]));
        a = fmaxf(a, __shfl_xor(a, 8));
        a = fmaxf(a, __shfl_xor(a, 16));
        a = fmaxf(a, __shfl_xor(a, 32));
        if ((lane >> 3) == 0) s_blk[128 + lc + j][wave >> 1] = a;
      }
    }
    __syncthreads();
    if (tid < 128 ? ROWWISE : COLWISE) s_blk[tid][0] = blk_scale<FMT>(fmaxf(s_blk[tid][0], s_blk[tid][1]), eps);  // (its own pair only)
    __syncthreads();
    if (ROWWISE) {
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const float sc = s_blk[lr + i][0];
        sbytes[i] = blk_scale_byte(sc);
        lo[i] = mx_patch4(cvt4_fp8<FMT>(f[i][0] * sc, f[i][1] * sc, f[i][2] * sc, f[i][3] * sc), nanmask, 8 * i);
        hi[i] = mx_patch4(cvt4_fp8<FMT>(f[i][4] * sc, f[i][5] * sc, f[i][6] * sc, f[i][7] * sc), nanmask, 8 * i + 4);
      }
      if (active) {
        store_rows8<MI_NT_Y>(y_row + (int64_t)r0 * cols + c0, cols, lo, hi);
        // the block's byte at each of its four 32-groups: one lane per group stores it for its 8 rows
        if ((lane & 3) == 0) store_scales8(s_row + (int64_t)(c0 / 32) * ldr + r0, sbytes);
      }
    }
    if (COLWISE) {
      float sc[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        sc[j] = s_blk[128 + lc + j][0];
        sbytes[j] = blk_scale_byte(sc[j]);
      }
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        lo[i] = mx_patch4(cvt4_fp8<FMT>(f[i][0] * sc[0], f[i][1] * sc[1], f[i][2] * sc[2], f[i][3] * sc[3]), nanmask, 8 * i);
        hi[i] = mx_patch4(cvt4_fp8<FMT>(f[i][4] * sc[4], f[i][5] * sc[5], f[i][6] * sc[6], f[i][7] * sc[7]), nanmask, 8 * i + 4);
      }
      if (active) {
        store_cols8<MI_NT_YT>(y_colT + (int64_t)c0 * ldr + r0, ldr, lo, hi);
        if (((lane >> 3) & 3) == 0) store_scales8(s_colT + (int64_t)(r0 / 32) * cols + c0, sbytes);
      }
    }
  } else {
    // 128 x 128 block = the tile: one maximum over the workgroup, one scale, one convert; the transposed store reuses its bytes
    float a = 0.0f;
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
      for (int j = 0; j < 8; ++j) a = fmaxf(a, fabsf(f[i][j]));
    const float sc = blk_scale<FMT>(block_max(a), eps);
    const u32 sb = blk_scale_byte(sc);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      sbytes[i] = sb;
      lo[i] = mx_patch4(cvt4_fp8<FMT>(f[i][0] * sc, f[i][1] * sc, f[i][2] * sc, f[i][3] * sc), nanmask, 8 * i);
      hi[i] = mx_patch4(cvt4_fp8<FMT>(f[i][4] * sc, f[i][5] * sc, f[i][6] * sc, f[i][7] * sc), nanmask, 8 * i + 4);
    }
    if (active) {
      if (ROWWISE) {
        store_rows8<MI_NT_Y>(y_row + (int64_t)r0 * cols + c0, cols, lo, hi);
        if ((lane & 3) == 0) store_scales8(s_row + (int64_t)(c0 / 32) * ldr + r0, sbytes);
      }
      if (COLWISE) {
        store_cols8<MI_NT_YT>(y_colT + (int64_t)c0 * ldr + r0, ldr, lo, hi);
        if (((lane >> 3) & 3) == 0) store_scales8(s_colT + (int64_t)(r0 / 32) * cols + c0, sbytes);
      }
    }
  }
}

// What every entry point below hands on unchanged: its name, the scaling granularity (blk false: MX, gran 0; blk true:
// Float8BlockScaling with gran = block_dim, 1 or 2, and eps = amax_epsilon), the four outputs, the format and the stream.
// (`blk` beside `gran`: a mi_blockfp8_* caller's block_dim arrives unchecked, and its 0 has to be refused by name, not run as MX.)
struct QuantCall {
  const char* who;
  bool blk;
  int gran;
  float eps;
  void *y_row, *s_row, *y_colT, *s_colT;
  int fmt;
  void* stream;
};

// The launch of every producer; the ONE place where the run-time granularity becomes the GRAN template argument.
template <int PRE>
static int launch_mx(const QuantCall& c, const void* x, const void* aux16, const float* aux32, float* colsum, int64_t rows, int64_t cols,
                     int64_t ld_rows = 0, const void* e0 = nullptr, const float* e1 = nullptr, int i0 = 0, int i1 = 0, int i2 = 0) {
  if (rows == 0 || cols == 0) return MI_OK;
  const int ldr = (int)(ld_rows > 0 ? ld_rows : rows);
  const int tiles_r = (int)((rows + 127) / 128), tiles_c = (int)((cols + 127) / 128);
  dim3 grid((unsigned)(tiles_r * tiles_c)), block(256);
#define MI_MX_LAUNCH_(GRAN)                                                                                                        \
  MI_LAUNCH_FMT_YT(c.fmt, c.y_row, c.y_colT, mxfp8_quant_kernel, (), (, PRE, GRAN), grid, block, 0, (hipStream_t)c.stream,          \
                   (const uint16_t*)x, (const uint16_t*)aux16, aux32, (uint8_t*)c.y_row, (uint8_t*)c.s_row, (uint8_t*)c.y_colT,     \
                   (uint8_t*)c.s_colT, colsum, (int)rows, (int)cols, tiles_c, ldr, (const uint16_t*)e0, e1, i0, i1, i2, c.eps)
  if constexpr (PRE == 4) {  // RoPE backward has no block-scaled form (quant_rope_bwd refuses one): MX is its only instantiation
    MI_MX_LAUNCH_(0);
  } else {
    if (c.gran == 0) MI_MX_LAUNCH_(0);
    else if (c.gran == 1) MI_MX_LAUNCH_(1);
    else MI_MX_LAUNCH_(2);
  }
#undef MI_MX_LAUNCH_
  MI_CHECK_LAUNCH(c.blk ? "mi_blockfp8_quantize launch" : "mi_mxfp8_quantize launch");
  return MI_OK;
}

// The argument check of every producer, on the [rows, cols] space that is quantised.
static int quant_check(const QuantCall& c, const void* x, int64_t rows, int64_t cols) {
  const char* who = c.who;
  MI_CHECK_ARG(x, "%s: null input", who);
  MI_CHECK_ARG((c.y_row && c.s_row) || (c.y_colT && c.s_colT), "%s: need (y_row,s_row) and/or (y_colT,s_colT)", who);
  MI_CHECK_ARG((!c.y_row) == (!c.s_row) && (!c.y_colT) == (!c.s_colT), "%s: data and scale pointers must pair up", who);
  MI_CHECK_ARG(rows >= 0 && cols >= 0 && rows % 32 == 0 && cols % 32 == 0,
               "%s: rows (%lld) and cols (%lld) must be multiples of 32", who, (long long)rows, (long long)cols);
  MI_CHECK_ARG(rows < (1LL << 31) && cols < (1LL << 31), "%s: shape too large", who);
  MI_CHECK_ARG(((uintptr_t)x % 16) == 0 && ((uintptr_t)c.y_row % 8) == 0 && ((uintptr_t)c.y_colT % 8) == 0 &&
                   ((uintptr_t)c.s_row % 8) == 0 && ((uintptr_t)c.s_colT % 8) == 0, "%s: misaligned pointer", who);
  MI_CHECK_ARG(c.fmt == MI_FMT_E4M3 || c.fmt == MI_FMT_E5M2, "%s: bad fmt %d", who, c.fmt);
  MI_CHECK_ARG(c.blk ? (c.gran == 1 || c.gran == 2) : c.gran == 0, "%s: block_dim %d must be 1 (1x128 blocks) or 2 (128x128 blocks)", who,
               c.gran);
  MI_CHECK_ARG(c.eps >= 0.0f, "%s: amax_epsilon must be non-negative", who);
  return MI_OK;
}

// ---- one body per producer: its own checks and its launch ----
static int quant_plain(const QuantCall& c, const void* x, float* colsum, int64_t rows, int64_t cols, int64_t ld_rows) {
  int rc = quant_check(c, x, rows, cols);
  if (rc != MI_OK) return rc;
  MI_CHECK_ARG(ld_rows >= rows && ld_rows % 8 == 0 && ld_rows < (1LL << 31), "%s: ld_rows (%lld) must be >= rows and a multiple of 8", c.who,
               (long long)ld_rows);
  // a 128 x 128 block is a tile of THIS call: as a row-block of a larger operand (ld_rows > rows) the tensor has to begin on one of the
  // operand's block rows, or its blocks are not the operand's.  The operand's buffers are at least 128-byte aligned, so the row
  // offset modulo 128 shows in the two pointers that advance by one byte per row.
  MI_CHECK_ARG(c.gran != 2 || ld_rows == rows || (((uintptr_t)c.s_row % 128) == 0 && ((uintptr_t)c.y_colT % 128) == 0),
               "%s: with block_dim 2 a row-block destination must start on a multiple of 128 rows of its operand", c.who);
  return launch_mx<0>(c, x, nullptr, nullptr, colsum, rows, cols, ld_rows);
}

static int quant_norm(const QuantCall& c, const void* x, const float* rstd, const void* gamma, int64_t rows, int64_t cols) {
  int rc = quant_check(c, x, rows, cols);
  if (rc != MI_OK) return rc;
  MI_CHECK_ARG(rstd && gamma && ((uintptr_t)gamma % 16) == 0, "%s: rstd / gamma missing or misaligned", c.who);
  return launch_mx<1>(c, x, gamma, rstd, nullptr, rows, cols);
}

static int quant_swiglu(const QuantCall& c, const void* h, int64_t rows, int64_t F) {
  int rc = quant_check(c, h, rows, F);
  if (rc != MI_OK) return rc;
  return launch_mx<2>(c, h, nullptr, nullptr, nullptr, rows, F);
}

static int quant_dswiglu(const QuantCall& c, const void* h, const void* dact, float* colsum, int64_t rows, int64_t F) {
  int rc = quant_check(c, h, rows, 2 * F);
  if (rc != MI_OK) return rc;
  MI_CHECK_ARG(dact && ((uintptr_t)dact % 16) == 0, "%s: dact missing or misaligned", c.who);
  return launch_mx<3>(c, h, dact, nullptr, colsum, rows, 2 * F);
}

static int quant_rope_bwd(const QuantCall& c, const void* dq, const void* dk, const void* dv, const float* cos_tab, const float* sin_tab,
                          int64_t rows, int64_t seq, int n_q_heads, int n_kv_heads, int head_dim) {
  MI_CHECK_ARG(!c.blk, "%s: RoPE backward has no block-scaled form", c.who);
  MI_CHECK_ARG(head_dim == 128, "%s: head_dim %d not supported (128)", c.who, head_dim);
  MI_CHECK_ARG(n_q_heads >= 1 && n_kv_heads >= 1 && seq >= 1, "%s: bad head counts / seq", c.who);
  const int64_t W = (int64_t)(n_q_heads + 2 * n_kv_heads) * head_dim;
  int rc = quant_check(c, dq, rows, W);
  if (rc != MI_OK) return rc;
  MI_CHECK_ARG(dk && dv && cos_tab && sin_tab && ((uintptr_t)dk % 16) == 0 && ((uintptr_t)dv % 16) == 0 &&
                   ((uintptr_t)cos_tab % 16) == 0 && ((uintptr_t)sin_tab % 16) == 0, "%s: null or misaligned input", c.who);
  return launch_mx<4>(c, dq, dk, cos_tab, nullptr, rows, W, 0, dv, sin_tab, n_q_heads, n_kv_heads, (int)seq);
}

}  // namespace mi

// ---- the C entry points (include/mi_fp8.h): mi_mxfp8_* with one E8M0 scale per 32 elements, mi_blockfp8_* the same producers with
// 1 x 128 (block_dim 1) or 128 x 128 (block_dim 2) power-of-two scales ----
#define MI_MX(name) {name, false, 0, 0.0f, y_row, s_row, y_colT, s_colT, fmt, stream}
#define MI_BLK(name) {name, true, block_dim, amax_epsilon, y_row, s_row, y_colT, s_colT, fmt, stream}

extern "C" int mi_mxfp8_quantize(const void* x_bf16, void* y_row, void* s_row, void* y_colT, void* s_colT,
                                 int64_t rows, int64_t cols, int fmt, void* stream) {
  return mi::quant_plain(MI_MX("mi_mxfp8_quantize"), x_bf16, nullptr, rows, cols, rows);
}

extern "C" int mi_mxfp8_quantize_ex(const void* x_bf16, void* y_row, void* s_row, void* y_colT, void* s_colT, float* colsum,
                                    int64_t rows, int64_t cols, int64_t ld_rows, int fmt, void* stream) {
  return mi::quant_plain(MI_MX("mi_mxfp8_quantize_ex"), x_bf16, colsum, rows, cols, ld_rows);
}

extern "C" int mi_mxfp8_norm_quantize(const void* x_bf16, const float* rstd, const void* gamma_bf16, void* y_row, void* s_row,
                                      void* y_colT, void* s_colT, int64_t rows, int64_t cols, int fmt, void* stream) {
  return mi::quant_norm(MI_MX("mi_mxfp8_norm_quantize"), x_bf16, rstd, gamma_bf16, rows, cols);
}

extern "C" int mi_mxfp8_swiglu_quantize(const void* h_bf16, void* y_row, void* s_row, void* y_colT, void* s_colT, int64_t rows,
                                        int64_t F, int fmt, void* stream) {
  return mi::quant_swiglu(MI_MX("mi_mxfp8_swiglu_quantize"), h_bf16, rows, F);
}

extern "C" int mi_mxfp8_dswiglu_quantize(const void* h_bf16, const void* dact_bf16, void* y_row, void* s_row, void* y_colT,
                                         void* s_colT, float* colsum, int64_t rows, int64_t F, int fmt, void* stream) {
  return mi::quant_dswiglu(MI_MX("mi_mxfp8_dswiglu_quantize"), h_bf16, dact_bf16, colsum, rows, F);
}

extern "C" int mi_mxfp8_rope_bwd_quantize(const void* dq_bf16, const void* dk_bf16, const void* dv_bf16, const float* cos_tab,
                                          const float* sin_tab, void* y_row, void* s_row, void* y_colT, void* s_colT, int64_t rows,
                                          int64_t seq, int n_q_heads, int n_kv_heads, int head_dim, int fmt, void* stream) {
  return mi::quant_rope_bwd(MI_MX("mi_mxfp8_rope_bwd_quantize"), dq_bf16, dk_bf16, dv_bf16, cos_tab, sin_tab, rows, seq, n_q_heads,
                            n_kv_heads, head_dim);
}

extern "C" int mi_blockfp8_quantize_ex(const void* x_bf16, void* y_row, void* s_row, void* y_colT, void* s_colT, float* colsum,
                                       int64_t rows, int64_t cols, int64_t ld_rows, int fmt, int block_dim, float amax_epsilon,
                                       void* stream) {
  return mi::quant_plain(MI_BLK("mi_blockfp8_quantize_ex"), x_bf16, colsum, rows, cols, ld_rows);
}

extern "C" int mi_blockfp8_norm_quantize(const void* x_bf16, const float* rstd, const void* gamma_bf16, void* y_row, void* s_row,
                                         void* y_colT, void* s_colT, int64_t rows, int64_t cols, int fmt, int block_dim,
                                         float amax_epsilon, void* stream) {
  return mi::quant_norm(MI_BLK("mi_blockfp8_norm_quantize"), x_bf16, rstd, gamma_bf16, rows, cols);
}

extern "C" int mi_blockfp8_swiglu_quantize(const void* h_bf16, void* y_row, void* s_row, void* y_colT, void* s_colT, int64_t rows,
                                           int64_t F, int fmt, int block_dim, float amax_epsilon, void* stream) {
  return mi::quant_swiglu(MI_BLK("mi_blockfp8_swiglu_quantize"), h_bf16, rows, F);
}

extern "C" int mi_blockfp8_dswiglu_quantize(const void* h_bf16, const void* dact_bf16, void* y_row, void* s_row, void* y_colT,
                                            void* s_colT, float* colsum, int64_t rows, int64_t F, int fmt, int block_dim,
                                            float amax_epsilon, void* stream) {
  return mi::quant_dswiglu(MI_BLK("mi_blockfp8_dswiglu_quantize"), h_bf16, dact_bf16, colsum, rows, F);
}
