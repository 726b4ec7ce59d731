// LayerNorm fused with the FP8 cast of the following GEMM's input (ABI 5 revision 12): TE's LayerNormLinear / LayerNormMLP with
// normalization="LayerNorm" (their default).  The LayerNorm counterpart of K9 (mi_fused.hip), with a work split of its own: LayerNorm
// models have widths that are no multiple of 512 (768, 1280, 1600, 2560), so every kernel here takes any cols % 8 == 0 and predicates
// the lanes past a row's end off.
//
//   mi_layernorm_stats  mean[r], rstd[r] = rsqrt(var + eps) (biased variance).  One wave per row, the row stays in registers
//                       (NVEC 16-byte vectors per lane, NVEC = 1, 2, 4, 8 or 16: the smallest that covers cols) between the two
//                       reductions: the mean first (per-lane chain, then a butterfly), then sum (x - mean)^2 from the registers.
//                       Two passes, not E[x^2] - mean^2: with a row mean of 64 and a spread of 0.25 the one-pass form subtracts
//                       two numbers near 4096 to get 0.06 and keeps about 8 of fp32's 24 bits; the two-pass form rounds each
//                       x - mean once (relative 2^-24) before it is squared.
//   mi_ln_cast          v = ((x - mean[r]) * rstd[r]) * g[c] + beta[c] (ln_value2, mi_common.h), g = gamma or 1 + gamma;
//                       y = sat_cast(v * *scale), yT, amax.  The persistent walk of norm_cast_kernel: per-wave 64 x 64 tiles, an
//                       8 x 8 block per lane, the next tile's loads (8 rows, gamma and beta slices, 8 means, 8 rstds) in flight.
//   mi_amax_ln          the same kernel body with the stores compiled out (AMAX_ONLY): exactly n_partial workgroups, each stores
//                       its maximum into partial[blockIdx.x]; the value code is shared, so the bits agree with the cast's amax.
//   mi_layernorm_bwd    xhat = (x - mean) * rstd, dyg = dy * g:
//                         dx = rstd * (dyg - mean_c(dyg) - xhat * mean_c(dyg * xhat)) (+ dres)
//                         dgamma_partial[b, c] = sum over block b's rows of dy * xhat,  dbeta_partial[b, c] = sum of dy
//                       WPR waves share a row; each keeps its slice of dy and x in registers between the reductions and the
//                       write, and the two row sums are exchanged through LDS (one barrier per row group).  A wave carries
//                       NV = NVEC / WPR vector steps: 16 NV fp32 column accumulators (twice RMSNorm's) + 4 NV of gamma + 8 NV of
//                       row data + the unpacked gamma the compiler keeps, about 52 NV + 26 VGPRs, so the row is split earlier than
//                       in rmsnorm_bwd_kernel: NV <= 3 up to 6144 columns and 4 only at 8192, which keeps at least two waves per
//                       SIMD and six 16-byte load pairs in flight per SIMD in every instance.  With four waves per row (R = 1)
//                       every column has one owner and the partials go from registers to memory; else the R row slots are added
//                       through LDS in a fixed order.  Instances (hipcc -Rpass-analysis=kernel-resource-usage, gfx950; scratch 0
//                       in every one):
//                         NVEC  cols <=  WPR  NV   VGPRs  waves/SIMD   LDS bytes
//                            1     512    1   1      76       6           8192
//                            2    1024    1   2     130       3          16384
//                            3    1536    1   3     182       2          24576
//                            4    2048    2   2     132       3          16448
//                            6    3072    2   3     184       2          24640
//                            8    4096    4   2     130       3             64
//                           12    6144    4   3     180       2             64
//                           16    8192    4   4     232       2             64
//                       The other kernels, scratch 0 as well: layernorm_stats_kernel<1, 2, 4, 8, 16> 25 / 28 / 58 / 233 / 146 VGPRs,
//                       ln_walk_kernel 172-174 (two waves per SIMD: the grid is two workgroups per CU).
#include "mi_common.h"

namespace mi {

constexpr int kLnMaxCols = 8192;

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

template <int NVEC>
__global__ __launch_bounds__(256) void layernorm_stats_kernel(const uint16_t* __restrict__ x, float* __restrict__ mean,
                                                              float* __restrict__ rstd, int rows, int cols, float eps) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const uint16_t* xr = x + (int64_t)row * cols;
  v4i q[NVEC];
  float acc = 0.0f;
#pragma unroll
  for (int v = 0; v < NVEC; ++v) {
    const int c = v * 512 + lane * 8;
    q[v] = (v4i){0, 0, 0, 0};
    if (c < cols) q[v] = *reinterpret_cast<const v4i*>(xr + c);
#pragma unroll
    for (int j = 0; j < 4; ++j) acc += __uint_as_float((u32)q[v][j] << 16) + __uint_as_float((u32)q[v][j] & 0xFFFF0000u);
  }
  const float mu = wave_sum(acc) / (float)cols;
  acc = 0.0f;
#pragma unroll
  for (int v = 0; v < NVEC; ++v)
    if (v * 512 + lane * 8 < cols) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float a = __uint_as_float((u32)q[v][j] << 16) - mu, b = __uint_as_float((u32)q[v][j] & 0xFFFF0000u) - mu;
        acc += a * a + b * b;
      }
    }
  acc = wave_sum(acc);
  if (lane == 0) {
    mean[row] = mu;
    rstd[row] = rsqrtf(acc / (float)cols + eps);
  }
}

// mi_ln_cast (AMAX_ONLY false) and mi_amax_ln (AMAX_ONLY true: FMT / WRITE_* unused, `partial` written instead of y / yT / amax).
template <int FMT, bool WRITE_Y, bool WRITE_T, bool AMAX_ONLY>
__global__ __launch_bounds__(256) void ln_walk_kernel(const uint16_t* __restrict__ x, const float* __restrict__ mean,
                                                      const float* __restrict__ rstd, const uint16_t* __restrict__ gamma,
                                                      const uint16_t* __restrict__ beta, uint8_t* __restrict__ y,
                                                      uint8_t* __restrict__ yT, const float* __restrict__ scale_p, float* amax_out,
                                                      float* __restrict__ partial, int rows, int cols, int tiles_c, int zero_centered) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ntiles = ((rows + 63) / 64) * tiles_c;
  const int stride = gridDim.x * 4;
  const int lr = (lane >> 3) * 8, lc = (lane & 7) * 8;
  const float scale = AMAX_ONLY ? 1.0f : *scale_p;
  const float gadd = zero_centered ? 1.0f : 0.0f;
  float amax = 0.0f;
  int t = blockIdx.x * 4 + wave;
  v4i nxt[8], nxt_g, nxt_b;
  v4f nxt_r[2], nxt_m[2];
  auto load_tile = [&](int tt, v4i (&raw)[8], v4i& gv, v4i& bv, v4f (&rs)[2], v4f (&mu)[2]) {
    const int r0 = (tt / tiles_c) * 64 + lr, c0 = (tt % tiles_c) * 64 + lc;
    if (r0 < rows && c0 < cols) {  // dims are multiples of 8: blocks are all-in or all-out
      const uint16_t* src = x + (int64_t)r0 * cols + c0;
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const v4i* p = reinterpret_cast<const v4i*>(src + (int64_t)i * cols);
        raw[i] = AMAX_ONLY ? *p : __builtin_nontemporal_load(p);  // the amax pass leaves x on the die for the cast behind it
      }
      gv = *reinterpret_cast<const v4i*>(gamma + c0);
      bv = *reinterpret_cast<const v4i*>(beta + c0);
      rs[0] = *reinterpret_cast<const v4f*>(rstd + r0);
      rs[1] = *reinterpret_cast<const v4f*>(rstd + r0 + 4);
      mu[0] = *reinterpret_cast<const v4f*>(mean + r0);
      mu[1] = *reinterpret_cast<const v4f*>(mean + r0 + 4);
    }
  };
#pragma unroll
  for (int i = 0; i < 8; ++i) nxt[i] = (v4i){0, 0, 0, 0};
  nxt_g = nxt_b = (v4i){0, 0, 0, 0};
  nxt_r[0] = nxt_r[1] = nxt_m[0] = nxt_m[1] = (v4f){0.f, 0.f, 0.f, 0.f};
  if (t < ntiles) load_tile(t, nxt, nxt_g, nxt_b, nxt_r, nxt_m);
  while (t < ntiles) {
    v4i raw[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) raw[i] = nxt[i];
    const v4i gv = nxt_g, bv = nxt_b;
    const v4f rs0 = nxt_r[0], rs1 = nxt_r[1], mu0 = nxt_m[0], mu1 = nxt_m[1];
    const int tn = t + stride;
    if (tn < ntiles) load_tile(tn, nxt, nxt_g, nxt_b, nxt_r, nxt_m);
    const int r0 = (t / tiles_c) * 64 + lr, c0 = (t % tiles_c) * 64 + lc;
    if ((r0 < rows) && (c0 < cols)) {  // (a block outside the tensor holds the previous tile's registers: never looked at)
      float g[8], b[8];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        g[2 * j] = __uint_as_float((u32)gv[j] << 16) + gadd;
        g[2 * j + 1] = __uint_as_float((u32)gv[j] & 0xFFFF0000u) + gadd;
        b[2 * j] = __uint_as_float((u32)bv[j] << 16);
        b[2 * j + 1] = __uint_as_float((u32)bv[j] & 0xFFFF0000u);
      }
      u32 lo[8], hi[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const float rs = i < 4 ? rs0[i & 3] : rs1[i & 3], mu = i < 4 ? mu0[i & 3] : mu1[i & 3];
        float f[8];
#pragma unroll
        for (int j = 0; j < 4; ++j)
          ln_value2((u32)raw[i][j], mu, rs, g[2 * j], g[2 * j + 1], b[2 * j], b[2 * j + 1], f[2 * j], f[2 * j + 1]);
#pragma unroll
        for (int j = 0; j < 8; ++j) amax = fmaxf(amax, (f[j] != f[j]) ? 0.0f : fabsf(f[j]));
        if (!AMAX_ONLY) {
          lo[i] = cvt4_fp8<FMT>(f[0] * scale, f[1] * scale, f[2] * scale, f[3] * scale);
          hi[i] = cvt4_fp8<FMT>(f[4] * scale, f[5] * scale, f[6] * scale, f[7] * scale);
        }
      }
      if (!AMAX_ONLY && WRITE_Y) store_rows8<MI_NT_Y>(y + (int64_t)r0 * cols + c0, cols, lo, hi);
      if (!AMAX_ONLY && WRITE_T) store_cols8<MI_NT_YT>(yT + (int64_t)c0 * rows + r0, rows, lo, hi);
    }
    t = tn;
  }
  if (AMAX_ONLY) {
    amax = block_max(amax);
    if (tid == 0) partial[blockIdx.x] = amax;
  } else {
    publish_amax(amax, amax_out);
  }
}

template <int NVEC, int WPR>
__global__ __launch_bounds__(256) void layernorm_bwd_kernel(const uint16_t* __restrict__ dy, const uint16_t* __restrict__ x,
                                                            const float* __restrict__ mean, const float* __restrict__ rstd,
                                                            const uint16_t* __restrict__ gamma, const uint16_t* __restrict__ dres,
                                                            uint16_t* __restrict__ dx, float* __restrict__ dgp,
                                                            float* __restrict__ dbp, int rows, int cols, int rows_per_block,
                                                            int zero_centered) {
  static_assert(NVEC % WPR == 0 && (WPR == 1 || WPR == 2 || WPR == 4), "row split");
  constexpr int NV = NVEC / WPR, R = 4 / WPR;
  __shared__ float s_acc[R > 1 ? R * NVEC * 512 : 1];  // the R row slots' column accumulators, dgamma then dbeta
  __shared__ float s_red[2][4][2];                     // [parity][wave]: per-wave parts of the two row sums of the rows in flight
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int slot = wave / WPR, part = wave % WPR;
  const int col0 = part * NV * 512 + lane * 8;
  const float gadd = zero_centered ? 1.0f : 0.0f;
  v4i gq[NV];  // gamma, packed bf16
  float dgacc[NV][8], dbacc[NV][8];
#pragma unroll
  for (int v = 0; v < NV; ++v) {
    gq[v] = (v4i){0, 0, 0, 0};
    if (col0 + v * 512 < cols) gq[v] = *reinterpret_cast<const v4i*>(gamma + col0 + v * 512);
#pragma unroll
    for (int j = 0; j < 8; ++j) dgacc[v][j] = dbacc[v][j] = 0.0f;
  }
  const int row_begin = blockIdx.x * rows_per_block;
  const int row_end = min(rows, row_begin + rows_per_block);
  const int iters = (row_end - row_begin + R - 1) / R;  // the same for every wave of the block: the loop holds a barrier
  for (int it = 0; it < iters; ++it) {
    const int row = row_begin + it * R + slot;
    const bool valid = row < row_end;
    const float rs = valid ? rstd[row] : 0.0f, mu = valid ? mean[row] : 0.0f;
    v4i dq[NV], xq[NV];
    float s1 = 0.0f, s2 = 0.0f;  // sum dyg, sum dyg * xhat
#pragma unroll
    for (int v = 0; v < NV; ++v) {
      dq[v] = (v4i){0, 0, 0, 0};
      xq[v] = (v4i){0, 0, 0, 0};
      const bool on = valid && col0 + v * 512 < cols;  // a lane past the row's end adds zeros (dy = 0) everywhere below
      if (on) {
        const int64_t off = (int64_t)row * cols + col0 + v * 512;
        dq[v] = *reinterpret_cast<const v4i*>(dy + off);
        xq[v] = *reinterpret_cast<const v4i*>(x + off);
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float d0 = __uint_as_float((u32)dq[v][j] << 16), d1 = __uint_as_float((u32)dq[v][j] & 0xFFFF0000u);
        const float x0 = (__uint_as_float((u32)xq[v][j] << 16) - mu) * rs, x1 = (__uint_as_float((u32)xq[v][j] & 0xFFFF0000u) - mu) * rs;
        const float g0 = __uint_as_float((u32)gq[v][j] << 16) + gadd, g1 = __uint_as_float((u32)gq[v][j] & 0xFFFF0000u) + gadd;
        dgacc[v][2 * j] += d0 * x0;
        dgacc[v][2 * j + 1] += d1 * x1;
        dbacc[v][2 * j] += d0;
        dbacc[v][2 * j + 1] += d1;
        s1 += d0 * g0 + d1 * g1;
        s2 += (d0 * g0) * x0 + (d1 * g1) * x1;
      }
    }
    s1 = wave_sum(s1);
    s2 = wave_sum(s2);
    if (WPR > 1) {
      if (lane == 0) {
        s_red[it & 1][wave][0] = s1;
        s_red[it & 1][wave][1] = s2;
      }
      __syncthreads();
      s1 = s_red[it & 1][slot * WPR][0];
      s2 = s_red[it & 1][slot * WPR][1];
#pragma unroll
      for (int q = 1; q < WPR; ++q) {  // fixed order: every wave of the row gets the same sums
        s1 += s_red[it & 1][slot * WPR + q][0];
        s2 += s_red[it & 1][slot * WPR + q][1];
      }
    }
    const float m1 = s1 / (float)cols, m2 = s2 / (float)cols;
#pragma unroll
    for (int v = 0; v < NV; ++v)
      if (valid && col0 + v * 512 < cols) {
        const int64_t off = (int64_t)row * cols + col0 + v * 512;
        v4i rv = {0, 0, 0, 0};
        if (dres) rv = *reinterpret_cast<const v4i*>(dres + off);
        v4i ov;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float d0 = __uint_as_float((u32)dq[v][j] << 16), d1 = __uint_as_float((u32)dq[v][j] & 0xFFFF0000u);
          const float x0 = (__uint_as_float((u32)xq[v][j] << 16) - mu) * rs, x1 = (__uint_as_float((u32)xq[v][j] & 0xFFFF0000u) - mu) * rs;
          const float g0 = __uint_as_float((u32)gq[v][j] << 16) + gadd, g1 = __uint_as_float((u32)gq[v][j] & 0xFFFF0000u) + gadd;
          float o0 = rs * ((d0 * g0 - m1) - x0 * m2), o1 = rs * ((d1 * g1 - m1) - x1 * m2);
          if (dres) {
            o0 += __uint_as_float((u32)rv[j] << 16);
            o1 += __uint_as_float((u32)rv[j] & 0xFFFF0000u);
          }
          ov[j] = (int)pack_bf16x2(o0, o1);
        }
        *reinterpret_cast<v4i*>(dx + off) = ov;
      }
  }
  // the block's partials (fixed order).  R == 1: every column has one owning lane, registers -> memory.
  float* const outs[2] = {dgp + (int64_t)blockIdx.x * cols, dbp + (int64_t)blockIdx.x * cols};
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    float(&acc)[NV][8] = k == 0 ? dgacc : dbacc;
    if (R == 1) {
#pragma unroll
      for (int v = 0; v < NV; ++v)
        if (col0 + v * 512 < cols) {
          *reinterpret_cast<v4f*>(outs[k] + col0 + v * 512) = (v4f){acc[v][0], acc[v][1], acc[v][2], acc[v][3]};
          *reinterpret_cast<v4f*>(outs[k] + col0 + v * 512 + 4) = (v4f){acc[v][4], acc[v][5], acc[v][6], acc[v][7]};
        }
    } else {
      if (k == 1) __syncthreads();  // the dgamma sums have been read
#pragma unroll
      for (int v = 0; v < NV; ++v)
#pragma unroll
        for (int j = 0; j < 8; ++j) s_acc[slot * (NVEC * 512) + col0 + v * 512 + j] = acc[v][j];
      __syncthreads();
      for (int c = threadIdx.x; c < cols; c += 256) {
        float a = s_acc[c];
#pragma unroll
        for (int q = 1; q < R; ++q) a += s_acc[q * (NVEC * 512) + c];
        outs[k][c] = a;
      }
    }
  }
}

static bool aligned16(const void* p) { return ((uintptr_t)p % 16) == 0; }

}  // namespace mi

extern "C" int mi_layernorm_stats(const void* x_bf16, float* mean, float* rstd, int64_t rows, int64_t cols, float eps, void* stream) {
  MI_CHECK_ARG(x_bf16 && mean && rstd, "mi_layernorm_stats: null pointer");
  MI_CHECK_ARG(rows >= 0 && rows < (1LL << 31) && cols > 0 && cols % 8 == 0 && cols <= mi::kLnMaxCols,
               "mi_layernorm_stats: cols must be a multiple of 8, at most %d", mi::kLnMaxCols);
  MI_CHECK_ARG(mi::aligned16(x_bf16) && mi::aligned16(mean) && mi::aligned16(rstd), "mi_layernorm_stats: pointers must be 16-byte aligned");
  if (rows == 0) return MI_OK;
  const int steps = (int)((cols + 511) / 512);
#define MI_LS(NV)                                                                                                            \
  hipLaunchKernelGGL((mi::layernorm_stats_kernel<NV>), dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream, \
                     (const uint16_t*)x_bf16, mean, rstd, (int)rows, (int)cols, eps)
  if (steps <= 1) MI_LS(1);
  else if (steps <= 2) MI_LS(2);
  else if (steps <= 4) MI_LS(4);
  else if (steps <= 8) MI_LS(8);
  else MI_LS(16);
#undef MI_LS
  MI_CHECK_LAUNCH("mi_layernorm_stats launch");
  return MI_OK;
}

// what mi_ln_cast and mi_amax_ln ask of their common arguments, under the caller's name
static int ln_walk_check(const char* who, const void* x, const float* mean, const float* rstd, const void* gamma, const void* beta,
                         int64_t rows, int64_t cols) {
  MI_CHECK_ARG(x && mean && rstd && gamma && beta, "%s: null input", who);
  MI_CHECK_ARG(rows >= 0 && cols >= 0 && rows % 8 == 0 && cols % 8 == 0, "%s: rows (%lld) and cols (%lld) must be multiples of 8", who,
               (long long)rows, (long long)cols);
  MI_CHECK_ARG(rows < (1LL << 31) && cols < (1LL << 31) && ((rows + 63) / 64) * ((cols + 63) / 64) < (1LL << 31) - 4 * 1024,
               "%s: shape too large", who);
  MI_CHECK_ARG(mi::aligned16(x) && mi::aligned16(mean) && mi::aligned16(rstd) && mi::aligned16(gamma) && mi::aligned16(beta),
               "%s: misaligned pointer (inputs must be 16-byte aligned)", who);
  return MI_OK;
}

extern "C" int mi_ln_cast(const void* x_bf16, const float* mean, const float* rstd, const void* gamma_bf16, const void* beta_bf16,
                          void* y_fp8, void* yT_fp8, const float* scale, float* amax, int64_t rows, int64_t cols, int zero_centered,
                          int fmt, void* stream) {
  int rc = ln_walk_check("mi_ln_cast", x_bf16, mean, rstd, gamma_bf16, beta_bf16, rows, cols);
  if (rc != MI_OK) return rc;
  MI_CHECK_ARG(scale, "mi_ln_cast: null input");
  MI_CHECK_ARG(y_fp8 || yT_fp8, "mi_ln_cast: at least one of y, yT must be non-null");
  MI_CHECK_ARG(((uintptr_t)y_fp8 % 8) == 0 && ((uintptr_t)yT_fp8 % 8) == 0, "mi_ln_cast: misaligned pointer (y, yT must be 8-byte aligned)");
  MI_CHECK_ARG(fmt == MI_FMT_E4M3 || fmt == MI_FMT_E5M2, "mi_ln_cast: bad fmt %d", fmt);
  if (rows == 0 || cols == 0) return MI_OK;
  const int tiles_r = (int)((rows + 63) / 64), tiles_c = (int)((cols + 63) / 64);  // 64 x 64 tiles, one per wave and step
  const int64_t wgs = ((int64_t)tiles_r * tiles_c + 3) / 4;
  int ncu = 256, devid = 0;
  if (hipGetDevice(&devid) != hipSuccess || hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, devid) != hipSuccess || ncu <= 0) ncu = 256;
  const int64_t cap = (int64_t)ncu * 2;  // two workgroups per CU, as mi_norm_cast
  dim3 grid((unsigned)(wgs < cap ? wgs : cap)), block(256);
  MI_LAUNCH_FMT_YT(fmt, y_fp8, yT_fp8, mi::ln_walk_kernel, (), (, false), grid, block, 0, (hipStream_t)stream, (const uint16_t*)x_bf16,
                   mean, rstd, (const uint16_t*)gamma_bf16, (const uint16_t*)beta_bf16, (uint8_t*)y_fp8, (uint8_t*)yT_fp8, scale, amax,
                   (float*)nullptr, (int)rows, (int)cols, tiles_c, zero_centered);
  MI_CHECK_LAUNCH("mi_ln_cast launch");
  return MI_OK;
}

// (an empty tensor still launches: every one of the n_partial entries is written, with 0)
extern "C" int mi_amax_ln(const void* x_bf16, const float* mean, const float* rstd, const void* gamma_bf16, const void* beta_bf16,
                          float* partial, int n_partial, int64_t rows, int64_t cols, int zero_centered, void* stream) {
  int rc = ln_walk_check("mi_amax_ln", x_bf16, mean, rstd, gamma_bf16, beta_bf16, rows, cols);
  if (rc != MI_OK) return rc;
  MI_CHECK_ARG(partial && ((uintptr_t)partial % 4) == 0, "mi_amax_ln: partial must be non-null and 4-byte aligned");
  MI_CHECK_ARG(n_partial >= 1 && n_partial <= 1024, "mi_amax_ln: n_partial %d outside 1..1024", n_partial);
  const int tiles_c = (int)((cols + 63) / 64);
  hipLaunchKernelGGL((mi::ln_walk_kernel<MI_FMT_E4M3, false, false, true>), dim3((unsigned)n_partial), dim3(256), 0, (hipStream_t)stream,
                     (const uint16_t*)x_bf16, mean, rstd, (const uint16_t*)gamma_bf16, (const uint16_t*)beta_bf16, (uint8_t*)nullptr,
                     (uint8_t*)nullptr, (const float*)nullptr, (float*)nullptr, partial, (int)rows, (int)cols, tiles_c < 1 ? 1 : tiles_c,
                     zero_centered);
  MI_CHECK_LAUNCH("mi_amax_ln launch");
  return MI_OK;
}

extern "C" int mi_layernorm_bwd(const void* dy_bf16, const void* x_bf16, const float* mean, const float* rstd, const void* gamma_bf16,
                                const void* dres_bf16, void* dx_bf16, float* dgamma_partial, float* dbeta_partial, int n_partials,
                                int64_t rows, int64_t cols, int zero_centered, void* stream) {
  MI_CHECK_ARG(dy_bf16 && x_bf16 && mean && rstd && gamma_bf16 && dx_bf16 && dgamma_partial && dbeta_partial,
               "mi_layernorm_bwd: null pointer");
  MI_CHECK_ARG(rows >= 0 && rows < (1LL << 31) && cols > 0 && cols % 8 == 0 && cols <= mi::kLnMaxCols,
               "mi_layernorm_bwd: cols must be a multiple of 8, at most %d", mi::kLnMaxCols);
  MI_CHECK_ARG(n_partials >= 1, "mi_layernorm_bwd: bad sizes");
  MI_CHECK_ARG(mi::aligned16(dy_bf16) && mi::aligned16(x_bf16) && mi::aligned16(mean) && mi::aligned16(rstd) &&
                   mi::aligned16(gamma_bf16) && mi::aligned16(dres_bf16) &&
                   mi::aligned16(dx_bf16) && mi::aligned16(dgamma_partial) && mi::aligned16(dbeta_partial),
               "mi_layernorm_bwd: misaligned pointer");
  const int rows_per_block = (int)((rows + n_partials - 1) / n_partials);
  const int rpb = rows_per_block < 1 ? 1 : rows_per_block;
  const int steps = (int)((cols + 511) / 512);
#define MI_LNB(NV, WPRv)                                                                                                      \
  hipLaunchKernelGGL((mi::layernorm_bwd_kernel<NV, WPRv>), dim3(n_partials), dim3(256), 0, (hipStream_t)stream,               \
                     (const uint16_t*)dy_bf16, (const uint16_t*)x_bf16, mean, rstd, (const uint16_t*)gamma_bf16,              \
                     (const uint16_t*)dres_bf16, (uint16_t*)dx_bf16, dgamma_partial, dbeta_partial, (int)rows, (int)cols, rpb, \
                     zero_centered)
  // the smallest instance that covers cols (the table in this file's header)
  if (steps <= 1) MI_LNB(1, 1);
  else if (steps <= 2) MI_LNB(2, 1);
  else if (steps <= 3) MI_LNB(3, 1);
  else if (steps <= 4) MI_LNB(4, 2);
  else if (steps <= 6) MI_LNB(6, 2);
  else if (steps <= 8) MI_LNB(8, 4);
  else if (steps <= 12) MI_LNB(12, 4);
  else MI_LNB(16, 4);
#undef MI_LNB
  MI_CHECK_LAUNCH("mi_layernorm_bwd launch");
  return MI_OK;
}
