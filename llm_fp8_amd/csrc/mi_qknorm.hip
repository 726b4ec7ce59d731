// Per-head QK RMSNorm fused into the RoPE split (Qwen3: HF `self_attn.q_norm` / `k_norm`; TE `MultiheadAttention(qk_norm_type=
// "RMSNorm", qk_norm_before_rope=True)`):
//   mi_qknorm_rope_qkv      fwd: mi_rope_qkv's split with every q / k head normalised over head_dim before the rotation
//   mi_qknorm_rope_qkv_bwd  bwd: conjugate rotation, RMSNorm backward per head, merge into d(qkv); gamma partials per block
// The item decomposition is mi_rope_qkv's (mi_fused.hip): one lane holds 8 elements of x1 and the matching 8 of x2 of a head, so the
// rotation is lane-local; a head is a group of D/16 consecutive lanes (8 for D = 128, 4 for D = 64) and the two per-head sums are
// __shfl_xor butterflies with offsets below the group size.  Items per row = (nq + 3 nk) * D/16, a multiple of the group size, and
// so are the block size and every stride: a group is entirely inside or entirely outside a loop bound and the rotate / copy
// branch, and no shuffle ever crosses a group.
#include "mi_common.h"

#include <math.h>

namespace mi {

// 8 bf16 (packed in a v4i) -> fp32
__device__ __forceinline__ void qkn_unpack8(const v4i p, float* __restrict__ f) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    f[2 * j] = __uint_as_float((u32)p[j] << 16);
    f[2 * j + 1] = __uint_as_float((u32)p[j] & 0xFFFF0000u);
  }
}

__device__ __forceinline__ void qkn_load8f(const float* __restrict__ p, float* __restrict__ f) {
  *reinterpret_cast<v4f*>(f) = *reinterpret_cast<const v4f*>(p);
  *reinterpret_cast<v4f*>(f + 4) = *reinterpret_cast<const v4f*>(p + 4);
}

// sum over the G lanes of a head group (G = 4 or 8, a power of two; the group is aligned to G inside the wave)
template <int G>
__device__ __forceinline__ float qkn_group_sum(float v) {
#pragma unroll
  for (int o = 1; o < G; o <<= 1) v += __shfl_xor(v, o);
  return v;
}

// fused: [rows, W] bf16, columns q (nq heads) | k (nk heads) | v (nk heads).  q, k, v: separate contiguous outputs.
// Per q / k head x: rstd = rsqrt(mean_D(x^2) + eps), n = (x * rstd) * gamma, out1 = n1 c - n2 s, out2 = n2 c + n1 s; v copied.
// rstd_out [rows, nq + nk] fp32.  Row r has position r % seq.
template <int D>
__global__ __launch_bounds__(256) void qknorm_rope_fwd_kernel(const uint16_t* __restrict__ fused, uint16_t* __restrict__ q,
                                                              uint16_t* __restrict__ k, uint16_t* __restrict__ v,
                                                              const uint16_t* __restrict__ gq, const uint16_t* __restrict__ gk,
                                                              float* __restrict__ rstd_out, const float* __restrict__ cosT,
                                                              const float* __restrict__ sinT, int rows, int seq, int nq, int nk,
                                                              float eps) {
  constexpr int half = D >> 1;
  constexpr int vph = half >> 3;  // lanes per head
  const int W = (nq + 2 * nk) * D;
  const int rot_items = (nq + nk) * vph;
  const int per_row = rot_items + 2 * nk * vph;
  const int64_t items = (int64_t)rows * per_row;
  for (int64_t it = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; it < items; it += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = it / per_row;
    const int w = (int)(it - r * per_row);
    const uint16_t* frow = fused + r * W;
    if (w < rot_items) {
      const int hd = w / vph, vv = w - hd * vph;
      const bool isq = hd < nq;
      uint16_t* sep = isq ? q + (r * nq + hd) * D : k + (r * nk + (hd - nq)) * D;
      const uint16_t* f1 = frow + hd * D + vv * 8;
      const uint16_t* gam = (isq ? gq : gk) + vv * 8;
      float x1[8], x2[8], g1[8], g2[8], c[8], sn[8];
      qkn_unpack8(*reinterpret_cast<const v4i*>(f1), x1);
      qkn_unpack8(*reinterpret_cast<const v4i*>(f1 + half), x2);
      qkn_unpack8(*reinterpret_cast<const v4i*>(gam), g1);
      qkn_unpack8(*reinterpret_cast<const v4i*>(gam + half), g2);
      const int pos = (int)(r % seq);
      qkn_load8f(cosT + (int64_t)pos * half + vv * 8, c);
      qkn_load8f(sinT + (int64_t)pos * half + vv * 8, sn);
      float ss = 0.0f;
#pragma unroll
      for (int j = 0; j < 8; ++j) ss += x1[j] * x1[j];
#pragma unroll
      for (int j = 0; j < 8; ++j) ss += x2[j] * x2[j];
      ss = qkn_group_sum<vph>(ss);
      const float rs = rsqrtf(ss * (1.0f / (float)D) + eps);
      if (vv == 0) rstd_out[r * (nq + nk) + hd] = rs;
      v4i o1, o2;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float a0 = (x1[2 * j] * rs) * g1[2 * j], a1 = (x1[2 * j + 1] * rs) * g1[2 * j + 1];
        const float b0 = (x2[2 * j] * rs) * g2[2 * j], b1 = (x2[2 * j + 1] * rs) * g2[2 * j + 1];
        o1[j] = (int)pack_bf16x2(a0 * c[2 * j] - b0 * sn[2 * j], a1 * c[2 * j + 1] - b1 * sn[2 * j + 1]);
        o2[j] = (int)pack_bf16x2(b0 * c[2 * j] + a0 * sn[2 * j], b1 * c[2 * j + 1] + a1 * sn[2 * j + 1]);
      }
      *reinterpret_cast<v4i*>(sep + vv * 8) = o1;
      *reinterpret_cast<v4i*>(sep + vv * 8 + half) = o2;
    } else {
      const int cv = w - rot_items;
      *reinterpret_cast<v4i*>(v + r * (int64_t)(nk * D) + cv * 8) = *reinterpret_cast<const v4i*>(frow + (nq + nk) * D + cv * 8);
    }
  }
}

// Backward.  Workgroup p owns rows [p * rows_per_block, min(rows, (p + 1) * rows_per_block)) and writes row p of dgp [gridDim.x, 2 D]:
// the sums of dn * xhat over its rows and all q heads (columns 0..D-1) resp. all k heads (D..2D-1).  A lane's columns never change
// (every stride is a multiple of the group size), so it sums its own items in walking order; then a butterfly over the wave's groups,
// the four waves through LDS in wave order: one fixed order, no atomics.
template <int D>
__global__ __launch_bounds__(256) void qknorm_rope_bwd_kernel(const uint16_t* __restrict__ dq, const uint16_t* __restrict__ dk,
                                                              const uint16_t* __restrict__ dv, const uint16_t* __restrict__ fx,
                                                              const float* __restrict__ rstd, const uint16_t* __restrict__ gq,
                                                              const uint16_t* __restrict__ gk, const float* __restrict__ cosT,
                                                              const float* __restrict__ sinT, uint16_t* __restrict__ dfused,
                                                              float* __restrict__ dgp, int rows, int rows_per_block, int seq, int nq,
                                                              int nk) {
  constexpr int half = D >> 1;
  constexpr int vph = half >> 3;
  __shared__ float s_dg[4][2 * D];
  const int W = (nq + 2 * nk) * D;
  const int rot_items = (nq + nk) * vph;
  const int per_row = rot_items + 2 * nk * vph;
  const int64_t row_begin = (int64_t)blockIdx.x * rows_per_block;
  const int64_t row_end = row_begin + rows_per_block < rows ? row_begin + rows_per_block : rows;
  const int64_t items = row_end > row_begin ? (row_end - row_begin) * per_row : 0;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int vv = threadIdx.x % vph;  // = w % vph of every item this lane walks
  float gqf[16], gkf[16];            // gamma_q / gamma_k at this lane's 16 columns
  qkn_unpack8(*reinterpret_cast<const v4i*>(gq + vv * 8), gqf);
  qkn_unpack8(*reinterpret_cast<const v4i*>(gq + vv * 8 + half), gqf + 8);
  qkn_unpack8(*reinterpret_cast<const v4i*>(gk + vv * 8), gkf);
  qkn_unpack8(*reinterpret_cast<const v4i*>(gk + vv * 8 + half), gkf + 8);
  float accq[16], acck[16];
#pragma unroll
  for (int j = 0; j < 16; ++j) accq[j] = acck[j] = 0.0f;
  for (int64_t it = threadIdx.x; it < items; it += 256) {
    const int64_t rl = it / per_row;
    const int w = (int)(it - rl * per_row);
    const int64_t r = row_begin + rl;
    uint16_t* drow = dfused + r * W;
    if (w < rot_items) {
      const int hd = w / vph;
      const bool isq = hd < nq;
      const uint16_t* sep = (isq ? dq + (r * nq + hd) * D : dk + (r * nk + (hd - nq)) * D) + vv * 8;
      const uint16_t* f1 = fx + r * W + hd * D + vv * 8;
      float d[16], x[16], c[8], sn[8], g[16];
      qkn_unpack8(*reinterpret_cast<const v4i*>(sep), d);
      qkn_unpack8(*reinterpret_cast<const v4i*>(sep + half), d + 8);
      qkn_unpack8(*reinterpret_cast<const v4i*>(f1), x);
      qkn_unpack8(*reinterpret_cast<const v4i*>(f1 + half), x + 8);
      const int pos = (int)(r % seq);
      qkn_load8f(cosT + (int64_t)pos * half + vv * 8, c);
      qkn_load8f(sinT + (int64_t)pos * half + vv * 8, sn);
      const float rs = rstd[r * (nq + nk) + hd];
      float dot = 0.0f;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float dn1 = d[j] * c[j] + d[j + 8] * sn[j];  // conjugate rotation
        const float dn2 = d[j + 8] * c[j] - d[j] * sn[j];
        x[j] = x[j] * rs;  // xhat
        x[j + 8] = x[j + 8] * rs;
        d[j] = dn1;
        d[j + 8] = dn2;
      }
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        g[j] = (isq ? gqf[j] : gkf[j]) * d[j];
        dot += g[j] * x[j];
      }
      dot = qkn_group_sum<vph>(dot);
      const float mean = dot * (1.0f / (float)D);
      if (isq) {
#pragma unroll
        for (int j = 0; j < 16; ++j) accq[j] += d[j] * x[j];
      } else {
#pragma unroll
        for (int j = 0; j < 16; ++j) acck[j] += d[j] * x[j];
      }
      v4i o1, o2;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        o1[j] = (int)pack_bf16x2(rs * (g[2 * j] - x[2 * j] * mean), rs * (g[2 * j + 1] - x[2 * j + 1] * mean));
        o2[j] = (int)pack_bf16x2(rs * (g[2 * j + 8] - x[2 * j + 8] * mean), rs * (g[2 * j + 9] - x[2 * j + 9] * mean));
      }
      *reinterpret_cast<v4i*>(drow + hd * D + vv * 8) = o1;
      *reinterpret_cast<v4i*>(drow + hd * D + vv * 8 + half) = o2;
    } else {
      const int cv = w - rot_items;
      *reinterpret_cast<v4i*>(drow + (nq + nk) * D + cv * 8) = *reinterpret_cast<const v4i*>(dv + r * (int64_t)(nk * D) + cv * 8);
    }
  }
  // every lane is here: the wave's groups (same columns, lanes vph apart), then the block's waves in wave order
#pragma unroll
  for (int j = 0; j < 16; ++j) {
#pragma unroll
    for (int o = vph; o < 64; o <<= 1) {
      accq[j] += __shfl_xor(accq[j], o);
      acck[j] += __shfl_xor(acck[j], o);
    }
  }
  if (lane < vph) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      s_dg[wave][vv * 8 + j] = accq[j];
      s_dg[wave][half + vv * 8 + j] = accq[j + 8];
      s_dg[wave][D + vv * 8 + j] = acck[j];
      s_dg[wave][D + half + vv * 8 + j] = acck[j + 8];
    }
  }
  __syncthreads();
  for (int cidx = threadIdx.x; cidx < 2 * D; cidx += 256)
    dgp[(int64_t)blockIdx.x * (2 * D) + cidx] = ((s_dg[0][cidx] + s_dg[1][cidx]) + s_dg[2][cidx]) + s_dg[3][cidx];
}

static inline bool qkn_aligned16(const void* p) { return ((uintptr_t)p % 16) == 0; }

}  // namespace mi

extern "C" int mi_qknorm_rope_qkv(const void* fused_bf16, void* q_bf16, void* k_bf16, void* v_bf16, const void* gamma_q_bf16,
                                  const void* gamma_k_bf16, float* rstd_out, const float* cos_tab, const float* sin_tab,
                                  int64_t rows, int64_t seq, int n_q_heads, int n_kv_heads, int head_dim, float eps, void* stream) {
  MI_CHECK_ARG(fused_bf16 && q_bf16 && k_bf16 && v_bf16 && gamma_q_bf16 && gamma_k_bf16 && rstd_out && cos_tab && sin_tab,
               "mi_qknorm_rope_qkv: null pointer");
  MI_CHECK_ARG(head_dim == 64 || head_dim == 128, "mi_qknorm_rope_qkv: head_dim %d not supported (64, 128)", head_dim);
  MI_CHECK_ARG(rows >= 0 && n_q_heads > 0 && n_kv_heads > 0, "mi_qknorm_rope_qkv: bad shape");
  MI_CHECK_ARG(seq > 0, "mi_qknorm_rope_qkv: seq must be positive");
  MI_CHECK_ARG(rows < (1LL << 31), "mi_qknorm_rope_qkv: too many rows");
  MI_CHECK_ARG(eps >= 0.0f && isfinite(eps), "mi_qknorm_rope_qkv: eps must be finite and not negative");
  MI_CHECK_ARG(mi::qkn_aligned16(fused_bf16) && mi::qkn_aligned16(q_bf16) && mi::qkn_aligned16(k_bf16) && mi::qkn_aligned16(v_bf16) &&
                   mi::qkn_aligned16(gamma_q_bf16) && mi::qkn_aligned16(gamma_k_bf16) && mi::qkn_aligned16(rstd_out) &&
                   mi::qkn_aligned16(cos_tab) && mi::qkn_aligned16(sin_tab),
               "mi_qknorm_rope_qkv: pointers must be 16-byte aligned");
  MI_CHECK_ARG(seq < (1LL << 31) && (int64_t)(n_q_heads + 2LL * n_kv_heads) * head_dim < (1LL << 31), "mi_qknorm_rope_qkv: bad shape");
  if (rows == 0) return MI_OK;
  const int64_t per_row = (int64_t)(n_q_heads + 3LL * n_kv_heads) * (head_dim / 16);
  int64_t blocks = (rows * per_row + 255) / 256;
  if (blocks > 8192) blocks = 8192;
#define MI_QKN_FWD(Dv)                                                                                                          \
  hipLaunchKernelGGL(mi::qknorm_rope_fwd_kernel<Dv>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream,                 \
                     (const uint16_t*)fused_bf16, (uint16_t*)q_bf16, (uint16_t*)k_bf16, (uint16_t*)v_bf16,                      \
                     (const uint16_t*)gamma_q_bf16, (const uint16_t*)gamma_k_bf16, rstd_out, cos_tab, sin_tab, (int)rows, (int)seq, \
                     n_q_heads, n_kv_heads, eps)
  if (head_dim == 128) MI_QKN_FWD(128);
  else MI_QKN_FWD(64);
#undef MI_QKN_FWD
  MI_CHECK_LAUNCH("mi_qknorm_rope_qkv launch");
  return MI_OK;
}

extern "C" int mi_qknorm_rope_qkv_bwd(const void* dq_bf16, const void* dk_bf16, const void* dv_bf16, const void* fused_x_bf16,
                                      const float* rstd, const void* gamma_q_bf16, const void* gamma_k_bf16, const float* cos_tab,
                                      const float* sin_tab, void* dfused_bf16, float* dgamma_partial, int n_partials, int64_t rows,
                                      int64_t seq, int n_q_heads, int n_kv_heads, int head_dim, void* stream) {
  MI_CHECK_ARG(dq_bf16 && dk_bf16 && dv_bf16 && fused_x_bf16 && rstd && gamma_q_bf16 && gamma_k_bf16 && cos_tab && sin_tab &&
                   dfused_bf16 && dgamma_partial,
               "mi_qknorm_rope_qkv_bwd: null pointer");
  MI_CHECK_ARG(head_dim == 64 || head_dim == 128, "mi_qknorm_rope_qkv_bwd: head_dim %d not supported (64, 128)", head_dim);
  MI_CHECK_ARG(rows >= 0 && n_q_heads > 0 && n_kv_heads > 0, "mi_qknorm_rope_qkv_bwd: bad shape");
  MI_CHECK_ARG(seq > 0, "mi_qknorm_rope_qkv_bwd: seq must be positive");
  MI_CHECK_ARG(rows < (1LL << 31), "mi_qknorm_rope_qkv_bwd: too many rows");
  MI_CHECK_ARG(n_partials >= 1 && n_partials < (1 << 24), "mi_qknorm_rope_qkv_bwd: n_partials must be at least 1 (and below 2^24)");
  MI_CHECK_ARG(mi::qkn_aligned16(dq_bf16) && mi::qkn_aligned16(dk_bf16) && mi::qkn_aligned16(dv_bf16) &&
                   mi::qkn_aligned16(fused_x_bf16) && mi::qkn_aligned16(rstd) && mi::qkn_aligned16(gamma_q_bf16) &&
                   mi::qkn_aligned16(gamma_k_bf16) && mi::qkn_aligned16(cos_tab) && mi::qkn_aligned16(sin_tab) &&
                   mi::qkn_aligned16(dfused_bf16) && mi::qkn_aligned16(dgamma_partial),
               "mi_qknorm_rope_qkv_bwd: pointers must be 16-byte aligned");
  MI_CHECK_ARG(seq < (1LL << 31) && (int64_t)(n_q_heads + 2LL * n_kv_heads) * head_dim < (1LL << 31), "mi_qknorm_rope_qkv_bwd: bad shape");
  const int64_t rpb64 = (rows + n_partials - 1) / n_partials;
  const int rpb = rpb64 < 1 ? 1 : (int)rpb64;
#define MI_QKN_BWD(Dv)                                                                                                          \
  hipLaunchKernelGGL(mi::qknorm_rope_bwd_kernel<Dv>, dim3((unsigned)n_partials), dim3(256), 0, (hipStream_t)stream,             \
                     (const uint16_t*)dq_bf16, (const uint16_t*)dk_bf16, (const uint16_t*)dv_bf16, (const uint16_t*)fused_x_bf16, \
                     rstd, (const uint16_t*)gamma_q_bf16, (const uint16_t*)gamma_k_bf16, cos_tab, sin_tab, (uint16_t*)dfused_bf16, \
                     dgamma_partial, (int)rows, rpb, (int)seq, n_q_heads, n_kv_heads)
  if (head_dim == 128) MI_QKN_BWD(128);
  else MI_QKN_BWD(64);
#undef MI_QKN_BWD
  MI_CHECK_LAUNCH("mi_qknorm_rope_qkv_bwd launch");
  return MI_OK;
}
