// The attention core of mi_attn.hip at the short lengths of the reference's collator: S in {16, 32, .., 112} (bf16, causal, GQA,
// head_dim 64 / 128, bshd operands with caller-given token strides, lse [B, H, S] in the log2 domain).  At these lengths the
// whole problem of one (batch, kv head) fits in one workgroup -- all keys and all H / G query heads of the group -- so both
// kernels are one launch of B x G workgroups of 4 waves, and K / V leave HBM once per kv head.
//
//   attn_short_fwd_kernel   K and V (image of 128 rows; rows at or past S are not fetched and read as zeros) go to LDS once by
//                     DMA.  The (head, 32-query-row slice) pairs of the group are dealt over the four waves.  A wave forms
//                     S^T = K . Q^T against ALL key blocks up to its diagonal (at most four 32 x 32 accumulators, query on the
//                     lane), so the softmax is one pass with no running state and no rescale: max, exp2, sum.  O^T = V^T . P^T
//                     comes straight from the accumulators; one normalisation.
//   attn_short_bwd_kernel   wave w owns keys 32 w .. 32 w + 31: K and V rows register-resident with the key on the lane, dK^T and
//                     dV^T in accumulators over the whole sweep of query heads x 32-row slices (Q and dO slices staged once for
//                     all four waves; delta = rowsum(dO * O) is summed from the staging registers, O never reaches LDS).  Per
//                     step a wave forms S, P, dP and dS ONCE (5 products in all: S, dP, dV, dK, dQ).  dS has the key on the
//                     lane; the dQ product sums over keys, so the wave writes its bf16 dS block to a private LDS tile and reads
//                     it back transposed (ds_read_b64_tr_b16) as the B operand of  dQ^T = K^T . dS^T  (K^T: transposed reads of
//                     the K image).  The fp32 partials of the waves that see the slice (causal: wave <= slice) are summed
//                     through LDS in wave order 0, 1, 2, 3 and the slice is stored as bf16 rows: no atomics, no sum across
//                     workgroups, bitwise reproducible.
#include "mi_attn_dev.h"
#include "mi_attn_host.h"

namespace mi {

constexpr int SH_ROWS = 128;  // rows of the K / V image (S <= 112)
constexpr int SH_PASS = 64;   // rows one DMA pass of the workgroup stages (dma_voffsets)

// K or V of one (batch, kv head) -> LDS image; ceil(S / 64) passes, rows at or past S arrive as zeros
template <int D>
__device__ __forceinline__ void stage_image(const uint16_t* base, int64_t ts, int S, char* img, int tid) {
  const rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)base, 0, (int)((((int64_t)S - 1) * ts + D) * 2), 0x00020000);
  int voff[D / 32];
  dma_voffsets<D>(voff, ts, tid);
  for (int j = 0; j < (S + SH_PASS - 1) / SH_PASS; ++j)
    stage_dma_checked<D>(rs, voff, (int)((int64_t)j * SH_PASS * ts * 2), img + j * (SH_PASS * D * 2), tid >> 6);
}

template <int D>
__global__ __launch_bounds__(256, D == 128 ? 1 : 2) void attn_short_fwd_kernel(  // (head_dim 128: 96 KiB of LDS, one workgroup per CU)
    const uint16_t* __restrict__ q, const uint16_t* __restrict__ k, const uint16_t* __restrict__ v, uint16_t* __restrict__ o,
    float* __restrict__ lse, int S, int H, int G, int64_t q_ts, int64_t k_ts, int64_t v_ts, int64_t o_ts, float c) {
  constexpr int IMG = SH_ROWS * D * 2;  // bytes of the K (or V) image
  constexpr int SL = 32 * D * 2;        // bytes of one wave's O slice
  constexpr int KT = D / 16, DB = D / 32;
  __shared__ __attribute__((aligned(16))) char lds[2 * IMG + 4 * SL];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, r = lane & 31, h = lane >> 5;
  const int g = blockIdx.x, b = blockIdx.y, rep = H / G;
  const char* kimg = lds;
  const char* vimg = lds + IMG;
  stage_image<D>(k + (int64_t)b * S * k_ts + (int64_t)g * D, k_ts, S, lds, tid);
  stage_image<D>(v + (int64_t)b * S * v_ts + (int64_t)g * D, v_ts, S, lds + IMG, tid);
  dma_wait_all();
  __syncthreads();

  // items = (head of the group, slice); wave w takes items w, w + 4, ..  A slice costs slice + 1 key blocks, so the slice index
  // is rotated by the round number: a wave's successive items walk through all slices (3 slices: 4 = 1 mod 3 rotates already)
  const int nsl = (S + 31) / 32, nitems = rep * nsl;
  for (int item = w; item < nitems; item += 4) {
    const int head = g * rep + item / nsl;
    const int sl = (item % nsl + (nsl == 3 ? 0 : item / 4)) % nsl;
    const int q0 = 32 * sl, qrow = q0 + r;
    bf8 qf[KT];
    {  // rows at or past S read row S - 1; nothing of theirs is stored
      const uint16_t* qp = q + ((int64_t)b * S + min(qrow, S - 1)) * q_ts + (int64_t)head * D + 8 * h;
#pragma unroll
      for (int t = 0; t < KT; ++t) qf[t] = as_bf8(*reinterpret_cast<const v4i*>(qp + 16 * t));
    }
    f16v sacc[4];
#pragma unroll
    for (int kb = 0; kb < 4; ++kb)
      if (kb <= sl) {  // wave-uniform: key blocks above the diagonal contribute nothing
#pragma unroll
        for (int i = 0; i < 16; ++i) sacc[kb][i] = 0.0f;
        bf8 ka = row_frag<D>(kimg, 32 * kb, 0, lane);  // K fragments one k-step ahead of their MFMAs (see attn_fwd_kernel)
#pragma unroll
        for (int t = 0; t < KT; ++t) {
          bf8 kn = ka;
          if (t + 1 < KT) kn = row_frag<D>(kimg, 32 * kb, t + 1, lane);
          __builtin_amdgcn_sched_barrier(0);
          sacc[kb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ka, qf[t], sacc[kb], 0, 0, 0);
          __builtin_amdgcn_sched_barrier(0);
          ka = kn;
        }
        if (kb == sl) {  // the diagonal block.  A row below S never sees a key at or past S, so this is the only mask
#pragma unroll
          for (int i = 0; i < 16; ++i)
            if (acc_row(i, h) > r) sacc[kb][i] = -INFINITY;
        }
      }
    // one-pass softmax over all keys of the row (key 32 sl is never masked: the maximum is finite)
    float mx = -INFINITY;
#pragma unroll
    for (int kb = 0; kb < 4; ++kb)
      if (kb <= sl) {
#pragma unroll
        for (int i = 0; i < 16; ++i) mx = fmaxf(mx, sacc[kb][i]);
      }
    mx = fmaxf(mx, __shfl_xor(mx, 32));
    const float mc = mx * c;
    float l = 0.0f;
#pragma unroll
    for (int kb = 0; kb < 4; ++kb)
      if (kb <= sl) {
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const float p = __builtin_amdgcn_exp2f(__builtin_fmaf(sacc[kb][i], c, -mc));  // masked: exp2(-inf) = 0
          sacc[kb][i] = p;
          l += p;
        }
      }
    l += __shfl_xor(l, 32);
    f16v oacc[DB];
#pragma unroll
    for (int d = 0; d < DB; ++d)
#pragma unroll
      for (int i = 0; i < 16; ++i) oacc[d][i] = 0.0f;
#pragma unroll
    for (int kb = 0; kb < 4; ++kb)
      if (kb <= sl) {
#pragma unroll
        for (int s = 0; s < 2; ++s) {
          const bf8 pf = acc_frag(sacc[kb], s);
          bf8 fa = tr_frag<D>(vimg, 32 * kb + 16 * s, 0, lane);
#pragma unroll
          for (int d = 0; d < DB; ++d) {
            bf8 fn = fa;
            if (d + 1 < DB) fn = tr_frag<D>(vimg, 32 * kb + 16 * s, 32 * (d + 1), lane);
            __builtin_amdgcn_sched_barrier(0);
            oacc[d] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa, pf, oacc[d], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
            fa = fn;
          }
        }
      }
    if (h == 0 && qrow < S) lse[((int64_t)b * H + head) * S + qrow] = mc + __builtin_amdgcn_logf(l);  // v_log_f32 = log2
    store_rows_from_accT<D, true>(oacc, 1.0f / l, lds + 2 * IMG + w * SL, o + ((int64_t)b * S + q0) * o_ts + (int64_t)head * D, o_ts,
                                  lane, S - q0);
  }
}

template <int D>
__global__ __launch_bounds__(256, D == 128 ? 1 : 2) void attn_short_bwd_kernel(
    const uint16_t* __restrict__ q, const uint16_t* __restrict__ k, const uint16_t* __restrict__ v, const uint16_t* __restrict__ o,
    const uint16_t* __restrict__ dout, const float* __restrict__ lse, uint16_t* __restrict__ dq, uint16_t* __restrict__ dk,
    uint16_t* __restrict__ dv, int S, int H, int G, int64_t q_ts, int64_t k_ts, int64_t v_ts, int64_t o_ts, int64_t do_ts,
    int64_t dq_ts, int64_t dk_ts, int64_t dv_ts, float c, float scale) {
  constexpr int IMG = SH_ROWS * D * 2;  // bytes of the K image
  constexpr int SL = 32 * D * 2;        // bytes of one 32-row slice image
  constexpr int KT = D / 16, DB = D / 32, CPR = D / 8;
  constexpr int NCH = 32 * CPR / 256;   // 16-byte chunks of a slice per thread
  constexpr int DST = 32 * 128;         // a wave's dS tile [32 keys][32 queries] bf16, rows of the head_dim 64 image (128 bytes)
  constexpr int PPITCH = D * 4 + 16;    // bytes of one fp32 row of a dQ partial (+16: the rows of one store spread over the banks)
  constexpr int PART = 32 * PPITCH;     // a wave's dQ partial [32 queries][D] fp32
  constexpr int OFF_Q = IMG, OFF_DO = OFF_Q + SL, OFF_ST = OFF_DO + SL, OFF_DS = OFF_ST + 256, OFF_PART = OFF_DS + 4 * DST;
  __shared__ __attribute__((aligned(16))) char lds[OFF_PART + 4 * PART];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, r = lane & 31, h = lane >> 5;
  const int g = blockIdx.x, b = blockIdx.y, rep = H / G;
  const int key_first = 32 * w;  // first key of this wave

  stage_image<D>(k + (int64_t)b * S * k_ts + (int64_t)g * D, k_ts, S, lds, tid);
  bf8 kf[KT], vf[KT];
  {
    const int lkey = min(key_first + r, S - 1);  // keys at or past S read key S - 1; nothing of theirs is stored
    const uint16_t* kp = k + ((int64_t)b * S + lkey) * k_ts + (int64_t)g * D + 8 * h;
    const uint16_t* vp = v + ((int64_t)b * S + lkey) * v_ts + (int64_t)g * D + 8 * h;
#pragma unroll
    for (int t = 0; t < KT; ++t) {
      kf[t] = as_bf8(*reinterpret_cast<const v4i*>(kp + 16 * t));
      vf[t] = as_bf8(*reinterpret_cast<const v4i*>(vp + 16 * t));
    }
  }
#pragma unroll
  for (int t = 0; t < KT; ++t) {
    retire(kf[t]);
    retire(vf[t]);
  }
  f16v dka[DB], dva[DB];
#pragma unroll
  for (int d = 0; d < DB; ++d)
#pragma unroll
    for (int i = 0; i < 16; ++i) { dka[d][i] = 0.0f; dva[d][i] = 0.0f; }

  const int nsl = (S + 31) / 32, nsteps = rep * nsl;
  // staging: thread -> NCH chunks each of the Q, dO and O slices; threads 0..31 lse
  v4i qreg[NCH], dreg[NCH], oreg[NCH];
  float sreg = 0.0f;
  auto load_step = [&](int step) {
    const int head = g * rep + step / nsl, q0 = (step % nsl) * 32;
    const int64_t tok = (int64_t)b * S + q0, col = (int64_t)head * D;
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      const int cidx = tid + 256 * i, row = cidx / CPR, ch = cidx % CPR;
      if (q0 + row >= S) {  // a query row past S adds exactly nothing: zeros, so that no 0 x NaN reaches the sums
        qreg[i] = v4i{0, 0, 0, 0};
        dreg[i] = v4i{0, 0, 0, 0};
        oreg[i] = v4i{0, 0, 0, 0};
      } else {
        qreg[i] = *reinterpret_cast<const v4i*>(q + (tok + row) * q_ts + col + ch * 8);
        dreg[i] = *reinterpret_cast<const v4i*>(dout + (tok + row) * do_ts + col + ch * 8);
        oreg[i] = *reinterpret_cast<const v4i*>(o + (tok + row) * o_ts + col + ch * 8);
      }
    }
    if (tid < 32) sreg = q0 + tid >= S ? 0.0f : lse[((int64_t)b * H + head) * S + q0 + tid];
  };
  auto store_step = [&]() {
    float* st = reinterpret_cast<float*>(lds + OFF_ST);
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      const int cidx = tid + 256 * i, row = cidx / CPR, ch = cidx % CPR;
      *reinterpret_cast<v4i*>(lds + OFF_Q + tile_off<D>(row, ch)) = qreg[i];
      *reinterpret_cast<v4i*>(lds + OFF_DO + tile_off<D>(row, ch)) = dreg[i];
      // delta of the row: the CPR neighbouring lanes that hold it sum their 8 products in a fixed butterfly
      float dl = 0.0f;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const u32 a = (u32)dreg[i][j], bb = (u32)oreg[i][j];
        dl += __uint_as_float(a << 16) * __uint_as_float(bb << 16) + __uint_as_float(a & 0xFFFF0000u) * __uint_as_float(bb & 0xFFFF0000u);
      }
#pragma unroll
      for (int m = 1; m < CPR; m <<= 1) dl += __shfl_xor(dl, m);
      if (ch == 0) st[32 + row] = dl;
    }
    if (tid < 32) st[tid] = sreg;
  };
  load_step(0);
  store_step();
  dma_wait_all();
  __syncthreads();

  const char* kimg = lds;
  const char* qt = lds + OFF_Q;
  const char* dt = lds + OFF_DO;
  const float* st = reinterpret_cast<const float*>(lds + OFF_ST);
  char* dst = lds + OFF_DS + w * DST;
  for (int step = 0; step < nsteps; ++step) {
    const bool more = step + 1 < nsteps;
    if (more) load_step(step + 1);
    const int head = g * rep + step / nsl, sl = step % nsl, q0 = 32 * sl;
    // wave-uniform: a slice before this wave's keys sees none of them.  (sl < nsl, so an active wave has keys below S; a wave
    // whose keys are all at or past S is never active: it meets the barriers and stages, no more)
    if (w <= sl) {
      f16v sacc, pacc;
#pragma unroll
      for (int i = 0; i < 16; ++i) { sacc[i] = 0.0f; pacc[i] = 0.0f; }
#pragma unroll
      for (int t = 0; t < KT; ++t) {
        sacc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(row_frag<D>(qt, 0, t, lane), kf[t], sacc, 0, 0, 0);
        pacc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(row_frag<D>(dt, 0, t, lane), vf[t], pacc, 0, 0, 0);
      }
      const bool diag = sl == w;
      f16v dsacc;
#pragma unroll
      for (int a = 0; a < 4; ++a) {
        const v4f ls = *reinterpret_cast<const v4f*>(st + 8 * a + 4 * h);
        const v4f dl = *reinterpret_cast<const v4f*>(st + 32 + 8 * a + 4 * h);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int i = 4 * a + e;
          float p = __builtin_amdgcn_exp2f(__builtin_fmaf(sacc[i], c, -ls[e]));
          if (diag && r > acc_row(i, h)) p = 0.0f;      // key above the diagonal (this also covers every key at or past S)
          if (q0 + acc_row(i, h) >= S) p = 0.0f;        // a select: p and dS of a row past S are 0 whatever exp2 gave
          sacc[i] = p;
          dsacc[i] = p * (pacc[i] - dl[e]);
        }
        // dS block -> the wave's tile [key][query]: registers 4 a .. 4 a + 3 are queries 8 a + 4 h .. + 3 of key r
        uint2 pk;
        pk.x = pack_bf16x2(dsacc[4 * a], dsacc[4 * a + 1]);
        pk.y = pack_bf16x2(dsacc[4 * a + 2], dsacc[4 * a + 3]);
        *reinterpret_cast<uint2*>(dst + tile_off<64>(r, a) + 8 * h) = pk;
      }
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const bf8 pf = acc_frag(sacc, s), dsf = acc_frag(dsacc, s);
#pragma unroll
        for (int d = 0; d < DB; ++d) {
          dva[d] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(tr_frag<D>(dt, 16 * s, 32 * d, lane), pf, dva[d], 0, 0, 0);
          dka[d] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(tr_frag<D>(qt, 16 * s, 32 * d, lane), dsf, dka[d], 0, 0, 0);
        }
      }
      // dQ^T partial of this wave's 32 keys: K^T (transposed reads of the image) . dS^T (the tile read back with the query on
      // the lane, in the key order of tr_frag: the same bf16 values the dK product used)
      __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0): the tile is private to the wave, no barrier needed
      __builtin_amdgcn_wave_barrier();
      f16v dqa[DB];
#pragma unroll
      for (int d = 0; d < DB; ++d)
#pragma unroll
        for (int i = 0; i < 16; ++i) dqa[d][i] = 0.0f;
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const bf8 dsT = tr_frag<64>(dst, 16 * s, 0, lane);
#pragma unroll
        for (int d = 0; d < DB; ++d)
          dqa[d] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(tr_frag<D>(kimg, key_first + 16 * s, 32 * d, lane), dsT, dqa[d], 0, 0, 0);
      }
      char* pw = lds + OFF_PART + w * PART + r * PPITCH;
#pragma unroll
      for (int d = 0; d < DB; ++d)
#pragma unroll
        for (int i = 0; i < 4; ++i)
          *reinterpret_cast<v4f*>(pw + (32 * d + 8 * i + 4 * h) * 4) = v4f{dqa[d][4 * i], dqa[d][4 * i + 1], dqa[d][4 * i + 2], dqa[d][4 * i + 3]};
    }
    // keep the loop-carried dK / dV accumulators in AGPRs (see attn_bwd_dkdv_kernel)
    if (D == 128) {
#pragma unroll
      for (int d = 0; d < DB; ++d) asm volatile("" : "+a"(dka[d]), "+a"(dva[d]));
    }
    __syncthreads();
    // the slice's dQ: partials of waves 0 .. sl, summed in that order by every thread for its chunks
#pragma unroll
    for (int it = 0; it < NCH; ++it) {
      const int idx = it * 256 + tid, row = idx / CPR, ch = idx % CPR;
      const char* pp = lds + OFF_PART + row * PPITCH + ch * 32;
      float acc[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[e] = reinterpret_cast<const float*>(pp)[e];
#pragma unroll
      for (int w2 = 1; w2 < 4; ++w2)
        if (w2 <= sl) {
#pragma unroll
          for (int e = 0; e < 8; ++e) acc[e] += reinterpret_cast<const float*>(pp + w2 * PART)[e];
        }
      v4i val;
#pragma unroll
      for (int j = 0; j < 4; ++j) val[j] = (int)pack_bf16x2(acc[2 * j] * scale, acc[2 * j + 1] * scale);
      if (q0 + row < S) *reinterpret_cast<v4i*>(dq + ((int64_t)b * S + q0 + row) * dq_ts + (int64_t)head * D + ch * 8) = val;
    }
    if (more) store_step();
    __syncthreads();
  }
  char* slice = lds + OFF_PART + w * PART;  // (free after the loop's last barrier)
  store_rows_from_accT<D, true>(dka, scale, slice, dk + ((int64_t)b * S + key_first) * dk_ts + (int64_t)g * D, dk_ts, lane, S - key_first);
  __builtin_amdgcn_wave_barrier();
  store_rows_from_accT<D, true>(dva, 1.0f, slice, dv + ((int64_t)b * S + key_first) * dv_ts + (int64_t)g * D, dv_ts, lane, S - key_first);
}

}  // namespace mi

extern "C" int mi_attn_short_fwd(const void* q, const void* k, const void* v, void* o, float* lse, int B, int S, int H, int G,
                                 int D, int64_t q_ts, int64_t k_ts, int64_t v_ts, int64_t o_ts, float scale, int causal,
                                 void* stream) {
  const char* fn = "mi_attn_short_fwd";
  if (const int rc = mi::attn_check_operands(fn, {{"q", q, q_ts, mi::ATT_ROWS}, {"k", k, k_ts, mi::ATT_KV}, {"v", v, v_ts, mi::ATT_KV},
                                                  {"o", o, o_ts, mi::ATT_ROWS}, {"lse", lse, 0, mi::ATT_F32}},
                                             B, S, H, G, D, 16, 112, G))  // (the grid is G x B)
    return rc;
  MI_CHECK_ARG(causal != 0, "%s: only the causal mask is implemented", fn);
  const float c = scale * 1.4426950408889634f;
  dim3 grid(G, B), block(256);
  hipStream_t st = (hipStream_t)stream;
#define MI_ATTN_SHORT_FWD(DD)                                                                                                   \
  hipLaunchKernelGGL((mi::attn_short_fwd_kernel<DD>), grid, block, 0, st, (const uint16_t*)q, (const uint16_t*)k, (const uint16_t*)v, \
                     (uint16_t*)o, lse, S, H, G, q_ts, k_ts, v_ts, o_ts, c)
  if (D == 128) MI_ATTN_SHORT_FWD(128); else MI_ATTN_SHORT_FWD(64);
#undef MI_ATTN_SHORT_FWD
  MI_CHECK_LAUNCH("mi_attn_short_fwd launch");
  return MI_OK;
}

extern "C" int mi_attn_short_bwd(const void* q, const void* k, const void* v, const void* o, const void* dout, const float* lse,
                                 void* dq, void* dk, void* dv, int B, int S, int H, int G, int D, int64_t q_ts, int64_t k_ts,
                                 int64_t v_ts, int64_t o_ts, int64_t do_ts, int64_t dq_ts, int64_t dk_ts, int64_t dv_ts,
                                 float scale, int causal, void* stream) {
  const char* fn = "mi_attn_short_bwd";
  if (const int rc = mi::attn_check_operands(
          fn, {{"q", q, q_ts, mi::ATT_ROWS}, {"k", k, k_ts, mi::ATT_KV}, {"v", v, v_ts, mi::ATT_KV}, {"o", o, o_ts, mi::ATT_ROWS},
               {"dout", dout, do_ts, mi::ATT_ROWS}, {"lse", lse, 0, mi::ATT_F32}, {"dq", dq, dq_ts, mi::ATT_ROWS},
               {"dk", dk, dk_ts, mi::ATT_ROWS}, {"dv", dv, dv_ts, mi::ATT_ROWS}},
          B, S, H, G, D, 16, 112, G))  // (the grid is G x B)
    return rc;
  MI_CHECK_ARG(causal != 0, "%s: only the causal mask is implemented", fn);
  const float c = scale * 1.4426950408889634f;
  dim3 grid(G, B), block(256);
  hipStream_t st = (hipStream_t)stream;
#define MI_ATTN_SHORT_BWD(DD)                                                                                                   \
  hipLaunchKernelGGL((mi::attn_short_bwd_kernel<DD>), grid, block, 0, st, (const uint16_t*)q, (const uint16_t*)k, (const uint16_t*)v, \
                     (const uint16_t*)o, (const uint16_t*)dout, lse, (uint16_t*)dq, (uint16_t*)dk, (uint16_t*)dv, S, H, G, q_ts,  \
                     k_ts, v_ts, o_ts, do_ts, dq_ts, dk_ts, dv_ts, c, scale)
  if (D == 128) MI_ATTN_SHORT_BWD(128); else MI_ATTN_SHORT_BWD(64);
#undef MI_ATTN_SHORT_BWD
  MI_CHECK_LAUNCH("mi_attn_short_bwd launch");
  return MI_OK;
}
