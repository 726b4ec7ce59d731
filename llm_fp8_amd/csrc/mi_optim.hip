// Optimiser step of the reference's loop (train_fp8.py:288-291: clip_grad_norm_(1.0) -> AdamW(fused=True).step()),
// HBM-bound: the clip coefficient is folded into the AdamW pass (no separate in-place scaling of the gradients) and the
// squared-norm reduction is one streaming pass with fixed-order partial sums (bitwise reproducible).
//   mi_sumsq_bf16   partial[b] = sum over block b's elements of g^2 (fp32), b < n_partials
//   mi_adamw_bf16   torch.optim.AdamW semantics for bf16 parameters with bf16 exp_avg / exp_avg_sq, fp32 math
//   mi_grad_accum_multi   the gradients of a window of micro-batches summed in fp32 and rounded to bf16 once
#include "mi_common.h"
#include <string>

namespace mi {

__global__ __launch_bounds__(256) void sumsq_kernel(const uint16_t* __restrict__ g, int64_t n, float* __restrict__ partial) {
  __shared__ float s_red[4];
  const int tid = threadIdx.x;
  float acc = 0.0f;
  const int64_t nvec = n >> 3;
  const bool aligned = ((uintptr_t)g & 15) == 0;
  if (aligned) {
    // four independent 16-byte loads in flight per lane and iteration (the pass is latency-bound otherwise)
    const int64_t stride = (int64_t)gridDim.x * 256;
    float acc4[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    int64_t i = (int64_t)blockIdx.x * 256 + tid;
    for (; i + 3 * stride < nvec; i += 4 * stride) {
      v4i v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) v[u] = __builtin_nontemporal_load(reinterpret_cast<const v4i*>(g) + i + u * stride);
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const u32 w = (u32)v[u][j];
          const float a = __uint_as_float(w << 16), b = __uint_as_float(w & 0xFFFF0000u);
          acc4[u] += a * a + b * b;
        }
    }
    for (; i < nvec; i += stride) {
      const v4i v = reinterpret_cast<const v4i*>(g)[i];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const u32 w = (u32)v[j];
        const float a = __uint_as_float(w << 16), b = __uint_as_float(w & 0xFFFF0000u);
        acc4[0] += a * a + b * b;
      }
    }
    acc = (acc4[0] + acc4[1]) + (acc4[2] + acc4[3]);
    for (int64_t i = (nvec << 3) + (int64_t)blockIdx.x * 256 + tid; i < n; i += (int64_t)gridDim.x * 256) {
      const float a = bf16_bits_to_float(g[i]);
      acc += a * a;
    }
  } else {
    for (int64_t i = (int64_t)blockIdx.x * 256 + tid; i < n; i += (int64_t)gridDim.x * 256) {
      const float a = bf16_bits_to_float(g[i]);
      acc += a * a;
    }
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) acc += __shfl_xor(acc, o);
  if ((tid & 63) == 0) s_red[tid >> 6] = acc;
  __syncthreads();
  if (tid == 0) partial[blockIdx.x] = (s_red[0] + s_red[1]) + (s_red[2] + s_red[3]);
}

struct AdamArgs {
  float lr, beta1, beta2, eps, weight_decay, step_size, bc2_sqrt;
};

__device__ __forceinline__ float adam_sqrt(float x) { return sqrtf(x); }
__device__ __forceinline__ double adam_sqrt(double x) { return sqrt(x); }

// The one AdamW formula.  T = float: the arithmetic of the bf16-state kernels (state of 8 significand bits: fp32 evaluation error is
// far below its rounding).  T = double: fp32 state, where fp32 evaluation would itself be the error -- exp_avg = m + (1 - b1)(g - m)
// cancels where m and g oppose, its fp32 error is then large against the result, and it goes into the weight through the update.
template <typename T>
__device__ __forceinline__ void adam_one(T& p, T g, T& m, T& v, const AdamArgs& a) {
  p *= (T(1) - T(a.lr) * T(a.weight_decay));
  m = m + (T(1) - T(a.beta1)) * (g - m);
  v = T(a.beta2) * v + (T(1) - T(a.beta2)) * g * g;
  const T denom = adam_sqrt(v) / T(a.bc2_sqrt) + T(a.eps);
  p -= T(a.step_size) * (m / denom);
}
// arithmetic type of a state type (Vec8<ST> below)
template <typename ST> struct AdamMath { typedef float T; };
template <> struct AdamMath<float> { typedef double T; };

// THE STEP GUARD (include/mi_fp8.h, "non-finite *grad_scale"): the caller's clip coefficient is NaN when the gradient norm was
// Inf or NaN, and the launch then behaves as after an update of exactly zero -- p, the moments and the master are neither loaded
// (p: only where an FP8 sink needs it) nor written, the gradient is not loaded, no random bits are drawn; a weight with a sink
// still gets its FP8 copies, quantised from the weight as stored.  Every AdamW kernel loads *grad_scale first and tests it
// here, once, the same way in every lane of the launch.  The exponent bits are tested as an integer: no floating-point flag
// of the build can fold the test away.
__device__ __forceinline__ bool skip_step(float gs) { return (__float_as_uint(gs) & 0x7F800000u) == 0x7F800000u; }

__global__ __launch_bounds__(256) void adamw_kernel(uint16_t* __restrict__ p, const uint16_t* __restrict__ g,
                                                    uint16_t* __restrict__ m, uint16_t* __restrict__ v, int64_t n,
                                                    const float* __restrict__ grad_scale, AdamArgs a) {
  const float gs = grad_scale ? *grad_scale : 1.0f;
  if (skip_step(gs)) return;
  const int64_t nvec = n >> 3;
  const bool aligned = ((((uintptr_t)p) | ((uintptr_t)g) | ((uintptr_t)m) | ((uintptr_t)v)) & 15) == 0;
  const int64_t t0 = (int64_t)blockIdx.x * 256 + threadIdx.x, stride = (int64_t)gridDim.x * 256;
  if (aligned) {
    for (int64_t i = t0; i < nvec; i += stride) {
      v4i pv = reinterpret_cast<const v4i*>(p)[i];
      const v4i gv = reinterpret_cast<const v4i*>(g)[i];
      v4i mv = reinterpret_cast<const v4i*>(m)[i];
      v4i vv = reinterpret_cast<const v4i*>(v)[i];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float pl = __uint_as_float((u32)pv[j] << 16), ph = __uint_as_float((u32)pv[j] & 0xFFFF0000u);
        const float gl = gs * __uint_as_float((u32)gv[j] << 16), gh = gs * __uint_as_float((u32)gv[j] & 0xFFFF0000u);
        float ml = __uint_as_float((u32)mv[j] << 16), mh = __uint_as_float((u32)mv[j] & 0xFFFF0000u);
        float vl = __uint_as_float((u32)vv[j] << 16), vh = __uint_as_float((u32)vv[j] & 0xFFFF0000u);
        adam_one(pl, gl, ml, vl, a);
        adam_one(ph, gh, mh, vh, a);
        pv[j] = (int)pack_bf16x2(pl, ph);
        mv[j] = (int)pack_bf16x2(ml, mh);
        vv[j] = (int)pack_bf16x2(vl, vh);
      }
      reinterpret_cast<v4i*>(p)[i] = pv;
      reinterpret_cast<v4i*>(m)[i] = mv;
      reinterpret_cast<v4i*>(v)[i] = vv;
    }
  }
  for (int64_t i = (aligned ? (nvec << 3) : 0) + t0; i < n; i += stride) {
    float pf = bf16_bits_to_float(p[i]), mf = bf16_bits_to_float(m[i]), vf = bf16_bits_to_float(v[i]);
    adam_one(pf, gs * bf16_bits_to_float(g[i]), mf, vf, a);
    p[i] = (uint16_t)float_to_bf16_bits(pf);
    m[i] = (uint16_t)float_to_bf16_bits(mf);
    v[i] = (uint16_t)float_to_bf16_bits(vf);
  }
}

// ---- multi-tensor forms: ONE launch over every tensor of a parameter group.  `chunks` [nchunks] = (tensor index, chunk index
// inside it); a workgroup owns one chunk.  (A 3B model has ~280 parameter tensors: 2 x 280 launches per step, most of them a few
// microseconds long, become 2.)
// THE TABLE.  `tab` [rows, T] int64 on the device, one column per tensor; built by optim.py (`table_rows`, the same row numbers as
// ROW_*), stated for callers in include/mi_fp8.h.  Every kernel below reads it through tab_at().
//   0 p  1 g  2 exp_avg  3 exp_avg_sq  4 numel                                      -- all a kernel without sinks reads
//   5 cols: 0 = no sink, the tensor's chunks are flat runs of chunk_elems elements (the walk of adamw_multi_kernel);
//           > 0 = a [numel / cols, cols] weight with a sink, its chunks are 128 x 128 tiles, row-major over the tiles
//   6..11, per-tensor sink (adamw_cast_multi_kernel):  6 y [rows, ld_y] or 0  7 yT [cols, ld_yT] or 0  8 ld_y  9 ld_yT
//           10 const float* scale  11 float* amax
//   6..11, MXFP8 sink (adamw_mxcast_multi_kernel):     6 y_row [rows, cols]  7 s_row [cols/32, ldr]  8 y_colT [cols, ldr]
//           9 s_colT [rows/32, cols]  10 ldr = rows of the whole operand the tensor is a row-block of  11 unused;
//           rows 6..9 point at the tensor's first row inside the operand's buffers
//   12 ST = float: the fp32 master weight (rows 2, 3 are then fp32 too and p is output only)
//   12, 13 SR = true (bf16 state, stochastic rounding): global index of the tensor's first element, tensor key
struct ChunkRef {
  int tensor, chunk;
};
enum TabRow {
  ROW_P, ROW_G, ROW_EXP_AVG, ROW_EXP_AVG_SQ, ROW_NUMEL, ROW_COLS,
  ROW_Y, ROW_YT, ROW_LD_Y, ROW_LD_YT, ROW_SCALE, ROW_AMAX, ROW_MASTER, ROW_SR_KEY,
  ROW_Y_ROW = ROW_Y, ROW_S_ROW, ROW_Y_COLT, ROW_S_COLT, ROW_LDR, ROW_SR_BASE = ROW_MASTER
};
__device__ __forceinline__ int64_t tab_at(const int64_t* __restrict__ tab, int T, int row, int t) { return tab[(int64_t)row * T + t]; }

__global__ __launch_bounds__(256) void sumsq_multi_kernel(const int64_t* __restrict__ tab, int T, const ChunkRef* __restrict__ chunks,
                                                          int chunk_elems, double* __restrict__ partial) {
  // The squares of bf16 values are exact in fp32 (8 x 8 significand bits); they are ACCUMULATED in fp64, so a chunk's partial does
  // not depend on how the elements are dealt to lanes, and the total does not depend on how the tensors are cut into chunks,
  // groups or row shards beyond 2^-52: distributed.ShardedFP8DP's clip coefficient is then the replicated run's, bit for bit
  // (in fp32 the chunking moved the last bit of the norm in a few percent of the steps).  The kernel stays HBM-bound.
  __shared__ double s_red[4];
  const ChunkRef cr = chunks[blockIdx.x];
  const uint16_t* g = reinterpret_cast<const uint16_t*>(tab_at(tab, T, ROW_G, cr.tensor));
  const int64_t n = tab_at(tab, T, ROW_NUMEL, cr.tensor);
  const int64_t lo = (int64_t)cr.chunk * chunk_elems, hi = min(n, lo + chunk_elems);
  const int tid = threadIdx.x;
  double acc0 = 0.0, acc1 = 0.0;
  if ((((uintptr_t)g) & 15) == 0) {  // chunk_elems is a multiple of 8: chunk starts stay 16-byte aligned
    const int64_t v0 = lo >> 3, v1 = hi >> 3;
    int64_t i = v0 + tid;
    for (; i + 256 < v1; i += 512) {
      const v4i a = __builtin_nontemporal_load(reinterpret_cast<const v4i*>(g) + i);
      const v4i b = __builtin_nontemporal_load(reinterpret_cast<const v4i*>(g) + i + 256);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const u32 wa = (u32)a[j], wb = (u32)b[j];
        const float a0 = __uint_as_float(wa << 16), a1 = __uint_as_float(wa & 0xFFFF0000u);
        const float b0 = __uint_as_float(wb << 16), b1 = __uint_as_float(wb & 0xFFFF0000u);
        acc0 += (double)(a0 * a0) + (double)(a1 * a1);
        acc1 += (double)(b0 * b0) + (double)(b1 * b1);
      }
    }
    for (; i < v1; i += 256) {
      const v4i a = reinterpret_cast<const v4i*>(g)[i];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const u32 wa = (u32)a[j];
        const float a0 = __uint_as_float(wa << 16), a1 = __uint_as_float(wa & 0xFFFF0000u);
        acc0 += (double)(a0 * a0) + (double)(a1 * a1);
      }
    }
    for (int64_t k = (v1 << 3) + tid; k < hi; k += 256) {
      const float a = bf16_bits_to_float(g[k]);
      acc0 += (double)(a * a);
    }
  } else {
    for (int64_t k = lo + tid; k < hi; k += 256) {
      const float a = bf16_bits_to_float(g[k]);
      acc0 += (double)(a * a);
    }
  }
  double acc = acc0 + acc1;
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) acc += __shfl_xor(acc, o);
  if ((tid & 63) == 0) s_red[tid >> 6] = acc;
  __syncthreads();
  if (tid == 0) partial[blockIdx.x] = (s_red[0] + s_red[1]) + (s_red[2] + s_red[3]);
}

// ---- fp32 gradient accumulation over a window of micro-batches (include/mi_fp8.h mi_grad_accum_multi states the contract).
// One launch per micro-batch over every tensor, the chunk walk of sumsq_multi_kernel.  Table [5, T]:
//   0 g (bf16, this micro-batch's gradient; may be 0 in FINISH)  1 acc (fp32 window sum)  2 numel  3 mode  4 out (bf16, FINISH)
// ADD: acc = acc + g.  SET: acc = g (acc is not read).  FINISH: out = RNE_bf16(acc + g), acc is not written; out may be g.
// Exactly one fp32 add per element (-ffp-contract=off, and there is no multiply to contract with); nothing is reused inside a
// launch, so every load is nontemporal.  Stores, by measurement on the 3B parameter set (profiles/grad_accum_fp32.txt): the
// fp32 sums are stored PLAIN (nontemporal: SET 1.38 x, ADD 1.05 x the time), the bf16 result of FINISH NONTEMPORAL (plain: 1.08 x).
// MI_ACCUM_NT_ACC_STORES / MI_ACCUM_NT_OUT_STORES build the other policy for the A/B (Makefile: accum_ab).
#ifndef MI_ACCUM_NT_ACC_STORES
#define MI_ACCUM_NT_ACC_STORES 0
#endif
#ifndef MI_ACCUM_NT_OUT_STORES
#define MI_ACCUM_NT_OUT_STORES 1
#endif
enum AccumRow { ACC_ROW_G, ACC_ROW_ACC, ACC_ROW_NUMEL, ACC_ROW_MODE, ACC_ROW_OUT };
enum AccumMode { ACCUM_ADD, ACCUM_SET, ACCUM_FINISH };

template <bool NT, typename V>
__device__ __forceinline__ void accum_store(V* dst, V v) {
  if constexpr (NT) __builtin_nontemporal_store(v, dst);
  else *dst = v;
}

// One element.  HAS_G = false: FINISH of a tensor with no gradient in the last micro-batch, the sum is rounded as it stands.
template <int MODE, bool HAS_G>
__device__ __forceinline__ float accum_one(float acc, float g) {
  if constexpr (MODE == ACCUM_SET) return g;
  else if constexpr (HAS_G) return acc + g;
  else return acc;
}

// A lane's 8 consecutive elements (vector index i): the loads and the add + stores are separate calls, so that the walk can have
// the loads of two vectors in flight.
template <int MODE, bool HAS_G>
struct Accum8 {
  v4i g;
  v4f a[2];
  __device__ __forceinline__ void load(const uint16_t* gp, const float* acc, int64_t i) {
    if constexpr (HAS_G) g = __builtin_nontemporal_load(reinterpret_cast<const v4i*>(gp) + i);
    if constexpr (MODE != ACCUM_SET) {
      a[0] = __builtin_nontemporal_load(reinterpret_cast<const v4f*>(acc) + 2 * i);
      a[1] = __builtin_nontemporal_load(reinterpret_cast<const v4f*>(acc) + 2 * i + 1);
    }
  }
  __device__ __forceinline__ void finish(float* acc, uint16_t* out, int64_t i) {
    float f[8];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float gl = 0.0f, gh = 0.0f, al = 0.0f, ah = 0.0f;
      if constexpr (HAS_G) {
        gl = __uint_as_float((u32)g[j] << 16);
        gh = __uint_as_float((u32)g[j] & 0xFFFF0000u);
      }
      if constexpr (MODE != ACCUM_SET) {
        al = a[j >> 1][(2 * j) & 3];
        ah = a[j >> 1][((2 * j) & 3) + 1];
      }
      f[2 * j] = accum_one<MODE, HAS_G>(al, gl);
      f[2 * j + 1] = accum_one<MODE, HAS_G>(ah, gh);
    }
    if constexpr (MODE == ACCUM_FINISH) {
      const v4i o = {(int)pack_bf16x2(f[0], f[1]), (int)pack_bf16x2(f[2], f[3]), (int)pack_bf16x2(f[4], f[5]),
                     (int)pack_bf16x2(f[6], f[7])};
      accum_store<MI_ACCUM_NT_OUT_STORES != 0>(reinterpret_cast<v4i*>(out) + i, o);
    } else {
      const v4f o0 = {f[0], f[1], f[2], f[3]}, o1 = {f[4], f[5], f[6], f[7]};
      accum_store<MI_ACCUM_NT_ACC_STORES != 0>(reinterpret_cast<v4f*>(acc) + 2 * i, o0);
      accum_store<MI_ACCUM_NT_ACC_STORES != 0>(reinterpret_cast<v4f*>(acc) + 2 * i + 1, o1);
    }
  }
};

// Elements [lo, hi) of one tensor.  g and out may be the same array (no __restrict__): a lane reads its elements before it
// writes them and no other lane touches them.
template <int MODE, bool HAS_G>
__device__ __forceinline__ void accum_chunk(const uint16_t* g, float* acc, uint16_t* out, int64_t lo, int64_t hi, int tid) {
  uintptr_t align = (uintptr_t)acc;
  if constexpr (HAS_G) align |= (uintptr_t)g;
  if constexpr (MODE == ACCUM_FINISH) align |= (uintptr_t)out;
  int64_t done = lo;
  if ((align & 15) == 0) {  // chunk_elems is a multiple of 8: chunk starts stay 16-byte (bf16) and 32-byte (fp32) aligned
    const int64_t v1 = hi >> 3;
    int64_t i = (lo >> 3) + tid;
    for (; i + 256 < v1; i += 512) {
      Accum8<MODE, HAS_G> x, y;
      x.load(g, acc, i);
      y.load(g, acc, i + 256);
      x.finish(acc, out, i);
      y.finish(acc, out, i + 256);
    }
    for (; i < v1; i += 256) {
      Accum8<MODE, HAS_G> x;
      x.load(g, acc, i);
      x.finish(acc, out, i);
    }
    done = v1 << 3;
  }
  for (int64_t k = done + tid; k < hi; k += 256) {
    float gv = 0.0f, av = 0.0f;
    if constexpr (HAS_G) gv = bf16_bits_to_float(g[k]);
    if constexpr (MODE != ACCUM_SET) av = acc[k];
    const float f = accum_one<MODE, HAS_G>(av, gv);
    if constexpr (MODE == ACCUM_FINISH) out[k] = (uint16_t)float_to_bf16_bits(f);
    else acc[k] = f;
  }
}

__global__ __launch_bounds__(256) void grad_accum_multi_kernel(const int64_t* __restrict__ tab, int T, const ChunkRef* __restrict__ chunks,
                                                               int chunk_elems) {
  const ChunkRef cr = chunks[blockIdx.x];
  if ((unsigned)cr.tensor >= (unsigned)T || cr.chunk < 0) return;
  const uint16_t* g = reinterpret_cast<const uint16_t*>(tab_at(tab, T, ACC_ROW_G, cr.tensor));
  float* acc = reinterpret_cast<float*>(tab_at(tab, T, ACC_ROW_ACC, cr.tensor));
  uint16_t* out = reinterpret_cast<uint16_t*>(tab_at(tab, T, ACC_ROW_OUT, cr.tensor));
  const int64_t n = tab_at(tab, T, ACC_ROW_NUMEL, cr.tensor), mode = tab_at(tab, T, ACC_ROW_MODE, cr.tensor);
  const int64_t lo = (int64_t)cr.chunk * chunk_elems, hi = min(n, lo + chunk_elems);
  const int tid = threadIdx.x;
  if (acc == nullptr) return;
  // the mode is the tensor's, the same in every lane of the workgroup; the host cannot read the table: any other value is "do nothing"
  if (mode == ACCUM_ADD) {
    if (g != nullptr) accum_chunk<ACCUM_ADD, true>(g, acc, nullptr, lo, hi, tid);
  } else if (mode == ACCUM_SET) {
    if (g != nullptr) accum_chunk<ACCUM_SET, true>(g, acc, nullptr, lo, hi, tid);
  } else if (mode == ACCUM_FINISH && out != nullptr) {
    if (g != nullptr) accum_chunk<ACCUM_FINISH, true>(g, acc, out, lo, hi, tid);
    else accum_chunk<ACCUM_FINISH, false>(nullptr, acc, out, lo, hi, tid);
  }
}

// ---- state type of the multi-tensor AdamW kernels.  ST = uint16_t: bf16 parameter, exp_avg and exp_avg_sq (torch's fused AdamW
// layout; the weight is read from and written to p).  ST = float: fp32 exp_avg / exp_avg_sq and an fp32 MASTER weight (ROW_MASTER)
// that carries the update unrounded; p is then output only, p = RNE_bf16(master).  Vec8<ST> = one lane's 8 consecutive values.
template <typename ST>
struct Vec8;
template <>
struct Vec8<uint16_t> {
  v4i x;
  __device__ __forceinline__ void load(const uint16_t* b, int64_t i) { x = reinterpret_cast<const v4i*>(b)[i]; }
  __device__ __forceinline__ void store(uint16_t* b, int64_t i) const { reinterpret_cast<v4i*>(b)[i] = x; }
  __device__ __forceinline__ float lo(int j) const { return __uint_as_float((u32)x[j] << 16); }
  __device__ __forceinline__ float hi(int j) const { return __uint_as_float((u32)x[j] & 0xFFFF0000u); }
  __device__ __forceinline__ void set(int j, float l, float h) { x[j] = (int)pack_bf16x2(l, h); }
};
template <>
struct Vec8<float> {  // 32 bytes: two 16-byte accesses
  v4f x[2];
  __device__ __forceinline__ void load(const float* b, int64_t i) {
    x[0] = reinterpret_cast<const v4f*>(b)[2 * i];
    x[1] = reinterpret_cast<const v4f*>(b)[2 * i + 1];
  }
  __device__ __forceinline__ void store(float* b, int64_t i) const {
    reinterpret_cast<v4f*>(b)[2 * i] = x[0];
    reinterpret_cast<v4f*>(b)[2 * i + 1] = x[1];
  }
  __device__ __forceinline__ float lo(int j) const { return x[j >> 1][(2 * j) & 3]; }
  __device__ __forceinline__ float hi(int j) const { return x[j >> 1][((2 * j) & 3) + 1]; }
  __device__ __forceinline__ void set(int j, float l, float h) {
    x[j >> 1][(2 * j) & 3] = l;
    x[j >> 1][((2 * j) & 3) + 1] = h;
  }
};
__device__ __forceinline__ float state_load(const uint16_t* b, int64_t k) { return bf16_bits_to_float(b[k]); }
__device__ __forceinline__ float state_load(const float* b, int64_t k) { return b[k]; }
__device__ __forceinline__ void state_store(uint16_t* b, int64_t k, float f) { b[k] = (uint16_t)float_to_bf16_bits(f); }
__device__ __forceinline__ void state_store(float* b, int64_t k, float f) { b[k] = f; }

// ---- stochastic rounding of the bf16 results (SR = true instantiations of the bf16-state kernels; include/mi_fp8.h
// mi_adamw_sr_bf16_multi states the rule and the generator).  Philox4x32-10, counter-based: the 16 random bits of an element are a
// function of (seed, step, tensor key, stream, global element index) alone, whichever walk reaches the element.
struct AdamSrArgs : AdamArgs {
  u32 k0, k1, step;  // seed low / high word, step mod 2^32
};
template <bool SR> struct AdamKernelArgs { typedef AdamArgs T; };
template <> struct AdamKernelArgs<true> { typedef AdamSrArgs T; };

__device__ __forceinline__ void philox4x32_10(u32 c0, u32 c1, u32 c2, u32 c3, u32 k0, u32 k1, u32 (&out)[4]) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const u32 h0 = __umulhi(0xD2511F53u, c0), l0 = 0xD2511F53u * c0;
    const u32 h1 = __umulhi(0xCD9E8D57u, c2), l1 = 0xCD9E8D57u * c2;
    c0 = h1 ^ c1 ^ k0;
    c1 = l1;
    c2 = h0 ^ c3 ^ k1;
    c3 = l0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// One tensor's generator inputs.  SR = false: empty, nothing is read or computed.
template <bool SR>
struct SrCtx {
  __device__ __forceinline__ SrCtx(const AdamArgs&, const int64_t* __restrict__, int, int) {}
};
template <>
struct SrCtx<true> {
  u32 k0, k1, step, key4;
  int64_t base;  // global index of the tensor's first element
  __device__ __forceinline__ SrCtx(const AdamSrArgs& a, const int64_t* __restrict__ tab, int T, int t) {
    k0 = a.k0; k1 = a.k1; step = a.step;
    base = tab_at(tab, T, ROW_SR_BASE, t);
    key4 = (u32)tab_at(tab, T, ROW_SR_KEY, t) << 2;
  }
  // the four words of `stream` for the 8 elements [8 v, 8 v + 8)
  __device__ __forceinline__ void words(int64_t v, u32 stream, u32 (&w)[4]) const {
    philox4x32_10((u32)v, (u32)((unsigned long long)v >> 32), step, key4 | stream, k0, k1, w);
  }
  // the 16 bits of global element e
  __device__ __forceinline__ u32 bits16(int64_t e, u32 stream) const {
    u32 w[4];
    words(e >> 3, stream, w);
    const int j = (int)(e & 7);
    return (w[j >> 1] >> (16 * (j & 1))) & 0xFFFFu;
  }
};
// fp32 -> bf16 bits with the 16 random bits r: finite x moves to its upper neighbour with probability (low 16 bits) / 65536;
// NaN and Inf convert as everywhere else
__device__ __forceinline__ u32 sr_bf16_bits(float x, u32 r) {
  const u32 b = __float_as_uint(x);
  return ((b & 0x7F800000u) == 0x7F800000u) ? float_to_bf16_bits(x) : (b + r) >> 16;
}
__device__ __forceinline__ u32 sr_pack_bf16x2(float lo, float hi, u32 word) {
  return sr_bf16_bits(lo, word & 0xFFFFu) | (sr_bf16_bits(hi, word >> 16) << 16);
}

// The tensor's addresses out of the table: `w` is what the update reads and writes at full state precision (p itself for bf16
// state, the fp32 master otherwise).
template <typename ST>
struct AdamPtrs {
  uint16_t* p;
  const uint16_t* g;
  ST *w, *m, *v;
  __device__ __forceinline__ AdamPtrs(const int64_t* __restrict__ tab, int T, int t) {
    p = reinterpret_cast<uint16_t*>(tab_at(tab, T, ROW_P, t));
    g = reinterpret_cast<const uint16_t*>(tab_at(tab, T, ROW_G, t));
    m = reinterpret_cast<ST*>(tab_at(tab, T, ROW_EXP_AVG, t));
    v = reinterpret_cast<ST*>(tab_at(tab, T, ROW_EXP_AVG_SQ, t));
    if constexpr (sizeof(ST) == 4) w = reinterpret_cast<ST*>(tab_at(tab, T, ROW_MASTER, t));
    else w = p;
  }
  __device__ __forceinline__ bool aligned16() const {
    if constexpr (sizeof(ST) == 4)
      return ((((uintptr_t)p) | ((uintptr_t)g) | ((uintptr_t)m) | ((uintptr_t)v) | ((uintptr_t)w)) & 15) == 0;
    else
      return ((((uintptr_t)p) | ((uintptr_t)g) | ((uintptr_t)m) | ((uintptr_t)v)) & 15) == 0;
  }
};

// AdamW on one lane's 8 consecutive elements (vector index i): load, update, store.  f = the 8 weights as stored in p -- the
// ROUNDED bf16 values, which is what the FP8 sinks quantise.  SR (bf16 state only): the three roundings are stochastic, one
// generator call per stream for the lane's 8 elements (sr.base is a multiple of 8 on this path).
template <typename ST, bool SR>
__device__ __forceinline__ void adam_vec8(const AdamPtrs<ST>& t, int64_t i, float gs, const AdamArgs& a, const SrCtx<SR>& sr,
                                          float (&f)[8]) {
  static_assert(!SR || sizeof(ST) == 2, "stochastic rounding is for bf16 state");
  Vec8<ST> wv, mv, vv;
  u32 pw[4];
  [[maybe_unused]] u32 rp[4], rm[4], rv[4];
  if constexpr (SR) {
    const int64_t v = (sr.base >> 3) + i;
    sr.words(v, 0, rp);
    sr.words(v, 1, rm);
    sr.words(v, 2, rv);
  }
  wv.load(t.w, i);
  const v4i gv = __builtin_nontemporal_load(reinterpret_cast<const v4i*>(t.g) + i);
  mv.load(t.m, i);
  vv.load(t.v, i);
  typedef typename AdamMath<ST>::T T;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    T pl = wv.lo(j), ph = wv.hi(j);
    const T gl = T(gs) * T(__uint_as_float((u32)gv[j] << 16)), gh = T(gs) * T(__uint_as_float((u32)gv[j] & 0xFFFF0000u));
    T ml = mv.lo(j), mh = mv.hi(j);
    T vl = vv.lo(j), vh = vv.hi(j);
    adam_one(pl, gl, ml, vl, a);
    adam_one(ph, gh, mh, vh, a);
    if constexpr (sizeof(ST) == 4) {
      wv.set(j, (float)pl, (float)ph);           // the master: the fp64 result rounded once to fp32 ...
      pw[j] = pack_bf16x2(wv.lo(j), wv.hi(j));   // ... and p = RNE_bf16 of that STORED value
    } else {
      if constexpr (SR) pw[j] = sr_pack_bf16x2(pl, ph, rp[j]);
      else pw[j] = pack_bf16x2(pl, ph);
      wv.x[j] = (int)pw[j];
    }
    if constexpr (SR) {
      mv.x[j] = (int)sr_pack_bf16x2(ml, mh, rm[j]);
      vv.x[j] = (int)sr_pack_bf16x2(vl, vh, rv[j]);
    } else {
      mv.set(j, (float)ml, (float)mh);
      vv.set(j, (float)vl, (float)vh);
    }
    f[2 * j] = __uint_as_float(pw[j] << 16);
    f[2 * j + 1] = __uint_as_float(pw[j] & 0xFFFF0000u);
  }
  wv.store(t.w, i);
  if constexpr (sizeof(ST) == 4) {
    const v4i pv = {(int)pw[0], (int)pw[1], (int)pw[2], (int)pw[3]};
    reinterpret_cast<v4i*>(t.p)[i] = pv;
  }
  mv.store(t.m, i);
  vv.store(t.v, i);
}
// A skipped step's form of adam_vec8 (skip_step): f = the lane's 8 weights as they stand in p; nothing else is read, nothing written.
__device__ __forceinline__ void stored_vec8(const uint16_t* p, int64_t i, float (&f)[8]) {
  const v4i pv = reinterpret_cast<const v4i*>(p)[i];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    f[2 * j] = __uint_as_float((u32)pv[j] << 16);
    f[2 * j + 1] = __uint_as_float((u32)pv[j] & 0xFFFF0000u);
  }
}

// Flat walk of one chunk: elements [chunk * chunk_elems, + chunk_elems) of the tensor, 8 per lane where every array is 16-byte
// aligned, one per lane otherwise and on the tail.  SR: a tensor whose first element is not at a multiple of 8 of the global index
// is walked element-wise too (a lane's 8 elements would straddle two generator calls).
template <typename ST, bool SR>
__device__ __forceinline__ void adam_flat_chunk(const AdamPtrs<ST>& t, int64_t n, int chunk, int chunk_elems, float gs,
                                                const AdamArgs& a, const SrCtx<SR>& sr, int tid) {
  const int64_t lo = (int64_t)chunk * chunk_elems, hi = min(n, lo + chunk_elems);
  int64_t done = lo;
  bool vec = t.aligned16();
  if constexpr (SR) vec = vec && (sr.base & 7) == 0;
  if (vec) {
    const int64_t v0 = lo >> 3, v1 = hi >> 3;
    for (int64_t i = v0 + tid; i < v1; i += 256) {
      float f[8];
      adam_vec8(t, i, gs, a, sr, f);
    }
    done = v1 << 3;
  }
  for (int64_t k = done + tid; k < hi; k += 256) {
    typedef typename AdamMath<ST>::T T;
    T pf = state_load(t.w, k), mf = state_load(t.m, k), vf = state_load(t.v, k);
    adam_one(pf, T(gs) * T(bf16_bits_to_float(t.g[k])), mf, vf, a);
    if constexpr (SR) {
      const int64_t e = sr.base + k;
      t.w[k] = (uint16_t)sr_bf16_bits(pf, sr.bits16(e, 0));
      t.m[k] = (uint16_t)sr_bf16_bits(mf, sr.bits16(e, 1));
      t.v[k] = (uint16_t)sr_bf16_bits(vf, sr.bits16(e, 2));
    } else {
      state_store(t.w, k, (float)pf);
      if constexpr (sizeof(ST) == 4) t.p[k] = (uint16_t)float_to_bf16_bits((float)pf);
      state_store(t.m, k, (float)mf);
      state_store(t.v, k, (float)vf);
    }
  }
}

__global__ __launch_bounds__(256) void adamw_multi_kernel(const int64_t* __restrict__ tab, int T, const ChunkRef* __restrict__ chunks,
                                                          int chunk_elems, const float* __restrict__ grad_scale, AdamArgs a) {
  const float gs = grad_scale ? *grad_scale : 1.0f;
  if (skip_step(gs)) return;  // no tensor of this launch has a sink
  const ChunkRef cr = chunks[blockIdx.x];
  const AdamPtrs<uint16_t> t(tab, T, cr.tensor);
  const int64_t n = tab_at(tab, T, ROW_NUMEL, cr.tensor);
  adam_flat_chunk(t, n, cr.chunk, chunk_elems, gs, a, SrCtx<false>(a, tab, T, cr.tensor), threadIdx.x);
}

// A lane's 8 x 8 block inside the chunk's 128 x 128 tile: wave w owns the 64 x 64 quadrant (w >> 1, w & 1), lane l its block
// (l >> 3, l & 7).  (r0, c0) = the block's first element in the [rows, cols] weight; it may lie outside (ragged tiles).
struct TileBlock {
  int64_t rows, r0, c0;
  __device__ __forceinline__ TileBlock(int64_t n, int64_t cols, int chunk, int tid) {
    rows = n / cols;
    const int tiles_c = (int)((cols + 127) >> 7);
    const int lane = tid & 63, wave = tid >> 6;
    const int tile_r = chunk / tiles_c, tile_c = chunk % tiles_c;
    r0 = (int64_t)tile_r * 128 + (wave >> 1) * 64 + (lane >> 3) * 8;
    c0 = (int64_t)tile_c * 128 + (wave & 1) * 64 + (lane & 7) * 8;
  }
};

// AdamW + FP8 weight cast in one pass (the weight-cast hand-off): under delayed scaling the scale the NEXT
// forward quantises a weight with is already final when the optimiser runs (the forward arena was updated at the end of this
// step's forward), and the optimiser streams every weight anyway.  For tensors with a "sink" (cols > 0) the chunk is a 128 x 128
// tile of the [rows, cols] weight (the tiling of cast_amax_kernel: 8 x 8 block per lane, in-register byte transpose): each
// element is updated, rounded to bf16, stored -- and that ROUNDED value is quantised exactly as mi_cast_amax would
// (y = sat(float(bf16) * scale), amax = max |bf16|), into y [rows, ld_y] and the transposed copy yT [cols, ld_yT].
// Tensors without a sink (cols == 0) take the flat path of adamw_multi_kernel.  Table: the per-tensor rows of THE TABLE above.
// SKIP (a skipped step, skip_step): the tile's values are the weight as it stands in p (stored_vec8) instead of the update's
// results; everything after them is the same code.  The kernel picks one of the two instantiations per workgroup, so the
// update's instantiation carries nothing of the other.
template <typename ST, bool SR, bool SKIP>
__device__ __forceinline__ void adamw_cast_tile(const int64_t* __restrict__ tab, int T, const ChunkRef cr, const AdamPtrs<ST>& t, int64_t n,
                                                int64_t cols, float gs, const typename AdamKernelArgs<SR>::T& a, const SrCtx<SR>& sr,
                                                int tid) {
  const int tensor = cr.tensor;
  uint8_t* y = reinterpret_cast<uint8_t*>(tab_at(tab, T, ROW_Y, tensor));
  uint8_t* yT = reinterpret_cast<uint8_t*>(tab_at(tab, T, ROW_YT, tensor));
  const int64_t ld_y = tab_at(tab, T, ROW_LD_Y, tensor), ld_yT = tab_at(tab, T, ROW_LD_YT, tensor);
  const float scale = *reinterpret_cast<const float*>(tab_at(tab, T, ROW_SCALE, tensor));
  float* amax_out = reinterpret_cast<float*>(tab_at(tab, T, ROW_AMAX, tensor));
  const TileBlock b(n, cols, cr.chunk, tid);
  const int64_t r0 = b.r0, c0 = b.c0;
  float amax = 0.0f;
  if (r0 < b.rows && c0 < cols) {
    u32 lo[8], hi[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      float f[8];  // the ROUNDED weight: what the next forward's cast would read
      if constexpr (SKIP) stored_vec8(t.p, ((r0 + i) * cols + c0) >> 3, f);
      else adam_vec8(t, ((r0 + i) * cols + c0) >> 3, gs, a, sr, f);
#pragma unroll
      for (int j = 0; j < 8; ++j) amax = fmaxf(amax, (f[j] != f[j]) ? 0.0f : fabsf(f[j]));
      lo[i] = cvt4_fp8<MI_FMT_E4M3>(f[0] * scale, f[1] * scale, f[2] * scale, f[3] * scale);
      hi[i] = cvt4_fp8<MI_FMT_E4M3>(f[4] * scale, f[5] * scale, f[6] * scale, f[7] * scale);
    }
    // nontemporal: the copies are read again only by the NEXT forward; as write-back lines the 64-byte row segments cost
    // 4.0 ms per step on the 3B parameter set, streamed 1.3 ms (tools/bench_adamw.py)
    if (y != nullptr) store_rows8<true>(y + r0 * ld_y + c0, ld_y, lo, hi);
    if (yT != nullptr) store_cols8<true>(yT + c0 * ld_yT + r0, ld_yT, lo, hi);
  }
  publish_amax(amax, amax_out);
}
template <typename ST, bool SR = false>
__global__ __launch_bounds__(256) void adamw_cast_multi_kernel(const int64_t* __restrict__ tab, int T, const ChunkRef* __restrict__ chunks,
                                                               int chunk_elems, const float* __restrict__ grad_scale,
                                                               typename AdamKernelArgs<SR>::T a) {
  const float gs = grad_scale ? *grad_scale : 1.0f;
  const bool skip = skip_step(gs);
  const ChunkRef cr = chunks[blockIdx.x];
  const int64_t cols = tab_at(tab, T, ROW_COLS, cr.tensor);
  if (skip && cols == 0) return;  // a skipped step leaves a tensor without a sink alone
  const AdamPtrs<ST> t(tab, T, cr.tensor);
  const SrCtx<SR> sr(a, tab, T, cr.tensor);
  const int64_t n = tab_at(tab, T, ROW_NUMEL, cr.tensor);
  const int tid = threadIdx.x;
  if (cols == 0) return adam_flat_chunk(t, n, cr.chunk, chunk_elems, gs, a, sr, tid);  // the walk of adamw_multi_kernel
  // tile of a weight with an FP8 sink
  if (skip) adamw_cast_tile<ST, SR, true>(tab, T, cr, t, n, cols, gs, a, sr, tid);
  else adamw_cast_tile<ST, SR, false>(tab, T, cr, t, n, cols, gs, a, sr, tid);
}

// AdamW + MXFP8 weight quantisation in one pass: the MXFP8 form of the weight-cast hand-off.  Block scaling has no state -- the
// E8M0 scale of a 32-element block comes from the block itself -- so the copies the NEXT forward needs (row-wise blocks for
// fprop, column-wise blocks, stored transposed, for dgrad) can be emitted as soon as the weight is updated.  Same tile walk as
// adamw_cast_multi_kernel (128 x 128 tile per workgroup, 8 x 8 block per lane); the quantisation of the ROUNDED bf16 weight is
// mxfp8_quant_kernel's: both call mx_quant_rows / mx_quant_cols (mi_common.h).  Table: the MXFP8 rows of THE TABLE above.
// SKIP: as in adamw_cast_tile
template <typename ST, bool SR, bool SKIP>
__device__ __forceinline__ void adamw_mxcast_tile(const int64_t* __restrict__ tab, int T, const ChunkRef cr, const AdamPtrs<ST>& t, int64_t n,
                                                  int64_t cols, float gs, const typename AdamKernelArgs<SR>::T& a, const SrCtx<SR>& sr,
                                                  int tid) {
  const int lane = tid & 63, tensor = cr.tensor;
  uint8_t* y_row = reinterpret_cast<uint8_t*>(tab_at(tab, T, ROW_Y_ROW, tensor));
  uint8_t* s_row = reinterpret_cast<uint8_t*>(tab_at(tab, T, ROW_S_ROW, tensor));
  uint8_t* y_colT = reinterpret_cast<uint8_t*>(tab_at(tab, T, ROW_Y_COLT, tensor));
  uint8_t* s_colT = reinterpret_cast<uint8_t*>(tab_at(tab, T, ROW_S_COLT, tensor));
  const int64_t ldr = tab_at(tab, T, ROW_LDR, tensor);
  const TileBlock b(n, cols, cr.chunk, tid);
  const int64_t r0 = b.r0, c0 = b.c0;
  const bool active = r0 < b.rows && c0 < cols;  // rows, cols multiples of 32: a 4-lane block group is all-active or all-inactive
  float f[8][8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    if (active) {  // the ROUNDED weight: what the next forward's quantiser would read
      if constexpr (SKIP) stored_vec8(t.p, ((r0 + i) * cols + c0) >> 3, f[i]);
      else adam_vec8(t, ((r0 + i) * cols + c0) >> 3, gs, a, sr, f[i]);
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) f[i][j] = 0.0f;
    }
  }
  const unsigned long long nanmask = mx_take_nans(f);
  u32 lo[8], hi[8], sbytes[8];
  // nontemporal stores, as in adamw_cast_multi_kernel
  mx_quant_rows<MI_FMT_E4M3>(f, nanmask, lo, hi, sbytes);  // row-wise blocks (32 columns = 4 lanes)
  if (active) {
    store_rows8<true>(y_row + r0 * cols + c0, cols, lo, hi);
    if ((lane & 3) == 0) store_scales8(s_row + (c0 / 32) * ldr + r0, sbytes);
  }
  mx_quant_cols<MI_FMT_E4M3>(f, nanmask, lo, hi, sbytes);  // column-wise blocks (32 rows = 4 lane rows), stored transposed
  if (active) {
    store_cols8<true>(y_colT + c0 * ldr + r0, ldr, lo, hi);
    if (((lane >> 3) & 3) == 0) store_scales8(s_colT + (r0 / 32) * cols + c0, sbytes);
  }
}
template <typename ST, bool SR = false>
__global__ __launch_bounds__(256) void adamw_mxcast_multi_kernel(const int64_t* __restrict__ tab, int T, const ChunkRef* __restrict__ chunks,
                                                                 int chunk_elems, const float* __restrict__ grad_scale,
                                                                 typename AdamKernelArgs<SR>::T a) {
  const float gs = grad_scale ? *grad_scale : 1.0f;
  const bool skip = skip_step(gs);
  const ChunkRef cr = chunks[blockIdx.x];
  const int64_t cols = tab_at(tab, T, ROW_COLS, cr.tensor);
  if (skip && cols == 0) return;  // a skipped step leaves a tensor without a sink alone
  const AdamPtrs<ST> t(tab, T, cr.tensor);
  const SrCtx<SR> sr(a, tab, T, cr.tensor);
  const int64_t n = tab_at(tab, T, ROW_NUMEL, cr.tensor);
  const int tid = threadIdx.x;
  if (cols == 0) return adam_flat_chunk(t, n, cr.chunk, chunk_elems, gs, a, sr, tid);  // the walk of adamw_multi_kernel
  if (skip) adamw_mxcast_tile<ST, SR, true>(tab, T, cr, t, n, cols, gs, a, sr, tid);
  else adamw_mxcast_tile<ST, SR, false>(tab, T, cr, t, n, cols, gs, a, sr, tid);
}

// Embedding weight gradient added IN PLACE into an existing [V, H] bf16 gradient (the tied lm_head / embedding table already
// holds the lm_head wgrad): grad[id, :] += alpha * sum over the tokens with that id of dY[token, :].  Replaces
// aten::embedding_dense_backward (zero-fill of a dense [V, H] + scatter) followed by a dense add -- 2 x 788 MB written and
// 3 x 788 MB read for Llama-3.2-3B -- by a pass over the touched rows only.  Deterministic: ids are sorted (stable) by the
// caller, the workgroup at the head of a run of equal ids sums that run in order in fp32 and is the only writer of the row.
__global__ __launch_bounds__(256) void embedding_grad_add_kernel(uint16_t* __restrict__ grad, const uint16_t* __restrict__ dy,
                                                                 const int64_t* __restrict__ sorted_ids,
                                                                 const int64_t* __restrict__ perm, int T, int H, int64_t V,
                                                                 float alpha, int64_t padding_idx) {
  const int i0 = blockIdx.x;
  const int64_t id = sorted_ids[i0];
  if (i0 > 0 && sorted_ids[i0 - 1] == id) return;  // not the head of its run
  if (id < 0 || id >= V || id == padding_idx) return;
  int i1 = i0 + 1;
  while (i1 < T && sorted_ids[i1] == id) ++i1;
  for (int c = threadIdx.x * 8; c < H; c += 2048) {
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int i = i0; i < i1; ++i) {
      const v4i v = *reinterpret_cast<const v4i*>(dy + perm[i] * (int64_t)H + c);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        acc[2 * j] += __uint_as_float((u32)v[j] << 16);
        acc[2 * j + 1] += __uint_as_float((u32)v[j] & 0xFFFF0000u);
      }
    }
    uint16_t* gp = grad + id * (int64_t)H + c;
    const v4i g = *reinterpret_cast<const v4i*>(gp);
    v4i o;
#pragma unroll
    for (int j = 0; j < 4; ++j)
      o[j] = (int)pack_bf16x2(__uint_as_float((u32)g[j] << 16) + alpha * acc[2 * j],
                              __uint_as_float((u32)g[j] & 0xFFFF0000u) + alpha * acc[2 * j + 1]);
    *reinterpret_cast<v4i*>(gp) = o;
  }
}

}  // namespace mi

static mi::AdamArgs make_adam_args(float lr, float beta1, float beta2, float eps, float weight_decay, int64_t step) {
  mi::AdamArgs a;
  a.lr = lr; a.beta1 = beta1; a.beta2 = beta2; a.eps = eps; a.weight_decay = weight_decay;
  const double bc1 = 1.0 - pow((double)beta1, (double)step), bc2 = 1.0 - pow((double)beta2, (double)step);
  a.step_size = (float)((double)lr / bc1);
  a.bc2_sqrt = (float)sqrt(bc2);
  return a;
}

// The argument check of the six multi-tensor entry points, before any launch.  `who` = the entry point (its __func__), for the
// message.  The calls with a sink_kind (fp32 state, stochastic rounding: `empty_ok`) accept an empty chunk list and name chunk_elems
// and sink_kind in messages of their own; the others have one message for every size.
static int check_multi(const char* who, bool empty_ok, bool pointers, int n_tensors, int n_chunks, int chunk_elems, int64_t step,
                       int sink_kind = 0) {
  const bool chunk_ok = chunk_elems >= 8 && chunk_elems % 8 == 0;
  MI_CHECK_ARG(pointers, "%s: null pointer", who);
  MI_CHECK_ARG(n_tensors >= 1 && n_chunks >= (empty_ok ? 0 : 1) && (empty_ok || chunk_ok) && step >= 1, "%s: bad sizes", who);
  MI_CHECK_ARG(chunk_ok, "%s: chunk_elems must be a positive multiple of 8", who);
  MI_CHECK_ARG(sink_kind == 0 || sink_kind == 1, "%s: sink_kind must be 0 (per-tensor FP8) or 1 (MXFP8)", who);
  return MI_OK;
}

// One workgroup of 256 lanes per chunk; `tail` = the kernel's arguments after chunk_elems.  An empty chunk list (where the check
// lets one through) is nothing to do.
template <typename Kernel, typename... Tail>
static int launch_multi(const char* who, Kernel kernel, const int64_t* table, int n_tensors, const int32_t* chunks, int n_chunks,
                        int chunk_elems, void* stream, Tail... tail) {
  if (n_chunks == 0) return MI_OK;
  hipLaunchKernelGGL(kernel, dim3((unsigned)n_chunks), dim3(256), 0, (hipStream_t)stream, table, n_tensors, (const mi::ChunkRef*)chunks,
                     chunk_elems, tail...);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? MI_OK : mi::hip_fail(e, (std::string(who) + " launch").c_str());
}

extern "C" int mi_sumsq_bf16_multi(const int64_t* table, int n_tensors, const int32_t* chunks, int n_chunks, int chunk_elems,
                                   double* partial, void* stream) {
  if (int rc = check_multi(__func__, false, table && chunks && partial, n_tensors, n_chunks, chunk_elems, 1)) return rc;
  return launch_multi(__func__, mi::sumsq_multi_kernel, table, n_tensors, chunks, n_chunks, chunk_elems, stream, partial);
}

extern "C" int mi_adamw_bf16_multi(const int64_t* table, int n_tensors, const int32_t* chunks, int n_chunks, int chunk_elems,
                                   const float* grad_scale, float lr, float beta1, float beta2, float eps, float weight_decay,
                                   int64_t step, void* stream) {
  if (int rc = check_multi(__func__, false, table && chunks, n_tensors, n_chunks, chunk_elems, step)) return rc;
  return launch_multi(__func__, mi::adamw_multi_kernel, table, n_tensors, chunks, n_chunks, chunk_elems, stream, grad_scale,
                      make_adam_args(lr, beta1, beta2, eps, weight_decay, step));
}

extern "C" int mi_adamw_cast_bf16_multi(const int64_t* table, int n_tensors, const int32_t* chunks, int n_chunks, int chunk_elems,
                                        const float* grad_scale, float lr, float beta1, float beta2, float eps, float weight_decay,
                                        int64_t step, void* stream) {
  if (int rc = check_multi(__func__, false, table && chunks, n_tensors, n_chunks, chunk_elems, step)) return rc;
  return launch_multi(__func__, mi::adamw_cast_multi_kernel<uint16_t>, table, n_tensors, chunks, n_chunks, chunk_elems, stream, grad_scale,
                      make_adam_args(lr, beta1, beta2, eps, weight_decay, step));
}

extern "C" int mi_adamw_mxcast_bf16_multi(const int64_t* table, int n_tensors, const int32_t* chunks, int n_chunks, int chunk_elems,
                                          const float* grad_scale, float lr, float beta1, float beta2, float eps, float weight_decay,
                                          int64_t step, void* stream) {
  if (int rc = check_multi(__func__, false, table && chunks, n_tensors, n_chunks, chunk_elems, step)) return rc;
  return launch_multi(__func__, mi::adamw_mxcast_multi_kernel<uint16_t>, table, n_tensors, chunks, n_chunks, chunk_elems, stream, grad_scale,
                      make_adam_args(lr, beta1, beta2, eps, weight_decay, step));
}

// fp32 optimiser state: the walks, the arithmetic and the FP8 emitters of the two kernels above, instantiated for an fp32 master
// weight and fp32 moments.  sink_kind 0 = the per-tensor table layout, 1 = the MXFP8 one.
extern "C" int mi_adamw_f32_multi(const int64_t* table, int n_tensors, const int32_t* chunks, int n_chunks, int chunk_elems,
                                  const float* grad_scale, float lr, float beta1, float beta2, float eps, float weight_decay,
                                  int64_t step, int sink_kind, void* stream) {
  if (int rc = check_multi(__func__, true, table && chunks, n_tensors, n_chunks, chunk_elems, step, sink_kind)) return rc;
  return launch_multi(__func__, sink_kind == 0 ? mi::adamw_cast_multi_kernel<float> : mi::adamw_mxcast_multi_kernel<float>, table, n_tensors,
                      chunks, n_chunks, chunk_elems, stream, grad_scale, make_adam_args(lr, beta1, beta2, eps, weight_decay, step));
}

// bf16 state with stochastic rounding: the SR instantiations of the same two kernels
extern "C" int mi_adamw_sr_bf16_multi(const int64_t* table, int n_tensors, const int32_t* chunks, int n_chunks, int chunk_elems,
                                      const float* grad_scale, float lr, float beta1, float beta2, float eps, float weight_decay,
                                      int64_t step, int sink_kind, uint64_t seed, void* stream) {
  if (int rc = check_multi(__func__, true, table && chunks, n_tensors, n_chunks, chunk_elems, step, sink_kind)) return rc;
  mi::AdamSrArgs a;
  static_cast<mi::AdamArgs&>(a) = make_adam_args(lr, beta1, beta2, eps, weight_decay, step);
  a.k0 = (mi::u32)(seed & 0xFFFFFFFFull);
  a.k1 = (mi::u32)(seed >> 32);
  a.step = (mi::u32)((uint64_t)step & 0xFFFFFFFFull);
  return launch_multi(__func__, sink_kind == 0 ? mi::adamw_cast_multi_kernel<uint16_t, true> : mi::adamw_mxcast_multi_kernel<uint16_t, true>,
                      table, n_tensors, chunks, n_chunks, chunk_elems, stream, grad_scale, a);
}

// fp32 gradient accumulation: one launch per micro-batch (include/mi_fp8.h)
extern "C" int mi_grad_accum_multi(const int64_t* table, int n_tensors, const int32_t* chunks, int n_chunks, int chunk_elems,
                                   void* stream) {
  if (int rc = check_multi(__func__, true, table && chunks, n_tensors, n_chunks, chunk_elems, 1)) return rc;
  return launch_multi(__func__, mi::grad_accum_multi_kernel, table, n_tensors, chunks, n_chunks, chunk_elems, stream);
}

extern "C" int mi_sumsq_bf16(const void* g_bf16, int64_t n, float* partial, int n_partials, void* stream) {
  MI_CHECK_ARG(g_bf16 && partial, "mi_sumsq_bf16: null pointer");
  MI_CHECK_ARG(n >= 0 && n_partials >= 1 && n_partials <= 65535, "mi_sumsq_bf16: bad sizes");
  hipLaunchKernelGGL(mi::sumsq_kernel, dim3(n_partials), dim3(256), 0, (hipStream_t)stream, (const uint16_t*)g_bf16, n, partial);
  MI_CHECK_LAUNCH("mi_sumsq_bf16 launch");
  return MI_OK;
}

extern "C" int mi_adamw_bf16(void* p_bf16, const void* g_bf16, void* exp_avg_bf16, void* exp_avg_sq_bf16, int64_t n,
                             const float* grad_scale, float lr, float beta1, float beta2, float eps, float weight_decay,
                             int64_t step, void* stream) {
  MI_CHECK_ARG(p_bf16 && g_bf16 && exp_avg_bf16 && exp_avg_sq_bf16, "mi_adamw_bf16: null pointer");
  MI_CHECK_ARG(n >= 0 && step >= 1, "mi_adamw_bf16: bad n / step");
  if (n == 0) return MI_OK;
  const mi::AdamArgs a = make_adam_args(lr, beta1, beta2, eps, weight_decay, step);
  int64_t blocks = ((n >> 3) + 255) / 256;
  if (blocks < 1) blocks = 1;
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(mi::adamw_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (uint16_t*)p_bf16,
                     (const uint16_t*)g_bf16, (uint16_t*)exp_avg_bf16, (uint16_t*)exp_avg_sq_bf16, n, grad_scale, a);
  MI_CHECK_LAUNCH("mi_adamw_bf16 launch");
  return MI_OK;
}

extern "C" int mi_embedding_grad_add(void* grad_bf16, const void* dy_bf16, const int64_t* sorted_ids, const int64_t* perm,
                                     int64_t tokens, int64_t hidden, int64_t vocab, float alpha, int64_t padding_idx, void* stream) {
  MI_CHECK_ARG(grad_bf16 && dy_bf16 && sorted_ids && perm, "mi_embedding_grad_add: null pointer");
  MI_CHECK_ARG(tokens >= 0 && tokens < (1LL << 31) && hidden > 0 && hidden % 8 == 0 && hidden < (1LL << 31) && vocab > 0,
               "mi_embedding_grad_add: bad shape (hidden a multiple of 8)");
  MI_CHECK_ARG(((uintptr_t)grad_bf16 % 16) == 0 && ((uintptr_t)dy_bf16 % 16) == 0, "mi_embedding_grad_add: misaligned pointer");
  if (tokens == 0) return MI_OK;
  hipLaunchKernelGGL(mi::embedding_grad_add_kernel, dim3((unsigned)tokens), dim3(256), 0, (hipStream_t)stream, (uint16_t*)grad_bf16,
                     (const uint16_t*)dy_bf16, sorted_ids, perm, (int)tokens, (int)hidden, vocab, alpha, padding_idx);
  MI_CHECK_LAUNCH("mi_embedding_grad_add launch");
  return MI_OK;
}
