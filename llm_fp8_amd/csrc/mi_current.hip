// Current scaling (Float8CurrentScaling): the per-tensor scale comes from the amax of the tensor that is about to be cast, so the
// amax has to exist BEFORE the cast runs.  Two kernels in front of the existing cast kernels (which take `scale` as a device pointer):
//
//   amax pass    read-only, HBM-bound (2 B per element for the plain form).  The walk of cast_amax_kernel (mi_cast.hip): every WAVE
//                walks 64-column tiles with stride = waves in the grid, 16-byte loads, the loads of its NEXT tile in flight while the
//                current one is reduced; wave reduction (DPP) -> LDS across the 4 waves -> ONE plain store per workgroup into
//                partial[blockIdx.x].  No atomics and no slot to zero first: every workgroup of the grid writes its entry (0 when it
//                had no tile), so the launch count per tensor is amax + scale + cast = 3, with no fill.
//                MODE 0  |x|                                  (mi_cast_amax)
//                MODE 1  |(x * rstd[r]) * gamma[c]|           (mi_norm_cast; norm_value2)
//                MODE 2  |silu(g) * u|                        (mi_swiglu_cast(_bias); swiglu_value2<0>)
//                MODE 3  |d * dsilu(g) * u|, |d * silu(g)|    (mi_dswiglu_cast(_bias); swiglu_value2<1>)
//                The fused modes call the value helpers of mi_common.h that the cast kernels call: the bf16 value is never
//                materialised, so the pass recomputes exactly what the cast will see.  NaN elements are ignored and Inf gives Inf,
//                as in the cast kernels' own amax.
//   scale kernel one workgroup: max over the partials, then TE's compute_scale_from_amax -> [amax, scale, scale_inv].
//
// MI_AMAX_NT (build-time): nontemporal (1) or plain (0, the product) loads in the amax pass.  The cast that follows re-reads the same
// tensor, and behind plain loads it finds more of it on the die: 8192 x 3072 takes 10.0 us plain against 12.3 us nontemporal alone,
// and the pair amax + mi_cast_amax 32.7 us against 37.2 us (the cast alone: 31.1 us; profiles/current_scaling.txt).
#include "mi_common.h"

#ifndef MI_AMAX_NT
#define MI_AMAX_NT 0
#endif

namespace mi {

template <bool NT>
__device__ __forceinline__ v4i ld16(const uint16_t* p) {
  if (NT) return __builtin_nontemporal_load(reinterpret_cast<const v4i*>(p));
  return *reinterpret_cast<const v4i*>(p);
}

__device__ __forceinline__ float amax_acc(float amax, float v) { return fmaxf(amax, (v != v) ? 0.0f : fabsf(v)); }

// A lane owns RPL rows x 8 columns of a tile of (8 * RPL) rows x 64 columns (8 lanes cover one 128-byte line of a row).  RPL = 8
// for the one-input modes (the cast kernels' 64 x 64 tile) and 4 where a tile has two or three inputs, so that the current tile and
// the prefetched one stay inside 128 VGPRs.  `cols` is the width of the walked space: the gate space [rows, F] for MODE 2 / 3.
template <int MODE, bool NT>
__global__ __launch_bounds__(256) void amax_kernel(const uint16_t* __restrict__ x, const uint16_t* __restrict__ d,
                                                   const float* __restrict__ rstd, const uint16_t* __restrict__ vec,
                                                   float* __restrict__ partial, int rows, int cols, int tiles_c) {
  constexpr int RPL = MODE <= 1 ? 8 : 4;
  constexpr int TR = 8 * RPL;
  constexpr int NIN = MODE == 3 ? 3 : (MODE == 2 ? 2 : 1);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ntiles = ((rows + TR - 1) / TR) * tiles_c;
  const int stride = gridDim.x * 4;
  const int lr = (lane >> 3) * RPL, lc = (lane & 7) * 8;
  const int64_t ldx = MODE >= 2 ? 2 * (int64_t)cols : (int64_t)cols;  // h is [rows, 2F]
  float amax = 0.0f;
  int t = blockIdx.x * 4 + wave;
  v4i nxt[NIN][RPL], nxt_v[2];
  v4f nxt_r[2];
  auto load_tile = [&](int tt, v4i (&raw)[NIN][RPL], v4i (&vv)[2], v4f (&rs)[2]) {
    const int r0 = (tt / tiles_c) * TR + lr, c0 = (tt % tiles_c) * 64 + lc;
    if (r0 < rows && c0 < cols) {  // rows, cols are multiples of 8 (and RPL divides 8): blocks are all-in or all-out
      const uint16_t* src = x + (int64_t)r0 * ldx + c0;
#pragma unroll
      for (int i = 0; i < RPL; ++i) {
        raw[0][i] = ld16<NT>(src + (int64_t)i * ldx);
        if (MODE >= 2) raw[1][i] = ld16<NT>(src + (int64_t)i * ldx + cols);
        if (MODE == 3) raw[NIN - 1][i] = ld16<NT>(d + ((int64_t)r0 + i) * cols + c0);
      }
      if (MODE == 1) {  // gamma slice and the 8 row statistics
        vv[0] = *reinterpret_cast<const v4i*>(vec + c0);
        rs[0] = *reinterpret_cast<const v4f*>(rstd + r0);
        rs[1] = *reinterpret_cast<const v4f*>(rstd + r0 + 4);
      }
      if (MODE >= 2 && vec != nullptr) {  // fc1 bias: gate slice, up slice
        vv[0] = *reinterpret_cast<const v4i*>(vec + c0);
        vv[1] = *reinterpret_cast<const v4i*>(vec + cols + c0);
      }
    } else {
#pragma unroll
      for (int n = 0; n < NIN; ++n)
#pragma unroll
        for (int i = 0; i < RPL; ++i) raw[n][i] = (v4i){0, 0, 0, 0};
    }
  };
  nxt_v[0] = nxt_v[1] = (v4i){0, 0, 0, 0};
  nxt_r[0] = nxt_r[1] = (v4f){0.f, 0.f, 0.f, 0.f};
  if (t < ntiles) load_tile(t, nxt, nxt_v, nxt_r);
  while (t < ntiles) {
    v4i raw[NIN][RPL];
#pragma unroll
    for (int n = 0; n < NIN; ++n)
#pragma unroll
      for (int i = 0; i < RPL; ++i) raw[n][i] = nxt[n][i];
    const v4i v0 = nxt_v[0], v1 = nxt_v[1];
    const v4f rs0 = nxt_r[0], rs1 = nxt_r[1];
    const int tn = t + stride;
    if (tn < ntiles) load_tile(tn, nxt, nxt_v, nxt_r);
    // (a lane outside the tensor holds zeros in `raw`: |0| leaves the maximum alone in MODE 0; the fused modes skip it, since
    // their value of a zero input need not be zero under a bias)
    if (MODE == 0) {
      // the raw bf16 magnitudes order like unsigned integers: packed u16 max, NaN-screened as in cast_amax_kernel
      u32 screen = 0;
#pragma unroll
      for (int i = 0; i < RPL; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) screen = nan_screen(screen, (u32)raw[0][i][j]);
      if (__builtin_expect(nan_seen(screen), 0)) {
#pragma unroll
        for (int i = 0; i < RPL; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const u32 w = (u32)raw[0][i][j];
            amax = amax_acc(amax, __uint_as_float(w << 16));
            amax = amax_acc(amax, __uint_as_float(w & 0xFFFF0000u));
          }
      } else {
        amax = fmaxf(amax, __uint_as_float(max(screen & 0xFFFFu, screen >> 16) << 16));
      }
    } else {
      const int r0 = (t / tiles_c) * TR + lr, c0 = (t % tiles_c) * 64 + lc;
      if (r0 < rows && c0 < cols) {
        float a[8], b[8];  // MODE 1: gamma; MODE 2 / 3: bias of the gate half, of the up half
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          a[2 * j] = __uint_as_float((u32)v0[j] << 16);
          a[2 * j + 1] = __uint_as_float((u32)v0[j] & 0xFFFF0000u);
          b[2 * j] = __uint_as_float((u32)v1[j] << 16);
          b[2 * j + 1] = __uint_as_float((u32)v1[j] & 0xFFFF0000u);
        }
#pragma unroll
        for (int i = 0; i < RPL; ++i) {
          if (MODE == 1) {
            const float rs = i < 4 ? rs0[i & 3] : rs1[i & 3];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              float f0, f1;
              norm_value2((u32)raw[0][i][j], rs, a[2 * j], a[2 * j + 1], f0, f1);
              amax = amax_acc(amax_acc(amax, f0), f1);
            }
          } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              const u32 wg = (u32)raw[0][i][j], wu = (u32)raw[NIN > 1 ? 1 : 0][i][j], wd = (u32)raw[NIN - 1][i][j];
              float f0[2] = {0.0f, 0.0f}, f1[2] = {0.0f, 0.0f};
              swiglu_value2<(MODE == 3 ? 1 : 0)>(wg, wu, wd, vec != nullptr, a + 2 * j, b + 2 * j, f0, f1);
              amax = amax_acc(amax_acc(amax, f0[0]), f0[1]);
              if (MODE == 3) amax = amax_acc(amax_acc(amax, f1[0]), f1[1]);
            }
          }
        }
      }
    }
    t = tn;
  }
  amax = block_max(amax);
  if (tid == 0) partial[blockIdx.x] = amax;
}

// TE's compute_scale_from_amax on the maximum of the partials; out3 = {amax, scale, scale_inv}
__global__ __launch_bounds__(256) void current_scale_kernel(const float* __restrict__ partial, int n, float fp8_max, float eps,
                                                            int pow2, float* __restrict__ out3) {
  const int tid = threadIdx.x;
  float m = 0.0f;
  for (int i = tid; i < n; i += 256) m = fmaxf(m, partial[i]);  // (the passes never write a NaN)
  const float amax = block_max(m);
  if (tid == 0) {
    const float scale = scale_from_amax(amax, fp8_max, eps, pow2 != 0);
    out3[0] = amax;
    out3[1] = scale;
    out3[2] = 1.0f / scale;
  }
}

template <int MODE>
static int launch_amax(const char* who, const void* x, const void* d, const float* rstd, const void* vec, float* partial,
                       int n_partial, int64_t rows, int64_t cols, hipStream_t st) {
  constexpr int TR = MODE <= 1 ? 64 : 32;
  const int64_t tiles_c = (cols + 63) / 64;
  MI_CHECK_ARG(((rows + TR - 1) / TR) * tiles_c < (1LL << 31) - 4 * 1024, "%s: shape too large", who);
  hipLaunchKernelGGL((amax_kernel<MODE, MI_AMAX_NT != 0>), dim3((unsigned)n_partial), dim3(256), 0, st, (const uint16_t*)x,
                     (const uint16_t*)d, rstd, (const uint16_t*)vec, partial, (int)rows, (int)cols, (int)tiles_c);
  MI_CHECK_LAUNCH(who);
  return MI_OK;
}

static int amax_common_check(const char* who, const void* x, const float* partial, int n_partial, int64_t rows, int64_t cols,
                             int width = 1) {
  MI_CHECK_ARG(x && partial, "%s: null pointer", who);
  MI_CHECK_ARG(n_partial >= 1 && n_partial <= 1024, "%s: n_partial %d outside 1..1024", who, n_partial);
  MI_CHECK_ARG(rows >= 0 && cols >= 0 && rows % 8 == 0 && cols % 8 == 0, "%s: rows (%lld) and cols (%lld) must be multiples of 8", who,
               (long long)rows, (long long)cols);
  MI_CHECK_ARG(rows < (1LL << 31) && width * cols < (1LL << 31), "%s: shape too large", who);  // width 2: h is [rows, 2F]
  MI_CHECK_ARG(((uintptr_t)x % 16) == 0 && ((uintptr_t)partial % 4) == 0, "%s: misaligned pointer", who);
  return MI_OK;
}

}  // namespace mi

// (an empty tensor still launches: every one of the n_partial entries is written, with 0)
extern "C" int mi_amax_bf16(const void* x_bf16, float* partial, int n_partial, int64_t rows, int64_t cols, void* stream) {
  int rc = mi::amax_common_check("mi_amax_bf16", x_bf16, partial, n_partial, rows, cols);
  if (rc != MI_OK) return rc;
  return mi::launch_amax<0>("mi_amax_bf16", x_bf16, nullptr, nullptr, nullptr, partial, n_partial, rows, cols, (hipStream_t)stream);
}

extern "C" int mi_amax_norm(const void* x_bf16, const float* rstd, const void* gamma_bf16, float* partial, int n_partial, int64_t rows,
                            int64_t cols, void* stream) {
  int rc = mi::amax_common_check("mi_amax_norm", x_bf16, partial, n_partial, rows, cols);
  if (rc != MI_OK) return rc;
  MI_CHECK_ARG(rstd && gamma_bf16 && ((uintptr_t)rstd % 16) == 0 && ((uintptr_t)gamma_bf16 % 16) == 0,
               "mi_amax_norm: rstd and gamma must be non-null and 16-byte aligned");
  return mi::launch_amax<1>("mi_amax_norm", x_bf16, nullptr, rstd, gamma_bf16, partial, n_partial, rows, cols, (hipStream_t)stream);
}

extern "C" int mi_amax_swiglu(const void* h_bf16, const void* bias_bf16, float* partial, int n_partial, int64_t rows, int64_t F,
                              void* stream) {
  int rc = mi::amax_common_check("mi_amax_swiglu", h_bf16, partial, n_partial, rows, F, 2);
  if (rc != MI_OK) return rc;
  MI_CHECK_ARG(((uintptr_t)bias_bf16 % 16) == 0, "mi_amax_swiglu: bias must be 16-byte aligned");
  return mi::launch_amax<2>("mi_amax_swiglu", h_bf16, nullptr, nullptr, bias_bf16, partial, n_partial, rows, F, (hipStream_t)stream);
}

extern "C" int mi_amax_dswiglu(const void* h_bf16, const void* bias_bf16, const void* dact_bf16, float* partial, int n_partial,
                               int64_t rows, int64_t F, void* stream) {
  int rc = mi::amax_common_check("mi_amax_dswiglu", h_bf16, partial, n_partial, rows, F, 2);
  if (rc != MI_OK) return rc;
  MI_CHECK_ARG(dact_bf16 && ((uintptr_t)dact_bf16 % 16) == 0, "mi_amax_dswiglu: dact must be non-null and 16-byte aligned");
  MI_CHECK_ARG(((uintptr_t)bias_bf16 % 16) == 0, "mi_amax_dswiglu: bias must be 16-byte aligned");
  return mi::launch_amax<3>("mi_amax_dswiglu", h_bf16, dact_bf16, nullptr, bias_bf16, partial, n_partial, rows, F, (hipStream_t)stream);
}

extern "C" int mi_current_scale(const float* partial, int n_partial, float fp8_max, float amax_epsilon, int pow2, float* out3,
                                void* stream) {
  MI_CHECK_ARG(partial && out3, "mi_current_scale: null pointer");
  MI_CHECK_ARG(n_partial >= 1 && n_partial <= (1 << 20), "mi_current_scale: n_partial %d outside 1..2^20", n_partial);
  MI_CHECK_ARG(fp8_max > 0.0f && amax_epsilon >= 0.0f, "mi_current_scale: fp8_max must be positive and amax_epsilon non-negative");
  hipLaunchKernelGGL(mi::current_scale_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, partial, n_partial, fp8_max, amax_epsilon,
                     pow2, out3);
  MI_CHECK_LAUNCH("mi_current_scale launch");
  return MI_OK;
}
