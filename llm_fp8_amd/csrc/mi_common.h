// Shared device/host helpers for libmi_fp8 (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <float.h>
#include <stdint.h>
#include <stdio.h>
#include <stdarg.h>
#include "../../include/mi_fp8.h"

namespace mi {

// thread-local error string behind mi_last_error()
void set_error(const char* fmt, ...);
int hip_fail(hipError_t e, const char* what);

#define MI_CHECK_AS(rc, cond, ...)         \
  do {                                     \
    if (!(cond)) {                         \
      mi::set_error(__VA_ARGS__);          \
      return rc;                           \
    }                                      \
  } while (0)
#define MI_CHECK_ARG(cond, ...) MI_CHECK_AS(MI_ERR_ARG, cond, __VA_ARGS__)
#define MI_CHECK_SHAPE(cond, ...) MI_CHECK_AS(MI_ERR_SHAPE, cond, __VA_ARGS__)

#define MI_CHECK_LAUNCH(what)                                   \
  do {                                                          \
    hipError_t e__ = hipGetLastError();                         \
    if (e__ != hipSuccess) return mi::hip_fail(e__, what);      \
  } while (0)

typedef int v4i __attribute__((ext_vector_type(4)));
typedef unsigned int v4u __attribute__((ext_vector_type(4)));
typedef int v8i __attribute__((ext_vector_type(8)));
typedef float v4f __attribute__((ext_vector_type(4)));
typedef unsigned int u32;

__device__ __forceinline__ float bf16_bits_to_float(u32 b) { return __uint_as_float(b << 16); }

// fp32 -> bf16 bits, RNE, NaN kept (plain cast lowers to v_cvt_pk_bf16_f32 on gfx950)
__device__ __forceinline__ u32 float_to_bf16_bits(float f) {
  __bf16 h = (__bf16)f;
  return (u32)__builtin_bit_cast(unsigned short, h);
}
// two fp32 -> packed bf16x2 (RNE, NaN kept): one v_cvt_pk_bf16_f32
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ u32 pack_bf16x2(float lo, float hi) {
  f32x2 v = {lo, hi};
  return __builtin_bit_cast(u32, __builtin_convertvector(v, bf16x2));
}

template <int FMT>
__device__ __forceinline__ float fp8_max_of() { return FMT == MI_FMT_E4M3 ? 448.0f : 57344.0f; }

// Two fp32 -> two fp8 bytes in the low half of the result.  Inputs are clamped to +-max first,
// so the hardware converter only ever sees in-range finite values (RNE); NaN is patched to 0x7F
// by the caller.
template <int FMT>
__device__ __forceinline__ u32 cvt_pk_fp8(float a, float b) {
  const float mx = fp8_max_of<FMT>();
  a = __builtin_amdgcn_fmed3f(a, -mx, mx);
  b = __builtin_amdgcn_fmed3f(b, -mx, mx);
  if (FMT == MI_FMT_E4M3) return (u32)__builtin_amdgcn_cvt_pk_fp8_f32(a, b, 0, false) & 0xFFFFu;
  return (u32)__builtin_amdgcn_cvt_pk_bf8_f32(a, b, 0, false) & 0xFFFFu;
}

// 4 fp32 -> one dword of 4 fp8 bytes (byte i = v[i]); NaN -> 0x7F.
template <int FMT>
__device__ __forceinline__ u32 cvt4_fp8(float v0, float v1, float v2, float v3) {
  const float mx = fp8_max_of<FMT>();
  float c0 = __builtin_amdgcn_fmed3f(v0, -mx, mx), c1 = __builtin_amdgcn_fmed3f(v1, -mx, mx);
  float c2 = __builtin_amdgcn_fmed3f(v2, -mx, mx), c3 = __builtin_amdgcn_fmed3f(v3, -mx, mx);
  int r = 0;
  if (FMT == MI_FMT_E4M3) {
    r = __builtin_amdgcn_cvt_pk_fp8_f32(c0, c1, r, false);
    r = __builtin_amdgcn_cvt_pk_fp8_f32(c2, c3, r, true);
  } else {
    r = __builtin_amdgcn_cvt_pk_bf8_f32(c0, c1, r, false);
    r = __builtin_amdgcn_cvt_pk_bf8_f32(c2, c3, r, true);
  }
  u32 u = (u32)r;
  // rare path: canonical NaN byte
  if (__builtin_expect((v0 != v0) | (v1 != v1) | (v2 != v2) | (v3 != v3), 0)) {
    if (v0 != v0) u = (u & 0xFFFFFF00u) | 0x0000007Fu;
    if (v1 != v1) u = (u & 0xFFFF00FFu) | 0x00007F00u;
    if (v2 != v2) u = (u & 0xFF00FFFFu) | 0x007F0000u;
    if (v3 != v3) u = (u & 0x00FFFFFFu) | 0x7F000000u;
  }
  return u;
}

// NaN screen on raw bf16 pairs: running packed-u16 max of the magnitudes; any lane value > 0x7F80
// afterwards means "this thread saw a NaN".  (v_max_f32 in IEEE mode turns max(a, sNaN) into qNaN
// and so forgets `a`; threads that saw a NaN take a sanitising slow path instead.)
typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ u32 nan_screen(u32 acc, u32 w) {
  u16x2 a = __builtin_bit_cast(u16x2, acc), b = __builtin_bit_cast(u16x2, w & 0x7FFF7FFFu);
  return __builtin_bit_cast(u32, __builtin_elementwise_max(a, b));
}
__device__ __forceinline__ bool nan_seen(u32 acc) { return max(acc & 0xFFFFu, acc >> 16) > 0x7F80u; }

// v_perm_b32: result byte i = byte sel[i] of the 8-byte pool {lo = bytes 0..3, hi = bytes 4..7}
__device__ __forceinline__ u32 bperm(u32 hi, u32 lo, u32 sel) { return __builtin_amdgcn_perm(hi, lo, sel); }

// 4x4 byte transpose: in r[i] = row i (byte j = col j) -> out c[j] = col j (byte i = row i)
__device__ __forceinline__ void transpose4x4(u32 r0, u32 r1, u32 r2, u32 r3, u32& c0, u32& c1, u32& c2,
                                             u32& c3) {
  u32 t01l = bperm(r1, r0, 0x05010400u);  // [r0b0, r1b0, r0b1, r1b1]
  u32 t01h = bperm(r1, r0, 0x07030602u);  // [r0b2, r1b2, r0b3, r1b3]
  u32 t23l = bperm(r3, r2, 0x05010400u);
  u32 t23h = bperm(r3, r2, 0x07030602u);
  c0 = bperm(t23l, t01l, 0x05040100u);  // [t01l.b0, t01l.b1, t23l.b0, t23l.b1]
  c1 = bperm(t23l, t01l, 0x07060302u);
  c2 = bperm(t23h, t01h, 0x05040100u);
  c3 = bperm(t23h, t01h, 0x07060302u);
}

// E8M0 biased exponent of (amax * 1/fp8_max), rounded up to the next power of two.
__device__ __forceinline__ u32 e8m0_roundup(float val) {
  u32 u = __float_as_uint(val);
  u32 e = (u >> 23) & 0xFFu, man = u & 0x7FFFFFu;
  if (man > 0 && e != 0xFEu && !(e == 0 && man <= 0x400000u)) ++e;
  if (val != val) e = 0xFFu;
  else if (isinf(val)) e = 0xFEu;
  else if (val == 0.0f) e = 0u;
  return e;
}
// 2^(127 - e) as fp32 (exact; subnormal for e = 254, NaN for e = 255)
__device__ __forceinline__ float e8m0_inv(u32 e) {
  if (e == 0xFFu) return __uint_as_float(0x7FC00000u);
  if (e == 0xFEu) return __uint_as_float(0x00400000u);
  return __uint_as_float((254u - e) << 23);
}

// TE's compute_scale_from_amax: fp8_max / max(amax, eps), 1 where that is no finite number; `pow2` rounds it DOWN to a power of
// two.  The per-tensor scale of current scaling (mi_current.hip) and the block scales of Float8BlockScaling (mi_mxfp8.hip).
__device__ __forceinline__ float scale_from_amax(float amax, float fp8_max, float eps, bool pow2) {
  const float a = amax < eps ? eps : amax;
  float scale = 1.0f;
  if (!(a == 0.0f) && !isinf(a)) {
    scale = fp8_max / a;  // IEEE fp32 division (no fast-math in this build)
    if (isinf(scale)) scale = FLT_MAX;
    if (scale != scale) scale = 1.0f;
  }
  if (pow2) scale = __uint_as_float(__float_as_uint(scale) & 0xFF800000u);  // mantissa cleared
  return scale;
}

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
  return v;
}

// The fp32 value `v` a fused cast kernel multiplies by *scale, per element.  The cast kernels (mi_fused.hip) and the amax passes of
// current scaling (mi_current.hip) both call these: an amax pass must see exactly the value the cast that follows will quantise.
__device__ __forceinline__ float sigmoidf_(float g) { return 1.0f / (1.0f + __expf(-g)); }

// mi_norm_cast: the two bf16 halves of the packed word `w` of row statistics `rs`, times their gamma
__device__ __forceinline__ void norm_value2(u32 w, float rs, float g0, float g1, float& v0, float& v1) {
  v0 = (__uint_as_float(w << 16) * rs) * g0;
  v1 = (__uint_as_float(w & 0xFFFF0000u) * rs) * g1;
}

// mi_swiglu_cast(_bias) (MODE 0): v0 = silu(g) * u.  mi_dswiglu_cast(_bias) (MODE 1): v0 = d * dsilu(g) * u (gate half),
// v1 = d * silu(g) (up half).  For the two bf16 halves of the packed words wg (gate), wu (up), wd (dact); `has_bias` (wave-uniform):
// the fc1 bias bg[0..1] / bu[0..1] is added, in fp32, to the unpacked gate / up values first.  MODE 0 leaves v1 alone.
template <int MODE>
__device__ __forceinline__ void swiglu_value2(u32 wg, u32 wu, u32 wd, bool has_bias, const float* bg, const float* bu, float* v0,
                                              float* v1) {
  float g2[2] = {__uint_as_float(wg << 16), __uint_as_float(wg & 0xFFFF0000u)};
  float u2[2] = {__uint_as_float(wu << 16), __uint_as_float(wu & 0xFFFF0000u)};
  const float d2[2] = {__uint_as_float(wd << 16), __uint_as_float(wd & 0xFFFF0000u)};
  if (has_bias) {
    g2[0] += bg[0];
    g2[1] += bg[1];
    u2[0] += bu[0];
    u2[1] += bu[1];
  }
#pragma unroll
  for (int e = 0; e < 2; ++e) {
    const float sg = sigmoidf_(g2[e]);
    if (MODE == 0) {
      v0[e] = g2[e] * sg * u2[e];
    } else {
      v0[e] = d2[e] * u2[e] * (sg * (1.0f + g2[e] * (1.0f - sg)));
      v1[e] = d2[e] * (g2[e] * sg);
    }
  }
}

}  // namespace mi
// 8-byte FP8 stores of the cast / quantise kernels (one 8 x 8 block per lane: 8 lanes = one 64-byte row segment).
// MI_NT_Y / MI_NT_YT (build-time, timing experiments): nontemporal stores for the row-major / the transposed copy.
#ifndef MI_NT_Y
#define MI_NT_Y 0
#endif
#ifndef MI_NT_YT
#define MI_NT_YT 0
#endif
#if defined(__HIPCC__)
namespace mi {
template <bool NT>
__device__ __forceinline__ void st8(uint8_t* p, unsigned int a, unsigned int b) {
  typedef unsigned int v2u_st8 __attribute__((ext_vector_type(2)));
  const v2u_st8 w = {a, b};
  if (NT) __builtin_nontemporal_store(w, reinterpret_cast<v2u_st8*>(p));
  else *reinterpret_cast<v2u_st8*>(p) = w;
}

// A lane's 8 x 8 block of FP8 bytes (row i: lo[i] = columns 0..3, hi[i] = columns 4..7), row-major: row i at dst + i * ld.
template <bool NT>
__device__ __forceinline__ void store_rows8(uint8_t* dst, int64_t ld, const u32 (&lo)[8], const u32 (&hi)[8]) {
#pragma unroll
  for (int i = 0; i < 8; ++i) st8<NT>(dst + i * ld, lo[i], hi[i]);
}
// The same block transposed in registers and stored column-major: column j (its 8 rows = 8 bytes) at dst + j * ld.
template <bool NT>
__device__ __forceinline__ void store_cols8(uint8_t* dst, int64_t ld, const u32 (&lo)[8], const u32 (&hi)[8]) {
  u32 a[4], b[4], c[4], d[4];
  transpose4x4(lo[0], lo[1], lo[2], lo[3], a[0], a[1], a[2], a[3]);  // cols 0..3, rows 0..3
  transpose4x4(lo[4], lo[5], lo[6], lo[7], b[0], b[1], b[2], b[3]);  // cols 0..3, rows 4..7
  transpose4x4(hi[0], hi[1], hi[2], hi[3], c[0], c[1], c[2], c[3]);  // cols 4..7, rows 0..3
  transpose4x4(hi[4], hi[5], hi[6], hi[7], d[0], d[1], d[2], d[3]);  // cols 4..7, rows 4..7
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    st8<NT>(dst + j * ld, a[j], b[j]);
    st8<NT>(dst + (j + 4) * ld, c[j], d[j]);
  }
}

// max of `v` over the 4 waves of a 256-thread workgroup.  Holds a barrier: every thread of the workgroup calls it.
__device__ __forceinline__ float block_max(float v) {
  __shared__ float s_max[4];
  v = wave_max(v);
  if ((threadIdx.x & 63) == 0) s_max[threadIdx.x >> 6] = v;
  __syncthreads();
  return fmaxf(fmaxf(s_max[0], s_max[1]), fmaxf(s_max[2], s_max[3]));
}
// Per-tensor amax of a cast kernel: the workgroup's max goes into *amax_out with ONE atomicMax on the float's bit pattern
// (non-negative floats order like unsigned ints).  Every thread of the workgroup calls it; amax_out is workgroup-uniform.
__device__ __forceinline__ void publish_amax(float amax, float* amax_out) {
  if (amax_out == nullptr) return;
  const float m = block_max(amax);
  // only a workgroup that would raise the value goes to the atomic unit: same-address atomics are served one at a time and a
  // wave cannot retire before its atomic has returned (thousands of workgroups per launch)
  if (threadIdx.x == 0 && m > 0.0f && m > __builtin_nontemporal_load(amax_out))
    atomicMax(reinterpret_cast<unsigned int*>(amax_out), __float_as_uint(m));
}

// ---- MXFP8 block quantiser of a lane's 8 x 8 value block f (mxfp8_quant_kernel, adamw_mxcast_multi_kernel): one E8M0 scale per
// 32 elements, which span 4 neighbouring lanes.  The shuffles are executed by every lane (inactive lanes carry zeros).
// NaN -> 0 in f, recorded in the returned mask (bit 8 i + j): the block amax then needs no per-element test (fmaxf semantics:
// NaN ignored) and the byte is patched to 0x7F after the cast.
__device__ __forceinline__ unsigned long long mx_take_nans(float (&f)[8][8]) {
  unsigned long long nanmask = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < 8; ++j)
      if (f[i][j] != f[i][j]) {
        nanmask |= 1ull << (8 * i + j);
        f[i][j] = 0.0f;
      }
  return nanmask;
}
// bytes of a packed fp8 word (elements (i, j0..j0+3), bit0 = 8 i + j0) -> 0x7F where the mask says the source was a NaN (rare path)
__device__ __forceinline__ u32 mx_patch4(u32 w, unsigned long long nanmask, int bit0) {
  if (__builtin_expect(nanmask != 0, 0)) {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if ((nanmask >> (bit0 + k)) & 1) w = (w & ~(0xFFu << (8 * k))) | (0x7Fu << (8 * k));
  }
  return w;
}
// row-wise blocks (32 columns = lanes l, l^1, l^2, l^3): bytes lo / hi and the scale byte of each of the lane's 8 rows
template <int FMT>
__device__ __forceinline__ void mx_quant_rows(const float (&f)[8][8], unsigned long long nanmask, u32 (&lo)[8], u32 (&hi)[8],
                                              u32 (&sbytes)[8]) {
  const float rcp = 1.0f / fp8_max_of<FMT>();
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    float a = 0.0f;
#pragma unroll
    for (int j = 0; j < 8; ++j) a = fmaxf(a, fabsf(f[i][j]));
    a = fmaxf(a, __shfl_xor(a, 1));
    a = fmaxf(a, __shfl_xor(a, 2));
    const u32 e = e8m0_roundup(a * rcp);
    const float inv = e8m0_inv(e);
    sbytes[i] = e;
    lo[i] = mx_patch4(cvt4_fp8<FMT>(f[i][0] * inv, f[i][1] * inv, f[i][2] * inv, f[i][3] * inv), nanmask, 8 * i);
    hi[i] = mx_patch4(cvt4_fp8<FMT>(f[i][4] * inv, f[i][5] * inv, f[i][6] * inv, f[i][7] * inv), nanmask, 8 * i + 4);
  }
}
// column-wise blocks (32 rows = lanes l, l^8, l^16, l^24): the same bytes by row, and the scale byte of each of the 8 columns
template <int FMT>
__device__ __forceinline__ void mx_quant_cols(const float (&f)[8][8], unsigned long long nanmask, u32 (&lo)[8], u32 (&hi)[8],
                                              u32 (&sbytes)[8]) {
  const float rcp = 1.0f / fp8_max_of<FMT>();
  float inv[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    float a = 0.0f;
#pragma unroll
    for (int i = 0; i < 8; ++i) a = fmaxf(a, fabsf(f[i][j]));
    a = fmaxf(a, __shfl_xor(a, 8));
    a = fmaxf(a, __shfl_xor(a, 16));
    const u32 e = e8m0_roundup(a * rcp);
    sbytes[j] = e;
    inv[j] = e8m0_inv(e);
  }
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    lo[i] = mx_patch4(cvt4_fp8<FMT>(f[i][0] * inv[0], f[i][1] * inv[1], f[i][2] * inv[2], f[i][3] * inv[3]), nanmask, 8 * i);
    hi[i] = mx_patch4(cvt4_fp8<FMT>(f[i][4] * inv[4], f[i][5] * inv[5], f[i][6] * inv[6], f[i][7] * inv[7]), nanmask, 8 * i + 4);
  }
}
// block-major scales: the scale bytes of a lane's 8 rows / 8 columns are 8 contiguous bytes
__device__ __forceinline__ void store_scales8(uint8_t* p, const u32 (&s)[8]) {
  st8<false>(p, s[0] | (s[1] << 8) | (s[2] << 16) | (s[3] << 24), s[4] | (s[5] << 8) | (s[6] << 16) | (s[7] << 24));
}
}  // namespace mi

// The launch ladder of the kernels that emit y, yT or both, in E4M3 or E5M2: KERNEL<FMT, LEAD WRITE_Y, WRITE_T TRAIL>.  LEAD and
// TRAIL are the parenthesised template arguments between FMT and the two flags (each FOLLOWED by its comma) and behind the flags
// (each PRECEDED by its comma); "()" for none.  The rest is hipLaunchKernelGGL's argument list.  The callers have checked that
// fmt is one of the two and that an output is present.
#define MI_TARGS_(...) __VA_ARGS__
#define MI_LAUNCH_YT_(FMTv, has_y, has_t, KERNEL, LEAD, TRAIL, ...)                                           \
  do {                                                                                                        \
    if ((has_y) && (has_t)) hipLaunchKernelGGL((KERNEL<FMTv, MI_TARGS_ LEAD true, true MI_TARGS_ TRAIL>), __VA_ARGS__); \
    else if (has_y) hipLaunchKernelGGL((KERNEL<FMTv, MI_TARGS_ LEAD true, false MI_TARGS_ TRAIL>), __VA_ARGS__);        \
    else hipLaunchKernelGGL((KERNEL<FMTv, MI_TARGS_ LEAD false, true MI_TARGS_ TRAIL>), __VA_ARGS__);                   \
  } while (0)
#define MI_LAUNCH_FMT_YT(fmt, ...)                                    \
  do {                                                                \
    if ((fmt) == MI_FMT_E4M3) MI_LAUNCH_YT_(MI_FMT_E4M3, __VA_ARGS__); \
    else MI_LAUNCH_YT_(MI_FMT_E5M2, __VA_ARGS__);                      \
  } while (0)
#endif

