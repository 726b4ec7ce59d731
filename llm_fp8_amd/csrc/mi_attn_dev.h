// Device helpers shared by the attention kernels (mi_attn.hip: S >= 128; mi_attn_short.hip: S <= 112): the XOR-swizzled bf16
// tile image in LDS, the row and transposed (ds_read_b64_tr_b16) fragment readers of the 32x32x16 MFMA operands, the
// accumulator -> bf16 fragment conversion, the LDS-DMA staging of K / V tiles and the accumulator -> bf16 row store.
#pragma once
#include "mi_common.h"

namespace mi {

typedef __bf16 bf8 __attribute__((ext_vector_type(8)));
typedef short s4v __attribute__((ext_vector_type(4)));
typedef short s8v __attribute__((ext_vector_type(8)));
typedef float f16v __attribute__((ext_vector_type(16)));
typedef __attribute__((address_space(3))) s4v lds_s4v;

// byte offset of 16-byte chunk `ch` of row `row` in a [rows][D] bf16 tile image; the XOR keeps both the ds_read_b128 row
// reads and the ds_read_b64_tr_b16 transposed reads of the 32x32x16 operands spread over the banks
template <int D>
__device__ __forceinline__ int tile_off(int row, int ch) {
  if (D == 128) return 256 * row + 16 * (ch ^ (((row & 3) << 2) | ((row >> 2) & 3)));
  return 128 * row + 16 * (ch ^ (((row & 1) << 2) | ((row >> 1) & 3)));
}

__device__ __forceinline__ bf8 as_bf8(v4i v) { return __builtin_bit_cast(bf8, v); }

// row fragment of the 32x32x16 A/B operand: lane (r, h) <- row r0 + r, elements [16 t + 8 h, +8)
template <int D>
__device__ __forceinline__ bf8 row_frag(const char* tile, int r0, int t, int lane) {
  const int r = lane & 31, h = lane >> 5;
  return as_bf8(*reinterpret_cast<const v4i*>(tile + tile_off<D>(r0 + r, 2 * t + h)));
}

// transposed fragment: lane (c = lane & 31, h) <- column c0 + c, rows {rb, rb+1, rb+2, rb+3, rb+8, .., rb+11}, rb = r0 + 4 h:
// exactly the row set a 32x32 accumulator keeps in registers 8 s .. 8 s + 7 (r0 = 16 s)
template <int D>
__device__ __forceinline__ bf8 tr_frag(const char* tile, int r0, int c0, int lane) {
  const int i16 = lane & 15, qq = i16 >> 2, pp = i16 & 3, half = (lane >> 4) & 1, h = lane >> 5;
  const int ch = (c0 >> 3) + 2 * half + (pp >> 1);
  const int rb = r0 + 4 * h + qq;
  const s4v lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4v*)(tile + tile_off<D>(rb, ch) + 8 * (pp & 1)));
  const s4v hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4v*)(tile + tile_off<D>(rb + 8, ch) + 8 * (pp & 1)));
  s8v v;
  v[0] = lo[0]; v[1] = lo[1]; v[2] = lo[2]; v[3] = lo[3]; v[4] = hi[0]; v[5] = hi[1]; v[6] = hi[2]; v[7] = hi[3];
  return __builtin_bit_cast(bf8, v);
}

// accumulator registers 8 s .. 8 s + 7 -> bf16 fragment (B operand of a product that sums over the accumulator's rows)
__device__ __forceinline__ bf8 acc_frag(const f16v& a, int s) {
  v4i v;
#pragma unroll
  for (int j = 0; j < 4; ++j) v[j] = (int)pack_bf16x2(a[8 * s + 2 * j], a[8 * s + 2 * j + 1]);
  return as_bf8(v);
}

__device__ __forceinline__ int acc_row(int reg, int h) { return (reg & 3) + 8 * (reg >> 2) + 4 * h; }

// Packed sequences (SEG in mi_attn.hip): token t's document as the kernels use it.  Whatever the arrays hold, the document starts
// in [0, t] and ends in [t + 1, S]: a token always sees itself, and nothing derived from these values leaves the row.
__device__ __forceinline__ int seg_lo(const int32_t* __restrict__ seg_start, int t) { return min(max(seg_start[t], 0), t); }
__device__ __forceinline__ int seg_hi(const int32_t* __restrict__ seg_end, int t, int S) { return min(max(seg_end[t], t + 1), S); }

// Make a prologue load complete HERE (a use the compiler cannot move): left alone, such loads sink towards their first use
// inside the tile loop, and the s_waitcnt vmcnt placed there also waits -- the counter is in-order -- for the NEXT tile's
// just-issued prefetch loads, every tile.
__device__ __forceinline__ void retire(bf8& f) {
  v4i tmp = __builtin_bit_cast(v4i, f);
  asm volatile("" : "+v"(tmp));
  f = as_bf8(tmp);
}
__device__ __forceinline__ void retire(float& f) { asm volatile("" : "+v"(f)); }

// LDS-DMA staging (buffer_load_dwordx4 ... lds): a wave-wide instruction deposits 64 x 16 bytes at consecutive LDS addresses,
// so the tile image's XOR swizzle is applied on the GLOBAL side: lane l of this wave's i-th instruction fetches the chunk
// (row, ch) whose image slot is byte (4 i + w) 1024 + 16 l.  No staging registers, no ds_write, no VALU address math per tile
// (per-lane voffset fixed for the kernel, tile advance in the scalar offset).
typedef __amdgpu_buffer_rsrc_t rsrc_t;
#define MI_LDS_PTR(p) ((__attribute__((address_space(3))) void*)(p))
template <int D>
__device__ __forceinline__ void dma_voffsets(int* voff, int64_t tok_stride, int tid) {
  const int lane = tid & 63, w = tid >> 6;
#pragma unroll
  for (int i = 0; i < D / 32; ++i) {
    const int p = (4 * i + w) * 1024 + 16 * lane;
    const int row = p / (2 * D), slot = (p % (2 * D)) / 16;
    const int ch = D == 128 ? slot ^ (((row & 3) << 2) | ((row >> 2) & 3)) : slot ^ (((row & 1) << 2) | ((row >> 1) & 3));
    voff[i] = (int)((int64_t)row * tok_stride * 2) + 16 * ch;
  }
}
template <int D>
__device__ __forceinline__ void stage_dma(rsrc_t rs, const int* voff, int soff, char* tile, int w) {
#pragma unroll
  for (int i = 0; i < D / 32; ++i)
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, MI_LDS_PTR(tile + (4 * i + w) * 1024), 16, voff[i], soff, 0, 0);
}
// TAIL form: the tile advance goes into the per-lane offset, the part of the address that the buffer's range check sees, so a
// row at or past S (past num_records) is not fetched and its 16 bytes of the image are zeros
template <int D>
__device__ __forceinline__ void stage_dma_checked(rsrc_t rs, const int* voff, int adv, char* tile, int w) {
#pragma unroll
  for (int i = 0; i < D / 32; ++i)
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, MI_LDS_PTR(tile + (4 * i + w) * 1024), 16, (int)((u32)voff[i] + (u32)adv), 0, 0, 0);
}
template <int D, bool TAIL>
__device__ __forceinline__ void stage_tile(rsrc_t rs, const int* voff, int adv, char* tile, int w) {
  if (TAIL) stage_dma_checked<D>(rs, voff, adv, tile, w);
  else stage_dma<D>(rs, voff, adv, tile, w);
}
__device__ __forceinline__ void dma_wait_all() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }

// O^T-style accumulators (d in registers, row index on the lane) -> bf16 rows of `out` through a wave-private LDS slice
// (TAIL: only the first `nrows` rows are stored; nrows <= 0 stores nothing)
template <int D, bool TAIL = false>
__device__ __forceinline__ void store_rows_from_accT(const f16v (&acc)[D / 32], float mul, char* slice, uint16_t* out,
                                                     int64_t row_stride, int lane, int nrows = 32) {
  const int r = lane & 31, h = lane >> 5;
  constexpr int CPR = D / 8;
#pragma unroll
  for (int d = 0; d < D / 32; ++d)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int ch = 4 * d + i;
      uint2 pk;
      pk.x = pack_bf16x2(acc[d][4 * i] * mul, acc[d][4 * i + 1] * mul);
      pk.y = pack_bf16x2(acc[d][4 * i + 2] * mul, acc[d][4 * i + 3] * mul);
      *reinterpret_cast<uint2*>(slice + r * (D * 2) + 16 * (ch ^ (r & (CPR - 1))) + 8 * h) = pk;
    }
  __builtin_amdgcn_s_waitcnt(0xc07f);
  __builtin_amdgcn_wave_barrier();
#pragma unroll
  for (int it = 0; it < 32 * CPR / 64; ++it) {
    const int idx = it * 64 + lane, row = idx / CPR, ch = idx % CPR;
    const v4i val = *reinterpret_cast<const v4i*>(slice + row * (D * 2) + 16 * (ch ^ (row & (CPR - 1))));
    if (!TAIL || row < nrows) *reinterpret_cast<v4i*>(out + (int64_t)row * row_stride + ch * 8) = val;
  }
}

}  // namespace mi
