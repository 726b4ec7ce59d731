// Grouped FP8 GEMM: up to 4 independent "TN" problems D_p = (A_p . B_p^T) * alpha_p in ONE persistent launch.
//
// Why: a Linear's backward is two GEMMs on the same grad_output -- dgrad dX[M,K] = G8[M,N] . W8T[K,N]^T and wgrad
// dW[N,K] = G8T[N,M] . X8T[K,M]^T (te_llama.py:77,80 call sites).  Launched one after the other each pays its
// own ramp (first operand panels from beyond L2), its own exposed last epilogue (128 KiB of output per CU that nothing
// overlaps) and, worst, its own wave quantisation: 3072x8192 is 384 tiles = 1.5 rounds on 256 CUs, 3072x3072 is 0.56 round.
// Here the tiles of all problems form one list, longest tiles first, dealt round-robin to the persistent workgroups, so the
// short problem's tiles fill the holes of the long one's last round and the pipeline (LDS-DMA prefetch, distributed epilogue)
// runs straight across the problem boundary.
//
// Kernel = the persistent 8-phase kernel of mi_gemm.hip (same LDS image, same two-wave-group phase schedule, same distributed
// whole-line epilogue) with every per-problem quantity -- buffer descriptors, leading dimensions, K-tile count, alpha, output
// -- carried per prefetch cursor and switched at tile boundaries.  No bias: what dgrad / wgrad need.  All problems share the
// operand formats (FA, FB) and the tile shape.
//
// MX = true (mi_gemm_mxfp8_grouped) is the same kernel with the block-scale path of gemm_256_p8<MX> (mi_gemm.hip): one 256-byte
// LDS-DMA run of E8M0 scales per wave and K-tile (wave w: operand w >> 2, k-block w & 3) for the NEXT step at the head of phase
// 0, two 4-KiB scale slots at a 272-byte k-block stride, row-interleaved A fragments (PERM) so that a lane's fragment scales
// are one LDS read.  The scale descriptor, the scale row count and the scale row of the tile belong to the cursor's problem and
// switch at tile boundaries like rsA / rsB; all of it is wave-uniform.  alpha is 1: nothing of a problem is read up front.
#include "mi_gemm_dev.h"
#include <algorithm>
#include <cstring>
#include <map>
#include <mutex>
#include <type_traits>
#include <vector>

namespace mi {

// prefetch cursor: the (tile, K-tile) of a future step with everything needed to stage from it (wave-uniform)
struct Cursor {
  int ti, kt, nk, oa, ob, lda, ldb;
  rsrc_t rsA, rsB;
  rsrc_t rsS;  // MX: this wave's scale operand (SA: waves 0-3, SB: waves 4-7) of the cursor's problem
  int ss, so;  // MX: scale rows of that operand (M or N), and tile's first row + this wave's k-block * rows
  int va0, va1, vb0, vb1;  // per-lane byte offsets (row * ld + chunk) of the wave's first piece of each half-tile: recomputed
                           // only when the cursor enters a tile (the leading dimensions belong to the tile's problem)
};
// what the epilogue of a finished tile needs of its problem
struct Epi {
  rsrc_t rsD;
  int ldd, d_off;
  float alpha;
};

template <int FA, int FB, int MA1, int NB1, bool MX = false>
__global__ __launch_bounds__(512, 2) void gemm_256_grp(GroupArgs ga) {
  constexpr int RA0 = 64, RA1 = 16 * MA1, RB0 = 32, RB1 = 16 * NB1;
  constexpr int TBM = 2 * (RA0 + RA1), TBN = 4 * (RB0 + RB1);
  constexpr int nA1 = MA1 / 2, nB1 = NB1;
  constexpr int W = nA1 + nB1 + 4;
  constexpr int EX = MX ? 1 : 0;  // extra LDS-DMA op per K-tile at the head of phase 0 (the scales of the next step)
  constexpr bool PERM = MX;       // A fragments row-interleaved: fragment i, row slot s <-> row F * s + i of the half (mi_gemm.hip)
  // MX: behind the operand buffers, [2 slots of 4 KiB][operand A, B][4 k-blocks][272 B] of E8M0 scales.  (Same array on purpose: with
  // an array of their own hipcc put `s_waitcnt vmcnt(0)` in front of every fragment read.)
  constexpr int kSK = 272, kSOp = 4 * kSK, kSSlot = 4096;
  __shared__ __attribute__((aligned(16))) uint8_t lds[kLdsBytes + (MX ? 2 * kSSlot : 0)];
  uint8_t* const slds = lds + kLdsBytes;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wr = wave >> 2, wc = wave & 3;
  const int G = gridDim.x, bid = blockIdx.x;
  // virtual index: XCD-major order of the workgroups (round-robin dispatch over the 8 XCDs: bid & 7 names the L2)
  const int q8 = G >> 3, r8 = G & 7, xcd = bid & 7;
  const int v = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + (bid >> 3);
  int my_cnt[kMaxGroup], my_tiles = 0;
#pragma unroll
  for (int q = 0; q < kMaxGroup; ++q) {
    my_cnt[q] = q < ga.n ? (int)ga.cnt[q][v] : 0;
    my_tiles += my_cnt[q];
  }

  // alpha of every problem, read ONCE (inside the tile walk a memory read of it put `s_waitcnt vmcnt(0)` -- a drain of the whole
  // LDS-DMA pipeline -- at every tile boundary), kept as wave-uniform values
  float alpha_of[kMaxGroup];
#pragma unroll
  for (int q = 0; q < kMaxGroup; ++q) {
    float a = 1.0f;
    if (!MX && q < ga.n) a = (*ga.p[q].sa_inv) * (*ga.p[q].sb_inv);
    alpha_of[q] = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, a)));
  }

  // ---- tile table: lane i holds (problem, tile row, tile column) of this workgroup's i-th tile, packed into one register:
  // tm in bits 0-13, tn in bits 14-27, problem in bits 28-29 (host: my_tiles <= 64, tiles_m, tiles_n < 16384).
  // Pass 1 (uniform loop over my tiles): the tile's id within its problem = R[p][j] + rank of v among the workgroups that have a
  // j-th tile of p (a 256-entry count by ballots); pass 2 (one vector evaluation): id -> (tm, tn) in the grouped tile order.
  int tab;
  {
    int my_id = 0, my_p = 0;
    int ti = 0;
#pragma unroll
    for (int q = 0; q < kMaxGroup; ++q) {
      if (q < ga.n) {
        // lane l looks at the counts of virtual workgroups 4 l .. 4 l + 3
        const unsigned c4 = reinterpret_cast<const unsigned*>(ga.cnt[q])[lane];
        for (int j = 0; j < my_cnt[q]; ++j, ++ti) {
          int rank = 0;
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            const bool f = (int)((c4 >> (8 * k)) & 255u) > j && (4 * lane + k) < v;
            rank += __builtin_popcountll(__builtin_amdgcn_ballot_w64(f));
          }
          if (lane == ti) {
            my_id = (int)ga.R[q][j] + rank;
            my_p = q;
          }
        }
      }
    }
    int tmn = ga.p[0].tiles_m, tnn = ga.p[0].tiles_n;
#pragma unroll
    for (int q = 1; q < kMaxGroup; ++q) {
      const bool is = my_p == q;
      tmn = is ? ga.p[q].tiles_m : tmn;
      tnn = is ? ga.p[q].tiles_n : tnn;
    }
    int tm, tn;
    tile_of_flat(my_id, max(tmn, 1), max(tnn, 1), tm, tn);
    tab = tm | (tn << 14) | (my_p << 28);
  }
  auto tile_of = [&](int ti, int& p, int& ra, int& rb) {
    const int t = __builtin_amdgcn_readlane(tab, ti);
    p = (t >> 28) & 3;
    ra = (t & 0x3FFF) * TBM;
    rb = ((t >> 14) & 0x3FFF) * TBN;
  };

  // ---- staging addresses.  A wave feeds 8-row x 128-byte pieces of each half-tile; lane (lr = lane >> 3, lc = lane & 7) reads
  // the swizzled 16-byte chunk lc ^ swz(lr) of a tile row; the wave's second piece of a half (where there is one) is the 8 rows
  // below (wave w feeds local rows [16 w, 16 w + 16) of a 128-row half, which never straddle a 32- or 64-row block), so the
  // scalar offset carries the 8 * ld.  The byte offsets row * ld + chunk are per cursor (the leading dimensions change with the problem) and are recomputed when a
  // cursor enters a tile -- never inside a K-tile: a dozen VALU per load segment cost the kernel 12 %.
  auto stage_rows = [&](int& a0, int& a1, int& b0, int& b1, int& chunk) {  // evaluated when a cursor enters a tile, from the lane id
    int ln;
    asm volatile("v_mov_b32 %0, %1" : "=v"(ln) : "v"(lane));  // (not hoisted: nothing of this stays live across the K loop)
    const int lr = ln >> 3;
    chunk = ((ln & 7) ^ swz_f(lr)) * 16;
    const int l0 = wave * 16 + lr;
    const int la = wave * nA1 * 8 + lr, lb = wave * nB1 * 8 + lr;
    const int p0 = l0 % RA0, p1 = la % RA1;
    a0 = (l0 / RA0) * (RA0 + RA1) + (PERM ? 4 * (p0 & 15) + (p0 >> 4) : p0);
    b0 = (l0 / RB0) * (RB0 + RB1) + l0 % RB0;
    a1 = (la / RA1) * (RA0 + RA1) + RA0 + (PERM ? MA1 * (p1 & 15) + (p1 >> 4) : p1);
    b1 = (lb / RB1) * (RB0 + RB1) + RB0 + lb % RB1;
  };

  // ---- prefetch cursors: the (tile, K-tile) of step s + 1 and s + 2 with everything needed to stage from them
  auto load_tile = [&](Cursor& c, int ti) {
    int p, ra, rb;
    tile_of(ti, p, ra, rb);
    const GroupProblem& P = ga.p[p];
    c.ti = ti;
    c.kt = 0;
    c.nk = P.nk;
    c.lda = P.lda;
    c.ldb = P.ldb;
    c.oa = ra * P.lda;
    c.ob = rb * P.ldb;
    c.rsA = __builtin_amdgcn_make_buffer_rsrc((void*)P.A, 0, P.a_bytes, 0x00020000);
    c.rsB = __builtin_amdgcn_make_buffer_rsrc((void*)P.B, 0, P.b_bytes, 0x00020000);
    if (MX) {  // block-major scales [K/32, rows]: rows = the problem's M (A side) or N (B side)
      const bool s_is_b = wave >= 4;
      c.ss = s_is_b ? P.tiles_n * TBN : P.tiles_m * TBM;
      c.so = (s_is_b ? rb : ra) + (wave & 3) * c.ss;
      c.rsS = __builtin_amdgcn_make_buffer_rsrc((void*)(s_is_b ? P.SB : P.SA), 0, P.nk * 4 * c.ss, 0x00020000);
    }
    int a0, a1, b0, b1, ch;
    stage_rows(a0, a1, b0, b1, ch);
    c.va0 = a0 * P.lda + ch;
    c.va1 = a1 * P.lda + ch;
    c.vb0 = b0 * P.ldb + ch;
    c.vb1 = b1 * P.ldb + ch;
  };
  auto advance = [&](Cursor& c) {  // next step; past the last one the cursor stays on the final K-tile (dead re-fetch)
    if (c.kt + 1 < c.nk) {
      ++c.kt;
    } else if (c.ti + 1 < my_tiles) {
      load_tile(c, c.ti + 1);
    }
  };
  enum { kA0 = 0, kA1 = 1, kB0 = 2, kB1 = 3 };
  auto stage_a = [&](const Cursor& c, int kind, int n, uint8_t* lds_half) {
    const int soff = c.oa + c.kt * BK, voff = kind == kA0 ? c.va0 : c.va1;
#pragma unroll
    for (int i = 0; i < 2; ++i)
      if (i < n)
        __builtin_amdgcn_raw_ptr_buffer_load_lds(c.rsA, LDS_PTR(lds_half + (wave * n + i) * 1024), 16, voff, soff + i * (PERM ? 32 : 8) * c.lda, 0, 0);
  };
  // MX: the 256 scale bytes of (this wave's operand and k-block, the cursor's K-tile, the tile's rows) into scale slot `slot`: ONE
  // LDS-DMA op per wave and K-tile, 16 lanes x 16 B.  (As 64 lanes x 4 B the 256 x 256 variant spilled a VGPR.)  A 192-row tile
  // reads 256 bytes all the same: what lies behind its rows is never used, and past the array the descriptor returns 0.
  auto stage_scales = [&](const Cursor& c, int slot) {
    if (MX && lane < 16)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(c.rsS, LDS_PTR(slds + slot * kSSlot + (wave >> 2) * kSOp + (wave & 3) * kSK), 16, lane * 16,
                                               c.kt * 4 * c.ss + c.so, 0, 0);
  };
  auto stage_b = [&](const Cursor& c, int kind, int n, uint8_t* lds_half) {
    const int soff = c.ob + c.kt * BK, voff = kind == kB0 ? c.vb0 : c.vb1;
#pragma unroll
    for (int i = 0; i < 2; ++i)
      if (i < n)
        __builtin_amdgcn_raw_ptr_buffer_load_lds(c.rsB, LDS_PTR(lds_half + (wave * n + i) * 1024), 16, voff, soff + i * 8 * c.ldb, 0, 0);
  };

  Cursor c1, c2;
  load_tile(c1, 0);
  Cursor c0 = c1;  // step 0
  advance(c1);
  c2 = c1;
  advance(c2);

  v4f acc[2][4][2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[a][i][b][j] = (v4f){0.f, 0.f, 0.f, 0.f};

  uint8_t* const buf0 = lds;
  uint8_t* const buf1 = lds + kBufBytes;
  // prologue: step 0 complete, (step 1: A0, B0) in flight
  stage_scales(c0, 0);
  stage_a(c0, kA0, 2, buf0 + kOffA0);
  stage_b(c0, kB0, 2, buf0 + kOffB0);
  stage_b(c0, kB1, nB1, buf0 + kOffB1);
  stage_a(c0, kA1, nA1, buf0 + kOffA1);
  stage_a(c1, kA0, 2, buf1 + kOffA0);
  stage_b(c1, kB0, 2, buf1 + kOffB0);
  asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_sched_barrier(0);
  if (wr == 1) __builtin_amdgcn_s_barrier();

  // ---- epilogue of the PREVIOUS tile (its problem's output, leading dimension and alpha), distributed over the four phases of
  // the next tile's first K-tile exactly as in mi_gemm.hip (epi_part): whole 128-byte lines where NB1 == 2
  auto epi_of = [&](int ti) -> Epi {
    int p, ra, rb;
    tile_of(ti, p, ra, rb);
    const GroupProblem& P = ga.p[p];
    Epi e;
    e.rsD = __builtin_amdgcn_make_buffer_rsrc((void*)P.D, 0, P.d_bytes, 0x00020000);
    e.ldd = P.ldd;
    e.d_off = (ra * P.ldd + rb) * 2;
    e.alpha = p == 0 ? alpha_of[0] : p == 1 ? alpha_of[1] : p == 2 ? alpha_of[2] : alpha_of[3];
    return e;
  };
  v4i held[2];
  auto epi_part = [&](auto a_c, auto part_c, const Epi& e, bool zero) __attribute__((always_inline)) {
    constexpr int a = decltype(a_c)::value, PART = decltype(part_c)::value;
    constexpr int F = a == 0 ? 4 : MA1, H = F / 2;
    constexpr int bf = a == 0 ? 0 : 1;
    int ln;
    asm volatile("v_mov_b32 %0, %1" : "=v"(ln) : "v"(lane));  // lane-derived store offsets: recomputed here, not kept live
    const int fr = ln & 15, fq = ln >> 4;
    const int ecol = (fq & 1) * 16 + (fq >> 1) * 8;
    auto zero_blk = [&](int i, int b) __attribute__((always_inline)) {
      if (zero) {
#pragma unroll
        for (int j = 0; j < (b == 0 ? 2 : NB1); ++j) acc[a][i][b][j] = (v4f){0.f, 0.f, 0.f, 0.f};
      }
    };
    auto pack_blk = [&](int i, int b) __attribute__((always_inline)) -> v4i {
      if (b == 1 && NB1 == 1) {
        const v4f v0 = acc[a][i][1][0] * e.alpha;
        return (v4i){(int)pack_bf16x2(v0[0], v0[1]), (int)pack_bf16x2(v0[2], v0[3]), 0, 0};
      }
      const v4f v0 = acc[a][i][b][0] * e.alpha, v1 = acc[a][i][b][1] * e.alpha;
      u32 p0x = pack_bf16x2(v0[0], v0[1]), p0y = pack_bf16x2(v0[2], v0[3]);
      u32 p1x = pack_bf16x2(v1[0], v1[1]), p1y = pack_bf16x2(v1[2], v1[3]);
      auto sx = __builtin_amdgcn_permlane16_swap(p0x, p1x, false, false);
      auto sy = __builtin_amdgcn_permlane16_swap(p0y, p1y, false, false);
      return (v4i){(int)sx[0], (int)sy[0], (int)sx[1], (int)sy[1]};
    };
    auto store_row = [&](int i, const v4i& o0, const v4i& o1) __attribute__((always_inline)) {
      constexpr int kRs = PERM ? F : 1;  // PERM: lane row slot s of fragment i holds row F * s + i of the half
      const int rowoff = e.d_off + ((a * RA0 + (PERM ? i : i * 16)) * e.ldd) * 2;
      if (NB1 == 2) {
        const bool lo = fr < 8;
        v4i x, y;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int t = lo ? o1[k] : o0[k];
          const int r = __builtin_amdgcn_update_dpp(0, t, 0x128, 0xF, 0xF, false);  // row_ror:8 = lane m ^ 8
          x[k] = lo ? o0[k] : r;
          y[k] = lo ? r : o1[k];
        }
        const int dvo = ((wr * (RA0 + RA1) + kRs * (fr & 7)) * e.ldd + wc * (RB0 + RB1) + (fr >> 3) * RB0 + ecol) * 2;
        __builtin_amdgcn_raw_buffer_store_b128((mi::v4u)x, e.rsD, dvo, rowoff, 16);
        asm volatile("s_nop 1" ::"v"(x) : "memory");
        __builtin_amdgcn_raw_buffer_store_b128((mi::v4u)y, e.rsD, dvo, rowoff + 8 * kRs * e.ldd * 2, 16);
        asm volatile("s_nop 1" ::"v"(y) : "memory");
      } else {
        const int dvo = ((wr * (RA0 + RA1) + kRs * fr) * e.ldd + wc * (RB0 + RB1)) * 2;
        __builtin_amdgcn_raw_buffer_store_b128((mi::v4u)o0, e.rsD, dvo + ecol * 2, rowoff, 16);
        asm volatile("s_nop 1" ::"v"(o0) : "memory");
        typedef unsigned int v2u __attribute__((ext_vector_type(2)));
        const v2u o2 = {(unsigned)o1[0], (unsigned)o1[1]};
        __builtin_amdgcn_raw_buffer_store_b64(o2, e.rsD, dvo + fq * 8, rowoff + RB0 * 2, 16);
        asm volatile("s_nop 1" ::"v"(o1) : "memory");
      }
    };
#pragma unroll
    for (int i = 0; i < F; ++i) {
      const bool first_rows = i < H;
      if (PART == 2 || (PART == 0 && first_rows)) {
        const v4i o0 = pack_blk(i, 0), o1 = pack_blk(i, 1);
        store_row(i, o0, o1);
        zero_blk(i, 0);
        zero_blk(i, 1);
      } else if (PART == 0) {
        held[i - H] = pack_blk(i, bf);
        zero_blk(i, bf);
      } else if (!first_rows) {
        const v4i oo = pack_blk(i, 1 - bf);
        if (bf == 0) store_row(i, held[i - H], oo);
        else store_row(i, oo, held[i - H]);
        zero_blk(i, 1 - bf);
      }
    }
  };
  using c0_t = std::integral_constant<int, 0>;
  using c1_t = std::integral_constant<int, 1>;
  using c2_t = std::integral_constant<int, 2>;

  // ---- one K-tile = 4 phases (mi_gemm.hip: ktile).  Waits: see the table there; stores per phase 4 | 4 | MA1 | MA1.
#define MI_WAIT_SYNC(MODE_, flag, PH)                                                                              \
  {                                                                                                                \
    constexpr int kAllow = (PH) == 0 ? W + EX - nA1 : (PH) == 1 ? W + EX : (PH) == 2 ? W + EX - 2 : W - nB1;       \
    constexpr int kX = (MODE_) == 0 ? 0                                                                            \
                     : (MODE_) == 1 ? ((PH) == 0 ? 4 : (PH) == 1 ? 8 : (PH) == 2 ? 8 + MA1 : 8 + 2 * MA1)          \
                                    : ((PH) <= 1 ? 4 + 2 * MA1 : (PH) == 2 ? MA1 : 0);                             \
    if ((flag) && kX != 0) wait_vmcnt<kAllow + kX>();                                                              \
    else wait_vmcnt<kAllow>();                                                                                     \
  }                                                                                                                \
  __builtin_amdgcn_s_barrier();                                                                                    \
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                                                               \
  __builtin_amdgcn_sched_barrier(0);                                                                               \
  __builtin_amdgcn_s_setprio(1);
#define MI_PIN(NI, NJ, EXPR)                                           \
  _Pragma("unroll") for (int i = 0; i < NI; ++i)                       \
  _Pragma("unroll") for (int j = 0; j < NJ; ++j) asm volatile("" : "+v"(EXPR));

  v8i af[4], b0f[2], b1f[2];
  // MX: block scales of the current K-tile -- A side: the lane's 4 (half 0) / MA1 (half 1) fragment scales packed in one register
  // (byte i = fragment i, selected by the MFMA's op_sel); B side: one byte per fragment
  int as0 = kUnitScale, as1 = kUnitScale, b0s[2] = {kUnitScale, kUnitScale}, b1s[2] = {kUnitScale, kUnitScale};
  // Per-lane LDS byte addresses of this lane's scales in slot 0 (k-block = lane >> 4, row slot = lane & 15); slot 1, the second
  // half and the B fragments are immediate offsets away.  Half 1 of a 192-row tile holds 2 bytes per row slot, not 4.  Recomputed
  // at the top of every K-tile from the lane id (a handful of VALU), not kept: the 256 x 256 variant has no VGPR to spare for them.
  auto scale_addrs = [&](int& sc_a, int& sc_a1, int& sc_b) __attribute__((always_inline)) {
    int ln;
    asm volatile("v_mov_b32 %0, %1" : "=v"(ln) : "v"(lane));
    const int sfr = ln & 15;
    const int s0 = (int)(size_t)LDS_PTR(slds) + (ln >> 4) * kSK;
    sc_a = s0 + wr * (RA0 + RA1) + 4 * sfr;
    sc_a1 = s0 + wr * (RA0 + RA1) + (MA1 == 4 ? 4 : 2) * sfr;
    sc_b = s0 + kSOp + wc * (RB0 + RB1) + sfr;
  };
  auto mma = [&](auto i_c, const v8i& a_, const v8i& b_, v4f& c_, int sa_, int sb_) __attribute__((always_inline)) {
    constexpr int I = decltype(i_c)::value;
    if (MX) c_ = mfma_ba_sel<FA, FB, I>(a_, b_, c_, sa_, sb_);
    else c_ = mfma_ba<FA, FB>(a_, b_, c_, kUnitScale, kUnitScale);
  };
  auto mma_i = [&](int i, const v8i& a_, const v8i& b_, v4f& c_, int sa_, int sb_) __attribute__((always_inline)) {
    switch (i) {
      case 0: mma(c0_t{}, a_, b_, c_, sa_, sb_); break;
      case 1: mma(c1_t{}, a_, b_, c_, sa_, sb_); break;
      case 2: mma(c2_t{}, a_, b_, c_, sa_, sb_); break;
      default: mma(std::integral_constant<int, 3>{}, a_, b_, c_, sa_, sb_); break;
    }
  };
  auto ktile = [&](auto mode_c, auto slot_c, uint8_t* cur, uint8_t* oth, bool flag, const Epi& pe) {
    constexpr int MODE = decltype(mode_c)::value;
    constexpr int SLOT = decltype(slot_c)::value;  // scale slot of this step = its LDS buffer
    // MX has no unit-scale zero-C form: its quadrants are zeroed by v_mov as the epilogue converts them (epi_part, zero = MX)
    constexpr bool ZC = MODE == 1 && !MX;
    // ---- phase 0: C[0][*][0][*]
    if (MODE == 1) {
      stage_scales(c1, SLOT ^ 1);
      stage_b(c1, kB1, nB1, oth + kOffB1);
      if (flag) epi_part(c0_t{}, c0_t{}, pe, MX);
      __builtin_amdgcn_sched_barrier(0);
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) b0f[j] = read_frag(cur + kOffB0, wc * 2 + j, lane);
#pragma unroll
    for (int i = 0; i < 4; ++i) af[i] = read_frag(cur + kOffA0, wr * 4 + i, lane);
    if (MX) {  // every scale of this K-tile up front (inline asm: consumed behind MI_WAIT_SYNC's lgkmcnt(0), like the fragments)
      int sc_a, sc_a1, sc_b;
      scale_addrs(sc_a, sc_a1, sc_b);
#pragma unroll
      for (int j = 0; j < 2; ++j) asm volatile("ds_read_u8 %0, %1 offset:%2" : "=v"(b0s[j]) : "v"(sc_b), "n"(SLOT * kSSlot + j * 16));
#pragma unroll
      for (int j = 0; j < NB1; ++j) asm volatile("ds_read_u8 %0, %1 offset:%2" : "=v"(b1s[j]) : "v"(sc_b), "n"(SLOT * kSSlot + RB0 + j * 16));
      asm volatile("ds_read_b32 %0, %1 offset:%2" : "=v"(as0) : "v"(sc_a), "n"(SLOT * kSSlot));
      if (MA1 == 4) asm volatile("ds_read_b32 %0, %1 offset:%2" : "=v"(as1) : "v"(sc_a1), "n"(SLOT * kSSlot + RA0));
      else asm volatile("ds_read_u16 %0, %1 offset:%2" : "=v"(as1) : "v"(sc_a1), "n"(SLOT * kSSlot + RA0));
    }
    if (MODE != 1) {
      stage_scales(c1, SLOT ^ 1);
      stage_b(c1, kB1, nB1, oth + kOffB1);
    }
    MI_WAIT_SYNC(MODE, flag, 0)
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        if (ZC) mfma_ba_zero<FA, FB>(af[i], b0f[j], acc[0][i][0][j], kUnitScale);
        else mma_i(i, af[i], b0f[j], acc[0][i][0][j], as0, b0s[j]);
      }
    MI_PIN(4, 2, acc[0][i][0][j])
    MI_PHASE_END();
    // ---- phase 1: C[0][*][1][*]
    if (MODE == 1) {
      stage_a(c1, kA1, nA1, oth + kOffA1);
      if (flag) epi_part(c0_t{}, c1_t{}, pe, MX);
      __builtin_amdgcn_sched_barrier(0);
    }
#pragma unroll
    for (int j = 0; j < NB1; ++j) b1f[j] = read_frag(cur + kOffB1, wc * NB1 + j, lane);
    if (MODE != 1) stage_a(c1, kA1, nA1, oth + kOffA1);
    MI_WAIT_SYNC(MODE, flag, 1)
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < NB1; ++j) {
        if (ZC) mfma_ba_zero<FA, FB>(af[i], b1f[j], acc[0][i][1][j], kUnitScale);
        else mma_i(i, af[i], b1f[j], acc[0][i][1][j], as0, b1s[j]);
      }
    MI_PIN(4, NB1, acc[0][i][1][j])
    MI_PHASE_END();
    // ---- phase 2: C[1][*][1][*]
    if (MODE == 1) {
      stage_a(c2, kA0, 2, cur + kOffA0);
      if (flag) epi_part(c1_t{}, c0_t{}, pe, MX);
      __builtin_amdgcn_sched_barrier(0);
    }
#pragma unroll
    for (int i = 0; i < MA1; ++i) af[i] = read_frag(cur + kOffA1, wr * MA1 + i, lane);
    if (MODE != 1) stage_a(c2, kA0, 2, cur + kOffA0);
    MI_WAIT_SYNC(MODE, flag, 2)
#pragma unroll
    for (int i = 0; i < MA1; ++i)
#pragma unroll
      for (int j = 0; j < NB1; ++j) {
        if (ZC) mfma_ba_zero<FA, FB>(af[i], b1f[j], acc[1][i][1][j], kUnitScale);
        else mma_i(i, af[i], b1f[j], acc[1][i][1][j], as1, b1s[j]);
      }
    MI_PIN(MA1, NB1, acc[1][i][1][j])
    MI_PHASE_END();
    // ---- phase 3: C[1][*][0][*]
    stage_b(c2, kB0, 2, cur + kOffB0);
    if (MODE == 1) {
      if (flag) epi_part(c1_t{}, c1_t{}, pe, MX);
      __builtin_amdgcn_sched_barrier(0);
    }
    MI_WAIT_SYNC(MODE, flag, 3)
#pragma unroll
    for (int i = 0; i < MA1; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        if (ZC) mfma_ba_zero<FA, FB>(af[i], b0f[j], acc[1][i][0][j], kUnitScale);
        else mma_i(i, af[i], b0f[j], acc[1][i][0][j], as1, b0s[j]);
      }
    MI_PIN(MA1, 2, acc[1][i][0][j])
    MI_PHASE_END();
    advance(c1);
    advance(c2);
  };

  Epi prev = epi_of(0);
  for (int ti = 0; ti < my_tiles; ++ti) {
    const bool have_prev = ti > 0;
    const int nk = ga.p[(__builtin_amdgcn_readlane(tab, ti) >> 28) & 3].nk;
    ktile(c1_t{}, c0_t{}, buf0, buf1, have_prev, prev);
    ktile(c2_t{}, c1_t{}, buf1, buf0, have_prev, prev);
    for (int pair = 1; pair < nk / 2; ++pair) {
      ktile(c0_t{}, c0_t{}, buf0, buf1, false, prev);
      ktile(c0_t{}, c1_t{}, buf1, buf0, false, prev);
    }
    prev = epi_of(ti);
  }
  if (wr == 0) __builtin_amdgcn_s_barrier();
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  if (my_tiles > 0) {
    epi_part(c0_t{}, c2_t{}, prev, false);
    epi_part(c1_t{}, c2_t{}, prev, false);
  }
#undef MI_WAIT_SYNC
#undef MI_PIN
}

// ---- host: longest-processing-time schedule of the group's tiles over the persistent workgroups, cached per shape
struct Sched {
  uint8_t cnt[kMaxGroup][kMaxWg];
  uint16_t R[kMaxGroup][kMaxPerWg];
  int max_per_wg;
  bool ok;
};

static Sched make_sched(int G, int n, const int* ntiles, const int* nk) {
  Sched sc;
  std::memset(&sc, 0, sizeof(sc));
  // problems arrive sorted by decreasing nk.  Greedy: every tile goes to the workgroup with the least work so far (ties: lowest
  // virtual index) -- the classic LPT rule; with tiles of few distinct lengths it is within one short tile of the optimum.
  std::vector<std::pair<long long, int>> heap;  // (load, v), min-heap
  heap.reserve(G);
  for (int v = 0; v < G; ++v) heap.emplace_back(0LL, v);
  auto cmp = [](const std::pair<long long, int>& a, const std::pair<long long, int>& b) { return a > b; };
  std::make_heap(heap.begin(), heap.end(), cmp);
  std::vector<int> per_wg(G, 0);
  sc.ok = true;
  for (int p = 0; p < n; ++p) {
    for (int t = 0; t < ntiles[p]; ++t) {
      std::pop_heap(heap.begin(), heap.end(), cmp);
      auto& top = heap.back();
      const int v = top.second;
      if (sc.cnt[p][v] == 255 || per_wg[v] == kMaxPerWg) sc.ok = false;
      else {
        ++sc.cnt[p][v];
        ++per_wg[v];
      }
      top.first += nk[p];
      std::push_heap(heap.begin(), heap.end(), cmp);
    }
    int run = 0;
    for (int j = 0; j < kMaxPerWg; ++j) {
      sc.R[p][j] = (uint16_t)run;
      int have = 0;
      for (int v = 0; v < G; ++v) have += sc.cnt[p][v] > j ? 1 : 0;
      run += have;
    }
    if (run != ntiles[p] || ntiles[p] > 65535) sc.ok = false;
  }
  sc.max_per_wg = 0;
  for (int v = 0; v < G; ++v) sc.max_per_wg = per_wg[v] > sc.max_per_wg ? per_wg[v] : sc.max_per_wg;
  return sc;
}

static const Sched& cached_sched(int G, int n, const int* ntiles, const int* nk) {
  static std::mutex mu;
  static std::map<std::vector<int>, Sched> cache;
  std::vector<int> key{G, n};
  for (int p = 0; p < n; ++p) {
    key.push_back(ntiles[p]);
    key.push_back(nk[p]);
  }
  std::lock_guard<std::mutex> lock(mu);
  auto it = cache.find(key);
  if (it == cache.end()) {
    if (cache.size() > 256) cache.clear();
    it = cache.emplace(key, make_sched(G, n, ntiles, nk)).first;
  }
  return it->second;
}

template <int FA, int FB, bool MX>
static int launch_grouped(const GroupArgs& ga, int cfg, int grid, hipStream_t st) {
  switch (cfg) {
    case 0: hipLaunchKernelGGL((gemm_256_grp<FA, FB, 4, 2, MX>), dim3(grid), dim3(512), 0, st, ga); break;
    case 1: hipLaunchKernelGGL((gemm_256_grp<FA, FB, 4, 1, MX>), dim3(grid), dim3(512), 0, st, ga); break;
    case 2: hipLaunchKernelGGL((gemm_256_grp<FA, FB, 2, 2, MX>), dim3(grid), dim3(512), 0, st, ga); break;
    default: hipLaunchKernelGGL((gemm_256_grp<FA, FB, 2, 1, MX>), dim3(grid), dim3(512), 0, st, ga); break;
  }
  MI_CHECK_LAUNCH(MX ? "mi_gemm_mxfp8_grouped launch" : "mi_gemm_fp8_grouped launch");
  return MI_OK;
}

template <bool MX>
static int launch_grouped_fmt(const GroupArgs& ga, int fmt_a, int fmt_b, int cfg, int grid, hipStream_t st) {
  return with_pair(fmt_a, fmt_b, [&](auto a, auto b) { return launch_grouped<a(), b(), MX>(ga, cfg, grid, st); });
}

// One problem of a group as the host path below takes it.  Each entry point fills it from its own ABI struct and runs its own
// argument checks on it (the two contracts differ in order, wording and return codes); everything after the checks is shared.
struct GroupIn {
  const void *A, *B, *sa, *sb;  // sa / sb: the device scalars sa_inv / sb_inv (per-tensor) or the E8M0 block scales SA / SB (MX)
  void* D;
  int64_t M, N, K, lda, ldb, ldd;
  int index;  // position in the caller's array (messages name it)
};

// tile shape that minimises K-tile steps x tile area / efficiency over the WHOLE group, among those that divide every problem
// (-1: none).  A persistent walk over a shared tile list has no per-problem round quantisation, only the tail of the whole list.
// Divisibility is all it asks: M, N <= 0 "divide", and the per-problem checks of the entry points refuse such a problem afterwards.
static int pick_group_cfg(const GroupIn* in, int n, int ncu) {
  static const double eff[4] = {1.0, 0.90, 0.90, 0.80};
  int cfg = -1;
  double best = 0;
  for (int c = 0; c < 4; ++c) {
    bool ok = true;
    double steps = 0;
    for (int i = 0; i < n; ++i) {
      if (in[i].M % kTileBm[c] || in[i].N % kTileBn[c]) ok = false;
      else steps += (double)(in[i].M / kTileBm[c]) * (in[i].N / kTileBn[c]) * (in[i].K / 128);
    }
    if (!ok) continue;
    const double cost = steps / ncu * kTileBm[c] * kTileBn[c] / eff[c];
    if (cfg < 0 || cost < best * 0.97) {
      cfg = c;
      best = cost;
    }
  }
  return cfg;
}

// longest tiles first: a round-robin deal of that order over the persistent workgroups is a longest-processing-time schedule
static void sort_by_decreasing_k(GroupIn* in, int n) {
  for (int i = 0; i < n; ++i)
    for (int j = i + 1; j < n; ++j)
      if (in[j].K > in[i].K) std::swap(in[i], in[j]);
}

// the size limits that end a problem's checks at both entry points (32-bit buffer offsets, 14-bit tile coordinates)
static bool group_sizes_ok(const char* who, const GroupIn& q, int cfg) {
  if (!(q.M * q.lda < (1LL << 31) && q.N * q.ldb < (1LL << 31) && q.M * q.ldd * 2 < (1LL << 31))) {
    set_error("%s: operands of problem %d exceed 2 GiB (32-bit buffer offsets)", who, q.index);
    return false;
  }
  if (!(q.M / kTileBm[cfg] < 16384 && q.N / kTileBn[cfg] < 16384)) {
    set_error("%s: problem %d has too many tiles per dimension", who, q.index);
    return false;
  }
  return true;
}

// What both entry points do once `in` (sorted by decreasing K) has passed their checks: tile lists, schedule, launch.
// four_wave: 256 x 256 tiles (cfg 0) on the four-wave kernel (mi_gemm_w4.hip): same schedule, other kernel; per-tensor only.
static int launch_group(const char* who, const GroupIn* in, int n, int cfg, int fmt_a, int fmt_b, bool mx, bool four_wave, void* stream) {
  GroupArgs ga;
  std::memset(&ga, 0, sizeof(ga));
  int total = 0, ntiles[kMaxGroup], nks[kMaxGroup];
  for (int k = 0; k < n; ++k) {
    const GroupIn& q = in[k];
    GroupProblem& P = ga.p[k];
    P.A = (const uint8_t*)q.A;
    P.B = (const uint8_t*)q.B;
    P.D = (uint16_t*)q.D;
    if (mx) {
      P.SA = (const uint8_t*)q.sa;
      P.SB = (const uint8_t*)q.sb;
    } else {
      P.sa_inv = (const float*)q.sa;
      P.sb_inv = (const float*)q.sb;
    }
    P.lda = (int)q.lda;
    P.ldb = (int)q.ldb;
    P.ldd = (int)q.ldd;
    P.nk = (int)(q.K / 128);
    P.tiles_m = (int)(q.M / kTileBm[cfg]);
    P.tiles_n = (int)(q.N / kTileBn[cfg]);
    P.ntiles = P.tiles_m * P.tiles_n;
    P.tile_base = total;
    P.a_bytes = (int)(q.M * q.lda);
    P.b_bytes = (int)(q.N * q.ldb);
    P.d_bytes = (int)(q.M * q.ldd * 2);
    ntiles[k] = P.ntiles;
    nks[k] = P.nk;
    total += P.ntiles;
  }
  ga.n = n;
  ga.total_tiles = total;
  const int ncu = num_cus();
  const int grid = total < ncu ? total : (ncu > kMaxWg ? kMaxWg : ncu);
  const Sched& sc = cached_sched(grid, n, ntiles, nks);
  if (!(sc.ok && sc.max_per_wg <= kMaxPerWg)) {
    set_error("%s: more than %d tiles per workgroup (%d tiles in all)", who, kMaxPerWg, total);
    return mx ? MI_ERR_SHAPE : MI_ERR_ARG;  // each entry point answers a shape it cannot take with the code it always has
  }
  std::memcpy(ga.cnt, sc.cnt, sizeof(ga.cnt));
  std::memcpy(ga.R, sc.R, sizeof(ga.R));
  hipStream_t st = (hipStream_t)stream;
  if (four_wave) return launch_w4_grouped(ga, fmt_a, fmt_b, grid, st);
  return mx ? launch_grouped_fmt<true>(ga, fmt_a, fmt_b, cfg, grid, st) : launch_grouped_fmt<false>(ga, fmt_a, fmt_b, cfg, grid, st);
}

}  // namespace mi

extern "C" int mi_gemm_mxfp8_grouped(const mi_gemm_mx_problem* problems, int n, int fmt_a, int fmt_b, int tile_cfg, void* stream) {
  using namespace mi;
  MI_CHECK_ARG(problems && n >= 1 && n <= kMaxGroup, "mi_gemm_mxfp8_grouped: 1 to %d problems", kMaxGroup);
  MI_CHECK_ARG((fmt_a == 0 || fmt_a == 1) && (fmt_b == 0 || fmt_b == 1), "mi_gemm_mxfp8_grouped: bad fmt");
  MI_CHECK_ARG(tile_cfg != 4, "mi_gemm_mxfp8_grouped: tile_cfg 4 (four-wave kernel) has no block-scaled form");
  MI_CHECK_ARG(tile_cfg >= -1 && tile_cfg < 4, "mi_gemm_mxfp8_grouped: tile_cfg must be -1 or 0-3");
  GroupIn in[kMaxGroup];
  for (int i = 0; i < n; ++i) {
    const mi_gemm_mx_problem& q = problems[i];
    MI_CHECK_ARG(q.A && q.SA && q.B && q.SB && q.D, "mi_gemm_mxfp8_grouped: null pointer in problem %d", i);
    MI_CHECK_ARG(((uintptr_t)q.A % 16) == 0 && ((uintptr_t)q.B % 16) == 0 && ((uintptr_t)q.D % 16) == 0 &&
                     ((uintptr_t)q.SA % 16) == 0 && ((uintptr_t)q.SB % 16) == 0,
                 "mi_gemm_mxfp8_grouped: operands and scales of problem %d must be 16-byte aligned", i);
    if (!(q.M > 0 && q.N > 0 && q.K > 0 && q.K % 256 == 0)) {
      set_error("mi_gemm_mxfp8_grouped: problem %d (%lld x %lld x %lld) needs M, N > 0 and K %% 256 == 0", i, (long long)q.M,
                (long long)q.N, (long long)q.K);
      return MI_ERR_SHAPE;
    }
    in[i] = {q.A, q.B, q.SA, q.SB, q.D, q.M, q.N, q.K, q.K, q.K, q.N, i};  // MX operands are tight
  }
  const int ncu = num_cus();
  const int cfg = tile_cfg < 0 ? pick_group_cfg(in, n, ncu) : tile_cfg;
  if (cfg < 0) {
    for (int i = 0; i < n; ++i)
      if (pick_group_cfg(in + i, 1, ncu) < 0) {
        set_error("mi_gemm_mxfp8_grouped: no tile shape divides problem %d (%lld x %lld)", i, (long long)in[i].M, (long long)in[i].N);
        return MI_ERR_SHAPE;
      }
    set_error("mi_gemm_mxfp8_grouped: no tile shape divides every one of the %d problems", n);
    return MI_ERR_SHAPE;
  }
  sort_by_decreasing_k(in, n);
  for (int k = 0; k < n; ++k) {
    const GroupIn& q = in[k];
    if (q.M % kTileBm[cfg] || q.N % kTileBn[cfg]) {
      set_error("mi_gemm_mxfp8_grouped: problem %d (%lld x %lld x %lld) does not fit tile shape %d x %d", q.index, (long long)q.M,
                (long long)q.N, (long long)q.K, kTileBm[cfg], kTileBn[cfg]);
      return MI_ERR_SHAPE;
    }
    if (!group_sizes_ok("mi_gemm_mxfp8_grouped", q, cfg)) return MI_ERR_SHAPE;
  }
  return launch_group("mi_gemm_mxfp8_grouped", in, n, cfg, fmt_a, fmt_b, true, false, stream);
}

extern "C" int mi_gemm_fp8_grouped(const mi_gemm_problem* problems, int n, int fmt_a, int fmt_b, int tile_cfg, void* stream) {
  using namespace mi;
  MI_CHECK_ARG(problems && n >= 1 && n <= kMaxGroup, "mi_gemm_fp8_grouped: 1 to %d problems", kMaxGroup);
  MI_CHECK_ARG((fmt_a == 0 || fmt_a == 1) && (fmt_b == 0 || fmt_b == 1), "mi_gemm_fp8_grouped: bad fmt");
  GroupIn in[kMaxGroup];
  for (int i = 0; i < n; ++i) {
    const mi_gemm_problem& q = problems[i];
    in[i] = {q.A, q.B, q.sa_inv, q.sb_inv, q.D, q.M, q.N, q.K, q.lda, q.ldb, q.ldd, i};
  }
  // tile shape: the caller's, or (any negative tile_cfg) the one pick_group_cfg finds for the whole group
  // tile_cfg 4 = 256 x 256 tiles on the four-wave kernel (mi_gemm_w4.hip; every problem K >= 512): same schedule, other kernel
  const bool four_wave = tile_cfg == 4;
  const int cfg = four_wave ? 0 : tile_cfg < 0 ? pick_group_cfg(in, n, num_cus()) : tile_cfg;
  MI_CHECK_ARG(cfg >= 0 && cfg < 4, "mi_gemm_fp8_grouped: no tile shape divides every problem");
  sort_by_decreasing_k(in, n);
  for (int k = 0; k < n; ++k) {
    const GroupIn& q = in[k];
    MI_CHECK_ARG(q.A && q.B && q.D && q.sa && q.sb, "mi_gemm_fp8_grouped: null pointer in problem %d", q.index);
    MI_CHECK_ARG(q.M > 0 && q.N > 0 && q.K > 0 && q.M % kTileBm[cfg] == 0 && q.N % kTileBn[cfg] == 0 && q.K % 256 == 0,
                 "mi_gemm_fp8_grouped: problem %d (%lld x %lld x %lld) does not fit tile shape %d x %d / K %% 256", q.index,
                 (long long)q.M, (long long)q.N, (long long)q.K, kTileBm[cfg], kTileBn[cfg]);
    MI_CHECK_ARG(q.lda >= q.K && q.ldb >= q.K && q.ldd >= q.N && q.lda % 16 == 0 && q.ldb % 16 == 0 && q.ldd % 4 == 0,
                 "mi_gemm_fp8_grouped: bad leading dimensions in problem %d", q.index);
    MI_CHECK_ARG(((uintptr_t)q.A % 16) == 0 && ((uintptr_t)q.B % 16) == 0 && ((uintptr_t)q.D % 16) == 0,
                 "mi_gemm_fp8_grouped: operands must be 16-byte aligned");
    if (!group_sizes_ok("mi_gemm_fp8_grouped", q, cfg)) return MI_ERR_ARG;
  }
  return launch_group("mi_gemm_fp8_grouped", in, n, cfg, fmt_a, fmt_b, false, four_wave, stream);
}
