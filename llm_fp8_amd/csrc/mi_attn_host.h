// Host side of the attention entry points (mi_attn.hip: mi_attn_fwd / mi_attn_bwd and their _win / _seg forms; mi_attn_short.hip:
// mi_attn_short_fwd / mi_attn_short_bwd): the operand checks all eight share.  Everything is refused here, on the host, before
// any launch, under the entry point's name.  What only one entry point asks (window >= 1, the segment pointers, causal) is
// checked by that entry point.
#pragma once
#include <climits>
#include <initializer_list>

#include "mi_common.h"

namespace mi {

enum AttnOperandKind {
  ATT_ROWS,  // bf16 [B, S, heads, D] behind a token stride: 16-byte row accesses, so 16-byte aligned and a stride multiple of 8
  ATT_KV,    // ATT_ROWS that the LDS DMA stages: its 32-bit buffer offsets span one batch, which must stay below 2 GiB
  ATT_F32,   // lse, fp32 [B, H, S]: 4-byte aligned
  ATT_PTR,   // delta, the backward's own workspace: non-null
};

struct AttnOperand {
  const char* name;
  const void* ptr;
  int64_t ts;  // token stride in elements (ATT_ROWS, ATT_KV)
  AttnOperandKind kind;
};

// s_min .. s_max: the sequence lengths the entry point's kernels take; grid_y: what its grid has in y (z is B).
inline int attn_check_operands(const char* fn, std::initializer_list<AttnOperand> operands, int B, int S, int H, int G, int D,
                               int s_min, int s_max, int grid_y) {
  MI_CHECK_ARG(B >= 1 && H >= 1 && G >= 1 && H % G == 0, "%s: bad B/H/G (%d, %d, %d)", fn, B, H, G);
  MI_CHECK_ARG(D == 128 || D == 64, "%s: head_dim %d not supported (64, 128)", fn, D);
  MI_CHECK_ARG(S >= s_min && S % 16 == 0, "%s: seq %d must be a multiple of 16 and at least %d", fn, S, s_min);
  MI_CHECK_ARG(S <= s_max, "%s: seq %d must be at most %d", fn, S, s_max);
  for (const AttnOperand& a : operands) {
    MI_CHECK_ARG(a.ptr, "%s: null pointer (%s)", fn, a.name);
    if (a.kind == ATT_PTR) continue;
    const int align = a.kind == ATT_F32 ? 4 : 16;
    MI_CHECK_ARG((uintptr_t)a.ptr % align == 0, "%s: %s must be %d-byte aligned", fn, a.name, align);
    if (a.kind == ATT_F32) continue;
    MI_CHECK_ARG(a.ts % 8 == 0, "%s: token strides must be multiples of 8 (%s: %lld)", fn, a.name, (long long)a.ts);
    MI_CHECK_ARG(a.kind != ATT_KV || (int64_t)S * a.ts * 2 < (1LL << 31),
                 "%s: one batch of %s must span < 2 GiB (32-bit buffer offsets of the LDS DMA)", fn, a.name);
  }
  MI_CHECK_ARG(grid_y <= 65535 && B <= 65535, "%s: grid too large", fn);
  return MI_OK;
}

}  // namespace mi
