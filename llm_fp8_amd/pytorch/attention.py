"""Attention pieces with the `transformer_engine.pytorch` surface used at te_llama.py:45-56,65-66,77:
`MultiheadAttention(...)`(hidden_states, attention_mask=, rotary_pos_emb=) and
`attention.RotaryPositionEmbedding(dim)(max_seq_len)`.

The two projections (`layernorm_qkv`, `proj`) are on the FP8 hot path; the attention core is bf16 (the
reference's core is bf16 flash-attn through TE, README.md:27-28): the hand-written flash-style HIP kernels of
csrc/mi_attn.hip for the shapes of the reference's configs and collator (causal, head_dim 64 / 128, seq >= 128 and
seq % 16 == 0 -- the reference pads a batch to a multiple of 16 -- no dropout), the one-workgroup-per-(batch, kv head)
kernels of csrc/mi_attn_short.hip for the same shapes at the lengths below 128 where they were measured faster (`_SHORT_MIN_S`;
`LLM_FP8_AMD_NO_SHORT_ATTN=1` turns that route off), torch `scaled_dot_product_attention` otherwise.

Sliding-window causal attention (`window_size=(left, 0)`, TE's and flash-attn's argument; W = left + 1 keys per query, HF's
`sliding_window`) runs on the band-limited instantiations of the same kernels (mi_attn_fwd_win / mi_attn_bwd_win: O(S * W) work)
under the conditions of the full-causal route; every other windowed case -- S < 128 with a real band, CPU tensors, dropout,
`LLM_FP8_AMD_NO_WINDOW_ATTN=1` -- takes `scaled_dot_product_attention` with a cached boolean band mask.

Packed sequences (`cu_seqlens_q`, TE's argument; HF's `cu_seq_lens_q`): one row of tokens holds several documents and a token
attends only inside its own.  The same kernels walk only the documents (mi_attn_fwd_seg / mi_attn_bwd_seg: O(sum len^2) work) under
the conditions of the full-causal route; every other packed case -- T < 128, CPU tensors, dropout, a window as well,
`LLM_FP8_AMD_NO_PACKED_ATTN=1` -- takes `scaled_dot_product_attention` with the boolean document mask.  RoPE needs nothing: its
scores depend on i - j only, so positions that run through the row give every document the scores of restarted ones.

`DotProductAttention.forward` is the one place that decides: it brings q, k, v to bshd, reduces the request to (band W or None,
documents or None, dropout), takes the kernels where `_flash_ok` / `_short_ok` admit the call, else one SDPA call whose mask
`_sdpa_mask` builds from the band and / or the documents, and restores the caller's layout."""
from __future__ import annotations

import os
import weakref
from typing import Optional, Tuple

import torch
import torch.nn.functional as F

from . import ops
from .module import DyHandoff, LayerNormLinear, Linear, RMSNorm, handoff_readers

__all__ = ["RotaryPositionEmbedding", "apply_rotary_pos_emb", "DotProductAttention", "MultiheadAttention"]


class RotaryPositionEmbedding(torch.nn.Module):
    """TE-style RoPE table: forward(max_seq_len) -> [s, 1, 1, dim] float32 of angles (base 10000 by
    default, as the reference constructs it at te_llama.py:65)."""

    def __init__(self, dim: int, rotary_percent: float = 1.0, seq_len_interpolation_factor=None,
                 pretrained_max_position_embeddings=None, rotary_base: float = 10000.0):
        super().__init__()
        if rotary_percent < 1.0:
            dim = int(dim * rotary_percent)
        self.dim = dim
        self.seq_len_interpolation_factor = seq_len_interpolation_factor
        inv_freq = 1.0 / (rotary_base ** (torch.arange(0, dim, 2, dtype=torch.float32) / dim))
        self.register_buffer("inv_freq", inv_freq, persistent=False)

    def forward(self, max_seq_len: int, offset: int = 0) -> torch.Tensor:
        seq = torch.arange(max_seq_len, device=self.inv_freq.device, dtype=torch.float32) + offset
        if self.seq_len_interpolation_factor is not None:
            seq = seq / self.seq_len_interpolation_factor
        freqs = torch.outer(seq, self.inv_freq)
        emb = torch.cat((freqs, freqs), dim=-1)
        return emb.reshape(emb.size(0), 1, 1, emb.size(1))


def _rotate_half(x: torch.Tensor) -> torch.Tensor:
    x1, x2 = x.chunk(2, dim=-1)
    return torch.cat((-x2, x1), dim=-1)


def apply_rotary_pos_emb(t: torch.Tensor, freqs: torch.Tensor, tensor_format: str = "sbhd") -> torch.Tensor:
    """t: [s,b,h,d] ("sbhd") or [b,s,h,d] ("bshd"); freqs: [s_max,1,1,d_rot] angles."""
    s = t.shape[0] if tensor_format == "sbhd" else t.shape[1]
    f = freqs[:s]
    if tensor_format == "bshd":
        f = f.transpose(0, 1)  # [1, s, 1, d]
    cos, sin = torch.cos(f).to(t.dtype), torch.sin(f).to(t.dtype)
    rot = f.shape[-1]
    tr, tp = t[..., :rot], t[..., rot:]
    out = tr * cos + _rotate_half(tr) * sin
    return out if tp.shape[-1] == 0 else torch.cat((out, tp), dim=-1)


_COS_SIN_CACHE = {}


def _cos_sin_tables(freqs: torch.Tensor, seq: int):
    """fp32 cos/sin [seq, D/2] of a TE angle table [s_max,1,1,D] (= cat(f, f)); cached per table and length."""
    key = (freqs.data_ptr(), freqs.shape, seq, str(freqs.device))
    hit = _COS_SIN_CACHE.get(key)
    if hit is None:
        half = freqs.shape[-1] // 2
        f = freqs[:seq, 0, 0, :half].float()
        hit = (torch.cos(f).contiguous(), torch.sin(f).contiguous())
        if len(_COS_SIN_CACHE) > 16:
            _COS_SIN_CACHE.clear()
        _COS_SIN_CACHE[key] = hit
    return hit


class _RoPESplitFn(torch.autograd.Function):
    """qkv [B,S,W] -> q [B,S,h,d], k, v [B,S,g,d] with RoPE on q, k: one HIP launch each way (mi_rope_qkv).
    `handoff` (module.DyHandoff, optional): the q|k|v projection that produced `qkv` has announced how its backward quantises
    grad_output; backward then emits that FP8 gradient directly (mi_rope_qkv_bwd_cast) and returns an unwritten placeholder."""

    @staticmethod
    def forward(ctx, qkv, cos, sin, n_q, n_kv, d, handoff=None):
        B, S, W = qkv.shape
        x = qkv.reshape(B * S, W)
        x = x if x.is_contiguous() else x.contiguous()
        q, k, v = ops.rope_qkv_forward(x, cos, sin, n_q, n_kv, d, S)
        ctx.save_for_backward(cos, sin)
        ctx.meta = (B, S, n_q, n_kv, d)
        ctx.handoff = handoff
        ctx.act_ref = weakref.ref(qkv) if handoff is not None else None  # to see hooks / retain_grad put on it before backward
        return q.view(B, S, n_q, d), k.view(B, S, n_kv, d), v.view(B, S, n_kv, d)

    @staticmethod
    def backward(ctx, dq, dk, dv):
        cos, sin = ctx.saved_tensors
        B, S, n_q, n_kv, d = ctx.meta
        T = B * S
        h = ctx.handoff
        if h is not None and h.offered() and handoff_readers(ctx.act_ref()):
            h = None  # somebody reads d(qkv): produce it for real
        if h is not None and h.offered() and d == 128 and T % (32 if h.mx else 8) == 0:
            args = (dq.reshape(T, n_q * d), dk.reshape(T, n_kv * d), dv.reshape(T, n_kv * d), cos, sin, n_q, n_kv, d, S)
            if h.mx:
                fp8 = ops.mxfp8_rope_bwd_quantize(*args, h.fmt, rowwise=h.want_y, colwise=h.want_t)
            else:
                fp8 = ops.rope_qkv_backward_cast(*args, h.scale, h.amax, h.fmt, want_y=h.want_y, want_t=h.want_t)
            g = torch.empty((B, S, (n_q + 2 * n_kv) * d), dtype=torch.bfloat16, device=dq.device)  # placeholder: never written
            h.put(fp8, g)
            return g, None, None, None, None, None, None
        g = ops.rope_qkv_backward(dq.reshape(T, n_q * d), dk.reshape(T, n_kv * d), dv.reshape(T, n_kv * d), cos, sin,
                                  n_q, n_kv, d, S)
        return g.view(B, S, -1), None, None, None, None, None, None


class _QKNormRoPESplitFn(torch.autograd.Function):
    """_RoPESplitFn with the per-head RMSNorm of q and k (weights gq, gk [d]) in front of the rotation: one HIP launch each way
    (mi_qknorm_rope_qkv / mi_qknorm_rope_qkv_bwd) plus the finish of the gamma partials.  Backward always writes the bf16 d(qkv):
    there is no FP8-emitting form, so the caller withdraws the projection's DyHandoff."""

    @staticmethod
    def forward(ctx, qkv, gq, gk, cos, sin, n_q, n_kv, d, eps):
        B, S, W = qkv.shape
        x = qkv.reshape(B * S, W)
        x = x if x.is_contiguous() else x.contiguous()
        q, k, v, rstd = ops.qknorm_rope_qkv_forward(x, gq, gk, cos, sin, n_q, n_kv, d, S, eps)
        ctx.save_for_backward(x, rstd, gq, gk, cos, sin)
        ctx.meta = (B, S, n_q, n_kv, d)
        return q.view(B, S, n_q, d), k.view(B, S, n_kv, d), v.view(B, S, n_kv, d)

    @staticmethod
    def backward(ctx, dq, dk, dv):
        x, rstd, gq, gk, cos, sin = ctx.saved_tensors
        B, S, n_q, n_kv, d = ctx.meta
        T = B * S
        g, dgq, dgk = ops.qknorm_rope_qkv_backward(dq.reshape(T, n_q * d), dk.reshape(T, n_kv * d), dv.reshape(T, n_kv * d), x, rstd,
                                                   gq, gk, cos, sin, n_q, n_kv, d, S, dgamma_dtype=gq.dtype)
        return g.view(B, S, -1), dgq, dgk, None, None, None, None, None, None


def _rows_ok(t: torch.Tensor, S: int, D: int) -> bool:
    """What the launchers ask of a bshd operand of S tokens per batch: rows of D-wide heads behind one token stride, a multiple of
    8, at a 16-byte aligned address."""
    return (t.stride(3) == 1 and t.stride(2) == D and t.stride(0) == S * t.stride(1) and t.stride(1) % 8 == 0
            and t.data_ptr() % 16 == 0)


def _launcher_dout(do: torch.Tensor) -> torch.Tensor:
    """dO as the backward launchers take it: itself where _rows_ok, else a copy (a misaligned contiguous view's .contiguous() is
    itself, so the copy is a clone)."""
    return do if _rows_ok(do, do.shape[1], do.shape[3]) else do.clone(memory_format=torch.contiguous_format)


class _FlashAttnFn(torch.autograd.Function):
    """bshd attention core on mi_attn_fwd / mi_attn_bwd (`window` = W: mi_attn_fwd_win / mi_attn_bwd_win; `segments` =
    ops.attn_segments' pair: mi_attn_fwd_seg / mi_attn_bwd_seg); saves q, k, v, o and the log-sum-exp, never the scores."""

    @staticmethod
    def forward(ctx, q, k, v, scale, causal, window=None, segments=None):
        o, lse = ops.attn_fwd(q, k, v, scale, causal, window=window, segments=segments)
        ctx.save_for_backward(q, k, v, o, lse)
        ctx.scale, ctx.causal, ctx.window, ctx.segments = scale, causal, window, segments
        return o

    @staticmethod
    def backward(ctx, do):
        q, k, v, o, lse = ctx.saved_tensors
        dq, dk, dv = ops.attn_bwd(_launcher_dout(do), q, k, v, o, lse, ctx.scale, ctx.causal, window=ctx.window, segments=ctx.segments)
        return dq, dk, dv, None, None, None, None


class _ShortAttnFn(torch.autograd.Function):
    """_FlashAttnFn at 16 <= S < 128, on mi_attn_short_fwd / mi_attn_short_bwd: one launch each way."""

    @staticmethod
    def forward(ctx, q, k, v, scale):
        o, lse = ops.attn_short_fwd(q, k, v, scale, True)
        ctx.save_for_backward(q, k, v, o, lse)
        ctx.scale = scale
        return o

    @staticmethod
    def backward(ctx, do):
        q, k, v, o, lse = ctx.saved_tensors
        dq, dk, dv = ops.attn_short_bwd(_launcher_dout(do), q, k, v, o, lse, ctx.scale, True)
        return dq, dk, dv, None


def _kernels_ok(q, k, v, causal: bool, dropout: float) -> bool:
    """What both kernel families ask of a call, the sequence length aside: bf16 on the device, causal, no dropout, head_dim 64 /
    128, S % 16 == 0, whole GQA groups, and operands the launchers take (one batch of each below 2 GiB)."""
    if not (q.is_cuda and q.dtype == k.dtype == v.dtype == torch.bfloat16 and dropout == 0.0 and causal):
        return False
    B, S, H, D = q.shape
    if D not in (64, 128) or S % 16 or H % k.shape[2]:
        return False
    return all(_rows_ok(t, S, D) and S * t.stride(1) * 2 < 2 ** 31 for t in (q, k, v))


def _flash_ok(q, k, v, causal: bool, dropout: float) -> bool:
    return _kernels_ok(q, k, v, causal, dropout) and q.shape[1] >= 128


# The kernels take every S in 16 .. 112; the module sends them only the lengths at which forward + backward was measured faster
# than the SDPA route by more than that route's own spread (profiles/attn_short_ab.txt, eager calls): from this S up, by head_dim.
# Below it both routes cost one host launch path (~70 us) and SDPA's is the shorter one.
_SHORT_MIN_S = {128: 64, 64: 80}


def _short_ok(q, k, v, causal: bool, dropout: float) -> bool:
    """_flash_ok's conditions at the lengths below one 128-row block: 16 <= S < 128, S % 16 == 0 (from _SHORT_MIN_S up)."""
    return (os.environ.get("LLM_FP8_AMD_NO_SHORT_ATTN") != "1" and _kernels_ok(q, k, v, causal, dropout)
            and _SHORT_MIN_S[q.shape[3]] <= q.shape[1] < 128)


_BAND_MASKS = {}


def _band_mask(S: int, W: int, device) -> torch.Tensor:
    """[S, S] bool, True = attend: key j of query i with i - W < j <= i.  Built once per (S, W, device)."""
    key = (S, W, str(device))
    hit = _BAND_MASKS.get(key)
    if hit is None:
        i = torch.arange(S, device=device)
        d = i[:, None] - i[None, :]
        hit = (d >= 0) & (d < W)
        if len(_BAND_MASKS) > 16:
            _BAND_MASKS.clear()
        _BAND_MASKS[key] = hit
    return hit


_SEGMENTS = {}


def _segments(cu_seqlens: torch.Tensor, T: int):
    """ops.attn_segments(cu_seqlens, 1, T), built once per model forward and not once per layer: cached on the identity and the
    version of the `cu_seqlens` tensor (an in-place write to it bumps the version)."""
    key = (id(cu_seqlens), cu_seqlens._version, T)
    hit = _SEGMENTS.get(key)
    if hit is None or hit[0]() is not cu_seqlens:  # (the weak reference: an id can be reused by a later tensor)
        if len(_SEGMENTS) > 16:
            _SEGMENTS.clear()
        hit = _SEGMENTS[key] = (weakref.ref(cu_seqlens), ops.attn_segments(cu_seqlens, 1, T))
    return hit[1]


def _sdpa_mask(S: int, W: Optional[int], segments, device) -> Optional[torch.Tensor]:
    """[S, S] bool, True = attend, for the SDPA route: the causal band of W keys and / or the documents of `segments` (_segments'
    pair for one packed row); None where there is neither."""
    mask = None if W is None else _band_mask(S, W, device)
    if segments is not None:
        j = torch.arange(S, device=device)
        docs = (segments[0][0, :, None] <= j[None, :]) & (j[None, :] <= j[:, None])
        mask = docs if mask is None else docs & mask
    return mask


class DotProductAttention(torch.nn.Module):
    """bf16 attention core.  q [b,s,h,d], k/v [b,s,g,d] (bshd) -> [b,s,h*d].
    Packed sequences: `cu_seqlens_q` (int32 or int64 [n + 1], TE's cumulative document lengths) with a batch of 1, or with
    qkv_format="thd" (q [t,h,d], k/v [t,g,d] -> [t,h*d]); `cu_seqlens_kv` is None or the same tensor (self-attention).
    `window_size` = (left, right) as in TE: None or left < 0 is the full mask; with a causal mask type right is 0 or -1 and
    (left, 0) lets a query see itself and the `left` keys before it (W = left + 1)."""

    def __init__(self, num_attention_heads: int, kv_channels: int, num_gqa_groups: Optional[int] = None,
                 attention_dropout: float = 0.0, attn_mask_type: str = "causal", qkv_format: str = "bshd",
                 window_size: Optional[Tuple[int, int]] = None, **_ignored):
        super().__init__()
        self.h, self.d = num_attention_heads, kv_channels
        self.g = num_gqa_groups or num_attention_heads
        self.p, self.attn_mask_type, self.qkv_format = attention_dropout, attn_mask_type, qkv_format
        if window_size is not None:
            left, right = window_size
            causal = attn_mask_type in ("causal", "padding_causal")
            if causal and right not in (0, -1):
                raise ValueError(f"window_size={tuple(window_size)}: with a causal mask type `right` must be 0 or -1")
            if not causal and left >= 0 and right != 0:  # (left, 0) without a causal type is the same band; the rest is two-sided
                raise NotImplementedError(f"window_size={tuple(window_size)} with attn_mask_type={attn_mask_type!r}: two-sided "
                                          "windows are not implemented")
            window_size = (int(left), int(right)) if left >= 0 else None
        self.window_size = window_size  # None: the full mask

    def forward(self, q, k, v, attention_mask=None, cu_seqlens_q=None, cu_seqlens_kv=None, max_seqlen_q=None, max_seqlen_kv=None):
        causal = self.attn_mask_type in ("causal", "padding_causal")
        packed = cu_seqlens_q is not None or cu_seqlens_kv is not None or self.qkv_format == "thd"
        if packed:
            if cu_seqlens_q is None:
                raise ValueError("packed sequences (qkv_format='thd' or cu_seqlens_kv) need cu_seqlens_q")
            if cu_seqlens_kv is not None and cu_seqlens_kv is not cu_seqlens_q:
                raise NotImplementedError("cu_seqlens_kv must be None or the tensor passed as cu_seqlens_q: packed sequences are "
                                          "implemented for self-attention only")
            if not causal:
                raise NotImplementedError(f"cu_seqlens_q with attn_mask_type={self.attn_mask_type!r}: packed sequences are causal")
        # the caller's layout -> bshd
        if self.qkv_format == "thd":
            q, k, v = (t.unsqueeze(0) for t in (q, k, v))
        elif self.qkv_format == "sbhd":
            q, k, v = (t.transpose(0, 1) for t in (q, k, v))
        if packed and q.shape[0] != 1:
            raise ValueError(f"cu_seqlens_q with a batch of {q.shape[0]}: a packed row is [1, T] (or qkv_format='thd')")
        # the request: a band of W keys (a window at least as long as the sequence is the plain causal mask: None), the documents
        # of a packed row, dropout
        S = q.shape[1]
        W = self.window_size[0] + 1 if self.window_size is not None and self.window_size[0] + 1 < S else None
        segments = _segments(cu_seqlens_q, S) if packed else None
        dropout = self.p if self.training else 0.0
        # the route.  The kernels of mi_attn.hip take a band or the documents, not both, where _flash_ok takes the call; the switch
        # of a mask selects the SDPA route that its kernels are tested and timed against.  mi_attn_short.hip has the plain causal mask.
        switch = "LLM_FP8_AMD_NO_PACKED_ATTN" if packed else "LLM_FP8_AMD_NO_WINDOW_ATTN"
        plain, both = W is None and not packed, W is not None and packed
        if not both and (plain or os.environ.get(switch) != "1") and _flash_ok(q, k, v, causal, dropout):
            o = _FlashAttnFn.apply(q, k, v, self.d ** -0.5, True, W, segments)
        elif plain and _short_ok(q, k, v, causal, dropout):
            o = _ShortAttnFn.apply(q, k, v, self.d ** -0.5)
        else:
            mask = _sdpa_mask(S, W, segments, q.device)
            is_causal = causal and mask is None  # (a band or document mask holds the diagonal itself)
            if mask is None and not causal and attention_mask is not None:
                mask = ~attention_mask if attention_mask.dtype == torch.bool else attention_mask  # TE: True = masked out
            o = F.scaled_dot_product_attention(*(t.transpose(1, 2) for t in (q, k, v)), attn_mask=mask, dropout_p=dropout,
                                               is_causal=is_causal, enable_gqa=(self.g != self.h)).transpose(1, 2)
        # bshd -> the caller's layout
        if self.qkv_format == "thd":
            return o.reshape(o.shape[1], self.h * self.d)
        if self.qkv_format == "sbhd":
            o = o.transpose(0, 1)
        return o.reshape(*o.shape[:2], self.h * self.d)


class MultiheadAttention(torch.nn.Module):
    """`layernorm_qkv` (LayerNormLinear with query_/key_/value_weight) -> RoPE -> attention -> `proj` (Linear).

    Arguments follow te.pytorch.MultiheadAttention as called at te_llama.py:45-56.  The default mask type is
    causal and, as in TE, a padding `attention_mask` passed with the causal type is ignored
    (SURVEY.md 8a row a5)."""

    def __init__(self, hidden_size: int, num_attention_heads: int, kv_channels: Optional[int] = None,
                 attention_dropout: float = 0.1, layernorm_epsilon: float = 1e-5, init_method=None,
                 output_layer_init_method=None, attn_mask_type: str = "causal", num_gqa_groups: Optional[int] = None,
                 input_layernorm: bool = False, attention_type: str = "self", fuse_qkv_params: bool = False,
                 zero_centered_gamma: bool = False, qkv_weight_interleaved: bool = True, bias: bool = True,
                 normalization: str = "LayerNorm", qkv_format: str = "sbhd", params_dtype=None, device="cuda",
                 qk_norm_type: Optional[str] = None, qk_norm_eps: float = 1e-6, qk_norm_before_rope: bool = True,
                 window_size: Optional[Tuple[int, int]] = None, **_ignored):
        super().__init__()
        assert attention_type == "self", "only self-attention is on the reference path"
        assert qkv_format in ("sbhd", "bshd")
        if qk_norm_type not in (None, "RMSNorm"):
            raise NotImplementedError(f"qk_norm_type={qk_norm_type!r}: only None and 'RMSNorm' are implemented")
        if not qk_norm_before_rope:
            raise NotImplementedError("qk_norm_before_rope=False is not implemented: the QK norm is applied before RoPE")
        self.qk_norm_type, self.qk_norm_eps = qk_norm_type, qk_norm_eps
        self.hidden_size, self.h = hidden_size, num_attention_heads
        self.d = kv_channels or hidden_size // num_attention_heads
        self.g = num_gqa_groups or num_attention_heads
        self.qkv_format, self.input_layernorm = qkv_format, input_layernorm
        q_out, kv_out = self.h * self.d, self.g * self.d
        self.split = (q_out, kv_out, kv_out)
        if fuse_qkv_params:
            psplit = None
        else:
            psplit = {"query_": q_out, "key_": kv_out, "value_": kv_out}
        if input_layernorm:
            self.layernorm_qkv = LayerNormLinear(hidden_size, sum(self.split), eps=layernorm_epsilon, bias=bias,
                                                 normalization=normalization, parameters_split=psplit,
                                                 params_dtype=params_dtype, device=device,
                                                 zero_centered_gamma=zero_centered_gamma, init_method=init_method)
        else:
            self.qkv = Linear(hidden_size, sum(self.split), bias=bias, params_dtype=params_dtype, device=device,
                              init_method=init_method)
        self.core_attention = DotProductAttention(self.h, self.d, self.g, attention_dropout, attn_mask_type, qkv_format,
                                                  window_size=window_size)
        self.proj = Linear(q_out, hidden_size, bias=bias, params_dtype=params_dtype, device=device,
                           init_method=output_layer_init_method or init_method)
        if qk_norm_type == "RMSNorm":  # per-head norm over head_dim (HF Qwen3 `q_norm` / `k_norm`): one weight [d] each
            self.q_norm = RMSNorm(self.d, eps=qk_norm_eps, params_dtype=params_dtype, device=device)
            self.k_norm = RMSNorm(self.d, eps=qk_norm_eps, params_dtype=params_dtype, device=device)

    def forward(self, hidden_states: torch.Tensor, attention_mask: Optional[torch.Tensor] = None,
                rotary_pos_emb=None, _with_skip: bool = False, _rstd=None, cu_seqlens_q=None, **_ignored):
        """`_with_skip` (extension): returns (out, skip); `_rstd`: statistics hand-off, see LayerNormLinear.forward.
        `cu_seqlens_q`: packed sequences, see DotProductAttention (a batch of 1)."""
        cu = cu_seqlens_q
        if _with_skip:
            if not self.input_layernorm:
                return self._attend(self.qkv(hidden_states), attention_mask, rotary_pos_emb, cu_seqlens_q=cu), hidden_states
            # the rotary split's backward hands the projection its grad_output already in FP8 (module.DyHandoff): only
            # when the two are wired back to back right here
            handoff = DyHandoff() if (rotary_pos_emb is not None and hidden_states.is_cuda and torch.is_grad_enabled()
                                      and os.environ.get("LLM_FP8_AMD_NO_DY_HANDOFF") != "1") else None
            qkv, skip = self.layernorm_qkv(hidden_states, _with_skip=True, _rstd=_rstd, _dy_handoff=handoff)
            return self._attend(qkv, attention_mask, rotary_pos_emb, handoff, cu_seqlens_q=cu), skip
        qkv = self.layernorm_qkv(hidden_states) if self.input_layernorm else self.qkv(hidden_states)
        return self._attend(qkv, attention_mask, rotary_pos_emb, cu_seqlens_q=cu)

    def _attend_qk_norm(self, qkv: torch.Tensor, attention_mask, rotary_pos_emb, handoff, cu_seqlens_q=None) -> torch.Tensor:
        """`_attend` with the per-head RMSNorm of q and k in front of RoPE.  Neither route has an FP8-emitting backward, so the
        q|k|v projection quantises its own grad_output: the hand-off is withdrawn on both."""
        if handoff is not None:
            handoff.withdraw()
        gq, gk = self.q_norm.weight, self.k_norm.weight
        if (rotary_pos_emb is not None and not isinstance(rotary_pos_emb, (tuple, list)) and qkv.is_cuda
                and qkv.dtype == torch.bfloat16 and self.qkv_format == "bshd" and self.d in (64, 128)
                and rotary_pos_emb.shape[-1] == self.d and gq.dtype == gk.dtype == torch.bfloat16
                and os.environ.get("LLM_FP8_AMD_NO_QK_NORM_FUSION") != "1"):
            cos, sin = _cos_sin_tables(rotary_pos_emb, qkv.shape[1])
            q, k, v = _QKNormRoPESplitFn.apply(qkv, gq, gk, cos, sin, self.h, self.g, self.d, float(self.qk_norm_eps))
            return self.proj(self.core_attention(q, k, v, attention_mask, cu_seqlens_q=cu_seqlens_q))
        # the torch route (and the CPU route): split, norm on the [.., h, d] views, rotate
        q, k, v = torch.split(qkv, self.split, dim=-1)
        a, b = qkv.shape[0], qkv.shape[1]
        q = self.q_norm(q.reshape(a, b, self.h, self.d)).to(qkv.dtype)  # (autocast runs the norm in fp32)
        k = self.k_norm(k.reshape(a, b, self.g, self.d)).to(qkv.dtype)
        v = v.reshape(a, b, self.g, self.d)
        if rotary_pos_emb is not None:
            fq, fk = rotary_pos_emb if isinstance(rotary_pos_emb, (tuple, list)) else (rotary_pos_emb, rotary_pos_emb)
            q = apply_rotary_pos_emb(q, fq, self.qkv_format)
            k = apply_rotary_pos_emb(k, fk, self.qkv_format)
        return self.proj(self.core_attention(q, k, v, attention_mask, cu_seqlens_q=cu_seqlens_q))

    def _attend(self, qkv: torch.Tensor, attention_mask, rotary_pos_emb, handoff=None, cu_seqlens_q=None) -> torch.Tensor:
        if self.qk_norm_type is not None:
            return self._attend_qk_norm(qkv, attention_mask, rotary_pos_emb, handoff, cu_seqlens_q)
        if (rotary_pos_emb is not None and not isinstance(rotary_pos_emb, (tuple, list)) and qkv.is_cuda
                and qkv.dtype == torch.bfloat16 and self.qkv_format == "bshd" and self.d % 16 == 0
                and rotary_pos_emb.shape[-1] == self.d):
            cos, sin = _cos_sin_tables(rotary_pos_emb, qkv.shape[1])
            q, k, v = _RoPESplitFn.apply(qkv, cos, sin, self.h, self.g, self.d, handoff)
            return self.proj(self.core_attention(q, k, v, attention_mask, cu_seqlens_q=cu_seqlens_q))
        if handoff is not None:
            handoff.withdraw()  # not the fused rotary path: the projection quantises its own grad_output
        q, k, v = torch.split(qkv, self.split, dim=-1)
        a, b = qkv.shape[0], qkv.shape[1]
        q = q.reshape(a, b, self.h, self.d)
        k = k.reshape(a, b, self.g, self.d)
        v = v.reshape(a, b, self.g, self.d)
        if rotary_pos_emb is not None:
            fq, fk = rotary_pos_emb if isinstance(rotary_pos_emb, (tuple, list)) else (rotary_pos_emb, rotary_pos_emb)
            q = apply_rotary_pos_emb(q, fq, self.qkv_format)
            k = apply_rotary_pos_emb(k, fk, self.qkv_format)
        ctx = self.core_attention(q, k, v, attention_mask, cu_seqlens_q=cu_seqlens_q)
        return self.proj(ctx)
