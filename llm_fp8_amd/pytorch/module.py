"""FP8 modules with the `transformer_engine.pytorch` surface the reference consumes:
`Linear` (accelerate utils/transformer_engine.py:52-59), `LayerNormLinear` / `LayerNormMLP`
(te_llama.py:45-63 via MultiheadAttention / LayerNormMLP), same parameter names as
`replace_params` writes (te_llama.py:194-238).

Every GEMM site is ONE autograd Function (`_FP8LinearFn`) whose forward/backward run only HIP kernels
from libmi_fp8.so:

  fwd:  x  --cast+T+amax-->  x8, x8T     w  --cast+T+amax-->  w8, w8T      y  = gemm(x8, w8)  (+bias)
  bwd:  dy --cast+T+amax-->  g8, g8T     dx = gemm(g8, w8T)                dw = gemm(g8T, x8T)

(SURVEY.md 3.4).  Weights stay bf16 `nn.Parameter`s; nothing here falls back to PyTorch matmuls when
FP8 is enabled.  Outside `fp8_autocast` (or with enabled=False) the modules are plain bf16 layers.
"""
from __future__ import annotations

import io
import os
from typing import List, NamedTuple, Optional, Sequence, Tuple

import torch
import torch.nn.functional as F

from ..common.recipe import DelayedScaling, Float8BlockScaling, Float8CurrentScaling, Format, MXFP8BlockScaling, Recipe, fmt_codes
from . import ops
from .fp8 import FP8GlobalStateManager, ModuleMeta

__all__ = ["Linear", "LayerNormLinear", "LayerNormMLP", "LayerNorm", "RMSNorm"]


def _as_bf16_2d(t: torch.Tensor) -> torch.Tensor:
    t2 = t.reshape(-1, t.shape[-1])
    if t2.dtype != torch.bfloat16:
        t2 = t2.to(torch.bfloat16)
    return t2.contiguous()


class DyHandoff:
    """grad_output of an FP8 Linear delivered already quantised by the op that produces it.

    The Linear's forward `offer`s what its backward will quantise grad_output with (delayed scaling: scale and amax slot are
    known in advance); the producer's backward (attention._RoPESplitFn) then emits the FP8 copies itself, `put`s them here and
    returns an UNWRITTEN bf16 placeholder as the autograd gradient; the Linear's backward `take`s the copies and never reads
    the placeholder.  One object per forward call, private to the module that wires the two together: nothing else may sit
    between them in the graph.  `take` checks that the gradient it was handed is that placeholder and fails loudly otherwise.
    Guard: a producer asks `handoff_readers` first -- with a tensor hook or `retain_grad()` on the activation in between, or
    under anomaly mode, it writes the real gradient and the hand-off is skipped for that backward pass."""
    __slots__ = ("scale", "amax", "fmt", "want_y", "want_t", "fp8", "ptr", "mx", "act_ref")

    def __init__(self):
        self.scale = self.amax = self.fmt = self.fp8 = self.ptr = None
        self.act_ref = None  # weakref to the activation the user can reach (the logits): see handoff_readers
        self.want_y = self.want_t = self.mx = False

    def offer(self, scale, amax, fmt, want_y, want_t, mx: bool = False):
        """Delayed scaling: (scale, amax slot, format); MXFP8 (`mx`): the format only, the producer `put`s the four tensors of
        ops.mxfp8_quantize (rowwise data + scales, columnwise data + scales) instead of (y, yT)."""
        self.scale, self.amax, self.fmt, self.want_y, self.want_t, self.mx = scale, amax, fmt, want_y, want_t, mx

    def withdraw(self):
        self.scale, self.mx = None, False

    def offered(self) -> bool:
        return (self.scale is not None or self.mx) and (self.want_y or self.want_t)

    def put(self, fp8: tuple, placeholder: torch.Tensor):
        self.fp8, self.ptr = fp8, placeholder.untyped_storage().data_ptr()

    def take(self, dy: torch.Tensor):
        if dy.untyped_storage().data_ptr() != self.ptr:
            raise RuntimeError("DyHandoff: the gradient reaching the Linear is not the producer's placeholder "
                               "(an op was inserted between the q|k|v projection and the rotary split)")
        fp8, self.fp8, self.ptr = self.fp8, None, None
        return fp8


def handoff_readers(t) -> bool:
    """True when something may READ the bf16 gradient that flows from a DyHandoff producer to its Linear: a tensor hook or
    `retain_grad()` on the activation between them (`t`, the producer's input), or autograd's anomaly mode (it scans every
    gradient for NaNs).  The producer then takes its ordinary route -- it writes the real gradient, `put`s nothing, and the
    Linear quantises what it receives -- instead of handing an unwritten placeholder to code that would read garbage."""
    if torch.is_anomaly_enabled():
        return True
    if t is None:
        return False
    return bool(getattr(t, "retains_grad", False)) or bool(getattr(t, "_backward_hooks", None))


class _GemmSpec:
    """Everything non-tensor a GEMM site needs: recipe, meta windows, slot base, update trigger."""
    __slots__ = ("recipe", "meta_fwd", "meta_bwd", "g", "fmt_fwd", "fmt_bwd", "trigger_bwd_update", "training", "eps",
                 "wcache", "first_mb", "with_skip", "rstd", "dy_handoff", "defer_bias", "q")

    def __init__(self, recipe, meta_fwd, meta_bwd, g, trigger_bwd_update, training, eps=1e-5, wcache=None, first_mb=None,
                 with_skip=False, rstd=None, dy_handoff=None, defer_bias=False):
        self.dy_handoff = dy_handoff
        # LayerNormMLP (fused SwiGLU): under delayed scaling the fc1 bias is added inside the SwiGLU kernels (always, when there
        # is one) and -- defer_bias, both recipes -- the fc2 bias is left to the caller's residual add (residual_add_stats(..., bias=...)): TE's
        # bias + activation fusion.  The bias add costs 12 % of a K = 3072 GEMM in its epilogue and nothing in an HBM-bound kernel.
        self.defer_bias = defer_bias
        self.eps = eps
        # rstd: RMSNorm statistics of the input already computed by the producer of the input (residual_add_stats)
        self.rstd = rstd
        # with_skip: the Function also returns its input as a second output (the residual branch); the gradient arriving
        # over it is added inside the RMSNorm-backward kernel instead of by a separate autograd add
        self.with_skip = with_skip
        # FP8 weight caching across micro-batches (TE `is_first_microbatch`): None = cast every
        # forward (what the reference does), True = cast and keep, False = reuse the kept FP8 weights and their scale_inv
        self.wcache, self.first_mb = wcache, first_mb
        self.recipe, self.meta_fwd, self.meta_bwd, self.g = recipe, meta_fwd, meta_bwd, g
        self.fmt_fwd, self.fmt_bwd = fmt_codes(recipe.fp8_format)
        # q: what differs between the recipes at a GEMM site (the only place that chooses)
        if recipe.mxfp8():
            self.q = _MXQ(self.fmt_fwd, self.fmt_bwd)
        elif recipe.current():
            self.q = _CurrentQ(recipe, self.fmt_fwd, self.fmt_bwd)
        elif recipe.block():
            self.q = _BlockQ(recipe, self.fmt_fwd, self.fmt_bwd)
        else:
            self.q = _DelayedQ(meta_fwd, meta_bwd, self.fmt_fwd, self.fmt_bwd)
        self.trigger_bwd_update = trigger_bwd_update
        self.training = training


class _Sink:
    """What WeightSink and MXWeightSink share: `parts` = (weight, first row, rows) of the operand, announced to the optimiser on the
    weights themselves, and `stamp` = what `_now()` gave when the optimiser last rewrote every part (the copies are current while
    it still gives that)."""
    __slots__ = ("parts", "stamp")
    # what the optimiser needs to know of a sink class (optim.ClippedAdamW): `attr` = the name the parts are announced under,
    # `unit` = what rows, cols (and, MXFP8, the row offset of a part) must be multiples of, `kind` = sink_kind of the C ABI;
    # table_rows(r0, K) = rows 6..11 of the device table for the [*, K] part at row r0 of the operand (include/mi_fp8.h)

    def _register(self, weights, ns) -> None:
        self.parts, r = [], 0
        for w, n in zip(weights, ns):
            self.parts.append((w, r, n))
            setattr(w, self.attr, (self, r, n))
            r += n
        self.stamp = None

    def holds(self, weights, mf) -> bool:
        return len(self.parts) == len(weights) and all(a is b for (a, _, _), b in zip(self.parts, weights))

    def _now(self):
        return _part_versions(self.parts)

    def fresh(self) -> bool:
        return self.stamp is not None and self.stamp == self._now()

    def mark(self) -> None:  # called by the optimiser after it rewrote every part in this step
        self.stamp = self._now()


class WeightSink(_Sink):
    """FP8 copies (w8 [N,K], w8T [K,N]) of one GEMM's weight operand that the OPTIMISER keeps current (optim.ClippedAdamW ->
    mi_adamw_cast_bf16_multi): under delayed scaling the scale of the next forward's weight cast is final once this step's
    forward has ended, and the optimiser streams every weight anyway, so it emits the bytes (and the amax) that forward
    would have produced -- bitwise -- and the forward skips its weight casts (141 launches and one read of all weights per
    step on Llama-3.2-3B).  `stamp` = (versions of the parts, generation of the scale arena) at emission; the copies are used
    only while both still match (no other write to the weights, no scale update in between: an evaluation pass or a second
    micro-batch re-casts as before)."""
    __slots__ = ("w8", "w8t", "arena", "scale", "amax")
    attr, unit, kind = "_mi_fp8_sink", 8, 0

    def __init__(self, weights, ns, N, K, dev, mf, slot):
        self.w8 = torch.empty((N, K), dtype=torch.uint8, device=dev)
        self.w8t = torch.empty((K, N), dtype=torch.uint8, device=dev)
        self.arena, self.scale, self.amax = mf.arena, mf.scale(slot), mf.amax(slot)
        self._register(weights, ns)

    def table_rows(self, r0, K):  # y, yT, ld_y, ld_yT, scale, amax
        return (self.w8.data_ptr() + r0 * K, self.w8t.data_ptr() + r0, K, self.w8.shape[0], self.scale.data_ptr(), self.amax.data_ptr())

    def holds(self, weights, mf) -> bool:
        return self.arena is mf.arena and super().holds(weights, mf)

    def _now(self):
        return _part_versions(self.parts), self.arena.generation


class MXWeightSink(_Sink):
    """MXFP8 copies (row-wise w8 [N,K] + E8M0 [K/32,N]; column-wise, stored transposed, wt8 [K,N] + E8M0 [N/32,K]) of one GEMM's
    weight operand that the OPTIMISER keeps current (optim.ClippedAdamW -> mi_adamw_mxcast_bf16_multi).  Block scaling has no
    state, so the only condition for using them is that nobody wrote the weights since: `stamp` = versions of the parts."""
    __slots__ = ("w8", "sc", "wt8", "sct")
    attr, unit, kind = "_mi_mx_sink", 32, 1

    def __init__(self, weights, ns, N, K, dev):
        self.w8 = torch.empty((N, K), dtype=torch.uint8, device=dev)
        self.sc = torch.empty((K // 32, N), dtype=torch.uint8, device=dev)
        self.wt8 = torch.empty((K, N), dtype=torch.uint8, device=dev)
        self.sct = torch.empty((N // 32, K), dtype=torch.uint8, device=dev)
        self._register(weights, ns)

    def table_rows(self, r0, K):  # y_row, s_row, y_colT, s_colT, ldr, unused
        return (self.w8.data_ptr() + r0 * K, self.sc.data_ptr() + r0, self.wt8.data_ptr() + r0, self.sct.data_ptr() + (r0 // 32) * K,
                self.w8.shape[0], 0)


def stepped_tensor(w):
    """The tensor the optimiser writes for a weight part: a row-sharded weight (distributed.ShardedFP8DP) is updated through its
    shard -- the module's Parameter is a storage-less view whose version never moves -- any other weight is itself."""
    h = getattr(w, "_mi_sharded", None)
    return w if h is None else h.shard


def _part_versions(parts) -> tuple:
    return tuple(stepped_tensor(w)._version for w, _, _ in parts)


# LLM_FP8_AMD_NO_MLP_BIAS_FUSION=1: keep both MLP biases in the GEMM epilogues (the round-2 behaviour; A/B switch)
_FUSE_MLP_BIAS = os.environ.get("LLM_FP8_AMD_NO_MLP_BIAS_FUSION") != "1"


def weight_sinks_enabled() -> bool:
    return os.environ.get("LLM_FP8_AMD_NO_OPT_WCAST") != "1"


def sharded_handle(weights):
    """distributed.ShardedFP8DP marks a weight whose bf16 master rows live 1/world per rank with `_mi_sharded` (the Parameter the
    module holds keeps its logical shape but no storage).  Such an operand has ONE source of FP8 bytes: its sink, filled by the
    optimiser's rows + an FP8 all-gather -- or, whenever the sink is not current (first step, scale arena moved on, checkpoint
    load, evaluation first), by `handle.dp.refresh_*`: quantise the local rows now and gather.  Returns the handle or None; a
    mix of sharded and replicated parts in one operand is refused."""
    hs = [getattr(w, "_mi_sharded", None) for w in weights]
    if all(h is None for h in hs):
        return None
    if any(h is None for h in hs):
        raise RuntimeError("an FP8 GEMM operand mixes row-sharded and replicated weight parts (distributed.ShardedFP8DP shards all "
                           "parts of an operand or none)")
    return hs[0]


def _master(w):
    """The bf16 master of a weight for the unquantised path (FP8 disabled): a row-sharded weight has none on this rank."""
    if getattr(w, "_mi_sharded", None) is not None and not w.is_contiguous():
        raise RuntimeError("this weight is row-sharded (distributed.ShardedFP8DP): its bf16 master exists 1/world per rank, so the "
                           "unquantised path cannot run -- keep FP8 enabled, or materialise the masters first with "
                           "dp.gather_master_weights() (and dp.reshard() afterwards)")
    return w


def _weight_ok_for_sink(w, K: int) -> bool:
    return (isinstance(w, torch.nn.Parameter) and w.dtype == torch.bfloat16 and w.dim() == 2 and w.shape[1] == K
            and (w.is_contiguous() or getattr(w, "_mi_sharded", None) is not None))


# What differs between the recipes at a GEMM site, behind the same few methods (`_GemmSpec.q` is one of the four classes below).  A quantised
# operand has one shape under both: (row, col), the row-wise copy [R, C] and the column-wise one, stored transposed [C, R], each a
# (data, scale) pair -- None data where the copy was not asked for.  `scale` is the one-element scale-inverse under delayed and
# current scaling and the block-major E8M0 tensor under MXFP8.  A GEMM contracts the row-wise copies of its operands: the forward takes `row` of
# the input and the weight, the backward pair takes `col` of both with the two copies of grad_output.  `g` is the GEMM's index in
# its module.  Each scaling granularity has ONE host path: _TensorQ (one scale per tensor) for delayed and current scaling, _MXQ
# (block scales) for MXFP8 and Float8BlockScaling; the concrete classes only say where a quantisation's numbers come from.


def _bf16_rows(w):
    """A weight part as the cast kernels read it: bf16 and contiguous -- the part itself where it already is both."""
    return (w if w.dtype == torch.bfloat16 else w.to(torch.bfloat16)).contiguous()


class _TensorQ:
    """Per-tensor scaling, what delayed and current scaling share: one fp32 scale per quantisation read by the cast kernels
    (ops.cast_amax and its fused producers), operands = FP8 bytes with a one-element scale-inverse, ops.gemm_fp8.  A subclass
    answers the two hooks -- where the numbers of one quantisation come from -- and keeps what is its own: the DyHandoff
    (`offer`, `taken`) and the optimiser-filled weight copies (`new_sink`, `refresh`, `sink_flat`)."""
    __slots__ = ("fmt_f", "fmt_b")

    # -- the two hooks; `role` is "x" (input of GEMM `g`), "w" (its weight) or "grad" (its grad_output) --
    def _scale(self, role: str, g: int, measure):
        """Asked before the cast is launched: (scale the cast reads, where it publishes its amax or None, `own`: handed back to
        _scale_inv).  `measure()` runs the amax pass(es) over the value the cast will see and returns their partials; a recipe that
        knows its scale in advance never calls it."""
        raise NotImplementedError

    def _scale_inv(self, role: str, g: int, own):
        """Asked after the cast was launched: the scale-inverse carried by (the row-wise copy, the column-wise copy)."""
        raise NotImplementedError

    @staticmethod
    def _amax_pass(fn, dev, grid, *args):
        """The measure step of one tensor: the pass `fn` (ops.amax_*) over `args` with ops.amax_grid(*grid) workgroups, into the
        device's partial buffer."""
        def measure():
            part = ops.amax_partial(dev, ops.amax_grid(*grid))
            fn(*args, part)
            return part
        return measure

    def _pairs(self, role: str, g: int, own, y, yT):
        si, si_t = self._scale_inv(role, g, own)
        return (y, si), (yT, si_t)

    def quantize(self, x2, g: int, want_t: bool, norm=None):
        """`norm` = (rstd, gamma): x2 is un-normalised and RMSNorm is fused into the cast."""
        if norm is None:
            scale, amax, own = self._scale("x", g, self._amax_pass(ops.amax_bf16, x2.device, x2.shape, x2))
            y, yT = ops.cast_amax(x2, scale, amax, self.fmt_f, want_t=want_t)
        else:
            scale, amax, own = self._scale("x", g, self._amax_pass(ops.amax_norm, x2.device, x2.shape, x2, norm[0], norm[1]))
            y, yT = ops.norm_cast(x2, norm[0], norm[1], scale, amax, self.fmt_f, want_t=want_t)
        return self._pairs("x", g, own, y, yT)

    def swiglu(self, h, g: int, want_t: bool, bias):
        scale, amax, own = self._scale("x", g, self._amax_pass(ops.amax_swiglu, h.device, (h.shape[0], h.shape[1] // 2, 32), h, bias))
        y, yT = ops.swiglu_cast(h, scale, amax, self.fmt_f, want_t=want_t, bias=bias)
        return self._pairs("x", g, own, y, yT)

    def quantize_grad(self, g2, g: int, want_y: bool, want_t: bool, colsum: bool = False):
        """-> (row, col, partial column sums or None)"""
        scale, amax, own = self._scale("grad", g, self._amax_pass(ops.amax_bf16, g2.device, g2.shape, g2))
        out = ops.cast_amax(g2, scale, amax, self.fmt_b, want_y=want_y, want_t=want_t, want_colsum=colsum)
        return (*self._pairs("grad", g, own, out[0], out[1]), out[2] if colsum else None)

    def dswiglu(self, h, dact, g: int, want_y: bool, want_t: bool, colsum: bool, bias):
        scale, amax, own = self._scale("grad", g, self._amax_pass(ops.amax_dswiglu, h.device, (h.shape[0], h.shape[1] // 2, 32),
                                                                   h, bias, dact))
        y, yT, cs = ops.dswiglu_cast(h, dact, scale, amax, self.fmt_b, want_y=want_y, want_t=want_t, want_colsum=colsum, bias=bias)
        return (*self._pairs("grad", g, own, y, yT), cs)

    def operands(self, a, b):
        """One GEMM's operand tuple as ops.gemm_fp8 and _grouped_or_two take it."""
        return a[0], b[0], a[1], b[1]

    def gemm(self, a, b, bias):
        return ops.gemm_fp8(a[0], b[0], a[1], b[1], self.fmt_f, self.fmt_f, bias=bias)

    # -- weights: `flat` is what the micro-batch cache holds under (cache_key, g) --
    def unflat(self, flat):
        w8, w8t, siw = flat
        return (w8, siw), (w8t, siw)

    def quantize_weights(self, weights, ns, N: int, K: int, dev, g: int, want_t: bool):
        """One scale for the whole operand (query | key | value), every part cast into its row-block.  Where the scale is measured,
        every part's amax pass fills its own segment of the partial buffer and ONE scale kernel covers all segments."""
        ws_ = list(weights)

        def measure():
            ws_[:] = [_bf16_rows(w) for w in ws_]           # (the casts below then take these as they are)
            grids = [ops.amax_grid(n, K) for n in ns]
            part, o = ops.amax_partial(dev, sum(grids)), 0
            for w, n in zip(ws_, grids):
                ops.amax_bf16(w, part[o:o + n])
                o += n
            return part

        scale, amax, own = self._scale("w", g, measure)
        w8 = torch.empty((N, K), dtype=torch.uint8, device=dev)
        w8t = torch.empty((K, N), dtype=torch.uint8, device=dev) if want_t else None
        r = 0
        for w, n in zip(ws_, ns):
            ops.cast_amax(_bf16_rows(w), scale, amax, self.fmt_f, y=w8[r:r + n], yT=None if w8t is None else w8t[:, r:r + n], want_t=want_t)
            r += n
        return w8, w8t, self._scale_inv("w", g, own)[1]


class _DelayedQ(_TensorQ):
    """Delayed scaling.  Meta slots of GEMM `g`: forward 3g = input, 3g + 1 = weight; backward 2g = grad_output: the scale is known in
    advance, the cast publishes its amax into the slot, nothing is measured.  What the forward saves for backward (`col` of an
    activation, both copies of a weight) carries the scale-inverse from scale_inv_snapshot() as of its quantisation -- the arena is
    rewritten at autocast exit, before backward; the snapshot is not -- while `row` of an activation and both copies of a
    grad_output, consumed in the pass that makes them, carry the live one."""
    __slots__ = ("mf", "mb")
    mx = False
    cache_key, sink_key = "ds", "sink"
    no_sink = "row-sharded weights of this shape cannot take an FP8 sink"
    swiglu_adds_bias = True     # the fc1 bias of the fused MLP is added inside the SwiGLU kernels
    colsum_dtypes = None        # a Linear's bias gradient rides on the cast of dy whatever the bias dtype

    def __init__(self, mf, mb, fmt_f: int, fmt_b: int):
        self.mf, self.mb, self.fmt_f, self.fmt_b = mf, mb, fmt_f, fmt_b

    def _slot(self, role: str, g: int):
        return (self.mb, 2 * g) if role == "grad" else (self.mf, 3 * g + (role == "w"))

    def _scale(self, role: str, g: int, measure):
        m, s = self._slot(role, g)
        return m.scale(s), m.amax(s), None

    def _scale_inv(self, role: str, g: int, own):
        m, s = self._slot(role, g)
        if role == "grad":
            si = m.scale_inv(s)
            return si, si
        # (the arena makes its snapshot -- one device copy per step -- when first asked: behind the step's first cast)
        saved = m.scale_inv_snapshot()[s:s + 1]
        return (m.scale_inv(s) if role == "x" else saved), saved

    def offer(self, handoff: DyHandoff, g: int, want_y: bool, want_t: bool) -> None:
        if self.mb is not None:
            handoff.offer(self.mb.scale(2 * g), self.mb.amax(2 * g), self.fmt_b, want_y, want_t)

    def taken(self, fp8, g: int):
        """(y, yT) that a DyHandoff producer `put`, as quantize_grad returns them."""
        return (*self._pairs("grad", g, None, fp8[0], fp8[1]), None)

    def new_sink(self, weights, ns, N: int, K: int, dev, g: int):  # None: an operand of this shape cannot take a sink
        return WeightSink(weights, ns, N, K, dev, self.mf, 3 * g + 1) if N % 8 == 0 and K % 8 == 0 else None

    def refresh(self, dp, sink) -> None:
        # the bytes in the sink were quantised with another scale generation (or never): the only bf16 source is the ranks'
        # shards -- cast the local rows with the CURRENT scale and gather (what a replicated run's forward cast does)
        dp.refresh_operand(sink, self.fmt_f)

    def sink_flat(self, sink, g: int):
        return sink.w8, sink.w8t, self.mf.scale_inv_snapshot()[3 * g + 1:3 * g + 2]


class _MXQ:
    """MXFP8 block scaling: no state, every quantisation finds its own E8M0 scales."""
    __slots__ = ("fmt_f", "fmt_b")
    mx = True
    cache_key, sink_key = "mx", "mxsink"
    no_sink = "row-sharded weights of this shape cannot take an MXFP8 sink"
    swiglu_adds_bias = False    # the quantising SwiGLU kernels have no bias form: the fc1 bias stays in the GEMM epilogue
    colsum_dtypes = (torch.bfloat16, torch.float32)  # ... only for these bias dtypes, else g2.sum(0)

    def __init__(self, fmt_f: int, fmt_b: int):
        self.fmt_f, self.fmt_b = fmt_f, fmt_b

    # -- the two hooks of a subclass with another scaling granularity (_BlockQ) --
    def _gran(self, role: str):
        """(block dim, amax_epsilon) of `role` ("x": input, "w": weight, "grad": grad_output), or None: MX's 32-element blocks."""
        return None

    def _part_rows(self) -> int:
        """The row multiple at which a weight part can be quantised into its row-block of the operand, without concatenation."""
        return 32

    def _plain(self, role: str, x, fmt: int, **kw):
        """The plain quantiser at the granularity of `role`, through the public pair of ops."""
        gran = self._gran(role)
        if gran is None:
            return ops.mxfp8_quantize(x, fmt, **kw)
        return ops.blockfp8_quantize(x, fmt, gran[0], amax_epsilon=gran[1], **kw)

    def quantize(self, x2, g: int, want_t: bool, norm=None):
        if norm is None:
            q = self._plain("x", x2, self.fmt_f, rowwise=True, colwise=want_t)
        else:
            q = ops._norm_quantize(x2, norm[0], norm[1], self.fmt_f, True, want_t, self._gran("x"))
        return q[:2], q[2:]

    def swiglu(self, h, g: int, want_t: bool, bias):
        assert bias is None
        q = ops._swiglu_quantize(h, self.fmt_f, True, want_t, self._gran("x"))
        return q[:2], q[2:]

    def quantize_grad(self, g2, g: int, want_y: bool, want_t: bool, colsum: bool = False):
        q = self._plain("grad", g2, self.fmt_b, rowwise=want_y, colwise=want_t, want_colsum=colsum)
        return q[:2], q[2:4], q[4] if colsum else None

    def dswiglu(self, h, dact, g: int, want_y: bool, want_t: bool, colsum: bool, bias):
        assert bias is None
        q = ops._dswiglu_quantize(h, dact, self.fmt_b, want_y, want_t, colsum, self._gran("grad"))
        return q[:2], q[2:4], q[4]

    def offer(self, handoff: DyHandoff, g: int, want_y: bool, want_t: bool) -> None:
        handoff.offer(None, None, self.fmt_b, want_y, want_t, mx=True)

    def taken(self, fp8, g: int):
        return fp8[:2], fp8[2:], None

    def operands(self, a, b):
        """One GEMM's operand tuple as ops.gemm_mxfp8 and _grouped_or_two take it."""
        return a + b

    def gemm(self, a, b, bias):
        return ops.gemm_mxfp8(a[0], a[1], b[0], b[1], self.fmt_f, self.fmt_f, bias=bias)

    def unflat(self, flat):
        return flat[:2], flat[2:]

    def quantize_weights(self, weights, ns, N: int, K: int, dev, g: int, want_t: bool):
        """Every part is quantised straight into its row-block of the operand's buffers (mi_mxfp8_quantize_ex / mi_blockfp8_quantize_ex),
        no bf16 concatenation -- unless a part's rows are no multiple of _part_rows().  One launch per part emits both copies."""
        fmt = self.fmt_f
        ws_ = [_bf16_rows(w) for w in weights]
        if len(ws_) == 1:
            return self._plain("w", ws_[0], fmt, rowwise=True, colwise=want_t)
        if any(n % self._part_rows() for n in ns):
            return self._plain("w", torch.cat(ws_, 0), fmt, rowwise=True, colwise=want_t)
        w8 = torch.empty((N, K), dtype=torch.uint8, device=dev)
        sc = torch.empty((K // 32, N), dtype=torch.uint8, device=dev)
        wt8 = torch.empty((K, N), dtype=torch.uint8, device=dev) if want_t else None
        sct = torch.empty((N // 32, K), dtype=torch.uint8, device=dev) if want_t else None
        r = 0
        for w, n in zip(ws_, ns):
            self._plain("w", w, fmt, rowwise=True, colwise=want_t,
                        out=(w8[r:r + n], sc[:, r:r + n], wt8[:, r:r + n] if want_t else None, sct[r // 32:(r + n) // 32] if want_t else None))
            r += n
        return w8, sc, wt8, sct

    def new_sink(self, weights, ns, N: int, K: int, dev, g: int):
        return MXWeightSink(weights, ns, N, K, dev) if N % 32 == 0 and K % 32 == 0 and all(n % 32 == 0 for n in ns) else None

    def refresh(self, dp, sink) -> None:
        dp.refresh_mx_operand(sink, self.fmt_f)

    def sink_flat(self, sink, g: int):
        return sink.w8, sink.sc, sink.wt8, sink.sct


class _BlockQ(_MXQ):
    """Float8BlockScaling: no state; every quantisation finds one power-of-two scale per 1 x 128 block along the contraction axis
    (scaling dim 1) or per 128 x 128 block (dim 2) and stores its inverse as the E8M0 byte of every 32-group the block covers, in
    the MX operand layout.  An operand therefore IS an MXFP8 operand: `operands`, `gemm`, `unflat`, the grouped dgrad + wgrad
    launch and its autotune key are _MXQ's.  With 128 x 128 weight blocks the column-wise weight copy is the byte transpose of the
    row-wise one under the same scales, so the forward and dgrad GEMMs see one quantised weight."""
    __slots__ = ("recipe",)
    cache_key, sink_key = "blk", "blksink"
    # the optimiser pass has no form that emits block-scaled copies (a 128 x 128 block's amax needs 128 updated rows before any of
    # them can be cast): no sink, the forward quantises the weights (the is_first_microbatch cache still keeps them across a
    # window) -- and distributed.ShardedFP8DP, which lives on optimiser-filled sinks, cannot run this recipe
    no_sink = ("Float8BlockScaling keeps no optimiser-filled FP8 weight copies, which row-sharded weights (distributed.ShardedFP8DP, "
               "--sharding_mode fsdp_fp8) depend on: use --sharding_mode replicated (GradArenaDP) with this recipe")

    def __init__(self, recipe: Float8BlockScaling, fmt_f: int, fmt_b: int):
        super().__init__(fmt_f, fmt_b)
        self.recipe = recipe

    def _gran(self, role: str):
        r = self.recipe
        if role == "x":
            return r.x_block_scaling_dim, r.fp8_quant_fwd_inp.amax_epsilon
        if role == "w":
            return r.w_block_scaling_dim, r.fp8_quant_fwd_weight.amax_epsilon
        return r.grad_block_scaling_dim, r.fp8_quant_bwd_grad.amax_epsilon

    def _part_rows(self) -> int:  # with 128 x 128 blocks a part has to fill whole block rows; 1 x 128 blocks only need the layout's unit
        return 128 if self.recipe.w_block_scaling_dim == 2 else 32

    def offer(self, handoff: DyHandoff, g: int, want_y: bool, want_t: bool) -> None:
        """Nothing: no DyHandoff producer has a block-scaled form.  RoPE backward and cross-entropy backward take their bf16 route
        and the Linear quantises the gradient it receives."""

    def taken(self, fp8, g: int):
        raise RuntimeError("Float8BlockScaling offers no DyHandoff, so no producer can have put FP8 copies into one")

    def new_sink(self, weights, ns, N: int, K: int, dev, g: int):
        return None


class _CurrentQ(_TensorQ):
    """Current scaling (Float8CurrentScaling): every quantisation is an amax pass over the tensor (the measure step, ops.amax_*: the
    value the cast will see, recomputed where the producer is fused), the scale kernel (ops.current_scale -> a fresh [amax, scale,
    scale_inv]) and the cast kernel delayed scaling uses, reading that scale and publishing no amax.  No history, no meta slots,
    nothing to update at autocast exit.  Operands are those of delayed scaling -- FP8 bytes with a one-element scale-inverse, here a
    view of the quantisation's own triple, which is what the saved column-wise copies carry into backward -- so the GEMMs, the
    grouped dgrad + wgrad launch and the algorithm table apply unchanged."""
    __slots__ = ("recipe",)
    _QPARAMS = {"x": "fp8_quant_fwd_inp", "w": "fp8_quant_fwd_weight", "grad": "fp8_quant_bwd_grad"}
    mx = False
    cache_key, sink_key = "cs", "cssink"
    # the optimiser cannot emit current-scaled bytes in its single pass over a weight (the scale needs the updated weight's amax
    # first): no sink, the forward quantises the weights (the is_first_microbatch cache still keeps them across a window) -- and
    # distributed.ShardedFP8DP, which lives on optimiser-filled sinks, cannot run this recipe
    no_sink = ("Float8CurrentScaling keeps no optimiser-filled FP8 weight copies, which row-sharded weights (distributed.ShardedFP8DP, "
               "--sharding_mode fsdp_fp8) depend on: use --sharding_mode replicated (GradArenaDP) with this recipe")
    swiglu_adds_bias = True
    colsum_dtypes = None

    def __init__(self, recipe: Float8CurrentScaling, fmt_f: int, fmt_b: int):
        self.recipe, self.fmt_f, self.fmt_b = recipe, fmt_f, fmt_b

    def _scale(self, role: str, g: int, measure):
        qp = getattr(self.recipe, self._QPARAMS[role])
        t3 = ops.current_scale(measure(), ops.FP8_MAX[self.fmt_b if role == "grad" else self.fmt_f], qp.amax_epsilon, qp.power_2_scale)
        return t3[1:2], None, t3

    def _scale_inv(self, role: str, g: int, t3):
        return t3[2:3], t3[2:3]

    def offer(self, handoff: DyHandoff, g: int, want_y: bool, want_t: bool) -> None:
        """Nothing: a DyHandoff producer needs the scale of grad_output before it has produced it.  RoPE backward and cross-entropy
        backward take their bf16 route and the Linear quantises the gradient it receives."""

    def taken(self, fp8, g: int):
        raise RuntimeError("Float8CurrentScaling offers no DyHandoff, so no producer can have put FP8 copies into one")

    def new_sink(self, weights, ns, N: int, K: int, dev, g: int):
        return None


def _weight_operand(spec: _GemmSpec, g: int, weights, ns, N: int, K: int, dev, need_t: bool):
    """FP8 copies (row, col) of the concatenated weight parts of GEMM `g` (query | key | value): from the micro-batch cache of
    the spec (see _GemmSpec), else from the sink the optimiser keeps current, else quantised now."""
    q, wc = spec.q, spec.wcache
    ck = (q.cache_key, g)
    if spec.first_mb is False and wc is not None:
        hit = wc.get(ck)
        if hit is not None:
            op = q.unflat(hit)
            if op[1][0] is not None or not need_t:
                return op
    # (no grad-mode test here: inside an autograd Function's forward grad mode is always off; fresh copies are the bytes a
    # cast would produce now in any mode)
    keep = spec.first_mb is True and wc is not None
    shard = sharded_handle(weights)
    if shard is not None and (wc is None or spec.fmt_fwd != 0):
        raise RuntimeError("row-sharded weights need the module's FP8 weight cache and an E4M3 forward format")
    flat = None
    if wc is not None and spec.fmt_fwd == 0 and (weight_sinks_enabled() or shard is not None):
        sink = wc.get((q.sink_key, g))
        if sink is None or not sink.holds(weights, spec.meta_fwd):
            # a training pass creates the sink the first time round and the optimiser fills it at its next step; an evaluation
            # pass may USE a fresh one (same bytes).  Row-sharded weights always go through the sink.
            sink = None
            if (spec.training or shard is not None) and all(_weight_ok_for_sink(w, K) for w in weights):
                sink = q.new_sink(weights, ns, N, K, dev, g)
                if sink is not None:
                    wc[(q.sink_key, g)] = sink
        if shard is not None:
            if sink is None:
                raise RuntimeError(q.no_sink)
            shard.dp.wait_operand(sink)        # an FP8 all-gather issued after the optimiser step may still be in flight
            if not sink.fresh():
                q.refresh(shard.dp, sink)
        if sink is not None and sink.fresh():
            flat = q.sink_flat(sink, g)
    if flat is None:
        flat = q.quantize_weights(weights, ns, N, K, dev, g, need_t or keep)
    if keep:
        wc[ck] = flat
    return q.unflat(flat)


class _AddStatsFn(torch.autograd.Function):
    """out = a + b (+ bias) and the RMSNorm statistics of `out` in one pass (mi_add_rmsnorm_stats / mi_add_bias_rmsnorm_stats).
    `bias`: a detached tensor -- the gradient of a deferred bias is produced by the module that owns it (column sums of dy)."""

    @staticmethod
    def forward(ctx, a, b, eps, bias=None):
        out, rstd = ops.add_rmsnorm_stats(a, b, eps, bias=bias)
        ctx.mark_non_differentiable(rstd)
        ctx.set_materialize_grads(False)  # autograd otherwise zero-fills a [tokens] fp32 gradient for rstd in every backward
        return out, rstd

    @staticmethod
    def backward(ctx, dout, _drstd):
        return dout, dout, None, None


def residual_add_stats(a: torch.Tensor, b: torch.Tensor, eps: float, bias: Optional[torch.Tensor] = None):
    """`a + b` for the residual stream, plus rstd (or None) for the RMSNorm that consumes the sum: (sum, rstd).
    `bias`: the deferred output bias of the module that produced `b` (LayerNormMLP(..., _defer_bias=True)): out = a + (b + bias)."""
    if (a.is_cuda and a.dtype == torch.bfloat16 and b.dtype == torch.bfloat16 and a.shape == b.shape and a.is_contiguous()
            and b.is_contiguous() and a.shape[-1] % 8 == 0 and (bias is None or a.shape[-1] == bias.numel())):
        bb = None if bias is None else bias.detach().to(torch.bfloat16).contiguous()
        return _AddStatsFn.apply(a, b, eps, bb)
    if bias is not None:
        b = b + bias.detach().to(b.dtype)
    return a + b, None


def _wgrad_out(weights, K: int) -> Optional[torch.Tensor]:
    """Destination of the weight-gradient GEMM inside the data-parallel gradient arena (distributed.GradArenaDP): the
    [sum N_i, K] block formed by the weights' slots when these are adjacent and in order, the parameters are bf16 and
    nothing has been accumulated into them yet (gradient accumulation adds into `.grad` instead).  None otherwise."""
    shard = getattr(weights[0], "_mi_sharded", None)
    if shard is not None:  # distributed.ShardedFP8DP: a transient [sum N_i, K] buffer that lives until its reduce-scatter has run
        return shard.dp.wgrad_buffer(weights, K)
    slot = getattr(weights[0], "_mi_grad_slot", None)
    if slot is None:
        return None
    arena, off = slot
    if arena.dtype != torch.bfloat16:
        return None
    end = off
    for w in weights:
        s = getattr(w, "_mi_grad_slot", None)
        if s is None or s[0] is not arena or s[1] != end or w.grad is not None or w.dtype != torch.bfloat16 or w.shape[1] != K:
            return None
        end += w.numel()
    return arena[off:end].view(-1, K)


def _grouped_or_two(q, grad, w_col, x_col, dw_out, need_dgrad: bool, need_wgrad: bool):
    """A Linear's two backward GEMMs on one grad_output: dX [M, K] = G8 [M, N] . W8T [K, N]^T and dW [N, K] = G8T [N, M] . X8T [K, M]^T;
    `grad` = (row, col[, column sums]) of grad_output, `w_col` / `x_col` the column-wise copies the forward saved.
    ONE grouped persistent launch (ops.gemm_fp8_grouped / ops.gemm_mxfp8_grouped) where that is faster (ops.grouped_gemm_choice:
    measured once per shape in a single-process run, the count model under torch.distributed; env LLM_FP8_AMD_GROUPED_GEMM =
    auto | plan | autotune | off) -- one ramp, one exposed epilogue, and the short problem's tiles fill the idle part of the long
    one's last round -- else two launches.  Bitwise the same results either way; `dw_out` (the gradient-arena slot) stays the
    wgrad's output.  (Under torch.distributed the GEMMs run one workgroup per tile so that RCCL's kernels get CUs: no persistent
    grouping there.)"""
    dgrad, wgrad, mx, fmt_b, fmt_f = q.operands(grad[0], w_col), q.operands(grad[1], x_col), q.mx, q.fmt_b, q.fmt_f
    if need_dgrad and need_wgrad and ops.default_gemm_algo() in (0, 4, 47) and os.environ.get("LLM_FP8_AMD_NO_GROUPED_GEMM") != "1":
        g8, wt8 = dgrad[0], dgrad[2 if mx else 1]
        M, N = g8.shape
        K = wt8.shape[0]
        # per-tensor operands may be row-strided views; block-scaled operands and their scales are tight
        layout_ok = (all(t.is_contiguous() for t in dgrad + wgrad) if mx else
                     all(t.stride(1) == 1 for t in dgrad[:2] + wgrad[:2]))
        if ops.grouped_gemm_ok(((M, K, N), (N, K, M))) and layout_ok:
            dx = torch.empty((M, K), dtype=torch.bfloat16, device=g8.device)
            dw = dw_out if dw_out is not None else torch.empty((N, K), dtype=torch.bfloat16, device=g8.device)
            probs = [dgrad + (dx,), wgrad + (dw,)]
            cfg = ops.grouped_gemm_choice(probs, fmt_b, fmt_f, mx=mx)  # cached per shape set: -1 = two launches are faster here
            if cfg >= 0:
                (ops.gemm_mxfp8_grouped if mx else ops.gemm_fp8_grouped)(probs, fmt_b, fmt_f, tile_cfg=cfg)
                return dx, dw
    gemm = ops.gemm_mxfp8 if mx else ops.gemm_fp8
    dx = gemm(*dgrad, fmt_b, fmt_f) if need_dgrad else None
    dw = gemm(*wgrad, fmt_b, fmt_f, out=dw_out) if need_wgrad else None
    return dx, dw


def _skip_2d(dskip: Optional[torch.Tensor], like: torch.Tensor) -> Optional[torch.Tensor]:
    """Residual-branch gradient as a contiguous bf16 [tokens, features] matrix for mi_rmsnorm_bwd's `dres`."""
    if dskip is None:
        return None
    d = dskip.reshape(like.shape)
    return d if (d.dtype == torch.bfloat16 and d.is_contiguous()) else d.to(torch.bfloat16).contiguous()


class LinearPlan(NamedTuple):
    """What one FP8 Linear node computes and keeps, decided once from which of its inputs need a gradient."""
    dgrad: bool     # the dX GEMM (and the RMSNorm backward of a fused norm): the input or the norm weight needs a gradient
    wgrad: bool     # the dW GEMM: any weight part needs one
    dbias: bool     # column sums of grad_output
    x_col: bool     # forward keeps the column-wise copy of the input (wgrad's operand)
    w_col: bool     # forward makes and keeps the column-wise copy of the weight (dgrad's operand)


def linear_plan(need_x: bool, need_bias: bool, need_ln: bool, need_w: bool) -> LinearPlan:
    dgrad, wgrad = bool(need_x or need_ln), bool(need_w)
    return LinearPlan(dgrad, wgrad, bool(need_bias), x_col=wgrad, w_col=dgrad)


class MLPPlan(NamedTuple):
    """The same for the fused fc1 -> SwiGLU -> fc2 node.  `dact`: anything upstream of the activation needs a gradient, so the
    fc2 dgrad GEMM and dSwiGLU run; without it (only fc2's own parameters train) backward ends at fc2."""
    dgrad: bool     # fc1's dX GEMM (+ RMSNorm backward)
    w1: bool        # fc1's dW GEMM
    b1: bool
    w2: bool        # fc2's dW GEMM
    b2: bool
    dact: bool
    x_col: bool     # forward keeps: column-wise input (fc1 wgrad)
    w1_col: bool    # ... column-wise fc1 weight (fc1 dgrad)
    h: bool         # ... the fc1 output (dSwiGLU)
    a_col: bool     # ... column-wise activation (fc2 wgrad)
    w2_col: bool    # ... column-wise fc2 weight (fc2 dgrad)


def mlp_plan(need_x: bool, need_w1: bool, need_b1: bool, need_w2: bool, need_b2: bool, need_ln: bool) -> MLPPlan:
    dgrad, w1, b1, w2, b2 = bool(need_x or need_ln), bool(need_w1), bool(need_b1), bool(need_w2), bool(need_b2)
    dact = dgrad or w1 or b1
    return MLPPlan(dgrad, w1, b1, w2, b2, dact, x_col=w1, w1_col=dgrad, h=dact, a_col=w2, w2_col=dact)


def grad_copies(need_row: bool, need_col: bool, colsum: bool) -> Optional[Tuple[bool, bool]]:
    """(row-wise, column-wise): the FP8 copies of a grad_output to ask its quantiser for -- `need_row` for the dgrad GEMM, `need_col`
    for the wgrad GEMM, `colsum` when a bias gradient rides on the pass.  None: nothing to do.  No cast kernel has a form that
    writes neither copy (they refuse it), so column sums alone ride on the row-wise one: the bias gradient stays the fixed-order
    sum it is on every other pattern, and the site's amax is published as always."""
    if need_row or need_col:
        return need_row, need_col
    return (True, False) if colsum else None


def _claim_bwd_update(ctx, spec: _GemmSpec) -> None:
    """The first GEMM Function of the outermost autocast region THAT WILL HAVE A BACKWARD carries the delayed-scaling backward
    update: every later Function consumes (part of) its output, so its backward is the region's last.  A Function none of whose
    inputs needs a gradient (a frozen module fed by a frozen embedding) has no backward and leaves the claim to the next."""
    if any(ctx.needs_input_grad):
        spec.trigger_bwd_update = FP8GlobalStateManager.is_first_fp8_module()


def _quantize_input(ctx, spec: _GemmSpec, x2, ln_w, want_t: bool, need_dgrad: bool):
    """The input of GEMM spec.g as an FP8 operand.  `ln_w` (with spec.eps): K9 -- x2 is the UN-normalised input and RMSNorm is
    fused into its quantisation; ctx.norm keeps what the RMSNorm backward needs."""
    ctx.norm = None
    if ln_w is None:
        return spec.q.quantize(x2, spec.g, want_t)
    gam = (ln_w if ln_w.dtype == torch.bfloat16 else ln_w.to(torch.bfloat16)).contiguous()
    # spec.rstd: the statistics came with the input (residual_add_stats)
    rstd = spec.rstd if spec.rstd is not None else ops.rmsnorm_stats(x2, spec.eps)
    if need_dgrad:
        ctx.norm = (x2, rstd, gam, ln_w.dtype)
    return spec.q.quantize(x2, spec.g, want_t, (rstd, gam))


def _finish_dx(ctx, dx, dskip, colsums=None):
    """The end of a GEMM Function's backward: RMSNorm backward of a fused norm with the residual-branch gradient added in the
    kernel, the update trigger, dx in the input's shape and dtype, `dskip` added where no kernel took it.
    `colsums`: the caller's bias gradients as (partial column sums, dtype) or None each -- ONE launch finishes them together
    with the RMSNorm weight gradient.  Returns (dx, dln, finished colsums)."""
    dln = None
    if ctx.norm is not None and dx is not None:
        xin, rstd, gam, ln_dtype = ctx.norm
        ctx.norm = None
        dx, dln = ops.rmsnorm_bwd(dx, xin, rstd, gam, dres=_skip_2d(dskip, dx), dgamma_dtype=ln_dtype, finish=colsums is None)
        dskip = None
        if colsums is not None:
            dln = (dln, ln_dtype)
    if colsums is not None:
        pend = [t for t in (*colsums, dln) if t is not None]
        if pend:
            done = iter(ops.colsum_finish_multi(pend))
            colsums = [None if t is None else next(done) for t in colsums]
            dln = None if dln is None else next(done)
    if ctx.spec.trigger_bwd_update:
        # this is the first GEMM Function of the outermost autocast that has a backward (_claim_bwd_update): its backward is the last
        FP8GlobalStateManager.reduce_and_update_fp8_tensors(forward=False)
    if dx is not None:
        dx = dx.view(ctx.x_shape).to(ctx.x_dtype)
    if dskip is not None:
        dx = dskip if dx is None else dx + dskip
    return dx, dln, colsums


class _FP8LinearFn(torch.autograd.Function):
    """y[M, sum N_i] = x[M,K] . cat(W_i)[N,K]^T (+ bias), FP8 operands, bf16 result."""

    @staticmethod
    def forward(ctx, x: torch.Tensor, bias: Optional[torch.Tensor], spec: _GemmSpec, ln_w: Optional[torch.Tensor],
                *weights: torch.Tensor):
        """`ln_w`: see _quantize_input."""
        x2 = _as_bf16_2d(x)
        M, K = x2.shape
        if M % 8 or K % 16:
            raise RuntimeError(f"FP8 Linear needs tokens % 8 == 0 and in_features % 16 == 0, got {M} x {K}")
        ns = [w.shape[0] for w in weights]
        N = sum(ns)
        q, g = spec.q, spec.g
        # (forward runs in no-grad mode; needs_input_grad is all-False when grad was disabled at apply time)
        nig = ctx.needs_input_grad
        plan = linear_plan(nig[0], nig[1], nig[3], any(nig[4:]))
        need_dgrad, need_wgrad = plan.dgrad, plan.wgrad
        _claim_bwd_update(ctx, spec)
        x8 = _quantize_input(ctx, spec, x2, ln_w, plan.x_col, need_dgrad)
        w8 = _weight_operand(spec, g, weights, ns, N, K, x2.device, plan.w_col)
        y = q.gemm(x8[0], w8[0], None if bias is None else bias.to(torch.bfloat16).contiguous())
        ctx.saved_fp8 = (x8[1], w8[1])
        if spec.dy_handoff is not None and bias is None and (need_wgrad or need_dgrad):
            q.offer(spec.dy_handoff, g, need_dgrad, need_wgrad)
        ctx.spec, ctx.ns, ctx.x_shape, ctx.x_dtype = spec, ns, x.shape, x.dtype
        ctx.w_dtypes = [w.dtype for w in weights]
        ctx.w_refs = weights if need_wgrad else None  # the Parameters themselves (not saved tensors): for _wgrad_out
        ctx.bias_dtype = None if bias is None else bias.dtype
        ctx.plan = plan
        if spec.with_skip:
            ctx.set_materialize_grads(False)
            return y.view(*x.shape[:-1], N), x
        return y.view(*x.shape[:-1], N)

    @staticmethod
    def backward(ctx, dy: torch.Tensor, dskip: Optional[torch.Tensor] = None):
        spec = ctx.spec
        q, g = spec.q, spec.g
        g2 = _as_bf16_2d(dy)
        x_col, w_col = ctx.saved_fp8
        ctx.saved_fp8 = None
        plan = ctx.plan
        db, dx, dw = None, None, None
        ride = plan.dbias and (q.colsum_dtypes is None or ctx.bias_dtype in q.colsum_dtypes)  # the bias gradient rides on the cast
        copies = grad_copies(plan.dgrad, plan.wgrad, ride)
        if spec.dy_handoff is not None and spec.dy_handoff.fp8 is not None:
            grad = q.taken(spec.dy_handoff.take(dy), g)  # already quantised by the op that produced it (dy is a placeholder)
        elif copies is None:
            grad = None                                  # only a bias gradient no quantiser pass can carry is wanted
        else:
            grad = q.quantize_grad(g2, g, *copies, colsum=ride)
            if ride:
                db = ops.colsum_finish(grad[2], ctx.bias_dtype)
        if plan.dgrad or plan.wgrad:
            dx, dw = _grouped_or_two(q, grad, w_col, x_col, _wgrad_out(ctx.w_refs, x_col[0].shape[0]) if plan.wgrad else None,
                                     plan.dgrad, plan.wgrad)
        if plan.dbias and db is None:
            db = g2.sum(0, dtype=torch.float32).to(ctx.bias_dtype)
        dx, dln, _ = _finish_dx(ctx, dx, dskip)
        dws: List[Optional[torch.Tensor]] = [None] * len(ctx.ns)
        if dw is not None:
            parts = torch.split(dw, ctx.ns, dim=0)
            dws = [p if p.dtype == dt else p.to(dt) for p, dt in zip(parts, ctx.w_dtypes)]
        return (dx, db, None, dln, *dws)


class _FP8SwiGLUMLPFn(torch.autograd.Function):
    """fc1 (FP8) -> SwiGLU fused with the FP8 quantisation of fc2's input -> fc2 (FP8): TE's LayerNormMLP structure
    (te_llama.py:58-63).  The bf16 activation is never materialised; backward fuses dSwiGLU with the quantisation of fc1's
    grad_output and returns the fc1 bias gradient from the same pass."""

    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2, spec: _GemmSpec, ln_w=None):
        x2 = _as_bf16_2d(x)
        M, K = x2.shape
        if M % 8 or K % 16:
            raise RuntimeError(f"FP8 LayerNormMLP needs tokens % 8 == 0 and hidden % 16 == 0, got {M} x {K}")
        q, dev = spec.q, x2.device
        nig = ctx.needs_input_grad
        # (the unfused route applies this Function without `ln_w`: needs_input_grad then has six entries)
        plan = mlp_plan(nig[0], nig[1], nig[2], nig[3], nig[4], len(nig) > 6 and nig[6])
        _claim_bwd_update(ctx, spec)
        x8 = _quantize_input(ctx, spec, x2, ln_w, plan.x_col, plan.dgrad)
        w1_8 = _weight_operand(spec, 0, (w1,), [w1.shape[0]], w1.shape[0], K, dev, plan.w1_col)
        # fc1: where the SwiGLU kernels take a bias the GEMM leaves it out and they add it (fp32) to the gate / up values they
        # unpack anyway; else it stays in the GEMM's epilogue
        b1_bf = None if b1 is None else b1.detach().to(torch.bfloat16).contiguous()
        fuse_b1 = b1_bf is not None and q.swiglu_adds_bias and _FUSE_MLP_BIAS and (b1_bf.data_ptr() % 16 == 0)
        h = q.gemm(x8[0], w1_8[0], None if fuse_b1 else b1_bf)
        a8 = q.swiglu(h, 1, plan.a_col, b1_bf if fuse_b1 else None)
        ctx.b1_fused = b1_bf if fuse_b1 else None
        w2_8 = _weight_operand(spec, 1, (w2,), [w2.shape[0]], w2.shape[0], w2.shape[1], dev, plan.w2_col)
        # fc2: with defer_bias the caller adds the bias in its residual add (LayerNormMLP.forward hands it over)
        y = q.gemm(a8[0], w2_8[0], None if (b2 is None or spec.defer_bias) else b2.to(torch.bfloat16).contiguous())
        ctx.saved_fp8 = (x8[1], w1_8[1], a8[1], w2_8[1], h if plan.h else None)
        ctx.spec, ctx.x_shape, ctx.x_dtype = spec, x.shape, x.dtype
        ctx.dtypes = (w1.dtype, None if b1 is None else b1.dtype, w2.dtype, None if b2 is None else b2.dtype)
        ctx.plan = plan
        ctx.w_refs = (w1, w2) if (plan.w1 or plan.w2) else None  # the Parameters themselves: for _wgrad_out
        if spec.with_skip:
            ctx.set_materialize_grads(False)
            return y.view(*x.shape[:-1], w2.shape[0]), x
        return y.view(*x.shape[:-1], w2.shape[0])

    @staticmethod
    def backward(ctx, dy, dskip=None):
        q = ctx.spec.q
        x_col, w1_col, a_col, w2_col, h = ctx.saved_fp8
        ctx.saved_fp8 = None
        dt_w1, dt_b1, dt_w2, dt_b2 = ctx.dtypes
        plan = ctx.plan
        db1 = db2 = dact = dw2 = dx = dw1 = None
        # fc2 backward (GEMM 1); its bias gradient rides on the quantisation of dy
        grad = q.quantize_grad(_as_bf16_2d(dy), 1, *grad_copies(plan.dact, plan.w2, plan.b2), colsum=plan.b2)
        if plan.b2:
            db2 = (grad[2], dt_b2)  # partial sums: finished with the layer's other column sums in _finish_dx
        if plan.dact or plan.w2:
            dact, dw2 = _grouped_or_two(q, grad, w2_col, a_col, _wgrad_out(ctx.w_refs[1:], a_col[0].shape[0]) if plan.w2 else None,
                                        plan.dact, plan.w2)
        if plan.dact:
            # dSwiGLU + quantisation of fc1's grad_output (GEMM 0) + fc1 bias gradient
            grad = q.dswiglu(h, dact, 0, *grad_copies(plan.dgrad, plan.w1, plan.b1), plan.b1, ctx.b1_fused)
            if plan.b1:
                db1 = (grad[2], dt_b1)
            if plan.dgrad or plan.w1:
                dx, dw1 = _grouped_or_two(q, grad, w1_col, x_col, _wgrad_out(ctx.w_refs[:1], x_col[0].shape[0]) if plan.w1 else None,
                                          plan.dgrad, plan.w1)
        dx, dln, (db1, db2) = _finish_dx(ctx, dx, dskip, (db1, db2))
        if dw1 is not None and dw1.dtype != dt_w1:
            dw1 = dw1.to(dt_w1)
        if dw2 is not None and dw2.dtype != dt_w2:
            dw2 = dw2.to(dt_w2)
        return dx, dw1, db1, dw2, db2, None, dln


class _FP8Module(torch.nn.Module):
    """Shared FP8 bookkeeping: lazily allocated meta windows, `_extra_state` (TE serialises its FP8
    metadata there; it ends up in `save_pretrained`, train_fp8.py:668-669)."""

    num_gemms = 1

    def __init__(self):
        super().__init__()
        self._meta_fwd: Optional[ModuleMeta] = None
        self._meta_bwd: Optional[ModuleMeta] = None
        self._meta_key = None
        self._pending_state = None
        self._wcache = {}  # FP8 weights kept across micro-batches (is_first_microbatch protocol)
        # used when forward() is called without `is_first_microbatch` (the decoder layer does not thread the flag through):
        # the training harness sets it per micro-batch of a gradient-accumulation window (train.train_step)
        self.default_is_first_microbatch = None

    def _spec(self, st, is_first_microbatch, g: int = 0, eps: float = 1e-5, **kw) -> _GemmSpec:
        """The spec of this module's GEMM `g` from what _prepare returned.  (Which Function carries the backward update trigger is
        settled in its forward: _claim_bwd_update.)"""
        recipe, mf, mb = st
        if is_first_microbatch is None:
            is_first_microbatch = self.default_is_first_microbatch
        return _GemmSpec(recipe, mf, mb, g, False, self.training, eps, self._wcache, is_first_microbatch, **kw)

    def _norm(self, x):  # (the modules with a norm in front)
        if self.normalization == "RMSNorm":
            return _rmsnorm(x, self.layer_norm_weight, self.eps, self.zero_centered_gamma)
        return _layernorm(x, self.layer_norm_weight, self.layer_norm_bias, self.eps, self.zero_centered_gamma)

    def _prepare(self, device) -> Optional[Tuple[Recipe, Optional[ModuleMeta], Optional[ModuleMeta]]]:
        """Called at the top of forward.  None -> run the plain bf16 path."""
        if not FP8GlobalStateManager.is_fp8_enabled():
            return None
        recipe = FP8GlobalStateManager.get_fp8_recipe()
        if recipe.mxfp8() or recipe.current() or recipe.block():  # no state: no meta windows, no arenas, an empty _extra_state
            return recipe, None, None
        key = (recipe.fp8_format, recipe.amax_history_len, recipe.amax_compute_algo, recipe.margin, str(device))
        if self._meta_key != key:
            if self._pending_state is not None:  # before any slot is taken: a refused state leaves the arenas and this module as they were
                for d in ("fwd", "bwd"):
                    ModuleMeta.check_history(self._pending_state[d], recipe.amax_history_len)
            fa = FP8GlobalStateManager.arena(recipe, True, device)
            ba = FP8GlobalStateManager.arena(recipe, False, device)
            self._meta_fwd = ModuleMeta(fa, fa.alloc(3 * self.num_gemms), 3 * self.num_gemms)
            self._meta_bwd = ModuleMeta(ba, ba.alloc(2 * self.num_gemms), 2 * self.num_gemms)
            self._meta_key = key
            if self._pending_state is not None:
                self._meta_fwd.load_state(self._pending_state["fwd"])
                self._meta_bwd.load_state(self._pending_state["bwd"])
                self._pending_state = None
        else:  # arenas may carry a new group / reduce flag
            FP8GlobalStateManager.arena(recipe, True, device)
            FP8GlobalStateManager.arena(recipe, False, device)
        return recipe, self._meta_fwd, self._meta_bwd

    def get_extra_state(self):
        to_cpu = lambda d: {k: v.cpu() for k, v in d.items()}
        if self._meta_fwd is not None:
            st = {"fwd": to_cpu(self._meta_fwd.state()), "bwd": to_cpu(self._meta_bwd.state())}
        elif self._pending_state is not None:
            # loaded, no FP8 forward yet (the meta windows do not exist): a save now must carry what was loaded, not drop it
            st = {"fwd": to_cpu(self._pending_state["fwd"]), "bwd": to_cpu(self._pending_state["bwd"])}
        else:
            return torch.empty(0, dtype=torch.uint8)
        buf = io.BytesIO()
        torch.save(st, buf)
        return torch.frombuffer(bytearray(buf.getvalue()), dtype=torch.uint8)

    def set_extra_state(self, state):
        if state is None or (isinstance(state, torch.Tensor) and state.numel() == 0):
            return
        st = torch.load(io.BytesIO(state.cpu().numpy().tobytes()), weights_only=True)
        if self._meta_fwd is not None:
            self._meta_fwd.load_state(st["fwd"])
            self._meta_bwd.load_state(st["bwd"])
        else:
            self._pending_state = st


def _rmsnorm(x: torch.Tensor, weight: torch.Tensor, eps: float, zero_centered_gamma: bool = False) -> torch.Tensor:
    w = weight + 1 if zero_centered_gamma else weight
    return F.rms_norm(x, (x.shape[-1],), w, eps)


def _layernorm(x, weight, bias, eps, zero_centered_gamma=False):
    w = weight + 1 if zero_centered_gamma else weight
    return F.layer_norm(x, (x.shape[-1],), w, bias, eps)


class RMSNorm(torch.nn.Module):
    def __init__(self, hidden_size: int, eps: float = 1e-5, params_dtype=None, device="cuda", zero_centered_gamma=False):
        super().__init__()
        self.eps, self.zero_centered_gamma = eps, zero_centered_gamma
        self.weight = torch.nn.Parameter(torch.ones(hidden_size, dtype=params_dtype or torch.get_default_dtype(), device=device))

    def forward(self, x):
        return _rmsnorm(x, self.weight, self.eps, self.zero_centered_gamma)


class LayerNorm(torch.nn.Module):
    """Present for `isinstance` checks in accelerate (utils/transformer_engine.py:109) and as a plain LN."""

    def __init__(self, hidden_size: int, eps: float = 1e-5, params_dtype=None, device="cuda", zero_centered_gamma=False):
        super().__init__()
        self.eps, self.zero_centered_gamma = eps, zero_centered_gamma
        dt = params_dtype or torch.get_default_dtype()
        self.weight = torch.nn.Parameter(torch.ones(hidden_size, dtype=dt, device=device))
        self.bias = torch.nn.Parameter(torch.zeros(hidden_size, dtype=dt, device=device))

    def forward(self, x):
        return _layernorm(x, self.weight, self.bias, self.eps, self.zero_centered_gamma)


def _init_weight(shape, dtype, device, init_method=None):
    w = torch.empty(shape, dtype=dtype, device=device)
    if init_method is not None:
        init_method(w)
    else:
        torch.nn.init.normal_(w, mean=0.0, std=0.023)  # TE default init_method_normal(0.023)
    return torch.nn.Parameter(w)


class Linear(_FP8Module):
    """Drop-in for `te.pytorch.Linear(in_features, out_features, bias=..., params_dtype=...)`."""

    def __init__(self, in_features: int, out_features: int, bias: bool = True, params_dtype=None, device="cuda",
                 init_method=None, **_ignored):
        super().__init__()
        self.in_features, self.out_features = in_features, out_features
        dt = params_dtype or torch.get_default_dtype()
        self.weight = _init_weight((out_features, in_features), dt, device, init_method)
        self.bias = torch.nn.Parameter(torch.zeros(out_features, dtype=dt, device=device)) if bias else None
        self.use_bias = bias

    def forward(self, inp: torch.Tensor, is_first_microbatch=None) -> torch.Tensor:
        st = self._prepare(inp.device)
        if st is None:
            if getattr(self, "_pending_norm", None) is not None:
                raise RuntimeError("Linear: a deferred RMSNorm is pending but FP8 is off for this forward")
            return F.linear(inp, _master(self.weight).to(inp.dtype), None if self.bias is None else self.bias.to(inp.dtype))
        # `offer_dy_handoff` (set on the lm_head by train.prepare_model): the output carries a DyHandoff through which the op
        # that consumes it directly (loss.causal_lm_loss) can deliver this layer's grad_output already quantised
        handoff = DyHandoff() if (getattr(self, "offer_dy_handoff", False) and self.training and torch.is_grad_enabled()
                                  and self.bias is None) else None
        # `_pending_norm` (llama._DeferredFinalNorm, the causal-LM head only): the RMSNorm in front of this Linear handed its
        # weight over instead of running, and is fused into the input cast as in LayerNormLinear (K9)
        pn, self._pending_norm = getattr(self, "_pending_norm", None), None
        ln_w, eps, rstd = None, 1e-5, None
        if pn is not None:
            ln_w, eps, rs, ptr, shape = pn
            if inp.data_ptr() != ptr or tuple(inp.shape) != shape:
                raise RuntimeError("Linear: a deferred RMSNorm is pending for another tensor than the one this forward received")
            rstd = _usable_rstd(rs, inp, eps)
        y = _FP8LinearFn.apply(inp, self.bias, self._spec(st, is_first_microbatch, eps=eps, rstd=rstd, dy_handoff=handoff), ln_w,
                               self.weight)
        if handoff is not None and handoff.offered():
            y._mi_dy_handoff = handoff
        return y

    def extra_repr(self):
        return f"in_features={self.in_features}, out_features={self.out_features}, bias={self.use_bias}"


class LayerNormLinear(_FP8Module):
    """Norm -> FP8 Linear.  With `parameters_split` the weight is kept as separate Parameters
    (`query_weight`, `key_weight`, `value_weight`, te_llama.py:200-217) that form ONE GEMM operand and
    share ONE weight amax/scale slot (SURVEY.md Appendix A "Fused-QKV")."""

    def __init__(self, in_features: int, out_features: int, eps: float = 1e-5, bias: bool = True,
                 normalization: str = "LayerNorm", parameters_split=None, params_dtype=None, device="cuda",
                 zero_centered_gamma: bool = False, init_method=None, return_layernorm_output: bool = False, **_ignored):
        super().__init__()
        assert normalization in ("LayerNorm", "RMSNorm")
        self.in_features, self.out_features, self.eps = in_features, out_features, eps
        self.normalization, self.zero_centered_gamma = normalization, zero_centered_gamma
        self.return_layernorm_output = return_layernorm_output
        dt = params_dtype or torch.get_default_dtype()
        self.layer_norm_weight = torch.nn.Parameter(
            torch.zeros(in_features, dtype=dt, device=device) if zero_centered_gamma else torch.ones(in_features, dtype=dt, device=device))
        self.layer_norm_bias = (torch.nn.Parameter(torch.zeros(in_features, dtype=dt, device=device))
                                if normalization == "LayerNorm" else None)
        if parameters_split is None:
            self.weight_names, sizes = ["weight"], [out_features]
            self.bias_names = ["bias"]
        else:
            if isinstance(parameters_split, dict):
                names, sizes = list(parameters_split.keys()), list(parameters_split.values())
            else:
                names = list(parameters_split)
                assert out_features % len(names) == 0
                sizes = [out_features // len(names)] * len(names)
            assert sum(sizes) == out_features
            self.weight_names = [f"{n.rstrip('_')}_weight" for n in names]
            self.bias_names = [f"{n.rstrip('_')}_bias" for n in names]
        self.split_sizes = sizes
        for n, sz in zip(self.weight_names, sizes):
            setattr(self, n, _init_weight((sz, in_features), dt, device, init_method))
        self.use_bias = bias
        for n, sz in zip(self.bias_names, sizes):
            if bias:
                setattr(self, n, torch.nn.Parameter(torch.zeros(sz, dtype=dt, device=device)))
            else:
                setattr(self, n, None)

    def _weights(self):
        return [getattr(self, n) for n in self.weight_names]

    def _bias(self):
        if not self.use_bias:
            return None
        bs = [getattr(self, n) for n in self.bias_names]
        return bs[0] if len(bs) == 1 else torch.cat(bs, 0)

    def forward(self, inp: torch.Tensor, is_first_microbatch=None, _with_skip: bool = False, _rstd=None, _dy_handoff=None):
        """`_with_skip` (extension used by MultiheadAttention / the decoder layer): returns (out, skip) where `skip` carries
        `inp` for the residual add, its gradient fused into the RMSNorm backward when the fused-norm path is active.
        `_rstd`: (rstd, eps) of `inp` from residual_add_stats, used instead of a statistics pass when eps matches."""
        st = self._prepare(inp.device)
        ws, b = self._weights(), self._bias()
        if st is not None and _can_fuse_norm(self, st[0], inp) and not self.return_layernorm_output:
            return _FP8LinearFn.apply(inp, b, self._spec(st, is_first_microbatch, eps=self.eps, with_skip=_with_skip,
                                                         rstd=_usable_rstd(_rstd, inp, self.eps), dy_handoff=_dy_handoff),
                                      self.layer_norm_weight, *ws)
        ln = self._norm(inp)
        if st is None:
            w = _master(ws[0]) if len(ws) == 1 else torch.cat([_master(w_) for w_ in ws], 0)
            out = F.linear(ln, w.to(ln.dtype), None if b is None else b.to(ln.dtype))
        else:
            out = _FP8LinearFn.apply(ln, b, self._spec(st, is_first_microbatch), None, *ws)
        if _with_skip:  # unfused route: the residual is the input itself (autograd adds its gradient)
            return out, inp
        return (out, ln) if self.return_layernorm_output else out


def _usable_rstd(handoff, inp: torch.Tensor, eps: float):
    """rstd from a (rstd, eps) hand-off if it belongs to `inp` (row count) and was computed with this module's eps."""
    if handoff is None:
        return None
    rstd, e = handoff
    if rstd is None or e != eps or rstd.numel() != inp.numel() // inp.shape[-1] or rstd.device != inp.device:
        return None
    return rstd


def _can_fuse_norm(mod, recipe, inp) -> bool:
    """K9 applies to RMSNorm (every recipe); the backward kernel keeps a whole row per wave (cols % 512, <= 8192)."""
    h = inp.shape[-1]
    return (getattr(mod, "fused_norm", True) and mod.normalization == "RMSNorm" and not mod.zero_centered_gamma
            and (recipe.delayed() or recipe.mxfp8() or recipe.current() or recipe.block()) and h % 512 == 0 and h // 512 in (1, 2, 3, 4, 5, 6, 7, 8, 10, 12, 14, 16))


def _swiglu(a: torch.Tensor) -> torch.Tensor:
    f = a.shape[-1] // 2
    return F.silu(a[..., :f]) * a[..., f:]


_ACTS = {
    "swiglu": (_swiglu, 2), "gelu": (lambda a: F.gelu(a, approximate="tanh"), 1), "relu": (F.relu, 1),
    "geglu": (lambda a: F.gelu(a[..., :a.shape[-1] // 2], approximate="tanh") * a[..., a.shape[-1] // 2:], 2),
    "silu": (F.silu, 1),
}


class LayerNormMLP(_FP8Module):
    """Norm -> fc1 (FP8) -> activation -> fc2 (FP8); parameters `layer_norm_weight`, `fc1_weight`
    [gate|up stacked: 2*ffn, hidden], `fc1_bias`, `fc2_weight`, `fc2_bias` (te_llama.py:58-63,219-238).
    `bias=True` is TE's default and the reference does not override it."""

    num_gemms = 2

    def __init__(self, hidden_size: int, ffn_hidden_size: int, eps: float = 1e-5, bias: bool = True,
                 normalization: str = "LayerNorm", activation: str = "gelu", params_dtype=None, device="cuda",
                 zero_centered_gamma: bool = False, init_method=None, output_layer_init_method=None, **_ignored):
        super().__init__()
        assert normalization in ("LayerNorm", "RMSNorm") and activation in _ACTS
        self.hidden_size, self.ffn_hidden_size, self.eps = hidden_size, ffn_hidden_size, eps
        self.normalization, self.activation, self.zero_centered_gamma = normalization, activation, zero_centered_gamma
        self.act_fn, mult = _ACTS[activation]
        dt = params_dtype or torch.get_default_dtype()
        self.layer_norm_weight = torch.nn.Parameter(
            torch.zeros(hidden_size, dtype=dt, device=device) if zero_centered_gamma else torch.ones(hidden_size, dtype=dt, device=device))
        self.layer_norm_bias = (torch.nn.Parameter(torch.zeros(hidden_size, dtype=dt, device=device))
                                if normalization == "LayerNorm" else None)
        self.fc1_weight = _init_weight((mult * ffn_hidden_size, hidden_size), dt, device, init_method)
        self.fc2_weight = _init_weight((hidden_size, ffn_hidden_size), dt, device, output_layer_init_method or init_method)
        self.use_bias = bias
        self.fc1_bias = torch.nn.Parameter(torch.zeros(mult * ffn_hidden_size, dtype=dt, device=device)) if bias else None
        self.fc2_bias = torch.nn.Parameter(torch.zeros(hidden_size, dtype=dt, device=device)) if bias else None
        self.fused_swiglu = True  # K10: SwiGLU fused with the FP8 cast (delayed scaling); False -> two Linears + torch ops

    def forward(self, inp: torch.Tensor, is_first_microbatch=None, _with_skip: bool = False, _rstd=None, _defer_bias: bool = False):
        """`_defer_bias` (extension, with `_with_skip`): returns (out, skip, bias) where `out` lacks the fc2 bias and `bias` is the
        tensor the caller must add (residual_add_stats(skip, out, eps, bias=bias)), or None when nothing was deferred."""
        st = self._prepare(inp.device)
        if (st is not None and self.activation == "swiglu" and self.fused_swiglu and _can_fuse_norm(self, st[0], inp)):
            # K9 + K10: norm -> cast, fc1, SwiGLU -> cast, fc2 in one autograd node
            # (the residual add that takes the deferred fc2 bias is recipe-independent: MXFP8 defers too; the fc1 bias stays in the
            # MXFP8 GEMM's epilogue, its quantising SwiGLU kernels have no bias form)
            defer = bool(_defer_bias and _with_skip and _FUSE_MLP_BIAS and self.fc2_bias is not None)
            res = _FP8SwiGLUMLPFn.apply(inp, self.fc1_weight, self.fc1_bias, self.fc2_weight, self.fc2_bias,
                                        self._spec(st, is_first_microbatch, eps=self.eps, with_skip=_with_skip,
                                                   rstd=_usable_rstd(_rstd, inp, self.eps), defer_bias=defer),
                                        self.layer_norm_weight)
            if _defer_bias and _with_skip:
                return res[0], res[1], (self.fc2_bias if defer else None)
            return res
        out = self._unfused(inp, st, is_first_microbatch)
        if _defer_bias and _with_skip:
            return out, inp, None
        return (out, inp) if _with_skip else out  # unfused route: the residual is the input itself

    def _unfused(self, inp, st, is_first_microbatch):
        ln = self._norm(inp)
        if st is None:
            h = F.linear(ln, _master(self.fc1_weight).to(ln.dtype), None if self.fc1_bias is None else self.fc1_bias.to(ln.dtype))
            return F.linear(self.act_fn(h), _master(self.fc2_weight).to(ln.dtype),
                            None if self.fc2_bias is None else self.fc2_bias.to(ln.dtype))
        recipe = st[0]
        if self.activation == "swiglu" and self.fused_swiglu and (not (recipe.mxfp8() or recipe.block()) or inp.numel() // inp.shape[-1] % 32 == 0):
            return _FP8SwiGLUMLPFn.apply(ln, self.fc1_weight, self.fc1_bias, self.fc2_weight, self.fc2_bias,
                                         self._spec(st, is_first_microbatch))
        h = _FP8LinearFn.apply(ln, self.fc1_bias, self._spec(st, is_first_microbatch), None, self.fc1_weight)
        return _FP8LinearFn.apply(self.act_fn(h), self.fc2_bias, self._spec(st, is_first_microbatch, 1), None, self.fc2_weight)
