"""FP8 recipes -- same names, fields and defaults as `transformer_engine.common.recipe`, which the
reference imports at te_llama.py:25, te_llama_hybrid.py:25, te_llama_mxfp8.py:25 and accelerate
builds at utils/transformer_engine.py:156-177."""
from __future__ import annotations

from dataclasses import dataclass, field
from enum import Enum
from typing import Callable, NamedTuple, Optional, Tuple, Union


class _FormatHelper(NamedTuple):
    max_fwd: float
    max_bwd: float


class Format(Enum):
    """E4M3: all tensors E4M3.  E5M2: all E5M2.  HYBRID: forward tensors E4M3, gradients E5M2."""
    E4M3 = _FormatHelper(max_fwd=448.0, max_bwd=448.0)
    E5M2 = _FormatHelper(max_fwd=57344.0, max_bwd=57344.0)
    HYBRID = _FormatHelper(max_fwd=448.0, max_bwd=57344.0)


class Recipe:
    def mxfp8(self) -> bool:
        return isinstance(self, MXFP8BlockScaling)

    def delayed(self) -> bool:
        return isinstance(self, DelayedScaling)

    def current(self) -> bool:
        return isinstance(self, Float8CurrentScaling)

    def block(self) -> bool:
        return isinstance(self, Float8BlockScaling)


@dataclass(frozen=True)
class DelayedScaling(Recipe):
    """Per-tensor delayed scaling (te_llama.py:39-40: history 16, algo "max"; accelerate default:
    HYBRID, history 1024, "most_recent")."""
    margin: int = 0
    fp8_format: Format = Format.HYBRID
    amax_history_len: int = 1024
    amax_compute_algo: Union[str, Callable] = "max"
    scaling_factor_compute_algo: Optional[Callable] = None
    reduce_amax: bool = True
    fp8_dpa: bool = False
    fp8_mha: bool = False
    interval: int = 1  # deprecated in TE, accepted for accelerate's TERecipeKwargs
    override_linear_precision: Tuple[bool, bool, bool] = (False, False, False)

    def __post_init__(self):
        assert self.fp8_format in (Format.E4M3, Format.E5M2, Format.HYBRID)
        if self.amax_compute_algo not in ("max", "most_recent"):
            raise ValueError("amax_compute_algo must be 'max' or 'most_recent' (callables are not supported)")
        if self.scaling_factor_compute_algo is not None:
            raise ValueError("custom scaling_factor_compute_algo is not supported")
        if self.amax_history_len < 1 or self.amax_history_len > 4096:
            raise ValueError("amax_history_len must be in [1, 4096]")
        if self.override_linear_precision != (False, False, False):
            raise ValueError("override_linear_precision is not supported")


@dataclass(frozen=True)
class MXFP8BlockScaling(Recipe):
    """OCP MX block scaling: one E8M0 scale per 32 elements along the contraction axis, no history
    (te_llama_mxfp8.py:28-29)."""
    margin: int = 0
    fp8_format: Format = Format.E4M3
    fp8_dpa: bool = False
    fp8_mha: bool = False

    def __post_init__(self):
        assert self.fp8_format in (Format.E4M3, Format.E5M2, Format.HYBRID)
        if self.margin != 0:
            raise ValueError("MXFP8BlockScaling margin must be 0")


@dataclass(frozen=True)
class QParams:
    """How one class of tensors is quantised under Float8CurrentScaling (TE's QParams)."""
    power_2_scale: bool = False
    amax_epsilon: float = 0.0


@dataclass(frozen=True)
class MMParams:
    """TE's MMParams.  Accepted and ignored: the FP8 GEMM here has one accumulation order."""
    use_split_accumulator: bool = True


@dataclass(frozen=True)
class Float8CurrentScaling(Recipe):
    """Per-tensor scaling from the live amax: every tensor is quantised with scale = fp8_max / amax of that very tensor, no history
    (TE's Float8CurrentScaling: same fields and defaults)."""
    fp8_format: Format = Format.HYBRID
    fp8_quant_fwd_inp: QParams = QParams(power_2_scale=False, amax_epsilon=0.0)
    fp8_quant_fwd_weight: QParams = QParams(power_2_scale=False, amax_epsilon=0.0)
    fp8_quant_bwd_grad: QParams = QParams(power_2_scale=False, amax_epsilon=0.0)
    fp8_gemm_fprop: MMParams = MMParams(use_split_accumulator=False)
    fp8_gemm_dgrad: MMParams = MMParams(use_split_accumulator=True)
    fp8_gemm_wgrad: MMParams = MMParams(use_split_accumulator=True)
    fp8_dpa: bool = False
    fp8_mha: bool = False

    def __post_init__(self):
        assert self.fp8_format in (Format.E4M3, Format.E5M2, Format.HYBRID)
        for q in (self.fp8_quant_fwd_inp, self.fp8_quant_fwd_weight, self.fp8_quant_bwd_grad):
            if not (q.amax_epsilon >= 0.0):
                raise ValueError("amax_epsilon must be non-negative")


@dataclass(frozen=True)
class Float8BlockScaling(Recipe):
    """Block scaling with power-of-two scales, no history (the DeepSeek-V3 style recipe): one scale per 1 x 128 block along the
    contraction axis for activations and gradients (scaling dim 1), one per 128 x 128 block for weights (scaling dim 2).
    Field names and defaults are those of TE's Float8BlockScaling as far as its public definition is known here; TE itself is not
    available to compare against, so parity with it is unpinned, as for the other recipes.
    Only power-of-two scales: the gfx950 scaled MFMA applies E8M0 (power-of-two) scales, which a power-of-two scale inverse is
    exactly; fp32 block scales would need a different GEMM main loop."""
    fp8_format: Format = Format.E4M3
    fp8_quant_fwd_inp: QParams = QParams(power_2_scale=True, amax_epsilon=0.0)
    fp8_quant_fwd_weight: QParams = QParams(power_2_scale=True, amax_epsilon=0.0)
    fp8_quant_bwd_grad: QParams = QParams(power_2_scale=True, amax_epsilon=0.0)
    x_block_scaling_dim: int = 1
    w_block_scaling_dim: int = 2
    grad_block_scaling_dim: int = 1
    fp8_gemm_fprop: MMParams = MMParams(use_split_accumulator=True)
    fp8_gemm_dgrad: MMParams = MMParams(use_split_accumulator=True)
    fp8_gemm_wgrad: MMParams = MMParams(use_split_accumulator=True)
    fp8_dpa: bool = False
    fp8_mha: bool = False

    def __post_init__(self):
        if self.fp8_format not in (Format.E4M3, Format.E5M2, Format.HYBRID):
            raise ValueError("fp8_format must be Format.E4M3, Format.E5M2 or Format.HYBRID")
        x, w, g = self.x_block_scaling_dim, self.w_block_scaling_dim, self.grad_block_scaling_dim
        for name, d in (("x_block_scaling_dim", x), ("w_block_scaling_dim", w), ("grad_block_scaling_dim", g)):
            if d not in (1, 2):
                raise ValueError(f"{name} must be 1 (1x128 blocks) or 2 (128x128 blocks), got {d!r}")
        if x == 2 and w == 2:
            raise ValueError("2D by 2D block scaling is not supported: x_block_scaling_dim and w_block_scaling_dim cannot both be 2")
        if w == 2 and g == 2:
            raise ValueError("2D by 2D block scaling is not supported: w_block_scaling_dim and grad_block_scaling_dim cannot both be 2")
        for q in (self.fp8_quant_fwd_inp, self.fp8_quant_fwd_weight, self.fp8_quant_bwd_grad):
            if not (q.amax_epsilon >= 0.0):
                raise ValueError("amax_epsilon must be non-negative")
            if not q.power_2_scale:
                raise ValueError("Float8BlockScaling needs power_2_scale=True: the gfx950 scaled MFMA applies E8M0 (power-of-two) "
                                 "block scales; fp32 block scales would need a different GEMM main loop")


def fmt_codes(fmt: Format) -> Tuple[int, int]:
    """(forward code, backward code) for the C ABI: 0 = E4M3, 1 = E5M2."""
    fwd = 1 if fmt is Format.E5M2 else 0
    bwd = 0 if fmt is Format.E4M3 else 1
    return fwd, bwd
