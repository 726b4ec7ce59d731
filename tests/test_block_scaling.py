"""CPU: Float8BlockScaling as far as no GPU is needed -- the recipe, its refusals and TE field names; the numpy restatement of the
arithmetic (tests/block_oracle.py) against hand-worked values; the recipe's `q` object at a GEMM site; the wrappers' refusal;
revision 3 of ABI 5 and the host refusals of the four entry points; and the cap check of the fused front-end GPU test."""
import dataclasses
import os
import re

import numpy as np
import pytest
import torch

from oracle import fp8_oracle as O
from tests import block_oracle as B
from tests.util import bf16_bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mi_blockfp8_quantize_ex", "mi_blockfp8_norm_quantize", "mi_blockfp8_swiglu_quantize", "mi_blockfp8_dswiglu_quantize")
FAKE = 0x10000  # non-null, 128-byte aligned; every call below is refused before anything is dereferenced or launched


# ------------------------------------------------------------------------------------------------------------ recipe
def test_recipe_fields_defaults_and_predicates():
    from llm_fp8_amd.common import recipe as R
    r = R.Float8BlockScaling()
    assert isinstance(r, R.Recipe)
    assert r.block() and not r.delayed() and not r.mxfp8() and not r.current()
    assert not R.DelayedScaling().block() and not R.MXFP8BlockScaling().block() and not R.Float8CurrentScaling().block()
    assert r.fp8_format is R.Format.E4M3 and r.fp8_dpa is False and r.fp8_mha is False
    for name in ("fp8_quant_fwd_inp", "fp8_quant_fwd_weight", "fp8_quant_bwd_grad"):
        q = getattr(r, name)
        assert isinstance(q, R.QParams) and q.power_2_scale is True and q.amax_epsilon == 0.0, name
    for name in ("fp8_gemm_fprop", "fp8_gemm_dgrad", "fp8_gemm_wgrad"):
        assert getattr(r, name) == R.MMParams(use_split_accumulator=True), name
    assert (r.x_block_scaling_dim, r.w_block_scaling_dim, r.grad_block_scaling_dim) == (1, 2, 1)
    assert [f.name for f in dataclasses.fields(r)] == [
        "fp8_format", "fp8_quant_fwd_inp", "fp8_quant_fwd_weight", "fp8_quant_bwd_grad", "x_block_scaling_dim",
        "w_block_scaling_dim", "grad_block_scaling_dim", "fp8_gemm_fprop", "fp8_gemm_dgrad", "fp8_gemm_wgrad", "fp8_dpa", "fp8_mha"]
    assert R.fmt_codes(r.fp8_format) == (0, 0)
    assert R.fmt_codes(R.Float8BlockScaling(fp8_format=R.Format.HYBRID).fp8_format) == (0, 1)
    assert R.fmt_codes(R.Float8BlockScaling(fp8_format=R.Format.E5M2).fp8_format) == (1, 1)
    assert "unpinned" in R.Float8BlockScaling.__doc__


def test_recipe_refusals():
    from llm_fp8_amd.common import recipe as R
    p2 = R.QParams(power_2_scale=True, amax_epsilon=0.0)
    with pytest.raises(ValueError, match="fp8_format"):
        R.Float8BlockScaling(fp8_format="E4M3")
    for name in ("x_block_scaling_dim", "w_block_scaling_dim", "grad_block_scaling_dim"):
        for bad in (0, 3, None):
            with pytest.raises(ValueError, match=name):
                R.Float8BlockScaling(**{name: bad})
    with pytest.raises(ValueError, match="x_block_scaling_dim and w_block_scaling_dim cannot both be 2"):
        R.Float8BlockScaling(x_block_scaling_dim=2, w_block_scaling_dim=2)
    with pytest.raises(ValueError, match="w_block_scaling_dim and grad_block_scaling_dim cannot both be 2"):
        R.Float8BlockScaling(grad_block_scaling_dim=2)
    for name in ("fp8_quant_fwd_inp", "fp8_quant_fwd_weight", "fp8_quant_bwd_grad"):
        with pytest.raises(ValueError, match="amax_epsilon"):
            R.Float8BlockScaling(**{name: R.QParams(power_2_scale=True, amax_epsilon=-1.0)})
        with pytest.raises(ValueError, match=r"power_2_scale=True.*E8M0.*fp32 block scales would need a different GEMM main loop"):
            R.Float8BlockScaling(**{name: R.QParams(power_2_scale=False)})
    # what is allowed: 1D everywhere, 2D activations against 1D weights, an epsilon
    R.Float8BlockScaling(w_block_scaling_dim=1)
    R.Float8BlockScaling(x_block_scaling_dim=2, w_block_scaling_dim=1, grad_block_scaling_dim=2)
    assert R.Float8BlockScaling(fp8_quant_fwd_inp=dataclasses.replace(p2, amax_epsilon=2.0 ** -10)).fp8_quant_fwd_inp.amax_epsilon == 2.0 ** -10


# ------------------------------------------------------------------------------------------------------------ oracle self-checks
def test_scale_rule_on_hand_picked_amax_values():
    f32 = np.float32
    flt_min, flt_max = f32(2.0 ** -126), np.finfo(np.float32).max
    # (amax, scale, byte) for E4M3 (448 = 1.75 * 2^8), worked out by hand:
    #   0, Inf            -> the rule's 1                                         -> byte 127
    #   448               -> 448 / 448 = 1                                        -> 127
    #   448 (1 + 2^-23)   -> quotient just below 1: in [1/2, 1), cleared to 1/2   -> 128
    #   448 (1 - 2^-23)   -> quotient just above 1: cleared to 1                  -> 127
    #   FLT_MIN, 1e-38    -> 1.75 * 2^134 overflows: FLT_MAX, cleared to 2^127    -> 0
    #   FLT_MAX           -> 1.75 * 2^8 / (2 - 2^-23) 2^127 = 1.75 (1 + ..) 2^-120 -> 2^-120 -> 247
    cases = [(f32(0), 1.0, 127), (f32(np.inf), 1.0, 127), (f32(448), 1.0, 127), (f32(448 * (1 + 2.0 ** -23)), 0.5, 128),
             (f32(448 * (1 - 2.0 ** -23)), 1.0, 127), (flt_min, 2.0 ** 127, 0), (f32(1e-38), 2.0 ** 127, 0), (flt_max, 2.0 ** -120, 247)]
    assert f32(448 * (1 + 2.0 ** -23)) > f32(448) > f32(448 * (1 - 2.0 ** -23))
    for amax, scale, byte in cases:
        s = B.scale_from_amax(np.array([amax]), O.E4M3)
        assert s[0] == f32(scale) and B.scale_byte(s)[0] == byte, (amax, s, B.scale_byte(s))
        assert np.ldexp(1.0, int(byte) - 127) * float(s[0]) == 1.0          # the byte decodes to 1 / scale exactly
    # E5M2 (57344 = 1.75 * 2^15): FLT_MAX -> 1.75 (1 + ..) 2^-113 -> 2^-113 -> byte 240; 57344 -> 1
    s = B.scale_from_amax(np.array([flt_max, f32(57344), f32(1.0)]), O.E5M2)
    assert list(s) == [f32(2.0 ** -113), f32(1.0), f32(2.0 ** 15)] and list(B.scale_byte(s)) == [240, 127, 112]
    # epsilon: a floor under the amax, not under the scale
    assert B.scale_from_amax(np.array([f32(0), f32(1e-6), f32(3.0)]), O.E4M3, eps=2.0 ** -10).tolist() == [2.0 ** 18, 2.0 ** 18, 2.0 ** 7]


def test_scale_byte_range_and_exact_inverse():
    rng = np.random.default_rng(3)
    bits = (rng.integers(0, 0xFF, 200000).astype(np.uint32) << 23) | rng.integers(0, 1 << 23, 200000).astype(np.uint32)
    edge = np.array([0, 1, 0x007FFFFF, 0x00800000, 0x7F7FFFFF, 0x7F800000, 0x43E00000], np.uint32)   # 0, subnormals, FLT_MIN, FLT_MAX, Inf, 448
    amax = np.concatenate([bits, edge]).view(np.float32)
    for fmt in (O.E4M3, O.E5M2):
        s = B.scale_from_amax(amax, fmt)
        b = B.scale_byte(s).astype(np.int64)
        assert b.min() >= 0 and b.max() <= 247 and (b != 0xFF).all()
        assert (s.view(np.uint32) & 0x007FFFFF == 0).all() and (s > 0).all() and np.isfinite(s).all()
        assert (np.ldexp(1.0, b - 127) * s.astype(np.float64) == 1.0).all()
        live = (amax > 0) & np.isfinite(amax)
        with np.errstate(over="ignore"):
            scaled = amax[live].astype(np.float64) * s[live]
        # rounded DOWN to a power of two: the block's amax lands in (fp8_max / 2, fp8_max] -- up to the quotient's own rounding --
        # unless the scale was capped at 2^127
        capped = s[live] == np.float32(2.0 ** 127)
        assert (scaled <= float(O.FP8_MAX[fmt]) * (1 + 2.0 ** -23)).all()
        assert (scaled[~capped] > float(O.FP8_MAX[fmt]) / 2 * (1 - 2.0 ** -23)).all()


def _operand(shape, seed, spread=3.0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(shape, generator=g) * torch.exp(torch.randn(shape[0], 1, generator=g) * spread)
    return bf16_bits(x.to(torch.bfloat16))


@pytest.mark.parametrize("fa,fb", [(O.E4M3, O.E4M3), (O.E5M2, O.E4M3)])
def test_quantise_gemm_round_trip_with_replicated_scales(fa, fb):
    """quantise -> O.gemm_mxfp8_tn on the replicated scale bytes == float64 matmul of the dequantised operands, and the
    dequantised operands are the inputs to FP8 precision (no block saturates: its amax lands at or below fp8_max)."""
    M, N, K = 160, 224, 416   # trailing short blocks in every direction
    a_bits, b_bits = _operand((M, K), 1), _operand((N, K), 2, spread=1.0)
    a, b = B.quantize(a_bits, fa, 1), B.quantize(b_bits, fb, 2)
    d = B.gemm(a[:2], b[:2], fa, fb)
    da, db = B.dequantize(a[0], a[1], fa), B.dequantize(b[0], b[1], fb)
    np.testing.assert_array_equal(d, (da @ db.T).astype(np.float32))
    for bits, deq, fmt, q in ((a_bits, da, fa, a), (b_bits, db, fb, b)):
        v = O.bf16_bits_to_f32(bits).astype(np.float64)
        mbits, emin = (3, -6) if fmt == O.E4M3 else (2, -14)
        inv = np.repeat(O.e8m0_to_f32(q[1].T).astype(np.float64), 32, axis=1)     # 1 / scale per element
        # half an ulp of a normal code, or half a subnormal step, in the block's scale
        assert (np.abs(deq - v) <= 2.0 ** -(mbits + 1) * np.abs(v) + 2.0 ** (emin - mbits - 1) * inv).all()
    # the column-wise copies contract the other axis: wgrad-style product of the two transposed copies
    g = B.quantize(_operand((M, N), 3), fa, 1)
    dw = B.gemm(g[2:], a[2:], fa, fa)
    np.testing.assert_array_equal(dw, (B.dequantize(g[2], g[3], fa) @ B.dequantize(a[2], a[3], fa).T).astype(np.float32))


@pytest.mark.parametrize("shape", [(32, 32), (128, 128), (160, 224), (256, 384)])
@pytest.mark.parametrize("fmt", [O.E4M3, O.E5M2])
def test_layout_transposes_and_trailing_short_blocks(shape, fmt):
    R, C = shape
    bits = _operand(shape, R + C)
    v = O.bf16_bits_to_f32(bits)
    for dim in (1, 2):
        y_row, s_row, y_colT, s_colT = B.quantize(bits, fmt, dim)
        assert y_row.shape == (R, C) and s_row.shape == (C // 32, R) and y_colT.shape == (C, R) and s_colT.shape == (R // 32, C)
        for s in (s_row, s_colT):
            assert s.max() <= 247
    y_row, s_row, y_colT, s_colT = B.quantize(bits, fmt, 2)
    np.testing.assert_array_equal(y_colT, y_row.T)
    # one byte per 128 x 128 tile in both scale tensors, the same byte
    for i in range(R // 32):
        for j in range(C // 32):
            tile = s_row[(j // 4) * 4, (i // 4) * 128]
            assert (s_row[j, i * 32:(i + 1) * 32] == tile).all() and (s_colT[i, j * 32:(j + 1) * 32] == tile).all()
    # a trailing short block is a block over the elements that exist: recompute the last row block of row 0 by hand
    y1, s1, _, _ = B.quantize(bits, fmt, 1)
    c0 = (C - 1) // 128 * 128
    amax = np.abs(v[0, c0:]).max()
    sc = B.scale_from_amax(np.array([amax]), fmt)[0]
    assert (s1[c0 // 32:, 0] == B.scale_byte(np.array([sc]))[0]).all()
    np.testing.assert_array_equal(y1[0, c0:], O.fp8_encode_sat((v[0, c0:] * sc).astype(np.float32), fmt))


def test_non_finite_elements_follow_the_contract():
    x = np.zeros((32, 256), np.float32)
    x[0, 3] = np.nan                      # NaN inside an otherwise-zero block: ignored by the amax, NaN byte
    x[1, 5], x[1, 6] = np.inf, 2.0        # Inf: amax Inf -> scale 1; Inf saturates
    x[2, 130], x[2, 131] = np.nan, 3.0
    y, s, yt, st = B.quantize_values(x, O.E4M3, 1)
    assert y[0, 3] == O.FP8_NAN_BYTE and s[0, 0] == 127 and (y[0, :3] == 0).all()
    assert y[1, 5] == 0x7E and s[0, 1] == 127 and y[1, 6] == O.fp8_encode_sat(np.array([2.0], np.float32), O.E4M3)[0]
    assert y[2, 130] == O.FP8_NAN_BYTE and s[4, 2] == 127 - 7 and y[2, 131] == O.fp8_encode_sat(np.array([384.0], np.float32), O.E4M3)[0]
    assert yt[3, 0] == O.FP8_NAN_BYTE and yt[5, 1] == 0x7E


# ------------------------------------------------------------------------------------------------------------ module / wrappers
def test_gemm_spec_carries_a_block_q_and_prepare_builds_no_state():
    import llm_fp8_amd.pytorch as te
    from llm_fp8_amd.common.recipe import Float8BlockScaling, Format
    from llm_fp8_amd.pytorch import module as M
    from llm_fp8_amd.pytorch.fp8 import FP8GlobalStateManager
    r = Float8BlockScaling(fp8_format=Format.HYBRID)
    q = M._GemmSpec(r, None, None, 0, False, True).q
    assert type(q) is M._BlockQ and q.recipe is r and (q.fmt_f, q.fmt_b) == (0, 1)
    assert q.mx is True and q.swiglu_adds_bias is M._MXQ.swiglu_adds_bias and q.colsum_dtypes == M._MXQ.colsum_dtypes
    others = (M._DelayedQ, M._MXQ, M._CurrentQ)
    assert len({q.cache_key} | {c.cache_key for c in others}) == 4 and len({q.sink_key} | {c.sink_key for c in others}) == 4
    for name in ("quantize", "swiglu", "quantize_grad", "dswiglu", "offer", "taken", "operands", "gemm", "unflat", "quantize_weights",
                 "new_sink"):
        assert callable(getattr(q, name)) and all(callable(getattr(c, name)) for c in others), name
    assert q.operands.__func__ is M._MXQ.operands and q.gemm.__func__ is M._MXQ.gemm and q.unflat.__func__ is M._MXQ.unflat
    assert q.new_sink((), (), 256, 256, None, 0) is None and "Float8BlockScaling" in q.no_sink
    h = M.DyHandoff()
    q.offer(h, 0, True, True)
    assert not h.offered()
    FP8GlobalStateManager.reset()
    lin = te.Linear(32, 32, bias=False, params_dtype=torch.bfloat16, device="cpu")
    try:
        FP8GlobalStateManager.FP8_ENABLED, FP8GlobalStateManager.FP8_RECIPE = True, r
        st = lin._prepare(torch.device("cpu"))
        assert st[0] is r and st[1] is None and st[2] is None
        assert lin._meta_fwd is None and lin.get_extra_state().numel() == 0
        assert FP8GlobalStateManager._arenas == {}
    finally:
        FP8GlobalStateManager.reset()
    norm = te.LayerNormLinear(512, 512, normalization="RMSNorm", bias=False, params_dtype=torch.bfloat16, device="cpu")
    assert M._can_fuse_norm(norm, r, torch.empty(8, 512))


def test_scenario_block_through_llama_and_the_argument_parser():
    from llm_fp8_amd import llama, train
    from llm_fp8_amd.common.recipe import Float8BlockScaling
    attn, mlp = llama.scenario_recipes("block")
    assert isinstance(attn, Float8BlockScaling) and attn is mlp and attn == Float8BlockScaling()
    assert llama.outer_recipe_for_scenario("block") is attn
    assert llama.decoder_layer_cls("block").scenario == "block"
    cfg = train.config_from_args(train.build_arg_parser().parse_args(["--use_te", "--fp8_scenario", "block"]))
    assert cfg.fp8_scenario == "block" and cfg.use_te


class _Layer(torch.nn.Module):
    """What distributed.uses_block_scaling looks at on a decoder layer."""

    def __init__(self, scenario):
        super().__init__()
        from llm_fp8_amd import llama
        self.attn_recipe, self.mlp_recipe = llama.scenario_recipes(scenario)
        self.proj = torch.nn.Linear(64, 64).to(torch.bfloat16)


def test_sharded_fp8_dp_refuses_the_recipe_and_auto_avoids_it(tmp_path, monkeypatch):
    import torch.distributed as dist
    from llm_fp8_amd import distributed as D, llama, train
    blk, dflt, cur = (torch.nn.Sequential(_Layer(s)) for s in ("block", "default", "current"))
    assert D.uses_block_scaling(blk) and not D.uses_block_scaling(dflt) and not D.uses_block_scaling(cur)
    assert not D.uses_current_scaling(blk) and D.uses_current_scaling(cur)      # the sibling keeps its meaning
    outer = torch.nn.Sequential(torch.nn.Linear(8, 8))
    llama.apply_fp8_autowrap(outer, llama.outer_recipe_for_scenario("block"))
    assert D.uses_block_scaling(outer)
    dist.init_process_group("gloo", init_method=f"file://{tmp_path}/rdzv", rank=0, world_size=1)
    try:
        with pytest.raises(RuntimeError, match=r"Float8BlockScaling.*replicated"):
            D.ShardedFP8DP(blk)
        monkeypatch.setattr(D, "fits_replicated", lambda *a, **k: False)
        monkeypatch.setattr(dist, "get_world_size", lambda *a, **k: 2)
        assert train.resolve_sharding_mode("auto", dflt, torch.device("cpu")) == "fsdp_fp8"
        assert train.resolve_sharding_mode("auto", blk, torch.device("cpu")) == "fsdp_full"
        assert train.resolve_sharding_mode("auto", outer, torch.device("cpu")) == "fsdp_full"
        monkeypatch.setattr(D, "fits_replicated", lambda *a, **k: True)
        assert train.resolve_sharding_mode("auto", blk, torch.device("cpu")) == "replicated"
    finally:
        monkeypatch.undo()
        dist.destroy_process_group()


# ------------------------------------------------------------------------------------------------------------ ABI
def test_header_library_and_binding_agree_on_revision_3_and_the_four_entry_points():
    from llm_fp8_amd import _lib
    src = open(os.path.join(ROOT, "include", "mi_fp8.h")).read()
    lib = _lib.load()
    ver = int(re.search(r"#define\s+MI_ABI_VERSION\s+(\d+)", src).group(1))
    rev = int(re.search(r"#define\s+MI_ABI_REVISION\s+(\d+)", src).group(1))
    assert ver == lib.mi_abi_version() == _lib.ABI_VERSION
    assert rev == lib.mi_abi_revision() == _lib.ABI_REVISION >= 3
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in NEW:
        decl = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, code, flags=re.S)
        twin = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name.replace("blockfp8", "mxfp8"), code, flags=re.S)
        assert decl and twin, name
        assert hasattr(lib, name) and name in _lib.REVISION_SIGNATURES and getattr(lib, name).argtypes == _lib.SIGNATURES[name]
        args, targs = [a.strip() for a in decl.group(1).split(",")], [a.strip() for a in twin.group(1).split(",")]
        assert len(args) == len(_lib.SIGNATURES[name])
        assert args == targs[:-1] + ["int block_dim", "float amax_epsilon", "void* stream"], name   # the twin's list + the two


def test_host_refusals_before_any_launch():
    from llm_fp8_amd import _lib
    lib = _lib.load()
    err = lambda: lib.mi_last_error()
    calls = {
        "mi_blockfp8_quantize_ex": lambda x=FAKE, p=FAKE, dim=1, eps=0.0, rows=128, ld=128:
            lib.mi_blockfp8_quantize_ex(x, p, p, p, p, None, rows, 128, ld, 0, dim, eps, None),
        "mi_blockfp8_norm_quantize": lambda x=FAKE, p=FAKE, dim=1, eps=0.0:
            lib.mi_blockfp8_norm_quantize(x, FAKE, FAKE, p, p, p, p, 128, 128, 0, dim, eps, None),
        "mi_blockfp8_swiglu_quantize": lambda x=FAKE, p=FAKE, dim=1, eps=0.0:
            lib.mi_blockfp8_swiglu_quantize(x, p, p, p, p, 128, 128, 0, dim, eps, None),
        "mi_blockfp8_dswiglu_quantize": lambda x=FAKE, p=FAKE, dim=1, eps=0.0:
            lib.mi_blockfp8_dswiglu_quantize(x, FAKE, p, p, p, p, None, 128, 128, 0, dim, eps, None),
    }
    for name, call in calls.items():
        assert call(x=None) == -1 and name.encode() in err() and b"null input" in err(), name
        assert call(p=None) == -1 and name.encode() in err(), name
        assert call(dim=3) == -1 and name.encode() in err() and b"block_dim 3" in err(), name
        assert call(dim=0) == -1 and b"block_dim 0" in err(), name
        assert call(eps=-1.0) == -1 and b"amax_epsilon" in err(), name
    ex = calls["mi_blockfp8_quantize_ex"]
    assert ex(rows=100) == -1 and b"multiples of 32" in err()
    assert ex(ld=96) == -1 and b"ld_rows" in err()
    # a 128 x 128 block row-block destination 32 rows into its operand (the pointers that advance one byte per row)
    assert ex(p=FAKE + 32, dim=2, ld=256) == -1 and b"multiple of 128 rows" in err()
    assert lib.mi_blockfp8_norm_quantize(FAKE, None, FAKE, FAKE, FAKE, FAKE, FAKE, 128, 128, 0, 1, 0.0, None) == -1 and b"rstd" in err()
    assert lib.mi_blockfp8_dswiglu_quantize(FAKE, None, FAKE, FAKE, FAKE, FAKE, None, 128, 128, 0, 1, 0.0, None) == -1 and b"dact" in err()


def test_ops_refuse_cpu_tensors_and_bad_dims():
    from llm_fp8_amd.pytorch import ops
    x = torch.zeros((32, 64), dtype=torch.bfloat16)
    for call in (lambda: ops.blockfp8_quantize(x, 0, 1), lambda: ops.blockfp8_norm_quantize(x, torch.ones(32), x[0], 0, 1),
                 lambda: ops.blockfp8_swiglu_quantize(x, 0, 2), lambda: ops.blockfp8_dswiglu_quantize(x, x[:, :32], 0, 1)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    with pytest.raises(ValueError, match="1x128"):
        ops._blk_dim(3)


# ------------------------------------------------------------------------------------------------------------ cap check
@pytest.mark.parametrize("shape", B.FUSED_SHAPES)
def test_fused_front_end_references_stay_below_the_caps(shape):
    """The GPU test of the fused SwiGLU / dSwiGLU front ends allows a block scale or a byte to differ only inside a band of 2^-17
    around a power of two / a rounding boundary, and caps how many may.  On its inputs (same seeds and shapes), count the reference
    blocks and values INSIDE those bands: both must stay below the caps, or the caps could not tell a wrong kernel from an unlucky
    seed.  (A seed that exceeded a cap would be changed, never the cap.)"""
    _, _, h, d = B.fused_inputs(shape)
    hb, db = bf16_bits(h), bf16_bits(d)
    cases = (("swiglu", O.swiglu_f32_device_order(hb), None), ("dswiglu", O.dswiglu_f32_device_order(hb, db), B.dswiglu_slack(hb, db)))
    for name, v32, slack in cases:
        for dim in (1, 2):
            for view, blocks, near, size, band in B.band_counts(v32, O.E4M3, dim, slack):
                print(f"{name} {shape} dim {dim} {view}: {near} of {blocks} scale quotients near a power of two (cap {B.scale_cap(blocks)}), "
                      f"{band} of {size} values in the byte band (cap {B.byte_cap(size)})")
                assert near <= B.scale_cap(blocks), (name, dim, view, near, blocks)
                assert band <= B.byte_cap(size), (name, dim, view, band, size)
