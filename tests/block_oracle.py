"""numpy restatement of the Float8BlockScaling arithmetic (include/mi_fp8.h, mi_blockfp8_*), built on oracle/fp8_oracle.py:

  block amax   max |v| over 128 consecutive elements of a row (dim 1; the column-wise copy: of a column) or over a 128 x 128 tile
               (dim 2), fmaxf semantics (NaN ignored, Inf gives Inf); a trailing short block covers the elements that exist
  scale        a = max(amax, eps); 1 when a is 0 or Inf, else fl32(fp8_max / a) with Inf -> FLT_MAX, mantissa cleared
  scale byte   254 - biased_exponent(scale): the E8M0 code of 1 / scale, stored at every 32-group position the block covers
  data byte    fp8_encode_sat(fl32(v * scale))

Outputs come in the device's layout: y_row [R, C], s_row [C/32, R], y_colT [C, R], s_colT [R/32, C].  Also the inputs and caps that
the fused front-end tests share between the CPU cap check and the GPU run."""
import numpy as np
import torch

from oracle import fp8_oracle as O

BLOCK = 128
REL_BAND = 2.0 ** -17   # the band of O.fp8_mismatches_near_boundary, also used for the scale quotient
FUSED_SHAPES = [(32, 512), (160, 1024), (1024, 3072)]


def scale_quotient(amax, fmt: int, eps: float = 0.0) -> np.ndarray:
    """fl32(fp8_max / max(amax, eps)), Inf where the divisor is 0 (the rule then takes 1), as float32."""
    a = np.maximum(np.asarray(amax, dtype=np.float32), np.float32(eps))
    with np.errstate(divide="ignore", over="ignore", invalid="ignore"):
        return (O.FP8_MAX[fmt] / a).astype(np.float32)


def scale_from_amax(amax, fmt: int, eps: float = 0.0) -> np.ndarray:
    """TE's compute_scale_from_amax with power-of-two forcing, float32."""
    a = np.maximum(np.asarray(amax, dtype=np.float32), np.float32(eps))
    q = scale_quotient(amax, fmt, eps)
    q = np.where(np.isinf(q), np.float32(O.FLT_MAX), q)
    q = np.where((a == 0) | np.isinf(a), np.float32(1.0), q).astype(np.float32)
    return (np.ascontiguousarray(q).view(np.uint32) & np.uint32(0xFF800000)).view(np.float32).reshape(q.shape)


def scale_byte(scale) -> np.ndarray:
    s = np.ascontiguousarray(scale, dtype=np.float32)
    return (254 - ((s.view(np.uint32) >> 23) & 0xFF).astype(np.int64)).astype(np.uint8).reshape(s.shape)


def _block_amax(v: np.ndarray, bh: int, bw: int) -> np.ndarray:
    """[R, C] -> [ceil(R/bh), ceil(C/bw)]: fmaxf-style maximum of |v| per block; short trailing blocks are padded with 0."""
    ab = np.abs(np.asarray(v, dtype=np.float32))
    ab = np.where(np.isnan(ab), np.float32(0), ab)
    R, C = ab.shape
    nr, nc = -(-R // bh), -(-C // bw)
    pad = np.zeros((nr * bh, nc * bw), np.float32)
    pad[:R, :C] = ab
    return pad.reshape(nr, bh, nc, bw).max(axis=(1, 3)).astype(np.float32)


def element_scales(v: np.ndarray, fmt: int, bh: int, bw: int, eps: float = 0.0):
    """(scale per element [R, C] float32, block amax, block scale) for blocks of bh x bw."""
    R, C = v.shape
    amax = _block_amax(v, bh, bw)
    sc = scale_from_amax(amax, fmt, eps)
    return np.repeat(np.repeat(sc, bh, axis=0), bw, axis=1)[:R, :C], amax, sc


def _quant(v: np.ndarray, S: np.ndarray, fmt: int):
    with np.errstate(over="ignore", invalid="ignore"):
        y = O.fp8_encode_sat((v * S).astype(np.float32), fmt)
    return y, np.ascontiguousarray(scale_byte(S)[:, ::32].T)   # block-major: [C/32, R]


def quantize_values(v32: np.ndarray, fmt: int, dim: int, eps: float = 0.0):
    """(y_row, s_row, y_colT, s_colT) of the float32 values `v32` [R, C] (R, C multiples of 32)."""
    v = np.ascontiguousarray(v32, dtype=np.float32)
    assert v.ndim == 2 and v.shape[0] % 32 == 0 and v.shape[1] % 32 == 0 and dim in (1, 2)
    vt = np.ascontiguousarray(v.T)
    if dim == 1:
        y_row, s_row = _quant(v, element_scales(v, fmt, 1, BLOCK, eps)[0], fmt)
        y_colT, s_colT = _quant(vt, element_scales(vt, fmt, 1, BLOCK, eps)[0], fmt)
    else:
        S = element_scales(v, fmt, BLOCK, BLOCK, eps)[0]
        y_row, s_row = _quant(v, S, fmt)
        y_colT, s_colT = _quant(vt, np.ascontiguousarray(S.T), fmt)
    return y_row, s_row, y_colT, s_colT


def quantize(x_bf16_bits: np.ndarray, fmt: int, dim: int, eps: float = 0.0):
    return quantize_values(O.bf16_bits_to_f32(x_bf16_bits), fmt, dim, eps)


def dequantize(y: np.ndarray, s_block_major: np.ndarray, fmt: int) -> np.ndarray:
    """float64 values of an operand (y [R, K], s [K/32, R])."""
    inv = np.repeat(O.e8m0_to_f32(s_block_major.T).astype(np.float64), 32, axis=1)
    return O.fp8_decode(y, fmt).astype(np.float64) * inv


def gemm(a, b, fmt_a: int, fmt_b: int, out_f32: bool = True):
    """O.gemm_mxfp8_tn on operands in the device layout: (y [M, K], s [K/32, M]) x (y [N, K], s [K/32, N])."""
    return O.gemm_mxfp8_tn(a[0], np.ascontiguousarray(a[1].T), b[0], np.ascontiguousarray(b[1].T), fmt_a, fmt_b, out_f32=out_f32)


def quotient_near_pow2(q) -> np.ndarray:
    """Mask: the (finite, positive) scale quotient lies within REL_BAND (relative) of a power of two, where a value a few float32
    ulps away may be rounded down to the neighbouring power of two."""
    q = np.asarray(q, dtype=np.float64)
    live = np.isfinite(q) & (q > 0)
    p2 = np.exp2(np.round(np.log2(np.where(live, q, 1.0))))
    return live & (np.abs(q / p2 - 1.0) <= REL_BAND)


def linear_fwd_bwd(x_bits, w_bits, dy_bits, fmt_f: int, fmt_b: int, bias_bits=None):
    """One te.Linear under Float8BlockScaling() (x and dy: 1 x 128 blocks, w: 128 x 128): (y, dx, dw) float32 before the bf16
    rounding of the output, and the weight's two operand copies."""
    x8 = quantize(x_bits, fmt_f, 1)
    w8 = quantize(w_bits, fmt_f, 2)
    g8 = quantize(dy_bits, fmt_b, 1)
    y = gemm(x8[:2], w8[:2], fmt_f, fmt_f).astype(np.float64)
    if bias_bits is not None:
        y = y + O.bf16_bits_to_f32(bias_bits).astype(np.float64)[None, :]
    dx = gemm(g8[:2], w8[2:], fmt_b, fmt_f)
    dw = gemm(g8[2:], x8[2:], fmt_b, fmt_f)
    return y.astype(np.float32), dx, dw, w8


# ---- the fused front ends: inputs (the recipe of test_mxfp8_fused_front_ends_vs_oracle) and caps shared by the CPU cap check and
# the GPU test ----
def fused_inputs(shape):
    R, C = shape
    g = torch.Generator().manual_seed(R + 3 * C)
    x = (torch.randn(R, C, generator=g) * torch.exp(torch.randn(R, 1, generator=g))).to(torch.bfloat16)
    gamma = (torch.rand(C, generator=g) + 0.5).to(torch.bfloat16)
    h = (torch.randn(R, 2 * C, generator=g) * 2).to(torch.bfloat16)
    d = (torch.randn(R, C, generator=g) / 8).to(torch.bfloat16)
    return x, gamma, h, d


def dswiglu_slack(h_bits, d_bits) -> np.ndarray:
    """The dsilu cancellation slack of the existing dSwiGLU tests: 2^-21 |d u| on the gate half, none on the up half."""
    hf, df = O.bf16_bits_to_f32(h_bits), O.bf16_bits_to_f32(d_bits)
    F = df.shape[1]
    return np.concatenate([np.abs(df * hf[:, F:]) * 2.0 ** -21, np.zeros_like(df)], axis=1).astype(np.float32)


def scale_cap(n_blocks: int) -> int:
    return int(max(2, 1e-4 * n_blocks))


def byte_cap(size: int) -> int:
    return int(max(2, 1e-3 * size))


def orientations(v32, dim: int, slack=None):
    """The two copies of a tensor as (values [r, c], block height, block width, slack) with blocks along the last axis for dim 1."""
    v = np.ascontiguousarray(v32, dtype=np.float32)
    st = None if slack is None else np.ascontiguousarray(slack.T)
    bh = 1 if dim == 1 else BLOCK
    return (("row", v, bh, BLOCK, slack), ("col", np.ascontiguousarray(v.T), bh, BLOCK, st))


def fused_views(v32, dim: int, slack=None):
    """What the fused front-end criterion looks at: both copies under dim 1; under dim 2 the row-wise copy only (the column-wise
    one is its byte transpose under the same scales, which the test checks by identity)."""
    views = orientations(v32, dim, slack)
    return views if dim == 1 else views[:1]


def band_counts(v32, fmt: int, dim: int, slack=None):
    """[(name, blocks, blocks whose scale quotient is near a power of two, size, values inside the byte band)] of the reference."""
    from tests.util import fp8_in_boundary_band
    out = []
    for name, mat, bh, bw, slk in fused_views(v32, dim, slack):
        S, amax, _ = element_scales(mat, fmt, bh, bw)
        near = quotient_near_pow2(scale_quotient(amax, fmt))
        with np.errstate(over="ignore", invalid="ignore"):
            vs = (mat * S).astype(np.float32)
        band = fp8_in_boundary_band(vs, fmt, REL_BAND, None if slk is None else slk * S)
        out.append((name, amax.size, int(near.sum()), mat.size, int(band.sum())))
    return out


def check_fused(got, v32, fmt: int, dim: int, name: str, exact: bool, slack=None):
    """The criterion of test_mxfp8_fused_front_ends_vs_oracle for block scales.  `got` = the device's (y_row, s_row, y_colT, s_colT)
    as numpy arrays; `v32` the float32 restatement in the device's operation order.  exact: scales and bytes identical.  Else a
    block scale may differ by one step, only where the scale quotient is within 2^-17 of a power of two, at most scale_cap of
    them; with the DEVICE's scale every differing byte must be explained by O.fp8_mismatches_near_boundary, at most byte_cap.
    Returns the figures [(view, scale mismatches, byte mismatches)]."""
    figures = []
    pairs = {"row": (got[0], got[1]), "col": (got[2], got[3])}
    for view, mat, bh, bw, slk in fused_views(v32, dim, slack):
        data, s_bm = pairs[view]
        r, c = mat.shape
        S, amax, sc = element_scales(mat, fmt, bh, bw)
        got_b = np.ascontiguousarray(s_bm.T)                       # [r, c/32]
        want_b = scale_byte(S)[:, ::32]
        # the device stores ONE byte per block: every 32-group of a block holds the same one
        grp = BLOCK // 32
        ri, ci = (np.arange(r) // bh) * bh, (np.arange(c // 32) // grp) * grp   # a block's first row / first 32-group
        assert np.array_equal(got_b, got_b[np.ix_(ri, ci)]), f"{name} {view}: the 32-groups of a block hold different scale bytes"
        mism = got_b != want_b
        if exact:
            assert not mism.any(), f"{name} {view}: {mism.sum()} scale bytes differ from the float32 restatement"
        else:
            blk_mism = mism[::bh, ::grp]                          # one entry per block
            q = scale_quotient(amax, fmt)
            step = np.abs(got_b.astype(np.int32) - want_b.astype(np.int32))[::bh, ::grp]
            assert (step[blk_mism] == 1).all(), f"{name} {view}: a block scale differs by more than one step"
            assert quotient_near_pow2(q)[blk_mism].all(), f"{name} {view}: a block scale differs away from a power-of-two boundary"
            assert blk_mism.sum() <= scale_cap(blk_mism.size), f"{name} {view}: {blk_mism.sum()} of {blk_mism.size} block scales differ"
        S_dev = np.repeat(np.ldexp(np.float32(1.0), 127 - got_b.astype(np.int64)).astype(np.float32), 32, axis=1)  # the DEVICE's scale
        with np.errstate(over="ignore", invalid="ignore"):
            vs = (mat * S_dev).astype(np.float32)
        if exact:
            np.testing.assert_array_equal(data, O.fp8_encode_sat(vs, fmt), err_msg=f"{name} {view}")
            n_mis = 0
        else:
            n_mis, n_bad = O.fp8_mismatches_near_boundary(data, vs, fmt, abs_slack=None if slk is None else slk * S_dev)
            assert n_bad == 0, f"{name} {view}: {n_bad} of {n_mis} mismatching bytes are NOT within 2^-17 of a rounding boundary"
            assert n_mis <= byte_cap(data.size), f"{name} {view}: {n_mis} of {data.size} bytes differ"
        figures.append((view, int(mism[::bh, ::grp].sum()), int(n_mis)))
    return figures
