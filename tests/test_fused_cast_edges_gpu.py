"""Exhaustive-gate and non-finite inputs for the fused FP8 emitters: mi_swiglu_cast(_bias), mi_dswiglu_cast(_bias), mi_norm_cast, their
MX twins (mi_mxfp8_swiglu_quantize, mi_mxfp8_dswiglu_quantize, mi_mxfp8_norm_quantize) and their current-scaling amax twins
(mi_amax_swiglu, mi_amax_dswiglu, mi_amax_norm).

The contract is the plain cast's (test_cast_exhaustive_all_bf16): bytes = O.fp8_encode_sat(value * scale) with NaN -> 0x7F and +-Inf /
over-range -> +-max code, amax = O.amax_f32 (NaN ignored, Inf gives Inf), MX block amax with the same fmaxf semantics
(O.mx_block_amax).  `value` is the float32 restatement in the device's operation order (oracle/fp8_oracle.py *_device_order).

Criteria.  No bound in this file is measured on the kernels:
  * identity wherever IEEE arithmetic alone decides the value (tests/util.py swiglu_sweep_reference: NaN, +-Inf, exact zero with its
    sign, sigmoid exactly 1 for g >= 17), and everywhere for the RMSNorm casts (no transcendental);
  * elsewhere the criteria of the benign-data tests in test_kernels_gpu.py: every byte that differs must be explained by
    O.fp8_mismatches_near_boundary (2^-17 relative, widened only by O.exp_arg_rel_band for |g| > 44 -- derivation there -- and the dsilu
    cancellation slack, never more than the existing one), at most max(2, 1e-3 size) of them; amax rtol 2e-6; column sums rtol 1e-4
    + 1e-4 max|column| sqrt(rows).
tests/test_oracle.py counts on the CPU how many reference values of these sweeps lie inside their band: fewer than the cap.

The inputs (tests/util.py): the gate half of h is the 256 x 256 tensor of all 65536 bf16 patterns ("full"), with Inf / NaN patterns
zeroed ("finite"), or with every |g| >= 2^64 zeroed as well ("bounded").  Under "finite" the largest gates times the tables' large
entries still overflow float32, so its amax is Inf like the full sweep's (asserted as such); the FINITE amax, the guarded atomicMax
and the planted NaN are checked on "bounded".

What these tests cannot tell apart: the `(v != v) ? 0 : |v|` in front of `fmaxf` in the fused kernels' amax (and amax_acc in
mi_current.hip) from a bare `fmaxf(amax, |v|)`.  The values are results of a multiply, so their NaNs are quiet, and fmaxf returns the
other operand for a quiet NaN: builds with either guard dropped pass this file (NaN bias column, planted NaN and all), whereas a
build without one of cvt4_fp8's 0x7F byte patches fails 33 of its 58 cases."""
import numpy as np
import pytest
import torch

from oracle import fp8_oracle as O
from tests import util as U
from tests.util import bits_to_bf16, u8

pytestmark = pytest.mark.gpu

FLT_MAX = float(np.finfo(np.float32).max)


@pytest.fixture(scope="module")
def ops(dev):
    from llm_fp8_amd.pytorch import ops as _ops
    from llm_fp8_amd import _lib
    assert _lib.load().mi_device_supported() == 1, "not a gfx950 device"
    return _ops


def _f32(v, dev):
    return torch.tensor([v], dtype=torch.float32, device=dev)


def _bits32(v) -> int:
    return int(np.asarray(v, dtype=np.float32).reshape(-1)[:1].view(np.uint32)[0])


def _dev_or_none(bits, dev):
    return None if bits is None else bits_to_bf16(bits, dev)


def _check_bytes(got, v_scaled, fmt, fixed, rel, slack, what):
    """identity at the `fixed` positions; every other differing byte explained by the rounding-boundary band; at most the cap of them"""
    want = O.fp8_encode_sat(v_scaled, fmt)
    bad = np.nonzero(fixed & (got != want))
    assert bad[0].size == 0, (f"{what}: {bad[0].size} bytes differ where IEEE arithmetic fixes the value; first at {bad[0][0], bad[1][0]}: "
                              f"value {v_scaled[bad][0]!r} got {got[bad][0]:#04x} want {want[bad][0]:#04x}")
    n_mis, n_bad = O.fp8_mismatches_near_boundary(got, v_scaled, fmt, rel=rel, abs_slack=slack)
    print(f"{what}: {n_mis} bytes differ from the restatement, {n_bad} unexplained")
    assert n_bad == 0, f"{what}: {n_bad} of {n_mis} mismatching bytes are NOT within their band of a rounding boundary"
    assert n_mis <= max(2, 1e-3 * got.size), f"{what}: {n_mis} of {got.size} bytes differ"


def _scaled(v32, scale):
    with np.errstate(over="ignore", invalid="ignore"):  # 3e38 * 16 overflows to Inf (-> max code); a signalling NaN operand
        return (v32 * np.float32(scale)).astype(np.float32)


def _run_swiglu(ops, dev, backward, h, d, bias, scale, amax, fmt, want_y=True, want_t=True):
    if backward:
        return ops.dswiglu_cast(h, d, _f32(scale, dev), amax, fmt, want_y=want_y, want_t=want_t, want_colsum=True, bias=bias)
    return (*ops.swiglu_cast(h, _f32(scale, dev), amax, fmt, want_y=want_y, want_t=want_t, bias=bias), None)


# ----------------------------------------------------------------------------------------- 2. SwiGLU / dSwiGLU, per-tensor
@pytest.mark.parametrize("bias_kind", ["none", "bias", "nan"])
@pytest.mark.parametrize("assign", [0, 1])
@pytest.mark.parametrize("fmt", [O.E4M3, O.E5M2])
@pytest.mark.parametrize("backward", [False, True], ids=["swiglu", "dswiglu"])
def test_swiglu_casts_on_the_exhaustive_gate_sweep(ops, dev, backward, fmt, assign, bias_kind):
    scale = U.DSWIGLU_SCALE if backward else U.SWIGLU_SCALE
    bias_bits = U.sweep_bias(bias_kind, assign)
    bias = _dev_or_none(bias_bits, dev)
    for kind in U.SWEEP_KINDS:
        what = f"{'dswiglu' if backward else 'swiglu'} fmt {fmt} assign {assign} bias {bias_kind} {kind}"
        h_bits, d_bits = U.gate_sweep(kind, assign)
        h, d = bits_to_bf16(h_bits, dev), bits_to_bf16(d_bits, dev)
        v32, fixed, rel, slack = U.swiglu_sweep_reference(h_bits, d_bits, bias_bits, backward, scale)
        amax = torch.zeros(1, dtype=torch.float32, device=dev)
        y, yT, cs = _run_swiglu(ops, dev, backward, h, d, bias, scale, amax, fmt)
        got = u8(y)
        _check_bytes(got, _scaled(v32, scale), fmt, fixed, rel, slack, what)
        np.testing.assert_array_equal(u8(yT), got.T)
        if bias_kind == "nan":  # the whole column of the NaN bias entry (both halves of the backward when it sits in the gate half)
            cols = [37, 37 + 256] if (backward and assign == 0) else [37]
            assert (got[:, cols] == O.FP8_NAN_BYTE).all(), f"{what}: a NaN bias entry must give 0x7F down its column"
        # amax: NaN ignored, Inf gives Inf
        a_ref = O.amax_f32(v32)
        print(f"{what}: amax {amax.item()!r} restatement {a_ref!r}")
        if kind == "bounded":
            assert np.isfinite(a_ref) and a_ref > 0
            np.testing.assert_allclose(amax.item(), a_ref, rtol=2e-6)
            # the guarded atomicMax: a non-zero slot below the result is raised to it, one above it is left alone
            assert 1.0 < a_ref < FLT_MAX / 2
            for start, expect in ((np.float32(1.0), amax.item()), (np.float32(2.0) * a_ref, np.float32(2.0) * a_ref)):
                slot = _f32(float(start), dev)
                _run_swiglu(ops, dev, backward, h, d, bias, scale, slot, fmt)
                assert _bits32(slot.item()) == _bits32(expect), f"{what}: amax slot started at {start!r}: {slot.item()!r}, expected {expect!r}"
        else:
            assert a_ref == np.inf and amax.item() == np.inf, f"{what}: amax {amax.item()!r}, restatement {a_ref!r}"
        if backward:  # fc1 bias gradient: per-128-row column sums
            with np.errstate(invalid="ignore", over="ignore"):
                ref = v32.astype(np.float64).sum(0)
                colmax = np.where(np.isfinite(v32), np.abs(v32), 0).max(0).astype(np.float64)
                ok = np.isfinite(ref) & (np.abs(ref) < FLT_MAX)
            got_cs = cs.sum(0).cpu().numpy().astype(np.float64)
            assert ok.any() and ((~ok).any() or kind != "full")
            assert not np.isfinite(got_cs[~ok]).any(), f"{what}: a column sum beyond float32 (or with a NaN / Inf term) came out finite"
            # the tolerance of test_dswiglu_cast_vs_oracle, with the column's own maximum in place of the tensor's (columns are
            # independent sums; the tensor's maximum, 1e38 here, would let every other column through)
            err = np.abs(got_cs[ok] - ref[ok])
            tol = 1e-4 * np.abs(ref[ok]) + 1e-4 * colmax[ok] * np.sqrt(256)
            assert (err <= tol).all(), f"{what}: column sums off by up to {(err / np.maximum(tol, 1e-300)).max():.3g} x the tolerance"
        if kind == "full":  # the y-only and yT-only instantiations: the same bytes and the same amax
            for want_y, want_t in ((True, False), (False, True)):
                a1 = torch.zeros(1, dtype=torch.float32, device=dev)
                y1, y1T, _ = _run_swiglu(ops, dev, backward, h, d, bias, scale, a1, fmt, want_y=want_y, want_t=want_t)
                assert (y1 is None) == (not want_y) and (y1T is None) == (not want_t)
                assert torch.equal(y1 if want_y else y1T, y if want_y else yT), f"{what}: single-output bytes differ"
                assert _bits32(a1.item()) == _bits32(amax.item())


# ----------------------------------------------------------------------------------------- 2. MX twins
def _check_mx(got, v32, fmt, name, exact, expect_inf, fixed=None, rel=None, abs_slack=None):
    """test_mxfp8_fused_front_ends_vs_oracle's criterion with fmaxf block amax: scales identical (`exact`) or one step apart next to
    a power-of-two boundary only; an Inf in the block -> E8M0 0xFE; bytes judged with the DEVICE's scale, both orientations."""
    y_row, s_row, y_colT, s_colT = got
    rcp = O._MAX_NORM_RCP[fmt]
    v32 = np.ascontiguousarray(v32, dtype=np.float32)
    tr = lambda a: None if a is None else np.ascontiguousarray(np.broadcast_to(a, v32.shape).T)
    for data, scales, mat, fx, rl, slk, ori in ((y_row, s_row, v32, fixed, rel, abs_slack, "row"),
                                                 (y_colT, s_colT, np.ascontiguousarray(v32.T), tr(fixed), tr(rel), tr(abs_slack), "col")):
        r, c = mat.shape
        blk = O.mx_block_amax(mat)
        with np.errstate(over="ignore"):
            want_e = O.float_to_e8m0_roundup((blk * rcp).astype(np.float32))
        got_e = u8(scales).T
        assert (got_e != 0xFF).all(), f"{name} {ori}: a NaN block scale (the block amax ignores NaN)"
        assert np.isinf(blk).any() == expect_inf
        assert (got_e[np.isinf(blk)] == 0xFE).all(), f"{name} {ori}: a block that holds an Inf must get E8M0 0xFE"
        mism = got_e != want_e
        print(f"{name} {ori}: {int(mism.sum())} of {mism.size} block scales differ")
        if exact:
            assert not mism.any(), f"{name} {ori}: {mism.sum()} block scales differ from the float32 restatement"
        else:
            # the band of the element that attains the block amax
            ab = np.abs(mat.reshape(r, c // 32, 32))
            arg = np.where(np.isnan(ab), np.float32(-1), ab).argmax(-1)
            rl_blk = np.take_along_axis(np.broadcast_to(rl, mat.shape).reshape(r, c // 32, 32), arg[..., None], -1)[..., 0]
            v = (blk * rcp).astype(np.float64)[mism]
            step = np.abs(got_e.astype(np.int32) - want_e.astype(np.int32))[mism]
            p2 = np.exp2(np.round(np.log2(np.maximum(v, 1e-300))))
            assert (step == 1).all() and (np.abs(v / p2 - 1.0) <= rl_blk[mism]).all(), f"{name} {ori}: a block scale differs away from a power-of-two boundary"
            assert mism.sum() <= max(2, 1e-4 * mism.size), f"{name} {ori}: {mism.sum()} of {mism.size} block scales differ"
        inv = np.ldexp(np.float32(1.0), 127 - got_e.astype(np.int64)).astype(np.float32)   # the DEVICE's scale
        with np.errstate(over="ignore", invalid="ignore"):
            v_scaled = (mat.reshape(r, c // 32, 32) * inv[:, :, None]).astype(np.float32).reshape(r, c)
        assert (u8(data)[np.isnan(mat)] == O.FP8_NAN_BYTE).all(), f"{name} {ori}: NaN positions must get 0x7F"
        if exact:
            np.testing.assert_array_equal(u8(data), O.fp8_encode_sat(v_scaled, fmt), err_msg=f"{name} {ori}")
        else:
            slack = None if slk is None else (slk.reshape(r, c // 32, 32) * inv[:, :, None].astype(np.float64)).reshape(r, c)
            _check_bytes(u8(data), v_scaled, fmt, fx, rl, slack, f"{name} {ori}")


@pytest.mark.parametrize("assign", [0, 1])
@pytest.mark.parametrize("fmt", [O.E4M3, O.E5M2])
@pytest.mark.parametrize("backward", [False, True], ids=["swiglu", "dswiglu"])
def test_mxfp8_swiglu_quantisers_on_the_exhaustive_gate_sweep(ops, dev, backward, fmt, assign):
    for kind in ("full", "bounded"):
        name = f"mx {'dswiglu' if backward else 'swiglu'} fmt {fmt} assign {assign} {kind}"
        h_bits, d_bits = U.gate_sweep(kind, assign)
        h, d = bits_to_bf16(h_bits, dev), bits_to_bf16(d_bits, dev)
        v32, fixed, rel, slack = U.swiglu_sweep_reference(h_bits, d_bits, None, backward, np.float32(1.0))
        if backward:
            out = ops.mxfp8_dswiglu_quantize(h, d, fmt=fmt, want_colsum=True)
        else:
            out = ops.mxfp8_swiglu_quantize(h, fmt=fmt)
        _check_mx(out[:4], v32, fmt, name, False, kind == "full", fixed, rel, slack)
        if backward:
            with np.errstate(invalid="ignore", over="ignore"):
                ref = v32.astype(np.float64).sum(0)
                colmax = np.where(np.isfinite(v32), np.abs(v32), 0).max(0).astype(np.float64)
                ok = np.isfinite(ref) & (np.abs(ref) < FLT_MAX)
            got_cs = out[4].sum(0).cpu().numpy().astype(np.float64)
            assert not np.isfinite(got_cs[~ok]).any()
            err = np.abs(got_cs[ok] - ref[ok])
            assert (err <= 1e-4 * np.abs(ref[ok]) + 1e-4 * colmax[ok] * np.sqrt(256)).all(), f"{name}: column sums"


# ----------------------------------------------------------------------------------------- 3. RMSNorm cast: identity
RSTD_TABLE = np.array([0.0, 1e-45, 2.0 ** -20, 1.0, 3.7, 1e30, np.inf, np.nan], np.float32)   # 1e-45: the smallest fp32 subnormal
GAMMA_TABLE = np.array([0.0, -1.0, 1.5, 2.0 ** -100, 3e38, np.inf, np.nan, 0.8125, -0.0, 1.0, 0.5625, 2.0], np.float32)


def _norm_sweep(kind):
    """(x bits [256, 256], rstd f32 [256], gamma bits [256]).  rstd by row and gamma by column from the tables; their entries that are
    non-finite or >= 1e30 appear only in every other block of 32 rows / columns (an ordinary entry elsewhere), so that half of the MX
    blocks keep an ordinary scale; "bounded" has none of them at all and |x| < 2^64: a finite amax."""
    i = np.arange(256)
    rs = RSTD_TABLE[(i + i // 8) % 8].copy()
    gm = GAMMA_TABLE[i % 12].copy()
    keep = ((i // 32) % 2 == 1) if kind == "full" else np.zeros(256, dtype=bool)
    with np.errstate(invalid="ignore"):
        rs = np.where(~keep & ~(np.abs(rs) < 1e30), np.float32(0.27), rs).astype(np.float32)
        gm = np.where(~keep & ~(np.abs(gm) < 1e30), np.float32(0.8125), gm).astype(np.float32)
    return U.all_bf16_bits(kind), rs, O.f32_to_bf16_bits(gm)


def _norm_reference(x_bits, rs, g_bits):
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        return O.norm_apply_f32_device_order(x_bits, rs, g_bits)


@pytest.mark.parametrize("kind", ["full", "bounded"])
@pytest.mark.parametrize("scale", [1.0, 32.0, 2.0 ** -20, 3e38])
@pytest.mark.parametrize("fmt", [O.E4M3, O.E5M2])
def test_norm_cast_exhaustive_is_identical_to_the_restatement(ops, dev, fmt, scale, kind):
    x_bits, rs, g_bits = _norm_sweep(kind)
    x, rstd, gamma = bits_to_bf16(x_bits, dev), torch.from_numpy(rs).to(dev), bits_to_bf16(g_bits, dev)
    v32 = _norm_reference(x_bits, rs, g_bits)
    want = O.fp8_encode_sat(_scaled(v32, scale), fmt)
    # an fp32 product that is SUBNORMAL must not be flushed: the sweep holds such intermediates (x * rstd) and results whose byte a
    # flush would change
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        xr = (O.bf16_bits_to_f32(x_bits) * rs[:, None]).astype(np.float32)
    tiny = np.float32(np.finfo(np.float32).tiny)
    sub = ((np.abs(xr) < tiny) & (xr != 0)) | ((np.abs(v32) < tiny) & (v32 != 0))
    if scale == 3e38:
        assert ((want[sub] & 0x7F) != 0).sum() > 100, "the sweep must hold subnormal products that reach a non-zero byte"
    amax = torch.zeros(1, dtype=torch.float32, device=dev)
    y, yT = ops.norm_cast(x, rstd, gamma, _f32(scale, dev), amax, fmt)
    got = u8(y)
    bad = np.nonzero(got != want)
    assert bad[0].size == 0, (f"{bad[0].size} bytes differ; first at {bad[0][0], bad[1][0]}: x {x_bits[bad][0]:#06x} rstd {rs[bad[0][0]]!r} "
                              f"value {v32[bad][0]!r} got {got[bad][0]:#04x} want {want[bad][0]:#04x}; {int(sub[bad].sum())} of them subnormal products")
    np.testing.assert_array_equal(u8(yT), got.T)
    a_ref = O.amax_f32(v32)
    assert _bits32(amax.item()) == _bits32(a_ref), f"amax {amax.item()!r} != amax_f32 of the restatement {a_ref!r}"
    assert (a_ref == np.inf) == (kind == "full")
    for want_y, want_t in ((True, False), (False, True)):
        a1 = torch.zeros(1, dtype=torch.float32, device=dev)
        y1, y1T = ops.norm_cast(x, rstd, gamma, _f32(scale, dev), a1, fmt, want_y=want_y, want_t=want_t)
        assert torch.equal(y1 if want_y else y1T, y if want_y else yT) and _bits32(a1.item()) == _bits32(a_ref)
    if kind == "bounded":  # the guarded atomicMax, as for the SwiGLU casts
        for start, expect in ((np.float32(2.0 ** -140), a_ref), (np.float32(2.0) * a_ref, np.float32(2.0) * a_ref)):
            slot = _f32(float(start), dev)
            ops.norm_cast(x, rstd, gamma, _f32(scale, dev), slot, fmt)
            assert _bits32(slot.item()) == _bits32(expect)


@pytest.mark.parametrize("kind", ["full", "bounded"])
@pytest.mark.parametrize("fmt", [O.E4M3, O.E5M2])
def test_mxfp8_norm_quantize_exhaustive_is_identical_to_the_restatement(ops, dev, fmt, kind):
    x_bits, rs, g_bits = _norm_sweep(kind)
    v32 = _norm_reference(x_bits, rs, g_bits)
    out = ops.mxfp8_norm_quantize(bits_to_bf16(x_bits, dev), torch.from_numpy(rs).to(dev), bits_to_bf16(g_bits, dev), fmt=fmt)
    _check_mx(out, v32, fmt, f"mx norm fmt {fmt} {kind}", True, kind == "full")


def test_rmsnorm_stats_on_degenerate_rows_then_the_cast(ops, dev):
    """Rows with an Inf, a NaN, all zeros and values whose squares overflow float32 -> rstd 0, NaN, rsqrt(eps) (the existing 2 ulp
    against the float32 restatement), 0; ordinary rows beside them.  That rstd then goes through mi_norm_cast: identity."""
    eps = 1e-5
    g = torch.Generator().manual_seed(11)
    x = torch.randn(8, 512, generator=g).to(torch.bfloat16)
    x[0, 77] = float("inf")
    x[1, 300] = float("nan")
    x[2] = 0
    x[3] = 1e30
    x_bits = U.bf16_bits(x)
    rstd = ops.rmsnorm_stats(x.to(dev), eps)
    r = rstd.cpu().numpy()
    print("rstd of the degenerate rows:", r[:4])
    assert r[0] == 0 and np.isnan(r[1]) and r[3] == 0
    with np.errstate(over="ignore", invalid="ignore"):
        r32 = O.rmsnorm_rstd_device_order(x_bits, eps)
    assert r32[0] == 0 and np.isnan(r32[1]) and r32[3] == 0 and r32[2] == np.float32(1.0) / np.sqrt(np.float32(eps))
    rows = [2, 4, 5, 6, 7]
    ulp = np.abs(r[rows].view(np.int32) - r32[rows].view(np.int32))
    assert ulp.max() <= 2, f"rstd differs from the float32 restatement by {ulp.max()} ulp"
    gamma = (torch.rand(512, generator=g) + 0.5).to(torch.bfloat16)
    v32 = _norm_reference(x_bits, r, U.bf16_bits(gamma))
    assert np.isnan(v32[0, 77]) and (v32[0, :77] == 0).all() and np.isnan(v32[1]).all() and (v32[2] == 0).all() and (v32[3] == 0).all()
    for fmt in (O.E4M3, O.E5M2):
        amax = torch.zeros(1, dtype=torch.float32, device=dev)
        y, yT = ops.norm_cast(x.to(dev), rstd, gamma.to(dev), _f32(32.0, dev), amax, fmt)
        np.testing.assert_array_equal(u8(y), O.fp8_encode_sat(_scaled(v32, 32.0), fmt))
        np.testing.assert_array_equal(u8(yT), u8(y).T)
        assert _bits32(amax.item()) == _bits32(O.amax_f32(v32))


# ----------------------------------------------------------------------------------------- 4. current-scaling amax twins
def _partials(ops, dev, call, grid):
    """max over the partials for n_partial in {1, 7, grid}: every entry written (the buffer starts as NaN), all three equal"""
    out = []
    for n in (1, 7, grid):
        p = torch.full((n,), float("nan"), dtype=torch.float32, device=dev)
        call(p)
        pn = p.cpu().numpy()
        assert not np.isnan(pn).any() and (pn >= 0).all(), f"n_partial {n}: an entry was not written (or is a NaN): {pn}"
        out.append(pn.max())
    assert _bits32(out[0]) == _bits32(out[1]) == _bits32(out[2]), f"the maximum depends on n_partial: {out}"
    return np.float32(out[0])


def _plant_nan_at_max(v32, gate_bits, F):
    """gate bits with a NaN where the restatement v32 (a finite tensor) has its maximum: (bits, row, gate column)"""
    r, c = np.unravel_index(np.abs(v32).argmax(), v32.shape)
    bits = gate_bits.copy()
    bits[r, c % F] = 0x7FC0
    return bits, r, c % F


@pytest.mark.parametrize("bias_kind", ["none", "bias"])
@pytest.mark.parametrize("backward", [False, True], ids=["swiglu", "dswiglu"])
def test_swiglu_amax_passes_on_the_sweeps_equal_the_casts_and_the_oracle(ops, dev, backward, bias_kind):
    scale, fmt, assign = (U.DSWIGLU_SCALE, O.E5M2, 1) if backward else (U.SWIGLU_SCALE, O.E4M3, 0)
    bias_bits = U.sweep_bias(bias_kind, assign)
    bias = _dev_or_none(bias_bits, dev)
    grid = ops.amax_grid(256, 256, 32)
    for kind in U.SWEEP_KINDS + ("planted",):
        h_bits, d_bits = U.gate_sweep("bounded" if kind == "planted" else kind, assign)
        if kind == "planted":
            v0 = U.swiglu_sweep_reference(h_bits, d_bits, bias_bits, backward, scale)[0]
            gate, r, c = _plant_nan_at_max(v0, h_bits[:, :256], 256)
            h_bits = np.ascontiguousarray(np.concatenate([gate, h_bits[:, 256:]], axis=1))
        h, d = bits_to_bf16(h_bits, dev), bits_to_bf16(d_bits, dev)
        v32 = U.swiglu_sweep_reference(h_bits, d_bits, bias_bits, backward, scale)[0]
        a_ref = O.amax_f32(v32)
        got = _partials(ops, dev, (lambda p: ops.amax_dswiglu(h, bias, d, p)) if backward else (lambda p: ops.amax_swiglu(h, bias, p)), grid)
        slot = torch.zeros(1, dtype=torch.float32, device=dev)
        _run_swiglu(ops, dev, backward, h, d, bias, scale, slot, fmt)
        print(f"{'dswiglu' if backward else 'swiglu'} bias {bias_kind} {kind}: amax pass {got!r} cast {slot.item()!r} restatement {a_ref!r}")
        assert _bits32(got) == _bits32(slot.item()), f"{kind}: the amax pass saw {got!r}, the cast published {slot.item()!r}"
        if kind in ("full", "finite"):
            assert got == np.inf == a_ref            # Inf gives Inf, the NaNs beside it are ignored
        else:
            assert np.isfinite(a_ref) and a_ref > 0
            np.testing.assert_allclose(got, a_ref, rtol=2e-6)
        if kind == "planted":                         # the NaN is out of the ranking: the runner-up is reported
            assert np.isnan(v32[r, c]) and a_ref < O.amax_f32(v0) and got < O.amax_f32(v0)


def test_norm_amax_pass_on_the_sweeps_equals_the_cast_and_the_oracle(ops, dev):
    grid = ops.amax_grid(256, 256)
    for kind in ("full", "bounded", "planted"):
        x_bits, rs, g_bits = _norm_sweep("bounded" if kind == "planted" else kind)
        if kind == "planted":
            x_bits[128:] = 0  # the negative patterns: every |value| would occur twice, and the runner-up would equal the maximum
            v0 = _norm_reference(x_bits, rs, g_bits)
            x_bits, r, c = _plant_nan_at_max(v0, x_bits, 256)
        x, rstd, gamma = bits_to_bf16(x_bits, dev), torch.from_numpy(rs).to(dev), bits_to_bf16(g_bits, dev)
        v32 = _norm_reference(x_bits, rs, g_bits)
        a_ref = O.amax_f32(v32)
        got = _partials(ops, dev, lambda p: ops.amax_norm(x, rstd, gamma, p), grid)
        slot = torch.zeros(1, dtype=torch.float32, device=dev)
        ops.norm_cast(x, rstd, gamma, _f32(32.0, dev), slot, O.E4M3)
        print(f"norm {kind}: amax pass {got!r} cast {slot.item()!r} restatement {a_ref!r}")
        assert _bits32(got) == _bits32(slot.item()) == _bits32(a_ref)
        assert (a_ref == np.inf) == (kind == "full")
        if kind == "planted":
            assert np.isnan(v32[r, c]) and a_ref < O.amax_f32(v0)
