"""CPU tests of the oracle itself (oracle/fp8_oracle.py).  PARITY UNPINNED w.r.t. the reference: it
ships no fixtures for this path; the oracle is pinned here against (a) hand-derived OCP FP8 / MX
known answers and (b) torch's independent float8 casts."""
import numpy as np
import pytest
import torch

from oracle import fp8_oracle as O


def _bf16_bits(t: torch.Tensor) -> np.ndarray:
    return t.to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)


def test_decode_tables_match_torch():
    b = torch.arange(256, dtype=torch.uint8)
    for fmt, dt in ((O.E4M3, torch.float8_e4m3fn), (O.E5M2, torch.float8_e5m2)):
        ref = b.view(dt).float().numpy()
        got = O.fp8_decode(b.numpy(), fmt)
        np.testing.assert_array_equal(np.isnan(ref), np.isnan(got))
        np.testing.assert_array_equal(ref[~np.isnan(ref)], got[~np.isnan(got)])


def test_encode_known_answers_e4m3():
    # value -> byte (OCP E4M3FN, RNE, saturating)
    kat = {0.0: 0x00, 1.0: 0x38, 17.0: 0x58, 19.0: 0x5A, 447.0: 0x7E, 448.0: 0x7E, 449.0: 0x7E,
           480.0: 0x7E, 1e5: 0x7E, float("inf"): 0x7E, -float("inf"): 0xFE, 2.0 ** -9: 0x01, 2.0 ** -10: 0x00,
           1.5 * 2.0 ** -10: 0x01, 3 * 2.0 ** -10: 0x02, 2.0 ** -6: 0x08, 0.9375 * 2.0 ** -6: 0x08,
           float("nan"): 0x7F}
    v = np.array(list(kat.keys()), dtype=np.float32)
    np.testing.assert_array_equal(O.fp8_encode_sat(v, O.E4M3), np.array(list(kat.values()), dtype=np.uint8))
    assert O.fp8_encode_sat(np.array([-0.0], np.float32), O.E4M3)[0] == 0x80


def test_encode_known_answers_e5m2():
    kat = {0.0: 0x00, 1.0: 0x3C, 57344.0: 0x7B, 61440.0: 0x7B, 1e9: 0x7B, float("inf"): 0x7B,
           -float("inf"): 0xFB, 2.0 ** -16: 0x01, 2.0 ** -17: 0x00, 1.5 * 2.0 ** -17: 0x01, 2.0 ** -14: 0x04,
           float("nan"): 0x7F, 1.125: 0x3C, 1.375: 0x3E, 1.25: 0x3D}
    v = np.array(list(kat.keys()), dtype=np.float32)
    np.testing.assert_array_equal(O.fp8_encode_sat(v, O.E5M2), np.array(list(kat.values()), dtype=np.uint8))


@pytest.mark.parametrize("fmt,dt", [(O.E4M3, torch.float8_e4m3fn), (O.E5M2, torch.float8_e5m2)])
def test_encode_matches_torch_on_all_bf16_and_random_f32(fmt, dt):
    mx = float(O.FP8_MAX[fmt])
    allbf = torch.arange(65536, dtype=torch.int32).to(torch.int16).view(torch.bfloat16).float()
    g = torch.Generator().manual_seed(0)
    rnd = torch.randn(200000, generator=g) * torch.exp(torch.randn(200000, generator=g) * 6)
    for x in (allbf, rnd, rnd * 1e-3, rnd * 1e3):
        finite = ~torch.isnan(x)
        ref = x.clamp(-mx, mx).to(dt).view(torch.uint8).numpy()
        got = O.fp8_encode_sat(x.numpy(), fmt)
        np.testing.assert_array_equal(ref[finite.numpy()], got[finite.numpy()])
        assert np.all(got[~finite.numpy()] == 0x7F)


def test_bf16_round_matches_torch():
    g = torch.Generator().manual_seed(1)
    x = torch.randn(100000, generator=g) * 37
    np.testing.assert_array_equal(O.f32_to_bf16_bits(x.numpy()), _bf16_bits(x))


def test_quantize_delayed_amax_and_scale():
    x = torch.tensor([[0.5, -3.0, float("nan"), 2.0] * 2] * 8)
    q, amax = O.quantize_delayed(_bf16_bits(x), np.float32(2.0), O.E4M3)
    assert amax == np.float32(3.0)
    assert q[0, 0] == 0x38 and q[0, 1] == 0xCC and q[0, 2] == 0x7F and q[0, 3] == 0x48


def test_scale_update_known_trajectory():
    H = 4
    hist = np.zeros((H, 2), np.float32)
    scale = np.ones(2, np.float32)
    seq = [(2.0, 0.0), (0.0, 0.0), (8.0, np.inf), (1.0, 3.0), (0.5, 0.0), (0.25, 0.0), (0.125, 0.0), (0.0625, 0.0)]
    exp_max = []
    for a0, a1 in seq:
        hist[0] = (a0, a1)
        hist, scale, inv = O.scale_update(hist, scale, np.float32(448.0), 0, "max")
        exp_max.append(scale.copy())
        assert hist[0, 0] == 0 and hist[0, 1] == 0
        np.testing.assert_array_equal(inv, np.float32(1) / scale)
    # slot 0, hand-traced: roll(-1) moves row 0 to row H-1 and zeroes the new row 0 (drops old row 1)
    np.testing.assert_allclose([s[0] for s in exp_max], [224, 224, 56, 56, 56, 56, 448, 896])
    # slot 1: 0 -> keep 1; inf -> keep; then 3 in window for 3 more steps
    np.testing.assert_allclose([s[1] for s in exp_max][:4], [1, 1, 1, 1])


def test_scale_update_most_recent_and_margin():
    hist = np.zeros((8, 1), np.float32)
    hist[0, 0] = 7.0
    hist[3, 0] = 100.0
    _, s, _ = O.scale_update(hist, np.ones(1, np.float32), np.float32(448.0), 1, "most_recent")
    assert s[0] == np.float32(448.0 / 7.0) / 2


def test_e8m0_roundup():
    v = np.array([1.0, 1.0000001, 0.75, 2.0 ** -127, 1.5 * 2.0 ** -127, 0.0, np.inf, np.nan, 2.0 ** 127, 3e38],
                 dtype=np.float32)
    np.testing.assert_array_equal(O.float_to_e8m0_roundup(v), [127, 128, 127, 0, 1, 0, 0xFE, 0xFF, 254, 254])


def test_mxfp8_quantize_roundtrip_bound_and_layout():
    g = torch.Generator().manual_seed(2)
    x = (torch.randn(64, 96, generator=g) * torch.exp(torch.randn(64, 1, generator=g) * 3)).to(torch.bfloat16)
    bits = _bf16_bits(x)
    q, e = O.mxfp8_quantize_rowwise(bits)
    assert q.shape == (64, 96) and e.shape == (64, 3)
    deq = O.fp8_decode(q, O.E4M3) * np.repeat(O.e8m0_to_f32(e), 32, axis=1)
    xf = x.float().numpy()
    amax_b = np.abs(xf).reshape(64, 3, 32).max(-1)
    # scaled values never exceed 448, and the block max uses the top binade (>= 224)
    scaled_max = amax_b / O.e8m0_to_f32(e)
    assert np.all(scaled_max <= 448.0) and np.all(scaled_max[amax_b > 0] > 224.0 * (1 - 2 ** -8))
    assert np.all(np.abs(deq - xf) <= np.repeat(O.e8m0_to_f32(e), 32, axis=1) * 16 + 1e-30)  # half-ulp at top binade = 16
    qc, ec = O.mxfp8_quantize_colwise(bits)
    q2, e2 = O.mxfp8_quantize_rowwise(np.ascontiguousarray(bits.T))
    np.testing.assert_array_equal(qc, q2)
    np.testing.assert_array_equal(ec, e2)


def test_gemm_oracle_against_float_matmul():
    g = torch.Generator().manual_seed(3)
    a = torch.randn(32, 64, generator=g)
    b = torch.randn(48, 64, generator=g)
    a8 = O.fp8_encode_sat(a.numpy(), O.E4M3)
    b8 = O.fp8_encode_sat(b.numpy(), O.E5M2)
    d = O.gemm_fp8_tn(a8, b8, O.E4M3, O.E5M2, 0.5, 2.0, out_f32=True)
    ref = O.fp8_decode(a8, O.E4M3).astype(np.float64) @ O.fp8_decode(b8, O.E5M2).astype(np.float64).T
    np.testing.assert_allclose(d, ref, rtol=1e-6)


def test_delayed_linear_oracle_runs_three_steps():
    g = torch.Generator().manual_seed(4)
    lin = O.DelayedLinearOracle(O.E4M3, O.E5M2, history_len=4)
    w = _bf16_bits(torch.randn(32, 64, generator=g) * 0.02)
    for step in range(3):
        x = _bf16_bits(torch.randn(16, 64, generator=g))
        dy = _bf16_bits(torch.randn(16, 32, generator=g) / 32)
        y = lin.forward(x, w)
        lin.end_forward()
        dx, dw, db = lin.backward(dy)
        lin.end_backward()
        assert y.shape == (16, 32) and dx.shape == (16, 64) and dw.shape == (32, 64) and db.shape == (32,)
    assert lin.s_fwd[0] > 1 and lin.s_fwd[1] > 1000 and lin.s_bwd[0] > 1000
    # relative error of the fp8 forward vs the float matmul stays at the few-percent level
    xf, wf = O.bf16_bits_to_f32(x), O.bf16_bits_to_f32(w)
    ref = xf @ wf.T
    err = np.linalg.norm(O.bf16_bits_to_f32(y) - ref) / np.linalg.norm(ref)
    assert err < 0.08, err


def test_device_order_restatements_agree_with_the_float64_ones():
    """The float32, kernel-order restatements of the fused front ends (used to pin the fused kernels byte for byte except at
    rounding boundaries) are the same functions as the float64 ones, to float32 accuracy."""
    rng = np.random.default_rng(5)
    h = O.f32_to_bf16_bits((rng.normal(size=(64, 256)) * 2).astype(np.float32))
    d = O.f32_to_bf16_bits((rng.normal(size=(64, 128)) / 8).astype(np.float32))
    a, b = O.swiglu_f32_device_order(h), O.swiglu_f32(h)
    assert np.all(np.abs(a - b) <= 4e-6 * np.maximum(np.abs(b), 1e-3))
    a, b = O.dswiglu_f32_device_order(h, d), O.dswiglu_f32(h, d)
    assert np.all(np.abs(a - b) <= 1e-5 * np.maximum(np.abs(b), 1e-3))
    x = O.f32_to_bf16_bits((rng.normal(size=(9, 1032)) * np.exp(rng.normal(size=(9, 1)))).astype(np.float32))  # 1032: a ragged last sweep
    gam = O.f32_to_bf16_bits((rng.random(1032) + 0.5).astype(np.float32))
    y64, rstd64 = O.rmsnorm_f32(x, gam, 1e-5)
    rstd32 = O.rmsnorm_rstd_device_order(x, 1e-5)
    np.testing.assert_allclose(rstd32, rstd64, rtol=1e-6)
    y32 = O.norm_apply_f32_device_order(x, rstd32, gam)
    np.testing.assert_allclose(y32, y64, rtol=2e-6, atol=1e-7)


def test_fp8_mismatch_classifier():
    v = np.array([1.0, 17.0, 17.0, 17.0, 98.0], np.float32)  # 17 is the midpoint of the E4M3 codes 16 and 18
    want = O.fp8_encode_sat(v, O.E4M3)
    got = want.copy()
    assert O.fp8_mismatches_near_boundary(got, v, O.E4M3) == (0, 0)
    got[1] = O.fp8_encode_sat(np.array([18.0], np.float32), O.E4M3)[0]   # neighbour code, value ON the boundary: explained
    assert O.fp8_mismatches_near_boundary(got, v, O.E4M3) == (1, 0)
    got[4] = O.fp8_encode_sat(np.array([104.0], np.float32), O.E4M3)[0]  # neighbour code of 96 (98 -> 96), but 98 is no boundary (100 is)
    assert O.fp8_mismatches_near_boundary(got, v, O.E4M3) == (2, 1)
    assert O.fp8_mismatches_near_boundary(got, v, O.E4M3, abs_slack=np.full(5, 10.0)) == (2, 0)


@pytest.mark.parametrize("B,S,H,G,D", [(2, 40, 3, 3, 64), (1, 96, 6, 2, 128), (2, 40, 8, 2, 64), (1, 96, 4, 1, 128)])
@pytest.mark.parametrize("causal", [True, False])
def test_attention_oracle_against_torch_float64_autograd(B, S, H, G, D, causal):
    """attention_f64 / attention_bwd_f64 (hand-derived backward) against torch float64 on the CPU: an explicit softmax with
    repeat_interleave for GQA, differentiated by autograd, and scaled_dot_product_attention for the forward."""
    g = torch.Generator().manual_seed(S * H + D + causal)
    q, k, v = (torch.randn(B, S, n, D, generator=g).to(torch.bfloat16) for n in (H, G, G))
    do = torch.randn(B, S, H, D, generator=g).to(torch.bfloat16)
    q = (q.float() * 2.0).to(torch.bfloat16)
    scale = D ** -0.5
    o, lse = O.attention_f64(_bf16_bits(q), _bf16_bits(k), _bf16_bits(v), scale, causal)
    dq, dk, dv = O.attention_bwd_f64(_bf16_bits(q), _bf16_bits(k), _bf16_bits(v), _bf16_bits(do), scale, causal)
    assert o.dtype == lse.dtype == dq.dtype == dk.dtype == dv.dtype == np.float64

    qr, kr, vr = (t.double().transpose(1, 2).requires_grad_(True) for t in (q, k, v))  # [B, n, S, D]
    ke, ve = kr.repeat_interleave(H // G, 1), vr.repeat_interleave(H // G, 1)
    s = (qr @ ke.transpose(-1, -2)) * scale
    if causal:
        s = s.masked_fill(torch.triu(torch.ones(S, S, dtype=torch.bool), 1), float("-inf"))
    o_t = torch.softmax(s, -1) @ ve
    lse_t = torch.logsumexp(s, -1) / np.log(2.0)
    o_t.backward(do.double().transpose(1, 2))
    o_sdpa = torch.nn.functional.scaled_dot_product_attention(qr.detach(), ke.detach(), ve.detach(), is_causal=causal,
                                                              scale=scale)

    def close(got, ref, what):  # float64 rounding level: both sides sum O(S + D) terms of size <= max|ref| * O(1)
        err = np.abs(got - ref).max() / np.abs(ref).max()
        assert err < 1e-12, f"{what}: max error {err:.3g} of max|ref|"

    close(o, o_t.detach().transpose(1, 2).numpy(), "o")
    close(o, o_sdpa.transpose(1, 2).numpy(), "o vs sdpa")
    close(lse, lse_t.detach().numpy(), "lse")
    close(dq, qr.grad.transpose(1, 2).numpy(), "dq")
    close(dk, kr.grad.transpose(1, 2).numpy(), "dk")
    close(dv, vr.grad.transpose(1, 2).numpy(), "dv")

    # o_bits: delta = rowsum(dO * O) of a stored bf16 O.  dS = P (dP - delta) is linear in delta, so dq and dk move by
    # -scale P (delta' - delta) times k and q; dv does not move
    o_bits = _bf16_bits(torch.from_numpy(o))
    dq2, dk2, dv2 = O.attention_bwd_f64(_bf16_bits(q), _bf16_bits(k), _bf16_bits(v), _bf16_bits(do), scale, causal, o_bits=o_bits)
    o_b = torch.from_numpy(O.bf16_bits_to_f32(o_bits).astype(np.float64)).transpose(1, 2)
    dd = ((do.double().transpose(1, 2) * (o_b - o_t.detach())).sum(-1, keepdims=True))  # delta' - delta [B, H, S, 1]
    p = torch.softmax(s.detach(), -1)
    ds_shift = -scale * p * dd
    close(dq2 - dq, (ds_shift @ ke.detach()).transpose(1, 2).numpy(), "dq shift from the stored O")
    dk_shift = (ds_shift.transpose(-1, -2) @ qr.detach()).reshape(B, G, H // G, S, D).sum(2)
    close(dk2 - dk, dk_shift.transpose(1, 2).numpy(), "dk shift from the stored O")
    assert np.array_equal(dv2, dv)


# ----------------------------------------------------------------------------------------- edge semantics of the fused casts
# (the kernels are held to these on the GPU in tests/test_fused_cast_edges_gpu.py)
_KAT_GATES = [np.nan, np.inf, -np.inf, 17, 30, 88, 89, 100, 3e38, -17, -30, -88, -88.5, -89, -100, -3e38, -0.0, 0.0]
_KAT_UPS = [1, 0, -1, np.nan, np.inf, -np.inf, 3e38]


def _kat_h():
    """h bits [18, 14]: gate i in every column of row i, up j in column 7 + j; plus the gates and ups as bf16-rounded float32"""
    g = O.round_to_bf16(np.array(_KAT_GATES, np.float32))
    u = O.round_to_bf16(np.array(_KAT_UPS, np.float32))
    h = np.concatenate([np.repeat(g[:, None], len(u), 1), np.repeat(u[None, :], len(g), 0)], axis=1)
    return O.f32_to_bf16_bits(h), g, u


def test_swiglu_restatements_known_answers_at_the_edges():
    """What silu(g) * u is at the edges follows from the restatement ((g * (1 / (1 + exp(-g)))) * u, every operation float32) and
    IEEE arithmetic alone; nothing here comes from a device.  Scale 16, both formats."""
    import warnings
    h_bits, g, u = _kat_h()
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        v = O.swiglu_f32_device_order(h_bits)
        v64 = O.swiglu_f32(h_bits)
    mx = {O.E4M3: 0x7E, O.E5M2: 0x7B}
    with np.errstate(over="ignore", invalid="ignore"):
        vs = (v * np.float32(16.0)).astype(np.float32)
    G, Uu = np.meshgrid(g, u, indexing="ij")
    with np.errstate(over="ignore", invalid="ignore"):
        gu = (G * Uu).astype(np.float32)
    fin_g = np.isfinite(G)
    for fmt in (O.E4M3, O.E5M2):
        b = O.fp8_encode_sat(vs, fmt)
        row = lambda x: _KAT_GATES.index(x) if not np.isnan(x) else 0
        col = lambda x: 3 if np.isnan(x) else _KAT_UPS.index(x)
        assert (b[np.isnan(G) | np.isnan(Uu)] == 0x7F).all()                      # NaN in gate or up
        assert b[row(np.inf), col(1)] == mx[fmt]                                  # +Inf * 1 (sigmoid 1)
        assert b[row(np.inf), col(0)] == 0x7F                                     # Inf * 0
        assert b[row(np.inf), col(-1)] == mx[fmt] | 0x80
        assert (b[row(-np.inf)] == 0x7F).all()                                    # -Inf * sigmoid(-Inf) = -Inf * 0
        # up = +-Inf under a finite gate that does not vanish in the product: +- max code, the sign of g * u
        for gi in (17, 30, 88, 89, 100, 3e38, -17, -30, -88, -88.5):
            sgn = 0x80 if gi < 0 else 0
            assert b[row(gi), col(np.inf)] == mx[fmt] | sgn and b[row(gi), col(-np.inf)] == mx[fmt] | (sgn ^ 0x80)
        assert b[row(3e38), col(1)] == mx[fmt]                                    # 3e38 * 16 overflows float32: + max code
        assert b[row(3e38), col(3e38)] == mx[fmt]
    # g >= 17: 1 + exp(-g) rounds to 1, the sigmoid is exactly 1 and silu(g) * u == g * u, bit for bit
    big = fin_g & (G >= 17)
    np.testing.assert_array_equal(v[big].view(np.uint32), gu[big].view(np.uint32))
    # g <= -89: exp(-g) overflows float32, the sigmoid is exactly 0 and g * 0 = -0.0; times u > 0: -0.0 (byte 0x80)
    for gi in (-89, -100, -3e38):
        r = _KAT_GATES.index(gi)
        assert v[r, 0] == 0 and np.signbit(v[r, 0]) and v[r, 6] == 0 and np.signbit(v[r, 6])      # u = 1, 3e38
        assert v[r, 2] == 0 and not np.signbit(v[r, 2])                                           # u = -1: +0.0
        assert np.isnan(v[r, 4]) and np.isnan(v[r, 5])                                            # -0.0 * +-Inf
        assert O.fp8_encode_sat(vs[r, :1], O.E4M3)[0] == 0x80 and O.fp8_encode_sat(vs[r, :1], O.E5M2)[0] == 0x80
    # -88.5: exp(88.5) is still finite, the sigmoid a float32 subnormal, the product a tiny negative number -- not flushed
    r = _KAT_GATES.index(-88.5)
    assert v[r, 0] < 0 and abs(v[r, 0] / v64[r, 0] - 1) < 1e-5
    # signed zero gates: sigmoid 1/2, the zero keeps its sign through both products
    rz, rp = _KAT_GATES.index(0.0), len(g) - 1
    assert np.signbit(g[rz]) and not np.signbit(g[rp])
    assert np.signbit(v[rz, 0]) and not np.signbit(v[rz, 2]) and not np.signbit(v[rp, 0]) and np.signbit(v[rp, 2])
    assert (v[[rz, rp]][:, [0, 1, 2, 6]] == 0).all() and np.isnan(v[[rz, rp]][:, [3, 4, 5]]).all()
    # the amax of such values: NaN ignored, Inf gives Inf
    assert O.amax_f32(v) == np.inf
    assert O.amax_f32(v[_KAT_GATES.index(30)][[0, 1, 2, 3]]) == np.float32(30.0)   # {30, 0, -30, NaN}
    assert O.amax_f32(np.array([np.nan, -3.0, 2.0], np.float32)) == np.float32(3.0)
    assert O.amax_f32(np.array([np.nan, np.nan], np.float32)) == 0
    # the float64 form agrees wherever both are finite and non-zero
    both = np.isfinite(v) & np.isfinite(v64) & (v != 0) & (v64 != 0)
    np.testing.assert_allclose(v[both], v64[both], rtol=1e-5)


def test_dswiglu_restatements_known_answers_at_the_edges():
    import warnings
    h_bits, g, u = _kat_h()
    d = O.round_to_bf16(np.array([0.5, -2.0, 0.5, -2.0, 0.5, -2.0, 0.5], np.float32))
    d_bits = O.f32_to_bf16_bits(np.repeat(d[None, :], len(g), 0))
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        v = O.dswiglu_f32_device_order(h_bits, d_bits)
        v64 = O.dswiglu_f32(h_bits, d_bits)
    F = len(u)
    left, right = v[:, :F], v[:, F:]
    G, Uu = np.meshgrid(g, u, indexing="ij")
    D = np.repeat(d[None, :], len(g), 0)
    with np.errstate(over="ignore", invalid="ignore"):
        du, dg = (D * Uu).astype(np.float32), (D * G).astype(np.float32)
    big = np.isfinite(G) & (G >= 17)
    # g >= 17: sigmoid exactly 1, dsilu = 1 * (1 + g * 0) = 1: the gate half is d * u, the up half d * g, bit for bit (NaN as NaN)
    ok = big & ~np.isnan(du)
    np.testing.assert_array_equal(left[ok].view(np.uint32), du[ok].view(np.uint32))
    assert np.isnan(left[big & np.isnan(du)]).all()
    np.testing.assert_array_equal(right[big].view(np.uint32), dg[big].view(np.uint32))
    r = _KAT_GATES.index(np.inf)
    assert np.isnan(left[r]).all()                        # g = +Inf: Inf * (1 - 1) inside dsilu
    assert (right[r] == np.inf * d).all()                 # d * (Inf * 1)
    r = _KAT_GATES.index(-np.inf)
    assert np.isnan(v[r]).all()                           # 0 * -Inf on both sides
    for gi in (-89, -100, -3e38):                         # sigmoid exactly 0: both halves are signed zeros (NaN under u = +-Inf / NaN)
        r = _KAT_GATES.index(gi)
        fin = np.isfinite(u)
        assert (left[r, fin] == 0).all() and np.isnan(left[r, ~fin]).all() and (right[r] == 0).all()
        assert (np.signbit(right[r]) == (d > 0)).all()    # d * (g * 0) = d * -0.0
    both = np.isfinite(v) & np.isfinite(v64) & (v != 0) & (v64 != 0)
    np.testing.assert_allclose(v[both], v64[both], rtol=2e-5)


def test_mx_block_amax_ignores_nan_and_keeps_inf():
    v = np.zeros((2, 64), np.float32)
    v[0, :32] = [np.nan, -5.0] + [1.0] * 30
    v[0, 32:] = np.nan
    v[1, :32] = [np.nan, -np.inf] + [3.0] * 30
    v[1, 40] = -0.25
    np.testing.assert_array_equal(O.mx_block_amax(v), np.array([[5.0, 0.0], [np.inf, 0.25]], np.float32))
    assert list(O.float_to_e8m0_roundup(O.mx_block_amax(v)[1] / np.float32(448.0))) == [0xFE, 117]   # 0.25 / 448 = 1.14 * 2^-11 -> 2^-10
    # the quantiser uses it: a NaN keeps its 0x7F byte and does not touch the block's scale
    x = O.f32_to_bf16_bits(np.array([[np.nan, 448.0] + [1.0] * 30], np.float32))
    q, e = O.mxfp8_quantize_rowwise(x)
    assert e[0, 0] == 127 and q[0, 0] == 0x7F and q[0, 1] == 0x7E and q[0, 2] == 0x38


@pytest.mark.parametrize("backward", [False, True])
def test_fused_cast_edge_sweeps_run_clean_and_stay_under_the_mismatch_cap(backward):
    """The inputs of tests/test_fused_cast_edges_gpu.py, evaluated by the oracle alone:
      * all four SwiGLU restatements run without a numpy warning on every bf16 pattern (warnings are errors here);
      * the number of reference values that lie INSIDE their rounding-boundary band -- where the device may legitimately produce the
        neighbouring code -- stays below the cap the GPU test puts on explained mismatches, max(2, 1e-3 size); the same for the
        MX block scales against max(2, 1e-4 blocks).  Were it not so, the tables in tests/util.py would have to change, not the cap."""
    import warnings
    from tests import util as U
    scale = U.DSWIGLU_SCALE if backward else U.SWIGLU_SCALE
    worst = worst_mx = 0
    for assign in (0, 1):
        for bias_kind in ("none", "bias", "nan"):
            for kind in U.SWEEP_KINDS:
                h, d = U.gate_sweep(kind, assign)
                b = U.sweep_bias(bias_kind, assign)
                with warnings.catch_warnings():
                    warnings.simplefilter("error")
                    v32, fixed, rel, slack = U.swiglu_sweep_reference(h, d, b, backward, scale)
                    if bias_kind == "none":
                        v64 = O.dswiglu_f32(h, d) if backward else O.swiglu_f32(h)
                with np.errstate(invalid="ignore"):
                    both = np.isfinite(v32) & np.isfinite(v64) & (np.abs(v64) > 1e-30) if bias_kind == "none" else None
                if both is not None:   # the two restatements are the same function on the whole sweep (dsilu: away from its zero)
                    err = np.abs(v32[both].astype(np.float64) - v64[both]) / np.abs(v64[both])
                    assert np.quantile(err, 0.999) < 1e-5
                assert (O.amax_f32(v32) == np.inf) == (kind != "bounded")
                with np.errstate(over="ignore", invalid="ignore"):
                    vs = (v32 * scale).astype(np.float32)
                for fmt in (O.E4M3, O.E5M2):
                    n = int((U.fp8_in_boundary_band(vs, fmt, rel, slack) & ~fixed).sum())
                    worst = max(worst, n)
                    assert n <= max(2, 1e-3 * v32.size), f"{n} reference values inside their band ({assign}, {bias_kind}, {kind}, fmt {fmt})"
                if bias_kind == "none" and kind != "finite":   # the MX twins take no bias and run the full and the bounded sweep
                    v1, fixed1, rel1, _ = U.swiglu_sweep_reference(h, d, None, backward, np.float32(1.0))
                    for fmt in (O.E4M3, O.E5M2):
                        n = U.mx_scales_in_band(v1, fixed1, rel1, fmt)
                        worst_mx = max(worst_mx, n)
                        assert n <= 2, f"{n} MX block scales inside their band ({assign}, {kind}, fmt {fmt})"
    print("most reference values inside a band:", worst, "block scales:", worst_mx)
