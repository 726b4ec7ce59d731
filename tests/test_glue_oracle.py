"""CPU: the criteria of tests/glue_oracle.py are sound and sharp.  Each is fed the output of a numpy "kernel" that restates the
device arithmetic in float32 -- it must accept it -- and outputs that are wrong in one way each -- it must reject every one.  The
ambiguity cap of the RoPE criterion is asserted here for the very inputs tests/test_glue_kernels_gpu.py runs on the device."""
import numpy as np
import pytest

from tests import glue_oracle as G


# ------------------------------------------------------------------------------------------------ the bf16 rounding itself
def test_rne_bf16_is_one_rounding_from_float64():
    every = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    finite = every[((every >> 7) & 0xFF) != 0xFF]
    v = G.bf16_to_f64(finite)
    np.testing.assert_array_equal(G.rne_bf16(v), finite)                       # every bf16 value is a fixed point, -0 included
    pos = np.sort(v[v > 0])
    mid = 0.5 * (pos[:-1] + pos[1:])                                            # exact in float64
    lo_bits, hi_bits = G.rne_bf16(pos[:-1]), G.rne_bf16(pos[1:])
    even = np.where(lo_bits % 2 == 0, lo_bits, hi_bits)
    np.testing.assert_array_equal(G.rne_bf16(mid), even)                        # ties go to the even pattern
    np.testing.assert_array_equal(G.rne_bf16(np.nextafter(mid, np.inf)), hi_bits)
    np.testing.assert_array_equal(G.rne_bf16(np.nextafter(mid, 0.0)), lo_bits)
    np.testing.assert_array_equal(G.rne_bf16(-np.nextafter(mid, np.inf)), hi_bits | 0x8000)
    # a value a float32 rounding would first move ONTO a tie and a second rounding then past it: 1 + 2^-8 + 2^-40 is above the
    # tie between 1 and 1 + 2^-7 (-> 0x3F81), but float32 rounds it to the tie itself, which then goes to even (0x3F80)
    x = 1.0 + 2.0 ** -8 + 2.0 ** -40
    assert G.rne_bf16(x) == 0x3F81
    top = float(G.bf16_to_f64(np.uint16(0x7F7F)))
    assert G.rne_bf16(top + 2.0 ** 119) == 0x7F80 and G.rne_bf16(np.nextafter(top + 2.0 ** 119, 0.0)) == 0x7F7F
    assert G.rne_bf16(-np.inf) == 0xFF80 and G.rne_bf16(np.nan) == 0x7FC0
    assert G.rne_bf16(2.0 ** -134) == 0 and G.rne_bf16(1.5 * 2.0 ** -133) == 2 and G.rne_bf16(-(2.0 ** -133)) == 0x8001
    f = np.random.default_rng(0).standard_normal(4096).astype(np.float32)
    u = f.view(np.uint32).astype(np.uint64)
    np.testing.assert_array_equal(G.f32_to_bf16(f), ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16))


# ------------------------------------------------------------------------------------------------ RoPE
def _rope_checks(case, out, cos, sin, qkv):
    """(all ok, ambiguous counts) of q and k outputs against float64."""
    B, S, nq, nkv, D, rows = case
    q, k, v = out
    oks, amb = [], []
    for got, src in ((q, qkv[:, :nq * D]), (k, qkv[:, nq * D:(nq + nkv) * D])):
        e, m = G.rope_ref(src, cos, sin, S, D, backward=False)
        ok, a = G.rounded_within(got, e, m)
        oks.append(bool(ok.all()))
        amb.append(int(a.sum()))
    return all(oks) and np.array_equal(v, qkv[:, (nq + nkv) * D:]), amb


@pytest.mark.parametrize("case", G.ROPE_CASES, ids=lambda c: "x".join(map(str, c)))
def test_rope_criterion_accepts_float32_kernel_and_caps_ambiguity(case, capsys):
    """The float32 restatement passes at every case, and the inputs the GPU test uses stay under the ambiguity cap, forward and
    backward, per compared tensor."""
    B, S, nq, nkv, D, rows = case
    inp = G.rope_case_inputs(case)
    assert inp["cos"].shape == (S + 3, D // 2) and np.isnan(inp["cos"][S:]).all() and np.isfinite(inp["cos"][:S]).all()
    ok, amb = _rope_checks(case, G.rope_kernel_f32(inp["qkv"], inp["cos"], inp["sin"], S, nq, nkv, D), inp["cos"], inp["sin"], inp["qkv"])
    assert ok
    counts = {"q": (amb[0], rows * nq * D), "k": (amb[1], rows * nkv * D)}
    for name, heads in (("dq", nq), ("dk", nkv)):
        e, m = G.rope_ref(inp[name], inp["cos"], inp["sin"], S, D, backward=True)
        counts[name] = (int(G.rounded_within(G.rne_bf16(e), e, m)[1].sum()), rows * heads * D)
    for name, (n_amb, n) in counts.items():
        assert n_amb <= G.rope_ambiguity_cap(n), f"{name}: {n_amb} of {n} ambiguous: change the input, not the cap"
    with capsys.disabled():
        print(f"\n  rope {case}: ambiguous " + ", ".join(f"{k} {a}/{n}" for k, (a, n) in counts.items()), end="")


@pytest.mark.parametrize("mutant", ["trunc", "pos+1", "sin_lane", "row_seq", "qk_swap"])
def test_rope_criterion_rejects_mutants(mutant):
    case = G.ROPE_CASES[2]  # (2, 40, 5, 3, 64): several heads of both kinds, two sequences
    B, S, nq, nkv, D, rows = case
    inp = G.rope_case_inputs(case)
    cos, sin = G.rope_tables(S, D, poison=False)        # row S is finite: "row_seq" must be caught by its values, not by a NaN
    good, _ = _rope_checks(case, G.rope_kernel_f32(inp["qkv"], cos, sin, S, nq, nkv, D), cos, sin, inp["qkv"])
    bad, _ = _rope_checks(case, G.rope_kernel_f32(inp["qkv"], cos, sin, S, nq, nkv, D, mutant=mutant), cos, sin, inp["qkv"])
    assert good and not bad


def test_rope_criterion_rejects_one_ulp_on_one_element():
    """What the old 98 % criterion let through: ONE element one bf16 ulp off, wherever the criterion is not ambiguous."""
    case = G.ROPE_CASES[3]
    B, S, nq, nkv, D, rows = case
    inp = G.rope_case_inputs(case)
    q, _, _ = G.rope_kernel_f32(inp["qkv"], inp["cos"], inp["sin"], S, nq, nkv, D)
    e, m = G.rope_ref(inp["qkv"][:, :nq * D], inp["cos"], inp["sin"], S, D, backward=False)
    ok, amb = G.rounded_within(q, e, m)
    assert ok.all()
    r, c = np.argwhere(~amb)[len(q) * 7]
    for step in (1, -1):
        bad = q.copy()
        bad[r, c] = int(q[r, c]) + step
        assert not G.rounded_within(bad, e, m)[0][r, c]


def test_rope_criterion_non_finite():
    """NaN exactly where float64 has it, +-Inf exactly where float64 has it."""
    e = np.array([np.nan, np.inf, -np.inf, 1.0, 1.0, 1.0])
    m = np.array([np.nan, np.inf, np.inf, 1.0, 1.0, 1.0])
    got = G.rne_bf16(np.array([np.nan, np.inf, -np.inf, 1.0, np.nan, np.inf]))
    np.testing.assert_array_equal(G.rounded_within(got, e, m)[0], [True, True, True, True, False, False])
    got = G.rne_bf16(np.array([1.0, -np.inf, np.nan, 1.0, 1.0, 1.0]))
    np.testing.assert_array_equal(G.rounded_within(got, e, m)[0], [False, False, False, True, True, True])


# ------------------------------------------------------------------------------------------------ column-sum finish
def _colsum_inputs(P, C, seed):
    rng = np.random.default_rng(seed)
    exact = rng.integers(-512, 513, (P, C)).astype(np.float32)
    rnd = (rng.standard_normal((P, C)) * np.exp(rng.standard_normal((P, C)))).astype(np.float32)
    return exact, rnd


@pytest.mark.parametrize("P,C", [(8, 33), (24, 40), (25, 31), (33, 32), (57, 40), (257, 33)])
def test_colsum_criteria_accept_kernel_and_reject_mutants(P, C):
    exact, rnd = _colsum_inputs(P, C, P * 100 + C)
    ref, _ = G.colsum_ref(exact)
    np.testing.assert_array_equal(G.colsum_kernel_f32(exact).astype(np.float64), ref)   # integers: any order is exact
    assert G.colsum_f32_ok(G.colsum_kernel_f32(rnd), rnd).all()
    for mutant in ("drop_last", "double", "skip_col"):
        assert not np.array_equal(G.colsum_kernel_f32(exact, mutant).astype(np.float64), ref), mutant
        ok = G.colsum_f32_ok(G.colsum_kernel_f32(rnd, mutant), rnd)
        assert (not ok[C - 1] and ok[:C - 1].all()) if mutant == "skip_col" else not ok.all(), mutant


def test_colsum_bound_is_100x_below_one_row():
    """The bound against the effect of one dropped row, |part[p, c]|, at the largest P used (the loosest bound): the median row
    is more than 100 bounds away."""
    P, C = 257, 3080
    _, rnd = _colsum_inputs(P, C, 1)
    _, mag = G.colsum_ref(rnd)
    bound = (P / 8 + 16) * 2.0 ** -24 * mag
    assert np.median(np.abs(rnd[-1]) / bound) > 100


# ------------------------------------------------------------------------------------------------ embedding gradient
def _embedding_inputs(V, H, T, seed):
    rng = np.random.default_rng(seed)
    grad = G.f32_to_bf16(rng.integers(-8, 9, (V, H)).astype(np.float32))
    dy = G.f32_to_bf16(rng.integers(-8, 9, (T, H)).astype(np.float32))
    ids = rng.integers(0, V, T)
    return grad, dy, ids


@pytest.mark.parametrize("alpha", [1.0, 0.5, -2.0])
def test_embedding_criteria_accept_kernel_and_reject_mutants(alpha):
    V, H, T, pad = 12, 2056, 40, 3
    grad, dy, ids = _embedding_inputs(V, H, T, 7)
    ids[:3] = pad
    ids[3:6] = (V, -1, 1 << 40)
    ref, touched = G.embedding_grad_ref(grad, dy, ids, alpha, pad)
    assert not touched[pad] and touched.sum() >= 8
    assert G.embedding_exact_ok(G.embedding_kernel_f32(grad, dy, ids, alpha, pad), ref).all()
    for mutant in ("lap2", "padding", "last_token"):
        ok = G.embedding_exact_ok(G.embedding_kernel_f32(grad, dy, ids, alpha, pad, mutant), ref)
        assert not ok.all(), mutant
        if mutant == "lap2":
            assert ok[:, :2048].all() and not ok[touched][:, 2048:].all()
        if mutant == "padding":
            assert ok[np.arange(V) != pad].all() and not ok[pad].all()


def test_embedding_ulp_criterion_on_random_values():
    rng = np.random.default_rng(3)
    V, H, T = 9, 264, 64
    grad = G.f32_to_bf16(rng.standard_normal((V, H)).astype(np.float32))
    dy = G.f32_to_bf16((rng.standard_normal((T, H)) * 0.7).astype(np.float32))
    ids = rng.integers(0, V, T)
    ref, _ = G.embedding_grad_ref(grad, dy, ids, 0.3, -1)
    assert G.embedding_ulp_ok(G.embedding_kernel_f32(grad, dy, ids, 0.3, -1), ref).all()
    assert not G.embedding_ulp_ok(G.embedding_kernel_f32(grad, dy, ids, 0.3, -1, "last_token"), ref).all()


# ------------------------------------------------------------------------------------------------ RMSNorm statistics
@pytest.mark.parametrize("cols", [8, 504, 520, 8192, 8200])
def test_rstd_criterion_accepts_kernel_and_rejects_mutants(cols):
    rng = np.random.default_rng(cols)
    x = G.f32_to_bf16((rng.standard_normal((5, cols)) * np.exp(rng.standard_normal((5, 1)))).astype(np.float32))
    x[3] = 0
    x[3, -1] = G.f32_to_bf16(np.float32(3.0))            # spike in the last element
    eps = 1e-5
    assert G.rstd_ok(G.rstd_kernel_f32(x, eps), x, eps).all()
    # the closed form of the spike row
    assert abs(G.rstd_ref(x, eps)[3] - 1.0 / np.sqrt(9.0 / cols + float(np.float32(eps)))) < 1e-12
    ok = G.rstd_ok(G.rstd_kernel_f32(x, eps, "skip_last_vec"), x, eps)
    assert not ok[3] and (cols > 520 or not ok.any())     # the spike row always; at few vectors every row
    assert not G.rstd_ok(G.rstd_kernel_f32(x, eps, "mean_cols+8"), x, eps).any()   # 5e-4 relative at cols = 8200: 50 x rtol


def test_rstd_criterion_degenerate_rows():
    cols = 16
    x = np.zeros((4, cols), dtype=np.uint16)
    x[1, 5] = 0x7F80                                       # Inf -> 0
    x[2, 0] = 0x7FC0                                       # NaN -> NaN
    x[3] = G.f32_to_bf16(np.float32(2.0))
    want = np.array([1.0 / np.sqrt(float(np.float32(1e-5))), 0.0, np.nan, 1.0 / np.sqrt(4.0 + float(np.float32(1e-5)))])
    np.testing.assert_allclose(G.rstd_ref(x, 1e-5), want, rtol=1e-15)
    assert G.rstd_ok(want.astype(np.float32), x, 1e-5).all()
    assert G.rstd_ref(x, 0.0)[0] == np.inf and G.rstd_ok(np.array([np.inf, 0, np.nan, 0.5], np.float32), x, 0.0).all()
    assert not G.rstd_ok(np.array([want[0], 1e-30, 0.0, want[3]], np.float32), x, 1e-5)[1:3].any()


def test_add_ref_is_the_float32_add():
    a = G.f32_to_bf16(np.array([[1.0, 3.0e38, 1.0, -0.0]], np.float32))
    b = G.f32_to_bf16(np.array([[2.0 ** -8, 3.0e38, 2.0 ** -9, 0.0]], np.float32))
    np.testing.assert_array_equal(G.add_ref(a, b), np.array([[0x3F80, 0x7F80, 0x3F80, 0x0000]], np.uint16))
    bias = G.f32_to_bf16(np.array([2.0 ** -8, 0, 2.0 ** -9, 0], np.float32))
    # (b + bias) first: 2^-8 + 2^-8 = 2^-7 then 1 + 2^-7 is a bf16 value
    np.testing.assert_array_equal(G.add_ref(a, b, bias)[0, [0, 2]], np.array([0x3F81, 0x3F80], np.uint16))
