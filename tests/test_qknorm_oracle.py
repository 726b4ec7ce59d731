"""CPU: the criteria of tests/qknorm_oracle.py are sound and sharp.  Each is fed the output of a numpy "kernel" that restates the
device arithmetic of mi_qknorm_rope_qkv / mi_qknorm_rope_qkv_bwd in float32 in the device's order -- it must accept it, at every
case and input scale, under the ambiguity caps -- and outputs that are wrong in one way each -- it must reject every one."""
import numpy as np
import pytest

from tests import glue_oracle as G
from tests import qknorm_oracle as Q

_ids = lambda c: "x".join(map(str, c))


def _forward_verdict(case, inp, out):
    """(everything ok, {tensor: (ambiguous, size)}) of a forward result (q, k, v, rstd) against float64."""
    B, S, nq, nkv, D, rows = case
    q, k, v, rstd = out
    ref = Q.forward_ref(inp, case)
    ok, amb = Q.forward_ok(np.concatenate([q, k], axis=1), ref, D)
    amb = amb.reshape(rows, -1)
    good = bool(ok.all()) and np.array_equal(v, ref["v"]) and bool(Q.rstd_ok(rstd, ref["rstd"], D).all())
    return good, {"q": (int(amb[:, :nq * D].sum()), rows * nq * D), "k": (int(amb[:, nq * D:].sum()), rows * nkv * D)}


def _backward_verdict(case, inp, rstd, n_partials, out):
    """(dx ok, dv copied, partials ok, ambiguous dx elements) of a backward result (dfused, partials) against float64 with the
    rstd the kernel was given."""
    B, S, nq, nkv, D, rows = case
    dfused, part = out
    H = nq + nkv
    ref = Q.backward_ref(inp, case, rstd)
    ok, amb = Q.dx_ok(dfused[:, :H * D], ref, D)
    part_ok = True
    for p, (lo, hi) in enumerate(Q.partial_rows(rows, n_partials)):
        e, bound = Q.gamma_sums(ref, case, lo, hi)
        part_ok &= bool(Q.gamma_ok(part[p], e, bound).all())
    e, bound = Q.gamma_sums(ref, case)
    part_ok &= bool(Q.gamma_ok(part.astype(np.float64).sum(0), e, bound).all())
    return bool(ok.all()), np.array_equal(dfused[:, H * D:], ref["dv"]), part_ok, int(amb.sum())


@pytest.mark.parametrize("scale", Q.QKNORM_SCALES + (2.0 ** -10,), ids=lambda s: f"scale{s:g}")
@pytest.mark.parametrize("case", Q.QKNORM_CASES, ids=_ids)
def test_criteria_accept_the_float32_kernels_and_cap_ambiguity(case, scale, capsys):
    """Forward and backward restatements pass at every case and input scale (2^-10 puts mean x^2 at the order of eps), and every
    compared tensor stays under its ambiguity cap."""
    B, S, nq, nkv, D, rows = case
    inp = Q.qknorm_case_inputs(case, scale)
    assert np.isnan(inp["cos"][S:]).all() and np.isfinite(inp["cos"][:S]).all()
    assert np.ptp(G.bf16_to_f64(inp["gamma_q"])) > 0.5 and np.ptp(G.bf16_to_f64(inp["gamma_k"])) > 0.5
    out = Q.forward_kernel_f32(inp, case)
    good, counts = _forward_verdict(case, inp, out)
    assert good
    for name, (a, n) in counts.items():
        assert a <= Q.forward_ambiguity_cap(n), f"{name}: {a} of {n} ambiguous: change the input, not the cap"
    n_partials = min(3, rows)
    dx_good, dv_good, part_good, a = _backward_verdict(case, inp, out[3], n_partials, Q.backward_kernel_f32(inp, case, out[3], n_partials))
    assert dx_good and dv_good and part_good
    n = rows * (nq + nkv) * D
    assert a <= Q.dx_ambiguity_cap(n), f"dx: {a} of {n} ambiguous: change the input, not the cap"
    with capsys.disabled():
        print(f"\n  qknorm {case} x{scale:g}: ambiguous " + ", ".join(f"{k} {a_}/{n_}" for k, (a_, n_) in counts.items()) + f", dx {a}/{n}", end="")


def _mutant_cases(mutant):
    """The cases in which a mutant computes something else: a norm after the rotation or a shifted position changes nothing in
    a sequence of one token (position 0 is the identity rotation)."""
    if mutant in ("norm_after_rope", "pos+1"):
        return [c for c in Q.QKNORM_CASES if c[1] > 1]
    return Q.QKNORM_CASES


@pytest.mark.parametrize("mutant", Q.FORWARD_MUTANTS)
def test_forward_criteria_reject_each_mutant(mutant):
    """Every forward mutant is refused in every case in which it computes something else.  eps left out is looked for where it
    matters: inputs scaled by 2^-10 put mean x^2 at the order of eps (at scale 1 its effect, 5e-7, is inside rho)."""
    scale = 2.0 ** -10 if mutant == "no_eps" else 1.0
    for case in _mutant_cases(mutant):
        inp = Q.qknorm_case_inputs(case, scale)
        if mutant == "pos+1":  # finite wrong table rows, so that the verdict comes from the values and not from a NaN
            inp["cos"], inp["sin"] = G.rope_tables(case[1], case[4], poison=False)
        good, _ = _forward_verdict(case, inp, Q.forward_kernel_f32(inp, case, mutant))
        assert not good, f"{mutant} accepted at {case}"


def test_forward_values_alone_reject_the_mutants_that_keep_rstd():
    """gamma_q for the k heads, the norm after the rotation and the neighbour's rstd leave v and the stored rstd right: it is the
    q / k interval test that has to catch them."""
    for mutant in ("gamma_q_for_k", "norm_after_rope", "rstd_neighbour"):
        for case in _mutant_cases(mutant):
            B, S, nq, nkv, D, rows = case
            inp = Q.qknorm_case_inputs(case)
            q, k, v, rstd = Q.forward_kernel_f32(inp, case, mutant)
            ref = Q.forward_ref(inp, case)
            assert Q.rstd_ok(rstd, ref["rstd"], D).all() and np.array_equal(v, ref["v"])
            assert not Q.forward_ok(np.concatenate([q, k], axis=1), ref, D)[0].all(), f"{mutant} accepted at {case}"


@pytest.mark.parametrize("case", Q.QKNORM_CASES, ids=_ids)
def test_gamma_criterion_rejects_a_missing_block(case):
    B, S, nq, nkv, D, rows = case
    inp = Q.qknorm_case_inputs(case)
    rstd = Q.forward_kernel_f32(inp, case)[3]
    n_partials = min(3, rows)
    dx_good, dv_good, part_good, _ = _backward_verdict(case, inp, rstd, n_partials,
                                                       Q.backward_kernel_f32(inp, case, rstd, n_partials, "drop_block"))
    assert dx_good and dv_good and not part_good


def test_dx_criterion_rejects_wrong_backward_inputs():
    """The backward restatement fed the forward mutants' view of the problem (gamma_q for the k heads, the neighbour's rstd, the
    position shifted by one) gives a dx the criterion refuses."""
    for case in [c for c in Q.QKNORM_CASES if c[1] > 1]:
        B, S, nq, nkv, D, rows = case
        inp = Q.qknorm_case_inputs(case)
        rstd = Q.forward_kernel_f32(inp, case)[3]
        n_partials = min(3, rows)
        wrong = dict(inp, gamma_k=inp["gamma_q"])
        assert not _backward_verdict(case, inp, rstd, n_partials, Q.backward_kernel_f32(wrong, case, rstd, n_partials))[0]
        assert not _backward_verdict(case, inp, rstd, n_partials, Q.backward_kernel_f32(inp, case, np.roll(rstd, -1, axis=1), n_partials))[0]
        cos, sin = G.rope_tables(S, D, poison=False)
        shifted = dict(inp, cos=np.roll(cos, -1, axis=0), sin=np.roll(sin, -1, axis=0))
        assert not _backward_verdict(case, inp, rstd, n_partials, Q.backward_kernel_f32(shifted, case, rstd, n_partials))[0]


def test_partial_rows_cover_every_row_once():
    for rows, n in ((1, 1), (1, 4), (29, 3), (80, 7), (2048, 512), (5, 8)):
        spans = Q.partial_rows(rows, n)
        assert len(spans) == n
        seen = [r for lo, hi in spans for r in range(lo, hi)]
        assert seen == list(range(rows))
