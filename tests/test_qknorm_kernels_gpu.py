"""GPU: mi_qknorm_rope_qkv / mi_qknorm_rope_qkv_bwd against the float64 references and criteria of tests/qknorm_oracle.py (whose
soundness tests/test_qknorm_oracle.py shows on the CPU).  The library is called through _lib.load() so that every output (q, k, v,
rstd, dfused, the gamma partials) sits in the middle of an allocation pre-filled with a sentinel (bf16 / fp32 NaN patterns, 64
elements on both sides): after the call the margins are unchanged and no sentinel is left inside.  Inputs that must not be read are
NaN inside the same allocation (table rows at or past `seq`, the elements after every input)."""
import numpy as np
import pytest
import torch

from tests import glue_oracle as G
from tests import qknorm_oracle as Q

pytestmark = pytest.mark.gpu

MARGIN = 64
_RAW = {torch.bfloat16: (torch.int16, 0x7FC0, np.uint16), torch.float32: (torch.int32, 0x7FC00000, np.uint32)}


class Guard:
    """A contiguous tensor `t` of `shape` in the middle of an allocation filled with the dtype's NaN sentinel, MARGIN elements (a
    multiple of 8: `t` stays 16-byte aligned) before and after it."""

    def __init__(self, shape, dtype, dev):
        self.n = int(np.prod(shape))
        self.raw_dtype, self.sentinel, self.np_raw = _RAW[dtype]
        self.buf = torch.empty(self.n + 2 * MARGIN, dtype=dtype, device=dev)
        self.buf.view(self.raw_dtype).fill_(self.sentinel)  # (both patterns are positive in the signed view)
        self.t = self.buf[MARGIN:MARGIN + self.n].view(shape)
        assert self.t.data_ptr() % 16 == 0

    def raw(self):
        return self.buf.view(self.raw_dtype).cpu().numpy().view(self.np_raw)

    def check(self, what):
        """Margins untouched, no sentinel left inside (no reference value of these tests is NaN)."""
        raw = self.raw()
        assert (raw[:MARGIN] == self.sentinel).all(), f"{what}: wrote before the output"
        assert (raw[MARGIN + self.n:] == self.sentinel).all(), f"{what}: wrote past the output"
        left = raw[MARGIN:MARGIN + self.n] == self.sentinel
        assert not left.any(), f"{what}: {int(left.sum())} elements never written"

    def bits(self):
        return self.raw()[MARGIN:MARGIN + self.n].reshape(self.t.shape)

    def f32(self):
        return self.t.cpu().numpy()


def _bf16_in(bits, dev):
    """bf16 input on the device followed, inside the same allocation, by MARGIN NaN elements that must not be read."""
    bits = np.ascontiguousarray(bits, dtype=np.uint16)
    buf = torch.empty(bits.size + MARGIN, dtype=torch.int16, device=dev)
    buf.fill_(0x7FC0)
    buf[:bits.size] = torch.from_numpy(bits.reshape(-1).view(np.int16)).to(dev)
    return buf.view(torch.bfloat16)[:bits.size].view(bits.shape)


def _f32_in(a, dev):
    a = np.ascontiguousarray(a, dtype=np.float32)
    buf = torch.full((a.size + MARGIN,), float("nan"), dtype=torch.float32, device=dev)
    buf[:a.size] = torch.from_numpy(a.reshape(-1)).to(dev)
    return buf[:a.size].view(a.shape)


def _run(dev, case, inp, n_partials, backward_twice=False):
    """One forward and one (or two) backward launches of a case into guarded outputs."""
    from llm_fp8_amd import _lib as L
    lib = L.load()
    assert lib.mi_device_supported() == 1, "not a gfx950 device"
    B, S, nq, nkv, D, rows = case
    W, H = (nq + 2 * nkv) * D, nq + nkv
    st = torch.cuda.current_stream().cuda_stream
    cos, sin = _f32_in(inp["cos"], dev), _f32_in(inp["sin"], dev)
    assert cos.shape == (S + G.ROPE_TABLE_PAD, D // 2) and torch.isnan(cos[S:]).all() and torch.isnan(sin[S:]).all()
    qkv, gq, gk = _bf16_in(inp["qkv"], dev), _bf16_in(inp["gamma_q"], dev), _bf16_in(inp["gamma_k"], dev)
    q, k, v = (Guard((rows, n * D), torch.bfloat16, dev) for n in (nq, nkv, nkv))
    rstd = Guard((rows, H), torch.float32, dev)
    L.check(lib.mi_qknorm_rope_qkv(qkv.data_ptr(), q.t.data_ptr(), k.t.data_ptr(), v.t.data_ptr(), gq.data_ptr(), gk.data_ptr(),
                                   rstd.t.data_ptr(), cos.data_ptr(), sin.data_ptr(), rows, S, nq, nkv, D, float(inp["eps"]), st),
            "mi_qknorm_rope_qkv")
    dq, dk, dv = (_bf16_in(inp[n], dev) for n in ("dq", "dk", "dv"))
    outs = []
    for _ in range(2 if backward_twice else 1):
        dfused = Guard((rows, W), torch.bfloat16, dev)
        part = Guard((n_partials, 2 * D), torch.float32, dev)
        L.check(lib.mi_qknorm_rope_qkv_bwd(dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), qkv.data_ptr(), rstd.t.data_ptr(),
                                           gq.data_ptr(), gk.data_ptr(), cos.data_ptr(), sin.data_ptr(), dfused.t.data_ptr(),
                                           part.t.data_ptr(), n_partials, rows, S, nq, nkv, D, st), "mi_qknorm_rope_qkv_bwd")
        outs.append((dfused, part))
    torch.cuda.synchronize()
    return dict(q=q, k=k, v=v, rstd=rstd, back=outs)


def _check_case(case, inp, res, n_partials, report):
    B, S, nq, nkv, D, rows = case
    H = nq + nkv
    for name in ("q", "k", "v", "rstd"):
        res[name].check(f"{name} {case}")
    ref = Q.forward_ref(inp, case)
    got = np.concatenate([res["q"].bits(), res["k"].bits()], axis=1)
    ok, amb = Q.forward_ok(got, ref, D)
    assert ok.all(), f"forward {case}: {int((~ok).sum())} of {ok.size} elements outside the rounding interval, first at {np.argwhere(~ok)[0]}"
    amb = amb.reshape(rows, -1)
    for name, a, n in (("q", int(amb[:, :nq * D].sum()), rows * nq * D), ("k", int(amb[:, nq * D:].sum()), rows * nkv * D)):
        report.append(f"{name} {a}/{n}")
        assert a <= Q.forward_ambiguity_cap(n), f"{name} {case}: {a} of {n} elements ambiguous"
    assert np.array_equal(res["v"].bits(), ref["v"]), f"v {case}: not a bitwise copy"
    rstd = res["rstd"].f32()
    assert Q.rstd_ok(rstd, ref["rstd"], D).all(), f"rstd {case}"
    # backward: the reference takes the rstd the kernel was given (its own forward's)
    refb = Q.backward_ref(inp, case, rstd)
    dfused, part = res["back"][0]
    dfused.check(f"dfused {case}")
    part.check(f"partials {case}")
    okd, ambd = Q.dx_ok(dfused.bits()[:, :H * D], refb, D)
    assert okd.all(), f"dx {case}: {int((~okd).sum())} of {okd.size} elements outside the rounding interval, first at {np.argwhere(~okd)[0]}"
    a, n = int(ambd.sum()), rows * H * D
    report.append(f"dx {a}/{n}")
    assert a <= Q.dx_ambiguity_cap(n), f"dx {case}: {a} of {n} elements ambiguous"
    assert np.array_equal(dfused.bits()[:, H * D:], refb["dv"]), f"dv {case}: not a bitwise copy"
    p = part.f32()
    for i, (lo, hi) in enumerate(Q.partial_rows(rows, n_partials)):
        e, bound = Q.gamma_sums(refb, case, lo, hi)
        assert Q.gamma_ok(p[i], e, bound).all(), f"gamma partial {i} {case}"
    return refb


@pytest.mark.parametrize("case", Q.QKNORM_CASES, ids=lambda c: "x".join(map(str, c)))
def test_forward_and_backward_against_float64(dev, case):
    B, S, nq, nkv, D, rows = case
    inp = Q.qknorm_case_inputs(case)
    n_partials = min(3, rows)
    report = []
    res = _run(dev, case, inp, n_partials, backward_twice=True)
    _check_case(case, inp, res, n_partials, report)
    (d1, p1), (d2, p2) = res["back"]
    assert np.array_equal(d1.raw(), d2.raw()) and np.array_equal(p1.raw(), p2.raw()), "two backward runs differ"
    print(f"qknorm {case}: ambiguous " + ", ".join(report))


def test_small_inputs_where_eps_matters(dev):
    """Inputs scaled by 2^-10: mean x^2 is of the order of eps, which a kernel that leaves eps out cannot hide."""
    case = Q.QKNORM_CASES[2]
    inp = Q.qknorm_case_inputs(case, 2.0 ** -10)
    report = []
    _check_case(case, inp, _run(dev, case, inp, 3), 3, report)
    print(f"qknorm {case} x2^-10: ambiguous " + ", ".join(report))


def test_more_partials_than_rows(dev):
    """Workgroups that own no row write zeros."""
    case = Q.QKNORM_CASES[1]
    inp = Q.qknorm_case_inputs(case)
    res = _run(dev, case, inp, 40)
    _check_case(case, inp, res, 40, [])
    p = res["back"][0][1].f32()
    assert (p[21:] == 0).all()


def test_the_4b_head_counts_and_the_finished_gamma_sums(dev):
    """(4, 512, 32, 8, 128, 2048): 917504 items, the 4B head counts; the partials of 512 workgroups finished by mi_colsum_finish
    are held to the float64 gamma sums under the bound of a sum of rows * heads addends in any order."""
    from llm_fp8_amd import _lib as L
    case = Q.QKNORM_BIG_CASE
    B, S, nq, nkv, D, rows = case
    inp = Q.qknorm_case_inputs(case)
    report = []
    res = _run(dev, case, inp, 512)
    refb = _check_case(case, inp, res, 512, report)
    part = res["back"][0][1]
    out = Guard((2 * D,), torch.float32, dev)
    L.check(L.load().mi_colsum_finish(part.t.data_ptr(), 512, 2 * D, out.t.data_ptr(), 1, torch.cuda.current_stream().cuda_stream),
            "mi_colsum_finish")
    torch.cuda.synchronize()
    out.check("finished gamma sums")
    e, bound = Q.gamma_sums(refb, case)
    assert Q.gamma_ok(out.f32(), e, bound).all()
    print(f"qknorm {case}: ambiguous " + ", ".join(report))


def test_ops_wrappers_match_the_entry_points(dev):
    """ops.qknorm_rope_qkv_forward / _backward: the same bits as the raw calls, gamma gradients = mi_colsum_finish of the partials."""
    from llm_fp8_amd.pytorch import ops
    case = Q.QKNORM_CASES[4]
    B, S, nq, nkv, D, rows = case
    inp = Q.qknorm_case_inputs(case)
    t = lambda n: torch.from_numpy(inp[n].view(np.int16)).to(dev).view(torch.bfloat16)
    cos, sin = (torch.from_numpy(np.ascontiguousarray(inp[n][:S])).to(dev) for n in ("cos", "sin"))
    q, k, v, rstd = ops.qknorm_rope_qkv_forward(t("qkv"), t("gamma_q"), t("gamma_k"), cos, sin, nq, nkv, D, S, float(inp["eps"]))
    n_partials = max(1, min(1024, (rows + 3) // 4))
    res = _run(dev, case, inp, n_partials)
    bits = lambda x: x.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)
    assert np.array_equal(bits(q), res["q"].bits()) and np.array_equal(bits(k), res["k"].bits()) and np.array_equal(bits(v), res["v"].bits())
    assert np.array_equal(rstd.cpu().numpy(), res["rstd"].f32())
    g, dgq, dgk = ops.qknorm_rope_qkv_backward(t("dq"), t("dk"), t("dv"), t("qkv"), rstd, t("gamma_q"), t("gamma_k"), cos, sin, nq, nkv, D, S)
    assert np.array_equal(bits(g), res["back"][0][0].bits())
    e, bound = Q.gamma_sums(Q.backward_ref(inp, case, rstd.cpu().numpy()), case)
    assert Q.gamma_ok(torch.cat([dgq, dgk]).cpu().numpy(), e, bound).all()
