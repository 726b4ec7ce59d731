"""GPU: the small HBM-bound kernels between the GEMMs against the float64 references and criteria of tests/glue_oracle.py (whose
soundness tests/test_glue_oracle.py shows on the CPU): RoPE split / merge with the kernel's own tables, the two fused RoPE-backward
casts against the two-kernel sequence, mi_embedding_grad_add, mi_colsum_finish(_multi), the three RMSNorm-statistics entry points,
mi_sumsq_bf16(_multi) and mi_adamw_bf16.  The library is called through _lib.load() so that every output can sit in the middle of
an allocation pre-filled with a sentinel (bf16 NaN, fp32 / fp64 NaN, 0xA5 bytes; at least 64 elements on both sides): after the
call the margins are unchanged and no sentinel is left inside.  Inputs that must not be read are NaN inside the same allocation
(table rows at or past `seq`, the elements after the last row).  Nothing is read or written outside an allocation."""
import ctypes
import math

import numpy as np
import pytest
import torch

from oracle import fp8_oracle as O
from tests import glue_oracle as G

pytestmark = pytest.mark.gpu

MARGIN = 64
_RAW = {torch.bfloat16: (torch.int16, 0x7FC0), torch.float32: (torch.int32, 0x7FC00000),
        torch.float64: (torch.int64, 0x7FF8000000000000), torch.uint8: (torch.uint8, 0xA5)}


@pytest.fixture(scope="module")
def ops(dev):
    from llm_fp8_amd.pytorch import ops as _ops
    from llm_fp8_amd import _lib
    assert _lib.load().mi_device_supported() == 1, "not a gfx950 device"
    return _ops


def _L():
    from llm_fp8_amd import _lib as L
    return L


def _st():
    return torch.cuda.current_stream().cuda_stream


class Guard:
    """A contiguous tensor `t` of `shape` in the middle of an allocation filled with the dtype's sentinel, `margin` elements (a
    multiple of 8, at least 64: `t` stays 16-byte aligned) before and after it."""

    def __init__(self, shape, dtype, dev, margin=MARGIN):
        assert margin >= MARGIN and margin % 8 == 0
        self.n, self.margin = int(np.prod(shape)), margin
        self.raw_dtype, self.sentinel = _RAW[dtype]
        self.buf = torch.empty(self.n + 2 * margin, dtype=dtype, device=dev)
        self.buf.view(self.raw_dtype).fill_(self.sentinel)
        self.t = self.buf[margin:margin + self.n].view(shape)
        assert self.t.data_ptr() % 16 == 0

    def ptr(self):
        return self.t.data_ptr()

    def check(self, what, allow=None):
        """Margins untouched; no sentinel inside, except where `allow` (bool numpy array of the output's shape: positions where
        the reference itself is NaN) says so.  FP8 bytes have no spare pattern: there the bitwise comparison with the separately
        allocated reference is what shows that every byte was written."""
        raw = self.buf.view(self.raw_dtype).cpu().numpy()
        m, n = self.margin, self.n
        assert (raw[:m] == raw.dtype.type(self.sentinel)).all(), f"{what}: wrote before the output"
        assert (raw[m + n:] == raw.dtype.type(self.sentinel)).all(), f"{what}: wrote past the output"
        if self.raw_dtype != torch.uint8:
            left = raw[m:m + n] == raw.dtype.type(self.sentinel)
            if allow is not None:
                left &= ~np.asarray(allow).reshape(-1)
            assert not left.any(), f"{what}: {int(left.sum())} elements never written"

    def bits(self):
        return self.t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def _bf16_in(bits, dev, tail=MARGIN):
    """bf16 input on the device followed, inside the same allocation, by `tail` NaN elements that must not be read."""
    bits = np.ascontiguousarray(bits, dtype=np.uint16)
    buf = torch.empty(bits.size + tail, dtype=torch.int16, device=dev)
    buf.fill_(0x7FC0)
    buf[:bits.size] = torch.from_numpy(bits.reshape(-1).view(np.int16)).to(dev)
    return buf.view(torch.bfloat16)[:bits.size].view(bits.shape)


def _f32_in(a, dev, tail=MARGIN):
    a = np.ascontiguousarray(a, dtype=np.float32)
    buf = torch.full((a.size + tail,), float("nan"), dtype=torch.float32, device=dev)
    buf[:a.size] = torch.from_numpy(a.reshape(-1)).to(dev)
    return buf[:a.size].view(a.shape)


def _int_bits(rng, shape, lim=8):
    return G.f32_to_bf16(rng.integers(-lim, lim + 1, shape).astype(np.float32))


def _normal_bits(rng, shape, scale=1.0):
    return G.f32_to_bf16((rng.standard_normal(shape) * scale).astype(np.float32))


# ================================================================================================ 1: RoPE split / merge
def _rope(fused, q, k, v, cos, sin, rows, S, nq, nkv, D, backward):
    L = _L()
    L.check(L.load().mi_rope_qkv(fused.data_ptr(), q.data_ptr(), k.data_ptr(), v.data_ptr(), cos.data_ptr(), sin.data_ptr(), rows, S,
                                 nq, nkv, D, int(backward), _st()), "mi_rope_qkv")


def _check_rotated(got_bits, src_bits, cos_h, sin_h, S, D, backward, what, report):
    e, m = G.rope_ref(src_bits, cos_h, sin_h, S, D, backward)
    ok, amb = G.rounded_within(got_bits, e, m)
    assert ok.all(), f"{what}: {int((~ok).sum())} of {ok.size} elements outside the rounding interval, first at {np.argwhere(~ok)[0]}"
    n_amb = int(amb.sum())
    report.append(f"{what} {n_amb}/{amb.size}")
    assert n_amb <= G.rope_ambiguity_cap(amb.size), f"{what}: {n_amb} of {amb.size} elements ambiguous"
    return e


def _rope_roundtrip(ops, dev, case, inp, report):
    """Forward and backward launches of one case into guarded outputs; returns everything the callers compare."""
    B, S, nq, nkv, D, rows = case
    W = (nq + 2 * nkv) * D
    cos, sin = torch.from_numpy(inp["cos"]).to(dev), torch.from_numpy(inp["sin"]).to(dev)
    assert cos.shape == (S + G.ROPE_TABLE_PAD, D // 2) and torch.isnan(cos[S:]).all() and torch.isnan(sin[S:]).all()
    cos_h, sin_h = cos.cpu().numpy(), sin.cpu().numpy()   # the reference uses the tables the kernel reads
    qkv = _bf16_in(inp["qkv"], dev)
    q, k, v = (Guard((rows, n * D), torch.bfloat16, dev) for n in (nq, nkv, nkv))
    _rope(qkv, q.t, k.t, v.t, cos, sin, rows, S, nq, nkv, D, False)
    dq, dk, dv = (_bf16_in(inp[n], dev) for n in ("dq", "dk", "dv"))
    back = Guard((rows, W), torch.bfloat16, dev)
    _rope(back.t, dq, dk, dv, cos, sin, rows, S, nq, nkv, D, True)
    torch.cuda.synchronize()
    return dict(cos=cos, sin=sin, cos_h=cos_h, sin_h=sin_h, qkv=qkv, q=q, k=k, v=v, dq=dq, dk=dk, dv=dv, back=back)


@pytest.mark.parametrize("case", G.ROPE_CASES, ids=lambda c: "x".join(map(str, c)))
def test_rope_split_and_merge_vs_float64(ops, dev, case, capsys):
    """Every rotated element inside [RNE_bf16(e - delta), RNE_bf16(e + delta)] of its float64 value e (glue_oracle.rounded_within),
    with at most max(2, 0.2 %) of a tensor where that interval holds two bf16 values; v bit-identical; seq 1, one vector pair
    per head, head_dim up to 256, a partial last sequence; NaN table rows at and past seq."""
    B, S, nq, nkv, D, rows = case
    inp = G.rope_case_inputs(case)
    report = []
    r = _rope_roundtrip(ops, dev, case, inp, report)
    a, b = nq * D, (nq + nkv) * D
    eq = _check_rotated(r["q"].bits(), inp["qkv"][:, :a], r["cos_h"], r["sin_h"], S, D, False, "q", report)
    ek = _check_rotated(r["k"].bits(), inp["qkv"][:, a:b], r["cos_h"], r["sin_h"], S, D, False, "k", report)
    np.testing.assert_array_equal(r["v"].bits(), inp["qkv"][:, b:])
    back = r["back"].bits()
    _check_rotated(back[:, :a], inp["dq"], r["cos_h"], r["sin_h"], S, D, True, "dq", report)
    _check_rotated(back[:, a:b], inp["dk"], r["cos_h"], r["sin_h"], S, D, True, "dk", report)
    np.testing.assert_array_equal(back[:, b:], inp["dv"])
    assert np.isfinite(eq).all() and np.isfinite(ek).all()
    for name in ("q", "k", "v", "back"):
        r[name].check(f"{case} {name}")
    # the same launches through the ops wrappers
    wq, wk, wv = ops.rope_qkv_forward(r["qkv"], r["cos"], r["sin"], nq, nkv, D, S)
    assert torch.equal(wq, r["q"].t) and torch.equal(wk, r["k"].t) and torch.equal(wv, r["v"].t)
    assert torch.equal(ops.rope_qkv_backward(r["dq"], r["dk"], r["dv"], r["cos"], r["sin"], nq, nkv, D, S), r["back"].t)
    with capsys.disabled():
        print(f"\n  ROPE-AMBIGUOUS {case}: " + ", ".join(report), end="")


def test_rope_non_finite_inputs(ops, dev):
    """A NaN in x1 of one head makes exactly that element and its partner at + D / 2 NaN; an Inf at position 0 (sin = 0, cos = 1)
    gives Inf in its own half and NaN (Inf * 0) in the partner half -- what float64 gives."""
    case = G.ROPE_CASES[3]
    B, S, nq, nkv, D, rows = case
    inp = G.rope_case_inputs(case)
    a = nq * D
    nan_at, inf_at = (5, 2 * D + 7), (0, a + 1 * D + 3)        # q head 2, row 5; k head 1, row 0 (position 0)
    inp["qkv"] = inp["qkv"].copy()
    inp["qkv"][nan_at] = 0x7FC0
    inp["qkv"][inf_at] = 0x7F80
    inp["dq"] = inp["dq"].copy()
    inp["dq"][nan_at] = 0x7FC0
    inp["dk"] = inp["dk"].copy()
    inp["dk"][inf_at[0], inf_at[1] - a] = 0xFF80               # -Inf on the way back
    report = []
    r = _rope_roundtrip(ops, dev, case, inp, report)
    b = (nq + nkv) * D
    want_nan = {(nan_at[0], nan_at[1]), (nan_at[0], nan_at[1] + D // 2), (inf_at[0], inf_at[1] + D // 2)}
    fwd = np.concatenate([r["q"].bits(), r["k"].bits()], axis=1)
    bwd = r["back"].bits()[:, :b]
    for got, srcs, backward, inf_bits in ((fwd, (inp["qkv"][:, :a], inp["qkv"][:, a:b]), False, 0x7F80),
                                          (bwd, (inp["dq"], inp["dk"]), True, 0xFF80)):
        e = np.concatenate([_check_rotated(got[:, lo:hi], s, r["cos_h"], r["sin_h"], S, D, backward, "non-finite", report)
                            for (lo, hi), s in zip(((0, a), (a, b)), srcs)], axis=1)
        gf = G.bf16_to_f64(got)
        assert {tuple(p) for p in np.argwhere(np.isnan(gf))} == want_nan == {tuple(p) for p in np.argwhere(np.isnan(e))}
        assert {tuple(p) for p in np.argwhere(np.isinf(gf))} == {inf_at} and got[inf_at] == inf_bits
    allow = np.zeros((rows, (nq + 2 * nkv) * D), dtype=bool)
    for p in want_nan:
        allow[p] = True
    r["q"].check("q", allow[:, :a])
    r["k"].check("k", allow[:, a:b])
    r["back"].check("back", allow)


# ================================================================================================ 2: fused RoPE-backward casts
def _cast_inputs(rows, S, nq, nkv, dev, seed):
    D = 128
    rng = np.random.default_rng(seed)
    dq = _normal_bits(rng, (rows, nq * D), 0.3)
    dk = _normal_bits(rng, (rows, nkv * D), 3.0)
    dv = _normal_bits(rng, (rows, nkv * D))
    cos_h, sin_h = G.rope_tables(S, D)
    return dq, dk, dv, torch.from_numpy(cos_h).to(dev), torch.from_numpy(sin_h).to(dev)


def _unfused_backward(dq, dk, dv, cos, sin, rows, S, nq, nkv, dev):
    D = 128
    ref = Guard((rows, (nq + 2 * nkv) * D), torch.bfloat16, dev)
    _rope(ref.t, dq, dk, dv, cos, sin, rows, S, nq, nkv, D, True)
    return ref


def _fused_cast(dq, dk, dv, cos, sin, y, yT, scale, amax, rows, S, nq, nkv, fmt):
    L = _L()
    p = lambda t: None if t is None else t.data_ptr()
    L.check(L.load().mi_rope_qkv_bwd_cast(dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), cos.data_ptr(), sin.data_ptr(), p(y), p(yT),
                                          scale.data_ptr(), p(amax), rows, S, nq, nkv, 128, fmt, _st()), "mi_rope_qkv_bwd_cast")


@pytest.mark.parametrize("fmt", [O.E4M3, O.E5M2])
@pytest.mark.parametrize("rows,S,nq,nkv", [(8, 8, 1, 1), (72, 12, 3, 1), (136, 17, 2, 2), (200, 25, 5, 1), (40, 12, 3, 1)])
def test_rope_bwd_cast_is_the_two_kernel_sequence(ops, dev, rows, S, nq, nkv, fmt):
    """mi_rope_qkv_bwd_cast == mi_rope_qkv(backward) (held to float64 above) + mi_cast_amax, bytes and amax: one 8-row block; 6 units
    per 64-row block, so a workgroup's four waves straddle two row blocks (72 rows) or the last workgroup is half empty (40 rows);
    positions that change inside a lane's 8 rows; y only, yT only and both; amax absent, already larger, and zero."""
    W = (nq + 2 * nkv) * 128
    dq_b, dk_b, dv_b, cos, sin = _cast_inputs(rows, S, nq, nkv, dev, rows + fmt)
    dq, dk, dv = (_bf16_in(x, dev) for x in (dq_b, dk_b, dv_b))
    scale = torch.tensor([37.0], device=dev)
    ref = _unfused_backward(dq, dk, dv, cos, sin, rows, S, nq, nkv, dev)
    a_ref = torch.zeros(1, device=dev)
    y_ref, t_ref = ops.cast_amax(ref.t, scale, a_ref, fmt)
    ref.check("unfused d(qkv)")
    for want_y, want_t, amax0 in ((True, True, 0.0), (True, False, None), (False, True, 1e9)):
        y = Guard((rows, W), torch.uint8, dev) if want_y else None
        yT = Guard((W, rows), torch.uint8, dev) if want_t else None
        amax = Guard((1,), torch.float32, dev) if amax0 is not None else None
        if amax is not None:
            amax.t.fill_(amax0)
        _fused_cast(dq, dk, dv, cos, sin, y and y.t, yT and yT.t, scale, amax and amax.t, rows, S, nq, nkv, fmt)
        torch.cuda.synchronize()
        what = f"y {want_y} yT {want_t} amax {amax0}"
        if y is not None:
            assert torch.equal(y.t, y_ref), what
            y.check(what)
        if yT is not None:
            assert torch.equal(yT.t, t_ref), what
            yT.check(what)
        if amax is not None:
            assert amax.t.item() == (a_ref.item() if amax0 == 0.0 else np.float32(1e9)) and a_ref.item() > 0, what
            amax.check(what)
    assert int((y_ref != 0).sum()) > rows * W // 2  # the comparison is not vacuous


@pytest.mark.parametrize("fmt", [O.E4M3, O.E5M2])
def test_rope_bwd_cast_amax_ignores_nan_and_takes_inf(ops, dev, fmt):
    rows, S, nq, nkv = 136, 17, 2, 2
    W = (nq + 2 * nkv) * 128
    dq_b, dk_b, dv_b, cos, sin = _cast_inputs(rows, S, nq, nkv, dev, 5)
    dq_b[9, 130] = 0x7FC0
    scale = torch.tensor([37.0], device=dev)
    for with_inf in (False, True):
        if with_inf:
            dv_b[77, 5] = 0x7F80
        dq, dk, dv = (_bf16_in(x, dev) for x in (dq_b, dk_b, dv_b))
        ref = _unfused_backward(dq, dk, dv, cos, sin, rows, S, nq, nkv, dev)
        a_ref = torch.zeros(1, device=dev)
        y_ref, t_ref = ops.cast_amax(ref.t, scale, a_ref, fmt)
        y, yT, amax = Guard((rows, W), torch.uint8, dev), Guard((W, rows), torch.uint8, dev), Guard((1,), torch.float32, dev)
        amax.t.fill_(0.0)
        _fused_cast(dq, dk, dv, cos, sin, y.t, yT.t, scale, amax.t, rows, S, nq, nkv, fmt)
        torch.cuda.synchronize()
        assert torch.equal(y.t, y_ref) and torch.equal(yT.t, t_ref)
        back = G.bf16_to_f64(ref.bits())
        assert np.isnan(back).sum() == 2                                  # the NaN and its partner half
        want = np.nanmax(np.abs(back))
        assert amax.t.item() == want == a_ref.item() and np.isinf(want) == with_inf
        for g_ in (y, yT, amax):
            g_.check(f"inf {with_inf}")


@pytest.mark.parametrize("nq,nkv", [(1, 1), (3, 1), (4, 4)])
@pytest.mark.parametrize("rows,S", [(32, 16), (96, 12), (160, 40)])
def test_mxfp8_rope_bwd_quantize_is_the_two_kernel_sequence(ops, dev, rows, S, nq, nkv):
    """mi_mxfp8_rope_bwd_quantize == mi_rope_qkv(backward) + mi_mxfp8_quantize, data and E8M0 scales: row-only, column-only and
    both, both formats; row counts below, at and beside the 128-row tile; a NaN planted in dq."""
    L = _L()
    D, W = 128, (nq + 2 * nkv) * 128
    dq_b, dk_b, dv_b, cos, sin = _cast_inputs(rows, S, nq, nkv, dev, rows * 10 + nq)
    dq_b[1, 5] = 0x7FC0
    dq, dk, dv = (_bf16_in(x, dev) for x in (dq_b, dk_b, dv_b))
    ref = _unfused_backward(dq, dk, dv, cos, sin, rows, S, nq, nkv, dev)
    shapes = ((rows, W), (W // 32, rows), (W, rows), (rows // 32, W))
    for fmt in (O.E4M3, O.E5M2):
        want = ops.mxfp8_quantize(ref.t, fmt)
        for rowwise, colwise in ((True, True), (True, False), (False, True)):
            outs = [Guard(s, torch.uint8, dev) if use else None for s, use in zip(shapes, (rowwise, rowwise, colwise, colwise))]
            ptrs = [None if o is None else o.ptr() for o in outs]
            L.check(L.load().mi_mxfp8_rope_bwd_quantize(dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), cos.data_ptr(), sin.data_ptr(),
                                                        *ptrs, rows, S, nq, nkv, D, fmt, _st()), "mi_mxfp8_rope_bwd_quantize")
            torch.cuda.synchronize()
            for o, w, name in zip(outs, want, ("y_row", "s_row", "y_colT", "s_colT")):
                if o is not None:
                    assert torch.equal(o.t, w), f"fmt {fmt} rowwise {rowwise} colwise {colwise}: {name}"
                    o.check(name)
    ref.check("unfused d(qkv)", allow=np.isnan(G.bf16_to_f64(ref.bits())))


# ================================================================================================ 3: embedding gradient
def _embedding_call(grad, dy, ids, alpha, padding_idx):
    """The wrapper's launch with caller-owned buffers: ids sorted (stable) on the device."""
    L = _L()
    sorted_ids, perm = torch.sort(ids.reshape(-1), stable=True)
    V, H = grad.shape
    L.check(L.load().mi_embedding_grad_add(grad.data_ptr(), dy.data_ptr(), sorted_ids.data_ptr(), perm.data_ptr(), ids.numel(), H, V,
                                           float(alpha), int(padding_idx), _st()), "mi_embedding_grad_add")


def _embedding_run(dev, grad_b, dy_b, ids, alpha, padding_idx, call=None):
    """Two runs from the same state into a guarded grad (a sentinel row and more after it): (bits, reference, touched rows)."""
    V, H = grad_b.shape
    runs = []
    for _ in range(2):
        g_ = Guard((V, H), torch.bfloat16, dev, margin=max(MARGIN, H))
        g_.t.copy_(torch.from_numpy(grad_b.view(np.int16)).to(dev).view(torch.bfloat16))
        dy = _bf16_in(dy_b, dev)
        idt = torch.from_numpy(np.asarray(ids, dtype=np.int64)).to(dev)
        (call or _embedding_call)(g_.t, dy, idt, alpha, padding_idx)
        torch.cuda.synchronize()
        g_.check("grad")
        runs.append(g_.bits())
    np.testing.assert_array_equal(runs[0], runs[1])
    ref, touched = G.embedding_grad_ref(grad_b, dy_b, ids, alpha, padding_idx)
    np.testing.assert_array_equal(runs[0][~touched], grad_b[~touched])
    return runs[0], ref, touched


@pytest.mark.parametrize("alpha", [1.0, 0.5, -2.0, 0.0])
@pytest.mark.parametrize("H", [8, 264, 2048, 2056, 4104])
def test_embedding_grad_add_exact(dev, H, alpha):
    """Small-integer dy and grad: the result is RNE_bf16 of the exact value whatever the order, so bit equality is required.  H = 8
    (one lane), 264, 2048 (every lane one lap), 2056 (one lane on its second lap), 4104 (two laps and a third lane-0 lap); ids hold
    0, V - 1 and the out-of-range V, -1, -5, 2^40; padding_idx is an id that occurs."""
    V, T = 24, 48
    rng = np.random.default_rng(H)
    grad_b, dy_b = _int_bits(rng, (V, H)), _int_bits(rng, (T, H))
    ids = rng.integers(0, V, T)
    ids[:9] = (0, V - 1, V, -1, -5, 1 << 40, V - 1, 5, 5)
    pad = 5
    got, ref, touched = _embedding_run(dev, grad_b, dy_b, ids, alpha, pad)
    assert touched[0] and touched[V - 1] and not touched[pad] and 8 <= touched.sum() < V
    ok = G.embedding_exact_ok(got, ref)
    assert ok.all(), f"{int((~ok).sum())} elements differ, first at {np.argwhere(~ok)[0]}"


@pytest.mark.parametrize("pattern", ["one_token", "one_run_of_3000", "distinct_descending", "wrapper_2d_ids_strided_dy"])
def test_embedding_grad_add_id_patterns(ops, dev, pattern):
    rng = np.random.default_rng(len(pattern))
    call, alpha, pad = None, 0.5, -1
    if pattern == "one_token":
        V, H, ids = 5, 2056, np.array([3])
    elif pattern == "one_run_of_3000":        # one workgroup sums 3000 rows (|sum| <= 24000: exact), the other 2999 return
        V, H, ids = 300, 264, np.full(3000, 7)
    elif pattern == "distinct_descending":
        V, H, ids = 50, 264, 49 - np.arange(40)
    else:                                      # ids [B, S] and dy a non-contiguous view: the wrapper flattens and copies
        V, H, ids = 30, 264, rng.integers(0, 30, (4, 9))
        call = lambda g_, dy, idt, a, p: ops.embedding_grad_add_(g_, dy, idt, alpha=a, padding_idx=p)
    T = ids.size
    grad_b, dy_b = _int_bits(rng, (V, H)), _int_bits(rng, (T, H))
    if call is not None:
        wide = np.concatenate([dy_b, _int_bits(rng, (T, 8))], axis=1)
        inner = call
        call = lambda g_, dy, idt, a, p: inner(g_, _bf16_in(wide, dev)[:, :H].view(4, 9, H), idt, a, p)
    got, ref, touched = _embedding_run(dev, grad_b, dy_b, ids, alpha, pad, call)
    assert touched.sum() == len(np.unique(ids))
    assert G.embedding_exact_ok(got, ref).all()


def test_embedding_grad_add_random_within_one_ulp(dev):
    """N(0, 0.7) dy, alpha = 0.3, 40 runs of 25 tokens: within one bf16 ulp of float64."""
    V, H, T = 64, 2056, 1000
    rng = np.random.default_rng(12)
    grad_b, dy_b = _normal_bits(rng, (V, H)), _normal_bits(rng, (T, H), 0.7)
    ids = rng.permutation(np.arange(T) % 40)
    got, ref, touched = _embedding_run(dev, grad_b, dy_b, ids, 0.3, -1)
    assert touched.sum() == 40
    ok = G.embedding_ulp_ok(got, ref)
    assert ok.all(), f"{int((~ok).sum())} elements beyond one bf16 ulp"


# ================================================================================================ 4: column-sum finish
FINISH_P = (1, 8, 24, 25, 32, 33, 56, 57, 63, 65, 257)


def _finish_inputs(P, C, seed):
    """(integer partials, random partials): N(0, 1) times a log-normal spread, column 0 cancelling (+x, -x, tiny)."""
    rng = np.random.default_rng(seed)
    exact = rng.integers(-512, 513, (P, C)).astype(np.float32)
    rnd = (rng.standard_normal((P, C)) * np.exp(rng.standard_normal((P, C)))).astype(np.float32)
    if P >= 3:
        rnd[:, 0] = 0
        rnd[0, 0], rnd[1, 0], rnd[2, 0] = 1234.5, -1234.5, 1e-4
    return exact, rnd


def _finish(part, P, C, dtype, dev):
    L = _L()
    out = Guard((C,), dtype, dev)
    L.check(L.load().mi_colsum_finish(part.data_ptr(), P, C, out.ptr(), 0 if dtype == torch.bfloat16 else 1, _st()), "mi_colsum_finish")
    torch.cuda.synchronize()
    out.check(f"finish P {P} C {C} {dtype}")
    return out


def _check_finish(o32, o16, part_h, exact, what):
    got32 = o32.t.cpu().numpy()
    if exact:   # integers in [-512, 512]: every partial sum is an integer below 2^24, any order is exact
        np.testing.assert_array_equal(got32.astype(np.float64), G.colsum_ref(part_h)[0], err_msg=what)
    else:
        ok = G.colsum_f32_ok(got32, part_h)
        assert ok.all(), f"{what}: columns {np.nonzero(~ok)[0][:8]} beyond the bound"
    np.testing.assert_array_equal(o16.bits(), G.f32_to_bf16(got32), err_msg=what)   # bf16 output = RNE of the fp32 output


@pytest.mark.parametrize("C", [1, 31, 32, 33, 40, 3080])
def test_colsum_finish_vs_float64(dev, C):
    """P around the 32-row unrolled loop's edges (24 / 25: first unrolled round; 32 / 33, 56 / 57: the tail loop's first and
    second step after it), C beside the 32-column workgroup (the c < C guard); a NaN row after the last partial row."""
    for P in FINISH_P:
        for exact, part_h in zip((True, False), _finish_inputs(P, C, P * 10000 + C)):
            part = _f32_in(part_h, dev, tail=max(MARGIN, C))
            _check_finish(_finish(part, P, C, torch.float32, dev), _finish(part, P, C, torch.bfloat16, dev), part_h, exact,
                          f"P {P} C {C} exact {exact}")


MULTI = ((24, 32, torch.bfloat16), (33, 33, torch.float32), (57, 1, torch.bfloat16), (8, 64, torch.float32))  # (P, C, out dtype)


@pytest.mark.parametrize("n", [1, 2, 3, 4])
def test_colsum_finish_multi_abutting_ranges(dev, n):
    """n descriptors whose block ranges abut (1 | 2 | 1 | 2 blocks), bf16 and fp32 outputs mixed: each output is bitwise the single
    finish and exact on integer partials."""
    L = _L()
    desc = MULTI[:n]
    for exact in (True, False):
        hosts = [_finish_inputs(P, C, 77 + i)[0 if exact else 1] for i, (P, C, _) in enumerate(desc)]
        parts = [_f32_in(h, dev, tail=max(MARGIN, h.shape[1])) for h in hosts]
        outs = [Guard((C,), dt, dev) for (_, C, dt) in desc]
        arr = lambda ct, vals: (ct * n)(*vals)
        L.check(L.load().mi_colsum_finish_multi(arr(ctypes.c_void_p, [p.data_ptr() for p in parts]), arr(ctypes.c_int64, [d[0] for d in desc]),
                                                arr(ctypes.c_int64, [d[1] for d in desc]), arr(ctypes.c_void_p, [o.ptr() for o in outs]),
                                                arr(ctypes.c_int, [0 if d[2] == torch.bfloat16 else 1 for d in desc]), n, _st()),
                "mi_colsum_finish_multi")
        torch.cuda.synchronize()
        for i, ((P, C, dt), h, part, o) in enumerate(zip(desc, hosts, parts, outs)):
            o.check(f"multi {i}")
            single = _finish(part, P, C, dt, dev)
            assert torch.equal(o.t.view(torch.int16 if dt == torch.bfloat16 else torch.int32),
                               single.t.view(torch.int16 if dt == torch.bfloat16 else torch.int32)), f"n {n} descriptor {i}"
            o32 = o if dt == torch.float32 else _finish(part, P, C, torch.float32, dev)
            o16 = o if dt == torch.bfloat16 else _finish(part, P, C, torch.bfloat16, dev)
            _check_finish(o32, o16, h, exact, f"n {n} descriptor {i} exact {exact}")


def test_colsum_finish_multi_wrapper_splits_six_into_two_launches(ops, dev):
    shapes = [(24, 32, torch.bfloat16), (33, 33, torch.float32), (57, 1, torch.bfloat16), (8, 64, torch.float32),
              (65, 40, torch.float32), (25, 31, torch.bfloat16)]
    hosts = [_finish_inputs(P, C, 5 + i)[0] for i, (P, C, _) in enumerate(shapes)]
    items = [(_f32_in(h, dev, tail=max(MARGIN, h.shape[1])), dt) for h, (_, _, dt) in zip(hosts, shapes)]
    for got, h, (part, _), (P, C, dt) in zip(ops.colsum_finish_multi(items), hosts, items, shapes):
        want = G.colsum_ref(h)[0]
        assert got.dtype == dt and got.shape == (C,) and torch.equal(got, ops.colsum_finish(part, dt))
        if dt == torch.float32:
            np.testing.assert_array_equal(got.cpu().numpy().astype(np.float64), want)
        else:
            np.testing.assert_array_equal(got.view(torch.int16).cpu().numpy().view(np.uint16), G.rne_bf16(want))


# ================================================================================================ 5: RMSNorm statistics
STATS_ROWS = (1, 3, 4, 5, 9)
EPS = 1e-5


def _stats_calls(dev, a_b, b_b, bias_b, eps, x_b=None):
    """The three entry points: {name: (guarded out or None, guarded rstd)}; mi_rmsnorm_stats runs on x (default a); inputs are
    followed by NaN."""
    L = _L()
    lib = L.load()
    rows, cols = a_b.shape
    a, b, bias = _bf16_in(a_b, dev), _bf16_in(b_b, dev), _bf16_in(bias_b, dev)
    x = a if x_b is None else _bf16_in(x_b, dev)
    res = {}
    for name in ("stats", "add", "add_bias"):
        rstd = Guard((rows,), torch.float32, dev)
        out = None if name == "stats" else Guard((rows, cols), torch.bfloat16, dev)
        if name == "stats":
            L.check(lib.mi_rmsnorm_stats(x.data_ptr(), rstd.ptr(), rows, cols, eps, _st()), name)
        elif name == "add":
            L.check(lib.mi_add_rmsnorm_stats(a.data_ptr(), b.data_ptr(), out.ptr(), rstd.ptr(), rows, cols, eps, _st()), name)
        else:
            L.check(lib.mi_add_bias_rmsnorm_stats(a.data_ptr(), b.data_ptr(), bias.data_ptr(), out.ptr(), rstd.ptr(), rows, cols, eps,
                                                  _st()), name)
        res[name] = (out, rstd)
    torch.cuda.synchronize()
    return res


def _check_stats(res, a_b, b_b, bias_b, eps, what, x_b=None):
    stats_in = a_b if x_b is None else x_b
    for name, (out, rstd) in res.items():
        x_b = stats_in if name == "stats" else G.add_ref(a_b, b_b, bias_b if name == "add_bias" else None)
        if out is not None:   # bf16(f32(a) + (f32(b) + f32(bias))): float32 adds cannot contract, this is the definition
            got = out.bits()
            nan = np.isnan(G.bf16_to_f64(x_b))
            np.testing.assert_array_equal(np.where(nan, 0, got), np.where(nan, 0, x_b), err_msg=f"{what} {name}: out")
            assert np.isnan(G.bf16_to_f64(got))[nan].all()
            out.check(f"{what} {name} out", allow=nan)
        got = rstd.t.cpu().numpy()
        ok = G.rstd_ok(got, x_b, eps)       # rtol (cols / 64 + 16) 2^-24: glue_oracle.rstd_rtol
        ref = G.rstd_ref(x_b, eps)
        assert ok.all(), f"{what} {name}: rstd rows {np.nonzero(~ok)[0]} off by {np.abs(got - ref)[~ok] / np.abs(ref)[~ok] * 2 ** 24} x 2^-24"
        rstd.check(f"{what} {name} rstd", allow=np.isnan(ref))


@pytest.mark.parametrize("cols", [8, 16, 504, 512, 520, 1032, 8192, 8200])
def test_rmsnorm_stats_family_vs_float64(dev, cols):
    """mi_rmsnorm_stats / mi_add_rmsnorm_stats / mi_add_bias_rmsnorm_stats: `out` bit-exact against the float32 add, rstd against
    float64 on the rounded out; row counts that do not fill the 4-row workgroup, widths beside the 512-column lap."""
    for rows in STATS_ROWS:
        rng = np.random.default_rng(cols * 16 + rows)
        a_b = G.f32_to_bf16((rng.standard_normal((rows, cols)) * np.exp(rng.standard_normal((rows, 1)))).astype(np.float32))
        b_b, bias_b = _normal_bits(rng, (rows, cols)), _normal_bits(rng, (cols,), 0.5)
        _check_stats(_stats_calls(dev, a_b, b_b, bias_b, EPS), a_b, b_b, bias_b, EPS, f"rows {rows} cols {cols}")


@pytest.mark.parametrize("cols", [8, 520, 8200])
def test_rmsnorm_stats_spike_and_degenerate_rows(dev, cols):
    """Rows that are zero except the first / the last element (rstd = 1 / sqrt(v^2 / cols + eps)), an all-zero row (rsqrt(eps);
    Inf under eps = 0), a + b overflowing to Inf (rstd 0, out Inf there), a NaN that poisons only its own row."""
    rng = np.random.default_rng(cols)
    rows = 7
    a_b, b_b = _normal_bits(rng, (rows, cols)), _normal_bits(rng, (rows, cols))
    bias_b = np.zeros(cols, dtype=np.uint16)
    three, big = G.f32_to_bf16(np.float32(3.0)), G.f32_to_bf16(np.float32(3.0e38))
    for r in (0, 1, 2):
        a_b[r], b_b[r] = 0, 0
    a_b[0, 0] = three
    a_b[1, -1] = three
    a_b[4, cols // 2], b_b[4, cols // 2] = big, big
    a_b[5, cols - 3] = 0x7FC0
    x_b = G.add_ref(a_b, b_b)     # mi_rmsnorm_stats gets the rounded sum: the same rows, the Inf included
    for eps in (EPS, 0.0):
        res = _stats_calls(dev, a_b, b_b, bias_b, eps, x_b)
        _check_stats(res, a_b, b_b, bias_b, eps, f"cols {cols} eps {eps}", x_b)
        for name, (out, rstd) in res.items():
            got = rstd.t.cpu().numpy().astype(np.float64)
            e32 = float(np.float32(eps))
            spike = 1.0 / np.sqrt(9.0 / cols + e32)
            assert abs(got[0] - spike) <= G.rstd_rtol(cols) * spike and abs(got[1] - spike) <= G.rstd_rtol(cols) * spike, name
            if eps == 0.0:
                assert got[2] == np.inf, name
            else:
                assert abs(got[2] - 1.0 / np.sqrt(e32)) <= G.rstd_rtol(cols) / np.sqrt(e32), name
            assert got[4] == 0.0 and np.isnan(got[5]) and np.isfinite(got[[0, 1, 3, 6]]).all(), name
            if out is not None:
                assert out.bits()[4, cols // 2] == 0x7F80, name


# ================================================================================================ 6: squared norms, mi_adamw_bf16
def _offset_bf16(bits, dev, offset):
    """bf16 tensor whose pointer is `offset` elements past a 16-byte boundary, NaN around it in the same allocation."""
    n = bits.size
    buf = torch.empty(n + 2 * MARGIN, dtype=torch.int16, device=dev)
    buf.fill_(0x7FC0)
    t = buf[MARGIN + offset:MARGIN + offset + n]
    t.copy_(torch.from_numpy(bits.view(np.int16)).to(dev))
    assert t.data_ptr() % 16 == 2 * offset
    return t, buf


@pytest.mark.parametrize("chunk_elems", [8, 2048, 65536])
def test_sumsq_multi_hand_built_table_exact(dev, chunk_elems):
    """mi_sumsq_bf16_multi on a hand-built table: small-integer gradients, so every chunk's float64 partial is exact (equal to
    math.fsum).  Tensor sizes around the 8-element vector and the chunk; per-chunk vector counts 255 .. 257 and 511 .. 513 (the
    two-vector unrolled loop's edges); one tensor offset by one element (the element-wise walk); an Inf and a NaN gradient make
    their own chunks' partials Inf / NaN and leave the others alone."""
    L = _L()
    rng = np.random.default_rng(chunk_elems)
    sizes = [1, 7, 8, 9, 2047, 2048 * 8 + 3, 65536 + 8] + [8 * k for k in (255, 256, 257, 511, 512, 513)] + [8 * 513 + 5, 2048 * 8 + 3, 4099]
    offsets = [0] * (len(sizes) - 2) + [1, 0]
    hosts = [_int_bits(rng, (n,)) for n in sizes]
    hosts[-1][100], hosts[-1][3000] = 0x7F80, 0x7FC0        # chunks 12 / 375 of 8, 0 / 1 of 2048, the same chunk of 65536
    keep = [_offset_bf16(h, dev, off) for h, off in zip(hosts, offsets)]
    nt = len(sizes)
    table = np.zeros((5, nt), dtype=np.int64)
    table[1] = [t.data_ptr() for t, _ in keep]
    table[4] = sizes
    chunks = np.array([(i, c) for i, n in enumerate(sizes) for c in range((n + chunk_elems - 1) // chunk_elems)], dtype=np.int32)
    want = []
    for i, c in chunks:
        v = G.bf16_to_f64(hosts[i][c * chunk_elems:(c + 1) * chunk_elems])
        with np.errstate(invalid="ignore", over="ignore"):
            want.append(math.fsum(v * v) if np.isfinite(v).all() else float(np.sum(v * v)))
    tab_d, chunks_d = torch.from_numpy(table).to(dev), torch.from_numpy(chunks).to(dev)
    part = Guard((len(chunks),), torch.float64, dev)
    L.check(L.load().mi_sumsq_bf16_multi(tab_d.data_ptr(), nt, chunks_d.data_ptr(), len(chunks), chunk_elems, part.ptr(), _st()),
            "mi_sumsq_bf16_multi")
    torch.cuda.synchronize()
    want = np.array(want)
    got = part.t.cpu().numpy()
    np.testing.assert_array_equal(got, want)                # equal_nan: the NaN chunk is NaN, the Inf chunk Inf
    n_bad = int((~np.isfinite(want)).sum())
    assert n_bad == (1 if chunk_elems == 65536 else 2) and (np.isnan(want).sum() == 1)
    part.check("partials", allow=np.isnan(want))


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("n_partials", [1, 3, 64])
def test_sumsq_single_exact(dev, n_partials, offset):
    """mi_sumsq_bf16 (exported, no Python caller): integer gradients in [-4, 4], so every fp32 partial and their total are exact
    integers below 2^24; aligned (four-vector unrolled loop, its tail, the element tail) and one-element-offset pointers."""
    L = _L()
    rng = np.random.default_rng(n_partials)
    for n in (1, 7, 8, 9, 2047, 2048 * 8 + 3, 65536 + 8, 8 * (4 * 64 * 256 + 5) + 3):   # the last: 4 strides of 64 x 256 vectors + a tail
        h = _int_bits(rng, (n,), lim=4)
        t, _keep = _offset_bf16(h, dev, offset)
        v = G.bf16_to_f64(h)
        want = math.fsum(v * v)
        assert want < 2 ** 24
        part = Guard((n_partials,), torch.float32, dev)
        L.check(L.load().mi_sumsq_bf16(t.data_ptr(), n, part.ptr(), n_partials, _st()), "mi_sumsq_bf16")
        torch.cuda.synchronize()
        part.check(f"n {n}")
        got = part.t.cpu().numpy().astype(np.float64)
        assert (got == np.floor(got)).all() and got.sum() == want, f"n {n}: {got.sum()} vs {want}"


@pytest.mark.parametrize("step", [1, 7])
@pytest.mark.parametrize("grad_scale", [None, 0.37])
@pytest.mark.parametrize("n", [8, 1000, 1003, 65536 + 24])
def test_adamw_single_is_bitwise_the_multi_form(dev, n, grad_scale, step):
    """mi_adamw_bf16 (exported, no Python caller) == mi_adamw_bf16_multi on the same single tensor, p / exp_avg / exp_avg_sq bit
    for bit (n = 1003: the element-wise tail after the 8-wide vectors); the multi form is held to float64 by
    test_kernel_widths_gpu.py."""
    L = _L()
    lib = L.load()
    rng = np.random.default_rng(n + step)
    host = [_normal_bits(rng, (n,)), _normal_bits(rng, (n,), 0.1), _normal_bits(rng, (n,), 0.05),
            G.f32_to_bf16((rng.standard_normal(n) ** 2 * 1e-3).astype(np.float32))]   # p, g, exp_avg, exp_avg_sq
    gs = None if grad_scale is None else torch.tensor([grad_scale], device=dev)
    hp = (1e-2, 0.9, 0.999, 1e-8, 0.1)
    results = []
    for multi in (False, True):
        gd = [Guard((n,), torch.bfloat16, dev) for _ in host]
        for g_, h in zip(gd, host):
            g_.t.copy_(torch.from_numpy(h.view(np.int16)).to(dev).view(torch.bfloat16))
        p, g, m, v = gd
        if multi:
            table = torch.tensor([[p.ptr()], [g.ptr()], [m.ptr()], [v.ptr()], [n]], dtype=torch.int64, device=dev)
            chunks = torch.tensor([(0, c) for c in range((n + 65535) // 65536)], dtype=torch.int32, device=dev)
            L.check(lib.mi_adamw_bf16_multi(table.data_ptr(), 1, chunks.data_ptr(), chunks.shape[0], 65536, None if gs is None else gs.data_ptr(),
                                            *hp, step, _st()), "mi_adamw_bf16_multi")
        else:
            L.check(lib.mi_adamw_bf16(p.ptr(), g.ptr(), m.ptr(), v.ptr(), n, None if gs is None else gs.data_ptr(), *hp, step, _st()),
                    "mi_adamw_bf16")
        torch.cuda.synchronize()
        for g_, name in zip(gd, "pgmv"):
            g_.check(f"multi {multi} {name}")
        np.testing.assert_array_equal(g.bits(), host[1])
        results.append([x.bits() for x in (p, m, v)])
    for single, multi, name, before in zip(results[0], results[1], ("p", "exp_avg", "exp_avg_sq"), (host[0], host[2], host[3])):
        np.testing.assert_array_equal(single, multi, err_msg=name)
        assert (single != before).any(), f"{name}: the step changed nothing"
