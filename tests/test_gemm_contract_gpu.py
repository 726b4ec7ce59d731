"""GPU: the part of the GEMM contract of include/mi_fp8.h that the shape / format / algo sweeps of test_kernels_gpu.py never reach.

A. Leading dimensions and interior pointers: A, B and D are views into larger parents (guard rows around them, a column offset
   of 16 bytes, every operand byte outside the views = 0x7F = NaN in both formats, D's parent pre-filled with a bit pattern).  The
   view of D must be bit for bit the run on tight copies, nothing outside it may change, and both agree with the float64 oracle.
B. Non-finite operand bytes, scales and bias: one poisoned byte poisons exactly its own output row or column and nothing else,
   a poisoned launch leaves nothing behind for the next one, alpha and the bf16 conversion overflow to the right infinity.
   MXFP8 twins: a NaN byte, a 0xFF block scale, an all-zero block under any scale byte.
Every comparison is bitwise, a set membership (finite / non-finite) or one of the existing criteria against the float64 oracle.

"Family" = generic (algo 1), fast (2, 3), eight-wave persistent (4, 5, 41-43), stream-K and its whole-tile twin (44, 45), four-wave
(6, 9), the pickers (0, 47), mi_gemm_fp8_grouped with tile_cfg -1, 3, 4.  Stream-K (44) needs more 256 x 256 tiles than CUs, so it
runs on the multi-round shape only, where every comparison is kernel against itself."""
import functools

import numpy as np
import pytest
import torch

from oracle import fp8_oracle as O
from tests.util import assert_gemm_close, assert_mfma_close, bits_to_bf16, rand_fp8

pytestmark = pytest.mark.gpu

SMALL = (768, 768, 512)      # divides by 256 and by 192, K = 512: every algo but 44 takes it; float64 reference on the host
MULTI = (4352, 4096, 512)    # 272 tiles of 256 x 256: a persistent grid walks more than one tile per workgroup
GROUP = [(768, 768, 512), (1536, 768, 768)]  # unequal K; M, N multiples of 768 so that tile_cfg 3 (192 x 192) and 4 both fit
GROUP_MULTI = [MULTI, (768, 768, 768)]
FMTS = [(O.E4M3, O.E4M3), (O.E5M2, O.E4M3)]
ALGOS_SMALL = [0, 1, 2, 3, 4, 5, 41, 42, 43, 45, 6, 9, 47]
F32_ALGOS = (0, 1, 2, 3)
FAMILIES = [("algo", a) for a in ALGOS_SMALL] + [("grouped", c) for c in (-1, 3, 4)]
FAMILIES_MULTI = [("algo", 4), ("algo", 9), ("algo", 44), ("grouped", -1), ("grouped", 4)]
SA, SB = np.float32(1 / 7.3), np.float32(1 / 0.011)
FILL16, FILL32 = 0x5A5A, 0x5A5A5A5A   # pre-fill of D's parent: a finite value no GEMM here produces by accident


def _fam_id(f):
    return f"{f[0]}{f[1]}"


@pytest.fixture(scope="module")
def ops(dev):
    from llm_fp8_amd.pytorch import ops as _ops
    from llm_fp8_amd import _lib
    assert _lib.load().mi_device_supported() == 1, "not a gfx950 device"
    return _ops


def _f32(v, dev):
    return torch.tensor([v], dtype=torch.float32, device=dev)


def _takes_bias(fam):
    return fam[0] == "algo" and fam[1] != 6   # of the four-wave kernels only the persistent one takes a bias; grouped: none


@functools.lru_cache(maxsize=None)
def _operands(shape, fa, fb):
    """Clean operands (no NaN / Inf byte) and a bf16 bias."""
    M, N, K = shape
    a8 = rand_fp8((M, K), fa, 1 + M + K, 4.0 if fa == O.E4M3 else 64.0)
    b8 = rand_fp8((N, K), fb, 2 + N + K, 4.0 if fb == O.E4M3 else 64.0)
    bias = O.f32_to_bf16_bits(np.random.default_rng(3).normal(size=N).astype(np.float32) * 10)
    assert np.isfinite(O.fp8_decode(a8, fa)).all() and np.isfinite(O.fp8_decode(b8, fb)).all()
    return a8, b8, bias


@functools.lru_cache(maxsize=None)
def _ref(shape, fa, fb, use_bias):
    a8, b8, bias = _operands(shape, fa, fb)
    return O.gemm_fp8_tn(a8, b8, fa, fb, SA, SB, bias if use_bias else None, out_f32=True)


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


# ============================================================================================== A. leading dimensions
GUARD = 4  # parent rows before and after the view (>= 2: a buffer resource of rows * ld bytes from the view's start stays inside;
           # even: with ldd = N + 4 a bf16 row is 8 bytes off a 16-byte multiple, and the view must start 16-byte aligned)


def _view_in_parent(rows, cols, ld, dtype, fill, dev, src=None):
    """A flat parent of (rows + 2 GUARD) * ld elements filled with `fill` (an integer bit pattern) and a [rows, cols] view of row
    stride ld that starts GUARD rows in, at a column offset that is a multiple of 16 bytes but not of 256.  Returns (parent as
    integers, view, bool mask of the parent's elements that belong to the view)."""
    es = torch.empty((), dtype=dtype).element_size()
    idt = {1: torch.uint8, 2: torch.int16, 4: torch.int32}[es]
    n = (rows + 2 * GUARD) * ld
    parent = torch.full((n,), fill, dtype=idt, device=dev)
    typed = parent.view(dtype)
    start = None
    for off in (16, 48, 80, 112, 144):
        cand = GUARD * ld + off // es
        if (parent.data_ptr() + cand * es) % 256 != 0:
            start = cand
            break
    assert start is not None
    view = typed.as_strided((rows, cols), (ld, 1), start)
    assert view.data_ptr() % 16 == 0 and view.data_ptr() % 256 != 0
    if src is not None:
        view.copy_(src)
    mask = torch.zeros(n, dtype=torch.bool, device=dev)
    mask.as_strided((rows, cols), (ld, 1), start).fill_(True)
    assert int(mask.sum()) == rows * cols
    return parent, view, mask


def _pads(shape, combo):
    """lda, ldb in {K + 16, K + 48, 2K} with lda != ldb; ldd in {N + 4, N + 8, N + 136}: three combinations in which every value
    of every leading dimension occurs once (N + 4 is the smallest legal one: odd rows are only 8-byte aligned)."""
    M, N, K = shape
    return [(K + 16, K + 48, N + 4), (K + 48, 2 * K, N + 8), (2 * K, K + 16, N + 136)][combo]


def _strided_problem(shape, fa, fb, combo, out_dtype, dev):
    M, N, K = shape
    a8, b8, _ = _operands(shape, fa, fb)
    lda, ldb, ldd = _pads(shape, combo)
    at, bt = torch.from_numpy(a8).to(dev), torch.from_numpy(b8).to(dev)
    pa, av, _ = _view_in_parent(M, K, lda, torch.uint8, 0x7F, dev, at)
    pb, bv, _ = _view_in_parent(N, K, ldb, torch.uint8, 0x7F, dev, bt)
    pd, dv, md = _view_in_parent(M, N, ldd, out_dtype, FILL16 if out_dtype == torch.bfloat16 else FILL32, dev)
    return dict(at=at, bt=bt, pa=pa, av=av, pb=pb, bv=bv, pd=pd, dv=dv, md=md, pa0=pa.clone(), pb0=pb.clone(),
                fill=FILL16 if out_dtype == torch.bfloat16 else FILL32)


def _assert_parents_intact(p, what):
    assert bool((p["pd"][~p["md"]] == p["fill"]).all()), f"{what}: D's parent changed outside the view (padding columns / guard rows)"
    assert torch.equal(p["pa"], p["pa0"]) and torch.equal(p["pb"], p["pb0"]), f"{what}: an operand's parent changed"


def _strided_gemm_case(ops, dev, algo, fa, fb, shape, combo, use_bias, out_dtype, oracle):
    what = f"algo {algo} fmt({fa},{fb}) {shape} pads {_pads(shape, combo)} bias {use_bias} {out_dtype}"
    p = _strided_problem(shape, fa, fb, combo, out_dtype, dev)
    a8, b8, bias = _operands(shape, fa, fb)
    bt = bits_to_bf16(bias, dev) if use_bias else None
    sa, sb = _f32(SA, dev), _f32(SB, dev)
    ops.gemm_fp8(p["av"], p["bv"], sa, sb, fa, fb, bias=bt, out=p["dv"], algo=algo)
    tight = ops.gemm_fp8(p["at"], p["bt"], sa, sb, fa, fb, bias=bt, out_dtype=out_dtype, algo=algo)
    torch.cuda.synchronize()
    assert torch.equal(_bits(p["dv"]), _bits(tight)), f"{what}: the view of D differs from the run on tight copies"
    _assert_parents_intact(p, what)
    if oracle:
        ref = _ref(shape, fa, fb, use_bias)
        if out_dtype == torch.bfloat16:
            assert_gemm_close(p["dv"].float().cpu().numpy(), ref, what)
        else:
            assert not use_bias
            assert_mfma_close(p["dv"].contiguous().cpu().numpy(), ref, a8, b8, fa, fb, float(SA) * float(SB))


@pytest.mark.parametrize("combo", [0, 1, 2])
@pytest.mark.parametrize("fa,fb", FMTS)
@pytest.mark.parametrize("algo", ALGOS_SMALL)
def test_strided_views_are_bitwise_the_tight_run_and_match_the_oracle(ops, dev, algo, fa, fb, combo):
    """A kernel that used K where it meant lda (or N for ldd) in any cursor reads 0x7F padding -> NaN, or lands outside the view."""
    for use_bias in ((False, True) if _takes_bias(("algo", algo)) else (False,)):
        _strided_gemm_case(ops, dev, algo, fa, fb, SMALL, combo, use_bias, torch.bfloat16, oracle=True)
    if algo in F32_ALGOS:
        _strided_gemm_case(ops, dev, algo, fa, fb, SMALL, combo, False, torch.float32, oracle=True)


@pytest.mark.parametrize("combo", [0, 1, 2])
@pytest.mark.parametrize("fa,fb", FMTS)
@pytest.mark.parametrize("algo", [4, 9, 44])
def test_strided_views_multi_round_are_bitwise_the_tight_run(ops, dev, algo, fa, fb, combo):
    """More than one tile per workgroup (the cursor advance between tiles, the stream-K ranges): kernel against itself."""
    for use_bias in (False, True):
        _strided_gemm_case(ops, dev, algo, fa, fb, MULTI, combo, use_bias, torch.bfloat16, oracle=False)


@pytest.mark.parametrize("combo", [0, 1, 2])
@pytest.mark.parametrize("fa,fb", FMTS)
@pytest.mark.parametrize("cfg", [-1, 3, 4])
def test_grouped_strided_views_are_bitwise_the_tight_run_and_match_the_oracle(ops, dev, cfg, fa, fb, combo):
    """Each problem of the group has its own paddings (32-bit buffer offsets, buffer sizes and store offsets per problem)."""
    sa, sb = _f32(SA, dev), _f32(SB, dev)
    ps = [_strided_problem(shape, fa, fb, (combo + i) % 3, torch.bfloat16, dev) for i, shape in enumerate(GROUP)]
    ops.gemm_fp8_grouped([(p["av"], p["bv"], sa, sb, p["dv"]) for p in ps], fa, fb, tile_cfg=cfg)
    tight = [torch.full(shape[:2], float("nan"), dtype=torch.bfloat16, device=dev) for shape in GROUP]
    ops.gemm_fp8_grouped([(p["at"], p["bt"], sa, sb, t) for p, t in zip(ps, tight)], fa, fb, tile_cfg=cfg)
    torch.cuda.synchronize()
    for p, t, shape in zip(ps, tight, GROUP):
        what = f"grouped cfg {cfg} fmt({fa},{fb}) problem {shape}"
        assert torch.equal(_bits(p["dv"]), _bits(t)), f"{what}: the view of D differs from the run on tight copies"
        _assert_parents_intact(p, what)
        assert_gemm_close(p["dv"].float().cpu().numpy(), _ref(shape, fa, fb, False), what)


def _bad_operands(kind, M, N, K, dev):
    """(a, b, out) of which one breaks one rule of the leading-dimension / alignment contract, and the message it must get."""
    u8z = lambda r, c: torch.zeros((r, c), dtype=torch.uint8, device=dev)
    a, b = u8z(M, K), u8z(N, K)
    out = torch.full((M, N), 1.0, dtype=torch.bfloat16, device=dev)
    if kind == "lda%16":
        a = u8z(M, K + 8)[:, :K]
    elif kind == "ldb%16":
        b = u8z(N, K + 24)[:, :K]
    elif kind == "ldd%4":
        out = torch.full((M, N + 2), 1.0, dtype=torch.bfloat16, device=dev)[:, :N]
    elif kind == "A+8":
        a = u8z(M, K + 16)[:, 8:8 + K]
    elif kind == "B+8":
        b = u8z(N, K + 16)[:, 8:8 + K]
    elif kind == "D+8":
        out = torch.full((M, N + 8), 1.0, dtype=torch.bfloat16, device=dev)[:, 4:4 + N]
    else:
        raise AssertionError(kind)
    return a, b, out, ("16-byte aligned" if "+8" in kind else "bad leading dimensions")


BAD_KINDS = ["lda%16", "ldb%16", "ldd%4", "A+8", "B+8", "D+8"]


@pytest.mark.parametrize("kind", BAD_KINDS)
def test_gemm_refuses_illegal_leading_dimensions_and_pointers(ops, dev, kind):
    M, N, K = 256, 256, 256
    one = _f32(1.0, dev)
    a, b, out, msg = _bad_operands(kind, M, N, K, dev)
    for algo in (0, 1, 3, 4, 6):
        with pytest.raises(RuntimeError, match=msg):
            ops.gemm_fp8(a, b, one, one, 0, 0, out=out, algo=algo)
    torch.cuda.synchronize()
    assert bool((out == 1.0).all()), "a refused call wrote to D"


@pytest.mark.parametrize("slot", [0, 1])
@pytest.mark.parametrize("kind", BAD_KINDS)
def test_grouped_gemm_refuses_illegal_leading_dimensions_and_pointers_in_each_slot(ops, dev, kind, slot):
    M, N, K = 256, 256, 256
    one = _f32(1.0, dev)
    good = (torch.zeros((M, K), dtype=torch.uint8, device=dev), torch.zeros((N, K), dtype=torch.uint8, device=dev), one, one,
            torch.full((M, N), 1.0, dtype=torch.bfloat16, device=dev))
    a, b, out, msg = _bad_operands(kind, M, N, K, dev)
    probs = [good, good]
    probs[slot] = (a, b, one, one, out)
    for cfg in (-1, 0):
        with pytest.raises(RuntimeError, match=msg):
            ops.gemm_fp8_grouped(probs, 0, 0, tile_cfg=cfg)
    torch.cuda.synchronize()
    assert bool((out == 1.0).all()) and bool((good[4] == 1.0).all()), "a refused call wrote to D"


def test_gemm_refuses_leading_dimensions_below_the_row_length(ops, dev):
    """ld < K / ld < N: no torch view expresses them, so straight through the C ABI (real tensors, nothing is launched)."""
    from llm_fp8_amd import _lib
    lib = _lib.load()
    M, N, K = 256, 256, 256
    a = torch.zeros((M, K), dtype=torch.uint8, device=dev)
    out = torch.full((M, N), 1.0, dtype=torch.bfloat16, device=dev)
    one = _f32(1.0, dev)
    st = torch.cuda.current_stream().cuda_stream
    for lda, ldb, ldd in ((K - 16, K, N), (K, K - 16, N), (K, K, N - 4)):
        for algo in (0, 1, 4):
            rc = lib.mi_gemm_fp8(a.data_ptr(), a.data_ptr(), out.data_ptr(), one.data_ptr(), one.data_ptr(), None, M, N, K, lda, ldb, ldd,
                                 0, 0, 0, algo, st)
            assert rc == -1
            with pytest.raises(RuntimeError, match="bad leading dimensions"):
                _lib.check(rc, "mi_gemm_fp8")
        for slot in (0, 1):
            arr = (_lib.GemmProblem * 2)()
            for i in range(2):
                l = (lda, ldb, ldd) if i == slot else (K, K, N)
                arr[i] = _lib.GemmProblem(a.data_ptr(), a.data_ptr(), out.data_ptr(), one.data_ptr(), one.data_ptr(), M, N, K, *l)
            import ctypes
            rc = lib.mi_gemm_fp8_grouped(ctypes.byref(arr), 2, 0, 0, -1, st)
            assert rc == -1
            with pytest.raises(RuntimeError, match=f"bad leading dimensions in problem {slot}"):
                _lib.check(rc, "mi_gemm_fp8_grouped")
    torch.cuda.synchronize()
    assert bool((out == 1.0).all()), "a refused call wrote to D"


# ============================================================================================== B. non-finite bytes, scales, bias
def _second(shapes, fa, fb, dev):
    """The clean second problem of a grouped launch (unequal K): tensors and its output buffer."""
    a8, b8, _ = _operands(shapes[1], fa, fb)
    return (torch.from_numpy(a8).to(dev), torch.from_numpy(b8).to(dev),
            torch.empty(shapes[1][:2], dtype=torch.bfloat16, device=dev))


def _make_runner(ops, dev, fam, shape, fa, fb):
    """run(a, b, bias=None, sa=, sb=, out_dtype=) -> D of the first problem through one family.  The grouped families carry a clean
    second problem along, whose output must never change."""
    M, N, K = shape
    state = {}
    if fam[0] == "grouped":
        shapes = GROUP if shape == SMALL else GROUP_MULTI
        a2, b2, o2 = _second(shapes, fa, fb, dev)

    def run(a, b, bias=None, sa=SA, sb=SB, out_dtype=torch.bfloat16):
        sa_t, sb_t = _f32(sa, dev), _f32(sb, dev)
        if fam[0] == "algo":
            return ops.gemm_fp8(a, b, sa_t, sb_t, fa, fb, bias=bias, out_dtype=out_dtype, algo=fam[1])
        assert bias is None and out_dtype == torch.bfloat16
        out = torch.full((M, N), 1.0, dtype=torch.bfloat16, device=dev)
        o2.fill_(float("nan"))
        ops.gemm_fp8_grouped([(a, b, sa_t, sb_t, out), (a2, b2, _f32(SA, dev), _f32(SB, dev), o2)], fa, fb, tile_cfg=fam[1])
        if "o2" not in state:
            state["o2"] = o2.clone()
            assert bool(torch.isfinite(o2).all())
        assert torch.equal(_bits(o2), _bits(state["o2"])), "the clean second problem of the group changed"
        return out

    return run


@functools.lru_cache(maxsize=None)
def _ref_nonfinite(shape, fa, fb, where, i, k, byte):
    """(bool mask of the non-finite outputs, bool mask of the NaN outputs) of the float64 reference with ONE byte of A
    (where = "a": row i) or of B ("b": row i of B = column i of D) replaced.  Small shape: the whole oracle GEMM.  Multi-round shape:
    the operands are clean (asserted in _operands), so every other row / column of the reference is finite by construction and
    only the poisoned one is evaluated."""
    M, N, K = shape
    a8, b8, _ = _operands(shape, fa, fb)
    a8, b8 = a8.copy(), b8.copy()
    (a8 if where == "a" else b8)[i, k] = byte
    if shape == SMALL:
        ref = O.gemm_fp8_tn(a8, b8, fa, fb, SA, SB, None, out_f32=True)
        return ~np.isfinite(ref), np.isnan(ref)
    nonf, nan = np.zeros((M, N), bool), np.zeros((M, N), bool)
    if where == "a":
        r = O.gemm_fp8_tn(a8[i:i + 1], b8, fa, fb, SA, SB, None, out_f32=True)
        nonf[i], nan[i] = ~np.isfinite(r[0]), np.isnan(r[0])
    else:
        r = O.gemm_fp8_tn(a8, b8[i:i + 1], fa, fb, SA, SB, None, out_f32=True)
        nonf[:, i], nan[:, i] = ~np.isfinite(r[:, 0]), np.isnan(r[:, 0])
    return nonf, nan


def _line_mask(M, N, row=None, col=None):
    m = np.zeros((M, N), bool)
    if row is not None:
        m[row] = True
    if col is not None:
        m[:, col] = True
    return m


def _assert_poisoned(out, clean, mask_np, kind, what):
    """Non-finite outputs == mask exactly; inside it `kind` ("nan", "+inf", "-inf", "nonfinite"); outside it the clean bits."""
    mask = torch.from_numpy(mask_np).to(out.device)
    nonf = ~torch.isfinite(out)
    assert torch.equal(nonf, mask), (f"{what}: {int((nonf & ~mask).sum())} non-finite outputs outside the poisoned line, "
                                     f"{int((mask & ~nonf).sum())} finite ones inside it")
    inside = out[mask].float()
    if kind == "nan":
        assert bool(torch.isnan(inside).all()), f"{what}: {int((~torch.isnan(inside)).sum())} poisoned outputs are Inf, not NaN"
    elif kind in ("+inf", "-inf"):
        assert bool((inside == float(kind)).all()), f"{what}: poisoned outputs are not all {kind}"
    assert torch.equal(_bits(out)[~mask], _bits(clean)[~mask]), f"{what}: outputs outside the poisoned line differ from the clean run"


def _poison_cases(shape, fa, fb, few):
    """(where, row of A or B, k, byte, kind).  Rows and k at the tile, wave and K-tile seams."""
    M, N, K = shape
    ks = [0, 127, 128, K - 1]
    rows_a, rows_b = [0, 255, 256, M - 1], [0, 255, 256, N - 1]
    if few:
        cases = [("a", r, k, 0x7F, "nan") for r, k in zip(rows_a, ks)] + [("b", rows_b[1], ks[2], 0x7F, "nan"), ("b", rows_b[3], ks[0], 0x7F, "nan")]
    else:
        cases = [("a", r, k, 0x7F, "nan") for r in rows_a for k in ks] + [("b", r, k, 0x7F, "nan") for r, k in zip(rows_b, ks)]
    if fa == O.E5M2:
        cases += [("a", 255, 127, 0x7C, "nonfinite"), ("a", 256, 128, 0xFC, "nonfinite")]
    if fb == O.E5M2:
        cases += [("b", 255, 127, 0x7C, "nonfinite"), ("b", 256, 128, 0xFC, "nonfinite")]
    return cases


def _poison_test(ops, dev, fam, shape, fa, fb, few):
    M, N, K = shape
    a8, b8, bias = _operands(shape, fa, fb)
    at, bt = torch.from_numpy(a8).to(dev), torch.from_numpy(b8).to(dev)
    run = _make_runner(ops, dev, fam, shape, fa, fb)
    clean = run(at, bt)
    assert bool(torch.isfinite(clean).all())
    for where, i, k, byte, kind in _poison_cases(shape, fa, fb, few):
        what = f"{_fam_id(fam)} fmt({fa},{fb}) {shape}: byte {byte:#04x} in {where.upper()}[{i},{k}]"
        want = _line_mask(M, N, row=i) if where == "a" else _line_mask(M, N, col=i)
        ref_nonf, ref_nan = _ref_nonfinite(shape, fa, fb, where, i, k, byte)
        assert np.array_equal(ref_nonf, want), f"{what}: the reference's non-finite set is not the poisoned line (vacuous test)"
        if kind == "nan":
            assert np.array_equal(ref_nan, want), f"{what}: the reference is not NaN on the whole line"
        pa, pb = at, bt
        if where == "a":
            pa = at.clone()
            pa[i, k] = byte
        else:
            pb = bt.clone()
            pb[i, k] = byte
        _assert_poisoned(run(pa, pb), clean, want, kind, what)
        again = run(at, bt)
        assert torch.equal(_bits(again), _bits(clean)), f"{what}: the clean launch after it differs from the first clean result"
    if _takes_bias(fam):
        bias_t = bits_to_bf16(bias, dev)
        clean_b = run(at, bt, bias=bias_t)
        assert bool(torch.isfinite(clean_b).all())
        for j, v, kind in ((255, float("nan"), "nan"), (256, float("inf"), "+inf"), (N - 1, float("-inf"), "-inf")):
            what = f"{_fam_id(fam)} fmt({fa},{fb}) {shape}: bias[{j}] = {v}"
            pbias = bias_t.clone()
            pbias[j] = v
            if shape == SMALL:
                refb = _ref(shape, fa, fb, False).astype(np.float64) + pbias.float().cpu().numpy().astype(np.float64)[None, :]
                assert np.array_equal(~np.isfinite(refb), _line_mask(M, N, col=j))
                assert (np.isnan(refb[:, j]).all() if kind == "nan" else (refb[:, j] == float(kind)).all())
            _assert_poisoned(run(at, bt, bias=pbias), clean_b, _line_mask(M, N, col=j), kind, what)
        assert torch.equal(_bits(run(at, bt, bias=bias_t)), _bits(clean_b))


@pytest.mark.parametrize("fa,fb", FMTS)
@pytest.mark.parametrize("fam", FAMILIES, ids=_fam_id)
def test_one_poisoned_byte_poisons_exactly_its_row_or_column(ops, dev, fam, fa, fb):
    """One 0x7F (NaN) byte of A at every (row, k) seam combination, of B at four, for E5M2 one +-Inf byte, one NaN / +-Inf bias
    element: through the scaled-MFMA main loop, the epilogue lane shuffles, the bias add and the grouped form."""
    _poison_test(ops, dev, fam, SMALL, fa, fb, few=False)


@pytest.mark.parametrize("fa,fb", FMTS)
@pytest.mark.parametrize("fam", FAMILIES_MULTI, ids=_fam_id)
def test_one_poisoned_byte_multi_round(ops, dev, fam, fa, fb):
    """More than one tile per workgroup; for algo 44 the poisoned tile may be one that two workgroups sum through the stream-K
    workspace, and the clean launch after it pins that workspace and flags carry nothing over."""
    _poison_test(ops, dev, fam, MULTI, fa, fb, few=True)


@pytest.mark.parametrize("fam", FAMILIES, ids=_fam_id)
def test_non_finite_and_zero_scales(ops, dev, fam):
    fa, fb = O.E4M3, O.E4M3
    M, N, K = SMALL
    a8, b8, bias = _operands(SMALL, fa, fb)
    at, bt = torch.from_numpy(a8).to(dev), torch.from_numpy(b8).to(dev)
    run = _make_runner(ops, dev, fam, SMALL, fa, fb)
    assert bool(torch.isfinite(run(at, bt)).all())  # finite accumulators
    biases = (None, bits_to_bf16(bias, dev)) if _takes_bias(fam) else (None,)
    for bias_t in biases:
        assert bool(torch.isnan(run(at, bt, bias=bias_t, sa=float("nan"))).all()), "sa_inv = NaN must give NaN everywhere"
        assert bool((~torch.isfinite(run(at, bt, bias=bias_t, sa=float("inf")))).all()), "sa_inv = Inf must leave nothing finite"
        z = run(at, bt, bias=bias_t, sa=0.0)
        if bias_t is None:
            assert bool((z.float() == 0).all()), "sa_inv = 0 must give +-0 everywhere"
        else:
            assert torch.equal(_bits(z), _bits(bias_t[None, :].expand(M, N))), "sa_inv = 0 must give exactly the bias"


def _overflow_operands(fa, fb):
    """Block rows 256..271 of A hold +-16 in every k (rows 264.. negative), block rows 192..207 of B hold 16; everything else has
    magnitude <= 1.  Block outputs are exactly +-16 * 16 * K = +-2^17, every other |output| <= 16 * K = 2^13."""
    M, N, K = SMALL
    cap = lambda b8, thr: np.where((b8 & 0x7F) > thr, (b8 & 0x80) | thr, b8).astype(np.uint8)
    a8 = cap(rand_fp8((M, K), fa, 21, 1.0), 0x38 if fa == O.E4M3 else 0x3C)   # 0x38 / 0x3C = 1.0
    b8 = cap(rand_fp8((N, K), fb, 22, 1.0), 0x38 if fb == O.E4M3 else 0x3C)
    s16 = lambda f: 0x58 if f == O.E4M3 else 0x4C                             # 16.0
    a8[256:264] = s16(fa)
    a8[264:272] = s16(fa) | 0x80
    b8[192:208] = s16(fb)
    block = np.zeros((M, N), bool)
    block[256:272, 192:208] = True
    exact = O.fp8_decode(a8, fa).astype(np.float64) @ O.fp8_decode(b8, fb).astype(np.float64).T
    assert (np.abs(exact[block]) == 2.0 ** 17).all() and np.abs(exact[~block]).max() <= 2.0 ** 13
    return a8, b8, block, exact


FLT_MAX = float(np.finfo(np.float32).max)
BF16_MAX = float(2.0 ** 128 - 2.0 ** 120)   # 0x7F7F
BF16_ULP = float(2.0 ** 120)                # spacing of bf16 in the top binade


@pytest.mark.parametrize("fa,fb", FMTS)
@pytest.mark.parametrize("fam", FAMILIES, ids=_fam_id)
def test_alpha_overflow_gives_inf_exactly_on_the_block(ops, dev, fam, fa, fb):
    """alpha = 2^60 * 2^53: the block's reference outputs are +-2^130 > 2 FLT_MAX, all others <= 2^126 < FLT_MAX / 2."""
    a8, b8, block, exact = _overflow_operands(fa, fb)
    sa, sb = 2.0 ** 60, 2.0 ** 53
    ref = exact * float(np.float32(sa) * np.float32(sb))
    assert (np.abs(ref[block]) > 2 * FLT_MAX).all() and (np.abs(ref[~block]) < FLT_MAX / 2).all()
    want = torch.from_numpy(np.where(block, np.sign(ref) * np.inf, 0.0).astype(np.float32)).to(dev)
    mask = torch.from_numpy(block).to(dev)
    at, bt = torch.from_numpy(a8).to(dev), torch.from_numpy(b8).to(dev)
    run = _make_runner(ops, dev, fam, SMALL, fa, fb)
    dts = (torch.bfloat16, torch.float32) if fam[0] == "algo" and fam[1] in F32_ALGOS else (torch.bfloat16,)
    for dt in dts:
        out = run(at, bt, sa=sa, sb=sb, out_dtype=dt).float()
        assert torch.equal(~torch.isfinite(out), mask), f"{_fam_id(fam)} {dt}: the non-finite set is not the block"
        assert torch.equal(out[mask], want[mask]), f"{_fam_id(fam)} {dt}: the block is not +-Inf with the reference's sign"


@pytest.mark.parametrize("fa,fb", FMTS)
@pytest.mark.parametrize("fam", FAMILIES, ids=_fam_id)
def test_bf16_conversion_overflow_gives_inf_exactly_on_the_block(ops, dev, fam, fa, fb):
    """The fp32 result is finite, its bf16 rounding is not.  alpha = (2 - 2^-10) 2^60 * 2^50: the block's reference values are exactly
    +-(2^128 - 2^117) = the largest finite bf16 + 7/8 of a bf16 ulp, below FLT_MAX = 2^128 - 2^104.  (A whole ulp above the largest
    finite bf16 is 2^128 itself, which no finite fp32 reaches: the margin taken is the widest one that exists, well past the
    half-ulp point 2^128 - 2^119 from which round-to-nearest-even goes to Inf.)  All other values are <= 2^124: far more than one
    ulp below the largest finite bf16."""
    a8, b8, block, exact = _overflow_operands(fa, fb)
    sa, sb = float(np.float32((2.0 - 2.0 ** -10) * 2.0 ** 60)), 2.0 ** 50
    ref = exact * float(np.float32(sa) * np.float32(sb))
    assert (np.abs(ref[block]) >= BF16_MAX + 0.75 * BF16_ULP).all() and (np.abs(ref[block]) < FLT_MAX).all()
    assert (np.abs(ref[~block]) <= BF16_MAX - BF16_ULP).all()
    want = torch.from_numpy(np.where(block, np.sign(ref) * np.inf, 0.0).astype(np.float32)).to(dev)
    mask = torch.from_numpy(block).to(dev)
    at, bt = torch.from_numpy(a8).to(dev), torch.from_numpy(b8).to(dev)
    run = _make_runner(ops, dev, fam, SMALL, fa, fb)
    out = run(at, bt, sa=sa, sb=sb).float()
    assert torch.equal(~torch.isfinite(out), mask), f"{_fam_id(fam)}: the non-finite bf16 set is not the block"
    assert torch.equal(out[mask], want[mask]), f"{_fam_id(fam)}: the block is not +-Inf with the reference's sign"
    if fam[0] == "algo" and fam[1] in F32_ALGOS:
        out32 = run(at, bt, sa=sa, sb=sb, out_dtype=torch.float32)
        assert bool(torch.isfinite(out32).all()), f"{_fam_id(fam)}: the fp32 output must stay finite"
        assert torch.equal(out32[mask], torch.from_numpy(ref[block].astype(np.float32)).to(dev))


# ---------------------------------------------------------------------------------------------- MXFP8 twins
MX_ALGOS = [1, 4, 5, 41, 42, 43, 44]


@functools.lru_cache(maxsize=None)
def _mx_operands(shape):
    M, N, K = shape
    rng = np.random.default_rng(M + N)
    a8, b8 = rand_fp8((M, K), O.E4M3, 31 + M, 1.0), rand_fp8((N, K), O.E4M3, 32 + N, 1.0)
    ae = rng.integers(120, 135, size=(M, K // 32)).astype(np.uint8)   # [rows, K/32]; the device layout is its transpose
    be = rng.integers(120, 135, size=(N, K // 32)).astype(np.uint8)
    return a8, ae, b8, be


def _mx_ref_line(shape, a8, ae, b8, be, where, i):
    """float64 reference of the poisoned row (where = "a") or column only; the rest is finite by construction (clean operands)."""
    if where == "a":
        return O.gemm_mxfp8_tn(a8[i:i + 1], ae[i:i + 1], b8, be, out_f32=True)[0]
    return O.gemm_mxfp8_tn(a8, ae, b8[i:i + 1], be[i:i + 1], out_f32=True)[:, 0]


def _mx_shape(algo):
    return MULTI if algo == 44 else SMALL


def _mx_setup(ops, dev, algo):
    shape = _mx_shape(algo)
    a8, ae, b8, be = _mx_operands(shape)
    t = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(dev)
    at, bt, aet, bet = t(a8), t(b8), t(ae.T), t(be.T)   # block-major scales [K/32, rows]
    run = lambda a, sa, b, sb: ops.gemm_mxfp8(a, sa, b, sb, algo=algo)
    clean = run(at, aet, bt, bet)
    assert bool(torch.isfinite(clean).all())
    return shape, (a8, ae, b8, be), (at, aet, bt, bet), run, clean


MX_SEAMS = [(0, 0), (255, 127), (256, 128), (-1, -1)]   # (row, k), -1 = last


@pytest.mark.parametrize("algo", MX_ALGOS)
def test_mx_nan_byte_poisons_exactly_its_row_or_column(ops, dev, algo):
    shape, (a8, ae, b8, be), (at, aet, bt, bet), run, clean = _mx_setup(ops, dev, algo)
    M, N, K = shape
    for where in ("a", "b"):
        for r, k in MX_SEAMS:
            R = M if where == "a" else N
            i, kk = r % R, k % K
            what = f"mx algo {algo}: NaN byte in {where.upper()}[{i},{kk}]"
            p8 = (a8 if where == "a" else b8).copy()
            p8[i, kk] = 0x7F
            line = _mx_ref_line(shape, p8 if where == "a" else a8, ae, p8 if where == "b" else b8, be, where, i)
            assert np.isnan(line).all(), f"{what}: the reference line is not NaN (vacuous test)"
            pt = (at if where == "a" else bt).clone()
            pt[i, kk] = 0x7F
            out = run(pt, aet, bt, bet) if where == "a" else run(at, aet, pt, bet)
            _assert_poisoned(out, clean, _line_mask(M, N, row=i) if where == "a" else _line_mask(M, N, col=i), "nan", what)
            assert torch.equal(_bits(run(at, aet, bt, bet)), _bits(clean)), f"{what}: the clean launch after it differs"


def _mx_ff_kind(out, mask):
    inside = out[mask].float()
    if bool(torch.isnan(inside).all()):
        return "NaN"
    if bool(torch.isinf(inside).all()):
        return "Inf"
    return "mixed NaN/Inf" if bool((~torch.isfinite(inside)).all()) else "partly finite"


def _mx_ff_run(ops, dev, algo):
    """{(operand, row, block): kind} of a 0xFF block scale, after asserting the poisoned line is non-finite and the rest clean."""
    shape, (a8, ae, b8, be), (at, aet, bt, bet), run, clean = _mx_setup(ops, dev, algo)
    M, N, K = shape
    kinds = {}
    for where in ("a", "b"):
        for r, k in MX_SEAMS:
            R = M if where == "a" else N
            i, blk = r % R, (k % K) // 32
            what = f"mx algo {algo}: 0xFF scale of {where.upper()} row {i} block {blk}"
            pe = (ae if where == "a" else be).copy()
            pe[i, blk] = 0xFF
            line = _mx_ref_line(shape, a8, pe if where == "a" else ae, b8, pe if where == "b" else be, where, i)
            assert np.isnan(line).all(), f"{what}: the oracle does not say NaN (vacuous test)"
            pt = (aet if where == "a" else bet).clone()
            pt[blk, i] = 0xFF
            out = run(at, pt, bt, bet) if where == "a" else run(at, aet, bt, pt)
            mask = _line_mask(M, N, row=i) if where == "a" else _line_mask(M, N, col=i)
            _assert_poisoned(out, clean, mask, "nonfinite", what)
            kinds[(where, i, blk)] = _mx_ff_kind(out, torch.from_numpy(mask).to(dev))
    return kinds


@pytest.mark.parametrize("algo", MX_ALGOS)
def test_mx_ff_block_scale_gives_a_non_finite_row_or_column(ops, dev, algo):
    """E8M0 0xFF is NaN in the OCP MX specification (the oracle says NaN); the quantisers never emit it.  What the scaled MFMA does
    with it is printed per algo; include/mi_fp8.h records it."""
    kinds = _mx_ff_run(ops, dev, algo)
    print(f"\n[0xFF block scale] mi_gemm_mxfp8 algo {algo}: {sorted(set(kinds.values()))}")


def test_mx_ff_block_scale_is_the_same_in_every_algo(ops, dev):
    """The generic kernel and the persistent ones must not disagree on what a 0xFF scale gives."""
    per_algo = {algo: _mx_ff_run(ops, dev, algo) for algo in MX_ALGOS if _mx_shape(algo) == SMALL}
    first = per_algo[1]
    for algo, kinds in per_algo.items():
        assert kinds == first, f"algo {algo} gives {kinds}, the generic kernel {first}"


@pytest.mark.parametrize("algo", MX_ALGOS)
def test_mx_all_zero_block_contributes_nothing_under_any_scale_byte(ops, dev, algo):
    shape, _, (at, aet, bt, bet), run, _ = _mx_setup(ops, dev, algo)
    M, N, K = shape
    for where in ("a", "b"):
        for r, k in MX_SEAMS[1:3]:
            R = M if where == "a" else N
            i, blk = r % R, (k % K) // 32
            zt = (at if where == "a" else bt).clone()
            zt[i, blk * 32:(blk + 1) * 32] = 0
            outs = {}
            for s in (127, 0, 1, 100, 200, 0xFE):
                st = (aet if where == "a" else bet).clone()
                st[blk, i] = s
                outs[s] = run(zt, st, bt, bet) if where == "a" else run(at, aet, zt, st)
            assert bool(torch.isfinite(outs[127]).all())
            for s, o in outs.items():
                assert torch.equal(_bits(o), _bits(outs[127])), \
                    f"mx algo {algo}: all-zero block {blk} of {where.upper()} row {i} under scale byte {s} changes the output"
