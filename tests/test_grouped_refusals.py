"""CPU: every call mi_gemm_fp8_grouped refuses is refused on the host with a pinned return code and a pinned mi_last_error()
text -- including WHICH defect is named when two problems are defective (problems are checked in decreasing-K order) -- and the
refusals the two grouped entry points issue from the code they share (the schedule).  Pointers are fake: nothing is dereferenced
and nothing is launched."""
import ctypes

import pytest

FAKE = 0x10000  # non-null, 16-byte aligned, never dereferenced: every case below is refused before a launch
ARG, SHAPE = -1, -2  # MI_ERR_ARG, MI_ERR_SHAPE
P = "mi_gemm_fp8_grouped: "


def _call(probs, fmt_a=0, fmt_b=0, tile_cfg=-1, n=None, null=False):
    """probs: list of dicts overriding the fields of a valid, tight 256 x 256 x 256 problem."""
    from llm_fp8_amd import _lib
    lib = _lib.load()
    arr = (_lib.GemmProblem * max(len(probs), 1))()
    for i, over in enumerate(probs):
        f = dict(A=FAKE, B=FAKE, D=FAKE, sa_inv=FAKE, sb_inv=FAKE, M=256, N=256, K=256)
        f.update(over)
        f.setdefault("lda", f["K"])
        f.setdefault("ldb", f["K"])
        f.setdefault("ldd", f["N"])
        arr[i] = _lib.GemmProblem(*(f[k] for k, _ in _lib.GemmProblem._fields_))
    rc = lib.mi_gemm_fp8_grouped(None if null else ctypes.byref(arr), len(probs) if n is None else n, fmt_a, fmt_b, tile_cfg, None)
    return rc, lib.mi_last_error().decode()


BIG = 1 << 23  # 256 * 2^23 = 2^31 bytes
FIT = "problem %d (%d x %d x %d) does not fit tile shape %d x %d / K %% 256"
CASES = [
    # (id, problems, keyword arguments, return code, message after the "mi_gemm_fp8_grouped: " prefix)
    ("n0", [{}] * 4, dict(n=0), ARG, "1 to 4 problems"),
    ("n5", [{}] * 4, dict(n=5), ARG, "1 to 4 problems"),
    ("null_problems", [{}], dict(null=True), ARG, "1 to 4 problems"),
    ("fmt_a2", [{}], dict(fmt_a=2), ARG, "bad fmt"),
    ("fmt_b_neg", [{}], dict(fmt_b=-1), ARG, "bad fmt"),
    ("cfg5", [{}], dict(tile_cfg=5), ARG, "no tile shape divides every problem"),
    # any negative tile_cfg means "pick one" (a valid group would be launched): shown on a group no tile shape divides
    ("cfg_minus2_picks", [{"M": 200}, {}], dict(tile_cfg=-2), ARG, "no tile shape divides every problem"),
    ("null_A", [{}, {"A": None}], {}, ARG, "null pointer in problem 1"),
    ("null_B", [{}, {"B": None}], {}, ARG, "null pointer in problem 1"),
    ("null_D", [{}, {"D": None}], {}, ARG, "null pointer in problem 1"),
    ("null_sa_inv", [{}, {"sa_inv": None}], {}, ARG, "null pointer in problem 1"),
    ("null_sb_inv", [{}, {"sb_inv": None}], {}, ARG, "null pointer in problem 1"),
    ("misaligned_A", [{}, {"A": FAKE + 8}], {}, ARG, "operands must be 16-byte aligned"),
    ("misaligned_B", [{}, {"B": FAKE + 8}], {}, ARG, "operands must be 16-byte aligned"),
    ("misaligned_D", [{}, {"D": FAKE + 8}], {}, ARG, "operands must be 16-byte aligned"),
    ("lda_lt_K", [{}, {"lda": 240}], {}, ARG, "bad leading dimensions in problem 1"),
    ("ldb_lt_K", [{}, {"ldb": 240}], {}, ARG, "bad leading dimensions in problem 1"),
    ("ldd_lt_N", [{}, {"ldd": 252}], {}, ARG, "bad leading dimensions in problem 1"),
    ("lda_mod_16", [{}, {"lda": 264}], {}, ARG, "bad leading dimensions in problem 1"),
    ("ldd_mod_4", [{}, {"ldd": 258}], {}, ARG, "bad leading dimensions in problem 1"),
    ("K384", [{}, {"K": 384}], {}, ARG, FIT % (1, 256, 256, 384, 256, 256)),
    ("M200", [{"M": 200}, {}], {}, ARG, "no tile shape divides every problem"),
    ("M0", [{}, {"M": 0}], {}, ARG, FIT % (1, 0, 256, 256, 256, 256)),
    ("N0", [{}, {"N": 0}], {}, ARG, FIT % (1, 256, 0, 256, 256, 256)),
    ("M0_of_192", [{"M": 576, "N": 576}, {"M": 0, "N": 576}], {}, ARG, FIT % (1, 0, 576, 256, 192, 192)),
    ("K0", [{}, {"K": 0}], {}, ARG, FIT % (1, 256, 256, 0, 256, 256)),
    ("192_only_with_256_only", [{"M": 576, "N": 576}, {"M": 512, "N": 512}], {}, ARG, "no tile shape divides every problem"),
    ("cfg0_misfit", [{"M": 768, "N": 768}, {"M": 200, "N": 768}], dict(tile_cfg=0), ARG, FIT % (1, 200, 768, 256, 256, 256)),
    ("cfg1_misfit", [{"M": 768, "N": 768}, {"M": 200, "N": 768}], dict(tile_cfg=1), ARG, FIT % (1, 200, 768, 256, 256, 192)),
    ("cfg2_misfit", [{"M": 768, "N": 768}, {"M": 200, "N": 768}], dict(tile_cfg=2), ARG, FIT % (1, 200, 768, 256, 192, 256)),
    ("cfg3_misfit", [{"M": 768, "N": 768}, {"M": 200, "N": 768}], dict(tile_cfg=3), ARG, FIT % (1, 200, 768, 256, 192, 192)),
    ("cfg2_on_256", [{}], dict(tile_cfg=2), ARG, FIT % (0, 256, 256, 256, 192, 256)),
    ("w4_on_192_only", [{"K": 512}, {"M": 576, "N": 576, "K": 512}], dict(tile_cfg=4), ARG, FIT % (1, 576, 576, 512, 256, 256)),
    ("w4_K256", [{"K": 512}, {}], dict(tile_cfg=4), SHAPE,
     "mi_gemm_fp8_grouped (four-wave kernel): every problem needs K >= 512 and K % 256 == 0"),
    ("A_of_2GiB", [{}, {"K": BIG}], {}, ARG, "operands of problem 1 exceed 2 GiB (32-bit buffer offsets)"),
    ("A_of_2GiB_by_lda", [{}, {"M": BIG, "lda": 256}], {}, ARG, "operands of problem 1 exceed 2 GiB (32-bit buffer offsets)"),
    ("D_of_2GiB", [{}, {"M": 1 << 15, "N": 1 << 15}], {}, ARG, "operands of problem 1 exceed 2 GiB (32-bit buffer offsets)"),
    ("D_of_2GiB_by_ldd", [{}, {"M": 1 << 14, "ldd": 1 << 16}], {}, ARG, "operands of problem 1 exceed 2 GiB (32-bit buffer offsets)"),
    ("16384_tile_rows", [{"M": 1 << 22, "N": 192}], {}, ARG, "problem 0 has too many tiles per dimension"),
    # a defect in each of two problems of unequal K: the problem of the larger K is checked first, whatever its position
    ("two_defects_long_second", [{"A": None}, {"K": 512, "ldd": 252}], {}, ARG, "bad leading dimensions in problem 1"),
    ("two_defects_long_first", [{"K": 512, "A": None}, {"ldd": 252}], {}, ARG, "null pointer in problem 0"),
    ("two_defects_2GiB_then_null", [{"B": None}, {"K": BIG}], {}, ARG, "operands of problem 1 exceed 2 GiB (32-bit buffer offsets)"),
    ("two_defects_misfit_then_2GiB", [{"M": 200, "K": 1024}, {"K": 512, "M": 1 << 15, "N": 1 << 15}, {}], dict(tile_cfg=0), ARG,
     FIT % (0, 200, 256, 1024, 256, 256)),
    ("two_defects_equal_K_keep_caller_order", [{"D": FAKE + 8}, {"B": None}], {}, ARG, "operands must be 16-byte aligned"),
]


@pytest.mark.parametrize("probs,kw,rc,msg", [c[1:] for c in CASES], ids=[c[0] for c in CASES])
def test_per_tensor_refusal_code_and_text(probs, kw, rc, msg):
    want = msg if msg.startswith("mi_gemm_fp8_grouped") else P + msg
    assert _call(probs, **kw) == (rc, want)


def test_schedule_overflow_is_refused_by_both_entry_points_with_their_own_code():
    """More than 64 tiles per workgroup: the check sits in the code the two entry points share; each keeps its own return code."""
    from llm_fp8_amd import _lib
    lib = _lib.load()
    arr = (_lib.GemmMxProblem * 4)(*[_lib.GemmMxProblem(FAKE, FAKE, FAKE, FAKE, FAKE, 1 << 15, 1 << 14, 256)] * 4)
    rc = lib.mi_gemm_mxfp8_grouped(ctypes.byref(arr), 4, 0, 0, -1, None)
    assert (rc, lib.mi_last_error().decode()) == (SHAPE, "mi_gemm_mxfp8_grouped: more than 64 tiles per workgroup (32768 tiles in all)")
    assert _call([{"M": 1 << 15, "N": 1 << 14}] * 4) == (ARG, P + "more than 64 tiles per workgroup (32768 tiles in all)")
    arr = (_lib.GemmMxProblem * 1)(_lib.GemmMxProblem(FAKE, FAKE, FAKE, FAKE, FAKE, 1 << 22, 192, 256))
    rc = lib.mi_gemm_mxfp8_grouped(ctypes.byref(arr), 1, 0, 0, -1, None)
    assert (rc, lib.mi_last_error().decode()) == (SHAPE, "mi_gemm_mxfp8_grouped: problem 0 has too many tiles per dimension")
