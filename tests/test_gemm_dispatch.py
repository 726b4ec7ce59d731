"""CPU: what an `algo` value of mi_gemm_fp8 / mi_gemm_mxfp8 / mi_gemm_fp8_clock means, pinned without a launch.
(a) Every refusal the three entry points issue after their argument checks, on the product library: return code and exact
    mi_last_error() text, and the order of the checks.  Pointers are fake: each case is refused before anything is launched.
(b) The plan of the accepted calls -- kernel family, build, tile shape, grid -- through the lab library's mi_gemm_plan_diag, which
    runs the same planner and never launches.  All algos give the same bits, so no output can show a wrong choice; this does.
    Without a GPU the CU count falls back to 256, the MI355X's, so the grids are the same on both machines."""
import ctypes
import os

import pytest

FAKE = 0x10000  # non-null, 16-byte aligned, never dereferenced
OK, ARG, SHAPE = 0, -1, -2
S = (256, 256, 512)
P8_NEEDS = "algo %d needs M,N %% 256 (or 192) == 0, K %% 256 == 0, bf16 output, operands < 2 GiB"
W4_NEEDS = "algo %d needs M,N,K %% 256 == 0, bf16 output, operands < 2 GiB"
FAST_NEEDS = "algo %d needs M,N %% 256 == 0 and K %% 128 == 0"
LAB = "algo %d is a timing / diagnostic build; it lives in the lab library (make -C llm_fp8_amd/csrc lab)"
W4P_SHAPE = "mi_gemm (w4 persistent): needs K >= 512, at most 64 tiles per workgroup and fewer than 16384 tiles per dimension"
SK_NEEDS = "mi_gemm: stream-K needs a registered workspace, 256-aligned M/N/K and more tiles than CUs (256 x 256 x 512)"
NO_TILE = "mi_gemm: no persistent tile shape divides 256 x 256"
W4_BIAS = "mi_gemm: of the four-wave kernels only the persistent one (algo 9) takes a bias (got algo 6)"
MX_ALGOS = "mi_gemm_mxfp8: algo must be 0, 1, 4, 5 or 40-45"

REFUSALS = [
    # (id, entry, shape (M, N, K), algo, keyword arguments, return code, text)
    ("fp8_forced_tile_misfit", "fp8", S, 41, {}, SHAPE, NO_TILE),
    ("fp8_streamk_no_workspace", "fp8", S, 44, {}, SHAPE, SK_NEEDS),
    ("fp8_unknown_48", "fp8", S, 48, {}, ARG, "mi_gemm_fp8: unknown algo 48"),
    ("fp8_unknown_99", "fp8", S, 99, {}, ARG, "mi_gemm_fp8: unknown algo 99"),
    ("fp8_unknown_minus1", "fp8", S, -1, {}, ARG, "mi_gemm_fp8: unknown algo -1"),
    ("fp8_unknown_31", "fp8", S, 31, {}, ARG, "mi_gemm_fp8: unknown algo 31"),
    ("fp8_lab_7", "fp8", S, 7, {}, ARG, "mi_gemm_fp8: " + LAB % 7),
    ("fp8_lab_23_undefined", "fp8", S, 23, {}, ARG, "mi_gemm_fp8: " + LAB % 23),
    ("fp8_lab_52_undefined", "fp8", S, 52, {}, ARG, "mi_gemm_fp8: " + LAB % 52),
    ("fp8_lab_before_shape", "fp8", (192, 256, 512), 7, {}, ARG, "mi_gemm_fp8: " + LAB % 7),
    ("fp8_p8_K384", "fp8", (256, 256, 384), 4, {}, SHAPE, "mi_gemm_fp8: " + P8_NEEDS % 4),
    ("fp8_p8_fp32_out", "fp8", S, 4, dict(out=1), SHAPE, "mi_gemm_fp8: " + P8_NEEDS % 4),
    ("fp8_p8_2GiB_by_lda", "fp8", S, 4, dict(lda=1 << 23), SHAPE, "mi_gemm_fp8: " + P8_NEEDS % 4),
    ("fp8_p8_per_tile_K384", "fp8", (256, 256, 384), 5, {}, SHAPE, "mi_gemm_fp8: " + P8_NEEDS % 5),
    ("fp8_streamk_K384", "fp8", (256, 256, 384), 44, {}, SHAPE, "mi_gemm_fp8: " + P8_NEEDS % 44),
    ("fp8_w4p_K256", "fp8", (256, 256, 256), 9, {}, SHAPE, W4P_SHAPE),
    ("fp8_w4p_M192", "fp8", (192, 256, 512), 9, {}, SHAPE, "mi_gemm_fp8: " + W4_NEEDS % 9),
    ("fp8_w4_bias", "fp8", S, 6, dict(bias=FAKE), ARG, W4_BIAS),
    ("fp8_w4_shape_before_bias", "fp8", (192, 256, 512), 6, dict(bias=FAKE), SHAPE, "mi_gemm_fp8: " + W4_NEEDS % 6),
    ("fp8_w4_M192", "fp8", (192, 256, 512), 6, {}, SHAPE, "mi_gemm_fp8: " + W4_NEEDS % 6),
    ("fp8_2ph_M192", "fp8", (192, 256, 512), 2, {}, SHAPE, "mi_gemm_fp8: " + FAST_NEEDS % 2),
    ("fp8_8ph_M192", "fp8", (192, 256, 512), 3, {}, SHAPE, "mi_gemm_fp8: " + FAST_NEEDS % 3),
    ("fp8_null_scale_before_algo", "fp8", S, 99, dict(scales=None), ARG, "mi_gemm_fp8: null scale pointer"),
    ("mx_algo_2", "mx", S, 2, {}, ARG, MX_ALGOS),
    ("mx_algo_9", "mx", S, 9, {}, ARG, MX_ALGOS),
    ("mx_algo_47", "mx", S, 47, {}, ARG, MX_ALGOS),
    ("mx_lab_18", "mx", S, 18, {}, ARG, MX_ALGOS),
    ("mx_K48", "mx", (256, 256, 48), 1, {}, ARG, "mi_gemm_mxfp8: K must be a multiple of 32"),
    ("mx_K_before_algo", "mx", (256, 256, 48), 99, {}, ARG, "mi_gemm_mxfp8: K must be a multiple of 32"),
    ("mx_algo_before_empty", "mx", (0, 256, 512), 2, {}, ARG, MX_ALGOS),
    ("mx_explicit_4_K384", "mx", (256, 256, 384), 4, {}, SHAPE, "mi_gemm_mxfp8: " + P8_NEEDS % 4),
    ("mx_explicit_4_fp32_out", "mx", S, 4, dict(out=1), SHAPE, "mi_gemm_mxfp8: " + P8_NEEDS % 4),
    ("mx_forced_tile_misfit", "mx", S, 41, {}, SHAPE, NO_TILE),
    ("mx_streamk_no_workspace", "mx", S, 44, {}, SHAPE, SK_NEEDS),
    ("mx_null_scale_before_algo", "mx", S, 99, dict(scales=None), ARG, "mi_gemm_mxfp8: null scale pointer"),
    ("clock_algo_1", "clock", S, 1, {}, ARG, "mi_gemm_fp8_clock: algo must be 0, 4 or 9"),
    ("clock_algo_5", "clock", S, 5, {}, ARG, "mi_gemm_fp8_clock: algo must be 0, 4 or 9"),
    ("clock_algo_before_empty", "clock", (0, 256, 512), 1, {}, ARG, "mi_gemm_fp8_clock: algo must be 0, 4 or 9"),
    ("clock_auto_K384", "clock", (256, 256, 384), 0, {}, SHAPE, "mi_gemm_fp8_clock: the shape does not run on a persistent kernel"),
    ("clock_auto_generic_shape", "clock", (264, 72, 48), 0, {}, SHAPE, "mi_gemm_fp8_clock: the shape does not run on a persistent kernel"),
    ("clock_p8_K384", "clock", (256, 256, 384), 4, {}, SHAPE, "mi_gemm_fp8_clock: " + P8_NEEDS % 4),
    ("clock_w4p_K256", "clock", (256, 256, 256), 9, {}, SHAPE, W4P_SHAPE),
    ("clock_w4p_M192", "clock", (192, 256, 512), 9, {}, SHAPE, "mi_gemm_fp8_clock: " + W4_NEEDS % 9),
    ("clock_null_stamps", "clock", S, 4, dict(stamps=None), ARG, "mi_gemm_fp8_clock: null pointer"),
]


def _call(lib, entry, shape, algo, bias=None, out=0, lda=None, scales=FAKE, stamps=FAKE, fa=0, fb=0):
    M, N, K = shape
    lda = K if lda is None else lda
    if entry == "fp8":
        rc = lib.mi_gemm_fp8(FAKE, FAKE, FAKE, scales, scales, bias, M, N, K, lda, K, N, fa, fb, out, algo, None)
    elif entry == "mx":
        rc = lib.mi_gemm_mxfp8(FAKE, scales, FAKE, scales, FAKE, bias, M, N, K, fa, fb, out, algo, None)
    else:
        rc = lib.mi_gemm_fp8_clock(FAKE, FAKE, FAKE, scales, scales, M, N, K, lda, K, N, algo, stamps, None)
    return rc, lib.mi_last_error().decode()


@pytest.mark.parametrize("case", REFUSALS, ids=[c[0] for c in REFUSALS])
def test_refusal_code_and_text(case):
    from llm_fp8_amd import _lib
    _, entry, shape, algo, kw, rc, text = case
    assert _call(_lib.load(), entry, shape, algo, **kw) == (rc, text)


def test_empty_output_is_ok_before_the_algo_is_looked_at():
    from llm_fp8_amd import _lib
    lib = _lib.load()
    for shape in ((0, 256, 512), (256, 0, 512)):
        for algo in (99, 7, 41, 0):
            assert _call(lib, "fp8", shape, algo)[0] == OK
        assert _call(lib, "mx", shape, 41)[0] == OK
        assert _call(lib, "clock", shape, 9)[0] == OK


# ---- (b) plans --------------------------------------------------------------------------------------------------------------
GENERIC, PH2, PH8, P8, STREAMK, W4, W4P = 1, 2, 3, 4, 5, 6, 7  # mi_gemm_plan.family
FIELDS = ("algo", "family", "build", "sched", "tile_cfg", "grid_x", "grid_y", "block", "one_tile_per_wg", "sk_units")
# shape (M, N, K[, lda]) -> algo -> FIELDS of the plan, or the return code.  Computed with the pick_algo, pick_tile_cfg and sk_units
# of the commit before the planner existed, and cross-checked against the launch site each call named there (no stream-K
# workspace can be registered without a GPU: 44 is refused).
PLANS = {
    (256, 256, 512): {
        0: (4, 4, 0, 0, 0, 1, 1, 512, 0, 0),
        47: (9, 7, 0, 0, 0, 1, 1, 256, 0, 0),
        4: (4, 4, 0, 0, 0, 1, 1, 512, 0, 0),
        5: (5, 4, 0, 0, 0, 1, 1, 512, 1, 0),
        6: (6, 6, 0, 0, 0, 1, 1, 256, 1, 0),
        9: (9, 7, 0, 0, 0, 1, 1, 256, 0, 0),
        40: (40, 4, 0, 0, 0, 1, 1, 512, 0, 0),
        41: -2,
        42: -2,
        43: -2,
        44: -2,
        45: (45, 4, 0, 0, 0, 1, 1, 512, 0, 0),
    },
    (256, 256, 256): {
        0: (4, 4, 0, 0, 0, 1, 1, 512, 0, 0),
        47: (4, 4, 0, 0, 0, 1, 1, 512, 0, 0),
        4: (4, 4, 0, 0, 0, 1, 1, 512, 0, 0),
        5: (5, 4, 0, 0, 0, 1, 1, 512, 1, 0),
        6: (6, 6, 0, 0, 0, 1, 1, 256, 1, 0),
        9: -2,
        40: (40, 4, 0, 0, 0, 1, 1, 512, 0, 0),
        41: -2,
        42: -2,
        43: -2,
        44: -2,
        45: (45, 4, 0, 0, 0, 1, 1, 512, 0, 0),
    },
    (256, 256, 384): {
        0: (3, 3, 0, 0, -1, 1, 1, 512, 0, 0),
        47: (3, 3, 0, 0, -1, 1, 1, 512, 0, 0),
        4: -2,
        5: -2,
        6: -2,
        9: -2,
        40: -2,
        41: -2,
        42: -2,
        43: -2,
        44: -2,
        45: -2,
    },
    (768, 768, 512): {
        0: (4, 4, 0, 0, 2, 12, 1, 512, 0, 0),
        47: (4, 4, 0, 0, 2, 12, 1, 512, 0, 0),
        4: (4, 4, 0, 0, 2, 12, 1, 512, 0, 0),
        5: (5, 4, 0, 0, 2, 12, 1, 512, 1, 0),
        6: (6, 6, 0, 0, 0, 9, 1, 256, 1, 0),
        9: (9, 7, 0, 0, 0, 9, 1, 256, 0, 0),
        40: (40, 4, 0, 0, 0, 9, 1, 512, 0, 0),
        41: (41, 4, 0, 0, 1, 12, 1, 512, 0, 0),
        42: (42, 4, 0, 0, 2, 12, 1, 512, 0, 0),
        43: (43, 4, 0, 0, 3, 16, 1, 512, 0, 0),
        44: -2,
        45: (45, 4, 0, 0, 2, 12, 1, 512, 0, 0),
    },
    (192, 576, 256): {
        0: (4, 4, 0, 0, 3, 3, 1, 512, 0, 0),
        47: (4, 4, 0, 0, 3, 3, 1, 512, 0, 0),
        4: (4, 4, 0, 0, 3, 3, 1, 512, 0, 0),
        5: (5, 4, 0, 0, 3, 3, 1, 512, 1, 0),
        6: -2,
        9: -2,
        40: -2,
        41: -2,
        42: -2,
        43: (43, 4, 0, 0, 3, 3, 1, 512, 0, 0),
        44: -2,
        45: (45, 4, 0, 0, 3, 3, 1, 512, 0, 0),
    },
    (264, 72, 48): {
        0: (1, 1, 0, 0, -1, 2, 5, 256, 0, 0),
        47: (1, 1, 0, 0, -1, 2, 5, 256, 0, 0),
        4: -2,
        5: -2,
        6: -2,
        9: -2,
        40: -2,
        41: -2,
        42: -2,
        43: -2,
        44: -2,
        45: -2,
    },
    (8192, 3072, 3072): {
        0: (4, 4, 0, 0, 0, 256, 1, 512, 0, 0),
        47: (9, 7, 0, 0, 0, 256, 1, 256, 0, 0),
        4: (4, 4, 0, 0, 0, 256, 1, 512, 0, 0),
        5: (5, 4, 0, 0, 0, 384, 1, 512, 1, 0),
        6: (6, 6, 0, 0, 0, 384, 1, 256, 1, 0),
        9: (9, 7, 0, 0, 0, 256, 1, 256, 0, 0),
        40: (40, 4, 0, 0, 0, 256, 1, 512, 0, 0),
        41: (41, 4, 0, 0, 1, 256, 1, 512, 0, 0),
        42: -2,
        43: -2,
        44: -2,
        45: (45, 4, 0, 0, 0, 256, 1, 512, 0, 0),
    },
    (8192, 3072, 8192): {
        0: (4, 4, 0, 0, 1, 256, 1, 512, 0, 0),
        47: (4, 4, 0, 0, 1, 256, 1, 512, 0, 0),
        4: (4, 4, 0, 0, 1, 256, 1, 512, 0, 0),
        5: (5, 4, 0, 0, 1, 512, 1, 512, 1, 0),
        6: (6, 6, 0, 0, 0, 384, 1, 256, 1, 0),
        9: (9, 7, 0, 0, 0, 256, 1, 256, 0, 0),
        40: (40, 4, 0, 0, 0, 256, 1, 512, 0, 0),
        41: (41, 4, 0, 0, 1, 256, 1, 512, 0, 0),
        42: -2,
        43: -2,
        44: -2,
        45: (45, 4, 0, 0, 1, 256, 1, 512, 0, 0),
    },
    (4352, 4096, 512): {
        0: (4, 4, 0, 0, 0, 256, 1, 512, 0, 0),
        47: (9, 7, 0, 0, 0, 256, 1, 256, 0, 0),
        4: (4, 4, 0, 0, 0, 256, 1, 512, 0, 0),
        5: (5, 4, 0, 0, 0, 272, 1, 512, 1, 0),
        6: (6, 6, 0, 0, 0, 272, 1, 256, 1, 0),
        9: (9, 7, 0, 0, 0, 256, 1, 256, 0, 0),
        40: (40, 4, 0, 0, 0, 256, 1, 512, 0, 0),
        41: -2,
        42: -2,
        43: -2,
        44: -2,
        45: (45, 4, 0, 0, 0, 256, 1, 512, 0, 0),
    },
    (256, 256, 512, 1 << 23): {
        0: (3, 3, 0, 0, -1, 1, 1, 512, 0, 0),
        47: (3, 3, 0, 0, -1, 1, 1, 512, 0, 0),
        4: -2,
        5: -2,
        6: -2,
        9: -2,
        40: -2,
        41: -2,
        42: -2,
        43: -2,
        44: -2,
        45: -2,
    },
}
# lab id -> (family, build, sched) on 256 x 256 x 512, E4M3 x E4M3, read off the launch chains of the same commit
BLOCK_EPILOGUE = 100
LAB_BUILDS = {7: (W4, 1, 0), 8: (W4, 2, 0), 10: (W4P, 1, 0), 11: (W4P, 2, 0), 12: (W4P, 3, 0), 13: (PH8, 1, 0), 14: (PH8, 2, 0),
              15: (P8, 1, 0), 16: (P8, 3, 0), 17: (P8, 4, 0), 20: (P8, 7, 0), 21: (P8, 8, 0), 22: (P8, 9, 0), 24: (P8, 11, 0),
              25: (P8, 12, 0), 26: (P8, 13, 0), 27: (P8, 14, 0), 28: (P8, 15, 0), 29: (P8, 16, 0), 30: (P8, 17, 0),
              46: (P8, BLOCK_EPILOGUE, 0), 54: (W4, 0, 1), 55: (W4, 1, 1), 56: (W4, 2, 1), 62: (W4, 0, 3), 63: (W4, 1, 3),
              64: (W4, 2, 3), 66: (W4, 0, 4), 67: (W4, 1, 4), 68: (W4, 2, 4), 70: (W4P, 4, 0), 71: (W4P, 5, 0), 72: (W4P, 6, 0),
              73: (W4P, 7, 0)}
STAMP_BUILDS = (8, 11, 14, 21, 22, 56, 64, 68, 73)  # the bias argument is a stamp buffer
FP8, MX, CLOCK = 0, 1, 2  # mi_gemm_plan_diag `entry`
TILE = {0: (256, 256), 1: (256, 192), 2: (192, 256), 3: (192, 192)}  # tile_cfg -> rows x columns of a persistent tile


@pytest.fixture(scope="module")
def plan():
    from llm_fp8_amd import _lib
    if not os.path.exists(_lib.LAB_LIB_PATH):
        pytest.skip("lab library not built")
    lab = ctypes.CDLL(_lib.LAB_LIB_PATH)  # loaded directly -- the package never does
    lab.mi_gemm_plan_diag.argtypes = _lib.LAB_SIGNATURES["mi_gemm_plan_diag"]
    lab.mi_last_error.restype = ctypes.c_char_p

    def query(entry, shape, algo, fa=0, fb=0, out=0, bias=0):
        M, N, K = shape[:3]
        p = _lib.GemmPlan()
        rc = lab.mi_gemm_plan_diag(entry, M, N, K, shape[3] if len(shape) > 3 else K, K, N, fa, fb, out, bias, algo, ctypes.byref(p))
        return rc, p, lab.mi_last_error().decode()
    return query


@pytest.mark.parametrize("shape", list(PLANS), ids=["x".join(map(str, s)) for s in PLANS])
def test_plan_of_the_product_algos(plan, shape):
    for algo, want in PLANS[shape].items():
        rc, p, text = plan(FP8, shape, algo)
        if isinstance(want, int):
            assert rc == want, (algo, text)
        else:
            assert rc == OK, (algo, text)
            assert tuple(getattr(p, f) for f in FIELDS) == want, algo
            assert (p.bias_use, p.mx) == (0, 0), algo
            bm, bn = TILE[p.tile_cfg] if p.family == P8 else (256, 256)  # the tiles the kernel is told to walk
            assert p.family == GENERIC or (p.tiles_m * bm, p.tiles_n * bn) == shape[:2], algo


def test_plan_of_the_lab_builds(plan):
    for algo, want in LAB_BUILDS.items():
        rc, p, text = plan(FP8, S, algo)
        assert rc == OK, (algo, text)
        assert (p.algo, p.family, p.build, p.sched) == (algo,) + want, algo
        assert p.bias_use == (2 if algo in STAMP_BUILDS else 0), algo
    for algo, build in ((18, 5), (19, 6)):  # the MX scale path without its effect: block-scaled only
        rc, p, text = plan(MX, S, algo)
        assert (rc, p.family, p.build, p.mx) == (OK, P8, build, 1), (algo, text)
        # through mi_gemm_fp8 the scale pointers are null and the kernel would fault: refused, nothing launched
        rc, _, text = plan(FP8, S, algo)
        assert (rc, text) == (ARG, f"mi_gemm: diagnostic algo {algo} reads MXFP8 block scales: call it through mi_gemm_mxfp8")


def test_plan_refusals_of_the_lab_library(plan):
    assert plan(FP8, (256, 256, 256), 29)[::2] == (SHAPE, "mi_gemm: algo 29 needs K >= 512")
    assert plan(FP8, S, 27, fa=1)[::2] == (ARG, "mi_gemm: diagnostic algo 27 is built for E4M3 x E4M3 only")
    assert plan(FP8, S, 11, fa=1)[::2] == (ARG, "mi_gemm (w4): the clock-stamp build is E4M3 x E4M3 only")
    assert plan(FP8, S, 23)[::2] == (ARG, "mi_gemm: unknown diagnostic algo 23")
    assert plan(FP8, S, 52)[::2] == (ARG, "mi_gemm (w4): no such schedule variant 22")
    assert plan(FP8, S, 99)[::2] == (ARG, "mi_gemm_fp8: unknown algo 99")
    assert plan(MX, S, 9)[::2] == (ARG, "mi_gemm_mxfp8: algo must be 0, 1, 4, 5, 18, 19 or 40-45")
    assert plan(FP8, (256, 256, 24), 0)[::2] == (ARG, "mi_gemm_fp8: M,N must be multiples of 8 and K of 16 (got 256,256,24)")
    assert plan(FP8, (256, 256, 512, 500), 0)[::2] == (ARG, "mi_gemm_fp8: bad leading dimensions")


def test_plan_of_an_empty_output_is_nothing_whatever_the_algo(plan):
    for algo in (99, 7, 41, 0):
        rc, p, _ = plan(FP8, (0, 256, 512), algo)
        assert (rc, p.family) == (OK, 0), algo


def test_plan_of_bias_block_scales_and_the_clock_entry(plan):
    for algo, family in ((4, P8), (9, W4P), (3, PH8), (1, GENERIC)):
        rc, p, text = plan(FP8, S, algo, bias=1)
        assert (rc, p.family, p.bias_use) == (OK, family, 1), (algo, text)
    # block-scaled auto: the persistent kernel, else the generic one (never the eight-phase kernel)
    for shape, want in ((S, (4, P8, 0)), ((8192, 3072, 8192), (4, P8, 1)), ((256, 256, 384), (1, GENERIC, -1)), ((264, 72, 64), (1, GENERIC, -1))):
        rc, p, text = plan(MX, shape, 0)
        assert (rc, p.algo, p.family, p.tile_cfg, p.mx) == (OK,) + want + (1,), (shape, text)
    # fp32 output: only the generic, two-phase and eight-phase kernels
    assert plan(FP8, S, 0, out=1)[1].family == PH8 and plan(FP8, S, 47, out=1)[1].family == PH8
    assert plan(FP8, (264, 72, 48), 0, out=1)[1].family == GENERIC
    # mi_gemm_fp8_clock: the stamped builds of the two persistent product kernels, same grid and tile shape
    for algo, want in ((0, (4, P8, 8, 0, 256)), (4, (4, P8, 8, 0, 256)), (9, (9, W4P, 2, 0, 256))):
        rc, p, text = plan(CLOCK, (8192, 3072, 3072), algo)
        assert (rc, p.algo, p.family, p.build, p.tile_cfg, p.grid_x, p.bias_use) == (OK,) + want + (2,), (algo, text)
