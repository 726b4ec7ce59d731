"""CPU: the grouped block-scaled GEMM entry point (mi_gemm_mxfp8_grouped, ABI 5) is declared, exported and bound; everything it
refuses is refused on the host, with the offending problem named and nothing dereferenced; the ops-level helpers that decide
between one grouped launch and two."""
import ctypes
import os
import re

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x10000  # non-null, 16-byte aligned, never dereferenced: every case below is refused before a launch
MI_ERR_ARG, MI_ERR_SHAPE = -1, -2


def _call(probs, fmt_a=0, fmt_b=0, tile_cfg=-1, n=None):
    """probs: list of dicts overriding the fields of a valid 256 x 256 x 256 problem."""
    from llm_fp8_amd import _lib
    lib = _lib.load()
    arr = (_lib.GemmMxProblem * max(len(probs), 1))()
    for i, over in enumerate(probs):
        f = dict(A=FAKE, SA=FAKE, B=FAKE, SB=FAKE, D=FAKE, M=256, N=256, K=256)
        f.update(over)
        arr[i] = _lib.GemmMxProblem(f["A"], f["SA"], f["B"], f["SB"], f["D"], f["M"], f["N"], f["K"])
    rc = lib.mi_gemm_mxfp8_grouped(ctypes.byref(arr), len(probs) if n is None else n, fmt_a, fmt_b, tile_cfg, None)
    return rc, lib.mi_last_error().decode()


def test_entry_point_is_declared_exported_and_bound_at_abi_5():
    from llm_fp8_amd import _lib
    src = open(os.path.join(ROOT, "include", "mi_fp8.h")).read()
    assert re.search(r"\bint\s+mi_gemm_mxfp8_grouped\s*\(\s*const\s+mi_gemm_mx_problem\s*\*", src)
    assert "typedef struct mi_gemm_mx_problem" in src
    lib = _lib.load()
    assert hasattr(lib, "mi_gemm_mxfp8_grouped")
    assert _lib.SIGNATURES["mi_gemm_mxfp8_grouped"] == _lib.SIGNATURES["mi_gemm_fp8_grouped"]
    m = re.search(r"#define\s+MI_ABI_VERSION\s+(\d+)", src)
    assert int(m.group(1)) == lib.mi_abi_version() == _lib.ABI_VERSION == 5
    # the structure the binding passes is the one the header lays out: five pointers, three int64
    assert [n for n, _ in _lib.GemmMxProblem._fields_] == ["A", "SA", "B", "SB", "D", "M", "N", "K"]
    assert ctypes.sizeof(_lib.GemmMxProblem) == 8 * 8


def test_number_of_problems_must_be_1_to_4():
    for n in (0, 5):
        rc, msg = _call([{}] * 4, n=n)
        assert rc == MI_ERR_ARG and "1 to 4 problems" in msg, (n, rc, msg)
    from llm_fp8_amd import _lib
    assert _lib.load().mi_gemm_mxfp8_grouped(None, 1, 0, 0, -1, None) == MI_ERR_ARG


def test_null_pointer_names_its_problem():
    for field in ("A", "SA", "B", "SB", "D"):
        rc, msg = _call([{}, {field: None}])
        assert rc == MI_ERR_ARG and "null pointer in problem 1" in msg, (field, rc, msg)


def test_shapes_no_tile_takes_are_refused():
    rc, msg = _call([{}, {"K": 384}])
    assert rc == MI_ERR_SHAPE and "problem 1" in msg and "K % 256" in msg, (rc, msg)
    rc, msg = _call([{"M": 200}, {}])
    assert rc == MI_ERR_SHAPE and "no tile shape divides problem 0" in msg, (rc, msg)
    rc, msg = _call([{"M": 576, "N": 576}, {"M": 512, "N": 512}])  # 192 only and 256 only: each has a tile, the group has none
    assert rc == MI_ERR_SHAPE and "no tile shape divides every one" in msg, (rc, msg)
    for cfg in (0, 1, 2, 3):  # an explicit tile shape names the problem it does not divide
        rc, msg = _call([{"M": 768, "N": 768}, {"M": 200, "N": 768}], tile_cfg=cfg)
        assert rc == MI_ERR_SHAPE and "problem 1" in msg and "does not fit tile shape" in msg, (cfg, rc, msg)
    # 256 divides, 192 does not: an explicit 192-row shape is refused, never replaced
    rc, msg = _call([{}], tile_cfg=2)
    assert rc == MI_ERR_SHAPE and "problem 0" in msg and "192 x 256" in msg, (rc, msg)


def test_misaligned_operands_are_refused():
    for field in ("A", "SA", "B", "SB", "D"):
        rc, msg = _call([{}, {field: FAKE + 8}])
        assert rc == MI_ERR_ARG and "problem 1" in msg and "16-byte aligned" in msg, (field, rc, msg)


def test_bad_format_and_tile_cfg_are_refused():
    for fa, fb in ((2, 0), (0, 2), (-1, 0)):
        rc, msg = _call([{}], fmt_a=fa, fmt_b=fb)
        assert rc == MI_ERR_ARG and "bad fmt" in msg, (fa, fb, rc, msg)
    rc, msg = _call([{}], tile_cfg=4)
    assert rc == MI_ERR_ARG and "tile_cfg 4" in msg and "four-wave" in msg, (rc, msg)
    for cfg in (5, -2):
        rc, msg = _call([{}], tile_cfg=cfg)
        assert rc == MI_ERR_ARG and "tile_cfg" in msg, (cfg, rc, msg)


def test_operands_of_2_gib_are_refused():
    big = 1 << 23  # 256 * 2^23 = 2^31 bytes
    for over in ({"K": big}, {"M": 1 << 15, "N": 1 << 15}):  # A and B of 2 GiB; an output of 2 GiB
        rc, msg = _call([{}, over])
        assert rc == MI_ERR_SHAPE and "problem 1" in msg and "2 GiB" in msg, (over, rc, msg)


def test_eligibility_of_the_3b_backward_pairs():
    """(dgrad, wgrad) of q|k|v, o-proj, fc1 and fc2 of Llama-3.2-3B at 8192 tokens, as module._MXQ.operands forms them for module._grouped_or_two."""
    from llm_fp8_amd.pytorch import ops
    M = 8192
    for k_in, n_out in ((3072, 5120), (3072, 3072), (3072, 16384), (8192, 3072)):
        assert ops.grouped_gemm_ok(((M, k_in, n_out), (n_out, k_in, M))), (k_in, n_out)
    assert not ops.grouped_gemm_ok(((64, 128, 96), (96, 128, 64)))       # no tile divides
    assert not ops.grouped_gemm_ok(((512, 512, 384), (384, 512, 512)))   # K % 256


def test_mx_and_per_tensor_groups_do_not_share_a_cache_entry():
    from llm_fp8_amd.pytorch import ops
    shapes = ((512, 768, 512), (768, 512, 512))
    saved = dict(ops._GROUP_TUNED)
    try:
        ops._GROUP_TUNED.clear()
        ops._GROUP_TUNED[(shapes, 1, 0)] = 4   # what grouped_gemm_autotune stores for the per-tensor group (4: the four-wave form)
        key = ops._tuned_key(shapes, 1, 0, True)
        assert ops._tuned_key(shapes, 1, 0, False) == (shapes, 1, 0)
        assert key != (shapes, 1, 0) and key not in ops._GROUP_TUNED
        ops._GROUP_TUNED[key] = 0
        # cached answers come back without touching the operands: meta tensors have no storage
        t = lambda r, c: torch.empty((r, c), dtype=torch.uint8, device="meta")
        o = lambda r, c: torch.empty((r, c), dtype=torch.bfloat16, device="meta")
        mx = [(t(M, K), t(K // 32, M), t(N, K), t(K // 32, N), o(M, N)) for M, N, K in shapes]
        pt = [(t(M, K), t(N, K), None, None, o(M, N)) for M, N, K in shapes]
        assert ops.grouped_gemm_autotune(mx, 1, 0, mx=True) == 0
        assert ops.grouped_gemm_autotune(pt, 1, 0) == 4
    finally:
        ops._GROUP_TUNED.clear()
        ops._GROUP_TUNED.update(saved)


def test_switch_off_returns_minus_one_without_touching_a_tensor(monkeypatch):
    from llm_fp8_amd.pytorch import ops
    monkeypatch.setenv("LLM_FP8_AMD_GROUPED_GEMM", "off")
    assert ops.grouped_gemm_choice([(None, None, None, None, None)] * 2, 1, 0, mx=True) == -1
    monkeypatch.setenv("LLM_FP8_AMD_GROUPED_GEMM", "plan")  # the count model: shapes only
    t = lambda r, c: torch.empty((r, c), dtype=torch.uint8, device="meta")
    shapes = ((8192, 3072, 8192), (8192, 3072, 8192))
    probs = [(t(M, K), None, t(N, K), None, None) for M, N, K in shapes]
    assert ops.grouped_gemm_choice(probs, 1, 0, mx=True) == ops.grouped_gemm_plan(shapes)
    assert ops.grouped_gemm_choice(probs, 1, 0, mx=True) in (-1, 0, 1, 2, 3)
