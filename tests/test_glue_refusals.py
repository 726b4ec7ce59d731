"""CPU: the calls the RoPE, embedding-gradient, column-sum, RMSNorm-statistics and squared-norm entry points refuse are refused on
the host, before a launch, with MI_ERR_ARG and a non-empty mi_last_error(); rows == 0 is MI_OK.  Pointers are fake: nothing is
dereferenced and nothing is launched.  The return codes are pinned; a message is pinned only where it names the defect."""
import ctypes

import pytest

FAKE = 0x10000  # non-null, 16-byte aligned, never dereferenced: every case below returns before a launch
OK, ARG = 0, -1  # MI_OK, MI_ERR_ARG


def _lib():
    from llm_fp8_amd import _lib as L
    return L.load()


def _rope(**over):
    a = dict(fused=FAKE, q=FAKE, k=FAKE, v=FAKE, cos=FAKE, sin=FAKE, rows=64, seq=16, nq=2, nkv=1, D=128, backward=0)
    a.update(over)
    return _lib().mi_rope_qkv(a["fused"], a["q"], a["k"], a["v"], a["cos"], a["sin"], a["rows"], a["seq"], a["nq"], a["nkv"], a["D"],
                              a["backward"], None)


def _rope_cast(**over):
    a = dict(dq=FAKE, dk=FAKE, dv=FAKE, cos=FAKE, sin=FAKE, y=FAKE, yT=FAKE, scale=FAKE, amax=FAKE, rows=64, seq=16, nq=2, nkv=1,
             D=128, fmt=0)
    a.update(over)
    return _lib().mi_rope_qkv_bwd_cast(a["dq"], a["dk"], a["dv"], a["cos"], a["sin"], a["y"], a["yT"], a["scale"], a["amax"], a["rows"],
                                       a["seq"], a["nq"], a["nkv"], a["D"], a["fmt"], None)


def _rope_mx(**over):
    a = dict(rows=64, seq=16, nq=2, nkv=1, D=128, fmt=0)
    a.update(over)
    return _lib().mi_mxfp8_rope_bwd_quantize(FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, a["rows"], a["seq"], a["nq"], a["nkv"],
                                             a["D"], a["fmt"], None)


def _embedding(**over):
    a = dict(grad=FAKE, dy=FAKE, tokens=8, hidden=264, vocab=100)
    a.update(over)
    return _lib().mi_embedding_grad_add(a["grad"], a["dy"], FAKE, FAKE, a["tokens"], a["hidden"], a["vocab"], 1.0, -1, None)


def _finish(**over):
    a = dict(P=8, C=40, out_dtype=0)
    a.update(over)
    return _lib().mi_colsum_finish(FAKE, a["P"], a["C"], FAKE, a["out_dtype"], None)


def _finish_multi(n):
    parts = (ctypes.c_void_p * 5)(*[FAKE] * 5)
    outs = (ctypes.c_void_p * 5)(*[FAKE] * 5)
    Ps = (ctypes.c_int64 * 5)(*[8] * 5)
    Cs = (ctypes.c_int64 * 5)(*[40] * 5)
    dts = (ctypes.c_int * 5)(*[0] * 5)
    return _lib().mi_colsum_finish_multi(parts, Ps, Cs, outs, dts, n, None)


def _add_bias(**over):
    a = dict(bias=FAKE, rows=4, cols=512)
    a.update(over)
    return _lib().mi_add_bias_rmsnorm_stats(FAKE, FAKE, a["bias"], FAKE, FAKE, a["rows"], a["cols"], 1e-5, None)


CASES = [
    # (id, call, message fragment or None)
    ("rope_head_dim_24", lambda: _rope(D=24), "head_dim must be a multiple of 16"),
    ("rope_head_dim_0", lambda: _rope(D=0), "head_dim must be a multiple of 16"),
    ("rope_null_table", lambda: _rope(cos=None), "null pointer"),
    ("rope_table_at_4_bytes", lambda: _rope(sin=FAKE + 4), "16-byte aligned"),
    ("rope_seq_0", lambda: _rope(seq=0), None),
    ("rope_cast_head_dim_64", lambda: _rope_cast(D=64), "head_dim 64 not supported"),
    ("rope_cast_rows_12", lambda: _rope_cast(rows=12), "rows a multiple of 8"),
    ("rope_cast_no_output", lambda: _rope_cast(y=None, yT=None), "at least one of y, yT"),
    ("rope_cast_fmt_2", lambda: _rope_cast(fmt=2), "bad fmt 2"),
    ("rope_mx_head_dim_64", lambda: _rope_mx(D=64), "head_dim 64 not supported"),
    ("embedding_hidden_12", lambda: _embedding(hidden=12), "hidden a multiple of 8"),
    ("embedding_misaligned_grad", lambda: _embedding(grad=FAKE + 8), "misaligned"),
    ("finish_P_0", lambda: _finish(P=0), None),
    ("finish_out_dtype_2", lambda: _finish(out_dtype=2), "bad out_dtype 2"),
    ("finish_multi_n_0", lambda: _finish_multi(0), "1 to 4 finishes"),
    ("finish_multi_n_5", lambda: _finish_multi(5), "1 to 4 finishes"),
    ("add_bias_cols_12", lambda: _add_bias(cols=12), None),
    ("add_bias_null_bias", lambda: _add_bias(bias=None), "null pointer"),
    ("sumsq_multi_chunk_elems_12", lambda: _lib().mi_sumsq_bf16_multi(FAKE, 1, FAKE, 1, 12, FAKE, None), None),
]


@pytest.mark.parametrize("call,fragment", [c[1:] for c in CASES], ids=[c[0] for c in CASES])
def test_refused_on_the_host_with_err_arg(call, fragment):
    assert call() == ARG
    msg = _lib().mi_last_error().decode()
    assert msg and (fragment is None or fragment in msg), msg


@pytest.mark.parametrize("call", [
    lambda: _rope(rows=0), lambda: _rope(rows=0, backward=1), lambda: _rope_cast(rows=0), lambda: _rope_mx(rows=0),
    lambda: _embedding(tokens=0), lambda: _add_bias(rows=0),
    lambda: _lib().mi_add_rmsnorm_stats(FAKE, FAKE, FAKE, FAKE, 0, 512, 1e-5, None),
    lambda: _lib().mi_rmsnorm_stats(FAKE, FAKE, 0, 512, 1e-5, None),
    lambda: _lib().mi_adamw_bf16(FAKE, FAKE, FAKE, FAKE, 0, None, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1, None),
], ids=["rope_fwd", "rope_bwd", "rope_cast", "rope_mx", "embedding", "add_bias_stats", "add_stats", "stats", "adamw"])
def test_nothing_to_do_is_ok(call):
    assert call() == OK
