"""CPU: what mi_qknorm_rope_qkv / mi_qknorm_rope_qkv_bwd refuse is refused on the host, before a launch, with MI_ERR_ARG and a
mi_last_error() that names the entry point; header, library and binding agree on the two symbols and on revision 6; the TE surface
refuses the QK-norm arguments it does not implement.  Pointers are fake: nothing is dereferenced and nothing is launched."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x10000  # non-null, 16-byte aligned, never dereferenced: every case below returns before a launch
ARG = -1        # MI_ERR_ARG
FWD_PTRS = ("fused", "q", "k", "v", "gamma_q", "gamma_k", "rstd", "cos", "sin")
BWD_PTRS = ("dq", "dk", "dv", "fused_x", "rstd", "gamma_q", "gamma_k", "cos", "sin", "dfused", "partial")


def _L():
    from llm_fp8_amd import _lib as L
    return L


def _fwd(**over):
    a = dict({p: FAKE for p in FWD_PTRS}, rows=64, seq=16, nq=2, nkv=1, D=128, eps=1e-6)
    a.update(over)
    return _L().load().mi_qknorm_rope_qkv(*[a[p] for p in FWD_PTRS], a["rows"], a["seq"], a["nq"], a["nkv"], a["D"], a["eps"], None)


def _bwd(**over):
    a = dict({p: FAKE for p in BWD_PTRS}, n_partials=4, rows=64, seq=16, nq=2, nkv=1, D=128)
    a.update(over)
    return _L().load().mi_qknorm_rope_qkv_bwd(*[a[p] for p in BWD_PTRS], a["n_partials"], a["rows"], a["seq"], a["nq"], a["nkv"], a["D"], None)


def _refused(rc, who, word=None):
    msg = _L().load().mi_last_error().decode()
    assert rc == ARG and msg.startswith(who + ":"), (rc, msg)
    if word is not None:
        assert word in msg, msg


@pytest.mark.parametrize("call,ptrs,who", [(_fwd, FWD_PTRS, "mi_qknorm_rope_qkv"), (_bwd, BWD_PTRS, "mi_qknorm_rope_qkv_bwd")],
                         ids=["forward", "backward"])
def test_host_refusals(call, ptrs, who):
    for p in ptrs:
        _refused(call(**{p: None}), who, "null")
        _refused(call(**{p: FAKE + 8}), who, "aligned")
    for D in (0, 16, 32, 96, 256, -128):
        _refused(call(D=D), who, "head_dim")
    _refused(call(rows=1 << 31), who, "rows")
    _refused(call(rows=-1), who)
    for seq in (0, -5):
        _refused(call(seq=seq), who, "seq")
    _refused(call(nq=0), who)
    _refused(call(nkv=0), who)


def test_forward_refuses_a_bad_eps_and_takes_no_rows():
    for eps in (-1e-6, float("inf"), float("-inf"), float("nan")):
        _refused(_fwd(eps=eps), "mi_qknorm_rope_qkv", "eps")
    assert _fwd(rows=0) == 0  # nothing to do: MI_OK, nothing launched
    assert _fwd(rows=0, eps=0.0, D=64) == 0


def test_backward_refuses_no_partials():
    for n in (0, -3):
        _refused(_bwd(n_partials=n), "mi_qknorm_rope_qkv_bwd", "n_partials")


def test_header_library_and_binding_agree_on_revision_6():
    L = _L()
    lib = L.load()
    src = open(os.path.join(ROOT, "include", "mi_fp8.h")).read()
    assert int(re.search(r"#define\s+MI_ABI_VERSION\s+(\d+)", src).group(1)) == lib.mi_abi_version() == L.ABI_VERSION == 5
    assert int(re.search(r"#define\s+MI_ABI_REVISION\s+(\d+)", src).group(1)) == lib.mi_abi_revision() == L.ABI_REVISION
    assert L.ABI_REVISION >= 6
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name, n_args in (("mi_qknorm_rope_qkv", 16), ("mi_qknorm_rope_qkv_bwd", 18)):
        decl = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", code)
        assert decl is not None, f"{name} is not declared in include/mi_fp8.h"
        assert len(decl.group(1).split(",")) == n_args == len(L.SIGNATURES[name])
        assert name in L.REVISION_SIGNATURES and hasattr(lib, name)


def test_multihead_attention_refuses_unbuilt_qk_norm_arguments():
    import llm_fp8_amd.pytorch as te
    kw = dict(hidden_size=64, num_attention_heads=2, kv_channels=32, bias=False, qkv_format="bshd", device="cpu")
    with pytest.raises(NotImplementedError, match="qk_norm_type"):
        te.MultiheadAttention(qk_norm_type="LayerNorm", **kw)
    with pytest.raises(NotImplementedError, match="qk_norm_type"):
        te.MultiheadAttention(qk_norm_type="L2Normalization", **kw)
    with pytest.raises(NotImplementedError, match="qk_norm_before_rope"):
        te.MultiheadAttention(qk_norm_type="RMSNorm", qk_norm_before_rope=False, **kw)
    m = te.MultiheadAttention(qk_norm_type="RMSNorm", qk_norm_eps=1e-6, **kw)
    assert tuple(m.q_norm.weight.shape) == tuple(m.k_norm.weight.shape) == (32,) and m.q_norm.eps == 1e-6
    plain = te.MultiheadAttention(**kw)
    assert not hasattr(plain, "q_norm") and not any("norm" in n and "layer" not in n for n, _ in plain.named_parameters())
