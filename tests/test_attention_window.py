"""CPU: the sliding-window attention surface.  Header, library and binding agree on revision 9 and the two `_win` entry points;
what they refuse is refused on the host, before a launch, under the entry point's name (fake pointers: nothing is dereferenced);
ops.attn_window_walk against counts read off the band mask; DotProductAttention's `window_size` follows TE's (left, right) on the SDPA route against a float64 band softmax; the Qwen3 layers
and train.TrainingConfig carry the window where the config says so."""
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x10000  # non-null, 16-byte aligned, never dereferenced: every case below returns before a launch
ARG = -1        # MI_ERR_ARG
FWD_PTRS = ("q", "k", "v", "o", "lse")
BWD_PTRS = ("q", "k", "v", "o", "dout", "lse", "delta", "dq", "dk", "dv")


def _L():
    from llm_fp8_amd import _lib as L
    return L


def _call(name, ptrs, strides, **over):
    a = dict({p: FAKE for p in ptrs}, B=1, S=256, H=4, G=2, D=64, scale=0.125, causal=1, window=32, **{s: 512 for s in strides})
    a.update(over)
    fn = getattr(_L().load(), name)
    return fn(*[a[p] for p in ptrs], a["B"], a["S"], a["H"], a["G"], a["D"], *[a[s] for s in strides], a["scale"], a["causal"],
              a["window"], None)


def _fwd(**over):
    return _call("mi_attn_fwd_win", FWD_PTRS, ("q_ts", "k_ts", "v_ts", "o_ts"), **over)


def _bwd(**over):
    return _call("mi_attn_bwd_win", BWD_PTRS, ("q_ts", "k_ts", "v_ts", "o_ts", "do_ts", "dq_ts", "dk_ts", "dv_ts"), **over)


def test_header_library_and_binding_agree_on_revision_9():
    L = _L()
    lib = L.load()
    src = open(os.path.join(ROOT, "include", "mi_fp8.h")).read()
    assert int(re.search(r"#define\s+MI_ABI_REVISION\s+(\d+)", src).group(1)) == lib.mi_abi_revision() == L.ABI_REVISION >= 9
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name, base in (("mi_attn_fwd_win", "mi_attn_fwd"), ("mi_attn_bwd_win", "mi_attn_bwd")):
        decl = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", code)
        assert decl is not None, f"{name} is not declared in include/mi_fp8.h"
        params = [p.strip() for p in decl.group(1).split(",")]
        assert params[-2:] == ["int window", "void* stream"], params[-2:]
        # the base entry point's argument list with `window` in front of the stream
        assert L.SIGNATURES[name] == L.SIGNATURES[base][:-1] + [L._c_int, L._p] and len(params) == len(L.SIGNATURES[name])
        assert name in L.REVISION_SIGNATURES and getattr(lib, name).argtypes == L.SIGNATURES[name]


@pytest.mark.parametrize("call,ptrs,who", [(_fwd, FWD_PTRS, "mi_attn_fwd_win"), (_bwd, BWD_PTRS, "mi_attn_bwd_win")],
                         ids=["forward", "backward"])
def test_host_refusals(call, ptrs, who):
    def refused(rc, word):
        msg = _L().load().mi_last_error().decode()
        assert rc == ARG and msg.startswith(who + ":") and word in msg, (rc, msg)

    for window in (0, -1, -(2 ** 31)):
        refused(call(window=window), "window")
    refused(call(causal=0), "causal")
    for S in (0, 64, 112, 120, 136, 200):
        refused(call(S=S), "seq")
    for p in ptrs:
        refused(call(**{p: None}), "null")
        if p not in ("lse", "delta"):
            refused(call(**{p: FAKE + 8}), "aligned")
    for D in (0, 32, 96, 256):
        refused(call(D=D), "head_dim")
    refused(call(H=4, G=3), "B/H/G")
    refused(call(B=0), "B/H/G")
    refused(call(q_ts=516), "strides")
    refused(call(k_ts=1 << 23), "2 GiB")
    refused(call(H=65536, G=1), "grid")


@pytest.mark.parametrize("S", [128, 256, 400, 1024, 1040])
def test_attn_window_walk_against_the_band_mask(S):
    """ops.attn_window_walk for every 128-row block against counts read off the boolean band mask itself."""
    from llm_fp8_amd.pytorch import ops
    i = np.arange(S)
    windows = {1, 2, 17, 32, 33, 63, 64, 65, 70, 96, 100, 127, 128, 129, 192, 193, 300, 513, 1000, S - 129, S - 1}
    for W in sorted(w for w in windows if 0 < w < S):  # (a window of S or more is the plain causal call)
        mask = (i[None, :] <= i[:, None]) & (i[None, :] > i[:, None] - W)  # [query, key]
        for block in range(-(-S // 128)):
            rows = slice(128 * block, min(128 * block + 128, S))
            keys = np.flatnonzero(mask[rows].any(0))          # keys some query row of the block sees
            j0 = int(keys[0]) // 64                           # first 64-key tile with a visible key
            diag = min(128 * block + 127, S - 1) // 64        # the diagonal tile, clamped to the row
            queries = np.flatnonzero(mask[:, rows].any(1))    # queries that see some key of the block
            slices = int(queries[-1]) // 32 - 4 * block + 1   # from the key block's first slice through the last one that sees it
            assert int(queries[0]) // 32 == 4 * block
            assert ops.attn_window_walk(S, W, block) == (j0, diag - j0 + 1, slices), (S, W, block)


def _band_f64(q, k, v, W):
    """float64 softmax attention over the causal band of W keys; q [B,S,H,D], k/v [B,S,G,D] -> [B,S,H*D]."""
    q, k, v = (t.double().numpy() for t in (q, k, v))
    B, S, H, D = q.shape
    k, v = (np.repeat(t, H // t.shape[2], axis=2) for t in (k, v))
    s = np.einsum("bihd,bjhd->bhij", q, k) * D ** -0.5
    i = np.arange(S)
    s = np.where((i[None, :] <= i[:, None]) & (i[None, :] > i[:, None] - W), s, -np.inf)
    p = np.exp(s - s.max(-1, keepdims=True))
    return np.einsum("bhij,bjhd->bihd", p / p.sum(-1, keepdims=True), v).reshape(B, S, H * D)


@pytest.mark.parametrize("window_size,W", [(None, 40), ((-1, 0), 40), ((-1, -1), 40), ((0, 0), 1), ((6, 0), 7), ((6, -1), 7),
                                           ((39, 0), 40), ((100, 0), 40)])
def test_dot_product_attention_window_size_on_cpu(window_size, W):
    from llm_fp8_amd.pytorch import attention as A
    B, S, H, G, D = 2, 40, 4, 2, 16
    g = torch.Generator().manual_seed(S + W)
    q, k, v = (torch.randn(B, S, n, D, generator=g) for n in (H, G, G))
    core = A.DotProductAttention(H, D, G, attention_dropout=0.0, attn_mask_type="causal", qkv_format="bshd", window_size=window_size)
    assert core.window_size == (None if window_size is None or window_size[0] < 0 else tuple(window_size))
    np.testing.assert_allclose(core(q, k, v).double().numpy(), _band_f64(q, k, v, W), rtol=1e-5, atol=1e-5)  # float32 SDPA


def test_window_size_refusals_and_multihead_pass_through():
    import llm_fp8_amd.pytorch as te
    from llm_fp8_amd.pytorch import attention as A
    for ws in ((8, 1), (8, 8), (-1, 3)):
        with pytest.raises(ValueError, match="right"):
            A.DotProductAttention(4, 16, 2, attn_mask_type="causal", window_size=ws)
    with pytest.raises(NotImplementedError, match="two-sided"):
        A.DotProductAttention(4, 16, 2, attn_mask_type="no_mask", window_size=(8, 8))
    kw = dict(hidden_size=64, num_attention_heads=2, kv_channels=32, bias=False, qkv_format="bshd", device="cpu")
    assert te.MultiheadAttention(window_size=(7, 0), **kw).core_attention.window_size == (7, 0)
    assert te.MultiheadAttention(**kw).core_attention.window_size is None


TINY = dict(num_hidden_layers=3, hidden_size=64, intermediate_size=128, num_attention_heads=4, num_key_value_heads=2, head_dim=16,
            vocab_size=128, max_position_embeddings=64)


def test_qwen3_layers_carry_the_window_of_their_layer_type():
    from llm_fp8_amd import qwen
    cfg = qwen.qwen3_config("qwen3-0.6b", use_sliding_window=True, sliding_window=24, max_window_layers=1, **TINY)
    layers = [qwen.TEQwen3DecoderLayer(cfg, i) for i in range(3)]
    assert [m.self_attention.core_attention.window_size for m in layers] == [None, (23, 0), (23, 0)]
    if getattr(cfg, "layer_types", None) is not None:  # `layer_types` wins over max_window_layers where transformers has it
        cfg.layer_types = ["sliding_attention", "full_attention", "sliding_attention"]
        assert [qwen.TEQwen3DecoderLayer(cfg, i).self_attention.core_attention.window_size for i in range(3)] == [(23, 0), None, (23, 0)]
    with pytest.raises(ValueError, match="layer_idx"):
        qwen.TEQwen3DecoderLayer(cfg)
    with pytest.raises(NotImplementedError, match="use_sliding_window=True selects no sliding layer"):
        qwen.TEQwen3DecoderLayer(qwen.qwen3_config("qwen3-0.6b", use_sliding_window=True, sliding_window=24, max_window_layers=3, **TINY), 0)
    plain = qwen.qwen3_config("qwen3-0.6b", **TINY)
    assert not plain.use_sliding_window and qwen.TEQwen3DecoderLayer(plain, 2).self_attention.core_attention.window_size is None


@pytest.mark.parametrize("name", ["qwen3-0.6b", "llama-3.2-1b"])
def test_training_config_sliding_window_reaches_every_layer(monkeypatch, name):
    from llm_fp8_amd import llama, qwen, train
    assert train.config_from_args(train.build_arg_parser().parse_args(["--sliding_window", "48"])).sliding_window == 48
    assert train.TrainingConfig().sliding_window is None
    # full-size layers would take seconds to build on a CPU: the two config makers get the TINY widths underneath the overrides
    for mod, fn in ((qwen, "qwen3_config"), (llama, "llama_config")):
        monkeypatch.setattr(mod, fn, lambda n, _make=getattr(mod, fn), **over: _make(n, **{**TINY, **over}))
    cfg = train.TrainingConfig(model_name=name, use_te=True, num_hidden_layers=2, sliding_window=48)
    model = train.create_model(cfg, "cpu")
    assert model.config.sliding_window == 48 and len(model.model.layers) == 2
    assert [m.self_attention.core_attention.window_size for m in model.model.layers] == [(47, 0), (47, 0)]
