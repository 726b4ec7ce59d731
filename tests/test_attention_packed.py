"""CPU: the packed-sequence attention surface.  Revision 10 and the two `_seg` entry points; their refusals on the host (fake
pointers: nothing is dereferenced); ops.attn_segments against a plain loop; the SDPA document-mask route of DotProductAttention
against per-document SDPA, with a window as well; what the module and the decoder layer refuse; the attention._segments cache; and
train.pack_batch / synthetic_batch(packed_docs=) / --packed_docs against a loop."""
import os
import re

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x10000  # non-null, 16-byte aligned, never dereferenced: every case below returns before a launch


def test_revision_10_exports_the_seg_entry_points():
    from llm_fp8_amd import _lib as L
    lib = L.load()
    src = open(os.path.join(ROOT, "include", "mi_fp8.h")).read()
    assert int(re.search(r"#define\s+MI_ABI_REVISION\s+(\d+)", src).group(1)) == lib.mi_abi_revision() == L.ABI_REVISION >= 10
    for name, base in (("mi_attn_fwd_seg", "mi_attn_fwd"), ("mi_attn_bwd_seg", "mi_attn_bwd")):
        assert re.search(r"\bint\s+" + name + r"\s*\(", src), f"{name} is not declared in include/mi_fp8.h"
        assert L.REVISION_SIGNATURES[name] == L.SIGNATURES[base][:-1] + [L._p, L._p, L._p] == getattr(lib, name).argtypes


@pytest.mark.parametrize("name,nptr,nstride", [("mi_attn_fwd_seg", 5, 4), ("mi_attn_bwd_seg", 10, 8)])
def test_host_refusals(name, nptr, nstride):
    from llm_fp8_amd import _lib as L

    def rc(S=256, causal=1, seg=(FAKE, FAKE)):
        return getattr(L.load(), name)(*[FAKE] * nptr, 1, S, 4, 2, 64, *[512] * nstride, 0.125, causal, *seg, None)

    for kw, word in ((dict(seg=(None, FAKE)), "null"), (dict(seg=(FAKE, None)), "null"), (dict(seg=(FAKE + 2, FAKE)), "aligned"),
                     (dict(causal=0), "causal"), (dict(S=64), "seq")):
        got, msg = rc(**kw), L.load().mi_last_error().decode()
        assert got == -1 and msg.startswith(name + ":") and word in msg, (got, msg)  # MI_ERR_ARG


@pytest.mark.parametrize("cu,B,S", [([0, 5, 6, 16], 1, 16), ([0, 3, 11], 1, 16), ([0, 10, 20, 29], 2, 16)])
def test_attn_segments_against_a_loop(cu, B, S):
    from llm_fp8_amd.pytorch import ops
    cuts = sorted(set(cu) | set(range(0, B * S + 1, S)))  # a short tail is one more document; a row end ends a document
    start, end = [], []
    for t in range(B * S):
        lo = max(c for c in cuts if c <= t)
        start.append(lo - t // S * S)
        end.append(min(c for c in cuts if c > t) - t // S * S)
    for dtype in (torch.int32, torch.int64):
        got = ops.attn_segments(torch.tensor(cu, dtype=dtype), B, S)
        assert all(g.dtype == torch.int32 and g.shape == (B, S) for g in got)
        assert got[0].flatten().tolist() == start and got[1].flatten().tolist() == end


def test_packed_refusals():
    from llm_fp8_amd.pytorch import attention as A, ops
    from llm_fp8_amd import llama
    q = torch.zeros(1, 128, 2, 64, dtype=torch.bfloat16)
    seg = ops.attn_segments(torch.tensor([0, 128]), 1, 128)
    with pytest.raises(ValueError, match="window"):
        ops.attn_fwd(q, q, q, 0.125, True, window=16, segments=seg)
    with pytest.raises(ValueError, match="window"):
        ops.attn_bwd(q, q, q, q, q, torch.zeros(1, 2, 128), 0.125, True, window=16, segments=seg)
    core = A.DotProductAttention(2, 64, 2, attention_dropout=0.0)
    cu = torch.tensor([0, 50, 128])
    with pytest.raises(NotImplementedError, match="cu_seqlens_kv"):
        core(q, q, q, cu_seqlens_q=cu, cu_seqlens_kv=cu.clone())
    with pytest.raises(ValueError, match="batch of 2"):
        core(q.expand(2, -1, -1, -1), q.expand(2, -1, -1, -1), q.expand(2, -1, -1, -1), cu_seqlens_q=cu)
    cfg = llama.llama_config("llama-3.2-1b", num_hidden_layers=1, hidden_size=64, intermediate_size=128, num_attention_heads=4,
                             num_key_value_heads=2, head_dim=16, vocab_size=128, max_position_embeddings=64)
    layer = llama.TELlamaDecoderLayer(cfg).to("cpu")
    with pytest.raises(ValueError, match="batch of 2"):
        layer(torch.zeros(2, 32, 64), cu_seq_lens_q=torch.tensor([0, 20, 64]))


@pytest.mark.parametrize("fmt", ["bshd", "sbhd", "thd"])
def test_dot_product_attention_packed_on_cpu_is_per_document_sdpa(fmt):
    from llm_fp8_amd.pytorch import attention as A
    T, H, G, D, lens = 48, 4, 2, 16, [17, 1, 30]
    g = torch.Generator().manual_seed(3)
    q, k, v = (torch.randn(T, n, D, generator=g) for n in (H, G, G))
    cu = torch.tensor([0, 17, 18, 48], dtype=torch.int32)
    shape = {"bshd": lambda t: t.unsqueeze(0), "sbhd": lambda t: t.unsqueeze(1), "thd": lambda t: t}[fmt]
    out = A.DotProductAttention(H, D, G, attention_dropout=0.0, qkv_format=fmt)(shape(q), shape(k), shape(v), cu_seqlens_q=cu,
                                                                                 cu_seqlens_kv=cu, max_seqlen_q=30, max_seqlen_kv=30)
    ref = torch.cat([F.scaled_dot_product_attention(*(t.transpose(0, 1) for t in doc), is_causal=True, enable_gqa=True).transpose(0, 1)
                     for doc in zip(*(t.split(lens) for t in (q, k, v)))]).reshape(T, H * D)
    assert out.shape == shape(ref).shape
    torch.testing.assert_close(out.reshape(T, H * D), ref, rtol=1e-5, atol=1e-5)  # float32 SDPA both ways


def test_packed_with_a_window_on_cpu_is_per_document_band_sdpa():
    """cu_seqlens_q together with window_size: the document mask AND the band, against SDPA on each document alone under that
    document's own band mask."""
    from llm_fp8_amd.pytorch import attention as A
    T, H, G, D, lens, W = 48, 4, 2, 16, [17, 1, 30], 5
    g = torch.Generator().manual_seed(4)
    q, k, v = (torch.randn(T, n, D, generator=g) for n in (H, G, G))
    cu = torch.tensor([0, 17, 18, 48], dtype=torch.int32)

    def band(n):
        d = torch.arange(n)[:, None] - torch.arange(n)[None, :]
        return (d >= 0) & (d < W)

    ref = torch.cat([F.scaled_dot_product_attention(*(t.transpose(0, 1) for t in doc), attn_mask=band(doc[0].shape[0]),
                                                    enable_gqa=True).transpose(0, 1)
                     for doc in zip(*(t.split(lens) for t in (q, k, v)))]).reshape(T, H * D)
    plain = A.DotProductAttention(H, D, G, attention_dropout=0.0, qkv_format="thd")(q, k, v, cu_seqlens_q=cu)
    assert (plain - ref).abs().max() > 1e-2  # the band is live: 5 keys against documents of 17 and 30
    for fmt, shape in (("bshd", lambda t: t.unsqueeze(0)), ("thd", lambda t: t)):
        core = A.DotProductAttention(H, D, G, attention_dropout=0.0, qkv_format=fmt, window_size=(W - 1, 0))
        out = core(shape(q), shape(k), shape(v), cu_seqlens_q=cu, cu_seqlens_kv=cu, max_seqlen_q=30, max_seqlen_kv=30)
        assert out.shape == shape(ref).shape
        torch.testing.assert_close(out.reshape(T, H * D), ref, rtol=1e-5, atol=1e-5)  # float32 SDPA both ways


def test_segments_cache_follows_the_tensor_its_version_and_the_length():
    from llm_fp8_amd.pytorch import attention as A, ops

    def same(got, cu, T):
        return all(torch.equal(a, b) for a, b in zip(got, ops.attn_segments(cu, 1, T)))

    cu = torch.tensor([0, 5, 6, 16], dtype=torch.int32)
    first = A._segments(cu, 16)
    assert A._segments(cu, 16) is first and same(first, cu, 16)  # one build per model forward, not one per layer
    cu[1] = 3  # an in-place write bumps the version: the arrays follow the new contents
    second = A._segments(cu, 16)
    assert second is not first and same(second, cu, 16) and second[0][0].tolist() == [0] * 3 + [3] * 3 + [6] * 10
    assert first[0][0].tolist() == [0] * 5 + [5] + [6] * 10  # what was handed out earlier is not rewritten
    twin = cu.clone()  # equal values, another tensor: a result of its own
    third = A._segments(twin, 16)
    assert third is not second and same(third, twin, 16) and A._segments(cu, 16) is second
    longer = A._segments(cu, 32)  # the same tensor cut out of a longer row: rebuilt, with the padded tail as one more document
    assert longer[0].shape == (1, 32) and same(longer, cu, 32) and longer[0][0, 16:].tolist() == [16] * 16
    assert A._segments(cu, 16) is second and A._segments(cu, 32) is longer
    # a tensor that has gone away takes its entry's claim with it: a new tensor is never served another one's arrays
    for n in range(40):
        fresh = torch.tensor([0, 1 + n % 15, 16], dtype=torch.int32)
        assert same(A._segments(fresh, 16), fresh, 16)
        del fresh


@pytest.mark.parametrize("T,n_docs", [(64, 1), (64, 5), (64, 64), (48, 47)])
def test_pack_batch_against_a_loop(T, n_docs):
    from llm_fp8_amd import train
    ids = torch.randint(0, 1000, (2, T // 2), generator=torch.Generator().manual_seed(T + n_docs))
    batch = train.pack_batch(ids, n_docs, torch.Generator().manual_seed(n_docs))
    cu = batch["cu_seq_lens_q"]
    assert cu.dtype == torch.int32 and cu.shape == (n_docs + 1,) and batch["cu_seq_lens_k"] is cu
    cuts = cu.tolist()
    assert cuts[0] == 0 and cuts[-1] == T and all(a < b for a, b in zip(cuts, cuts[1:]))
    flat = ids.flatten().tolist()
    position, labels = [], []
    for lo, hi in zip(cuts, cuts[1:]):
        for t in range(lo, hi):
            position.append(t - lo)
            labels.append(-100 if t == lo else flat[t])
    assert batch["input_ids"].shape == batch["labels"].shape == batch["position_ids"].shape == (1, T)
    assert batch["input_ids"][0].tolist() == flat
    assert batch["position_ids"][0].tolist() == position
    assert batch["labels"][0].tolist() == labels
    assert batch["max_length_q"] >= max(b - a for a, b in zip(cuts, cuts[1:])) and batch["max_length_k"] == batch["max_length_q"]
    assert "attention_mask" not in batch
    # another seed cuts elsewhere (with n_docs == T, or one document, there is one way to cut)
    if 1 < n_docs < T - 1:
        assert train.pack_batch(ids, n_docs, torch.Generator().manual_seed(n_docs + 1))["cu_seq_lens_q"].tolist() != cuts


def test_pack_batch_refusals_and_synthetic_batch():
    from llm_fp8_amd import train
    ids = torch.zeros(2, 8, dtype=torch.long)
    for n in (0, -1, 17):
        with pytest.raises(ValueError, match="packed_docs"):
            train.pack_batch(ids, n)
    assert train.pack_batch(ids, 16)["cu_seq_lens_q"].tolist() == list(range(17))
    cfg = train.TrainingConfig(batch_size=2, max_seq_length=24, packed_docs=5)
    batch = train.synthetic_batch(cfg, 100, "cpu", torch.Generator().manual_seed(0))
    assert set(batch) == set(train.pack_batch(ids, 3)) and batch["input_ids"].shape == (1, 48)
    assert batch["cu_seq_lens_q"].shape == (6,) and batch["cu_seq_lens_q"][-1].item() == 48
    assert int(batch["input_ids"].max()) < 100 and (batch["labels"] == -100).sum().item() == 5
    assert train.config_from_args(train.build_arg_parser().parse_args(["--packed_docs", "5"])).packed_docs == 5
    assert train.config_from_args(train.build_arg_parser().parse_args([])).packed_docs == 0 == train.TrainingConfig().packed_docs
    plain = train.synthetic_batch(train.TrainingConfig(batch_size=2, max_seq_length=24), 100, "cpu", torch.Generator().manual_seed(0))
    assert set(plain) == {"input_ids", "attention_mask", "labels"} and torch.equal(plain["input_ids"].reshape(1, 48), batch["input_ids"])
