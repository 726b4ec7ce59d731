"""CPU: the Qwen3 family (llm_fp8_amd/qwen.py) computes what HF's Qwen3ForCausalLM computes -- per-head QK RMSNorm before RoPE, the
config's rotary base, head_dim != hidden / heads -- loads and saves HF-layout checkpoints, and train.create_model picks the family
from the model name.  The yardstick for "computes the same" is HF against itself: eager against sdpa attention on the same model."""
import os

import pytest
import torch


def _tiny_cfg(**kw):
    from llm_fp8_amd import qwen
    base = dict(vocab_size=128, hidden_size=64, num_attention_heads=4, num_key_value_heads=2, head_dim=32, intermediate_size=128,
                num_hidden_layers=2, rope_theta=1e6, rms_norm_eps=1e-6, tie_word_embeddings=True, max_position_embeddings=64)
    base.update(kw)
    return qwen.qwen3_config("qwen3-0.6b", **base)


def _hf_model(cfg, attn="eager", state=None, dtype=torch.float32):
    """Vanilla HF Qwen3 with every norm weight re-drawn in [0.5, 1.5] (all-ones norms would hide a dropped or swapped weight)."""
    from transformers.models.qwen3.modeling_qwen3 import Qwen3ForCausalLM
    cfg = type(cfg).from_dict(cfg.to_dict())
    cfg._attn_implementation = attn
    prev = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    try:
        torch.manual_seed(0)
        m = Qwen3ForCausalLM(cfg)
    finally:
        torch.set_default_dtype(prev)
    if state is None:
        g = torch.Generator().manual_seed(1)
        with torch.no_grad():
            for n, p in m.named_parameters():
                if n.endswith("norm.weight"):
                    p.copy_(0.5 + torch.rand(p.shape, generator=g))
    else:
        m.load_state_dict(state)
    return m.eval()


@pytest.fixture(scope="module")
def pair():
    """(config, HF eager model, HF sdpa model, TE model) sharing one set of fp32 weights."""
    from llm_fp8_amd import qwen
    cfg = _tiny_cfg()
    eager = _hf_model(cfg, "eager")
    sdpa = _hf_model(cfg, "sdpa", state=eager.state_dict())
    ours = qwen.TEQwen3ForCausalLM.from_hf_state_dict(eager.state_dict(), cfg, torch_dtype=torch.float32).eval()
    assert torch.get_default_dtype() == torch.float32
    return cfg, eager, sdpa, ours


def _batches():
    g = torch.Generator().manual_seed(2)
    ids = torch.randint(0, 128, (2, 16), generator=g)
    full = torch.ones(2, 16, dtype=torch.long)
    padded = full.clone()
    padded[1, 11:] = 0  # right padding: under a causal mask no kept position sees a padded one
    out = []
    for mask in (full, padded):
        labels = ids.clone()
        labels[mask == 0] = -100
        out.append((ids, mask, labels))
    return out


def test_te_qwen3_matches_hf_within_hfs_own_eager_sdpa_spread(pair, capsys):
    cfg, eager, sdpa, ours = pair
    for ids, mask, labels in _batches():
        with torch.no_grad():
            e = eager(input_ids=ids, attention_mask=mask, labels=labels)
            s = sdpa(input_ids=ids, attention_mask=mask, labels=labels)
            o = ours(input_ids=ids, attention_mask=mask, labels=labels)
        keep = mask.bool()
        yard = (e.logits[keep] - s.logits[keep]).abs().max().item()
        diff = (o.logits[keep] - e.logits[keep]).abs().max().item()
        with capsys.disabled():
            print(f"\n  qwen3 tiny, {int(keep.sum())} positions: HF eager vs sdpa {yard:.3g}, ours vs HF eager {diff:.3g}, "
                  f"max |logit| {e.logits[keep].abs().max().item():.3g}, loss {e.loss.item():.6f} / {o.loss.item():.6f}", end="")
        assert yard > 0.0, "the yardstick is degenerate: eager and sdpa agree to the bit"
        assert diff <= 100 * yard
        assert abs(o.loss.item() - e.loss.item()) <= 100 * max(yard, abs(e.loss.item() - s.loss.item()))


def test_te_qwen3_carries_the_qk_norm_and_the_rotary_base(pair):
    from llm_fp8_amd import qwen
    cfg, eager, _, ours = pair
    hsd, sd = eager.state_dict(), ours.state_dict()
    layer = ours.model.layers[0]
    assert isinstance(layer, qwen.TEQwen3DecoderLayer) and layer.self_attention.qk_norm_type == "RMSNorm"
    assert layer.self_attention.d == 32 and layer.self_attention.qk_norm_eps == cfg.rms_norm_eps
    for i in range(cfg.num_hidden_layers):
        for n in ("q_norm", "k_norm"):
            assert torch.equal(sd[f"model.layers.{i}.self_attention.{n}.weight"], hsd[f"model.layers.{i}.self_attn.{n}.weight"])
    assert qwen.rope_base(cfg) == 1e6
    inv = 1.0 / (1e6 ** (torch.arange(0, 32, 2, dtype=torch.float32) / 32))
    assert torch.allclose(layer.te_rope_emb[3, 0, 0, :16], 3 * inv)


def test_a_dropped_norm_a_wrong_base_or_swapped_gammas_would_be_seen(pair):
    """The gate of the comparison test is sharp: each of the three defects moves the logits by far more than 100 x the yardstick."""
    from llm_fp8_amd import llama, qwen
    cfg, eager, sdpa, _ = pair
    ids, mask, labels = _batches()[0]
    with torch.no_grad():
        e = eager(input_ids=ids).logits
        yard = (e - sdpa(input_ids=ids).logits).abs().max().item()
    hsd = eager.state_dict()

    def logits_of(state, patch=None):
        m = qwen.TEQwen3ForCausalLM.from_hf_state_dict(state, cfg, torch_dtype=torch.float32).eval()
        if patch is not None:
            patch(m)
        with torch.no_grad():
            return m(input_ids=ids).logits

    swapped = {k.replace("q_norm", "@").replace("k_norm", "q_norm").replace("@", "k_norm"): v for k, v in hsd.items()}
    ones = {k: (torch.ones_like(v) if k.endswith(("q_norm.weight", "k_norm.weight")) else v) for k, v in hsd.items()}

    def base_10000(m):
        for layer in m.model.layers:
            layer.te_rope_emb = llama._rope_table(32, cfg.max_position_embeddings, "cpu")

    for name, got in (("swapped", logits_of(swapped)), ("ones", logits_of(ones)), ("base", logits_of(hsd, base_10000))):
        assert (got - e).abs().max().item() > 1000 * yard, name


def test_state_dict_goes_back_to_vanilla_hf(pair):
    from llm_fp8_amd import llama
    cfg, eager, _, ours = pair
    back = llama.to_hf_state_dict(ours.state_dict(), cfg)
    hsd = eager.state_dict()
    res = _hf_model(cfg, state=hsd).load_state_dict(back, strict=False)
    assert not res.missing_keys and not res.unexpected_keys
    assert set(back) == set(hsd)
    for k in hsd:
        assert torch.equal(back[k], hsd[k]), k  # q_norm / k_norm among them, bitwise


def test_checkpoint_round_trip(tmp_path, pair):
    from transformers.models.qwen3.modeling_qwen3 import Qwen3ForCausalLM
    from llm_fp8_amd import checkpoint, qwen
    cfg, eager, _, ours = pair
    out = tmp_path / "ckpt"
    files = checkpoint.save_pretrained(ours, str(out))
    assert files and os.path.isfile(out / "config.json")
    again = qwen.TEQwen3ForCausalLM.from_pretrained_local(str(out), config=cfg, torch_dtype=torch.float32)
    a, b = ours.state_dict(), again.state_dict()
    assert set(a) == set(b)
    for k in a:
        if isinstance(a[k], torch.Tensor):
            assert torch.equal(a[k], b[k]), k
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("error")  # load_into warns about parameters no shard covered: there must be none
        checkpoint.load_into(again, str(out), cfg)
    vanilla = Qwen3ForCausalLM.from_pretrained(str(out), torch_dtype=torch.float32)
    for k, v in eager.state_dict().items():
        assert torch.equal(vanilla.state_dict()[k], v), k


def test_create_model_picks_the_family_by_name():
    from transformers.models.llama.modeling_llama import LlamaForCausalLM
    from transformers.models.qwen3.modeling_qwen3 import Qwen3ForCausalLM
    from llm_fp8_amd import llama, qwen, train
    tiny = dict(num_hidden_layers=1, vocab_size=64)
    for name, hf_cls, layer_cls in (("qwen3-0.6b", Qwen3ForCausalLM, qwen.TEQwen3DecoderLayer), ("Qwen/Qwen3-0.6B", Qwen3ForCausalLM, qwen.TEQwen3DecoderLayer),
                                    ("llama-3.2-1b", LlamaForCausalLM, llama.TELlamaDecoderLayer)):
        for use_te in (True, False):
            m = train.create_model(train.TrainingConfig(model_name=name, use_te=use_te, **tiny), torch.device("cpu"))
            assert isinstance(m, hf_cls), (name, use_te)
            assert isinstance(m.model.layers[0], layer_cls) == use_te
            assert isinstance(m.model.layers[0], qwen.TEQwen3DecoderLayer) == (use_te and hf_cls is Qwen3ForCausalLM)
    for name in ("qwen3-7b", "qwen2-7b", "mistral-7b"):
        with pytest.raises(KeyError) as err:
            train.create_model(train.TrainingConfig(model_name=name, **tiny), torch.device("cpu"))
        assert "qwen3-0.6b" in str(err.value) and "llama-3.2-1b" in str(err.value)


def test_published_shapes():
    from llm_fp8_amd import qwen
    want = {"qwen3-0.6b": (1024, 3072, 28, 16, 8, 128, True), "qwen3-1.7b": (2048, 6144, 28, 16, 8, 128, True),
            "qwen3-4b": (2560, 9728, 36, 32, 8, 128, True), "qwen3-8b": (4096, 12288, 36, 32, 8, 128, False)}
    for name, w in want.items():
        for alias in (name, "Qwen/" + name.replace("qwen3", "Qwen3").upper().replace("QWEN3", "Qwen3")):
            c = qwen.qwen3_config(alias)
            assert (c.hidden_size, c.intermediate_size, c.num_hidden_layers, c.num_attention_heads, c.num_key_value_heads, c.head_dim,
                    c.tie_word_embeddings) == w
            assert c.vocab_size == 151936 and c.rms_norm_eps == 1e-6 and c.max_position_embeddings == 40960
            assert qwen.rope_base(c) == 1e6 and not c.attention_bias


def test_refused_configs():
    from llm_fp8_amd import qwen
    for kw, word in ((dict(attention_bias=True), "attention_bias"), (dict(use_sliding_window=True, sliding_window=8), "use_sliding_window"),
                     (dict(rope_parameters={"rope_type": "yarn", "rope_theta": 1e6, "factor": 2.0, "original_max_position_embeddings": 32}),
                      "rope_type")):
        cfg = _tiny_cfg(**kw)
        with pytest.raises(NotImplementedError, match=word):
            qwen.TEQwen3ForCausalLM(cfg)
