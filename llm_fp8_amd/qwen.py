"""Counterpart of the reference's te_qwen.py on top of `llm_fp8_amd.pytorch`: Qwen3 decoder layers in the TE layout, the same
monkey-patch and loaders as llama.py, the same five FP8 scenarios.

A Qwen3 decoder layer is a Llama decoder layer (RMSNorm, GQA with an explicit head_dim, SwiGLU, no biases) plus an RMSNorm over
head_dim on every query and key head between the q|k|v projection and RoPE (HF `self_attn.q_norm` / `self_attn.k_norm`), and a
rotary base of 1e6.  The reference's wrapper builds a plain TE attention and drops the two norm weights at load, so it does not
compute Qwen3; this one follows HF: `MultiheadAttention(qk_norm_type="RMSNorm", qk_norm_eps=rms_norm_eps)` and the weights are
loaded and saved under HF's names.

No weights or config.json exist offline: the configs below are the published values AS RECALLED -- they could not be checked
against the hub from here.  `**overrides` and a local `config.json` (`Qwen3Config.from_pretrained(dir)`) win over them.
"""
from __future__ import annotations

from contextlib import contextmanager
from typing import Dict

from . import llama
from .llama import TELlamaDecoderLayer, TELlamaForCausalLM, _drop_padding_mask, _install_final_norm_fusion, scenario_recipes

QWEN3_CONFIGS: Dict[str, dict] = {
    "qwen3-0.6b": dict(hidden_size=1024, intermediate_size=3072, num_hidden_layers=28, num_attention_heads=16,
                       num_key_value_heads=8, head_dim=128, tie_word_embeddings=True),
    "qwen3-1.7b": dict(hidden_size=2048, intermediate_size=6144, num_hidden_layers=28, num_attention_heads=16,
                       num_key_value_heads=8, head_dim=128, tie_word_embeddings=True),
    "qwen3-4b": dict(hidden_size=2560, intermediate_size=9728, num_hidden_layers=36, num_attention_heads=32,
                     num_key_value_heads=8, head_dim=128, tie_word_embeddings=True),
    "qwen3-8b": dict(hidden_size=4096, intermediate_size=12288, num_hidden_layers=36, num_attention_heads=32,
                     num_key_value_heads=8, head_dim=128, tie_word_embeddings=False),
}
_ALIASES = {f"qwen/{k}": k for k in QWEN3_CONFIGS}


def is_qwen3_name(name: str) -> bool:
    """train.create_model's family rule: names starting `qwen3` or `qwen/qwen3` are Qwen3, everything else is Llama."""
    return name.lower().startswith(("qwen3", "qwen/qwen3"))


def qwen3_config(name: str, **overrides):
    """Hard-coded Qwen3Config (see the module docstring: values as recalled, unchecked; overrides win)."""
    from transformers import Qwen3Config
    key = name.lower()
    key = _ALIASES.get(key, key)
    if key not in QWEN3_CONFIGS:
        raise KeyError(f"unknown model {name!r}; known: {sorted(QWEN3_CONFIGS) + sorted(llama.LLAMA_CONFIGS)}")
    kw = dict(vocab_size=151936, rms_norm_eps=1e-6, max_position_embeddings=40960, rope_theta=1000000.0, hidden_act="silu",
              attention_bias=False, use_sliding_window=False, initializer_range=0.02, use_cache=False,
              bos_token_id=151643, eos_token_id=151645)
    kw.update(QWEN3_CONFIGS[key])
    kw.update(overrides)
    for tok in ("bos_token_id", "eos_token_id"):  # a vocabulary cut down for a test has no room for the published ids
        if kw[tok] is not None and kw[tok] >= kw["vocab_size"]:
            kw[tok] = None
    cfg = Qwen3Config(**kw)
    cfg._attn_implementation = "sdpa"
    return cfg


def rope_base(config) -> float:
    """The rotary base of a Qwen3Config: `rope_parameters["rope_theta"]` where transformers keeps it there, else `rope_theta`."""
    params = getattr(config, "rope_parameters", None)
    if isinstance(params, dict) and params.get("rope_theta") is not None:
        return float(params["rope_theta"])
    theta = getattr(config, "rope_theta", None)
    if theta is None:
        raise ValueError("Qwen3 config carries no rope_theta")
    return float(theta)


def _rope_type(config) -> str:
    for attr in ("rope_parameters", "rope_scaling"):
        params = getattr(config, attr, None)
        if isinstance(params, dict):
            return str(params.get("rope_type", params.get("type", "default")))
    return "default"


class TEQwen3DecoderLayer(TELlamaDecoderLayer):
    """TELlamaDecoderLayer with the per-head QK RMSNorm and the config's rotary base; `forward` (both routes) is inherited."""

    def __init__(self, config, *args, **kwargs):
        if _rope_type(config) != "default":
            raise NotImplementedError(f"TEQwen3DecoderLayer: rope_type {_rope_type(config)!r} is not implemented (only 'default')")
        if getattr(config, "use_sliding_window", False):
            raise NotImplementedError("TEQwen3DecoderLayer: use_sliding_window=True is not implemented (full causal attention only)")
        if getattr(config, "attention_bias", False):
            raise NotImplementedError("TEQwen3DecoderLayer: attention_bias=True is not implemented")
        super().__init__(config, *args, _attention_kwargs=dict(qk_norm_type="RMSNorm", qk_norm_eps=config.rms_norm_eps),
                         _mlp_kwargs=dict(eps=config.rms_norm_eps), _rope_base=rope_base(config), **kwargs)


def decoder_layer_cls(scenario: str):
    scenario_recipes(scenario)  # validate
    return type(f"TEQwen3DecoderLayer_{scenario}", (TEQwen3DecoderLayer,), {"scenario": scenario})


@contextmanager
def replace_decoder(te_decoder_cls):
    """Swap HF's Qwen3DecoderLayer while Qwen3ForCausalLM is being built (llama.replace_decoder for the other family)."""
    import transformers
    mod = transformers.models.qwen3.modeling_qwen3
    original = mod.Qwen3DecoderLayer
    mod.Qwen3DecoderLayer = te_decoder_cls
    try:
        yield
    finally:
        mod.Qwen3DecoderLayer = original


class TEQwen3ForCausalLM(TELlamaForCausalLM):
    """HF owns embeddings / final norm / lm_head / loss, our layers own the decoder.  `from_pretrained_local` and
    `from_hf_state_dict` are TELlamaForCausalLM's (they build `cls(config, scenario)` and copy through llama.replace_params, which
    knows the two QK-norm weights).  The Llama model's two model-level pieces apply unchanged: the padding-mask hook (the layers
    are causal and ignore the mask) and the final-norm fusion (Qwen3RMSNorm has LlamaRMSNorm's `weight` / `variance_epsilon`)."""

    def __new__(cls, config, scenario: str = "default"):
        from transformers.models.qwen3.modeling_qwen3 import Qwen3ForCausalLM
        with replace_decoder(te_decoder_cls=decoder_layer_cls(scenario)):
            model = Qwen3ForCausalLM(config)
        model.model.register_forward_pre_hook(_drop_padding_mask, with_kwargs=True)
        _install_final_norm_fusion(model)
        return model
