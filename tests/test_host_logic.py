"""CPU: host-side logic that needs no GPU -- recipes, state-dict mapping both ways, tile picking rules mirrored in Python."""
import pytest
import torch


def test_recipe_surface_matches_te_defaults():
    from llm_fp8_amd.common.recipe import DelayedScaling, Format, MXFP8BlockScaling, fmt_codes
    r = DelayedScaling()
    assert r.fp8_format is Format.HYBRID and r.amax_history_len == 1024 and r.amax_compute_algo == "max" and r.margin == 0
    assert Format.HYBRID.value.max_fwd == 448.0 and Format.HYBRID.value.max_bwd == 57344.0 and Format.E4M3.value.max_bwd == 448.0
    assert fmt_codes(Format.HYBRID) == (0, 1) and fmt_codes(Format.E4M3) == (0, 0) and fmt_codes(Format.E5M2) == (1, 1)
    assert MXFP8BlockScaling().mxfp8() and not r.mxfp8() and r.delayed()
    with pytest.raises(ValueError):
        DelayedScaling(amax_compute_algo="median")
    # accelerate's TERecipeKwargs call shape (utils/transformer_engine.py:156-177)
    DelayedScaling(margin=0, interval=1, fp8_format=Format.E4M3, amax_history_len=16, amax_compute_algo="max",
                   override_linear_precision=(False, False, False))


def test_scenario_recipes_follow_the_three_reference_files():
    from llm_fp8_amd import llama
    from llm_fp8_amd.common.recipe import Format
    a, m = llama.scenario_recipes("default")      # te_llama.py:39-40
    assert a.fp8_format is Format.HYBRID and m.fp8_format is Format.E4M3 and a.amax_history_len == m.amax_history_len == 16
    a, m = llama.scenario_recipes("hybrid")       # te_llama_hybrid.py:39
    assert a is m and a.fp8_format is Format.HYBRID
    a, m = llama.scenario_recipes("mxfp8")        # te_llama_mxfp8.py:28-29
    assert a is m and a.mxfp8() and a.fp8_format is Format.E4M3
    o = llama.outer_recipe_for_scenario("default")  # train_fp8.py:144-146 -> TERecipeKwargs() defaults
    assert o.fp8_format is Format.HYBRID and o.amax_history_len == 1024 and o.amax_compute_algo == "most_recent"
    o = llama.outer_recipe_for_scenario("mxfp8")    # train_fp8.py:158-165
    assert o.fp8_format is Format.E4M3 and o.amax_history_len == 16 and o.delayed()


def test_replace_params_and_its_inverse_roundtrip():
    from transformers.models.llama.modeling_llama import LlamaForCausalLM
    from llm_fp8_amd import llama
    cfg = llama.llama_config("llama-3.2-1b", num_hidden_layers=2, hidden_size=64, intermediate_size=128, num_attention_heads=4,
                             num_key_value_heads=2, head_dim=16, vocab_size=128, max_position_embeddings=64)
    torch.manual_seed(0)
    hf = LlamaForCausalLM(cfg)
    te_model = llama.TELlamaForCausalLM.from_hf_state_dict(hf.state_dict(), cfg, "default", torch_dtype=torch.float32)
    sd = te_model.state_dict()
    assert "model.layers.1.layernorm_mlp.fc1_weight" in sd and "model.layers.0.self_attention.layernorm_qkv.key_weight" in sd
    assert "model.layers.0.layernorm_mlp.fc1_bias" in sd  # TE-only parameters
    back = llama.to_hf_state_dict(sd, cfg)
    ref = hf.state_dict()
    assert set(back.keys()) == set(ref.keys())
    for k in ref:
        assert torch.equal(back[k].float(), ref[k].float()), k
    hf2 = LlamaForCausalLM(cfg)
    hf2.load_state_dict(back)  # vanilla HF can load what we save
    sd["model.layers.0.layernorm_mlp.fc2_bias"] = torch.ones_like(sd["model.layers.0.layernorm_mlp.fc2_bias"])
    with pytest.raises(ValueError, match="no MLP bias"):
        llama.to_hf_state_dict(sd, cfg)


def test_llama_config_table():
    from llm_fp8_amd import llama
    c = llama.llama_config("meta-llama/Llama-3.2-3B")
    assert (c.hidden_size, c.intermediate_size, c.num_hidden_layers, c.num_attention_heads, c.num_key_value_heads, c.head_dim) == (3072, 8192, 28, 24, 8, 128)
    assert c.vocab_size == 128256 and c.tie_word_embeddings
    c = llama.llama_config("llama-3.1-8b")
    assert (c.hidden_size, c.intermediate_size, c.num_hidden_layers) == (4096, 14336, 32) and not c.tie_word_embeddings
    with pytest.raises(KeyError):
        llama.llama_config("gpt-2")


def test_committed_bench_line_has_the_contract_fields():
    """The newest committed headline bench line (profiles/r01*_bench_3b_default.json, printed by bench.py on the GPU box)
    carries every field of the bench contract, incl. the `roofline` and `cpu_baseline` objects."""
    import glob
    import json
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    files = sorted(glob.glob(os.path.join(root, "profiles", "r*_bench_3b_default.json")))
    assert files, "no committed bench line"
    d = json.load(open(files[-1]))
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
              "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert k in d, k
    assert d["unit"] == "tokens/s" and d["higher_is_better"] is True and d["scaling"] == "weak" and d["vs_baseline"] is None
    assert "workload" in d["config"] and "model" not in d["config"]
    r = d["roofline"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert k in r, k
    assert r["bound"] == "mfma" and r["unit"] == "TFLOP/s" and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-9
    c = d["cpu_baseline"]
    for k in ("value", "unit", "cores", "kind", "sample"):
        assert k in c, k
    assert c["kind"] in ("port", "reference")
    tokens = 16 * 512 * d["n_gpus"]
    assert abs(d["value"] - tokens / (d["ms_per_step"] * 1e-3)) / d["value"] < 1e-6


def test_padding_mask_never_reaches_hfs_mask_builder():
    """te_llama.py:68-82 forwards `attention_mask`, TE's causal core ignores it.  HF's mask builder would synchronise the host on
    it once per forward; the model hands it a 4-D placeholder instead (llama._drop_padding_mask).  Outputs must not change."""
    import torch
    from transformers import LlamaConfig
    from llm_fp8_amd import llama
    cfg = LlamaConfig(hidden_size=64, intermediate_size=128, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=2,
                      vocab_size=256, max_position_embeddings=128)
    torch.manual_seed(0)
    model = llama.TELlamaForCausalLM(cfg)
    ids = torch.randint(0, 256, (2, 32))
    seen = []
    h = model.model.layers[0].register_forward_pre_hook(lambda m, a, kw: seen.append(kw.get("attention_mask")), with_kwargs=True)
    with torch.no_grad():
        with_mask = model(input_ids=ids, attention_mask=torch.ones_like(ids)).logits
        no_mask = model(input_ids=ids).logits
        four_d = torch.ones((2, 1, 32, 32), dtype=torch.bool).tril()
        model(input_ids=ids, attention_mask=four_d)
        h.remove()
        model.model._forward_pre_hooks.clear()  # HF's own path (2-D mask -> its builder)
        plain = model(input_ids=ids, attention_mask=torch.ones_like(ids)).logits
    assert torch.equal(with_mask, no_mask) and torch.equal(with_mask, plain)
    assert seen[0] is not None and seen[0].dim() == 4 and seen[0].numel() == 1  # the placeholder reached the decoder layers
    assert seen[2] is four_d or (seen[2].shape == four_d.shape)  # a caller's prepared 4-D mask is passed through untouched


def test_rmsnorm_bwd_width_tests_cover_every_dispatcher_instance():
    """tests/test_kernel_widths_gpu.py runs mi_rmsnorm_bwd at cols = 512 x NVEC for exactly the NVEC of the MI_RB(NVEC, WPR)
    instances in mi_fused.hip: an instance added there without a GPU test fails here, on any machine."""
    import os
    import re
    from tests import test_kernel_widths_gpu as widths
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "llm_fp8_amd", "csrc", "mi_fused.hip")).read()
    body = src[src.index('extern "C" int mi_rmsnorm_bwd('):]
    body = body[:body.index("#undef MI_RB")]
    inst = [(int(a), int(b)) for a, b in re.findall(r"MI_RB\(\s*(\d+)\s*,\s*(\d+)\s*\)", body)]
    assert len(inst) >= 12 and len({v for v, _ in inst}) == len(inst), inst
    assert {1, 2, 4} >= {w for _, w in inst}
    assert sorted(v for v, _ in inst) == sorted(widths.RB_VECS)
    assert widths.RB_WIDTHS == tuple(512 * v for v in widths.RB_VECS)


def test_sink_stamp_follows_the_shard_of_a_row_sharded_weight():
    """module.WeightSink / MXWeightSink declare their FP8 copies current while the parts' versions (and, delayed scaling, the scale
    arena's generation) are what they were at emission.  A row-sharded weight (distributed.ShardedFP8DP) is written through its
    shard only -- the module's Parameter is a storage-less view whose version never moves -- so the shard's version must count."""
    from types import SimpleNamespace
    from llm_fp8_amd.distributed import _ShardHandle
    from llm_fp8_amd.pytorch.module import MXWeightSink, WeightSink, stepped_tensor

    def sharded(rows, K):
        w = torch.nn.Parameter(torch.randn(rows, K).to(torch.bfloat16))
        shard = torch.nn.Parameter(w.detach()[: rows // 2].clone())
        w._mi_sharded = _ShardHandle(None, shard, 0, rows // 2)
        w.data = torch.zeros(1, dtype=w.dtype).expand(w.shape)
        return w, shard

    arena = SimpleNamespace(generation=0)
    mf = SimpleNamespace(arena=arena, scale=lambda i: torch.ones(1), amax=lambda i: torch.zeros(1))
    (w1, s1), (w2, s2) = sharded(64, 64), sharded(32, 64)
    plain = torch.nn.Parameter(torch.randn(32, 64).to(torch.bfloat16))
    assert stepped_tensor(w1) is s1 and stepped_tensor(plain) is plain   # what ClippedAdamW counts as rewritten
    for make in (lambda ws, ns: WeightSink(ws, ns, sum(ns), 64, "cpu", mf, 1), lambda ws, ns: MXWeightSink(ws, ns, sum(ns), 64, "cpu")):
        for parts, shards in (([w1, w2], [s1, s2]), ([plain], [plain])):
            sink = make(parts, [p.shape[0] for p in parts])
            assert not sink.fresh()
            sink.mark()
            assert sink.fresh()
            for t in shards:
                v = tuple(p._version for p in parts)
                torch.autograd.graph.increment_version(t)   # what ClippedAdamW does after writing through raw addresses
                assert not sink.fresh(), "a write to a shard left the sink current"
                sink.mark()
                assert sink.fresh()
                if t is not plain:
                    assert tuple(p._version for p in parts) == v   # the module Parameter's own counter did not move
            if isinstance(sink, WeightSink):
                arena.generation += 1
                assert not sink.fresh()


def _extra_blob(n_fwd=3, n_bwd=2, H=16, seed=0):
    """A blob with the layout of _FP8Module.get_extra_state for a one-GEMM module, filled with values no default state has."""
    import io
    g = torch.Generator().manual_seed(seed)
    side = lambda n: {"scale": 1 + torch.rand(n, generator=g), "scale_inv": 0.1 + torch.rand(n, generator=g),
                      "amax_history": torch.rand(H, n, generator=g)}
    st = {"fwd": side(n_fwd), "bwd": side(n_bwd)}
    buf = io.BytesIO()
    torch.save(st, buf)
    return st, torch.frombuffer(bytearray(buf.getvalue()), dtype=torch.uint8)


def _decode_extra(blob):
    import io
    return torch.load(io.BytesIO(blob.cpu().numpy().tobytes()), weights_only=True)


def test_loaded_fp8_state_survives_a_save_before_the_first_forward():
    """set_extra_state parks the blob until the first FP8 forward allocates the meta windows.  A save in between (a layout
    conversion, a checkpoint at step 0) must write what was loaded, not an empty tensor: load -> state_dict() -> load into a third
    module carries every scale and the whole amax history."""
    import llm_fp8_amd.pytorch as te
    st, blob = _extra_blob()
    a = te.Linear(64, 64, device="cpu")
    sd = a.state_dict()
    assert sd["_extra_state"].numel() == 0          # nothing loaded, no forward: still the empty tensor
    sd["_extra_state"] = blob
    b = te.Linear(64, 64, device="cpu")
    b.load_state_dict(sd)
    assert b._pending_state is not None and b._meta_fwd is None
    sd_b = b.state_dict()
    assert sd_b["_extra_state"].numel() > 0, "a save before the first forward dropped the loaded FP8 state"
    c = te.Linear(64, 64, device="cpu")
    c.load_state_dict(sd_b)
    for got in (_decode_extra(sd_b["_extra_state"]), c._pending_state, _decode_extra(c.state_dict()["_extra_state"])):
        assert set(got) == {"fwd", "bwd"}
        for d in ("fwd", "bwd"):
            assert set(got[d]) == {"scale", "scale_inv", "amax_history"}
            for k, v in st[d].items():
                assert got[d][k].dtype == v.dtype and torch.equal(got[d][k], v), (d, k)


def test_a_state_of_another_history_length_is_refused_before_anything_is_written():
    """ModuleMeta.load_state checks the amax-history length first: scale and scale_inv of the window are not overwritten, the
    arena's generation does not move.  A module whose pending state does not fit refuses at every FP8 forward and takes no slots."""
    import llm_fp8_amd.pytorch as te
    from llm_fp8_amd.common.recipe import DelayedScaling, Format
    from llm_fp8_amd.pytorch.fp8 import FP8GlobalStateManager as G, MetaArena, ModuleMeta
    G.reset()
    try:
        recipe = DelayedScaling(fp8_format=Format.HYBRID, amax_history_len=4, amax_compute_algo="max")
        arena = G.arena(recipe, True, "cpu")
        meta = ModuleMeta(arena, arena.alloc(3), 3)
        st, blob = _extra_blob(H=16)
        gen = arena.generation
        with pytest.raises(RuntimeError, match="amax history length 16 in checkpoint != recipe's 4"):
            meta.load_state(st["fwd"])
        assert arena.generation == gen
        assert torch.equal(arena.scale, torch.ones(MetaArena.CAP)) and torch.equal(arena.scale_inv, torch.ones(MetaArena.CAP))
        assert not arena.hist.any()
        lin = te.Linear(64, 64, device="cpu")
        lin.set_extra_state(blob)
        G.FP8_ENABLED, G.FP8_RECIPE = True, recipe  # FP8 "enabled" by hand: the autocast wants a GPU
        for _ in range(2):
            with pytest.raises(RuntimeError, match="amax history length"):
                lin._prepare("cpu")
            assert lin._meta_fwd is None and lin._pending_state is not None and arena.used == 3
        fit = DelayedScaling(fp8_format=Format.HYBRID, amax_history_len=16, amax_compute_algo="max")
        G.FP8_RECIPE = fit
        lin._prepare("cpu")
        assert lin._pending_state is None and torch.equal(lin._meta_fwd.state()["amax_history"], st["fwd"]["amax_history"])
    finally:
        G.reset()
