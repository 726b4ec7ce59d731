"""CPU: file-level checkpoint I/O in the HF <-> fused layout (te_llama.py:100-178, train_fp8.py:657-681)."""
import json
import os

import pytest
import torch


def _tiny_cfg(**kw):
    from llm_fp8_amd import llama
    base = dict(num_hidden_layers=2, hidden_size=64, intermediate_size=128, num_attention_heads=4, num_key_value_heads=2,
                head_dim=16, vocab_size=128, max_position_embeddings=64)
    base.update(kw)
    return llama.llama_config("llama-3.2-1b", **base)


def _hf_model(cfg, seed=0):
    from transformers.models.llama.modeling_llama import LlamaForCausalLM
    torch.manual_seed(seed)
    prev = torch.get_default_dtype()
    torch.set_default_dtype(torch.bfloat16)
    try:
        m = LlamaForCausalLM(cfg)
    finally:
        torch.set_default_dtype(prev)
    return m


@pytest.mark.parametrize("tied", [True, False])
@pytest.mark.parametrize("sharded", [False, True])
def test_hf_checkpoint_dir_loads_into_te_model_and_saves_back_for_vanilla_hf(tmp_path, tied, sharded):
    from transformers.models.llama.modeling_llama import LlamaForCausalLM
    from llm_fp8_amd import checkpoint, llama
    cfg = _tiny_cfg(tie_word_embeddings=tied)
    hf = _hf_model(cfg)
    src = tmp_path / "src"
    # the checkpoint a user would have on disk: vanilla HF save_pretrained (safetensors), optionally sharded
    hf.save_pretrained(str(src), safe_serialization=True, max_shard_size="40KB" if sharded else "5GB")
    assert os.path.isfile(src / ("model.safetensors.index.json" if sharded else "model.safetensors"))
    shards = checkpoint.resolve_shards(str(src))
    assert (len(shards) > 1) == sharded

    te_model = llama.TELlamaForCausalLM.from_pretrained_local(str(src), config=cfg, scenario="hybrid", torch_dtype=torch.bfloat16)
    assert torch.get_default_dtype() == torch.float32  # restored (the reference leaves bf16 behind: SURVEY.md Appendix C.5)
    sd, hsd = te_model.state_dict(), hf.state_dict()
    f = cfg.intermediate_size
    for i in range(cfg.num_hidden_layers):
        p = f"model.layers.{i}."
        assert torch.equal(sd[p + "self_attention.layernorm_qkv.query_weight"], hsd[p + "self_attn.q_proj.weight"])
        assert torch.equal(sd[p + "self_attention.layernorm_qkv.key_weight"], hsd[p + "self_attn.k_proj.weight"])
        assert torch.equal(sd[p + "self_attention.proj.weight"], hsd[p + "self_attn.o_proj.weight"])
        assert torch.equal(sd[p + "layernorm_mlp.fc1_weight"][:f], hsd[p + "mlp.gate_proj.weight"])
        assert torch.equal(sd[p + "layernorm_mlp.fc1_weight"][f:], hsd[p + "mlp.up_proj.weight"])
        assert torch.equal(sd[p + "layernorm_mlp.fc2_weight"], hsd[p + "mlp.down_proj.weight"])
        assert torch.equal(sd[p + "layernorm_mlp.layer_norm_weight"], hsd[p + "post_attention_layernorm.weight"])
    assert torch.equal(sd["model.embed_tokens.weight"], hsd["model.embed_tokens.weight"])
    assert torch.equal(sd["lm_head.weight"], hsd["lm_head.weight"])
    assert torch.equal(sd["model.norm.weight"], hsd["model.norm.weight"])

    # ... and back: the saved directory must load into a VANILLA LlamaForCausalLM with identical weights
    out = tmp_path / "out"
    files = checkpoint.save_pretrained(te_model, str(out), max_shard_bytes=(40 << 10) if sharded else (5 << 30))
    assert (len(files) > 1) == sharded and os.path.isfile(out / "config.json")
    if sharded:
        idx = json.load(open(out / "model.safetensors.index.json"))
        assert set(idx["weight_map"].values()) == {os.path.basename(fn) for fn in files}
    back = LlamaForCausalLM.from_pretrained(str(out), torch_dtype=torch.bfloat16)
    bsd = back.state_dict()
    assert set(bsd) == set(hsd)
    for k in hsd:
        assert torch.equal(bsd[k], hsd[k]), k


def test_te_layout_roundtrip_keeps_te_names_and_biases(tmp_path):
    from llm_fp8_amd import checkpoint, llama
    cfg = _tiny_cfg()
    torch.manual_seed(1)
    m = llama.TELlamaForCausalLM(cfg, "default")
    with torch.no_grad():
        m.model.layers[0].layernorm_mlp.fc1_bias.normal_()   # a trained TE-only bias: HF layout must refuse it, TE layout keeps it
    with pytest.raises(ValueError):
        checkpoint.save_pretrained(m, str(tmp_path / "hf"), layout="hf")
    checkpoint.save_pretrained(m, str(tmp_path / "te"), layout="te")
    m2 = llama.TELlamaForCausalLM.from_pretrained_local(str(tmp_path / "te"), config=cfg, scenario="default", torch_dtype=torch.float32)
    for (k, a), (k2, b) in zip(m.state_dict().items(), m2.state_dict().items()):
        assert k == k2
        if isinstance(a, torch.Tensor) and not k.endswith("_extra_state"):
            assert torch.equal(a.float(), b.float()), k


def test_save_refuses_row_sharded_weights_without_their_master(tmp_path):
    """distributed.ShardedFP8DP leaves a module's GEMM weight as a storage-less expanded view carrying `_mi_sharded`; written as it
    is, `.contiguous()` would turn it into an all-zero tensor.  save_pretrained must refuse, and save the real values once the
    master is materialised again (gather_master_weights puts a full tensor back into `.data`)."""
    from llm_fp8_amd import checkpoint, llama
    from llm_fp8_amd.distributed import _ShardHandle
    cfg = _tiny_cfg()
    torch.manual_seed(2)
    m = llama.TELlamaForCausalLM(cfg, "default")
    p = m.model.layers[1].layernorm_mlp.fc2_weight
    full = p.detach().clone()
    n = p.shape[0] // 2
    p._mi_sharded = _ShardHandle(None, torch.nn.Parameter(full[:n].clone()), 0, n)  # rank 0 of 2
    p.data = torch.zeros(1, dtype=p.dtype).expand(p.shape)
    with pytest.raises(RuntimeError, match="gather_master_weights"):
        checkpoint.save_pretrained(m, str(tmp_path / "hollow"))
    assert not (tmp_path / "hollow" / "model.safetensors").exists()
    p.data = full.clone()
    checkpoint.save_pretrained(m, str(tmp_path / "full"))
    from safetensors.torch import load_file
    got = load_file(str(tmp_path / "full" / "model.safetensors"))["model.layers.1.mlp.down_proj.weight"]
    assert torch.equal(got.view(torch.int16), full.view(torch.int16))


def test_missing_or_pickled_checkpoints_are_refused(tmp_path):
    from llm_fp8_amd import checkpoint
    (tmp_path / "pytorch_model.bin").write_bytes(b"not read")
    with pytest.raises(AssertionError, match="Only sharded PyTorch ckpt format"):  # te_llama.py:150
        checkpoint.resolve_shards(str(tmp_path))
    (tmp_path / "model.safetensors.index.json").write_text(json.dumps({"weight_map": {"a": "model-00001-of-00002.safetensors"}}))
    with pytest.raises(FileNotFoundError):
        checkpoint.resolve_shards(str(tmp_path))


def test_train_harness_saves_and_reloads(tmp_path):
    """--output_dir / --load_dir of the harness (train_fp8.py:657-681): CPU plumbing config, bf16, no TE."""
    from transformers.models.llama.modeling_llama import LlamaForCausalLM
    from llm_fp8_amd import train
    out = tmp_path / "ckpt"
    args = ["--model_name", "llama-3.2-1b", "--batch_size", "1", "--max_seq_length", "16", "--mixed_precision", "bf16",
            "--num_hidden_layers", "1", "--vocab_size", "256", "--num_steps", "2", "--sharding_mode", "none"]
    train.main(args + ["--output_dir", str(out)])
    assert os.path.isfile(out / "model.safetensors") and os.path.isfile(out / "config.json")
    m = LlamaForCausalLM.from_pretrained(str(out), torch_dtype=torch.bfloat16)
    assert m.config.num_hidden_layers == 1 and m.config.vocab_size == 256
    train.main(args + ["--load_dir", str(out), "--use_te"])  # TE-layer model started from the saved HF-layout checkpoint


def test_train_harness_refuses_an_unsavable_layout_before_the_first_step(tmp_path, capsys, monkeypatch):
    """--use_te trains the TE-only MLP biases, which the HF layout (the default --save_layout) cannot hold: the run must say so
    before it spends a step, not after its last one; with --save_layout te it saves, and a second run starts from the files."""
    from safetensors.torch import load_file
    from llm_fp8_amd import train
    args = ["--model_name", "llama-3.2-1b", "--batch_size", "1", "--max_seq_length", "16", "--mixed_precision", "bf16", "--use_te",
            "--num_hidden_layers", "1", "--vocab_size", "256", "--num_steps", "2", "--sharding_mode", "none"]
    capsys.readouterr()
    with pytest.raises(ValueError, match="--save_layout te"):
        train.main(args + ["--output_dir", str(tmp_path / "hf")])
    assert '"step"' not in capsys.readouterr().out, "the harness trained before it refused"
    assert not (tmp_path / "hf").exists()
    out = tmp_path / "te"
    train.main(args + ["--output_dir", str(out), "--save_layout", "te"])
    printed = capsys.readouterr().out
    assert printed.count('"step"') == 2 and '"saved"' in printed
    saved = load_file(str(out / "model.safetensors"))
    bias = saved["model.layers.0.layernorm_mlp.fc1_bias"]
    assert bool(torch.count_nonzero(bias)), "the bias did not train: the refusal above would have been for nothing"
    seen = {}
    real = train.create_optimizer

    def spy(model, cfg):
        seen.update({n: p.detach().clone() for n, p in model.named_parameters()})
        return real(model, cfg)

    monkeypatch.setattr(train, "create_optimizer", spy)
    train.main(args + ["--load_dir", str(out), "--num_steps", "1"])
    assert '"step": 0' in capsys.readouterr().out
    assert len(seen) > 0
    for n, p in seen.items():  # what the second run started from: the files, bit for bit (lm_head.weight is tied, not stored)
        if n in saved:
            assert torch.equal(p.view(torch.int16), saved[n].view(torch.int16)), n
    assert "model.layers.0.layernorm_mlp.fc1_bias" in seen and "model.layers.0.self_attention.proj.weight" in seen


def test_gradient_accumulation_matches_the_large_batch():
    """train_step with N micro-batches = one step on the N x batch (loss / N, one optimiser step; train_multi_gpu.py:661,714-737)."""
    from llm_fp8_amd import train
    cfg = train.TrainingConfig(model_name="llama-3.2-1b", batch_size=2, max_seq_length=16, mixed_precision="bf16", use_te=False,
                               num_hidden_layers=1, vocab_size=128, sharding_mode="none", num_warmup_steps=0, learning_rate=1e-3)
    dev = torch.device("cpu")

    def fresh():
        torch.manual_seed(7)
        m = train.create_model(cfg, dev).float()
        opt, sched = train.create_optimizer(m, cfg)
        m.train()
        grads = {}
        step = opt.step

        def spy(*a, **k):  # gradients as the optimiser sees them (AdamW's first update is ~lr * sign(g): compare g, not w)
            grads.update({n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None})
            return step(*a, **k)

        opt.step = spy
        return m, opt, sched, grads

    g = torch.Generator().manual_seed(3)
    mbs = [train.synthetic_batch(cfg, 128, dev, generator=g) for _ in range(4)]
    big = {k: torch.cat([mb[k] for mb in mbs]) for k in mbs[0]}
    m1, o1, s1, g1 = fresh()
    l1 = train.train_step(m1, mbs, o1, s1, cfg)
    m2, o2, s2, g2 = fresh()
    l2 = train.train_step(m2, big, o2, s2, cfg)
    assert abs(float(l1.detach()) - float(l2.detach())) < 1e-5
    assert g1.keys() == g2.keys() and len(g1) > 0
    for k in g1:
        assert torch.allclose(g1[k], g2[k], rtol=1e-4, atol=1e-7), k
    assert s1.last_epoch == s2.last_epoch == 1  # ONE scheduler step per accumulation window
