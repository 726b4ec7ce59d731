"""GPU: new weights in a model that has already stepped.  After two training steps every GEMM weight has FP8 copies the optimiser
keeps current (module.WeightSink under `default`, module.MXWeightSink under `mxfp8`), declared fresh by the parts' `_version`.  A
write to a weight must make the next forward quantise it again: the sequence

    2 training steps -> a write -> 1 evaluation forward under no_grad -> 2 training steps

is run as it is and with LLM_FP8_AMD_NO_OPT_WCAST=1 (every forward casts for itself); all losses, the evaluation loss, the parameters
and the moments must agree bit for bit, and the evaluation forward must have re-quantised every weight part of every operand the
write touched (and nothing else).  Control: with module._part_versions returning a constant the sinks never go stale, and the run
must DIFFER from the cast-always run.

One asymmetry is designed around, not tested: under delayed scaling the optimiser deposits amax(w) of the weights it has just
written into history row 0, for a forward that -- after a write -- never runs on them; the cast-always run never sees that value.
The two runs agree only where the written operand's amax is at least the replaced one's (row 0 is a `max`).  Every write here
grows the amax (another seed's weights times 2; factors of 1.5), and the test asserts that precondition."""
import contextlib

import pytest
import torch

pytestmark = pytest.mark.gpu

SEED, OTHER_SEED = 31, 977
TINY = dict(hidden_size=512, intermediate_size=1024, num_attention_heads=4, num_key_value_heads=2, head_dim=128)
WRITES = ("load_state_dict", "hf_dir", "one_part", "detached")
# weight parts the evaluation forward must quantise again: 2 layers x (q, k, v, proj, fc1, fc2) after a whole-model write; the
# three parts of layer 1's q | k | v operand after a write to its key part alone; layer 0's fc2
RECAST = {"load_state_dict": 12, "hf_dir": 12, "one_part": 3, "detached": 1}
_CACHE = {}  # (scenario, write) -> the cast-always run, shared by the comparison and the control


@contextlib.contextmanager
def _env(nowcast: bool):
    from llm_fp8_amd import llama
    from llm_fp8_amd.pytorch.fp8 import FP8GlobalStateManager as G
    mp = pytest.MonkeyPatch()
    lc = llama.llama_config
    mp.setattr(llama, "llama_config", lambda name, **kw: lc(name, **{**TINY, **kw}))
    for v in ("LLM_FP8_AMD_OPT_STATE", "LLM_FP8_AMD_TORCH_ADAMW", "LLM_FP8_AMD_NO_STEP_GUARD"):
        mp.delenv(v, raising=False)
    if nowcast:
        mp.setenv("LLM_FP8_AMD_NO_OPT_WCAST", "1")
    else:
        mp.delenv("LLM_FP8_AMD_NO_OPT_WCAST", raising=False)
    G.reset()
    try:
        yield mp
    finally:
        mp.undo()
        G.reset()


def _cfg(scenario):
    from llm_fp8_amd import train
    return train.TrainingConfig(model_name="llama-3.2-3b", batch_size=2, max_seq_length=128, mixed_precision="fp8", fp8_scenario=scenario,
                                use_te=True, sharding_mode="none", num_hidden_layers=2, vocab_size=512, learning_rate=1e-3,
                                num_warmup_steps=0)


def _model(scenario, device, seed):
    from llm_fp8_amd import train
    from llm_fp8_amd.pytorch.fp8 import FP8GlobalStateManager as G
    G.reset()
    cfg = _cfg(scenario)
    torch.manual_seed(seed)
    return train.prepare_model(train.create_model(cfg, device), cfg), cfg


@pytest.fixture(scope="module")
def other(dev, tmp_path_factory):
    """Another seed's weights, times 2 (see the module docstring): as a state dict without the `_extra_state` keys, and as an
    HF-layout directory."""
    from llm_fp8_amd import checkpoint
    hf_dir = str(tmp_path_factory.mktemp("other_hf"))
    with _env(False):
        model, _ = _model("default", torch.device(dev), OTHER_SEED)
        with torch.no_grad():
            for p in model.parameters():
                p.mul_(2.0)  # (the TE-only MLP biases are zero and stay zero: the HF layout can hold the model)
        sd = {k: v.detach().clone() for k, v in model.state_dict().items() if not k.endswith("_extra_state")}
        checkpoint.save_pretrained(model, hf_dir, layout="hf")
    return {"sd": sd, "hf_dir": hf_dir}


def _grows(new, old):
    assert float(new.abs().max()) >= float(old.abs().max()) > 0, "the write does not grow the operand's amax (module docstring)"


def _write(kind, model, other):
    """The write, and the precondition on the amax of every GEMM weight it replaces."""
    from llm_fp8_amd import checkpoint
    l0, l1 = model.model.layers[0], model.model.layers[1]
    if kind in ("load_state_dict", "hf_dir"):
        for n, p in model.named_parameters():
            if p.dim() == 2:
                _grows(other["sd"][n], p.detach())
        if kind == "load_state_dict":  # only the version counters can catch it: no `_extra_state`, so no arena generation moves
            res = model.load_state_dict(other["sd"], strict=False)
            assert not res.unexpected_keys and all(k.endswith("_extra_state") for k in res.missing_keys)
        else:                          # llama.replace_params: copy_ on state-dict tensors, [:f] / [f:] slice copies into fc1_weight
            checkpoint.load_into(model, other["hf_dir"], model.config)
        got = model.state_dict()
        for k in ("model.layers.1.layernorm_mlp.fc1_weight", "model.layers.0.self_attention.layernorm_qkv.key_weight", "model.embed_tokens.weight"):
            assert torch.equal(got[k], other["sd"][k]), f"{k} was not written"
    elif kind == "one_part":           # one part of a multi-part operand: the whole q | k | v sink must go stale
        with torch.no_grad():
            l1.self_attention.layernorm_qkv.key_weight.mul_(1.5)
    elif kind == "detached":           # a detached alias shares the version counter
        l0.layernorm_mlp.fc2_weight.detach().mul_(1.5)
    else:
        raise ValueError(kind)


def _run(scenario, write, dev, other, nowcast, mutant=False):
    from llm_fp8_amd import train
    from llm_fp8_amd.optim import ClippedAdamW
    from llm_fp8_amd.pytorch import module as M, ops
    device = torch.device(dev)
    with _env(nowcast) as mp:
        if mutant:
            mp.setattr(M, "_part_versions", lambda parts: (0,) * len(parts))
        seen = {"on": False, "n": 0}
        entry = "mxfp8_quantize" if scenario == "mxfp8" else "cast_amax"
        real = getattr(ops, entry)

        def counting(x, *a, **k):
            if seen["on"] and (isinstance(x, torch.nn.Parameter) or x.requires_grad and x.is_leaf):
                seen["n"] += 1
            return real(x, *a, **k)

        mp.setattr(ops, entry, counting)
        model, cfg = _model(scenario, device, SEED)
        model.train()
        opt, sched = train.create_optimizer(model, cfg)
        assert isinstance(opt, ClippedAdamW)
        gen = torch.Generator(device=device).manual_seed(12)
        batches = [train.synthetic_batch(cfg, 512, device, gen) for _ in range(5)]
        losses = [train.train_step(model, b, opt, sched, cfg).detach().float().clone() for b in batches[:2]]
        sinks = [s for m in model.modules() for k, s in getattr(m, "_wcache", {}).items() if isinstance(k, tuple) and k[0] in ("sink", "mxsink")]
        if nowcast:
            assert not any(s.fresh() for s in sinks)
        else:  # per layer q | k | v, proj, fc1, fc2 (+ the lm_head under its delayed-scaling outer recipe)
            assert len(sinks) >= 8 and all(s.fresh() for s in sinks), "not every sink is fresh after two steps"
        _write(write, model, other)
        model.eval()
        seen["on"] = True
        with torch.no_grad():
            ev = model(**batches[2]).loss.detach().float().clone()
        seen["on"] = False
        model.train()
        losses += [train.train_step(model, b, opt, sched, cfg).detach().float().clone() for b in batches[3:]]
        params = {n: p.detach().clone() for n, p in model.named_parameters()}
        names = {p: n for n, p in model.named_parameters()}
        moments = {names[p]: (st["exp_avg"].clone(), st["exp_avg_sq"].clone()) for p, st in opt.state.items()}
    return {"losses": losses, "eval": ev, "params": params, "moments": moments, "recast": seen["n"]}


def _cast_always(scenario, write, dev, other):
    if (scenario, write) not in _CACHE:
        _CACHE[scenario, write] = _run(scenario, write, dev, other, nowcast=True)
    return _CACHE[scenario, write]


def _i32(t):
    return t.view(torch.int32)


def _mismatches(a, b):
    out = [f"loss {i + 1}" for i, (x, y) in enumerate(zip(a["losses"], b["losses"])) if not torch.equal(_i32(x), _i32(y))]
    if not torch.equal(_i32(a["eval"]), _i32(b["eval"])):
        out.append("evaluation loss")
    assert a["params"].keys() == b["params"].keys() and a["moments"].keys() == b["moments"].keys() and len(a["moments"]) > 0
    out += [f"parameter {n}" for n, p in a["params"].items() if not torch.equal(p.view(torch.int16), b["params"][n].view(torch.int16))]
    for n, ms in a["moments"].items():
        for name, x, y in zip(("exp_avg", "exp_avg_sq"), ms, b["moments"][n]):
            if x.dtype != y.dtype or not torch.equal(x.view(torch.int16), y.view(torch.int16)):
                out.append(f"{name} of {n}")
    return out


@pytest.mark.parametrize("write", WRITES)
@pytest.mark.parametrize("scenario", ["default", "mxfp8"])
def test_a_write_to_a_stepped_weight_reaches_the_next_forward(dev, other, scenario, write):
    as_is = _run(scenario, write, dev, other, nowcast=False)
    always = _cast_always(scenario, write, dev, other)
    assert len(as_is["losses"]) == len(always["losses"]) == 4
    bad = _mismatches(as_is, always)
    assert not bad, f"{scenario} / {write}: differs from the cast-always run in {len(bad)} place(s): {bad[:6]}"
    assert always["recast"] == 12, always["recast"]  # the yardstick of the count: every decoder weight part, once
    assert as_is["recast"] == RECAST[write], f"{scenario} / {write}: the evaluation forward re-quantised {as_is['recast']} weight parts"


@pytest.mark.parametrize("scenario", ["default", "mxfp8"])
def test_sinks_that_ignore_the_version_counters_are_noticed(dev, other, scenario):
    """The mutant keeps running on the FP8 images of the weights load_state_dict replaced."""
    mutant = _run(scenario, "load_state_dict", dev, other, nowcast=False, mutant=True)
    always = _cast_always(scenario, "load_state_dict", dev, other)
    assert mutant["recast"] == 0
    assert _mismatches(mutant, always), "stale FP8 weight copies went unnoticed"
