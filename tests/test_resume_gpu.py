"""GPU: an interrupted run continues bit for bit.  A tiny model (2 layers, hidden 512, 4 heads of 128, 2 KV heads, FFN 1024, vocab
512, batch 2 x 128: every GEMM dimension a 256-multiple, so the persistent GEMMs, the fused casts, the flash attention and the
optimiser's sink path run) trains 4 steps straight; a second run stops after 2, writes the model through checkpoint.save_pretrained
and the optimiser / scheduler state through torch.save, drops everything, rebuilds from ANOTHER seed, loads (model first, optimiser
second) and trains 2 more.  Losses, parameters, optimiser state and -- delayed scaling -- amax histories and scales must be the
straight run's, bitwise: the kernels are deterministic, the resumed forward casts the weights with the saved scale (the bytes the
optimiser's sink emission gives) and re-deposits the same weight amax by `max` into the saved history row 0.  No tolerance applies.

Negative controls (a resume without the `_extra_state` keys, a resume without the optimiser state) must DIFFER, so the comparison
would notice a loss.  Two more: a load followed by a save before any forward keeps the FP8 state, and a checkpoint of another
amax_history_len is refused before anything is written."""
import contextlib
import dataclasses
import io
import os
import shutil

import pytest
import torch

pytestmark = pytest.mark.gpu

SEED, OTHER_SEED = 31, 977      # the run's initial weights | the rebuilt model's: nothing of it may survive the load
STEPS, CUT = 4, 2
STATE_KEYS = ("step", "exp_avg", "exp_avg_sq", "master")
TINY = dict(hidden_size=512, intermediate_size=1024, num_attention_heads=4, num_key_value_heads=2, head_dim=128)


@dataclasses.dataclass(frozen=True)
class Case:
    scenario: str = "default"
    opt_state: str = "bf16"
    layout: str = "te"
    model: str = "llama-3.2-3b"
    ga: int = 1

    def __str__(self):
        return "-".join(str(v) for v in dataclasses.astuple(self))


CASES = ([Case(s) for s in ("default", "hybrid", "mxfp8", "current", "block")]
         + [Case(s, o) for s in ("default", "mxfp8") for o in ("fp32", "bf16_sr")]   # both sink kinds x master re-keying / the SR stream
         + [Case(layout="hf"),           # train.save_model: HF names + fp8_extra_state.safetensors, replace_params on the way back
            Case(model="qwen3-0.6b"),    # q_norm / k_norm ride through the file
            Case(ga=2)])                 # the save falls between two accumulation windows


def _bits(t):
    return t.detach().contiguous().view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


@contextlib.contextmanager
def _env():
    """The tiny shapes behind the config tables, none of the A/B switches, a clean FP8 state before and after."""
    from llm_fp8_amd import llama, qwen
    from llm_fp8_amd.pytorch.fp8 import FP8GlobalStateManager as G
    mp = pytest.MonkeyPatch()
    lc, qc = llama.llama_config, qwen.qwen3_config
    mp.setattr(llama, "llama_config", lambda name, **kw: lc(name, **{**TINY, **kw}))
    mp.setattr(qwen, "qwen3_config", lambda name, **kw: qc(name, **{**TINY, "max_position_embeddings": 256, **kw}))
    for v in ("LLM_FP8_AMD_NO_OPT_WCAST", "LLM_FP8_AMD_OPT_STATE", "LLM_FP8_AMD_TORCH_ADAMW", "LLM_FP8_AMD_NO_STEP_GUARD"):
        mp.delenv(v, raising=False)
    G.reset()
    try:
        yield mp
    finally:
        mp.undo()
        G.reset()


def _cfg(case: Case, **kw):
    from llm_fp8_amd import train
    qwen3 = case.model.startswith("qwen3")  # (1e-2 there: a norm weight near 1 has a bf16 spacing of 2^-7, test_qwen3_gpu.py)
    return train.TrainingConfig(model_name=case.model, batch_size=2, max_seq_length=128, mixed_precision="fp8", fp8_scenario=case.scenario,
                                use_te=True, sharding_mode="none", num_hidden_layers=2, vocab_size=512, learning_rate=1e-2 if qwen3 else 1e-3,
                                num_warmup_steps=0, gradient_accumulation_steps=case.ga, optimizer_state=case.opt_state, **kw)


def _batches(case: Case, device):
    from llm_fp8_amd import train
    gen = torch.Generator(device=device).manual_seed(12)
    cfg = _cfg(case)
    steps = [[train.synthetic_batch(cfg, 512, device, gen) for _ in range(case.ga)] for _ in range(STEPS)]
    return [mbs if case.ga > 1 else mbs[0] for mbs in steps]


def _build(case: Case, device, seed):
    from llm_fp8_amd import train
    from llm_fp8_amd.optim import ClippedAdamW
    from llm_fp8_amd.pytorch.fp8 import FP8GlobalStateManager as G
    G.reset()
    cfg = _cfg(case)
    torch.manual_seed(seed)
    model = train.prepare_model(train.create_model(cfg, device), cfg)
    with torch.no_grad():
        for n, p in model.named_parameters():
            if seed == SEED and n.endswith(("q_norm.weight", "k_norm.weight")):
                p.copy_(0.5 + torch.rand(p.shape, device=device))  # away from one: a gamma the file dropped must show
            if case.layout == "hf" and n.endswith(("fc1_bias", "fc2_bias")):
                p.requires_grad_(False)  # the HF layout cannot hold a trained TE-only MLP bias
    model.train()
    opt, sched = train.create_optimizer(model, cfg)
    assert isinstance(opt, ClippedAdamW) and opt._mode == case.opt_state
    return model, opt, sched, cfg


def _snapshot(model, opt):
    from llm_fp8_amd.pytorch.fp8 import FP8GlobalStateManager as G
    names = {p: n for n, p in model.named_parameters()}
    return {"params": {n: p.detach().clone() for n, p in model.named_parameters()},
            "state": {names[p]: {k: (v.detach().clone() if torch.is_tensor(v) else v) for k, v in st.items() if k in STATE_KEYS}
                      for p, st in opt.state.items()},
            "arenas": {key: {"used": a.used, "hist": a.hist[:, :a.used].clone(), "scale": a.scale[:a.used].clone(),
                             "scale_inv": a.scale_inv[:a.used].clone()} for key, a in G._arenas.items()}}


def _train(model, opt, sched, cfg, batches):
    from llm_fp8_amd import train
    return [train.train_step(model, b, opt, sched, cfg).detach().float().clone() for b in batches]


def _straight(case, device, batches):
    model, opt, sched, cfg = _build(case, device, SEED)
    losses = _train(model, opt, sched, cfg, batches)
    return dict(_snapshot(model, opt), losses=losses)


def _first_half(case, device, batches, out_dir):
    """Two steps, then the files: the model in `case.layout`, optimizer.pt, scheduler.pt.  Returns the two losses."""
    from llm_fp8_amd import checkpoint, train
    model, opt, sched, cfg = _build(case, device, SEED)
    losses = _train(model, opt, sched, cfg, batches[:CUT])
    if case.layout == "hf":
        train.save_model(model, dataclasses.replace(cfg, output_dir=out_dir), "hf")
        assert os.path.isfile(os.path.join(out_dir, checkpoint.EXTRA_SINGLE))
    else:
        checkpoint.save_pretrained(model, out_dir, layout="te")
    torch.save(opt.state_dict(), os.path.join(out_dir, "optimizer.pt"))
    torch.save(sched.state_dict(), os.path.join(out_dir, "scheduler.pt"))
    return losses


def _load(case, device, ckpt, load_opt=True):
    """A fresh model and optimiser from another seed, then the files: the model first, the optimiser second."""
    from llm_fp8_amd import checkpoint
    model, opt, sched, cfg = _build(case, device, OTHER_SEED)
    checkpoint.load_into(model, ckpt, model.config, strict=True)
    if load_opt:
        opt.load_state_dict(torch.load(os.path.join(ckpt, "optimizer.pt"), weights_only=True))
    sched.load_state_dict(torch.load(os.path.join(ckpt, "scheduler.pt"), weights_only=True))
    return model, opt, sched, cfg


def _second_half(case, device, batches, ckpt, first_losses, **kw):
    model, opt, sched, cfg = _load(case, device, ckpt, **kw)
    losses = first_losses + _train(model, opt, sched, cfg, batches[CUT:])
    return dict(_snapshot(model, opt), losses=losses)


def _assert_same(got, want, case):
    assert len(got["losses"]) == len(want["losses"]) == STEPS
    for i, (a, b) in enumerate(zip(got["losses"], want["losses"])):
        assert torch.equal(_bits(a), _bits(b)), f"{case}: loss of step {i + 1} {a.item()!r} != {b.item()!r}"
    assert got["params"].keys() == want["params"].keys()
    for n, b in want["params"].items():
        a = got["params"][n]
        assert a.dtype == b.dtype == torch.bfloat16 and torch.equal(a.view(torch.int16), b.view(torch.int16)), f"{case}: parameter {n}"
    assert got["state"].keys() == want["state"].keys() and len(want["state"]) > 0
    for n, ws in want["state"].items():
        gs = got["state"][n]
        assert gs.keys() == ws.keys() and {"step", "exp_avg", "exp_avg_sq"} <= ws.keys(), (case, n, sorted(gs), sorted(ws))
        assert ("master" in ws) == (case.opt_state == "fp32")
        for k, b in ws.items():
            a = gs[k]
            if torch.is_tensor(b):
                assert torch.is_tensor(a) and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b)), f"{case}: {k} of {n}"
            else:
                assert a == b == STEPS, f"{case}: {k} of {n}: {a} / {b}"
    assert got["arenas"].keys() == want["arenas"].keys()
    assert bool(want["arenas"]) == (case.scenario not in ("current", "block")), "delayed-scaling state where none is expected, or none where it is"
    for key, wa in want["arenas"].items():
        ga = got["arenas"][key]
        assert ga["used"] == wa["used"] > 0, (case, key)
        for k in ("hist", "scale", "scale_inv"):
            assert torch.equal(_bits(ga[k]), _bits(wa[k])), f"{case}: {k} of arena {key}"


def _differs(got, want) -> bool:
    """The step-3 loss or the final weights are not the straight run's."""
    return (not torch.equal(_bits(got["losses"][CUT]), _bits(want["losses"][CUT]))
            or any(not torch.equal(got["params"][n].view(torch.int16), b.view(torch.int16)) for n, b in want["params"].items()))


def _decode(blob):
    return torch.load(io.BytesIO(blob.cpu().numpy().tobytes()), weights_only=True)


@pytest.fixture(scope="module")
def default_run(dev, tmp_path_factory):
    """Scenario `default` once for every test that resumes it: the batches, the straight run, the 2-step checkpoint."""
    case, device = Case(), torch.device(dev)
    ckpt = str(tmp_path_factory.mktemp("default_2_steps"))
    with _env():
        batches = _batches(case, device)
        straight = _straight(case, device, batches)
        first = _first_half(case, device, batches, ckpt)
    return {"case": case, "batches": batches, "straight": straight, "ckpt": ckpt, "first": first}


@pytest.mark.parametrize("case", CASES, ids=str)
def test_interrupted_run_continues_bit_for_bit(dev, default_run, tmp_path, case):
    device = torch.device(dev)
    with _env():
        if case == default_run["case"]:
            batches, straight, ckpt, first = (default_run[k] for k in ("batches", "straight", "ckpt", "first"))
        else:
            batches, ckpt = _batches(case, device), str(tmp_path / "ckpt")
            straight = _straight(case, device, batches)
            first = _first_half(case, device, batches, ckpt)
        resumed = _second_half(case, device, batches, ckpt, first)
    if case.model.startswith("qwen3"):
        assert sum(n.endswith(("q_norm.weight", "k_norm.weight")) for n in straight["params"]) == 4
    _assert_same(resumed, straight, case)


@pytest.mark.parametrize("lost", ["extra_state", "optimizer"])
def test_a_resume_that_loses_state_differs(dev, default_run, tmp_path, lost):
    """The controls of the test above: without the `_extra_state` keys in the files (every scale back at 1, the histories empty),
    or without the optimiser state (moments and step count back at zero), step 3 must not be the straight run's."""
    from safetensors.torch import load_file, save_file
    from llm_fp8_amd import checkpoint
    case, device, ckpt = default_run["case"], torch.device(dev), default_run["ckpt"]
    if lost == "extra_state":
        ckpt = str(tmp_path / "no_extra")
        shutil.copytree(default_run["ckpt"], ckpt)
        fn = os.path.join(ckpt, checkpoint.SAFE_SINGLE)
        state = load_file(fn)
        kept = {k: v for k, v in state.items() if not k.endswith("_extra_state")}
        assert 0 < len(kept) < len(state)
        save_file(kept, fn, metadata={"format": "pt"})
    with _env():
        resumed = _second_half(case, device, default_run["batches"], ckpt, default_run["first"], load_opt=lost != "optimizer")
    assert _differs(resumed, default_run["straight"]), f"a resume without the {lost} went unnoticed"


def test_load_then_save_before_any_forward_keeps_the_fp8_state(dev, default_run, tmp_path):
    """Load the 2-step checkpoint into a fresh model and save it again at once: every `_extra_state` of the second save holds the
    tensors of the first, and a resume from the second save is the straight run."""
    from safetensors.torch import load_file
    from llm_fp8_amd import checkpoint
    case, device, ckpt = default_run["case"], torch.device(dev), default_run["ckpt"]
    again = str(tmp_path / "again")
    with _env():
        model, opt, sched, _ = _load(case, device, ckpt)
        checkpoint.save_pretrained(model, again, layout="te")
        del model, opt, sched
        for fn in ("optimizer.pt", "scheduler.pt"):
            shutil.copy(os.path.join(ckpt, fn), os.path.join(again, fn))
        a, b = (load_file(os.path.join(d, checkpoint.SAFE_SINGLE)) for d in (ckpt, again))
        assert a.keys() == b.keys()
        with_state = 0
        for k in (k for k in a if k.endswith("_extra_state")):
            assert a[k].numel() > 0, f"{k}: the checkpoint of a delayed-scaling run carries no state here"
            assert b[k].numel() > 0, f"{k}: the save before the first forward dropped the loaded FP8 state"
            da, db = _decode(a[k]), _decode(b[k])
            for d in ("fwd", "bwd"):
                for f in ("scale", "scale_inv", "amax_history"):
                    assert db[d][f].dtype == da[d][f].dtype and torch.equal(_bits(db[d][f]), _bits(da[d][f])), (k, d, f)
            with_state += 1
        assert with_state == 2 * 3 + 1  # per layer layernorm_qkv, proj, layernorm_mlp; the lm_head
        resumed = _second_half(case, device, default_run["batches"], again, default_run["first"])
    _assert_same(resumed, default_run["straight"], case)


def test_checkpoint_of_another_history_length_is_refused_whole(dev, default_run):
    """The checkpoint was written under amax_history_len 16; the decoder of the model it is loaded into runs 8.  The first FP8
    forward raises -- and so does the next: the state stays pending, no slot is taken and no arena is written; ModuleMeta.load_state
    itself refuses before it touches scale, scale_inv or the generation counter."""
    from llm_fp8_amd import checkpoint, llama
    from llm_fp8_amd.common.recipe import DelayedScaling, Format
    from llm_fp8_amd.pytorch.fp8 import FP8GlobalStateManager as G, ModuleMeta
    case, device = default_run["case"], torch.device(dev)
    attn = DelayedScaling(fp8_format=Format.HYBRID, amax_history_len=8, amax_compute_algo="max")
    mlp = DelayedScaling(fp8_format=Format.E4M3, amax_history_len=8, amax_compute_algo="max")
    with _env() as mp:
        mp.setattr(llama, "scenario_recipes", lambda scenario: (attn, mlp))
        model, _, _, _ = _build(case, device, OTHER_SEED)
        checkpoint.load_into(model, default_run["ckpt"], model.config, strict=True)
        qkv = model.model.layers[0].self_attention.layernorm_qkv
        for _ in range(2):
            with pytest.raises(RuntimeError, match="amax history length 16 in checkpoint != recipe's 8"):
                model(**default_run["batches"][0])
            assert qkv._meta_fwd is None and qkv._pending_state is not None
            for a in G._arenas.values():
                assert a.used == 0 and a.generation == 0, a.key
                assert not a.hist.any() and bool((a.scale == 1).all()) and bool((a.scale_inv == 1).all()), a.key
        st = qkv._pending_state["fwd"]
        n = st["scale"].numel()
        assert not bool((st["scale"] == 1).all()), "the saved scales are the defaults: an overwrite would not show"
        arena = G.arena(attn, True, device)
        meta = ModuleMeta(arena, arena.alloc(n), n)
        gen = arena.generation
        with pytest.raises(RuntimeError, match="amax history length 16"):
            meta.load_state(st)
        assert arena.generation == gen and not arena.hist.any()
        assert bool((arena.scale == 1).all()) and bool((arena.scale_inv == 1).all()), "scales were written before the refusal"
