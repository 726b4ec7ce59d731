"""The FP8 modules under every requires_grad pattern.

The GEMM Functions read ctx.needs_input_grad and decide from it which FP8 copies every cast kernel writes, what is kept for backward,
which backward GEMMs run (and whether as one grouped launch), and which Function carries the delayed-scaling backward update.  The rest
of the suite builds every module all-trainable, so only one value of each of those branches is run there.

Oracle: the ALL-TRAINABLE TWIN, bit for bit.  A module under pattern P (the set of its tensor inputs that require grad) must give the
same output bits, the same gradient bits for every tensor in P, `.grad is None` for every other one, and -- delayed scaling -- the same
amax histories and scales as an identical module with everything trainable, fed the same x / dy in its own fresh FP8 state.  No tolerance:
the cast kernels write the same bytes of one copy whether or not the other is written, `_grouped_or_two` is bitwise the same either way,
and the column-sum / RMSNorm-backward finishes add in a fixed order.  The all-trainable path itself is held to the float64 / oracle
references by test_modules_gpu.py, test_current_scaling_gpu.py and test_block_scaling_gpu.py; bit equality carries that to every pattern.

One state exclusion: under a LayerNormMLP pattern inside {fc2_weight, fc2_bias} nothing upstream of the activation needs a gradient, fc1's
grad_output is never formed, and fc1's backward amax slots (backward slots 0 and 1 of the module) stay as they were.  Every other site
publishes its amax under every pattern: a bias-only site still quantises its grad_output (the column sums ride on the row-wise copy).
"""
import itertools

import pytest
import torch

pytestmark = pytest.mark.gpu

B, S, H, FFN = 2, 128, 512, 768   # 256 tokens; 512 = the smallest width the fused RMSNorm takes; all multiples of 256 (grouped launch)
QKV = {"query_": 512, "key_": 128, "value_": 128}
MODES = {"delayed": ("off", "plan"), "mxfp8": ("off", "plan"), "current": ("plan",), "block": ("plan",)}
RECIPE_MODE = [(r, m) for r, ms in MODES.items() for m in ms]


@pytest.fixture()
def te(dev):
    import llm_fp8_amd.pytorch as te_
    from llm_fp8_amd.pytorch.fp8 import FP8GlobalStateManager
    FP8GlobalStateManager.reset()
    yield te_
    FP8GlobalStateManager.reset()


def _recipe(name):
    from llm_fp8_amd.common.recipe import DelayedScaling, Float8BlockScaling, Float8CurrentScaling, Format, MXFP8BlockScaling
    if name == "delayed":
        return DelayedScaling(fp8_format=Format.HYBRID, amax_history_len=4, amax_compute_algo="max")
    return {"mxfp8": MXFP8BlockScaling, "current": Float8CurrentScaling, "block": Float8BlockScaling}[name]()


def _bits_equal(a, b) -> bool:
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    return torch.equal(a.detach().contiguous().reshape(-1).view(torch.uint8), b.detach().contiguous().reshape(-1).view(torch.uint8))


def _subsets(groups):
    names = list(groups)
    for n in range(1, len(names) + 1):
        for combo in itertools.combinations(names, n):
            yield frozenset(t for gname in combo for t in groups[gname])


class _GemmCounter:
    """Counts GEMM problems launched through llm_fp8_amd.pytorch.ops (a grouped launch counts its problems)."""

    def __init__(self, monkeypatch):
        from llm_fp8_amd.pytorch import ops
        self.problems = self.grouped = 0
        for name in ("gemm_fp8", "gemm_mxfp8"):
            monkeypatch.setattr(ops, name, self._wrap(getattr(ops, name), False))
        for name in ("gemm_fp8_grouped", "gemm_mxfp8_grouped"):
            monkeypatch.setattr(ops, name, self._wrap(getattr(ops, name), True))

    def _wrap(self, fn, grouped):
        def counted(*a, **kw):
            if grouped:
                self.grouped += 1
                self.problems += len(a[0])
            else:
                self.problems += 1
            return fn(*a, **kw)
        return counted


class _Case:
    """One module variant: how to build it, its pattern groups, how to call it."""

    def __init__(self, name, build, groups, n_out, extra=(), call=None, skip=False, bwd_gemms=None, state_exempt=None):
        self.name, self.build, self.groups, self.n_out, self.extra = name, build, groups, n_out, tuple(extra)
        self.call = call or (lambda m, x: m(x))
        self.skip, self.bwd_gemms, self.state_exempt = skip, bwd_gemms, state_exempt
        self.all = frozenset(t for ts in groups.values() for t in ts)

    def patterns(self):
        return list(_subsets(self.groups)) + [frozenset(p) for p in self.extra]


def _linear_gemms(ln, weights):
    def n(P):
        return int("x" in P or (ln is not None and ln in P)) + int(any(w in P for w in weights))
    return n


def _mlp_gemms(P):
    d = "x" in P or "layer_norm_weight" in P
    dact = d or "fc1_weight" in P or "fc1_bias" in P
    return int(dact) + int("fc2_weight" in P) + int(d) + int("fc1_weight" in P)


def _mlp_exempt(P):
    """Backward amax slots left alone under P: fc1's, when nothing upstream of the activation needs a gradient (module docstring)."""
    return (0, 1) if P <= {"fc2_weight", "fc2_bias"} else ()


def _cases(te, dev):
    bf = dict(params_dtype=torch.bfloat16, device=dev)
    qkv_w, qkv_b = [f"{n}weight" for n in QKV], [f"{n}bias" for n in QKV]
    lnl_groups = {"x": ["x"], "ln": ["layer_norm_weight"], "w": qkv_w, "b": qkv_b}
    # partial patterns: query frozen with key and value trainable; only the key bias trainable
    lnl_extra = [{"key_weight", "value_weight"}, {"key_bias"}]
    mlp_groups = {n: [n] for n in ("x", "layer_norm_weight", "fc1_weight", "fc1_bias", "fc2_weight", "fc2_bias")}

    def lnl(fused):
        def build():
            m = te.LayerNormLinear(H, sum(QKV.values()), eps=1e-5, bias=True, normalization="RMSNorm", parameters_split=QKV, **bf)
            m.fused_norm = fused
            return m
        return build

    def mlp(fused=True):
        def build():
            m = te.LayerNormMLP(H, FFN, eps=1e-5, bias=True, normalization="RMSNorm", activation="swiglu", **bf)
            m.fused_norm = fused   # False: torch's RMSNorm, then the fused fc1 -> SwiGLU -> fc2 node applied WITHOUT a norm weight
            return m
        return build

    return {
        "linear_bias": _Case("Linear(512->768, bias)", lambda: te.Linear(H, 768, bias=True, **bf), {"x": ["x"], "w": ["weight"], "b": ["bias"]},
                             768, extra=[set()], bwd_gemms=_linear_gemms(None, ["weight"])),
        "linear_nobias": _Case("Linear(512->768, no bias)", lambda: te.Linear(H, 768, bias=False, **bf), {"x": ["x"], "w": ["weight"]},
                               768, extra=[set()], bwd_gemms=_linear_gemms(None, ["weight"])),
        "lnl_fused": _Case("LayerNormLinear(512->q512|k128|v128, fused RMSNorm)", lnl(True), lnl_groups, 768, extra=lnl_extra,
                           bwd_gemms=_linear_gemms("layer_norm_weight", qkv_w)),
        "lnl_unfused": _Case("LayerNormLinear(512->q512|k128|v128, unfused norm)", lnl(False), lnl_groups, 768, extra=lnl_extra,
                             bwd_gemms=_linear_gemms("layer_norm_weight", qkv_w)),
        "mlp": _Case("LayerNormMLP(512, 768, swiglu)", mlp(), mlp_groups, H, bwd_gemms=_mlp_gemms, state_exempt=_mlp_exempt),
        "mlp_skip": _Case("LayerNormMLP(512, 768, swiglu, _with_skip)", mlp(), mlp_groups, H, call=lambda m, x: m(x, _with_skip=True),
                          skip=True, bwd_gemms=_mlp_gemms, state_exempt=_mlp_exempt),
        "mlp_unfused_norm": _Case("LayerNormMLP(512, 768, swiglu, unfused norm)", mlp(False), mlp_groups, H, bwd_gemms=_mlp_gemms,
                                  state_exempt=_mlp_exempt),
    }


def _param_values(mod, seed):
    """Values for every parameter, none of them the constructor's ones / zeros: norm weights away from 1, biases away from 0."""
    g = torch.Generator().manual_seed(seed)
    vals = {}
    for name, p in mod.named_parameters():
        r = torch.randn(p.shape, generator=g)
        if "layer_norm_weight" in name:
            v = 1.0 + 0.25 * r
        elif name.endswith("bias"):
            v = 0.1 * r
        else:
            v = 0.05 * r
        vals[name] = v.to(torch.bfloat16)
    return vals


def _data(n_out, steps, dev, seed):
    """Per step (x, dy, dskip): magnitudes change from step to step so that the delayed scales leave 1.0 and keep moving."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for s in range(steps):
        x = (torch.randn(B, S, H, generator=g) * (0.5 + s)).to(torch.bfloat16).to(dev)
        dy = (torch.randn(B, S, n_out, generator=g) * 2.0 ** (3 * s - 6)).to(torch.bfloat16).to(dev)
        dskip = (torch.randn(B, S, H, generator=g) * 2.0 ** (2 * s - 5)).to(torch.bfloat16).to(dev)
        out.append((x, dy, dskip))
    return out


def _run(te, case, P, recipe, vals, data, counter=None):
    """The module under pattern P in fresh FP8 state -> one record per step: output, gradients, delayed-scaling state, backward GEMMs."""
    from llm_fp8_amd.pytorch.fp8 import FP8GlobalStateManager
    FP8GlobalStateManager.reset()
    mod = case.build()
    with torch.no_grad():
        for name, p in mod.named_parameters():
            p.copy_(vals[name])
    for name, p in mod.named_parameters():
        p.requires_grad_(name in P)
    mod.train()
    recs = []
    for x, dy, dskip in data:
        xd = x.clone().requires_grad_("x" in P)
        with te.fp8_autocast(enabled=True, fp8_recipe=recipe):
            out = case.call(mod, xd)
        y = out[0] if case.skip else out
        rec = {"y": y.detach().clone(), "y_requires_grad": y.requires_grad}
        n0 = counter.problems if counter is not None else 0
        if y.requires_grad:
            if case.skip:
                torch.autograd.backward([y, out[1]], [dy, dskip])
            else:
                y.backward(dy)
        rec["bwd_gemms"] = (counter.problems - n0) if counter is not None else None
        rec["grads"] = {"x": xd.grad, **{name: p.grad for name, p in mod.named_parameters()}}
        for p in mod.parameters():
            p.grad = None
        rec["fwd"] = None if mod._meta_fwd is None else mod._meta_fwd.state()
        rec["bwd"] = None if mod._meta_bwd is None else mod._meta_bwd.state()
        recs.append(rec)
    return recs


def _check_against_twin(case, recipe_name, mode, P, got, twin):
    where = f"{case.name} / {recipe_name} / grouped={mode} / pattern {sorted(P) or 'EMPTY'}"
    exempt = case.state_exempt(P) if case.state_exempt is not None else ()
    for step, (a, b) in enumerate(zip(got, twin)):
        at = f"{where} / step {step}"
        assert _bits_equal(a["y"], b["y"]), f"{at}: output differs from the all-trainable twin"
        assert a["y_requires_grad"] == bool(P), f"{at}: output requires_grad = {a['y_requires_grad']}"
        for name in case.all:
            if name in P:
                assert a["grads"][name] is not None, f"{at}: no gradient for {name}"
                assert _bits_equal(a["grads"][name], b["grads"][name]), f"{at}: gradient of {name} differs from the all-trainable twin"
            else:
                assert a["grads"][name] is None, f"{at}: {name} does not require grad but got a gradient"
        if P:
            assert a["bwd_gemms"] == case.bwd_gemms(P), (f"{at}: backward launched {a['bwd_gemms']} GEMM problems, "
                                                        f"{case.bwd_gemms(P)} results were asked for")
        if a["fwd"] is None:
            assert b["fwd"] is None
            continue
        keep = [i for i in range(a["bwd"]["scale"].shape[0]) if i not in exempt]
        for key in ("scale", "scale_inv", "amax_history"):
            assert _bits_equal(a["fwd"][key], b["fwd"][key]), f"{at}: forward {key} differs from the all-trainable twin"
            if P:  # (the empty pattern has no backward at all: nothing there to trigger a backward update, while the twin's has run)
                assert _bits_equal(a["bwd"][key][..., keep], b["bwd"][key][..., keep]), f"{at}: backward {key} differs from the all-trainable twin"


@pytest.mark.parametrize("recipe_name,mode", RECIPE_MODE)
@pytest.mark.parametrize("case_name", ["linear_bias", "linear_nobias", "lnl_fused", "lnl_unfused", "mlp", "mlp_skip", "mlp_unfused_norm"])
def test_every_pattern_equals_the_all_trainable_twin(te, dev, monkeypatch, case_name, recipe_name, mode):
    monkeypatch.setenv("LLM_FP8_AMD_GROUPED_GEMM", mode)
    case = _cases(te, dev)[case_name]
    recipe = _recipe(recipe_name)
    steps = 3 if recipe_name == "delayed" else 1   # the other recipes keep no state: a second step repeats the first
    vals = _param_values(case.build(), seed=11)
    data = _data(case.n_out, steps, dev, seed=12)
    counter = _GemmCounter(monkeypatch)
    twin = _run(te, case, case.all, recipe, vals, data, counter)
    # the twin is worth comparing with: it took the grouped launch exactly when asked to, its gradients are finite and not all zero,
    # and -- delayed scaling -- its backward scales have left 1.0 after the first step
    assert (counter.grouped > 0) == (mode == "plan"), f"{case.name} / {recipe_name}: {counter.grouped} grouped launches under grouped={mode}"
    for name, g in twin[0]["grads"].items():
        assert g is not None and torch.isfinite(g.float()).all() and g.float().abs().sum() > 0, f"{case.name} / {recipe_name}: twin gradient {name}"
    if recipe_name == "delayed":
        assert twin[0]["bwd"]["scale"][0].item() != 1.0 and twin[0]["fwd"]["scale"][0].item() != 1.0
    patterns = case.patterns()
    # every subset of the groups, the partial patterns and (Linear) the empty set: 8 / 4 for Linear, 17 for LayerNormLinear, 63 for the MLP
    assert len(set(patterns)) == len(patterns) == 2 ** len(case.groups) - 1 + len(case.extra), len(patterns)
    compared = 0
    for P in patterns:
        got = _run(te, case, P, recipe, vals, data, counter)
        assert len(got) == len(twin) == steps
        _check_against_twin(case, recipe_name, mode, P, got, twin)
        compared += sum(len(P) for _ in got)
    torch.cuda.synchronize()
    print(f"[frozen] {case.name} / {recipe_name} / grouped={mode}: {len(patterns)} patterns x {steps} steps, {compared} gradients compared bit for bit, "
          f"{counter.problems} GEMM problems launched ({counter.grouped} grouped launches)")
    assert compared == steps * sum(len(P) for P in patterns) > 0


# ---- the backward scale update with a frozen head of the model: the first FP8 module of the region has no backward ----
def _chain_run(te, dev, build_pair, call_first, frozen: bool, vals, data, recipe):
    from llm_fp8_amd.pytorch.fp8 import FP8GlobalStateManager
    FP8GlobalStateManager.reset()
    m0, m1 = build_pair()
    with torch.no_grad():
        for i, m in enumerate((m0, m1)):
            for name, p in m.named_parameters():
                p.copy_(vals[i][name])
    for p in m0.parameters():
        p.requires_grad_(not frozen)
    recs = []
    for x, dy, _ in data:
        xd = x.clone().requires_grad_(not frozen)
        with te.fp8_autocast(enabled=True, fp8_recipe=recipe):
            y = m1(call_first(m0, xd))
        y.backward(dy)
        recs.append({"bwd": m1._meta_bwd.state(), "grads": {n: p.grad.clone() for n, p in m1.named_parameters()}, "y": y.detach().clone()})
        for p in (*m0.parameters(), *m1.parameters()):
            p.grad = None
    return recs


@pytest.mark.parametrize("chain", ["linear_linear", "mlp_lnl"])
def test_backward_scales_update_behind_a_frozen_first_module(te, dev, monkeypatch, chain):
    """Module 0 fully frozen and x without grad, module 1 trainable, one autocast region: module 0's Function has no backward, yet
    module 1's backward amax history and scale must move exactly as in the all-trainable chain (the region's backward update runs once
    as long as ANY FP8 module of it has a backward)."""
    monkeypatch.setenv("LLM_FP8_AMD_GROUPED_GEMM", "plan")
    bf = dict(params_dtype=torch.bfloat16, device=dev)
    if chain == "linear_linear":
        build_pair = lambda: (te.Linear(H, H, bias=True, **bf), te.Linear(H, 768, bias=True, **bf))
    else:
        build_pair = lambda: (te.LayerNormMLP(H, FFN, eps=1e-5, bias=True, normalization="RMSNorm", activation="swiglu", **bf),
                              te.LayerNormLinear(H, sum(QKV.values()), eps=1e-5, bias=True, normalization="RMSNorm", parameters_split=QKV, **bf))
    recipe = _recipe("delayed")
    vals = [_param_values(m, seed=21 + i) for i, m in enumerate(build_pair())]
    data = _data(768, 3, dev, seed=22)
    twin = _chain_run(te, dev, build_pair, lambda m, x: m(x), False, vals, data, recipe)
    got = _chain_run(te, dev, build_pair, lambda m, x: m(x), True, vals, data, recipe)
    assert twin[0]["bwd"]["scale"][0].item() != 1.0, f"{chain}: the twin's backward scale did not move"
    for step, (a, b) in enumerate(zip(got, twin)):
        at = f"{chain} / frozen module 0 / step {step}"
        assert _bits_equal(a["y"], b["y"]), f"{at}: output"
        if step == 0:
            assert a["bwd"]["scale"][0].item() != 1.0, f"{at}: module 1's backward scale is still its initial 1.0 -- the backward update never ran"
        for key in ("amax_history", "scale", "scale_inv"):
            assert _bits_equal(a["bwd"][key], b["bwd"][key]), f"{at}: module 1 backward {key} differs from the all-trainable chain"
        for name in a["grads"]:
            assert _bits_equal(a["grads"][name], b["grads"][name]), f"{at}: module 1 gradient of {name}"


# ---- model level: a tiny TELlamaForCausalLM under the freeze patterns of a fine-tune ----
VOCAB = 1024
SCENARIOS = ["default", "mxfp8"]   # delayed scaling (HYBRID attention region, E4M3 MLP region, outer lm_head recipe) and MXFP8
FREEZE = ["embedding", "embedding_layer0", "all_but_norms_and_biases", "query_weights"]


def _frozen(pattern, name) -> bool:
    if pattern is None:
        return False
    emb = name in ("model.embed_tokens.weight", "lm_head.weight")   # tied: one Parameter under two names
    if pattern == "embedding":
        return emb
    if pattern == "embedding_layer0":
        return emb or name.startswith("model.layers.0.")
    if pattern == "all_but_norms_and_biases":
        return not (name.endswith("bias") or name.endswith("layer_norm_weight") or name == "model.norm.weight")
    assert pattern == "query_weights"
    return name.endswith("query_weight")


def _tiny_model(dev, scenario, pattern):
    """2 layers, hidden 512, 4 heads over 1 KV head of 128, ffn 768, through train.prepare_model; biases and norm weights perturbed."""
    from llm_fp8_amd import llama, train
    from llm_fp8_amd.pytorch.fp8 import FP8GlobalStateManager
    FP8GlobalStateManager.reset()
    cfg = train.TrainingConfig(model_name="llama-3.2-1b", batch_size=B, max_seq_length=S, mixed_precision="fp8", fp8_scenario=scenario,
                               use_te=True, num_hidden_layers=2, vocab_size=VOCAB, learning_rate=1e-3, num_warmup_steps=0)
    config = llama.llama_config(cfg.model_name, hidden_size=H, intermediate_size=FFN, num_hidden_layers=2, num_attention_heads=4,
                                num_key_value_heads=1, head_dim=128, vocab_size=VOCAB)
    torch.manual_seed(0)
    prev = torch.get_default_dtype()
    torch.set_default_dtype(torch.bfloat16)
    try:
        with torch.device(dev):
            model = llama.TELlamaForCausalLM(config, scenario)
    finally:
        torch.set_default_dtype(prev)
    model.to(dev)
    model.config.use_cache = False
    g = torch.Generator().manual_seed(5)
    with torch.no_grad():
        for name, p in model.named_parameters():
            if name.endswith("bias"):
                p.copy_((0.02 * torch.randn(p.shape, generator=g)).to(p.dtype))
            elif name.endswith("layer_norm_weight") or name == "model.norm.weight":
                p.copy_((1.0 + 0.1 * torch.randn(p.shape, generator=g)).to(p.dtype))
    model = train.prepare_model(model, cfg)
    assert model.lm_head.weight is model.model.embed_tokens.weight
    for name, p in model.named_parameters():
        p.requires_grad_(not _frozen(pattern, name))
    model.train()
    gb = torch.Generator().manual_seed(6)
    ids = torch.randint(0, VOCAB, (B, S), generator=gb).to(dev)
    batch = {"input_ids": ids, "attention_mask": torch.ones_like(ids), "labels": ids.clone()}
    return model, cfg, batch


def _bwd_states(model):
    """Backward delayed-scaling state of every FP8 module that has one, by module name."""
    return {name: m._meta_bwd.state() for name, m in model.named_modules() if getattr(m, "_meta_bwd", None) is not None}


_STEP1: dict = {}   # scenario -> the all-trainable twin's first step (loss, gradients, backward states), computed once


def _first_step(dev, scenario, pattern):
    model, cfg, batch = _tiny_model(dev, scenario, pattern)
    loss = model(**batch).loss
    loss.backward()
    rec = {"loss": loss.detach().clone(), "grads": {n: (None if p.grad is None else p.grad.detach().clone()) for n, p in model.named_parameters()},
           "bwd": _bwd_states(model)}
    return rec


@pytest.mark.parametrize("pattern", FREEZE)
@pytest.mark.parametrize("scenario", SCENARIOS)
def test_model_first_step_gradients_equal_the_all_trainable_twin(te, dev, monkeypatch, scenario, pattern):
    monkeypatch.setenv("LLM_FP8_AMD_GROUPED_GEMM", "plan")
    if scenario not in _STEP1:
        _STEP1[scenario] = _first_step(dev, scenario, None)
    twin, got = _STEP1[scenario], _first_step(dev, scenario, pattern)
    at = f"tiny llama / {scenario} / frozen: {pattern}"
    n_frozen = sum(_frozen(pattern, name) for name in got["grads"])
    print(f"[frozen] {at}: loss {got['loss'].item():.6f} (twin {twin['loss'].item():.6f}), {len(got['grads'])} parameters, {n_frozen} frozen, "
          f"{len(got['bwd'])} modules with backward scaling state")
    # 22 = 2 layers x (norm + q, k, v weights; o-proj weight; norm + fc1 / fc2 weights and biases) + the tied embedding + the final norm
    assert torch.isfinite(got["loss"]) and 0 < n_frozen < len(got["grads"]) == 22
    assert _bits_equal(got["loss"], twin["loss"]), f"{at}: loss {got['loss'].item()} vs {twin['loss'].item()}"
    n_train = 0
    for name, g in got["grads"].items():
        if _frozen(pattern, name):
            assert g is None, f"{at}: frozen {name} got a gradient"
        else:
            n_train += 1
            assert g is not None, f"{at}: trainable {name} got no gradient"
            assert _bits_equal(g, twin["grads"][name]), f"{at}: gradient of {name} differs from the all-trainable twin"
    assert n_train > 0
    if scenario == "default" and pattern == "embedding_layer0":
        # layer 0 has no backward: the region's backward update must still run, behind layer 1's first Function
        checked = 0
        for name, st in got["bwd"].items():
            if not name.startswith("model.layers.1."):
                continue
            checked += 1
            assert st["scale"][0].item() != 1.0, f"{at}: backward scale of {name} is still its initial 1.0"
            for key in ("amax_history", "scale", "scale_inv"):
                assert _bits_equal(st[key], twin["bwd"][name][key]), f"{at}: backward {key} of {name} differs from the all-trainable twin"
        assert checked == 3, checked   # layernorm_qkv, proj, layernorm_mlp


def _three_steps(dev, scenario, pattern):
    from llm_fp8_amd import train
    model, cfg, batch = _tiny_model(dev, scenario, pattern)
    before = {n: p.detach().clone() for n, p in model.named_parameters()}
    opt, sched = train.create_optimizer(model, cfg)
    assert type(opt).__name__ == "ClippedAdamW"
    losses = [train.train_step(model, batch, opt, sched, cfg).detach().clone() for _ in range(3)]
    return losses, before, {n: p.detach().clone() for n, p in model.named_parameters()}


@pytest.mark.parametrize("pattern", FREEZE)
@pytest.mark.parametrize("scenario", SCENARIOS)
def test_model_three_steps_same_with_and_without_weight_sinks(te, dev, monkeypatch, scenario, pattern):
    """Three optimiser steps with the optimiser-filled FP8 weight copies (WeightSink / MXWeightSink) and with LLM_FP8_AMD_NO_OPT_WCAST=1:
    same losses, same parameters, bit for bit -- a sink with a part the optimiser never writes (a frozen query_weight beside trainable
    key / value weights) must never be read as fresh -- and the frozen parameters do not move."""
    monkeypatch.setenv("LLM_FP8_AMD_GROUPED_GEMM", "plan")
    monkeypatch.delenv("LLM_FP8_AMD_NO_OPT_WCAST", raising=False)
    losses_on, before, after_on = _three_steps(dev, scenario, pattern)
    monkeypatch.setenv("LLM_FP8_AMD_NO_OPT_WCAST", "1")
    losses_off, _, after_off = _three_steps(dev, scenario, pattern)
    at = f"tiny llama / {scenario} / frozen: {pattern}"
    print(f"[frozen] {at}: losses with sinks {[round(l.item(), 6) for l in losses_on]}, without {[round(l.item(), 6) for l in losses_off]}")
    assert len(losses_on) == len(losses_off) == 3 and len(before) == len(after_on) == len(after_off)
    assert losses_on[2].item() != losses_on[0].item(), f"{at}: the loss did not move in three steps"
    for step, (a, b) in enumerate(zip(losses_on, losses_off)):
        assert torch.isfinite(a), f"{at}: loss of step {step} is {a.item()}"
        assert _bits_equal(a, b), f"{at}: loss of step {step}: {a.item()} with sinks, {b.item()} without"
    moved = 0
    for name in before:
        assert _bits_equal(after_on[name], after_off[name]), f"{at}: {name} after 3 steps differs between sinks on and off"
        if _frozen(pattern, name):
            assert _bits_equal(after_on[name], before[name]), f"{at}: frozen {name} changed"
        else:
            moved += int(not _bits_equal(after_on[name], before[name]))
    n_train = sum(not _frozen(pattern, name) for name in before)
    still = sorted(n for n in before if not _frozen(pattern, n) and _bits_equal(after_on[n], before[n]))
    print(f"[frozen] {at}: {moved} of {n_train} trainable parameters moved, {len(before) - n_train} frozen ones did not; trainable but unmoved: {still}")
    # Adam's steps are ~lr = 1e-3 per element.  Weights and biases (|p| < 0.25: a bf16 ulp of at most 2^-10) must move; a norm weight
    # (1 +- 0.1 here: ulp 2^-7, three steps stay under half of it) rounds back to itself in bf16 and may stand still.
    is_norm = lambda n: n.endswith("layer_norm_weight") or n == "model.norm.weight"
    assert moved > 0 and all(is_norm(n) for n in still), f"{at}: trainable parameters that did not move: {[n for n in still if not is_norm(n)]}"
