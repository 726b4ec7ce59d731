"""GPU: optim.ClippedAdamW(state_dtype=torch.float32) -- fp32 master weights and fp32 moments behind the fused AdamW + FP8 cast
pass (mi_adamw_f32_multi).  A: one step against float64 from the device's own fp32 state; B: the FP8 / MXFP8 sinks are bitwise a
fresh quantisation of the updated bf16 weight, and the tile walk is the flat walk's arithmetic; C: a 64-step trajectory at the
default learning rate keeps the displacement that bf16 state rounds away; D: save / resume; E: an external write re-seeds the
master; F: misaligned fp32 moments take the flat walk; G: the training harness end to end; H: sharded = replicated.

The float64 step is `_f64_step` below (the formula of oracle.fp8_oracle.adamw_step_f64 on fp32 state).  Bound of A, E and F on
master / exp_avg / exp_avg_sq: 8 x 2^-24 x the magnitudes of the terms the kernel adds (its fp32 evaluation error, the slack
tests/test_kernel_widths_gpu.py::_adam_ref uses) + half an fp32 ulp of the result (the rounding of the stored value)."""
import copy
import json
import math
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHUNK = 65536
FLAT_SIZES = [(CHUNK,), (CHUNK + 8,), (2 * CHUNK + 13,), (7,), (1,), (200, 333), (129, 131)]  # 2-D: no multiples of the 128 tile
G0 = dict(lr=1e-2, weight_decay=0.1, betas=(0.9, 0.999), eps=1e-8)   # the g0 / g1 groups of test_kernel_widths_gpu._adam_case
G1 = dict(lr=1e-5, weight_decay=0.0, betas=(0.8, 0.95), eps=1e-6)
F32 = torch.float32


@pytest.fixture()
def te_reset(dev):
    from llm_fp8_amd.pytorch.fp8 import FP8GlobalStateManager
    FP8GlobalStateManager.reset()
    yield
    FP8GlobalStateManager.reset()


def _np(t):
    return t.detach().double().cpu().numpy().ravel()


def _f32_ulp(x):
    """Spacing of fp32 at |x| (24 significand bits), float64; the subnormal spacing below 2^-126."""
    return 2.0 ** (np.floor(np.log2(np.maximum(np.abs(x), 2.0 ** -126))) - 23)


def _f64_step(w, g, m, v, step, hp, coef):
    """float64 AdamW step from fp32 state: [(value, slack)] for master, exp_avg, exp_avg_sq.  Hyper-parameters as the kernel
    receives them (fp32); `coef` is the clip coefficient the kernel multiplies the gradient with."""
    lr, eps, wd, b1, b2 = (float(np.float32(x)) for x in (hp["lr"], hp["eps"], hp["weight_decay"], *hp["betas"]))
    g = g * coef
    m1 = b1 * m + (1.0 - b1) * g
    v1 = b2 * v + (1.0 - b2) * g * g
    upd = lr / (1.0 - b1 ** step) * m1 / (np.sqrt(v1) / np.sqrt(1.0 - b2 ** step) + eps)
    w1 = w * (1.0 - lr * wd) - upd
    u = 8 * 2.0 ** -24
    return [(w1, u * (np.abs(w) + np.abs(upd))), (m1, u * (np.abs(m) + np.abs(g))), (v1, u * np.abs(v1))]


def _before(opt, p, start=None):
    """(weight the step must start from, gradient, exp_avg, exp_avg_sq) as float64, read from the device before the step."""
    st = opt.state.get(p) or {}
    w = _np(start) if start is not None else _np(st["master"]) if "master" in st else _np(p)
    zeros = np.zeros(p.numel())
    return w, _np(p.grad), _np(st["exp_avg"]) if "exp_avg" in st else zeros, _np(st["exp_avg_sq"]) if "exp_avg_sq" in st else zeros


def _clip_coef(opt, befores, mgn):
    """The coefficient the kernels received: torch's fp32 arithmetic on the device's fp32 norm, itself checked against float64."""
    if mgn is None:
        return 1.0
    norm = math.sqrt(sum(float((b[1] ** 2).sum()) for b in befores))
    got = np.float32(opt.last_grad_norm.item())
    assert abs(float(got) - norm) <= 1e-6 * norm, f"grad norm {got} vs float64 {norm}"
    return float(min(np.float32(1.0), np.float32(mgn) / (got + np.float32(1e-6))))


def _check_state(opt, p, before, step, hp, coef, what):
    """Bound A on master / exp_avg / exp_avg_sq, all three fp32, and bits(p) == RNE_bf16(master) for every element.  (The bound on
    the master, 8 x 2^-24 x (|w| + |update|), has no room for the fp32 error of exp_avg = b1 m + (1 - b1) g where the two terms
    cancel: fp32 evaluation of the update misses it by up to 10 x on a few elements in 100 k.  The fp32-state kernels evaluate the
    step in fp64 and round once into the fp32 state.)"""
    st = opt.state[p]
    assert st["step"] == step, what
    worst = {}
    for name, (ref, slack) in zip(("master", "exp_avg", "exp_avg_sq"), _f64_step(*before, step, hp, coef)):
        t = st[name]
        assert t.dtype == F32 and t.shape == p.shape, f"{what}: {name} is {t.dtype} {tuple(t.shape)}"
        err, tol = np.abs(_np(t) - ref), slack + 0.5 * _f32_ulp(ref)
        worst[name] = float((err / tol).max())
        assert (err <= tol).all(), f"{what} {name}: {(err > tol).sum()} of {err.size} beyond the bound, worst {worst[name]:.3g} x"
    assert torch.equal(p.detach().view(torch.int16), st["master"].to(torch.bfloat16).view(torch.int16)), f"{what}: p != RNE_bf16(master)"
    return worst


# ------------------------------------------------------------------------------------------------ A: one step against float64
@pytest.mark.parametrize("case", ["clip", "tiny"])
def test_fp32_state_one_step_vs_float64(dev, case):
    """Steps 1, 2 and (after setting state["step"] = 999) 1000, each from the device's own fp32 state read back before it.  Tensors
    straddle the 64 Ki-element chunk (full, + an 8-element tail, two chunks + 13, 7 and 1 elements, two 2-D shapes); two groups
    with different hyper-parameters; the second tensor gets a zero gradient.  clip: norm ~ 600, clipped; tiny: gradients ~ 1e-12 on
    parameters ~ 1e-6, eps dominates the denominator."""
    from llm_fp8_amd.optim import ClippedAdamW
    assert ClippedAdamW.CHUNK == CHUNK
    gscale, pscale = {"clip": (1.0, 1.0), "tiny": (1e-12, 1e-6)}[case]
    gen = torch.Generator().manual_seed({"clip": 1, "tiny": 4}[case])
    groups = [(FLAT_SIZES[:4], G0), (FLAT_SIZES[4:], G1)]
    params = [[torch.nn.Parameter((torch.randn(s, generator=gen) * pscale).to(torch.bfloat16).to(dev)) for s in sizes] for sizes, _ in groups]
    opt = ClippedAdamW([dict(params=ps, **hp) for ps, (_, hp) in zip(params, groups)], max_grad_norm=1.0, state_dtype=F32)
    worst = {}
    for step in (1, 2, 1000):
        if step == 1000:
            for ps in params:
                for p in ps:
                    opt.state[p]["step"] = 999
        for gi, ps in enumerate(params):
            for k, p in enumerate(ps):
                gr = torch.randn(p.shape, generator=gen) * gscale
                if gi == 0 and k == 1:
                    gr.zero_()
                p.grad = gr.to(torch.bfloat16).to(dev)
        before = [[_before(opt, p) for p in ps] for ps in params]
        opt.step()
        torch.cuda.synchronize()
        coef = _clip_coef(opt, [b for bs in before for b in bs], 1.0)
        assert (coef < 1.0) == (case == "clip")
        for gi, (ps, (_, hp)) in enumerate(zip(params, groups)):
            for k, p in enumerate(ps):
                w = _check_state(opt, p, before[gi][k], step, hp, coef, f"{case} step {step} group {gi} {tuple(p.shape)}")
                worst = {n: max(worst.get(n, 0.0), x) for n, x in w.items()}
    print(f"fp32 state {case}: worst error / bound {worst}")


# ------------------------------------------------------------------------------------------------ B: sinks
def _sink_linear(dev, seed, K, N, recipe):
    """An FP8 Linear after one training forward / backward: its [N, K] weight has an optimiser sink."""
    import llm_fp8_amd.pytorch as te
    torch.manual_seed(seed)
    lin = te.Linear(K, N, bias=False, params_dtype=torch.bfloat16, device=dev)
    x = torch.randn(64, K, device=dev, dtype=torch.bfloat16)
    with te.fp8_autocast(enabled=True, fp8_recipe=recipe):
        y = lin(x)
    y.float().pow(2).mean().backward()
    return lin


def _delayed():
    from llm_fp8_amd.common.recipe import DelayedScaling, Format
    return DelayedScaling(fp8_format=Format.HYBRID, amax_history_len=4, amax_compute_algo="max")


def _sink_run(dev, monkeypatch, mx, nowcast):
    """One fp32-state step on a sink weight (+ a flat tensor with an 8-element tail under delayed scaling).  `nowcast`: the same
    tensors with LLM_FP8_AMD_NO_OPT_WCAST=1, i.e. down the flat walk."""
    from llm_fp8_amd.common.recipe import MXFP8BlockScaling
    from llm_fp8_amd.optim import ClippedAdamW
    from llm_fp8_amd.pytorch.fp8 import FP8GlobalStateManager
    FP8GlobalStateManager.reset()
    if nowcast:
        monkeypatch.setenv("LLM_FP8_AMD_NO_OPT_WCAST", "1")
    else:
        monkeypatch.delenv("LLM_FP8_AMD_NO_OPT_WCAST", raising=False)
    # 200 x 144 and 224 x 160: 128 x 128 tiles ragged both ways (MXFP8 needs multiples of 32)
    lin = _sink_linear(dev, 160, 160, 224, MXFP8BlockScaling()) if mx else _sink_linear(dev, 144, 144, 200, _delayed())
    w = lin.weight
    tensors = [w]
    if not mx:
        g = torch.Generator().manual_seed(9)
        flat = torch.nn.Parameter(torch.randn(CHUNK + 8, generator=g).to(torch.bfloat16).to(dev))
        flat.grad = torch.randn(CHUNK + 8, generator=g).to(torch.bfloat16).to(dev)
        tensors.append(flat)
    opt = ClippedAdamW(tensors, max_grad_norm=1.0, state_dtype=F32, **G0)
    sink_of = opt._mx_sink_of if mx else opt._sink_of
    assert (sink_of(w) is None) == nowcast, "the weight is not on the walk this run is about"
    sink = None if nowcast else sink_of(w)[0]
    amax0 = sink.amax.clone() if sink is not None and not mx else None
    opt.step()
    torch.cuda.synchronize()
    state = [tuple(opt.state[p][k].clone() for k in ("master", "exp_avg", "exp_avg_sq")) + (p.detach().clone(),) for p in tensors]
    return w, sink, amax0, state, opt


@pytest.mark.parametrize("mx", [False, True], ids=["per_tensor", "mxfp8"])
def test_fp32_state_sinks_are_bitwise_a_fresh_quantisation(te_reset, dev, monkeypatch, mx):
    from llm_fp8_amd.pytorch import ops
    w, sink, amax0, tiled, opt = _sink_run(dev, monkeypatch, mx, nowcast=False)
    assert all(pl["chunks_cast"] is not None for pl in opt._plans.values())
    assert torch.equal(w.detach().view(torch.int16), opt.state[w]["master"].to(torch.bfloat16).view(torch.int16))
    assert not torch.equal(opt.state[w]["master"], w.detach().float()), "the master carries nothing below bf16"
    wq = w.detach().clone()
    if mx:
        for got, ref, name in zip((sink.w8, sink.sc, sink.wt8, sink.sct), ops.mxfp8_quantize(wq, ops.E4M3), ("w8", "sc", "wt8", "sct")):
            assert torch.equal(got, ref), f"MXFP8 sink {name} is not mi_mxfp8_quantize of the updated weight"
    else:
        y, yT = ops.cast_amax(wq, sink.scale, amax0, ops.E4M3)  # amax0: the slot as it was before the step, maxed as the step did
        assert torch.equal(sink.w8, y) and torch.equal(sink.w8t, yT), "FP8 sink is not mi_cast_amax of the updated weight"
        assert amax0.item() > 0 and torch.equal(sink.amax.view(torch.int32), amax0.view(torch.int32)), (sink.amax, amax0)
    assert sink.fresh()
    # the flat walk (LLM_FP8_AMD_NO_OPT_WCAST=1) and the tile walk are one arithmetic
    _, _, _, flat, _ = _sink_run(dev, monkeypatch, mx, nowcast=True)
    for a, b in zip(tiled, flat):
        for u, v, name in zip(a, b, ("master", "exp_avg", "exp_avg_sq", "p")):
            assert u.dtype == v.dtype and torch.equal(u, v), f"{name} {tuple(u.shape)}: the tile walk differs from the flat walk"


# ------------------------------------------------------------------------------------------------ C: trajectory
def test_fp32_state_keeps_the_displacement_at_the_default_learning_rate(dev):
    """64 steps at TrainingConfig's learning rate on weights of magnitude 0.02: the update (~ lr = 1.41e-5) is far below half a
    bf16 ulp of the weight (6e-5), so bf16 state drops most of them; the fp32 master must carry them.  Figure: relative L2 error
    of the displacement p_64 - p_0 against float64 AdamW on the same bf16 gradients.  fp32 arithmetic gives 1.1e-4 and bf16 state
    0.92 (emulated on the CPU); the bound 1e-2 sits ~90 x from each.  (Measured: 9.9e-6 with fp32 state, whose step is
    evaluated in fp64, and 0.92 with bf16 state.)"""
    from llm_fp8_amd.optim import ClippedAdamW
    n, steps = CHUNK + 8, 64
    hp = dict(lr=1.41e-5, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2)
    gen = torch.Generator().manual_seed(1234)
    p0 = (0.02 * torch.randn(n, generator=gen)).to(torch.bfloat16)
    grads = [(1e-3 * torch.randn(n, generator=gen) + 5e-4).to(torch.bfloat16) for _ in range(steps)]
    w = p0.double().numpy().copy()
    m, v = np.zeros(n), np.zeros(n)
    for t, g in enumerate(grads, 1):
        (w, _), (m, _), (v, _) = _f64_step(w, g.double().numpy(), m, v, t, hp, 1.0)[:3]
    ref = w - p0.double().numpy()
    fig = {}
    for name, dt in (("fp32", F32), ("bf16", torch.bfloat16)):
        p = torch.nn.Parameter(p0.clone().to(dev))
        opt = ClippedAdamW([p], max_grad_norm=None, state_dtype=dt, **hp)
        for g in grads:
            p.grad = g.to(dev)
            opt.step()
        torch.cuda.synchronize()
        end = _np(opt.state[p]["master"]) if dt == F32 else _np(p)
        fig[name] = float(np.linalg.norm((end - p0.double().numpy()) - ref) / np.linalg.norm(ref))
        moved = float((_np(p) != p0.double().numpy()).mean())
        print(f"displacement error after {steps} steps, {name} state: {fig[name]:.3e} (bf16 weights that moved: {100 * moved:.1f} %)")
    assert fig["fp32"] <= 1e-2, fig


# ------------------------------------------------------------------------------------------------ D: save and resume
def test_fp32_state_save_and_resume_is_bitwise(dev):
    from llm_fp8_amd.optim import ClippedAdamW
    gen = torch.Generator().manual_seed(77)
    sizes = [(CHUNK + 8,), (129, 131)]
    init = [torch.randn(s, generator=gen).to(torch.bfloat16) for s in sizes]
    grads = [[torch.randn(s, generator=gen).to(torch.bfloat16).to(dev) for s in sizes] for _ in range(5)]
    make = lambda src: [torch.nn.Parameter(t.detach().clone().to(dev)) for t in src]

    def run(opt, params, steps):
        for gs in steps:
            for p, g in zip(params, gs):
                p.grad = g.clone()
            opt.step()

    pa = make(init)
    oa = ClippedAdamW(pa, max_grad_norm=1.0, state_dtype=F32, **G0)
    run(oa, pa, grads)
    pb = make(init)
    ob = ClippedAdamW(pb, max_grad_norm=1.0, state_dtype=F32, **G0)
    run(ob, pb, grads[:3])
    pc = make(pb)
    oc = ClippedAdamW(pc, max_grad_norm=1.0, state_dtype=F32, **G0)
    oc.load_state_dict(copy.deepcopy(ob.state_dict()))
    for p in pc:
        assert all(oc.state[p][k].dtype == F32 for k in ("master", "exp_avg", "exp_avg_sq"))
    run(oc, pc, grads[3:])
    torch.cuda.synchronize()
    for a, c in zip(pa, pc):
        assert oa.state[a]["step"] == oc.state[c]["step"] == 5
        assert torch.equal(a.detach().view(torch.int16), c.detach().view(torch.int16)), "p differs after the resume"
        for k in ("master", "exp_avg", "exp_avg_sq"):
            assert torch.equal(oa.state[a][k], oc.state[c][k]), f"{k} differs after the resume"
        assert not torch.equal(oa.state[a]["master"], a.detach().float())  # there was a residue to lose


# ------------------------------------------------------------------------------------------------ E: external write
def test_fp32_state_external_write_reseeds_the_master(dev):
    """Somebody writes the parameter between two steps (a checkpoint load, a copy from another model): the next step starts from
    the value written, not from the stale master, and keeps the moments.  The write goes through `Tensor.copy_` under no_grad,
    which moves `p._version` -- the signal the optimiser (like the FP8 weight sinks) goes by; a `.data` write does not move it
    (llama.replace_params says why the package never writes that way) and is, by design, not seen."""
    from llm_fp8_amd.optim import ClippedAdamW
    gen = torch.Generator().manual_seed(5)
    p = torch.nn.Parameter(torch.randn(CHUNK + 8, generator=gen).to(torch.bfloat16).to(dev))
    other = (3.0 * torch.randn(CHUNK + 8, generator=gen)).to(torch.bfloat16).to(dev)
    opt = ClippedAdamW([p], max_grad_norm=1.0, state_dtype=F32, **G0)
    p.grad = torch.randn(CHUNK + 8, generator=gen).to(torch.bfloat16).to(dev)
    opt.step()
    stale = opt.state[p]["master"].clone()
    with torch.no_grad():
        p.copy_(other)
    p.grad = torch.randn(CHUNK + 8, generator=gen).to(torch.bfloat16).to(dev)
    before = _before(opt, p, start=other)
    opt.step()
    torch.cuda.synchronize()
    coef = _clip_coef(opt, [before], 1.0)
    print("external write:", _check_state(opt, p, before, 2, G0, coef, "step after an external write"))
    assert (opt.state[p]["master"] - stale).abs().mean().item() > 1.0  # moved to `other` (|other - stale| ~ 3), not a step from `stale`


def test_fp32_state_loaded_before_the_weights_reseeds_the_master(dev):
    """The load order the class docstring warns of: the optimiser state first, the model's weights second.  The second load writes
    the parameters (`copy_`, as load_state_dict does), `p._version` moves past the `master_version` the first load recorded, and
    the next step re-seeds every master from the bf16 parameter -- the SAME bf16 values here, so only the fp32 residue is lost.
    That step must be a valid step from master == float(p), with the loaded moments and step count kept."""
    from llm_fp8_amd.optim import ClippedAdamW
    gen = torch.Generator().manual_seed(78)
    sizes = [(CHUNK + 8,), (129, 131)]
    grads = [[torch.randn(s, generator=gen).to(torch.bfloat16).to(dev) for s in sizes] for _ in range(4)]
    pa = [torch.nn.Parameter(torch.randn(s, generator=gen).to(torch.bfloat16).to(dev)) for s in sizes]
    oa = ClippedAdamW(pa, max_grad_norm=1.0, state_dtype=F32, **G0)
    for gs in grads[:3]:
        for p, g in zip(pa, gs):
            p.grad = g.clone()
        oa.step()
    saved = copy.deepcopy(oa.state_dict())
    pb = [torch.nn.Parameter(torch.zeros_like(p)) for p in pa]       # a fresh model: not the weights the state goes with
    ob = ClippedAdamW(pb, max_grad_norm=1.0, state_dtype=F32, **G0)
    ob.load_state_dict(saved)                                        # the optimiser first ...
    with torch.no_grad():
        for p, a in zip(pb, pa):
            p.copy_(a.detach())                                      # ... the weights second
    for p, a, g in zip(pb, pa, grads[3]):
        st, sa = ob.state[p], oa.state[a]
        assert st["master_version"] != p._version, "the second load did not move the version: nothing to pin"
        assert torch.equal(st["master"], sa["master"]) and not torch.equal(sa["master"], a.detach().float())  # a residue to lose
        p.grad = g.clone()
    before = [_before(ob, p, start=p.detach()) for p in pb]          # the step must start from float(p), not from the loaded master
    for p, a, b in zip(pb, pa, before):
        assert np.array_equal(b[2], _np(oa.state[a]["exp_avg"])) and np.array_equal(b[3], _np(oa.state[a]["exp_avg_sq"]))
    ob.step()
    torch.cuda.synchronize()
    coef = _clip_coef(ob, before, 1.0)
    for p, b in zip(pb, before):
        print("optimiser loaded before the weights:", _check_state(ob, p, b, 4, G0, coef, f"step after the late weight load {tuple(p.shape)}"))
        assert ob.state[p]["master_version"] == p._version


# ------------------------------------------------------------------------------------------------ F: misaligned state
def test_fp32_state_sink_weight_with_misaligned_moments(te_reset, dev):
    """fp32 moments that are views at a 4-byte offset (a loaded optimiser state can be): the tile walk issues 16-byte accesses on
    them unconditionally, so the weight takes the flat walk (element-wise), meets the float64 bound, and its sink -- not
    rewritten -- is not declared current."""
    from llm_fp8_amd.optim import ClippedAdamW
    w = _sink_linear(dev, 200, 144, 200, _delayed()).weight
    opt = ClippedAdamW([w], max_grad_norm=1.0, state_dtype=F32, **G0)
    assert opt._sink_of(w) is not None
    n = w.numel()
    bufs = [torch.zeros(n + 4, dtype=F32, device=dev) for _ in range(2)]
    opt.state[w]["step"] = 0
    opt.state[w]["exp_avg"] = bufs[0][1:1 + n].view(w.shape)
    opt.state[w]["exp_avg_sq"] = bufs[1][1:1 + n].view(w.shape)
    assert all(opt.state[w][k].data_ptr() % 16 == 4 for k in ("exp_avg", "exp_avg_sq"))
    assert opt._sink_of(w) is None, "misaligned moments must keep the weight off the tile walk"
    sink = w._mi_fp8_sink[0]
    g = torch.Generator(device=dev).manual_seed(5)
    for step in (1, 2):
        w.grad = torch.randn(w.shape, device=dev, generator=g).to(torch.bfloat16)
        before = _before(opt, w)
        opt.step()
        torch.cuda.synchronize()
        coef = _clip_coef(opt, [before], 1.0)
        print(f"misaligned moments step {step}:", _check_state(opt, w, before, step, G0, coef, f"misaligned moments step {step}"))
        assert not sink.fresh()
    assert bufs[0][0].item() == 0.0 and bufs[0][-3:].abs().sum().item() == 0.0  # nothing written around the views


# ------------------------------------------------------------------------------------------------ G: end to end
@pytest.mark.parametrize("scenario", ["default", "mxfp8"])
def test_fp32_state_training_harness_end_to_end(te_reset, dev, scenario, monkeypatch):
    from llm_fp8_amd import train
    from llm_fp8_amd.optim import ClippedAdamW
    from llm_fp8_amd.pytorch import ops
    monkeypatch.delenv("LLM_FP8_AMD_OPT_STATE", raising=False)
    monkeypatch.delenv("LLM_FP8_AMD_NO_OPT_WCAST", raising=False)
    cfg = train.TrainingConfig(model_name="llama-3.2-1b", num_hidden_layers=2, vocab_size=4096, batch_size=4, max_seq_length=128,
                               use_te=True, optimizer_state="fp32", fp8_scenario=scenario)
    torch.manual_seed(3)
    model = train.prepare_model(train.create_model(cfg, dev), cfg)
    opt, sched = train.create_optimizer(model, cfg)
    assert type(opt) is ClippedAdamW and opt.state_dtype == F32
    model.train()
    gen = torch.Generator(device=dev).manual_seed(8)
    losses = [train.train_step(model, train.synthetic_batch(cfg, 4096, dev, gen), opt, sched, cfg).item() for _ in range(3)]
    torch.cuda.synchronize()
    assert all(math.isfinite(l) for l in losses), losses
    trainable = [p for p in model.parameters() if p.requires_grad]
    assert len(opt.state) == len(trainable) > 0
    for p in trainable:  # norm weights and the embedding included
        st = opt.state[p]
        assert st["step"] == 3
        assert all(t.dtype == F32 for t in st.values() if torch.is_tensor(t)) and {"master", "exp_avg", "exp_avg_sq"} <= set(st)
        assert torch.equal(p.detach().view(torch.int16), st["master"].to(torch.bfloat16).view(torch.int16)), tuple(p.shape)
    checked = 0
    for mod in model.modules():
        for k, sink in list(getattr(mod, "_wcache", {}).items()):
            if not (isinstance(k, tuple) and k[0] in ("sink", "mxsink")):
                continue
            assert sink.fresh(), f"{type(mod).__name__} {k}: the optimiser left this sink stale"
            for w, lo, n in sink.parts:
                x = w.detach().contiguous()
                if k[0] == "sink":
                    y, yT = ops.cast_amax(x, sink.scale, None, ops.E4M3)
                    assert torch.equal(sink.w8[lo:lo + n], y) and torch.equal(sink.w8t[:, lo:lo + n], yT), (type(mod).__name__, k)
                else:
                    y, sc, wt, sct = ops.mxfp8_quantize(x, ops.E4M3)
                    assert (torch.equal(sink.w8[lo:lo + n], y) and torch.equal(sink.sc[:, lo:lo + n], sc)
                            and torch.equal(sink.wt8[:, lo:lo + n], wt) and torch.equal(sink.sct[lo // 32:(lo + n) // 32], sct)), (type(mod).__name__, k)
            checked += 1
    assert checked >= 2 * 4, checked  # per layer: q|k|v, proj, fc1, fc2


# ------------------------------------------------------------------------------------------------ H: sharded = replicated
def _free_port() -> str:
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as sk:
        sk.bind(("127.0.0.1", 0))
        return str(sk.getsockname()[1])


def test_fp32_state_sharded_fp8_dp_matches_the_replicated_run(dev):
    """tests/fsdp_fp8_worker.py unchanged, driven into fp32 state by LLM_FP8_AMD_OPT_STATE, launched as
    test_distributed_gpu.py::test_sharded_fp8_dp_matches_the_replicated_run launches (2, "default"): two ranks sharing the GPU over
    gloo.  The state is per parameter and per row shard, the clip norm is float64 and the gathers read the bf16 shard = RNE(master),
    so the sharded run must still be the replicated one bit for bit."""
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", LLM_FP8_AMD_DIST_BACKEND="gloo", LLM_FP8_AMD_SHARE_DEVICE="1",
               LLM_FP8_AMD_OPT_STATE="fp32")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", _free_port(), os.path.join(ROOT, "tests", "fsdp_fp8_worker.py"), "default"]
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    outs = sorted((json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")), key=lambda o: o["rank"])
    assert len(outs) == 2, r.stdout[-2000:]
    for o in outs:
        assert o["losses_equal"] and o["eval_equal"] and o["weights_equal"] and o["arenas_equal"], o
        assert o["sinks"]["checked"] > 0 and o["sinks"]["mismatch"] == 0 and o["sinks"]["train_stale"] == 0, o
        # fp32 moments on the shards: 2 x 4 bytes per owned element (the bf16 layout has 2 x 2), so the mode did reach the workers
        assert o["mem"]["shard_moment_bytes"] * 2 == 4 * o["mem"]["sharded_logical_bytes"], o["mem"]
