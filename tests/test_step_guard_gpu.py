"""GPU: the step guard (include/mi_fp8.h "THE STEP GUARD"; optim.ClippedAdamW(skip_nonfinite=...)).  Every comparison is bitwise.
1: every AdamW entry point called directly with a non-finite *grad_scale -- the state is untouched (0xA5 margins intact), the FP8
copies of a sink tensor are what mi_cast_amax / mi_mxfp8_quantize make of the unchanged weight; 2: one ClippedAdamW per state
mode, three steps with the second poisoned -- it leaves no trace but the step count; 3: a Linear and a LayerNormMLP trained four
steps with the second poisoned -- the sinks stay current and right, and the run equals the one whose forward casts itself.

Shapes of tests/test_optim_paths_gpu.py: a flat tensor of 6149 elements (vector body + element tail), the same one element off a
16-byte boundary (element-wise walk), a 200 x 144 weight with a per-tensor sink (2 x 2 ragged tiles), a 160 x 96 weight with an
MXFP8 sink (2 x 1 tiles)."""
import math

import pytest
import torch

from tests.test_optim_fp32_state_gpu import CHUNK, G0, _delayed
from tests.test_optim_paths_gpu import MODES, N_FLAT, SEED, _guarded, _header_table, _margins_intact, _mx, _tensor, te_reset  # noqa: F401

pytestmark = pytest.mark.gpu
BF16, F32 = torch.bfloat16, torch.float32
NONFINITE = {"nan": float("nan"), "+inf": float("inf"), "-inf": float("-inf")}
SHAPES = {"tiled": (200, 144), "mxw": (160, 96), "flat": (N_FLAT,), "off": (N_FLAT,)}
# entry point -> (name, state mode, sink kind or None, tensors, chunk list)
TILED, MXW, FLAT = ("tiled", "flat", "off"), ("mxw", "flat", "off"), ("flat", "off")
CH_TILED, CH_MXW, CH_FLAT = [[0, 0], [0, 1], [0, 2], [0, 3], [1, 0], [2, 0]], [[0, 0], [0, 1], [1, 0], [2, 0]], [[0, 0], [1, 0]]
ENTRIES = {
    "bf16_multi": ("mi_adamw_bf16_multi", "bf16", None, FLAT, CH_FLAT),
    "cast": ("mi_adamw_cast_bf16_multi", "bf16", None, TILED, CH_TILED),
    "mxcast": ("mi_adamw_mxcast_bf16_multi", "bf16", None, MXW, CH_MXW),
    "f32_fp8": ("mi_adamw_f32_multi", "fp32", 0, TILED, CH_TILED),
    "f32_mx": ("mi_adamw_f32_multi", "fp32", 1, MXW, CH_MXW),
    "sr_fp8": ("mi_adamw_sr_bf16_multi", "bf16_sr", 0, TILED, CH_TILED),
    "sr_mx": ("mi_adamw_sr_bf16_multi", "bf16_sr", 1, MXW, CH_MXW),
}


def _raw(t):
    return t.detach().contiguous().view(torch.uint8)


def _a5(shape, dtype, dev):
    """A tensor of 0xA5 bytes inside a 0xA5 allocation: an output nobody has written yet."""
    t, buf = _guarded(torch.zeros(shape, dtype=dtype, device=dev))
    t.view(torch.uint8).fill_(0xA5)
    return t, buf


def _poisoned_grad(shape, gen, dev):
    """Finite values, one NaN and one Inf: 0 * Inf = NaN, so a kernel that multiplied by a zero coefficient would show."""
    g = torch.randn(shape, generator=gen).to(BF16).to(dev)
    g.view(-1)[3] = float("nan")
    g.view(-1)[g.numel() // 2 + 1] = float("inf")
    return g


def _state(name, mode, gen, dev):
    """One tensor's state in guarded allocations: dict what -> (tensor, allocation), the gradient, and the snapshot of the state."""
    shape = SHAPES[name]
    sdt = F32 if mode == "fp32" else BF16
    held = {"p": _guarded(torch.randn(shape, generator=gen).to(BF16).to(dev), 1 if name == "off" else 0),
            "exp_avg": _guarded((1e-2 * torch.randn(shape, generator=gen)).to(sdt).to(dev)),
            "exp_avg_sq": _guarded((1e-4 * torch.rand(shape, generator=gen)).to(sdt).to(dev))}
    if mode == "fp32":
        held["master"] = _guarded(held["p"][0].float() * (1.0 + 2.0 ** -12))
    assert held["p"][0].data_ptr() % 16 == (2 if name == "off" else 0)
    return held, _poisoned_grad(shape, gen, dev)


def _check_state_untouched(held, before, grad, grad_before, what):
    for k, (t, buf) in held.items():
        assert torch.equal(_raw(t), before[k]), f"{what} {k}: a skipped launch wrote it"
        _margins_intact(t, buf, f"{what} {k}")
    assert torch.equal(_raw(grad), grad_before), f"{what}: the gradient changed"


# ------------------------------------------------------------------------------------------------ 1: direct calls
@pytest.mark.parametrize("gs", list(NONFINITE))
@pytest.mark.parametrize("entry", list(ENTRIES))
def test_a_non_finite_grad_scale_skips_the_launch(dev, entry, gs):
    from llm_fp8_amd import _lib
    from llm_fp8_amd.pytorch import ops
    lib = _lib.load()
    name, mode, kind, names, refs = ENTRIES[entry]
    mx = names is MXW
    gen = torch.Generator().manual_seed(21)
    scale = torch.tensor([37.5], dtype=F32, device=dev)
    cols, tensors, sinks = [], [], {}
    for i, n in enumerate(names):
        held, grad = _state(n, mode, gen, dev)
        p = held["p"][0]
        col = dict(p=p.data_ptr(), g=grad.data_ptr(), m=held["exp_avg"][0].data_ptr(), v=held["exp_avg_sq"][0].data_ptr(), numel=p.numel(),
                   sink=None, master=held["master"][0].data_ptr() if mode == "fp32" else None, base=8 * i, key=40 + i)
        if n in ("tiled", "mxw"):
            N, K = SHAPES[n]
            if mx:   # 6 y_row  7 s_row  8 y_colT  9 s_colT  10 ldr  11 unused
                out = {"w8": _a5((N, K), torch.uint8, dev), "sc": _a5((K // 32, N), torch.uint8, dev),
                       "wt8": _a5((K, N), torch.uint8, dev), "sct": _a5((N // 32, K), torch.uint8, dev)}
                col["sink"] = [K, out["w8"][0].data_ptr(), out["sc"][0].data_ptr(), out["wt8"][0].data_ptr(), out["sct"][0].data_ptr(), N, 0]
            else:    # 6 y  7 yT  8 ld_y  9 ld_yT  10 scale  11 amax (a slot that no cast has deposited into yet: 0)
                out = {"w8": _a5((N, K), torch.uint8, dev), "w8t": _a5((K, N), torch.uint8, dev), "amax": _guarded(torch.zeros(1, dtype=F32, device=dev))}
                col["sink"] = [K, out["w8"][0].data_ptr(), out["w8t"][0].data_ptr(), K, N, scale.data_ptr(), out["amax"][0].data_ptr()]
            sinks[n] = out
        cols.append(col)
        tensors.append((n, held, {k: _raw(t).clone() for k, (t, _) in held.items()}, grad, _raw(grad).clone()))
    table = torch.tensor(_header_table(cols, mode), dtype=torch.int64).to(dev)
    chunks = torch.tensor(refs, dtype=torch.int32).to(dev)
    coef = torch.tensor([NONFINITE[gs]], dtype=F32, device=dev)
    tail = {"bf16": (), "fp32": (kind,), "bf16_sr": (kind, SEED)}[mode]
    rc = getattr(lib, name)(table.data_ptr(), len(cols), chunks.data_ptr(), len(refs), CHUNK, coef.data_ptr(), G0["lr"], *G0["betas"],
                            G0["eps"], G0["weight_decay"], 3, *tail, torch.cuda.current_stream().cuda_stream)
    _lib.check(rc, name)
    torch.cuda.synchronize()
    for n, held, before, grad, grad_before in tensors:
        _check_state_untouched(held, before, grad, grad_before, f"{entry} {gs} {n}")
    # the copies of the sink tensor: those of the forward's quantiser on the unchanged weight
    for n, out in sinks.items():
        w = tensors[names.index(n)][1]["p"][0]
        if mx:
            want = dict(zip(("w8", "sc", "wt8", "sct"), ops.mxfp8_quantize(w, ops.E4M3)))
        else:
            amax = torch.zeros(1, dtype=F32, device=dev)
            y, yT = ops.cast_amax(w, scale, amax, ops.E4M3)
            want = {"w8": y, "w8t": yT, "amax": amax}
            assert torch.equal(out["w8t"][0], out["w8"][0].t()), f"{entry} {gs}: w8t != w8.t()"
            assert amax.item() == w.float().abs().max().item() > 0.0
        for k, (t, buf) in out.items():
            assert torch.equal(_raw(t), _raw(want[k])), f"{entry} {gs} {n}: {k} is not the forward's quantisation of the stored weight"
            _margins_intact(t, buf, f"{entry} {gs} {n} sink {k}")


@pytest.mark.parametrize("gs", list(NONFINITE))
def test_a_non_finite_grad_scale_skips_the_single_tensor_call(dev, gs):
    from llm_fp8_amd import _lib
    lib = _lib.load()
    gen = torch.Generator().manual_seed(22)
    coef = torch.tensor([NONFINITE[gs]], dtype=F32, device=dev)
    for n in ("flat", "off"):
        held, grad = _state(n, "bf16", gen, dev)
        before, grad_before = {k: _raw(t).clone() for k, (t, _) in held.items()}, _raw(grad).clone()
        rc = lib.mi_adamw_bf16(held["p"][0].data_ptr(), grad.data_ptr(), held["exp_avg"][0].data_ptr(), held["exp_avg_sq"][0].data_ptr(),
                               N_FLAT, coef.data_ptr(), G0["lr"], *G0["betas"], G0["eps"], G0["weight_decay"], 3,
                               torch.cuda.current_stream().cuda_stream)
        _lib.check(rc, "mi_adamw_bf16")
        torch.cuda.synchronize()
        _check_state_untouched(held, before, grad, grad_before, f"mi_adamw_bf16 {gs} {n}")


# ------------------------------------------------------------------------------------------------ 2: ClippedAdamW
NAMES = ("tiled", "mxw", "flat", "off")


def _make(dev, mode, **kw):
    """The four tensors (the two weights come with their sinks, out of a Linear's first forward) under one ClippedAdamW."""
    from llm_fp8_amd.optim import ClippedAdamW
    gen = torch.Generator().manual_seed(5)
    params = [_tensor(dev, n, gen) for n in NAMES]
    for i, p in enumerate(params):
        p._mi_sr_key = (40 + i, 8 * i)
    return params, ClippedAdamW(params, max_grad_norm=1.0, **MODES[mode], **G0, **kw)


def _grads(dev, step):
    gen = torch.Generator().manual_seed(100 + step)
    return [(0.1 * torch.randn(SHAPES[n], generator=gen)).to(BF16).to(dev) for n in NAMES]


def _step(params, opt, step, poison=False):
    for p, g in zip(params, _grads(params[0].device, step)):
        p.grad = g
    if poison:
        params[0].grad[17, 5] = float("inf")
    opt.step()


def _snapshot(params, opt):
    """Every tensor the optimiser owns or writes, as raw bytes: parameter, moments, master, and the FP8 copies of the sinks."""
    out = {}
    for n, p in zip(NAMES, params):
        out[n, "p"] = _raw(p).clone()
        for k, t in opt.state[p].items():
            if torch.is_tensor(t):
                out[n, k] = _raw(t).clone()
        for attr, fields in (("_mi_fp8_sink", ("w8", "w8t")), ("_mi_mx_sink", ("w8", "sc", "wt8", "sct"))):
            if hasattr(p, attr):
                for f in fields:
                    out[n, attr, f] = _raw(getattr(getattr(p, attr)[0], f)).clone()
    return out


@pytest.mark.parametrize("mode", list(MODES))
def test_a_poisoned_step_leaves_no_trace_but_the_count(te_reset, dev, monkeypatch, mode):
    monkeypatch.delenv("LLM_FP8_AMD_NO_OPT_WCAST", raising=False)
    monkeypatch.delenv("MI_DEBUG_SINK", raising=False)
    params, opt = _make(dev, mode)
    assert opt._guard_active() and opt.last_step_skipped is None and opt.skipped_steps is None
    _step(params, opt, 1)
    assert opt.last_step_skipped.dtype == torch.bool and opt.last_step_skipped.shape == () and opt.last_step_skipped.is_cuda
    assert opt.skipped_steps.dtype == torch.int64 and opt.skipped_steps.is_cuda
    assert not opt.last_step_skipped.item() and opt.skipped_steps.item() == 0 and math.isfinite(opt.last_grad_norm.item())
    after1 = _snapshot(params, opt)
    versions = [p._version for p in params]
    _step(params, opt, 2, poison=True)
    after2 = _snapshot(params, opt)
    assert opt.last_step_skipped.item() is True and opt.skipped_steps.item() == 1
    assert not math.isfinite(opt.last_grad_norm.item())
    assert after1.keys() == after2.keys() and len(after1) >= 4 * 3 + 6
    for k in after1:
        assert torch.equal(after1[k], after2[k]), f"{mode}: the skipped step changed {k}"
    # the host cannot know: the step is counted, versions move, sinks are stamped current
    for p, v in zip(params, versions):
        assert opt.state[p]["step"] == 2 and p._version > v
        if mode == "fp32":
            assert opt.state[p]["master_version"] == p._version
    assert params[0]._mi_fp8_sink[0].fresh() and params[1]._mi_mx_sink[0].fresh()
    _step(params, opt, 3)
    assert not opt.last_step_skipped.item() and opt.skipped_steps.item() == 1
    after3 = _snapshot(params, opt)
    # the twin never ran step 2: its step count is advanced instead
    twins, topt = _make(dev, mode)
    _step(twins, topt, 1)
    for p in twins:
        topt.state[p]["step"] += 1
    _step(twins, topt, 3)
    want = _snapshot(twins, topt)
    assert want.keys() == after3.keys()
    for k in want:
        assert torch.equal(after3[k], want[k]), f"{mode}: {k} differs from the run without step 2"
        assert not torch.equal(after3[k], after1[k]) or k[-1] in ("sc", "sct"), f"{mode}: step 3 did not move {k}"
    assert "skipped_steps" not in repr(opt.state_dict().keys()) and set(opt.state_dict()) == {"state", "param_groups"}


@pytest.mark.parametrize("mode", list(MODES))
def test_without_the_guard_the_same_step_poisons_the_weights(te_reset, dev, monkeypatch, mode):
    """The parent's behaviour, asserted so that the test above shows what the guard prevents."""
    monkeypatch.delenv("LLM_FP8_AMD_NO_OPT_WCAST", raising=False)
    params, opt = _make(dev, mode, skip_nonfinite=False)
    assert not opt._guard_active()
    _step(params, opt, 1)
    _step(params, opt, 2, poison=True)
    assert opt.last_step_skipped is None and opt.skipped_steps is None and not math.isfinite(opt.last_grad_norm.item())
    assert torch.isnan(params[0].detach()[17, 5]).item() and torch.isnan(opt.state[params[0]]["exp_avg"][17, 5]).item()


def test_without_a_norm_the_guard_is_inactive(dev):
    from llm_fp8_amd.optim import ClippedAdamW
    p = torch.nn.Parameter(torch.ones(64, dtype=BF16, device=dev))
    opt = ClippedAdamW([p], max_grad_norm=None, skip_nonfinite=True, **G0)
    p.grad = torch.full((64,), 0.5, dtype=BF16, device=dev)
    opt.step()
    assert opt.last_step_skipped is None and opt.skipped_steps is None and opt.last_grad_norm is None


# ------------------------------------------------------------------------------------------------ 3: sinks through the modules
def _module_run(dev, which, recipe_name, steps=4):
    """`steps` training steps of one module under ClippedAdamW, the gradient of step 2 poisoned.  Returns the losses and, per forward
    after the first, how many sinks were checked."""
    import llm_fp8_amd.pytorch as te
    from llm_fp8_amd.optim import ClippedAdamW
    from llm_fp8_amd.pytorch import ops
    from llm_fp8_amd.pytorch.fp8 import FP8GlobalStateManager
    from llm_fp8_amd.pytorch.module import weight_sinks_enabled
    FP8GlobalStateManager.reset()
    torch.manual_seed(31)
    if which == "linear":
        mod = te.Linear(256, 512, bias=True, params_dtype=BF16, device=dev)
    else:
        mod = te.LayerNormMLP(256, 512, bias=True, normalization="RMSNorm", activation="swiglu", params_dtype=BF16, device=dev)
    recipe = _delayed() if recipe_name == "delayed" else _mx()
    opt = ClippedAdamW(list(mod.parameters()), lr=1e-2, max_grad_norm=1.0)
    xs = [torch.randn(64, 256, device=dev, dtype=BF16) for _ in range(steps)]
    losses, checked = [], []

    def check_sinks():
        n = 0
        for k, sink in list(getattr(mod, "_wcache", {}).items()):
            if not (isinstance(k, tuple) and k[0] in ("sink", "mxsink")):
                continue
            assert sink.fresh(), f"{which} {recipe_name} {k}: stale at a forward after the optimiser's step"
            for w, lo, rows in sink.parts:
                x = w.detach().contiguous()
                if k[0] == "sink":
                    y, yT = ops.cast_amax(x, sink.scale, None, ops.E4M3)
                    ok = torch.equal(sink.w8[lo:lo + rows], y) and torch.equal(sink.w8t[:, lo:lo + rows], yT)
                else:
                    y, sc, wt, sct = ops.mxfp8_quantize(x, ops.E4M3)
                    ok = (torch.equal(sink.w8[lo:lo + rows], y) and torch.equal(sink.sc[:, lo:lo + rows], sc)
                          and torch.equal(sink.wt8[:, lo:lo + rows], wt) and torch.equal(sink.sct[lo // 32:(lo + rows) // 32], sct))
                assert ok, f"{which} {recipe_name} {k}: the copies are not a forward quantisation of the weight as it is now"
            n += 1
        return n

    for step in range(1, steps + 1):
        if step > 1 and weight_sinks_enabled():
            checked.append(check_sinks())
        with te.fp8_autocast(enabled=True, fp8_recipe=recipe):
            y = mod(xs[step - 1])
        loss = y.float().pow(2).mean()
        loss.backward()
        if step == 2:
            w = mod.weight if which == "linear" else mod.fc2_weight
            w.grad[3, 7] = float("inf")
        opt.step()
        opt.zero_grad()
        losses.append(loss.detach().clone())
    assert opt.skipped_steps.item() == 1
    return [l.item() for l in losses], checked


@pytest.mark.parametrize("recipe_name", ["delayed", "mxfp8"])
@pytest.mark.parametrize("which", ["linear", "mlp"])
def test_sinks_stay_current_and_right_across_a_skipped_step(te_reset, dev, monkeypatch, which, recipe_name):
    monkeypatch.delenv("LLM_FP8_AMD_NO_OPT_WCAST", raising=False)
    monkeypatch.delenv("MI_DEBUG_SINK", raising=False)
    losses, checked = _module_run(dev, which, recipe_name)
    assert len(checked) == 3 and checked[0] >= (1 if which == "linear" else 2) and checked == checked[:1] * 3, checked
    assert all(math.isfinite(l) for l in losses), losses
    monkeypatch.setenv("LLM_FP8_AMD_NO_OPT_WCAST", "1")
    ref, none = _module_run(dev, which, recipe_name)
    assert none == []
    assert losses[2:] == ref[2:] and losses == ref, (losses, ref)
