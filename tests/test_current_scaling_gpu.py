"""GPU: Float8CurrentScaling -- the amax passes (exact against the oracle's amax; the fused modes against the amax the existing cast
kernels publish), the scale kernel (bitwise against TE's compute_scale_from_amax restated in numpy below), the quantised bytes, a
Linear against the oracle at its FIRST call (where delayed scaling is blind), exact power-of-two covariance, the fused modules
against their unfused routes, and a training step of scenario `current`."""
import numpy as np
import pytest
import torch

from oracle import fp8_oracle as O
from tests.util import assert_gemm_close, bf16_bits, bits_to_bf16, u8

pytestmark = pytest.mark.gpu

FP8_MAX = {O.E4M3: 448.0, O.E5M2: 57344.0}
BF16_MIN_SUBNORMAL = float(np.array([1], dtype=np.uint32).view(np.float32)[0] * np.float32(2.0 ** 16))  # bits 0x0001 = 2^-133


def scale_rule(amax, fp8_max, eps=0.0, pow2=False):
    """TE's compute_scale_from_amax in float32: (amax, scale, scale_inv)."""
    amax, eps, one = np.float32(amax), np.float32(eps), np.float32(1.0)
    a = eps if amax < eps else amax
    with np.errstate(over="ignore", divide="ignore", invalid="ignore"):
        if a == 0 or np.isinf(a):
            s = one
        else:
            s = np.float32(fp8_max) / a
            if np.isinf(s):
                s = np.float32(O.FLT_MAX)
            if np.isnan(s):
                s = one
        if pow2:
            s = (np.array([s], dtype=np.float32).view(np.uint32) & np.uint32(0xFF800000)).view(np.float32)[0]
        return amax, np.float32(s), np.float32(one / np.float32(s))


def _bits32(v):
    return np.asarray(v, dtype=np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def ops(dev):
    from llm_fp8_amd import _lib
    from llm_fp8_amd.pytorch import ops as _ops
    assert _lib.load().mi_device_supported() == 1, "not a gfx950 device"
    return _ops


# ------------------------------------------------------------------------------------------------------------ 1. plain amax
def _two_tiles_per_wave_shape(ops):
    """Ragged both ways, and every wave of the default grid (ops.amax_grid: two workgroups of four waves per CU) walks at least
    two 64 x 64 tiles: 5 column tiles (the last 8 wide), enough row tiles (the last 8 high)."""
    waves = 4 * ops.amax_grid(1 << 20, 1 << 12)  # the grid of a tensor large enough to reach the cap
    tiles_r = -(-(2 * waves + 1) // 5)
    return tiles_r * 64 - 56, 4 * 64 + 8


_BASE = {}


def _base(shape, dev):
    """Random bf16 [R, C] with |x| < 64, once per shape: (bits on the host, tensor on the device)."""
    if shape not in _BASE:
        g = torch.Generator().manual_seed(shape[0] * 31 + shape[1])
        x = (torch.randn(shape, generator=g) * 3).clamp_(-60, 60).to(torch.bfloat16)
        _BASE[shape] = (bf16_bits(x), x.to(dev))
    return _BASE[shape]


def _amax_of(ops, x, n):
    part = torch.full((n,), -7.0, dtype=torch.float32, device=x.device)  # sentinel: every entry must be overwritten
    ops.amax_bf16(x, part)
    p = part.cpu().numpy()
    assert (p != np.float32(-7.0)).all() and (p >= 0).all(), "an entry of the partial buffer was not written"
    return p


@pytest.mark.parametrize("shape", [(8, 8), (136, 72), (72, 136), "two-tiles"])
def test_plain_amax_is_exact(ops, dev, shape):
    if shape == "two-tiles":
        shape = _two_tiles_per_wave_shape(ops)
        assert -(-shape[0] // 64) * -(-shape[1] // 64) >= 2 * 4 * ops.amax_grid(*shape) and shape[0] % 64 and shape[1] % 64
    R, C = shape
    bits0, x0 = _base(shape, dev)
    peak = np.uint16(0x447A)  # 1000.0
    last_tile = ((R - 1) // 64 * 64, (C - 1) // 64 * 64)
    for pos in ((0, 0), (0, C - 1), (R - 1, 0), (R - 1, C - 1), last_tile):
        bits = bits0.copy()
        bits[pos] = peak | (0x8000 if pos[0] else 0)  # (negative in the lower corners: the amax is of |x|)
        x = x0.clone()
        x[pos] = -1000.0 if pos[0] else 1000.0
        want = O.amax_f32(O.bf16_bits_to_f32(bits))
        assert want == np.float32(1000.0)
        for n in (1, 7, ops.amax_grid(R, C)):
            p = _amax_of(ops, x, n)
            assert _bits32(p.max()) == _bits32(want), (pos, n, p.max())
    # without a planted peak: the base tensor's own amax, wherever it is
    assert _bits32(_amax_of(ops, x0, ops.amax_grid(R, C)).max()) == _bits32(O.amax_f32(O.bf16_bits_to_f32(bits0)))


@pytest.mark.parametrize("shape", [(8, 8), (136, 72)])
def test_plain_amax_nan_inf_and_zero(ops, dev, shape):
    R, C = shape
    bits0, x0 = _base(shape, dev)
    for n in (1, 7, ops.amax_grid(R, C)):
        x = x0.clone()
        x[R // 2, C - 1] = float("nan")            # one NaN is ignored
        bits = bits0.copy()
        bits[R // 2, C - 1] = 0x7FC0
        assert _bits32(_amax_of(ops, x, n).max()) == _bits32(O.amax_f32(O.bf16_bits_to_f32(bits)))
        x[R - 1, 0] = float("-inf")                # an Inf gives Inf (the NaN is still there)
        assert _amax_of(ops, x, n).max() == np.inf
        p = _amax_of(ops, torch.zeros_like(x0), n)
        assert (p == 0).all()
        sub_bits = np.zeros(shape, dtype=np.uint16)
        sub_bits[0, 0] = 0x0001                      # the smallest bf16 subnormal is not flushed
        sub = bits_to_bf16(sub_bits, dev)
        assert _bits32(_amax_of(ops, sub, n).max()) == _bits32(np.float32(BF16_MIN_SUBNORMAL))


# ------------------------------------------------------------------------------------------------------------ 2. fused modes
def _zero(dev):
    return torch.zeros(1, dtype=torch.float32, device=dev)


def _one(dev):
    return torch.ones(1, dtype=torch.float32, device=dev)


def _max_partial(ops, fn, *args, n):
    part = torch.full((n,), -7.0, dtype=torch.float32, device=args[0].device)
    fn(*args, part)
    p = part.cpu().numpy()
    assert (p >= 0).all(), "an entry of the partial buffer was not written"
    return p.max()


@pytest.mark.parametrize("shape", [(8, 512), (136, 1024)])
def test_norm_amax_equals_what_norm_cast_publishes(ops, dev, shape):
    R, C = shape
    g = torch.Generator().manual_seed(R + C)
    x = (torch.randn(shape, generator=g) * torch.exp(torch.randn(R, 1, generator=g))).to(torch.bfloat16).to(dev)
    gamma = (1 + 0.2 * torch.randn(C, generator=g)).to(torch.bfloat16).to(dev)
    rstd = ops.rmsnorm_stats(x, 1e-5)
    amax = _zero(dev)
    ops.norm_cast(x, rstd, gamma, _one(dev), amax, O.E4M3)   # the parent's kernel at scale 1 into a zeroed slot: the yardstick
    want = amax.cpu().numpy()[0]
    assert want > 0
    for n in (1, 7, ops.amax_grid(R, C)):
        assert _bits32(_max_partial(ops, ops.amax_norm, x, rstd, gamma, n=n)) == _bits32(want), n


@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("shape", [(8, 8), (136, 72)])
def test_swiglu_and_dswiglu_amax_equal_what_the_cast_kernels_publish(ops, dev, shape, with_bias):
    R, F = shape
    g = torch.Generator().manual_seed(R * 3 + F + int(with_bias))
    h = (torch.randn(R, 2 * F, generator=g) * 2).to(torch.bfloat16).to(dev)
    dact = (torch.randn(R, F, generator=g) / 8).to(torch.bfloat16).to(dev)
    bias = (torch.randn(2 * F, generator=g) / 2).to(torch.bfloat16).to(dev) if with_bias else None
    a_f, a_b = _zero(dev), _zero(dev)
    ops.swiglu_cast(h, _one(dev), a_f, O.E4M3, bias=bias)
    ops.dswiglu_cast(h, dact, _one(dev), a_b, O.E5M2, bias=bias)
    want_f, want_b = a_f.cpu().numpy()[0], a_b.cpu().numpy()[0]
    assert want_f > 0 and want_b > 0
    for n in (1, 7, ops.amax_grid(R, F, 32)):
        assert _bits32(_max_partial(ops, ops.amax_swiglu, h, bias, n=n)) == _bits32(want_f), n
        assert _bits32(_max_partial(ops, ops.amax_dswiglu, h, bias, dact, n=n)) == _bits32(want_b), n


# ------------------------------------------------------------------------------------------------------------ 3. scale rule
@pytest.mark.parametrize("fp8_max", [448.0, 57344.0])
def test_scale_rule_bitwise(ops, dev, fp8_max):
    rng = np.random.default_rng(int(fp8_max))
    rand = np.exp(rng.uniform(np.log(1e-30), np.log(1e30), size=24)).astype(np.float32)
    cases = [(a, 0.0, False) for a in rand] + [(0.0, 0.0, False), (np.inf, 0.0, False), (BF16_MIN_SUBNORMAL, 0.0, False),
                                                 (3e-5, 1e-3, False), (0.0, 1e-3, False), (7.0, 1e-3, False)]
    cases += [(a, 0.0, True) for a in rand[:8]] + [(3e-5, 1e-3, True), (BF16_MIN_SUBNORMAL, 0.0, True)]
    for amax, eps, pow2 in cases:
        host = np.zeros(7, dtype=np.float32)
        host[3] = np.float32(amax)                 # the maximum over the partials, wherever it sits
        host[5] = np.float32(amax) / np.float32(2) if np.isfinite(amax) else np.float32(1.0)
        part = torch.from_numpy(host).to(dev)
        got = ops.current_scale(part, fp8_max, eps, pow2).cpu().numpy()
        want = scale_rule(amax, fp8_max, eps, pow2)
        assert (_bits32(got) == _bits32(np.array(want))).all(), (amax, eps, pow2, got, want)
        if pow2:
            unrounded = scale_rule(amax, fp8_max, eps, False)[1]
            assert got[1] <= unrounded and (_bits32(got[1]) & 0x7FFFFF) == 0 and got[1] * 2 > unrounded
    assert scale_rule(BF16_MIN_SUBNORMAL, fp8_max)[1] == np.float32(O.FLT_MAX)
    assert scale_rule(3e-5, fp8_max, 1e-3)[1] == np.float32(fp8_max) / np.float32(1e-3)


# ------------------------------------------------------------------------------------------------------------ 4. bytes
@pytest.mark.parametrize("fmt", [O.E4M3, O.E5M2])
@pytest.mark.parametrize("shape", [(136, 72), (256, 512)])
def test_quantised_bytes_and_carried_scale_inverse(dev, shape, fmt):
    from llm_fp8_amd.common.recipe import Float8CurrentScaling
    from llm_fp8_amd.pytorch.module import _CurrentQ
    g = torch.Generator().manual_seed(shape[0] + fmt)
    x = (torch.randn(shape, generator=g) * 0.37).to(torch.bfloat16)
    bits = bf16_bits(x)
    _, s_ref, si_ref = scale_rule(O.amax_f32(O.bf16_bits_to_f32(bits)), FP8_MAX[fmt])
    want, _ = O.quantize_delayed(bits, s_ref, fmt)
    q = _CurrentQ(Float8CurrentScaling(), fmt, fmt)
    row, col = q.quantize(x.to(dev), 0, True)
    grow, gcol, cs = q.quantize_grad(x.to(dev), 0, True, True)
    assert cs is None
    for (y, si), (yT, siT) in ((row, col), (grow, gcol)):
        np.testing.assert_array_equal(u8(y), want)
        np.testing.assert_array_equal(u8(yT), want.T)
        assert _bits32(si.cpu().numpy()[0]) == _bits32(si_ref) == _bits32(siT.cpu().numpy()[0])


# ------------------------------------------------------------------------------------------------------------ 5. Linear
def _linear_case(factor, seed=5):
    g = torch.Generator().manual_seed(seed)
    w = (torch.randn(512, 256, generator=g) * 0.05).to(torch.bfloat16)
    x = (torch.randn(256, 256, generator=g) * factor).to(torch.bfloat16)
    dy = (torch.randn(256, 512, generator=g) / 32 * factor).to(torch.bfloat16)
    return x, w, dy


def _run_linear(te, dev, recipe, x, w, dy):
    from llm_fp8_amd.pytorch.fp8 import FP8GlobalStateManager
    FP8GlobalStateManager.reset()
    lin = te.Linear(256, 512, bias=False, params_dtype=torch.bfloat16, device=dev)  # fresh: no warm-up, no history
    with torch.no_grad():
        lin.weight.copy_(w)
    xd = x.to(dev).requires_grad_(True)
    with te.fp8_autocast(enabled=True, fp8_recipe=recipe):
        y = lin(xd)
    y.backward(dy.to(dev))
    torch.cuda.synchronize()
    FP8GlobalStateManager.reset()
    return y.detach(), xd.grad.detach(), lin.weight.grad.detach()


def _oracle_linear(x, w, dy):
    """gemm_fp8_tn of the oracle-quantised operands under the numpy scale rule: E4M3 forward, E5M2 gradients."""
    q = {}
    for name, t, fmt in (("x", x, O.E4M3), ("w", w, O.E4M3), ("g", dy, O.E5M2)):
        bits = bf16_bits(t)
        _, s, si = scale_rule(O.amax_f32(O.bf16_bits_to_f32(bits)), FP8_MAX[fmt])
        q[name] = (O.quantize_delayed(bits, s, fmt)[0], si)
    (x8, xi), (w8, wi), (g8, gi) = q["x"], q["w"], q["g"]
    f = O.bf16_bits_to_f32
    y = f(O.gemm_fp8_tn(x8, w8, O.E4M3, O.E4M3, xi, wi))
    dx = f(O.gemm_fp8_tn(g8, np.ascontiguousarray(w8.T), O.E5M2, O.E4M3, gi, wi))
    dw = f(O.gemm_fp8_tn(np.ascontiguousarray(g8.T), np.ascontiguousarray(x8.T), O.E5M2, O.E4M3, gi, xi))
    return y, dx, dw


def _close(got, ref):
    for name, a, b in zip(("y", "dx", "dw"), got, ref):
        assert_gemm_close(a.float().cpu().numpy(), b, name)


@pytest.mark.parametrize("log2_factor", [0, -12, 12])
def test_linear_against_the_oracle_at_the_first_call(dev, log2_factor):
    import llm_fp8_amd.pytorch as te
    from llm_fp8_amd.common.recipe import DelayedScaling, Float8CurrentScaling
    x, w, dy = _linear_case(2.0 ** log2_factor)
    ref = _oracle_linear(x, w, dy)
    _close(_run_linear(te, dev, Float8CurrentScaling(), x, w, dy), ref)
    if log2_factor == -12:
        # what the test is able to see: a fresh delayed-scaling module quantises with scale 1 and loses these inputs
        with pytest.raises(AssertionError):
            _close(_run_linear(te, dev, DelayedScaling(), x, w, dy), ref)


# ------------------------------------------------------------------------------------------------------------ 6. covariance
def test_exact_power_of_two_covariance(dev):
    import llm_fp8_amd.pytorch as te
    from llm_fp8_amd.common.recipe import Float8CurrentScaling
    x, w, dy = _linear_case(1.0, seed=9)
    x5, dy7 = x * 32, dy * 2.0 ** -7
    # nothing under- or overflows: the factors are exact on the inputs, on the scales of the numpy rule and on the outputs
    assert torch.equal(x5 / 32, x) and torch.equal(dy7 * 128, dy)
    for t, t2, k, fmt in ((x, x5, 32.0, O.E4M3), (dy, dy7, 2.0 ** -7, O.E5M2)):
        a, a2 = (O.amax_f32(O.bf16_bits_to_f32(bf16_bits(u))) for u in (t, t2))
        (_, s, si), (_, s2, si2) = scale_rule(a, FP8_MAX[fmt]), scale_rule(a2, FP8_MAX[fmt])
        assert a2 == np.float32(k) * a and s2 * np.float32(k) == s and si2 == si * np.float32(k)
        assert np.isfinite([s, s2, si, si2]).all() and min(s, s2, si, si2) > 2.0 ** -100
    r = Float8CurrentScaling()
    y, dx, dw = _run_linear(te, dev, r, x, w, dy)
    y5, dx5, dw5 = _run_linear(te, dev, r, x5, w, dy)
    y7, dx7, dw7 = _run_linear(te, dev, r, x, w, dy7)
    for t in (y, dx, dw):
        assert torch.isfinite(t).all() and t.float().abs().max() < 2.0 ** 100
        nz = t.float().abs()
        assert nz[nz > 0].min() > 2.0 ** -100
    assert torch.equal(y5, y * 32) and torch.equal(dw5, dw * 32)
    assert torch.equal(dx5, dx)                                  # dx does not depend on x
    assert torch.equal(y7, y)
    assert torch.equal(dx7, dx * 2.0 ** -7) and torch.equal(dw7, dw * 2.0 ** -7)


# ------------------------------------------------------------------------------------------------------------ 7. modules
# fused / unfused RMS-error ratio, the largest over the outputs and gradients of both modules as measured on an MI355X (the
# LayerNormMLP's layer_norm_weight gradient; every other quantity is within 0.998 .. 1.007), and the bound: that plus 25 %
MODULE_RATIO_MEASURED = 1.0101
MODULE_RATIO_BOUND = MODULE_RATIO_MEASURED * 1.25


def _rms(a, b):
    return float((a.double() - b.double()).pow(2).mean().sqrt())


def _module_runs(te, dev, kind, fused, grouped, monkeypatch):
    from llm_fp8_amd.common.recipe import Float8CurrentScaling
    from llm_fp8_amd.pytorch.fp8 import FP8GlobalStateManager
    FP8GlobalStateManager.reset()
    if grouped:
        monkeypatch.delenv("LLM_FP8_AMD_NO_GROUPED_GEMM", raising=False)
    else:
        monkeypatch.setenv("LLM_FP8_AMD_NO_GROUPED_GEMM", "1")
    torch.manual_seed(17)
    g = torch.Generator().manual_seed(23)
    if kind == "lnl":
        mod = te.LayerNormLinear(512, 768, normalization="RMSNorm", bias=False, params_dtype=torch.bfloat16, device=dev)
        mod.fused_norm = fused
        n_out = 768
    else:
        mod = te.LayerNormMLP(512, 1024, normalization="RMSNorm", activation="swiglu", bias=True, params_dtype=torch.bfloat16, device=dev)
        mod.fused_norm = mod.fused_swiglu = fused
        n_out = 512
        with torch.no_grad():
            mod.fc1_bias.copy_((torch.randn(2048, generator=g) * 0.1).to(torch.bfloat16))
            mod.fc2_bias.copy_((torch.randn(512, generator=g) * 0.1).to(torch.bfloat16))
    with torch.no_grad():
        mod.layer_norm_weight.copy_((1 + 0.1 * torch.randn(512, generator=g)).to(torch.bfloat16))
    x = (torch.randn(256, 512, generator=g) * torch.exp(0.5 * torch.randn(256, 1, generator=g))).to(torch.bfloat16).to(dev)
    dy = (torch.randn(256, n_out, generator=g) / 16).to(torch.bfloat16).to(dev)
    xd = x.clone().requires_grad_(True)
    with te.fp8_autocast(enabled=True, fp8_recipe=Float8CurrentScaling()):
        y = mod(xd)
    y.backward(dy)
    torch.cuda.synchronize()
    out = {"y": y.detach(), "dx": xd.grad.detach()}
    out.update({n: p.grad.detach() for n, p in mod.named_parameters()})
    # fp64 evaluation of the bf16 module (FP8 disabled)
    ref_mod = mod.to(torch.float64)
    for p in ref_mod.parameters():
        p.grad = None
    x64 = x.double().requires_grad_(True)
    with te.fp8_autocast(enabled=False):
        y64 = ref_mod(x64)
    y64.backward(dy.double())
    ref = {"y": y64.detach(), "dx": x64.grad.detach()}
    ref.update({n: p.grad.detach() for n, p in ref_mod.named_parameters()})
    FP8GlobalStateManager.reset()
    return out, ref


@pytest.mark.parametrize("kind", ["lnl", "mlp"])
def test_fused_modules_against_their_unfused_routes(dev, kind, monkeypatch):
    """LayerNormLinear (RMSNorm, 512 -> 768) and LayerNormMLP (512 -> 1024, swiglu, bias) on 256 tokens under the recipe: the fused
    route (norm -> cast and SwiGLU -> cast in one kernel each, amax from the recomputing pass) against the route with both fusions
    off, which quantises a bf16-rounded intermediate.  Both are compared with an fp64 evaluation of the module with FP8 disabled:
    the fused route's RMS error in the output and in every gradient may exceed the unfused route's by at most the margin.
    Measured ratio fused / unfused: LayerNormLinear y 0.9984, dx 1.0000, dgamma 1.0000, dW 1.0001; LayerNormMLP y 0.9981, dx 1.0045,
    dgamma 1.0101, dW1 1.0007, db1 1.0061, dW2 0.9995, db2 1.0000.  Margin = the largest, 1.0101; bound = that + 25 % = 1.2626.
    The same runs under LLM_FP8_AMD_NO_GROUPED_GEMM=1 give the same bits."""
    import llm_fp8_amd.pytorch as te
    fused, ref = _module_runs(te, dev, kind, True, True, monkeypatch)
    unfused, ref_u = _module_runs(te, dev, kind, False, True, monkeypatch)
    assert sorted(fused) == sorted(unfused) == sorted(ref)
    worst = 0.0
    for name in sorted(fused):
        assert torch.equal(ref[name], ref_u[name]), name            # the yardstick does not depend on the route
        ef, eu = _rms(fused[name], ref[name]), _rms(unfused[name], ref[name])
        scale = float(ref[name].pow(2).mean().sqrt())
        print(f"{kind} {name}: rms error fused {ef:.4e} unfused {eu:.4e} (rms of the value {scale:.4e}) ratio {ef / eu:.4f}")
        assert eu > 0 and eu < 0.1 * scale and ef < 0.1 * scale, name  # both routes are FP8-accurate at all
        worst = max(worst, ef / eu)
    print(f"{kind}: largest fused / unfused ratio {worst:.4f}")
    assert worst <= MODULE_RATIO_BOUND, (worst, MODULE_RATIO_BOUND)
    for is_fused, want in ((True, fused), (False, unfused)):
        again, _ = _module_runs(te, dev, kind, is_fused, False, monkeypatch)
        for name in want:
            assert torch.equal(again[name], want[name]), (name, is_fused)


# ------------------------------------------------------------------------------------------------------------ 8. training step
def _tiny_cfg(train, scenario, ga=1):
    return train.TrainingConfig(model_name="llama-3.2-3b", batch_size=2, max_seq_length=128, mixed_precision="fp8",
                                fp8_scenario=scenario, use_te=True, sharding_mode="none", num_hidden_layers=2, vocab_size=512,
                                learning_rate=1e-3, num_warmup_steps=0, gradient_accumulation_steps=ga)


def test_training_step_end_to_end(dev, monkeypatch):
    """TELlamaForCausalLM, 2 layers, hidden 512, 4 heads of 128, 2 KV heads, FFN 1024, vocab 512, batch 2 x 128, ClippedAdamW, scenario
    `current`: three steps on one repeated batch stay finite and the third loss is below the first; the step-0 loss deviates from
    the bf16 loss of the same weights (FP8 disabled) by at most twice what scenario `mxfp8` does.  Measured on an MI355X: bf16
    6.370163, current 6.371914 (|deviation| 1.750e-03), mxfp8 6.368985 (1.179e-03); losses 6.3719, 5.5698, 4.9050 and, accumulated
    over two micro-batches, 6.3724, 5.5667, 4.9032.  With gradient_accumulation_steps = 2 the weights are quantised once per window:
    27 calls of _CurrentQ.quantize_weights in three steps either way (9 GEMM sites)."""
    import llm_fp8_amd.pytorch as te
    from llm_fp8_amd import llama, train
    from llm_fp8_amd.optim import ClippedAdamW
    from llm_fp8_amd.pytorch import module as M
    from llm_fp8_amd.pytorch.fp8 import FP8GlobalStateManager as G
    device = torch.device(dev)
    orig_cfg = llama.llama_config
    monkeypatch.setattr(llama, "llama_config", lambda name, **kw: orig_cfg(name, **{**dict(
        hidden_size=512, intermediate_size=1024, num_attention_heads=4, num_key_value_heads=2, head_dim=128), **kw}))
    calls = {"n": 0}
    real_qw = M._CurrentQ.quantize_weights

    def counted(self, *a, **k):
        calls["n"] += 1
        return real_qw(self, *a, **k)

    monkeypatch.setattr(M._CurrentQ, "quantize_weights", counted)
    gen = torch.Generator(device=device).manual_seed(12)
    batch = train.synthetic_batch(_tiny_cfg(train, "current"), 512, device, gen)
    half = [{k: v[i:i + 1] for k, v in batch.items()} for i in range(2)]
    state = {}

    def build(scenario, ga=1):
        G.reset()
        cfg = _tiny_cfg(train, scenario, ga)
        torch.manual_seed(31)
        model = train.prepare_model(train.create_model(cfg, device), cfg)
        if state:
            model.load_state_dict(state["sd"], strict=False)
        else:
            state["sd"] = {k: v.clone() for k, v in model.state_dict().items() if not k.endswith("_extra_state")}
        model.train()
        return model, cfg

    def steps(scenario, ga=1, n=3):
        model, cfg = build(scenario, ga)
        opt, sched = train.create_optimizer(model, cfg)
        assert isinstance(opt, ClippedAdamW)
        calls["n"] = 0
        losses = [train.train_step(model, batch if ga == 1 else half, opt, sched, cfg).item() for _ in range(n)]
        return losses, calls["n"]

    try:
        cur, n_cur = steps("current")
        mx, _ = steps("mxfp8", n=1)
        # bf16 loss of the same weights: every fp8_autocast region of the model disabled
        real_autocast = te.fp8_autocast
        monkeypatch.setattr(te, "fp8_autocast", lambda enabled=True, **kw: real_autocast(enabled=False, **kw))
        model, cfg = build("current")
        with torch.no_grad():
            ref = model(**batch).loss.item()
        monkeypatch.setattr(te, "fp8_autocast", real_autocast)
        cur2, n_cur2 = steps("current", ga=2)
    finally:
        G.reset()
    dev_cur, dev_mx = abs(cur[0] - ref), abs(mx[0] - ref)
    print(f"losses current {cur}; accumulated {cur2}; step-0 loss bf16 {ref:.6f} current {cur[0]:.6f} mxfp8 {mx[0]:.6f}: "
          f"|current - bf16| = {dev_cur:.3e}, |mxfp8 - bf16| = {dev_mx:.3e}; quantize_weights calls {n_cur} / {n_cur2}")
    assert all(np.isfinite(cur)) and cur[2] < cur[0], cur
    assert all(np.isfinite(cur2)) and cur2[2] < cur2[0], cur2
    sites = 2 * 4 + 1                              # per layer q|k|v, proj, fc1, fc2; the lm_head
    assert n_cur == 3 * sites, n_cur               # every forward quantises every weight operand once
    assert n_cur2 == 3 * sites, n_cur2             # two micro-batches per step, ONE quantisation per window
    assert dev_cur <= 2 * dev_mx, (dev_cur, dev_mx)
