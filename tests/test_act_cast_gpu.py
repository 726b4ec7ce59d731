"""GELU / GeGLU fused with the FP8 cast (mi_act_cast, mi_dact_cast, mi_amax_act, mi_amax_dact) against float64 numpy, and the
LayerNormMLP route through them.

Module tolerance (test_module_route): relative Frobenius error of the output and of every gradient against _reference, the float64
module on dequantised operands.  TOL holds, per case and tensor, what the unfused route (fused_swiglu=False: two FP8 Linears around
the torch activation) measured against that reference on MI355X over seeds 0-4 at tokens 128, hidden 512, ffn 256: (its largest
error, largest minus smallest over the seeds).  The fused route is allowed their sum.  It measured 0.007-0.026 where the unfused
route has 0.017-0.050 (it skips two bf16 roundings), and the same as the unfused route behind a torch LayerNorm; every figure is in
profiles/act_cast.txt."""
import numpy as np
import pytest
import torch

from oracle import fp8_oracle as O
from tests.util import u8

pytestmark = pytest.mark.gpu
TOL = {  # (act, current scaling, normalization, bias): {tensor: (unfused max, unfused spread)}
    ("gelu", False, "RMSNorm", True): {"out": (0.02474, 0.00161), "dx": (0.03617, 0.00346), "layer_norm_weight": (0.03733, 0.00721), "fc1_weight": (0.03977, 0.00297), "fc2_weight": (0.03269, 0.00162), "fc1_bias": (0.0102, 0.00121), "fc2_bias": (0.00178, 0.00024)},
    ("geglu", False, "RMSNorm", True): {"out": (0.02102, 0.00102), "dx": (0.04766, 0.00334), "layer_norm_weight": (0.04972, 0.00585), "fc1_weight": (0.05016, 0.00301), "fc2_weight": (0.04015, 0.00303), "fc1_bias": (0.01829, 0.0012), "fc2_bias": (0.00178, 0.00024)},
    ("gelu", True, "RMSNorm", True): {"out": (0.02383, 0.00256), "dx": (0.03096, 0.00254), "layer_norm_weight": (0.0316, 0.00508), "fc1_weight": (0.03435, 0.00351), "fc2_weight": (0.03179, 0.00411), "fc1_bias": (0.00877, 0.00193), "fc2_bias": (0.00178, 0.00024)},
    ("geglu", True, "RMSNorm", True): {"out": (0.02065, 0.00347), "dx": (0.04652, 0.00511), "layer_norm_weight": (0.04865, 0.00784), "fc1_weight": (0.04911, 0.00624), "fc2_weight": (0.03975, 0.00664), "fc1_bias": (0.01636, 0.00349), "fc2_bias": (0.00178, 0.00024)},
    ("geglu", False, "LayerNorm", False): {"out": (0.03944, 0.00078), "dx": (0.04858, 0.00413), "layer_norm_weight": (0.04848, 0.00444), "fc1_weight": (0.05131, 0.00431), "fc2_weight": (0.03936, 0.00075), "layer_norm_bias": (0.04872, 0.00282)},
}
SHAPES = [(8, 8), (136, 72), (256, 264)]  # smallest; short last 128-row block, F no multiple of 16; two column tiles, the last with 8 columns


def _gelu64(x):
    """(gelu_tanh(x), its derivative) in float64; s (1 - s) as s * (1 - s) is exactly 0 where s saturates."""
    with np.errstate(over="ignore"):
        s = 1.0 / (1.0 + np.exp(-2.0 * 0.7978845608 * (x + 0.044715 * x ** 3)))
    return x * s, s + x * s * (1.0 - s) * 2.0 * 0.7978845608 * (1.0 + 0.134145 * x * x)


def _act64(h, act, d=None):
    """act(h), or with `d` the gradient d(act)/dh contracted with d, in float64: h [R, F] (gelu) or [R, 2F] (geglu)."""
    g, u = (h, 1.0) if act == "gelu" else (h[:, :h.shape[1] // 2], h[:, h.shape[1] // 2:])
    a, da = _gelu64(g)
    if d is None:
        return a * u
    return d * da * u if act == "gelu" else np.concatenate([d * da * u, d * a], axis=1)


def _fp8_close(y, yT, v, scale, fmt):
    """The criterion of test_swiglu_cast_vs_oracle: no byte more than one code from the float64 reference, >= 99.5 % identical."""
    got, want = u8(y).astype(np.int16), O.fp8_encode_sat((v * scale).astype(np.float32), fmt).astype(np.int16)
    diff, same_sign = np.abs((got & 0x7F) - (want & 0x7F)), ((got ^ want) & 0x80) == 0
    assert ((diff <= 1) & same_sign | ((got & 0x7F) + (want & 0x7F) <= 1)).all() and (diff == 0).mean() >= 0.995
    np.testing.assert_array_equal(u8(yT), u8(y).T)
    assert np.isfinite(O.fp8_decode(u8(y), fmt)).all()


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("act", ["gelu", "geglu"])
def test_kernels_vs_float64(dev, act, with_bias, shape):
    from llm_fp8_amd.pytorch import ops
    R, F = shape
    W = F * ops.ACT_CODES[act]
    g = torch.Generator().manual_seed(R * 5 + F + W)
    h = (torch.randn(R, W, generator=g) * 2).to(torch.bfloat16)
    h[1::4] = ((torch.rand(R, W, generator=g) * 120 - 60).to(torch.bfloat16))[1::4]  # saturated branches of gelu'
    d = (torch.randn(R, F, generator=g) / 8).to(torch.bfloat16)
    bias = (torch.randn(W, generator=g) * 0.5).to(torch.bfloat16) if with_bias else None
    h64 = h.double().numpy() + (bias.double().numpy()[None, :] if with_bias else 0.0)
    hd, dd, bd = h.to(dev), d.to(dev), None if bias is None else bias.to(dev)
    one = lambda v: torch.tensor([v], dtype=torch.float32, device=dev)
    part = torch.empty(7, dtype=torch.float32, device=dev)
    # forward, E4M3
    v, amax = _act64(h64, act), torch.zeros(1, dtype=torch.float32, device=dev)
    y, yT = ops.act_cast(hd, act, one(16.0), amax, O.E4M3, bias=bd)
    _fp8_close(y, yT, v, 16.0, O.E4M3)
    ops.amax_act(hd, act, bd, part)
    assert part.max().item() == amax.item()
    np.testing.assert_allclose(amax.item(), np.abs(v).max(), rtol=1e-5)
    # backward, E5M2
    v, amax = _act64(h64, act, d.double().numpy()), torch.zeros(1, dtype=torch.float32, device=dev)
    y, yT, cs = ops.dact_cast(hd, dd, act, one(64.0), amax, O.E5M2, want_colsum=True, bias=bd)
    _fp8_close(y, yT, v, 64.0, O.E5M2)
    ops.amax_dact(hd, act, bd, dd, part)
    assert part.max().item() == amax.item()
    np.testing.assert_allclose(amax.item(), np.abs(v).max(), rtol=1e-5)
    assert cs.shape == ((R + 127) // 128, W) and torch.isfinite(cs).all()
    np.testing.assert_allclose(cs.sum(0).cpu().numpy(), v.sum(0), rtol=1e-4, atol=1e-4 * np.abs(v).max() * np.sqrt(R))


def _qdq(v, fmt, current):
    """v quantised to FP8 and back, in float64: scale 1 (delayed scaling's first step) or fp8_max / amax (current scaling)."""
    v32 = v.astype(np.float32)
    s = np.float32({O.E4M3: 448.0, O.E5M2: 57344.0}[fmt]) / np.abs(v32).max() if current else np.float32(1.0)
    return O.fp8_decode(O.fp8_encode_sat(v32 * s, fmt), fmt).astype(np.float64) / np.float64(s)


def _reference(mod, x, dy, current):
    """Output and gradients of `mod` in float64 on the dequantised operands of its six quantisations."""
    p = {k: v.detach().double().cpu() for k, v in mod.named_parameters()}
    x64 = x.detach().double().cpu().requires_grad_(True)
    lw, lb = p["layer_norm_weight"].requires_grad_(True), p.get("layer_norm_bias")
    if mod.normalization == "RMSNorm":
        xn = x64 * torch.rsqrt(x64.pow(2).mean(-1, keepdim=True) + mod.eps) * lw
    else:
        xn = torch.nn.functional.layer_norm(x64, x64.shape[-1:], lw, lb.requires_grad_(True), mod.eps)
    b1, b2 = (p[k].numpy() if k in p else 0.0 for k in ("fc1_bias", "fc2_bias"))
    x8, w1, w2 = _qdq(xn.detach().numpy(), O.E4M3, current), _qdq(p["fc1_weight"].numpy(), O.E4M3, current), _qdq(p["fc2_weight"].numpy(), O.E4M3, current)
    h = x8 @ w1.T + b1
    a8, dy64 = _qdq(_act64(h, mod.activation), O.E4M3, current), dy.double().cpu().numpy()
    dy8 = _qdq(dy64, O.E5M2, current)
    dh = _act64(h, mod.activation, dy8 @ w2)
    dh8 = _qdq(dh, O.E5M2, current)
    xn.backward(torch.from_numpy(dh8 @ w1))
    ref = {"out": a8 @ w2.T + b2, "dx": x64.grad.numpy(), "layer_norm_weight": lw.grad.numpy(), "fc1_weight": dh8.T @ x8,
           "fc2_weight": dy8.T @ a8, "fc1_bias": dh.sum(0), "fc2_bias": dy64.sum(0)}
    if lb is not None:
        ref["layer_norm_bias"] = lb.grad.numpy()
    return {k: v for k, v in ref.items() if k in ("out", "dx") or k in p}


def route_errors(dev, act, current, norm, bias, seed, fused):
    """({tensor: relative Frobenius error against _reference}, KernelTimer summary) of one forward + backward of LayerNormMLP."""
    import llm_fp8_amd.pytorch as te
    from llm_fp8_amd.common.recipe import DelayedScaling, Float8CurrentScaling, Format
    from llm_fp8_amd.pytorch.profiler import KernelTimer
    torch.manual_seed(seed)
    mod = te.LayerNormMLP(512, 256, normalization=norm, activation=act, bias=bias, params_dtype=torch.bfloat16, device=dev)
    mod.fused_swiglu = fused
    with torch.no_grad():
        for k, q in mod.named_parameters():
            if "bias" in k or k == "layer_norm_weight":
                q.add_(torch.randn_like(q) * 0.1)
    x = torch.randn(128, 512, device=dev, dtype=torch.bfloat16).requires_grad_(True)
    dy = (torch.randn(128, 512, device=dev) / 16).to(torch.bfloat16)
    recipe = Float8CurrentScaling(fp8_format=Format.HYBRID) if current else DelayedScaling(fp8_format=Format.HYBRID)
    with KernelTimer().install() as timer:
        with te.fp8_autocast(enabled=True, fp8_recipe=recipe):
            out = mod(x)
        out.backward(dy)
    torch.cuda.synchronize()
    got = {"out": out, "dx": x.grad, **{k: q.grad for k, q in mod.named_parameters()}}
    ref = _reference(mod, x, dy, current)
    err = {k: float(np.linalg.norm(got[k].detach().double().cpu().numpy() - r) / np.linalg.norm(r)) for k, r in ref.items()}
    return err, timer.summarize()


@pytest.mark.parametrize("act,current,norm,bias", sorted(TOL))
def test_module_route(dev, monkeypatch, act, current, norm, bias):
    monkeypatch.setattr(torch.nn.functional, "gelu", None)  # a torch GELU on the route is a TypeError
    err, kinds = route_errors(dev, act, current, norm, bias, seed=0, fused=True)
    print(act, current, norm, err)
    assert kinds["act_cast"]["launches"] == 1 and kinds["dact_cast"]["launches"] == 1
    assert sorted(err) == sorted(TOL[act, current, norm, bias]) and all(e <= sum(TOL[act, current, norm, bias][k]) for k, e in err.items()), err
