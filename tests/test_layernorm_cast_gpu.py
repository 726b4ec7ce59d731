"""LayerNorm fused with the FP8 cast (mi_layernorm_stats, mi_ln_cast, mi_amax_ln, mi_layernorm_bwd) against float64 numpy, and the
LayerNormLinear / LayerNormMLP routes through them.

Module tolerance (test_module_route): relative Frobenius error of the output and of every gradient against the float64 module on
dequantised operands (_reference of tests/test_act_cast_gpu.py for the MLP, _linear_reference here).  TOL holds, per case and tensor,
what the unfused route (fused_norm = False: torch's LayerNorm in front of the FP8 node) measured against that reference on MI355X
over seeds 0-4 at 128 tokens, hidden 768: (its largest error, largest minus smallest over the seeds).  The fused route is allowed
their sum.  Every figure is in profiles/layernorm_cast.txt."""
import numpy as np
import pytest
import torch

from oracle import fp8_oracle as O
from tests import glue_oracle as G
from tests.test_act_cast_gpu import _fp8_close, _qdq, _reference

pytestmark = pytest.mark.gpu
EPS = 1e-5
TOL = {  # (module, zero_centered_gamma, layer_norm_bias frozen, current scaling): {tensor: (unfused max, unfused spread)}
    ("linear", False, False, False): {"out": (0.01653, 0.00057), "dx": (0.00236, 2e-05), "layer_norm_weight": (0.00244, 0.0002), "layer_norm_bias": (0.0025, 0.00017), "weight": (0.01666, 0.0005), "bias": (0.00178, 0.00022)},
    ("linear", False, False, True): {"out": (0.01654, 0.00812), "dx": (0.00235, 2e-05), "layer_norm_weight": (0.00245, 0.00013), "layer_norm_bias": (0.00248, 0.0003), "weight": (0.01664, 0.00813), "bias": (0.00178, 0.00022)},
    ("linear", True, False, False): {"out": (0.01641, 0.00049), "dx": (0.003, 8e-05), "layer_norm_weight": (0.00244, 0.0002), "layer_norm_bias": (0.0025, 0.00017), "weight": (0.01666, 0.00041), "bias": (0.00178, 0.00022)},
    ("linear", True, False, True): {"out": (0.01859, 0.00517), "dx": (0.00298, 7e-05), "layer_norm_weight": (0.00245, 0.00013), "layer_norm_bias": (0.00248, 0.0003), "weight": (0.01859, 0.00484), "bias": (0.00178, 0.00022)},
    ("mlp", False, False, False): {"out": (0.02675, 0.00123), "dx": (0.03427, 0.00215), "layer_norm_weight": (0.03543, 0.0043), "fc1_weight": (0.03776, 0.00211), "fc2_weight": (0.03194, 0.00089), "fc1_bias": (0.01111, 0.00112), "fc2_bias": (0.00177, 0.00016), "layer_norm_bias": (0.03777, 0.00699)},
    ("mlp", False, False, True): {"out": (0.02824, 0.00528), "dx": (0.03499, 0.00674), "layer_norm_weight": (0.03498, 0.00715), "fc1_weight": (0.03895, 0.00897), "fc2_weight": (0.03407, 0.00662), "fc1_bias": (0.01147, 0.00423), "fc2_bias": (0.00177, 0.00016), "layer_norm_bias": (0.03891, 0.01317)},
    ("mlp", False, True, False): {"out": (0.02675, 0.00123), "dx": (0.03427, 0.00215), "layer_norm_weight": (0.03543, 0.0043), "fc1_weight": (0.03776, 0.00211), "fc2_weight": (0.03194, 0.00089), "fc1_bias": (0.01111, 0.00112), "fc2_bias": (0.00177, 0.00016)},
    ("mlp", False, True, True): {"out": (0.02824, 0.00528), "dx": (0.03499, 0.00674), "layer_norm_weight": (0.03498, 0.00715), "fc1_weight": (0.03895, 0.00897), "fc2_weight": (0.03407, 0.00662), "fc1_bias": (0.01147, 0.00423), "fc2_bias": (0.00177, 0.00016)},
}


@pytest.fixture(scope="module")
def ops():
    from llm_fp8_amd.pytorch import ops as o
    return o


def _rows(rows, cols, g, offset_every=4, first=0):
    """bf16 [rows, cols]: N(0, 4) rows, every `offset_every`-th from `first` a large-offset row (mean 64, spread 0.25 before rounding)."""
    x = torch.randn(rows, cols, generator=g) * 2
    x[first::offset_every] = 64 + 0.25 * torch.randn(rows, cols, generator=g)[first::offset_every]
    return x.to(torch.bfloat16)


def _stats64(x):
    x64 = x.double().numpy()
    mean = x64.mean(1)
    return x64, mean, 1.0 / np.sqrt(((x64 - mean[:, None]) ** 2).mean(1) + EPS)


@pytest.mark.parametrize("cols", [8, 520, 768, 8192])
@pytest.mark.parametrize("rows", [1, 37])
def test_stats_vs_float64(ops, dev, rows, cols):
    x = _rows(rows, cols, torch.Generator().manual_seed(rows + cols))
    x64, mean, rstd = _stats64(x)
    got_m, got_r = (t.cpu().numpy().astype(np.float64) for t in ops.layernorm_stats(x.to(dev), EPS))
    em, er = np.abs(got_m - mean) / np.abs(x64).mean(1), np.abs(got_r - rstd) / rstd
    print(f"stats {rows}x{cols}: mean err / mean|x| {em.max():.3g} (bound {(cols / 64 + 16) * 2.0 ** -24:.3g}), rstd rel {er.max():.3g}")
    assert (em <= (cols / 64 + 16) * 2.0 ** -24).all() and (er <= G.rstd_rtol(cols) + 2 * 2.0 ** -24).all()


def cast_inputs(shape, zero_centered):
    """(x, mean fp32, rstd fp32, gamma, beta, float64 value the cast quantises): a quarter of the rows are large-offset rows."""
    R, C = shape
    g = torch.Generator().manual_seed(R * 3 + C + zero_centered)
    x = _rows(R, C, g, first=1)
    x64, mean, rstd = _stats64(x)
    mean, rstd = torch.from_numpy(mean).float(), torch.from_numpy(rstd).float()
    gamma = (torch.rand(C, generator=g) + (-0.5 if zero_centered else 0.5)).to(torch.bfloat16)
    beta = (torch.randn(C, generator=g) * 0.5).to(torch.bfloat16)
    gg = gamma.double().numpy() + (1.0 if zero_centered else 0.0)
    v = (x64 - mean.double().numpy()[:, None]) * rstd.double().numpy()[:, None] * gg + beta.double().numpy()
    return x, mean, rstd, gamma, beta, v


@pytest.mark.parametrize("zero_centered", [False, True])
@pytest.mark.parametrize("shape", [(8, 8), (136, 72), (256, 264)])
def test_cast_and_amax_vs_float64(ops, dev, shape, zero_centered):
    x, mean, rstd, gamma, beta, v = cast_inputs(shape, zero_centered)
    xd, md, rd, gd, bd = (t.to(dev) for t in (x, mean, rstd, gamma, beta))
    amax, scale = torch.zeros(1, dtype=torch.float32, device=dev), torch.tensor([16.0], dtype=torch.float32, device=dev)
    y, yT = ops.ln_cast(xd, md, rd, gd, bd, scale, amax, O.E4M3, zero_centered=zero_centered)
    _fp8_close(y, yT, v, 16.0, O.E4M3)
    np.testing.assert_allclose(amax.item(), np.abs(v).max(), rtol=1e-5)
    part = torch.empty(7, dtype=torch.float32, device=dev)
    ops.amax_ln(xd, md, rd, gd, bd, zero_centered, part)
    assert part.max().item() == amax.item()


# every instance of the dispatcher: its largest width where a row is split over 2 or 4 waves, and widths that are no multiple of 512
@pytest.mark.parametrize("dres,n_partials,zero_centered", [(False, 1, False), (True, 512, True), (True, 1, False)])
@pytest.mark.parametrize("cols", [8, 520, 768, 1600, 2048, 3072, 4096, 6144, 8192])
@pytest.mark.parametrize("rows", [1, 3, 37])
def test_bwd_vs_float64(ops, dev, rows, cols, dres, n_partials, zero_centered):
    g = torch.Generator().manual_seed(cols + rows)
    x = (torch.randn(rows, cols, generator=g) * torch.exp(torch.randn(rows, 1, generator=g)) + torch.randn(rows, 1, generator=g)).to(torch.bfloat16)
    gamma = (torch.rand(cols, generator=g) + (-0.5 if zero_centered else 0.5)).to(torch.bfloat16)
    dy = (torch.randn(rows, cols, generator=g) / 8).to(torch.bfloat16)
    res = (torch.randn(rows, cols, generator=g) / 8).to(torch.bfloat16)
    x64, mean, rstd = _stats64(x)
    xhat, dy64 = (x64 - mean[:, None]) * rstd[:, None], dy.double().numpy()
    dyg = dy64 * (gamma.double().numpy() + (1.0 if zero_centered else 0.0))
    dx_ref = rstd[:, None] * (dyg - dyg.mean(1, keepdims=True) - xhat * (dyg * xhat).mean(1, keepdims=True))
    dx_ref = dx_ref + (res.double().numpy() if dres else 0.0)
    xd, gd, dyd = x.to(dev), gamma.to(dev), dy.to(dev)
    md, rd = ops.layernorm_stats(xd, EPS)
    kw = dict(dres=res.to(dev) if dres else None, n_partials=n_partials, zero_centered=zero_centered)
    dx, dgam, dbet = ops.layernorm_bwd(dyd, xd, md, rd, gd, **kw)
    d = np.abs(dx.double().cpu().numpy() - dx_ref)
    tol = 2.0 ** -7 * np.abs(dx_ref) + 1e-5 * np.abs(dx_ref).max()
    assert (d <= tol).all(), f"dx max diff {d.max():.3g} at {np.unravel_index((d - tol).argmax(), d.shape)}"
    for got, ref in ((dgam, (dy64 * xhat).sum(0)), (dbet, dy64.sum(0))):
        np.testing.assert_allclose(got.cpu().numpy(), ref, rtol=1e-4, atol=1e-4 * np.abs(ref).max())
    again = ops.layernorm_bwd(dyd, xd, md, rd, gd, **kw)
    assert all(torch.equal(a, b) for a, b in zip((dx, dgam, dbet), again)), "not bitwise reproducible"


def _linear_reference(mod, x, dy, current):
    """Output and gradients of a LayerNormLinear in float64 on the dequantised operands of its three quantisations."""
    p = {k: v.detach().double().cpu() for k, v in mod.named_parameters()}
    x64 = x.detach().double().cpu().requires_grad_(True)
    lw, lb = p["layer_norm_weight"].requires_grad_(True), p["layer_norm_bias"].requires_grad_(True)
    xc = x64 - x64.mean(-1, keepdim=True)
    xn = xc * torch.rsqrt(xc.pow(2).mean(-1, keepdim=True) + mod.eps) * (lw + 1 if mod.zero_centered_gamma else lw) + lb
    x8, w8 = _qdq(xn.detach().numpy(), O.E4M3, current), _qdq(p["weight"].numpy(), O.E4M3, current)
    dy64 = dy.double().cpu().numpy()
    dy8 = _qdq(dy64, O.E5M2, current)
    xn.backward(torch.from_numpy(dy8 @ w8))
    return {"out": x8 @ w8.T + p["bias"].numpy(), "dx": x64.grad.numpy(), "layer_norm_weight": lw.grad.numpy(),
            "layer_norm_bias": lb.grad.numpy(), "weight": dy8.T @ x8, "bias": dy64.sum(0)}


def route_errors(dev, kind, zero_centered, frozen_bias, current, seed, fused, patch=None):
    """{tensor: relative Frobenius error against the float64 reference} of one forward + backward at 128 tokens, hidden 768.
    `patch` (a monkeypatch): torch's layer_norm is taken away while the module runs."""
    import llm_fp8_amd.pytorch as te
    from llm_fp8_amd.common.recipe import DelayedScaling, Float8CurrentScaling, Format
    torch.manual_seed(seed)
    kw = dict(zero_centered_gamma=zero_centered, params_dtype=torch.bfloat16, device=dev)
    mod = te.LayerNormLinear(768, 256, **kw) if kind == "linear" else te.LayerNormMLP(768, 256, activation="gelu", **kw)
    mod.fused_norm = fused
    with torch.no_grad():
        for k, q in mod.named_parameters():
            if "bias" in k or k == "layer_norm_weight":
                q.add_(torch.randn_like(q) * 0.1)
    mod.layer_norm_bias.requires_grad_(not frozen_bias)
    x = (torch.randn(128, 768, device=dev) + 0.5).to(torch.bfloat16).requires_grad_(True)
    dy = (torch.randn(128, 256 if kind == "linear" else 768, device=dev) / 16).to(torch.bfloat16)
    recipe = Float8CurrentScaling(fp8_format=Format.HYBRID) if current else DelayedScaling(fp8_format=Format.HYBRID)
    if patch is not None:
        patch.setattr(torch.nn.functional, "layer_norm", None)  # a torch LayerNorm on the route is a TypeError
    with te.fp8_autocast(enabled=True, fp8_recipe=recipe):
        out = mod(x)
    out.backward(dy)
    torch.cuda.synchronize()
    if patch is not None:
        patch.undo()
    got = {"out": out, "dx": x.grad, **{k: q.grad for k, q in mod.named_parameters()}}
    ref = (_linear_reference if kind == "linear" else _reference)(mod, x, dy, current)
    if frozen_bias:
        assert got["layer_norm_bias"] is None
        del ref["layer_norm_bias"]
    return {k: float(np.linalg.norm(got[k].detach().double().cpu().numpy() - r) / np.linalg.norm(r)) for k, r in ref.items()}


CASES = [("linear", False, False), ("mlp", False, False), ("linear", True, False), ("mlp", False, True)]


@pytest.mark.parametrize("current", [False, True])
@pytest.mark.parametrize("kind,zero_centered,frozen_bias", CASES)
def test_module_route(dev, monkeypatch, kind, zero_centered, frozen_bias, current):
    err = route_errors(dev, kind, zero_centered, frozen_bias, current, seed=0, fused=True, patch=monkeypatch)
    print(kind, zero_centered, frozen_bias, current, err)
    tol = TOL[kind, zero_centered, frozen_bias, current]
    assert sorted(err) == sorted(tol) and all(e <= sum(tol[k]) for k, e in err.items()), err
