"""Attention core at 16 <= S <= 112 (csrc/mi_attn_short.hip: one workgroup per (batch, kv head), one launch each way): float64
parity, strides / isolation / reproducibility, the module route, and the refusals."""
import numpy as np
import pytest
import torch

from llm_fp8_amd.pytorch.attention import _SHORT_MIN_S
from oracle import fp8_oracle as O
from tests.util import bf16_bits

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops(dev):
    from llm_fp8_amd.pytorch import ops as _ops
    from llm_fp8_amd import _lib
    assert _lib.load().mi_device_supported() == 1, "not a gfx950 device"
    return _ops


# ---- inputs and bounds of tests/test_attention_gpu.py (_rand, _check_fwd, _check_bwd), copied unchanged: the project's own
# bounds for the same arithmetic
def _rand(B, S, H, G, D, seed):
    """q (times 2: a sharper softmax), k, v, dO/4, bf16 on the CPU: the inputs of test_kernels_gpu's oracle tests."""
    g = torch.Generator().manual_seed(seed)
    q, k, v = (torch.randn(B, S, n, D, generator=g).to(torch.bfloat16) for n in (H, G, G))
    do = (torch.randn(B, S, H, D, generator=g) / 4).to(torch.bfloat16)
    return q * 2.0, k, v, do


def _check_fwd(o, lse, o_ref, lse_ref, v, what):
    # the bounds of test_attn_fwd_vs_oracle: P is rounded to bf16 before P.V and O to bf16 at the end (2^-8 relative each,
    # on values bounded by max|v|); lse is an fp32 log-sum-exp of fp32 scores
    np.testing.assert_allclose(o.float().cpu().numpy(), o_ref, rtol=2 ** -6, atol=2 ** -7 * float(v.abs().max()), err_msg=what)
    np.testing.assert_allclose(lse.cpu().numpy(), lse_ref, rtol=0, atol=2e-3, err_msg=what)


def _check_bwd(got, ref, name):
    # the bounds of test_attn_bwd_vs_oracle: P, dS and the outputs are rounded to bf16 (2^-8 each); errors add over the
    # contraction like a random walk
    got = got.float().cpu().numpy()
    tol = 2 ** -6 * np.abs(ref) + 2 ** -7 * np.sqrt(np.mean(ref ** 2))
    bad = np.abs(got - ref) > tol
    assert bad.mean() < 1e-3, f"{name}: {bad.sum()} / {bad.size} outside tolerance, max diff {np.abs(got - ref).max():.4g}"
    rel = np.linalg.norm(got - ref) / np.linalg.norm(ref)
    assert rel < 6e-3, f"{name}: relative Frobenius error {rel:.4g}"


# ------------------------------------------------------------------------------------------------ 1. float64
@pytest.mark.parametrize("H,G", [(2, 2), (6, 2), (4, 1)])  # groups of 1, 3 and 4 query heads
@pytest.mark.parametrize("D", [64, 128])
# S -> 32-row slices (nsl): 16 -> 1 (three idle key waves), 32 -> 1 (one full slice), 48 -> 2 (a partial second slice), 64 -> 2 (two
# full), 80 -> 3 (a partial third), 96 -> 3 (three full), 112 -> 4 (the last partial).  80 and 96 are the `nsl == 3` deal of the
# (head, slice) items over the waves, the one case that does not rotate the slice by item / 4
@pytest.mark.parametrize("S", [16, 32, 48, 64, 80, 96, 112])
def test_short_vs_float64(ops, dev, S, D, H, G):
    B, scale = 2, D ** -0.5
    q, k, v, do = _rand(B, S, H, G, D, seed=S + D + H)
    o_ref, lse_ref = O.attention_f64(bf16_bits(q), bf16_bits(k), bf16_bits(v), scale, True)
    qd, kd, vd, dod = (t.to(dev) for t in (q, k, v, do))
    o, lse = ops.attn_short_fwd(qd, kd, vd, scale, True)
    _check_fwd(o, lse, o_ref, lse_ref, v, f"S{S} D{D} H{H} G{G}")
    # as test_attn_grid_vs_float64: delta = rowsum(dO * O) of the stored bf16 O just checked, in the reference too
    refs = O.attention_bwd_f64(bf16_bits(q), bf16_bits(k), bf16_bits(v), bf16_bits(do), scale, True, o_bits=bf16_bits(o))
    grads = ops.attn_short_bwd(dod, qd, kd, vd, o, lse, scale, True)
    for got, ref, name in zip(grads, refs, ("dq", "dk", "dv")):
        _check_bwd(got, ref, name)


# ------------------------------------------------------------------------------------------------ 2. strides and isolation
CANARY = 0x7FC1  # a bf16 quiet NaN: whatever reads it into a sum poisons the result


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("S", [48, 80])  # 80: a partial third slice and an idle fourth key wave
def test_strided_views_canaries_batches_and_reproducibility(ops, dev, S, D):
    """q, k, v column slices of one fused [B, S, (H + 2G) D] buffer; o, dO, dq, dk, dv views with token strides of their own
    inside NaN-canary buffers; lse between NaN guards.  Bitwise the contiguous call, nothing else written, batch 0 independent
    of batch 1, and a second call gives the same bits (the dQ reduction has a fixed order)."""
    B, H, G, scale = 2, 6, 2, D ** -0.5
    q, k, v, do = (t.to(dev) for t in _rand(B, S, H, G, D, seed=D))
    fused = torch.cat([t.reshape(B, S, -1) for t in (q, k, v)], dim=-1).contiguous()
    fused0 = fused.clone()
    qv, kv, vv = (t.view(B, S, -1, D) for t in fused.split([H * D, G * D, G * D], dim=-1))
    width = {"o": H, "do": H, "dq": H, "dk": G, "dv": G}
    ts = {n: width[n] * D + 8 * (i + 1) for i, n in enumerate(width)}
    span = (B * S + 128) * max(ts.values())  # 128 canary tokens and more behind the last token at every stride
    bufs = {n: torch.full((span,), CANARY, dtype=torch.int16, device=dev) for n in width}
    shape = {n: (B, S, width[n], D) for n in width}
    stride = {n: (S * ts[n], ts[n], D, 1) for n in width}
    view = {n: bufs[n].view(torch.bfloat16).as_strided(shape[n], stride[n]) for n in width}
    view["do"].copy_(do)
    do0 = bufs["do"].clone()

    o_c, lse_c = ops.attn_short_fwd(q, k, v, scale, True)
    dq_c, dk_c, dv_c = ops.attn_short_bwd(do, q, k, v, o_c, lse_c, scale, True)
    guard, n_lse = 256, B * H * S
    lse_buf = torch.full((guard + n_lse + guard,), float("nan"), device=dev)
    lse_s = lse_buf[guard:guard + n_lse].view(B, H, S)
    ops.attn_short_fwd(qv, kv, vv, scale, True, out=(view["o"], lse_s))
    ops.attn_short_bwd(view["do"], qv, kv, vv, view["o"], lse_s, scale, True, out=(view["dq"], view["dk"], view["dv"]))
    torch.cuda.synchronize()

    assert torch.equal(lse_s, lse_c) and torch.isfinite(lse_c).all(), "lse"
    assert torch.isnan(lse_buf[:guard]).all() and torch.isnan(lse_buf[guard + n_lse:]).all(), "lse: a guard element was written"
    for n, ref in (("o", o_c), ("dq", dq_c), ("dk", dk_c), ("dv", dv_c)):
        assert torch.isfinite(ref).all(), f"{n} is not finite"
        assert torch.equal(view[n].view(torch.int16), ref.view(torch.int16)), f"{n}: strided call differs from the contiguous one"
        outside = torch.ones(span, dtype=torch.bool, device=dev)
        outside.as_strided(shape[n], stride[n]).fill_(False)
        assert (bufs[n][outside] == CANARY).all(), f"{n}: an element outside the tensor was written"
    assert torch.equal(fused, fused0) and torch.equal(bufs["do"], do0), "an input was written"

    q1, k1, v1, do1 = (t[:1].contiguous() for t in (q, k, v, do))
    o_1, lse_1 = ops.attn_short_fwd(q1, k1, v1, scale, True)
    one = (o_1, lse_1) + ops.attn_short_bwd(do1, q1, k1, v1, o_1, lse_1, scale, True)
    o_2, lse_2 = ops.attn_short_fwd(q, k, v, scale, True)
    again = (o_2, lse_2) + ops.attn_short_bwd(do, q, k, v, o_2, lse_2, scale, True)
    for n, first, b0, second in zip(("o", "lse", "dq", "dk", "dv"), (o_c, lse_c, dq_c, dk_c, dv_c), one, again):
        assert torch.equal(b0, first[:1]), f"{n}: batch 0 depends on batch 1"
        assert torch.equal(second, first), f"{n}: a second call gave other bits"


# ------------------------------------------------------------------------------------------------ 3. module route
# every (S, D) the module sends to the short kernels, from the table itself: D = 128 with S in 64 .. 112, D = 64 with S in 80 .. 112
ADMITTED = [(S, D) for D, lo in sorted(_SHORT_MIN_S.items()) for S in range(lo, 128, 16)]


@pytest.mark.parametrize("S,D", ADMITTED)
def test_dot_product_attention_short_route_matches_sdpa(dev, monkeypatch, S, D):
    """The construction and the bound of test_dot_product_attention_flash_path_matches_sdpa; the other side is the same module
    with the short route switched off."""
    from llm_fp8_amd.pytorch import attention as A
    from llm_fp8_amd.pytorch.profiler import KernelTimer
    B, H, G = 2, 6, 2
    core = A.DotProductAttention(H, D, G, attention_dropout=0.0, attn_mask_type="causal", qkv_format="bshd")
    torch.manual_seed(3)
    q, k, v = (torch.randn(B, S, n, D, device=dev, dtype=torch.bfloat16, requires_grad=True) for n in (H, G, G))
    assert A._short_ok(q, k, v, True, 0.0) and not A._flash_ok(q, k, v, True, 0.0)
    with KernelTimer().install() as timer:
        o = core(q, k, v)
        go = torch.randn_like(o) / 4
        o.backward(go)
    torch.cuda.synchronize()
    launches = {n: s["launches"] for n, s in timer.summarize().items() if n.startswith("attn")}
    assert launches == {"attn_short_fwd": 1, "attn_short_bwd": 1}, launches
    got = (o.detach(), q.grad.clone(), k.grad.clone(), v.grad.clone())
    q.grad = k.grad = v.grad = None
    monkeypatch.setenv("LLM_FP8_AMD_NO_SHORT_ATTN", "1")
    assert not A._short_ok(q, k, v, True, 0.0)
    o2 = core(q, k, v)
    o2.backward(go)
    for a, b, name in zip(got, (o2.detach(), q.grad, k.grad, v.grad), ("o", "dq", "dk", "dv")):
        rel = ((a.float() - b.float()).norm() / b.float().norm()).item()
        assert rel < 1e-2, f"{name}: {rel:.4g}"


@pytest.mark.parametrize("D", sorted(_SHORT_MIN_S))
def test_below_the_table_the_module_stays_off_the_short_kernels(dev, monkeypatch, D):
    """At the largest multiple of 16 below _SHORT_MIN_S[D] (a length the kernels take, test 1) the module keeps the SDPA route."""
    from llm_fp8_amd.pytorch import attention as A
    from llm_fp8_amd.pytorch.profiler import KernelTimer
    monkeypatch.delenv("LLM_FP8_AMD_NO_SHORT_ATTN", raising=False)
    B, S, H, G = 2, _SHORT_MIN_S[D] - 16, 6, 2
    assert S >= 16 and S % 16 == 0
    core = A.DotProductAttention(H, D, G, attention_dropout=0.0, attn_mask_type="causal", qkv_format="bshd")
    torch.manual_seed(5)
    q, k, v = (torch.randn(B, S, n, D, device=dev, dtype=torch.bfloat16, requires_grad=True) for n in (H, G, G))
    assert not A._short_ok(q, k, v, True, 0.0) and not A._flash_ok(q, k, v, True, 0.0)
    with KernelTimer().install() as timer:
        o = core(q, k, v)
        o.backward(torch.randn_like(o) / 4)
    torch.cuda.synchronize()
    assert not [n for n in timer.summarize() if n.startswith("attn")], sorted(timer.summarize())
    assert all(torch.isfinite(t).all() for t in (o, q.grad, k.grad, v.grad))


# ------------------------------------------------------------------------------------------------ 4. refusals
@pytest.mark.parametrize("S,H,G,D,causal", [(128, 4, 2, 64, True), (24, 4, 2, 64, True), (0, 4, 2, 64, True), (64, 4, 2, 96, True),
                                            (64, 3, 2, 64, True), (64, 4, 2, 64, False)])
def test_refused_by_both_launchers_and_short_ok(ops, dev, S, H, G, D, causal):
    from llm_fp8_amd.pytorch import attention as A
    q, k, v = (torch.randn(1, S, n, D, device=dev, dtype=torch.bfloat16) for n in (H, G, G))
    assert not A._short_ok(q, k, v, causal, 0.0)
    with pytest.raises(RuntimeError, match="mi_attn_short_fwd"):
        ops.attn_short_fwd(q, k, v, D ** -0.5, causal)
    o, lse = torch.zeros_like(q), torch.zeros(1, H, S, device=dev)
    with pytest.raises(RuntimeError, match="mi_attn_short_bwd"):
        ops.attn_short_bwd(o, q, k, v, o, lse, D ** -0.5, causal)
