"""Sliding-window causal attention (the WIN instantiations of csrc/mi_attn.hip through mi_attn_fwd_win / mi_attn_bwd_win): float64
parity of o, lse, dq, dk, dv at the windows where the band walk can go wrong, the bitwise identities, and the module and model
routes against the SDPA band-mask route."""
import numpy as np
import pytest
import torch

from tests.util import bf16_bits
from oracle.fp8_oracle import bf16_bits_to_f32

pytestmark = pytest.mark.gpu
CANARY = 0x7FC1  # a bf16 quiet NaN
GUARD = 4096     # sentinel elements in front of and behind every output


@pytest.fixture(scope="module")
def ops(dev):
    from llm_fp8_amd.pytorch import ops as _ops
    from llm_fp8_amd import _lib
    assert _lib.load().mi_device_supported() == 1, "not a gfx950 device"
    return _ops


def _band_ref(q, k, v, do, scale, W):
    """float64 band attention of bf16 tensors, forward and analytic backward -> o, lse (log2 domain), dq, dk, dv."""
    q, k, v, do = (bf16_bits_to_f32(bf16_bits(t)).astype(np.float64) for t in (q, k, v, do))
    B, S, H, D = q.shape
    G = k.shape[2]
    kk, vv = (np.repeat(t, H // G, axis=2) for t in (k, v))
    s = np.einsum("bihd,bjhd->bhij", q, kk) * scale
    i = np.arange(S)
    s = np.where((i[None, :] <= i[:, None]) & (i[None, :] > i[:, None] - W), s, -np.inf)
    m = s.max(-1, keepdims=True)
    p = np.exp(s - m)
    l = p.sum(-1, keepdims=True)
    p /= l
    o = np.einsum("bhij,bjhd->bihd", p, vv)
    dp = np.einsum("bihd,bjhd->bhij", do, vv)
    ds = p * (dp - (p * dp).sum(-1, keepdims=True)) * scale
    dq = np.einsum("bhij,bjhd->bihd", ds, kk)
    dk, dv = (np.einsum("bhij,bihd->bjhd", t, x).reshape(B, S, G, H // G, D).sum(3) for t, x in ((ds, q), (p, do)))
    return o, (m[..., 0] + np.log(l[..., 0])) / np.log(2.0), dq, dk, dv


def _inputs(dev, B, S, H, G, D, seed, fused):
    """q (times 2: a sharper softmax), k, v, dO / 4 on the device; `fused`: q, k, v are column slices of one [B, S, (H + 2G) D] buffer."""
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(B, S, (H + 2 * G) * D, generator=g)
    qkv[..., :H * D] *= 2.0
    qkv = qkv.to(torch.bfloat16).to(dev)
    q, k, v = (t.unflatten(-1, (-1, D)) for t in qkv.split((H * D, G * D, G * D), dim=-1))
    if not fused:
        q, k, v = (t.contiguous() for t in (q, k, v))
    return q, k, v, (torch.randn(B, S, H, D, generator=g) / 4).to(torch.bfloat16).to(dev)


def _guarded(shape, dtype, dev):
    """A tensor in the middle of a sentinel-filled allocation -> (whole buffer, view)."""
    n = int(np.prod(shape))
    buf = (torch.full((n + 2 * GUARD,), CANARY, dtype=torch.int16, device=dev).view(torch.bfloat16) if dtype == torch.bfloat16
           else torch.full((n + 2 * GUARD,), float("nan"), device=dev))
    return buf, buf[GUARD:GUARD + n].view(shape)


def _run(ops, q, k, v, do, scale, W, backward=True):
    """Windowed forward (+ backward) into guarded outputs; the surroundings must come back untouched and every output finite."""
    B, S, H, D = q.shape
    shapes = [(q.shape, torch.bfloat16), ((B, H, S), torch.float32)] + [(t.shape, torch.bfloat16) for t in (q, k, v)] * backward
    bufs, views = zip(*(_guarded(s, dt, q.device) for s, dt in shapes))
    o, lse = ops.attn_fwd(q, k, v, scale, True, out=views[:2], window=W)
    if backward:
        ops.attn_bwd(do, q, k, v, o, lse, scale, True, out=views[2:], window=W)
    for name, buf, view in zip(("o", "lse", "dq", "dk", "dv"), bufs, views):
        edge = torch.cat((buf[:GUARD], buf[-GUARD:]))
        assert torch.isnan(edge).all(), f"{name}: an element outside the tensor was written"
        assert torch.isfinite(view).all(), f"{name} is not finite"
    return views


def _check(o, lse, grads, ref, v, what):
    # P and O rounded to bf16 (2^-8 each, values bounded by max|v|); lse an fp32 log-sum-exp of fp32 scores (the
    # 2e-3 of the other attention tests); gradients 6e-3 relative Frobenius error (P, dS and the outputs rounded to bf16)
    o_ref, lse_ref = ref[:2]
    err = np.abs(o.float().cpu().numpy() - o_ref)
    assert (err <= 2 ** -6 * np.abs(o_ref) + 2 ** -7 * float(v.abs().max())).all(), f"{what}: o off by {err.max():.4g}"
    assert np.abs(lse.cpu().numpy() - lse_ref).max() <= 2e-3, f"{what}: lse off by {np.abs(lse.cpu().numpy() - lse_ref).max():.4g}"
    for name, got, r in zip(("dq", "dk", "dv"), grads, ref[2:]):
        rel = np.linalg.norm(got.float().cpu().numpy() - r) / np.linalg.norm(r)
        assert rel <= 6e-3, f"{what}: {name} relative Frobenius error {rel:.4g}"


SHAPES = [(4, 1, 64, False), (4, 4, 128, True), (2, 2, 128, False)]  # H, G, D, fused qkv views
# W below 32; not a multiple of 32 / 64; across the 64-key tile and the 128-row block; 17 and 33: a row's first visited tile is all
# masked for it; S = 400: TAIL, the last dK/dV slice on the tail
WINDOWS = [(256, w) for w in (2, 17, 33, 64, 65, 100, 128, 129, 200)] + [(400, 48), (400, 130), (400, 399), (128, 16), (128, 127)]


@pytest.mark.parametrize("H,G,D,fused", SHAPES)
@pytest.mark.parametrize("S,W", WINDOWS)
def test_window_vs_float64(ops, dev, S, W, H, G, D, fused):
    q, k, v, do = _inputs(dev, 2, S, H, G, D, seed=S + W + D, fused=fused)
    scale = D ** -0.5
    o, lse, dq, dk, dv = _run(ops, q, k, v, do, scale, W)
    _check(o, lse, (dq, dk, dv), _band_ref(q, k, v, do, scale, W), v, f"S{S} W{W} H{H} G{G} D{D}")
    again = _run(ops, q, k, v, do, scale, W)  # no atomics, no sum across workgroups: the same bits
    for name, a, b in zip(("o", "lse", "dq", "dk", "dv"), (o, lse, dq, dk, dv), again):
        assert torch.equal(a.view(torch.int32 if a.dtype == torch.float32 else torch.int16),
                           b.view(torch.int32 if b.dtype == torch.float32 else torch.int16)), f"{name}: two runs differ"


@pytest.mark.parametrize("H,G,D,fused", SHAPES)
@pytest.mark.parametrize("S", [128, 256, 400])
def test_window_of_one_sees_only_itself(ops, dev, S, H, G, D, fused):
    q, k, v, do = _inputs(dev, 2, S, H, G, D, seed=S + D, fused=fused)
    scale = D ** -0.5
    o, lse = _run(ops, q, k, v, do, scale, 1, backward=False)
    v_ref = v.float().repeat_interleave(H // G, dim=2).cpu().numpy().astype(np.float64)  # o == v of the row's kv head
    s_ii = (q.double() * k.double().repeat_interleave(H // G, dim=2)).sum(-1).permute(0, 2, 1).cpu().numpy()
    err = np.abs(o.float().cpu().numpy() - v_ref)
    assert (err <= 2 ** -6 * np.abs(v_ref) + 2 ** -7 * float(v.abs().max())).all(), err.max()
    assert np.abs(lse.cpu().numpy() - s_ii * scale / np.log(2.0)).max() <= 2e-3


@pytest.mark.parametrize("S,D", [(256, 64), (400, 128)])
@pytest.mark.parametrize("extra", [0, 5])
def test_window_of_the_whole_sequence_is_the_causal_kernels(ops, dev, S, D, extra):
    q, k, v, do = _inputs(dev, 2, S, 4, 2, D, seed=S + extra, fused=True)
    scale = D ** -0.5
    o, lse = ops.attn_fwd(q, k, v, scale, True)
    ref = (o, lse) + ops.attn_bwd(do, q, k, v, o, lse, scale, True)
    for name, a, b in zip(("o", "lse", "dq", "dk", "dv"), ref, _run(ops, q, k, v, do, scale, S + extra)):
        assert torch.equal(a, b), f"{name}: window {S + extra} >= S differs from the call without a window"


def test_dot_product_attention_window_route_matches_sdpa(dev, monkeypatch):
    """The HIP route of DotProductAttention(window_size=(W - 1, 0)) against the same module under LLM_FP8_AMD_NO_WINDOW_ATTN=1 on
    float32 copies of the inputs, by the criteria above."""
    from llm_fp8_amd.pytorch import attention as A
    from llm_fp8_amd.pytorch.profiler import KernelTimer
    B, S, H, G, D, W = 2, 256, 4, 2, 128, 80
    core = A.DotProductAttention(H, D, G, attention_dropout=0.0, attn_mask_type="causal", qkv_format="bshd", window_size=(W - 1, 0))
    q, k, v, do = _inputs(dev, B, S, H, G, D, seed=7, fused=True)

    def run(ts):
        ts = [t.detach().clone().requires_grad_() for t in ts]
        out = core(*ts)
        out.backward(do.reshape(B, S, H * D).to(out.dtype))
        return [out.detach().view(B, S, H, D)] + [t.grad for t in ts]

    monkeypatch.delenv("LLM_FP8_AMD_NO_WINDOW_ATTN", raising=False)
    with KernelTimer().install() as timer:
        got = run((q, k, v))
    launches = {n: s["launches"] for n, s in timer.summarize().items()}
    assert launches.get("attn_fwd_win") == 1 and launches.get("attn_bwd_win") == 1, launches
    monkeypatch.setenv("LLM_FP8_AMD_NO_WINDOW_ATTN", "1")
    ref = [t.double().cpu().numpy() for t in run((q.float(), k.float(), v.float()))]
    err = np.abs(got[0].float().cpu().numpy() - ref[0])
    assert (err <= 2 ** -6 * np.abs(ref[0]) + 2 ** -7 * float(v.abs().max())).all(), err.max()
    for name, g, r in zip(("dq", "dk", "dv"), got[1:], ref[1:]):
        rel = np.linalg.norm(g.float().cpu().numpy() - r) / np.linalg.norm(r)
        assert rel <= 6e-3, f"{name}: relative Frobenius error {rel:.4g}"


# (HIP route's gradient error against the float32 HF model) / (SDPA route's): first measured 1.0024 (1.8020e-2 against 1.7977e-2;
# losses 6.300087 and 6.300066 against HF's 6.299743), plus 25 % -- the precedent of the current-scaling fused / unfused ratio
QWEN3_ERROR_RATIO = 1.0024 * 1.25


def test_tiny_qwen3_with_a_sliding_layer(dev, monkeypatch):
    """2-layer Qwen3, use_sliding_window, max_window_layers = 1 (layer 0 full, layer 1 a window of 96), S = 256, bf16 with every
    fp8_autocast region off so that only the attention core differs between the routes.  Loss and parameter gradients of the HIP
    route, of the SDPA band-mask route and of HF's own Qwen3ForCausalLM in float32 on the CPU with the same weights: the HIP
    route's error against HF may exceed the SDPA route's by QWEN3_ERROR_RATIO at most."""
    import llm_fp8_amd.pytorch as te
    from transformers.models.qwen3.modeling_qwen3 import Qwen3ForCausalLM
    from llm_fp8_amd import llama, qwen
    real_autocast = te.fp8_autocast
    monkeypatch.setattr(te, "fp8_autocast", lambda enabled=True, **kw: real_autocast(enabled=False, **kw))
    cfg = qwen.qwen3_config("qwen3-0.6b", num_hidden_layers=2, hidden_size=256, intermediate_size=512, num_attention_heads=4,
                            num_key_value_heads=2, head_dim=64, vocab_size=512, max_position_embeddings=256,
                            tie_word_embeddings=False, use_sliding_window=True, sliding_window=96, max_window_layers=1)
    torch.manual_seed(0)
    hf = Qwen3ForCausalLM(cfg).to(torch.bfloat16).float()  # float32 arithmetic on bf16-representable weights
    model = qwen.TEQwen3ForCausalLM.from_hf_state_dict(hf.state_dict(), cfg, "default").to(dev)
    assert [m.self_attention.core_attention.window_size for m in model.model.layers] == [None, (95, 0)]
    ids = torch.randint(0, cfg.vocab_size, (2, 256), generator=torch.Generator().manual_seed(1))

    def grads_of(m, x):
        m.zero_grad(set_to_none=True)
        loss = m(input_ids=x, labels=x).loss
        loss.backward()
        return loss.item(), {n: p.grad.detach().double().cpu() for n, p in m.named_parameters() if p.grad is not None}

    def te_run():
        loss, g = grads_of(model, ids.to(dev))
        return loss, llama.to_hf_state_dict({n: t for n, t in g.items() if not n.endswith("_bias")}, cfg)

    loss_ref, g_ref = grads_of(hf, ids)
    monkeypatch.delenv("LLM_FP8_AMD_NO_WINDOW_ATTN", raising=False)
    loss_hip, g_hip = te_run()
    monkeypatch.setenv("LLM_FP8_AMD_NO_WINDOW_ATTN", "1")
    loss_sdpa, g_sdpa = te_run()
    assert set(g_ref) <= set(g_hip) and set(g_ref) <= set(g_sdpa)
    total = lambda g: np.sqrt(sum(float((g[n] - g_ref[n]).pow(2).sum()) for n in g_ref) / sum(float(g_ref[n].pow(2).sum()) for n in g_ref))
    e_hip, e_sdpa = total(g_hip), total(g_sdpa)
    print(f"loss HF {loss_ref:.6f} HIP {loss_hip:.6f} SDPA {loss_sdpa:.6f}; gradient error vs HF: HIP {e_hip:.4e} SDPA {e_sdpa:.4e} "
          f"ratio {e_hip / e_sdpa:.4f}")
    assert e_hip <= QWEN3_ERROR_RATIO * e_sdpa, (e_hip, e_sdpa)
    # the loss is an fp32 mean over 510 tokens of bf16 logits: the routes differ by attention outputs rounded to bf16 (2^-8) twice
    assert abs(loss_hip - loss_ref) <= abs(loss_sdpa - loss_ref) + 2 ** -7 * abs(loss_ref), (loss_hip, loss_sdpa, loss_ref)
