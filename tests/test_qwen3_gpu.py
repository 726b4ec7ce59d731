"""GPU: the QK-norm attention module and a tiny Qwen3 model on the device.  (a) MultiheadAttention(qk_norm_type="RMSNorm") on the
fused route (mi_qknorm_rope_qkv) is at least as close to an fp32 evaluation of the same module as the torch route is; (b) a tiny
Qwen3 trains for three steps through train's own step under four FP8 scenarios; (c) the fused route withdraws the q|k|v
projection's DyHandoff."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu

SWITCH = "LLM_FP8_AMD_NO_QK_NORM_FUSION"


def _attention(dev, qk_norm=True):
    import llm_fp8_amd.pytorch as te
    torch.manual_seed(5)
    m = te.MultiheadAttention(hidden_size=512, num_attention_heads=4, kv_channels=128, num_gqa_groups=2, bias=False,
                              attention_dropout=0.0, layernorm_epsilon=1e-6, normalization="RMSNorm", input_layernorm=True,
                              fuse_qkv_params=False, qkv_format="bshd", params_dtype=torch.bfloat16, device=dev,
                              **(dict(qk_norm_type="RMSNorm", qk_norm_eps=1e-6) if qk_norm else {}))
    with torch.no_grad():  # norm weights away from one: a dropped or swapped gamma must show
        for n, p in m.named_parameters():
            if "norm" in n:
                p.copy_(0.5 + torch.rand(p.shape, device=dev))
    return m


def _rope(dev, rows=256):
    import llm_fp8_amd.pytorch as te
    return te.attention.RotaryPositionEmbedding(128, rotary_base=1e6)(max_seq_len=rows).to(dev)


def _grads(m, x, dy, rope):
    """(output, input gradient, gamma gradients, q|k|v weight gradient) of one forward + backward, as float32 on the CPU."""
    m.zero_grad(set_to_none=True)
    x = x.detach().clone().requires_grad_(True)
    out = m(x, rotary_pos_emb=rope)
    out.backward(dy)
    ln = m.layernorm_qkv
    wg = torch.cat([ln.query_weight.grad, ln.key_weight.grad, ln.value_weight.grad], 0)
    gam = torch.cat([m.q_norm.weight.grad, m.k_norm.weight.grad], 0)
    return [t.detach().float().cpu() for t in (out, x.grad, gam, wg)]


def test_fused_route_is_no_further_from_fp32_than_the_torch_route(dev, monkeypatch):
    """hidden 512, 4 heads, 2 KV heads, D 128, bf16, batch 2 x seq 128, no FP8 autocast.  Reference: the same module, weights and
    inputs converted to fp32, on the CPU (the torch route with torch's attention).  Each of max-abs and rms error of the output,
    the input gradient, the gamma gradients and the q|k|v weight gradient on the fused route is at most 1.25 x the torch route's:
    the fused route rounds q and k once where the torch route rounds after every elementwise step and rotates with bf16 tables;
    the 0.25 allows for summation-order noise in the attention backward both share.
    Recorded on an MI355X (fused / torch): output max-abs 1.708 / 1.708, rms 0.07104 / 0.07122; input gradient 0.7934 / 0.8068,
    0.06714 / 0.06797; gamma gradients 0.298 / 0.298, 0.06478 / 0.0746; q|k|v weight gradient 0.04634 / 0.04244, 0.003619 / 0.00365."""
    from llm_fp8_amd.pytorch import attention as A
    m = _attention(dev)
    rope = _rope(dev)
    g = torch.Generator(device=dev).manual_seed(6)
    x = torch.randn(2, 128, 512, device=dev, dtype=torch.bfloat16, generator=g)
    dy = (torch.randn(2, 128, 512, device=dev, generator=g) / 16).to(torch.bfloat16)
    calls = {"n": 0}
    real = A._QKNormRoPESplitFn.forward

    def counted(*a, **k):
        calls["n"] += 1
        return real(*a, **k)

    monkeypatch.setattr(A._QKNormRoPESplitFn, "forward", staticmethod(counted))
    monkeypatch.delenv(SWITCH, raising=False)
    fused = _grads(m, x, dy, rope)
    assert calls["n"] == 1, "the fused route did not run"
    monkeypatch.setenv(SWITCH, "1")
    plain = _grads(m, x, dy, rope)
    assert calls["n"] == 1, "the switch did not force the torch route"
    ref_m = copy.deepcopy(m).float().cpu()
    ref = _grads(ref_m, x.float().cpu(), dy.float().cpu(), rope.cpu())
    for name, f, p, r in zip(("output", "input gradient", "gamma gradients", "qkv weight gradient"), fused, plain, ref):
        ef, ep = f - r, p - r
        fa, pa = ef.abs().max().item(), ep.abs().max().item()
        fr, pr = ef.pow(2).mean().sqrt().item(), ep.pow(2).mean().sqrt().item()
        print(f"{name}: max-abs fused {fa:.4g} torch {pa:.4g}; rms fused {fr:.4g} torch {pr:.4g}; max |ref| {r.abs().max().item():.4g}")
        assert torch.isfinite(f).all() and torch.isfinite(p).all()
        assert fa <= 1.25 * pa, name
        assert fr <= 1.25 * pr, name


def test_fused_route_withdraws_the_dy_handoff(dev, monkeypatch):
    """Under delayed scaling the q|k|v projection offers its grad_output quantisation to the rotary split; the QK-norm split has no
    FP8-emitting backward, so after the forward the hand-off is not offered (and the backward runs); the plain rotary split of the
    same module without QK norm keeps it, which shows that the observation sees an offer when there is one."""
    import llm_fp8_amd.pytorch as te
    from llm_fp8_amd.common.recipe import DelayedScaling, Format
    from llm_fp8_amd.pytorch import attention as A
    from llm_fp8_amd.pytorch.fp8 import FP8GlobalStateManager
    monkeypatch.delenv(SWITCH, raising=False)
    monkeypatch.delenv("LLM_FP8_AMD_NO_DY_HANDOFF", raising=False)
    made = []

    class Recorded(A.DyHandoff):
        __slots__ = ()

        def __init__(self):
            super().__init__()
            made.append(self)

    monkeypatch.setattr(A, "DyHandoff", Recorded)
    rope = _rope(dev)
    recipe = DelayedScaling(fp8_format=Format.HYBRID, amax_history_len=16, amax_compute_algo="max")
    seen = {}
    try:
        for qk_norm in (True, False):
            FP8GlobalStateManager.reset()
            m = _attention(dev, qk_norm)
            x = torch.randn(2, 128, 512, device=dev, dtype=torch.bfloat16, requires_grad=True)
            made.clear()
            with te.fp8_autocast(enabled=True, fp8_recipe=recipe):
                out, skip = m(x, rotary_pos_emb=rope, _with_skip=True)
            assert len(made) == 1
            seen[qk_norm] = made[0].offered()
            (out.float().sum() + skip.float().sum()).backward()
            torch.cuda.synchronize()
            assert torch.isfinite(x.grad).all() and torch.isfinite(m.layernorm_qkv.query_weight.grad).all()
            if qk_norm:
                assert torch.isfinite(m.q_norm.weight.grad).all() and m.q_norm.weight.grad.abs().sum() > 0
    finally:
        FP8GlobalStateManager.reset()
    assert seen == {True: False, False: True}


def _tiny_cfg(train, scenario):
    return train.TrainingConfig(model_name="qwen3-0.6b", batch_size=2, max_seq_length=128, mixed_precision="fp8", fp8_scenario=scenario,
                                use_te=True, sharding_mode="none", num_hidden_layers=2, vocab_size=512, learning_rate=1e-2,
                                num_warmup_steps=0)  # (1e-2: a bf16 weight near 1 has a spacing of 2^-7, a step of 1e-3 would round away)


def test_tiny_qwen3_trains_under_four_scenarios(dev, monkeypatch):
    """TEQwen3ForCausalLM, 2 layers, hidden 512, 4 heads of 128, 2 KV heads, FFN 1024, vocab 512, batch 2 x 128, ClippedAdamW, one
    repeated batch, three steps under each of default, mxfp8, current, block on the fused route: losses finite, no non-finite
    gradient, every q_norm / k_norm weight moved.
    First-step loss: `ref` is the loss of the same weights with every FP8 region off on the torch route.  The torch route under a
    scenario deviates from `ref` by that scenario's FP8 noise; `yard` is the largest such deviation over the four scenarios (the
    maximum, so that one scenario's errors cancelling by chance does not shrink the yardstick).  The fused route changes q and k by
    less than their bf16 rounding, so its first-step loss must deviate from `ref` by at most 2 x yard under every scenario.
    Recorded on an MI355X: bf16 6.340910; torch route default 6.350278, mxfp8 6.349259, current 6.346507, block 6.349897
    (yardstick 9.37e-3); fused route first-step deviations 8.26e-3, 8.09e-3, 4.69e-3, 8.91e-3."""
    import llm_fp8_amd.pytorch as te
    from llm_fp8_amd import qwen, train
    from llm_fp8_amd.optim import ClippedAdamW
    from llm_fp8_amd.pytorch import attention as A
    from llm_fp8_amd.pytorch.fp8 import FP8GlobalStateManager as G
    device = torch.device(dev)
    orig_cfg = qwen.qwen3_config
    monkeypatch.setattr(qwen, "qwen3_config", lambda name, **kw: orig_cfg(name, **{**dict(
        hidden_size=512, intermediate_size=1024, num_attention_heads=4, num_key_value_heads=2, head_dim=128,
        max_position_embeddings=256), **kw}))
    gen = torch.Generator(device=device).manual_seed(12)
    batch = train.synthetic_batch(_tiny_cfg(train, "default"), 512, device, gen)
    state = {}
    calls = {"n": 0}
    real = A._QKNormRoPESplitFn.forward

    def counted(*a, **k):
        calls["n"] += 1
        return real(*a, **k)

    monkeypatch.setattr(A._QKNormRoPESplitFn, "forward", staticmethod(counted))

    def build(scenario):
        G.reset()
        cfg = _tiny_cfg(train, scenario)
        torch.manual_seed(31)
        model = train.prepare_model(train.create_model(cfg, device), cfg)
        if state:
            model.load_state_dict(state["sd"], strict=False)
        else:
            with torch.no_grad():
                for n, p in model.named_parameters():
                    if n.endswith(("q_norm.weight", "k_norm.weight")):
                        p.copy_(0.5 + torch.rand(p.shape, device=device))
            state["sd"] = {k: v.clone() for k, v in model.state_dict().items() if not k.endswith("_extra_state")}
        model.train()
        assert isinstance(model.model.layers[0], qwen.TEQwen3DecoderLayer)
        return model, cfg

    def first_loss(scenario):
        model, _ = build(scenario)
        with torch.no_grad():
            return model(**batch).loss.item()

    try:
        monkeypatch.setenv(SWITCH, "1")
        real_autocast = te.fp8_autocast
        monkeypatch.setattr(te, "fp8_autocast", lambda enabled=True, **kw: real_autocast(enabled=False, **kw))
        ref = first_loss("default")
        monkeypatch.setattr(te, "fp8_autocast", real_autocast)
        scenarios = ("default", "mxfp8", "current", "block")
        torch_route = {s: first_loss(s) for s in scenarios}
        assert calls["n"] == 0
        monkeypatch.delenv(SWITCH)
        fused = {}
        for s in scenarios:
            model, cfg = build(s)
            opt, sched = train.create_optimizer(model, cfg)
            assert isinstance(opt, ClippedAdamW)
            norms = {n: p.detach().clone() for n, p in model.named_parameters() if n.endswith(("q_norm.weight", "k_norm.weight"))}
            assert len(norms) == 4
            bad = []
            for n, p in model.named_parameters():
                p.register_post_accumulate_grad_hook(lambda q, n=n: bad.append((n, torch.isfinite(q.grad).all())))
            before = calls["n"]
            losses = [train.train_step(model, batch, opt, sched, cfg).item() for _ in range(3)]
            assert calls["n"] == before + 3 * 2, "the fused QK-norm split did not run in every layer and step"
            fused[s] = losses
            assert all(torch.isfinite(torch.tensor(losses))), (s, losses)
            assert bad and all(bool(ok) for _, ok in bad), (s, [n for n, ok in bad if not bool(ok)])
            assert {n for n, _ in bad} >= set(norms)
            for n, p in model.named_parameters():
                if n in norms:
                    assert not torch.equal(p.detach(), norms[n]), (s, n)
    finally:
        G.reset()
    yard = max(abs(torch_route[s] - ref) for s in scenarios)
    print(f"bf16 loss {ref:.6f}; torch route " + ", ".join(f"{s} {torch_route[s]:.6f}" for s in scenarios) + f"; yardstick {yard:.3e}")
    for s in scenarios:
        print(f"{s}: fused losses {fused[s]}, first-step deviation {abs(fused[s][0] - ref):.3e}")
    assert yard > 0
    for s in scenarios:
        assert abs(fused[s][0] - ref) <= 2 * yard, s
