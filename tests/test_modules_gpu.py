"""GPU parity of the module/autograd surface (Linear, LayerNormLinear, LayerNormMLP, MultiheadAttention,
fp8_autocast state machine, te_llama counterpart) against the CPU oracle and the HF bf16 layer."""
import numpy as np
import pytest
import torch

from oracle import fp8_oracle as O
from tests.util import assert_gemm_close, bf16_bits, bits_to_bf16

pytestmark = pytest.mark.gpu


@pytest.fixture()
def te(dev):
    import llm_fp8_amd.pytorch as te_
    from llm_fp8_amd.pytorch.fp8 import FP8GlobalStateManager
    FP8GlobalStateManager.reset()
    yield te_
    FP8GlobalStateManager.reset()


def _recipes():
    from llm_fp8_amd.common.recipe import DelayedScaling, Format, MXFP8BlockScaling
    return DelayedScaling, Format, MXFP8BlockScaling


def _f(t):
    return t.detach().float().cpu().numpy()


@pytest.mark.parametrize("fmt_name,fwd,bwd", [("HYBRID", O.E4M3, O.E5M2), ("E4M3", O.E4M3, O.E4M3)])
@pytest.mark.parametrize("use_bias", [False, True])
def test_linear_delayed_scaling_three_steps_vs_oracle(te, dev, fmt_name, fwd, bwd, use_bias):
    DelayedScaling, Format, _ = _recipes()
    recipe = DelayedScaling(fp8_format=getattr(Format, fmt_name), amax_history_len=4, amax_compute_algo="max")
    M, K, N = 64, 128, 96
    g = torch.Generator().manual_seed(7)
    lin = te.Linear(K, N, bias=use_bias, params_dtype=torch.bfloat16, device=dev)
    with torch.no_grad():
        lin.weight.copy_((torch.randn(N, K, generator=g) * 0.05).to(torch.bfloat16))
        if use_bias:
            lin.bias.copy_((torch.randn(N, generator=g)).to(torch.bfloat16))
    orc = O.DelayedLinearOracle(fwd, bwd, history_len=4, algo="max")
    wbits = bf16_bits(lin.weight)
    bbits = bf16_bits(lin.bias) if use_bias else None
    for step in range(3):
        x = (torch.randn(M, K, generator=g) * (step + 1)).to(torch.bfloat16)
        dy = (torch.randn(M, N, generator=g) / 32).to(torch.bfloat16)
        xd = x.to(dev).requires_grad_(True)
        with te.fp8_autocast(enabled=True, fp8_recipe=recipe):
            y = lin(xd)
        y.backward(dy.to(dev))
        y_ref = O.bf16_bits_to_f32(orc.forward(bf16_bits(x), wbits, bbits))
        orc.end_forward()
        dx_ref, dw_ref, db_ref = orc.backward(bf16_bits(dy))
        orc.end_backward()
        # the oracle's bf16 outputs carry 1 bf16 ulp of their own; compare in f32 with the GEMM tolerance
        assert_gemm_close(_f(y), y_ref, f"y step {step}")
        assert_gemm_close(_f(xd.grad), O.bf16_bits_to_f32(dx_ref), f"dx step {step}")
        assert_gemm_close(_f(lin.weight.grad), O.bf16_bits_to_f32(dw_ref), f"dw step {step}")
        if use_bias:
            np.testing.assert_allclose(_f(lin.bias.grad), O.bf16_bits_to_f32(db_ref), rtol=2 ** -7, atol=1e-3)
        lin.weight.grad = None
        if use_bias:
            lin.bias.grad = None
        # delayed-scaling state: bit-exact (amaxes of the given inputs, K3 arithmetic)
        sf, sb = lin._meta_fwd.state(), lin._meta_bwd.state()
        np.testing.assert_array_equal(sf["scale"].cpu().numpy()[:2], orc.s_fwd[:2], err_msg=f"fwd scale step {step}")
        np.testing.assert_array_equal(sf["amax_history"].cpu().numpy()[:, :2], orc.h_fwd[:, :2])
        np.testing.assert_array_equal(sb["scale"].cpu().numpy()[:1], orc.s_bwd[:1], err_msg=f"bwd scale step {step}")
        np.testing.assert_array_equal(sb["amax_history"].cpu().numpy()[:, :1], orc.h_bwd[:, :1])
        np.testing.assert_array_equal(sf["scale_inv"].cpu().numpy()[:2], orc.si_fwd[:2])


def test_linear_mxfp8_vs_oracle(te, dev):
    _, Format, MXFP8BlockScaling = _recipes()
    recipe = MXFP8BlockScaling(fp8_format=Format.E4M3)
    M, K, N = 64, 128, 96
    g = torch.Generator().manual_seed(8)
    lin = te.Linear(K, N, bias=True, params_dtype=torch.bfloat16, device=dev)
    with torch.no_grad():
        lin.weight.copy_((torch.randn(N, K, generator=g) * 0.05).to(torch.bfloat16))
        lin.bias.copy_(torch.randn(N, generator=g).to(torch.bfloat16))
    x = (torch.randn(M, K, generator=g) * torch.exp(torch.randn(M, 1, generator=g))).to(torch.bfloat16)
    dy = (torch.randn(M, N, generator=g) / 32).to(torch.bfloat16)
    xd = x.to(dev).requires_grad_(True)
    with te.fp8_autocast(enabled=True, fp8_recipe=recipe):
        y = lin(xd)
    y.backward(dy.to(dev))
    y_r, dx_r, dw_r, db_r = O.mxfp8_linear_fwd_bwd(bf16_bits(x), bf16_bits(lin.weight), bf16_bits(dy), bf16_bits(lin.bias))
    assert_gemm_close(_f(y), O.bf16_bits_to_f32(y_r), "mx y")
    assert_gemm_close(_f(xd.grad), O.bf16_bits_to_f32(dx_r), "mx dx")
    assert_gemm_close(_f(lin.weight.grad), O.bf16_bits_to_f32(dw_r), "mx dw")
    np.testing.assert_allclose(_f(lin.bias.grad), O.bf16_bits_to_f32(db_r), rtol=2 ** -7, atol=1e-3)


def test_linear_mxfp8_hybrid_vs_oracle(te, dev):
    """MXFP8BlockScaling(fp8_format=HYBRID): forward E4M3 x E4M3; grad_output quantised as E5M2 (row-wise blocks for dgrad, column-wise
    for wgrad) and the (E5M2, E4M3) block-scaled dgrad and wgrad GEMMs.  Built like test_linear_mxfp8_vs_oracle."""
    _, Format, MXFP8BlockScaling = _recipes()
    recipe = MXFP8BlockScaling(fp8_format=Format.HYBRID)
    M, K, N = 64, 128, 96
    g = torch.Generator().manual_seed(18)
    lin = te.Linear(K, N, bias=True, params_dtype=torch.bfloat16, device=dev)
    with torch.no_grad():
        lin.weight.copy_((torch.randn(N, K, generator=g) * 0.05).to(torch.bfloat16))
        lin.bias.copy_(torch.randn(N, generator=g).to(torch.bfloat16))
    x = (torch.randn(M, K, generator=g) * torch.exp(torch.randn(M, 1, generator=g))).to(torch.bfloat16)
    dy = (torch.randn(M, N, generator=g) * torch.exp(torch.randn(M, 1, generator=g) * 2) / 32).to(torch.bfloat16)
    xd = x.to(dev).requires_grad_(True)
    with te.fp8_autocast(enabled=True, fp8_recipe=recipe):
        y = lin(xd)
    y.backward(dy.to(dev))
    xb, wb, gb = bf16_bits(x), bf16_bits(lin.weight), bf16_bits(dy)
    fwd, bwd = O.E4M3, O.E5M2
    x8, xe = O.mxfp8_quantize_rowwise(xb, fwd)
    w8, we = O.mxfp8_quantize_rowwise(wb, fwd)
    y_r = O.gemm_mxfp8_tn(x8, xe, w8, we, fwd, fwd, bf16_bits(lin.bias))
    g8, ge = O.mxfp8_quantize_rowwise(gb, bwd)        # [M, N], blocks along N (dgrad contracts N)
    wt8, wte = O.mxfp8_quantize_colwise(wb, fwd)      # [K, N]
    dx_r = O.gemm_mxfp8_tn(g8, ge, wt8, wte, bwd, fwd)
    gt8, gte = O.mxfp8_quantize_colwise(gb, bwd)      # [N, M], blocks along M (wgrad contracts M)
    xt8, xte = O.mxfp8_quantize_colwise(xb, fwd)      # [K, M]
    dw_r = O.gemm_mxfp8_tn(gt8, gte, xt8, xte, bwd, fwd)
    # the E5M2 quantisation is what is new: it must differ from the E4M3 one, or the comparison below could not tell them apart
    assert not np.array_equal(g8, O.mxfp8_quantize_rowwise(gb, fwd)[0])
    db_r = O.f32_to_bf16_bits(O.bf16_bits_to_f32(gb).astype(np.float64).sum(axis=0).astype(np.float32))
    assert_gemm_close(_f(y), O.bf16_bits_to_f32(y_r), "mx hybrid y")
    assert_gemm_close(_f(xd.grad), O.bf16_bits_to_f32(dx_r), "mx hybrid dx")
    assert_gemm_close(_f(lin.weight.grad), O.bf16_bits_to_f32(dw_r), "mx hybrid dw")
    np.testing.assert_allclose(_f(lin.bias.grad), O.bf16_bits_to_f32(db_r), rtol=2 ** -7, atol=1e-3)


def test_layernorm_linear_split_weights_share_one_slot(te, dev):
    """q|k|v as three Parameters == one Linear on the concatenated weight (same single amax/scale slot)."""
    DelayedScaling, Format, _ = _recipes()
    recipe = DelayedScaling(fp8_format=Format.HYBRID, amax_history_len=4, amax_compute_algo="max")
    h, sizes = 128, {"query_": 64, "key_": 32, "value_": 32}
    torch.manual_seed(3)
    lnl = te.LayerNormLinear(h, 128, eps=1e-5, bias=False, normalization="RMSNorm", parameters_split=sizes,
                             params_dtype=torch.bfloat16, device=dev)
    with torch.no_grad():
        lnl.key_weight.mul_(5.0)
        lnl.layer_norm_weight.copy_(torch.rand(h) + 0.5)
    ref = te.Linear(h, 128, bias=False, params_dtype=torch.bfloat16, device=dev)
    with torch.no_grad():
        ref.weight.copy_(torch.cat([lnl.query_weight, lnl.key_weight, lnl.value_weight], 0))
    x = torch.randn(4, 16, h, device=dev, dtype=torch.bfloat16)
    for _ in range(2):
        xa = x.clone().requires_grad_(True)
        xb = x.clone().requires_grad_(True)
        with te.fp8_autocast(enabled=True, fp8_recipe=recipe):
            ya = lnl(xa)
        with te.fp8_autocast(enabled=True, fp8_recipe=recipe):
            yb = ref(torch.nn.functional.rms_norm(xb, (h,), lnl.layer_norm_weight, 1e-5))
        assert torch.equal(ya, yb)
        gy = torch.randn_like(ya) / 16
        ya.backward(gy)
        yb.backward(gy)
        assert torch.equal(xa.grad, xb.grad)
        gcat = torch.cat([lnl.query_weight.grad, lnl.key_weight.grad, lnl.value_weight.grad], 0)
        assert torch.equal(gcat, ref.weight.grad)
        for p in list(lnl.parameters()) + list(ref.parameters()):
            p.grad = None
    assert torch.equal(lnl._meta_fwd.state()["scale"], ref._meta_fwd.state()["scale"])


def test_layernorm_mlp_matches_two_linears_and_bf16(te, dev):
    DelayedScaling, Format, _ = _recipes()
    recipe = DelayedScaling(fp8_format=Format.E4M3, amax_history_len=16, amax_compute_algo="max")
    h, f = 128, 256
    torch.manual_seed(5)
    mlp = te.LayerNormMLP(h, f, eps=1e-5, normalization="RMSNorm", activation="swiglu", params_dtype=torch.bfloat16, device=dev)
    with torch.no_grad():
        mlp.fc1_bias.normal_(0, 0.1)
        mlp.fc2_bias.normal_(0, 0.1)
    assert mlp.fc1_weight.shape == (2 * f, h) and mlp.fc2_weight.shape == (h, f)
    x = torch.randn(2, 32, h, device=dev, dtype=torch.bfloat16)
    # warm the scales (first iteration quantises with scale 1)
    for _ in range(2):
        with te.fp8_autocast(enabled=True, fp8_recipe=recipe):
            y8 = mlp(x.clone().requires_grad_(True))
        y8.sum().backward()
    xr = x.clone().requires_grad_(True)
    with te.fp8_autocast(enabled=True, fp8_recipe=recipe):
        y8 = mlp(xr)
    yb = mlp(x)  # outside autocast: plain bf16 path of the same module
    rel = (y8.float() - yb.float()).norm() / yb.float().norm()
    assert rel < 0.08, f"fp8 vs bf16 relative error {rel:.4f}"
    y8.backward(torch.randn_like(y8) / 16)
    for p in (mlp.fc1_weight, mlp.fc2_weight, mlp.fc1_bias, mlp.fc2_bias, mlp.layer_norm_weight):
        assert p.grad is not None and torch.isfinite(p.grad.float()).all()
    assert mlp._meta_fwd.n == 6 and mlp._meta_bwd.n == 4  # G = 2 (SURVEY Appendix A "Slots")


def test_autocast_state_machine(te, dev):
    """Outermost exit updates all forward slots once; nested exits do not; no update under no_grad; backward
    update fires after the first module's backward; disabled autocast runs bf16."""
    DelayedScaling, Format, _ = _recipes()
    from llm_fp8_amd.pytorch.fp8 import FP8GlobalStateManager as S
    r_in = DelayedScaling(fp8_format=Format.HYBRID, amax_history_len=4, amax_compute_algo="max")
    r_out = DelayedScaling(fp8_format=Format.HYBRID, amax_history_len=8, amax_compute_algo="most_recent")
    a = te.Linear(64, 64, bias=False, params_dtype=torch.bfloat16, device=dev)
    b = te.Linear(64, 64, bias=False, params_dtype=torch.bfloat16, device=dev)
    x = torch.randn(16, 64, device=dev, dtype=torch.bfloat16, requires_grad=True)
    with te.fp8_autocast(enabled=True, fp8_recipe=r_out):
        with te.fp8_autocast(enabled=True, fp8_recipe=r_in):
            h = a(x)
            assert S.FP8_AUTOCAST_DEPTH == 2
        # inner exit: nothing updated yet, amax still in row 0
        assert a._meta_fwd.state()["amax_history"][0, 0].item() > 0
        assert a._meta_fwd.state()["scale"][0].item() == 1.0
        y = b(h)
    assert S.FP8_AUTOCAST_DEPTH == 0
    sa, sb = a._meta_fwd.state(), b._meta_fwd.state()
    assert sa["amax_history"].shape[0] == 4 and sb["amax_history"].shape[0] == 8  # each module under its own recipe
    assert sa["scale"][0].item() > 1.0 and sb["scale"][0].item() > 1.0 and sa["amax_history"][0].abs().sum().item() == 0
    # backward: module `a` was the first FP8 module -> bwd update happens in its backward (the last one)
    assert b._meta_bwd.state()["scale"][0].item() == 1.0
    y.sum().backward()
    assert b._meta_bwd.state()["scale"][0].item() > 1.0 and a._meta_bwd.state()["scale"][0].item() > 1.0
    # no_grad (the reference's eval loop, train_fp8.py:323-327): quantise with current scales, never update
    before = a._meta_fwd.state()
    with torch.no_grad():
        with te.fp8_autocast(enabled=True, fp8_recipe=r_in):
            a(x)
    after = a._meta_fwd.state()
    assert torch.equal(before["scale"], after["scale"]) and after["amax_history"][0, 0].item() > 0
    # enabled=False -> bf16 path, bit-identical to F.linear
    with te.fp8_autocast(enabled=False):
        yb = a(x)
    assert torch.equal(yb, torch.nn.functional.linear(x, a.weight))


def test_extra_state_roundtrip(te, dev):
    DelayedScaling, Format, _ = _recipes()
    r = DelayedScaling(fp8_format=Format.HYBRID, amax_history_len=4, amax_compute_algo="max")
    a = te.Linear(64, 32, params_dtype=torch.bfloat16, device=dev)
    x = torch.randn(16, 64, device=dev, dtype=torch.bfloat16, requires_grad=True)
    with te.fp8_autocast(enabled=True, fp8_recipe=r):
        a(x).sum().backward()
    sd = a.state_dict()
    assert "_extra_state" in sd
    b = te.Linear(64, 32, params_dtype=torch.bfloat16, device=dev)
    b.load_state_dict(sd)
    with te.fp8_autocast(enabled=True, fp8_recipe=r):
        yb = b(x)
    with te.fp8_autocast(enabled=True, fp8_recipe=r):
        ya = a(x)
    assert torch.equal(ya, yb)


def _tiny_cfg():
    from llm_fp8_amd import llama
    return llama.llama_config("llama-3.2-1b", num_hidden_layers=2, hidden_size=256, intermediate_size=512,
                              num_attention_heads=4, num_key_value_heads=2, head_dim=64, vocab_size=1024,
                              max_position_embeddings=256, rope_theta=10000.0)


@pytest.mark.parametrize("scenario", ["default", "hybrid", "mxfp8"])
def test_te_decoder_layer_vs_hf_bf16_layer(te, dev, scenario):
    """The TE-shaped layer with replace_params-mapped weights tracks HF's bf16 LlamaDecoderLayer
    (rope_theta set to TE's base 10000 so both use the same RoPE)."""
    from transformers.models.llama.modeling_llama import LlamaForCausalLM
    from llm_fp8_amd import llama
    cfg = _tiny_cfg()
    torch.manual_seed(0)
    hf = LlamaForCausalLM(cfg).to(dev).to(torch.bfloat16)
    tem = llama.TELlamaForCausalLM.from_hf_state_dict(hf.state_dict(), cfg, scenario).to(dev)
    names = dict(tem.named_parameters())
    assert "model.layers.0.self_attention.layernorm_qkv.query_weight" in names
    assert "model.layers.1.layernorm_mlp.fc1_weight" in names and "model.layers.1.layernorm_mlp.fc2_bias" in names
    f = cfg.intermediate_size
    assert torch.equal(names["model.layers.0.layernorm_mlp.fc1_weight"][:f], hf.model.layers[0].mlp.gate_proj.weight)
    assert torch.equal(names["model.layers.0.layernorm_mlp.fc1_weight"][f:], hf.model.layers[0].mlp.up_proj.weight)
    ids = torch.randint(0, cfg.vocab_size, (2, 64), device=dev)
    hf.train(); tem.train()
    for _ in range(3):  # let delayed scaling settle
        out = tem(input_ids=ids, labels=ids)
        out.loss.backward()
        tem.zero_grad()
    ref = hf(input_ids=ids, labels=ids)
    out = tem(input_ids=ids, labels=ids)
    rel = (out.logits.float() - ref.logits.float()).norm() / ref.logits.float().norm()
    assert rel < 0.08, f"{scenario}: logits relative error {rel:.4f}"
    assert abs(out.loss.item() - ref.loss.item()) < 0.05 * abs(ref.loss.item())
    out.loss.backward(); ref.loss.backward()
    g8 = tem.model.layers[0].self_attention.proj.weight.grad.float()
    gb = hf.model.layers[0].self_attn.o_proj.weight.grad.float()
    grel = (g8 - gb).norm() / gb.norm()
    assert grel < 0.25, f"{scenario}: o_proj grad relative error {grel:.4f}"


@pytest.mark.parametrize("scenario,expected", [
    ("default", {"cast_amax": 12, "gemm_fp8": 12, "swiglu_cast": 1, "dswiglu_cast": 1}),
    ("mxfp8", {"mxfp8_quantize": 14, "gemm_mxfp8": 12})])
def test_decoder_layer_step_launch_counts(te, dev, scenario, expected):
    """Launches per kind of one forward + backward of a decoder layer of the model above: the host
    code around the GEMM sites serves both recipes, and a change to it must neither add nor drop a launch for either."""
    from transformers.models.llama.modeling_llama import LlamaForCausalLM
    from llm_fp8_amd import llama
    from llm_fp8_amd.pytorch.profiler import KernelTimer
    cfg = _tiny_cfg()
    torch.manual_seed(0)
    tem = llama.TELlamaForCausalLM.from_hf_state_dict(LlamaForCausalLM(cfg).to(dev).to(torch.bfloat16).state_dict(), cfg, scenario).to(dev)
    ids = torch.randint(0, cfg.vocab_size, (2, 64), device=dev)
    tem.train()
    for _ in range(3):
        tem(input_ids=ids, labels=ids).loss.backward()
        tem.zero_grad()
    x = torch.randn(2, 64, cfg.hidden_size, device=dev, dtype=torch.bfloat16, requires_grad=True)
    with KernelTimer().install() as timer:
        y = tem.model.layers[0](x)
        y.backward(torch.randn_like(y) / 16)
    torch.cuda.synchronize()
    assert {k: v["launches"] for k, v in timer.summarize().items()} == expected


@pytest.mark.parametrize("use_te,scenario", [(True, "default"), (True, "mxfp8"), (False, "default")])
def test_train_steps_run_and_update_once_per_step(te, dev, use_te, scenario):
    from llm_fp8_amd import llama, train
    from llm_fp8_amd.pytorch.fp8 import FP8GlobalStateManager as S
    cfg = train.TrainingConfig(model_name="llama-3.2-1b", batch_size=2, max_seq_length=64, mixed_precision="fp8",
                               fp8_scenario=scenario, use_te=use_te, num_hidden_layers=2, vocab_size=2048,
                               learning_rate=1e-3, num_warmup_steps=0)
    torch.manual_seed(0)
    model = train.prepare_model(train.create_model(cfg, dev), cfg)
    lm_head = model.lm_head
    assert isinstance(lm_head, te.Linear) and lm_head.weight is model.model.embed_tokens.weight  # tie kept
    if not use_te:
        assert isinstance(model.model.layers[0].self_attn.q_proj, te.Linear)
    opt, sched = train.create_optimizer(model, cfg)
    model.train()
    batch = train.synthetic_batch(cfg, 2048, dev)
    losses = []
    for step in range(6):
        losses.append(train.train_step(model, batch, opt, sched, cfg).item())
    assert all(np.isfinite(losses)) and losses[-1] < losses[0], losses
    # exactly one forward update per step: the lm_head history (outer recipe) has rolled 6 times
    hist = lm_head._meta_fwd.state()["amax_history"]
    # row 0 is the slot the NEXT forward fills; the input slot is empty between steps.  The weight slot (column 1) already
    # holds the amax of the updated weight when the optimiser keeps the FP8 copies current (module.WeightSink): it deposits
    # the value the next forward's cast would have
    assert hist[0, 0].item() == 0 and hist[0, 2:].abs().sum().item() == 0
    from llm_fp8_amd.pytorch.module import weight_sinks_enabled
    if not weight_sinks_enabled():
        assert hist[0, 1].item() == 0
    n_nonzero = int((hist[:, 0] > 0).sum().item())
    assert n_nonzero == min(6, hist.shape[0] - 1), n_nonzero
    model.eval()
    with torch.no_grad():
        out = model(**batch)
    assert torch.isfinite(out.loss)


def test_fused_mx_mlp_matches_unfused(te, dev):
    """MXFP8: fused norm/SwiGLU quantisers vs the unfused module path (torch rms_norm / silu*mul then plain quantise)."""
    _, Format, MXFP8BlockScaling = _recipes()
    recipe = MXFP8BlockScaling(fp8_format=Format.E4M3)
    h, f = 512, 1024
    torch.manual_seed(12)
    a = te.LayerNormMLP(h, f, normalization="RMSNorm", activation="swiglu", params_dtype=torch.bfloat16, device=dev)
    b = te.LayerNormMLP(h, f, normalization="RMSNorm", activation="swiglu", params_dtype=torch.bfloat16, device=dev)
    with torch.no_grad():
        a.fc1_bias.normal_(0, 0.1); a.fc2_bias.normal_(0, 0.1); a.layer_norm_weight.copy_(torch.linspace(0.5, 1.5, h))
    b.load_state_dict(a.state_dict())
    b.fused_swiglu = False
    b.fused_norm = False
    x = torch.randn(2, 64, h, device=dev, dtype=torch.bfloat16)
    xa, xb = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
    with te.fp8_autocast(enabled=True, fp8_recipe=recipe):
        ya, yb = a(xa), b(xb)
    gy = torch.randn_like(ya) / 16
    ya.backward(gy); yb.backward(gy)
    for got, ref, name in ((ya, yb, "y"), (xa.grad, xb.grad, "dx"), (a.fc1_weight.grad, b.fc1_weight.grad, "dw1"),
                           (a.fc2_weight.grad, b.fc2_weight.grad, "dw2"), (a.fc1_bias.grad, b.fc1_bias.grad, "db1"),
                           (a.layer_norm_weight.grad, b.layer_norm_weight.grad, "dgamma")):
        rel = (got.float() - ref.float()).norm() / ref.float().norm()
        assert rel < 0.05, f"{name}: rel {rel:.4f}"  # two FP8 quantisations of values that differ by a bf16 rounding


def test_fused_swiglu_mlp_matches_unfused(te, dev):
    """K10 fusion (SwiGLU + cast in one kernel, bf16 activation never materialised) vs the two-Linear path:
    same scales and amaxes up to the bf16 rounding of the activation the unfused path inserts."""
    DelayedScaling, Format, _ = _recipes()
    recipe = DelayedScaling(fp8_format=Format.HYBRID, amax_history_len=4, amax_compute_algo="max")
    h, f = 256, 512
    torch.manual_seed(11)
    a = te.LayerNormMLP(h, f, normalization="RMSNorm", activation="swiglu", params_dtype=torch.bfloat16, device=dev)
    b = te.LayerNormMLP(h, f, normalization="RMSNorm", activation="swiglu", params_dtype=torch.bfloat16, device=dev)
    with torch.no_grad():
        a.fc1_bias.normal_(0, 0.1); a.fc2_bias.normal_(0, 0.1)
    b.load_state_dict(a.state_dict())
    b.fused_swiglu = False
    x = torch.randn(4, 64, h, device=dev, dtype=torch.bfloat16)
    for step in range(3):
        xa, xb = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
        with te.fp8_autocast(enabled=True, fp8_recipe=recipe):
            ya = a(xa)
        with te.fp8_autocast(enabled=True, fp8_recipe=recipe):
            yb = b(xb)
        gy = torch.randn_like(ya) / 16
        ya.backward(gy); yb.backward(gy)
        for got, ref, name in ((ya, yb, "y"), (xa.grad, xb.grad, "dx"), (a.fc1_weight.grad, b.fc1_weight.grad, "dw1"),
                               (a.fc2_weight.grad, b.fc2_weight.grad, "dw2"), (a.fc1_bias.grad, b.fc1_bias.grad, "db1"),
                               (a.fc2_bias.grad, b.fc2_bias.grad, "db2")):
            rel = (got.float() - ref.float()).norm() / ref.float().norm()
            assert rel < 0.03, f"step {step} {name}: rel {rel:.4f}"
        for p in list(a.parameters()) + list(b.parameters()):
            p.grad = None
    sa, sb = a._meta_fwd.state()["scale"], b._meta_fwd.state()["scale"]
    assert torch.equal(sa[:2], sb[:2])  # fc1 input / weight amaxes are identical
    assert torch.allclose(sa[3:5], sb[3:5], rtol=0.02)  # fc2 input amax: fp32 act vs bf16-rounded act


def test_clipped_adamw_matches_torch_clip_plus_fused_adamw(dev):
    """ClippedAdamW == clip_grad_norm_(1.0) + torch.optim.AdamW(fused=True) (train_fp8.py:288-291) up to the bf16 rounding
    of the rescaled gradient that torch's in-place clip inserts."""
    from llm_fp8_amd.optim import ClippedAdamW
    torch.manual_seed(0)
    shapes = [(1024, 512), (333,), (7, 9), (4096, 1024)]
    pa = [torch.nn.Parameter(torch.randn(s, device=dev).to(torch.bfloat16)) for s in shapes]
    pb = [torch.nn.Parameter(p.detach().clone()) for p in pa]
    oa = ClippedAdamW(pa, lr=1e-2, max_grad_norm=1.0)
    ob = torch.optim.AdamW(pb, lr=1e-2, fused=True)
    for step in range(4):
        for x, y in zip(pa, pb):
            g = (torch.randn_like(x, dtype=torch.float32) * (0.01 if step == 3 else 1.0)).to(torch.bfloat16)  # last step: norm < 1, no clipping
            x.grad, y.grad = g.clone(), g.clone()
        ref_norm = torch.nn.utils.clip_grad_norm_(pb, 1.0)
        ob.step()
        oa.step()
        assert abs(oa.last_grad_norm.item() - ref_norm.item()) <= 2e-3 * ref_norm.item()
        for x, y in zip(pa, pb):
            assert torch.isfinite(x).all()
            d = (x.float() - y.float()).abs()
            assert (d <= 2.0 ** -6 * y.float().abs() + 1e-3).all(), f"step {step}: max diff {d.max().item()}"  # <= 1-2 bf16 ulps
    assert (torch.cat([(x.float() - y.float()).abs().reshape(-1) for x, y in zip(pa, pb)]) == 0).float().mean() > 0.9


def test_fused_rmsnorm_paths_match_unfused(te, dev):
    """K9 (RMSNorm fused into the FP8 cast + HIP backward) vs torch rms_norm followed by the plain cast: the fused path
    skips the bf16 rounding of the normalised activation, everything else is identical."""
    DelayedScaling, Format, _ = _recipes()
    recipe = DelayedScaling(fp8_format=Format.HYBRID, amax_history_len=4, amax_compute_algo="max")
    h = 512
    torch.manual_seed(21)
    mods = []
    for fused in (True, False):
        lnl = te.LayerNormLinear(h, 768, eps=1e-5, bias=False, normalization="RMSNorm", parameters_split={"query_": 512, "key_": 128, "value_": 128},
                                 params_dtype=torch.bfloat16, device=dev)
        mlp = te.LayerNormMLP(h, 1024, normalization="RMSNorm", activation="swiglu", params_dtype=torch.bfloat16, device=dev)
        lnl.fused_norm = mlp.fused_norm = fused
        mods.append((lnl, mlp))
    mods[1][0].load_state_dict(mods[0][0].state_dict()); mods[1][1].load_state_dict(mods[0][1].state_dict())
    with torch.no_grad():
        for lnl, mlp in mods:
            lnl.layer_norm_weight.copy_(torch.linspace(0.5, 1.5, h)); mlp.layer_norm_weight.copy_(torch.linspace(1.5, 0.5, h))
    x = torch.randn(2, 64, h, device=dev, dtype=torch.bfloat16)
    for step in range(3):
        outs = []
        for lnl, mlp in mods:
            xi = x.clone().requires_grad_(True)
            with te.fp8_autocast(enabled=True, fp8_recipe=recipe):
                y = lnl(xi)
                z = mlp(xi)
            (y.float().pow(2).mean() + z.float().pow(2).mean()).backward()
            outs.append((y, z, xi.grad, lnl.layer_norm_weight.grad.clone(), mlp.layer_norm_weight.grad.clone(), lnl.key_weight.grad.clone()))
            for p in list(lnl.parameters()) + list(mlp.parameters()):
                p.grad = None
        for a, b, name in zip(outs[0], outs[1], ("y", "z", "dx", "dgamma_qkv", "dgamma_mlp", "dw_k")):
            rel = (a.float() - b.float()).norm() / b.float().norm()
            if step > 0:  # step 0 quantises with scale 1 (tiny gradients land in the FP8 subnormals): not comparable
                assert rel < 0.05, f"step {step} {name}: rel {rel:.4f}"  # FP8 re-quantisation noise of one bf16-ulp input change
    assert torch.equal(mods[0][0]._meta_fwd.state()["scale"][1:2], mods[1][0]._meta_fwd.state()["scale"][1:2])


def test_fused_causal_lm_loss_matches_hf(dev):
    from transformers.loss.loss_utils import ForCausalLMLoss
    from llm_fp8_amd.loss import causal_lm_loss
    torch.manual_seed(0)
    B, S, V = 3, 40, 4096
    logits = (torch.randn(B, S, V, device=dev) * 3).to(torch.bfloat16)
    labels = torch.randint(0, V, (B, S), device=dev)
    labels[0, 5:9] = -100
    la = logits.clone().requires_grad_(True)
    lb = logits.clone().requires_grad_(True)
    a = causal_lm_loss(la, labels, V)
    b = ForCausalLMLoss(lb, labels, V)
    assert abs(a.item() - b.item()) <= 2e-4 * abs(b.item())
    (a * 2.0).backward()
    (b * 2.0).backward()
    d = (la.grad.float() - lb.grad.float()).abs()
    assert (d <= 2.0 ** -7 * lb.grad.float().abs() + 1e-7).all()
    assert la.grad[0, 4:8].abs().sum().item() == 0  # rows whose shifted label is ignored get no gradient


@pytest.mark.parametrize("kind", ["linear", "mlp", "mx"])
def test_is_first_microbatch_reuses_fp8_weights(te, dev, kind):
    """TE's micro-batch protocol: is_first_microbatch=True casts and keeps the FP8 weights,
    False reuses them -- no weight-cast launches -- and gives the same result as re-casting unchanged weights."""
    from llm_fp8_amd.pytorch.profiler import KernelTimer
    DelayedScaling, Format, MXFP8BlockScaling = _recipes()
    recipe = MXFP8BlockScaling() if kind == "mx" else DelayedScaling(fp8_format=Format.HYBRID, amax_history_len=4, amax_compute_algo="max")
    torch.manual_seed(2)
    if kind == "mlp":
        mod = te.LayerNormMLP(256, 512, normalization="RMSNorm", activation="swiglu", params_dtype=torch.bfloat16, device=dev)
    else:
        mod = te.Linear(256, 512, params_dtype=torch.bfloat16, device=dev)
    x = torch.randn(64, 256, device=dev, dtype=torch.bfloat16, requires_grad=True)

    def run(flag):
        t = KernelTimer()
        with t.install():
            with te.fp8_autocast(enabled=True, fp8_recipe=recipe):
                y = mod(x, is_first_microbatch=flag)
            y.float().pow(2).mean().backward()
        torch.cuda.synchronize()
        s = t.summarize()
        casts = sum(v["launches"] for k, v in s.items() if k in ("cast_amax", "mxfp8_quantize", "norm_cast"))
        return y.detach().clone(), casts

    run(None)  # settle the delayed scales a little
    y_first, c_first = run(True)
    y_reuse, c_reuse = run(False)
    y_recast, c_recast = run(None)
    n_w = 2 if kind == "mlp" else 1
    assert c_reuse == c_first - n_w and c_recast == c_first
    rel = (y_reuse.float() - y_recast.float()).norm() / y_recast.float().norm()
    assert rel < 0.02  # weights unchanged: only the (delayed) scale the weights were quantised with differs
    assert torch.isfinite(mod.fc1_weight.grad if kind == "mlp" else mod.weight.grad).all()


def test_dot_product_attention_flash_path_matches_sdpa(te, dev):
    """DotProductAttention on the hand-written kernels vs the torch SDPA route (same module, flash path disabled)."""
    from llm_fp8_amd.pytorch import attention as A
    B, S, H, G, D = 2, 256, 6, 2, 128
    core = A.DotProductAttention(H, D, G, attention_dropout=0.0, attn_mask_type="causal", qkv_format="bshd")
    torch.manual_seed(3)
    q, k, v = (torch.randn(B, S, n, D, device=dev, dtype=torch.bfloat16, requires_grad=True) for n in (H, G, G))
    assert A._flash_ok(q, k, v, True, 0.0)
    o = core(q, k, v)
    go = torch.randn_like(o) / 4
    o.backward(go)
    got = (o.detach(), q.grad.clone(), k.grad.clone(), v.grad.clone())
    q.grad = k.grad = v.grad = None
    saved = A._flash_ok
    A._flash_ok = lambda *a, **kw: False
    try:
        o2 = core(q, k, v)
        o2.backward(go)
    finally:
        A._flash_ok = saved
    for a, b, name in zip(got, (o2.detach(), q.grad, k.grad, v.grad), ("o", "dq", "dk", "dv")):
        rel = ((a.float() - b.float()).norm() / b.float().norm()).item()
        assert rel < 1e-2, f"{name}: {rel:.4g}"


@pytest.mark.parametrize("scenario", ["default", "mxfp8"])
def test_decoder_layer_skip_fusion_matches_plain_residual(te, dev, scenario):
    """The `_with_skip` route (residual gradient added inside the RMSNorm-backward kernel) against plain `h + f(h)`."""
    from llm_fp8_amd import llama
    cfg = llama.llama_config("llama-3.2-1b", num_hidden_layers=1, hidden_size=512, intermediate_size=1024, num_attention_heads=4,
                             num_key_value_heads=2, head_dim=128, vocab_size=1024, max_position_embeddings=256)
    torch.manual_seed(5)
    prev = torch.get_default_dtype()
    torch.set_default_dtype(torch.bfloat16)
    try:
        with torch.device(dev):
            layer = llama.decoder_layer_cls(scenario)(cfg, 0)
    finally:
        torch.set_default_dtype(prev)
    layer.to(dev).train()
    x = torch.randn(2, 128, cfg.hidden_size, device=dev, dtype=torch.bfloat16)

    def plain(h):
        with te.fp8_autocast(enabled=True, fp8_recipe=layer.attn_recipe):
            h = h + layer.self_attention(h, rotary_pos_emb=layer.te_rope_emb)
        with te.fp8_autocast(enabled=True, fp8_recipe=layer.mlp_recipe):
            return h + layer.layernorm_mlp(h)

    for _ in range(3):  # settle the delayed-scaling state: same input every time, so both routes then see the same scales
        xi = x.clone().requires_grad_(True)
        layer(xi).float().square().mean().backward()
        layer.zero_grad()
    outs = []
    for fn in (layer, plain):
        xi = x.clone().requires_grad_(True)
        y = fn(xi)
        y.float().square().mean().backward()
        outs.append((y.detach(), xi.grad.clone(), layer.self_attention.layernorm_qkv.layer_norm_weight.grad.clone(),
                     layer.layernorm_mlp.fc1_weight.grad.clone()))
        layer.zero_grad()
    for a, b, name in zip(outs[0], outs[1], ("y", "dx", "dgamma", "dw1")):
        rel = ((a.float() - b.float()).norm() / b.float().norm()).item()
        assert rel < (3e-2 if name == "dgamma" else 1e-2), f"{name}: {rel:.4g}"  # only the rounding of dx + dskip moves (and what it re-quantises to upstream)


@pytest.mark.parametrize("scenario", ["default", "mxfp8"])
def test_grad_output_handoffs_are_bitwise_the_unfused_path(te, dev, scenario, monkeypatch):
    """module.DyHandoff (RoPE backward -> q|k|v projection, cross-entropy backward -> lm_head: grad_output delivered in FP8 by
    the op that produces it, placeholder through autograd) against the ordinary route: same losses, weights and amax
    histories after 3 optimiser steps, bit for bit."""
    from llm_fp8_amd import train
    from llm_fp8_amd.pytorch.fp8 import FP8GlobalStateManager as G
    from llm_fp8_amd.pytorch import ops as _ops

    def run(disable):
        G.reset()
        if disable:
            monkeypatch.setenv("LLM_FP8_AMD_NO_DY_HANDOFF", "1")
        else:
            monkeypatch.delenv("LLM_FP8_AMD_NO_DY_HANDOFF", raising=False)
        calls = {"rope": 0}
        name = "mxfp8_rope_bwd_quantize" if scenario == "mxfp8" else "rope_qkv_backward_cast"
        orig = getattr(_ops, name)
        monkeypatch.setattr(_ops, name, lambda *a, **k: (calls.__setitem__("rope", calls["rope"] + 1), orig(*a, **k))[1])
        cfg = train.TrainingConfig(model_name="llama-3.2-3b", batch_size=2, max_seq_length=128, mixed_precision="fp8",
                                   fp8_scenario=scenario, use_te=True, sharding_mode="none", num_hidden_layers=2, vocab_size=2048,
                                   learning_rate=1e-3, num_warmup_steps=0)
        torch.manual_seed(21)
        device = torch.device(dev)
        model = train.prepare_model(train.create_model(cfg, device), cfg)
        opt, sched = train.create_optimizer(model, cfg)
        model.train()
        gen = torch.Generator(device=device).manual_seed(8)
        losses = [train.train_step(model, train.synthetic_batch(cfg, 2048, device, gen), opt, sched, cfg).item() for _ in range(3)]
        hist = torch.cat([a.hist[:, :a.used].reshape(-1) for a in G._arenas.values()]).clone()
        flat = torch.cat([p.detach().reshape(-1).view(torch.int16) for p in model.parameters()]).clone()
        monkeypatch.setattr(_ops, name, orig)
        return losses, hist, flat, calls["rope"]

    try:
        l1, h1, w1, n1 = run(False)
        l0, h0, w0, n0 = run(True)
    finally:
        G.reset()
    # 2 layers x 3 steps through the fused RoPE route (head_dim 128), in its delayed-scaling or its MXFP8 form
    assert n0 == 0 and n1 == 6, (n1, n0)
    assert l1 == l0, (l1, l0)
    assert torch.equal(h1, h0) and torch.equal(w1, w0)


@pytest.mark.parametrize("scenario,accum", [("default", 1), ("hybrid", 1), ("default", 2)])
def test_optimizer_weight_cast_handoff_is_bitwise_the_forward_cast(te, dev, scenario, accum, monkeypatch):
    """module.WeightSink + mi_adamw_cast_bf16_multi: the optimiser emits the FP8 weights (and their amax) of the next forward;
    against the ordinary route (every forward casts its weights): same losses, weights, Adam moments and amax histories after 4
    optimiser steps, bit for bit -- and the forward really stops casting weights.  accum = 2: the second micro-batch of a
    window sees a NEWER scale than the optimiser used, so it must fall back to casting."""
    from llm_fp8_amd import train
    from llm_fp8_amd.pytorch.fp8 import FP8GlobalStateManager as G
    from llm_fp8_amd.pytorch import ops as _ops

    def run(disable):
        G.reset()
        if disable:
            monkeypatch.setenv("LLM_FP8_AMD_NO_OPT_WCAST", "1")
        else:
            monkeypatch.delenv("LLM_FP8_AMD_NO_OPT_WCAST", raising=False)
        calls = {"n": 0}
        orig = _ops.cast_amax

        def counting(x, *a, **k):
            if isinstance(x, torch.nn.Parameter) or getattr(x, "_is_param", False) or x.requires_grad and x.is_leaf:
                calls["n"] += 1
            return orig(x, *a, **k)

        monkeypatch.setattr(_ops, "cast_amax", counting)
        cfg = train.TrainingConfig(model_name="llama-3.2-3b", batch_size=2, max_seq_length=128, mixed_precision="fp8",
                                   fp8_scenario=scenario, use_te=True, sharding_mode="none", num_hidden_layers=2, vocab_size=2048,
                                   learning_rate=1e-3, num_warmup_steps=0)
        torch.manual_seed(23)
        device = torch.device(dev)
        model = train.prepare_model(train.create_model(cfg, device), cfg)
        opt, sched = train.create_optimizer(model, cfg)
        model.train()
        gen = torch.Generator(device=device).manual_seed(9)
        losses = []
        for _ in range(4):
            mbs = [train.synthetic_batch(cfg, 2048, device, gen) for _ in range(accum)]
            losses.append(train.train_step(model, mbs if accum > 1 else mbs[0], opt, sched, cfg).item())
        # an evaluation pass in between must not disturb anything (it quantises with the current scales and casts for itself)
        model.eval()
        with torch.no_grad():
            ev = model(**train.synthetic_batch(cfg, 2048, device, gen)).loss.item()
        model.train()
        losses.append(train.train_step(model, train.synthetic_batch(cfg, 2048, device, gen), opt, sched, cfg).item())
        # the optimiser deposits amax(w) into history row 0 right away, the ordinary route at the next forward's weight cast:
        # compare the state at a common point -- after one more training-mode forward (its exit rolls the histories)
        losses.append(model(**train.synthetic_batch(cfg, 2048, device, gen)).loss.item())
        hist = torch.cat([torch.cat([a.hist[:, :a.used].reshape(-1), a.scale[:a.used]]) for a in G._arenas.values()]).clone()
        flat = torch.cat([p.detach().reshape(-1).view(torch.int16) for p in model.parameters()]).clone()
        mom = torch.cat([opt.state[p]["exp_avg_sq"].reshape(-1).view(torch.int16) for p in model.parameters() if p in opt.state]).clone()
        monkeypatch.setattr(_ops, "cast_amax", orig)
        return losses, ev, hist, flat, mom, calls["n"]

    try:
        l1, e1, h1, w1, m1, n1 = run(False)
        l0, e0, h0, w0, m0, n0 = run(True)
    finally:
        G.reset()
    assert l1 == l0 and e1 == e0, (l1, l0)
    assert torch.equal(h1, h0) and torch.equal(w1, w0) and torch.equal(m1, m0)
    assert n1 < n0, (n1, n0)   # weight casts really disappeared from the forwards that follow an optimiser step


@pytest.mark.parametrize("accum", [1, 2])
def test_optimizer_mxfp8_weight_handoff_is_bitwise_the_forward_quantiser(te, dev, accum, monkeypatch):
    """module.MXWeightSink + mi_adamw_mxcast_bf16_multi: under MXFP8 the optimiser emits the row- and column-block copies (and
    E8M0 scales) of every decoder weight for the next forward.  Against the ordinary route (every forward quantises its weights):
    same losses, weights and Adam moments after 5 optimiser steps and an evaluation pass in between, bit for bit -- and the
    forwards that follow an optimiser step stop quantising weights."""
    from llm_fp8_amd import train
    from llm_fp8_amd.pytorch.fp8 import FP8GlobalStateManager as G
    from llm_fp8_amd.pytorch import ops as _ops

    def run(disable):
        G.reset()
        if disable:
            monkeypatch.setenv("LLM_FP8_AMD_NO_OPT_WCAST", "1")
        else:
            monkeypatch.delenv("LLM_FP8_AMD_NO_OPT_WCAST", raising=False)
        calls = {"n": 0}
        orig = _ops.mxfp8_quantize

        def counting(x, *a, **k):
            if isinstance(x, torch.nn.Parameter):
                calls["n"] += 1
            return orig(x, *a, **k)

        monkeypatch.setattr(_ops, "mxfp8_quantize", counting)
        cfg = train.TrainingConfig(model_name="llama-3.2-3b", batch_size=2, max_seq_length=128, mixed_precision="fp8",
                                   fp8_scenario="mxfp8", use_te=True, sharding_mode="none", num_hidden_layers=2, vocab_size=2048,
                                   learning_rate=1e-3, num_warmup_steps=0)
        torch.manual_seed(23)
        device = torch.device(dev)
        model = train.prepare_model(train.create_model(cfg, device), cfg)
        opt, sched = train.create_optimizer(model, cfg)
        model.train()
        gen = torch.Generator(device=device).manual_seed(9)
        losses = []
        for _ in range(4):
            mbs = [train.synthetic_batch(cfg, 2048, device, gen) for _ in range(accum)]
            losses.append(train.train_step(model, mbs if accum > 1 else mbs[0], opt, sched, cfg).item())
        model.eval()
        with torch.no_grad():
            ev = model(**train.synthetic_batch(cfg, 2048, device, gen)).loss.item()
        model.train()
        losses.append(train.train_step(model, train.synthetic_batch(cfg, 2048, device, gen), opt, sched, cfg).item())
        flat = torch.cat([p.detach().reshape(-1).view(torch.int16) for p in model.parameters()]).clone()
        mom = torch.cat([opt.state[p]["exp_avg_sq"].reshape(-1).view(torch.int16) for p in model.parameters() if p in opt.state]).clone()
        monkeypatch.setattr(_ops, "mxfp8_quantize", orig)
        return losses, ev, flat, mom, calls["n"]

    try:
        l1, e1, w1, m1, n1 = run(False)
        l0, e0, w0, m0, n0 = run(True)
    finally:
        G.reset()
    assert l1 == l0 and e1 == e0, (l1, l0)
    assert torch.equal(w1, w0) and torch.equal(m1, m0)
    assert n1 < n0, (n1, n0)


def test_grouped_backward_gemms_change_nothing(te, dev, monkeypatch):
    """module._grouped_or_two: a Linear's dgrad + wgrad as ONE grouped launch (forced on for every eligible site through the autotune
    cache) against two launches: identical losses, weights and amax histories after 3 optimiser steps, bit for bit."""
    from llm_fp8_amd import train
    from llm_fp8_amd.pytorch.fp8 import FP8GlobalStateManager as G
    from llm_fp8_amd.pytorch import ops as _ops

    def run(grouped):
        G.reset()
        calls = {"n": 0}
        if grouped:
            monkeypatch.delenv("LLM_FP8_AMD_NO_GROUPED_GEMM", raising=False)

            def autotune(problems, fa, fb, iters=3, mx=False):
                assert mx is False  # the per-tensor sites must not ask for the block-scaled candidates and cache entry
                return 0 if all(a.shape[0] % 256 == 0 and b.shape[0] % 256 == 0 for a, b, _, _, _ in problems) else 3

            monkeypatch.setattr(_ops, "grouped_gemm_autotune", autotune)
            orig = _ops.gemm_fp8_grouped
            monkeypatch.setattr(_ops, "gemm_fp8_grouped", lambda *a, **k: (calls.__setitem__("n", calls["n"] + 1), orig(*a, **k))[1])
        else:
            monkeypatch.setenv("LLM_FP8_AMD_NO_GROUPED_GEMM", "1")
        cfg = train.TrainingConfig(model_name="llama-3.2-3b", batch_size=2, max_seq_length=384, mixed_precision="fp8",
                                   fp8_scenario="default", use_te=True, sharding_mode="none", num_hidden_layers=2, vocab_size=3072,
                                   learning_rate=1e-3, num_warmup_steps=0)
        torch.manual_seed(31)
        device = torch.device(dev)
        model = train.prepare_model(train.create_model(cfg, device), cfg)
        opt, sched = train.create_optimizer(model, cfg)
        model.train()
        gen = torch.Generator(device=device).manual_seed(12)
        losses = [train.train_step(model, train.synthetic_batch(cfg, 3072, device, gen), opt, sched, cfg).item() for _ in range(3)]
        hist = torch.cat([a.hist[:, :a.used].reshape(-1) for a in G._arenas.values()]).clone()
        flat = torch.cat([p.detach().reshape(-1).view(torch.int16) for p in model.parameters()]).clone()
        return losses, hist, flat, calls["n"]

    try:
        l1, h1, w1, n1 = run(True)
        l0, h0, w0, n0 = run(False)
    finally:
        G.reset()
    assert n1 >= 3 * 2 * 4 and n0 == 0, (n1, n0)   # 3 steps x 2 layers x (q|k|v, proj, fc2, fc1) (+ lm_head) grouped launches
    assert l1 == l0, (l1, l0)
    assert torch.equal(h1, h0) and torch.equal(w1, w0)


def test_dy_handoff_steps_aside_when_the_gradient_is_observed(te, dev):
    """module.handoff_readers: `retain_grad()` / a tensor hook on the logits, or anomaly mode, must see the REAL d(logits), not
    the unwritten placeholder of the cross-entropy -> lm_head hand-off; and the step must equal the no-hand-off step bit for bit."""
    from llm_fp8_amd import train
    from llm_fp8_amd.pytorch.fp8 import FP8GlobalStateManager as G

    def run(observe):
        G.reset()
        cfg = train.TrainingConfig(model_name="llama-3.2-3b", batch_size=2, max_seq_length=128, mixed_precision="fp8",
                                   fp8_scenario="default", use_te=True, sharding_mode="none", num_hidden_layers=1, vocab_size=2048,
                                   learning_rate=1e-3, num_warmup_steps=0)
        torch.manual_seed(5)
        device = torch.device(dev)
        model = train.prepare_model(train.create_model(cfg, device), cfg)
        model.train()
        batch = train.synthetic_batch(cfg, 2048, device, torch.Generator(device=device).manual_seed(2))
        out = model(**batch)
        seen = {}
        if observe == "retain":
            out.logits.retain_grad()
        elif observe == "hook":
            out.logits.register_hook(lambda g: seen.__setitem__("g", g.clone()))
        if observe == "anomaly":
            with torch.autograd.detect_anomaly(check_nan=True):
                out.loss.backward()
        else:
            out.loss.backward()
        g = out.logits.grad if observe == "retain" else seen.get("g")
        w = model.lm_head.weight.grad.clone()
        return g, w

    try:
        import os
        os.environ["LLM_FP8_AMD_NO_DY_HANDOFF"] = "1"
        g_ref, w_ref = run("hook")          # ordinary route: the true d(logits)
        del os.environ["LLM_FP8_AMD_NO_DY_HANDOFF"]
        for mode in ("retain", "hook", "anomaly", None):
            g, w = run(mode)
            assert torch.equal(w, w_ref), mode   # same lm_head wgrad whichever route
            if mode in ("retain", "hook"):
                assert g is not None and torch.equal(g, g_ref), mode
    finally:
        os.environ.pop("LLM_FP8_AMD_NO_DY_HANDOFF", None)
        G.reset()


def test_local_embedding_grad_rows_added_in_place(te, dev):
    """distributed.install_local_embedding_grad (what train.wrap_distributed does without a wrapper): the tied table's gradient
    = lm_head wgrad + embedding rows, the rows added in place; against autograd's dense route on the same model and batch."""
    from llm_fp8_amd import train
    from llm_fp8_amd.distributed import install_local_embedding_grad
    from llm_fp8_amd.pytorch.fp8 import FP8GlobalStateManager as G
    grads = []
    for install in (False, True):
        G.reset()
        cfg = train.TrainingConfig(model_name="llama-3.2-1b", batch_size=2, max_seq_length=128, mixed_precision="fp8",
                                   fp8_scenario="default", use_te=True, sharding_mode="none", num_hidden_layers=1, vocab_size=1024,
                                   learning_rate=1e-3, num_warmup_steps=0)
        torch.manual_seed(4)
        device = torch.device(dev)
        model = train.prepare_model(train.create_model(cfg, device), cfg)
        if install:
            assert install_local_embedding_grad(model) == 1
        model.train()
        gen = torch.Generator(device=device).manual_seed(2)
        batch = train.synthetic_batch(cfg, 1024, device, gen)
        model(**batch).loss.backward()
        table = model.get_input_embeddings().weight
        assert model.get_output_embeddings().weight is table
        grads.append(table.grad.float().clone())
    G.reset()
    dense, inplace = grads
    err = (dense - inplace).abs()
    # (the dense route rounds twice and sums repeated tokens' rows in bf16: long runs of repeats are checked against fp64 in
    # test_kernels_gpu.py::test_embedding_grad_add_in_place instead)
    tol = 2.0 ** -6 * torch.maximum(dense.abs(), inplace.abs()) + 2e-3 * dense.abs().max()
    assert float((err / tol).max()) <= 1.0 and float(inplace.abs().sum()) > 0


def test_residual_stats_handoff_between_decoder_layers(te, dev):
    """The residual add hands the next norm's rstd over (inside a layer as an argument, across layers on the tensor); a
    tensor modified in place, or a norm with another eps, ignores the hand-off."""
    from llm_fp8_amd import llama
    from llm_fp8_amd.pytorch import ops
    from llm_fp8_amd.pytorch.module import residual_add_stats, _usable_rstd
    cfg = llama.llama_config("llama-3.2-1b", num_hidden_layers=1, hidden_size=512, intermediate_size=1024, num_attention_heads=4,
                             num_key_value_heads=2, head_dim=128, vocab_size=1024, max_position_embeddings=256)
    torch.manual_seed(9)
    prev = torch.get_default_dtype()
    torch.set_default_dtype(torch.bfloat16)
    try:
        with torch.device(dev):
            layer = llama.decoder_layer_cls("default")(cfg, 0)
    finally:
        torch.set_default_dtype(prev)
    layer.to(dev).train()
    x = torch.randn(2, 128, cfg.hidden_size, device=dev, dtype=torch.bfloat16)
    with torch.no_grad():
        h = layer(x)
        tag = h._mi_rstd
        assert tag[1] == layer.self_attention.layernorm_qkv.eps and tag[2] == h._version
        np.testing.assert_allclose(tag[0].cpu().numpy(), ops.rmsnorm_stats(h.view(-1, cfg.hidden_size), tag[1]).cpu().numpy(), rtol=1e-6)
        assert llama._handed_rstd(h) is not None
        y_handed = layer(h)
        h2 = h.clone()                       # same values, no tag: the layer computes the statistics itself
        assert llama._handed_rstd(h2) is None
        y_plain = layer(h2)
        rel = ((y_handed.float() - y_plain.float()).norm() / y_plain.float().norm()).item()
        assert rel < 2e-3, rel               # rstd differs by summation order only (<= 1 ulp of f32) -> rare FP8 rounding flips
        h.mul_(2.0)                          # in-place change: stale statistics must not be used
        assert llama._handed_rstd(h) is None
    assert _usable_rstd((tag[0], 1e-6), h, 1e-5) is None and _usable_rstd((tag[0][:5], 1e-5), h, 1e-5) is None
    # autograd: the add distributes the gradient to both branches
    a = torch.randn(64, 512, device=dev, dtype=torch.bfloat16, requires_grad=True)
    b = torch.randn(64, 512, device=dev, dtype=torch.bfloat16, requires_grad=True)
    s, rstd = residual_add_stats(a, b, 1e-5)
    assert rstd is not None and not rstd.requires_grad
    w = torch.randn_like(s)
    (s * w).sum().backward()
    assert torch.equal(a.grad, w) and torch.equal(b.grad, w)
    s32, none = residual_add_stats(a.float(), b.float(), 1e-5)  # not bf16: plain add
    assert none is None and torch.equal(s32, a.float() + b.float())


@pytest.mark.parametrize("scenario", ["default", "hybrid", "mxfp8"])
def test_fp8_training_curve_tracks_hf_bf16(te, dev, scenario):
    """The reference validates its FP8 paths by loss curves against bf16 (paper/conference_101719.tex:280-297).  Same seeded
    4-layer model, same 40 batches, AdamW 1e-3: each scenario's FP8 curve follows the HF bf16 curve (bounded lag, see below)
    and settles on the same plateau within 3 %."""
    from transformers.models.llama.modeling_llama import LlamaForCausalLM
    from llm_fp8_amd import llama, train
    config = llama.llama_config("llama-3.2-1b", num_hidden_layers=4, hidden_size=512, intermediate_size=1536, num_attention_heads=4,
                                num_key_value_heads=2, head_dim=128, vocab_size=4096, max_position_embeddings=256, rope_theta=10000.0)
    torch.manual_seed(11)
    prev = torch.get_default_dtype()
    torch.set_default_dtype(torch.bfloat16)
    try:
        hf = LlamaForCausalLM(config)
    finally:
        torch.set_default_dtype(prev)
    g = torch.Generator().manual_seed(12)
    # a learnable toy language: next token = (3 * token + 1) mod 61 with 10 % noise, so the curve goes well below ln(V)
    B, S, steps = 8, 128, 40
    batches = []
    for _ in range(steps):
        x = torch.randint(0, 61, (B, 1), generator=g)
        seq = [x]
        for _ in range(S - 1):
            nxt = (3 * seq[-1] + 1) % 61
            noise = torch.randint(0, 61, (B, 1), generator=g)
            seq.append(torch.where(torch.rand(B, 1, generator=g) < 0.1, noise, nxt))
        batches.append(torch.cat(seq, 1).to(dev))

    def curve(model):
        model.train()
        opt = torch.optim.AdamW(model.parameters(), lr=1e-3)
        out = []
        for ids in batches:
            loss = model(input_ids=ids, labels=ids).loss
            loss.backward()
            torch.nn.utils.clip_grad_norm_(model.parameters(), 1.0)
            opt.step()
            opt.zero_grad()
            out.append(float(loss.detach()))
        return out

    cfg = train.TrainingConfig(model_name="llama-3.2-1b", mixed_precision="fp8", use_te=True, fp8_scenario=scenario)
    tem = train.prepare_model(llama.TELlamaForCausalLM.from_hf_state_dict(hf.state_dict(), config, scenario).to(dev), cfg)
    fp8_curve = curve(tem)
    ref_curve = curve(hf.to(dev))
    assert ref_curve[-1] < 0.2 * ref_curve[0], ref_curve  # the toy task is learnable (8.4 -> 0.77)
    # measured: hybrid and mxfp8 follow the bf16 curve step for step (one transient bump of 12 % at step 9); the "ours" recipe
    # (E4M3 gradients in the MLP) runs up to ~5 steps behind during the steep phase and reaches the same plateau
    lag = 6 if scenario == "default" else 2
    for i in range(3, steps):
        assert fp8_curve[i] <= 1.13 * max(ref_curve[max(0, i - lag):i + 1]), (scenario, i, fp8_curve[i], ref_curve[max(0, i - lag):i + 1])
        assert fp8_curve[i] >= 0.88 * min(ref_curve[i:i + 2]), (scenario, i, fp8_curve[i], ref_curve[i])
    tail_fp8, tail_ref = sum(fp8_curve[-10:]) / 10, sum(ref_curve[-10:]) / 10
    assert abs(tail_fp8 - tail_ref) < 0.03 * tail_ref, (scenario, tail_fp8, tail_ref)

@pytest.mark.gpu
@pytest.mark.parametrize("scenario", ["default", "mxfp8"])
def test_final_norm_fused_into_the_lm_head(te, dev, scenario, monkeypatch):
    """llama._install_final_norm_fusion: inside LlamaForCausalLM.forward HF's final RMSNorm hands its weight to the FP8 lm_head
    (K9 fusion in the head's input cast, statistics from the last decoder layer's residual add) instead of running its torch
    elementwise chain.  Against the unfused route (LLM_FP8_AMD_NO_FINAL_NORM_FUSION=1): HF's norm must not run, the first loss
    and every gradient agree within the rounding the fusion removes (HF rounds the normalised activations to bf16 twice before
    the cast), the norm weight gets its gradient, and three optimiser steps track each other."""
    from llm_fp8_amd import train
    from llm_fp8_amd.pytorch.fp8 import FP8GlobalStateManager as G
    from transformers.models.llama.modeling_llama import LlamaRMSNorm

    def run(disable):
        G.reset()
        if disable:
            monkeypatch.setenv("LLM_FP8_AMD_NO_FINAL_NORM_FUSION", "1")
        else:
            monkeypatch.delenv("LLM_FP8_AMD_NO_FINAL_NORM_FUSION", raising=False)
        calls = {"hf": 0}
        orig = LlamaRMSNorm.forward
        monkeypatch.setattr(LlamaRMSNorm, "forward", lambda self, x: (calls.__setitem__("hf", calls["hf"] + 1), orig(self, x))[1])
        cfg = train.TrainingConfig(model_name="llama-3.2-3b", batch_size=2, max_seq_length=128, mixed_precision="fp8",
                                   fp8_scenario=scenario, use_te=True, sharding_mode="none", num_hidden_layers=2, vocab_size=2048,
                                   learning_rate=1e-3, num_warmup_steps=0)
        torch.manual_seed(33)
        device = torch.device(dev)
        model = train.prepare_model(train.create_model(cfg, device), cfg)
        opt, sched = train.create_optimizer(model, cfg)
        model.train()
        gen = torch.Generator(device=device).manual_seed(9)
        batch = train.synthetic_batch(cfg, 2048, device, gen)
        out = model(**batch)
        out.loss.backward()
        first = out.loss.item()
        grads = {n: p.grad.detach().float().clone() for n, p in model.named_parameters() if p.grad is not None}
        opt.zero_grad(set_to_none=True)
        losses = [train.train_step(model, train.synthetic_batch(cfg, 2048, device, gen), opt, sched, cfg).item() for _ in range(3)]
        # evaluation (FP8 off under no_grad, as accelerate's wrapper does): HF's norm runs, whatever the switch says
        model.eval()
        before = calls["hf"]
        with torch.no_grad():
            ev = model(**batch).loss.item()
        model.train()
        monkeypatch.setattr(LlamaRMSNorm, "forward", orig)
        return first, grads, losses, calls["hf"], calls["hf"] - before, ev

    try:
        f1, g1, l1, n1, e1, ev1 = run(False)
        f0, g0, l0, n0, e0, ev0 = run(True)
    finally:
        G.reset()
    assert n0 == 4 + 1 and e0 == 1, (n0, e0)       # unfused: HF's final norm in each of the 4 training forwards and in the eval pass
    assert n1 == 1 and e1 == 1, (n1, e1)           # fused: only in the eval pass
    assert abs(f1 - f0) <= 2e-3 * abs(f0), (f1, f0)
    assert "model.norm.weight" in g1 and g1["model.norm.weight"].abs().max() > 0
    ds = {n: float((g1[n] - g0[n]).norm() / (g0[n].norm() + 1e-12)) for n in g0}
    assert ds["model.norm.weight"] <= 0.02, ds
    # MXFP8 has no scaling state: every gradient agrees to < 1 %.  Under delayed scaling the FIRST backward quantises its
    # gradients with scale 1 (TE's initial state: most E5M2 / E4M3 values sit in the subnormal range or underflow),
    # where the different bf16 roundings of the two routes flip a visible share of the quantised values
    assert max(ds.values()) <= (0.02 if scenario == "mxfp8" else 0.4), ds
    assert all(abs(a - b) <= 5e-3 * abs(b) for a, b in zip(l1, l0)), (l1, l0)
    assert abs(ev1 - ev0) <= 5e-3 * abs(ev0), (ev1, ev0)

@pytest.mark.gpu
def test_grad_norm_does_not_depend_on_grouping_or_row_sharding(dev):
    """optim.ClippedAdamW's squared norm: exact fp32 squares accumulated in float64 (mi_sumsq_bf16_multi), float64 totals, one
    rounding at the end -- so the clip coefficient is the same bit pattern however the parameters are cut into groups, chunks or
    row shards (distributed.ShardedFP8DP's groups against the replicated wrapper's: in fp32 the association moved the last bit in
    a few percent of the steps and a handful of weights then rounded differently).  Against float64 torch on the same gradients."""
    from llm_fp8_amd.optim import ClippedAdamW
    torch.manual_seed(5)
    shapes = [(2048, 1536), (4096, 1024), (777,), (1536, 2048), (33, 65)]
    grads = [(torch.randn(s, device=dev) * (10.0 ** (i - 2))).to(torch.bfloat16) for i, s in enumerate(shapes)]
    exact = torch.sqrt(sum((g.double() ** 2).sum() for g in grads)).to(torch.float32).item()

    def norm_of(partition):
        """partition: list of groups, a group = list of (tensor index, row slice or None)"""
        groups = []
        for grp in partition:
            ps = []
            for idx, rows in grp:
                g = grads[idx] if rows is None else grads[idx][rows].contiguous()
                p = torch.nn.Parameter(torch.zeros_like(g))
                p.grad = g.clone()
                ps.append(p)
            groups.append({"params": ps})
        opt = ClippedAdamW(groups, lr=0.0, max_grad_norm=1.0)
        opt.step()
        return opt.last_grad_norm.item()

    one_group = norm_of([[(i, None) for i in range(5)]])
    per_tensor = norm_of([[(i, None)] for i in range(5)])
    reversed_ = norm_of([[(i, None) for i in reversed(range(5))]])
    row_shards = norm_of([[(0, slice(0, 1024)), (1, slice(0, 2048)), (3, slice(0, 768))],
                          [(0, slice(1024, 2048)), (1, slice(2048, 4096)), (3, slice(768, 1536))], [(2, None), (4, None)]])
    assert one_group == per_tensor == reversed_ == row_shards == exact, (one_group, per_tensor, reversed_, row_shards, exact)
