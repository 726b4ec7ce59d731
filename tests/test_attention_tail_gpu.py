"""Attention core at sequence lengths that are a multiple of 16 but not of 128 (the TAIL instantiations of csrc/mi_attn.hip:
a partial last 128-row block, 64-key tile and 32-row query slice): identity with the full-block kernels on a prefix, float64,
a known answer up to the last row, isolation of everything at or past S, the module route, and the lengths still refused."""
import numpy as np
import pytest
import torch

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


# ------------------------------------------------------------------------------------------------ 1. prefix identity
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("S", [144, 176, 208, 240])
def test_causal_prefix_is_the_full_block_kernels(ops, dev, S, D):
    """Causal attention over the first S tokens of a 256-token sequence, against the full-block kernels run on all 256 with
    dO = 0 at and past S.  Derived, not measured: both runs walk the same tiles in the same order; a causal row below S never
    sees a later key (its p there is exactly 0 in both, times zeros here and times finite K / V there); a query row with
    dO = 0 has delta = 0 and dP = 0, so it adds p * 0 = exact zeros to dK and dV.  Equal as values (0.0 == -0.0)."""
    B, H, G, SF = 2, 8, 2, 256
    scale = D ** -0.5
    q, k, v, do = (t.to(dev) for t in _rand(B, SF, H, G, D, seed=S + D))
    do[:, S:] = 0
    o_f, lse_f = ops.attn_fwd(q, k, v, scale, True)
    dq_f, dk_f, dv_f = ops.attn_bwd(do, q, k, v, o_f, lse_f, scale, True)
    qs, ks, vs, dos = (t[:, :S].contiguous() for t in (q, k, v, do))
    o_t, lse_t = ops.attn_fwd(qs, ks, vs, scale, True)
    assert torch.equal(o_t, o_f[:, :S]), "o"
    assert torch.equal(lse_t, lse_f[:, :, :S]), "lse"
    dq_t, dk_t, dv_t = ops.attn_bwd(dos, qs, ks, vs, o_t, lse_t, scale, True)
    for name, got, ref in (("dq", dq_t, dq_f), ("dk", dk_t, dk_f), ("dv", dv_t, dv_f)):
        assert torch.equal(got, ref[:, :S]), f"{name}: {(got != ref[:, :S]).sum().item()} elements differ"


# ------------------------------------------------------------------------------------------------ 2. float64
ORACLE_CASES = [(2, 144, 4, 1, 64, True), (2, 208, 8, 2, 128, True), (1, 400, 8, 2, 128, True),
                (2, 144, 4, 1, 64, False), (2, 208, 8, 2, 128, False)]


@pytest.mark.parametrize("B,S,H,G,D,causal", ORACLE_CASES)
def test_tail_vs_float64(ops, dev, B, S, H, G, D, causal):
    q, k, v, do = _rand(B, S, H, G, D, seed=B * S + H * G + D + 1)
    scale = D ** -0.5
    o_ref, lse_ref = O.attention_f64(bf16_bits(q), bf16_bits(k), bf16_bits(v), scale, causal)
    qd, kd, vd, dod = (t.to(dev) for t in (q, k, v, do))
    o, lse = ops.attn_fwd(qd, kd, vd, scale, causal)
    _check_fwd(o, lse, o_ref, lse_ref, v, f"B{B} S{S} H{H} G{G} D{D} causal={causal}")
    # as test_attn_grid_vs_float64: delta = rowsum(dO * O) of the stored bf16 O just checked, in the reference too
    refs = O.attention_bwd_f64(bf16_bits(q), bf16_bits(k), bf16_bits(v), bf16_bits(do), scale, causal, o_bits=bf16_bits(o))
    grads = ops.attn_bwd(dod, qd, kd, vd, o, lse, scale, causal)
    for got, ref, name in zip(grads, refs, ("dq", "dk", "dv")):
        _check_bwd(got, ref, name)


# ------------------------------------------------------------------------------------------------ 3. known answer: q = 0
@pytest.mark.parametrize("S", [144, 400])
def test_zero_query_lse_up_to_the_last_row(ops, dev, S):
    """q = 0, causal (test_zero_query_known_answer): row r sees r + 1 keys of score 0, lse[r] = log2(r + 1) for every row up
    to S - 1.  A key at or past S counted in, or a row of the partial block dropped, shows in that row."""
    B, H, G, D = 2, 4, 2, 64
    g = torch.Generator(device=dev).manual_seed(S)
    q = torch.zeros(B, S, H, D, device=dev, dtype=torch.bfloat16)
    k, v = (torch.randn(B, S, G, D, device=dev, dtype=torch.bfloat16, generator=g) for _ in range(2))
    lse = torch.full((B, H, S), float("nan"), device=dev)
    o = torch.empty_like(q)
    ops.attn_fwd(q, k, v, D ** -0.5, True, out=(o, lse))
    lse_ref = np.broadcast_to(np.log2(np.arange(1, S + 1, dtype=np.float64)), (B, H, S))
    # lse = 0 * c + v_log_f32(l) with l = r + 1 summed exactly in fp32: v_log_f32's error, within 4 ulps
    tol = 4 * np.spacing(np.maximum(lse_ref, 1.0).astype(np.float32)).astype(np.float64)
    err = np.abs(lse.double().cpu().numpy() - lse_ref)
    bad = np.argwhere(~(err <= tol))
    assert bad.size == 0, f"lse off at {len(bad)} (b, h, row), first {bad[:5].tolist()}: got {lse[tuple(bad[0])].item()!r}"


# ------------------------------------------------------------------------------------------------ 4. isolation
CANARY = 0x7FC1  # a bf16 quiet NaN: whatever reads it into a sum poisons the result


@pytest.mark.parametrize("D,causal", [(64, True), (128, True), (64, False), (128, False)])
def test_nothing_at_or_past_S_is_read_or_written(ops, dev, D, causal):
    """The scheme of test_distinct_token_strides_bitwise_and_canaries at S = 144: every operand and output a view with its
    own token stride inside a buffer of NaN canaries, with 128 canary tokens and more behind the last batch (the rows the
    partial block would reach), and batch 1 right behind batch 0 (the rows batch 0's partial block would reach)."""
    B, S, H, G = 2, 144, 8, 2
    scale = D ** -0.5
    width = {"q": H, "k": G, "v": G, "o": H, "do": H, "dq": H, "dk": G, "dv": G}
    pad = {"q": 8, "k": 16, "v": 24, "o": 32, "do": 40, "dq": 48, "dk": 56, "dv": 64}
    ts = {n: width[n] * D + pad[n] for n in width}
    span = (B * S + 128) * max(ts.values())  # >= 128 tokens of canaries behind the last token at every stride
    bufs = {n: torch.full((span,), CANARY, dtype=torch.int16, device=dev) for n in width}
    shape = {n: (B, S, width[n], D) for n in width}
    stride = {n: (S * ts[n], ts[n], D, 1) for n in width}
    view = {n: bufs[n].view(torch.bfloat16).as_strided(shape[n], stride[n]) for n in width}

    q, k, v, do = (t.to(dev) for t in _rand(B, S, H, G, D, seed=D + causal))
    for n, t in (("q", q), ("k", k), ("v", v), ("do", do)):
        view[n].copy_(t)
    before = {n: bufs[n].clone() for n in ("q", "k", "v", "do")}

    o_c, lse_c = ops.attn_fwd(q, k, v, scale, causal)
    dq_c, dk_c, dv_c = ops.attn_bwd(do, q, k, v, o_c, lse_c, scale, causal)
    for n, t in (("o", o_c), ("lse", lse_c), ("dq", dq_c), ("dk", dk_c), ("dv", dv_c)):
        assert torch.isfinite(t).all(), f"{n} (contiguous call) is not finite"

    guard = 256
    lse_buf = torch.full((guard + B * H * S + guard,), float("nan"), device=dev)
    lse_s = lse_buf[guard:guard + B * H * S].view(B, H, S)
    o_s, _ = ops.attn_fwd(view["q"], view["k"], view["v"], scale, causal, out=(view["o"], lse_s))
    assert o_s.data_ptr() == view["o"].data_ptr()
    dq_s, dk_s, dv_s = ops.attn_bwd(view["do"], view["q"], view["k"], view["v"], view["o"], lse_s, scale, causal,
                                    out=(view["dq"], view["dk"], view["dv"]))
    torch.cuda.synchronize()

    assert torch.equal(lse_s, lse_c), "lse"
    assert torch.isnan(lse_buf[:guard]).all() and torch.isnan(lse_buf[guard + B * H * S:]).all(), "lse: a guard element was written"
    for n, got, ref in (("o", view["o"], o_c), ("dq", dq_s, dq_c), ("dk", dk_s, dk_c), ("dv", dv_s, dv_c)):
        assert torch.equal(got.view(torch.int16), ref.view(torch.int16)), f"{n}: strided call differs from the contiguous one"
        assert torch.isfinite(got).all(), f"{n} is not finite"
    for n in ("q", "k", "v", "do"):
        assert torch.equal(bufs[n], before[n]), f"input {n} was written"
    for n in ("o", "dq", "dk", "dv"):
        outside = torch.ones(span, dtype=torch.bool, device=dev)
        outside.as_strided(shape[n], stride[n]).fill_(False)
        assert outside.sum().item() == span - B * S * width[n] * D
        assert (bufs[n][outside] == CANARY).all(), f"{n}: an element outside the tensor was written"

    # batch 0 of the two-batch run is the run on batch 0 alone: nothing of batch 1 reached it
    q1, k1, v1, do1 = (t[:1].contiguous() for t in (q, k, v, do))
    o_1, lse_1 = ops.attn_fwd(q1, k1, v1, scale, causal)
    dq_1, dk_1, dv_1 = ops.attn_bwd(do1, q1, k1, v1, o_1, lse_1, scale, causal)
    assert torch.equal(lse_1, lse_c[:1]), "lse: batch 0 depends on batch 1"
    for n, one, two in (("o", o_1, o_c), ("dq", dq_1, dq_c), ("dk", dk_1, dk_c), ("dv", dv_1, dv_c)):
        assert torch.equal(one.view(torch.int16), two[:1].view(torch.int16)), f"{n}: batch 0 depends on batch 1"


# ------------------------------------------------------------------------------------------------ 5. module route
@pytest.mark.parametrize("S", [144, 400])
def test_flash_ok_takes_multiples_of_16(dev, S):
    from llm_fp8_amd.pytorch import attention as A
    q, k, v = (torch.randn(2, S, n, 128, device=dev, dtype=torch.bfloat16) for n in (6, 2, 2))
    assert A._flash_ok(q, k, v, True, 0.0)


def test_dot_product_attention_flash_path_matches_sdpa_at_400(dev):
    """The construction and the bound of test_dot_product_attention_flash_path_matches_sdpa, at S = 400."""
    from llm_fp8_amd.pytorch import attention as A
    B, S, H, G, D = 2, 400, 6, 2, 128
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


def test_training_step_at_144_runs_the_attention_kernels(dev):
    """One forward + backward of a 1-layer Llama (the config of test_decoder_layer_skip_fusion_matches_plain_residual, default
    recipe) on a batch of 2 x 144 tokens: the attention core is one attn_fwd and one attn_bwd launch, not the SDPA route."""
    from transformers.models.llama.modeling_llama import LlamaForCausalLM
    from llm_fp8_amd import llama
    from llm_fp8_amd.pytorch.fp8 import FP8GlobalStateManager
    from llm_fp8_amd.pytorch.profiler import KernelTimer
    cfg = llama.llama_config("llama-3.2-1b", num_hidden_layers=1, hidden_size=512, intermediate_size=1024, num_attention_heads=4,
                             num_key_value_heads=2, head_dim=128, vocab_size=1024, max_position_embeddings=256)
    FP8GlobalStateManager.reset()
    try:
        torch.manual_seed(0)
        model = llama.TELlamaForCausalLM.from_hf_state_dict(LlamaForCausalLM(cfg).to(dev).to(torch.bfloat16).state_dict(), cfg,
                                                            "default").to(dev)
        model.train()
        ids = torch.randint(0, cfg.vocab_size, (2, 144), device=dev)
        with KernelTimer().install() as timer:
            loss = model(input_ids=ids, labels=ids).loss
            loss.backward()
        torch.cuda.synchronize()
        launches = {k: v["launches"] for k, v in timer.summarize().items()}
        assert launches.get("attn_fwd") == 1 and launches.get("attn_bwd") == 1, launches
        assert torch.isfinite(loss).item(), loss
        grads = [(n, p.grad) for n, p in model.named_parameters() if p.requires_grad]
        assert grads and all(g is not None for _, g in grads), [n for n, g in grads if g is None]
        for n, g in grads:
            assert torch.isfinite(g).all(), f"gradient of {n} is not finite"
    finally:
        FP8GlobalStateManager.reset()


# ------------------------------------------------------------------------------------------------ 6. refusals
@pytest.mark.parametrize("S", [64, 136, 200])
def test_short_and_odd_lengths_stay_refused(ops, dev, S):
    """Below one full block, or not a multiple of 16: refused by both launchers (named in the message) and by _flash_ok."""
    from llm_fp8_amd.pytorch import attention as A
    B, H, G, D = 1, 4, 2, 64
    q, k, v = (torch.randn(B, S, n, D, device=dev, dtype=torch.bfloat16) for n in (H, G, G))
    assert not A._flash_ok(q, k, v, True, 0.0)
    with pytest.raises(RuntimeError, match="mi_attn_fwd"):
        ops.attn_fwd(q, k, v, D ** -0.5, True)
    o = torch.zeros(B, S, H, D, device=dev, dtype=torch.bfloat16)
    lse = torch.zeros(B, H, S, device=dev)
    with pytest.raises(RuntimeError, match="mi_attn_bwd"):
        ops.attn_bwd(o, q, k, v, o, lse, D ** -0.5, True)
