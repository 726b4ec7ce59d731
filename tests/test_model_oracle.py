"""tests/model_oracle.py on the CPU: (1) with quantisers and roundings switched to the identity, its hand-written forward and backward
chained over a 2-layer model equal float64 autograd through HF's Llama and Qwen3; (2) its quantisers are bitwise the numpy oracles;
(3) the float32 twins are deterministic and, per tensor of a teacher-forced layer, nearer to the float64 emulation than quantisation
itself moves that tensor -- so the GPU criterion of tests/test_model_parity_gpu.py (a multiple of the twins' distance) is tighter
than the quantisation noise."""
import numpy as np
import pytest
import torch

from oracle import fp8_oracle as O
from tests import block_oracle as BO
from tests import glue_oracle as G
from tests import model_oracle as M

LLAMA = dict(hidden_size=256, intermediate_size=512, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=2, head_dim=64,
             vocab_size=1024)
QWEN3 = dict(hidden_size=512, intermediate_size=1024, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=2, head_dim=128,
             vocab_size=512)


def _hf_model(family: str):
    """float64 HF model, eager attention, MLP biases, rotary base 10000 for Llama (what TELlamaDecoderLayer builds its table with)."""
    if family == "llama":
        from transformers import LlamaConfig
        from transformers.models.llama.modeling_llama import LlamaForCausalLM
        cfg = LlamaConfig(**LLAMA, mlp_bias=True, rope_theta=10000.0, tie_word_embeddings=True, rms_norm_eps=1e-5, attention_bias=False)
        cfg._attn_implementation = "eager"
        torch.manual_seed(1)
        model = LlamaForCausalLM(cfg)
    else:
        from transformers import Qwen3Config
        from transformers.models.qwen3.modeling_qwen3 import Qwen3ForCausalLM
        cfg = Qwen3Config(**QWEN3, rope_theta=1000000.0, tie_word_embeddings=True, rms_norm_eps=1e-6, attention_bias=False,
                          use_sliding_window=False, bos_token_id=None, eos_token_id=None)
        cfg._attn_implementation = "eager"
        torch.manual_seed(2)
        model = Qwen3ForCausalLM(cfg)
        for layer in model.model.layers:  # HF's Qwen3 MLP has no bias option: the TE layer's fc1_bias / fc2_bias need one to map to
            for name in ("gate_proj", "up_proj", "down_proj"):
                old = getattr(layer.mlp, name)
                new = torch.nn.Linear(old.in_features, old.out_features, bias=True)
                new.weight = old.weight
                setattr(layer.mlp, name, new)
    model = model.double()
    M.redraw_(model, seed=11)
    return model, cfg


def _oracle_params(sd, n_layers, qk_norm):
    """HF names -> model_oracle's, the mapping of llama.replace_params (q|k|v separate, gate | up stacked) plus the biases."""
    f = lambda k: sd[k].detach().numpy().astype(np.float64)
    layers = []
    for i in range(n_layers):
        p = f"model.layers.{i}."
        d = dict(ln1=f(p + "input_layernorm.weight"), wq=f(p + "self_attn.q_proj.weight"), wk=f(p + "self_attn.k_proj.weight"),
                 wv=f(p + "self_attn.v_proj.weight"), wo=f(p + "self_attn.o_proj.weight"), ln2=f(p + "post_attention_layernorm.weight"),
                 w1=np.concatenate([f(p + "mlp.gate_proj.weight"), f(p + "mlp.up_proj.weight")], 0),
                 b1=np.concatenate([f(p + "mlp.gate_proj.bias"), f(p + "mlp.up_proj.bias")], 0),
                 w2=f(p + "mlp.down_proj.weight"), b2=f(p + "mlp.down_proj.bias"))
        if qk_norm:
            d.update(gq=f(p + "self_attn.q_norm.weight"), gk=f(p + "self_attn.k_norm.weight"))
        layers.append(d)
    return dict(table=f("model.embed_tokens.weight"), norm=f("model.norm.weight"), layers=layers)


_HF_OF = dict(ln1="input_layernorm.weight", wq="self_attn.q_proj.weight", wk="self_attn.k_proj.weight", wv="self_attn.v_proj.weight",
              wo="self_attn.o_proj.weight", ln2="post_attention_layernorm.weight", w2="mlp.down_proj.weight", b2="mlp.down_proj.bias",
              gq="self_attn.q_norm.weight", gk="self_attn.k_norm.weight")


def _hf_grads(grads, inter):
    """model_oracle's gradient names -> HF parameter names."""
    out = {"model.embed_tokens.weight": grads["table"], "model.norm.weight": grads["norm"]}
    for name, g in grads.items():
        if not name.startswith("layers."):
            continue
        _, i, n = name.split(".")
        p = f"model.layers.{i}."
        if n == "w1":
            out[p + "mlp.gate_proj.weight"], out[p + "mlp.up_proj.weight"] = g[:inter], g[inter:]
        elif n == "b1":
            out[p + "mlp.gate_proj.bias"], out[p + "mlp.up_proj.bias"] = g[:inter], g[inter:]
        else:
            out[p + _HF_OF[n]] = g
    return out


def _eager_attention_f64(module, query, key, value, attention_mask, scaling, dropout=0.0, **_kw):
    """HF's eager_attention_forward with the softmax left in the dtype of its input: HF's own takes it in float32 whatever the
    model's dtype, which caps a float64 model's gradients at 1e-7."""
    from transformers.models.llama.modeling_llama import repeat_kv
    k, v = repeat_kv(key, module.num_key_value_groups), repeat_kv(value, module.num_key_value_groups)
    w = torch.matmul(query, k.transpose(2, 3)) * scaling
    if attention_mask is not None:
        w = w + attention_mask[:, :, :, :k.shape[-2]]
    w = torch.softmax(w, dim=-1)
    return torch.matmul(w, v).transpose(1, 2).contiguous(), w


def _rmsnorm_f64(self, x):
    """HF's LlamaRMSNorm / Qwen3RMSNorm forward without its cast of the input to float32 (a down-cast for a float64 model)."""
    return self.weight * (x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + self.variance_epsilon))


@pytest.mark.parametrize("family", ["llama", "qwen3"])
def test_identity_emulation_equals_float64_autograd_through_hf(family, capsys, monkeypatch):
    import importlib
    hf_mod = importlib.import_module(f"transformers.models.{family}.modeling_{family}")
    monkeypatch.setattr(hf_mod, "eager_attention_forward", _eager_attention_f64)
    monkeypatch.setattr(getattr(hf_mod, {"llama": "LlamaRMSNorm", "qwen3": "Qwen3RMSNorm"}[family]), "forward", _rmsnorm_f64)
    model, cfg = _hf_model(family)
    B, S = 2, 144
    ids, labels = M.draw_batch(cfg.vocab_size, B, S, seed=5)
    # HF's ForCausalLMLoss casts the logits to float32: the same loss (labels shifted by one, mean over labels != -100) on the
    # float64 logits instead
    logits = model(input_ids=torch.from_numpy(ids)).logits
    hf_loss = torch.nn.functional.cross_entropy(logits.reshape(B * S, -1), torch.from_numpy(M.shift_labels(labels)), ignore_index=-100)
    hf_loss.backward()
    cos, sin = model.model.rotary_emb(torch.zeros(1, dtype=torch.float64), torch.arange(S)[None])
    half = cfg.head_dim // 2
    ecfg = M.Config(B, S, cfg.num_attention_heads, cfg.num_key_value_heads, cfg.head_dim, cfg.rms_norm_eps, cos[0, :, :half].numpy(),
                    sin[0, :, :half].numpy(), qk_norm=family == "qwen3", rnd=M.ident)
    params = _oracle_params(model.state_dict(), cfg.num_hidden_layers, family == "qwen3")
    loss, grads = M.model(params, ids, labels, ecfg)
    got = _hf_grads(grads, cfg.intermediate_size)
    want = {n: p.grad.numpy() for n, p in model.named_parameters()}
    assert set(got) == set(want)                                   # every parameter, none twice
    assert abs(loss - hf_loss.item()) <= 1e-9 * abs(hf_loss.item())
    worst = {n: M.rel_err(got[n], want[n]) for n in want}
    with capsys.disabled():
        print(f"\n[{family}] loss {loss:.12f}; worst relative gradient error {max(worst.values()):.2e} ({max(worst, key=worst.get)})")
    for n, e in worst.items():
        assert np.linalg.norm(want[n]) > 0, n
        assert e <= 1e-9, (n, e)


def test_test_data_has_the_edges_the_issue_asks_for():
    ids, labels = M.draw_batch(1024, 2, 144, seed=5)
    assert (labels == -100).sum() >= 8 and ((labels >= 0) & (labels < 1024)).sum() > 200
    assert len(np.unique(ids)) < ids.size - 8                      # repeated token ids
    assert labels[labels != -100].tolist() == ids[labels != -100].tolist()


# ------------------------------------------------------------------------------------------------ quantisers
def _edge_blocks(seed, rows=64, cols=256):
    """Random values over several decades plus the edges: zeros, a zero block, values at and past the FP8 maxima, bf16 subnormals."""
    rng = np.random.default_rng(seed)
    v = (rng.standard_normal((rows, cols)) * np.exp2(rng.integers(-12, 6, (rows, 1)))).astype(np.float32)
    v[3, :32] = 0.0
    v[5] = 0.0
    v[7, 40:44] = [448.0, -57344.0, 1e-39, 3.0e38]
    return G.bf16_to_f32(G.f32_to_bf16(v))


@pytest.mark.parametrize("fmt", [O.E4M3, O.E5M2])
def test_quantisers_are_bitwise_the_numpy_oracles(fmt):
    x = _edge_blocks(3)
    bits = G.f32_to_bf16(x)
    # delayed: bytes and amax of O.quantize_delayed
    for scale in (np.float32(1.0), np.float32(37.25), np.float32(2.0 ** -9)):
        want, amax = O.quantize_delayed(bits, scale, fmt)
        assert np.array_equal(M.per_tensor_bytes(x, scale, fmt), want)
        q = M.DelayedQ({"k": scale}, fmt, fmt)
        op = q.quant(x.astype(np.float64), "x", "k")
        assert np.array_equal(op.row, O.fp8_decode(want, fmt).astype(np.float64)) and op.row is op.col
        assert op.alpha == np.float32(1.0) / scale and q.amax["k"] == amax
    # current: the scale of the live amax
    amax = O.amax_f32(x)
    s = M.current_scale(amax, fmt)
    assert s == np.float32(O.FP8_MAX[fmt] / amax) and M.current_scale(0.0, fmt) == 1.0 and M.current_scale(np.inf, fmt) == 1.0
    op = M.CurrentQ(fmt, fmt).quant(x.astype(np.float64), "grad", None)
    assert np.array_equal(op.row, O.fp8_decode(O.quantize_delayed(bits, s, fmt)[0], fmt).astype(np.float64))
    # MXFP8: both copies
    y, e = O.mxfp8_quantize_rowwise(bits, fmt)
    yc, ec = O.mxfp8_quantize_colwise(bits, fmt)
    assert all(np.array_equal(a, b) for a, b in zip(M.mx_codes(x, fmt), (y, e)))
    op = M.MXQ(fmt, fmt).quant(x.astype(np.float64), "w", None)
    deq = lambda yy, ee: O.fp8_decode(yy, fmt).astype(np.float64) * np.repeat(O.e8m0_to_f32(ee).astype(np.float64), 32, axis=1)
    assert np.array_equal(op.row, deq(y, e), equal_nan=True) and np.array_equal(op.col, deq(yc, ec).T, equal_nan=True)
    # block scaling: 1 x 128 for activations and gradients, 128 x 128 for weights
    for role, dim in (("x", 1), ("grad", 1), ("w", 2)):
        y_row, s_row, y_colT, s_colT = BO.quantize(bits, fmt, dim)
        op = M.BlockQ(fmt, fmt).quant(x.astype(np.float64), role, None)
        assert np.array_equal(op.row, BO.dequantize(y_row, s_row, fmt), equal_nan=True)
        assert np.array_equal(op.col, BO.dequantize(y_colT, s_colT, fmt).T, equal_nan=True)


def test_emulated_linear_is_the_single_linear_oracles():
    """The three GEMMs of model_oracle on one Linear give the bits of O.DelayedLinearOracle, O.mxfp8_linear_fwd_bwd and
    block_oracle.linear_fwd_bwd."""
    rng = np.random.default_rng(9)
    bf = lambda *s, k=1.0: G.f32_to_bf16((rng.standard_normal(s) * k).astype(np.float32))
    xb, wb, gb = bf(64, 256), bf(128, 256, k=0.05), bf(64, 128, k=0.01)
    x, w, g = (G.bf16_to_f64(t) for t in (xb, wb, gb))

    def run(q):
        X, W, Gd = q.quant(x, "x", "x"), q.quant(w, "w", "w"), q.quant(g, "grad", "g")
        return [G.rne_bf16(t) for t in (M.fwd_gemm(M.F64, X, W), M.dgrad_gemm(M.F64, Gd, W), M.wgrad_gemm(M.F64, Gd, X))]

    orc = O.DelayedLinearOracle(O.E4M3, O.E5M2)
    orc.s_fwd[:2], orc.s_bwd[0] = (np.float32(50.0), np.float32(900.0)), np.float32(20000.0)
    orc.si_fwd[:2], orc.si_bwd[0] = np.float32(1) / orc.s_fwd[:2], np.float32(1) / orc.s_bwd[0]
    want = [orc.forward(xb, wb), *orc.backward(gb)[:2]]
    got = run(M.DelayedQ({"x": orc.s_fwd[0], "w": orc.s_fwd[1], "g": orc.s_bwd[0]}))
    assert all(np.array_equal(a, b) for a, b in zip(got, want))
    y, dx, dw, _ = O.mxfp8_linear_fwd_bwd(xb, wb, gb)
    assert all(np.array_equal(a, b) for a, b in zip(run(M.MXQ()), (y, dx, dw)))
    y, dx, dw, _ = BO.linear_fwd_bwd(xb, wb, gb, O.E4M3, O.E4M3)
    assert all(np.array_equal(a, G.f32_to_bf16(b)) for a, b in zip(run(M.BlockQ()), (y, dx, dw)))


# ------------------------------------------------------------------------------------------------ twins
def _layer_case(family, S=144, seed=0):
    """A teacher-forced layer without a device: bf16 boundary tensors, parameters and scales of the magnitudes a trained-from-init
    model has (weights N(0, 0.02), hidden state O(1), a gradient of 1e-3)."""
    shp = LLAMA if family == "llama" else QWEN3
    H, I, nq, nkv, D = shp["hidden_size"], shp["intermediate_size"], shp["num_attention_heads"], shp["num_key_value_heads"], shp["head_dim"]
    rng = np.random.default_rng([seed, H])
    bf = lambda *s, k=1.0, m=0.0: G.bf16_to_f64(G.f32_to_bf16((m + rng.standard_normal(s) * k).astype(np.float32)))
    p = dict(ln1=bf(H, k=0.25, m=1.0), wq=bf(nq * D, H, k=0.02), wk=bf(nkv * D, H, k=0.02), wv=bf(nkv * D, H, k=0.02),
             wo=bf(H, nq * D, k=0.02), ln2=bf(H, k=0.25, m=1.0), w1=bf(2 * I, H, k=0.02), b1=bf(2 * I, k=0.05), w2=bf(H, I, k=0.02),
             b2=bf(H, k=0.05))
    if family == "qwen3":
        p.update(gq=bf(D, k=0.25, m=1.0), gk=bf(D, k=0.25, m=1.0))
    B = 2
    cos, sin = G.rope_tables(S, D, poison=False)
    cfg = M.Config(B, S, nq, nkv, D, 1e-5 if family == "llama" else 1e-6, cos, sin, qk_norm=family == "qwen3",
                   fused=H % 512 == 0)
    return p, bf(B * S, H), bf(B * S, H, k=1e-3), cfg


class _Warmup(M.CurrentQ):
    """Collects the amax of every slot: the scales a delayed-scaling run would have settled on."""

    def __init__(self, fmt_f, fmt_b):
        super().__init__(fmt_f, fmt_b)
        self.scales = {}

    def _quant(self, v, role, key):
        fmt = self.fmt(role)
        self.scales[key] = M.current_scale(O.amax_f32(M._f32(v)), fmt)
        return super()._quant(v, role, key)


def _quantisers(scenario, p, x, dout, cfg):
    """(attention-region, MLP-region) quantisers of llama.scenario_recipes."""
    if scenario in ("default", "hybrid"):
        fa, fm = (O.E4M3, O.E5M2), ((O.E4M3, O.E4M3) if scenario == "default" else (O.E4M3, O.E5M2))
        wa, wm = _Warmup(*fa), _Warmup(*fm)
        out, k = M.layer_forward(p, x, cfg, wa, wm)
        M.layer_backward(p, k, dout, cfg, wa, wm)
        return M.DelayedQ(wa.scales, *fa), M.DelayedQ(wm.scales, *fm)
    q = {"current": M.CurrentQ(O.E4M3, O.E5M2), "mxfp8": M.MXQ(), "block": M.BlockQ()}[scenario]
    return q, q


def _run_layer(p, x, dout, cfg, qa, qm, ar):
    out, k = M.layer_forward(p, x, cfg, qa, qm, ar)
    dx, gr = M.layer_backward(p, k, dout, cfg, qa, qm, ar)
    gr.pop("dh1_own")
    return dict(out=out, dx=dx, **gr)


@pytest.mark.parametrize("family,scenario", [("llama", s) for s in ("default", "hybrid", "mxfp8", "current", "block")]
                         + [("qwen3", "default"), ("qwen3", "mxfp8")])
def test_twins_are_deterministic_and_nearer_than_quantisation(family, scenario, capsys):
    p, x, dout, cfg = _layer_case(family)
    qa, qm = _quantisers(scenario, p, x, dout, cfg)
    ref = _run_layer(p, x, dout, cfg, qa, qm, M.F64)
    unq = _run_layer(p, x, dout, cfg, M.IdentityQ(), M.IdentityQ(), M.F64)   # (the bf16 roundings stay)
    twins = [_run_layer(p, x, dout, cfg, qa, qm, M.twin(s)) for s in M.TWIN_SEEDS]
    again = _run_layer(p, x, dout, cfg, qa, qm, M.twin(M.TWIN_SEEDS[1]))
    assert all(np.array_equal(again[n], twins[1][n]) for n in ref)            # deterministic per seed
    assert any(not np.array_equal(twins[0][n], twins[1][n]) for n in ref)     # ... and the seed matters
    lines = []
    for n in ref:
        e_ref = max(M.rel_err(t[n], ref[n]) for t in twins)
        d_q = M.rel_err(unq[n], ref[n])
        lines.append(f"  {n:4s} e_ref {e_ref:.2e}  quantised-vs-unquantised {d_q:.2e}")
        if d_q == 0.0:   # no quantiser upstream of this tensor (the fc2 bias gradient: column sums of the incoming gradient)
            assert e_ref <= M.BF16_FLOOR, (n, e_ref)
        else:
            assert e_ref < d_q, (n, e_ref, d_q)
    with capsys.disabled():
        print(f"\n[{family} {scenario}]\n" + "\n".join(lines))


def test_head_counts_only_the_labels_the_kernels_count():
    """A label at or past the vocabulary adds nothing to the sum and nothing to the count (mi_ce_forward ignores it)."""
    rng = np.random.default_rng(4)
    B, S, H, V = 2, 16, 64, 128
    cos, sin = G.rope_tables(S, 64, poison=False)
    cfg = M.Config(B, S, 1, 1, 64, 1e-5, cos, sin, rnd=M.ident)
    p = dict(table=rng.standard_normal((V, H)) * 0.05, norm=1.0 + 0.2 * rng.standard_normal(H))
    x = rng.standard_normal((B * S, H))
    labels = rng.integers(0, V, (B, S))
    labels[0, 3], labels[1, 5], labels[1, 9] = V, V + 7, -100
    got = M.head(p, x, labels, cfg, M.IdentityQ())
    clean = np.where((labels >= 0) & (labels < V), labels, -100)
    xt = torch.tensor(x, requires_grad=True)
    logits = torch.nn.functional.rms_norm(xt, (H,), torch.tensor(p["norm"]), 1e-5) @ torch.tensor(p["table"]).T
    want = torch.nn.functional.cross_entropy(logits, torch.from_numpy(M.shift_labels(clean)), ignore_index=-100)
    want.backward()
    assert abs(got["loss"] - want.item()) <= 1e-12 * abs(want.item())
    assert M.rel_err(got["dx"], xt.grad.numpy()) <= 1e-10
    wrong = M.head(p, x, labels, cfg, M.IdentityQ(), counted=lambda lab: (lab != -100).sum())
    assert abs(wrong["loss"] - want.item()) > 1e-3 * abs(want.item())        # the old denominator would be seen
