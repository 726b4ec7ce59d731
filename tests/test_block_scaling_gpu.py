"""GPU: Float8BlockScaling -- the block quantiser (1 x 128 and 128 x 128 power-of-two scales in the MX operand layout) against the
numpy restatement (tests/block_oracle.py), its row-block form and fused front ends, the MX GEMMs on its operands, and the recipe
through Linear, LayerNormLinear, LayerNormMLP and a training step."""
import numpy as np
import pytest
import torch

from oracle import fp8_oracle as O
from tests import block_oracle as B
from tests.util import assert_gemm_close, bf16_bits, u8

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops(dev):
    from llm_fp8_amd.pytorch import ops as _ops
    from llm_fp8_amd import _lib
    assert _lib.load().mi_device_supported() == 1, "not a gfx950 device"
    return _ops


def _np4(out):
    return tuple(None if t is None else u8(t) for t in out[:4])


def _s_colT_from_s_row(s_row):
    """128 x 128 blocks: the scale of the 32-group (rows 32 i.., column c) is the scale of (row 32 i, columns 32 (c // 32)..)."""
    return np.ascontiguousarray(np.repeat(s_row, 32, axis=0)[:, ::32].T)


def _edge_input(shape):
    """The input recipe of test_mxfp8_quantize_bitexact."""
    g = torch.Generator().manual_seed(shape[1])
    x = torch.randn(shape, generator=g) * torch.exp(torch.randn(shape[0], 1, generator=g) * 5)
    x[:, :32] = 0  # all-zero blocks
    if shape[1] >= 64:
        x[1, 40] = float("inf")
        x[2, 41] = float("nan")
        x[3, 33:64] = 1e-30
    x[5, 3] = float("nan")  # NaN inside an otherwise-zero block
    x[6, 7] = 3e38
    return x.to(torch.bfloat16)


# ------------------------------------------------------------------------------------------------------------ quantiser
@pytest.mark.parametrize("shape", [(32, 32), (128, 128), (160, 224), (256, 384), (1024, 3072)])
@pytest.mark.parametrize("fmt", [O.E4M3, O.E5M2])
@pytest.mark.parametrize("dim", [1, 2])
def test_blockfp8_quantize_bitexact(ops, dev, shape, fmt, dim):
    x = _edge_input(shape)
    want = B.quantize(bf16_bits(x), fmt, dim)
    xd = x.to(dev)
    got = _np4(ops.blockfp8_quantize(xd, fmt, dim))
    for name, a, b in zip(("y_row", "s_row", "y_colT", "s_colT"), got, want):
        np.testing.assert_array_equal(a, b, err_msg=f"{name} dim {dim}")
    assert max(got[1].max(), got[3].max()) <= 247
    yr, sr, yc, sc = ops.blockfp8_quantize(xd, fmt, dim, colwise=False)
    assert yc is None and sc is None
    np.testing.assert_array_equal(u8(yr), want[0])
    np.testing.assert_array_equal(u8(sr), want[1])
    yr, sr, yc, sc = ops.blockfp8_quantize(xd, fmt, dim, rowwise=False)
    assert yr is None and sr is None
    np.testing.assert_array_equal(u8(yc), want[2])
    np.testing.assert_array_equal(u8(sc), want[3])
    if dim == 2:
        np.testing.assert_array_equal(got[2], got[0].T)
        np.testing.assert_array_equal(got[3], _s_colT_from_s_row(got[1]))


@pytest.mark.parametrize("fmt", [O.E4M3, O.E5M2])
@pytest.mark.parametrize("dim", [1, 2])
def test_blockfp8_quantize_amax_epsilon(ops, dev, fmt, dim):
    x = _edge_input((160, 224))
    eps = 2.0 ** -10
    want = B.quantize(bf16_bits(x), fmt, dim, eps)
    plain = B.quantize(bf16_bits(x), fmt, dim)
    if dim == 1:  # (every 128 x 128 tile of this input has an amax above the epsilon; the 1 x 128 blocks of zeros and of 1e-30 do not)
        assert any((a != b).any() for a, b in zip(want, plain))  # the epsilon changes some block of this input
    got = _np4(ops.blockfp8_quantize(x.to(dev), fmt, dim, amax_epsilon=eps))
    for name, a, b in zip(("y_row", "s_row", "y_colT", "s_colT"), got, want):
        np.testing.assert_array_equal(a, b, err_msg=f"{name} dim {dim}")


@pytest.mark.parametrize("fmt", [O.E4M3, O.E5M2])
@pytest.mark.parametrize("dim", [1, 2])
def test_blockfp8_quantize_row_blocks_and_colsum(ops, dev, fmt, dim):
    """Parts quantised through `out=` views into one operand's buffers == quantising the bf16 concatenation (all four outputs, bit
    for bit), with the partial column sums each part emits; a 128 x 128 block destination 32 rows into its operand is refused."""
    g = torch.Generator().manual_seed(31)
    K = 384
    parts = [(torch.randn(n, K, generator=g) * s).to(torch.bfloat16).to(dev) for n, s in ((256, 1.0), (128, 30.0), (128, 1e-3))]
    N = sum(p.shape[0] for p in parts)
    ref = ops.blockfp8_quantize(torch.cat(parts, 0), fmt, dim)
    want = B.quantize(bf16_bits(torch.cat(parts, 0)), fmt, dim)
    for a, b in zip(ref, want):
        np.testing.assert_array_equal(u8(a), b)
    w8 = torch.zeros((N, K), dtype=torch.uint8, device=dev)
    sc = torch.zeros((K // 32, N), dtype=torch.uint8, device=dev)
    wt8 = torch.zeros((K, N), dtype=torch.uint8, device=dev)
    sct = torch.zeros((N // 32, K), dtype=torch.uint8, device=dev)
    r = 0
    for p in parts:
        n = p.shape[0]
        out = ops.blockfp8_quantize(p, fmt, dim, out=(w8[r:r + n], sc[:, r:r + n], wt8[:, r:r + n], sct[r // 32:(r + n) // 32]),
                                    want_colsum=True)
        cs = out[4]
        assert cs.shape == (n // 128, K)
        np.testing.assert_allclose(ops.colsum_finish(cs, torch.float32).cpu().numpy(), p.float().sum(0).cpu().numpy(), rtol=1e-5, atol=1e-4)
        r += n
    for got, ref_t in zip((w8, sc, wt8, sct), ref):
        assert torch.equal(got, ref_t)
    # row-only block
    w8b, scb = torch.zeros_like(w8), torch.zeros_like(sc)
    ops.blockfp8_quantize(parts[1], fmt, dim, rowwise=True, colwise=False, out=(w8b[256:384], scb[:, 256:384], None, None))
    assert torch.equal(w8b[256:384], ref[0][256:384]) and torch.equal(scb[:, 256:384], ref[1][:, 256:384])
    # 128 x 128 blocks: a destination that starts 32 rows into the operand would not hold the operand's blocks
    dest = (w8[32:160], sc[:, 32:160], wt8[:, 32:160], sct[1:5])
    if dim == 2:
        with pytest.raises(RuntimeError, match="multiple of 128 rows"):
            ops.blockfp8_quantize(parts[1], fmt, 2, out=dest)
    else:
        ops.blockfp8_quantize(parts[1], fmt, 1, out=dest)   # 1 x 128 blocks: any multiple of 32 rows is a valid row-block
        assert torch.equal(w8[32:160], ref[0][256:384])     # (the row-wise copy does not depend on the row offset)


@pytest.mark.parametrize("shape", B.FUSED_SHAPES)
@pytest.mark.parametrize("dim", [1, 2])
def test_blockfp8_fused_front_ends_vs_oracle(ops, dev, shape, dim):
    """The block quantiser fused with RMSNorm / SwiGLU / dSwiGLU, held to the criterion of test_mxfp8_fused_front_ends_vs_oracle
    against the oracle's *_device_order restatements (B.check_fused).  RMSNorm (no transcendental; the device's own rstd): scales
    and bytes identical.  SwiGLU / dSwiGLU (device v_exp_f32 against numpy's exp): a block scale may differ by one step only where
    fl32(fp8_max / amax) is within 2^-17 of a power of two, at most max(2, 1e-4 blocks) of them; with the device's scale every
    differing byte must be explained by O.fp8_mismatches_near_boundary (dsilu slack as in the MX test), at most max(2, 1e-3 size);
    dSwiGLU column sums: rtol 1e-4, atol 1e-4 max|dh| sqrt(R).  tests/test_block_scaling.py counts, on the CPU, how many reference
    blocks and values lie inside those bands for these inputs."""
    R, C = shape
    fmt = O.E4M3
    x, gamma, h, d = B.fused_inputs(shape)
    rstd = ops.rmsnorm_stats(x.to(dev), 1e-5)
    y32 = O.norm_apply_f32_device_order(bf16_bits(x), rstd.cpu().numpy(), bf16_bits(gamma))
    got = _np4(ops.blockfp8_norm_quantize(x.to(dev), rstd, gamma.to(dev), fmt, dim))
    print("norm", shape, dim, B.check_fused(got, y32, fmt, dim, "block norm", exact=True))
    for name, a, b in zip(("y_row", "s_row", "y_colT", "s_colT"), got, B.quantize_values(y32, fmt, dim)):
        np.testing.assert_array_equal(a, b, err_msg=f"norm {name}")
    hb, db = bf16_bits(h), bf16_bits(d)
    got = _np4(ops.blockfp8_swiglu_quantize(h.to(dev), fmt, dim))
    print("swiglu", shape, dim, B.check_fused(got, O.swiglu_f32_device_order(hb), fmt, dim, "block swiglu", exact=False))
    if dim == 2:
        np.testing.assert_array_equal(got[2], got[0].T)
        np.testing.assert_array_equal(got[3], _s_colT_from_s_row(got[1]))
    out = ops.blockfp8_dswiglu_quantize(h.to(dev), d.to(dev), fmt, dim, want_colsum=True)
    got = _np4(out)
    print("dswiglu", shape, dim, B.check_fused(got, O.dswiglu_f32_device_order(hb, db), fmt, dim, "block dswiglu", exact=False,
                                               slack=B.dswiglu_slack(hb, db)))
    if dim == 2:
        np.testing.assert_array_equal(got[2], got[0].T)
        np.testing.assert_array_equal(got[3], _s_colT_from_s_row(got[1]))
    dh = O.dswiglu_f32(hb, db)
    np.testing.assert_allclose(out[4].sum(0).cpu().numpy(), dh.astype(np.float64).sum(0), rtol=1e-4, atol=1e-4 * np.abs(dh).max() * np.sqrt(R))
    # one copy alone holds the bytes of the pair
    alone = ops.blockfp8_swiglu_quantize(h.to(dev), fmt, dim, rowwise=False)
    both = ops.blockfp8_swiglu_quantize(h.to(dev), fmt, dim)
    assert alone[0] is None and torch.equal(alone[2], both[2]) and torch.equal(alone[3], both[3])


# ------------------------------------------------------------------------------------------------------------ GEMM
def _rows_spread(shape, seed, spread):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * torch.exp(torch.randn(shape[0], 1, generator=g) * spread)).to(torch.bfloat16)


@pytest.mark.parametrize("mnk", [(128, 128, 128), (160, 224, 416), (256, 512, 1024)])
@pytest.mark.parametrize("fa,fb", [(O.E4M3, O.E4M3), (O.E5M2, O.E4M3)])
def test_gemm_mxfp8_on_block_scaled_operands(ops, dev, mnk, fa, fb):
    """A under 1 x 128 blocks, B under 128 x 128 blocks, quantised on the device: ops.gemm_mxfp8 reads the replicated scale bytes
    unchanged and is held against the float64 product of the dequantised operands within O.gemm_tolerance."""
    M, N, K = mnk
    a, b = _rows_spread((M, K), M + K, 2.0).to(dev), _rows_spread((N, K), N + 7, 0.5).to(dev)
    a8, sa, _, _ = ops.blockfp8_quantize(a, fa, 1, colwise=False)
    b8, sb, _, _ = ops.blockfp8_quantize(b, fb, 2, colwise=False)
    ref = (B.dequantize(u8(a8), u8(sa), fa) @ B.dequantize(u8(b8), u8(sb), fb).T).astype(np.float32)
    # and the operands are the restatement's, so the product is the recipe's
    np.testing.assert_array_equal(u8(a8), B.quantize(bf16_bits(a), fa, 1)[0])
    np.testing.assert_array_equal(u8(sb), B.quantize(bf16_bits(b), fb, 2)[1])
    d = ops.gemm_mxfp8(a8, sa, b8, sb, fa, fb)
    assert_gemm_close(d.float().cpu().numpy(), ref, f"block-scaled gemm {mnk}")
    full = (a.double() @ b.double().t()).cpu().numpy()
    assert np.sqrt(np.mean((d.double().cpu().numpy() - full) ** 2)) < 0.1 * np.sqrt(np.mean(full ** 2))


@pytest.mark.parametrize("fa,fb", [(O.E4M3, O.E4M3), (O.E5M2, O.E4M3)])
def test_grouped_launch_on_block_scaled_operands_equals_the_single_launches(ops, dev, fa, fb):
    """A Linear's dgrad + wgrad (256 tokens, 512 -> 1024) as one gemm_mxfp8_grouped launch: the bits of the two single launches."""
    M, K, N = 256, 512, 1024
    g = ops.blockfp8_quantize(_rows_spread((M, N), 1, 1.0).to(dev), fa, 1)
    x = ops.blockfp8_quantize(_rows_spread((M, K), 2, 1.0).to(dev), fb, 1)
    w = ops.blockfp8_quantize(_rows_spread((N, K), 3, 0.2).to(dev), fb, 2)
    dgrad, wgrad = (g[0], g[1], w[2], w[3]), (g[2], g[3], x[2], x[3])
    dx = torch.empty((M, K), dtype=torch.bfloat16, device=dev)
    dw = torch.empty((N, K), dtype=torch.bfloat16, device=dev)
    assert ops.grouped_gemm_ok(((M, K, N), (N, K, M)))
    ops.gemm_mxfp8_grouped([dgrad + (dx,), wgrad + (dw,)], fa, fb)
    assert torch.equal(dx, ops.gemm_mxfp8(*dgrad, fa, fb, algo=4))
    assert torch.equal(dw, ops.gemm_mxfp8(*wgrad, fa, fb, algo=4))
    assert_gemm_close(dx.float().cpu().numpy(),
                      (B.dequantize(u8(g[0]), u8(g[1]), fa) @ B.dequantize(u8(w[2]), u8(w[3]), fb).T).astype(np.float32), "grouped dx")


# ------------------------------------------------------------------------------------------------------------ modules
@pytest.fixture()
def te(dev):
    import llm_fp8_amd.pytorch as te_
    from llm_fp8_amd.pytorch.fp8 import FP8GlobalStateManager
    FP8GlobalStateManager.reset()
    yield te_
    FP8GlobalStateManager.reset()


def _f(t):
    return t.detach().float().cpu().numpy()


@pytest.mark.parametrize("fmt_name,fwd,bwd", [("E4M3", O.E4M3, O.E4M3), ("HYBRID", O.E4M3, O.E5M2)])
def test_linear_block_scaling_vs_oracle(te, dev, monkeypatch, fmt_name, fwd, bwd):
    """te.Linear(512 -> 768) on 256 tokens under Float8BlockScaling: y, dx and dW against the numpy restatement (quantise, GEMM,
    bf16) within O.gemm_tolerance; the forward and dgrad weight operands are byte transposes under the same scales; with
    is_first_microbatch the weight is quantised once per window; LLM_FP8_AMD_NO_GROUPED_GEMM=1 gives the same bits."""
    from llm_fp8_amd.common.recipe import Float8BlockScaling, Format
    from llm_fp8_amd.pytorch import module as M_
    recipe = Float8BlockScaling(fp8_format=getattr(Format, fmt_name))
    M, K, N = 256, 512, 768
    g = torch.Generator().manual_seed(8)
    lin = te.Linear(K, N, bias=True, params_dtype=torch.bfloat16, device=dev)
    with torch.no_grad():
        lin.weight.copy_((torch.randn(N, K, generator=g) * 0.05).to(torch.bfloat16))
        lin.bias.copy_(torch.randn(N, generator=g).to(torch.bfloat16))
    x = (torch.randn(M, K, generator=g) * torch.exp(torch.randn(M, 1, generator=g))).to(torch.bfloat16)
    dy = (torch.randn(M, N, generator=g) * torch.exp(torch.randn(M, 1, generator=g) * 2) / 32).to(torch.bfloat16)
    seen = []
    real_qw = M_._BlockQ.quantize_weights

    def counted(self, *a, **k):
        flat = real_qw(self, *a, **k)
        seen.append(flat)
        return flat

    monkeypatch.setattr(M_._BlockQ, "quantize_weights", counted)

    def run(first_mb=None):
        lin.weight.grad = lin.bias.grad = None
        xd = x.to(dev).requires_grad_(True)
        with te.fp8_autocast(enabled=True, fp8_recipe=recipe):
            y = lin(xd, is_first_microbatch=first_mb)
        y.backward(dy.to(dev))
        return y.detach(), xd.grad.detach(), lin.weight.grad.detach(), lin.bias.grad.detach()

    monkeypatch.delenv("LLM_FP8_AMD_NO_GROUPED_GEMM", raising=False)
    y, dx, dw, db = run()
    y_r, dx_r, dw_r, w_ref = B.linear_fwd_bwd(bf16_bits(x), bf16_bits(lin.weight), bf16_bits(dy), fwd, bwd, bf16_bits(lin.bias))
    assert_gemm_close(_f(y), y_r, "block y")
    assert_gemm_close(_f(dx), dx_r, "block dx")
    assert_gemm_close(_f(dw), dw_r, "block dw")
    np.testing.assert_allclose(_f(db), dy.double().sum(0).float().numpy(), rtol=2 ** -7, atol=1e-3)
    assert len(seen) == 1
    w8, sc, wt8, sct = seen[0]
    assert torch.equal(wt8, w8.t().contiguous())                       # ONE quantised weight for forward and dgrad
    np.testing.assert_array_equal(u8(sct), _s_colT_from_s_row(u8(sc)))
    for a, b in zip((w8, sc, wt8, sct), w_ref):
        np.testing.assert_array_equal(u8(a), b)
    # the micro-batch cache: one quantisation per window
    del seen[:]
    first = run(True)
    for _ in range(2):
        again = run(False)
        assert all(torch.equal(a, b) for a, b in zip(first, again))
    assert len(seen) == 1 and all(torch.equal(a, b) for a, b in zip(first, (y, dx, dw, db)))
    lin._wcache.clear()
    monkeypatch.setenv("LLM_FP8_AMD_NO_GROUPED_GEMM", "1")
    assert all(torch.equal(a, b) for a, b in zip(run(), (y, dx, dw, db)))


def _rms(a, b):
    return float((a.double() - b.double()).pow(2).mean().sqrt())


def _module_runs(te, dev, kind, fused, recipe):
    """Outputs and gradients of the module under `recipe`, and the fp64 evaluation with FP8 disabled (the runs of
    test_current_scaling_gpu._module_runs with the recipe as a parameter)."""
    from llm_fp8_amd.pytorch.fp8 import FP8GlobalStateManager
    FP8GlobalStateManager.reset()
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
    with te.fp8_autocast(enabled=True, fp8_recipe=recipe):
        y = mod(xd)
    y.backward(dy)
    torch.cuda.synchronize()
    out = {"y": y.detach(), "dx": xd.grad.detach()}
    out.update({n: p.grad.detach() for n, p in mod.named_parameters()})
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
def test_modules_against_fp64_and_the_existing_recipes(te, dev, kind):
    """LayerNormLinear (RMSNorm, 512 -> 768) and LayerNormMLP (512, FFN 1024, swiglu, bias) on 256 tokens, the fused route and the
    route with both fusions off, against an fp64 evaluation with FP8 disabled.  Every output and gradient: RMS error below 0.1 x
    the rms of the value, and at most 1.25 x the larger of the errors the `mxfp8` and `current` recipes (existing code: the
    reference) give for the same module, inputs and route -- FP8's relative rounding error does not depend on the scale granularity
    on this data; the 25 % are the margin test_fused_modules_against_their_unfused_routes grants.  A second run gives the same bits."""
    from llm_fp8_amd.common.recipe import Float8BlockScaling, Float8CurrentScaling, MXFP8BlockScaling
    for fused in (True, False):
        blk, ref = _module_runs(te, dev, kind, fused, Float8BlockScaling())
        mx, ref_m = _module_runs(te, dev, kind, fused, MXFP8BlockScaling())
        cur, ref_c = _module_runs(te, dev, kind, fused, Float8CurrentScaling())
        assert sorted(blk) == sorted(mx) == sorted(cur) == sorted(ref)
        failed = []
        for name in sorted(blk):
            assert torch.equal(ref[name], ref_m[name]) and torch.equal(ref[name], ref_c[name]), name
            eb, em, ec = (_rms(t[name], ref[name]) for t in (blk, mx, cur))
            scale = float(ref[name].pow(2).mean().sqrt())
            print(f"{kind} {'fused' if fused else 'unfused'} {name}: rms error block {eb:.4e} mxfp8 {em:.4e} current {ec:.4e} "
                  f"(rms of the value {scale:.4e}) block / max(mxfp8, current) {eb / max(em, ec):.4f}")
            assert 0 < eb < 0.1 * scale, name
            if eb > 1.25 * max(em, ec):
                failed.append((name, eb, em, ec))
        assert not failed, failed
        again, _ = _module_runs(te, dev, kind, fused, Float8BlockScaling())
        for name in blk:
            assert torch.equal(again[name], blk[name]), (name, fused)


# ------------------------------------------------------------------------------------------------------------ training step
def _tiny_cfg(train, scenario, ga=1, **kw):
    return train.TrainingConfig(model_name="llama-3.2-3b", batch_size=2, max_seq_length=128, mixed_precision="fp8",
                                fp8_scenario=scenario, use_te=True, sharding_mode="none", num_hidden_layers=2, vocab_size=512,
                                learning_rate=1e-3, num_warmup_steps=0, gradient_accumulation_steps=ga, **kw)


def test_training_step_end_to_end(dev, monkeypatch, tmp_path):
    """The tiny model of test_current_scaling_gpu.py::test_training_step_end_to_end (2 layers, hidden 512, 4 heads of 128, 2 KV heads,
    FFN 1024, vocab 512, batch 2 x 128) under scenario `block`: three steps stay finite and the third loss is below the first; the
    step-0 loss deviates from the bf16 loss of the same weights by at most 2 x the larger of the deviations of `mxfp8` and
    `current`; with gradient_accumulation_steps = 2 the weights are quantised once per window; save_pretrained + reload give an
    empty _extra_state and the same step-0 loss."""
    import llm_fp8_amd.pytorch as te
    from llm_fp8_amd import llama, train
    from llm_fp8_amd.pytorch import module as M
    from llm_fp8_amd.pytorch.fp8 import FP8GlobalStateManager as G
    device = torch.device(dev)
    orig_cfg = llama.llama_config
    monkeypatch.setattr(llama, "llama_config", lambda name, **kw: orig_cfg(name, **{**dict(
        hidden_size=512, intermediate_size=1024, num_attention_heads=4, num_key_value_heads=2, head_dim=128), **kw}))
    calls = {"n": 0}
    real_qw = M._BlockQ.quantize_weights

    def counted(self, *a, **k):
        calls["n"] += 1
        return real_qw(self, *a, **k)

    monkeypatch.setattr(M._BlockQ, "quantize_weights", counted)
    gen = torch.Generator(device=device).manual_seed(12)
    batch = train.synthetic_batch(_tiny_cfg(train, "block"), 512, device, gen)
    half = [{k: v[i:i + 1] for k, v in batch.items()} for i in range(2)]
    state = {}

    def build(scenario, ga=1, **kw):
        G.reset()
        cfg = _tiny_cfg(train, scenario, ga, **kw)
        torch.manual_seed(31)
        model = train.prepare_model(train.create_model(cfg, device), cfg)
        if "load_dir" not in kw:
            if state:
                model.load_state_dict(state["sd"], strict=False)
            else:
                state["sd"] = {k: v.clone() for k, v in model.state_dict().items() if not k.endswith("_extra_state")}
        model.train()
        return model, cfg

    def steps(scenario, ga=1, n=3):
        model, cfg = build(scenario, ga)
        opt, sched = train.create_optimizer(model, cfg)
        calls["n"] = 0
        losses = [train.train_step(model, batch if ga == 1 else half, opt, sched, cfg).item() for _ in range(n)]
        return losses, calls["n"]

    def loss0(model):
        with torch.no_grad():
            return model(**batch).loss.item()

    try:
        blk, n_blk = steps("block")
        mx, _ = steps("mxfp8", n=1)
        cur, _ = steps("current", n=1)
        real_autocast = te.fp8_autocast
        monkeypatch.setattr(te, "fp8_autocast", lambda enabled=True, **kw: real_autocast(enabled=False, **kw))
        ref = loss0(build("block")[0])
        monkeypatch.setattr(te, "fp8_autocast", real_autocast)
        blk2, n_blk2 = steps("block", ga=2)
        # save_pretrained and a reload: no FP8 state to carry, the same step-0 loss
        model, cfg = build("block", output_dir=str(tmp_path / "ckpt"))
        extra = {k: v for k, v in model.state_dict().items() if k.endswith("_extra_state")}
        assert extra and all(v.numel() == 0 for v in extra.values())
        before = loss0(model)
        train.save_model(model, cfg)
        del model
        model2, _ = build("block", load_dir=str(tmp_path / "ckpt"))
        extra2 = {k: v for k, v in model2.state_dict().items() if k.endswith("_extra_state")}
        assert extra2 and all(v.numel() == 0 for v in extra2.values())
        after = loss0(model2)
    finally:
        G.reset()
    dev_blk, dev_mx, dev_cur = abs(blk[0] - ref), abs(mx[0] - ref), abs(cur[0] - ref)
    print(f"losses block {blk}; accumulated {blk2}; step-0 loss bf16 {ref:.6f} block {blk[0]:.6f} mxfp8 {mx[0]:.6f} current {cur[0]:.6f}: "
          f"|block - bf16| = {dev_blk:.3e}, |mxfp8 - bf16| = {dev_mx:.3e}, |current - bf16| = {dev_cur:.3e}; "
          f"quantize_weights calls {n_blk} / {n_blk2}; reload {before:.6f} -> {after:.6f}")
    assert all(np.isfinite(blk)) and blk[2] < blk[0], blk
    assert all(np.isfinite(blk2)) and blk2[2] < blk2[0], blk2
    sites = 2 * 4 + 1                              # per layer q|k|v, proj, fc1, fc2; the lm_head
    assert n_blk == 3 * sites, n_blk               # every forward quantises every weight operand once
    assert n_blk2 == 3 * sites, n_blk2             # two micro-batches per step, ONE quantisation per window
    assert dev_blk <= 2 * max(dev_mx, dev_cur), (dev_blk, dev_mx, dev_cur)
    assert before == after, (before, after)
