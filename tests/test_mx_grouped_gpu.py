"""GPU: mi_gemm_mxfp8_grouped (a Linear's block-scaled dgrad + wgrad in one persistent launch) -- every problem's output is bit
for bit what mi_gemm_mxfp8(algo 4) writes for it alone, poison stays in its row / column of its own problem, and the module
layer computes the same bits with the grouped launch as with two launches."""
import numpy as np
import pytest
import torch

from oracle import fp8_oracle as O
from tests.util import assert_gemm_close

pytestmark = pytest.mark.gpu

TILES = ((256, 256), (256, 192), (192, 256), (192, 192))
FMTS = [(O.E4M3, O.E4M3), (O.E5M2, O.E4M3)]
# the group list of test_kernels_gpu.py (per-tensor grouped GEMM)
GROUPS = [
    [(512, 768, 512), (768, 512, 512)],
    [(2048, 1024, 768), (1024, 768, 2048), (512, 512, 1280)],  # three problems, K-tile counts 6, 16, 10
    [(512, 768, 256), (768, 256, 512)],                       # K 256 vs 512
    [(2048, 768, 1024), (1024, 768, 2048)],                   # 192-column tiles
    [(4096, 3072, 3072), (3072, 3072, 4096)],                 # o-proj backward at M = 4096: > 1 round, mixed K
    [(1536, 1536, 256), (768, 384, 1024), (384, 1920, 512)],  # three problems, 192 x 192 tiles
    [(8192, 3072, 8192), (8192, 3072, 8192)],                 # fc2 backward of Llama-3.2-3B at full size
    [(256, 256, 256)],                                        # a single problem, a single tile
]
SMALL = 768 * 1024 * 1024  # M N K up to which a problem is also compared with the oracle


@pytest.fixture()
def ops(dev):
    from llm_fp8_amd.pytorch import ops as ops_
    return ops_


def _operands(group, fa, fb, dev, seed):
    """Per problem (a8, sa, b8, sb, out): random data bytes with the NaN / Inf encodings masked as the per-tensor grouped test does,
    random E8M0 bytes in 124..130 (block scales 2^-3 .. 2^3), outputs pre-filled with NaN.
    Finite: |data| < 64 after the mask, so a K = 8192 sum stays below 2^13 * 2^12 * 2^6 = 2^31, far inside bf16 (also checked on
    the oracle for the small problems).
    Why not wider: the scale PRODUCTS of one dot product then span 2^12, inside the ~2^14 alignment window of the scaled MFMA that
    the project's fp32 bound for this instruction (7 * 2^-14 * sum |a||b|, test_kernels_gpu.py) documents.  With a wider band an
    output dominated by its largest scale products, and cancelling there, carries the truncation of everything else as an error
    the GEMM tolerance (2^-7 |ref| + 1e-3 rms, made for operands of one magnitude) does not allow for -- in the single launch
    just the same: at 119..135 mi_gemm_mxfp8(algo 4) alone sits at 0.97 of that tolerance, at 124..130 and below at the 0.5 that
    is the bf16 rounding of the output."""
    g = torch.Generator(device=dev).manual_seed(seed)
    probs = []
    for (M, N, K) in group:
        a8 = torch.randint(0, 256, (M, K), generator=g, device=dev, dtype=torch.uint8)
        b8 = torch.randint(0, 256, (N, K), generator=g, device=dev, dtype=torch.uint8)
        for t, f in ((a8, fa), (b8, fb)):
            if f == O.E4M3:
                t[(t & 0x7F) >= 0x68] &= 0xBF
            else:
                t[(t & 0x7F) >= 0x54] &= 0xCF
        sa = torch.randint(124, 131, (K // 32, M), generator=g, device=dev, dtype=torch.uint8)
        sb = torch.randint(124, 131, (K // 32, N), generator=g, device=dev, dtype=torch.uint8)
        out = torch.full((M, N), float("nan"), dtype=torch.bfloat16, device=dev)
        probs.append((a8, sa, b8, sb, out))
    return probs


def _bits(t):
    return t.view(torch.int16)


def _oracle(p, fa, fb):
    a8, sa, b8, sb, _ = p
    n = lambda t: t.cpu().numpy()
    return O.gemm_mxfp8_tn(n(a8), np.ascontiguousarray(n(sa).T), n(b8), np.ascontiguousarray(n(sb).T), fa, fb, out_f32=True)


def _cfgs_that_divide(group):
    return [-1] + [c for c, (bm, bn) in enumerate(TILES) if all(M % bm == 0 and N % bn == 0 for M, N, K in group)]


def test_premise_single_mx_kernel_gives_one_set_of_bits_for_every_tile_shape(ops, dev):
    """mi_gemm_mxfp8 algos 40-43 (and 4) on a shape all four tile shapes divide: identical bits.  The bitwise criterion below
    (against algo 4, whatever the grouped tile shape) rests on this."""
    for fa, fb in FMTS:
        (a8, sa, b8, sb, _), = _operands([(1536, 1536, 512)], fa, fb, dev, 3 + fa)
        ref = ops.gemm_mxfp8(a8, sa, b8, sb, fa, fb, algo=4)
        for algo in (40, 41, 42, 43):
            assert torch.equal(_bits(ops.gemm_mxfp8(a8, sa, b8, sb, fa, fb, algo=algo)), _bits(ref)), (algo, fa, fb)


@pytest.mark.parametrize("group", GROUPS)
@pytest.mark.parametrize("fa,fb", FMTS)
def test_grouped_mx_gemm_is_bitwise_the_single_launch(ops, dev, group, fa, fb):
    probs = _operands(group, fa, fb, dev, len(group) * 7 + fa)
    alone = [ops.gemm_mxfp8(a8, sa, b8, sb, fa, fb, algo=4) for a8, sa, b8, sb, _ in probs]
    refs = [_oracle(p, fa, fb) if M * N * K <= SMALL else None for p, (M, N, K) in zip(probs, group)]
    for r in refs:
        assert r is None or np.isfinite(r).all()  # the scale band keeps the reference itself finite
    for cfg in _cfgs_that_divide(group):  # the library's choice and every explicit tile shape that divides the group
        for p in probs:
            p[4].fill_(float("nan"))
        ops.gemm_mxfp8_grouped(probs, fa, fb, tile_cfg=cfg)
        for p, one, ref, (M, N, K) in zip(probs, alone, refs, group):
            assert torch.equal(_bits(p[4]), _bits(one)), f"problem {M}x{N}x{K} (tile cfg {cfg}) differs from its own launch"
            if ref is not None:
                assert_gemm_close(p[4].float().cpu().numpy(), ref, f"grouped mx {M}x{N}x{K} cfg {cfg}")


@pytest.mark.parametrize("fa,fb", FMTS)
def test_explicit_tile_shape_that_does_not_divide_is_refused_not_replaced(ops, dev, fa, fb):
    probs = _operands([(512, 768, 512), (768, 512, 512)], fa, fb, dev, 1)
    with pytest.raises(RuntimeError, match="does not fit tile shape"):
        ops.gemm_mxfp8_grouped(probs, fa, fb, tile_cfg=3)
    with pytest.raises(RuntimeError, match="tile_cfg 4"):
        ops.gemm_mxfp8_grouped(probs, fa, fb, tile_cfg=4)
    assert all(torch.isnan(p[4]).all() for p in probs)  # nothing was launched


@pytest.mark.parametrize("fa,fb", FMTS)
@pytest.mark.parametrize("cfg", [0, 3])
def test_poison_stays_in_its_row_or_column_of_its_own_problem(ops, dev, fa, fb, cfg):
    """One NaN data byte and one 0xFF scale byte in problem 0 of a two-problem group: exactly that row / column of problem 0 is
    non-finite, everything else keeps its clean bits, and problem 1 is bitwise its clean run."""
    group = [(768, 1536, 512), (1536, 768, 768)]
    probs = _operands(group, fa, fb, dev, 17 + fa)
    ops.gemm_mxfp8_grouped(probs, fa, fb, tile_cfg=cfg)
    clean = [p[4].clone() for p in probs]
    assert all(torch.isfinite(c).all() for c in clean)
    a8, sa, b8, sb, out0 = probs[0]
    row, col = 389, 1201
    for where in ("A data", "A scale", "B data", "B scale"):
        saved = [t.clone() for t in (a8, sa, b8, sb)]
        if where == "A data":
            a8[row, 77] = 0x7F
        elif where == "A scale":
            sa[5, row] = 0xFF
        elif where == "B data":
            b8[col, 300] = 0x7F
        else:
            sb[9, col] = 0xFF
        for p in probs:
            p[4].fill_(0)
        ops.gemm_mxfp8_grouped(probs, fa, fb, tile_cfg=cfg)
        bad = ~torch.isfinite(out0)
        want = torch.zeros_like(bad)
        if where.startswith("A"):
            want[row, :] = True
        else:
            want[:, col] = True
        assert torch.equal(bad, want), where
        assert torch.equal(_bits(out0)[~want], _bits(clean[0])[~want]), where
        assert torch.equal(_bits(probs[1][4]), _bits(clean[1])), where
        for t, s in zip((a8, sa, b8, sb), saved):
            t.copy_(s)


@pytest.mark.parametrize("fa,fb", FMTS)
@pytest.mark.parametrize("k_in,n_out", [(3072, 5120), (3072, 3072), (3072, 16384), (8192, 3072)])
def test_full_size_3b_backward_pairs(ops, dev, k_in, n_out, fa, fb):
    """q|k|v, o-proj, fc1 and fc2 of Llama-3.2-3B at 8192 tokens: dgrad [M, in] = G [M, out] . WT [in, out]^T and
    wgrad [out, in] = GT [out, M] . XT [in, M]^T in one launch, bitwise the two single launches."""
    M = 8192
    group = [(M, k_in, n_out), (n_out, k_in, M)]
    probs = _operands(group, fa, fb, dev, k_in + n_out + fa)
    ops.gemm_mxfp8_grouped(probs, fa, fb)
    for (a8, sa, b8, sb, out), shape in zip(probs, group):
        assert torch.equal(_bits(out), _bits(ops.gemm_mxfp8(a8, sa, b8, sb, fa, fb, algo=4))), shape


def test_grouped_mx_launch_is_reproducible_under_load(ops, dev):
    """The same grouped launch again and again while another stream runs a GEMM: identical bits (no race between the two wave
    groups on the staged block scales across a problem switch)."""
    fa, fb = O.E5M2, O.E4M3
    group = [(8192, 3072, 5120), (5120, 3072, 8192)]
    probs = _operands(group, fa, fb, dev, 5)
    (la, lsa, lb, lsb, lout), = _operands([(4096, 4096, 1024)], fa, fb, dev, 6)
    ops.gemm_mxfp8_grouped(probs, fa, fb)
    ref = [p[4].clone() for p in probs]
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    for _ in range(6):
        with torch.cuda.stream(side):
            for _ in range(4):
                ops.gemm_mxfp8(la, lsa, lb, lsb, fa, fb, out=lout, algo=4)
        for p in probs:
            p[4].fill_(float("nan"))
        ops.gemm_mxfp8_grouped(probs, fa, fb)
        torch.cuda.synchronize()
        for p, r in zip(probs, ref):
            assert torch.equal(_bits(p[4]), _bits(r))


def _force_grouped(monkeypatch, ops_, calls):
    """Every eligible site takes the grouped launch (through the autotune, as the per-tensor twin of this test does)."""
    monkeypatch.delenv("LLM_FP8_AMD_NO_GROUPED_GEMM", raising=False)
    monkeypatch.delenv("LLM_FP8_AMD_GROUPED_GEMM", raising=False)

    real = ops_.grouped_gemm_autotune

    def autotune(problems, fa, fb, iters=3, mx=False):
        # a block-scaled group (second operand slot: the [K/32, M] scales of the first) must ask for the block-scaled candidates
        # and cache entry, a per-tensor one (the model's delayed-scaling Linear) must not
        a, sa = problems[0][:2]
        assert mx is (sa.shape == (a.shape[1] // 32, a.shape[0]))
        if not mx:
            return real(problems, fa, fb, iters, mx=False)  # measured, as it is without this stand-in
        return 0 if all(a.shape[0] % 256 == 0 and b.shape[0] % 256 == 0 for a, _, b, _, _ in problems) else 3

    monkeypatch.setattr(ops_, "grouped_gemm_autotune", autotune)
    orig = ops_.gemm_mxfp8_grouped
    monkeypatch.setattr(ops_, "gemm_mxfp8_grouped", lambda *a, **k: (calls.__setitem__("n", calls["n"] + 1), orig(*a, **k))[1])
    return orig


def test_grouped_mx_backward_gemms_change_nothing(dev, monkeypatch):
    """module._grouped_or_two: the MXFP8 recipe with every eligible backward pair as ONE grouped launch against
    LLM_FP8_AMD_NO_GROUPED_GEMM=1: identical losses and parameter bits after 3 optimiser steps."""
    from llm_fp8_amd import train
    from llm_fp8_amd.pytorch.fp8 import FP8GlobalStateManager as G
    from llm_fp8_amd.pytorch import ops as ops_

    def run(grouped):
        G.reset()
        calls = {"n": 0}
        orig = None
        if grouped:
            orig = _force_grouped(monkeypatch, ops_, calls)
        else:
            monkeypatch.setenv("LLM_FP8_AMD_NO_GROUPED_GEMM", "1")
            real = ops_.gemm_mxfp8_grouped
            monkeypatch.setattr(ops_, "gemm_mxfp8_grouped", lambda *a, **k: (calls.__setitem__("n", calls["n"] + 1), real(*a, **k))[1])
        cfg = train.TrainingConfig(model_name="llama-3.2-3b", batch_size=2, max_seq_length=384, mixed_precision="fp8",
                                   fp8_scenario="mxfp8", use_te=True, sharding_mode="none", num_hidden_layers=2, vocab_size=3072,
                                   learning_rate=1e-3, num_warmup_steps=0)
        torch.manual_seed(31)
        device = torch.device(dev)
        model = train.prepare_model(train.create_model(cfg, device), cfg)
        opt, sched = train.create_optimizer(model, cfg)
        model.train()
        gen = torch.Generator(device=device).manual_seed(12)
        losses = [train.train_step(model, train.synthetic_batch(cfg, 3072, device, gen), opt, sched, cfg).item() for _ in range(3)]
        flat = torch.cat([p.detach().reshape(-1).view(torch.int16) for p in model.parameters()]).clone()
        monkeypatch.undo()
        return losses, flat, calls["n"]

    try:
        l1, w1, n1 = run(True)
        l0, w0, n0 = run(False)
    finally:
        G.reset()
    assert n1 >= 3 * 2 * 4 and n0 == 0, (n1, n0)   # 3 steps x 2 layers x (q|k|v, proj, fc2, fc1) grouped launches
    assert l1 == l0, (l1, l0)
    assert torch.equal(w1, w0)


def test_hybrid_mx_linear_grouped_backward_bits(dev, monkeypatch):
    """MXFP8BlockScaling(fp8_format=HYBRID) Linear (E5M2 grad_output x E4M3 weights / activations) at a shape the grouped kernel
    takes: dgrad and wgrad from one grouped launch are bitwise those of two launches."""
    import llm_fp8_amd.pytorch as te
    from llm_fp8_amd.common.recipe import Format, MXFP8BlockScaling
    from llm_fp8_amd.pytorch.fp8 import FP8GlobalStateManager as G
    from llm_fp8_amd.pytorch import ops as ops_
    recipe = MXFP8BlockScaling(fp8_format=Format.HYBRID)
    M, K, N = 512, 768, 1024
    g = torch.Generator().manual_seed(18)
    w = (torch.randn(N, K, generator=g) * 0.05).to(torch.bfloat16)
    x = (torch.randn(M, K, generator=g) * torch.exp(torch.randn(M, 1, generator=g))).to(torch.bfloat16)
    dy = (torch.randn(M, N, generator=g) * torch.exp(torch.randn(M, 1, generator=g) * 2) / 32).to(torch.bfloat16)

    def run(grouped):
        G.reset()
        calls = {"n": 0, "fmts": None}
        if grouped:
            orig = _force_grouped(monkeypatch, ops_, calls)
            monkeypatch.setattr(ops_, "gemm_mxfp8_grouped", lambda probs, fa, fb, **k: (
                calls.__setitem__("n", calls["n"] + 1), calls.__setitem__("fmts", (fa, fb)), orig(probs, fa, fb, **k))[2])
        else:
            monkeypatch.setenv("LLM_FP8_AMD_NO_GROUPED_GEMM", "1")
        lin = te.Linear(K, N, bias=False, params_dtype=torch.bfloat16, device=dev)
        with torch.no_grad():
            lin.weight.copy_(w)
        xd = x.to(dev).requires_grad_(True)
        with te.fp8_autocast(enabled=True, fp8_recipe=recipe):
            y = lin(xd)
        y.backward(dy.to(dev))
        torch.cuda.synchronize()
        monkeypatch.undo()
        return xd.grad.clone(), lin.weight.grad.clone(), calls

    try:
        dx1, dw1, c1 = run(True)
        dx0, dw0, c0 = run(False)
    finally:
        G.reset()
    assert c1["n"] == 1 and c1["fmts"] == (O.E5M2, O.E4M3) and c0["n"] == 0
    assert torch.isfinite(dx1).all() and torch.isfinite(dw1).all()
    assert torch.equal(_bits(dx1), _bits(dx0)) and torch.equal(_bits(dw1), _bits(dw0))
