"""Attention core (csrc/mi_attn.hip: forward, dQ pass, dK/dV pass) against float64 where the kernels can go wrong: the models'
GQA ratio 4, odd numbers of 128-row blocks, S up to 4096, B / G / S/128 all different, known-answer softmax cases, a
distinct token stride per operand, and the shapes the launchers refuse."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import fp8_oracle as O
from tests.util import bf16_bits

pytestmark = pytest.mark.gpu

U32 = 2.0 ** -24  # fp32 unit roundoff
U16 = 2.0 ** -8   # bf16 unit roundoff
TINY = 2.0 ** -126  # smallest normal fp32 (and bf16): exp2 results and products below it may flush to 0


@pytest.fixture(scope="module")
def ops(dev):
    from llm_fp8_amd.pytorch import ops as _ops
    from llm_fp8_amd import _lib
    assert _lib.load().mi_device_supported() == 1, "not a gfx950 device"
    return _ops


def _f64(t: torch.Tensor) -> np.ndarray:
    return t.detach().double().cpu().numpy()


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


# ------------------------------------------------------------------------------------------------ distinct token strides
CANARY = 0x7FC1  # a bf16 quiet NaN: a kernel that reads padding with a wrong stride poisons its output


@pytest.mark.parametrize("D,causal", [(64, True), (128, True), (128, False)])
def test_distinct_token_strides_bitwise_and_canaries(ops, dev, D, causal):
    """q, k, v, o, dO, dQ, dK, dV each with its own token stride (padded by a different multiple of 8 elements): bitwise the
    contiguous call (same kernels, same summation order), and no padding element is touched."""
    B, S, H, G = 2, 384, 8, 2
    scale = D ** -0.5
    width = {"q": H, "k": G, "v": G, "o": H, "do": H, "dq": H, "dk": G, "dv": G}
    pad = {"q": 8, "k": 16, "v": 24, "o": 32, "do": 40, "dq": 48, "dk": 56, "dv": 64}
    ts = {n: width[n] * D + pad[n] for n in width}
    # every buffer holds B*S tokens at the LARGEST stride: a kernel that walks an operand with another operand's stride
    # reads wrong data inside the allocation instead of leaving it
    span = B * S * max(ts.values())
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

    lse_s = torch.full_like(lse_c, float("nan"))
    o_s, _ = ops.attn_fwd(view["q"], view["k"], view["v"], scale, causal, out=(view["o"], lse_s))
    assert o_s.data_ptr() == view["o"].data_ptr()
    dq_s, dk_s, dv_s = ops.attn_bwd(view["do"], view["q"], view["k"], view["v"], view["o"], lse_s, scale, causal,
                                    out=(view["dq"], view["dk"], view["dv"]))
    torch.cuda.synchronize()

    assert torch.equal(lse_s, lse_c), "lse"
    for n, got, ref in (("o", view["o"], o_c), ("dq", dq_s, dq_c), ("dk", dk_s, dk_c), ("dv", dv_s, dv_c)):
        assert torch.equal(got.view(torch.int16), ref.view(torch.int16)), f"{n}: strided call differs from the contiguous one"
    for n in ("q", "k", "v", "do"):
        assert torch.equal(bufs[n], before[n]), f"input {n} was written"
    for n in ("o", "dq", "dk", "dv"):
        outside = torch.ones(span, dtype=torch.bool, device=dev)
        outside.as_strided(shape[n], stride[n]).fill_(False)
        assert outside.sum().item() == span - B * S * width[n] * D
        assert (bufs[n][outside] == CANARY).all(), f"{n}: padding between tokens was written"


# ------------------------------------------------------------------------------------------------ known answer: q = 0
@pytest.mark.parametrize("B,S,H,G,D,causal", [(1, 4096, 4, 1, 64, True), (1, 4096, 8, 2, 128, True), (2, 640, 8, 2, 128, True),
                                              (3, 384, 4, 1, 64, True), (1, 1024, 8, 2, 64, False), (2, 384, 4, 1, 128, False)])
def test_zero_query_known_answer(ops, dev, B, S, H, G, D, causal):
    """q = 0: every visible score is exactly 0 and exp2(0) = 1, so row r sees n_r = r + 1 keys (causal; S otherwise) with
    weight 1 / n_r.  lse = log2(n_r), o[r] = mean(v[visible]), dv[k] = sum over the group's heads and q >= k of dO[q] / n_q,
    dk = 0.  An off-by-one on the diagonal changes n_r and shows as an lse error in that row."""
    rep = H // G
    scale = D ** -0.5
    g = torch.Generator(device=dev).manual_seed(S + D + B)
    q = torch.zeros(B, S, H, D, device=dev, dtype=torch.bfloat16)
    k, v = (torch.randn(B, S, G, D, device=dev, dtype=torch.bfloat16, generator=g) for _ in range(2))
    do = torch.randn(B, S, H, D, device=dev, dtype=torch.bfloat16, generator=g)
    o, lse = ops.attn_fwd(q, k, v, scale, causal)
    dq, dk, dv = ops.attn_bwd(do, q, k, v, o, lse, scale, causal)

    n = np.arange(1, S + 1, dtype=np.float64) if causal else np.full(S, float(S))
    lse_ref = np.broadcast_to(np.log2(n), (B, H, S))
    # lse = 0 * c + v_log_f32(l) with l = n_r summed exactly in fp32 (integers < 2^24): v_log_f32's error, within 4 ulps
    tol = 4 * np.spacing(np.maximum(lse_ref, 1.0).astype(np.float32)).astype(np.float64)
    err = np.abs(lse.double().cpu().numpy() - lse_ref)
    bad = np.argwhere(err > tol)
    assert bad.size == 0, f"lse off at {len(bad)} (b, h, row), first {bad[:5].tolist()}: got {lse[tuple(bad[0])].item()!r}"

    vd, dod = _f64(v), _f64(do)
    if causal:
        vsum, vabs = np.cumsum(vd, 1), np.cumsum(np.abs(vd), 1)
    else:
        vsum, vabs = np.broadcast_to(vd.sum(1, keepdims=True), vd.shape), np.broadcast_to(np.abs(vd).sum(1, keepdims=True), vd.shape)
    o_ref = np.repeat(vsum / n[None, :, None, None], rep, 2)
    # fp32 sum of n exact terms ((n - 1) u sum|v|), times fl(1 / l) and its product (2 u), then one bf16 rounding
    e = np.repeat((n[None, :, None, None] + 1) * U32 * vabs / n[None, :, None, None], rep, 2)
    tol = U16 * np.abs(o_ref) + (1 + U16) * e
    err = np.abs(_f64(o) - o_ref)
    assert (err <= tol).all(), f"o: {(err > tol).sum()} outside, worst row {np.unravel_index(np.argmax(err - tol), err.shape)}"

    w = dod / n[None, :, None, None]  # dO[q] / n_q
    wa = np.abs(w)
    if causal:
        dv_ref, dv_abs = np.flip(np.cumsum(np.flip(w, 1), 1), 1), np.flip(np.cumsum(np.flip(wa, 1), 1), 1)
    else:
        dv_ref, dv_abs = np.broadcast_to(w.sum(1, keepdims=True), w.shape), np.broadcast_to(wa.sum(1, keepdims=True), w.shape)
    dv_ref = dv_ref.reshape(B, S, G, rep, D).sum(3)
    dv_abs = dv_abs.reshape(B, S, G, rep, D).sum(3)
    # P = exp2(-lse) rounded to bf16 (2^-8 + 2^-16 from lse and exp2), an fp32 sum of rep * S products, one bf16 rounding
    e = (U16 + 2.0 ** -16 + rep * S * U32) * dv_abs
    tol = U16 * np.abs(dv_ref) + (1 + U16) * e
    err = np.abs(_f64(dv) - dv_ref)
    assert (err <= tol).all(), f"dv: {(err > tol).sum()} outside, worst (b, key, g, d) {np.unravel_index(np.argmax(err - tol), err.shape)}"
    assert not dk.any(), "dk must be exactly 0 (every dS is multiplied by q = 0)"
    assert torch.isfinite(dq).all()


# ------------------------------------------------------------------------------------------------ shape grid vs float64
# (B, S, H, G, D): rep 4 at both D; S / 128 = 3, 5, 7; S up to 4096 at B = 1; (4, 384, 8, 2) and (2, 640, 6, 3) have B, G and
# S / 128 pairwise different, so a workgroup id decomposed in the wrong order lands on a wrong (b, g)
GRID = [(1, 384, 8, 2, 64), (1, 640, 8, 2, 128), (2, 896, 4, 1, 64), (4, 384, 8, 2, 64), (2, 640, 6, 3, 128),
        (1, 1024, 4, 1, 128), (1, 2048, 2, 2, 128), (1, 4096, 2, 1, 64)]
NONCAUSAL = {(1, 384, 8, 2, 64), (2, 640, 6, 3, 128), (1, 1024, 4, 1, 128)}
GRID_CASES = [pytest.param(*s, True, id="-".join(map(str, s)) + "-causal") for s in GRID] + \
             [pytest.param(*s, False, id="-".join(map(str, s)) + "-full") for s in GRID if s in NONCAUSAL]


@pytest.mark.parametrize("B,S,H,G,D,causal", GRID_CASES)
def test_attn_grid_vs_float64(ops, dev, B, S, H, G, D, causal):
    q, k, v, do = _rand(B, S, H, G, D, seed=B * S + H * G + D + 1)
    scale = D ** -0.5
    o_ref, lse_ref = O.attention_f64(bf16_bits(q), bf16_bits(k), bf16_bits(v), scale, causal)
    qd, kd, vd, dod = (t.to(dev) for t in (q, k, v, do))
    o, lse = ops.attn_fwd(qd, kd, vd, scale, causal)
    _check_fwd(o, lse, o_ref, lse_ref, v, f"B{B} S{S} H{H} G{G} D{D} causal={causal}")
    # the backward takes delta = rowsum(dO * O) of the stored bf16 O just checked; the reference does the same (o_bits)
    refs = O.attention_bwd_f64(bf16_bits(q), bf16_bits(k), bf16_bits(v), bf16_bits(do), scale, causal, o_bits=bf16_bits(o))
    grads = ops.attn_bwd(dod, qd, kd, vd, o, lse, scale, causal)
    for got, ref, name in zip(grads, refs, ("dq", "dk", "dv")):
        _check_bwd(got, ref, name)


# ------------------------------------------------------------------------------------------------ adversarial softmax
def _adversarial(kind, B, S, H, G, D, seed):
    """bf16 (q, k, v, dO) whose scores s = scale q.k follow a pattern: feature 0 carries it, the rest is small noise."""
    g = torch.Generator().manual_seed(seed)
    scale = D ** -0.5
    c = scale * np.log2(np.e)  # score -> log2 units
    q = torch.randn(B, S, H, D, generator=g) * 0.25
    k = torch.randn(B, S, G, D, generator=g) * 0.25
    v = torch.randn(B, S, G, D, generator=g)
    do = torch.randn(B, S, H, D, generator=g) / 4
    if kind == "late_max":  # s rises 4 log2 units per 64-key tile: the running max moves up in every tile
        q[..., 0] = 8.0
        k[..., 0] = (torch.arange(S, dtype=torch.float32) * (4.0 / 64 / (8.0 * c)))[None, :, None]
    elif kind == "early_max":  # key 0 leads by 200 log2 units: every later p = 2^-200 underflows to 0 in fp32
        q[..., 0] = 8.0
        k[..., 0] = 0.0
        k[:, 0, :, 0] = 200.0 / (8.0 * c)
    elif kind == "sharp":  # scores of order 100 and more: P is nearly one-hot
        q = torch.randn(B, S, H, D, generator=g) * 8.0
        k = torch.randn(B, S, G, D, generator=g) * 8.0
    elif kind == "ties":  # integer q.k (exact in fp32) over three repeating key rows: every row's max is shared by S / 3 keys
        q = torch.randint(-1, 2, (B, S, H, D), generator=g).float()
        base = torch.randint(-1, 2, (B, 3, G, D), generator=g).float()
        k = base[:, torch.arange(S) % 3]
    return tuple(t.to(torch.bfloat16) for t in (q, k, v, do))


def _bwd_term_bounds(q, k, v, do, o_ref, scale, causal):
    """Per-element error bounds of (dq, dk, dv) from the sizes of the terms (float64), see test_attn_adversarial_bwd."""
    q, k, v, do = (_f64(t) for t in (q, k, v, do))
    B, S, H, D = q.shape
    G = k.shape[2]
    rep = H // G
    bq, bk, bv = np.zeros_like(q), np.zeros_like(k), np.zeros_like(v)
    mask = np.triu(np.ones((S, S), dtype=bool), 1)
    for h in range(H):
        gi = h // rep
        qh, kg, vg, doh, oh = q[:, :, h], k[:, :, gi], v[:, :, gi], do[:, :, h], o_ref[:, :, h]
        s = np.einsum("bqd,bkd->bqk", qh, kg) * scale
        mag = np.einsum("bqd,bkd->bqk", np.abs(qh), np.abs(kg))  # sum_d |q_d k_d|
        if causal:
            s = np.where(mask[None], -np.inf, s)
            mag = np.where(mask[None], 0.0, mag)
        p = np.exp(s - s.max(-1, keepdims=True))
        p /= p.sum(-1, keepdims=True)
        dp = np.einsum("bqd,bkd->bqk", doh, vg)
        dp_abs = np.einsum("bqd,bkd->bqk", np.abs(doh), np.abs(vg))
        delta = (doh * oh).sum(-1, keepdims=True)
        delta_abs = (np.abs(doh) * np.abs(oh)).sum(-1, keepdims=True)
        # relative error of the recomputed P: fp32 scores here and in the forward's lse (D u sum|q k| each, times scale)
        eps_p = 2 * scale * D * U32 * mag.max(-1, keepdims=True)
        # |dS~ - dS| <= [P (P -> bf16, dS -> bf16, eps_p, fp32 sums) + P underflow] (|dP| + |delta|) + P [fp32 dP + bf16 O in delta]
        a = ((p * (2 * U16 + eps_p + 2.0 ** -11) + TINY) * (np.abs(dp) + np.abs(delta))
             + p * (D * U32 * dp_abs + (U16 + D * U32) * delta_abs))
        bq[:, :, h] = scale * np.einsum("bqk,bkd->bqd", a, np.abs(kg))
        bk[:, :, gi] += scale * np.einsum("bqk,bqd->bkd", a, np.abs(qh))
        bv[:, :, gi] += np.einsum("bqk,bqd->bkd", p * (U16 + eps_p + 2.0 ** -11) + TINY, np.abs(doh))
    return bq, bk, bv


ADV_SHAPES = [(1, 1024, 8, 2, 64, True), (2, 384, 4, 1, 128, False)]


@pytest.mark.parametrize("kind", ["late_max", "early_max", "sharp", "ties"])
@pytest.mark.parametrize("B,S,H,G,D,causal", ADV_SHAPES)
def test_attn_adversarial_fwd(ops, dev, kind, B, S, H, G, D, causal):
    q, k, v, _ = _adversarial(kind, B, S, H, G, D, seed=S + D)
    scale = D ** -0.5
    o_ref, lse_ref = O.attention_f64(bf16_bits(q), bf16_bits(k), bf16_bits(v), scale, causal)
    o, lse = ops.attn_fwd(q.to(dev), k.to(dev), v.to(dev), scale, causal)
    _check_fwd(o, lse, o_ref, lse_ref, v, kind)


@pytest.mark.parametrize("kind", ["late_max", "early_max", "sharp", "ties"])
@pytest.mark.parametrize("B,S,H,G,D,causal", ADV_SHAPES)
def test_attn_adversarial_bwd(ops, dev, kind, B, S, H, G, D, causal):
    q, k, v, do = _adversarial(kind, B, S, H, G, D, seed=S + D + 1)
    scale = D ** -0.5
    o_ref, _ = O.attention_f64(bf16_bits(q), bf16_bits(k), bf16_bits(v), scale, causal)
    refs = O.attention_bwd_f64(bf16_bits(q), bf16_bits(k), bf16_bits(v), bf16_bits(do), scale, causal)
    bounds = _bwd_term_bounds(q, k, v, do, o_ref, scale, causal)
    qd, kd, vd, dod = (t.to(dev) for t in (q, k, v, do))
    o, lse = ops.attn_fwd(qd, kd, vd, scale, causal)
    grads = ops.attn_bwd(dod, qd, kd, vd, o, lse, scale, causal)
    for got, ref, bound, name in zip(grads, refs, bounds, ("dq", "dk", "dv")):
        # dS = P (dP - delta) cancels, so the bound comes from the terms: scale sum |dS~ - dS| |k or q| (dq, dk) or
        # sum P~ err |dO| (dv) per _bwd_term_bounds, plus one bf16 rounding of the output (or its flush below TINY)
        tol = U16 * np.abs(ref) + (1 + U16) * bound + TINY
        err = np.abs(_f64(got) - ref)
        assert (err <= tol).all(), (f"{kind} {name}: {(err > tol).sum()} / {err.size} outside the term bound, "
                                    f"worst {np.unravel_index(np.argmax(err - tol), err.shape)} err {err.max():.3g}, "
                                    f"max err / tol {(err / tol).max():.3g}")


# ------------------------------------------------------------------------------------------------ full size vs device fp32
def _torch_attn_fp32(q, k, v, scale, causal=True):
    """fp32 torch attention on the device (full sizes); q [B,S,H,D], k/v [B,S,G,D] -> (o [B,S,H,D], lse_log2 [B,H,S])."""
    B, S, H, D = q.shape
    G = k.shape[2]
    qf, kf, vf = (t.float().transpose(1, 2) for t in (q, k, v))
    kf, vf = kf.repeat_interleave(H // G, 1), vf.repeat_interleave(H // G, 1)
    s = (qf @ kf.transpose(-1, -2)) * scale
    if causal:
        s = s.masked_fill(torch.triu(torch.ones(S, S, dtype=torch.bool, device=q.device), 1), float("-inf"))
    lse2 = torch.logsumexp(s, -1) / np.log(2.0)
    return (torch.softmax(s, -1) @ vf).transpose(1, 2), lse2


@pytest.mark.parametrize("B,S,H,G,D", [(16, 512, 32, 8, 64), (8, 1024, 32, 8, 128), (8, 1024, 24, 8, 128)],
                         ids=["1B-b16-s512", "8B-b8-s1024", "3B-b8-s1024"])
def test_attn_full_size_vs_torch_fp32_and_reproducible(ops, dev, B, S, H, G, D):
    g = torch.Generator(device=dev).manual_seed(B + S + H + D)
    q, k, v = (torch.randn(B, S, n, D, device=dev, dtype=torch.bfloat16, generator=g) for n in (H, G, G))
    do = torch.randn(B, S, H, D, device=dev, dtype=torch.bfloat16, generator=g) / 4
    scale = D ** -0.5
    o, lse = ops.attn_fwd(q, k, v, scale, True)
    o2, lse2 = ops.attn_fwd(q, k, v, scale, True)
    dq, dk, dv = ops.attn_bwd(do, q, k, v, o, lse, scale, True)
    dq2, dk2, dv2 = ops.attn_bwd(do, q, k, v, o, lse, scale, True)
    assert torch.equal(o, o2) and torch.equal(lse, lse2)  # no atomics: bitwise reproducible
    assert torch.equal(dq, dq2) and torch.equal(dk, dk2) and torch.equal(dv, dv2)
    qr, kr, vr = (t.detach().float().requires_grad_(True) for t in (q, k, v))
    o_ref, lse_ref = _torch_attn_fp32(qr, kr, vr, scale, True)
    # the bounds of test_attn_fwd_strided_views_and_full_size / test_attn_bwd_full_size_vs_torch_autograd_and_reproducible
    assert torch.isfinite(o).all()
    err = (o.float() - o_ref).abs().max().item()
    assert err < 2 ** -6 * float(v.abs().max()), err
    assert (lse - lse_ref).abs().max().item() < 2e-3
    o_ref.backward(do.float())
    for got, ref, name in ((dq, qr.grad, "dq"), (dk, kr.grad, "dk"), (dv, vr.grad, "dv")):
        rel = ((got.float() - ref).norm() / ref.norm()).item()
        assert rel < 6e-3, f"{name}: {rel:.4g}"


# ------------------------------------------------------------------------------------------------ refusals
def _qkv(dev, B, S, H, G, D):
    return tuple(torch.randn(B, S, n, D, device=dev, dtype=torch.bfloat16) for n in (H, G, G))


def _fused(dev, B, S, H, G, D, extra):
    """q, k, v as column slices of one [B, S, (H + 2G) D + extra] buffer (token stride (H + 2G) D + extra)."""
    W = (H + 2 * G) * D + extra
    x = torch.randn(B, S, W, device=dev, dtype=torch.bfloat16)
    return (x[..., :H * D].view(B, S, H, D), x[..., H * D:(H + G) * D].view(B, S, G, D),
            x[..., (H + G) * D:(H + 2 * G) * D].view(B, S, G, D))


def _misaligned(dev, shape):
    """a contiguous bf16 tensor whose address is 2 bytes past a 16-byte boundary (token stride still a multiple of 8)."""
    flat = torch.randn(int(np.prod(shape)) + 8, device=dev).to(torch.bfloat16)
    t = flat[1:1 + int(np.prod(shape))].view(shape)
    assert t.data_ptr() % 16 == 2
    return t


def _case(name, dev):
    if name.startswith("S"):
        return _qkv(dev, 1, int(name[1:]), 4, 2, 64)
    if name.startswith("D"):
        return _qkv(dev, 1, 128, 4, 2, int(name[1:]))
    if name == "H6-G4":
        return _qkv(dev, 1, 128, 6, 4, 64)
    if name == "stride-not-8":
        return _fused(dev, 2, 128, 4, 2, 64, extra=4)
    q, k, v = _qkv(dev, 2, 128, 4, 2, 64)
    if name == "k-misaligned":
        return q, _misaligned(dev, k.shape), v
    assert name == "v-misaligned"
    return q, k, _misaligned(dev, v.shape)


REFUSED = ["S64", "S200", "S1000", "D32", "D96", "D256", "H6-G4", "stride-not-8", "k-misaligned", "v-misaligned"]


@pytest.mark.parametrize("name", REFUSED)
def test_launchers_and_flash_ok_refuse_the_same_shapes(ops, dev, name):
    from llm_fp8_amd.pytorch import attention as A
    q, k, v = _case(name, dev)
    B, S, H, D = q.shape
    assert not A._flash_ok(q, k, v, True, 0.0), name
    with pytest.raises(RuntimeError, match="mi_attn_fwd"):
        ops.attn_fwd(q, k, v, D ** -0.5, True)
    o = torch.zeros(B, S, H, D, device=dev, dtype=torch.bfloat16)
    lse = torch.zeros(B, H, S, device=dev)
    with pytest.raises(RuntimeError, match="mi_attn_bwd"):
        ops.attn_bwd(o, q, k, v, o, lse, D ** -0.5, True)


def test_launchers_refuse_misaligned_q_o_and_gradients(ops, dev):
    """The kernels make 16-byte accesses on q, o, dO, dQ, dK and dV as well: a misaligned one is refused, never launched."""
    from llm_fp8_amd.pytorch import attention as A
    B, S, H, G, D = 2, 128, 4, 2, 64
    scale = D ** -0.5
    q, k, v = _qkv(dev, B, S, H, G, D)
    lse = torch.zeros(B, H, S, device=dev)
    qm = _misaligned(dev, q.shape)
    assert not A._flash_ok(qm, k, v, True, 0.0)
    with pytest.raises(RuntimeError, match="mi_attn_fwd"):
        ops.attn_fwd(qm, k, v, scale, True)
    with pytest.raises(RuntimeError, match="mi_attn_fwd"):
        ops.attn_fwd(q, k, v, scale, True, out=(_misaligned(dev, q.shape), lse))
    o, lse = ops.attn_fwd(q, k, v, scale, True)
    do = torch.randn_like(o)
    outs = (torch.empty_like(q), torch.empty_like(k), torch.empty_like(v))
    bad = {"q": (do, qm, k, v, o, None), "o": (do, q, k, v, _misaligned(dev, o.shape), None),
           "do": (_misaligned(dev, o.shape), q, k, v, o, None),
           "dq": (do, q, k, v, o, (_misaligned(dev, q.shape), outs[1], outs[2])),
           "dk": (do, q, k, v, o, (outs[0], _misaligned(dev, k.shape), outs[2])),
           "dv": (do, q, k, v, o, (outs[0], outs[1], _misaligned(dev, v.shape)))}
    for name, (a_do, a_q, a_k, a_v, a_o, out) in bad.items():
        with pytest.raises(RuntimeError, match="mi_attn_bwd"):
            ops.attn_bwd(a_do, a_q, a_k, a_v, a_o, lse, scale, True, out=out)
    torch.cuda.synchronize()


def test_dot_product_attention_refused_shape_is_the_sdpa_route(dev):
    from llm_fp8_amd.pytorch import attention as A
    B, S, H, G, D = 2, 200, 4, 2, 64
    core = A.DotProductAttention(H, D, G, attention_dropout=0.0, attn_mask_type="causal", qkv_format="bshd")
    q, k, v = (t.requires_grad_(True) for t in _qkv(dev, B, S, H, G, D))
    assert not A._flash_ok(q, k, v, True, 0.0)
    o = core(q, k, v)
    go = torch.randn_like(o)
    o.backward(go)
    got = (o.detach(), q.grad.clone(), k.grad.clone(), v.grad.clone())
    q.grad = k.grad = v.grad = None
    ref = F.scaled_dot_product_attention(q.transpose(1, 2), k.transpose(1, 2), v.transpose(1, 2), is_causal=True,
                                         enable_gqa=True).transpose(1, 2).reshape(B, S, H * D)
    ref.backward(go)
    for a, b, name in zip(got, (ref.detach(), q.grad, k.grad, v.grad), ("o", "dq", "dk", "dv")):
        assert torch.equal(a, b), name


@pytest.mark.parametrize("layout", ["stride-not-8", "misaligned"])
def test_flash_backward_takes_any_grad_output_layout(dev, layout):
    """_FlashAttnFn.backward hands dO to the launcher only as an aligned view with a token stride of a multiple of 8; any
    other gradient layout is copied first, and the gradients are bitwise those of a contiguous dO."""
    from llm_fp8_amd.pytorch import attention as A
    B, S, H, G, D = 2, 256, 8, 2, 64
    core = A.DotProductAttention(H, D, G, attention_dropout=0.0, attn_mask_type="causal", qkv_format="bshd")
    q, k, v = (t.requires_grad_(True) for t in _qkv(dev, B, S, H, G, D))
    assert A._flash_ok(q, k, v, True, 0.0)
    go = torch.randn(B, S, H * D, device=dev, dtype=torch.bfloat16)
    core(q, k, v).backward(go)
    want = (q.grad.clone(), k.grad.clone(), v.grad.clone())
    q.grad = k.grad = v.grad = None
    if layout == "stride-not-8":
        go2 = torch.zeros(B, S, H * D + 4, device=dev, dtype=torch.bfloat16)[..., :H * D]
        go2.copy_(go)
        assert go2.stride(1) % 8 == 4
    else:
        go2 = _misaligned(dev, go.shape)
        go2.copy_(go)
    core(q, k, v).backward(go2)
    for a, b, name in zip((q.grad, k.grad, v.grad), want, ("dq", "dk", "dv")):
        assert torch.equal(a, b), name
