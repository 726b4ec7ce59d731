"""GPU parity of the non-GEMM kernels of the step at the widths and sizes the step runs them, against float64 references:
RMSNorm backward at every width its dispatcher accepts, fused cross-entropy at the full Llama-3 vocabulary and at the edge
rows (masked -inf logits, ignored / out-of-range labels, saturating values), ClippedAdamW against a one-step float64 AdamW
on tensors that straddle the 64 Ki-element chunk, and RoPE at the 3B / 1B attention shapes (a second round of the
grid-stride loop)."""
import math

import numpy as np
import pytest
import torch

from oracle import fp8_oracle as O
from tests.util import bf16_bits, bits_to_bf16

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops(dev):
    from llm_fp8_amd.pytorch import ops as _ops
    from llm_fp8_amd import _lib
    assert _lib.load().mi_device_supported() == 1, "not a gfx950 device"
    return _ops


def _lib():
    from llm_fp8_amd import _lib as L
    return L


def _bf16_ulp(x: np.ndarray) -> np.ndarray:
    """Spacing of bf16 at |x| (8 significand bits), float64; bf16's smallest normal spacing below 2^-126."""
    e = np.floor(np.log2(np.maximum(np.abs(x), 2.0 ** -126)))
    return 2.0 ** (e - 7)


# ----------------------------------------------------------------------------------------- A: RMSNorm backward
# cols / 512 of every MI_RB(NVEC, WPR) instance of mi_rmsnorm_bwd (mi_fused.hip); test_host_logic checks this list against
# the dispatcher, so an instance added there without a test here fails on any machine
RB_VECS = (1, 2, 3, 4, 5, 6, 7, 8, 10, 12, 14, 16)
RB_WIDTHS = tuple(512 * v for v in RB_VECS)


# rows: one row; fewer rows than the R = 4 / WPR slots of a block; a partial last row group; and (with the default 512
# partials, 6 rows per block) a last non-empty block of ONE row followed by blocks with none
@pytest.mark.parametrize("rows", [1, 3, 37, 3001])
@pytest.mark.parametrize("cols", RB_WIDTHS)
def test_rmsnorm_bwd_every_width_vs_float64(ops, dev, cols, rows):
    g = torch.Generator().manual_seed(cols + rows)
    x = (torch.randn(rows, cols, generator=g) * torch.exp(torch.randn(rows, 1, generator=g))).to(torch.bfloat16)
    gamma = (torch.rand(cols, generator=g) + 0.5).to(torch.bfloat16)
    dy = (torch.randn(rows, cols, generator=g) / 8).to(torch.bfloat16)
    dres = (torch.randn(rows, cols, generator=g) / 8).to(torch.bfloat16)
    eps = 1e-5
    xd, gd, dyd, dresd = x.to(dev), gamma.to(dev), dy.to(dev), dres.to(dev)
    rstd = ops.rmsnorm_stats(xd, eps)
    refs = {False: O.rmsnorm_bwd_f32(bf16_bits(dy), bf16_bits(x), bf16_bits(gamma), eps),
            True: O.rmsnorm_bwd_f32(bf16_bits(dy), bf16_bits(x), bf16_bits(gamma), eps, dres_bits=bf16_bits(dres))}
    for with_res in (False, True):
        dx_ref, dg_ref = refs[with_res]
        for n_partials in (1, 7, 512):
            kw = dict(dres=dresd if with_res else None, n_partials=n_partials)
            dx, dgam = ops.rmsnorm_bwd(dyd, xd, rstd, gd, **kw)
            what = f"cols {cols} rows {rows} dres {with_res} n_partials {n_partials}"
            d = np.abs(dx.float().cpu().numpy().astype(np.float64) - dx_ref)
            tol = 2.0 ** -7 * np.abs(dx_ref) + 1e-5 * np.abs(dx_ref).max()
            assert (d <= tol).all(), f"{what}: dx max diff {d.max():.3g} at {np.unravel_index((d - tol).argmax(), d.shape)}"
            np.testing.assert_allclose(dgam.cpu().numpy(), dg_ref, rtol=1e-4, atol=1e-4 * np.abs(dg_ref).max(), err_msg=what)
            dx2, dgam2 = ops.rmsnorm_bwd(dyd, xd, rstd, gd, **kw)
            assert torch.equal(dx, dx2) and torch.equal(dgam, dgam2), f"{what}: not bitwise reproducible"


@pytest.mark.parametrize("cols", [512 * v for v in (9, 11, 13, 15, 17)] + [520, 1000, 3000, 8200])
def test_rmsnorm_bwd_refuses_widths_without_an_instance(ops, dev, cols):
    rows = 4
    x = torch.ones(rows, cols, dtype=torch.bfloat16, device=dev)
    rstd = torch.ones(rows, dtype=torch.float32, device=dev)
    gamma = torch.ones(cols, dtype=torch.bfloat16, device=dev)
    with pytest.raises(RuntimeError, match="mi_rmsnorm_bwd"):
        ops.rmsnorm_bwd(x, x, rstd, gamma)
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------------------- B: cross-entropy
# Bounds.  The kernels use __expf / __logf (v_exp_f32 / v_log_f32 on a scaled argument: a few fp32 ulps each) and fp32
# online sums of up to V terms per row in a fixed tree (~70 sequential adds per lane at V = 128256), so the sum of
# exponentials carries <~ 1e-6 relative error, i.e. lse <~ 1e-6 absolute from the log, plus the fp32 rounding of lse itself
# (2^-24 |lse|).  LSE_REL / LSE_ABS leave 2-10x headroom over that.  d(logits) = exp(x - lse) * gscale rounded to bf16:
# one bf16 ulp for the rounding, plus exp's relative error, which is the absolute error of the fp32 lse it is given
# (4 x 2^-24 |lse| + 2e-5) -- at |lse| ~ 3e4 that is ~1e-2 relative: the bf16 logits there are 128 apart anyway.
LSE_REL, LSE_ABS = 2e-6, 1e-5


def _ce_run(logits, labels, gscale):
    """(lse, loss, d, gscale tensor) of mi_ce_forward + mi_ce_backward on device tensors (logits bf16 [T, V], labels int64 [T])."""
    L = _lib()
    lib = L.load()
    T, V = logits.shape
    st = torch.cuda.current_stream().cuda_stream
    lse = torch.empty(T, dtype=torch.float32, device=logits.device)
    rows = torch.empty(T, dtype=torch.float32, device=logits.device)
    L.check(lib.mi_ce_forward(logits.data_ptr(), labels.data_ptr(), lse.data_ptr(), rows.data_ptr(), T, V, st), "mi_ce_forward")
    gs = torch.tensor([gscale], dtype=torch.float32, device=logits.device)
    d = torch.empty_like(logits)
    L.check(lib.mi_ce_backward(logits.data_ptr(), labels.data_ptr(), lse.data_ptr(), gs.data_ptr(), d.data_ptr(), T, V, st),
            "mi_ce_backward")
    return lse, rows, d, gs


def _ce_cast_matches_two_kernel_sequence(ops, logits, labels, lse, d, gs, fmt):
    """mi_ce_backward_cast == mi_ce_backward followed by mi_cast_amax: FP8 bytes both ways and the amax, bit for bit."""
    L = _lib()
    T, V = logits.shape
    dev = logits.device
    scale = torch.tensor([4096.0], device=dev)
    a_ref = torch.zeros(1, device=dev)
    y_ref, t_ref = ops.cast_amax(d, scale, a_ref, fmt)
    y = torch.zeros((T, V), dtype=torch.uint8, device=dev)
    yt = torch.zeros((V, T), dtype=torch.uint8, device=dev)
    a = torch.zeros(1, device=dev)
    L.check(L.load().mi_ce_backward_cast(logits.data_ptr(), labels.data_ptr(), lse.data_ptr(), gs.data_ptr(), y.data_ptr(),
                                         yt.data_ptr(), scale.data_ptr(), a.data_ptr(), T, V, fmt,
                                         torch.cuda.current_stream().cuda_stream), "mi_ce_backward_cast")
    torch.cuda.synchronize()
    assert torch.equal(y, y_ref), "fused CE backward cast: y bytes differ from mi_ce_backward + mi_cast_amax"
    assert torch.equal(yt, t_ref), "fused CE backward cast: yT bytes differ from mi_ce_backward + mi_cast_amax"
    assert torch.equal(a, a_ref) and a.item() > 0
    del y, yt, y_ref, t_ref


def _check_ce_vs_f64(x_bits, labels_np, lse, loss, d, gscale, what):
    lse_r, loss_r, d_r = O.cross_entropy_f64(x_bits, labels_np, gscale)
    lse_g = lse.cpu().numpy().astype(np.float64)
    assert np.isfinite(lse_g).all(), f"{what}: non-finite lse in rows {np.nonzero(~np.isfinite(lse_g))[0][:8]}"
    e = np.abs(lse_g - lse_r)
    tol = LSE_REL * np.abs(lse_r) + LSE_ABS
    assert (e <= tol).all(), f"{what}: lse max err {e.max():.3g} (row {e.argmax()}, lse {lse_r[e.argmax()]:.6g})"
    xl = np.abs(O.bf16_bits_to_f32(x_bits[np.arange(len(labels_np)), np.clip(labels_np, 0, x_bits.shape[1] - 1)]))
    e = np.abs(loss.cpu().numpy().astype(np.float64) - loss_r)
    tol = LSE_REL * np.abs(lse_r) + LSE_ABS + 2.0 ** -24 * xl
    assert (e <= tol).all(), f"{what}: loss max err {e.max():.3g} (row {e.argmax()})"
    dg = d.float().cpu().numpy().astype(np.float64)
    p = np.exp(O.bf16_bits_to_f32(x_bits).astype(np.float64) - lse_r[:, None])
    dl = 4 * 2.0 ** -24 * np.abs(lse_r) + 2e-5
    tol = _bf16_ulp(d_r) + abs(gscale) * p * dl[:, None] + 1e-30
    e = np.abs(dg - d_r)
    assert (e <= tol).all(), f"{what}: d(logits) max err {e.max():.3g} at {np.unravel_index((e - tol).argmax(), e.shape)}"


def test_ce_full_vocab_vs_float64(ops, dev):
    """V = 128256 (Llama-3): ~63 strided 8-element chunks per lane.  lse, per-row loss and d(logits) (gscale != 1) against
    float64 on 320 rows (a multiple of 8, not of 128: also checks the fused cast there), ignored rows included."""
    T, V = 320, 128256
    g = torch.Generator().manual_seed(128256)
    x = (torch.randn(T, V, generator=g) * 3).to(torch.bfloat16)
    labels = torch.randint(0, V, (T,), generator=g)
    labels[::13] = -100
    labels[5] = 0
    labels[6] = V - 1
    gscale = 0.37 / 300
    xd, ld = x.to(dev), labels.to(dev)
    lse, loss, d, gs = _ce_run(xd, ld, gscale)
    _check_ce_vs_f64(bf16_bits(x), labels.numpy(), lse, loss, d, gscale, f"T {T} V {V}")
    _ce_cast_matches_two_kernel_sequence(ops, xd, ld, lse, d, gs, O.E5M2)


@pytest.mark.parametrize("T", [8192, 1000])
def test_ce_step_shape_vs_device_fp32(ops, dev, T):
    """The step's lm_head shape (T = 8192 tokens, V = 128256; V = 1002 x 128 column tiles) and a T that is a multiple of 8 but
    not of 128: lse / loss / d(logits) against torch's fp32 log-softmax on the device (a float64 reference on the host would not
    fit the time), and the fused backward cast bit for bit against mi_ce_backward + mi_cast_amax."""
    V = 128256
    torch.manual_seed(T)
    xd = (torch.randn(T, V, device=dev) * 3).to(torch.bfloat16)
    ld = torch.randint(0, V, (T,), device=dev)
    ld[::17] = -100
    gscale = 1.0 / T
    lse, loss, d, gs = _ce_run(xd, ld, gscale)
    valid = ld >= 0
    for r0 in range(0, T, 1024):
        sl = slice(r0, min(T, r0 + 1024))
        xf = xd[sl].float()
        lse_r = torch.logsumexp(xf, dim=1)
        assert torch.isfinite(lse[sl]).all()
        # the fp32 torch reference carries an error of the same kind as the kernel: twice the float64 bound
        assert ((lse[sl] - lse_r).abs() <= 2 * (LSE_REL * lse_r.abs() + LSE_ABS)).all(), f"rows {sl}: lse"
        lab = ld[sl].clamp(min=0)
        loss_r = torch.where(valid[sl], lse_r - xf.gather(1, lab[:, None])[:, 0], torch.zeros_like(lse_r))
        assert ((loss[sl] - loss_r).abs() <= 2 * (LSE_REL * lse_r.abs() + LSE_ABS)).all(), f"rows {sl}: loss"
        p = torch.exp(xf - lse_r[:, None])
        d_r = p.clone()
        d_r[torch.arange(d_r.shape[0], device=dev)[valid[sl]], lab[valid[sl]]] -= 1.0
        d_r *= torch.where(valid[sl], gscale, 0.0)[:, None]
        ulp = torch.exp2(torch.floor(torch.log2(d_r.abs().clamp(min=2.0 ** -126))) - 7)
        tol = ulp + gscale * p * (4 * 2.0 ** -24 * lse_r.abs() + 4e-5)[:, None] + 1e-30
        err = (d[sl].float() - d_r).abs()
        assert (err <= tol).all(), f"rows {sl}: d(logits) max err {err.max().item():.3g}"
        del xf, p, d_r, ulp, tol, err
    _ce_cast_matches_two_kernel_sequence(ops, xd, ld, lse, d, gs, O.E4M3)


def _ce_edge_rows(V: int, seed: int):
    """bf16 logits and labels of the edge rows at vocabulary V (a multiple of 8), padded with random rows to a multiple of 8."""
    g = np.random.default_rng(seed)
    rows, labs = [], []

    def rnd(scale=3.0):
        return (g.standard_normal(V) * scale).astype(np.float32)

    rows.append(rnd()); labs.append(0)
    rows.append(rnd()); labs.append(V - 1)
    rows.append(rnd()); labs.append(-100)
    rows.append(rnd()); labs.append(V)           # label >= V: ignored, like -100
    rows.append(rnd()); labs.append(V + 12345)
    rows.append(np.full(V, 1.5, np.float32)); labs.append(V // 3)                    # all logits equal
    r = rnd(); j = int(g.integers(V)); r[j] = r.max() + 80.0; rows.append(r); labs.append(j)          # spike, label on it
    r = rnd(); j = int(g.integers(V)); r[j] = r.max() + 80.0; rows.append(r); labs.append((j + 1) % V)  # spike, label off it
    rows.append(30000.0 + rnd(300.0)); labs.append(int(g.integers(V)))           # near +3e4 (bf16 spacing 128 there)
    rows.append(-30000.0 + rnd(300.0)); labs.append(int(g.integers(V)))          # near -3e4
    if V >= 16:
        # -inf over whole 8-element lanes: at the start of the row (up to all of waves 0 and 1: 1024 columns) and in the
        # middle; the label is on a finite entry
        n0 = min(1024, (V // 2) // 8 * 8)
        r = rnd(); r[:n0] = -np.inf; rows.append(r); labs.append(V - 1)
        c0 = (V // 3) // 8 * 8
        n1 = max(8, min(512, (V // 4) // 8 * 8))
        r = rnd(); r[c0:c0 + n1] = -np.inf; rows.append(r); labs.append(0 if c0 > 0 else V - 1)
        r = rnd(); r[:8] = -np.inf; r[c0:c0 + 8] = -np.inf; rows.append(r); labs.append(V - 1)  # single lanes
    while len(rows) % 8:
        rows.append(rnd()); labs.append(int(g.integers(V)))
    return O.f32_to_bf16_bits(np.stack(rows)), np.array(labs, dtype=np.int64)


@pytest.mark.parametrize("V", [8, 520, 1536, 2048, 4096, 128256])
def test_ce_edge_rows_vs_float64(ops, dev, V):
    """Edge rows against float64, directly on the kernels and through causal_lm_loss.  A label >= V is treated as ignored
    (loss 0, zero gradient), exactly like -100, and like -100 it does not count in causal_lm_loss's token count (the mean's
    denominator counts what the kernels count); this test pins both.  V < 2048: whole waves (V = 8, 520: lanes too) see no columns.  Rows of -inf
    logits over whole lanes (masked vocabulary) must give HF's finite loss: before ce_fwd_kernel guarded its per-lane and
    cross-wave online updates, exp(-inf - -inf) made lse NaN."""
    from llm_fp8_amd.loss import causal_lm_loss
    x_bits, labels = _ce_edge_rows(V, V)
    T = x_bits.shape[0]
    xd = bits_to_bf16(x_bits, dev)
    ld = torch.from_numpy(labels).to(dev)
    gscale = 0.5
    lse, loss, d, gs = _ce_run(xd, ld, gscale)
    _check_ce_vs_f64(x_bits, labels, lse, loss, d, gscale, f"V {V}")
    _ce_cast_matches_two_kernel_sequence(ops, xd, ld, lse, d, gs, O.E5M2)
    # the same rows through the autograd surface: mean over the labels inside [0, V), gradient = d(mean) * 2
    la = xd[None].clone().requires_grad_(True)
    out = causal_lm_loss(la, ld[None], V, shift_labels=ld[None])
    (out * 2.0).backward()
    n = int(((labels >= 0) & (labels < V)).sum())
    assert n < int((labels != -100).sum())   # the rows hold a label >= V: the two counts differ
    lse_r, loss_r, _ = O.cross_entropy_f64(x_bits, labels)
    xl = np.abs(O.bf16_bits_to_f32(x_bits[np.arange(T), np.clip(labels, 0, V - 1)]).astype(np.float64))
    tol = ((LSE_REL * np.abs(lse_r) + LSE_ABS + 2.0 ** -24 * xl).sum() + T * 2.0 ** -24 * np.abs(loss_r).sum()) / n
    assert abs(out.item() - loss_r.sum() / n) <= tol, f"V {V}: causal_lm_loss {out.item()} vs float64 {loss_r.sum() / n}"
    _check_ce_vs_f64(x_bits, labels, lse, loss, la.grad[0], 2.0 / n, f"V {V} via causal_lm_loss")


def test_causal_lm_loss_fallback_for_vocab_not_multiple_of_8(dev):
    """V % 8 != 0: causal_lm_loss hands the call to HF's ForCausalLMLoss; value and gradient are HF's."""
    from transformers.loss.loss_utils import ForCausalLMLoss
    from llm_fp8_amd.loss import causal_lm_loss
    torch.manual_seed(1001)
    B, S, V = 2, 24, 1001
    logits = (torch.randn(B, S, V, device=dev) * 3).to(torch.bfloat16)
    labels = torch.randint(0, V, (B, S), device=dev)
    labels[1, 3:7] = -100
    la, lb = logits.clone().requires_grad_(True), logits.clone().requires_grad_(True)
    a = causal_lm_loss(la, labels, V)
    b = ForCausalLMLoss(lb, labels, V)
    assert torch.equal(a, b)
    a.backward()
    b.backward()
    assert torch.equal(la.grad, lb.grad)


# ----------------------------------------------------------------------------------------- C: ClippedAdamW
CHUNK = 65536
FLAT_SIZES = [(CHUNK,), (CHUNK + 8,), (2 * CHUNK + 13,), (7,), (1,), (200, 333), (129, 131)]  # 2-D: not multiples of TILE = 128


def _state_bits(opt, p):
    st = opt.state[p]
    return bf16_bits(p), bf16_bits(st["exp_avg"]), bf16_bits(st["exp_avg_sq"])


def _adam_ref(before, step, hp, coef):
    """float64 AdamW step from the device state before it: [(value, fp32 slack)] for p, exp_avg, exp_avg_sq.  The
    hyper-parameters are those the kernels receive: fp32 (1 - fp32(0.999) is 1.3e-5 relative away from 1 - 0.999, more
    than the whole fp32 error of the step).  The slack is the kernel's fp32 evaluation error (8 x 2^-24 x the magnitudes of
    the terms it adds): it only matters where the terms cancel and one bf16 ulp of the small result is less than that."""
    pb, mb, vb, gb = before
    if mb is None:
        mb = vb = np.zeros_like(pb)
    h = {k: float(np.float32(hp[k])) for k in ("lr", "eps", "weight_decay")}
    b1, b2 = (float(np.float32(b)) for b in hp["betas"])
    p, m, v = O.adamw_step_f64(pb, gb, mb, vb, step, h["lr"], b1, b2, h["eps"], h["weight_decay"], grad_scale=coef)
    f = lambda b: np.abs(O.bf16_bits_to_f32(b).astype(np.float64))
    pf, gf, mf = f(pb), f(gb) * coef, f(mb)
    upd = h["lr"] / (1.0 - b1 ** step) * np.abs(m) / (np.sqrt(v) / np.sqrt(1.0 - b2 ** step) + h["eps"])
    u = 8 * 2.0 ** -24
    return [(p, u * (pf + upd)), (m, u * (mf + gf)), (v, u * np.abs(v))]


def _check_adam_tensor(got_bits, ref, what):
    """Each of p / exp_avg / exp_avg_sq within one bf16 ulp (+ the fp32 slack) of the float64 step, and -- the kernel's fp32
    arithmetic is ~1e-7 relative -- equal to the bf16 rounding of the float64 value except near rounding ties (AdamW's
    constants put a few 1e-3 of the moments within 1e-7 of one): a term of a quarter ulp (a dropped weight decay of
    lr * wd = 1e-3) moves ~20 % of the elements.  Returns (mismatches, size)."""
    ref64, slack = ref
    got = O.bf16_bits_to_f32(got_bits).astype(np.float64)
    e = np.abs(got - ref64)
    tol = _bf16_ulp(ref64) + slack
    assert (e <= tol).all(), f"{what}: {(e > tol).sum()} elements beyond 1 bf16 ulp, max err {e.max():.3g}"
    return int((got_bits != O.f32_to_bf16_bits(ref64.astype(np.float32))).sum()), got_bits.size


def _adam_case(case):
    """(param groups as (sizes, hyper-parameters, grad scale), max_grad_norm, param scale)."""
    g0 = dict(lr=1e-2, weight_decay=0.1, betas=(0.9, 0.999), eps=1e-8)
    g1 = dict(lr=1e-5, weight_decay=0.0, betas=(0.8, 0.95), eps=1e-6)
    g2 = dict(lr=3e-2, weight_decay=0.5, betas=(0.9, 0.99), eps=1e-8)  # decay of 1.5 %: several bf16 ulps per step
    if case == "clip":      # norm ~ 600 > 1: clipped
        return [(FLAT_SIZES[:4], g0, 1.0), (FLAT_SIZES[4:], g1, 1.0), ([(300, 40)], g2, 1.0)], 1.0, 1.0
    if case == "noclip":    # norm ~ 0.6 < 1: coefficient 1
        return [(FLAT_SIZES, g0, 1e-3), ([(8, 24)], g1, 1e-3)], 1.0, 1.0
    if case == "none":      # max_grad_norm None: no norm pass
        return [(FLAT_SIZES[:3], g2, 1.0), (FLAT_SIZES[3:], g0, 1.0)], None, 1.0
    if case == "tiny":      # gradients ~1e-12, parameters ~1e-6: eps dominates the denominator and the update is ~ p
        return [(FLAT_SIZES, g0, 1e-12), ([(64, 40)], g1, 1e-12)], 1.0, 1e-6
    raise ValueError(case)


@pytest.mark.parametrize("case", ["clip", "noclip", "none", "tiny"])
def test_clipped_adamw_vs_float64_one_step(dev, case):
    """Every step (1, 2 and, after setting state["step"], 1000) against a float64 AdamW step started from the device's own
    state before the step (errors do not compound); the gradient norm / clip coefficient against the float64 norm.  Tensors
    straddle CHUNK (full, full + an 8-element tail, 2 chunks + a 13-element tail, 7, 1 elements); the 2nd tensor of every first
    group gets a zero gradient; two or three groups with different hyper-parameters."""
    from llm_fp8_amd.optim import ClippedAdamW
    assert ClippedAdamW.CHUNK == CHUNK
    groups, mgn, pscale = _adam_case(case)
    gen = torch.Generator().manual_seed({"clip": 1, "noclip": 2, "none": 3, "tiny": 4}[case])
    params, gscales = [], []
    for sizes, hp, gsc in groups:
        ps = [torch.nn.Parameter((torch.randn(s, generator=gen) * pscale).to(torch.bfloat16).to(dev)) for s in sizes]
        params.append(ps)
        gscales.append(gsc)
    opt = ClippedAdamW([dict(params=ps, lr=hp["lr"], weight_decay=hp["weight_decay"], betas=hp["betas"], eps=hp["eps"])
                        for ps, (_, hp, _) in zip(params, groups)], max_grad_norm=mgn)
    mism, tot = {}, {}
    for step in (1, 2, 1000):
        if step == 1000:
            for ps in params:
                for p in ps:
                    opt.state[p]["step"] = 999
        for gi, ps in enumerate(params):
            for k, p in enumerate(ps):
                gr = torch.randn(p.shape, generator=gen) * gscales[gi]
                if gi == 0 and k == 1:
                    gr.zero_()
                p.grad = gr.to(torch.bfloat16).to(dev)
        before = [[(_state_bits(opt, p) if opt.state[p] else (bf16_bits(p), None, None)) + (bf16_bits(p.grad),) for p in ps]
                  for ps in params]
        opt.step()
        torch.cuda.synchronize()
        sq = sum(float((O.bf16_bits_to_f32(b[3]).astype(np.float64) ** 2).sum()) for bs in before for b in bs)
        norm = math.sqrt(sq)
        coef = 1.0
        if mgn is not None:
            got_norm = opt.last_grad_norm.item()
            assert abs(got_norm - norm) <= 1e-6 * norm, f"step {step}: grad norm {got_norm} vs float64 {norm}"
            coef = min(1.0, mgn / (norm + 1e-6))
            got_coef = min(np.float32(1.0), np.float32(mgn) / (np.float32(got_norm) + np.float32(1e-6)))
            assert abs(float(got_coef) - coef) <= 1e-6 * coef, f"step {step}: clip coefficient {got_coef} vs {coef}"
            assert (coef < 1.0) == (case == "clip")
        for gi, (ps, (_, hp, _)) in enumerate(zip(params, groups)):
            for k, p in enumerate(ps):
                ref = _adam_ref(before[gi][k], step, hp, coef)
                assert opt.state[p]["step"] == step
                for got, r, name in zip(_state_bits(opt, p), ref, ("p", "exp_avg", "exp_avg_sq")):
                    n_bad, n = _check_adam_tensor(got, r, f"{case} step {step} group {gi} tensor {tuple(p.shape)} {name}")
                    mism[name] = mism.get(name, 0) + n_bad
                    tot[name] = tot.get(name, 0) + n
    for name in mism:
        assert mism[name] <= 1e-2 * tot[name], f"{case}: {mism[name]} / {tot[name]} of {name} are not the bf16 rounding of the float64 step"


def _sink_linear(dev, seed):
    """An FP8 Linear (200 x 144 weight: 128 x 128 tiles ragged both ways) after one training forward / backward under delayed
    scaling: its weight has an optimiser sink (module.WeightSink)."""
    import llm_fp8_amd.pytorch as te
    from llm_fp8_amd.common.recipe import DelayedScaling, Format
    torch.manual_seed(seed)
    lin = te.Linear(144, 200, bias=False, params_dtype=torch.bfloat16, device=dev)
    x = torch.randn(64, 144, device=dev, dtype=torch.bfloat16)
    recipe = DelayedScaling(fp8_format=Format.HYBRID, amax_history_len=4, amax_compute_algo="max")
    with te.fp8_autocast(enabled=True, fp8_recipe=recipe):
        y = lin(x)
    y.float().pow(2).mean().backward()
    return lin


def test_clipped_adamw_sink_path_vs_float64(te_reset, dev):
    """The weight-cast hand-off route (mi_adamw_cast_bf16_multi: a sink weight in 128 x 128 tiles + a flat tensor with an
    8-element tail in the same launch) meets the float64 bound of the flat route."""
    from llm_fp8_amd.optim import ClippedAdamW
    w = _sink_linear(dev, 144).weight
    flat = torch.nn.Parameter(torch.randn(CHUNK + 8, device=dev).to(torch.bfloat16))
    hp = dict(lr=1e-2, weight_decay=0.1, betas=(0.9, 0.999), eps=1e-8)
    opt = ClippedAdamW([w, flat], max_grad_norm=1.0, **hp)
    assert opt._sink_of(w) is not None, "the weight did not get an FP8 sink: the test would not take the cast path"
    for step in (1, 2):
        w.grad = torch.randn(w.shape, device=dev).to(torch.bfloat16)
        flat.grad = torch.randn(flat.shape, device=dev).to(torch.bfloat16)
        before = [(_state_bits(opt, p) if opt.state[p] else (bf16_bits(p), None, None)) + (bf16_bits(p.grad),) for p in (w, flat)]
        opt.step()
        torch.cuda.synchronize()
        assert opt._plans and all(pl["chunks_cast"] is not None for pl in opt._plans.values())
        norm = math.sqrt(sum(float((O.bf16_bits_to_f32(b[3]).astype(np.float64) ** 2).sum()) for b in before))
        coef = min(1.0, 1.0 / (norm + 1e-6))
        for p, bef in zip((w, flat), before):
            for got, r, name in zip(_state_bits(opt, p), _adam_ref(bef, step, hp, coef), ("p", "exp_avg", "exp_avg_sq")):
                n_bad, n = _check_adam_tensor(got, r, f"sink step {step} {tuple(p.shape)} {name}")
                assert n_bad <= 1e-2 * n, f"sink step {step} {tuple(p.shape)}: {n_bad} / {n} of {name} off the bf16 rounding"


def test_clipped_adamw_sink_weight_with_misaligned_moments(te_reset, dev):
    """Adam moments that are views at a 2-byte offset (a loaded optimiser state can be): the tile path of the *_cast kernels
    issues 16-byte loads on them unconditionally, so such a weight must take the flat path -- and give exactly the result of
    the run with aligned moments."""
    from llm_fp8_amd.optim import ClippedAdamW
    hp = dict(lr=1e-2, weight_decay=0.1, betas=(0.9, 0.999), eps=1e-8)

    def run(offset):
        w = _sink_linear(dev, 200).weight
        opt = ClippedAdamW([w], max_grad_norm=1.0, **hp)
        n = w.numel()
        m_buf = torch.zeros(n + 8, dtype=torch.bfloat16, device=dev)
        v_buf = torch.zeros(n + 8, dtype=torch.bfloat16, device=dev)
        opt.state[w]["step"] = 0
        opt.state[w]["exp_avg"] = m_buf[offset:offset + n].view(w.shape)
        opt.state[w]["exp_avg_sq"] = v_buf[offset:offset + n].view(w.shape)
        assert (opt.state[w]["exp_avg"].data_ptr() % 16 == 0) == (offset == 0)
        assert (opt._sink_of(w) is not None) == (offset == 0), "misaligned moments must keep the weight off the tile path"
        g = torch.Generator(device=dev).manual_seed(5)
        for _ in range(2):
            w.grad = torch.randn(w.shape, device=dev, generator=g).to(torch.bfloat16)
            opt.step()
        torch.cuda.synchronize()
        return w.detach().clone(), opt.state[w]["exp_avg"].clone(), opt.state[w]["exp_avg_sq"].clone()

    a, b = run(0), run(1)
    for u, v_, name in zip(a, b, ("p", "exp_avg", "exp_avg_sq")):
        assert torch.equal(u.view(torch.int16), v_.view(torch.int16)), f"misaligned moments: {name} differs from the aligned run"


@pytest.fixture()
def te_reset(dev):
    from llm_fp8_amd.pytorch.fp8 import FP8GlobalStateManager
    FP8GlobalStateManager.reset()
    yield
    FP8GlobalStateManager.reset()


# ----------------------------------------------------------------------------------------- D: RoPE at the step's shapes
def _rope_call(qkv, cos, sin, nq, nkv, D, S, backward, outs):
    L = _lib()
    T = qkv.shape[0]
    a, b, c = outs
    L.check(L.load().mi_rope_qkv(qkv.data_ptr(), a.data_ptr(), b.data_ptr(), c.data_ptr(), cos.data_ptr(), sin.data_ptr(), T, S,
                                 nq, nkv, D, int(backward), torch.cuda.current_stream().cuda_stream), "mi_rope_qkv")


@pytest.mark.parametrize("B,S,nq,nkv,D", [(16, 512, 24, 8, 128), (16, 512, 32, 8, 64)])  # Llama-3.2-3B / 1B attention
def test_rope_qkv_at_step_shape_vs_oracle(ops, dev, B, S, nq, nkv, D):
    """The 3B shape has 8192 rows x 384 items > 8192 blocks x 256 threads: the grid-stride loop goes round twice.  Outputs are
    NaN-filled first, so an item the kernel never visits fails the comparison."""
    import llm_fp8_amd.pytorch as te
    from llm_fp8_amd.pytorch.attention import _cos_sin_tables
    T, W = B * S, (nq + 2 * nkv) * D
    g = torch.Generator().manual_seed(W)
    qkv = torch.randn(T, W, generator=g).to(torch.bfloat16)
    freqs = te.attention.RotaryPositionEmbedding(D)(max_seq_len=S).to(dev)
    cos, sin = _cos_sin_tables(freqs, S)
    nan = lambda n: torch.full((T, n), float("nan"), dtype=torch.bfloat16, device=dev)
    q, k, v = nan(nq * D), nan(nkv * D), nan(nkv * D)
    _rope_call(qkv.to(dev), cos, sin, nq, nkv, D, S, False, (q, k, v))
    ref_q, ref_k, ref_v = ops.rope_qkv_forward(qkv.to(dev), cos, sin, nq, nkv, D, S)
    assert torch.equal(q, ref_q) and torch.equal(k, ref_k) and torch.equal(v, ref_v)  # the ops wrapper: same launch
    pos = np.tile(np.arange(S), B)
    bits = bf16_bits(qkv)
    xmax = np.abs(O.bf16_bits_to_f32(bits)).max()

    def close(got, ref_bits, what):
        gf, rf = got.float().cpu().numpy(), O.bf16_bits_to_f32(ref_bits)
        assert np.isfinite(gf).all(), f"{what}: {(~np.isfinite(gf)).sum()} elements not written"
        # device cos/sin come from torch.cos on the GPU: 1 bf16 ulp on a few elements
        assert np.all(np.abs(gf - rf) <= 2.0 ** -7 * np.abs(rf) + 1e-5 * xmax), what
        assert (bf16_bits(got) == ref_bits).mean() > 0.98, what

    close(q, O.rope_f32(bits[:, :nq * D], pos, D), "q")
    close(k, O.rope_f32(bits[:, nq * D:(nq + nkv) * D], pos, D), "k")
    np.testing.assert_array_equal(bf16_bits(v), bits[:, (nq + nkv) * D:])
    back = torch.full((T, W), float("nan"), dtype=torch.bfloat16, device=dev)
    _rope_call(back, cos, sin, nq, nkv, D, S, True, (q, k, v))
    assert torch.equal(back, ops.rope_qkv_backward(q, k, v, cos, sin, nq, nkv, D, S))
    close(back[:, :nq * D], O.rope_f32(bf16_bits(q), pos, D, conj=True), "dq")
    close(back[:, nq * D:(nq + nkv) * D], O.rope_f32(bf16_bits(k), pos, D, conj=True), "dk")
    np.testing.assert_array_equal(bf16_bits(back[:, (nq + nkv) * D:]), bf16_bits(v))
