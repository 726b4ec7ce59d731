"""GPU: optim.ClippedAdamW(stochastic_rounding=True) -- bf16 weights and moments rounded stochastically in the fused AdamW + FP8
cast pass (mi_adamw_sr_bf16_multi).  1: the stored bits are the numpy twin's (tests/sr_twin.py) on every walk; 2: the rounding
probabilities and the independence of the streams; 3: every stored value is a bf16 neighbour of the float64 update; 4: the summed
displacement at the default learning rate; 5: exp_avg_sq decays; 6: sinks; 7: shards; 8: resume; 9: the harness; 10: the default
modes do not reach the new entry point.

Figures measured on the device (profiles/optim_stochastic_rounding.txt): test 4 summed-displacement error 0.18 % with stochastic
rounding (bound 5 %), 86.1 % in default mode; test 5 mean(exp_avg_sq) / start 0.77401 against 0.999^256 = 0.77404 (bound 1.5e-3).
Both are the numpy model's figures to the last digit printed: over the 64 steps the kernel and the twin round alike."""
import copy
import math

import numpy as np
import pytest
import torch

from tests import sr_twin as S
from tests.test_optim_fp32_state_gpu import CHUNK, G0, _clip_coef, _delayed, _f64_step, _np, _sink_linear
from tests.test_optim_sr import displacement_figures, displacement_inputs, displacement_reference

pytestmark = pytest.mark.gpu
BF16, F32 = torch.bfloat16, torch.float32


@pytest.fixture()
def te_reset(dev):
    from llm_fp8_amd.pytorch.fp8 import FP8GlobalStateManager
    FP8GlobalStateManager.reset()
    yield
    FP8GlobalStateManager.reset()


def _bits(t):
    return t.detach().contiguous().view(torch.int16).cpu().numpy().view(np.uint16).ravel()


def _sr_opt(params, seed=0, mgn=None, **hp):
    from llm_fp8_amd.optim import ClippedAdamW
    return ClippedAdamW(params, max_grad_norm=mgn, stochastic_rounding=True, sr_seed=seed, **hp)


def _mx():
    from llm_fp8_amd.common.recipe import MXFP8BlockScaling
    return MXFP8BlockScaling()


# ------------------------------------------------------------------------------------------------ 1: known answer
def test_known_answer_on_every_walk(te_reset, dev):
    """g = 0, zero moments, lr = 2^-6, weight_decay = 2^-3: the update is the one fp32 product p (1 - 2^-9), so the stored weight
    must be the twin's (bits + r) >> 16 exactly; a second step from a KNOWN exp_avg / exp_avg_sq (g = 0: exp_avg + (1 - b1)(0 -
    exp_avg) and b2 exp_avg_sq, two fp32 operations each) pins the moment streams the same way.  One data vector, one key, base 0,
    walked four ways: flat (vector body + 5-element tail), the same at a 2-byte offset (element-wise), a 200 x 144 weight with a
    per-tensor sink (partial 128 x 128 tiles) and a 160 x 96 weight with an MXFP8 sink; and elements [3, 3 + 2053) of it as a
    tensor of their own with base 3 (no multiple of 8: element-wise, each element still draws the bits of its global index)."""
    key, seed = 5, 0x123456789ABCDEF0
    hp = dict(lr=2.0 ** -6, weight_decay=2.0 ** -3, betas=(0.9, 0.999), eps=1e-8)
    n_all, n_flat = 200 * 144, 8 * 256 * 3 + 5
    gen = torch.Generator().manual_seed(21)
    p0 = torch.randn(n_all, generator=gen).to(BF16)
    m0 = (1e-2 * torch.randn(n_all, generator=gen)).to(BF16)
    v0 = (1e-4 * torch.rand(n_all, generator=gen)).to(BF16)

    flat = torch.nn.Parameter(p0[:n_flat].clone().to(dev))
    buf = torch.zeros(n_flat + 8, dtype=BF16, device=dev)
    off = torch.nn.Parameter(buf[1:1 + n_flat])
    tiled = _sink_linear(dev, 144, 144, 200, _delayed()).weight
    mxw = _sink_linear(dev, 96, 96, 160, _mx()).weight
    tensors = [flat, off, tiled, mxw]
    with torch.no_grad():
        for t in tensors:
            t.copy_(p0[:t.numel()].view(t.shape))
            t._mi_sr_key = (key, 0)
    assert flat.data_ptr() % 16 == 0 and off.data_ptr() % 16 == 2
    part = torch.nn.Parameter(p0[3:3 + 2053].clone().to(dev))
    part._mi_sr_key = (key, 3)
    part.grad = torch.zeros_like(part)
    opt = _sr_opt(tensors + [part], seed=seed, **hp)
    assert opt._sink_of(tiled) is not None and opt._mx_sink_of(mxw) is not None
    e = np.arange(n_all, dtype=np.uint64)
    zeros = np.zeros(n_all, np.float32)

    for t in tensors:
        t.grad = torch.zeros_like(t)
    opt.step()
    torch.cuda.synchronize()
    pf = p0.float().numpy() * np.float32(1.0 - 2.0 ** -9)
    want_p = S.sr_bf16_bits(pf, S.sr_bits16(seed, 1, key, 0, e))
    assert (want_p != S.rne_bf16_bits(pf)).mean() > 0.2, "the inputs do not tell stochastic rounding from round-to-nearest"
    got = [_bits(t) for t in tensors]
    for t, b in zip(tensors, got):
        assert np.array_equal(b, want_p[:b.size]), f"weight {tuple(t.shape)}: {(b != want_p[:b.size]).sum()} of {b.size} differ from the twin"
        assert not _bits(opt.state[t]["exp_avg"]).any() and not _bits(opt.state[t]["exp_avg_sq"]).any()  # a bf16 value (0) never moves
    for b in got[1:]:
        k = min(b.size, got[0].size)
        assert np.array_equal(b[:k], got[0][:k]), "two walks disagree where their data coincide"
    assert buf[0].item() == 0.0 and buf[1 + n_flat:].abs().sum().item() == 0.0  # nothing written around the view
    assert np.array_equal(_bits(part), want_p[3:3 + 2053]), "a tensor that starts at global element 3 drew other bits"

    # second step from a known state: exp_avg and exp_avg_sq
    with torch.no_grad():
        for t in tensors:
            opt.state[t]["exp_avg"].copy_(m0[:t.numel()].view(t.shape))
            opt.state[t]["exp_avg_sq"].copy_(v0[:t.numel()].view(t.shape))
    opt.step()
    torch.cuda.synchronize()
    _, mf, vf = S.adam_f32(zeros, zeros, m0.float().numpy(), v0.float().numpy(), 2, hp["lr"], hp["betas"], hp["eps"], hp["weight_decay"])
    want_m = S.sr_bf16_bits(mf, S.sr_bits16(seed, 2, key, 1, e))
    want_v = S.sr_bf16_bits(vf, S.sr_bits16(seed, 2, key, 2, e))
    for t in tensors:
        gm, gv = _bits(opt.state[t]["exp_avg"]), _bits(opt.state[t]["exp_avg_sq"])
        assert opt.state[t]["step"] == 2
        assert np.array_equal(gm, want_m[:gm.size]), f"exp_avg {tuple(t.shape)}: {(gm != want_m[:gm.size]).sum()} differ from the twin"
        assert np.array_equal(gv, want_v[:gv.size]), f"exp_avg_sq {tuple(t.shape)}: {(gv != want_v[:gv.size]).sum()} differ from the twin"
    got2 = [_bits(t) for t in tensors]
    for b in got2[1:]:
        k = min(b.size, got2[0].size)
        assert np.array_equal(b[:k], got2[0][:k]), "two walks disagree on the weight of the second step"


# ------------------------------------------------------------------------------------------------ 2: probabilities
N2 = 1 << 20


def _ups(dev, wd, key=0, seed=0, step0=0, moment=False):
    """Up / down pattern of 2^20 values that sit at a known place between two bf16 neighbours.  Weight: 1.0 x (1 - lr wd) with
    lr = 2^-6 (zero gradient and moments); moment: exp_avg = 1.0 with b1 = 1 - 2^-9 and g = 0 gives exactly 1 - 2^-9."""
    p = torch.nn.Parameter(torch.ones(N2, dtype=BF16, device=dev))
    p._mi_sr_key = (key, 0)
    p.grad = torch.zeros_like(p)
    opt = _sr_opt([p], seed=seed, lr=2.0 ** -6, weight_decay=wd, betas=(1.0 - 2.0 ** -9, 0.999), eps=1e-8)
    opt.state[p] = {"step": step0, "exp_avg": torch.full_like(p, 1.0 if moment else 0.0), "exp_avg_sq": torch.zeros_like(p)}
    opt.step()
    torch.cuda.synchronize()
    b = _bits(opt.state[p]["exp_avg"] if moment else p)
    assert np.isin(b, (0x3F7F, 0x3F80)).all(), "a value left its two neighbours"
    return b == 0x3F80


def test_rounding_probabilities_and_independent_streams(dev):
    base = _ups(dev, 2.0 ** -3)                       # 1 - 2^-9: exactly halfway, P(up) = 1/2
    assert abs(int(base.sum()) - N2 // 2) <= 3072, base.sum()      # 6 sqrt(N / 4)
    three_q = _ups(dev, 2.0 ** -4)                    # 1 - 2^-10: P(up) = 3/4
    assert abs(int(three_q.sum()) - 3 * N2 // 4) <= 2660, three_q.sum()  # 6 sqrt(N 3/16)
    assert np.array_equal(base, _ups(dev, 2.0 ** -3)), "the same five inputs gave other bits"
    for what, other in (("step 1 / step 2", _ups(dev, 2.0 ** -3, step0=1)), ("tensor key 0 / 1", _ups(dev, 2.0 ** -3, key=1)),
                        ("seed 0 / 1", _ups(dev, 2.0 ** -3, seed=1)), ("weight / moment stream", _ups(dev, 2.0 ** -3, moment=True))):
        agree = int((base == other).sum())
        print(f"{what}: agree on {agree} of {N2}")
        assert abs(int(other.sum()) - N2 // 2) <= 3072, (what, other.sum())
        assert abs(agree - N2 // 2) <= 3072, (what, agree)


# ------------------------------------------------------------------------------------------------ 3: neighbours
def _bf16_grid(x, up):
    """float64 -> the bf16 value at or above (`up`) / at or below x, exact (8 significand bits, subnormal spacing 2^-133)."""
    _, ex = np.frexp(x)
    ulp = np.ldexp(1.0, np.maximum(ex - 1, -126) - 7)
    q = x / ulp
    return (np.ceil(q) if up else np.floor(q)) * ulp


@pytest.mark.parametrize("case", ["clip", "small"])
def test_every_stored_value_is_a_bf16_neighbour_of_the_float64_update(te_reset, dev, case):
    """Random p, g, exp_avg, exp_avg_sq, three steps, flat tensors around the 64 Ki chunk and a weight on the tile walk.  u = the
    float64 update from the device's own state before the step, delta = the fp32 evaluation bound of
    tests/test_optim_fp32_state_gpu.py test A (8 x 2^-24 x the magnitudes of the terms added): every stored weight, exp_avg and
    exp_avg_sq lies in [floor_bf16(u - delta), ceil_bf16(u + delta)].  clip: gradient norm ~ 700, clipped; small: ~ 0.07, not."""
    gscale = {"clip": 1.0, "small": 1e-4}[case]
    gen = torch.Generator().manual_seed({"clip": 31, "small": 32}[case])
    sizes = [(CHUNK + 8,), (2 * CHUNK + 13,), (7,), (200, 333)]
    params = [torch.nn.Parameter(torch.randn(s, generator=gen).to(BF16).to(dev)) for s in sizes]
    params.append(_sink_linear(dev, 144, 144, 200, _delayed()).weight)
    opt = _sr_opt(params, seed=17, mgn=1.0, **G0)
    for p in params:
        opt.state[p] = {"step": 0, "exp_avg": (1e-2 * gscale * torch.randn(p.shape, generator=gen)).to(BF16).to(dev),
                        "exp_avg_sq": (1e-4 * gscale * gscale * torch.rand(p.shape, generator=gen)).to(BF16).to(dev)}
    assert opt._sink_of(params[-1]) is not None
    for step in (1, 2, 3):
        for p in params:
            p.grad = (gscale * torch.randn(p.shape, generator=gen)).to(BF16).to(dev)
        before = [(_np(p), _np(p.grad), _np(opt.state[p]["exp_avg"]), _np(opt.state[p]["exp_avg_sq"])) for p in params]
        opt.step()
        torch.cuda.synchronize()
        coef = _clip_coef(opt, before, 1.0)
        assert (coef < 1.0) == (case == "clip")
        for p, b in zip(params, before):
            stored = (_np(p), _np(opt.state[p]["exp_avg"]), _np(opt.state[p]["exp_avg_sq"]))
            for name, got, (u, delta) in zip(("weight", "exp_avg", "exp_avg_sq"), stored, _f64_step(*b, step, G0, coef)):
                lo, hi = _bf16_grid(u - delta, False), _bf16_grid(u + delta, True)
                bad = (got < lo) | (got > hi)
                assert not bad.any(), f"{case} step {step} {tuple(p.shape)} {name}: {bad.sum()} of {bad.size} outside their neighbours"


# ------------------------------------------------------------------------------------------------ 4: displacement
def test_summed_displacement_at_the_default_learning_rate(dev):
    """The inputs of profiles/optim_fp32_state.txt section 3 (65 544 weights of magnitude 0.02, 64 steps, lr 1.41e-5): the update is
    far below half a bf16 ulp, so round-to-nearest drops most of it.  |sum(p_64 - p_0) - sum(d_ref)| <= 5 % of |sum(d_ref)|, d_ref
    from float64 AdamW: six sigma of the rounding noise, 6 x 2^-13 x sqrt(n 64) / 2 (n x 64 independent roundings, each with a
    standard deviation of at most half the ulp 2^-13 of a weight below 2^-5), is 2.9 % of it; the rest covers the second-order
    effect of the rounded moments (numpy model, tests/test_optim_sr.py: 0.2 %).  The default mode must FAIL the same bound."""
    from llm_fp8_amd.optim import ClippedAdamW
    n, steps, hp, p0, grads = displacement_inputs()
    ref = displacement_reference(p0, grads, hp)
    start = p0.double().numpy()
    grads = [g.to(dev) for g in grads]
    fig = {}
    for name, kw in (("bf16_sr", dict(stochastic_rounding=True, sr_seed=42)), ("bf16", {}), ("fp32", dict(state_dtype=F32))):
        p = torch.nn.Parameter(p0.clone().to(dev))
        opt = ClippedAdamW([p], max_grad_norm=None, **kw, **hp)
        for g in grads:
            p.grad = g
            opt.step()
        torch.cuda.synchronize()
        assert opt.state[p]["exp_avg"].dtype == (F32 if name == "fp32" else BF16)
        fig[name] = displacement_figures(_np(p), start, ref)
        print(f"{name:8s} summed displacement off by {100 * fig[name][0]:.3f} %, per-weight relative L2 error {fig[name][1]:.4f}, "
              f"weights that moved {100 * fig[name][2]:.1f} %")
        if name == "fp32":
            print(f"fp32     per-weight relative L2 error of the master {displacement_figures(_np(opt.state[p]['master']), start, ref)[1]:.3e}")
    assert fig["bf16_sr"][0] <= 0.05, fig
    assert fig["bf16"][0] > 0.05, fig


# ------------------------------------------------------------------------------------------------ 5: second-moment decay
def test_exp_avg_sq_decays_with_zero_gradients(dev):
    """b2 = 0.999 changes exp_avg_sq by 1e-3 of itself, below half a bf16 ulp (2^-9): round-to-nearest never lets it decay.
    65 536 elements at 2^-20, g = 0, 256 steps: mean / start within 1.5e-3 of 0.999^256 = 0.77404 (six sigma of the mean:
    6 x (ulp / v0 <= 2^-7) x sqrt(256) / (2 sqrt(n)) = 1.5e-3); the default mode leaves every element where it was."""
    from llm_fp8_amd.optim import ClippedAdamW
    n, steps, v0 = 65536, 256, 2.0 ** -20
    hp = dict(lr=1.41e-5, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2)
    for sr in (True, False):
        p = torch.nn.Parameter(torch.full((n,), 0.02, dtype=BF16, device=dev))
        p.grad = torch.zeros_like(p)
        opt = ClippedAdamW([p], max_grad_norm=None, stochastic_rounding=sr, sr_seed=42, **hp)
        opt.state[p] = {"step": 0, "exp_avg": torch.zeros_like(p), "exp_avg_sq": torch.full_like(p, v0)}
        for _ in range(steps):
            opt.step()
        torch.cuda.synchronize()
        v = _np(opt.state[p]["exp_avg_sq"])
        ratio = float(v.mean() / v0)
        print(f"stochastic rounding {sr}: mean(exp_avg_sq) / start after {steps} steps = {ratio:.5f} (0.999^256 = {0.999 ** 256:.5f})")
        if sr:
            assert abs(ratio - 0.999 ** 256) <= 1.5e-3, ratio
        else:
            assert (v == v0).all()


# ------------------------------------------------------------------------------------------------ 6: sinks
@pytest.mark.parametrize("mx", [False, True], ids=["per_tensor", "mxfp8"])
def test_sinks_are_bitwise_a_fresh_quantisation_of_the_rounded_weight(te_reset, dev, mx):
    from llm_fp8_amd.pytorch import ops
    # 200 x 144 and 224 x 160: 128 x 128 tiles ragged both ways (MXFP8 needs multiples of 32)
    lin = _sink_linear(dev, 160, 160, 224, _mx()) if mx else _sink_linear(dev, 144, 144, 200, _delayed())
    w = lin.weight
    opt = _sr_opt([w], seed=3, mgn=1.0, **G0)
    s = (opt._mx_sink_of if mx else opt._sink_of)(w)
    assert s is not None
    sink = s[0]
    amax0 = None if mx else sink.amax.clone()
    opt.step()
    torch.cuda.synchronize()
    assert sink.fresh()
    assert all(pl["chunks_cast"] is not None for pl in opt._plans.values())
    wq = w.detach().clone()
    if mx:
        for got, ref, name in zip((sink.w8, sink.sc, sink.wt8, sink.sct), ops.mxfp8_quantize(wq, ops.E4M3), ("w8", "sc", "wt8", "sct")):
            assert torch.equal(got, ref), f"MXFP8 sink {name} is not mi_mxfp8_quantize of the updated weight"
    else:
        y, yT = ops.cast_amax(wq, sink.scale, amax0, ops.E4M3)  # amax0: the slot as it was before the step, maxed as the step did
        assert torch.equal(sink.w8, y) and torch.equal(sink.w8t, yT), "FP8 sink is not mi_cast_amax of the updated weight"
        assert amax0.item() > 0 and torch.equal(sink.amax.view(torch.int32), amax0.view(torch.int32)), (sink.amax, amax0)


# ------------------------------------------------------------------------------------------------ 7: shards
def test_row_shards_draw_the_bits_of_the_whole_weight(te_reset, dev):
    """A 256 x 96 weight stepped whole, as two 128-row shards that write the rows of its sink (distributed.ShardedFP8DP's layout:
    `_mi_shard_of`), and as two plain 128-row tensors, each shard keyed (key of the whole, r0 x cols): identical bits."""
    N, K, key, seed = 256, 96, 3, 9
    lins = [_sink_linear(dev, 77, K, N, _delayed()) for _ in range(2)]
    wa, wb = lins[0].weight, lins[1].weight
    with torch.no_grad():
        wb.copy_(wa)
    grad = wa.grad.clone()
    start = wa.detach().clone()
    sa, sb = wa._mi_fp8_sink[0], wb._mi_fp8_sink[0]
    assert torch.equal(sa.scale, sb.scale)
    with torch.no_grad():
        sb.amax.copy_(sa.amax)

    wa._mi_sr_key = (key, 0)
    oa = _sr_opt([wa], seed=seed, mgn=1.0, **G0)
    assert oa._sink_of(wa) is not None
    oa.step()

    def shards(with_sink):
        out = []
        for r0 in (0, 128):
            sp = torch.nn.Parameter(start[r0:r0 + 128].clone())
            sp.grad = grad[r0:r0 + 128].clone()
            sp._mi_sr_key = (key, r0 * K)
            if with_sink:
                sp._mi_shard_of = (wb, r0, 128)
            out.append(sp)
        return out

    for with_sink in (True, False):
        sps = shards(with_sink)
        ob = _sr_opt(sps, seed=seed, mgn=1.0, **G0)
        assert all((ob._sink_of(sp) is not None) == with_sink for sp in sps)
        ob.step()
        torch.cuda.synchronize()
        assert torch.equal(oa.last_grad_norm, ob.last_grad_norm)
        for name, whole, parts in (("weight", wa.detach(), [sp.detach() for sp in sps]),
                                   ("exp_avg", oa.state[wa]["exp_avg"], [ob.state[sp]["exp_avg"] for sp in sps]),
                                   ("exp_avg_sq", oa.state[wa]["exp_avg_sq"], [ob.state[sp]["exp_avg_sq"] for sp in sps])):
            assert np.array_equal(_bits(whole), _bits(torch.cat(parts))), f"{name}: shards (sink {with_sink}) differ from the whole weight"
        if with_sink:
            assert torch.equal(sa.w8, sb.w8) and torch.equal(sa.w8t, sb.w8t), "the shards' rows of the sink differ"
            assert torch.equal(sa.amax.view(torch.int32), sb.amax.view(torch.int32))
    assert not np.array_equal(_bits(wa), _bits(start))


# ------------------------------------------------------------------------------------------------ 8: resume
def test_save_and_resume_continue_the_same_stream(dev):
    gen = torch.Generator().manual_seed(77)
    sizes = [(CHUNK + 8,), (129, 131)]
    init = [torch.randn(s, generator=gen).to(BF16) for s in sizes]
    grads = [[torch.randn(s, generator=gen).to(BF16).to(dev) for s in sizes] for _ in range(4)]
    make = lambda src: [torch.nn.Parameter(t.detach().clone().to(dev)) for t in src]

    def run(opt, params, steps):
        for gs in steps:
            for p, g in zip(params, gs):
                p.grad = g.clone()
            opt.step()

    pa = make(init)
    oa = _sr_opt(pa, seed=5, mgn=1.0, **G0)
    run(oa, pa, grads)
    pb = make(init)
    ob = _sr_opt(pb, seed=5, mgn=1.0, **G0)
    run(ob, pb, grads[:2])
    pc = make(pb)
    oc = _sr_opt(pc, seed=5, mgn=1.0, **G0)
    oc.load_state_dict(copy.deepcopy(ob.state_dict()))
    run(oc, pc, grads[2:])
    torch.cuda.synchronize()
    for a, c in zip(pa, pc):
        assert oa.state[a]["step"] == oc.state[c]["step"] == 4
        assert np.array_equal(_bits(a), _bits(c)), "p differs after the resume"
        for k in ("exp_avg", "exp_avg_sq"):
            assert oc.state[c][k].dtype == BF16 and np.array_equal(_bits(oa.state[a][k]), _bits(oc.state[c][k])), f"{k} differs after the resume"


# ------------------------------------------------------------------------------------------------ 9: the harness
def _harness_run(dev, scenario, seed):
    from llm_fp8_amd import train
    from llm_fp8_amd.optim import ClippedAdamW
    from llm_fp8_amd.pytorch.fp8 import FP8GlobalStateManager
    FP8GlobalStateManager.reset()
    cfg = train.TrainingConfig(model_name="llama-3.2-1b", num_hidden_layers=2, vocab_size=4096, batch_size=4, max_seq_length=128,
                               use_te=True, optimizer_state="bf16_sr", fp8_scenario=scenario, seed=seed)
    torch.manual_seed(3)
    model = train.prepare_model(train.create_model(cfg, dev), cfg)
    opt, sched = train.create_optimizer(model, cfg)
    assert type(opt) is ClippedAdamW and opt._sr and opt.state_dtype == BF16 and opt.sr_seed == seed
    assert [p._mi_sr_key for p in model.parameters()] == [(i, 0) for i, _ in enumerate(model.parameters())]
    model.train()
    gen = torch.Generator(device=dev).manual_seed(8)
    losses = [train.train_step(model, train.synthetic_batch(cfg, 4096, dev, gen), opt, sched, cfg).item() for _ in range(3)]
    torch.cuda.synchronize()
    return model, opt, losses


@pytest.mark.parametrize("scenario", ["default", "mxfp8"])
def test_training_harness_end_to_end(te_reset, dev, scenario, monkeypatch):
    from llm_fp8_amd.pytorch import ops
    monkeypatch.delenv("LLM_FP8_AMD_OPT_STATE", raising=False)
    monkeypatch.delenv("LLM_FP8_AMD_NO_OPT_WCAST", raising=False)
    model, opt, losses = _harness_run(dev, scenario, 42)
    assert all(math.isfinite(l) for l in losses), losses
    trainable = [p for p in model.parameters() if p.requires_grad]
    assert len(opt.state) == len(trainable) > 0
    for p in trainable:
        st = opt.state[p]
        assert st["step"] == 3 and set(st) == {"step", "exp_avg", "exp_avg_sq"} and st["exp_avg"].dtype == st["exp_avg_sq"].dtype == BF16
    checked = 0
    for mod in model.modules():
        for k, sink in list(getattr(mod, "_wcache", {}).items()):
            if not (isinstance(k, tuple) and k[0] in ("sink", "mxsink")):
                continue
            assert sink.fresh(), f"{type(mod).__name__} {k}: the optimiser left this sink stale"
            for w, lo, n in sink.parts:
                x = w.detach().contiguous()
                if k[0] == "sink":
                    y, yT = ops.cast_amax(x, sink.scale, None, ops.E4M3)
                    assert torch.equal(sink.w8[lo:lo + n], y) and torch.equal(sink.w8t[:, lo:lo + n], yT), (type(mod).__name__, k)
                else:
                    y, sc, wt, sct = ops.mxfp8_quantize(x, ops.E4M3)
                    assert (torch.equal(sink.w8[lo:lo + n], y) and torch.equal(sink.sc[:, lo:lo + n], sc)
                            and torch.equal(sink.wt8[:, lo:lo + n], wt) and torch.equal(sink.sct[lo // 32:(lo + n) // 32], sct)), (type(mod).__name__, k)
            checked += 1
    assert checked >= 2 * 4, checked  # per layer: q|k|v, proj, fc1, fc2
    first = [_bits(p) for p in trainable]
    del model, opt
    model2, _, losses2 = _harness_run(dev, scenario, 42)
    assert losses2 == losses
    assert all(np.array_equal(a, _bits(p)) for a, p in zip(first, (p for p in model2.parameters() if p.requires_grad))), "same seed, other bits"
    del model2
    model3, _, _ = _harness_run(dev, scenario, 43)
    assert any(not np.array_equal(a, _bits(p)) for a, p in zip(first, (p for p in model3.parameters() if p.requires_grad))), "another seed, same bits"


# ------------------------------------------------------------------------------------------------ 10: the default modes
def test_default_and_fp32_modes_do_not_reach_the_new_entry_point(dev, monkeypatch):
    from llm_fp8_amd import _lib
    from llm_fp8_amd.optim import ClippedAdamW
    real = _lib.require

    def require(name, why):
        if name == "mi_adamw_sr_bf16_multi":
            raise RuntimeError(f"{why} needs {name}")
        return real(name, why)
    monkeypatch.setattr(_lib, "require", require)
    gen = torch.Generator().manual_seed(1)
    for kw in ({}, dict(state_dtype=F32)):
        p = torch.nn.Parameter(torch.randn(CHUNK + 8, generator=gen).to(BF16).to(dev))
        before = p.detach().clone()
        p.grad = torch.randn(CHUNK + 8, generator=gen).to(BF16).to(dev)
        opt = ClippedAdamW([p], **kw, **G0)
        opt.step()
        torch.cuda.synchronize()
        assert not torch.equal(p.detach(), before)
        assert all("sr_seed" not in g and "stochastic_rounding" not in g for g in opt.state_dict()["param_groups"])
    q = torch.nn.Parameter(torch.randn(16, generator=gen).to(BF16).to(dev))
    q.grad = torch.zeros_like(q)
    with pytest.raises(RuntimeError, match="mi_adamw_sr_bf16_multi"):
        ClippedAdamW([q], stochastic_rounding=True, **G0).step()
