"""GPU: the per-tensor quantisers (module._DelayedQ, module._CurrentQ) against the primitives they are made of, called directly
here -- the call lists below are the specification -- bit for bit: FP8 bytes of both copies, partial column sums, the published
amax and the bits of the scale-inverse every copy carries.  And the KernelTimer spans of one step of a tiny Linear and a tiny
LayerNormMLP under delayed scaling, current scaling and MXFP8 (kind, label, work, bytes -- bench.py selects by kind), plus those
of the wrappers such a step does not reach.  What the bytes ARE is held against the oracles by test_kernels_gpu.py,
test_current_scaling_gpu.py and test_modules_gpu.py."""
import pytest
import torch

from oracle import fp8_oracle as O

pytestmark = pytest.mark.gpu

R, C, F = 64, 256, 512         # x [R, C]; h [R, 2F]; dact [R, F]
G = 1                          # GEMM index: forward slots 3 (input), 4 (weight), backward slot 2
KINDS = ["delayed", "current"]
FMTS = [O.E4M3, O.E5M2]
COPIES = [(True, True), (False, True), (True, False)]


@pytest.fixture(scope="module")
def data(dev):
    g = torch.Generator().manual_seed(355)
    bf = lambda t: t.to(torch.bfloat16).to(dev)
    return {"x": bf(torch.randn(R, C, generator=g) * 3), "h": bf(torch.randn(R, 2 * F, generator=g) * 2),
            "dact": bf(torch.randn(R, F, generator=g) / 16), "gamma": bf(1 + 0.1 * torch.randn(C, generator=g)),
            "rstd": (0.5 + torch.rand(R, generator=g)).to(dev), "bias": bf(torch.randn(2 * F, generator=g) / 4),
            "w": [bf(torch.randn(64, C, generator=g) / 8), (torch.randn(32, C, generator=g) / 4).to(dev),   # the middle part fp32
                  bf(torch.randn(32, C, generator=g) / 16)]}


class Env:
    """A quantiser of `kind` with both formats `fmt`, and the numbers one quantisation must use, obtained from the primitives."""

    def __init__(self, kind, fmt, dev):
        from llm_fp8_amd.common.recipe import Float8CurrentScaling, Format, QParams
        from llm_fp8_amd.pytorch import module as M, ops
        from llm_fp8_amd.pytorch.fp8 import MetaArena, ModuleMeta
        self.kind, self.fmt, self.ops, self.dev = kind, fmt, ops, dev
        if kind == "delayed":
            arenas = [MetaArena((Format.HYBRID, 4, "max", 0, fwd), dev) for fwd in (True, False)]
            for a, first in zip(arenas, (5, 3)):
                a.alloc(first)
            self.mf, self.mb = ModuleMeta(arenas[0], arenas[0].alloc(6), 6), ModuleMeta(arenas[1], arenas[1].alloc(4), 4)
            for a in arenas:                                 # another scale in every slot, its inverse beside it
                a.scale[:a.used] = 2.0 ** torch.arange(-3, a.used - 3, device=dev) * 1.3
                a.scale_inv[:a.used] = 1.0 / a.scale[:a.used]
            self.q = M._DelayedQ(self.mf, self.mb, fmt, fmt)
        else:
            self.qp = {"x": QParams(power_2_scale=True, amax_epsilon=0.0), "w": QParams(power_2_scale=False, amax_epsilon=1e-3),
                       "grad": QParams(power_2_scale=False, amax_epsilon=0.0)}
            self.q = M._CurrentQ(Float8CurrentScaling(fp8_quant_fwd_inp=self.qp["x"], fp8_quant_fwd_weight=self.qp["w"],
                                                      fp8_quant_bwd_grad=self.qp["grad"]), fmt, fmt)

    def slot(self, role):
        m, s = (self.mb, 2 * G) if role == "grad" else (self.mf, 3 * G + (role == "w"))
        return m.arena, m.start + s

    def numbers(self, role, passes):
        """-> (scale, amax destination or None, expected scale-inverse of the row copy, of the column copy).  Delayed scaling: a
        copy of the slot's scale, a zeroed amax cell of the test's own, the live scale-inverse and -- on what the forward saves --
        the snapshot's.  Current scaling: `passes` = [(amax pass, its arguments, grid)] run into segments of a partial buffer of
        the test's own, then ONE scale kernel; no amax destination, the triple's third element on every copy."""
        ops = self.ops
        if self.kind == "delayed":
            a, i = self.slot(role)
            a.hist[0, i] = 0
            live, snap = a.scale_inv[i:i + 1].clone(), a.snapshot()[i:i + 1].clone()
            si = {"x": (live, snap), "w": (snap, snap), "grad": (live, live)}[role]
            return a.scale[i:i + 1].clone(), torch.zeros(1, device=self.dev), si[0], si[1]
        grids = [ops.amax_grid(*grid) for _, _, grid in passes]
        part, o = torch.empty(sum(grids), dtype=torch.float32, device=self.dev), 0
        for (fn, args, _), n in zip(passes, grids):
            fn(*args, part[o:o + n])
            o += n
        t3 = ops.current_scale(part, ops.FP8_MAX[self.fmt], self.qp[role].amax_epsilon, self.qp[role].power_2_scale)
        return t3[1:2], None, t3[2:3], t3[2:3]

    def check(self, role, amax, got_pairs, want_data, si_row, si_col):
        """Bytes of both copies, the scale-inverse bits they carry, and (delayed scaling) the amax the quantiser published."""
        for (data, si), want, want_si in zip(got_pairs, want_data, (si_row, si_col)):
            assert (data is None) == (want is None)
            assert data is None or (data.dtype == torch.uint8 and torch.equal(data, want))
            assert si.shape == (1,) and torch.equal(si.view(torch.int32), want_si.view(torch.int32))
        if self.kind == "delayed":
            a, i = self.slot(role)
            assert torch.equal(a.hist[0, i:i + 1].view(torch.int32), amax.view(torch.int32)) and float(amax) > 0


@pytest.fixture(params=[(k, f) for k in KINDS for f in FMTS], ids=lambda p: f"{p[0]}-{'e4m3' if p[1] == O.E4M3 else 'e5m2'}")
def env(request, dev):
    from llm_fp8_amd import _lib
    assert _lib.load().mi_device_supported() == 1, "not a gfx950 device"
    return Env(*request.param, dev)


def _cs_same(got, want):
    assert (got is None) == (want is None)
    assert got is None or (got.dtype == torch.float32 and torch.equal(got.view(torch.int32), want.view(torch.int32)))


@pytest.mark.parametrize("want_t", [True, False])
def test_quantize(env, data, want_t):
    ops, x, rstd, gamma = env.ops, data["x"], data["rstd"], data["gamma"]
    scale, amax, si_row, si_col = env.numbers("x", [(ops.amax_bf16, (x,), (R, C))])
    want = ops.cast_amax(x, scale, amax, env.fmt, want_t=want_t)
    env.check("x", amax, env.q.quantize(x, G, want_t), want, si_row, si_col)
    scale, amax, si_row, si_col = env.numbers("x", [(ops.amax_norm, (x, rstd, gamma), (R, C))])
    want_n = ops.norm_cast(x, rstd, gamma, scale, amax, env.fmt, want_t=want_t)
    env.check("x", amax, env.q.quantize(x, G, want_t, norm=(rstd, gamma)), want_n, si_row, si_col)
    assert not torch.equal(want[0], want_n[0])


@pytest.mark.parametrize("with_bias", [False, True])
def test_swiglu(env, data, with_bias):
    ops, h, bias = env.ops, data["h"], (data["bias"] if with_bias else None)
    for want_t in (True, False):
        scale, amax, si_row, si_col = env.numbers("x", [(ops.amax_swiglu, (h, bias), (R, F, 32))])
        want = ops.swiglu_cast(h, scale, amax, env.fmt, want_t=want_t, bias=bias)
        env.check("x", amax, env.q.swiglu(h, G, want_t, bias), want, si_row, si_col)


@pytest.mark.parametrize("colsum", [False, True])
def test_quantize_grad(env, data, colsum):
    ops, g2 = env.ops, data["x"]
    for want_y, want_t in COPIES:
        scale, amax, si_row, si_col = env.numbers("grad", [(ops.amax_bf16, (g2,), (R, C))])
        want = ops.cast_amax(g2, scale, amax, env.fmt, want_y=want_y, want_t=want_t, want_colsum=colsum)
        row, col, cs = env.q.quantize_grad(g2, G, want_y, want_t, colsum=colsum)
        env.check("grad", amax, (row, col), want[:2], si_row, si_col)
        _cs_same(cs, want[2] if colsum else None)


@pytest.mark.parametrize("colsum", [False, True])
@pytest.mark.parametrize("with_bias", [False, True])
def test_dswiglu(env, data, with_bias, colsum):
    ops, h, dact, bias = env.ops, data["h"], data["dact"], (data["bias"] if with_bias else None)
    for want_y, want_t in COPIES:
        scale, amax, si_row, si_col = env.numbers("grad", [(ops.amax_dswiglu, (h, bias, dact), (R, F, 32))])
        want = ops.dswiglu_cast(h, dact, scale, amax, env.fmt, want_y=want_y, want_t=want_t, want_colsum=colsum, bias=bias)
        row, col, cs = env.q.dswiglu(h, dact, G, want_y, want_t, colsum, bias)
        env.check("grad", amax, (row, col), want[:2], si_row, si_col)
        _cs_same(cs, want[2])
        assert (cs is not None) == colsum


@pytest.mark.parametrize("want_t", [True, False])
@pytest.mark.parametrize("parts", [1, 3])
def test_quantize_weights(env, data, parts, want_t):
    """Rows 64 | 32 | 32 at K = 256, the middle part fp32: ONE scale for the operand, every part cast into its row block."""
    ops = env.ops
    ws = data["w"][:parts]
    ns = [w.shape[0] for w in ws]
    bf = [w.to(torch.bfloat16).contiguous() for w in ws]
    scale, amax, si_row, si_col = env.numbers("w", [(ops.amax_bf16, (w,), (n, C)) for w, n in zip(bf, ns)])
    outs = [ops.cast_amax(w, scale, amax, env.fmt, want_t=want_t) for w in bf]
    want8 = torch.cat([o[0] for o in outs], 0)
    want8t = torch.cat([o[1] for o in outs], 1) if want_t else None
    flat = env.q.quantize_weights(ws, ns, sum(ns), C, env.dev, G, want_t)
    assert len(flat) == 3 and flat[0].is_contiguous() and (flat[1] is None or flat[1].is_contiguous())
    env.check("w", amax, env.q.unflat(flat), (want8, want8t), si_row, si_col)


# ------------------------------------------------------------------------------------------------------------ timer spans
T = 256     # tokens of the step: with 256 x 256 tiles dividing every GEMM the backward pairs are eligible for the grouped launch


def _step_spans(dev, name):
    """(kind, label, work, bytes) of every span of one forward + backward of Linear(256 -> 512) and LayerNormMLP(256 / 512), both
    with biases, on T tokens, under recipe `name`.  The grouped-launch decision is the count model's (no timing)."""
    import llm_fp8_amd.pytorch as te
    from llm_fp8_amd.common import recipe as RC
    from llm_fp8_amd.pytorch.fp8 import FP8GlobalStateManager
    from llm_fp8_amd.pytorch.profiler import KernelTimer
    recipe = {"delayed": RC.DelayedScaling, "current": RC.Float8CurrentScaling, "mxfp8": RC.MXFP8BlockScaling}[name]()
    FP8GlobalStateManager.reset()
    torch.manual_seed(11)
    lin = te.Linear(256, 512, bias=True, params_dtype=torch.bfloat16, device=dev)
    mlp = te.LayerNormMLP(256, 512, bias=True, normalization="RMSNorm", activation="swiglu", params_dtype=torch.bfloat16, device=dev)
    x = torch.randn(T, 256, device=dev, dtype=torch.bfloat16, requires_grad=True)
    dy, dz = torch.randn(T, 512, device=dev, dtype=torch.bfloat16), torch.randn(T, 256, device=dev, dtype=torch.bfloat16)
    timer = KernelTimer()
    try:
        with timer.install():
            with te.fp8_autocast(enabled=True, fp8_recipe=recipe):
                y, z = lin(x), mlp(x)
            y.backward(dy)
            z.backward(dz)
        torch.cuda.synchronize()
    finally:
        FP8GlobalStateManager.reset()
    assert KernelTimer.active is None
    return [s[:4] for s in timer.spans]


# recorded on the commit before the quantisers and the launch wrappers were unified (repr: 2.0 and 2 are different entries)
STEP_SPANS = {
    "delayed": [
        ('cast_amax', '256x256', 65536.0, 262144.0),
        ('cast_amax', '512x256', 131072.0, 524288.0),
        ('gemm_fp8', '256x512x256', 67108864.0, 458752),
        ('cast_amax', '256x256', 65536.0, 262144.0),
        ('cast_amax', '1024x256', 262144.0, 1048576.0),
        ('gemm_fp8', '256x1024x256', 134217728.0, 851968),
        ('swiglu_cast', '256x512', 131072.0, 786432.0),
        ('cast_amax', '256x512', 131072.0, 524288.0),
        ('gemm_fp8', '256x256x512', 67108864.0, 393216),
        ('cast_amax', '256x512', 131072.0, 524288.0),
        ('gemm_fp8', '256x256x512+512x256x256', 134217728.0, 851968),
        ('cast_amax', '256x256', 65536.0, 262144.0),
        ('gemm_fp8', '256x512x256+256x512x256', 134217728.0, 917504),
        ('dswiglu_cast', '256x512', 262144.0, 1310720.0),
        ('gemm_fp8', '256x256x1024+1024x256x256', 268435456.0, 1507328),
    ],
    "current": [
        ('amax', '256x256', 65536.0, 131072.0),
        ('cast_amax', '256x256', 65536.0, 262144.0),
        ('amax', '512x256', 131072.0, 262144.0),
        ('cast_amax', '512x256', 131072.0, 524288.0),
        ('gemm_fp8', '256x512x256', 67108864.0, 458752),
        ('amax', '256x256', 65536.0, 131072.0),
        ('cast_amax', '256x256', 65536.0, 262144.0),
        ('amax', '1024x256', 262144.0, 524288.0),
        ('cast_amax', '1024x256', 262144.0, 1048576.0),
        ('gemm_fp8', '256x1024x256', 134217728.0, 851968),
        ('amax', 'swiglu 256x512', 131072.0, 524288.0),
        ('swiglu_cast', '256x512', 131072.0, 786432.0),
        ('amax', '256x512', 131072.0, 262144.0),
        ('cast_amax', '256x512', 131072.0, 524288.0),
        ('gemm_fp8', '256x256x512', 67108864.0, 393216),
        ('amax', '256x512', 131072.0, 262144.0),
        ('cast_amax', '256x512', 131072.0, 524288.0),
        ('gemm_fp8', '256x256x512+512x256x256', 134217728.0, 851968),
        ('amax', '256x256', 65536.0, 131072.0),
        ('cast_amax', '256x256', 65536.0, 262144.0),
        ('gemm_fp8', '256x512x256+256x512x256', 134217728.0, 917504),
        ('amax', 'dswiglu 256x512', 262144.0, 786432.0),
        ('dswiglu_cast', '256x512', 262144.0, 1310720.0),
        ('gemm_fp8', '256x256x1024+1024x256x256', 268435456.0, 1507328),
    ],
    "mxfp8": [
        ('mxfp8_quantize', '256x256', 65536.0, 266240.0),
        ('mxfp8_quantize', '512x256', 131072.0, 532480.0),
        ('gemm_mxfp8', '256x512x256', 67108864.0, 458752),
        ('mxfp8_quantize', '256x256', 65536.0, 266240.0),
        ('mxfp8_quantize', '1024x256', 262144.0, 1064960.0),
        ('gemm_mxfp8', '256x1024x256', 134217728.0, 851968),
        ('mxfp8_quantize', 'swiglu 256x512', 131072.0, 794624.0),
        ('mxfp8_quantize', '256x512', 131072.0, 532480.0),
        ('gemm_mxfp8', '256x256x512', 67108864.0, 393216),
        ('mxfp8_quantize', '256x512', 131072.0, 532480.0),
        ('gemm_mxfp8', '256x256x512+512x256x256', 134217728.0, 851968),
        ('mxfp8_quantize', '256x256', 65536.0, 266240.0),
        ('gemm_mxfp8', '256x512x256+256x512x256', 134217728.0, 917504),
        ('mxfp8_quantize', 'dswiglu 256x1024', 262144.0, 1327104.0),
        ('gemm_mxfp8', '256x256x1024+1024x256x256', 268435456.0, 1507328),
    ],
}


@pytest.mark.parametrize("name", ["delayed", "current", "mxfp8"])
def test_step_spans(dev, monkeypatch, name):
    monkeypatch.setenv("LLM_FP8_AMD_GROUPED_GEMM", "plan")
    monkeypatch.delenv("LLM_FP8_AMD_NO_GROUPED_GEMM", raising=False)
    monkeypatch.delenv("LLM_FP8_AMD_GEMM_ALGO", raising=False)
    got = _step_spans(dev, name)
    print(name, repr(got))
    assert repr(got) == repr(STEP_SPANS[name])


def _direct_spans(dev):
    """The wrappers a step of those two modules does not reach (hidden 256 is below what the fused norm takes), one call each: the
    norm cast, both grouped GEMM launches with the tile shape given, the RoPE-backward cast and the attention pair."""
    from llm_fp8_amd.pytorch import ops
    from llm_fp8_amd.pytorch.profiler import KernelTimer
    g = torch.Generator().manual_seed(9)
    u8 = lambda *s: torch.randint(0, 120, s, generator=g, dtype=torch.uint8).to(dev)
    one = torch.ones(1, device=dev)
    out = lambda m, n: torch.empty((m, n), dtype=torch.bfloat16, device=dev)
    e8 = lambda *s: torch.full(s, 127, dtype=torch.uint8, device=dev)
    pt = [(u8(256, 256), u8(512, 256), one, one, out(256, 512)), (u8(512, 256), u8(256, 256), one, one, out(512, 256))]
    mx = [(a, e8(256 // 32, a.shape[0]), b, e8(256 // 32, b.shape[0]), o) for a, b, _, _, o in pt]
    seq, n_q, n_kv, D = 128, 2, 1, 128
    x, rstd = torch.randn(R, C, generator=g).to(torch.bfloat16).to(dev), torch.ones(R, device=dev)
    gamma = torch.ones(C, dtype=torch.bfloat16, device=dev)
    dq, dk, dv = ((torch.randn(seq, n * D, generator=g)).to(torch.bfloat16).to(dev) for n in (n_q, n_kv, n_kv))
    ang = torch.outer(torch.arange(seq, dtype=torch.float32), 1.0 / (10000.0 ** (torch.arange(0, D, 2, dtype=torch.float32) / D)))
    cos, sin = torch.cos(ang).contiguous().to(dev), torch.sin(ang).contiguous().to(dev)
    q4, k4, v4 = (torch.randn(1, seq, n, D, generator=g).to(torch.bfloat16).to(dev) for n in (n_q, n_kv, n_kv))
    timer = KernelTimer()
    with timer.install():
        ops.norm_cast(x, rstd, gamma, one, None, O.E4M3)
        ops.gemm_fp8_grouped(pt, O.E5M2, O.E4M3, tile_cfg=0)
        ops.gemm_mxfp8_grouped(mx, O.E5M2, O.E4M3, tile_cfg=0)
        ops.rope_qkv_backward_cast(dq, dk, dv, cos, sin, n_q, n_kv, D, seq, one, None, O.E5M2, want_y=True, want_t=False)
        o4, lse = ops.attn_fwd(q4, k4, v4, D ** -0.5, causal=True)
        ops.attn_bwd(torch.ones_like(o4), q4, k4, v4, o4, lse, D ** -0.5, causal=True)
    torch.cuda.synchronize()
    return [s[:4] for s in timer.spans]


# (from the wrappers' span arguments on that commit: elements / FLOPs as floats; the GEMMs' byte counts are integers)
DIRECT_SPANS = [
    ('norm_cast', '64x256', 16384.0, 65536.0),
    ('gemm_fp8', '256x512x256+512x256x256', 134217728.0, 917504),
    ('gemm_mxfp8', '256x512x256+512x256x256', 134217728.0, 917504),
    ('cast_amax', 'rope 128x512', 65536.0, 196608.0),
    ('attn_fwd', '1x128x2x128', 8388608.0, 196608.0),
    ('attn_bwd', '1x128x2x128', 29360128.0, 327680.0),
]


def test_direct_spans(dev):
    got = _direct_spans(dev)
    print(repr(got))
    assert repr(got) == repr(DIRECT_SPANS)
