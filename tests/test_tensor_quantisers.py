"""CPU: the per-tensor quantisers (module._DelayedQ, module._CurrentQ) characterised call by call.  Every ops function they launch
through is replaced by a recording fake on CPU tensors; pinned are the exact sequence of calls, every argument, and WHICH tensors
are handed over and returned -- delayed scaling: the meta slots 3g (input), 3g + 1 (weight) of the forward window and 2g of the
backward one, the live scale-inverse on what is consumed in the same pass and the arena's snapshot on what is saved for backward,
no amax pass, no grid lookup, no scale kernel; current scaling: amax pass(es) into the partial buffer, ONE scale kernel, the cast
reading view [1:2] of its triple with amax=None, every copy carrying view [2:3]."""
import inspect

import pytest
import torch

from llm_fp8_amd.common.recipe import Float8CurrentScaling, Format, QParams
from llm_fp8_amd.pytorch import module as M
from llm_fp8_amd.pytorch import ops
from llm_fp8_amd.pytorch.fp8 import MetaArena, ModuleMeta

CPU = torch.device("cpu")
G = 1                          # the GEMM's index in its module: slots 3, 4 (forward) and 2 (backward) of the windows below
FMT_F, FMT_B = ops.E4M3, ops.E5M2
R, C, F = 64, 96, 48           # x [R, C]; h [R, 2F]; dact [R, F]
AMAX_PASSES = ("amax_bf16", "amax_norm", "amax_swiglu", "amax_dswiglu")
CURRENT_ONLY = AMAX_PASSES + ("amax_partial", "amax_grid", "current_scale")
FAKED = ("cast_amax", "norm_cast", "swiglu_cast", "dswiglu_cast", "gemm_fp8") + CURRENT_ONLY
QP = {"x": QParams(power_2_scale=True, amax_epsilon=1e-3), "w": QParams(power_2_scale=False, amax_epsilon=2e-3),
      "grad": QParams(power_2_scale=True, amax_epsilon=3e-3)}


def _loc(t):
    return (t.untyped_storage().data_ptr(), t.storage_offset(), tuple(t.shape), tuple(t.stride()), t.dtype)


def _eq(got, want) -> bool:
    """Tensors: the same memory seen the same way (a view equals another view of the same elements); a predicate: called."""
    if isinstance(want, torch.Tensor):
        return isinstance(got, torch.Tensor) and _loc(got) == _loc(want)
    if callable(want):
        return bool(want(got))
    return type(got) is type(want) and got == want


def _u8(*shape):
    return torch.zeros(shape, dtype=torch.uint8)


class Recorder:
    """Fakes of the ops functions: each records (name, all parameters by name, defaults filled in) and returns what the real one
    would, as CPU tensors.  `grid` of the fake amax_grid: rows // 32 + 1 workgroups."""

    def __init__(self, monkeypatch, arenas=()):
        self.calls, self.triples, self.snap_made = [], [], []
        self.buf = torch.zeros(64, dtype=torch.float32)     # the device's partial buffer
        self.arenas = arenas
        for name in FAKED:
            monkeypatch.setattr(ops, name, self._fake(name, inspect.signature(getattr(ops, name))))

    def _fake(self, name, sig):
        def fake(*a, **k):
            bound = sig.bind(*a, **k)
            bound.apply_defaults()
            args = dict(bound.arguments)
            self.calls.append((name, args))
            return getattr(self, "_" + name, lambda **kw: None)(**args)
        return fake

    def _pair(self, rows, cols, want_y, want_t, y=None, yT=None):
        self.snap_made.append(tuple(a._snap is not None for a in self.arenas))   # at the time of the cast
        return (y if y is not None or not want_y else _u8(rows, cols)), (yT if yT is not None or not want_t else _u8(cols, rows))

    def _cast_amax(self, x, scale, amax, fmt, want_y, want_t, y, yT, want_colsum):
        pair = self._pair(*x.shape, want_y, want_t, y, yT)
        return (*pair, torch.zeros((x.shape[0] + 63) // 64, x.shape[1])) if want_colsum else pair

    def _norm_cast(self, x, rstd, gamma, scale, amax, fmt, want_y, want_t):
        return self._pair(*x.shape, want_y, want_t)

    def _swiglu_cast(self, h, scale, amax, fmt, want_y, want_t, bias):
        return self._pair(h.shape[0], h.shape[1] // 2, want_y, want_t)

    def _dswiglu_cast(self, h, dact, scale, amax, fmt, want_y, want_t, want_colsum, bias):
        return (*self._pair(*h.shape, want_y, want_t), torch.zeros((h.shape[0] + 127) // 128, h.shape[1]) if want_colsum else None)

    def _gemm_fp8(self, a8, b8, **kw):
        return torch.zeros(a8.shape[0], b8.shape[0], dtype=torch.bfloat16)

    def _amax_grid(self, rows, cols, tile_rows):
        return rows // 32 + 1

    def _amax_partial(self, device, n):
        return self.buf[:n]

    def _current_scale(self, partial, fp8_max, amax_epsilon, pow2):
        self.triples.append(torch.zeros(3, dtype=torch.float32))
        return self.triples[-1]

    def check(self, expected):
        assert [c[0] for c in self.calls] == [e[0] for e in expected]
        for i, ((name, got), (_, want)) in enumerate(zip(self.calls, expected)):
            assert list(got) == list(want), (i, name, list(got), list(want))
            for key in want:
                assert _eq(got[key], want[key]), (i, name, key, got[key], want[key])


# the calls as the quantisers make them, every parameter spelled out (the defaults are those of ops at the time of writing)
def cast_amax(x, scale, amax, fmt, want_y=True, want_t=True, y=None, yT=None, want_colsum=False):
    return "cast_amax", dict(x=x, scale=scale, amax=amax, fmt=fmt, want_y=want_y, want_t=want_t, y=y, yT=yT, want_colsum=want_colsum)


def norm_cast(x, rstd, gamma, scale, amax, fmt, want_y=True, want_t=True):
    return "norm_cast", dict(x=x, rstd=rstd, gamma=gamma, scale=scale, amax=amax, fmt=fmt, want_y=want_y, want_t=want_t)


def swiglu_cast(h, scale, amax, fmt, want_y=True, want_t=True, bias=None):
    return "swiglu_cast", dict(h=h, scale=scale, amax=amax, fmt=fmt, want_y=want_y, want_t=want_t, bias=bias)


def dswiglu_cast(h, dact, scale, amax, fmt, want_y=True, want_t=True, want_colsum=False, bias=None):
    return "dswiglu_cast", dict(h=h, dact=dact, scale=scale, amax=amax, fmt=fmt, want_y=want_y, want_t=want_t,
                                want_colsum=want_colsum, bias=bias)


def amax_grid(rows, cols, tile_rows=64):
    return "amax_grid", dict(rows=rows, cols=cols, tile_rows=tile_rows)


class Env:
    """One quantiser of `kind` ("delayed" / "current") over recording fakes, and what a quantisation of `role` must use."""

    def __init__(self, kind, monkeypatch):
        self.kind = kind
        if kind == "delayed":
            fwd, bwd = MetaArena((Format.HYBRID, 4, "max", 0, True), CPU), MetaArena((Format.HYBRID, 4, "max", 0, False), CPU)
            fwd.alloc(5), bwd.alloc(3)                      # windows that do not start at slot 0 of their arenas
            self.mf, self.mb = ModuleMeta(fwd, fwd.alloc(6), 6), ModuleMeta(bwd, bwd.alloc(4), 4)
            self.rec = Recorder(monkeypatch, (fwd, bwd))
            self.q = M._DelayedQ(self.mf, self.mb, FMT_F, FMT_B)
        else:
            self.recipe = Float8CurrentScaling(fp8_format=Format.HYBRID, fp8_quant_fwd_inp=QP["x"], fp8_quant_fwd_weight=QP["w"],
                                               fp8_quant_bwd_grad=QP["grad"])
            self.rec = Recorder(monkeypatch)
            self.q = M._CurrentQ(self.recipe, FMT_F, FMT_B)

    def numbers(self, role, passes):
        """-> (the calls in front of the cast, scale, amax destination, scale-inverse on the row copy, on the column copy).
        `passes`: the amax passes of current scaling as (grid call, pass name, its arguments without `partial`) -- call AFTER the
        method under test (it reads the triple the fake scale kernel returned, and the arena's snapshot)."""
        if self.kind == "delayed":
            m, s = (self.mb, 2 * G) if role == "grad" else (self.mf, 3 * G + (role == "w"))
            a, i = m.arena, m.start + s
            live = a.scale_inv[i:i + 1]
            snap = None if role == "grad" else a._snap[i:i + 1]      # (a gradient makes no snapshot of the backward arena)
            si = {"x": (live, snap), "w": (snap, snap), "grad": (live, live)}[role]
            return [], a.scale[i:i + 1], a.hist[0, i:i + 1], si[0], si[1]
        assert len(self.rec.triples) == 1
        t3, buf = self.rec.triples[0], self.rec.buf
        grids = [g[1]["rows"] // 32 + 1 for g, _, _ in passes]
        pre, o = [g for g, _, _ in passes] + [("amax_partial", dict(device=CPU, n=sum(grids)))], 0
        for (_, name, args), n in zip(passes, grids):
            pre.append((name, dict(**args, partial=buf[o:o + n])))
            o += n
        fmt = FMT_B if role == "grad" else FMT_F
        pre.append(("current_scale", dict(partial=buf[:o], fp8_max=ops.FP8_MAX[fmt], amax_epsilon=QP[role].amax_epsilon,
                                          pow2=QP[role].power_2_scale)))
        return pre, t3[1:2], None, t3[2:3], t3[2:3]


@pytest.fixture(params=["delayed", "current"])
def env(request, monkeypatch):
    return Env(request.param, monkeypatch)


def _bf(*shape, seed=0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)).to(torch.bfloat16)


def _operand(got, y, si):
    """A (data, scale-inverse) pair: `y` is the very tensor the cast returned (or None), `si` the expected one-element view."""
    assert got[0] is y and _eq(got[1], si), (got, y, si)


# ------------------------------------------------------------------------------------------------------------ activations
@pytest.mark.parametrize("want_t", [True, False])
@pytest.mark.parametrize("with_norm", [False, True])
def test_quantize(env, with_norm, want_t):
    x2 = _bf(R, C)
    norm = (torch.rand(R), _bf(C, seed=1)) if with_norm else None
    row, col = env.q.quantize(x2, G, want_t, norm=norm)
    if with_norm:
        pre, scale, amax, si_row, si_col = env.numbers("x", [(amax_grid(R, C), "amax_norm", dict(x=x2, rstd=norm[0], gamma=norm[1]))])
        env.rec.check(pre + [norm_cast(x2, norm[0], norm[1], scale, amax, FMT_F, want_t=want_t)])
    else:
        pre, scale, amax, si_row, si_col = env.numbers("x", [(amax_grid(R, C), "amax_bf16", dict(x=x2))])
        env.rec.check(pre + [cast_amax(x2, scale, amax, FMT_F, want_t=want_t)])
    assert (amax is None) == (env.kind == "current")
    y, yT = row[0], col[0]
    assert y.shape == (R, C) and ((yT is None) if not want_t else yT.shape == (C, R))
    _operand(row, y, si_row)
    _operand(col, yT, si_col)


@pytest.mark.parametrize("want_t", [True, False])
@pytest.mark.parametrize("with_bias", [False, True])
def test_swiglu(env, with_bias, want_t):
    h, bias = _bf(R, 2 * F), (_bf(2 * F, seed=2) if with_bias else None)
    row, col = env.q.swiglu(h, G, want_t, bias)
    pre, scale, amax, si_row, si_col = env.numbers("x", [(amax_grid(R, F, 32), "amax_swiglu", dict(h=h, bias=bias))])
    env.rec.check(pre + [swiglu_cast(h, scale, amax, FMT_F, want_t=want_t, bias=bias)])
    assert (amax is None) == (env.kind == "current")
    assert row[0].shape == (R, F) and ((col[0] is None) if not want_t else col[0].shape == (F, R))
    _operand(row, row[0], si_row)
    _operand(col, col[0], si_col)


# ------------------------------------------------------------------------------------------------------------ gradients
COPIES = [(True, True), (False, True), (True, False)]


@pytest.mark.parametrize("want_y,want_t", COPIES)
@pytest.mark.parametrize("colsum", [False, True])
def test_quantize_grad(env, colsum, want_y, want_t):
    g2 = _bf(R, C)
    row, col, cs = env.q.quantize_grad(g2, G, want_y, want_t, colsum=colsum)
    pre, scale, amax, si_row, si_col = env.numbers("grad", [(amax_grid(R, C), "amax_bf16", dict(x=g2))])
    env.rec.check(pre + [cast_amax(g2, scale, amax, FMT_B, want_y=want_y, want_t=want_t, want_colsum=colsum)])
    assert (amax is None) == (env.kind == "current")
    assert (row[0] is not None) == want_y and (col[0] is not None) == want_t
    assert (cs.shape == (1, C)) if colsum else (cs is None)
    _operand(row, row[0], si_row)
    _operand(col, col[0], si_col)


@pytest.mark.parametrize("want_y,want_t", COPIES)
@pytest.mark.parametrize("colsum", [False, True])
@pytest.mark.parametrize("with_bias", [False, True])
def test_dswiglu(env, with_bias, colsum, want_y, want_t):
    h, dact, bias = _bf(R, 2 * F), _bf(R, F, seed=3), (_bf(2 * F, seed=2) if with_bias else None)
    row, col, cs = env.q.dswiglu(h, dact, G, want_y, want_t, colsum, bias)
    pre, scale, amax, si_row, si_col = env.numbers("grad", [(amax_grid(R, F, 32), "amax_dswiglu", dict(h=h, bias=bias, dact=dact))])
    env.rec.check(pre + [dswiglu_cast(h, dact, scale, amax, FMT_B, want_y=want_y, want_t=want_t, want_colsum=colsum, bias=bias)])
    assert (amax is None) == (env.kind == "current")
    assert (row[0] is not None) == want_y and (col[0] is not None) == want_t
    assert (cs.shape == (1, 2 * F)) if colsum else (cs is None)
    _operand(row, row[0], si_row)
    _operand(col, col[0], si_col)


# ------------------------------------------------------------------------------------------------------------ weights
@pytest.mark.parametrize("want_t", [True, False])
@pytest.mark.parametrize("parts", ["one", "three"])
def test_quantize_weights(env, parts, want_t):
    """Rows 64 | 32 | 32 at K = 64, the middle part fp32 and the last one a non-contiguous view: every part is cast into its row
    block of ONE operand; a bf16 contiguous part is handed over as it is, another one converted once."""
    K = 64
    if parts == "one":
        ws = [_bf(64, K)]
    else:
        ws = [_bf(64, K), _bf(32, K, seed=1).float(), _bf(K, 32, seed=2).t()]
    ns = [w.shape[0] for w in ws]
    N = sum(ns)
    w8, w8t, siw = env.q.quantize_weights(ws, ns, N, K, CPU, G, want_t)
    assert w8.shape == (N, K) and w8.dtype == torch.uint8 and ((w8t is None) if not want_t else (w8t.shape == (K, N) and w8t.dtype == torch.uint8))
    casts = [c for c in env.rec.calls if c[0] == "cast_amax"]
    assert len(casts) == len(ws)
    sent = [c[1]["x"] for c in casts]                        # what the casts were handed: checked here, then expected as such
    for w, x in zip(ws, sent):
        assert x.dtype == torch.bfloat16 and x.is_contiguous() and torch.equal(x, w.to(torch.bfloat16))
        assert (x is w) == (w.dtype == torch.bfloat16 and w.is_contiguous())
    pre, scale, amax, si_row, si_col = env.numbers("w", [(amax_grid(n, K), "amax_bf16", dict(x=(lambda got, x=x: got is x)))
                                                         for n, x in zip(ns, sent)])
    expected, r = pre, 0
    for n, x in zip(ns, sent):
        expected.append(cast_amax(lambda got, x=x: got is x, scale, amax, FMT_F, y=w8[r:r + n], yT=w8t[:, r:r + n] if want_t else None,
                                  want_t=want_t))
        r += n
    env.rec.check(expected)
    assert (amax is None) == (env.kind == "current")
    assert _eq(siw, si_row) and _eq(siw, si_col)            # one scale-inverse for both copies: the snapshot's / the triple's
    (a, sa), (b, sb) = env.q.unflat((w8, w8t, siw))
    assert a is w8 and b is w8t and sa is siw and sb is siw


# ------------------------------------------------------------------------------------------------------------ the rest
def test_delayed_scaling_measures_nothing_and_snapshots_after_the_first_cast(monkeypatch):
    """No amax pass, no grid (device-property) lookup, no partial buffer, no scale kernel under delayed scaling -- and the arena's
    snapshot (one device copy per step) is made after the first cast has been launched, not before it."""
    env = Env("delayed", monkeypatch)
    x2, h, dact = _bf(R, C), _bf(R, 2 * F), _bf(R, F)
    assert env.mf.arena._snap is None and env.mb.arena._snap is None
    env.q.quantize(x2, G, True)
    assert env.rec.snap_made == [(False, False)] and env.mf.arena._snap is not None
    env.q.quantize(x2, G, True, norm=(torch.rand(R), _bf(C)))
    env.q.swiglu(h, G, True, None)
    env.q.quantize_weights([_bf(64, 64), _bf(32, 64)], [64, 32], 96, 64, CPU, G, True)
    env.q.quantize_grad(x2, G, True, True, colsum=True)
    env.q.dswiglu(h, dact, G, True, True, True, None)
    assert env.mb.arena._snap is None                       # gradients carry the live scale-inverse only
    names = [c[0] for c in env.rec.calls]
    assert names == ["cast_amax", "norm_cast", "swiglu_cast", "cast_amax", "cast_amax", "cast_amax", "dswiglu_cast"]
    assert not set(names) & set(CURRENT_ONLY)


def test_operands_and_gemm(env):
    a, b = (_u8(R, C), torch.ones(1)), (_u8(32, C), torch.ones(1))
    assert all(x is y for x, y in zip(env.q.operands(a, b), (a[0], b[0], a[1], b[1])))
    bias = _bf(32)
    out = env.q.gemm(a, b, bias)
    assert out.shape == (R, 32)
    env.rec.check([("gemm_fp8", dict(a8=a[0], b8=b[0], sa_inv=a[1], sb_inv=b[1], fmt_a=FMT_F, fmt_b=FMT_F, bias=bias, out=None,
                                     out_dtype=torch.bfloat16, algo=None))])
    for cls in (M._DelayedQ, M._CurrentQ):
        assert cls.mx is False and cls.swiglu_adds_bias is True and cls.colsum_dtypes is None
    assert (M._DelayedQ.cache_key, M._DelayedQ.sink_key, M._CurrentQ.cache_key, M._CurrentQ.sink_key) == ("ds", "sink", "cs", "cssink")
    assert "Float8CurrentScaling" in M._CurrentQ.no_sink and "Float8CurrentScaling" not in M._DelayedQ.no_sink


def test_offer_taken_and_sinks(env):
    q, h = env.q, M.DyHandoff()
    q.offer(h, G, True, False)
    fp8 = (_u8(R, C), _u8(C, R))
    if env.kind == "current":
        assert not h.offered() and q.new_sink((), (), 256, 256, CPU, G) is None
        with pytest.raises(RuntimeError, match="Float8CurrentScaling offers no DyHandoff"):
            q.taken(fp8, G)
        return
    a, i = env.mb.arena, env.mb.start + 2 * G
    assert h.offered() and _eq(h.scale, a.scale[i:i + 1]) and _eq(h.amax, a.hist[0, i:i + 1])
    assert (h.fmt, h.want_y, h.want_t, h.mx) == (FMT_B, True, False, False)
    row, col, cs = q.taken(fp8, G)
    assert cs is None
    _operand(row, fp8[0], a.scale_inv[i:i + 1])
    _operand(col, fp8[1], a.scale_inv[i:i + 1])
    w = torch.nn.Parameter(_bf(64, 64))
    sink = q.new_sink([w], [64], 64, 64, CPU, G)
    fa, fi = env.mf.arena, env.mf.start + 3 * G + 1
    assert isinstance(sink, M.WeightSink) and _eq(sink.scale, fa.scale[fi:fi + 1]) and _eq(sink.amax, fa.hist[0, fi:fi + 1])
    assert q.new_sink([w], [60], 60, 64, CPU, G) is None
    w8, w8t, siw = q.sink_flat(sink, G)
    assert w8 is sink.w8 and w8t is sink.w8t and _eq(siw, fa._snap[fi:fi + 1])
    assert env.rec.calls == []
