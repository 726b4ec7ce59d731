"""GPU: the block-scaled quantiser family behind one host path.  The eight public functions (ops.mxfp8_* and ops.blockfp8_* for the
plain, norm, swiglu and dswiglu producers) are forwards to one implementation per producer that takes the granularity -- None for
MX, (dim, amax_epsilon) for Float8BlockScaling.  Pinned here: every forward hands `dim`, `amax_epsilon`, `out=` and `want_colsum`
through unchanged (bit for bit against the implementation called directly), and the KernelTimer spans keep their kind, label and
element / byte counts.  What the bytes ARE is held by test_block_scaling_gpu.py and test_kernels_gpu.py against the oracles."""
import math

import pytest
import torch

from oracle import fp8_oracle as O

pytestmark = pytest.mark.gpu

R, C = 160, 96          # both dimensions end in a partial 128 tile; with F = 96 the dSwiGLU up half begins inside a 128-column tile
EPS = 2.0 ** -10
GRANS = [None, (1, EPS), (2, EPS)]
ORIENT = [(True, False), (False, True), (True, True)]
FMAX = {O.E4M3: 448.0, O.E5M2: 57344.0}


@pytest.fixture(scope="module")
def ops(dev):
    from llm_fp8_amd.pytorch import ops as _ops
    from llm_fp8_amd import _lib
    assert _lib.load().mi_device_supported() == 1, "not a gfx950 device"
    return _ops


@pytest.fixture(scope="module")
def data(dev):
    """Inputs whose result depends on the granularity AND on amax_epsilon: row scales spread over decades, a block of values
    far below EPS, and rows 128.. all zero (an all-zero 1 x 128 block in every such row, an all-zero 128 x 128 tile)."""
    g = torch.Generator().manual_seed(96)
    spread = torch.exp(torch.randn(R, 1, generator=g) * 3)
    x = torch.randn(R, C, generator=g) * spread
    x[3, 32:64] = 1e-30
    x[128:] = 0
    h = torch.randn(R, 2 * C, generator=g) * spread.clamp(max=8.0)
    h[128:] = 0
    dact = torch.randn(R, C, generator=g) * spread
    dact[128:] = 0
    bf = lambda t: t.to(torch.bfloat16).to(dev)
    return {"x": bf(x), "h": bf(h), "dact": bf(dact), "gamma": bf(1 + 0.1 * torch.randn(C, generator=g)),
            "rstd": (1 / spread[:, 0]).float().to(dev)}


def _same(got, want):
    assert len(got) == len(want)
    for a, b in zip(got, want):
        assert (a is None) == (b is None)
        assert a is None or (a.dtype == b.dtype and torch.equal(a, b))


def _public(ops, prod, gran):
    """The public function of (producer, granularity) with the granularity bound the way a caller passes it."""
    if gran is None:
        return getattr(ops, "mxfp8_" + prod)
    fn = getattr(ops, "blockfp8_" + prod)
    return lambda *a, **k: fn(*a, dim=gran[0], amax_epsilon=gran[1], **k)


# ------------------------------------------------------------------------------------------------------------ forward equality
@pytest.mark.parametrize("fmt", [O.E4M3, O.E5M2])
@pytest.mark.parametrize("gran", GRANS, ids=["mx", "dim1", "dim2"])
@pytest.mark.parametrize("prod", ["quantize", "norm_quantize", "swiglu_quantize", "dswiglu_quantize"])
def test_public_functions_are_the_unified_path(ops, data, prod, gran, fmt):
    x, h, dact, gamma, rstd = (data[k] for k in ("x", "h", "dact", "gamma", "rstd"))
    for rowwise, colwise in ORIENT:
        pub = _public(ops, prod, gran)
        if prod == "quantize":
            for cs in (False, True):
                got = pub(x, fmt, rowwise=rowwise, colwise=colwise, want_colsum=cs)
                assert len(got) == (5 if cs else 4)
                _same(got, ops._quantize(x, fmt, rowwise, colwise, None, cs, gran))
        elif prod == "norm_quantize":
            got = pub(x, rstd, gamma, fmt, rowwise=rowwise, colwise=colwise)
            _same(got, ops._norm_quantize(x, rstd, gamma, fmt, rowwise, colwise, gran))
        elif prod == "swiglu_quantize":
            got = pub(h, fmt, rowwise=rowwise, colwise=colwise)
            _same(got, ops._swiglu_quantize(h, fmt, rowwise, colwise, gran))
        else:
            for cs in (False, True):
                got = pub(h, dact, fmt, rowwise=rowwise, colwise=colwise, want_colsum=cs)
                assert len(got) == 5 and (got[4] is not None) == cs
                _same(got, ops._dswiglu_quantize(h, dact, fmt, rowwise, colwise, cs, gran))
        assert (got[0] is not None) == rowwise and (got[2] is not None) == colwise
        shape = (R, 2 * C) if prod == "dswiglu_quantize" else (R, C)
        if rowwise:
            assert got[0].shape == shape and got[1].shape == (shape[1] // 32, shape[0])
        if colwise:
            assert got[2].shape == shape[::-1] and got[3].shape == (shape[0] // 32, shape[1])


@pytest.mark.parametrize("fmt", [O.E4M3, O.E5M2])
def test_dim_and_epsilon_reach_the_kernel(ops, data, fmt):
    """The equality above would also hold if both sides dropped an argument: the three granularities, and EPS against 0, give
    different bytes on this input -- through the public functions, positional `dim` included."""
    x = data["x"]
    mx = ops.mxfp8_quantize(x, fmt)
    d1, d2 = ops.blockfp8_quantize(x, fmt, 1), ops.blockfp8_quantize(x, fmt, 2)
    d1e, d2e = ops.blockfp8_quantize(x, fmt, 1, amax_epsilon=EPS), ops.blockfp8_quantize(x, fmt, 2, amax_epsilon=EPS)
    _same(d1, ops._quantize(x, fmt, True, True, None, False, (1, 0.0)))
    _same(d2, ops._quantize(x, fmt, True, True, None, False, (2, 0.0)))
    outs = [mx, d1, d2, d1e, d2e]
    for i in range(len(outs)):
        for j in range(i + 1, len(outs)):
            assert not torch.equal(outs[i][1], outs[j][1]), (i, j)   # the row-wise scale bytes tell all five apart


@pytest.mark.parametrize("fmt", [O.E4M3, O.E5M2])
@pytest.mark.parametrize("dim", [1, 2])
@pytest.mark.parametrize("prod", ["quantize", "norm_quantize", "swiglu_quantize", "dswiglu_quantize"])
def test_amax_epsilon_on_an_all_zero_input(ops, dev, prod, dim, fmt):
    """amax 0 < epsilon: every block's scale is fp8_max / epsilon rounded down to a power of two 2^k, its byte 127 - k (with
    epsilon 0 the scale is 1 and the byte 127); the data bytes are zero."""
    z = lambda *s: torch.zeros(s, dtype=torch.bfloat16, device=dev)
    args = {"quantize": (z(R, C),), "norm_quantize": (z(R, C), torch.ones(R, device=dev), z(C) + 1),
            "swiglu_quantize": (z(R, 2 * C),), "dswiglu_quantize": (z(R, 2 * C), z(R, C))}[prod]
    fn = getattr(ops, "blockfp8_" + prod)
    byte = 127 - math.floor(math.log2(FMAX[fmt] / EPS))
    for eps, want in ((EPS, byte), (0.0, 127)):
        got = fn(*args, fmt, dim, amax_epsilon=eps)
        assert int(got[0].max()) == 0 and int(got[2].max()) == 0
        assert bool((got[1] == want).all()) and bool((got[3] == want).all()), (eps, want)


@pytest.mark.parametrize("fmt", [O.E4M3, O.E5M2])
@pytest.mark.parametrize("gran", GRANS, ids=["mx", "dim1", "dim2"])
def test_out_row_blocks_pass_through(ops, dev, gran, fmt):
    """Two parts of 128 rows quantised through `out=` views into one operand's buffers (128 x 128 blocks need parts that start on
    a block row): the public function against the implementation called directly, and both against the concatenation."""
    g = torch.Generator().manual_seed(7)
    parts = [(torch.randn(128, C, generator=g) * s).to(torch.bfloat16).to(dev) for s in (1.0, 1e-4)]
    pub = _public(ops, "quantize", gran)
    N = 256

    def fill(call):
        bufs = (torch.zeros((N, C), dtype=torch.uint8, device=dev), torch.zeros((C // 32, N), dtype=torch.uint8, device=dev),
                torch.zeros((C, N), dtype=torch.uint8, device=dev), torch.zeros((N // 32, C), dtype=torch.uint8, device=dev))
        sums = []
        for i, p in enumerate(parts):
            r = 128 * i
            views = (bufs[0][r:r + 128], bufs[1][:, r:r + 128], bufs[2][:, r:r + 128], bufs[3][r // 32:(r + 128) // 32])
            ret = call(p, views)
            assert len(ret) == 5 and all(a is b for a, b in zip(ret[:4], views))
            sums.append(ret[4])
        return bufs, sums

    got, got_cs = fill(lambda p, views: pub(p, fmt, out=views, want_colsum=True))
    want, want_cs = fill(lambda p, views: ops._quantize(p, fmt, True, True, views, True, gran))
    _same(got, want)
    _same(got_cs, want_cs)
    _same(got, pub(torch.cat(parts, 0), fmt))


# ------------------------------------------------------------------------------------------------------------ timer spans
def test_kernel_timer_spans(ops, data):
    """One call of each public function under an installed KernelTimer records one span: kind "mxfp8_quantize" /
    "blockfp8_quantize" (bench.py selects by kind), label "RxC" for the plain form and "<producer> RxC" for the fused ones, R x C
    elements, and as bytes the bf16 inputs read plus, per copy written, one FP8 byte and 1/32 scale byte per element."""
    from llm_fp8_amd.pytorch.profiler import KernelTimer
    x, h, dact, gamma, rstd = (data[k] for k in ("x", "h", "dact", "gamma", "rstd"))
    out_bytes = lambda r, c, copies: r * c * (1 + 1 / 32) * copies
    calls = [  # (family, call, label, elements, bytes)
        (fam, call, label, float(r * c), float(inp + out_bytes(r, c, copies)))
        for fam in ("mxfp8", "blockfp8")
        for call, label, r, c, inp, copies in (
            (lambda f: f("quantize")(x, O.E4M3), f"{R}x{C}", R, C, 2 * R * C, 2),
            (lambda f: f("norm_quantize")(x, rstd, gamma, O.E4M3, colwise=False), f"norm {R}x{C}", R, C, 2 * R * C, 1),
            (lambda f: f("swiglu_quantize")(h, O.E4M3), f"swiglu {R}x{C}", R, C, 2 * R * 2 * C, 2),   # reads h [R, 2C]
            (lambda f: f("dswiglu_quantize")(h, dact, O.E5M2, rowwise=False), f"dswiglu {R}x{2 * C}", R, 2 * C,
             2 * R * 2 * C + 2 * R * C, 1))]                                                            # reads h and dact [R, C]
    timer = KernelTimer()
    with timer.install():
        for fam, call, *_ in calls:
            call(lambda prod: getattr(ops, f"{fam}_{prod}"))
    torch.cuda.synchronize()
    assert KernelTimer.active is None and len(timer.spans) == len(calls) == 8
    for span, (fam, _, label, elems, nbytes) in zip(timer.spans, calls):
        assert span[:4] == (fam + "_quantize", label, elems, nbytes), (span[:4], fam, label)
        assert type(span[2]) is float and type(span[3]) is float


def test_rope_bwd_quantize_shares_the_helpers(ops, dev):
    """mxfp8_rope_bwd_quantize allocates and calls through the family's helpers too: its outputs are those of RoPE backward followed
    by mxfp8_quantize, and its span is kind "mxfp8_quantize", label "rope TxW", T x W elements, the bf16 d(qkv) read once plus the
    two copies written."""
    from llm_fp8_amd.pytorch.profiler import KernelTimer
    T, seq, n_q, n_kv, D = 64, 32, 2, 1, 128
    W = (n_q + 2 * n_kv) * D
    g = torch.Generator().manual_seed(5)
    dq, dk, dv = ((torch.randn(T, n * D, generator=g)).to(torch.bfloat16).to(dev) for n in (n_q, n_kv, n_kv))
    ang = torch.outer(torch.arange(seq, dtype=torch.float32), 1.0 / (10000.0 ** (torch.arange(0, D, 2, dtype=torch.float32) / D)))
    cos, sin = torch.cos(ang).contiguous().to(dev), torch.sin(ang).contiguous().to(dev)
    timer = KernelTimer(kinds=("mxfp8_quantize",))
    with timer.install():
        got = ops.mxfp8_rope_bwd_quantize(dq, dk, dv, cos, sin, n_q, n_kv, D, seq, O.E5M2)
    want = ops.mxfp8_quantize(ops.rope_qkv_backward(dq, dk, dv, cos, sin, n_q, n_kv, D, seq), O.E5M2)
    torch.cuda.synchronize()
    _same(got, want)
    assert [s[:4] for s in timer.spans] == [("mxfp8_quantize", f"rope {T}x{W}", float(T * W), float(2 * T * W + T * W * (1 + 1 / 32) * 2))]
