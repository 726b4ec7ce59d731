"""GPU: the paths of optim.ClippedAdamW.step() pinned from outside, for the three state modes (bf16, fp32, bf16 with stochastic
rounding) and every partition content (no sink; per-tensor sink + flat; MXFP8 sink + flat; both sinks + flat).  1: which entry
points of csrc/mi_optim.hip a step calls, in which order and with which counts; 2: the device table and both chunk lists of every
plan, against a table this file builds from the tensors' addresses and the layout in include/mi_fp8.h (the literals of
tests/test_optim_host.py on real objects); 3: the bits a step leaves are those of ONE direct call of the entry point on a
hand-built table over clones, with every output of that call inside a 0xA5-filled allocation.

Shapes: a 200 x 144 weight under DelayedScaling (128 x 128 tiles ragged both ways), a 160 x 96 weight under MXFP8BlockScaling, a
flat tensor of 8*256*3 + 5 elements (vector body + element tail) and the same at a 2-byte offset (element-wise walk)."""
import pytest
import torch

from tests.test_optim_fp32_state_gpu import CHUNK, G0, _delayed, _sink_linear

pytestmark = pytest.mark.gpu
BF16, F32 = torch.bfloat16, torch.float32
N_FLAT = 8 * 256 * 3 + 5
SEED = 0x123456789ABCDEF0
MODES = {"bf16": {}, "fp32": dict(state_dtype=F32), "bf16_sr": dict(stochastic_rounding=True, sr_seed=SEED)}
CONTENTS = {"none": ("flat", "off"), "fp8": ("tiled", "flat", "off"), "mx": ("mxw", "flat", "off"), "both": ("mxw", "tiled", "flat", "off")}
MARGIN = 64


@pytest.fixture()
def te_reset(dev):
    from llm_fp8_amd.pytorch.fp8 import FP8GlobalStateManager
    FP8GlobalStateManager.reset()
    yield
    FP8GlobalStateManager.reset()


def _mx():
    from llm_fp8_amd.common.recipe import MXFP8BlockScaling
    return MXFP8BlockScaling()


def _tensor(dev, name, gen):
    """One named parameter with a gradient."""
    if name == "tiled":
        return _sink_linear(dev, 144, 144, 200, _delayed()).weight
    if name == "mxw":
        return _sink_linear(dev, 96, 96, 160, _mx()).weight
    data = torch.randn(N_FLAT, generator=gen).to(BF16).to(dev)
    if name == "off":
        buf = torch.zeros(N_FLAT + 8, dtype=BF16, device=dev)
        p = torch.nn.Parameter(buf[1:1 + N_FLAT])
        with torch.no_grad():
            p.copy_(data)
        assert p.data_ptr() % 16 == 2
    else:
        p = torch.nn.Parameter(data)
        assert p.data_ptr() % 16 == 0
    p.grad = torch.randn(N_FLAT, generator=gen).to(BF16).to(dev)
    return p


def _opt(params, mode, mgn):
    from llm_fp8_amd.optim import ClippedAdamW
    return ClippedAdamW(params, max_grad_norm=mgn, **MODES[mode], **G0)


class _Spy:
    """The library with its optimiser entry points recorded: (name, arguments) in call order."""

    def __init__(self, lib, log):
        self._lib, self._log = lib, log

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith(("mi_adamw", "mi_sumsq")):
            return fn

        def call(*args):
            self._log.append((name, args))
            return fn(*args)
        return call


def _spied_step(opt, monkeypatch):
    from llm_fp8_amd import _lib
    log = []
    spy = _Spy(_lib.load(), log)
    with monkeypatch.context() as m:
        m.setattr(_lib, "load", lambda: spy)
        m.setattr(_lib, "require", lambda name, why: getattr(spy, name))
        opt.step()
    torch.cuda.synchronize()
    return log


# ------------------------------------------------------------------------------------------------ the header's table
def _sink_rows(p, mx):
    """Rows 5..11 of one tensor as include/mi_fp8.h lays them out, from what the module announced on the weight."""
    ann = getattr(p, "_mi_mx_sink" if mx else "_mi_fp8_sink", None)
    if ann is None:
        return None
    sink, r0, n = ann
    assert n == p.shape[0]
    K, N = p.shape[1], sink.w8.shape[0]
    if mx:   # 6 y_row  7 s_row  8 y_colT  9 s_colT  10 ldr  11 unused
        return [K, sink.w8.data_ptr() + r0 * K, sink.sc.data_ptr() + r0, sink.wt8.data_ptr() + r0, sink.sct.data_ptr() + (r0 // 32) * K, N, 0]
    return [K, sink.w8.data_ptr() + r0 * K, sink.w8t.data_ptr() + r0, K, N, sink.scale.data_ptr(), sink.amax.data_ptr()]  # y yT ld_y ld_yT scale amax


def _header_table(cols, mode):
    """[rows, T] from per-tensor columns dict(p, g, m, v, numel, sink (rows 5..11 or None), master, base, key)."""
    rows = [[c["p"] for c in cols], [c["g"] for c in cols], [c["m"] for c in cols], [c["v"] for c in cols], [c["numel"] for c in cols]]
    rows += [[(c["sink"] or [0] * 7)[i] for c in cols] for i in range(7)]
    if mode == "fp32":
        rows.append([c["master"] for c in cols])
    if mode == "bf16_sr":
        rows += [[c["base"] for c in cols], [c["key"] for c in cols]]
    return rows


# what the chunk lists of a plan must be, by the plan's tensors and kind: (flat list, cast list).  6149 flat elements are one
# chunk; 200 x 144 is one flat chunk or 2 x 2 tiles; 160 x 96 one flat chunk or 2 x 1 tiles; a tensor without a sink OF THE PLAN'S
# KIND keeps its flat chunks on the cast list
CHUNKS = {
    (("flat", "off"), False): ([[0, 0], [1, 0]], [[0, 0], [1, 0]]),
    (("tiled", "flat", "off"), False): ([[0, 0], [1, 0], [2, 0]], [[0, 0], [0, 1], [0, 2], [0, 3], [1, 0], [2, 0]]),
    (("mxw", "flat", "off"), False): ([[0, 0], [1, 0], [2, 0]], [[0, 0], [1, 0], [2, 0]]),
    (("mxw",), True): ([[0, 0]], [[0, 0], [0, 1]]),
    (("mxw", "tiled", "flat", "off"), False): ([[0, 0], [1, 0], [2, 0], [3, 0]], [[0, 0], [1, 0], [1, 1], [1, 2], [1, 3], [2, 0], [3, 0]]),
}
# the plans a step leaves per partition content: the whole partition (squared norm; also the update where no weight has an MXFP8
# sink), then the MXFP8 part and the rest
PLANS = {"none": [(("flat", "off"), False)], "fp8": [(("tiled", "flat", "off"), False)],
         "mx": [(("mxw", "flat", "off"), False), (("mxw",), True), (("flat", "off"), False)],
         "both": [(("mxw", "tiled", "flat", "off"), False), (("mxw",), True), (("tiled", "flat", "off"), False)]}
# the update launches: (tensors, flat chunks, cast chunks, kind); the MXFP8 launch first
UPDATES = {"none": [(2, 2, 2, 0)], "fp8": [(3, 3, 6, 0)], "mx": [(1, 1, 2, 1), (2, 2, 2, 0)], "both": [(1, 1, 2, 1), (3, 3, 6, 0)]}


# ------------------------------------------------------------------------------------------------ 1 + 2: launches and tables
@pytest.mark.parametrize("content", list(CONTENTS))
@pytest.mark.parametrize("mode", list(MODES))
def test_step_launches_and_device_tables(te_reset, dev, monkeypatch, mode, content):
    monkeypatch.delenv("LLM_FP8_AMD_NO_OPT_WCAST", raising=False)
    monkeypatch.delenv("MI_DEBUG_SINK", raising=False)
    gen = torch.Generator().manual_seed(5)
    names = CONTENTS[content]
    params = {n: _tensor(dev, n, gen) for n in names}
    for i, p in enumerate(params.values()):
        p._mi_sr_key = (40 + i, 8 * i)
    opt = _opt(list(params.values()), mode, 1.0)
    for step in (1, 2):  # the second step goes through the plan cache
        log = _spied_step(opt, monkeypatch)
        # ---- 1: one squared norm over the partition, then the update(s)
        want = [("mi_sumsq_bf16_multi", len(names), len(names), None)]
        for T, n_flat, n_cast, kind in UPDATES[content]:
            has_sink = n_cast != n_flat
            if mode == "fp32":
                want.append(("mi_adamw_f32_multi", T, n_cast, (kind,)))
            elif mode == "bf16_sr":
                want.append(("mi_adamw_sr_bf16_multi", T, n_cast, (kind, SEED)))
            elif has_sink:
                want.append(("mi_adamw_mxcast_bf16_multi" if kind else "mi_adamw_cast_bf16_multi", T, n_cast, ()))
            else:
                want.append(("mi_adamw_bf16_multi", T, n_flat, ()))
        got = []
        for name, a in log:
            assert a[4] == CHUNK, (name, a)
            if name == "mi_sumsq_bf16_multi":
                got.append((name, a[1], a[3], None))
            else:
                assert a[11] == step and a[5] is not None, (name, a)  # the partition's step; the clip coefficient's address
                assert tuple(a[6:11]) == (G0["lr"], *G0["betas"], G0["eps"], G0["weight_decay"]), (name, a)
                got.append((name, a[1], a[3], tuple(a[12:-1])))
        assert got == want, (mode, content, step)
        # ---- 2: every plan's table and chunk lists
        by_id = {id(p): n for n, p in params.items()}
        plans = {(tuple(by_id[i] for i in key[1]), key[2]): plan for key, plan in opt._plans.items()}
        assert sorted(plans) == sorted(PLANS[content])
        for (pnames, mx), plan in plans.items():
            assert plan["mx"] is mx
            cols = []
            for n in pnames:
                p, st = params[n], opt.state[params[n]]
                cols.append(dict(p=p.data_ptr(), g=p.grad.data_ptr(), m=st["exp_avg"].data_ptr(), v=st["exp_avg_sq"].data_ptr(),
                                 numel=p.numel(), sink=_sink_rows(p, mx), master=st["master"].data_ptr() if mode == "fp32" else None,
                                 key=p._mi_sr_key[0], base=p._mi_sr_key[1]))
            assert plan["table"].cpu().tolist() == _header_table(cols, mode), (mode, content, pnames, mx)
            assert [s is not None for s in plan["sinks"]] == [c["sink"] is not None for c in cols]
            flat, cast = CHUNKS[(pnames, mx)]
            assert plan["chunks"].cpu().tolist() == flat and plan["n_chunks"] == len(flat)
            if mode == "bf16" and cast == flat:
                assert plan["chunks_cast"] is None
            else:
                assert plan["chunks_cast"].cpu().tolist() == cast and plan["n_chunks_cast"] == len(cast)
    if content != "none":
        for p in params.values():
            for attr in ("_mi_fp8_sink", "_mi_mx_sink"):
                if hasattr(p, attr):
                    assert getattr(p, attr)[0].fresh()


# ------------------------------------------------------------------------------------------------ 3: bits
def _guarded(src, off=0):
    """A copy of `src` in the middle of an allocation filled with 0xA5 bytes: MARGIN (+ `off`) elements before it, MARGIN after."""
    n = src.numel()
    buf = torch.empty(n + 2 * MARGIN + off, dtype=src.dtype, device=src.device)
    buf.view(torch.uint8).fill_(0xA5)
    t = buf[MARGIN + off:MARGIN + off + n].view(src.shape)
    t.copy_(src.detach())
    return t, buf


def _margins_intact(t, buf, what):
    raw = buf.view(torch.uint8)
    lo = t.data_ptr() - buf.data_ptr()
    hi = lo + t.numel() * t.element_size()
    assert bool((raw[:lo] == 0xA5).all()), f"{what}: wrote before the tensor"
    assert bool((raw[hi:] == 0xA5).all()), f"{what}: wrote past the tensor"


@pytest.mark.parametrize("kind", ["none", "fp8", "mx"])
@pytest.mark.parametrize("mode", list(MODES))
def test_a_step_leaves_the_bits_of_one_direct_call(te_reset, dev, monkeypatch, mode, kind):
    from llm_fp8_amd import _lib
    monkeypatch.delenv("LLM_FP8_AMD_NO_OPT_WCAST", raising=False)
    monkeypatch.delenv("MI_DEBUG_SINK", raising=False)
    lib = _lib.load()
    gen = torch.Generator().manual_seed(6)
    names = {"none": ("flat", "off"), "fp8": ("tiled", "flat", "off"), "mx": ("mxw",)}[kind]
    params = [_tensor(dev, n, gen) for n in names]
    sdt = F32 if mode == "fp32" else BF16
    opt = _opt(params, mode, None)
    held = []  # (what, tensor the step writes, the clone the direct call writes, the clone's allocation)
    cols = []
    for i, (n, p) in enumerate(zip(names, params)):
        p._mi_sr_key = (40 + i, 8 * i)
        off = 1 if n == "off" else 0
        # the step's own state, inside guarded allocations too
        m, mbuf = _guarded((1e-2 * torch.randn(p.shape, generator=gen)).to(sdt).to(dev))
        v, vbuf = _guarded((1e-4 * torch.rand(p.shape, generator=gen)).to(sdt).to(dev))
        opt.state[p] = {"step": 2, "exp_avg": m, "exp_avg_sq": v}
        outs = [("p", p, None), ("exp_avg", m, mbuf), ("exp_avg_sq", v, vbuf)]
        if mode == "fp32":
            w, wbuf = _guarded(p.detach().float() * (1.0 + 2.0 ** -12))
            opt.state[p].update(master=w, master_version=p._version)
            outs.append(("master", w, wbuf))
        col = dict(g=p.grad.data_ptr(), numel=p.numel(), key=40 + i, base=8 * i, sink=None, master=None)
        for what, t, tbuf in outs:
            c, cbuf = _guarded(t, off if what == "p" else 0)
            col[{"p": "p", "exp_avg": "m", "exp_avg_sq": "v", "master": "master"}[what]] = c.data_ptr()
            held.append((f"{n} {what}", t, tbuf, c, cbuf))
        ann = getattr(p, "_mi_mx_sink" if kind == "mx" else "_mi_fp8_sink", None)
        assert (ann is not None) == (n in ("tiled", "mxw"))
        if ann is not None:
            sink, r0, _ = ann
            assert r0 == 0
            K, N = p.shape[1], sink.w8.shape[0]
            fields = ("w8", "sc", "wt8", "sct") if kind == "mx" else ("w8", "w8t", "amax")
            cl = {}
            for f in fields:
                cl[f], cbuf = _guarded(getattr(sink, f))
                held.append((f"{n} sink {f}", getattr(sink, f), None, cl[f], cbuf))
            ptr = {f: c.data_ptr() for f, c in cl.items()}
            col["sink"] = ([K, ptr["w8"], ptr["sc"], ptr["wt8"], ptr["sct"], N, 0] if kind == "mx" else
                           [K, ptr["w8"], ptr["w8t"], K, N, sink.scale.data_ptr(), ptr["amax"]])
        cols.append(col)
    assert (opt._sink_of(params[0]) is not None) == (kind == "fp8") and (opt._mx_sink_of(params[0]) is not None) == (kind == "mx")
    # ---- one direct call on the clones
    table = torch.tensor(_header_table(cols, mode), dtype=torch.int64).to(dev)
    refs = {"none": [[0, 0], [1, 0]], "fp8": CHUNKS[(("tiled", "flat", "off"), False)][1], "mx": CHUNKS[(("mxw",), True)][1]}[kind]
    chunks = torch.tensor(refs, dtype=torch.int32).to(dev)
    st = torch.cuda.current_stream().cuda_stream
    k = 1 if kind == "mx" else 0
    name, tail = {"fp32": ("mi_adamw_f32_multi", (k,)), "bf16_sr": ("mi_adamw_sr_bf16_multi", (k, SEED)),
                  "bf16": ({"none": "mi_adamw_bf16_multi", "fp8": "mi_adamw_cast_bf16_multi", "mx": "mi_adamw_mxcast_bf16_multi"}[kind], ())}[mode]
    rc = getattr(lib, name)(table.data_ptr(), len(cols), chunks.data_ptr(), len(refs), CHUNK, None, G0["lr"], *G0["betas"], G0["eps"],
                            G0["weight_decay"], 3, *tail, st)
    _lib.check(rc, name)
    # ---- the step on the originals
    before = [p.detach().clone() for p in params]
    log = _spied_step(opt, monkeypatch)
    assert [c[0] for c in log] == [name]  # max_grad_norm=None: no squared norm; one launch, of the entry point called above
    for p, b in zip(params, before):
        assert opt.state[p]["step"] == 3 and not torch.equal(p.detach(), b)
    for what, t, tbuf, c, cbuf in held:
        assert t.dtype == c.dtype and torch.equal(t.detach().view(torch.uint8), c.view(torch.uint8)), f"{mode} {kind} {what}: the step's bits differ"
        _margins_intact(c, cbuf, f"{what} (direct call)")
        if tbuf is not None:
            _margins_intact(t, tbuf, f"{what} (step)")
