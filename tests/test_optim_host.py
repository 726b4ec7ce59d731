"""CPU: the host side of optim.ClippedAdamW's fused update as far as no GPU is needed -- the refusals of the six `_multi` entry
points of csrc/mi_optim.hip (return code and the full text of mi_last_error()), the rules by which a weight gets or loses its FP8
sink (`_sink_of` / `_mx_sink_of`), and the two pure functions behind `_plan`: the chunk lists and the device table, against
literals written out from the table description in include/mi_fp8.h.  tests/test_optim_paths_gpu.py ties the same layout to
real tensors on the device."""
import types

import pytest
import torch

FAKE = 0x10000  # non-null, 16-byte aligned; every call below is refused (or has nothing to do) before anything is dereferenced
ADAM = (1e-3, 0.9, 0.999, 1e-8, 1e-2)
CHUNK = 65536
MI_OK, MI_ERR_ARG = 0, -1
BF16_CALLS = ("mi_adamw_bf16_multi", "mi_adamw_cast_bf16_multi", "mi_adamw_mxcast_bf16_multi")
KIND_CALLS = ("mi_adamw_f32_multi", "mi_adamw_sr_bf16_multi")  # these take sink_kind and accept n_chunks == 0


# ------------------------------------------------------------------------------------------------ refusals
def _call(lib, name, table=FAKE, n_tensors=1, chunks=FAKE, n_chunks=4, chunk_elems=CHUNK, partial=FAKE, step=1, sink_kind=0):
    head = (table, n_tensors, chunks, n_chunks, chunk_elems)
    if name == "mi_sumsq_bf16_multi":
        return lib.mi_sumsq_bf16_multi(*head, partial, None)
    tail = {"mi_adamw_f32_multi": (sink_kind,), "mi_adamw_sr_bf16_multi": (sink_kind, 7)}.get(name, ())
    return getattr(lib, name)(*head, None, *ADAM, step, *tail, None)


def _refused(lib, name, text, **kw):
    assert _call(lib, name, **kw) == MI_ERR_ARG, (name, kw)
    assert lib.mi_last_error() == f"{name}: {text}".encode(), (name, kw, lib.mi_last_error())


def test_sumsq_multi_refusals():
    from llm_fp8_amd import _lib
    lib, name = _lib.load(), "mi_sumsq_bf16_multi"
    for kw in (dict(table=None), dict(chunks=None), dict(partial=None)):
        _refused(lib, name, "null pointer", **kw)
    for kw in (dict(n_tensors=0), dict(n_chunks=0), dict(chunk_elems=0), dict(chunk_elems=4), dict(chunk_elems=12)):
        _refused(lib, name, "bad sizes", **kw)


@pytest.mark.parametrize("name", BF16_CALLS)
def test_bf16_multi_refusals(name):
    """One message for every size defect, and n_chunks == 0 is one of them."""
    from llm_fp8_amd import _lib
    lib = _lib.load()
    for kw in (dict(table=None), dict(chunks=None)):
        _refused(lib, name, "null pointer", **kw)
    for kw in (dict(n_tensors=0), dict(n_chunks=0), dict(chunk_elems=0), dict(chunk_elems=4), dict(chunk_elems=12), dict(step=0)):
        _refused(lib, name, "bad sizes", **kw)


@pytest.mark.parametrize("name", KIND_CALLS)
def test_f32_and_sr_multi_refusals_and_the_empty_chunk_list(name):
    from llm_fp8_amd import _lib
    lib = _lib.load()
    for kw in (dict(table=None), dict(chunks=None)):
        _refused(lib, name, "null pointer", **kw)
    for kw in (dict(n_tensors=0), dict(step=0)):
        _refused(lib, name, "bad sizes", **kw)
    for ce in (0, 4, 12):
        _refused(lib, name, "chunk_elems must be a positive multiple of 8", chunk_elems=ce)
    for kind in (-1, 2):
        _refused(lib, name, "sink_kind must be 0 (per-tensor FP8) or 1 (MXFP8)", sink_kind=kind)
    for kind in (0, 1):
        assert _call(lib, name, n_chunks=0, sink_kind=kind) == MI_OK  # nothing to do: returns before the launch
    # the checks run in this order: pointers, sizes, chunk_elems, sink_kind -- and all of them before the n_chunks == 0 return
    _refused(lib, name, "bad sizes", n_tensors=0, chunk_elems=12, sink_kind=2)
    _refused(lib, name, "chunk_elems must be a positive multiple of 8", chunk_elems=12, sink_kind=2, n_chunks=0)
    _refused(lib, name, "sink_kind must be 0 (per-tensor FP8) or 1 (MXFP8)", sink_kind=2, n_chunks=0)


# ------------------------------------------------------------------------------------------------ sink lookup
def _opt(**kw):
    from llm_fp8_amd.optim import ClippedAdamW
    return ClippedAdamW([torch.nn.Parameter(torch.zeros(8, dtype=torch.bfloat16))], **kw)


def _weight(rows=64, cols=96):
    p = torch.nn.Parameter(torch.zeros(rows, cols, dtype=torch.bfloat16))
    assert p.data_ptr() % 16 == 0
    return p


def _operand(N=224, K=96):  # as far as the lookup reads a sink: the [N, K] FP8 copy's shape
    return types.SimpleNamespace(w8=types.SimpleNamespace(shape=(N, K)))


def _at_2_bytes(shape, dtype=torch.bfloat16):
    n = shape[0] * shape[1]
    t = torch.zeros(n + 8, dtype=dtype)[1:1 + n].view(shape)
    assert t.data_ptr() % 16 != 0
    return t


def _announce(p, sink, r0, n):
    p._mi_fp8_sink = (sink, r0, n)
    p._mi_mx_sink = (sink, r0, n)
    return p


def test_a_weight_with_a_sink_resolves_to_sink_row_offset_and_rows():
    opt, sink = _opt(), _operand()
    p = _announce(_weight(), sink, 32, 64)
    assert opt._sink_of(p) == (sink, 32, 64) and opt._mx_sink_of(p) == (sink, 32, 64)
    assert opt._sink_of(_weight()) is None and opt._mx_sink_of(_weight()) is None  # nothing announced
    q = _weight()
    q._mi_fp8_sink = (sink, 0, 64)  # the two kinds are announced under different names
    assert opt._sink_of(q) == (sink, 0, 64) and opt._mx_sink_of(q) is None


def test_every_way_a_weight_falls_back_to_the_flat_path(monkeypatch):
    monkeypatch.delenv("LLM_FP8_AMD_NO_OPT_WCAST", raising=False)
    opt, sink = _opt(), _operand()
    both = lambda p: (opt._sink_of(p), opt._mx_sink_of(p))
    flat1d = torch.nn.Parameter(torch.zeros(64 * 96, dtype=torch.bfloat16))
    assert both(_announce(flat1d, sink, 0, 64 * 96)) == (None, None)                                   # not 2-D
    strided = torch.nn.Parameter(torch.zeros(96, 64, dtype=torch.bfloat16).t())
    assert strided.shape == (64, 96) and not strided.is_contiguous()
    assert both(_announce(strided, sink, 0, 64)) == (None, None)                                       # not contiguous
    assert both(_announce(_weight(60, 96), sink, 0, 60)) == (None, None)                               # rows off 8 (and 32)
    assert both(_announce(_weight(64, 100), _operand(224, 100), 0, 64)) == (None, None)                # cols off 8 (and 32)
    s48 = _announce(_weight(48, 96), sink, 0, 48)                                                      # units: 8 per tensor, 32 MXFP8
    assert both(s48) == ((sink, 0, 48), None)
    k40 = _operand(224, 40)
    assert both(_announce(_weight(64, 40), k40, 0, 64)) == ((k40, 0, 64), None)
    # the row offset: MXFP8 needs a multiple of 32, the per-tensor path does not look at it
    assert both(_announce(_weight(), sink, 8, 64)) == ((sink, 8, 64), None)
    assert both(_announce(_weight(), sink, 3, 64)) == ((sink, 3, 64), None)
    assert both(_announce(_weight(), sink, 0, 32)) == (None, None)                                     # n is not the weight's rows
    assert both(_announce(_weight(), _operand(224, 128), 0, 64)) == (None, None)                       # K is not the weight's cols
    good = _announce(_weight(), sink, 32, 64)
    assert both(good) == ((sink, 32, 64),) * 2
    monkeypatch.setenv("LLM_FP8_AMD_NO_OPT_WCAST", "1")
    assert both(good) == (None, None)
    monkeypatch.setenv("LLM_FP8_AMD_NO_OPT_WCAST", "0")
    assert both(good) == ((sink, 32, 64),) * 2


def test_a_misaligned_gradient_moment_or_master_keeps_the_weight_off_the_tile_path():
    sink = _operand()
    for name in ("grad", "exp_avg", "exp_avg_sq"):
        opt, p = _opt(), _announce(_weight(), sink, 0, 64)
        p.grad = torch.zeros_like(p)
        opt.state[p] = {"exp_avg": torch.zeros_like(p), "exp_avg_sq": torch.zeros_like(p)}
        assert opt._sink_of(p) == (sink, 0, 64) and opt._mx_sink_of(p) == (sink, 0, 64)
        if name == "grad":
            p.grad = _at_2_bytes(p.shape)
        else:
            opt.state[p][name] = _at_2_bytes(p.shape)
        assert opt._sink_of(p) is None and opt._mx_sink_of(p) is None, name
    # the master counts with fp32 state only
    for f32 in (False, True):
        opt = _opt(state_dtype=torch.float32) if f32 else _opt()
        p = _announce(_weight(), sink, 0, 64)
        opt.state[p] = {"master": _at_2_bytes(p.shape, torch.float32)}
        assert (opt._sink_of(p) is None) == f32 and (opt._mx_sink_of(p) is None) == f32


def test_a_row_shard_resolves_through_the_full_weight():
    opt, sink = _opt(), _operand()
    full = _announce(_weight(128, 96), sink, 64, 128)
    shard = _weight(32, 96)
    shard._mi_shard_of = (full, 32, 32)
    assert opt._sink_of(shard) == (sink, 96, 32) and opt._mx_sink_of(shard) == (sink, 96, 32)
    shard._mi_shard_of = (full, 16, 32)  # row 80 of the operand: fine per tensor, no multiple of 32 for MXFP8
    assert opt._sink_of(shard) == (sink, 80, 32) and opt._mx_sink_of(shard) is None
    shard._mi_shard_of = (_weight(128, 96), 32, 32)  # the full weight has no sink
    _announce(shard, sink, 0, 32)                    # what the shard itself says does not count
    assert opt._sink_of(shard) is None and opt._mx_sink_of(shard) is None


# ------------------------------------------------------------------------------------------------ chunk lists and the table
class _Buf:
    """What the table builder asks of a tensor: an address and a shape."""

    def __init__(self, ptr, shape=()):
        self._ptr, self.shape = ptr, shape

    def data_ptr(self):
        return self._ptr


def _fp8_sink(N, K):
    from llm_fp8_amd.pytorch.module import WeightSink
    s = WeightSink.__new__(WeightSink)
    s.w8, s.w8t, s.scale, s.amax = _Buf(0x100000, (N, K)), _Buf(0x200000, (K, N)), _Buf(0x300040), _Buf(0x300080)
    return s


def _mx_sink(N, K):
    from llm_fp8_amd.pytorch.module import MXWeightSink
    s = MXWeightSink.__new__(MXWeightSink)
    s.w8, s.sc = _Buf(0x400000, (N, K)), _Buf(0x500000, (K // 32, N))
    s.wt8, s.sct = _Buf(0x600000, (K, N)), _Buf(0x700000, (N // 32, K))
    return s


def test_the_sinks_say_what_they_are():
    from llm_fp8_amd.pytorch.module import MXWeightSink, WeightSink
    assert (WeightSink.attr, WeightSink.unit, WeightSink.kind) == ("_mi_fp8_sink", 8, 0)
    assert (MXWeightSink.attr, MXWeightSink.unit, MXWeightSink.kind) == ("_mi_mx_sink", 32, 1)
    # rows 6..11 of a part that starts at row r0 of the operand (include/mi_fp8.h)
    assert _fp8_sink(400, 144).table_rows(200, 144) == (0x100000 + 200 * 144, 0x200000 + 200, 144, 400, 0x300040, 0x300080)
    assert _mx_sink(224, 96).table_rows(32, 96) == (0x400000 + 32 * 96, 0x500000 + 32, 0x600000 + 32, 0x700000 + 1 * 96, 224, 0)


def test_chunk_lists():
    from llm_fp8_amd import optim
    fp8, mx = _fp8_sink(200, 144), _mx_sink(224, 96)
    # a flat tensor of CHUNK + 11 elements: two flat chunks on both lists
    assert optim.chunk_refs([CHUNK + 11], [(CHUNK + 11,)], [None]) == ([(0, 0), (0, 1)], [(0, 0), (0, 1)])
    assert optim.chunk_refs([CHUNK], [(CHUNK,)], [None]) == ([(0, 0)], [(0, 0)])
    # 200 x 144 with a per-tensor sink: one flat chunk, 2 x 2 tiles of 128 x 128
    assert optim.chunk_refs([200 * 144], [(200, 144)], [(fp8, 0, 200)]) == ([(0, 0)], [(0, 0), (0, 1), (0, 2), (0, 3)])
    # 160 x 96 with an MXFP8 sink: 2 x 1 tiles
    assert optim.chunk_refs([160 * 96], [(160, 96)], [(mx, 32, 160)]) == ([(0, 0)], [(0, 0), (0, 1)])
    # together, in the tensors' order; a sink-less tensor keeps its flat chunks inside the cast list
    flat, cast = optim.chunk_refs([CHUNK + 11, 200 * 144, 7, 384 * 256], [(CHUNK + 11,), (200, 144), (7,), (384, 256)],
                                  [None, (fp8, 0, 200), None, None])
    assert flat == [(0, 0), (0, 1), (1, 0), (2, 0), (3, 0), (3, 1)]
    assert cast == [(0, 0), (0, 1), (1, 0), (1, 1), (1, 2), (1, 3), (2, 0), (3, 0), (3, 1)]


# three tensors: 0 flat, 1 a sink weight, 2 flat; addresses (p, g, exp_avg, exp_avg_sq, master)
ADDRS = [(0x1000, 0x2000, 0x3000, 0x4000, 0x5000), (0x11000, 0x12000, 0x13000, 0x14000, 0x15000),
         (0x21002, 0x22000, 0x23000, 0x24000, 0x25000)]
HEAD = [[0x1000, 0x11000, 0x21002], [0x2000, 0x12000, 0x22000], [0x3000, 0x13000, 0x23000], [0x4000, 0x14000, 0x24000]]


def test_table_rows_per_tensor_sink(monkeypatch):
    from llm_fp8_amd import optim
    monkeypatch.delenv("MI_DEBUG_SINK", raising=False)
    sink = _fp8_sink(200, 144)
    sizes, shapes, sinks = [CHUNK + 11, 200 * 144, 7], [(CHUNK + 11,), (200, 144), (7,)], [None, (sink, 0, 200), None]
    want = HEAD + [[CHUNK + 11, 28800, 7],            # 4 numel
                   [0, 144, 0],                       # 5 cols: 0 = flat
                   [0, 0x100000, 0],                  # 6 y
                   [0, 0x200000, 0],                  # 7 yT
                   [0, 144, 0],                       # 8 ld_y
                   [0, 200, 0],                       # 9 ld_yT
                   [0, 0x300040, 0],                  # 10 scale
                   [0, 0x300080, 0]]                  # 11 amax
    assert optim.table_rows(ADDRS, sizes, shapes, sinks, "bf16") == want
    # fp32 state: 13 rows, row 12 the master
    assert optim.table_rows(ADDRS, sizes, shapes, sinks, "fp32") == want + [[0x5000, 0x15000, 0x25000]]
    # stochastic rounding: 14 rows, row 12 the element base, row 13 the tensor key
    keys = [(5, 3), (6, 4096), (7, 0)]
    assert optim.table_rows(ADDRS, sizes, shapes, sinks, "bf16_sr", keys) == want + [[3, 4096, 0], [5, 6, 7]]
    with pytest.raises(ValueError, match="element base 4100 of a weight with an FP8 sink must be a multiple of 8"):
        optim.table_rows(ADDRS, sizes, shapes, sinks, "bf16_sr", [(5, 3), (6, 4100), (7, 0)])
    # a part further down the operand: rows 200 .. 399 of a [400, 144] operand
    low = _fp8_sink(400, 144)
    got = optim.table_rows(ADDRS, sizes, shapes, [None, (low, 200, 200), None], "bf16")
    assert [r[1] for r in got[5:]] == [144, 0x100000 + 200 * 144, 0x200000 + 200, 144, 400, 0x300040, 0x300080]
    # MI_DEBUG_SINK (tools/bench_adamw.py) masks the outputs of this kind off: noT row 7, none rows 6 and 7
    for mode, masked in (("full", ()), ("noT", (7,)), ("none", (6, 7))):
        monkeypatch.setenv("MI_DEBUG_SINK", mode)
        exp = [[0] * 3 if i in masked else r for i, r in enumerate(want)]
        assert optim.table_rows(ADDRS, sizes, shapes, sinks, "bf16") == exp, mode


def test_table_rows_mxfp8_sink(monkeypatch):
    from llm_fp8_amd import optim
    monkeypatch.delenv("MI_DEBUG_SINK", raising=False)
    sink = _mx_sink(224, 96)  # the weight is rows 32 .. 191 of a [224, 96] operand
    sizes, shapes, sinks = [CHUNK + 11, 160 * 96, 7], [(CHUNK + 11,), (160, 96), (7,)], [None, (sink, 32, 160), None]
    want = HEAD + [[CHUNK + 11, 15360, 7],            # 4 numel
                   [0, 96, 0],                        # 5 cols
                   [0, 0x400000 + 32 * 96, 0],        # 6 y_row
                   [0, 0x500000 + 32, 0],             # 7 s_row
                   [0, 0x600000 + 32, 0],             # 8 y_colT
                   [0, 0x700000 + 1 * 96, 0],         # 9 s_colT: block row 32 / 32 = 1
                   [0, 224, 0],                       # 10 ldr
                   [0, 0, 0]]                         # 11 unused
    assert optim.table_rows(ADDRS, sizes, shapes, sinks, "bf16") == want
    assert optim.table_rows(ADDRS, sizes, shapes, sinks, "fp32") == want + [[0x5000, 0x15000, 0x25000]]
    assert optim.table_rows(ADDRS, sizes, shapes, sinks, "bf16_sr", [(1, 0), (1, 8), (2, 5)]) == want + [[0, 8, 5], [1, 1, 2]]
    for mode in ("noT", "none"):  # the masking is the per-tensor kind's alone
        monkeypatch.setenv("MI_DEBUG_SINK", mode)
        assert optim.table_rows(ADDRS, sizes, shapes, sinks, "bf16") == want, mode


def test_row_constants_are_the_headers_numbers():
    from llm_fp8_amd import optim
    assert [optim.ROW_P, optim.ROW_G, optim.ROW_EXP_AVG, optim.ROW_EXP_AVG_SQ, optim.ROW_NUMEL, optim.ROW_COLS] == [0, 1, 2, 3, 4, 5]
    assert (optim.ROW_SINK, optim.ROW_Y, optim.ROW_YT) == (6, 6, 7)
    assert (optim.ROW_MASTER, optim.ROW_SR_BASE, optim.ROW_SR_KEY) == (12, 12, 13)
