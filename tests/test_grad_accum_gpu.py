"""GPU: fp32 gradient accumulation.  `mi_grad_accum_multi` against the numpy oracle (tests/grad_accum_oracle.py) bit for bit, with
every device buffer inside a sentinel-filled allocation; `GradAccumulator` and train.train_step on a tiny model (the shape of
tests/test_resume_gpu.py: 2 layers, hidden 512, 4 heads of 128, 2 KV heads, FFN 1024, vocab 512, batch 2 x 128) against the
oracle of the micro-batch gradients, against autograd's bf16 accumulation, through a dropped step, and with a single batch."""
import contextlib

import numpy as np
import pytest
import torch

from tests import grad_accum_oracle as GO
from tests.util import bf16_bits

pytestmark = pytest.mark.gpu

CHUNK = 65536
PAD = 64                                   # sentinel elements on either side of a buffer
SENT = {2: 0x5A5A, 4: 0x5A5A5A5A}          # by element size
ADD, SET, FINISH = 0, 1, 2
INF, NINF, NAN = 0x7F80, 0xFF80, 0x7FC0
# per micro-batch (five of them), one planted element each: +-0; -0 throughout; bf16 subnormals; Inf stays; Inf meets -Inf in a
# later micro-batch; NaN; two values near the bf16 maximum (2^127 and 2^127 - 2^119) whose float32 sum is finite and rounds to Inf
# in bf16, in the first two and in the last two micro-batches; 256 + 2^-17 - 256 + 2^-17, which depends on the order of the adds
PLANTED = ((0x0000, 0x8000, 0x0000, 0x8000, 0x0000), (0x8000,) * 5, (0x0001, 0x8001, 0x007F, 0x0001, 0x8002),
           (INF, 0x3F80, 0x3F80, 0xBF80, 0x3F80), (0x3F80, INF, 0x3F80, NINF, 0x3F80), (0x3F80, 0x3F80, NAN, 0x3F80, 0x3F80),
           (0x7F00, 0x7EFF, 0, 0, 0), (0, 0, 0, 0x7EFF, 0x7F00), (0x4380, 0x3700, 0xC380, 0x3700, 0))


class Guarded:
    """A device buffer of n elements inside a sentinel-filled allocation; `shift` elements move it off the 16-byte grid."""

    def __init__(self, n, elem_size, dev, shift=0):
        self.itype = {2: torch.int16, 4: torch.int32}[elem_size]
        self.utype = {2: np.uint16, 4: np.uint32}[elem_size]
        self.sent = SENT[elem_size]
        self.lo, self.n = PAD + shift, n
        self.raw = torch.full((PAD + shift + n + PAD,), self.sent, dtype=self.itype, device=dev)
        assert self.raw.data_ptr() % 16 == 0
        self.ptr = self.raw.data_ptr() + self.lo * elem_size

    def write(self, values):
        v = np.ascontiguousarray(values)
        assert v.size == self.n and v.dtype.itemsize == self.raw.element_size()
        signed = {np.uint16: np.int16, np.uint32: np.int32}[self.utype]
        self.raw[self.lo:self.lo + self.n].copy_(torch.from_numpy(v.view(signed)))

    def snapshot(self):
        return self.raw.cpu().numpy().view(self.utype).copy()

    @staticmethod
    def split(snap, g):
        """(left sentinels, contents, right sentinels) of a snapshot."""
        return snap[:g.lo], snap[g.lo:g.lo + g.n], snap[g.lo + g.n:]

    def contents(self):
        return self.split(self.snapshot(), self)[1]

    def assert_sentinels(self, what):
        left, _, right = self.split(self.snapshot(), self)
        assert (left == self.sent).all() and (right == self.sent).all(), f"{what}: written outside the buffer"


def _random_bf16(rng, n):
    """bf16 bits with exponents spread over 2^-20 .. 2^10: most float32 adds of two of them round."""
    return GO.f32_to_bf16_rne((rng.normal(size=n) * np.exp2(rng.uniform(-20, 10, size=n))).astype(np.float32))


def _micro_batches(rng, n, n_micro=5):
    gs = [_random_bf16(rng, n) for _ in range(n_micro)]
    k = len(PLANTED)
    for base in ([0, n - k] if n >= 2 * k else []):  # at the head (vector path) and at the very end (the tail)
        for j, col in enumerate(PLANTED):
            for m in range(n_micro):
                gs[m][base + j] = col[m]
    return gs


def _launch(dev, tensors, modes):
    """One launch over `tensors` = [(g Guarded or None, acc Guarded, out Guarded or None)] with the per-tensor `modes`."""
    from llm_fp8_amd import grad_accum
    from llm_fp8_amd.pytorch import ops
    sizes = tuple(acc.n for _, acc, _ in tensors)
    rows = [[0 if g is None else g.ptr for g, _, _ in tensors], [acc.ptr for _, acc, _ in tensors], list(sizes), list(modes),
            [0 if out is None else out.ptr for _, _, out in tensors]]
    table = torch.tensor(rows, dtype=torch.int64, device=dev)
    refs = grad_accum.chunk_refs(sizes)
    chunks = torch.tensor(refs, dtype=torch.int32, device=dev).reshape(-1, 2)
    ops.grad_accum_multi(table, len(tensors), chunks, len(refs), CHUNK)
    torch.cuda.synchronize()


def test_kernel_matches_the_oracle_after_each_of_five_launches(dev):
    rng = np.random.default_rng(20)
    sizes = [1, 7, 8, 9, 2047, 2048, 2049, 4095, 4096, 4097, 65535, 65536, 65537, 2 * 65536 + 13]
    # (n, shift of g in bf16 elements, shift of acc in fp32 elements, separate out): g at an odd 2-byte offset; acc 4-byte but not
    # 16-byte aligned; out != g
    specs = [(n, 0, 0, False) for n in sizes] + [(4097 + 24, 1, 0, False), (2049 + 24, 0, 1, False), (65537 + 24, 0, 0, True)]
    tensors, grads = [], []
    for n, gshift, ashift, separate in specs:
        g, acc = Guarded(n, 2, dev, gshift), Guarded(n, 4, dev, ashift)
        out = Guarded(n, 2, dev) if separate else g
        assert g.ptr % 16 == 2 * gshift and acc.ptr % 16 == 4 * ashift
        acc.write(np.full(n, 0x7FC00000, dtype=np.uint32))  # NaN: a SET that read acc would show
        tensors.append((g, acc, out))
        grads.append(_micro_batches(rng, n))
    assert any(GO.is_nan_bf16(GO.window_total(gs)).any() for gs in grads)
    modes = [SET, ADD, ADD, ADD, FINISH]
    for m, mode in enumerate(modes):
        for (g, _, _), gs in zip(tensors, grads):
            g.write(gs[m])
        before = [(g.snapshot(), acc.snapshot(), out.snapshot()) for g, acc, out in tensors]
        _launch(dev, tensors, [mode] * len(tensors))
        for t, ((g, acc, out), gs) in enumerate(zip(tensors, grads)):
            what = f"launch {m} (mode {mode}), tensor {t} of {acc.n} elements"
            for buf in {id(b): b for b in (g, acc, out)}.values():
                buf.assert_sentinels(what)
            if mode != FINISH:
                assert np.array_equal(g.snapshot(), before[t][0]), f"{what}: g was written"
                bad = GO.mismatches_f32(acc.contents().view(np.float32), GO.window_sum(gs[:m + 1]))
                assert bad == 0, f"{what}: {bad} elements of acc are not the oracle's"
            else:
                assert np.array_equal(acc.snapshot(), before[t][1]), f"{what}: acc was written"
                if out is not g:
                    assert np.array_equal(g.snapshot(), before[t][0]), f"{what}: g was written though out is elsewhere"
                bad = GO.mismatches(out.contents(), gs)
                assert bad == 0, f"{what}: {bad} elements of out are not the oracle's"


def test_kernel_mixes_modes_in_one_launch(dev):
    rng = np.random.default_rng(21)
    n_set, n_add, n_fin, n_fin0, n_bad = 4097, 65537, 2049, 9 + CHUNK, 777
    mk = lambda n: (Guarded(n, 2, dev), Guarded(n, 4, dev))
    (g_set, a_set), (g_add, a_add), (g_fin, a_fin), (g_bad, a_bad) = mk(n_set), mk(n_add), mk(n_fin), mk(n_bad)
    a_fin0, o_fin0 = Guarded(n_fin0, 4, dev), Guarded(n_fin0, 2, dev)
    bits = {k: _random_bf16(rng, n) for k, n in (("set", n_set), ("add", n_add), ("fin", n_fin), ("bad", n_bad))}
    sums = {k: GO.window_sum(_micro_batches(rng, n, 3)) for k, n in (("add", n_add), ("fin", n_fin), ("fin0", n_fin0), ("bad", n_bad))}
    for g, k in ((g_set, "set"), (g_add, "add"), (g_fin, "fin"), (g_bad, "bad")):
        g.write(bits[k])
    a_set.write(np.full(n_set, 0x7FC00000, dtype=np.uint32))
    for a, k in ((a_add, "add"), (a_fin, "fin"), (a_fin0, "fin0"), (a_bad, "bad")):
        a.write(sums[k])
    tensors = [(g_set, a_set, None), (g_add, a_add, None), (g_fin, a_fin, g_fin), (None, a_fin0, o_fin0), (g_bad, a_bad, g_bad)]
    everything = [g_set, a_set, g_add, a_add, g_fin, a_fin, a_fin0, o_fin0, g_bad, a_bad]
    before = {id(b): b.snapshot() for b in everything}
    _launch(dev, tensors, [SET, ADD, FINISH, FINISH, 7])  # 7: no mode, the tensor is left alone
    for b in everything:
        b.assert_sentinels("mixed launch")
    for b in (g_set, g_add, a_fin, a_fin0, g_bad, a_bad):  # must not be written
        assert np.array_equal(b.snapshot(), before[id(b)])
    with np.errstate(all="ignore"):
        assert GO.mismatches_f32(a_set.contents().view(np.float32), GO.bf16_to_f32(bits["set"])) == 0
        assert GO.mismatches_f32(a_add.contents().view(np.float32), sums["add"] + GO.bf16_to_f32(bits["add"])) == 0
        assert GO.mismatches_bf16(g_fin.contents(), GO.f32_to_bf16_rne(sums["fin"] + GO.bf16_to_f32(bits["fin"]))) == 0
        assert GO.mismatches_bf16(o_fin0.contents(), GO.f32_to_bf16_rne(sums["fin0"])) == 0


# ---- the tiny model

SEED = 31
N_MICRO = 4
TINY = dict(hidden_size=512, intermediate_size=1024, num_attention_heads=4, num_key_value_heads=2, head_dim=128)
SWITCHES = ("LLM_FP8_AMD_NO_OPT_WCAST", "LLM_FP8_AMD_OPT_STATE", "LLM_FP8_AMD_TORCH_ADAMW", "LLM_FP8_AMD_NO_STEP_GUARD",
            "LLM_FP8_AMD_GRAD_ACCUM", "LLM_FP8_AMD_DENSE_EMBEDDING_GRAD")


@contextlib.contextmanager
def _env(tie=True):
    """The tiny shapes behind the config table, none of the A/B switches, a clean FP8 state before and after."""
    from llm_fp8_amd import llama
    from llm_fp8_amd.pytorch.fp8 import FP8GlobalStateManager as G
    mp = pytest.MonkeyPatch()
    lc = llama.llama_config
    mp.setattr(llama, "llama_config", lambda name, **kw: lc(name, **{**TINY, "tie_word_embeddings": tie, **kw}))
    for v in SWITCHES:
        mp.delenv(v, raising=False)
    G.reset()
    try:
        yield mp
    finally:
        mp.undo()
        G.reset()


def _build(device, mode, scenario="current"):
    from llm_fp8_amd import train
    from llm_fp8_amd.optim import ClippedAdamW
    cfg = train.TrainingConfig(model_name="llama-3.2-3b", batch_size=2, max_seq_length=128, mixed_precision="fp8", fp8_scenario=scenario,
                               use_te=True, sharding_mode="none", num_hidden_layers=2, vocab_size=512, learning_rate=1e-3,
                               num_warmup_steps=0, gradient_accumulation_steps=N_MICRO, grad_accum_dtype=mode)
    torch.manual_seed(SEED)
    model = train.wrap_distributed(train.prepare_model(train.create_model(cfg, device), cfg), cfg, device)
    model.train()
    opt, sched = train.create_optimizer(model, cfg)
    assert isinstance(opt, ClippedAdamW) and (getattr(opt, "grad_accumulator", None) is not None) == (mode == "fp32")
    return model, opt, sched, cfg


def _batches(cfg, device, windows=1):
    from llm_fp8_amd import train
    gen = torch.Generator(device=device).manual_seed(12)
    return [[train.synthetic_batch(cfg, 512, device, gen) for _ in range(N_MICRO)] for _ in range(windows)]


def _backward(model, mb, i, n):
    """One micro-batch as train.train_step runs it."""
    from llm_fp8_amd import train
    train._set_first_microbatch(model, i == 0)
    (model(**mb).loss / n).backward()
    if i == n - 1:
        train._set_first_microbatch(model, None)


def _grad_bits(model):
    return {name: None if p.grad is None else bf16_bits(p.grad).reshape(-1) for name, p in model.named_parameters()}


def _fp32_window(model, acc, batches):
    """A window driven by hand: (clones of every micro-batch's gradients, the totals left in .grad), as bf16 bits by name."""
    n, clones = len(batches), []
    for i, mb in enumerate(batches):
        _backward(model, mb, i, n)
        clones.append(_grad_bits(model))  # .grad was None before this backward: this IS the micro-batch's gradient
        assert all(c is not None for c in clones[-1].values())
        acc.accumulate(last=i == n - 1)
        if i < n - 1:
            assert acc.has_content()
            for name, p in model.named_parameters():
                buf = acc._buffers[p.device]
                assert p.grad is None, name
                assert p.main_grad.dtype == torch.float32 and p.main_grad.shape == p.shape and p.main_grad.data_ptr() % 16 == 0
                assert p.main_grad.untyped_storage().data_ptr() == buf.untyped_storage().data_ptr(), name
            if i == n - 2:  # the fp32 sums themselves, once
                for name, p in model.named_parameters():
                    want = GO.window_sum([c[name] for c in clones])
                    assert GO.mismatches_f32(p.main_grad.detach().cpu().numpy().reshape(-1), want) == 0, name
    assert not acc.has_content()
    return clones, _grad_bits(model)


def _assert_totals_are_the_oracle(clones, totals):
    for name, got in totals.items():
        bad = GO.mismatches(got, [c[name] for c in clones])
        assert bad == 0, f"{name}: {bad} of {got.size} elements are not the oracle's"


@pytest.fixture(scope="module")
def tied_run(dev):
    """Two windows on one accumulator, tied embedding, scenario `current` (no scaling state depends on history): per window
    (clones, totals).  Shared, and left unchanged, by the tests below."""
    with _env():
        model, opt, _, cfg = _build(dev, "fp32")
        acc = opt.grad_accumulator
        assert acc.bytes() >= 4 * sum(p.numel() for p in model.parameters()) and not acc._buffers  # nothing allocated before the first use
        out = []
        for batches in _batches(cfg, dev, windows=2):
            out.append(_fp32_window(model, acc, batches))
            opt.zero_grad()
        assert sum(b.numel() * 4 for b in acc._buffers.values()) == acc.bytes()
        return out


def test_accumulator_totals_match_the_oracle_tied(tied_run):
    (clones, totals), _ = tied_run
    _assert_totals_are_the_oracle(clones, totals)


def test_second_window_on_the_same_accumulator(tied_run):
    (_, first), (clones, totals) = tied_run
    _assert_totals_are_the_oracle(clones, totals)
    assert any((first[k] != totals[k]).any() for k in totals)  # other batches: nothing of the first window is what is compared


def test_accumulator_totals_match_the_oracle_untied(dev):
    with _env(tie=False):
        model, opt, _, cfg = _build(dev, "fp32")
        assert model.get_output_embeddings().weight is not model.get_input_embeddings().weight
        clones, totals = _fp32_window(model, opt.grad_accumulator, _batches(cfg, dev)[0])
        _assert_totals_are_the_oracle(clones, totals)


def test_parameter_without_a_gradient_in_the_last_micro_batch(dev):
    from llm_fp8_amd.grad_accum import GradAccumulator
    rng = np.random.default_rng(3)
    n = 2 * CHUNK + 13
    ps = {k: torch.nn.Parameter(torch.zeros(n, dtype=torch.bfloat16, device=dev)) for k in ("first_only", "first_two", "last_only", "never")}
    # which micro-batches give which parameter a gradient
    plan = {"first_only": (1, 0, 0), "first_two": (1, 1, 0), "last_only": (0, 0, 1), "never": (0, 0, 0)}
    acc = GradAccumulator(ps.values())
    given = {k: [] for k in ps}
    for m in range(3):
        for k, p in ps.items():
            g = _random_bf16(rng, n) if plan[k][m] else None
            given[k].append(g)
            p.grad = None if g is None else torch.from_numpy(g.view(np.int16)).view(torch.bfloat16).to(dev)
        last_obj = ps["last_only"].grad
        acc.accumulate(last=m == 2)
    assert not acc.has_content()
    for k in ("first_only", "first_two"):  # FINISH with no gradient: a new .grad = RNE(acc)
        assert ps[k].grad is not None and ps[k].grad.dtype == torch.bfloat16 and ps[k].grad.shape == ps[k].shape
        assert GO.mismatches(bf16_bits(ps[k].grad), given[k]) == 0, k
    assert ps["last_only"].grad is last_obj and np.array_equal(bf16_bits(last_obj), given["last_only"][2])  # left alone
    assert ps["never"].grad is None


def test_fp32_mode_is_closer_to_the_exact_sum_than_autograd_accumulation(dev, tied_run):
    (clones, totals_fp32), _ = tied_run
    with _env():
        model, opt, _, cfg = _build(dev, "bf16")
        batches = _batches(cfg, dev)[0]
        # the same inputs: this model's micro-batch gradients, each taken from a clean .grad, are the other run's
        for i, mb in enumerate(batches):
            opt.zero_grad(set_to_none=True)
            _backward(model, mb, i, N_MICRO)
            for name, g in _grad_bits(model).items():
                assert np.array_equal(g, clones[i][name]), f"micro-batch {i}, {name}: the two runs' gradients differ"
        # today's path: autograd adds every micro-batch into the bf16 .grad
        opt.zero_grad(set_to_none=True)
        for i, mb in enumerate(batches):
            _backward(model, mb, i, N_MICRO)
        totals_bf16 = _grad_bits(model)
    err = {"fp32": 0.0, "bf16": 0.0}
    differ = 0
    for name in totals_fp32:
        exact = sum(GO.bf16_to_f32(c[name]).astype(np.float64) for c in clones)
        for mode, t in (("fp32", totals_fp32), ("bf16", totals_bf16)):
            err[mode] += float(np.abs(GO.bf16_to_f32(t[name]).astype(np.float64) - exact).sum())
        differ += int((totals_fp32[name] != totals_bf16[name]).sum())
    print(f"sum |total - exact|: fp32 mode {err['fp32']:.6e}, bf16 mode {err['bf16']:.6e}; {differ} elements differ")
    assert np.isfinite(err["fp32"]) and np.isfinite(err["bf16"])
    assert differ > 0          # the modes are not the same path
    assert err["fp32"] < err["bf16"]


def test_step_guard_drops_a_poisoned_window_and_the_next_is_clean(dev):
    from llm_fp8_amd import train
    with _env():
        model, opt, sched, cfg = _build(dev, "fp32")
        acc = opt.grad_accumulator
        first, second = _batches(cfg, dev, windows=2)
        weights = {n: p.detach().clone() for n, p in model.named_parameters()}
        inner, calls = acc.accumulate, []

        def poisoned(last):
            calls.append(last)
            if len(calls) == 2:  # a non-final micro-batch
                next(p for p in model.parameters() if p.grad is not None).grad.view(-1)[5] = float("inf")
            return inner(last)

        acc.accumulate = poisoned
        train.train_step(model, first, opt, sched, cfg)
        acc.accumulate = inner
        assert calls == [False, False, False, True]
        assert bool(opt.last_step_skipped.item()) and int(opt.skipped_steps.item()) == 1
        for n, p in model.named_parameters():
            assert torch.equal(p.detach().view(torch.int16), weights[n].view(torch.int16)), f"{n} changed in a dropped step"
        assert not acc.has_content() and all(p.grad is None for p in model.parameters())
        clones, totals = _fp32_window(model, acc, second)
        _assert_totals_are_the_oracle(clones, totals)
        for name, t in totals.items():
            assert np.isfinite(GO.bf16_to_f32(t)).all(), name


def _count_launches(mp):
    from llm_fp8_amd.pytorch import ops
    inner, calls = ops.grad_accum_multi, []

    def counted(*args, **kwargs):
        calls.append(args[1])
        return inner(*args, **kwargs)

    mp.setattr(ops, "grad_accum_multi", counted)
    return calls


def test_single_batch_never_touches_the_accumulator(dev):
    from llm_fp8_amd import train
    with _env() as mp:
        model, opt, sched, cfg = _build(dev, "fp32")
        calls = _count_launches(mp)
        produced, seen = {}, {}
        for name, p in model.named_parameters():
            p.register_post_accumulate_grad_hook(lambda q, name=name: produced.__setitem__(name, q.grad.data_ptr()))
        step = opt.step

        def spying_step(*args, **kwargs):
            seen.update({name: p.grad.data_ptr() for name, p in model.named_parameters() if p.grad is not None})
            return step(*args, **kwargs)

        opt.step = spying_step
        loss = train.train_step(model, _batches(cfg, dev)[0][0], opt, sched, cfg)
        assert torch.isfinite(loss).item()
        assert calls == [] and not opt.grad_accumulator._buffers and not opt.grad_accumulator.has_content()
        assert produced and seen == produced  # the optimiser stepped the very tensors autograd produced
        assert not any(hasattr(p, "main_grad") for p in model.parameters())


@pytest.mark.parametrize("scenario", ["default", "mxfp8"])
def test_train_step_with_four_micro_batches(dev, scenario):
    from llm_fp8_amd import train
    with _env() as mp:
        model, opt, sched, cfg = _build(dev, "fp32", scenario)
        calls = _count_launches(mp)
        initial = {n: p.detach().clone() for n, p in model.named_parameters()}
        n_params = sum(1 for _ in model.parameters())
        for batches in _batches(cfg, dev, windows=2):
            loss = train.train_step(model, batches, opt, sched, cfg)
            assert torch.isfinite(loss).item()
            assert not opt.grad_accumulator.has_content()  # after train_step's optimizer.zero_grad()
        assert calls == [n_params] * (2 * N_MICRO)         # ONE launch per micro-batch, over every parameter
        assert not bool(opt.last_step_skipped.item())
        # every weight moved, except the RMSNorm gammas: they start at 1.0, where half a bf16 ulp (2^-9 downwards) is more than
        # one AdamW step at lr = 1e-3; the bf16 weight rounds back to 1.0 after each step, so the steps do not add up
        moved = {n for n, p in model.named_parameters() if not torch.equal(p.detach(), initial[n])}
        gammas = {n for n, p in initial.items() if p.dim() == 1 and bool((p == 1).all())}
        assert moved | gammas == set(initial) and len(gammas) == 5 and n_params == 22
        # zero_grad abandons a window that was begun
        _backward(model, batches[0], 0, N_MICRO)
        opt.grad_accumulator.accumulate(last=False)
        assert opt.grad_accumulator.has_content()
        opt.zero_grad()
        assert not opt.grad_accumulator.has_content()
