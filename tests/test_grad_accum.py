"""CPU: fp32 gradient accumulation (grad_accum_dtype fp32).  The numpy oracle (tests/grad_accum_oracle.py) accepts a float32
restatement of the kernel's three modes and rejects two restatements that are each wrong in one way; the entry point's host
refusals; flag / variable resolution; create_optimizer's refusals; the memory accounting."""
import numpy as np
import pytest
import torch

from tests import grad_accum_oracle as GO

N_MICRO = 4


def _window(seed=5, n=4096):
    """Four micro-batches of bf16 bits, exponents spread over 2^-20 .. 2^10 (most float32 adds round), with the special values."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(N_MICRO):
        v = (rng.normal(size=n) * np.exp2(rng.uniform(-20, 10, size=n))).astype(np.float32)
        out.append(GO.f32_to_bf16_rne(v))
    # 0x7F00 = 2^127 and 0x7EFF = 2^127 - 2^119: their float32 sum 2^128 - 2^119 is finite and is the tie between the largest bf16
    # and Inf, which goes to the even side: Inf
    inf, ninf, nan = 0x7F80, 0xFF80, 0x7FC0
    # the last column, 256 + 2^-17 - 256 + 2^-17, is 2^-17 in micro-batch order and 0 when summed pairwise
    for k, col in enumerate(((0x0000, 0x8000, 0x0000, 0x8000), (0x8000, 0x8000, 0x8000, 0x8000), (0x0001, 0x8001, 0x007F, 0x0001),
                             (inf, 0x3F80, 0x3F80, 0x3F80), (0x3F80, inf, 0x3F80, ninf), (nan, 0x3F80, 0, 0),
                             (0x7F00, 0x7EFF, 0, 0), (0x7EFF, 0, 0, 0x7F00), (0x4380, 0x3700, 0xC380, 0x3700))):
        for m in range(N_MICRO):
            out[m][k] = col[m]
    return out


def _kernel_restatement(grads):
    """mi_grad_accum_multi as the header states it: SET, ADD ..., FINISH, every element on its own, float32 throughout."""
    acc = np.empty(grads[0].shape, dtype=np.float32)
    with np.errstate(all="ignore"):
        for m, g in enumerate(grads):
            f = GO.bf16_to_f32(g)
            if m == 0:
                acc[:] = f                      # SET: acc is not read
            elif m < len(grads) - 1:
                acc[:] = acc + f                # ADD
            else:
                return GO.f32_to_bf16_rne(acc + f)  # FINISH: acc is not written


def _bf16_accumulation(grads):
    """Wrong in one way: the running sum is rounded to bf16 after every add (autograd's accumulation into a bf16 .grad)."""
    acc = grads[0].copy()
    with np.errstate(all="ignore"):
        for g in grads[1:]:
            acc = GO.f32_to_bf16_rne(GO.bf16_to_f32(acc) + GO.bf16_to_f32(g))
    return acc


def _pairwise_order(grads):
    """Wrong in one way: float32, but (g0 + g1) + (g2 + g3)."""
    f = [GO.bf16_to_f32(g) for g in grads]
    with np.errstate(all="ignore"):
        return GO.f32_to_bf16_rne((f[0] + f[1]) + (f[2] + f[3]))


def test_oracle_rounding_on_known_values():
    f = np.array([1.0, 1.00390625, 1.01171875, 3.3895313892515355e38, 3.4028234663852886e38, -0.0, 1e-45, np.inf], dtype=np.float32)
    #             exact  tie -> even (down)  tie -> even (up)   the largest bf16    rounds to Inf          -0    denormal -> 0
    assert GO.f32_to_bf16_rne(f).tolist() == [0x3F80, 0x3F80, 0x3F82, 0x7F7F, 0x7F80, 0x8000, 0x0000, 0x7F80]
    assert GO.is_nan_bf16(GO.f32_to_bf16_rne(np.array([np.nan], dtype=np.float32))).all()
    bits = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    assert GO.mismatches_bf16(GO.f32_to_bf16_rne(GO.bf16_to_f32(bits)), bits) == 0  # every bf16 value converts to itself


def test_oracle_accepts_the_float32_restatement():
    grads = _window()
    got = _kernel_restatement(grads)
    assert GO.mismatches(got, grads) == 0
    want = GO.window_total(grads)
    assert GO.is_nan_bf16(want[[4, 5]]).all() and want[3] == 0x7F80   # Inf meets -Inf; NaN; Inf stays
    assert want[6] == 0x7F80 and want[7] == 0x7F80                    # a finite float32 sum that rounds to Inf in bf16
    assert np.isfinite(GO.window_sum(grads)[[6, 7]]).all()
    assert want[0] == 0x0000 and want[1] == 0x8000                    # +0 + -0 = +0, a sum of -0 is -0


@pytest.mark.parametrize("wrong", [_bf16_accumulation, _pairwise_order])
def test_oracle_rejects_a_restatement_wrong_in_one_way(wrong):
    grads = _window()
    got, want = wrong(grads), GO.window_total(grads)
    assert (got != want).any()            # the inputs do tell the variant from the oracle ...
    assert GO.mismatches(got, grads) > 0  # ... and the oracle's comparison says so


def test_entry_point_reports_host_refusals():
    from llm_fp8_amd import _lib
    lib = _lib.load()
    fn = _lib.require("mi_grad_accum_multi", "the test")
    fake = 0x10000  # non-null; refused before anything is launched or dereferenced
    for args, what in (((None, 1, fake, 1, 65536, None), b"null"), ((fake, 1, None, 1, 65536, None), b"null"),
                       ((fake, 0, fake, 1, 65536, None), b"bad sizes"), ((fake, -3, fake, 1, 65536, None), b"bad sizes"),
                       ((fake, 1, fake, 1, 0, None), b"multiple of 8"), ((fake, 1, fake, 1, -8, None), b"multiple of 8"),
                       ((fake, 1, fake, 1, 65532, None), b"multiple of 8"), ((fake, 1, fake, -1, 65536, None), b"bad sizes")):
        rc = fn(*args)
        assert rc == -1 and what in lib.mi_last_error(), (args, lib.mi_last_error())
    assert b"mi_grad_accum_multi" in lib.mi_last_error()
    with pytest.raises(RuntimeError, match="mi_grad_accum_multi"):
        _lib.check(rc, "mi_grad_accum_multi")
    assert fn(fake, 1, fake, 0, 65536, None) == 0  # an empty chunk list: nothing to do
    assert _lib.revision() >= 7 and _lib.ABI_REVISION >= 7 and "mi_grad_accum_multi" in _lib.REVISION_SIGNATURES


def test_wrapper_refuses_cpu_tensors():
    from llm_fp8_amd.pytorch import ops
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.grad_accum_multi(torch.zeros((5, 1), dtype=torch.int64), 1, torch.zeros((1, 2), dtype=torch.int32), 1, 65536)


def test_flag_and_variable_resolution(monkeypatch):
    from llm_fp8_amd import train
    monkeypatch.delenv("LLM_FP8_AMD_GRAD_ACCUM", raising=False)
    assert train.TrainingConfig().grad_accum_dtype is None
    assert train.resolve_grad_accum_dtype(train.TrainingConfig()) == "bf16"
    assert train.resolve_grad_accum_dtype(None) == "bf16"
    assert train.resolve_grad_accum_dtype("fp32") == "fp32"
    monkeypatch.setenv("LLM_FP8_AMD_GRAD_ACCUM", "fp32")
    assert train.resolve_grad_accum_dtype(train.TrainingConfig()) == "fp32"
    assert train.resolve_grad_accum_dtype(train.TrainingConfig(grad_accum_dtype="bf16")) == "bf16"  # the flag wins
    for bad in ("fp16", "FP32", "float32"):
        with pytest.raises(ValueError, match="one of"):
            train.resolve_grad_accum_dtype(bad)
    monkeypatch.setenv("LLM_FP8_AMD_GRAD_ACCUM", "fp64")
    with pytest.raises(ValueError, match="fp64"):
        train.resolve_grad_accum_dtype(train.TrainingConfig())
    parse = lambda *argv: train.config_from_args(train.build_arg_parser().parse_args(list(argv)))
    assert parse().grad_accum_dtype is None
    assert parse("--grad_accum_dtype", "fp32").grad_accum_dtype == "fp32"
    assert parse("--grad_accum_dtype", "bf16").grad_accum_dtype == "bf16"
    with pytest.raises(SystemExit):
        parse("--grad_accum_dtype", "fp16")


class _Wrapper(torch.nn.Module):
    def __init__(self, module):
        super().__init__()
        self.module = module


@pytest.mark.parametrize("wrapper", ["GradArenaDP", "ShardedFP8DP", "FullyShardedDataParallel", "DistributedDataParallel"])
def test_create_optimizer_refuses_a_wrapped_model(monkeypatch, wrapper):
    from llm_fp8_amd import train
    monkeypatch.delenv("LLM_FP8_AMD_GRAD_ACCUM", raising=False)
    monkeypatch.delenv("LLM_FP8_AMD_TORCH_ADAMW", raising=False)
    model = type(wrapper, (_Wrapper,), {})(torch.nn.Linear(8, 8).to(torch.bfloat16))  # create_optimizer goes by the type's name
    with pytest.raises(RuntimeError, match=f"grad_accum_dtype='fp32'.*wrapped in {wrapper}"):
        train.create_optimizer(model, train.TrainingConfig(grad_accum_dtype="fp32"))


def test_create_optimizer_refuses_cpu_parameters_and_torch_adamw(monkeypatch):
    from llm_fp8_amd import train
    monkeypatch.delenv("LLM_FP8_AMD_GRAD_ACCUM", raising=False)
    monkeypatch.delenv("LLM_FP8_AMD_TORCH_ADAMW", raising=False)
    monkeypatch.delenv("LLM_FP8_AMD_OPT_STATE", raising=False)
    model = torch.nn.Linear(8, 8).to(torch.bfloat16)
    with pytest.raises(RuntimeError, match="grad_accum_dtype='fp32' needs ClippedAdamW.*not all on the GPU"):
        train.create_optimizer(model, train.TrainingConfig(grad_accum_dtype="fp32"))
    monkeypatch.setenv("LLM_FP8_AMD_GRAD_ACCUM", "fp32")  # the variable selects the mode as the flag does
    with pytest.raises(RuntimeError, match="grad_accum_dtype='fp32' needs ClippedAdamW"):
        train.create_optimizer(model, train.TrainingConfig())
    # the default mode builds torch's AdamW for the same model as it always did, and hangs nothing on it
    opt, _ = train.create_optimizer(model, train.TrainingConfig(grad_accum_dtype="bf16"))
    assert isinstance(opt, torch.optim.AdamW) and not hasattr(opt, "grad_accumulator")
    # LLM_FP8_AMD_TORCH_ADAMW=1: the message names every reason that applies
    monkeypatch.delenv("LLM_FP8_AMD_GRAD_ACCUM", raising=False)
    monkeypatch.setenv("LLM_FP8_AMD_TORCH_ADAMW", "1")
    with pytest.raises(RuntimeError, match="grad_accum_dtype='fp32' needs ClippedAdamW.*LLM_FP8_AMD_TORCH_ADAMW=1 selects torch's AdamW"):
        train.create_optimizer(model, train.TrainingConfig(grad_accum_dtype="fp32"))
    with pytest.raises(RuntimeError, match="not all on the GPU and LLM_FP8_AMD_TORCH_ADAMW=1 selects.* and the parameters are not all bf16"):
        train.create_optimizer(torch.nn.Linear(8, 8), train.TrainingConfig(grad_accum_dtype="fp32"))


def test_accumulator_layout_needs_no_gpu():
    """Offsets are 16-byte aligned and nothing is allocated before the first use."""
    from llm_fp8_amd.grad_accum import GradAccumulator
    ps = [torch.nn.Parameter(torch.zeros(n, dtype=torch.bfloat16)) for n in (3, 8, 1, 5)]
    frozen = torch.nn.Parameter(torch.zeros(7, dtype=torch.bfloat16), requires_grad=False)
    acc = GradAccumulator(ps + [frozen, ps[0]])
    assert [acc._offset[id(p)] for p in ps] == [0, 4, 12, 16] and acc.bytes() == 4 * 24
    assert not acc._buffers and not acc.has_content() and not any(hasattr(p, "main_grad") for p in ps)
    acc.accumulate(last=False)  # no parameter has a gradient: nothing to do, nothing launched
    acc.accumulate(last=True)
    assert not acc._buffers


def test_replicated_state_bytes_counts_four_bytes_per_trainable_parameter():
    from llm_fp8_amd import distributed as D
    m = torch.nn.Sequential(torch.nn.Linear(16, 32), torch.nn.Linear(32, 8)).to(torch.bfloat16)
    m[1].bias.requires_grad_(False)
    trainable = sum(p.numel() for p in m.parameters() if p.requires_grad)
    assert trainable == 16 * 32 + 32 + 32 * 8
    for state in ("bf16", "fp32", "bf16_sr"):
        base = D.replicated_state_bytes(m, optimizer_state=state)
        assert D.replicated_state_bytes(m, optimizer_state=state, fp32_grad_accum=False) == base
        assert D.replicated_state_bytes(m, optimizer_state=state, fp32_grad_accum=True) == base + 4 * trainable
    assert D.fits_replicated(m, torch.device("cpu"), fp32_grad_accum=True)


def test_resolve_sharding_mode_passes_the_accumulation_mode(monkeypatch):
    from llm_fp8_amd import distributed as D, train
    import torch.distributed as dist
    seen = {}

    def fits(model, device, fraction=0.5, optimizer_state="bf16", fp32_grad_accum=False):
        seen["accum"] = fp32_grad_accum
        return True

    monkeypatch.delenv("LLM_FP8_AMD_GRAD_ACCUM", raising=False)
    monkeypatch.setattr(D, "fits_replicated", fits)
    monkeypatch.setattr(dist, "get_world_size", lambda *a, **k: 2)
    m = torch.nn.Linear(8, 8)
    assert train.resolve_sharding_mode("auto", m, torch.device("cpu"), None, "fp32") == "replicated" and seen["accum"] is True
    assert train.resolve_sharding_mode("auto", m, torch.device("cpu")) == "replicated" and seen["accum"] is False
