"""CPU: stochastic rounding of the bf16 optimiser state (optim.ClippedAdamW(stochastic_rounding=True), mi_adamw_sr_bf16_multi) as
far as no GPU is needed -- the C ABI (header, library and binding agree; host refusals), the generator's known answers, the
`bf16_sr` mode through flag, config and environment, the keys a row shard gets, and the numpy model of the feature inside the
bounds the GPU tests use (tests/test_optim_sr_gpu.py tests 4 and 5), so that those bounds hold under the reference algorithm alone."""
import copy
import os
import re

import numpy as np
import pytest
import torch

from tests import sr_twin as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x10000  # non-null, 16-byte aligned; every call below is refused (or has nothing to do) before anything is dereferenced
ADAM = (1e-3, 0.9, 0.999, 1e-8, 1e-2)
NAME = "mi_adamw_sr_bf16_multi"


def test_header_library_and_binding_agree_on_revision_4_and_the_signature():
    from llm_fp8_amd import _lib
    src = open(os.path.join(ROOT, "include", "mi_fp8.h")).read()
    lib = _lib.load()
    rev = int(re.search(r"#define\s+MI_ABI_REVISION\s+(\d+)", src).group(1))
    assert int(re.search(r"#define\s+MI_ABI_VERSION\s+(\d+)", src).group(1)) == lib.mi_abi_version() == _lib.ABI_VERSION == 5
    assert rev == lib.mi_abi_revision() == _lib.ABI_REVISION >= 4
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert hasattr(lib, NAME), f"libmi_fp8.so does not export {NAME}"
    assert NAME in _lib.SIGNATURES and NAME in _lib.REVISION_SIGNATURES
    assert getattr(lib, NAME).argtypes == _lib.SIGNATURES[NAME]
    decl = re.search(r"int\s+%s\s*\((.*?)\)\s*;" % NAME, code, flags=re.S).group(1)
    args = [" ".join(a.split()) for a in decl.split(",")]
    assert len(args) == len(_lib.SIGNATURES[NAME]) == 15
    assert args[:6] == ["const int64_t* table", "int n_tensors", "const int32_t* chunks", "int n_chunks", "int chunk_elems",
                        "const float* grad_scale"]
    assert [a.split()[0] for a in args[6:11]] == ["float"] * 5
    assert args[11:] == ["int64_t step", "int sink_kind", "uint64_t seed", "void* stream"]
    import ctypes
    assert _lib.SIGNATURES[NAME][11:] == [ctypes.c_int64, ctypes.c_int, ctypes.c_uint64, ctypes.c_void_p]
    # mi_adamw_f32_multi's list + the seed
    assert _lib.SIGNATURES[NAME][:13] + _lib.SIGNATURES[NAME][14:] == _lib.SIGNATURES["mi_adamw_f32_multi"]


def test_host_refusals_before_any_launch():
    from llm_fp8_amd import _lib
    lib = _lib.load()
    call = lambda table=FAKE, n_tensors=1, chunks=FAKE, n_chunks=4, chunk_elems=65536, step=1, sink_kind=0, seed=7: getattr(lib, NAME)(
        table, n_tensors, chunks, n_chunks, chunk_elems, None, *ADAM, step, sink_kind, seed, None)
    for kw in (dict(table=None), dict(chunks=None), dict(n_tensors=0), dict(n_tensors=-3), dict(chunk_elems=0), dict(chunk_elems=-8),
               dict(chunk_elems=12), dict(chunk_elems=65537), dict(sink_kind=-1), dict(sink_kind=2), dict(step=0), dict(step=-5)):
        assert call(**kw) == -1, kw                                   # MI_ERR_ARG
        assert NAME.encode() in lib.mi_last_error(), kw
    for sink_kind in (0, 1):
        assert call(n_chunks=0, sink_kind=sink_kind, seed=2 ** 64 - 1) == 0   # nothing to do: MI_OK, nothing launched
    with pytest.raises(RuntimeError, match="sink_kind"):
        _lib.check(call(sink_kind=7), NAME)


def test_philox4x32_10_known_answers():
    ones = 0xFFFFFFFF
    for ctr, key, want in (((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
                           ((ones,) * 4, (ones, ones), "408f276d 41c83b0e a20bc7c6 6d5451fd"),
                           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
                            "d16cfe09 94fdcceb 5001e420 24126ea1")):
        assert " ".join("%08x" % int(w[0]) for w in S.philox4x32_10(*ctr, *key)) == want


def test_the_bits_of_an_element_and_the_rounding_rule():
    # element j of a vector: bits [16 (j & 1), + 16) of word j >> 1 of the call with counter (v, 0, step, key << 2 | stream)
    seed, step, key = (0x299f31d0 << 32) | 0xa4093822, 0x13198a2e, 0x03707344 >> 2
    w = S.philox4x32_10(0x243f6a88, 0, step, (key << 2) | 1, seed & 0xFFFFFFFF, seed >> 32)
    e = (0x243f6a88 << 3) + np.arange(8)
    want = [(int(w[j >> 1][0]) >> (16 * (j & 1))) & 0xFFFF for j in range(8)]
    assert S.sr_bits16(seed, step, key, 1, e).tolist() == want
    assert S.sr_bits16(seed, step + 2 ** 32, key, 1, e).tolist() == want                 # step mod 2^32
    assert S.sr_bits16(seed, step, key, 1, e[::-1]).tolist() == want[::-1]               # a function of the element alone
    # a bf16 value never moves; the fraction decides; NaN / Inf take the round-to-nearest conversion; the top may become Inf
    x = np.array([1.0, -1.0, 0.0, 3.0e38], np.float32)
    assert S.sr_bf16_bits(x, 0xFFFF).tolist() == S.rne_bf16_bits(x).tolist()[:3] + [0x7F62]
    half = np.array([0x3F7F8000, 0xBF7F8000], np.uint32).view(np.float32)
    assert S.sr_bf16_bits(half, 0x7FFF).tolist() == [0x3F7F, 0xBF7F] and S.sr_bf16_bits(half, 0x8000).tolist() == [0x3F80, 0xBF80]
    big = np.array([0x7F7F0001], np.uint32).view(np.float32)
    assert S.sr_bf16_bits(big, 0xFFFF).tolist() == [0x7F80] and S.sr_bf16_bits(big, 0).tolist() == [0x7F7F]
    odd = np.array([np.inf, -np.inf, np.nan], np.float32)
    assert S.sr_bf16_bits(odd, 0xFFFF).tolist()[:2] == [0x7F80, 0xFF80] and (S.sr_bf16_bits(odd, 0xFFFF)[2] & 0x7FFF) > 0x7F80


def _params(n=2, dtype=torch.bfloat16):
    g = torch.Generator().manual_seed(3)
    return [torch.nn.Parameter(torch.randn(5, 8, generator=g).to(dtype)) for _ in range(n)]


def test_keywords_and_the_refusal_with_fp32_state():
    from llm_fp8_amd.optim import ClippedAdamW
    opt = ClippedAdamW(_params(), stochastic_rounding=True, sr_seed=11)
    assert opt.state_dtype == torch.bfloat16 and opt._sr and opt.sr_seed == 11
    assert all(g["stochastic_rounding"] is True and g["sr_seed"] == 11 for g in opt.param_groups)
    with pytest.raises(ValueError, match="stochastic_rounding"):
        ClippedAdamW(_params(), state_dtype=torch.float32, stochastic_rounding=True)
    ClippedAdamW(_params(), state_dtype=torch.float32, stochastic_rounding=False, sr_seed=5)  # the seed alone asks for nothing


def _fake_state(opt):
    g = torch.Generator().manual_seed(11)
    for p in (q for grp in opt.param_groups for q in grp["params"]):
        opt.state[p] = {"step": 3, "exp_avg": torch.randn(p.shape, generator=g).to(torch.bfloat16),
                        "exp_avg_sq": torch.rand(p.shape, generator=g).to(torch.bfloat16)}


def test_default_mode_state_dict_is_unchanged_key_for_key_and_the_mode_travels_only_when_on():
    from llm_fp8_amd.optim import ClippedAdamW
    plain = ClippedAdamW(_params())
    _fake_state(plain)
    sd = plain.state_dict()
    assert [sorted(g) for g in sd["param_groups"]] == [["betas", "eps", "lr", "params", "weight_decay"]]
    assert all(sorted(st) == ["exp_avg", "exp_avg_sq", "step"] for st in sd["state"].values())
    sr = ClippedAdamW(_params(), stochastic_rounding=True, sr_seed=9)
    _fake_state(sr)
    sd_sr = sr.state_dict()
    assert [sorted(g) for g in sd_sr["param_groups"]] == [["betas", "eps", "lr", "params", "sr_seed", "stochastic_rounding", "weight_decay"]]
    assert all(sorted(st) == ["exp_avg", "exp_avg_sq", "step"] and st["exp_avg"].dtype == torch.bfloat16 for st in sd_sr["state"].values())
    # the layout is torch's: both load into torch.optim.AdamW and into each other
    torch.optim.AdamW(_params()).load_state_dict(copy.deepcopy(sd))
    again = ClippedAdamW(_params(), stochastic_rounding=True, sr_seed=1)
    again.load_state_dict(copy.deepcopy(sd_sr))
    assert again.param_groups[0]["sr_seed"] == 9                       # a resumed run continues the saved stream
    again.load_state_dict(copy.deepcopy(sd))                           # a default-mode state: the mode stays this optimiser's
    assert again.param_groups[0]["stochastic_rounding"] is True and again.param_groups[0]["sr_seed"] == 1
    plain.load_state_dict(copy.deepcopy(sd_sr))
    assert sorted(plain.state_dict()["param_groups"][0]) == ["betas", "eps", "lr", "params", "weight_decay"]


def test_flag_config_and_environment_resolve_the_mode(monkeypatch):
    from llm_fp8_amd import train
    monkeypatch.delenv("LLM_FP8_AMD_OPT_STATE", raising=False)
    parse = lambda argv: train.config_from_args(train.build_arg_parser().parse_args(argv))
    assert "bf16_sr" in train.OPTIMIZER_STATES
    assert train.resolve_optimizer_state(parse([])) == "bf16"
    assert parse(["--optimizer_state", "bf16_sr"]).optimizer_state == "bf16_sr"
    assert train.resolve_optimizer_state(parse(["--optimizer_state", "bf16_sr"])) == "bf16_sr"
    assert train.resolve_optimizer_state(train.TrainingConfig(optimizer_state="bf16_sr")) == "bf16_sr"
    monkeypatch.setenv("LLM_FP8_AMD_OPT_STATE", "bf16_sr")
    assert train.resolve_optimizer_state(parse([])) == "bf16_sr"                                  # None -> the environment
    assert train.resolve_optimizer_state(parse(["--optimizer_state", "bf16"])) == "bf16"          # the flag wins
    assert train.resolve_optimizer_state(parse(["--optimizer_state", "fp32"])) == "fp32"
    monkeypatch.setenv("LLM_FP8_AMD_OPT_STATE", "fp32")
    assert train.resolve_optimizer_state(parse(["--optimizer_state", "bf16_sr"])) == "bf16_sr"


def test_create_optimizer_refuses_bf16_sr_where_it_would_build_torch_adamw(monkeypatch):
    from llm_fp8_amd import train
    monkeypatch.delenv("LLM_FP8_AMD_OPT_STATE", raising=False)
    model = torch.nn.Linear(8, 8).to(torch.bfloat16)  # CPU parameters: torch.optim.AdamW
    with pytest.raises(RuntimeError, match="bf16_sr.*not all on the GPU.*torch.optim.AdamW would be built instead"):
        train.create_optimizer(model, train.TrainingConfig(optimizer_state="bf16_sr"))
    monkeypatch.setenv("LLM_FP8_AMD_OPT_STATE", "bf16_sr")
    with pytest.raises(RuntimeError, match="bf16_sr"):
        train.create_optimizer(model, train.TrainingConfig())
    opt, _ = train.create_optimizer(model, train.TrainingConfig(optimizer_state="bf16"))
    assert type(opt) is torch.optim.AdamW


def test_replicated_state_bytes_of_bf16_sr_is_the_bf16_figure():
    from llm_fp8_amd.distributed import replicated_state_bytes
    m = torch.nn.Sequential(torch.nn.Linear(16, 32), torch.nn.Linear(32, 8)).to(torch.bfloat16)
    assert replicated_state_bytes(m, optimizer_state="bf16_sr") == replicated_state_bytes(m, optimizer_state="bf16") == replicated_state_bytes(m)


def test_sr_keys_by_position_and_a_shard_gets_its_parents_key_and_first_element():
    from llm_fp8_amd import train
    from llm_fp8_amd.distributed import ShardedFP8DP
    from llm_fp8_amd.optim import ClippedAdamW

    class Wrapper(torch.nn.Module):  # a data-parallel wrapper as far as assign_sr_keys looks: `.module`
        def __init__(self, m):
            super().__init__()
            self.module = m
    inner = torch.nn.Sequential(torch.nn.Linear(16, 64, bias=False), torch.nn.Linear(64, 8)).to(torch.bfloat16)
    train.assign_sr_keys(Wrapper(inner))
    assert [p._mi_sr_key for p in inner.parameters()] == [(0, 0), (1, 0), (2, 0)]
    # the shards of ShardedFP8DP.optimizer_param_groups: rows [r0, r0 + n) of a [64, 16] weight keyed 0
    full = inner[0].weight
    shards = {}
    for r0 in (0, 32):
        sp = torch.nn.Parameter(full.data[r0:r0 + 32].clone())
        sp._mi_shard_of = (full, r0, 32)
        shards[r0] = sp
    fake = type("Fake", (), {"_shards": shards, "_sharded": {id(full): full}, "module": inner, "group": None})()
    groups = ShardedFP8DP.optimizer_param_groups(fake)
    assert [p._mi_sr_key for p in groups[1]["params"]] == [(0, 0), (0, 32 * 16)]
    assert all(p is not full for p in groups[0]["params"]) and groups[1]["sharded"] is True
    # the optimiser: `_mi_sr_key` when present, else (running index over the param groups, 0)
    a, b, c = _params(3)
    b._mi_sr_key = (77, 4096)
    opt = ClippedAdamW([{"params": [a]}, {"params": [b, c]}], stochastic_rounding=True)
    assert [opt._sr_key(p) for p in (a, b, c)] == [(0, 0), (77, 4096), (2, 0)]
    c._mi_sr_key = (1 << 30, 0)
    with pytest.raises(ValueError, match="tensor key"):
        opt._sr_key(c)


# ---- the numpy model of the feature inside the bounds of the GPU tests 4 and 5 (same inputs, same seeds, same figures)
def displacement_inputs():
    """The inputs of profiles/optim_fp32_state.txt section 3 (tests/test_optim_fp32_state_gpu.py test C)."""
    n, steps = 65536 + 8, 64
    hp = dict(lr=1.41e-5, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2)
    gen = torch.Generator().manual_seed(1234)
    p0 = (0.02 * torch.randn(n, generator=gen)).to(torch.bfloat16)
    grads = [(1e-3 * torch.randn(n, generator=gen) + 5e-4).to(torch.bfloat16) for _ in range(steps)]
    return n, steps, hp, p0, grads


def displacement_reference(p0, grads, hp):
    """float64 AdamW on the same bf16 gradients: the displacement p_64 - p_0."""
    lr, eps, wd, b1, b2 = (float(np.float32(x)) for x in (hp["lr"], hp["eps"], hp["weight_decay"], *hp["betas"]))
    w = p0.double().numpy().copy()
    m, v = np.zeros_like(w), np.zeros_like(w)
    for t, g in enumerate(grads, 1):
        g = g.double().numpy()
        m = b1 * m + (1.0 - b1) * g
        v = b2 * v + (1.0 - b2) * g * g
        w = w * (1.0 - lr * wd) - lr / (1.0 - b1 ** t) * m / (np.sqrt(v) / np.sqrt(1.0 - b2 ** t) + eps)
    return w - p0.double().numpy()


def displacement_figures(end, p0, ref):
    """(summed-displacement error / |sum of the reference|, per-weight relative L2 error, share of the weights that moved)."""
    d = end - p0
    return (abs(d.sum() - ref.sum()) / abs(ref.sum()), float(np.linalg.norm(d - ref) / np.linalg.norm(ref)), float((d != 0).mean()))


def test_the_model_keeps_the_summed_displacement_within_5_percent_and_round_to_nearest_does_not():
    n, steps, hp, p0, grads = displacement_inputs()
    ref = displacement_reference(p0, grads, hp)
    p0b = p0.view(torch.int16).numpy().view(np.uint16)
    fig = {}
    for sr in (True, False):
        pb, mb, vb = p0b.copy(), np.zeros(n, np.uint16), np.zeros(n, np.uint16)
        for t, g in enumerate(grads, 1):
            pb, mb, vb = S.model_step(pb, g.float().numpy(), mb, vb, t, hp, seed=42, key=0, base=0, sr=sr)
        fig[sr] = displacement_figures(S.bf16_bits_to_f32(pb).astype(np.float64), p0.double().numpy(), ref)
        print(f"model, stochastic rounding {sr}: summed displacement off by {100 * fig[sr][0]:.2f} %, per-weight relative L2 error "
              f"{fig[sr][1]:.3f}, weights that moved {100 * fig[sr][2]:.1f} %")
    assert fig[True][0] <= 0.05, fig
    assert fig[False][0] > 0.05, fig


def test_the_model_lets_exp_avg_sq_decay_and_round_to_nearest_does_not():
    n, steps = 65536, 256
    hp = dict(lr=1.41e-5, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2)
    v0 = 2.0 ** -20
    g = np.zeros(n, np.float32)
    for sr in (True, False):
        pb = S.rne_bf16_bits(np.full(n, 0.02, np.float32))
        mb, vb = np.zeros(n, np.uint16), S.f32_to_bf16_bits_exact(np.full(n, v0, np.float32))
        for t in range(1, steps + 1):
            pb, mb, vb = S.model_step(pb, g, mb, vb, t, hp, seed=42, key=0, base=0, sr=sr)
        ratio = float(S.bf16_bits_to_f32(vb).astype(np.float64).mean() / v0)
        print(f"model, stochastic rounding {sr}: mean(exp_avg_sq) / start after {steps} steps {ratio:.5f} (0.999^256 = {0.999 ** 256:.5f})")
        if sr:
            assert abs(ratio - 0.999 ** 256) <= 1.5e-3, ratio
        else:
            assert ratio == 1.0
