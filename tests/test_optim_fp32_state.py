"""CPU: the fp32 optimiser state of optim.ClippedAdamW as far as no GPU is needed -- the C ABI of mi_adamw_f32_multi (header,
library and binding agree; host refusals), the revision number next to MI_ABI_VERSION, the keyword and its harness switches
(`TrainingConfig.optimizer_state`, `--optimizer_state`, LLM_FP8_AMD_OPT_STATE), `load_state_dict` in and across the two modes,
and the memory estimate behind `--sharding_mode auto`."""
import copy
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x10000  # non-null, 16-byte aligned; every call below is refused (or has nothing to do) before anything is dereferenced
ADAM = (1e-3, 0.9, 0.999, 1e-8, 1e-2)


def _header():
    return open(os.path.join(ROOT, "include", "mi_fp8.h")).read()


def test_header_library_and_binding_agree_on_the_revision_and_the_new_entry_points():
    from llm_fp8_amd import _lib
    src = _header()
    lib = _lib.load()
    ver = int(re.search(r"#define\s+MI_ABI_VERSION\s+(\d+)", src).group(1))
    rev = int(re.search(r"#define\s+MI_ABI_REVISION\s+(\d+)", src).group(1))
    assert ver == lib.mi_abi_version() == _lib.ABI_VERSION == 5          # an added entry point does not move the version
    assert rev == lib.mi_abi_revision() == _lib.ABI_REVISION >= 1
    assert _lib.revision() == rev
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in ("mi_adamw_f32_multi", "mi_abi_revision"):
        assert re.search(r"\bint\s+%s\s*\(" % name, code), f"{name} is not declared in include/mi_fp8.h"
        assert hasattr(lib, name), f"libmi_fp8.so does not export {name}"
        assert name in _lib.SIGNATURES and name in _lib.REVISION_SIGNATURES
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name]
    # the declaration, argument for argument: 5 table / chunk arguments, grad_scale, 5 floats, step, sink_kind, stream
    decl = re.search(r"int\s+mi_adamw_f32_multi\s*\((.*?)\)\s*;", code, flags=re.S).group(1)
    args = [a.strip() for a in decl.split(",")]
    assert len(args) == len(_lib.SIGNATURES["mi_adamw_f32_multi"]) == 14
    assert args[-2] == "int sink_kind" and args[-3] == "int64_t step" and args[-1] == "void* stream"
    assert [a.split()[0] for a in args[6:11]] == ["float"] * 5


def test_host_refusals_before_any_launch():
    from llm_fp8_amd import _lib
    lib = _lib.load()
    call = lambda table=FAKE, n_tensors=1, chunks=FAKE, n_chunks=4, chunk_elems=65536, step=1, sink_kind=0: lib.mi_adamw_f32_multi(
        table, n_tensors, chunks, n_chunks, chunk_elems, None, *ADAM, step, sink_kind, None)
    for kw in (dict(table=None), dict(chunks=None), dict(n_tensors=0), dict(n_tensors=-3), dict(chunk_elems=0), dict(chunk_elems=-8),
               dict(chunk_elems=12), dict(chunk_elems=65537), dict(sink_kind=-1), dict(sink_kind=2)):
        assert call(**kw) == -1, kw                                   # MI_ERR_ARG
        assert b"mi_adamw_f32_multi" in lib.mi_last_error(), kw
    for sink_kind in (0, 1):
        assert call(n_chunks=0, sink_kind=sink_kind) == 0               # nothing to do: MI_OK, nothing launched
    with pytest.raises(RuntimeError, match="sink_kind"):
        _lib.check(call(sink_kind=7), "mi_adamw_f32_multi")


def test_a_library_without_the_revision_still_binds_and_the_request_is_refused(monkeypatch):
    """LLM_FP8_AMD_LIB may point at a build of ABI 5 from before the revision (A/B timing): it loads, and asking it for fp32
    state says what is missing."""
    from llm_fp8_amd import _lib

    class Old:  # the surface of such a build, as far as `require` looks
        def mi_abi_version(self):
            return 5
    monkeypatch.setattr(_lib, "_lib", Old())
    assert _lib.revision() == 0
    with pytest.raises(RuntimeError, match=r"mi_adamw_f32_multi.*revision"):
        _lib.require("mi_adamw_f32_multi", "ClippedAdamW(state_dtype=torch.float32)")


def _params(n=2, dtype=torch.bfloat16):
    g = torch.Generator().manual_seed(3)
    return [torch.nn.Parameter(torch.randn(5, 8, generator=g).to(dtype)) for _ in range(n)]


def test_state_dtype_keyword():
    from llm_fp8_amd.optim import ClippedAdamW
    assert ClippedAdamW(_params()).state_dtype == torch.bfloat16
    assert ClippedAdamW(_params(), state_dtype=torch.float32).state_dtype == torch.float32
    for bad in (torch.float16, torch.float64, None, "fp32"):
        with pytest.raises(ValueError, match="state_dtype"):
            ClippedAdamW(_params(), state_dtype=bad)


def test_create_optimizer_refuses_fp32_state_where_it_would_build_torch_adamw(monkeypatch):
    from llm_fp8_amd import train
    monkeypatch.delenv("LLM_FP8_AMD_OPT_STATE", raising=False)
    model = torch.nn.Linear(8, 8).to(torch.bfloat16)  # CPU parameters: torch.optim.AdamW
    with pytest.raises(RuntimeError, match="fp32.*not all on the GPU"):
        train.create_optimizer(model, train.TrainingConfig(optimizer_state="fp32"))
    monkeypatch.setenv("LLM_FP8_AMD_OPT_STATE", "fp32")  # the environment route reaches the same refusal
    with pytest.raises(RuntimeError, match="fp32"):
        train.create_optimizer(model, train.TrainingConfig())
    opt, _ = train.create_optimizer(model, train.TrainingConfig(optimizer_state="bf16"))  # explicit beats the environment
    assert type(opt) is torch.optim.AdamW


def test_flag_and_environment_resolve_as_documented(monkeypatch):
    from llm_fp8_amd import train
    monkeypatch.delenv("LLM_FP8_AMD_OPT_STATE", raising=False)
    parse = lambda argv: train.config_from_args(train.build_arg_parser().parse_args(argv))
    assert train.TrainingConfig().optimizer_state is None and parse([]).optimizer_state is None
    assert train.resolve_optimizer_state(parse([])) == "bf16"
    assert parse(["--optimizer_state", "fp32"]).optimizer_state == "fp32"
    assert train.resolve_optimizer_state(parse(["--optimizer_state", "fp32"])) == "fp32"
    with pytest.raises(SystemExit):
        parse(["--optimizer_state", "fp16"])
    monkeypatch.setenv("LLM_FP8_AMD_OPT_STATE", "fp32")
    assert train.resolve_optimizer_state(parse([])) == "fp32"                                   # None -> the environment
    assert train.resolve_optimizer_state(parse(["--optimizer_state", "bf16"])) == "bf16"        # the flag wins
    monkeypatch.setenv("LLM_FP8_AMD_OPT_STATE", "fp64")
    with pytest.raises(ValueError, match="fp64"):
        train.resolve_optimizer_state(train.TrainingConfig())


def _fake_state(opt, dtype, with_master):
    """Per-parameter state as a step would leave it, with values bf16 cannot hold (so a trip through bf16 shows)."""
    g = torch.Generator().manual_seed(11)
    for p in (q for grp in opt.param_groups for q in grp["params"]):
        st = opt.state[p]
        st["step"] = 3
        st["exp_avg"] = (torch.randn(p.shape, generator=g) * 1e-3).to(dtype)
        st["exp_avg_sq"] = (torch.rand(p.shape, generator=g) * 1e-6).to(dtype)
        if with_master:
            st["master"] = p.detach().float() * (1 + 2.0 ** -12)  # rounds to p, is not p
            st["master_version"] = 12345


def test_load_state_dict_keeps_fp32_state_for_bf16_parameters():
    from llm_fp8_amd.optim import ClippedAdamW
    src = ClippedAdamW(_params(), state_dtype=torch.float32)
    _fake_state(src, torch.float32, True)
    sd = copy.deepcopy(src.state_dict())
    params = _params()
    dst = ClippedAdamW(params, state_dtype=torch.float32)
    dst.load_state_dict(sd)
    for ps, pd in zip(src.param_groups[0]["params"], params):
        a, b = src.state[ps], dst.state[pd]
        assert b["step"] == 3
        for k in ("exp_avg", "exp_avg_sq", "master"):
            assert b[k].dtype == torch.float32 and torch.equal(a[k], b[k]), k   # bitwise: no trip through the parameter's bf16
        assert not torch.equal(b["master"], pd.detach().float())                  # the loaded master, not a re-seed
        assert b["master_version"] == pd._version                                 # trusted until somebody writes the parameter


def test_load_bf16_state_into_fp32_mode_upcasts_and_seeds_the_master():
    from llm_fp8_amd.optim import ClippedAdamW
    src = ClippedAdamW(_params())
    _fake_state(src, torch.bfloat16, False)
    params = _params()
    dst = ClippedAdamW(params, state_dtype=torch.float32)
    dst.load_state_dict(copy.deepcopy(src.state_dict()))
    for ps, pd in zip(src.param_groups[0]["params"], params):
        a, b = src.state[ps], dst.state[pd]
        for k in ("exp_avg", "exp_avg_sq"):
            assert b[k].dtype == torch.float32 and torch.equal(b[k], a[k].float())
        assert b["master"].dtype == torch.float32 and torch.equal(b["master"], pd.detach().float())
        assert b["master_version"] == pd._version


def test_load_fp32_state_into_bf16_mode_downcasts_and_drops_the_master():
    from llm_fp8_amd.optim import ClippedAdamW
    src = ClippedAdamW(_params(), state_dtype=torch.float32)
    _fake_state(src, torch.float32, True)
    params = _params()
    dst = ClippedAdamW(params)
    dst.load_state_dict(copy.deepcopy(src.state_dict()))
    for ps, pd in zip(src.param_groups[0]["params"], params):
        a, b = src.state[ps], dst.state[pd]
        assert "master" not in b and "master_version" not in b
        for k in ("exp_avg", "exp_avg_sq"):
            assert b[k].dtype == torch.bfloat16 and torch.equal(b[k], a[k].to(torch.bfloat16))
    # bf16 -> bf16 is torch's own load, unchanged
    again = ClippedAdamW(_params())
    again.load_state_dict(copy.deepcopy(dst.state_dict()))
    assert all(st["exp_avg"].dtype == torch.bfloat16 and set(st) == {"step", "exp_avg", "exp_avg_sq"} for st in again.state.values())


def test_replicated_state_grows_by_8_bytes_per_trainable_parameter():
    from llm_fp8_amd.distributed import fits_replicated, replicated_state_bytes
    m = torch.nn.Sequential(torch.nn.Linear(16, 32), torch.nn.Linear(32, 8)).to(torch.bfloat16)
    m[1].bias.requires_grad_(False)
    trainable = sum(p.numel() for p in m.parameters() if p.requires_grad)
    base = replicated_state_bytes(m)
    assert replicated_state_bytes(m, optimizer_state="bf16") == base
    assert replicated_state_bytes(m, optimizer_state="fp32") == base + 8 * trainable
    assert fits_replicated(m, torch.device("cpu"), optimizer_state="fp32")
