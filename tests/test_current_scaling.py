"""CPU: Float8CurrentScaling as far as no GPU is needed -- the recipe and its TE field names, revision 2 of ABI 5 (header, library
and binding agree on the five new entry points; host refusals), scenario `current` through llama / train, the recipe's `q` object
at a GEMM site, no arena from an autocast region, and the sharded data-parallel wrapper's refusal."""
import dataclasses
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mi_amax_bf16", "mi_amax_norm", "mi_amax_swiglu", "mi_amax_dswiglu", "mi_current_scale")
FAKE = 0x10000  # non-null, 16-byte aligned; every call below is refused before anything is dereferenced or launched


def test_recipe_fields_defaults_and_predicates():
    from llm_fp8_amd.common import recipe as R
    r = R.Float8CurrentScaling()
    assert isinstance(r, R.Recipe)
    assert r.current() and not r.delayed() and not r.mxfp8()
    assert not R.DelayedScaling().current() and not R.MXFP8BlockScaling().current()
    assert r.fp8_format is R.Format.HYBRID and r.fp8_dpa is False and r.fp8_mha is False
    for name in ("fp8_quant_fwd_inp", "fp8_quant_fwd_weight", "fp8_quant_bwd_grad"):
        q = getattr(r, name)
        assert isinstance(q, R.QParams) and q.power_2_scale is False and q.amax_epsilon == 0.0, name
    for name in ("fp8_gemm_fprop", "fp8_gemm_dgrad", "fp8_gemm_wgrad"):
        assert isinstance(getattr(r, name), R.MMParams) and isinstance(getattr(r, name).use_split_accumulator, bool), name
    assert [f.name for f in dataclasses.fields(r)] == [
        "fp8_format", "fp8_quant_fwd_inp", "fp8_quant_fwd_weight", "fp8_quant_bwd_grad", "fp8_gemm_fprop", "fp8_gemm_dgrad",
        "fp8_gemm_wgrad", "fp8_dpa", "fp8_mha"]
    r2 = R.Float8CurrentScaling(fp8_format=R.Format.E4M3, fp8_quant_fwd_inp=R.QParams(power_2_scale=True, amax_epsilon=1e-6),
                                fp8_gemm_fprop=R.MMParams(use_split_accumulator=True))
    assert r2.fp8_quant_fwd_inp.power_2_scale and r2.fp8_quant_fwd_weight.amax_epsilon == 0.0
    assert R.fmt_codes(r.fp8_format) == (0, 1) and R.fmt_codes(r2.fp8_format) == (0, 0)
    with pytest.raises(ValueError, match="amax_epsilon"):
        R.Float8CurrentScaling(fp8_quant_bwd_grad=R.QParams(amax_epsilon=-1.0))


def test_header_library_and_binding_agree_on_revision_2_and_the_five_entry_points():
    from llm_fp8_amd import _lib
    src = open(os.path.join(ROOT, "include", "mi_fp8.h")).read()
    lib = _lib.load()
    ver = int(re.search(r"#define\s+MI_ABI_VERSION\s+(\d+)", src).group(1))
    rev = int(re.search(r"#define\s+MI_ABI_REVISION\s+(\d+)", src).group(1))
    assert ver == lib.mi_abi_version() == _lib.ABI_VERSION == 5
    assert rev == lib.mi_abi_revision() == _lib.ABI_REVISION >= 2
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in NEW:
        decl = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, code, flags=re.S)
        assert decl, f"{name} is not declared in include/mi_fp8.h"
        assert hasattr(lib, name), f"libmi_fp8.so does not export {name}"
        assert name in _lib.SIGNATURES and name in _lib.REVISION_SIGNATURES
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name]
        assert len(decl.group(1).split(",")) == len(_lib.SIGNATURES[name]), name
        assert decl.group(1).split(",")[-1].strip() == "void* stream", name
    assert re.search(r"Revisions of version 5:.*?\n \*\s+2\s+mi_amax_bf16", src, flags=re.S), "revision history lacks revision 2"


def test_host_refusals_before_any_launch():
    from llm_fp8_amd import _lib
    lib = _lib.load()
    plain = lambda x=FAKE, p=FAKE, n=4, r=64, c=64: lib.mi_amax_bf16(x, p, n, r, c, None)
    for kw in (dict(x=None), dict(p=None), dict(n=0), dict(n=1025), dict(r=12), dict(c=20), dict(r=-8), dict(x=FAKE + 2)):
        assert plain(**kw) == -1, kw                                   # MI_ERR_ARG
        assert b"mi_amax_bf16" in lib.mi_last_error(), kw
    assert lib.mi_amax_norm(FAKE, None, FAKE, FAKE, 4, 64, 512, None) == -1 and b"mi_amax_norm" in lib.mi_last_error()
    assert lib.mi_amax_norm(FAKE, FAKE, FAKE + 8, FAKE, 4, 64, 512, None) == -1
    assert lib.mi_amax_swiglu(FAKE, FAKE + 8, FAKE, 4, 64, 64, None) == -1 and b"mi_amax_swiglu" in lib.mi_last_error()
    assert lib.mi_amax_swiglu(FAKE, None, FAKE, 4, 64, 60, None) == -1
    assert lib.mi_amax_dswiglu(FAKE, None, None, FAKE, 4, 64, 64, None) == -1 and b"mi_amax_dswiglu" in lib.mi_last_error()
    scale = lambda p=FAKE, n=4, mx=448.0, eps=0.0, out=FAKE: lib.mi_current_scale(p, n, mx, eps, 0, out, None)
    for kw in (dict(p=None), dict(out=None), dict(n=0), dict(mx=0.0), dict(eps=-1.0)):
        assert scale(**kw) == -1, kw
        assert b"mi_current_scale" in lib.mi_last_error(), kw


def test_scenario_current_through_llama_and_the_argument_parser():
    from llm_fp8_amd import llama, train
    from llm_fp8_amd.common.recipe import Float8CurrentScaling
    attn, mlp = llama.scenario_recipes("current")
    assert isinstance(attn, Float8CurrentScaling) and attn is mlp
    assert isinstance(llama.outer_recipe_for_scenario("current"), Float8CurrentScaling)
    assert llama.decoder_layer_cls("current").scenario == "current"
    cfg = train.config_from_args(train.build_arg_parser().parse_args(["--use_te", "--fp8_scenario", "current"]))
    assert cfg.fp8_scenario == "current" and cfg.use_te
    with pytest.raises(SystemExit):
        train.build_arg_parser().parse_args(["--fp8_scenario", "currant"])


def test_gemm_spec_carries_a_current_q_and_prepare_builds_no_state():
    import llm_fp8_amd.pytorch as te
    from llm_fp8_amd.common.recipe import DelayedScaling, Float8CurrentScaling, MXFP8BlockScaling
    from llm_fp8_amd.pytorch import module as M
    from llm_fp8_amd.pytorch.fp8 import FP8GlobalStateManager
    r = Float8CurrentScaling()
    spec = M._GemmSpec(r, None, None, 0, False, True)
    q = spec.q
    assert type(q) is M._CurrentQ and q.recipe is r and (q.fmt_f, q.fmt_b) == (0, 1)
    assert q.mx is False and q.swiglu_adds_bias is True
    assert len({q.cache_key, M._DelayedQ.cache_key, M._MXQ.cache_key}) == 3 and len({q.sink_key, M._DelayedQ.sink_key, M._MXQ.sink_key}) == 3
    for name in ("quantize", "swiglu", "quantize_grad", "dswiglu", "offer", "taken", "operands", "gemm", "unflat", "quantize_weights",
                 "new_sink"):
        assert callable(getattr(q, name)) and callable(getattr(M._DelayedQ, name)), name
    assert q.new_sink((), (), 256, 256, None, 0) is None
    h = M.DyHandoff()
    q.offer(h, 0, True, True)
    assert not h.offered()
    assert type(M._GemmSpec(MXFP8BlockScaling(), None, None, 0, False, True).q) is M._MXQ
    assert type(M._GemmSpec(DelayedScaling(), None, None, 0, False, True).q) is M._DelayedQ
    # _prepare under the recipe: no meta windows, an empty _extra_state (FP8 "enabled" by hand: the autocast wants a GPU)
    FP8GlobalStateManager.reset()
    lin = te.Linear(32, 32, bias=False, params_dtype=torch.bfloat16, device="cpu")
    try:
        FP8GlobalStateManager.FP8_ENABLED, FP8GlobalStateManager.FP8_RECIPE = True, r
        st = lin._prepare(torch.device("cpu"))
        assert st[0] is r and st[1] is None and st[2] is None
        assert lin._meta_fwd is None and lin.get_extra_state().numel() == 0
        assert FP8GlobalStateManager._arenas == {}
    finally:
        FP8GlobalStateManager.reset()
    norm = te.LayerNormLinear(512, 512, normalization="RMSNorm", bias=False, params_dtype=torch.bfloat16, device="cpu")
    assert M._can_fuse_norm(norm, r, torch.empty(8, 512))


def test_autocast_with_the_recipe_leaves_no_arena(monkeypatch):
    from llm_fp8_amd.common.recipe import Float8CurrentScaling
    from llm_fp8_amd.pytorch import fp8
    monkeypatch.setattr(fp8, "check_fp8_support", lambda: (True, ""))
    fp8.FP8GlobalStateManager.reset()
    with fp8.fp8_autocast(enabled=True, fp8_recipe=Float8CurrentScaling()):
        assert fp8.FP8GlobalStateManager.get_fp8_recipe().current()
        with fp8.fp8_autocast(enabled=True, fp8_recipe=Float8CurrentScaling()):
            pass
    assert fp8.FP8GlobalStateManager._arenas == {} and not fp8.FP8GlobalStateManager.is_fp8_enabled()
    fp8.FP8GlobalStateManager.reset()


class _Layer(torch.nn.Module):
    """What distributed.uses_current_scaling looks at on a decoder layer."""

    def __init__(self, scenario):
        super().__init__()
        from llm_fp8_amd import llama
        self.attn_recipe, self.mlp_recipe = llama.scenario_recipes(scenario)
        self.proj = torch.nn.Linear(64, 64).to(torch.bfloat16)


def test_sharded_fp8_dp_refuses_the_recipe_and_auto_avoids_it(tmp_path, monkeypatch):
    """gloo at world size 1 in this process: ShardedFP8DP refuses a model of scenario `current` when wrapping it (and wraps the same
    model under delayed scaling), and `auto` never resolves to fsdp_fp8 for it."""
    import torch.distributed as dist
    from llm_fp8_amd import distributed as D, llama, train
    cur, dflt = torch.nn.Sequential(_Layer("current")), torch.nn.Sequential(_Layer("default"))
    assert D.uses_current_scaling(cur) and not D.uses_current_scaling(dflt)
    outer = torch.nn.Sequential(torch.nn.Linear(8, 8))
    llama.apply_fp8_autowrap(outer, llama.outer_recipe_for_scenario("current"))
    assert D.uses_current_scaling(outer)
    dist.init_process_group("gloo", init_method=f"file://{tmp_path}/rdzv", rank=0, world_size=1)
    try:
        with pytest.raises(RuntimeError, match=r"Float8CurrentScaling.*replicated"):
            D.ShardedFP8DP(cur)
        assert isinstance(D.ShardedFP8DP(dflt), D.ShardedFP8DP)
        # a model too large to replicate, on more than one rank
        monkeypatch.setattr(D, "fits_replicated", lambda *a, **k: False)
        monkeypatch.setattr(dist, "get_world_size", lambda *a, **k: 2)
        assert train.resolve_sharding_mode("auto", dflt, torch.device("cpu")) == "fsdp_fp8"
        assert train.resolve_sharding_mode("auto", cur, torch.device("cpu")) == "fsdp_full"
        assert train.resolve_sharding_mode("auto", outer, torch.device("cpu")) == "fsdp_full"
        monkeypatch.setattr(D, "fits_replicated", lambda *a, **k: True)
        assert train.resolve_sharding_mode("auto", cur, torch.device("cpu")) == "replicated"
    finally:
        monkeypatch.undo()
        dist.destroy_process_group()
