"""CPU: the step guard of optim.ClippedAdamW (`skip_nonfinite`: a step whose gradient norm is Inf or NaN is dropped on the device) as
far as no GPU is needed -- header, library and binding agree on revision 5; the coefficient the kernels receive; the keyword's
three values against a library of revision 4; flag, environment switch and TrainingConfig; `state_dict()` keeps torch's layout."""
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_library_and_binding_agree_on_revision_5():
    from llm_fp8_amd import _lib, optim
    src = open(os.path.join(ROOT, "include", "mi_fp8.h")).read()
    lib = _lib.load()
    rev = int(re.search(r"#define\s+MI_ABI_REVISION\s+(\d+)", src).group(1))
    assert int(re.search(r"#define\s+MI_ABI_VERSION\s+(\d+)", src).group(1)) == lib.mi_abi_version() == _lib.ABI_VERSION == 5
    assert rev == lib.mi_abi_revision() == _lib.ABI_REVISION >= 5
    assert _lib.revision() == rev and optim.GUARD_REVISION == 5
    # revision 5 is a change of semantics: no symbol came with it
    assert not [n for n in _lib.SIGNATURES if "guard" in n or "skip" in n]


def _parent_coef(total_sq, max_norm):
    """The expression ClippedAdamW.step() had before the guard."""
    total = total_sq.sqrt().to(torch.float32)
    return total, (max_norm / (total + 1e-6)).clamp(max=1.0).reshape(1)


def _bits(t):
    return t.view(torch.int32).tolist()


@pytest.mark.parametrize("max_norm", [1.0, 0.3, 1e4])
def test_coefficient_is_the_parents_for_a_finite_norm(max_norm):
    from llm_fp8_amd.optim import guarded_clip_coefficient
    gen = torch.Generator().manual_seed(11)
    totals = [0.0, 1e-300, 1e-14, 1e-12, 2.5e-7, 0.25 * max_norm ** 2, max_norm ** 2, 1.0, 1.0 + 2.0 ** -30, 3.0, 1e8, 1e30, 3.0e76]
    totals += (10.0 ** (torch.rand(200, generator=gen, dtype=torch.float64) * 40 - 20)).tolist()
    below = 0
    for x in totals:
        t = torch.tensor(x, dtype=torch.float64)
        norm, coef = guarded_clip_coefficient(t, max_norm)
        want_norm, want = _parent_coef(t, max_norm)
        assert bool(torch.isfinite(want_norm)), x
        assert norm.dtype == coef.dtype == torch.float32 and norm.shape == () and coef.shape == (1,)
        assert _bits(norm.reshape(1)) == _bits(want_norm.reshape(1)) and _bits(coef) == _bits(want), (x, coef, want)
        below += float(want) == 1.0
    assert 0 < below < len(totals)  # both sides of max_norm were seen


@pytest.mark.parametrize("total", [float("inf"), float("nan"), 1e300])  # 1e300: finite in float64, its root is not in fp32
def test_coefficient_is_nan_for_a_non_finite_norm(total):
    from llm_fp8_amd.optim import guarded_clip_coefficient
    norm, coef = guarded_clip_coefficient(torch.tensor(total, dtype=torch.float64), 1.0)
    assert not bool(torch.isfinite(norm)) and coef.shape == (1,) and bool(torch.isnan(coef).all())
    # what the kernels test: every exponent bit set
    assert coef.view(torch.int32).item() & 0x7F800000 == 0x7F800000


class _Rev4:
    """A library of ABI 5 revision 4: everything the optimiser asks a library before a step."""

    def mi_abi_version(self):
        return 5

    def mi_abi_revision(self):
        return 4


def _opt(**kw):
    from llm_fp8_amd.optim import ClippedAdamW
    return ClippedAdamW([torch.nn.Parameter(torch.zeros(8, dtype=torch.bfloat16))], **kw)


def test_keyword_against_a_library_of_revision_4(monkeypatch):
    from llm_fp8_amd import _lib
    monkeypatch.setattr(_lib, "load", lambda: _Rev4())
    assert _lib.revision() == 4
    assert _opt()._guard_active() is False                       # None: off, the older build keeps working
    assert _opt(skip_nonfinite=False)._guard_active() is False
    with pytest.raises(RuntimeError, match=r"skip_nonfinite=True.*revision 4.*before revision 5"):
        _opt(skip_nonfinite=True)
    assert _opt(skip_nonfinite=True, max_grad_norm=None)._guard_active() is False   # no norm, no guard: nothing to refuse
    with pytest.raises(ValueError, match="skip_nonfinite"):
        _opt(skip_nonfinite="yes")


def test_keyword_against_this_library():
    assert _opt()._guard_active() is True
    assert _opt(skip_nonfinite=True)._guard_active() is True
    assert _opt(skip_nonfinite=False)._guard_active() is False
    for kw in ({}, dict(skip_nonfinite=True), dict(skip_nonfinite=False)):
        assert _opt(max_grad_norm=None, **kw)._guard_active() is False
    opt = _opt()
    assert opt.last_step_skipped is None and opt.skipped_steps is None


def test_flag_environment_and_config(monkeypatch):
    from llm_fp8_amd import train
    monkeypatch.delenv("LLM_FP8_AMD_NO_STEP_GUARD", raising=False)
    assert train.TrainingConfig().skip_nonfinite_steps is True
    ap = train.build_arg_parser()
    on, off = train.config_from_args(ap.parse_args([])), train.config_from_args(ap.parse_args(["--no_skip_nonfinite_steps"]))
    assert on.skip_nonfinite_steps is True and off.skip_nonfinite_steps is False
    assert train.resolve_skip_nonfinite(on) is None and train.resolve_skip_nonfinite(off) is False
    monkeypatch.setenv("LLM_FP8_AMD_NO_STEP_GUARD", "1")
    assert train.resolve_skip_nonfinite(on) is False and train.resolve_skip_nonfinite(off) is False
    monkeypatch.setenv("LLM_FP8_AMD_NO_STEP_GUARD", "0")
    assert train.resolve_skip_nonfinite(on) is None


def test_state_dict_keeps_torchs_layout():
    p = torch.nn.Parameter(torch.zeros(8, dtype=torch.bfloat16))
    ref = torch.optim.AdamW([p], lr=1e-3).state_dict()
    for kw in ({}, dict(skip_nonfinite=True), dict(skip_nonfinite=False)):
        sd = _opt(lr=1e-3, **kw).state_dict()
        assert set(sd) == {"state", "param_groups"} and sd["state"] == {}
        assert set(sd["param_groups"][0]) == {"lr", "betas", "eps", "weight_decay", "params"} <= set(ref["param_groups"][0])
        assert "skip" not in repr(sd)
