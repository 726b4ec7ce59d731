"""CPU: mi_layernorm_stats, mi_ln_cast, mi_amax_ln and mi_layernorm_bwd refuse bad arguments on the host, before any launch, by name;
their revision and signatures; which modules module._can_fuse_norm sends to them."""
import re
from pathlib import Path

import pytest
import torch

P, OFF = 0x10000, 0x10008  # fake pointers: 16-byte aligned, and 8 bytes off
#      (x, mean, R, C): every call below differs from the valid (P, P, 8, 8) in one argument
BAD = {"null x": (None, P, 8, 8), "null mean": (P, None, 8, 8), "misaligned x": (OFF, P, 8, 8), "misaligned mean": (P, OFF, 8, 8),
       "rows % 8": (P, P, 12, 8), "cols % 8": (P, P, 8, 20), "cols > 8192": (P, P, 8, 8200)}
CALLS = {  # the entry point's argument list around (x, mean, R, C), every other argument valid
    "mi_layernorm_stats": lambda f, x, m, R, C: f(x, m, P, R, C, 1e-5, None),
    "mi_ln_cast": lambda f, x, m, R, C: f(x, m, P, P, P, P, P, P, P, R, C, 0, 0, None),
    "mi_amax_ln": lambda f, x, m, R, C: f(x, m, P, P, P, P, 4, R, C, 0, None),
    "mi_layernorm_bwd": lambda f, x, m, R, C: f(P, x, m, P, P, None, P, P, P, 4, R, C, 0, None),
}
WALKS = ("mi_ln_cast", "mi_amax_ln")  # rows % 8 is theirs (8 x 8 blocks); the width limit is the other two's (a row in registers)


@pytest.mark.parametrize("entry,case", [(e, c) for e in sorted(CALLS) for c in sorted(BAD)
                                        if (c != "rows % 8" or e in WALKS) and (c != "cols > 8192" or e not in WALKS)])
def test_refused_on_the_host_by_name(entry, case):
    from llm_fp8_amd import _lib
    lib = _lib.load()
    rc = CALLS[entry](getattr(lib, entry), *BAD[case])
    assert rc == -1 and lib.mi_last_error().decode().startswith(entry + ":"), lib.mi_last_error()


def test_revision_and_signatures():
    from llm_fp8_amd import _lib
    lib, src = _lib.load(), (Path(__file__).resolve().parents[1] / "include" / "mi_fp8.h").read_text()
    assert int(re.search(r"#define\s+MI_ABI_REVISION\s+(\d+)", src).group(1)) == lib.mi_abi_revision() == _lib.ABI_REVISION >= 12
    for name in CALLS:
        decl = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", src)
        assert decl and len(decl.group(1).split(",")) == len(_lib.REVISION_SIGNATURES[name]) and hasattr(lib, name), name


@pytest.mark.parametrize("norm,zero_centered,hidden,want", [
    ("LayerNorm", False, 768, (True, True, False, False)), ("LayerNorm", True, 1600, (True, True, False, False)),
    ("LayerNorm", False, 8200, (False,) * 4), ("LayerNorm", False, 8192, (True, True, False, False)),
    ("RMSNorm", False, 512, (True,) * 4), ("RMSNorm", False, 768, (False,) * 4), ("RMSNorm", True, 512, (False,) * 4)])
def test_can_fuse_norm(norm, zero_centered, hidden, want):
    """(delayed, current, MXFP8, block scaling): LayerNorm under the per-tensor recipes at any hidden % 16 up to 8192; RMSNorm as before."""
    import llm_fp8_amd.pytorch as te
    from llm_fp8_amd.common import recipe as R
    from llm_fp8_amd.pytorch import module as M
    mod = te.LayerNormLinear(hidden, 16, normalization=norm, zero_centered_gamma=zero_centered, bias=False,
                             params_dtype=torch.bfloat16, device="cpu")
    recipes = (R.DelayedScaling(), R.Float8CurrentScaling(), R.MXFP8BlockScaling(), R.Float8BlockScaling())
    assert tuple(bool(M._can_fuse_norm(mod, r, torch.empty(8, hidden))) for r in recipes) == want
    mod.fused_norm = False
    assert not any(M._can_fuse_norm(mod, r, torch.empty(8, hidden)) for r in recipes)
