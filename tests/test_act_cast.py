"""CPU: mi_act_cast, mi_dact_cast, mi_amax_act and mi_amax_dact refuse bad arguments on the host, before any launch, by name."""
import pytest

P, OFF = 0x10000, 0x10008  # fake pointers: 16-byte aligned, and 8 bytes off
#           (h, bias, dact, R, F, act): every call below differs from the valid (P, P, P, 8, 8, 1) in one argument
BAD = {"act 0": (P, P, P, 8, 8, 0), "act 3": (P, P, P, 8, 8, 3), "null h": (None, P, P, 8, 8, 1), "misaligned h": (OFF, P, P, 8, 8, 2),
       "misaligned bias": (P, OFF, P, 8, 8, 1), "rows % 8": (P, None, P, 12, 8, 2), "F % 8": (P, None, P, 8, 20, 1),
       "null dact": (P, P, None, 8, 8, 1), "misaligned dact": (P, P, OFF, 8, 8, 2)}


@pytest.mark.parametrize("entry,case", [(e, c) for e in ("mi_act_cast", "mi_dact_cast", "mi_amax_act", "mi_amax_dact") for c in sorted(BAD)
                                        if "dact" in e or "dact" not in c])  # (the forward entry points take no dact)
def test_refused_on_the_host_by_name(entry, case):
    from llm_fp8_amd import _lib
    lib = _lib.load()
    h, bias, dact, R, F, act = BAD[case]
    takes_dact = entry in ("mi_dact_cast", "mi_amax_dact")
    head = (h, bias) + ((dact,) if takes_dact else ())
    if "amax" in entry:
        rc = getattr(lib, entry)(*head, P, 4, R, F, act, None)
    else:
        rc = getattr(lib, entry)(*head, P, P, P, None, *((None,) if takes_dact else ()), R, F, act, 0, None)
    assert rc == -1 and lib.mi_last_error().decode().startswith(entry + ":"), lib.mi_last_error()
