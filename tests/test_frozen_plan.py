"""CPU: what the FP8 GEMM Functions compute and keep under every requires_grad pattern (module.linear_plan / mlp_plan /
grad_copies) and which Function claims the delayed-scaling backward update (module._claim_bwd_update).  The GPU counterpart, bit for
bit against an all-trainable twin, is tests/test_frozen_params_gpu.py."""
import itertools
from types import SimpleNamespace


def test_linear_plan_keeps_exactly_what_its_backward_gemms_read():
    from llm_fp8_amd.pytorch.module import linear_plan
    for x, b, ln, w in itertools.product((False, True), repeat=4):
        p = linear_plan(x, b, ln, w)
        assert p.dgrad == (x or ln) and p.wgrad == w and p.dbias == b
        assert p.w_col == p.dgrad       # dX = G8 . W8T^T reads the weight's column-wise copy
        assert p.x_col == p.wgrad       # dW = G8T . X8T^T reads the input's
    assert linear_plan(True, True, True, True) == (True, True, True, True, True)   # the all-trainable path: everything, as before
    assert linear_plan(1, 0, 0, 0).dgrad is True                                    # plain bools whatever autograd hands in


def test_mlp_plan_keeps_exactly_what_its_backward_reads():
    from llm_fp8_amd.pytorch.module import mlp_plan
    for x, w1, b1, w2, b2, ln in itertools.product((False, True), repeat=6):
        p = mlp_plan(x, w1, b1, w2, b2, ln)
        assert (p.dgrad, p.w1, p.b1, p.w2, p.b2) == (x or ln, w1, b1, w2, b2)
        # anything upstream of the activation -- the fc1 BIAS included -- needs dact, hence h and fc2's column-wise weight
        assert p.dact == (x or ln or w1 or b1)
        assert p.h == p.dact and p.w2_col == p.dact
        assert p.a_col == w2 and p.x_col == w1 and p.w1_col == p.dgrad
        if p.dgrad or p.w1 or p.b1:
            assert p.h and p.w2_col, "backward would feed None into dSwiGLU / the fc2 dgrad GEMM"
    assert all(mlp_plan(*(True,) * 6))
    only_b1 = mlp_plan(False, False, True, False, False, False)
    assert only_b1.h and only_b1.w2_col and not (only_b1.x_col or only_b1.w1_col or only_b1.a_col)
    only_b2 = mlp_plan(False, False, False, False, True, False)
    assert only_b2.b2 and not only_b2.dact                      # backward ends at fc2: nothing is kept
    assert not (only_b2.x_col or only_b2.w1_col or only_b2.h or only_b2.a_col or only_b2.w2_col)


def test_grad_copies_never_asks_a_cast_kernel_for_neither_copy():
    from llm_fp8_amd.pytorch.module import grad_copies
    for row, col, cs in itertools.product((False, True), repeat=3):
        got = grad_copies(row, col, cs)
        if row or col:
            assert got == (row, col)               # what the GEMMs read, nothing more
        elif cs:
            assert got == (True, False)            # a bias gradient alone rides on the row-wise copy
        else:
            assert got is None                     # nothing to quantise
        assert got is None or any(got)


def test_backward_update_is_claimed_by_the_first_function_with_a_backward():
    from llm_fp8_amd.pytorch import module as M
    from llm_fp8_amd.pytorch.fp8 import FP8GlobalStateManager as S
    S.reset()
    try:
        S.IS_FIRST_FP8_MODULE = True   # what entering the outermost fp8_autocast sets
        frozen, first, later = (SimpleNamespace(trigger_bwd_update=False) for _ in range(3))
        M._claim_bwd_update(SimpleNamespace(needs_input_grad=(False, False, None, False, False)), frozen)
        assert not frozen.trigger_bwd_update and S.IS_FIRST_FP8_MODULE     # no backward: the claim stays open
        M._claim_bwd_update(SimpleNamespace(needs_input_grad=(False, True, None, False, False)), first)
        assert first.trigger_bwd_update and not S.IS_FIRST_FP8_MODULE
        M._claim_bwd_update(SimpleNamespace(needs_input_grad=(True, True, None, True, True)), later)
        assert not later.trigger_bwd_update                                # once per region
    finally:
        S.reset()
