"""numpy restatement of fp32 gradient accumulation (include/mi_fp8.h mi_grad_accum_multi): the bf16 gradients of a window's
micro-batches are widened to float32 and added sequentially, in micro-batch order, one IEEE float32 add each; the sum is rounded
to bf16 once, round-to-nearest-even ON THE RAW BITS (no library conversion to trust).  float32 denormals are kept (numpy does
not flush), NaN and Inf follow from the arithmetic, and a sum beyond the bf16 range rounds to Inf."""
import numpy as np


def bf16_to_f32(bits: np.ndarray) -> np.ndarray:
    """uint16 bf16 bit patterns -> float32 (exact)."""
    return (np.asarray(bits, dtype=np.uint16).astype(np.uint32) << np.uint32(16)).view(np.float32)


def f32_to_bf16_rne(x: np.ndarray) -> np.ndarray:
    """float32 -> bf16 bit patterns, round to nearest even; NaN stays NaN (quiet bit set), overflow rounds to Inf."""
    b = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    rounded = (b + np.uint64(0x7FFF) + ((b >> np.uint64(16)) & np.uint64(1))) >> np.uint64(16)
    nan = (b & np.uint64(0x7FFFFFFF)) > np.uint64(0x7F800000)
    return np.where(nan, (b >> np.uint64(16)) | np.uint64(0x40), rounded).astype(np.uint16)


def window_sum(grads) -> np.ndarray:
    """float32 sum of a window: `grads` = the micro-batches' bf16 bit arrays in order (None: no gradient in that micro-batch).
    The first contribution is taken as it is (SET), every later one is one float32 add (ADD / FINISH)."""
    acc = None
    with np.errstate(all="ignore"):
        for g in grads:
            if g is None:
                continue
            f = bf16_to_f32(g)
            acc = f.copy() if acc is None else (acc + f).astype(np.float32)
    assert acc is not None and acc.dtype == np.float32
    return acc


def window_total(grads) -> np.ndarray:
    """bf16 bits of the window's gradient: the float32 sum rounded once."""
    return f32_to_bf16_rne(window_sum(grads))


def is_nan_bf16(bits: np.ndarray) -> np.ndarray:
    bits = np.asarray(bits, dtype=np.uint16)
    return (bits & np.uint16(0x7FFF)) > np.uint16(0x7F80)


def is_nan_f32(x: np.ndarray) -> np.ndarray:
    return (np.ascontiguousarray(x, dtype=np.float32).view(np.uint32) & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000)


def mismatches_bf16(got_bits: np.ndarray, want_bits: np.ndarray) -> int:
    """Elements where `got` is not `want`: a NaN is compared as "is NaN", everything else by its bits (so -0 is not +0)."""
    got, want = np.asarray(got_bits, dtype=np.uint16), np.asarray(want_bits, dtype=np.uint16)
    assert got.shape == want.shape
    gn, wn = is_nan_bf16(got), is_nan_bf16(want)
    return int(np.count_nonzero((gn != wn) | (~wn & (got != want))))


def mismatches_f32(got: np.ndarray, want: np.ndarray) -> int:
    """The same for float32 sums."""
    got, want = np.ascontiguousarray(got, dtype=np.float32), np.ascontiguousarray(want, dtype=np.float32)
    assert got.shape == want.shape
    gn, wn = is_nan_f32(got), is_nan_f32(want)
    return int(np.count_nonzero((gn != wn) | (~wn & (got.view(np.uint32) != want.view(np.uint32)))))


def mismatches(got_bits: np.ndarray, grads) -> int:
    """Elements of a window's bf16 result that are not the oracle's."""
    return mismatches_bf16(got_bits, window_total(grads))
