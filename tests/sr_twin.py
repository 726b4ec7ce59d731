"""numpy twin of the stochastic rounding of mi_adamw_sr_bf16_multi (include/mi_fp8.h): Philox4x32-10, the 16 bits of an element,
the rounding rule, and a model of ClippedAdamW(stochastic_rounding=True) on the CPU (fp32 arithmetic in the kernel's order)."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Counter words (arrays or ints) and key words -> the four output words as uint32 arrays."""
    c0, c1, c2, c3 = (np.atleast_1d(np.asarray(c, dtype=np.uint64)) & MASK for c in np.broadcast_arrays(c0, c1, c2, c3))
    k0, k1 = int(k0) & MASK, int(k1) & MASK
    for _ in range(10):
        p0, p1 = c0 * np.uint64(M0), c2 * np.uint64(M1)
        c0, c1, c2, c3 = ((p1 >> np.uint64(32)) ^ c1 ^ np.uint64(k0), p1 & np.uint64(MASK),
                          (p0 >> np.uint64(32)) ^ c3 ^ np.uint64(k1), p0 & np.uint64(MASK))
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return [c.astype(np.uint32) for c in (c0, c1, c2, c3)]


def sr_bits16(seed, step, key, stream, e):
    """The 16 random bits of the global element indices `e` (stream 0 weight, 1 exp_avg, 2 exp_avg_sq)."""
    e = np.asarray(e, dtype=np.uint64)
    v = e >> np.uint64(3)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    w = philox4x32_10(v & np.uint64(MASK), v >> np.uint64(32), int(step) & MASK, ((int(key) << 2) | int(stream)) & MASK,
                      seed & MASK, seed >> 32)
    j = (e & np.uint64(7)).astype(np.int64)
    word = np.choose(j >> 1, w)
    return ((word >> (16 * (j & 1)).astype(np.uint32)) & np.uint32(0xFFFF)).astype(np.uint32)


def rne_bf16_bits(x):
    """fp32 array -> bf16 bits, round to nearest even, NaN kept quiet (the conversion of the other kernels)."""
    b = np.asarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    r = ((b + np.uint64(0x7FFF) + ((b >> np.uint64(16)) & np.uint64(1))) >> np.uint64(16)).astype(np.uint32)
    nan = np.isnan(np.asarray(x, dtype=np.float32))
    return np.where(nan, ((b >> np.uint64(16)).astype(np.uint32) | np.uint32(0x40)), r).astype(np.uint16)


def sr_bf16_bits(x, r):
    """The rounding rule: finite fp32 x with bits b -> (b + r) >> 16; NaN and Inf as rne_bf16_bits."""
    x = np.asarray(x, dtype=np.float32)
    b = x.view(np.uint32).astype(np.uint64)
    out = ((b + np.asarray(r, dtype=np.uint64)) >> np.uint64(16)).astype(np.uint16)
    return np.where(np.isfinite(x), out, rne_bf16_bits(x)).astype(np.uint16)


def bf16_bits_to_f32(bits):
    return (np.asarray(bits, dtype=np.uint16).astype(np.uint32) << np.uint32(16)).view(np.float32)


def f32_to_bf16_bits_exact(x):
    """Bits of fp32 values that ARE bf16 values."""
    b = np.asarray(x, dtype=np.float32).view(np.uint32)
    assert not (b & np.uint32(0xFFFF)).any()
    return (b >> np.uint32(16)).astype(np.uint16)


def adam_f32(p, g, m, v, step, lr, betas, eps, weight_decay):
    """The kernels' fp32 step (adam_one in mi_optim.hip, operation for operation) on float32 arrays: unrounded p, m, v."""
    f = np.float32
    b1, b2 = f(betas[0]), f(betas[1])
    step_size = f(float(f(lr)) / (1.0 - float(b1) ** step))
    bc2_sqrt = f(np.sqrt(1.0 - float(b2) ** step))
    p = p * (f(1) - f(lr) * f(weight_decay))
    m = m + (f(1) - b1) * (g - m)
    v = b2 * v + (f(1) - b2) * g * g
    denom = np.sqrt(v) / bc2_sqrt + f(eps)
    p = p - step_size * (m / denom)
    return p.astype(f), m.astype(f), v.astype(f)


def model_step(pb, g, mb, vb, step, hp, seed=0, key=0, base=0, sr=True):
    """One step of the bf16-state optimiser on bf16 BITS (uint16 arrays); g float32.  sr=False: round to nearest even."""
    p, m, v = adam_f32(bf16_bits_to_f32(pb), np.asarray(g, dtype=np.float32), bf16_bits_to_f32(mb), bf16_bits_to_f32(vb), step,
                       hp["lr"], hp["betas"], hp["eps"], hp["weight_decay"])
    if not sr:
        return rne_bf16_bits(p), rne_bf16_bits(m), rne_bf16_bits(v)
    e = base + np.arange(p.size, dtype=np.uint64)
    return tuple(sr_bf16_bits(x, sr_bits16(seed, step, key, s, e)) for s, x in enumerate((p, m, v)))
