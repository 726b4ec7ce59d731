"""Plain numpy float64 references and acceptance criteria for the small HBM-bound kernels between the GEMMs (RoPE split / merge,
the embedding gradient, the column-sum finish, the RMSNorm statistics), the inputs the RoPE tests share, and numpy "kernels" that
restate the device arithmetic in float32 -- right, or wrong in one named way -- with which tests/test_glue_oracle.py shows on the
CPU that every criterion accepts a right kernel and rejects a wrong one.  tests/test_glue_kernels_gpu.py holds the HIP kernels to
the same criteria.  No torch and no GPU in here."""
import numpy as np

# ------------------------------------------------------------------------------------------------ bf16
BF16_NAN = np.uint16(0x7FC0)


def bf16_to_f64(bits) -> np.ndarray:
    """uint16 bf16 patterns -> float64 (exact)."""
    return (np.asarray(bits, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def rne_bf16(x) -> np.ndarray:
    """float64 -> bf16 patterns with ONE round-to-nearest-even, straight from float64 (never through float32: a double rounding
    would move values that sit just beside a bf16 tie).  bf16 = 8 significand bits over float32's exponent range: spacing
    2^(e - 7) for |x| in [2^e, 2^(e+1)), 2^-133 below 2^-126; 2^128 - 2^119 and above rounds to Inf.  NaN -> 0x7FC0."""
    x = np.asarray(x, dtype=np.float64)
    a = np.abs(x)
    fin = np.isfinite(x)
    _, ex = np.frexp(np.where(fin, a, 1.0))            # a = m * 2^ex, m in [0.5, 1): e = ex - 1
    quantum = np.ldexp(1.0, np.maximum(ex - 1, -126) - 7)
    with np.errstate(invalid="ignore", over="ignore"):
        r = np.rint(np.where(fin, a, 0.0) / quantum) * quantum   # rint rounds ties to even; both scalings are exact
        r = np.where(fin, r, a)
        r = np.where(r >= 2.0 ** 128, np.inf, r)
        f32 = np.copysign(r, x).astype(np.float32)               # exact: r is a bf16 value (or Inf / NaN)
    bits = (f32.view(np.uint32) >> 16).astype(np.uint16)
    return np.where(np.isnan(x), BF16_NAN, bits)


def f32_to_bf16(x) -> np.ndarray:
    """float32 -> bf16 patterns, RNE (one rounding: float32 -> float64 is exact)."""
    return rne_bf16(np.asarray(x, dtype=np.float32).astype(np.float64))


def bf16_to_f32(bits) -> np.ndarray:
    return (np.asarray(bits, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32)


def bf16_ulp(x) -> np.ndarray:
    """Spacing of bf16 at |x| (float64)."""
    _, ex = np.frexp(np.maximum(np.abs(np.asarray(x, dtype=np.float64)), 2.0 ** -126))
    return np.ldexp(1.0, ex - 1 - 7)


# ------------------------------------------------------------------------------------------------ RoPE
# (B, S, n_q, n_kv, D, rows): rows = B * S except in the last case, whose last sequence is partial (rows = 2 S + 5)
ROPE_CASES = [(1, 1, 1, 1, 16, 1), (3, 7, 3, 1, 32, 21), (2, 40, 5, 3, 64, 80), (1, 24, 4, 4, 128, 24), (2, 16, 2, 1, 256, 32),
              (3, 12, 2, 2, 64, 29)]
ROPE_TABLE_PAD = 3  # table rows at and past `seq`: NaN, never to be read


def rope_tables(S: int, D: int, poison: bool = True):
    """fp32 cos / sin [S + 3, D / 2] of the usual angles pos / 10000^(2 i / D); the last three rows NaN (poison) or the angles of
    positions S .. S + 2 (a finite wrong row for the CPU mutants)."""
    pos = np.arange(S + ROPE_TABLE_PAD, dtype=np.float64)[:, None]
    ang = pos / 10000.0 ** (np.arange(0, D, 2, dtype=np.float64) / D)[None, :]
    cos, sin = np.cos(ang).astype(np.float32), np.sin(ang).astype(np.float32)
    if poison:
        cos[S:], sin[S:] = np.nan, np.nan
    return cos, sin


def rope_case_inputs(case):
    """The inputs of one RoPE case, the same on the CPU and on the device: bf16 patterns of N(0, 1) values for the fused forward
    input [rows, W] and for the backward's dq [rows, n_q D], dk, dv [rows, n_kv D], and the poisoned tables."""
    B, S, nq, nkv, D, rows = case
    rng = np.random.default_rng([B, S, nq, nkv, D, rows])
    draw = lambda n: f32_to_bf16(rng.standard_normal((rows, n)).astype(np.float32))
    cos, sin = rope_tables(S, D)
    return dict(qkv=draw((nq + 2 * nkv) * D), dq=draw(nq * D), dk=draw(nkv * D), dv=draw(nkv * D), cos=cos, sin=sin)


def rope_ref(x_bits, cos, sin, S: int, D: int, backward: bool):
    """float64 rotation of x [rows, heads * D] (row r at position r % S) with the given fp32 tables: (e, m), the exact value of
    every element (e1 = x1 c - x2 s, e2 = x2 c + x1 s over the halves of a head, s negated for the backward) and the magnitude
    |x1 c| + |x2 s| resp. |x2 c| + |x1 s| its rounding errors scale with."""
    x = bf16_to_f64(x_bits)
    rows, width = x.shape
    h = D // 2
    pos = np.arange(rows) % S
    c = np.asarray(cos, dtype=np.float64)[pos][:, None, :]
    s = np.asarray(sin, dtype=np.float64)[pos][:, None, :] * (-1.0 if backward else 1.0)
    x = x.reshape(rows, width // D, D)
    x1, x2 = x[..., :h], x[..., h:]
    with np.errstate(invalid="ignore"):
        e = np.concatenate([x1 * c - x2 * s, x2 * c + x1 * s], axis=-1)
        m = np.concatenate([np.abs(x1 * c) + np.abs(x2 * s), np.abs(x2 * c) + np.abs(x1 * s)], axis=-1)
    return e.reshape(rows, width), m.reshape(rows, width)


def rounded_within(got_bits, e, m):
    """(ok, ambiguous) per element for a bf16 result of an fp32 evaluation of e whose error is at most
        delta = 3 * 2^-24 * m + 2^-126
    (two product roundings and one sum rounding in fp32 are at most 2 * 2^-24 * m to first order, any FMA contraction does
    better; the third unit is slack for the second-order terms; 2^-126 covers fp32's subnormal spacing).  With
    lo = RNE_bf16(e - delta), hi = RNE_bf16(e + delta) an element is ok when lo <= got <= hi as real numbers, got is NaN exactly
    where e is and +-Inf exactly where e is.  Elements with lo != hi are ambiguous: the criterion admits two bf16 values there, so
    the callers cap their number (rope_ambiguity_cap)."""
    e = np.asarray(e, dtype=np.float64)
    got = bf16_to_f64(got_bits)
    with np.errstate(invalid="ignore"):
        delta = 3.0 * 2.0 ** -24 * np.asarray(m, dtype=np.float64) + 2.0 ** -126
        lo, hi = bf16_to_f64(rne_bf16(e - delta)), bf16_to_f64(rne_bf16(e + delta))
        inside = (lo <= got) & (got <= hi)
    e_nan, e_inf = np.isnan(e), np.isinf(e)
    ok = np.where(e_nan, np.isnan(got), np.where(e_inf, got == e, inside & np.isfinite(got)))
    ambiguous = ~e_nan & ~e_inf & (lo != hi)
    return ok, ambiguous


def rope_ambiguity_cap(n: int) -> int:
    """At most max(2, 0.2 %) of a compared tensor may be ambiguous under rounded_within (measured for N(0, 1) inputs: 0.03 % at
    D = 128 / S = 512, 0.05 % at D = 64 / S = 40, none at D = 16 / S = 7)."""
    return max(2, int(0.002 * n))


def rope_kernel_f32(fused_bits, cos, sin, S, nq, nkv, D, mutant=None):
    """The forward split in float32 as the device evaluates it (two rounded products, one rounded sum, one RNE to bf16): q, k, v
    bf16 patterns.  mutant: None, "trunc" (truncation to bf16 instead of RNE), "pos+1" (row r takes position r + 1), "sin_lane"
    (the sign of sin flipped in one element of every eight), "row_seq" (position 0 reads table row S), "qk_swap" (the last q head
    and the first k head change places)."""
    x = bf16_to_f32(fused_bits)
    rows = x.shape[0]
    h = D // 2
    pos = np.arange(rows) % S
    if mutant == "pos+1":
        pos = (np.arange(rows) + 1) % S
    if mutant == "row_seq":
        pos = np.where(pos == 0, S, pos)
    c = np.asarray(cos, dtype=np.float32)[pos][:, None, :]
    s = np.asarray(sin, dtype=np.float32)[pos][:, None, :]
    if mutant == "sin_lane":
        s = s * np.where(np.arange(h) % 8 == 5, np.float32(-1), np.float32(1))[None, None, :]
    heads = x[:, :(nq + nkv) * D].reshape(rows, nq + nkv, D).copy()
    if mutant == "qk_swap":
        heads[:, [nq - 1, nq]] = heads[:, [nq, nq - 1]]
    x1, x2 = heads[..., :h], heads[..., h:]
    with np.errstate(invalid="ignore"):
        o = np.concatenate([x1 * c - x2 * s, x2 * c + x1 * s], axis=-1).astype(np.float32)
    if mutant == "trunc":
        out = (np.ascontiguousarray(o).view(np.uint32) >> 16).astype(np.uint16)
    else:
        out = f32_to_bf16(o)
    return (out[:, :nq].reshape(rows, nq * D), out[:, nq:].reshape(rows, nkv * D),
            np.asarray(fused_bits, dtype=np.uint16)[:, (nq + nkv) * D:].copy())


# ------------------------------------------------------------------------------------------------ embedding gradient
def embedding_grad_ref(grad_bits, dy_bits, ids, alpha, padding_idx: int):
    """(float64 grad[id] + alpha * sum of the rows of dy whose id it is, mask of the rows touched); ids outside [0, V) and
    padding_idx are skipped.  alpha is the float32 the kernel receives."""
    out = bf16_to_f64(grad_bits).copy()
    V = out.shape[0]
    dy = bf16_to_f64(dy_bits)
    ids = np.asarray(ids, dtype=np.int64).reshape(-1)
    keep = (ids >= 0) & (ids < V) & (ids != padding_idx)
    acc = np.zeros_like(out)
    np.add.at(acc, ids[keep], dy[keep])
    touched = np.zeros(V, dtype=bool)
    touched[ids[keep]] = True
    out[touched] += float(np.float32(alpha)) * acc[touched]
    return out, touched


def embedding_exact_ok(got_bits, ref64) -> np.ndarray:
    """Integer inputs (|v| <= 8) and alpha in {1, 0.5, -2, 0}: every fp32 partial sum is an exact integer below 2^24 and alpha times
    it is exact, so whatever the order the result is RNE_bf16 of the exact value: bit equality."""
    return np.asarray(got_bits, dtype=np.uint16) == rne_bf16(ref64)


def embedding_ulp_ok(got_bits, ref64) -> np.ndarray:
    """Random inputs: within one bf16 ulp (at the larger of the two magnitudes) of the float64 value."""
    got = bf16_to_f64(got_bits)
    return np.abs(got - ref64) <= bf16_ulp(np.maximum(np.abs(got), np.abs(ref64)))


def embedding_kernel_f32(grad_bits, dy_bits, ids, alpha, padding_idx, mutant=None):
    """The device walk in float32: per id the rows of its run added in token order, then grad + alpha * acc and one RNE.  mutant:
    None, "lap2" (columns from 2048 on -- a lane's second lap -- are not updated), "padding" (padding_idx is not skipped),
    "last_token" (the last token of every run is dropped)."""
    out = np.asarray(grad_bits, dtype=np.uint16).copy()
    V, H = out.shape
    dy = bf16_to_f32(dy_bits)
    ids = np.asarray(ids, dtype=np.int64).reshape(-1)
    order = np.argsort(ids, kind="stable")
    a = np.float32(alpha)
    hi_col = min(H, 2048) if mutant == "lap2" else H
    for i in np.unique(ids):
        if i < 0 or i >= V or (i == padding_idx and mutant != "padding"):
            continue
        run = order[ids[order] == i]
        if mutant == "last_token":
            run = run[:-1]
        acc = np.zeros(H, dtype=np.float32)
        for t in run:
            acc += dy[t]
        new = f32_to_bf16(bf16_to_f32(out[i]) + a * acc)
        out[i, :hi_col] = new[:hi_col]
    return out


# ------------------------------------------------------------------------------------------------ column-sum finish
def colsum_ref(part):
    """(float64 column sums, float64 column sums of |part|) of fp32 partials [P, C]."""
    p = np.asarray(part, dtype=np.float64)
    return p.sum(0), np.abs(p).sum(0)


def colsum_f32_ok(got_f32, part) -> np.ndarray:
    """fp32 output: |got - ref| <= (P / 8 + 16) * 2^-24 * sum_p |part[p, c]|.  The kernel adds a column in 8 row groups of 4 chains:
    at most P / 8 sequential adds in a chain, then 3 adds to combine the chains and 8 for the groups; each add rounds a partial sum
    that is at most sum |part| by at most 2^-24 of it, so (P / 8 + 11) units bound any such order and 16 leaves 5 to spare.  One
    dropped or doubled row is an error of |part[p, c]| ~ sum |part| / P: 100 times the bound or more for every P used."""
    ref, mag = colsum_ref(part)
    P = np.asarray(part).shape[0]
    return np.abs(np.asarray(got_f32, dtype=np.float64) - ref) <= (P / 8 + 16) * 2.0 ** -24 * mag


def colsum_kernel_f32(part, mutant=None):
    """The finish in float32 in the kernel's order (row group py takes rows py, py + 8, ..: four chains while 32 rows remain, one
    after that).  mutant: None, "drop_last" (the last partial row), "double" (row 0 twice), "skip_col" (column C - 1 stays 0)."""
    part = np.asarray(part, dtype=np.float32)
    if mutant == "drop_last":
        part = part[:-1]
    if mutant == "double":
        part = np.concatenate([part, part[:1]], axis=0)
    P, C = part.shape
    groups = []
    for py in range(8):
        a = [np.zeros(C, dtype=np.float32) for _ in range(4)]
        p = py
        while p + 24 < P:
            for u in range(4):
                a[u] = a[u] + part[p + 8 * u]
            p += 32
        while p < P:
            a[0] = a[0] + part[p]
            p += 8
        groups.append((a[0] + a[1]) + (a[2] + a[3]))
    out = np.zeros(C, dtype=np.float32)
    for g in groups:
        out = out + g
    if mutant == "skip_col":
        out[C - 1] = 0
    return out


# ------------------------------------------------------------------------------------------------ RMSNorm statistics
def add_ref(a_bits, b_bits, bias_bits=None) -> np.ndarray:
    """bf16(f32(a) + f32(b)), with a bias bf16(f32(a) + (f32(b) + f32(bias))): float32 adds cannot contract, so this is the
    definition of `out`, bit for bit."""
    a, b = bf16_to_f32(a_bits), bf16_to_f32(b_bits)
    with np.errstate(over="ignore", invalid="ignore"):
        if bias_bits is not None:
            b = (b + bf16_to_f32(bias_bits)[None, :]).astype(np.float32)
        return f32_to_bf16((a + b).astype(np.float32))


def rstd_ref(x_bits, eps) -> np.ndarray:
    """float64 1 / sqrt(mean_c x^2 + eps) per row; eps is the float32 the kernel receives.  A row with an Inf gives 0, a NaN row
    NaN, a zero row under eps = 0 Inf, as IEEE arithmetic does."""
    x = bf16_to_f64(x_bits)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        return 1.0 / np.sqrt((x * x).sum(1) / x.shape[1] + float(np.float32(eps)))


def rstd_rtol(cols: int) -> float:
    """(cols / 64 + 16) * 2^-24: a lane adds cols / 512 vectors of 8 squares, cols / 64 multiply-add steps in its chain; 6 shuffle
    adds; the division, the add of eps and the rsqrt at 2 ulp each (the rsqrt figure is an assumption)."""
    return (cols / 64 + 16) * 2.0 ** -24


def rstd_ok(got_f32, x_bits, eps) -> np.ndarray:
    ref = rstd_ref(x_bits, eps)
    got = np.asarray(got_f32, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        close = np.abs(got - ref) <= rstd_rtol(np.asarray(x_bits).shape[1]) * np.abs(ref)
    return np.where(np.isfinite(ref), close, (got == ref) | (np.isnan(got) & np.isnan(ref)))


def rstd_kernel_f32(x_bits, eps, mutant=None):
    """The statistics pass in float32 in the kernel's order (lane l takes the 8-element vectors l, l + 64, ..; a butterfly over the
    64 lanes).  mutant: None, "skip_last_vec" (the last vector of a row), "mean_cols+8" (the mean taken over cols + 8)."""
    x = bf16_to_f32(x_bits)
    rows, cols = x.shape
    nvec = cols // 8 - (1 if mutant == "skip_last_vec" else 0)
    acc = np.zeros((rows, 64), dtype=np.float32)
    for v in range(nvec):
        xv = x[:, 8 * v:8 * v + 8]
        for j in range(4):
            acc[:, v % 64] = acc[:, v % 64] + ((xv[:, 2 * j] * xv[:, 2 * j]) + (xv[:, 2 * j + 1] * xv[:, 2 * j + 1]))
    o = 32
    while o >= 1:
        acc = acc + acc[:, np.arange(64) ^ o]
        o >>= 1
    n = np.float32(cols + (8 if mutant == "mean_cols+8" else 0))
    with np.errstate(divide="ignore"):
        return (np.float32(1) / np.sqrt(acc[:, 0] / n + np.float32(eps))).astype(np.float32)
