"""Plain numpy float64 references and acceptance criteria for the per-head QK RMSNorm fused into the RoPE split
(mi_qknorm_rope_qkv / mi_qknorm_rope_qkv_bwd, include/mi_fp8.h), the inputs the tests share, and numpy "kernels" that restate the
device arithmetic in float32 in the device's order -- right, or wrong in one named way -- with which tests/test_qknorm_oracle.py shows
on the CPU that every criterion accepts a right kernel and rejects a wrong one.  tests/test_qknorm_kernels_gpu.py holds the HIP kernels
to the same criteria.  No torch and no GPU in here.

The criteria have the form of glue_oracle.rounded_within: with e the float64 value of an element and delta a bound on the error of the
device's fp32 evaluation, lo = RNE_bf16(e - delta) <= got <= hi = RNE_bf16(e + delta).  delta is counted, not tuned.  u = 2^-24.
  rho = (D / 8 + 9) u   relative error of a head's rstd: a lane's D / 8 multiply-adds, 3 shuffle adds, then the division, the add of
                        eps and the rsqrt at 2 ulp each (the rsqrt figure is an assumption, as in glue_oracle.rstd_rtol)
  forward:  n = (x rstd) gamma, out1 = n1 c - n2 s, out2 = n2 c + n1 s:  delta = (6 u + rho) m + 2^-126,
            m = |n1 c| + |n2 s| resp. |n2 c| + |n1 s|   (x rstd, its product with gamma, the rotation's product and sum: 4 u and rho
            to first order; 2 u slack for the second order)
  dx:       dn = conjugate rotation, g = gamma dn, xhat = x rstd, dx = rstd (g - xhat mean_D(g xhat)):
            delta = ((11 + D / 8) u + 2 rho) m_dx + 2^-126,  m_dx = rstd (|gamma| m_dn + |xhat| mean_D(|gamma| m_dn |xhat|))
  gamma partial sums (fp32): |got - e| <= ((terms + 4) u + rho) sum m_dn |xhat|, `terms` the number of addends of the column.
On the CPU the float32 restatements below leave no element outside over QKNORM_CASES and the input scales 1e-3, 1, 30 and 2^-10.
The ambiguity caps (at most max(2, 0.5 %) of a forward tensor and max(2, 2.5 %) of a dx tensor may have lo != hi) are conditions,
not measurements; test_qknorm_oracle prints the counts (at most 0.23 % forward and 1.27 % for dx on those inputs)."""
import numpy as np

from tests import glue_oracle as G

U = 2.0 ** -24
EPS = 1e-6

# (B, S, n_q, n_kv, D, rows): rows = B * S except in the last case, whose last sequence is partial
QKNORM_CASES = [(1, 1, 1, 1, 64, 1), (3, 7, 3, 1, 64, 21), (2, 40, 5, 3, 128, 80), (1, 24, 4, 4, 128, 24), (2, 16, 8, 2, 128, 32),
                (3, 12, 2, 2, 64, 29)]
QKNORM_BIG_CASE = (4, 512, 32, 8, 128, 2048)  # GPU only: the 4B head counts, more than one pass of a capped grid
QKNORM_SCALES = (1e-3, 1.0, 30.0)


def rho(D: int) -> float:
    return (D / 8 + 9) * U


def qknorm_case_inputs(case, scale: float = 1.0):
    """The inputs of one case, the same on the CPU and on the device: bf16 patterns of scale * N(0, 1) for the fused forward input
    [rows, W], of N(0, 1) for dq / dk / dv, of 1 + 0.5 N(0, 1) for the two gammas [D] (never all ones: with a constant gamma the
    norm and the rotation commute and a norm applied after the rotation would go unseen), and glue_oracle's poisoned tables."""
    B, S, nq, nkv, D, rows = case
    rng = np.random.default_rng([B, S, nq, nkv, D, rows, 7])
    draw = lambda n, s=1.0: G.f32_to_bf16((rng.standard_normal((rows, n)) * s).astype(np.float32))
    cos, sin = G.rope_tables(S, D)
    qkv = draw((nq + 2 * nkv) * D, scale)
    gam = lambda: G.f32_to_bf16((1.0 + 0.5 * rng.standard_normal(D)).astype(np.float32))
    return dict(qkv=qkv, dq=draw(nq * D), dk=draw(nkv * D), dv=draw(nkv * D), gamma_q=gam(), gamma_k=gam(), cos=cos, sin=sin,
                eps=np.float32(EPS))


def _heads(bits, rows, n, D):
    return G.bf16_to_f64(bits).reshape(rows, n, D)


def _gamma64(inp, nq, nkv):
    """[nq + nkv, D] float64: gamma_q for the q heads, gamma_k for the k heads."""
    gq, gk = G.bf16_to_f64(inp["gamma_q"]), G.bf16_to_f64(inp["gamma_k"])
    return np.concatenate([np.repeat(gq[None], nq, 0), np.repeat(gk[None], nkv, 0)], axis=0)


def _tables64(inp, rows, S):
    pos = np.arange(rows) % S
    return (np.asarray(inp["cos"], dtype=np.float64)[pos][:, None, :], np.asarray(inp["sin"], dtype=np.float64)[pos][:, None, :])


def forward_ref(inp, case):
    """float64: dict(rstd [rows, nq + nkv], e / m [rows, (nq + nkv) D] -- the exact rotated values of the q then k heads and the
    magnitudes their rounding errors scale with -- and v, the bf16 patterns to be copied)."""
    B, S, nq, nkv, D, rows = case
    h = D // 2
    x = _heads(inp["qkv"][:, :(nq + nkv) * D], rows, nq + nkv, D)
    rstd = 1.0 / np.sqrt((x * x).mean(-1) + float(inp["eps"]))
    n = x * rstd[..., None] * _gamma64(inp, nq, nkv)[None]
    c, s = _tables64(inp, rows, S)
    n1, n2 = n[..., :h], n[..., h:]
    e = np.concatenate([n1 * c - n2 * s, n2 * c + n1 * s], axis=-1)
    m = np.concatenate([np.abs(n1 * c) + np.abs(n2 * s), np.abs(n2 * c) + np.abs(n1 * s)], axis=-1)
    return dict(rstd=rstd, e=e.reshape(rows, -1), m=m.reshape(rows, -1), v=np.asarray(inp["qkv"], dtype=np.uint16)[:, (nq + nkv) * D:])


def backward_ref(inp, case, rstd=None):
    """float64 backward with the given rstd [rows, nq + nkv] (default: forward_ref's): dict(dx / m_dx [rows, (nq + nkv) D], t / m_t
    [rows, nq + nkv, D] -- the addends dn * xhat of the gamma sums and their magnitudes m_dn |xhat| --, dv patterns)."""
    B, S, nq, nkv, D, rows = case
    h = D // 2
    if rstd is None:
        rstd = forward_ref(inp, case)["rstd"]
    rstd = np.asarray(rstd, dtype=np.float64)[..., None]
    x = _heads(inp["qkv"][:, :(nq + nkv) * D], rows, nq + nkv, D)
    d = np.concatenate([_heads(inp["dq"], rows, nq, D), _heads(inp["dk"], rows, nkv, D)], axis=1)
    c, s = _tables64(inp, rows, S)
    d1, d2 = d[..., :h], d[..., h:]
    dn = np.concatenate([d1 * c + d2 * s, d2 * c - d1 * s], axis=-1)
    m_dn = np.concatenate([np.abs(d1 * c) + np.abs(d2 * s), np.abs(d2 * c) + np.abs(d1 * s)], axis=-1)
    gam = _gamma64(inp, nq, nkv)[None]
    xh = x * rstd
    g = gam * dn
    dx = rstd * (g - xh * (g * xh).mean(-1, keepdims=True))
    m_dx = rstd * (np.abs(gam) * m_dn + np.abs(xh) * (np.abs(gam) * m_dn * np.abs(xh)).mean(-1, keepdims=True))
    return dict(dx=dx.reshape(rows, -1), m_dx=m_dx.reshape(rows, -1), t=dn * xh, m_t=m_dn * np.abs(xh), dv=np.asarray(inp["dv"], dtype=np.uint16))


def gamma_sums(ref_b, case, row_lo=0, row_hi=None):
    """(e, bound) [2 D]: the float64 sums of dn * xhat over rows [row_lo, row_hi) and all q heads (first D) resp. all k heads, and
    the bound ((terms + 4) u + rho) sum m_dn |xhat| on the error of an fp32 evaluation in any order."""
    B, S, nq, nkv, D, rows = case
    row_hi = rows if row_hi is None else row_hi
    t, m = ref_b["t"][row_lo:row_hi], ref_b["m_t"][row_lo:row_hi]
    n = max(row_hi - row_lo, 0)
    e = np.concatenate([t[:, :nq].sum((0, 1)), t[:, nq:].sum((0, 1))])
    mag = np.concatenate([m[:, :nq].sum((0, 1)), m[:, nq:].sum((0, 1))])
    terms = np.concatenate([np.full(D, n * nq), np.full(D, n * nkv)])
    return e, ((terms + 4) * U + rho(D)) * mag


def partial_rows(rows: int, n_partials: int):
    """[(lo, hi)] per workgroup: the rows it owns (hi <= lo: none)."""
    rpb = max(1, -(-rows // n_partials))
    return [(min(p * rpb, rows), min((p + 1) * rpb, rows)) for p in range(n_partials)]


# ------------------------------------------------------------------------------------------------ criteria
def within(got_bits, e, delta):
    """(ok, ambiguous) per element: glue_oracle.rounded_within with the caller's delta."""
    e = np.asarray(e, dtype=np.float64)
    got = G.bf16_to_f64(got_bits).reshape(e.shape)
    with np.errstate(invalid="ignore"):
        lo, hi = G.bf16_to_f64(G.rne_bf16(e - delta)), G.bf16_to_f64(G.rne_bf16(e + delta))
        inside = (lo <= got) & (got <= hi)
    e_nan, e_inf = np.isnan(e), np.isinf(e)
    ok = np.where(e_nan, np.isnan(got), np.where(e_inf, got == e, inside & np.isfinite(got)))
    return ok, ~e_nan & ~e_inf & (lo != hi)


def forward_delta(m, D):
    return (6 * U + rho(D)) * np.asarray(m, dtype=np.float64) + 2.0 ** -126


def dx_delta(m_dx, D):
    return ((11 + D / 8) * U + 2 * rho(D)) * np.asarray(m_dx, dtype=np.float64) + 2.0 ** -126


def forward_ok(got_bits, ref_f, D):
    return within(got_bits, ref_f["e"], forward_delta(ref_f["m"], D))


def dx_ok(got_bits, ref_b, D):
    return within(got_bits, ref_b["dx"], dx_delta(ref_b["m_dx"], D))


def rstd_ok(got_f32, ref_rstd, D) -> np.ndarray:
    ref = np.asarray(ref_rstd, dtype=np.float64)
    return np.abs(np.asarray(got_f32, dtype=np.float64).reshape(ref.shape) - ref) <= rho(D) * np.abs(ref)


def gamma_ok(got_f32, e, bound) -> np.ndarray:
    return np.abs(np.asarray(got_f32, dtype=np.float64).reshape(-1) - e) <= bound


def forward_ambiguity_cap(n: int) -> int:
    return max(2, int(0.005 * n))


def dx_ambiguity_cap(n: int) -> int:
    return max(2, int(0.025 * n))


# ------------------------------------------------------------------------------------------------ float32 restatements
FORWARD_MUTANTS = ("no_eps", "mean_half", "gamma_q_for_k", "norm_after_rope", "rstd_neighbour", "pos+1")


def _lane_sum(p, D):
    """p [rows, heads, D] float32 addends -> [rows, heads]: the device's order.  Lane vv of a head's D / 16 lanes adds the 8 addends
    of its first-half vector, then the 8 of its second-half vector; then a butterfly with offsets 1, 2, (4) over the lanes."""
    rows, H, _ = p.shape
    vph = D // 16
    p = p.reshape(rows, H, 2, vph, 8)
    acc = np.zeros((rows, H, vph), dtype=np.float32)
    for half in range(2):
        for j in range(8):
            acc = acc + p[:, :, half, :, j]
    o = 1
    while o < vph:
        acc = acc + acc[..., np.arange(vph) ^ o]
        o <<= 1
    return acc[..., 0]


def _rotate_f32(a, c, s):
    h = a.shape[-1] // 2
    a1, a2 = a[..., :h], a[..., h:]
    return np.concatenate([a1 * c - a2 * s, a2 * c + a1 * s], axis=-1).astype(np.float32)


def forward_kernel_f32(inp, case, mutant=None):
    """The forward in float32 in the device's order: (q, k, v bf16 patterns, rstd float32 [rows, nq + nkv]).  mutant: None, "no_eps"
    (eps left out), "mean_half" (the mean taken over D / 2), "gamma_q_for_k" (the k heads scaled by gamma_q), "norm_after_rope" (x
    rotated first, then normalised and scaled), "rstd_neighbour" (head i takes the rstd of head i + 1), "pos+1" (row r takes
    position r + 1)."""
    B, S, nq, nkv, D, rows = case
    H = nq + nkv
    x = G.bf16_to_f32(inp["qkv"][:, :H * D]).reshape(rows, H, D)
    gq, gk = G.bf16_to_f32(inp["gamma_q"]), G.bf16_to_f32(inp["gamma_k"])
    gam = np.concatenate([np.repeat(gq[None], nq, 0), np.repeat(gq[None] if mutant == "gamma_q_for_k" else gk[None], nkv, 0)], axis=0)[None]
    pos = (np.arange(rows) + (1 if mutant == "pos+1" else 0)) % S
    c = np.asarray(inp["cos"], dtype=np.float32)[pos][:, None, :]
    s = np.asarray(inp["sin"], dtype=np.float32)[pos][:, None, :]
    ss = _lane_sum((x * x).astype(np.float32), D)
    inv = np.float32(2.0 / D if mutant == "mean_half" else 1.0 / D)
    eps = np.float32(0.0) if mutant == "no_eps" else np.float32(inp["eps"])
    with np.errstate(divide="ignore"):
        rs = (np.float32(1) / np.sqrt(ss * inv + eps)).astype(np.float32)
    use = np.roll(rs, -1, axis=1) if mutant == "rstd_neighbour" else rs
    if mutant == "norm_after_rope":
        o = ((_rotate_f32(x, c, s) * use[..., None]).astype(np.float32) * gam).astype(np.float32)
    else:
        o = _rotate_f32(((x * use[..., None]).astype(np.float32) * gam).astype(np.float32), c, s)
    out = G.f32_to_bf16(o)
    return (out[:, :nq].reshape(rows, nq * D), out[:, nq:].reshape(rows, nkv * D),
            np.asarray(inp["qkv"], dtype=np.uint16)[:, H * D:].copy(), rs)


def backward_kernel_f32(inp, case, rstd, n_partials, mutant=None):
    """The backward in float32 in the device's order: (dfused bf16 patterns [rows, W], partials float32 [n_partials, 2 D]).  A
    workgroup of 256 lanes walks the items of its rows (item = one lane's 16 elements of a head, D / 16 items per head, heads in
    q | k order) 256 at a time; a lane adds its addends in walking order, then the lanes of a wave that hold the same columns are
    combined by a butterfly and the four waves in wave order.  mutant: None, "drop_block" (the rows of workgroup 1, or of
    workgroup 0 if there is only one, are missing from the gamma sums)."""
    B, S, nq, nkv, D, rows = case
    H, h, vph = nq + nkv, D // 2, D // 16
    rs = np.asarray(rstd, dtype=np.float32).reshape(rows, H)[..., None]
    x = G.bf16_to_f32(inp["qkv"][:, :H * D]).reshape(rows, H, D)
    d = np.concatenate([G.bf16_to_f32(inp["dq"]).reshape(rows, nq, D), G.bf16_to_f32(inp["dk"]).reshape(rows, nkv, D)], axis=1)
    gq, gk = G.bf16_to_f32(inp["gamma_q"]), G.bf16_to_f32(inp["gamma_k"])
    gam = np.concatenate([np.repeat(gq[None], nq, 0), np.repeat(gk[None], nkv, 0)], axis=0)[None]
    pos = np.arange(rows) % S
    c = np.asarray(inp["cos"], dtype=np.float32)[pos][:, None, :]
    s = np.asarray(inp["sin"], dtype=np.float32)[pos][:, None, :]
    d1, d2 = d[..., :h], d[..., h:]
    dn = np.concatenate([d1 * c + d2 * s, d2 * c - d1 * s], axis=-1).astype(np.float32)
    xh = (x * rs).astype(np.float32)
    g = (gam * dn).astype(np.float32)
    mean = (_lane_sum((g * xh).astype(np.float32), D) * np.float32(1.0 / D)).astype(np.float32)[..., None]
    dx = (rs * (g - (xh * mean).astype(np.float32)).astype(np.float32)).astype(np.float32)
    dfused = np.concatenate([G.f32_to_bf16(dx).reshape(rows, H * D), np.asarray(inp["dv"], dtype=np.uint16)], axis=1)
    # gamma partials
    t = (dn * xh).astype(np.float32).reshape(rows, H, 2, vph, 8)  # [row, head, half, lane of the head, element]
    per_row = (nq + 3 * nkv) * vph
    part = np.zeros((n_partials, 2 * D), dtype=np.float32)
    blocks = partial_rows(rows, n_partials)
    dropped = (1 if n_partials > 1 else 0) if mutant == "drop_block" else -1
    for p, (lo, hi) in enumerate(blocks):
        acc = np.zeros((256, 2, 2, 8), dtype=np.float32)  # [lane, q / k, half, element]
        if hi > lo and p != dropped:
            items = (hi - lo) * per_row
            for first in range(0, items, 256):
                it = np.arange(first, min(first + 256, items))
                r, w = lo + it // per_row, it % per_row
                rot = w < H * vph
                it, r, w = it[rot], r[rot], w[rot]
                hd, vv = w // vph, w % vph
                add = t[r, hd, :, vv, :]  # [n, half, 8]
                isk = (hd >= nq).astype(np.int64)
                acc[it % 256, isk] = acc[it % 256, isk] + add
        acc = acc.reshape(4, 64, 2, 2, 8)  # [wave, lane, ...]
        o = vph
        while o < 64:
            acc = acc + acc[:, np.arange(64) ^ o]
            o <<= 1
        tot = ((acc[0] + acc[1]) + acc[2]) + acc[3]  # [lane, q / k, half, 8]; lanes 0 .. vph - 1 hold the columns
        part[p] = tot[:vph].transpose(1, 2, 0, 3).reshape(2 * D)  # [q / k, half, vv, 8] = column order
    return dfused, part
