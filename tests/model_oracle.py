"""Float64 emulation of one decoder layer (Llama, Qwen3), the causal-LM head and the embedding gradient, forward and the
hand-written backward, in the arithmetic include/mi_fp8.h states -- TEST INFRASTRUCTURE.  numpy on the CPU; every FP8 / E8M0 / bf16
code comes from oracle/fp8_oracle.py, tests/block_oracle.py and tests/glue_oracle.py (no encoder of its own).

A segment is fed the bf16 values that crossed its boundaries in a real run (teacher forcing), so FP8 rounding decisions that flip do
not feed a second GEMM chain.  A decoder layer can be forced in the middle as well (the residual sum h1 between its attention and MLP
halves and the gradient of h1): each half is then two GEMMs deep.

Where a bf16 rounding sits (`rnd`), fused route (hidden % 512 == 0: llama.TELlamaDecoderLayer.route == "fused"):

  forward   x (bf16 in) -> rstd fp32 -> (x rstd) gamma                     fp32, quantised directly        mi_norm_cast
            q|k|v GEMM                                                     rnd                             GEMM epilogue
            [per-head RMSNorm ->] RoPE                                     rnd once at the store           mi_(qknorm_)rope_qkv
            attention output                                               rnd                             mi_attn_fwd
            o_proj GEMM                                                    rnd
            x + attn                                                       rnd (rstd of the ROUNDED sum)   mi_add_rmsnorm_stats
            fc1 GEMM                                                       rnd  (bias: see below)
            silu(g) u                                                      fp32, quantised directly        mi_swiglu_cast(_bias)
            fc2 GEMM, no bias                                              rnd
            h + (fc2 + b2)                                                 rnd                             mi_add_bias_rmsnorm_stats
  backward  column sums of dy (fc2 bias)                                   fp32 sum, rnd                   mi_cast_amax_colsum + finish
            every dgrad / wgrad GEMM                                       rnd
            dSwiGLU and its column sums (fc1 bias)                         fp32, quantised directly; rnd of the sums
            RMSNorm backward + residual gradient                           rnd once, dgamma: fp32 sum, rnd mi_rmsnorm_bwd
            attention dq, dk, dv (K/V: heads of a group summed in fp32)    rnd                             mi_attn_bwd
            conjugate RoPE [+ QK-norm backward], head_dim 64 or QK norm    rnd                             mi_(qknorm_)rope_qkv_bwd
  head      final norm as the decoder norms; logits                        rnd
            loss                                                           fp32
            d(logits): delayed scaling                                     fp32, quantised directly        mi_ce_backward_cast
                       every other recipe                                  rnd, then quantised             mi_ce_backward
  embedding rnd(lm_head wgrad) + sum of the rows                           rnd                             mi_embedding_grad_add

fc1 bias: per-tensor recipes (delayed, current) add it in fp32 inside the SwiGLU kernels to the ROUNDED GEMM output; block-scaled
recipes (mxfp8, block) keep it in the GEMM epilogue, in front of the rounding (`Quantiser.swiglu_adds_bias`).

Unfused-norm route (`fused=False`: a hidden size the fused norm kernels do not take, module._can_fuse_norm): the normalised activation
is a bf16 tensor (one rnd) that the Linear quantises; the fc2 bias sits in the GEMM epilogue; in backward the norm's input gradient is
a bf16 tensor to which autograd adds the residual gradient (two rnd instead of one).

Arithmetic modes (`Arith`): f64 -- everything between the roundings in float64; twin(seed) -- every GEMM, attention product, softmax
and row / column reduction in float32 with the contraction order permuted by `seed`: the freedom a device has (fp32 accumulation in
some order), with identical quantisers, roundings and inputs -- plus the one rounding the device makes where it stores no tensor:
the attention kernels' bf16 MFMA operands P and dS (Arith.mfma)."""
import numpy as np

from oracle import fp8_oracle as O
from tests import block_oracle as BO
from tests import glue_oracle as G

E4M3, E5M2 = O.E4M3, O.E5M2


def rb(x):
    """One round-to-nearest-even to bf16, straight from float64."""
    return G.bf16_to_f64(G.rne_bf16(x))


def ident(x):
    return np.asarray(x, dtype=np.float64)


# ------------------------------------------------------------------------------------------------ arithmetic modes
class Arith:
    """seed None: float64.  Otherwise the twin: float32 with the contraction order permuted, deterministic per seed."""

    def __init__(self, seed=None):
        self.seed, self.n = seed, 0

    def _perm(self, k):
        self.n += 1
        return np.random.default_rng([self.seed, self.n]).permutation(k)

    def mm(self, a, b):
        """a [..., M, K] @ b [..., K, N]"""
        if self.seed is None:
            return a @ b
        p = self._perm(a.shape[-1])
        return (a[..., p].astype(np.float32) @ np.take(b, p, axis=-2).astype(np.float32)).astype(np.float64)

    def sum(self, x, axis):
        if self.seed is None:
            return x.sum(axis)
        p = self._perm(x.shape[axis])
        return np.take(x, p, axis=axis).astype(np.float32).sum(axis, dtype=np.float32).astype(np.float64)

    def f(self, x):
        """A value a kernel holds in fp32 after a transcendental or a reduction (rstd, exp): rounded to float32 in the twin."""
        return x if self.seed is None else np.asarray(x).astype(np.float32).astype(np.float64)


    def mfma(self, x):
        """An operand the attention kernels hand to a bf16 MFMA from registers (P in the forward, P and dS in the backward:
        mi_attn.hip packs the fp32 accumulators to bf16 pairs).  No bf16 TENSOR is stored there, so the float64 mode keeps the
        value; the twin rounds it, as the device does -- measured on the MI355X, this rounding (2^-9 per element of P) moves the
        attention output by 1e-3 and, through the FP8 decisions it flips in the o_proj, fc1 and fc2 inputs, the layer's other
        tensors by up to 2e-2: more than fp32 accumulation order does."""
        return x if self.seed is None else rb(x)


F64 = Arith()


def twin(seed):
    return Arith(seed)


# ------------------------------------------------------------------------------------------------ quantisers
class Operand:
    """A quantised GEMM operand [R, C]: `row` = the values of the copy contracted along C, `col` = of the copy contracted along R
    (both in the tensor's own orientation, float64, exact), `alpha` = the float32 scale-inverse of a per-tensor scale (else 1)."""
    __slots__ = ("row", "col", "alpha")

    def __init__(self, row, col, alpha=np.float32(1.0)):
        self.row, self.col, self.alpha = row, col, np.float32(alpha)


def _f32(v):
    with np.errstate(over="ignore", invalid="ignore"):
        return np.ascontiguousarray(np.asarray(v, dtype=np.float64).astype(np.float32))


class Quantiser:
    swiglu_adds_bias = True   # the fc1 bias is added inside the SwiGLU kernels (per-tensor recipes)
    ce_handoff = False        # cross-entropy backward emits the head's FP8 grad_output from fp32 (delayed scaling)

    def __init__(self, fmt_f=E4M3, fmt_b=E5M2):
        self.fmt_f, self.fmt_b = fmt_f, fmt_b
        self._weights = {}

    def fmt(self, role):
        return self.fmt_b if role == "grad" else self.fmt_f

    def quant(self, v, role, key):
        """role: "x" (a GEMM's input) | "w" (its weight) | "grad" (its grad_output); key: the slot's name ("fc1.x", ...).  A weight
        is quantised once per quantiser object, key and array: its bits do not depend on the arithmetic mode."""
        if role != "w":
            return self._quant(v, role, key)
        hit = self._weights.get(key)
        if hit is None or hit[0] is not v:
            hit = self._weights[key] = (v, self._quant(v, role, key))
        return hit[1]

    def _quant(self, v, role, key):
        raise NotImplementedError


class IdentityQ(Quantiser):
    """No quantisation (with `rnd = ident`: the exact function the hand-written backward differentiates)."""

    def _quant(self, v, role, key):
        v = np.asarray(v, dtype=np.float64)
        return Operand(v, v)


def per_tensor_bytes(v, scale, fmt):
    """FP8 bytes of sat_cast(fl32(v) * scale): O.quantize_delayed for values that are not bf16."""
    with np.errstate(over="ignore", invalid="ignore"):
        return O.fp8_encode_sat(_f32(v) * np.float32(scale), fmt)


def _per_tensor(v, scale, fmt):
    d = O.fp8_decode(per_tensor_bytes(v, scale, fmt), fmt).astype(np.float64)
    return Operand(d, d, np.float32(1.0) / np.float32(scale))


class DelayedQ(Quantiser):
    """Delayed scaling: the scale of every slot is an input (`scales[key]`, float32, read from the device before the pass);
    `amax[key]` collects what each slot's cast would publish."""
    ce_handoff = True

    def __init__(self, scales, fmt_f=E4M3, fmt_b=E5M2):
        super().__init__(fmt_f, fmt_b)
        self.scales, self.amax = scales, {}

    def _quant(self, v, role, key):
        self.amax[key] = O.amax_f32(_f32(v))
        return _per_tensor(v, self.scales[key], self.fmt(role))


def current_scale(amax, fmt):
    """Float8CurrentScaling's default QParams (amax_epsilon 0, no power-of-two forcing): fl32(fp8_max / amax), Inf -> FLT_MAX, 1
    for an amax of 0 or Inf: block_oracle.scale_from_amax without the mantissa clearing."""
    a = np.float32(amax)
    q = BO.scale_quotient(a, fmt)
    q = np.where(np.isinf(q), np.float32(O.FLT_MAX), q)
    return np.float32(np.where((a == 0) | np.isinf(a), np.float32(1.0), q))


class CurrentQ(Quantiser):
    def _quant(self, v, role, key):
        fmt = self.fmt(role)
        return _per_tensor(v, current_scale(O.amax_f32(_f32(v)), fmt), fmt)


def mx_codes(v32, fmt):
    """(FP8 bytes [R, C], E8M0 bytes [R, C / 32]) of float32 values: O.mxfp8_quantize_rowwise for values that are not bf16."""
    v32 = np.ascontiguousarray(v32, dtype=np.float32)
    r, c = v32.shape
    e = O.float_to_e8m0_roundup((O.mx_block_amax(v32) * O._MAX_NORM_RCP[fmt]).astype(np.float32))
    with np.errstate(over="ignore", invalid="ignore"):
        inv = np.ldexp(np.float32(1.0), 127 - e.astype(np.int64)).astype(np.float32)
        y = (v32.reshape(r, c // O.MX_BLOCK, O.MX_BLOCK) * inv[:, :, None]).astype(np.float32)
    return O.fp8_encode_sat(y, fmt).reshape(r, c), e


def _mx_values(v32, fmt):
    y, e = mx_codes(v32, fmt)
    return O.fp8_decode(y, fmt).astype(np.float64) * np.repeat(O.e8m0_to_f32(e).astype(np.float64), O.MX_BLOCK, axis=1)


class MXQ(Quantiser):
    """MXFP8: the row-wise copy has its 32-blocks along the last axis, the column-wise copy along the first (quantised separately)."""
    swiglu_adds_bias = False

    def __init__(self, fmt_f=E4M3, fmt_b=E4M3):
        super().__init__(fmt_f, fmt_b)

    def _quant(self, v, role, key):
        v32, fmt = _f32(v), self.fmt(role)
        return Operand(_mx_values(v32, fmt), _mx_values(np.ascontiguousarray(v32.T), fmt).T)


class BlockQ(Quantiser):
    """Float8BlockScaling(): 1 x 128 blocks for activations and gradients, 128 x 128 for weights (block_oracle.quantize_values)."""
    swiglu_adds_bias = False
    DIM = {"x": 1, "w": 2, "grad": 1}

    def __init__(self, fmt_f=E4M3, fmt_b=E4M3):
        super().__init__(fmt_f, fmt_b)

    def _quant(self, v, role, key):
        fmt = self.fmt(role)
        y_row, s_row, y_colT, s_colT = BO.quantize_values(_f32(v), fmt, self.DIM[role])
        return Operand(BO.dequantize(y_row, s_row, fmt), BO.dequantize(y_colT, s_colT, fmt).T)


def gemm(ar, a_vals, b_vals_t, alpha_a, alpha_b):
    """a [M, K] . b^T with b given as [N, K]; alpha = one float32 product, as in the GEMM epilogue."""
    return ar.mm(a_vals, b_vals_t.T) * np.float64(np.float32(alpha_a) * np.float32(alpha_b))


def fwd_gemm(ar, x: Operand, w: Operand):       # y [M, N] = x [M, K] . w [N, K]^T
    return gemm(ar, x.row, w.row, x.alpha, w.alpha)


def dgrad_gemm(ar, g: Operand, w: Operand):     # dx [M, K] = g [M, N] . w [N, K]   (contraction along N: w's column-wise copy)
    return ar.mm(g.row, w.col) * np.float64(g.alpha * w.alpha)


def wgrad_gemm(ar, g: Operand, x: Operand):     # dw [N, K] = g [M, N]^T . x [M, K] (contraction along M: both column-wise copies)
    return ar.mm(g.col.T, x.col) * np.float64(g.alpha * x.alpha)


# ------------------------------------------------------------------------------------------------ pieces
def _rstd(ar, x, eps):
    return ar.f(1.0 / np.sqrt(ar.sum(x * x, -1) / x.shape[-1] + eps))


def _norm_bwd(ar, dy, x, rstd, gamma):
    """(dx, dgamma) of y = (x rstd) gamma: O.rmsnorm_bwd_f32's formulas with the given rstd."""
    xh = x * rstd[..., None]
    wdy = dy * gamma
    c = ar.sum(wdy * xh, -1) / x.shape[-1]
    return rstd[..., None] * (wdy - xh * c[..., None]), dy * xh


def _rotate(n, c, s, conj=False):
    h = n.shape[-1] // 2
    n1, n2 = n[..., :h], n[..., h:]
    if conj:
        return np.concatenate([n1 * c + n2 * s, n2 * c - n1 * s], axis=-1)
    return np.concatenate([n1 * c - n2 * s, n2 * c + n1 * s], axis=-1)


def _sigmoid(g):
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-g))


class Config:
    """Shapes and constants of one model: B, S (tokens = B S, row r at position r % S), n_q / n_kv heads of D, eps of the decoder
    norms, qk_norm (Qwen3; its eps is `eps` too), cos / sin [>= S, D / 2] (the fp32 tables the device reads), `fused` route, and
    `rnd` (rb, or ident for the exact function)."""

    def __init__(self, B, S, n_q, n_kv, D, eps, cos, sin, qk_norm=False, fused=True, rnd=rb):
        self.B, self.S, self.n_q, self.n_kv, self.D, self.eps, self.qk_norm, self.fused, self.rnd = B, S, n_q, n_kv, D, eps, qk_norm, fused, rnd
        pos = np.arange(B * S) % S
        self.c = np.asarray(cos, dtype=np.float64)[pos][:, None, :]
        self.s = np.asarray(sin, dtype=np.float64)[pos][:, None, :]


LAYER_PARAMS = ("ln1", "wq", "wk", "wv", "wo", "ln2", "w1", "b1", "w2", "b2")  # + "gq", "gk" under qk_norm


# ------------------------------------------------------------------------------------------------ decoder layer
def layer_forward(p, x, cfg: Config, q_attn: Quantiser, q_mlp: Quantiser, ar: Arith = F64, h1=None):
    """p: float64 parameters (LAYER_PARAMS; w1 = gate | up stacked, b1 likewise), x [T, H] -> (out [T, H], cache).
    `h1` (teacher forcing inside the layer): the recorded sum x + attention that the MLP half is fed instead of the emulation's own,
    which stays in cache["h1_own"] for the comparison -- each half is then two GEMMs deep."""
    rnd, T = cfg.rnd, x.shape[0]
    nq, nkv, D, B, S = cfg.n_q, cfg.n_kv, cfg.D, cfg.B, cfg.S
    k = {"x": x}
    # input norm -> q|k|v
    k["rstd1"] = _rstd(ar, x, cfg.eps)
    xn = x * k["rstd1"][:, None] * p["ln1"]
    k["Xq"] = q_attn.quant(xn if cfg.fused else rnd(xn), "x", "qkv.x")
    if "_wqkv" not in p:   # one GEMM operand (kept on the dict: the quantisers recognise a weight they have seen by identity)
        p["_wqkv"] = np.concatenate([p["wq"], p["wk"], p["wv"]], 0)
    k["Wqkv"] = q_attn.quant(p["_wqkv"], "w", "qkv.w")
    qkv = rnd(fwd_gemm(ar, k["Xq"], k["Wqkv"]))
    # split, per-head norm, rotation
    heads = qkv[:, :(nq + nkv) * D].reshape(T, nq + nkv, D)
    k["heads"] = heads
    n = heads
    if cfg.qk_norm:
        k["rstd_h"] = _rstd(ar, heads, cfg.eps)
        k["gam_h"] = np.concatenate([np.repeat(p["gq"][None], nq, 0), np.repeat(p["gk"][None], nkv, 0)], 0)
        n = heads * k["rstd_h"][..., None] * k["gam_h"][None]
    rot = rnd(_rotate(n, cfg.c, cfg.s))
    q = rot[:, :nq].reshape(B, S, nq, D)
    kk = rot[:, nq:].reshape(B, S, nkv, D)
    v = qkv[:, (nq + nkv) * D:].reshape(B, S, nkv, D)
    k["q"], k["k"], k["v"] = q, kk, v
    # causal GQA attention
    scale = D ** -0.5
    rep = nq // nkv
    qh = q.transpose(0, 2, 1, 3)                                   # [B, nq, S, D]
    kh = np.repeat(kk.transpose(0, 2, 1, 3), rep, axis=1)
    vh = np.repeat(v.transpose(0, 2, 1, 3), rep, axis=1)
    sc = ar.mm(qh, kh.transpose(0, 1, 3, 2)) * scale
    sc = np.where(np.triu(np.ones((S, S), dtype=bool), 1)[None, None], -np.inf, sc)
    m = sc.max(-1, keepdims=True)
    pe = ar.f(np.exp(sc - m))
    l = ar.sum(pe, -1)[..., None]
    k["lse"] = m + np.log(l)
    o = rnd(ar.mm(ar.mfma(pe), vh) / l).transpose(0, 2, 1, 3)      # [B, S, nq, D]
    k["o"] = o
    # o_proj, residual
    k["Oq"] = q_attn.quant(o.reshape(T, nq * D), "x", "proj.x")
    k["Wo"] = q_attn.quant(p["wo"], "w", "proj.w")
    attn = rnd(fwd_gemm(ar, k["Oq"], k["Wo"]))
    k["h1_own"] = rnd(x + attn)
    h1 = k["h1_own"] if h1 is None else h1
    k["h1"] = h1
    # MLP
    k["rstd2"] = _rstd(ar, h1, cfg.eps)
    xn2 = h1 * k["rstd2"][:, None] * p["ln2"]
    k["X1"] = q_mlp.quant(xn2 if cfg.fused else rnd(xn2), "x", "fc1.x")
    k["W1"] = q_mlp.quant(p["w1"], "w", "fc1.w")
    acc = fwd_gemm(ar, k["X1"], k["W1"])
    hb = rnd(acc) + p["b1"] if q_mlp.swiglu_adds_bias else rnd(acc + p["b1"])
    k["hb"] = hb
    F = hb.shape[1] // 2
    g, u = hb[:, :F], hb[:, F:]
    act = g * _sigmoid(g) * u
    k["A"] = q_mlp.quant(act, "x", "fc2.x")
    k["W2"] = q_mlp.quant(p["w2"], "w", "fc2.w")
    acc2 = fwd_gemm(ar, k["A"], k["W2"])
    out = rnd(h1 + (rnd(acc2) + p["b2"])) if cfg.fused else rnd(h1 + rnd(acc2 + p["b2"]))
    return out, k


def layer_backward(p, k, dout, cfg: Config, q_attn: Quantiser, q_mlp: Quantiser, ar: Arith = F64, dh1=None):
    """-> (dx [T, H], {parameter name: gradient}).  `dh1`: the recorded gradient of h1, fed to the attention half instead of the
    emulation's own, which is returned as gradient "dh1_own"."""
    rnd, T = cfg.rnd, dout.shape[0]
    nq, nkv, D, B, S = cfg.n_q, cfg.n_kv, cfg.D, cfg.B, cfg.S
    gr = {}
    # fc2
    G2 = q_mlp.quant(dout, "grad", "fc2.grad")
    gr["b2"] = rnd(ar.sum(dout, 0))
    dact = rnd(dgrad_gemm(ar, G2, k["W2"]))
    gr["w2"] = rnd(wgrad_gemm(ar, G2, k["A"]))
    # dSwiGLU, fc1
    hb = k["hb"]
    F = hb.shape[1] // 2
    g, u = hb[:, :F], hb[:, F:]
    sg = _sigmoid(g)
    dh = np.concatenate([dact * u * (sg * (1.0 + g * (1.0 - sg))), dact * (g * sg)], axis=1)
    gr["b1"] = rnd(ar.sum(dh, 0))
    G1 = q_mlp.quant(dh, "grad", "fc1.grad")
    dxn2 = rnd(dgrad_gemm(ar, G1, k["W1"]))
    gr["w1"] = rnd(wgrad_gemm(ar, G1, k["X1"]))
    dn, t = _norm_bwd(ar, dxn2, k["h1"], k["rstd2"], p["ln2"])
    gr["ln2"] = rnd(ar.sum(t, 0))
    gr["dh1_own"] = rnd(dn + dout) if cfg.fused else rnd(rnd(dn) + dout)
    dh1 = gr["dh1_own"] if dh1 is None else dh1
    # o_proj
    Gp = q_attn.quant(dh1, "grad", "proj.grad")
    do = rnd(dgrad_gemm(ar, Gp, k["Wo"])).reshape(B, S, nq, D)
    gr["wo"] = rnd(wgrad_gemm(ar, Gp, k["Oq"]))
    # attention backward: P from the stored log-sum-exp, delta = rowsum(dO * O) of the stored (rounded) O
    scale = D ** -0.5
    rep = nq // nkv
    qh = k["q"].transpose(0, 2, 1, 3)
    kh = np.repeat(k["k"].transpose(0, 2, 1, 3), rep, axis=1)
    vh = np.repeat(k["v"].transpose(0, 2, 1, 3), rep, axis=1)
    doh = do.transpose(0, 2, 1, 3)
    oh = k["o"].transpose(0, 2, 1, 3)
    sc = ar.mm(qh, kh.transpose(0, 1, 3, 2)) * scale
    sc = np.where(np.triu(np.ones((S, S), dtype=bool), 1)[None, None], -np.inf, sc)
    pr = ar.f(np.exp(sc - k["lse"]))
    dvh = ar.mm(ar.mfma(pr).transpose(0, 1, 3, 2), doh)
    dp = ar.mm(doh, vh.transpose(0, 1, 3, 2))
    delta = ar.sum(doh * oh, -1)[..., None]
    ds = ar.mfma(pr * (dp - delta) * scale)
    dqh = ar.mm(ds, kh)
    dkh = ar.mm(ds.transpose(0, 1, 3, 2), qh)
    dq = rnd(dqh).transpose(0, 2, 1, 3).reshape(T, nq, D)
    dk = rnd(dkh.reshape(B, nkv, rep, S, D).sum(2)).transpose(0, 2, 1, 3).reshape(T, nkv, D)
    dv = rnd(dvh.reshape(B, nkv, rep, S, D).sum(2)).transpose(0, 2, 1, 3).reshape(T, nkv * D)
    # conjugate rotation, per-head norm backward
    d = _rotate(np.concatenate([dq, dk], 1), cfg.c, cfg.s, conj=True)
    if cfg.qk_norm:
        dxh, t = _norm_bwd(ar, d, k["heads"], k["rstd_h"], k["gam_h"][None])
        gr["gq"] = rnd(ar.sum(t[:, :nq].reshape(T * nq, D), 0))
        gr["gk"] = rnd(ar.sum(t[:, nq:].reshape(T * nkv, D), 0))
        d = dxh
    dqkv = rnd(np.concatenate([d.reshape(T, (nq + nkv) * D), dv], 1))
    # q|k|v
    Gq = q_attn.quant(dqkv, "grad", "qkv.grad")
    dxn = rnd(dgrad_gemm(ar, Gq, k["Wqkv"]))
    dw = rnd(wgrad_gemm(ar, Gq, k["Xq"]))
    gr["wq"], gr["wk"], gr["wv"] = dw[:nq * D], dw[nq * D:(nq + nkv) * D], dw[(nq + nkv) * D:]
    dn, t = _norm_bwd(ar, dxn, k["x"], k["rstd1"], p["ln1"])
    gr["ln1"] = rnd(ar.sum(t, 0))
    dx = rnd(dn + dh1) if cfg.fused else rnd(rnd(dn) + dh1)
    return dx, gr


# ------------------------------------------------------------------------------------------------ head
def shift_labels(labels):
    """[B, S] -> [B S]: the label of position s is token s + 1, the last position of a sequence has none (-100)."""
    lab = np.asarray(labels, dtype=np.int64)
    return np.concatenate([lab[:, 1:], np.full((lab.shape[0], 1), -100, dtype=np.int64)], axis=1).reshape(-1)


def head(p, x, labels, cfg: Config, q: Quantiser, ar: Arith = F64, counted=None):
    """Final RMSNorm (p["norm"]), lm_head (p["table"] [V, H]), shifted-label cross-entropy, mean over the valid tokens: a label
    outside [0, V) is ignored (mi_ce_forward), in the sum and in the count.  -> dict(logits, loss, dx, norm, table): `table` is the
    lm_head's share of the table's gradient.  `counted` (mutants only): another rule for the denominator, a mask -> count."""
    rnd, lab = cfg.rnd, shift_labels(labels)
    V = p["table"].shape[0]
    rstd = _rstd(ar, x, cfg.eps)
    xn = x * rstd[:, None] * p["norm"]
    X = q.quant(xn if cfg.fused else rnd(rnd(x * rstd[:, None]) * p["norm"]), "x", "head.x")
    W = q.quant(p["table"], "w", "head.w")
    logits = rnd(fwd_gemm(ar, X, W))
    valid = (lab >= 0) & (lab < V)
    n_valid = max(int(valid.sum()) if counted is None else int(counted(lab)), 1)
    m = logits.max(-1, keepdims=True)
    e = ar.f(np.exp(logits - m))
    lse = m[:, 0] + np.log(ar.sum(e, -1))
    rows = np.arange(x.shape[0])
    safe = np.where(valid, lab, 0)
    loss = ar.sum(np.where(valid, lse - logits[rows, safe], 0.0), 0) / n_valid
    d = ar.f(np.exp(logits - lse[:, None]))
    d[rows[valid], safe[valid]] -= 1.0
    gscale = 1.0 / n_valid if rnd is ident else float(np.float32(1.0) / np.float32(n_valid))   # a float32 device scalar
    d *= np.where(valid, gscale, 0.0)[:, None]
    Gd = q.quant(d if q.ce_handoff else rnd(d), "grad", "head.grad")
    dxn = rnd(dgrad_gemm(ar, Gd, W))
    dtab = rnd(wgrad_gemm(ar, Gd, X))
    dn, t = _norm_bwd(ar, dxn, x, rstd, p["norm"])
    return dict(logits=logits, loss=loss, dx=rnd(dn), norm=rnd(ar.sum(t, 0)), table=dtab)


# ------------------------------------------------------------------------------------------------ embedding
def embedding_grad(dtable_head, dh0, ids, cfg: Config, ar: Arith = F64):
    """The tied table's gradient: the lm_head's share plus, per token id, the sum of the rows of the first hidden state's
    gradient (every occurrence of a repeated id counts), one rounding."""
    ids = np.asarray(ids, dtype=np.int64).reshape(-1)
    acc = np.zeros_like(dtable_head)
    if ar.seed is None:
        np.add.at(acc, ids, dh0)
    else:
        a32 = np.zeros(acc.shape, dtype=np.float32)
        p = ar._perm(ids.size)
        np.add.at(a32, ids[p], dh0[p].astype(np.float32))
        acc = a32.astype(np.float64)
    return cfg.rnd(dtable_head + acc)


# ------------------------------------------------------------------------------------------------ a whole model, chained
def model(params, ids, labels, cfg: Config, q_attn=None, q_mlp=None, q_head=None, ar: Arith = F64):
    """Forward and backward through embedding, every layer and the head, each segment fed the previous one's output (NOT teacher
    forced: for the comparison with autograd under identity quantisers).  params: dict(table, norm, layers=[{...}]).
    -> (loss, {name: gradient}) with the layers' names prefixed `layers.<i>.`."""
    q_attn, q_mlp, q_head = q_attn or IdentityQ(), q_mlp or IdentityQ(), q_head or IdentityQ()
    ids = np.asarray(ids, dtype=np.int64)
    h = params["table"][ids.reshape(-1)]
    caches = []
    for p in params["layers"]:
        h, k = layer_forward(p, h, cfg, q_attn, q_mlp, ar)
        caches.append(k)
    hd = head(params, h, labels, cfg, q_head, ar)
    grads, d = {"norm": hd["norm"]}, hd["dx"]
    for i in reversed(range(len(caches))):
        d, gr = layer_backward(params["layers"][i], caches[i], d, cfg, q_attn, q_mlp, ar)
        grads.update({f"layers.{i}.{n}": g for n, g in gr.items() if n != "dh1_own"})
    grads["table"] = embedding_grad(hd["table"], d, ids, cfg, ar)
    return hd["loss"], grads


# ------------------------------------------------------------------------------------------------ test data (CPU and GPU tests)
def draw_batch(vocab: int, B: int, S: int, seed: int):
    """(input_ids, labels) int64 [B, S]: ids drawn from a quarter of the vocabulary (so many repeat, within and across the
    sequences) with one id planted eight times; labels = ids, a run and a scatter of positions set to -100."""
    rng = np.random.default_rng([seed, vocab, B, S])
    ids = rng.integers(0, max(vocab // 4, 2), (B, S)).astype(np.int64)
    ids.reshape(-1)[rng.choice(B * S, 8, replace=False)] = vocab - 1
    labels = ids.copy()
    labels[0, 5:12] = -100
    labels.reshape(-1)[rng.choice(B * S, 6, replace=False)] = -100
    return ids, labels


def redraw_(module, seed: int) -> None:
    """Norm weights (decoder, final and QK norms) re-drawn around 1 and biases around 0, in place: at their initial 1 and 0 a wrong
    gamma, a dropped bias or a bias gradient that is never used would go unseen.  Every other parameter keeps its initial value."""
    import torch
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, prm in module.named_parameters():
            parts = name.split(".")
            if parts[-1].endswith("bias"):
                prm.copy_((0.05 * torch.randn(prm.shape, generator=gen)).to(prm.dtype))
            elif parts[-1] == "layer_norm_weight" or (parts[-1] == "weight" and "norm" in parts[-2]):
                prm.copy_((1.0 + 0.25 * torch.randn(prm.shape, generator=gen)).to(prm.dtype))


# ------------------------------------------------------------------------------------------------ comparison
def rel_err(got, ref) -> float:
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(np.linalg.norm((got - ref).ravel()) / max(np.linalg.norm(ref.ravel()), 1e-300))


BF16_FLOOR = 2.0 ** -9   # rms relative error of one bf16 rounding
MARGIN = 4.0             # over max(e_ref, floor): e_ref is a maximum over four samples of a heavy-tailed flip count, and the
#                          device's exp2 / rsqrt are approximations a few fp32 ulp wide that the twin does not model
TWIN_SEEDS = (0, 1, 2, 3)


def bound(e_ref: float) -> float:
    return MARGIN * max(e_ref, BF16_FLOOR)
