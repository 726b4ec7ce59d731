"""Per-head QK RMSNorm + RoPE split: the fused pair (mi_qknorm_rope_qkv / mi_qknorm_rope_qkv_bwd, attention._QKNormRoPESplitFn) against
the torch route of MultiheadAttention._attend_qk_norm (split, RMSNorm on the head views, apply_rotary_pos_emb), forward + backward,
at the attention shapes of Qwen3-0.6B and Qwen3-4B (batch 16 x seq 512).  The two routes are alternated inside each of three repeats;
a repeat times ITERS forward + backward pairs between two device events after WARM untimed ones.  The fused kernels are also timed
alone, against the bytes they have to move (computed here from the shapes).

    python tools/bench_qknorm.py [--iters 30] [--warm 5] [--repeats 3]"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import llm_fp8_amd.pytorch as te  # noqa: E402
from llm_fp8_amd.pytorch import attention as A, ops  # noqa: E402

SHAPES = {"qwen3-0.6b": (16, 8), "qwen3-4b": (32, 8)}  # (query heads, KV heads); head_dim 128
B, S, D, EPS = 16, 512, 128, 1e-6


def bytes_moved(nq, nkv):
    """(forward, backward) bytes the fused kernels read + write: fused in, q | k | v out, rstd; dq | dk | dv and the q | k columns of
    the saved input in, d(qkv) out, rstd.  Tables, gammas and partials are below 1 MB."""
    T, W, H = B * S, (nq + 2 * nkv) * D, nq + nkv
    fwd = 2 * T * W * 2 + T * H * 4
    bwd = T * W * 2 + T * H * D * 2 + T * W * 2 + T * H * 4
    return fwd, bwd


def timed(fn, iters, warm):
    for _ in range(warm):
        fn()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters  # ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warm", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_qknorm.py needs the GPU: nothing is measured without one")
    dev = torch.device("cuda:0")
    print(f"device {torch.cuda.get_device_name(0)}; batch {B} x seq {S}, head_dim {D}; {a.repeats} repeats of {a.iters} fwd+bwd, routes alternated")
    for name, (nq, nkv) in SHAPES.items():
        torch.manual_seed(0)
        m = te.MultiheadAttention(hidden_size=nq * D, num_attention_heads=nq, kv_channels=D, num_gqa_groups=nkv, bias=False,
                                  input_layernorm=True, normalization="RMSNorm", qkv_format="bshd", params_dtype=torch.bfloat16,
                                  device=dev, qk_norm_type="RMSNorm", qk_norm_eps=EPS)
        W = (nq + 2 * nkv) * D
        qkv = torch.randn(B, S, W, device=dev, dtype=torch.bfloat16, requires_grad=True)
        rope = te.attention.RotaryPositionEmbedding(D, rotary_base=1e6)(max_seq_len=S).to(dev)
        cos, sin = A._cos_sin_tables(rope, S)
        gq, gk = m.q_norm.weight, m.k_norm.weight
        grads = [torch.randn(B, S, h, D, device=dev, dtype=torch.bfloat16) for h in (nq, nkv, nkv)]

        def fused():
            out = A._QKNormRoPESplitFn.apply(qkv, gq, gk, cos, sin, nq, nkv, D, EPS)
            torch.autograd.backward(out, grads)

        def torch_route():
            q, k, v = torch.split(qkv, m.split, dim=-1)
            q = A.apply_rotary_pos_emb(m.q_norm(q.reshape(B, S, nq, D)).to(qkv.dtype), rope, "bshd")
            k = A.apply_rotary_pos_emb(m.k_norm(k.reshape(B, S, nkv, D)).to(qkv.dtype), rope, "bshd")
            torch.autograd.backward((q, k, v.reshape(B, S, nkv, D)), grads)

        x2 = qkv.detach().reshape(B * S, W)
        q_, k_, v_, rstd = ops.qknorm_rope_qkv_forward(x2, gq.detach(), gk.detach(), cos, sin, nq, nkv, D, S, EPS)
        g2 = [g.reshape(B * S, -1) for g in grads]
        fwd_only = lambda: ops.qknorm_rope_qkv_forward(x2, gq.detach(), gk.detach(), cos, sin, nq, nkv, D, S, EPS)
        bwd_only = lambda: ops.qknorm_rope_qkv_backward(*g2, x2, rstd, gq.detach(), gk.detach(), cos, sin, nq, nkv, D, S)
        res = {"fused": [], "torch": [], "fwd": [], "bwd": []}
        for _ in range(a.repeats):
            for key, fn in (("fused", fused), ("torch", torch_route), ("fwd", fwd_only), ("bwd", bwd_only)):
                qkv.grad = gq.grad = gk.grad = None
                res[key].append(timed(fn, a.iters, a.warm))
        fb, bb = bytes_moved(nq, nkv)
        med = {k: statistics.median(v) for k, v in res.items()}
        fmt = lambda v: " / ".join(f"{x:.3f}" for x in v)
        print(f"{name} (q {nq}, kv {nkv}, rows {B * S}, W {W}):")
        print(f"  fused fwd+bwd  {fmt(res['fused'])} ms   (median {med['fused']:.3f})")
        print(f"  torch fwd+bwd  {fmt(res['torch'])} ms   (median {med['torch']:.3f})   torch / fused = {med['torch'] / med['fused']:.2f}")
        print(f"  fused forward alone   {fmt(res['fwd'])} ms: {fb / 1e6:.0f} MB -> {fb / med['fwd'] / 1e9:.2f} TB/s")
        print(f"  fused backward alone  {fmt(res['bwd'])} ms (with the finish of the gamma partials): {bb / 1e6:.0f} MB -> {bb / med['bwd'] / 1e9:.2f} TB/s")


if __name__ == "__main__":
    main()
