"""Current scaling's extra pass (GPU box): mi_amax_bf16 with nontemporal and with plain loads, each followed by the mi_cast_amax that
re-reads the same tensor, against the cast alone.  The question: does a plain-load amax pass leave the tensor in the Infinity Cache
for the cast (a lower SUM for the pair), or is the streaming form faster?

The product library is built with plain loads (mi_current.hip, MI_AMAX_NT = 0: the lower sum, profiles/current_scaling.txt);
`make -C llm_fp8_amd/csrc amax_nt` builds tools/bin/libmi_fp8_amax_nt.so, the same sources with nontemporal loads.  Both are loaded
into this process and every round times every variant once, in rotating order (clock drift hits all alike); medians and the
10th / 90th percentiles are printed, one line each.  Also: the other amax modes and the scale kernel at the step's shapes (product
library)."""
import argparse
import ctypes
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from llm_fp8_amd import _lib  # noqa: E402
from llm_fp8_amd.pytorch import ops  # noqa: E402

NT_LIB = os.path.join(ROOT, "tools", "bin", "libmi_fp8_amax_nt.so")


def _amax_fn(lib):
    fn = lib.mi_amax_bf16
    fn.argtypes, fn.restype = _lib.SIGNATURES["mi_amax_bf16"], ctypes.c_int
    return fn


def timed_rounds(variants, rounds, warmup=3):
    """variants: {name: [callables]} -- each callable is one launch; returns {name: array [rounds, launches] of microseconds}."""
    names = list(variants)
    for n in names:
        for _ in range(warmup):
            for f in variants[n]:
                f()
    torch.cuda.synchronize()
    out = {n: [] for n in names}
    for r in range(rounds):
        for n in names[r % len(names):] + names[:r % len(names)]:
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(len(variants[n]) + 1)]
            ev[0].record()
            for f, e in zip(variants[n], ev[1:]):
                f()
                e.record()
            torch.cuda.synchronize()
            out[n].append([a.elapsed_time(b) * 1e3 for a, b in zip(ev[:-1], ev[1:])])
    return {n: np.array(v) for n, v in out.items()}


def line(label, us, nbytes):
    med, lo, hi = np.median(us), np.percentile(us, 10), np.percentile(us, 90)
    print(f"{label:46s} {med:8.2f} us  (p10 {lo:7.2f}, p90 {hi:7.2f})  {nbytes / med / 1e6:6.2f} TB/s", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=8192)
    ap.add_argument("--cols", type=int, default=3072)
    ap.add_argument("--rounds", type=int, default=200)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    R, C = args.rows, args.cols
    g = torch.Generator(device=dev).manual_seed(0)
    x = torch.randn((R, C), generator=g, device=dev).to(torch.bfloat16)
    plain = _amax_fn(_lib.load())
    if not os.path.exists(NT_LIB):
        raise SystemExit(f"{NT_LIB} not found: run `make -C llm_fp8_amd/csrc amax_nt`")
    nt = _amax_fn(ctypes.CDLL(NT_LIB))
    n = ops.amax_grid(R, C)
    part = torch.empty(n, dtype=torch.float32, device=dev)
    scale = torch.ones(1, dtype=torch.float32, device=dev)
    y = torch.empty((R, C), dtype=torch.uint8, device=dev)
    yT = torch.empty((C, R), dtype=torch.uint8, device=dev)
    st = torch.cuda.current_stream().cuda_stream

    def amax_with(fn):
        def run():
            rc = fn(x.data_ptr(), part.data_ptr(), n, R, C, st)
            assert rc == 0, rc
        return run

    cast = lambda: ops.cast_amax(x, scale, None, 0, y=y, yT=yT)
    # both builds give the same bits
    amax_with(nt)()
    a = part.max().item()
    amax_with(plain)()
    assert a == part.max().item() == x.float().abs().max().item()
    t = timed_rounds({"nt": [amax_with(nt), cast], "plain": [amax_with(plain), cast], "cast": [cast],
                      "nt_alone": [amax_with(nt)], "plain_alone": [amax_with(plain)]}, args.rounds)
    print(f"# {R} x {C} bf16 ({R * C * 2 / 1e6:.1f} MB), n_partial {n}, {args.rounds} interleaved rounds", flush=True)
    line("mi_amax_bf16 nontemporal, alone", t["nt_alone"][:, 0], 2 * R * C)
    line("mi_amax_bf16 plain, alone", t["plain_alone"][:, 0], 2 * R * C)
    line("mi_cast_amax (y + yT), alone", t["cast"][:, 0], 4 * R * C)
    for k, name in (("nt", "nontemporal"), ("plain", "plain")):
        line(f"pair {name}: mi_amax_bf16", t[k][:, 0], 2 * R * C)
        line(f"pair {name}: the mi_cast_amax that follows", t[k][:, 1], 4 * R * C)
        line(f"pair {name}: sum", t[k].sum(1), 6 * R * C)
    # the fused modes at the step's shapes (product library)
    F = 8192
    h = torch.randn((R, 2 * F), generator=g, device=dev).to(torch.bfloat16)
    d = torch.randn((R, F), generator=g, device=dev).to(torch.bfloat16)
    gamma = torch.ones(C, dtype=torch.bfloat16, device=dev)
    rstd = ops.rmsnorm_stats(x, 1e-5)
    p2 = torch.empty(ops.amax_grid(R, F, 32), dtype=torch.float32, device=dev)
    t = timed_rounds({"norm": [lambda: ops.amax_norm(x, rstd, gamma, part)], "swiglu": [lambda: ops.amax_swiglu(h, None, p2)],
                      "dswiglu": [lambda: ops.amax_dswiglu(h, None, d, p2)],
                      "scale": [lambda: ops.current_scale(part, 448.0)]}, max(20, args.rounds // 4))
    line(f"mi_amax_norm {R} x {C}", t["norm"][:, 0], 2 * R * C)
    line(f"mi_amax_swiglu {R} x {F}", t["swiglu"][:, 0], 4 * R * F)
    line(f"mi_amax_dswiglu {R} x {F}", t["dswiglu"][:, 0], 6 * R * F)
    line("mi_current_scale (+ the torch.empty(3))", t["scale"][:, 0], 4 * n)


if __name__ == "__main__":
    main()
