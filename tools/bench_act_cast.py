"""GELU / GeGLU fused casts (mi_act_cast, mi_dact_cast) on the GPU; the figures of profiles/act_cast.txt.
  python tools/bench_act_cast.py           kernel times at tokens 8192 x ffn 8192: the fused kernels, the unfused chain they replace
                                           (torch activation, mi_cast_amax, colsum finish) and the SwiGLU kernels at the same size
  python tools/bench_act_cast.py errors    error of the fused and of the unfused LayerNormMLP route against the float64 reference of
                                           tests/test_act_cast_gpu.py, seeds 0-4: the source of that test's tolerance table"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F

from llm_fp8_amd.pytorch import ops

dev = torch.device("cuda:0")


def errors():
    from tests.test_act_cast_gpu import TOL, route_errors
    for case in sorted(TOL):
        for fused in (False, True):
            for seed in range(5):
                err, kinds = route_errors(dev, *case, seed=seed, fused=fused)
                print(json.dumps({"case": case, "fused": fused, "seed": seed, "err": err,
                                  "launches": {k: v["launches"] for k, v in kinds.items()}}), flush=True)


def times():
    R, FF = 8192, 8192
    one = torch.ones(1, dtype=torch.float32, device=dev)
    amax = torch.zeros(1, dtype=torch.float32, device=dev)
    torch.manual_seed(0)

    def timeit(fn, iters=30):
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(iters):
            fn()
        e.record(); torch.cuda.synchronize()
        return s.elapsed_time(e) * 1e3 / iters  # us

    res = {}

    def bench(name, fn):
        res.setdefault(name, []).append(timeit(fn))

    ACTF = {"gelu": lambda a: F.gelu(a, approximate="tanh"),
            "geglu": lambda a: F.gelu(a[..., :a.shape[-1] // 2], approximate="tanh") * a[..., a.shape[-1] // 2:]}
    for rnd in range(5):
        for act, w in (("gelu", 1), ("geglu", 2)):
            h = torch.randn(R, w * FF, device=dev, dtype=torch.bfloat16)
            bias = torch.randn(w * FF, device=dev, dtype=torch.bfloat16)
            d = (torch.randn(R, FF, device=dev) / 8).to(torch.bfloat16)
            bench(f"{act} fused fwd", lambda: ops.act_cast(h, act, one, amax, 0, bias=bias))
            bench(f"{act} fused bwd (+colsum)", lambda: ops.dact_cast(h, d, act, one, amax, 1, want_colsum=True, bias=bias))
            def un_fwd():
                a = ACTF[act](h)
                ops.cast_amax(a, one, amax, 0)
            hr = h.clone().requires_grad_(True)
            a = ACTF[act](hr)
            def un_bwd():
                (dh,) = torch.autograd.grad(a, hr, d, retain_graph=True)
                y, yT, cs = ops.cast_amax(dh, one, amax, 1, want_colsum=True)
                ops.colsum_finish(cs)
            bench(f"{act} unfused fwd (act + cast)", un_fwd)
            bench(f"{act} unfused bwd (act bwd + cast + colsum + finish)", un_bwd)
            del a, hr
        h = torch.randn(R, 2 * FF, device=dev, dtype=torch.bfloat16)
        bias = torch.randn(2 * FF, device=dev, dtype=torch.bfloat16)
        d = (torch.randn(R, FF, device=dev) / 8).to(torch.bfloat16)
        bench("swiglu fwd", lambda: ops.swiglu_cast(h, one, amax, 0, bias=bias))
        bench("swiglu bwd (+colsum)", lambda: ops.dswiglu_cast(h, d, one, amax, 1, want_colsum=True, bias=bias))
    for k, v in res.items():
        v = sorted(v)
        print(f"{k:55s} median {v[len(v)//2]:8.1f} us  min {v[0]:8.1f}  max {v[-1]:8.1f}", flush=True)


if __name__ == "__main__":
    errors() if sys.argv[1:] == ["errors"] else times()
