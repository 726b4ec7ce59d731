"""LayerNorm fused with the FP8 cast (mi_layernorm_stats, mi_ln_cast, mi_layernorm_bwd) on the GPU; the figures of
profiles/layernorm_cast.txt.
  python tools/bench_layernorm_cast.py          chain times at tokens 8192 x hidden 768, 1600, 4096, one process, the chains
                                                alternating inside each of 5 rounds, 30 iterations per measurement after warm-up:
                                                  forward   stats + ln_cast          against  F.layer_norm + cast_amax
                                                  backward  layernorm_bwd (+ dres)   against  autograd's LayerNorm backward + residual add
                                                and the bytes each chain moves, from the shapes
  python tools/bench_layernorm_cast.py errors   error of the fused and of the unfused module route against the float64 reference of
                                                tests/test_layernorm_cast_gpu.py, seeds 0-4: the source of that test's tolerance table"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F

from llm_fp8_amd.pytorch import ops

dev = torch.device("cuda:0")


def errors():
    from tests.test_layernorm_cast_gpu import CASES, route_errors
    for case in CASES:
        for current in (False, True):
            for fused in (False, True):
                for seed in range(5):
                    err = route_errors(dev, *case, current, seed=seed, fused=fused)
                    print(json.dumps({"case": [*case, current], "fused": fused, "seed": seed, "err": err}), flush=True)


def times():
    R = 8192
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

    res, moved = {}, {}
    for rnd in range(5):
        for C in (768, 1600, 4096):
            x = torch.randn(R, C, device=dev, dtype=torch.bfloat16)
            gamma = (torch.rand(C, device=dev) + 0.5).to(torch.bfloat16)
            beta = torch.randn(C, device=dev, dtype=torch.bfloat16)
            dy = (torch.randn(R, C, device=dev) / 8).to(torch.bfloat16)
            dres = (torch.randn(R, C, device=dev) / 8).to(torch.bfloat16)
            mean, rstd = ops.layernorm_stats(x, 1e-5)

            def fused_fwd():
                m, r = ops.layernorm_stats(x, 1e-5)
                ops.ln_cast(x, m, r, gamma, beta, one, amax, 0)

            def unfused_fwd():
                ops.cast_amax(F.layer_norm(x, (C,), gamma, beta, 1e-5), one, amax, 0)

            xr, gr, br = (t.clone().requires_grad_(True) for t in (x, gamma, beta))
            yn = F.layer_norm(xr, (C,), gr, br, 1e-5)

            def unfused_bwd():
                dx, dg, db = torch.autograd.grad(yn, (xr, gr, br), dy, retain_graph=True)
                return dx + dres

            RC = R * C  # elements; bytes below: bf16 = 2, FP8 = 1 (two copies), the [C] and [R] vectors left out
            chains = {"fwd fused   (stats + ln_cast)": (fused_fwd, (2 + 2 + 2) * RC),             # x twice; y, yT
                      "fwd unfused (layer_norm + cast_amax)": (unfused_fwd, (2 + 2 + 2 + 2) * RC),  # x, xn out, xn in; y, yT
                      "bwd fused   (layernorm_bwd + finish)": (lambda: ops.layernorm_bwd(dy, x, mean, rstd, gamma, dres=dres), (2 + 2 + 2 + 2) * RC),
                      "bwd unfused (autograd + residual add)": (unfused_bwd, (2 + 2 + 2 + 2 + 2 + 2) * RC)}  # dy, x, dx out; dx, dres in, sum out
            for name, (fn, nbytes) in chains.items():  # alternating: one measurement of each chain per round and width
                res.setdefault((C, name), []).append(timeit(fn))
                moved[C, name] = nbytes
            del yn, xr, gr, br
    for (C, name), v in res.items():
        v = sorted(v)
        print(f"8192 x {C:5d}  {name:40s} median {v[len(v) // 2]:8.1f} us  min {v[0]:8.1f}  max {v[-1]:8.1f}  "
              f"{moved[C, name] / 1e6:7.1f} MB  {moved[C, name] / v[len(v) // 2] / 1e6:6.2f} TB/s", flush=True)


if __name__ == "__main__":
    errors() if sys.argv[1:] == ["errors"] else times()
