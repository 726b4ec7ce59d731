"""Sliding-window causal attention, forward + backward of one layer, three routes per (shape, window):
    window   DotProductAttention(window_size=(W - 1, 0)) on the band-limited kernels (mi_attn_fwd_win / mi_attn_bwd_win)
    causal   the full-causal kernels on the same operands (no window: what a window costs if it is ignored; the band kernels
             do about (W + 64) / (S / 2) of their MFMA work)
    sdpa     the same windowed module under LLM_FP8_AMD_NO_WINDOW_ATTN=1 (torch SDPA with the cached boolean band mask)
Device time: at these sizes a forward + backward runs for hundreds of microseconds, longer than its host launch path, and the
timed calls are enqueued back to back between two events.  The (shape, window) list is walked `repeats` + 1 times with the
three routes alternating (the first pass is a warm-up and is dropped); printed: median and min .. max of the repeats, in
microseconds per forward + backward.

    python tools/bench_attn_window.py                      3B (H 24, G 8, D 128) and 1B (H 32, G 8, D 64) shapes, 8192 tokens
    python tools/bench_attn_window.py --repeats 3 4,2048,24,8,128,512     B,S,H,G,D,W cases"""
import argparse, os, statistics, sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from llm_fp8_amd.pytorch import attention as A

dev = torch.device("cuda:0")
DEFAULT = [(8192 // S, S, H, 8, D, W) for H, D in ((24, 128), (32, 64)) for S in (512, 2048, 4096) for W in (128, 512, 1024) if W < S]


def timeit(fn, n, warm=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n * 1e3


def step_fns(B, S, H, G, D, W):
    kw = dict(attention_dropout=0.0, attn_mask_type="causal", qkv_format="bshd")
    banded, full = A.DotProductAttention(H, D, G, window_size=(W - 1, 0), **kw), A.DotProductAttention(H, D, G, **kw)
    q, k, v = (torch.randn(B, S, n, D, device=dev, dtype=torch.bfloat16, requires_grad=True) for n in (H, G, G))
    go = torch.randn(B, S, H * D, device=dev, dtype=torch.bfloat16)
    assert A._flash_ok(q, k, v, True, 0.0)

    def run(core, switch):
        def fn():
            os.environ["LLM_FP8_AMD_NO_WINDOW_ATTN"] = switch
            q.grad = k.grad = v.grad = None
            core(q, k, v).backward(go)
        return fn
    return {"window": run(banded, "0"), "causal": run(full, "0"), "sdpa": run(banded, "1")}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("cases", nargs="*", help="B,S,H,G,D,W")
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    cases = [tuple(int(x) for x in s.split(",")) for s in a.cases] or DEFAULT
    routes = ("window", "causal", "sdpa")
    times = {}
    for rep in range(a.repeats + 1):
        for c in cases:
            fns = step_fns(*c)  # (built per visit: the operands of all cases together would not fit beside SDPA's score tensors)
            for route in routes:
                t = timeit(fns[route], 10 if route == "sdpa" else 30)
                if rep:
                    times.setdefault((c, route), []).append(t)
            del fns
    for c in cases:
        line = "B{} S{} H{} G{} D{} W{}:".format(*c)
        med = {}
        for route in routes:
            t = times[(c, route)]
            med[route] = statistics.median(t)
            line += f"   {route} {med[route]:8.1f} us ({min(t):8.1f} .. {max(t):8.1f})"
        print(line + f"   causal / window {med['causal'] / med['window']:5.2f}   sdpa / window {med['sdpa'] / med['window']:5.2f}", flush=True)
