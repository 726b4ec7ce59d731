"""Attention core at 16 <= S <= 112, forward + backward of one layer: attention._ShortAttnFn (mi_attn_short_*) against
DotProductAttention with LLM_FP8_AMD_NO_SHORT_ATTN=1 (torch SDPA, what these lengths took before).  Two timings per shape and
route, in microseconds per forward + backward:
    eager    the calls as a training step makes them, on an idle device: host launch path and kernels, whichever is longer
    queued   the same calls enqueued behind ~25 ms of other work, so the host runs ahead: device time only
The shape list is walked `repeats` + 1 times with the two routes alternating (the first pass is a warm-up and is dropped), so
the repeats are interleaved; printed: median and min .. max of the repeats.

    python tools/bench_attn_short.py                       the 3B and 1B shapes at every S, five repeats
    python tools/bench_attn_short.py --repeats 3 16,64,24,8,128     B,S,H,G,D shapes"""
import argparse, os, statistics, sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from llm_fp8_amd.pytorch import attention as A

dev = torch.device("cuda:0")
DEFAULT = [(16, S, H, 8, D) for H, D in ((24, 128), (32, 64)) for S in range(16, 128, 16)]
_BUSY = None


def timeit(fn, queued, n, warm=20):
    global _BUSY
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    if queued:
        if _BUSY is None:
            _BUSY = torch.randn(8192, 8192, device=dev, dtype=torch.bfloat16)
        for _ in range(24):
            torch.mm(_BUSY, _BUSY)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n * 1e3


def step_fns(B, S, H, G, D):
    core = A.DotProductAttention(H, D, G, attention_dropout=0.0, attn_mask_type="causal", qkv_format="bshd")
    q, k, v = (torch.randn(B, S, n, D, device=dev, dtype=torch.bfloat16, requires_grad=True) for n in (H, G, G))
    go = torch.randn(B, S, H * D, device=dev, dtype=torch.bfloat16)
    assert not A._short_ok(q, k, v, True, 0.0) and not A._flash_ok(q, k, v, True, 0.0)  # (the switch is set: `core` is SDPA)

    def short():
        q.grad = k.grad = v.grad = None
        A._ShortAttnFn.apply(q, k, v, D ** -0.5).reshape(B, S, H * D).backward(go)

    def sdpa():
        q.grad = k.grad = v.grad = None
        core(q, k, v).backward(go)
    return {"short": short, "sdpa": sdpa}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("shapes", nargs="*", help="B,S,H,G,D")
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    os.environ["LLM_FP8_AMD_NO_SHORT_ATTN"] = "1"
    shapes = [tuple(int(x) for x in s.split(",")) for s in a.shapes] or DEFAULT
    fns = {s: step_fns(*s) for s in shapes}
    times = {}
    for queued in (False, True):  # (all eager passes first: the filler work of the queued ones would disturb them)
        for rep in range(a.repeats + 1):
            for s in shapes:
                for route in ("short", "sdpa"):
                    t = timeit(fns[s][route], queued, 100 if queued else 500)
                    if rep:
                        times.setdefault((s, route, queued), []).append(t)
    for queued in (False, True):
        print("eager" if not queued else "queued (device time)")
        for s in shapes:
            line = "  B{} S{} H{} G{} D{}:".format(*s)
            med = {}
            for route in ("short", "sdpa"):
                t = times[(s, route, queued)]
                med[route] = statistics.median(t)
                line += f"   {route} {med[route]:7.1f} us ({min(t):7.1f} .. {max(t):7.1f})"
            print(line + f"   sdpa / short {med['sdpa'] / med['short']:5.2f}", flush=True)
