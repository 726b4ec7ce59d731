"""Packed-sequence causal attention, forward + backward of one layer on one row of T tokens, three routes per document layout:
    packed   DotProductAttention(...)(q, k, v, cu_seqlens_q=cu) on the document-limited kernels (mi_attn_fwd_seg / mi_attn_bwd_seg)
    causal   the full-causal kernels on the same operands (no cu_seqlens: what the row costs if the documents are ignored)
    sdpa     the packed call under LLM_FP8_AMD_NO_PACKED_ATTN=1 (torch SDPA with the boolean document mask)
Layouts: `uniform` = documents of --doc tokens each; `ragged` = the same number of documents with seeded random lengths (each >= 1).
Device time between two events around back-to-back calls; the layouts are walked `repeats` + 1 times with the three routes
alternating (the first pass is a warm-up and is dropped); printed: median and min .. max of the repeats, in microseconds per
forward + backward, and the share of the causal (i, j) pairs that lie inside a document.

    python tools/bench_attn_packed.py                          3B shape (H 24, G 8, D 128), T 8192, documents of 512
    python tools/bench_attn_packed.py --repeats 3 --doc 1024 8192,32,8,64      T,H,G,D cases"""
import argparse, os, statistics, sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from llm_fp8_amd.pytorch import attention as A

dev = torch.device("cuda:0")


def timeit(fn, n, warm=3):
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


def layouts(T, doc, seed):
    n = T // doc
    cuts = torch.randperm(T - 1, generator=torch.Generator().manual_seed(seed))[:n - 1].sort().values + 1
    return {"uniform": torch.arange(0, T + 1, doc, dtype=torch.int32),
            "ragged": torch.cat((torch.zeros(1, dtype=torch.int64), cuts, torch.tensor([T]))).to(torch.int32)}


def step_fns(T, H, G, D, cu):
    core = A.DotProductAttention(H, D, G, attention_dropout=0.0, attn_mask_type="causal", qkv_format="bshd")
    q, k, v = (torch.randn(1, T, n, D, device=dev, dtype=torch.bfloat16, requires_grad=True) for n in (H, G, G))
    go = torch.randn(1, T, H * D, device=dev, dtype=torch.bfloat16)
    assert A._flash_ok(q, k, v, True, 0.0)

    def run(switch, **kw):
        def fn():
            os.environ["LLM_FP8_AMD_NO_PACKED_ATTN"] = switch
            q.grad = k.grad = v.grad = None
            core(q, k, v, **kw).backward(go)
        return fn
    return {"packed": run("0", cu_seqlens_q=cu), "causal": run("0"), "sdpa": run("1", cu_seqlens_q=cu)}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("cases", nargs="*", help="T,H,G,D")
    ap.add_argument("--doc", type=int, default=512, help="tokens per document of the uniform layout (T / doc documents in both)")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    cases = [tuple(int(x) for x in s.split(",")) for s in a.cases] or [(8192, 24, 8, 128)]
    routes = ("packed", "causal", "sdpa")
    times, share = {}, {}
    for rep in range(a.repeats + 1):
        for c in cases:
            for name, cu in layouts(c[0], a.doc, a.seed).items():
                lens = (cu[1:] - cu[:-1]).double()
                share[(c, name)] = float((lens * (lens + 1)).sum() / (c[0] * (c[0] + 1.0)))
                fns = step_fns(*c, cu.to(dev))  # (built per visit: SDPA's score tensors need the room)
                for route in routes:
                    t = timeit(fns[route], 5 if route == "sdpa" else 30)
                    if rep:
                        times.setdefault((c, name, route), []).append(t)
                del fns
    for (c, name), s in share.items():
        line = "T{} H{} G{} D{} {} ({:.1%} of the causal pairs):".format(*c, name, s)
        med = {}
        for route in routes:
            t = times[(c, name, route)]
            med[route] = statistics.median(t)
            line += f"   {route} {med[route]:8.1f} us ({min(t):8.1f} .. {max(t):8.1f})"
        print(line + f"   causal / packed {med['causal'] / med['packed']:5.2f}   sdpa / packed {med['sdpa'] / med['packed']:5.2f}", flush=True)
