"""Float8BlockScaling against MXFP8 on one GPU: the quantise kernels, and a training step.

  kernels   the block quantiser at 8192 x 3072 (1 x 128 blocks: both copies; 128 x 128 blocks: both copies) against mi_mxfp8_quantize
            at the same shape, and the three fused front ends (RMSNorm, SwiGLU, dSwiGLU) against their MX twins at the Llama-3.2-3B
            shapes (8192 tokens, hidden 3072, FFN 8192).  The two sides alternate `--reps` times; every launch is timed with device
            events and one line per kernel and repeat is printed (median and p10 / p90 over `--iters` launches).  Under
            `rocprofv3 --kernel-trace --stats -- python tools/bench_block_scaling.py kernels` the kernel durations come from the
            trace instead; the template arguments in the kernel names tell the sides apart (the last one: 0 = MX, 1 = 1 x 128,
            2 = 128 x 128).
  step      train.train_step of Llama-3.2-3B, batch 16 x 512, under --fp8_scenario block against mxfp8: the sides alternate
            `--reps` times, each on a freshly built model; device events around every step after `--warmup` steps; medians and the
            spread are printed per repeat and over all."""
import argparse
import gc
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from llm_fp8_amd.pytorch import ops  # noqa: E402


def _timed(fn, iters, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(iters + 1)]
    ev[0].record()
    for e in ev[1:]:
        fn()
        e.record()
    torch.cuda.synchronize()
    return np.array([a.elapsed_time(b) * 1e3 for a, b in zip(ev[:-1], ev[1:])])


def kernels(a):
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(1)
    T, H, F = a.tokens, a.hidden, a.ffn
    x = torch.randn(T, H, device=dev, generator=g).to(torch.bfloat16)
    gamma = (torch.rand(H, device=dev, generator=g) + 0.5).to(torch.bfloat16)
    rstd = ops.rmsnorm_stats(x, 1e-5)
    h = (torch.randn(T, 2 * F, device=dev, generator=g) * 2).to(torch.bfloat16)
    d = (torch.randn(T, F, device=dev, generator=g) / 8).to(torch.bfloat16)
    E = ops.E4M3
    cases = [
        ("quantize", lambda: ops.mxfp8_quantize(x, E), {1: lambda: ops.blockfp8_quantize(x, E, 1), 2: lambda: ops.blockfp8_quantize(x, E, 2)}),
        ("norm", lambda: ops.mxfp8_norm_quantize(x, rstd, gamma, E),
         {1: lambda: ops.blockfp8_norm_quantize(x, rstd, gamma, E, 1), 2: lambda: ops.blockfp8_norm_quantize(x, rstd, gamma, E, 2)}),
        ("swiglu", lambda: ops.mxfp8_swiglu_quantize(h, E),
         {1: lambda: ops.blockfp8_swiglu_quantize(h, E, 1), 2: lambda: ops.blockfp8_swiglu_quantize(h, E, 2)}),
        ("dswiglu", lambda: ops.mxfp8_dswiglu_quantize(h, d, E, want_colsum=True),
         {1: lambda: ops.blockfp8_dswiglu_quantize(h, d, E, 1, want_colsum=True),
          2: lambda: ops.blockfp8_dswiglu_quantize(h, d, E, 2, want_colsum=True)}),
    ]
    for name, mx, blk in cases:
        for rep in range(a.reps):
            for side, fn in (("mx", mx), ("block dim 1", blk[1]), ("block dim 2", blk[2])):
                us = _timed(fn, a.iters)
                print(f"{name:9s} rep {rep} {side:12s} median {np.median(us):8.2f} us  (p10 {np.percentile(us, 10):8.2f}, "
                      f"p90 {np.percentile(us, 90):8.2f})", flush=True)


def _one_side(scenario, a, device):
    from llm_fp8_amd import train
    from llm_fp8_amd.pytorch.fp8 import FP8GlobalStateManager
    FP8GlobalStateManager.reset()
    cfg = train.TrainingConfig(model_name=a.model_name, batch_size=a.batch_size, max_seq_length=a.max_seq_length, mixed_precision="fp8",
                               fp8_scenario=scenario, use_te=True, sharding_mode="none")
    torch.manual_seed(cfg.seed)
    model = train.prepare_model(train.create_model(cfg, device), cfg)
    model = train.wrap_distributed(model, cfg, device)  # (one process: the single-process path, as train.main takes it)
    opt, sched = train.create_optimizer(model, cfg)
    model.train()
    vocab = model.config.vocab_size
    ms, loss = [], None
    for step in range(a.warmup + a.steps):
        batch = train.synthetic_batch(cfg, vocab, device)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        loss = train.train_step(model, batch, opt, sched, cfg)
        e1.record()
        torch.cuda.synchronize()
        if step >= a.warmup:
            ms.append(e0.elapsed_time(e1))
    lv = loss.item()
    del model, opt, sched, loss
    gc.collect()
    torch.cuda.empty_cache()
    FP8GlobalStateManager.reset()
    return np.array(ms), lv


def step(a):
    device = torch.device("cuda:0")
    torch.cuda.set_device(device)
    allms = {"block": [], "mxfp8": []}
    for rep in range(a.reps):
        for scenario in ("block", "mxfp8"):
            ms, lv = _one_side(scenario, a, device)
            allms[scenario].append(ms)
            print(json.dumps({"scenario": scenario, "rep": rep, "median_ms": round(float(np.median(ms)), 3), "min_ms": round(float(ms.min()), 3),
                              "max_ms": round(float(ms.max()), 3), "steps": len(ms), "last_loss": lv}), flush=True)
    med = {s: float(np.median(np.concatenate(v))) for s, v in allms.items()}
    reps = {s: [round(float(np.median(m)), 3) for m in v] for s, v in allms.items()}
    print(json.dumps({"median_ms": med, "per_rep_median_ms": reps, "block_minus_mxfp8_ms": round(med["block"] - med["mxfp8"], 3)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="mode", required=True)
    k = sub.add_parser("kernels")
    k.add_argument("--tokens", type=int, default=8192)
    k.add_argument("--hidden", type=int, default=3072)
    k.add_argument("--ffn", type=int, default=8192)
    k.add_argument("--reps", type=int, default=3)
    k.add_argument("--iters", type=int, default=50)
    s = sub.add_parser("step")
    s.add_argument("--model_name", default="meta-llama/Llama-3.2-3B")
    s.add_argument("--batch_size", type=int, default=16)
    s.add_argument("--max_seq_length", type=int, default=512)
    s.add_argument("--reps", type=int, default=3)
    s.add_argument("--steps", type=int, default=12)
    s.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    (kernels if a.mode == "kernels" else step)(a)


if __name__ == "__main__":
    main()
