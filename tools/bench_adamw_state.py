"""Time ClippedAdamW.step() on the Llama-3.2-3B parameter set in the optimiser-state modes: bf16 state, fp32 state
(state_dtype=torch.float32: fp32 master weights and moments) and bf16_sr (bf16 state, stochastic rounding of the weight and both
moments), under delayed scaling and under MXFP8: HIP events around each step, 3 warm-ups, 10 repetitions per block.
The rate is against the bytes of the update pass with a sink: 16 B per parameter (bf16 state, bf16_sr), 30 B (fp32 state).

  python tools/bench_adamw_state.py [--modes bf16,fp32] [--scenarios default,mxfp8] [--rounds 1] [--reps 10]

The model is built once per scenario; every mode gets its own optimiser on it and the modes are timed in alternating blocks,
`--rounds` times each.  A library of an earlier revision (LLM_FP8_AMD_LIB) runs the modes it has: `--modes bf16`."""
import argparse, gc, os, statistics, sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from llm_fp8_amd import _lib, train
from llm_fp8_amd.pytorch.fp8 import FP8GlobalStateManager

BYTES = {"bf16": 16, "fp32": 30, "bf16_sr": 16}
ap = argparse.ArgumentParser()
ap.add_argument("--modes", default="bf16,fp32")
ap.add_argument("--scenarios", default="default,mxfp8")
ap.add_argument("--rounds", type=int, default=1)
ap.add_argument("--reps", type=int, default=10)
args = ap.parse_args()
modes = args.modes.split(",")
assert all(m in BYTES for m in modes), modes

dev = torch.device("cuda:0")
print(f"library {_lib.LIB_PATH} (ABI {_lib.ABI_VERSION} revision {_lib.revision()})", flush=True)
for scenario in args.scenarios.split(","):
    FP8GlobalStateManager.reset()
    cfg = lambda mode: train.TrainingConfig(model_name="llama-3.2-3b", batch_size=2, max_seq_length=128, mixed_precision="fp8",
                                            fp8_scenario=scenario, use_te=True, optimizer_state=mode)
    torch.manual_seed(0)
    model = train.prepare_model(train.create_model(cfg(modes[0]), dev), cfg(modes[0]))
    opts = {mode: train.create_optimizer(model, cfg(mode)) for mode in modes}
    model.train()
    batch = train.synthetic_batch(cfg(modes[0]), model.config.vocab_size, dev)
    for _ in range(2):  # every weight gets its sink
        train.train_step(model, batch, *opts[modes[0]], cfg(modes[0]))
    params = [p for p in model.parameters() if p.requires_grad]
    n = sum(p.numel() for p in params)
    for p in params:
        if p.grad is None:
            p.grad = torch.zeros_like(p)
        p.grad.normal_(0, 1e-3)
    for mode in modes:
        for _ in range(3):
            opts[mode][0].step()
    torch.cuda.synchronize()
    for rnd in range(args.rounds):
        for mode in modes:
            opt, bpp = opts[mode][0], BYTES[mode]
            ms = []
            for _ in range(args.reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                opt.step()
                e1.record()
                torch.cuda.synchronize()
                ms.append(e0.elapsed_time(e1))
            med = statistics.median(ms)
            print(f"{scenario:8s} state={mode:8s} round {rnd}: opt.step() median {med:6.2f} ms (min {min(ms):.2f}, max {max(ms):.2f}) over {args.reps} reps "
                  f"after 3 warm-ups; {n / 1e9:.3f} B params x {bpp} B = {n * bpp / 1e9:.1f} GB -> {n * bpp / med / 1e9:.2f} TB/s  "
                  "(clip norm pass + update, all launches of the step)", flush=True)
    del model, opts, params, batch
    gc.collect()
    torch.cuda.empty_cache()
