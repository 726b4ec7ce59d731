"""Time ClippedAdamW.step() on the Llama-3.2-3B parameter set with bf16 state and with fp32 state (state_dtype=torch.float32:
fp32 master weights and moments), under delayed scaling and under MXFP8: HIP events around each step, 3 warm-ups, 10 repetitions.
The rate is against the bytes of the update pass with a sink: 16 B per parameter (bf16 state), 30 B (fp32 state)."""
import gc, os, statistics, sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from llm_fp8_amd import train
from llm_fp8_amd.pytorch.fp8 import FP8GlobalStateManager

dev = torch.device("cuda:0")
for scenario in ("default", "mxfp8"):
    for mode, bpp in (("bf16", 16), ("fp32", 30)):
        FP8GlobalStateManager.reset()
        cfg = train.TrainingConfig(model_name="llama-3.2-3b", batch_size=2, max_seq_length=128, mixed_precision="fp8", fp8_scenario=scenario,
                                   use_te=True, optimizer_state=mode)
        torch.manual_seed(0)
        model = train.prepare_model(train.create_model(cfg, dev), cfg)
        opt, sched = train.create_optimizer(model, cfg)
        model.train()
        batch = train.synthetic_batch(cfg, model.config.vocab_size, dev)
        for _ in range(2):
            train.train_step(model, batch, opt, sched, cfg)
        params = [p for p in model.parameters() if p.requires_grad]
        n = sum(p.numel() for p in params)
        for p in params:
            if p.grad is None:
                p.grad = torch.zeros_like(p)
            p.grad.normal_(0, 1e-3)
        for _ in range(3):
            opt.step()
        torch.cuda.synchronize()
        ms = []
        for _ in range(10):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            opt.step()
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        med = statistics.median(ms)
        line = (f"{scenario:8s} state={mode}: opt.step() median {med:6.2f} ms (min {min(ms):.2f}, max {max(ms):.2f}) over 10 reps after 3 warm-ups; "
                f"{n / 1e9:.3f} B params x {bpp} B = {n * bpp / 1e9:.1f} GB -> {n * bpp / med / 1e9:.2f} TB/s  (clip norm pass + update, all launches of the step)")
        print(line, flush=True)
        del model, opt, sched, params, batch
        gc.collect()
        torch.cuda.empty_cache()
