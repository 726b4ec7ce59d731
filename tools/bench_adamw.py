"""Time ClippedAdamW.step() on the Llama-3.2-3B parameter set: plain multi-tensor update vs update + FP8 weight casts
(mi_adamw_cast_bf16_multi), with the FP8 outputs masked off one by one (MI_DEBUG_SINK = full | noT | none).
With MI_BASE_LIB = a saved libmi_fp8.so: interleaved A/B of the fused step of this build against that one instead."""
import os, sys, time
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from llm_fp8_amd import train

dev = torch.device("cuda:0")
# BENCH_ADAMW_SCENARIO: "default" (per-tensor sinks, mi_adamw_cast_*) | "mxfp8" (block-scaled sinks, mi_adamw_mxcast_*); BENCH_ADAMW_STATE: bf16 | fp32
cfg = train.TrainingConfig(model_name="llama-3.2-3b", batch_size=2, max_seq_length=128, mixed_precision="fp8", use_te=True,
                           fp8_scenario=os.environ.get("BENCH_ADAMW_SCENARIO", "default"), optimizer_state=os.environ.get("BENCH_ADAMW_STATE"))
model = train.prepare_model(train.create_model(cfg, dev), cfg)
opt, sched = train.create_optimizer(model, cfg)
model.train()
batch = train.synthetic_batch(cfg, model.config.vocab_size, dev)
for _ in range(2):
    train.train_step(model, batch, opt, sched, cfg)
params = [p for p in model.parameters() if p.requires_grad]
n = sum(p.numel() for p in params)


def time_step(tag, iters=6):
    for p in params:
        if p.grad is None:
            p.grad = torch.zeros_like(p)
        p.grad.normal_(0, 1e-3)
    opt.step()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        opt.step()
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / iters
    print(f"{tag:28s} {ms:7.2f} ms per step  ({n/1e9:.2f} B params: {n*16/ms/1e9:6.2f} TB/s at 16 B/param, {n*14/ms/1e9:6.2f} at 14)", flush=True)


def ab_against_base(base_path, rounds=8, inner=2):
    """Interleaved A/B of the fused step in one process: this build (cur) against the saved build at `base_path` (base), and base
    against a second copy of its file (base2): base2 / base is the noise of the machine.  optim.py asks _lib.load() at every step."""
    import shutil
    import tempfile
    from llm_fp8_amd import _lib
    cur = _lib.load()
    copy = shutil.copy(base_path, os.path.join(tempfile.mkdtemp(), "libmi_fp8_base2.so"))
    libs = {"base": _lib._bind(base_path, _lib.SIGNATURES), "cur": cur, "base2": _lib._bind(copy, _lib.SIGNATURES)}
    for p in params:
        if p.grad is None:
            p.grad = torch.zeros_like(p)
        p.grad.normal_(0, 1e-3)
    keys, tot = list(libs), {k: 0.0 for k in libs}
    for r in range(-1, rounds):  # round -1: warm-up, not counted
        for k in keys[r % 3:] + keys[:r % 3]:
            _lib._lib = libs[k]
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(inner):
                opt.step()
            e1.record()
            torch.cuda.synchronize()
            if r >= 0:
                tot[k] += e0.elapsed_time(e1) / inner
    _lib._lib = cur
    ms = {k: tot[k] / rounds for k in keys}
    print(f"adamw A/B {cfg.fp8_scenario} state={os.environ.get('BENCH_ADAMW_STATE', 'default')}: base {ms['base']:7.3f} ms  cur {ms['cur']:7.3f} ms  "
          f"cur/base {ms['cur']/ms['base']:.4f}  base2/base {ms['base2']/ms['base']:.4f}", flush=True)


if os.environ.get("MI_BASE_LIB"):  # A/B against a saved build instead of the sink sweep below
    ab_against_base(os.environ["MI_BASE_LIB"])
    sys.exit(0)

for mode in ("full", "noT", "none"):
    os.environ["MI_DEBUG_SINK"] = mode
    opt._plans.clear()
    time_step(f"adamw_cast sinks={mode}")
os.environ.pop("MI_DEBUG_SINK")
os.environ["LLM_FP8_AMD_NO_OPT_WCAST"] = "1"
opt._plans.clear()
time_step("plain adamw_multi")
