"""Time mi_grad_accum_multi (fp32 gradient accumulation, include/mi_fp8.h) alone on the Llama-3.2-3B parameter set -- the tensor
sizes tools/bench_adamw.py steps -- per mode, next to mi_sumsq_bf16_multi over the same tensors (both are pure streams), and
A/B the store policy (fp32 sums stored plain, the bf16 result nontemporal) against the build with the other policy on both
(`make -C llm_fp8_amd/csrc accum_ab`; MI_ACCUM_AB_LIB names another file).  Bytes per element: SET 6, ADD 10, FINISH 8, squared norm 2."""
import os, sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from llm_fp8_amd import _lib, grad_accum, train
from llm_fp8_amd.optim import CHUNK

dev = torch.device("cuda:0")
cfg = train.TrainingConfig(model_name="llama-3.2-3b", batch_size=2, max_seq_length=128, mixed_precision="fp8", use_te=True)
model = train.create_model(cfg, dev)
sizes = tuple(p.numel() for p in model.parameters() if p.requires_grad)
del model
torch.cuda.empty_cache()
n = sum(sizes)
grads = [torch.empty(s, dtype=torch.bfloat16, device=dev).normal_(0, 1e-3) for s in sizes]
flat = torch.zeros(sum((s + 3) // 4 * 4 for s in sizes), dtype=torch.float32, device=dev)
accs, off = [], 0
for s in sizes:
    accs.append(flat[off:off + s])
    off += (s + 3) // 4 * 4
refs = grad_accum.chunk_refs(sizes)
chunks = torch.tensor(refs, dtype=torch.int32, device=dev).reshape(-1, 2)
partials = torch.empty(len(refs), dtype=torch.float64, device=dev)
stream = torch.cuda.current_stream().cuda_stream


def accum_table(mode):
    g = [t.data_ptr() for t in grads]
    return torch.tensor([g, [a.data_ptr() for a in accs], list(sizes), [mode] * len(sizes), g], dtype=torch.int64, device=dev)


tables = {name: accum_table(mode) for name, mode in (("SET", grad_accum.MODE_SET), ("ADD", grad_accum.MODE_ADD), ("FINISH", grad_accum.MODE_FINISH))}
sumsq_table = torch.tensor([[0] * len(sizes), [t.data_ptr() for t in grads], [0] * len(sizes), [0] * len(sizes), list(sizes)],
                           dtype=torch.int64, device=dev)  # optim.ROW_G = 1, ROW_NUMEL = 4
BYTES = {"SET": 6, "ADD": 10, "FINISH": 8, "sumsq": 2}


def launch(lib, what):
    if what == "sumsq":
        rc = lib.mi_sumsq_bf16_multi(sumsq_table.data_ptr(), len(sizes), chunks.data_ptr(), len(refs), CHUNK, partials.data_ptr(), stream)
    else:
        rc = lib.mi_grad_accum_multi(tables[what].data_ptr(), len(sizes), chunks.data_ptr(), len(refs), CHUNK, stream)
    _lib.check(rc, what)


def reset():
    """FINISH writes the rounded sum over g: start every timing from the same small values."""
    for t in grads:
        t.normal_(0, 1e-3)
    flat.zero_()


def time_ms(lib, what, iters=10):
    reset()
    launch(lib, what)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        launch(lib, what)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


cur = _lib.load()
print(f"{len(sizes)} tensors, {n / 1e9:.3f} B elements, {len(refs)} chunks of {CHUNK}", flush=True)
for what in ("SET", "ADD", "FINISH", "sumsq"):
    ms = time_ms(cur, what)
    print(f"{what:7s} {ms * 1e3:9.1f} us  {n * BYTES[what] / ms / 1e9:6.2f} TB/s at {BYTES[what]} B/element", flush=True)

other_path = os.environ.get("MI_ACCUM_AB_LIB") or os.path.join(os.path.dirname(_lib.LAB_LIB_PATH), "libmi_fp8_accum_ab.so")
if os.path.exists(other_path):
    # interleaved A/B in one process: this build (kept) against the other policy, and this build against itself (noise).  SET and
    # ADD store only the fp32 sums (kept: plain, other: nontemporal), FINISH only the bf16 result (kept: nontemporal, other: plain)
    libs = {"kept": cur, "other": _lib._bind(other_path, _lib.SIGNATURES), "kept2": cur}
    rounds = 5
    for what in ("SET", "ADD", "FINISH"):
        keys, tot = list(libs), {k: 0.0 for k in libs}
        for r in range(rounds):
            for k in keys[r % 3:] + keys[:r % 3]:
                tot[k] += time_ms(libs[k], what, iters=5)
        ms = {k: tot[k] / rounds for k in keys}
        print(f"store policy A/B {what:7s} kept {ms['kept'] * 1e3:9.1f} us  other {ms['other'] * 1e3:9.1f} us  "
              f"other/kept {ms['other'] / ms['kept']:.4f}  kept2/kept {ms['kept2'] / ms['kept']:.4f}", flush=True)
else:
    print(f"no {other_path}: store-policy A/B skipped (make -C llm_fp8_amd/csrc accum_ab)", flush=True)
