"""Worker of tests/test_step_guard_dist_gpu.py: launched by torch.distributed.run.  The comparison of tests/fsdp_fp8_worker.py
(distributed.ShardedFP8DP against distributed.GradArenaDP on the same data: identical losses, evaluation loss, master weights and
scale arenas; every current FP8 copy checked at every forward) with the gradient of step 2 of 4 POISONED on every rank: one element
of the final norm's weight gradient is +Inf, so the norm is Inf, the step guard of optim.ClippedAdamW drops the step on every rank
alike, and the FP8 copies the sharded run gathers after that step are the ones the optimiser re-emitted from the unchanged rows.
Prints one JSON line per rank."""
import json
import os
import sys

import torch
import torch.distributed as dist

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from llm_fp8_amd import train  # noqa: E402
from tests.fsdp_fp8_worker import _arena_diffs, _deterministic_hf_rmsnorm, run  # noqa: E402

_create_optimizer = train.create_optimizer
SKIPPED = []  # per run: (skipped_steps, guard active)


def create_optimizer_poisoning_step_2(model, cfg):
    opt, sched = _create_optimizer(model, cfg)
    inner = model
    while isinstance(getattr(inner, "module", None), torch.nn.Module):
        inner = inner.module
    target = dict(inner.named_parameters())["model.norm.weight"]
    inner_step, n_step = opt.step, [0]

    def step(*a, **k):
        if n_step[0] == 1:
            assert target.grad is not None
            target.grad.view(-1)[5] = float("inf")
        n_step[0] += 1
        out = inner_step(*a, **k)
        if n_step[0] == 4:
            SKIPPED.append((int(opt.skipped_steps.item()), bool(opt._guard_active())))
        return out
    opt.step = step
    return opt, sched


def main():
    scenario = sys.argv[1]
    rank, local, world, device = train.setup_distributed()
    _deterministic_hf_rmsnorm()
    train.create_optimizer = create_optimizer_poisoning_step_2
    l_rep, e_rep, w_rep, a_rep, _, _ = run("replicated", scenario, rank, device)
    l_sh, e_sh, w_sh, a_sh, info, _ = run("fsdp_fp8", scenario, rank, device)
    arena_diffs = [[when] + d for when, a, b in zip(("after training", "after evaluation"), a_rep, a_sh) for d in _arena_diffs(a, b)]
    print(json.dumps({"rank": rank, "world": world, "losses_equal": l_rep == l_sh, "eval_equal": e_rep == e_sh,
                      "weights_equal": bool(torch.equal(w_rep, w_sh)), "weights_finite": bool(torch.isfinite(w_sh.view(torch.bfloat16).float()).all()),
                      "arenas_equal": not arena_diffs and len(a_rep) == len(a_sh) == 2, "arena_diffs": arena_diffs,
                      "losses": l_sh, "losses_rep": l_rep, "eval": [e_rep, e_sh], "skipped": SKIPPED,
                      "sharded_weights": info.get("sharded_weights", 0),
                      "sinks": {k: info.get("sinks_" + k) for k in ("checked", "mismatch", "stale", "train_stale")}}), flush=True)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
