"""GPU, several processes: the step guard under the data-parallel wrappers (tests/step_guard_worker.py).  The gradient of step 2 of
4 is non-finite on every rank; distributed.GradArenaDP's ranks see the same reduced gradients and distributed.ShardedFP8DP's shard
total is all-reduced before the coefficient is formed, so every rank drops the same step, and the sharded run gathers the FP8 copies
the optimiser re-emitted from the unchanged rows.  The two runs must stay identical, as in
tests/test_distributed_gpu.py::test_sharded_fp8_dp_matches_the_replicated_run, and finite."""
import json
import math
import os
import subprocess
import sys

import pytest

from tests.test_distributed_gpu import ROOT, _free_port

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("world,scenario", [(2, "default"), (1, "mxfp8")])
def test_a_skipped_step_under_the_wrappers(dev, world, scenario):
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("LLM_FP8_AMD_NO_STEP_GUARD", "LLM_FP8_AMD_NO_OPT_WCAST", "LLM_FP8_AMD_TORCH_ADAMW"):
        env.pop(k, None)
    if world == 1:
        env.update(LLM_FP8_AMD_FORCE_DIST="1", LLM_FP8_AMD_FORCE_COLLECTIVES="1")
    else:
        env.update(LLM_FP8_AMD_DIST_BACKEND="gloo", LLM_FP8_AMD_SHARE_DEVICE="1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(world), "--master-addr", "127.0.0.1",
           "--master-port", _free_port(), os.path.join(ROOT, "tests", "step_guard_worker.py"), scenario]
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    outs = sorted((json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")), key=lambda o: o["rank"])
    assert len(outs) == world, r.stdout[-2000:]
    for o in outs:
        assert o["skipped"] == [[1, True], [1, True]], o     # both runs dropped exactly the poisoned step
        assert o["sharded_weights"] >= 12, o
        assert o["losses_equal"] and o["eval_equal"] and o["weights_equal"], o
        assert o["arenas_equal"], o
        assert o["sinks"]["checked"] > 0 and o["sinks"]["mismatch"] == 0, o
        assert o["sinks"]["train_stale"] == 0, o             # the copies of the skipped step were re-emitted and gathered too
        assert len(o["losses"]) == 4 and all(math.isfinite(l) for l in o["losses"] + o["losses_rep"] + o["eval"]), o
        assert o["weights_finite"], o
