"""GPU box: the reference's multi-GPU wrappers (FSDP FULL_SHARD per decoder layer, DDP) around the FP8 model, launched
exactly like the driver launches bench.py (torch.distributed.run, nccl = RCCL), at world size 1 -- the single GPU of
the box.  Exercises flat-parameter views, hooks, clip_grad_norm_ and the amax arenas under the wrappers."""
import json
import os
import subprocess
import sys

import pytest
import socket

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port() -> str:
    """A rendezvous port nobody holds right now: consecutive parametrised cases otherwise re-bind one fixed port seconds after the
    previous torchrun closed it (one run of the sharded cases once sat in rendezvous until the outer timeout)."""
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as sk:
        sk.bind(("127.0.0.1", 0))
        return str(sk.getsockname()[1])



@pytest.mark.parametrize("mode,scenario", [("fsdp_full", "default"), ("ddp", "default"), ("fsdp_full", "mxfp8"),
                                           ("replicated", "default"), ("replicated", "mxfp8")])
def test_train_harness_under_wrappers_world1(dev, mode, scenario):
    # replicated: the gradient-arena wrapper with its RCCL all-reduces forced on at world size 1 (stream hand-over, hooks)
    env = dict(os.environ, LLM_FP8_AMD_FORCE_DIST="1", HSA_ENABLE_IPC_MODE_LEGACY="0", LLM_FP8_AMD_FORCE_COLLECTIVES="1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1", "--master-addr", "127.0.0.1",
           "--master-port", _free_port(), "-m", "llm_fp8_amd.train", "--model_name", "llama-3.2-1b", "--num_hidden_layers", "2",
           "--vocab_size", "4096", "--batch_size", "4", "--max_seq_length", "128", "--mixed_precision", "fp8", "--use_te",
           "--fp8_scenario", scenario, "--sharding_mode", mode, "--num_steps", "4", "--learning_rate", "1e-3",
           "--num_warmup_steps", "0", "--repeat_batch"]
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 4 and all(l["loss"] == l["loss"] for l in lines), r.stdout[-2000:]
    assert lines[-1]["loss"] < lines[0]["loss"]


@pytest.mark.parametrize("world,scenario", [(1, "default"), (1, "mxfp8"), (2, "default")])
def test_fsdp_full_shard_matches_the_unwrapped_run(dev, world, scenario):
    """a12 (train_multi_gpu.py:381-460): FSDP FULL_SHARD around each decoder layer must reproduce the unwrapped run -- same loss,
    and per-parameter gradients equal to the (mean over ranks of the) unwrapped gradients: bit for bit at world size 1 (RCCL),
    within the bf16 reduce-scatter's rounding with 2 ranks sharing the box's GPU (gloo transport: RCCL refuses two ranks per device)."""
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    if world == 1:
        env["LLM_FP8_AMD_FORCE_DIST"] = "1"
    else:
        env.update(LLM_FP8_AMD_DIST_BACKEND="gloo", LLM_FP8_AMD_SHARE_DEVICE="1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(world), "--master-addr", "127.0.0.1",
           "--master-port", _free_port(), os.path.join(ROOT, "tests", "fsdp_equiv_worker.py"), scenario]
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    if world == 2 and r.returncode != 0 and ("reduce_scatter" in r.stderr or "not supported" in r.stderr or "NotImplementedError" in r.stderr):
        pytest.skip("this torch build's gloo backend lacks a collective FSDP needs on CUDA tensors: " + r.stderr[-300:])
    assert r.returncode == 0, r.stderr[-3000:]
    outs = sorted((json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")), key=lambda o: o["rank"])
    assert len(outs) == world, r.stdout[-2000:]
    for o in outs:
        assert o["params"] >= 20, o
        assert o["loss"] == o["ref_loss"], o                       # same forward arithmetic: identical loss
        if world == 1:
            assert o["exact"] == o["params"] and o["worst_rel"] == 0.0, o   # nothing to reduce: gradients bit for bit
        else:
            assert o["worst_rel"] <= 2.0 ** -7, o                  # bf16 sum of two bf16 gradients, then x 1/2


@pytest.mark.parametrize("world,scenario", [(2, "default"), (2, "hybrid"), (2, "mxfp8"), (1, "default"), (1, "mxfp8"), (2, "default-bf16"),
                                            (1, "default+nowcast"), (2, "default+nowcast"), (1, "mxfp8+nowcast"), (2, "mxfp8+nowcast"),
                                            (1, "default+skipgrad"), (2, "hybrid+skipgrad"), (1, "default+ckpt")])
def test_sharded_fp8_dp_matches_the_replicated_run(dev, world, scenario):
    """SURVEY.md 8f rank 3 (second half): distributed.ShardedFP8DP, the FULL_SHARD counterpart (train_multi_gpu.py:392-406, :414-445)
    -- bf16 master rows, gradients and AdamW moments of every GEMM weight at 1/world per rank, reduce-scattered wgrads out of
    transient buffers, asynchronous FP8 (+ E8M0 for MXFP8) all-gathers per operand, no gather in backward -- must train exactly
    like the replicated wrapper: identical losses at every step, identical evaluation loss, identical master weights after
    gather_master_weights(); and the RESIDENT state of the sharded weights is 1/world: masters, shard gradients and moments are
    measured from the tensors that exist after training.  `default-bf16` = `--mixed_precision bf16 --use_te` (no outer
    autocast: every layer's own autocast bumps the scale arena, so every sink is stale at every forward and is refreshed from
    the shards -- the stale-master hole of round 2).  2 ranks share the box's GPU (gloo transport); world 1 runs RCCL.

    Routes where the optimiser does NOT rewrite every FP8 copy (the copies must then be refreshed from the shards, not re-gathered
    as they were): `+nowcast` (LLM_FP8_AMD_NO_OPT_WCAST=1), `+skipgrad` (one operand without a gradient at step 2: the replicated
    forward recasts it and deposits its amax, so must the sharded one -- visible in the scale arenas).  Every case compares both
    runs' scale arenas bitwise and checks every current FP8 copy at every forward against a fresh quantisation of the rank's shard.
    `+ckpt`: torch's AdamW is refused for the sharded wrapper, save_pretrained refuses a model without gathered masters, and writes
    the replicated run's tensors after gather_master_weights()."""
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    if world == 1:
        env.update(LLM_FP8_AMD_FORCE_DIST="1", LLM_FP8_AMD_FORCE_COLLECTIVES="1")
    else:
        env.update(LLM_FP8_AMD_DIST_BACKEND="gloo", LLM_FP8_AMD_SHARE_DEVICE="1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(world), "--master-addr", "127.0.0.1",
           "--master-port", _free_port(), os.path.join(ROOT, "tests", "fsdp_fp8_worker.py"), scenario]
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    outs = sorted((json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")), key=lambda o: o["rank"])
    assert len(outs) == world, r.stdout[-2000:]
    for o in outs:
        assert o["sharded_weights"] >= 12, o                 # 2 layers x (q, k, v, proj, fc1, fc2)
        assert o["losses_equal"] and o["eval_equal"] and o["weights_equal"], o
        assert o["arenas_equal"], o                          # scale + amax history: same deposits in both runs
        assert o["sinks"]["checked"] > 0 and o["sinks"]["mismatch"] == 0, o   # the FP8 copies used are this step's bytes
        if not any(f in o["flags"] for f in ("nowcast", "skipgrad")) and not scenario.endswith("-bf16"):
            assert o["sinks"]["train_stale"] == 0, o   # optimiser-written copies: every one gathered after the step, none refreshed
        if "ckpt" in o["flags"]:
            c = o["ckpt"]
            assert c["torch_adamw_refused"] and c["save_before_gather_refused"] and c["files_equal"], o
        assert all(l == l for l in o["losses"]), o
        m = o["mem"]
        assert m["master_bytes"] * world == m["sharded_logical_bytes"], m       # bf16 master rows: exactly 1 / world
        assert m["shard_grad_bytes"] * world == m["sharded_logical_bytes"], m   # persistent gradients: 1 / world
        assert m["shard_moment_bytes"] * world == 2 * m["sharded_logical_bytes"], m  # two bf16 moments per owned element
        assert m["module_param_storage_bytes"] <= 8 * o["sharded_weights"], m   # the modules' Parameters hold no master storage
        assert m["full_grads_alive"] == 0, m                                    # no full-size gradient survives the step
        if world == 2:
            assert o["moment_elems"][1] < 0.75 * o["moment_elems"][0], o   # the decoder's moments are halved (the tied table is not sharded)
    if world == 2:
        assert outs[0]["losses"] != outs[1]["losses"]        # the ranks trained on different data


@pytest.mark.parametrize("scenario", ["default", "mxfp8"])
def test_two_ranks_share_the_gpu_gradient_arena(dev, scenario):
    """Two ranks on the one GPU (gloo transport, CUDA tensors): replicas stay identical through 4 optimiser steps, and the
    reduced gradient is exactly the bf16 mean of the two ranks' local gradients."""
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", LLM_FP8_AMD_DIST_BACKEND="gloo", LLM_FP8_AMD_SHARE_DEVICE="1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", _free_port(), os.path.join(ROOT, "tests", "dp_two_rank_worker.py"), scenario]
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    outs = sorted((json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")), key=lambda o: o["rank"])
    assert len(outs) == 2, r.stdout[-2000:]
    a, b = outs
    assert a["optimizer"] == b["optimizer"] == "ClippedAdamW" and a["buckets"] >= 3
    assert a["checksum"] == b["checksum"] and a["absum"] == b["absum"], "replicas diverged"
    assert a["losses"] != b["losses"]                      # the ranks trained on different data
    assert all(l == l for l in a["losses"] + b["losses"]) and a["losses"][-1] < a["losses"][0]
    for o in outs:
        assert o["worst_grad_err"] == 0.0 and o["aliased"] == o["n_params"] and o["local_differs"] > 0.0, o
        # the tied embedding table: bucket part exact; row-sparse part = aten's deterministic scatter of the all-gathered rows
        # (bitwise), and within bf16 summation error of an exact fp64 scatter
        assert o["table_bitwise"] and o["table_rel_err"] <= 1.0 and o["table_rows_touched"] > 100, o


def test_bench_two_rank_path_on_one_gpu(dev):
    """bench.py launched the way the driver launches it for N = 2 (torch.distributed.run, one JSON line from rank 0), with the
    two ranks sharing the box's GPU over gloo: the N > 1 code path of the bench itself (barriers, max-over-ranks time, the
    resolved parallelism mode), on a 2-layer model."""
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", LLM_FP8_AMD_DIST_BACKEND="gloo", LLM_FP8_AMD_SHARE_DEVICE="1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", _free_port(), os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1", "--layers", "2",
           "--batch", "4", "--full", "--no-cpu-baseline"]
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    out = lines[0]
    assert out["n_gpus"] == 2 and out["scaling"] == "weak" and out["config"]["global_batch"] == 8
    assert out["config"]["parallelism"].startswith("dp2 replicated")
    assert out["value"] > 0 and abs(out["value"] - 8 * 512 / (out["ms_per_step"] * 1e-3)) < 1e-6 * out["value"]
    assert out["final_loss"] == out["final_loss"] and "roofline" in out and "cpu_baseline" not in out
