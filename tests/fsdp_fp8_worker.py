"""Worker of tests/test_distributed_gpu.py::test_sharded_fp8_dp_*: launched by torch.distributed.run.  distributed.ShardedFP8DP
(`--sharding_mode fsdp_fp8`: row-sharded optimiser + weight cast, FP8 all-gather) against distributed.GradArenaDP (`replicated`)
on the same data: same averaged gradients, same AdamW arithmetic on every row, same FP8 bytes -- so the losses of every step and
the final master weights (after gather_master_weights) must be IDENTICAL.  Prints one JSON line per rank.

Scenario suffixes, joined with `+` (set in-process before either run, so both runs take the same route):
  nowcast   LLM_FP8_AMD_NO_OPT_WCAST=1: the optimiser writes no FP8 copy, every sharded sink is refreshed from the shards;
  skipgrad  at step 2 of 4 one whole GEMM operand (layer 1's fc2 weight; its shard in the sharded run) has no gradient;
  ckpt      also: LLM_FP8_AMD_TORCH_ADAMW=1 must be refused for the sharded wrapper, save_pretrained must refuse the sharded
            model before gather_master_weights() and, after it, write the tensors the replicated run writes.
Every sharded run also checks the gathered FP8 copies at each forward of every FP8 module against a fresh quantisation of this
rank's shard (`_SinkCheck`), and both runs' scale arenas (scale + amax history) are compared bitwise at the end."""
import json
import os
import sys
import tempfile

import torch
import torch.distributed as dist

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from llm_fp8_amd import train  # noqa: E402
from llm_fp8_amd.pytorch.fp8 import FP8GlobalStateManager as G  # noqa: E402


class _MulWeightDeterministic(torch.autograd.Function):
    """`weight * h` of HF's LlamaRMSNorm with a weight gradient that does not depend on timing.  torch's column sum over the tokens
    (reduce_kernel<128, 4, bf16>: partial sums of several workgroups combined by the last one to finish) returned different values
    in ~1 run of 6 when three processes share the GPU, as they do under pytest here (two ranks + the pytest process): 94 of 2048
    elements of `model.norm.weight.grad`, every 4th in a range, on ONE rank, everything upstream bit-identical -- found with the
    MI_DEBUG_SHARD_DUMP traces below.  That is the only torch reduction left on the path in the bf16 + use_te scenario (with FP8 on,
    the final norm is fused into the lm_head); it moved the clip coefficient by a last bit and broke the bitwise comparison of two
    CORRECT runs.  Here: one contiguous row per output element, no cross-workgroup stage."""

    @staticmethod
    def forward(ctx, w, h):
        ctx.save_for_backward(w, h)
        return w * h

    @staticmethod
    def backward(ctx, g):
        w, h = ctx.saved_tensors
        gw = (g.float() * h.float()).reshape(-1, h.shape[-1]).t().contiguous().sum(dim=1).to(w.dtype)
        return gw, g * w


def _deterministic_hf_rmsnorm():
    from transformers.models.llama.modeling_llama import LlamaRMSNorm

    def forward(self, hidden_states):  # LlamaRMSNorm.forward with the last multiply routed through the Function above
        input_dtype = hidden_states.dtype
        hs = hidden_states.to(torch.float32)
        hs = hs * torch.rsqrt(hs.pow(2).mean(-1, keepdim=True) + self.variance_epsilon)
        return _MulWeightDeterministic.apply(self.weight, hs.to(input_dtype))

    LlamaRMSNorm.forward = forward


class _SinkCheck:
    """Forward pre- and post-hooks on every FP8 module of a ShardedFP8DP model: for each sharded sink that is current (`fresh()`)
    when the module starts (the bytes the forward is about to use) and when it ends (after a refresh), this rank's rows must be
    bitwise what the cast kernels make of this rank's shard NOW -- delayed scaling: cast with the sink's scale (no amax deposit),
    plus w8T == w8.T in full; MXFP8: rows of w8, columns of sc / wt8, row blocks of sct.  A stale copy declared current fails
    here even where a loss happens to match.  `train_stale`: sinks a training forward found stale before it started, i.e. that
    the optimiser did not rewrite and the post-step gather did not carry."""

    def __init__(self, dp):
        self.dp, self.checked, self.mismatch, self.stale, self.train_stale, self.handles = dp, 0, 0, 0, 0, []
        for m in dp._fp8_modules:
            self.handles.append(m.register_forward_pre_hook(lambda mod, args: self.check(mod, True)))
            self.handles.append(m.register_forward_hook(lambda mod, args, out: self.check(mod, False)))

    def check(self, m, before: bool):
        from llm_fp8_amd.pytorch import ops
        for k, sink in list(m._wcache.items()):
            if not (isinstance(k, tuple) and k[0] in ("sink", "mxsink")):
                continue
            if not all(getattr(w, "_mi_sharded", None) is not None for w, _, _ in sink.parts):
                continue
            self.dp.wait_operand(sink)
            if not sink.fresh():
                self.stale += 1
                self.train_stale += int(before and m.training)
                continue
            ok = True
            for w, row_off, _n in sink.parts:
                h = w._mi_sharded
                lo, hi = row_off + h.r0, row_off + h.r0 + h.rows
                x = h.shard.data
                if k[0] == "sink":
                    y, _ = ops.cast_amax(x, sink.scale, None, ops.E4M3, want_t=False)
                    ok = ok and torch.equal(sink.w8[lo:hi], y)
                else:
                    y, sc, wt, sct = ops.mxfp8_quantize(x, ops.E4M3, rowwise=True, colwise=True)
                    ok = (ok and torch.equal(sink.w8[lo:hi], y) and torch.equal(sink.sc[:, lo:hi], sc)
                          and torch.equal(sink.wt8[:, lo:hi], wt) and torch.equal(sink.sct[lo // 32:hi // 32], sct))
            if k[0] == "sink":
                ok = ok and torch.equal(sink.w8t, sink.w8.t())
            self.checked += 1
            self.mismatch += int(not ok)

    def remove(self):
        for h in self.handles:
            h.remove()


def _arena_state():
    """scale and the used amax-history columns of every scale arena, as raw bits.  The newest history row holds this rank's
    deposits since the last update, which the next update MAX-reduces over the ranks first -- a sharded rank has deposited the
    amax of ITS weight rows only -- so that row is compared as the update will see it (reduced on a copy)."""
    out = {}
    for k, a in G._arenas.items():
        h = a.hist[:, :a.used].clone()
        if a.used and dist.get_world_size() > 1:
            dist.all_reduce(h[0], op=dist.ReduceOp.MAX)
        out[str(k)] = (a.scale[:a.used].clone().view(torch.int32), h.view(torch.int32))
    return out


def _arena_diffs(a, b) -> list:
    """[arena, what, history rows that differ] for every difference (empty when the arenas are bitwise equal)."""
    if a.keys() != b.keys():
        return [["keys", sorted(a), sorted(b)]]
    out = []
    for k in a:
        if not torch.equal(a[k][0], b[k][0]):
            out.append([k, "scale", int((a[k][0] != b[k][0]).sum())])
        if a[k][1].shape != b[k][1].shape:
            out.append([k, "hist shape", list(a[k][1].shape), list(b[k][1].shape)])
        elif not torch.equal(a[k][1], b[k][1]):
            out.append([k, "hist rows", (a[k][1] != b[k][1]).any(dim=1).nonzero().flatten().tolist()])
    return out


def _files_equal(d0, d1) -> bool:
    from safetensors.torch import load_file
    fs = sorted(f for f in os.listdir(d0) if f.endswith(".safetensors"))
    if not fs or fs != sorted(f for f in os.listdir(d1) if f.endswith(".safetensors")):
        return False
    for f in fs:
        a, b = load_file(os.path.join(d0, f)), load_file(os.path.join(d1, f))
        if a.keys() != b.keys():
            return False
        for k in a:
            if a[k].dtype != b[k].dtype or a[k].shape != b[k].shape:
                return False
            if k.endswith("_extra_state") and a[k].numel():  # FP8 metadata, a torch.save blob: compare what it holds
                import io
                sa, sb = (torch.load(io.BytesIO(t.numpy().tobytes()), weights_only=True) for t in (a[k], b[k]))
                if not all(torch.equal(sa[d][n].view(torch.int32), sb[d][n].view(torch.int32)) for d in ("fwd", "bwd") for n in sa[d]):
                    return False
                continue
            if not torch.equal(a[k].contiguous().view(-1).view(torch.uint8), b[k].contiguous().view(-1).view(torch.uint8)):
                return False
    return True


def run(mode, scenario, rank, device, steps=4, mixed_precision="fp8", flags=(), ckpt_dir=None):
    G.reset()
    cfg = train.TrainingConfig(model_name="llama-3.2-1b", batch_size=4, max_seq_length=128, mixed_precision=mixed_precision,
                               fp8_scenario=scenario, use_te=True, sharding_mode=mode, num_hidden_layers=2,
                               vocab_size=4096, learning_rate=1e-3, num_warmup_steps=0)
    torch.manual_seed(4321)
    model = train.prepare_model(train.create_model(cfg, device), cfg)
    dp = train.wrap_distributed(model, cfg, device)
    opt, sched = train.create_optimizer(dp, cfg)
    dp.train()
    gen = torch.Generator(device=device).manual_seed(70 + rank)
    losses, trace = [], []
    dump = os.environ.get("MI_DEBUG_SHARD_DUMP")
    gsum = []
    if dump:  # per-step checksums of every GEMM weight's gradient rows owned by this rank, taken right before the optimiser consumes them
        world = torch.distributed.get_world_size()
        orig_step = opt.step

        def step_with_dump(*a, **k):
            rec = {}
            for n, p in model.named_parameters():
                h = getattr(p, "_mi_sharded", None)
                sharded_kind = p.dim() == 2 and "embed" not in n and "lm_head" not in n
                if h is not None:
                    g = h.shard.grad
                elif sharded_kind:
                    rows = p.shape[0] // world
                    g = None if p.grad is None else p.grad[rank * rows:(rank + 1) * rows]
                else:
                    g = p.grad
                if g is not None:
                    rec[n] = g.contiguous().view(torch.int16).to(torch.int64).sum() if g.dtype == torch.bfloat16 else g.double().sum()
            gsum.append(rec)
            return orig_step(*a, **k)
        opt.step = step_with_dump
    if "skipgrad" in flags:  # step 2: no gradient for one whole GEMM operand (ClippedAdamW skips it), on every rank
        fc2 = dict(model.named_parameters())["model.layers.1.layernorm_mlp.fc2_weight"]
        h = getattr(fc2, "_mi_sharded", None)
        target = fc2 if h is None else h.shard
        assert (h is not None) == (mode == "fsdp_fp8")
        inner_step, n_step = opt.step, [0]

        def step_skipping(*a, **k):
            if n_step[0] == 1:
                assert target.grad is not None
                target.grad = None
            n_step[0] += 1
            return inner_step(*a, **k)
        opt.step = step_skipping
    check = _SinkCheck(dp) if mode == "fsdp_fp8" else None
    for _ in range(steps):
        loss_t = train.train_step(dp, train.synthetic_batch(cfg, 4096, device, gen), opt, sched, cfg)
        if dump:  # device-side copies only (no host synchronisation that would hide a timing dependence); written out at the end
            trace.append({"loss": loss_t.detach().clone(), "grad_norm": opt.last_grad_norm.detach().clone() if getattr(opt, "last_grad_norm", None) is not None else None,
                          "arenas": {str(k): (a.scale[:a.used].clone(), a.hist[:, :a.used].clone()) for k, a in G._arenas.items()}})
        losses.append(loss_t)
    losses = [l.item() for l in losses]
    arenas = [_arena_state()]
    if dump:
        out = [{"loss": t["loss"].item(), "grad_norm": None if t["grad_norm"] is None else t["grad_norm"].item(),
                "arenas": {k: {"scale": v[0].float().cpu().tolist(), "hist": v[1].float().cpu().tolist()} for k, v in t["arenas"].items()}} for t in trace]
        for t, rec in zip(out, gsum):
            t["grad_checksums"] = {n: float(v.item()) for n, v in rec.items()}
        with open(os.path.join(dump, f"trace_{mode}_{mixed_precision}_{scenario}_r{rank}_{os.getpid()}.json"), "w") as fh:
            json.dump(out, fh)
    # an evaluation pass (FP8 still on inside the layers, as in the reference): must run on the gathered FP8 copies, not on stale masters
    dp.eval()
    with torch.no_grad():
        ev = dp(**train.synthetic_batch(cfg, 4096, device, torch.Generator(device=device).manual_seed(5))).loss.item()
    dp.train()
    arenas.append(_arena_state())
    info = dp.describe()   # BEFORE the masters are materialised: the resident training state
    if check is not None:
        check.remove()
        info.update(sinks_checked=check.checked, sinks_mismatch=check.mismatch, sinks_stale=check.stale,
                    sinks_train_stale=check.train_stale)
    if "ckpt" in flags:
        from llm_fp8_amd import checkpoint
        if mode == "fsdp_fp8":
            os.environ["LLM_FP8_AMD_TORCH_ADAMW"] = "1"
            try:
                train.create_optimizer(dp, cfg)
                info["torch_adamw_refused"] = False
            except RuntimeError:
                info["torch_adamw_refused"] = True
            finally:
                del os.environ["LLM_FP8_AMD_TORCH_ADAMW"]
            try:
                checkpoint.save_pretrained(model, os.path.join(ckpt_dir, "sharded_before_gather"), layout="te")
                info["save_before_gather_refused"] = False
            except RuntimeError:
                info["save_before_gather_refused"] = True
        else:
            checkpoint.save_pretrained(model, os.path.join(ckpt_dir, "replicated"), layout="te")  # TE names: trained MLP biases
    if mode == "fsdp_fp8":
        shard_ids = {id(sp) for sp in dp._shards.values()}
        info["shard_moment_bytes"] = sum(st[k].numel() * st[k].element_size() for p_, st in opt.state.items() if id(p_) in shard_ids
                                         for k in ("exp_avg", "exp_avg_sq"))
        info["full_grads_alive"] = sum(1 for p_ in dp._sharded.values() if p_.grad is not None)
    if hasattr(dp, "gather_master_weights"):
        dp.gather_master_weights()
        if "ckpt" in flags:
            checkpoint.save_pretrained(model, os.path.join(ckpt_dir, "sharded"), layout="te")
    flat = torch.cat([p.detach().reshape(-1).view(torch.int16) for p in model.parameters()]).clone()
    if hasattr(dp, "reshard"):
        dp.reshard()
        assert all(p_.untyped_storage().nbytes() <= 8 for p_ in dp._sharded.values())
    moments = sum(st["exp_avg"].numel() for st in opt.state.values())
    del dp, opt, model
    torch.cuda.empty_cache()
    return losses, ev, flat, arenas, info, moments


def main():
    scenario, *flags = sys.argv[1].split("+")
    unknown = set(flags) - {"nowcast", "skipgrad", "ckpt"}
    assert not unknown, f"unknown scenario suffix(es) {sorted(unknown)}"
    mp = "fp8"
    if scenario.endswith("-bf16"):  # --mixed_precision bf16 --use_te: no outer autocast, every layer's own autocast updates the arena
        scenario, mp = scenario[:-5], "bf16"
    if "nowcast" in flags:
        os.environ["LLM_FP8_AMD_NO_OPT_WCAST"] = "1"
    rank, local, world, device = train.setup_distributed()
    _deterministic_hf_rmsnorm()
    with tempfile.TemporaryDirectory(prefix="fsdp_fp8_ckpt_") as ckpt_dir:
        l_rep, e_rep, w_rep, a_rep, _, mom_rep = run("replicated", scenario, rank, device, mixed_precision=mp, flags=flags,
                                                      ckpt_dir=ckpt_dir)
        l_sh, e_sh, w_sh, a_sh, info, mom_sh = run("fsdp_fp8", scenario, rank, device, mixed_precision=mp, flags=flags,
                                                    ckpt_dir=ckpt_dir)
        arena_diffs = [[when] + d for when, a, b in zip(("after training", "after evaluation"), a_rep, a_sh) for d in _arena_diffs(a, b)]
        ckpt = {}
        if "ckpt" in flags:
            ckpt = {k: info[k] for k in ("torch_adamw_refused", "save_before_gather_refused")}
            ckpt["files_equal"] = _files_equal(os.path.join(ckpt_dir, "replicated"), os.path.join(ckpt_dir, "sharded"))
    print(json.dumps({"rank": rank, "world": world, "flags": flags, "losses_equal": l_rep == l_sh, "eval_equal": e_rep == e_sh,
                      "weights_equal": bool(torch.equal(w_rep, w_sh)),
                      "arenas_equal": not arena_diffs and len(a_rep) == len(a_sh) == 2, "arena_diffs": arena_diffs,
                      "losses": l_sh, "losses_rep": l_rep, "eval": [e_rep, e_sh],
                      "sharded_weights": info.get("sharded_weights", 0), "moment_elems": [mom_rep, mom_sh],
                      "sinks": {k: info.get("sinks_" + k) for k in ("checked", "mismatch", "stale", "train_stale")}, "ckpt": ckpt,
                      "mem": {k: info.get(k) for k in ("sharded_logical_bytes", "master_bytes", "shard_grad_bytes", "shard_moment_bytes",
                                                       "module_param_storage_bytes", "fp8_operand_bytes", "full_grads_alive")}}), flush=True)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
