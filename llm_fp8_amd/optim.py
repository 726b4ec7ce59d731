"""`ClippedAdamW`: the reference's `clip_grad_norm_(params, max_norm)` + `AdamW(fused=True).step()` pair
(train_fp8.py:288-291) as two streaming HIP passes: one reproducible squared-norm reduction over the gradients and one
AdamW update with the clip coefficient folded in (the gradients are never rescaled in place), each ONE multi-tensor launch
per parameter group (device tables of tensor addresses + a chunk list).  bf16 parameters with bf16
`exp_avg` / `exp_avg_sq`, fp32 math -- the state layout of torch's fused AdamW, so `state_dict()` is interchangeable.
`state_dtype=torch.float32` keeps an fp32 master weight and fp32 moments behind the same passes instead (`ClippedAdamW`);
`stochastic_rounding=True` keeps the bf16 layout and rounds the weight and both moments stochastically."""
from __future__ import annotations

import os
from typing import Optional

import torch

from . import _lib
from .pytorch.module import MXWeightSink, WeightSink, stepped_tensor

CHUNK = 65536  # elements per workgroup of the multi-tensor kernels (128 KiB of bf16)
TILE = 128  # a sink tensor's chunks are TILE x TILE tiles of the weight matrix

# Rows of the device table [rows, tensors] int64, the one contract between this file and the kernels.  include/mi_fp8.h states the
# layout (mi_adamw_cast_bf16_multi ff.), csrc/mi_optim.hip's `TabRow` carries the same numbers.  Rows 6..11 are the sink's own
# (WeightSink.table_rows / MXWeightSink.table_rows); 12 rows with bf16 state, 13 with fp32 state, 14 with stochastic rounding.
ROW_P, ROW_G, ROW_EXP_AVG, ROW_EXP_AVG_SQ, ROW_NUMEL, ROW_COLS, ROW_SINK, ROW_SINK_END = 0, 1, 2, 3, 4, 5, 6, 12
ROW_Y, ROW_YT = 6, 7  # per-tensor sink: the FP8 copy and its transpose (what MI_DEBUG_SINK masks off)
ROW_MASTER = ROW_SR_BASE = 12  # fp32 state: the master weight | stochastic rounding: global index of the tensor's first element
ROW_SR_KEY = 13


def chunk_refs(sizes, shapes, sinks):
    """(flat, cast) chunk lists [(tensor, chunk)] of one table: `flat` cuts every tensor into CHUNK elements; `cast` walks a tensor
    with a sink in TILE x TILE tiles (row-major over the tiles) and leaves the others their flat chunks."""
    flat, cast = [], []
    for t, (n, shape, s) in enumerate(zip(sizes, shapes, sinks)):
        own = [(t, c) for c in range((n + CHUNK - 1) // CHUNK)]
        flat.extend(own)
        if s is not None:
            own = [(t, c) for c in range(((shape[0] + TILE - 1) // TILE) * ((shape[1] + TILE - 1) // TILE))]
        cast.extend(own)
    return flat, cast


def table_rows(addrs, sizes, shapes, sinks, mode, sr_keys=None):
    """The table as a list of rows.  `addrs`: per tensor the addresses of (p, grad, exp_avg, exp_avg_sq, master); `sinks`: per tensor
    None or (sink, first row in the operand, rows); `mode`: "bf16" | "fp32" | "bf16_sr"; `sr_keys`: per tensor (key, element base)."""
    rows = [[a[r] for a in addrs] for r in range(ROW_NUMEL)] + [list(sizes)] + [[0] * len(sizes) for _ in range(ROW_COLS, ROW_SINK_END)]
    dbg = os.environ.get("MI_DEBUG_SINK", "full")  # tools/bench_adamw.py: mask the FP8 outputs off (timing only)
    for t, (shape, s) in enumerate(zip(shapes, sinks)):
        if s is None:
            continue
        sink, r0, _ = s
        rows[ROW_COLS][t] = shape[1]
        for r, x in zip(range(ROW_SINK, ROW_SINK_END), sink.table_rows(r0, shape[1])):
            rows[r][t] = x
        if sink.kind == 0 and dbg in ("none", "noT"):
            rows[ROW_YT][t] = 0
            if dbg == "none":
                rows[ROW_Y][t] = 0
    if mode == "fp32":
        rows.append([a[4] for a in addrs])  # ROW_MASTER
    elif mode == "bf16_sr":
        for s, (_, base) in zip(sinks, sr_keys):
            if s is not None and base % 8:
                raise ValueError(f"ClippedAdamW: element base {base} of a weight with an FP8 sink must be a multiple of 8")
        rows.append([base for _, base in sr_keys])  # ROW_SR_BASE
        rows.append([key for key, _ in sr_keys])    # ROW_SR_KEY
    return rows


# (mode, the partition walks the cast list) -> (entry point for sink kind 0 / 1, the plan's chunk list, how many of (sink kind, seed)
# follow `step` in the argument list, what to tell _lib.require where the entry point is younger than the ABI version)
_LAUNCH = {("bf16", False): (("mi_adamw_bf16_multi",) * 2, "chunks", 0, None),
           ("bf16", True): (("mi_adamw_cast_bf16_multi", "mi_adamw_mxcast_bf16_multi"), "chunks_cast", 0, None),
           ("fp32", True): (("mi_adamw_f32_multi",) * 2, "chunks_cast", 1, "ClippedAdamW(state_dtype=torch.float32)"),
           ("bf16_sr", True): (("mi_adamw_sr_bf16_multi",) * 2, "chunks_cast", 2, "ClippedAdamW(stochastic_rounding=True)")}

GUARD_REVISION = 5  # include/mi_fp8.h: from this revision on the update kernels take a non-finite *grad_scale as "skip"


def guarded_clip_coefficient(total_sq: torch.Tensor, max_norm: float):
    """(norm, coefficient) from the float64 sum of the squared gradients: `norm` = its root rounded once to fp32, `coefficient`
    [1] fp32 = clip_grad_norm_'s `(max_norm / (norm + 1e-6)).clamp(max=1)` where the norm is finite -- bit for bit -- and NaN
    where it is Inf or NaN, which the update kernels read as "skip this step".  `norm - norm` is +0 for a finite norm and NaN
    otherwise, and the coefficient of a finite norm is positive, so adding it changes no bit.  Torch ops only, no host sync."""
    norm = total_sq.sqrt().to(torch.float32)
    coef = (max_norm / (norm + 1e-6)).clamp(max=1.0) + (norm - norm)
    return norm, coef.reshape(1)


class ClippedAdamW(torch.optim.Optimizer):
    """`state_dtype` is the precision the optimiser state is KEPT in between steps (a step is evaluated in fp32 for bf16 state and in fp64 for fp32 state).

    `torch.bfloat16` (default): torch's fused-AdamW layout.  The updated weight is rounded straight back into the bf16 parameter,
    so an update below half a bf16 ulp of the weight (most of them at lr ~ 1e-5) is lost, and `exp_avg_sq` stalls likewise.

    `torch.float32`: per parameter an fp32 `master` weight and fp32 `exp_avg` / `exp_avg_sq` (+8 bytes per parameter).  Every
    parameter of the optimiser is handled this way.  The update reads and writes the master; the bf16 parameter becomes an
    OUTPUT of the step, `p = RNE_bf16(master)`, and the FP8 copies of the weight sinks are quantised from that rounded value
    as in the default mode.  The master is seeded from `p.float()` when the state is created, and again whenever somebody else
    wrote the parameter since this optimiser's last step (a checkpoint load, `copy_` from another model): that is detected by
    `p._version`, and such a write DISCARDS the fp32 residue of that tensor -- the step starts from the value written.  A write
    that autograd's version counter does not see (`p.data.copy_(...)`, a raw kernel) is not detected, here as for the FP8 weight
    copies: the next step overwrites it from the master.  `load_state_dict` keeps the three tensors in fp32 and trusts a loaded
    master (load the model's weights BEFORE the optimiser state, or the load counts as an external write).

    `stochastic_rounding=True` (bf16 state only; `mi_adamw_sr_bf16_multi`): the layout of the default mode, but the updated weight,
    `exp_avg` and `exp_avg_sq` are rounded to bf16 stochastically -- fp32 bits b become `(b + r) >> 16` with 16 random bits r -- so
    an update below half a bf16 ulp moves the weight with the matching probability and `exp_avg_sq` decays, at no extra memory.
    The bits come from a counter-based generator (Philox4x32-10) keyed by `sr_seed` and counted by the parameter's `step`, a tensor
    key and the element's index: a run is reproducible, a resumed run continues the same stream, and a row shard draws the bits
    its rows would draw in the whole weight.  Key and first element index of a tensor are `p._mi_sr_key = (key, base)` when set,
    else (position of the parameter over the param groups, 0).  With fp32 state the master carries the residue and
    `p = RNE(master)` is right: the combination is refused.  `stochastic_rounding` and `sr_seed` are kept in the param groups
    (and so in `state_dict()`) only in this mode.

    `skip_nonfinite` (the step guard): a step whose gradient norm is Inf or NaN is DROPPED on the device, as AMP's GradScaler
    drops one, instead of writing NaN into every weight, moment and FP8 copy.  The clip coefficient of such a step is NaN
    (`guarded_clip_coefficient`) and the update kernels read a non-finite coefficient as "skip" (include/mi_fp8.h, revision 5):
    parameter, moments and master are not written; the FP8 / MXFP8 copies of the weight sinks are still emitted, from the
    unchanged weight with the current scale.  No launch is added and the host never waits.  `None` (default): on where the
    loaded library has revision >= 5, off with an older build (LLM_FP8_AMD_LIB, for A/B timing); `True`: an older library is
    refused; `False`: off, a non-finite norm poisons the state as it always did.  The guard needs the norm: with
    `max_grad_norm=None` it is inactive whatever the keyword says, and the launch sequence is unchanged.
    `last_step_skipped` is a 0-dim bool tensor on the device saying whether the last `step()` was dropped (None while the guard
    is inactive) and `skipped_steps` an int64 device counter of the dropped steps (None before the first guarded step); the
    optimiser never reads either, and neither is part of `state_dict()`.  The host does not know that a step was dropped, so
    everything it does after a step happens as after any other: `state["step"]` counts the dropped step (the bias corrections
    and the stochastic-rounding stream move on, and so does the caller's LR scheduler), the sinks are stamped current,
    `p._version` moves and `master_version` follows it."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, max_grad_norm: Optional[float] = 1.0,
                 state_dtype: torch.dtype = torch.bfloat16, stochastic_rounding: bool = False, sr_seed: int = 0,
                 skip_nonfinite: Optional[bool] = None):
        if state_dtype not in (torch.bfloat16, torch.float32):
            raise ValueError(f"ClippedAdamW: state_dtype must be torch.bfloat16 or torch.float32, not {state_dtype!r}")
        if stochastic_rounding and state_dtype == torch.float32:
            raise ValueError("ClippedAdamW: stochastic_rounding=True is for bf16 state; with state_dtype=torch.float32 the master "
                             "weight carries the residue and p = RNE(master) is the right rounding")
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)
        self._sr = bool(stochastic_rounding)
        self.sr_seed = int(sr_seed) & 0xFFFFFFFFFFFFFFFF
        if self._sr:
            defaults.update(stochastic_rounding=True, sr_seed=self.sr_seed)
        super().__init__(params, defaults)
        self.max_grad_norm = max_grad_norm
        self.state_dtype = state_dtype
        self._f32 = state_dtype == torch.float32
        self._mode = "fp32" if self._f32 else "bf16_sr" if self._sr else "bf16"  # train.OPTIMIZER_STATES
        self._plans = {}
        self.last_grad_norm: Optional[torch.Tensor] = None
        if skip_nonfinite not in (None, True, False):
            raise ValueError(f"ClippedAdamW: skip_nonfinite must be None, True or False, not {skip_nonfinite!r}")
        self.skip_nonfinite = skip_nonfinite
        self.last_step_skipped: Optional[torch.Tensor] = None
        self.skipped_steps: Optional[torch.Tensor] = None
        if skip_nonfinite:
            self._guard_active()  # refuse an older library now, not at the first step

    def _guard_active(self) -> bool:
        """Whether step() forms the guarded coefficient: there is a norm, the keyword allows it and the library's kernels know
        the contract."""
        if self.max_grad_norm is None or self.skip_nonfinite is False:
            return False
        rev = _lib.revision()
        if rev >= GUARD_REVISION:
            return True
        if self.skip_nonfinite:
            raise RuntimeError(f"ClippedAdamW(skip_nonfinite=True) needs update kernels that skip on a non-finite grad_scale, which "
                               f"{_lib.LIB_PATH} (ABI {_lib.ABI_VERSION} revision {rev}) does not have: it was built before revision "
                               f"{GUARD_REVISION}; rebuild it, or unset LLM_FP8_AMD_LIB")
        return False

    def _grads(self):
        out = []
        for group in self.param_groups:
            for p in group["params"]:
                if p.grad is not None:
                    if not (p.is_cuda and p.dtype == torch.bfloat16 and p.grad.dtype == torch.bfloat16):
                        raise RuntimeError("ClippedAdamW handles bf16 parameters resident on the GPU only")
                    out.append((group, p))
        return out

    CHUNK, TILE = CHUNK, TILE

    def _sink_of(self, p, cls=WeightSink):
        """(sink, row offset, rows) when the FP8 copies of this weight are kept current by the optimiser: `cls` = module.WeightSink
        (delayed scaling) or module.MXWeightSink."""
        if os.environ.get("LLM_FP8_AMD_NO_OPT_WCAST") == "1":  # the switch of module.weight_sinks_enabled: the forward casts
            return None
        s = getattr(p, cls.attr, None)
        sh = getattr(p, "_mi_shard_of", None)
        if sh is not None:  # a row shard of a master weight (distributed.ShardedFP8DP): rows [r0, r0 + n) of the full operand part
            full, sr0, sn = sh
            fs = getattr(full, cls.attr, None)
            s = None if fs is None else (fs[0], fs[1] + sr0, sn)
        if s is None or not p.is_contiguous() or p.dim() != 2 or not self._aligned16(p):
            return None
        sink, r0, n = s
        u = cls.unit
        if n != p.shape[0] or sink.w8.shape[1] != p.shape[1] or p.shape[0] % u or p.shape[1] % u:
            return None
        if cls is MXWeightSink and r0 % u:  # the E8M0 scales of the column blocks are per 32 rows of the OPERAND
            return None
        return s

    def _mx_sink_of(self, p):
        return self._sink_of(p, MXWeightSink)

    def _aligned16(self, p) -> bool:
        """The tile path of the *_cast kernels issues 16-byte loads / stores on the parameter, its gradient, both moments and
        (fp32 state) the master unconditionally; a tensor at an odd storage offset (a loaded optimiser state, a `.grad` view)
        takes the flat path."""
        st = self.state.get(p, {})
        others = (p.grad, st.get("exp_avg"), st.get("exp_avg_sq"), st.get("master") if self._f32 else None)
        return p.data_ptr() % 16 == 0 and all(t is None or t.data_ptr() % 16 == 0 for t in others)

    def _sr_key(self, p):
        """(tensor key, global index of the first element) of the stochastic-rounding generator for `p`."""
        k = getattr(p, "_mi_sr_key", None)
        if k is None:
            index = getattr(self, "_sr_index", None)
            if index is None or id(p) not in index:
                index = self._sr_index = {id(q): i for i, q in enumerate(q for g in self.param_groups for q in g["params"])}
            k = (index[id(p)], 0)
        key, base = int(k[0]), int(k[1])
        if not (0 <= key < 1 << 30 and base >= 0):
            raise ValueError(f"ClippedAdamW: _mi_sr_key {k!r}: the tensor key must be in [0, 2^30) and the element base >= 0")
        return key, base

    def _plan(self, group_items, sinks, dev, mx=False):
        """Device tables of one parameter group for the multi-tensor kernels; `sinks` = per tensor None or (sink, row offset, rows),
        of the kind `mx` says.  The chunk lists only depend on the tensor sizes (and on which tensors have an FP8 sink) and are built
        once; the address table is re-uploaded when an address changed (gradients are new tensors every step, though the caching
        allocator usually hands back the same blocks)."""
        # one plan per PARTITION (the parameters of a group that share a step count), not per group: two partitions of one
        # group must not share address table / partial sums
        key = (id(group_items[0][0]), tuple(id(p) for _, p in group_items), mx)
        sizes = tuple(p.numel() for _, p in group_items)
        shapes = [p.shape for _, p in group_items]
        sink_sig = tuple(None if s is None else (id(s[0]), s[1]) for s in sinks)
        plan = self._plans.get(key)
        if plan is None or plan["sizes"] != sizes or plan["sink_sig"] != sink_sig:
            refs, refs_cast = chunk_refs(sizes, shapes, sinks)
            # mi_adamw_f32_multi and mi_adamw_sr_bf16_multi always walk the cast list
            any_sink = self._mode != "bf16" or any(s is not None for s in sinks)
            nrows = {"bf16": ROW_MASTER, "fp32": ROW_MASTER + 1, "bf16_sr": ROW_SR_KEY + 1}[self._mode]
            plan = {"sizes": sizes, "sink_sig": sink_sig, "chunks": torch.tensor(refs, dtype=torch.int32).to(dev), "n_chunks": len(refs), "addr": None,
                    "chunks_cast": torch.tensor(refs_cast, dtype=torch.int32).to(dev) if any_sink else None, "n_chunks_cast": len(refs_cast),
                    "table": torch.empty((nrows, len(sizes)), dtype=torch.int64, device=dev),
                    "host": [torch.empty((nrows, len(sizes)), dtype=torch.int64).pin_memory() for _ in range(2)], "flip": 0,
                    "uploaded": [None, None],
                    "partials": torch.empty(len(refs), dtype=torch.float64, device=dev)}
            self._plans[key] = plan
        addrs = [(p.data_ptr(), p.grad.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(), st["master"].data_ptr() if self._f32 else None)
                 for p, st in ((p, self.state[p]) for _, p in group_items)]
        rows = table_rows(addrs, sizes, shapes, sinks, self._mode, [self._sr_key(p) for _, p in group_items] if self._sr else None)
        plan["sinks"] = sinks
        plan["mx"] = mx
        if plan["addr"] != rows:
            # two pinned staging buffers, each guarded by an event recorded behind its last upload: the host may run several
            # steps ahead of the device, and rewriting a buffer whose async H2D copy has not run yet would hand the kernels
            # the addresses of a LATER step
            slot = plan["flip"]
            plan["flip"] ^= 1
            if plan["uploaded"][slot] is not None:
                plan["uploaded"][slot].synchronize()
            host = plan["host"][slot]
            host.copy_(torch.tensor(rows, dtype=torch.int64))
            plan["table"].copy_(host, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record()
            plan["uploaded"][slot] = ev
            plan["addr"] = rows
        return plan

    def _seed_master(self, p, state):
        """fp32 state: the master exists, is fp32, and goes with the parameter as it is now.  An external write of `p` since our
        last step (its version moved) re-seeds the master IN PLACE from the value written: the fp32 residue is gone."""
        master = state.get("master")
        if master is None or master.dtype != torch.float32 or master.shape != p.shape or master.device != p.device:
            state["master"] = p.detach().to(torch.float32, memory_format=torch.preserve_format, copy=True)
        elif state.get("master_version") != p._version:
            master.copy_(p.detach())
        else:
            return
        state["master_version"] = p._version

    @torch.no_grad()
    def load_state_dict(self, state_dict):
        """torch.optim.Optimizer.load_state_dict casts every floating state tensor to the PARAMETER's dtype, which would turn an
        fp32 master and fp32 moments back into bf16.  fp32 mode takes the three tensors from `state_dict` itself, in fp32 (a bf16-mode
        state is upcast and the master seeded from `p`); bf16 mode keeps torch's behaviour and drops the master of an fp32-mode
        state.  A loaded master is trusted: it is taken to go with the parameters as they are at this moment."""
        super().load_state_dict(state_dict)
        for group in self.param_groups:  # the mode is this optimiser's; the seed of a saved stochastic-rounding run is kept
            if self._sr:
                group["stochastic_rounding"] = True
                group.setdefault("sr_seed", self.sr_seed)
            else:
                group.pop("stochastic_rounding", None)
                group.pop("sr_seed", None)
        if not self._f32:
            for st in self.state.values():
                st.pop("master", None)
                st.pop("master_version", None)
            return
        saved_ids = [i for g in state_dict["param_groups"] for i in g["params"]]
        ours = [p for g in self.param_groups for p in g["params"]]
        for pid, p in zip(saved_ids, ours):
            src = state_dict["state"].get(pid)
            if src is None:
                continue
            st = self.state[p]
            for k in ("exp_avg", "exp_avg_sq", "master"):
                if torch.is_tensor(src.get(k)):
                    st[k] = src[k].to(device=p.device, dtype=torch.float32)
            if "master" in st:
                st["master_version"] = p._version
            else:
                self._seed_master(p, st)

    def _launch(self, lib, plan, n_tensors, coef_ptr, group, step, st):
        """The update of one plan: fp32 state also passes the partition's sink kind, stochastic rounding the kind and the group's seed."""
        names, chunks, n_extra, _ = _LAUNCH[self._mode, plan["chunks_cast"] is not None]
        kind = 1 if plan["mx"] else 0
        b1, b2 = group["betas"]
        rc = getattr(lib, names[kind])(plan["table"].data_ptr(), n_tensors, plan[chunks].data_ptr(), plan["n_" + chunks], CHUNK, coef_ptr,
                                       float(group["lr"]), b1, b2, group["eps"], group["weight_decay"], step,
                                       *(kind, int(group.get("sr_seed", self.sr_seed)) & 0xFFFFFFFFFFFFFFFF)[:n_extra], st)
        _lib.check(rc, names[kind])

    @torch.no_grad()
    def step(self, closure=None):
        assert closure is None
        items = self._grads()
        if not items:
            return None
        lib = _lib.load()
        names, _, _, why = _LAUNCH[self._mode, True]
        if why is not None:
            _lib.require(names[0], why)
        dev = items[0][1].device
        st = torch.cuda.current_stream().cuda_stream
        by_group = {}
        for group, p in items:
            state = self.state[p]
            if not state:
                state["step"] = 0
                state["exp_avg"] = torch.zeros_like(p, dtype=self.state_dtype, memory_format=torch.preserve_format)
                state["exp_avg_sq"] = torch.zeros_like(p, dtype=self.state_dtype, memory_format=torch.preserve_format)
            if self._f32:
                for k in ("exp_avg", "exp_avg_sq"):  # the kernel reads 4 bytes per element: never hand it a narrower moment
                    if state[k].dtype != torch.float32:
                        state[k] = state[k].to(torch.float32)
                self._seed_master(p, state)
            if torch.is_tensor(state["step"]):  # a state_dict written by torch's AdamW keeps `step` as a tensor
                state["step"] = int(state["step"].item())
            if not p.grad.is_contiguous():
                p.grad = p.grad.contiguous()
            assert p.is_contiguous()
            by_group.setdefault((id(group), state["step"]), []).append((group, p))
        # The squared norm is taken over the partitions above (ONE fixed summation order, whatever sinks exist); the update of a
        # partition that holds weights with an MXFP8 sink is split in two launches (another kernel and another table layout).
        # Every parameter's sinks are looked up here, once per step: (per-tensor sink, MXFP8 sink).
        fp8 = {id(p): self._sink_of(p) for _, p in items}
        mxs = {id(p): self._sink_of(p, MXWeightSink) for _, p in items}
        plan_of = lambda gi, found, mx=False: self._plan(gi, tuple(found[id(p)] for _, p in gi), dev, mx)
        plans = [(gi, plan_of(gi, fp8)) for gi in by_group.values()]
        updates = []
        for gi, plan in plans:
            gi_mx = [it for it in gi if mxs[id(it[1])] is not None]
            if gi_mx:
                gi_rest = [it for it in gi if mxs[id(it[1])] is None]
                updates.append((gi_mx, plan_of(gi_mx, mxs, True)))
                if gi_rest:
                    updates.append((gi_rest, plan_of(gi_rest, fp8)))
            else:
                updates.append((gi, plan))
        coef_ptr = self.last_step_skipped = None
        if self.max_grad_norm is not None:
            # squared norm: one launch per parameter group, one FLOAT64 partial per 64 Ki-element chunk (exact squares, fp64 sums)
            for gi, plan in plans:
                _lib.check(lib.mi_sumsq_bf16_multi(plan["table"].data_ptr(), len(gi), plan["chunks"].data_ptr(), plan["n_chunks"],
                                                   CHUNK, plan["partials"].data_ptr(), st), "mi_sumsq_bf16_multi")
            # Partials and totals stay in FLOAT64 and the norm is rounded to fp32 once: the wrappers partition the parameters
            # differently (distributed.ShardedFP8DP: one group of row shards + the replicated rest, summed over ranks), and in
            # fp32 the association of those sums moves the last bit of the clip coefficient -- a handful of weights then round
            # differently and a sharded run stops being bitwise the replicated one (seen once the MLP bias fusion changed the
            # gradients' low bits).  In float64 the order only matters below 2^-52 of the total.
            total = shard_total = None
            for gi, plan in plans:
                t = plan["partials"].sum(dtype=torch.float64)
                if gi[0][0].get("sharded", False):  # row shards of ShardedFP8DP: every rank holds different rows
                    shard_total = t if shard_total is None else shard_total + t
                else:
                    total = t if total is None else total + t
            if shard_total is not None:
                import torch.distributed as dist
                grp = next((gi[0][0].get("dp_group") for gi, _ in plans if gi[0][0].get("sharded", False)), None)
                if dist.is_available() and dist.is_initialized() and dist.get_world_size(grp) > 1:
                    dist.all_reduce(shard_total, op=dist.ReduceOp.SUM, group=grp)
                total = shard_total if total is None else total + shard_total
            if self._guard_active():
                # a non-finite norm makes the coefficient NaN, which every update kernel below reads as "skip"
                total, coef = guarded_clip_coefficient(total, self.max_grad_norm)
                self.last_step_skipped = torch.isnan(coef).reshape(())
                if self.skipped_steps is None:
                    self.skipped_steps = torch.zeros((), dtype=torch.int64, device=dev)
                self.skipped_steps += self.last_step_skipped
            else:
                total = total.sqrt().to(torch.float32)
                coef = (self.max_grad_norm / (total + 1e-6)).clamp(max=1.0).reshape(1)  # clip_grad_norm_'s coefficient
            self.last_grad_norm = total
            coef_ptr = coef.data_ptr()
        touched, sinks_seen = set(), {}
        for gi, plan in updates:
            group = gi[0][0]
            for _, p in gi:
                self.state[p]["step"] += 1
            self._launch(lib, plan, len(gi), coef_ptr, group, int(self.state[gi[0][1]]["step"]), st)
            # the kernels write through raw addresses: tell autograd (and every cache keyed on `_version`, wcast.py)
            torch.autograd.graph.increment_version([p for _, p in gi])
            if self._f32:
                for _, p in gi:
                    self.state[p]["master_version"] = p._version  # a later mismatch = somebody else wrote p: re-seed
            touched.update(id(p) for _, p in gi)
            for s in plan["sinks"]:
                if s is not None:
                    sinks_seen[id(s[0])] = s[0]
        for sink in sinks_seen.values():  # copies are current only if EVERY part of the operand was rewritten in this step
            # (a row-sharded part, distributed.ShardedFP8DP, was updated through its shard: this rank's rows of the copies)
            if all(id(stepped_tensor(w)) in touched for w, _, _ in sink.parts):
                sink.mark()
            else:
                sink.stamp = None
        return None
