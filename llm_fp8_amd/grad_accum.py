"""`GradAccumulator`: fp32 gradient accumulation over a window of micro-batches (`--grad_accum_dtype fp32`).

Autograd accumulates into a bf16 `.grad`: the window's gradient is rounded to bf16 after every micro-batch but the first.  Here
every parameter gets an fp32 `main_grad` (the name TE / Megatron users know), ONE multi-tensor launch per micro-batch
(`mi_grad_accum_multi`, include/mi_fp8.h) folds that micro-batch's bf16 gradients into it, and the last launch of the window
rounds the sum to bf16 once, into `.grad`.  The optimiser reads `.grad` as it always did."""
from __future__ import annotations

import torch

from .optim import CHUNK
from .pytorch import ops

# rows of the device table [5, tensors] int64 and the per-tensor modes: include/mi_fp8.h mi_grad_accum_multi
ROW_G, ROW_ACC, ROW_NUMEL, ROW_MODE, ROW_OUT, N_ROWS = 0, 1, 2, 3, 4, 5
MODE_ADD, MODE_SET, MODE_FINISH = 0, 1, 2
ALIGN_ELEMS = 4  # main_grad views start at a multiple of 4 fp32 elements: 16 bytes, the kernel's vector path


def chunk_refs(sizes):
    """[(tensor, chunk)] of one launch: every tensor cut into CHUNK elements."""
    return [(t, c) for t, n in enumerate(sizes) for c in range((n + CHUNK - 1) // CHUNK)]


class GradAccumulator:
    """`accumulate(last)` is called after each micro-batch's backward; see the module docstring.

    Between micro-batches `p.grad` is None (the bf16 dW is freed and the next backward's first write is a plain assignment: no
    `AccumulateGrad` add runs) and `p.main_grad`, an fp32 view into one flat buffer per device, holds the window's sum so far.
    After `accumulate(last=True)` `p.grad` is the window's gradient and `main_grad` is dead: the next window starts by
    overwriting it.  The buffers are allocated at the first use and kept; `bytes()` is their size."""

    def __init__(self, params):
        seen, self.params = set(), []
        for p in params:
            if id(p) not in seen and p.requires_grad:
                seen.add(id(p))
                self.params.append(p)
        # layout: per device, each parameter's first element in the flat buffer
        self._offset, self._total = {}, {}
        for p in self.params:
            off = self._total.get(p.device, 0)
            self._offset[id(p)] = off
            self._total[p.device] = off + (p.numel() + ALIGN_ELEMS - 1) // ALIGN_ELEMS * ALIGN_ELEMS
        self._buffers = {}
        self._content = set()  # id(p) of the parameters whose main_grad holds something of the current window
        self._plans = {}

    def bytes(self) -> int:
        return 4 * sum(self._total.values())

    def has_content(self) -> bool:
        return bool(self._content)

    def reset(self) -> None:
        """Abandon the window: what the main_grads hold is dead.  `.grad` is not touched."""
        self._content.clear()

    def attach(self, optimizer) -> "GradAccumulator":
        """Hang the accumulator on the optimiser as `optimizer.grad_accumulator`; `optimizer.zero_grad()` also abandons the window."""
        optimizer.grad_accumulator = self
        inner = optimizer.zero_grad

        def zero_grad(*args, **kwargs):
            self.reset()
            return inner(*args, **kwargs)

        optimizer.zero_grad = zero_grad
        return self

    def _allocate(self, dev) -> None:
        buf = self._buffers[dev] = torch.empty(self._total[dev], dtype=torch.float32, device=dev)
        for p in self.params:
            if p.device == dev:
                off = self._offset[id(p)]
                p.main_grad = buf[off:off + p.numel()].view(p.shape)

    def _plan(self, sizes, dev):
        """Chunk list (cached by the tuple of sizes), device table and its two pinned staging buffers."""
        plan = self._plans.get((dev, sizes))
        if plan is None:
            refs = chunk_refs(sizes)
            plan = {"chunks": torch.tensor(refs, dtype=torch.int32).reshape(-1, 2).to(dev), "n_chunks": len(refs),
                    "table": torch.empty((N_ROWS, len(sizes)), dtype=torch.int64, device=dev),
                    "host": [torch.empty((N_ROWS, len(sizes)), dtype=torch.int64).pin_memory() for _ in range(2)],
                    "uploaded": [None, None], "flip": 0, "addr": None}
            self._plans[dev, sizes] = plan
        return plan

    def _upload(self, plan, rows) -> None:
        """optim.ClippedAdamW._plan's upload: the host may run ahead of the device, and rewriting a staging buffer whose async
        copy has not run yet would hand the kernel the addresses of a LATER micro-batch -- each buffer waits for its own event."""
        if plan["addr"] == rows:
            return
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

    @torch.no_grad()
    def accumulate(self, last: bool) -> None:
        by_dev = {}
        for p in self.params:
            g, has = p.grad, id(p) in self._content
            if p.numel() == 0 or (g is None and not (last and has)):
                continue
            if not (p.is_cuda and p.dtype == torch.bfloat16 and (g is None or (g.dtype == torch.bfloat16 and g.device == p.device))):
                raise RuntimeError("GradAccumulator handles bf16 parameters with bf16 gradients resident on the GPU only")
            if p.device not in self._buffers:
                self._allocate(p.device)
            if g is not None and not g.is_contiguous():
                g = p.grad = g.contiguous()
            if not last:
                item = (p, g, MODE_ADD if has else MODE_SET, None)
                self._content.add(id(p))
            elif not has:
                continue  # its only contribution came in this very micro-batch: .grad already is the answer
            elif g is not None:
                item = (p, g, MODE_FINISH, g)  # in place, into the last micro-batch's gradient
            else:
                p.grad = out = torch.empty_like(p, memory_format=torch.contiguous_format)
                item = (p, None, MODE_FINISH, out)
            by_dev.setdefault(p.device, []).append(item)
        if last:
            self._content.clear()
        for dev, items in by_dev.items():
            with torch.cuda.device(dev):
                plan = self._plan(tuple(p.numel() for p, _, _, _ in items), dev)
                rows = [[0 if g is None else g.data_ptr() for _, g, _, _ in items],
                        [p.main_grad.data_ptr() for p, _, _, _ in items],
                        [p.numel() for p, _, _, _ in items],
                        [mode for _, _, mode, _ in items],
                        [0 if out is None else out.data_ptr() for _, _, _, out in items]]
                self._upload(plan, rows)
                ops.grad_accum_multi(plan["table"], len(items), plan["chunks"], plan["n_chunks"], CHUNK)
            if not last:
                for p, _, _, _ in items:
                    p.grad = None  # freed behind the launch (the allocator is stream-ordered)
