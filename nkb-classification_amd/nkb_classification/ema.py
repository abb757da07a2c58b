"""Exponential moving average of the model's weights (ModelEmaV2 of the ConvNeXt / DeiT-III recipes) on the flat arena.

The EMA of every parameter is ONE fp32 tensor the size of the parameter arena, advanced by one launch per step
(nkb_optim_step, kind NKB_OPTIM_EMA: e = (d * e) + ((1 - d) * w), 12 bytes per parameter).  Float buffers (BatchNorm running
statistics) follow the same rule through the same entry point, one small launch per buffer; integer buffers are copied.
Validation and checkpoints see the averaged weights through `applied()`, which swaps them into the arena and restores the
raw ones bit for bit.  Under data parallelism every rank advances its own copy from identical weights: no communication.

    model.ema = ModelEma(model, decay=0.9998)       # after parallel.attach; engine.train_epoch then calls model.ema.update()
    with model.ema.applied():
        val_epoch(model, ...)
    torch.save(model.ema.state_dict(), "ema_last.pth")     # the model's own keys: eval.py loads it like any checkpoint

`warmup=True` ramps the decay as d_t = min(decay, (1 + t) / (10 + t)), t the number of updates so far (the rule of timm's
ModelEmaV3 restated from memory: parity unpinned, timm is not a dependency).
"""
from __future__ import annotations

from contextlib import contextmanager

import torch

from . import hip


def ema_decay(decay: float, warmup: bool, t: int) -> float:
    """The decay of update number t (0-based)."""
    return min(decay, (1.0 + t) / (10.0 + t)) if warmup else decay


class ModelEma:
    def __init__(self, model, decay: float = 0.9998, warmup: bool = False, bf16_shadow: bool = False):
        decay = float(decay)
        if not 0.0 <= decay <= 1.0:
            raise ValueError(f"Invalid EMA decay: {decay} (must lie in [0, 1])")
        arena = getattr(model, "arena", None)
        if arena is not None and not arena.still_packed() and hasattr(model, "_pack"):
            device = next(model.parameters()).device        # the arena is packed on the first forward: do it now (as parallel.attach does)
            if device.type == "cuda":
                model._pack(device)
        if arena is None or not arena.still_packed():
            raise NotImplementedError("ModelEma averages the packed parameter arena in one launch and needs a model whose "
                                      "parameters live there, on the GPU; there is no per-tensor torch fallback")
        self.model, self.arena = model, arena
        self.decay, self.warmup = decay, bool(warmup)
        self.num_updates = 0
        self.flat = arena.flat_param.detach().clone()
        self._base = arena.flat_param.data_ptr()
        # bf16 of the averaged weights, written by the same launch (14 B per parameter): applied() then needs no conversion pass
        self.shadow = torch.empty(arena.total, device=arena.device, dtype=torch.bfloat16) if bf16_shadow else None
        self._shadow_fresh = False
        persistent = set(model.state_dict().keys())
        self._buffers = [(name, b) for name, b in model.named_buffers() if name in persistent]
        for name, b in self._buffers:
            if b.is_floating_point() and (b.dtype != torch.float32 or not b.is_contiguous()):
                raise NotImplementedError(f"ModelEma: float buffer {name} must be contiguous fp32, got {b.dtype}")
        self.buffers = [b.detach().clone() for _, b in self._buffers]
        self._saved = None

    # ---- the update -------------------------------------------------------------------------------------------------
    def current_decay(self) -> float:
        return ema_decay(self.decay, self.warmup, self.num_updates)

    @torch.no_grad()
    def update(self):
        """One NKB_OPTIM_EMA launch over the arena and one per float buffer; nothing waits for the device."""
        d = self.current_decay()
        a = self.arena
        if a.flat_param.data_ptr() != self._base or a.total != self.flat.numel():
            raise RuntimeError("ModelEma: the parameter arena was re-packed (model.to() / .float()) after the EMA was built")
        with torch.cuda.device(a.device):
            hip.ema_step(self.flat, a.flat_param, self.shadow, a.total, d)
            for e, (_, b) in zip(self.buffers, self._buffers):
                if b.is_floating_point():
                    if b.numel():
                        hip.ema_step(e, b, None, b.numel(), d)
                else:
                    e.copy_(b)
        self._shadow_fresh = self.shadow is not None
        self.num_updates += 1

    def launches_per_update(self) -> int:
        """nkb_optim_step launches of one update(): the arena's and one per non-empty float buffer."""
        return 1 + sum(1 for _, b in self._buffers if b.is_floating_point() and b.numel())

    # ---- seeing the averaged weights ------------------------------------------------------------------------------------
    def _swap_in(self, flat, buffers):
        a = self.arena
        a.flat_param.copy_(flat)
        for (_, b), src in zip(self._buffers, buffers):
            b.copy_(src)
        a.mark_dirty()

    @contextmanager
    def applied(self):
        """The model computes with the EMA weights and buffers inside the block; the raw ones come back bit for bit on exit,
        also when the block raises."""
        a = self.arena
        with torch.no_grad():
            if self._saved is None:
                self._saved = (torch.empty_like(a.flat_param), [torch.empty_like(b) for _, b in self._buffers])
            saved_flat, saved_buffers = self._saved
            saved_flat.copy_(a.flat_param)
            for dst, (_, b) in zip(saved_buffers, self._buffers):
                dst.copy_(b)
        try:
            with torch.no_grad():
                self._swap_in(self.flat, self.buffers)
                if self._shadow_fresh and a.shadow is not None:
                    a.shadow.copy_(self.shadow)              # the launch's own bf16 of these values: no conversion pass
                    a.shadow_version = a.version
            yield self.model
        finally:
            with torch.no_grad():
                self._swap_in(saved_flat, saved_buffers)

    def state_dict(self):
        """The model's own keys with EMA values: what model.state_dict() returns inside applied(), as copies."""
        with self.applied():
            return {k: v.detach().clone() for k, v in self.model.state_dict().items()}

    @torch.no_grad()
    def load_state_dict(self, state):
        """Inverse of state_dict(): the EMA takes the values of a model state dict; the model itself is left as it was."""
        with self.applied():
            self.model.load_state_dict(state)
            self.flat.copy_(self.arena.flat_param)
            for e, (_, b) in zip(self.buffers, self._buffers):
                e.copy_(b)
        self._shadow_fresh = False
