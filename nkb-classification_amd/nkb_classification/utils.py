"""Optimizer / scheduler factories and small config helpers.

Drop-in for /root/reference/nkb_classification/utils.py: `get_optimizer` (utils.py:10-42) keeps the two
parameter groups (backbone / classifier) with per-group lr and weight decay and the same optimizer
families, but the update itself is one fused HIP launch per group over the model's flat parameter arena
(nkb_optim_step) instead of torch's foreach kernels.  Beyond the reference: `type: "adamw"`, the optional keys
`betas`, `eps`, `momentum`, `dampening`, `nesterov`, `decoupled_weight_decay`, `amsgrad` (refused when true) and
`layer_decay` (one backbone group per transformer block); a config without them builds what the reference builds.
`parse_clip_grad` reads the optional `cfg.clip_grad`.  `get_scheduler` (utils.py:45-61) returns the stock
torch schedulers, which only touch `param_groups[i]["lr"]` on the host.
"""
from __future__ import annotations

import json
import math
import sys
from pathlib import Path

import numpy as np
import torch
from torch.optim import lr_scheduler

from . import hip

_KIND = {"adam": 0, "adamw": 0, "nadam": 1, "radam": 2, "sgd": 3}
# optional cfg.optimizer keys that reach the optimizer's defaults, and the kinds whose torch class takes them
_OPTIONS = {"betas": ("adam", "adamw", "nadam", "radam"), "eps": ("adam", "adamw", "nadam", "radam"),
            "momentum": ("sgd",), "dampening": ("sgd",), "nesterov": ("sgd",),
            "decoupled_weight_decay": ("adam", "radam"), "amsgrad": ("adam", "adamw")}


def _step_scalars(kind: str, state: dict, *, lr: float, beta1: float, beta2: float, eps: float,
                  momentum_decay: float = 4e-3, decoupled: bool = False, momentum: float = 0.0, dampening: float = 0.0,
                  nesterov: bool = False):
    """Advance the per-group step counter and return (kernel kind, (c0, c1, c2, c3)).

    The scalars are the step-dependent coefficients of torch.optim's single-tensor formulas, evaluated in
    double precision on the host exactly as torch does before it hands them to its kernels.  c3 = 1 asks adam / radam for
    decoupled weight decay (adamw is adam with c3 = 1).  sgd reads `momentum`, never `beta1` (callers hand it Adam's betas);
    with a momentum the kernel's beta1 is that momentum, c0 the factor on the gradient in the buffer update, c1 Nesterov.
    """
    step = state["step"] = state.get("step", 0) + 1
    if kind == "sgd":
        if momentum == 0.0:
            return 3, (0.0, 0.0, 0.0, 0.0)
        # torch clones the gradient into the buffer on the first step that has a momentum: no dampening there
        fresh = not state.get("momentum_buffer", False)
        state["momentum_buffer"] = True
        return 3, (1.0 if fresh else 1.0 - dampening, 1.0 if nesterov else 0.0, 0.0, 0.0)
    c3 = 1.0 if (decoupled or kind == "adamw") else 0.0
    bc1 = 1.0 - beta1 ** step
    bc2 = 1.0 - beta2 ** step
    if kind in ("adam", "adamw"):
        return 0, (lr / bc1, math.sqrt(bc2), 0.0, c3)
    if kind == "nadam":
        mu = beta1 * (1.0 - 0.5 * (0.96 ** (step * momentum_decay)))
        mu_next = beta1 * (1.0 - 0.5 * (0.96 ** ((step + 1) * momentum_decay)))
        # torch keeps mu_product in a float32 state tensor (NAdam._init_group), so it is rounded to fp32 every step
        mu_product = state["mu_product"] = float(np.float32(state.get("mu_product", 1.0)) * np.float32(mu))
        return 1, (bc2, lr * (1.0 - mu) / (1.0 - mu_product), lr * mu_next / (1.0 - mu_product * mu_next), 0.0)
    if kind == "radam":
        rho_inf = 2.0 / (1.0 - beta2) - 1.0
        rho_t = rho_inf - 2.0 * step * (beta2 ** step) / bc2
        rect = 0.0
        if rho_t > 5.0:
            rect = math.sqrt((rho_t - 4.0) * (rho_t - 2.0) * rho_inf / ((rho_inf - 4.0) * (rho_inf - 2.0) * rho_t))
        return 2, (bc1, math.sqrt(bc2), rect, c3)
    raise NotImplementedError(kind)


class FusedOptimizer(torch.optim.Optimizer):
    """Adam / AdamW / NAdam(decoupled) / RAdam / SGD (momentum, dampening, Nesterov) with the defaults of the torch class
    of the same name; the math runs in nkb_optim_step.  `options` override those defaults the way the torch constructors'
    keyword arguments do, with torch's validation; like every other hyper-parameter they are read from the group at each
    step, so schedulers that cycle `momentum` or `betas` work.  amsgrad is refused: it needs a third state buffer.

    When every parameter of a group is a view into the model's flat arena (see model.ParamArena) the group is
    updated by ONE launch over the contiguous range, which also refreshes the bf16 shadow weights; otherwise
    each parameter gets its own launch.  `grad_scale` (e.g. 1/world_size) is folded into the kernel.
    `clip_grad_norm_` / `clip_grad_value_` arm the next step(): its launches clip the gradients as they read them.
    """

    def __init__(self, params, kind: str, arena=None, **options):
        self.kind = kind
        # hyper-parameter keys and defaults of the torch optimizer the reference instantiates (utils.py:29-39)
        if kind == "sgd":
            defaults = dict(lr=1e-3, weight_decay=0.0, momentum=0, dampening=0, nesterov=False, maximize=False)
        else:
            defaults = dict(lr=1e-3, weight_decay=1e-2 if kind == "adamw" else 0.0, betas=(0.9, 0.999), eps=1e-8,
                            maximize=False, decoupled_weight_decay=kind in ("nadam", "adamw"))
            if kind == "nadam":
                defaults["momentum_decay"] = 4e-3
            if kind in ("adam", "adamw"):
                defaults["amsgrad"] = False
        for k, val in options.items():
            if kind not in _OPTIONS.get(k, ()):
                raise TypeError(f"optimizer '{kind}' got an unexpected option '{k}'")
            defaults[k] = tuple(val) if k == "betas" else val
        _validate(kind, defaults)
        super().__init__(params, defaults)
        self.arena = arena
        self.grad_scale = 1.0
        self._gstate = [dict() for _ in self.param_groups]

    def _arena_range(self, group):
        """(lo, hi) element range when the group's parameters and gradients tile one arena range, else None."""
        a = self.arena
        if a is None or not a.packed:
            return None
        ps = group["params"]
        if not ps or any(p.grad is None for p in ps):
            return None
        rng = a.range_of(ps)
        if rng is None:
            return None
        lo, hi = rng
        base_p, base_g = a.flat_param.data_ptr(), a.flat_grad.data_ptr()
        if ps[0].data_ptr() != base_p + 4 * a.offset_of(ps[0]) or ps[0].grad.data_ptr() != base_g + 4 * a.offset_of(ps[0]):
            return None
        if ps[-1].grad.data_ptr() != base_g + 4 * a.offset_of(ps[-1]):
            return None
        return lo, hi

    def rollback_last_step(self):
        """Undo the host-side bookkeeping of the most recent step() (its step counters and NAdam's mu_product): the
        gradient scaler found that the device skipped that step (amp.HipGradScaler), and torch does not count skipped steps."""
        if self._prev_gstate is not None:
            self._gstate = self._prev_gstate
            self._prev_gstate = None

    _prev_gstate = None

    # ---- gradient clipping, decided on the device (nkbhip.h: NKB_OPTIM_CLIP_NORM / NKB_OPTIM_CLIP_VALUE) ------------------------
    # torch's idiom `scaler.unscale_(opt); clip_grad_norm_(params); scaler.step(opt)` keeps its place and order, but nothing is
    # scaled between backward and step: the clip methods ARM the next step(), whose launches derive the coefficient from a device
    # record and apply it to each gradient as they read it.  The gradient arena itself stays as backward left it.
    _clip = None              # kind bit of the armed form, cleared by step()
    _clip_rec = None          # device record {skip, bound, P, 0, partials[P]}
    _clip_offsets = None      # int64 device offsets of the P chunks of flat_grad (built once per arena)
    _clip_P = 0
    _clip_bound = None        # host copy of rec[1]
    _clip_rec0_set = False    # rec[0] may hold a scaler's flag from an earlier step

    def _clip_arena(self, what: str):
        a = self.arena
        if a is None or not a.packed or not all(a.owns(p) for g in self.param_groups for p in g["params"]):
            raise NotImplementedError(f"{what} clips inside the fused launches over the packed parameter arena and needs every "
                                      "parameter of every group to live there; there is no torch fallback "
                                      "(torch.nn.utils.clip_grad_norm_ would read the norm back on the host)")
        if self._clip_rec is None or self._clip_rec.device != a.flat_grad.device or self._clip_total != a.total:
            offs = hip.clip_chunk_offsets(a.total)
            self._clip_P, self._clip_total = len(offs) - 1, a.total
            self._clip_offsets = torch.tensor(offs, dtype=torch.int64, device=a.flat_grad.device)
            self._clip_rec = torch.zeros(hip.OPTIM_RECORD_HEAD + self._clip_P, dtype=torch.float32, device=a.flat_grad.device)
            self._clip_rec[2].fill_(float(self._clip_P))
            self._clip_bound, self._clip_rec0_set = None, False
        return a

    _clip_total = -1

    def _clip_set_bound(self, bound: float):
        if self._clip_bound != bound:                   # a device-side fill: the bound changes once per run, if at all
            self._clip_rec[1].fill_(bound)
            self._clip_bound = bound

    @torch.no_grad()
    def clip_grad_norm_(self, max_norm, return_norm=False):
        """torch.nn.utils.clip_grad_norm_(parameters, max_norm) (norm_type 2) for the NEXT step(): one nkb_segment_sumsq pass over the
        gradient arena leaves partial sums of squares in the device record, and every launch of the step scales the gradients it
        reads by min(1, max_norm / (norm + 1e-6)).  Call it after backward (and after scaler.unscale_).  return_norm=True returns the
        total norm as a device scalar; nothing waits for the device."""
        max_norm = float(max_norm)
        if not max_norm >= 0.0:
            raise ValueError(f"Invalid max_norm value: {max_norm}")
        a = self._clip_arena("clip_grad_norm_")
        with torch.cuda.device(a.flat_grad.device):
            self._clip_set_bound(max_norm)
            rec = self._clip_rec
            hip.segment_sumsq(a.flat_grad, self._clip_offsets, self._clip_P, rec[hip.OPTIM_RECORD_HEAD:])
            self._clip = hip.OPTIM_CLIP_NORM
            if return_norm:
                return rec[hip.OPTIM_RECORD_HEAD:].sum().sqrt() * abs(float(self.grad_scale))
        return None

    @torch.no_grad()
    def clip_grad_value_(self, clip_value):
        """torch.nn.utils.clip_grad_value_(parameters, clip_value) for the NEXT step(): its launches clamp each (averaged) gradient
        to [-clip_value, clip_value] as they read it."""
        clip_value = float(clip_value)
        if not clip_value >= 0.0:
            raise ValueError(f"Invalid clip_value value: {clip_value}")
        a = self._clip_arena("clip_grad_value_")
        with torch.cuda.device(a.flat_grad.device):
            self._clip_set_bound(clip_value)
        self._clip = hip.OPTIM_CLIP_VALUE

    def _clip_launch_args(self, skip_flag):
        """(kind bits, skip_flag) of this step's launches: an armed clip hands them the record, with the scaler's flag (one float,
        copied device to device on the stream) or 0 in its first word."""
        bits, self._clip = self._clip, None
        if bits is None:
            return 0, skip_flag
        rec = self._clip_rec
        if skip_flag is not None:
            rec[0:1].copy_(skip_flag.reshape(-1)[0:1], non_blocking=True)
            self._clip_rec0_set = True
        elif self._clip_rec0_set:
            rec[0:1].zero_()
            self._clip_rec0_set = False
        return bits, rec

    @torch.no_grad()
    def step(self, closure=None, skip_flag=None):
        """skip_flag: device float; when it is non-zero at execution time the launches of this step do nothing."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        self._prev_gstate = [dict(g) for g in self._gstate]
        dev = next((p.device for g in self.param_groups for p in g["params"] if p.is_cuda), None)
        if dev is not None and dev != torch.device("cuda", torch.cuda.current_device()):
            with torch.cuda.device(dev):        # kernels go to the stream of the device that holds the parameters
                return self._step_impl(loss, skip_flag)
        return self._step_impl(loss, skip_flag)

    def _step_impl(self, loss, skip_flag):
        clip_bits, skip_flag = self._clip_launch_args(skip_flag)
        touched_arena = False
        shadowed = 0            # arena elements whose bf16 shadow this step's launches rewrote
        for group, gstate in zip(self.param_groups, self._gstate):
            live = [p for p in group["params"] if p.grad is not None]
            if not live:
                continue
            _validate(self.kind, group)                       # (a scheduler or the user may have rewritten the group)
            sgd = self.kind == "sgd"
            beta1, beta2 = (float(group["momentum"]), 0.0) if sgd else group.get("betas", (0.0, 0.0))
            dampening = float(group["dampening"]) if sgd else 0.0
            eps = group.get("eps", 0.0)
            lr, wd = float(group["lr"]), float(group["weight_decay"])
            kcode, sc = _step_scalars(self.kind, gstate, lr=lr, beta1=beta1, beta2=beta2, eps=eps,
                                      momentum_decay=group.get("momentum_decay", 4e-3),
                                      decoupled=bool(group.get("decoupled_weight_decay", False)),
                                      momentum=beta1 if sgd else 0.0, dampening=dampening,
                                      nesterov=bool(group.get("nesterov", False)))
            momentum = sgd and beta1 != 0.0
            rng = self._arena_range(group)
            if rng is not None:
                lo, hi = rng
                a = self.arena
                m, v = a.moments()
                shadow = a.shadow[lo:hi] if a.shadow is not None else None
                # (SGD with momentum keeps its buffer in the first moment and never reads the second)
                hip.optim_step(kcode | clip_bits, a.flat_param[lo:hi], a.flat_grad[lo:hi], m[lo:hi], None if momentum else v[lo:hi], shadow, hi - lo,
                               lr, wd, beta1, beta2, eps, self.grad_scale, *sc, skip_flag=skip_flag)
                touched_arena = True
                if shadow is not None and len(live) == len(group["params"]):
                    shadowed += hi - lo
                continue
            for p in live:
                hip.require_device(p, "optimizer.step")
                st = self.state[p]
                if "exp_avg" not in st and not sgd:
                    st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                psc = sc
                if momentum:                             # "first step" is this parameter's own: torch clones the gradient then
                    fresh = "momentum_buffer" not in st
                    if fresh:
                        st["momentum_buffer"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    psc = (1.0 if fresh else 1.0 - dampening,) + tuple(sc[1:])
                g = p.grad
                if g.dtype != torch.float32 or p.dtype != torch.float32:
                    raise RuntimeError("FusedOptimizer: parameters and gradients must be fp32")
                if not (_dense(p) and _dense(g) and p.stride() == g.stride()):
                    raise RuntimeError("FusedOptimizer: parameter/gradient must be dense with equal strides")
                hip.optim_step(kcode | clip_bits, p, g, st.get("momentum_buffer") if sgd else st.get("exp_avg"), st.get("exp_avg_sq"), None,
                               p.numel(), lr, wd, beta1, beta2, eps, self.grad_scale, *psc, skip_flag=skip_flag)
                if self.arena is not None and self.arena.owns(p):
                    touched_arena = True
        if touched_arena:
            self.arena.mark_dirty()
            if shadowed == self.arena.total:
                # every parameter went through a launch that also wrote its bf16 shadow: the engine's own refresh of the
                # whole shadow (one more pass over the arena per step) is redundant for this version
                self.arena.shadow_version = self.arena.version
        return loss


def _validate(kind: str, group: dict):
    """torch's constructor checks for the hyper-parameters nkb_optim_step reads, in torch's wording."""
    if group["lr"] < 0.0:
        raise ValueError(f"Invalid learning rate: {group['lr']}")
    if group["weight_decay"] < 0.0:
        raise ValueError(f"Invalid weight_decay value: {group['weight_decay']}")
    if kind == "sgd":
        if group["momentum"] < 0.0:
            raise ValueError(f"Invalid momentum value: {group['momentum']}")
        if group["nesterov"] and (group["momentum"] <= 0 or group["dampening"] != 0):
            raise ValueError("Nesterov momentum requires a momentum and zero dampening")
        if group["momentum"] != 0 and group["dampening"] == 1:
            # nkb_optim_step reads a zero factor on the gradient (c0 = 1 - dampening) as plain SGD
            raise NotImplementedError("dampening=1 with a momentum is not implemented: no gradient would ever enter the buffer "
                                      "after the first step")
        return
    if group["eps"] < 0.0:
        raise ValueError(f"Invalid epsilon value: {group['eps']}")
    for i, b in enumerate(group["betas"]):
        if not 0.0 <= b < 1.0:
            raise ValueError(f"Invalid beta parameter at index {i}: {b}")
    if group.get("amsgrad", False):
        raise NotImplementedError("amsgrad=True is not implemented: it needs a third state buffer, and nkb_optim_step "
                                  "has no pointer for one")
    if kind == "nadam" and not group.get("decoupled_weight_decay", True):
        raise NotImplementedError("nadam runs with decoupled weight decay only, as the reference builds it")


def parse_clip_grad(spec):
    """cfg.clip_grad -> None or ("norm" | "value", bound).  {"max_norm": 1.0} and {"clip_value": 0.5} are torch's names;
    {"mode": "norm" | "value", "clip_grad": x} timm's (its `clip_mode` / `clip_grad`; "agc" is not implemented)."""
    if spec is None:
        return None
    if not isinstance(spec, dict):
        raise ValueError(f"clip_grad must be a dict such as {{'max_norm': 1.0}} or {{'clip_value': 0.5}}, got {spec!r}")
    unknown = set(spec) - {"max_norm", "clip_value", "mode", "clip_grad"}
    if unknown:
        raise ValueError(f"clip_grad: unknown keys {sorted(unknown)}")
    given = [k for k in ("max_norm", "clip_value", "clip_grad") if k in spec]
    if len(given) != 1:
        raise ValueError(f"clip_grad needs exactly one of max_norm, clip_value or (with mode) clip_grad, got {sorted(spec)}")
    key = given[0]
    mode = spec.get("mode")
    if mode is not None and mode not in ("norm", "value"):
        raise ValueError(f"clip_grad: mode must be 'norm' or 'value', got {mode!r}"
                         + (" (adaptive gradient clipping is not implemented)" if mode == "agc" else ""))
    if key == "clip_grad":
        if mode is None:
            raise ValueError("clip_grad: the key clip_grad needs a mode ('norm' or 'value')")
    else:
        implied = "norm" if key == "max_norm" else "value"
        if mode is not None and mode != implied:
            raise ValueError(f"clip_grad: mode {mode!r} contradicts the key {key}")
        mode = implied
    bound = float(spec[key])
    if not bound >= 0.0:
        raise ValueError(f"Invalid {'max_norm' if mode == 'norm' else 'clip_value'} value: {bound}")
    return mode, bound


def _dense(t: torch.Tensor) -> bool:
    return t.is_contiguous() or t.is_contiguous(memory_format=torch.channels_last) or \
        t.numel() == t.untyped_storage().nbytes() // t.element_size()


def _backbone_groups(model, layer_decay, lr, wd):
    """Layer-wise lr decay, the usual ViT fine-tuning rule (BEiT / MAE / DINOv2 recipes; restated, not pinned against timm, which
    is not a dependency): the backbone's layer ids come from its `layer_groups()` (id 0 the embeddings, i + 1 block i, depth + 1
    what follows the blocks); id k of `top = depth + 1` trains at `lr * layer_decay ** (top - k)`.  One group per id that has
    parameters, in id order: each is one contiguous arena range, so it still costs one launch."""
    d = float(layer_decay)
    if not 0.0 < d <= 1.0:
        raise ValueError(f"layer_decay must lie in (0, 1], got {layer_decay}")
    layer_groups = getattr(model.emb_model, "layer_groups", None)
    if layer_groups is None:
        raise NotImplementedError(f"layer_decay is implemented for the ViT families only (timm-style ViT, unicom ViT), "
                                  f"not for {type(model.emb_model).__name__}")
    per_id = layer_groups()
    top = len(per_id) - 1
    return [{"params": ps, "lr": lr * d ** (top - k), "weight_decay": wd} for k, ps in enumerate(per_id) if ps]


def get_optimizer(model, cfg_optimizer):
    lr = cfg_optimizer.get("lr", 0.001)
    wd = cfg_optimizer.get("weight_decay", 0.0)
    backbone_lr, backbone_wd = cfg_optimizer.get("backbone_lr", lr), cfg_optimizer.get("backbone_weight_decay", wd)
    if cfg_optimizer.get("layer_decay") is not None:
        groups = _backbone_groups(model, cfg_optimizer["layer_decay"], backbone_lr, backbone_wd)
    else:
        groups = [{"params": list(model.emb_model.parameters()), "lr": backbone_lr, "weight_decay": backbone_wd}]
    groups.append({"params": list(model.classifier.parameters()),
                   "lr": cfg_optimizer.get("classifier_lr", lr),
                   "weight_decay": cfg_optimizer.get("classifier_weight_decay", wd)})
    kind = cfg_optimizer["type"].lower()
    if kind == "sparse_adam":
        # utils.py:36 builds torch's SparseAdam; it needs sparse gradients, which no model of this package produces.
        return torch.optim.SparseAdam(groups)
    if kind not in _KIND:
        raise NotImplementedError(f'Unknown optimizer in config: {cfg_optimizer["type"]}')
    options = {k: cfg_optimizer[k] for k in _OPTIONS if k in cfg_optimizer}
    return FusedOptimizer(groups, kind, arena=getattr(model, "arena", None), **options)


def get_scheduler(opt, lr_policy):
    if len(lr_policy) == 0:
        return None
    kind = lr_policy["type"]
    if kind == "step":
        return lr_scheduler.StepLR(opt, step_size=lr_policy["step_size"], gamma=lr_policy["gamma"])
    if kind == "multistep":
        return lr_scheduler.MultiStepLR(opt, milestones=lr_policy["steps"], gamma=lr_policy["gamma"])
    if kind == "cosine":
        return lr_scheduler.CosineAnnealingLR(opt, T_max=lr_policy["n_epochs"])
    raise NotImplementedError("Learning rate policy {} not implemented.".format(kind))


# ---- classes / config helpers (utils.py:64-105) --------------------------------------------
def save_classes(classes, save_path):
    if not isinstance(classes, (list, dict)):
        raise NotImplementedError(f"unknown classes config type {type(classes)}")
    with open(save_path, "w") as f:
        json.dump(classes, f)


def load_classes(classes):
    if isinstance(classes, (list, dict)):
        return classes
    if isinstance(classes, (str, Path)):
        with open(classes, "r") as f:
            return json.load(f)
    raise NotImplementedError(f"unknown classes config type {type(classes)}")


def get_classes_configs(classes):
    if isinstance(classes, list):
        c2i = {c: i for i, c in enumerate(classes)}
        return c2i, {i: c for c, i in c2i.items()}
    if isinstance(classes, dict):
        c2i = {t: {c: i for i, c in enumerate(cs)} for t, cs in classes.items()}
        return c2i, {t: {i: c for c, i in m.items()} for t, m in c2i.items()}
    raise NotImplementedError(f"unknown classes config type {type(classes)}")


def read_py_config(path):
    """Same contract as utils.py:101-105: returns the import statement the caller exec()s."""
    path = Path(path)
    sys.path.append(str(path.parent))
    return f"import {path.stem} as cfg"
