"""The optimizer options on the GPU: AdamW, RAdam with decoupled decay, SGD with momentum / dampening / Nesterov and layer-wise lr decay.

The reference everywhere is torch's own optimizer class on the CPU in fp32, fed the same gradients; the bound is the one
tests/test_ops_gpu.py::test_optimizer_kernel_matches_torch holds for the same kernel over the same eight steps (rtol 1e-5, atol 2e-6,
lr 1e-2, weight decay 0.05).  Model-level tests copy the engine's gradients to a CPU clone of the parameters after each backward and
step the torch class built over the same groups, so only the update itself is compared."""
import functools
import sys
from pathlib import Path

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

from nkb_classification import hip, utils  # noqa: E402
from nkb_classification.amp import HipGradScaler  # noqa: E402
from nkb_classification.losses import get_loss  # noqa: E402
from nkb_classification.model import get_model  # noqa: E402
from nkb_classification.utils import _step_scalars, get_optimizer, get_scheduler  # noqa: E402

DEV = "cuda:0"
CLASSES = ["a", "b", "c"]
LR, WD, STEPS = 1e-2, 0.05, 8
TOL = dict(rtol=1e-5, atol=2e-6)
VIT = "vit_tiny192_test"        # the reduced member tests/test_vit_members_gpu.py runs most of its cases on (depth 2, T = 17)

# mode -> (kind for _step_scalars, its keyword arguments, beta1 handed to the kernel, torch constructor)
MODES = {
    "adamw": ("adamw", {}, 0.9, lambda p: torch.optim.AdamW(p, lr=LR, weight_decay=WD)),
    "radam_decoupled": ("radam", dict(decoupled=True), 0.9,
                        lambda p: torch.optim.RAdam(p, lr=LR, weight_decay=WD, decoupled_weight_decay=True)),
    "sgd_momentum": ("sgd", dict(momentum=0.9), 0.9, lambda p: torch.optim.SGD(p, lr=LR, weight_decay=WD, momentum=0.9)),
    "sgd_dampening": ("sgd", dict(momentum=0.9, dampening=0.1), 0.9, lambda p: torch.optim.SGD(p, lr=LR, weight_decay=WD, momentum=0.9, dampening=0.1)),
    "sgd_nesterov": ("sgd", dict(momentum=0.9, nesterov=True), 0.9, lambda p: torch.optim.SGD(p, lr=LR, weight_decay=WD, momentum=0.9, nesterov=True)),
}
GUARD = 4            # elements in front of and behind every operand: 16 bytes in fp32, 8 in bf16 (the vector form's alignments)


@functools.lru_cache(maxsize=None)
def _reference(mode, n):
    """torch on the CPU, once per (mode, n): start, gradients, parameters after every step, final state buffers.  Read-only."""
    gen = torch.Generator().manual_seed(8 + n)
    p0 = torch.randn(n, generator=gen)
    ref_p = p0.clone().requires_grad_(True)
    opt = MODES[mode][3]([ref_p])
    grads, traj = [], []
    for _ in range(STEPS):
        g = torch.randn(n, generator=gen)
        ref_p.grad = g.clone()
        opt.step()
        grads.append(g)
        traj.append(ref_p.detach().clone())
    st = opt.state[ref_p]
    m = st["momentum_buffer"] if mode.startswith("sgd") else st["exp_avg"]
    return p0, grads, traj, m.clone(), (None if mode.startswith("sgd") else st["exp_avg_sq"].clone())


def _guarded(n, offset, dtype=torch.float32, fill=0.0, sentinel=-7.0):
    """(whole buffer, view of n elements that starts `offset` elements past a 16-byte boundary), sentinels around the view."""
    whole = torch.full((n + 2 * GUARD + 4,), sentinel, device=DEV, dtype=dtype)
    view = whole[GUARD + offset:GUARD + offset + n]
    view.fill_(fill)
    return whole, view


def _guards_intact(whole, n, offset, sentinel=-7.0):
    lo = GUARD + offset
    return bool((whole[:lo] == sentinel).all()) and bool((whole[lo + n:] == sentinel).all())


@pytest.mark.parametrize("n", [10007, 3, 4])
@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "odd_start"])
@pytest.mark.parametrize("mode", list(MODES))
def test_kernel_matches_torch(mode, offset, n):
    """Through hip.optim_step.  n = 10007 launches 5 blocks of 256 threads: 2501 groups of four over a stride of 1280, so threads run
    the two-groups-in-flight iteration and the single-group one, plus the n % 4 tail; n = 3 is tail only; n = 4 one group.  offset 1
    starts every operand off a 16-byte boundary (the one-parameter-per-thread kernel).  SGD passes v = None."""
    kind, kw, beta1, _ = MODES[mode]
    sgd = kind == "sgd"
    p0, grads, traj, m_ref, v_ref = _reference(mode, n)
    pw, p = _guarded(n, offset)
    p.copy_(p0)
    mw, m = _guarded(n, offset)
    vw, v = (None, None) if sgd else _guarded(n, offset)
    sw, shadow = _guarded(n, offset, dtype=torch.bfloat16)
    _, gd = _guarded(n, offset)
    state = {}
    for step in range(STEPS):
        k, sc = _step_scalars(kind, state, lr=LR, beta1=beta1, beta2=0.999, eps=1e-8, **kw)
        gd.copy_(grads[step])
        hip.optim_step(k, p, gd, m, v, shadow, n, LR, WD, beta1, 0.0 if sgd else 0.999, 0.0 if sgd else 1e-8, 1.0, *sc)
        torch.cuda.synchronize()
        torch.testing.assert_close(p.cpu(), traj[step], msg=lambda s: f"{mode} step {step + 1}: {s}", **TOL)
    torch.testing.assert_close(m.cpu(), m_ref, msg=lambda s: f"{mode} first moment / momentum buffer: {s}", **TOL)
    if not sgd:
        torch.testing.assert_close(v.cpu(), v_ref, msg=lambda s: f"{mode} second moment: {s}", **TOL)
        assert _guards_intact(vw, n, offset)
    assert torch.equal(shadow.cpu(), p.cpu().bfloat16())
    assert _guards_intact(mw, n, offset) and _guards_intact(pw, n, offset) and _guards_intact(sw, n, offset)


@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "odd_start"])
@pytest.mark.parametrize("mode", list(MODES))
def test_skip_flag_leaves_everything_untouched(mode, offset):
    kind, kw, beta1, _ = MODES[mode]
    sgd = kind == "sgd"
    n = 10007
    gen = torch.Generator().manual_seed(3)
    _, p = _guarded(n, offset)
    _, m = _guarded(n, offset)
    _, v = _guarded(n, offset)
    _, g = _guarded(n, offset)
    _, shadow = _guarded(n, offset, dtype=torch.bfloat16, fill=0.5)
    for t in (p, m, g):
        t.copy_(torch.randn(n, generator=gen))
    v.copy_(torch.rand(n, generator=gen))
    before = [t.clone() for t in (p, m, v, shadow)]
    skip = torch.ones(1, device=DEV)
    state = {"step": 3, "momentum_buffer": True}
    k, sc = _step_scalars(kind, state, lr=LR, beta1=beta1, beta2=0.999, eps=1e-8, **kw)
    hip.optim_step(k, p, g, m, None if sgd else v, shadow, n, LR, WD, beta1, 0.999, 1e-8, 1.0, *sc, skip_flag=skip)
    torch.cuda.synchronize()
    for name, a, b in zip(("p", "m", "v", "shadow"), (p, m, v, shadow), before):
        assert torch.equal(a, b), (mode, name)
    skip.zero_()                    # the same launch with the flag down does move them: the flag is what held it back
    hip.optim_step(k, p, g, m, None if sgd else v, shadow, n, LR, WD, beta1, 0.999, 1e-8, 1.0, *sc, skip_flag=skip)
    torch.cuda.synchronize()
    assert not torch.equal(p, before[0]) and not torch.equal(m, before[1]) and not torch.equal(shadow, before[3])
    assert torch.equal(v, before[2]) == sgd


@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "odd_start"])
def test_kind_3_with_zero_scalars_stays_plain_sgd(offset):
    """Callers from before the momentum form hand kind 3 Adam's betas with zeros in c0..c3 (tests/test_ops_gpu.py does): that is
    still plain SGD, whatever beta1 holds, and it reads and writes neither moment (NULL is accepted for both)."""
    n = 10007
    gen = torch.Generator().manual_seed(4)
    p0, g0 = torch.randn(n, generator=gen), torch.randn(n, generator=gen)
    ref = p0.clone().requires_grad_(True)
    ref.grad = g0.clone()
    torch.optim.SGD([ref], lr=LR, weight_decay=WD).step()
    for with_moments in (True, False):
        _, p = _guarded(n, offset)
        _, g = _guarded(n, offset)
        _, m = _guarded(n, offset, fill=0.25)
        _, v = _guarded(n, offset, fill=0.25)
        p.copy_(p0); g.copy_(g0)
        k, sc = _step_scalars("sgd", {}, lr=LR, beta1=0.9, beta2=0.999, eps=1e-8, momentum_decay=4e-3)
        assert (k, sc) == (3, (0.0, 0.0, 0.0, 0.0))
        hip.optim_step(k, p, g, m if with_moments else None, v if with_moments else None, None, n, LR, WD, 0.9, 0.999, 1e-8, 1.0, *sc)
        torch.cuda.synchronize()
        torch.testing.assert_close(p.cpu(), ref.detach(), **TOL)
        assert bool((m == 0.25).all()) and bool((v == 0.25).all())


@pytest.mark.parametrize("case", ["kind_4", "sgd_momentum_without_m", "adam_without_v", "nesterov_without_momentum"])
def test_refusals_leave_operands_untouched(case):
    n = 1000
    p, g, m, v = (torch.randn(n, device=DEV) for _ in range(4))
    shadow = torch.full((n,), 0.5, device=DEV, dtype=torch.bfloat16)
    before = [t.clone() for t in (p, g, m, v, shadow)]
    args = {
        "kind_4": dict(kind=4, m=m, v=v, beta1=0.9, c0=1.0, c1=1.0),
        "sgd_momentum_without_m": dict(kind=3, m=None, v=None, beta1=0.9, c0=1.0, c1=0.0),
        "adam_without_v": dict(kind=0, m=m, v=None, beta1=0.9, c0=LR / 0.1, c1=0.0316),
        "nesterov_without_momentum": dict(kind=3, m=m, v=None, beta1=0.0, c0=1.0, c1=1.0),
    }[case]
    with pytest.raises(RuntimeError, match="optim_step"):
        hip.optim_step(args["kind"], p, g, args["m"], args["v"], shadow, n, LR, WD, args["beta1"], 0.999, 1e-8, 1.0, args["c0"], args["c1"])
    torch.cuda.synchronize()
    for a, b in zip((p, g, m, v, shadow), before):
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------------ model level ----
def _cfg_model(name):
    return dict(model=name, pretrained=False, backbone_dropout=0.0, classifier_dropout=0.0, classifier_initialization="kaiming_normal_",
                task="single")


MODELS = {"resnet_tiny_basic": 4, VIT: 2}          # name -> batch; both take 64 x 64 images
OPT_CFGS = {
    "adamw": (dict(type="adamw", lr=LR, backbone_lr=3e-3, weight_decay=WD, classifier_weight_decay=0.01), torch.optim.AdamW, {}),
    "sgd_nesterov": (dict(type="sgd", lr=LR, backbone_lr=3e-3, weight_decay=WD, classifier_weight_decay=0.01, momentum=0.9, nesterov=True),
                     torch.optim.SGD, dict(momentum=0.9, nesterov=True)),
    "sgd_dampening": (dict(type="sgd", lr=LR, backbone_lr=3e-3, weight_decay=WD, classifier_weight_decay=0.01, momentum=0.9, dampening=0.1),
                      torch.optim.SGD, dict(momentum=0.9, dampening=0.1)),
}


def _model(name, seed=0):
    torch.manual_seed(seed)
    model = get_model(_cfg_model(name), CLASSES, DEV)
    g = torch.Generator().manual_seed(5)
    with torch.no_grad():                         # (1-D parameters off their zero / one initial values, as tests/test_model_gpu.py does)
        for p in model.parameters():
            if p.dim() == 1:
                p.copy_((torch.rand(p.shape, generator=g) * 0.5 + 0.5).to(DEV))
    model.train()
    return model


def _batches(batch, count, seed=7):
    g = torch.Generator().manual_seed(seed)
    return [(torch.randn(batch, 3, 64, 64, generator=g).to(DEV), torch.randint(0, len(CLASSES), (batch,), generator=g).to(DEV))
            for _ in range(count)]


class _Twin:
    """CPU clones of the model's parameters under the torch class built over the same groups (same order, lr, weight decay)."""

    def __init__(self, model, opt, cls, kw):
        self.pairs = []
        groups = []
        for g in opt.param_groups:
            clones = [torch.nn.Parameter(p.detach().cpu().clone()) for p in g["params"]]
            self.pairs += list(zip(g["params"], clones))
            groups.append(dict(params=clones, lr=g["lr"], weight_decay=g["weight_decay"]))
        assert len(self.pairs) == len(list(model.parameters()))
        self.opt = cls(groups, **kw)

    def step(self):
        """Take the engine's current gradients and step torch's optimizer."""
        for p, c in self.pairs:
            c.grad = p.grad.detach().cpu().clone()
        self.opt.step()

    def assert_params_match(self, what):
        torch.cuda.synchronize()
        for i, (p, c) in enumerate(self.pairs):
            torch.testing.assert_close(p.detach().cpu(), c.detach(), msg=lambda s: f"{what}, parameter {i} {tuple(c.shape)}: {s}", **TOL)


def _train_step(model, opt, crit, x, y):
    opt.zero_grad()
    crit(model(x), y).backward()
    torch.cuda.synchronize()


@pytest.mark.parametrize("opt_name", ["adamw", "sgd_nesterov"])
@pytest.mark.parametrize("name", list(MODELS))
def test_three_model_steps_match_torch_fp32(name, opt_name):
    cfg, cls, kw = OPT_CFGS[opt_name]
    model = _model(name)
    opt = get_optimizer(model, cfg)
    assert len(opt.param_groups) == 2 and opt.param_groups[0]["lr"] == 3e-3 and opt.param_groups[1]["weight_decay"] == 0.01
    twin = _Twin(model, opt, cls, kw)
    crit = get_loss(dict(task="single", type="CrossEntropyLoss"), DEV)
    for x, y in _batches(MODELS[name], 3):
        _train_step(model, opt, crit, x, y)
        assert all(opt._arena_range(g) is not None for g in opt.param_groups)       # one launch per group
        twin.step()
        opt.step()
    twin.assert_params_match(f"{name} {opt_name} after three steps")
    if opt_name == "sgd_nesterov":
        m = model.arena.moments()[0]
        for p, c in twin.pairs:
            buf = twin.opt.state[c]["momentum_buffer"]
            got = model.arena._view(m, model.arena.offset_of(p), p)
            torch.testing.assert_close(got.cpu(), buf, **TOL)


@pytest.mark.parametrize("name,cfg", [
    ("resnet_tiny_basic", OPT_CFGS["adamw"][0]),
    ("resnet_tiny_basic", OPT_CFGS["sgd_nesterov"][0]),
    (VIT, dict(OPT_CFGS["adamw"][0], layer_decay=0.75)),
    (VIT, dict(OPT_CFGS["sgd_nesterov"][0], layer_decay=0.75)),
], ids=["resnet-adamw", "resnet-sgd_nesterov", "vit-adamw-layer_decay", "vit-sgd_nesterov-layer_decay"])
def test_bf16_steps_rewrite_the_whole_shadow(name, cfg):
    """bf16: the launches of one step together rewrite the bf16 shadow of every parameter, so the step marks the shadow current
    (the engine then skips its own refresh pass) and the shadow equals the rounded masters — with two groups and with depth + 3."""
    model = _model(name)
    opt = get_optimizer(model, cfg)
    crit = get_loss(dict(task="single", type="CrossEntropyLoss"), DEV)
    a = model.arena
    for x, y in _batches(MODELS[name], 3, seed=9):
        with torch.autocast("cuda", dtype=torch.bfloat16):
            _train_step(model, opt, crit, x, y)
        opt.step()
        torch.cuda.synchronize()
        assert a.shadow is not None and torch.equal(a.shadow, a.flat_param.bfloat16())
        assert getattr(a, "shadow_version", -1) == a.version
        assert torch.isfinite(a.flat_param).all()


@pytest.mark.parametrize("poison", [(False, True, False), (True, False, False)], ids=["good-inf-good", "inf-good-good"])
@pytest.mark.parametrize("opt_name", ["adamw", "sgd_dampening"])
def test_scaler_skips_on_inf_and_leaves_no_trace(opt_name, poison):
    """HipGradScaler: a step whose gradients hold an inf is skipped on the device (parameters and the momentum buffer / moments stay
    bit-identical), and the good steps around it match a torch run that never saw the skipped one: AdamW's bias corrections and SGD's
    'first step clones the gradient' (no dampening there) both count good steps only."""
    cfg, cls, kw = OPT_CFGS[opt_name]
    model = _model("resnet_tiny_basic")
    opt = get_optimizer(model, cfg)
    twin = _Twin(model, opt, cls, kw)
    crit = get_loss(dict(task="single", type="CrossEntropyLoss"), DEV)
    scaler = HipGradScaler("cuda", init_scale=1024.0, growth_interval=1000)
    a = model.arena
    good = 0
    for (x, y), bad in zip(_batches(4, 3, seed=13), poison):
        opt.zero_grad()
        scaler.scale(crit(model(x), y)).backward()
        if bad:
            a.flat_grad[a.total // 2] = float("inf")
        torch.cuda.synchronize()
        p_before, m_before = a.flat_param.clone(), a.moments()[0].clone()
        scaler.step(opt)                       # unscales the gradient arena in place, then the fused launches test the flag
        scaler.update()
        torch.cuda.synchronize()
        if bad:
            assert torch.equal(a.flat_param, p_before) and torch.equal(a.moments()[0], m_before)
        else:
            good += 1
            twin.step()                        # the unscaled gradients the engine's own step just used
            assert not torch.equal(a.flat_param, p_before)
            twin.assert_params_match(f"{opt_name} after good step {good}")
    scaler.settle()
    assert [gs["step"] for gs in opt._gstate] == [good, good] and good == 2
    assert scaler.get_scale() == 512.0


def test_layer_decay_groups_ranges_steps_and_schedule(monkeypatch):
    model = _model(VIT)
    depth = len(model.emb_model.blocks)
    cfg = dict(type="adamw", lr=LR, backbone_lr=4e-3, weight_decay=WD, classifier_weight_decay=0.0, layer_decay=0.75)
    opt = get_optimizer(model, cfg)
    groups = opt.param_groups
    assert len(groups) == depth + 3
    want_lr = [4e-3 * 0.75 ** (depth + 1 - k) for k in range(depth + 2)] + [LR]
    assert [g["lr"] for g in groups] == want_lr
    assert [g["weight_decay"] for g in groups] == [WD] * (depth + 2) + [0.0]
    assert sum(len(g["params"]) for g in groups) == len(list(model.parameters()))
    twin = _Twin(model, opt, torch.optim.AdamW, {})
    crit = get_loss(dict(task="single", type="CrossEntropyLoss"), DEV)
    launches = []
    real = hip.optim_step
    monkeypatch.setattr(utils.hip, "optim_step", lambda *a, **k: (launches.append(a[6]), real(*a, **k))[1])
    for x, y in _batches(2, 2, seed=17):
        _train_step(model, opt, crit, x, y)
        ranges = [opt._arena_range(g) for g in groups]
        assert all(r is not None for r in ranges)
        assert ranges[0][0] == 0 and ranges[-1][1] == model.arena.total
        assert all(r0[1] == r1[0] for r0, r1 in zip(ranges, ranges[1:]))           # the groups tile the arena in order
        twin.step()
        opt.step()
    assert launches == [hi - lo for lo, hi in ranges] * 2                          # one launch per group per step
    twin.assert_params_match("layer_decay, two AdamW steps")
    sch = get_scheduler(opt, dict(type="cosine", n_epochs=5))
    for epoch in range(1, 4):
        sch.step()
        lrs = [g["lr"] for g in groups]
        assert lrs[-1] < LR
        assert [l / lrs[-1] for l in lrs] == pytest.approx([w / LR for w in want_lr], rel=1e-12)
