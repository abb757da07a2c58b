"""Gradient clipping and weight EMA through the optimizer, the scaler and engine.train_epoch, on the tiny models the model tests use
(batch 8, three steps, 64 x 64 images).

Clipping is compared bit for bit against a twin model whose gradient arena was multiplied by the host-computed coefficient
(test_optim_clip_ema_gpu.expected_coef, nkbhip.h's order) and stepped plain; the returned norm against the float64 norm of the
gradient arena at relative error (chunk_len + P + 8) * 2^-24, which any order of fp32 additions of once-rounded squares (plus the
P partials' sum and the square root) satisfies.  The EMA is compared bit for bit against the numpy fp32 recurrence over
parameter snapshots taken after each step."""
import types

import numpy as np
import pytest
import torch

from test_optim_clip_ema_gpu import expected_coef

from nkb_classification import hip, utils
from nkb_classification.amp import HipGradScaler
from nkb_classification.ema import ModelEma, ema_decay
from nkb_classification.engine import train_epoch
from nkb_classification.logging import BaseLogger
from nkb_classification.losses import get_loss
from nkb_classification.model import get_model
from nkb_classification.utils import get_optimizer

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CLASSES = ["a", "b", "c"]
BATCH, STEPS = 8, 3
RESNET, VIT = "resnet_tiny_basic", "vit_tiny192_test"
f32 = np.float32
OPT = {
    RESNET: dict(type="adamw", lr=1e-2, backbone_lr=3e-3, weight_decay=0.05),
    VIT: dict(type="adamw", lr=1e-2, backbone_lr=3e-3, weight_decay=0.05, layer_decay=0.75),
    "sgd": dict(type="sgd", lr=1e-2, weight_decay=0.05, momentum=0.9, nesterov=True),
}


def _model(name, seed=0):
    torch.manual_seed(seed)
    model = get_model(dict(model=name, pretrained=False, backbone_dropout=0.0, classifier_dropout=0.0,
                           classifier_initialization="kaiming_normal_", task="single"), CLASSES, DEV)
    g = torch.Generator().manual_seed(5)
    with torch.no_grad():                         # (1-D parameters off their zero / one initial values, as tests/test_model_gpu.py does)
        for p in model.parameters():
            if p.dim() == 1:
                p.copy_((torch.rand(p.shape, generator=g) * 0.5 + 0.5).to(DEV))
    model.train()
    return model


def _batches(count=STEPS, seed=7, device=DEV):
    g = torch.Generator().manual_seed(seed)
    return [(torch.randn(BATCH, 3, 64, 64, generator=g).to(device), torch.randint(0, len(CLASSES), (BATCH,), generator=g).to(device))
            for _ in range(count)]


def _cfg(**extra):
    return types.SimpleNamespace(task="single", enable_mixed_presicion=False, log_gradients=False,
                                 show_full_current_loss_in_terminal=False, **extra)


def _crit():
    return get_loss(dict(task="single", type="CrossEntropyLoss"), DEV)


def _backward(model, opt, crit, x, y):
    opt.zero_grad()
    crit(model(x), y).backward()


def _bits(t):
    return t.view(torch.int32)


@pytest.mark.parametrize("name,opt_cfg,max_norm", [(RESNET, OPT[RESNET], 0.05), (VIT, OPT[VIT], 0.05), (RESNET, OPT["sgd"], 0.05)],
                         ids=["resnet-adamw", "vit-adamw-layer_decay", "resnet-sgd_nesterov"])
def test_clip_grad_norm_follows_the_prescaled_twin_bit_for_bit(name, opt_cfg, max_norm):
    model, twin = _model(name), _model(name)
    opt, topt = get_optimizer(model, opt_cfg), get_optimizer(twin, opt_cfg)
    crit = _crit()
    a, b = model.arena, twin.arena
    clipped = 0
    for step, (x, y) in enumerate(_batches()):
        _backward(model, opt, crit, x, y)
        _backward(twin, topt, crit, x, y)
        if step == 0:                                        # (the arenas are packed by the first forward)
            assert torch.equal(a.flat_param, b.flat_param)
            chunk, P = hip.clip_chunks(a.total)
        b.flat_grad.copy_(a.flat_grad)                       # the twin steps on exactly these gradients
        grad_before = a.flat_grad.clone()
        norm = opt.clip_grad_norm_(max_norm, return_norm=True)
        exact = float(a.flat_grad.double().pow(2).sum().sqrt())
        assert abs(float(norm) - exact) <= (chunk + P + 8) * 2.0 ** -24 * exact, (float(norm), exact)
        partials = opt._clip_rec[4:].cpu().numpy()
        assert len(partials) == P and opt._clip_rec[:4].tolist() == [0.0, float(f32(max_norm)), float(P), 0.0]
        coef = expected_coef(partials, max_norm, 1.0)
        clipped += coef < 1.0
        b.flat_grad.mul_(float(coef))
        opt.step()
        topt.step()
        torch.cuda.synchronize()
        assert torch.equal(_bits(a.flat_grad), _bits(grad_before))              # the clip never rescales the arena itself
        assert torch.equal(_bits(a.flat_param), _bits(b.flat_param))
        ma, mb = a.moments(), b.moments()
        assert torch.equal(_bits(ma[0]), _bits(mb[0])) and torch.equal(_bits(ma[1]), _bits(mb[1]))
        assert opt._clip is None
    assert clipped == STEPS             # max_norm lies below these models' gradient norms: every step was really clipped


def test_clip_grad_value_follows_the_clamped_twin_bit_for_bit():
    model, twin = _model(RESNET), _model(RESNET)
    opt, topt = get_optimizer(model, OPT[RESNET]), get_optimizer(twin, OPT[RESNET])
    crit = _crit()
    a, b = model.arena, twin.arena
    for x, y in _batches():
        _backward(model, opt, crit, x, y)
        _backward(twin, topt, crit, x, y)
        bound = float(a.flat_grad.abs().max()) * 0.1
        b.flat_grad.copy_(a.flat_grad).clamp_(-bound, bound)
        assert not torch.equal(b.flat_grad, a.flat_grad)
        opt.clip_grad_value_(bound)
        opt.step()
        topt.step()
        torch.cuda.synchronize()
        assert torch.equal(_bits(a.flat_param), _bits(b.flat_param))


def _train(cfg, name=RESNET, opt_cfg=None, scaler=None, ema=None, hook=None):
    model = _model(name)
    opt = get_optimizer(model, opt_cfg or OPT[name])
    if ema is not None:
        model.ema = ModelEma(model, **ema)
    if hook is not None:
        hook(model)
    res = train_epoch(model, _batches(device="cpu"), opt, None, scaler or HipGradScaler("cuda", enabled=False), _crit(), DEV, cfg,
                      BaseLogger(cfg, CLASSES))
    torch.cuda.synchronize()
    return model, opt, res


def test_max_norm_above_the_norm_is_bit_identical_to_no_clipping():
    plain, _, _ = _train(_cfg())
    loose, _, _ = _train(_cfg(clip_grad={"max_norm": 1e9}))
    tight, _, _ = _train(_cfg(clip_grad={"max_norm": 0.05}))
    assert torch.equal(_bits(plain.arena.flat_param), _bits(loose.arena.flat_param))
    assert torch.equal(_bits(plain.arena.moments()[1]), _bits(loose.arena.moments()[1]))
    assert not torch.equal(plain.arena.flat_param, tight.arena.flat_param)


def test_plain_step_launches_what_it_launched_before(monkeypatch):
    """without cfg.clip_grad and model.ema: no segment_sumsq pass, no EMA launch, no clip bit, the scaler's own flag as skip_flag"""
    calls = []
    real_step, real_sumsq = hip.optim_step, hip.segment_sumsq
    monkeypatch.setattr(utils.hip, "optim_step", lambda *a, **k: (calls.append(("optim", a[0], k.get("skip_flag"))), real_step(*a, **k))[1])
    monkeypatch.setattr(utils.hip, "segment_sumsq", lambda *a, **k: (calls.append(("sumsq",)), real_sumsq(*a, **k))[1])
    _, opt, _ = _train(_cfg())
    assert [c[0] for c in calls] == ["optim"] * (2 * STEPS) and all(c[1] == 0 and c[2] is None for c in calls)
    assert opt._clip_rec is None


@pytest.mark.parametrize("poison", [(False, True, False), (True, False, False)], ids=["good-inf-good", "inf-good-good"])
def test_scaler_skips_an_inf_step_with_clipping_armed(poison):
    model = _model(RESNET)
    opt = get_optimizer(model, OPT[RESNET])
    crit = _crit()
    scaler = HipGradScaler("cuda", init_scale=1024.0, growth_interval=1000)
    a = model.arena
    good = 0
    for (x, y), bad in zip(_batches(seed=13), poison):
        opt.zero_grad()
        scaler.scale(crit(model(x), y)).backward()
        if bad:
            a.flat_grad[a.total // 2] = float("inf")
        scaler.unscale_(opt)
        opt.clip_grad_norm_(0.05)
        torch.cuda.synchronize()
        before = [t.clone() for t in (a.flat_param, *a.moments())]
        scaler.step(opt)                       # no second unscale; the record's first word takes the scaler's flag
        scaler.update()
        torch.cuda.synchronize()
        same = [torch.equal(_bits(t), _bits(s)) for t, s in zip((a.flat_param, *a.moments()), before)]
        if bad:
            assert all(same)
        else:
            good += 1
            assert not any(same) and bool(torch.isfinite(a.flat_param).all())
    scaler.settle()
    assert [gs["step"] for gs in opt._gstate] == [good, good] and good == 2
    assert scaler.get_scale() == 512.0


def test_every_layer_decay_group_carries_the_clip_bit(monkeypatch):
    model = _model(VIT)
    opt = get_optimizer(model, OPT[VIT])
    depth = len(model.emb_model.blocks)
    assert len(opt.param_groups) == depth + 3
    kinds = []
    real = hip.optim_step
    monkeypatch.setattr(utils.hip, "optim_step", lambda *a, **k: (kinds.append((a[0], k.get("skip_flag"))), real(*a, **k))[1])
    crit = _crit()
    (x, y), = _batches(1)
    for arm, bit in ((lambda: opt.clip_grad_norm_(0.05), hip.OPTIM_CLIP_NORM), (lambda: opt.clip_grad_value_(1e-3), hip.OPTIM_CLIP_VALUE),
                     (lambda: None, 0)):
        _backward(model, opt, crit, x, y)
        arm()
        kinds.clear()
        opt.step()
        assert len(kinds) == depth + 3
        assert all(k == bit and ((rec is opt._clip_rec) if bit else rec is None) for k, rec in kinds), kinds      # kind 0 adam | bit
    torch.cuda.synchronize()


def test_refusals_outside_the_packed_arena():
    p = torch.nn.Parameter(torch.zeros(8, device=DEV))
    opt = utils.FusedOptimizer([p], "adam")
    p.grad = torch.ones_like(p)
    with pytest.raises(NotImplementedError, match="arena"):
        opt.clip_grad_norm_(1.0)
    with pytest.raises(NotImplementedError, match="arena"):
        opt.clip_grad_value_(1.0)
    with pytest.raises(NotImplementedError, match="arena"):
        ModelEma(torch.nn.Linear(4, 4).to(DEV))
    cfg = _cfg(clip_grad={"max_norm": 1.0})
    model = _model(RESNET)
    with pytest.raises(NotImplementedError, match="fused optimizer"):
        train_epoch(model, _batches(1, device="cpu"), torch.optim.SGD(model.parameters(), lr=0.1), None, HipGradScaler("cuda", enabled=False),
                    _crit(), DEV, cfg, BaseLogger(cfg, CLASSES))


def test_train_epoch_with_clipping_and_ema_follows_the_numpy_recurrence():
    snaps = []

    def hook(model):
        ema, real = model.ema, model.ema.update

        def update():
            torch.cuda.synchronize()
            snaps.append((model.arena.flat_param.cpu().numpy().copy(), [b.cpu().numpy().copy() for _, b in ema._buffers]))
            real()
        ema.update = update
        hook.start = (ema.flat.cpu().numpy().copy(), [b.cpu().numpy().copy() for b in ema.buffers])

    cfg = _cfg(clip_grad={"max_norm": 0.05})
    cfg.log_gradients = True
    model, opt, res = _train(cfg, ema=dict(decay=0.9998, warmup=True), hook=hook)
    ema = model.ema
    assert len(snaps) == STEPS == ema.num_updates
    assert len(res["metrics_grad_log"]["Gradients/ClipNorm"]) == STEPS
    assert all(float(v) > 0.05 for v in res["metrics_grad_log"]["Gradients/ClipNorm"])
    assert ema.launches_per_update() == 1 + sum(1 for _, b in ema._buffers if b.is_floating_point())
    e, eb = hook.start
    assert any(b.dtype.kind == "f" for b in eb) and any(b.dtype.kind == "i" for b in eb)        # BatchNorm statistics and counters
    for t, (w, wb) in enumerate(snaps):
        d = ema_decay(0.9998, True, t)
        assert d == (1.0 + t) / (10.0 + t)
        d32, omd32 = f32(d), f32(1.0 - d)
        e = ((d32 * e).astype(f32) + (omd32 * w).astype(f32)).astype(f32)
        eb = [((d32 * x).astype(f32) + (omd32 * y).astype(f32)).astype(f32) if x.dtype.kind == "f" else y.copy() for x, y in zip(eb, wb)]
    assert np.array_equal(ema.flat.cpu().numpy().view(np.int32), e.view(np.int32))
    for got, want, (bname, _) in zip(ema.buffers, eb, ema._buffers):
        assert np.array_equal(got.cpu().numpy(), want), bname
    assert not np.array_equal(e, snaps[-1][0])                     # the average is not the raw weights

    # applied(): the model computes with the EMA values; a fresh model loaded from ema.state_dict() gives the same logits bit for bit
    a = model.arena
    raw_flat, raw_buffers = a.flat_param.clone(), [b.clone() for _, b in ema._buffers]
    x = _batches(1, seed=23)[0][0]
    model.eval()
    with torch.no_grad():
        raw_logits = model(x).clone()
        with ema.applied():
            ema_logits = model(x).clone()
            inside = {k: v.clone() for k, v in model.state_dict().items()}
    sd = ema.state_dict()
    assert sd.keys() == model.state_dict().keys() == inside.keys()
    assert all(torch.equal(sd[k], inside[k]) for k in sd)
    fresh = _model(RESNET, seed=3)
    fresh.load_state_dict(sd)
    fresh.eval()
    with torch.no_grad():
        fresh_logits = fresh(x)
    torch.cuda.synchronize()
    assert torch.equal(_bits(ema_logits), _bits(fresh_logits)) and not torch.equal(ema_logits, raw_logits)
    # after exit everything is back bit for bit, also when the block raises
    with pytest.raises(KeyError):
        with ema.applied():
            assert torch.equal(a.flat_param, ema.flat)
            raise KeyError("inside")
    assert torch.equal(_bits(a.flat_param), _bits(raw_flat))
    for (bname, b), saved in zip(ema._buffers, raw_buffers):
        assert torch.equal(b, saved), bname
    with torch.no_grad():
        assert torch.equal(_bits(model(x)), _bits(raw_logits))
    # load_state_dict is the inverse of state_dict and leaves the model alone
    other = ModelEma(fresh, decay=0.5)
    other.load_state_dict(model.state_dict())
    back = other.state_dict()
    assert all(torch.equal(back[k], v) for k, v in model.state_dict().items())
    assert all(torch.equal(fresh.state_dict()[k], sd[k]) for k in sd)


def test_ema_bf16_shadow_is_the_rounded_average():
    model = _model(RESNET)
    ema = ModelEma(model, decay=0.5, bf16_shadow=True)
    with torch.no_grad():
        model.arena.flat_param.mul_(1.5)
    ema.update()
    torch.cuda.synchronize()
    assert torch.equal(ema.shadow, ema.flat.bfloat16()) and not torch.equal(ema.flat, model.arena.flat_param)


def test_train_py_with_clip_grad_and_model_ema(tmp_path):
    """train.py -cfg with both keys: validation and best.pth on the averaged weights, last.pth raw, ema_last.pth beside it, an
    ordinary state dict with the model's keys"""
    import subprocess
    import sys
    from pathlib import Path
    root = Path(__file__).resolve().parents[1] / "nkb-classification_amd"
    cfg = (root / "configs" / "synthetic_singletask_config.py").read_text().replace('"runs/synthetic_single"', repr(str(tmp_path / "exp")))
    cfg = cfg.replace('"n_images": 256', '"n_images": 64').replace('"n_images": 128', '"n_images": 32').replace('"batch_size": 64', '"batch_size": 16')
    cfg += '\nclip_grad = {"max_norm": 1.0}\nmodel_ema = {"decay": 0.9, "warmup": True}\n'
    (tmp_path / "cfg.py").write_text(cfg)
    r = subprocess.run([sys.executable, str(root / "train.py"), "-cfg", str(tmp_path / "cfg.py")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    w = tmp_path / "exp" / "weights"
    assert (w / "last.pth").exists() and (w / "ema_last.pth").exists() and (w / "scripted_last.pt").exists()
    last, ema = torch.load(w / "last.pth", map_location="cpu"), torch.load(w / "ema_last.pth", map_location="cpu")
    assert list(last.keys()) == list(ema.keys())
    assert all(torch.isfinite(v).all() for v in ema.values() if v.is_floating_point())
    assert not torch.equal(last["emb_model.conv1.weight"], ema["emb_model.conv1.weight"])
    assert not torch.equal(last["emb_model.layer4.1.bn2.running_var"], ema["emb_model.layer4.1.bn2.running_var"])
    assert torch.equal(last["emb_model.bn1.num_batches_tracked"], ema["emb_model.bn1.num_batches_tracked"])
    if (w / "best.pth").exists():               # written when an epoch's validation accuracy beat 0: the averaged weights of that epoch
        assert list(torch.load(w / "best.pth", map_location="cpu").keys()) == list(last.keys())
