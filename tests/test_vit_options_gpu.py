"""The CLIP (pre_norm), DINOv2 (LayerScale) and DeiT-III (LayerScale, no_embed_class) ViT members on the HIP engine against the twin of
tests/vit_options_reference.py (timm parity unpinned), in the form and at the bars of tests/test_vit_members_gpu.py: single-step
gradients in fp32 against the float64 twin, a NAdam trajectory through train_epoch, eval logits, a frozen backbone, a bf16 step against
the autocast yardstick, bit-reproducibility and recorded plans against the Python path, the member past the fused-attention range
(T = 290) and the launch counts of nkb_layer_scale.

The 1-D parameters (LayerNorm, LayerScale gamma, biases) are randomised into [0.5, 1] as tests/test_model_gpu.py does, so the
LayerScale branches carry gradient.  The float64 / fp32 / autocast reference step of a (member, batch) pair is computed once per
module and read only."""
import sys
import types
from pathlib import Path

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

from vit_options_reference import MEMBERS, ViTClassifier  # noqa: E402
from nkb_classification import hip  # noqa: E402
from nkb_classification import model as model_mod  # noqa: E402
from nkb_classification.engine import train_epoch  # noqa: E402
from nkb_classification.logging import BaseLogger  # noqa: E402
from nkb_classification.losses import get_loss  # noqa: E402
from nkb_classification.model import get_model  # noqa: E402
from nkb_classification.utils import get_optimizer  # noqa: E402
from oracle import torch_engine  # noqa: E402

DEV = "cuda:0"
CLASSES = ["a", "b", "c"]
SMALL = ["vit_clip_test", "vit_dinov2_test", "deit3_test"]
LONG = "vit_dinov2_long_test"


def _cfg_model(name):
    return dict(model=name, pretrained=False, backbone_dropout=0.0, classifier_dropout=0.0, classifier_initialization="kaiming_normal_",
                task="single")


def _relerr(a, b):
    a, b = torch.as_tensor(a, dtype=torch.float64), torch.as_tensor(b, dtype=torch.float64)
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-12)).item()


def _twin(name, seed=0):
    torch.manual_seed(seed)
    twin = ViTClassifier(name, len(CLASSES))
    g = torch.Generator().manual_seed(5)
    with torch.no_grad():
        for p in twin.parameters():
            if p.dim() == 1:
                p.copy_(torch.rand(p.shape, generator=g) * 0.5 + 0.5)
    return twin


def _pair(name, seed=0):
    twin = _twin(name, seed)
    model = get_model(_cfg_model(name), CLASSES, DEV)
    model.load_state_dict(twin.state_dict())
    return twin, model


def _batch(name, n=4, seed=7):
    hw = MEMBERS[name][0]
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, 3, hw, hw, generator=g), torch.randint(0, len(CLASSES), (n,), generator=g)


def _hip_step(model, x, y):
    crit = get_loss(dict(task="single", type="CrossEntropyLoss"), DEV)
    out = model(x.to(DEV))
    crit(out, y.to(DEV)).backward()
    torch.cuda.synchronize()
    return out.detach().float().cpu()


_REF = {}


def _reference(name, n, seed):
    """One train step of the twin on batch (n, seed) in float64 (the truth), in fp32 and under torch.autocast("cpu", bfloat16):
    (state dict, batch, fp32 logits, {parameter: gradient} for each of the three).  Computed once, never written afterwards."""
    key = (name, n, seed)
    if key not in _REF:
        t32 = _twin(name)
        state = {k: v.clone() for k, v in t32.state_dict().items()}
        t64, t16 = ViTClassifier(name, len(CLASSES)).double(), ViTClassifier(name, len(CLASSES))
        t64.load_state_dict(state); t16.load_state_dict(state)
        x, y = _batch(name, n, seed)
        t32.train(); t64.train(); t16.train()
        ref32 = t32(x)
        torch.nn.functional.cross_entropy(ref32, y).backward()
        torch.nn.functional.cross_entropy(t64(x.double()), y).backward()
        with torch.autocast("cpu", dtype=torch.bfloat16):
            yl = t16(x)
        torch.nn.functional.cross_entropy(yl.float(), y).backward()
        grads = lambda m: {k: p.grad.detach().double() for k, p in m.named_parameters()}
        _REF[key] = (state, (x, y), ref32.detach(), grads(t64), grads(t32), grads(t16))
    return _REF[key]


def _model_with(name, state):
    model = get_model(_cfg_model(name), CLASSES, DEV)
    model.load_state_dict(state)
    return model


def _explicit(name):
    """The tensors the options add or change the gradient path of."""
    opts = MEMBERS[name][5]
    names = ["emb_model.cls_token", "emb_model.pos_embed"]
    if opts.get("pre_norm"):
        names += ["emb_model.norm_pre.weight", "emb_model.norm_pre.bias"]
    if opts.get("init_values") is not None:
        names += [f"emb_model.blocks.{i}.{ls}.gamma" for i in range(MEMBERS[name][3]) for ls in ("ls1", "ls2")]
    return names


def _check_fp32_step(name, n, seed):
    """Logits within 1e-3 of the fp32 twin with the same argmax; every tensor's gradient within max(2e-2, 4 x the fp32 twin's own error)
    of the float64 twin; the whole gradient within 3e-3 in L2; the options' own tensors are there, carry gradient and hold the bar."""
    state, (x, y), ref32, g64, g32, _ = _reference(name, n, seed)
    model = _model_with(name, state)
    model.train()
    out = _hip_step(model, x, y)
    print(f"\n[{name} bs {n} fp32] logits {_relerr(out, ref32):.2e}")
    assert _relerr(out, ref32) < 1e-3
    assert out.argmax(-1).tolist() == ref32.argmax(-1).tolist()
    gmax = max(g.abs().max().item() for g in g64.values())
    num = den = 0.0
    worst = (0.0, "")
    errs = {}
    got = dict(model.named_parameters())
    assert set(got) == set(g64)
    for k, p in got.items():
        assert p.grad is not None, k
        ref = g64[k]
        assert p.grad.shape == ref.shape, k
        scale = max(ref.abs().max().item(), 1e-6 * gmax)
        e_hip = (p.grad.cpu().double() - ref).abs().max().item() / scale
        e_cpu = (g32[k] - ref).abs().max().item() / scale
        errs[k] = (e_hip, e_cpu)
        worst = max(worst, (e_hip, k))
        num += (p.grad.cpu().double() - ref).pow(2).sum().item()
        den += ref.pow(2).sum().item()
    print(f"[{name} bs {n} fp32] gradient L2 {(num / den) ** 0.5:.2e}  worst tensor {worst}")
    for k in _explicit(name):
        print(f"[{name}] {k}: error {errs[k][0]:.2e} (fp32 twin {errs[k][1]:.2e}), |grad|max {g64[k].abs().max().item():.2e}")
    for k, (e_hip, e_cpu) in errs.items():
        assert e_hip <= max(2e-2, 4 * e_cpu), (k, e_hip, e_cpu)
    for k in _explicit(name):
        assert g64[k].abs().max().item() > 1e-6 * gmax, k               # the tensor is on a live gradient path in this test
        assert errs[k][0] <= max(2e-2, 4 * errs[k][1]), (k, errs[k])
    assert (num / den) ** 0.5 < 3e-3, (num / den) ** 0.5


def _check_bf16_step(name, n, seed):
    """bf16: the engine's gradient L2 error against the float64 twin is at most 1.25 x the error of the twin run under
    torch.autocast("cpu", bfloat16) on the same batch, + 5e-3."""
    state, (x, y), _, g64, _, g16 = _reference(name, n, seed)
    model = _model_with(name, state)
    model.train()
    with torch.autocast("cuda", dtype=torch.bfloat16):
        out = _hip_step(model, x, y)
    names = list(g64)
    ph = dict(model.named_parameters())
    truth = torch.cat([g64[k].flatten() for k in names])
    yard = torch.cat([g16[k].flatten() for k in names])
    got = torch.cat([ph[k].grad.detach().cpu().double().flatten() for k in names])
    assert torch.isfinite(got).all() and torch.isfinite(out).all()
    l2, yl2 = ((got - truth).norm() / truth.norm()).item(), ((yard - truth).norm() / truth.norm()).item()
    print(f"\n[{name} bs {n} bf16] gradient L2 error {l2:.3e}, autocast yardstick {yl2:.3e}")
    assert l2 <= 1.25 * yl2 + 5e-3, (l2, yl2)


@pytest.mark.parametrize("name", SMALL)
def test_single_step_gradients_match_the_float64_twin(name):
    """T = 17 (patch 16 at 64 px) and T = 26 (patch 14 at 70 px: K = 588 through the padded patch-embedding scratch), batch 4."""
    _check_fp32_step(name, 4, 7)


@pytest.mark.parametrize("name", SMALL)
def test_bf16_step_against_the_autocast_yardstick(name):
    _check_bf16_step(name, 4, 7)


def test_long_member_takes_the_unfused_attention_path_in_fp32():
    """vit_dinov2_long_test, batch 2: T = 290, past the fused-attention range, with LayerScale; the fp32 bars above."""
    _check_fp32_step(LONG, 2, 17)


def test_long_member_bf16_step_against_the_autocast_yardstick():
    """... and in bf16 (T = 290 > 256: the materialised attention path in bf16, as the 384-pixel members take)."""
    _check_bf16_step(LONG, 2, 17)


@pytest.mark.parametrize("name", SMALL)
def test_three_nadam_steps_follow_the_twin_and_eval_saves_nothing(name):
    """Eval logits first, on a model that has never trained: nothing is saved for a backward pass.  Then train_epoch with NAdam, three
    steps, fp32: running losses, the final eval logits and the norm of every parameter follow the twin's own fp32 trajectory at 1e-3."""
    twin, model = _pair(name)
    hw = MEMBERS[name][0]
    model.eval(); twin.eval()
    x, _ = _batch(name, seed=11)
    with torch.no_grad():
        out, want = model(x.to(DEV)).cpu(), twin(x)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            out16 = model(x.to(DEV)).float().cpu()
    assert _relerr(out, want) < 1e-3 and out.argmax(-1).tolist() == want.argmax(-1).tolist()
    assert _relerr(out16, want) < 5e-2
    assert len(model._engines) == 2
    for eng in model._engines.values():
        assert not any("x" in v or "mask" in v or "z" in v or "qkv" in v for v in eng.saved.values() if isinstance(v, dict)), list(eng.saved)
    batches = torch_engine.synthetic_batches(12, 4, len(CLASSES), seed=1234, hw=hw)
    opt_cfg = dict(type="nadam", lr=1e-4, weight_decay=0.01)
    cfg = types.SimpleNamespace(task="single", enable_mixed_presicion=False, log_gradients=False, show_full_current_loss_in_terminal=False)
    opt = get_optimizer(model, opt_cfg)
    crit = get_loss(dict(task="single", type="CrossEntropyLoss"), DEV)
    tr = train_epoch(model, batches, opt, None, torch.amp.GradScaler("cuda", enabled=False), crit, DEV, cfg, BaseLogger(cfg, CLASSES))
    ref = torch_engine.train_epoch(twin, batches, torch_engine.make_optimizer(twin, opt_cfg), None,
                                   torch_engine.Criterion(dict(task="single", type="CrossEntropyLoss")), torch_engine.EpochLog(False))
    assert len(tr["running_loss"]) == 3
    assert _relerr(tr["running_loss"], ref["running_loss"]) < 1e-3
    assert tr["ground_truth"] == ref["ground_truth"]
    model.eval(); twin.eval()
    with torch.no_grad():
        out, want = model(x.to(DEV)).cpu(), twin(x)
    # (after three steps the position embedding has moved: deit3's zero-class-row copy must have followed the arena)
    assert _relerr(out, want) < 1e-3 and out.argmax(-1).tolist() == want.argmax(-1).tolist()
    sd, td = model.state_dict(), twin.state_dict()
    for k, v in td.items():
        assert abs(float(sd[k].float().norm()) - float(v.float().norm())) <= 1e-3 * max(1.0, float(v.float().norm())), k


@pytest.mark.parametrize("name", SMALL)
def test_frozen_backbone_only_updates_head(name):
    twin, model = _pair(name)
    model.set_backbone_state("freeze"); twin.set_backbone_state("freeze")
    x, y = _batch(name, seed=9)
    model.train(); twin.train()
    _hip_step(model, x, y)
    torch.nn.functional.cross_entropy(twin(x), y).backward()
    assert all(p.grad is None for p in model.emb_model.parameters())
    for (n, p), (_, q) in zip(model.classifier.named_parameters(), twin.classifier.named_parameters()):
        assert _relerr(p.grad.cpu(), q.grad) < 1e-3, n


def test_deit3_zero_class_row_copy_follows_the_arena():
    """no_embed_class: nkb_vit_assemble reads an engine-owned [T, D] copy of pos_embed whose row 0 is zero.  After an optimizer step
    (lr large enough to move every entry) and after load_state_dict the copy equals the parameter again on the next forward, its
    class row is still zero, and the eval logits match the twin's."""
    name = "deit3_test"
    twin, model = _pair(name)
    x, y = _batch(name, seed=13)
    model.train()
    opt = get_optimizer(model, dict(type="nadam", lr=1e-2))
    before = model.emb_model.pos_embed.detach().clone()
    _hip_step(model, x, y)
    opt.step()
    _hip_step(model, x, y)                                         # the forward after the step refreshes the copy
    eng = model._active
    pos0, pos = eng.ws.get("pe.pos0", (17, 128), torch.float32), model.emb_model.pos_embed.detach()
    assert not torch.equal(pos, before)
    assert torch.equal(pos0[1:], pos[0]) and not pos0[0].any()
    with torch.no_grad():
        twin.emb_model.pos_embed.copy_(torch.randn(twin.emb_model.pos_embed.shape, generator=torch.Generator().manual_seed(1)) * 0.5)
    model.load_state_dict(twin.state_dict())
    model.eval(); twin.eval()
    with torch.no_grad():
        out, want = model(x.to(DEV)).cpu(), twin(x)
    assert _relerr(out, want) < 1e-3 and out.argmax(-1).tolist() == want.argmax(-1).tolist()
    assert torch.equal(pos0[1:], twin.emb_model.pos_embed[0].to(DEV)) and not pos0[0].any()


def _grads(model, x, y, steps):
    """Gradients of the last of `steps` identical steps (no optimizer step in between: the weights never move)."""
    out = None
    for _ in range(steps):
        for p in model.parameters():
            p.grad = None
        out = _hip_step(model, x, y)
    return out, {n: p.grad.detach().clone() for n, p in model.named_parameters()}


@pytest.mark.parametrize("amp", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("name", SMALL)
def test_same_step_twice_and_recorded_plans_give_identical_gradients(name, amp, monkeypatch):
    """The same step twice gives bit-identical gradients (LayerScale's dgamma goes through per-block partial rows and an ordered sum),
    and the recorded-plan path (default; the fourth step replays the plans) gives the gradients of the Python path bit for bit."""
    state = _reference(name, 4, 7)[0]
    model = _model_with(name, state)
    x, y = _batch(name, seed=4)
    model.train()
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=amp):
        o1, g1 = _grads(model, x, y, 1)
        o4, g4 = _grads(model, x, y, 3)                            # steps 2, 3 (records), 4 (replays)
        assert len(model._active.plans) >= 2
        monkeypatch.setattr(model_mod, "_PLANS", False)
        fresh = _model_with(name, state)
        fresh.train()
        o0, g0 = _grads(fresh, x, y, 2)
        assert len(fresh._active.plans) == 0
    assert torch.equal(o1, o4) and torch.equal(o1, o0)
    for n in g1:
        assert torch.equal(g1[n], g4[n]), n
        assert torch.equal(g1[n], g0[n]), n


@pytest.mark.parametrize("name,per_block", [("vit_dinov2_test", 4), ("deit3_test", 4), (LONG, 4), ("vit_clip_test", 0),
                                            ("vit_tiny_test", 0), ("vit_small_test", 0)])
@pytest.mark.parametrize("amp", [False, True], ids=["fp32", "bf16"])
def test_layer_scale_launch_counts(name, per_block, amp):
    """One train step of a LayerScale member launches nkb_layer_scale 4 x depth times (two per block forward, two per block backward);
    members without init_values keep the residual in the GEMM epilogue and never launch it."""
    model = get_model(_cfg_model(name), CLASSES, DEV)
    hw, depth = model.emb_model.img, len(model.emb_model.blocks)
    g = torch.Generator().manual_seed(3)
    x, y = torch.randn(2, 3, hw, hw, generator=g), torch.randint(0, len(CLASSES), (2,), generator=g)
    model.train()
    n0 = hip.kernel_launches("layer_scale")
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=amp):
        _hip_step(model, x, y)
    assert hip.kernel_launches("layer_scale") - n0 == per_block * depth
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in model.parameters())
