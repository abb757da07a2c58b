"""The 192-wide ViT members on the HIP engine against the twin of tests/vit_members_reference.py (oracle.torch_models.VisionTransformer
plus the head; timm parity unpinned): single-step gradients in fp32 against the float64 twin at the bars of tests/test_resnet_dt_gpu.py,
a NAdam trajectory through train_epoch, eval logits, bit-reproducibility, recorded plans against the Python path, a bf16 step against
the autocast yardstick (the form of tests/test_parity_bench_size_gpu.py), the 384-px member (T = 577: unfused attention at D = 192)
and one bf16 train step of vit_tiny_patch16_224, where no GEMM is inside the gemm8p envelope.

The 1-D parameters are randomised into [0.5, 1] as tests/test_model_gpu.py does."""
import sys
import types
from pathlib import Path

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

from vit_members_reference import MEMBERS, ViTClassifier  # noqa: E402
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
SMALL = "vit_tiny192_test"


def _cfg_model(name=SMALL):
    return dict(model=name, pretrained=False, backbone_dropout=0.0, classifier_dropout=0.0, classifier_initialization="kaiming_normal_",
                task="single")


def _relerr(a, b):
    a, b = torch.as_tensor(a, dtype=torch.float64), torch.as_tensor(b, dtype=torch.float64)
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-12)).item()


def _pair(name=SMALL, seed=0):
    torch.manual_seed(seed)
    twin = ViTClassifier(name, len(CLASSES))
    g = torch.Generator().manual_seed(5)
    with torch.no_grad():
        for p in twin.parameters():
            if p.dim() == 1:
                p.copy_(torch.rand(p.shape, generator=g) * 0.5 + 0.5)
    model = get_model(_cfg_model(name), CLASSES, DEV)
    model.load_state_dict(twin.state_dict())
    return twin, model


def _batch(name=SMALL, n=4, seed=7):
    hw = MEMBERS[name][0]
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, 3, hw, hw, generator=g), torch.randint(0, len(CLASSES), (n,), generator=g)


def _hip_step(model, x, y):
    crit = get_loss(dict(task="single", type="CrossEntropyLoss"), DEV)
    out = model(x.to(DEV))
    crit(out, y.to(DEV)).backward()
    torch.cuda.synchronize()
    return out.detach().float().cpu()


@pytest.mark.parametrize("name", [SMALL, "vit_tiny192_p32_test"])
def test_single_step_gradients_match_the_float64_twin(name):
    """Logits within 1e-3 of the fp32 twin with the same argmax; every tensor's gradient within max(2e-2, 4 x the fp32 twin's own
    error) of the float64 twin; the whole gradient within 3e-3 in L2.  T = 17 (patch 16 at 64 px) and T = 10 (patch 32 at 96 px)."""
    t32, model = _pair(name)
    t64 = ViTClassifier(name, len(CLASSES)).double()
    t64.load_state_dict(t32.state_dict())
    x, y = _batch(name)
    t32.train(); t64.train(); model.train()
    ref32 = t32(x)
    torch.nn.functional.cross_entropy(ref32, y).backward()
    torch.nn.functional.cross_entropy(t64(x.double()), y).backward()
    out = _hip_step(model, x, y)
    assert _relerr(out, ref32.detach()) < 1e-3
    assert out.argmax(-1).tolist() == ref32.argmax(-1).tolist()
    p64, p32 = dict(t64.named_parameters()), dict(t32.named_parameters())
    gmax = max(p.grad.abs().max().item() for p in p64.values())
    num = den = 0.0
    worst = (0.0, "")
    for n, p in model.named_parameters():
        assert p.grad is not None, n
        assert p.grad.shape == p32[n].grad.shape
        ref = p64[n].grad
        scale = max(ref.abs().max().item(), 1e-6 * gmax)
        e_hip = (p.grad.cpu().double() - ref).abs().max().item() / scale
        e_cpu = (p32[n].grad.double() - ref).abs().max().item() / scale
        worst = max(worst, (e_hip, n))
        assert e_hip <= max(2e-2, 4 * e_cpu), (n, e_hip, e_cpu)
        num += (p.grad.cpu().double() - ref).pow(2).sum().item()
        den += ref.pow(2).sum().item()
    print(f"\n[{name}] logits {_relerr(out, ref32.detach()):.2e}  gradient L2 {(num / den) ** 0.5:.2e}  worst tensor {worst}")
    assert (num / den) ** 0.5 < 3e-3, (num / den) ** 0.5


def test_three_nadam_steps_follow_the_twin_and_eval_logits_match():
    """train_epoch with NAdam, three steps, fp32: running losses, the final eval logits and the norm of every parameter follow the
    twin's own fp32 trajectory at the 1e-3 bar of the golden-trajectory tests."""
    twin, model = _pair()
    model.eval(); twin.eval()
    x, _ = _batch(seed=11)
    with torch.no_grad():
        out, want = model(x.to(DEV)).cpu(), twin(x)
    assert _relerr(out, want) < 1e-3 and out.argmax(-1).tolist() == want.argmax(-1).tolist()
    batches = torch_engine.synthetic_batches(12, 4, len(CLASSES), seed=1234, hw=64)
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
    assert _relerr(out, want) < 1e-3 and out.argmax(-1).tolist() == want.argmax(-1).tolist()
    sd, td = model.state_dict(), twin.state_dict()
    for k, v in td.items():
        assert abs(float(sd[k].float().norm()) - float(v.float().norm())) <= 1e-3 * max(1.0, float(v.float().norm())), k


def _grads(model, x, y, steps):
    """Gradients of the last of `steps` identical steps (no optimizer step in between: the weights never move)."""
    out = None
    for _ in range(steps):
        for p in model.parameters():
            p.grad = None
        out = _hip_step(model, x, y)
    return out, {n: p.grad.detach().clone() for n, p in model.named_parameters()}


@pytest.mark.parametrize("amp", [False, True], ids=["fp32", "bf16"])
def test_same_step_twice_and_recorded_plans_give_identical_gradients(amp, monkeypatch):
    """The same step twice gives bit-identical gradients (the engine runs the workspace form of the LayerNorm backward: no float
    atomics), and the recorded-plan path (default; the fourth step replays the plans) gives the gradients of the Python path bit for bit."""
    twin, model = _pair()
    x, y = _batch(seed=4)
    model.train()
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=amp):
        o1, g1 = _grads(model, x, y, 1)
        o4, g4 = _grads(model, x, y, 3)                            # steps 2, 3 (records), 4 (replays)
        assert len(model._active.plans) >= 2
        monkeypatch.setattr(model_mod, "_PLANS", False)
        fresh = get_model(_cfg_model(), CLASSES, DEV)
        fresh.load_state_dict(twin.state_dict())
        fresh.train()
        o0, g0 = _grads(fresh, x, y, 2)
        assert len(fresh._active.plans) == 0
    assert torch.equal(o1, o4) and torch.equal(o1, o0)
    for n in g1:
        assert torch.equal(g1[n], g4[n]), n
        assert torch.equal(g1[n], g0[n]), n


def test_bf16_step_against_the_autocast_yardstick():
    """Batch 8, bf16: the engine's gradient L2 error against the float64 twin is at most 1.25 x the error of the twin run under
    torch.autocast("cpu", bfloat16) on the same batch, + 5e-3."""
    t32, model = _pair()
    t64 = ViTClassifier(SMALL, len(CLASSES)).double()
    t64.load_state_dict(t32.state_dict())
    x, y = _batch(n=8, seed=21)
    t32.train(); t64.train(); model.train()
    torch.nn.functional.cross_entropy(t64(x.double()), y).backward()
    with torch.autocast("cpu", dtype=torch.bfloat16):
        yl = t32(x)
    torch.nn.functional.cross_entropy(yl.float(), y).backward()
    with torch.autocast("cuda", dtype=torch.bfloat16):
        out = _hip_step(model, x, y)
    names = [n for n, _ in t64.named_parameters()]
    p64, p32, ph = dict(t64.named_parameters()), dict(t32.named_parameters()), dict(model.named_parameters())
    truth = torch.cat([p64[n].grad.flatten() for n in names])
    yard = torch.cat([p32[n].grad.double().flatten() for n in names])
    got = torch.cat([ph[n].grad.detach().cpu().double().flatten() for n in names])
    assert torch.isfinite(got).all() and torch.isfinite(out).all()
    l2, yl2 = ((got - truth).norm() / truth.norm()).item(), ((yard - truth).norm() / truth.norm()).item()
    print(f"\n[{SMALL} bs 8 bf16] gradient L2 error {l2:.3e}, autocast yardstick {yl2:.3e}")
    assert l2 <= 1.25 * yl2 + 5e-3, (l2, yl2)


def test_384px_member_takes_the_unfused_attention_path_in_fp32():
    """vit_tiny_patch16_384 at batch 2, one fp32 step against the fp32 twin on the CPU: T = 577, three heads, twelve blocks.  Logits
    within 1e-3 with the same argmax, every tensor's gradient within 2e-2 of the twin's (relative to the tensor's largest entry)."""
    name = "vit_tiny_patch16_384"
    twin, model = _pair(name)
    x, y = _batch(name, n=2, seed=17)
    twin.train(); model.train()
    ref = twin(x)
    torch.nn.functional.cross_entropy(ref, y).backward()
    out = _hip_step(model, x, y)
    assert _relerr(out, ref.detach()) < 1e-3
    assert out.argmax(-1).tolist() == ref.argmax(-1).tolist()
    pt = dict(twin.named_parameters())
    gmax = max(p.grad.abs().max().item() for p in pt.values())
    worst = (0.0, "")
    for n, p in model.named_parameters():
        assert p.grad is not None and p.grad.shape == pt[n].grad.shape, n
        r = pt[n].grad.double()
        e = (p.grad.cpu().double() - r).abs().max().item() / max(r.abs().max().item(), 1e-6 * gmax)
        worst = max(worst, (e, n))
        assert e <= 2e-2, (n, e)
    print(f"\n[{name} bs 2 fp32] logits {_relerr(out, ref.detach()):.2e}  worst tensor {worst}")


def test_vit_tiny_224_bf16_train_step_stays_off_gemm8p():
    """vit_tiny_patch16_224, batch 8, bf16: finite loss, a finite gradient for every parameter, and no launch of the eight-phase
    GEMM core (K = 192 is no multiple of 128 and N = 192 / 576 none of 256: nothing at this width qualifies)."""
    name = "vit_tiny_patch16_224"
    model = get_model(_cfg_model(name), CLASSES, DEV)
    x, y = _batch(name, n=8, seed=23)
    model.train()
    crit = get_loss(dict(task="single", type="CrossEntropyLoss"), DEV)
    n0 = hip.kernel_launches("gemm8p")
    with torch.autocast("cuda", dtype=torch.bfloat16):
        out = model(x.to(DEV))
        loss = crit(out, y.to(DEV))
    loss.backward()
    torch.cuda.synchronize()
    assert hip.kernel_launches("gemm8p") == n0
    assert torch.isfinite(loss).item() and torch.isfinite(out).all()
    seen = 0
    for n, p in model.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), n
        seen += 1
    assert seen == 4 + 12 * 12 + 2 + 2
