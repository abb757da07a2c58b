"""SE / ECA ResNet members on the HIP engine against the twin of tests/seresnet_reference.py (our own pure-torch restatement; timm parity
unpinned), on the reduced members seresnet_tiny_basic, seresnet_tiny_bottleneck and ecaresnet_tiny_bottleneck (and once on ecaresnet26t
at 70x73 for the deep stem and the avg_down shortcuts): single-step gradients in fp32 against the float64 twin, a bf16 step against the
autocast yardstick, eval mode on the folded path after a train step, bit-reproducibility, recorded plans against the Python path, a
frozen backbone, and the plain members' untouched launches.

The 1-D parameters are randomised into [0.5, 1] as tests/test_resnet_dt_gpu.py does: zero_init_last sets the closing BatchNorm's gamma
to 0, which would silence the whole operator."""
import sys
from pathlib import Path

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

from seresnet_reference import TINY, SEResNetClassifier  # noqa: E402
from nkb_classification import hip  # noqa: E402
from nkb_classification import model as model_mod  # noqa: E402
from nkb_classification.losses import get_loss  # noqa: E402
from nkb_classification.model import get_model  # noqa: E402
from nkb_classification.utils import get_optimizer  # noqa: E402

DEV = "cuda:0"
CLASSES = ["a", "b", "c"]
# launches of one fp32 step followed by one bf16 step of resnet_tiny_bottleneck (batch 4, 64x64), per NkbLaunchCounter, read on the commit
# before the SE / ECA members: the plain members must execute exactly what they executed
PLAIN_COUNTERS = {"avgpool2": 0, "conv1p": 0, "convp": 0, "dwconv": 0, "gemm8p": 0, "gemm8p_ragged": 0, "gemm_fp8": 0, "gram_bn_apply": 3,
                  "gram_conv": 2, "gramr": 0, "layer_scale": 0, "stem3": 0, "stemp": 2, "wgrad3x3": 1, "wgrad8f": 0, "wgrad8p": 0, "wgradr": 0}


def _cfg_model(name):
    return dict(model=name, pretrained=False, backbone_dropout=0.0, classifier_dropout=0.0, classifier_initialization="kaiming_normal_",
                task="single")


def _relerr(a, b):
    a, b = torch.as_tensor(a, dtype=torch.float64), torch.as_tensor(b, dtype=torch.float64)
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-12)).item()


def _pair(name, seed=0):
    torch.manual_seed(seed)
    twin = SEResNetClassifier(_cfg_model(name), CLASSES)
    g = torch.Generator().manual_seed(5)
    with torch.no_grad():
        for p in twin.parameters():
            if p.dim() == 1:
                p.copy_(torch.rand(p.shape, generator=g) * 0.5 + 0.5)
    model = get_model(_cfg_model(name), CLASSES, DEV)
    model.load_state_dict(twin.state_dict())
    return twin, model


def _batch(shape=(4, 3, 64, 64), seed=7):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g), torch.randint(0, len(CLASSES), (shape[0],), generator=g)


def _hip_step(model, x, y):
    crit = get_loss(dict(task="single", type="CrossEntropyLoss"), DEV)
    out = model(x.to(DEV))
    crit(out, y.to(DEV)).backward()
    torch.cuda.synchronize()
    return out.detach().float().cpu()


@pytest.mark.parametrize("name,shape", [(n, (4, 3, 64, 64)) for n in TINY] + [("ecaresnet26t", (4, 3, 70, 73))],
                         ids=list(TINY) + ["ecaresnet26t_70x73"])
def test_single_step_gradients_match_the_float64_twin(name, shape):
    """The fp32 bars of tests/test_resnet_dt_gpu.py: logits within 1e-3 of the fp32 twin with the same argmax; every tensor's gradient
    within max(2e-2, 4 x the fp32 twin's own error) of the float64 twin; the whole gradient within 3e-3 in L2."""
    t32, model = _pair(name)
    t64 = SEResNetClassifier(_cfg_model(name), CLASSES).double()
    t64.load_state_dict(t32.state_dict())
    x, y = _batch(shape)
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
    seen_se = 0
    for pname, p in model.named_parameters():
        assert p.grad is not None, pname
        assert p.grad.shape == p32[pname].grad.shape
        ref = p64[pname].grad
        scale = max(ref.abs().max().item(), 1e-6 * gmax)
        e_hip = (p.grad.cpu().double() - ref).abs().max().item() / scale
        e_cpu = (p32[pname].grad.double() - ref).abs().max().item() / scale
        worst = max(worst, (e_hip, pname))
        assert e_hip <= max(2e-2, 4 * e_cpu), (pname, e_hip, e_cpu)
        if ".se." in pname:
            seen_se += 1
            assert float(ref.abs().max()) > 0, pname                 # the operator is alive
        num += (p.grad.cpu().double() - ref).pow(2).sum().item()
        den += ref.pow(2).sum().item()
    assert seen_se >= 4
    print(f"\n[{name} {shape}] logits {_relerr(out, ref32.detach()):.2e}  gradient L2 {(num / den) ** 0.5:.2e}  worst tensor {worst}")
    assert (num / den) ** 0.5 < 3e-3, (num / den) ** 0.5


@pytest.mark.parametrize("name", TINY)
def test_bf16_step_against_the_autocast_yardstick(name):
    """Batch 4, 64x64, bf16: the engine's gradient L2 error against the float64 twin is at most 1.25 x the error of the twin run under
    torch.autocast("cpu", bfloat16) on the same batch, + 5e-3 (the bar of tests/test_resnet_dt_gpu.py)."""
    t32, model = _pair(name)
    t64 = SEResNetClassifier(_cfg_model(name), CLASSES).double()
    t64.load_state_dict(t32.state_dict())
    x, y = _batch(seed=21)
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
    print(f"\n[{name} bs 4 bf16] gradient L2 error {l2:.3e}, autocast yardstick {yl2:.3e}")
    assert l2 <= 1.25 * yl2 + 5e-3, (l2, yl2)


@pytest.mark.parametrize("name", TINY)
def test_eval_after_a_train_step_matches_the_twin_on_the_folded_path(name):
    """One SGD step on both sides (the running statistics move), then eval: the folded convolutions deliver the normalised map and the
    attention passes run without BatchNorm vectors; nothing is saved."""
    twin, model = _pair(name)
    x, y = _batch(seed=9)
    model.train(); twin.train()
    opt = get_optimizer(model, dict(type="sgd", lr=1e-2))
    opt_t = torch.optim.SGD(twin.parameters(), lr=1e-2)
    _hip_step(model, x, y)
    opt.step()
    torch.nn.functional.cross_entropy(twin(x), y).backward()
    opt_t.step()
    model.eval(); twin.eval()
    x2, _ = _batch(seed=2)
    with torch.no_grad():
        out, ref = model(x2.to(DEV)).float().cpu(), twin(x2)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            out16 = model(x2.to(DEV)).float().cpu()
    assert _relerr(out, ref) < 1e-3 and out.argmax(-1).tolist() == ref.argmax(-1).tolist()
    assert _relerr(out16, ref) < 5e-2
    eng = model._engines[torch.float32]
    last = "layer2.0.2" if "bottleneck" in name else "layer2.0.1"
    assert last in eng._fold                                          # the closing BatchNorm was folded into its convolution


def _grads(model, x, y, steps):
    """Gradients of the last of `steps` identical steps (no optimizer step in between: the weights never move)."""
    out = None
    for _ in range(steps):
        for p in model.parameters():
            p.grad = None
        out = _hip_step(model, x, y)
    return out, {n: p.grad.detach().clone() for n, p in model.named_parameters()}


@pytest.mark.parametrize("amp", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("name", TINY)
def test_same_step_twice_and_recorded_plans_give_identical_gradients(name, amp, monkeypatch):
    """The same step twice gives bit-identical gradients (no float atomics in the new kernels), and the recorded-plan path (default;
    the fourth step replays the plans) gives the gradients of the Python path (plans off) bit for bit."""
    twin, model = _pair(name)
    x, y = _batch(seed=4)
    model.train()
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=amp):
        o1, g1 = _grads(model, x, y, 1)
        o4, g4 = _grads(model, x, y, 3)                            # steps 2, 3 (records), 4 (replays)
        assert len(model._active.plans) >= 2
        monkeypatch.setattr(model_mod, "_PLANS", False)
        fresh = get_model(_cfg_model(name), CLASSES, DEV)
        fresh.load_state_dict(twin.state_dict())
        fresh.train()
        o0, g0 = _grads(fresh, x, y, 2)
        assert len(fresh._active.plans) == 0
    assert torch.equal(o1, o4) and torch.equal(o1, o0)
    for n in g1:
        assert torch.equal(g1[n], g4[n]), n
        assert torch.equal(g1[n], g0[n]), n


def test_frozen_backbone_only_updates_head():
    twin, model = _pair("seresnet_tiny_bottleneck")
    model.set_backbone_state("freeze"); twin.set_backbone_state("freeze")
    x, y = _batch(seed=9)
    model.train(); twin.train()
    _hip_step(model, x, y)
    torch.nn.functional.cross_entropy(twin(x), y).backward()
    assert all(p.grad is None for p in model.emb_model.parameters())
    for (n, p), (_, q) in zip(model.classifier.named_parameters(), twin.classifier.named_parameters()):
        assert _relerr(p.grad.cpu(), q.grad) < 1e-3, n
    model.set_backbone_state("unfreeze")
    _hip_step(model, x, y)
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in model.emb_model.parameters())


def test_plain_member_launch_counters_are_unchanged():
    model = get_model(_cfg_model("resnet_tiny_bottleneck"), CLASSES, DEV)
    x, y = _batch(seed=8)
    model.train()
    before = {k: hip.kernel_launches(k) for k in hip._LAUNCH_COUNTERS}
    for amp in (False, True):
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=amp):
            _hip_step(model, x, y)
    got = {k: hip.kernel_launches(k) - before[k] for k in PLAIN_COUNTERS}
    print(f"\n[resnet_tiny_bottleneck fp32 + bf16 step] {got}")
    assert PLAIN_COUNTERS and got == PLAIN_COUNTERS
    assert not any(hasattr(blk, "se") for _, blk in model.emb_model.blocks())
