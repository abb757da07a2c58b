"""The QuickGELU CLIP members on the HIP engine against the twin of tests/vit_quickgelu_reference.py (timm parity unpinned), in the form
and at the bars of tests/test_vit_options_gpu.py, whose helpers and test bodies run here by import against the new twin; the fc1
epilogue path (nkb_linear_gelu act 9) and the fp8 mode in a model at the bars of tests/test_step_semantics_gpu.py."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import test_vit_options_gpu as tvo  # noqa: E402
import vit_quickgelu_reference as vq  # noqa: E402
from nkb_classification import hip, vit  # noqa: E402
from nkb_classification.losses import get_loss  # noqa: E402
from nkb_classification.model import get_model  # noqa: E402

DEV = "cuda:0"
NAME, WIDE = "vit_clip_quickgelu_test", "vit_clip_quickgelu_f8_test"


@pytest.fixture(autouse=True)
def _against_the_quickgelu_twin(monkeypatch):
    """tests/test_vit_options_gpu.py builds its twins from ViTClassifier and MEMBERS of its own namespace: for this module they are
    the QuickGELU twin (which still answers the other names with the plain twin) and the table with the new rows."""
    monkeypatch.setattr(tvo, "ViTClassifier", vq.ViTClassifier)
    monkeypatch.setattr(tvo, "MEMBERS", {**tvo.MEMBERS, **vq.MEMBERS})


def test_the_twin_in_use_applies_quickgelu():
    twin = tvo._twin(NAME)
    assert all(isinstance(b.mlp, vq.QuickGELUMlp) for b in twin.emb_model.blocks)
    model = get_model(tvo._cfg_model(NAME), tvo.CLASSES, DEV)
    assert model.emb_model.act == "quick_gelu" and list(model.state_dict()) == list(twin.state_dict())


def test_single_step_gradients_match_the_float64_twin():
    tvo._check_fp32_step(NAME, 4, 7)


def test_bf16_step_against_the_autocast_yardstick():
    tvo._check_bf16_step(NAME, 4, 7)


def test_three_nadam_steps_follow_the_twin_and_eval_saves_nothing():
    tvo.test_three_nadam_steps_follow_the_twin_and_eval_saves_nothing(NAME)


def test_frozen_backbone_only_updates_head():
    tvo.test_frozen_backbone_only_updates_head(NAME)


@pytest.mark.parametrize("amp", [False, True], ids=["fp32", "bf16"])
def test_recorded_plans_replay_to_the_bits_of_the_python_path(amp, monkeypatch):
    tvo.test_same_step_twice_and_recorded_plans_give_identical_gradients(NAME, amp, monkeypatch)


@pytest.mark.parametrize("amp", [False, True], ids=["fp32", "bf16"])
def test_step_with_backbone_dropout_takes_the_elementwise_backward_with_the_saved_kind(amp):
    """drop1 active: the mask sits between fc2's data gradient and the activation's, so the forward pass keeps the pre-activation and
    the backward pass is nkb_gelu(dy) — with the kind the forward pass recorded."""
    cfg = dict(tvo._cfg_model(NAME), backbone_dropout=0.1)
    model = get_model(cfg, tvo.CLASSES, DEV)
    model.load_state_dict(tvo._reference(NAME, 4, 7)[0])
    x, y = tvo._batch(NAME, seed=3)
    model.train()
    torch.manual_seed(5)
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=amp):
        out = tvo._hip_step(model, x, y)
    eng = model._active
    sv = eng.saved["b0.act"]
    assert "x" in sv and "gp" not in sv and sv["kind"] == hip.ACT_QUICK_GELU
    assert torch.isfinite(out).all()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in model.parameters())
    # a GELU member on the same path records the GELU kind
    gelu = get_model(dict(tvo._cfg_model("vit_clip_test"), backbone_dropout=0.1), tvo.CLASSES, DEV)
    gelu.train()
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=amp):
        tvo._hip_step(gelu, x, y)
    assert gelu._active.saved["b0.act"]["kind"] == hip.ACT_GELU


def _cos(a, b):
    num = sum((a[n].double() * b[n].double()).sum().item() for n in a)
    return num / (sum(a[n].double().pow(2).sum().item() for n in a) * sum(b[n].double().pow(2).sum().item() for n in b)) ** 0.5


def _wide_twin(classes, activation_matters=False):
    """The twin of the dim-256 member, 1-D parameters randomised into [0.5, 1] as everywhere here.
    activation_matters: at the initialisation's weight scale (std 0.02) two blocks of MLP move the logits by so little that exact-erf
    GELU in place of QuickGELU changes them by 1.3e-3 of the largest logit (fp32 twin against itself), a quarter of what bf16 rounding
    does (5.6e-3, the twin under autocast) — no end-to-end test can tell the activations apart there.  This state dict puts the MLP
    where a trained tower has it: fc1 / fc2 weights of std 1 / sqrt(fan_in) and 8 / sqrt(fan_in), and fc1's biases in [-2.5, -2], the
    negative tail where the two functions differ by 40 % of their value (gelu(-2) = -0.0455, quickgelu(-2) = -0.0643).  The fp32 twin
    then moves by 8.7e-2 of the largest logit when its activation is swapped, against 1.1e-2 of bf16 rounding."""
    torch.manual_seed(0)
    twin = vq.ViTClassifier(WIDE, len(classes))
    g = torch.Generator().manual_seed(5)
    with torch.no_grad():
        for p in twin.parameters():
            if p.dim() == 1:
                p.copy_(torch.rand(p.shape, generator=g) * 0.5 + 0.5)
        if activation_matters:
            for blk in twin.emb_model.blocks:
                for lin, gain in ((blk.mlp.fc1, 1.0), (blk.mlp.fc2, 8.0)):
                    lin.weight.copy_(torch.randn(lin.weight.shape, generator=g) * gain / lin.weight.shape[1] ** 0.5)
                blk.mlp.fc1.bias.sub_(3.0)
    return twin


def test_bf16_quickgelu_epilogue_in_a_model_against_the_fp32_twin(monkeypatch):
    """vit_clip_quickgelu_f8_test (dim 256) in bf16 with the eight-phase core forced on for its small GEMMs: fc1 writes quickgelu(pre)
    and quickgelu'(pre) from its epilogue (act 9) and the fc2 data gradient multiplies by the saved derivative.  Bars of
    test_timm_vit_bf16_gelu_epilogue_against_oracle.  The same weights in the GELU member of the same width give logits further from
    these than that error: the activation differs end to end."""
    classes = ["a", "b", "c", "d"]
    twin = _wide_twin(classes, activation_matters=True)
    model = get_model(tvo._cfg_model(WIDE), classes, DEV)
    model.load_state_dict(twin.state_dict())
    # vit_clip_test widened the same way (dim 256, 4 heads): same keys and shapes, exact-erf GELU
    monkeypatch.setitem(vit._VITS, "vit_clip_f8_test", dict(vit._VITS["vit_clip_test"], dim=256, heads=4))
    gelu = get_model(tvo._cfg_model("vit_clip_f8_test"), classes, DEV)
    assert gelu.emb_model.act == "gelu"
    gelu.load_state_dict(twin.state_dict())
    g = torch.Generator().manual_seed(8)
    x, y = torch.randn(64, 3, 64, 64, generator=g), torch.randint(0, 4, (64,), generator=g)
    twin.train(); model.train(); gelu.train()
    ref = twin(x)
    torch.nn.functional.cross_entropy(ref, y).backward()
    crit = get_loss(dict(task="single", type="CrossEntropyLoss"), DEV)
    hip.gemm8p_config(True, 1, 128)
    try:
        assert hip.linear_gelu_fused_ok(hip.BF16, 64 * 17, 256, 1024)
        n0 = hip.kernel_launches("gemm8p")
        with torch.autocast("cuda", dtype=torch.bfloat16):
            out = model(x.to(DEV))
            loss = crit(out, y.to(DEV))
        assert hip.kernel_launches("gemm8p") > n0
        eng = model._engines[torch.bfloat16]
        assert "gp" in eng.saved["b0.act"] and "x" not in eng.saved["b0.act"]      # the epilogue form ran: no pre-activation kept
        loss.backward()
        with torch.autocast("cuda", dtype=torch.bfloat16):
            out_gelu = gelu(x.to(DEV))
        assert "gp" in gelu._engines[torch.bfloat16].saved["b0.act"]
        torch.cuda.synchronize()
    finally:
        hip.gemm8p_config(True, 192, 768)
    scale = ref.detach().abs().max().item()
    err = (out.detach().float().cpu() - ref.detach()).abs().max().item() / scale
    got = {n: p.grad.detach().cpu() for n, p in model.named_parameters()}
    want = {n: p.grad for n, p in twin.named_parameters()}
    assert set(got) == set(want)
    cos = _cos(got, want)
    gap = (out_gelu.detach().float() - out.detach().float()).abs().max().item() / scale
    print(f"\n[{WIDE} bf16, act 9] logits relerr {err:.3e}, gradient cosine {cos:.6f}; GELU member of the same weights differs by {gap:.3e}")
    assert err < 3e-2 and cos > 0.999
    assert gap > err


def test_fp8_train_step_tracks_bf16_and_the_twin():
    """The fp8 mode on vit_clip_quickgelu_f8_test, 128 images, two passes (delayed scaling in effect on the second): fc1 runs in fp8 and
    the activation on nkb_gelu_fwd_dgelu with the QuickGELU kind.  Form and bounds of test_timm_vit_fp8_train_step_tracks_bf16_and_oracle."""
    classes = ["a", "b", "c", "d"]
    twin = _wide_twin(classes)
    g = torch.Generator().manual_seed(5)
    x, y = torch.randn(128, 3, 64, 64, generator=g), torch.randint(0, 4, (128,), generator=g)
    twin.train()
    ref_out = twin(x)
    torch.nn.functional.cross_entropy(ref_out, y).backward()
    ref_g = {n: p.grad.clone() for n, p in twin.named_parameters()}
    crit = get_loss(dict(task="single", type="CrossEntropyLoss"), DEV)
    res = {}
    for mode in ("bf16", "fp8"):
        model = get_model(tvo._cfg_model(WIDE), classes, DEV)
        model.load_state_dict(twin.state_dict())
        model.train()
        model.fp8_linear = mode == "fp8"
        for _ in range(2):
            for p in model.parameters():
                p.grad = None
            with torch.autocast("cuda", dtype=torch.bfloat16):
                out = model(x.to(DEV))
                loss = crit(out, y.to(DEV))
            loss.backward()
        torch.cuda.synchronize()
        eng = model._engines[torch.bfloat16]
        assert (len(eng._f8w) == 8) == (mode == "fp8")          # 2 blocks x (qkv, proj, fc1, fc2) took the fp8 kernel
        assert "gp" in eng.saved["b0.act"]                       # the derivative was kept (by the elementwise pass in fp8 mode)
        res[mode] = (out.detach().float().cpu(), loss.item(), {n: p.grad.detach().float().cpu() for n, p in model.named_parameters()})
    o16, l16, g16 = res["bf16"]
    o8, l8, g8 = res["fp8"]
    scale = ref_out.detach().abs().max().item()
    e16 = (o16 - ref_out.detach()).abs().max().item() / scale
    e8 = (o8 - ref_out.detach()).abs().max().item() / scale
    c16, c8 = _cos(g16, ref_g), _cos(g8, ref_g)
    qb = [n for n in ref_g if n.endswith("attn.qkv.bias")]
    cq = min(torch.nn.functional.cosine_similarity(g8[n].flatten().double(), ref_g[n].flatten().double(), dim=0).item() for n in qb)
    print(f"\n[{WIDE} fp8] logits relerr bf16 {e16:.3e} fp8 {e8:.3e}; loss {l16:.4f} / {l8:.4f}; grad cosine vs twin bf16 {c16:.5f} "
          f"fp8 {c8:.5f}; qkv bias {cq:.5f}")
    assert len(qb) == 2 and cq > 0.97
    assert e8 < 0.15 and e16 < 2e-2 and abs(l8 - l16) < 3e-2 * abs(l16)
    assert c8 > 0.97 and c16 > 0.995
