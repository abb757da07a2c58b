"""The QuickGELU CLIP towers (`vit_*_clip_quickgelu_*`) without a GPU: the registry, the TorchScript twin against the twin of
tests/vit_quickgelu_reference.py (timm parity unpinned: timm is not installed), host-side validation of the new `act` codes and the
`kind` parameter through the C ABI, the proof that the yardstick of tests/quickgelu_gemm_reference.py rejects the activation bugs this
feature exists for, and the compiled QuickGELU instance of the eight-phase kernel held to what tests/test_isa_guard.py asks of its
siblings."""
import ctypes
import re
import sys
from pathlib import Path

import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tests"))

import gemm_reference as gr  # noqa: E402
import quickgelu_gemm_reference as qr  # noqa: E402
from vit_quickgelu_reference import GELU_TWIN, MEMBERS, ViTClassifier, quick_gelu, quick_gelu_grad  # noqa: E402
from nkb_classification import hip  # noqa: E402
from nkb_classification.model import SingletaskClassifier, get_model  # noqa: E402
from nkb_classification.scripted import build_scriptable  # noqa: E402
from nkb_classification.vit import vit_members  # noqa: E402

CLASSES = ["a", "b", "c"]
FULL = [n for n in MEMBERS if not n.endswith("_test")]


def _cfg(name):
    return dict(model=name, pretrained=False, backbone_dropout=0.0, classifier_dropout=0.0, classifier_initialization="kaiming_normal_",
                task="single")


# ---- 1. registry ------------------------------------------------------------------------------------------------------------
def test_the_four_names_are_the_issue_s():
    assert FULL == ["vit_base_patch32_clip_quickgelu_224", "vit_base_patch16_clip_quickgelu_224", "vit_large_patch14_clip_quickgelu_224",
                    "vit_large_patch14_clip_quickgelu_336"]


@pytest.mark.parametrize("name", FULL + ["vit_clip_quickgelu_test"])
def test_member_builds_with_the_keys_and_shapes_of_its_gelu_twin(name):
    """Built on the meta device (up to 304 M parameters): keys, shapes, the activation and the twin's layout, no values."""
    with torch.device("meta"):
        model = SingletaskClassifier(_cfg(name), CLASSES)
        gelu = SingletaskClassifier(_cfg(GELU_TWIN[name]), CLASSES)
        twin = ViTClassifier(name, len(CLASSES))
    sd, gd, td = model.state_dict(), gelu.state_dict(), twin.state_dict()
    assert list(sd) == list(gd) == list(td)
    shapes = lambda d: {k: tuple(v.shape) for k, v in d.items()}
    assert shapes(sd) == shapes(gd) == shapes(td)
    count = MEMBERS[name][6]
    if count is not None:
        assert sum(v.numel() for k, v in sd.items() if k.startswith("emb_model.")) == count
    em, eg = model.emb_model, gelu.emb_model
    assert em.act == "quick_gelu" and eg.act == "gelu"
    assert all(b.mlp.act == "quick_gelu" for b in em.blocks) and all(b.mlp.act == "gelu" for b in eg.blocks)
    assert (em.img, em.patch, em.heads, em.pre_norm, em.ln_eps) == (eg.img, eg.patch, eg.heads, True, 1e-5)
    assert em.family == "vit" and em.n_tokens == eg.n_tokens


def test_members_build_through_get_model_and_are_listed():
    model = get_model(_cfg("vit_base_patch32_clip_quickgelu_224"), CLASSES, "cpu")
    assert model.emb_model.act == "quick_gelu" and model.emb_size == 768
    assert get_model(_cfg("vit_base_patch32_clip_224"), CLASSES, "cpu").emb_model.act == "gelu"
    assert get_model(_cfg("vit_tiny_test"), CLASSES, "cpu").emb_model.act == "gelu"
    listed = vit_members()
    for name in MEMBERS:
        assert (name in listed) == (not name.endswith("_test")), name
    with pytest.raises(NotImplementedError) as e:
        get_model(_cfg("vit_so400m_patch14_siglip_224"), CLASSES, "cpu")
    for name in FULL:
        assert name in str(e.value)
    with pytest.raises(NotImplementedError):
        get_model(_cfg("vit_huge_patch14_clip_quickgelu_224"), CLASSES, "cpu")


def test_engine_refuses_an_unknown_activation_name():
    from nkb_classification.hipnet import HipEngine
    from nkb_classification.vit import HipViT

    class M:
        act = "tanh_gelu"
    with pytest.raises(ValueError, match="tanh_gelu"):
        HipEngine.mlp_act_kind(M())
    with pytest.raises(ValueError, match="tanh_gelu"):
        HipViT(img=64, patch=16, dim=128, depth=1, heads=2, act="tanh_gelu")
    assert HipEngine.mlp_act_kind(object()) == hip.ACT_GELU == 0 and hip.ACT_QUICK_GELU == 1


# ---- 2. scripted twin -------------------------------------------------------------------------------------------------------
def test_scripted_twin_applies_quickgelu():
    """torch.jit.script export of vit_clip_quickgelu_test equals the tests/ twin at the bar of tests/test_vit_options_cpu.py (rtol and
    atol 1e-5) and differs from the GELU export of the same weights by more than 1e-3."""
    name = "vit_clip_quickgelu_test"
    torch.manual_seed(0)
    twin = ViTClassifier(name, len(CLASSES)).eval()
    g = torch.Generator().manual_seed(5)
    with torch.no_grad():
        for p in twin.parameters():
            if p.dim() == 1:
                p.copy_(torch.rand(p.shape, generator=g) * 0.5 + 0.5)
    model = get_model(_cfg(name), CLASSES, "cpu")
    model.load_state_dict(twin.state_dict())
    scripted = torch.jit.script(build_scriptable(model)).eval()
    gelu_model = get_model(_cfg(GELU_TWIN[name]), CLASSES, "cpu")
    gelu_model.load_state_dict(twin.state_dict())
    gelu_scripted = torch.jit.script(build_scriptable(gelu_model)).eval()
    x = torch.randn(2, 3, 64, 64)
    with torch.no_grad():
        out, want, other = scripted(x), twin(x), gelu_scripted(x)
    torch.testing.assert_close(out, want, rtol=1e-5, atol=1e-5)
    assert (out - other).abs().max().item() > 1e-3
    # the twin's activation is the formula of the issue, and its derivative the one the kernels store
    v = torch.linspace(-8, 8, 4001, dtype=torch.float64, requires_grad=True)
    u = quick_gelu(v)
    assert torch.equal(u, v * torch.sigmoid(1.702 * v))
    (d,) = torch.autograd.grad(u.sum(), v)
    torch.testing.assert_close(quick_gelu_grad(v.detach()), d, rtol=1e-12, atol=1e-12)


# ---- 3. host validation, no launch ------------------------------------------------------------------------------------------
_P = ctypes.c_void_p(64)


def _linear_gelu(act, y2=None, M=64, K=64, N=64):
    return (1, act, None, None, None, None, None, y2, M, K, N, None)


def test_new_act_codes_and_kinds_are_validated_on_the_host():
    lib = hip.load()
    assert len(hip._SIGS) == 125 and len(hip._PURE) == 45
    assert len(hip._SIGS["nkb_linear_gelu"][1]) == 12
    assert len(hip._SIGS["nkb_gelu"][1]) == 7 and len(hip._SIGS["nkb_gelu_fwd_dgelu"][1]) == 7
    inside, outside = (50432, 768, 3072), (200, 128, 192)
    assert lib.nkb_linear_gelu_fused_ok(1, *inside) == 1 and lib.nkb_linear_gelu_fused_ok(1, *outside) == 0
    M, K, N = inside
    for args, text in [
        (_linear_gelu(9, None, M, K, N), b"linear_gelu: act 9 needs y2"),
        (_linear_gelu(9, _P, *outside), b"linear_gelu: act 9 needs y2 and a shape of the eight-phase core"),
        (_linear_gelu(9, _P), b"linear_gelu: act 9 needs y2 and a shape of the eight-phase core"),
        (_linear_gelu(5), b"linear_gelu: act 5 needs y2"),
        (_linear_gelu(6), b"linear_gelu: unsupported dtype/act/shape (K=64 N=64)"),
        (_linear_gelu(10, _P), b"linear_gelu: unsupported dtype/act/shape (K=64 N=64)"),
        (_linear_gelu(0), b"linear_gelu: unsupported dtype/act/shape (K=64 N=64)"),
        (_linear_gelu(7), b"linear_gelu: act 7 needs y2"),
        (_linear_gelu(8, M=1 << 26), b"linear_gelu: operand exceeds"),
    ]:
        rc = lib.nkb_linear_gelu(*args)
        assert rc != 0 and text in lib.nkb_last_error(), (args, rc, lib.nkb_last_error())
    for kind in (2, -1, 7):
        rc = lib.nkb_gelu(1, None, None, None, 8, kind, None)
        assert rc != 0 and b"kind" in lib.nkb_last_error() and b"gelu:" in lib.nkb_last_error(), lib.nkb_last_error()
        for dtype in (0, 1):
            rc = lib.nkb_gelu_fwd_dgelu(dtype, None, None, None, 8, kind, None)
            assert rc != 0 and b"kind" in lib.nkb_last_error() and b"gelu_fwd_dgelu:" in lib.nkb_last_error(), lib.nkb_last_error()
    # the element-count refusals are what they were, for both kinds
    for kind in (0, 1):
        assert lib.nkb_gelu(1, None, None, None, 12, kind, None) != 0 and b"not a multiple of 8" in lib.nkb_last_error()
    header = (ROOT / "include" / "nkbhip.h").read_text()
    assert "#define NKB_ACT_GELU 0" in header and "#define NKB_ACT_QUICK_GELU 1" in header
    for word in ("act 7", "act 8", "act 9", "act 6 is unassigned"):
        assert word in header, word


# ---- 4. the yardstick rejects the bug this feature exists for -----------------------------------------------------------------
def test_yardstick_rejects_a_wrong_activation_and_a_wrong_derivative():
    """On a pre-activation of N(0, 1) over 2 x 2 tiles of 256 x 256: the yardstick (fp32 pre-activation, QuickGELU in fp32, y and y2
    rounded to bf16) sits at the bf16 rounding level, and each mutant exceeds max(C_BOUND * yardstick, FLOOR) in its worst tile — the
    exact-erf GELU on both outputs, the two derivative mutants on y2 (they leave y alone)."""
    g = torch.Generator().manual_seed(3)
    p = torch.randn(512, 512, generator=g, dtype=torch.float64)
    ref = qr.outputs(p, None, exact=True)
    yard = qr.outputs(p, None, exact=False)
    for out in ("y", "y2"):
        r, err, bound = gr.ratio(yard[out], ref[out], yard[out], out, gr.Geo())
        print(f"yardstick {out}: err {err:.2e} bound {bound:.2e}")
        assert 5e-4 < err < 4e-3 and r <= 1.0 / gr.C_BOUND + 1e-9
    figures = {}
    for m in qr.MUTANTS:
        mut = qr.outputs(p, None, exact=False, mutant=m)
        figures[m] = {out: gr.ratio(mut[out], ref[out], yard[out], out, gr.Geo()) for out in ("y", "y2")}
        print(m, {k: f"err {v[1]:.2e} ratio {v[0]:.1f}" for k, v in figures[m].items()})
    assert figures["erf_gelu"]["y"][0] > 1.0 and figures["erf_gelu"]["y2"][0] > 1.0
    assert figures["derivative_without_second_term"]["y2"][0] > 1.0
    assert figures["derivative_factor_missing"]["y2"][0] > 1.0
    for m in ("derivative_without_second_term", "derivative_factor_missing"):
        assert torch.equal(qr.outputs(p, None, exact=False, mutant=m)["y"], yard["y"])
    # the per-element size of the bug: exact-erf GELU in place of QuickGELU is off by up to 0.020
    v = torch.linspace(-6, 6, 24001, dtype=torch.float64)
    gap = (gr._gelu(v)[0] - qr.quick_gelu_pair(v)[0]).abs().max().item()
    assert 0.019 < gap < 0.021, gap


def test_quickgelu_pair_is_finite_where_the_exponential_overflows():
    """The kernels' order of evaluation, in fp32: u = x s, u' = s + 1.702 (u (1 - s)).  Where exp overflows to +inf, s = 0 and both
    results are 0; where 1.702 x itself would overflow (|x| > 2e38, finite in fp32 and in bf16) the textbook order s (1 + 1.702 x (1 - s))
    multiplies an infinity by a zero — this order never forms it."""
    x = torch.tensor([-90.0, -60.0, -30.0, -12.0, -1e-4, 0.0, 1e-4, 12.0, 30.0, 90.0, 3e38, -3e38], dtype=torch.float32)
    e = torch.exp(-1.702 * x)
    assert torch.isinf(e[0]) and torch.isinf(e[-1])
    s = 1.0 / (1.0 + e)
    u = x * s
    d = s + 1.702 * (u * (1.0 - s))
    assert torch.isfinite(u).all() and torch.isfinite(d).all()
    assert not torch.isfinite(s * (1.0 + 1.702 * x * (1.0 - s))).all()
    ref = qr.quick_gelu_pair(x[:10].double())
    torch.testing.assert_close(u[:10].double(), ref[0], rtol=1e-5, atol=1e-30)
    torch.testing.assert_close(d[:10].double(), ref[1], rtol=1e-5, atol=1e-30)
    assert u[0] == 0 and d[0] == 0 and u[-1] == 0 and d[-1] == 0 and u[5] == 0 and d[5] == 0.5 and u[10] == x[10] and d[10] == 1


# ---- the compiled instance ---------------------------------------------------------------------------------------------------
def test_quickgelu_instance_of_the_persistent_kernel_keeps_its_loop_clean():
    """gemm8p_kernel<true, G8_QGELU> (mangled ...ILb1ELi4ELb0E...) is cut from the template of the bf16 persistent kernel and is held
    to what tests/test_isa_guard.py holds that one to: no compiler-visible global load, no spill traffic inside the k-loop, exactly one
    wait on the vector-memory counter there (the counted vmcnt(6) of phase 4), no scratch at all, and no more registers than the
    exact-erf GELU instance needs.  The ragged companion's QuickGELU instances exist next to the two existing ones."""
    from test_isa_guard import _assembly
    text = _assembly("gemm8p.hip")
    found = re.findall(r"\n(_Z\w*gemm8p_kernelILb1ELi4ELb0E\w*):[^\n]*\n(.*?)\n\.Lfunc_end\d+:", text, flags=re.S)
    assert len(found) == 1
    name, body = found[0]
    lines = body.split("\n")
    in_asm, visible = False, []
    for l in lines:
        if ";;#ASMSTART" in l:
            in_asm = True
        elif ";;#ASMEND" in l:
            in_asm = False
        elif not in_asm and re.match(r"\s*(global_load|buffer_load|flat_load)", l):
            visible.append(l.strip())
    assert not visible, visible[:3]
    assert not [l for l in lines if "scratch_" in l]
    mf = [i for i, l in enumerate(lines) if "v_mfma" in l]
    head = max(i for i in range(mf[0]) if "Loop Header" in lines[i])
    assert [l.strip() for l in lines[head:mf[-1]] if "vmcnt" in l] == ["s_waitcnt vmcnt(6)"]
    assert sum("v_exp_f32" in l for l in lines) > 0 and sum("v_rcp_f32" in l for l in lines) > 0

    def figure(kernel, key):
        meta = re.search(r"\.name:\s+" + re.escape(kernel) + r"\n(.*?)\.wavefront_size", text, flags=re.S).group(1)
        return int(re.search(key + r":\s+(\d+)", meta).group(1))
    erf = re.search(r"\n(_Z\w*gemm8p_kernelILb1ELi0ELb0E\w*):", text).group(1)
    assert figure(name, r"\.private_segment_fixed_size") == 0
    assert figure(name, r"\.vgpr_count") <= figure(erf, r"\.vgpr_count")
    assert figure(name, r"\.sgpr_count") <= figure(erf, r"\.sgpr_count")
    ragged = set(re.findall(r"\n_Z\w*gemm8p_ragged_kernelILi(\d)E\w*:", text))
    assert ragged == {"1", "2", "5", "6"}, ragged
