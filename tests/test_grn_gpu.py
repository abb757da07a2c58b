"""Global response normalisation (csrc/grn.hip through hip.grn / hip.grn_backward: forward, data gradient with and without the fused
multiplier, weight + bias gradient, fp32 and bf16) against float64 on the CPU.

The truth is the closed form of the operator and its gradient (checked below against float64 autograd of the twin's timm expression,
an all-zero (image, channel) pair included):
    S = sum_p u^2   G = sqrt(S)   m = mean_c G + eps   N = G / m   s = 1 + w N   out = u s + bias
    P = sum_p g u   Q = sum_p g   dbias = sum_b Q   dweight = sum_b N P
    dN = w P   A = sum_c dN G   dG = dN / m - A / (Ch m^2)   t = dG / G (0 where S == 0)   du = g s + u t

The bounds are derived, not tuned.  u = 2^-24, gamma_k = k u / (1 - k u), k = HW + Ch + 16: the sum over the pixels, the sum over the
channels and fewer than 16 scalar roundings in any chain.  They are applied to the same formulas evaluated on absolute values:
    out      gamma_k (|u| (1 + |w| N) + |bias|)
    du       gamma_k (|g| s_ + |u| t_),  s_ = 1 + |w| N,  t_ = (|w| P_ / m + A_ / (Ch m^2)) / G,  P_ = sum_p |g||u|,  A_ = sum_c |w| P_ G
    dweight  gamma_{k+N} sum_b N P_
    dbias    gamma_{N HW} sum |g|
bf16 adds 2^-8 |ref| for the single rounding of out / du; the fused multiplier adds one rounding (k + 1) and scales the bound by |mul|.
The test prints, next to the engine's worst error / bound ratio, the same ratio for torch's own fp32 CPU result on the same data."""
import sys
from pathlib import Path

import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, str(Path(__file__).resolve().parent))

from convnextv2_reference import grn as twin_grn  # noqa: E402
from nkb_classification import hip  # noqa: E402

DEV = "cuda:0"
U = 2.0 ** -24
EPS = 1e-6
# (Ch, HW, N): a real stage-0 image; the widest table with an odd HW; a 17x18 grid; the 64-px test member's last stage; HW = 1 (G = |u|);
# more (image, channel group) work items than workgroups (12 800 > 8 per CU), the path every batch-256 launch takes
SHAPES = [(512, 3136, 2), (4096, 49, 3), (512, 306, 2), (1024, 4, 4), (1024, 1, 2), (4096, 49, 200)]
DTYPES = [torch.float32, torch.bfloat16]


def _gamma(k):
    return k * U / (1 - k * U)


def _data(Ch, HW, N, dtype, seed=0):
    g = torch.Generator().manual_seed(seed + Ch + 7 * HW + N)
    u = torch.randn(N, HW, Ch, generator=g).to(dtype)            # representable in the compute dtype
    gy = torch.randn(N, HW, Ch, generator=g).to(dtype)
    u[0, :, 5] = 0                                               # one all-zero (image, channel) pair: t = 0 there, everything finite
    w = torch.rand(Ch, generator=g) * 2 - 1                      # fp32, unrounded
    b = torch.randn(Ch, generator=g)
    return u, gy, w, b


def _closed_form(u, gy, w, b, dt=torch.float64, magnitudes=False):
    """dict(out, du, dw, db) in dtype dt on the CPU; magnitudes: the same formulas on absolute values with sums for differences."""
    u, gy, w, b = u.to(dt), gy.to(dt), w.to(dt), b.to(dt)
    Ch = u.shape[-1]
    S = (u * u).sum(1)
    G = S.sqrt()
    m = G.mean(-1, keepdim=True) + EPS
    Nn = G / m
    if magnitudes:
        u, gy, w, b = u.abs(), gy.abs(), w.abs(), b.abs()
    s = 1 + w * Nn
    P, Q = (gy * u).sum(1), gy.sum(1)
    dN = w * P
    A = (dN * G).sum(-1, keepdim=True)
    dG = dN / m + A / (Ch * m * m) if magnitudes else dN / m - A / (Ch * m * m)
    t = torch.where(S > 0, dG / G.clamp_min(1e-300 if dt == torch.float64 else 1e-30), torch.zeros_like(dG))
    out = u * s[:, None, :] + b
    du = gy * s[:, None, :]
    du.addcmul_(u, t[:, None, :])
    return dict(out=out, du=du, dw=(Nn * P).sum(0), db=Q.sum(0))


def test_closed_form_equals_autograd_of_the_twin():
    u, gy, w, b = _data(128, 30, 3, torch.float32, seed=9)
    us, ws, bs = (t.double().clone().requires_grad_(True) for t in (u, w, b))
    out = twin_grn(us, ws, bs, EPS)
    du, dw, db = torch.autograd.grad(out, (us, ws, bs), gy.double())
    cf = _closed_form(u, gy, w, b)
    for k, ref in dict(out=out.detach(), du=du, dw=dw, db=db).items():
        assert torch.isfinite(ref).all() and (cf[k] - ref).abs().max().item() <= 1e-12 * max(1.0, ref.abs().max().item()), k
    assert bool((du[0, :, 5] == gy.double()[0, :, 5]).all())     # the zero pair: s = 1, t = 0


def _run_engine(u, gy, w, b, dtype, mul=None, init=None):
    N, HW, Ch = u.shape
    d = hip.dt(dtype)
    ud, gd, wd, bd = u.to(DEV), gy.to(DEV), w.to(DEV), b.to(DEV)
    md = mul.to(DEV) if mul is not None else None
    work = torch.empty(hip.grn_workspace(N, HW, Ch), device=DEV)
    runs = []
    for _ in range(2):
        out, du = torch.full_like(ud, 7.0), torch.full_like(ud, 7.0)
        sumsq = torch.full((N, Ch), 7.0, device=DEV)
        dw = torch.zeros(Ch, device=DEV) if init is None else init[0].to(DEV)
        db = torch.zeros(Ch, device=DEV) if init is None else init[1].to(DEV)
        hip.grn(d, ud, wd, bd, out, sumsq, N, HW, Ch, eps=EPS)
        hip.grn_backward(d, gd, ud, wd, sumsq, du, dw, db, N, HW, Ch, eps=EPS, mul=md, workspace=work)
        runs.append(dict(out=out, du=du, dw=dw, db=db, sumsq=sumsq))
    torch.cuda.synchronize()
    for k in runs[0]:
        assert torch.equal(runs[0][k], runs[1][k]), f"{k}: two launches differ"
    return {k: v.cpu() for k, v in runs[0].items()}


def _check(Ch, HW, N, dtype, with_mul=False):
    u, gy, w, b = _data(Ch, HW, N, dtype)
    mul = None
    if with_mul:
        mul = torch.randn(N, HW, Ch, generator=torch.Generator().manual_seed(11)).to(dtype)
    ref, mag = _closed_form(u, gy, w, b), _closed_form(u, gy, w, b, magnitudes=True)
    t32 = _closed_form(u, gy, w, b, torch.float32)
    got = _run_engine(u, gy, w, b, dtype, mul)
    k = HW + Ch + 16
    rnd = 2.0 ** -8 if dtype == torch.bfloat16 else 0.0
    if with_mul:
        ref["du"] = ref["du"] * mul.double()
        t32["du"] = t32["du"] * mul.float()
        du_bound = _gamma(k + 1) * mag["du"] * mul.double().abs() + rnd * ref["du"].abs()
    else:
        du_bound = _gamma(k) * mag["du"] + rnd * ref["du"].abs()
    bounds = dict(out=_gamma(k) * mag["out"] + rnd * ref["out"].abs(), du=du_bound, dw=_gamma(k + N) * mag["dw"], db=_gamma(N * HW) * mag["db"])
    assert bool((got["sumsq"][0, 5] == 0).all()) and all(bool(torch.isfinite(v).all()) for v in got.values())
    tiny = 1e-300
    line = []
    for name, bound in bounds.items():
        g64 = got[name].double()
        ratio = ((g64 - ref[name]).abs() / (bound + tiny)).max().item()
        r32 = t32[name]
        if dtype == torch.bfloat16 and name in ("out", "du"):
            r32 = r32.to(torch.bfloat16)
        r32 = ((r32.double() - ref[name]).abs() / (bound + tiny)).max().item()
        line.append(f"{name} {ratio:.3f} (torch fp32 cpu {r32:.3f})")
    print(f"\n[grn Ch={Ch} HW={HW} N={N} {str(dtype)[6:]}{' mul' if with_mul else ''}] worst |err| / bound: " + "  ".join(line))
    for name, bound in bounds.items():
        assert got[name].shape == ref[name].shape, name
        bad = (got[name].double() - ref[name]).abs() > bound
        assert not bool(bad.any()), (name, int(bad.sum()), ((got[name].double() - ref[name]).abs() / (bound + tiny)).max().item())
    return u, gy, w, b, got


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape", SHAPES, ids=[f"Ch{c}_HW{h}_N{n}" for c, h, n in SHAPES])
def test_grn_all_passes_against_float64(shape, dtype):
    Ch, HW, N = shape
    if N >= 200:                                                 # the multi-item case is what it claims to be (csrc/grn.hip: 64 channels
        cus = torch.cuda.get_device_properties(0).multi_processor_count      # per item, at most 8 workgroups per CU)
        assert N * (Ch // 64) > 8 * cus
    _check(Ch, HW, N, dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
def test_grn_backward_with_the_fused_multiplier(dtype):
    """du * mul in the apply pass (the activation derivative of the MLP: GELU backward rides along), one more rounding."""
    _check(512, 306, 2, dtype, with_mul=True)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
def test_grn_parameter_gradients_accumulate(dtype):
    """dweight / dbias are "+=": onto a non-zero start the result is exactly fl(start + the sums a zero start gives)."""
    Ch, HW, N = 1024, 4, 4
    u, gy, w, b = _data(Ch, HW, N, dtype)
    zero = _run_engine(u, gy, w, b, dtype)
    g = torch.Generator().manual_seed(2)
    init = (torch.randn(Ch, generator=g), torch.randn(Ch, generator=g))
    acc = _run_engine(u, gy, w, b, dtype, init=(init[0].clone(), init[1].clone()))
    assert torch.equal(acc["dw"], init[0] + zero["dw"]) and torch.equal(acc["db"], init[1] + zero["db"])
    assert not torch.equal(acc["dw"], zero["dw"])
