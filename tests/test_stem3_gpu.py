"""The new device code of the ResNet-D/T members against float64 torch on the CPU, through the C ABI:
nkb_stem3_conv (narrow 3x3 / stride 1 / pad 1: every channel pair, forward and data gradient, fp32 and bf16, statistics, strides,
bias + ReLU), the generic deterministic weight gradient and the BatchNorm kernels at the narrow widths they had never run at, and
nkb_avgpool2x2 forward / backward.

Bounds.  fp32: the exact-fp32 MFMA is a chain of fused multiply-adds, one rounding per product, so for ANY accumulation order
|err| <= gamma_K (sum |w||x| + |bias|) with K = 9 Cin + 1, gamma_k = k u / (1 - k u), u = 2^-24 (Higham, Accuracy and Stability, 3.1).
bf16: operands are bf16-representable values fed to both sides; the bar is tol(bfloat16, 9 Cin) of tests/test_ops_gpu.py, what the
generic kernel is held to — the ratio to the fp32-accumulate bound plus the output rounding 2^-8 |y| is printed next to it."""
import math
import sys
from pathlib import Path

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

sys.path.insert(0, str(Path(__file__).resolve().parent))

from test_ops_gpu import tol  # noqa: E402
from nkb_classification import hip  # noqa: E402

DEV = "cuda"
DTYPES = [torch.float32, torch.bfloat16]
U = 2.0 ** -24
SHAPES = [(1, 5, 3), (2, 9, 11), (3, 16, 20), (2, 6, 112)]          # (2, 6, 112): the real row width (strip / halo splits of the launch)
# (kind, contraction channels, output channels): the three forward pairs and the three data-gradient pairs of the deep stem
PAIRS = [("fwd", 24, 32), ("fwd", 32, 32), ("fwd", 32, 64), ("dgrad", 32, 24), ("dgrad", 32, 32), ("dgrad", 64, 32)]


def gamma(k):
    return k * U / (1 - k * U)


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def _problem(kind, ci, co, N, H, W, dtype, seed, bias=False):
    """float64 truth of y = conv(x, w) (fwd) or of dX = conv^T(dY, w) (dgrad: ci = channels of dY, co = channels of dX), the operands in
    the layouts the engine hands the kernel, and S = sum |w||x| (+ |bias|) per output element."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, ci, H, W, generator=g).to(dtype).double()
    b = torch.randn(co, generator=g).double() if bias else None
    if kind == "fwd":
        w = (torch.randn(co, ci, 3, 3, generator=g) / math.sqrt(9 * ci)).to(dtype).double()
        ref = F.conv2d(x, w, b, padding=1)
        S = F.conv2d(x.abs(), w.abs(), b.abs() if bias else None, padding=1)
        wk = nhwc(w)                                               # [Cout][R][S][Cin]
    else:
        w = (torch.randn(ci, co, 3, 3, generator=g) / math.sqrt(9 * ci)).to(dtype).double()      # forward filter [Cout_f = ci][Cin_f = co]
        ref = F.conv_transpose2d(x, w, padding=1)
        S = F.conv_transpose2d(x.abs(), w.abs(), padding=1)
        if bias:
            ref, S = ref + b.view(1, -1, 1, 1), S + b.abs().view(1, -1, 1, 1)
        wk = w.permute(1, 2, 3, 0).contiguous()                    # [Cin_f][R][S][Cout_f]: the data-gradient layout of nkb_wprep
    return x, wk, b, nhwc(ref), nhwc(S)


def _run(kind, ci, co, N, H, W, dtype, x, wk, b=None, relu=False, stats=True, ldx=None, ldy=None):
    d = hip.dt(dtype)
    ldx, ldy = ldx or ci, ldy or co
    xd = torch.full((N, H, W, ldx), 7.0, dtype=dtype, device=DEV)
    xd[..., :ci] = nhwc(x).to(DEV, dtype)
    yd = torch.full((N, H, W, ldy), -77.0, dtype=dtype, device=DEV)
    tiles = hip.stem3_tiles(d, N, H, W, ci, co)
    assert tiles > 0
    st = torch.full((hip.bn_stats_floats(tiles, co),), float("nan"), device=DEV) if stats else None
    hip.stem3_conv(d, xd, wk.to(DEV, dtype), yd, N=N, H=H, W=W, Cin=ci, ldx=ldx, Cout=co, ldy=ldy, dgrad=kind == "dgrad",
                   bias=b.float().to(DEV) if b is not None else None, stats=st, relu=relu, tiles=tiles)
    torch.cuda.synchronize()
    return yd, st, tiles


def _check(tag, got, ref, S, K, dtype, y_for_rounding=None):
    err = (got.double() - ref).abs()
    bound = gamma(K) * S + (2.0 ** -8 * ref.abs() if dtype == torch.bfloat16 else 0.0)
    ratio = (err / bound.clamp_min(1e-300)).max().item()
    print(f"{tag}: max err {err.max().item():.3e}, max err / derived bound {ratio:.3f}")
    if dtype == torch.float32:
        assert (err <= bound).all(), (tag, ratio)
    else:
        torch.testing.assert_close(got.float(), ref.float(), **tol(dtype, K - 1))


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("kind,ci,co", PAIRS, ids=[f"{k}-{a}to{b}" for k, a, b in PAIRS])
def test_narrow_conv_against_float64(kind, ci, co, dtype):
    K = 9 * ci + 1
    for si, (N, H, W) in enumerate(SHAPES):
        x, wk, _, ref, S = _problem(kind, ci, co, N, H, W, dtype, seed=10 + si)
        yd, st, tiles = _run(kind, ci, co, N, H, W, dtype, x, wk)
        got = yd.cpu()
        _check(f"{kind} {ci}->{co} {N}x{H}x{W} {dtype}", got, ref, S, K, dtype)
        # statistics: sums of the STORED values, one row per workgroup, nothing written behind the advertised rows
        rows = st[:tiles * 2 * co].view(tiles, 2, co).double().sum(0).cpu()
        stored = got.double().reshape(-1, co)
        torch.testing.assert_close(rows[0], stored.sum(0), rtol=1e-4, atol=1e-2)
        torch.testing.assert_close(rows[1], (stored * stored).sum(0), rtol=1e-4, atol=1e-2)
        yd2, st2, _ = _run(kind, ci, co, N, H, W, dtype, x, wk)
        assert torch.equal(yd, yd2) and torch.equal(st[:tiles * 2 * co], st2[:tiles * 2 * co])      # no atomics: same bits
        # without statistics the output is the same
        yd3, _, _ = _run(kind, ci, co, N, H, W, dtype, x, wk, stats=False)
        assert torch.equal(yd, yd3)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("kind,ci,co", PAIRS, ids=[f"{k}-{a}to{b}" for k, a, b in PAIRS])
def test_narrow_conv_strides_bias_relu(kind, ci, co, dtype):
    """ldx = C + 8, ldy = C + 8 with sentinel-filled padding that must come back untouched; bias + ReLU in the epilogue (the eval fold)."""
    K = 9 * ci + 1
    N, H, W = 2, 9, 11
    x, wk, b, ref, S = _problem(kind, ci, co, N, H, W, dtype, seed=31, bias=True)
    yd, st, tiles = _run(kind, ci, co, N, H, W, dtype, x, wk, b=b, relu=True, ldx=ci + 8, ldy=co + 8)
    assert (yd[..., co:] == -77.0).all()                          # padding columns are never written
    got = yd[..., :co].cpu()
    _check(f"{kind} {ci}->{co} bias+relu ld+8 {dtype}", got, ref.clamp_min(0), S, K, dtype)
    stored = got.double().reshape(-1, co)
    rows = st[:tiles * 2 * co].view(tiles, 2, co).double().sum(0).cpu()
    torch.testing.assert_close(rows[0], stored.sum(0), rtol=1e-4, atol=1e-2)
    torch.testing.assert_close(rows[1], (stored * stored).sum(0), rtol=1e-4, atol=1e-2)
    # bias without ReLU, packed rows
    yd, _, _ = _run(kind, ci, co, N, H, W, dtype, x, wk, b=b, stats=False)
    _check(f"{kind} {ci}->{co} bias {dtype}", yd.cpu(), ref, S, K, dtype)


WG_CASES = [(24, 32), (32, 32), (32, 64), ("im2row", 24)]


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("ci,co", WG_CASES, ids=[f"{a}to{b}" for a, b in WG_CASES])
def test_generic_weight_gradient_at_the_narrow_shapes(ci, co, dtype):
    """The three stem weight gradients stay on the deterministic nkb_conv_wgrad (its check is Cin % 8): 3x3 at 24 / 32 input channels,
    and the first convolution (3 -> 24, 3x3 / stride 2) as a 1x1 product over its im2row matrix (27 columns padded to the k-tile)."""
    d = hip.dt(dtype)
    for N, P, Q in ((2, 9, 11), (2, 6, 112)):
        g = torch.Generator().manual_seed(P)
        if ci == "im2row":
            H, W = 2 * P, 2 * Q
            img = torch.randn(N, 3, H, W, generator=g).to(dtype).float()
            x64 = img.double().requires_grad_(True)
            w64 = (torch.randn(co, 3, 3, 3, generator=g) / math.sqrt(27)).double().requires_grad_(True)
            y = F.conv2d(x64, w64, stride=2, padding=1)
            kp = 128 // (2 if dtype == torch.bfloat16 else 4)
            xd = torch.empty(N, P, Q, kp, device=DEV, dtype=dtype)
            hip.im2row(d, img.to(DEV), xd, N, 3, H, W, 3, 3, 2, 1, kp)
            geom = dict(N=N * P * Q, H=1, W=1, Cin=kp, ldx=kp, P=1, Q=1, Cout=co, lddy=co)
            shape = (co, kp)
            pick = lambda dw: dw[:, :27].reshape(co, 3, 3, 3)          # noqa: E731   k = (r * 3 + s) * 3 + c
        else:
            x64 = torch.randn(N, ci, P, Q, generator=g).to(dtype).double().requires_grad_(True)
            w64 = (torch.randn(co, ci, 3, 3, generator=g) / math.sqrt(9 * ci)).double().requires_grad_(True)
            y = F.conv2d(x64, w64, padding=1)
            xd = nhwc(x64.detach()).to(DEV, dtype)
            geom = dict(N=N, H=P, W=Q, Cin=ci, ldx=ci, P=P, Q=Q, Cout=co, lddy=co, R=3, S=3, stride=1, pad=1)
            shape = (co, 3, 3, ci)
            pick = lambda dw: dw                                       # noqa: E731
        dy = torch.randn(y.shape, generator=g).to(dtype).double()
        y.backward(dy)
        ref = nhwc(w64.grad).float()
        dyd = nhwc(dy).to(DEV, dtype)
        need = hip.conv_wgrad_workspace(d, N=geom["N"], P=geom["P"], Q=geom["Q"], Cin=geom["Cin"], Cout=co, R=geom.get("R", 1),
                                        S=geom.get("S", 1), stride=geom.get("stride", 1), pad=geom.get("pad", 0))
        work = torch.full((need + 7,), float("nan"), device=DEV)
        runs = []
        for _ in range(2):
            dw = torch.zeros(shape, device=DEV)
            hip.conv_wgrad(d, dyd, xd, dw, workspace=work, **geom)
            torch.cuda.synchronize()
            runs.append(dw)
        assert torch.equal(runs[0], runs[1])
        assert torch.isnan(work[need:]).all()
        t = tol(torch.float32, N * P * Q)
        if dtype == torch.bfloat16:
            t = dict(rtol=1e-3, atol=1e-3 * math.sqrt(N * P * Q))
        got = pick(runs[0].cpu())
        print(f"wgrad {ci}->{co} {N}x{P}x{Q} {dtype}: max err {(got - ref).abs().max().item():.3e}")
        torch.testing.assert_close(got, ref, **t)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("C", [24, 32])
def test_batchnorm_kernels_at_the_narrow_widths(dtype, C):
    """bn_finalize / bn_apply (+ReLU) / bn_backward at 3 and 4 sixteen-byte vectors per row (bf16), bars of test_ops_gpu's BN tests."""
    torch.manual_seed(3)
    N, H, W = 2, 9, 11
    rows = N * H * W
    x = (torch.randn(N, C, H, W) * 2 + 0.5).to(dtype).float().requires_grad_(True)
    bn = torch.nn.BatchNorm2d(C)
    with torch.no_grad():
        bn.weight.uniform_(0.5, 1.5)
        bn.bias.normal_()
    y = torch.relu(bn(x))
    dy = torch.randn_like(y).to(dtype).float()
    y.backward(dy)
    d = hip.dt(dtype)
    xd = nhwc(x.detach()).to(DEV, dtype)
    xf = xd.float().reshape(rows, C)
    cut = 77
    partials = torch.zeros(hip.bn_stats_floats(2, C), device=DEV)
    partials[:4 * C].view(2, 2, C).copy_(torch.stack([torch.stack([xf[:cut].sum(0), (xf[:cut] ** 2).sum(0)]),
                                                      torch.stack([xf[cut:].sum(0), (xf[cut:] ** 2).sum(0)])]))
    gamma_, beta = bn.weight.detach().to(DEV), bn.bias.detach().to(DEV)
    rm, rv = torch.zeros(C, device=DEV), torch.ones(C, device=DEV)
    scale, shift, mean, invstd = (torch.empty(C, device=DEV) for _ in range(4))
    hip.bn_finalize(partials, 2, C, rows, gamma_, beta, rm, rv, 0.1, 1e-5, True, scale, shift, mean, invstd)
    yd = torch.full_like(xd, -5.0)
    hip.bn_apply(d, xd, None, yd, scale, shift, rows, C, True)
    torch.cuda.synchronize()
    torch.testing.assert_close(rm.cpu(), bn.running_mean, rtol=1e-4, atol=1e-5)
    torch.testing.assert_close(rv.cpu(), bn.running_var, rtol=1e-4, atol=1e-5)
    torch.testing.assert_close(yd.float().cpu(), nhwc(y.detach()), **tol(dtype))
    dgamma, dbeta = torch.zeros(C, device=DEV), torch.zeros(C, device=DEV)
    dx = torch.full_like(xd, -5.0)
    ws = torch.empty(hip.bn_backward_ws(rows, C), device=DEV)
    yact = nhwc(y.detach()).to(DEV, dtype)                         # mask from the torch activation: both sides agree on borderline zeros
    hip.bn_backward(d, nhwc(dy).to(DEV, dtype), xd, yact, mean, invstd, gamma_, rows, C, dgamma, dbeta, dx, None, ws)
    torch.cuda.synchronize()
    t = tol(dtype, rows)
    torch.testing.assert_close(dbeta.cpu(), bn.bias.grad, **t)
    torch.testing.assert_close(dgamma.cpu(), bn.weight.grad, **t)
    torch.testing.assert_close(dx.float().cpu(), nhwc(x.grad), **tol(dtype, 4))
    # the form the stem uses: mask recomputed from x * scale + shift
    dgamma.zero_(); dbeta.zero_()
    hip.bn_backward(d, nhwc(dy).to(DEV, dtype), xd, None, mean, invstd, gamma_, rows, C, dgamma, dbeta, dx, None, ws,
                    fscale=scale, fshift=shift)
    torch.cuda.synchronize()
    if dtype == torch.float32:      # in bf16 the torch reference masks on unrounded values; borderline zeros may differ
        torch.testing.assert_close(dbeta.cpu(), bn.bias.grad, **t)
        torch.testing.assert_close(dgamma.cpu(), bn.weight.grad, **t)
        torch.testing.assert_close(dx.float().cpu(), nhwc(x.grad), **tol(dtype, 4))
    else:
        assert torch.isfinite(dx.float()).all() and torch.isfinite(dgamma).all()


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("C", [64, 256])
def test_avgpool2x2_forward_backward(dtype, C):
    """AvgPool2d(2, 2, ceil_mode=True, count_include_pad=False): fp32 forward within gamma_4 * sum|x| / count, backward within 2 ulp
    (the division is by 1, 2 or 4: exact); bf16 adds the output rounding 2^-8 |y|.  Every input-gradient element is written."""
    d = hip.dt(dtype)
    for si, (N, H, W) in enumerate([(2, 9, 10), (1, 1, 1), (2, 18, 19), (1, 7, 8)]):
        g = torch.Generator().manual_seed(50 + si)
        x = torch.randn(N, C, H, W, generator=g).to(dtype).double().requires_grad_(True)
        ref = F.avg_pool2d(x, 2, 2, ceil_mode=True, count_include_pad=False)
        S = F.avg_pool2d(x.detach().abs(), 2, 2, ceil_mode=True, count_include_pad=False)      # sum |x| / count
        P, Q = (H + 1) // 2, (W + 1) // 2
        assert ref.shape == (N, C, P, Q)
        gy = torch.randn(N, C, P, Q, generator=g).to(dtype).double()
        ref.backward(gy)
        xd = nhwc(x.detach()).to(DEV, dtype)
        yd = torch.full((N, P, Q, C), -77.0, device=DEV, dtype=dtype)
        hip.avgpool2x2(d, False, xd, yd, N, H, W, C)
        dxd = torch.full((N, H, W, C), -77.0, device=DEV, dtype=dtype)      # sentinel: every element must be written
        hip.avgpool2x2(d, True, nhwc(gy).to(DEV, dtype), dxd, N, H, W, C)
        torch.cuda.synchronize()
        r = nhwc(ref.detach())
        out_rnd = 2.0 ** -8 if dtype == torch.bfloat16 else 0.0
        err = (yd.cpu().double() - r).abs()
        assert (err <= gamma(4) * nhwc(S) + out_rnd * r.abs()).all(), (N, H, W, err.max().item())
        rg = nhwc(x.grad)
        errg = (dxd.cpu().double() - rg).abs()
        assert (errg <= (2 * 2.0 ** -23 + out_rnd) * rg.abs()).all(), (N, H, W, errg.max().item())
