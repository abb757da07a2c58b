"""Every instance of the depthwise 7x7 convolution (csrc/dwconv.hip: forward, data gradient, weight + bias gradient, fp32 and bf16)
and of the layer scale against float64 torch on the CPU (F.conv2d(groups=C) and autograd).

The bounds are derived, not tuned.  u = 2^-24, gamma_k = k u / (1 - k u):
  forward / data gradient   fp32: |err| <= gamma_50 (|bias| + sum |w||x|) per element (49 products and the bias, any order);
                            bf16: the same + 2^-8 |y| for the single rounding of the output.  In bf16 the activations are
                            bf16-representable values fed to both sides; the filter is the unrounded fp32 master.
  weight / bias gradient    |err| <= gamma_M sum |g||x| per element, M = N H W — holds for ANY summation order, so it does not depend
                            on how the kernel splits the sum.
The test prints, next to the engine's worst error / bound ratio, the same ratio for torch's own fp32 CPU result on the same data."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from nkb_classification import hip  # noqa: E402

DEV = "cuda:0"
U = 2.0 ** -24
# the last two: more (image, row chunk, column strip) work items than weight-gradient splits (1 280 > 1 024, 200 > 128), so that one
# wave sums several items — the path every batch-256 launch takes
SHAPES = [(128, 56, 56, 2), (256, 28, 28, 2), (512, 14, 14, 3), (1024, 7, 7, 3), (128, 17, 18, 2), (128, 5, 3, 1),
          (128, 56, 56, 40), (1024, 7, 7, 200)]
DTYPES = [torch.float32, torch.bfloat16]


def _gamma(k):
    return k * U / (1 - k * U)


def _data(C, H, W, N, dtype, seed=0):
    g = torch.Generator().manual_seed(seed + C + 7 * H + W)
    x = torch.randn(N, H, W, C, generator=g).to(dtype)           # NHWC, representable in the compute dtype
    gy = torch.randn(N, H, W, C, generator=g).to(dtype)
    w = torch.randn(C, 1, 7, 7, generator=g) * 0.2               # fp32 master, unrounded
    b = torch.randn(C, generator=g)
    return x, gy, w, b


def _nchw(t):
    return t.permute(0, 3, 1, 2)


def _truth(x, gy, w, b, dt=torch.float64):
    """(y, dx, dw, db) in dtype dt on the CPU, all NHWC / [C,1,7,7]; and the magnitude sums of the bounds (float64 only)."""
    xs = _nchw(x.to(dt)).clone().requires_grad_(True)
    ws, bs = w.to(dt).clone().requires_grad_(True), b.to(dt).clone().requires_grad_(True)
    y = F.conv2d(xs, ws, bs, padding=3, groups=x.shape[-1])
    dx, dw, db = torch.autograd.grad(y, (xs, ws, bs), _nchw(gy.to(dt)))
    return y.detach().permute(0, 2, 3, 1), dx.permute(0, 2, 3, 1), dw, db


def _magnitudes(x, gy, w, b):
    return _truth(x.abs(), gy.abs(), w.abs(), b.abs())


def _flat_w(dw):
    return dw.reshape(dw.shape[0], 49)


def _run_engine(x, gy, w, b, dtype, ld_extra=0):
    N, H, W, C = x.shape
    d = hip.dt(dtype)
    ld = C + ld_extra
    def dev(t):
        buf = torch.full((N, H, W, ld), 7.0, dtype=dtype, device=DEV)
        buf[..., :C] = t.to(DEV)
        return buf
    xd, gd = dev(x), dev(gy)
    wd, bd = w.reshape(C, 49).contiguous().to(DEV), b.to(DEV)
    y = torch.full((N, H, W, ld), 7.0, dtype=dtype, device=DEV)
    dx = torch.full((N, H, W, ld), 7.0, dtype=dtype, device=DEV)
    hip.dwconv(d, xd, wd, bd, y, N=N, H=H, W=W, C=C, ldx=ld, ldy=ld)
    hip.dwconv(d, gd, wd, None, dx, N=N, H=H, W=W, C=C, ldx=ld, ldy=ld, dgrad=True)
    work = torch.empty(hip.dwconv_wgrad_workspace(d, N, H, W, C), device=DEV)
    outs = []
    for _ in range(2):
        dw, db = torch.zeros(C, 49, device=DEV), torch.zeros(C, device=DEV)
        hip.dwconv_wgrad(d, gd, xd, dw, db, N=N, H=H, W=W, C=C, ldg=ld, ldx=ld, workspace=work)
        outs.append((dw, db))
    torch.cuda.synchronize()
    if ld_extra:
        assert bool((y[..., C:] == 7.0).all()) and bool((dx[..., C:] == 7.0).all())      # the row padding is never written
    return y[..., :C].cpu(), dx[..., :C].cpu(), outs


def _check(C, H, W, N, dtype, ld_extra=0):
    x, gy, w, b = _data(C, H, W, N, dtype)
    y64, dx64, dw64, db64 = _truth(x, gy, w, b)
    ym, dxm, dwm, dbm = _magnitudes(x, gy, w, b)
    y, dx, outs = _run_engine(x, gy, w, b, dtype, ld_extra)
    (dw, db), (dw2, db2) = outs
    if N >= 40:
        # the multi-item cases are what they claim to be.  Mirrors csrc/dwconv.hip: DW_ROWS = 14 rows per chunk, DW_TW = 7 columns per
        # strip, 50 C floats of workspace per split (valid where H is a multiple of 14 or below it, as in both shapes)
        floats = hip.dwconv_wgrad_workspace(hip.dt(dtype), N, H, W, C)
        assert N * ((H + 13) // 14) * ((W + 6) // 7) > floats // (50 * C)
    assert torch.equal(dw, dw2) and torch.equal(db, db2)                  # two launches, identical bits
    M = N * H * W
    out_round = 2.0 ** -8 if dtype == torch.bfloat16 else 0.0
    tiny = 1e-300
    bounds = dict(
        y=(y.double(), y64, _gamma(50) * ym + out_round * y64.abs()),
        dx=(dx.double(), dx64, _gamma(50) * dxm + out_round * dx64.abs()),
        dw=(_flat_w(dw.cpu().double()), _flat_w(dw64), _gamma(M) * _flat_w(dwm)),
        db=(db.cpu().double(), db64, _gamma(M) * dbm),
    )
    # torch's own fp32 CPU result on the same data, against the same truth and bound (the tighter evidence)
    t32 = dict(zip(("y", "dx", "dw", "db"), _truth(x, gy, w, b, torch.float32)))
    line = []
    for k, (got, ref, bound) in bounds.items():
        ratio = ((got - ref).abs() / (bound + tiny)).max().item()
        ref32 = t32[k].double()
        if k == "dw":
            ref32 = _flat_w(ref32)
        if dtype == torch.bfloat16 and k in ("y", "dx"):
            ref32 = ref32.to(torch.bfloat16).double()
        r32 = ((ref32 - ref).abs() / (bound + tiny)).max().item()
        line.append(f"{k} {ratio:.3f} (torch fp32 cpu {r32:.3f})")
    print(f"\n[dwconv C={C} {H}x{W} N={N} {str(dtype)[6:]} ld+{ld_extra}] worst |err| / bound: " + "  ".join(line))
    for k, (got, ref, bound) in bounds.items():
        assert got.shape == ref.shape, k
        bad = (got - ref).abs() > bound
        assert not bool(bad.any()), (k, int(bad.sum()), ((got - ref).abs() / (bound + tiny)).max().item())


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape", SHAPES, ids=[f"C{c}_{h}x{w}_N{n}" for c, h, w, n in SHAPES])
def test_dwconv_all_passes_against_float64(shape, dtype):
    _check(*shape, dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
def test_dwconv_strided_rows(dtype):
    """Pixel stride larger than C (ldx = ldy = C + 64): operands embedded in wider rows; the padding is never written."""
    _check(128, 17, 18, 2, dtype, ld_extra=64)


def test_dwconv_data_gradient_adds_the_residual_gradient():
    """The optional add operand (the residual path's gradient in a block's backward): dx = add + dgrad(g), one rounding."""
    C, H, W, N = 128, 9, 10, 2
    for dtype in DTYPES:
        x, gy, w, b = _data(C, H, W, N, dtype, seed=3)
        _, dx64, _, _ = _truth(x, gy, w, b)
        _, dxm, _, _ = _magnitudes(x, gy, w, b)
        add = x                                              # any tensor of the same shape
        d = hip.dt(dtype)
        out = torch.empty(N, H, W, C, dtype=dtype, device=DEV)
        hip.dwconv(d, gy.to(DEV), w.reshape(C, 49).contiguous().to(DEV), None, out, N=N, H=H, W=W, C=C, ldx=C, ldy=C, dgrad=True,
                   add=add.to(DEV))
        ref = dx64 + add.double()
        bound = _gamma(51) * (dxm + add.double().abs()) + (2.0 ** -8 if dtype == torch.bfloat16 else 0.0) * ref.abs()
        assert bool(((out.cpu().double() - ref).abs() <= bound).all())


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("rows,C", [(6272, 128), (300, 1024), (37, 192)])
def test_layer_scale_against_float64(rows, C, dtype):
    """out = add + gamma z (one fused multiply-add, then the output rounding); backward gz = gamma g, dgamma = sum_m g z with
    |err| <= gamma_rows sum |g z| for any order; two launches give identical bits."""
    g = torch.Generator().manual_seed(rows + C)
    z, a, gr = (torch.randn(rows, C, generator=g).to(dtype) for _ in range(3))
    gam = torch.rand(C, generator=g) + 0.5
    d = hip.dt(dtype)
    zd, ad, gd, gmd = z.to(DEV), a.to(DEV), gr.to(DEV), gam.to(DEV)
    out, gz = torch.empty_like(zd), torch.empty_like(zd)
    hip.layer_scale(d, False, zd, ad, gmd, out, rows, C)
    work = torch.empty(hip.layer_scale_workspace(rows, C), device=DEV)
    dgs = []
    for _ in range(2):
        dg = torch.zeros(C, device=DEV)
        hip.layer_scale(d, True, zd, gd, gmd, gz, rows, C, dgamma=dg, workspace=work)
        dgs.append(dg)
    torch.cuda.synchronize()
    assert torch.equal(dgs[0], dgs[1])
    rnd = 2.0 ** -8 if dtype == torch.bfloat16 else 0.0
    z64, a64, g64, gm64 = z.double(), a.double(), gr.double(), gam.double()
    ref = a64 + gm64 * z64
    assert bool(((out.cpu().double() - ref).abs() <= _gamma(2) * (a64.abs() + (gm64 * z64).abs()) + rnd * ref.abs()).all())
    ref = gm64 * g64
    assert bool(((gz.cpu().double() - ref).abs() <= (_gamma(1) + rnd) * ref.abs()).all())
    ref = (g64 * z64).sum(0)
    assert bool(((dgs[0].cpu().double() - ref).abs() <= _gamma(rows) * (g64 * z64).abs().sum(0)).all())
