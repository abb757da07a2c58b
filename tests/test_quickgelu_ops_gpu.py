"""QuickGELU kernels through the C ABI: nkb_gelu / nkb_gelu_fwd_dgelu with kind 1 (csrc/transformer.hip), acts 7 / 8 of
nkb_linear_gelu on the generic kernel (csrc/conv_igemm.hip) and act 9 on the eight-phase core (csrc/gemm8p.hip: the QuickGELU
instance of the persistent kernel, its run-time epilogue on a ragged row block, and both instances of the ragged-row companion),
against float64.  The GEMM outputs are held to the yardstick, metric and bound of tests/gemm_reference.py (tests/test_quickgelu_cpu.py
proves that the bound rejects a wrong activation and a wrong derivative); every figure is printed (-rP)."""
import math
from dataclasses import replace

import pytest
import torch

import gemm_reference as gr
import quickgelu_gemm_reference as qr

pytestmark = pytest.mark.gpu

from nkb_classification import hip  # noqa: E402
from test_gemm8p_gpu import G, SENT, _bits, _cus, _guards_intact, _input, _output  # noqa: E402
from test_ops_gpu import tol  # noqa: E402

DEV = "cuda"
DTYPES = [torch.float32, torch.bfloat16]
SPECIAL = [0.0, 1e-4, -1e-4, 12.0, -12.0, -30.0, -90.0]


def _points(dtype, seed):
    """5000 = 625 x 8 values (whole 16-byte vectors): N(0, 2^2) with the special points in front, rounded to the dtype"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(5000, generator=g) * 2
    x[:len(SPECIAL)] = torch.tensor(SPECIAL)
    return x.to(dtype)


def _hold_elementwise(tag, got, ref, dtype):
    got, ref = got.double().cpu(), ref.double()
    assert torch.isfinite(got).all(), tag
    err = (got - ref).abs()
    if dtype == torch.float32:
        print(f"{tag}: max abs error {err.max().item():.3e}")
        torch.testing.assert_close(got, ref, **tol(torch.float32))
    else:
        # half a bf16 ulp of the stored value plus an fp32-level term for rcp and exp2, the form tests/test_attention_gpu.py uses for P
        bound = (2.0 ** -8 + 2.0 ** -20) * ref.abs() + 1e-6
        worst = (err / bound).max().item()
        print(f"{tag}: worst error / bound {worst:.3f}")
        assert worst <= 1.0, (tag, worst)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
def test_elementwise_quickgelu_forward_backward_and_in_place_derivative(dtype):
    d, n = hip.dt(dtype), 5000
    x, dy = _points(dtype, 11), _points(dtype, 12)
    u64, d64 = qr.quick_gelu_pair(x.double())
    xd, dyd = x.to(DEV), dy.to(DEV)
    y, dx, y2 = torch.empty_like(xd), torch.empty_like(xd), torch.empty_like(xd)
    hip.gelu(d, xd, None, y, n, hip.ACT_QUICK_GELU)
    hip.gelu(d, xd, dyd, dx, n, kind=hip.ACT_QUICK_GELU)
    gp = xd.clone()
    hip.gelu_fwd_dgelu(d, gp, y2, gp, n, hip.ACT_QUICK_GELU)         # in place: gp now holds quickgelu'(x)
    torch.cuda.synchronize()
    _hold_elementwise("forward", y, u64, dtype)
    _hold_elementwise("backward", dx, dy.double() * d64, dtype)
    _hold_elementwise("forward of fwd_dgelu", y2, u64, dtype)
    _hold_elementwise("stored derivative", gp, d64, dtype)
    # where the exponential overflows (-90; fp32 also -60) both results are zeros, and 0 gives (0, 1/2)
    i0, i90 = SPECIAL.index(0.0), SPECIAL.index(-90.0)
    assert y[i90].item() == 0 and gp[i90].item() == 0 and y[i0].item() == 0 and gp[i0].item() == 0.5
    # kind 0 is the exact-erf kernel, bit for bit what a call without the argument gives
    a, b, c, e = (torch.empty_like(xd) for _ in range(4))
    hip.gelu(d, xd, None, a, n)
    hip.gelu(d, xd, None, b, n, hip.ACT_GELU)
    hip.gelu(d, xd, dyd, c, n)
    hip.gelu(d, xd, dyd, e, n, kind=0)
    g0, g1, z0, z1 = xd.clone(), xd.clone(), torch.empty_like(xd), torch.empty_like(xd)
    hip.gelu_fwd_dgelu(d, g0, z0, g0, n)
    hip.gelu_fwd_dgelu(d, g1, z1, g1, n, 0)
    torch.cuda.synchronize()
    for p, q in ((a, b), (c, e), (g0, g1), (z0, z1)):
        assert torch.equal(_bits(p), _bits(q))
    torch.testing.assert_close(a.float().cpu(), torch.nn.functional.gelu(x.float()), **tol(dtype))
    assert not torch.equal(a, y)


def test_elementwise_quickgelu_is_finite_at_the_ends_of_the_range():
    """|x| up to the largest finite value of the dtype (1.702 x overflows there; the kernels never form it) and across the point
    where exp(-1.702 x) overflows: every output finite, in both dtypes."""
    for dtype in DTYPES:
        big = torch.finfo(dtype).max
        x = torch.tensor([big, -big, big / 2, -big / 2, 52.0, -52.0, 52.5, -52.5, 75.0, -75.0, 88.0, -88.0, 1e30, -1e30, 1e-30, -1e-30],
                         dtype=dtype, device=DEV)
        y, dx, gp = torch.empty_like(x), torch.empty_like(x), x.clone()
        hip.gelu(hip.dt(dtype), x, None, y, 16, hip.ACT_QUICK_GELU)
        hip.gelu(hip.dt(dtype), x, torch.ones_like(x), dx, 16, hip.ACT_QUICK_GELU)
        hip.gelu_fwd_dgelu(hip.dt(dtype), gp, torch.empty_like(x), gp, 16, hip.ACT_QUICK_GELU)
        torch.cuda.synchronize()
        assert torch.isfinite(y.float()).all() and torch.isfinite(dx.float()).all() and torch.isfinite(gp.float()).all(), dtype
        assert y[0].item() == x[0].item() and y[1].item() == 0 and dx[0].item() == 1 and dx[1].item() == 0
        assert torch.equal(_bits(dx), _bits(gp))


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
def test_generic_kernel_acts_7_and_8(dtype):
    """M = 200, K = 128, N = 192: the eight-phase core refuses that width, so both acts run the generic epilogue (no gemm8p launch).
    act 7 is the twin of act 1: it stores the pre-activation ROUNDED to the dtype in y2 and applies QuickGELU to that stored value
    (what act 8 differentiates later), so the bf16 yardstick rounds the pre-activation where the kernel does.  The rows of the
    output buffers past M (where the last tile's overhang past N and M would land) are NaN before and after."""
    M, K, N = 200, 128, 192
    d = hip.dt(dtype)
    g = torch.Generator().manual_seed(21)
    x = torch.randn(M, K, generator=g).to(dtype)
    w = (torch.randn(N, K, generator=g) / math.sqrt(K) * 1.5).to(dtype)
    bias = torch.randn(N, generator=g) * 0.5
    gy = torch.randn(M, K, generator=g).to(dtype)                  # fc2's incoming gradient, [M][K2] with K2 = K
    w2t = (torch.randn(N, K, generator=g) / math.sqrt(N)).to(dtype)
    y = torch.full((M + 8, N), float("nan"), device=DEV, dtype=dtype)
    y2 = torch.full((M + 8, N), float("nan"), device=DEV, dtype=dtype)
    dpre = torch.full((M + 8, N), float("nan"), device=DEV, dtype=dtype)
    n0 = hip.kernel_launches("gemm8p")
    hip.linear_gelu(d, 7, x.to(DEV), w.to(DEV), bias.to(DEV), None, y, y2, M, K, N)
    hip.linear_gelu(d, 8, gy.to(DEV), w2t.to(DEV), None, y2, dpre, None, M, K, N)
    torch.cuda.synchronize()
    assert hip.kernel_launches("gemm8p") == n0
    for t in (y, y2, dpre):
        assert torch.isnan(t[M:].float()).all() and torch.isfinite(t[:M].float()).all()
    p = gr.product(x.double(), w.double())
    pre64 = p + bias.double()
    pre_stored = y2[:M].double().cpu()
    p2 = gr.product(gy.double(), w2t.double())
    if dtype == torch.float32:
        torch.testing.assert_close(pre_stored, pre64, **tol(dtype, K))
        torch.testing.assert_close(y[:M].double().cpu(), qr.quick_gelu_pair(pre64)[0], **tol(dtype, K))
        torch.testing.assert_close(dpre[:M].double().cpu(), p2 * qr.quick_gelu_pair(pre_stored)[1], **tol(dtype, K))
        return
    pre_yard = gr.bf((p.float() + bias))                           # fp32 accumulator + bias, rounded where the kernel stores it
    qr.hold("act7", "y2", pre_stored, pre64, pre_yard)
    qr.hold("act7", "y", y[:M].double().cpu(), qr.quick_gelu_pair(pre64)[0], gr.bf(qr.quick_gelu_pair(pre_yard)[0]))
    # act 8 multiplies by quickgelu'(aux) of the aux it is GIVEN (the stored pre-activation): reference and yardstick take the same aux
    ref8 = p2 * qr.quick_gelu_pair(pre_stored)[1]
    yard8 = gr.bf(p2.float() * qr.quick_gelu_pair(pre_stored.float())[1])
    qr.hold("act8", "y", dpre[:M].double().cpu(), ref8, yard8)


GELU2 = [c for c in gr.CASES if c.epi == "gelu2"]
# the issue's cases are every gelu2 Case of the table (a full-tile walk and the companion at R = 1); two more of the same epilogue reach
# the instances those leave out: the companion's two-fragment form (R = 100) and the persistent kernel's run-time epilogue on a ragged
# row block that stays with it (M = 300: two row blocks, no round saved by the companion)
EXTRA = [replace(next(c for c in GELU2 if c.companion), name="ragged_R100", M=64 * 256 + 100, regime="R = 100, S = 16"),
         gr.Case("small_M300", gr.G_TRUE0, "two row blocks, the second ragged, run-time epilogue", 300, 256, 256, "gelu2", everywhere=True)]


@pytest.mark.parametrize("case", GELU2 + EXTRA, ids=lambda c: c.name)
def test_act9_on_the_eight_phase_core(case):
    assert len(GELU2) >= 2 and any(c.companion for c in GELU2)
    if case.cus256 and _cus() != 256:
        pytest.skip("the walk regime of this case is the one 256 CUs give")
    M, N, K = case.M, case.N, case.K
    x, w, xv, wv, ep = gr.make(case, M, DEV, seed=7)
    geo = gr.geo_of(case, M)
    xb, wb = _input(x, K), _input(w, K)
    if case.everywhere:
        hip.gemm8p_config(True, 1, 128)
    try:
        assert hip.linear_gelu_fused_ok(hip.BF16, M, K, N)
        runs = []
        for _ in range(2):
            n0 = {k: hip.kernel_launches(k) for k in ("gemm8p", "gemm8p_ragged")}
            ybuf, y = _output(M, N, N)
            y2buf, y2 = _output(M, N, N)
            hip.linear_gelu(hip.BF16, 9, xb, wb, ep.bias, None, y, y2, M, K, N)
            torch.cuda.synchronize()
            dn = {k: hip.kernel_launches(k) - n0[k] for k in n0}
            assert dn == dict(gemm8p=1, gemm8p_ragged=int(geo.ragged is not None)), dn
            runs.append((ybuf, y2buf))
        # act 4 (activation-agnostic) on the stored derivative: d_pre = (g W^T) * quickgelu'(pre), g = x and W = w of the case
        dbuf, dpre = _output(M, N, N)
        hip.linear_gelu(hip.BF16, 4, xb, wb, None, runs[0][1][G:], dpre, None, M, K, N)
        torch.cuda.synchronize()
    finally:
        if case.everywhere:
            hip.gemm8p_config(True, 192, 768)
    for a, b in zip(*runs):
        assert torch.equal(_bits(a), _bits(b)), f"{case.name}: outputs differ between two runs"
        assert _guards_intact(a, M, N, SENT), f"{case.name}: wrote outside its rows"            # rows past M untouched
    assert _guards_intact(dbuf, M, N, SENT)
    p = gr.product(xv, wv)
    ref, yard = qr.outputs(p, ep.bias, exact=True), qr.outputs(p, ep.bias, exact=False)
    got_y, got_y2 = runs[0][0][G:G + M].double(), runs[0][1][G:G + M].double()
    assert torch.isfinite(got_y).all() and torch.isfinite(got_y2).all()
    qr.hold(case.name, "y", got_y, ref["y"], yard["y"], geo)
    qr.hold(case.name, "y2", got_y2, ref["y2"], yard["y2"], geo)
    # the exact-erf epilogue (act 5) would not have passed: this is not the GELU kernel under another number
    erf = qr.outputs(p, ep.bias, exact=False, mutant="erf_gelu")
    assert gr.ratio(erf["y"], ref["y"], yard["y"], "y", geo)[0] > 1.0
    geo4 = gr.Geo(ragged=geo.ragged)
    ref4 = gr.outputs(p, gr.Epi(aux=ref["y2"]), exact=True)["y"]
    yard4 = gr.outputs(p, gr.Epi(aux=yard["y2"]), exact=False)["y"]
    qr.hold(case.name + " act4", "y", dpre[:M].double(), ref4, yard4, geo4)
