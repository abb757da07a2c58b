"""The fused stem tail (bn1 -> ReLU -> 3x3/2 max-pool, `nkb_bn_relu_maxpool_sel`) on tiny tensors, through the C ABI.

Forward: y, idx and xsel are bit-identical with the library's own unfused path (`nkb_bn_apply` with ReLU, then `nkb_maxpool`; xsel is c
at the returned slots) — the definition the fused kernel's comments give, so no tolerance.  Backward apply: dc against a float64
evaluation of dc = k1*g'' + k2*c + k3 from the same stored inputs and the sums the library's reduction produced, within one storage
rounding of the result plus the fp32 evaluation error of a three-term sum that may cancel: 2^-8 (fp32: 2^-23) * |ref| +
2^-20 * (|k1*g''| + |k2*c| + |k3|).  g'' and k1, k2, k3 enter that sum as the kernel forms them (see the test).  Two calls give
identical bytes.

The shapes cover odd and even extents, windows that are all edge, pooled heights the forward kernel's row band does not divide (and
more than one band), one chunk per pixel, a chunk count that is no power of two and more than one workgroup; the inputs cover ties,
all-zero windows, four-term gradient sums and NaNs at the first, middle and last tap of a window.
"""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from nkb_classification import hip  # noqa: E402

DEV = "cuda"
BF, F32 = torch.bfloat16, torch.float32
SHAPES = [
    (1, 1, 1, 8, BF), (1, 2, 3, 8, BF), (3, 7, 7, 64, BF), (2, 5, 9, 16, BF), (1, 16, 16, 72, BF), (2, 12, 10, 64, BF),
    (2, 7, 9, 4, F32), (1, 6, 6, 12, F32),
    (1, 33, 6, 8, BF),        # 17 pooled rows: three bands of the forward kernel, the last one short
    (4, 20, 20, 64, BF),      # several workgroups in both kernels
]
KINDS = ["random", "ties", "negative", "fourmax", "nan_first", "nan_middle", "nan_last", "nan_two"]
CASES = [(s, k) for s in SHAPES for k in KINDS]
IDS = [f"{n}x{h}x{w}x{c}-{'bf16' if dt == BF else 'f32'}-{k}" for (n, h, w, c, dt), k in CASES]


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF else torch.int32)


def window_taps(p, q, H, W):
    """(slot, h, w) of the taps of pooled position (p, q) that lie inside the image, in row-major order"""
    return [(3 * r + s, 2 * p - 1 + r, 2 * q - 1 + s) for r in range(3) for s in range(3)
            if 0 <= 2 * p - 1 + r < H and 0 <= 2 * q - 1 + s < W]


@functools.lru_cache(maxsize=None)
def run(shape, kind):
    """inputs, the unfused reference and two fused forward + backward calls for one case; computed once, read by every test"""
    N, H, W, C, dtype = shape
    d = hip.dt(dtype)
    P, Q = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    rows = N * H * W
    gen = torch.Generator().manual_seed(1000 * SHAPES.index(shape) + KINDS.index(kind))
    c = torch.randn(N, H, W, C, generator=gen)
    gamma = torch.rand(C, generator=gen) + 0.5
    beta = torch.full((C,), 0.1)
    if kind == "ties":
        c = (c * 2).round() / 4                            # multiples of 0.25 in a narrow range: most windows hold ties
    if kind == "fourmax":
        c[:, 1::4, 1::4, :] = 8.0 + torch.rand(c[:, 1::4, 1::4, :].shape, generator=gen)
    c = c.to(dtype)
    cf = c.float().reshape(rows, C)
    mean = cf.mean(0)
    invstd = (cf.var(0, unbiased=False) + 1e-5).rsqrt()
    if kind == "negative":
        beta = torch.full((C,), -40.0)                     # every c*scale + shift is negative: every window is an all-zero tie
    scale = (gamma * invstd).contiguous()
    shift = (beta - mean * scale).contiguous()
    if kind.startswith("nan"):
        p, q = min(1, P - 1), min(1, Q - 1)
        taps = window_taps(p, q, H, W)
        pick = dict(nan_first=[taps[0]], nan_middle=[taps[len(taps) // 2]], nan_last=[taps[-1]], nan_two=[taps[0], taps[-1]])[kind]
        for _, h, w in pick:
            c[:, h, w, :] = float("nan")
    g = torch.randn(N, P, Q, C, generator=gen).to(dtype)
    c, g, gamma, mean, invstd, scale, shift = (t.to(DEV) for t in (c, g, gamma, mean, invstd, scale, shift))
    # the unfused path
    a = torch.empty_like(c)
    hip.bn_apply(d, c, None, a, scale, shift, rows, C, True)
    y0 = torch.empty(N, P, Q, C, device=DEV, dtype=dtype)
    i0 = torch.empty(N, P, Q, C, device=DEV, dtype=torch.uint8)
    hip.maxpool(d, False, a, y0, i0, N, H, W, C)
    outs = []
    for _ in range(2):
        y = torch.full_like(y0, 3.0)
        idx = torch.full_like(i0, 77)
        xs = torch.full_like(y0, 5.0)
        hip.bn_relu_maxpool(d, False, c, scale, shift, mean, invstd, None, y, idx, None, None, None, None, N, H, W, C, xsel=xs)
        dg, db = torch.zeros(C, device=DEV), torch.zeros(C, device=DEV)
        dc = torch.full_like(c, 9.0)
        work = torch.empty(hip.bn_relu_maxpool_ws(N, H, W, C), device=DEV)
        hip.bn_relu_maxpool(d, True, c, scale, shift, mean, invstd, gamma, g, idx, dc, dg, db, work, N, H, W, C, xsel=xs)
        outs.append(dict(y=y, idx=idx, xsel=xs, dc=dc, dg=dg, db=db))
    torch.cuda.synchronize()
    cpu = lambda t: t.cpu()
    return dict(N=N, H=H, W=W, C=C, P=P, Q=Q, dtype=dtype, c=cpu(c), g=cpu(g), gamma=cpu(gamma), mean=cpu(mean), invstd=cpu(invstd),
                scale=cpu(scale), shift=cpu(shift), y0=cpu(y0), i0=cpu(i0), outs=[{k: cpu(v) for k, v in o.items()} for o in outs])


def slot_coords(idx, P, Q):
    """input row / column behind every pooled element's slot"""
    pp, qq = torch.meshgrid(torch.arange(P), torch.arange(Q), indexing="ij")
    hh = (2 * pp - 1)[None, :, :, None] + idx.long() // 3
    ww = (2 * qq - 1)[None, :, :, None] + idx.long() % 3
    return hh, ww


@pytest.mark.parametrize("shape,kind", CASES, ids=IDS)
def test_forward_is_bit_identical_with_bn_apply_then_maxpool(shape, kind):
    r = run(shape, kind)
    N, H, W, C, P, Q = (r[k] for k in "NHWCPQ")
    o = r["outs"][0]
    assert int(r["i0"].max()) <= 8
    hh, ww = slot_coords(r["i0"], P, Q)
    assert bool(((hh >= 0) & (hh < H) & (ww >= 0) & (ww < W)).all()), "the reference names a tap outside the image"
    nn = torch.arange(N)[:, None, None, None].expand_as(hh)
    cc = torch.arange(C)[None, None, None, :].expand_as(hh)
    xsel0 = r["c"][nn, hh, ww, cc]
    assert torch.equal(o["idx"], r["i0"])
    assert torch.equal(bits(o["y"]), bits(r["y0"]))
    assert torch.equal(bits(o["xsel"]), bits(xsel0))
    if kind == "negative":      # all-zero ties: the first valid tap wins
        first = torch.tensor([[window_taps(p, q, H, W)[0][0] for q in range(Q)] for p in range(P)], dtype=torch.uint8)
        assert torch.equal(o["idx"], first[None, :, :, None].expand_as(o["idx"]))
        assert not bool(o["y"].float().any())
    if kind == "ties" and H * W >= 25:
        a = torch.relu((r["c"].float() * r["scale"] + r["shift"]).to(r["dtype"]).float())
        tied = sum(int(((a[:, h, w, :] == o["y"][:, p, q, :].float()).sum()))
                   for p in range(P) for q in range(Q) for _, h, w in window_taps(p, q, H, W)) - o["y"].numel()
        assert tied > o["y"].numel() // 4, "the input set holds too few ties to test their order"


@pytest.mark.parametrize("shape,kind", CASES, ids=IDS)
def test_backward_apply_against_float64(shape, kind):
    r = run(shape, kind)
    N, H, W, C, P, Q, dtype = (r[k] for k in ("N", "H", "W", "C", "P", "Q", "dtype"))
    o = r["outs"][0]
    c64, g64 = r["c"].double(), r["g"].double()
    # g'' in float64: every pooled gradient goes to the pixel its window's slot names
    hh, ww = slot_coords(o["idx"], P, Q)
    nn = torch.arange(N)[:, None, None, None].expand_as(hh)
    cc = torch.arange(C)[None, None, None, :].expand_as(hh)
    flat = ((nn * H + hh) * W + ww) * C + cc
    gpp64 = torch.zeros(N * H * W * C, dtype=torch.float64).index_add_(0, flat.reshape(-1), g64.reshape(-1)).reshape(N, H, W, C)
    cnt = torch.zeros(N * H * W * C).index_add_(0, flat.reshape(-1), torch.ones(flat.numel())).reshape(N, H, W, C)
    if kind == "fourmax" and H >= 4 and W >= 4:
        assert int(cnt[:, 1, 1, :].min()) == 4, "the input set has no four-term gradient sum"
    # g'' as the kernel forms it: an fp32 sum over the (at most) four windows that hold the pixel, in the candidate order
    # (p0,q0), (p0,q1), (p1,q0), (p1,q1), each counted where its slot names the pixel.  Up to four terms that may cancel: their fp32
    # rounding is relative to the terms, not to |k1*g''|, and like that of the constants below it is no part of the bound.
    h = torch.arange(H)[:, None].expand(H, W)
    w = torch.arange(W)[None, :].expand(H, W)
    p01, q01 = (h >> 1, (h + 1) >> 1), (w >> 1, (w + 1) >> 1)
    gf, idx = r["g"].float(), o["idx"].long()
    gpp = torch.zeros(N, H, W, C)
    for k in range(4):
        pk, qk = p01[k >> 1], q01[k & 1]
        ok = (pk < P) & (qk < Q)
        if k >> 1:
            ok = ok & (p01[1] != p01[0])
        if k & 1:
            ok = ok & (q01[1] != q01[0])
        pc, qc = pk.clamp(max=P - 1), qk.clamp(max=Q - 1)
        slot = (h - (2 * pk - 1)) * 3 + (w - (2 * qk - 1))
        hit = ok[None, :, :, None] & (idx[:, pc, qc, :] == slot[None, :, :, None])
        gpp = gpp + torch.where(hit, gf[:, pc, qc, :], torch.zeros(()))
    live = (r["c"].float() * r["scale"] + r["shift"]).to(dtype).float() > 0          # rnd_T(c*scale + shift) > 0, as the kernel
    gpp = torch.where(live, gpp, torch.zeros_like(gpp)).double()
    gpp64 = torch.where(live, gpp64, torch.zeros_like(gpp64))
    assert bool(((gpp - gpp64).abs() <= 2.0 ** -22 * torch.zeros(N * H * W * C, dtype=torch.float64).index_add_(
        0, flat.reshape(-1), g64.abs().reshape(-1)).reshape(N, H, W, C)).all()), "the two forms of g'' disagree"
    # The per-channel constants as the kernel forms them: fp32, from the library's own sums (dbeta / dgamma start at zero, so they
    # are the reduction's sums exactly), in the kernel's operation order.  k3 is itself a difference of two products that can cancel;
    # its fp32 rounding is relative to those products, not to |k3|, and is no part of the bound, which prices the three-term sum.
    # With g'' and the constants in float64 instead, the worst error / bound measured on MI355X was 1.047 (1x6x6x12 fp32, fourmax)
    # and below 1 in every other case; that figure is printed below as well.
    ga, is_, mu = r["gamma"], r["invstd"], r["mean"]
    inv_count = torch.tensor(1.0) / torch.tensor(float(N * H * W))
    a = ga * is_
    sdy, sdyx = o["db"] * inv_count, o["dg"] * inv_count
    k1, k2, k3 = a, (-a) * is_ * sdyx, (-a) * sdy + a * is_ * sdyx * mu
    a64 = ga.double() * is_.double()
    sdy64, sdyx64 = o["db"].double() / (N * H * W), o["dg"].double() / (N * H * W)
    k64 = (a64, -a64 * is_.double() * sdyx64, -a64 * sdy64 + a64 * is_.double() * sdyx64 * mu.double())
    rel = 2.0 ** -8 if dtype == BF else 2.0 ** -23
    got = o["dc"].double()

    def compare(k1, k2, k3, gpp):
        ref = k1 * gpp + k2 * c64 + k3
        bound = rel * ref.abs() + 2.0 ** -20 * ((k1 * gpp).abs() + (k2 * c64).abs() + k3.abs().expand_as(ref))
        nan = torch.isnan(ref)
        err = torch.where(nan, torch.zeros_like(ref), (got - ref).abs())
        bound = torch.where(nan, torch.zeros_like(ref), bound)
        ratio = torch.where(err > 0, err / bound.clamp_min(1e-300), torch.zeros_like(err)).max().item()
        return nan, err, bound, ratio

    nan, err, bound, worst = compare(k1.double(), k2.double(), k3.double(), gpp)
    print(f"dc: worst error / bound {worst:.3f} (g'' and the constants in float64: {compare(*k64, gpp64)[3]:.3f})")
    assert torch.equal(torch.isnan(got), nan)
    assert int(nan.sum()) == (0 if not kind.startswith("nan") else N * C * (2 if kind == "nan_two" and H * W > 1 else 1))
    assert bool((err <= bound).all()), worst


@pytest.mark.parametrize("shape,kind", CASES, ids=IDS)
def test_two_calls_give_identical_bytes(shape, kind):
    a, b = run(shape, kind)["outs"]
    for k in ("y", "xsel", "dc"):
        assert torch.equal(bits(a[k]), bits(b[k])), k
    assert torch.equal(a["idx"], b["idx"])
    assert torch.equal(a["dg"].view(torch.int32), b["dg"].view(torch.int32))
    assert torch.equal(a["db"].view(torch.int32), b["db"].view(torch.int32))
