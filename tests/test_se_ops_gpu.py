"""Channel attention of the SE / ECA closing stage (csrc/se.hip through hip.se_forward / hip.se_backward: pool, gate, apply forward; reduce,
gate, apply backward; fp32 and bf16) against float64 on the CPU.

The truth is the closed form of the operator and its gradient (checked below against float64 autograd of the twin's modules behind a
training-mode BatchNorm).  c is the raw conv output [N][HW][C], (scale, shift, mean, invstd) its BatchNorm vectors, r the shortcut:
    cm = mean_p c    z = scale cm + shift    SE: h = relu(W1 z + b1), s = sigmoid(W2 h + b2)    ECA: s = sigmoid(conv1d_k(z)), zero padded
    out = relu((c scale + shift) s[b] + r)
    gm = g [out > 0]   A = sum_p gm   B = sum_p gm c   ds = (scale B + shift A) s (1 - s)
    SE:  dW2 = ds^T h, db2 = sum_b ds, dh = (ds W2) [h > 0], dW1 = dh^T z, db1 = sum_b dh, dz = dh W1
    ECA: dw[j] = sum_{b,ch} ds[b][ch] z[b][ch + j - pad],  dz[b][ch] = sum_j w[j] ds[b][ch - j + pad]
    S1 = sum_b (s A + dz)   S2 = sum_b (s (B - mean A) + dz (cm - mean))   dgamma = invstd S2   dbeta = S1
    dc = scale (gm s[b] + dz[b] / HW - S1 / M - (c - mean) invstd^2 S2 / M),  M = N HW

The bounds are derived, not tuned: a first-order running error analysis of exactly this chain.  u = 2^-24, gamma_k = k u / (1 - k u);
every quantity q carries (|q|_, e_q): the same formula on absolute values, and an error bound built from the error bounds of its inputs
(times the absolute derivative: <= 1/4 for the sigmoid, <= 1 for s (1 - s)) plus gamma_k |q|_ with k = the number of terms of its own
sum plus its scalar roundings (8 for the sigmoid: expf, the add, the division and slack for expf's own error).  Second-order products of
two error terms are below 2^-20 of the bound; the factor 1.01 covers them.  bf16 adds 2^-8 |ref| for each rounding of a stored output
(out, dc; the on-the-fly normalised projection shortcut is rounded as nkb_bn_apply rounds it: one more 2^-8 |r|).  The two masks of the
backward pass ([out > 0], [h > 0]) are the engine's own from its forward pass, which is checked first (a bit may differ from the
reference's only where |out| is inside its bound).  The test prints, next to the engine's worst error / bound ratio, the same ratio for
torch's own fp32 CPU evaluation of the closed form on the same data."""
import sys
from pathlib import Path

import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, str(Path(__file__).resolve().parent))

from seresnet_reference import EcaModule, SEModule, eca_k, se_rd  # noqa: E402
from nkb_classification import hip  # noqa: E402

DEV = "cuda:0"
U = 2.0 ** -24
# (C, HW, N, kind): layer1 of a BasicBlock member at full size; a 17 x 18 map with an odd row count; the widest stage; HW = 1; more images
# than gate workgroups can hold at once (SE_IPG images each) and more (image, channel group) work items than the reduce grid
CASES = [(64, 3136, 2, "se"), (256, 306, 3, "se"), (256, 306, 3, "eca"), (2048, 49, 3, "se"), (2048, 49, 3, "eca"), (2048, 1, 2, "se"),
         (2048, 1, 2, "eca"), (512, 4, 200, "se")]
IDS = [f"C{c}_HW{h}_N{n}_{k}" for c, h, n, k in CASES]
DTYPES = [torch.float32, torch.bfloat16]


def _gamma(k):
    return k * U / (1 - k * U)


def _data(C, HW, N, kind, dtype, proj=False, seed=0):
    g = torch.Generator().manual_seed(seed + C + 7 * HW + N)
    d = dict(kind=kind, C=C, HW=HW, N=N)
    d["c"] = (torch.randn(N, HW, C, generator=g) * 1.5 + 0.3).to(dtype)
    d["g"] = torch.randn(N, HW, C, generator=g).to(dtype)
    r = torch.randn(N, HW, C, generator=g)
    r[0] = -100.0                                              # image 0: every output is clipped, its g is all masked
    d["r"] = r.to(dtype)
    c64 = d["c"].double().reshape(-1, C)
    mean, var = c64.mean(0), c64.var(0, unbiased=False)
    invstd = (var + 1e-5).rsqrt()
    gamma = torch.rand(C, generator=g).double() + 0.5
    gamma[3] = 0.0                                             # one channel with gamma = 0: y = beta there, the gate gets no gradient through B
    beta = torch.randn(C, generator=g).double() * 0.3
    scale = gamma * invstd
    d["bn"] = torch.stack([scale, beta - mean * scale, mean, invstd]).float().contiguous()
    d["gamma"] = gamma
    if proj:                                                   # the shortcut is a raw projection output with its own scale / shift
        d["rbn"] = torch.stack([torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.2]).float().contiguous()
    if kind == "se":
        rd = se_rd(C)
        d["w1"] = torch.randn(rd, C, generator=g) / C ** 0.5
        d["b1"] = torch.randn(rd, generator=g) * 0.1 + 0.1
        d["w2"] = torch.randn(C, rd, generator=g) / rd ** 0.5
        d["b2"] = torch.randn(C, generator=g) * 0.1
    else:
        d["w1"] = torch.randn(eca_k(C), generator=g) * 0.5
    return d


def _conv_taps(w, v, transpose=False):
    """sum_j w[j] v[..., ch + j - pad] (transpose: ch - j + pad), zero padded, written out tap by tap."""
    k, C = w.numel(), v.shape[-1]
    pad = (k - 1) // 2
    out = torch.zeros_like(v)
    for j in range(k):
        o = (pad - j) if transpose else (j - pad)
        lo, hi = max(0, -o), min(C, C - o)
        out[..., lo:hi] += w[j] * v[..., lo + o:hi + o]
    return out


def _forward(d, dt=torch.float64, eval_form=False):
    """(values, magnitudes-and-errors) of the forward chain in dtype dt."""
    C, HW = d["C"], d["HW"]
    c, r = d["c"].to(dt), d["r"].to(dt)
    if eval_form:
        scale, shift = torch.ones(C, dtype=dt), torch.zeros(C, dtype=dt)
    else:
        scale, shift = d["bn"][0].to(dt), d["bn"][1].to(dt)
    v, e = {}, {}
    v["cm"] = c.mean(1)
    e["cm_"] = c.abs().mean(1)
    e["cm"] = _gamma(HW + 2) * e["cm_"]                       # the sum, the rounded 1 / HW and the product
    v["z"] = scale * v["cm"] + shift
    e["z_"] = scale.abs() * e["cm_"] + shift.abs()
    e["z"] = scale.abs() * e["cm"] + _gamma(2) * e["z_"]
    if d["kind"] == "se":
        w1, b1, w2, b2 = (d[k].to(dt) for k in ("w1", "b1", "w2", "b2"))
        rd = w1.shape[0]
        v["h"] = torch.relu(v["z"] @ w1.T + b1)
        e["h"] = e["z"] @ w1.abs().T + _gamma(C + 1) * (e["z_"] @ w1.abs().T + b1.abs())
        pre = v["h"] @ w2.T + b2
        e_pre = e["h"] @ w2.abs().T + _gamma(rd + 1) * (v["h"] @ w2.abs().T + b2.abs())
    else:
        w = d["w1"].to(dt)
        pre = _conv_taps(w, v["z"])
        e_pre = _conv_taps(w.abs(), e["z"]) + _gamma(w.numel()) * _conv_taps(w.abs(), e["z_"])
    v["s"] = torch.sigmoid(pre)
    e["s"] = 0.25 * e_pre + _gamma(8) * v["s"]
    if "rbn" in d:
        rr = r * d["rbn"][0].to(dt) + d["rbn"][1].to(dt)
        e_r = _gamma(2) * (r.abs() * d["rbn"][0].to(dt) + d["rbn"][1].to(dt).abs()) + (2.0 ** -8 * rr.abs() if d["c"].dtype == torch.bfloat16 else 0.0)
    else:
        rr, e_r = r, 0.0
    s_ = v["s"][:, None, :]
    pre_out = (c * scale + shift) * s_ + rr
    mag = (c.abs() * scale.abs() + shift.abs())
    v["out"] = torch.relu(pre_out)
    e["out"] = mag * e["s"][:, None, :] + _gamma(6) * (mag * s_ + rr.abs()) + e_r
    v["pre_out"] = pre_out
    return v, e


def _backward(d, fv, fe, mask, hmask, dt=torch.float64):
    C, HW, N = d["C"], d["HW"], d["N"]
    M = N * HW
    c, g = d["c"].to(dt), d["g"].to(dt)
    scale, shift, mean, invstd = (d["bn"][i].to(dt) for i in range(4))
    v, e = {}, {}
    fe = {k: t.to(dt) for k, t in fe.items()}                 # (a float32 evaluation only wants the values; its bounds are not used)
    gm = g * mask.to(dt)
    A, B = gm.sum(1), (gm * c).sum(1)
    A_, B_ = gm.abs().sum(1), (gm.abs() * c.abs()).sum(1)
    eA, eB = _gamma(HW) * A_, _gamma(HW + 1) * B_
    s, es = fv["s"], fe["s"]
    q = scale * B + shift * A
    q_ = scale.abs() * B_ + shift.abs() * A_
    eq = scale.abs() * eB + shift.abs() * eA + _gamma(3) * q_
    sp = s * (1 - s)
    esp = es + _gamma(3) * sp
    ds = q * sp
    ds_ = q_ * sp
    eds = eq * sp + q_ * esp + _gamma(2) * ds_
    z, z_, ez = fv["z"], fe["z_"], fe["z"]
    if d["kind"] == "se":
        w1, w2 = d["w1"].to(dt), d["w2"].to(dt)
        rd = w1.shape[0]
        h, eh = fv["h"], fe["h"]
        hm = hmask.to(dt)
        dh = (ds @ w2) * hm
        dh_ = (ds_ @ w2.abs()) * hm
        edh = (eds @ w2.abs() + _gamma(C) * (ds_ @ w2.abs())) * hm
        dz = dh @ w1
        dz_ = dh_ @ w1.abs()
        edz = edh @ w1.abs() + _gamma(rd) * dz_
        v["dw2"] = ds.T @ h
        e["dw2"] = eds.T @ h + ds_.T @ eh + _gamma(N + 1) * (ds_.T @ h)
        v["db2"] = ds.sum(0)
        e["db2"] = eds.sum(0) + _gamma(N) * ds_.sum(0)
        v["dw1"] = dh.T @ z
        e["dw1"] = edh.T @ z_ + dh_.T @ ez + _gamma(N + 1) * (dh_.T @ z_)
        v["db1"] = dh.sum(0)
        e["db1"] = edh.sum(0) + _gamma(N) * dh_.sum(0)
    else:
        w = d["w1"].to(dt)
        k = w.numel()
        pad = (k - 1) // 2
        dz = _conv_taps(w, ds, transpose=True)
        dz_ = _conv_taps(w.abs(), ds_, transpose=True)
        edz = _conv_taps(w.abs(), eds, transpose=True) + _gamma(k) * dz_
        dw, edw = torch.zeros(k, dtype=dt), torch.zeros(k, dtype=dt)
        for j in range(k):
            o = j - pad
            lo, hi = max(0, -o), min(C, C - o)
            dw[j] = (ds[:, lo:hi] * z[:, lo + o:hi + o]).sum()
            edw[j] = ((eds[:, lo:hi] * z_[:, lo + o:hi + o]).sum() + (ds_[:, lo:hi] * ez[:, lo + o:hi + o]).sum()
                      + _gamma(N * C + 2) * (ds_[:, lo:hi] * z_[:, lo + o:hi + o]).sum())
        v["dw1"], e["dw1"] = dw, edw
    cm, cm_, ecm = fv["cm"], fe["cm_"], fe["cm"]
    S1 = (s * A + dz).sum(0)
    S1_ = (s * A_ + dz_).sum(0)
    eS1 = (es * A_ + s * eA + edz).sum(0) + _gamma(N + 2) * S1_
    S2 = (s * (B - mean * A) + dz * (cm - mean)).sum(0)
    S2_ = (s * (B_ + mean.abs() * A_) + dz_ * (cm_ + mean.abs())).sum(0)
    eS2 = (es * (B_ + mean.abs() * A_) + s * (eB + mean.abs() * eA) + edz * (cm_ + mean.abs()) + dz_ * ecm).sum(0) + _gamma(N + 4) * S2_
    v["dgamma"], e["dgamma"] = invstd * S2, invstd * eS2 + _gamma(1) * invstd * S2_
    v["dbeta"], e["dbeta"] = S1, eS1
    v["dz"], e["dz"] = dz, edz
    i2 = invstd * invstd
    cc = c - mean
    v["dc"] = scale * (gm * s[:, None, :] + dz[:, None, :] / HW - S1 / M - cc * (i2 * S2 / M))
    cmag = c.abs() + mean.abs()
    e["dc"] = scale.abs() * (gm.abs() * es[:, None, :] + edz[:, None, :] / HW + eS1 / M + cmag * (i2 * eS2 / M)) + _gamma(16) * scale.abs() * (
        gm.abs() * s[:, None, :] + dz_[:, None, :] / HW + S1_ / M + cmag * (i2 * S2_ / M))
    return v, e


def test_closed_form_equals_autograd_of_the_twin():
    """The closed form with the TRUE batch statistics against float64 autograd of BatchNorm2d (train) -> SEModule / EcaModule -> + r -> ReLU."""
    for kind in ("se", "eca"):
        C, HW, N = 128, 30, 3
        d = _data(C, HW, N, kind, torch.float32, seed=9)
        d["r"][0] = torch.randn(HW, C, generator=torch.Generator().manual_seed(1))          # keep image 0 alive here
        c64 = d["c"].double().reshape(-1, C)
        mean, var = c64.mean(0), c64.var(0, unbiased=False)
        invstd = (var + 1e-5).rsqrt()
        gamma, beta = d["gamma"], torch.linspace(-0.3, 0.4, C, dtype=torch.float64)
        scale = gamma * invstd
        d["bn"] = torch.stack([scale, beta - mean * scale, mean, invstd])                    # float64: the exact statistics
        bn = torch.nn.BatchNorm2d(C, eps=1e-5).double().train()
        mod = (SEModule(C) if kind == "se" else EcaModule(C)).double()
        with torch.no_grad():
            bn.weight.copy_(gamma); bn.bias.copy_(beta)
            if kind == "se":
                mod.fc1.weight.copy_(d["w1"].double().view(-1, C, 1, 1)); mod.fc1.bias.copy_(d["b1"].double())
                mod.fc2.weight.copy_(d["w2"].double().view(C, -1, 1, 1)); mod.fc2.bias.copy_(d["b2"].double())
            else:
                mod.conv.weight.copy_(d["w1"].double().view(1, 1, -1))
        x = d["c"].double().view(N, 5, 6, C).permute(0, 3, 1, 2).clone().requires_grad_(True)
        rr = d["r"].double().view(N, 5, 6, C).permute(0, 3, 1, 2)
        out = torch.relu(mod(bn(x)) + rr)
        params = [bn.weight, bn.bias] + list(mod.parameters())
        grads = torch.autograd.grad(out, [x] + params, d["g"].double().view(N, 5, 6, C).permute(0, 3, 1, 2))
        fv, fe = _forward(d)
        bv, _ = _backward(d, fv, fe, fv["out"] > 0, fv["h"] > 0 if kind == "se" else None)
        nhwc = lambda t: t.permute(0, 2, 3, 1).reshape(N, HW, C)     # noqa: E731
        pairs = [(fv["out"], nhwc(out.detach())), (bv["dc"], nhwc(grads[0])), (bv["dgamma"], grads[1]), (bv["dbeta"], grads[2])]
        if kind == "se":
            pairs += [(bv["dw1"], grads[3].view(-1, C)), (bv["db1"], grads[4]), (bv["dw2"], grads[5].view(C, -1)), (bv["db2"], grads[6])]
        else:
            pairs += [(bv["dw1"], grads[3].view(-1))]
        for i, (mine, ref) in enumerate(pairs):
            assert torch.isfinite(ref).all() and (mine - ref).abs().max().item() <= 1e-12 * max(1.0, ref.abs().max().item()), (kind, i)
        assert bool((bv["dgamma"][3].abs() > 0)) and bool((grads[0][:, 3] == 0).all())     # gamma = 0: no data gradient, a weight gradient


def _unpack_bits(bits, N, HW, C, epc):
    b = bits.cpu().view(N, HW, C // epc, 1)
    return ((b >> torch.arange(epc, dtype=torch.uint8).view(1, 1, 1, epc)) & 1).bool().view(N, HW, C)


def _run_forward(d, dtype, eval_form=False):
    C, HW, N = d["C"], d["HW"], d["N"]
    se = d["kind"] == "se"
    rd = d["w1"].shape[0] if se else 0
    dev = {k: v.to(DEV) for k, v in d.items() if isinstance(v, torch.Tensor)}
    work = torch.full((hip.se_workspace(N, C, rd),), 7.0, device=DEV)
    out = torch.full_like(dev["c"], 7.0)
    epc = 8 if dtype == torch.bfloat16 else 4
    bits = None if eval_form else torch.full((N * HW, C // epc), 0xAA, dtype=torch.uint8, device=DEV)
    hip.se_forward(hip.dt(dtype), dev["c"], dev["r"], out, None if eval_form else dev["bn"], work, N, HW, C, dev["w1"], dev.get("b1"),
                   dev.get("w2"), dev.get("b2"), bits=bits, res_bnvec=dev.get("rbn"))
    torch.cuda.synchronize()
    nc = N * C
    got = dict(out=out.cpu(), cm=work[:nc].view(N, C).cpu(), s=work[nc:2 * nc].view(N, C).cpu())
    if se:
        h0 = 6 * nc + 2 * C + C // 4                              # the workspace layout of include/nkbhip.h
        got["h"] = work[h0:h0 + N * rd].view(N, rd).cpu()
    return got, dev, work, bits


def _compare(tag, names, got, ref, err, t32, dtype, stored=()):
    tiny, line, worst = 1e-300, [], {}
    for name in names:
        bound = 1.01 * err[name] + (2.0 ** -8 * ref[name].abs() if dtype == torch.bfloat16 and name in stored else 0.0)
        assert got[name].shape == ref[name].shape, name
        assert bool(torch.isfinite(got[name]).all()), name
        diff = (got[name].double() - ref[name]).abs()
        r32 = t32[name].to(dtype) if name in stored else t32[name]
        ratio, ratio32 = (diff / (bound + tiny)).max().item(), ((r32.double() - ref[name]).abs() / (bound + tiny)).max().item()
        line.append(f"{name} {ratio:.3f} (torch fp32 cpu {ratio32:.3f})")
        worst[name] = (ratio, int((diff > bound).sum()))
    print(f"\n[{tag}] worst |err| / bound: " + "  ".join(line))
    for name, (ratio, bad) in worst.items():
        assert bad == 0, (tag, name, bad, ratio)


def _check(case, dtype, proj=False):
    C, HW, N, kind = case
    d = _data(C, HW, N, kind, dtype, proj=proj)
    tag = f"se_ops C={C} HW={HW} N={N} {kind} {str(dtype)[6:]}{' proj' if proj else ''}"
    fv, fe = _forward(d)
    f32, _ = _forward(d, torch.float32)
    got, dev, work, bits = _run_forward(d, dtype)
    names = ["cm", "s", "out"] + (["h"] if kind == "se" else [])
    _compare(tag + " fwd", names, got, fv, fe, f32, dtype, stored=("out",))
    epc = 8 if dtype == torch.bfloat16 else 4
    mask = _unpack_bits(bits, N, HW, C, epc)
    assert bool((mask == (got["out"] > 0)).all())                                 # bit e = stored out > 0
    slack = 1.01 * fe["out"] + (2.0 ** -8 * fv["out"].abs() if dtype == torch.bfloat16 else 0.0)
    assert not bool(((mask != (fv["pre_out"] > 0)) & (fv["pre_out"].abs() > slack)).any())
    assert not bool(mask[0].any())                                                # image 0: all masked
    if kind == "eca":                                                             # the taps at the two channel edges: zero padding, not wrap-around
        pad = (d["w1"].numel() - 1) // 2
        for ch in list(range(pad + 1)) + list(range(C - pad - 1, C)):
            assert bool(((got["s"][:, ch].double() - fv["s"][:, ch]).abs() <= 1.01 * fe["s"][:, ch]).all()), ch
        wrap = torch.sigmoid(sum(d["w1"][j].double() * torch.roll(fv["z"], pad - j, -1) for j in range(d["w1"].numel())))
        assert bool(((wrap[:, 0] - fv["s"][:, 0]).abs() > 10 * fe["s"][:, 0]).any())          # (the circular form is far outside the bound)
    hmask = got["h"] > 0 if kind == "se" else None
    bv, be = _backward(d, fv, fe, mask, hmask)
    b32, _ = _backward(d, f32, fe, mask, hmask, torch.float32)
    pnames = ["dw1", "db1", "dw2", "db2"] if kind == "se" else ["dw1"]
    g = torch.Generator().manual_seed(4)
    init = {k: torch.randn(bv[k].shape, generator=g) for k in pnames + ["dgamma", "dbeta"]}
    runs = []
    for _ in range(2):
        acc = {k: v.clone().to(DEV) for k, v in init.items()}
        dc = torch.full_like(dev["c"], 7.0)
        hip.se_backward(hip.dt(dtype), dev["g"], dev["c"], bits, dc, dev["bn"], work, N, HW, C, dev["w1"], dev.get("w2"), dw1=acc["dw1"],
                        db1=acc.get("db1"), dw2=acc.get("dw2"), db2=acc.get("db2"), dgamma=acc["dgamma"], dbeta=acc["dbeta"])
        torch.cuda.synchronize()
        nc = N * C
        runs.append(dict(dc=dc.cpu(), dz=work[4 * nc:5 * nc].view(N, C).cpu(), **{k: v.cpu() for k, v in acc.items()}))
    for k in runs[0]:
        assert torch.equal(runs[0][k], runs[1][k]), f"{k}: two launches differ"
    gotb = dict(runs[0])
    for k in init:                                          # "+=" onto a non-zero start: one more rounding of the sum
        bv[k] = bv[k] + init[k].double()
        b32[k] = b32[k] + init[k]
        be[k] = be[k] + U * bv[k].abs()
        assert not torch.equal(gotb[k], init[k]), k
    _compare(tag + " bwd", ["dz", "dc"] + list(init), gotb, bv, be, b32, dtype, stored=("dc",))
    assert bool((gotb["dc"][:, :, 3] == 0).all())           # gamma = 0: scale = 0, no gradient reaches c there


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_se_chain_against_float64(case, dtype):
    _check(case, dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("kind", ["se", "eca"])
def test_se_chain_with_a_raw_projection_shortcut(kind, dtype):
    """r = rnd(res * rscale + rshift) formed on the fly, as nkb_bn_apply does for a block's first unit."""
    _check((256, 306, 3, kind), dtype, proj=True)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("kind", ["se", "eca"])
def test_eval_form_without_bn_vectors(kind, dtype):
    """Eval: c is the normalised map of the folded convolution; identity affine, no bits, nothing else changes."""
    C, HW, N = 256, 306, 3
    d = _data(C, HW, N, kind, dtype)
    fv, fe = _forward(d, eval_form=True)
    f32, _ = _forward(d, torch.float32, eval_form=True)
    got, _, _, bits = _run_forward(d, dtype, eval_form=True)
    assert bits is None
    _compare(f"se_ops eval C={C} HW={HW} N={N} {kind} {str(dtype)[6:]}", ["cm", "s", "out"], got, fv, fe, f32, dtype, stored=("out",))
