"""Float64 reference of the ViT attention on the engine layout, the bf16 rounding yardstick, the error metric and bound that
tests/test_attention_gpu.py holds the HIP kernels to, and mutants that make the reference subtly wrong in the ways an attention
kernel goes wrong.  tests/test_attention_reference.py proves on the CPU that the bound rejects every mutant.  No test lives here.

Layout (hipnet.HipEngine.attention): qkv [B*T, 3*H*dh] laid out [which][head][dh]; o and dO [B*T, H*dh]; lse [B*H, T], the
natural-log log-sum-exp of the scaled scores of each query row (what csrc/attention.hip stores for the backward kernels).

The bound.  An output of a bf16 kernel cannot be closer to the float64 truth than the same math in float32 rounded to bf16 at
the points where the kernel rounds (the yardstick), and a correct kernel is not much further: it rounds the same fp32 values at
the same points, so its error is the yardstick's to within a few per cent.  A kernel output passes when its error is at most
max(C_BOUND * yardstick error, FLOOR).  C_BOUND is small because the errors that matter are small: counting one extra zero key
at T = 255 moves o by 0.24 %, about the size of the rounding error itself, and is caught only because the two add in quadrature
(sqrt(2) > C_BOUND).  FLOOR covers outputs the yardstick computes exactly while a kernel need not: at T = 1, o = v and
dq = dk = dS = 0, where the kernels' fp32 lse round trip leaves P = 1 - O(1e-7) and gradients of a few 1e-4 of RMS_FLOOR.
"""
import math

import torch

DH = 64
SCALE = DH ** -0.5            # 1/8, a power of two: dS and dS / scale round to bf16 identically

# the bound: max(C_BOUND * yardstick error, FLOOR).  The fused backward packs dS / scale, not dS, to bf16 (same rounding here).
C_BOUND = 1.15
FLOOR = 1e-3
# a slice whose reference is (near) zero is measured against this RMS instead of its own norm (dq = dk = dS = 0 at T = 1, dk = 0
# where Q = 0); for P and dS it is divided by T (a row of P sums to 1)
RMS_FLOOR = dict(o=1e-2, dq=1e-2, dk=1e-2, dv=1e-2, colsum=1e-2, P=1e-2, dS=1e-2)
LSE_RTOL = 1e-5               # |lse - ref| <= LSE_RTOL * (1 + |ref|): fp32 sums of exact bf16 products, no rounding to bf16
FP32_RTOL = 2e-5              # the fp32 (materialised, exact-fp32 MFMA) path: relative Frobenius error per slice

MUTANTS = ("pad_keys", "drop_last_key", "row_from_next_image", "swap_k_heads", "lse_extra_key")


def bf(x: torch.Tensor) -> torch.Tensor:
    """x rounded to bf16 (round to nearest even), kept in x's dtype."""
    return x.to(torch.bfloat16).to(x.dtype)


def split_qkv(qkv, B, T, H):
    """[B*T, 3*H*dh] -> q, k, v, each [B, H, T, dh]"""
    x = qkv.reshape(B, T, 3, H, -1).permute(2, 0, 3, 1, 4)
    return x[0], x[1], x[2]


def heads(x, B, T, H):
    """[B*T, H*dh] -> [B, H, T, dh]"""
    return x.reshape(B, T, H, -1).permute(0, 2, 1, 3)


def rows(x):
    """[B, H, T, dh] -> [B*T, H*dh]"""
    B, H, T, dh = x.shape
    return x.permute(0, 2, 1, 3).reshape(B * T, H * dh)


def join_qkv(dq, dk, dv):
    """three [B, H, T, dh] -> [B*T, 3*H*dh]"""
    return torch.cat([rows(dq), rows(dk), rows(dv)], 1)


def _fit_keys(x, T):
    """gradient rows of the keys a mutant attended to, back on the T keys of the image (extra keys dropped, a dropped key: 0)"""
    if x.shape[2] >= T:
        return x[:, :, :T]
    return torch.cat([x, x.new_zeros(*x.shape[:2], T - x.shape[2], x.shape[3])], 2)


def _attend(q, k, v, do, *, exact, delta_from="o", lse_fn=None):
    """One attention forward + backward over [B, H, T, dh] operands (keys may number other than T: the pad / drop mutants).
    exact: float64 math, no rounding (the reference).  Otherwise float32 rounded to bf16 where the kernels round:
      forward: P = softmax, normalised, to bf16 before P V; o to bf16; lse stays fp32.
      backward: P recomputed in fp32 from the stored lse; dS (= dS / scale * scale, scale a power of two) to bf16 before
        dQ = dS K and dK = dS^T Q, P to bf16 before dV = P^T dO; every stored gradient to bf16.  delta_from names where
        delta = rowsum(P o dP) comes from, per kernel:
          "o"  - rowsum(dO o O) with O the bf16 forward output (nkb_attn_backward, the fused backward)
          "p"  - rowsum(P o dP) of the fp32 P (nkb_attn_backward_ds)
          "pb" - rowsum(P o dP) and dS of the forward's bf16 P (the materialised path: nkb_attn_softmax's backward)"""
    r = (lambda x: x) if exact else bf
    Tk = k.shape[2]
    s = (q @ k.transpose(-2, -1)) * SCALE
    m = s.amax(-1, keepdim=True) if Tk else s.new_full((*s.shape[:-1], 1), -math.inf)
    e = torch.exp(s - m)
    z = e.sum(-1, keepdim=True)
    lse = (m + torch.log(z)).squeeze(-1)
    pn = r(e / z) if Tk else e
    o = r(pn @ v)
    if lse_fn is not None:
        lse = lse_fn(lse)
    p = torch.exp(s - lse[..., None])
    dp = do @ v.transpose(-2, -1)
    if exact or delta_from == "o":
        delta = (do * o).sum(-1, keepdim=True)
    elif delta_from == "p":
        delta = (p * dp).sum(-1, keepdim=True)
    else:
        p = pn
        delta = (p * dp).sum(-1, keepdim=True)
    ds = r(p * (dp - delta) * SCALE)
    pb = r(p)
    dq = r(ds @ k)
    dk = r(ds.transpose(-2, -1) @ q)
    dv = r(pb.transpose(-2, -1) @ do)
    return dict(o=o, lse=lse, P=pb, dS=ds, dq=dq, dk=dk, dv=dv)


def _finish(res, B, T, H):
    out = dict(o=rows(res["o"]), lse=res["lse"].reshape(B * H, T), P=res["P"], dS=res["dS"],
               dq=res["dq"], dk=_fit_keys(res["dk"], T), dv=_fit_keys(res["dv"], T))
    out["dqkv"] = join_qkv(out["dq"], out["dk"], out["dv"])
    out["colsum"] = out["dqkv"].sum(0)
    return out


def reference(qkv, do, B, T, H, mutant=None):
    """float64 truth for the given (already bf16-representable) inputs: o [B*T, D], lse [B*H, T], P and dS [B, H, T, T],
    dq / dk / dv [B, H, T, dh], dqkv [B*T, 3D] and its column sums.  With `mutant`: the exact effect of that mistake (None
    where it does not exist at this shape)."""
    q, k, v = split_qkv(qkv.double(), B, T, H)
    do = heads(do.double(), B, T, H)
    lse_fn = None
    if mutant is not None:
        m = _mutate(mutant, q, k, v, do, T)
        if m is None:
            return None
        q, k, v, do, lse_fn = m
    return _finish(_attend(q, k, v, do, exact=True, lse_fn=lse_fn), B, T, H)


def yardstick(qkv, do, B, T, H, delta_from="o", mutant=None):
    """The same math in float32, rounded to bf16 where the kernels round (see _attend); with `mutant`, what a kernel carrying
    that mistake would compute (None where the mutant does not exist at this shape)."""
    q, k, v = split_qkv(qkv.float(), B, T, H)
    do = heads(do.float(), B, T, H)
    lse_fn = None
    if mutant is not None:
        m = _mutate(mutant, q, k, v, do, T)
        if m is None:
            return None
        q, k, v, do, lse_fn = m
    return _finish(_attend(q, k, v, do, exact=False, delta_from=delta_from, lse_fn=lse_fn), B, T, H)


def pad_keys(T):
    """zero keys a kernel could wrongly count at this T: the padding of the last 16-key block, or where T % 16 == 0 and the
    block count is odd, the 16 rows of the skipped half of the last 32-key step; 0 where T is a multiple of 32"""
    return (-T) % 16 or (-T) % 32


def _mutate(name, q, k, v, do, T):
    """operands (and an lse map) of a kernel carrying the named mistake; None where the mistake cannot happen at this shape"""
    B, H = q.shape[:2]
    lse_fn = None
    if name == "pad_keys":                    # 1. the zero padding keys enter the softmax
        n = pad_keys(T)
        if n == 0:
            return None
        z = k.new_zeros(B, H, n, k.shape[3])
        k, v = torch.cat([k, z], 2), torch.cat([v, z], 2)
    elif name == "drop_last_key":             # 2. the last valid key is masked off
        k, v = k[:, :, :T - 1], v[:, :, :T - 1]
    elif name == "row_from_next_image":       # 3. the last query row of image 0 (its q, and in the backward its dO) read from image 1
        if B < 2:
            return None
        q, do = q.clone(), do.clone()
        q[0, :, T - 1] = q[1, :, T - 1]
        do[0, :, T - 1] = do[1, :, T - 1]
    elif name == "swap_k_heads":              # 4. K of heads 0 and 1 swapped
        if H < 2:
            return None
        k = k.clone()
        k[:, [0, 1]] = k[:, [1, 0]]
    elif name == "lse_extra_key":             # 5. the stored lse counts one extra zero key (o is right; the backward's P is not)
        lse_fn = lambda lse: torch.logaddexp(lse, torch.zeros_like(lse))
    else:
        raise ValueError(name)
    return q, k, v, do, lse_fn


# ---- the metric -------------------------------------------------------------------------------------------------------
def _slices(name, x, B, T, H):
    """an output as [slices, elements]: one slice per (image, head) (per image for the column sums)"""
    x = x.double()
    if name == "o":
        return heads(x, B, T, H).reshape(B * H, -1)
    if name in ("dq", "dk", "dv", "P", "dS"):
        return x.reshape(B * H, -1)
    if name == "colsum":
        return x.reshape(1, -1)
    raise ValueError(name)


def rel_err(name, x, ref, B, T, H) -> float:
    """max over (image, head) slices of ||x - ref||_F / max(||ref||_F, floor * sqrt(n)) (floor: RMS_FLOOR); inf if x is not
    finite"""
    xs, rs = _slices(name, x, B, T, H), _slices(name, ref, B, T, H)
    if not torch.isfinite(xs).all():
        return math.inf
    floor = RMS_FLOOR[name] / (T if name in ("P", "dS") else 1)
    den = rs.norm(dim=1).clamp_min(floor * math.sqrt(rs.shape[1]))
    return ((xs - rs).norm(dim=1) / den).max().item()


def bound(yard_err: float) -> float:
    return max(C_BOUND * yard_err, FLOOR)


def lse_err(x, ref) -> float:
    """max |lse - ref| / (1 + |ref|); passes at <= LSE_RTOL"""
    x, ref = x.double(), ref.double()
    if not torch.isfinite(x).all():
        return math.inf
    return ((x - ref).abs() / (1 + ref.abs())).max().item()


GRADS = ("dq", "dk", "dv")


def worst_ratio(out, ref, yard, B, T, H, names=("o",) + GRADS):
    """max over the named outputs of error / bound, and the lse error / LSE_RTOL: a kernel passes at <= 1"""
    ratios = {n: rel_err(n, out[n], ref[n], B, T, H) / bound(rel_err(n, yard[n], ref[n], B, T, H)) for n in names}
    ratios["lse"] = lse_err(out["lse"], ref["lse"]) / LSE_RTOL
    return ratios


# ---- inputs -----------------------------------------------------------------------------------------------------------
REGIMES = ("random", "uniform", "sharp")


def inputs(regime, B, T, H, seed=0):
    """bf16-representable fp32 qkv [B*T, 3D] and dO [B*T, D]: N(0, 1); Q = 0 (uniform scores); Q x 8 (near one-hot rows)"""
    g = torch.Generator().manual_seed(seed)
    D = H * DH
    qkv = bf(torch.randn(B * T, 3 * D, generator=g))
    do = bf(torch.randn(B * T, D, generator=g))
    if regime == "uniform":
        qkv[:, :D] = 0
    elif regime == "sharp":
        qkv[:, :D] *= 8
    elif regime != "random":
        raise ValueError(regime)
    return qkv, do


# key counts 1..16 (nkb = ceil(T / 16)), each aligned and, where it has room, ragged; the GPU sweep and the CPU proof share it
SWEEP = (1, 16, 17, 32, 33, 48, 63, 64, 80, 96, 97, 112, 127, 128, 144, 160, 176, 192, 197, 208, 224, 240, 255, 256)
SWEEP_BH = (2, 2)             # B * H = 4: all four wave rotations (blockIdx & 3) of the forward kernel; B, H >= 2 for mutants 3, 4
