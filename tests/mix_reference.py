"""Float64 reference, fp32 yardstick, bounds, mutants and case table of the mixed losses (nkb_loss_forward with NKB_LOSS_MIXED and
nkb_loss_backward with bit 1; contract and operation order in include/nkbhip.h), and the blend / box rule of nkb_image_prep's flag
bit 3 on arrays.  tests/test_mix_cpu.py proves on the CPU that the reference equals torch and that the checks reject every mutant;
tests/test_mix_loss_gpu.py and tests/test_image_mix_gpu.py hold the kernels to them.  No test lives here.

The mixed loss of a row with labels y, y2 and weight lam (the kernel rounds the float64 lam of the table to fp32; oml = 1 - lam):
  cross entropy  a_c = lam (1 - eps) w[y] [c = y] + oml (1 - eps) w[y2] [c = y2] + (eps / C) w_c,  loss_r = -sum_c a_c log p_c,
                 wsum_r = lam w[y] + oml w[y2], A = sum_c a_c;  'mean' divides by sum wsum_r;
  focal          loss_r = lam focal(y) + oml focal(y2) with the per-label formula of kind 1, wsum_r = 1;
  gradient       dlogits_rj = g (A_r p_j - c1_r [j = y] - c2_r [j = y2] - ew_j [sm_r]).
A row is dropped when either label equals ignore_index; either label outside [0, C) gives NaN.

The bounds (derived from U, A_EXP, A_LOG and A_POW of loss_optim_reference; nothing here is measured or tuned on a kernel's output):
  probs, lse     as loss_optim_reference: e_l(c) = e_lse + U |log p_c| for every column c;
  bit-exact      against the fp32 yardstick: argmax, sm, the pad words, ew (one division on the host, one product), for cross entropy
                 c1, c2 and wsum (products and one sum of fp32 inputs, in the documented order), and dlogits against the yardstick
                 evaluated on the forward outputs the SAME launch pair stored (probs, records, ew, out2[1]);
  CE loss_r      sum_c |a_c| e_l(c) + (C + 10) U T, T = sum_c |a_c log p_c|: the any-order bound of a sum of C + 2 terms is
                 (C + 5) U T, the coefficients carry at most three roundings and the products one; one U is margin;
  CE A           (C + 10) U sum_c |a_c| alike; c1, c2, wsum against the float64 reference: 4 U of their magnitude;
  focal          (e_L, e_k) of each label from loss_optim_reference.focal_terms with A_POW; loss_r: lam e_L1 + oml e_L2 +
                 3 U (|lam L1| + |oml L2|); c_i: lam_i e_k_i + 3 U |c_i|; A: e_c1 + e_c2 + U |A|;
  out2           as loss_optim_reference: (B + 3) U sum |terms| plus the terms' own bounds, one rounding for the quotient.
No element is left out of any check."""
from dataclasses import dataclass
from types import SimpleNamespace
from typing import Optional

import numpy as np
import torch

from loss_optim_reference import A_LOG, A_POW, NAN, S, focal_terms
from conv_reference import U
from transformer_reference import A_EXP, ulp32

INF = float("inf")
LOSS_MUTANTS = ("lam_swapped", "delta_lost", "smoothing_unweighted", "normaliser_wy_only")
IMAGE_MUTANTS = ("partner_own_flips", "closed_box")
ROW_FIELDS = ("loss_rows", "wsum", "A", "c1", "c2")


@dataclass(frozen=True)
class Case:
    name: str
    B: int
    C: int
    focal: bool = False
    pad: tuple = (0, 0, 0)          # columns behind C in a row of logits / probs / dlogits
    weight: bool = False
    eps: float = 0.0                # label smoothing (cross entropy)
    gamma: float = 2.0              # focal
    lam: str = "random"             # one | zero | half | random
    ignore: int = -100              # -100, or -1: the in-range class C - 1
    ignored: str = "none"           # none | y | y2 | both (some rows through either label) | all
    bad: str = "none"               # none | y | y2
    reduction: int = 0
    per_row: bool = False

    @property
    def kind_arg(self):
        return 16 | int(self.focal)

    @property
    def gamma_arg(self):
        return self.gamma if self.focal else self.eps


def ignore_value(c: Case):
    return c.C - 1 if c.ignore == -1 else c.ignore


def make(c: Case, seed: int = 0):
    gen = torch.Generator().manual_seed(seed * 1000003 + sum(ord(ch) * (i + 1) for i, ch in enumerate(c.name)) % 999983)
    B, C = c.B, c.C
    d = SimpleNamespace()
    d.x = (2.0 * torch.randn(B, C, generator=gen)).float().contiguous()
    ig = ignore_value(c)
    y = torch.randint(0, C, (B,), generator=gen)
    y2 = torch.randint(0, C, (B,), generator=gen)
    y2 = torch.where(torch.arange(B) % 4 == 0, y, y2)                 # y2 == y on every fourth row
    if 0 <= ig < C and C > 1:
        y = torch.where(y == ig, (y + 1) % (C - 1), y)
        y2 = torch.where(y2 == ig, (y2 + 1) % (C - 1), y2)
    rows = torch.arange(B)
    if c.ignored in ("y", "both"):
        y[rows % 3 == 1] = ig
    if c.ignored in ("y2", "both"):
        y2[rows % 5 == 2] = ig
        y2[B - 1] = ig
    if c.ignored == "all":
        y[rows % 2 == 0] = ig
        y2[rows % 2 == 1] = ig
    if c.bad != "none":
        (y if c.bad == "y" else y2)[0 if B < 3 else 2] = C if c.bad == "y" else -1
    d.y, d.y2 = y, y2
    d.lam = dict(one=torch.ones(B), zero=torch.zeros(B), half=torch.full((B,), 0.5),
                 random=torch.rand(B, generator=gen, dtype=torch.float64))[c.lam].double()     # random: not fp32 numbers
    d.table = torch.stack([y, y2, d.lam.view(torch.int64)])
    d.weight = None
    if c.weight:
        d.weight = torch.rand(C, generator=gen) + 0.5
        d.weight[C // 2] = 0.0
    d.gout = torch.randn(B, generator=gen) if c.per_row else torch.tensor([0.75])
    return d


def wave_sum_rows(T):
    """sum over the columns of T [B, C] in the order of a 64-lane wave: lane l adds its columns l, l + 64, .. in rising order,
    then the xor butterfly with offsets 32, 16, .., 1 (every lane ends with the same bits)"""
    B, C = T.shape
    trips = -(-C // 64)
    Tp = torch.zeros(B, trips * 64, dtype=T.dtype)
    Tp[:, :C] = T
    Tp = Tp.reshape(B, trips, 64)
    v = torch.zeros(B, 64, dtype=T.dtype)
    for t in range(trips):
        v = v + Tp[:, t]
    lanes = torch.arange(64)
    o = 32
    while o:
        v = v + v[:, lanes ^ o]
        o >>= 1
    return v[:, 0]


def _focal_label(lp, w, gam, dt):
    """loss_optim_reference._loss's focal formula for one label: (L, k, the row quantities focal_terms wants)"""
    zero = torch.zeros_like(lp)
    pt = torch.exp(lp)
    om = 1.0 - pt
    f = torch.pow(om, gam)
    gm1 = float(S(gam) - S(1.0))
    fm1 = zero if gam == 0.0 else torch.where(om <= 0.0, zero, gam * torch.pow(om, gm1))
    return (-w * f) * lp, w * (f - (fm1 * pt) * lp), dict(gamma=gam, om=om, pt=pt, f=f, logpt=lp, w=w, g0=fm1)


def dlogits_of(c: Case, d, P, A, c1, c2, sm, ew, out1, dt, mutant=None):
    """g (((A p - c1 [j == y]) - c2 [j == y2]) - ew_j [sm]) in dtype dt from the given forward outputs"""
    B, C = c.B, c.C
    g = d.gout.to(dt)
    g = (g if c.per_row else g[:1].expand(B)) * out1.to(dt)
    j = torch.arange(C)[None, :]
    t = A.to(dt)[:, None] * P.to(dt)
    t = torch.where(j == d.y[:, None], t - c1.to(dt)[:, None], t)
    hit2 = j == d.y2[:, None]
    if mutant == "delta_lost":
        hit2 = hit2 & (d.y2 != d.y)[:, None]
    t = torch.where(hit2, t - c2.to(dt)[:, None], t)
    t = torch.where(sm.bool()[:, None], t - ew.to(dt)[None, :], t)
    return g[:, None] * t


def outputs(c: Case, d, *, exact: bool, mutant: Optional[str] = None):
    """exact: the float64 reference with its e_<name> bounds; else the fp32 yardstick in the documented operation order"""
    dt = torch.float64 if exact else torch.float32
    B, C = c.B, c.C
    X = d.x.to(dt)
    mx = X.max(1).values
    E = torch.exp(X - mx[:, None])
    se = E.sum(1)
    lse = mx + torch.log(se)
    P = E * (1.0 / se)[:, None]
    isn = torch.isnan(X)
    hit = X == mx[:, None]
    out = {"probs": P.double(), "argmax": torch.where(hit, torch.arange(C)[None, :], C).min(1).values.double()}
    assert not bool(isn.any())
    LP = X - lse[:, None]
    lam = d.lam.float().to(dt)
    one = torch.ones(B, dtype=dt)
    oml = one - lam
    if mutant == "lam_swapped":
        lam, oml = oml, lam
    zero, nanv = torch.zeros(B, dtype=dt), torch.full((B,), NAN, dtype=dt)
    ig = ignore_value(c)
    y, y2 = d.y, d.y2
    ign = (y == ig) | (y2 == ig)
    badl = ~ign & ((y < 0) | (y >= C) | (y2 < 0) | (y2 >= C))
    ok = ~ign & ~badl
    yc, y2c = y.clamp(0, C - 1), y2.clamp(0, C - 1)
    lp1, lp2 = LP.gather(1, yc[:, None])[:, 0], LP.gather(1, y2c[:, None])[:, 0]
    wv = d.weight.to(dt) if c.weight else torch.ones(C, dtype=dt)
    w1, w2 = wv[yc], wv[y2c]
    if exact:
        diff = (X - mx[:, None]).abs()
        rho = 2 * A_EXP * U + 2 * U * diff.max(1).values
        r_se = rho + (C + 3) * U
        out["e_probs"] = P * (2 * rho + (C + 3) * U)[:, None] + 2 * A_EXP * 2.0 ** -149
        e_lse = A_LOG * ulp32(torch.log(se)) + 1.01 * r_se + U * lse.abs()
        E_L = e_lse[:, None] + U * LP.abs()
        el1, el2 = E_L.gather(1, yc[:, None])[:, 0], E_L.gather(1, y2c[:, None])[:, 0]
    if not c.focal:
        eps = S(c.eps)
        smooth = float(eps) > 0.0
        keep = (S(1.0) - eps).to(dt) if not exact else torch.tensor(1.0 - float(eps), dtype=dt)
        epsC = (eps / S(C)).to(dt) if not exact else torch.tensor(float(eps) / C, dtype=dt)
        ew = epsC * (torch.ones(C, dtype=dt) if mutant == "smoothing_unweighted" else wv)
        c1, c2 = (lam * keep) * w1, (oml * keep) * w2
        hard = c1 * lp1 + c2 * lp2
        if smooth:
            Sm = wave_sum_rows(ew[None, :] * LP) if not exact else (ew[None, :] * LP).sum(1)
            SW = wave_sum_rows(ew[None, :].expand(B, C).contiguous()) if not exact else ew.sum().expand(B)
            loss, A = -(hard + Sm), (c1 + c2) + SW
        else:
            loss, A = -hard, c1 + c2
        wsum = lam * w1 if mutant == "normaliser_wy_only" else lam * w1 + oml * w2
        sm = ok & smooth
        if exact:
            T = (c1 * lp1).abs() + (c2 * lp2).abs()
            e_loss = c1.abs() * el1 + c2.abs() * el2
            mag = c1.abs() + c2.abs()
            if smooth:
                T = T + (ew[None, :] * LP).abs().sum(1)
                e_loss = e_loss + (ew.abs()[None, :] * E_L).sum(1)
                mag = mag + ew.abs().sum()
            e_loss = e_loss + (C + 10) * U * T
            e_A = (C + 10) * U * mag
            e_c1, e_c2 = 4 * U * c1.abs(), 4 * U * c2.abs()
            e_wsum = 4 * U * ((lam * w1).abs() + (oml * w2).abs())
    else:
        gam = float(S(c.gamma))
        ew = torch.zeros(C, dtype=dt)
        L1, k1, q1 = _focal_label(lp1, w1, gam, dt)
        L2, k2, q2 = _focal_label(lp2, w2, gam, dt)
        loss = lam * L1 + oml * L2
        c1, c2 = lam * k1, oml * k2
        A = c1 + c2
        wsum = one
        sm = torch.zeros(B, dtype=torch.bool)
        if exact:
            q1["e_l"], q2["e_l"] = el1, el2
            (eL1, ek1), (eL2, ek2) = focal_terms(q1, A_POW), focal_terms(q2, A_POW)
            e_loss = lam * eL1 + oml * eL2 + 3 * U * ((lam * L1).abs() + (oml * L2).abs())
            e_c1, e_c2 = lam * ek1 + 3 * U * c1.abs(), oml * ek2 + 3 * U * c2.abs()
            e_A = e_c1 + e_c2 + U * A.abs()
            e_wsum = zero
    pick = lambda v: torch.where(ok, v, torch.where(badl, nanv, zero))          # noqa: E731
    loss, A, c1, c2 = pick(loss), pick(A), pick(c1), pick(c2)
    wsum = torch.where(ok, wsum, torch.where(badl, one, zero))
    out.update(loss_rows=loss.double(), wsum=wsum.double(), A=A.double(), c1=c1.double(), c2=c2.double(), sm=sm.double(),
               ew=ew.double(), pad=torch.zeros(2 * B, dtype=torch.float64))
    a, b = loss.sum(), wsum.sum()
    mean = c.reduction == 0
    if mean:
        o0 = a / b if b > 0 else zero[0]
        o1 = 1.0 / b if b > 0 else zero[0]
    else:
        o0, o1 = a, one[0]
    out["out0"], out["out1"] = o0.double().reshape(1), o1.double().reshape(1)
    if exact:
        keepb = lambda e: torch.where(ok, e, zero)                                # noqa: E731
        out.update(e_loss_rows=keepb(e_loss), e_A=keepb(e_A), e_c1=keepb(e_c1), e_c2=keepb(e_c2), e_wsum=keepb(e_wsum))
        e_a = (B + 3) * U * loss.abs().sum() + keepb(e_loss).sum()
        e_b = (B + 3) * U * wsum.abs().sum() + keepb(e_wsum).sum()
        if mean and b > 0:
            out["e_out0"] = (1.01 * (e_a / b + a.abs() * e_b / (b * b)) + U * (a / b).abs()).reshape(1)
            out["e_out1"] = (1.01 * e_b / (b * b) + U / b).reshape(1)
        else:
            out["e_out0"], out["e_out1"] = (zero[0] if mean else e_a).reshape(1), zero[:1]
    out["dlogits"] = dlogits_of(c, d, P, A, c1, c2, sm, ew, o1, dt, mutant).double()
    return out


# ---- the checks --------------------------------------------------------------------------------------------------------------------
def _worst(got, ref, bound):
    """(ratio, err, bound) of the worst element; a NaN or an infinity must sit exactly where the reference has one"""
    got, ref = got.double().reshape(-1), ref.double().reshape(-1)
    bound = bound.double().reshape(-1).expand_as(ref) if isinstance(bound, torch.Tensor) else torch.full_like(ref, float(bound))
    if got.numel() != ref.numel():
        return INF, INF, 0.0
    if ref.numel() == 0:
        return 0.0, 0.0, 0.0
    same = (got == ref) | (torch.isnan(got) & torch.isnan(ref))
    fin = torch.isfinite(got) & torch.isfinite(ref) & torch.isfinite(bound)
    err = torch.where(same, torch.zeros_like(ref), torch.where(fin, (got - ref).abs(), torch.full_like(ref, INF)))
    ratio = torch.where(err == 0, torch.zeros_like(ref), err / bound.clamp_min(0.0))
    ratio = torch.where(torch.isnan(ratio), torch.full_like(ratio, INF), ratio)
    i = int(ratio.argmax())
    return float(ratio[i]), float(err[i]), float(bound[i])


def exact_fields(c: Case):
    """outputs held bit for bit to the yardstick"""
    return ("argmax", "sm", "pad", "ew") + (() if c.focal else ("c1", "c2", "wsum"))


def verdict(c: Case, d, ref: dict, got: dict, yard: dict) -> dict:
    """{output: (ratio, err, bound)}; a ratio above 1 fails.  ref: outputs(exact=True); yard: outputs(exact=False);
    got: the same names from the code under test (dlogits from ITS forward outputs)"""
    res = {}
    for name in ("probs", "out0", "out1") + ROW_FIELDS:
        res[name] = _worst(got[name], ref[name], ref["e_" + name])
    for name in exact_fields(c):
        res[name + "=="] = _worst(got[name], yard[name], 0.0)
    f = lambda k: got[k].float()                                                  # noqa: E731
    want = dlogits_of(c, d, f("probs"), f("A"), f("c1"), f("c2"), got["sm"], f("ew"), f("out1")[0], torch.float32)
    res["dlogits=="] = _worst(got["dlogits"], want.double(), 0.0)
    return res


def rejecting(c: Case, d, mutant: str):
    """the checks that reject the yardstick made wrong by `mutant` on this case"""
    ref, yard = outputs(c, d, exact=True), outputs(c, d, exact=False)
    bad = outputs(c, d, exact=False, mutant=mutant)
    return [k for k, (ratio, _, _) in verdict(c, d, ref, bad, yard).items() if not ratio <= 1.0]


# ---- the case table ----------------------------------------------------------------------------------------------------------------
LOSS_B = (1, 3, 5, 67)
LOSS_C = (1, 2, 63, 64, 65, 130, 1000)
LOSS_PADS = ((0, 0, 0), (3, 5, 7), (9, 1, 4))
LAMS = ("one", "zero", "half", "random")


def _name(c):
    return (f"{'focal' if c.focal else 'ce'}-B{c.B}-C{c.C}-pad{''.join(map(str, c.pad))}{'-w' if c.weight else ''}-eps{c.eps:g}-"
            f"lam{c.lam}-ign{c.ignore}{c.ignored}{'-bad' + c.bad if c.bad != 'none' else ''}-red{c.reduction}{'-rowg' if c.per_row else ''}")


def _case(**kw):
    return Case(**{**kw, "name": _name(Case(name="", **kw))})


def _cases():
    out, i = [], 0
    for focal in (False, True):
        for B in LOSS_B:
            for C in LOSS_C:
                # every (B, C) once per kind, the other axes cycling against each other with coprime periods
                out.append(_case(B=B, C=C, focal=focal, pad=LOSS_PADS[i % 3], weight=i % 2 == 1, eps=0.1 if (i // 2) % 2 else 0.0,
                                 gamma=(2.0, 0.5, 0.0, 1.0)[i % 4], lam=LAMS[(i // 3) % 4],
                                 ignore=-1 if (i % 7 == 3 and C > 2) else -100, ignored=("none", "y", "y2", "both")[(i // 2) % 4],
                                 reduction=i % 3, per_row=(i // 3) % 2 == 1))
                i += 1
    for focal in (False, True):
        for weight in (False, True):
            for lam in LAMS:               # every lam form on the walk's second trip with and without weights and smoothing
                out.append(_case(B=5, C=65, focal=focal, pad=LOSS_PADS[1], weight=weight, eps=0.1, lam=lam, ignored="both",
                                 per_row=True))
                out.append(_case(B=5, C=65, focal=focal, pad=LOSS_PADS[2], weight=weight, eps=0.0, lam=lam))
        out.append(_case(B=5, C=65, focal=focal, weight=True, eps=0.1, ignored="all"))
        out.append(_case(B=3, C=2, focal=focal, eps=0.1, ignored="all", reduction=1))
        for bad in ("y", "y2"):
            out.append(_case(B=5, C=65, focal=focal, weight=True, eps=0.1, bad=bad, pad=LOSS_PADS[1]))
    seen, uniq = set(), []
    for c in out:
        if c.name not in seen:
            seen.add(c.name)
            uniq.append(c)
    return uniq


CASES = _cases()


# ---- flag bit 3 of nkb_image_prep on arrays ------------------------------------------------------------------------------------------
def make_mix_words(partner, *, lam=None, box=None):
    """words 10..15 of a record: a blend with float32 lam (oml = float32(1) - lam), or a box (y1, x1, y2, x2)"""
    w = np.zeros(6, np.int32)
    w[0] = partner
    if box is None:
        w[1] = 1
        f = w.view(np.float32)
        f[2] = np.float32(lam)
        f[3] = np.float32(1.0) - np.float32(lam)
    else:
        w[1] = 2
        w[2:6] = box
    return w


def mix_images(plain_of, flags, records, Ho, Wo, mutant=None):
    """out [B, 3, Ho, Wo] float32 under the rule of include/nkbhip.h.  plain_of(k, fl): the un-mixed value of image k, float32
    [3, Ho, Wo], evaluated with the flag byte fl (bits 0..2); records: int32 [B, 64]"""
    B = len(flags)
    out = []
    for b in range(B):
        fl = int(flags[b])
        mine = plain_of(b, fl & 7)
        if not fl & 8:
            out.append(mine)
            continue
        rec = np.asarray(records[b], np.int32)
        p, mode = int(rec[10]), int(rec[11])
        if p == b or not 0 <= p < B or mode not in (1, 2):
            out.append(mine)
            continue
        pf = int(flags[p]) & 7
        if mutant == "partner_own_flips":
            pf = (fl & 3) | (pf & 4)
        other = plain_of(p, pf)
        if mode == 1:
            lam, oml = rec.view(np.float32)[12], rec.view(np.float32)[13]
            out.append((lam * mine.astype(np.float32)) + (oml * other.astype(np.float32)))
        else:
            y1, x1, y2, x2 = (int(v) for v in rec[12:16])
            if mutant == "closed_box":
                y2, x2 = y2 + 1, x2 + 1
            y1, x1, y2, x2 = max(y1, 0), max(x1, 0), min(y2, Ho), min(x2, Wo)
            res = mine.copy()
            if y2 > y1 and x2 > x1:
                res[:, y1:y2, x1:x2] = other[:, y1:y2, x1:x2]
            out.append(res)
    return np.stack(out).astype(np.float32)
