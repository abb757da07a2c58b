"""Float64 reference of the BatchNorm and pooling kernels of csrc/elementwise.hip (nkb_bn_finalize, nkb_bn_apply, nkb_bn_backward,
nkb_bn_backward_from_stats, nkb_maxpool3x3s2 and the two global-average modes of nkb_avgpool), the fp32 yardstick (the same math in
the kernels' documented order and rounding places), the derived bounds that tests/test_bn_pool_gpu.py holds the kernels to, mutants
that make the yardstick wrong the way these kernels go wrong, and the case table both test files walk.  tests/test_bn_reference.py
proves on the CPU that the reference equals torch's batch_norm / max_pool2d / adaptive_avg_pool2d and their autograd in float64 and
that the checks reject every mutant.  No test lives here.

The operations, float64 from the same stored operands (rnd = the store rounding of the compute dtype, M = rows):
  finalize   s, ss = column sums of the fp32 partials [tiles][2][C] exactly as given; mean = s / count, var = max(ss / count -
             mean^2, 0) (biased), invstd = 1 / sqrt(var + eps), scale = gamma invstd, shift = beta - mean scale, running = (1 -
             momentum) running + momentum (mean | unbiased var; the biased one when count == 1).  Eval mode: scale / shift from the
             running statistics, nothing else written.
  apply      y = act(x scale + shift (+ res | + rnd(res res_scale + res_shift))); bit e of byte `chunk` of a row = stored y > 0.
  backward   g' = dy under the mask (yact > 0 | the bit array | rnd(x fscale + fshift) > 0 | none), s1 = sum g', s2 = sum g' (x -
             mean) invstd, dbeta += s1, dgamma += s2, dx = gamma invstd (g' - s1 / M - xhat s2 / M), dy_masked = g'.
  from_stats the same finish from [tiles][2][C] sums of g' and g' (x - mean): s1 = sum_t stats[t][0], s2 = invstd sum_t stats[t][1].
  max-pool   3x3 / stride 2 / pad 1 with -inf padding, the first tap in row-major order wins ties, NaN propagates (a later NaN
             takes the slot); backward routes every pooled gradient to the pixel its stored slot names.
  avg-pool   y = sum_k x[n][k][c] / HW; backward dx = g / HW.

The bounds (derived; none is tuned on a kernel's output; U = 2^-24, R_BF16 = 2^-8):
  exact cases   carry the precision and are the checks that detect a lost, duplicated or misrouted row.  Operands are chosen so
             that every fp32 sum is exact in any order: gradients are integers in [-3, 3], x integers in [-8, 8], mean an integer
             vector in [-2, 2], invstd in {0.5, 1, 2}, so a term is a multiple of 0.5 of magnitude <= 3 * 10 * 2 and rows * 3 * 10
             * 2 < 2^24 keeps every partial sum representable; fscale is 1 or 2 and fshift an integer + 0.5 (no mask element on the
             edge); apply: x, res, shift multiples of 0.25 in [-4, 4], scale and res_scale powers of two.  Then sums, dgamma / dbeta
             (accumulated into integer pre-fills), dy_masked, y, the bits, the max-pool outputs and the avg-pool of HW = 2^k equal
             the reference value for value.  `representable` (asserted on the CPU) checks that claim before a GPU is involved.
             bf16 exact cases without a residual carry one channel with scale = 2^-140: x scale is a positive fp32 subnormal that
             the bf16 store rounds to zero, the only place where "stored y > 0" and "y > 0 before the store" differ.
  stores     |got - ref| <= r (|ref| + e) + e + t,  r = R_BF16 for a bf16 store and 0 for fp32, e = n U sum |operand terms| with n
             the fp32 roundings of the documented expression counted for separate multiply and add (a contracted one has fewer):
             apply n = 2 (+ 1 with a residual) over |x scale| + |shift| + |res'|; avg-pool forward n = HW + 3 over sum |x| / HW
             (HW - 1 additions, 1 / HW, the product); avg-pool backward n = 2; max-pool backward n = 3 (at most four routed
             terms).  t = 2^-134 (bf16) / 2^-150 (fp32): half the smallest subnormal, the absolute part of a store that
             underflows.  The inner rnd of the res_scale form may land on either neighbour when the fp32 value sits within 2 U
             (|res res_scale| + |res_shift|) of a rounding tie: the element is held to the better of the two.
  dx         the form tests/test_stem_tail_gpu.py uses for the same three-term expression: r |ref| + 2^-20 (|k1 g'| + |k2 x| +
             |k3|), ref = k1 g' + k2 x + k3 in float64 with k1 = gamma invstd, k2 = -k1 invstd s2 / M, k3 = -k1 s1 / M + k1 invstd
             (s2 / M) mean formed in fp32 in the kernel's operation order from the sums the LIBRARY produced (k3 with its two
             multiply-adds separate or contracted, the element is held to the best); the library's sums are held to the reduction
             bound separately.  Because s / M enters with weight 1 / M, this check cannot see 1 / (M - 1) in place of 1 / M once
             1 / M is below the store's precision: that mutant exists at M <= 64 (bf16) / 4096 (fp32).
  reductions sums, dgamma, dbeta: |got - ref| <= (rows + 3) U (sum |terms| + |pre-fill|) per channel (from_stats: tiles in place
             of rows).  Valid for ANY fp32 summation order (rows - 1 additions of partial sums below sum |terms|, the three
             roundings of a term, the final store and accumulate).  It is deliberately loose and exists to catch formula errors;
             the exact cases carry the precision.
  finalize   per output, roundings x U x magnitude, the reference evaluated from the same fp32 partials (their own error is not
             this kernel's), plus D = (tiles + 4) 2^-53 (ss / count + mean^2), the kernel's double accumulation, on var:
             mean: U |mean|; invstd: n = 6 (the store of var, + eps, sqrtf and the division at one ulp = 2 U each), + D / (2 (var
             + eps)); scale: n = 7; shift: 9 U |mean scale| + U |shift| (mean, invstd, two products, the subtraction);
             running: 3 U (|(1 - m) old| + |m new|) (1 - m, the product, the sum | the stored statistic, the product, the sum).
  bits       bit-exact against the STORED y.
  mask edge  an element whose float64 |x fscale + fshift| < MASK_EDGE (|x fscale| + |fshift|) may fall on either side: it is left
             out of the element checks and its |term| is added to the reduction bounds.  At most MASK_SHARE of a case's elements
             may be left out (expected with the table's inputs: about 1e-6); exact cases have none.
"""
import math
from dataclasses import dataclass
from types import SimpleNamespace
from typing import Optional

import torch

from conv_reference import MASK_EDGE, MASK_SHARE, R_BF16, TORCH_DT, U, bf, pack_bits, unpack_bits

GARBAGE = 1e4
TINY = {"bf16": 2.0 ** -134, "f32": 2.0 ** -150}
TINY_SCALE = 2.0 ** -140
INF = float("inf")

MUTANTS = ("drop_last_row", "drop_second_row", "dup_tail_row", "row_past_end", "mask_ge", "mask_unrounded", "xhat_no_mean",
           "inv_rows_minus_one", "biased_running_var", "momentum_swapped", "res_unnormalised", "bits_prerounding", "last_wins_ties",
           "window_wraps", "no_inv_hw")
# the outputs whose check rejects each mutant (tests/test_bn_reference.py asserts exactly this)
REJECTED_BY = dict(drop_last_row=("sums", "dgamma", "dbeta", "y"), drop_second_row=("sums", "dgamma", "dbeta"),
                   dup_tail_row=("sums", "dgamma", "dbeta"), row_past_end=("sums", "dgamma", "dbeta", "y"),
                   mask_ge=("sums", "dbeta", "dgamma", "dym"), mask_unrounded=("sums", "dbeta", "dgamma", "dym"),
                   xhat_no_mean=("sums", "dgamma"), inv_rows_minus_one=("dx",), biased_running_var=("running_var",),
                   momentum_swapped=("running_mean", "running_var"), res_unnormalised=("y",), bits_prerounding=("bits",),
                   last_wins_ties=("idx",), window_wraps=("y",), no_inv_hw=("y",))
# mutants of a formula: also random cases must reject them (row and mask mutants hide inside the loose reduction bound there)
FORMULA_MUTANTS = ("xhat_no_mean", "inv_rows_minus_one", "biased_running_var", "momentum_swapped", "res_unnormalised", "no_inv_hw")


@dataclass(frozen=True)
class Case:
    kind: str                       # apply | bwd | fin | fs | maxpool | avgpool
    name: str
    dtype: str = "bf16"
    rows: int = 0
    C: int = 0
    exact: bool = False
    res: str = "none"               # apply: none | res | proj (res_scale / res_shift)
    relu: bool = True
    bits: bool = True
    mask: str = "none"              # bwd: none | yact | bits | fmask
    dx: bool = True
    dym: str = "none"               # none | sep | inplace
    tiles: int = 0                  # fin / fs
    count: int = 0
    training: bool = True
    cond: str = "normal"            # fin: normal | bad (mean 100, std 0.1)
    N: int = 0                      # pools (avg-pool: H = HW, W = 1)
    H: int = 0
    W: int = 0
    fill: str = "random"

    @property
    def big(self):
        return max(self.rows, self.tiles, self.N * self.H * self.W) * self.C > (1 << 21)


# ---- helpers ---------------------------------------------------------------------------------------------------------------------
def chunk(dtype):
    return 8 if dtype == "bf16" else 4


def f32(t):
    """a float64 tensor rounded to fp32, kept in float64"""
    return t.float().double()


def rnd(t, dtype):
    """the store rounding of the compute dtype, kept in t's dtype"""
    return bf(t) if dtype == "bf16" else t.float().to(t.dtype)


def bwd_geometry(rows, C, dtype):
    """(chunks per row, threads, threads per chunk column, blocks) of nkb_bn_backward's reduction, by its documented sizing rule"""
    cpr = C // chunk(dtype)
    threads = 256
    while threads < cpr:
        threads *= 2
    tpc = threads // cpr
    blocks = min(512, max(1, -(-rows // (tpc * 16))))
    return cpr, threads, tpc, blocks


def apply_geometry(rows, C, dtype):
    """(grid, row stride) of bn_apply_kernel / bn_bwd_apply_kernel (grid_cols)"""
    cpr = C // chunk(dtype)
    g0 = cpr // math.gcd(cpr, 256)
    g = min(-(-rows * cpr // 256), 2048)
    g = max(-(-g // g0) * g0, g0)
    return g, g * 256 // cpr


def partitions(C):
    return 64 if C <= 128 else 32 if C <= 256 else 16


def stats_floats(tiles, C):
    """nkb_bn_stats_floats"""
    return tiles * 2 * C + 2 + (partitions(C) * 4 * C if tiles > 128 else 0)


def bwd_ws_floats(rows, C):
    """nkb_bn_backward_workspace_floats"""
    return min(max((rows + 7) // 8, 1), 4096) * 2 * C + 2 * C


def _elem(got, ref, bound, skip=None):
    """(worst err / bound, that err, that bound); a NaN must sit exactly where the reference has one"""
    got, ref = got.double(), ref.double()
    nan = torch.isnan(ref)
    err = (got - ref).abs()
    err = torch.where(nan, torch.where(torch.isnan(got), 0.0, INF).to(err), err)
    err = torch.where(torch.isnan(err), torch.full_like(err, INF), err)
    if skip is not None:
        err = torch.where(skip, torch.zeros_like(err), err)
    bound = bound.expand_as(err)
    ratio = torch.where(err > 0, err / bound.clamp_min(1e-300), torch.zeros_like(err))
    return ratio, err, bound


def _worst(ratio, err, bound):
    if ratio.numel() == 0:
        return (0.0, 0.0, 0.0)
    i = int(ratio.reshape(-1).argmax())
    return (ratio.reshape(-1)[i].item(), err.reshape(-1)[i].item(), bound.reshape(-1)[i].item())


def _store(got, ref, e, dtype, skip=None):
    r = R_BF16 if dtype == "bf16" else 0.0
    ref = ref.double()
    return _elem(got, ref, r * (ref.abs() + e) + e + TINY[dtype], skip)


def _same(got, ref, skip=None):
    """value for value (NaN where the reference has one): ratio 0 or inf"""
    return _elem(got, ref, torch.zeros((), dtype=torch.float64, device=ref.device), skip)


def _colsum(t, exact, order=None, gs=1):
    """column sum of [rows][C]: float64, or fp32 in torch's order / (order == "strided") per residue of the row index mod gs first"""
    if exact:
        return t.double().sum(0)
    t = t.float()
    if order == "strided":
        r = torch.arange(t.shape[0], device=t.device) % gs
        return torch.zeros(gs, t.shape[1], device=t.device).index_add_(0, r, t).sum(0)
    return t.sum(0)


# ---- operands --------------------------------------------------------------------------------------------------------------------
def make(c: Case, device, seed: int = 0):
    """the stored operands of a case, on `device`; generated on the CPU from a seed that depends on the case's name alone"""
    gen = torch.Generator().manual_seed(seed * 1000003 + sum(ord(ch) * (i + 1) for i, ch in enumerate(c.name)) % 999983)
    dt = TORCH_DT[c.dtype]
    C = c.C
    randn = lambda *s: torch.randn(*s, generator=gen)
    rint = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=gen).float()
    pick = lambda vals, *s: torch.tensor(vals)[torch.randint(0, len(vals), s, generator=gen)]
    d = SimpleNamespace()
    tiny = c.exact and c.dtype == "bf16" and C > 1
    if c.kind == "apply":
        if c.exact:
            d.x, d.res = rint(-16, 16, c.rows, C) * 0.25, rint(-16, 16, c.rows, C) * 0.25
            d.scale, d.shift = pick([0.5, 1.0, 2.0, -1.0], C), rint(-16, 16, C) * 0.25
            d.res_scale, d.res_shift = pick([0.5, 1.0], C), rint(-16, 16, C) * 0.25
            if tiny and c.res == "none":
                d.scale[1], d.shift[1] = TINY_SCALE, 0.0
        else:
            d.x = randn(C) + (torch.rand(C, generator=gen) + 0.5) * randn(c.rows, C)
            d.res = randn(c.rows, C)
            d.scale = (torch.rand(C, generator=gen) + 0.5) * pick([1.0, 1.0, 1.0, -1.0], C)
            d.shift, d.res_scale, d.res_shift = randn(C), torch.rand(C, generator=gen) + 0.5, 0.5 * randn(C)
        d.x, d.res = d.x.to(dt), d.res.to(dt)
        if c.res == "none":
            d.res = None
        if c.res != "proj":
            d.res_scale = d.res_shift = None
    elif c.kind in ("bwd", "fs"):
        if c.exact:
            d.dy, d.x = rint(-3, 3, c.rows, C), rint(-8, 8, c.rows, C)
            d.mean, d.invstd, d.gamma = rint(-2, 2, C), pick([0.5, 1.0, 2.0], C), pick([0.5, 1.0, 2.0], C)
            d.yact = rint(-2, 2, c.rows, C)
            d.fscale, d.fshift = pick([1.0, 2.0], C), rint(-6, 6, C) + 0.5
            if tiny:
                d.fscale[1], d.fshift[1] = TINY_SCALE, 0.0
            d.dgamma0, d.dbeta0 = rint(-5, 5, C), rint(-5, 5, C)
        else:
            d.x = (randn(C) + (torch.rand(C, generator=gen) * 1.5 + 0.5) * randn(c.rows, C)).to(dt).float()
            d.dy, d.yact = randn(c.rows, C), randn(c.rows, C)
            d.mean = d.x.mean(0)
            d.invstd = (d.x.var(0, unbiased=False) + 1e-5).rsqrt() if c.rows > 1 else torch.ones(C)
            d.gamma = torch.rand(C, generator=gen) + 0.5
            d.fscale = d.gamma * d.invstd
            d.fshift = 0.1 - d.mean * d.fscale
            d.dgamma0, d.dbeta0 = randn(C), randn(C)
        d.bitmask = torch.rand(c.rows, C, generator=gen) < 0.6
        d.dy, d.x, d.yact = d.dy.to(dt), d.x.to(dt), d.yact.to(dt)
        if c.kind == "fs":
            d.stats = rint(-3, 3, c.tiles, 2, C) if c.exact else 4.0 * randn(c.tiles, 2, C)
    elif c.kind == "fin":
        R = max(c.count // c.tiles, 1)
        m, s = (torch.full((C,), 100.0), torch.full((C,), 0.1)) if c.cond == "bad" else (randn(C), torch.rand(C, generator=gen) * 1.5 + 0.5)
        x = (m + s * randn(c.tiles, R, C)).double()
        d.partials = torch.stack([x.sum(1), (x * x).sum(1)], 1).float()
        d.gamma, d.beta = torch.rand(C, generator=gen) + 0.5, randn(C)
        d.rm, d.rv = randn(C), torch.rand(C, generator=gen) + 0.5
        d.momentum, d.eps = torch.tensor(0.1).item(), torch.tensor(1e-5).item()          # the fp32 values the kernel receives
    elif c.kind == "maxpool":
        N, H, W = c.N, c.H, c.W
        P, Q = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        x = randn(N, H, W, C)
        if c.fill == "ties":
            x = (x * 2).round() / 4
        if c.fill == "negative":
            x = -1.0 - x.abs().round()
        if c.fill.startswith("nan"):
            p, q = min(1, P - 1), min(1, Q - 1)
            taps = [(2 * p - 1 + r, 2 * q - 1 + s) for r in range(3) for s in range(3) if 0 <= 2 * p - 1 + r < H and 0 <= 2 * q - 1 + s < W]
            h, w = dict(nan_first=taps[0], nan_middle=taps[len(taps) // 2], nan_last=taps[-1])[c.fill]
            x[:, h, w, :] = float("nan")
        d.x = x.to(dt)
        d.g = (rint(-3, 3, N, P, Q, C) if c.exact else randn(N, P, Q, C)).to(dt)
    elif c.kind == "avgpool":
        d.x = (rint(-1, 1, c.N, c.H, C) if c.exact else randn(c.N, c.H, C)).to(dt)
        d.g = (rint(-3, 3, c.N, C) if c.exact else randn(c.N, C)).to(dt)
    for k, v in vars(d).items():
        if isinstance(v, torch.Tensor):
            setattr(d, k, v.contiguous().to(device))
    return d


# ---- the operations: exact = float64 reference, otherwise the fp32 yardstick (with an optional mutant) ---------------------------------
def _finalize(c, d, exact, mutant, order):
    up = (lambda t: t.double()) if exact else (lambda t: t.float())
    p = d.partials.double()
    if order == "strided" and not exact:          # the kernel's two-level order, still in double
        T = p.shape[0]
        pad = torch.zeros(-T % 16, 2, c.C, dtype=p.dtype, device=p.device)
        s = torch.cat([p, pad]).reshape(-1, 16, 2, c.C).sum(0).sum(0)
    else:
        s = p.sum(0)
    out = {}
    gamma, beta, rm, rv = up(d.gamma), up(d.beta), up(d.rm), up(d.rv)
    mom, eps, cnt = d.momentum, d.eps, float(c.count)
    if c.training:
        m = s[0] / cnt
        v = (s[1] / cnt - m * m).clamp_min(0.0)
        unb = v * cnt / (cnt - 1.0) if c.count > 1 and mutant != "biased_running_var" else v
        mean, var, unb = up(m), up(v), up(unb)
        a, b = (mom, 1.0 - mom) if mutant == "momentum_swapped" else (1.0 - mom, mom)
        if not exact:
            a, b = torch.tensor(a).float(), torch.tensor(b).float()
        out["running_mean"] = a * rm + b * mean
        out["running_var"] = a * rv + b * unb
        out["mean"] = mean
    else:
        mean, var = rm, rv
    invstd = 1.0 / torch.sqrt(var + eps)
    out["scale"] = gamma * invstd
    out["shift"] = beta - mean * gamma * invstd
    if c.training:
        out["invstd"] = invstd
    return {k: v.double() for k, v in out.items()}


def _apply(c, d, exact, mutant):
    up = (lambda t: t.double()) if exact else (lambda t: t.float())
    x = up(d.x)
    a = x * up(d.scale) + up(d.shift)
    terms = (x * up(d.scale)).abs() + up(d.shift).abs()
    out = {}
    if d.res is not None:
        q = up(d.res)
        if d.res_scale is not None and mutant != "res_unnormalised":
            inner = q * up(d.res_scale) + up(d.res_shift)
            q = rnd(inner, c.dtype)
            if exact:       # the neighbour the fp32 evaluation may round to instead
                ei = 2 * U * ((up(d.res) * up(d.res_scale)).abs() + up(d.res_shift).abs())
                lo, hi = rnd(inner - ei, c.dtype), rnd(inner + ei, c.dtype)
                out["q_alt"] = torch.where(lo != q, lo, hi)
        terms = terms + q.abs()
        if "q_alt" in out:
            alt = a + out.pop("q_alt")
            out["y_alt"] = alt.clamp_min(0.0) if c.relu else alt
        a = a + q
    y = torch.where(torch.isnan(a), a, a.clamp_min(0.0)) if c.relu else a
    out["y"] = y if exact else rnd(y, c.dtype)
    out["terms"] = terms
    if c.bits:
        out["bits"] = (y if mutant == "bits_prerounding" else rnd(y, c.dtype)) > 0
    if mutant == "drop_last_row" and not exact:       # the row is never written: the output keeps its NaN
        out["y"] = out["y"].clone()
        out["y"][-1] = float("nan")
    return out


def _mask(c, d, exact, mutant):
    """(mask, skip): skip marks the recomputed-mask elements on the edge (float64 only)"""
    up = (lambda t: t.double()) if exact else (lambda t: t.float())
    if c.kind == "fs" or c.mask == "none":
        return None, None
    if c.mask == "yact":
        return (up(d.yact) >= 0) if mutant == "mask_ge" else (up(d.yact) > 0), None
    if c.mask == "bits":
        return d.bitmask, None
    xs = up(d.x) * up(d.fscale)
    v = xs + up(d.fshift)
    skip = (v.abs() < MASK_EDGE * (xs.abs() + up(d.fshift).abs())) if exact else None
    if mutant != "mask_unrounded":
        v = rnd(v, c.dtype)
    return (v >= 0) if mutant == "mask_ge" else (v > 0), skip


def _backward(c, d, exact, mutant, order):
    up = (lambda t: t.double()) if exact else (lambda t: t.float())
    rows, C = c.rows, c.C
    x, mean, invstd, gamma = up(d.x), up(d.mean), up(d.invstd), up(d.gamma)
    mask, skip = _mask(c, d, exact, mutant)
    g = up(d.dy) if mask is None else torch.where(mask, up(d.dy), torch.zeros((), dtype=x.dtype, device=x.device))
    out = {"g": g, "skip": skip}
    if c.kind == "fs":
        st = d.stats.double()
        if mutant == "drop_last_row":
            st = st[:-1]
        if mutant == "row_past_end":
            st = torch.cat([st, torch.full_like(st[:1], GARBAGE)])
        s = st.sum(0)
        s1, s2 = up(s[0]), up(s[1] * d.invstd.double())
        out["abs1"], out["abs2"] = d.stats[:, 0].double().abs().sum(0), (d.stats[:, 1].double().abs().sum(0) * d.invstd.double().abs())
    else:
        t1 = g
        t2 = g * x * invstd if mutant == "xhat_no_mean" else g * (x - mean) * invstd
        _, _, tpc, blocks = bwd_geometry(rows, C, c.dtype)
        gs = blocks * tpc
        if mutant == "drop_last_row":
            t1, t2 = t1[:-1], t2[:-1]
        if mutant == "drop_second_row":
            keep = torch.arange(rows, device=x.device) != gs
            t1, t2 = t1[keep], t2[keep]
        if mutant == "dup_tail_row":
            t1, t2 = torch.cat([t1, t1[-1:]]), torch.cat([t2, t2[-1:]])
        if mutant == "row_past_end":
            extra = torch.full_like(t1[:1], GARBAGE)
            t1, t2 = torch.cat([t1, extra]), torch.cat([t2, extra * (extra - mean) * invstd])
        s1, s2 = _colsum(t1, exact, order, gs), _colsum(t2, exact, order, gs)
        out["abs1"], out["abs2"] = t1.double().abs().sum(0), t2.double().abs().sum(0)
        if skip is not None:
            edge = torch.where(skip, up(d.dy).abs(), torch.zeros_like(x))
            out["edge1"], out["edge2"] = edge.sum(0), (edge * ((x - mean) * invstd).abs()).sum(0)
    out["sums"] = torch.stack([s1, s2]).double()
    out["dbeta"], out["dgamma"] = (up(d.dbeta0) + s1).double(), (up(d.dgamma0) + s2).double()
    if c.dx:
        if exact:
            out["dx"] = gamma * invstd * (g - s1 / rows - (x - mean) * invstd * s2 / rows)
        else:
            inv = 1.0 / torch.tensor(float(rows - 1 if mutant == "inv_rows_minus_one" else rows))
            a = gamma * invstd
            sdy, sdyx = s1 * inv, s2 * inv
            k1, k2, k3 = a, (-a) * invstd * sdyx, (-a) * sdy + a * invstd * sdyx * mean
            out["dx"] = rnd(k1 * g + (k2 * x + k3), c.dtype).double()
        if c.kind == "bwd" and c.dym != "none":
            out["dym"] = g.double()
    return out


def _pool_taps(c, x, mutant):
    """the nine taps of every pooled position: values [9][N][P][Q][C] and validity [9][P][Q]"""
    N, H, W, C = x.shape
    P, Q = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    dev = x.device
    pp, qq = torch.arange(P, device=dev)[:, None], torch.arange(Q, device=dev)[None, :]
    flat = x.reshape(N, H * W, C)
    vals, valid = [], []
    for r in range(3):
        for s in range(3):
            h, w = (2 * pp - 1 + r).expand(P, Q), (2 * qq - 1 + s).expand(P, Q)
            pix = h * W + w
            ok = (h >= 0) & (h < H) & (w >= 0) & (w < W)
            if mutant == "window_wraps":       # a column outside the image reads the neighbouring row's pixel
                ok = (h >= 0) & (h < H) & (pix >= 0) & (pix < H * W)
            vals.append(flat[:, pix.clamp(0, H * W - 1).reshape(-1), :].reshape(N, P, Q, C))
            valid.append(ok)
    return torch.stack(vals), torch.stack(valid)


def _maxpool(c, d, exact, mutant):
    up = (lambda t: t.double()) if exact else (lambda t: t.float())
    x = up(d.x)
    N, H, W, C = x.shape
    vals, valid = _pool_taps(c, x, mutant)
    P, Q = vals.shape[2:4]
    best = torch.full((N, P, Q, C), -INF, dtype=x.dtype, device=x.device)
    idx = torch.zeros((N, P, Q, C), dtype=torch.long, device=x.device)
    seen = torch.zeros((1, P, Q, 1), dtype=torch.bool, device=x.device)
    for k in range(9):
        v, ok = vals[k], valid[k][None, :, :, None]
        gt = (v >= best) if mutant == "last_wins_ties" else (v > best)
        take = ok & (~seen | gt | torch.isnan(v))
        best, idx = torch.where(take, v, best), torch.where(take, torch.full_like(idx, k), idx)
        seen = seen | ok
    # backward: every pooled gradient to pixel (2p - 1 + slot / 3, 2q - 1 + slot % 3)
    g = up(d.g)
    pp = torch.arange(P, device=x.device)[None, :, None, None]
    qq = torch.arange(Q, device=x.device)[None, None, :, None]
    nn = torch.arange(N, device=x.device)[:, None, None, None]
    cc = torch.arange(C, device=x.device)[None, None, None, :]
    hh, ww = 2 * pp - 1 + idx // 3, 2 * qq - 1 + idx % 3
    flat = (((nn * H + hh.clamp(0, H - 1)) * W + ww.clamp(0, W - 1)) * C + cc).reshape(-1)
    dx = torch.zeros(N * H * W * C, dtype=g.dtype, device=x.device).index_add_(0, flat, g.reshape(-1)).reshape(N, H, W, C)
    gabs = torch.zeros(N * H * W * C, dtype=torch.float64, device=x.device).index_add_(0, flat, g.double().abs().reshape(-1))
    return {"y": best.double(), "idx": idx, "dx": (dx if exact else rnd(dx, c.dtype)).double(), "gabs": gabs.reshape(N, H, W, C)}


def _avgpool(c, d, exact, mutant, order):
    up = (lambda t: t.double()) if exact else (lambda t: t.float())
    x, g = up(d.x), up(d.g)
    HW = c.H
    if mutant == "drop_last_row":
        x = x[:, :-1]
    if mutant == "row_past_end":
        x = torch.cat([x, torch.full_like(x[:, :1], GARBAGE)], 1)
    s = x.flip(1).sum(1) if order == "strided" else x.sum(1)
    if exact:
        y, dx = s / HW, (g / HW)[:, None, :].expand(c.N, HW, c.C)
    else:
        inv = 1.0 if mutant == "no_inv_hw" else (1.0 / torch.tensor(float(HW)))
        y, dx = rnd(s * inv, c.dtype), rnd(g * (1.0 / torch.tensor(float(HW))), c.dtype)[:, None, :].expand(c.N, HW, c.C)
    return {"y": y.double(), "dx": dx.double(), "xabs": up(d.x).double().abs().sum(1) / HW}


def outputs(c: Case, d, *, exact: bool, mutant: Optional[str] = None, order: Optional[str] = None):
    if c.kind == "fin":
        return _finalize(c, d, exact, mutant, order)
    if c.kind == "apply":
        return _apply(c, d, exact, mutant)
    if c.kind in ("bwd", "fs"):
        return _backward(c, d, exact, mutant, order)
    if c.kind == "maxpool":
        return _maxpool(c, d, exact, mutant)
    return _avgpool(c, d, exact, mutant, order)


def mutant_applies(c: Case, mutant: str) -> bool:
    """whether the mutant can exist at the case at all (whether it changes anything there is decided by `rejecting`)"""
    k = c.kind
    table = dict(
        drop_last_row=(k in ("bwd", "fs") and c.rows > 1 and c.tiles != 1) or (k == "avgpool" and c.H > 1) or k == "apply",
        drop_second_row=k == "bwd" and c.rows > bwd_geometry(c.rows, c.C, c.dtype)[2] * bwd_geometry(c.rows, c.C, c.dtype)[3],
        dup_tail_row=k == "bwd", row_past_end=k in ("bwd", "fs", "avgpool"),
        mask_ge=k == "bwd" and c.mask in ("yact", "fmask"), mask_unrounded=k == "bwd" and c.mask == "fmask",
        xhat_no_mean=k == "bwd", inv_rows_minus_one=k in ("bwd", "fs") and c.dx and c.rows <= (64 if c.dtype == "bf16" else 4096) and c.rows > 1,
        biased_running_var=k == "fin" and c.training and c.count > 1, momentum_swapped=k == "fin" and c.training,
        res_unnormalised=k == "apply" and c.res == "proj", bits_prerounding=k == "apply" and c.bits,
        last_wins_ties=k == "maxpool", window_wraps=k == "maxpool", no_inv_hw=k == "avgpool" and c.H > 1)
    return table[mutant]


# ---- the checks ------------------------------------------------------------------------------------------------------------------
def _dx_check(c, d, ref, got):
    """dx against k1 g' + k2 x + k3 with the constants formed in fp32, in the kernel's order, from the sums `got` carries"""
    x64, g64 = d.x.double(), ref["g"].double()
    ga, is_, mu = d.gamma.double(), d.invstd.double(), d.mean.double()
    s1, s2 = got["sums"][0].double(), got["sums"][1].double()
    inv = f32(1.0 / torch.tensor(float(c.rows), dtype=torch.float64, device=x64.device))
    a = f32(ga * is_)
    sdy, sdyx = f32(s1 * inv), f32(s2 * inv)
    k1, k2 = a, f32(f32(-a * is_) * sdyx)
    t1, u = f32(-a * sdy), f32(f32(a * is_) * sdyx)
    t2 = f32(u * mu)
    r = R_BF16 if c.dtype == "bf16" else 0.0
    best = None
    for k3 in (f32(t1 + t2), f32(-a * sdy + t2), f32(t1 + u * mu)):
        dref = k1 * g64 + k2 * x64 + k3
        bound = r * dref.abs() + 2.0 ** -20 * ((k1 * g64).abs() + (k2 * x64).abs() + k3.abs()) + TINY[c.dtype]
        res = _elem(got["dx"], dref, bound, ref["skip"])
        best = res if best is None else tuple(torch.where(res[0] < best[0], n, o) for n, o in zip(res, best))
    return _worst(*best)


def verdict(c: Case, d, ref: dict, got: dict) -> dict:
    """{output: (worst err / bound, err, bound)} of `got` (a kernel's or a yardstick's outputs as float64 / bool / long tensors)"""
    v = {}
    if c.kind == "fin":
        p = d.partials.double()
        cnt = float(c.count)
        mom = d.momentum
        if c.training:
            s, ab = p.sum(0), p.abs().sum(0)
            m = s[0] / cnt
            var = (s[1] / cnt - m * m).clamp_min(0.0)
            D = (c.tiles + 4) * 2.0 ** -53 * (ab[1] / cnt + m * m)
            dm = (c.tiles + 4) * 2.0 ** -53 * ab[0] / cnt
            unb = var * cnt / (cnt - 1.0) if c.count > 1 else var
            v["mean"] = _worst(*_elem(got["mean"], ref["mean"], U * m.abs() + dm))
            v["running_mean"] = _worst(*_elem(got["running_mean"], ref["running_mean"],
                                              3 * U * (((1 - mom) * d.rm.double()).abs() + (mom * m).abs()) + mom * dm))
            v["running_var"] = _worst(*_elem(got["running_var"], ref["running_var"],
                                             3 * U * (((1 - mom) * d.rv.double()).abs() + mom * unb) + 2 * mom * D))
            mean = m
        else:
            var, mean, D, dm = d.rv.double(), d.rm.double(), 0.0, 0.0
        rel = D / (2 * (var + d.eps))
        is_ = ref["invstd"] if c.training else 1.0 / torch.sqrt(var + d.eps)
        sc = ref["scale"]
        if c.training:
            v["invstd"] = _worst(*_elem(got["invstd"], is_, is_ * (6 * U + rel)))
        v["scale"] = _worst(*_elem(got["scale"], sc, sc.abs() * (7 * U + rel)))
        v["shift"] = _worst(*_elem(got["shift"], ref["shift"], (mean * sc).abs() * (9 * U + rel) + U * ref["shift"].abs() + sc.abs() * dm))
        return v
    if c.kind == "apply":
        e = (2 + (d.res is not None)) * U * ref["terms"]
        if c.exact:
            res = _same(got["y"], rnd(ref["y"], c.dtype))
        else:
            res = _store(got["y"], ref["y"], e, c.dtype)
            if "y_alt" in ref:
                alt = _store(got["y"], ref["y_alt"], e, c.dtype)
                res = tuple(torch.where(alt[0] < res[0], n, o) for n, o in zip(alt, res))
        v["y"] = _worst(*res)
        if c.bits:      # against the stored y the same `got` carries
            v["bits"] = _worst(*_same(got["bits"].double(), (got["y"] > 0).double()))
        return v
    if c.kind in ("bwd", "fs"):
        n = (c.tiles if c.kind == "fs" else c.rows) + 3
        pre = {"sums": 0.0, "dbeta": d.dbeta0.double().abs(), "dgamma": d.dgamma0.double().abs()}
        for name in ("sums", "dbeta", "dgamma"):
            a1, a2 = ref["abs1"] + ref.get("edge1", 0.0), ref["abs2"] + ref.get("edge2", 0.0)
            if c.exact:
                res = _same(got[name], ref[name])
            elif name == "sums":
                res = _elem(got[name], ref[name], torch.stack([n * U * a1 + ref.get("edge1", 0.0), n * U * a2 + ref.get("edge2", 0.0)]))
            else:
                ab, ed = (a1, ref.get("edge1", 0.0)) if name == "dbeta" else (a2, ref.get("edge2", 0.0))
                res = _elem(got[name], ref[name], n * U * (ab + pre[name]) + ed)
            v[name] = _worst(*res)
        if c.dx:
            v["dx"] = _dx_check(c, d, ref, got)
        if "dym" in ref:
            v["dym"] = _worst(*_same(got["dym"], ref["dym"], ref["skip"]))
        return v
    if c.kind == "maxpool":
        v["y"] = _worst(*_same(got["y"], ref["y"]))
        v["idx"] = _worst(*_same(got["idx"].double(), ref["idx"].double()))
        v["dx"] = _worst(*(_same(got["dx"], rnd(ref["dx"], c.dtype)) if c.exact else _store(got["dx"], ref["dx"], 3 * U * ref["gabs"], c.dtype)))
        return v
    # avgpool
    HW = c.H
    if c.exact and HW & (HW - 1) == 0:
        v["y"] = _worst(*_same(got["y"], rnd(ref["y"], c.dtype)))
        v["dx"] = _worst(*_same(got["dx"], rnd(ref["dx"], c.dtype)))
    else:
        v["y"] = _worst(*_store(got["y"], ref["y"], (HW + 3) * U * ref["xabs"], c.dtype))
        v["dx"] = _worst(*_store(got["dx"], ref["dx"], 2 * U * ref["dx"].abs(), c.dtype))
    return v


def representable(c: Case, d, ref: dict) -> bool:
    """every output an exact case compares value for value is a number of its output type (but for the 2^-140 channel, whose
    point is that it is not: its float64 value must round to zero)"""
    t = lambda v: bool((rnd(v, c.dtype) == v).all())
    f = lambda v: bool((f32(v) == v).all())
    if c.kind == "apply":
        tiny = d.scale.double().abs() == TINY_SCALE
        return t(ref["y"][:, ~tiny]) and bool((rnd(ref["y"][:, tiny], c.dtype) == 0).all())
    if c.kind in ("bwd", "fs"):
        return f(ref["sums"]) and f(ref["dbeta"]) and f(ref["dgamma"]) and t(ref["g"])
    if c.kind == "maxpool":
        return t(ref["dx"]) and t(torch.nan_to_num(ref["y"], nan=0.0))
    return t(ref["y"]) and t(ref["dx"]) if c.H & (c.H - 1) == 0 else True


def mask_share(c: Case, ref: dict) -> float:
    s = ref.get("skip")
    return 0.0 if s is None else s.float().mean().item()


def rejecting(c: Case, d, mutant: str, ref=None, yard=None):
    """the outputs whose check rejects the mutated yardstick; None where the mutant changes nothing at this case"""
    if not mutant_applies(c, mutant):
        return None
    ref = ref if ref is not None else outputs(c, d, exact=True)
    yard = yard if yard is not None else outputs(c, d, exact=False)
    mut = outputs(c, d, exact=False, mutant=mutant)
    keys = [k for k in mut if isinstance(mut[k], torch.Tensor) and k in yard and k not in ("g", "skip", "terms", "abs1", "abs2", "gabs", "xabs")]
    same = all(mut[k].shape == yard[k].shape and bool(((mut[k] == yard[k]) | ((mut[k] != mut[k]) & (yard[k] != yard[k]))).all()) for k in keys)
    if same:
        return None
    return [k for k, (r, _, _) in verdict(c, d, ref, mut).items() if r > 1.0]


# ---- the case table --------------------------------------------------------------------------------------------------------------
def _cases():
    out = []
    # apply / bwd-apply loop shapes: one trip; chunk counts that do not divide 256; several trips with a ragged last one; past the
    # 2048-block cap
    small = [(37, 64, "bf16"), (37, 64, "f32"), (301, 192, "bf16"), (53, 24, "bf16"), (53, 24, "f32"), (97, 1000, "f32")]
    large = [(2 * 2048 * 2 + 2048 + 77, 2048, "bf16"), (2 * 65536 + 65536 + 5, 64, "bf16")]
    variants = [("none", True, True), ("res", True, True), ("proj", True, True), ("none", False, False)]
    for rows, C, dt in small:
        for res, relu, bits in variants:
            for exact in (True, False):
                out.append(Case("apply", f"apply-{rows}x{C}-{dt}-{res}{'-relu' if relu else ''}-{'exact' if exact else 'random'}",
                                dt, rows, C, exact, res=res, relu=relu, bits=bits))
    for rows, C, dt in large:
        out.append(Case("apply", f"apply-{rows}x{C}-{dt}-none-relu-exact", dt, rows, C, True, res="none"))
        out.append(Case("apply", f"apply-{rows}x{C}-{dt}-res-relu-exact", dt, rows, C, True, res="res"))
        out.append(Case("apply", f"apply-{rows}x{C}-{dt}-proj-relu-random", dt, rows, C, False, res="proj"))
    # backward: the reduction shapes x the three mask sources x exact / random; the (dx, dy_masked) forms rotate through them
    forms = [(True, "none"), (True, "sep"), (True, "inplace"), (False, "none"), (True, "sep"), (False, "sep"), (True, "inplace"), (False, "inplace")]
    reduce_shapes = [(144, 64, "bf16"), (144, 64, "f32"), (16 * 32 * 3 + 1, 64, "bf16"), (512 * 16 + 1024 + 513, 2048, "bf16"),
                     (16 * 3 + 5, 4096, "bf16"), (16 * 3 + 5, 2048, "f32"), (10 * 16 * 2 + 7, 192, "bf16")]
    i = 0
    for rows, C, dt in reduce_shapes:
        for mask in ("yact", "bits", "fmask"):
            for exact in (True, False):
                dx, dym = forms[i % len(forms)]
                i += 1
                out.append(Case("bwd", f"bwd-{rows}x{C}-{dt}-{mask}-{'exact' if exact else 'random'}-{'dx' if dx else 'nodx'}-{dym}",
                                dt, rows, C, exact, mask=mask, dx=dx, dym=dym))
    # the apply-loop shapes through the backward's second kernel (the recomputed mask is what the train step runs), and no mask
    for j, (rows, C, dt) in enumerate(small + large):
        dym = ("sep", "inplace", "none")[j % 3]
        out.append(Case("bwd", f"bwd-{rows}x{C}-{dt}-fmask-random-dx-{dym}", dt, rows, C, False, mask="fmask", dym=dym))
        if (rows, C, dt) in small:
            out.append(Case("bwd", f"bwd-{rows}x{C}-{dt}-fmask-exact-dx-{dym}", dt, rows, C, True, mask="fmask", dym=dym))
    out.append(Case("bwd", "bwd-37x64-bf16-none-random-dx-sep", "bf16", 37, 64, False, mask="none", dym="sep"))
    out.append(Case("bwd", "bwd-37x64-f32-none-exact-dx-none", "f32", 37, 64, True, mask="none"))
    # the walk of bn_bwd_finalize_kernel over the block partials: fp32 at C = 64 has 16 threads per chunk column, so
    # rows = (blocks - 1) * 256 + 1 gives `blocks` workgroups; exact variant only
    for blocks in (1, 63, 64, 193, 256, 257, 512):
        rows = (blocks - 1) * 256 + 1
        assert bwd_geometry(rows, 64, "f32")[3] == blocks and rows * 60 < 2 ** 24
        out.append(Case("bwd", f"bwdwalk-{blocks}blocks-{rows}x64-f32-bits-exact", "f32", rows, 64, True, mask="bits", dx=False))
    # finalize and backward_from_stats
    for tiles in (1, 2, 17, 128, 129, 300, 1568):
        for C in (64, 72, 256, 2048):
            out.append(Case("fin", f"fin-{tiles}x{C}", "f32", C=C, tiles=tiles, count=tiles * 4))
            out.append(Case("fs", f"fs-{tiles}x{C}-bf16-random", "bf16", 53, C, False, tiles=tiles))
            out.append(Case("fs", f"fs-{tiles}x{C}-{'f32' if C != 72 else 'bf16'}-exact", "f32" if C != 72 else "bf16", 53, C, True, tiles=tiles))
    for tiles, C in ((129, 2112), (392, 4096)):      # more than 32 channel columns: the two-launch form
        out.append(Case("fin", f"fin-{tiles}x{C}", "f32", C=C, tiles=tiles, count=tiles * 4))
        out.append(Case("fs", f"fs-{tiles}x{C}-bf16-exact", "bf16", 53, C, True, tiles=tiles))
        out.append(Case("fs", f"fs-{tiles}x{C}-f32-random", "f32", 53, C, False, tiles=tiles))
    out.append(Case("fin", "fin-1x64-count1", "f32", C=64, tiles=1, count=1))
    out.append(Case("fin", "fin-17x64-eval", "f32", C=64, tiles=17, count=68, training=False))
    out.append(Case("fin", "fin-300x72-eval", "f32", C=72, tiles=300, count=1200, training=False))
    out.append(Case("fin", "fin-17x64-bad", "f32", C=64, tiles=17, count=17 * 8, cond="bad"))
    out.append(Case("fin", "fin-300x72-bad", "f32", C=72, tiles=300, count=300 * 8, cond="bad"))
    # max-pool
    for N, H, W, C in ((1, 1, 1, 8), (1, 2, 3, 8), (2, 5, 9, 16), (3, 7, 7, 64), (1, 33, 6, 72), (2, 56, 56, 64)):
        for fill in ("random", "ties", "negative", "nan_first", "nan_middle", "nan_last"):
            out.append(Case("maxpool", f"maxpool-{N}x{H}x{W}x{C}-bf16-{fill}", "bf16", C=C, N=N, H=H, W=W, fill=fill,
                            exact=fill in ("ties", "negative")))
    for fill in ("random", "ties", "nan_middle"):
        out.append(Case("maxpool", f"maxpool-2x5x9x4-f32-{fill}", "f32", C=4, N=2, H=5, W=9, fill=fill, exact=fill == "ties"))
    # global avg-pool
    for HW in (1, 7, 49, 64, 196):
        for C in (8, 72, 2048):
            for N in (1, 5):
                for dt in ("bf16", "f32"):
                    out.append(Case("avgpool", f"avgpool-{N}x{HW}x{C}-{dt}-random", dt, C=C, N=N, H=HW, W=1))
                    if HW in (1, 64) and C != 2048:
                        out.append(Case("avgpool", f"avgpool-{N}x{HW}x{C}-{dt}-exact", dt, C=C, N=N, H=HW, W=1, exact=True))
    out.append(Case("avgpool", "avgpool-1025x1x2048-bf16-random", "bf16", C=2048, N=1025, H=1, W=1))      # two grid-stride trips
    assert 1025 * 2048 // 8 > 64 * 4096
    return tuple(out)


CASES = _cases()
assert len({c.name for c in CASES}) == len(CASES)
BWD_FORMS = {(c.dx, c.dym) for c in CASES if c.kind == "bwd"}
assert BWD_FORMS == {(a, b) for a in (True, False) for b in ("none", "sep", "inplace")}
