"""Float64 reference of the kernels at the two ends of the training step: csrc/loss.hip (nkb_loss_forward, nkb_loss_backward),
csrc/optim.hip (nkb_optim_step, nkb_grad_unscale_check, nkb_scaler_update, nkb_bucket_sum_bf16, nkb_segment_sumsq) and
csrc/imgprep.hip (nkb_image_prep); the fp32 yardstick (the same math in the kernels' documented operation order, one rounding per
operation: the library is built with -ffp-contract=off and fp32 divide / sqrtf round correctly, which torch's fp32 CPU arithmetic
reproduces but for its square root, taken from numpy here), the derived bounds tests/test_loss_optim_gpu.py holds the kernels to, mutants that make the yardstick wrong the way
such kernels go wrong, and the case table both test files walk.  tests/test_loss_optim_reference.py proves on the CPU that the
reference equals torch and that the checks reject every mutant.  No test lives here.

The loss follows the contract of include/nkbhip.h and csrc/loss.hip.  Where that differs from torch:
  * a batch whose rows are all ignored, or whose kept rows all carry class weight 0, gives loss 0 and factor out2[1] = 0;
    F.cross_entropy gives NaN (0 / 0);
  * a label outside [0, C) that is not ignore_index gives a NaN loss (row_state loss NaN, wsum 1, coef NaN) and a NaN dlogits row;
    torch asserts on the device;
  * focal is -alpha[y] (1 - p_y)^gamma log p_y and its 'mean' divides by the number of kept rows, not by the sum of alpha;
  * reduction 2 ('none') returns the sum in out2[0] like 'sum'; the per-row losses are the first float of each row_state entry;
  * the focal gradient term gamma p_y log p_y (1 - p_y)^(gamma - 1) is taken as its limit 0 at p_y == 1 (autograd of the literal
    expression gives inf * 0 = NaN there for 0 < gamma < 1);
  * argmax equals torch.argmax on every row (first maximum, first NaN, column 0 for a row of -inf); probs equal torch.softmax,
    NaN rows included.
CE(weight) 'mean' is the weighted mean sum(w_y nll) / sum(w_y).  Outputs: probs, argmax, the three floats (loss, wsum, coef) of each
row_state entry, out2[0..1], dlogits = gout * out2[1] * coef * (p - onehot).

Optimizer: one step of torch.optim's single-tensor Adam (L2) / AdamW / NAdam (decoupled) / RAdam (L2, decoupled; unrectified while
rho_t <= 5, i.e. steps 1..5 at beta2 0.999) / SGD (plain, momentum on a fresh buffer, dampening, Nesterov) from an arbitrary state
(w, g, m, v) at an arbitrary step number; grad_scale multiplies the gradient first; the shadow is rnd_bf16(w_new).  The step scalars
come from utils._step_scalars (host code, covered by tests/test_optim_options_cpu.py).

The bounds (derived; none is tuned on a kernel's output; U = 2^-24):
  bit-exact   against the fp32 yardstick, value for value (a NaN where the yardstick has one): every output of nkb_optim_step (only
              + - * / and sqrtf), the values and the flag of grad_unscale_check, scaler_update, both outputs of bucket_sum_bf16,
              image_prep, argmax, and dlogits against the yardstick evaluated on the forward outputs the SAME launch pair stored
              (probs, coef, out2[1]): dlogits = ((gout * out2[1]) * coef) * (p - onehot) is three roundings.  The CPU file ties each
              yardstick to the float64 reference.  Optimizer inputs keep every intermediate a normal number: v is strictly positive,
              and a separate pair of cases has v == 0, g == 0.
  exact cases CE unweighted, equal logits in a row, C and B powers of two, per-row grad_out distinct small integers: probs == 1 / C
              and dlogits == g_r / B (1 / C - onehot) value for value, which shows any lost, swapped or duplicated row or column.
              Integer segment_sumsq / bucket_sum inputs with partial sums below 2^24; unscale by a power of two.  `representable`
              (asserted on the CPU) proves each claim per case.
  probs       e = p (2 rho + (C + 3) U) + 2 A_EXP 2^-149, rho = 2 A_EXP U + 2 U max_j |x_j - max| (the subtraction's rounding enters
              the exponent; A_EXP is transformer_reference's measured allowance; (C + 3) U is the any-order bound of the row sum).
  lse         e_lse = A_LOG ulp(log se) + 1.01 (rho + (C + 3) U) + U |lse|; log p_y: e_l = e_lse + U |log p_y|.
  CE          loss_r: |w| e_l + 2 U |loss_r|; wsum and coef are copies of w.
  focal       the kernel forms pt = expf(log p_y), om = 1 - pt, f = powf(om, gamma).  The operand magnitude of om is 1, so the
              library functions and the subtraction are allowed A_POW U absolute on om and A_POW U relative on the result:
              om lies in [om - d, om + d], d = A_POW U + pt expm1(e_l), and f within the width of (.)^gamma over that interval
              plus A_POW U f_hi.  The same for gamma (.)^(gamma - 1) over [max(om - d, 2^-24), om + d] (2^-24 is the smallest
              positive 1 - pt of fp32; the guard om <= 0 -> 0 adds 0 to the interval where om - d <= 0).  loss_r and coef_r follow by
              the product rule with three roundings each.
  out2        a = sum loss_r, b = sum wsum_r: (B + 3) U sum |terms| (any order) plus the terms' own bounds; the quotient and
              the reciprocal add one rounding each.
  segment_sumsq  (len + 3) U sum x^2 (any order; the squares round once each).
  library     logf and powf have no accuracy statement on this machine; measured on an MI355X with these fp32 kernels against this
              reference (test_loss_optim_gpu.py::test_library_function_error): logf at every se the kernel forms exactly (rows of k
              equal maxima and -inf elsewhere, se = k = 1..2048), in ulps of |log se|; the focal chain on rows (0, a), a on a grid
              of 2^15 points in [-88, 0], both labels (1 - pt covers (0, 1]), gamma in {0.5, 1, 2, 5}: the smallest A for which the
              bound above holds for loss_r (powf at gamma) and for coef_r (powf at gamma - 1).  Allowance = twice the worst,
              rounded up to a power of two, as MEASURED of transformer_reference.  Unmeasured constants are NaN: every loss-value
              check then fails closed.
No element is left out of any check.
"""
import math
from dataclasses import dataclass
from types import SimpleNamespace
from typing import Optional

import numpy as np
import torch

from bn_reference import GARBAGE, INF, TINY, _elem, _store, _worst, f32, rnd
from conv_reference import U
from transformer_reference import A_EXP, ulp32

# MEASURED on one MI355X (tests/test_loss_optim_gpu.py::test_library_function_error prints them); None = not measured yet.  pow is 0:
# on the grid the derived part of the bound of loss_r alone covers the observed error, so the allowance comes from pow_m1
MEASURED = dict(log=1.843, pow=0.0, pow_m1=0.239)    # A_LOG = 4 (2 x 1.843 = 3.69), A_POW = 0.5 (2 x 0.239 = 0.48)


def allowance(*measured):
    """twice the worst measured error, rounded up to a power of two; NaN (every check that uses it fails) while unmeasured"""
    if any(m is None for m in measured):
        return float("nan")
    return 2.0 ** math.ceil(math.log2(max(2.0 * max(measured), 2.0 ** -10)))


A_LOG = allowance(MEASURED["log"])
A_POW = allowance(MEASURED["pow"], MEASURED["pow_m1"])

NAN = float("nan")
OM_MIN = 2.0 ** -24          # the smallest positive 1 - pt of fp32

LOSS_MUTANTS = ("ignored_in_normaliser", "weight_not_in_normaliser", "focal_normalised_by_alpha", "no_max_subtraction", "last_max_wins",
                "tail_dropped", "second_trip_dropped", "ld_as_C", "ldp_for_ldd", "focal_grad_without_term", "literal_inf_times_0",
                "per_row_as_scalar", "sum_divided", "reduce_drops_from_256")
OPTIM_MUTANTS = ("l2_as_decoupled", "decoupled_as_l2", "decay_after_moment", "eps_inside_sqrt", "c0_c1_swapped", "nadam_old_m",
                 "radam_always_rectified", "nesterov_old_buffer", "dampening_on_fresh", "scale_after_decay", "optim_tail_dropped",
                 "second_group_dropped", "second_trip_dropped_optim", "shadow_from_old_w", "shadow_truncated")
OTHER_MUTANTS = ("check_before_scaling", "tail_unchecked", "growth_not_held", "tracker_not_reset", "bf16_accumulation", "stride_as_n",
                 "segment_end_inclusive", "pad_rounded_up", "flip_before_pad", "channels_reversed", "std_without_255")
MUTANTS = LOSS_MUTANTS + OPTIM_MUTANTS + OTHER_MUTANTS
ROWS3 = ("loss_rows", "wsum", "coef")
REJECTED_BY = dict(
    ignored_in_normaliser=("wsum", "out0", "out1"), weight_not_in_normaliser=("wsum", "out0", "out1"),
    focal_normalised_by_alpha=("wsum", "out0", "out1"), no_max_subtraction=("probs", "loss_rows", "coef", "out0"),
    last_max_wins=("argmax",), tail_dropped=("probs", "argmax", "loss_rows", "coef", "out0", "dlogits"),
    second_trip_dropped=("probs", "argmax", "loss_rows", "coef", "out0", "dlogits"),
    ld_as_C=("probs", "argmax", "loss_rows", "coef", "out0", "dlogits"),
    ldp_for_ldd=("dlogits",), focal_grad_without_term=("coef",), literal_inf_times_0=("coef",), per_row_as_scalar=("dlogits",),
    sum_divided=("out0",), reduce_drops_from_256=("out0", "out1", "dlogits"),
    l2_as_decoupled=("w", "m", "v", "shadow"), decoupled_as_l2=("w", "m", "v", "shadow"), decay_after_moment=("w", "m", "v", "shadow"),
    eps_inside_sqrt=("w", "shadow"), c0_c1_swapped=("w", "shadow"), nadam_old_m=("w", "shadow"), radam_always_rectified=("w", "shadow"),
    nesterov_old_buffer=("w", "shadow"), dampening_on_fresh=("w", "m", "shadow"), scale_after_decay=("w", "m", "v", "shadow"),
    optim_tail_dropped=("w", "m", "v", "shadow"), second_group_dropped=("w", "m", "v", "shadow"),
    second_trip_dropped_optim=("w", "m", "v", "shadow"), shadow_from_old_w=("shadow",), shadow_truncated=("shadow",),
    check_before_scaling=("found",), tail_unchecked=("found",), growth_not_held=("scale",), tracker_not_reset=("tracker",),
    bf16_accumulation=("out", "out16"), stride_as_n=("out", "out16"), segment_end_inclusive=("out",),
    pad_rounded_up=("out",), flip_before_pad=("out",), channels_reversed=("out",), std_without_255=("out",))

VARIANTS = ("adam", "adamw", "nadam", "radam", "radam_decoupled", "sgd", "sgd_momentum_fresh", "sgd_dampening", "sgd_nesterov")
HYPER = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, momentum=0.9, dampening=0.25)


@dataclass(frozen=True)
class Case:
    kind: str                       # loss | optim | unscale | scaler | bucket | segsq | prep
    name: str
    exact: bool = False
    # loss
    B: int = 0
    C: int = 0
    focal: bool = False
    pad: tuple = (0, 0, 0)          # columns behind C in a row of logits / probs / dlogits
    weight: bool = False            # class weight / alpha present (one entry is 0)
    gamma: float = 0.0
    ignore: int = -100              # -100, or -1: the in-range class C - 1
    ignored: str = "none"           # none | some | all
    bad: str = "none"               # none | neg (a label -1) | C (a label C)
    reduction: int = 0
    per_row: bool = False
    form: str = "train"             # train | logger (target, row_state, out2 NULL) | noprobs (probs NULL with row_state)
    fill: str = "random"            # random | offset | spread | equal | ties | nan1 | nan2 | pinf | ninf | ksame | grid
    # optim / unscale / bucket
    variant: str = ""
    n: int = 0
    offset: int = 0                 # elements the fp32 operands start behind a 16-byte boundary
    shadow: str = "aligned"         # aligned | odd (off its 8-byte boundary) | none
    wd: float = 0.0
    gscale: float = 1.0
    step: int = 1
    skip: str = "none"              # none | 0 | 1
    zero_state: bool = False        # v == 0, g == 0
    scale: float = 65536.0
    bad_at: str = "none"            # unscale: none | first | mid | lastvec | lasttail | overflow
    found0: float = 0.0
    nparts: int = 1
    form3: str = "both"             # bucket: f32 | bf16 | both
    # scaler: (found_inf, tracker, interval, scale)
    scaler: tuple = ()
    # segsq
    lengths: tuple = ()
    # prep
    img: tuple = ()                 # (Bn, Hs, Ws, Ho, Wo)
    sizes: str = "random"           # random | none | one (h = w = 1) | full
    flags: str = "cycle"            # cycle (0..3) | none
    fillv: float = 0.0
    out_offset: int = 0             # floats `out` starts behind a 16-byte boundary

    @property
    def elements(self):
        return max(self.B * (self.C + max(self.pad)), self.n * max(self.nparts, 1), sum(self.lengths),
                   (self.img[0] * self.img[3] * self.img[4] * 3) if self.img else 0)

    @property
    def big(self):
        return self.elements > (1 << 20)


def S(v):
    """an fp32 scalar (what a float argument of the C ABI carries)"""
    return torch.tensor(float(v), dtype=torch.float32)


def same(got, ref):
    """value for value, a NaN exactly where the reference has one: ratio 0 or inf.  (bn_reference._same, but equal infinities are
    equal: the unscaled gradients and the scaler hold them on purpose.)"""
    got, ref = got.double(), ref.double()
    ok = (got == ref) | (torch.isnan(got) & torch.isnan(ref))
    err = torch.where(ok, torch.zeros_like(ref), torch.full_like(ref, INF))
    return err, err, torch.zeros_like(ref)


def _rsum(t, order, dim=-1):
    return t.flip(dim).sum(dim) if order == "strided" else t.sum(dim)


def _padded(t, pad, fill=GARBAGE):
    return torch.cat([t, torch.full((t.shape[0], pad), fill, dtype=t.dtype)], 1) if pad else t


# ---- the library's sizing rules ------------------------------------------------------------------------------------------------------
def optim_path(c: Case):
    """vector: fp32 operands on a 16-byte boundary and the shadow (if any) on an 8-byte one"""
    return "vector" if c.offset % 4 == 0 and c.shadow != "odd" else "scalar"


def optim_grid(c: Case):
    return max(min((c.n // 8 + 255) // 256, 2048), 1) if optim_path(c) == "vector" else min((c.n + 255) // 256, 4096)


def ignore_value(c: Case):
    return c.C - 1 if c.ignore == -1 else c.ignore


# ---- operands --------------------------------------------------------------------------------------------------------------------
def make(c: Case, seed: int = 0):
    """the stored operands of a case, on the CPU, from a seed that depends on the case's name alone"""
    gen = torch.Generator().manual_seed(seed * 1000003 + sum(ord(ch) * (i + 1) for i, ch in enumerate(c.name)) % 999983)
    randn = lambda *s: torch.randn(*s, generator=gen)
    rand = lambda *s: torch.rand(*s, generator=gen)
    rint = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=gen)
    d = SimpleNamespace()
    if c.kind == "loss":
        B, C = c.B, c.C
        if c.fill in ("equal",):
            x = rint(-3, 3, B, 1).float().expand(B, C).clone()
        elif c.fill == "ties":
            x = rint(0, 2, B, C).float()
            if C > 64:
                x[0, :] = 0.0
                x[0, C - 1], x[0, C - 65] = 2.0, 2.0            # the same lane, two trips: the earlier column wins
        elif c.fill == "ksame":                                   # row r: r + 1 zeros, -inf elsewhere: se == r + 1 exactly
            x = torch.where(torch.arange(C)[None, :] <= torch.arange(B)[:, None], 0.0, -INF)
        elif c.fill == "grid":                                    # rows (0, a)
            x = torch.stack([torch.zeros(B), torch.linspace(-88.0, 0.0, B)], 1)
        else:
            x = 2.0 * randn(B, C)
        if c.fill == "offset":
            x = x + 1e4
        if c.fill == "spread":
            x[torch.arange(B), rint(0, C - 1, B)] += 200.0
        special = dict(nan1=(NAN,), nan2=(NAN, NAN), pinf=(INF,), ninf=None)
        if c.fill in special:                                     # the odd rows stay finite
            for r in range(0, B, 2):
                if c.fill == "ninf":
                    x[r, :] = -INF
                else:
                    cols = [(1 + 5 * r) % C, (2 + 7 * r + C // 2) % C][:len(special[c.fill])]
                    x[r, cols] = special[c.fill][0]
                    if r % 4 == 0 and c.fill == "nan2":
                        x[r, :min(3, C)] = torch.tensor([0.0, NAN, NAN])[:min(3, C)]      # NaNs at columns 1 and 2
        d.x = x.float().contiguous()
        ig = ignore_value(c)
        y = rint(0, C - 1, B)
        if c.fill == "spread":                                    # the label is the dominant column in every second row: pt == 1
            y = torch.where(torch.arange(B) % 2 == 0, d.x.argmax(1), y)
        if c.fill == "ksame":
            y = torch.zeros(B, dtype=torch.int64)
        if c.fill == "grid":
            y = torch.arange(B) % 2
        if 0 <= ig < C:
            y = torch.where(y == ig, (y + 1) % C if C > 1 else y, y)
        if c.ignored == "some":
            y[torch.arange(B) % 3 == 1] = ig
            y[B - 1] = ig
        elif c.ignored == "all":
            y[:] = ig
        if c.bad != "none":
            y[0 if B < 3 else 2] = -1 if c.bad == "neg" else C
        d.target = y
        d.weight = None
        if c.weight:
            d.weight = rand(C) + 0.5
            d.weight[C // 2] = 0.0
        d.gout = rint(1, 64, B).float() if c.exact else (randn(B) if c.per_row else torch.tensor([0.75]))
        if c.exact:
            d.gout = (torch.randperm(B, generator=gen) % 64 + 1).float() if c.per_row else torch.tensor([3.0])
    elif c.kind == "optim":
        n = c.n
        d.w, d.g, d.m = randn(n), randn(n) * (0.3 / c.gscale if c.gscale != 1.0 else 0.3), 0.1 * randn(n)
        d.v = 1e-3 + 0.01 * rand(n)
        if c.zero_state:
            d.g, d.v, d.m = torch.zeros(n), torch.zeros(n), torch.zeros(n)
        if c.variant == "sgd_momentum_fresh":
            d.m = torch.zeros(n)
    elif c.kind == "unscale":
        n = c.n
        d.g = (rint(-4096, 4096, n).float() * 16.0) if c.exact else randn(n) * 100.0
        pos = dict(first=0, mid=n // 2, lastvec=max((n // 4) * 4 - 1, 0), lasttail=n - 1, overflow=n // 3)
        if c.bad_at != "none":
            d.g[pos[c.bad_at]] = 3e38 if c.bad_at == "overflow" else (INF if (n + len(c.bad_at)) % 2 else NAN)
    elif c.kind == "bucket":
        stride = -(-c.n // 8) * 8 + 8
        d.stride = stride
        v = rint(-64, 64, c.nparts, stride).float() if c.exact else randn(c.nparts, stride)
        d.parts = v.to(torch.bfloat16)
    elif c.kind == "segsq":
        off = [3]
        for i, L in enumerate(c.lengths):
            off.append(off[-1] + L)
        d.offsets = torch.tensor(off, dtype=torch.int64)
        d.x = rint(-8, 8, off[-1] + 5).float() if c.exact else randn(off[-1] + 5)
    elif c.kind == "prep":
        Bn, Hs, Ws, Ho, Wo = c.img
        d.src = rint(0, 255, Bn, Hs, Ws, 3).to(torch.uint8)
        if c.sizes == "none":
            d.sizes = None
        elif c.sizes == "one":
            d.sizes = torch.ones(Bn, 2, dtype=torch.int32)
        elif c.sizes == "full":
            d.sizes = torch.tensor([[Hs, Ws]] * Bn, dtype=torch.int32)
        else:
            d.sizes = torch.stack([rint(1, Hs, Bn), rint(1, Ws, Bn)], 1).to(torch.int32)
            d.sizes[0] = torch.tensor([max(Hs - 1, 1), max(Ws - 2, 1)])
        d.flags = None if c.flags == "none" else (torch.arange(Bn) % 4).to(torch.uint8)
        d.mean, d.std = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
    return d


# ---- the loss ----------------------------------------------------------------------------------------------------------------------
def argmax_rows(X, last=False):
    """torch.argmax per row: the first (mutant: last) NaN if the row has one, else the first maximum"""
    C = X.shape[1]
    isn = torch.isnan(X)
    mx = torch.where(isn, torch.full_like(X, -INF), X).max(1, keepdim=True).values
    hit = torch.where(isn.any(1, keepdim=True), isn, X == mx)
    idx = torch.arange(C)[None, :]
    return torch.where(hit, idx, -1).max(1).values if last else torch.where(hit, idx, C).min(1).values


def dlogits_of(c: Case, d, P, coef, out1, dt, mutant=None):
    """((gout * out2[1]) * coef) * (p - onehot) in dtype dt, from the given forward outputs"""
    B, C = c.B, c.C
    g = d.gout.to(dt)
    g = g if (c.per_row and mutant != "per_row_as_scalar") else g[:1].expand(B)
    onehot = (d.target[:, None] == torch.arange(C)[None, :]).to(dt)
    dl = ((g * out1.to(dt)) * coef.to(dt))[:, None] * (P.to(dt) - onehot)
    if mutant == "ldp_for_ldd":           # written with the stride of probs into the buffer laid out with dlogits' stride
        ldp, ldd = C + c.pad[1], C + c.pad[2]
        buf = torch.full((B * max(ldp, ldd) + C,), NAN, dtype=dt)
        buf[(torch.arange(B)[:, None] * ldp + torch.arange(C)[None, :]).reshape(-1)] = dl.reshape(-1)
        dl = buf[torch.arange(B)[:, None] * ldd + torch.arange(C)[None, :]]
    return dl


def focal_terms(q, A):
    """bounds of the focal loss_r and coef_r (float64 row quantities q) with A ulps allowed to the powf chain"""
    g, om, pt, f, lp, e_l, w = q["gamma"], q["om"], q["pt"], q["f"], q["logpt"].abs(), q["e_l"], q["w"].abs()
    dl = A * U + pt * torch.expm1(e_l)
    lo, hi = (om - dl).clamp_min(0.0), om + dl
    f_lo, f_hi = lo ** g, hi ** g
    E_f = torch.maximum(f_hi - f, f - f_lo) + A * U * f_hi
    L = lp + e_l
    e_loss = w * (E_f * L + f * e_l + 3 * U * f_hi * L)
    if g == 0.0:
        return e_loss, w * (E_f + 2 * U * f_hi)
    ga, gb = g * lo.clamp_min(OM_MIN) ** (g - 1.0), g * hi ** (g - 1.0)
    g_hi = torch.maximum(ga, gb)
    g_lo = torch.where(lo <= 0.0, torch.zeros_like(ga), torch.minimum(ga, gb))
    E_g = torch.maximum(g_hi - q["g0"], q["g0"] - g_lo) + (A + 1) * U * g_hi
    d_pt = pt * torch.expm1(e_l + A * U)
    pt_hi = pt + d_pt
    E_t = E_g * pt_hi * L + q["g0"] * (d_pt * L + pt * e_l) + 3 * U * g_hi * pt_hi * L
    return e_loss, w * (E_f + E_t + 2 * U * (f_hi + g_hi * pt_hi * L))


def _loss(c: Case, d, exact, mutant, order):
    dt = torch.float64 if exact else torch.float32
    B, C = c.B, c.C
    X = d.x.to(dt)
    if mutant == "ld_as_C":
        flat = torch.cat([_padded(d.x, c.pad[0]).reshape(-1), torch.full((C,), GARBAGE)])
        X = flat[torch.arange(B)[:, None] * C + torch.arange(C)[None, :]].to(dt)
    used = torch.ones(C, dtype=torch.bool)
    if mutant == "tail_dropped":
        used[(C // 64) * 64:] = False
    if mutant == "second_trip_dropped":
        used[64:128] = False
    Xu = torch.where(used[None, :], X, torch.full_like(X, -INF))
    out = {"argmax": argmax_rows(Xu, last=mutant == "last_max_wins").double()}
    mx = Xu.max(1).values
    sub = torch.zeros_like(mx) if mutant == "no_max_subtraction" else mx
    E = torch.where(used[None, :], torch.exp(Xu - sub[:, None]), torch.zeros_like(X))
    se = _rsum(E, order)
    lse = sub + torch.log(se)
    P = E * (1.0 / se)[:, None]
    P = torch.where(used[None, :], P, torch.full_like(P, NAN))
    if c.form != "noprobs":
        out["probs"] = P.double()
    if exact:
        diff = (X - mx[:, None]).abs()
        rho = 2 * A_EXP * U + 2 * U * torch.where(torch.isfinite(diff), diff, torch.zeros_like(diff)).max(1).values
        r_se = rho + (C + 3) * U
        out["e_probs"] = torch.nan_to_num(P, nan=0.0) * (2 * rho + (C + 3) * U)[:, None] + 2 * A_EXP * 2.0 ** -149
    if c.form == "logger":
        return out
    y = d.target
    ig = ignore_value(c)
    ign = y == ig
    badl = ~ign & ((y < 0) | (y >= C))
    ok = ~ign & ~badl
    yc = y.clamp(0, C - 1)
    logpt = X.gather(1, yc[:, None])[:, 0] - lse
    w = d.weight.to(dt)[yc] if c.weight else torch.ones(B, dtype=dt)
    one, zero = torch.ones(B, dtype=dt), torch.zeros(B, dtype=dt)
    if not c.focal:
        loss, wsum, coef = -w * logpt, w, w
        if mutant == "weight_not_in_normaliser":
            wsum = one
        if exact:
            e_lse = A_LOG * ulp32(torch.log(se)) + 1.01 * r_se + U * lse.abs()
            e_l = e_lse + U * logpt.abs()
            e_loss, e_coef = w.abs() * e_l + 2 * U * loss.abs(), zero
    else:
        gam = float(S(c.gamma))
        pt = torch.exp(logpt)
        om = 1.0 - pt
        f = torch.pow(om, gam)
        gm1 = float(S(gam) - S(1.0))
        raw = gam * torch.pow(om, gm1)
        guard = (om <= 0.0) if mutant != "literal_inf_times_0" else torch.zeros(B, dtype=torch.bool)
        fm1 = zero if gam == 0.0 else torch.where(guard, zero, raw)
        loss, wsum = (-w * f) * logpt, one
        coef = w * f if mutant == "focal_grad_without_term" else w * (f - (fm1 * pt) * logpt)
        if mutant == "focal_normalised_by_alpha":
            wsum = w
        if exact:
            e_lse = A_LOG * ulp32(torch.log(se)) + 1.01 * r_se + U * lse.abs()
            e_l = e_lse + U * logpt.abs()
            out["focal_q"] = dict(gamma=gam, om=om, pt=pt, f=f, logpt=logpt, e_l=e_l, w=w, g0=fm1)
            e_loss, e_coef = focal_terms(out["focal_q"], A_POW)
    nanv = torch.full((B,), NAN, dtype=dt)
    keepw = wsum
    loss = torch.where(ok, loss, torch.where(badl, nanv, zero))
    wsum = torch.where(ok, wsum, torch.where(badl, one, keepw if mutant == "ignored_in_normaliser" else zero))
    coef = torch.where(ok, coef, torch.where(badl, nanv, zero))
    out["loss_rows"], out["wsum"], out["coef"] = loss.double(), wsum.double(), coef.double()
    sl = slice(0, 256) if mutant == "reduce_drops_from_256" else slice(None)
    a, b = _rsum(loss[sl], order), _rsum(wsum[sl], order)
    mean = c.reduction == 0
    if mean or (mutant == "sum_divided" and c.reduction == 1):
        o0 = a / b if b > 0 else zero[0]
        o1 = (1.0 / b if b > 0 else zero[0]) if mean else one[0]
    else:
        o0, o1 = a, one[0]
    out["out0"], out["out1"] = o0.double().reshape(1), o1.double().reshape(1)
    if exact:
        e_loss = torch.where(ok, e_loss, zero)
        out["e_loss_rows"], out["e_coef"] = e_loss, torch.where(ok, e_coef, zero)
        e_a = (B + 3) * U * loss.abs().sum() + e_loss.sum()
        e_b = (B + 3) * U * wsum.abs().sum()
        if mean and b > 0:
            out["e_out0"] = (1.01 * (e_a / b + a.abs() * e_b / (b * b)) + U * (a / b).abs()).reshape(1)
            out["e_out1"] = (1.01 * e_b / (b * b) + U / b).reshape(1)
        else:
            out["e_out0"], out["e_out1"] = (zero[0] if mean else e_a).reshape(1), zero[:1]
    if c.form == "train":
        out["dlogits"] = dlogits_of(c, d, P, coef, o1, dt, mutant).double()
    return out


# ---- the optimizer -----------------------------------------------------------------------------------------------------------------
def step_scalars(c: Case):
    """(kind code, the float arguments of nkb_optim_step as Python doubles) for the case's variant at its step number"""
    from nkb_classification.utils import _step_scalars
    v = c.variant
    kind = "sgd" if v.startswith("sgd") else "radam" if v.startswith("radam") else v
    state = {"step": c.step - 1}
    kw = dict(lr=HYPER["lr"], beta1=HYPER["beta1"], beta2=HYPER["beta2"], eps=HYPER["eps"])
    if kind == "nadam":       # mu_product of the steps before this one, rounded to fp32 at every step as torch keeps it
        st = {}
        for _ in range(c.step - 1):
            _step_scalars("nadam", st, **kw)
        state = st if c.step > 1 else {}
    if kind == "sgd":
        mom = 0.0 if v == "sgd" else HYPER["momentum"]
        if v != "sgd_momentum_fresh":
            state["momentum_buffer"] = True
        kw.update(momentum=mom, dampening=HYPER["dampening"] if v == "sgd_dampening" else 0.0, nesterov=v == "sgd_nesterov")
    if v == "radam_decoupled":
        kw.update(decoupled=True)
    code, cs = _step_scalars(kind, state, **kw)
    beta1 = kw.get("momentum", 0.0) if kind == "sgd" else HYPER["beta1"]
    return code, dict(lr=HYPER["lr"], wd=c.wd, beta1=beta1, beta2=HYPER["beta2"], eps=HYPER["eps"], gs=c.gscale, c0=cs[0], c1=cs[1],
                      c2=cs[2], c3=cs[3])


def _sqrt(t):
    """the correctly rounded square root.  torch's vectorised fp32 sqrt on the CPU is not (0.7 % of the values of a uniform sample are
    one ulp off on an AVX-512 build), sqrtf of the kernels and numpy's (the hardware instruction) are."""
    return torch.from_numpy(np.sqrt(t.contiguous().numpy())) if t.dtype == torch.float32 else torch.sqrt(t)


def optim_update(kind, a, w, g, m, v, mutant=None):
    """one element-wise step in the dtype of the operands; `a` holds 0-dim tensors of that dtype.  Returns (w, m, v)."""
    one = torch.ones((), dtype=w.dtype)
    mom = kind == 3 and bool(a["beta1"] != 0) and bool(a["c0"] != 0)
    if mutant == "scale_after_decay":
        grad = g
    else:
        grad = g * a["gs"]
    if kind == 3:
        grad = grad + a["wd"] * w
        if mutant == "scale_after_decay":
            grad = grad * a["gs"]
        if mom:
            m_old = m
            m = a["beta1"] * m + a["c0"] * grad
            grad = (grad + a["beta1"] * (m_old if mutant == "nesterov_old_buffer" else m)) if bool(a["c1"] != 0) else m
        return w - a["lr"] * grad, m, v
    decoupled = kind == 1 or bool(a["c3"] != 0)
    if mutant == "l2_as_decoupled" and not decoupled:
        decoupled = True
    elif mutant == "decoupled_as_l2" and decoupled:
        decoupled = False
    late = mutant == "decay_after_moment"
    if decoupled and not late:
        w = w * (one - a["lr"] * a["wd"])
    elif not decoupled and not late:
        grad = grad + a["wd"] * w
    if mutant == "scale_after_decay":
        grad = grad * a["gs"]
    m_old = m
    m = m + (grad - m) * (one - a["beta1"])
    v = v * a["beta2"] + (one - a["beta2"]) * grad * grad
    if late and not decoupled:
        grad = grad + a["wd"] * w
    inside = mutant == "eps_inside_sqrt"
    if kind == 0:
        c0, c1 = (a["c1"], a["c0"]) if mutant == "c0_c1_swapped" else (a["c0"], a["c1"])
        denom = _sqrt(v + a["eps"]) / c1 if inside else _sqrt(v) / c1 + a["eps"]
        w = w - c0 * (m / denom)
    elif kind == 1:
        denom = _sqrt(v / a["c0"] + a["eps"]) if inside else _sqrt(v / a["c0"]) + a["eps"]
        w = w - a["c1"] * (grad / denom)
        w = w - a["c2"] * ((m_old if mutant == "nadam_old_m" else m) / denom)
    else:
        bc = m / a["c0"]
        if bool(a["c2"] > 0) or mutant == "radam_always_rectified":
            den = _sqrt(v + a["eps"]) if inside else _sqrt(v) + a["eps"]
            w = w - a["lr"] * bc * a["c2"] * (a["c1"] / den)
        else:
            w = w - a["lr"] * bc
    if late and decoupled:
        w = w * (one - a["lr"] * a["wd"])
    return w, m, v


def _truncate_bf16(t):
    return (t.float().view(torch.int32) & -65536).view(torch.float32)


def _optim(c: Case, d, exact, mutant, round_args=True):
    dt = torch.float64 if exact else torch.float32
    code, args = step_scalars(c)
    if mutant == "dampening_on_fresh":
        args["c0"] = 1.0 - HYPER["dampening"]
    a = {k: (S(v).to(dt) if round_args else torch.tensor(v, dtype=torch.float64)) for k, v in args.items()}
    w0, g, m0, v0 = d.w.to(dt), d.g.to(dt), d.m.to(dt), d.v.to(dt)
    w, m, v = optim_update(code, a, w0, g, m0, v0, mutant)
    mode = "adam" if code != 3 else ("momentum" if (args["beta1"] != 0 and args["c0"] != 0) else "plain")
    n = c.n
    i = torch.arange(n)
    keep = torch.zeros(n, dtype=torch.bool)          # elements the (mutated) launch leaves untouched
    if c.skip == "1":
        keep[:] = True
    vecp, grid = optim_path(c) == "vector", optim_grid(c)
    stride = grid * 256
    if mutant == "optim_tail_dropped" and vecp:
        keep |= i >= (n // 4) * 4
    if mutant == "second_group_dropped" and vecp:
        keep |= (i < (n // 4) * 4) & ((i // 4) % (2 * stride) >= stride)
    if mutant == "second_trip_dropped_optim":
        keep |= ((i < (n // 4) * 4) & (i // 4 >= 2 * stride)) if vecp else (i >= stride)
    w, m, v = torch.where(keep, w0, w), torch.where(keep, m0, m), torch.where(keep, v0, v)
    out = {"w": w.double(), "m": (m if mode != "plain" else m0).double(), "v": (v if mode == "adam" else v0).double()}
    if c.shadow != "none":
        src = torch.where(keep, torch.full_like(w, NAN), w0 if mutant == "shadow_from_old_w" else w)     # the shadow region starts as NaN
        out["shadow"] = (_truncate_bf16(src) if mutant == "shadow_truncated" else src if exact else rnd(src, "bf16")).double()
    out["terms"] = w0.abs().double() + 1.0
    return out


# ---- the rest ----------------------------------------------------------------------------------------------------------------------
def _unscale(c, d, exact, mutant):
    dt = torch.float64 if exact else torch.float32
    inv = (1.0 / S(c.scale).to(dt))
    g0 = d.g.to(dt)
    g = g0 * inv
    gf = g if not exact else g.float()                # the flag is decided on the fp32 value
    probe = g0.float() if mutant == "check_before_scaling" else gf
    if mutant == "tail_unchecked":
        probe = probe[:(c.n // 4) * 4]
    found = 1.0 if bool((~torch.isfinite(probe)).any()) else c.found0
    return {"g": g.double(), "found": torch.tensor([found], dtype=torch.float64)}


def scaler_step(scale, tracker, found, growth, backoff, interval, mutant=None):
    """GradScaler.update() in plain Python on fp32 values: (scale, tracker, found_inf, last_found_inf)"""
    f = np.float32
    scale = f(scale)
    if found != 0.0:
        scale, tracker = f(scale * f(backoff)), (tracker if mutant == "tracker_not_reset" else 0)
    else:
        t = tracker + 1
        if t == interval:
            with np.errstate(over="ignore"):
                ns = f(scale * f(growth))
            if np.isfinite(ns) or mutant == "growth_not_held":
                scale = ns
            tracker = 0
        else:
            tracker = t
    return float(scale), tracker, 0.0, float(found)


def _scaler(c, d, exact, mutant):
    found, tracker, interval, scale = c.scaler
    s, t, f, last = scaler_step(scale, tracker, found, 2.0, 0.5, interval, mutant)
    T = lambda v: torch.tensor([v], dtype=torch.float64)
    return {"scale": T(s), "tracker": T(t), "found": T(f), "last": T(last)}


def _bucket(c, d, exact, mutant):
    n = c.n
    parts = d.parts.float()
    if mutant == "stride_as_n":
        flat = torch.cat([parts.reshape(-1), torch.zeros(n)])
        parts = torch.stack([flat[p * n:p * n + d.stride] for p in range(c.nparts)])
    parts = parts[:, :n]
    if exact:
        acc = parts.double().sum(0)
    else:
        acc = torch.zeros(n)
        for p in range(c.nparts):
            acc = acc + parts[p]
            if mutant == "bf16_accumulation":
                acc = rnd(acc, "bf16")
    out = {}
    if c.form3 in ("f32", "both"):
        out["out"] = acc.double()
    if c.form3 in ("bf16", "both"):
        out["out16"] = (acc if exact else rnd(acc, "bf16")).double()
    out["terms"] = parts.double().abs().sum(0)
    return out


def _segsq(c, d, exact, mutant, order):
    x = d.x.double() if exact else d.x.float()
    res, ab = [], []
    for k, L in enumerate(c.lengths):
        lo, hi = int(d.offsets[k]), int(d.offsets[k + 1]) + (1 if mutant == "segment_end_inclusive" else 0)
        sq = x[lo:hi] * x[lo:hi]
        res.append(_rsum(sq, order))
        ab.append(d.x.double()[lo:hi].pow(2).sum())
    return {"out": torch.stack(res).double(), "abs": torch.stack(ab)}


def _prep(c, d, exact, mutant):
    dt = torch.float64 if exact else torch.float32
    Bn, Hs, Ws, Ho, Wo = c.img
    fill = S(c.fillv).to(dt)
    canvas = torch.empty(Bn, Ho, Wo, 3, dtype=dt)
    for b in range(Bn):
        h, w = (int(d.sizes[b, 0]), int(d.sizes[b, 1])) if d.sizes is not None else (Hs, Ws)
        up = 1 if mutant == "pad_rounded_up" else 0
        top, left = (Ho - h + up) // 2, (Wo - w + up) // 2
        fl = int(d.flags[b]) if d.flags is not None else 0
        img = d.src[b, :h, :w].to(dt)
        P = fill.expand(Ho, Wo, 3).clone()
        dims = [k for k, bit in ((1, 1), (0, 2)) if fl & bit]
        if mutant == "flip_before_pad" and dims:
            img = img.flip(dims)
        P[top:top + h, left:left + w] = img
        if mutant != "flip_before_pad" and dims:
            P = P.flip(dims)
        canvas[b] = P
    k255 = S(255.0).to(dt)
    mean, std = torch.stack([S(v) for v in d.mean]).to(dt), torch.stack([S(v) for v in d.std]).to(dt)
    m = mean * k255
    r = 1.0 / std if mutant == "std_without_255" else 1.0 / (std * k255)
    o = ((canvas - m) * r).permute(0, 3, 1, 2)
    if mutant == "channels_reversed":
        o = o.flip(1)
    return {"out": o.contiguous().double(), "terms": (canvas.abs() + m.abs()).permute(0, 3, 1, 2).double() * r.abs().double()[None, :, None, None]}


def outputs(c: Case, d, *, exact: bool, mutant: Optional[str] = None, order: Optional[str] = None):
    k = c.kind
    if k == "loss":
        return _loss(c, d, exact, mutant, order)
    if k == "optim":
        return _optim(c, d, exact, mutant)
    if k == "unscale":
        return _unscale(c, d, exact, mutant)
    if k == "scaler":
        return _scaler(c, d, exact, mutant)
    if k == "bucket":
        return _bucket(c, d, exact, mutant)
    if k == "segsq":
        return _segsq(c, d, exact, mutant, order)
    return _prep(c, d, exact, mutant)


def mutant_applies(c: Case, mutant: str) -> bool:
    k = c.kind
    loss = k == "loss" and c.fill in ("random", "offset", "spread", "equal", "ties")
    train = loss and c.form != "logger"
    clean = train and c.bad == "none"
    opt = k == "optim" and c.skip != "1" and not c.zero_state
    v = c.variant
    adamf = opt and not v.startswith("sgd")
    vec = opt and optim_path(c) == "vector"
    stride = optim_grid(c) * 256 if k == "optim" else 0
    img = c.img or (0, 0, 0, 0, 0)
    table = dict(
        ignored_in_normaliser=clean and c.ignored != "none" and c.reduction == 0,
        weight_not_in_normaliser=clean and not c.focal and c.weight and c.ignored != "all",
        focal_normalised_by_alpha=clean and c.focal and c.weight and c.ignored != "all",
        no_max_subtraction=loss and c.fill == "offset", last_max_wins=loss and c.fill in ("equal", "ties") and c.C > 1,
        tail_dropped=loss and c.C % 64 != 0, second_trip_dropped=loss and c.C > 64,
        ld_as_C=loss and c.pad[0] > 0 and c.B > 1, ldp_for_ldd=clean and c.form == "train" and c.pad[1] != c.pad[2] and c.B > 1 and c.ignored != "all",
        focal_grad_without_term=clean and c.focal and c.gamma > 0 and c.ignored != "all" and c.fill == "random" and c.C > 1,
        literal_inf_times_0=clean and c.focal and 0 < c.gamma < 1 and c.fill == "spread" and c.ignored == "none",
        per_row_as_scalar=clean and c.form == "train" and c.per_row and c.B > 1 and c.ignored != "all",
        sum_divided=clean and c.reduction == 1 and c.ignored != "all" and c.C > 1,
        reduce_drops_from_256=clean and c.B > 256 and c.ignored != "all" and c.C > 1,
        l2_as_decoupled=adamf and v in ("adam", "radam") and c.wd > 0, decoupled_as_l2=adamf and v in ("adamw", "nadam", "radam_decoupled") and c.wd > 0,
        decay_after_moment=adamf and c.wd > 0, eps_inside_sqrt=adamf and not (v.startswith("radam") and c.step <= 5),
        c0_c1_swapped=opt and v in ("adam", "adamw"), nadam_old_m=opt and v == "nadam",
        radam_always_rectified=opt and v.startswith("radam") and c.step <= 5,
        nesterov_old_buffer=opt and v == "sgd_nesterov", dampening_on_fresh=opt and v == "sgd_momentum_fresh",
        scale_after_decay=opt and c.gscale != 1.0 and c.wd > 0 and v in ("adam", "radam", "sgd", "sgd_dampening", "sgd_nesterov", "sgd_momentum_fresh"),
        optim_tail_dropped=vec and c.n % 4 != 0, second_group_dropped=vec and c.n // 4 > stride,
        second_trip_dropped_optim=opt and (c.n // 4 > 2 * stride if vec else c.n > stride),
        shadow_from_old_w=opt and c.shadow != "none", shadow_truncated=opt and c.shadow != "none",
        check_before_scaling=k == "unscale" and c.bad_at == "overflow", tail_unchecked=k == "unscale" and c.bad_at == "lasttail" and c.n % 4 != 0,
        growth_not_held=k == "scaler", tracker_not_reset=k == "scaler",
        bf16_accumulation=k == "bucket" and c.nparts > 2 and not c.exact, stride_as_n=k == "bucket" and c.nparts > 1,
        segment_end_inclusive=k == "segsq", pad_rounded_up=k == "prep" and c.sizes == "random", flip_before_pad=k == "prep" and c.sizes == "random" and c.flags != "none",
        channels_reversed=k == "prep", std_without_255=k == "prep")
    return bool(table[mutant])


# ---- the checks ------------------------------------------------------------------------------------------------------------------
BIT_EXACT = dict(optim=("w", "m", "v", "shadow"), unscale=("g", "found"), scaler=("scale", "tracker", "found", "last"),
                 bucket=("out", "out16"), prep=("out",))


def verdict(c: Case, d, ref: dict, got: dict, yard: Optional[dict] = None) -> dict:
    """{output: (worst err / bound, err, bound)} of `got` (a kernel's or a yardstick's outputs as float64 tensors); only the outputs
    `got` carries are judged"""
    v = {}
    k = c.kind
    if k in BIT_EXACT:
        yard = yard if yard is not None else outputs(c, d, exact=False)
        for name in BIT_EXACT[k]:
            if name in got and name in yard:
                v[name] = _worst(*same(got[name], yard[name]))
        return v
    if k == "segsq":
        v["out"] = _worst(*(same(got["out"], ref["out"]) if c.exact else
                            _elem(got["out"], ref["out"], (torch.tensor(c.lengths, dtype=torch.float64) + 3) * U * ref["abs"] + TINY["f32"])))
        return v
    # loss
    if "argmax" in got:
        v["argmax"] = _worst(*same(got["argmax"], ref["argmax"]))
    if "probs" in got:
        v["probs"] = _worst(*(same(got["probs"], ref["probs"]) if c.exact else _elem(got["probs"], ref["probs"], ref["e_probs"] + TINY["f32"])))
    for name in ("loss_rows", "coef", "out0", "out1"):
        if name in got:
            v[name] = _worst(*_elem(got[name], ref[name], ref["e_" + name] + TINY["f32"]))
    if "wsum" in got:
        v["wsum"] = _worst(*same(got["wsum"], ref["wsum"]))
    if "dlogits" in got:
        if c.exact:
            v["dlogits"] = _worst(*same(got["dlogits"], ref["dlogits"]))
        else:      # the yardstick on the forward outputs the same launch pair stored
            want = dlogits_of(c, d, got["probs"], got["coef"], got["out1"], torch.float32)
            v["dlogits"] = _worst(*same(got["dlogits"], want))
    return v


def yardstick_to_reference(c: Case, d, ref, yard) -> dict:
    """ties the fp32 yardstick of a bit-exact kind to the float64 reference: a few U of the operand terms and the store rounding"""
    v = {}
    k = c.kind
    if k == "optim":
        for name in ("w", "m", "v"):
            v[name] = _worst(*_elem(yard[name], ref[name], 64 * U * ref["terms"]))
        if "shadow" in ref:
            v["shadow"] = _worst(*_store(yard["shadow"], ref["shadow"], 64 * U * ref["terms"], "bf16"))
    elif k == "unscale":
        fin = torch.isfinite(ref["g"]) & torch.isfinite(yard["g"])
        v["nonfinite"] = _worst(*same(torch.isfinite(yard["g"]).double(), torch.isfinite(f32(ref["g"])).double()))
        v["g"] = _worst(*_elem(torch.where(fin, yard["g"], 0.0), torch.where(fin, ref["g"], 0.0), 3 * U * torch.where(fin, ref["g"], 0.0).abs() + TINY["f32"]))
        v["found"] = _worst(*same(yard["found"], ref["found"]))
    elif k == "bucket":
        for name in ("out", "out16"):
            if name in ref:
                v[name] = _worst(*_store(yard[name], ref[name], (c.nparts + 1) * U * ref["terms"], "bf16" if name == "out16" else "f32"))
    elif k == "prep":
        v["out"] = _worst(*_elem(yard["out"], ref["out"], 6 * U * ref["terms"] + TINY["f32"]))
    return v


def _pow2(n):
    return n > 0 and n & (n - 1) == 0


def representable(c: Case, d, ref: dict) -> bool:
    """every output an exact case compares value for value is an fp32 number and every fp32 operation behind it is exact"""
    f = lambda t: bool((f32(t) == t).all())
    if c.kind == "loss":
        ok = _pow2(c.B) and _pow2(c.C) and not c.focal and not c.weight and c.ignored == "none" and c.bad == "none" and c.reduction == 0
        ok = ok and bool((d.x == d.x[:, :1]).all()) and bool((d.gout == d.gout.round()).all()) and d.gout.abs().max().item() <= 64
        ok = ok and bool((ref["probs"] == 1.0 / c.C).all()) and f(ref["dlogits"]) and f(ref["out1"]) and ref["out1"].item() == 1.0 / c.B
        return ok and f(d.gout.double() / c.B) and (not c.per_row or c.B > 64 or d.gout.unique().numel() == c.B)
    if c.kind == "segsq":
        x = d.x.double()
        return bool((x == x.round()).all()) and ref["abs"].max().item() < 2.0 ** 24 and f(ref["out"])
    if c.kind == "bucket":
        p = d.parts.double()
        return bool((p == p.round()).all()) and ref["terms"].max().item() < 2.0 ** 24 and ("out" not in ref or f(ref["out"]))
    if c.kind == "unscale":
        return _pow2(int(c.scale)) and f(ref["g"])
    return True


def rejecting(c: Case, d, mutant: str, ref=None, yard=None):
    """the outputs whose check rejects the mutated yardstick; None where the mutant changes nothing at this case"""
    if not mutant_applies(c, mutant):
        return None
    ref = ref if ref is not None else outputs(c, d, exact=True)
    yard = yard if yard is not None else outputs(c, d, exact=False)
    mut = outputs(c, d, exact=False, mutant=mutant)
    keys = [k for k in mut if isinstance(mut[k], torch.Tensor) and k in yard and not k.startswith(("abs", "terms", "e_"))]
    if all(mut[k].shape == yard[k].shape and bool(((mut[k] == yard[k]) | ((mut[k] != mut[k]) & (yard[k] != yard[k]))).all()) for k in keys):
        return None
    if c.kind == "loss" and not c.exact and "dlogits" in mut and mutant not in ("ldp_for_ldd", "per_row_as_scalar"):
        # a kernel with this fault feeds its own wrong forward outputs to a correct backward
        mut["dlogits"] = dlogits_of(c, d, mut["probs"], mut["coef"], mut["out1"], torch.float32).double()
    return [k for k, (r, _, _) in verdict(c, d, ref, mut, yard).items() if not r <= 1.0]


# ---- the case table --------------------------------------------------------------------------------------------------------------
LOSS_C = (1, 2, 3, 63, 64, 65, 130, 1000)
LOSS_B = (1, 3, 4, 5, 9, 257, 600)
LOSS_PADS = ((0, 0, 0), (3, 5, 7), (9, 1, 4))
GAMMAS = (0.0, 0.5, 1.0, 2.0, 5.0)
IGNORES = ((-100, "none"), (-100, "some"), (-1, "none"), (-1, "some"), (-100, "all"), (-1, "all"))
OPTIM_N = (1, 3, 4, 5, 8, 2047, 10007)
OPTIM_BIG = 4 * (3 * 2048 * 256 + 1000) + 3          # the second grid trip with and without its second group, plus a tail
UNSCALE_BIG = 4096 * 256 * 4 + 4 * 300 + 3
BUCKET_BIG = 4096 * 256 * 8 + 8 * 100 + 5


def _loss_name(c):
    return (f"loss-{'focal%g' % c['gamma'] if c['focal'] else 'ce'}-{c['B']}x{c['C']}-pad{'.'.join(map(str, c['pad']))}"
            f"{'-w' if c['weight'] else ''}-ig{c['ignore']}{c['ignored']}-{c['bad']}-red{c['reduction']}{'-perrow' if c['per_row'] else ''}"
            f"-{c['form']}-{c['fill']}{'-exact' if c.get('exact') else ''}")


def _loss_case(**kw):
    base = dict(B=1, C=1, focal=False, pad=(0, 0, 0), weight=False, gamma=0.0, ignore=-100, ignored="none", bad="none", reduction=0,
                per_row=False, form="train", fill="random")
    base.update(kw)
    return Case("loss", _loss_name(base), **base)


def _cases():
    out = []
    i = 0
    for C in LOSS_C:
        for B in LOSS_B:
            ig, igd = IGNORES[(i // 2) % 6]
            if B == 1 and igd == "some":
                igd = "none"
            out.append(_loss_case(B=B, C=C, focal=i % 2 == 1, gamma=GAMMAS[(i // 2) % 5] if i % 2 else 0.0, pad=LOSS_PADS[i % 3],
                                  weight=(i // 3) % 2 == 1, ignore=ig, ignored=igd, bad=("none", "none", "none", "neg", "none", "C", "none")[i % 7],
                                  reduction=(i // 2) % 3, per_row=(i // 4) % 2 == 1))
            i += 1
        i += 1
    for j, (B, C) in enumerate(((5, 3), (9, 65), (257, 130), (4, 1000))):
        for focal in (False, True):
            g = GAMMAS[1 + (j % 4)] if focal else 0.0
            out.append(_loss_case(B=B, C=C, focal=focal, gamma=g, pad=LOSS_PADS[1], fill="offset", weight=focal))
            out.append(_loss_case(B=B, C=C, focal=focal, gamma=0.5 if focal else 0.0, pad=LOSS_PADS[2], fill="spread", per_row=True))
            out.append(_loss_case(B=B, C=C, focal=focal, gamma=g, pad=LOSS_PADS[j % 3], form="noprobs", reduction=j % 3, weight=not focal,
                                  ignored="some"))
        out.append(_loss_case(B=B, C=C, focal=True, gamma=2.0, fill="spread", reduction=1))
        for fill in ("random", "ties", "equal", "nan1", "nan2", "pinf", "ninf"):
            out.append(_loss_case(B=B, C=C, pad=LOSS_PADS[(j + 1) % 3], form="logger", fill=fill))
        out.append(_loss_case(B=B, C=C, pad=LOSS_PADS[1], fill="ties", reduction=2))
    for B, C in ((1, 1), (4, 2), (8, 64), (512, 128), (2, 1024)):
        for per_row in (False, True):
            out.append(_loss_case(B=B, C=C, pad=LOSS_PADS[1 + (B % 2)], fill="equal", per_row=per_row, exact=True))
    # the optimizer
    i = 0
    for v in VARIANTS:
        for n in OPTIM_N + (OPTIM_BIG, OPTIM_BIG):
            big = n == OPTIM_BIG
            scalar_big = big and i % 2 == 1
            shadow = ("aligned", "odd", "none", "aligned")[i % 4]
            offset = (0, 1)[(i // 2) % 2]
            if big:
                offset, shadow = (1, "aligned") if scalar_big else (0, ("aligned", "none")[(i // 2) % 2])
            c = Case("optim", "", variant=v, n=n, offset=offset, shadow=shadow, wd=(0.0, 0.05)[(i + i // 3) % 2], gscale=(1.0, 0.25, 1.0 / 3.0)[i % 3],
                     step=(1, 5, 6, 100)[(i + i // 4) % 4], skip=("none", "0", "none", "1", "0")[i % 5])
            out.append(Case(**{**c.__dict__, "name": f"optim-{v}-n{n}-off{c.offset}-shadow_{c.shadow}-wd{c.wd}-gs{c.gscale:.3g}-step{c.step}-skip_{c.skip}"}))
            i += 1
        for zs in (0, 1):
            if v in ("adam", "radam"):
                out.append(Case("optim", f"optim-{v}-n1029-zero-state-{'vector' if zs else 'scalar'}", variant=v, n=1029, offset=1 - zs, zero_state=True, step=6,
                                wd=0.05))
    # grad_unscale_check
    i = 0
    for n in (1, 3, 4, 5, 1027, UNSCALE_BIG):
        for bad_at in ("none", "none", "first", "mid", "lastvec", "lasttail"):
            scale = (65536.0, 3.0)[i % 2]
            found0 = 1.0 if (bad_at == "none" and i % 2 == 1) or i % 5 == 4 else 0.0
            i += 1
            if n == UNSCALE_BIG and bad_at in ("first", "mid"):
                continue
            out.append(Case("unscale", f"unscale-n{n}-scale{scale:g}-{bad_at}-found{found0:g}-{i}", n=n, scale=scale, bad_at=bad_at, found0=found0,
                            exact=scale == 65536.0 and bad_at == "none"))
    for n in (5, 1027):
        out.append(Case("unscale", f"unscale-n{n}-scale0.0625-overflow", n=n, scale=0.0625, bad_at="overflow"))
    # scaler_update: found_inf x (tracker + 1 below / at the interval) x (growth finite / overflowing)
    for found in (0.0, 1.0):
        for tracker, interval in ((0, 3), (2, 3), (0, 1), (5, 3)):
            for scale in (65536.0, 3e38):
                out.append(Case("scaler", f"scaler-found{found:g}-tracker{tracker}of{interval}-scale{scale:g}", scaler=(found, tracker, interval, scale)))
    # bucket_sum_bf16
    i = 0
    for nparts in (1, 2, 3, 8):
        for n in (1, 7, 8, 9, 1003):
            out.append(Case("bucket", f"bucket-{nparts}x{n}-{('f32', 'bf16', 'both')[i % 3]}-{'exact' if i % 2 else 'random'}", n=n, nparts=nparts,
                            form3=("f32", "bf16", "both")[i % 3], exact=i % 2 == 1))
            i += 1
    out.append(Case("bucket", f"bucket-2x{BUCKET_BIG}-both-random", n=BUCKET_BIG, nparts=2))
    # segment_sumsq
    L = (0, 1, 63, 64, 255, 256, 257, 5000)
    out.append(Case("segsq", "segsq-random", lengths=L))
    out.append(Case("segsq", "segsq-exact", lengths=L[::-1], exact=True))
    out.append(Case("segsq", "segsq-one-empty", lengths=(0,)))
    # image_prep
    i = 0
    for Wo in (8, 9, 10, 11):
        for Hs, Ws, Ho in ((5, 6, 8), (8, Wo, 8), (4, 3, 9)):
            for sizes in ("random", "none", "one", "full"):
                Wsrc = min(Ws, Wo)
                c = dict(img=(5, Hs, Wsrc, Ho, Wo), sizes=sizes, flags=("cycle", "cycle", "none")[i % 3], fillv=(0.0, 114.0)[i % 2],
                         out_offset=(0, 1, 0, 2)[i % 4] if Wo == 8 else (0, 1)[i % 2])
                out.append(Case("prep", f"prep-5x{Hs}x{Wsrc}-to-{Ho}x{Wo}-{sizes}-flags_{c['flags']}-fill{c['fillv']:g}-off{c['out_offset']}", **c))
                i += 1
    out.append(Case("prep", "prep-33x8x8-to-256x1024-random-2trips", img=(33, 8, 8, 256, 1024), fillv=114.0))
    out.append(Case("prep", "prep-33x8x8-to-256x1022-random-2trips", img=(33, 8, 8, 256, 1022), fillv=114.0))
    return tuple(out)


CASES = _cases()
assert len({c.name for c in CASES}) == len(CASES)
