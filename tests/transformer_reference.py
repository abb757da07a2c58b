"""Float64 reference of the row kernels of csrc/transformer.hip (nkb_layernorm with nkb_layernorm_param_reduce, nkb_gelu,
nkb_gelu_fwd_dgelu, nkb_relu6, nkb_scale_rows, nkb_attn_softmax, nkb_head_transpose, nkb_vit_assemble, nkb_colsum2d, nkb_dropout),
the fp32 yardstick (the same math in the kernels' documented order with their rounding places; the library is built with
-ffp-contract=off, so a multiply and an add round separately, which torch's fp32 CPU arithmetic reproduces), the derived bounds that
tests/test_transformer_ops_gpu.py holds the kernels to, mutants that make the yardstick wrong the way these kernels go wrong, and
the case table both test files walk.  tests/test_transformer_reference.py proves on the CPU that the reference equals torch's
layer_norm / gelu / relu6 / softmax and their autograd in float64 and that the checks reject every mutant.  No test lives here.

The operations, float64 from the same stored (rounded) operands (rnd = the store rounding of the compute dtype):
  ln forward    mean = sum_D x / D, var = sum_D (x - mean)^2 / D (biased, two passes), rstd = 1 / sqrt(var + eps),
                y = (x - mean) rstd gamma + beta.
  ln backward   from the mean / rstd the caller supplies: xhat = (x - mean) rstd, dgamma += sum_rows dy xhat, dbeta += sum_rows dy,
                g = dy gamma, c1 = mean_D g, c2 = mean_D (g xhat), dx = rstd (g - c1 - xhat c2) (+ add; add is read with the OUTPUT
                stride).  Second outputs, from the STORED row: the row-scaled copy rnd(rnd(dx) row_scale[row / rows_per_sample]); the
                fp8 bytes / amax of (row_scale) rnd(dx) and colsum += their column sums (forward: the fp8 bytes / amax of rnd(y)).
  gelu          y = x Phi(x), Phi = (1 + erf(x / sqrt 2)) / 2; dx = dy (Phi + x phi(x)), phi = exp(-x^2 / 2) / sqrt(2 pi).
  quick_gelu    s = 1 / (1 + exp(-1.702 x)), y = x s; dx = dy (s + 1.702 y (1 - s)).   The forward-keeping-derivative form writes
                y and the derivative itself (the derivative possibly over x).
  relu6         y = min(max(x, 0), 6); dx = dy where 0 < x < 6 (strict at both ends), 0 elsewhere.
  scale_rows    out[b][i] = x[b][i] scale[b] (+ add[b][i]).
  softmax       forward p = softmax(scale s) over the first `cols` of a row of lds floats, written to ldp columns, zero from cols on;
                backward ds = scale p (dp - sum_cols dp p) with p the stored probabilities, zero from cols on.
  transpose     out[z][d][t] = in[zo sio + zi sii + t ld_in + d] for t < T, 0 for T <= t < ldt, z = zo inner + zi.
  assemble      x[b][0] = cls + pos[0], x[b][1 + p] = tok[b][p] + pos[1 + p] (cls == NULL: x[b][t] = tok[b][t] + pos[t]); backward:
                d_tok[b][p] = g[b][1 + p].
  colsum        out[c] += sum_rows x[r][c] (leading dimension ld).
  dropout       keep_i = hash(seed, i) >= thresh(p) (mix32 / dropout_thresh / dropout_hi_term / dropout_hash / dropout_keep of
                csrc/common.h, restated here on integers), out = keep ? in / (1 - p) : 0 (+ add), mask byte = keep; the backward
                applies the stored mask.  Indices at or above 2^32 (where the high index word enters the hash) are out of reach at
                test size: the twin is compared with the C++ functions there, the kernel is not.

The bounds (derived; none is tuned on a kernel's output; U = 2^-24, R_BF16 = 2^-8):
  bit-exact   one or two fp32 operations and one store rounding, which the fp32 yardstick reproduces value for value: relu6 forward
              and backward, scale_rows, assemble (forward one addition, backward a copy), transpose (a copy plus zeros), the dropout
              mask against the host twin, dropout forward and backward (scale = 1 / (1 - p) formed in fp32, in scale, then + add),
              the scaled copy against rnd(fp32(stored dx x row_scale)).  The comparison target is the yardstick; the CPU file ties the
              yardstick to the float64 reference within 3 U of the operand terms.
  exact cases carry the precision of the reductions and are the checks that see a lost, duplicated or misrouted row or column.
              ln backward: dy integers in [-3, 3], x integers in [-8, 8], the supplied mean integers in [-2, 2], rstd and gamma in
              {0.5, 1, 2}; a dgamma term is a multiple of 0.5 of magnitude <= 60, and rows * 60 + |prefill| < 2^24 * 0.5 keeps every
              partial sum representable, so every fp32 sum is exact in any order; dgamma / dbeta (accumulated into integer prefills)
              equal the reference value for value at every width and parameter-gradient form.  dx is exact where D is a power of
              two: c1 and c2 are then exact quotients, xhat c2 a multiple of 2^-3 / D below 2^24 of them (D <= 512), and
              `representable` checks every intermediate of the documented expression per case.  colsum: integers, integer prefill.
              softmax forward: a row of equal scores (also scale s = 1e4) with cols a power of two is exactly 1 / cols.  ln forward:
              integer rows at D a power of two give mean exactly.  `representable` (asserted on the CPU) proves the claim per case.
  stores      |got - ref| <= r (|ref| + e) + e + t, r = R_BF16 for a bf16 store and 0 for fp32, e = n U sum |operand terms| with n
              counted from the documented expression, t = 2^-134 (bf16) / 2^-150 (fp32).
              ln mean: (D + 1) U sum |x| / D (D - 1 additions, the division) =: dmu.  ln rstd: rstd (6 U + dvar / (2 (var + eps)))
              (the division by D, + eps, sqrtf and the division at one ulp = 2 U each), dvar = dmu^2 + (D + 6) U (var + dmu^2):
              sum (x - mean) = 0, so an error of the mean enters the two-pass variance only squared.  ln y: 4 U (|(x - mean) rstd
              gamma| + |beta|) + |gamma| (rstd dmu + |x - mean| drstd).
  ln dx       the three-term form of bn_reference / test_stem_tail_gpu.py with c1, c2 rebuilt in float64: r |ref| + 2^-20 (|rstd g| +
              |rstd c1| + |rstd xhat c2| + |add|) + rstd (D + 3) U (mean_D |g| + |xhat| mean_D |g xhat|) + t.  The last term is the
              any-order bound of the two wave sums: there they are the library's own outputs and held separately, here they are
              internal, so their allowance enters the element that consumes them.
  reductions  dgamma, dbeta, colsum of random cases: (rows + 3) U (sum |terms| + |prefill|) per column, valid for ANY order.  It is
              deliberately loose; the exact cases carry the precision.  The atomic forms are held to the same bound on both launches
              (their order is not fixed); every other form must repeat bit for bit.  The column sums of the fp8 form are compared
              with the float64 sums of the library's own stored dx (x row_scale).
  library     erff / expf have no accuracy statement on this machine (no document of the device library ships with it), so the
              allowance was measured on an MI355X with the fp32 kernels, as twice the worst error rounded up to a power of two, in
              ulps of the magnitude M of the operand terms:
                gelu forward    M = |x| (1 + |erf|) / 2 (= |ref| for x >= 0; for x < 0 the sum 1 + erf cancels and the error stays
                                at the scale of the terms: in ulps of |ref| itself the fp32 kernel is unbounded there, e.g. x = -6
                                stores -0 where the reference is -5.9e-9)
                gelu derivative M = (1 + |erf|) / 2 + |x| phi(x)
                exponent        softmax of the row (0, a), a on a uniform grid of 2^16 points in [-88, 0]: M = |ref|
              over all finite bf16 bit patterns with |x| <= 16 as inputs (gelu).  Measured: gelu forward 1.350, gelu derivative
              1.167, exponent 2.418 ulps (the last includes the two roundings of the normalisation); allowances A_GELU_FWD = 4,
              A_GELU_DER = 4, A_EXP = 8 (MEASURED and the constants below).  In ulps of |ref| itself the gelu forward measures
              1.7e7, which is why M is not |ref|.
              gelu e = A ulp(M); quick_gelu e = |terms| (2 A_EXP U + 4 U |1.702 x| + 10 U) (the exponent's argument carries the
              rounding of 1.702 x; the bf16 form uses the hardware exp2 / rcp at one ulp each and a rounded constant); softmax
              forward e = |ref| (2 rho + (cols + 3) U), rho = 2 A_EXP U + 2 U max_row |scale s|; backward e = (cols + 4) U |scale p|
              (|dp| + sum |dp p|).  A bf16 store adds its rounding r to these; nothing here is rtol 2e-2.
(Noted, not acted on: the VW = 2 instances with an even NP cannot be reached through nkb_layernorm, any D with D % 256 == 0 takes
VW = 4.)  No element is left out of any check.  Inputs hold no value at a ReLU6 edge but the deliberate 0, -0, 6, their neighbours and 7.
"""
import math
from dataclasses import dataclass
from types import SimpleNamespace
from typing import Optional

import torch

from bn_reference import GARBAGE, INF, TINY, _elem, _same, _store, _worst, f32, rnd
from conv_reference import R_BF16, TORCH_DT, U

# MEASURED on one MI355X (tests/test_transformer_ops_gpu.py::test_library_function_error prints them): the worst error of the fp32
# kernels in ulps of M as defined above, and the allowance = twice that, rounded up to a power of two
MEASURED = dict(gelu_fwd=1.350, gelu_der=1.167, exp=2.418)
A_GELU_FWD = 4.0        # 2 x 1.350 = 2.70
A_GELU_DER = 4.0        # 2 x 1.167 = 2.33
A_EXP = 8.0             # 2 x 2.418 = 4.84

QA = 1.702
LN_SLICES = 16
M32 = 0xFFFFFFFF

MUTANTS = ("tail_padded_width", "unbiased_variance", "tail_reads_pad", "eps_outside_sqrt", "single_pass_variance",
           "dgamma_from_dy_gamma", "dx_without_c2", "add_input_stride", "drop_last_row", "drop_second_row", "dup_row",
           "drop_last_slice", "final_assigns", "colsum_prerounding", "row_scale_by_row",
           "tanh_gelu", "der_const_sqrt_pi", "quick_1p7", "relu6_inclusive",
           "no_max_subtraction", "scale_after_max", "pad_not_zeroed", "dot_over_ldp", "bwd_no_scale",
           "not_transposed", "transpose_pad_not_zeroed", "cls_takes_pos1", "bwd_keeps_cls_row", "colsum_drop_last_block",
           "thresh_gt", "seed_words_swapped", "add_dropped_with_element")
# the outputs whose check rejects each mutant (tests/test_transformer_reference.py asserts exactly this)
REJECTED_BY = dict(
    tail_padded_width=("mean", "rstd", "y"), unbiased_variance=("rstd", "y"), tail_reads_pad=("mean", "rstd", "y"),
    eps_outside_sqrt=("rstd", "y"), single_pass_variance=("rstd", "y"), dgamma_from_dy_gamma=("dgamma",), dx_without_c2=("dx",),
    add_input_stride=("dx",), drop_last_row=("dgamma", "dbeta", "dx", "y", "colsum", "copy"), drop_second_row=("dgamma", "dbeta", "colsum"),
    dup_row=("dgamma", "dbeta", "colsum"), drop_last_slice=("dgamma", "dbeta", "colsum"), final_assigns=("dgamma", "dbeta", "colsum"),
    colsum_prerounding=("colsum",), row_scale_by_row=("copy", "colsum"),
    tanh_gelu=("y", "dx", "gp"), der_const_sqrt_pi=("dx", "gp"), quick_1p7=("y", "dx", "gp"), relu6_inclusive=("dx",),
    no_max_subtraction=("p",), scale_after_max=("p",), pad_not_zeroed=("p", "ds"), dot_over_ldp=("ds",), bwd_no_scale=("ds",),
    not_transposed=("out",), transpose_pad_not_zeroed=("out",), cls_takes_pos1=("x",), bwd_keeps_cls_row=("dtok",),
    colsum_drop_last_block=("out",), thresh_gt=("mask", "out", "dx"), seed_words_swapped=("mask", "out", "dx"),
    add_dropped_with_element=("out", "dx"))
# mutants of a formula: also random cases must reject them (row mutants hide inside the loose reduction bound there)
FORMULA_MUTANTS = ("tail_padded_width", "unbiased_variance", "tail_reads_pad", "eps_outside_sqrt", "single_pass_variance",
                   "relu6_inclusive", "thresh_gt", "dgamma_from_dy_gamma", "dx_without_c2",
                   "add_input_stride", "colsum_prerounding", "row_scale_by_row", "tanh_gelu", "der_const_sqrt_pi", "quick_1p7",
                   "scale_after_max", "pad_not_zeroed", "dot_over_ldp", "bwd_no_scale", "not_transposed",
                   "transpose_pad_not_zeroed", "cls_takes_pos1", "bwd_keeps_cls_row", "seed_words_swapped",
                   "add_dropped_with_element")


@dataclass(frozen=True)
class Case:
    kind: str                       # ln | act | scale | softmax | transpose | assemble | colsum | dropout
    name: str
    dtype: str = "bf16"
    rows: int = 0
    D: int = 0                      # ln width | softmax cols | transpose dh | assemble D | colsum C | scale inner | act / dropout n
    exact: bool = False
    # ln
    add: bool = False
    pad: tuple = (0, 0, 0)          # elements behind D in a row of x / dy / out (add shares out's)
    second: str = "none"            # none | e4m3 | e5m2 | scaled
    row_scale: bool = False
    rps: int = 0
    stats: bool = True              # forward writes mean / rstd
    cond: str = "normal"            # normal | bad (mean 100, std 0.1) | small (std 2^-9)
    # act
    op: str = ""                    # gelu | quick_gelu | relu6
    fill: str = "random"            # act: sweep | grid | random; softmax: random | equal | equal_large
    # softmax / transpose / assemble / colsum / dropout
    ld: int = 0                     # softmax ldp | transpose ldt | colsum ld
    lds: int = 0
    scale: float = 1.0
    T: int = 0                      # transpose T | assemble Tn
    outer: int = 1
    inner: int = 1
    which: int = 0                  # transpose: 0 q, 1 k, 2 v of a fused qkv row; -1 a plain [z][T][dh] source
    cls: bool = True
    offset: int = 0                 # assemble: elements the tok view is shifted by (4 = 8 bytes in bf16)
    form: str = "atomic"            # colsum: atomic | work
    p: float = 0.0
    seed: int = 0
    alias: str = "none"             # dropout: none | in | add (out == in, out == add)

    @property
    def elements(self):
        k = self.kind
        if k == "ln":
            return self.rows * (self.D + max(self.pad))
        if k in ("act", "dropout"):
            return self.D
        if k == "softmax":
            return self.rows * max(self.ld, self.lds)
        if k == "transpose":
            return self.outer * self.inner * max(self.T, self.ld) * self.D * (3 if self.which >= 0 else 1)
        if k == "assemble":
            return self.rows * self.T * self.D
        if k == "colsum":
            return self.rows * self.ld
        return self.rows * self.D

    @property
    def big(self):
        return self.elements > (1 << 21)


# ---- the library's sizing rules ------------------------------------------------------------------------------------------------------
def vec(dtype):
    return 8 if dtype == "bf16" else 4


def ln_full_lanes(D):
    return D % 128 == 0 and 128 <= D <= (2048 if D % 256 == 0 else 1024)


def ln_form(D):
    """(tail, VW, NP) of nkb_layernorm at width D"""
    tail = not ln_full_lanes(D)
    vw = 4 if tail or D % 256 == 0 else 2
    return tail, vw, (-(-D // 256) if tail else D // (64 * vw))


def ln_bwd_blocks(rows, workspace=True):
    """partial rows (= workgroups) of a backward launch"""
    g = (rows + 3) // 4
    return max(min(g, (rows + 43) // 44, 1024), 1) if workspace else min(g, 512)


def ln_fwd_blocks(rows, fp8=False):
    return min((rows + 3) // 4, 1024 if fp8 else 4096)


def ln_ws_floats(D):
    """nkb_layernorm_workspace_floats"""
    return 2048 * 2 * D


def colsum_splits(rows):
    return max(min((rows + 255) // 256, 256), 1)


def ulp32(v):
    """the fp32 ulp at the magnitude of v (float64 tensor), the subnormal spacing below 2^-126"""
    e = torch.floor(torch.log2(v.abs().clamp_min(2.0 ** -126)))
    return torch.exp2(e - 23)


# ---- the dropout generator of csrc/common.h on integers (int64 tensors holding 32-bit words) ------------------------------------------
def mix32(h):
    h = h ^ (h >> 16)
    h = (h * 0x7feb352d) & M32
    h = h ^ (h >> 15)
    h = (h * 0x846ca68b) & M32          # (the int64 product wraps; its low 32 bits are those of the unsigned product)
    return h ^ (h >> 16)


def dropout_thresh(p):
    v = float(torch.tensor(p, dtype=torch.float32).double()) * 4294967296.0
    return int(4294967295.0 if v > 4294967295.0 else v)


def dropout_hi_term(i_hi, seed_hi):
    return (i_hi * 0x9e3779b9 + seed_hi) & M32


def dropout_hash(i_lo, hi_term, seed_lo):
    return mix32((mix32(i_lo ^ seed_lo) + hi_term) & M32)


def dropout_keep(i, seed, p, mutant=None):
    """i: int64 tensor of element indices (below 2^63); the keep decisions as a bool tensor"""
    lo, hi = seed & M32, (seed >> 32) & M32
    if mutant == "seed_words_swapped":
        lo, hi = hi, lo
    h = dropout_hash(i & M32, dropout_hi_term((i >> 32) & M32, hi), lo)
    return (h > dropout_thresh(p)) if mutant == "thresh_gt" else (h >= dropout_thresh(p))


def _unmix32(h):
    """the inverse of mix32 on a Python integer"""
    h ^= h >> 16
    h = (h * pow(0x846ca68b, -1, 1 << 32)) & M32
    h ^= (h >> 15) ^ (h >> 30)
    h = (h * pow(0x7feb352d, -1, 1 << 32)) & M32
    return h ^ (h >> 16)


def seed_hitting(i, p, seed_hi):
    """the seed (with the given high word) under which element i hashes to exactly thresh(p): the one element at which `>=` and
    `>` differ, which random seeds meet once in 2^32 elements"""
    lo = _unmix32((_unmix32(dropout_thresh(p)) - dropout_hi_term(i >> 32, seed_hi)) & M32) ^ (i & M32)
    return (seed_hi << 32) | lo


# ---- operands --------------------------------------------------------------------------------------------------------------------
def bf16_sweep():
    """all finite bf16 values with |x| <= 16 (both zeros included), as a float32 tensor padded with zeros to a multiple of 8"""
    bits = torch.arange(0, 1 << 16, dtype=torch.int32)
    v = (bits << 16).view(torch.float32)
    v = v[torch.isfinite(v) & (v.abs() <= 16.0)]
    return torch.cat([v, torch.zeros(-v.numel() % 8)])


EDGES = (0.0, -0.0, 6.0, 7.0)


def _edge_values(dtype):
    """0, -0, 6, their neighbours in the dtype, and 7"""
    out = []
    for e in (0.0, 6.0):
        t = torch.tensor([e], dtype=TORCH_DT[dtype])
        i = t.view(torch.int16 if dtype == "bf16" else torch.int32)
        out += [t.float(), (i + 1).view(t.dtype).float(), -((i + 1).view(t.dtype).float()) if e == 0.0 else (i - 1).view(t.dtype).float()]
    return torch.cat(out + [torch.tensor([-0.0, 7.0])])


def make(c: Case, device, seed: int = 0):
    """the stored operands of a case, on `device`; generated on the CPU from a seed that depends on the case's name alone"""
    gen = torch.Generator().manual_seed(seed * 1000003 + sum(ord(ch) * (i + 1) for i, ch in enumerate(c.name)) % 999983)
    dt = TORCH_DT[c.dtype]
    randn = lambda *s: torch.randn(*s, generator=gen)
    rand = lambda *s: torch.rand(*s, generator=gen)
    rint = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=gen).float()
    pick = lambda vals, *s: torch.tensor(vals)[torch.randint(0, len(vals), s, generator=gen)]
    d = SimpleNamespace()
    rows, D = c.rows, c.D
    if c.kind == "ln":
        d.eps = torch.tensor(1e-6).item()           # the fp32 value the kernel receives
        if c.exact:
            d.x, d.dy, d.addv = rint(-8, 8, rows, D), rint(-3, 3, rows, D), rint(-4, 4, rows, D)
            d.gamma, d.beta = pick([0.5, 1.0, 2.0], D), rint(-4, 4, D)
            d.bmean, d.brstd = rint(-2, 2, rows), pick([0.5, 1.0, 2.0], rows)
            d.dgamma0, d.dbeta0, d.colsum0 = rint(-5, 5, D), rint(-5, 5, D), rint(-5, 5, D)
        else:
            m, s = dict(normal=(0.3, 2.0), bad=(100.0, 0.1), small=(0.0, 2.0 ** -9))[c.cond]
            d.x = ((m + s * randn(rows, D)) * (rand(rows, 1) + 0.5)).to(dt).float()
            d.dy, d.addv = 0.5 * randn(rows, D), 0.5 * randn(rows, D)
            d.gamma, d.beta = rand(D) + 0.5, 0.1 * randn(D)
            x64 = d.x.double()
            mu = x64.mean(1)
            d.bmean = mu.float()
            d.brstd = (1.0 / torch.sqrt(((x64 - mu[:, None]) ** 2).mean(1) + d.eps)).float()
            d.dgamma0, d.dbeta0, d.colsum0 = randn(D), randn(D), randn(D)
        d.x, d.dy, d.addv = d.x.to(dt), d.dy.to(dt), d.addv.to(dt)
        if c.row_scale:
            n = -(-rows // c.rps)
            d.rsc = pick([0.0, 1.0, 2.0] if c.exact else [0.0, 1.0 / 0.9, 1.0 / 0.7], n)
            d.rsc[0] = d.rsc[0] if n == 1 else 2.0 if c.exact else 1.0 / 0.9
            if n > 1:
                d.rsc[1] = 0.0
        d.qscale = 16.0
    elif c.kind == "act":
        if c.fill == "sweep":
            x = bf16_sweep()
        elif c.fill == "grid":
            x = torch.cat([torch.linspace(-12.0, 12.0, 1 << 16), _edge_values("f32")])
            x = torch.cat([x, torch.zeros(-x.numel() % 8)])
        else:
            x = 3.0 * randn(max(D - 8, 0)).to(dt).float()
            x = torch.where((x == 0.0) | (x == 6.0), torch.ones_like(x), x)      # no value at a ReLU6 edge but the deliberate ones
            x = torch.cat([_edge_values(c.dtype), x])[:D]
        assert x.numel() == D, (c.name, x.numel())
        d.x = x.to(dt)
        d.dy = (rint(-3, 3, D) if c.op == "relu6" else randn(D)).to(dt)
    elif c.kind == "scale":
        d.x, d.addv = randn(rows, D).to(dt), randn(rows, D).to(dt)
        d.scale = torch.tensor([0.0, 1.0, 1.0 / 0.9, 2.0, 1.0 / 0.9])[:rows].clone() if rows > 1 else torch.tensor([1.0 / 0.9])
        d.scale = d.scale.float()
    elif c.kind == "softmax":
        if c.fill == "equal":
            d.s = pick([-3.0, 0.5, 7.0], rows, 1).expand(rows, D).clone()
        elif c.fill == "equal_large":
            d.s = torch.full((rows, D), 1e4 / c.scale)
        else:
            d.s = 4.0 * randn(rows, D) / math.sqrt(c.scale)
        d.dp = randn(rows, D)
        z = (d.s.double() * float(torch.tensor(c.scale, dtype=torch.float32)))
        d.p = rnd(torch.softmax(z, 1), c.dtype).to(dt)
    elif c.kind == "transpose":
        Z, W = c.outer * c.inner, (3 if c.which >= 0 else 1) * c.inner * D
        d.src = randn(c.outer, c.T, W).to(dt)           # [outer][T][(3) inner dh]
    elif c.kind == "assemble":
        d.tok = randn(rows, c.T - (1 if c.cls else 0), D).to(dt)
        d.clsv, d.pos = randn(D), randn(c.T, D)
        d.g = randn(rows, c.T, D).to(dt)
    elif c.kind == "colsum":
        d.x = (rint(-8, 8, rows, D) if c.exact else randn(rows, D)).to(dt)
        d.out0 = rint(-5, 5, D) if c.exact else randn(D)
    elif c.kind == "dropout":
        d.x, d.addv = randn(D).to(dt), randn(D).to(dt)
        d.g = randn(D).to(dt)
    for k, v in vars(d).items():
        if isinstance(v, torch.Tensor):
            setattr(d, k, v.contiguous().to(device))
    return d


# ---- the operations: exact = float64 reference, otherwise the fp32 yardstick (with an optional mutant) ---------------------------------
def _rsum(t, order):
    """sum over the last dimension: torch's order, or ("strided") from the far end"""
    return t.flip(-1).sum(-1) if order == "strided" else t.sum(-1)


def _padded(t, pad, fill=GARBAGE):
    """[rows][D] -> [rows][D + pad] with `fill` behind D"""
    return torch.cat([t, torch.full((t.shape[0], pad), fill, dtype=t.dtype, device=t.device)], 1) if pad else t


def _param_reduce(terms, rows_idx, rows, prefill, exact, mutant, order):
    """prefill + the column sums of terms[rows_idx] the way the workspace form forms them: per-block partial rows (block of row r =
    (r mod 4 blocks) / 4), LN_SLICES contiguous slices of them, the slice sums in slice order"""
    t = terms[rows_idx]
    if exact:
        return prefill.double() + t.double().sum(0)
    blocks = ln_bwd_blocks(rows)
    blk = (rows_idx % (4 * blocks)) // 4
    if order == "strided":
        t, blk = t.flip(0), blk.flip(0)
    P = torch.zeros(blocks, t.shape[1], dtype=t.dtype, device=t.device).index_add_(0, blk, t)
    per = -(-blocks // LN_SLICES)
    total = torch.zeros(t.shape[1], dtype=t.dtype, device=t.device)
    sl = range(LN_SLICES - 1 if mutant == "drop_last_slice" else LN_SLICES)
    for s in (reversed(sl) if order == "strided" else sl):
        total = total + P[s * per:min(blocks, (s + 1) * per)].sum(0)
    return total if mutant == "final_assigns" else prefill.to(t.dtype) + total


def _ln(c, d, exact, mutant, order):
    up = (lambda t: t.double()) if exact else (lambda t: t.float())
    rows, D = c.rows, c.D
    tail, _, np_ = ln_form(D)
    dev = d.x.device
    x, gamma, beta = up(d.x), up(d.gamma), up(d.beta)
    out = {}
    # forward
    xe, Dn = x, D
    if mutant == "tail_reads_pad" and tail:
        xe = _padded(x, min(256 * np_, D + c.pad[0]) - D)
    if mutant == "tail_padded_width" and tail:
        Dn = 256 * np_
    mu = _rsum(xe, order) / Dn
    a = xe - mu[:, None]
    var = (_rsum(xe * xe, order) / Dn - mu * mu) if mutant == "single_pass_variance" else _rsum(a * a, order) / Dn
    if mutant == "unbiased_variance":
        var = _rsum(a * a, order) / (Dn - 1)
    rs = 1.0 / (torch.sqrt(var) + d.eps) if mutant == "eps_outside_sqrt" else 1.0 / torch.sqrt(var + d.eps)
    y = a[:, :D] * rs[:, None] * gamma + beta
    out["mean"], out["rstd"], out["y"] = mu.double(), rs.double(), (y if exact else rnd(y, c.dtype)).double()
    if exact:
        dmu = (D + 1) * U * x.abs().sum(1) / D
        dvar = dmu * dmu + (D + 6) * U * (var + dmu * dmu)
        out["e_mean"], out["e_rstd"] = dmu, rs * (6 * U + dvar / (2 * (var + d.eps)))
        out["e_y"] = 4 * U * ((a * rs[:, None] * gamma).abs() + beta.abs()) + gamma.abs() * (rs * dmu)[:, None] + (a * gamma).abs() * out["e_rstd"][:, None]
    # backward, from the supplied statistics
    mean, rstd, g0 = up(d.bmean)[:, None], up(d.brstd)[:, None], up(d.dy)
    xh = (x - mean) * rstd
    tg = (g0 * gamma) * xh if mutant == "dgamma_from_dy_gamma" else g0 * xh
    g = g0 * gamma
    c1, c2 = _rsum(g, order)[:, None] / D, _rsum(g * xh, order)[:, None] / D
    o = rstd * (g - c1) if mutant == "dx_without_c2" else rstd * (g - c1 - xh * c2)
    if c.add:
        av = up(d.addv)
        if mutant == "add_input_stride":          # row r read at r * (the stride of dy) in a buffer laid out with out's stride
            flat = _padded(av, c.pad[2]).reshape(-1)
            idx = torch.arange(rows, device=dev)[:, None] * (D + c.pad[1]) + torch.arange(D, device=dev)[None, :]
            av = flat[idx]
        o = o + av
    dx = o if exact else rnd(o, c.dtype)
    idx = torch.arange(rows, device=dev)
    if mutant == "drop_last_row":
        idx = idx[:-1]
    if mutant == "drop_second_row":
        idx = idx[idx != 4 * ln_bwd_blocks(rows)]
    if mutant == "dup_row":
        idx = torch.cat([idx, idx[-1:]])
    out["dgamma"] = _param_reduce(tg, idx, rows, d.dgamma0, exact, mutant, order).double()
    out["dbeta"] = _param_reduce(g0, idx, rows, d.dbeta0, exact, mutant, order).double()
    out["abs_g"], out["abs_b"] = (g0 * xh).double().abs().sum(0), g0.double().abs().sum(0)
    if mutant == "drop_last_row" and not exact:       # the row is never written: the outputs keep their NaN
        dx, out["y"] = dx.clone(), out["y"].clone()
        dx[-1], out["y"][-1] = float("nan"), float("nan")
    out["dx"] = dx.double()
    if exact:
        out["e_dx"] = 2.0 ** -20 * ((rstd * g).abs() + (rstd * c1).abs() + (rstd * xh * c2).abs() + (av.abs() if c.add else 0.0)) \
            + rstd.abs() * (D + 3) * U * (g.abs().mean(1, keepdim=True) + xh.abs() * (g * xh).abs().mean(1, keepdim=True))
        out["chain"] = (xh, g, c1, c2, xh * c2, g - c1, g - c1 - xh * c2, rstd * (g - c1 - xh * c2), o)
    if c.second != "none":
        r = torch.arange(rows, device=dev)
        sel = r.clamp_max(d.rsc.numel() - 1) if (c.row_scale and mutant == "row_scale_by_row") else (r // max(c.rps, 1))
        rsc = up(d.rsc)[sel][:, None] if c.row_scale else torch.ones(rows, 1, dtype=x.dtype, device=dev)
        stored = rnd(o, c.dtype)
        if c.second == "scaled":
            out["copy"] = rnd(f32(stored.double() * rsc.double()), c.dtype).double()
        else:
            terms = (o if mutant == "colsum_prerounding" else stored) * rsc
            out["colsum"] = _param_reduce(terms, idx, rows, d.colsum0, exact, mutant, order).double()
            out["rsc_rows"] = rsc.double()
    return out


def _act(c, d, exact, mutant):
    up = (lambda t: t.double()) if exact else (lambda t: t.float())
    x, dy = up(d.x), up(d.dy)
    out = {}
    if c.op == "relu6":
        out["y"] = x.clamp(0.0, 6.0)
        m = (x >= 0) & (x <= 6) if mutant == "relu6_inclusive" else (x > 0) & (x < 6)
        out["dx"] = torch.where(m, dy, torch.zeros_like(dy))
        return {k: v.double() for k, v in out.items()}
    if c.op == "gelu":
        if mutant == "tanh_gelu":
            t = torch.tanh(0.7978845608028654 * (x + 0.044715 * x * x * x))
            Phi = 0.5 * (1.0 + t)
            der = Phi + 0.5 * x * (1 - t * t) * 0.7978845608028654 * (1 + 3 * 0.044715 * x * x)
        else:
            k = 0.5641895835477563 if mutant == "der_const_sqrt_pi" else 0.3989422804014327
            er = torch.erf(x * 0.70710678118654752)
            Phi = 0.5 * (1.0 + er)
            der = Phi + x * k * torch.exp(-0.5 * x * x)
            if exact:
                out["m_y"] = 0.5 * x.abs() * (1 + er.abs())
                out["m_der"] = 0.5 * (1 + er.abs()) + (x * k * torch.exp(-0.5 * x * x)).abs()
        y = x * Phi
    else:
        a = 1.7 if mutant == "quick_1p7" else QA
        s = 1.0 / (1.0 + torch.exp(-a * x))
        y = x * s
        der = s + a * (y * (1.0 - s))
        if exact:
            rel = 2 * A_EXP * U + 4 * U * (QA * x).abs() + 10 * U
            out["m_y"], out["m_der"] = y.abs() * rel, (s.abs() + QA * y.abs()) * rel
    st = (lambda t: t) if exact else (lambda t: rnd(t, c.dtype))
    out["y"], out["gp"], out["dx"] = st(y), st(der), st(dy * der)
    out["der"] = der
    return {k: v.double() for k, v in out.items()}


def _scale(c, d, exact, mutant):
    up = (lambda t: t.double()) if exact else (lambda t: t.float())
    v = up(d.x) * up(d.scale)[:, None]
    out = {"terms": v.abs() + (up(d.addv).abs() if c.add else 0.0)}
    if c.add:
        v = v + up(d.addv)
    out["out"] = (v if exact else rnd(v, c.dtype)).double()
    return out


def _softmax(c, d, exact, mutant, order):
    up = (lambda t: t.double()) if exact else (lambda t: t.float())
    rows, cols, ldp = c.rows, c.D, c.ld
    sc = torch.tensor(c.scale, dtype=torch.float32).double().item()
    s = up(d.s)
    z = s * sc
    if mutant == "no_max_subtraction":
        e = torch.exp(z)
    elif mutant == "scale_after_max":
        e = torch.exp((s - s.max(1, keepdim=True).values) * sc * sc)
    else:
        e = torch.exp(z - z.max(1, keepdim=True).values)
    p = e * (1.0 / _rsum(e, order))[:, None]
    fillv = float("nan") if mutant == "pad_not_zeroed" else 0.0           # the output region starts as NaN
    pad = lambda t: _padded(t, ldp - cols, fillv)
    out = {"p": pad(p if exact else rnd(p, c.dtype)).double()}
    ps, dp = up(d.p), up(d.dp)
    if mutant == "dot_over_ldp":          # the columns behind `cols` of the score gradient hold garbage, those of p zeros but for a stale one
        dot = _rsum(dp * ps, order) + (min(ldp, c.lds) - cols) * GARBAGE * GARBAGE
    else:
        dot = _rsum(dp * ps, order)
    ds = ps * (dp - dot[:, None]) if mutant == "bwd_no_scale" else sc * ps * (dp - dot[:, None])
    out["ds"] = pad(ds if exact else rnd(ds, c.dtype)).double()
    if exact:
        rho = 2 * A_EXP * U + 2 * U * z.abs().max(1, keepdim=True).values
        out["e_p"] = _padded(p * (2 * rho + (cols + 3) * U), ldp - cols, 0.0)
        out["e_ds"] = _padded((cols + 4) * U * (sc * ps).abs() * (dp.abs() + (dp * ps).abs().sum(1, keepdim=True)), ldp - cols, 0.0)
    return out


def _transpose(c, d, exact, mutant):
    dh, T, ldt = c.D, c.T, c.ld
    src = d.src.double()                                   # [outer][T][(3) inner dh]
    W = src.shape[2]
    off = max(c.which, 0) * c.inner * dh
    v = src[:, :, off:off + c.inner * dh].reshape(c.outer, T, c.inner, dh)
    o = v.permute(0, 2, 3, 1).reshape(c.outer * c.inner, dh, T)
    if mutant == "not_transposed":
        o = v.permute(0, 2, 1, 3).reshape(c.outer * c.inner, T * dh).reshape(c.outer * c.inner, dh, T)
    fillv = float("nan") if mutant == "transpose_pad_not_zeroed" else 0.0
    o = torch.cat([o, torch.full((o.shape[0], dh, ldt - T), fillv, dtype=o.dtype, device=o.device)], 2)
    return {"out": o}


def _assemble(c, d, exact, mutant):
    up = (lambda t: t.double()) if exact else (lambda t: t.float())
    B, Tn, D = c.rows, c.T, c.D
    tok, pos = up(d.tok), up(d.pos)
    if c.cls:
        first = (up(d.clsv) + pos[1 if mutant == "cls_takes_pos1" else 0]).expand(B, 1, D)
        x = torch.cat([first, tok + pos[1:]], 1)
        dtok = d.g.double()[:, :Tn - 1] if mutant == "bwd_keeps_cls_row" else d.g.double()[:, 1:]
    else:
        x = tok + pos
        dtok = None
    out = {"x": (x if exact else rnd(x, c.dtype)).double(), "terms": x.abs()}
    if dtok is not None:
        out["dtok"] = dtok.contiguous()
    return out


def _colsum(c, d, exact, mutant, order):
    x = d.x.double() if exact else d.x.float()
    rows = c.rows
    out = {"abs": d.x.double().abs().sum(0)}
    if exact:
        out["out"] = d.out0.double() + x.sum(0)
        return out
    ry = colsum_splits(rows)
    rpb = -(-rows // ry)
    blk = torch.arange(rows, device=x.device) // rpb
    if order == "strided":
        x, blk = x.flip(0), blk.flip(0)
    P = torch.zeros(ry, c.D, device=x.device).index_add_(0, blk, x)
    if mutant == "colsum_drop_last_block":
        P = P[:int(blk.max())]
    out["out"] = (d.out0.float() + (P.flip(0).sum(0) if order == "strided" else P.sum(0))).double()
    return out


def _dropout(c, d, exact, mutant):
    up = (lambda t: t.double()) if exact else (lambda t: t.float())
    n = c.D
    keep = dropout_keep(torch.arange(n, dtype=torch.int64, device=d.x.device), c.seed, c.p, mutant)
    p32 = torch.tensor(c.p, dtype=torch.float32)
    scale = (1.0 / (1.0 - p32.double())).item() if exact else (1.0 / (1.0 - p32)).item()
    zero = torch.zeros((), dtype=torch.float64 if exact else torch.float32, device=d.x.device)
    av = up(d.addv)
    st = (lambda t: t.double()) if exact else (lambda t: rnd(t, c.dtype).double())

    def apply(v):
        o = torch.where(keep, up(v) * scale, zero)
        if mutant == "add_dropped_with_element":
            return st(torch.where(keep, o + av, zero))
        return st(o + av if c.add else o)
    return {"mask": keep, "out": apply(d.x), "dx": apply(d.g), "terms": (up(d.x) * scale).abs() + av.abs(),
            "terms_dx": (up(d.g) * scale).abs() + av.abs()}


def outputs(c: Case, d, *, exact: bool, mutant: Optional[str] = None, order: Optional[str] = None):
    k = c.kind
    if k == "ln":
        return _ln(c, d, exact, mutant, order)
    if k == "act":
        return _act(c, d, exact, mutant)
    if k == "scale":
        return _scale(c, d, exact, mutant)
    if k == "softmax":
        return _softmax(c, d, exact, mutant, order)
    if k == "transpose":
        return _transpose(c, d, exact, mutant)
    if k == "assemble":
        return _assemble(c, d, exact, mutant)
    if k == "colsum":
        return _colsum(c, d, exact, mutant, order)
    return _dropout(c, d, exact, mutant)


def mutant_applies(c: Case, mutant: str) -> bool:
    """whether the mutant can exist at the case at all (whether it changes anything there is decided by `rejecting`)"""
    k = c.kind
    ln = k == "ln"
    tail = ln and ln_form(c.D)[0]
    table = dict(
        tail_padded_width=tail and c.D % 256 != 0, unbiased_variance=ln and c.cond != "bad", tail_reads_pad=tail and c.pad[0] > 0 and c.D % 256 != 0,
        eps_outside_sqrt=ln and c.cond == "small", single_pass_variance=ln and c.cond == "bad", dgamma_from_dy_gamma=ln,
        dx_without_c2=ln, add_input_stride=ln and c.add and c.pad[1] != c.pad[2] and c.rows > 1, drop_last_row=ln,
        drop_second_row=ln and c.rows > 4 * ln_bwd_blocks(c.rows), dup_row=ln, drop_last_slice=ln and ln_bwd_blocks(c.rows) >= LN_SLICES,
        final_assigns=ln, colsum_prerounding=ln and c.second in ("e4m3", "e5m2") and c.rows <= 300,
        row_scale_by_row=ln and c.row_scale and c.rps > 1 and c.rows > 1,
        tanh_gelu=k == "act" and c.op == "gelu" and c.D > 16, der_const_sqrt_pi=k == "act" and c.op == "gelu" and c.D > 16,
        quick_1p7=k == "act" and c.op == "quick_gelu" and c.D > 16,
        relu6_inclusive=k == "act" and c.op == "relu6",
        no_max_subtraction=k == "softmax" and c.fill == "equal_large", scale_after_max=k == "softmax" and c.scale != 1.0,
        pad_not_zeroed=k == "softmax" and c.ld > c.D, dot_over_ldp=k == "softmax" and c.ld > c.D, bwd_no_scale=k == "softmax" and c.scale != 1.0,
        not_transposed=k == "transpose" and c.T > 1 and c.D > 1, transpose_pad_not_zeroed=k == "transpose" and c.ld > c.T,
        cls_takes_pos1=k == "assemble" and c.cls, bwd_keeps_cls_row=k == "assemble" and c.cls,
        colsum_drop_last_block=k == "colsum", thresh_gt=k == "dropout" and c.fill == "edge", seed_words_swapped=k == "dropout" and c.p > 0,
        add_dropped_with_element=k == "dropout" and c.add and c.p > 0)
    return bool(table[mutant])


# ---- the checks ------------------------------------------------------------------------------------------------------------------
BIT_EXACT = {"scale": ("out",), "transpose": ("out",), "assemble": ("x", "dtok"), "dropout": ("mask", "out", "dx")}


def _reduction(got, ref, n, ab, pre):
    return _elem(got, ref, n * U * (ab + pre.double().abs()))


def _ln_dx_exact(c, d, ref):
    """the documented expression of dx is exact in fp32 at this case: every intermediate is a number of fp32 and the two wave sums
    are sums of multiples of a power of two whose absolute sum stays below 2^24 of them"""
    if not c.exact or c.D & (c.D - 1):
        return False
    xh, g, c1, c2 = ref["chain"][:4]
    ok = all(bool((f32(v) == v).all()) for v in ref["chain"])
    ok = ok and bool(((g * 2) == (g * 2).round()).all()) and g.abs().sum(1).max().item() <= 2.0 ** 23
    ok = ok and bool((((g * xh) * 4) == ((g * xh) * 4).round()).all()) and (g * xh).abs().sum(1).max().item() <= 2.0 ** 22
    return ok


def verdict(c: Case, d, ref: dict, got: dict) -> dict:
    """{output: (worst err / bound, err, bound)} of `got` (a kernel's or a yardstick's outputs as float64 / bool tensors); only
    the outputs `got` carries are judged"""
    v = {}
    k = c.kind
    if k in BIT_EXACT or (k == "act" and c.op == "relu6"):
        yard = outputs(c, d, exact=False)
        for name in (BIT_EXACT.get(k) or ("y", "dx")):
            if name in got and name in yard:
                v[name] = _worst(*_same(got[name].double(), yard[name].double()))
        return v
    if k == "ln":
        D, rows = c.D, c.rows
        if "mean" in got:
            v["mean"] = _worst(*(_same(got["mean"], ref["mean"]) if c.exact and D & (D - 1) == 0 else
                                 _elem(got["mean"], ref["mean"], ref["e_mean"] + TINY["f32"])))
            v["rstd"] = _worst(*_elem(got["rstd"], ref["rstd"], ref["e_rstd"]))
        if "y" in got:
            v["y"] = _worst(*_store(got["y"], ref["y"], ref["e_y"], c.dtype))
        for name, ab, pre in (("dgamma", "abs_g", d.dgamma0), ("dbeta", "abs_b", d.dbeta0)):
            if name in got:
                v[name] = _worst(*(_same(got[name], ref[name]) if c.exact else _reduction(got[name], ref[name], rows + 3, ref[ab], pre)))
        if "dx" in got:
            if _ln_dx_exact(c, d, ref):
                v["dx"] = _worst(*_same(got["dx"], rnd(ref["dx"], c.dtype)))
            else:
                r = R_BF16 if c.dtype == "bf16" else 0.0
                v["dx"] = _worst(*_elem(got["dx"], ref["dx"], r * ref["dx"].abs() + ref["e_dx"] + TINY[c.dtype]))
        if "colsum" in got:          # against the float64 sums of the stored dx the same `got` carries
            terms = got["dx"].double() * ref["rsc_rows"]
            v["colsum"] = _worst(*_reduction(got["colsum"], d.colsum0.double() + terms.sum(0), rows + 3, terms.abs().sum(0), d.colsum0))
        if "copy" in got:
            sel = torch.arange(rows, device=got["dx"].device) // c.rps
            want = rnd(f32(got["dx"].double() * d.rsc.double()[sel][:, None]), c.dtype)
            v["copy"] = _worst(*_same(got["copy"], want))
        return v
    if k == "act":
        gelu = c.op == "gelu"
        e_y = A_GELU_FWD * ulp32(ref["m_y"]) if gelu else ref["m_y"]
        e_d = A_GELU_DER * ulp32(ref["m_der"]) if gelu else ref["m_der"]
        for name, e in (("y", e_y), ("gp", e_d), ("dx", e_d * d.dy.double().abs() + U * ref["dx"].abs())):
            if name in got:
                v[name] = _worst(*_store(got[name], ref[name], e, c.dtype))
        return v
    if k == "softmax":
        for name, e in (("p", "e_p"), ("ds", "e_ds")):
            if name in got:
                if name == "p" and c.fill.startswith("equal") and c.D & (c.D - 1) == 0:
                    v[name] = _worst(*_same(got[name], ref[name]))
                else:
                    v[name] = _worst(*_store(got[name], ref[name], ref[e], c.dtype))
        return v
    # colsum
    if "out" in got:
        v["out"] = _worst(*(_same(got["out"], ref["out"]) if c.exact else _reduction(got["out"], ref["out"], c.rows + 3, ref["abs"], d.out0)))
    return v


def yardstick_to_reference(c: Case, d, ref, yard) -> dict:
    """ties the fp32 yardstick of a bit-exact kind to the float64 reference: within 3 U of the operand terms and the store rounding"""
    v = {}
    k = c.kind
    if k == "scale":
        v["out"] = _worst(*_store(yard["out"], ref["out"], 3 * U * ref["terms"], c.dtype))
    elif k == "assemble":
        v["x"] = _worst(*_store(yard["x"], ref["x"], 3 * U * ref["terms"], c.dtype))
        if "dtok" in ref:
            v["dtok"] = _worst(*_same(yard["dtok"], ref["dtok"]))
    elif k == "dropout":
        v["mask"] = _worst(*_same(yard["mask"].double(), ref["mask"].double()))
        v["out"] = _worst(*_store(yard["out"], ref["out"], 3 * U * ref["terms"], c.dtype))
        v["dx"] = _worst(*_store(yard["dx"], ref["dx"], 3 * U * ref["terms_dx"], c.dtype))
    elif k == "transpose":
        v["out"] = _worst(*_same(yard["out"], ref["out"]))
    elif k == "act" and c.op == "relu6":
        v["y"], v["dx"] = _worst(*_same(yard["y"], ref["y"])), _worst(*_same(yard["dx"], ref["dx"]))
    return v


def representable(c: Case, d, ref: dict) -> bool:
    """every output an exact case compares value for value is a number of its output type, and every fp32 sum behind it is exact in
    any order (terms are multiples of a power of two q, and sum |terms| + |prefill| stays below 2^24 q)"""
    t = lambda v: bool((rnd(v, c.dtype) == v).all())
    f = lambda v: bool((f32(v) == v).all())
    if c.kind == "ln":
        x, dy = d.x.double(), d.dy.double()
        xh = (x - d.bmean.double()[:, None]) * d.brstd.double()[:, None]
        tg = dy * xh
        ok = bool(((tg * 2) == (tg * 2).round()).all()) and bool((dy == dy.round()).all())
        ok = ok and (tg.abs().sum(0) + d.dgamma0.double().abs()).max().item() <= 2.0 ** 23
        ok = ok and (dy.abs().sum(0) + d.dbeta0.double().abs()).max().item() <= 2.0 ** 24
        ok = ok and f(ref["dgamma"]) and f(ref["dbeta"])
        if c.D & (c.D - 1) == 0:
            ok = ok and bool((x == x.round()).all()) and x.abs().sum(1).max().item() <= 2.0 ** 24 and f(ref["mean"])
            if c.D <= 256:
                ok = ok and _ln_dx_exact(c, d, ref)
        return ok
    if c.kind == "colsum":
        x = d.x.double()
        return bool((x == x.round()).all()) and (x.abs().sum(0) + d.out0.double().abs()).max().item() <= 2.0 ** 24 and f(ref["out"])
    if c.kind == "softmax":
        return t(ref["p"]) and bool((ref["p"][:, :c.D] == 1.0 / c.D).all())
    return True


def rejecting(c: Case, d, mutant: str, ref=None, yard=None):
    """the outputs whose check rejects the mutated yardstick; None where the mutant changes nothing at this case"""
    if not mutant_applies(c, mutant):
        return None
    ref = ref if ref is not None else outputs(c, d, exact=True)
    yard = yard if yard is not None else outputs(c, d, exact=False)
    mut = outputs(c, d, exact=False, mutant=mutant)
    keys = [k for k in mut if isinstance(mut[k], torch.Tensor) and k in yard and not k.startswith(("abs", "terms", "e_", "m_", "rsc_"))]
    same = all(mut[k].shape == yard[k].shape and bool(((mut[k] == yard[k]) | ((mut[k] != mut[k]) & (yard[k] != yard[k]))).all()) for k in keys)
    if same:
        return None
    return [k for k, (r, _, _) in verdict(c, d, ref, mut).items() if r > 1.0]


# ---- the case table --------------------------------------------------------------------------------------------------------------
LN_VW4 = (256, 512, 768, 1024, 1280, 2048)
LN_VW2 = (128, 384, 640, 896)
LN_TAIL = (8, 64, 72, 96, 192, 248, 264, 1032, 1152, 2040)
LN_ROWS = (1, 3, 4, 5, 45, 37, 300)
LN_PADS = ((0, 0, 0), (8, 16, 24), (0, 0, 0), (24, 8, 16))


def _ln_cases():
    out = []
    i = 0
    for D in LN_VW4 + LN_VW2 + LN_TAIL:
        for rows in LN_ROWS:
            for dt in ("bf16", "f32"):
                exact, add, pad = i % 2 == 0, (i // 2) % 2 == 0, LN_PADS[(i // 3) % 4]
                i += 1
                out.append(Case("ln", f"ln-{rows}x{D}-{dt}-{'exact' if exact else 'random'}{'-add' if add else ''}-pad{pad[0]}.{pad[1]}.{pad[2]}",
                                dt, rows, D, exact, add=add, pad=pad))
            i += 1
    # grid caps: the second trip of the 512-block atomic backward, of the 4096-block forward, the 1024-block workspace cap
    for rows, widths in ((2053, (8, 128, 256, 768)), (16389, (8, 128, 256, 768)), (45061, (8, 256))):
        for j, D in enumerate(widths):
            dt = "bf16" if D == 768 or j % 2 == 0 else "f32"
            out.append(Case("ln", f"ln-{rows}x{D}-{dt}-exact-add", dt, rows, D, True, add=True))
            if rows == 2053:
                out.append(Case("ln", f"ln-{rows}x{D}-{dt}-random-pad8.16.24", dt, rows, D, False, pad=(8, 16, 24)))
    # partial-row counts of the slice reduction: 1 (above), 15, 16, 17 (1024 above): empty and uneven slices
    for rows, blocks in ((650, 15), (700, 16), (730, 17), (1450, 33)):
        assert ln_bwd_blocks(rows) == blocks
        for D, dt in ((8, "f32"), (72, "bf16"), (256, "bf16")):
            out.append(Case("ln", f"ln-{rows}x{D}-{dt}-exact-{blocks}partials", dt, rows, D, True, add=D == 72))
    # the class-token stride: x and dx rows T D apart, dy packed
    for D, dt in ((192, "bf16"), (384, "f32"), (768, "bf16")):
        out.append(Case("ln", f"ln-5x{D}-{dt}-random-cls", dt, 5, D, False, pad=(4 * D, 0, 4 * D)))
        out.append(Case("ln", f"ln-5x{D}-{dt}-exact-cls", dt, 5, D, True, pad=(4 * D, 0, 4 * D)))
    # forward without mean / rstd
    for D, dt in ((72, "bf16"), (128, "f32"), (256, "bf16")):
        out.append(Case("ln", f"ln-37x{D}-{dt}-random-nostats", dt, 37, D, False, stats=False))
    # conditioning: mean 100 / std 0.1 (fp32: bf16 cannot hold it) and a variance at the scale of eps
    for D in (64, 256, 1024):
        out.append(Case("ln", f"ln-37x{D}-f32-random-bad", "f32", 37, D, False, cond="bad"))
        out.append(Case("ln", f"ln-37x{D}-f32-random-small", "f32", 37, D, False, cond="small"))
        out.append(Case("ln", f"ln-37x{D}-bf16-random-small", "bf16", 37, D, False, cond="small"))
    # the 64-register backward (bf16, workspace, D in 256 512 768) runs in every case above at those widths; the register form at
    # the same widths with a second output: fp8 copies with and without row_scale, the scaled copy
    for D in (256, 512, 768, 1024):
        for rows in (5, 300):
            for second, rs in (("e5m2", False), ("e5m2", True), ("e4m3", True), ("scaled", True)):
                for exact in (True, False):
                    out.append(Case("ln", f"ln-{rows}x{D}-bf16-{'exact' if exact else 'random'}-{second}{'-rowscale' if rs else ''}",
                                    "bf16", rows, D, exact, add=True, second=second, row_scale=rs, rps=1 if rows == 5 and second == "e4m3" else 50 if rows == 300 else 2))
    for D in (256, 1024):      # past the 1024-block cap of the fp8 forward
        out.append(Case("ln", f"ln-4101x{D}-bf16-random-scaled-rowscale", "bf16", 4101, D, False, second="scaled", row_scale=True, rps=197))
        out.append(Case("ln", f"ln-4101x{D}-bf16-exact-e4m3-rowscale", "bf16", 4101, D, True, second="e4m3", row_scale=True, rps=197))
    return out


def _cases():
    out = _ln_cases()
    # activations: the exhaustive bf16 sweep, the fp32 grid, one vector, the second grid trip (256 * 4096 vectors + 1)
    nsweep, ngrid = bf16_sweep().numel(), (1 << 16) + 8
    for op in ("gelu", "quick_gelu", "relu6"):
        out.append(Case("act", f"act-{op}-bf16-sweep", "bf16", D=nsweep, op=op, fill="sweep"))
        out.append(Case("act", f"act-{op}-f32-grid", "f32", D=ngrid, op=op, fill="grid"))
        for dt in ("bf16", "f32"):
            out.append(Case("act", f"act-{op}-{dt}-one-vector", dt, D=vec(dt), op=op))
            out.append(Case("act", f"act-{op}-{dt}-random-2trips", dt, D=(256 * 4096 + 1) * vec(dt), op=op))
    # scale_rows
    for dt in ("bf16", "f32"):
        for rows, inner in ((1, vec(dt)), (5, vec(dt)), (5, 261 * vec(dt)), (1, 261 * vec(dt))):
            for add in (False, True):
                out.append(Case("scale", f"scale-{rows}x{inner}-{dt}{'-add' if add else ''}", dt, rows, inner, add=add))
    # softmax
    for dt in ("bf16", "f32"):
        for cols in (1, 8, 17, 63, 64, 65, 197):
            for ldp in sorted({-(-cols // 8) * 8, -(-cols // 64) * 64}):
                for rows, scale in ((1, 1.0), (5, 0.125)):
                    out.append(Case("softmax", f"softmax-{rows}x{cols}-ldp{ldp}-{dt}-scale{scale}", dt, rows, cols, ld=ldp, lds=ldp + 8, scale=scale))
        for cols in (1, 8, 64):
            for fill in ("equal", "equal_large"):
                out.append(Case("softmax", f"softmax-5x{cols}-ldp{-(-(cols + 1) // 8) * 8}-{dt}-{fill}", dt, 5, cols, True, ld=-(-(cols + 1) // 8) * 8,
                                lds=-(-cols // 8) * 8 + 16, scale=0.125, fill=fill))
        out.append(Case("softmax", f"softmax-32773x8-ldp8-{dt}-scale0.125", dt, 32768 + 5, 8, ld=8, lds=16, scale=0.125))
    # head transpose: the engine's qkv strides (q, k, v) and a plain source
    i = 0
    for T in (1, 17, 64, 65, 197):
        for dh in (8, 64, 72):
            for ldt in sorted({-(-T // 8) * 8, -(-T // 64) * 64}):
                for outer, inner in ((1, 1), (3, 2)):
                    dt, which = ("bf16", "f32")[i % 2], (0, 1, 2, -1)[(i // 2) % 4]
                    i += 1
                    out.append(Case("transpose", f"transpose-T{T}-dh{dh}-ldt{ldt}-{outer}x{inner}-{dt}-{'qkvp'[which]}", dt, D=dh, T=T, ld=ldt,
                                    outer=outer, inner=inner, which=which))
    # token assembly
    for B, Tn, D in ((1, 2, 8), (3, 5, 128), (2, 5, 12), (3, 17, 192)):
        for dt in ("bf16", "f32"):
            for cls in (True, False):
                out.append(Case("assemble", f"assemble-{B}x{Tn}x{D}-{dt}{'' if cls else '-nocls'}", dt, B, D, T=Tn, cls=cls))
        if D % 8 == 0:
            out.append(Case("assemble", f"assemble-{B}x{Tn}x{D}-bf16-offset8bytes", "bf16", B, D, T=Tn, offset=4))
    # column sums: the atomic form and the workspace form at 2, 6, 48 and 256 splits
    for C in (8, 64, 72, 96, 70):
        for dt in ("bf16", "f32"):
            for form, rws in (("atomic", (1, 3, 4, 256, 257)), ("work", (257, 1300, 12100, 65541))):
                for rows in rws:
                    exact = (rows + C) % 2 == 0 or rows > 1300
                    out.append(Case("colsum", f"colsum-{rows}x{C}-{dt}-{form}-{'exact' if exact else 'random'}", dt, rows, C, exact,
                                    ld=C + (8 if C != 70 else 2), form=form))
    assert [colsum_splits(r) for r in (257, 1300, 12100, 65541)] == [2, 6, 48, 256]
    # dropout
    seeds = (0, 0x1234567, 0x9e3779b97f4a7c15)
    i = 0
    for n in (1, 255, 256, 257, 256 * 4096 + 3):
        for p in (0.0, 0.1, 0.5, 0.999):
            dt, seed = ("bf16", "f32")[i % 2], seeds[i % 3]
            add, alias = i % 2 == 1 or n == 257, ("none", "in", "add")[(i // 2) % 3]
            i += 1
            if alias == "add" and not add:
                alias = "none"
            out.append(Case("dropout", f"dropout-{n}-p{p}-{dt}-seed{seed:x}{'-add' if add else ''}-alias_{alias}", dt, D=n, p=p, seed=seed,
                            add=add, alias=alias))
    # one element whose hash equals the threshold: the only place where `>=` and `>` differ
    for j, (p, hi) in enumerate(((0.5, 0), (0.1, 0x9e3779b9), (0.0, 7))):
        seed = seed_hitting(77, p, hi)
        out.append(Case("dropout", f"dropout-256-p{p}-{'bf16' if j % 2 else 'f32'}-seed{seed:x}-edge", "bf16" if j % 2 else "f32", D=256, p=p,
                        seed=seed, fill="edge", add=j == 1))
    return tuple(out)


CASES = _cases()
assert len({c.name for c in CASES}) == len(CASES)
