"""Float64 reference of the weight-gradient kernels (conv_wgrad_kernel<T> of csrc/conv_igemm.hip behind nkb_conv_wgrad /
nkb_conv_wgrad_assign, nkb_stem_wgrad and nkb_gemm_tn_batched; wgrad3x3p_kernel<PWS, 3> of csrc/wgrad3x3.hip; wgradr_kernel<3, 4> /
<2, 8> of csrc/wgradr.hip; wgrad8p_kernel of csrc/wgrad256.hip; and the wgrad_reduce kernels behind them), two data regimes with
their operand makers and verdicts, mutants that make the reference wrong the way these kernels go wrong, and the case table that
tests/test_wgrad_reference.py (CPU) and tests/test_wgrad_gpu.py walk.  No test lives here.

The operation (include/nkbhip.h):
    dW[co][(r, s, ci)] (+)= sum_m dY[m][co] * rows[m][(r, s, ci)]          rows: conv_reference.gather_index, mode 0
    dbias[co]          (+)= sum_m dY[m][co]
    packed stem (nkb_stem_wgrad): the same over the (R = 7, S = cprw, Cin = EPC) view of xp[N][H][Wp][4] — a 16-byte chunk is one
        "pixel" of EPC channels, the vertical stride / padding are 2 / 3 and the horizontal ones, in chunks, 1 / 2 (bf16: 4 chunks
        = image pixels 2q - 4 .. 2q + 3) or 2 / 3 (fp32: 8 chunks = pixels 2q - 3 .. 2q + 4); dwp[Cout][7 * cprw * EPC]
    batched (nkb_gemm_tn_batched): out[z][a][b] = sum_m A[z][m][a] B[z][m][b], z = zo * inner + zi at element offsets
        zo * s?o + zi * s?i, stored in the compute dtype
Forms: "slab" (a workspace: per-split fp32 slabs, then wgrad_reduce adds them to dw in split order), "assign" (the same, dw
overwritten), "atomic" (no workspace: fp32 atomics into dw), "direct" (the batched entry: one split, stored once).

A worst-case fp32 bound over thousands of pixels cannot see one dropped pixel, so every case runs in two regimes:

  exact     operands are integers -2 .. 2 (exact in bf16 and fp32), the previous contents of dw / dbias integers -3 .. 3.  Every
            product, every partial sum and the result are integers of magnitude at most 4 M + 3 < 2^24, so every fp32 addition is
            exact in any order (inside the MFMA, across stages, splits, the reduce tree, atomics): the result must EQUAL the
            float64 reference.  The direct store must equal the reference rounded once to bf16 (round to nearest even).  This
            regime rejects every indexing, staging, split and reduce error with zero tolerance.
  positive  operands are |N(0, 1)| rounded to the compute dtype, previous contents |N(0, 1)| in fp32: no term is negative, so every
            partial sum is at most the result `total` = previous + sum, and the sum of the absolute terms is the result itself.
            Count of roundings an element can see (each is at most 2^-24 = U relative to a partial sum, hence to `total`):
              K  accumulations of the K = M pixels summed (bf16 products are exact in fp32: 8 x 8 significant bits; the order
                 inside an MFMA and across stages is free, the count is not: one rounding per term added),
              S  additions of the S split partials — the reduce kernel's chains and its fixed tree, or S atomic adds —
                 (dbias: S = the bias partials, splits x column tiles for the generic kernel),
              c  = 1 for the addition of the previous contents (present in "slab"; kept for the other forms: a larger bound)
                 + 1 for fp32 operands, whose products are themselves rounded (each by U of itself, so their sum by U of total).
            Hence |got - total| <= A (K + S + c) U total, with A = A_MFMA and U from tests/conv_reference.py.  A = 2 is an
            ALLOWANCE for the MFMA's internal summation (and the second-order terms, below 0.1 % of the bound at K + S < 2^14),
            which nobody here has measured; with random data the error sits about sqrt(K) below the bound, so A decides no
            verdict.  The bf16 direct store adds R_BF16 the way conv_reference does: r (total + e) + e, r = R_BF16.
            This regime holds the kernels to fp32 accumulation (an accumulator rounded to bf16 per stage, or fp32 operands
            truncated to bf16, are off by 2^-9 .. 2^-8 of the result).
No constant is fitted to what the kernels return.

Checks of a verdict: "dw", "dbias" (where the case has a bias gradient) and "guard" (nothing outside dw / dbias / the advertised
workspace was written).  REJECTED_BY names the regime and the check that rejects each mutant.
"""
import math
from dataclasses import dataclass, replace
from typing import Optional

import torch

import conv_reference as cr
from conv_reference import A_MFMA, R_BF16, TORCH_DT, U
from gemm_reference import bf

GARBAGE = 1e4           # what padding columns and the rows behind M hold in the GPU test's buffers (finite: an over-read is a wrong number)
GR = 3                  # rows of garbage behind the last row of an operand
FAMILY = dict(generic=0, wgrad3x3=1, wgradr=2, wgrad8p=3)        # NKB_WGRAD_* of include/nkbhip.h
REDUCE_NAME = {0: "none", 1: "wgrad_reduce_kernel<1>", 2: "wgrad_reduce_kernel<4>", 3: "wgrad_reduce_kernel<16>",
               4: "wgrad_reduce_scalar_kernel"}

MUTANTS = ("drop_pixel", "stale_stage", "tail_rows_read", "pad_columns_read", "split_dropped", "split_twice", "empty_split_garbage",
           "tap_shifted", "halo_wrap", "image_bleed", "hw_swapped", "stride_ignored", "transposed_result", "cout_tail_dropped",
           "ntot_tail_dropped", "row_tail_written", "bias_one_tile", "bias_not_reduced", "assign_accumulates", "accumulate_assigns",
           "batch_stride_swapped", "acc_bf16", "f32_operands_bf16")
# (regime, check) that rejects each mutant; tests/test_wgrad_reference.py asserts exactly this
REJECTED_BY = dict(
    drop_pixel=("exact", "dw"), stale_stage=("exact", "dw"), tail_rows_read=("exact", "dw"), pad_columns_read=("exact", "dw"),
    split_dropped=("exact", "dw"), split_twice=("exact", "dw"), empty_split_garbage=("exact", "dw"), tap_shifted=("exact", "dw"),
    halo_wrap=("exact", "dw"), image_bleed=("exact", "dw"), hw_swapped=("exact", "dw"), stride_ignored=("exact", "dw"),
    transposed_result=("exact", "dw"), cout_tail_dropped=("exact", "dw"), ntot_tail_dropped=("exact", "dw"),
    row_tail_written=("exact", "guard"), bias_one_tile=("exact", "dbias"), bias_not_reduced=("exact", "dbias"),
    assign_accumulates=("exact", "dw"), accumulate_assigns=("exact", "dw"), batch_stride_swapped=("exact", "dw"),
    acc_bf16=("positive", "dw"), f32_operands_bf16=("positive", "dw"))
INDEXING_MUTANTS = tuple(m for m in MUTANTS if REJECTED_BY[m][0] == "exact")


# ---- kernels ---------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Kern:
    """One weight-gradient kernel as nkb_wgrad_last_kernel tells them apart (bits 0-7 of its answer)"""
    family: str                 # generic | wgrad3x3 | wgradr | wgrad8p
    dtype: str = "bf16"
    pws: int = 0                # wgrad3x3: log2 of the strip row's slots
    wide: bool = False          # wgradr: <2, 8>
    transposed: bool = False    # wgradr: the 256-channel tiles on X
    direct: bool = False        # generic: the store in the compute dtype (nkb_gemm_tn_batched)

    @property
    def code(self):
        v = {"generic": int(self.dtype == "bf16") | int(self.direct) << 1, "wgrad3x3": self.pws,
             "wgradr": int(self.wide) | int(self.transposed) << 1, "wgrad8p": 0}[self.family]
        return FAMILY[self.family] | v << 4

    def __str__(self):
        return {"generic": f"conv_wgrad_kernel<{self.dtype}>{' direct store' if self.direct else ''}",
                "wgrad3x3": f"wgrad3x3p_kernel<{self.pws},3>",
                "wgradr": f"wgradr_kernel<{'2,8' if self.wide else '3,4'}>{' transposed' if self.transposed else ''}",
                "wgrad8p": "wgrad8p_kernel"}[self.family]


def decode(code: int) -> dict:
    """the fields of nkb_wgrad_last_kernel's answer"""
    return dict(kern=code & 0xFF, slabs=bool(code >> 8 & 1), reduce=code >> 9 & 7, assign=bool(code >> 12 & 1), two=bool(code >> 13 & 1),
                splits=code >> 16)


GB, GF = Kern("generic", "bf16"), Kern("generic", "f32")
GBD, GFD = Kern("generic", "bf16", direct=True), Kern("generic", "f32", direct=True)
W3 = {p: Kern("wgrad3x3", pws=p) for p in (3, 4, 5, 6)}
WR, WRT, WRW = Kern("wgradr"), Kern("wgradr", transposed=True), Kern("wgradr", wide=True)
W8 = Kern("wgrad8p")
# every kernel the dispatch can produce, written out from it (the wide form exists only in the plain orientation: it needs both
# channel counts in multiples of 256, and those take the plain branch of wr_plan)
KERNELS = (GB, GF, GBD, GFD, W3[3], W3[4], W3[5], W3[6], WR, WRT, WRW, W8)
# (reduce kernel, assigned, two ranges) that the GPU cases must reach between them.  wgrad_reduce_kernel's tail for n % 4 != 0 is
# not in the list: every caller passes n == slab, and a slab that is no multiple of 4 goes to the scalar kernel — no entry reaches it.
REDUCES = ((1, False, False), (2, False, False), (3, False, False), (4, False, False), (1, True, False), (2, True, False),
           (3, True, False), (4, True, False), (2, False, True), (2, True, True))


# ---- cases -----------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Case:
    """One weight gradient.  entry conv: x [N][H][W][Cin], dY [N][P][Q][Cout] (GEMM-shaped: N = rows, H = W = 1); stem: the image is
    N x H x W (x 4 channels, packed); tn: N = the rows summed, Cout = Na, Cin = Nb, batch = (outer, inner)."""
    name: str
    entry: str                  # conv | stem | tn
    kern: Kern
    N: int
    H: int
    W: int
    Cin: int
    Cout: int
    R: int = 1
    S: int = 1
    stride: int = 1
    pad: int = 0
    bias: bool = False
    pads: tuple = (8, 8)        # ldx - Cin, lddy - Cout
    batch: tuple = (1, 1)
    unaligned: bool = False     # dw and dbias one float off a 16-byte boundary
    reserve: int = 0            # nkb_rowres_reserve_cus while the case runs
    wide_m: bool = False        # N is the smallest row count of the wide wgradr form for the chip's CU count (resolve)
    search_m: bool = False      # N is found by the NKB_WGRAD256=2 child as the smallest eligible row count
    big: bool = False           # the CPU proof leaves the costly mutants of this case out

    @property
    def dtype(self):
        return self.kern.dtype


@dataclass(frozen=True)
class Geo:
    Hx: int
    Wx: int
    Cin: int
    R: int
    S: int
    sh: int
    sw: int
    ph: int
    pw: int
    P: int
    Q: int
    M: int
    Ntot: int
    ldx: int
    lddy: int
    xrows: int


def _up(v, m):
    return -(-v // m) * m


def geom(c: Case) -> Geo:
    epc = 8 if c.dtype == "bf16" else 4
    if c.entry == "stem":
        cprw = 4 if c.dtype == "bf16" else 8
        Wc = _up(c.W, 2) * 4 // epc
        sw, pw = (1, 2) if c.dtype == "bf16" else (2, 3)
        P, Q = (c.H - 1) // 2 + 1, (c.W - 1) // 2 + 1
        return Geo(c.H, Wc, epc, 7, cprw, 2, sw, 3, pw, P, Q, c.N * P * Q, 7 * cprw * epc, epc, _up(c.Cout, epc) + c.pads[1], c.N * c.H * Wc)
    if c.entry == "tn":
        return Geo(c.N, 1, c.Cin, 1, 1, 1, 1, 0, 0, c.N, 1, c.N, c.Cin, c.Cin + c.pads[0], _up(c.Cout, epc) + c.pads[1], c.N)
    P, Q = (c.H + 2 * c.pad - c.R) // c.stride + 1, (c.W + 2 * c.pad - c.S) // c.stride + 1
    return Geo(c.H, c.W, c.Cin, c.R, c.S, c.stride, c.stride, c.pad, c.pad, P, Q, c.N * P * Q, c.R * c.S * c.Cin, c.Cin + c.pads[0],
               _up(c.Cout, epc) + c.pads[1], c.N * c.H * c.W)


def min_wide_m(c: Case, cus: int) -> int:
    """smallest row count at which wr_plan (csrc/wgradr.hip) takes the wide form: rows per split, rounded up to 32, >= 2048 at
    (CUs - reserve) / tiles splits of 256 x 256 tiles; + 1 keeps it off a multiple of 32"""
    tiles = (c.Cout // 256) * (c.Cin // 256)
    sp = max(1, (cus - c.reserve) // tiles)
    return 2016 * sp + 1


def resolve(c: Case, cus: int = 256, found_m: Optional[int] = None) -> Case:
    """the case with its row count filled in where that depends on the chip (wide_m) or on a search (search_m)"""
    if c.wide_m:
        return replace(c, N=min_wide_m(c, cus))
    if c.search_m and found_m is not None:
        return replace(c, N=found_m)
    return c


# ---- plans: the split of the pixels, restated from the launchers -------------------------------------------------------------------
@dataclass(frozen=True)
class Plan:
    splits: int
    bounds: tuple           # ((first row, end row) of every split)
    stage: int              # pixels of one pipeline stage
    tilesN: int             # column tiles of the generic kernel (bias partials = splits x tilesN)
    bias_parts: int


def _sg(n):
    return 3 if n >= 48 else 2 if n >= 6 else 1


def plan(c: Case, cus: int = 256) -> Plan:
    g = geom(c)
    M = g.M
    rng = lambda rows, splits: tuple((s * rows, min(M, (s + 1) * rows)) for s in range(splits))
    f = c.kern.family
    if f == "generic":
        tw = 128 if c.dtype == "bf16" else 64
        tilesC, tilesN = -(-c.Cout // tw), -(-g.Ntot // tw)
        if c.entry == "tn":
            return Plan(1, ((0, M),), 64, tilesN, 0)
        target = 768 if c.entry == "stem" else 256
        splits = max(1, min(-(-target // (tilesC * tilesN)), (M + 255) // 256))
        rps = _up(-(-M // splits), 64)
        splits = -(-M // rps)
        return Plan(splits, rng(rps, splits), 64, tilesN, splits * tilesN)
    if f == "wgrad3x3":
        pw = 1 << c.kern.pws
        ks = -(-(c.N * (c.H + 1) * pw) // 64)
        tiles = (c.Cout // 64) * (c.Cin // 64)
        sp = -(-256 // tiles)
        if sp > ks // 4:
            sp = max(ks // 4, 1)
        per = -(-ks // sp)
        splits = -(-ks // per)
        # a model of the split in pixel space: pixel (n, h, w) sits in strip slot (n (H + 1) + h) pw + w, a split owns per * 64 slots
        m = torch.arange(M)
        n, rem = m // (c.H * c.W), m % (c.H * c.W)
        sid = (((n * (c.H + 1) + rem // c.W) * pw + rem % c.W) // (per * 64)).tolist()
        bounds = tuple((sid.index(s) if s in sid else M, M - sid[::-1].index(s) if s in sid else M) for s in range(splits))
        return Plan(splits, bounds, 64, 1, 0)
    if f == "wgradr":
        if c.kern.transposed:
            ntile = (c.Cin // 256) * (c.Cout // 128)
        else:
            ntile = (c.Cout // 256) * (c.Cin // 128)
        if c.kern.wide:
            ntile //= 2
        sp = max(1, (cus - c.reserve) // ntile)
        rows = max(256, _up(-(-M // sp), 32))
        splits = -(-M // rows)
        return Plan(splits, rng(rows, splits), 32, 1, splits)
    tiles = (c.Cout // 256) * (c.Cin // 256)
    target = 128 if 2.0 * M * 65536.0 * tiles < 220.0e9 else 256
    stages = M // 64
    splits = min(max(1, (target + tiles // 2) // tiles), stages)
    sps = -(-stages // splits)
    splits = -(-stages // sps)
    return Plan(splits, rng(sps * 64, splits), 64, 1, splits)


def expected_reduce(c: Case, pl: Plan, assign: bool):
    """(reduce kernel, assigned, two ranges) of the LAST reduce launch of the case's slab / assign form"""
    f = c.kern.family
    if c.bias:
        if f == "wgradr":                                   # one launch for the weight slabs and the bias partials
            return (_sg(pl.splits), assign, True)
        parts = pl.bias_parts
        return (4 if (c.Cout % 4 or c.unaligned) else _sg(parts), assign, False)
    return (4 if c.unaligned else _sg(pl.splits), assign, False)


# ---- operands ----------------------------------------------------------------------------------------------------------------------
@dataclass
class Data:
    """Operands of one case, unpadded: x / dy in the compute dtype, the previous contents of dw / dbias in fp32"""
    x: torch.Tensor                 # [rows of x][Cin]            (tn: [Z][M][Nb])
    dy: torch.Tensor                # [M][Cout]                   (tn: [Z][M][Na])
    pre_dw: torch.Tensor            # [Cout][Ntot] fp32           (tn: unused)
    pre_db: Optional[torch.Tensor]  # [Cout] fp32


def make(c: Case, device, regime: str, seed: int = 0) -> Data:
    g = torch.Generator(device=device).manual_seed(seed)
    dt = TORCH_DT[c.dtype]
    ge = geom(c)
    if regime == "exact":
        val = lambda *s: torch.randint(-2, 3, s, generator=g, device=device).to(dt)
        pre = lambda *s: torch.randint(-3, 4, s, generator=g, device=device).float()
    else:
        val = lambda *s: torch.randn(*s, generator=g, device=device).abs().to(dt)
        pre = lambda *s: torch.randn(*s, generator=g, device=device).abs()
    Z = c.batch[0] * c.batch[1]
    if c.entry == "tn":
        return Data(val(Z, ge.M, c.Cin), val(Z, ge.M, c.Cout), pre(1, 1), None)
    return Data(val(ge.xrows, ge.Cin), val(ge.M, c.Cout), pre(c.Cout, ge.Ntot), pre(c.Cout) if c.bias else None)


# ---- the gather --------------------------------------------------------------------------------------------------------------------
def _cr_case(c: Case):
    return cr.Case(c.name, "conv_gemm", None, c.N, c.H, c.W, c.Cin, c.Cout, c.R, c.S, c.stride, c.pad, 0)


def gather_general(c: Case, device, mutant=None):
    """conv_reference.gather_index (mode 0) with separate vertical / horizontal stride and padding (the packed stem's view)"""
    g = geom(c)
    m = torch.arange(g.M, device=device)
    n, rem = m // (g.P * g.Q), m % (g.P * g.Q)
    pp, qq = rem // g.Q, rem % g.Q
    sh, sw = (1, 1) if mutant == "stride_ignored" else (g.sh, g.sw)
    src, val = [], []
    for r in range(g.R):
        for s in range(g.S):
            hs, ws = pp * sh + r - g.ph, qq * sw + s - g.pw
            if mutant == "tap_shifted" and r * g.S + s == (g.R * g.S) // 2:       # the middle tap reads its right neighbour's column
                ws = ws + 1
            ok = (hs >= 0) & (hs < g.Hx) & (ws >= 0) & (ws < g.Wx)
            flat = (n * g.Hx + hs) * g.Wx + ws
            src.append(torch.where(ok, flat, torch.zeros_like(flat)))
            val.append(ok)
    return torch.stack(src, 1), torch.stack(val, 1)


def gather_index(c: Case, device, mutant=None):
    """(src [M][R*S] flat pixel of x, valid [M][R*S]); the square-stride convolutions take conv_reference's"""
    if c.entry == "conv" and mutant in (None, "halo_wrap", "image_bleed", "hw_swapped"):
        return cr.gather_index(_cr_case(c), device, mutant)
    return gather_general(c, device, mutant)


def _trunc_bf16(t):
    return (t.float().contiguous().view(torch.int32) & -65536).view(torch.float32)


def rows(c: Case, d: Data, mutant=None, z=0):
    """(X [M][Ntot], dY [M][Cout]) in float64"""
    x, dy = (d.x[z], d.dy[z]) if c.entry == "tn" else (d.x, d.dy)
    if mutant == "batch_stride_swapped":                   # slice (zo, zi) of A read at zo * inner-stride + zi * outer-stride
        outer, inner = c.batch
        dy = d.dy[(z % inner * inner + z // inner) % (outer * inner)]
    if mutant == "f32_operands_bf16":
        x, dy = _trunc_bf16(x), _trunc_bf16(dy)
    if c.entry == "tn":
        return x.double(), dy.double()
    src, val = gather_index(c, x.device, mutant)
    return (x.double()[src] * val[:, :, None]).reshape(src.shape[0], -1), dy.double()


def mutant_exists(c: Case, form: str, mutant: str, pl: Plan) -> bool:
    g = geom(c)
    conv = c.entry == "conv"
    slabs = form in ("slab", "assign")
    tw = 128 if c.dtype == "bf16" else 64
    return {
        "drop_pixel": True,
        "stale_stage": pl.bounds[0][1] - pl.bounds[0][0] >= 2 * pl.stage,
        "tail_rows_read": True,
        "pad_columns_read": g.lddy > c.Cout,
        "split_dropped": pl.splits >= 2 and form != "direct",
        "split_twice": pl.splits >= 2 and form != "direct",
        "empty_split_garbage": slabs and any(b <= a for a, b in pl.bounds),
        "tap_shifted": g.R * g.S > 1,
        "halo_wrap": conv and c.S == 3 and c.stride == 1 and c.pad == 1 and c.W > 1 and c.H * c.N > 1,
        "image_bleed": conv and c.R == 3 and c.pad == 1 and c.N > 1 and c.stride == 1,
        "hw_swapped": conv and c.H != c.W and not (c.R == 1 and c.S == 1 and c.stride == 1),
        "stride_ignored": g.sh > 1 or g.sw > 1,
        "transposed_result": True,
        "cout_tail_dropped": c.Cout % 8 != 0,
        "ntot_tail_dropped": g.Ntot % tw != 0,
        "row_tail_written": True,
        "bias_one_tile": c.bias and c.kern.family == "generic" and pl.tilesN >= 2,
        "bias_not_reduced": c.bias and slabs and pl.bias_parts >= 2,
        "assign_accumulates": form == "assign",
        "accumulate_assigns": form == "slab",
        "batch_stride_swapped": c.entry == "tn",
        "acc_bf16": c.dtype == "bf16" and g.M > pl.stage,
        "f32_operands_bf16": c.dtype == "f32",
    }[mutant]


# ---- the reference -----------------------------------------------------------------------------------------------------------------
def _partials(X, DY, pl: Plan, per_stage: Optional[str] = None):
    """[S][Cout][Ntot] float64: every split's product; per_stage "f32" / "bf16": the accumulator is rounded after every stage"""
    out = []
    for a, b in pl.bounds:
        if per_stage is None or b <= a:
            out.append(DY[a:b].t() @ X[a:b])
            continue
        acc = torch.zeros(DY.shape[1], X.shape[1], dtype=torch.float64, device=X.device)
        for s0 in range(a, b, pl.stage):
            acc = acc + DY[s0:min(b, s0 + pl.stage)].t() @ X[s0:min(b, s0 + pl.stage)]
            acc = bf(acc) if per_stage == "bf16" else acc.float().double()
        out.append(acc)
    return torch.stack(out)


def _bias_partials(DY, pl: Plan):
    """[splits * tilesN][Cout]: column tile t of the generic kernel sums dY over the stages st of its split with st % tilesN == t"""
    out = []
    for a, b in pl.bounds:
        m = torch.arange(a, max(a, b), device=DY.device)
        for t in range(pl.tilesN):
            out.append(DY[a:max(a, b)][((m - a) // pl.stage) % pl.tilesN == t].sum(0))
    return torch.stack(out)


def reference(c: Case, d: Data, form: str, mutant: Optional[str] = None, pl: Optional[Plan] = None, *, rounded: Optional[str] = None):
    """What a launch of `form` must leave: dict(dw [Z * Cout][Ntot], dbias [Cout] or None, past) in float64, with `mutant` applied
    (None where it does not exist).  rounded None: exact float64, the reference.  "split" / "stage": the yardstick — partial sums
    rounded to fp32 per split / per stage, the reduce, the addition of the previous contents and the store rounded the way the
    kernels round."""
    pl = pl or plan(c)
    if mutant is not None and not mutant_exists(c, form, mutant, pl):
        return None
    g = geom(c)
    f32 = (lambda t: t.float().double()) if rounded else (lambda t: t)
    Z = c.batch[0] * c.batch[1]
    dws = []
    dbias = None
    for z in range(Z):
        X, DY = rows(c, d, mutant, z)
        per_stage = "bf16" if mutant == "acc_bf16" else "f32" if rounded == "stage" else None
        parts = _partials(X, DY, pl, per_stage)
        if rounded == "split":
            parts = f32(parts)
        bparts = _bias_partials(DY, pl)                                            # [splits * tilesN][Cout]
        if mutant == "drop_pixel":                          # the last pixel of the last split is missing
            parts[-1] -= torch.outer(DY[-1], X[-1])
        elif mutant == "stale_stage":                       # stage 1 of split 0 multiplies dY by stage 0's X rows
            a, st = pl.bounds[0][0], pl.stage
            parts[0] += DY[a + st:a + 2 * st].t() @ (X[a:a + st] - X[a + st:a + 2 * st])
        elif mutant == "tail_rows_read":                    # the GR rows of garbage behind row M take part
            parts[-1] += GR * GARBAGE * GARBAGE
            bparts[-1] += GR * GARBAGE
        elif mutant == "pad_columns_read":                  # the channel after the last one is a padding column of dY
            parts[:, -1] += GARBAGE * torch.stack([X[a:b].sum(0) for a, b in pl.bounds])
            bparts[-1, -1] += GARBAGE * g.M
        elif mutant == "split_dropped":
            parts[1] = 0
        elif mutant == "split_twice":
            parts[1] *= 2
        elif mutant == "empty_split_garbage":               # an unwritten slab: whatever the workspace held (the test fills it with NaN)
            for s, (a, b) in enumerate(pl.bounds):
                if b <= a:
                    parts[s] = float("nan")
        elif mutant == "bias_one_tile":                     # only the stages that column tile 0 owns (stage % tilesN == 0) are summed
            bparts.reshape(pl.splits, pl.tilesN, -1)[:, 1:] = 0
        elif mutant == "bias_not_reduced":                  # only the first partial reaches dbias
            bparts[1:] = 0
        # the sum over the splits, in split order
        tot, btot = parts[0], bparts[0]
        for s in range(1, parts.shape[0]):
            tot = f32(tot + parts[s])
        for s in range(1, bparts.shape[0]):
            btot = f32(btot + bparts[s])
        if mutant == "transposed_result":
            tot = tot.t().contiguous().reshape(tot.shape)
        elif mutant == "cout_tail_dropped":
            tot = tot.clone()
            tot[c.Cout // 8 * 8:] = 0
        elif mutant == "ntot_tail_dropped":
            tw = 128 if c.dtype == "bf16" else 64
            tot = tot.clone()
            tot[:, g.Ntot // tw * tw:] = 0
        if form == "direct":
            dws.append(bf(tot) if c.dtype == "bf16" else tot)          # stored once, in the compute dtype
            continue
        adds = (form != "assign") != (mutant in ("assign_accumulates", "accumulate_assigns"))
        dws.append(f32(tot + d.pre_dw.double()) if adds else tot)
        if c.bias:
            dbias = f32(btot + d.pre_db.double()) if adds else btot
    return dict(dw=torch.cat(dws), dbias=dbias, past=mutant == "row_tail_written")


def totals(c: Case, d: Data, form: str, pl: Optional[Plan] = None):
    """the unrounded float64 result before the direct store's rounding: what the positive-regime bound scales with"""
    pl = pl or plan(c)
    Z = c.batch[0] * c.batch[1]
    adds = form in ("slab", "atomic")
    tw, tb = [], None
    for z in range(Z):
        X, DY = rows(c, d, None, z)
        t = DY.t() @ X
        tw.append(t + d.pre_dw.double() if adds else t)
        if c.bias:
            tb = DY.sum(0) + (d.pre_db.double() if adds else 0)
    return torch.cat(tw), tb


# ---- the verdicts ------------------------------------------------------------------------------------------------------------------
def bound(c: Case, total: torch.Tensor, K: int, S: int, direct: bool = False) -> torch.Tensor:
    """the positive-regime bound (derived in the module docstring)"""
    e = A_MFMA * (K + S + 1 + int(c.dtype == "f32")) * U * total
    return R_BF16 * (total + e) + e if direct and c.dtype == "bf16" else e


def verdict(c: Case, d: Data, regime: str, form: str, got: dict, pl: Optional[Plan] = None, want: Optional[dict] = None,
            tot=None) -> dict:
    """{check: (ratio, err, bound)}; a ratio <= 1 passes.  exact: the bound is 0 and the ratio 0 or inf (bit equality with the
    float64 reference).  got: dw [Z * Cout][Ntot] and dbias [Cout] in float64, past (something outside the outputs was written)."""
    pl = pl or plan(c)
    g = geom(c)
    res = {}
    if regime == "exact":
        want = want or reference(c, d, form, pl=pl)
        for k in ("dw", "dbias"):
            if want[k] is None:
                continue
            bad = ~(got[k] == want[k])
            err = torch.nan_to_num((got[k] - want[k]).abs(), nan=math.inf).max().item()
            res[k] = (math.inf if bool(bad.any()) else 0.0, err, 0.0)
    else:
        tw, tb = tot or totals(c, d, form, pl)
        for k, t, S in (("dw", tw, pl.splits), ("dbias", tb, pl.bias_parts)):
            if t is None:
                continue
            bnd = bound(c, t, g.M, S, form == "direct")
            err = torch.nan_to_num((got[k] - t).abs(), nan=math.inf)
            q = err / bnd.clamp_min(1e-300)
            i = int(q.argmax())
            res[k] = (q.flatten()[i].item(), err.flatten()[i].item(), bnd.flatten()[i].item())
    res["guard"] = (math.inf if got.get("past") else 0.0, 0.0, 0.0)
    return res


def rejecting(c: Case, d: Data, regime: str, form: str, mutant: str, pl: Optional[Plan] = None):
    """the checks that reject the reference with `mutant` applied, as {check: ratio}; None where the mutant does not exist"""
    pl = pl or plan(c)
    mut = reference(c, d, form, mutant, pl)
    if mut is None:
        return None
    return {k: v[0] for k, v in verdict(c, d, regime, form, mut, pl).items() if not v[0] <= 1.0}


def forms(c: Case):
    """the forms a case's entry has, in the order the GPU test runs them"""
    return ("direct",) if c.entry == "tn" else ("slab", "atomic") if c.entry == "stem" else ("slab", "assign", "atomic")


# ---- the case table ----------------------------------------------------------------------------------------------------------------
K3, K3S2, K1S2, K7 = (3, 3, 1, 1), (3, 3, 2, 1), (1, 1, 2, 0), (7, 7, 2, 3)


def _conv(name, kern, N, H, W, Cin, Cout, k=(1, 1, 1, 0), **kw):
    return Case(name, "conv", kern, N, H, W, Cin, Cout, *k, **kw)


def _gemm(name, kern, M, Cin, Cout, **kw):
    return Case(name, "conv", kern, M, 1, 1, Cin, Cout, **kw)


CASES = (
    # ---- conv_wgrad_kernel<bf16> through nkb_conv_wgrad / _assign: non-square maps, channel tails, a partial last column tile ----
    _conv("g_3x3_b_1split", GB, 2, 7, 9, 24, 44, K3),                                   # M = 126: one split, Ntot = 9 * 24
    _conv("g_3x3_b_2splits", GB, 2, 11, 13, 24, 44, K3, bias=True),                     # M = 286: a ragged second split
    _conv("g_3x3s2_b_bias", GB, 2, 11, 13, 136, 140, K3S2, bias=True),                  # 10 column tiles: bias partials on <4>
    _conv("g_1x1s2_b_cout46_bias", GB, 3, 11, 13, 64, 46, K1S2, bias=True),             # Cout % 4 != 0: the scalar reduce
    _conv("g_7x7s2_b", GB, 2, 11, 13, 8, 44, K7),
    _conv("g_3x3_b_8splits", GB, 2, 29, 31, 24, 140, K3, bias=True, pads=(16, 16)),     # M = 1798: wgrad_reduce_kernel<4>
    _gemm("g_1x1_b_49splits", GB, 48 * 256 + 37, 64, 64),                               # wgrad_reduce_kernel<16>
    _conv("g_3x3_b_unaligned", GB, 2, 11, 13, 24, 44, K3, bias=True, unaligned=True),
    # ---- conv_wgrad_kernel<float> ----
    _conv("g_3x3_f_bias", GF, 2, 11, 13, 12, 44, K3, bias=True),
    _conv("g_3x3s2_f", GF, 2, 11, 13, 36, 140, K3S2),
    _conv("g_1x1s2_f_cout46_bias", GF, 3, 11, 13, 32, 46, K1S2, bias=True),
    _conv("g_7x7s2_f", GF, 2, 11, 13, 4, 44, K7, pads=(16, 16)),
    _gemm("g_1x1_f_8splits", GF, 1798, 136, 140, bias=True),
    _gemm("g_1x1_f_49splits", GF, 48 * 256 + 37, 64, 64, bias=True),
    _conv("g_3x3_f_unaligned", GF, 2, 7, 9, 12, 44, K3, unaligned=True),
    # ---- conv_wgrad_kernel through nkb_stem_wgrad: odd width ----
    Case("stem_b", "stem", GB, 2, 23, 29, 8, 64),
    Case("stem_f", "stem", GF, 2, 23, 29, 4, 64),
    Case("stem_b_cout44", "stem", GB, 3, 12, 10, 8, 44),
    # ---- conv_wgrad_kernel through nkb_gemm_tn_batched: outer 2 x inner 3, distinct strides, a tail in Na with lda = roundup(Na) ----
    Case("tn_b_197", "tn", GBD, 197, 1, 1, 72, 44, batch=(2, 3), pads=(8, 0)),
    Case("tn_b_70", "tn", GBD, 70, 1, 1, 64, 140, batch=(2, 3), pads=(8, 0)),
    Case("tn_f_197", "tn", GFD, 197, 1, 1, 36, 42, batch=(2, 3), pads=(8, 0)),
    Case("tn_f_70", "tn", GFD, 70, 1, 1, 72, 68, batch=(2, 3), pads=(8, 0)),
    # ---- wgrad3x3p_kernel<3 | 4 | 5 | 6, 3>: full strip rows at W = 7 / 15 / 31, W = 62, non-square maps, one k-step ----
    _conv("w3_pws3_7x7", W3[3], 3, 7, 7, 128, 64, K3),
    _conv("w3_pws4_15x15", W3[4], 5, 15, 15, 64, 64, K3),
    _conv("w3_pws5_31x31", W3[5], 2, 31, 31, 64, 64, K3),
    _conv("w3_pws6_62x62", W3[6], 1, 62, 62, 64, 64, K3, pads=(16, 16)),
    _conv("w3_pws5_8x20", W3[5], 2, 8, 20, 64, 64, K3),
    _conv("w3_pws3_12x5", W3[3], 7, 12, 5, 64, 128, K3),
    _conv("w3_pws3_one_kstep", W3[3], 1, 7, 7, 64, 64, K3),
    _conv("w3_pws4_9x9_192", W3[4], 3, 9, 9, 64, 192, K3),
    _conv("w3_pws4_14x14_192in", W3[4], 2, 14, 14, 192, 64, K3),
    # ---- wgradr_kernel<3, 4> plain and transposed, <2, 8> ----
    _gemm("wr_128to256_bias", WR, 4096 + 33, 128, 256, bias=True),                      # a last split of 33 rows: a ragged stage
    _gemm("wr_256to128_t_oddstages", WRT, 4096 + 70, 256, 128),                         # a last split of 70 rows: 3 stages + the zero one
    _gemm("wr_384to256_bias_oddstages", WR, 4096 + 70, 384, 256, bias=True, pads=(16, 16)),
    _gemm("wr_256to384_t", WRT, 4096 + 33, 256, 384),
    _gemm("wr_wide_1024to512_bias", WRW, 0, 1024, 512, bias=True, reserve=128, wide_m=True, big=True),
)
# the NKB_WGRAD256=2 child's cases (tests/wgrad8p_probe.py)
PROBE_CASES = (
    _gemm("w8_1024to1024_bias", W8, 4096, 1024, 1024, bias=True, search_m=True, big=True),
    _gemm("w8_256to512", W8, 4096, 256, 512, search_m=True, pads=(16, 16), big=True),
)
FAMILIES = ("conv_bf16", "conv_f32", "stem", "tn", "wgrad3x3", "wgradr", "wgrad8p")


def family_of(c: Case) -> str:
    if c.kern.family != "generic":
        return c.kern.family
    return c.entry if c.entry != "conv" else "conv_" + c.dtype


__all__ = ["Case", "Kern", "Plan", "Data", "CASES", "PROBE_CASES", "KERNELS", "REDUCES", "MUTANTS", "REJECTED_BY", "INDEXING_MUTANTS",
           "FAMILIES", "family_of", "geom", "plan", "resolve", "min_wide_m", "make", "rows", "gather_index", "gather_general",
           "reference", "totals", "bound", "verdict", "rejecting", "forms", "expected_reduce", "decode", "mutant_exists", "GARBAGE",
           "GR", "REDUCE_NAME"]
