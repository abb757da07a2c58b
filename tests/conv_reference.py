"""Float64 reference of the implicit-GEMM convolution family (csrc/conv_igemm.hip: conv_igemm_kernel<T, TC, TP, BNB, HALO> behind
nkb_conv_gemm, nkb_conv_dgrad_bn, nkb_conv_dgrad_s2class, nkb_conv_affine_residual, nkb_conv_cat_relu_bits, nkb_conv_cat_bias,
nkb_conv_dgrad_bn_cat, nkb_conv_dgrad_bn_add, nkb_gemm_batched and nkb_linear_gelu), the rounding yardstick, the derived bounds
that tests/test_conv_igemm_gpu.py holds every kernel instance to, mutants that make the yardstick wrong the way this kernel goes
wrong, and the case table both test files walk.  tests/test_conv_reference.py proves on the CPU that the reference equals torch's
convolution and its autograd in float64 and that the bounds reject every mutant.  No test lives here.

The operation (include/nkbhip.h).  Every launch is rows . w^T with rows an explicit gather of filter taps:
    mode 0:  rows[m][(r, s, ci)] = x[n, p*stride + r - pad, q*stride + s - pad, ci]              m = (n, p, q)
    mode 1:  rows[m][(r, s, ci)] = x[n, (h + pad - r) / stride, (w + pad - s) / stride, ci]      m = (n, h, w), non-integral skipped
    class (ph, pw) of the stride-2 data gradient: mode 1 at stride 1 with pad (ph, pw) over (1|2) x (1|2) taps; row m = (n, h', w')
        of the class lands in row (n, 2h' + ph, 2w' + pw) of the full grid
    K-concatenated: rows = [a | x];   batched: slice z = zo * inner + zi at element offsets zo * s?o + zi * s?i
and the epilogue in the kernel's order: + bias; + the residual operand (full grid, under add_bits, or on the even sub-grid
add_h x add_w); the BN mask, recomputed as rnd(c * scale + shift) > 0 or read from the bit array; ReLU / ReLU6 / act 1 to 4; or
the affine closing stage relu(acc * oscale + shift + res') with res' = rnd(res * res_scale + res_shift); the store in the compute
dtype or in fp32.  Second outputs: per-row-tile sums of y and y^2 (BN epilogues: of g' and g' * (c - mean)) and the ReLU bit mask
of the stored y, a byte per 8 channels in bf16 and per 4 channels in fp32.

The yardstick is the same math done the way the kernel does it: the float64 product rounded to fp32, the epilogue in fp32, bf16
rounding exactly where the kernel rounds.

The bounds (derived; none is measured on the code under test):
  element   |got - ref| <= r (|ref| + e) + e,  r = 2^-8 for a bf16 store and 0 for an fp32 store (bf16 carries 8 significant bits:
            round to nearest is off by up to 2^-8 of a value just above a power of two and by 2^-9 only just below the next one, so
            2^-9 would reject correctly rounded results — tests/test_conv_reference.py shows one).  e starts as A K 2^-24 (|x| . |w|)
            with K the number of accumulated terms (K roundings of partial sums that never exceed |x| . |w|), and every epilogue
            operation adds one fp32 ulp of its result and scales e by its Lipschitz constant.  A = 2 is an ALLOWANCE for the MFMA's
            internal summation order, which nobody here has measured; with random data the typical error sits about sqrt(K) below
            the bound, so A decides no verdict.
  tile      the instance's own TP pixels x TC channels, tiles of at least 4096 elements (smaller edge tiles rest on the element
            bound), bf16 stores only: relative Frobenius error against the float64 reference <= max(C_BOUND * yardstick error, FLOOR)
            with both constants from tests/gemm_reference.py.
  stats     against float64 sums of the kernel's OWN stored output (and the given c, mean): |got - sum| <= TP 2^-24 sum |terms| per
            channel and tile.  A tile's sum is a chain of at most TP fp32 additions, each off by at most 2^-24 of a partial sum that
            never exceeds sum |terms| (the kernel's chain is shorter: per-thread rows, then 256 / (TC / 8) partials; the rounding of
            each product and of c - mean fits in the difference).  A sum over unrounded values misses it by an order of magnitude.
  bits      bit-exact against the stored output.
  BN mask   an element whose float64 |c scale + shift| is below 2^-20 (|c scale| + |shift|) may fall on either side and is left
            out; at most 1e-3 of a case's elements may be (expected with normal data: about 1e-6).
"""
import math
from dataclasses import dataclass, replace
from typing import Optional

import torch

from gemm_reference import C_BOUND, FLOOR, RMS_FLOOR, bf, tile_errors, tile_count

U = 2.0 ** -24                  # half an fp32 ulp, relative
A_MFMA = 2.0                    # allowance for the MFMA's internal summation order (see the docstring)
R_BF16 = 2.0 ** -8               # unit roundoff of bf16 (8 significant bits, round to nearest)
MIN_TILE = 4096                 # tiles below this many elements rest on the element bound
MASK_EDGE = 2.0 ** -20
MASK_SHARE = 1e-3
KTE = {"bf16": 64, "f32": 32}   # elements of one k-tile (128 bytes of a row)
TORCH_DT = {"bf16": torch.bfloat16, "f32": torch.float32}
EPI = dict(GENERAL=0, BN_MASK=1, BN_BITS=2, LEAN=3, AFFINE_BITS=4, BN_BITS_LEAN=6, BN_MASK_LEAN=7, LEAN_CAT=8)

MUTANTS = ("drop_tap", "stale_tap", "halo_wrap", "image_bleed", "hw_swapped", "parity_not_skipped", "class_row_unmapped",
           "subgrid_add_shifted", "add_bits_ignored", "bits_stride_cout", "kt2_off_by_one", "batch_stride_swapped", "bias_shift",
           "double_round", "stats_unrounded", "cout_tail_dropped", "row_tail_written")
# the output whose bound rejects each mutant (tests/test_conv_reference.py asserts exactly this)
REJECTED_BY = dict(drop_tap="y", stale_tap="y", halo_wrap="y", image_bleed="y", hw_swapped="y", parity_not_skipped="y",
                   class_row_unmapped="y", subgrid_add_shifted="y", add_bits_ignored="y", bits_stride_cout="y", kt2_off_by_one="y",
                   batch_stride_swapped="y", bias_shift="y", double_round="y", stats_unrounded="stats", cout_tail_dropped="y",
                   row_tail_written="guard")


# ---- instances -------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Inst:
    """conv_igemm_kernel<T, TC, TP, BNB, HALO>"""
    dtype: str
    tc: int            # 128 (x 128 pixels) or 64 (x 256 pixels)
    epi: str
    halo: bool = False

    @property
    def tp(self):
        return 128 if self.tc == 128 else 256

    @property
    def code(self):
        """what nkb_conv_last_instance answers after a launch of this instance on the plain tile walk"""
        return int(self.dtype == "bf16") | int(self.tc == 64) << 1 | int(self.halo) << 2 | EPI[self.epi] << 4

    def __str__(self):
        return f"conv_igemm_kernel<{self.dtype},{self.tc},{self.tp},EPI_{self.epi}{',HALO' if self.halo else ''}>"


GROUPED_BIT = 1 << 3
# Every instance launch_conv / launch_conv_tile can produce, written out from the dispatch (not computed from its rule):
#   fp32 has neither lean epilogues nor HALO, and no EPI_AFFINE_BITS / EPI_LEAN_CAT: three epilogues on two tiles
#   bf16: EPI_GENERAL, EPI_BN_MASK, EPI_BN_BITS and their lean forms, each with and without HALO on both tiles;
#         EPI_AFFINE_BITS on the 128 x 128 tile only, with and without HALO; EPI_LEAN_CAT (1x1 only: never HALO) on both tiles
INSTANCES = (
    Inst("f32", 128, "GENERAL"), Inst("f32", 64, "GENERAL"), Inst("f32", 128, "BN_MASK"), Inst("f32", 64, "BN_MASK"),
    Inst("f32", 128, "BN_BITS"), Inst("f32", 64, "BN_BITS"),
    Inst("bf16", 128, "GENERAL"), Inst("bf16", 128, "GENERAL", True), Inst("bf16", 64, "GENERAL"), Inst("bf16", 64, "GENERAL", True),
    Inst("bf16", 128, "LEAN"), Inst("bf16", 128, "LEAN", True), Inst("bf16", 64, "LEAN"), Inst("bf16", 64, "LEAN", True),
    Inst("bf16", 128, "BN_MASK"), Inst("bf16", 128, "BN_MASK", True), Inst("bf16", 64, "BN_MASK"), Inst("bf16", 64, "BN_MASK", True),
    Inst("bf16", 128, "BN_MASK_LEAN"), Inst("bf16", 128, "BN_MASK_LEAN", True), Inst("bf16", 64, "BN_MASK_LEAN"),
    Inst("bf16", 64, "BN_MASK_LEAN", True),
    Inst("bf16", 128, "BN_BITS"), Inst("bf16", 128, "BN_BITS", True), Inst("bf16", 64, "BN_BITS"), Inst("bf16", 64, "BN_BITS", True),
    Inst("bf16", 128, "BN_BITS_LEAN"), Inst("bf16", 128, "BN_BITS_LEAN", True), Inst("bf16", 64, "BN_BITS_LEAN"),
    Inst("bf16", 64, "BN_BITS_LEAN", True),
    Inst("bf16", 128, "AFFINE_BITS"), Inst("bf16", 128, "AFFINE_BITS", True),
    Inst("bf16", 128, "LEAN_CAT"), Inst("bf16", 64, "LEAN_CAT"),
)


# ---- cases -----------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Case:
    """One launch.  Convolutions: x [N][H][W][Cin] -> y over the grid (P, Q) (mode 1: H, W are dY's, out = the gradient's grid).
    GEMM-shaped entries (cat, dgrad_bn_add, batched, linear_gelu): N = 1, H = rows, W = 1.  Leading dimensions are C + the pad."""
    name: str
    entry: str              # conv_gemm dgrad_bn s2class affine cat_relu_bits cat_bias dgrad_bn_cat dgrad_bn_add batched linear_gelu
    inst: Inst
    N: int
    H: int
    W: int
    Cin: int
    Cout: int
    R: int = 1
    S: int = 1
    stride: int = 1
    pad: int = 0
    mode: int = 0
    out: Optional[tuple] = None     # mode 1 at stride 2 / parity class: the gradient's (Hout, Wout)
    cls: Optional[tuple] = None     # parity class (ph, pw)
    K2: int = 0                     # K-concatenated: channels of the second tensor (Cin = those of the first)
    batch: tuple = (1, 1)           # (outer, inner)
    epi: str = "plain"
    act: int = 0
    pads: tuple = (8, 8, 8)         # ldx - Cin, ldy - Cout, ldadd - Cout
    grouped: bool = False           # the launch takes the grouped tile walk

    @property
    def dtype(self):
        return self.inst.dtype


def dims(c: Case):
    """(P, Q, M, Mfull, pad_h, pad_w, Ktot): the launch's pixel grid, its rows, the rows of the tensor it writes into, its padding"""
    ph, pw = (c.cls if c.cls is not None else (c.pad, c.pad))
    if c.cls is not None:
        Ho, Wo = c.out
        P, Q = (Ho - c.cls[0] + 1) // 2, (Wo - c.cls[1] + 1) // 2
        return P, Q, c.N * P * Q, c.N * Ho * Wo, ph, pw, c.R * c.S * c.Cin
    if c.mode == 1:
        P, Q = c.out if c.out is not None else (c.H, c.W)
    else:
        P, Q = (c.H + 2 * c.pad - c.R) // c.stride + 1, (c.W + 2 * c.pad - c.S) // c.stride + 1
    return P, Q, c.N * P * Q, c.N * P * Q, ph, pw, c.R * c.S * c.Cin + c.K2


def class_taps(ph, pw):
    """filter rows / columns of a 3x3 stride-2 filter that reach parity class (ph, pw): r = (ph + 1) % 2 + 2 ri"""
    return ([0, 2] if ph else [1]), ([0, 2] if pw else [1])


def class_filter(wt: torch.Tensor, ph: int, pw: int) -> torch.Tensor:
    """[C][3][3][K] gather-form data-gradient filter -> the class's [C][Rc][Sc][K] (what nkb_wprep modes 2..5 lay out)"""
    rs, ss = class_taps(ph, pw)
    return wt[:, rs][:, :, ss].contiguous()


def out_rows(c: Case, device) -> Optional[torch.Tensor]:
    """row of the full grid that row m of a parity-class launch writes; None: row m itself"""
    if c.cls is None:
        return None
    P, Q, M, *_ = dims(c)
    m = torch.arange(M, device=device)
    n, rem = m // (P * Q), m % (P * Q)
    return (n * c.out[0] + 2 * (rem // Q) + c.cls[0]) * c.out[1] + 2 * (rem % Q) + c.cls[1]


@dataclass
class Data:
    """Operands of one case, unpadded, as tensors of the compute dtype (fp32 for the per-channel vectors)."""
    x: torch.Tensor                              # [N*H*W][Cin] (batched: [Z][M][K])
    w: torch.Tensor                              # [Cout][R*S*Cin + K2] (batched: [Z][N][K])
    x2: Optional[torch.Tensor] = None            # [M][K2]
    bias: Optional[torch.Tensor] = None          # [Cout] fp32 (affine: the shift)
    add: Optional[torch.Tensor] = None           # [rows of the add tensor][Cout]
    add_kind: str = "full"                       # full | sub
    add_hw: tuple = (0, 0)
    add_bits: Optional[torch.Tensor] = None      # [Mfull][Cout] bool
    relu: int = 0
    act: int = 0
    aux: Optional[torch.Tensor] = None           # act 2, 3, 4
    out_f32: bool = False
    stats: bool = False
    bn: Optional[str] = None                     # mask | bits
    c: Optional[torch.Tensor] = None             # [Mfull][Cout]
    scale: Optional[torch.Tensor] = None
    shift: Optional[torch.Tensor] = None
    mean: Optional[torch.Tensor] = None
    bn_bits: Optional[torch.Tensor] = None       # [Mfull][Cout] bool
    oscale: Optional[torch.Tensor] = None        # affine closing stage
    res_scale: Optional[torch.Tensor] = None
    res_shift: Optional[torch.Tensor] = None
    out_bits: bool = False


# ---- bit arrays ------------------------------------------------------------------------------------------------------------------
def pack_bits(mask: torch.Tensor, dtype: str, ld: int, fill: int = 0) -> torch.Tensor:
    """[rows][C] bool -> [rows][ld / chunk] bytes, chunk = 8 channels (bf16) / 4 (fp32): bit e of byte j = channel chunk * j + e;
    bytes past ceil(C / chunk) hold `fill`"""
    ch = 8 if dtype == "bf16" else 4
    rows, C = mask.shape
    nb = -(-C // ch)
    m = torch.zeros(rows, nb * ch, dtype=torch.int32, device=mask.device)
    m[:, :C] = mask.to(torch.int32)
    sh = torch.arange(ch, device=mask.device, dtype=torch.int32)
    out = torch.full((rows, ld // ch), fill, dtype=torch.uint8, device=mask.device)
    out[:, :nb] = (m.reshape(rows, nb, ch) << sh).sum(-1).to(torch.uint8)
    return out


def unpack_bits(bits: torch.Tensor, dtype: str, C: int) -> torch.Tensor:
    """[rows][>= ceil(C / chunk)] bytes -> [rows][C] bool"""
    ch = 8 if dtype == "bf16" else 4
    sh = torch.arange(ch, device=bits.device, dtype=torch.int32)
    nb = -(-C // ch)
    return ((bits[:, :nb].to(torch.int32)[:, :, None] >> sh) & 1).bool().reshape(bits.shape[0], -1)[:, :C]


def _restride_bits(mask, dtype, ld, C):
    """the bits a kernel sees that indexes a [rows][ld / chunk] bit array with C / chunk as its row stride"""
    ch = 8 if dtype == "bf16" else 4
    flat = pack_bits(mask, dtype, ld, fill=0xFF).flatten()
    rows = mask.shape[0]
    return unpack_bits(flat[:rows * (C // ch)].reshape(rows, C // ch), dtype, C)


# ---- the gather ------------------------------------------------------------------------------------------------------------------
def gather_index(c: Case, device, mutant=None):
    """(src [M][R*S] flat pixel of x, valid [M][R*S]) for every filter tap of every output row"""
    P, Q, M, _, pad_h, pad_w, _ = dims(c)
    m = torch.arange(M, device=device)
    n, rem = m // (P * Q), m % (P * Q)
    pp, qq = rem // Q, rem % Q
    src, val = [], []
    for r in range(c.R):
        for s in range(c.S):
            if c.mode == 0:
                hs, ws = pp * c.stride + r - pad_h, qq * c.stride + s - pad_w
                okh, okw = (hs >= 0) & (hs < c.H), (ws >= 0) & (ws < c.W)
            else:
                th, tw = pp + pad_h - r, qq + pad_w - s
                hs, ws = th // c.stride, tw // c.stride
                okh, okw = (th >= 0) & (hs < c.H), (tw >= 0) & (ws < c.W)
                if mutant != "parity_not_skipped":
                    okh, okw = okh & (th % c.stride == 0), okw & (tw % c.stride == 0)
            ok = okh & okw
            flat = (n * c.H + hs) * c.W + ws
            if mutant == "hw_swapped":
                flat = (n * c.W + hs) * c.H + ws
                ok = ok & (flat >= 0) & (flat < c.N * c.H * c.W)
            if mutant == "halo_wrap":                  # the left neighbour of an image row's first pixel: the pixel before it in memory
                wrap = okh & (ws == -1) & (flat >= 0)
                ok = ok | wrap
            if mutant == "image_bleed":                # the row above an image's first row: the previous image's last row
                ok = ok | ((hs == -1) & (n > 0) & okw)
            src.append(torch.where(ok, flat, torch.zeros_like(flat)))
            val.append(ok)
    return torch.stack(src, 1), torch.stack(val, 1)


def mutant_exists(c: Case, d: Data, mutant: str) -> bool:
    P, Q, M, Mfull, pad_h, pad_w, Ktot = dims(c)
    gemm = c.entry in ("cat_relu_bits", "cat_bias", "dgrad_bn_cat", "dgrad_bn_add", "batched", "linear_gelu")
    kt = Ktot // KTE[c.dtype]
    # (a sub-grid residual reaches only class (0, 0) of a parity-class launch)
    adds = d.add is not None and not (d.add_kind == "sub" and c.cls not in (None, (0, 0)))
    return {
        "drop_tap": True,
        "stale_tap": kt >= 2,
        "halo_wrap": not gemm and c.S == 3 and c.stride == 1 and pad_w == 1 and c.W > 1 and c.H * c.N > 1,
        "image_bleed": not gemm and c.R == 3 and pad_h == 1 and c.N > 1 and c.stride == 1,
        "hw_swapped": not gemm and c.H != c.W and not (c.R == 1 and c.S == 1 and c.stride == 1),
        "parity_not_skipped": c.mode == 1 and c.stride == 2,
        "class_row_unmapped": c.cls is not None,
        "subgrid_add_shifted": adds and d.add_kind == "sub",
        "add_bits_ignored": d.add_bits is not None,
        "bits_stride_cout": d.add_bits is not None or d.bn_bits is not None or d.out_bits,
        "kt2_off_by_one": c.K2 > 0,
        "batch_stride_swapped": c.entry == "batched",
        "bias_shift": d.bias is not None,
        "double_round": c.dtype == "bf16" and not d.out_f32 and (d.bias is not None or adds or d.oscale is not None
                                                                  or d.act in (1, 2, 4)),
        "stats_unrounded": d.stats and c.dtype == "bf16",
        "cout_tail_dropped": c.Cout % 8 != 0,
        "row_tail_written": True,
    }[mutant]


def _rows(c: Case, d: Data, mutant, z=None):
    """the gathered rows [M][Ktot] and the filter matrix [Cout][Ktot] in float64"""
    if c.entry == "batched":
        x, w = d.x[z], d.w[z]
        if mutant == "batch_stride_swapped":           # slice (zo, zi) read at zo * inner-stride + zi * outer-stride
            outer, inner = c.batch
            zo, zi = z // inner, z % inner
            x = d.x[(zi * inner + zo) % (outer * inner)]
        return x.double(), w.double()
    src, val = gather_index(c, d.x.device, mutant)
    xs = d.x.double()
    A = (xs[src] * val[:, :, None]).reshape(src.shape[0], -1)
    if d.x2 is not None:
        x2 = d.x2.double()
        if mutant == "kt2_off_by_one":                 # the second tensor's k-tiles start one k-tile late: the first reads nothing
            kte = KTE[c.dtype]
            x2 = torch.cat([torch.zeros_like(x2[:, :kte]), x2[:, :-kte]], 1)
        A = torch.cat([A, x2], 1)
    return A, d.w.double()


def _tile0(c: Case, M):
    """(rows, columns) of the output tile the k-tile mutants strike: the last row tile's first column tile"""
    tp, tc = c.inst.tp, c.inst.tc
    r0 = (M - 1) // tp * tp
    return slice(r0, M), slice(0, min(tc, c.Cout))


def _product(c: Case, A, Wm, exact, mutant, order):
    """(acc, |rows| . |w|): float64 (exact) or rounded to fp32 the way an accumulator holds it (order "ktile": fp32 partial sums per
    k-tile, added sequentially)"""
    kte = KTE[c.dtype]
    KT = A.shape[1] // kte
    if order == "ktile" and not exact:
        acc = torch.zeros(A.shape[0], Wm.shape[0], dtype=torch.float32, device=A.device)
        for k in range(KT):
            acc = acc + (A[:, k * kte:(k + 1) * kte] @ Wm[:, k * kte:(k + 1) * kte].t()).float()
        p = acc.double()
    else:
        p = A @ Wm.t()
    if mutant in ("drop_tap", "stale_tap"):
        rs, cs = _tile0(c, A.shape[0])
        k = KT // 2
        blk, prev = slice(k * kte, (k + 1) * kte), slice((k - 1) * kte, k * kte)
        p = p.clone()
        p[rs, cs] -= A[rs, blk] @ Wm[cs, blk].t()
        if mutant == "stale_tap":                      # this k-tile's activation tile is still the previous k-tile's
            p[rs, cs] += A[rs, prev] @ Wm[cs, blk].t()
    return (p if exact else p.float().double()), A.abs() @ Wm.abs().t()


def _gelu(v):
    cdf = 0.5 * (1 + torch.erf(v * (1 / math.sqrt(2))))
    return v * cdf, cdf + v * torch.exp(-0.5 * v * v) * (1 / math.sqrt(2 * math.pi))


def _add_rows(c: Case, d: Data, M, device, mutant):
    """(row of the add tensor, whether the row receives it, row of add_bits) for every launch row m"""
    P, Q, *_ = dims(c)
    m = torch.arange(M, device=device)
    orow = out_rows(c, device)
    full = m if orow is None else orow
    if d.add_kind == "full":
        return full, torch.ones(M, dtype=torch.bool, device=device), full
    if c.cls is not None:                               # the even (h, w) grid IS class (0, 0), row for row
        am, ok = m, torch.full((M,), c.cls == (0, 0), device=device)
    else:
        n, rem = m // (P * Q), m % (P * Q)
        hh, ww = rem // Q, rem % Q
        ok = (hh % 2 == 0) & (ww % 2 == 0)
        am = (n * d.add_hw[0] + hh // 2) * d.add_hw[1] + ww // 2
    if mutant == "subgrid_add_shifted":
        am = am + 1
    return am.clamp(0, d.add.shape[0] - 1), ok, full


def outputs(c: Case, d: Data, *, exact: bool, mutant: Optional[str] = None, order: Optional[str] = None):
    """One launch's outputs.  exact: float64 throughout, nothing rounded (the reference; it also carries the element bound's `e` and
    the mask elements `skip` that are left out).  Otherwise the yardstick, with `mutant` applied (None where it does not exist).
    y is [Mfull][Cout] float64 with NaN in the rows the launch does not write; stats [tiles][2][Cout]; bits [Mfull][Cout] bool."""
    if mutant is not None and not mutant_exists(c, d, mutant):
        return None
    P, Q, M, Mfull, *_ = dims(c)
    dev = d.x.device
    if mutant == "class_row_unmapped" and d.bn is not None:      # c taken at the launch row m instead of the remapped row
        c2 = d.c.clone()
        c2[out_rows(c, dev)] = d.c[:M]
        return outputs(c, replace(d, c=c2), exact=exact, order=order)
    lowp = c.dtype == "bf16"
    rnd = (lambda t: t) if exact or not lowp else bf
    f = (lambda t: t) if exact else (lambda t: t.float().double())         # one fp32 rounding of an fp32 operation's result
    Z = c.batch[0] * c.batch[1]
    accs, aps = [], []
    for z in range(Z):
        A, Wm = _rows(c, d, mutant, z)
        a, ap = _product(c, A, Wm, exact, mutant, order)
        accs.append(a), aps.append(ap)
    v, ap = torch.cat(accs), torch.cat(aps)
    K = A.shape[1]
    e = A_MFMA * K * U * ap
    ulp = lambda t: 2 * U * t.abs()
    out = {}
    if mutant == "double_round":
        v = bf(v)
    bias = d.bias.double() if d.bias is not None else None
    if mutant == "bias_shift":
        bias = torch.roll(bias, -1)
    orow = out_rows(c, dev)
    full = torch.arange(v.shape[0], device=dev) if orow is None else orow
    skip = torch.zeros_like(v, dtype=torch.bool)
    if d.oscale is not None or c.entry == "cat_relu_bits":
        res = d.add.double() if d.add is not None else torch.zeros_like(v)
        if d.res_scale is not None:
            res = rnd(f(f(res * d.res_scale.double()) + d.res_shift.double()))
        if d.oscale is not None:
            e = e * d.oscale.double().abs() + ulp(v * d.oscale.double())
            v = f(v * d.oscale.double())
        if d.res_scale is not None and lowp:
            e = e + R_BF16 * res.abs()                      # res' is rounded to bf16 before it is added: half a bf16 ulp of it
        v = f(f(v + bias) + res)
        e = e + 2 * ulp(v) + ulp(res)
        v = v.clamp_min(0)
    else:
        if bias is not None:
            v = f(v + bias)
            e = e + ulp(v)
        if d.add is not None:
            am, ok, bm = _add_rows(c, d, v.shape[0], dev, mutant)
            addv = d.add.double()[am] * ok[:, None]
            if d.add_bits is not None and mutant != "add_bits_ignored":
                bits = d.add_bits if mutant != "bits_stride_cout" else _restride_bits(d.add_bits, c.dtype, c.Cout + c.pads[2], c.Cout)
                addv = addv * bits[bm]
            v = f(v + addv)
            e = e + ulp(v)
        if d.bn is not None:
            if d.bn == "mask":
                cs = d.c.double()[full] * d.scale.double()
                t = cs + d.shift.double()
                keep = rnd(f(f(cs) + d.shift.double())) > 0
                skip = t.abs() < MASK_EDGE * (cs.abs() + d.shift.double().abs())
            else:
                bits = d.bn_bits
                if mutant == "bits_stride_cout" and d.add_bits is None:
                    bits = _restride_bits(bits, c.dtype, c.Cout + c.pads[1], c.Cout)
                keep = bits[full]
            v = torch.where(keep, v, torch.zeros_like(v))
        if d.relu:
            v = v.clamp(0, 6) if d.relu == 2 else v.clamp_min(0)
        if d.act == 1:
            pre = rnd(v)
            out["y2"], out["e2"] = pre, e
            v = f(_gelu(pre)[0])
            # |gelu'| <= 1.13 on the error of the stored pre-activation (a bf16 store: half a bf16 ulp more); erff and the
            # products: an allowance of 8 fp32 roundings
            e = 1.13 * (e + (R_BF16 * pre.abs() if lowp else 0)) + 8 * U * (pre.abs() + 1)
        elif d.act == 2:
            g = _gelu(d.aux.double())[1]
            v, e = f(v * g), e * g.abs() + 8 * U * (v.abs() + 1)
        elif d.act == 3:
            a = d.aux.double()
            v = torch.where((a > 0) & (a < 6), v, torch.zeros_like(v))
        elif d.act == 4:
            a = d.aux.double()
            v, e = f(v * a), e * a.abs() + ulp(v * a)
    stored = v if (d.out_f32 or not lowp) else rnd(v)
    if mutant == "cout_tail_dropped":
        stored = stored.clone()
        stored[:, c.Cout // 8 * 8:] = float("nan")
    y = torch.full((Z * Mfull, c.Cout), float("nan"), dtype=torch.float64, device=dev)
    if mutant == "class_row_unmapped" and d.bn is None:
        y[:M] = stored
    else:
        y[full] = stored
    out.update(y=y, e=e, skip=skip, rows=full)
    if d.stats:
        src = v if mutant == "stats_unrounded" else stored
        out["stats"] = stat_sums(c, d, torch.nan_to_num(src), full)[0]
    if d.out_bits:
        bits = torch.zeros(Mfull, c.Cout, dtype=torch.bool, device=dev)
        bits[full] = stored > 0
        if mutant == "bits_stride_cout":                         # written with Cout / 8 as the row stride: rows land elsewhere
            bits = _restride_bits(bits, c.dtype, c.Cout + c.pads[1], c.Cout)
        out["bits"] = bits
    out["past"] = mutant == "row_tail_written"
    return out


def stat_sums(c: Case, d: Data, y_rows: torch.Tensor, full: torch.Tensor):
    """float64 per-row-tile sums [tiles][2][Cout] of the launch rows' stored values y_rows [M][Cout] (plane 1: y^2, BN epilogues
    y * (c - mean)), and the sums of |terms| the bound scales with"""
    tp = c.inst.tp
    M = y_rows.shape[0]
    T = -(-M // tp)
    second = y_rows * ((d.c.double()[full] - d.mean.double()) if d.bn is not None else y_rows)
    planes = torch.stack([y_rows, second], 1)                    # [M][2][Cout]
    z = torch.zeros(T * tp, 2, c.Cout, dtype=torch.float64, device=y_rows.device)
    z[:M] = planes
    z = z.reshape(T, tp, 2, c.Cout)
    return z.sum(1), z.abs().sum(1)


# ---- the verdict -----------------------------------------------------------------------------------------------------------------
def verdict(c: Case, d: Data, ref: dict, yard: dict, got: dict) -> dict:
    """{check: (ratio, err, bound)}; a ratio <= 1 passes.  got: y [Z * Mfull][Cout] float64 (NaN where nothing was written), and as
    the launch has them y2, stats [tiles][2][Cout], bits [Mfull][Cout] bool, past (something was written outside the output)."""
    res = {}
    rows = ref["rows"]
    lowp_store = c.dtype == "bf16" and not d.out_f32
    r = R_BF16 if lowp_store else 0.0
    Z = c.batch[0] * c.batch[1]
    Mfull = ref["y"].shape[0] // Z
    sel = rows
    for name, en in (("y", "e"), ("y2", "e2")):
        if name not in ref:
            continue
        g, rf, e = got[name][sel], ref[name][sel], ref[en]
        keep = ~ref["skip"]
        bound = r * (rf.abs() + e) + e
        err = (g - rf).abs()
        q = torch.where(keep, err / bound.clamp_min(1e-300), torch.zeros_like(err))
        q = torch.where(torch.isnan(q) & keep, torch.full_like(q, math.inf), q)
        i = int(q.argmax())
        res[name + "_elem"] = (q.flatten()[i].item(), err.flatten()[i].item(), bound.flatten()[i].item())
        if lowp_store:
            tp, tc = c.inst.tp, c.inst.tc
            worst = (0.0, 0.0, FLOOR)
            for z in range(Z):
                zs = slice(z * g.shape[0] // Z, (z + 1) * g.shape[0] // Z)
                gz = torch.where(keep[zs], g[zs], rf[zs])
                yz = torch.where(keep[zs], yard[name][sel][zs], rf[zs])
                eg, ey = tile_errors(gz, rf[zs], tp, tc, RMS_FLOOR["y"]), tile_errors(yz, rf[zs], tp, tc, RMS_FLOOR["y"])
                big = tile_count(gz.shape[0], gz.shape[1], tp, tc, g.device) >= MIN_TILE
                bnd = torch.clamp(C_BOUND * ey, min=FLOOR)
                rt = torch.where(big, eg / bnd, torch.zeros_like(eg))
                rt = torch.where(torch.isnan(rt), torch.full_like(rt, math.inf), rt)
                j = int(rt.argmax())
                if rt.flatten()[j].item() >= worst[0]:
                    worst = (rt.flatten()[j].item(), eg.flatten()[j].item(), bnd.flatten()[j].item())
            res[name + "_tile"] = worst
    if c.cls is not None:                               # the other classes' rows stay as they were
        other = torch.ones(Mfull, dtype=torch.bool, device=rows.device)
        other[rows] = False
        touched = int((~torch.isnan(got["y"][other])).sum())
        res["y_untouched"] = (math.inf if touched else 0.0, float(touched), 0.0)
    share = ref["skip"].float().mean().item()
    res["mask_share"] = (share / MASK_SHARE, share, MASK_SHARE)
    if d.stats:
        own = torch.nan_to_num(got["y"][sel], nan=math.inf)
        want, mag = stat_sums(c, d, own, rows)
        bound = c.inst.tp * U * mag
        err = (got["stats"] - want).abs()
        q = torch.where(err <= bound, err / bound.clamp_min(1e-300), torch.full_like(err, math.inf))
        q = torch.where(err == 0, torch.zeros_like(q), q)
        i = int(torch.nan_to_num(q, nan=math.inf).argmax())
        res["stats"] = (torch.nan_to_num(q, nan=math.inf).flatten()[i].item(), err.flatten()[i].item(), bound.flatten()[i].item())
    if d.out_bits:
        want = torch.zeros_like(got["bits"])
        want[rows] = got["y"][rows] > 0
        bad = int((got["bits"] != want).sum())
        res["bits"] = (math.inf if bad else 0.0, float(bad), 0.0)
    res["guard"] = (math.inf if got.get("past") else 0.0, 0.0, 0.0)
    return res


def rejecting(c: Case, d: Data, mutant: str, ref=None, yard=None):
    """the checks that reject the yardstick with `mutant` applied, as {check: ratio}; None where the mutant does not exist"""
    mut = outputs(c, d, exact=False, mutant=mutant)
    if mut is None:
        return None
    ref = ref or outputs(c, d, exact=True)
    yard = yard or outputs(c, d, exact=False)
    return {k: v[0] for k, v in verdict(c, d, ref, yard, mut).items() if not v[0] <= 1.0}


# ---- operands --------------------------------------------------------------------------------------------------------------------
def make(c: Case, device, seed: int = 0) -> Data:
    """The operands of a case: activations N(0, 1), filters N(0, 1 / K) (outputs of unit variance), every epilogue operand O(1)."""
    g = torch.Generator(device=device).manual_seed(seed)
    dt = TORCH_DT[c.dtype]
    P, Q, M, Mfull, _, _, Ktot = dims(c)
    rn = lambda *s: torch.randn(*s, generator=g, device=device)
    ru = lambda *s: torch.rand(*s, generator=g, device=device)
    C = c.Cout
    Z = c.batch[0] * c.batch[1]
    if c.entry == "batched":
        d = Data(x=rn(Z, M, c.Cin).to(dt), w=(rn(Z, C, c.Cin) / math.sqrt(c.Cin)).to(dt))
    else:
        d = Data(x=rn(c.N * c.H * c.W, c.Cin).to(dt), w=(rn(C, Ktot) / math.sqrt(Ktot)).to(dt))
    if c.K2:
        d.x2 = rn(M, c.K2).to(dt)
    e = c.epi
    d.act = c.act
    if c.act in (2, 3, 4):
        d.aux = ((rn(M, C) * 3).clamp(0, 6) if c.act == 3 else rn(M, C)).to(dt)
    if "bias" in e or c.entry in ("cat_bias", "cat_relu_bits", "affine", "dgrad_bn_cat", "dgrad_bn_add") or c.act == 1:
        d.bias = rn(C) * 0.5
    d.relu = 2 if "relu6" in e else 1 if "relu" in e else 0
    d.out_f32 = "f32out" in e
    d.stats = "stats" in e
    add_dt = torch.float32 if d.out_f32 else dt
    if "subadd" in e:
        d.add_kind = "sub"
        Ho, Wo = (c.out if c.cls is not None else (P, Q))
        d.add_hw = ((Ho + 1) // 2, (Wo + 1) // 2)
        d.add = rn(c.N * d.add_hw[0] * d.add_hw[1], C).to(add_dt)
    elif "add" in e or c.entry in ("affine", "dgrad_bn_add"):
        d.add = rn(Mfull, C).to(add_dt)
    if "addbits" in e:
        d.add_bits = ru(Mfull, C) < 0.6
    if c.entry == "affine":
        d.oscale = ru(C) + 0.5
        d.out_bits = True
        if "resaff" in e:
            d.res_scale, d.res_shift = ru(C) + 0.5, rn(C) * 0.3
    if c.entry == "cat_relu_bits":
        d.out_bits = True
    if "bnmask" in e or "bnbits" in e:
        d.bn = "mask" if "bnmask" in e else "bits"
        d.c = rn(Mfull, C).to(dt)
        d.mean = rn(C) * 0.1
        if d.bn == "mask":
            d.scale, d.shift = ru(C) + 0.5, rn(C) * 0.3
        else:
            d.bn_bits = ru(Mfull, C) < 0.6
        d.stats = "nostats" not in e
    return d


# ---- the case table --------------------------------------------------------------------------------------------------------------
B, F = "bf16", "f32"
I = Inst


def _conv(name, inst, N, H, W, Cin, Cout, k=(1, 1, 1, 0), mode=0, out=None, epi="plain", entry="conv_gemm", **kw):
    R, S, stride, pad = k
    return Case(name, entry, inst, N, H, W, Cin, Cout, R, S, stride, pad, mode, out, epi=epi, **kw)


def _gemm(name, entry, inst, M, K, Cout, **kw):
    return Case(name, entry, inst, 1, M, 1, K, Cout, **kw)


K3, K3S2, K1S2, K31 = (3, 3, 1, 1), (3, 3, 2, 1), (1, 1, 2, 0), (3, 1, 1, 1)
BITS = (8, 16, 16)               # a tensor with a bit array beside it: leading dimension C + 16

_CLS = []
for _i, (_ph, _pw) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
    _rc, _sc = (2 if _ph else 1), (2 if _pw else 1)
    for _j, _var in enumerate(("plain", "add", "subadd", "bnmask")):
        _dt = (B, F)[(_i + _j) % 2]
        _out = ((12, 13), (13, 12))[(_i + _j // 2) % 2]
        _hd = ((_out[0] - 1) // 2 + 1, (_out[1] - 1) // 2 + 1)
        _wide = (_i + _j) % 3 != 0
        _C = (136 if _wide else 40) if _var != "plain" else (140 if _wide else 44)      # plain: a channel tail (C % 8 = 4)
        _inst = I(_dt, 128 if _wide else 64, "BN_MASK" if _var == "bnmask" else "GENERAL")
        _CLS.append(Case(f"class{_ph}{_pw}_{_var}_{_dt}", "s2class", _inst, 2, _hd[0], _hd[1], KTE[_dt] * (1 + _j % 2), _C, _rc, _sc,
                         1, 0, 1, _out, (_ph, _pw), epi=_var))

CASES = (
    # ---- nkb_conv_gemm, bf16 ----
    _conv("f3x3_lean_halo", I(B, 128, "LEAN", True), 2, 11, 13, 64, 136, K3, epi="bias_relu"),
    _conv("f3x3_lean_halo_stats", I(B, 128, "LEAN", True), 3, 5, 13, 128, 192, K3, epi="stats"),
    _conv("f3x3_narrow_lean_halo", I(B, 64, "LEAN", True), 2, 11, 13, 64, 40, K3, epi="bias_stats"),
    _conv("f3x3_narrow_tail_halo", I(B, 64, "GENERAL", True), 2, 7, 9, 64, 44, K3, epi="bias_stats"),
    _conv("f3x3_tail_add_halo", I(B, 128, "GENERAL", True), 2, 7, 9, 128, 140, K3, epi="add_relu"),
    _conv("d3x3_narrow_lean_halo", I(B, 64, "LEAN", True), 3, 11, 13, 128, 64, K3, mode=1),
    _conv("d3x3_f32out_halo", I(B, 128, "GENERAL", True), 2, 7, 9, 64, 192, K3, mode=1, epi="add_f32out"),
    _conv("f3x3_1x1map_halo", I(B, 128, "LEAN", True), 5, 1, 1, 128, 136, K3, epi="bias"),
    _conv("f3x3_w2_halo", I(B, 64, "LEAN", True), 3, 5, 2, 64, 64, K3, epi="bias_relu6"),
    _conv("d3x3_w2_halo", I(B, 128, "LEAN", True), 3, 5, 2, 64, 136, K3, mode=1),
    _conv("f1x1_add_relu", I(B, 128, "LEAN"), 2, 11, 13, 128, 192, epi="add_relu"),
    _conv("f1x1_narrow_relu6", I(B, 64, "LEAN"), 3, 11, 13, 64, 64, epi="bias_relu6"),
    _conv("f1x1_addbits", I(B, 128, "GENERAL"), 3, 5, 13, 64, 136, epi="add_addbits", pads=BITS),
    _conv("f1x1_narrow_f32out", I(B, 64, "GENERAL"), 2, 11, 13, 64, 40, epi="bias_f32out"),
    _conv("f1x1s2_stats", I(B, 128, "LEAN"), 3, 11, 13, 64, 136, K1S2, epi="stats"),
    _conv("f3x3s2_narrow", I(B, 64, "LEAN"), 3, 11, 13, 64, 40, K3S2, epi="bias_relu_stats"),
    _conv("f1x1_narrow_tail", I(B, 64, "GENERAL"), 3, 11, 13, 128, 44, epi="bias_relu"),
    _conv("f3x3s2_tail", I(B, 128, "GENERAL"), 3, 11, 13, 128, 140, K3S2, epi="bias_relu_stats"),
    _conv("d3x3s2_subadd", I(B, 128, "GENERAL"), 2, 6, 7, 64, 136, K3S2, mode=1, out=(11, 13), epi="subadd"),
    _conv("d3x3s2_narrow", I(B, 64, "LEAN"), 3, 6, 7, 128, 64, K3S2, mode=1, out=(11, 13)),
    _conv("f3x1_narrow", I(B, 64, "LEAN"), 2, 7, 9, 64, 64, K31, epi="bias"),
    _conv("grouped_walk", I(B, 128, "LEAN"), 8, 9, 29, 1024, 1544, epi="bias_relu", grouped=True),
    # ---- nkb_conv_gemm, fp32 ----
    _conv("f3x3_f32_stats", I(F, 128, "GENERAL"), 2, 11, 13, 32, 136, K3, epi="bias_stats"),
    _conv("d3x3_f32_narrow", I(F, 64, "GENERAL"), 3, 11, 13, 64, 40, K3, mode=1, epi="add_relu"),
    _conv("f3x3_f32_1x1map", I(F, 128, "GENERAL"), 5, 1, 1, 32, 136, K3, epi="bias"),
    _conv("f1x1_f32_addbits", I(F, 128, "GENERAL"), 3, 5, 13, 64, 136, epi="add_addbits", pads=BITS),
    _conv("f1x1_f32_narrow_tail", I(F, 64, "GENERAL"), 2, 11, 13, 32, 44, epi="bias_relu6"),
    _conv("f1x1s2_f32", I(F, 128, "GENERAL"), 3, 11, 13, 32, 192, K1S2, epi="stats"),
    _conv("f3x3s2_f32_narrow", I(F, 64, "GENERAL"), 3, 11, 13, 32, 64, K3S2, epi="bias_relu_stats"),
    _conv("d3x3s2_f32_subadd", I(F, 128, "GENERAL"), 2, 6, 7, 64, 136, K3S2, mode=1, out=(11, 13), epi="subadd"),
    _conv("f3x1_f32", I(F, 128, "GENERAL"), 2, 7, 9, 32, 140, K31, epi="bias"),
    # ---- nkb_conv_dgrad_bn: recomputed mask (with statistics: lean; without: the general loop), bits with every residual form ----
    _conv("dbn_mask_halo", I(B, 128, "BN_MASK_LEAN", True), 2, 11, 13, 64, 136, K3, 1, entry="dgrad_bn", epi="bnmask"),
    _conv("dbn_mask_narrow_halo", I(B, 64, "BN_MASK_LEAN", True), 3, 11, 13, 128, 40, K3, 1, entry="dgrad_bn", epi="bnmask"),
    _conv("dbn_mask_1x1", I(B, 128, "BN_MASK_LEAN"), 3, 5, 13, 128, 192, mode=1, entry="dgrad_bn", epi="bnmask"),
    _conv("dbn_mask_narrow_s2", I(B, 64, "BN_MASK_LEAN"), 2, 6, 7, 64, 64, K3S2, 1, (11, 13), entry="dgrad_bn", epi="bnmask"),
    _conv("dbn_mask_nostats_halo", I(B, 128, "BN_MASK", True), 2, 7, 9, 64, 136, K3, 1, entry="dgrad_bn", epi="bnmask_nostats"),
    _conv("dbn_mask_nostats_narrow_halo", I(B, 64, "BN_MASK", True), 2, 11, 13, 64, 40, K3, 1, entry="dgrad_bn", epi="bnmask_nostats"),
    _conv("dbn_mask_nostats_s2", I(B, 128, "BN_MASK"), 2, 6, 7, 64, 136, K3S2, 1, (11, 13), entry="dgrad_bn", epi="bnmask_nostats"),
    _conv("dbn_mask_nostats_narrow_1x1", I(B, 64, "BN_MASK"), 3, 11, 13, 64, 64, mode=1, entry="dgrad_bn", epi="bnmask_nostats"),
    _conv("dbn_bits_halo", I(B, 128, "BN_BITS_LEAN", True), 2, 11, 13, 64, 136, K3, 1, entry="dgrad_bn", epi="bnbits_add_addbits",
          pads=BITS),
    _conv("dbn_plain_narrow_halo", I(B, 64, "BN_BITS_LEAN", True), 3, 11, 13, 64, 40, K3, 1, entry="dgrad_bn", epi="bnbits_add",
          pads=BITS),
    _conv("dbn_sub_s2", I(B, 128, "BN_BITS_LEAN"), 2, 6, 7, 128, 192, K3S2, 1, (11, 13), entry="dgrad_bn", epi="bnbits_subadd",
          pads=BITS),
    _conv("dbn_bits_narrow_1x1", I(B, 64, "BN_BITS_LEAN"), 3, 11, 13, 64, 64, mode=1, entry="dgrad_bn", epi="bnbits_add_addbits",
          pads=BITS),
    _conv("dbn_none_halo", I(B, 128, "BN_BITS", True), 2, 7, 9, 64, 136, K3, 1, entry="dgrad_bn", epi="bnbits", pads=BITS),
    _conv("dbn_none_narrow_halo", I(B, 64, "BN_BITS", True), 2, 11, 13, 64, 40, K3, 1, entry="dgrad_bn", epi="bnbits", pads=BITS),
    _conv("dbn_none_1x1", I(B, 128, "BN_BITS"), 3, 5, 13, 64, 136, mode=1, entry="dgrad_bn", epi="bnbits", pads=BITS),
    _conv("dbn_none_narrow_s2", I(B, 64, "BN_BITS"), 2, 6, 7, 64, 40, K3S2, 1, (11, 13), entry="dgrad_bn", epi="bnbits", pads=BITS),
    _conv("dbn_f32_mask", I(F, 128, "BN_MASK"), 2, 11, 13, 32, 136, K3, 1, entry="dgrad_bn", epi="bnmask"),
    _conv("dbn_f32_mask_narrow", I(F, 64, "BN_MASK"), 3, 11, 13, 64, 40, mode=1, entry="dgrad_bn", epi="bnmask"),
    _conv("dbn_f32_bits", I(F, 128, "BN_BITS"), 2, 11, 13, 32, 136, K3, 1, entry="dgrad_bn", epi="bnbits_add_addbits", pads=BITS),
    _conv("dbn_f32_sub_narrow", I(F, 64, "BN_BITS"), 2, 6, 7, 32, 64, K3S2, 1, (11, 13), entry="dgrad_bn", epi="bnbits_subadd",
          pads=BITS),
    _conv("dbn_f32_plain", I(F, 128, "BN_BITS"), 3, 5, 13, 32, 192, mode=1, entry="dgrad_bn", epi="bnbits_add", pads=BITS),
    _conv("dbn_f32_none_narrow", I(F, 64, "BN_BITS"), 2, 7, 9, 32, 40, K3, 1, entry="dgrad_bn", epi="bnbits", pads=BITS),
    # ---- the four parity classes of the stride-2 3x3 data gradient: plain, residual, sub-grid residual, fused BN ----
    *_CLS,
    # ---- the Gram-form closing stages ----
    _conv("affine_1x1", I(B, 128, "AFFINE_BITS"), 2, 11, 13, 64, 136, entry="affine", epi="affine", pads=BITS),
    _conv("affine_1x1_resaff", I(B, 128, "AFFINE_BITS"), 3, 5, 13, 128, 192, entry="affine", epi="affine_resaff", pads=BITS),
    _conv("affine_1x1s2_resaff", I(B, 128, "AFFINE_BITS"), 3, 11, 13, 64, 136, K1S2, entry="affine", epi="affine_resaff", pads=BITS),
    _conv("affine_3x3_halo", I(B, 128, "AFFINE_BITS", True), 2, 11, 13, 64, 192, K3, entry="affine", epi="affine", pads=BITS),
    _gemm("cat_relu_bits_136", "cat_relu_bits", I(B, 128, "AFFINE_BITS"), 286, 64, 136, K2=128, epi="relu", pads=BITS),
    _gemm("cat_bias_40", "cat_bias", I(B, 64, "LEAN_CAT"), 286, 128, 40, K2=64),
    _gemm("cat_bias_136", "cat_bias", I(B, 128, "LEAN_CAT"), 286, 64, 136, K2=128),
    _gemm("dbn_cat", "dgrad_bn_cat", I(B, 128, "BN_MASK_LEAN"), 286, 128, 136, K2=64, epi="bnmask"),
    _gemm("dbn_cat_f32", "dgrad_bn_cat", I(F, 64, "BN_MASK"), 286, 32, 40, K2=64, epi="bnmask"),
    _gemm("dbn_add", "dgrad_bn_add", I(B, 128, "BN_MASK"), 286, 128, 136, epi="bnmask"),
    _gemm("dbn_add_f32", "dgrad_bn_add", I(F, 128, "BN_MASK"), 195, 64, 192, epi="bnmask"),
    # ---- nkb_gemm_batched: outer = 2, inner = 3, distinct strides ----
    _gemm("batched", "batched", I(B, 128, "LEAN"), 70, 64, 72, batch=(2, 3)),
    _gemm("batched_f32out", "batched", I(B, 64, "GENERAL"), 70, 128, 40, batch=(2, 3), epi="f32out"),
    _gemm("batched_f32", "batched", I(F, 128, "GENERAL"), 70, 32, 72, batch=(2, 3)),
    _gemm("batched_tail", "batched", I(B, 128, "GENERAL"), 70, 64, 76, batch=(2, 3)),
    # ---- nkb_linear_gelu at a width the eight-phase core refuses (N = 192) ----
    *(_gemm(f"linear_act{a}", "linear_gelu", I(B, 128, "GENERAL"), 200, 128, 192, act=a, pads=(0, 0, 0)) for a in (1, 2, 3, 4)),
    _gemm("linear_act1_f32", "linear_gelu", I(F, 128, "GENERAL"), 200, 64, 192, act=1, pads=(0, 0, 0)),
    _gemm("linear_act2_f32", "linear_gelu", I(F, 128, "GENERAL"), 200, 32, 192, act=2, pads=(0, 0, 0)),
)

CONV_ENTRIES = ("conv_gemm", "dgrad_bn", "s2class", "affine")       # the entries whose rows are a gather over an image

__all__ = ["Case", "Data", "Inst", "CASES", "INSTANCES", "MUTANTS", "REJECTED_BY", "GROUPED_BIT", "make", "dims", "outputs", "verdict",
           "rejecting", "pack_bits", "unpack_bits", "class_filter", "class_taps", "out_rows", "gather_index", "stat_sums", "KTE",
           "TORCH_DT", "CONV_ENTRIES", "mutant_exists"]
