"""Float64 reference of the gemm8p GEMM core (csrc/gemm8p.hip: the persistent 256 x 256 kernels, their fp8 forms and the ragged-row
companion), the rounding yardstick, the error metric and bound that tests/test_gemm8p_gpu.py holds the HIP kernels to, and mutants
that make the yardstick subtly wrong in the ways a GEMM kernel goes wrong.  tests/test_gemm_reference.py proves on the CPU that the
bound rejects every mutant.  No test lives here.

The operation: y = epi(deq * x w^T), x [M][K], w [N][K].  bf16 operands enter as their values; fp8 operands enter as their exactly
decoded values and deq = deq_x * deq_w (the two per-tensor dequantisation factors, fp32).  The epilogue, in the kernels' order:
    v = deq * p + bias;  v = row_scale[m // rows_per_sample] * v (with add);  v += add;
    v *= aux (aux_mode 0) | v where 0 < aux < 6 (aux_mode 1) | v where the mask bit is set (mask_in);
    GELU (relu 3: y = gelu(v), y2 = gelu'(v)) | ReLU (relu 1) | ReLU6 (relu 2);  y = bf16(v)
and the second outputs: BatchNorm statistics (sums of y and y^2 per 128 rows, of the STORED bf16 y), the fp8 copy
yq = fp8(y * qscale) with its amax max |y|, the ReLU6 mask bits 0 < y < 6 (of the stored y), and colsum += column sums of y.

The yardstick.  A bf16 kernel cannot be closer to the float64 truth than the same math done the way the kernel does it: the float64
product rounded to fp32 (the accumulator), the epilogue in fp32, bf16 rounding exactly where the kernel rounds (the stored y and
y2; the GELU derivative from the fp32 pre-activation).  A correct kernel is not much further.  The one thing the yardstick leaves
out is the ORDER of the kernel's fp32 accumulation: its error is about sqrt(K) * 2^-24 of the product's scale, 2e-6 at K = 4096,
three orders of magnitude below the bf16 rounding (2^-9) that dominates the yardstick's own error, so it cannot move a ratio.
Likewise the epilogue's erf approximation (|error| <= 1.5e-7) and FMA contraction.

The metric: relative Frobenius error per output tile, 256 x 256 on the persistent kernels and R x 64 column blocks on the rows the
ragged companion computes (so one wrong tile among 2 048 is not averaged away); a tile whose reference is (near) zero is measured
against RMS_FLOOR instead of its own norm.  The bound: max(C_BOUND * yardstick error, FLOOR), per tile.  C_BOUND is below sqrt(2):
a product rounded to bf16 before the epilogue adds a second rounding error of the same size, in quadrature.  FLOOR covers tiles the
yardstick computes exactly (an all-zero ReLU tile, exact small-integer data) and is five times below the bf16 rounding level.
"""
import math
from dataclasses import dataclass, replace
from typing import Optional

import torch

C_BOUND = 1.15
FLOOR = 2e-4
RMS_FLOOR = dict(y=1e-2, y2=1e-2, yq=1e-2, stats_sum=1e-1, stats_sq=1e-1, colsum=1e-1)
TILE = 256                    # the persistent kernels' output tile
RAGGED_COLS = 64              # the companion's column block
KSLICE = {False: 32, True: 64}    # K depth of one MFMA slice: bf16 / fp8
KTILE = {False: 64, True: 128}    # K depth of one k-tile (128 bytes of a row): bf16 / fp8
FP8 = {0: (torch.float8_e4m3fn, 448.0), 1: (torch.float8_e5m2, 57344.0)}   # q_kind -> (format, largest finite value)
U0_EDGE = 1e-4                # |pre| below which the kernels' fp32 sums of O(1) terms may land on either side of 0 (seen: 1.6e-5)
U6_EDGE = 6 * 2 ** -8         # a reference within this of 6 may store as 6.0 (bf16 spacing below 8 is 2^-5; half of it, with margin)

MUTANTS = ("drop_kslice", "stale_kslice", "acc_not_cleared", "bias_shift", "operand_next_row", "row_scale_off",
           "double_round", "mask_inclusive", "ragged_split_missing", "deq_missing")


@dataclass
class Epi:
    """One launch's epilogue.  Tensors live on the device of the product; bf16 operands as bf16-valued tensors of any float dtype."""
    bias: Optional[torch.Tensor] = None          # [N] fp32
    add: Optional[torch.Tensor] = None           # [M][N]
    row_scale: Optional[torch.Tensor] = None     # [samples] fp32, with add
    rows_per_sample: int = 1
    aux: Optional[torch.Tensor] = None           # [M][N]
    aux_mode: int = 0                            # 0 multiply, 1 keep where 0 < aux < 6
    mask_in: Optional[torch.Tensor] = None       # [M][N] bool
    relu: int = 0                                # 0 none, 1 ReLU, 2 ReLU6, 3 GELU (+ y2 = GELU')
    deq: Optional[tuple] = None                  # fp8: (deq_x, deq_w) as python floats holding fp32 values
    stats: bool = False
    colsum: Optional[torch.Tensor] = None        # [N] fp32: the initial value colsum is added to
    yq: Optional[tuple] = None                   # (qscale, q_kind)
    mask_out: bool = False


@dataclass
class Geo:
    """Where the tile mutants strike and which rows the companion computed.  ragged = (M0, S): rows [M0, M) are the companion's,
    its K split S ways; None: the persistent kernel owns every row."""
    fp8: bool = False
    ragged: Optional[tuple] = None


def bf(x: torch.Tensor) -> torch.Tensor:
    """x rounded to bf16 (round to nearest even), kept in x's dtype."""
    return x.to(torch.bfloat16).to(x.dtype)


def f32(x: float) -> float:
    return float(torch.tensor(x, dtype=torch.float32))


def quantize(y: torch.Tensor, qscale: float, kind: int) -> torch.Tensor:
    """fp8 copy of a bf16-valued tensor: fp8(clamp(y * qscale)) in fp32 arithmetic, round to nearest even (nkb_fp8_quantize)."""
    dt, lim = FP8[kind]
    return (y.float() * qscale).clamp(-lim, lim).to(dt)


def unpack_bits(bits: torch.Tensor) -> torch.Tensor:
    """[M][N / 8] bytes -> [M][N] bool, bit e of byte (m, c) = element (m, 8 c + e)"""
    sh = torch.arange(8, device=bits.device, dtype=torch.int32)
    return ((bits.to(torch.int32)[:, :, None] >> sh) & 1).bool().reshape(bits.shape[0], -1)


def product(x: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    """x w^T in float64 (exact for the operands of these tests: bf16 / fp8 values, K <= 4096, no cancellation below 2^-53)"""
    return x.double() @ w.double().t()


def _gelu(v):
    c = 0.5 * (1 + torch.erf(v * (1 / math.sqrt(2))))
    return v * c, c + v * torch.exp(-0.5 * v * v) * (1 / math.sqrt(2 * math.pi))


def _row_operand(t, mutant):
    if t is None or mutant != "operand_next_row":
        return t
    return torch.cat([t[1:], t[-1:]], 0)                   # row m reads row m + 1 (the last row itself)


def _tile_product(x, w, r0, r1, c0, c1, k0, k1):
    return x[r0:r1, k0:k1].double() @ w[c0:c1, k0:k1].double().t()


def mutant_tile(M, N):
    """(rows, cols) of the tile the tile mutants strike: the second row block (the first if there is one), last column block"""
    tm = 1 if M > TILE else 0
    tn = N // TILE - 1 if N >= TILE else 0
    return (tm * TILE, min(M, tm * TILE + TILE)), (tn * TILE, min(N, tn * TILE + TILE))


def _mutate_product(p, x, w, geo: Geo, mutant):
    """the float64 product as a kernel with `mutant` would accumulate it; None: the mistake does not exist at this geometry"""
    M, N = p.shape
    K = x.shape[1]
    (r0, r1), (c0, c1) = mutant_tile(M, N)
    ks, kt = KSLICE[geo.fp8], KTILE[geo.fp8]
    k0 = (K // 2) // kt * kt                                 # a slice in the middle of the k-loop, at a k-tile boundary
    if mutant == "drop_kslice":
        p = p.clone()
        p[r0:r1, c0:c1] -= _tile_product(x, w, r0, r1, c0, c1, k0, k0 + ks)
        return p
    if mutant == "stale_kslice":                              # this k-tile's slice read from the buffer of the previous k-tile
        if k0 < kt:
            return None
        p = p.clone()
        p[r0:r1, c0:c1] += _tile_product(x, w, r0, r1, c0, c1, k0 - kt, k0 - kt + ks) - _tile_product(x, w, r0, r1, c0, c1, k0, k0 + ks)
        return p
    if mutant == "acc_not_cleared":                           # the tile before it in the walk left its sum in the accumulators
        if r0 < TILE:
            return None
        p = p.clone()
        p[r0:r1, c0:c1] += p[r0 - TILE:r1 - TILE, c0:c1]
        return p
    if mutant == "ragged_split_missing":                      # one of the companion's S K-splits never arrives in a column block
        if geo.ragged is None:
            return None
        M0, S = geo.ragged
        if S < 2:
            return None
        kk = K // S
        p = p.clone()
        p[M0:, :RAGGED_COLS] -= _tile_product(x, w, M0, M, 0, RAGGED_COLS, (S - 1) * kk, K)
        return p
    return p


def outputs(p: torch.Tensor, e: Epi, *, exact: bool, mutant: Optional[str] = None, x=None, w=None, geo: Geo = Geo()):
    """The launch's outputs from the float64 product p [M][N].  exact: float64 throughout, nothing rounded (the reference).
    Otherwise the yardstick (see the module docstring), with `mutant` applied; None where the mutant does not exist here.
    Returns dict: y [M][N] (+ y2, stats_sum / stats_sq [ceil(M / 128)][N], yq (decoded / qscale), amax, bits, colsum)."""
    if mutant is not None:
        if mutant in ("bias_shift",) and e.bias is None:
            return None
        if mutant == "operand_next_row" and e.add is None and e.aux is None and e.mask_in is None:
            return None
        if mutant == "row_scale_off" and (e.row_scale is None or e.rows_per_sample >= p.shape[0]):
            return None
        if mutant == "mask_inclusive" and not ((e.aux is not None and e.aux_mode == 1) or e.mask_out):
            return None
        if mutant == "deq_missing" and e.deq is None:
            return None
        p = _mutate_product(p, x, w, geo, mutant)
        if p is None:
            return None
    M, N = p.shape
    dt = torch.float64 if exact else torch.float32
    r = (lambda t: t) if exact else bf
    v = p.to(dt)
    if e.deq is not None:
        dx, dw = e.deq
        if exact:
            v = v * dx * dw
        else:
            v = v * (f32(dx * dw) if mutant != "deq_missing" else dx)
    if mutant == "double_round":
        v = bf(v)
    if e.bias is not None:
        b = e.bias.to(dt)
        if mutant == "bias_shift":
            b = torch.roll(b, -1)                             # column n reads bias[n + 1]
        v = v + b
    add = _row_operand(e.add, mutant)
    if add is not None:
        if e.row_scale is not None:
            m = torch.arange(M, device=p.device)
            idx = m // e.rows_per_sample
            if mutant == "row_scale_off":                     # the first row of every sample takes the previous sample's scale
                idx = torch.clamp((m - 1) // e.rows_per_sample, min=0)
            v = v * e.row_scale.to(dt)[idx][:, None]
        v = v + add.to(dt)
    lo_ok = (lambda a: a >= 0) if mutant == "mask_inclusive" else (lambda a: a > 0)
    hi_ok = (lambda a: a <= 6) if mutant == "mask_inclusive" else (lambda a: a < 6)
    aux = _row_operand(e.aux, mutant)
    if aux is not None:
        a = aux.to(dt)
        v = v * a if e.aux_mode == 0 else torch.where(lo_ok(a) & hi_ok(a), v, torch.zeros_like(v))
    mask_in = _row_operand(e.mask_in, mutant)
    if mask_in is not None:
        v = torch.where(mask_in, v, torch.zeros_like(v))
    out = {"pre": v} if e.mask_out else {}
    if e.relu == 3:
        v, d = _gelu(v)
        out["y2"] = r(d)
    elif e.relu == 1:
        v = v.clamp_min(0)
    elif e.relu == 2:
        v = v.clamp(0, 6)
    y = r(v)
    out["y"] = y
    y64 = y.double()
    if e.stats:
        P = (M + 127) // 128
        pad = torch.zeros(P * 128 - M, N, dtype=torch.float64, device=p.device)
        yy = torch.cat([y64, pad]).reshape(P, 128, N)
        out["stats_sum"], out["stats_sq"] = yy.sum(1), (yy * yy).sum(1)
    if e.yq is not None:
        qscale, kind = e.yq
        if exact:
            out["yq"] = y64
        else:
            out["yq"] = quantize(y, qscale, kind).double() / qscale
        out["amax"] = y64.abs().max().item()
    if e.mask_out:
        out["bits"] = lo_ok(y64) & hi_ok(y64)
    if e.colsum is not None:
        out["colsum"] = e.colsum.double() + y64.sum(0)
    return out


def tile_sumsq(t: torch.Tensor, rows: int, cols: int) -> torch.Tensor:
    """sum of squares per (rows x cols) tile of a 2-D float64 tensor (the last tiles may be partial)"""
    M, N = t.shape
    tm, tn = -(-M // rows), -(-N // cols)
    z = torch.zeros(tm * rows, tn * cols, dtype=torch.float64, device=t.device)
    z[:M, :N] = t
    return (z * z).reshape(tm, rows, tn, cols).sum((1, 3))


def tile_count(M, N, rows, cols, device):
    ones = torch.ones(M, N, dtype=torch.float64, device=device)
    return tile_sumsq(ones, rows, cols)


def regions(M: int, geo: Geo, out: str):
    """(first row, last row + 1, tile rows, tile cols) of the tiles the metric uses for output `out`"""
    if out in ("stats_sum", "stats_sq"):                      # one partial row per 128 output rows: a 256-row tile = 2 rows
        return [(0, (M + 127) // 128, 2, TILE)]
    if out == "colsum":
        return [(0, 1, 1, TILE)]
    if geo.ragged is None:
        return [(0, M, TILE, TILE)]
    M0 = geo.ragged[0]
    return [(0, M0, TILE, TILE), (M0, M, M - M0, RAGGED_COLS)]


def tile_errors(got: torch.Tensor, ref: torch.Tensor, rows: int, cols: int, rms_floor: float) -> torch.Tensor:
    """relative Frobenius error per tile: ||got - ref|| / max(||ref||, rms_floor * sqrt(elements of the tile))"""
    got, ref = got.double(), ref.double()
    if got.dim() == 1:
        got, ref = got[None], ref[None]
    e2 = tile_sumsq(got - ref, rows, cols)
    r2 = tile_sumsq(ref, rows, cols)
    n = tile_count(*ref.shape, rows, cols, ref.device)
    return e2.sqrt() / torch.maximum(r2.sqrt(), rms_floor * n.sqrt())


def ratio(got: torch.Tensor, ref: torch.Tensor, yard: torch.Tensor, out: str, geo: Geo):
    """the worst tile of err(got) / max(C_BOUND * err(yardstick), FLOOR) (<= 1 passes), as (ratio, err, bound)"""
    worst = (0.0, 0.0, FLOOR)
    M = got.shape[0] if got.dim() > 1 else 1
    for (a, b, tr, tc) in regions(M, geo, out):
        g, rf, yd = (t[a:b] if t.dim() > 1 else t for t in (got, ref, yard))
        eg = tile_errors(g, rf, tr, tc, RMS_FLOOR[out])
        ey = tile_errors(yd, rf, tr, tc, RMS_FLOOR[out])
        bound = torch.clamp(C_BOUND * ey, min=FLOOR)
        rt = eg / bound
        i = int(rt.flatten().argmax())
        if rt.flatten()[i].item() >= worst[0] or math.isnan(rt.flatten()[i].item()):
            worst = (rt.flatten()[i].item(), eg.flatten()[i].item(), bound.flatten()[i].item())
    return worst


def bits_agree(bits: torch.Tensor, pre_ref: torch.Tensor) -> bool:
    """the ReLU6 mask bits against the reference pre-activation (outputs()["pre"]): equal to 0 < pre < 6 wherever pre is not within
    the kernel's fp32 evaluation of deq * p + b of 0 (U0_EDGE) or within bf16 rounding below 6 (U6_EDGE, stored as 6.0)"""
    v = pre_ref.double()
    want = (v > 0) & (v < 6)
    near = (v.abs() <= U0_EDGE) | ((v > 6 - U6_EDGE) & (v < 6))
    return bool(((bits == want) | near).all())


def amax_agrees(amax: float, y_ref: torch.Tensor) -> bool:
    """max |y| of the stored bf16 y against the reference's: within one bf16 rounding"""
    ref = y_ref.double().abs().max().item()
    return abs(amax - ref) <= ref * 2 ** -8 + 1e-30


def outputs_of(e: Epi):
    """names of the tensor outputs the metric measures for a launch with epilogue e"""
    names = ["y"]
    if e.relu == 3:
        names.append("y2")
    if e.stats:
        names += ["stats_sum", "stats_sq"]
    if e.yq is not None:
        names.append("yq")
    if e.colsum is not None:
        names.append("colsum")
    return names


def worst_mutant_ratio(p, e: Epi, x, w, geo: Geo, mutant: str):
    """largest ratio over the outputs of the yardstick with `mutant` applied; None where the mutant does not exist here.  A mask
    output counts as failing (inf) when its bits disagree with the reference beyond rounding."""
    ref = outputs(p, e, exact=True)
    yard = outputs(p, e, exact=False)
    mut = outputs(p, e, exact=False, mutant=mutant, x=x, w=w, geo=geo)
    if mut is None:
        return None
    worst = 0.0
    for o in outputs_of(e):
        worst = max(worst, ratio(mut[o], ref[o], yard[o], o, geo)[0])
    if e.mask_out and not bits_agree(mut["bits"], ref["pre"]):
        worst = math.inf
    return worst


# ---- the case table of tests/test_gemm8p_gpu.py (the CPU proof runs the same cases at a reduced M) ---------------------------
@dataclass(frozen=True)
class Case:
    name: str
    instance: str             # the kernel instance the case is there for
    regime: str               # the walk it takes there
    M: int
    N: int
    K: int
    epi: str                  # see make()
    mode: Optional[int] = None    # fp8: 0 = e4m3 x e4m3, 1 = e5m2 activations-side x e4m3 weights; None: bf16
    pad: tuple = (0, 0, 0, 0)     # ldx - K, ldw - K, ldy - N, ldadd - N
    companion: bool = False       # the M % 256 ragged rows go to gemm8p_ragged_kernel
    everywhere: bool = False      # gemm8p_config(True, 1, 128): problems below the default envelope take the kernel
    cus256: bool = False          # the walk regime named is the one 256 CUs give

    @property
    def fp8(self):
        return self.mode is not None


G_TRUE0, G_FALSE0 = "gemm8p_kernel<true,0>", "gemm8p_kernel<false,0>"
G_F8 = {(0, False): "gemm8p_kernel<true,1>", (1, False): "gemm8p_kernel<true,2>",
        (0, True): "gemm8p_kernel<true,1,true>", (1, True): "gemm8p_kernel<true,2,true>"}
G_R1, G_R2 = "gemm8p_ragged_kernel<1>", "gemm8p_ragged_kernel<2>"
INSTANCES = (G_TRUE0, G_FALSE0, *G_F8.values(), G_R1, G_R2)
QOUT_EPIS = ("f8_relu6_bits", "f8_mask_colsum", "f8_q_add", "f8_q_aux")
VIT_M, UNI_M, UNI_T = 197 * 256, 128 * 256, 256       # ViT-B/16 at batch 256 (T = 197); unicom ViT-L/14 at batch 128 (T = 256)


def _f8(name, regime, M, N, K, epi, mode, **kw):
    return Case(name, G_F8[(mode, epi in QOUT_EPIS)], regime, M, N, K, epi, mode=mode, **kw)


CASES = (
    # ViT-B/16, batch 256 (hipnet.linear / linear_gelu_keep_derivative / linear_backward*): 9 to 36 tiles per row of 197 blocks
    Case("vit_qkv", G_TRUE0, "1773 tiles: 254 workgroups x 7, group_m 8", VIT_M, 2304, 768, "bias", cus256=True),
    Case("vit_proj", G_TRUE0, "591 tiles: 197 workgroups x 3", VIT_M, 768, 768, "bias_add", cus256=True),
    Case("vit_fc1", G_TRUE0, "2364 tiles: 237 x 10, group_m 8, GELU + GELU'", VIT_M, 3072, 768, "gelu2", cus256=True),
    Case("vit_fc2", G_TRUE0, "591 tiles: 197 x 3 at K = 3072", VIT_M, 768, 3072, "bias_add", cus256=True),
    Case("vit_fc2_dgrad", G_TRUE0, "2364 tiles, times the saved GELU'", VIT_M, 3072, 768, "mul", cus256=True),
    Case("vit_fc1_dgrad", G_TRUE0, "591 tiles: 197 x 3 at K = 3072", VIT_M, 768, 3072, "plain", cus256=True),
    Case("vit_qkv_dgrad", G_TRUE0, "591 tiles: 197 x 3 at K = 2304", VIT_M, 768, 2304, "plain", cus256=True),
    # unicom ViT-L/14 bf16, batch 128: 2048-tile launches (256 x 8, group_m 8), drop-path scale in the residual epilogue
    Case("uni_fc1", G_TRUE0, "2048 tiles: 256 x 8, group_m 8, ReLU6", UNI_M, 4096, 1024, "bias_relu6", cus256=True),
    Case("uni_fc2_dgrad", G_TRUE0, "2048 tiles, ReLU6 mask", UNI_M, 4096, 1024, "mask6", cus256=True),
    Case("uni_proj", G_TRUE0, "512 tiles: 256 x 2, row_scale", UNI_M, 1024, 1024, "rowscale", cus256=True),
    Case("uni_fc2", G_TRUE0, "512 tiles: 256 x 2 at K = 4096, row_scale", UNI_M, 1024, 4096, "rowscale", cus256=True),
    # unicom fp8, both operand modes: fc1 (ReLU6 bits + fp8 copy), fc2 data gradient (mask bits + fp8 copy + column sums), residuals
    *(_f8(f"uni8_fc1_m{m}", "2048 tiles: 256 x 8, group_m 8", UNI_M, 4096, 1024, "f8_relu6_bits", m, cus256=True) for m in (0, 1)),
    *(_f8(f"uni8_fc2_dgrad_m{m}", "2048 tiles: 256 x 8, group_m 8, colsum", UNI_M, 4096, 1024, "f8_mask_colsum", m, cus256=True)
      for m in (0, 1)),
    *(_f8(f"uni8_proj_m{m}", "512 tiles: 256 x 2, row_scale", UNI_M, 1024, 1024, "f8_res", m, cus256=True) for m in (0, 1)),
    *(_f8(f"uni8_fc1_dgrad_m{m}", "512 tiles: 256 x 2 at K = 4096, residual", UNI_M, 1024, 4096, "f8_add", m, cus256=True)
      for m in (0, 1)),
    # ResNet-50 at batch 256: layer3's 1024 -> 256 1x1 on 14 x 14 with BatchNorm statistics (196 tiles, one per workgroup)
    Case("rn50_l3_stats", G_FALSE0, "196 tiles, one per workgroup, LDS epilogue", 256 * 196, 256, 1024, "stats"),
    # ragged rows on the companion: R = 1 ... 128, split counts S = 1 ... 16, every ragged-eligible epilogue
    Case("ragged_R1", G_R1, "R = 1, S = 16", 64 * 256 + 1, 1024, 4096, "gelu2", companion=True, cus256=True),
    Case("ragged_R63", G_R1, "R = 63, S = 8, strided", 64 * 256 + 63, 1024, 1024, "bias_add", pad=(64, 0, 64, 128), companion=True,
         cus256=True),
    Case("ragged_R64", G_R1, "R = 64, S = 1 (K = 128)", 64 * 256 + 64, 1024, 128, "mul", companion=True, everywhere=True,
         cus256=True),
    Case("ragged_R65", G_R2, "R = 65, S = 16", 64 * 256 + 65, 1024, 4096, "mask6", companion=True, cus256=True),
    Case("ragged_R127", G_R2, "R = 127, S = 8, 64 column blocks", 16 * 256 + 127, 4096, 1024, "bias_relu", companion=True, cus256=True),
    Case("ragged_R128", G_R2, "R = 128, S = 2", 64 * 256 + 128, 1024, 256, "bias_relu6", companion=True, everywhere=True, cus256=True),
    Case("ragged_not_taken", G_TRUE0, "M % 256 = 100 on the persistent kernel (256 tiles: no round saved)", 63 * 256 + 100, 1024, 1024,
         "bias_add", cus256=True),
    # fp8 with a ragged last row block at a multi-tile walk (the round-5 memory fault)
    _f8("f8_ragged_m0", "336 tiles: 168 x 2, M % 256 = 77", 20 * 256 + 77, 4096, 1024, "f8_relu6_bits", 0, cus256=True),
    _f8("f8_ragged_m1", "336 tiles: 168 x 2, M % 256 = 77", 20 * 256 + 77, 4096, 1024, "f8_mask_colsum", 1, cus256=True),
    # small M
    *(Case(f"small_M{m}", G_TRUE0, "one partial row block", m, 256, 256, "bias_add", everywhere=True) for m in (1, 255, 257)),
    _f8("small8_M1", "one row", 1, 256, 256, "f8_res", 0),
    _f8("small8_M257", "two row blocks, one row in the second", 257, 512, 256, "f8_q_aux", 1),
    # strided operands (ldx > K, ldw > K, ldy > N, ldadd > N) at a multi-tile shape, one per instance (the bf16 entry points keep ldw = K)
    Case("strided_true0", G_TRUE0, "304 tiles: 152 x 2, strided", 75 * 256 + 30, 1024, 256, "bias_add", pad=(64, 0, 64, 128),
         everywhere=True, cus256=True),
    Case("strided_stats", G_FALSE0, "82 tiles, strided", 40 * 256 + 17, 512, 768, "stats", pad=(64, 0, 72, 0), everywhere=True),
    _f8("strided8_m0", "52 tiles, strided", 12 * 256 + 5, 1024, 512, "f8_res", 0, pad=(64, 128, 64, 32)),
    _f8("strided8_m1", "52 tiles, strided", 12 * 256 + 5, 1024, 512, "f8_add", 1, pad=(32, 16, 8, 96)),
    _f8("strided8_q_m0", "52 tiles, strided", 12 * 256 + 5, 1024, 512, "f8_q_add", 0, pad=(64, 128, 64, 32)),
    _f8("strided8_q_m1", "52 tiles, strided", 12 * 256 + 5, 1024, 512, "f8_q_aux", 1, pad=(16, 48, 24, 0)),
)


def ragged_split(K: int, N: int) -> int:
    """the K-split count S g8_launch_ragged picks (csrc/gemm8p.hip)"""
    blocks, deep, S = N // RAGGED_COLS, 256 if K >= 2048 else 128, 1
    for c in range(2, 17):
        if K % (32 * c) == 0 and K // c >= deep and blocks * c <= 768:
            S = c
    return S


def geo_of(case: Case, M: int) -> Geo:
    R = M % TILE
    return Geo(fp8=case.fp8, ragged=(M - R, ragged_split(case.K, case.N)) if case.companion and R else None)


def cpu_M(case: Case) -> int:
    """M for the CPU proof: the case's own where it is small, else two row blocks plus the case's ragged rest (or 100 rows)"""
    if case.M <= 3 * TILE:
        return case.M
    return 2 * TILE + (case.M % TILE or 100)


def make(case: Case, M: int, device, seed: int = 0):
    """Operands of a case at M rows on `device`: x [M][K] and w [N][K] as bf16 (bf16 cases) or fp8 (fp8 cases) tensors, their
    float64 values xv / wv (fp8: the decoded values), and the Epi with everything the launch reads.  Outputs are O(1)."""
    g = torch.Generator(device=device).manual_seed(seed)
    N, K = case.N, case.K

    def rn(*shape):
        return torch.randn(*shape, generator=g, device=device)

    ep = Epi()
    if case.fp8:
        tx = torch.float8_e5m2 if case.mode == 1 else torch.float8_e4m3fn
        limx = 57344.0 if case.mode == 1 else 448.0
        sx, sw = f32(limx / 3.7), f32(448.0 * math.sqrt(K) / 3.9)
        x = (rn(M, K) * sx).clamp(-limx, limx).to(tx)
        w = (rn(N, K) * sw).clamp(-448.0, 448.0).to(torch.float8_e4m3fn)
        ep.deq = (f32(1 / sx), f32(1 / sw))
    else:
        x = rn(M, K).to(torch.bfloat16)
        w = (rn(N, K) / math.sqrt(K)).to(torch.bfloat16)
    xv, wv = x.double(), w.double()
    u6 = lambda: (rn(M, N) * 4).clamp(0, 6).to(torch.bfloat16)          # a ReLU6 output: zeros, interior values and sixes
    e = case.epi
    if e in ("bias", "bias_relu", "bias_relu6", "bias_add", "rowscale", "gelu2", "f8_relu6_bits", "f8_res", "f8_q_add"):
        ep.bias = rn(N) * {"bias_relu6": 1.0, "f8_relu6_bits": 3.0}.get(e, 0.5)       # (3: a good share of the fp8 fc1 outputs clamp at 6)
    if e in ("bias_add", "rowscale", "f8_res", "f8_add", "f8_q_add"):
        ep.add = rn(M, N).to(torch.bfloat16)
    if e in ("rowscale", "f8_res"):
        ep.rows_per_sample = UNI_T if M >= UNI_T else 50
        S = -(-M // ep.rows_per_sample)
        ep.row_scale = (torch.arange(S, device=device) % 3 != 2).float() / 0.75   # kept samples 1 / 0.75, dropped 0
    if e == "mul":
        ep.aux = (rn(M, N) * 0.5 + 0.5).to(torch.bfloat16)
    if e in ("mask6", "f8_q_aux"):
        ep.aux, ep.aux_mode = u6(), 1
    if e == "f8_mask_colsum":
        a = u6()
        ep.mask_in = (a > 0) & (a < 6)
        if M % TILE == 0:
            ep.colsum = torch.full((N,), 0.5, device=device)
    ep.relu = {"bias_relu": 1, "bias_relu6": 2, "f8_relu6_bits": 2, "gelu2": 3}.get(e, 0)
    ep.stats = e == "stats"
    if e in ("f8_relu6_bits", "f8_q_add"):
        ep.yq = (56.0, 0)
    if e in ("f8_mask_colsum", "f8_q_aux"):
        ep.yq = (f32(57344.0 / 9.0), 1)
    ep.mask_out = e == "f8_relu6_bits"
    return x, w, xv, wv, ep


__all__ = ["Case", "CASES", "INSTANCES", "make", "cpu_M", "geo_of", "ragged_split", "Epi", "Geo", "outputs", "product", "ratio", "MUTANTS", "C_BOUND", "FLOOR", "RMS_FLOOR", "bf", "quantize", "unpack_bits",
           "bits_agree", "amax_agrees", "outputs_of", "worst_mutant_ratio", "replace"]
