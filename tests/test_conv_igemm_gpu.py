"""Every instance of conv_igemm_kernel<T, TC, TP, BNB, HALO> (csrc/conv_igemm.hip) against the float64 reference of
tests/conv_reference.py, through the ten entry points that reach it, at non-square grids, padded leading dimensions, ragged row and
channel tails, image boundaries inside a tile, the parity classes of the stride-2 data gradient, K-concatenated and batched
products, and one launch on the grouped tile walk.

Outputs, bit arrays and statistics sit inside guard rows and padding columns holding a finite sentinel that must come back
unchanged; output regions start as NaN; padding columns and trailing rows of every input hold finite garbage (1e4), padding bytes
of the bit arrays 0xFF.  Every case is held to the derived bounds of conv_reference (element, tile, statistics against the stored
output, bit-exact masks, the cap on BN-mask elements left out), prints "RATIO instance case output err= bound= ratio=" for its
worst tile and "ELEM ..." for its worst element (visible with -rP), is bit-identical on a second launch, must have run the instance
its case names (nkb_conv_last_instance) and must leave the gemm8p / convp launch counters alone.  tests/test_conv_reference.py
proves on the CPU that these bounds reject subtly wrong kernels."""
import pytest
import torch

import conv_reference as cr

pytestmark = pytest.mark.gpu

from nkb_classification import hip  # noqa: E402

DEV = "cuda"
G = 4                   # guard rows on each side of an output
GR = 3                  # garbage rows past the end of an input
SENT = -8192.0          # bf16 / fp32-exact sentinel of the guard zones
BYTE_SENT = 0x5A
GARBAGE = 1e4
COUNTERS = ("gemm8p", "gemm8p_ragged", "convp")
RAN = {}


def _input(t, ld, garbage=GARBAGE):
    """t [rows][C] inside a [rows + GR][ld] buffer: padding columns and the rows past the end hold finite garbage"""
    rows, C = t.shape
    buf = torch.full((rows + GR, ld), garbage, device=DEV).to(t.dtype)
    buf[:rows, :C] = t
    return buf


def _bits_input(mask, dtype, ld):
    b = cr.pack_bits(mask, dtype, ld, fill=0xFF)
    return torch.cat([b, torch.full((GR, b.shape[1]), 0xFF, dtype=torch.uint8, device=DEV)])


def _output(rows, cols, ld, dtype, fill=float("nan"), sent=SENT):
    """a [G + rows + G][ld] buffer: guards and padding columns hold the sentinel, the output region `fill`; (buffer, view at row G)"""
    buf = torch.full((G + rows + G, ld), sent, device=DEV, dtype=dtype)
    buf[G:G + rows, :cols] = fill
    return buf, buf[G:]


def _guards_intact(buf, rows, cols, sent):
    b = buf.reshape(-1, G + rows + G, buf.shape[-1])
    s = torch.full_like(b[:1, :1, :1], sent)
    return bool((b[:, :G] == s).all()) and bool((b[:, G + rows:] == s).all()) and bool((b[:, G:G + rows, cols:] == s).all())


def _raw(t):
    return t.view(torch.uint8) if t.dtype.itemsize == 1 else t.view(torch.int16) if t.dtype.itemsize == 2 else t.view(torch.int32)


def _launch(c, d):
    """one launch of the case's entry point; returns {name: (buffer, rows, cols, sentinel)} of everything it writes"""
    dt = cr.TORCH_DT[c.dtype]
    hd = hip.dt(dt)
    P, Q, M, Mfull, _, _, Ktot = cr.dims(c)
    C = c.Cout
    ldx, ldy, ldadd = c.Cin + c.pads[0], C + c.pads[1], C + c.pads[2]
    ydt = torch.float32 if d.out_f32 else dt
    Z = c.batch[0] * c.batch[1]
    bufs = {}
    if c.entry == "batched":
        outer, inner = c.batch
        K, Kp = c.Cin, c.Cin + c.pads[0]
        xb = torch.full((outer * M + GR, inner, Kp), GARBAGE, device=DEV).to(dt)
        xb[:outer * M, :, :K] = d.x.reshape(outer, inner, M, K).permute(0, 2, 1, 3).reshape(outer * M, inner, K)
        wb = torch.full((Z, C + GR, Kp), GARBAGE, device=DEV).to(dt)
        wb[:, :C, :K] = d.w
        ybuf = torch.full((Z, G + M + G, ldy), SENT, device=DEV, dtype=ydt)
        ybuf[:, G:G + M, :C] = float("nan")
        bufs["y"] = (ybuf, M, C, SENT)
        rows_y = (G + M + G) * ldy
        hip.gemm_batched(hd, xb, wb, ybuf[0, G:], M, C, K, inner * Kp, Kp, ldy, outer, inner, (M * inner * Kp, Kp),
                         (inner * (C + GR) * Kp, (C + GR) * Kp), (inner * rows_y, rows_y), out_f32=d.out_f32)
        return bufs
    x = _input(d.x, ldx)
    w = _input(d.w, Ktot)
    ybuf, y = _output(Mfull, C, ldy, ydt)
    bufs["y"] = (ybuf, Mfull, C, SENT)
    add = _input(d.add, ldadd) if d.add is not None else None
    add_bits = _bits_input(d.add_bits, c.dtype, ldadd) if d.add_bits is not None else None
    cbuf = _input(d.c, ldy) if d.c is not None else None
    bn_bits = _bits_input(d.bn_bits, c.dtype, ldy) if d.bn_bits is not None else None
    x2 = _input(d.x2, c.K2 + c.pads[0]) if d.x2 is not None else None
    stats = None
    if d.stats:
        T = hip.stat_tiles(hd, M, C)
        assert T == -(-M // c.inst.tp)
        stats = torch.full((T + 1, 2, C), SENT, device=DEV)
        stats[:T] = float("nan")
        bufs["stats"] = (stats, T, C, SENT)
    obits = None
    if d.out_bits:
        bbuf, obits = _output(Mfull, C // 8, ldy // 8, torch.uint8, 0xAA, BYTE_SENT)
        bufs["bits"] = (bbuf, Mfull, C // 8, BYTE_SENT)
    geom = dict(N=c.N, H=c.H, W=c.W, Cin=c.Cin, ldx=ldx, P=P, Q=Q, Cout=C, ldy=ldy, R=c.R, S=c.S, stride=c.stride, pad=c.pad)
    if c.entry == "conv_gemm":
        hip.conv_gemm(hd, c.mode, x, w, y, add=add, ldadd=ldadd if add is not None else 0, bias=d.bias, stats=stats, relu=d.relu,
                      out_f32=d.out_f32, add_hw=d.add_hw, add_bits=add_bits, **geom)
    elif c.entry == "dgrad_bn":
        hip.conv_dgrad_bn(hd, x, w, y, cbuf, d.scale, d.shift, d.mean, stats, relu_bits=bn_bits, add=add,
                          ldadd=ldadd if add is not None else 0, add_bits=add_bits, add_hw=d.add_hw, **geom)
    elif c.entry == "s2class":
        hip.conv_dgrad_s2class(hd, x, w, y, add, cbuf, d.scale, d.shift, d.mean, stats, c.N, c.H, c.W, c.Cin, ldx, c.out[0], c.out[1],
                               C, ldy, ldadd if add is not None else 0, c.cls[0], c.cls[1], d.add_hw[0], d.add_hw[1])
    elif c.entry == "affine":
        hip.conv_affine_residual(hd, x, w, y, d.oscale, d.bias, add, ldadd, d.res_scale, d.res_shift, obits, **geom)
    elif c.entry == "cat_relu_bits":
        hip.conv_cat_relu_bits(hd, x, ldx, c.Cin, x2, x2.shape[1], c.K2, w, d.bias, y, obits, M, C, ldy)
    elif c.entry == "cat_bias":
        hip.conv_cat_bias(hd, x, ldx, c.Cin, x2, x2.shape[1], c.K2, w, d.bias, y, M, C, ldy)
    elif c.entry == "dgrad_bn_cat":
        hip.conv_dgrad_bn_cat(hd, x, ldx, c.Cin, x2, x2.shape[1], c.K2, w, d.bias, y, cbuf, d.scale, d.shift, d.mean, stats, M, C, ldy)
    elif c.entry == "dgrad_bn_add":
        hip.conv_dgrad_bn_add(hd, x, ldx, c.Cin, w, d.bias, add, ldadd, y, cbuf, d.scale, d.shift, d.mean, stats, M, C, ldy)
    elif c.entry == "linear_gelu":
        y2 = None
        if c.act == 1:
            y2buf, y2 = _output(M, C, ldy, dt)
            bufs["y2"] = (y2buf, M, C, SENT)
        aux = _input(d.aux, ldy) if d.aux is not None else None
        hip.linear_gelu(hd, c.act, x, w, d.bias, aux, y, y2, M, c.Cin, C)
    else:
        raise AssertionError(c.entry)
    return bufs


@pytest.mark.parametrize("case", cr.CASES, ids=lambda c: c.name)
def test_conv_igemm_instance_against_float64_reference(case):
    c = case
    d = cr.make(c, DEV, seed=11)
    P, Q, M, Mfull, *_ = cr.dims(c)
    runs = []
    for _ in range(2):
        n0 = {k: hip.kernel_launches(k) for k in COUNTERS}
        runs.append(_launch(c, d))
        code = hip.conv_last_instance()
        torch.cuda.synchronize()
        assert {k: hip.kernel_launches(k) - n0[k] for k in COUNTERS} == dict.fromkeys(COUNTERS, 0), "the launch went to another core"
        assert code & ~cr.GROUPED_BIT == c.inst.code, f"{c.name}: ran instance code {code:#x}, the case names {c.inst} ({c.inst.code:#x})"
        assert bool(code & cr.GROUPED_BIT) == c.grouped, f"{c.name}: grouped tile walk {bool(code & cr.GROUPED_BIT)}"
    RAN[c.inst] = RAN.get(c.inst, 0) + 1
    a, b = runs
    for name, (buf, rows, cols, sent) in a.items():
        assert torch.equal(_raw(buf), _raw(b[name][0])), f"{c.name}: {name} differs between two launches"
        if name == "stats":
            assert bool((buf[rows:] == sent).all()), f"{c.name}: statistics written past their {rows} tile rows"
        else:
            assert _guards_intact(buf, rows, cols, sent), f"{c.name}: {name} wrote outside its rows / columns"
    ybuf, rows, C, _ = a["y"]
    got = {"y": ybuf.reshape(-1, G + rows + G, ybuf.shape[-1])[:, G:G + rows, :C].reshape(-1, C).double(), "past": False}
    if "y2" in a:
        got["y2"] = a["y2"][0][G:G + M, :C].double()
    if "stats" in a:
        got["stats"] = a["stats"][0][:a["stats"][1]].double()
    if "bits" in a:
        got["bits"] = cr.unpack_bits(a["bits"][0][G:G + Mfull], c.dtype, C)
    ref = cr.outputs(c, d, exact=True)
    yard = cr.outputs(c, d, exact=False)
    v = cr.verdict(c, d, ref, yard, got)
    for name, (ratio, err, bound) in v.items():
        kind = "RATIO" if name.endswith("_tile") else "ELEM"
        print(f"{kind} {c.inst} {c.name} {name} err={err:.3e} bound={bound:.3e} ratio={ratio:.3f}")
    for name, (ratio, err, bound) in v.items():
        assert ratio <= 1.0, f"{c.name}: {name} error {err:.3e} > bound {bound:.3e} ({c.inst})"


def test_every_instance_ran(request):
    """the instances this session's cases ran are the whole list the dispatch can produce"""
    if request.config.getoption("keyword"):
        pytest.skip("run with a -k selection: not every case ran")
    assert set(RAN) == set(cr.INSTANCES), sorted(map(str, set(cr.INSTANCES) ^ set(RAN)))
