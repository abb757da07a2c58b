"""Every instance of the gemm8p GEMM core (csrc/gemm8p.hip: gemm8p_kernel<false,0> / <true,0>, the fp8 forms <true,1|2[,true]> and
gemm8p_ragged_kernel<1|2>) against the float64 reference of tests/gemm_reference.py, at the step's own launches (ViT-B/16, unicom
bf16 and fp8, ResNet-50 at full M), ragged rows on the companion, fp8 with a ragged row block, small M and strided operands.

Outputs sit inside guard rows and padding columns holding a finite sentinel that must come back unchanged; output regions start as
NaN; input padding columns and the rows past M hold finite garbage.  Every output is held to max(C_BOUND * yardstick error, FLOOR)
per tile and prints a "RATIO instance case output err= bound= ratio=" line (visible with -rP); a second run is bit-identical; the
fp8 copy, its amax and the mask bits are bit-exact against the separate quantise pass / the stored output; launch counters show
that the intended kernel ran.  tests/test_gemm_reference.py proves on the CPU that the bound rejects subtly wrong kernels."""
import pytest
import torch

import gemm_reference as gr

pytestmark = pytest.mark.gpu

from nkb_classification import hip  # noqa: E402

DEV = "cuda"
G = 4                   # guard rows on each side of an output
GR = 3                  # garbage rows past M of an input
SENT = -8192.0          # bf16 / fp32-exact sentinel of the guard zones
BYTE_SENT = 0x5A
GARBAGE = {torch.bfloat16: 1e4, torch.float8_e4m3fn: 448.0, torch.float8_e5m2: 8192.0, torch.uint8: 0xFF}
COUNTERS = ("gemm8p", "gemm8p_ragged", "gemm_fp8")
RAN = set()


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _input(t, ld):
    """t [M][C] inside a [M + GR][ld] buffer: padding columns and the rows past M hold finite garbage"""
    M, C = t.shape
    buf = torch.full((M + GR, ld), GARBAGE[t.dtype], device=DEV).to(t.dtype)
    buf[:M, :C] = t
    return buf


def _output(M, N, ld, dtype=torch.bfloat16, fill=float("nan"), sent=SENT):
    """a [G + M + G][ld] buffer: guards and padding columns hold the sentinel, the output region `fill`; returns (buffer, view at row G)"""
    buf = torch.full((G + M + G, ld), sent, device=DEV, dtype=dtype)
    buf[G:G + M, :N] = fill
    return buf, buf[G:]


def _guards_intact(buf, M, N, sent):
    s = torch.full_like(buf[:1, :1], sent)
    ok = bool((buf[:G] == s).all()) and bool((buf[G + M:] == s).all())
    return ok and bool((buf[G:G + M, N:] == s).all())


def _bits(t):
    return t.view(torch.uint8) if t.dtype.itemsize == 1 else t.view(torch.int16) if t.dtype.itemsize == 2 else t.view(torch.int32)


def _pack_mask(mask):
    M, N = mask.shape
    sh = torch.arange(8, device=mask.device, dtype=torch.int32)
    return ((mask.reshape(M, N // 8, 8).to(torch.int32) << sh).sum(-1)).to(torch.uint8)


def _launch(case, M, x, w, ep, ldx, ldw, ldy, ldadd, keep_y=True):
    """one launch of the case's entry point on the current stream; returns the output buffers (name -> (buffer, rows, cols, sentinel))"""
    N, K = case.N, case.K
    bufs = {}
    ybuf, y = _output(M, N, ldy)
    bufs["y"] = (ybuf, M, N, SENT)
    bias = ep.bias
    add = _input(ep.add, ldadd) if ep.add is not None else None
    if not case.fp8:
        y2 = None
        if ep.relu == 3:
            y2buf, y2 = _output(M, N, ldy)
            bufs["y2"] = (y2buf, M, N, SENT)
        if case.epi == "rowscale":
            hip.linear_residual_scaled(hip.BF16, x, w, bias, add, ep.row_scale, ep.rows_per_sample, y, M, K, N)
        elif case.epi == "mul":
            hip.linear_gelu(hip.BF16, 4, x, w, None, _input(ep.aux, N), y, None, M, K, N)
        elif case.epi == "mask6":
            hip.linear_gelu(hip.BF16, 3, x, w, None, _input(ep.aux, N), y, None, M, K, N)
        elif case.epi == "gelu2":
            hip.linear_gelu(hip.BF16, 5, x, w, bias, None, y, y2, M, K, N)
        else:
            stats = None
            if ep.stats:
                P = hip.stat_tiles(hip.BF16, M, N)
                assert P == (M + 127) // 128
                sbuf = torch.full((P + 1, 2, N), SENT, device=DEV)
                sbuf[:P] = float("nan")
                stats = sbuf
                bufs["stats"] = (sbuf, P, N, SENT)
            hip.conv_gemm(hip.BF16, 0, x, w, y, N=M, H=1, W=1, Cin=K, ldx=ldx, P=1, Q=1, Cout=N, ldy=ldy, bias=bias, relu=ep.relu,
                          add=add, ldadd=ldadd if add is not None else 0, stats=stats)
        return bufs
    kw = {}
    if ep.yq is not None:
        qscale, kind = ep.yq
        qbuf, yq = _output(M, N, N, torch.uint8, 0x7F, BYTE_SENT)
        st = torch.tensor([qscale, 1.0 / qscale, 0.0], device=DEV)
        bufs["yq"] = (qbuf, M, N, BYTE_SENT)
        bufs["q_state"] = (st, None, None, None)
        kw.update(yq=yq, q_state=st, q_kind=kind)
    if ep.mask_out:
        bbuf, bits = _output(M, N // 8, N // 8, torch.uint8, 0xAA, BYTE_SENT)
        bufs["bits"] = (bbuf, M, N // 8, BYTE_SENT)
        kw.update(mask_out=bits)
    if ep.mask_in is not None:
        kw.update(mask_in=_input(_pack_mask(ep.mask_in), N // 8))
    if ep.colsum is not None:
        cs = ep.colsum.clone()
        bufs["colsum"] = (cs, None, None, None)
        kw.update(colsum=cs, colsum_work=torch.empty(M // 256 * N, device=DEV))
    if ep.aux is not None:
        kw.update(aux=_input(ep.aux, ldy), aux_mode=ep.aux_mode)
    if ep.row_scale is not None:
        kw.update(row_scale=ep.row_scale, rows_per_sample=ep.rows_per_sample)
    dx = torch.tensor([ep.deq[0]], device=DEV)
    dw = torch.tensor([ep.deq[1]], device=DEV)
    hip.gemm_fp8(case.mode, x.view(torch.uint8), w.view(torch.uint8), y if keep_y else None, M, K, N, deq_x=dx, deq_w=dw, bias=bias,
                 add=add, ldadd=ldadd if add is not None else 0, ldx=ldx, ldw=ldw, ldy=ldy, relu=ep.relu, **kw)
    if not keep_y:
        del bufs["y"]
    return bufs


def _hold(case, out, got, ref, yard, geo):
    r, err, bound = gr.ratio(got, ref, yard, out, geo)
    print(f"RATIO {case.instance} {case.name} {out} err={err:.3e} bound={bound:.3e} ratio={r:.3f}")
    assert r <= 1.0, f"{case.name}: {out} error {err:.3e} > bound {bound:.3e} in its worst tile"


@pytest.mark.parametrize("case", gr.CASES, ids=lambda c: c.name)
def test_gemm8p_instance_against_float64_reference(case):
    if case.cus256 and _cus() != 256:
        pytest.skip("the walk regime of this case is the one 256 CUs give")
    M, N, K = case.M, case.N, case.K
    ldx, ldw, ldy, ldadd = K + case.pad[0], K + case.pad[1], N + case.pad[2], N + case.pad[3]
    x, w, xv, wv, ep = gr.make(case, M, DEV, seed=7)
    geo = gr.geo_of(case, M)
    xb, wb = _input(x, ldx), _input(w, ldw)
    if case.everywhere:
        hip.gemm8p_config(True, 1, 128)
    try:
        runs = []
        for r in range(2):
            n0 = {k: hip.kernel_launches(k) for k in COUNTERS}
            runs.append(_launch(case, M, xb, wb, ep, ldx, ldw, ldy, ldadd))
            torch.cuda.synchronize()
            dn = {k: hip.kernel_launches(k) - n0[k] for k in COUNTERS}
            if case.fp8:
                assert dn == dict(gemm8p=0, gemm8p_ragged=0, gemm_fp8=1), dn
            else:
                assert dn == dict(gemm8p=1, gemm8p_ragged=int(geo.ragged is not None), gemm_fp8=0), dn
        extra = None
        if case.fp8 and (ep.mask_out or ep.colsum is not None):      # the engine's form: no bf16 output at all
            extra = _launch(case, M, xb, wb, ep, ldx, ldw, ldy, ldadd, keep_y=False)
            torch.cuda.synchronize()
    finally:
        if case.everywhere:
            hip.gemm8p_config(True, 192, 768)
    a, b = runs
    for name, (buf, rows, cols, sent) in a.items():
        assert torch.equal(_bits(buf), _bits(b[name][0])), f"{case.name}: {name} differs between two runs"
        if name == "stats":
            assert bool((buf[rows:] == sent).all()), f"{case.name}: statistics written past their {rows} partial rows"
        elif rows is not None:
            assert _guards_intact(buf, rows, cols, sent), f"{case.name}: {name} wrote outside its rows / columns"
    if extra is not None:
        for name, (buf, *_rest) in extra.items():
            assert torch.equal(_bits(buf), _bits(a[name][0])), f"{case.name}: {name} differs without the bf16 output"
    RAN.add(case.instance)
    if geo.ragged is not None:
        RAN.add(gr.G_R1 if M % 256 <= 64 else gr.G_R2)
    # against the float64 reference
    y = a["y"][0][G:G + M, :N]
    assert torch.isfinite(y.float()).all()
    p = gr.product(xv, wv)
    ref = gr.outputs(p, ep, exact=True)
    yard = gr.outputs(p, ep, exact=False)
    got = {"y": y.double()}
    if "y2" in a:
        got["y2"] = a["y2"][0][G:G + M, :N].double()
    if "stats" in a:
        st = a["stats"][0][:a["stats"][1]].double()
        got["stats_sum"], got["stats_sq"] = st[:, 0], st[:, 1]
    if "yq" in a:
        qscale, kind = ep.yq
        yq = a["yq"][0][G:G + M]
        got["yq"] = yq.view(gr.FP8[kind][0]).double() / qscale
        # bit-exact against the separate quantise pass over the stored output, amax included
        st2 = torch.tensor([qscale, 1.0 / qscale, 0.0], device=DEV)
        yq2 = torch.empty(M, N, device=DEV, dtype=torch.uint8)
        yc = y.contiguous()
        hip.fp8_quantize(hip.BF16, kind, yc, M * N, st2, yq2)
        torch.cuda.synchronize()
        assert torch.equal(yq, yq2)
        amax = a["q_state"][0][2].item()
        assert amax == st2[2].item() == yc.float().abs().max().item()
        assert gr.amax_agrees(amax, ref["y"])
    if "bits" in a:
        bits = gr.unpack_bits(a["bits"][0][G:G + M])
        yf = y.float()
        assert torch.equal(bits, (yf > 0) & (yf < 6))
        assert gr.bits_agree(bits, ref["pre"])
    if "colsum" in a:
        got["colsum"] = a["colsum"][0].double()
    for out in gr.outputs_of(ep):
        _hold(case, out, got[out], ref[out], yard[out], geo)


def test_ragged_companion_on_two_streams():
    """Interleaved ragged-eligible launches on two streams (A1, A2 on one, then B1, B2 on the other) and one more on the default
    stream: concurrent companions must not share their fp32 slabs or tickets.  Every output equals its single-stream result bitwise."""
    if _cus() != 256:
        pytest.skip("the companion is taken for this shape on 256 CUs")
    M, N, K = 64 * 256 + 65, 1024, 4096                     # R = 65 rows on the companion, S = 16 splits
    g = torch.Generator(device=DEV).manual_seed(5)
    xs = [torch.randn(M, K, generator=g, device=DEV).to(torch.bfloat16) for _ in range(5)]
    w = (torch.randn(N, K, generator=g, device=DEV) / K ** 0.5).to(torch.bfloat16)
    bias = torch.randn(N, generator=g, device=DEV)

    def launch(x, y):
        hip.conv_gemm(hip.BF16, 0, x, w, y, N=M, H=1, W=1, Cin=K, ldx=K, P=1, Q=1, Cout=N, ldy=N, bias=bias)

    want = []
    for x in xs:
        y = torch.full((M, N), float("nan"), device=DEV, dtype=torch.bfloat16)
        launch(x, y)
        want.append(y)
    torch.cuda.synchronize()
    ys = [torch.full((M, N), float("nan"), device=DEV, dtype=torch.bfloat16) for _ in xs]
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    sa.wait_stream(torch.cuda.current_stream())
    sb.wait_stream(torch.cuda.current_stream())
    n0 = hip.kernel_launches("gemm8p_ragged")
    with torch.cuda.stream(sa):
        launch(xs[0], ys[0])
        launch(xs[1], ys[1])
    with torch.cuda.stream(sb):
        launch(xs[2], ys[2])
        launch(xs[3], ys[3])
    launch(xs[4], ys[4])
    torch.cuda.synchronize()
    assert hip.kernel_launches("gemm8p_ragged") == n0 + 5
    for i, (y, ref) in enumerate(zip(ys, want)):
        assert torch.equal(_bits(y), _bits(ref)), f"launch {i} differs from its single-stream result"


def test_every_instance_ran():
    if _cus() != 256:
        pytest.skip("the full-M cases run on 256 CUs only")
    assert RAN == set(gr.INSTANCES), sorted(set(gr.INSTANCES) - RAN)
