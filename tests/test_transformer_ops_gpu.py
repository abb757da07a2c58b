"""nkb_layernorm (with nkb_layernorm_param_reduce), nkb_gelu, nkb_gelu_fwd_dgelu, nkb_relu6, nkb_scale_rows, nkb_attn_softmax,
nkb_head_transpose, nkb_vit_assemble, nkb_colsum2d and nkb_dropout (csrc/transformer.hip) against the float64 reference of
tests/transformer_reference.py, at the smallest shapes at which each path of their dispatch can go wrong: every LayerNorm width
class (full-lane VW 4 / VW 2, the masked tail) at row counts around the four-rows-per-block walk, the second trip of every grid cap,
the partial-row counts that leave slices of the parameter reduction empty or uneven, all three parameter-gradient forms, the
64-register backward next to the register form, the second outputs; the vector and scalar paths of the token assembly; the split
counts at which the column-sum reduction switches kernel.

Outputs sit inside guard rows holding a finite sentinel that must come back unchanged; output regions start as NaN; the columns
between the width and the stride hold a sentinel in outputs (it must survive) and finite garbage (1e4) in inputs (a masked lane must
not read it); garbage rows sit behind every input; workspaces have exactly the advertised size plus a sentinel tail.  Every case
runs twice and must repeat bit for bit, except the outputs of the forms documented as atomic (the atomic LayerNorm parameter
gradients and the atomic column sums over more than one block): their summation order is not fixed, so each of the two launches is
held to the reduction bound instead (exact cases: value for value).  Every case prints "RATIO kernel case output err= bound= ratio="
for its worst element (visible with -rP).  tests/test_transformer_reference.py proves on the CPU that these checks reject subtly
wrong kernels."""
import pytest
import torch

import transformer_reference as tr

pytestmark = pytest.mark.gpu

from nkb_classification import hip  # noqa: E402

DEV = "cuda"
G = 4                   # guard rows on each side of an output
GR = 3                  # garbage rows past the end of an input
GF = 64                 # guard elements on each side of a flat output
SENT = -8192.0          # bf16 / fp32-exact sentinel of the guard zones
BYTE_SENT = 0x5A
TAIL = 64               # sentinel floats behind a workspace
NAN = float("nan")
KERNEL = dict(ln="nkb_layernorm", act="nkb_gelu", scale="nkb_scale_rows", softmax="nkb_attn_softmax", transpose="nkb_head_transpose",
              assemble="nkb_vit_assemble", colsum="nkb_colsum2d", dropout="nkb_dropout")


class Out:
    """[G + rows + G][cols + pad]: the guard rows and the pad columns hold `sent`, the region between them `fill`"""

    def __init__(self, rows, cols, dtype, fill=NAN, sent=SENT, pad=0):
        self.rows, self.cols = rows, cols
        self.guard = torch.full((1,), sent, device=DEV, dtype=dtype)
        self.buf = torch.full((G + rows + G, cols + pad), sent, device=DEV, dtype=dtype)
        self.buf[G:G + rows, :cols] = fill
        self.view = self.buf[G:]
        self.data = self.buf[G:G + rows, :cols]

    def intact(self):
        return (bool((self.buf[:G] == self.guard).all()) and bool((self.buf[G + self.rows:] == self.guard).all())
                and bool((self.buf[:, self.cols:] == self.guard).all()))


def _vec(n, fill=NAN):
    return Out(1, n, torch.float32, fill)


def _flat(n, dtype, fill=NAN, sent=SENT):
    """n elements between GF guard elements: an Out of one row whose view starts at the data"""
    o = Out.__new__(Out)
    o.rows, o.cols = 1, n
    o.guard = torch.full((1,), sent, device=DEV, dtype=dtype)
    o.buf = torch.full((GF + n + GF,), sent, device=DEV, dtype=dtype)
    o.buf[GF:GF + n] = fill
    o.view = o.buf[GF:]
    o.data = o.buf[GF:GF + n]
    o.intact = lambda: bool((o.buf[:GF] == o.guard).all()) and bool((o.buf[GF + n:] == o.guard).all())
    return o


def _input(t, pad=0, garbage=tr.GARBAGE):
    """t [rows][C] (or [n]) followed by `pad` columns and GR rows of finite garbage"""
    if t.dim() == 1:
        return torch.cat([t, torch.full((GR * 8,), garbage, device=DEV).to(t.dtype)])
    t = t.reshape(-1, t.shape[-1])
    if pad:
        t = torch.cat([t, torch.full((t.shape[0], pad), garbage, device=DEV).to(t.dtype)], 1)
    return torch.cat([t, torch.full((GR, t.shape[1]), garbage, device=DEV).to(t.dtype)]).contiguous()


def _workspace(advertised):
    """exactly the advertised floats (NaN) plus a sentinel tail; (buffer, view)"""
    buf = torch.full((advertised + TAIL,), SENT, device=DEV)
    buf[:advertised] = NAN
    return buf, buf[:advertised]


def _raw(t):
    return t.view(torch.uint8) if t.dtype.itemsize == 1 else t.view(torch.int16) if t.dtype.itemsize == 2 else t.view(torch.int32)


def _ln_launch(c, d):
    """forward, then the backward in its three parameter-gradient forms; ({name: Out | (buffer, advertised)}, {form: got}, atomic)"""
    dt, hd = tr.TORCH_DT[c.dtype], hip.dt(tr.TORCH_DT[c.dtype])
    rows, D = c.rows, c.D
    ldx, ldg, ldo = D + c.pad[0], D + c.pad[1], D + c.pad[2]
    x, dy = _input(d.x, c.pad[0]), _input(d.dy, c.pad[1])
    add = _input(d.addv, c.pad[2]) if c.add else None
    bmean, brstd = _input(d.bmean), _input(d.brstd)
    fp8 = c.second in ("e4m3", "e5m2")
    kind = hip.E4M3 if c.second == "e4m3" else hip.E5M2
    state = lambda: torch.tensor([d.qscale, 1.0 / d.qscale, 0.0], device=DEV)
    o, got = {}, {}
    # forward
    o["y"] = Out(rows, D, dt, pad=c.pad[2])
    if c.stats:
        o["mean"], o["rstd"] = _vec(rows), _vec(rows)
    kw = {}
    if fp8:
        o["yq"] = Out(rows, D, torch.uint8, 0xAA, BYTE_SENT)
        st = state()
        kw = dict(yq=o["yq"].view, q_state=st, q_kind=kind)
    hip.layernorm_fwd(hd, x, ldx, d.gamma, d.beta, o["y"].view, ldo, o["mean"].view if c.stats else None, o["rstd"].view if c.stats else None,
                      rows, D, d.eps, **kw)
    got["fwd"] = dict(y=o["y"].data.double())
    if c.stats:
        got["fwd"].update(mean=o["mean"].data[0].double(), rstd=o["rstd"].data[0].double())
    if fp8:      # the bytes and the amax nkb_fp8_quantize makes of the stored rows
        st2, q2 = state(), torch.empty(rows, D, dtype=torch.uint8, device=DEV)
        hip.fp8_quantize(hip.BF16, kind, o["y"].data.contiguous(), rows * D, st2, q2)
        assert torch.equal(o["yq"].data, q2) and st[2].item() == st2[2].item(), f"{c.name}: forward fp8 copy"
    # backward
    adv = hip.layernorm_ws(D)
    assert adv == tr.ln_ws_floats(D)
    forms = ["work", "partial"] + (["atomic"] if not fp8 else [])
    for form in forms:
        dg, db, dx = _vec(D, d.dgamma0), _vec(D, d.dbeta0), Out(rows, D, dt, pad=c.pad[2])
        o[form + ".dgamma"], o[form + ".dbeta"], o[form + ".dx"] = dg, db, dx
        wbuf, ws = _workspace(adv)
        o[form + ".workspace"] = (wbuf, adv)
        kw, st, cs = {}, None, None
        if fp8:
            o[form + ".q"], cs, st = Out(rows, D, torch.uint8, 0xAA, BYTE_SENT), _vec(D, d.colsum0), state()
            o[form + ".colsum"] = cs
            kw = dict(yq=o[form + ".q"].view, q_state=st, q_kind=kind, row_scale=d.rsc if c.row_scale else None, rows_per_sample=c.rps,
                      colsum=cs.view)
        elif c.second == "scaled":
            o[form + ".copy"] = Out(rows, D, dt)
            kw = dict(yq=o[form + ".copy"].view, q_kind=2, row_scale=d.rsc, rows_per_sample=c.rps)
        if form == "partial":
            kw.pop("colsum", None)
            hip.layernorm_bwd(hd, dy, ldg, x, ldx, d.gamma, bmean, brstd, add, dx.view, ldo, None, None, rows, D, workspace=ws, **kw)
            hip.layernorm_param_reduce(ws, rows, D, 3 if fp8 else 2, dg.view, db.view, cs.view if fp8 else None)
        else:
            hip.layernorm_bwd(hd, dy, ldg, x, ldx, d.gamma, bmean, brstd, add, dx.view, ldo, dg.view, db.view, rows, D,
                              workspace=ws if form == "work" else None, **kw)
        g = dict(dx=dx.data.double(), dgamma=dg.data[0].double(), dbeta=db.data[0].double())
        if fp8:
            g["colsum"] = cs.data[0].double()
            # the bytes and the amax nkb_fp8_quantize makes of the stored rows (x row_scale, the product in fp32), and where its width
            # rule (C % 512 == 0) admits it nkb_fp8_quantize_colsum of the stored rows
            stq, qq = state(), torch.empty(rows, D, dtype=torch.uint8, device=DEV)
            if c.row_scale:
                sel = torch.arange(rows, device=DEV) // c.rps
                hip.fp8_quantize(hip.F32, kind, (dx.data.float() * d.rsc[sel][:, None]).contiguous(), rows * D, stq, qq)
            else:
                hip.fp8_quantize(hip.BF16, kind, dx.data.contiguous(), rows * D, stq, qq)
            assert torch.equal(o[form + ".q"].data, qq) and st[2].item() == stq[2].item(), f"{c.name}: {form} backward fp8 copy"
            if D % 512 == 0:
                stq, qq, col = state(), torch.empty(rows, D, dtype=torch.uint8, device=DEV), torch.zeros(D, device=DEV)
                w2 = torch.empty(hip.fp8_quantize_colsum_workspace(rows, D), device=DEV)
                hip.fp8_quantize_colsum(kind, dx.data.contiguous(), rows, D, D, stq, qq, col, w2, row_scale=d.rsc if c.row_scale else None,
                                        rows_per_sample=c.rps if c.row_scale else 0)
                assert torch.equal(o[form + ".q"].data, qq) and st[2].item() == stq[2].item(), f"{c.name}: {form} backward fp8 copy (fused pass)"
        if c.second == "scaled":
            g["copy"] = o[form + ".copy"].data.double()
        got[form] = g
    atomic = {"atomic.dgamma", "atomic.dbeta"} if tr.ln_bwd_blocks(rows, workspace=False) > 1 else set()
    return o, got, atomic


def _act_launch(c, d):
    dt, hd = tr.TORCH_DT[c.dtype], hip.dt(tr.TORCH_DT[c.dtype])
    n = c.D
    x, dy = _input(d.x), _input(d.dy)
    o = {k: _flat(n, dt) for k in ("y", "dx")}
    if c.op == "relu6":
        hip.relu6(hd, x, None, o["y"].view, n)
        hip.relu6(hd, x, dy, o["dx"].view, n)
        return o, {"": {k: o[k].data.double() for k in o}}, set()
    kind = hip.ACT_KINDS[c.op]
    hip.gelu(hd, x, None, o["y"].view, n, kind)
    hip.gelu(hd, x, dy, o["dx"].view, n, kind)
    o.update({k: _flat(n, dt) for k in ("y2", "gp", "y3")})
    o["inplace"] = _flat(n, dt, d.x)
    hip.gelu_fwd_dgelu(hd, x, o["y2"].view, o["gp"].view, n, kind)
    hip.gelu_fwd_dgelu(hd, o["inplace"].view, o["y3"].view, o["inplace"].view, n, kind)
    assert torch.equal(_raw(o["y3"].data), _raw(o["y2"].data)) and torch.equal(_raw(o["inplace"].data), _raw(o["gp"].data)), f"{c.name}: in place"
    return o, {"": dict(y=o["y"].data.double(), dx=o["dx"].data.double()), "keep": dict(y=o["y2"].data.double(), gp=o["gp"].data.double())}, set()


def _other_launch(c, d):
    dt, hd = tr.TORCH_DT[c.dtype], hip.dt(tr.TORCH_DT[c.dtype])
    rows, D = c.rows, c.D
    o, got, atomic = {}, {}, set()
    if c.kind == "scale":
        o["out"] = Out(rows, D, dt)
        hip.scale_rows(hd, _input(d.x), _input(d.addv) if c.add else None, o["out"].view, _input(d.scale), rows, D)
        got = dict(out=o["out"].data.double())
    elif c.kind == "softmax":
        o["p"], o["ds"] = Out(rows, c.ld, dt), Out(rows, c.ld, dt)
        hip.attn_softmax(hd, False, _input(d.s, c.lds - D), c.lds, None, o["p"].view, c.ld, rows, D, c.scale)
        hip.attn_softmax(hd, True, _input(d.dp, c.lds - D), c.lds, _input(d.p, c.ld - D), o["ds"].view, c.ld, rows, D, c.scale)
        got = dict(p=o["p"].data.double(), ds=o["ds"].data.double())
    elif c.kind == "transpose":
        Z, W = c.outer * c.inner, d.src.shape[2]
        src = _input(d.src.reshape(-1))
        o["out"] = Out(Z * D, c.ld, dt)
        hip.head_transpose(hd, src[max(c.which, 0) * c.inner * D:], W, c.T * W, D, c.outer, c.inner, o["out"].view, c.T, D, c.ld)
        got = dict(out=o["out"].data.reshape(Z, D, c.ld).double())
    elif c.kind == "assemble":
        B, Tn = rows, c.T
        tok = torch.cat([torch.full((c.offset,), tr.GARBAGE, device=DEV).to(dt), _input(d.tok.reshape(-1))])[c.offset:]
        assert tok.data_ptr() % 16 == (2 * c.offset) % 16
        o["x"] = Out(B * Tn, D, dt)
        hip.vit_assemble(hd, False, tok, d.clsv if c.cls else None, d.pos, o["x"].view, B, Tn, D)
        got = dict(x=o["x"].data.reshape(B, Tn, D).double())
        if c.cls:
            o["dtok"] = Out(B * (Tn - 1), D, dt)
            hip.vit_assemble(hd, True, o["dtok"].view, d.clsv, d.pos, _input(d.g.reshape(B * Tn, D)), B, Tn, D)
            got["dtok"] = o["dtok"].data.reshape(B, Tn - 1, D).double()
    elif c.kind == "colsum":
        o["out"] = _vec(D, d.out0)
        ws = None
        if c.form == "work":
            wbuf, ws = _workspace(256 * D)
            o["workspace"] = (wbuf, 256 * D)
        elif tr.colsum_splits(rows) > 1:
            atomic = {"out"}
        hip.colsum2d(hd, _input(d.x, c.ld - D), o["out"].view, rows, D, c.ld, ws)
        got = dict(out=o["out"].data[0].double())
    else:
        n = D
        o["mask"] = _flat(n, torch.uint8, 0xAA, BYTE_SENT)
        for name, src, backward in (("out", d.x, False), ("dx", d.g, True)):
            a = _flat(n, dt, d.addv, tr.GARBAGE) if c.add else None       # (a fresh one: out == add overwrites it)
            if c.alias == "in":
                o[name] = _flat(n, dt, src)
                inp = o[name].view
            elif c.alias == "add":
                o[name], inp = a, _input(src)
            else:
                o[name], inp = _flat(n, dt), _input(src)
            hip.dropout(hd, backward, inp, a.view if c.add else None, o[name].view, o["mask"].view, n, c.p, c.seed)
        got = dict(mask=o["mask"].data != 0, out=o["out"].data.double(), dx=o["dx"].data.double())
        assert bool((o["mask"].data <= 1).all()), "a mask byte that is neither 0 nor 1"
    return o, {"": got}, atomic


def _launch(c, d):
    return _ln_launch(c, d) if c.kind == "ln" else _act_launch(c, d) if c.kind == "act" else _other_launch(c, d)


def _judge(c, d, ref, got, label=""):
    bad = []
    for form, g in got.items():
        for name, (ratio, err, bound) in tr.verdict(c, d, ref, g).items():
            print(f"RATIO {KERNEL[c.kind]} {c.name} {label}{form + '.' if form else ''}{name} err={err:.3e} bound={bound:.3e} ratio={ratio:.3f}")
            if not ratio <= 1.0:
                bad.append(f"{form}.{name}: error {err:.3e} > bound {bound:.3e}")
    return bad


@pytest.mark.parametrize("case", tr.CASES, ids=lambda c: c.name)
def test_kernel_against_float64_reference(case):
    c = case
    d = tr.make(c, DEV, seed=11)
    runs = []
    for _ in range(2):
        runs.append(_launch(c, d))
        torch.cuda.synchronize()
    (a, got, atomic), (b, got2, _) = runs
    for name, v in a.items():
        if name in atomic:
            continue
        x, y = (v.buf, b[name].buf) if isinstance(v, Out) else (v[0], b[name][0])
        assert torch.equal(_raw(x), _raw(y)), f"{c.name}: {name} differs between two launches"
    for name, v in a.items():
        if isinstance(v, Out):
            assert v.intact(), f"{c.name}: {name} wrote outside its region"
        else:
            assert bool((v[0][v[1]:] == SENT).all()), f"{c.name}: {name} written past its {v[1]} advertised floats"
    ref = tr.outputs(c, d, exact=True)
    bad = _judge(c, d, ref, got)
    if atomic:      # the second launch of an atomic form is a result of its own
        bad += _judge(c, d, ref, {k: v for k, v in got2.items() if any(n.startswith(k) for n in atomic) or k == ""}, "second-launch ")
    assert not bad, f"{c.name}: {bad}"


def _sweep32():
    return tr.bf16_sweep().to(DEV)


def test_library_function_error():
    """The basis of A_GELU_FWD, A_GELU_DER and A_EXP: the worst error of the fp32 kernels in ulps of the magnitude of the operand
    terms (transformer_reference's docstring), over every finite bf16 bit pattern with |x| <= 16 and, for the exponent, the softmax
    of (0, a) with a on a uniform grid of 2^16 points in [-88, 0].  Each allowance is at least twice the measured worst."""
    x = _sweep32()
    n = x.numel()
    y, y2, gp = (torch.empty(n, device=DEV) for _ in range(3))
    hip.gelu(hip.F32, x, None, y, n)
    hip.gelu_fwd_dgelu(hip.F32, x, y2, gp, n)
    torch.cuda.synchronize()
    x64 = x.double()
    er = torch.erf(x64 * 0.70710678118654752)
    dens = x64 * 0.3989422804014327 * torch.exp(-0.5 * x64 * x64)
    ref_y, ref_d = x64 * 0.5 * (1 + er), 0.5 * (1 + er) + dens
    m_y, m_d = 0.5 * x64.abs() * (1 + er.abs()), 0.5 * (1 + er.abs()) + dens.abs()
    fwd = ((y.double() - ref_y).abs() / tr.ulp32(m_y)).max().item()
    fwd2 = ((y2.double() - ref_y).abs() / tr.ulp32(m_y)).max().item()
    der = ((gp.double() - ref_d).abs() / tr.ulp32(m_d)).max().item()
    literal = ((y.double() - ref_y).abs() / tr.ulp32(ref_y)).max().item()
    a = torch.linspace(-88.0, 0.0, 1 << 16, device=DEV)
    s = torch.stack([torch.zeros_like(a), a], 1).contiguous()
    p = torch.empty_like(s)
    hip.attn_softmax(hip.F32, False, s, 2, None, p, 2, s.shape[0], 2, 1.0)
    torch.cuda.synchronize()
    ref_p = torch.softmax(s.double(), 1)
    ex = ((p.double() - ref_p).abs() / tr.ulp32(ref_p)).max().item()
    print(f"MEASURED gelu_fwd={max(fwd, fwd2):.3f} gelu_der={der:.3f} exp={ex:.3f} ulps (gelu forward in ulps of |ref| itself: {literal:.3e})")
    assert 2 * max(fwd, fwd2) <= tr.A_GELU_FWD and 2 * der <= tr.A_GELU_DER and 2 * ex <= tr.A_EXP


def test_gelu_refuses_an_unknown_dtype():
    x, out = torch.zeros(8, device=DEV), torch.full((8,), NAN, device=DEV)
    for kind in (hip.ACT_GELU, hip.ACT_QUICK_GELU):
        with pytest.raises(RuntimeError, match="gelu: bad dtype"):
            hip.gelu(7, x, None, out, 8, kind)
    with pytest.raises(RuntimeError, match="unknown activation kind"):
        hip.gelu(hip.F32, x, None, out, 8, 5)
    with pytest.raises(RuntimeError, match="multiple of"):
        hip.gelu(hip.BF16, x, None, out, 12)
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())


def test_zero_extent_calls_return_without_a_launch():
    """rows == 0 (and its kin) is a valid call that does nothing: each entry point returns before its launch, as nkb_scale_rows does
    (decided from the code: an empty grid is a launch error, which would surface here as a RuntimeError).  Negative extents are
    refused."""
    keep = torch.full((64,), 3.0, device=DEV)
    out = keep.clone()
    f = hip.F32
    hip.layernorm_fwd(f, keep, 8, keep, keep, out, 8, out, out, 0, 8, 1e-6)
    hip.layernorm_bwd(f, keep, 8, keep, 8, keep, keep, keep, None, out, 8, out, out, 0, 8)
    hip.attn_softmax(f, False, keep, 8, None, out, 8, 0, 8, 1.0)
    hip.attn_softmax(f, True, keep, 8, keep, out, 8, 0, 8, 1.0)
    hip.head_transpose(f, keep, 8, 64, 8, 0, 1, out, 8, 8, 8)
    hip.head_transpose(f, keep, 8, 64, 8, 1, 0, out, 8, 8, 8)
    hip.vit_assemble(f, False, keep, keep, keep, out, 0, 2, 8)
    hip.vit_assemble(f, True, out, keep, keep, keep, 0, 2, 8)
    hip.colsum2d(f, keep, out, 0, 8, 8)
    hip.colsum2d(f, keep, out, 0, 8, 8, torch.empty(256 * 8, device=DEV))
    hip.scale_rows(f, keep, None, out, keep, 0, 8)
    torch.cuda.synchronize()
    assert torch.equal(out, keep)
    for call in (lambda: hip.layernorm_fwd(f, keep, 8, keep, keep, out, 8, out, out, -1, 8, 1e-6),
                 lambda: hip.attn_softmax(f, False, keep, 8, None, out, 8, -1, 8, 1.0),
                 lambda: hip.head_transpose(f, keep, 8, 64, 8, -1, 1, out, 8, 8, 8),
                 lambda: hip.vit_assemble(f, False, keep, keep, keep, out, -1, 2, 8),
                 lambda: hip.colsum2d(f, keep, out, -1, 8, 8)):
        with pytest.raises(RuntimeError):
            call()
    torch.cuda.synchronize()
    assert torch.equal(out, keep)
