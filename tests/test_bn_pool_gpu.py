"""nkb_bn_finalize, nkb_bn_apply, nkb_bn_backward, nkb_bn_backward_from_stats, nkb_maxpool3x3s2 and the global-average modes of
nkb_avgpool (csrc/elementwise.hip) against the float64 reference of tests/bn_reference.py, at the smallest shapes at which each
path of their loops and dispatch can go wrong: one and several trips of the two-rows-per-trip loops with a ragged last one, chunk
counts that do not divide 256, the block caps, every walk length of the block-partial finalize, the 128 / 129 tile boundary, the
two-launch form past 32 channel columns and the wrap of the ticket ring.

Outputs sit inside guard rows holding a finite sentinel that must come back unchanged; output regions start as NaN; rows past the
end of every input hold finite garbage (1e4), bit-array padding 0xFF; workspaces have exactly the advertised size plus a sentinel
tail.  Every case is held to the derived bounds of bn_reference (exact cases value for value), is bit-identical on a second launch
and prints "RATIO kernel case output err= bound= ratio=" for its worst element (visible with -rP).  tests/test_bn_reference.py
proves on the CPU that these checks reject subtly wrong kernels."""
import pytest
import torch

import bn_reference as br

pytestmark = pytest.mark.gpu

from nkb_classification import hip  # noqa: E402

DEV = "cuda"
G = 4                   # guard rows on each side of an output
GR = 3                  # garbage rows past the end of an input
SENT = -8192.0          # bf16 / fp32-exact sentinel of the guard zones
BYTE_SENT = 0x5A
TAIL = 64               # sentinel floats behind a workspace
NAN = float("nan")
KERNEL = dict(apply="nkb_bn_apply", bwd="nkb_bn_backward", fin="nkb_bn_finalize", fs="nkb_bn_backward_from_stats",
              maxpool="nkb_maxpool3x3s2", avgpool="nkb_avgpool")


class Out:
    """[G + rows + G][cols]: the guards hold `sent`, the region between them `fill` (a value or a [rows][cols] tensor)"""

    def __init__(self, rows, cols, dtype, fill=NAN, sent=SENT):
        self.rows = rows
        self.guard = torch.full((1,), sent, device=DEV, dtype=dtype)
        self.buf = torch.full((G + rows + G, cols), sent, device=DEV, dtype=dtype)
        self.buf[G:G + rows] = fill
        self.view = self.buf[G:]
        self.data = self.buf[G:G + rows]

    def intact(self):
        return bool((self.buf[:G] == self.guard).all()) and bool((self.buf[G + self.rows:] == self.guard).all())


def _vec(C, fill=NAN):
    return Out(1, C, torch.float32, fill)


def _input(t, garbage=br.GARBAGE):
    """t [rows][C] followed by GR rows of finite garbage"""
    t = t.reshape(-1, t.shape[-1])
    return torch.cat([t, torch.full((GR, t.shape[1]), garbage, device=DEV).to(t.dtype)])


def _bits_input(mask, dtype):
    b = br.pack_bits(mask, dtype, mask.shape[1])
    return torch.cat([b, torch.full((GR, b.shape[1]), 0xFF, dtype=torch.uint8, device=DEV)])


def _workspace(advertised, head=None):
    """exactly the advertised floats (head: the input block at their start, the rest NaN) plus a sentinel tail; (buffer, view)"""
    buf = torch.full((advertised + TAIL,), SENT, device=DEV)
    buf[:advertised] = NAN
    if head is not None:
        buf[:head.numel()] = head.reshape(-1)
    return buf, buf[:advertised]


def _raw(t):
    return t.view(torch.uint8) if t.dtype.itemsize == 1 else t.view(torch.int16) if t.dtype.itemsize == 2 else t.view(torch.int32)


def _launch(c, d):
    """one launch (the pools: forward, then backward); ({name: Out | (buffer, advertised)}, got)"""
    dt, hd = br.TORCH_DT[c.dtype], hip.dt(br.TORCH_DT[c.dtype])
    rows, C = c.rows, c.C
    cpr = C // br.chunk(c.dtype)
    o, got = {}, {}
    if c.kind == "apply":
        o["y"] = Out(rows, C, dt)
        if c.bits:
            o["bits"] = Out(rows, cpr, torch.uint8, 0xAA, BYTE_SENT)
        hip.bn_apply(hd, _input(d.x), _input(d.res) if d.res is not None else None, o["y"].view, d.scale, d.shift, rows, C, c.relu,
                     relu_bits=o["bits"].view if c.bits else None, res_scale=d.res_scale, res_shift=d.res_shift)
        got["y"] = o["y"].data.double()
        if c.bits:
            got["bits"] = br.unpack_bits(o["bits"].data, c.dtype, C)
    elif c.kind == "bwd":
        inplace = c.dym == "inplace"
        o["dgamma"], o["dbeta"] = _vec(C, d.dgamma0), _vec(C, d.dbeta0)
        if inplace:
            o["dy"] = Out(rows, C, dt, d.dy, br.GARBAGE)
            dy = o["dy"].view
        else:
            dy = _input(d.dy)
        if c.dx:
            o["dx"] = Out(rows, C, dt)
        if c.dym == "sep":
            o["dym"] = Out(rows, C, dt)
        adv = hip.bn_backward_ws(rows, C)
        assert adv == br.bwd_ws_floats(rows, C)
        wbuf, ws = _workspace(adv)
        o["workspace"] = (wbuf, adv)
        hip.bn_backward(hd, dy, _input(d.x), _input(d.yact) if c.mask == "yact" else None, d.mean, d.invstd, d.gamma, rows, C,
                        o["dgamma"].view, o["dbeta"].view, o["dx"].view if c.dx else None,
                        dy if inplace else o["dym"].view if c.dym == "sep" else None, ws,
                        fscale=d.fscale if c.mask == "fmask" else None, fshift=d.fshift if c.mask == "fmask" else None,
                        relu_bits=_bits_input(d.bitmask, c.dtype) if c.mask == "bits" else None)
        blocks = br.bwd_geometry(rows, C, c.dtype)[3]
        got["sums"] = ws[blocks * 2 * C:blocks * 2 * C + 2 * C].reshape(2, C).double()
        got["dgamma"], got["dbeta"] = o["dgamma"].data[0].double(), o["dbeta"].data[0].double()
        if c.dx:
            got["dx"] = o["dx"].data.double()
            if c.dym != "none":
                got["dym"] = (o["dy"] if inplace else o["dym"]).data.double()
        else:       # no second kernel: nothing but the sums and the parameter gradients is written
            if inplace:
                assert torch.equal(_raw(o["dy"].data), _raw(d.dy)), "dy changed although dx == NULL"
            if c.dym == "sep":
                assert bool(torch.isnan(o["dym"].data).all()), "dy_masked written although dx == NULL"
    elif c.kind == "fs":
        adv = hip.bn_stats_floats(c.tiles, C)
        assert adv == br.stats_floats(c.tiles, C)
        sbuf, st = _workspace(adv, d.stats)
        o["stats"] = (sbuf, adv)
        o["dgamma"], o["dbeta"], o["sums"], o["dx"] = _vec(C, d.dgamma0), _vec(C, d.dbeta0), _vec(2 * C), Out(rows, C, dt)
        hip.bn_backward_from_stats(hd, _input(d.dy), _input(d.x), st, c.tiles, d.mean, d.invstd, d.gamma, rows, C, o["dgamma"].view,
                                   o["dbeta"].view, o["dx"].view, o["sums"].view)
        assert torch.equal(st[:d.stats.numel()], d.stats.reshape(-1)), "the tile sums are an input"
        got = dict(sums=o["sums"].data.reshape(2, C).double(), dgamma=o["dgamma"].data[0].double(), dbeta=o["dbeta"].data[0].double(),
                   dx=o["dx"].data.double())
    elif c.kind == "fin":
        adv = hip.bn_stats_floats(c.tiles, C)
        assert adv == br.stats_floats(c.tiles, C)
        sbuf, st = _workspace(adv, d.partials)
        o["stats"] = (sbuf, adv)
        o["running_mean"], o["running_var"] = _vec(C, d.rm), _vec(C, d.rv)
        for k in ("scale", "shift", "mean", "invstd"):
            o[k] = _vec(C)
        hip.bn_finalize(st, c.tiles, C, c.count, d.gamma, d.beta, o["running_mean"].view, o["running_var"].view, d.momentum, d.eps,
                        c.training, o["scale"].view, o["shift"].view, o["mean"].view, o["invstd"].view)
        assert torch.equal(st[:d.partials.numel()], d.partials.reshape(-1)), "the partial sums are an input"
        if c.training:
            got = {k: o[k].data[0].double() for k in ("scale", "shift", "mean", "invstd", "running_mean", "running_var")}
        else:
            got = {k: o[k].data[0].double() for k in ("scale", "shift")}
            assert torch.equal(o["running_mean"].data[0], d.rm) and torch.equal(o["running_var"].data[0], d.rv), "eval mode wrote running statistics"
            assert bool(torch.isnan(o["mean"].data).all()) and bool(torch.isnan(o["invstd"].data).all()), "eval mode wrote mean / invstd"
    elif c.kind == "maxpool":
        N, H, W = c.N, c.H, c.W
        P, Q = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        o["y"], o["idx"] = Out(N * P * Q, C, dt), Out(N * P * Q, C, torch.uint8, 0xAA, BYTE_SENT)
        o["dx"] = Out(N * H * W, C, dt)
        hip.maxpool(hd, False, _input(d.x), o["y"].view, o["idx"].view, N, H, W, C)
        hip.maxpool(hd, True, _input(d.g), o["dx"].view, o["idx"].view, N, H, W, C)
        got = dict(y=o["y"].data.reshape(N, P, Q, C).double(), idx=o["idx"].data.reshape(N, P, Q, C).long(),
                   dx=o["dx"].data.reshape(N, H, W, C).double())
    else:
        N, HW = c.N, c.H
        o["y"], o["dx"] = Out(N, C, dt), Out(N * HW, C, dt)
        hip.avgpool(hd, False, _input(d.x), o["y"].view, N, HW, C)
        hip.avgpool(hd, True, _input(d.g), o["dx"].view, N, HW, C)
        got = dict(y=o["y"].data.double(), dx=o["dx"].data.reshape(N, HW, C).double())
    return o, got


def _check_guards(c, o):
    for name, v in o.items():
        if isinstance(v, Out):
            assert v.intact(), f"{c.name}: {name} wrote outside its rows"
        else:
            buf, adv = v
            assert bool((buf[adv:] == SENT).all()), f"{c.name}: {name} written past its {adv} advertised floats"


@pytest.mark.parametrize("case", br.CASES, ids=lambda c: c.name)
def test_kernel_against_float64_reference(case):
    c = case
    d = br.make(c, DEV, seed=11)
    runs = []
    for _ in range(2):
        runs.append(_launch(c, d))
        torch.cuda.synchronize()
    (a, got), (b, _) = runs
    for name, v in a.items():
        x, y = (v.buf, b[name].buf) if isinstance(v, Out) else (v[0], b[name][0])
        assert torch.equal(_raw(x), _raw(y)), f"{c.name}: {name} differs between two launches"
    _check_guards(c, a)
    ref = br.outputs(c, d, exact=True)
    v = br.verdict(c, d, ref, got)
    for name, (ratio, err, bound) in v.items():
        print(f"RATIO {KERNEL[c.kind]} {c.name} {name} err={err:.3e} bound={bound:.3e} ratio={ratio:.3f}")
    assert br.mask_share(c, ref) <= br.MASK_SHARE
    for name, (ratio, err, bound) in v.items():
        assert ratio <= 1.0, f"{c.name}: {name} error {err:.3e} > bound {bound:.3e}"


RING_CALLS = 300


@pytest.mark.parametrize("kind", ["fin", "fs"])
def test_ticket_ring_wraps(kind):
    """300 consecutive one-launch reductions at (tiles, C) = (129, 64), alternating three inputs: the 128-slot ticket ring wraps
    twice, and every call is compared with the reference of its input"""
    tiles, C = 129, 64
    cases = [br.Case(kind, f"ring-{kind}-{i}", "f32", 53 if kind == "fs" else 0, C, False, tiles=tiles, count=tiles * 4) for i in range(3)]
    data = [br.make(c, DEV, seed=11) for c in cases]
    adv = hip.bn_stats_floats(tiles, C)
    stats = [_workspace(adv, d.stats if kind == "fs" else d.partials) for d in data]
    n = RING_CALLS
    pre = lambda k: torch.stack([getattr(data[i % 3], k) for i in range(n)])
    if kind == "fin":
        names = ("scale", "shift", "mean", "invstd", "running_mean", "running_var")
        outs = {k: Out(n, C, torch.float32) for k in names[:4]}
        outs["running_mean"], outs["running_var"] = Out(n, C, torch.float32, pre("rm")), Out(n, C, torch.float32, pre("rv"))
        for i in range(n):
            d, o = data[i % 3], {k: outs[k].data[i] for k in names}
            hip.bn_finalize(stats[i % 3][1], tiles, C, cases[0].count, d.gamma, d.beta, o["running_mean"], o["running_var"], d.momentum,
                            d.eps, True, o["scale"], o["shift"], o["mean"], o["invstd"])
    else:
        names = ("sums", "dgamma", "dbeta", "dx")
        hd = hip.dt(torch.float32)
        outs = dict(sums=Out(n, 2 * C, torch.float32), dgamma=Out(n, C, torch.float32, pre("dgamma0")),
                    dbeta=Out(n, C, torch.float32, pre("dbeta0")), dx=Out(n * 53, C, torch.float32))
        xs, gs = [_input(d.x) for d in data], [_input(d.dy) for d in data]
        for i in range(n):
            d = data[i % 3]
            hip.bn_backward_from_stats(hd, gs[i % 3], xs[i % 3], stats[i % 3][1], tiles, d.mean, d.invstd, d.gamma, 53, C,
                                       outs["dgamma"].data[i], outs["dbeta"].data[i], outs["dx"].data[i * 53:], outs["sums"].data[i])
    torch.cuda.synchronize()
    for k, o in outs.items():
        assert o.intact(), k
    for buf, _ in stats:
        assert bool((buf[adv:] == SENT).all())
    refs = [br.outputs(c, d, exact=True) for c, d in zip(cases, data)]
    worst = {}
    for i in range(n):
        if kind == "fin":
            got = {k: outs[k].data[i].double() for k in names}
        else:
            got = dict(sums=outs["sums"].data[i].reshape(2, C).double(), dgamma=outs["dgamma"].data[i].double(),
                       dbeta=outs["dbeta"].data[i].double(), dx=outs["dx"].data[i * 53:(i + 1) * 53].double())
        if i >= 3:
            for k in got:
                first = outs[k].data[(i % 3) * 53:(i % 3 + 1) * 53] if k == "dx" else outs[k].data[i % 3]
                mine = outs[k].data[i * 53:(i + 1) * 53] if k == "dx" else outs[k].data[i]
                assert torch.equal(_raw(mine), _raw(first)), f"call {i}: {k} differs from call {i % 3} on the same input"
            continue
        for k, (ratio, err, bound) in br.verdict(cases[i % 3], data[i % 3], refs[i % 3], got).items():
            if ratio >= worst.get(k, (-1.0,))[0]:
                worst[k] = (ratio, err, bound, i)
    for k, (ratio, err, bound, i) in worst.items():
        print(f"RATIO {KERNEL[kind]} ring-call-{i} {k} err={err:.3e} bound={bound:.3e} ratio={ratio:.3f}")
    assert all(r[0] <= 1.0 for r in worst.values()), worst
