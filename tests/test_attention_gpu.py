"""Every instance of the fused attention kernels (csrc/attention.hip: one per key-block count nkb = ceil(T/16), 1..16) and every
engine attention path against the float64 reference of tests/attn_reference.py, in three input regimes, with guard zones
around every output and finite garbage around every input.

bf16 outputs are held to max(C_BOUND * yardstick error, FLOOR) per (image, head) slice; lse to LSE_RTOL * (1 + |lse|); the fp32
materialised path to FP32_RTOL.  tests/test_attention_reference.py proves on the CPU that these bounds reject subtly wrong
kernels.  Each check prints a "RATIO path output T= err= bound=" line (visible with -rP)."""
import math

import pytest
import torch

import attn_reference as ar

pytestmark = pytest.mark.gpu

from nkb_classification import hip  # noqa: E402

DEV = "cuda"
BF = torch.bfloat16
DH = ar.DH
MARGIN = 256            # guard elements on each side of an output (keeps 16-byte alignment)
GROWS = 3               # garbage rows on each side of an input
GARBAGE = 1e4

assert {(T + 15) // 16 for T in ar.SWEEP} == set(range(1, 17))


def _hold(path, name, x, ref, yard, B, T, H):
    e = ar.rel_err(name, x, ref[name], B, T, H)
    b = ar.bound(ar.rel_err(name, yard[name], ref[name], B, T, H))
    print(f"RATIO {path} {name} T={T} B={B} H={H} err={e:.3e} bound={b:.3e} ratio={e / b:.3f}")
    assert e <= b, f"{path}: {name} at T={T} B={B} H={H}: error {e:.3e} > bound {b:.3e}"


def _hold_lse(path, lse, ref, T, B, H):
    e = ar.lse_err(lse, ref["lse"])
    print(f"RATIO {path} lse T={T} B={B} H={H} err={e:.3e} bound={ar.LSE_RTOL:.1e} ratio={e / ar.LSE_RTOL:.3f}")
    assert e <= ar.LSE_RTOL, f"{path}: lse at T={T}: error {e:.3e}"


def _guarded(shape, dtype):
    """a NaN-filled flat buffer with MARGIN guard elements on each side, and the output view inside it"""
    n = math.prod(shape)
    buf = torch.full((n + 2 * MARGIN,), float("nan"), dtype=dtype, device=DEV)
    return buf, buf[MARGIN:MARGIN + n].view(shape)


def _bits(t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def _nan_bits(dtype):
    return _bits(torch.full((1,), float("nan"), dtype=dtype, device=DEV))


def _margins_intact(buf, what):
    nb = _nan_bits(buf.dtype)
    for part in (buf[:MARGIN], buf[-MARGIN:]):
        assert torch.equal(_bits(part), nb.expand(MARGIN)), f"{what}: a write outside the output"


def _input(x, dtype):
    """x [rows, cols] on the device inside GROWS rows of large finite garbage on each side (reads outside show in the values)"""
    buf = torch.full((x.shape[0] + 2 * GROWS, x.shape[1]), GARBAGE, dtype=dtype, device=DEV)
    buf[GROWS:GROWS + x.shape[0]] = x.to(DEV, dtype)
    return buf[GROWS:GROWS + x.shape[0]]


def _kernel_paths(B, T, H, regime, seed):
    """(a) nkb_attn_forward, (b) nkb_attn_backward, (c) nkb_attn_backward_ds with and without dQ"""
    D = H * DH
    qkv, do = ar.inputs(regime, B, T, H, seed=seed)
    ref = ar.reference(qkv, do, B, T, H)
    yo = ar.yardstick(qkv, do, B, T, H, delta_from="o")
    yp = ar.yardstick(qkv, do, B, T, H, delta_from="p")
    qkv_d, do_d = _input(qkv, BF), _input(do, BF)

    # (a) forward
    obuf, o = _guarded((B * T, D), BF)
    lbuf, lse = _guarded((B * H, T), torch.float32)
    hip.attn_forward(hip.BF16, qkv_d, o, lse, B, T, H, DH, ar.SCALE)
    torch.cuda.synchronize()
    _margins_intact(obuf, "attn_forward o")
    _margins_intact(lbuf, "attn_forward lse")
    _hold("fwd", "o", o.cpu(), ref, yo, B, T, H)
    _hold_lse("fwd", lse.cpu(), ref, T, B, H)
    if regime == "uniform":        # every score 0: exactly T terms of exp(0) in the denominator
        assert (lse.cpu().double() - math.log(T)).abs().max().item() <= ar.LSE_RTOL * (1 + math.log(T))

    # (b) fused backward, twice: with the column sums (onto a non-zero start), then without; bit-identical d_qkv
    o_in, lse_in = _input(o, BF), _input(lse, torch.float32)
    dbuf, dqkv = _guarded((B * T, 3 * D), BF)
    c0 = 0.5
    colsum = torch.full((3 * D,), c0, device=DEV)
    work = torch.empty(B * 3 * D, device=DEV)
    hip.attn_backward(hip.BF16, qkv_d, do_d, o_in, lse_in, dqkv, B, T, H, DH, ar.SCALE, colsum=colsum, colsum_work=work)
    dbuf2, dqkv2 = _guarded((B * T, 3 * D), BF)
    hip.attn_backward(hip.BF16, qkv_d, do_d, o_in, lse_in, dqkv2, B, T, H, DH, ar.SCALE)
    torch.cuda.synchronize()
    _margins_intact(dbuf, "attn_backward dqkv")
    _margins_intact(dbuf2, "attn_backward dqkv (second run)")
    assert torch.equal(_bits(dqkv), _bits(dqkv2)), "attn_backward: not bit-identical on a second run"
    g = dqkv.cpu()
    got = dict(zip(("dq", "dk", "dv"), ar.split_qkv(g, B, T, H)))
    for n in ar.GRADS:
        _hold("bwd", n, got[n], ref, yo, B, T, H)
    cs = colsum.cpu().double() - c0
    torch.testing.assert_close(cs, g.double().sum(0), rtol=1e-5, atol=1e-5 * g.double().abs().max().item() * (B * T) ** 0.5)
    _hold("bwd", "colsum", cs, ref, yo, B, T, H)

    # (c) backward dS, without and with dQ; ldp beyond roundup(T, 16) must keep its sentinel, [T, roundup) must be 0
    T16 = (T + 15) // 16 * 16
    ldp = T16 + 16
    outs = []
    for with_dq in (False, True):
        pbuf, P = _guarded((B * H, T, ldp), BF)
        sbuf, dS = _guarded((B * H, T, ldp), BF)
        qbuf, dq = _guarded((B * T, 3 * D), BF)
        hip.attn_backward_ds(hip.BF16, qkv_d, do_d, lse_in, P, dS, ldp, B, T, H, DH, ar.SCALE,
                             dq=dq if with_dq else None, ld_dq=3 * D if with_dq else 0)
        torch.cuda.synchronize()
        for buf, what in ((pbuf, "P"), (sbuf, "dS"), (qbuf, "dq")):
            _margins_intact(buf, "attn_backward_ds " + what)
        nb = _nan_bits(BF)
        for t, what in ((P, "P"), (dS, "dS")):
            assert torch.equal(_bits(t[:, :, T16:]), nb.expand(B * H, T, ldp - T16)), f"attn_backward_ds {what}: wrote past ldp"
            assert (t[:, :, T:T16].float() == 0).all(), f"attn_backward_ds {what}: columns [T, roundup(T, 16)) not zero"
        Pc, dSc = P[:, :, :T].cpu().double(), dS[:, :, :T].cpu()
        Pr = ref["P"].reshape(B * H, T, T)
        assert ((Pc - Pr).abs() <= 2.0 ** -8 * Pr.abs() + 1e-6).all(), \
            f"attn_backward_ds P: off by more than bf16 rounding, max {(Pc - Pr).abs().max().item():.3e}"
        _hold("ds", "dS", dSc.reshape(B, H, T, T), ref, yp, B, T, H)
        if with_dq:
            q_third = dq[:, :D].cpu()
            assert torch.equal(_bits(dq[:, D:]), nb.expand(B * T, 2 * D)), "attn_backward_ds: wrote outside the Q third"
            _hold("ds", "dq", ar.heads(q_third, B, T, H), ref, yp, B, T, H)
        outs.append((P[:, :, :T16].clone(), dS[:, :, :T16].clone()))
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(*outs)), "attn_backward_ds: P / dS differ with and without dQ"


def _engine(dtype, fused, qkv, do, B, T, H):
    from nkb_classification.hipnet import HipEngine
    from nkb_classification.runtime import ParamArena
    eng = HipEngine(ParamArena(), torch.device(DEV), dtype)
    eng.fused_attention = fused
    o = eng.attention("a", qkv.to(DEV, dtype), B, T, H, True).float().cpu()
    assert eng.saved["a"].get("fused", False) == (fused and dtype == BF and T <= 256)
    g = eng.attention_backward("a", do.to(DEV, dtype), "dqkv").float().cpu()
    torch.cuda.synchronize()
    return dict(o=o, **dict(zip(("dq", "dk", "dv"), ar.split_qkv(g, B, T, H))))


def _engine_paths(B, T, H, regime, seed, monkeypatch, fused=True):
    """(d) HipEngine: the fused path, the fused-dS path (with and without dQ in the dS kernel), the materialised path in bf16
    and fp32"""
    import nkb_classification.hipnet as hipnet
    qkv, do = ar.inputs(regime, B, T, H, seed=seed)
    ref = ar.reference(qkv, do, B, T, H)
    runs = []
    if fused:
        runs.append(("eng.fused", True, True, True, "o"))
        runs += [("eng.ds_dq%d" % dq, True, False, dq, "p") for dq in (True, False)]
    runs.append(("eng.materialised", False, True, True, "pb"))
    for path, fused_attn, fused_bwd, fused_dq, delta_from in runs:
        monkeypatch.setattr(hipnet, "_ATTN_FUSED_BWD", fused_bwd)
        monkeypatch.setattr(hipnet, "_ATTN_FUSED_DQ", fused_dq)
        got = _engine(BF, fused_attn, qkv, do, B, T, H)
        yard = ar.yardstick(qkv, do, B, T, H, delta_from=delta_from)
        for n in ("o",) + ar.GRADS:
            _hold(path, n, got[n], ref, yard, B, T, H)
    monkeypatch.undo()
    got = _engine(torch.float32, False, qkv, do, B, T, H)
    for n in ("o",) + ar.GRADS:
        e = ar.rel_err(n, got[n], ref[n], B, T, H)
        print(f"RATIO eng.fp32 {n} T={T} B={B} H={H} err={e:.3e} bound={ar.FP32_RTOL:.1e} ratio={e / ar.FP32_RTOL:.3f}")
        assert e <= ar.FP32_RTOL, f"fp32 materialised path: {n} at T={T}: error {e:.3e}"


@pytest.mark.parametrize("T", ar.SWEEP)
def test_attention_kernels_every_key_block_count(T, monkeypatch):
    B, H = ar.SWEEP_BH
    for i, regime in enumerate(ar.REGIMES):
        _kernel_paths(B, T, H, regime, seed=100 * T + i)
        _engine_paths(B, T, H, regime, seed=100 * T + i, monkeypatch=monkeypatch)


@pytest.mark.parametrize("geom", [(2, 197, 12), (2, 256, 16), (4, 200, 1)], ids=lambda g: "B%dT%dH%d" % g)
def test_attention_production_geometry(geom, monkeypatch):
    """ViT-B/16 (12 heads in a 2304-wide qkv row), unicom ViT-L/14 (T = 256, 16 heads, 3072 wide), one head"""
    B, T, H = geom
    _kernel_paths(B, T, H, "random", seed=T + H)
    _engine_paths(B, T, H, "random", seed=T + H, monkeypatch=monkeypatch)


@pytest.mark.parametrize("T", [257, 577])
def test_attention_materialised_beyond_fused_range(T, monkeypatch):
    for i, regime in enumerate(ar.REGIMES):
        _engine_paths(2, T, 2, regime, seed=T + i, monkeypatch=monkeypatch, fused=False)


def test_attention_entry_points_reject_what_they_cannot_run():
    B, H = 1, 1
    qkv = torch.zeros(300, 3 * H * DH, device=DEV, dtype=BF)
    do, o = torch.zeros(300, H * DH, device=DEV, dtype=BF), torch.zeros(300, H * DH, device=DEV, dtype=BF)
    lse = torch.zeros(300, device=DEV)
    P = torch.zeros(300 * 320, device=DEV, dtype=BF)
    dqkv = torch.zeros_like(qkv)
    for T, dh, dt in ((0, DH, hip.BF16), (257, DH, hip.BF16), (16, 32, hip.BF16), (16, DH, hip.dt(torch.float32))):
        with pytest.raises(RuntimeError, match="attn_forward"):
            hip.attn_forward(dt, qkv, o, lse, B, T, H, dh, ar.SCALE)
        with pytest.raises(RuntimeError, match="attn_backward"):
            hip.attn_backward(dt, qkv, do, o, lse, dqkv, B, T, H, dh, ar.SCALE)
        with pytest.raises(RuntimeError, match="attn_backward_ds"):
            hip.attn_backward_ds(dt, qkv, do, lse, P, P, 272, B, T, H, dh, ar.SCALE)
    torch.cuda.synchronize()
    assert (qkv == 0).all() and (o == 0).all() and (dqkv == 0).all() and (P == 0).all()
