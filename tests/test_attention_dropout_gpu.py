"""Attention dropout inside the fused attention kernels (csrc/attention.hip, the DROP flavour): the kernels regenerate nkb_dropout's
keep mask from (seed, element index) instead of reading a stored one.

  1, 2  the regenerated mask, read back through the kernels' own outputs, equals nkb_dropout's mask bytes bit for bit (forward,
        and pass B of the backward kernel, which owns the transposed tile);
  3, 4  every kernel instance (one per key-block count) and the production geometries against the float64 reference of
        tests/attn_dropout_reference.py with keep taken from nkb_dropout's bytes, held to attn_reference's bound (proved on the CPU
        by tests/test_attention_dropout_reference.py), with guard zones around every output and garbage around every input;
  5     drop_p == 0 runs today's kernel: bit-identical outputs, whatever the other dropout arguments say;
  6     HipEngine routes active dropout to the fused kernels and keeps no P / Pd / mask; the materialised path (NKB_FUSED_ATTN=0)
        draws the same mask from the same seed;
  7     a whole ViT with backbone dropout trains to bit-identical parameters with launch plans on (C and Python replay) and off,
        and its losses with the fused kernels stay as close to an fp32 run as the materialised bf16 path's do.
Each bound check prints a "RATIO path output T= err= bound=" line (visible with -rP)."""
import math

import pytest
import torch

import attn_dropout_reference as adr
import attn_reference as ar

pytestmark = pytest.mark.gpu

from nkb_classification import hip  # noqa: E402

DEV = "cuda"
BF = torch.bfloat16
DH = ar.DH
MARGIN = 256            # guard elements on each side of an output (keeps 16-byte alignment)
GROWS = 3               # garbage rows on each side of an input
GARBAGE = 1e4


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


def _margins_intact(buf, what):
    nb = _bits(torch.full((1,), float("nan"), dtype=buf.dtype, device=DEV))
    for part in (buf[:MARGIN], buf[-MARGIN:]):
        assert torch.equal(_bits(part), nb.expand(MARGIN)), f"{what}: a write outside the output"


def _input(x, dtype):
    """x [rows, cols] on the device inside GROWS rows of large finite garbage on each side (reads outside show in the values)"""
    buf = torch.full((x.shape[0] + 2 * GROWS, x.shape[1]), GARBAGE, dtype=dtype, device=DEV)
    buf[GROWS:GROWS + x.shape[0]] = x.to(DEV, dtype)
    return buf[GROWS:GROWS + x.shape[0]]


def _seed_buf():
    """the 8-byte seed hand-off buffer inside guard words"""
    buf = torch.full((3,), -1, dtype=torch.int64, device=DEV)
    return buf, buf[1:2]


def _dropout_mask(seed, p, BH, T, ld):
    """the mask bytes nkb_dropout writes for a [BH, T, ld] tensor of ones: uint8 [BH, T, ld]"""
    ones = torch.ones(BH, T, ld, dtype=BF, device=DEV)
    mask = torch.full((BH, T, ld), 7, dtype=torch.uint8, device=DEV)
    hip.dropout(hip.BF16, False, ones, None, torch.empty_like(ones), mask, ones.numel(), p, seed)
    torch.cuda.synchronize()
    assert int(mask.max()) <= 1
    return mask


def _round64(T):
    return (T + 63) // 64 * 64


# ---- 1, 2: mask identity --------------------------------------------------------------------------------------------------------
def _mask_identity_case(T, backward):
    B, H, p, seed = 2, 2, 0.25, 0x1234_5678_9ABC_DEF + T
    D, ld, c = H * DH, _round64(T), 1 / (1 - 0.25)
    want = _dropout_mask(seed, p, B * H, T, ld)[:, :, :T].reshape(B, H, T, T).bool()
    g = torch.Generator().manual_seed(T)
    got = torch.zeros(B, H, T, T, dtype=torch.bool, device=DEV)
    pd = c / T                                            # P = 1 / T in every row (Q = 0), Pd = bf16(P * c) where kept
    for w in range((T + 63) // 64):
        n = min(64, T - 64 * w)
        qkv = ar.bf(torch.randn(B, T, 3, H, DH, generator=g))
        qkv[:, :, 0] = 0
        qkv[:, :, 2] = 0
        do = torch.zeros(B, T, H, DH)
        eye = torch.eye(n)[None, :, None, :].expand(B, n, H, n)
        if backward:
            do[:, 64 * w:64 * w + n, :, :n] = eye       # dO[q][q - 64 w] = 1, V = 0: dV[k][q - 64 w] = Pd[q][k]
        else:
            qkv[:, 64 * w:64 * w + n, 2, :, :n] = eye   # V[k][k - 64 w] = 1: O[q][k - 64 w] = Pd[q][k]
        qkv_d, do_d = _input(qkv.reshape(B * T, 3 * D), BF), _input(do.reshape(B * T, D), BF)
        obuf, o = _guarded((B * T, D), BF)
        lbuf, lse = _guarded((B * H, T), torch.float32)
        sbuf, sd = _seed_buf()
        hip.attn_forward(hip.BF16, qkv_d, o, lse, B, T, H, DH, ar.SCALE, drop_p=p, seed=seed, drop_ld=ld, seed_out=sd)
        torch.cuda.synchronize()
        assert sbuf.tolist() == [-1, seed, -1], "seed_out does not hold the seed (or its neighbours were written)"
        _margins_intact(obuf, "attn_forward o")
        _margins_intact(lbuf, "attn_forward lse")
        assert (lse.double() - math.log(T)).abs().max().item() <= ar.LSE_RTOL * (1 + math.log(T)), "lse must be that of the undropped scores"
        if backward:
            assert (o.float() == 0).all()
            dbuf, dqkv = _guarded((B * T, 3 * D), BF)
            hip.attn_backward(hip.BF16, qkv_d, do_d, _input(o, BF), _input(lse, torch.float32), dqkv, B, T, H, DH, ar.SCALE,
                              drop_p=p, seed_dev=sd, drop_ld=ld)
            torch.cuda.synchronize()
            _margins_intact(dbuf, "attn_backward dqkv")
            vals = dqkv.reshape(B, T, 3, H, DH)[:, :, 2, :, :n].float().permute(0, 2, 3, 1)     # [b, h, q - 64 w, k]
        else:
            vals = o.reshape(B, T, H, DH)[:, :, :, :n].float().permute(0, 2, 1, 3)              # [b, h, q, k - 64 w]
        nz = vals != 0
        assert ((vals[nz] - pd).abs() <= 2.0 ** -8 * pd).all(), "a kept element is not bf16(P / (1 - p))"
        if backward:
            got[:, :, 64 * w:64 * w + n, :] = nz
        else:
            got[:, :, :, 64 * w:64 * w + n] = nz
    assert torch.equal(got, want), f"{(got != want).sum().item()} of {want.numel()} keep decisions differ from nkb_dropout's mask"
    n_el, frac = want.numel(), want.float().mean().item()
    sigma = math.sqrt(p * (1 - p) / n_el)
    print(f"KEEP T={T} fraction={frac:.5f} expected={1 - p} sigma={sigma:.2e} z={(frac - (1 - p)) / sigma:.2f}")
    assert abs(frac - (1 - p)) <= 5 * sigma


@pytest.mark.parametrize("T", [48, 197, 256])
def test_forward_regenerates_nkb_dropouts_mask(T):
    _mask_identity_case(T, backward=False)


@pytest.mark.parametrize("T", [48, 197, 256])
def test_backward_pass_b_regenerates_nkb_dropouts_mask(T):
    _mask_identity_case(T, backward=True)


# ---- 3, 4: against the float64 reference ----------------------------------------------------------------------------------------
def _against_reference(B, T, H, regime, p, seed):
    D, ld = H * DH, _round64(T)
    rng_seed = 0x0BAD_5EED_0000_0000 + seed
    qkv, do = ar.inputs(regime, B, T, H, seed=seed)
    keep = _dropout_mask(rng_seed, p, B * H, T, ld)[:, :, :T].reshape(B, H, T, T).bool().cpu()
    ref = adr.reference(qkv, do, keep, p, B, T, H)
    yard = adr.yardstick(qkv, do, keep, p, B, T, H)
    plain = ar.reference(qkv, do, B, T, H)
    qkv_d, do_d = _input(qkv, BF), _input(do, BF)
    path = "drop%g" % p

    obuf, o = _guarded((B * T, D), BF)
    lbuf, lse = _guarded((B * H, T), torch.float32)
    sbuf, sd = _seed_buf()
    hip.attn_forward(hip.BF16, qkv_d, o, lse, B, T, H, DH, ar.SCALE, drop_p=p, seed=rng_seed, drop_ld=ld, seed_out=sd)
    torch.cuda.synchronize()
    _margins_intact(obuf, "attn_forward o")
    _margins_intact(lbuf, "attn_forward lse")
    assert sbuf.tolist() == [-1, rng_seed, -1]
    _hold(path + ".fwd", "o", o.cpu(), ref, yard, B, T, H)
    _hold_lse(path + ".fwd", lse.cpu(), plain, T, B, H)

    o_in, lse_in = _input(o, BF), _input(lse, torch.float32)
    dbuf, dqkv = _guarded((B * T, 3 * D), BF)
    c0 = 0.5
    colsum = torch.full((3 * D,), c0, device=DEV)
    work = torch.empty(B * 3 * D, device=DEV)
    hip.attn_backward(hip.BF16, qkv_d, do_d, o_in, lse_in, dqkv, B, T, H, DH, ar.SCALE, colsum=colsum, colsum_work=work,
                      drop_p=p, seed_dev=sd, drop_ld=ld)
    dbuf2, dqkv2 = _guarded((B * T, 3 * D), BF)
    hip.attn_backward(hip.BF16, qkv_d, do_d, o_in, lse_in, dqkv2, B, T, H, DH, ar.SCALE, drop_p=p, seed_dev=sd, drop_ld=ld)
    torch.cuda.synchronize()
    _margins_intact(dbuf, "attn_backward dqkv")
    _margins_intact(dbuf2, "attn_backward dqkv (second run)")
    assert sbuf.tolist() == [-1, rng_seed, -1]
    assert torch.equal(_bits(dqkv), _bits(dqkv2)), "attn_backward: not bit-identical on a second run"
    g = dqkv.cpu()
    got = dict(zip(("dq", "dk", "dv"), ar.split_qkv(g, B, T, H)))
    for n in ar.GRADS:
        _hold(path + ".bwd", n, got[n], ref, yard, B, T, H)
    cs = colsum.cpu().double() - c0
    torch.testing.assert_close(cs, g.double().sum(0), rtol=1e-5, atol=1e-5 * max(g.double().abs().max().item(), 1e-3) * (B * T) ** 0.5)


@pytest.mark.parametrize("T", ar.SWEEP)
def test_dropout_kernels_every_key_block_count(T):
    B, H = ar.SWEEP_BH
    _against_reference(B, T, H, ar.REGIMES[ar.SWEEP.index(T) % 3], 0.25, seed=100 * T)
    if T == 197:
        for p in (0.1, 0.5):
            _against_reference(B, T, H, "random", p, seed=100 * T + int(10 * p))


@pytest.mark.parametrize("geom", [(2, 197, 12), (2, 256, 16)], ids=lambda g: "B%dT%dH%d" % g)
def test_dropout_kernels_production_geometry(geom):
    B, T, H = geom
    _against_reference(B, T, H, "random", 0.1, seed=T + H)


# ---- 5: p = 0 -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [48, 197])
def test_zero_drop_p_is_the_kernel_without_dropout(T):
    B, H = 2, 2
    D = H * DH
    qkv, do = ar.inputs("random", B, T, H, seed=T)
    qkv_d, do_d = qkv.to(DEV, BF), do.to(DEV, BF)
    outs = []
    for kw_f, kw_b in (({}, {}), (dict(drop_p=0.0, seed=987654321987, drop_ld=3, seed_out=None), dict(drop_p=0.0, seed_dev=None, drop_ld=-5))):
        o = torch.full((B * T, D), float("nan"), dtype=BF, device=DEV)
        lse = torch.full((B * H, T), float("nan"), device=DEV)
        dqkv = torch.full((B * T, 3 * D), float("nan"), dtype=BF, device=DEV)
        hip.attn_forward(hip.BF16, qkv_d, o, lse, B, T, H, DH, ar.SCALE, **kw_f)
        hip.attn_backward(hip.BF16, qkv_d, do_d, o, lse, dqkv, B, T, H, DH, ar.SCALE, **kw_b)
        torch.cuda.synchronize()
        outs.append((o, lse, dqkv))
    for a, b in zip(*outs):
        assert torch.equal(_bits(a), _bits(b))


# ---- 6: engine routing and memory -----------------------------------------------------------------------------------------------
def test_engine_keeps_active_dropout_on_the_fused_kernels():
    from nkb_classification.hipnet import HipEngine
    from nkb_classification.runtime import ParamArena
    B, T, H, p = 2, 197, 2, 0.25
    qkv, do = ar.inputs("random", B, T, H, seed=11)
    res = {}
    for fused in (True, False):
        eng = HipEngine(ParamArena(), torch.device(DEV), BF)
        eng.fused_attention = fused
        torch.manual_seed(5)
        o = eng.attention("a", qkv.to(DEV, BF), B, T, H, True, drop_p=p).float().cpu()
        sv = eng.saved["a"]
        if fused:
            assert sv.get("fused") and sv["p"] == p and sv["drop_ld"] == _round64(T) and sv["seed"].numel() == 1
            assert "a.drop" not in eng.saved and not any(k in sv for k in ("P", "Pd", "mask"))
            assert "a.P" not in eng.ws._bufs and "a.drop.mask" not in eng.ws._bufs and "a.drop.y" not in eng.ws._bufs
            assert "a.seed" in eng.ws._bufs
        else:
            assert not sv.get("fused") and "mask" in eng.saved["a.drop"]      # the materialised path saves a mask as before
            keep = eng.saved["a.drop"]["mask"][:, :, :T].reshape(B, H, T, T).bool().cpu()
        g = eng.attention_backward("a", do.to(DEV, BF), "dqkv").float().cpu()
        torch.cuda.synchronize()
        res[fused] = dict(o=o, **dict(zip(("dq", "dk", "dv"), ar.split_qkv(g, B, T, H))))
    ref = adr.reference(qkv, do, keep, p, B, T, H)
    for fused, path in ((True, "fused"), (False, "materialised")):
        yard = adr.yardstick(qkv, do, keep, p, B, T, H, path=path)
        for n in ("o",) + ar.GRADS:
            _hold("eng." + path, n, res[fused][n], ref, yard, B, T, H)
    # eval mode and p = 0 take the kernel without dropout and save nothing for it
    eng = HipEngine(ParamArena(), torch.device(DEV), BF)
    eng.attention("e", qkv.to(DEV, BF), B, T, H, False, drop_p=p)
    assert "e" not in eng.saved and "e.seed" not in eng.ws._bufs
    eng.attention("z", qkv.to(DEV, BF), B, T, H, True, drop_p=0.0)
    assert eng.saved["z"].get("fused") and "p" not in eng.saved["z"] and "z.seed" not in eng.ws._bufs


def test_engine_with_the_split_backward_keeps_dropout_materialised(monkeypatch):
    import nkb_classification.hipnet as hipnet
    from nkb_classification.hipnet import HipEngine
    from nkb_classification.runtime import ParamArena
    monkeypatch.setattr(hipnet, "_ATTN_FUSED_BWD", False)
    eng = HipEngine(ParamArena(), torch.device(DEV), BF)
    qkv, _ = ar.inputs("random", 1, 17, 2, seed=1)
    eng.attention("a", qkv.to(DEV, BF), 1, 17, 2, True, drop_p=0.25)
    assert not eng.saved["a"].get("fused") and "a.drop" in eng.saved


# ---- 7: whole model -------------------------------------------------------------------------------------------------------------
def test_vit_with_backbone_dropout_plans_and_fused_against_materialised(monkeypatch):
    """vit_tiny_test (17 tokens, 2 heads of 64) in bf16 with backbone_dropout = 0.25: full batches (eager steps, then replayed plans), an
    evaluation pass in between, a partial batch.  (a) parameters bit-identical with plans on (C replay, Python replay) and off: the
    seed reaches the backward plan through device memory, one host draw per site and step.  (b) NKB_FUSED_ATTN on against off from
    the same seeds: both draw the same masks, so their per-step losses differ by bf16 rounding only.  Truth: the same schedule in fp32,
    eager, whose attention masks are drawn at the bf16 pitch (the fp32 engine pads P to 32 columns, the bf16 engine to 64; every other
    dropout site indexes a flat tensor and needs no help).  The fused run may deviate (relative, worst step) 1.25 x as far from it as
    the materialised run, + 5e-3 — the margin tests/test_parity_bench_size_gpu.py uses between two bf16 implementations."""
    from nkb_classification import model as model_mod
    from nkb_classification.hipnet import HipEngine
    from nkb_classification.losses import get_loss
    from nkb_classification.model import get_model
    from nkb_classification.utils import get_optimizer
    dev = "cuda:0"
    cfg_model = dict(model="vit_tiny_test", pretrained=False, backbone_dropout=0.25, classifier_dropout=0.0,
                     classifier_initialization="kaiming_normal_", task="single")
    crit = get_loss(dict(task="single", type="CrossEntropyLoss"), dev)
    g = torch.Generator().manual_seed(12)
    xs = [torch.randn(8, 3, 64, 64, generator=g).to(dev) for _ in range(3)] + [torch.randn(5, 3, 64, 64, generator=g).to(dev)]
    ys = [torch.randint(0, 3, (x.shape[0],), generator=g).to(dev) for x in xs]
    schedule = [0, 1, 2, 0, 1, 3, "eval", 2, 0, 1, 2, 3, 3, 0]

    def run(plans_on, c_replay=True, fused=True, dtype=BF):
        monkeypatch.setattr(model_mod, "_PLANS", plans_on)
        monkeypatch.setattr(hip, "_PLAN_C", c_replay)
        monkeypatch.setenv("NKB_FUSED_ATTN", "1" if fused else "0")
        torch.manual_seed(0)
        model = get_model(dict(cfg_model), ["a", "b", "c"], dev)
        opt = get_optimizer(model, dict(type="nadam", lr=1e-3, weight_decay=0.01))
        torch.manual_seed(77)                        # dropout seed stream
        model.train()
        losses = []
        for item in schedule:
            if item == "eval":
                model.eval()
                with torch.no_grad():
                    model(xs[0])
                model.train()
                continue
            opt.zero_grad()
            with torch.autocast("cuda", dtype=BF, enabled=dtype == BF):
                loss = crit(model(xs[item]), ys[item])
            loss.backward()
            opt.step()
            losses.append(loss.item())
        torch.cuda.synchronize()
        eng = model._engines[dtype]
        assert eng.fused_attention == fused
        sites = [k for k in eng.saved if k.endswith(".attn")]
        assert len(sites) == 2
        for k in sites:
            assert bool(eng.saved[k].get("fused")) == (fused and dtype == BF)
            assert ((k + ".drop") in eng.saved) == (not (fused and dtype == BF))
        return model.arena.flat_param.clone(), len(eng.plans), losses

    p_on, n_on, l_fused = run(True)
    p_py, n_py, _ = run(True, c_replay=False)
    p_off, n_off, l_off = run(False)
    assert n_off == 0 and n_on >= 2 and n_py == n_on
    assert torch.equal(p_on, p_off) and torch.equal(p_py, p_off)
    assert l_fused == l_off

    _, _, l_mat = run(True, fused=False)

    orig = HipEngine.dropout

    def dropout_at_bf16_pitch(self, key, x, p, train, add=None):
        if not (key.endswith(".attn.drop") and train and p > 0):
            return orig(self, key, x, p, train, add)
        BH, T, Tp = x.shape
        ld = _round64(T)
        assert Tp <= ld and add is None
        wide = torch.empty(BH, T, ld, dtype=torch.uint8, device=x.device)
        ones = torch.ones(BH, T, ld, dtype=x.dtype, device=x.device)
        hip.dropout(hip.dt(x.dtype), False, ones, None, torch.empty_like(ones), wide, ones.numel(), p, hip.fresh_seed())
        mask = self.ws.get(key + ".mask", x.shape, torch.uint8)
        mask.copy_(wide[:, :, :Tp])
        y = self.ws.get(key + ".y", x.shape, x.dtype)
        hip.dropout(hip.dt(x.dtype), True, x, None, y, mask, x.numel(), p, 0)
        self.saved[key] = dict(mask=mask, p=p)
        return y

    monkeypatch.setattr(HipEngine, "dropout", dropout_at_bf16_pitch)
    _, _, l_true = run(False, fused=False, dtype=torch.float32)
    monkeypatch.setattr(HipEngine, "dropout", orig)

    dev_f = max(abs(a - t) / abs(t) for a, t in zip(l_fused, l_true))
    dev_m = max(abs(a - t) / abs(t) for a, t in zip(l_mat, l_true))
    bar = 1.25 * dev_m + 5e-3
    print(f"RATIO vit_tiny_test losses fused-vs-fp32 {dev_f:.3e} materialised-vs-fp32 {dev_m:.3e} bar {bar:.3e} ratio={dev_f / bar:.3f}")
    assert all(math.isfinite(v) for v in l_fused + l_mat + l_true)
    assert dev_f <= bar, (l_fused, l_mat, l_true)
