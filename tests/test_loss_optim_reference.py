"""CPU proof that tests/test_loss_optim_gpu.py can fail: the float64 loss reference of tests/loss_optim_reference.py equals
F.cross_entropy(weight, ignore_index) and a literal float64 transcription of the focal formula under torch autograd wherever the
two contracts agree, and every documented divergence holds as documented; the float64 optimizer reference equals
torch.optim.{Adam, AdamW, NAdam, RAdam, SGD} run in float64 for eight steps; the fp32 yardstick lies inside every bound in two
summation orders; exact cases are representable; every mutant of the yardstick is rejected by the outputs REJECTED_BY names and by
no other; no case leaves an element out of a check."""
import pytest
import torch
import torch.nn.functional as F

import loss_optim_reference as lo

_CACHE = {}
SMALL = [c for c in lo.CASES if not c.big]
UNMEASURED = lo.A_LOG != lo.A_LOG or lo.A_POW != lo.A_POW


def _setup(case):
    """(operands, reference, yardstick) of a case, computed once and left unchanged"""
    if case.name not in _CACHE:
        d = lo.make(case, seed=7)
        _CACHE[case.name] = (d, lo.outputs(case, d, exact=True), lo.outputs(case, d, exact=False))
    return _CACHE[case.name]


def _close(a, b, tol=1e-11):
    a, b = a.double(), b.double()
    scale = max(b.abs().max().item(), 1.0) if b.numel() else 1.0
    return a.shape == b.shape and (a.numel() == 0 or (a - b).abs().max().item() <= tol * scale)


def test_allowances_are_measured():
    """the loss-value checks fail closed until logf and powf are measured on the GPU"""
    assert not UNMEASURED, "A_LOG / A_POW are unmeasured: run test_loss_optim_gpu.py::test_library_function_error on an MI355X"
    assert lo.A_LOG >= 2 * lo.MEASURED["log"] and lo.A_POW >= 2 * max(lo.MEASURED["pow"], lo.MEASURED["pow_m1"])


FINITE = ("random", "offset", "spread", "equal", "ties")


@pytest.mark.parametrize("case", [c for c in SMALL if c.kind == "loss" and c.form == "train" and c.fill in FINITE], ids=lambda c: c.name)
def test_loss_reference_equals_torch_autograd_in_float64(case):
    c = case
    d, ref, _ = _setup(c)
    B, C = c.B, c.C
    x = d.x.double().clone().requires_grad_(True)
    y, ig = d.target, lo.ignore_value(c)
    w = d.weight.double() if c.weight else None
    assert _close(ref["probs"], torch.softmax(x.detach(), 1), 1e-13)
    assert torch.equal(ref["argmax"].long(), torch.argmax(d.x, 1))
    kept = y != ig
    if c.bad != "none":                       # divergence: a NaN loss and a NaN dlogits row, where torch asserts
        r = 0 if B < 3 else 2
        assert torch.isnan(ref["out0"]).all() and torch.isnan(ref["dlogits"][r]).all() and ref["wsum"][r] == 1
        assert torch.isnan(ref["loss_rows"][r]) and torch.isnan(ref["coef"][r])
        return
    if not c.focal:
        per = F.cross_entropy(x, y, weight=w, ignore_index=ig, reduction="none")
        norm = ((w[y.clamp(0, C - 1)] if c.weight else torch.ones(B, dtype=torch.float64)) * kept).sum()
    else:                                     # the literal formula: -alpha[y] (1 - p_y)^gamma log p_y over kept rows, mean over their count
        logp = torch.log_softmax(x, 1).gather(1, y.clamp(0, C - 1)[:, None])[:, 0]
        a = w[y.clamp(0, C - 1)] if c.weight else 1.0
        per = torch.where(kept, -a * (1.0 - logp.exp()) ** c.gamma * logp, torch.zeros(B, dtype=torch.float64))
        norm = kept.sum().double()
    assert _close(ref["loss_rows"], per.detach(), 1e-12)
    empty = not bool(norm > 0)
    if c.reduction == 0:
        if empty:                             # divergence: loss 0 and factor 0, where F.cross_entropy gives 0 / 0 = NaN
            assert ref["out0"].item() == 0.0 and ref["out1"].item() == 0.0 and bool((ref["dlogits"] == 0).all())
            if not c.focal:
                assert torch.isnan(F.cross_entropy(x, y, weight=w, ignore_index=ig))
            return
        total = per.sum() / norm
        if not c.focal:
            assert _close(total.detach(), F.cross_entropy(x, y, weight=w, ignore_index=ig).detach(), 1e-12)
    else:
        total = per.sum()
        assert ref["out1"].item() == 1.0
    assert _close(ref["out0"], total.detach().reshape(1), 1e-12)
    # the backward: scalar grad_out on the reduced loss, per-row grad_out on the per-row terms of that reduction
    g = d.gout.double()
    obj = (per * g / (norm if c.reduction == 0 else 1.0)).sum() if c.per_row else total * g[0]
    (gx,) = torch.autograd.grad(obj, x)
    pt1 = c.focal and 0 < c.gamma < 1 and bool(torch.isnan(gx).any())
    if pt1:                                   # divergence: the limit 0 of the second gradient term at p_y == 1, where autograd has inf * 0
        rows = torch.isnan(gx).any(1)
        assert bool(torch.isfinite(ref["dlogits"]).all()) and _close(ref["dlogits"][~rows], gx[~rows], 1e-10)
    else:
        assert _close(ref["dlogits"], gx, 1e-10)


def test_argmax_and_softmax_of_rows_that_are_not_finite():
    """argmax is torch.argmax and probs are NaN exactly where torch.softmax's are; a row with NaNs at columns 1 and 2 gives 1, a row
    of -inf gives 0"""
    seen = set()
    for c in SMALL:
        if c.kind == "loss" and c.fill in ("nan1", "nan2", "pinf", "ninf", "ties", "equal"):
            d, ref, yard = _setup(c)
            assert torch.equal(ref["argmax"].long(), torch.argmax(d.x, 1)), c.name
            assert torch.equal(yard["argmax"], ref["argmax"])
            assert torch.equal(torch.isnan(ref["probs"]), torch.isnan(torch.softmax(d.x.double(), 1))), c.name
            if c.fill == "nan2" and c.C >= 3:
                assert ref["argmax"][0].item() == 1
            if c.fill == "ninf":
                assert ref["argmax"][0].item() == 0 and torch.isnan(ref["probs"][0]).all()
            seen.add(c.fill)
    assert seen == {"nan1", "nan2", "pinf", "ninf", "ties", "equal"}
    for row, want in (([0.0, lo.NAN, lo.NAN], 1), ([lo.NAN, 1.0, lo.NAN], 0), ([-lo.INF] * 3, 0), ([1.0, lo.INF, lo.INF], 1), ([2.0, 2.0, 1.0], 0)):
        t = torch.tensor([row])
        assert lo.argmax_rows(t).item() == want == torch.argmax(t, 1).item()


TORCH_OPT = dict(adam=(torch.optim.Adam, {}), adamw=(torch.optim.AdamW, {}), nadam=(torch.optim.NAdam, dict(decoupled_weight_decay=True)),
                 radam=(torch.optim.RAdam, {}), radam_decoupled=(torch.optim.RAdam, dict(decoupled_weight_decay=True)),
                 sgd=(torch.optim.SGD, {}), sgd_momentum_fresh=(torch.optim.SGD, dict(momentum=0.9)),
                 sgd_dampening=(torch.optim.SGD, dict(momentum=0.9, dampening=0.25)), sgd_nesterov=(torch.optim.SGD, dict(momentum=0.9, nesterov=True)))


@pytest.mark.parametrize("variant", lo.VARIANTS)
@pytest.mark.parametrize("wd", (0.0, 0.05))
def test_optimizer_reference_equals_torch_optim_in_float64(variant, wd):
    """eight steps from a fresh state: the step scalars of utils._step_scalars (NAdam's float32 mu_product included) and the
    float64 element update against torch.optim in float64"""
    from nkb_classification.utils import _step_scalars
    gen = torch.Generator().manual_seed(5)
    n = 37
    w0 = torch.randn(n, generator=gen, dtype=torch.float64)
    grads = [torch.randn(n, generator=gen, dtype=torch.float64) for _ in range(8)]
    cls, extra = TORCH_OPT[variant]
    p = w0.clone().requires_grad_(True)
    kw = dict(lr=lo.HYPER["lr"], weight_decay=wd, **extra)
    if not variant.startswith("sgd"):
        kw.update(betas=(lo.HYPER["beta1"], lo.HYPER["beta2"]), eps=lo.HYPER["eps"])
    opt = cls([p], **kw)
    kind = "sgd" if variant.startswith("sgd") else "radam" if variant.startswith("radam") else variant
    state, w, m, v = {}, w0.clone(), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    for g in grads:
        p.grad = g.clone()
        opt.step()
        skw = dict(lr=lo.HYPER["lr"], beta1=lo.HYPER["beta1"], beta2=lo.HYPER["beta2"], eps=lo.HYPER["eps"])
        if kind == "sgd":
            skw.update(momentum=extra.get("momentum", 0.0), dampening=extra.get("dampening", 0.0), nesterov=extra.get("nesterov", False))
        if variant == "radam_decoupled":
            skw.update(decoupled=True)
        code, cs = _step_scalars(kind, state, **skw)
        T = lambda x: torch.tensor(x, dtype=torch.float64)
        a = dict(lr=T(lo.HYPER["lr"]), wd=T(wd), beta1=T(extra.get("momentum", 0.0) if kind == "sgd" else lo.HYPER["beta1"]), beta2=T(lo.HYPER["beta2"]),
                 eps=T(lo.HYPER["eps"]), gs=T(1.0), c0=T(cs[0]), c1=T(cs[1]), c2=T(cs[2]), c3=T(cs[3]))
        w, m, v = lo.optim_update(code, a, w, g, m, v)
        assert _close(w, p.detach(), 1e-13), variant
    if variant.startswith("radam"):
        assert state["step"] == 8       # steps 1..5 unrectified, 6..8 rectified


@pytest.mark.parametrize("case", [c for c in SMALL if c.kind == "optim"][::3], ids=lambda c: c.name)
def test_optimizer_case_reference_is_the_torch_step_from_its_state(case):
    """the case's reference (arbitrary state, its step number, grad_scale) is optim_update with the scalars of that step, and the
    shadow is the bf16 rounding of the new weights"""
    c = case
    d, ref, yard = _setup(c)
    code, args = lo.step_scalars(c)
    a = {k: lo.S(v).double() for k, v in args.items()}
    w, m, v = lo.optim_update(code, a, d.w.double(), d.g.double(), d.m.double(), d.v.double())
    if c.skip == "1":
        w, m, v = d.w.double(), d.m.double(), d.v.double()
    assert torch.equal(ref["w"], w)
    if "shadow" in yard and c.skip != "1":
        assert torch.equal(yard["shadow"], lo.rnd(yard["w"], "bf16"))
    if c.variant.startswith("radam"):
        assert (args["c2"] == 0.0) == (c.step <= 5)


def test_plain_references():
    """unscale, bucket sum, segment sum of squares and image_prep against their plain expressions"""
    for c in SMALL:
        if c.kind == "unscale":
            d, ref, _ = _setup(c)
            assert ref["found"].item() == (1.0 if c.bad_at != "none" else c.found0)
        elif c.kind == "bucket":
            d, ref, _ = _setup(c)
            assert torch.equal(ref.get("out", ref.get("out16")), d.parts.double()[:, :c.n].sum(0))
        elif c.kind == "segsq":
            d, ref, _ = _setup(c)
            for k, L in enumerate(c.lengths):
                lo_, hi = int(d.offsets[k]), int(d.offsets[k + 1])
                assert hi - lo_ == L and _close(ref["out"][k], (d.x.double()[lo_:hi] ** 2).sum(), 1e-14)
        elif c.kind == "prep":
            d, ref, _ = _setup(c)
            Bn, Hs, Ws, Ho, Wo = c.img
            for b in range(Bn):
                h, w = (int(d.sizes[b, 0]), int(d.sizes[b, 1])) if d.sizes is not None else (Hs, Ws)
                fl = int(d.flags[b]) if d.flags is not None else 0
                top, left = (Ho - h) // 2, (Wo - w) // 2
                for (yy, xx) in ((0, 0), (Ho - 1, Wo - 1), (Ho // 2, Wo // 2), (top, left)):
                    yf, xf = (Ho - 1 - yy if fl & 2 else yy), (Wo - 1 - xx if fl & 1 else xx)
                    inside = 0 <= yf - top < h and 0 <= xf - left < w
                    for ch in range(3):
                        P = float(d.src[b, yf - top, xf - left, ch]) if inside else float(lo.S(c.fillv))
                        mean, std = float(lo.S(d.mean[ch])), float(lo.S(d.std[ch]))
                        assert abs(ref["out"][b, ch, yy, xx].item() - (P - 255.0 * mean) / (255.0 * std)) <= 1e-12 * 255
    for found in (0.0, 1.0):
        for tracker, interval, scale in ((0, 3, 65536.0), (2, 3, 65536.0), (2, 3, 3e38)):
            s, t, f, last = lo.scaler_step(scale, tracker, found, 2.0, 0.5, interval)
            sc, gt, fi = torch.full((1,), scale), torch.full((1,), tracker, dtype=torch.int32), torch.full((1,), found)
            torch._amp_update_scale_(sc, gt, fi, 2.0, 0.5, interval)
            held = scale == 3e38 and not found and tracker + 1 == interval
            assert t == gt.item() and (s == sc.item() or held) and f == 0.0 and last == found
            if held:
                assert s == float(torch.tensor(3e38))


@pytest.mark.parametrize("case", SMALL, ids=lambda c: c.name)
def test_yardstick_is_inside_every_bound(case):
    d, ref, yard = _setup(case)
    for label, y in (("torch's order", yard), ("second order", lo.outputs(case, d, exact=False, order="strided"))):
        v = lo.verdict(case, d, ref, y)
        assert v, "nothing was judged"
        assert all(r <= 1.0 for r, _, _ in v.values()), (label, v)
    for k, (r, err, bound) in lo.yardstick_to_reference(case, d, ref, yard).items():
        assert r <= 1.0, f"{case.name}: the yardstick's {k} is {err:.3e} from the reference (bound {bound:.3e})"
    if case.exact:
        assert lo.representable(case, d, ref), "an exact case whose float64 reference is no number of its output type"


JUDGED = dict(loss=dict(train=("argmax", "probs", "loss_rows", "wsum", "coef", "out0", "out1", "dlogits"), logger=("argmax", "probs"),
                        noprobs=("argmax", "loss_rows", "wsum", "coef", "out0", "out1")),
              unscale=("g", "found"), scaler=("scale", "tracker", "found", "last"), segsq=("out",), prep=("out",))


@pytest.mark.parametrize("case", SMALL, ids=lambda c: c.name)
def test_no_element_is_left_out(case):
    """every output of the case is judged, over all of its elements: a yardstick with one element moved (any one, here the first, a
    middle one and the last) fails the check of that output and of no other"""
    c = case
    d, ref, yard = _setup(c)
    if c.kind == "loss":
        want = JUDGED["loss"][c.form]
    elif c.kind == "optim":
        want = ("w", "m", "v") + (("shadow",) if c.shadow != "none" else ())
    elif c.kind == "bucket":
        want = dict(f32=("out",), bf16=("out16",), both=("out", "out16"))[c.form3]
    else:
        want = JUDGED[c.kind]
    assert set(lo.verdict(c, d, ref, yard)) == set(want)
    for name in want:
        n = yard[name].numel()
        for pos in sorted({0, n // 2, n - 1}):
            y = dict(yard)
            t = yard[name].clone().reshape(-1)
            t[pos] = t[pos] * 2.0 + 1.0 if bool(torch.isfinite(t[pos])) else 0.0
            y[name] = t.reshape(yard[name].shape)
            if c.kind == "loss" and name in ("probs", "coef", "out1") and "dlogits" in y and not c.exact:
                y["dlogits"] = lo.dlogits_of(c, d, y["probs"], y["coef"], y["out1"], torch.float32).double()
            bad = {k for k, (r, _, _) in lo.verdict(c, d, ref, y).items() if not r <= 1.0}
            assert bad == {name}, (name, pos, bad)


@pytest.mark.parametrize("mutant", lo.MUTANTS)
def test_mutant_is_rejected_by_the_outputs_it_corrupts(mutant):
    hit = 0
    for case in SMALL + [c for c in lo.CASES if c.big and c.kind == "optim" and mutant in ("second_group_dropped", "second_trip_dropped_optim")][:2]:
        if not lo.mutant_applies(case, mutant):
            continue
        d, ref, yard = _setup(case) if not case.big else (lambda d: (d, None, lo.outputs(case, d, exact=False)))(lo.make(case, seed=7))
        rej = lo.rejecting(case, d, mutant, ref if ref is not None else {}, yard)
        if rej is None:
            continue
        hit += 1
        assert rej and set(rej) <= set(lo.REJECTED_BY[mutant]), f"{case.name}: {mutant} is rejected by {rej}, not by {lo.REJECTED_BY[mutant]}"
    assert hit >= 1, f"{mutant} exists at no case"
    assert set(lo.MUTANTS) == set(lo.REJECTED_BY)


def test_table_covers_what_the_kernels_dispatch_on():
    L = [c for c in lo.CASES if c.kind == "loss"]
    T = [c for c in L if c.fill == "random" and c.form == "train"]
    assert {c.C for c in T} >= set(lo.LOSS_C) and {c.B for c in T} >= set(lo.LOSS_B)
    assert {(c.B, c.C) for c in T} >= {(b, k) for b in lo.LOSS_B for k in lo.LOSS_C}
    assert any(c.B * c.C > 2048 * 256 for c in T) and any(c.B > 256 for c in T)
    assert {c.pad for c in T} == set(lo.LOSS_PADS) and all(len(set(p)) == 3 for p in lo.LOSS_PADS[1:])
    assert {c.gamma for c in T if c.focal} == set(lo.GAMMAS) and {c.weight for c in T if c.focal} == {c.weight for c in T if not c.focal} == {True, False}
    assert {(c.ignore, c.ignored) for c in T} == set(lo.IGNORES) and {c.bad for c in T} == {"none", "neg", "C"}
    assert {(c.focal, c.reduction) for c in T} == {(f, r) for f in (False, True) for r in (0, 1, 2)} and {c.per_row for c in T} == {True, False}
    assert {c.form for c in L} == {"train", "logger", "noprobs"}
    assert {c.fill for c in L} >= {"offset", "spread", "ties", "equal", "nan1", "nan2", "pinf", "ninf"}
    assert any(c.fill == "spread" and c.focal and c.gamma == 0.5 for c in L)
    assert any(c.exact and c.B > 256 for c in L) and any(c.exact and c.C > 64 for c in L)
    O = [c for c in lo.CASES if c.kind == "optim" and not c.zero_state]
    for v in lo.VARIANTS:
        mine = [c for c in O if c.variant == v]
        assert {c.n for c in mine} == set(lo.OPTIM_N) | {lo.OPTIM_BIG}, v
        assert {lo.optim_path(c) for c in mine if c.n == lo.OPTIM_BIG} == {"vector", "scalar"}
        assert {c.offset for c in mine} == {0, 1} and {c.shadow for c in mine} == {"aligned", "odd", "none"}
        assert {c.wd for c in mine} == {0.0, 0.05} and len({c.gscale for c in mine}) == 3
        assert {c.step for c in mine} == {1, 5, 6, 100} and {c.skip for c in mine} == {"none", "0", "1"}
    n4, stride = lo.OPTIM_BIG // 4, 2048 * 256
    assert 3 * stride < n4 < 4 * stride and lo.OPTIM_BIG % 4 and lo.OPTIM_BIG > 4096 * 256
    assert sum(c.zero_state for c in lo.CASES) == 4
    Un = [c for c in lo.CASES if c.kind == "unscale"]
    assert {c.n for c in Un} >= {1, 3, 4, 5, 1027, lo.UNSCALE_BIG} and lo.UNSCALE_BIG > 4096 * 256 * 4
    assert {c.bad_at for c in Un} == {"none", "first", "mid", "lastvec", "lasttail", "overflow"}
    assert {c.found0 for c in Un if c.bad_at == "none"} == {0.0, 1.0} and {c.scale for c in Un} >= {65536.0, 3.0}
    Bu = [c for c in lo.CASES if c.kind == "bucket"]
    assert {c.nparts for c in Bu} == {1, 2, 3, 8} and {c.n for c in Bu} == {1, 7, 8, 9, 1003, lo.BUCKET_BIG} and {c.form3 for c in Bu} == {"f32", "bf16", "both"}
    assert len([c for c in lo.CASES if c.kind == "scaler"]) == 16
    Pr = [c for c in lo.CASES if c.kind == "prep"]
    assert {c.img[4] % 4 for c in Pr} == {0, 1, 2, 3} and {c.sizes for c in Pr} == {"random", "none", "one", "full"}
    assert {c.fillv for c in Pr} == {0.0, 114.0} and {c.flags for c in Pr} == {"cycle", "none"}
    assert any(c.out_offset % 4 and c.img[4] % 4 == 0 for c in Pr) and any(c.img[0] * c.img[3] * ((c.img[4] + 3) // 4) > 256 * 32 * 256 for c in Pr)
