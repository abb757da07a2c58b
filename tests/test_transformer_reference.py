"""CPU proof that tests/test_transformer_ops_gpu.py can fail: the float64 reference of tests/transformer_reference.py equals torch's
layer_norm, gelu, relu6 and softmax and their autograd in float64 (and the plain tensor expressions of the other operations) on
every case below 2^21 elements (the larger ones are the same formulas at another size), every exact case is representable, the fp32
yardstick sits inside every bound in two summation orders, every mutant of the yardstick is rejected by exactly the outputs
REJECTED_BY names, and the integer twin of the dropout generator agrees with the C++ functions of csrc/common.h (compiled for the
host from their text in that header, plus recorded vectors of that same program for a machine without a host compiler)."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest
import torch
import torch.nn.functional as F

import transformer_reference as tr

DEV = "cpu"
_CACHE = {}
SMALL = [c for c in tr.CASES if not c.big]
COMMON_H = Path(__file__).resolve().parents[1] / "nkb-classification_amd" / "csrc" / "common.h"


def _setup(case):
    """(operands, reference, yardstick) of a case, computed once and left unchanged"""
    if case.name not in _CACHE:
        d = tr.make(case, DEV, seed=7)
        _CACHE[case.name] = (d, tr.outputs(case, d, exact=True), tr.outputs(case, d, exact=False))
    return _CACHE[case.name]


def _close(a, b, tol=1e-11):
    a, b = a.double(), b.double()
    scale = max(b.abs().max().item(), 1.0) if b.numel() else 1.0
    return a.shape == b.shape and (a.numel() == 0 or (a - b).abs().max().item() <= tol * scale)


@pytest.mark.parametrize("case", [c for c in SMALL if c.kind == "ln"][::3], ids=lambda c: c.name)
def test_layernorm_reference_equals_torch_autograd_in_float64(case):
    """with the row's own statistics as the supplied mean / rstd the backward is the autograd of F.layer_norm"""
    c = case
    d = tr.make(c, DEV, seed=3)
    ref = tr.outputs(c, d, exact=True)
    x = d.x.double().clone().requires_grad_(True)
    gamma, beta = d.gamma.double().clone().requires_grad_(True), d.beta.double().clone().requires_grad_(True)
    y = F.layer_norm(x, (c.D,), gamma, beta, eps=d.eps)
    assert _close(ref["y"], y.detach(), 1e-10)
    assert _close(ref["mean"], x.detach().mean(1)) and _close(ref["rstd"], (x.detach().var(1, unbiased=False) + d.eps).rsqrt())
    d.bmean, d.brstd = ref["mean"], ref["rstd"]
    ref = tr.outputs(c, d, exact=True)
    gx, gg, gb = torch.autograd.grad(y, (x, gamma, beta), d.dy.double())
    assert _close(ref["dx"] - (d.addv.double() if c.add else 0.0), gx, 1e-9)
    assert _close(ref["dgamma"] - d.dgamma0.double(), gg, 1e-9) and _close(ref["dbeta"] - d.dbeta0.double(), gb, 1e-9)
    if c.second == "scaled":
        sel = torch.arange(c.rows) // c.rps
        assert torch.equal(ref["copy"], tr.rnd(tr.f32(tr.rnd(ref["dx"], c.dtype) * d.rsc.double()[sel][:, None]), c.dtype))
    if c.second in ("e4m3", "e5m2"):
        sel = torch.arange(c.rows) // max(c.rps, 1)
        sc = d.rsc.double()[sel][:, None] if c.row_scale else 1.0
        assert _close(ref["colsum"], d.colsum0.double() + (tr.rnd(ref["dx"], c.dtype) * sc).sum(0), 1e-12)


@pytest.mark.parametrize("case", [c for c in SMALL if c.kind == "act"], ids=lambda c: c.name)
def test_activation_reference_equals_torch_autograd_in_float64(case):
    c = case
    d = tr.make(c, DEV, seed=3)
    ref = tr.outputs(c, d, exact=True)
    x = d.x.double().clone().requires_grad_(True)
    y = dict(gelu=lambda t: F.gelu(t), quick_gelu=lambda t: t * torch.sigmoid(1.702 * t), relu6=F.relu6)[c.op](x)
    (gx,) = torch.autograd.grad(y, x, d.dy.double())
    assert _close(ref["y"], y.detach(), 1e-12)
    if c.op == "relu6":      # torch's own relu6 backward includes the lower edge on some builds: the strict rule is hardtanh_backward's
        edge = (d.x.double() == 0) | (d.x.double() == 6)
        assert bool((ref["dx"][edge] == 0).all()) and _close(ref["dx"][~edge], gx[~edge])
    else:
        assert _close(ref["dx"], gx, 1e-12) and _close(ref["gp"] * d.dy.double(), gx, 1e-12)


@pytest.mark.parametrize("case", [c for c in SMALL if c.kind == "softmax"], ids=lambda c: c.name)
def test_softmax_reference_equals_torch_autograd_in_float64(case):
    c = case
    d = tr.make(c, DEV, seed=3)
    ref = tr.outputs(c, d, exact=True)
    sc = float(torch.tensor(c.scale, dtype=torch.float32))
    s = d.s.double().clone().requires_grad_(True)
    p = torch.softmax(s * sc, 1)
    assert _close(ref["p"][:, :c.D], p.detach(), 1e-13) and bool((ref["p"][:, c.D:] == 0).all()) and ref["p"].shape[1] == c.ld
    # the backward takes the STORED probabilities: the autograd identity holds for them as a function value
    ps = d.p.double()
    want = sc * ps * (d.dp.double() - (d.dp.double() * ps).sum(1, keepdim=True))
    assert _close(ref["ds"][:, :c.D], want, 1e-13) and bool((ref["ds"][:, c.D:] == 0).all())
    (gs,) = torch.autograd.grad(p, s, d.dp.double())
    p64 = p.detach()
    assert _close(sc * p64 * (d.dp.double() - (d.dp.double() * p64).sum(1, keepdim=True)), gs, 1e-12)


@pytest.mark.parametrize("case", [c for c in SMALL if c.kind in ("scale", "transpose", "assemble", "colsum", "dropout")], ids=lambda c: c.name)
def test_other_references_equal_the_plain_expressions(case):
    c = case
    d, ref, yard = _setup(c)
    if c.kind == "scale":
        want = d.x.double() * d.scale.double()[:, None] + (d.addv.double() if c.add else 0.0)
        assert torch.equal(ref["out"], want)
    elif c.kind == "transpose":
        Z = c.outer * c.inner
        want = torch.zeros(Z, c.D, c.ld, dtype=torch.float64)
        off = max(c.which, 0) * c.inner * c.D
        for zo in range(c.outer):
            for zi in range(c.inner):
                want[zo * c.inner + zi, :, :c.T] = d.src.double()[zo, :, off + zi * c.D:off + (zi + 1) * c.D].t()
        assert torch.equal(ref["out"], want)
    elif c.kind == "assemble":
        B, Tn, D = c.rows, c.T, c.D
        want = torch.empty(B, Tn, D, dtype=torch.float64)
        if c.cls:
            want[:, 0], want[:, 1:] = d.clsv.double() + d.pos.double()[0], d.tok.double() + d.pos.double()[1:]
            assert torch.equal(ref["dtok"], d.g.double()[:, 1:])
        else:
            want[:] = d.tok.double() + d.pos.double()
        assert torch.equal(ref["x"], want)
    elif c.kind == "colsum":
        assert _close(ref["out"], d.out0.double() + d.x.double().sum(0), 1e-13)
    else:
        keep = tr.dropout_keep(torch.arange(c.D), c.seed, c.p)
        p32 = float(torch.tensor(c.p, dtype=torch.float32))
        for name, src in (("out", d.x), ("dx", d.g)):
            want = torch.where(keep, src.double() / (1.0 - p32), torch.zeros((), dtype=torch.float64)) + (d.addv.double() if c.add else 0.0)
            assert _close(ref[name], want, 1e-15)
        assert torch.equal(ref["mask"], keep)
    for k, (r, err, bound) in tr.yardstick_to_reference(c, d, ref, yard).items():
        assert r <= 1.0, f"{c.name}: the yardstick's {k} is {err:.3e} from the reference (bound {bound:.3e})"


@pytest.mark.parametrize("case", SMALL, ids=lambda c: c.name)
def test_yardstick_is_inside_every_bound(case):
    d, ref, yard = _setup(case)
    for label, y in (("torch's order", yard), ("second order", tr.outputs(case, d, exact=False, order="strided"))):
        v = tr.verdict(case, d, ref, y)
        assert v, "nothing was judged"
        print(case.name, label, {k: f"{r:.3f}" for k, (r, _, _) in v.items()})
        assert all(r <= 1.0 for r, _, _ in v.values()), (label, v)
    if case.exact:
        assert tr.representable(case, d, ref), "an exact case whose float64 reference is no number of its output type"


def test_exact_dx_widths():
    """dx is compared value for value at least at D = 8, 64, 128 and 256"""
    widths = set()
    for c in SMALL:
        if c.kind == "ln" and c.exact:
            d, ref, _ = _setup(c)
            if tr._ln_dx_exact(c, d, ref):
                widths.add(c.D)
    assert {8, 64, 128, 256} <= widths, widths


@pytest.mark.parametrize("mutant", tr.MUTANTS)
def test_mutant_is_rejected_by_the_outputs_it_corrupts(mutant):
    """Every exact case at which the mutant changes the yardstick rejects it, and so does every random case for the mutants of a
    formula; the checks that reject belong to outputs tr.REJECTED_BY names, and to no other."""
    hit = 0
    for case in SMALL:
        if not tr.mutant_applies(case, mutant):
            continue
        d, ref, yard = _setup(case)
        rej = tr.rejecting(case, d, mutant, ref, yard)
        if rej is None or not (case.exact or mutant in tr.FORMULA_MUTANTS):
            continue
        hit += 1
        assert rej and set(rej) <= set(tr.REJECTED_BY[mutant]), f"{case.name}: {mutant} is rejected by {rej}, not by {tr.REJECTED_BY[mutant]}"
    assert hit >= 1, f"{mutant} exists at no case"
    assert set(tr.MUTANTS) == set(tr.REJECTED_BY)


def test_table_covers_what_the_kernels_dispatch_on():
    ln = [c for c in tr.CASES if c.kind == "ln"]
    for D in tr.LN_VW4 + tr.LN_VW2 + tr.LN_TAIL:
        mine = [c for c in ln if c.D == D]
        assert {c.rows for c in mine} >= set(tr.LN_ROWS) and {c.dtype for c in mine} == {"bf16", "f32"}
        assert {c.exact for c in mine} == {True, False} and {c.add for c in mine} == {True, False}
        assert any(len(set(c.pad)) == 3 for c in mine), D
    assert {tr.ln_form(D)[1:] for D in tr.LN_VW4} == {(4, n) for n in (1, 2, 3, 4, 5, 8)}
    assert {tr.ln_form(D)[1:] for D in tr.LN_VW2} == {(2, n) for n in (1, 3, 5, 7)}
    assert all(tr.ln_form(D)[0] for D in tr.LN_TAIL) and {tr.ln_form(D)[2] for D in tr.LN_TAIL} == {1, 2, 5, 8}
    assert {1, 15, 16, 17, 1024} <= {tr.ln_bwd_blocks(c.rows) for c in ln}
    assert any((c.rows + 3) // 4 > 512 for c in ln) and any((c.rows + 3) // 4 > 4096 for c in ln) and any((c.rows + 43) // 44 > 1024 for c in ln)
    assert any(c.second != "none" and (c.rows + 3) // 4 > 1024 for c in ln)
    assert {(c.second, c.row_scale) for c in ln} >= {("e5m2", False), ("e5m2", True), ("e4m3", True), ("scaled", True)}
    assert {tr.colsum_splits(c.rows) for c in tr.CASES if c.kind == "colsum" and c.form == "work"} == {2, 6, 48, 256}
    assert any(c.kind == "colsum" and c.D % 4 for c in tr.CASES)
    assert any(c.kind == "softmax" and (c.rows + 3) // 4 > 256 * 32 for c in tr.CASES)
    assert any(c.kind in ("act", "dropout") and c.D // (tr.vec(c.dtype) if c.kind == "act" else 1) > 256 * 4096 * 256 // 256 for c in tr.CASES)
    assert any(c.kind == "dropout" and c.seed >> 32 for c in tr.CASES)
    assert {c.alias for c in tr.CASES if c.kind == "dropout"} == {"none", "in", "add"}
    for c in ln:
        if c.exact:
            assert c.rows * 60 + 5 < 2 ** 23


def test_sizing_rules_match_the_library():
    """the host-side sizing the table relies on is the library's (this entry point launches nothing)"""
    from nkb_classification import hip
    for D in (8, 72, 256, 2048):
        assert tr.ln_ws_floats(D) == hip.layernorm_ws(D)
        assert 1024 * 3 * D + tr.LN_SLICES * 3 * D <= tr.ln_ws_floats(D)


def test_kept_share_of_the_host_twin():
    """the kept share sits within 4 sqrt(p (1 - p) / n) of 1 - p at n = 2^20 (a binomial bound, four standard deviations)"""
    n = 1 << 20
    i = torch.arange(n)
    for p in (0.1, 0.5, 0.999):
        for seed in (0, 0x1234567, 0x9e3779b97f4a7c15):
            share = tr.dropout_keep(i, seed, p).double().mean().item()
            assert abs(share - (1 - p)) <= 4 * (p * (1 - p) / n) ** 0.5, (p, seed, share)
    assert bool(tr.dropout_keep(i, 5, 0.0).all())


# (index, seed, p) -> (hash, thresh, keep): the output of the program below, recorded
RECORDED = (((0, 0, 0.1), (0, 429496736, 0)), ((77, 305419896, 0.5), (2207615182, 2147483648, 1)),
            ((4294967296, 11400714819323198485, 0.999), (998066836, 4290672384, 0)),
            ((1234567890123, 81985529216486895, 0.25), (891995047, 1073741824, 0)), ((255, 1, 0.0), (3299840524, 0, 1)))


def _twin(i, seed, p):
    it = torch.tensor([i], dtype=torch.int64)
    h = tr.dropout_hash(it & tr.M32, tr.dropout_hi_term((it >> 32) & tr.M32, (seed >> 32) & tr.M32), seed & tr.M32)
    return int(h), tr.dropout_thresh(p), int(tr.dropout_keep(it, seed, p))


def test_dropout_twin_matches_recorded_vectors():
    for (i, seed, p), want in RECORDED:
        assert _twin(i, seed, p) == want
    for p in (0.5, 0.1, 0.0):
        for hi in (0, 0x9e3779b9):
            seed = tr.seed_hitting(77, p, hi)
            assert _twin(77, seed, p)[0] == tr.dropout_thresh(p) and seed >> 32 == hi


def test_dropout_twin_matches_the_cpp_generator(tmp_path):
    """mix32 ... dropout_keep are __host__ __device__ in csrc/common.h: their text, compiled for the host as it stands, is evaluated
    on 4000 (index, seed, p) triples, indices above 2^32 and seeds with a high word included.  Without a host compiler the recorded
    vectors above (the same program's output) stand alone."""
    cxx = next((x for x in ("c++", "g++", "clang++") if shutil.which(x)), None)
    if cxx is None:
        test_dropout_twin_matches_recorded_vectors()
        return
    src = COMMON_H.read_text()
    body = src[src.index("__host__ __device__ __forceinline__ unsigned mix32"):src.index("// ---- division by a runtime constant")]
    assert all(re.search(rf"\b{f}\(", body) for f in ("mix32", "dropout_thresh", "dropout_hi_term", "dropout_hash", "dropout_keep"))
    prog = "#include <cstdio>\n#define __host__\n#define __device__\n#define __forceinline__ inline\n" + body + r"""
int main() {
    unsigned long long i, seed; float p;
    while (scanf("%llu %llu %f", &i, &seed, &p) == 3)
        printf("%u %u %d\n", dropout_hash((unsigned)i, dropout_hi_term((unsigned)(i >> 32), (unsigned)(seed >> 32)), (unsigned)seed),
               dropout_thresh(p), (int)dropout_keep(i, (unsigned)seed, (unsigned)(seed >> 32), dropout_thresh(p)));
    return 0;
}
"""
    (tmp_path / "twin.cpp").write_text(prog)
    subprocess.run([cxx, "-O1", "-o", str(tmp_path / "twin"), str(tmp_path / "twin.cpp")], check=True)
    gen = torch.Generator().manual_seed(9)
    n = 4000
    idx = torch.randint(0, 1 << 40, (n,), generator=gen)
    idx[:64] = torch.arange(64)
    seeds = [int(a) << 32 | int(b) for a, b in zip(torch.randint(0, 1 << 32, (n,), generator=gen), torch.randint(0, 1 << 32, (n,), generator=gen))]
    seeds[:8] = [0] * 8
    ps = [(0.0, 0.1, 0.5, 0.999, 0.25, 0.9999999)[k % 6] for k in range(n)]
    text = "".join(f"{int(i)} {s} {p!r}\n" for i, s, p in zip(idx, seeds, ps))
    out = subprocess.run([str(tmp_path / "twin")], input=text, capture_output=True, text=True, check=True).stdout.split("\n")
    for k in range(n):
        assert tuple(int(t) for t in out[k].split()) == _twin(int(idx[k]), seeds[k], ps[k]), (int(idx[k]), seeds[k], ps[k])
