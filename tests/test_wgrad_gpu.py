"""Every weight-gradient kernel against the float64 reference of tests/wgrad_reference.py: conv_wgrad_kernel<bf16 | float> through
nkb_conv_wgrad / nkb_conv_wgrad_assign, nkb_stem_wgrad and nkb_gemm_tn_batched, wgrad3x3p_kernel<3 | 4 | 5 | 6, 3>, wgradr_kernel<3, 4>
plain and transposed and <2, 8>, wgrad8p_kernel (in a child process under NKB_WGRAD256=2: tests/wgrad8p_probe.py), and the four
wgrad_reduce kernels behind them.

Every case runs in two data regimes: integers -2 .. 2, where the result must equal the float64 reference bit for bit, and
|N(0, 1)|, where it must stay inside the derived bound A (K + S + c) 2^-24 of the result.  Operands lie in buffers with padding columns
and trailing rows of finite garbage (1e4), dw / dbias between guard zones of a sentinel, the workspace is handed over at its advertised
size and followed by NaN words.  Per regime a case runs the slab form twice (bit-identical), the assign form where the entry has one,
then the atomic form; after every launch nkb_wgrad_last_kernel must name the kernel, the form, the split count of the restated plan
and the reduce kernel the case's name promises, and the family launch counters move only for the family that ran.  Each case prints
"RATIO kernel case form check err= bound= ratio=" for the positive regime (visible with -rP); a last test asserts that the kernels
and reduce paths the cases ran are the whole list.  tests/test_wgrad_reference.py proves on the CPU that these verdicts reject
subtly wrong kernels."""
import json
import os
import subprocess
import sys
from pathlib import Path

import pytest
import torch

import wgrad_reference as wr

pytestmark = pytest.mark.gpu

from nkb_classification import hip  # noqa: E402

ROOT = Path(__file__).resolve().parents[1]
DEV = "cuda"
G = 64                  # guard floats on each side of dw / dbias (a multiple of 4: the outputs stay 16-byte aligned)
GROWS = 4               # guard rows on each side of a batched output
TAIL = 8                # NaN words behind the advertised workspace
SENT = -8192.0          # bf16 / fp32-exact sentinel of the guard zones
COUNTERS = {"wgrad3x3": "wgrad3x3", "wgradr": "wgradr", "wgrad8p": "wgrad8p"}
RAN_KERNELS, RAN_REDUCES, WORST = set(), set(), {}


def cu_count() -> int:
    return torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count


def _input(t, ld):
    """t [rows][C] inside a [rows + GR][ld] buffer: padding columns and the rows behind the last one hold finite garbage"""
    rows, C = t.shape
    buf = torch.full((rows + wr.GR, ld), wr.GARBAGE, device=DEV).to(t.dtype)
    buf[:rows, :C] = t
    return buf


def _output(pre, unaligned):
    """pre (fp32, any shape) flat between two guard zones of the sentinel; (buffer, offset of the output)"""
    n = pre.numel()
    off = G + (1 if unaligned else 0)
    buf = torch.full((off + n + G,), SENT, device=DEV)
    buf[off:off + n] = pre.flatten()
    return buf, off


def _raw(t):
    return t.view(torch.int16) if t.dtype.itemsize == 2 else t.view(torch.int32)


class Launcher:
    """the operand buffers of one case and regime, and one launch of a form"""

    def __init__(self, c, d):
        self.c, self.d, self.g = c, d, wr.geom(c)
        g = self.g
        self.hd = hip.dt(wr.TORCH_DT[c.dtype])
        if c.entry == "tn":
            outer, inner = c.batch
            M, Na, Nb = g.M, c.Cout, c.Cin
            self.lda, self.ldb, self.ldo = g.lddy, g.ldx, Nb + 8
            a = torch.full((outer * M + wr.GR, inner, self.lda), wr.GARBAGE, device=DEV).to(d.dy.dtype)
            a[:outer * M, :, :Na] = d.dy.reshape(outer, inner, M, Na).permute(0, 2, 1, 3).reshape(outer * M, inner, Na)
            b = torch.full((outer * inner, M + wr.GR, self.ldb), wr.GARBAGE, device=DEV).to(d.x.dtype)
            b[:, :M, :Nb] = d.x
            self.a, self.b = a, b
            self.need = 0
            return
        self.x = _input(d.x, g.ldx)
        self.dy = _input(d.dy, g.lddy)
        if c.entry == "stem":
            self.need = hip.stem_wgrad_workspace(self.hd, c.N, c.H, c.W, c.Cout)
        else:
            self.need = hip.conv_wgrad_workspace(self.hd, N=c.N, P=g.P, Q=g.Q, Cin=c.Cin, Cout=c.Cout, R=c.R, S=c.S, stride=c.stride,
                                                 pad=c.pad, has_bias=c.bias)

    def launch(self, form):
        """one launch; returns (got for wr.verdict, raw tensors for the bit-identity check)"""
        c, d, g = self.c, self.d, self.g
        if form == "direct":
            outer, inner = c.batch
            M, Na, Nb = g.M, c.Cout, c.Cin
            rows_o = GROWS + Na + GROWS
            out = torch.full((outer * inner, rows_o, self.ldo), SENT, device=DEV, dtype=d.dy.dtype)
            out[:, GROWS:GROWS + Na, :Nb] = float("nan")
            hip.gemm_tn_batched(self.hd, self.a, self.b, out[0, GROWS:], M, Na, Nb, inner * self.lda, self.ldb, self.ldo, outer, inner,
                                (M * inner * self.lda, self.lda), (inner * (M + wr.GR) * self.ldb, (M + wr.GR) * self.ldb),
                                (inner * rows_o * self.ldo, rows_o * self.ldo))
            code = hip.wgrad_last_kernel()
            torch.cuda.synchronize()
            s = torch.full_like(out[:1, :1, :1], SENT)
            past = not (bool((out[:, :GROWS] == s).all()) and bool((out[:, GROWS + Na:] == s).all())
                        and bool((out[:, GROWS:GROWS + Na, Nb:] == s).all()))
            return dict(dw=out[:, GROWS:GROWS + Na, :Nb].double().reshape(-1, Nb), dbias=None, past=past), [_raw(out)], code
        slabs = form in ("slab", "assign")
        work = torch.full((self.need + TAIL,), float("nan"), device=DEV) if slabs else None
        wbuf, woff = _output(d.pre_dw, c.unaligned)
        dw = wbuf[woff:woff + d.pre_dw.numel()]
        bbuf = db = None
        if c.bias:
            bbuf, boff = _output(d.pre_db, c.unaligned)
            db = bbuf[boff:boff + c.Cout]
        ws = work[:self.need] if slabs else None
        if c.entry == "stem":
            hip.stem_wgrad(self.hd, self.dy, self.x, dw, c.N, c.H, c.W, c.Cout, g.lddy, ws)
        else:
            hip.conv_wgrad(self.hd, self.dy, self.x, dw, N=c.N, H=c.H, W=c.W, Cin=c.Cin, ldx=g.ldx, P=g.P, Q=g.Q, Cout=c.Cout,
                           lddy=g.lddy, R=c.R, S=c.S, stride=c.stride, pad=c.pad, dbias=db, workspace=ws, assign=form == "assign")
        code = hip.wgrad_last_kernel()
        torch.cuda.synchronize()
        past = not (bool((wbuf[:woff] == SENT).all()) and bool((wbuf[woff + dw.numel():] == SENT).all()))
        if c.bias:
            past = past or not (bool((bbuf[:boff] == SENT).all()) and bool((bbuf[boff + c.Cout:] == SENT).all()))
        if slabs:
            past = past or not bool(torch.isnan(work[self.need:]).all())
        got = dict(dw=dw.double().reshape(c.Cout, g.Ntot), dbias=db.double() if c.bias else None, past=past)
        return got, [_raw(wbuf)] + ([_raw(bbuf)] if c.bias else []), code


def run_case(c, cus=None):
    """Runs a case in both regimes and every form of its entry.  Returns dict(lines, failures, kernel, reduces, worst): the printed
    figures, what failed (empty: the case passes), the kernel code and reduce paths the query named, the worst positive-regime ratio."""
    cus = cus or cu_count()
    pl = wr.plan(c, cus)
    lines, fails, reduces, worst = [], [], set(), 0.0
    kernel = None
    hip.rowres_reserve_cus(c.reserve)
    try:
        for regime in ("exact", "positive"):
            d = wr.make(c, DEV, regime, seed=11)
            L = Launcher(c, d)
            seen = {}
            for form in ("direct", "direct") if c.entry == "tn" else ("slab",) + wr.forms(c):
                n0 = {k: hip.kernel_launches(v) for k, v in COUNTERS.items()}
                got, raw, code = L.launch(form)
                moved = {k: hip.kernel_launches(v) - n0[k] for k, v in COUNTERS.items()}
                want_moved = {k: int(k == c.kern.family) for k in COUNTERS}
                if moved != want_moved:
                    fails.append(f"{regime} {form}: launch counters moved by {moved}, the case names {c.kern}")
                dec = wr.decode(code)
                kernel = dec["kern"]
                slabs = form in ("slab", "assign")
                want = dict(kern=c.kern.code, slabs=slabs, splits=pl.splits)
                red = (dec["reduce"], dec["assign"], dec["two"])
                want_red = wr.expected_reduce(c, pl, form == "assign") if slabs else (0, False, False)
                if {k: dec[k] for k in want} != want or red != want_red:
                    fails.append(f"{regime} {form}: the query answers {dec}, the case names {want} with the reduce {want_red}")
                elif slabs:
                    reduces.add(red)
                if form in seen:
                    if not all(torch.equal(a, b) for a, b in zip(seen[form], raw)):
                        fails.append(f"{regime} {form}: a second launch differs from the first")
                else:
                    seen[form] = raw
                v = wr.verdict(c, d, regime, form, got, pl)
                for check, (ratio, err, bnd) in v.items():
                    tag = "RATIO" if regime == "positive" and check != "guard" else "CHECK"
                    lines.append(f"{tag} {c.kern} {c.name} {regime} {form} {check} err={err:.3e} bound={bnd:.3e} ratio={ratio:.4f}")
                    if regime == "positive" and check != "guard" and ratio == ratio:
                        worst = max(worst, ratio)
                    if not ratio <= 1.0:
                        fails.append(f"{regime} {form}: {check} err {err:.3e} > bound {bnd:.3e}")
    finally:
        hip.rowres_reserve_cus(0)
    return dict(name=c.name, lines=lines, failures=fails, kernel=kernel, reduces=sorted(reduces), worst=worst, M=wr.geom(c).M)


def _record(c, rep):
    for line in rep["lines"]:
        print(line)
    fam = wr.family_of(c)
    WORST[fam] = max(WORST.get(fam, 0.0), rep["worst"])
    print(f"WORST {fam} {c.name} M={rep['M']} ratio={rep['worst']:.4f}")
    assert not rep["failures"], f"{c.name} ({c.kern}): " + "; ".join(rep["failures"])
    RAN_KERNELS.add(c.kern)
    RAN_REDUCES.update(tuple(r) for r in rep["reduces"])


@pytest.mark.parametrize("case", wr.CASES, ids=lambda c: c.name)
def test_wgrad_kernel_against_float64_reference(case):
    c = wr.resolve(case, cu_count())
    _record(c, run_case(c))


def test_wgrad8p_kernel_in_a_child_process_under_its_switch():
    """NKB_WGRAD256 is read once per process, and only the value 2 routes a launch to wgrad8p_kernel: one fresh child runs the probe
    cases — it finds each one's smallest eligible row count with the launch counter and the query — and prints its verdicts."""
    env = dict(os.environ, NKB_WGRAD256="2")
    r = subprocess.run([sys.executable, str(ROOT / "tests" / "wgrad8p_probe.py")], env=env, capture_output=True, text=True, timeout=300)
    reps = [json.loads(line[len("PROBE "):]) for line in r.stdout.splitlines() if line.startswith("PROBE {")]
    assert r.returncode == 0 and "PROBE OK" in r.stdout and len(reps) == len(wr.PROBE_CASES), (r.stdout[-3000:], r.stderr[-3000:])
    for case, rep in zip(wr.PROBE_CASES, reps):
        assert rep["name"] == case.name and rep["kernel"] == case.kern.code and rep["M"] % 64 == 0 and rep["M"] >= 4096, rep
        assert rep["not_eligible_below"], rep
        _record(wr.resolve(case, found_m=rep["M"]), rep)


def test_every_kernel_and_reduce_path_ran(request):
    """the kernels and reduce paths this session's cases ran are the whole list the dispatch can produce"""
    if request.config.getoption("keyword"):
        pytest.skip("run with a -k selection: not every case ran")
    for fam in wr.FAMILIES:
        print(f"WORST {fam} ratio={WORST.get(fam, float('nan')):.4f}")
    assert RAN_KERNELS == set(wr.KERNELS), sorted(map(str, set(wr.KERNELS) ^ RAN_KERNELS))
    assert RAN_REDUCES >= set(wr.REDUCES), sorted(set(wr.REDUCES) - RAN_REDUCES)
