"""Child process of tests/test_wgrad_gpu.py under NKB_WGRAD256=2 (read once per process: the only value that routes a weight gradient
to wgrad8p_kernel of csrc/wgrad256.hip).  For every case of wgrad_reference.PROBE_CASES it finds the smallest eligible row count (a
multiple of 64, >= 4096) with the wgrad8p launch counter and nkb_wgrad_last_kernel — not by restating the eligibility rule —, runs
the case the way the parent runs its own (both regimes, every form), and prints one line `PROBE {json}`; `PROBE OK` at the end."""
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
for p in (ROOT, ROOT / "nkb-classification_amd", ROOT / "tests"):
    sys.path.insert(0, str(p))

import torch  # noqa: E402

import test_wgrad_gpu as tg  # noqa: E402
import wgrad_reference as wr  # noqa: E402
from nkb_classification import hip  # noqa: E402

MAX_M = 1 << 16


def takes_wgrad8p(c, M, x, dy, dw):
    """one atomic-form launch at M rows: did it go to wgrad8p_kernel?"""
    n0 = hip.kernel_launches("wgrad8p")
    hip.conv_wgrad(hip.BF16, dy, x, dw, N=M, H=1, W=1, Cin=c.Cin, ldx=x.shape[1], P=1, Q=1, Cout=c.Cout, lddy=dy.shape[1])
    took = wr.decode(hip.wgrad_last_kernel())["kern"] == c.kern.code
    torch.cuda.synchronize()
    assert took == (hip.kernel_launches("wgrad8p") == n0 + 1), "the launch counter and the query disagree"
    return took


def smallest_eligible_m(c):
    """doubling, then bisection over the multiples of 64 (the rule is monotone in M: longer inputs only add stages per split); the row
    count below the answer is launched once more and must not be eligible"""
    g = wr.geom(c)
    x = torch.zeros(MAX_M, g.ldx, device=tg.DEV, dtype=torch.bfloat16)
    dy = torch.zeros(MAX_M, g.lddy, device=tg.DEV, dtype=torch.bfloat16)
    dw = torch.zeros(c.Cout, c.Cin, device=tg.DEV)
    hi = 4096
    while not takes_wgrad8p(c, hi, x, dy, dw):
        hi *= 2
        assert hi <= MAX_M, f"{c.name}: no eligible row count up to {MAX_M}"
    lo = hi // 2 if hi > 4096 else 4096 - 64         # lo: not eligible (or below the floor)
    while hi - lo > 64:
        mid = (lo + hi) // 2 // 64 * 64
        if takes_wgrad8p(c, mid, x, dy, dw):
            hi = mid
        else:
            lo = mid
    below = hi == 4096 or not takes_wgrad8p(c, hi - 64, x, dy, dw)
    return hi, below


def main():
    assert torch.cuda.is_available()
    for case in wr.PROBE_CASES:
        M, below = smallest_eligible_m(case)
        rep = tg.run_case(wr.resolve(case, found_m=M))
        rep["not_eligible_below"] = below
        print("PROBE " + json.dumps(rep), flush=True)
    print("PROBE OK")


if __name__ == "__main__":
    main()
