"""LayerNorm (csrc/transformer.hip) at the token counts of a batch-256 ViT step, bf16: D = 192 (ViT-Tiny: the masked-tail kernels, 48
of 64 lanes active) next to D = 384 (ViT-Small: the full-lane kernels, the unchanged control).  The time of the forward and of the
workspace-form backward with the residual operand (HIP events, median of alternating repetitions; the backward includes its two
small parameter-gradient reduce launches) next to the launch's bytes over the achievable HBM rate, and the outputs against torch's
own LayerNorm on the same operands.
Usage: python scripts/layernorm_check.py [quick] [rows]"""
import os
import sys

import torch
import torch.nn.functional as F

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
sys.path.insert(0, os.path.join(R, "nkb-classification_amd"))
from nkb_classification import hip  # noqa: E402

DEV = torch.device("cuda", 0)
d = hip.BF16
HBM_TBS = 6.0            # achievable HBM rate
EPS = 1e-6


def med(f, reps):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ts = []
    for _ in range(reps):
        ev[0].record(); f(); ev[1].record(); torch.cuda.synchronize()
        ts.append(ev[0].elapsed_time(ev[1]) * 1e3)
    return sorted(ts)[len(ts) // 2]


def run(M, D, reps):
    torch.manual_seed(D)
    x = (torch.randn(M, D, device=DEV) * 1.5 + 0.3).to(torch.bfloat16)
    g = torch.randn(M, D, device=DEV).to(torch.bfloat16)
    add = torch.randn(M, D, device=DEV).to(torch.bfloat16)
    gamma, beta = torch.rand(D, device=DEV) + 0.5, torch.randn(D, device=DEV)
    y, dx = torch.empty_like(x), torch.empty_like(x)
    mean, rstd = torch.empty(M, device=DEV), torch.empty(M, device=DEV)
    dg, db = torch.zeros(D, device=DEV), torch.zeros(D, device=DEV)
    work = torch.empty(hip.layernorm_ws(D), device=DEV)
    fwd = lambda: hip.layernorm_fwd(d, x, D, gamma, beta, y, D, mean, rstd, M, D, EPS)                                   # noqa: E731
    bwd = lambda: hip.layernorm_bwd(d, g, D, x, D, gamma, mean, rstd, add, dx, D, dg, db, M, D, workspace=work)         # noqa: E731
    fwd(); bwd()
    torch.cuda.synchronize()
    xt = x.float().requires_grad_(True)
    gt, bt = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    yt = F.layer_norm(xt, (D,), gt, bt, EPS)
    yt.backward(g.float())
    ok = True
    for name, got, ref, bar in (("y", y, yt, 2e-2), ("dx", dx, xt.grad + add.float(), 2e-2), ("dgamma", dg, gt.grad, 1e-3), ("dbeta", db, bt.grad, 1e-3)):
        err = (got.float() - ref.float()).abs().max().item() / ref.float().abs().max().item()
        ok &= err < bar
    # byte model: forward x in, y out (+ the two statistics); backward dy, x, the residual in, dx out (+ the statistics read back)
    fb, bb = 4.0 * M * D + 8.0 * M, 8.0 * M * D + 8.0 * M
    lanes = min(64, D // 4) if D <= 256 else None
    if reps:
        tf, tb = med(fwd, reps), med(bwd, reps)
        ff, bf = fb / HBM_TBS / 1e6, bb / HBM_TBS / 1e6
        print(f"{M} x {D}  forward {tf:6.1f} us (floor {ff:5.1f} us, x{tf / ff:4.2f})  backward {tb:6.1f} us (floor {bf:5.1f} us, x{tb / bf:4.2f})"
              f"{f'  active lanes {lanes}/64' if lanes else ''}  {'ok' if ok else 'MISMATCH'}", flush=True)
    else:
        print(f"{M} x {D}  {'ok' if ok else 'MISMATCH'}", flush=True)
    return ok


if __name__ == "__main__":
    quick = len(sys.argv) > 1 and sys.argv[1] == "quick"
    rows = int(sys.argv[2]) if len(sys.argv) > 2 else (2048 if quick else 50432)
    allok = True
    for D in (192, 384):
        allok &= run(rows, D, 0 if quick else 9)
    print("ALL OK" if allok else "MISMATCH")
    sys.exit(0 if allok else 1)
