"""Depthwise 7x7 convolution (csrc/dwconv.hip) at the four convnext_base shapes, batch 256, bf16: the time of each pass (HIP events,
median of alternating repetitions) next to its two floors — the launch's bytes over the achievable HBM rate and its FLOPs over the
fp32 vector peak — and next to torch's own bf16 channels-last depthwise conv2d forward / backward on the same operands (the
yardstick; torch's backward is data + weight + bias gradient in one call).  Also checks the outputs against torch's.
Usage: python scripts/dwconv_check.py [quick] [batch]"""
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
HBM_TBS = 6.0            # achievable HBM rate (a table swept in order)
VEC_TFLOPS = 157.3       # fp32 vector peak: 64 FLOP/clk/SIMD x 1024 SIMDs x 2.4 GHz (packed FMA; 78.6 with scalar v_fma_f32)


def med(f, reps):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ts = []
    for _ in range(reps):
        ev[0].record(); f(); ev[1].record(); torch.cuda.synchronize()
        ts.append(ev[0].elapsed_time(ev[1]) * 1e3)
    return sorted(ts)[len(ts) // 2]


def run(N, H, W, C, reps):
    torch.manual_seed(C + H)
    x = torch.randn(N, H, W, C, device=DEV).to(torch.bfloat16)
    g = torch.randn(N, H, W, C, device=DEV).to(torch.bfloat16)
    w = torch.randn(C, 49, device=DEV) * 0.1
    b = torch.randn(C, device=DEV)
    y, dx = torch.empty_like(x), torch.empty_like(x)
    dw, db = torch.zeros(C, 49, device=DEV), torch.zeros(C, device=DEV)
    work = torch.empty(hip.dwconv_wgrad_workspace(d, N, H, W, C), device=DEV)
    geom = dict(N=N, H=H, W=W, C=C, ldx=C, ldy=C)
    fwd = lambda: hip.dwconv(d, x, w, b, y, **geom)                                            # noqa: E731
    dgr = lambda: hip.dwconv(d, g, w, None, dx, dgrad=True, **geom)                            # noqa: E731
    wgr = lambda: hip.dwconv_wgrad(d, g, x, dw, db, N=N, H=H, W=W, C=C, ldg=C, ldx=C, workspace=work)   # noqa: E731
    # the yardstick: torch's bf16 channels-last depthwise convolution on the same values
    xt = x.permute(0, 3, 1, 2).detach().requires_grad_(True)                                   # NCHW view of NHWC memory = channels_last
    wt = w.view(C, 1, 7, 7).to(torch.bfloat16).requires_grad_(True)
    bt = b.to(torch.bfloat16).requires_grad_(True)
    gt = g.permute(0, 3, 1, 2)
    tf = lambda: F.conv2d(xt, wt, bt, padding=3, groups=C)                                     # noqa: E731
    yt = tf()

    def tb():
        xt.grad = wt.grad = bt.grad = None
        yt.backward(gt, retain_graph=True)
    fwd(); dgr(); wgr(); tb()
    torch.cuda.synchronize()
    ok = True
    for name, got, ref in (("y", y, yt.permute(0, 2, 3, 1)), ("dx", dx, xt.grad.permute(0, 2, 3, 1)), ("dw", dw, wt.grad.reshape(C, 49)),
                           ("db", db, bt.grad)):
        err = (got.float() - ref.float()).abs().max().item() / ref.float().abs().max().item()
        ok &= err < 3e-2                                                                        # (torch rounds w, b, dw, db to bf16)
    px = N * H * W * C
    # the byte model of the launches' own profiler scopes (csrc/dwconv.hip): both activations once + the fp32 filter and bias; the
    # weight gradient also writes its per-wave slabs (the ordered reduce that reads them back is a launch of its own)
    flop, byts, wbyts = 2.0 * 49 * px, 4.0 * px + 200.0 * C, 4.0 * px + 4.0 * work.numel()
    floors = (f"floors: HBM {byts / HBM_TBS / 1e6:6.1f} us (weight gradient {wbyts / HBM_TBS / 1e6:6.1f}), "
              f"fp32 vector {flop / VEC_TFLOPS / 1e6:6.1f} us")
    if reps:
        t = [med(f, reps) for f in (fwd, dgr, wgr, tf, tb)]
        print(f"C={C:4d} {H:2d}x{W:<2d} N={N:3d}  forward {t[0]:7.1f} us  data gradient {t[1]:7.1f} us  weight+bias gradient {t[2]:7.1f} us  "
              f"({floors})   torch bf16 channels-last: forward {t[3]:7.1f} us, backward (all three) {t[4]:7.1f} us   "
              f"{'ok' if ok else 'MISMATCH'}", flush=True)
    else:
        print(f"C={C:4d} {H:2d}x{W:<2d} N={N:3d}  {'ok' if ok else 'MISMATCH'}", flush=True)
    return ok


if __name__ == "__main__":
    quick = len(sys.argv) > 1 and sys.argv[1] == "quick"
    batch = int(sys.argv[2]) if len(sys.argv) > 2 else (8 if quick else 256)
    allok = True
    for C, H in ((128, 56), (256, 28), (512, 14), (1024, 7)):
        allok &= run(batch, H, H, C, 0 if quick else 9)
    print("ALL OK" if allok else "MISMATCH")
    sys.exit(0 if allok else 1)
