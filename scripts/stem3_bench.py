"""Per-kernel times of the ResNet-D/T device code at the bench's size (batch 256, 224 x 224 images -> 112 x 112 stem maps): the two
narrow forwards, the two narrow data gradients (csrc/stem3.hip), the three stem weight gradients (generic nkb_conv_wgrad) and the 2x2
average pools of the three stride-2 shortcuts, each against its byte floor (bytes from the shapes over 6.3 TB/s).
Usage: python scripts/stem3_bench.py [--iters 10] [--stem 24,32]    (under `rocprofv3 --kernel-trace --stats -- python ...` the launches
appear in this order, `iters` + 2 times each)"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "nkb-classification_amd"))
from nkb_classification import hip  # noqa: E402

HBM = 6.3e12


def timed(name, fn, iters, nbytes, flops=0.0):
    fn(); fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    us = a.elapsed_time(b) * 1e3 / iters
    floor = nbytes / HBM * 1e6
    print(f"{name:34s} {us:9.1f} us   floor {floor:7.1f} us   x{us / floor:5.1f}   {nbytes / us / 1e6:6.2f} TB/s"
          + (f"   {flops / us / 1e6:7.1f} TFLOP/s" if flops else ""), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--stem", default="24,32")
    args = ap.parse_args()
    c1, c2 = (int(v) for v in args.stem.split(","))
    N, H, W, dev, T, d = args.batch, 112, 112, "cuda", torch.bfloat16, hip.BF16
    M = N * H * W
    act = {c: torch.randn(N, H, W, c, device=dev).to(T) for c in {c1, c2, 64}}
    out = {c: torch.empty(N, H, W, c, device=dev, dtype=T) for c in {c1, c2, 64}}
    for ci, co in ((c1, c2), (c2, 64)):
        w = (torch.randn(co, 3, 3, ci, device=dev) / (3 * ci ** 0.5)).to(T)
        tiles = hip.stem3_tiles(d, N, H, W, ci, co)
        st = torch.empty(hip.bn_stats_floats(tiles, co), device=dev)
        timed(f"stem3 fwd {ci}->{co} (+stats)", lambda: hip.stem3_conv(d, act[ci], w, out[co], N=N, H=H, W=W, Cin=ci, ldx=ci, Cout=co,
                                                                     ldy=co, stats=st, tiles=tiles), args.iters, 2.0 * M * (ci + co),
              2.0 * M * 9 * ci * co)
    for ci, co in ((64, c2), (c2, c1)):
        w = (torch.randn(co, 3, 3, ci, device=dev) / (3 * ci ** 0.5)).to(T)
        timed(f"stem3 dgrad {ci}->{co}", lambda: hip.stem3_conv(d, act[ci], w, out[co], N=N, H=H, W=W, Cin=ci, ldx=ci, Cout=co, ldy=co,
                                                              dgrad=True), args.iters, 2.0 * M * (ci + co), 2.0 * M * 9 * ci * co)
    col = torch.randn(M, 64, device=dev).to(T)
    for name, x, geom, shape in (
            (f"wgrad stem0 im2row 64->{c1}", col, dict(N=M, H=1, W=1, Cin=64, ldx=64, P=1, Q=1, Cout=c1, lddy=c1), (c1, 64)),
            (f"wgrad stem1 3x3 {c1}->{c2}", act[c1], dict(N=N, H=H, W=W, Cin=c1, ldx=c1, P=H, Q=W, Cout=c2, lddy=c2, R=3, S=3, stride=1, pad=1),
             (c2, 3, 3, c1)),
            (f"wgrad stem 3x3 {c2}->64", act[c2], dict(N=N, H=H, W=W, Cin=c2, ldx=c2, P=H, Q=W, Cout=64, lddy=64, R=3, S=3, stride=1, pad=1),
             (64, 3, 3, c2))):
        co = geom["Cout"]
        need = hip.conv_wgrad_workspace(d, N=geom["N"], P=geom["P"], Q=geom["Q"], Cin=geom["Cin"], Cout=co, R=geom.get("R", 1),
                                        S=geom.get("S", 1), stride=geom.get("stride", 1), pad=geom.get("pad", 0))
        work = torch.empty(max(need, 1), device=dev)
        dw = torch.zeros(shape, device=dev)
        timed(name, lambda: hip.conv_wgrad(d, act[co], x, dw, workspace=work, **geom), args.iters, 2.0 * M * (geom["Cin"] + co),
              2.0 * M * co * dw[0].numel())
    for h, c in ((56, 256), (28, 512), (14, 1024)):
        x = torch.randn(N, h, h, c, device=dev).to(T)
        y = torch.empty(N, h // 2, h // 2, c, device=dev, dtype=T)
        dx = torch.empty_like(x)
        nb = 2.0 * (x.numel() + y.numel())
        timed(f"avgpool2x2 fwd {h}x{h}x{c}", lambda: hip.avgpool2x2(d, False, x, y, N, h, h, c), args.iters, nb)
        timed(f"avgpool2x2 bwd {h}x{h}x{c}", lambda: hip.avgpool2x2(d, True, y, dx, N, h, h, c), args.iters, nb)


if __name__ == "__main__":
    main()
