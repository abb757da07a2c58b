"""Fused optimizer step standalone: ms and TB/s for ResNet-50 / ViT-B / ViT-L sized flat ranges.  Bytes per parameter: 30 for the
Adam family (master weight and both moments read + written, gradient read, bf16 shadow written), 22 for SGD with momentum (no second
moment), 14 for plain SGD.  Each figure is the median of --repeats timed windows of --iters launches; min and max show the spread.

  python scripts/optim_bench.py [--n 304000000 ...] [--kinds nadam adam adamw radam sgd sgd_momentum sgd_nesterov] [--iters 50] [--repeats 5]

NKBHIP_LIB selects the library (hip.load).  --against OTHER.so loads a second build of the library into the same process and
alternates the timed windows between the two on the same buffers (other first): run-to-run differences between processes (several
per cent on a shared machine) then drop out of the comparison.  Hand the other build only kinds it knows."""
import argparse, ctypes, os, statistics, sys, torch
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, os.path.join(R, "nkb-classification_amd"))
from nkb_classification import hip
from nkb_classification.utils import _step_scalars
KINDS = {   # name -> (kind for _step_scalars, its keyword arguments, beta1, bytes per parameter, uses v)
    "nadam": ("nadam", {}, 0.9, 30, True), "adam": ("adam", {}, 0.9, 30, True), "adamw": ("adamw", {}, 0.9, 30, True),
    "radam": ("radam", {}, 0.9, 30, True), "radam_decoupled": ("radam", dict(decoupled=True), 0.9, 30, True),
    "sgd": ("sgd", {}, 0.0, 14, True),      # (plain SGD is handed both moments, as FusedOptimizer does; it touches neither)
    "sgd_momentum": ("sgd", dict(momentum=0.9), 0.9, 22, False), "sgd_nesterov": ("sgd", dict(momentum=0.9, nesterov=True), 0.9, 22, False),
}
ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, nargs="+", default=[25_557_032, 86_567_656, 304_000_000])
ap.add_argument("--kinds", nargs="+", default=["nadam", "adam", "sgd"], choices=list(KINDS))
ap.add_argument("--iters", type=int, default=10)
ap.add_argument("--repeats", type=int, default=1)
ap.add_argument("--tag", default="")
ap.add_argument("--against", default=None, metavar="OTHER.so")
args = ap.parse_args()
libs = [("", hip.load())]
if args.against:
    other = ctypes.CDLL(args.against)
    other.nkb_optim_step.restype, other.nkb_optim_step.argtypes = hip._SIGS["nkb_optim_step"]
    libs = [("other ", other), ("this  ", hip.load())]
dev = "cuda"
for n in args.n:
    p, g, m, v = (torch.randn(n, device=dev) * 0.01 for _ in range(4))
    v.abs_()
    sh = torch.empty(n, device=dev, dtype=torch.bfloat16)
    for name in args.kinds:
        kind, kw, beta1, bpp, uses_v = KINDS[name]
        k, sc = _step_scalars(kind, {"step": 9, "momentum_buffer": True}, lr=1e-3, beta1=beta1, beta2=0.999, eps=1e-8, momentum_decay=4e-3, **kw)
        def fn(lib):
            hip.check(lib.nkb_optim_step(k, hip.ptr(p), hip.ptr(g), hip.ptr(m), hip.ptr(v if uses_v else None), hip.ptr(sh), n, 1e-3, 0.01,
                                         beta1, 0.999, 1e-8, 1.0, *sc, None, hip.stream()), "optim_step")
        for _, lib in libs:
            for _ in range(3): fn(lib)
        torch.cuda.synchronize()
        times = {tag: [] for tag, _ in libs}
        for _ in range(args.repeats):
            for tag, lib in libs:
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(args.iters): fn(lib)
                b.record(); torch.cuda.synchronize()
                times[tag].append(a.elapsed_time(b) / args.iters)
        for tag, t in times.items():
            ms = statistics.median(t)
            print(f"{args.tag}{tag}n={n / 1e6:6.1f}M {name:15s}: {ms * 1e3:8.1f} us  [{min(t) * 1e3:.1f} .. {max(t) * 1e3:.1f}]  "
                  f"{n * bpp / ms / 1e9:5.2f} TB/s at {bpp} B/param", flush=True)
    del p, g, m, v, sh
