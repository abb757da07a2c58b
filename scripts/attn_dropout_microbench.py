"""Attention with dropout, standalone timing (ViT-B/16: B=256, T=197, H=12; unicom L/14 extents: B=128, T=256, H=16; bf16, dh=64):
the fused forward and fused backward kernel at p = 0 and p = 0.1 (the DROP flavour regenerates nkb_dropout's mask), next to the
materialised sequence at p = 0.1 (HipEngine with fused_attention off: score GEMM, softmax, dropout, P V GEMM; backward: five batched
GEMMs, mask re-applied, softmax backward).  The variants alternate over ROUNDS rounds; each line gives the median and the spread
(min .. max) of the per-round means, in microseconds.
Usage: python scripts/attn_dropout_microbench.py [--p0-only]     (--p0-only: the p = 0 kernels alone, through the binding's
positional arguments only, so the same file also times a library and binding from before the dropout arguments existed)"""
import os, statistics, sys, torch
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, os.path.join(R, "nkb-classification_amd"))
from nkb_classification import hip
dev, ROUNDS, P = "cuda", 7, 0.1
P0_ONLY = "--p0-only" in sys.argv


def timeit(fn, n=20):
    for _ in range(3): fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n): fn()
    b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b) / n * 1e3


for (B, T, H) in [(256, 197, 12), (128, 256, 16)]:
    dh = 64; D = H * dh; Tp = (T + 63) // 64 * 64
    qkv = (torch.randn(B * T, 3 * D, device=dev) * 0.5).to(torch.bfloat16)
    o = torch.empty(B * T, D, device=dev, dtype=torch.bfloat16); lse = torch.empty(B * H, T, device=dev)
    do = torch.randn(B * T, D, device=dev).to(torch.bfloat16); dqkv = torch.empty_like(qkv)
    seed = torch.zeros(1, dtype=torch.int64, device=dev)
    variants = {
        "fwd p=0": lambda: hip.attn_forward(hip.BF16, qkv, o, lse, B, T, H, dh, dh ** -0.5),
        "bwd p=0": lambda: hip.attn_backward(hip.BF16, qkv, do, o, lse, dqkv, B, T, H, dh, dh ** -0.5),
    }
    if not P0_ONLY:
        from nkb_classification.hipnet import HipEngine
        from nkb_classification.runtime import ParamArena
        eng = HipEngine(ParamArena(), torch.device(dev), torch.bfloat16)
        eng.fused_attention = False
        variants.update({
            "fwd p=%g" % P: lambda: hip.attn_forward(hip.BF16, qkv, o, lse, B, T, H, dh, dh ** -0.5, drop_p=P, seed=12345, drop_ld=Tp, seed_out=seed),
            "bwd p=%g" % P: lambda: hip.attn_backward(hip.BF16, qkv, do, o, lse, dqkv, B, T, H, dh, dh ** -0.5, drop_p=P, seed_dev=seed, drop_ld=Tp),
            "materialised fwd p=%g" % P: lambda: eng.attention("a", qkv, B, T, H, True, drop_p=P),
            "materialised bwd p=%g" % P: lambda: eng.attention_backward("a", do, "dqkv"),
        })
    times = {k: [] for k in variants}
    for _ in range(ROUNDS):
        for k, fn in variants.items():
            times[k].append(timeit(fn))
    for k, v in times.items():
        print(f"B={B} T={T} H={H} {k:26s} median {statistics.median(v):8.1f} us  spread {min(v):8.1f} .. {max(v):8.1f}")
    if not P0_ONLY:
        print(f"B={B} T={T} H={H} workspace of the materialised path: {eng.ws.nbytes() / 2 ** 20:.0f} MiB")
