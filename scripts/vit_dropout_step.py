"""One ViT train step with backbone dropout on, timed: vit_base_patch16_224, batch 256, bf16, backbone_dropout = 0.1 (the value of
the sample configs), model / optimizer / loss as bench.py builds them.  Prints one JSON line: ms per step (median and min .. max over
ROUNDS blocks of STEPS steps), peak allocated memory, and which attention path the engine took.
Usage: python scripts/vit_dropout_step.py [--dropout 0.1] [--batch 256] [--model vit_base_patch16_224]
       NKB_FUSED_ATTN=0 python scripts/vit_dropout_step.py      (the materialised attention path)"""
import argparse, json, os, statistics, sys, time, torch
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, os.path.join(R, "nkb-classification_amd"))
from nkb_classification.losses import get_loss
from nkb_classification.model import get_model
from nkb_classification.utils import get_optimizer

ap = argparse.ArgumentParser()
ap.add_argument("--dropout", type=float, default=0.1)
ap.add_argument("--batch", type=int, default=256)
ap.add_argument("--model", default="vit_base_patch16_224")
ap.add_argument("--steps", type=int, default=10)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--warmup", type=int, default=6)
args = ap.parse_args()
dev = "cuda:0"
torch.manual_seed(0)
cfg = dict(task="single", model=args.model, pretrained=False, backbone_dropout=args.dropout, classifier_dropout=0.0,
           classifier_initialization="kaiming_normal_")
model = get_model(cfg, [str(i) for i in range(1000)], dev)
opt = get_optimizer(model, dict(type="nadam", lr=1e-4, backbone_lr=1e-5, classifier_lr=1e-4, weight_decay=0.01,
                                backbone_weight_decay=0.01, classifier_weight_decay=0.2))
crit = get_loss(dict(task="single", type="CrossEntropyLoss"), dev)
x = torch.randn(args.batch, 3, 224, 224, device=dev)
y = torch.randint(0, 1000, (args.batch,), device=dev)
model.train()


def step():
    opt.zero_grad()
    with torch.autocast("cuda", dtype=torch.bfloat16):
        loss = crit(model(x), y)
    loss.backward()
    opt.step()
    return loss


for _ in range(args.warmup):
    step()
torch.cuda.synchronize()
blocks = []
for _ in range(args.rounds):
    t0 = time.perf_counter()
    for _ in range(args.steps):
        loss = step()
    torch.cuda.synchronize()
    blocks.append((time.perf_counter() - t0) / args.steps * 1e3)
eng = model._engines[torch.bfloat16]
site = next((v for k, v in eng.saved.items() if k.endswith(".attn")), {})
print(json.dumps(dict(model=args.model, batch=args.batch, backbone_dropout=args.dropout, ms_per_step=round(statistics.median(blocks), 3),
                      ms_min=round(min(blocks), 3), ms_max=round(max(blocks), 3), loss=round(loss.item(), 4),
                      peak_allocated_mib=round(torch.cuda.max_memory_allocated() / 2 ** 20),
                      workspace_mib=round(eng.ws.nbytes() / 2 ** 20), attention="fused" if site.get("fused") else "materialised")))
