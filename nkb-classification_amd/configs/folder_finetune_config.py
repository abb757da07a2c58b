# The transformer fine-tuning recipe of folder_mixup_config.py (device input path, Mixup / CutMix, label smoothing, AdamW with
# layer-wise lr decay) plus the two remaining pieces of the DeiT / BEiT / ConvNeXt / DINOv2 recipes:
#   clip_grad  {"max_norm": x} (torch.nn.utils.clip_grad_norm_) or {"clip_value": x} (clip_grad_value_); timm's spelling
#              {"mode": "norm" | "value", "clip_grad": x} is accepted too.  One reduction pass over the gradient arena; the
#              coefficient is derived and applied on the device inside the optimizer launches (no host read-back).
#   model_ema  {"decay": d, "warmup": bool} (ModelEmaV2): one launch per step averages the weight arena.  Validation runs on the
#              averaged weights, best.pth / scripted_best.pt hold them, last.pth keeps the raw weights training resumes from
#              and ema_last.pth the average; eval.py loads either like any checkpoint.
# Point `root` at an ImageFolder tree (root/<class>/<image>).
device = "cuda:0"
enable_mixed_presicion = True      # bf16 compute, fp32 accumulate / statistics / master weights
enable_gradient_scaler = False     # bf16 needs no loss scaling
compile = False
log_gradients = False
show_full_current_loss_in_terminal = False
task = "single"
n_epochs = 2
backbone_state_policy = {0: "unfreeze"}
img_size = 224
mean, std = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
train_data = {
    "root": "data/train", "size": img_size, "batch_size": 64, "shuffle": True, "num_workers": 8, "drop_last": True,
    "device_pipeline": True, "device": device, "seed": 0, "mean": mean, "std": std, "fill": 0,
    "hflip_p": 0.5,
    "mixup": {"mixup_alpha": 0.8, "cutmix_alpha": 1.0, "prob": 1.0, "switch_prob": 0.5, "mode": "batch"},
}
val_data = {"root": "data/val", "size": img_size, "batch_size": 64, "shuffle": False, "num_workers": 8,
            "device_pipeline": True, "device": device, "mean": mean, "std": std, "fill": 0}
train_pipeline = None
val_pipeline = None
model = {"task": task, "model": "deit_small_patch16_224", "pretrained": False, "backbone_dropout": 0.0, "classifier_dropout": 0.0,
         "classifier_initialization": "kaiming_normal_"}
optimizer = {"type": "adamw", "lr": 5e-4, "weight_decay": 0.05, "backbone_lr": 5e-4, "backbone_weight_decay": 0.05,
             "classifier_lr": 5e-4, "classifier_weight_decay": 0.05, "layer_decay": 0.75}
lr_policy = {"type": "cosine", "n_epochs": n_epochs}
criterion = {"task": task, "type": "CrossEntropyLoss", "label_smoothing": 0.1}
clip_grad = {"max_norm": 1.0}
model_ema = {"decay": 0.9998, "warmup": True}
experiment = {"comet": None, "local": {"path": "runs/folder_finetune"}}
