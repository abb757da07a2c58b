# A transformer fine-tuning recipe on the device input path: Mixup / CutMix and label smoothing (the DeiT / ConvNeXt recipes),
# AdamW with layer-wise lr decay.  `mixup` takes timm.data.Mixup's argument names (mixup_alpha, cutmix_alpha, prob, switch_prob,
# mode = "batch" | "pair" | "elem"); the images are mixed inside the one launch of nkb_image_prep that turns the uint8 batch into
# the fp32 tensor, and the labels of a mixed batch reach the criterion as a losses.MixedTarget (y, the partner's y2, lam per
# row).  Label smoothing belongs to the criterion (`label_smoothing`), not to `mixup`.  Validation is neither mixed nor — as in
# torch — exempt from the smoothing of the shared criterion.
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
experiment = {"comet": None, "local": {"path": "runs/folder_mixup"}}
