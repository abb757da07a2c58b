# The reference's single-task training stack (configs/singletask_config.py:162-219) on the device input path:
#   LongestMaxSize -> PadIfNeeded -> HorizontalFlip -> VerticalFlip -> RandomBrightnessContrast -> HueSaturationValue ->
#   CoarseDropout -> Normalize -> ToTensorV2
# expressed in the `data` keys of get_dataset(device_pipeline=True): decode + LongestMaxSize on the host workers, uint8 H2D one
# batch ahead, everything after it in one launch of nkb_image_prep.  The three augmentation dicts take albumentations' argument
# names plus `p`.  An albumentations Compose in `train_pipeline` is translated into the same keys (explicit keys win), so a
# reference config can keep its pipeline and add only `device_pipeline` / `device` to its data dicts.
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
img_size = 128
mean, std = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
train_data = {
    "root": "data/train", "size": img_size, "batch_size": 64, "shuffle": True, "num_workers": 8, "drop_last": True,
    "device_pipeline": True, "device": device, "seed": 0, "mean": mean, "std": std,
    "fill": 0,                     # PadIfNeeded(border_mode=cv2.BORDER_CONSTANT, value=0)
    "hflip_p": 0.5,                # HorizontalFlip(p=0.5)
    "vflip_p": 0.5,                # VerticalFlip(p=0.5)
    "brightness_contrast": {"brightness_limit": (-0.2, 0.2), "contrast_limit": (0.1, -0.5), "p": 0.5},
    "hue_saturation_value": {"hue_shift_limit": 0, "sat_shift_limit": 10, "val_shift_limit": 50, "p": 0.5},
    "coarse_dropout": {"max_holes": 4, "min_holes": 1, "max_height": 0.2, "min_height": 0.05, "max_width": 0.2,
                       "min_width": 0.05, "fill_value": [0, 0.5, 1], "p": 0.5},
}
val_data = {"root": "data/val", "size": img_size, "batch_size": 64, "shuffle": False, "num_workers": 8,
            "device_pipeline": True, "device": device, "mean": mean, "std": std, "fill": 0}
train_pipeline = None
val_pipeline = None
model = {"task": task, "model": "resnet50", "pretrained": False, "backbone_dropout": 0.0, "classifier_dropout": 0.0,
         "classifier_initialization": "kaiming_normal_"}
optimizer = {"type": "nadam", "lr": 1e-4, "weight_decay": 0.2, "backbone_lr": 1e-4, "backbone_weight_decay": 0.01,
             "classifier_lr": 1e-3, "classifier_weight_decay": 0.2}
lr_policy = {"type": "cosine", "n_epochs": n_epochs}
criterion = {"task": task, "type": "CrossEntropyLoss"}
experiment = {"comet": None, "local": {"path": "runs/folder_device_pipeline"}}
