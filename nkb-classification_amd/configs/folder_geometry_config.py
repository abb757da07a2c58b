# The stack most of the reference's archived configs share, on the device input path:
#   LongestMaxSize -> PadIfNeeded(border_mode=cv2.BORDER_REFLECT_101) -> Resize(same size) -> MotionBlur(blur_limit=3,
#   allow_shifted=True, p=0.5) -> RandomBrightnessContrast -> Normalize -> ToTensorV2
# expressed in the `data` keys of get_dataset(device_pipeline=True): decode + LongestMaxSize on the host workers, uint8 H2D one
# batch ahead, everything after it in one launch of nkb_image_prep.  `pad_border` is PadIfNeeded's border ("constant" pads with
# `fill`, "reflect_101" mirrors the image without repeating its edge pixel); `motion_blur` takes albumentations' argument names
# plus `p`; the Resize onto the stack's own size is a no-op and has no key.  An albumentations Compose in `train_pipeline` is
# translated into the same keys (explicit keys win).
#
# The timm-style recipe (RandomResizedCrop + flip + Mixup / CutMix, label smoothing in the criterion) on the same path: the host
# resizes the longest side to `source_size`, the device cuts every crop from that canvas and resamples it to `size`:
#   train_data = {..., "size": 224, "source_size": 288, "pad_border": "constant", "hflip_p": 0.5,
#                 "random_resized_crop": {"scale": (0.08, 1.0), "ratio": (3 / 4, 4 / 3), "p": 1.0},
#                 "mixup": {"mixup_alpha": 0.8, "cutmix_alpha": 1.0, "prob": 1.0, "switch_prob": 0.5, "mode": "batch"}}
#   criterion = {"task": task, "type": "CrossEntropyLoss", "label_smoothing": 0.1}
# (`source_size` > `size` needs random_resized_crop with p = 1; validation keeps source_size = size.)
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
    "device_pipeline": True, "device": device, "seed": 0, "mean": mean, "std": std,
    "pad_border": "reflect_101",   # PadIfNeeded(border_mode=cv2.BORDER_REFLECT_101)
    "motion_blur": {"blur_limit": (3, 3), "allow_shifted": True, "p": 0.5},
    "brightness_contrast": {"brightness_limit": 0.2, "contrast_limit": 0.2, "p": 0.5},
}
val_data = {"root": "data/val", "size": img_size, "batch_size": 64, "shuffle": False, "num_workers": 8,
            "device_pipeline": True, "device": device, "mean": mean, "std": std, "pad_border": "reflect_101"}
train_pipeline = None
val_pipeline = None
model = {"task": task, "model": "resnet50", "pretrained": False, "backbone_dropout": 0.0, "classifier_dropout": 0.0,
         "classifier_initialization": "kaiming_normal_"}
optimizer = {"type": "nadam", "lr": 1e-4, "weight_decay": 0.2, "backbone_lr": 1e-4, "backbone_weight_decay": 0.01,
             "classifier_lr": 1e-3, "classifier_weight_decay": 0.2}
lr_policy = {"type": "cosine", "n_epochs": n_epochs}
criterion = {"task": task, "type": "CrossEntropyLoss"}
experiment = {"comet": None, "local": {"path": "runs/folder_geometry"}}
