"""MI355X-native mirror of the reference's `data/transforms.py` (reference data/transforms.py:100-207).  The reference
runs its chain per sample on the host (numpy / cv2) inside DataLoader workers; here the raw uint8 data stays in HBM and
HIP passes (csrc/data_ops.hip) produce the normalised float tensors `Trainer.update_*` consumes:

  * `c3d_bcd_preprocess` / `c3d_scd_label_preprocess` / `c3d_bda_label_preprocess` behind the `Device*BatchTransform`
    classes: random_flip -> random_exchange -> normalize -> to_tensor over a raw batch the caller hands in (the synthetic
    loaders of the script mirrors);
  * `c3d_augment_gather` behind `resident.DeviceAugmentLoader`: the whole training recipe normalize -> scale ->
    random_crop_resize -> random_flip -> random_exchange -> to_tensor, gathered from a resident file data set
    (`resident.ResidentStore`), driven by the per-epoch table `draw_augmentation_table` draws and
    `validate_augment_table` checks on the host before it is uploaded.

Nothing runs on the host per step.  The aspect-preserving `resize` of the reference is used by none of its pipelines and
has no mirror.

`BCDTransforms.DEFAULT_MEAN/STD` and `IMAGENET_MEAN/STD` are the reference's constants."""
import numpy as np
import torch

from .. import ops


class BCDTransforms:
    DEFAULT_MEAN = [0.5, 0.5, 0.5, 0.5, 0.5, 0.5]
    DEFAULT_STD = [0.5, 0.5, 0.5, 0.5, 0.5, 0.5]
    IMAGENET_MEAN = [0.406, 0.456, 0.485, 0.406, 0.456, 0.485]
    IMAGENET_STD = [0.225, 0.224, 0.229, 0.225, 0.224, 0.229]


def draw_augmentation_flags(batch, rng, train=True):
    """Per-sample (flip0, flip1, exchange) decisions, each with probability 0.5 as in the reference's
    random_flip / random_exchange (data/transforms.py:100-124); all zero for the validation transform."""
    if not train:
        return np.zeros((batch, 3), dtype=np.uint8)
    return (rng.random((batch, 3)) < 0.5).astype(np.uint8)


AUG_COLUMNS = ("index", "do_crop", "x1", "y1", "flip0", "flip1", "exchange", "reserved")


def crop_area_of(in_width):
    """reference data/transforms.py:185: `int(7.0 / 224.0 * args.in_width)`."""
    return int(7.0 / 224.0 * in_width)


def draw_augmentation_table(indices, rng, crop_area, train=True):
    """int32 [len(indices), 8] = (index, do_crop, x1, y1, flip0, flip1, exchange, 0) for `c3d_augment_gather`, drawn with a
    numpy Generator as the reference's random_crop_resize / random_flip / random_exchange draw per sample
    (data/transforms.py:79-124): p = 0.5 for the crop with x1, y1 uniform on [0, crop_area] INCLUSIVE (`random.randint`),
    p = 0.5 for each flip and for the exchange.  The validation transform draws nothing: only the index column is set."""
    indices = np.asarray(indices, dtype=np.int64).reshape(-1)
    table = np.zeros((len(indices), 8), dtype=np.int32)
    table[:, 0] = indices
    if train and len(indices):
        n = len(indices)
        table[:, 1] = rng.random(n) < 0.5
        table[:, 2] = rng.integers(0, crop_area + 1, size=n)
        table[:, 3] = rng.integers(0, crop_area + 1, size=n)
        table[:, 2:4] *= table[:, 1:2]                   # offsets only where the crop fires
        table[:, 4:7] = rng.random((n, 3)) < 0.5
    return table


def validate_augment_table(table, n_store, height, width):
    """Host-side check of a table BEFORE it is uploaded (the kernel cannot refuse device data; it only clamps): int32
    [B, 8], 0 <= index < n_store, 0 <= x1 with 2 * x1 < width, 0 <= y1 with 2 * y1 < height, flags in {0, 1}."""
    table = np.asarray(table)
    if table.dtype != np.int32 or table.ndim != 2 or table.shape[1] != 8:
        raise ValueError(f"augmentation table must be int32 [B, 8], got {table.dtype} {table.shape}")
    if len(table) == 0:
        return table
    if table[:, 0].min() < 0 or table[:, 0].max() >= n_store:
        raise ValueError(f"augmentation table index out of range [0, {n_store}): "
                         f"min {int(table[:, 0].min())}, max {int(table[:, 0].max())}")
    if table[:, 2].min() < 0 or 2 * int(table[:, 2].max()) >= width:
        raise ValueError(f"crop offset x1 must satisfy 0 <= x1 and 2 * x1 < {width}: got {int(table[:, 2].min())}..{int(table[:, 2].max())}")
    if table[:, 3].min() < 0 or 2 * int(table[:, 3].max()) >= height:
        raise ValueError(f"crop offset y1 must satisfy 0 <= y1 and 2 * y1 < {height}: got {int(table[:, 3].min())}..{int(table[:, 3].max())}")
    flags = table[:, [1, 4, 5, 6]]
    if flags.min() < 0 or flags.max() > 1:
        raise ValueError("do_crop / flip0 / flip1 / exchange must be 0 or 1")
    return table


class DeviceBatchTransform:
    """`(image6 u8 [B,H,W,6], label u8 [B,H,W], flags u8 [B,3]) -> (pre, post, label)` float tensors on the GPU."""

    def __init__(self, device, mean=BCDTransforms.DEFAULT_MEAN, std=BCDTransforms.DEFAULT_STD):
        self.device = torch.device(device)
        self.mean = torch.tensor(mean, dtype=torch.float32, device=self.device)
        self.std = torch.tensor(std, dtype=torch.float32, device=self.device)

    def __call__(self, image6, label=None, flags=None):
        image6 = torch.as_tensor(image6).to(self.device, non_blocking=True).contiguous()
        ops.require_gpu(image6, "raw image batch")
        if image6.dtype != torch.uint8 or image6.dim() != 4 or image6.shape[-1] != 6:
            raise ValueError("image6 must be uint8 [B, H, W, 6] (pre RGB | post RGB)")
        B, H, W, _ = image6.shape
        if label is not None:
            label = torch.as_tensor(label).to(self.device, non_blocking=True).contiguous()
            if label.dtype != torch.uint8 or tuple(label.shape) != (B, H, W):
                raise ValueError("label must be uint8 [B, H, W]")
        if flags is not None:
            flags = torch.as_tensor(flags).to(self.device, non_blocking=True).contiguous()
            if flags.dtype != torch.uint8 or tuple(flags.shape) != (B, 3):
                raise ValueError("flags must be uint8 [B, 3]")
        pre = torch.empty((B, 3, H, W), dtype=torch.float32, device=self.device)
        post = torch.empty_like(pre)
        lab = torch.empty((B, 1, H, W), dtype=torch.float32, device=self.device) if label is not None else None
        ops.bcd_preprocess(image6, label, flags, self.mean, self.std, pre, post, lab, B, H, W)
        return pre, post, lab


class SCDTransforms(BCDTransforms):
    """reference data/transforms.py:210-224: same normalisation constants as BCDTransforms."""


class DeviceSCDBatchTransform:
    """`(image6 u8 [B,H,W,6], label3 u8 [B,H,W,3], flags u8 [B,3]) -> (pre, post f32 [B,3,H,W], labels int64 [B,3,H,W])`
    on the GPU: the tensor side of reference SCDTransforms (data/transforms.py:300-357: random_flip, random_exchange --
    which also swaps the two class maps --, normalize, to_tensor) and the `.long()` of scripts/train_SCD.py:207-213.
    The image runs through the BCD pass (identical arithmetic), the labels through `c3d_scd_label_preprocess`."""

    def __init__(self, device, mean=SCDTransforms.DEFAULT_MEAN, std=SCDTransforms.DEFAULT_STD):
        self.image = DeviceBatchTransform(device, mean, std)
        self.device = self.image.device

    def __call__(self, image6, label3, flags=None):
        label3 = torch.as_tensor(label3).to(self.device, non_blocking=True).contiguous()
        B, H, W = label3.shape[:3]
        if label3.dtype != torch.uint8 or label3.dim() != 4 or label3.shape[-1] != 3:
            raise ValueError("label3 must be uint8 [B, H, W, 3] (pre classes, post classes, change)")
        if flags is not None:
            flags = torch.as_tensor(flags).to(self.device, non_blocking=True).contiguous()
        pre, post, _ = self.image(image6, None, flags)
        labels = torch.empty((B, 3, H, W), dtype=torch.int64, device=self.device)
        ops.scd_label_preprocess(label3, flags, labels, B, H, W)
        return pre, post, labels


class BDATransforms(BCDTransforms):
    """reference data/transforms.py:413-427: same normalisation constants as BCDTransforms.  `get_transform_pipelines`
    (reference :567-620) composes cv2 geometry (scale, random_crop_resize) with flip / exchange / normalize / to_tensor.  This
    batch-level pair covers flip / exchange / normalize / to_tensor (`DeviceBDABatchTransform`); the full recipe over a
    file data set is `resident.DeviceAugmentLoader`."""

    @classmethod
    def get_transform_pipelines(cls, args):
        """(train_transform, val_transform): callables `(image6 u8 [B,H,W,6], label2 u8 [B,H,W,2], rng) -> device tensors`."""
        mean = getattr(args, "normalize_mean", cls.DEFAULT_MEAN)
        std = getattr(args, "normalize_std", cls.DEFAULT_STD)
        state = {}

        def make(train):
            def transform(image6, label2, rng=None):
                if "t" not in state:
                    state["t"] = DeviceBDABatchTransform(torch.device("cuda", torch.cuda.current_device()), mean, std)
                flags = draw_augmentation_flags(len(image6), rng or np.random.default_rng(), train=train)
                return state["t"](image6, label2, flags)
            return transform
        return make(True), make(False)


class DeviceBDABatchTransform:
    """`(image6 u8 [B,H,W,6], label2 u8 [B,H,W,2], flags u8 [B,3]) -> (pre, post f32 [B,3,H,W], label_loc f32 [B,1,H,W],
    label_cls int64 [B,H,W])` on the GPU: the tensor side of reference BDATransforms (data/transforms.py:502-556:
    random_flip, random_exchange -- which swaps the IMAGES only --, normalize, to_tensor) and the label arithmetic of
    scripts/train_BDA.py:194-195 (`label[:, 0].float()`, `torch.prod(label, dim=1).long()`).  The image runs through the BCD
    pass (identical arithmetic), the labels through `c3d_bda_label_preprocess`."""

    def __init__(self, device, mean=BCDTransforms.DEFAULT_MEAN, std=BCDTransforms.DEFAULT_STD):
        self.image = DeviceBatchTransform(device, mean, std)
        self.device = self.image.device

    def __call__(self, image6, label2, flags=None):
        label2 = torch.as_tensor(label2).to(self.device, non_blocking=True).contiguous()
        if label2.dtype != torch.uint8 or label2.dim() != 4 or label2.shape[-1] != 2:
            raise ValueError("label2 must be uint8 [B, H, W, 2] (localisation, damage class)")
        B, H, W = label2.shape[:3]
        if flags is not None:
            flags = torch.as_tensor(flags).to(self.device, non_blocking=True).contiguous()
            if flags.dtype != torch.uint8 or tuple(flags.shape) != (B, 3):
                raise ValueError("flags must be uint8 [B, 3]")
        pre, post, _ = self.image(image6, None, flags)
        label_loc = torch.empty((B, 1, H, W), dtype=torch.float32, device=self.device)
        label_cls = torch.empty((B, H, W), dtype=torch.int64, device=self.device)
        ops.bda_label_preprocess(label2, flags, label_loc, label_cls, B, H, W)
        return pre, post, label_loc, label_cls


def cc_normalize_table(mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225)):
    """f32 [3, 256]: Normalize(mean, std)(FloatTensor(u8 / 255.)) for every byte value, with the reference's own
    arithmetic (data/dataset.py:413: numpy u8 / 255. is a float64 division, rounded to f32 by FloatTensor;
    scripts/train_CC.py:466-469 / torchvision Normalize: f32 `sub_(mean).div_(std)`)."""
    v = torch.from_numpy(np.arange(256, dtype=np.uint8) / 255.).to(torch.float32)          # f64 divide -> f32
    m = torch.tensor(mean, dtype=torch.float32).view(3, 1)
    s = torch.tensor(std, dtype=torch.float32).view(3, 1)
    return (v.view(1, 256) - m) / s


class DeviceCCBatchTransform:
    """`(img u8 [B,2,3,H,W], swap u8 [B] or None) -> (pre, post)` f32 [B,3,H,W] on the GPU: reference
    data/dataset.py:411-424 (`/ 255.`, per-image Normalize, the TRAIN split's pair swap) in one HIP pass."""

    def __init__(self, device, mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225)):
        self.device = torch.device(device)
        self.lut = cc_normalize_table(mean, std).to(self.device).contiguous()

    def __call__(self, img, swap=None):
        img = torch.as_tensor(img).to(self.device, non_blocking=True).contiguous()
        ops.require_gpu(img, "raw image pair batch")
        if img.dtype != torch.uint8 or img.dim() != 5 or tuple(img.shape[1:3]) != (2, 3):
            raise ValueError("img must be uint8 [B, 2, 3, H, W]")
        B, _, _, H, W = img.shape
        if swap is not None:
            swap = torch.as_tensor(swap).to(self.device, non_blocking=True).contiguous()
            if swap.dtype != torch.uint8 or tuple(swap.shape) != (B,):
                raise ValueError("swap must be uint8 [B]")
        pre = torch.empty((B, 3, H, W), dtype=torch.float32, device=self.device)
        post = torch.empty_like(pre)
        ops.cc_preprocess(img, swap, self.lut, pre, post, B, H, W)
        return pre, post
