"""Training from file data sets without host work per step: `ResidentStore` decodes a split ONCE into a uint8 store
(`[N, Hs, Ws, 6]` images, `[N, Hs, Ws(, L)]` labels) that lives in HBM, and `DeviceAugmentLoader` turns one epoch into one
uploaded `[n, 8]` table and one `c3d_augment_gather` launch per step: gather of the shuffled samples plus the reference's
whole transform chain (reference data/transforms.py:166-207; scripts/train_BCD.py:43-84 for the DataLoader calls this
loader stands in for).  LEVIR-CD cut to 256 x 256 is 7 120 x 256 x 256 x 7 B = 3.3 GB as uint8."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from .. import _lib as L
from .. import ops
from .transforms import BCDTransforms, crop_area_of, draw_augmentation_table, validate_augment_table

TASKS = {"bcd": L.AUG_BCD, "scd": L.AUG_SCD, "bda": L.AUG_BDA}
LABEL_CHANNELS = {"bcd": 1, "scd": 3, "bda": 2}


class ResidentStore:
    """uint8 image and label arrays of one split, on the GPU when they fit the byte budget (`resident_gb`), otherwise in
    pinned host memory (then a gathered uint8 batch is copied per step and the kernel runs with index = b)."""

    def __init__(self, images, labels, device, resident_gb=16.0):
        self.device = torch.device(device)
        images, labels = torch.as_tensor(images), torch.as_tensor(labels)
        if images.dtype != torch.uint8 or images.dim() != 4 or images.shape[-1] != 6:
            raise ValueError("images must be uint8 [N, H, W, 6] (pre | post)")
        if labels.dtype != torch.uint8 or labels.shape[:3] != images.shape[:3] or labels.dim() not in (3, 4):
            raise ValueError("labels must be uint8 [N, H, W] or [N, H, W, L] matching the images")
        self.n, self.height, self.width = (int(v) for v in images.shape[:3])
        self.label_channels = 1 if labels.dim() == 3 else int(labels.shape[3])
        self.nbytes = images.numel() + labels.numel()
        self.on_device = self.nbytes <= resident_gb * 2 ** 30
        if self.on_device:
            self.images, self.labels = images.to(self.device).contiguous(), labels.to(self.device).contiguous()
        else:
            pin = lambda t: t if t.is_pinned() or not torch.cuda.is_available() else t.contiguous().pin_memory()  # noqa: E731
            self.images, self.labels = pin(images.cpu()), pin(labels.cpu())

    def __len__(self):
        return self.n

    @classmethod
    def from_dataset(cls, dataset, device, num_workers=4, resident_gb=16.0):
        """Decode every sample of `dataset` (BCDDataset / SCDDataset / BDADataset: anything with `raw(i)`) once, on a pool of
        `num_workers` threads, into pinned uint8 and hand the arrays to the store.  All samples must share one size."""
        n = len(dataset)
        if n == 0:
            raise ValueError(f"no samples under {dataset.file_root}/{dataset.split}")
        img0, lab0 = dataset.raw(0)
        pin = torch.cuda.is_available()
        images = torch.empty((n,) + img0.shape, dtype=torch.uint8, pin_memory=pin)
        labels = torch.empty((n,) + lab0.shape, dtype=torch.uint8, pin_memory=pin)
        img_np, lab_np = images.numpy(), labels.numpy()

        def decode(i):
            img, lab = (img0, lab0) if i == 0 else dataset.raw(i)
            if img.shape != img0.shape or lab.shape != lab0.shape:
                raise ValueError(f"mixed image sizes: {dataset.pre_images[i]} is {img.shape[0]} x {img.shape[1]} but "
                                 f"{dataset.pre_images[0]} is {img0.shape[0]} x {img0.shape[1]}; cut the data set to one size")
            img_np[i], lab_np[i] = img, lab

        with ThreadPoolExecutor(max_workers=max(1, int(num_workers))) as pool:
            list(pool.map(decode, range(n)))
        return cls(images, labels, device, resident_gb)


class DeviceAugmentLoader:
    """Stand-in for the reference's `DataLoader(dataset, batch_size, shuffle=train, drop_last=False)` over a
    `ResidentStore`.  Every `__iter__` is one epoch: one permutation seeded by `(seed, epoch)` (the identity for
    validation) of which rank r takes `perm[r::world]` (cut to `N // world` so that all ranks step together), one table
    drawn by `draw_augmentation_table`, validated on the host and uploaded ONCE; a step is one `c3d_augment_gather` launch
    on a slice of it.  Validation loaders pass no table.  Yields what the script loops unpack:
    bcd `(img f32 [B,6,H,W], label f32 [B,1,H,W])`, scd `(img, labels int64 [B,3,H,W])`,
    bda `(img, label_loc f32 [B,1,H,W], label_cls int64 [B,H,W])`."""

    def __init__(self, store, batch_size, task, train, seed=0, rank=0, world=1, drop_last=False, out_size=None,
                 mean=BCDTransforms.DEFAULT_MEAN, std=BCDTransforms.DEFAULT_STD):
        if task not in TASKS:
            raise ValueError(f"task must be one of {sorted(TASKS)}")
        if store.label_channels != LABEL_CHANNELS[task]:
            raise ValueError(f"task {task} needs {LABEL_CHANNELS[task]} label channel(s), the store has {store.label_channels}")
        self.store, self.bs, self.task, self.train = store, int(batch_size), task, bool(train)
        self.seed, self.rank, self.world, self.drop_last = int(seed), int(rank), int(world), bool(drop_last)
        self.height, self.width = (store.height, store.width) if out_size is None else (int(out_size[0]), int(out_size[1]))
        self.crop_area = crop_area_of(self.width)
        self.n = len(store) // self.world if self.world > 1 else len(store)
        self.nb = self.n // self.bs if self.drop_last else -(-self.n // self.bs)
        self.epoch = 0
        dev = store.device
        self.mean = torch.tensor(mean, dtype=torch.float32, device=dev)
        self.std = torch.tensor(std, dtype=torch.float32, device=dev)
        self.two_pass = self.train and (self.height, self.width) != (store.height, store.width)
        self.scratch = None

    def __len__(self):
        return self.nb

    def set_epoch(self, epoch):
        self.epoch = int(epoch)

    def epoch_table(self, epoch):
        """The host table of one epoch, int32 [n, 8], index column = store index."""
        if self.train:
            rng = np.random.default_rng([self.seed, int(epoch)])
            indices = rng.permutation(len(self.store))[self.rank::self.world][:self.n]
        else:
            rng, indices = None, np.arange(len(self.store))[self.rank::self.world][:self.n]
        return draw_augmentation_table(indices, rng, self.crop_area, train=self.train)

    def __iter__(self):
        st, dev = self.store, self.store.device
        H, W, B = self.height, self.width, self.bs
        host_table = validate_augment_table(self.epoch_table(self.epoch), len(st), H, W)
        self.epoch += 1
        table = None
        if not st.on_device:
            indices = torch.from_numpy(host_table[:, 0].astype(np.int64))
            host_table = host_table.copy()
            host_table[:, 0] = np.arange(len(host_table)) % B        # the kernel reads the copied batch: index = b
        if self.train:
            table = torch.from_numpy(host_table).to(dev)             # once per epoch
        if self.two_pass and self.scratch is None:
            self.scratch = torch.empty((2, B, 3, H, W), dtype=torch.float32, device=dev)
        task = TASKS[self.task]
        for i in range(self.nb):
            lo, hi = i * B, min((i + 1) * B, self.n)
            b = hi - lo
            if st.on_device:
                images, labels, n_src = st.images, st.labels, len(st)
                # validation reads the samples in order: a view of the store that starts at this batch
                if table is None:
                    images, labels, n_src = images[lo:hi], labels[lo:hi], b
            else:
                images = st.images[indices[lo:hi]].pin_memory().to(dev, non_blocking=True)
                labels = st.labels[indices[lo:hi]].pin_memory().to(dev, non_blocking=True)
                n_src = b
            pre = torch.empty((b, 3, H, W), dtype=torch.float32, device=dev)
            post = torch.empty_like(pre)
            label_b = None
            if self.task == "bcd":
                label_a = torch.empty((b, 1, H, W), dtype=torch.float32, device=dev)
            elif self.task == "scd":
                label_a = torch.empty((b, 3, H, W), dtype=torch.int64, device=dev)
            else:
                label_a = torch.empty((b, 1, H, W), dtype=torch.float32, device=dev)
                label_b = torch.empty((b, H, W), dtype=torch.int64, device=dev)
            ops.augment_gather(images, labels, None if table is None else table[lo:hi], self.mean, self.std, pre, post,
                               label_a, label_b, self.scratch, task, n_src, st.height, st.width, b, H, W)
            img = torch.cat([pre, post], dim=1)
            yield (img, label_a) if label_b is None else (img, label_a, label_b)


def build_file_loaders(args, dataset_cls, task, device, rank=0, world=1):
    """(train, val, test) `DeviceAugmentLoader`s over `<args.file_root>/{train,val,test}`: what the reference's
    `create_data_loaders` builds (scripts/train_BCD.py:31-89), with its shuffle / drop_last choices."""
    from .transforms import BCDTransforms as T
    mean, std = getattr(args, "normalize_mean", T.DEFAULT_MEAN), getattr(args, "normalize_std", T.DEFAULT_STD)
    gb = float(getattr(args, "resident_gb", 16.0))
    loaders = []
    for split in ("train", "val", "test"):
        store = ResidentStore.from_dataset(dataset_cls(args.file_root, split), device, getattr(args, "num_workers", 4), gb)
        train = split == "train"
        loaders.append(DeviceAugmentLoader(store, args.batch_size, task, train, seed=16, rank=rank if train else 0,
                                           world=world if train else 1, drop_last=False,
                                           out_size=(args.in_height, args.in_width), mean=mean, std=std))
    return loaders
