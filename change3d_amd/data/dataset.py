"""File data sets of the BCD / SCD / BDA recipes: the reference's `data/dataset.py` classes (reference
data/dataset.py:23-47 BCDDataset, :124-150 SCDDataset, :238-263 BDADataset) with the same constructor signature,
directory layout and raw return values -- `[H, W, 6]` uint8 image (pre | post) and a uint8 label array.  The transform
chain is NOT applied per sample on the host: `ResidentStore` (resident.py) decodes a split once and the
`c3d_augment_gather` kernel does the whole chain on the GPU.

Decoding is PIL's.  The reference reads BCD / SCD through `skimage.io.imread` (RGB channel order, labels with
`as_gray=True`) and BDA through `cv2.imread` (BGR channel order, labels with flag 0): so `BDADataset` reverses the channel
order of PIL's RGB array and the other two do not.  Label files must be single-channel 8-bit images: skimage's `as_gray`
turns a colour file into floats in [0, 1] (and cv2's flag 0 into a luma mix), and neither path is mirrored here, so a
colour label file is refused by name.
"""
import os
from os.path import join as osp

import numpy as np
from PIL import Image


def read_rgb(path):
    """uint8 [H, W, 3] in RGB order (what skimage.io.imread returns for an 8-bit colour file)."""
    with Image.open(path) as im:
        if im.mode != "RGB":
            im = im.convert("RGB")
        return np.asarray(im, dtype=np.uint8)


def read_label(path):
    """uint8 [H, W] of a single-channel 8-bit label file; anything else is refused."""
    with Image.open(path) as im:
        if im.mode not in ("L", "P", "1"):
            raise ValueError(f"label file {path} has mode {im.mode}: label files must be single-channel 8-bit images "
                             f"(a colour label would go through skimage's as_gray float path, which is not mirrored)")
        if im.mode == "1":
            return np.asarray(im.convert("L"), dtype=np.uint8)
        return np.asarray(im, dtype=np.uint8)        # "P": the palette indices are the class ids


class _PairDataset:
    """Shared part: file lists, the existence check of the reference's `_validate_files`, raw decode."""
    LIST_DIR = "label"
    BGR = False

    def __init__(self, file_root, split, transform=None):
        if not os.path.exists(file_root):
            raise FileNotFoundError(f"Dataset root path does not exist: {file_root}")
        self.file_root, self.split, self.transform = file_root, split, transform
        self.file_list = sorted(os.listdir(osp(file_root, split, self.LIST_DIR)))
        self.pre_images = [osp(file_root, split, "t1", x) for x in self.file_list]
        self.post_images = [osp(file_root, split, "t2", x) for x in self.file_list]
        self.label_files = self._label_files()
        for what, paths in [("Pre-change image", self.pre_images), ("Post-change image", self.post_images)] + \
                [("Ground truth mask", p) for p in self.label_files]:
            for p in paths:
                if not os.path.exists(p):
                    raise FileNotFoundError(f"{what} not found: {p}")

    def __len__(self):
        return len(self.file_list)

    def raw(self, idx):
        """(image uint8 [H, W, 6], label uint8 [H, W] or [H, W, L]) before any transform."""
        pre, post = read_rgb(self.pre_images[idx]), read_rgb(self.post_images[idx])
        if self.BGR:
            pre, post = pre[:, :, ::-1], post[:, :, ::-1]
        if pre.shape != post.shape:
            raise ValueError(f"{self.pre_images[idx]} is {pre.shape[:2]} but its partner {self.post_images[idx]} is {post.shape[:2]}")
        labels = [read_label(p[idx]) for p in self.label_files]
        for lab, p in zip(labels, self.label_files):
            if lab.shape != pre.shape[:2]:
                raise ValueError(f"{p[idx]} is {lab.shape} but its image {self.pre_images[idx]} is {pre.shape[:2]}")
        img = np.concatenate((pre, post), axis=2)
        label = labels[0] if len(labels) == 1 else np.stack(labels, axis=2)
        return img, label

    def __getitem__(self, idx):
        img, label = self.raw(idx)
        if self.transform:
            img, label = self.transform(img, label)
        return img, label


class BCDDataset(_PairDataset):
    """`<file_root>/<split>/{t1,t2,label}/<name>`: ([H, W, 6] RGB | RGB, [H, W] change mask).  reference data/dataset.py:23-97
    (skimage.io.imread: RGB order; the file list is that of `label`, sorted here so that the sample order is reproducible)."""
    LABEL_CHANNELS = 1

    def _label_files(self):
        self.label_change = [osp(self.file_root, self.split, "label", x) for x in self.file_list]
        return [self.label_change]


class SCDDataset(_PairDataset):
    """`<file_root>/<split>/{t1,t2,label1,label2,change}/<name>`: ([H, W, 6] RGB | RGB, [H, W, 3] = pre classes, post
    classes, change mask).  reference data/dataset.py:124-211 (skimage.io.imread: RGB order; file list of `label1`)."""
    LIST_DIR = "label1"
    LABEL_CHANNELS = 3

    def _label_files(self):
        d = lambda sub: [osp(self.file_root, self.split, sub, x) for x in self.file_list]  # noqa: E731
        self.pre_label, self.post_label, self.label_change = d("label1"), d("label2"), d("change")
        return [self.pre_label, self.post_label, self.label_change]


class BDADataset(_PairDataset):
    """`<file_root>/<split>/{t1,t2}/<name>` and `{label1,label2}/<name with 'disaster' -> 'disaster_target'>`:
    ([H, W, 6] BGR | BGR, [H, W, 2] = localisation, damage class).  reference data/dataset.py:238-320 reads with
    cv2.imread, whose channel order is BGR: PIL's RGB array is reversed here, for this data set only."""
    LIST_DIR = "t1"
    LABEL_CHANNELS = 2
    BGR = True

    def _label_files(self):
        d = lambda sub: [osp(self.file_root, self.split, sub, x.replace("disaster", "disaster_target")) for x in self.file_list]  # noqa: E731
        self.label_loc, self.label_cls = d("label1"), d("label2")
        return [self.label_loc, self.label_cls]
