"""Host reference for `c3d_augment_gather` (helper of test_data_cpu.py / test_augment_gpu.py, not a test module).

cv2 is not installed, so the resampling cannot be pinned to it: the arithmetic is restated, not pinned.  The independent
yardstick is torch on the CPU, whose `F.interpolate(mode="bilinear", align_corners=False, antialias=False)` and legacy
`mode="nearest"` are documented to follow OpenCV's conventions.  `reference_sample` chains, on CPU tensors: the reference's
own numpy normalisation lines (data/transforms.py:126-137), slicing, F.interpolate, flip, channel swap -- in the order
of the reference's recipe normalize -> scale -> random_crop_resize -> random_flip -> random_exchange -> to_tensor.
"""
import numpy as np
import torch
import torch.nn.functional as F


def _resize(img_hwc, label_hwl, height, width):
    """cv2.resize(img, (w, h)) [INTER_LINEAR] and cv2.resize(label, (w, h), INTER_NEAREST) through torch; the identity when
    the size already matches (cv2 copies)."""
    if img_hwc.shape[:2] == (height, width):
        return img_hwc, label_hwl
    t = torch.from_numpy(np.ascontiguousarray(img_hwc)).permute(2, 0, 1)[None]
    img = F.interpolate(t, size=(height, width), mode="bilinear", align_corners=False, antialias=False)[0].permute(1, 2, 0).numpy()
    lt = torch.from_numpy(np.ascontiguousarray(label_hwl)).permute(2, 0, 1)[None].float()
    lab = F.interpolate(lt, size=(height, width), mode="nearest")[0].permute(1, 2, 0).numpy().astype(label_hwl.dtype)
    return img, lab


def reference_sample(image6, label, row, mean, std, height, width, task):
    """One output sample.  image6 u8 [Hs, Ws, 6]; label u8 [Hs, Ws] or [Hs, Ws, L]; row = the sample's table row (index
    ignored) or None.  Returns (pre f32 [3,H,W], post f32 [3,H,W], labels) with labels = (f32 [1,H,W],) for bcd,
    (int64 [3,H,W],) for scd, (loc f32 [1,H,W], cls int64 [H,W]) for bda."""
    mean_array = np.array(mean, dtype=np.float32).reshape(1, 1, -1)
    std_array = np.array(std, dtype=np.float32).reshape(1, 1, -1)
    img = image6.astype(np.float32) / 255.0                      # normalize
    img = (img - mean_array) / std_array
    lab = label if label.ndim == 3 else label[:, :, None]
    img, lab = _resize(img, lab, height, width)                  # scale
    _, do_crop, x1, y1, flip0, flip1, exchange, _ = (0,) * 8 if row is None else (int(v) for v in row)
    if do_crop:                                                  # random_crop_resize
        img, lab = _resize(img[y1:height - y1, x1:width - x1], lab[y1:height - y1, x1:width - x1], height, width)
    if flip0:                                                    # random_flip: cv2.flip(., 0) reverses the rows
        img, lab = img[::-1], lab[::-1]
    if flip1:
        img, lab = img[:, ::-1], lab[:, ::-1]
    if exchange:                                                 # random_exchange
        img = np.concatenate((img[:, :, 3:6], img[:, :, 0:3]), axis=2)
        if task == "scd":
            lab = np.stack((lab[:, :, 1], lab[:, :, 0], lab[:, :, 2]), axis=2)
    chw = torch.from_numpy(np.ascontiguousarray(img.transpose(2, 0, 1)))       # to_tensor
    lt = torch.from_numpy(np.ascontiguousarray(lab.transpose(2, 0, 1)))
    if task == "bcd":
        labels = (torch.from_numpy(np.ceil(lt.numpy() / 255.0).astype(np.float32)),)
    elif task == "scd":
        labels = (lt.long(),)
    else:
        labels = (lt[0:1].float(), torch.prod(lt.long(), dim=0))
    return chw[0:3].contiguous(), chw[3:6].contiguous(), labels


def reference_batch(images, labels, table, mean, std, height, width, task):
    """Batch form: images u8 [N,Hs,Ws,6], labels u8 [N,Hs,Ws(,L)], table int32 [B,8] or None (index = b, no augmentation)."""
    n = len(images) if table is None else len(table)
    out = [reference_sample(images[b if table is None else int(table[b, 0])], labels[b if table is None else int(table[b, 0])],
                            None if table is None else table[b], mean, std, height, width, task) for b in range(n)]
    pre, post = torch.stack([o[0] for o in out]), torch.stack([o[1] for o in out])
    return pre, post, tuple(torch.stack([o[2][k] for o in out]) for k in range(len(out[0][2])))


# ------------------------------------------------------------------------------------------------------------------
# The kernel's arithmetic restated in numpy (f32 taps, f64 coordinate, separate multiplies and add): what the CPU tests
# hold against the torch chain above, so that the tolerance of the GPU test is known before a GPU is involved.
def _lin_coords(dst, src):
    d = np.arange(dst)
    if src == dst:
        return d, np.zeros(dst, dtype=np.float32)
    c = ((d + 0.5) * (float(src) / float(dst)) - 0.5).astype(np.float32)
    s = np.floor(c).astype(np.int64)
    f = (c - s.astype(np.float32)).astype(np.float32)
    f[s < 0] = 0
    s[s < 0] = 0
    f[s >= src - 1] = 0
    s[s >= src - 1] = src - 1
    return s, f


def _near_coords(dst, src):
    return np.minimum(np.arange(dst) * src // dst, src - 1)


def _lerp(a, b, f):
    one = np.float32(1.0)
    return np.where(f == 0, a, (a * (one - f)).astype(np.float32) + (b * f).astype(np.float32)).astype(np.float32)


def _kernel_resize(img, lab, height, width):
    hs, ws = img.shape[:2]
    sy, fy = _lin_coords(height, hs)
    sx, fx = _lin_coords(width, ws)
    sy1, sx1 = np.minimum(sy + 1, hs - 1), np.minimum(sx + 1, ws - 1)
    fxb, fyb = fx[None, :, None], fy[:, None, None]
    h0 = _lerp(img[sy][:, sx], img[sy][:, sx1], fxb)
    h1 = _lerp(img[sy1][:, sx], img[sy1][:, sx1], fxb)
    return _lerp(h0, h1, fyb), lab[_near_coords(height, hs)][:, _near_coords(width, ws)]


def kernel_model_sample(image6, label, row, mean, std, height, width):
    """(img f32 [H,W,6], label u8 [H,W,L]) before the task's label arithmetic, by the kernel's own formulas."""
    mean_array = np.array(mean, dtype=np.float32).reshape(1, 1, -1)
    std_array = np.array(std, dtype=np.float32).reshape(1, 1, -1)
    img = (image6.astype(np.float32) / np.float32(255.0) - mean_array) / std_array
    lab = label if label.ndim == 3 else label[:, :, None]
    img, lab = _kernel_resize(img, lab, height, width)
    _, do_crop, x1, y1, flip0, flip1, exchange, _ = (0,) * 8 if row is None else (int(v) for v in row)
    if do_crop:
        img, lab = _kernel_resize(img[y1:height - y1, x1:width - x1], lab[y1:height - y1, x1:width - x1], height, width)
    if flip0:
        img, lab = img[::-1], lab[::-1]
    if flip1:
        img, lab = img[:, ::-1], lab[:, ::-1]
    if exchange:
        img = np.concatenate((img[:, :, 3:6], img[:, :, 0:3]), axis=2)
    return np.ascontiguousarray(img), np.ascontiguousarray(lab)


def synth_store(n, height, width, label_channels, seed, num_class=7):
    """Seeded uint8 arrays with per-pixel varying content: images [n,H,W,6]; labels [n,H,W] in {0, 255} for one channel,
    [n,H,W,L] with classes varying per pixel otherwise (channel 0 of a 2-channel label is a 0/1 localisation map)."""
    rng = np.random.default_rng(seed)
    images = rng.integers(0, 256, size=(n, height, width, 6), dtype=np.uint8)
    if label_channels == 1:
        labels = (rng.integers(0, 2, size=(n, height, width)) * 255).astype(np.uint8)
    else:
        labels = rng.integers(0, num_class, size=(n, height, width, label_channels)).astype(np.uint8)
        if label_channels == 2:
            labels[..., 0] = rng.integers(0, 2, size=(n, height, width))
        if label_channels == 3:
            labels[..., 2] = rng.integers(0, 2, size=(n, height, width))
    return images, labels
