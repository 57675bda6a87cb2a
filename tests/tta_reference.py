"""Numpy restatement of the test-time-augmentation views (include/change3d_hip.h "Views"), written from the definition and
not from the kernels: a view code v in 0..7 transposes the last two axes if v & 4, then reverses the rows if v & 2, then the
columns if v & 1; the inverse undoes the two reversals and then transposes.  `fold32` is c3d_scene_fold_views as stated --
sequential f32 adds in ascending view order from the first view's value, one f32 divide -- for the exact comparison,
`fold64` the float64 mean for the bounded one.  `invert=False` and `descending=True` are the negative controls."""
import numpy as np

SETS = {"none": (0,), "hflip": (0, 1), "flips": (0, 1, 2, 3), "d4": (0, 1, 2, 3, 4, 5, 6, 7)}


def view(a, v):
    a = np.swapaxes(a, -2, -1) if v & 4 else a
    a = a[..., ::-1, :] if v & 2 else a
    return a[..., ::-1] if v & 1 else a


def inverse(a, v):
    a = a[..., ::-1] if v & 1 else a
    a = a[..., ::-1, :] if v & 2 else a
    return np.swapaxes(a, -2, -1) if v & 4 else a


def mask_of(codes):
    return sum(1 << v for v in set(codes))


def gather_views(tiles, codes):
    """tiles [n, ...] -> [n * nv, ...], entry i * nv + j = view codes[j] of tile i."""
    return np.stack([np.ascontiguousarray(view(t, v)) for t in tiles for v in codes])


def _fold(values, codes, dtype, invert, descending):
    nv = len(codes)
    v = values.reshape((-1, nv) + values.shape[1:])
    undo = inverse if invert else view
    order = range(nv - 1, -1, -1) if descending else range(nv)
    acc = None
    for j in order:
        term = np.ascontiguousarray(undo(v[:, j], codes[j])).astype(dtype)
        acc = term if acc is None else (acc + term).astype(dtype)
    return (acc / dtype(nv)).astype(dtype)


def fold32(values, codes, invert=True, descending=False):
    """values f32 [cnt * nv, C, th, tw] -> f32 [cnt, C, th, tw], every operation rounded to f32."""
    assert values.dtype == np.float32
    return _fold(values, codes, np.float32, invert, descending)


def fold64(values, codes, invert=True):
    return _fold(values, codes, np.float64, invert, False)
