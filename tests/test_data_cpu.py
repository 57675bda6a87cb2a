"""File data sets, the augmentation table and its host validation (no GPU): change3d_amd/data/dataset.py,
draw_augmentation_table / validate_augment_table, the loader's epoch bookkeeping, and the host reference of
test_augment_gpu.py held against the kernel's arithmetic restated in numpy."""
import os
import sys

import numpy as np
import pytest
import torch
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import augment_reference as R  # noqa: E402

from change3d_amd.data import dataset as D  # noqa: E402
from change3d_amd.data.transforms import (BCDTransforms, crop_area_of, draw_augmentation_flags,  # noqa: E402
                                          draw_augmentation_table, validate_augment_table)


def write_tree(root, task, split="train", n=3, height=12, width=16, seed=0):
    """A small PNG tree in the reference's layout; returns {name: (pre, post, [labels])} of what was written."""
    rng = np.random.default_rng(seed)
    subs = {"bcd": ["label"], "scd": ["label1", "label2", "change"], "bda": ["label1", "label2"]}[task]
    for sub in ["t1", "t2"] + subs:
        os.makedirs(os.path.join(root, split, sub), exist_ok=True)
    written = {}
    for i in range(n):
        name = f"area_{i:03d}_post_disaster.png" if task == "bda" else f"tile_{i:03d}.png"
        lname = name.replace("disaster", "disaster_target") if task == "bda" else name
        pre = rng.integers(0, 256, size=(height, width, 3), dtype=np.uint8)
        post = rng.integers(0, 256, size=(height, width, 3), dtype=np.uint8)
        Image.fromarray(pre, "RGB").save(os.path.join(root, split, "t1", name))
        Image.fromarray(post, "RGB").save(os.path.join(root, split, "t2", name))
        labels = []
        for sub in subs:
            if task == "bcd":                                   # change mask {0, 255}
                lab = (rng.integers(0, 2, size=(height, width)) * 255).astype(np.uint8)
            elif sub == "change" or (task == "bda" and sub == "label1"):   # 0 / 1 change mask, 0 / 1 localisation
                lab = rng.integers(0, 2, size=(height, width), dtype=np.uint8)
            else:                                               # class ids
                lab = rng.integers(0, 5, size=(height, width), dtype=np.uint8)
            Image.fromarray(lab, "L").save(os.path.join(root, split, sub, lname))
            labels.append(lab)
        written[name] = (pre, post, labels)
    return written


@pytest.mark.parametrize("task,cls,channels", [("bcd", D.BCDDataset, 1), ("scd", D.SCDDataset, 3), ("bda", D.BDADataset, 2)])
def test_datasets_read_the_reference_layouts(tmp_path, task, cls, channels):
    written = write_tree(str(tmp_path), task)
    ds = cls(str(tmp_path), "train")
    assert len(ds) == 3
    for i in range(len(ds)):
        name = ds.file_list[i]
        pre, post, labels = written[name]                       # pairing is by file name
        img, lab = ds[i]
        assert img.dtype == np.uint8 and img.shape == (12, 16, 6)
        assert lab.dtype == np.uint8 and lab.shape == ((12, 16) if channels == 1 else (12, 16, channels))
        if task == "bda":                                       # cv2.imread order: BGR
            assert np.array_equal(img[:, :, 0:3], pre[:, :, ::-1]) and np.array_equal(img[:, :, 3:6], post[:, :, ::-1])
        else:                                                   # skimage.io.imread order: RGB
            assert np.array_equal(img[:, :, 0:3], pre) and np.array_equal(img[:, :, 3:6], post)
        got = [lab] if channels == 1 else [lab[:, :, k] for k in range(channels)]
        for g, w in zip(got, labels):
            assert np.array_equal(g, w)


@pytest.mark.parametrize("task,cls,victim", [("bcd", D.BCDDataset, "t2"), ("scd", D.SCDDataset, "change"), ("bda", D.BDADataset, "label2")])
def test_missing_partner_is_a_file_not_found_error(tmp_path, task, cls, victim):
    write_tree(str(tmp_path), task)
    d = os.path.join(str(tmp_path), "train", victim)
    os.remove(os.path.join(d, sorted(os.listdir(d))[1]))
    with pytest.raises(FileNotFoundError):
        cls(str(tmp_path), "train")
    with pytest.raises(FileNotFoundError):
        cls(str(tmp_path / "nowhere"), "train")


def test_colour_label_file_is_refused_by_name(tmp_path):
    write_tree(str(tmp_path), "bcd")
    bad = os.path.join(str(tmp_path), "train", "label", "tile_001.png")
    Image.fromarray(np.zeros((12, 16, 3), dtype=np.uint8), "RGB").save(bad)
    ds = D.BCDDataset(str(tmp_path), "train")
    with pytest.raises(ValueError, match="tile_001.png"):
        ds[1]


def test_resident_store_refuses_mixed_sizes_and_names_the_file(tmp_path):
    from change3d_amd.data.resident import ResidentStore
    write_tree(str(tmp_path), "bcd")
    for sub, mode, shape in [("t1", "RGB", (10, 16, 3)), ("t2", "RGB", (10, 16, 3)), ("label", "L", (10, 16))]:
        Image.fromarray(np.zeros(shape, dtype=np.uint8), mode).save(os.path.join(str(tmp_path), "train", sub, "tile_002.png"))
    with pytest.raises(ValueError, match="tile_002.png"):
        ResidentStore.from_dataset(D.BCDDataset(str(tmp_path), "train"), "cpu", num_workers=2)


def test_resident_store_decodes_a_split_on_the_thread_pool(tmp_path):
    from change3d_amd.data.resident import ResidentStore
    written = write_tree(str(tmp_path), "scd", n=5)
    ds = D.SCDDataset(str(tmp_path), "train")
    store = ResidentStore.from_dataset(ds, "cpu", num_workers=3)
    assert len(store) == 5 and (store.height, store.width, store.label_channels) == (12, 16, 3)
    for i, name in enumerate(ds.file_list):
        assert np.array_equal(store.images[i, :, :, 0:3].numpy(), written[name][0])
        assert np.array_equal(store.labels[i, :, :, 2].numpy(), written[name][2][2])


def test_draw_table_ranges_and_inclusive_upper_bound():
    ca = crop_area_of(256)
    assert ca == 8 and crop_area_of(64) == 2 and crop_area_of(224) == 7
    t = draw_augmentation_table(np.arange(4000) % 37, np.random.default_rng(3), ca, train=True)
    assert t.dtype == np.int32 and t.shape == (4000, 8)
    assert np.array_equal(t[:, 0], np.arange(4000) % 37) and not t[:, 7].any()
    for col in (1, 4, 5, 6):
        assert set(np.unique(t[:, col])) == {0, 1} and 0.45 < t[:, col].mean() < 0.55
    crop = t[:, 1] == 1
    assert t[crop, 2].min() == 0 and t[crop, 2].max() == ca and t[crop, 3].min() == 0 and t[crop, 3].max() == ca
    assert not t[~crop, 2:4].any()
    validate_augment_table(t, 37, 256, 256)


def test_draw_table_validation_is_all_zero_and_seeded_draws_repeat():
    v = draw_augmentation_table(np.arange(10), None, 8, train=False)
    assert np.array_equal(v[:, 0], np.arange(10)) and not v[:, 1:].any()
    a = draw_augmentation_table(np.arange(64), np.random.default_rng([16, 2]), 8)
    b = draw_augmentation_table(np.arange(64), np.random.default_rng([16, 2]), 8)
    c = draw_augmentation_table(np.arange(64), np.random.default_rng([16, 3]), 8)
    assert np.array_equal(a, b) and not np.array_equal(a, c)
    # the flag draw that was here before is untouched
    assert draw_augmentation_flags(5, np.random.default_rng(0)).shape == (5, 3)


def test_host_validation_refuses_bad_tables():
    good = draw_augmentation_table(np.arange(8), np.random.default_rng(0), 8)
    validate_augment_table(good, 8, 256, 256)
    bad = good.copy(); bad[3, 0] = 8
    with pytest.raises(ValueError, match="index"):
        validate_augment_table(bad, 8, 256, 256)
    bad = good.copy(); bad[3, 0] = -1
    with pytest.raises(ValueError, match="index"):
        validate_augment_table(bad, 8, 256, 256)
    bad = good.copy(); bad[0, 1:4] = (1, 128, 0)
    with pytest.raises(ValueError, match="x1"):
        validate_augment_table(bad, 8, 256, 256)
    bad = good.copy(); bad[0, 1:4] = (1, 0, 32)
    with pytest.raises(ValueError, match="y1"):
        validate_augment_table(bad, 8, 64, 256)
    with pytest.raises(ValueError, match="int32"):
        validate_augment_table(good.astype(np.int64), 8, 256, 256)
    with pytest.raises(ValueError, match="0 or 1"):
        bad = good.copy(); bad[0, 5] = 2
        validate_augment_table(bad, 8, 256, 256)


class _HostStore:
    """What the loader's epoch bookkeeping needs of a store, without a device."""
    def __init__(self, n):
        self.n, self.height, self.width, self.label_channels, self.device, self.on_device = n, 64, 64, 1, torch.device("cpu"), True

    def __len__(self):
        return self.n


def test_loader_epochs_ranks_and_lengths():
    from change3d_amd.data.resident import DeviceAugmentLoader
    mk = lambda **kw: DeviceAugmentLoader(_HostStore(38), 8, "bcd", True, seed=16, **kw)  # noqa: E731
    one = mk()
    assert len(one) == 5 and len(mk(drop_last=True)) == 4                  # drop_last=False keeps the partial batch
    e0, e0b, e1 = one.epoch_table(0), mk().epoch_table(0), one.epoch_table(1)
    assert np.array_equal(e0, e0b) and not np.array_equal(e0[:, 0], e1[:, 0])
    assert sorted(e0[:, 0]) == list(range(38))
    r0, r1 = mk(rank=0, world=2).epoch_table(4), mk(rank=1, world=2).epoch_table(4)
    assert len(r0) == len(r1) == 19 and not set(r0[:, 0]) & set(r1[:, 0])
    assert sorted(np.concatenate([r0[:, 0], r1[:, 0]])) == list(range(38))     # disjoint and covering
    val = DeviceAugmentLoader(_HostStore(38), 8, "bcd", False).epoch_table(7)
    assert np.array_equal(val[:, 0], np.arange(38)) and not val[:, 1:].any()
    with pytest.raises(ValueError, match="label channel"):
        DeviceAugmentLoader(_HostStore(38), 8, "scd", True)


def test_dropin_dataset_import_resolves():
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(root, "change3d_amd", "dropin"), root]))
    code = ("import data.dataset as RSDataset; import change3d_amd.data.dataset as M; "
            "assert RSDataset.BCDDataset is M.BCDDataset and RSDataset.SCDDataset is M.SCDDataset and RSDataset.BDADataset is M.BDADataset")
    subprocess.run([sys.executable, "-c", code], check=True, env=env, timeout=120)


def test_new_entry_is_declared_and_exported():
    from change3d_amd import _lib
    assert "c3d_augment_gather" in _lib.check_exports()
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "change3d_hip.h")).read()
    assert "int c3d_augment_gather(" in header


@pytest.mark.parametrize("size", [(64, 64, 64, 64), (96, 80, 96, 80), (256, 256, 300, 280)])
def test_torch_chain_agrees_with_the_kernel_arithmetic(size):
    """The yardstick of the GPU test (torch's bilinear / nearest on the CPU) against the kernel's formulas in numpy: labels
    exact; images within 1e-5 where the output extent is a power of two, 1e-4 where it is not (torch computes the source
    coordinate in f32 from an f32 scale, the kernel -- like cv2 -- in double, and a coordinate that differs by an f32 ulp
    moves a value by ulp x the local gradient)."""
    H, W, Hs, Ws = size
    ca = crop_area_of(W)
    images, labels = R.synth_store(1, Hs, Ws, 3, seed=5)
    tol = 1e-5 if (H & (H - 1)) == 0 and (W & (W - 1)) == 0 else 1e-4
    for x1, y1 in [(0, 0), (ca, ca), (0, ca), (1, ca - 1)]:
        for mean, std in [(BCDTransforms.DEFAULT_MEAN, BCDTransforms.DEFAULT_STD), (BCDTransforms.IMAGENET_MEAN, BCDTransforms.IMAGENET_STD)]:
            row = [0, 1, x1, y1, 1, 1, 0, 0]
            pre, post, (lab,) = R.reference_sample(images[0], labels[0], row, mean, std, H, W, "scd")
            img, klab = R.kernel_model_sample(images[0], labels[0], row, mean, std, H, W)
            assert np.abs(torch.cat([pre, post]).numpy().transpose(1, 2, 0) - img).max() <= tol
            assert np.array_equal(lab.numpy(), klab.transpose(2, 0, 1).astype(np.int64))


def test_reference_chain_without_crop_is_the_oracle_transform():
    from oracle import transforms as OT
    images, labels = R.synth_store(2, 16, 16, 1, seed=2)
    for flags in [(0, 0, 0), (1, 0, 1), (1, 1, 0)]:
        row = [0, 0, 0, 0, flags[0], flags[1], flags[2], 0]
        pre, post, (lab,) = R.reference_sample(images[1], labels[1], row, BCDTransforms.IMAGENET_MEAN, BCDTransforms.IMAGENET_STD, 16, 16, "bcd")
        want = OT.bcd_transform_sample(images[1], labels[1], flags, BCDTransforms.IMAGENET_MEAN, BCDTransforms.IMAGENET_STD)
        assert torch.equal(torch.cat([pre, post]), torch.as_tensor(want[0]).float().reshape(6, 16, 16))
        assert torch.equal(lab.reshape(-1), torch.as_tensor(want[1]).float().reshape(-1))
