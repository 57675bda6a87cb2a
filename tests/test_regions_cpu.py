"""The restatement of `c3d_scene_regions` (tests/regions_reference.py) against `scipy.ndimage.label` key by key, against the
restatement of `c3d_scene_objects` on 0 / 1 maps, and the structure that the shared key maps claim.  No GPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import objects_reference as O  # noqa: E402
import regions_cases as RC  # noqa: E402
import regions_reference as R  # noqa: E402

STRUCTURE = {4: [[0, 1, 0], [1, 1, 1], [0, 1, 0]], 8: [[1, 1, 1]] * 3}


def _same_partition(a, b):
    """two label maps name the same sets: the pairs (a, b) are a bijection"""
    pairs = np.unique(np.stack([a.ravel(), b.ravel()]), axis=1)
    return len(np.unique(pairs[0])) == pairs.shape[1] == len(np.unique(pairs[1]))


@pytest.mark.parametrize("connectivity", [4, 8])
def test_regions_equal_scipy_label_per_key(connectivity):
    ndimage = pytest.importorskip("scipy.ndimage")
    for name, key in RC.key_maps(37, 45, seed=5):
        got = R.regions(key, connectivity)
        assert ((got > 0) == (key > 0)).all(), name
        total = 0
        for k in np.unique(key[key > 0]):
            lab, n = ndimage.label(key == k, structure=STRUCTURE[connectivity])
            total += n
            sel = key == k
            assert _same_partition(got[sel], lab[sel]), (name, k)
        assert got.max() == total, name
        first = [int(np.flatnonzero(got.ravel() == i)[0]) for i in range(1, min(int(got.max()), 50) + 1)]
        assert first == sorted(first), name                 # raster order of the first pixel over all keys together


@pytest.mark.parametrize("connectivity", [4, 8])
def test_binary_maps_give_the_objects_of_the_mask(connectivity):
    rng = np.random.default_rng(3)
    for density in (0.3, 0.59, 0.8):
        key = (rng.random((33, 41)) < density).astype(np.uint8)
        score = rng.random((33, 41), dtype=np.float32)
        for min_area in (1, 3):
            want = O.objects(key, score=score, connectivity=connectivity, min_area=min_area, max_objects=100)
            got = R.region_objects(key, score=score, connectivity=connectivity, min_area=min_area, max_objects=100)
            assert np.array_equal(got["labels"], want["labels"]) and np.array_equal(got["counts"], want["counts"])
            rows = int(want["counts"][1])
            assert np.array_equal(np.delete(got["table"], 5, axis=1), np.delete(want["table"], 5, axis=1))
            assert (got["table"][:rows, 5] == 1).all() and (got["table"][rows:, 5] == 0).all()
            assert np.array_equal(got["object_key"], (want["labels"] > 0).astype(np.uint8))


def test_the_key_maps_have_the_structure_they_claim():
    H, W = 12, 14
    maps = dict(RC.key_maps(H, W))
    assert R.regions(maps["checkerboard"], 4).max() == H * W and R.regions(maps["checkerboard"], 8).max() == 2
    assert R.regions(maps["stripes_v"], 8).max() == W and R.regions(maps["stripes_h"], 4).max() == H
    snake = R.regions(maps["serpentine"], 4)
    assert len(np.unique(snake[maps["serpentine"] == 1])) == 1
    assert (maps["nozero"] > 0).all() and R.regions(maps["one_key"], 4).max() == 1 and R.regions(maps["zero"], 8).max() == 0
    assert R.regions(maps["rings"], 4).max() == (min(H, W) + 1) // 2
    key = np.array([[1, 2], [2, 1]], np.uint8)              # two regions cross at the lattice point
    assert R.regions(key, 8).tolist() == [[1, 2], [2, 1]] and R.regions(key, 4).max() == 4


def test_the_class_is_the_key_and_min_area_drops():
    key = np.array([[9, 9, 0, 200], [9, 0, 0, 200], [255, 0, 7, 7]], np.uint8)
    out = R.region_objects(key, connectivity=4, min_area=2, max_objects=8)
    assert out["counts"].tolist() == [3, 3] and out["table"][:3, 5].tolist() == [9, 200, 7]
    assert out["object_key"].tolist() == [[9, 9, 0, 200], [9, 0, 0, 200], [0, 0, 7, 7]]
    cut = R.region_objects(key, connectivity=4, min_area=1, max_objects=2)
    assert cut["counts"].tolist() == [4, 2] and cut["labels"].max() == 4 and cut["table"][:, 5].tolist() == [9, 200]
