"""`c3d_scene_regions` on the MI355X against the restatement of tests/regions_reference.py: every output must be EQUAL (all
arithmetic is integer).  Scene sizes sit around the multiples of the keyed local phase's LDS tile
(`ops.scene_regions_tile()`); the key maps are those of `regions_cases.key_maps`."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import regions_cases as RC  # noqa: E402
import regions_reference as R  # noqa: E402

from change3d_amd import _lib as L  # noqa: E402
from change3d_amd import ops  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
TH, TW = ops.scene_regions_tile()
SIZES = [(1, 1), (1, 2 * TW + 2), (2 * TH + 2, 1), (TH - 1, TW + 1), (TH, TW), (TH + 1, 2 * TW + 1), (4 * TH + 5, 5 * TW - 3)]
NAMES = [name for name, _ in RC.key_maps(2, 2)]


@functools.lru_cache(maxsize=None)
def _maps(size):
    return dict(RC.key_maps(size[0], size[1], seed=size[0] * 1000 + size[1]))


@functools.lru_cache(maxsize=None)
def _regions(size, name, connectivity):
    return R.regions(_maps(size)[name], connectivity)


@functools.lru_cache(maxsize=None)
def _score(size):
    """scores with NaN, negatives, values above 1 and exact 0 / 1"""
    rng = np.random.default_rng(size[0] * 7 + size[1])
    score = rng.random(size, dtype=np.float32) * 1.2 - 0.1
    special = rng.random(size)
    score[special < 0.05] = np.nan
    score[(special >= 0.05) & (special < 0.1)] = 1.0
    score[(special >= 0.1) & (special < 0.15)] = 0.0
    return score


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _run(key, score=None, **kw):
    out = ops.scene_regions(_dev(key), _dev(score), **kw)
    torch.cuda.synchronize()
    return out


def _assert_equal(got, want, what):
    labels, table, none, object_key, counts = got
    assert none is None
    assert counts.dtype == torch.int32 and torch.equal(counts.cpu(), torch.from_numpy(want["counts"])), (what, counts, want["counts"])
    assert labels.dtype == torch.int32 and torch.equal(labels.cpu(), torch.from_numpy(want["labels"])), what
    assert table.dtype == torch.int32 and torch.equal(table.cpu(), torch.from_numpy(want["table"])), what
    if object_key is not None:
        assert object_key.dtype == torch.uint8 and torch.equal(object_key.cpu(), torch.from_numpy(want["object_key"])), what


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_every_output_equals_the_restatement(size, name):
    key, score = _maps(size)[name], _score(size)
    for connectivity in (4, 8):
        for min_area in (1, 3):
            kw = dict(connectivity=connectivity, min_area=min_area, max_objects=size[0] * size[1])
            want = R.region_objects(key, score, labels0=_regions(size, name, connectivity), **kw)
            _assert_equal(_run(key, score, **kw), want, (size, name, connectivity, min_area))


def test_the_checkerboard_is_every_pixel_or_two_crossing_regions():
    size = SIZES[5]
    key = _maps(size)["checkerboard"]
    labels, table, _, _, counts = _run(key, connectivity=4, max_objects=50)
    assert counts.tolist() == [size[0] * size[1], 50]                   # truncated: the ids past the table stay in the labels
    assert torch.equal(labels.cpu().ravel(), torch.arange(1, size[0] * size[1] + 1, dtype=torch.int32))
    assert table[:, 0].eq(1).all() and torch.equal(table[:, 5].cpu(), torch.from_numpy(key.ravel()[:50].astype(np.int32)))
    _assert_equal(_run(key, connectivity=4, max_objects=50), R.region_objects(key, connectivity=4, max_objects=50), "cut")
    labels, table, _, _, counts = _run(key, connectivity=8, max_objects=50)
    assert counts.tolist() == [2, 2] and torch.equal(labels.cpu(), torch.from_numpy(key.astype(np.int32)))


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("size", SIZES[3:], ids=lambda s: f"{s[0]}x{s[1]}")
def test_a_binary_key_map_gives_the_objects_of_the_mask(size, connectivity):
    key, score = _maps(size)["iid1"], _dev(_score(size))
    k = _dev(key)
    for min_area in (1, 4):
        got = ops.scene_regions(k, score, connectivity=connectivity, min_area=min_area, max_objects=4096)
        want = ops.scene_objects(k, None, score, connectivity=connectivity, min_area=min_area, max_objects=4096)
        assert torch.equal(got[0], want[0]) and torch.equal(got[4], want[4])
        keep = [0, 1, 2, 3, 4, 6, 7]
        assert torch.equal(got[1][:, keep], want[1][:, keep])
        rows = int(want[4][1])
        assert got[1][:rows, 5].eq(1).all() and got[1][rows:, 5].eq(0).all() and want[1][:, 5].eq(0).all()
        assert torch.equal(got[3], (want[0] > 0).to(torch.uint8))


def test_optional_pointers_a_dirty_workspace_and_two_runs():
    size = SIZES[6]
    key, score = _maps(size)["blocks7"], _score(size)
    kw = dict(connectivity=8, min_area=2, max_objects=3000)
    want = R.region_objects(key, score, labels0=_regions(size, "blocks7", 8), **kw)
    first = _run(key, score, **kw)
    _assert_equal(first, want, "first")
    nbytes = L.lib().c3d_scene_regions_ws_bytes(*size)
    dirty = torch.full((nbytes,), 0xA5, dtype=torch.uint8, device=DEV)
    second = _run(key, score, ws=dirty, **kw)
    for a, b in zip(first, second):
        assert a is None and b is None or torch.equal(a, b)
    bare = _run(key, None, want_object_key=False, **kw)
    assert bare[3] is None
    _assert_equal(bare, R.region_objects(key, None, labels0=_regions(size, "blocks7", 8), **kw), "bare")


def test_refusals():
    key = torch.zeros((4, 4), dtype=torch.uint8, device=DEV)
    with pytest.raises(L.Change3DHipError):
        ops.scene_regions(key, connectivity=6)
    with pytest.raises(L.Change3DHipError):
        ops.scene_regions(key, max_objects=0)
    with pytest.raises(ValueError):
        ops.scene_regions(key.to(torch.int32))
    assert L.lib().c3d_scene_regions_ws_bytes(0, 4) == -1 and L.lib().c3d_scene_regions_ws_bytes(65536, 32768) == -2
