"""`c3d_regions_sieve` on the MI355X against the restatement of tests/sieve_reference.py: the map, the regions and `info` must
be EQUAL (all arithmetic is integer).  The hand-counted cases are blown up (`regions_cases.stretch`) so that a small region
and its target lie in different tiles of the labelling."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import regions_cases as RC  # noqa: E402
import regions_reference as R  # noqa: E402
import sieve_reference as S  # noqa: E402

from change3d_amd import _lib as L  # noqa: E402
from change3d_amd import ops  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SIZE = (150, 200)                                           # 3 x 4 tiles with ragged edges
SURVEY = {"blocks4": lambda: RC.block_noise(*SIZE, 4, seed=0, block=16), "blocks7": lambda: RC.block_noise(*SIZE, 7, seed=0, block=16)}


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _run(key, min_area, **kw):
    out = ops.regions_sieve(_dev(key), min_area, **kw)
    torch.cuda.synchronize()
    return out


@functools.lru_cache(maxsize=None)
def _survey_map(name):
    return SURVEY[name]()


@functools.lru_cache(maxsize=None)
def _want(name, min_area, connectivity):
    return S.sieve(_survey_map(name), min_area, connectivity)


def _assert_equal(got, want, connectivity, what, entries=True):
    labels, table, none, key_out, counts, info = got
    assert none is None and key_out.dtype == torch.uint8 and info.dtype == torch.int32
    assert torch.equal(key_out.cpu(), torch.from_numpy(want["key_out"])), what
    cols = slice(None) if entries else [0, 1, 2, 3, 4, 5, 7]
    assert info.cpu().numpy()[cols].tolist() == want["info"][cols].tolist(), (what, info, want["info"])
    regions = R.region_objects(want["key_out"], connectivity=connectivity, max_objects=table.shape[0])
    assert torch.equal(counts.cpu(), torch.from_numpy(regions["counts"])), what
    assert torch.equal(labels.cpu(), torch.from_numpy(regions["labels"])), what
    assert torch.equal(table.cpu(), torch.from_numpy(regions["table"])), what


@pytest.mark.parametrize("name", sorted(RC.HAND))
def test_hand_counted_cases_across_tiles(name):
    key, min_area, connectivity, after = RC.stretch(name)
    want = S.sieve(key, min_area, connectivity)
    assert np.array_equal(want["key_out"], after)
    got = _run(key, min_area, connectivity=connectivity, max_objects=64)
    _assert_equal(got, want, connectivity, name)


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("min_area", [2, 9, 16])
@pytest.mark.parametrize("name", sorted(SURVEY))
def test_survey_maps(name, min_area, connectivity):
    want = _want(name, min_area, connectivity)
    assert want["info"][0] == 0 and want["info"][1] >= 1
    got = _run(_survey_map(name), min_area, connectivity=connectivity, max_objects=SIZE[0] * SIZE[1] // 2)
    _assert_equal(got, want, connectivity, (name, min_area, connectivity))


@pytest.mark.parametrize("connectivity", [4, 8])
def test_noise_is_all_small_and_takes_several_rounds(connectivity):
    key = RC.iid(70, 90, 49, seed=11)                       # 50 keys: every region is small, and they merge step by step
    want = S.sieve(key, 16, connectivity, max_rounds=16)
    assert want["info"][0] == 0 and want["info"][1] >= 3, want["info"]
    got = _run(key, 16, connectivity=connectivity, max_rounds=16, max_objects=6300)
    _assert_equal(got, want, connectivity, connectivity)


@pytest.mark.parametrize("connectivity", [4, 8])
def test_min_area_one_is_the_identity(connectivity):
    key = _survey_map("blocks7")
    score = _dev(np.random.default_rng(5).random(SIZE, dtype=np.float32))
    got = ops.regions_sieve(_dev(key), 1, score=score, connectivity=connectivity, max_objects=20000)
    want = ops.scene_regions(_dev(key), score, connectivity=connectivity, max_objects=20000)
    assert torch.equal(got[3].cpu(), torch.from_numpy(key)) and got[5][:5].tolist() == [0, 0, 0, 0, 0]
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and torch.equal(got[4], want[4])
    assert int(got[5][5]) == int(want[4][0])


def test_one_round_where_two_are_needed():
    key = _survey_map("blocks7")
    assert _want("blocks7", 16, 4)["info"][1] == 2
    want = S.sieve(key, 16, 4, max_rounds=1)
    assert want["info"][0] == S.ST_NOT_CONVERGED
    assert np.array_equal(want["key_out"], S.paint(key, S.analyse(key, 4, 16)))    # the map after one round
    got = _run(key, 16, connectivity=4, max_rounds=1, max_objects=20000)
    assert int(got[5][0]) == L.SIEVE_ST_NOT_CONVERGED
    _assert_equal(got, want, 4, "one round")


def test_a_table_too_small_gives_the_input_back():
    key = _survey_map("blocks7")
    full = _want("blocks7", 16, 4)
    assert full["info"][6] > 64 * 16                                                # far more pairs than slots
    want = S.sieve(key, 16, 4, table_capacity=64)
    assert want["info"][0] == S.ST_TABLE_FULL and np.array_equal(want["key_out"], key)
    got = _run(key, 16, connectivity=4, max_objects=20000, table_capacity=64)
    assert int(got[5][0]) == L.SIEVE_ST_TABLE_FULL and 0 < int(got[5][6]) <= 64     # the entries that fitted
    _assert_equal(got, want, 4, "table full", entries=False)
    assert ops.regions_sieve_plan(*SIZE, 64)[1] == 64 and ops.regions_sieve_plan(*SIZE)[1] >= 8 * SIZE[0] * SIZE[1] - 8 * sum(SIZE)


def test_labels_are_the_regions_of_the_output_map_with_scores():
    key = _survey_map("blocks4")
    score = _dev(np.random.default_rng(6).random(SIZE, dtype=np.float32))
    got = ops.regions_sieve(_dev(key), 9, score=score, connectivity=8, max_objects=5000)
    again = ops.scene_regions(got[3], score, connectivity=8, max_objects=5000)
    assert torch.equal(got[0], again[0]) and torch.equal(got[1], again[1]) and torch.equal(got[4], again[4])
    assert int(got[1][:int(got[4][1]), 0].min()) >= 9


def test_a_dirty_workspace_and_two_runs():
    key = _dev(_survey_map("blocks7"))
    kw = dict(connectivity=8, max_objects=20000)
    first = ops.regions_sieve(key, 16, **kw)
    nbytes, _ = ops.regions_sieve_plan(*SIZE)
    dirty = torch.full((nbytes,), 0xA5, dtype=torch.uint8, device=DEV)
    second = ops.regions_sieve(key, 16, ws=dirty, **kw)
    third = ops.regions_sieve(key, 16, ws=dirty, **kw)                               # the workspace of a finished call
    for a, b, c in zip(first, second, third):
        assert a is None and b is None or (torch.equal(a, b) and torch.equal(a, c))


def test_refusals():
    key = torch.zeros((4, 4), dtype=torch.uint8, device=DEV)
    for kw in (dict(min_area=0), dict(min_area=2 ** 20 + 1), dict(min_area=2, max_rounds=0), dict(min_area=2, max_rounds=65537)):
        with pytest.raises(ValueError):
            ops.regions_sieve(key, **kw)
    with pytest.raises(L.Change3DHipError):
        ops.regions_sieve(key, 2, connectivity=5)
    with pytest.raises(L.Change3DHipError):
        ops.regions_sieve(key, 2, table_capacity=48)                                 # not a power of two
    ws = torch.zeros(ops.regions_sieve_plan(4, 4)[0], dtype=torch.uint8, device=DEV)
    out = [torch.zeros(16, dtype=torch.int32, device=DEV) for _ in range(4)]
    rc = L.lib().c3d_regions_sieve(key.data_ptr(), None, 4, 4, 8, 2, 8, 2, 16, key.data_ptr(), out[0].data_ptr(), out[1].data_ptr(),
                                   out[2].data_ptr(), out[3].data_ptr(), ws.data_ptr(), None)
    assert rc == -1                                                                  # key_out must not alias key
