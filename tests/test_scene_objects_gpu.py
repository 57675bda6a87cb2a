"""`c3d_scene_objects` on the MI355X against the restatement of tests/objects_reference.py: every output must be EQUAL (all
arithmetic is integer).  Scene sizes sit around the multiples of the local phase's LDS tile (`ops.scene_label_tile()`): one
pixel, one row, one column, exactly one tile, more than two tiles each way with ragged edges, and a width that is no multiple
of 4; the masks are those of `objects_reference.mask_list`."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import objects_reference as R  # noqa: E402

from change3d_amd import _lib as L  # noqa: E402
from change3d_amd import ops  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
TH, TW = ops.scene_label_tile()
SIZES = [(1, 1), (1, TW + 6), (TH + 3, 1), (TH, TW), (2 * TH + 3, 2 * TW + 6), (TH + 1, 3 * TW - 1)]
MASKS = [name for name, _ in R.mask_list(2, 2, TH, TW)]
N_CLS = 5


@functools.lru_cache(maxsize=None)
def _masks(size):
    return dict(R.mask_list(size[0], size[1], TH, TW, seed=size[0] * 1000 + size[1]))


@functools.lru_cache(maxsize=None)
def _components(size, name, connectivity):
    return R.components(_masks(size)[name], connectivity)


@functools.lru_cache(maxsize=None)
def _side_inputs(size):
    """Class map with values past n_cls, and scores with NaN, negatives, values above 1 and exact 0 / 1."""
    rng = np.random.default_rng(size[0] * 7 + size[1])
    cls = rng.integers(0, N_CLS + 2, size=size, dtype=np.uint8)
    score = rng.random(size, dtype=np.float32) * 1.2 - 0.1
    special = rng.random(size)
    score[special < 0.05] = np.nan
    score[(special >= 0.05) & (special < 0.1)] = 1.0
    score[(special >= 0.1) & (special < 0.15)] = 0.0
    return cls, score


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _run(mask, cls=None, score=None, **kw):
    out = ops.scene_objects(_dev(mask), _dev(cls), _dev(score), **kw)
    torch.cuda.synchronize()
    return out


def _assert_equal(got, want, what):
    labels, table, hist, object_cls, counts = got
    assert counts.dtype == torch.int32 and torch.equal(counts.cpu(), torch.from_numpy(want["counts"])), (what, counts, want["counts"])
    assert labels.dtype == torch.int32 and torch.equal(labels.cpu(), torch.from_numpy(want["labels"])), what
    assert table.dtype == torch.int32 and torch.equal(table.cpu(), torch.from_numpy(want["table"])), what
    if hist is not None:
        assert torch.equal(hist.cpu().to(torch.int64), torch.from_numpy(want["hist"])), what
    if object_cls is not None:
        assert object_cls.dtype == torch.uint8 and torch.equal(object_cls.cpu(), torch.from_numpy(want["object_cls"])), what


@pytest.mark.parametrize("name", MASKS)
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_every_output_equals_the_restatement(size, name):
    mask = _masks(size)[name]
    cls, score = _side_inputs(size)
    for connectivity in (4, 8):
        for min_area in (1, 2, 9):
            kw = dict(connectivity=connectivity, min_area=min_area, n_cls=N_CLS, first_class=1, max_objects=size[0] * size[1] // 2 + 1)
            want = R.objects(mask, cls, score, labels0=_components(size, name, connectivity), **kw)
            got = _run(mask, cls, score, **kw)
            assert got[2] is not None and got[3] is not None
            _assert_equal(got, want, (size, name, connectivity, min_area))


def test_the_mask_list_has_the_structure_it_claims():
    size = SIZES[4]
    m = _masks(size)
    assert _components(size, "checkerboard", 8).max() == 1 and _components(size, "checkerboard", 4).max() == m["checkerboard"].sum()
    assert _components(size, "serpentine", 4).max() == 1 and _components(size, "u", 4).max() == 1
    for d in ("diagonal", "antidiagonal"):
        assert _components(size, d, 8).max() == 1 and _components(size, d, 4).max() == m[d].sum() > TH


@pytest.mark.parametrize("name", ["checkerboard", "random0.3", "random0.59", "u"])
@pytest.mark.parametrize("size", SIZES[3:], ids=lambda s: f"{s[0]}x{s[1]}")
def test_truncation_at_three_objects(size, name):
    mask = _masks(size)[name]
    cls, score = _side_inputs(size)
    kw = dict(connectivity=4, min_area=1, n_cls=N_CLS, first_class=1, max_objects=3)
    want = R.objects(mask, cls, score, labels0=_components(size, name, 4), **kw)
    got = _run(mask, cls, score, **kw)
    _assert_equal(got, want, (size, name))
    assert tuple(got[1].shape) == (3, 8) and tuple(got[2].shape) == (3, N_CLS)
    if name != "u":
        assert int(got[4][0]) > 3 and int(got[4][1]) == 3 and int(got[0].max()) == int(got[4][0])   # the ids past the table stay


@pytest.mark.parametrize("missing", ["cls_map", "score", "object_cls", "hist", "all"])
def test_optional_pointers_may_be_null(missing):
    size = SIZES[4]
    mask = _masks(size)["random0.59"]
    cls, score = _side_inputs(size)
    if missing in ("cls_map", "all"):
        cls = None
    if missing in ("score", "all"):
        score = None
    kw = dict(connectivity=8, min_area=2, n_cls=N_CLS, first_class=1, max_objects=4096)
    want = R.objects(mask, cls, score, labels0=_components(size, "random0.59", 8), **kw)
    got = _run(mask, cls, score, want_object_cls=missing not in ("object_cls", "all"), want_hist=missing not in ("hist", "all"), **kw)
    assert (got[2] is None) == (missing in ("cls_map", "hist", "all")) and (got[3] is None) == (missing in ("object_cls", "all"))
    _assert_equal(got, want, missing)
    if cls is None:
        assert int(got[1][:, 5].abs().sum()) == 0
    if score is None:
        assert int(got[1][:, 7].abs().sum()) == 0


def test_votes_ties_first_class_and_an_object_that_only_votes_background():
    """Five bars of 2 x 6 pixels, two of them across a seam: a 6 : 6 tie of classes 2 and 3 (-> 2), a 3 : 3 tie of 4 and 1 under
    a majority of class 0 (first_class = 1 -> 1, first_class = 0 -> 0), only class 0 (-> 0), only classes >= n_cls (-> 0,
    counted nowhere), and a clear majority of the highest class."""
    H, W = TH + 8, 2 * TW + 4
    mask, cls = np.zeros((H, W), np.uint8), np.zeros((H, W), np.uint8)
    bars = [(2, 3), (2, TW - 3), (TH - 1, 20), (TH - 1, TW + 30), (TH + 5, TW - 3)]       # two of them lie across a seam
    votes = [[2] * 6 + [3] * 6, [0] * 6 + [4, 4, 1, 4, 1, 1], [0] * 12, [N_CLS] * 6 + [N_CLS + 1] * 6, [4] * 7 + [1] * 5]
    for (y, x), v in zip(bars, votes):
        mask[y:y + 2, x:x + 6] = 1
        cls[y:y + 2, x:x + 6] = np.array(v, np.uint8).reshape(2, 6)
    for first_class in (1, 0, 3):
        kw = dict(connectivity=8, min_area=1, n_cls=N_CLS, first_class=first_class, max_objects=8)
        want = R.objects(mask, cls, None, **kw)
        got = _run(mask, cls, None, **kw)
        _assert_equal(got, want, first_class)
        if first_class == 1:
            assert got[1][:5, 5].tolist() == [2, 1, 0, 0, 4] and got[2][3].tolist() == [0] * N_CLS and got[2][2].tolist() == [12, 0, 0, 0, 0]
        if first_class == 0:
            assert got[1][:5, 5].tolist() == [2, 0, 0, 0, 4]
    kw["first_class"] = 1
    assert R.objects(mask, cls, None, ties="high", **kw)["table"][:2, 5].tolist() == [3, 4]      # the wrong rule is told apart


def test_score_roundings_on_the_device():
    """One object per row of 4 pixels: means that land exactly on .5 in fixed point, and the special values."""
    rows = [[0.0, 0.0, 0.0, 1.0 / 65535.0 * 2], [1.0, 1.0, 1.0, 1.0], [np.nan, -3.0, 7.0, 0.5], [1.0 / 65535.0, 0.0, 0.0, 1.0 / 65535.0],
            [0.25, 0.75, 0.5, 0.5], [3.0 / 65535.0, 0, 0, 3.0 / 65535.0]]
    mask = np.zeros((2 * len(rows), 4), np.uint8)
    score = np.zeros(mask.shape, np.float32)
    mask[0::2] = 1
    score[0::2] = np.array(rows, np.float32)
    want = R.objects(mask, None, score, connectivity=4, max_objects=8)
    got = _run(mask, None, score, connectivity=4, max_objects=8)
    _assert_equal(got, want, "score")
    assert got[1][:6, 7].tolist() == [1, 65535, (65535 + 32768 + 2) // 4, 1, 32768, 2]


def test_two_runs_agree_bit_for_bit():
    size = SIZES[4]
    cls, score = _side_inputs(size)
    for name in ("random0.59", "serpentine"):
        a = _run(_masks(size)[name], cls, score, connectivity=8, n_cls=N_CLS, max_objects=4096)
        b = _run(_masks(size)[name], cls, score, connectivity=8, n_cls=N_CLS, max_objects=4096)
        assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_refusals_return_their_error_and_launch_nothing():
    lib = L.lib()
    H, W = 8, 8
    mask = torch.ones((H, W), dtype=torch.uint8, device=DEV)
    cls = torch.ones((H, W), dtype=torch.uint8, device=DEV)
    labels = torch.full((H, W), -7, dtype=torch.int32, device=DEV)
    table = torch.full((4, 8), -7, dtype=torch.int32, device=DEV)
    counts = torch.full((2,), -7, dtype=torch.int32, device=DEV)
    ws = torch.empty(lib.c3d_scene_label_ws_bytes(H, W, 16), dtype=torch.uint8, device=DEV)
    p = lambda t: None if t is None else t.data_ptr()  # noqa: E731

    def call(mask=mask, cls=None, Hs=H, Ws=W, conn=8, n_cls=1, max_objects=4, labels=labels, table=table, counts=counts, ws=ws):
        return lib.c3d_scene_objects(p(mask), p(cls), None, Hs, Ws, conn, 1, n_cls, 1, max_objects, p(labels), p(table), None, None,
                                     p(counts), p(ws), None)

    before = ops.launch_count()
    for conn in (0, 6, 9, -4):
        assert call(conn=conn) == -1                                 # C3D_E_BADARG
    assert call(Hs=65536, Ws=32768) == -2                            # C3D_E_UNSUPPORTED: Hs * Ws = 2^31
    assert call(cls=cls, n_cls=0) == -1 and call(cls=cls, n_cls=17) == -1
    assert call(max_objects=0) == -1 and call(max_objects=-5) == -1
    assert call(labels=None) == -1 and call(table=None) == -1 and call(counts=None) == -1 and call(ws=None) == -1 and call(mask=None) == -1
    assert lib.c3d_scene_label_ws_bytes(65536, 32768, 1) == -2 and lib.c3d_scene_label_ws_bytes(8, 8, 17) == -1
    assert lib.c3d_scene_label_ws_bytes(0, 8, 1) == -1
    torch.cuda.synchronize()
    assert ops.launch_count() == before
    for t in (labels, table, counts):
        assert int((t != -7).sum()) == 0                             # nothing was written
    with pytest.raises(L.Change3DHipError):
        ops.scene_objects(mask, connectivity=5)
    with pytest.raises(L.Change3DHipError):
        ops.scene_objects(mask, max_objects=0)
    assert call() == 0                                               # the same arguments, accepted
    torch.cuda.synchronize()
    assert ops.launch_count() > before and counts.tolist() == [1, 1] and table[0].tolist() == [64, 0, 0, 7, 7, 0, 0, 0]
