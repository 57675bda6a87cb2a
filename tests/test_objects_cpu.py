"""The restatement that the GPU tests of `c3d_scene_objects` compare with (tests/objects_reference.py), checked on the host:
against `scipy.ndimage.label` label for label, against `np.bincount`, on hand-made votes and scores, and against wrong
variants of itself, which the mask list must tell apart."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import objects_reference as R  # noqa: E402

TH = TW = 8                                               # a stand-in tile: the masks only need seams to lie across
SIZES = [(1, 1), (1, TW + 6), (TH + 3, 1), (TH, TW), (2 * TH + 3, 2 * TW + 6), (TH + 1, 3 * TW - 1)]


def _all_masks():
    for size in SIZES:
        for name, mask in R.mask_list(size[0], size[1], TH, TW, seed=size[0] * 100 + size[1]):
            yield size, name, mask


def test_labels_equal_scipy_label_for_label():
    ndimage = pytest.importorskip("scipy.ndimage")
    structure = {4: None, 8: np.ones((3, 3), dtype=int)}
    n = 0
    for size, name, mask in _all_masks():
        for connectivity in (4, 8):
            want, count = ndimage.label(mask, structure=structure[connectivity])
            got = R.components(mask, connectivity)
            assert got.dtype == np.int32 and np.array_equal(got, want) and got.max() == count, (size, name, connectivity)
            n += 1
    assert n == len(SIZES) * 10 * 2
    rng = np.random.default_rng(3)
    for _ in range(40):                                   # and on masks of no particular structure
        mask = rng.random(rng.integers(1, 30, size=2)) < rng.random()
        for connectivity in (4, 8):
            assert np.array_equal(R.components(mask, connectivity), ndimage.label(mask, structure=structure[connectivity])[0])


def test_filter_against_bincount():
    for size, name, mask in _all_masks():
        labels = R.components(mask, 4)
        area = np.bincount(labels.ravel())
        for min_area in (0, 1, 2, 9):
            got = R.filter_small(labels, min_area)
            big = np.flatnonzero(area >= max(min_area, 1))
            big = big[big > 0]
            assert got.max() == len(big), (size, name, min_area)
            assert np.array_equal(got > 0, np.isin(labels, big))
            for new, old in enumerate(big, start=1):      # the order of the survivors is kept
                assert np.array_equal(got == new, labels == old)
            if min_area <= 1:
                assert np.array_equal(got, labels)


def test_votes_ties_first_class_and_out_of_range_classes():
    mask = np.zeros((9, 6), np.uint8)
    cls = np.zeros((9, 6), np.uint8)
    rows = {0: [2, 2, 3, 3, 0, 0], 2: [0, 0, 0, 0, 4, 1], 4: [0] * 6, 6: [9, 9, 9, 5, 5, 1], 8: [4, 4, 4, 1, 1, 0]}
    for y, v in rows.items():
        mask[y] = 1
        cls[y] = v
    out = R.objects(mask, cls, None, connectivity=4, n_cls=5, first_class=1, max_objects=6)
    assert out["counts"].tolist() == [5, 5]
    assert out["table"][:5, 5].tolist() == [2, 1, 0, 1, 4]                         # tie -> lowest; class 0 never wins from first_class 1
    assert out["hist"][3].tolist() == [0, 1, 0, 0, 0]                              # 9 and 5 are >= n_cls: counted nowhere
    assert out["hist"][2].tolist() == [6, 0, 0, 0, 0] and out["table"][5].tolist() == [0] * 8
    assert np.array_equal(out["object_cls"][::2], np.repeat(np.array([[2, 1, 0, 1, 4]], np.uint8).T, 6, axis=1))
    assert int(out["object_cls"][1::2].sum()) == 0
    assert R.objects(mask, cls, None, connectivity=4, n_cls=5, first_class=0, max_objects=6)["table"][:5, 5].tolist() == [0, 0, 0, 1, 4]
    assert R.objects(mask, cls, None, connectivity=4, n_cls=5, first_class=3, max_objects=6)["table"][:5, 5].tolist() == [3, 4, 0, 0, 4]
    assert R.objects(mask, None, None, connectivity=4, max_objects=6)["hist"] is None
    assert out["table"][1].tolist()[:5] == [6, 0, 2, 5, 2] and out["table"][1, 6] == 12


def test_score_q_special_values_and_half_roundings():
    q = R.score_fixed(np.array([0.0, 1.0, np.nan, -2.0, 3.0, 0.5, 1.0 / 65535.0, np.inf, -np.inf], np.float32))
    assert q.tolist() == [0, 65535, 0, 0, 65535, 32768, 1, 65535, 0]               # 32767.5 rounds to the even 32768
    mask = np.ones((1, 4), np.uint8)
    for values, want in (([0, 0, 0, 2], 1), ([0, 0, 0, 1], 0), ([1, 0, 0, 1], 1), ([3, 0, 0, 3], 2), ([65535] * 4, 65535)):
        score = (np.array([values], np.float64) / 65535.0).astype(np.float32)
        assert R.score_fixed(score).tolist() == [values]
        assert R.objects(mask, None, score, max_objects=1)["table"][0, 7] == want  # (S + 2) // 4: a mean at .5 goes up
    assert R.objects(mask, None, None, max_objects=1)["table"][0, 7] == 0


def test_truncation_at_max_objects():
    mask = R.mask_list(5, 7, TH, TW)[2][1]                                         # checkerboard: 18 objects at 4-connectivity
    cls = np.full(mask.shape, 2, np.uint8)
    full = R.objects(mask, cls, None, connectivity=4, n_cls=3, max_objects=32)
    cut = R.objects(mask, cls, None, connectivity=4, n_cls=3, max_objects=3)
    assert full["counts"].tolist() == [18, 18] and cut["counts"].tolist() == [18, 3]
    assert np.array_equal(cut["labels"], full["labels"]) and cut["table"].shape == (3, 8) and cut["hist"].shape == (3, 3)
    assert np.array_equal(cut["table"], full["table"][:3])
    assert np.array_equal(cut["object_cls"], np.where(full["labels"] <= 3, full["object_cls"], 0))
    assert int((cut["object_cls"] > 0).sum()) == 3 and int((full["object_cls"] > 0).sum()) == 18


def test_negative_controls_are_told_apart_by_the_mask_list():
    swapped = ties_high = 0
    for size, name, mask in _all_masks():
        swapped += not np.array_equal(R.components(mask, 4), R.components(mask, 8))
        cls = np.random.default_rng(1).integers(0, 3, size=mask.shape, dtype=np.uint8)
        a = R.objects(mask, cls, None, n_cls=3, max_objects=mask.size)
        b = R.objects(mask, cls, None, n_cls=3, max_objects=mask.size, ties="high")
        ties_high += not np.array_equal(a["table"], b["table"])
    assert swapped >= 1 and ties_high >= 1                                         # told apart at all is what counts
    for name in ("checkerboard", "diagonal", "antidiagonal"):
        mask = dict(R.mask_list(*SIZES[4], TH, TW))[name]
        assert R.components(mask, 8).max() == 1 and R.components(mask, 4).max() == mask.sum() > 1
    for name in ("serpentine", "u"):
        mask = dict(R.mask_list(*SIZES[4], TH, TW))[name]
        assert R.components(mask, 4).max() == 1


def test_predict_scene_parser_accepts_the_new_flags():
    from change3d_amd.scripts import predict_scene
    p = predict_scene.build_parser()
    a = p.parse_args(["--task", "BDA", "--weights", "w.pth", "--objects", "--min_area", "9", "--connectivity", "4", "--label1", "a.png",
                      "--label2", "b.png"])
    assert (a.task, a.objects, a.min_area, a.connectivity) == ("BDA", True, 9, 4)
    b = p.parse_args(["--weights", "w.pth"])
    assert (b.task, b.objects, b.min_area, b.connectivity) == ("BCD", False, 1, 8)
    with pytest.raises(SystemExit):
        p.parse_args(["--weights", "w.pth", "--connectivity", "6"])
    c = p.parse_args(["--task", "SCD", "--weights", "w.pth", "--objects"])
    assert [predict_scene.num_classes(x) for x in (a, b, c)] == [5, 1, 7]          # the task's default, for every caller
    assert predict_scene.num_classes(p.parse_args(["--task", "SCD", "--weights", "w.pth", "--num_class", "9"])) == 9
