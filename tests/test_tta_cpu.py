"""The eight test-time-augmentation views as a group, on the host: the numpy restatement (tests/tta_reference.py) against
np.rot90 / np.fliplr, the named sets, the bank model of the kernels' LDS block, and the argument checks of
`SceneInferencer(..., tta=...)`, which must raise without a GPU."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import tta_reference as TR  # noqa: E402

from change3d_amd import infer  # noqa: E402

A = np.arange(5 * 5, dtype=np.float32).reshape(5, 5) ** 1.5            # no symmetry of the square leaves it unchanged


def test_every_code_is_a_rotation_of_an_optional_mirror():
    """The dihedral group of the square is {rot90^k, rot90^k o fliplr}: every code must be one of them, and all eight differ."""
    group = {(k, m): np.rot90(np.fliplr(A) if m else A, k) for k in range(4) for m in (0, 1)}
    hit = set()
    for v in range(8):
        match = [key for key, g in group.items() if np.array_equal(TR.view(A, v), g)]
        assert len(match) == 1, (v, match)
        hit.add(match[0])
    assert len(hit) == 8
    for v in range(8):
        for w in range(v):
            assert not np.array_equal(TR.view(A, v), TR.view(A, w)), (v, w)


def test_the_definition_in_numpy_terms():
    for v in range(8):
        V = A.swapaxes(-2, -1) if v & 4 else A
        V = V[..., ::-1, :] if v & 2 else V
        V = V[..., ::-1] if v & 1 else V
        assert np.array_equal(TR.view(A, v), V)
    stack = np.stack([A, 2 * A])                                         # leading axes are carried along
    assert np.array_equal(TR.view(stack, 5)[1], TR.view(2 * A, 5))


def test_inverse_undoes_view_and_only_the_quarter_turns_are_not_involutions():
    B = np.arange(4 * 6, dtype=np.float32).reshape(4, 6)
    for v in range(8):
        assert np.array_equal(TR.inverse(TR.view(A, v), v), A) and np.array_equal(TR.view(TR.inverse(A, v), v), A)
        if v < 4:
            assert np.array_equal(TR.inverse(TR.view(B, v), v), B)        # the plain views need no square
        involution = np.array_equal(TR.view(TR.view(A, v), v), A)
        assert involution == (v not in (5, 6)), v
    assert np.array_equal(TR.view(TR.view(A, 5), 6), A) and np.array_equal(TR.view(TR.view(A, 6), 5), A)
    assert np.array_equal(TR.inverse(A, 5), TR.view(A, 6)) and np.array_equal(TR.inverse(A, 6), TR.view(A, 5))
    assert {v for v in range(8) if np.array_equal(TR.view(A, v), np.rot90(A, 1)) or np.array_equal(TR.view(A, v), np.rot90(A, 3))} == {5, 6}


def test_named_sets_and_masks():
    want = {"none": (0,), "hflip": (0, 1), "flips": (0, 1, 2, 3), "d4": tuple(range(8))}
    assert infer.VIEW_SETS == want and TR.SETS == want
    assert [infer.view_mask(want[k]) for k in ("none", "hflip", "flips", "d4")] == [0x01, 0x03, 0x0f, 0xff]
    from change3d_amd import _lib
    assert (_lib.VIEWS_NONE, _lib.VIEWS_HFLIP, _lib.VIEWS_FLIPS, _lib.VIEWS_D4) == (0x01, 0x03, 0x0f, 0xff)
    assert infer.view_codes("flips") == (0, 1, 2, 3) and infer.view_codes([5, 0, 3, 3]) == (0, 3, 5)
    assert infer.view_codes(np.array([6, 1])) == (1, 6)
    assert infer.view_mask((0, 3, 5)) == TR.mask_of((0, 3, 5)) == 0b101001
    from change3d_amd import ops
    assert [ops.view_count(m) for m in (1, 3, 15, 255, 0b101001)] == [1, 2, 4, 8, 3]


def test_fold_restatement_is_the_mean_of_the_inverted_views():
    rng = np.random.default_rng(0)
    # multiples of 2^-8: partial sums of up to eight equal values then fit 24 bits, so every add and the divide by 1, 2, 4, 8
    # are exact; a full-precision value already rounds at x + x + x
    tiles = (np.round(rng.standard_normal((3, 2, 6, 6)) * 256) / 256).astype(np.float32)
    for codes in ((0,), (0, 1), (0, 1, 2, 3), tuple(range(8)), (0, 3, 5)):
        values = TR.gather_views(tiles, codes)
        assert values.shape == (3 * len(codes), 2, 6, 6)
        # the same tile under every view folds back to itself: nv equal values, the divide by 3 may round
        assert np.allclose(TR.fold32(values, codes), tiles, rtol=2 ** -22, atol=0)
        if len(codes) in (1, 2, 4, 8):
            assert np.array_equal(TR.fold32(values, codes), tiles)
        assert np.allclose(TR.fold64(values, codes), tiles, rtol=1e-15, atol=0)
        if 5 in codes or 6 in codes:
            assert not np.array_equal(TR.fold32(values, codes, invert=False), TR.fold32(values, codes))


def test_lds_block_is_conflict_free_in_the_bank_model():
    """tools/tta_lds_check.py: the [32][33] block costs one LDS cycle per 32-lane half by rows and by columns; pitch 32 does not."""
    import tta_lds_check
    rows, cols = tta_lds_check.block_cycles(33)
    assert rows == cols == 2
    assert tta_lds_check.block_cycles(32)[1] > 2


class _Stub(torch.nn.Module):
    def __init__(self, th=64, tw=64):
        super().__init__()
        self.args = SimpleNamespace(in_height=th, in_width=tw, num_class=7)
        self.w = torch.nn.Parameter(torch.zeros(1))


def test_inferencer_validates_tta_on_the_host():
    for tta in (None, "none", "hflip", "flips", "d4", (0,), [0, 5], (7, 2)):
        infer.SceneInferencer(_Stub(), "bcd", tta=tta)
    for bad in ("rot", "", (), (8,), (-1, 0), (0, 1.5), 3, ("d4",), (True,)):
        with pytest.raises(ValueError):
            infer.SceneInferencer(_Stub(), "bcd", tta=bad)
    infer.SceneInferencer(_Stub(64, 32), "bcd", tta="flips")             # the plain views need no square
    for tta in ("d4", (0, 4), (6,)):
        with pytest.raises(ValueError, match="square"):
            infer.SceneInferencer(_Stub(64, 32), "bcd", tta=tta)
    infer.SceneInferencer(_Stub(), "scd", batch=8, tta="d4")
    with pytest.raises(ValueError, match="batch"):
        infer.SceneInferencer(_Stub(), "scd", batch=7, tta="d4")
    with pytest.raises(ValueError, match="batch"):
        infer.SceneInferencer(_Stub(), "bcd", batch=1, tta="hflip")
    assert infer.SceneInferencer(_Stub(), "bcd").views is None
    assert infer.SceneInferencer(_Stub(), "bcd", tta="flips").views == (0, 1, 2, 3)
