"""`c3d_scene_gather_views` and `c3d_scene_fold_views` on the MI355X.  Both are exact, so every comparison is `torch.equal`:
the gather against the views (tests/tta_reference.py) of `c3d_scene_gather`'s own output, which test_scene_ops_gpu.py pins to
the oracle; the fold against the f32 restatement of its definition -- sequential adds in ascending view order, one divide.

Shapes: tile 32 is one LDS block, 18 has no vector path and overhangs its block, 40 has the vector path and partial blocks
on both axes (the overhang of a partial block is where a transposing view can go wrong), 32 x 16 is the plain views off the
square, and the 16 x 16 cases have more work items than the capped grid has workgroups, so its loop wraps."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tta_reference as TR  # noqa: E402

from change3d_amd import infer, ops  # noqa: E402
from change3d_amd._lib import Change3DHipError  # noqa: E402
from change3d_amd.data.transforms import BCDTransforms as BT  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SINGLES = [(v,) for v in range(8)]
PLAIN = [(v,) for v in range(4)] + [TR.SETS["hflip"], TR.SETS["flips"]]
SQUARE = SINGLES + [TR.SETS["hflip"], TR.SETS["flips"], TR.SETS["d4"], (0, 3, 5)]
GRID_CAP = 256 * 8                                                        # workgroups of either kernel's largest grid


def _scene(Hs, Ws):
    return np.random.default_rng(Hs * 1000 + Ws).integers(0, 256, size=(Hs, Ws, 6), dtype=np.uint8)


def _origins(Hs, Ws, th, tw, sy, sx):
    py, px = infer.axis_plan(Hs, th, sy), infer.axis_plan(Ws, tw, sx)
    return np.stack([np.repeat(py.starts, px.n), np.tile(px.starts, py.n)], axis=1).astype(np.int32)


def _consts():
    return torch.tensor(BT.DEFAULT_MEAN, device=DEV), torch.tensor(BT.DEFAULT_STD, device=DEV)


def _plain_gather(scene, origins, th, tw):
    n = len(origins)
    pre, post = torch.empty((n, 3, th, tw), device=DEV), torch.empty((n, 3, th, tw), device=DEV)
    ops.scene_gather(scene, origins, *_consts(), pre, post, scene.shape[0], scene.shape[1], n, th, tw)
    return pre.cpu().numpy(), post.cpu().numpy()


def _views_gather(scene, origins, th, tw, codes, misalign=False):
    """(pre, post) of c3d_scene_gather_views in NaN-filled buffers with one float of slack on either side."""
    n, nv = len(origins), len(codes)
    count = n * nv * 3 * th * tw
    bufs = [torch.full((count + 8,), float("nan"), device=DEV) for _ in range(2)]
    at = 5 if misalign else 4                                             # torch allocations are 16-byte aligned and beyond
    pre, post = (b[at:at + count].view(n * nv, 3, th, tw) for b in bufs)
    assert (pre.data_ptr() % 16 != 0) == misalign
    ops.scene_gather_views(scene, origins, *_consts(), pre, post, scene.shape[0], scene.shape[1], n, th, tw, TR.mask_of(codes))
    kernel = ops.last_kernel()
    for b in bufs:                                                        # nothing outside the outputs was written
        assert bool(torch.isnan(b[:at]).all()) and bool(torch.isnan(b[at + count:]).all())
    return pre.cpu(), post.cpu(), kernel


def _check_gather(Hs, Ws, th, tw, sy, sx, sets, vector):
    scene = torch.from_numpy(_scene(Hs, Ws)).to(DEV)
    origins = torch.from_numpy(_origins(Hs, Ws, th, tw, sy, sx)).to(DEV)
    base = _plain_gather(scene, origins, th, tw)
    for codes in sets:
        pre, post, kernel = _views_gather(scene, origins, th, tw, codes)
        assert kernel == f"scene_gather_views_kernel<{'true' if vector else 'false'}>", kernel
        for got, plain in ((pre, base[0]), (post, base[1])):
            assert torch.equal(got, torch.from_numpy(TR.gather_views(plain, codes))), (codes, Hs, Ws, th, tw, sy)


@pytest.mark.parametrize("s", [32, 16])
@pytest.mark.parametrize("size", [(50, 70), (33, 37), (9, 100)])
def test_gather_views_are_the_views_of_the_plain_gather(size, s):
    _check_gather(*size, 32, 32, s, s, SQUARE, vector=True)


@pytest.mark.parametrize("t,vector", [(18, False), (40, True)])
def test_gather_views_with_partial_lds_blocks(t, vector):
    """18: scalar stores, one block that overhangs by 14; 40: vector stores, 2 x 2 blocks of which three are partial."""
    _check_gather(50, 70, t, t, t, t, SQUARE, vector)
    _check_gather(33, 37, t, t, t - 6, t - 6, [TR.SETS["d4"]], vector)


def test_gather_views_off_the_square():
    _check_gather(50, 70, 32, 16, 32, 16, PLAIN, vector=True)
    _check_gather(50, 70, 32, 16, 16, 8, [TR.SETS["flips"]], vector=True)
    scene = torch.from_numpy(_scene(50, 70)).to(DEV)
    origins = torch.from_numpy(_origins(50, 70, 32, 16, 32, 16)).to(DEV)
    n = len(origins)
    pre, post = torch.empty((n * 8, 3, 32, 16), device=DEV), torch.empty((n * 8, 3, 32, 16), device=DEV)
    for mask in (0x10, 0x21, 0xff, 0, 0x100, -1):                         # a transposing view off the square; no view; bits above 7
        with pytest.raises(Change3DHipError, match="code -1"):            # C3D_E_BADARG
            ops.scene_gather_views(scene, origins, *_consts(), pre, post, 50, 70, n, 32, 16, mask)
    with pytest.raises(Change3DHipError, match="code -1"):
        ops.scene_gather_views(scene, origins, *_consts(), pre, post, 50, 70, n, 16, 16, 0x1ff)


def test_gather_views_misaligned_output_takes_the_scalar_path():
    scene = torch.from_numpy(_scene(50, 70)).to(DEV)
    origins = torch.from_numpy(_origins(50, 70, 32, 32, 16, 16)).to(DEV)
    base = _plain_gather(scene, origins, 32, 32)
    codes = TR.SETS["d4"]
    pre, post, kernel = _views_gather(scene, origins, 32, 32, codes, misalign=True)
    assert kernel == "scene_gather_views_kernel<false>", kernel
    assert torch.equal(pre, torch.from_numpy(TR.gather_views(base[0], codes)))
    assert torch.equal(post, torch.from_numpy(TR.gather_views(base[1], codes)))


def test_gather_views_grid_wraps_and_two_runs_agree():
    """2100 tiles of 16 x 16 (one block each) against a grid capped at 2048 workgroups; origins anywhere, the fold clamps."""
    Hs, Ws, t, n = 61, 83, 16, GRID_CAP + 52
    rng = np.random.default_rng(3)
    scene = torch.from_numpy(_scene(Hs, Ws)).to(DEV)
    origins = torch.from_numpy(rng.integers(-40, 100, size=(n, 2)).astype(np.int32)).to(DEV)
    base = _plain_gather(scene, origins, t, t)
    codes = TR.SETS["d4"]
    pre, post, _ = _views_gather(scene, origins, t, t, codes)
    assert torch.equal(pre, torch.from_numpy(TR.gather_views(base[0], codes)))
    assert torch.equal(post, torch.from_numpy(TR.gather_views(base[1], codes)))
    pre2, post2, _ = _views_gather(scene, origins, t, t, codes)
    assert torch.equal(pre, pre2) and torch.equal(post, post2)


# --------------------------------------------------------------------------------------------------------------- fold
def _fold(values, cnt, C, th, tw, codes, misalign=False):
    """c3d_scene_fold_views into the slot range ring[1, 2:2 + cnt] of a NaN-filled ring [3, cnt + 4, C, th, tw]."""
    ring = torch.full((3 * (cnt + 4) * C * th * tw + 4,), float("nan"), device=DEV)
    ring = ring[1:1 - 4].view(3, cnt + 4, C, th, tw) if misalign else ring[:-4].view(3, cnt + 4, C, th, tw)
    dst = ring[1, 2:2 + cnt]
    assert dst.is_contiguous() and dst.data_ptr() != ring.data_ptr()
    ops.scene_fold_views(torch.from_numpy(values).to(DEV), dst, cnt, C, th, tw, TR.mask_of(codes))
    kernel = ops.last_kernel()
    outside = torch.ones(ring.shape[:2], dtype=torch.bool)
    outside[1, 2:2 + cnt] = False
    assert bool(torch.isnan(ring.cpu()[outside]).all()) and not bool(torch.isnan(dst).any())    # the rest of the ring is untouched
    return dst.cpu(), kernel


def _values(cnt, nv, C, th, tw, seed=0):
    return np.random.default_rng(seed + cnt * 3 + nv * 5 + C * 7 + th * 11 + tw).standard_normal((cnt * nv, C, th, tw)).astype(np.float32)


def _check_fold(cnt, C, th, tw, codes, vector):
    values = _values(cnt, len(codes), C, th, tw)
    got, kernel = _fold(values, cnt, C, th, tw, codes)
    assert kernel == f"scene_fold_views_kernel<{'true' if vector else 'false'}>", kernel
    assert torch.equal(got, torch.from_numpy(TR.fold32(values, codes))), (cnt, C, th, tw, codes)
    if codes == (0,):
        assert torch.equal(got, torch.from_numpy(values))                 # view_mask == 1 copies bit for bit
    if 5 in codes or 6 in codes:                                          # control: V in place of V^-1 is another map
        assert not torch.equal(got, torch.from_numpy(TR.fold32(values, codes, invert=False)))
    if codes == TR.SETS["d4"]:                                            # control: the order of the adds is visible
        assert not torch.equal(got, torch.from_numpy(TR.fold32(values, codes, descending=True)))
    return values, got


@pytest.mark.parametrize("t,vector", [(32, True), (18, False), (40, True)])
@pytest.mark.parametrize("cnt", [1, 5])
@pytest.mark.parametrize("C", [1, 7])
def test_fold_is_the_f32_mean_of_the_inverted_views(C, cnt, t, vector):
    for codes in SQUARE:
        _check_fold(cnt, C, t, t, codes, vector)


@pytest.mark.parametrize("C,cnt", [(1, 5), (7, 1)])
def test_fold_off_the_square(C, cnt):
    for codes in PLAIN:
        _check_fold(cnt, C, 32, 16, codes, vector=True)
    values = torch.zeros((cnt * 8, C, 32, 16), device=DEV)
    dst = torch.zeros((cnt, C, 32, 16), device=DEV)
    for mask in (0x10, 0xff, 0, 0x100):
        with pytest.raises(Change3DHipError, match="code -1"):
            ops.scene_fold_views(values[:cnt * ops.view_count(mask)], dst, cnt, C, 32, 16, mask)


def test_fold_misaligned_ring_takes_the_scalar_path():
    values = _values(2, 8, 3, 32, 32)
    got, kernel = _fold(values, 2, 3, 32, 32, TR.SETS["d4"], misalign=True)
    assert kernel == "scene_fold_views_kernel<false>", kernel
    assert torch.equal(got, torch.from_numpy(TR.fold32(values, TR.SETS["d4"])))


def test_fold_grid_wraps_and_two_runs_agree():
    """300 entries x 7 channels of one 16 x 16 block each: 2100 work items against 2048 workgroups."""
    cnt, C, t = 300, 7, 16
    assert cnt * C > GRID_CAP
    values, got = _check_fold(cnt, C, t, t, (0, 3, 5), vector=True)
    again, _ = _fold(values, cnt, C, t, t, (0, 3, 5))
    assert torch.equal(got, again)
    values, got = _check_fold(5, 7, 40, 40, TR.SETS["d4"], vector=True)
    again, _ = _fold(values, 5, 7, 40, 40, TR.SETS["d4"])
    assert torch.equal(got, again)
