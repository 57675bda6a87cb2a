"""Whole-scene tiling without a GPU: geometry properties, the reflect fold against np.pad itself, the window, refusals, and
negative controls that show the GPU bound of test_scene_ops_gpu.py tells a wrong stitch from a right one."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import scene_reference as R  # noqa: E402

from change3d_amd import infer  # noqa: E402
from change3d_amd._lib import Change3DHipError  # noqa: E402

GRID = [(extent, t, s) for extent in (1, 5, 9, 32, 33, 37, 50, 70, 100) for t, s in ((32, 32), (32, 16), (32, 24), (32, 8), (7, 3), (6, 6))]


@pytest.mark.parametrize("extent,t,s", GRID)
def test_axis_plan_properties(extent, t, s):
    p = infer.axis_plan(extent, t, s)
    m, n, k, starts = R.plan(extent, t, s)
    assert (p.margin, p.n, p.k, list(p.starts)) == (m, n, k, starts)
    cover = np.zeros(extent, dtype=np.int64)
    central = np.zeros(extent, dtype=np.int64)
    for st in starts:
        for y in range(extent):
            cover[y] += st <= y < st + t
            central[y] += st + m <= y < st + m + s
    assert (central == 1).all()                       # every pixel lies in exactly one tile's central region
    assert cover.max() <= k and cover.min() >= 1      # so at most k x k tiles cover a pixel of the scene
    # strips: disjoint, in order, the whole axis; a strip's rows are covered by tile rows i-k+1 .. i only
    edge = 0
    for i in range(n):
        y0, y1 = infer.strip_rows(p, i)
        if y1 > y0:
            assert y0 == edge
            edge = y1
        for y in range(y0, y1):
            rows = [r for r, st in enumerate(starts) if st <= y < st + t]
            assert max(rows) <= i and min(rows) >= i - k + 1, (y, rows, i)
    assert edge == extent


@pytest.mark.parametrize("extent", [1, 2, 3, 9, 37])
def test_fold_is_np_pad_reflect_for_any_overhang(extent):
    over = 3 * extent + 5                             # larger than the extent: several reflections
    want = np.pad(np.arange(extent), (over, over), mode="reflect")
    coords = np.arange(-over, extent + over)
    assert np.array_equal(infer.reflect_index(coords, extent), want)
    assert [R.fold(int(c), extent) for c in coords] == list(want)


def test_windows():
    for t in (1, 7, 32, 256):
        h = infer.window_vector("hann", t)
        assert h.dtype == np.float32 and (h > 0).all() and np.array_equal(h, R.window("hann", t))
        assert np.array_equal(h, h[::-1].copy()) or np.allclose(h, h[::-1], rtol=1e-6, atol=0)
        assert np.array_equal(infer.window_vector("flat", t), np.ones(t, dtype=np.float32))
    with pytest.raises(ValueError):
        infer.window_vector("cosine", 8)


@pytest.mark.parametrize("t,s", [(32, 31), (32, 33), (32, 0), (32, -2), (8, 5)])
def test_refusals(t, s):
    with pytest.raises(ValueError):
        infer.axis_plan(100, t, s)
    with pytest.raises(ValueError):
        R.plan(100, t, s)


def test_inferencer_refuses_bad_arguments_and_cpu_models():
    from change3d_amd import synthetic as synth
    from change3d_amd.model.trainer import Trainer
    net = Trainer(synth.make_args(size=32))
    for kw in (dict(stride=31), dict(stride=0), dict(stride=34), dict(window="cosine"), dict(batch=0)):
        with pytest.raises(ValueError):
            infer.SceneInferencer(net, "bcd", **kw)
    with pytest.raises(ValueError):
        infer.SceneInferencer(net, "bda")
    inf = infer.SceneInferencer(net, "bcd")
    assert (inf.sy, inf.sx) == (16, 16) and not net.training
    with pytest.raises(Change3DHipError):
        inf.predict(torch.zeros((40, 50, 6), dtype=torch.uint8))      # CPU model: no fallback


def _case(seed, Hs, Ws, t, s, C):
    rng = np.random.default_rng(seed)
    _, ny, _, _ = R.plan(Hs, t, s)
    _, nx, _, _ = R.plan(Ws, t, s)
    tiles = rng.random((ny, nx, C, t, t)).astype(np.float32) if C == 1 else rng.standard_normal((ny, nx, C, t, t)).astype(np.float32)
    return tiles


@pytest.mark.parametrize("C", [1, 6])
@pytest.mark.parametrize("s", [16, 24, 8])
def test_negative_controls_exceed_the_gpu_bound(s, C):
    """A stitch that drops one tap, or that applies the window transposed, is further from the true blend than the bound the
    GPU result must meet -- by orders of magnitude, so the bound can tell them apart."""
    Hs, Ws, t = 50, 70, 32
    tiles = _case(3, Hs, Ws, t, s, C)
    wy, wx = R.window("hann", t), R.window("flat", t)     # two different vectors: outer(v, v) is its own transpose
    true = R.stitch(tiles, Hs, Ws, s, s, wy, wx)
    lim = R.bound(true)
    assert lim.max() < 1e-5
    dropped = R.stitch(tiles, Hs, Ws, s, s, wy, wx, drop_tap=(1, 1))
    turned = R.stitch(tiles, Hs, Ws, s, s, wy, wx, transpose_window=True)
    for wrong in (dropped, turned):
        diff = np.abs(wrong["blend"] - true["blend"])
        diff[np.isnan(diff)] = np.inf                 # a pixel only the dropped tile covered: 0 / 0
        excess = diff - lim
        assert excess.max() > 1e3 * lim.max(), excess.max()
    # the scatter canvas agrees with a direct per-pixel gather in float64 (the definition, restated a third way)
    y, x = 17, 41
    my = (t - s) // 2
    num = den = 0.0
    for i in range(tiles.shape[0]):
        for j in range(tiles.shape[1]):
            ly, lx = y - (i * s - my), x - (j * s - my)
            if 0 <= ly < t and 0 <= lx < t:
                w = float(wy[ly]) * float(wx[lx])
                num, den = num + w * float(tiles[i, j, 0, ly, lx]), den + w
    assert abs(num / den - true["blend"][0, y, x]) < 1e-14
