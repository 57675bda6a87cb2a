"""`c3d_scene_gather` and `c3d_scene_stitch` on the MI355X at t = 32 (the kernels are generic in the tile size): the gather
bit for bit against the oracle's BCD normalisation of np.pad(reflect) crops, the stitch against the float64 scatter of
scene_reference.py under a derived bound, driven strip by strip through the k-slot ring exactly as `predict` does.

The stitch bound.  Per pixel and channel the kernel forms w_j = fl(wy * wx) (one rounding), accumulates num = fma(w_j, p_j,
num) over the `taps` covering tiles (one rounding each), and divides (one rounding); to first order in u = 2^-24 that is
taps + 2 roundings on terms of size w_j |p_j|, and one more unit is left for the denominator, which is a sum of positive
terms taken in the same order: |result - exact| <= (taps + 3) * u * sum(w |p|) / sum(w), taps <= k * k being the number of
tiles that cover the pixel.  (A worst-case count that lets every rounding of the denominator line up against the
numerator's would be 2 * taps + 2; the tighter constant is the one asserted, and the worst measured error / bound of every
case is printed and kept in profiles/scene_infer.txt.)  Where |blend - 0.5| (mask) or the top-two margin (argmax) of the
float64 blend exceeds the bound the u8 outputs must be exact; the pixels left out may be 0.1 % of a case at most."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import scene_reference as R  # noqa: E402

from change3d_amd import infer, ops  # noqa: E402
from change3d_amd._lib import Change3DHipError  # noqa: E402
from change3d_amd.data.transforms import BCDTransforms as BT  # noqa: E402
from oracle import transforms as ot  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
T = 32
SCENES = [(50, 70), (33, 37), (9, 100), (32, 32)]
STRIDES = [32, 16, 24, 8]
CONSTANTS = [(BT.DEFAULT_MEAN, BT.DEFAULT_STD), (BT.IMAGENET_MEAN, BT.IMAGENET_STD)]


def _scene(Hs, Ws):
    return np.random.default_rng(Hs * 1000 + Ws).integers(0, 256, size=(Hs, Ws, 6), dtype=np.uint8)


def _gather(scene, s, mean, std):
    Hs, Ws = scene.shape[:2]
    py, px = infer.axis_plan(Hs, T, s), infer.axis_plan(Ws, T, s)
    origins = np.stack([np.repeat(py.starts, px.n), np.tile(px.starts, py.n)], axis=1).astype(np.int32)
    n = len(origins)
    pre = torch.full((n, 3, T, T), float("nan"), device=DEV)
    post = torch.full((n, 3, T, T), float("nan"), device=DEV)
    ops.scene_gather(torch.from_numpy(scene).to(DEV), torch.from_numpy(origins).to(DEV), torch.tensor(mean, device=DEV),
                     torch.tensor(std, device=DEV), pre, post, Hs, Ws, n, T, T)
    assert ops.last_kernel().startswith("scene_gather_kernel"), ops.last_kernel()
    torch.cuda.synchronize()
    return pre.cpu(), post.cpu()


@pytest.mark.parametrize("s", STRIDES)
@pytest.mark.parametrize("size", SCENES)
def test_gather_is_the_oracle_normalisation_of_np_pad_crops(size, s):
    scene = _scene(*size)
    crops = R.crops(scene, T, T, s, s)
    for mean, std in CONSTANTS:
        pre, post = _gather(scene, s, mean, std)
        want = np.stack([ot.bcd_transform_sample(c, np.zeros((T, T), np.uint8), (0, 0, 0), mean, std)[0] for c in crops])
        assert torch.equal(pre, torch.from_numpy(want[:, 0:3])) and torch.equal(post, torch.from_numpy(want[:, 3:6]))
    pre2, post2 = _gather(scene, s, *CONSTANTS[1])
    assert torch.equal(pre, pre2) and torch.equal(post, post2)                     # two runs: bit-identical


def test_gather_of_one_whole_tile_is_c3d_bcd_preprocess():
    scene = _scene(32, 32)
    for mean, std in CONSTANTS:
        pre, post = _gather(scene, 32, mean, std)
        p, q = torch.empty((1, 3, T, T), device=DEV), torch.empty((1, 3, T, T), device=DEV)
        ops.bcd_preprocess(torch.from_numpy(scene[None]).to(DEV), None, None, torch.tensor(mean, device=DEV),
                           torch.tensor(std, device=DEV), p, q, None, 1, T, T)
        assert torch.equal(pre, p.cpu()) and torch.equal(post, q.cpu())


def test_gather_clamps_whatever_the_table_holds():
    """Origins far outside the scene (the geometry never asks for them) fold back: every output is a scene pixel's value."""
    scene = _scene(33, 37)
    origins = np.array([[-100000, 2 ** 31 - 40], [-2 ** 31, -2 ** 31], [2 ** 31 - 1, 5], [7, -3]], dtype=np.int32)
    n = len(origins)
    pre, post = torch.empty((n, 3, T, T), device=DEV), torch.empty((n, 3, T, T), device=DEV)
    mean, std = CONSTANTS[0]
    ops.scene_gather(torch.from_numpy(scene).to(DEV), torch.from_numpy(origins).to(DEV), torch.tensor(mean, device=DEV),
                     torch.tensor(std, device=DEV), pre, post, 33, 37, n, T, T)
    torch.cuda.synchronize()
    ys = np.stack([[R.fold(int(o[0]) + y, 33) for y in range(T)] for o in origins])
    xs = np.stack([[R.fold(int(o[1]) + x, 37) for x in range(T)] for o in origins])
    for i in range(n):
        crop = scene[ys[i]][:, xs[i]]
        want = ot.bcd_transform_sample(crop, np.zeros((T, T), np.uint8), (0, 0, 0), mean, std)[0]
        assert torch.equal(pre[i].cpu(), torch.from_numpy(want[0:3])) and torch.equal(post[i].cpu(), torch.from_numpy(want[3:6]))


# ------------------------------------------------------------------------------------------------------------- stitch
def _tiles(Hs, Ws, s, C, seed=0):
    rng = np.random.default_rng(seed + Hs * 7 + Ws * 13 + s * 17 + C)
    ny, nx = R.plan(Hs, T, s)[1], R.plan(Ws, T, s)[1]
    if C == 1:
        return rng.random((ny, nx, C, T, T)).astype(np.float32)                   # probabilities
    return rng.standard_normal((ny, nx, C, T, T)).astype(np.float32)              # logits


@functools.lru_cache(maxsize=None)
def _reference(Hs, Ws, s, C, wname_y, wname_x):
    return R.stitch(_tiles(Hs, Ws, s, C), Hs, Ws, s, s, R.window(wname_y, T), R.window(wname_x, T))


def _run_stitch(tiles, Hs, Ws, s, wname_y, wname_x, blend=True):
    """Row by row through the k-slot ring, as SceneInferencer.predict drives it."""
    ny, nx, C = tiles.shape[:3]
    py, px = infer.axis_plan(Hs, T, s), infer.axis_plan(Ws, T, s)
    st = infer.SceneStitcher(py, px, C, wname_y, DEV, blend=blend)
    st.wx = torch.from_numpy(infer.window_vector(wname_x, T)).to(DEV)
    st.ring.fill_(float("nan"))                                                   # a slot read before it is written shows
    if st.blend is not None:
        st.blend.fill_(float("nan"))
    st.cls.fill_(255)
    dt = torch.from_numpy(tiles).to(DEV)
    launched = False
    for row in range(ny):
        st.put(row, 0, dt[row])
        before = ops.launch_count()
        st.stitch(row)
        if ops.launch_count() > before:
            launched = True
            assert ops.last_kernel().startswith("scene_stitch_kernel"), ops.last_kernel()
    assert launched
    torch.cuda.synchronize()
    return (st.blend.cpu().numpy() if blend else None), st.cls.cpu().numpy()


def _check_outputs(tag, blend, cls, ref, C):
    lim = R.bound(ref)
    err = np.abs(blend.astype(np.float64) - ref["blend"])
    ratio = float((err / lim).max())
    print(f"PARITY {tag}: max |err| {err.max():.3e}  max bound {lim.max():.3e}  worst err/bound {ratio:.3f}  "
          f"taps <= {int(ref['taps'].max())}")
    assert np.isfinite(blend).all() and (err <= lim).all(), (tag, ratio)
    if C == 1:
        decided = np.abs(ref["blend"][0] - 0.5) > lim[0]
        want = (ref["blend"][0] > 0.5).astype(np.uint8)
    else:
        order = np.argsort(ref["blend"], axis=0)
        top, second = order[-1], order[-2]
        take = lambda a, i: np.take_along_axis(a, i[None], axis=0)[0]  # noqa: E731
        decided = take(ref["blend"], top) - take(ref["blend"], second) > take(lim, top) + take(lim, second)
        want = top.astype(np.uint8)
    share = 1.0 - decided.mean()
    assert share <= 1e-3, (tag, share)
    assert np.array_equal(cls[decided], want[decided]), tag
    return ratio, share


@pytest.mark.parametrize("s", STRIDES)
@pytest.mark.parametrize("size", SCENES)
def test_stitch_against_the_float64_scatter(size, s):
    Hs, Ws = size
    for C in (1, 6):
        tiles = _tiles(Hs, Ws, s, C)
        for wy, wx in (("hann", "hann"), ("flat", "flat"), ("hann", "flat")):     # the last: wy and wx must not be mixed up
            ref = _reference(Hs, Ws, s, C, wy, wx)
            blend, cls = _run_stitch(tiles, Hs, Ws, s, wy, wx)
            _check_outputs(f"{Hs}x{Ws} s={s} C={C} {wy}/{wx}", blend, cls, ref, C)
            if (wy, wx) == ("hann", "hann"):
                blend2, cls2 = _run_stitch(tiles, Hs, Ws, s, wy, wx)               # two runs: bit-identical
                assert np.array_equal(blend.view(np.uint32), blend2.view(np.uint32)) and np.array_equal(cls, cls2)
                _, cls3 = _run_stitch(tiles, Hs, Ws, s, wy, wx, blend=False)       # u8 output alone
                assert np.array_equal(cls, cls3)


def test_argmax_tie_picks_the_lower_index():
    Hs, Ws, s = 50, 70, 16
    tiles = _tiles(Hs, Ws, s, 6).copy()
    tiles[:, :, 4] = tiles[:, :, 2] = np.abs(tiles[:, :, 2]) + 10.0                # channels 2 and 4 equal and largest
    blend, cls = _run_stitch(tiles, Hs, Ws, s, "hann", "hann")
    assert np.array_equal(blend[2].view(np.uint32), blend[4].view(np.uint32)) and (cls == 2).all()


def test_gate_multiplies_the_class_map():
    Hs, Ws, s = 33, 37, 24
    tiles = _tiles(Hs, Ws, s, 6)
    _, cls = _run_stitch(tiles, Hs, Ws, s, "hann", "hann")
    py, px = infer.axis_plan(Hs, T, s), infer.axis_plan(Ws, T, s)
    st = infer.SceneStitcher(py, px, 6, "hann", DEV)
    gate = torch.from_numpy((np.random.default_rng(1).random((Hs, Ws)) < 0.5).astype(np.uint8)).to(DEV)
    dt = torch.from_numpy(tiles).to(DEV)
    for row in range(py.n):
        st.put(row, 0, dt[row])
        st.stitch(row, gate=gate)
    torch.cuda.synchronize()
    assert np.array_equal(st.cls.cpu().numpy(), cls * gate.cpu().numpy())


def test_refusals():
    py, px = infer.axis_plan(50, T, 16), infer.axis_plan(70, T, 16)
    st = infer.SceneStitcher(py, px, 1, "hann", DEV)
    for kw in (dict(sy=15), dict(sy=33), dict(sy=0), dict(row=4), dict(row=-1), dict(C=0)):
        a = dict(Hs=50, Ws=70, C=1, th=T, tw=T, sy=16, sx=16, row=0)
        a.update(kw)
        with pytest.raises(Change3DHipError):
            ops.scene_stitch(st.ring, st.wy, st.wx, None, st.cls, **a)
    with pytest.raises(Change3DHipError):
        ops.scene_stitch(st.ring, st.wy, st.wx, None, None, 50, 70, 1, T, T, 16, 16, 0)
    # a ring of 2 GiB or more is refused before anything is launched (the pointers are never followed)
    with pytest.raises(Change3DHipError, match="-2"):
        ops.scene_stitch(st.ring, st.wy, st.wx, None, st.cls, 4096, 40000, 16, 256, 256, 128, 128, 0)
    with pytest.raises(Change3DHipError, match="2 GiB"):
        infer.SceneStitcher(infer.axis_plan(4096, 256, 128), infer.axis_plan(40000, 256, 128), 16, "hann", DEV)


# ---------------------------------------------------------------------------------------- the two axes are independent
@pytest.mark.parametrize("size", [(33, 37), (50, 70)])
def test_non_square_tile_and_two_strides(size):
    """th = 32, tw = 16 with strides 16 and 8 (ky = kx = 2, my = 8, mx = 4): a th / tw or sy / sx mix-up anywhere in the
    kernels' indexing, in the window staging or in SceneStitcher.put moves pixels and fails here."""
    Hs, Ws = size
    th, tw, sy, sx = 32, 16, 16, 8
    scene = _scene(Hs, Ws)
    py, px = infer.axis_plan(Hs, th, sy), infer.axis_plan(Ws, tw, sx)
    origins = np.stack([np.repeat(py.starts, px.n), np.tile(px.starts, py.n)], axis=1).astype(np.int32)
    n = len(origins)
    mean, std = CONSTANTS[0]
    pre, post = torch.full((n, 3, th, tw), float("nan"), device=DEV), torch.full((n, 3, th, tw), float("nan"), device=DEV)
    ops.scene_gather(torch.from_numpy(scene).to(DEV), torch.from_numpy(origins).to(DEV), torch.tensor(mean, device=DEV),
                     torch.tensor(std, device=DEV), pre, post, Hs, Ws, n, th, tw)
    torch.cuda.synchronize()
    want = np.stack([ot.bcd_transform_sample(c, np.zeros((th, tw), np.uint8), (0, 0, 0), mean, std)[0]
                     for c in R.crops(scene, th, tw, sy, sx)])
    assert torch.equal(pre.cpu(), torch.from_numpy(want[:, 0:3])) and torch.equal(post.cpu(), torch.from_numpy(want[:, 3:6]))
    for C in (1, 6):
        rng = np.random.default_rng(Hs + C)
        shape = (py.n, px.n, C, th, tw)
        tiles = (rng.random(shape) if C == 1 else rng.standard_normal(shape)).astype(np.float32)
        ref = R.stitch(tiles, Hs, Ws, sy, sx, R.window("hann", th), R.window("hann", tw))
        st = infer.SceneStitcher(py, px, C, "hann", DEV, blend=True)
        st.ring.fill_(float("nan"))
        st.blend.fill_(float("nan"))
        dt = torch.from_numpy(tiles).to(DEV)
        for row in range(py.n):
            st.put(row, 0, dt[row])
            st.stitch(row)
        torch.cuda.synchronize()
        _check_outputs(f"{Hs}x{Ws} t={th}x{tw} s={sy}x{sx} C={C} hann/hann", st.blend.cpu().numpy(), st.cls.cpu().numpy(), ref, C)
