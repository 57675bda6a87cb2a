"""`c3d_scene_edt` against its restatement (tests/edt_reference.py): every value equal, through the C entry with canary rows
around `dist2`.  All four flag combinations and caps 0, 1, 4 and 25 on the smallest shapes that reach every path -- both sides
of the rows of a column-pass chunk and of the pixels of a row-pass workgroup -- and on hand-made contents; a dirty workspace,
a non-default stream, the refusals, and a negative control for the cap rule."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import edt_reference as R  # noqa: E402

from change3d_amd import _lib as L  # noqa: E402
from change3d_amd import ops  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
PAD, CANARY = 2, -7777
CAPS = (0, 1, 4, 25)
FLAGS = (0, R.INVERT, R.BORDER, R.INVERT | R.BORDER)


def _edt(mask, flags, cap2, ws=None, fill_ws=None, d_mask=None):
    """The C entry on an output with canary rows on both sides: (rc, dist2 as numpy)."""
    Hs, Ws = mask.shape
    d_mask = torch.from_numpy(np.ascontiguousarray(mask)).to(DEV) if d_mask is None else d_mask
    out = torch.full((Hs + 2 * PAD, Ws), CANARY, dtype=torch.int32, device=DEV)
    if ws is None:
        ws = torch.empty(L.lib().c3d_scene_edt_ws_bytes(Hs, Ws), dtype=torch.uint8, device=DEV)
    if fill_ws is not None:
        ws.fill_(fill_ws)
    rc = L.lib().c3d_scene_edt(d_mask.data_ptr(), Hs, Ws, flags, cap2, out[PAD:].data_ptr(), ws.data_ptr(),
                               torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    out = out.cpu().numpy()
    assert (out[:PAD] == CANARY).all() and (out[Hs + PAD:] == CANARY).all(), "a canary row was written"
    return rc, out[PAD:Hs + PAD]


def _check_all(mask, flags=FLAGS, caps=CAPS):
    """Every flag combination and cap on one mask: the uncapped restatement once per flags, the cap rule on top of it."""
    d_mask = torch.from_numpy(np.ascontiguousarray(mask)).to(DEV)
    for f in flags:
        full = R.edt2(mask, invert=bool(f & R.INVERT), border=bool(f & R.BORDER))
        for cap2 in caps:
            rc, got = _edt(mask, f, cap2, d_mask=d_mask)
            want = R.apply_cap(full, cap2)
            assert rc == 0 and np.array_equal(got, want), (mask.shape, f, cap2, np.argwhere(got != want)[:5])


TILE = functools.lru_cache(maxsize=None)(lambda: ops.scene_edt_tile())


def _shapes():
    """By name, so that collection needs no device: T = (rows of a chunk, pixels of a row-pass workgroup)."""
    names = ["1x1", "1x37", "37x1", "37x53", "3x2500", "2500x3"]
    names += [f"rows:{k}" for k in ("T-1", "T", "T+1", "2T+3")] + [f"cols:{k}" for k in ("T-1", "T", "T+1", "2T+3")]
    return names


def _shape_of(name):
    if ":" not in name:
        return tuple(int(v) for v in name.split("x"))
    axis, k = name.split(":")
    T = TILE()[0 if axis == "rows" else 1]
    n = {"T-1": T - 1, "T": T, "T+1": T + 1, "2T+3": 2 * T + 3}[k]
    return (n, 70) if axis == "rows" else (5, n)


@pytest.mark.parametrize("name", _shapes())
def test_random_masks_on_every_path(name):
    shape = _shape_of(name)
    assert 2 <= TILE()[0] and 64 <= TILE()[1] <= 16384
    for k, density in enumerate((0.01, 0.5, 0.99)):
        rng = np.random.default_rng(1000 * shape[0] + shape[1] + k)
        _check_all((rng.random(shape) < density).astype(np.uint8) * 255)


def _contents():
    yy, xx = np.mgrid[0:40, 0:50]
    corner = np.ones((200, 300), np.uint8)
    corner[0, 0] = 0                                        # the long uncapped search: every pixel walks to column 0
    far_corner = np.ones((200, 300), np.uint8)
    far_corner[199, 299] = 0
    two = np.ones((9, 21), np.uint8)
    two[4, 2] = two[4, 18] = 0                              # (4, 10) is 64 from both
    sparse = np.ones((200, 300), np.uint8)
    for y, x in ((13, 31), (57, 222), (101, 140), (160, 17), (188, 290)):
        sparse[y, x] = 0                                    # the nearest site of most pixels lies in neither their row nor column
    return {"all_zero": np.zeros((37, 53), np.uint8), "all_nonzero": np.full((37, 53), 7, np.uint8), "corner_site": corner,
            "far_corner_site": far_corner, "two_equidistant": two, "checkerboard": ((yy + xx) % 2).astype(np.uint8),
            "five_sparse_sites": sparse}


@pytest.mark.parametrize("name", list(_contents()))
def test_hand_made_contents(name):
    mask = _contents()[name]
    _check_all(mask)
    if name == "all_nonzero":
        assert (_edt(mask, 0, 0)[1] == R.FAR).all() and (_edt(mask, 0, 4)[1] == R.FAR).all()
        assert _edt(mask, R.BORDER, 0)[1].max() == 19 * 19
    if name == "two_equidistant":
        assert _edt(mask, 0, 0)[1][4, 10] == 64
    if name == "corner_site":
        assert _edt(mask, 0, 0)[1][199, 299] == 199 ** 2 + 299 ** 2


def test_sites_far_apart_in_a_tall_and_in_a_wide_scene():
    """Carries across many chunks and a search across several workgroups' segments, uncapped and at a cap that reaches neither."""
    rows, pixels = TILE()
    tall = np.ones((5 * rows + 7, 3), np.uint8)
    tall[0, 1] = tall[-1, 0] = 0
    wide = np.ones((3, 2 * pixels + 77), np.uint8)
    wide[1, 0] = wide[2, -1] = 0
    for mask in (tall, wide):
        _check_all(mask, caps=(0, 25, (rows + 3) ** 2, 10 ** 9))


def test_two_runs_agree_bit_for_bit_also_on_a_dirty_workspace():
    rng = np.random.default_rng(3)
    mask = (rng.random((131, 1100)) < 0.9).astype(np.uint8)
    ws = torch.empty(L.lib().c3d_scene_edt_ws_bytes(*mask.shape), dtype=torch.uint8, device=DEV)
    for flags, cap2 in ((0, 0), (R.BORDER, 25), (R.INVERT, 4)):
        first = _edt(mask, flags, cap2, ws=ws, fill_ws=0)
        again = _edt(mask, flags, cap2, ws=ws)                # what the first call left behind
        dirty = _edt(mask, flags, cap2, ws=ws, fill_ws=0xFF)
        assert first[0] == again[0] == dirty[0] == 0
        assert first[1].tobytes() == again[1].tobytes() == dirty[1].tobytes()
        assert np.array_equal(first[1], R.edt2(mask, bool(flags & R.INVERT), bool(flags & R.BORDER), cap2))


def test_non_default_stream_and_the_python_op():
    rng = np.random.default_rng(4)
    mask = (rng.random((70, 90)) < 0.8).astype(np.uint8)
    d_mask = torch.from_numpy(mask).to(DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        plain = ops.scene_edt(d_mask)
        out = torch.empty((70, 90), dtype=torch.int32, device=DEV)
        ws = torch.empty(L.lib().c3d_scene_edt_ws_bytes(70, 90) + 64, dtype=torch.uint8, device=DEV)
        same = ops.scene_edt(d_mask, invert=True, border=True, cap2=25, out=out, ws=ws)
    side.synchronize()
    assert same is out and plain.dtype == torch.int32 and plain.shape == (70, 90)
    assert np.array_equal(plain.cpu().numpy(), R.edt2(mask))
    assert np.array_equal(out.cpu().numpy(), R.edt2(mask, invert=True, border=True, cap2=25))
    with pytest.raises(L.Change3DHipError):
        ops.scene_edt(d_mask.cpu())
    with pytest.raises(ValueError):
        ops.scene_edt(d_mask.to(torch.int32))
    with pytest.raises(ValueError):
        ops.scene_edt(d_mask, cap2=-1)


def test_refusals_leave_the_output_untouched():
    mask = torch.ones((37, 53), dtype=torch.uint8, device=DEV)
    out = torch.full((37, 53), CANARY, dtype=torch.int32, device=DEV)
    ws = torch.empty(L.lib().c3d_scene_edt_ws_bytes(37, 53), dtype=torch.uint8, device=DEV)
    good = dict(mask=mask.data_ptr(), Hs=37, Ws=53, flags=0, cap2=0, dist2=out.data_ptr(), ws=ws.data_ptr())
    stream = torch.cuda.current_stream().cuda_stream
    bad = [(dict(mask=None), -1), (dict(dist2=None), -1), (dict(ws=None), -1), (dict(flags=4), -1), (dict(flags=-1), -1),
           (dict(flags=7), -1), (dict(cap2=-1), -1), (dict(cap2=-2 ** 31), -1), (dict(Hs=0), -1), (dict(Ws=0), -1), (dict(Hs=-3), -1),
           (dict(Hs=16385), -2), (dict(Ws=16385), -2), (dict(Hs=2 ** 31 - 1), -2)]
    before = ops.launch_count()
    for change, code in bad:
        assert L.lib().c3d_scene_edt(*{**good, **change}.values(), stream) == code, change
    torch.cuda.synchronize()
    assert (out == CANARY).all() and ops.launch_count() == before
    assert L.lib().c3d_scene_edt_ws_bytes(16384, 16384) > 0 and L.lib().c3d_scene_edt_ws_bytes(16385, 1) == -2
    assert L.lib().c3d_scene_edt(*{**good, "flags": 3, "cap2": 2 ** 31 - 1}.values(), stream) == 0      # the largest of both
    torch.cuda.synchronize()
    assert ops.launch_count() == before + 3
    assert np.array_equal(out.cpu().numpy(), R.edt2(np.ones((37, 53), np.uint8), invert=True, border=True))


def test_negative_control_sees_the_cap_rule():
    rng = np.random.default_rng(6)
    mask = (rng.random((37, 53)) < 0.97).astype(np.uint8)
    full = R.edt2(mask)
    assert (full == 4).any() and (full > 4).any()
    rc, got = _edt(mask, 0, 4)
    assert rc == 0 and np.array_equal(got, R.apply_cap(full, 4))
    assert not np.array_equal(got, R.apply_cap(full, 4, cap_strict=True)), "a value equal to the cap is kept"
