"""The restatement of the distance transform and the boundary counts (tests/edt_reference.py) against scipy and against the
definition, the host arithmetic of the boundary scores, and the C-ABI surface of the new entries.  No GPU."""
import ctypes as C
import os

import numpy as np
import pytest

import sys
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import edt_reference as R  # noqa: E402

from change3d_amd import _lib as L  # noqa: E402
from change3d_amd import ops  # noqa: E402
from change3d_amd.boundary_metrics import scores_from_totals  # noqa: E402

SHAPES = [(1, 1), (1, 37), (37, 1), (37, 53), (65, 130), (60, 90), (50, 70)]
DENSITIES = [0.02, 0.3, 0.9, 0.999]


def _mask(shape, density, seed):
    """u8, nonzero with probability `density`; at least one zero, so that scipy's transform has a site."""
    m = (np.random.default_rng(seed).random(shape) < density).astype(np.uint8) * 3
    m.flat[(seed * 7) % m.size] = 0
    return m


def _scipy2(mask):
    ndimage = pytest.importorskip("scipy.ndimage")
    return np.rint(ndimage.distance_transform_edt(mask) ** 2).astype(np.int64)


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("density", DENSITIES)
def test_restatement_equals_scipy(shape, density):
    m = _mask(shape, density, seed=shape[0] * 131 + shape[1])
    assert np.array_equal(R.edt2(m), _scipy2(m))
    if (m == 0).sum() < m.size:                              # INVERT: the transform of mask == 0
        assert np.array_equal(R.edt2(m, invert=True), _scipy2(m == 0))
    padded = _scipy2(np.pad(m, 1))[1:-1, 1:-1]               # BORDER: one ring of sites around the scene
    assert np.array_equal(R.edt2(m, border=True), padded)
    assert np.array_equal(R.edt2(m, invert=True, border=True), _scipy2(np.pad(m == 0, 1))[1:-1, 1:-1])


@pytest.mark.parametrize("shape", [(1, 1), (1, 37), (37, 1), (9, 14), (37, 53)])
def test_restatement_equals_the_definition(shape):
    for density in (0.05, 0.6, 0.98):
        m = _mask(shape, density, seed=shape[1])
        for invert in (False, True):
            for border in (False, True):
                assert np.array_equal(R.edt2(m, invert, border), R.brute2(m, invert, border)), (density, invert, border)


def test_cap_rule():
    m = _mask((37, 53), 0.97, seed=5)
    full = R.edt2(m)
    assert full.max() > 25
    for cap2 in (1, 4, 25):
        capped = R.edt2(m, cap2=cap2)
        assert np.array_equal(capped[full <= cap2], full[full <= cap2]) and (capped[full > cap2] == R.FAR).all()
        assert (full == cap2).any() and not np.array_equal(capped, R.edt2(m, cap2=cap2, cap_strict=True))
    assert np.array_equal(R.edt2(m, cap2=0), full) and np.array_equal(R.edt2(m, cap2=10 ** 9), full)


def test_no_site_rule():
    ones, zeros = np.ones((9, 14), np.uint8), np.zeros((9, 14), np.uint8)
    assert (R.edt2(ones) == R.FAR).all() and (R.edt2(zeros, invert=True) == R.FAR).all() and (R.edt2(ones, cap2=4) == R.FAR).all()
    assert not R.edt2(zeros).any() and not R.edt2(ones, invert=True).any()
    bordered = R.edt2(ones, border=True)                     # the distance to the outside
    assert bordered[0, 0] == 1 and bordered[4, 6] == 25 and bordered.max() == 25
    assert R.FAR == L.EDT_FAR == 0x3fffffff > 2 * 16383 ** 2 and (R.INVERT, R.BORDER) == (L.EDT_INVERT, L.EDT_BORDER)


def test_boundary_radius2():
    assert [ops.boundary_radius2(r) for r in (1, 1.5, 2, 2.9, 5, 1024)] == [1, 2, 4, 8, 25, 1 << 20]
    assert ops.boundary_radius2(0.5) == 0 and ops.boundary_radius2(1024.0) == L.BOUNDARY_R2_MAX
    for bad in (0, -1, 1024.5, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            ops.boundary_radius2(bad)


def test_scores_from_totals():
    s = scores_from_totals([38, 514, 140, 69, 140, 70, 1, 0])
    p, r = 69 / 140, 70 / 140
    assert s["boundary_iou"] == 38 / 514 and s["boundary_precision"] == p and s["boundary_recall"] == r
    assert s["boundary_f1"] == 2 * p * r / (p + r) and s["scenes"] == 1 and s["inter"] == 38 and s["hit_g"] == 70
    z = scores_from_totals([0] * 8)
    assert [z[k] for k in ("boundary_iou", "boundary_precision", "boundary_recall", "boundary_f1")] == [0.0] * 4
    e = scores_from_totals([0, 276, 140, 0, 0, 0, 1, 0])      # an empty ground truth: no recall, no hit
    assert [e[k] for k in ("boundary_iou", "boundary_precision", "boundary_recall", "boundary_f1")] == [0.0] * 4
    big = scores_from_totals(np.array([2 ** 40, 2 ** 41, 3, 3, 5, 5, 9, 0], dtype=np.int64))
    assert big["boundary_iou"] == 0.5 and big["boundary_f1"] == 1.0 and isinstance(big["inter"], int)


def test_fixed_counts_of_two_discs():
    shape = (96, 120)
    A, B = R.disc(shape, 40, 50, 25), R.disc(shape, 42, 53, 25)
    want = {1: (10, 270, 140, 29, 140, 29), 2: (38, 514, 140, 69, 140, 69), 5: (378, 1030, 140, 140, 140, 140)}
    for d, counts in want.items():
        got = R.boundary_counts(A, B, d * d, d * d, border=True)
        assert got[:6] == counts and got[6:] == (1, 0)
    assert R.boundary_counts(A, A, 4, 4)[:6] == (276, 276, 140, 140, 140, 140)
    assert R.boundary_counts(A, np.zeros(shape, np.uint8), 4, 4)[:6] == (0, 276, 140, 0, 0, 0)
    # the border matters only where an object touches the scene's edge
    assert R.boundary_counts(A, B, 4, 4, border=False) == R.boundary_counts(A, B, 4, 4, border=True)
    Q = R.disc((40, 40), 0, 0, 20)
    assert R.boundary_counts(Q, Q, 4, 4, border=False) != R.boundary_counts(Q, Q, 4, 4, border=True)


def test_library_exports_and_header_declare_the_new_entries():
    names = L.check_exports()
    i32, i64, vp = C.c_int32, C.c_int64, C.c_void_p
    assert {"c3d_scene_edt_ws_bytes", "c3d_scene_edt_tile", "c3d_scene_edt", "c3d_boundary_counts_ws_bytes",
            "c3d_boundary_counts"} <= set(names)
    assert L.SIGNATURES["c3d_scene_edt_ws_bytes"] == (i64, [i32, i32]) == L.SIGNATURES["c3d_boundary_counts_ws_bytes"]
    assert L.SIGNATURES["c3d_scene_edt"] == (i32, [vp, i32, i32, i32, i32, vp, vp, vp])
    assert L.SIGNATURES["c3d_boundary_counts"] == (i32, [vp, vp, i32, i32, i32, i32, i32, vp, vp, vp, vp])
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "change3d_hip.h")).read()
    for text in ("int64_t c3d_scene_edt_ws_bytes(", "int c3d_scene_edt_tile(", "int c3d_scene_edt(", "int64_t c3d_boundary_counts_ws_bytes(",
                 "int c3d_boundary_counts(", "#define C3D_EDT_INVERT 1", "#define C3D_EDT_BORDER 2", "#define C3D_EDT_FAR 0x3fffffff"):
        assert text in header, text
    # host-only entries: the size rules and the two extents, without a device
    lib = L.lib()
    assert lib.c3d_scene_edt_ws_bytes(0, 5) == -1 and lib.c3d_scene_edt_ws_bytes(5, -1) == -1
    assert lib.c3d_scene_edt_ws_bytes(16385, 5) == -2 and lib.c3d_boundary_counts_ws_bytes(5, 16385) == -2
    assert lib.c3d_boundary_counts_ws_bytes(0, 1) == -1
    assert 0 < lib.c3d_scene_edt_ws_bytes(1, 1) <= lib.c3d_scene_edt_ws_bytes(16384, 16384) < 2 ** 40
    assert lib.c3d_boundary_counts_ws_bytes(37, 53) > 2 * lib.c3d_scene_edt_ws_bytes(37, 53)
    rows, pixels = ops.scene_edt_tile()
    assert 2 <= rows <= 1024 and 64 <= pixels <= 16384
    assert lib.c3d_scene_edt_tile(None) == -1


def test_predict_scene_parser_refuses_bad_radii(capsys):
    from change3d_amd.scripts.predict_scene import parse_args
    base = ["--weights", "w.pth"]
    args = parse_args(base + ["--boundary", "2.5"])
    assert args.boundary == 2.5 and args.boundary_tol is None
    assert parse_args(base).boundary is None
    assert parse_args(base + ["--boundary", "1024", "--boundary_tol", "1"]).boundary_tol == 1.0
    for bad in (["--boundary", "0"], ["--boundary", "0.5"], ["--boundary", "1025"], ["--boundary", "-2"], ["--boundary", "nan"],
                ["--boundary", "x"], ["--boundary", "2", "--boundary_tol", "0"], ["--boundary_tol", "2"]):
        with pytest.raises(SystemExit) as e:
            parse_args(base + bad)
        assert e.value.code == 2, bad
    capsys.readouterr()
