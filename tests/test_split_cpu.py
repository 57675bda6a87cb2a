"""The restatement that the GPU tests of `c3d_scene_split` compare with (tests/split_reference.py), checked on the host: two
growth algorithms against each other, the core against scipy, the properties of the definition (connected pieces, a
partition, identity at r2 = 0), the figures of the hand-made cases, a negative control; then the parser of predict_scene.py
and the C-ABI surface of the new entries.  No GPU."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import objects_reference as R  # noqa: E402
import split_reference as S  # noqa: E402

from change3d_amd import _lib as L  # noqa: E402
from change3d_amd import ops  # noqa: E402

LIST_SIZE, LIST_TILE = (70, 75), 64


@functools.lru_cache(maxsize=None)
def _cases():
    """list of (name, mask, r2): the hand-made cases at their radius, the masks of `objects_reference.mask_list` at r2 = 1, 4."""
    out = list(S.hand_cases())
    out += [("two_discs", S.two_discs(), r2) for r2 in (25, 144)]
    for name, mask in R.mask_list(*LIST_SIZE, LIST_TILE, LIST_TILE, seed=5):
        out += [(name, mask, 1), (name, mask, 4)]
    return out


@functools.lru_cache(maxsize=None)
def _split(i, connectivity):
    name, mask, r2 = _cases()[i]
    return S.split(mask, r2, connectivity=connectivity, max_objects=mask.size // 2 + 1)


@pytest.mark.parametrize("connectivity", [4, 8])
def test_dijkstra_equals_the_level_synchronous_bfs(connectivity):
    for name, mask, r2 in _cases():
        ids, _ = S.seed_ids(S.core_of(mask, r2), connectivity)
        d0, o0 = S.grow_dijkstra(mask, ids, connectivity)
        d1, o1 = S.grow_bfs(mask, ids, connectivity)
        assert np.array_equal(d0, d1) and np.array_equal(o0, o1), (name, r2)


def test_the_core_equals_scipys_transform_of_the_padded_mask():
    ndimage = pytest.importorskip("scipy.ndimage")
    for name, mask, r2 in _cases():
        d2 = np.rint(ndimage.distance_transform_edt(np.pad(mask, 1))[1:-1, 1:-1] ** 2).astype(np.int64)
        assert np.array_equal(S.core_of(mask, r2), d2 > r2), (name, r2)
        assert np.array_equal(S.core_of(mask, 0), mask != 0)


@pytest.mark.parametrize("connectivity", [4, 8])
def test_pieces_are_connected_and_partition_the_mask(connectivity):
    for i, (name, mask, r2) in enumerate(_cases()):
        out = _split(i, connectivity)
        assert np.array_equal(out["labels"] > 0, mask != 0), (name, r2)                  # min_area = 1: nothing is lost
        assert S.pieces_are_connected(out["labels"], connectivity), (name, r2)
        n = int(out["counts"][0])
        assert int(out["labels"].max()) == n and int(out["table"][:n, 0].sum()) == int((mask != 0).sum())
        assert n >= int(R.components(mask, connectivity).max())                          # splitting never merges
        firsts = out["table"][:n, 6]
        assert np.all(np.diff(firsts) > 0)                                               # raster order of the own first pixel


@pytest.mark.parametrize("connectivity", [4, 8])
def test_radius_zero_is_the_component_labelling(connectivity):
    rng = np.random.default_rng(3)
    for name, mask, _ in _cases():
        cls = rng.integers(0, 6, size=mask.shape, dtype=np.uint8)
        score = rng.random(mask.shape, dtype=np.float32)
        kw = dict(connectivity=connectivity, min_area=2, n_cls=5, first_class=1, max_objects=64)
        want = R.objects(mask, cls, score, **kw)
        got = S.split(mask, 0, cls, score, **kw)
        for k in ("labels", "table", "hist", "object_cls", "counts"):
            assert np.array_equal(got[k], want[k]), (name, k)
        assert int(got["info"][1]) == int(R.components(mask, connectivity).max())


def test_the_figures_of_the_hand_made_cases():
    discs = S.two_discs()
    assert discs.shape == (96, 160)
    for r2 in (25, 144):
        for c in (4, 8):
            out = S.split(discs, r2, connectivity=c)
            assert out["counts"].tolist() == [1, 1] and int(out["table"][0, 0]) == 5423 and int(out["info"][1]) == 1
    assert S.split(discs, 400, connectivity=4)["table"][:3, 0].tolist() == [2728, 2695, 0]
    assert S.split(discs, 400, connectivity=8)["table"][:3, 0].tolist() == [2730, 2693, 0]
    bell = S.split(S.dumbbell(), 4)
    assert bell["counts"].tolist() == [2, 2] and int(bell["info"][1]) == 2 and int(R.components(S.dumbbell()).max()) == 1
    assert abs(int(bell["table"][0, 0]) - int(bell["table"][1, 0])) <= 2                 # the neck is shared out evenly
    grid = S.bridged_grid()
    out = S.split(grid, 4)
    assert int(R.components(grid).max()) == 1 and int(out["info"][1]) == 36 and out["counts"].tolist() == [36, 36]
    ring = S.split(S.ring(), 4)
    n_comp = int(R.components(S.ring()).max())
    assert n_comp == 2 and int(ring["info"][1]) == 2 and ring["counts"].tolist() == [2, 2]
    thin = S.ring().copy()
    thin[12:36, 44:70] = 0                                                               # the ring alone: no seed, one piece
    alone = S.split(thin, 4)
    assert int(alone["info"][1]) == 1 and alone["counts"].tolist() == [2, 2] and int(alone["labels"][4, 4]) == 1
    snake = S.thick_serpentine()
    assert snake.shape == (67, 131)
    for c, depth in ((4, 1824), (8, 1768)):
        out = S.split(snake, 4, connectivity=c)
        assert int(out["info"][1]) == 1 and out["depth"] == depth
        assert out["counts"].tolist() == [1, 1]


def test_the_wrong_tie_rule_is_told_apart():
    differs = 0
    for name, mask, r2 in _cases():
        if np.array_equal(S.split(mask, r2)["labels"], S.split(mask, r2, ties="high")["labels"]):
            continue
        differs += 1
    assert differs >= 1
    # ties are real: two seeds at equal distance from the pixels between them
    m = np.ones((3, 9), np.uint8)
    ids = np.full((3, 9), -1, np.int64)
    ids[:, 0], ids[:, 8] = 0, 8
    _, low = S.grow_dijkstra(m, ids, 4)
    _, high = S.grow_dijkstra(m, ids, 4, ties="high")
    assert low[1].tolist() == [0, 0, 0, 0, 0, 8, 8, 8, 8] and high[1].tolist() == [0, 0, 0, 0, 8, 8, 8, 8, 8]


def test_predict_scene_parser_takes_and_refuses_the_split_options(capsys):
    from change3d_amd.scripts.predict_scene import parse_args
    base = ["--weights", "w.pth"]
    args = parse_args(base + ["--objects", "--split_objects", "3"])
    assert args.split_objects == 3.0 and args.split_rounds is None and args.split == "test"
    assert parse_args(base + ["--objects"]).split_objects is None
    args = parse_args(base + ["--objects", "--split_objects", "1024", "--split_rounds", "65536", "--split", "val"])
    assert args.split_objects == 1024.0 and args.split_rounds == 65536 and args.split == "val"
    for bad in (["--split_objects", "3"], ["--objects", "--split_objects", "0"], ["--objects", "--split_objects", "0.5"],
                ["--objects", "--split_objects", "1025"], ["--objects", "--split_objects", "nan"], ["--objects", "--split_objects", "x"],
                ["--objects", "--split_rounds", "4"], ["--objects", "--split_objects", "2", "--split_rounds", "0"],
                ["--objects", "--split_objects", "2", "--split_rounds", "65537"]):
        with pytest.raises(SystemExit) as e:
            parse_args(base + bad)
        assert e.value.code == 2, bad
    capsys.readouterr()


def test_library_exports_and_header_declare_the_new_entries():
    names = L.check_exports()
    i32, i64, vp = C.c_int32, C.c_int64, C.c_void_p
    assert {"c3d_scene_split_ws_bytes", "c3d_scene_split_tile", "c3d_scene_split"} <= set(names)
    assert L.SIGNATURES["c3d_scene_split_ws_bytes"] == (i64, [i32, i32, i32])
    assert L.SIGNATURES["c3d_scene_split"] == (i32, [vp] * 3 + [i32] * 9 + [vp] * 8)
    assert (L.SPLIT_ST_NOT_CONVERGED, L.SPLIT_ST_BAD_LABELS) == (S.NOT_CONVERGED, S.BAD_LABELS) == (1, 2)
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "change3d_hip.h")).read()
    for text in ("int64_t c3d_scene_split_ws_bytes(", "int c3d_scene_split_tile(", "int c3d_scene_split(",
                 "#define C3D_SPLIT_ST_NOT_CONVERGED 1", "#define C3D_SPLIT_ST_BAD_LABELS 2"):
        assert text in header, text
    lib = L.lib()                                                                        # host-only entries, without a device
    assert lib.c3d_scene_split_ws_bytes(0, 5, 1) == -1 and lib.c3d_scene_split_ws_bytes(5, 5, 17) == -1
    assert lib.c3d_scene_split_ws_bytes(65536, 32768, 1) == -2
    assert lib.c3d_scene_split_ws_bytes(37, 53, 1) > lib.c3d_scene_label_ws_bytes(37, 53, 1) + 37 * 53 * 16
    assert lib.c3d_scene_split_ws_bytes(20000, 8, 1) > 0                                 # r2 = 0 runs past the transform's limit
    th, tw = ops.scene_split_tile()
    assert 8 <= th <= 256 and 8 <= tw <= 256 and lib.c3d_scene_split_tile(None) == -1
