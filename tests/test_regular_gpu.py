"""`c3d_rings_regularize` against its restatement (tests/regular_reference.py): ring rows, vertices and counts exactly equal.
Hand-made tables, ids without a direction, pass-through and bad rows with canaries, rings on both sides of every tier limit
in one table, thousands of small rings, the corners of the coordinate range with a long direction, every frac_bits, two
negative controls, determinism on a dirty workspace and a non-default stream, refusals, and one round trip on the device."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fill_cases as FK  # noqa: E402
import regular_cases as K  # noqa: E402
import regular_reference as R  # noqa: E402
import simplify_cases as SK  # noqa: E402
from simplify_reference import table as make_table  # noqa: E402

from change3d_amd import _lib as L  # noqa: E402
from change3d_amd import ops  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
PAD, CANARY = 3, -7777
E_BADARG = -1                                                # C3D_E_BADARG
NAMES = ("rings", "vertices", "counts")


def _call(table, hull, frac_bits, ws=None, fill_ws=None):
    """The C entry on output buffers with canary rows on both sides: (rc, dict of numpy outputs)."""
    rings, vertices, counts = table
    max_rings, max_vertices, max_objects, max_hv = rings.shape[0], vertices.shape[0], hull[0].shape[0], hull[1].shape[0]
    d_in = [torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(DEV) for a in (rings, vertices, counts, hull[0], hull[1], hull[3])]
    d_rects = torch.from_numpy(np.ascontiguousarray(hull[2], dtype=np.int64)).to(DEV)
    r_out = torch.full((max_rings + 2 * PAD, 8), CANARY, dtype=torch.int32, device=DEV)
    v_out = torch.full((max_vertices + 2 * PAD, 2), CANARY, dtype=torch.int32, device=DEV)
    c_out = torch.full((5 + 2 * PAD,), CANARY, dtype=torch.int32, device=DEV)
    if ws is None:
        ws = torch.empty(L.lib().c3d_rings_regularize_ws_bytes(max_rings, max_vertices, max_objects), dtype=torch.uint8, device=DEV)
    if fill_ws is not None:
        ws.fill_(fill_ws)
    rc = L.lib().c3d_rings_regularize(d_in[0].data_ptr(), d_in[1].data_ptr(), d_in[2].data_ptr(), max_rings, max_vertices,
                                      d_in[3].data_ptr(), d_in[4].data_ptr(), d_rects.data_ptr(), d_in[5].data_ptr(), max_objects,
                                      max_hv, frac_bits, r_out[PAD:].data_ptr(), v_out[PAD:].data_ptr(), c_out[PAD:].data_ptr(),
                                      ws.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    bufs = [b.cpu().numpy() for b in (r_out, v_out, c_out)]
    for buf in bufs:
        assert (buf[:PAD] == CANARY).all() and (buf[len(buf) - PAD:] == CANARY).all(), "a canary row was written"
    return rc, dict(zip(NAMES, (b[PAD:len(b) - PAD] for b in bufs)))


def _same(got, want):
    assert np.array_equal(got["counts"], want["counts"]), (got["counts"], want["counts"])
    diff = np.argwhere((got["rings"] != want["rings"]).any(axis=1))[:3].ravel()
    assert np.array_equal(got["rings"], want["rings"]), (diff, got["rings"][diff], want["rings"][diff])
    written = int(got["counts"][3])
    diff = np.argwhere((got["vertices"][:written] != want["vertices"][:written]).any(axis=1))[:3].ravel()
    assert diff.size == 0, (diff, got["vertices"][diff], want["vertices"][diff])
    assert (got["vertices"][written:] == CANARY).all(), "a vertex row past counts_out[3] was written"


def _check(table, hull, frac_bits=4, **kw):
    """Device against restatement: exact.  Returns (restatement, device outputs)."""
    want = R.regularize(*table, *hull, frac_bits)
    rc, got = _call(table, hull, frac_bits, **kw)
    assert rc == 0
    _same(got, want)
    return want, got


def _tables(case, max_objects=None, spare_rings=2, spare_vertices=3):
    lists, ids, dirs = case
    table = make_table(lists, max_rings=len(lists) + spare_rings, max_vertices=sum(len(v) for v in lists) + spare_vertices, ids=ids)
    return table, K.hull_tables(dirs, (max(ids) + 2) if max_objects is None else max_objects)


HAND_MADE = K.hand_made()
LIMITS = functools.lru_cache(maxsize=None)(lambda: ops.rings_regularize_limits())
FLAGS = {"n3": [0], "n4_junction_at_0": [1], "R0": [0], "R2": [0], "zero_edge": [0], "run_wraps_0": [1], "tie45": [1], "gcd": [1],
         "negative_u": [1, 1], "holes": [1, 1, 1], "not_contiguous": [1, 1, 1, 1], "no_direction": [0, 0, 1, 0, 0],
         "empty_ring": [0, 1, 0]}


@pytest.mark.parametrize("name", list(HAND_MADE))
def test_hand_made_tables(name):
    table, hull = _tables(HAND_MADE[name])
    want, got = _check(table, hull)
    rows = len(HAND_MADE[name][0])
    assert got["counts"][4] == 0 and got["counts"][1] == rows and not got["rings"][rows:].any()
    assert got["rings"][:rows, 3].tolist() == FLAGS[name]
    if name == "n4_junction_at_0":
        assert got["vertices"][:4].tolist() == [[16 * x, 16 * y] for x, y in HAND_MADE[name][0][0]]
    if name == "n3":
        assert got["rings"][0, 1:3].tolist() == [0, 3] and got["vertices"][:3].tolist() == [[16, 16], [144, 16], [144, 80]]
    if name == "run_wraps_0":
        assert got["rings"][0, 2] == 4 and got["rings"][0, 7] == 5


@pytest.mark.parametrize("frac_bits", [0, 4, 8])
def test_every_frac_bits_on_one_table(frac_bits):
    lists, ids, dirs = [], [], {}
    for name in ("gcd", "negative_u", "holes", "tie45", "run_wraps_0", "no_direction"):
        rl, ri, rd = HAND_MADE[name]
        base = max(ids, default=0)
        lists += rl
        ids += [base + i for i in ri]
        dirs.update({base + i: d for i, d in rd.items()})
    want, got = _check(*_tables((lists, ids, dirs)), frac_bits=frac_bits)
    assert got["counts"][4] == 0 and got["rings"][:, 3].sum() >= 8


@pytest.mark.parametrize("which", [0, 1])
def test_rings_on_both_sides_of_a_tier_limit(which):
    T = LIMITS()[which]
    assert 4 <= LIMITS()[0] < LIMITS()[1] <= 1 << 16
    small = [K.WOBBLY, [(1, 1), (9, 1), (9, 5), (1, 5)], [(1, 1), (9, 1), (9, 5)]]
    lists, ids = [], []
    for k, n in enumerate((T - 1, T, T + 1)):                # small rings between the long ones: the tiers alternate
        lists += [K.stair_ring(n, seed=10 * which + k), small[k]]
        ids += [1 + k % 2, 3]
    lists.append([(p[0], p[1]) for p in K.stair_ring(T + 1, seed=3)])   # a long ring of an id without a direction: copied
    ids.append(4)
    want, got = _check(*_tables((lists, ids, {1: (1, 0), 2: (5, -2), 3: (3, 1), 4: None})))
    assert got["counts"][4] == 0 and got["rings"][:7, 3].tolist() == [1, 1, 1, 1, 1, 0, 0]
    assert got["rings"][[0, 2, 4], 7].tolist() == [T - 1, T, T + 1] and (got["rings"][[0, 2, 4], 2] > T // 2).all()
    assert got["rings"][6, 2] == T + 1


def test_thousands_of_small_rings_exercise_the_scan():
    lists, ids, dirs = K.many_small(9000, seed=7)            # more rows than one step of the scan takes
    want, got = _check(*_tables((lists, ids, dirs), max_objects=45))
    flags = got["rings"][:9000, 3]
    assert got["counts"][4] == 0 and 3000 < flags.sum() < 9000 and got["counts"][1] == 9000
    starts = got["rings"][:9000, 1].astype(np.int64)
    assert np.array_equal(starts[1:], np.cumsum(got["rings"][:8999, 2]))


def test_the_corners_of_the_coordinate_range_with_a_long_direction():
    """S * A + W leaves 64 bits here (tests/test_regular_cpu.py shows it on the same case): no 64-bit shortcut can be taken."""
    want, got = _check(*_tables(K.FULL_RANGE), frac_bits=8)
    assert got["rings"][:2, 3].tolist() == [1, 1] and got["counts"][4] == 0
    assert np.abs(got["vertices"][:int(got["counts"][3])]).max() <= 2 * 16384 * 256


def test_negative_controls_see_the_tie_rule_and_the_floor_division():
    for name, wrong in (("tie45", dict(tie="strict")), ("negative_u", dict(division="truncate"))):
        table, hull = _tables(HAND_MADE[name])
        rc, got = _call(table, hull, 4)
        bad = R.regularize(*table, *hull, 4, **wrong)
        n = int(got["counts"][3])
        assert rc == 0 and n == bad["counts"][3] and not np.array_equal(got["vertices"][:n], bad["vertices"][:n]), (name, wrong)


def _mixed():
    lists, ids, dirs = [], [], {}
    for name in ("holes", "gcd", "not_contiguous", "negative_u"):
        rl, ri, rd = HAND_MADE[name]
        base = max(ids, default=0)
        lists += rl
        ids += [base + i for i in ri]
        dirs.update({base + i: d for i, d in rd.items()})
    lists.append(K.stair_ring(100, seed=1))
    ids.append(max(ids) + 1)
    dirs[ids[-1]] = (2, 5)
    return _tables((lists, ids, dirs)), max(ids)


def test_pass_through_bad_rows_and_bad_counts():
    ((rings, vertices, counts), hull), top = _mixed()
    rings[1, 1] = -1                                         # a ring the outlines call had no room for: silently passed through
    counts[4] = R.ST_TRUNCATED
    hull[3][4] = 128                                         # the hull call's status is carried too
    want, got = _check((rings, vertices, counts), hull)
    assert got["counts"][4] == R.ST_TRUNCATED | 128 and got["rings"][1, 1:4].tolist() == [-1, 0, 0]
    for change in ("n_past_the_end", "negative_n", "coordinate", "negative_coordinate", "big_coordinate_in_a_big_ring", "id_zero",
                   "id_past_the_table", "rows_past_the_table", "negative_counts", "shared_vertices_outgrow_the_list"):
        ((rings, vertices, counts), hull), top = _mixed()
        row, flagged = 2, True
        if change == "n_past_the_end":
            rings[row, 2] = int(counts[3]) - int(rings[row, 1]) + 1
        elif change == "negative_n":
            rings[row, 2] = -3
        elif change == "coordinate":
            vertices[int(rings[row, 1]) + 1, 0] = 16385
        elif change == "negative_coordinate":
            vertices[int(rings[row, 1]), 1] = -1
        elif change == "big_coordinate_in_a_big_ring":
            row = rings.shape[0] - 3                         # the staircase of 100 vertices
            vertices[int(rings[row, 1]) + 77, 1] = 1 << 20
        elif change == "id_zero":
            rings[row, 0] = 0
        elif change == "id_past_the_table":
            rings[row, 0] = top + 3
        elif change == "rows_past_the_table":
            counts[1], flagged = rings.shape[0] + 100, False  # clamped: the spare rows are zero rows, id 0, n 0
            rings[-1] = (1, -1, 5, 0, 0, 0, 0, 0)
            rings[-2] = (1, -1, 5, 0, 0, 0, 0, 0)
        elif change == "negative_counts":
            counts[1], flagged = -5, False
        elif change == "shared_vertices_outgrow_the_list":
            rings[-1] = rings[-3]                            # the staircase twice more: copied or not, it no longer fits
            rings[-2] = rings[-3]
            rings[-1, 0] = top + 1                           # an id without a direction
            counts[0] = counts[1] = rings.shape[0]
        want, got = _check((rings, vertices, counts), hull)
        assert bool(got["counts"][4] & R.ST_BAD_ROW) == flagged, change
        if flagged and change != "shared_vertices_outgrow_the_list":
            assert got["rings"][row, 1:4].tolist() == [-1, 0, 0]
    for where in (0, 1):
        ((rings, vertices, counts), hull), top = _mixed()
        (counts if where == 0 else hull[3])[4] = R.ST_BAD_COUNTS | R.ST_TRUNCATED
        want, got = _check((rings, vertices, counts), hull)
        assert got["counts"].tolist() == [0, 0, 0, 0, R.ST_BAD_COUNTS | R.ST_TRUNCATED] and not got["rings"].any()


def test_refusals_enqueue_nothing():
    ((rings, vertices, counts), hull), top = _mixed()
    d = [torch.from_numpy(a).to(DEV) for a in (rings, vertices, counts) + tuple(hull)]
    out = [torch.zeros_like(d[0]), torch.zeros_like(d[1]), torch.zeros(5, dtype=torch.int32, device=DEV)]
    sizes = (rings.shape[0], vertices.shape[0], hull[0].shape[0], hull[1].shape[0])
    ws = torch.zeros(L.lib().c3d_rings_regularize_ws_bytes(sizes[0], sizes[1], sizes[2]), dtype=torch.uint8, device=DEV)
    ptrs = [d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), sizes[0], sizes[1], d[3].data_ptr(), d[4].data_ptr(), d[5].data_ptr(),
            d[6].data_ptr(), sizes[2], sizes[3], 4] + [t.data_ptr() for t in out] + [ws.data_ptr(), 0]
    before = ops.launch_count()
    for slot in (0, 1, 2, 5, 6, 7, 8, 12, 13, 14, 15):
        args = list(ptrs)
        args[slot] = None
        assert L.lib().c3d_rings_regularize(*args) == E_BADARG
    for slot in (3, 4, 9, 10):
        for value in (0, -1):
            args = list(ptrs)
            args[slot] = value
            assert L.lib().c3d_rings_regularize(*args) == E_BADARG
    for value in (-1, 9):
        args = list(ptrs)
        args[11] = value
        assert L.lib().c3d_rings_regularize(*args) == E_BADARG
    ws_bytes = L.lib().c3d_rings_regularize_ws_bytes
    assert ws_bytes(0, 1, 1) == E_BADARG and ws_bytes(1, 0, 1) == E_BADARG and ws_bytes(1, 1, 0) == E_BADARG and ws_bytes(1, 1, 1) > 0
    assert ops.launch_count() == before
    torch.cuda.synchronize()
    assert not any(t.any() for t in out)
    with pytest.raises(ValueError):
        ops.rings_regularize(*d, frac_bits=9)
    with pytest.raises(L.Change3DHipError):
        ops.rings_regularize(d[0].cpu(), *d[1:])
    with pytest.raises(L.Change3DHipError):
        ops.rings_regularize(*d[:6], d[6].cpu())
    assert ops.launch_count() == before


def test_dirty_workspace_other_stream_and_repeatability():
    wave, lds = LIMITS()
    lists = [K.stair_ring(lds + 200, 1), K.stair_ring(700, 2), K.WOBBLY, K.stair_ring(wave + 9, 4)]
    table, hull = _tables((lists, [1, 2, 2, 3], {1: (3, 1), 2: (1, 0), 3: (-5, 2)}))
    want = R.regularize(*table, *hull, 4)
    runs = []
    for fill in (0x00, 0xFF, None):
        rc, got = _call(table, hull, 4, fill_ws=fill)
        assert rc == 0
        _same(got, want)
        runs.append(got)
    for other in runs[1:]:
        assert all(np.array_equal(runs[0][n], other[n]) for n in NAMES)
    assert "regular_write_block_kernel" in ops.last_kernel()
    d = [torch.from_numpy(a).to(DEV) for a in table + tuple(hull)]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    before = ops.launch_count()
    with torch.cuda.stream(side):
        out = ops.rings_regularize(*d, frac_bits=4)
    side.synchronize()
    assert ops.launch_count() - before == 5, "the header documents 5 launches"
    got = dict(zip(NAMES, (t.cpu().numpy() for t in out)))
    written = int(got["counts"][3])
    assert np.array_equal(got["rings"], want["rings"]) and np.array_equal(got["counts"], want["counts"])
    assert np.array_equal(got["vertices"][:written], want["vertices"][:written])


@pytest.mark.parametrize("split", [False, True])
def test_round_trip_on_the_device(split):
    """Traced (or split) masks, 256 x 256: simplify, hull, regularise, fill at 1/16 px.  Device against restatement on the
    device's own inputs, and the fill accepts every ring."""
    Hs = Ws = 256
    mask = np.zeros((Hs, Ws), np.uint8)
    if split:
        mask[20:95, 30:140] = FK.touching_mask(75, 110)
    else:
        mask[:136, :200] = SK.blobs(136, 200, 30, 9, seed=2)
        for k, d in enumerate(((3, 1), (1, 1))):
            mask[150:246, 10 + 120 * k:106 + 120 * k] = K.rotated_rectangle(d)
    N = Hs * Ws
    m = torch.from_numpy(mask).to(DEV)
    if split:
        labels, table, _, _, counts, info = ops.scene_split(m, 3.0, connectivity=8, max_objects=4096)
    else:
        labels, table, _, _, counts = ops.scene_objects(m, connectivity=8, max_objects=4096)
    rings, vertices, rc = ops.scene_outlines(labels, counts, connectivity=8, max_objects=4096, max_rings=8192, max_vertices=N)
    s_rings, s_vertices, sc = ops.outlines_simplify(rings, vertices, rc, 1.0)
    hull = ops.rings_hull(rings, vertices, rc, max_objects=4096)
    r_rings, r_vertices, qc = ops.rings_regularize(s_rings, s_vertices, sc, *hull, frac_bits=4)
    filled, _, _, _, _, info = ops.rings_fill(r_rings, r_vertices, qc, Hs, Ws, frac_bits=4, max_objects=4096)
    torch.cuda.synchronize()
    assert int(rc[4]) == 0 and int(sc[4]) == 0 and int(hull[3][4]) == 0 and int(qc[4]) == 0 and int(info[0]) == 0
    want = R.regularize(*(t.cpu().numpy() for t in (s_rings, s_vertices, sc) + tuple(hull)), 4)
    got = dict(zip(NAMES, (t.cpu().numpy() for t in (r_rings, r_vertices, qc))))
    written = int(got["counts"][3])
    assert np.array_equal(got["counts"], want["counts"]) and np.array_equal(got["rings"], want["rings"])
    assert np.array_equal(got["vertices"][:written], want["vertices"][:written])
    assert int(info[1]) == int(qc[1]) and bool((filled > 0).any())
    if not split:
        assert got["rings"][:, 3].sum() >= 2, "the two rotated rectangles at least are regularised"
