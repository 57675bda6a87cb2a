"""`c3d_rings_conflicts` against its restatement (tests/conflicts_reference.py) through the C ABI, with canary rows round every
output.  Everything is an integer and equality is exact, value for value; the columns of `info` that describe the grid are
held against the header's grid rule as tests/conflicts_cases.py restates it.  The smallest shapes that reach each path: one
hand-made table per class between two ids, long diagonals over many cells, edges on cell borders, the corners of the coordinate
range at three frac_bits, crowded cells on both sides of the wave tier and of 1..4 chunks, two survey scenes of split pieces,
every flag, the work cap at and below `work`, accumulation in stream order, a dirty workspace and another stream, refusals, and
three negative controls."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conflicts_cases as K  # noqa: E402
import conflicts_reference as R  # noqa: E402

from change3d_amd import _lib as L  # noqa: E402
from change3d_amd import ops  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
PAD, CANARY = 3, -7777
E_BADARG = -1                                                # C3D_E_BADARG
ST_BAD_COUNTS = 2                                            # C3D_OUTLINE_ST_BAD_COUNTS
NAMES = ("conflict", "counts", "info")
HAND_MADE = K.hand_made()
LIMITS = functools.lru_cache(maxsize=None)(lambda: ops.rings_conflicts_limits())


def _ws(table, max_ids):
    n = L.lib().c3d_rings_conflicts_ws_bytes(table[0].shape[0], table[1].shape[0], max_ids)
    assert n > 0
    return torch.empty(n, dtype=torch.uint8, device=DEV)


def _call(table, frac_bits, max_ids, max_work=2 ** 32, totals=None, fill_ws=None):
    """The C entry on output buffers with canary rows on both sides: (rc, dict of numpy outputs)."""
    d = [torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(DEV) for a in table]
    conflict = torch.full((max_ids + 2 * PAD, 8), CANARY, dtype=torch.int64, device=DEV)
    counts = torch.full((8 + 2 * PAD,), CANARY, dtype=torch.int64, device=DEV)
    info = torch.full((8 + 2 * PAD,), CANARY, dtype=torch.int64, device=DEV)
    ws = _ws(table, max_ids)
    if fill_ws is not None:
        ws.fill_(fill_ws)
    rc = L.lib().c3d_rings_conflicts(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), table[0].shape[0], table[1].shape[0], frac_bits,
                                     max_ids, max_work, conflict[PAD:].data_ptr(), counts[PAD:].data_ptr(), info[PAD:].data_ptr(),
                                     None if totals is None else totals.data_ptr(), ws.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    bufs = [b.cpu().numpy() for b in (conflict, counts, info)]
    for buf in bufs:
        assert (buf[:PAD] == CANARY).all() and (buf[len(buf) - PAD:] == CANARY).all(), "a canary row was written"
    return rc, dict(zip(NAMES, (b[PAD:len(b) - PAD] for b in bufs)))


def _same(got, want, grid=None):
    assert np.array_equal(got["conflict"], want["conflict"]), (got["conflict"], want["conflict"])
    assert np.array_equal(got["counts"], want["counts"]), (got["counts"], want["counts"])
    for k in R.FIXED_INFO:
        assert got["info"][k] == want["info"][k], (k, got["info"], want["info"])
    if grid is not None:
        assert got["info"][1:6].tolist() == [grid[k] for k in ("shift", "cells_x", "cells_y", "entries", "work")], (got["info"], grid)


@functools.lru_cache(maxsize=None)
def _want(name):
    """The restatement and the grid of a named case, computed once."""
    c = HAND_MADE[name] if name in HAND_MADE else K.crowded(int(name))
    table = K.tables(c)
    return R.conflicts(table, c["frac_bits"], c["max_ids"], ring_limit=LIMITS()[3]), K.grid(table, c["frac_bits"], c["max_ids"], LIMITS())


def _check(c, table=None, over_work=False, max_work=2 ** 32, **kw):
    table = K.tables(c) if table is None else table
    want = R.conflicts(table, c["frac_bits"], c["max_ids"], over_work=over_work, ring_limit=LIMITS()[3])
    grid = K.grid(table, c["frac_bits"], c["max_ids"], LIMITS())
    rc, got = _call(table, c["frac_bits"], c["max_ids"], max_work=max_work, **kw)
    assert rc == 0
    _same(got, want, grid)
    return got


@pytest.mark.parametrize("name", list(HAND_MADE))
def test_hand_made_tables(name):
    c = HAND_MADE[name]
    want, grid = _want(name)
    rc, got = _call(K.tables(c), c["frac_bits"], c["max_ids"])
    assert rc == 0
    if name == "diagonals":
        assert got["info"][2] * got["info"][3] > 1, "the long edges' boxes must span many cells"
    _same(got, want, grid)
    for i, row in (c["want"] or {}).items():
        assert tuple(got["conflict"][i - 1, 3:]) == row
    if name == "bow_tie_alone":
        assert got["conflict"][0].tolist() == [0, 0, 4, 0, 0, 0, 0, 0] and got["counts"].tolist() == [1, 0, 0, 0, 0, 0, 0, 0]
    if name == "two_neighbours":
        assert got["conflict"][:3, 1].tolist() == [3, 3, 1]
    if name == "diagonals":
        assert got["counts"][5] == 4, "each pair of long edges once, however many cells hold both"
    if name == "borders":
        assert got["info"][1] <= 4, "every vertex lies on the border of a cell"
        assert got["counts"][:2].tolist() == [64, 0] and got["info"][6] == 2 * 7 * 8
    if name.startswith("frac"):
        assert got["conflict"][0, 0] == 0 and got["conflict"][0, 3] >= 1


@pytest.mark.parametrize("t", [21, 22, 85, 86, 171, 257])
def test_crowded_cells_on_both_sides_of_the_wave_tier_and_of_one_to_four_chunks(t):
    wave, chunk, tile = LIMITS()[:3]
    assert (wave, chunk, tile) == (64, 256, 256), "the sizes above aim at these edges"
    c = K.crowded(t)
    want, grid = _want(str(t))
    assert (grid["cells_x"], grid["cells_y"]) == (1, 1) and grid["cells"][(0, 0)] == 3 * t, "one cell holds every edge"
    rc, got = _call(K.tables(c), 0, c["max_ids"])
    assert rc == 0
    _same(got, want, grid)
    assert got["counts"][0] == t and got["counts"][5] > t and got["info"][5] == 3 * t * (3 * t - 1) // 2
    assert "conflicts_tail_kernel" in ops.last_kernel()


def test_two_survey_scenes_of_split_pieces():
    for seed, n_conflict in ((2, 10), (37, 11)):
        raw = K.scene_case(K.scene(seed, "split", 8))
        got = _check(raw)
        assert got["counts"][1] == 0 and got["counts"][5] == 0 and got["counts"][6] == 0 and got["info"][6] > 0, "raw pieces are clean"
        got = _check(K.scene_case(K.simplified_scene(seed, "split", 8, 1.0)))
        assert got["counts"][1] == n_conflict


def _flags_case():
    """id 1 checked and crossing id 2; id 2 only a 2-gon besides (still checked); id 3 incomplete (a start < 0 row patched in)
    although its square crosses id 1; id 4 all vertices equal (empty); id 5 no row; id 6 checked, far away."""
    rings = [K.sq(0, 0, 10), K.sq(5, 5, 10), [(40, 0), (50, 0)], K.sq(-5, -5, 10), [(7, 7), (7, 7), (7, 7)], K.sq(80, 0, 10), K.sq(100, 100, 4)]
    c = K.case(rings, ids=[1, 2, 2, 3, 4, 6, 3], max_ids=8)
    table = K.tables(c)
    table[0][6, 1] = -1
    return c, table


def test_every_flag_in_one_table():
    c, table = _flags_case()
    got = _check(c, table=table)
    assert got["conflict"][:, 0].tolist() == [0, 0, 2, 1, 1, 0, 0, 0]
    assert got["conflict"][0].tolist() == [0, 2, 4, 2, 0, 0, 0, 0], "the crossings with the incomplete id 3 are not counted"
    assert got["conflict"][2].tolist() == [2, 0, 0, 0, 0, 0, 0, 0]
    assert got["counts"].tolist() == [3, 2, 2, 1, 0, 2, 0, 0] and got["info"][0] == 12


def test_the_work_cap_at_and_below_work():
    for c in (HAND_MADE["cross"], K.crowded(22), HAND_MADE["diagonals"]):
        free = _check(c)
        work = int(free["info"][5])
        assert work > 0
        at = _check(c, max_work=work)
        assert all(np.array_equal(free[n], at[n]) for n in NAMES)
        below = _check(c, over_work=True, max_work=work - 1)
        rows = below["conflict"]
        checked = free["conflict"][:, 0] == 0
        assert (rows[checked & (free["conflict"][:, 2] > 0), 0] == 3).all() and not rows[:, [1, 3, 4, 5, 6, 7]].any()
        assert np.array_equal(rows[:, 2], free["conflict"][:, 2])
        assert below["counts"].tolist() == [0, 0, int(free["counts"][2]), 0, int(free["counts"][0]), 0, 0, 0]
        assert below["info"][5] == work and below["info"][6] == 0 and below["info"][7] == 0
    c, table = _flags_case()
    got = _check(c, table=table, over_work=True, max_work=0)
    assert got["conflict"][:, 0].tolist() == [3, 3, 2, 1, 1, 3, 0, 0] and got["counts"][:5].tolist() == [0, 0, 2, 1, 3]


def test_bad_rows_bad_counts_and_rows_cut():
    c = HAND_MADE["two_neighbours"]
    for change in ("start", "negative_n", "past_the_end", "coordinate", "bad_counts", "status_carried", "rows_cut"):
        table = K.tables(c)
        if change == "start":
            table[0][2, 1] = -1
        elif change == "negative_n":
            table[0][2, 2] = -4
        elif change == "past_the_end":
            table[0][2, 2] = int(table[2][3]) - int(table[0][2, 1]) + 1
        elif change == "coordinate":
            table[1][1, 0] = 32769
        elif change == "bad_counts":
            table[2][4] = ST_BAD_COUNTS | 1
        elif change == "status_carried":
            table[2][4] = 5
        elif change == "rows_cut":
            table[2][1] = 2                                  # K becomes 2: the rows of ids 3 .. are zeroed by the call
        got = _check(c, table=table)
        expect = {"start": [0, 0, 2], "negative_n": [0, 0, 2], "past_the_end": [0, 0, 2], "coordinate": [2, 0, 0], "bad_counts": [0, 0, 0],
                  "status_carried": [0, 0, 0], "rows_cut": [0, 0, 0]}[change]
        assert got["conflict"][:3, 0].tolist() == expect, change
        assert got["counts"][7] == {"bad_counts": ST_BAD_COUNTS | 1, "status_carried": 5}.get(change, 0), change
        if change in ("start", "negative_n", "past_the_end", "rows_cut"):
            assert got["counts"][5] == 0, "without the bar nothing crosses"
        if change == "bad_counts":
            assert not got["conflict"].any() and got["info"][0] == 0


def test_two_calls_accumulate_in_stream_order():
    totals = torch.zeros(8, dtype=torch.int64, device=DEV)
    runs = []
    for name, status in (("two_neighbours", 0), ("same", 4), ("opposite", 1)):
        c = HAND_MADE[name]
        table = K.tables(c)
        table[2][4] = status                                 # the status is OR-ed in
        rc, got = _call(table, 0, c["max_ids"], totals=totals)
        assert rc == 0
        runs.append(got)
    t = totals.cpu().numpy()
    assert np.array_equal(t[:7], sum(r["counts"][:7] for r in runs)) and t[7] == 5
    assert t[:7].tolist() == [7, 5, 0, 0, 0, 4, 1]


def test_dirty_workspace_other_stream_and_repeatability():
    rings = [t for t in K.crowded(22)["rings"]] + HAND_MADE["diagonals"]["rings"][:12]
    c = K.case(rings, ids=list(range(1, len(rings) + 1)))
    table = K.tables(c)
    want = R.conflicts(table, 0, c["max_ids"])
    runs = []
    for fill in (0x00, 0xA5, None, 0xFF):
        rc, got = _call(table, 0, c["max_ids"], fill_ws=fill)
        assert rc == 0
        _same(got, want, K.grid(table, 0, c["max_ids"], LIMITS()))
        runs.append(got)
    assert all(np.array_equal(runs[0][n], r[n]) for r in runs[1:] for n in NAMES)
    d = [torch.from_numpy(a).to(DEV) for a in table]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    before = ops.launch_count()
    with torch.cuda.stream(side):
        out = ops.rings_conflicts(*d, 0, c["max_ids"])
        again = ops.rings_conflicts(*d, 0, c["max_ids"])
    side.synchronize()
    assert ops.launch_count() - before == 28, "the header documents 14 launches"
    assert all(torch.equal(a, b) for a, b in zip(out, again))
    assert all(np.array_equal(runs[0][n], t.cpu().numpy()) for n, t in zip(NAMES, out))


def test_refusals_enqueue_nothing():
    c = HAND_MADE["cross"]
    table = K.tables(c)
    d = [torch.from_numpy(a).to(DEV) for a in table]
    out = [torch.zeros((c["max_ids"], 8), dtype=torch.int64, device=DEV), torch.zeros(8, dtype=torch.int64, device=DEV),
           torch.zeros(8, dtype=torch.int64, device=DEV)]
    ws = _ws(table, c["max_ids"])
    ptrs = [d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), table[0].shape[0], table[1].shape[0], 0, c["max_ids"], 2 ** 32,
            out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), None, ws.data_ptr(), 0]
    before = ops.launch_count()
    fn = L.lib().c3d_rings_conflicts
    for slot in (0, 1, 2, 8, 9, 10, 12):
        args = list(ptrs)
        args[slot] = None
        assert fn(*args) == E_BADARG, slot
    for slot in (3, 4, 6):
        for value in (0, -1):
            args = list(ptrs)
            args[slot] = value
            assert fn(*args) == E_BADARG, slot
    for value in (-1, 9):
        args = list(ptrs)
        args[5] = value
        assert fn(*args) == E_BADARG
    args = list(ptrs)
    args[7] = -1
    assert fn(*args) == E_BADARG
    ws_bytes = L.lib().c3d_rings_conflicts_ws_bytes
    for slot in range(3):
        sizes = [1] * 3
        sizes[slot] = 0
        assert ws_bytes(*sizes) == E_BADARG
    assert ws_bytes(1, 1, 1) > 0
    assert ops.launch_count() == before
    torch.cuda.synchronize()
    assert not any(t.any() for t in out)
    with pytest.raises(ValueError):
        ops.rings_conflicts(*d, 9)
    with pytest.raises(ValueError):
        ops.rings_conflicts(*d, 0, max_work=-1)
    with pytest.raises(L.Change3DHipError):
        ops.rings_conflicts(d[0].cpu(), *d[1:], 0)
    with pytest.raises(L.Change3DHipError):
        ops.rings_conflicts(*d, 0, max_objects=0)
    assert ops.launch_count() == before


@pytest.mark.parametrize("name,wrong", [("bow_tie_alone", dict(same_id=True)), ("opposite", dict(direction=False)),
                                        ("touch_vv", dict(strict=False))])
def test_negative_controls_differ_from_the_device(name, wrong):
    c = HAND_MADE[name]
    table = K.tables(c)
    rc, got = _call(table, 0, c["max_ids"])
    bad = R.conflicts(table, 0, c["max_ids"], **wrong)
    assert rc == 0 and not np.array_equal(got["conflict"], bad["conflict"]), (name, wrong)
    assert got["counts"][1] == 0 and bad["counts"][1] > 0
    _same(got, R.conflicts(table, 0, c["max_ids"]))
