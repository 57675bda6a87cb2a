"""`c3d_rings_valid` against its restatement (tests/valid_reference.py) through the C ABI, with canary rows round every output.
Everything is an integer and equality is exact, value for value.  The smallest shapes that reach each path: the hand-made
table of every pair class, two rows of the survey of noisy masks, stars on both sides of the wave tier, stars whose chunk
counts 1..5 cover the even and the odd job schedule, the c/2 offset, a partial last chunk and the LDS tile edge, one id of
interleaved rings, rings on both sides of the length that many workgroups share (checked and copied, and one whose pairs are
evaluated), an id on each side of the ring limit, the corners of the coordinate range at three frac_bits, every flag, the work cap at and below m (m - 1) / 2,
accumulation in stream order, a dirty workspace and another stream, refusals, and three negative controls."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import valid_cases as K  # noqa: E402
import valid_reference as V  # noqa: E402

from change3d_amd import _lib as L  # noqa: E402
from change3d_amd import ops  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
PAD, CANARY = 3, -7777
E_BADARG = -1                                                # C3D_E_BADARG
ST_BAD_COUNTS = 2                                            # C3D_OUTLINE_ST_BAD_COUNTS
NAMES = ("valid", "counts")
HAND_MADE = K.hand_made()
LIMITS = functools.lru_cache(maxsize=None)(lambda: ops.rings_valid_limits())


def _ws(table, max_ids):
    n = L.lib().c3d_rings_valid_ws_bytes(table[0].shape[0], table[1].shape[0], max_ids)
    assert n > 0
    return torch.empty(n, dtype=torch.uint8, device=DEV)


def _call(table, frac_bits, max_ids, max_id_work=2 ** 32, totals=None, fill_ws=None):
    """The C entry on output buffers with canary rows on both sides: (rc, dict of numpy outputs)."""
    d = [torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(DEV) for a in table]
    valid = torch.full((max_ids + 2 * PAD, 8), CANARY, dtype=torch.int64, device=DEV)
    counts = torch.full((8 + 2 * PAD,), CANARY, dtype=torch.int64, device=DEV)
    ws = _ws(table, max_ids)
    if fill_ws is not None:
        ws.fill_(fill_ws)
    rc = L.lib().c3d_rings_valid(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), table[0].shape[0], table[1].shape[0], frac_bits,
                                 max_ids, max_id_work, valid[PAD:].data_ptr(), counts[PAD:].data_ptr(),
                                 None if totals is None else totals.data_ptr(), ws.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    bufs = [b.cpu().numpy() for b in (valid, counts)]
    for buf in bufs:
        assert (buf[:PAD] == CANARY).all() and (buf[len(buf) - PAD:] == CANARY).all(), "a canary row was written"
    return rc, dict(zip(NAMES, (b[PAD:len(b) - PAD] for b in bufs)))


def _same(got, want):
    for name in NAMES:
        assert np.array_equal(got[name], want[name]), (name, got[name], want[name])


def _check(c, table=None, **kw):
    table = K.tables(c) if table is None else table
    want = V.valid(table, c["frac_bits"], c["max_ids"], ring_limit=LIMITS()[3], **kw)
    rc, got = _call(table, c["frac_bits"], c["max_ids"], **kw)
    assert rc == 0
    _same(got, want)
    return got


@functools.lru_cache(maxsize=None)
def _star_case(n):
    """{n/k} at frac_bits 8 on a radius of 30000 px, where the rounding to the lattice is far below the distance of a vertex
    from the chord that passes it, also at n = 1025: exactly n (k - 1) crossings (tests/test_valid_cpu.py)."""
    k = 2 if n % 2 else 3
    return K.case([K.star(n, k, radius=30000 * 256)], frac_bits=8), n * (k - 1)


@pytest.mark.parametrize("name", list(HAND_MADE))
def test_hand_made_tables(name):
    c = HAND_MADE[name]
    got = _check(c)
    if c["want"] is not None:
        assert tuple(got["valid"][0, 4:]) == c["want"]
    if name.startswith("frac"):
        assert got["valid"][0, 0] == 0 and got["valid"][0, 4] >= 1
    if name == "interleaved":
        assert got["counts"].tolist() == [3, 2, 0, 0, 0, 3, 0, 0]


def test_two_rows_of_the_survey():
    for seed, connectivity, i, tol, want in ((4, 4, 30, 1.0, (0, 1)), (27, 8, 2, 2.0, (2, 0))):
        got = _check(K.case(K.simplified(K.traced(seed, connectivity)[i], tol)))
        assert tuple(got["valid"][0, 4:6]) == want and got["counts"][1] == 1
        got = _check(K.case(K.traced(seed, connectivity)[i]))
        assert got["counts"][:2].tolist() == [1, 0], "raw rings are valid"


@pytest.mark.parametrize("n", [5, 63, 64, 65])
def test_stars_on_both_sides_of_the_wave_tier(n):
    assert LIMITS()[0] == 64
    c, crossings = _star_case(n)
    got = _check(c)
    assert got["valid"][0].tolist() == [0, 1, n, 0, crossings, 0, 0, 0]


@pytest.mark.parametrize("n", [255, 256, 257, 511, 513, 769, 1025])
def test_stars_of_one_to_five_chunks(n):
    wave, chunk, tile = LIMITS()[:3]
    assert chunk == 256 and tile == 256, "the sizes above aim at these edges"
    c, crossings = _star_case(n)
    got = _check(c)
    assert got["valid"][0].tolist() == [0, 1, n, 0, crossings, 0, 0, 0]
    assert "valid_tail_kernel" in ops.last_kernel()


def test_one_ring_that_many_workgroups_share_with_its_pairs_evaluated():
    """The pure-Python restatement needs minutes for this n, so the count asserted is the constructed n (k - 1); it was
    confirmed once on the CPU with valid_reference.count_pairs at this n, radius and frac_bits."""
    n = LIMITS()[4] + 1
    c, crossings = _star_case(n)
    rc, got = _call(K.tables(c), c["frac_bits"], c["max_ids"])
    assert rc == 0
    assert got["valid"][0].tolist() == [0, 1, n, 0, crossings, 0, 0, 0]


def test_rings_on_both_sides_of_the_length_that_many_workgroups_share():
    big = LIMITS()[4]
    rings = [K.P.polygon(big, 1, radius=20000), K.P.square(30000, 30000, 50), K.P.polygon(big + 1, 2, radius=25000),
             K.P.polygon(2 * big + 77, 3, radius=30000)]
    rings[3][5000] = rings[3][4999]                          # one degenerate edge deep inside a ring that many workgroups copy
    c = K.case(rings, ids=[1, 2, 3, 1], max_ids=4)           # id 1: a ring of the limit, then one of twice that, not contiguous
    table = K.tables(c)
    # the long ids come out over the work cap: their rows still carry rings, m and the degenerate count of the gather
    got = _check(c, table=table, max_id_work=6)
    assert got["valid"].tolist() == [[3, 2, 12364, 1, 0, 0, 0, 0], [0, 1, 4, 0, 0, 0, 0, 0], [3, 1, 4097, 0, 0, 0, 0, 0], [0] * 8]
    assert got["counts"].tolist() == [1, 0, 0, 0, 2, 0, 0, 0]
    table[1][int(table[0][3, 1]) + 2 * big + 50, 1] = -32769   # one coordinate out of range deep inside the longest ring
    got = _check(c, table=table, max_id_work=6)
    assert got["valid"][0].tolist() == [2, 0, 0, 0, 0, 0, 0, 0]
    assert got["counts"].tolist() == [1, 0, 0, 1, 1, 0, 0, 0]


def test_an_id_on_each_side_of_the_ring_limit():
    limit = LIMITS()[3]
    rings, ids = [], []
    for k in range(2 * limit + 1):                           # id 1 gets `limit` rings, id 2 one more, interleaved
        rings.append(K.P.square(12 * ((k // 2) % 256), 60 * ((k // 2) // 256) + 30 * (k % 2), 5))
        ids.append(2 if k == 2 * limit else 1 + k % 2)
    got = _check(K.case(rings, ids=ids, max_ids=3), max_id_work=6)
    assert got["valid"].tolist() == [[3, 16384, 65536, 0, 0, 0, 0, 0], [2, 0, 0, 0, 0, 0, 0, 0], [0] * 8]
    assert got["counts"].tolist() == [0, 0, 0, 1, 1, 0, 0, 0]


def test_both_tiers_and_every_flag_in_one_table():
    chunk = LIMITS()[1]
    rings = [K.star(2 * chunk + 3, 2, radius=9000, centre=(-20000, -20000)), K.P.square(0, 0, 10), K.star(9, 4, radius=3000, centre=(20000, 0)),
             [(5, 5), (6, 6)], K.P.square(100, 100, 10), K.star(chunk + 1, 2, radius=8000, centre=(0, 20000)), K.P.square(5, 5, 10)]
    c = K.case(rings, ids=[1, 2, 3, 4, 5, 6, 2], max_ids=9)
    table = K.tables(c)
    table[0][4, 1] = -1                                      # id 5: a row with start < 0
    got = _check(c, table=table, max_id_work=(2 * chunk + 3) * (2 * chunk + 2) // 2 - 1)
    assert got["valid"][:, 0].tolist() == [3, 0, 0, 1, 2, 0, 0, 0, 0]
    assert got["valid"][1, 4:].tolist() == [2, 0, 0, 0] and got["counts"][:5].tolist() == [3, 3, 1, 1, 1]


def test_the_work_cap_at_and_below_the_pairs_of_an_id():
    for c, m in ((HAND_MADE["bow_tie"], 4), (_star_case(65)[0], 65)):
        got = _check(c, max_id_work=m * (m - 1) // 2)
        assert got["valid"][0, 0] == 0 and got["valid"][0, 4] > 0
        got = _check(c, max_id_work=m * (m - 1) // 2 - 1)
        assert got["valid"][0].tolist() == [3, 1, m, 0, 0, 0, 0, 0] and got["counts"].tolist() == [0, 0, 0, 0, 1, 0, 0, 0]
    got = _check(HAND_MADE["triangle"], max_id_work=2)
    assert got["valid"][0, 0] == 3
    got = _check(K.case([[(1, 1), (1, 1), (1, 2)]]), max_id_work=0)   # m = 2: one pair
    assert got["valid"][0].tolist() == [3, 1, 2, 1, 0, 0, 0, 0]


def test_start_below_zero_bad_rows_ids_past_the_last_and_bad_counts():
    c = HAND_MADE["flags"]
    for change in ("start", "negative_n", "past_the_end", "coordinate", "bad_counts", "status_carried", "rows_cut"):
        table = K.tables(c)
        if change == "start":
            table[0][2, 1] = -1
        elif change == "negative_n":
            table[0][2, 2] = -4
        elif change == "past_the_end":
            table[0][4, 2] = int(table[2][3]) - int(table[0][4, 1]) + 1
        elif change == "coordinate":
            table[1][1, 0] = 32769
        elif change == "bad_counts":
            table[2][4] = ST_BAD_COUNTS | 1
        elif change == "status_carried":
            table[2][4] = 5
        elif change == "rows_cut":
            table[2][1] = 3                                  # K becomes 3: the rows of ids 4 .. 8 are zeroed by the call
        got = _check(c, table=table)
        expect = {"start": [0, 1, 2, 1, 1, 0, 0, 0], "negative_n": [0, 1, 2, 1, 1, 0, 0, 0], "past_the_end": [0, 1, 0, 1, 1, 2, 0, 0],
                  "coordinate": [2, 1, 0, 1, 1, 0, 0, 0], "bad_counts": [0] * 8, "status_carried": [0, 1, 0, 1, 1, 0, 0, 0],
                  "rows_cut": [0, 1, 0, 0, 0, 0, 0, 0]}[change]
        assert got["valid"][:, 0].tolist() == expect, change
        assert got["counts"][7] == {"bad_counts": ST_BAD_COUNTS | 1, "status_carried": 5}.get(change, 0), change
        if change in ("bad_counts", "rows_cut"):
            assert not got["valid"][3:].any()


def test_two_calls_accumulate_in_stream_order():
    totals = torch.zeros(8, dtype=torch.int64, device=DEV)
    runs = []
    for name, status in (("interleaved", 0), ("flags", 4), ("spike", 1)):
        c = HAND_MADE[name]
        table = K.tables(c)
        table[2][4] = status                                 # the status is OR-ed in
        rc, got = _call(table, 0, c["max_ids"], totals=totals)
        assert rc == 0
        runs.append(got)
    t = totals.cpu().numpy()
    assert np.array_equal(t[:7], sum(r["counts"][:7] for r in runs)) and t[7] == 5
    assert t[:7].tolist() == [7, 3, 3, 0, 0, 3, 1]


def test_dirty_workspace_other_stream_and_repeatability():
    chunk = LIMITS()[1]
    rings = [K.star(3 * chunk + 5, 2, radius=9000, centre=(-9000, -9000)), K.P.square(9000, 9000, 40), K.star(33, 7, radius=4000, centre=(9000, -9000)),
             K.P.square(9010, 9010, 40), [(9000, 9000), (9040, 9040), (9040, 9000)]]
    c = K.case(rings, ids=[1, 2, 3, 2, 2])
    table = K.tables(c)
    want = V.valid(table, 0, c["max_ids"])
    runs = []
    for fill in (0x00, 0xA5, None, 0xFF):
        rc, got = _call(table, 0, c["max_ids"], fill_ws=fill)
        assert rc == 0
        _same(got, want)
        runs.append(got)
    d = [torch.from_numpy(a).to(DEV) for a in table]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    before = ops.launch_count()
    with torch.cuda.stream(side):
        out = ops.rings_valid(*d, 0, c["max_ids"])
        again = ops.rings_valid(*d, 0, c["max_ids"])
    side.synchronize()
    assert ops.launch_count() - before == 20, "the header documents 10 launches"
    assert all(torch.equal(a, b) for a, b in zip(out, again))
    assert all(np.array_equal(runs[0][n], t.cpu().numpy()) for n, t in zip(NAMES, out))


def test_refusals_enqueue_nothing():
    c = HAND_MADE["bow_tie"]
    table = K.tables(c)
    d = [torch.from_numpy(a).to(DEV) for a in table]
    out = [torch.zeros((c["max_ids"], 8), dtype=torch.int64, device=DEV), torch.zeros(8, dtype=torch.int64, device=DEV)]
    ws = _ws(table, c["max_ids"])
    ptrs = [d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), table[0].shape[0], table[1].shape[0], 0, c["max_ids"], 2 ** 32,
            out[0].data_ptr(), out[1].data_ptr(), None, ws.data_ptr(), 0]
    before = ops.launch_count()
    for slot in (0, 1, 2, 8, 9, 11):
        args = list(ptrs)
        args[slot] = None
        assert L.lib().c3d_rings_valid(*args) == E_BADARG, slot
    for slot in (3, 4, 6):
        for value in (0, -1):
            args = list(ptrs)
            args[slot] = value
            assert L.lib().c3d_rings_valid(*args) == E_BADARG, slot
    for value in (-1, 9):
        args = list(ptrs)
        args[5] = value
        assert L.lib().c3d_rings_valid(*args) == E_BADARG
    args = list(ptrs)
    args[7] = -1
    assert L.lib().c3d_rings_valid(*args) == E_BADARG
    ws_bytes = L.lib().c3d_rings_valid_ws_bytes
    for slot in range(3):
        sizes = [1] * 3
        sizes[slot] = 0
        assert ws_bytes(*sizes) == E_BADARG
    assert ws_bytes(1, 1, 1) > 0
    assert ops.launch_count() == before
    torch.cuda.synchronize()
    assert not any(t.any() for t in out)
    with pytest.raises(ValueError):
        ops.rings_valid(*d, 9)
    with pytest.raises(ValueError):
        ops.rings_valid(*d, 0, max_id_work=-1)
    with pytest.raises(L.Change3DHipError):
        ops.rings_valid(d[0].cpu(), *d[1:], 0)
    with pytest.raises(L.Change3DHipError):
        ops.rings_valid(*d, 0, max_objects=0)
    assert ops.launch_count() == before


@pytest.mark.parametrize("name,wrong", [("corner_shared", dict(strict=False)), ("spike", dict(adjacent_overlap=False)),
                                        ("interleaved", dict(ring_adjacency=False))])
def test_negative_controls_differ_from_the_device(name, wrong):
    c = HAND_MADE[name]
    table = K.tables(c)
    rc, got = _call(table, 0, c["max_ids"])
    bad = V.valid(table, 0, c["max_ids"], **wrong)
    assert rc == 0 and not np.array_equal(got["valid"][0, 4:], bad["valid"][0, 4:]), (name, wrong)
    _same(got, V.valid(table, 0, c["max_ids"]))
