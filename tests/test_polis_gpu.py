"""`c3d_rings_polis` against its restatement (tests/polis_reference.py) through the C ABI, with canary rows round every output:
integers exactly equal, doubles within the bound derived in the header -- a distance within 8 u of the exact one, a mean over
n of them within (n + 8) u, PoLiS within (n_p + n_g + 16) u, u = 2^-53 -- and exactly equal where the value is 0.  The
smallest shapes that reach each path: both tiers, the sizes round a job and an LDS tile, an id of interleaved rings with a
hole, the ring-ordering limit, mixed frac_bits at the corners of the coordinate range, degenerate edges, every flag, the
work cap on both sides, accumulation in stream order, a dirty workspace and another stream, refusals, and three negative
controls."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import polis_cases as K  # noqa: E402
import polis_reference as R  # noqa: E402

from change3d_amd import _lib as L  # noqa: E402
from change3d_amd import ops  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
PAD, CANARY = 3, -7777
E_BADARG = -1                                                # C3D_E_BADARG
NAMES = ("pair", "pair_n", "counts", "sums")
U = 2.0 ** -53
HAND_MADE = K.hand_made()
LIMITS = functools.lru_cache(maxsize=None)(lambda: ops.rings_polis_limits())


def _ws(tp, tg, max_p, max_g):
    n = L.lib().c3d_rings_polis_ws_bytes(tp[0].shape[0], tp[1].shape[0], max_p, tg[0].shape[0], tg[1].shape[0], max_g)
    assert n > 0
    return torch.empty(n, dtype=torch.uint8, device=DEV)


def _call(tp, f_p, tg, f_g, match, max_g, max_pair_work=2 ** 32, totals=None, total_sums=None, fill_ws=None):
    """The C entry on output buffers with canary rows on both sides: (rc, dict of numpy outputs)."""
    d = [torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(DEV) for a in tp + tg + (match,)]
    max_p = match.shape[0]
    pair = torch.full((max_p + 2 * PAD, 4), float(CANARY), dtype=torch.float64, device=DEV)
    pair_n = torch.full((max_p + 2 * PAD, 4), CANARY, dtype=torch.int32, device=DEV)
    counts = torch.full((8 + 2 * PAD,), CANARY, dtype=torch.int64, device=DEV)
    sums = torch.full((4 + 2 * PAD,), float(CANARY), dtype=torch.float64, device=DEV)
    ws = _ws(tp, tg, max_p, max_g)
    if fill_ws is not None:
        ws.fill_(fill_ws)
    rc = L.lib().c3d_rings_polis(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), tp[0].shape[0], tp[1].shape[0], f_p,
                                 d[3].data_ptr(), d[4].data_ptr(), d[5].data_ptr(), tg[0].shape[0], tg[1].shape[0], f_g,
                                 d[6].data_ptr(), max_p, max_g, max_pair_work, pair[PAD:].data_ptr(), pair_n[PAD:].data_ptr(),
                                 counts[PAD:].data_ptr(), sums[PAD:].data_ptr(), None if totals is None else totals.data_ptr(),
                                 None if total_sums is None else total_sums.data_ptr(), ws.data_ptr(),
                                 torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    bufs = [b.cpu().numpy() for b in (pair, pair_n, counts, sums)]
    for buf in bufs:
        assert (buf[:PAD] == CANARY).all() and (buf[len(buf) - PAD:] == CANARY).all(), "a canary row was written"
    return rc, dict(zip(NAMES, (b[PAD:len(b) - PAD] for b in bufs)))


def _close(got, want, bound, what):
    """|got - want| <= bound * |want| element by element, and equality wherever the restatement gives 0."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert np.array_equal(got[want == 0], want[want == 0]), what
    err = np.abs(got - want)
    assert (err <= bound * np.abs(want)).all(), (what, (err / np.maximum(np.abs(want), 1e-300) / U).max())


def _same(got, want):
    assert np.array_equal(got["pair_n"], want["pair_n"]), (got["pair_n"], want["pair_n"])
    assert np.array_equal(got["counts"], want["counts"]), (got["counts"], want["counts"])
    _close(got["pair"], want["pair"], R.bounds(want["pair_n"]), "pair")
    scored = want["pair_n"][:, 3] == 0
    widest = float((want["pair_n"][:, 1] + want["pair_n"][:, 2])[scored].max(initial=0)) + 16 + int(want["counts"][0])
    _close(got["sums"][[0, 1, 3]], want["sums"][[0, 1, 3]], widest * U, "sums")
    _close(got["sums"][2:3], want["sums"][2:3], 8 * U, "max")
    assert got["sums"][2] == got["pair"][:, 1].max(initial=0.0)


def _check(c, **kw):
    tp, tg, match = K.tables(c)
    ref_kw = {k: v for k, v in kw.items() if k == "max_pair_work"}
    want = R.polis(tp, c["P"][2], tg, c["G"][2], match, c["max_g"], ring_limit=LIMITS()[3], **ref_kw)
    rc, got = _call(tp, c["P"][2], tg, c["G"][2], match, c["max_g"], **kw)
    assert rc == 0
    _same(got, want)
    return want, got


@pytest.mark.parametrize("name", list(HAND_MADE))
def test_hand_made_tables(name):
    want, got = _check(HAND_MADE[name])
    assert got["counts"][6] == 0 and got["counts"][0] >= 1
    if name == "holes_interleaved":
        assert got["pair_n"][0].tolist() == [2, 4, 12, 0] and got["pair"][0, 2] == 3.5, "the hole ring is the nearest boundary"
        assert not got["pair"][1].any(), "identical triangles"
    if name == "flags":
        assert got["pair_n"][:, 3].tolist() == [0, 1, 2, 0, 2, 1, 0, 0]
    if name.startswith("frac"):
        assert got["pair"][0, 1] > 0 and got["pair"][0, 1] < 65536


def test_the_first_sizes_of_the_job_tier_and_the_sizes_round_a_job_and_a_tile():
    wave, chunk, tile = LIMITS()[:3]
    assert wave == 64 and chunk >= wave and tile >= 64
    for n_p, n_g in ((wave, wave), (wave + 1, 3), (3, wave + 1), (chunk, tile + 1), (chunk + 1, tile + 1), (2 * chunk + 1, tile + 1)):
        want, got = _check(K.sized(n_p, n_g, seed=n_p))
        assert got["pair_n"][0].tolist() == [1, n_p, n_g, 0] and got["pair"][0, 0] > 0
    assert "polis_totals_kernel" in ops.last_kernel()


def test_both_tiers_and_every_flag_in_one_table():
    wave, chunk, tile = LIMITS()[:3]
    P = [K.polygon(n, seed=n, centre=(20000 * (k % 3) - 20000, 20000 * (k // 3) - 20000)) for k, n in enumerate((5, chunk + 7, 30, 2 * chunk + 3, 64, 9))]
    G = [K.polygon(n, seed=n + 1, centre=(20000 * (k % 3) - 19900, 20000 * (k // 3) - 20050)) for k, n in enumerate((7, 40, tile + 3, chunk + 1, 64, 9))]
    c = K.case(P, G, {1: 1, 2: 2, 3: 3, 4: 4, 5: 5, 6: 0}, max_p=9, max_g=8)
    want, got = _check(c)
    assert got["counts"][:4].tolist() == [5, 1, 0, 0]


def test_an_id_on_each_side_of_the_ring_limit():
    limit = LIMITS()[3]
    rings_p, ids_p = [], []
    for k in range(2 * limit + 1):                           # id 1 gets `limit` rings, id 2 one more, interleaved
        rings_p.append(K.square(12 * ((k // 2) % 256), 60 * ((k // 2) // 256) + 30 * (k % 2), 5))
        ids_p.append(2 if k == 2 * limit else 1 + k % 2)
    c = K.case(rings_p, [K.square(1, 1, 5), K.square(1, 31, 5)], {1: 1, 2: 2}, ids_p=ids_p)
    want, got = _check(c)
    assert got["pair_n"][:2].tolist() == [[1, 4 * limit, 4, 0], [2, 0, 4, 2]]


def test_rings_on_both_sides_of_the_length_that_many_workgroups_share():
    big = LIMITS()[4]
    P = [K.polygon(big, 1, radius=20000), K.square(30000, 30000, 50), K.polygon(big + 1, 2, radius=25000), K.polygon(2 * big + 77, 3, radius=30000)]
    G = [K.square(0, 0, 9000), K.square(30010, 30010, 40), K.polygon(5, 9, radius=24000)]
    c = K.case(P, G, {1: 1, 2: 2, 3: 3}, ids_p=[1, 2, 3, 1])  # id 1: a ring of the limit, then one of twice that, not contiguous
    want, got = _check(c)
    assert got["pair_n"][:3].tolist() == [[1, 3 * big + 77, 4, 0], [2, 4, 4, 0], [3, big + 1, 5, 0]]
    tp, tg, match = K.tables(c)
    tp[1][int(tp[0][3, 1]) + 2 * big + 50, 1] = -32769         # one coordinate out of range deep inside the longest ring
    rc, got = _call(tp, 0, tg, 0, match, c["max_g"])
    assert rc == 0 and got["pair_n"][:3, 3].tolist() == [2, 0, 0] and got["pair_n"][0, 1] == 0
    _same(got, R.polis(tp, 0, tg, 0, match, c["max_g"]))


def test_start_below_zero_bad_rows_bad_partner_and_bad_counts():
    c = HAND_MADE["flags"]
    for change in ("start", "negative_n", "past_the_end", "coordinate", "partner", "partner_negative", "bad_counts_p", "bad_counts_g",
                   "status_carried", "gt_incomplete"):
        tp, tg, match = K.tables(c)
        if change == "start":
            tp[0][0, 1] = -1
        elif change == "negative_n":
            tp[0][3, 2] = -4
        elif change == "past_the_end":
            tp[0][3, 2] = int(tp[2][3]) - int(tp[0][3, 1]) + 1
        elif change == "coordinate":
            tp[1][1, 0] = 32769
        elif change == "partner":
            match[5, 0] = c["max_g"] + 1
        elif change == "partner_negative":
            match[0, 0] = -1
        elif change == "bad_counts_p":
            tp[2][4] = R.ST_BAD_COUNTS
        elif change == "bad_counts_g":
            tg[2][4] = R.ST_BAD_COUNTS | 1
        elif change == "status_carried":
            tp[2][4], tg[2][4] = 1, 4
        elif change == "gt_incomplete":
            tg[0][3, 1] = -1
        want = R.polis(tp, 0, tg, 0, match, c["max_g"])
        rc, got = _call(tp, 0, tg, 0, match, c["max_g"])
        assert rc == 0
        _same(got, want)
        expect = {"start": [2, 1, 2, 0, 2, 1, 0, 0], "negative_n": [0, 1, 2, 2, 2, 1, 0, 0], "past_the_end": [0, 1, 2, 2, 2, 1, 0, 0],
                  "coordinate": [2, 1, 2, 0, 2, 1, 0, 0], "partner": [0, 1, 2, 0, 2, 1, 0, 0], "partner_negative": [1, 1, 2, 0, 2, 1, 0, 0],
                  "bad_counts_p": [0] * 8, "bad_counts_g": [2, 1, 2, 2, 2, 1, 0, 0], "status_carried": [0, 1, 2, 0, 2, 1, 0, 0],
                  "gt_incomplete": [0, 1, 2, 2, 2, 1, 0, 0]}[change]
        assert got["pair_n"][:, 3].tolist() == expect, change
        status = {"partner": R.ST_BAD_PARTNER, "partner_negative": R.ST_BAD_PARTNER, "bad_counts_p": R.ST_BAD_COUNTS,
                  "bad_counts_g": R.ST_BAD_COUNTS | 1, "status_carried": 5}.get(change, 0)
        assert got["counts"][6] == status, change


def test_the_work_cap_on_both_sides():
    for c, n_p, n_g in ((HAND_MADE["triangles"], 3, 3), (K.sized(70, 9, seed=4), 70, 9)):
        want, got = _check(c, max_pair_work=2 * n_p * n_g)
        assert got["pair_n"][0, 3] == 0
        want, got = _check(c, max_pair_work=2 * n_p * n_g - 1)
        assert got["pair_n"][0].tolist() == [1, n_p, n_g, 3] and got["counts"][:4].tolist() == [0, 0, 0, 1] and not got["pair"].any()
    want, got = _check(HAND_MADE["triangles"], max_pair_work=0)
    assert got["counts"][3] == 1


def test_two_calls_accumulate_in_stream_order():
    totals = torch.zeros(8, dtype=torch.int64, device=DEV)
    total_sums = torch.zeros(4, dtype=torch.float64, device=DEV)
    runs = []
    for name in ("holes_interleaved", "flags"):
        c = HAND_MADE[name]
        tp, tg, match = K.tables(c)
        if name == "flags":
            match[5, 0] = 77                                 # the status bit is OR-ed in
        rc, got = _call(tp, 0, tg, 0, match, c["max_g"], totals=totals, total_sums=total_sums)
        assert rc == 0
        runs.append(got)
    t, s = totals.cpu().numpy(), total_sums.cpu().numpy()
    assert np.array_equal(t[:6], runs[0]["counts"][:6] + runs[1]["counts"][:6]) and t[6] == R.ST_BAD_PARTNER and t[7] == 0
    assert s[0] == runs[0]["sums"][0] + runs[1]["sums"][0] and s[1] == runs[0]["sums"][1] + runs[1]["sums"][1]
    assert s[2] == max(runs[0]["sums"][2], runs[1]["sums"][2]) and s[3] == runs[0]["sums"][3] + runs[1]["sums"][3]


def test_dirty_workspace_other_stream_and_repeatability():
    wave, chunk, tile = LIMITS()[:3]
    P = [K.polygon(2 * chunk + 5, 1), K.square(9000, 9000, 40), K.polygon(33, 3, centre=(-9000, 9000)), K.square(9010, 9010, 10)[::-1]]
    G = [K.polygon(tile + 9, 2, centre=(60, 10)), K.polygon(12, 4, radius=60, centre=(9020, 9020)), K.polygon(wave, 5, centre=(-9100, 9000))]
    c = K.case(P, G, {1: 1, 2: 2, 3: 3}, ids_p=[1, 2, 3, 2])
    tp, tg, match = K.tables(c)
    want = R.polis(tp, 0, tg, 0, match, c["max_g"])
    runs = []
    for fill in (0x00, 0xA5, None, 0xFF):
        rc, got = _call(tp, 0, tg, 0, match, c["max_g"], fill_ws=fill)
        assert rc == 0
        _same(got, want)
        runs.append(got)
    for other in runs[1:]:
        assert all(np.array_equal(runs[0][n], other[n]) for n in NAMES), "two runs differ in a bit"
    d = [torch.from_numpy(a).to(DEV) for a in tp + tg + (match,)]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    before = ops.launch_count()
    with torch.cuda.stream(side):
        out = ops.rings_polis(*d[:3], 0, *d[3:6], 0, d[6], c["max_g"])
        again = ops.rings_polis(*d[:3], 0, *d[3:6], 0, d[6], c["max_g"])
    side.synchronize()
    assert ops.launch_count() - before == 20, "the header documents 10 launches"
    assert all(torch.equal(a, b) for a, b in zip(out, again))
    assert all(np.array_equal(runs[0][n], t.cpu().numpy()) for n, t in zip(NAMES, out))


def test_refusals_enqueue_nothing():
    c = HAND_MADE["triangles"]
    tp, tg, match = K.tables(c)
    d = [torch.from_numpy(a).to(DEV) for a in tp + tg + (match,)]
    out = [torch.zeros((match.shape[0], 4), dtype=torch.float64, device=DEV), torch.zeros((match.shape[0], 4), dtype=torch.int32, device=DEV),
           torch.zeros(8, dtype=torch.int64, device=DEV), torch.zeros(4, dtype=torch.float64, device=DEV)]
    ws = _ws(tp, tg, match.shape[0], c["max_g"])
    ptrs = [d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), tp[0].shape[0], tp[1].shape[0], 0, d[3].data_ptr(), d[4].data_ptr(),
            d[5].data_ptr(), tg[0].shape[0], tg[1].shape[0], 0, d[6].data_ptr(), match.shape[0], c["max_g"], 2 ** 32] + \
           [t.data_ptr() for t in out] + [None, None, ws.data_ptr(), 0]
    before = ops.launch_count()
    for slot in (0, 1, 2, 6, 7, 8, 12, 16, 17, 18, 19, 22):
        args = list(ptrs)
        args[slot] = None
        assert L.lib().c3d_rings_polis(*args) == E_BADARG, slot
    for slot in (3, 4, 9, 10, 13, 14):
        for value in (0, -1):
            args = list(ptrs)
            args[slot] = value
            assert L.lib().c3d_rings_polis(*args) == E_BADARG, slot
    for slot in (5, 11):
        for value in (-1, 9):
            args = list(ptrs)
            args[slot] = value
            assert L.lib().c3d_rings_polis(*args) == E_BADARG, slot
    args = list(ptrs)
    args[15] = -1
    assert L.lib().c3d_rings_polis(*args) == E_BADARG
    ws_bytes = L.lib().c3d_rings_polis_ws_bytes
    for slot in range(6):
        sizes = [1] * 6
        sizes[slot] = 0
        assert ws_bytes(*sizes) == E_BADARG
    assert ws_bytes(1, 1, 1, 1, 1, 1) > 0
    assert ops.launch_count() == before
    torch.cuda.synchronize()
    assert not any(t.any() for t in out)
    with pytest.raises(ValueError):
        ops.rings_polis(*d[:3], 9, *d[3:6], 0, d[6], c["max_g"])
    with pytest.raises(ValueError):
        ops.rings_polis(*d[:3], 0, *d[3:6], 0, d[6], c["max_g"], max_pair_work=-1)
    with pytest.raises(L.Change3DHipError):
        ops.rings_polis(d[0].cpu(), *d[1:3], 0, *d[3:6], 0, d[6], c["max_g"])
    with pytest.raises(L.Change3DHipError):
        ops.rings_polis(*d[:3], 0, *d[3:6], 0, d[6], 0)
    assert ops.launch_count() == before


@pytest.mark.parametrize("name,wrong", [("squares_apart", dict(segment=False)), ("holes_interleaved", dict(join=True)),
                                        ("triangles", dict(closing=False))])
def test_negative_controls_differ_from_the_device_beyond_the_bound(name, wrong):
    c = HAND_MADE[name]
    tp, tg, match = K.tables(c)
    rc, got = _call(tp, c["P"][2], tg, c["G"][2], match, c["max_g"])
    bad = R.polis(tp, c["P"][2], tg, c["G"][2], match, c["max_g"], **wrong)
    bound = R.bounds(bad["pair_n"])[0, 0]
    assert rc == 0 and abs(got["pair"][0, 0] - bad["pair"][0, 0]) > 1000 * bound * max(got["pair"][0, 0], bad["pair"][0, 0]), (name, wrong)
