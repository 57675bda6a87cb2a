"""`c3d_rings_fill` against its restatement (tests/fill_reference.py) and against the label maps its input was traced from:
labels, table, counts, info, mask and cls_map exactly equal.  Round trips through `scene_objects` / `scene_split`,
`scene_outlines` and `outlines_simplify` at tolerance 0; tables built by hand at four precisions; boxes on both sides of the
tier limits; overlap; bad rows; canaries, refusals, a dirty workspace, a non-default stream; two negative controls."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fill_cases as K  # noqa: E402
import fill_reference as R  # noqa: E402

from change3d_amd import _lib as L  # noqa: E402
from change3d_amd import ops  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
PAD, CANARY = 3, -7777
CANARY8 = 0xA5
OUT_NAMES = ("labels", "table", "counts_obj", "mask", "cls_map", "info")


def _call(rings, vertices, counts, Hs, Ws, f=0, id_cls=None, max_objects=16, ws=None, fill_ws=None, want_maps=True):
    """The C entry on output buffers with canary rows on both sides: (rc, dict of numpy outputs)."""
    d_in = [torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(DEV) for a in (rings, vertices, counts)]
    max_rings, max_vertices = d_in[0].shape[0], d_in[1].shape[0]
    d_cls = None if id_cls is None else torch.from_numpy(np.ascontiguousarray(id_cls, dtype=np.uint8)).to(DEV)
    bufs = dict(labels=torch.full((Hs + 2 * PAD, Ws), CANARY, dtype=torch.int32, device=DEV),
                table=torch.full((max_objects + 2 * PAD, 8), CANARY, dtype=torch.int32, device=DEV),
                counts_obj=torch.full((2 + 2 * PAD,), CANARY, dtype=torch.int32, device=DEV),
                mask=torch.full((Hs + 2 * PAD, Ws), CANARY8, dtype=torch.uint8, device=DEV),
                cls_map=torch.full((Hs + 2 * PAD, Ws), CANARY8, dtype=torch.uint8, device=DEV),
                info=torch.full((4 + 2 * PAD,), CANARY, dtype=torch.int32, device=DEV))
    if ws is None:
        ws = torch.empty(L.lib().c3d_rings_fill_ws_bytes(max_rings, max_vertices, max_objects, Hs, Ws), dtype=torch.uint8, device=DEV)
    if fill_ws is not None:
        ws.fill_(fill_ws)
    ptr = {k: v[PAD:].data_ptr() for k, v in bufs.items()}
    rc = L.lib().c3d_rings_fill(d_in[0].data_ptr(), d_in[1].data_ptr(), d_in[2].data_ptr(), max_rings, max_vertices, f,
                                None if d_cls is None else d_cls.data_ptr(), max_objects, Hs, Ws, ptr["labels"], ptr["table"],
                                ptr["counts_obj"], ptr["mask"] if want_maps else None, ptr["cls_map"] if want_maps else None,
                                ptr["info"], ws.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    out = {}
    for k, v in bufs.items():
        a = v.cpu().numpy()
        canary = CANARY8 if a.dtype == np.uint8 else CANARY
        assert (a[:PAD] == canary).all() and (a[len(a) - PAD:] == canary).all(), f"a canary row of {k} was written"
        out[k] = a[PAD:len(a) - PAD]
        if not want_maps and k in ("mask", "cls_map"):
            assert (out[k] == CANARY8).all()
    return rc, out


def _same(got, want, names=OUT_NAMES):
    for k in names:
        assert np.array_equal(got[k], want[k]), (k, np.argwhere(got[k] != want[k])[:6].tolist(), got["info"], want["info"])


def _check(rings, vertices, counts, Hs, Ws, f=0, id_cls=None, max_objects=16):
    want = R.fill(rings, vertices, counts, Hs, Ws, f, id_cls, max_objects)
    rc, got = _call(rings, vertices, counts, Hs, Ws, f, id_cls, max_objects)
    assert rc == 0
    _same(got, want)
    return want, got


# ------------------------------------------------------------------------------------------------------ round trips
@functools.lru_cache(maxsize=None)
def _masks(H, W):
    return K.masks(H, W)


def _round_trip(mask, connectivity, labelled=None, tol=None):
    """scene_objects (or the given labelling) -> scene_outlines [-> outlines_simplify] -> rings_fill gives the labels back."""
    Hs, Ws = mask.shape
    N = Hs * Ws
    m = torch.from_numpy(mask).to(DEV)
    if labelled is None:
        labels, table, _, _, counts = ops.scene_objects(m, connectivity=connectivity, max_objects=N)
    else:
        labels, table, counts = labelled
    rings, vertices, rc = ops.scene_outlines(labels, counts, connectivity=connectivity, max_objects=N, max_rings=N, max_vertices=4 * N)
    assert int(rc[4]) == 0
    if tol is not None:
        rings, vertices, rc = ops.outlines_simplify(rings, vertices, rc, tol)
        assert int(rc[4]) == 0
    back, table_b, counts_b, mask_b, _, info = ops.rings_fill(rings, vertices, rc, Hs, Ws, max_objects=N, want_mask=True)
    torch.cuda.synchronize()
    n = int(counts[1])
    assert torch.equal(back, labels)
    assert torch.equal(table_b[:, :5], table[:, :5]) and torch.equal(table_b[:, 6], table[:, 6]) and not table_b[:, 7].any()
    assert counts_b.tolist() == [n, n] and info.tolist() == [0, int(rc[1]), n, 0]
    assert torch.equal(mask_b, (labels > 0).to(torch.uint8))
    return n


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("shape", [(63, 65), (64, 64), (65, 130)])
def test_round_trip_gives_the_labels_back(shape, connectivity):
    for name, mask in _masks(*shape).items():
        n = _round_trip(mask, connectivity)
        assert (n == 0) == (name == "empty"), name


@pytest.mark.parametrize("connectivity", [4, 8])
def test_round_trip_on_the_widest_band(connectivity):
    assert _round_trip(K.wide_mask(70, 16384), connectivity) > 100


@pytest.mark.parametrize("connectivity", [4, 8])
def test_round_trip_of_split_pieces_that_share_edges(connectivity):
    mask = K.touching_mask(75, 110)
    m = torch.from_numpy(mask).to(DEV)
    N = mask.size
    whole = int(ops.scene_objects(m, connectivity=connectivity, max_objects=N)[4][1])
    labels, table, _, _, counts, info = ops.scene_split(m, 3.0, connectivity=connectivity, max_objects=N)
    assert int(info[0]) == 0 and int(counts[1]) > whole, "the split made pieces that touch"
    _round_trip(mask, connectivity, labelled=(labels, table, counts))


@pytest.mark.parametrize("connectivity", [4, 8])
def test_round_trip_through_the_simplifier_at_tolerance_zero(connectivity):
    for name in ("blobs", "ring_with_holes", "serpentine", "diagonal"):
        _round_trip(_masks(65, 130)[name], connectivity, tol=0.0)


# -------------------------------------------------------------------------------------------------- hand-built tables
@pytest.mark.parametrize("f", [0, 1, 4, 8])
@pytest.mark.parametrize("name", list(K.hand_built(0)))
def test_hand_built_tables(name, f):
    ring_lists, ids, max_objects = K.hand_built(f)[name]
    id_cls = (np.arange(max_objects) * 7 + 3).astype(np.uint8)
    want, got = _check(*R.table(ring_lists, ids), K.HS, K.WS, f, id_cls, max_objects)
    assert got["info"][0] == 0 and got["info"][1] == len(ring_lists) and got["info"][2] == max(ids)
    area = got["table"][:, 0]
    if name == "hole_and_twice":
        assert area[0] == 66 * 86 - 20 * 20 + 8 * 8 - 8 * 10 and area[1] == 0 and area[2] == 8 * 10, "hole, island, thrice = once"
        assert got["table"][1].tolist() == [0, 0, 0, 0, 0, int(id_cls[1]), 0, 0], "a ring listed twice cancels itself: zeros except cls"
    if name == "cw_and_ccw":
        assert area[0] == area[1] == 27 * 37, "orientation does not matter"
    if name == "degenerate":
        assert area[:5].tolist() == [0, 0, 0, 0, 0] and area[5] == 30 * 30 and got["counts_obj"].tolist() == [8, 8]
    if name == "outside":
        assert area[10] == 0 and area[0] > 0 and (got["labels"] > 0).all(), "id 1 covers the scene, id 11 lies outside"
    if name == "overlap":
        assert area[0] == 55 * 55 - 25 * 25 - 10 * 10 and area[1] == 25 * 25 - 10 * 10 and area[2] == 100
        assert area[3] == 0 and area[4] == 25 * 40, "identical polygons: the larger id owns every pixel"
        assert area[5] > 0 and area[6] > 0 and (got["labels"][want["labels"] == 6] == 6).all()


def _tier_table():
    """Boxes of T - 1, T and T + 1 rows or columns for each tier limit T, an object across three bands, in one table."""
    limits = sorted(set(ops.rings_fill_limits()))
    rings, ids, x = [], [], 2
    for T in limits:
        for w, h in ((T - 1, T - 1), (T, T), (T + 1, T), (T, T + 1), (T + 1, T + 1), (T, 3), (3, T + 1)):
            rings.append([(x, 2), (x + w, 2), (x + w, 2 + h), (x, 2 + h), (x + 2, 2 + h // 2)])   # a notch in the left side: no rectangle
            ids.append(len(ids) + 1)
            x += w + 2
    top = max(limits) + 6
    band = max(limits)
    rings.append([(5, top), (x - 3, top + 7), (x - 40, top + 2 * band + 9), (60, top + band)])           # spans three bands
    ids.append(len(ids) + 1)
    rings.append([(30, top + 20), (50, top + 20), (40, top + 2 * band)])                                 # a hole of it, over two
    ids.append(ids[-1])
    return rings, ids, top + 2 * band + 12, x + 2


def test_boxes_on_both_sides_of_the_tier_limits():
    assert all(8 <= v <= 4096 for v in ops.rings_fill_limits())
    rings, ids, Hs, Ws = _tier_table()
    want, got = _check(*R.table(rings, ids), Hs, Ws, 0, None, len(rings) + 1)
    t = got["table"]
    T = ops.rings_fill_limits()[0]
    assert (t[:5, 3] - t[:5, 1] + 1).tolist() == [T - 1, T, T + 1, T, T + 1] and (t[:5, 4] - t[:5, 2] + 1).tolist() == [T - 1, T, T, T + 1, T + 1]
    last = t[max(ids) - 1]
    assert last[4] - last[2] + 1 > 2 * ops.rings_fill_limits()[1], "three bands"


def test_three_thousand_one_pixel_objects():
    Hs, Ws = 100, 125
    cells = [(y, x) for y in range(0, Hs, 2) for x in range(0, Ws, 2)][:3000]
    rings = [K.rect(x, y, x + 1, y + 1, ccw=(k % 2 == 1)) for k, (y, x) in enumerate(cells)]
    want, got = _check(*R.table(rings), Hs, Ws, 0, None, 3001)
    assert got["counts_obj"].tolist() == [3000, 3000] and (got["table"][:3000, 0] == 1).all() and got["table"][3000].tolist() == [0] * 8
    assert got["labels"][cells[2999]] == 3000


# ------------------------------------------------------------------------------------------------------------ bad rows
def _mixed_table(f=0):
    lists, ids, _ = K.hand_built(f)["scattered"]
    return R.table(lists, ids, max_rings=len(lists) + 2, max_vertices=sum(len(v) for v in lists) + 4)


def test_pass_through_and_bad_rows():
    rings, vertices, counts = _mixed_table()
    rings[4, 1] = -1                                         # the simplifier's pass-through: skipped silently, whatever its id
    rings[4, 0] = 99
    want, got = _check(rings, vertices, counts, K.HS, K.WS, 0, None, 3)
    assert got["info"].tolist() == [0, 6, 3, 0]
    for change, bit in (("n_past_the_end", R.ST_BAD_RING), ("negative_n", R.ST_BAD_RING), ("coordinate", R.ST_BAD_RING),
                        ("negative_coordinate", R.ST_BAD_RING), ("id_zero", R.ST_BAD_ID), ("id_above", R.ST_BAD_ID),
                        ("id_and_ring", R.ST_BAD_ID | R.ST_BAD_RING)):
        rings, vertices, counts = _mixed_table()
        counts[4] = 1                                        # C3D_OUTLINE_ST_TRUNCATED is carried along
        row = 4
        if change == "n_past_the_end":
            rings[row, 2] = int(counts[3]) - int(rings[row, 1]) + 1
        elif change == "negative_n":
            rings[row, 2] = -5
        elif change == "coordinate":
            vertices[int(rings[row, 1]) + 2] = (32769, 3)
        elif change == "negative_coordinate":
            vertices[int(rings[row, 1]) + 1] = (3, -32769)
        elif change == "id_zero":
            rings[row, 0] = 0
        elif change == "id_above":
            rings[row, 0] = 4
        else:
            rings[row, 0], rings[row, 2] = -3, 1 << 30
        want, got = _check(rings, vertices, counts, K.HS, K.WS, 0, None, 3)
        assert got["info"].tolist() == [1 | bit, 6, 3, 0], change
        assert got["labels"][22, 3] == 0 and got["labels"][50, 30] == 1, "without its outer ring the hole of id 1 is the object"
    rings, vertices, counts = _mixed_table()
    counts[1] = 4                                            # fewer rows than the table holds: only those are read
    want, got = _check(rings, vertices, counts, K.HS, K.WS, 0, None, 3)
    assert got["info"].tolist() == [0, 4, 3, 0]
    counts[1] = 1000                                         # more rows than the table has; the rows past the rings have n = 0, id 0
    want, got = _check(rings, vertices, counts, K.HS, K.WS, 0, None, 3)
    assert got["info"].tolist() == [R.ST_BAD_ID, 7, 3, 0]


def test_bad_counts_fill_nothing():
    rings, vertices, counts = _mixed_table()
    counts[4] = R.ST_BAD_COUNTS | 1
    want, got = _check(rings, vertices, counts, K.HS, K.WS, 0, np.full(3, 9, dtype=np.uint8), 3)
    assert got["counts_obj"].tolist() == [-1, 0] and got["info"].tolist() == [R.ST_BAD_COUNTS | 1, 0, 0, 0]
    assert not got["labels"].any() and not got["table"].any() and not got["mask"].any() and not got["cls_map"].any()


# ---------------------------------------------------------------------------------------------------------- robustness
def test_refusals_leave_the_outputs_untouched():
    rings, vertices, counts = (torch.from_numpy(a).to(DEV) for a in _mixed_table())
    Hs, Ws, max_objects = K.HS, K.WS, 3
    ws = torch.empty(L.lib().c3d_rings_fill_ws_bytes(len(rings), len(vertices), max_objects, Hs, Ws), dtype=torch.uint8, device=DEV)
    outs = dict(labels=torch.full((Hs, Ws), CANARY, dtype=torch.int32, device=DEV), table=torch.full((max_objects, 8), CANARY, dtype=torch.int32, device=DEV),
                counts_obj=torch.full((2,), CANARY, dtype=torch.int32, device=DEV), mask=torch.full((Hs, Ws), CANARY8, dtype=torch.uint8, device=DEV),
                cls_map=torch.full((Hs, Ws), CANARY8, dtype=torch.uint8, device=DEV), info=torch.full((4,), CANARY, dtype=torch.int32, device=DEV))
    good = dict(rings=rings.data_ptr(), vertices=vertices.data_ptr(), counts=counts.data_ptr(), max_rings=len(rings), max_vertices=len(vertices),
                frac_bits=0, id_cls=None, max_objects=max_objects, Hs=Hs, Ws=Ws, labels=outs["labels"].data_ptr(), table=outs["table"].data_ptr(),
                counts_obj=outs["counts_obj"].data_ptr(), mask=outs["mask"].data_ptr(), cls_map=outs["cls_map"].data_ptr(),
                info=outs["info"].data_ptr(), ws=ws.data_ptr())
    badarg = [dict(rings=None), dict(vertices=None), dict(counts=None), dict(labels=None), dict(table=None), dict(counts_obj=None), dict(info=None),
              dict(ws=None), dict(max_rings=0), dict(max_vertices=-1), dict(max_objects=0), dict(frac_bits=-1), dict(frac_bits=9), dict(Hs=0), dict(Ws=-3)]
    stream = torch.cuda.current_stream().cuda_stream
    for change in badarg:
        assert L.lib().c3d_rings_fill(*{**good, **change}.values(), stream) == -1, change                  # C3D_E_BADARG
    for change in (dict(Hs=16385), dict(Ws=16385)):
        assert L.lib().c3d_rings_fill(*{**good, **change}.values(), stream) == -2, change                  # C3D_E_UNSUPPORTED
    assert L.lib().c3d_rings_fill_ws_bytes(0, 1, 1, 1, 1) == -1 and L.lib().c3d_rings_fill_ws_bytes(1, 1, 1, 16385, 1) == -2
    torch.cuda.synchronize()
    for k, v in outs.items():
        assert (v == (CANARY8 if v.dtype == torch.uint8 else CANARY)).all(), k
    assert L.lib().c3d_rings_fill(*good.values(), stream) == 0
    torch.cuda.synchronize()
    assert outs["info"].tolist() == [0, 7, 3, 0]


def test_two_calls_agree_bit_for_bit_also_on_a_dirty_workspace():
    rings, ids, Hs, Ws = _tier_table()
    table = R.table(rings, ids)
    n = len(rings) + 1
    ws = torch.empty(L.lib().c3d_rings_fill_ws_bytes(len(table[0]), len(table[1]), n, Hs, Ws), dtype=torch.uint8, device=DEV)
    first = _call(*table, Hs, Ws, 0, None, n, ws=ws, fill_ws=0)
    again = _call(*table, Hs, Ws, 0, None, n, ws=ws)           # what the first call left behind
    dirty = _call(*table, Hs, Ws, 0, None, n, ws=ws, fill_ws=0xFF)
    other = _call(*R.table(rings[:9], ids[:9], max_rings=len(table[0]), max_vertices=len(table[1])), Hs, Ws, 0, None, n, ws=ws)
    back = _call(*table, Hs, Ws, 0, None, n, ws=ws, want_maps=False)
    assert first[0] == 0 and other[0] == 0 and other[1]["info"][2] == ids[8] < first[1]["info"][2] + 1
    for run in (again, dirty):
        assert run[0] == 0
        _same(run[1], first[1])
    _same(back[1], first[1], ("labels", "table", "counts_obj", "info"))


def test_non_default_stream_and_the_python_op():
    ring_lists, ids, max_objects = K.hand_built(4)["scattered"]
    table = R.table(ring_lists, ids)
    id_cls = np.array([4, 2, 9], dtype=np.uint8)
    want = R.fill(*table, K.HS, K.WS, 4, id_cls, max_objects)
    dev = [torch.from_numpy(a).to(DEV) for a in table]
    cls = torch.from_numpy(id_cls).to(DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        out = ops.rings_fill(*dev, K.HS, K.WS, frac_bits=4, id_cls=cls, max_objects=max_objects, want_mask=True, want_cls_map=True)
        bare = ops.rings_fill(*dev, K.HS, K.WS, frac_bits=4, max_objects=max_objects)
    side.synchronize()
    _same(dict(zip(OUT_NAMES, (t.cpu().numpy() for t in out))), want)
    assert bare[3] is None and bare[4] is None and np.array_equal(bare[0].cpu().numpy(), want["labels"]) and not bare[1][:, 5].any()
    with pytest.raises(ValueError):
        ops.rings_fill(*dev, K.HS, K.WS, frac_bits=9)
    with pytest.raises(L.Change3DHipError):
        ops.rings_fill(*dev, 16385, K.WS)
    with pytest.raises(L.Change3DHipError):
        ops.rings_fill(dev[0].cpu(), dev[1], dev[2], K.HS, K.WS)


def test_negative_controls_see_strictness_and_the_parity_rule():
    for name, f, variant in (("strictness", 1, dict(strict=False)), ("stars_and_triangles", 0, dict(winding=True))):
        ring_lists, ids, max_objects = K.hand_built(f)[name]
        table = R.table(ring_lists, ids)
        rc, got = _call(*table, K.HS, K.WS, f, None, max_objects)
        wrong = R.fill(*table, K.HS, K.WS, f, None, max_objects, **variant)
        assert rc == 0 and not np.array_equal(got["labels"], wrong["labels"]), (name, variant)
