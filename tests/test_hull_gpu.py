"""`c3d_rings_hull` against its restatement (tests/hull_reference.py): hull rows, hull vertices, rectangle rows and counts
exactly equal.  Hand-made tables, point clouds on both sides of every tier limit in one table, hulls with more vertices than
a workgroup is wide in every upper tier, ties, two negative controls, truncation, pass-through and bad rows with canaries,
refusals, determinism on a dirty workspace and a non-default stream, and traced masks whose hulls are filled back."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fill_cases as FK  # noqa: E402
import hull_cases as K  # noqa: E402
import hull_reference as R  # noqa: E402
import simplify_cases as SK  # noqa: E402
from simplify_reference import table as make_table  # noqa: E402

from change3d_amd import _lib as L  # noqa: E402
from change3d_amd import ops  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
PAD, CANARY = 3, -7777
E_BADARG = -1                                                # C3D_E_BADARG
NAMES = ("hulls", "vertices", "rects", "counts")


def _call(rings, vertices, counts, max_objects, max_hull_vertices, ws=None, fill_ws=None):
    """The C entry on output buffers with canary rows on both sides: (rc, dict of numpy outputs)."""
    max_rings, max_vertices = rings.shape[0], vertices.shape[0]
    d_in = [torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(DEV) for a in (rings, vertices, counts)]
    h_out = torch.full((max_objects + 2 * PAD, 8), CANARY, dtype=torch.int32, device=DEV)
    v_out = torch.full((max_hull_vertices + 2 * PAD, 2), CANARY, dtype=torch.int32, device=DEV)
    r_out = torch.full((max_objects + 2 * PAD, 8), CANARY, dtype=torch.int64, device=DEV)
    c_out = torch.full((5 + 2 * PAD,), CANARY, dtype=torch.int32, device=DEV)
    if ws is None:
        ws = torch.empty(L.lib().c3d_rings_hull_ws_bytes(max_rings, max_vertices, max_objects), dtype=torch.uint8, device=DEV)
    if fill_ws is not None:
        ws.fill_(fill_ws)
    rc = L.lib().c3d_rings_hull(d_in[0].data_ptr(), d_in[1].data_ptr(), d_in[2].data_ptr(), max_rings, max_vertices, max_objects,
                                max_hull_vertices, h_out[PAD:].data_ptr(), v_out[PAD:].data_ptr(), r_out[PAD:].data_ptr(),
                                c_out[PAD:].data_ptr(), ws.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    bufs = [b.cpu().numpy() for b in (h_out, v_out, r_out, c_out)]
    for buf in bufs:
        assert (buf[:PAD] == CANARY).all() and (buf[len(buf) - PAD:] == CANARY).all(), "a canary row was written"
    return rc, dict(zip(NAMES, (b[PAD:len(b) - PAD] for b in bufs)))


def _same(got, want):
    assert np.array_equal(got["counts"], want["counts"]), (got["counts"], want["counts"])
    assert np.array_equal(got["hulls"], want["hulls"]), (np.argwhere(got["hulls"] != want["hulls"])[:5], got["hulls"][:4], want["hulls"][:4])
    assert np.array_equal(got["rects"], want["rects"]), (np.argwhere(got["rects"] != want["rects"])[:5], got["rects"][:4], want["rects"][:4])
    written = int(got["counts"][3])
    assert np.array_equal(got["vertices"][:written], want["vertices"][:written])
    assert (got["vertices"][written:] == CANARY).all(), "a vertex row past counts_out[3] was written"


def _check(table, max_objects, max_hull_vertices=None, fast=False, **kw):
    """Device against restatement: exact.  Returns (restatement, device outputs)."""
    rings, vertices, counts = table
    max_hull_vertices = vertices.shape[0] if max_hull_vertices is None else max_hull_vertices
    want = R.hulls(rings, vertices, counts, max_objects, max_hull_vertices, fast=fast)
    rc, got = _call(rings, vertices, counts, max_objects, max_hull_vertices, **kw)
    assert rc == 0
    _same(got, want)
    return want, got


def _table(ring_lists, ids, spare_rings=2, spare_vertices=3):
    return make_table(ring_lists, max_rings=len(ring_lists) + spare_rings, max_vertices=sum(len(v) for v in ring_lists) + spare_vertices,
                      ids=ids)


HAND_MADE = K.hand_made()
LIMITS = functools.lru_cache(maxsize=None)(lambda: ops.rings_hull_limits())


@pytest.mark.parametrize("name", list(HAND_MADE))
def test_hand_made_tables(name):
    ring_lists, ids = HAND_MADE[name]
    want, got = _check(_table(ring_lists, ids), max_objects=max(ids) + 2)
    h, r, c = got["hulls"], got["rects"], got["counts"]
    assert c[4] == 0 and c[1] == max(ids) and (h[max(ids):] == 0).all() and (r[max(ids):] == 0).all()
    if name == "single_point":
        assert h[0].tolist() == [1, 0, 1, 0, 0, 5, 7, 1] and r[0].tolist() == [-1, 0, 0, 0, 0, 0, 0, 0]
    if name == "two_points":
        assert h[0].tolist() == [1, 0, 2, 0, 0, 9, 3, 2] and got["vertices"][:2].tolist() == [[9, 3], [2, 8]] and r[0, 0] == -1
    if name == "collinear":
        assert h[0, 2] == 2 and got["vertices"][:2].tolist() == [[1, 1], [9, 5]] and h[0, 7] == 5
    if name == "duplicates":
        assert h[0, 2:4].tolist() == [4, 50] and h[0, 7] == 9
    if name == "side_points":
        assert got["vertices"][:4].tolist() == [[2, 2], [10, 2], [10, 10], [2, 10]] and h[0, 3] == 128
    if name == "plus":
        assert h[0, 2] == 8 and h[0, 5:7].tolist() == [2, 0]
    if name == "holed":
        assert h[0, 2] == 4 and h[0, 7] == 8 and c[0] == 1
    if name == "interleaved":
        assert h[:2, 1].tolist() == [0, int(h[0, 2])] and c[0] == 2
    if name == "gap":
        assert h[1].tolist() == [2, -1, 0, 0, 0, 0, 0, 0] and r[1, 0] == -1 and h[2, 1] == 4 and c[:2].tolist() == [2, 3]
    if name == "full_range":
        assert r[0, 1] == 16383 ** 2 + 1 and r[0, 0] == 0
    if name == "axis_rectangle":
        assert r[0].tolist() == [0, 81, 0, 81, 45, 0, 1, 2], "four equal areas: the first edge wins"
    if name == "diamond":
        assert r[0, 0] == 0 and r[0, 1] == 72 and (r[0, 3] - r[0, 2]) * r[0, 4] == 72 * 72
    if name == "thin_diagonal":
        assert r[0, 0] == 1, "the rectangle on the long diagonal edge is the smallest"


@pytest.mark.parametrize("which", [0, 1])
def test_clouds_on_both_sides_of_a_tier_limit(which):
    T = LIMITS()[which]
    assert 4 <= LIMITS()[0] < LIMITS()[1] <= 1 << 20
    small = [[(1, 1), (9, 1), (9, 5)], [(3, 2), (4, 2), (4, 3), (3, 3)]]
    ring_lists, ids = [], []
    for k, n in enumerate((T - 1, T, T + 1)):                # small ids between the clouds: the tiers alternate along the table
        pts = K.cloud(n, seed=10 * which + k)
        half = n // 2
        ring_lists += [pts[:half], small[k % 2], pts[half:]]  # a cloud in two rings that are not neighbours
        ids += [3 * k + 1, 3 * k + 2, 3 * k + 1]
    want, got = _check(_table(ring_lists, ids), max_objects=10, fast=T > 1000)
    assert got["counts"][4] == 0 and got["hulls"][[0, 3, 6], 7].tolist() == [T - 1, T, T + 1] and got["counts"][0] == 6


def test_more_candidates_than_the_lds_tier_holds():
    T = LIMITS()[1]
    pts = K.square_sides(T // 4 + 100)
    assert len(pts) > T
    ring_lists = K.chunks(pts, 1000) + [K.cloud(500, 3, 200, 9000)] + K.chunks(K.cloud(300, 4, 200, 9000), 7)
    ring_lists += K.chunks(K.cloud(17 * 1100, 6, 200, 9000), 17) + [K.cloud(3000, 8, 200, 9000)]   # many rings of every length class
    ids = [2] * len(ring_lists)
    ring_lists.append([(1, 1), (4, 1), (2, 5)])
    ids.append(1)
    want, got = _check(_table(ring_lists, ids), max_objects=3, fast=True)
    assert got["hulls"][1, 2] == 4 and got["hulls"][1, 7] == len(pts) + 800 + 17 * 1100 + 3000 and got["rects"][1, 0] == 0


WIDEST_WORKGROUP = 1024                                      # no workgroup of the device has more threads


@pytest.mark.parametrize("case", ["lds", "hbm", "lds_2048"])
def test_more_hull_vertices_than_a_workgroup_is_wide(case):
    wave, lds = LIMITS()
    poly = K.convex_polygon(2048 if case == "lds_2048" else 1040)
    assert len(poly) > WIDEST_WORKGROUP and R.hull_fast(poly[5:] + poly[:5]) == R.hull_fast(poly) and len(R.hull_fast(poly)) == len(poly)
    cx, cy = (sum(c) // len(poly) for c in zip(*poly))
    if case == "hbm":                                        # copies of the vertices: none is strictly inside, all are candidates
        filler = poly * (lds // len(poly) + 1)
        assert len(filler) > lds
    else:                                                    # points well inside, which the prefilter may drop
        filler = K.cloud(wave + 1, 7, min(cx, cy) - 20, min(cx, cy) + 20)
    rng = np.random.default_rng(5)
    pts = [poly[k] for k in rng.permutation(len(poly))] + filler
    ring_lists, ids = K.chunks(pts, 700) + [[(0, 0), (5, 0), (5, 5), (0, 5)]], None
    ids = [2] * (len(ring_lists) - 1) + [1]
    want, got = _check(_table(ring_lists, ids), max_objects=2, fast=True)
    assert got["hulls"][1, 2] == len(poly) and got["counts"][2] == len(poly) + 4 and got["rects"][1, 0] >= 0


def test_rows_that_share_vertices_outgrow_the_staging_list():
    """Five ids name the same 200 vertices: their hulls together have 1000, the vertex list 203.  The workgroup tier keeps
    what fits and walks the rest again; the result is the same."""
    poly = K.convex_polygon(200)
    rings, vertices, counts = make_table([poly], max_rings=6, max_vertices=len(poly) + 3)
    for r in range(1, 5):
        rings[r] = rings[0]
        rings[r, 0] = r + 1
    counts[0] = counts[1] = 5
    want, got = _check((rings, vertices, counts), max_objects=6, max_hull_vertices=1007, fast=True)
    assert got["counts"].tolist() == [5, 5, 1000, 1000, 0] and got["hulls"][:5, 2].tolist() == [200] * 5
    assert all(np.array_equal(got["vertices"][:200], got["vertices"][200 * r:200 * r + 200]) for r in range(1, 5))


def test_negative_controls_see_the_tie_rule_and_the_collinear_rule():
    for name, wrong, part in (("axis_rectangle", dict(tie="largest"), "rects"), ("diamond", dict(tie="largest"), "rects"),
                              ("side_points", dict(collinear="nearest"), "hulls"), ("collinear", dict(collinear="nearest"), "vertices")):
        ring_lists, ids = HAND_MADE[name]
        rings, vertices, counts = _table(ring_lists, ids)
        rc, got = _call(rings, vertices, counts, 3, vertices.shape[0])
        bad = R.hulls(rings, vertices, counts, 3, vertices.shape[0], **wrong)
        n = int(got["counts"][3]) if part == "vertices" else 3
        assert rc == 0 and not np.array_equal(got[part][:n], bad[part][:n]), (name, wrong)


def _mixed_table():
    lists, ids = [], []
    for name in ("holed", "plus", "interleaved", "side_points", "diamond"):
        rl, ri = HAND_MADE[name]
        base = max(ids, default=0)
        lists += rl
        ids += [base + i for i in ri]
    lists.append(K.cloud(100, 5))
    ids.append(max(ids) + 1)
    return _table(lists, ids), max(ids)


def test_prefix_truncation_keeps_the_rows_and_the_rectangles():
    (rings, vertices, counts), top = _mixed_table()
    full = R.hulls(rings, vertices, counts, top + 1, vertices.shape[0])
    sizes = full["hulls"][:top, 2].tolist()
    for room in (1, sizes[0], sizes[0] + sizes[1] - 1, sum(sizes[:3]), sum(sizes) - 1, sum(sizes)):
        want, got = _check((rings, vertices, counts), top + 1, max_hull_vertices=room)
        cut = room < sum(sizes)
        assert (got["counts"][4] == R.ST_HULL_TRUNCATED) == cut and got["counts"][2] == sum(sizes) and got["counts"][3] <= room
        assert np.array_equal(got["rects"], full["rects"]) and np.array_equal(got["hulls"][:, 2:], full["hulls"][:, 2:])
        starts = got["hulls"][:top, 1].tolist()
        first = starts.index(-1) if -1 in starts else top
        assert all(s == -1 for s in starts[first:]) and starts[:first] == full["hulls"][:first, 1].tolist()


def test_pass_through_bad_rows_and_bad_counts():
    (rings, vertices, counts), top = _mixed_table()
    rings[1, 1] = -1                                         # a ring the outlines call had no room for: silently skipped
    counts[4] = R.ST_TRUNCATED
    want, got = _check((rings, vertices, counts), top + 1)
    assert got["counts"][4] == R.ST_TRUNCATED and got["hulls"][0, 7] == 4
    for change in ("n_past_the_end", "negative_n", "coordinate", "negative_coordinate", "big_coordinate_in_a_big_ring", "id_zero",
                   "id_past_the_table", "rows_past_the_table", "negative_counts"):
        (rings, vertices, counts), top = _mixed_table()
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
            row = rings.shape[0] - 3                         # the cloud of 100 points
            vertices[int(rings[row, 1]) + 77, 1] = 1 << 20
        elif change == "id_zero":
            rings[row, 0] = 0
        elif change == "id_past_the_table":
            rings[row, 0] = top + 2
        elif change == "rows_past_the_table":
            counts[1], flagged = rings.shape[0] + 100, False  # clamped: the spare rows are zero rows, id 0
            rings[-1] = (1, -1, 5, 0, 0, 0, 0, 0)
            rings[-2] = (1, -1, 5, 0, 0, 0, 0, 0)
        elif change == "negative_counts":
            counts[1], flagged = -5, False
        want, got = _check((rings, vertices, counts), top + 1)
        assert bool(got["counts"][4] & R.ST_BAD_ROW) == flagged, change
    (rings, vertices, counts), top = _mixed_table()
    counts[4] = R.ST_BAD_COUNTS | R.ST_TRUNCATED
    want, got = _check((rings, vertices, counts), top + 1)
    assert got["counts"].tolist() == [0, 0, 0, 0, R.ST_BAD_COUNTS] and not got["hulls"].any() and not got["rects"].any()


def test_refusals_enqueue_nothing():
    (rings, vertices, counts), top = _mixed_table()
    d = [torch.from_numpy(a).to(DEV) for a in (rings, vertices, counts)]
    out = [torch.zeros((top, 8), dtype=torch.int32, device=DEV), torch.zeros((50, 2), dtype=torch.int32, device=DEV),
           torch.zeros((top, 8), dtype=torch.int64, device=DEV), torch.zeros(5, dtype=torch.int32, device=DEV)]
    ws = torch.zeros(L.lib().c3d_rings_hull_ws_bytes(rings.shape[0], vertices.shape[0], top), dtype=torch.uint8, device=DEV)
    ptrs = [t.data_ptr() for t in d] + [rings.shape[0], vertices.shape[0], top, 50] + [t.data_ptr() for t in out] + [ws.data_ptr(), 0]
    before = ops.launch_count()
    for slot in (0, 1, 2, 7, 8, 9, 10, 11):
        args = list(ptrs)
        args[slot] = None
        assert L.lib().c3d_rings_hull(*args) == E_BADARG
    for slot in (3, 4, 5, 6):
        for value in (0, -1):
            args = list(ptrs)
            args[slot] = value
            assert L.lib().c3d_rings_hull(*args) == E_BADARG
    assert L.lib().c3d_rings_hull_ws_bytes(0, 1, 1) == E_BADARG and L.lib().c3d_rings_hull_ws_bytes(1, 0, 1) == E_BADARG
    assert L.lib().c3d_rings_hull_ws_bytes(1, 1, 0) == E_BADARG and L.lib().c3d_rings_hull_ws_bytes(1, 1, 1) > 0
    assert ops.launch_count() == before
    torch.cuda.synchronize()
    assert not any(t.any() for t in out)
    with pytest.raises(L.Change3DHipError):
        ops.rings_hull(*d, max_objects=0)
    with pytest.raises(L.Change3DHipError):
        ops.rings_hull(*d, max_objects=top, max_hull_vertices=0)
    with pytest.raises(L.Change3DHipError):
        ops.rings_hull(d[0].cpu(), d[1], d[2])


def test_dirty_workspace_other_stream_and_repeatability():
    T = LIMITS()[0]
    lists = [K.cloud(T + 40, 1), K.cloud(700, 2), K.square_sides(40, 900)]
    rings, vertices, counts = _table(lists + HAND_MADE["plus"][0], [1, 2, 4, 5])
    want = R.hulls(rings, vertices, counts, 6, vertices.shape[0], fast=True)
    runs = []
    for fill in (0x00, 0xFF, None):
        rc, got = _call(rings, vertices, counts, 6, vertices.shape[0], fill_ws=fill)
        assert rc == 0
        _same(got, want)
        runs.append(got)
    for other in runs[1:]:
        assert all(np.array_equal(runs[0][n], other[n]) for n in NAMES)
    assert "hull_block_kernel" in ops.last_kernel()
    d = [torch.from_numpy(a).to(DEV) for a in (rings, vertices, counts)]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        out = ops.rings_hull(*d, max_objects=6)
    side.synchronize()
    got = dict(zip(NAMES, (t.cpu().numpy() for t in out)))
    written = int(got["counts"][3])
    assert np.array_equal(got["hulls"], want["hulls"]) and np.array_equal(got["rects"], want["rects"])
    assert np.array_equal(got["counts"], want["counts"]) and np.array_equal(got["vertices"][:written], want["vertices"][:written])


def _traced(mask, connectivity, labelled=None):
    """Hulls of the device outlines of a mask: device op against restatement, then the hulls filled back on the device."""
    Hs, Ws = mask.shape
    N = Hs * Ws
    m = torch.from_numpy(mask).to(DEV)
    if labelled is None:
        labels, table, _, _, counts = ops.scene_objects(m, connectivity=connectivity, max_objects=N)
    else:
        labels, table, counts = labelled
    rings, vertices, rc = ops.scene_outlines(labels, counts, connectivity=connectivity, max_objects=N, max_rings=N, max_vertices=4 * N)
    hulls, hv, rects, hc = ops.rings_hull(rings, vertices, rc, max_objects=N)
    filled, _, _, _, _, info = ops.rings_fill(hulls, hv, hc, Hs, Ws, max_objects=N)
    covered = ((filled >= labels) | (labels <= 0)).all()    # a hull may reach over a neighbour: the largest id wins there
    exact = torch.equal(filled, labels)
    torch.cuda.synchronize()
    assert int(rc[4]) == 0 and int(hc[4]) == 0 and int(info[0]) == 0
    n = int(counts[1])
    want = R.hulls(rings.cpu().numpy(), vertices.cpu().numpy(), rc.cpu().numpy(), N, 4 * N, fast=True)
    got = dict(zip(NAMES, (t.cpu().numpy() for t in (hulls, hv, rects, hc))))
    written = int(got["counts"][3])
    assert np.array_equal(got["counts"], want["counts"]) and got["counts"][:2].tolist() == [n, n]
    assert np.array_equal(got["hulls"], want["hulls"]) and np.array_equal(got["rects"], want["rects"])
    assert np.array_equal(got["vertices"][:written], want["vertices"][:written])
    assert bool(covered), "a labelled pixel lies outside its object's hull"
    assert (got["hulls"][:n, 3] >= 2 * table[:n, 0].cpu().numpy()).all(), "a hull is smaller than its object"
    return exact, got


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("name", ["blobs", "disc", "serpentine", "scene"])
def test_hulls_of_traced_masks_cover_their_objects(name, connectivity):
    mask = {"blobs": lambda: SK.blobs(96, 96, 12, 7, seed=1).astype(np.uint8), "disc": lambda: SK.disc(96, 40),
            "serpentine": lambda: SK.serpentine(40, 40), "scene": lambda: SK.blobs(136, 200, 30, 9, seed=2).astype(np.uint8)}[name]()
    _traced(np.ascontiguousarray(mask), connectivity)


@pytest.mark.parametrize("connectivity", [4, 8])
def test_hulls_of_split_pieces(connectivity):
    mask = FK.touching_mask(75, 110)
    m = torch.from_numpy(mask).to(DEV)
    labels, table, _, _, counts, info = ops.scene_split(m, 3.0, connectivity=connectivity, max_objects=mask.size)
    assert int(info[0]) == 0
    _traced(mask, connectivity, labelled=(labels, table, counts))


def test_hulls_of_axis_rectangles_fill_back_to_the_labels():
    exact, got = _traced(K.rect_mask(), 8)
    assert exact and got["counts"][0] == 6 and (got["rects"][:6, 0] == 0).all() and (got["hulls"][:6, 2] == 4).all()
