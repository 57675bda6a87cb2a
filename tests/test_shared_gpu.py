"""`c3d_outlines_simplify_shared` against its restatement (tests/shared_reference.py): ring rows, kept vertices, left labels,
counts and info exactly equal, with canary rows on both sides of every output.  Hand-made label maps, the survey on the device
chain, combs on both sides of both tier limits in one table, a recursion deeper than a workgroup is wide, truncation,
pass-through and bad rows, a dirty workspace, a non-default stream, refusals, the twin property and the round trip through
c3d_rings_fill on the device result alone, and c3d_rings_conflicts on the shared result."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conflicts_cases as C  # noqa: E402
import shared_cases as SC  # noqa: E402
import shared_reference as R  # noqa: E402
import valid_cases as K  # noqa: E402

from change3d_amd import _lib as L  # noqa: E402
from change3d_amd import ops  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
PAD, CANARY = 3, -7777
NAMES = ("rings", "vertices", "left", "counts", "info")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(DEV)


def _call(c, table, q, max_objects=65536, max_out=None, ws=None, fill_ws=None):
    """The C entry on output buffers with canary rows on both sides: (rc, dict of numpy arrays)."""
    rings, vertices, counts = table
    max_rings, max_vertices = rings.shape[0], vertices.shape[0]
    max_out = 2 * max_vertices if max_out is None else max_out
    Hs, Ws = c["labels"].shape
    d = [_dev(a) for a in (c["labels"], c["counts_obj"], rings, vertices, counts)]
    out = [torch.full(shape, CANARY, dtype=torch.int32, device=DEV) for shape in
           ((max_rings + 2 * PAD, 8), (max_out + 2 * PAD, 2), (max_out + 2 * PAD,), (5 + 2 * PAD,), (8 + 2 * PAD,))]
    if ws is None:
        ws = torch.empty(L.lib().c3d_outlines_simplify_shared_ws_bytes(Hs, Ws, max_rings, max_vertices), dtype=torch.uint8, device=DEV)
    if fill_ws is not None:
        ws.fill_(fill_ws)
    rc = L.lib().c3d_outlines_simplify_shared(d[0].data_ptr(), d[1].data_ptr(), Hs, Ws, max_objects, d[2].data_ptr(), d[3].data_ptr(),
                                              d[4].data_ptr(), max_rings, max_vertices, q, max_out, *(o[PAD:].data_ptr() for o in out),
                                              ws.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    bufs = [o.cpu().numpy() for o in out]
    for buf in bufs:
        assert (buf[:PAD] == CANARY).all() and (buf[len(buf) - PAD:] == CANARY).all(), "a canary row was written"
    return rc, dict(zip(NAMES, (b[PAD:len(b) - PAD] for b in bufs)))


def _same(got, want):
    assert np.array_equal(got["counts"], want["counts"]), (got["counts"], want["counts"])
    assert np.array_equal(got["info"], want["info"]), (got["info"], want["info"])
    assert np.array_equal(got["rings"], want["rings"]), (np.argwhere(got["rings"] != want["rings"])[:5], got["rings"][:4], want["rings"][:4])
    written = int(got["counts"][3])
    assert np.array_equal(got["vertices"][:written], want["vertices"][:written])
    assert np.array_equal(got["left"][:written], want["left"][:written])
    assert (got["vertices"][written:] == CANARY).all() and (got["left"][written:] == CANARY).all(), "a row past counts_out[3] was written"


def _check(c, table, q, max_objects=65536, max_out=None):
    want = R.simplify_shared(c["labels"], c["counts_obj"], *table, q, max_objects=max_objects, max_vertices_out=max_out)
    rc, got = _call(c, table, q, max_objects, max_out)
    assert rc == 0
    _same(got, want)
    return want, got


HAND_MADE = SC.hand_made()


@pytest.mark.parametrize("tol", SC.TOLERANCES_HAND)
@pytest.mark.parametrize("name", sorted(HAND_MADE))
def test_hand_made_maps(name, tol):
    c = HAND_MADE[name]
    rings, vertices, counts = SC.table(c)
    n_rings, n_vertices = int(counts[1]), int(counts[3])
    table = (rings[:n_rings + 2].copy(), vertices[:n_vertices + 3].copy(), counts)
    want, got = _check(c, table, R.tol2_q(tol))
    assert int(got["counts"][4]) == 0 and R.twin_failures(got) == []
    geo, _ = R.geometry(got)
    if name == "t_junction":
        assert int(got["info"][0]) == 1 and (4, 3) in geo[3][0]
    if name == "four_at_a_point":
        assert all((3, 3) in geo[i][0] for i in (1, 2, 3, 4))
    if name == "island":
        hole = [r for r in geo[1] if R.shoelace2(r) < 0][0]
        assert hole[0] == geo[2][0][0] and hole[1:] == geo[2][0][1:][::-1] and int(got["info"][3]) == 3
    if name == "collapse" and tol == 2.0:
        assert int(got["info"][5]) >= 1
    if name == "one_node":
        assert int(got["info"][1]) == 2 and int(got["info"][2]) == 2 and int(got["info"][3]) == 2
    if name == "pinch_8":                                    # one ring through the pinch twice: two closed arcs
        assert got["info"][1:4].tolist() == [2, 2, 2] and int(got["counts"][1]) == 1
    if name == "pinch_4":
        assert int(got["counts"][1]) == 4 and all((3, 3) in ring for i in (1, 2) for ring in geo[i])


def _device_chain(seed, labelling, conn):
    mask = torch.from_numpy(K.survey_mask(seed)).to(DEV)
    n = K.SIZE * K.SIZE
    if labelling == "components":
        labels, _, _, _, counts_obj = ops.scene_objects(mask, connectivity=conn, max_objects=n)
    else:
        labels, _, _, _, counts_obj = ops.scene_split(mask, 1.0, connectivity=conn, max_objects=n)[:5]
    rings, vertices, counts = ops.scene_outlines(labels, counts_obj, conn, max_objects=n, max_rings=n, max_vertices=4 * n)
    return labels, counts_obj, rings, vertices, counts


@functools.lru_cache(maxsize=None)
def _survey(seed, labelling, conn, tol):
    """(device result, restatement on the device's own labels and table) of one survey mask, as numpy dicts."""
    n = K.SIZE * K.SIZE
    d = _device_chain(seed, labelling, conn)
    out = ops.outlines_simplify_shared(*d, tol, max_objects=n)
    got = dict(zip(("rings", "vertices", "counts", "left", "info"), (t.cpu().numpy() for t in out)))
    host = [t.cpu().numpy() for t in d]
    want = R.simplify_shared(*host, R.tol2_q(tol), max_objects=n)
    return got, want, d, out


@pytest.mark.parametrize("labelling,conn", SC.LABELLINGS)
def test_survey_on_the_device_chain(labelling, conn):
    for seed in SC.GPU_SEEDS:
        for tol in (1.0, 2.0):
            got, want, _, _ = _survey(seed, labelling, conn, tol)
            assert int(got["counts"][4]) == 0 and int(got["counts"][1]) > 0
            for name in ("counts", "info", "rings"):
                assert np.array_equal(got[name], want[name]), (seed, tol, name)
            w = int(got["counts"][3])
            assert np.array_equal(got["vertices"][:w], want["vertices"][:w]) and np.array_equal(got["left"][:w], want["left"][:w])
            assert R.twin_failures(got) == [], "the twin property, on the device result alone"


@pytest.mark.parametrize("labelling,conn", SC.LABELLINGS)
def test_tolerance_zero_fills_back_to_the_labels_on_the_device(labelling, conn):
    n = K.SIZE * K.SIZE
    for seed in SC.GPU_SEEDS:
        labels, counts_obj, rings, vertices, counts = _device_chain(seed, labelling, conn)
        r, v, c, _, info = ops.outlines_simplify_shared(labels, counts_obj, rings, vertices, counts, 0.0, max_objects=n)
        filled = ops.rings_fill(r, v, c, K.SIZE, K.SIZE, max_objects=n)
        assert int(info[5]) == 0 and int(filled[5][0]) == 0 and torch.equal(filled[0], labels)


@pytest.mark.parametrize("conn", [4, 8])
def test_conflicts_of_the_shared_result(conn):
    n = K.SIZE * K.SIZE
    for seed in SC.GPU_SEEDS:
        got, want, _, out = _survey(seed, "split", conn, 1.0)
        rows, _ = C.fast_counts(R.geometry(want)[0])
        conflict, counts, _ = ops.rings_conflicts(out[0], out[1], out[2], 0, max_objects=n)
        conflict = conflict.cpu().numpy()
        assert int(counts[7]) == 0
        for i, v in rows.items():
            assert conflict[i - 1, 3:8].tolist() == list(v), (seed, i)
        assert int(counts[1]) == len(C.in_conflict(rows))


LIMITS = functools.lru_cache(maxsize=None)(lambda: ops.outlines_simplify_shared_limits())


@pytest.mark.parametrize("tol", [0.5, 1.5])
def test_combs_on_both_sides_of_both_tier_limits(tol):
    wave, lds = LIMITS()
    assert 16 <= wave < lds <= 1 << 20
    sizes = [wave - 1, wave, wave + 1, lds - 1, lds, lds + 1]
    c = SC.comb_labels(sizes)
    table = SC.table(c)
    lab = R.Labels(c["labels"], c["counts_obj"], 65536)
    rings, vertices, counts = table
    augmented = {int(r[0]): len(R.augment([tuple(p) for p in vertices[r[1]:r[1] + r[2]].tolist()], lab)) for r in rings[:int(counts[1])]}
    assert [augmented[j + 1] for j in range(len(sizes))] == sizes
    table = (rings[:int(counts[1]) + 1].copy(), vertices[:int(counts[3]) + 2].copy(), counts)
    want, got = _check(c, table, R.tol2_q(tol))
    assert int(got["counts"][4]) == 0 and int(got["info"][1]) > 0 and R.twin_failures(got) == []
    kept = {int(r[0]): int(r[2]) for r in got["rings"][:int(counts[1])]}
    assert all(sizes[j] // 2 < kept[j + 1] <= sizes[j] if tol < 1 else 3 <= kept[j + 1] < 16 for j in range(len(sizes)))
    assert tol > 1 or want["depth"] > 1024, "the teeth of one pixel stand out at half a pixel and fall at one and a half"


def test_recursion_deeper_than_a_workgroup_is_wide():
    """The tips of a comb tie; the smallest (vy, vx) is the leftmost, so every split cuts one vertex off the chord."""
    c = SC.comb_labels([4 * 600 + 1])
    want, got = _check(c, SC.table(c), R.tol2_q(0.5))
    assert LIMITS()[0] < 2401 <= LIMITS()[1] and want["depth"] > 1024 and int(got["counts"][4]) == 0


def test_truncation_is_prefix_shaped():
    c = HAND_MADE["four_at_a_point"]
    table = SC.table(c)
    full, _ = _check(c, table, 16)
    need = int(full["counts"][3])
    for room in (need - 1, need - 5, 1):
        want, got = _check(c, table, 16, max_out=room)
        assert int(got["counts"][2]) == need and int(got["counts"][3]) < need and int(got["counts"][4]) == R.ST_TRUNCATED
        cut = [int(r[1]) < 0 for r in got["rings"][:int(got["counts"][1])]]
        assert cut[-1] and cut == sorted(cut)
    _check(c, table, 16, max_out=need)


def test_pass_through_and_bad_rows():
    c = HAND_MADE["neck"]
    base = SC.table(c)
    for change in ("pass", "diagonal", "zero_edge", "outside", "negative", "n_small", "n_past_the_end", "bad_counts", "rows"):
        rings, vertices, counts = (a.copy() for a in base)
        row, status = 1, R.ST_BAD_INPUT
        at = int(rings[row, 1])
        if change == "pass":
            rings[row, 1], counts[4], status = -1, R.ST_TRUNCATED, R.ST_TRUNCATED
        elif change == "diagonal":
            vertices[at + 1] += (1, 1)
        elif change == "zero_edge":
            vertices[at + 1] = vertices[at]
        elif change == "outside":
            vertices[at:at + int(rings[row, 2]), 0] += 9     # past Ws
        elif change == "negative":
            vertices[at, 0] = -1
        elif change == "n_small":
            rings[row, 2] = 3
        elif change == "n_past_the_end":
            rings[row, 2] = int(counts[3]) - at + 1
        elif change == "bad_counts":
            counts[4], status = R.ST_BAD_COUNTS | R.ST_TRUNCATED, R.ST_BAD_COUNTS
        else:
            counts[1], status = 2, 0
        want, got = _check(c, (rings, vertices, counts), 16)
        assert int(got["counts"][4]) == status, change
        if change == "bad_counts":
            assert not got["rings"].any() and not got["info"].any() and (got["vertices"] == CANARY).all()
        elif change == "rows":
            assert not got["rings"][2:].any()
        else:
            assert got["rings"][row, 1:4].tolist() == [-1, 0, 0] and got["rings"][0, 1] == 0 and got["rings"][2, 1] > 0, change


def test_augmented_rings_without_room_are_bad_input():
    """One row names the whole vertex list as a single ring again and again: the augmented rings outgrow 2 max_vertices."""
    c = HAND_MADE["t_junction"]
    rings, vertices, counts = SC.table(c)
    n = int(rings[0, 2])
    rings, vertices = rings[:8].copy(), vertices[:n + 1].copy()
    rings[:8] = rings[0]
    counts = np.array([8, 8, n, n, 0], dtype=np.int32)
    want, got = _check(c, (rings, vertices, counts), 16)
    assert int(got["counts"][4]) == R.ST_BAD_INPUT and got["rings"][0, 1] == 0 and got["rings"][7, 1] == -1


def test_two_calls_agree_bit_for_bit_also_on_a_dirty_workspace():
    wave, lds = LIMITS()
    c = SC.comb_labels([40, wave + 3, 500, lds + 9])
    table = SC.table(c)
    ws = torch.empty(L.lib().c3d_outlines_simplify_shared_ws_bytes(*c["labels"].shape, len(table[0]), len(table[1])), dtype=torch.uint8,
                     device=DEV)
    first = _call(c, table, R.tol2_q(1.5), ws=ws, fill_ws=0)
    again = _call(c, table, R.tol2_q(1.5), ws=ws)
    dirty = _call(c, table, R.tol2_q(1.5), ws=ws, fill_ws=0xFF)
    other = _call(c, table, R.tol2_q(0.5), ws=ws)
    back = _call(c, table, R.tol2_q(1.5), ws=ws)
    assert first[0] == 0 and int(first[1]["counts"][4]) == 0 and other[0] == 0 and other[1]["counts"][2] > first[1]["counts"][2]
    for run in (again, dirty, back):
        assert run[0] == 0 and all(np.array_equal(run[1][n], first[1][n]) for n in NAMES)


def test_non_default_stream_and_the_python_op():
    c = HAND_MADE["neck"]
    table = SC.table(c)
    want = R.simplify_shared(c["labels"], c["counts_obj"], *table, R.tol2_q(1.5))
    d = [_dev(a) for a in (c["labels"], c["counts_obj"], *table)]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    before = ops.launch_count()
    with torch.cuda.stream(side):
        r, v, cnt, left, info = ops.outlines_simplify_shared(*d, 1.5)
    side.synchronize()
    assert ops.launch_count() - before == 10, "the header documents 10 launches"
    assert r.shape == d[2].shape and v.shape == (2 * len(d[3]), 2) and left.shape == (2 * len(d[3]),) and info.shape == (8,)
    w = int(cnt[3])
    got = dict(rings=r.cpu().numpy(), vertices=v.cpu().numpy(), left=left.cpu().numpy(), counts=cnt.cpu().numpy(), info=info.cpu().numpy())
    for name in ("rings", "counts", "info"):
        assert np.array_equal(got[name], want[name])
    assert np.array_equal(got["vertices"][:w], want["vertices"][:w]) and np.array_equal(got["left"][:w], want["left"][:w])
    with pytest.raises(ValueError):
        ops.outlines_simplify_shared(*d, 1025.0)
    with pytest.raises(L.Change3DHipError):
        ops.outlines_simplify_shared(d[0].cpu(), *d[1:], 1.0)
    with pytest.raises(L.Change3DHipError):
        ops.outlines_simplify_shared(*d, 1.0, max_vertices_out=0)


def test_refusals_leave_the_outputs_untouched():
    c = HAND_MADE["neck"]
    table = SC.table(c)
    d = [_dev(a) for a in (c["labels"], c["counts_obj"], *table)]
    Hs, Ws = c["labels"].shape
    max_rings, max_vertices = len(table[0]), len(table[1])
    ws = torch.empty(L.lib().c3d_outlines_simplify_shared_ws_bytes(Hs, Ws, max_rings, max_vertices), dtype=torch.uint8, device=DEV)
    outs = [torch.full(s, CANARY, dtype=torch.int32, device=DEV) for s in ((max_rings, 8), (2 * max_vertices, 2), (2 * max_vertices,), (5,), (8,))]
    good = dict(labels=d[0].data_ptr(), counts_obj=d[1].data_ptr(), Hs=Hs, Ws=Ws, max_objects=64, rings=d[2].data_ptr(),
                vertices=d[3].data_ptr(), counts=d[4].data_ptr(), max_rings=max_rings, max_vertices=max_vertices, tol2_q=16,
                max_out=2 * max_vertices, rings_out=outs[0].data_ptr(), vertices_out=outs[1].data_ptr(), left_out=outs[2].data_ptr(),
                counts_out=outs[3].data_ptr(), info=outs[4].data_ptr(), ws=ws.data_ptr())
    bad = [{k: None} for k in ("labels", "counts_obj", "rings", "vertices", "counts", "rings_out", "vertices_out", "left_out", "counts_out",
                               "info", "ws")]
    bad += [dict(Hs=0), dict(Ws=-1), dict(max_objects=0), dict(max_rings=0), dict(max_vertices=0), dict(max_out=0), dict(tol2_q=-1),
            dict(tol2_q=R.TOL2_Q_MAX + 1)]
    before = ops.launch_count()
    for change in bad:
        rc = L.lib().c3d_outlines_simplify_shared(*{**good, **change}.values(), torch.cuda.current_stream().cuda_stream)
        assert rc == -1, (change, rc)                       # C3D_E_BADARG
    rc = L.lib().c3d_outlines_simplify_shared(*{**good, "Ws": 16385}.values(), torch.cuda.current_stream().cuda_stream)
    assert rc not in (0, -1)                                # C3D_E_UNSUPPORTED
    ws_bytes = L.lib().c3d_outlines_simplify_shared_ws_bytes
    assert ws_bytes(8, 8, 0, 5) == -1 and ws_bytes(8, 8, 5, 0) == -1 and ws_bytes(0, 8, 5, 5) == -1 and ws_bytes(8, 16385, 5, 5) not in (0, -1)
    assert ws_bytes(8, 8, 5, 5) > 0
    assert ops.launch_count() == before
    torch.cuda.synchronize()
    assert all((o == CANARY).all() for o in outs)


def test_negative_controls_differ_from_the_device():
    for name, tol, variant in (("stairs", 0.5, dict(tie="index")), ("t_junction", 0.0, dict(insert_nodes=False))):
        c = HAND_MADE[name]
        table = SC.table(c)
        rc, got = _call(c, table, R.tol2_q(tol))
        wrong = R.simplify_shared(c["labels"], c["counts_obj"], *table, R.tol2_q(tol), **variant)
        w = int(got["counts"][3])
        assert rc == 0 and not (np.array_equal(got["counts"], wrong["counts"]) and np.array_equal(got["rings"], wrong["rings"])
                                and np.array_equal(got["vertices"][:w], wrong["vertices"][:w])), name
