"""`c3d_outlines_simplify_safe` against its restatement (tests/safe_reference.py) through the C entry, with canary rows on both
sides of every output: ring rows, kept vertices, left labels, levels, counts, info and safe exactly equal.  Hand-made label maps,
the survey, a scene of five raising rounds cut short, combs on both sides of the Douglas-Peucker's tier limits, crowded cells on
both sides of the detector's, the work cap, a ring that collapses in round 0, tolerance 0, the shared call where round 0 is
clean, c3d_rings_valid and c3d_rings_conflicts on converged outputs, truncation, bad counts, refusals, a dirty workspace, a
second stream, and two negative controls."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import safe_cases as SA  # noqa: E402
import safe_reference as S  # noqa: E402
import shared_cases as SC  # noqa: E402
import shared_reference as R  # noqa: E402

from change3d_amd import _lib as L  # noqa: E402
from change3d_amd import ops  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
PAD, CANARY = 3, -7777
NAMES = ("rings", "vertices", "left", "level", "counts", "info", "safe")
LIMITS = functools.lru_cache(maxsize=None)(lambda: ops.outlines_simplify_safe_limits())


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(DEV)


def _call(c, table, q, max_rounds=8, max_work=2 ** 32, max_objects=65536, max_out=None, ws=None, fill_ws=None):
    """The C entry on output buffers with canary rows on both sides: (rc, dict of numpy arrays)."""
    rings, vertices, counts = table
    max_rings, max_vertices = rings.shape[0], vertices.shape[0]
    max_out = 2 * max_vertices if max_out is None else max_out
    Hs, Ws = c["labels"].shape
    d = [_dev(a) for a in (c["labels"], c["counts_obj"], rings, vertices, counts)]
    shapes = ((max_rings + 2 * PAD, 8), (max_out + 2 * PAD, 2), (max_out + 2 * PAD,), (max_out + 2 * PAD,), (5 + 2 * PAD,), (8 + 2 * PAD,))
    out = [torch.full(shape, CANARY, dtype=torch.int32, device=DEV) for shape in shapes]
    out.append(torch.full((8 + 2 * PAD,), CANARY, dtype=torch.int64, device=DEV))
    if ws is None:
        ws = torch.empty(L.lib().c3d_outlines_simplify_safe_ws_bytes(Hs, Ws, max_rings, max_vertices, max_out), dtype=torch.uint8, device=DEV)
    if fill_ws is not None:
        ws.fill_(fill_ws)
    rc = L.lib().c3d_outlines_simplify_safe(d[0].data_ptr(), d[1].data_ptr(), Hs, Ws, max_objects, d[2].data_ptr(), d[3].data_ptr(),
                                            d[4].data_ptr(), max_rings, max_vertices, q, max_rounds, max_work, max_out,
                                            *(o[PAD:].data_ptr() for o in out), ws.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    bufs = [o.cpu().numpy() for o in out]
    for buf in bufs:
        assert (buf[:PAD] == CANARY).all() and (buf[len(buf) - PAD:] == CANARY).all(), "a canary row was written"
    return rc, dict(zip(NAMES, (b[PAD:len(b) - PAD] for b in bufs)))


def _same(got, want, tail=True):
    assert np.array_equal(got["safe"], want["safe"]), (got["safe"], want["safe"])
    assert np.array_equal(got["counts"], want["counts"]), (got["counts"], want["counts"])
    assert np.array_equal(got["info"], want["info"]), (got["info"], want["info"])
    assert np.array_equal(got["rings"], want["rings"]), (np.argwhere(got["rings"] != want["rings"])[:5], got["rings"][:4], want["rings"][:4])
    written = int(got["counts"][3])
    for name in ("vertices", "left", "level"):
        assert np.array_equal(got[name][:written], want[name][:written]), name
        assert not tail or (got[name][written:] == CANARY).all(), "a row past counts_out[3] was written"


def _check(c, table, q, fast=True, tail=True, **kw):
    ref = {k: v for k, v in kw.items() if k in ("max_rounds", "max_work", "max_objects")}
    want = S.simplify_safe(c["labels"], c["counts_obj"], *table, q, limits=LIMITS()[4:6], max_vertices_out=kw.get("max_out"), fast=fast,
                           history=kw.pop("history", None), **ref)
    rc, got = _call(c, table, q, **kw)
    assert rc == 0
    _same(got, want, tail)
    return want, got


def _tight(c):
    rings, vertices, counts = SC.table(c)
    return rings[:int(counts[1]) + 2].copy(), vertices[:int(counts[3]) + 3].copy(), counts


def _shared(c, table, q):
    d = [_dev(a) for a in (c["labels"], c["counts_obj"], *table)]
    r, v, cnt, left, info = ops.outlines_simplify_shared(*d, 0.0 if q == 0 else (q / 16) ** 0.5)
    return dict(rings=r.cpu().numpy(), vertices=v.cpu().numpy(), left=left.cpu().numpy(), counts=cnt.cpu().numpy(), info=info.cpu().numpy())


def _downstream_is_clean(got, max_objects):
    """c3d_rings_valid and c3d_rings_conflicts on a converged output."""
    table = [_dev(got[n]) for n in ("rings", "vertices", "counts")]
    valid, v_counts = ops.rings_valid(*table, 0, max_objects=max_objects)
    conflict, c_counts, _ = ops.rings_conflicts(*table, 0, max_objects=max_objects)
    valid, conflict = valid.cpu().numpy(), conflict.cpu().numpy()
    checked = valid[:, 0] == 0
    assert int(v_counts[0]) > 0 and int(v_counts[4]) == 0 and not valid[checked][:, [4, 5, 7]].any()
    assert int(c_counts[4]) == 0 and not conflict[:, [3, 4, 7]].any()


HAND_MADE = SA.HAND_MADE()


@pytest.mark.parametrize("tol", SA.TOLERANCES_HAND)
@pytest.mark.parametrize("name", sorted(HAND_MADE))
def test_hand_made_maps(name, tol):
    c = HAND_MADE[name]
    table = _tight(c)
    q = R.tol2_q(tol)
    want, got = _check(c, table, q, fast=False)
    assert int(got["safe"][7]) == S.ST_CONVERGED and int(got["counts"][4]) == 0 and int(got["info"][5]) == 0
    assert R.twin_failures(got) == []
    clean = int(got["safe"][4]) == 0 and int(got["safe"][6]) == 0
    if tol == 0.0:
        assert clean and got["safe"].tolist()[:3] == [1, 0, 0]
    if clean:                                                # round 0 marks nothing: the shared call on the device
        shared = _shared(c, table, q)
        w = int(got["counts"][3])
        assert np.array_equal(got["rings"], shared["rings"]) and np.array_equal(got["counts"], shared["counts"])
        assert np.array_equal(got["vertices"][:w], shared["vertices"][:w]) and np.array_equal(got["left"][:w], shared["left"][:w])
        assert np.array_equal(got["info"][:6], shared["info"][:6])
    if name == "collapse" and tol == 2.0:                    # object 2 falls under one chord in round 0 and is whole at the end
        assert int(got["safe"][6]) >= 1 and int(got["safe"][1]) >= 1 and all(int(r[2]) >= 3 for r in got["rings"][:int(got["counts"][1])])
    _downstream_is_clean(got, 16)


@pytest.mark.parametrize("labelling,conn", SA.LABELLINGS)
def test_survey(labelling, conn):
    raised = 0
    for seed in SA.GPU_SEEDS:
        c, table, _ = SA.survey_prep(seed, labelling, conn)
        for tol in (1.0, 2.0):
            want, got = _check(c, table, R.tol2_q(tol), max_objects=SA.MAX_OBJECTS)
            assert int(got["safe"][7]) == S.ST_CONVERGED and int(got["safe"][5]) == 0 and int(got["info"][5]) == 0
            assert R.twin_failures(got) == [], "the twin property, on the device result alone"
            raised += int(got["safe"][1])
            if tol == 2.0 and seed % 4 == 0:
                _downstream_is_clean(got, SA.MAX_OBJECTS)
    assert raised > len(SA.GPU_SEEDS)


def test_five_raising_rounds_and_the_rounds_cut_short():
    c, table, _ = SA.survey_prep(*SA.DEEP_SCENE)
    q = R.tol2_q(2.0)
    history = []
    want, got = _check(c, table, q, max_objects=SA.MAX_OBJECTS, history=history)
    assert got["safe"].tolist()[:2] == [6, 5] and int(got["safe"][7]) == S.ST_CONVERGED
    _downstream_is_clean(got, SA.MAX_OBJECTS)
    for rounds in (1, 2):
        want, got = _check(c, table, q, max_objects=SA.MAX_OBJECTS, max_rounds=rounds)
        assert got["safe"].tolist()[:2] == [rounds, rounds] and int(got["safe"][7]) == S.ST_NOT_CONVERGED
        step = history[rounds - 1][0]                        # the exact intermediate output: that round's simplify step
        w = int(step["counts"][3])
        assert np.array_equal(got["rings"], step["rings"]) and np.array_equal(got["vertices"][:w], step["vertices"][:w])
        assert R.twin_failures(got) == []
    _check(c, table, q, max_objects=SA.MAX_OBJECTS, max_rounds=6)
    want, got = _check(c, table, q, max_objects=SA.MAX_OBJECTS, max_rounds=64)
    assert got["safe"].tolist()[:2] == [6, 5]


@pytest.mark.parametrize("tol", [1.5, 2.0])
def test_combs_on_both_sides_of_both_tier_limits(tol):
    wave, lds = LIMITS()[:2]
    assert 16 <= wave < lds <= 1 << 20
    sizes = [wave - 1, wave, wave + 1, lds - 1, lds, lds + 1]
    c = SC.comb_labels(sizes)
    table = _tight(c)
    lab = R.Labels(c["labels"], c["counts_obj"], 65536)
    rings, vertices, counts = table
    augmented = {int(r[0]): len(R.augment([tuple(p) for p in vertices[r[1]:r[1] + r[2]].tolist()], lab)) for r in rings[:int(counts[1])]}
    assert [augmented[j + 1] for j in range(len(sizes))] == sizes
    want, got = _check(c, table, R.tol2_q(tol))
    assert int(got["counts"][4]) == 0 and int(got["safe"][7]) == S.ST_CONVERGED and R.twin_failures(got) == []
    # the one-pixel neighbours collapse in round 0: the wall each shares with its comb is raised, so every tier reads a level
    top = {int(r[0]): int(got["level"][r[1]:r[1] + r[2]].max()) for r in got["rings"][:int(counts[1])]}
    assert int(got["safe"][6]) > 0 and all(top[j + 1] >= 1 for j in range(len(sizes)))


@pytest.mark.parametrize("t", [8, 30, 100, 128])
def test_crowded_cells_on_both_sides_of_the_wave_tier_and_at_two_chunks(t):
    cell_wave, chunk = LIMITS()[2:4]
    c = SA.nested_ls(t, patch=3)
    history = []
    want, got = _check(c, _tight(c), R.tol2_q(2.0), history=history)
    most = [step["most"] for step, _, _, _ in history]
    assert {8: max(most) <= cell_wave, 30: cell_wave < min(most) and max(most) <= chunk, 100: chunk < min(most) <= max(most) < 2 * chunk,
            128: min(most) == max(most) == 2 * chunk}[t], most
    assert int(got["safe"][4]) > 0 and int(got["safe"][1]) >= 3 and int(got["safe"][7]) == S.ST_CONVERGED
    _downstream_is_clean(got, int(c["counts_obj"][1]) + 1)


def test_work_cap_at_and_below_work():
    c = SA.nested_ls(30, patch=3)
    table = _tight(c)
    q = R.tol2_q(2.0)
    history = []
    full, _ = _check(c, table, q, history=history)
    work = [step["work"] for step, _, _, _ in history]
    assert work[0] < max(work) and int(full["info"][7]) == work[-1]
    want, got = _check(c, table, q, max_work=max(work))
    assert int(got["safe"][7]) == S.ST_CONVERGED
    want, got = _check(c, table, q, max_work=work[0] - 1)     # over in round 0: nothing is evaluated, the output is round 0's
    assert got["safe"].tolist() == [1, 0, 0, 0, 0, 0, int(full["safe"][6]), S.ST_OVER_WORK]
    want, got = _check(c, table, q, max_work=work[0])         # at the work of round 0, below that of a later round
    late = next(k for k, v in enumerate(work) if v > work[0])
    assert got["safe"].tolist()[:2] == [late + 1, late] and int(got["safe"][7]) == S.ST_OVER_WORK
    step = history[late][0]
    assert np.array_equal(got["rings"], step["rings"])
    want, got = _check(HAND_MADE["neck"], _tight(HAND_MADE["neck"]), 0, max_work=0)
    assert int(got["safe"][7]) == S.ST_OVER_WORK


def test_truncation_is_prefix_shaped():
    c = HAND_MADE["neck"]
    table = _tight(c)
    q = R.tol2_q(2.0)
    full, _ = _check(c, table, q, fast=False)
    need = int(full["counts"][3])
    assert int(full["safe"][1]) >= 1
    for room in (need - 1, need - 5, 1):                     # a later round keeps more and so writes less: the rows between are an
        want, got = _check(c, table, q, fast=False, tail=False, max_out=room)   # earlier round's, the canaries past max_out stand
        assert int(got["counts"][3]) < int(got["counts"][2]) and int(got["counts"][4]) & R.ST_TRUNCATED
        cut = [int(r[1]) < 0 for r in got["rings"][:int(got["counts"][1])]]
        assert cut[-1] and cut == sorted(cut)
    _check(c, table, q, fast=False, max_out=need)


def test_bad_counts_and_bad_rows():
    c = HAND_MADE["neck"]
    base = _tight(c)
    for change in ("bad_counts", "pass", "diagonal", "rows"):
        rings, vertices, counts = (a.copy() for a in base)
        at = int(rings[1, 1])
        if change == "bad_counts":
            counts[4] = R.ST_BAD_COUNTS | R.ST_TRUNCATED
        elif change == "pass":
            rings[1, 1], counts[4] = -1, R.ST_TRUNCATED
        elif change == "diagonal":
            vertices[at + 1] += (1, 1)
        else:
            counts[1] = 2
        want, got = _check(c, (rings, vertices, counts), R.tol2_q(2.0), fast=False)
        if change == "bad_counts":
            assert got["counts"].tolist() == [0, 0, 0, 0, R.ST_BAD_COUNTS] and got["safe"].tolist() == [1, 0, 0, 0, 0, 0, 0, 0]
            assert not got["rings"].any() and not got["info"].any() and (got["vertices"] == CANARY).all()
        elif change == "diagonal":
            assert int(got["counts"][4]) == R.ST_BAD_INPUT and got["rings"][1, 1:4].tolist() == [-1, 0, 0]


def test_refusals_leave_the_outputs_untouched():
    c = HAND_MADE["neck"]
    table = _tight(c)
    d = [_dev(a) for a in (c["labels"], c["counts_obj"], *table)]
    Hs, Ws = c["labels"].shape
    max_rings, max_vertices = len(table[0]), len(table[1])
    ws_bytes = L.lib().c3d_outlines_simplify_safe_ws_bytes
    ws = torch.empty(ws_bytes(Hs, Ws, max_rings, max_vertices, 2 * max_vertices), dtype=torch.uint8, device=DEV)
    outs = [torch.full(s, CANARY, dtype=torch.int32, device=DEV) for s in ((max_rings, 8), (2 * max_vertices, 2), (2 * max_vertices,),
                                                                           (2 * max_vertices,), (5,), (8,))]
    outs.append(torch.full((8,), CANARY, dtype=torch.int64, device=DEV))
    good = dict(labels=d[0].data_ptr(), counts_obj=d[1].data_ptr(), Hs=Hs, Ws=Ws, max_objects=64, rings=d[2].data_ptr(),
                vertices=d[3].data_ptr(), counts=d[4].data_ptr(), max_rings=max_rings, max_vertices=max_vertices, tol2_q=16, max_rounds=8,
                max_work=2 ** 32, max_out=2 * max_vertices, rings_out=outs[0].data_ptr(), vertices_out=outs[1].data_ptr(),
                left_out=outs[2].data_ptr(), level_out=outs[3].data_ptr(), counts_out=outs[4].data_ptr(), info=outs[5].data_ptr(),
                safe=outs[6].data_ptr(), ws=ws.data_ptr())
    bad = [{k: None} for k in ("labels", "counts_obj", "rings", "vertices", "counts", "rings_out", "vertices_out", "left_out", "level_out",
                               "counts_out", "info", "safe", "ws")]
    bad += [dict(Hs=0), dict(Ws=-1), dict(max_objects=0), dict(max_rings=0), dict(max_vertices=0), dict(max_out=0), dict(max_out=2 ** 29 + 1),
            dict(tol2_q=-1), dict(tol2_q=R.TOL2_Q_MAX + 1), dict(max_rounds=0), dict(max_rounds=65), dict(max_work=-1)]
    before = ops.launch_count()
    for change in bad:
        rc = L.lib().c3d_outlines_simplify_safe(*{**good, **change}.values(), torch.cuda.current_stream().cuda_stream)
        assert rc == -1, (change, rc)                       # C3D_E_BADARG
    rc = L.lib().c3d_outlines_simplify_safe(*{**good, "Ws": 16385}.values(), torch.cuda.current_stream().cuda_stream)
    assert rc not in (0, -1)                                # C3D_E_UNSUPPORTED
    assert ws_bytes(8, 8, 0, 5, 5) == -1 and ws_bytes(8, 8, 5, 0, 5) == -1 and ws_bytes(0, 8, 5, 5, 5) == -1 and ws_bytes(8, 8, 5, 5, 0) == -1
    assert ws_bytes(8, 16385, 5, 5, 5) not in (0, -1) and ws_bytes(8, 8, 5, 5, 5) > 0
    assert ops.launch_count() == before
    torch.cuda.synchronize()
    assert all((o == CANARY).all() for o in outs)
    with pytest.raises(ValueError):
        ops.outlines_simplify_safe(*d, 1.0, max_rounds=0)
    with pytest.raises(ValueError):
        ops.outlines_simplify_safe(*d, 1025.0)
    with pytest.raises(L.Change3DHipError):
        ops.outlines_simplify_safe(d[0].cpu(), *d[1:], 1.0)
    with pytest.raises(L.Change3DHipError):
        ops.outlines_simplify_safe(*d, 1.0, max_vertices_out=0)


def test_two_calls_agree_bit_for_bit_also_on_a_dirty_workspace():
    c, table, _ = SA.survey_prep(*SA.DEEP_SCENE)
    q = R.tol2_q(2.0)
    ws = torch.empty(L.lib().c3d_outlines_simplify_safe_ws_bytes(*c["labels"].shape, len(table[0]), len(table[1]), 2 * len(table[1])),
                     dtype=torch.uint8, device=DEV)
    first = _call(c, table, q, max_objects=SA.MAX_OBJECTS, ws=ws, fill_ws=0)
    again = _call(c, table, q, max_objects=SA.MAX_OBJECTS, ws=ws)
    dirty = _call(c, table, q, max_objects=SA.MAX_OBJECTS, ws=ws, fill_ws=0xFF)
    other = _call(c, table, R.tol2_q(1.0), max_objects=SA.MAX_OBJECTS, ws=ws)
    back = _call(c, table, q, max_objects=SA.MAX_OBJECTS, ws=ws)
    assert first[0] == 0 and int(first[1]["safe"][1]) == 5 and other[0] == 0 and other[1]["counts"][2] != first[1]["counts"][2]
    for run in (again, dirty, back):
        assert run[0] == 0 and all(np.array_equal(run[1][n], first[1][n]) for n in NAMES)


def test_non_default_stream_and_the_python_op():
    c = HAND_MADE["neck"]
    table = SC.table(c)
    want = S.simplify_safe(c["labels"], c["counts_obj"], *table, R.tol2_q(2.0), limits=LIMITS()[4:6])
    d = [_dev(a) for a in (c["labels"], c["counts_obj"], *table)]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    before = ops.launch_count()
    with torch.cuda.stream(side):
        r, v, cnt, left, info, level, safe = ops.outlines_simplify_safe(*d, 2.0, max_rounds=5)
    side.synchronize()
    assert ops.launch_count() - before == 7 + 16 * 5, "the header documents 7 + 16 max_rounds launches"
    assert r.shape == d[2].shape and v.shape == (2 * len(d[3]), 2) and left.shape == level.shape == (2 * len(d[3]),)
    assert info.shape == (8,) and safe.shape == (8,) and safe.dtype == torch.int64
    w = int(cnt[3])
    got = dict(rings=r, vertices=v, left=left, level=level, counts=cnt, info=info, safe=safe)
    got = {k: t.cpu().numpy() for k, t in got.items()}
    for name in ("rings", "counts", "info", "safe"):
        assert np.array_equal(got[name], want[name]), name
    for name in ("vertices", "left", "level"):
        assert np.array_equal(got[name][:w], want[name][:w]), name
    assert int(safe[1]) >= 1


def test_negative_controls_differ_from_the_device():
    """Without the touch_ve clause a vertex of one chord inside another goes unseen: on survey mask 2 (4-connected components,
    1 px) that restatement ends with other vertices than the device and with a pair that the rule calls defective.  Levels
    kept per ring end with the same geometry wherever it was tried -- every defective pair that marks an arc marks its twin too,
    the twin's edge being the same segment -- so that control shows in what is counted once per key: `neck` at 2 px raises a
    shared wall, which per ring is two arcs above level 0 and by key one."""
    c, table, _ = SA.survey_prep(2, "components", 4)
    q = R.tol2_q(1.0)
    rc, got = _call(c, table, q, max_objects=SA.MAX_OBJECTS)
    wrong = S.simplify_safe(c["labels"], c["counts_obj"], *table, q, limits=LIMITS()[4:6], max_objects=SA.MAX_OBJECTS, touch_ve=False)
    w = int(got["counts"][3])
    assert rc == 0 and int(got["safe"][7]) == S.ST_CONVERGED and int(wrong["safe"][7]) == S.ST_CONVERGED
    assert not (np.array_equal(got["rings"], wrong["rings"]) and np.array_equal(got["vertices"][:w], wrong["vertices"][:w]))
    assert S.detect(S.edges_of(wrong))[1] >= 1, "what the wrong rule leaves is a defect by the right one"
    c = HAND_MADE["neck"]
    table = _tight(c)
    q = R.tol2_q(2.0)
    rc, got = _call(c, table, q)
    wrong = S.simplify_safe(c["labels"], c["counts_obj"], *table, q, limits=LIMITS()[4:6], per_ring=True)
    assert rc == 0 and int(got["safe"][2]) >= 1 and int(wrong["safe"][2]) > int(got["safe"][2])
