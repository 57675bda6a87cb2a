"""`c3d_outlines_simplify` against its restatement (tests/simplify_reference.py): ring rows, kept vertices and counts exactly
equal, on tables built by hand -- no tracing.  Hand-made shapes at five tolerances, rings on both sides of every tier limit
in one table, recursion deeper than a workgroup is wide, pass-through and bad rows, canaries, refusals, determinism on a
dirty workspace, a non-default stream, two negative controls, and `predict(simplify=)` / `predict_scene --simplify` end to
end."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import simplify_cases as K  # noqa: E402
import simplify_reference as S  # noqa: E402

from change3d_amd import _lib as L  # noqa: E402
from change3d_amd import ops  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAD, CANARY = 3, -7777


def _call(rings, vertices, counts, q, ws=None, fill_ws=None):
    """The C entry on output buffers with canary rows on both sides: (rc, rings_out, vertices_out, counts_out) as numpy."""
    max_rings, max_vertices = rings.shape[0], vertices.shape[0]
    d_in = [torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(DEV) for a in (rings, vertices, counts)]
    r_out = torch.full((max_rings + 2 * PAD, 8), CANARY, dtype=torch.int32, device=DEV)
    v_out = torch.full((max_vertices + 2 * PAD, 2), CANARY, dtype=torch.int32, device=DEV)
    c_out = torch.full((5 + 2 * PAD,), CANARY, dtype=torch.int32, device=DEV)
    if ws is None:
        ws = torch.empty(L.lib().c3d_outlines_simplify_ws_bytes(max_rings, max_vertices), dtype=torch.uint8, device=DEV)
    if fill_ws is not None:
        ws.fill_(fill_ws)
    rc = L.lib().c3d_outlines_simplify(d_in[0].data_ptr(), d_in[1].data_ptr(), d_in[2].data_ptr(), max_rings, max_vertices, q,
                                       r_out[PAD:].data_ptr(), v_out[PAD:].data_ptr(), c_out[PAD:].data_ptr(), ws.data_ptr(),
                                       torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    r_out, v_out, c_out = r_out.cpu().numpy(), v_out.cpu().numpy(), c_out.cpu().numpy()
    for buf in (r_out, v_out, c_out):
        assert (buf[:PAD] == CANARY).all() and (buf[len(buf) - PAD:] == CANARY).all(), "a canary row was written"
    return rc, r_out[PAD:len(r_out) - PAD], v_out[PAD:len(v_out) - PAD], c_out[PAD:PAD + 5]


def _check(rings, vertices, counts, q, want=None):
    """Device against restatement: exact.  Returns (restatement, device rings, vertices, counts)."""
    want = S.simplify(rings, vertices, counts, q) if want is None else want
    rc, r_out, v_out, c_out = _call(rings, vertices, counts, q)
    assert rc == 0
    assert np.array_equal(c_out, want["counts"]), (c_out, want["counts"])
    assert np.array_equal(r_out, want["rings"]), (np.argwhere(r_out != want["rings"])[:5], r_out[:4], want["rings"][:4])
    written = int(c_out[3])
    assert np.array_equal(v_out[:written], want["vertices"][:written])
    assert (v_out[written:] == CANARY).all(), "a vertex row past counts_out[3] was written"
    return want, r_out, v_out, c_out


HAND_MADE = K.hand_made()


@pytest.mark.parametrize("tol", K.TOLERANCES)
@pytest.mark.parametrize("name", list(HAND_MADE))
def test_hand_made_shapes(name, tol):
    table = S.table(HAND_MADE[name], max_rings=len(HAND_MADE[name]) + 2, max_vertices=sum(len(v) for v in HAND_MADE[name]) + 3)
    want, r_out, v_out, c_out = _check(*table, S.tol2_q(tol))
    assert c_out[4] == 0 and c_out[1] == len(HAND_MADE[name])
    if tol == 0 and name not in ("degenerate",):
        assert np.array_equal(v_out[:c_out[3]], table[1][:c_out[3]]) and c_out[3] == table[2][3]
    if name == "pixel":
        assert r_out[0].tolist() == [1, 0, 4 if tol <= 0.5 else 3, 2 if tol <= 0.5 else 1, 4, 3, 2, 4]   # a corner lies 0.707 px off the diagonal
    if name == "strictness" and tol == 1.0:
        assert r_out[:2, 2].tolist() == [3, 4], "a vertex on the tolerance is dropped, one lattice step further out it is kept"
    if name == "full_range" and tol == 1024.0:
        assert r_out[:2, 2].tolist() == [3, 4], "1448 and 1449 off the diagonal lie on either side of 1024 px"
    if name == "winding" and tol == 0:
        assert r_out[0, 2] == 20 and r_out[0, 3] == 5 * 2 ** 29 - 2 ** 32, "the shoelace sum of five turns, modulo 2^32"
    if tol == 1024.0 and name not in ("degenerate", "full_range", "winding"):
        assert (r_out[:c_out[1], 2] == 3).all() and (r_out[:c_out[1], 3] != 0).all()


LIMITS = functools.lru_cache(maxsize=None)(lambda: ops.outlines_simplify_limits())


@pytest.mark.parametrize("which", [0, 1])
@pytest.mark.parametrize("tol", [1.0, 150.0])
def test_rings_on_both_sides_of_a_tier_limit(which, tol):
    T = LIMITS()[which]
    assert 4 <= LIMITS()[0] < LIMITS()[1] <= 1 << 20
    small = [[(1, 1), (9, 1), (9, 5)], [(3, 2), (4, 2), (4, 3), (3, 3)]]
    ring_lists = []
    for k, n in enumerate((T - 1, T, T + 1)):                # rings of 3 and 4 vertices between them: the scan crosses tiers
        ring_lists += [K.lattice_ring(n, seed=10 * which + k), small[k % 2], small[(k + 1) % 2]]
    table = S.table(ring_lists, max_rings=len(ring_lists) + 1, max_vertices=sum(len(v) for v in ring_lists) + 5)
    want, r_out, _, c_out = _check(*table, S.tol2_q(tol))
    assert c_out[4] == 0 and r_out[:9, 7].tolist() == [len(v) for v in ring_lists]
    assert all(3 <= r_out[r, 2] <= r_out[r, 7] for r in (0, 3, 6))
    assert tol < 150 or all(r_out[r, 2] < r_out[r, 7] for r in (0, 3, 6)), "the noisy circles lose vertices at 150 px"


WIDEST_WORKGROUP = 1024                                      # no workgroup of the device has more threads


@pytest.mark.parametrize("case", ["wave", "lds", "hbm"])
def test_recursion_deeper_than_a_workgroup_is_wide(case):
    wave, lds = LIMITS()
    assert lds >= 1200, "the comb of the LDS tier needs room for more teeth than a workgroup has threads"
    ring = {"wave": K.zigzag_ring(wave - 6), "lds": K.zigzag_ring(1040), "hbm": K.zigzag_ring(1040, filler=lds - 1000)}[case]
    info = {}
    S.simplify_ring(ring, S.tol2_q(1.0), info=info)
    if case == "wave":                                       # a ring of one wave cannot be deeper than it has vertices
        assert 4 < len(ring) <= wave and info["depth"] >= len(ring) - 6
    else:                                                    # deeper than any workgroup is wide, whatever the kernel's is
        assert (wave < len(ring) <= lds if case == "lds" else len(ring) > lds) and info["depth"] > WIDEST_WORKGROUP
    table = S.table([ring, [(0, 0), (5, 0), (5, 5), (0, 5)]])
    want, r_out, _, c_out = _check(*table, S.tol2_q(1.0))
    assert c_out[4] == 0 and r_out[0, 2] >= info["depth"]


def _mixed_table():
    lists = HAND_MADE["holed"] + HAND_MADE["plus"] + HAND_MADE["staircase"] + HAND_MADE["L"] + [K.lattice_ring(100, 5, 50, 8, 60)]
    return S.table(lists, max_rings=9, max_vertices=sum(len(v) for v in lists) + 4)


def test_pass_through_and_bad_rows():
    rings, vertices, counts = _mixed_table()
    rings[1, 1] = -1                                         # a ring the outlines call had no room for
    counts[4] = S.ST_TRUNCATED
    want, r_out, _, c_out = _check(rings, vertices, counts, S.tol2_q(1.0))
    assert c_out[4] == S.ST_TRUNCATED and r_out[1, 1:4].tolist() == [-1, 0, 0] and r_out[2, 1] == r_out[0, 2]
    for change in ("n_past_the_end", "negative_n", "coordinate", "negative_coordinate", "big_coordinate_in_a_big_ring", "overlap"):
        rings, vertices, counts = _mixed_table()
        row = 3
        if change == "n_past_the_end":
            rings[row, 2] = int(counts[3]) - int(rings[row, 1]) + 1
        elif change == "negative_n":
            rings[row, 2] = -5
        elif change == "coordinate":
            vertices[int(rings[row, 1]) + 2] = (16385, 3)
        elif change == "negative_coordinate":
            vertices[int(rings[row, 1]) + 2] = (3, -1)
        elif change == "big_coordinate_in_a_big_ring":
            row = 5
            vertices[int(rings[row, 1]) + 70] = (1 << 30, 0)
        else:                                                # every row names the whole list: their state has no room
            row = 1
            rings[:6, 1] = 0
            rings[:6, 2] = int(counts[3])
        want, r_out, _, c_out = _check(rings, vertices, counts, S.tol2_q(1.0))
        assert c_out[4] == S.ST_BAD_INPUT, change
        assert r_out[row, 1:4].tolist() == [-1, 0, 0] and r_out[row, 7] == rings[row, 2] and r_out[0, 1] == 0 and r_out[0, 2] >= 3
    rings, vertices, counts = _mixed_table()
    counts[1] = 4                                            # fewer rows than rings found: only those are read
    counts[4] = S.ST_TRUNCATED
    want, r_out, _, c_out = _check(rings, vertices, counts, S.tol2_q(1.0))
    assert c_out[:2].tolist() == [6, 4] and not r_out[4:].any()
    counts[1] = 1000                                         # more rows than the table has
    want, r_out, _, c_out = _check(rings, vertices, counts, S.tol2_q(1.0))
    assert c_out[1] == 9


def test_bad_counts_simplify_nothing():
    rings, vertices, counts = _mixed_table()
    counts[4] = S.ST_BAD_COUNTS | S.ST_TRUNCATED
    want, r_out, v_out, c_out = _check(rings, vertices, counts, 16)
    assert c_out.tolist() == [0, 0, 0, 0, S.ST_BAD_COUNTS] and not r_out.any() and (v_out == CANARY).all()


def test_refusals_leave_the_outputs_untouched():
    rings, vertices, counts = (torch.from_numpy(a).to(DEV) for a in _mixed_table())
    ws = torch.empty(L.lib().c3d_outlines_simplify_ws_bytes(*map(len, (rings, vertices))), dtype=torch.uint8, device=DEV)
    r_out = torch.full((len(rings), 8), CANARY, dtype=torch.int32, device=DEV)
    v_out = torch.full((len(vertices), 2), CANARY, dtype=torch.int32, device=DEV)
    c_out = torch.full((5,), CANARY, dtype=torch.int32, device=DEV)
    good = dict(rings=rings.data_ptr(), vertices=vertices.data_ptr(), counts=counts.data_ptr(), max_rings=len(rings),
                max_vertices=len(vertices), tol2_q=16, rings_out=r_out.data_ptr(), vertices_out=v_out.data_ptr(),
                counts_out=c_out.data_ptr(), ws=ws.data_ptr())
    bad = [dict(rings=None), dict(vertices=None), dict(counts=None), dict(rings_out=None), dict(vertices_out=None), dict(counts_out=None),
           dict(ws=None), dict(max_rings=0), dict(max_rings=-4), dict(max_vertices=0), dict(tol2_q=-1), dict(tol2_q=S.TOL2_Q_MAX + 1),
           dict(tol2_q=1 << 40)]
    for change in bad:
        rc = L.lib().c3d_outlines_simplify(*{**good, **change}.values(), torch.cuda.current_stream().cuda_stream)
        assert rc == -1, (change, rc)                       # C3D_E_BADARG
    torch.cuda.synchronize()
    assert (r_out == CANARY).all() and (v_out == CANARY).all() and (c_out == CANARY).all()
    assert L.lib().c3d_outlines_simplify(*{**good, "tol2_q": S.TOL2_Q_MAX}.values(), torch.cuda.current_stream().cuda_stream) == 0
    torch.cuda.synchronize()
    assert c_out[:2].tolist() == [6, 6] and int(c_out[4]) == 0 and (r_out[:6, 2] == 3).all()


def test_two_calls_agree_bit_for_bit_also_on_a_dirty_workspace():
    lists = [K.lattice_ring(n, n, 3000, 300) for n in (40, 64, 65, 500, LIMITS()[1] + 9)] + HAND_MADE["plus"]
    table = S.table(lists)
    ws = torch.empty(L.lib().c3d_outlines_simplify_ws_bytes(len(table[0]), len(table[1])), dtype=torch.uint8, device=DEV)
    first = _call(*table, S.tol2_q(40.0), ws=ws, fill_ws=0)
    again = _call(*table, S.tol2_q(40.0), ws=ws)              # what the first call left behind
    dirty = _call(*table, S.tol2_q(40.0), ws=ws, fill_ws=0xFF)
    other = _call(*table, S.tol2_q(3.0), ws=ws)               # another tolerance's leftovers
    back = _call(*table, S.tol2_q(40.0), ws=ws)
    assert first[0] == 0 and first[3][4] == 0 and other[0] == 0 and other[3][2] > first[3][2]
    for run in (again, dirty, back):
        assert run[0] == 0 and all(np.array_equal(a, b) for a, b in zip(run[1:], first[1:]))


def test_non_default_stream_and_the_python_op():
    table = _mixed_table()
    want = S.simplify(*table, S.tol2_q(1.5))
    dev = [torch.from_numpy(a).to(DEV) for a in table]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        r_out, v_out, c_out = ops.outlines_simplify(*dev, 1.5)
    side.synchronize()
    assert r_out.shape == dev[0].shape and v_out.shape == dev[1].shape and r_out.dtype == v_out.dtype == c_out.dtype == torch.int32
    assert np.array_equal(c_out.cpu().numpy(), want["counts"]) and np.array_equal(r_out.cpu().numpy(), want["rings"])
    assert np.array_equal(v_out[:int(c_out[3])].cpu().numpy(), want["vertices"][:int(c_out[3])])
    with pytest.raises(ValueError):
        ops.outlines_simplify(*dev, 1025.0)
    with pytest.raises(L.Change3DHipError):
        ops.outlines_simplify(dev[0].cpu(), dev[1], dev[2], 1.0)


def test_negative_controls_see_strictness_and_the_segment_distance():
    for name, q, variant in (("strictness", 16, dict(strict=False)), ("hook", S.tol2_q(2.0), dict(segment=False))):
        table = S.table(HAND_MADE[name])
        rc, r_out, v_out, c_out = _call(*table, q)
        wrong = S.simplify(*table, q, **variant)
        assert rc == 0 and not (np.array_equal(c_out, wrong["counts"]) and np.array_equal(r_out, wrong["rings"])
                                and np.array_equal(v_out[:c_out[3]], wrong["vertices"][:c_out[3]])), (name, variant)


@pytest.fixture(scope="module")
def bcd_model():
    from test_scene_bda_gpu import _model
    return _model("bcd")


def test_predict_with_simplify_end_to_end(bcd_model):
    from change3d_amd.infer import SceneInferencer, SceneObjects, SceneOutlines
    from test_scene_bda_gpu import _scene
    scene = _scene(70, 90, 2)                               # a little over one 64 x 64 tile
    inf = SceneInferencer(bcd_model, "bcd", stride=32, batch=5)
    raw = inf.predict(scene, objects=True, min_area=2, outlines=True)
    none = inf.predict(scene, objects=True, min_area=2, outlines=True, simplify=None)
    out = inf.predict(scene, objects=True, min_area=2, outlines=True, simplify=1.0)
    assert len(raw) == len(none) == 4 and len(out) == 5 and isinstance(out[2], SceneObjects)
    assert isinstance(out[3], SceneOutlines) and isinstance(out[4], SceneOutlines)
    n = int(raw[3].counts[3])
    for a, b in zip(raw[3], out[3]):
        assert torch.equal(a[:n] if a.shape[-1] == 2 else a, b[:n] if b.shape[-1] == 2 else b)
    rings, vertices, counts = ops.outlines_simplify(*out[3], 1.0)
    assert torch.equal(out[4].counts, counts) and torch.equal(out[4].rings, rings)
    assert torch.equal(out[4].vertices[:int(counts[3])], vertices[:int(counts[3])])
    want = S.simplify(*(t.cpu().numpy() for t in out[3]), S.tol2_q(1.0))
    assert np.array_equal(counts.cpu().numpy(), want["counts"]) and np.array_equal(rings.cpu().numpy(), want["rings"])
    assert int(counts[4]) == 0 and int(counts[0]) == int(out[3].counts[0]) > 0 and 0 < int(counts[2]) <= int(out[3].counts[2])
    with pytest.raises(ValueError):
        inf.predict(scene, objects=True, simplify=1.0)


def test_predict_scene_simplify_in_a_child_process(bcd_model, tmp_path):
    from PIL import Image
    from test_scene_bda_gpu import T, _scene
    scene = _scene(70, 90, 4)
    Image.fromarray(scene[:, :, 0:3]).save(tmp_path / "a.png")
    Image.fromarray(scene[:, :, 3:6]).save(tmp_path / "b.png")
    torch.save(bcd_model.state_dict(), tmp_path / "best_model.pth")
    docs = {}
    for name, extra in (("raw", []), ("simple", ["--simplify", "1.0"])):
        cmd = [sys.executable, "-m", "change3d_amd.scripts.predict_scene", "--task", "BCD", "--weights", str(tmp_path / "best_model.pth"),
               "--pre", str(tmp_path / "a.png"), "--post", str(tmp_path / "b.png"), "--stride", "32", "--batch_size", "5", "--act_dtype",
               "f32", "--in_height", str(T), "--in_width", str(T), "--pretrained", "/nonexistent", "--out_dir", str(tmp_path / name),
               "--objects", "--polygons"] + extra
        done = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
        assert done.returncode == 0, done.stderr[-3000:] + done.stdout[-2000:]
        docs[name] = json.loads((tmp_path / name / "objects" / "scene.geojson").read_text())
    raw, simple = docs["raw"], docs["simple"]
    assert len(raw["features"]) == len(simple["features"]) > 0
    total = lambda doc: sum(len(ring) - 1 for f in doc["features"] for ring in f["geometry"]["coordinates"])  # noqa: E731
    for f, g in zip(simple["features"], raw["features"]):
        assert "vertices" not in g["properties"] and f["properties"]["id"] == g["properties"]["id"]
        rings = f["geometry"]["coordinates"]
        assert all(ring[0] == ring[-1] and len(ring) >= 4 for ring in rings)
        assert f["properties"]["vertices"] == sum(len(ring) - 1 for ring in rings) <= f["properties"]["vertices_raw"]
        assert f["properties"]["vertices_raw"] == sum(len(ring) - 1 for ring in g["geometry"]["coordinates"])
    assert total(simple) < total(raw)
