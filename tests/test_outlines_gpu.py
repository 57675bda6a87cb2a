"""`c3d_scene_outlines` against its restatement (tests/outlines_reference.py): rings, vertices and counts exactly equal, on
labels that `ops.scene_objects` made, so that the pair is tested as it is used.  Hand-made masks, sizes around the chunk,
wave and tile seams, upstream filtering and truncation, truncation of the outputs between canary rows, a negative control
on the turn rule, determinism on a dirty workspace, a non-default stream, the refusals, and `predict(outlines=True)` /
`predict_scene --polygons` end to end."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import outlines_reference as R  # noqa: E402

from change3d_amd import _lib as L  # noqa: E402
from change3d_amd import ops  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAD, CANARY = 3, -7777


def _labelled(mask, connectivity, min_area=1, max_objects=None):
    mask = np.ascontiguousarray(mask, dtype=np.uint8)
    max_objects = mask.size if max_objects is None else max_objects
    labels, _, _, _, counts = ops.scene_objects(torch.from_numpy(mask).to(DEV), connectivity=connectivity, min_area=min_area,
                                                max_objects=max_objects, want_object_cls=False)
    return labels, counts, max_objects


def _call(labels, counts, connectivity, max_objects, max_rings, max_vertices, ws=None, fill_ws=None):
    """The C entry on output buffers with canary rows on both sides: (rc, rings, vertices, counts) as numpy, canaries checked."""
    Hs, Ws = labels.shape
    rings = torch.full((max(max_rings, 0) + 2 * PAD, 8), CANARY, dtype=torch.int32, device=DEV)
    verts = torch.full((max(max_vertices, 0) + 2 * PAD, 2), CANARY, dtype=torch.int32, device=DEV)
    out = torch.full((5 + 2 * PAD,), CANARY, dtype=torch.int32, device=DEV)
    if ws is None:
        ws = torch.empty(max(L.lib().c3d_scene_outlines_ws_bytes(Hs, Ws), 256), dtype=torch.uint8, device=DEV)
    if fill_ws is not None:
        ws.fill_(fill_ws)
    rc = L.lib().c3d_scene_outlines(labels.data_ptr(), counts.data_ptr(), Hs, Ws, connectivity, max_objects, max_rings, max_vertices,
                                    rings[PAD:].data_ptr(), verts[PAD:].data_ptr(), out[PAD:].data_ptr(), ws.data_ptr(),
                                    torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    rings, verts, out = rings.cpu().numpy(), verts.cpu().numpy(), out.cpu().numpy()
    for buf in (rings, verts, out):
        assert (buf[:PAD] == CANARY).all() and (buf[len(buf) - PAD:] == CANARY).all(), "a canary row was written"
    return rc, rings[PAD:len(rings) - PAD], verts[PAD:len(verts) - PAD], out[PAD:PAD + 5]


def _check(mask, connectivity, min_area=1, max_objects=None, max_rings=None, max_vertices=None):
    """Device against restatement on `mask`: exact.  Returns (restatement, device rings, vertices, counts)."""
    labels, counts, max_objects = _labelled(mask, connectivity, min_area, max_objects)
    n = labels.numel()
    max_rings = n + 2 if max_rings is None else max_rings
    max_vertices = 4 * n + 2 if max_vertices is None else max_vertices
    want = R.outlines(labels.cpu().numpy(), counts.cpu().numpy(), connectivity, max_objects, max_rings, max_vertices)
    rc, rings, verts, got = _call(labels, counts, connectivity, max_objects, max_rings, max_vertices)
    assert rc == 0
    assert np.array_equal(got, want["counts"]), (got, want["counts"])
    assert np.array_equal(rings, want["rings"]), np.argwhere(rings != want["rings"])[:5]
    written = int(got[3])
    assert np.array_equal(verts[:written], want["vertices"][:written])
    assert (verts[written:] == CANARY).all(), "a vertex row past counts[3] was written"
    return want, rings, verts, got


def _frames(size, offsets):
    m = np.zeros((size, size), np.uint8)
    for o in offsets:
        m[o:size - o, o] = m[o:size - o, size - 1 - o] = m[o, o:size - o] = m[size - 1 - o, o:size - o] = 1
    return m


def _hand_made():
    rng = np.random.default_rng(1)
    yy, xx = np.mgrid[0:96, 0:160]
    pixel = np.zeros((5, 7), np.uint8)
    pixel[2, 3] = 1
    wide = np.ones((4, 7), np.uint8)
    wide[1:3, 2:5] = 0
    diag_holes = np.ones((4, 4), np.uint8)
    diag_holes[1, 1] = diag_holes[2, 2] = 0
    cross = np.zeros((9, 11), np.uint8)
    cross[4, :] = cross[:, 5] = 1
    nested = _frames(13, (0, 2, 4))
    nested[6, 6] = 1
    cy, cx = np.mgrid[0:64, 0:64]
    return [("pixel", pixel), ("1x1", np.ones((1, 1), np.uint8)), ("1x1_empty", np.zeros((1, 1), np.uint8)),
            ("1xN", (rng.random((1, 70)) < 0.6).astype(np.uint8)), ("Nx1", (rng.random((70, 1)) < 0.6).astype(np.uint8)),
            ("diagonal_pair", np.array([[1, 0], [0, 1]], np.uint8)), ("ring", _frames(3, (0,))), ("wide_hole", wide),
            ("diagonal_holes", diag_holes), ("four_borders", cross), ("foreground", np.ones((66, 70), np.uint8)),
            ("empty", np.zeros((10, 10), np.uint8)), ("checkerboard", ((cy + cx) % 2 == 0).astype(np.uint8)),
            ("serpentine", ((yy % 2 == 0) | ((yy % 4 == 1) & (xx == 159)) | ((yy % 4 == 3) & (xx == 0))).astype(np.uint8)),
            ("nested", nested)]


HAND_MADE = dict(_hand_made())


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("name", list(HAND_MADE))
def test_hand_made_masks(name, connectivity):
    want, rings, _, counts = _check(HAND_MADE[name], connectivity)
    assert counts[4] == 0
    if name in ("empty", "1x1_empty"):
        assert counts.tolist() == [0, 0, 0, 0, 0]
    if name == "foreground":
        assert counts.tolist()[:4] == [1, 1, 4, 4] and rings[0].tolist() == [1, 0, 4, 66 * 70, 2 * (66 + 70), 0, 0, 0]
    if name == "serpentine":                                # one outline of thousands of edges: most doubling rounds
        assert counts[0] == 1 and rings[0, 4] > 10000 and rings[0, 3] == int(HAND_MADE[name].sum())
    if name == "checkerboard":
        assert counts[0] == (2048 if connectivity == 4 else 1 + 62 * 62 // 2)   # every inner background pixel is a hole
    if name == "nested":                                    # object inside hole inside object, three deep, and a centre pixel
        assert sorted(rings[:counts[1], 3].tolist()) == sorted([169, -121, 81, -49, 25, -9, 1])


@pytest.mark.parametrize("size", [(h, w) for h in (63, 64, 65) for w in (127, 128, 129)] + [(97, 131)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_random_masks_around_the_seams(size):
    rng = np.random.default_rng(size[0] * 1000 + size[1])
    for density in (0.3, 0.59, 0.9):
        mask = (rng.random(size) < density).astype(np.uint8)
        for connectivity in (4, 8):
            _, _, _, counts = _check(mask, connectivity)
            assert counts[4] == 0 and counts[0] == counts[1] > 0


@pytest.mark.parametrize("connectivity", [4, 8])
def test_inputs_as_produced_upstream(connectivity):
    mask = (np.random.default_rng(5).random((65, 129)) < 0.45).astype(np.uint8)
    want, rings, _, counts = _check(mask, connectivity, min_area=5)        # removed specks are background
    assert counts[4] == 0
    want, rings, _, counts = _check(mask, connectivity, min_area=1, max_objects=7)   # ids above the table own no edges
    assert counts[4] == R.ST_TRUNCATED and counts[0] > 0 and set(rings[:counts[1], 0].tolist()) == set(range(1, 8))


@functools.lru_cache(maxsize=None)
def _truncation_case():
    mask = (np.random.default_rng(11).random((40, 50)) < 0.3).astype(np.uint8)
    labels, counts, max_objects = _labelled(mask, 8)
    n = labels.numel()
    full = R.outlines(labels.cpu().numpy(), counts.cpu().numpy(), 8, max_objects, n, 4 * n)
    return mask, int(full["counts"][0]), int(full["counts"][2])


@pytest.mark.parametrize("case", ["exact", "rings-1", "vertices-1", "both-1", "far", "one"])
def test_truncation_is_prefix_shaped_and_in_range(case):
    mask, nr, nv = _truncation_case()
    max_rings, max_vertices = {"exact": (nr, nv), "rings-1": (nr - 1, nv), "vertices-1": (nr, nv - 1), "both-1": (nr - 1, nv - 1),
                               "far": (nr // 7, nv // 5), "one": (1, 1)}[case]
    want, rings, _, counts = _check(mask, 8, max_rings=max_rings, max_vertices=max_vertices)
    assert counts[0] == nr and counts[2] == nv and counts[1] == min(nr, max_rings)
    assert counts[4] == (0 if case == "exact" else R.ST_TRUNCATED)
    fit = rings[:counts[1], 1] >= 0
    k = int(fit.sum())
    assert fit[:k].all() and (rings[k:counts[1], 1] == -1).all()
    if case == "exact":
        assert k == nr and counts[3] == nv
    if case == "vertices-1":                                # the last ring alone does not fit
        assert k == nr - 1 and rings[nr - 1, 1] == -1 and counts[3] == nv - rings[nr - 1, 2]
    if case == "both-1":                                    # the ring table ends before the ring that would not fit
        assert k == nr - 1 and counts[3] < nv
    if case == "one":
        assert k == 0 and counts[3] == 0 and rings[0, 1] == -1 and rings[0, 0] > 0


def test_negative_control_sees_the_turn_rule():
    for mask, connectivity in ((np.array([[1, 0], [0, 1]], np.uint8), 8), ((np.random.default_rng(2).random((33, 47)) < 0.59).astype(np.uint8), 8),
                               ((np.random.default_rng(2).random((33, 47)) < 0.59).astype(np.uint8), 4)):
        labels, counts, max_objects = _labelled(mask, connectivity)
        n = labels.numel()
        rc, rings, verts, got = _call(labels, counts, connectivity, max_objects, n + 2, 4 * n + 2)
        wrong = R.outlines(labels.cpu().numpy(), counts.cpu().numpy(), connectivity, max_objects, n + 2, 4 * n + 2, flip=True)
        assert rc == 0 and not (np.array_equal(got, wrong["counts"]) and np.array_equal(rings, wrong["rings"])
                                and np.array_equal(verts[:got[3]], wrong["vertices"][:got[3]]))


def test_two_calls_agree_bit_for_bit_also_on_a_dirty_workspace():
    mask = (np.random.default_rng(8).random((65, 129)) < 0.59).astype(np.uint8)
    labels, counts, max_objects = _labelled(mask, 8)
    n = labels.numel()
    ws = torch.empty(L.lib().c3d_scene_outlines_ws_bytes(*labels.shape), dtype=torch.uint8, device=DEV)
    first = _call(labels, counts, 8, max_objects, n, 4 * n, ws=ws, fill_ws=0)
    again = _call(labels, counts, 8, max_objects, n, 4 * n, ws=ws)                 # what the first call left behind
    dirty = _call(labels, counts, 8, max_objects, n, 4 * n, ws=ws, fill_ws=0xFF)
    other = _call(labels.flip(0).contiguous(), counts, 8, max_objects, n, 4 * n, ws=ws)    # another scene's leftovers
    back = _call(labels, counts, 8, max_objects, n, 4 * n, ws=ws)
    assert first[0] == 0 and first[3][4] == 0 and other[0] == 0
    for run in (again, dirty, back):
        assert run[0] == 0 and all(np.array_equal(a, b) for a, b in zip(run[1:], first[1:]))


def test_non_default_stream_and_the_python_op():
    mask = (np.random.default_rng(9).random((64, 127)) < 0.5).astype(np.uint8)
    labels, counts, max_objects = _labelled(mask, 4)
    want = R.outlines(labels.cpu().numpy(), counts.cpu().numpy(), 4, max_objects, 900, 9000)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        rings, vertices, out = ops.scene_outlines(labels, counts, connectivity=4, max_objects=max_objects, max_rings=900, max_vertices=9000)
    side.synchronize()
    assert rings.shape == (900, 8) and vertices.shape == (9000, 2) and rings.dtype == vertices.dtype == out.dtype == torch.int32
    assert np.array_equal(out.cpu().numpy(), want["counts"]) and np.array_equal(rings.cpu().numpy(), want["rings"])
    assert np.array_equal(vertices[:int(out[3])].cpu().numpy(), want["vertices"][:int(out[3])])
    d_rings, d_vertices, _ = ops.scene_outlines(labels, counts, connectivity=4, max_objects=max_objects)
    assert (d_rings.shape[0], d_vertices.shape[0]) == ops.scene_outlines_defaults(64, 127, max_objects)
    with pytest.raises(L.Change3DHipError):
        ops.scene_outlines(labels, counts, connectivity=6)
    with pytest.raises(L.Change3DHipError):
        ops.scene_outlines(labels.cpu(), counts)


def test_refusals_leave_the_outputs_untouched():
    labels, counts, max_objects = _labelled(np.ones((6, 9), np.uint8), 8)
    ws = torch.empty(L.lib().c3d_scene_outlines_ws_bytes(6, 9), dtype=torch.uint8, device=DEV)
    rings = torch.full((8, 8), CANARY, dtype=torch.int32, device=DEV)
    verts = torch.full((16, 2), CANARY, dtype=torch.int32, device=DEV)
    out = torch.full((5,), CANARY, dtype=torch.int32, device=DEV)
    good = dict(labels=labels.data_ptr(), counts_obj=counts.data_ptr(), Hs=6, Ws=9, connectivity=8, max_objects=max_objects,
                max_rings=8, max_vertices=16, rings=rings.data_ptr(), vertices=verts.data_ptr(), counts=out.data_ptr(), ws=ws.data_ptr())
    bad = [dict(labels=None), dict(counts_obj=None), dict(rings=None), dict(vertices=None), dict(counts=None), dict(ws=None),
           dict(Hs=0), dict(Ws=0), dict(Hs=-3), dict(connectivity=6), dict(connectivity=0), dict(max_objects=0), dict(max_rings=0),
           dict(max_vertices=0), dict(max_vertices=-1)]
    for change in bad:
        rc = L.lib().c3d_scene_outlines(*{**good, **change}.values(), torch.cuda.current_stream().cuda_stream)
        assert rc == -1, (change, rc)                       # C3D_E_BADARG
    for Hs, Ws in ((1 << 15, 1 << 14), (1 << 29, 1), (46341, 46341)):
        rc = L.lib().c3d_scene_outlines(*{**good, "Hs": Hs, "Ws": Ws}.values(), torch.cuda.current_stream().cuda_stream)
        assert rc == -2 and L.lib().c3d_scene_outlines_ws_bytes(Hs, Ws) == -2           # C3D_E_UNSUPPORTED
    assert L.lib().c3d_scene_outlines_ws_bytes(0, 9) == -1 and L.lib().c3d_scene_outlines_ws_bytes(6, -1) == -1
    torch.cuda.synchronize()
    assert (rings == CANARY).all() and (verts == CANARY).all() and (out == CANARY).all()
    assert L.lib().c3d_scene_outlines(*good.values(), torch.cuda.current_stream().cuda_stream) == 0
    torch.cuda.synchronize()
    assert out.tolist() == [1, 1, 4, 4, 0] and rings[0].tolist() == [1, 0, 4, 54, 30, 0, 0, 0]


def test_bad_counts_trace_nothing():
    labels, counts, max_objects = _labelled(np.ones((6, 9), np.uint8), 8)
    bad = torch.tensor([-1, 0], dtype=torch.int32, device=DEV)
    rc, rings, verts, out = _call(labels, bad, 8, max_objects, 8, 16)
    assert rc == 0 and out.tolist() == [0, 0, 0, 0, R.ST_BAD_COUNTS] and not rings.any() and (verts == CANARY).all()


@pytest.fixture(scope="module")
def bcd_model():
    from test_scene_bda_gpu import _model
    return _model("bcd")


def test_predict_with_outlines_end_to_end(bcd_model):
    from change3d_amd.infer import SceneInferencer, SceneObjects, SceneOutlines
    from test_scene_bda_gpu import _scene
    scene = _scene(70, 90, 2)                               # a little over one 64 x 64 tile
    inf = SceneInferencer(bcd_model, "bcd", stride=32, batch=5)
    plain = inf.predict(scene, objects=True, min_area=2)
    out = inf.predict(scene, objects=True, min_area=2, outlines=True)
    assert len(plain) == 3 and isinstance(plain[-1], SceneObjects) and len(out) == 4
    assert isinstance(out[2], SceneObjects) and isinstance(out[3], SceneOutlines)
    assert all(torch.equal(a, b) for a, b in zip(plain[:2], out[:2])) and torch.equal(plain[2].labels, out[2].labels)
    objects, outlines = out[2], out[3]
    rings, vertices, counts = ops.scene_outlines(objects.labels, objects.counts, connectivity=8)
    assert torch.equal(outlines.counts, counts) and torch.equal(outlines.rings, rings)
    assert torch.equal(outlines.vertices[:int(counts[3])], vertices[:int(counts[3])])
    assert int(counts[4]) == 0 and int(counts[0]) >= int(objects.counts[0]) > 0
    labels, r, v = objects.labels.cpu().numpy(), rings[:int(counts[1])].cpu().numpy(), vertices.cpu().numpy()
    for i in range(1, int(objects.counts[0]) + 1):
        own = [v[row[1]:row[1] + row[2]] for row in r if row[0] == i]
        assert np.array_equal(R.rasterise(own, 70, 90), labels == i)
    small = inf.predict(scene, objects=True, min_area=2, outlines=True, max_rings=2, max_vertices=5)[3]
    assert small.rings.shape == (2, 8) and small.vertices.shape == (5, 2) and int(small.counts[4]) == R.ST_TRUNCATED
    with pytest.raises(ValueError):
        inf.predict(scene, outlines=True)


def test_predict_scene_polygons_in_a_child_process(bcd_model, tmp_path):
    from PIL import Image
    from test_scene_bda_gpu import T, _scene
    scene = _scene(70, 90, 4)
    Image.fromarray(scene[:, :, 0:3]).save(tmp_path / "a.png")
    Image.fromarray(scene[:, :, 3:6]).save(tmp_path / "b.png")
    torch.save(bcd_model.state_dict(), tmp_path / "best_model.pth")
    cmd = [sys.executable, "-m", "change3d_amd.scripts.predict_scene", "--task", "BCD", "--weights", str(tmp_path / "best_model.pth"),
           "--pre", str(tmp_path / "a.png"), "--post", str(tmp_path / "b.png"), "--stride", "32", "--batch_size", "5", "--act_dtype", "f32",
           "--in_height", str(T), "--in_width", str(T), "--pretrained", "/nonexistent", "--out_dir", str(tmp_path / "out"), "--objects",
           "--polygons"]
    done = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert done.returncode == 0, done.stderr[-3000:] + done.stdout[-2000:]
    doc = json.loads((tmp_path / "out" / "objects" / "scene.geojson").read_text())
    lines = (tmp_path / "out" / "objects" / "scene.csv").read_text().splitlines()
    assert doc["type"] == "FeatureCollection" and len(doc["features"]) == len(lines) - 1 > 0
    for feature, line in zip(doc["features"], lines[1:]):
        f = line.split(",")
        assert feature["properties"]["id"] == int(f[0]) and feature["properties"]["area"] == int(f[1])
        assert all(ring[0] == ring[-1] and len(ring) >= 5 for ring in feature["geometry"]["coordinates"])
