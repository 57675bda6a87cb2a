"""`c3d_rings_hull` in the layers above it: `predict(shapes=True)` against the op on `predict`'s own outlines, with and
without simplification and splitting, and `predict_scene --shapes` in a child process on a small synthetic pair: the files
parse, every rectangle holds its hull, and the properties agree with the restatement."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hull_reference as R  # noqa: E402

from change3d_amd import ops  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HS, WS = 150, 170


@pytest.fixture(scope="module")
def bcd_model():
    from test_scene_bda_gpu import _model
    return _model("bcd")


def test_predict_with_shapes_equals_the_op_on_its_own_outlines(bcd_model):
    from change3d_amd.infer import SceneInferencer, SceneOutlines, SceneShapes
    from test_scene_bda_gpu import _scene
    scene = _scene(70, 90, 2)
    inf = SceneInferencer(bcd_model, "bcd", stride=32, batch=5)
    for extra in (dict(), dict(simplify=1.0), dict(split=2.0), dict(simplify=1.0, simplify_check=True)):
        today = inf.predict(scene, objects=True, min_area=2, outlines=True, **extra)
        before = ops.launch_count()
        off = inf.predict(scene, objects=True, min_area=2, outlines=True, shapes=False, **extra)
        plain = ops.launch_count() - before
        before = ops.launch_count()
        out = inf.predict(scene, objects=True, min_area=2, outlines=True, shapes=True, **extra)
        assert ops.launch_count() - before == plain + 9, "shapes=True adds the nine launches of c3d_rings_hull and nothing else"
        assert len(today) == len(off) == len(out) - 1 and isinstance(out[-1], SceneShapes) and isinstance(out[3], SceneOutlines)
        for a, b, c in zip(today, off, out[:-1]):            # exactly today's tuple in front of the SceneShapes
            n = int(a.counts[3]) if isinstance(a, SceneOutlines) else None   # vertex rows past the written count are not initialised
            for x, y, z in zip(*(t if isinstance(t, tuple) else (t,) for t in (a, b, c))):
                if x is None:
                    assert y is None and z is None
                elif isinstance(x, tuple):                   # the match of a SceneFill
                    assert all(torch.equal(p, q) and torch.equal(p, r) for p, q, r in zip(x, y, z))
                elif n is not None and x.dim() == 2 and x.shape[-1] == 2:
                    assert torch.equal(x[:n], y[:n]) and torch.equal(x[:n], z[:n])
                else:
                    assert torch.equal(x, y) and torch.equal(x, z)
        raw, shapes = out[3], out[-1]
        hulls, hv, rects, hc = ops.rings_hull(*raw, max_objects=out[2].table.shape[0])
        written = int(hc[3])
        assert torch.equal(shapes.hulls, hulls) and torch.equal(shapes.rects, rects) and torch.equal(shapes.counts, hc)
        assert torch.equal(shapes.vertices[:written], hv[:written])
        rows = int(out[2].counts[1])
        assert rows > 0 and shapes.counts.tolist()[:2] == [rows, rows] and int(shapes.counts[4]) == 0
        want = R.hulls(*(t.cpu().numpy() for t in raw), hulls.shape[0], hv.shape[0], fast=True)
        assert np.array_equal(hulls.cpu().numpy(), want["hulls"]) and np.array_equal(rects.cpu().numpy(), want["rects"])
        assert np.array_equal(hv[:written].cpu().numpy(), want["vertices"][:written])
    with pytest.raises(ValueError):
        inf.predict(scene, objects=True, shapes=True)
    with pytest.raises(ValueError):
        inf.predict(scene, shapes=True)


def _run(tmp, name, extra):
    from test_scene_bda_gpu import T
    cmd = [sys.executable, "-m", "change3d_amd.scripts.predict_scene", "--task", "BCD", "--weights", str(tmp / "best_model.pth"), "--pre",
           str(tmp / "a.png"), "--post", str(tmp / "b.png"), "--stride", "32", "--batch_size", "32", "--act_dtype", "f32", "--in_height", str(T),
           "--in_width", str(T), "--pretrained", "/nonexistent", "--out_dir", str(tmp / name)] + extra
    done = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert done.returncode == 0, done.stderr[-3000:] + done.stdout[-2000:]
    return done.stdout.splitlines()


def test_predict_scene_shapes_end_to_end_in_a_child_process(bcd_model, tmp_path):
    from PIL import Image
    from test_scene_bda_gpu import _scene
    tmp = tmp_path
    scene = _scene(HS, WS, 6)
    Image.fromarray(scene[:, :, 0:3]).save(tmp / "a.png")
    Image.fromarray(scene[:, :, 3:6]).save(tmp / "b.png")
    torch.save(bcd_model.state_dict(), tmp / "best_model.pth")
    sizes = ["--max_rings", str(HS * WS), "--max_vertices", str(4 * HS * WS), "--min_area", "4"]
    plain = _run(tmp, "plain", ["--objects", "--polygons"] + sizes)
    lines = _run(tmp, "shapes", ["--objects", "--polygons", "--shapes"] + sizes)
    assert [ln.replace(str(tmp / "shapes"), str(tmp / "plain")) for ln in lines[:-1]] == plain and lines[-1].startswith("shapes: objects = ")
    assert sorted(os.listdir(tmp / "plain" / "objects")) == ["scene.csv", "scene.geojson"]
    assert (tmp / "plain" / "objects" / "scene.csv").read_bytes() == (tmp / "shapes" / "objects" / "scene.csv").read_bytes()
    docs = {k: json.loads((tmp / "shapes" / "objects" / f"scene{k}.geojson").read_text()) for k in ("", ".hulls", ".rects")}
    before = json.loads((tmp / "plain" / "objects" / "scene.geojson").read_text())
    feats = docs[""]["features"]
    assert len(feats) == len(before["features"]) == len(docs[".hulls"]["features"]) == len(docs[".rects"]["features"]) >= 1
    names = ("hull_area", "hull_vertices", "solidity", "rect_area", "rect_long", "rect_short", "rect_angle", "rectangularity")
    sol, rec = [], []
    for f, b, fh, fr in zip(feats, before["features"], docs[".hulls"]["features"], docs[".rects"]["features"]):
        p = f["properties"]
        assert f["geometry"] == b["geometry"] and {k: v for k, v in p.items() if k not in names} == b["properties"]
        assert fh["properties"] == fr["properties"] == {k: p[k] for k in ("id", "area", "cls", "score")}
        pts = [tuple(v) for ring in f["geometry"]["coordinates"] for v in ring]
        h = R.hull(pts) if len(pts) < 300 else R.hull_fast(pts)
        row = R.rect(h)
        (hull_ring,), (rect_ring,) = fh["geometry"]["coordinates"], fr["geometry"]["coordinates"]
        assert [tuple(v) for v in hull_ring] == h + h[:1] and len(rect_ring) == 5 and rect_ring[0] == rect_ring[4]
        P, Q = h[row[0]], h[(row[0] + 1) % len(h)]
        corners, a, b_ = R.rect_corners(P, (Q[0] - P[0], Q[1] - P[1]), row)
        assert np.allclose(rect_ring[:4], corners, rtol=0, atol=1e-9)
        for q in h:                                          # every hull vertex inside the rectangle, within 1e-9 px
            for i in range(4):
                (ax, ay), (bx, by) = rect_ring[i], rect_ring[i + 1]
                side = ((bx - ax) ** 2 + (by - ay) ** 2) ** 0.5
                assert ((bx - ax) * (q[1] - ay) - (by - ay) * (q[0] - ax)) / side >= -1e-9
        hull_area, rect_area = R.shoelace2(h) / 2, (row[3] - row[2]) * row[4] / row[1]
        assert p["hull_area"] == hull_area and p["hull_vertices"] == len(h) and p["rect_area"] == round(rect_area, 4)
        assert p["solidity"] == round(p["area"] / hull_area, 4) <= 1 and p["rectangularity"] == round(p["area"] / rect_area, 4) <= 1
        assert p["rect_long"] == round(max(a, b_), 4) and p["rect_short"] == round(min(a, b_), 4) and 0 <= p["rect_angle"] < 180
        sol.append(p["solidity"])
        rec.append(p["rectangularity"])
    m = re.fullmatch(r"shapes: objects = (\d+) solidity_mean = ([\d.]+) rectangularity_mean = ([\d.]+)", lines[-1])
    assert m and int(m.group(1)) == len(feats)
    assert abs(float(m.group(2)) - np.mean(sol)) < 1e-4 and abs(float(m.group(3)) - np.mean(rec)) < 1e-4


def test_shapes_flag_needs_polygons(capsys):
    from change3d_amd.scripts.predict_scene import parse_args
    with pytest.raises(SystemExit):
        parse_args(["--weights", "w.pth", "--pre", "a.png", "--post", "b.png", "--objects", "--shapes"])
    assert "--shapes describes the polygons: it needs --polygons" in capsys.readouterr().err
    assert parse_args(["--weights", "w.pth", "--pre", "a.png", "--post", "b.png", "--objects", "--polygons", "--shapes"]).shapes
