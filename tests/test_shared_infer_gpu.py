"""`c3d_outlines_simplify_shared` in the layers above it: one 96 x 96 scene -- a noisy 20 x 20 mask of the survey, split into
pieces that share walls, beside one clean rectangle -- through `SceneInferencer.predict(simplify_shared=True)` and
`predict_scene --simplify_shared`.  The model is a stand-in that answers with the red channel of the first image, so the mask is
the one drawn here; everything after the model is the device pipeline."""
import json
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import shared_cases as SC  # noqa: E402
import shared_reference as R  # noqa: E402
import valid_cases as K  # noqa: E402

from change3d_amd import ops  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZE, T, TOL, SPLIT, SEED = 96, 64, 1.0, 1, 37


class _RedChannel(torch.nn.Module):
    """update_bcd = 1 where the first image's red channel is above the mean, else 0."""

    def __init__(self):
        super().__init__()
        self.args = SimpleNamespace(in_height=T, in_width=T, num_class=1)
        self.anchor = torch.nn.Parameter(torch.zeros(1))

    def update_bcd(self, pre, post):
        return (pre[:, 0:1] > 0).float()


def _scene():
    scene = np.zeros((SIZE, SIZE, 6), np.uint8)
    scene[4:24, 4:24, 0] = K.survey_mask(SEED) * 255
    scene[40:70, 50:85, 0] = 255
    return scene


def _inferencer():
    from change3d_amd.infer import SceneInferencer
    return SceneInferencer(_RedChannel().to(torch.device("cuda:0")), "bcd", stride=32, batch=8)


def _collapsed(row, raw_row):
    return row[1] < 0 or row[2] < 3 or row[3] == 0 or (row[3] > 0) != (raw_row[3] > 0)


@pytest.mark.gpu
def test_predict_with_simplify_shared_equals_the_ops_chained_by_hand():
    from change3d_amd.infer import SceneConflicts, SceneOutlines, SceneSharedOutlines, SceneValidity
    inf, scene = _inferencer(), _scene()
    kw = dict(objects=True, outlines=True, split=SPLIT, simplify=TOL, validity=True, conflicts=True, max_objects=64)
    runs = []
    for extra in ({}, dict(simplify_shared=False), dict(simplify_shared=True)):
        ops.trace_begin()                                    # the names of the launches, in order
        try:
            result = inf.predict(scene, **kw, **extra)
        finally:
            names = [n for n, _ in ops.trace_end()]
        runs.append((result, names))
    (today, names_today), (off, names_off), (out, names_on) = runs
    assert names_off == names_today and "c3d_outlines_simplify_shared" not in names_off, "simplify_shared=False is today's path"
    assert names_on == [n if n != "c3d_outlines_simplify" else "c3d_outlines_simplify_shared" for n in names_today]
    assert type(today[4]) is SceneOutlines and type(off[4]) is SceneOutlines and torch.equal(today[4].rings, off[4].rings)
    objects, raw, shared = out[2], out[3], out[4]
    assert isinstance(shared, SceneSharedOutlines) and shared._fields[:3] == SceneOutlines._fields and len(out) == len(today)
    assert isinstance(out[-3], SceneValidity) and isinstance(out[-1], SceneConflicts)
    want = ops.outlines_simplify_shared(objects.labels, objects.counts, *raw, TOL, max_objects=64)
    w = int(want[2][3])
    for a, b in zip(shared, want):
        assert torch.equal(a[:w], b[:w]) if a.dim() and a.shape[0] == want[1].shape[0] else torch.equal(a, b)
    host = R.simplify_shared(*(t.cpu().numpy() for t in (objects.labels, objects.counts, *raw)), R.tol2_q(TOL), max_objects=64)
    assert np.array_equal(shared.rings.cpu().numpy(), host["rings"]) and np.array_equal(shared.info.cpu().numpy(), host["info"])
    assert int(shared.info[4]) > 0 and int(shared.counts[4]) == 0
    valid = ops.rings_valid(*shared[:3], max_objects=64)
    conflict = ops.rings_conflicts(*shared[:3], max_objects=64)
    assert all(torch.equal(a, b) for a, b in zip(out[-3], valid)) and all(torch.equal(a, b) for a, b in zip(out[-1], conflict))
    assert int(out[-1].counts[1]) < int(today[-1].counts[1]), "fewer pieces in conflict than simplified ring by ring"
    with pytest.raises(ValueError):
        inf.predict(scene, objects=True, outlines=True, simplify_shared=True)


DRIVER = """
import sys
sys.path.insert(0, {tests!r})
import test_shared_infer_gpu as me
from change3d_amd.scripts import predict_scene
predict_scene.build_model = lambda args, device: me._RedChannel().to(device)
predict_scene.main(sys.argv[1:])
"""


@pytest.mark.gpu
def test_predict_scene_simplify_shared_in_a_child_process(tmp_path):
    from PIL import Image
    scene = _scene()
    Image.fromarray(scene[:, :, 0:3]).save(tmp_path / "a.png")
    Image.fromarray(scene[:, :, 3:6]).save(tmp_path / "b.png")
    argv = ["--task", "BCD", "--weights", "unused", "--pre", str(tmp_path / "a.png"), "--post", str(tmp_path / "b.png"), "--stride", "32",
            "--batch_size", "8", "--in_height", str(T), "--in_width", str(T), "--out_dir", str(tmp_path / "out"), "--objects",
            "--split_objects", str(SPLIT), "--polygons", "--simplify", str(TOL), "--simplify_shared", "--conflicts", "--simplify_check",
            "--shapes", "--validity", "--regularize"]          # every stage that takes the shared table
    done = subprocess.run([sys.executable, "-c", DRIVER.format(tests=os.path.dirname(os.path.abspath(__file__)))] + argv, cwd=ROOT,
                          capture_output=True, text=True, timeout=300)
    assert done.returncode == 0, done.stderr[-3000:] + done.stdout[-2000:]
    out = _inferencer().predict(scene, objects=True, outlines=True, split=SPLIT, simplify=TOL, simplify_shared=True, max_objects=65536)
    objects, raw, shared = out[2], out[3], out[4]
    info = [int(v) for v in shared.info.cpu().tolist()]
    lines = done.stdout.splitlines()
    assert (f"shared: tol = 1 objects = {int(objects.counts[1])} nodes = {info[1]} arcs = {info[2]} shared_arcs = {info[4]} "
            f"collapsed = {info[5]}") in lines
    assert any(ln.startswith("conflicts[simplified]:") for ln in lines) and any(ln.startswith("regularize:") for ln in lines) and info[5] > 0
    regular = json.loads((tmp_path / "out" / "objects" / "scene.regular.geojson").read_text())
    doc = json.loads((tmp_path / "out" / "objects" / "scene.geojson").read_text())
    rows_raw = raw.rings[:int(raw.counts[1])].cpu().tolist()
    rows = shared.rings[:int(raw.counts[1])].cpu().tolist()
    vertices, left = shared.vertices.cpu().tolist(), shared.left.cpu().tolist()
    assert len(doc["features"]) == int(objects.counts[1]) >= 3
    for f in doc["features"]:
        i = f["properties"]["id"]
        own = [(r, q) for r, q in zip(rows, rows_raw) if r[0] == i]
        kept = [(r, q) for r, q in own if not _collapsed(r, q)]
        assert f["properties"]["collapsed"] == (len(kept) < len(own))
        assert f["properties"]["neighbours"] == sorted({v for r, _ in own if r[1] >= 0 for v in left[r[1]:r[1] + r[2]] if v > 0})
        if any(q[3] > 0 and _collapsed(r, q) for r, q in own):
            assert f["geometry"] is None
            continue
        kept.sort(key=lambda rq: rq[1][3] <= 0)             # the outline first
        assert [ring[:-1] for ring in f["geometry"]["coordinates"]] == [vertices[r[1]:r[1] + r[2]] for r, _ in kept]
        assert f["properties"]["vertices"] == sum(r[2] for r, _ in kept)
    assert any(f["properties"]["collapsed"] for f in doc["features"]) and any(f["properties"]["neighbours"] for f in doc["features"])
    assert [(f["properties"]["id"], f["geometry"] is None) for f in regular["features"]] == \
           [(f["properties"]["id"], f["geometry"] is None) for f in doc["features"]]
    assert any(f["properties"]["regular"] for f in regular["features"])


def _feature_collection(name, tol):
    """polygons_geojson on the restatement's result of a hand-made map."""
    from change3d_amd.scripts.predict_scene import polygons_geojson
    c = SC.hand_made()[name]
    rings, vertices, counts = SC.table(c)
    out = R.simplify_shared(c["labels"], c["counts_obj"], rings, vertices, counts, R.tol2_q(tol))
    n = int(counts[1])
    table = np.zeros((int(c["labels"].max()), 8), dtype=np.int64)
    for i in range(len(table)):
        table[i, 0] = int((c["labels"] == i + 1).sum())
    w = int(out["counts"][3])
    return polygons_geojson(table, rings[:n], vertices[:int(counts[3])], (out["rings"][:n], out["vertices"][:w]), shared=out["left"][:w])[0]


def test_a_collapsed_outline_is_written_with_a_null_geometry():
    doc = _feature_collection("collapse", 2.0)
    by_id = {f["properties"]["id"]: f for f in doc["features"]}
    assert by_id[2]["geometry"] is None and by_id[2]["properties"]["collapsed"] and by_id[2]["properties"]["neighbours"] == [1]
    assert by_id[1]["geometry"] is not None and not by_id[1]["properties"]["collapsed"] and by_id[1]["properties"]["neighbours"] == [2]
    doc = _feature_collection("collapse", 0.0)
    assert all(f["geometry"] is not None and not f["properties"]["collapsed"] for f in doc["features"])
    doc = _feature_collection("island", 2.0)
    by_id = {f["properties"]["id"]: f for f in doc["features"]}
    assert by_id[1]["properties"]["neighbours"] == [2] and by_id[2]["properties"]["neighbours"] == [1]
    assert len(by_id[1]["geometry"]["coordinates"]) == 2
    assert by_id[1]["geometry"]["coordinates"][1][0] == by_id[2]["geometry"]["coordinates"][0][0]


def test_the_parser_refuses_the_fall_backs(capsys):
    from change3d_amd.scripts.predict_scene import parse_args
    common = ["--weights", "w.pth", "--pre", "a.png", "--post", "b.png", "--objects", "--polygons"]
    for extra in (["--simplify_shared"], ["--simplify", "1", "--simplify_shared", "--simplify_min_iou", "0.5"],
                  ["--simplify", "1", "--simplify_shared", "--simplify_valid"], ["--simplify", "1", "--simplify_shared", "--simplify_clean"]):
        with pytest.raises(SystemExit):
            parse_args(common + extra)
        capsys.readouterr()
    args = parse_args(common + ["--simplify", "1", "--simplify_shared", "--regularize", "--simplify_check", "--conflicts"])
    assert args.simplify_shared and args.regularize and not args.simplify_clean
    assert not parse_args(common + ["--simplify", "1"]).simplify_shared
