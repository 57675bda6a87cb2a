"""`c3d_outlines_simplify_safe` in the layers above it: one 64 x 64 scene -- a noisy 20 x 20 mask of the survey, split into pieces
that share walls, beside one clean rectangle -- through `SceneInferencer.predict(simplify_safe=True)` and `predict_scene
--simplify_safe`.  The model is a stand-in that answers with the red channel of the first image, so the mask is the one drawn
here; everything after the model is the device pipeline.  The argument refusals need no GPU."""
import json
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import safe_reference as S  # noqa: E402
import shared_reference as R  # noqa: E402
import valid_cases as K  # noqa: E402

from change3d_amd import ops  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZE, T, TOL, SPLIT, SEED = 64, 64, 2.0, 1, 37


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
    scene[34:58, 30:60, 0] = 255
    return scene


def _inferencer(device="cuda:0"):
    from change3d_amd.infer import SceneInferencer
    return SceneInferencer(_RedChannel().to(torch.device(device)), "bcd", stride=32, batch=8)


@pytest.mark.gpu
def test_predict_with_simplify_safe_equals_the_ops_chained_by_hand():
    from change3d_amd.infer import SceneConflicts, SceneSafeOutlines, SceneSharedOutlines, SceneValidity
    inf, scene = _inferencer(), _scene()
    kw = dict(objects=True, outlines=True, split=SPLIT, simplify=TOL, simplify_shared=True, validity=True, conflicts=True, max_objects=64)
    runs = []
    for extra in ({}, dict(simplify_safe=False), dict(simplify_safe=True), dict(simplify_safe=True, safe_rounds=2)):
        ops.trace_begin()                                    # the names of the launches, in order
        try:
            result = inf.predict(scene, **kw, **extra)
        finally:
            names = [n for n, _ in ops.trace_end()]
        runs.append((result, names))
    (today, names_today), (off, names_off), (out, names_on), (short, _) = runs
    assert names_off == names_today and "c3d_outlines_simplify_safe" not in names_off, "simplify_safe=False is today's path"
    assert names_on == [n if n != "c3d_outlines_simplify_shared" else "c3d_outlines_simplify_safe" for n in names_today]
    assert type(today[4]) is SceneSharedOutlines and type(off[4]) is SceneSharedOutlines and torch.equal(today[4].rings, off[4].rings)
    objects, raw, safe = out[2], out[3], out[4]
    assert isinstance(safe, SceneSafeOutlines) and isinstance(safe, SceneSharedOutlines) and len(safe) == 5 and len(out) == len(today)
    assert isinstance(out[-3], SceneValidity) and isinstance(out[-1], SceneConflicts)
    want = ops.outlines_simplify_safe(objects.labels, objects.counts, *raw, TOL, max_objects=64)
    w = int(want[2][3])
    for a, b in zip(tuple(safe) + (safe.level, safe.safe), want):
        assert torch.equal(a[:w], b[:w]) if a.dim() and a.shape[0] == want[1].shape[0] else torch.equal(a, b)
    host = S.simplify_safe(*(t.cpu().numpy() for t in (objects.labels, objects.counts, *raw)), R.tol2_q(TOL), max_objects=64, fast=True,
                           limits=ops.outlines_simplify_safe_limits()[4:6])
    assert np.array_equal(safe.rings.cpu().numpy(), host["rings"]) and np.array_equal(safe.safe.cpu().numpy(), host["safe"])
    assert np.array_equal(safe.info.cpu().numpy(), host["info"])
    assert int(safe.safe[7]) == 0 and int(safe.safe[1]) >= 1 and int(safe.safe[4]) > 0 and int(safe.info[5]) == 0
    valid = ops.rings_valid(*safe[:3], max_objects=64)
    conflict = ops.rings_conflicts(*safe[:3], max_objects=64)
    assert all(torch.equal(a, b) for a, b in zip(out[-3], valid)) and all(torch.equal(a, b) for a, b in zip(out[-1], conflict))
    assert int(today[-1].counts[1]) > 0 and int(out[-1].counts[1]) == 0, "the shared rule leaves pieces in conflict, the safe one none"
    assert int(out[-3].counts[1]) == 0 and not out[-3].valid[:, 7].any() and not out[-1].conflict[:, 7].any()
    assert int(short[4].safe[0]) == min(2, int(safe.safe[0]))


def test_the_argument_refusals_need_no_gpu():
    inf, scene = _inferencer("cpu"), _scene()
    kw = dict(objects=True, outlines=True, simplify=TOL)
    for bad in (dict(simplify_safe=True), dict(simplify_shared=True, safe_rounds=3), dict(simplify_shared=True, simplify_safe=True, safe_rounds=0),
                dict(simplify_shared=True, simplify_safe=True, safe_rounds=65)):
        with pytest.raises(ValueError):
            inf.predict(scene, **kw, **bad)
    with pytest.raises(ValueError):
        inf.predict(scene, objects=True, outlines=True, simplify_shared=True, simplify_safe=True)


DRIVER = """
import sys
sys.path.insert(0, {tests!r})
import test_safe_infer_gpu as me
from change3d_amd.scripts import predict_scene
predict_scene.build_model = lambda args, device: me._RedChannel().to(device)
predict_scene.main(sys.argv[1:])
"""


@pytest.mark.gpu
def test_predict_scene_simplify_safe_in_a_child_process(tmp_path):
    from PIL import Image
    scene = _scene()
    Image.fromarray(scene[:, :, 0:3]).save(tmp_path / "a.png")
    Image.fromarray(scene[:, :, 3:6]).save(tmp_path / "b.png")
    argv = ["--task", "BCD", "--weights", "unused", "--pre", str(tmp_path / "a.png"), "--post", str(tmp_path / "b.png"), "--stride", "32",
            "--batch_size", "8", "--in_height", str(T), "--in_width", str(T), "--out_dir", str(tmp_path / "out"), "--objects",
            "--split_objects", str(SPLIT), "--polygons", "--simplify", str(TOL), "--simplify_safe", "--conflicts", "--validity"]
    driver = DRIVER.format(tests=os.path.dirname(os.path.abspath(__file__)))
    done = subprocess.run([sys.executable, "-c", driver] + argv, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert done.returncode == 0, done.stderr[-3000:] + done.stdout[-2000:]
    out = _inferencer().predict(scene, objects=True, outlines=True, split=SPLIT, simplify=TOL, simplify_shared=True, simplify_safe=True,
                                max_objects=65536)
    objects, raw, safe = out[2], out[3], out[4]
    rounds, raised, refined, at_cap, first, last, _, status = (int(v) for v in safe.safe.cpu().tolist())
    lines = done.stdout.splitlines()
    assert status == 0 and raised >= 1
    assert f"safe: tol = 2 rounds = {rounds} raised = {raised} arcs_refined = {refined} arcs_raw = {at_cap} defects = {first} -> 0" in lines
    assert any(ln.startswith("shared:") for ln in lines) and any(ln.startswith("conflicts[simplified]:") for ln in lines)
    doc = json.loads((tmp_path / "out" / "objects" / "scene.geojson").read_text())
    host = S.simplify_safe(*(t.cpu().numpy() for t in (objects.labels, objects.counts, *raw)), R.tol2_q(TOL), fast=True)
    per_id = {}
    for r, slots in host["slots"].items():                   # the arcs of every id above level 0, each ring's own arcs
        i = int(host["rings"][r, 0])
        per_id[i] = per_id.get(i, 0) + sum(1 for s in set(slots) if host["levels"].get(s, 0) > 0)
    assert len(doc["features"]) == int(objects.counts[1]) >= 3
    for f in doc["features"]:
        p = f["properties"]
        assert p["refined"] == per_id.get(p["id"], 0) and not p["collapsed"] and f["geometry"] is not None
        assert p["valid"] and p["conflicts"] == 0
    assert sum(f["properties"]["refined"] > 0 for f in doc["features"]) >= 2
    # one round is not enough for this scene: the run ends with an error that names the flag
    done = subprocess.run([sys.executable, "-c", driver] + argv + ["--safe_rounds", "1"], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert done.returncode != 0 and "--safe_rounds" in done.stderr + done.stdout


def test_the_parser_implies_simplify_shared_and_inherits_its_refusals(capsys):
    from change3d_amd.scripts.predict_scene import parse_args
    common = ["--weights", "w.pth", "--pre", "a.png", "--post", "b.png", "--objects", "--polygons"]
    for extra in (["--simplify_safe"], ["--simplify", "1", "--simplify_safe", "--simplify_min_iou", "0.5"],
                  ["--simplify", "1", "--simplify_safe", "--simplify_valid"], ["--simplify", "1", "--simplify_safe", "--simplify_clean"],
                  ["--simplify", "1", "--simplify_shared", "--safe_rounds", "4"], ["--simplify", "1", "--simplify_safe", "--safe_rounds", "0"],
                  ["--simplify", "1", "--simplify_safe", "--safe_rounds", "65"]):
        with pytest.raises(SystemExit):
            parse_args(common + extra)
        capsys.readouterr()
    args = parse_args(common + ["--simplify", "1", "--simplify_safe"])
    assert args.simplify_safe and args.simplify_shared and args.safe_rounds == 8
    assert parse_args(common + ["--simplify", "1", "--simplify_safe", "--safe_rounds", "12"]).safe_rounds == 12
    plain = parse_args(common + ["--simplify", "1", "--simplify_shared"])
    assert not plain.simplify_safe and plain.safe_rounds is None
