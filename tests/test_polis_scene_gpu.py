"""`c3d_rings_polis` in the layers above it: one 96 x 96 scene of four rotated rectangles taken through the device pipeline
(objects, outlines, simplify, hull, regularise; the true rectangles filled and matched) and scored at its three stages against
the restatement, `PolygonEvaluator` over two scenes with one read-back, and `predict_scene --polygon_scores` in child processes
on a synthetic 300 x 280 pair: its CSV and its closing lines against the ops chained by hand, and every other file and line
unchanged by the flag."""
import filecmp
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import polis_cases as K  # noqa: E402
import polis_reference as R  # noqa: E402
import regular_cases as RK  # noqa: E402
from fill_reference import table as make_table  # noqa: E402

from change3d_amd import ops, vector_labels  # noqa: E402
from change3d_amd.polygon_metrics import PolygonEvaluator, scores_from_totals  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HS, WS = 300, 280
U = 2.0 ** -53
STAGES = ("raw", "simplified", "regularised")


def _rectangles(flip=False):
    """(mask u8 [96, 96] of four rotated rectangles of 24 x 14 px, one per quadrant; the ring table of the true ones at 1/16 px)."""
    mask = np.zeros((96, 96), np.uint8)
    truth = []
    for k, d in enumerate(K.DIRECTIONS[::-1] if flip else K.DIRECTIONS):
        y0, x0 = 48 * (k // 2), 48 * (k % 2)
        mask[y0:y0 + 48, x0:x0 + 48] = RK.rotated_rectangle(d, long_px=24, short_px=14, size=48)
        truth.append(K.true_rectangle(d, long_px=24, short_px=14, f=4, centre=(x0 + 24, y0 + 24)))
    return mask, make_table(truth, max_rings=6, max_vertices=20)


def _device_stages(mask, truth):
    """[(stage, (rings, vertices, counts), frac_bits)] of the mask, the truth's device tables, and match_p: all on the device."""
    m = torch.from_numpy(mask).to(DEV)
    labels, table, _, _, counts = ops.scene_objects(m, connectivity=8, max_objects=16)
    raw = ops.scene_outlines(labels, counts, connectivity=8, max_objects=16, max_rings=32, max_vertices=2048)
    simple = ops.outlines_simplify(*raw, 1.0)
    hull = ops.rings_hull(*raw, max_objects=16)
    regular = ops.rings_regularize(*simple, *hull, frac_bits=4)
    gt = [torch.from_numpy(a).to(DEV) for a in truth]
    labels_g, table_g, counts_g, _, _, info = ops.rings_fill(*gt, 96, 96, frac_bits=4, max_objects=8)
    match_p = ops.objects_match(labels, table, counts, labels_g, table_g, counts_g)[0]
    assert int(info[0]) == 0 and int(raw[2][4]) == 0 and int(regular[2][4]) == 0
    return [("raw", raw, 0), ("simplified", simple, 0), ("regularised", regular, 4)], gt, match_p


def _close(got, want, bound):
    assert np.array_equal(got[want == 0], want[want == 0])
    assert (np.abs(got - want) <= bound * np.abs(want)).all(), (np.abs(got - want) / np.maximum(np.abs(want), 1e-300) / U).max()


def test_the_three_stages_of_a_scene_of_rotated_rectangles_against_the_restatement():
    mask, truth = _rectangles()
    stages, gt, match_p = _device_stages(mask, truth)
    match = match_p.cpu().numpy()
    assert sorted(match[:4, 0].tolist()) == [1, 2, 3, 4], "every rectangle found its true one"
    for stage, rings, f in stages:
        pair, pair_n, counts, sums = (t.cpu().numpy() for t in ops.rings_polis(*rings, f, *gt, 4, match_p, 8))
        want = R.polis(tuple(t.cpu().numpy() for t in rings), f, truth, 4, match, 8)
        assert np.array_equal(pair_n, want["pair_n"]) and np.array_equal(counts, want["counts"]) and counts[:4].tolist() == [4, 0, 0, 0]
        _close(pair, want["pair"], R.bounds(want["pair_n"]))
        _close(sums[[0, 1, 3]], want["sums"][[0, 1, 3]], (float((pair_n[:, 1] + pair_n[:, 2]).max()) + 20) * U)
        assert sums[2] == pair[:, 1].max() and (pair_n[:4, 2] == 4).all() and (pair[:4, 0] < 1.0).all()
        print(f"{stage}: n = {pair_n[:4, 1].tolist()} polis = {np.round(pair[:4, 0], 3).tolist()} hausdorff = {np.round(pair[:4, 1], 3).tolist()}")


def test_polygon_evaluator_over_two_scenes_with_one_read_back():
    evaluator = PolygonEvaluator(device=DEV)
    per_scene = []
    for flip in (False, True):
        mask, truth = _rectangles(flip)
        stages, gt, match_p = _device_stages(mask, truth)
        _, rings, f = stages[2]
        out = evaluator.update(*rings, f, *gt, 4, match_p, 8)
        per_scene.append([t.clone() for t in out])
    s = evaluator.scores()
    counts = sum(c[2].cpu().numpy() for c in per_scene)
    sums = [c[3].cpu().numpy() for c in per_scene]
    want = scores_from_totals(counts, [sums[0][0] + sums[1][0], sums[0][1] + sums[1][1], max(sums[0][2], sums[1][2]), sums[0][3] + sums[1][3]])
    assert s == want and s["pairs"] == 8 and s["n_ratio"] == 1.0 and evaluator.scenes == 2 and 0 < s["polis"] < s["hausdorff_mean"] <= s["hausdorff_max"]
    evaluator.reset()
    assert evaluator.scores()["pairs"] == 0


@pytest.fixture(scope="module")
def bcd_model():
    from test_scene_bda_gpu import _model
    return _model("bcd")


@pytest.fixture(scope="module")
def scene_dir(bcd_model, tmp_path_factory):
    """The pair, the weights and a polygon label file: the outlines of 40 of the model's own objects, so that they match."""
    from PIL import Image
    from change3d_amd.infer import SceneInferencer
    from change3d_amd.scripts.predict_scene import polygons_geojson
    from test_scene_bda_gpu import _scene
    tmp = tmp_path_factory.mktemp("polis_scene")
    scene = _scene(HS, WS, 6)
    Image.fromarray(scene[:, :, 0:3]).save(tmp / "a.png")
    Image.fromarray(scene[:, :, 3:6]).save(tmp / "b.png")
    torch.save(bcd_model.state_dict(), tmp / "best_model.pth")
    out = SceneInferencer(bcd_model, "bcd", stride=32, batch=32).predict(scene, objects=True, outlines=True,
                                                                         max_rings=HS * WS, max_vertices=4 * HS * WS)
    rows, ring_rows, written = int(out[2].counts[1]), int(out[3].counts[1]), int(out[3].counts[3])
    doc, skipped = polygons_geojson(out[2].table[:rows].cpu().numpy(), out[3].rings[:ring_rows].cpu().numpy(), out[3].vertices[:written].cpu().numpy())
    assert not skipped and len(doc["features"]) >= 5
    doc["features"] = doc["features"][:40]
    (tmp / "gt.geojson").write_text(json.dumps(doc))
    return tmp


def _run(tmp, name, extra):
    from test_scene_bda_gpu import T
    cmd = [sys.executable, "-m", "change3d_amd.scripts.predict_scene", "--task", "BCD", "--weights", str(tmp / "best_model.pth"), "--pre",
           str(tmp / "a.png"), "--post", str(tmp / "b.png"), "--stride", "32", "--batch_size", "32", "--act_dtype", "f32", "--in_height", str(T),
           "--in_width", str(T), "--pretrained", "/nonexistent", "--out_dir", str(tmp / name), "--objects", "--polygons",
           "--simplify", "1.0", "--regularize", "--label_polygons", str(tmp / "gt.geojson")] + extra
    done = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert done.returncode == 0, done.stderr[-3000:] + done.stdout[-2000:]
    return done.stdout.splitlines()


def test_predict_scene_polygon_scores_in_child_processes(bcd_model, scene_dir):
    from change3d_amd.infer import SceneInferencer
    from change3d_amd.object_metrics import ObjectEvaluator
    from test_scene_bda_gpu import _scene
    tmp = scene_dir
    with_flag = _run(tmp, "with", ["--polygon_scores"])
    without = _run(tmp, "without", [])
    # without the flag nothing moves: the same lines but the closing ones, the same files but the CSV, byte for byte
    closing = [ln for ln in with_flag if ln.startswith("polygons[")]
    assert [ln.split(":")[0] for ln in closing] == [f"polygons[{s}]" for s in STAGES] and with_flag[-3:] == closing
    strip = lambda lines: [ln.replace(str(tmp / "without"), "").replace(str(tmp / "with"), "") for ln in lines]   # noqa: E731
    assert strip(with_flag[:-3]) == strip(without) and not [ln for ln in without if "polygons[" in ln]
    assert with_flag.index(closing[0]) > [k for k, ln in enumerate(with_flag) if ln.startswith("objects:")][0]
    cmp = filecmp.dircmp(tmp / "with" / "objects", tmp / "without" / "objects")
    assert cmp.left_only == ["scene.polis.csv"] and not cmp.right_only
    match, mismatch, errors = filecmp.cmpfiles(tmp / "with" / "objects", tmp / "without" / "objects", cmp.common_files, shallow=False)
    assert not mismatch and not errors and "scene.regular.geojson" in match
    assert filecmp.cmp(tmp / "with" / "scene.png", tmp / "without" / "scene.png", shallow=False)
    # the ops chained by hand
    out = SceneInferencer(bcd_model, "bcd", stride=32, batch=32).predict(_scene(HS, WS, 6), objects=True, outlines=True,
                                                                         simplify=1.0, regularize=True)
    objects, raw, simple, regular = out[2], out[3], out[4], out[5]
    rings, vertices, counts, id_cls = vector_labels.read_polygons(str(tmp / "gt.geojson"), 4)
    gt = [torch.from_numpy(a).to(DEV) for a in (rings, vertices, counts)]
    n = len(id_cls)
    labels_g, table_g, counts_g, _, _, info = ops.rings_fill(*gt, HS, WS, frac_bits=4, max_objects=n)
    match_p, _ = ObjectEvaluator(device=DEV).update_labeled(objects, labels_g, table_g, counts_g)
    rows = int(objects.counts[1])
    csv = (tmp / "with" / "objects" / "scene.polis.csv").read_text().splitlines()
    assert csv[0] == "stage,id,gt_id,n,n_gt,polis,hausdorff,flag" and len(csv) == 1 + 3 * rows
    at = 1
    for stage, table, f, line in zip(STAGES, (raw, simple, regular), (0, 0, 4), closing):
        evaluator = PolygonEvaluator(device=DEV)
        pair, pair_n, _, _ = evaluator.update(table.rings, table.vertices, table.counts, f, *gt, 4, match_p, n)
        s = evaluator.scores()
        assert line == (f"polygons[{stage}]: pairs = {s['pairs']} polis = {s['polis']:.4f} hausdorff_mean = {s['hausdorff_mean']:.4f} "
                        f"hausdorff_max = {s['hausdorff_max']:.4f} n_ratio = {s['n_ratio']:.4f} skipped = {s['incomplete'] + s['over_work']}")
        want = [f"{stage},{k + 1},{g},{n_p},{n_g},{p[0]:.4f},{p[1]:.4f},{flag}"
                for k, (p, (g, n_p, n_g, flag)) in enumerate(zip(pair[:rows].cpu().tolist(), pair_n[:rows].cpu().tolist()))]
        assert csv[at:at + rows] == want
        at += rows
        assert s["pairs"] >= 5 and s["incomplete"] == 0 and s["over_work"] <= 1   # the scene-filling object of this noise may pass the cap
        if stage == "raw":                                   # the labels are the raw polygons of these very objects
            assert s["polis"] == 0.0 and s["hausdorff_max"] == 0.0 and s["n_ratio"] == 1.0
        else:
            assert 0.0 < s["polis"] < 2.0 and s["n_ratio"] < 1.0


def test_the_parser_refuses_the_flag_without_its_inputs():
    from change3d_amd.scripts.predict_scene import parse_args
    base = ["--weights", "w", "--polygon_scores"]
    for extra in ([], ["--objects", "--polygons"], ["--label_polygons", "x", "--objects"]):
        with pytest.raises(SystemExit):
            parse_args(base + extra)
    assert parse_args(base + ["--objects", "--polygons", "--label_polygons", "x"]).polygon_scores
