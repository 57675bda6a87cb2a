"""`c3d_scene_regions` and `c3d_regions_sieve` in the layers above them: `SceneInferencer.predict(objects=True, regions=..)` for
SCD with a pixelwise stub model (the pattern of tests/test_split_infer_gpu.py) against the ops applied to the class maps it
returns, the region labels through the tracer, the fill and the crossing-free simplifier on the device, and `predict_scene
--regions`.  The argument refusals need no GPU.

The scene is drawn so that the stub answers two noisy class maps: pre G = 40 x the pre class, post G = 40 x the post class,
pre R = 255 where something changed."""
import json
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import regions_cases as RC  # noqa: E402
import regions_reference as R  # noqa: E402

from change3d_amd import _lib as L  # noqa: E402
from change3d_amd import ops  # noqa: E402
from change3d_amd.data.transforms import BCDTransforms as BT  # noqa: E402
from change3d_amd.infer import SceneInferencer, SceneObjects, SceneRegionObjects, region_classes  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T, HS, WS, NUM_CLASS, SIEVE = 64, 80, 110, 7, 6
MODES = ("pre", "post", "transition")


class Stub(torch.nn.Module):
    """update_scd, per pixel: the class heads answer -(normalised G - the class's centre)^2 with the centre of class c at
    G = 40 c, the change head sigmoid(4 x normalised pre R)."""

    def __init__(self):
        super().__init__()
        self.args = SimpleNamespace(in_height=T, in_width=T, num_class=NUM_CLASS)
        mean, std = BT.DEFAULT_MEAN, BT.DEFAULT_STD
        self.centres = torch.nn.Parameter(torch.tensor([[(40.0 * c / 255.0 - mean[g]) / std[g] for c in range(NUM_CLASS)]
                                                        for g in (1, 4 if len(mean) >= 6 else 1)], dtype=torch.float32))

    def update_scd(self, pre, post):
        logits = lambda x, side: -(x[:, 1:2] - self.centres[side].view(1, NUM_CLASS, 1, 1)) ** 2  # noqa: E731
        return logits(pre, 0), logits(post, 1), torch.sigmoid(4.0 * pre[:, 0:1])


def _scene():
    pre = RC.block_noise(HS, WS, NUM_CLASS, seed=21, block=8, noise=0.12)
    post = RC.block_noise(HS, WS, NUM_CLASS, seed=22, block=8, noise=0.12)
    change = (RC.block_noise(HS, WS, 3, seed=23, block=16, noise=0.02) > 0).astype(np.uint8)
    scene = np.random.default_rng(3).integers(0, 30, size=(HS, WS, 6), dtype=np.uint8)
    scene[..., 0] = change * 255
    scene[..., 1] = pre * 40
    scene[..., 4] = post * 40
    return scene, pre * change, post * change, change


def _inferencer(device="cuda:0"):
    return SceneInferencer(Stub().to(torch.device(device)), "scd", stride=32, batch=5)


def _key(out, mode):
    pre, post = out[0], out[1]
    return {"pre": pre, "post": post, "transition": (pre.to(torch.int16) * NUM_CLASS + post).to(torch.uint8)}[mode]


@pytest.mark.gpu
@pytest.mark.parametrize("sieve", [None, SIEVE])
@pytest.mark.parametrize("mode", MODES)
def test_predict_regions_equal_the_ops_on_the_returned_class_maps(mode, sieve):
    scene, pre, post, change = _scene()
    inf = _inferencer()
    plain = inf.predict(scene)
    assert np.array_equal(plain[0].cpu().numpy(), pre) and np.array_equal(plain[1].cpu().numpy(), post)   # the stub answers the drawing
    for connectivity in (4, 8):
        out = inf.predict(scene, objects=True, regions=mode, sieve=sieve, connectivity=connectivity, max_objects=4096)
        assert len(out) == len(plain) + 1 and all(torch.equal(a, b) for a, b in zip(plain, out))
        found = out[-1]
        assert isinstance(found, SceneRegionObjects) and isinstance(found, SceneObjects) and len(found) == 5 and found.hist is None
        key = _key(out, mode)
        assert len(torch.unique(key)) > 4
        if sieve is None:
            labels, table, _, object_key, counts = ops.scene_regions(key, connectivity=connectivity, max_objects=4096)
            assert torch.equal(found.key_map, key) and found.info.tolist() == [0] * 8
            want = R.region_objects(key.cpu().numpy(), connectivity=connectivity, max_objects=4096)
            assert np.array_equal(found.labels.cpu().numpy(), want["labels"]) and np.array_equal(found.table.cpu().numpy(), want["table"])
        else:
            labels, table, _, object_key, counts, info = ops.regions_sieve(key, sieve, connectivity=connectivity, max_objects=4096)
            assert torch.equal(found.key_map, object_key) and torch.equal(found.info, info)
            assert int(info[0]) == 0 and int(info[1]) >= 1 and int(info[4]) == 0
            assert int(found.table[:int(counts[1]), 0].min()) >= sieve
        assert torch.equal(found.labels, labels) and torch.equal(found.table, table) and torch.equal(found.counts, counts)
        assert torch.equal(found.object_cls, object_key)
        rows = int(counts[1])
        assert 10 < rows == int(counts[0]) and torch.equal(found.table[:rows, 5].cpu(), found.key_map.ravel()[found.table[:rows, 6].long()].cpu().int())
    dropped = inf.predict(scene, objects=True, regions=mode, sieve=sieve, min_area=60, max_objects=4096)[-1]   # above the sieve
    assert int(dropped.table[:int(dropped.counts[1]), 0].min()) >= 60 and int(dropped.counts[0]) < rows     # min_area still drops
    assert torch.equal(dropped.object_cls, torch.where(dropped.labels > 0, dropped.key_map, torch.zeros_like(dropped.key_map)))


@pytest.mark.gpu
def test_regions_none_is_the_call_without_the_argument():
    scene = _scene()[0]
    inf = _inferencer()
    inf.predict(scene, objects=True, outlines=True)                          # the tables and windows are uploaded
    runs = []
    for extra in ({}, dict(regions=None, sieve=None, sieve_rounds=None)):
        ops.trace_begin()
        try:
            result = inf.predict(scene, objects=True, outlines=True, min_area=2, **extra)
        finally:
            names = [n for n, _ in ops.trace_end()]
        runs.append((result, names))
    (a, names_a), (b, names_b) = runs
    assert names_a == names_b and "c3d_scene_regions" not in names_a and "c3d_scene_objects" in names_a
    assert len(a) == len(b) and type(a[3]) is type(b[3]) is SceneObjects
    assert all(torch.equal(x, y) for x, y in zip(a[:3], b[:3])) and torch.equal(a[3].labels, b[3].labels) and torch.equal(a[3].table, b[3].table)
    assert torch.equal(a[4].rings, b[4].rings) and torch.equal(a[4].counts, b[4].counts)


def test_the_argument_refusals_need_no_gpu():
    scene = _scene()[0]
    inf = _inferencer("cpu")
    for bad in (dict(objects=True, regions="both"), dict(regions="pre"), dict(objects=True, regions="pre", split=3),
                dict(objects=True, sieve=4), dict(objects=True, regions="pre", sieve_rounds=3), dict(objects=True, regions="pre", sieve=0),
                dict(objects=True, regions="pre", sieve=4, sieve_rounds=0), dict(objects=True, regions="post", sieve=2 ** 20 + 1)):
        with pytest.raises(ValueError):
            inf.predict(scene, **bad)
    wide = _inferencer("cpu")
    wide.num_class = 17
    with pytest.raises(ValueError, match="16"):
        wide.predict(scene, objects=True, regions="transition")
    bcd = SceneInferencer(Stub(), "scd", stride=32, batch=5)
    bcd.task = "bcd"
    with pytest.raises(ValueError, match="SCD"):
        bcd.predict(scene, objects=True, regions="pre")
    assert region_classes(23, "transition", 7) == (3, 2) and region_classes(5, "pre", 7) == (5, 0) and region_classes(5, "post", 7) == (0, 5)


@pytest.mark.gpu
@pytest.mark.parametrize("connectivity", [4, 8])
def test_the_region_labels_go_through_the_tracer_the_fill_and_the_safe_simplifier(connectivity):
    scene = _scene()[0]
    inf = _inferencer()
    kw = dict(objects=True, regions="transition", connectivity=connectivity, max_objects=4096, outlines=True, max_rings=HS * WS,
              max_vertices=4 * HS * WS)
    for sieve in (None, SIEVE):
        out = inf.predict(scene, sieve=sieve, simplify=1.0, simplify_shared=True, simplify_safe=True, conflicts=True, **kw)
        found, raw, safe = out[3], out[4], out[5]
        assert isinstance(found, SceneRegionObjects) and int(raw.counts[4]) == 0
        back = ops.rings_fill(*raw, HS, WS, max_objects=4096)
        assert torch.equal(back[0], found.labels), "fill(trace(labels)) == labels"
        assert int(safe.safe[7]) == 0, safe.safe                             # converged
        for conflicts in out[-2:]:                                           # of the raw rings, of the simplified ones
            assert int(conflicts.conflict[:, 3].sum()) == 0 and int(conflicts.conflict[:, 4].sum()) == 0     # no cross, no same


DRIVER = """
import sys
sys.path.insert(0, {tests!r})
import test_regions_infer_gpu as me
from change3d_amd.scripts import predict_scene
predict_scene.build_model = lambda args, device: me.Stub().to(device)
predict_scene.main(sys.argv[1:])
"""


@pytest.mark.gpu
def test_predict_scene_regions_in_a_child_process(tmp_path):
    from PIL import Image
    scene, pre, post, change = _scene()
    Image.fromarray(scene[:, :, 0:3]).save(tmp_path / "a.png")
    Image.fromarray(scene[:, :, 3:6]).save(tmp_path / "b.png")
    for name, m in (("l1", pre), ("l2", post), ("ch", change)):          # 0 / 1: the SCD label side multiplies by it
        Image.fromarray(m).save(tmp_path / f"{name}.png")
    base = ["--task", "SCD", "--weights", "unused", "--pre", str(tmp_path / "a.png"), "--post", str(tmp_path / "b.png"), "--stride", "32",
            "--batch_size", "5", "--in_height", str(T), "--in_width", str(T), "--objects"]
    driver = DRIVER.format(tests=os.path.dirname(os.path.abspath(__file__)))

    def run(out_dir, extra):
        return subprocess.run([sys.executable, "-c", driver] + base + ["--out_dir", str(tmp_path / out_dir)] + extra, cwd=ROOT,
                              capture_output=True, text=True, timeout=300)

    done = run("regions", ["--regions", "transition", "--sieve", str(SIEVE), "--polygons", "--label1", str(tmp_path / "l1.png"),
                           "--label2", str(tmp_path / "l2.png"), "--change", str(tmp_path / "ch.png")])
    assert done.returncode == 0, done.stderr[-3000:] + done.stdout[-2000:]
    found = _inferencer().predict(scene, objects=True, regions="transition", sieve=SIEVE)[-1]
    rows, info = int(found.counts[1]), found.info.tolist()
    assert f"regions: mode = transition objects = {rows} moved = {info[2]} pixels = {info[3]} rounds = {info[1]}" in done.stdout.splitlines()
    lines = (tmp_path / "regions" / "objects" / "scene.csv").read_text().splitlines()
    assert lines[0] == "id,area,x0,y0,x1,y1,cls,score,from,to" and len(lines) == rows + 1
    table = found.table[:rows].cpu().tolist()
    for line, row in zip(lines[1:], table):
        cells = line.split(",")
        assert int(cells[6]) == row[5] and (int(cells[8]), int(cells[9])) == divmod(row[5], NUM_CLASS) and int(cells[1]) == row[0]
    doc = json.loads((tmp_path / "regions" / "objects" / "scene.geojson").read_text())
    assert len(doc["features"]) == rows
    for f in doc["features"]:
        p = f["properties"]
        assert (p["from"], p["to"]) == divmod(p["cls"], NUM_CLASS) and p["cls"] == table[p["id"] - 1][5]
    key = found.key_map.cpu().numpy()
    for side, want in zip(("from", "to"), divmod(key, NUM_CLASS)):
        assert np.array_equal(np.asarray(Image.open(tmp_path / "regions" / "regions" / f"scene.{side}.png")), want)
    assert (tmp_path / "regions" / "objects" / "scene.match.csv").exists()       # the labelled regions were joined and scored

    # without --regions: the files and lines of the components of the change mask, in the format they always had
    plain = run("plain", [])
    assert plain.returncode == 0, plain.stderr[-3000:]
    assert not any(ln.startswith("regions:") for ln in plain.stdout.splitlines()) and not (tmp_path / "plain" / "regions").exists()
    objects = _inferencer().predict(scene, objects=True)[-1]
    want = "id,area,x0,y0,x1,y1,cls,score\n" + "".join(
        f"{k + 1},{a},{x0},{y0},{x1},{y1},{c},{q / 65535:.4f}\n"
        for k, (a, x0, y0, x1, y1, c, _, q) in enumerate(objects.table[:int(objects.counts[1])].cpu().tolist()))
    assert (tmp_path / "plain" / "objects" / "scene.csv").read_text() == want
    assert sorted(os.listdir(tmp_path / "plain")) == ["change", "objects", "pred1", "pred2"]

    # one round where the scene needs more: the run would end with an error that names the flag
    from change3d_amd.scripts.predict_scene import check_sieve
    short = _inferencer().predict(scene, objects=True, regions="transition", sieve=SIEVE, connectivity=4, sieve_rounds=1)[-1]
    assert int(short.info[0]) == L.SIEVE_ST_NOT_CONVERGED and int(found.info[0]) == 0
    with pytest.raises(SystemExit, match="--sieve_rounds"):
        check_sieve("scene", short, 1)
    check_sieve("scene", found, 8)
