"""`c3d_rings_conflicts` in the layers above it: one 96 x 96 scene -- a noisy 20 x 20 mask of the survey, whose split pieces
conflict once simplified at 1 px, beside one clean rectangle -- through `SceneInferencer.predict(conflicts=True)` and
`predict_scene --conflicts --simplify_clean`.  The model is a stand-in that answers with the red channel of the first image, so
the mask is the one drawn here; everything after the model is the device pipeline."""
import json
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conflicts_cases as K  # noqa: E402
import conflicts_reference as R  # noqa: E402

from change3d_amd import ops  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SIZE, T, TOL, SPLIT, SEED = 96, 64, 1.0, 1, 37
CONFLICT_LAUNCHES = 14                                       # as include/change3d_hip.h documents them
KEYS = ("conflicts", "conflict_with", "shared_walls")


class _RedChannel(torch.nn.Module):
    """update_bcd = 1 where the first image's red channel is above the mean, else 0."""

    def __init__(self):
        super().__init__()
        self.args = SimpleNamespace(in_height=T, in_width=T, num_class=1)
        self.anchor = torch.nn.Parameter(torch.zeros(1))

    def update_bcd(self, pre, post):
        return (pre[:, 0:1] > 0).float()


def _mask():
    mask = np.zeros((SIZE, SIZE), np.uint8)
    mask[4:24, 4:24] = K.K.survey_mask(SEED)
    mask[40:70, 50:85] = 1
    return mask


def _scene():
    scene = np.zeros((SIZE, SIZE, 6), np.uint8)
    scene[:, :, 0] = _mask() * 255
    return scene


def _inferencer():
    from change3d_amd.infer import SceneInferencer
    return SceneInferencer(_RedChannel().to(DEV), "bcd", stride=32, batch=8)


def _same_but_spare_vertex_rows(a, b):
    assert len(a) == len(b)
    for p, q in zip(a, b):
        n = int(p.counts[3]) if hasattr(p, "vertices") else None
        for x, y in zip(*(t if isinstance(t, tuple) else (t,) for t in (p, q))):
            if x is None:
                assert y is None
            elif isinstance(x, tuple):
                assert all(torch.equal(u, v) for u, v in zip(x, y))
            elif n is not None and x.dim() == 2 and x.shape[-1] == 2:
                assert torch.equal(x[:n], y[:n])
            else:
                assert torch.equal(x, y)


def test_predict_with_conflicts_equals_the_restatement_on_its_own_rings():
    from change3d_amd.infer import SceneConflicts, SceneValidity
    inf, scene = _inferencer(), _scene()
    kw = dict(objects=True, outlines=True, split=SPLIT, simplify=TOL, regularize=True, validity=True, max_objects=64)
    today = inf.predict(scene, **kw)
    before = ops.launch_count()
    off = inf.predict(scene, conflicts=False, **kw)
    plain = ops.launch_count() - before
    before = ops.launch_count()
    out = inf.predict(scene, conflicts=True, **kw)
    assert ops.launch_count() - before == plain + 3 * CONFLICT_LAUNCHES
    assert torch.equal(out[1].cpu(), torch.from_numpy(_mask())), "the stand-in model draws the mask"
    assert len(out) == len(today) + 3 and all(isinstance(v, SceneConflicts) for v in out[-3:])
    assert all(isinstance(v, SceneValidity) for v in out[-6:-3]), "after the validity entries, last of all"
    _same_but_spare_vertex_rows(today, off)
    _same_but_spare_vertex_rows(today, out[:-3])
    raw, simple, regular = out[3], out[4], out[5]
    bad = {}
    for stage, table, f, got in (("raw", raw, 0, out[-3]), ("simplified", simple, 0, out[-2]), ("regular", regular, 4, out[-1])):
        want = R.conflicts(tuple(t.cpu().numpy() for t in table), f, 64)
        assert np.array_equal(got.conflict.cpu().numpy(), want["conflict"]), stage
        assert np.array_equal(got.counts.cpu().numpy(), want["counts"]), stage
        assert all(int(got.info[k]) == want["info"][k] for k in R.FIXED_INFO), stage
        bad[stage] = int(want["counts"][1])
        assert want["counts"][0] == int(out[2].counts[1]) >= 3 and want["counts"][2:5].tolist() == [0, 0, 0], "every object is checked"
    assert bad["raw"] == 0 and int(out[-3].counts[5]) == 0 and int(out[-3].counts[6]) == 0 and int(out[-3].info[6]) > 0, "raw pieces share walls only"
    assert bad["simplified"] >= 2
    with pytest.raises(ValueError):
        inf.predict(scene, objects=True, conflicts=True)


def _main(tmp, name, extra, capsys, monkeypatch):
    from change3d_amd.scripts import predict_scene
    monkeypatch.setattr(predict_scene, "build_model", lambda args, device: _RedChannel().to(device))
    predict_scene.main(["--task", "BCD", "--weights", "unused", "--pre", str(tmp / "a.png"), "--post", str(tmp / "b.png"), "--stride", "32",
                        "--batch_size", "8", "--in_height", str(T), "--in_width", str(T), "--out_dir", str(tmp / name), "--objects",
                        "--split_objects", str(SPLIT), "--polygons", "--simplify", str(TOL), "--regularize"] + extra)
    return capsys.readouterr().out.splitlines()


def _written(doc, frac_bits):
    """The restatement on the polygons of a FeatureCollection as it was written."""
    rings, ids = [], []
    for f in doc["features"]:
        for ring in f["geometry"]["coordinates"]:
            rings.append([(int(round(x * (1 << frac_bits))), int(round(y * (1 << frac_bits)))) for x, y in ring[:-1]])
            ids.append(f["properties"]["id"])
    c = K.case(rings, ids=ids, frac_bits=frac_bits)
    return R.conflicts(K.tables(c), frac_bits, c["max_ids"])


def test_predict_scene_conflicts_and_the_fall_back_loop(tmp_path, capsys, monkeypatch):
    from PIL import Image
    tmp, scene = tmp_path, _scene()
    Image.fromarray(scene[:, :, 0:3]).save(tmp / "a.png")
    Image.fromarray(scene[:, :, 3:6]).save(tmp / "b.png")
    plain = _main(tmp, "plain", [], capsys, monkeypatch)
    told = _main(tmp, "told", ["--conflicts"], capsys, monkeypatch)
    clean = _main(tmp, "clean", ["--simplify_clean", "--regularize_clean"], capsys, monkeypatch)
    out = _inferencer().predict(scene, objects=True, outlines=True, split=SPLIT, simplify=TOL, regularize=True, conflicts=True)
    stages = dict(zip(("raw", "simplified", "regular"), out[-3:]))
    # the closing lines, after everything a run without the flag prints
    assert [ln.replace(str(tmp / "told"), str(tmp / "plain")) for ln in told[:-3]] == plain
    # the `regularize:` line counts what is written: objects that --regularize_clean put back are fallbacks there
    differ = [(a, b) for a, b in zip([ln.replace(str(tmp / "clean"), str(tmp / "plain")) for ln in clean[:-3]], plain) if a != b]
    assert len(clean) == len(plain) + 3 and all(a.startswith("regularize:") for a, _ in differ)
    assert not [ln for ln in plain if ln.startswith("conflicts[")]
    for line, (stage, v) in zip(told[-3:], stages.items()):
        c = [int(x) for x in v.counts.cpu().tolist()]
        assert line == (f"conflicts[{stage}]: objects = {c[0]} clean = {c[0] - c[1]} in_conflict = {c[1]} unchecked = 0 "
                        f"crossings = {c[5]} overlaps = {c[6]} shared_walls = {int(v.info[6])}"), line
    # the files: the three properties are all that --conflicts adds
    docs = {n: {k: json.loads((tmp / n / "objects" / f"scene{k}.geojson").read_text()) for k in ("", ".regular")}
            for n in ("plain", "told", "clean")}
    for n in ("told", "clean"):
        assert (tmp / n / "objects" / "scene.csv").read_bytes() == (tmp / "plain" / "objects" / "scene.csv").read_bytes()
        assert (tmp / n / "scene.png").read_bytes() == (tmp / "plain" / "scene.png").read_bytes()
    for kind, stage in (("", "simplified"), (".regular", "regular")):
        rows = stages[stage].conflict.cpu().numpy()
        feats = docs["told"][kind]["features"]
        assert len(feats) == len(docs["plain"][kind]["features"]) >= 3
        for f, b in zip(feats, docs["plain"][kind]["features"]):
            p = dict(f["properties"])
            got = {k: p.pop(k) for k in KEYS}
            row = rows[p["id"] - 1]
            assert got == dict(conflicts=int(row[3] + row[4]), conflict_with=int(row[1]), shared_walls=int(row[5]))
            assert p == b["properties"] and f["geometry"] == b["geometry"]
        assert not any(k in b["properties"] for b in docs["plain"][kind]["features"] for k in KEYS)
    assert _written(docs["told"][""], 0)["counts"][1] >= 2, "the simplified pieces conflict as written"
    # the loop: what is written shows no crossing and no same-direction overlap, and says so
    for kind, f_bits, line in (("", 0, clean[-2]), (".regular", 4, clean[-1])):
        want = _written(docs["clean"][kind], f_bits)
        assert want["counts"][5] == 0 and want["counts"][6] == 0 and want["counts"][1] == 0, kind
        words = line.split()
        assert line.startswith("conflicts[") and "in_conflict = 0" in line and "remaining = 0" in line and int(words[words.index("rounds") + 2]) >= 1
        assert f"shared_walls = {int(want['info'][6])}" in line
        for f in docs["clean"][kind]["features"]:
            row = want["conflict"][f["properties"]["id"] - 1]
            assert (f["properties"]["conflicts"], f["properties"]["conflict_with"], f["properties"]["shared_walls"]) == (0, 0, int(row[5]))
    fallen = [f for f, t in zip(docs["clean"][""]["features"], docs["told"][""]["features"]) if f["geometry"] != t["geometry"]]
    assert len(fallen) >= 2 and all(f["properties"]["vertices"] == f["properties"]["vertices_raw"] for f in fallen)
    # no round allowed: the objects in conflict are named and the run ends with an error
    with pytest.raises(SystemExit) as err:
        _main(tmp, "none", ["--simplify_clean", "--clean_rounds", "0"], capsys, monkeypatch)
    assert "--clean_rounds" in str(err.value) and "scene:" in str(err.value)


def test_the_parser_ties_the_flags_to_their_stages(capsys):
    from change3d_amd.scripts.predict_scene import parse_args
    common = ["--weights", "w.pth", "--pre", "a.png", "--post", "b.png", "--objects"]
    for extra in (["--conflicts"], ["--polygons", "--simplify_clean"], ["--polygons", "--simplify", "1", "--regularize_clean"],
                  ["--polygons", "--conflicts", "--clean_rounds", "-1"]):
        with pytest.raises(SystemExit):
            parse_args(common + extra)
        capsys.readouterr()
    args = parse_args(common + ["--polygons", "--simplify", "1", "--simplify_clean"])
    assert args.conflicts and args.simplify_clean and not args.regularize_clean and args.clean_rounds == 8
    assert not parse_args(common + ["--polygons"]).conflicts
