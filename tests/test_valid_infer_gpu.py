"""`c3d_rings_valid` in the layers above it: one 96 x 96 scene -- a noisy 20 x 20 mask of the survey whose second object
crosses itself once simplified at 2 px, beside one clean rectangle -- through `SceneInferencer.predict(validity=True)` and
`predict_scene --validity --simplify_valid`.  The model is a stand-in that answers with the red channel of the first image, so
the mask is the one drawn here; everything after the model is the device pipeline."""
import json
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import valid_cases as K  # noqa: E402
import valid_reference as V  # noqa: E402

from change3d_amd import ops  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SIZE, T, TOL = 96, 64, 2.0
VALID_LAUNCHES = 10                                          # as include/change3d_hip.h documents them
KEYS = ("valid", "crossings", "overlaps", "touches")


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
    mask[4:24, 4:24] = K.survey_mask(27)
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
            elif n is not None and x.dim() == 2 and x.shape[-1] == 2:
                assert torch.equal(x[:n], y[:n])
            else:
                assert torch.equal(x, y)


def test_predict_with_validity_equals_the_restatement_on_its_own_rings():
    from change3d_amd.infer import SceneValidity
    inf, scene = _inferencer(), _scene()
    kw = dict(objects=True, outlines=True, simplify=TOL, regularize=True, max_objects=64)
    today = inf.predict(scene, **kw)
    before = ops.launch_count()
    off = inf.predict(scene, validity=False, **kw)
    plain = ops.launch_count() - before
    before = ops.launch_count()
    out = inf.predict(scene, validity=True, **kw)
    assert ops.launch_count() - before == plain + 3 * VALID_LAUNCHES
    assert torch.equal(out[1].cpu(), torch.from_numpy(_mask())), "the stand-in model draws the mask"
    assert len(out) == len(today) + 3 and all(isinstance(v, SceneValidity) for v in out[-3:])
    _same_but_spare_vertex_rows(today, off)
    _same_but_spare_vertex_rows(today, out[:-3])
    raw, simple, regular = out[3], out[4], out[5]
    invalid = {}
    for stage, table, f, got in (("raw", raw, 0, out[-3]), ("simplified", simple, 0, out[-2]), ("regular", regular, 4, out[-1])):
        want = V.valid(tuple(t.cpu().numpy() for t in table), f, 64)
        assert np.array_equal(got.valid.cpu().numpy(), want["valid"]), stage
        assert np.array_equal(got.counts.cpu().numpy(), want["counts"]), stage
        invalid[stage] = int(want["counts"][1])
        assert want["counts"][0] == int(out[2].counts[1]) >= 3 and want["counts"][2:5].tolist() == [0, 0, 0], "every object is checked"
    assert invalid["raw"] == 0 and invalid["simplified"] >= 1
    rows = out[-2].valid.cpu().numpy()
    assert rows[1, 4] == 2 and rows[1, 0] == 0, "object 2 is the survey's seed 27, 8-connectivity, id 2: two crossings at 2 px"
    with pytest.raises(ValueError):
        inf.predict(scene, objects=True, validity=True)


def _main(tmp, name, extra, capsys, monkeypatch):
    from change3d_amd.scripts import predict_scene
    monkeypatch.setattr(predict_scene, "build_model", lambda args, device: _RedChannel().to(device))
    predict_scene.main(["--task", "BCD", "--weights", "unused", "--pre", str(tmp / "a.png"), "--post", str(tmp / "b.png"), "--stride", "32",
                        "--batch_size", "8", "--in_height", str(T), "--in_width", str(T), "--out_dir", str(tmp / name), "--objects",
                        "--polygons", "--simplify", str(TOL), "--regularize"] + extra)
    return capsys.readouterr().out.splitlines()


def test_predict_scene_validity_and_the_fallback_to_raw_vertices(tmp_path, capsys, monkeypatch):
    from PIL import Image
    tmp, scene = tmp_path, _scene()
    Image.fromarray(scene[:, :, 0:3]).save(tmp / "a.png")
    Image.fromarray(scene[:, :, 3:6]).save(tmp / "b.png")
    plain = _main(tmp, "plain", [], capsys, monkeypatch)
    told = _main(tmp, "told", ["--validity"], capsys, monkeypatch)
    fallen = _main(tmp, "fallen", ["--validity", "--simplify_valid", "--regularize_valid"], capsys, monkeypatch)
    out = _inferencer().predict(scene, objects=True, outlines=True, simplify=TOL, regularize=True, validity=True)
    stages = dict(zip(("raw", "simplified", "regular"), out[-3:]))
    # the closing lines, after everything a run without the flag prints
    for lines, name in ((told, "told"), (fallen, "fallen")):
        closing = lines[-3:]
        assert [ln.replace(str(tmp / name), str(tmp / "plain")) for ln in lines[:-3]] == plain
        for line, (stage, v) in zip(closing, stages.items()):
            c = [int(x) for x in v.counts.cpu().tolist()]
            assert line == (f"validity[{stage}]: objects = {c[0]} valid = {c[0] - c[1]} invalid = {c[1]} unchecked = 0 "
                            f"crossings = {c[5]} overlaps = {c[6]}"), line
    assert not [ln for ln in plain if ln.startswith("validity[")]
    # the files: the four properties are all that --validity adds
    docs = {n: {k: json.loads((tmp / n / "objects" / f"scene{k}.geojson").read_text()) for k in ("", ".regular")}
            for n in ("plain", "told", "fallen")}
    for n in ("told", "fallen"):
        assert (tmp / n / "objects" / "scene.csv").read_bytes() == (tmp / "plain" / "objects" / "scene.csv").read_bytes()
        assert (tmp / n / "scene.png").read_bytes() == (tmp / "plain" / "scene.png").read_bytes()
    for kind, stage in (("", "simplified"), (".regular", "regular")):
        rows = stages[stage].valid.cpu().numpy()
        feats = docs["told"][kind]["features"]
        assert len(feats) == len(docs["plain"][kind]["features"]) >= 3
        for f, b in zip(feats, docs["plain"][kind]["features"]):
            p = dict(f["properties"])
            got = {k: p.pop(k) for k in KEYS}
            row = rows[p["id"] - 1]
            assert got == dict(valid=bool(row[0] == 0 and row[4] == 0 and row[5] == 0), crossings=int(row[4]), overlaps=int(row[5]),
                               touches=int(row[6] + row[7]))
            assert p == b["properties"] and f["geometry"] == b["geometry"]
        assert not any(k in b["properties"] for b in docs["plain"][kind]["features"] for k in KEYS)
    # the fallback: object 2 is written on its raw vertices, valid: false; the valid objects are where they were
    bad = {k + 1 for k, row in enumerate(stages["simplified"].valid[:int(out[2].counts[1])].cpu().tolist()) if row[4] or row[5]}
    assert 2 in bad
    raw_rings, raw_vertices = out[3].rings.cpu().numpy(), out[3].vertices.cpu().numpy()
    for f, t in zip(docs["fallen"][""]["features"], docs["told"][""]["features"]):
        p = f["properties"]
        if p["id"] not in bad:
            assert f == t
            continue
        assert p["valid"] is False and p["crossings"] + p["overlaps"] >= 1 and p["vertices"] == p["vertices_raw"]
        want = sorted(raw_vertices[s:s + n].tolist() + [raw_vertices[s].tolist()] for i, s, n in raw_rings[:, :3].tolist() if i == p["id"])
        assert sorted(f["geometry"]["coordinates"]) == want, "the raw vertices in every ring"
    bad_regular = {k + 1 for k, row in enumerate(stages["regular"].valid[:int(out[2].counts[1])].cpu().tolist()) if row[4] or row[5]}
    for f, t, m in zip(docs["fallen"][".regular"]["features"], docs["told"][".regular"]["features"], docs["fallen"][""]["features"]):
        if f["properties"]["id"] in bad_regular:
            assert f["properties"]["regular"] is False and f["geometry"] == m["geometry"] and f["properties"]["valid"] is False
        elif f["properties"]["id"] not in bad:
            assert f == t


def test_the_parser_ties_the_flags_to_their_stages(capsys):
    from change3d_amd.scripts.predict_scene import parse_args
    common = ["--weights", "w.pth", "--pre", "a.png", "--post", "b.png", "--objects"]
    for extra in (["--validity"], ["--polygons", "--simplify_valid"], ["--polygons", "--simplify", "1", "--regularize_valid"]):
        with pytest.raises(SystemExit):
            parse_args(common + extra)
        capsys.readouterr()
    args = parse_args(common + ["--polygons", "--simplify", "1", "--simplify_valid"])
    assert args.validity and args.simplify_valid and not args.regularize_valid
    assert not parse_args(common + ["--polygons"]).validity
