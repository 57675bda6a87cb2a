"""BDA (xBD) as a scene task and the objects of a scene, on the MI355X with a seeded 64 x 64 model: one tile against the plain
`update_bda` eval forward bit for bit, a 100 x 150 scene against the float64 stitch of the model's own per-tile outputs, the
two maps where float64 decides, the `SceneObjects` of `predict(objects=True)` against the restatement applied to the device's
own maps (exact), and `predict_scene --task BDA --objects` end to end on an xBD-layout tree.

Bound and undecided-pixel rule: test_scene_ops_gpu.py, as in test_scene_infer_gpu.py."""
import contextlib
import io
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import objects_reference as O  # noqa: E402
import scene_reference as R  # noqa: E402

from change3d_amd import ops  # noqa: E402
from change3d_amd import synthetic as synth  # noqa: E402
from change3d_amd.data.transforms import BCDTransforms as BT  # noqa: E402
from change3d_amd.infer import SceneInferencer, SceneObjects  # noqa: E402
from change3d_amd.model.trainer import Trainer  # noqa: E402
from oracle import transforms as ot  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
T, NUM_CLASS, SCD_CLASS = 64, 5, 7


def _scene(Hs, Ws, seed):
    return np.random.default_rng(seed).integers(0, 256, size=(Hs, Ws, 6), dtype=np.uint8)


def _normalised(crops):
    img = np.stack([ot.bcd_transform_sample(c, np.zeros(c.shape[:2], np.uint8), (0, 0, 0), BT.DEFAULT_MEAN, BT.DEFAULT_STD)[0]
                    for c in crops])
    return torch.from_numpy(img[:, 0:3]).to(DEV), torch.from_numpy(img[:, 3:6]).to(DEV)


def _model(task):
    """Seeded weights; BatchNorm running statistics of one momentum-1 train pass, as in test_scene_infer_gpu.py."""
    args = {"bcd": lambda: synth.make_args(size=T),
            "bda": lambda: synth.make_args(num_perception_frame=2, size=T, dataset="xBD", num_class=NUM_CLASS),
            "scd": lambda: synth.make_args(num_perception_frame=3, size=T, dataset="SECOND", num_class=SCD_CLASS)}[task]()
    args.act_dtype = torch.float32
    with contextlib.redirect_stdout(io.StringIO()):
        net = Trainer(args)
    net.load_state_dict(synth.synth_state_dict(net, seed=16, mask_margin=0.25))
    net = net.to(DEV).train()
    bns = [m for m in net.modules() if isinstance(m, torch.nn.BatchNorm3d)]
    for m in bns:
        m.momentum = 1.0
    pre, post = _normalised(R.crops(_scene(100, 150, 5), T, T, 32, 32)[:8])
    with torch.no_grad():
        getattr(net, "update_" + task)(pre, post)
    for m in bns:
        m.momentum = 0.1
    ops.bump_weights_version()
    return net.eval()


@pytest.fixture(scope="module")
def bda_model():
    return _model("bda")


@pytest.fixture(scope="module")
def bcd_model():
    return _model("bcd")


def _tile_outputs(net, scene, s, batch):
    """(damage logits, localisation probability) of every tile, in `predict`'s batches: two arrays [ny, nx, C, T, T]."""
    crops = R.crops(scene, T, T, s, s)
    ny, nx = R.plan(scene.shape[0], T, s)[1], R.plan(scene.shape[1], T, s)[1]
    pre, post = _normalised(crops)
    outs = []
    with torch.no_grad():
        for j in range(0, len(crops), batch):
            outs.append([t.float().cpu().numpy() for t in net.update_bda(pre[j:j + batch], post[j:j + batch])])
    heads = [np.concatenate([o[h] for o in outs]) for h in range(2)]
    return [h.reshape(ny, nx, h.shape[1], T, T) for h in heads]


def _assert_objects(objects, mask, cls_map, score, n_cls, **kw):
    """`objects` against the restatement applied to the device's own maps: exact."""
    assert isinstance(objects, SceneObjects)
    cpu = lambda t: None if t is None else t.cpu().numpy()  # noqa: E731
    want = O.objects(cpu(mask), cpu(cls_map), cpu(score), n_cls=n_cls, first_class=1, **kw)
    assert np.array_equal(cpu(objects.counts), want["counts"]), (cpu(objects.counts), want["counts"])
    assert np.array_equal(cpu(objects.labels), want["labels"]) and np.array_equal(cpu(objects.table), want["table"])
    assert np.array_equal(cpu(objects.object_cls), want["object_cls"])
    if cls_map is None:
        assert objects.hist is None
    else:
        assert np.array_equal(cpu(objects.hist).astype(np.int64), want["hist"])
    return want


def test_bda_one_tile_is_the_plain_eval_forward(bda_model):
    scene = _scene(T, T, 1)
    loc_prob, loc_mask, damage, logits = SceneInferencer(bda_model, "bda", stride=T, window="flat").predict(torch.from_numpy(scene))
    pre, post = torch.empty((1, 3, T, T), device=DEV), torch.empty((1, 3, T, T), device=DEV)
    ops.bcd_preprocess(torch.from_numpy(scene[None]).to(DEV), None, None, torch.tensor(BT.DEFAULT_MEAN, device=DEV),
                       torch.tensor(BT.DEFAULT_STD, device=DEV), pre, post, None, 1, T, T)
    with torch.no_grad():
        want_cls, want_loc = bda_model.update_bda(pre, post)
    assert loc_prob.dtype == torch.float32 and loc_mask.dtype == damage.dtype == torch.uint8 and tuple(logits.shape) == (NUM_CLASS, T, T)
    assert torch.equal(loc_prob, want_loc[0, 0].float()) and torch.equal(logits, want_cls[0].float())
    mask = (want_loc[0, 0] > 0.5).to(torch.uint8)
    assert torch.equal(loc_mask, mask) and torch.equal(damage, want_cls[0].argmax(0).to(torch.uint8) * mask)
    assert 0.02 < float(want_loc.mean()) < 0.98 and float(want_loc.std()) > 0.01   # not saturated: the comparison says something


@pytest.mark.parametrize("shape", [(T, T, T, "flat", 5), (100, 150, 32, "hann", 5), (100, 150, 32, "hann", 3)])
def test_bda_scene_against_the_float64_stitch_and_its_objects_against_the_restatement(bda_model, shape):
    Hs, Ws, s, window, batch = shape
    scene = _scene(Hs, Ws, 2)
    inf = SceneInferencer(bda_model, "bda", stride=s, window=window, batch=batch)
    plain = inf.predict(scene)
    loc_prob, loc_mask, damage, logits, objects = inf.predict(torch.from_numpy(scene), objects=True, min_area=2, connectivity=4,
                                                              max_objects=256)
    assert len(plain) == 4 and all(torch.equal(a, b) for a, b in zip(plain, (loc_prob, loc_mask, damage, logits)))
    tiles_cls, tiles_loc = _tile_outputs(bda_model, scene, s, batch)
    wy = wx = R.window(window, T)
    ref_loc, ref_cls = R.stitch(tiles_loc, Hs, Ws, s, s, wy, wx), R.stitch(tiles_cls, Hs, Ws, s, s, wy, wx)
    for got, ref, what in ((loc_prob[None], ref_loc, "loc_prob"), (logits, ref_cls, "cls_logits")):
        lim = R.bound(ref)
        err = np.abs(got.cpu().numpy().astype(np.float64) - ref["blend"])
        print(f"PARITY predict bda {what} {Hs}x{Ws} s={s} batch={batch}: max |err| {err.max():.3e}  worst err/bound "
              f"{(err / np.maximum(lim, 1e-300)).max():.3f}")
        assert (err <= lim).all(), what
    lim = R.bound(ref_loc)
    ok_m, want_m = np.abs(ref_loc["blend"][0] - 0.5) > lim[0], (ref_loc["blend"][0] > 0.5).astype(np.uint8)
    assert 1.0 - ok_m.mean() <= 1e-3 and np.array_equal(loc_mask.cpu().numpy()[ok_m], want_m[ok_m])
    lim = R.bound(ref_cls)
    order = np.argsort(ref_cls["blend"], axis=0)
    take = lambda a, i: np.take_along_axis(a, i[None], axis=0)[0]  # noqa: E731
    ok = take(ref_cls["blend"], order[-1]) - take(ref_cls["blend"], order[-2]) > take(lim, order[-1]) + take(lim, order[-2])
    ok &= ok_m
    assert 1.0 - ok.mean() <= 1e-3
    assert np.array_equal(damage.cpu().numpy()[ok], (order[-1].astype(np.uint8) * want_m)[ok])
    assert torch.equal(loc_mask, (loc_prob > 0.5).to(torch.uint8))
    assert torch.equal(damage, logits.argmax(0).to(torch.uint8) * loc_mask) and int(damage.max()) < NUM_CLASS
    _assert_objects(objects, loc_mask, damage, loc_prob, NUM_CLASS, min_area=2, connectivity=4, max_objects=256)
    assert tuple(objects.table.shape) == (256, 8) and tuple(objects.hist.shape) == (256, NUM_CLASS)


def test_bcd_objects_leave_the_maps_alone_and_equal_the_restatement(bcd_model):
    scene = _scene(100, 150, 2)
    inf = SceneInferencer(bcd_model, "bcd", stride=32, batch=5)
    prob, mask = inf.predict(scene)
    prob2, mask2, objects = inf.predict(scene, objects=True, min_area=3, max_objects=64)
    assert torch.equal(prob, prob2) and torch.equal(mask, mask2)
    want = _assert_objects(objects, mask, None, prob, 1, min_area=3, connectivity=8, max_objects=64)
    assert int(want["object_cls"].sum()) == 0
    with pytest.raises(ValueError):
        inf.predict(scene, objects=True, connectivity=6)


def _write_xbd_tree(root, scene, loc, dmg, name="guatemala-volcano_00000000_post_disaster.png"):
    from PIL import Image
    for sub in ("t1", "t2", "label1", "label2"):
        os.makedirs(root / "test" / sub)
    Image.fromarray(scene[:, :, 0:3]).save(root / "test" / "t1" / name)
    Image.fromarray(scene[:, :, 3:6]).save(root / "test" / "t2" / name)
    target = name.replace("disaster", "disaster_target")
    Image.fromarray(loc).save(root / "test" / "label1" / target)
    Image.fromarray(dmg).save(root / "test" / "label2" / target)
    return os.path.splitext(name)[0]


def test_predict_scene_bda_objects_end_to_end(bda_model, tmp_path, capsys):
    from PIL import Image
    from change3d_amd.scripts import predict_scene
    Hs, Ws = 100, 150
    scene = _scene(Hs, Ws, 4)
    rng = np.random.default_rng(9)
    loc = (rng.random((Hs, Ws)) < 0.4).astype(np.uint8)
    dmg = rng.integers(1, NUM_CLASS, size=(Hs, Ws), dtype=np.uint8)
    name = _write_xbd_tree(tmp_path, scene, loc, dmg)
    torch.save(bda_model.state_dict(), tmp_path / "best_model.pth")
    out = tmp_path / "out"
    predict_scene.main(["--task", "BDA", "--objects", "--min_area", "2", "--weights", str(tmp_path / "best_model.pth"), "--file_root",
                        str(tmp_path), "--split", "test", "--out_dir", str(out), "--stride", "32", "--batch_size", "5", "--act_dtype",
                        "f32", "--in_height", str(T), "--in_width", str(T), "--pretrained", "/nonexistent"])
    printed = capsys.readouterr().out
    bgr = np.concatenate((scene[:, :, 2::-1], scene[:, :, :2:-1]), axis=2)             # BDADataset reads in cv2's channel order
    loc_prob, loc_mask, damage, logits, objects = SceneInferencer(bda_model, "bda", stride=32, batch=5).predict(
        np.ascontiguousarray(bgr), objects=True, min_area=2)
    read = lambda sub, ext=".png": np.asarray(Image.open(out / sub / (name + ext)))  # noqa: E731
    assert np.array_equal(read("loc"), loc_mask.cpu().numpy() * 255) and np.array_equal(read("damage"), damage.cpu().numpy())
    assert np.array_equal(read("damage_objects"), objects.object_cls.cpu().numpy())
    lines = (out / "objects" / (name + ".csv")).read_text().splitlines()
    assert lines[0] == "id,area,x0,y0,x1,y1,cls,score"
    found, rows = objects.counts.tolist()
    assert len(lines) == 1 + rows and found == rows
    table = objects.table[:rows].cpu().numpy()
    for k, line in enumerate(lines[1:]):
        f = line.split(",")
        assert [int(v) for v in f[:7]] == [k + 1] + table[k, :6].tolist() and f[7] == f"{table[k, 7] / 65535:.4f}"
    assert re.search(r"loc_f1_score = -?[0-9.na]+\s+harmonic_mean_f1 = -?[0-9.na]+\s+oaf1 = -?[0-9.na]+\s+damage_f1_score = \[", printed)
    assert re.search(r"Objects:\s+harmonic_mean_f1 = -?[0-9.na]+\s+damage_f1_score = \[", printed)
    from change3d_amd.model.utils import BDAEvaluator
    ev = BDAEvaluator(NUM_CLASS, DEV)
    ev.add_batch(logits[None], loc_prob[None, None], torch.from_numpy(loc).to(DEV).float()[None],
                 torch.from_numpy(loc.astype(np.int64) * dmg).to(DEV)[None])
    loc_f1 = ev.scores()[0]
    assert f"loc_f1_score = {loc_f1:.4f}" in printed


def test_predict_scene_bcd_prints_the_same_score_line_with_and_without_objects(bcd_model, tmp_path, capsys):
    from PIL import Image
    from change3d_amd.scripts import predict_scene
    Hs, Ws = 100, 150
    scene = _scene(Hs, Ws, 4)
    label = (np.random.default_rng(9).random((Hs, Ws)) < 0.3).astype(np.uint8) * 255
    Image.fromarray(scene[:, :, 0:3]).save(tmp_path / "a.png")
    Image.fromarray(scene[:, :, 3:6]).save(tmp_path / "b.png")
    Image.fromarray(label).save(tmp_path / "label.png")
    torch.save(bcd_model.state_dict(), tmp_path / "best_model.pth")
    argv = ["--task", "BCD", "--weights", str(tmp_path / "best_model.pth"), "--pre", str(tmp_path / "a.png"), "--post",
            str(tmp_path / "b.png"), "--label", str(tmp_path / "label.png"), "--stride", "32",
            "--batch_size", "5", "--act_dtype", "f32", "--in_height", str(T), "--in_width", str(T), "--pretrained", "/nonexistent"]
    predict_scene.main(argv + ["--out_dir", str(tmp_path / "plain")])
    plain = capsys.readouterr().out
    predict_scene.main(argv + ["--out_dir", str(tmp_path / "objects"), "--objects"])
    with_objects = capsys.readouterr().out
    score = lambda text: [l for l in text.splitlines() if l.startswith("Test:")]  # noqa: E731
    assert len(score(plain)) == 1 and score(plain) == score(with_objects)
    assert (tmp_path / "plain" / "scene.png").read_bytes() == (tmp_path / "objects" / "scene.png").read_bytes()
    assert not (tmp_path / "plain" / "objects").exists()
    lines = (tmp_path / "objects" / "objects" / "scene.csv").read_text().splitlines()
    _, mask, objects = SceneInferencer(bcd_model, "bcd", stride=32, batch=5).predict(torch.from_numpy(scene), objects=True)
    assert lines[0] == "id,area,x0,y0,x1,y1,cls,score" and len(lines) == 1 + int(objects.counts[1])


def test_scd_objects_of_the_change_mask_voted_over_the_post_classes(tmp_path, capsys):
    """`predict(objects=True)` for SCD against the restatement, and `predict_scene --task SCD --objects` writes their CSV."""
    from PIL import Image
    from change3d_amd.scripts import predict_scene
    net = _model("scd")
    scene = _scene(100, 150, 6)
    inf = SceneInferencer(net, "scd", stride=32, batch=5)
    plain = inf.predict(scene)
    pre_cls, post_cls, change, objects = inf.predict(scene, objects=True, min_area=2)
    assert len(plain) == 3 and all(torch.equal(a, b) for a, b in zip(plain, (pre_cls, post_cls, change)))
    _assert_objects(objects, change, post_cls, None, SCD_CLASS, min_area=2, connectivity=8, max_objects=65536)
    assert int(objects.table[:, 7].abs().sum()) == 0       # no score map: score_q is 0
    Image.fromarray(scene[:, :, 0:3]).save(tmp_path / "a.png")
    Image.fromarray(scene[:, :, 3:6]).save(tmp_path / "b.png")
    torch.save(net.state_dict(), tmp_path / "best_model.pth")
    argv = ["--task", "SCD", "--weights", str(tmp_path / "best_model.pth"), "--pre", str(tmp_path / "a.png"), "--post",
            str(tmp_path / "b.png"), "--stride", "32", "--batch_size", "5", "--act_dtype", "f32", "--in_height", str(T),
            "--in_width", str(T), "--pretrained", "/nonexistent"]
    predict_scene.main(argv + ["--out_dir", str(tmp_path / "plain")])
    predict_scene.main(argv + ["--out_dir", str(tmp_path / "objects"), "--objects", "--min_area", "2"])
    capsys.readouterr()
    for sub in ("pred1", "pred2", "change"):
        assert (tmp_path / "plain" / sub / "scene.png").read_bytes() == (tmp_path / "objects" / sub / "scene.png").read_bytes()
    assert np.array_equal(np.asarray(Image.open(tmp_path / "objects" / "change" / "scene.png")), change.cpu().numpy() * 255)
    assert not (tmp_path / "plain" / "objects").exists()
    lines = (tmp_path / "objects" / "objects" / "scene.csv").read_text().splitlines()
    rows = int(objects.counts[1])
    table = objects.table[:rows].cpu().numpy()
    assert lines[0] == "id,area,x0,y0,x1,y1,cls,score" and len(lines) == 1 + rows
    for k, line in enumerate(lines[1:]):
        f = line.split(",")
        assert [int(v) for v in f[:7]] == [k + 1] + table[k, :6].tolist() and f[7] == "0.0000"
