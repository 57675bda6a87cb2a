"""`SceneInferencer.predict` and `scripts/predict_scene.py` on the MI355X with seeded 64 x 64 models: one tile against the
plain eval forward bit for bit, a 100 x 150 scene against the float64 stitch of the model's own per-tile outputs (same
batches, crops cut with numpy), the SCD post-processing, and the script end to end on PNG files.

Bound and undecided-pixel rule: test_scene_ops_gpu.py.  The per-tile outputs are the model's own on both sides, so the
only difference is the stitch's f32 arithmetic."""
import contextlib
import io
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import scene_reference as R  # noqa: E402

from change3d_amd import ops  # noqa: E402
from change3d_amd import synthetic as synth  # noqa: E402
from change3d_amd.data.transforms import BCDTransforms as BT  # noqa: E402
from change3d_amd.infer import SceneInferencer  # noqa: E402
from change3d_amd.model.trainer import Trainer  # noqa: E402
from oracle import transforms as ot  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
T, NUM_CLASS = 64, 7


def _scene(Hs, Ws, seed):
    return np.random.default_rng(seed).integers(0, 256, size=(Hs, Ws, 6), dtype=np.uint8)


def _normalised(crops):
    img = np.stack([ot.bcd_transform_sample(c, np.zeros(c.shape[:2], np.uint8), (0, 0, 0), BT.DEFAULT_MEAN, BT.DEFAULT_STD)[0]
                    for c in crops])
    return torch.from_numpy(img[:, 0:3]).to(DEV), torch.from_numpy(img[:, 3:6]).to(DEV)


def _model(task):
    """Seeded weights; the BatchNorm running statistics are those of one momentum-1 train pass, as in test_model_gpu.py (the
    synthetic ones saturate every eval output)."""
    args = synth.make_args(size=T) if task == "bcd" else synth.make_args(num_perception_frame=3, size=T, dataset="SECOND",
                                                                         num_class=NUM_CLASS)
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
        net.update_bcd(pre, post) if task == "bcd" else net.update_scd(pre, post)
    for m in bns:
        m.momentum = 0.1
    ops.bump_weights_version()
    return net.eval()


@pytest.fixture(scope="module")
def bcd_model():
    return _model("bcd")


@pytest.fixture(scope="module")
def scd_model():
    return _model("scd")


def _tile_outputs(net, task, scene, s, batch):
    """The model's outputs for every tile, in `predict`'s batches, on crops cut with numpy: list of [ny, nx, C, T, T]."""
    crops = R.crops(scene, T, T, s, s)
    ny, nx = R.plan(scene.shape[0], T, s)[1], R.plan(scene.shape[1], T, s)[1]
    pre, post = _normalised(crops)
    outs = []
    with torch.no_grad():
        for j in range(0, len(crops), batch):
            o = net.update_bcd(pre[j:j + batch], post[j:j + batch]) if task == "bcd" else net.update_scd(pre[j:j + batch], post[j:j + batch])
            outs.append([t.float().cpu().numpy() for t in ([o] if task == "bcd" else o)])
    heads = [np.concatenate([o[h] for o in outs]) for h in range(len(outs[0]))]
    return [h.reshape(ny, nx, h.shape[1], T, T) for h in heads]


def _decided_mask(ref):
    lim = R.bound(ref)
    return np.abs(ref["blend"][0] - 0.5) > lim[0], (ref["blend"][0] > 0.5).astype(np.uint8)


def _decided_argmax(ref):
    lim = R.bound(ref)
    order = np.argsort(ref["blend"], axis=0)
    top, second = order[-1], order[-2]
    take = lambda a, i: np.take_along_axis(a, i[None], axis=0)[0]  # noqa: E731
    return take(ref["blend"], top) - take(ref["blend"], second) > take(lim, top) + take(lim, second), top.astype(np.uint8)


def test_bcd_one_tile_is_the_plain_eval_forward(bcd_model):
    scene = _scene(T, T, 1)
    prob, mask = SceneInferencer(bcd_model, "bcd", stride=T, window="flat").predict(torch.from_numpy(scene))
    pre, post = torch.empty((1, 3, T, T), device=DEV), torch.empty((1, 3, T, T), device=DEV)
    ops.bcd_preprocess(torch.from_numpy(scene[None]).to(DEV), None, None, torch.tensor(BT.DEFAULT_MEAN, device=DEV),
                       torch.tensor(BT.DEFAULT_STD, device=DEV), pre, post, None, 1, T, T)
    with torch.no_grad():
        want = bcd_model.eval().update_bcd(pre, post)[0, 0]
    assert prob.dtype == torch.float32 and mask.dtype == torch.uint8 and prob.shape == mask.shape == (T, T)
    assert torch.equal(prob, want) and torch.equal(mask, (want > 0.5).to(torch.uint8))
    assert 0.02 < float(want.mean()) < 0.98 and float(want.std()) > 0.01          # not saturated: the comparison says something


@pytest.mark.parametrize("batch", [5, 3])
def test_bcd_scene_against_the_float64_stitch_of_the_models_own_tiles(bcd_model, batch):
    """4 x 5 tiles.  Batch 5 is one tile row per forward; batch 3 does not divide the 20 tiles and its batches span tile
    rows, so strips go out in the middle of a batch."""
    Hs, Ws, s = 100, 150, 32
    scene = _scene(Hs, Ws, 2)
    inf = SceneInferencer(bcd_model, "bcd", stride=s, window="hann", batch=batch)
    prob, mask = inf.predict(scene)                                                # a numpy array on the host is taken too
    prob2, mask2 = inf.predict(torch.from_numpy(scene).to(DEV))
    assert torch.equal(prob, prob2) and torch.equal(mask, mask2)
    tiles, = _tile_outputs(bcd_model, "bcd", scene, s, batch)
    assert tiles.shape[:2] == (4, 5)
    ref = R.stitch(tiles, Hs, Ws, s, s, R.window("hann", T), R.window("hann", T))
    lim = R.bound(ref)
    err = np.abs(prob.cpu().numpy().astype(np.float64) - ref["blend"][0])
    print(f"PARITY predict bcd {Hs}x{Ws} s={s} batch={batch}: max |err| {err.max():.3e}  worst err/bound {(err / lim[0]).max():.3f}")
    assert (err <= lim[0]).all()
    decided, want = _decided_mask(ref)
    assert 1.0 - decided.mean() <= 1e-3
    assert np.array_equal(mask.cpu().numpy()[decided], want[decided])
    assert torch.equal(mask, (prob > 0.5).to(torch.uint8))


@pytest.mark.parametrize("shape", [(T, T, T, "flat", 32), (100, 150, 32, "hann", 5), (100, 150, 32, "hann", 3)])
def test_scd_class_maps_and_change_mask(scd_model, shape):
    Hs, Ws, s, window, batch = shape
    scene = _scene(Hs, Ws, 3)
    pre_cls, post_cls, change = SceneInferencer(scd_model, "scd", stride=s, window=window, batch=batch).predict(torch.from_numpy(scene))
    for m in (pre_cls, post_cls, change):
        assert m.dtype == torch.uint8 and tuple(m.shape) == (Hs, Ws)
    heads = _tile_outputs(scd_model, "scd", scene, s, batch)
    refs = [R.stitch(h, Hs, Ws, s, s, R.window(window, T), R.window(window, T)) for h in heads]
    ok_c, want_c = _decided_mask(refs[2])
    assert 1.0 - ok_c.mean() <= 1e-3 and np.array_equal(change.cpu().numpy()[ok_c], want_c[ok_c])
    assert 0 < int(change.sum()) < Hs * Ws                                         # both values occur: the multiply is visible
    for got, ref in ((pre_cls, refs[0]), (post_cls, refs[1])):
        ok, want = _decided_argmax(ref)
        ok &= ok_c
        assert 1.0 - ok.mean() <= 1e-3
        assert np.array_equal(got.cpu().numpy()[ok], (want * want_c)[ok])          # reference scripts/train_SCD.py:148-154
        assert int((got * (1 - change)).sum()) == 0 and int(got.max()) < NUM_CLASS
    if Hs == T:                                                                    # one tile: torch's own post-processing
        pre, post = _normalised(scene[None])
        with torch.no_grad():
            a, b, c = scd_model.update_scd(pre, post)
        chg = (c[0, 0] > 0.5).to(torch.uint8)
        assert torch.equal(change, chg)
        assert torch.equal(pre_cls, a[0].argmax(0).to(torch.uint8) * chg) and torch.equal(post_cls, b[0].argmax(0).to(torch.uint8) * chg)


def test_predict_scene_script_end_to_end(bcd_model, tmp_path, capsys):
    from PIL import Image
    from change3d_amd.scripts import predict_scene
    from change3d_amd.utils.metric_tool import ConfuseMatrixMeter
    Hs, Ws = 100, 150
    scene = _scene(Hs, Ws, 4)
    label = (np.random.default_rng(9).random((Hs, Ws)) < 0.3).astype(np.uint8) * 255
    Image.fromarray(scene[:, :, 0:3]).save(tmp_path / "a.png")
    Image.fromarray(scene[:, :, 3:6]).save(tmp_path / "b.png")
    Image.fromarray(label).save(tmp_path / "label.png")
    torch.save(bcd_model.state_dict(), tmp_path / "best_model.pth")
    argv = ["--task", "BCD", "--weights", str(tmp_path / "best_model.pth"), "--pre", str(tmp_path / "a.png"), "--post",
            str(tmp_path / "b.png"), "--label", str(tmp_path / "label.png"), "--out_dir", str(tmp_path / "out"), "--stride", "32",
            "--batch_size", "5", "--act_dtype", "f32", "--in_height", str(T), "--in_width", str(T), "--pretrained", "/nonexistent"]
    predict_scene.main(argv)
    printed = capsys.readouterr().out
    _, mask = SceneInferencer(bcd_model, "bcd", stride=32, batch=5).predict(torch.from_numpy(scene))
    mask = mask.cpu().numpy()
    back = np.asarray(Image.open(tmp_path / "out" / "scene.png"))
    assert back.dtype == np.uint8 and np.array_equal(back, mask * 255)
    meter = ConfuseMatrixMeter(n_class=2)
    meter.update_cm(mask.astype(np.int64), (label > 0).astype(np.int64))
    s = meter.get_scores()
    got = dict(re.findall(r"(Kappa|IoU|F1|R|P) \(te\) = (-?[0-9.]+)", printed))
    want = {"Kappa": s["Kappa"], "IoU": s["IoU"], "F1": s["F1"], "R": s["recall"], "P": s["precision"]}
    assert got == {k: f"{v:.4f}" for k, v in want.items()}, (got, want)
