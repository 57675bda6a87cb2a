"""`SceneInferencer(..., tta=...)` and `predict_scene --tta` on the MI355X.

Stub models make the chain gather view -> model -> inverse view -> ring slot -> strip checkable without a network:
  * the PIXELWISE stub maps every pixel by itself, so all views of a tile carry the same values and `tta="d4"` must return
    what `tta=None` returns, bit for bit, in every map and table.  Its outputs are rounded to multiples of 2^-12: the fold
    adds sequentially, and x + x + x already rounds for a full-precision x, while partial sums of up to eight equal
    multiples of 2^-12 below 512 fit 24 bits, so every add and the divide by 8 are exact;
  * the POSITION-DEPENDENT stub multiplies that by a fixed asymmetric ramp over the tile, so a view that is not undone, or
    undone by the wrong inverse, shows.

The float64 restatement: numpy crops (scene_reference.crops), their views, the model itself on exactly those inputs (tile-
major, view-minor, `batch // nv` tiles per forward, as `predict` runs them), then inverse views and mean in float64
(tta_reference) and `scene_reference.stitch`.  Bound per element, with taps = tiles covering the pixel, U = 2^-24, Abar = the
float64 mean over the views of |p_j| and absw = stitch(Abar)["absw"]:

    |predict - restatement| <= (taps + 3 + nv) * U * absw

the stitch bound of test_scene_ops_gpu.py ((taps + 3) * U * sum(w |p|) / sum(w)) plus the fold's nv roundings (nv - 1 adds
and one divide, each at most U relative to a partial sum that is at most nv * Abar, divided by nv), carried through the
stitch's convex combination.  Masks and argmax maps are compared where the restatement is decided by more than the bound
(the rule of test_scene_infer_gpu.py); the undecided share of the reference is capped at 1e-3 as there."""
import contextlib
import io
import os
import re
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import scene_reference as R  # noqa: E402
import tta_reference as TR  # noqa: E402

from change3d_amd import ops  # noqa: E402
from change3d_amd import synthetic as synth  # noqa: E402
from change3d_amd.data.transforms import BCDTransforms as BT  # noqa: E402
from change3d_amd.infer import SceneInferencer  # noqa: E402
from change3d_amd.model.trainer import Trainer  # noqa: E402
from oracle import transforms as ot  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
T, S, HS, WS = 64, 32, 100, 150
NUM_CLASS = {"bcd": 1, "scd": 7, "bda": 5}


def _scene(Hs, Ws, seed):
    return np.random.default_rng(seed).integers(0, 256, size=(Hs, Ws, 6), dtype=np.uint8)


def _normalised(crops):
    return np.stack([ot.bcd_transform_sample(c, np.zeros(c.shape[:2], np.uint8), (0, 0, 0), BT.DEFAULT_MEAN, BT.DEFAULT_STD)[0]
                     for c in crops])


class Stub(torch.nn.Module):
    """update_*: per pixel a fixed mix of the six input channels per output channel -- sigmoid for the probability heads, raw
    for the logit heads -- times `ramp` (ones: pixelwise), rounded to multiples of 2^-12 where `grid` is set."""

    def __init__(self, task, ramp=False, grid=False):
        super().__init__()
        self.args = SimpleNamespace(in_height=T, in_width=T, num_class=NUM_CLASS[task])
        self.decoder_loc = self.decoder_cls = torch.nn.Identity()       # what SceneInferencer asks of a BDA model
        rng = np.random.default_rng(11)
        self.mix = torch.nn.Parameter(torch.from_numpy(rng.uniform(-1.0, 1.0, size=(3, 7, 6)).astype(np.float32)))
        y, x = np.meshgrid(np.arange(T), np.arange(T), indexing="ij")
        r = 0.5 + (3 * y + x * x / T) / (8.0 * T) if ramp else np.ones((T, T))    # no symmetry of the square keeps it
        self.register_buffer("ramp", torch.from_numpy(r.astype(np.float32)))
        self.grid = grid

    def _head(self, pre, post, h, C, prob):
        x = torch.cat([pre, post], dim=1)
        out = []
        for c in range(C):                                                # elementwise only: a pixel's value depends on nothing else
            acc = self.mix[h, c, 0] * x[:, 0]
            for k in range(1, 6):
                acc = acc + self.mix[h, c, k] * x[:, k]
            out.append(acc)
        o = torch.stack(out, dim=1)
        o = (torch.sigmoid(o) if prob else o) * self.ramp
        return torch.round(o * 4096.0) / 4096.0 if self.grid else o

    def update_bcd(self, pre, post):
        return self._head(pre, post, 0, 1, True)

    def update_scd(self, pre, post):
        return self._head(pre, post, 0, 7, False), self._head(pre, post, 1, 7, False), self._head(pre, post, 2, 1, True)

    def update_bda(self, pre, post):
        return self._head(pre, post, 0, 5, False), self._head(pre, post, 1, 1, True)


def _same(a, b):
    if isinstance(a, torch.Tensor):
        return isinstance(b, torch.Tensor) and a.dtype == b.dtype and torch.equal(a, b)
    if isinstance(a, tuple):
        return isinstance(b, tuple) and len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    return a is None and b is None


@pytest.mark.parametrize("batch", [8, 24])
@pytest.mark.parametrize("task", ["bcd", "scd", "bda"])
def test_pixelwise_stub_d4_is_the_plain_prediction_bit_for_bit(task, batch):
    """4 x 5 tiles; batch 8 is one tile per forward, batch 24 three, so a forward spans tile rows."""
    net = Stub(task, grid=True).to(DEV)
    scene = torch.from_numpy(_scene(HS, WS, 21))
    plain = SceneInferencer(net, task, stride=S, window="hann", batch=batch)
    d4 = SceneInferencer(net, task, stride=S, window="hann", batch=batch, tta="d4")
    want, got = plain.predict(scene), d4.predict(scene)
    assert ops.view_count(0xff) == 8 and len(want) == len(got) == {"bcd": 2, "scd": 3, "bda": 4}[task]
    assert _same(want, got)
    assert 0 < int(want[{"bcd": 1, "scd": 2, "bda": 1}[task]].sum()) < HS * WS        # the mask has both values
    want = plain.predict(scene, objects=True, outlines=True)
    got = d4.predict(scene, objects=True, outlines=True)
    assert len(got) == len(want) and _same(want[:-2], got[:-2])
    (obj_w, out_w), (obj_g, out_g) = want[-2:], got[-2:]
    rows, ring_rows, written = int(obj_w.counts[1]), int(out_w.counts[1]), int(out_w.counts[3])
    assert rows > 0 and ring_rows >= rows and written >= 4 * ring_rows and int(out_w.counts[4]) == 0
    assert _same((obj_w.labels, obj_w.counts, obj_w.object_cls, obj_w.table[:rows]), (obj_g.labels, obj_g.counts, obj_g.object_cls, obj_g.table[:rows]))
    assert _same(None if obj_w.hist is None else obj_w.hist[:rows], None if obj_g.hist is None else obj_g.hist[:rows])
    assert _same((out_w.counts, out_w.rings[:ring_rows], out_w.vertices[:written]),     # rows past the counts are not defined
                 (out_g.counts, out_g.rings[:ring_rows], out_g.vertices[:written]))


def test_single_identity_view_is_the_plain_prediction():
    net = Stub("bda", ramp=True).to(DEV)
    scene = torch.from_numpy(_scene(HS, WS, 22))
    want = SceneInferencer(net, "bda", stride=S, batch=7).predict(scene)
    for tta in ((0,), "none"):
        assert _same(want, SceneInferencer(net, "bda", stride=S, batch=7, tta=tta).predict(scene))


# ----------------------------------------------------------------------------------------------- float64 restatement
def _view_outputs(net, task, scene, codes, batch):
    """The model's outputs for every tile under every view, on numpy crops, in `predict`'s batches: list of f64 [n * nv, C, T, T]."""
    x = TR.gather_views(_normalised(R.crops(scene, T, T, S, S)), codes)   # [n * nv, 6, T, T], tile-major, view-minor
    pre, post = torch.from_numpy(x[:, 0:3].copy()).to(DEV), torch.from_numpy(x[:, 3:6].copy()).to(DEV)
    step = (batch // len(codes)) * len(codes)
    outs = []
    with torch.no_grad():
        for j in range(0, len(x), step):
            o = getattr(net, "update_" + task)(pre[j:j + step], post[j:j + step])
            outs.append([t.float().cpu().numpy().astype(np.float64) for t in ([o] if task == "bcd" else o)])
    return [np.concatenate([o[h] for o in outs]) for h in range(len(outs[0]))]


def _restate(values, codes, Hs, Ws, invert=True):
    """dict(blend, lim, taps) of one head from its per-view outputs [n * nv, C, T, T]."""
    nv = len(codes)
    ny, nx = R.plan(Hs, T, S)[1], R.plan(Ws, T, S)[1]
    wy = wx = R.window("hann", T)
    mean = TR.fold64(values, codes, invert=invert)
    abar = TR.fold64(np.abs(values), codes, invert=invert)
    ref = R.stitch(mean.reshape(ny, nx, -1, T, T), Hs, Ws, S, S, wy, wx)
    absw = R.stitch(abar.reshape(ny, nx, -1, T, T), Hs, Ws, S, S, wy, wx)["absw"]
    return dict(blend=ref["blend"], lim=(ref["taps"][None] + 3 + nv) * R.U * absw)


def _decided_mask(ref):
    return np.abs(ref["blend"][0] - 0.5) > ref["lim"][0], (ref["blend"][0] > 0.5).astype(np.uint8)


def _decided_argmax(ref):
    order = np.argsort(ref["blend"], axis=0)
    top, second = order[-1], order[-2]
    take = lambda a, i: np.take_along_axis(a, i[None], axis=0)[0]  # noqa: E731
    return take(ref["blend"], top) - take(ref["blend"], second) > take(ref["lim"], top) + take(ref["lim"], second), top.astype(np.uint8)


def _check_blend(tag, got, ref):
    err = np.abs(got.cpu().numpy().astype(np.float64) - ref["blend"])
    worst = float((err / ref["lim"]).max())
    print(f"PARITY tta {tag}: max |err| {err.max():.3e}  worst err/bound {worst:.3f}")
    assert (err <= ref["lim"]).all(), (tag, worst)
    return err


def _check_against_restatement(net, task, scene, codes, batch, tag):
    """`predict(tta=codes)` against the restatement, every returned map; returns (outputs, per-head restatements)."""
    Hs, Ws = scene.shape[:2]
    out = SceneInferencer(net, task, stride=S, window="hann", batch=batch, tta=codes).predict(torch.from_numpy(scene))
    heads = _view_outputs(net, task, scene, codes, batch)
    refs = [_restate(h, codes, Hs, Ws) for h in heads]
    if task == "bcd":
        prob, mask = out
        _check_blend(f"{tag} bcd prob", prob[None], refs[0])
        decided, want = _decided_mask(refs[0])
        assert 1.0 - decided.mean() <= 1e-3
        assert np.array_equal(mask.cpu().numpy()[decided], want[decided])
        assert torch.equal(mask, (prob > 0.5).to(torch.uint8))
    elif task == "bda":
        loc_prob, loc_mask, damage, logits = out
        _check_blend(f"{tag} bda loc", loc_prob[None], refs[1])
        _check_blend(f"{tag} bda damage logits", logits, refs[0])
        ok_l, want_l = _decided_mask(refs[1])
        assert 1.0 - ok_l.mean() <= 1e-3 and np.array_equal(loc_mask.cpu().numpy()[ok_l], want_l[ok_l])
        assert torch.equal(loc_mask, (loc_prob > 0.5).to(torch.uint8))
        ok, want = _decided_argmax(refs[0])
        ok &= ok_l
        assert 1.0 - ok.mean() <= 1e-3 and np.array_equal(damage.cpu().numpy()[ok], (want * want_l)[ok])
    else:
        pre_cls, post_cls, change = out
        ok_c, want_c = _decided_mask(refs[2])
        assert 1.0 - ok_c.mean() <= 1e-3 and np.array_equal(change.cpu().numpy()[ok_c], want_c[ok_c])
        assert 0 < int(change.sum()) < Hs * Ws
        for got, ref in ((pre_cls, refs[0]), (post_cls, refs[1])):
            ok, want = _decided_argmax(ref)
            ok &= ok_c
            assert 1.0 - ok.mean() <= 1e-3
            assert np.array_equal(got.cpu().numpy()[ok], (want * want_c)[ok])
            assert int((got * (1 - change)).sum()) == 0 and int(got.max()) < NUM_CLASS[task]
    return out, heads, refs


@pytest.mark.parametrize("codes", [TR.SETS["hflip"], TR.SETS["flips"], TR.SETS["d4"], (0, 5)], ids=["hflip", "flips", "d4", "0-5"])
@pytest.mark.parametrize("task", ["bcd", "scd", "bda"])
def test_position_dependent_stub_against_the_float64_restatement(task, codes):
    net = Stub(task, ramp=True).to(DEV)
    scene = _scene(HS, WS, 23)
    batch = 24 if len(codes) == 8 else 10                                 # 3, 5, 2 and 5 tiles per forward: forwards span tile rows
    out, heads, refs = _check_against_restatement(net, task, scene, codes, batch, f"stub {'-'.join(map(str, codes))}")
    if task == "scd":
        return
    # control: the views left as the model returned them (no inverse) are far outside the bound
    got, h = (out[0][None], 0) if task == "bcd" else (out[3], 0)
    v = heads[h].reshape((-1, len(codes)) + heads[h].shape[1:])
    wy = wx = R.window("hann", T)
    raw = R.stitch(v.mean(axis=1).reshape(4, 5, -1, T, T), HS, WS, S, S, wy, wx)
    assert (np.abs(got.cpu().numpy().astype(np.float64) - raw["blend"]) / refs[h]["lim"]).max() > 1e3
    if 5 in codes:                                                        # control: the quarter turn undone by itself, not by its inverse
        swapped = np.stack([TR.inverse(v[:, j], {5: 6, 6: 5}.get(c, c)) for j, c in enumerate(codes)]).mean(axis=0)
        ref = R.stitch(swapped.reshape(4, 5, -1, T, T), HS, WS, S, S, wy, wx)
        assert (np.abs(got.cpu().numpy().astype(np.float64) - ref["blend"]) / refs[h]["lim"]).max() > 1e3


# ------------------------------------------------------------------------------------------------------ real models
def _model(task):
    """The seeded 64 x 64 models of test_scene_infer_gpu.py, built the same way: seeded weights, BatchNorm running statistics
    from one momentum-1 train pass."""
    args = synth.make_args(size=T) if task == "bcd" else synth.make_args(num_perception_frame=3, size=T, dataset="SECOND",
                                                                         num_class=NUM_CLASS["scd"])
    args.act_dtype = torch.float32
    with contextlib.redirect_stdout(io.StringIO()):
        net = Trainer(args)
    net.load_state_dict(synth.synth_state_dict(net, seed=16, mask_margin=0.25))
    net = net.to(DEV).train()
    bns = [m for m in net.modules() if isinstance(m, torch.nn.BatchNorm3d)]
    for m in bns:
        m.momentum = 1.0
    x = _normalised(R.crops(_scene(100, 150, 5), T, T, 32, 32)[:8])
    pre, post = torch.from_numpy(x[:, 0:3].copy()).to(DEV), torch.from_numpy(x[:, 3:6].copy()).to(DEV)
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


@pytest.mark.parametrize("tta,batch", [("flips", 12), ("d4", 24)])
def test_bcd_model_against_the_restatement_of_its_own_view_outputs(bcd_model, tta, batch):
    """3 tiles per forward against 5 tile columns: forwards span tile rows."""
    _check_against_restatement(bcd_model, "bcd", _scene(HS, WS, 2), TR.SETS[tta], batch, f"model {tta}")


@pytest.mark.parametrize("tta,batch", [("flips", 12), ("d4", 24)])
def test_scd_model_against_the_restatement_of_its_own_view_outputs(scd_model, tta, batch):
    _check_against_restatement(scd_model, "scd", _scene(HS, WS, 3), TR.SETS[tta], batch, f"model {tta}")


def test_predict_scene_script_with_tta(bcd_model, tmp_path, capsys):
    from PIL import Image
    from change3d_amd.scripts import predict_scene
    from change3d_amd.utils.metric_tool import ConfuseMatrixMeter
    scene = _scene(HS, WS, 4)
    label = (np.random.default_rng(9).random((HS, WS)) < 0.3).astype(np.uint8) * 255
    Image.fromarray(scene[:, :, 0:3]).save(tmp_path / "a.png")
    Image.fromarray(scene[:, :, 3:6]).save(tmp_path / "b.png")
    Image.fromarray(label).save(tmp_path / "label.png")
    torch.save(bcd_model.state_dict(), tmp_path / "best_model.pth")
    argv = ["--task", "BCD", "--weights", str(tmp_path / "best_model.pth"), "--pre", str(tmp_path / "a.png"), "--post",
            str(tmp_path / "b.png"), "--label", str(tmp_path / "label.png"), "--out_dir", str(tmp_path / "out"), "--stride", "32",
            "--batch_size", "12", "--act_dtype", "f32", "--in_height", str(T), "--in_width", str(T), "--pretrained", "/nonexistent",
            "--tta", "flips"]
    predict_scene.main(argv)
    printed = capsys.readouterr().out
    prob, mask = SceneInferencer(bcd_model, "bcd", stride=32, batch=12, tta="flips").predict(torch.from_numpy(scene))
    plain, _ = SceneInferencer(bcd_model, "bcd", stride=32, batch=12).predict(torch.from_numpy(scene))
    assert not torch.equal(prob, plain)                                   # the views are not the plain prediction
    mask = mask.cpu().numpy()
    back = np.asarray(Image.open(tmp_path / "out" / "scene.png"))
    assert back.dtype == np.uint8 and np.array_equal(back, mask * 255)
    meter = ConfuseMatrixMeter(n_class=2)
    meter.update_cm(mask.astype(np.int64), (label > 0).astype(np.int64))
    s = meter.get_scores()
    got = dict(re.findall(r"(Kappa|IoU|F1|R|P) \(te\) = (-?[0-9.]+)", printed))
    want = {"Kappa": s["Kappa"], "IoU": s["IoU"], "F1": s["F1"], "R": s["recall"], "P": s["precision"]}
    assert got == {k: f"{v:.4f}" for k, v in want.items()}, (got, want)
    with pytest.raises(SystemExit):
        predict_scene.parse_args(argv[:-1] + ["rot90"])
