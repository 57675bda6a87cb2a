"""`SceneInferencer.predict(objects=True, split=R)` on the MI355X with a pixelwise stub model (the pattern of
tests/test_tta_infer_gpu.py): the `SceneObjects` it appends against the restatement of tests/split_reference.py applied to the
device's own stitched maps (exact) for BCD, SCD and BDA, the BDA building votes following the pieces, `split=None` against a
call without the argument, and the refusals.

The scene is drawn so that the stub's mask is a set of shapes, two pairs of which touch: pre R = 255 inside the shapes, post
G = 60 x the class the stub answers there."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import edt_reference as E  # noqa: E402
import split_reference as S  # noqa: E402

from change3d_amd import _lib as L  # noqa: E402
from change3d_amd import ops  # noqa: E402
from change3d_amd.data.transforms import BCDTransforms as BT  # noqa: E402
from change3d_amd.infer import SceneInferencer, SceneObjects, SceneOutlines, SceneSplitObjects  # noqa: E402
from change3d_amd.object_metrics import ObjectEvaluator  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
T, HS, WS = 64, 100, 150
NUM_CLASS = {"bcd": 1, "scd": 7, "bda": 5}
RADIUS = 4.5                                                 # r2 = 20


class Stub(torch.nn.Module):
    """update_*: per pixel; the probability heads answer sigmoid(4 x normalised pre R), the logit heads -(normalised post G -
    the class's centre)^2 with the centre of class c at G = 60 c."""

    def __init__(self, task):
        super().__init__()
        self.args = SimpleNamespace(in_height=T, in_width=T, num_class=NUM_CLASS[task])
        self.decoder_loc = self.decoder_cls = torch.nn.Identity()       # what SceneInferencer asks of a BDA model
        mean, std = BT.DEFAULT_MEAN, BT.DEFAULT_STD
        m, s = (mean[4], std[4]) if len(mean) >= 6 else (mean[1], std[1])
        self.centres = torch.nn.Parameter(torch.tensor([(60.0 * c / 255.0 - m) / s for c in range(7)], dtype=torch.float32))

    def _prob(self, pre):
        return torch.sigmoid(4.0 * pre[:, 0:1])

    def _logits(self, post, C):
        return -(post[:, 1:2] - self.centres[:C].view(1, C, 1, 1)) ** 2

    def update_bcd(self, pre, post):
        return self._prob(pre)

    def update_scd(self, pre, post):
        return self._logits(pre, 7), self._logits(post, 7), self._prob(pre)

    def update_bda(self, pre, post):
        return self._logits(post, 5), self._prob(pre)


def _scene():
    """u8 [HS, WS, 6] and the class map drawn into post G: two overlapping discs of classes 1 and 3, two blocks of classes 2 and
    4 joined by a neck, a lone disc of class 2, a thin bar (no seed) of class 1."""
    shape = (HS, WS)
    parts = [(E.disc(shape, 30, 32, 16), 1), (E.disc(shape, 30, 64, 16), 3), (E.disc(shape, 75, 120, 12), 2)]
    blocks = np.zeros(shape, np.uint8)
    blocks[60:84, 10:34] = 1
    parts.append((blocks.copy(), 2))
    blocks[:] = 0
    blocks[60:84, 44:68] = 1
    blocks[70:73, 34:44] = 1
    parts.append((blocks.copy(), 4))
    bar = np.zeros(shape, np.uint8)
    bar[8:11, 90:140] = 1
    parts.append((bar, 1))
    mask, cls = np.zeros(shape, np.uint8), np.zeros(shape, np.uint8)
    for m, c in parts:
        cls[(m != 0) & (mask == 0)] = c
        mask |= m
    scene = np.random.default_rng(3).integers(0, 40, size=(HS, WS, 6), dtype=np.uint8)
    scene[..., 0] = mask * 255
    scene[..., 1] = cls * 60                                # pre G: the SCD pre classes
    scene[..., 4] = cls * 60
    return scene, mask, cls


def _found(task, out):
    """(mask, cls_map, score, n_cls) that `predict` hands to the objects call, from its own results."""
    if task == "bcd":
        return out[1], None, out[0], 1
    if task == "bda":
        return out[1], out[2], out[0], NUM_CLASS[task]
    return out[2], out[1], None, NUM_CLASS[task]


def _assert_split_objects(objects, want):
    cpu = lambda t: None if t is None else t.cpu().numpy()  # noqa: E731
    assert isinstance(objects, SceneObjects) and isinstance(objects, SceneSplitObjects) and len(objects) == 5
    assert np.array_equal(cpu(objects.counts), want["counts"]), (cpu(objects.counts), want["counts"])
    assert np.array_equal(cpu(objects.labels), want["labels"]) and np.array_equal(cpu(objects.table), want["table"])
    assert np.array_equal(cpu(objects.object_cls), want["object_cls"])
    if want["hist"] is None:
        assert objects.hist is None
    else:
        assert np.array_equal(cpu(objects.hist).astype(np.int64), want["hist"])
    info = objects.info.tolist()
    assert info[:2] == want["info"].tolist() and info[3] == 0 and 1 <= info[2] < 32


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("task", ["bcd", "scd", "bda"])
def test_split_objects_equal_the_restatement_on_the_stitched_mask(task, connectivity):
    scene, drawn, _ = _scene()
    inf = SceneInferencer(Stub(task).to(DEV), task, stride=32, batch=5)
    plain = inf.predict(scene)
    out = inf.predict(torch.from_numpy(scene), objects=True, min_area=2, connectivity=connectivity, max_objects=64, split=RADIUS)
    assert len(out) == len(plain) + 1 and all(torch.equal(a, b) for a, b in zip(plain, out))
    mask, cls_map, score, n_cls = _found(task, out)
    cpu = lambda t: None if t is None else t.cpu().numpy()  # noqa: E731
    assert np.array_equal(cpu(mask), drawn)                                  # the stub answers the drawing
    want = S.split(cpu(mask), ops.boundary_radius2(RADIUS), cpu(cls_map), cpu(score), connectivity=connectivity, min_area=2, n_cls=n_cls,
                   first_class=1, max_objects=64)
    _assert_split_objects(out[-1], want)
    whole = inf.predict(scene, objects=True, min_area=2, connectivity=connectivity, max_objects=64)[-1]
    assert want["counts"].tolist() == [6, 6] and whole.counts.tolist() == [4, 4] and not isinstance(whole, SceneSplitObjects)


def test_bda_building_votes_follow_the_pieces():
    scene, drawn, drawn_cls = _scene()
    inf = SceneInferencer(Stub("bda").to(DEV), "bda", stride=32, batch=5)
    loc_prob, loc_mask, damage, logits, whole = inf.predict(scene, objects=True, max_objects=16)
    split = inf.predict(scene, objects=True, max_objects=16, split=RADIUS)[-1]
    assert np.array_equal(damage.cpu().numpy(), drawn_cls)
    assert whole.table[:4, 5].tolist() == [1, 1, 4, 2]                       # bar; the discs as one building: class 1 has more pixels
    assert split.table[:6, 5].tolist() == [1, 1, 3, 2, 4, 2]                 # bar, disc, disc, block, block with the neck, lone disc
    painted = split.object_cls.cpu().numpy()
    agree = (painted == drawn_cls)[drawn != 0].mean()
    assert agree > 0.97 and (whole.object_cls.cpu().numpy() == drawn_cls)[drawn != 0].mean() < 0.8
    # the pieces go on unchanged: outlines, simplification, object scores
    out = inf.predict(scene, objects=True, max_objects=16, split=RADIUS, outlines=True, simplify=1.0)
    assert isinstance(out[-3], SceneSplitObjects) and isinstance(out[-2], SceneOutlines) and isinstance(out[-1], SceneOutlines)
    assert torch.equal(out[-3].labels, split.labels) and out[-2].counts.tolist()[0] == 6 and out[-2].counts.tolist()[4] == 0
    ev = ObjectEvaluator(n_cls=5, connectivity=8, device=DEV)
    ev.update(split, torch.from_numpy(drawn).to(DEV), torch.from_numpy(drawn_cls).to(DEV))   # the truth is not split: 4 objects
    s = ev.scores()
    assert s["tp"] + s["fp"] == 6 and s["tp"] + s["fn"] == 4


def test_split_none_is_the_call_without_the_argument():
    scene, _, _ = _scene()
    inf = SceneInferencer(Stub("bda").to(DEV), "bda", stride=32, batch=5)
    inf.predict(scene, objects=True, outlines=True)                          # the tables and windows are uploaded
    n0 = ops.launch_count()
    a = inf.predict(scene, objects=True, outlines=True, min_area=2)
    n1 = ops.launch_count()
    b = inf.predict(scene, objects=True, outlines=True, min_area=2, split=None, split_rounds=None)
    n2 = ops.launch_count()
    assert n1 - n0 == n2 - n1 and len(a) == len(b) and type(a[4]) is type(b[4]) is SceneObjects

    def same(x, y):
        if isinstance(x, tuple):
            return len(x) == len(y) and all(same(u, v) for u, v in zip(x, y))
        return (x is None and y is None) or torch.equal(x, y)

    assert same(tuple(a[:5]), tuple(b[:5])) and torch.equal(a[5].rings, b[5].rings) and torch.equal(a[5].counts, b[5].counts)


def test_refusals():
    scene, _, _ = _scene()
    inf = SceneInferencer(Stub("bcd").to(DEV), "bcd", stride=32, batch=5)
    before = ops.launch_count()
    with pytest.raises(ValueError, match="objects=True"):
        inf.predict(scene, split=3)
    with pytest.raises(ValueError):
        inf.predict(scene, objects=True, split=0)
    with pytest.raises(ValueError):
        inf.predict(scene, objects=True, split=1025)
    with pytest.raises(ValueError):
        inf.predict(scene, objects=True, split=2, split_rounds=0)
    with pytest.raises(ValueError):
        inf.predict(scene, objects=True, split_rounds=4)
    assert ops.launch_count() == before
    cut = inf.predict(scene, objects=True, split=RADIUS, split_rounds=1)[-1]
    assert cut.info.tolist()[0] == L.SPLIT_ST_NOT_CONVERGED
    from change3d_amd.scripts.predict_scene import check_split
    with pytest.raises(SystemExit, match="--split_rounds"):
        check_split("scene", cut)
    check_split("scene", inf.predict(scene, objects=True, split=RADIUS)[-1])
    check_split("scene", inf.predict(scene, objects=True)[-1])
