"""`c3d_objects_match` on the MI355X against the restatement of tests/objects_match_reference.py, through `ops.scene_objects` on
both masks and `ops.objects_match`: rows, confusion matrix and integer counts must be EQUAL; `sum_iou` may differ by the bound
of any float64 summation order over correctly rounded quotients, TP * 2^-52 * sum_iou.  Scene widths lie below, at and above
a wave, are no multiples of 4, and a wave's 256 pixels run across row ends.  Then class votes, accumulation over scenes,
`ObjectEvaluator`, bit-identical reruns, the status bits, the refusals, and `predict_scene --objects` with labels end to end."""
import contextlib
import functools
import io
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import objects_match_reference as M  # noqa: E402
import objects_reference as O  # noqa: E402
import scene_reference as SR  # noqa: E402

from change3d_amd import _lib as L  # noqa: E402
from change3d_amd import ops  # noqa: E402
from change3d_amd import synthetic as synth  # noqa: E402
from change3d_amd.data.transforms import BCDTransforms as BT  # noqa: E402
from change3d_amd.infer import SceneInferencer, SceneObjects  # noqa: E402
from change3d_amd.model.trainer import Trainer  # noqa: E402
from change3d_amd.object_metrics import ObjectEvaluator  # noqa: E402
from oracle import transforms as ot  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SIZES = [(5, 1), (9, 63), (20, 64), (37, 65), (40, 130), (70, 257)]
NAMES = [name for name, _, _, _ in M.mask_pairs(2, 2)]
N_CLS = 5
EPS = 2.0 ** -52


@functools.lru_cache(maxsize=None)
def _pairs(size):
    return {name: (p, g, conns) for name, p, g, conns in M.mask_pairs(size[0], size[1], seed=size[0] * 1000 + size[1])}


@functools.lru_cache(maxsize=None)
def _class_maps(size):
    """Two u8 class maps with values past N_CLS."""
    rng = np.random.default_rng(size[0] * 13 + size[1])
    return rng.integers(0, N_CLS + 2, size=size, dtype=np.uint8), rng.integers(0, N_CLS + 2, size=size, dtype=np.uint8)


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@functools.lru_cache(maxsize=None)
def _objects(size, name, conn, with_cls=False, max_p=None):
    """(labels, table, counts) of the prediction and of the ground truth, on the device; computed once and left unchanged."""
    p, g, _ = _pairs(size)[name]
    cls_p, cls_g = _class_maps(size) if with_cls else (None, None)
    rows = size[0] * size[1] // 2 + 1
    kw = dict(connectivity=conn, n_cls=N_CLS if with_cls else 1, first_class=1, want_hist=False, want_object_cls=False)
    a = ops.scene_objects(_dev(p), _dev(cls_p), None, max_objects=max_p or rows, **kw)
    b = ops.scene_objects(_dev(g), _dev(cls_g), None, max_objects=rows, **kw)
    return (a[0], a[1], a[4]), (b[0], b[1], b[4])


def _want(a, b, **kw):
    return M.match(*(t.cpu().numpy() for t in a), *(t.cpu().numpy() for t in b), **kw)


def _assert_equal(got, want, what):
    match_p, match_g, conf, counts, sum_iou = got
    assert match_p.dtype == torch.int32 and torch.equal(match_p.cpu(), torch.from_numpy(want["match_p"])), what
    assert match_g.dtype == torch.int32 and torch.equal(match_g.cpu(), torch.from_numpy(want["match_g"])), what
    assert conf.dtype == torch.int64 and torch.equal(conf.cpu(), torch.from_numpy(want["conf"])), (what, conf, want["conf"])
    assert counts.dtype == torch.int64 and torch.equal(counts.cpu(), torch.from_numpy(want["counts"])), (what, counts, want["counts"])
    tp, s = int(want["counts"][1]), float(sum_iou[0])
    print(f"{what}: counts {counts.tolist()} sum_iou {s!r} restatement {want['sum_iou']!r}")
    assert abs(s - want["sum_iou"]) <= tp * EPS * want["sum_iou"], (what, s, want["sum_iou"])
    rows = match_p.cpu().numpy()
    rows = rows[rows[:, 0] > 0]
    assert (rows[:, 1].astype(np.float64) / rows[:, 2].astype(np.float64)).tolist() == [float(v) for v in want["ious"]], what
    assert int(conf.sum()) == int(counts[1] + counts[2] + counts[3])


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_every_output_equals_the_restatement(size, name):
    for conn in _pairs(size)[name][2]:
        a, b = _objects(size, name, conn)
        got = ops.objects_match(*a, *b)
        assert ops.last_kernel() == "match_finalise_kernel"
        _assert_equal(got, _want(a, b), (size, name, conn))


@pytest.mark.parametrize("thr", [0.5, 0.6, 0.75, 0.999])
def test_other_thresholds(thr):
    for name in ("shift1", "split", "random", "identical"):
        a, b = _objects((40, 130), name, 8)
        _assert_equal(ops.objects_match(*a, *b, iou_thr=thr), _want(a, b, iou_thr=thr), (name, thr))


@pytest.mark.parametrize("name", ["shift1", "split", "merge", "random"])
@pytest.mark.parametrize("size", SIZES[3:], ids=lambda s: f"{s[0]}x{s[1]}")
def test_class_votes_fill_the_confusion_matrix(size, name):
    a, b = _objects(size, name, 8, True)
    got = ops.objects_match(*a, *b, n_cls=N_CLS)
    want = _want(a, b, n_cls=N_CLS)
    _assert_equal(got, want, (size, name))
    assert int(got[2].sum()) == int(want["counts"][1:4].sum()) and (name == "random" or int(got[2][1:, 1:].sum()) > 0)
    narrow = ops.objects_match(*a, *b, n_cls=3)              # classes 3 and 4 of the tables count as 0
    _assert_equal(narrow, _want(a, b, n_cls=3), (size, name, "n_cls 3"))


@pytest.mark.parametrize("scenes", [2, 3])
def test_totals_accumulate_over_scenes(scenes):
    cases = [((40, 130), "shift1"), ((37, 65), "random"), ((70, 257), "split")][:scenes]
    totals = torch.zeros(5 + N_CLS * N_CLS, dtype=torch.int64, device=DEV)
    total_iou = torch.zeros(1, dtype=torch.float64, device=DEV)
    wants = []
    for size, name in cases:
        a, b = _objects(size, name, 8, True)
        ops.objects_match(*a, *b, n_cls=N_CLS, totals=totals, total_iou=total_iou)
        wants.append(_want(a, b, n_cls=N_CLS))
    s = M.scores(wants, N_CLS)
    assert totals[:5].tolist() == [s["tp"], s["fp"], s["fn"], s["pairs"], 0]
    assert torch.equal(totals[5:].cpu().view(N_CLS, N_CLS), torch.from_numpy(s["conf"]))
    sum_iou = sum(w["sum_iou"] for w in wants)
    assert abs(float(total_iou[0]) - sum_iou) <= (s["tp"] + scenes) * EPS * sum_iou


def test_object_evaluator_scores_equal_the_restatement():
    cases = [((40, 130), "shift1"), ((37, 65), "random"), ((70, 257), "merge")]
    ev = ObjectEvaluator(n_cls=N_CLS, iou_thr=0.5, connectivity=8, device=DEV)
    wants = []
    for size, name in cases:
        (labels, table, counts), b = _objects(size, name, 8, True)
        _, g, _ = _pairs(size)[name]
        match_p, match_g = ev.update(SceneObjects(labels, table, counts, None, None), _dev(g), _dev(_class_maps(size)[1]))
        want = _want((labels, table, counts), b, n_cls=N_CLS)
        wants.append(want)
        rows_g = int(b[2][1])
        assert torch.equal(match_p.cpu(), torch.from_numpy(want["match_p"]))
        assert torch.equal(match_g[:rows_g].cpu(), torch.from_numpy(want["match_g"][:rows_g])) and not bool(match_g[rows_g:].any())
    got, want = ev.scores(), M.scores(wants, N_CLS)
    assert ev.scenes == 3 and got["tp"] > 0 and got["fp"] > 0 and got["fn"] > 0
    for k in ("tp", "fp", "fn", "pairs", "status", "precision", "recall", "f1", "rq", "class_f1"):
        assert got[k] == want[k], (k, got[k], want[k])
    assert np.array_equal(got["conf"], want["conf"])
    assert abs(got["sq"] - want["sq"]) <= (got["tp"] + 4) * EPS * want["sq"] and abs(got["pq"] - want["pq"]) <= (got["tp"] + 6) * EPS * want["pq"]
    ev.reset()
    assert ev.scores()["tp"] == 0 and ev.scores()["pq"] == 0.0


def test_two_runs_agree_bit_for_bit():
    for size, name, conn in (((70, 257), "random", 8), ((70, 257), "checker_vs_full", 4), ((40, 130), "shift1", 8)):
        a, b = _objects(size, name, conn)
        x, y = ops.objects_match(*a, *b), ops.objects_match(*a, *b)
        torch.cuda.synchronize()
        assert all(torch.equal(u, v) for u, v in zip(x, y)) and x[4].view(torch.int64).item() == y[4].view(torch.int64).item()


def test_a_full_table_sets_its_status_bit_and_returns():
    a, b = _objects((40, 130), "stripes", 4)
    want = _want(a, b)
    assert want["counts"][0] == 1300
    got = ops.objects_match(*a, *b, table_capacity=64)
    torch.cuda.synchronize()
    counts = got[3].tolist()
    assert counts[4] == M.ST_TABLE_FULL and counts[0] == 64 and counts[5] == 0
    _assert_equal(ops.objects_match(*a, *b, table_capacity=2048), want, "stripes in 2048 slots")     # 1300 pairs fit
    ev = ObjectEvaluator(connectivity=4, device=DEV, table_capacity=64)
    ev.update(SceneObjects(*a, None, None), _dev(_pairs((40, 130))["stripes"][1]))
    with pytest.raises(L.Change3DHipError, match="pair table full"):
        ev.scores()


@pytest.mark.parametrize("name", ["shift1", "random", "checker_vs_full"])
def test_truncation_at_three_predicted_objects(name):
    size = (40, 130)
    a, b = _objects(size, name, 4, False, 3)
    assert tuple(a[1].shape) == (3, 8) and int(a[2][0]) > 3 and int(a[2][1]) == 3 and int(a[0].max()) > 3
    got = ops.objects_match(*a, *b)
    want = _want(a, b)
    assert want["counts"][4] == M.ST_TRUNCATED and tuple(got[0].shape) == (3, 4)
    _assert_equal(got, want, name)                          # the surviving rows: ids past the table are background
    ev = ObjectEvaluator(connectivity=4, device=DEV)
    ev.update(SceneObjects(*a, None, None), _dev(_pairs(size)[name][1]))
    with pytest.raises(L.Change3DHipError, match="max_objects"):
        ev.scores()


def test_refusals_return_their_error_and_launch_nothing():
    lib = L.lib()
    (lp, tp_, cp), (lg, tg, cg) = _objects((20, 64), "shift1", 8)
    H, W = 20, 64
    rows = tp_.shape[0]
    match_p = torch.full((rows, 4), -7, dtype=torch.int32, device=DEV)
    match_g = torch.full((rows, 4), -7, dtype=torch.int32, device=DEV)
    conf = torch.full((16 * 16,), -7, dtype=torch.int64, device=DEV)
    counts = torch.full((6,), -7, dtype=torch.int64, device=DEV)
    sum_iou = torch.full((1,), -7.0, dtype=torch.float64, device=DEV)
    nbytes, cap = ops.objects_match_plan(H, W)
    assert cap == 4096 and nbytes == 256 + 12 * cap
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    p = lambda t: None if t is None else t.data_ptr()  # noqa: E731

    def call(thr=0.5, n_cls=1, capacity=cap, Hs=H, Ws=W, max_p=rows, max_g=rows, match_p=match_p, match_g=match_g, conf=conf,
             counts=counts, sum_iou=sum_iou, ws=ws, labels_p=lp):
        return lib.c3d_objects_match(p(labels_p), p(tp_), p(cp), p(lg), p(tg), p(cg), Hs, Ws, max_p, max_g, n_cls, thr, capacity,
                                     p(match_p), p(match_g), p(conf), p(counts), p(sum_iou), None, None, p(ws), None)

    before = ops.launch_count()
    for thr in (0.49, 1.0, float("nan"), -1.0, 0.0, 2.0):
        assert call(thr=thr) == -1                                   # C3D_E_BADARG
    assert call(n_cls=17) == -1 and call(n_cls=0) == -1
    assert call(capacity=48) == -1 and call(capacity=-64) == -1 and call(capacity=0) == -1
    assert call(max_p=0) == -1 and call(max_g=0) == -1
    assert call(match_p=None) == -1 and call(match_g=None) == -1 and call(conf=None) == -1 and call(counts=None) == -1
    assert call(sum_iou=None) == -1 and call(ws=None) == -1 and call(labels_p=None) == -1
    assert call(Hs=65536, Ws=32768) == -2                            # C3D_E_UNSUPPORTED: Hs * Ws = 2^31
    cap_io = L.i64(48)
    assert lib.c3d_objects_match_ws_bytes(H, W, cap_io) == -1 and lib.c3d_objects_match_ws_bytes(65536, 32768, L.i64(0)) == -2
    assert lib.c3d_objects_match_ws_bytes(0, W, L.i64(0)) == -1 and lib.c3d_objects_match_ws_bytes(H, W, None) == -1
    torch.cuda.synchronize()
    assert ops.launch_count() == before
    for t in (match_p, match_g, conf, counts):
        assert int((t != -7).sum()) == 0                             # nothing was written
    for bad in (dict(iou_thr=0.49), dict(iou_thr=1.0), dict(iou_thr=float("nan")), dict(n_cls=17), dict(table_capacity=48)):
        with pytest.raises(L.Change3DHipError):
            ops.objects_match(lp, tp_, cp, lg, tg, cg, **bad)
    with pytest.raises(ValueError):
        ObjectEvaluator(iou_thr=0.49, device=DEV)
    assert call() == 0                                               # the same arguments, accepted
    torch.cuda.synchronize()
    want = _want((lp, tp_, cp), (lg, tg, cg))
    assert ops.launch_count() == before + 4 and counts.tolist() == want["counts"].tolist() and conf[0].item() == want["conf"][0, 0]
    assert conf[1].item() == -7                                      # n_cls = 1: a single cell


# ---------------------------------------------------------------------------------------- predict_scene end to end
T = 64


def _scene(Hs, Ws, seed):
    return np.random.default_rng(seed).integers(0, 256, size=(Hs, Ws, 6), dtype=np.uint8)


def _model(task):
    """Seeded weights; BatchNorm running statistics of one momentum-1 train pass, as in test_scene_bda_gpu.py."""
    args = {"bcd": lambda: synth.make_args(size=T),
            "bda": lambda: synth.make_args(num_perception_frame=2, size=T, dataset="xBD", num_class=N_CLS)}[task]()
    args.act_dtype = torch.float32
    with contextlib.redirect_stdout(io.StringIO()):
        net = Trainer(args)
    net.load_state_dict(synth.synth_state_dict(net, seed=16, mask_margin=0.25))
    net = net.to(DEV).train()
    bns = [m for m in net.modules() if isinstance(m, torch.nn.BatchNorm3d)]
    for m in bns:
        m.momentum = 1.0
    crops = SR.crops(_scene(100, 150, 5), T, T, 32, 32)[:8]
    img = np.stack([ot.bcd_transform_sample(c, np.zeros(c.shape[:2], np.uint8), (0, 0, 0), BT.DEFAULT_MEAN, BT.DEFAULT_STD)[0]
                    for c in crops])
    with torch.no_grad():
        getattr(net, "update_" + task)(torch.from_numpy(img[:, 0:3]).to(DEV), torch.from_numpy(img[:, 3:6]).to(DEV))
    for m in bns:
        m.momentum = 0.1
    ops.bump_weights_version()
    return net.eval()


def _object_line(s, per_class):
    line = (f"objects: tp = {s['tp']} fp = {s['fp']} fn = {s['fn']} precision = {s['precision']:.4f} recall = {s['recall']:.4f} "
            f"f1 = {s['f1']:.4f} sq = {s['sq']:.4f} rq = {s['rq']:.4f} pq = {s['pq']:.4f}")
    return line + (f" class_f1 = [{', '.join(f'{v:.4f}' for v in s['class_f1'])}]" if per_class else "")


def _assert_match_csv(path, want, rows_p, rows_g):
    lines = path.read_text().splitlines()
    assert lines[0] == "id,gt_id,inter,union,covered" and lines[1 + rows_p:3 + rows_p] == ["# gt", "id,pred_id,inter,union,covered"]
    assert len(lines) == 3 + rows_p + rows_g
    assert [[int(v) for v in l.split(",")] for l in lines[1:1 + rows_p]] == [[k + 1] + r for k, r in enumerate(want["match_p"][:rows_p].tolist())]
    assert [[int(v) for v in l.split(",")] for l in lines[3 + rows_p:]] == [[k + 1] + r for k, r in enumerate(want["match_g"][:rows_g].tolist())]


def _restated(objects, gt_mask, gt_cls, n_cls):
    """The restatement applied to the downloaded maps of the prediction and to the labels of the ground truth."""
    gt = O.objects(gt_mask, gt_cls, None, connectivity=8, min_area=1, n_cls=n_cls, first_class=1, max_objects=65536)
    want = M.match(objects.labels.cpu().numpy(), objects.table.cpu().numpy(), objects.counts.cpu().numpy(), gt["labels"], gt["table"],
                   gt["counts"], n_cls=n_cls)
    return want, int(objects.counts[1]), int(gt["counts"][1])


def test_predict_scene_bcd_object_scores_end_to_end(tmp_path, capsys):
    from PIL import Image
    from change3d_amd.scripts import predict_scene
    net = _model("bcd")
    Hs, Ws = 100, 150
    scene = _scene(Hs, Ws, 4)
    label = (np.random.default_rng(9).random((Hs, Ws)) < 0.3).astype(np.uint8) * 255
    Image.fromarray(scene[:, :, 0:3]).save(tmp_path / "a.png")
    Image.fromarray(scene[:, :, 3:6]).save(tmp_path / "b.png")
    Image.fromarray(label).save(tmp_path / "label.png")
    torch.save(net.state_dict(), tmp_path / "best_model.pth")
    argv = ["--task", "BCD", "--weights", str(tmp_path / "best_model.pth"), "--pre", str(tmp_path / "a.png"), "--post",
            str(tmp_path / "b.png"), "--stride", "32", "--batch_size", "5", "--act_dtype", "f32", "--in_height", str(T), "--in_width",
            str(T), "--pretrained", "/nonexistent", "--objects"]
    predict_scene.main(argv + ["--out_dir", str(tmp_path / "plain")])
    plain = capsys.readouterr().out
    predict_scene.main(argv + ["--out_dir", str(tmp_path / "scored"), "--label", str(tmp_path / "label.png")])
    scored = capsys.readouterr().out
    assert "objects:" not in plain and not (tmp_path / "plain" / "objects" / "scene.match.csv").exists()
    for f in ("scene.png", os.path.join("objects", "scene.csv")):    # what does not depend on the labels
        assert (tmp_path / "plain" / f).read_bytes() == (tmp_path / "scored" / f).read_bytes()
    _, _, objects = SceneInferencer(net, "bcd", stride=32, batch=5).predict(torch.from_numpy(scene), objects=True)
    want, rows_p, rows_g = _restated(objects, label, None, 1)
    lines = scored.splitlines()
    k = [i for i, l in enumerate(lines) if l.startswith("Test:")]
    assert len(k) == 1 and lines[k[0] + 1] == _object_line(M.scores([want], 1), False) and rows_g > 0
    _assert_match_csv(tmp_path / "scored" / "objects" / "scene.match.csv", want, rows_p, rows_g)


def test_predict_scene_bda_object_scores_end_to_end(tmp_path, capsys):
    from PIL import Image
    from change3d_amd.scripts import predict_scene
    net = _model("bda")
    Hs, Ws = 100, 150
    scene = _scene(Hs, Ws, 4)
    rng = np.random.default_rng(9)
    loc = (rng.random((Hs, Ws)) < 0.4).astype(np.uint8)
    dmg = rng.integers(1, N_CLS, size=(Hs, Ws), dtype=np.uint8)
    name = "guatemala-volcano_00000000_post_disaster.png"
    for sub in ("t1", "t2", "label1", "label2"):
        os.makedirs(tmp_path / "test" / sub)
    Image.fromarray(scene[:, :, 0:3]).save(tmp_path / "test" / "t1" / name)
    Image.fromarray(scene[:, :, 3:6]).save(tmp_path / "test" / "t2" / name)
    Image.fromarray(loc).save(tmp_path / "test" / "label1" / name.replace("disaster", "disaster_target"))
    Image.fromarray(dmg).save(tmp_path / "test" / "label2" / name.replace("disaster", "disaster_target"))
    torch.save(net.state_dict(), tmp_path / "best_model.pth")
    out = tmp_path / "out"
    predict_scene.main(["--task", "BDA", "--objects", "--min_area", "2", "--iou_thr", "0.5", "--weights", str(tmp_path / "best_model.pth"),
                        "--file_root", str(tmp_path), "--split", "test", "--out_dir", str(out), "--stride", "32", "--batch_size", "5",
                        "--act_dtype", "f32", "--in_height", str(T), "--in_width", str(T), "--pretrained", "/nonexistent"])
    printed = capsys.readouterr().out
    bgr = np.concatenate((scene[:, :, 2::-1], scene[:, :, :2:-1]), axis=2)             # BDADataset reads in cv2's channel order
    objects = SceneInferencer(net, "bda", stride=32, batch=5).predict(np.ascontiguousarray(bgr), objects=True, min_area=2)[-1]
    want, rows_p, rows_g = _restated(objects, loc, loc * dmg, N_CLS)
    lines = printed.splitlines()
    k = [i for i, l in enumerate(lines) if l.startswith("Objects:")]
    assert len(k) == 1 and lines[k[0] + 1] == _object_line(M.scores([want], N_CLS), True) and rows_g > 0
    stem = os.path.splitext(name)[0]
    _assert_match_csv(out / "objects" / (stem + ".match.csv"), want, rows_p, rows_g)
    # the same pair without labels: what does not depend on them is byte for byte the same, and nothing is scored
    plain = tmp_path / "plain"
    predict_scene.main(["--task", "BDA", "--objects", "--min_area", "2", "--weights", str(tmp_path / "best_model.pth"), "--pre",
                        str(tmp_path / "test" / "t1" / name), "--post", str(tmp_path / "test" / "t2" / name), "--out_dir", str(plain),
                        "--stride", "32", "--batch_size", "5", "--act_dtype", "f32", "--in_height", str(T), "--in_width", str(T),
                        "--pretrained", "/nonexistent"])
    unlabelled = capsys.readouterr().out
    assert "objects:" not in unlabelled and "Objects:" not in unlabelled and "Test:" not in unlabelled
    assert not (plain / "objects" / "scene.match.csv").exists()
    for sub, ext in (("loc", ".png"), ("damage", ".png"), ("damage_objects", ".png"), ("objects", ".csv")):
        assert (plain / sub / ("scene" + ext)).read_bytes() == (out / sub / (stem + ext)).read_bytes(), sub
