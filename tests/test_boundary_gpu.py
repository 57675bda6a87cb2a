"""`c3d_boundary_counts` against its restatement (tests/edt_reference.py): all eight counts equal, on discs, identical, disjoint
and empty masks, a quarter disc at the scene's corner with and without the border, and random blobs; `totals` over three calls,
the refusals, `BoundaryEvaluator`, and `predict_scene --boundary` end to end."""
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import edt_reference as R  # noqa: E402

from change3d_amd import _lib as L  # noqa: E402
from change3d_amd import ops  # noqa: E402
from change3d_amd.boundary_metrics import BoundaryEvaluator, scores_from_totals  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CANARY = -7777
RADII = ((1, 1), (2, 2), (5, 3))                           # (d, tau)


def _blobs(shape, seed, level):
    """A thresholded smooth field: what a change map looks like."""
    rng = np.random.default_rng(seed)
    field = rng.standard_normal((shape[0] // 8 + 2, shape[1] // 8 + 2))
    field = np.kron(field, np.ones((8, 8)))[:shape[0], :shape[1]]
    for _ in range(3):                                      # a few box blurs round the blocks off
        field = (field + np.roll(field, 1, 0) + np.roll(field, -1, 0) + np.roll(field, 1, 1) + np.roll(field, -1, 1)) / 5
    return (field > level).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def _cases():
    """name -> (pred, gt, border)."""
    S = (96, 120)
    A, B, empty = R.disc(S, 40, 50, 25), R.disc(S, 42, 53, 25), np.zeros(S, np.uint8)
    quarter_p, quarter_g = R.disc((40, 50), 0, 0, 20), R.disc((40, 50), 0, 0, 23)
    return {"two_discs": (A, B, True), "identical": (A, A, True), "disjoint": (R.disc(S, 30, 30, 12), R.disc(S, 60, 90, 14), True),
            "empty_prediction": (empty, B, True), "empty_ground_truth": (A, empty, True), "both_empty": (empty, empty, True),
            "quarter_disc_border": (quarter_p, quarter_g, True), "quarter_disc_no_border": (quarter_p, quarter_g, False),
            "random_blobs": (_blobs((130, 190), 1, 0.1) * 255, _blobs((130, 190), 2, 0.1), True),
            "random_blobs_no_border": (_blobs((130, 190), 3, -0.2), _blobs((130, 190), 4, 0.0) * 9, False)}


@functools.lru_cache(maxsize=None)
def _want(name, d, tau):
    pred, gt, border = _cases()[name]
    return R.boundary_counts(pred, gt, d * d, tau * tau, border)


def _counts(pred, gt, d2, tau2, flags, totals=None, fill_ws=None):
    """The C entry on a counts buffer with canaries on both sides: (rc, counts as a tuple)."""
    Hs, Ws = pred.shape
    d_pred, d_gt = (torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in (pred, gt))
    out = torch.full((8 + 4,), CANARY, dtype=torch.int64, device=DEV)
    ws = torch.empty(L.lib().c3d_boundary_counts_ws_bytes(Hs, Ws), dtype=torch.uint8, device=DEV)
    if fill_ws is not None:
        ws.fill_(fill_ws)
    rc = L.lib().c3d_boundary_counts(d_pred.data_ptr(), d_gt.data_ptr(), Hs, Ws, d2, tau2, flags, out[2:].data_ptr(),
                                     None if totals is None else totals.data_ptr(), ws.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    out = out.tolist()
    assert out[:2] == [CANARY] * 2 and out[10:] == [CANARY] * 2, "a canary was written"
    return rc, tuple(out[2:10])


@pytest.mark.parametrize("radii", RADII)
@pytest.mark.parametrize("name", list(_cases()))
def test_counts_equal_the_restatement(name, radii):
    pred, gt, border = _cases()[name]
    d, tau = radii
    rc, got = _counts(pred, gt, d * d, tau * tau, L.EDT_BORDER if border else 0, fill_ws=0xFF if d == 2 else None)
    assert rc == 0 and got == _want(name, d, tau), (got, _want(name, d, tau))
    if name == "two_discs" and d == tau:
        assert got[:6] == {1: (10, 270, 140, 29, 140, 29), 2: (38, 514, 140, 69, 140, 69)}[d]
    if name == "identical":
        assert got[0] == got[1] > 0 and got[2] == got[3] == got[4] == got[5] == 140
    if name == "disjoint":
        assert got[0] == 0 and got[3] == got[5] == 0 and got[2] > 0 and got[4] > 0
    if name == "both_empty":
        assert got == (0, 0, 0, 0, 0, 0, 1, 0)
    if name == "empty_prediction":
        assert got[0] == got[2] == got[3] == got[5] == 0 and got[1] > 0 and got[4] == 140


def test_the_border_changes_the_counts_of_a_quarter_disc():
    for d, tau in RADII:
        with_border, without = _want("quarter_disc_border", d, tau), _want("quarter_disc_no_border", d, tau)
        assert with_border[1] > without[1] and with_border[2] > without[2] and with_border[4] > without[4]


def test_totals_accumulate_in_stream_order():
    totals = torch.zeros(8, dtype=torch.int64, device=DEV)
    want = np.zeros(8, dtype=np.int64)
    for name, (d, tau) in (("two_discs", (2, 2)), ("random_blobs", (5, 3)), ("quarter_disc_no_border", (1, 1))):
        pred, gt, border = _cases()[name]
        counts = ops.boundary_counts(*(torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in (pred, gt)), d, tau, border=border,
                                     totals=totals)
        assert counts.dtype == torch.int64 and tuple(counts.tolist()) == _want(name, d, tau)
        want += np.array(_want(name, d, tau))
    assert totals.tolist() == want.tolist() and totals[6].item() == 3


def test_two_runs_agree_on_a_non_default_stream():
    pred, gt, _ = _cases()["random_blobs"]
    d_pred, d_gt = (torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in (pred, gt))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        a = ops.boundary_counts(d_pred, d_gt, 5, 3)
        b = ops.boundary_counts(d_pred, d_gt, 5, 3)
        c = ops.boundary_counts(d_pred, d_gt, 5.9, 3.9)      # floor(5.9^2) = 34, floor(3.9^2) = 15
    side.synchronize()
    assert tuple(a.tolist()) == tuple(b.tolist()) == _want("random_blobs", 5, 3)
    assert tuple(c.tolist()) == R.boundary_counts(pred, gt, 34, 15, True)


def test_refusals_leave_the_outputs_untouched():
    pred, gt, _ = _cases()["two_discs"]
    Hs, Ws = pred.shape
    d_pred, d_gt = (torch.from_numpy(a).to(DEV) for a in (pred, gt))
    counts = torch.full((8,), CANARY, dtype=torch.int64, device=DEV)
    totals = torch.full((8,), CANARY, dtype=torch.int64, device=DEV)
    ws = torch.empty(L.lib().c3d_boundary_counts_ws_bytes(Hs, Ws), dtype=torch.uint8, device=DEV)
    good = dict(pred=d_pred.data_ptr(), gt=d_gt.data_ptr(), Hs=Hs, Ws=Ws, d2=4, tau2=4, flags=L.EDT_BORDER, counts=counts.data_ptr(),
                totals=totals.data_ptr(), ws=ws.data_ptr())
    stream = torch.cuda.current_stream().cuda_stream
    before = ops.launch_count()
    bad = [(dict(pred=None), -1), (dict(gt=None), -1), (dict(counts=None), -1), (dict(ws=None), -1), (dict(d2=0), -1), (dict(d2=-4), -1),
           (dict(d2=(1 << 20) + 1), -1), (dict(tau2=0), -1), (dict(tau2=(1 << 20) + 1), -1), (dict(flags=L.EDT_INVERT), -1),
           (dict(flags=4), -1), (dict(Hs=0), -1), (dict(Ws=-1), -1), (dict(Hs=16385), -2), (dict(Ws=16385), -2)]
    for change, code in bad:
        assert L.lib().c3d_boundary_counts(*{**good, **change}.values(), stream) == code, change
    torch.cuda.synchronize()
    assert ops.launch_count() == before and (counts == CANARY).all() and (totals == CANARY).all()
    totals.zero_()
    assert L.lib().c3d_boundary_counts(*{**good, "totals": None}.values(), stream) == 0                 # totals may be NULL
    assert L.lib().c3d_boundary_counts(*{**good, "d2": 1 << 20, "tau2": 1 << 20}.values(), stream) == 0  # the largest radii
    torch.cuda.synchronize()
    assert ops.launch_count() == before + 16
    assert tuple(counts.tolist()) == tuple(totals.tolist()) == R.boundary_counts(pred, gt, 1 << 20, 1 << 20, True)
    for bad_radius in (0, 0.5, -2, 1025, float("nan")):
        with pytest.raises(ValueError):
            ops.boundary_counts(d_pred, d_gt, bad_radius)
        with pytest.raises(ValueError):
            ops.boundary_counts(d_pred, d_gt, 2, bad_radius)
        with pytest.raises(ValueError):
            BoundaryEvaluator(bad_radius, device=DEV)
    with pytest.raises(L.Change3DHipError):
        ops.boundary_counts(d_pred.cpu(), d_gt, 2)
    with pytest.raises(ValueError):
        ops.boundary_counts(d_pred, d_gt[:50], 2)
    assert ops.launch_count() == before + 16


def test_evaluator_accumulates_without_a_synchronisation():
    ev = BoundaryEvaluator(5, tau=3, device=DEV)
    names = ("two_discs", "random_blobs", "identical")
    pairs = [tuple(torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in _cases()[n][:2]) for n in names]
    ev.update(*pairs[0])                                     # the first call loads the kernels
    ev.reset()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")                  # a synchronising call raises
    try:
        for pred, gt in pairs:
            ev.update(pred, gt)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    got = ev.scores()
    total = np.sum([_want(n, 5, 3) for n in names], axis=0)
    want = scores_from_totals(total.tolist())
    assert got == want and got["scenes"] == 3 == ev.scenes and 0 < got["boundary_iou"] < 1 and 0 < got["boundary_f1"] <= 1
    ev.reset()
    assert ev.scores()["boundary_f1"] == 0.0 and ev.scores()["union"] == 0
    with pytest.raises(ValueError):
        ev.update(pairs[0][0].cpu(), pairs[0][1])


# ---------------------------------------------------------------------------------------- predict_scene end to end
@pytest.fixture(scope="module")
def bcd_model():
    from test_scene_bda_gpu import _model
    return _model("bcd")


def test_predict_scene_boundary_in_a_child_process(bcd_model, tmp_path):
    from PIL import Image
    from test_scene_bda_gpu import T, _scene
    scene = _scene(70, 90, 4)
    label = _blobs((70, 90), 7, 0.0) * 255
    Image.fromarray(scene[:, :, 0:3]).save(tmp_path / "a.png")
    Image.fromarray(scene[:, :, 3:6]).save(tmp_path / "b.png")
    Image.fromarray(label).save(tmp_path / "label.png")
    torch.save(bcd_model.state_dict(), tmp_path / "best_model.pth")
    runs = {}
    for name, extra in (("plain", []), ("boundary", ["--boundary", "2"])):
        cmd = [sys.executable, "-m", "change3d_amd.scripts.predict_scene", "--task", "BCD", "--weights", str(tmp_path / "best_model.pth"),
               "--pre", str(tmp_path / "a.png"), "--post", str(tmp_path / "b.png"), "--label", str(tmp_path / "label.png"), "--stride", "32",
               "--batch_size", "5", "--act_dtype", "f32", "--in_height", str(T), "--in_width", str(T), "--pretrained", "/nonexistent",
               "--out_dir", str(tmp_path / name), "--objects"] + extra
        done = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
        assert done.returncode == 0, done.stderr[-3000:] + done.stdout[-2000:]
        runs[name] = done.stdout
    files = lambda name: {os.path.relpath(os.path.join(d, f), tmp_path / name): open(os.path.join(d, f), "rb").read()  # noqa: E731
                          for d, _, fs in os.walk(tmp_path / name) for f in fs}
    assert files("plain") == files("boundary") and len(files("plain")) >= 3
    assert "boundary:" not in runs["plain"]
    strip = lambda text: [ln for ln in text.replace(str(tmp_path), "").splitlines() if not ln.startswith("boundary:")]  # noqa: E731
    assert [ln.replace("/boundary", "/plain") for ln in strip(runs["boundary"])] == strip(runs["plain"])
    mask = np.asarray(Image.open(tmp_path / "plain" / "scene.png"))
    assert 0 < (mask > 0).sum() < mask.size
    for name, d, tau in (("boundary", 2.0, 2.0),):
        lines = runs[name].splitlines()
        at = [k for k, ln in enumerate(lines) if ln.startswith("boundary:")]
        assert len(at) == 1 and lines[at[0] - 1].startswith("objects:"), lines[-4:]
        got = dict(re.findall(r"(\w+) = ([0-9.]+)", lines[at[0]]))
        s = scores_from_totals(R.boundary_counts(mask, label, int(d * d), int(tau * tau), True))
        want = dict(d=f"{d:g}", tol=f"{tau:g}", biou=f"{s['boundary_iou']:.4f}", precision=f"{s['boundary_precision']:.4f}",
                    recall=f"{s['boundary_recall']:.4f}", f1=f"{s['boundary_f1']:.4f}")
        assert got == want, (lines[at[0]], want)
