"""`c3d_scene_split` on the MI355X against the restatement of tests/split_reference.py, through the C entry with canary rows
around every output: labels, table, hist, object_cls, counts and info[0:2] must be EQUAL (all arithmetic is integer).  Scene
sizes sit around the multiples of the growth tile (`ops.scene_split_tile()`); the masks are those of
`objects_reference.mask_list` and the hand-made cases of the restatement."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import objects_match_reference as M  # noqa: E402
import objects_reference as R  # noqa: E402
import outlines_reference as O  # noqa: E402
import split_reference as S  # noqa: E402

from change3d_amd import _lib as L  # noqa: E402
from change3d_amd import ops  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
T = ops.scene_split_tile()[0]
assert ops.scene_split_tile() == (T, T)
PAD, CANARY = 2, -77
N_CLS = 5
OTHER = 70                                                   # the extent of the axis that a "rows:" / "cols:" shape does not vary
SHAPES = {"1x1": (1, 1), "1x37": (1, 37), "37x1": (37, 1), "37x53": (37, 53)}
for _k, _v in (("T-1", T - 1), ("T", T), ("T+1", T + 1), ("2T+3", 2 * T + 3)):
    SHAPES["rows:" + _k] = (_v, OTHER)
    SHAPES["cols:" + _k] = (OTHER, _v)
SHAPES["2T+3x2T+3"] = (2 * T + 3, 2 * T + 3)
MASKS = [name for name, _ in R.mask_list(2, 2, T, T)]
R2S = (0, 1, 4, 25)


@functools.lru_cache(maxsize=None)
def _masks(shape):
    return dict(R.mask_list(shape[0], shape[1], T, T, seed=shape[0] * 1000 + shape[1]))


@functools.lru_cache(maxsize=None)
def _side_inputs(shape):
    rng = np.random.default_rng(shape[0] * 7 + shape[1])
    cls = rng.integers(0, N_CLS + 2, size=shape, dtype=np.uint8)
    score = rng.random(shape, dtype=np.float32) * 1.2 - 0.1
    score[rng.random(shape) < 0.05] = np.nan
    return cls, score


def _grow(mask, r2, connectivity):
    """(labels0 of the pieces before the area filter, number of seeds, depth) of the restatement."""
    ids, n_seeds = S.seed_ids(S.core_of(mask, r2), connectivity)
    d, owner = S.grow_dijkstra(mask, ids, connectivity)
    return S.piece_labels(mask, owner, connectivity), n_seeds, int(d.max()) if d.size else 0


@functools.lru_cache(maxsize=None)
def _grown_list(shape, name, r2, connectivity):
    return _grow(_masks(shape)[name], r2, connectivity)


@functools.lru_cache(maxsize=None)
def _grown_hand(i, connectivity, r2=None):
    name, mask, r2_case = S.hand_cases()[i]
    return _grow(mask, r2_case if r2 is None else r2, connectivity)


def _want(mask, grown, cls=None, score=None, **kw):
    out = R.objects(mask, cls, score, labels0=grown[0], **kw)
    out["info"] = np.array([0, grown[1]], dtype=np.int32)
    return out


def _guarded(rows, cols, dtype):
    """A [rows, cols] device tensor with PAD canary rows on both sides: (whole, view)."""
    whole = torch.full((rows + 2 * PAD, cols), _canary(dtype), dtype=dtype, device=DEV)
    return whole, whole[PAD:PAD + rows]


def _canary(dtype):
    return CANARY & 0xff if str(dtype).endswith("uint8") else CANARY    # torch and numpy dtypes


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _split(mask, r2, cls=None, score=None, connectivity=8, min_area=1, n_cls=1, first_class=1, max_objects=None, max_rounds=4096,
           ws=None, fill_ws=None, stream=None):
    """The C entry: (rc, dict of numpy outputs); asserts that no canary row was written."""
    Hs, Ws = mask.shape
    max_objects = Hs * Ws // 2 + 1 if max_objects is None else max_objects
    d_mask, d_cls, d_score = _dev(mask), _dev(cls), _dev(score)
    bufs = dict(labels=_guarded(Hs, Ws, torch.int32), table=_guarded(max_objects, 8, torch.int32),
                hist=_guarded(max_objects, n_cls, torch.int32), object_cls=_guarded(Hs, Ws, torch.uint8),
                counts=_guarded(1, 2, torch.int32), info=_guarded(1, 4, torch.int32))
    if ws is None:
        ws = torch.empty(L.lib().c3d_scene_split_ws_bytes(Hs, Ws, n_cls if cls is not None else 1), dtype=torch.uint8, device=DEV)
    if fill_ws is not None:
        ws.fill_(fill_ws)
    p = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    st = torch.cuda.current_stream().cuda_stream if stream is None else stream.cuda_stream
    rc = L.lib().c3d_scene_split(p(d_mask), p(d_cls), p(d_score), Hs, Ws, connectivity, min_area, n_cls, first_class, max_objects, r2,
                                 max_rounds, p(bufs["labels"][1]), p(bufs["table"][1]), p(bufs["hist"][1]) if cls is not None else None,
                                 p(bufs["object_cls"][1]), p(bufs["counts"][1]), p(bufs["info"][1]), p(ws), st)
    torch.cuda.synchronize()
    out = {}
    for k, (whole, view) in bufs.items():
        w = whole.cpu().numpy()
        rows = view.shape[0]
        assert (w[:PAD] == _canary(w.dtype)).all() and (w[PAD + rows:] == _canary(w.dtype)).all(), f"a canary row of {k} was written"
        out[k] = w[PAD:PAD + rows]
    out["counts"], out["info"] = out["counts"][0], out["info"][0]
    if cls is None:
        assert (out["hist"] == CANARY).all()                 # no class map: `hist` is left alone
        out["hist"] = None
    return rc, out


def _assert_equal(got, want, what):
    assert np.array_equal(got["counts"], want["counts"]), (what, got["counts"], want["counts"], got["info"])
    assert np.array_equal(got["info"][:2], want["info"][:2]) and got["info"][3] == 0, (what, got["info"], want["info"])
    assert np.array_equal(got["labels"], want["labels"]), (what, np.argwhere(got["labels"] != want["labels"])[:5])
    assert np.array_equal(got["table"], want["table"]), (what, np.argwhere(got["table"] != want["table"])[:5])
    if want["hist"] is not None:
        assert np.array_equal(got["hist"].astype(np.int64), want["hist"]), what
    assert np.array_equal(got["object_cls"], want["object_cls"]), what


@pytest.mark.parametrize("name", MASKS)
@pytest.mark.parametrize("shape", list(SHAPES), ids=list(SHAPES))
def test_every_output_equals_the_restatement(shape, name):
    size = SHAPES[shape]
    mask = _masks(size)[name]
    cls, score = _side_inputs(size)
    for r2 in R2S:
        for connectivity in (4, 8):
            grown = _grown_list(size, name, r2, connectivity)
            # with and without the class map and the score, min_area 1 and 5: all four over the two connectivities and radii
            for min_area, side in ((1, True), (5, False)) if (r2 in (0, 4)) == (connectivity == 8) else ((5, True), (1, False)):
                kw = dict(connectivity=connectivity, min_area=min_area, n_cls=N_CLS if side else 1, first_class=1,
                          max_objects=size[0] * size[1] // 2 + 1)
                c, s = (cls, score) if side else (None, None)
                rc, got = _split(mask, r2, c, s, **kw)
                assert rc == 0
                _assert_equal(got, _want(mask, grown, c, s, **kw), (shape, name, r2, connectivity, min_area, side))
                assert 0 <= got["info"][2] <= 4096


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("i", range(len(S.hand_cases())), ids=[c[0] for c in S.hand_cases()])
def test_hand_made_cases_at_their_own_sizes(i, connectivity):
    name, mask, r2 = S.hand_cases()[i]
    rng = np.random.default_rng(i)
    cls = rng.integers(0, N_CLS, size=mask.shape, dtype=np.uint8)
    score = rng.random(mask.shape, dtype=np.float32)
    kw = dict(connectivity=connectivity, min_area=1, n_cls=N_CLS, first_class=1, max_objects=64)
    rc, got = _split(mask, r2, cls, score, **kw)
    assert rc == 0
    grown = _grown_hand(i, connectivity)
    _assert_equal(got, _want(mask, grown, cls, score, **kw), (name, connectivity))
    if name == "two_discs":
        assert got["table"][:2, 0].tolist() == ([2728, 2695] if connectivity == 4 else [2730, 2693])
        for small in (25, 144):
            rc, one = _split(mask, small, connectivity=connectivity, max_objects=4)
            assert rc == 0 and one["counts"].tolist() == [1, 1] and one["table"][0, 0] == 5423 and one["info"][1] == 1
    if name == "bridged_grid":
        assert got["counts"].tolist() == [36, 36] and got["info"][1] == 36


@pytest.mark.parametrize("name", ["checkerboard", "random0.3", "random0.8", "foreground"])
def test_truncation_below_the_number_of_pieces(name):
    size = SHAPES["37x53"]
    mask = _masks(size)[name]
    cls, score = _side_inputs(size)
    r2 = 1
    grown = _grown_list(size, name, r2, 4)
    n = int(grown[0].max())
    for max_objects in sorted({1, 3, max(n - 1, 1)}):
        kw = dict(connectivity=4, min_area=1, n_cls=N_CLS, first_class=1, max_objects=max_objects)
        rc, got = _split(mask, r2, cls, score, **kw)
        assert rc == 0
        _assert_equal(got, _want(mask, grown, cls, score, **kw), (name, max_objects))
        assert got["counts"].tolist() == [n, min(n, max_objects)] and int(got["labels"].max()) == n


@pytest.mark.parametrize("shape", ["37x53", "rows:T+1", "2T+3x2T+3"])
def test_radius_zero_is_scene_objects(shape):
    size = SHAPES[shape]
    cls, score = _side_inputs(size)
    for name in MASKS:
        mask = _masks(size)[name]
        for connectivity in (4, 8):
            kw = dict(connectivity=connectivity, min_area=2, n_cls=N_CLS, first_class=1, max_objects=512)
            plain = ops.scene_objects(_dev(mask), _dev(cls), _dev(score), **kw)
            split = ops.scene_split(_dev(mask), 0, _dev(cls), _dev(score), **kw)
            torch.cuda.synchronize()
            assert len(split) == 6 and all(torch.equal(a, b) for a, b in zip(plain, split[:5])), (shape, name, connectivity)
            info = split[5].tolist()
            assert info[0] == 0 and info[2] == 0 and info[3] == 0 and info[1] == int(R.components(mask, connectivity).max())


def test_dirty_workspace_other_stream_and_two_runs():
    size = SHAPES["2T+3x2T+3"]
    mask = _masks(size)["random0.8"]
    cls, score = _side_inputs(size)
    kw = dict(connectivity=8, min_area=1, n_cls=N_CLS, first_class=1, max_objects=2048)
    ws = torch.empty(L.lib().c3d_scene_split_ws_bytes(*size, N_CLS), dtype=torch.uint8, device=DEV)
    first = _split(mask, 4, cls, score, ws=ws, fill_ws=0, **kw)
    again = _split(mask, 4, cls, score, ws=ws, **kw)             # on what the first call left behind
    dirty = _split(mask, 4, cls, score, ws=ws, fill_ws=0xFF, **kw)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        other = _split(mask, 4, cls, score, stream=side, **kw)
    _assert_equal(first[1], _want(mask, _grown_list(size, "random0.8", 4, 8), cls, score, **kw), "random0.8")
    for run in (again, dirty, other):
        assert run[0] == 0
        for k in first[1]:
            assert np.array_equal(run[1][k], first[1][k]), k     # info[2] too: the rounds are the same from run to run


@pytest.mark.parametrize("connectivity", [4, 8])
def test_thick_serpentine_rounds(connectivity):
    name, mask, r2 = S.hand_cases()[4]
    assert name == "thick_serpentine"
    grown = _grown_hand(4, connectivity)
    assert grown[1] == 1 and grown[2] == (1824 if connectivity == 4 else 1768)
    kw = dict(connectivity=connectivity, min_area=1, max_objects=8)
    rc, cut = _split(mask, r2, max_rounds=1, **kw)               # the canaries are checked inside
    assert rc == 0 and cut["info"][0] == S.NOT_CONVERGED and cut["info"][2] == 1 and cut["info"][1] == 1
    assert cut["labels"].min() >= 0 and cut["labels"].max() <= 1 and 0 < (cut["labels"] > 0).sum() < (mask != 0).sum()
    rc, full = _split(mask, r2, max_rounds=4096, **kw)
    assert rc == 0 and full["info"][0] == 0 and 1 < full["info"][2] <= 4096
    _assert_equal(full, _want(mask, grown, **kw), name)
    used = int(full["info"][2])
    print(f"thick serpentine, connectivity {connectivity}: {used} rounds changed something")
    rc, exact = _split(mask, r2, max_rounds=used + 1, **kw)      # one round more than those that change something: converged
    assert rc == 0 and exact["info"][0] == 0 and exact["info"][2] == used and np.array_equal(exact["labels"], full["labels"])
    rc, short = _split(mask, r2, max_rounds=used, **kw)          # the last round still changed something: not known to be done
    assert rc == 0 and short["info"][0] == S.NOT_CONVERGED and short["info"][2] == used


def test_negative_control_sees_the_tie_rule():
    size = SHAPES["37x53"]
    mask = _masks(size)["random0.8"]
    rc, got = _split(mask, 1, connectivity=4)
    wrong = S.split(mask, 1, connectivity=4, ties="high", max_objects=size[0] * size[1] // 2 + 1)
    assert rc == 0 and not np.array_equal(got["labels"], wrong["labels"])


@pytest.mark.parametrize("i", [0, 2], ids=["two_discs", "bridged_grid"])
def test_outlines_of_split_labels(i):
    name, mask, r2 = S.hand_cases()[i]
    want_split = _want(mask, _grown_hand(i, 8), connectivity=8, max_objects=64)
    labels, table, hist, object_cls, counts, info = ops.scene_split(_dev(mask), np.sqrt(r2), connectivity=8, max_objects=64)
    rings, vertices, ocounts = ops.scene_outlines(labels, counts, connectivity=8, max_objects=64, max_rings=256, max_vertices=8192)
    torch.cuda.synchronize()
    assert torch.equal(labels.cpu(), torch.from_numpy(want_split["labels"])) and info.tolist()[:2] == want_split["info"].tolist()
    want = O.outlines(want_split["labels"], want_split["counts"], 8, 64, 256, 8192)
    got_counts = ocounts.cpu().numpy()
    assert np.array_equal(got_counts, want["counts"]) and np.array_equal(rings.cpu().numpy(), want["rings"])
    written = int(got_counts[3])
    assert np.array_equal(vertices.cpu().numpy()[:written], want["vertices"][:written])
    assert int(got_counts[0]) >= int(want_split["counts"][0]) > 1       # one ring per piece at least: touching pieces are cut apart


@pytest.mark.parametrize("i", [0, 1, 2], ids=["two_discs", "dumbbell", "bridged_grid"])
def test_objects_match_of_split_against_unsplit(i):
    name, mask, r2 = S.hand_cases()[i]
    d_mask = _dev(mask)
    a = ops.scene_split(d_mask, np.sqrt(r2), connectivity=8, max_objects=64)
    b = ops.scene_objects(d_mask, connectivity=8, max_objects=64)
    pa, pb = (a[0], a[1], a[4]), (b[0], b[1], b[4])
    got = ops.objects_match(*pa, *pb)
    torch.cuda.synchronize()
    want = M.match(*(t.cpu().numpy() for t in pa), *(t.cpu().numpy() for t in pb))
    for k, t in zip(("match_p", "match_g", "conf", "counts"), got):
        assert np.array_equal(t.cpu().numpy(), want[k]), (name, k)
    assert abs(float(got[4][0]) - want["sum_iou"]) <= 1e-12
    tp, fp, fn = (int(v) for v in want["counts"][1:4])
    assert (tp, fn) in ((1, 0), (0, 1)) and tp + fp == int(a[4][0]) > 1   # one whole component against its pieces


def test_refusals_return_their_error_and_launch_nothing():
    lib = L.lib()
    H, W = 8, 8
    mask = torch.ones((H, W), dtype=torch.uint8, device=DEV)
    cls = torch.ones((H, W), dtype=torch.uint8, device=DEV)
    labels = torch.full((H, W), -7, dtype=torch.int32, device=DEV)
    table = torch.full((4, 8), -7, dtype=torch.int32, device=DEV)
    counts = torch.full((2,), -7, dtype=torch.int32, device=DEV)
    info = torch.full((4,), -7, dtype=torch.int32, device=DEV)
    ws = torch.empty(lib.c3d_scene_split_ws_bytes(H, W, 16), dtype=torch.uint8, device=DEV)
    p = lambda t: None if t is None else t.data_ptr()  # noqa: E731

    def call(mask=mask, cls=None, Hs=H, Ws=W, conn=8, n_cls=1, first_class=1, max_objects=4, r2=1, max_rounds=8, labels=labels,
             table=table, counts=counts, info=info, ws=ws):
        return lib.c3d_scene_split(p(mask), p(cls), None, Hs, Ws, conn, 1, n_cls, first_class, max_objects, r2, max_rounds, p(labels),
                                   p(table), None, None, p(counts), p(info), p(ws), None)

    before = ops.launch_count()
    for conn in (0, 6, 9, -4):
        assert call(conn=conn) == -1                                 # C3D_E_BADARG
    assert call(Hs=65536, Ws=32768) == -2                            # C3D_E_UNSUPPORTED: Hs * Ws = 2^31
    assert call(Hs=16385, Ws=8) == -2 and call(Hs=8, Ws=16385) == -2  # r2 > 0 past the limits of the transform
    assert call(cls=cls, n_cls=0) == -1 and call(cls=cls, n_cls=17) == -1
    assert call(max_objects=0) == -1 and call(max_objects=-5) == -1 and call(first_class=-1) == -1
    assert call(Hs=0) == -1 and call(Ws=-3) == -1
    assert call(r2=-1) == -1 and call(r2=(1 << 20) + 1) == -1
    assert call(max_rounds=0) == -1 and call(max_rounds=65537) == -1 and call(max_rounds=-2) == -1
    assert call(labels=None) == -1 and call(table=None) == -1 and call(counts=None) == -1 and call(ws=None) == -1
    assert call(mask=None) == -1 and call(info=None) == -1
    torch.cuda.synchronize()
    assert ops.launch_count() == before
    for t in (labels, table, counts, info):
        assert int((t != -7).sum()) == 0                             # nothing was written
    with pytest.raises(L.Change3DHipError):
        ops.scene_split(mask, 1, connectivity=5)
    with pytest.raises(ValueError):
        ops.scene_split(mask, 1, max_rounds=0)
    with pytest.raises(ValueError):
        ops.scene_split(mask, -1)
    with pytest.raises(ValueError):
        ops.scene_split(mask, 1025)
    assert call(r2=1 << 20, max_rounds=65536 // 64) == 0             # the largest radius: the whole scene erodes away, one piece
    torch.cuda.synchronize()
    assert ops.launch_count() > before and counts.tolist() == [1, 1] and table[0].tolist() == [64, 0, 0, 7, 7, 0, 0, 0]
    assert info.tolist() == [0, 0, 0, 0]
