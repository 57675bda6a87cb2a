"""The restatement of `c3d_objects_match` (tests/objects_match_reference.py) checked on the CPU: against a brute-force double
loop over object pairs, on a hand-worked 3 x 8 case with literal rows, for uniqueness of a match at 0.5, and with negative
controls that must bite; then `ObjectEvaluator`'s host formulas, the `_lib` signatures and `predict_scene`'s parser."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import objects_match_reference as M  # noqa: E402
import objects_reference as O  # noqa: E402

SMALL = [(5, 1), (9, 63), (20, 64)]
FROM_9x63 = [(9, 63), (20, 64), (37, 65), (40, 130), (70, 257)]


@functools.lru_cache(maxsize=None)
def _pairs(size):
    return {name: (p, g, conns) for name, p, g, conns in M.mask_pairs(size[0], size[1], seed=size[0] * 1000 + size[1])}


@functools.lru_cache(maxsize=None)
def _labelled(size, name, connectivity, with_cls=False):
    """The two `objects_reference.objects` results of a mask pair (labels, table, counts as c3d_scene_objects defines them)."""
    p, g, _ = _pairs(size)[name]
    n = size[0] * size[1]
    cls = np.ones(size, np.uint8) if with_cls else None
    kw = dict(connectivity=connectivity, n_cls=2 if with_cls else 1, max_objects=n // 2 + 1)
    return O.objects(p, cls, None, **kw), O.objects(g, cls, None, **kw)


def _match(a, b, **kw):
    return M.match(a["labels"], a["table"], a["counts"], b["labels"], b["table"], b["counts"], **kw)


@pytest.mark.parametrize("size", SMALL, ids=lambda s: f"{s[0]}x{s[1]}")
def test_restatement_equals_the_double_loop_over_object_pairs(size):
    for name, (_, _, conns) in _pairs(size).items():
        for conn in conns:
            a, b = _labelled(size, name, conn)
            got = _match(a, b)
            n_p, n_g = int(a["counts"][1]), int(b["counts"][1])
            matches, cov_p, cov_g, pairs = M.brute_force(a["labels"], b["labels"], n_p, n_g)
            assert got["counts"].tolist() == [pairs, len(matches), n_p - len(matches), n_g - len(matches), 0, 0], (name, conn)
            assert got["match_p"][:n_p, 3].tolist() == cov_p and got["match_g"][:n_g, 3].tolist() == cov_g
            assert [(k + 1, *r[:3]) for k, r in enumerate(got["match_p"].tolist()) if r[0]] == \
                [(p, g, i, u) for p, g, i, u in matches]
            assert sorted((r[0], k + 1, r[1], r[2]) for k, r in enumerate(got["match_g"].tolist()) if r[0]) == sorted(matches)
            assert got["ious"] == [i / u for _, _, i, u in matches]
            assert int(got["conf"].sum()) == n_p + n_g - len(matches)
            assert not got["match_p"][n_p:].any() and not got["match_g"][n_g:].any()


def test_hand_worked_3x8():
    pred = np.array([[1, 1, 1, 0, 0, 1, 1, 0],
                     [1, 1, 1, 0, 0, 0, 0, 0],
                     [0, 0, 0, 0, 0, 0, 0, 1]], np.uint8)
    gt = np.array([[0, 1, 1, 1, 0, 1, 1, 1],
                   [0, 1, 1, 1, 0, 0, 0, 0],
                   [0, 0, 0, 0, 0, 0, 0, 0]], np.uint8)
    a, b = O.objects(pred, max_objects=4), O.objects(gt, max_objects=3)
    assert a["counts"].tolist() == [3, 3] and b["counts"].tolist() == [2, 2]
    got = _match(a, b)
    # blocks of 6 overlapping in 4: IoU 4 / 8, exactly one half, no match;  2 of 3 pixels: 2 / 3 matches;  one pixel alone
    assert got["match_p"].tolist() == [[0, 0, 0, 4], [2, 2, 3, 2], [0, 0, 0, 0], [0, 0, 0, 0]]
    assert got["match_g"].tolist() == [[0, 0, 0, 4], [2, 2, 3, 2], [0, 0, 0, 0]]
    assert got["counts"].tolist() == [2, 1, 2, 1, 0, 0] and got["conf"].tolist() == [[4]]
    assert got["sum_iou"] == 2.0 / 3.0 and got["ious"] == [2.0 / 3.0]
    assert _match(a, b, iou_thr=0.7)["counts"].tolist() == [2, 0, 3, 2, 0, 0]
    loose = _match(a, b, strict=False)
    assert loose["match_p"][0].tolist() == [1, 4, 8, 4] and loose["counts"].tolist() == [2, 2, 1, 0, 0, 0]
    # the table of the prediction holds two rows only: object 3 is background, and the call says so
    cut = O.objects(pred, max_objects=2)
    got = _match(cut, b)
    assert cut["counts"].tolist() == [3, 2] and got["counts"].tolist() == [2, 1, 1, 1, M.ST_TRUNCATED, 0]
    bad = dict(cut, counts=np.array([-1, 2], np.int32))
    assert _match(bad, b)["counts"][4] == M.ST_BAD_COUNTS


@pytest.mark.parametrize("size", SMALL + FROM_9x63[2:], ids=lambda s: f"{s[0]}x{s[1]}")
def test_a_match_at_one_half_is_unique_on_both_sides(size):
    for name, (_, _, conns) in _pairs(size).items():
        for conn in conns:
            a, b = _labelled(size, name, conn)
            labels_p, labels_g = a["labels"].astype(np.int64), b["labels"].astype(np.int64)
            both = (labels_p > 0) & (labels_g > 0)
            keys, inter = np.unique((labels_p[both] << 32) | labels_g[both], return_counts=True)
            p, g = keys >> 32, keys & 0xFFFFFFFF
            union = a["table"][p - 1, 0].astype(np.int64) + b["table"][g - 1, 0] - inter
            hit = inter.astype(np.float64) > 0.5 * union.astype(np.float64)
            assert len(set(p[hit].tolist())) == int(hit.sum()) == len(set(g[hit].tolist())), (name, conn)
            got = _match(a, b)
            for k, row in enumerate(got["match_p"].tolist()):
                if row[0]:
                    assert got["match_g"][row[0] - 1, :3].tolist() == [k + 1, row[1], row[2]]


@pytest.mark.parametrize("size", FROM_9x63, ids=lambda s: f"{s[0]}x{s[1]}")
def test_the_mask_pairs_have_the_structure_they_claim(size):
    res = {name: _match(*_labelled(size, name, conns[0])) for name, (_, _, conns) in _pairs(size).items()}
    pairs, tp, fp, fn = (lambda n: res[n]["counts"][:4].tolist())("identical")
    assert tp == pairs > 0 and fp == fn == 0 and all(v == 1.0 for v in res["identical"]["ious"])
    assert min(res["shift1"]["counts"][:4]) > 0                               # TP, FP and FN together
    assert res["shift2"]["counts"][0] > 0 and res["shift2"]["counts"][1] == 0
    pairs, tp, fp, fn = res["split"]["counts"][:4].tolist()                   # two predicted objects per label, at most one matches
    assert tp > 0 and fp >= pairs - tp > 0 and tp + fn == res["identical"]["counts"][1]
    assert res["split"]["counts"][[2, 3]].tolist() == res["merge"]["counts"][[3, 2]].tolist()
    assert res["half"]["counts"][0] > 0 and res["half"]["counts"][1] == 0
    a, b = _labelled(size, "checker_vs_full", 4)
    assert b["counts"][0] == 1 and a["counts"][0] == (size[0] * size[1] + 1) // 2 == res["checker_vs_full"]["match_g"][0, 3]
    a, b = _labelled(size, "stripes", 4)
    assert res["stripes"]["counts"][0] == int(a["counts"][0]) * int(b["counts"][0]) > int(a["counts"][0]) + int(b["counts"][0])
    assert min(res["random"]["counts"][[0, 2, 3]]) > 0
    assert res["empty_prediction"]["counts"][:4].tolist() == [0, 0, 0, res["identical"]["counts"][1]]
    assert res["empty_label"]["counts"][:4].tolist() == [0, 0, res["identical"]["counts"][1], 0]
    assert res["both_empty"]["counts"].tolist() == [0] * 6 and res["both_empty"]["sum_iou"] == 0.0


def test_negative_controls_bite():
    size = (20, 64)
    a, b = _labelled(size, "half", 8)
    assert _match(a, b)["counts"][1] == 0 and _match(a, b, strict=False)["counts"][1] > 0          # >= instead of >
    a, b = _labelled(size, "merge", 8, True)
    right, wrong = _match(a, b, n_cls=2), _match(a, b, n_cls=2, conf_gt_rows=False)
    assert right["conf"][1, 0] == right["counts"][3] and right["conf"][0, 1] == right["counts"][2] and right["conf"][1, 1] == right["counts"][1]
    assert not np.array_equal(right["conf"], wrong["conf"])                                         # conf's axes swapped


def test_object_evaluator_host_formulas():
    from change3d_amd.object_metrics import scores_from_totals
    conf = [[0, 2, 1], [1, 3, 1], [2, 0, 4]]                # rows: ground truth
    flat = [v for row in conf for v in row]
    s = scores_from_totals([8, 3, 3, 20, 0] + flat, 6.5, 3)
    assert (s["tp"], s["fp"], s["fn"], s["pairs"], s["status"]) == (8, 3, 3, 20, 0)
    assert s["precision"] == 8 / 11 and s["recall"] == 8 / 11 and s["f1"] == 16 / 22
    assert s["sq"] == 6.5 / 8 and s["rq"] == 8 / 11 and s["pq"] == (6.5 / 8) * (8 / 11)
    assert s["conf"].tolist() == conf and s["class_f1"] == [2 * 3 / (5 + 5), 2 * 4 / (6 + 6)]
    z = scores_from_totals([0, 0, 0, 0, 0, 0], 0.0, 1)      # nothing anywhere: every denominator is 0
    assert all(z[k] == 0.0 for k in ("precision", "recall", "f1", "sq", "rq", "pq")) and z["class_f1"] == [] and z["conf"].tolist() == [[0]]
    m = scores_from_totals([0, 4, 0, 0, 0] + [0, 4, 0, 0], 0.0, 2)        # only false alarms
    assert m["precision"] == 0.0 and m["recall"] == 0.0 and m["rq"] == 0.0 and m["pq"] == 0.0 and m["class_f1"] == [0.0]
    results = [dict(counts=np.array([5, 2, 1, 0, 0, 0]), conf=np.array([[1, 0], [0, 2]]), sum_iou=1.5),
               dict(counts=np.array([7, 1, 0, 3, 0, 0]), conf=np.array([[0, 0], [3, 1]]), sum_iou=0.75)]
    want = M.scores(results, 2)
    got = scores_from_totals([3, 1, 3, 12, 0, 1, 0, 3, 3], 2.25, 2)
    assert all(got[k] == want[k] for k in want if k != "conf") and np.array_equal(got["conf"], want["conf"])


def test_lib_declares_the_two_new_symbols():
    from change3d_amd import _lib as L
    res, args = L.SIGNATURES["c3d_objects_match_ws_bytes"]
    assert res is C.c_int64 and len(args) == 3
    res, args = L.SIGNATURES["c3d_objects_match"]
    assert res is C.c_int32 and len(args) == 22 and args[11] is C.c_double and args[12] is C.c_int64
    assert (L.MATCH_ST_TABLE_FULL, L.MATCH_ST_TRUNCATED, L.MATCH_ST_BAD_COUNTS) == (M.ST_TABLE_FULL, M.ST_TRUNCATED, M.ST_BAD_COUNTS)
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "change3d_hip.h")).read()
    assert "int64_t c3d_objects_match_ws_bytes(" in header and "int c3d_objects_match(" in header


def test_predict_scene_parser_knows_iou_thr():
    from change3d_amd.scripts import predict_scene
    p = predict_scene.build_parser()
    for bad in ("0.49", "1.0", "nan"):
        with pytest.raises(SystemExit):
            p.parse_args(["--weights", "w", "--iou_thr", bad])
    assert p.parse_args(["--weights", "w"]).iou_thr == 0.5
    assert p.parse_args(["--weights", "w", "--objects", "--iou_thr", "0.75"]).iou_thr == 0.75
