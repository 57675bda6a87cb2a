"""The restatement of `c3d_rings_polis` (tests/polis_reference.py) against independent witnesses, without a GPU: exact
fractions with an integer square root, closed forms, a dense sampling of the boundary queried through a k-d tree, exact
invariance under a change of frac_bits, the rotated rectangles of the regulariser taken through the reference pipeline with
their scores printed, the host score arithmetic, the negative controls of the GPU test, and the `ops` bindings."""
import math
import os
import sys
from fractions import Fraction

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hull_reference as HR  # noqa: E402
import objects_reference as O  # noqa: E402
import outlines_reference as T  # noqa: E402
import polis_cases as K  # noqa: E402
import polis_reference as R  # noqa: E402
import regular_cases as RK  # noqa: E402
import regular_reference as RR  # noqa: E402
import simplify_reference as SR  # noqa: E402

from change3d_amd import _lib as L  # noqa: E402
from change3d_amd import ops, polygon_metrics  # noqa: E402

U = 2.0 ** -53
HAND_MADE = K.hand_made()


def _run(c, **kw):
    tp, tg, match = K.tables(c)
    return R.polis(tp, c["P"][2], tg, c["G"][2], match, c["max_g"], **kw)


def _exact_v(p, a, b):
    ex, ey, wx, wy = b[0] - a[0], b[1] - a[1], p[0] - a[0], p[1] - a[1]
    L2, t, c = ex * ex + ey * ey, wx * ex + wy * ey, wx * ey - wy * ex
    if L2 == 0 or t <= 0:
        return Fraction(wx * wx + wy * wy)
    if t >= L2:
        return Fraction((p[0] - b[0]) ** 2 + (p[1] - b[1]) ** 2)
    return Fraction(c * c, L2)


def _sqrt(q, digits=40):
    """sqrt of a Fraction to `digits` decimal places, from an integer square root."""
    s = 10 ** digits
    return Fraction(math.isqrt(q.numerator * q.denominator * s * s), q.denominator * s)


def _exact_pair(rp, rg):
    """(polis, hausdorff, mean_pg, mean_gp) of two ring lists as Fractions."""
    ep, eg = R.edges_of(rp), R.edges_of(rg)
    d_pg = [_sqrt(min(_exact_v(v, a, b) for a, b in eg)) for ring in rp for v in ring]
    d_gp = [_sqrt(min(_exact_v(v, a, b) for a, b in ep)) for ring in rg for v in ring]
    m_pg, m_gp = sum(d_pg) / len(d_pg), sum(d_gp) / len(d_gp)
    return (m_pg + m_gp) / 2, max(d_pg + d_gp), m_pg, m_gp


def _rel(got, exact):
    return 0.0 if exact == 0 and got == 0 else float(abs(Fraction(got) - exact) / exact)


def test_restatement_against_fractions_on_random_polygons():
    rng = np.random.default_rng(3)
    worst = [0.0, 0.0]
    for trial in range(12):
        n_p, n_g = (int(v) for v in rng.integers(3, 40, 2))
        scale = int(rng.choice([50, 5000, 2 ** 22]))
        c = K.case([K.polygon(n_p, trial, radius=scale)], [K.polygon(n_g, trial + 50, radius=scale, centre=(scale // 7, -scale // 9))],
                   {1: 1}, f_p=8, f_g=8)
        out = _run(c)
        exact = [v / 256 for v in _exact_pair(*(c[s][0] for s in "PG"))]
        assert out["pair_n"][0].tolist() == [1, n_p, n_g, 0]
        bound = R.bounds(out["pair_n"])[0]
        for k in range(4):
            err = _rel(float(out["pair"][0, k]), exact[k])
            assert err <= bound[k], (trial, k, err / U)
            worst[0 if k == 1 else 1] = max(worst[0 if k == 1 else 1], err / U)
    print(f"worst error against fractions: a distance {worst[0]:.2f} u, a mean {worst[1]:.2f} u")


def test_closed_forms():
    sq = K.square(0, 0, 100)
    same = _run(K.case([sq, K.polygon(17, 2)], [sq, K.polygon(17, 2)], {1: 1, 2: 2}))
    assert not same["pair"].any() and same["counts"][:6].tolist() == [2, 0, 0, 0, 21, 21] and same["sums"].tolist() == [0.0, 0.0, 0.0, 2.0]
    for e in (1, 3, 17):
        out = _run(K.case([K.square(e, e, 100 - 2 * e)], [sq], {1: 1}))
        polis, haus, inner, outer = out["pair"][0]
        assert inner == e and abs(outer - e * math.sqrt(2)) <= 8 * U * outer and haus == outer
        assert abs(polis - e * (1 + math.sqrt(2)) / 2) <= 24 * U * polis


def test_dense_sampling_of_the_boundary_through_a_kd_tree():
    cKDTree = pytest.importorskip("scipy.spatial").cKDTree
    c = HAND_MADE["holes_interleaved"]
    out = _run(c)
    rings_g2 = [r for r, i in zip(c["G"][0], c["G"][1]) if i == 2]
    step, samples = 0.01, []
    for a, b in R.edges_of(rings_g2):
        k = int(math.ceil(math.hypot(b[0] - a[0], b[1] - a[1]) / step))
        samples += [(a[0] + (b[0] - a[0]) * j / k, a[1] + (b[1] - a[1]) * j / k) for j in range(k + 1)]
    sampled, _ = cKDTree(np.asarray(samples)).query(np.asarray(c["P"][0][0], dtype=np.float64))
    exact = R.distances(c["P"][0][0], R.edges_of(rings_g2))
    assert all(s + 1e-9 >= e >= s - step / 2 - 1e-9 for s, e in zip(sampled.tolist(), exact))
    assert abs(out["pair"][0, 2] - sum(exact) / 4) <= 12 * U * out["pair"][0, 2]
    assert out["pair"][0, 2] == 3.5, "the square inside the hole is 2, 4, 6 and 2 px from the hole ring, 12 px and more from the outline"


def test_a_change_of_frac_bits_changes_no_bit():
    c0 = HAND_MADE["holes_interleaved"]
    up = lambda rings: [[(x * 16, y * 16) for x, y in ring] for ring in rings]   # noqa: E731
    c4 = K.case(up(c0["P"][0]), up(c0["G"][0]), c0["match"], f_p=4, f_g=4, ids_p=c0["P"][1], ids_g=c0["G"][1])
    mixed = K.case(c0["P"][0], up(c0["G"][0]), c0["match"], f_p=0, f_g=4, ids_p=c0["P"][1], ids_g=c0["G"][1])
    a, b, m = _run(c0), _run(c4), _run(mixed)
    for other in (b, m):
        assert all(np.array_equal(a[k], other[k]) for k in ("pair", "pair_n", "counts", "sums"))
    assert a["counts"][0] == 2 and a["pair"][0].all() and not a["pair"][1].any()


def test_flags_counts_and_the_work_cap():
    c = HAND_MADE["flags"]
    out = _run(c)
    assert out["pair_n"][:, 3].tolist() == [0, 1, 2, 0, 2, 1, 0, 0] and out["counts"][:6].tolist() == [2, 2, 2, 0, 8, 8]
    assert out["pair_n"][4].tolist() == [2, 0, 4, 2] and not out["pair"][[1, 2, 4, 5, 6, 7]].any() and out["counts"][6] == 0
    tp, tg, match = K.tables(c)
    tp[0][0, 1] = -1                                         # id 1 has a ring the outlines call had no room for
    match[5, 0] = 9                                          # a partner past max_g
    out = R.polis(tp, 0, tg, 0, match, c["max_g"])
    assert out["pair_n"][:, 3].tolist() == [2, 1, 2, 0, 2, 1, 0, 0] and out["counts"][6] == R.ST_BAD_PARTNER
    assert _run(c, max_pair_work=32)["counts"][:4].tolist() == [2, 2, 2, 0]
    assert _run(c, max_pair_work=31)["counts"][:4].tolist() == [0, 2, 2, 2]
    many = K.case([K.square(10 * k, 0, 5) for k in range(5)], [K.square(0, 0, 5)], {1: 1}, ids_p=[1] * 5)
    assert _run(many, ring_limit=5)["pair_n"][0].tolist() == [1, 20, 4, 0] and _run(many, ring_limit=4)["pair_n"][0].tolist() == [1, 0, 4, 2]


@pytest.mark.parametrize("name,wrong", [("squares_apart", dict(segment=False)), ("holes_interleaved", dict(join=True)),
                                        ("triangles", dict(closing=False))])
def test_the_negative_controls_differ_where_the_gpu_test_says(name, wrong):
    good, bad = _run(HAND_MADE[name]), _run(HAND_MADE[name], **wrong)
    assert abs(good["pair"][0, 0] - bad["pair"][0, 0]) > 1e-3 * good["pair"][0, 0], (name, good["pair"][0], bad["pair"][0])


def _stages(d):
    """The rings of one rotated rectangle after tracing, simplifying at 1 px and regularising: (name, table, frac_bits)."""
    mask = RK.rotated_rectangle(d)
    H, W = mask.shape
    labels = O.components(mask, 8)
    raw = T.outlines(labels, np.array([1, 1], np.int32), 8, max_objects=4, max_rings=8, max_vertices=4 * H * W)
    simple = SR.simplify(raw["rings"], raw["vertices"], raw["counts"], SR.tol2_q(1.0))
    hull = HR.hulls(raw["rings"], raw["vertices"], raw["counts"], 4, 4 * H * W)
    regular = RR.regularize(simple["rings"], simple["vertices"], simple["counts"], hull["hulls"], hull["vertices"], hull["rects"],
                            hull["counts"], 4)
    return [(name, (t["rings"], t["vertices"], t["counts"]), f) for name, t, f in (("raw", raw, 0), ("simplified", simple, 0),
                                                                                   ("regularised", regular, 4))]


@pytest.mark.parametrize("d", K.DIRECTIONS)
def test_rotated_rectangles_through_the_reference_pipeline(d):
    """Printed and recorded in the README; a measurement, not a threshold.  Measured on 40 x 25 px against the true rectangle
    rounded to 1/16 px (vertices, PoLiS, vertex Hausdorff in px) for raw / simplified / regularised: (3, 1) 84 0.294 0.572 / 4
    0.190 0.435 / 4 0.109 0.158; (2, 5) 100 0.306 0.638 / 19 0.316 0.634 / 4 0.140 0.244; (5, -2) 100 0.306 0.638 / 7 0.296
    0.604 / 4 0.100 0.188; (1, 1) 184 0.177 0.486 / 4 0.350 0.486 / 4 0.133 0.133."""
    truth = SR.table([K.true_rectangle(d)], max_rings=2, max_vertices=8, ids=[1])
    match = np.array([[1, 1, 1, 1], [0, 0, 0, 0]], dtype=np.int32)
    seen = {}
    for name, table, f in _stages(d):
        out = R.polis(table, f, truth, 4, match, 1)
        assert out["pair_n"][0, 3] == 0 and out["pair_n"][0, 2] == 4
        seen[name] = out["pair"][0]
        print(f"rotated rectangle along {d}: {name} n = {out['pair_n'][0, 1]} polis = {out['pair'][0, 0]:.3f} hausdorff = {out['pair'][0, 1]:.3f}")
    assert seen["regularised"][0] < seen["raw"][0] and seen["regularised"][1] < seen["raw"][1]


def test_host_score_arithmetic():
    s = polygon_metrics.scores_from_totals([4, 1, 2, 3, 40, 16, 0, 0], [2.0, 6.0, 2.5, 10.0])
    assert s == dict(pairs=4, polis=0.5, hausdorff_mean=1.5, hausdorff_max=2.5, n_ratio=2.5, vertices=40, vertices_gt=16, no_partner=1,
                     incomplete=2, over_work=3, status=0)
    empty = polygon_metrics.scores_from_totals([0] * 8, [0.0] * 4)
    assert empty["polis"] == 0.0 and empty["n_ratio"] == 0.0 and empty["hausdorff_max"] == 0.0 and empty["pairs"] == 0


def test_ops_bindings_exist_and_refuse_host_tensors():
    assert callable(ops.rings_polis) and callable(ops.rings_polis_limits) and callable(polygon_metrics.PolygonEvaluator)
    assert L.POLIS_ST_BAD_PARTNER == R.ST_BAD_PARTNER == 512
    wave, chunk, tile, ring_limit, big = ops.rings_polis_limits()
    assert 3 <= wave <= 64 and chunk >= 64 and tile >= 64 and ring_limit >= 4 and big >= wave
    c = HAND_MADE["triangles"]
    tp, tg, match = K.tables(c)
    host = [torch.from_numpy(a) for a in tp + tg + (match,)]
    with pytest.raises(L.Change3DHipError):
        ops.rings_polis(*host[:3], 0, *host[3:6], 0, host[6], c["max_g"])
