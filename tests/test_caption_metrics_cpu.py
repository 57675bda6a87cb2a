"""Caption metrics, the host side: the tests' restatement (tests/caption_metrics_reference.py) against the numbers recorded
from the reference's own scorers (tests/golden/cc_metrics.npz, tools/gen_golden_cc_metrics.py), its negative controls, and
the host paths of change3d_amd/caption_metrics.py.  No GPU."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import caption_metrics_reference as cr  # noqa: E402

CORPORA = ["levir", "tiny_vocab", "single", "pair", "edges"]


def load_corpus(name):
    """(hyps, refs, recorded) of one fixture corpus: token lists and the dict of recorded arrays"""
    z = np.load(os.path.join(HERE, "golden", "cc_metrics.npz"))
    rec = {k[len(name) + 1:]: z[k] for k in z.files if k.startswith(name + "_")}
    hyps = [rec["hyp"][i, :n].tolist() for i, n in enumerate(rec["hyp_len"])]
    refs = [[rec["refs"][i, j, :n].tolist() for j, n in enumerate(row)] for i, row in enumerate(rec["ref_len"])]
    return hyps, refs, rec


@pytest.mark.parametrize("name", CORPORA)
def test_restatement_reproduces_the_recorded_reference_numbers(name):
    """Equality everywhere, the corpus means included: the restatement calls np.mean on the same array the reference does, so
    numpy's summation order is the same and no bound is needed."""
    hyps, refs, rec = load_corpus(name)
    s = cr.score_corpus(hyps, refs)
    assert np.array_equal(s["stats"], rec["stats"])
    assert s["totals"] == rec["totals"].tolist()
    assert [s[f"Bleu_{k}"] for k in range(1, 5)] == rec["bleu"].tolist()
    assert np.array_equal(np.array(s["lcs"], dtype=np.int32), rec["lcs"])
    assert np.array_equal(s["rouge"], rec["rouge"]) and np.array_equal(s["cider"], rec["cider"])
    assert s["ROUGE_L"] == rec["ROUGE_L"] and s["CIDEr"] == rec["CIDEr"]


def test_fixture_is_small_and_covers_the_lengths():
    assert os.path.getsize(os.path.join(HERE, "golden", "cc_metrics.npz")) < 512 * 1024
    for name in CORPORA:
        hyps, refs, _ = load_corpus(name)
        assert len(hyps) <= 64
    hyps, refs, _ = load_corpus("tiny_vocab")
    assert {0, 1, 2, 3, 4, 63, 64} <= {len(h) for h in hyps}
    assert {1, 64} <= {len(r) for rs in refs for r in rs}


@pytest.mark.parametrize("name", ["levir", "tiny_vocab"])
def test_control_dropping_the_clipping_moves_bleu_and_cider(name):
    hyps, refs, rec = load_corpus(name)
    s = cr.score_corpus(hyps, refs, clip=False)
    assert s["totals"][6:10] != rec["totals"].tolist()[6:10]
    assert s["Bleu_1"] > rec["bleu"][0]
    assert s["CIDEr"] != rec["CIDEr"] and not np.array_equal(s["cider"], rec["cider"])


@pytest.mark.parametrize("name", ["levir", "tiny_vocab", "edges"])
def test_control_closest_length_tie_to_the_longer_reference_moves_bleu(name):
    hyps, refs, rec = load_corpus(name)
    s = cr.score_corpus(hyps, refs, tie_shorter=False)
    assert s["totals"][1] > int(rec["totals"][1])
    assert np.array_equal(s["stats"][:, [0] + list(range(2, 10))], rec["stats"][:, [0] + list(range(2, 10))])


@pytest.mark.parametrize("name", CORPORA)
def test_control_bigram_length_quirk(name):
    """The reference's `length` counts bigrams (`n == 1` is zero-based): max(len - 1, 0) instead of len.  "Fixing" it CANNOT move
    a score, on this fixture or on any corpus the scorer accepts: references are never empty, so delta = (lh - 1) - (lr - 1) =
    lh - lr for every non-empty hypothesis, and an empty hypothesis has no n-gram at all and scores 0 whatever its penalty is.
    So this control asserts what is true -- the repaired variant is identical -- and the property that can be observed, that the
    length penalty is applied at all, is the control next to it."""
    hyps, refs, rec = load_corpus(name)
    s = cr.score_corpus(hyps, refs, bigram_length=False)
    assert np.array_equal(s["cider"], rec["cider"])


@pytest.mark.parametrize("name", ["levir", "tiny_vocab", "edges", "single"])
def test_control_dropping_the_length_penalty_moves_cider(name):
    hyps, refs, rec = load_corpus(name)
    s = cr.score_corpus(hyps, refs, length_penalty=False)
    assert s["CIDEr"] > rec["CIDEr"]


def test_split_restatement():
    nochange = [[1, 2, 3], [4, 5]]
    hyps = [[1, 2, 3], [9], None, [4, 5], [4, 5, 6]]
    refs = [[[7], [1, 2, 3]], [[7], [4, 5]], [[1, 2, 3], [8]], [[4, 5], [9, 9]], [[7], [1, 2, 3]]]
    assert cr.split_corpus(hyps, refs, nochange) == ([0, 1, 4], [2, 3], 1, 1)


# ------------------------------------------------------------------------------------------------ CaptionScorer, host
def test_pack_corpus_layout_and_none_hypothesis():
    from change3d_amd.caption_metrics import pack_corpus
    h, hl, r, rl = pack_corpus([[5, 6, 7], None, []], [[[1], [2, 3]], [[4, 4, 4], [0]], [[65534], [9]]])
    assert h.dtype == np.int32 and h.shape == (3, 64) and r.shape == (3, 2, 64) and rl.shape == (3, 2)
    assert hl.tolist() == [3, 0, 0] and rl.tolist() == [[1, 2], [3, 1], [1, 1]]
    assert h[0, :4].tolist() == [5, 6, 7, -1] and (h[1:] == -1).all()
    assert r[1, 0, :4].tolist() == [4, 4, 4, -1] and r[2, 0, 0] == 65534 and r[1, 1, :2].tolist() == [0, -1]


def test_pack_corpus_refuses_what_the_kernels_do_not_take():
    from change3d_amd.caption_metrics import pack_corpus
    with pytest.raises(ValueError, match="no tokens"):
        pack_corpus([[1]], [[[1], []]])
    with pytest.raises(ValueError, match="at most 64"):
        pack_corpus([[1] * 65], [[[1]]])
    with pytest.raises(ValueError, match="at most 64"):
        pack_corpus([[1]], [[[1] * 65]])
    with pytest.raises(ValueError, match="outside"):
        pack_corpus([[65535]], [[[1]]])
    with pytest.raises(ValueError, match="outside"):
        pack_corpus([[1]], [[[-1]]])
    with pytest.raises(ValueError):
        pack_corpus([[1], [2]], [[[1]], [[1], [2]]])            # ragged reference counts
    with pytest.raises(ValueError):
        pack_corpus([[1]], [[[1]] * 8])                         # more than 7 references
    pack_corpus([[1] * 64], [[[65534] * 64]])                   # the limits themselves are fine


def test_scorer_bleu_is_the_restatements_expression():
    from change3d_amd.caption_metrics import bleu_from_totals
    for name in CORPORA:
        _, _, rec = load_corpus(name)
        assert bleu_from_totals(rec["totals"].tolist()) == rec["bleu"].tolist()


def test_plan_is_host_only():
    from change3d_amd import ops
    assert ops.cap_metrics_plan(1929, 5, 64, ref_tokens=1000) == (256 + 12 * 8192, 8192)      # next power of two >= 2 * 4 * 1000
    assert ops.cap_metrics_plan(2, 1, 4) == (256 + 12 * 64, 64)                                # no count given: N * R * L
    assert ops.cap_metrics_plan(7, 5, 64, table_capacity=16) == (256 + 12 * 16, 16)
    assert ops.cap_metrics_plan(7, 8, 64) is None and ops.cap_metrics_plan(7, 5, 65) is None   # C3D_E_UNSUPPORTED
    from change3d_amd._lib import Change3DHipError
    with pytest.raises(Change3DHipError):
        ops.cap_metrics_plan(7, 5, 64, table_capacity=24)                                      # not a power of two
