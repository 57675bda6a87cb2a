"""Caption metrics on the device (csrc/caption_metrics.hip, change3d_amd/caption_metrics.py) against the tests' restatement of
the reference scorers (tests/caption_metrics_reference.py, itself pinned to the recorded reference numbers by
test_caption_metrics_cpu.py).  Integers -- BLEU statistics, LCS lengths, document frequencies read from the table, flags,
accuracy counts -- must be equal, and so must Bleu_1..4, which the host computes from the integer totals with the reference's
expressions.  ROUGE-L and CIDEr per image: within 1e-12 relative + 1e-15 absolute -- every term is non-negative, so nothing
cancels; at most 64 terms per sum and about 20 further operations give about 100 * 2^-52 = 2e-14, the rest is margin for a
1-ulp log / exp / sqrt.  Corpus means: within M * 2^-52 (relative) of the mean of the per-image device values."""
import contextlib
import functools
import io
import math
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import caption_metrics_reference as cr  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RTOL, ATOL = 1e-12, 1e-15
FIXTURE = ["levir", "tiny_vocab", "single", "pair", "edges"]


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")


@functools.lru_cache(maxsize=None)
def fixture(name):
    z = np.load(os.path.join(HERE, "golden", "cc_metrics.npz"))
    rec = {k[len(name) + 1:]: z[k] for k in z.files if k.startswith(name + "_")}
    hyps = [rec["hyp"][i, :n].tolist() for i, n in enumerate(rec["hyp_len"])]
    refs = [[rec["refs"][i, j, :n].tolist() for j, n in enumerate(row)] for i, row in enumerate(rec["ref_len"])]
    return hyps, refs, rec


def key_of(gram):
    return sum((t + 1) << (16 * i) for i, t in enumerate(gram))


def table_of(out):
    """(status, {key: count}) from the workspace of a call: the debug read the header documents"""
    cap, ws = out["capacity"], out["ws"].cpu().numpy()
    keys = ws[256:256 + 8 * cap].view(np.uint64)
    counts = ws[256 + 8 * cap:256 + 12 * cap].view(np.uint32)
    return int(ws[:4].view(np.uint32)[0]), {int(k): int(c) for k, c in zip(keys, counts) if k}


def close(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    err, bound = np.abs(got - want), RTOL * np.abs(want) + ATOL
    worst = float((err / bound).max()) if err.size else 0.0
    print(f"worst |device - restatement| / bound = {worst:.3e}")
    return bool((err <= bound).all())


def check(hyps, refs, select=None, table_capacity=0, scorer=None):
    """one `score` of CaptionScorer against the restatement run on the selected images alone; returns the device pieces"""
    from change3d_amd.caption_metrics import CaptionScorer
    if scorer is None:
        scorer = CaptionScorer(DEV)
        scorer.add(hyps, refs)
    idx = list(range(len(hyps))) if select is None else list(select)
    want = cr.score_corpus([hyps[i] for i in idx], [refs[i] for i in idx])
    scores, per = scorer.score(select, per_image=True, table_capacity=table_capacity)
    assert sorted(scores) == ["Bleu_1", "Bleu_2", "Bleu_3", "Bleu_4", "CIDEr", "ROUGE_L"]
    assert per["stats"].dtype == torch.int32 and per["lcs"].dtype == torch.int32 and per["rouge"].dtype == torch.float64
    assert torch.equal(per["stats"].cpu().long(), torch.from_numpy(want["stats"]))
    assert torch.equal(per["lcs"].cpu(), torch.tensor(want["lcs"], dtype=torch.int32))
    assert [scores[f"Bleu_{k}"] for k in range(1, 5)] == [want[f"Bleu_{k}"] for k in range(1, 5)]
    rouge, cider = per["rouge"].cpu().numpy(), per["cider"].cpu().numpy()
    assert close(rouge, want["rouge"]), "ROUGE-L per image"
    assert close(cider, want["cider"]), "CIDEr per image"
    M = len(idx)
    for key, arr in (("ROUGE_L", rouge), ("CIDEr", cider)):
        mean = math.fsum(arr.tolist()) / M
        assert abs(scores[key] - mean) <= M * 2.0 ** -52 * abs(mean), (key, scores[key], mean)
    return scorer, scores, per


def random_corpus(n, R, vocab, lens, seed):
    rng = np.random.default_rng(seed)
    refs = [[[int(t) for t in rng.integers(0, vocab, size=int(rng.integers(lens[0], lens[1] + 1)))] for _ in range(R)]
            for _ in range(n)]
    hyps = []
    for i, rs in enumerate(refs):
        h = list(rs[i % R])
        for j in range(len(h)):
            if rng.random() < 0.2:
                h[j] = int(rng.integers(0, vocab))
        hyps.append(h[:int(rng.integers(0, len(h) + 1))] if i % 7 == 3 else h)
    return hyps, refs


# --------------------------------------------------------------------------------------------------------- the fixture
@pytest.mark.parametrize("name", FIXTURE)
def test_fixture_corpora_match_their_recorded_scores(name):
    """N = 1 (ref_len = 1) / 2 / 7 / 48 / 64, R = 1 and 5, hypothesis lengths 0..4, 63, 64, reference lengths 1 and 64, a
    vocabulary of 2, tokens 0 and 65534, closest-length ties, n-grams in every image (idf exactly 0)."""
    _need_gpu()
    hyps, refs, rec = fixture(name)
    _, scores, per = check(hyps, refs)
    assert torch.equal(per["stats"].cpu().long(), torch.from_numpy(rec["stats"]))
    assert torch.equal(per["lcs"].cpu(), torch.from_numpy(rec["lcs"]))
    assert [scores[f"Bleu_{k}"] for k in range(1, 5)] == rec["bleu"].tolist()
    assert close(per["rouge"].cpu().numpy(), rec["rouge"]) and close(per["cider"].cpu().numpy(), rec["cider"])
    assert close(scores["ROUGE_L"], rec["ROUGE_L"]) and close(scores["CIDEr"], rec["CIDEr"])


@pytest.mark.parametrize("n,R", [(1, 5), (2, 5), (7, 1), (7, 5), (3, 7)])
def test_image_and_reference_counts(n, R):
    _need_gpu()
    hyps, refs = random_corpus(n, R, 2, (1, 9), seed=10 * n + R)
    check(hyps, refs)


def test_zero_idf_and_zero_norm():
    """every n-gram of the hypotheses occurs in every image's references: idf exactly 0, the hypothesis norm is 0, the division
    is skipped and the score is exactly 0 -- a log(N) - log(df) that is one ulp off zero would give a score near 10 instead"""
    _need_gpu()
    refs = [[[4, 5, 6, 7], [1 + i, 2]] for i in range(3)]
    hyps = [[4, 5, 6, 7], [5, 6], [4, 5, 6, 7, 4]]             # the last one has the n-gram (7, 4) that no reference has
    _, _, per = check(hyps, refs)
    cider = per["cider"].cpu().tolist()
    assert cider[0] == 0.0 and cider[1] == 0.0 and cider[2] == 0.0   # (7, 4) has weight but matches nothing
    hyps[2] = [4, 5, 3, 2]                                     # (3, 2) is in one image only: a positive score
    _, _, per = check(hyps, refs)
    assert per["cider"][2].item() > 0.0


def test_closest_length_ties():
    _need_gpu()
    hyps = [[1, 2, 3, 4], [1, 2, 3, 4, 5], [1, 2]]
    refs = [[[1, 2, 3, 4, 5, 6], [1, 2]], [[9] * 7, [9] * 3], [[1], [1, 2, 3]]]     # |l - t| = 2 / 2 / 1 on both sides
    _, _, per = check(hyps, refs)
    assert per["stats"][:, 1].tolist() == [2, 3, 1]


# ---------------------------------------------------------------------------------------------------- subsets, flags
def test_subsets_over_one_upload_equal_their_own_corpus():
    _need_gpu()
    from change3d_amd.caption_metrics import CaptionScorer
    hyps, refs, _ = fixture("tiny_vocab")
    hyps, refs = hyps[:24], refs[:24]
    scorer = CaptionScorer(DEV)
    scorer.add(hyps[:10], refs[:10])
    scorer.add(hyps[10:], refs[10:])                           # appended chunks are one corpus
    tables = []
    for sel in (None, list(range(0, 24, 2)), [23, 1, 5], [7]):
        check(hyps, refs, sel, scorer=scorer)
        idx = list(range(24)) if sel is None else sel
        status, table = table_of(scorer.run(sel))
        want = cr.document_frequency([refs[i] for i in idx])
        assert status == 0 and table == {key_of(g): int(c) for g, c in want.items()}
        tables.append(table)
    assert tables[0] != tables[1]                              # the document frequency is the subset's own
    sel = torch.tensor([3, 4], dtype=torch.int64, device=DEV)  # a device index list
    assert scorer.score(sel) == scorer.score([3, 4])


def test_nochange_bookkeeping_and_split():
    _need_gpu()
    from change3d_amd.caption_metrics import CaptionScorer
    nochange = [[10, 11, 12], [13, 14], [10, 11]]
    hyps = [[10, 11, 12], [1, 2], [13, 14], None, [10, 11, 12, 1], [10, 11]]
    refs = [[[5, 6], [13, 14]],            # reference 1 and the hypothesis: both
            [[5], [10, 11, 12]],           # reference 1 only
            [[13, 14], [7, 8]],            # the hypothesis only (reference 0 does not count)
            [[5, 6], [10, 11]],            # reference 1, no caption
            [[10, 11, 12], [10, 11, 12, 1]],   # a prefix / an extension is no match
            [[5], [10, 11, 13]]]
    scorer = CaptionScorer(DEV)
    scorer.add(hyps, refs)
    out = scorer.run(None, nochange)
    assert out["flags"].cpu().tolist() == [3, 1, 2, 1, 0, 2]
    assert out["totals"][10:14].cpu().tolist() == [3, 1, 3, 1] and int(out["totals"][16]) == 0
    idx_n, idx_c, acc_n, acc_c = scorer.split(nochange)
    want = cr.split_corpus(hyps, refs, nochange)
    assert (idx_n, idx_c) == want[:2] and acc_n == want[2] / len(idx_n) and acc_c == want[3] / len(idx_c)
    check(hyps, refs, idx_n, scorer=scorer)
    check(hyps, refs, idx_c, scorer=scorer)
    assert scorer.split([]) == ([], list(range(6)), None, 1.0)     # no table: every pair is a change pair
    one = CaptionScorer(DEV)                                       # a single reference is the flagged one
    one.add([[1], [13, 14]], [[[13, 14]], [[2]]])
    assert one.run(None, nochange)["flags"].cpu().tolist() == [1, 2]


def test_strip_on_the_device():
    _need_gpu()
    from change3d_amd import ops
    from change3d_amd.caption_metrics import CaptionScorer
    S, E, P = 98, 99, 0
    rng = np.random.default_rng(5)
    raw_h = rng.integers(1, 98, size=(6, 70)).astype(np.int32)         # 70 raw columns: two passes of 64
    raw_h[0, [0, 1, 30, 68, 69]] = [S, S, P, E, P]                     # both ends and the middle
    raw_h[0, 40:50] = P
    raw_h[1, 3:] = P                                                   # three words, then padding
    raw_h[2, :] = P                                                    # nothing left: an empty hypothesis
    raw_h[3, :] = np.where(np.arange(70) % 2 == 0, E, raw_h[3])        # every other token
    raw_h[4, 64:] = P                                                  # exactly 64 kept
    raw_h[5, 5:] = E
    raw_r = rng.integers(1, 98, size=(6, 2, 52)).astype(np.int32)
    raw_r[:, :, 0] = S
    raw_r[:, :, 20] = E
    raw_r[:, :, 21:] = P
    raw_r[1, 1, 5] = P
    tok, n = ops.cap_strip(torch.from_numpy(raw_h).to(DEV), S, E, P)
    strip = lambda row: [int(w) for w in row if w not in (S, E, P)]    # noqa: E731  (reference scripts/train_CC.py:336-343)
    hyps, refs = [strip(r) for r in raw_h], [[strip(c) for c in caps] for caps in raw_r]
    assert n.cpu().tolist() == [len(h) for h in hyps] and max(map(len, hyps)) == 64 and min(map(len, hyps)) == 0
    for i, h in enumerate(hyps):
        assert tok[i].cpu().tolist() == h + [-1] * (64 - len(h))
    dev = CaptionScorer(DEV)
    dev.add(torch.from_numpy(raw_h).to(DEV), torch.from_numpy(raw_r).to(DEV).long(), strip=(S, E, P))
    _, scores, per = check(hyps, refs)
    got, got_per = dev.score(per_image=True)
    assert got == scores and all(torch.equal(got_per[k], per[k]) for k in per)


def test_bad_input_is_a_status_not_a_fault():
    _need_gpu()
    from change3d_amd._lib import Change3DHipError
    from change3d_amd.caption_metrics import CaptionScorer
    long_row = torch.full((1, 70), 7, dtype=torch.int32, device=DEV)   # 70 tokens are left after stripping
    ref = torch.tensor([[[1, 2, 3]]], dtype=torch.int32, device=DEV)
    scorer = CaptionScorer(DEV)
    scorer.add(long_row, ref, strip=(97, 98, 99))
    with pytest.raises(Change3DHipError, match="longer than 64"):
        scorer.score()
    scorer = CaptionScorer(DEV)
    scorer.add(torch.tensor([[1, 70000]], dtype=torch.int32, device=DEV), ref, strip=(97, 98, 99))
    with pytest.raises(Change3DHipError, match="status 4"):
        scorer.score()
    scorer = CaptionScorer(DEV)
    scorer.add([[1], [2]], [[[1]], [[2]]])
    with pytest.raises(Change3DHipError, match="outside the corpus"):
        scorer.score([0, 2])
    with pytest.raises(Change3DHipError, match="outside the corpus"):
        scorer.score([-1])
    assert scorer.score([1, 0])["Bleu_1"] > 0.99


# ------------------------------------------------------------------------------------------------------------ the table
@functools.lru_cache(maxsize=None)
def table_corpus(limit=16384):
    """vocabulary 30, 5 references of 3..12 words: images are added while their distinct reference n-grams still fit `limit`
    slots, so the smallest capacity that fits is almost full"""
    hyps, refs = random_corpus(400, 5, 30, (3, 12), seed=77)
    seen, n = set(), 0
    for rs in refs:
        new = seen | {g for r in rs for g in cr.precook(r)}
        if len(new) > limit:
            break
        seen, n = new, n + 1
    return hyps[:n], refs[:n], len(seen)


def test_table_at_the_plans_capacity_and_at_the_smallest_that_fits():
    _need_gpu()
    from change3d_amd import ops
    hyps, refs, distinct = table_corpus()
    assert 200 <= len(hyps) <= 400 and 16384 - 200 < distinct <= 16384, (len(hyps), distinct)
    want = {key_of(g): int(c) for g, c in cr.document_frequency(refs).items()}
    ref_tokens = sum(len(r) for rs in refs for r in rs)
    scorer, scores, per = check(hyps, refs)                    # the plan's capacity
    out = scorer.run()
    assert out["capacity"] == ops.cap_metrics_plan(len(hyps), 5, 64, ref_tokens)[1] >= 8 * ref_tokens
    assert table_of(out) == (0, want)
    _, tight, tight_per = check(hyps, refs, table_capacity=16384, scorer=scorer)   # > 98 % full: long probes, wrap-around
    assert table_of(scorer.run(table_capacity=16384)) == (0, want)
    assert tight == scores and all(torch.equal(tight_per[k], per[k]) for k in per)  # the capacity changes no bit


def test_table_too_small_is_reported_and_stays_inside_its_buffer():
    _need_gpu()
    from change3d_amd import ops
    from change3d_amd._lib import Change3DHipError
    from change3d_amd.caption_metrics import CaptionScorer
    hyps, refs, distinct = table_corpus()
    scorer = CaptionScorer(DEV)
    scorer.add(hyps, refs)
    with pytest.raises(Change3DHipError, match="table is full"):
        scorer.score(table_capacity=8192)
    nbytes, cap = ops.cap_metrics_plan(len(hyps), 5, 64, table_capacity=8192)
    ws = torch.full((nbytes + 4096,), 0xA5, dtype=torch.uint8, device=DEV)
    out = ops.cap_metrics(*scorer.corpus(), table_capacity=8192, ws=ws)
    status, table = table_of(out)
    assert status == 1 and int(out["totals"][16]) == 1 and len(table) == 8192     # full, and every slot holds a real n-gram
    want = cr.document_frequency(refs)
    assert all(table[k] == int(want_c) for k, want_c in ((key_of(g), c) for g, c in want.items()) if k in table)
    assert set(table) <= {key_of(g) for g in want}
    assert bool((ws[nbytes:] == 0xA5).all())                                       # nothing behind the table was touched
    assert bool((out["cider"] == 0).all())                                         # no score rather than a wrong one
    assert torch.equal(out["stats"].cpu().long(), torch.from_numpy(cr.score_corpus(hyps, refs)["stats"]))


def test_two_runs_agree_bit_for_bit():
    _need_gpu()
    from change3d_amd.caption_metrics import CaptionScorer
    hyps, refs, _ = table_corpus()
    scorer = CaptionScorer(DEV)
    scorer.add(hyps, refs)
    a, b = scorer.run(), scorer.run()
    for k in ("stats", "lcs", "flags", "rouge", "cider", "totals"):
        assert torch.equal(a[k], b[k]), k
    assert table_of(a) == table_of(b)                          # as sets: the slot order may differ


def test_last_kernel_names_the_metrics_kernel():
    _need_gpu()
    from change3d_amd import ops
    from change3d_amd.caption_metrics import CaptionScorer
    scorer = CaptionScorer(DEV)
    scorer.add([[1, 2]], [[[1, 2, 3]]])
    n0 = ops.launch_count()
    scorer.score()
    assert ops.last_kernel() == "cap_metrics_reduce_kernel" and ops.launch_count() - n0 == 3
    ops.cap_strip(torch.zeros((2, 5), dtype=torch.int32, device=DEV), 1, 2, 3)
    assert ops.last_kernel() == "cap_strip_kernel"


def test_refused_shapes():
    _need_gpu()
    from change3d_amd import ops
    from change3d_amd._lib import Change3DHipError
    z = lambda *s: torch.ones(s, dtype=torch.int32, device=DEV)   # noqa: E731
    with pytest.raises(Change3DHipError):
        ops.cap_metrics(z(2, 65), z(2), z(2, 1, 65), z(2, 1))      # rows wider than a wave
    with pytest.raises(Change3DHipError):
        ops.cap_metrics(z(2, 8), z(2), z(2, 8, 8), z(2, 8))        # eight references


# ----------------------------------------------------------------------------------------------------------- the script
def test_validate_scores_the_captions_it_produced(capsys):
    _need_gpu()
    import beam_reference as BR
    from change3d_amd.caption_metrics import CaptionScorer
    from change3d_amd.model.trainer import Trainer
    from change3d_amd.scripts.train_CC import validate
    from change3d_amd import synthetic
    from oracle import caption as oc, synth
    (seed, es, end_id, beam), seeds = BR.MARGIN_ROWS[0]
    args, ora, sd, _ = oc.beam_case(seed, es)
    V = args.vocab_size
    with contextlib.redirect_stdout(io.StringIO()):
        net = Trainer(args)
    net.load_state_dict(sd)
    net = net.to(DEV)
    args.beam_size = beam
    pairs = []
    for d in seeds[:5]:
        pre, post, _ = synth.synth_batch(1, 32, seed=d)
        pairs.append((pre.to(DEV), post.to(DEV)))
    start_id, pad_id = V - 2, 0
    allcaps = synthetic.synth_captions(5 * 3, seed=2, vocab_size=V, max_len=20)[0].view(5, 3, -1)
    allcaps = torch.where(allcaps == V - 1, end_id, allcaps)                        # this case's <end> id
    special = {start_id, end_id, pad_id}
    refs = [[[w for w in c if w not in special] for c in caps] for caps in allcaps.tolist()]
    nochange = [refs[1][1], refs[3][1]]
    metrics, hyps = validate(args, net, pairs, allcaps, (start_id, end_id, pad_id), nochange_rows=nochange, eval_batch=4,
                             return_hyps=True)
    assert sorted(metrics) == ["Bleu_1", "Bleu_2", "Bleu_3", "Bleu_4", "CIDEr", "ROUGE_L"]
    scorer = CaptionScorer(DEV)
    scorer.add(hyps, refs)
    assert metrics == scorer.score()
    want = cr.score_corpus(hyps, refs)
    assert [metrics[f"Bleu_{k}"] for k in range(1, 5)] == [want[f"Bleu_{k}"] for k in range(1, 5)]
    assert close(metrics["ROUGE_L"], want["ROUGE_L"]) and close(metrics["CIDEr"], want["CIDEr"])
    text = capsys.readouterr().out
    for line in ("len(nochange_references): 2", "len(change_references): 3", "nochange_metric:", "change_metric:", "nochange_acc:",
                 "change_acc:", "ROUGE_L ", "CIDEr "):
        assert line in text, text
