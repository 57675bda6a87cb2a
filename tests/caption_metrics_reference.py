"""Plain-Python restatement of the reference's caption scorers on token lists: BLEU-1..4 (eval_func/bleu/bleu_scorer.py),
ROUGE-L (eval_func/rouge/rouge.py) and CIDEr (eval_func/cider/cider_scorer.py) as `model/utils.py::eval_caption_score` calls
them, and the change / no-change bookkeeping of scripts/train_CC.py:347-376.  The same float64 operations in the same order
(numpy's log / sqrt / mean where the reference uses numpy's), so tests/golden/cc_metrics.npz -- recorded from the reference's
own classes by tools/gen_golden_cc_metrics.py -- is reproduced exactly.  The tests' yardstick on machines without the
reference tree; no METEOR (it drives a java process).

A sentence is a list of ints.  The reference joins `str(token)` with spaces: its `"".split()` is `[]` for BLEU and CIDEr, and
its `"".split(" ")` is `[""]` for ROUGE, so an empty hypothesis has ROUGE length 1 and matches nothing.

The keyword switches exist for the negative controls only: each one "repairs" a property the kernels must keep."""
import math

import numpy as np


def precook(words, n=4):
    """n-gram counts in the reference's dict order: order 1..n, ascending first occurrence."""
    counts = {}
    for k in range(1, n + 1):
        for i in range(len(words) - k + 1):
            g = tuple(words[i:i + k])
            counts[g] = counts.get(g, 0) + 1
    return counts


# ----------------------------------------------------------------------------------------------------------------- BLEU
def bleu_stats(hyp, refs, clip=True, tie_shorter=True):
    """The ten integers of one image: testlen, closest reference length, guess[4], correct[4]."""
    maxcounts = {}
    for ref in refs:
        for g, c in precook(ref).items():
            maxcounts[g] = max(maxcounts.get(g, 0), c)
    testlen = len(hyp)
    if tie_shorter:
        reflen = min((abs(len(r) - testlen), len(r)) for r in refs)[1]
    else:
        reflen = min((abs(len(r) - testlen), -len(r)) for r in refs)[1] * -1
    guess = [max(0, testlen - k + 1) for k in range(1, 5)]
    correct = [0] * 4
    for g, c in precook(hyp).items():
        correct[len(g) - 1] += min(maxcounts.get(g, 0), c) if clip else (c if g in maxcounts else 0)
    return [testlen, reflen] + guess + correct


def bleu_from_totals(totals):
    """Bleu_1..4 of a corpus from the sums of `bleu_stats` (bleu_scorer.py:247-256)."""
    small, tiny = 1e-9, 1e-15
    testlen, reflen, guess, correct = totals[0], totals[1], totals[2:6], totals[6:10]
    bleus = []
    bleu = 1.
    for k in range(4):
        bleu *= float(correct[k] + tiny) / (guess[k] + small)
        bleus.append(bleu ** (1. / (k + 1)))
    ratio = (testlen + tiny) / (reflen + small)
    if ratio < 1:
        for k in range(4):
            bleus[k] *= math.exp(1 - 1 / ratio)
    return bleus


# -------------------------------------------------------------------------------------------------------------- ROUGE-L
def lcs(a, b):
    if len(a) < len(b):
        a, b = b, a
    lengths = [[0] * (len(b) + 1) for _ in range(len(a) + 1)]
    for j in range(1, len(b) + 1):
        for i in range(1, len(a) + 1):
            if a[i - 1] == b[j - 1]:
                lengths[i][j] = lengths[i - 1][j - 1] + 1
            else:
                lengths[i][j] = max(lengths[i - 1][j], lengths[i][j - 1])
    return lengths[len(a)][len(b)]


def rouge_image(hyp, refs):
    """(score, [lcs per reference])"""
    beta = 1.2
    len_c = max(len(hyp), 1)
    ls = [lcs(r, hyp) for r in refs]
    prec_max = max(c / float(len_c) for c in ls)
    rec_max = max(c / float(len(r)) for c, r in zip(ls, refs))
    if prec_max != 0 and rec_max != 0:
        score = ((1 + beta ** 2) * prec_max * rec_max) / float(rec_max + beta ** 2 * prec_max)
    else:
        score = 0.0
    return score, ls


# ---------------------------------------------------------------------------------------------------------------- CIDEr
def document_frequency(refs_list):
    df = {}
    for refs in refs_list:
        for g in set(g for ref in refs for g in precook(ref)):
            df[g] = df.get(g, 0.0) + 1
    return df


def cider_images(hyps, refs_list, clip=True, bigram_length=True, length_penalty=True, sigma=6.0):
    """Per-image CIDEr of a corpus (cider_scorer.py:106-182); the document frequency is the corpus's own."""
    df_all = document_frequency(refs_list)
    ref_len = np.log(float(len(refs_list)))
    if len(refs_list) == 1:
        ref_len = 1

    def counts2vec(words):
        vec = [{} for _ in range(4)]
        length = 0
        norm = [0.0] * 4
        for g, tf in precook(words).items():
            df = np.log(max(1.0, df_all.get(g, 0.0)))
            n = len(g) - 1
            vec[n][g] = float(tf) * (ref_len - df)
            norm[n] += pow(vec[n][g], 2)
            if n == (1 if bigram_length else 0):
                length += tf
        return vec, [np.sqrt(x) for x in norm], length

    def sim(vec_h, vec_r, norm_h, norm_r, len_h, len_r):
        delta = float(len_h - len_r) if length_penalty else 0.0
        val = np.array([0.0] * 4)
        for n in range(4):
            for g in vec_h[n]:
                vr = vec_r[n].get(g, 0.0)
                val[n] += (min(vec_h[n][g], vr) if clip else vec_h[n][g]) * vr
            if norm_h[n] != 0 and norm_r[n] != 0:
                val[n] /= (norm_h[n] * norm_r[n])
            val[n] *= np.e ** (-(delta ** 2) / (2 * sigma ** 2))
        return val

    scores = []
    for hyp, refs in zip(hyps, refs_list):
        vec, norm, length = counts2vec(hyp)
        score = np.array([0.0] * 4)
        for ref in refs:
            vec_r, norm_r, len_r = counts2vec(ref)
            score += sim(vec, vec_r, norm, norm_r, length, len_r)
        score_avg = np.mean(score)
        score_avg /= len(refs)
        score_avg *= 10.0
        scores.append(score_avg)
    return np.array(scores)


# --------------------------------------------------------------------------------------------------------------- corpus
def score_corpus(hyps, refs_list, clip=True, bigram_length=True, tie_shorter=True, length_penalty=True):
    """What `eval_caption_score` returns without METEOR, plus the per-image pieces:
    {"Bleu_1".."Bleu_4", "ROUGE_L", "CIDEr", "stats" int64 [M, 10], "totals" [10], "lcs" [M][R], "rouge" f64 [M], "cider" f64 [M]}."""
    hyps = [[] if h is None else list(h) for h in hyps]
    for refs in refs_list:
        if any(len(r) == 0 for r in refs):
            raise ValueError("a reference with no tokens")
    stats = np.array([bleu_stats(h, r, clip, tie_shorter) for h, r in zip(hyps, refs_list)], dtype=np.int64).reshape(len(hyps), 10)
    totals = [int(v) for v in stats.sum(0)]
    bleus = bleu_from_totals(totals)
    rl = [rouge_image(h, r) for h, r in zip(hyps, refs_list)]
    rouge = np.array([s for s, _ in rl])
    cider = cider_images(hyps, refs_list, clip, bigram_length, length_penalty)
    out = {f"Bleu_{k + 1}": bleus[k] for k in range(4)}
    out.update({"ROUGE_L": np.mean(rouge), "CIDEr": np.mean(cider), "stats": stats, "totals": totals, "lcs": [l for _, l in rl],
                "rouge": rouge, "cider": cider})
    return out


def split_corpus(hyps, refs_list, nochange):
    """scripts/train_CC.py:347-376: (no-change indices, change indices, nochange_acc count, change_acc count).  An image is a
    no-change image when its reference 1 (reference 0 if it has only one) is one of the `nochange` sentences."""
    nochange = [list(s) for s in nochange]
    idx_n, idx_c, acc_n, acc_c = [], [], 0, 0
    for i, (h, refs) in enumerate(zip(hyps, refs_list)):
        h = [] if h is None else list(h)
        if list(refs[1 if len(refs) > 1 else 0]) in nochange:
            idx_n.append(i)
            acc_n += h in nochange
        else:
            idx_c.append(i)
            acc_c += h not in nochange
    return idx_n, idx_c, acc_n, acc_c
