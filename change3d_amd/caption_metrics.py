"""Caption scores of a change-captioning validation pass, computed on the device (csrc/caption_metrics.hip): what the
reference's `eval_caption_score` (model/utils.py:509-530) returns -- Bleu_1..Bleu_4, ROUGE_L, CIDEr -- without METEOR, which
drives a java process and is not computed (no substitute value is invented: the key is absent), plus the change / no-change
split of reference scripts/train_CC.py:347-376.

    scorer = CaptionScorer(device)
    scorer.add(hyps, refs)                                   # lists as `evaluate()` yields them, or device tensors + strip=
    idx_n, idx_c, acc_n, acc_c = scorer.split(nochange_rows)
    scores = scorer.score()                                  # or score(select=idx_c): CIDEr's document frequency is the subset's

The corpus is uploaded once; every `score` is one C call (a memset and three launches) and one host synchronisation."""
import math

import numpy as np
import torch

from . import _lib as L
from . import ops

MAX_LEN = 64          # tokens of a sentence: one wave64 lane per position
MAX_TOKEN = 65534     # an n-gram key holds token + 1 in 16 bits


def pack_sentences(sents):
    """list of token lists -> (int32 [n, 64] padded with -1, int32 [n] lengths).  ValueError for a sentence longer than 64 or a
    token outside [0, 65534]."""
    tok = np.full((len(sents), MAX_LEN), -1, dtype=np.int32)
    lens = np.zeros(len(sents), dtype=np.int32)
    for i, s in enumerate(sents):
        s = [int(t) for t in s]
        if len(s) > MAX_LEN:
            raise ValueError(f"a sentence of {len(s)} tokens: the caption metrics take at most {MAX_LEN}")
        if s and (min(s) < 0 or max(s) > MAX_TOKEN):
            raise ValueError(f"token {min(s) if min(s) < 0 else max(s)} outside [0, {MAX_TOKEN}]")
        tok[i, :len(s)] = s
        lens[i] = len(s)
    return tok, lens


def pack_corpus(hyps, refs):
    """(hyps, refs) as `evaluate()` and the loader yield them -- hyps[i] a token list or None (no caption: an empty hypothesis),
    refs[i] the R reference token lists of image i -- -> hyp [N, 64], hyp_len [N], refs [N, R, 64], ref_len [N, R] (numpy int32).
    ValueError for a reference with no tokens: the reference's `"".split(" ")` is `[""]` there, two empty strings would score
    1, and no data set has such a reference."""
    if len(hyps) != len(refs) or not len(hyps):
        raise ValueError(f"{len(hyps)} hypotheses for {len(refs)} images")
    R = len(refs[0])
    if R < 1 or R > L.CAP_METRICS_MAX_REFS or any(len(r) != R for r in refs):
        raise ValueError(f"every image needs the same number of references, 1 .. {L.CAP_METRICS_MAX_REFS}")
    if any(len(s) == 0 for r in refs for s in r):
        raise ValueError("a reference with no tokens")
    h, hl = pack_sentences([[] if s is None else s for s in hyps])
    r, rl = pack_sentences([s for rs in refs for s in rs])
    return h, hl, r.reshape(len(hyps), R, MAX_LEN), rl.reshape(len(hyps), R)


def bleu_from_totals(totals):
    """Bleu_1..4 from (testlen, reflen, guess[4], correct[4]) summed over the corpus, in Python floats with the reference's
    expressions (eval_func/bleu/bleu_scorer.py:247-256)."""
    small = 1e-9
    tiny = 1e-15
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


_STATUS = {L.CAP_ST_TABLE_FULL: "the document-frequency table is full (table_capacity too small)",
           L.CAP_ST_BAD_SELECTION: "a selection index lies outside the corpus",
           L.CAP_ST_BAD_SENTENCE: "a sentence is longer than 64 tokens after stripping, holds a token outside [0, 65534], or a "
                                  "reference is empty"}


class CaptionScorer:
    def __init__(self, device="cuda"):
        self.device = torch.device(device)
        self._chunks = []          # (hyp, hyp_len, refs, ref_len): numpy (not uploaded yet) or device tensors
        self._corpus = None
        self._ref_tokens = 0       # upper bound of the sum of the reference lengths: sizes the table
        self.R = None

    def __len__(self):
        return sum(int(c[0].shape[0]) for c in self._chunks)

    def add(self, hyp, refs, strip=None):
        """Lists: `hyp` the hypotheses of some images (token lists, None = no caption), `refs` their reference lists, special
        tokens already removed.  Tensors: `hyp` int [B, Lh], `refs` int [B, R, Lr] raw rows on the device and `strip` =
        (start_id, end_id, pad_id), removed there (c3d_cap_strip); nothing is read back."""
        if torch.is_tensor(hyp):
            if strip is None or len(strip) != 3:
                raise ValueError("device rows need strip=(start_id, end_id, pad_id)")
            ops.require_gpu(hyp, "CaptionScorer.add hypotheses")
            ops.require_gpu(refs, "CaptionScorer.add references")
            B, R = int(refs.shape[0]), int(refs.shape[1])
            if hyp.dim() != 2 or refs.dim() != 3 or hyp.shape[0] != B or not 1 <= R <= L.CAP_METRICS_MAX_REFS:
                raise ValueError(f"hyp {tuple(hyp.shape)} / refs {tuple(refs.shape)}: want [B, Lh] and [B, R <= 7, Lr]")
            h, hl = ops.cap_strip(hyp.to(torch.int32).contiguous(), *strip)
            r, rl = ops.cap_strip(refs.to(torch.int32).reshape(B * R, -1).contiguous(), *strip)
            chunk = (h, hl, r.view(B, R, MAX_LEN), rl.view(B, R))
            self._ref_tokens += B * R * min(int(refs.shape[2]), MAX_LEN)
        else:
            chunk = pack_corpus(hyp, refs)
            R = chunk[2].shape[1]
            self._ref_tokens += int(chunk[3].sum())
        if self.R is not None and R != self.R:
            raise ValueError(f"{R} references per image after {self.R}")
        self.R = R
        self._chunks.append(chunk)
        self._corpus = None

    def corpus(self):
        """The four device tensors of everything added so far (uploaded and concatenated once)."""
        if self._corpus is None:
            if not self._chunks:
                raise ValueError("CaptionScorer: nothing was added")
            parts = [[t if torch.is_tensor(t) else torch.from_numpy(t).to(self.device) for t in c] for c in self._chunks]
            self._corpus = tuple(torch.cat([p[k] for p in parts]).contiguous() for k in range(4))
            self._chunks = [self._corpus]
        return self._corpus

    def _index(self, select):
        if select is None:
            return None
        if torch.is_tensor(select):
            return select.to(device=self.device, dtype=torch.int32).contiguous()
        if len(select) == 0:
            raise ValueError("an empty selection has no score")
        return torch.tensor([int(i) for i in select], dtype=torch.int32, device=self.device)

    def run(self, select=None, nochange=None, table_capacity=0):
        """One c3d_cap_metrics call; everything stays on the device (ops.cap_metrics's dict)."""
        hyp, hyp_len, refs, ref_len = self.corpus()
        nc = nc_len = None
        if nochange is not None and len(nochange):
            a, b = pack_sentences(nochange)
            nc, nc_len = torch.from_numpy(a).to(self.device), torch.from_numpy(b).to(self.device)
        return ops.cap_metrics(hyp, hyp_len, refs, ref_len, sel=self._index(select), nochange=nc, nochange_len=nc_len,
                               ref_tokens=self._ref_tokens, table_capacity=table_capacity)

    @staticmethod
    def _totals(out):
        totals = out["totals"].cpu()                          # the one host synchronisation
        status = int(totals[16])
        if status:
            raise L.Change3DHipError("c3d_cap_metrics: " + "; ".join(m for bit, m in _STATUS.items() if status & bit) +
                                     f" (status {status})")
        return totals

    def score(self, select=None, per_image=False, table_capacity=0):
        """{"Bleu_1", .., "Bleu_4", "ROUGE_L", "CIDEr"} of the whole corpus or of the images in `select` (indices in the order
        they were added).  `per_image=True`: (scores, {"stats" i32 [M, 10], "lcs" i32 [M, R], "rouge" f64 [M], "cider" f64 [M]}),
        the arrays on the device."""
        out = self.run(select, None, table_capacity)
        totals = self._totals(out)
        M = int(out["stats"].shape[0])
        bleus = bleu_from_totals([int(v) for v in totals[:10]])
        sums = totals[14:16].view(torch.float64)
        scores = {f"Bleu_{k + 1}": bleus[k] for k in range(4)}
        scores["ROUGE_L"] = float(sums[0]) / M
        scores["CIDEr"] = float(sums[1]) / M
        if per_image:
            return scores, {k: out[k] for k in ("stats", "lcs", "rouge", "cider")}
        return scores

    def split(self, nochange_rows):
        """scripts/train_CC.py:347-376 on token rows: (indices of the images whose reference 1 is one of `nochange_rows`, indices
        of the others, nochange_acc, change_acc) -- the share of the first whose hypothesis is a no-change sentence too, and of
        the second whose hypothesis is none; None for an empty side."""
        out = self.run(None, nochange_rows)
        totals = self._totals(out)
        flags = out["flags"].cpu()
        idx_n = torch.nonzero(flags & 1).flatten().tolist()
        idx_c = torch.nonzero((flags & 1) == 0).flatten().tolist()
        n_n, hit_n, n_c, hit_c = (int(v) for v in totals[10:14])
        assert n_n == len(idx_n) and n_c == len(idx_c)
        return idx_n, idx_c, (hit_n / n_n if n_n else None), (hit_c / n_c if n_c else None)
