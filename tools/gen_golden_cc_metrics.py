"""tests/golden/cc_metrics.npz: seeded token corpora and what the REAL reference scorers say about them (data only).

Imports the reference's `Bleu`, `Rouge` and `Cider` classes and nothing else of it (`model/utils.py` would pull in METEOR and
its java process), feeds them the strings `model/utils.py::eval_caption_score` builds (`' '.join(str(token))`), and records per
corpus `<name>_`: hyp / hyp_len / refs / ref_len (int32, rows padded with -1), stats (int64 [N, 10]: testlen, closest
reference length, guess[4], correct[4]), totals (their sums), bleu (f64 [4]), lcs (int32 [N, R]), rouge / cider (f64 [N]) and the
corpus means ROUGE_L / CIDEr.  Corpora hold at most 64 images.  The archive is written with fixed member dates and order, so
a second run reproduces it byte for byte.  Refuses to run without the reference tree.

Usage: python tools/gen_golden_cc_metrics.py [--out tests/golden/cc_metrics.npz]"""
import argparse
import io
import os
import sys
import zipfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import ref_import  # noqa: E402

LMAX = 64


def corpora():
    """name -> (hyps, refs): lists of token lists.  Every path of the kernels' tests has a corpus here."""
    out = {}
    rng = np.random.default_rng(20260)

    def sent(n, vocab, lo=0):
        return [int(t) for t in rng.integers(lo, lo + vocab, size=n)]

    def noisy(ref, vocab, p):
        """a hypothesis near `ref`: words dropped, replaced or repeated with probability p each"""
        h = []
        for t in ref:
            u = rng.random()
            if u < p:
                continue
            h.append(int(rng.integers(0, vocab)) if u < 2 * p else t)
            if u > 1 - p:
                h.append(t)
        return h[:LMAX]

    # captions as the LEVIR-CC loader yields them: 5 references of 5..50 words over 501 ids, a hypothesis near one of them
    hyps, refs = [], []
    for i in range(48):
        r = [sent(int(rng.integers(5, 51)), 499, 1) for _ in range(5)]
        refs.append(r)
        hyps.append(noisy(r[i % 5], 499, 0.15))
    out["levir"] = (hyps, refs)

    # vocabulary 2..4: repeated n-grams, tf > 1, clipping; every short and the two longest hypothesis lengths
    hyps, refs = [], []
    lens_h = [0, 1, 2, 3, 4, 63, 64] + [int(v) for v in rng.integers(0, 65, size=57)]
    for i, lh in enumerate(lens_h):
        v = 2 + i % 3
        refs.append([sent(int(rng.choice([1, 2, 3, 5, 8, 20, 64])), v) for _ in range(5)])
        hyps.append(sent(lh, v))
    out["tiny_vocab"] = (hyps, refs)

    # one image, one reference: ref_len is 1, not log 1
    out["single"] = ([[3, 4, 5, 4, 5]], [[[3, 4, 5, 6, 4, 5]]])

    # two images that share every reference n-gram (idf exactly 0: the zero-norm branch) next to n-grams of one image only
    out["pair"] = ([[7, 8, 9], [7, 8, 9, 10, 11]], [[[7, 8, 9]], [[7, 8, 9, 10, 12]]])

    # seven images: tokens 0 and 65534 ((0,) against (0, 0), the top field), closest-length ties on both sides, an empty hypothesis
    hyps = [[0, 0, 65534, 0], [65534] * 6, [0] * 5, [], [1, 2, 3, 4, 5, 6], [0, 65534, 0, 65534], [5, 5, 5]]
    refs = [[[0, 0, 0], [0, 65534, 0, 0, 65534], [65534, 0], [0], [0, 0, 65534, 0, 1]],
            [[65534] * 4, [65534] * 8, [65534, 0] * 3, [0, 65534], [65534]],
            [[0] * 7, [0] * 3, [0, 0], [0] * 64, [1, 0]],
            [[1, 2], [3], [1, 2, 3], [2, 2], [1]],
            [[1, 2, 3, 4], [1, 2, 3, 4, 5, 6, 7, 8], [6, 5, 4, 3, 2, 1], [1, 3, 5], [2, 4, 6, 1, 2, 3, 4]],
            [[0, 65534] * 32, [65534, 0] * 2, [0], [65534], [0, 65534, 0]],
            [[5], [5, 5], [5, 5, 5, 5, 5], [6, 5], [5, 6, 5, 5]]]
    out["edges"] = (hyps, refs)
    return out


def pack(sents):
    a = np.full((len(sents), LMAX), -1, dtype=np.int32)
    for i, s in enumerate(sents):
        a[i, :len(s)] = s
    return a, np.array([len(s) for s in sents], dtype=np.int32)


def score_with_reference(hyps, refs):
    sys.dont_write_bytecode = True
    if ref_import.REFERENCE_ROOT not in sys.path:
        sys.path.insert(0, ref_import.REFERENCE_ROOT)
    from eval_func.bleu.bleu import Bleu
    from eval_func.cider.cider import Cider
    from eval_func.rouge.rouge import Rouge
    hypo = [[" ".join(str(x) for x in h)] for h in hyps]
    ref = [[" ".join(str(x) for x in r) for r in rs] for rs in refs]
    bleu, _ = Bleu(4).compute_score(ref, hypo)
    rouge_mean, rouge = Rouge().compute_score(ref, hypo)
    cider_mean, cider = Cider().compute_score(ref, hypo)
    # the integers behind BLEU, from the scorer the Bleu class drives
    scorer = sys.modules[Bleu.__module__].BleuScorer(n=4)
    for h, r in zip(hypo, ref):
        scorer += (h[0], r)
    scorer.compute_score(option="closest")
    stats = np.array([[c["testlen"], scorer._single_reflen(c["reflen"], "closest", c["testlen"])] + c["guess"] + c["correct"]
                      for c in scorer.ctest], dtype=np.int64)
    my_lcs = sys.modules[Rouge.__module__].my_lcs
    lcs = np.array([[my_lcs(r.split(" "), h[0].split(" ")) for r in rs] for h, rs in zip(hypo, ref)], dtype=np.int32)
    return {"stats": stats, "totals": stats.sum(0), "bleu": np.array(bleu, dtype=np.float64), "lcs": lcs,
            "rouge": np.asarray(rouge, dtype=np.float64), "cider": np.asarray(cider, dtype=np.float64),
            "ROUGE_L": np.float64(rouge_mean), "CIDEr": np.float64(cider_mean)}


def write_npz(path, arrays):
    """np.savez with fixed member dates: the same arrays give the same bytes"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_STORED) as z:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asarray(arrays[name]), allow_pickle=False)
            z.writestr(zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "cc_metrics.npz"))
    args = ap.parse_args()
    if not os.path.isdir(os.path.join(ref_import.REFERENCE_ROOT, "eval_func")):
        raise SystemExit("gen_golden_cc_metrics: the reference tree is not present; the fixture can only be generated next to it")
    arrays = {}
    for name, (hyps, refs) in corpora().items():
        assert len(hyps) <= 64 and len({len(r) for r in refs}) == 1
        h, hl = pack(hyps)
        r, rl = pack([s for rs in refs for s in rs])
        R = len(refs[0])
        rec = score_with_reference(hyps, refs)
        rec.update({"hyp": h, "hyp_len": hl, "refs": r.reshape(len(hyps), R, LMAX), "ref_len": rl.reshape(len(hyps), R)})
        for k, v in rec.items():
            arrays[f"{name}_{k}"] = v
        print(f"[gen_golden_cc_metrics] {name}: {len(hyps)} images x {R} references  Bleu_4 {rec['bleu'][3]:.4f} ROUGE_L "
              f"{rec['ROUGE_L']:.4f} CIDEr {rec['CIDEr']:.4f}")
    write_npz(args.out, arrays)
    print(f"[gen_golden_cc_metrics] wrote {args.out} ({os.path.getsize(args.out) / 1024:.1f} kB)")


if __name__ == "__main__":
    main()
