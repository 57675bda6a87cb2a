"""Caption metrics on the device against the host scorers, one process on the MI355X: a LEVIR-CC-sized corpus (1 929 pairs, 5
references of 5..50 words, vocabulary 501, about half of the pairs "no change") is packed and uploaded once and scored three
times as the validation does -- the no-change subset, the change subset, all pairs.  Reports the device time of each scoring
call (events around c3d_cap_metrics), the wall time of `CaptionScorer.score` with its one synchronisation, the packing and
upload of the list inputs, the plain-Python restatement of the reference scorers (tests/caption_metrics_reference.py) on the
same host, and the worst |device - restatement| / bound of the per-image ROUGE-L and CIDEr (bound = 1e-12 relative + 1e-15).

Usage: python tools/caption_metrics_step.py [--out profiles/caption_metrics.txt] [--pairs 1929] [--reps 20]"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import caption_metrics_reference as cr  # noqa: E402
from change3d_amd import _lib, ops  # noqa: E402
from change3d_amd.caption_metrics import CaptionScorer  # noqa: E402

NOCHANGE = [[1, 2, 3, 4, 5, 6, 7], [8, 3, 9, 10], [1, 11, 2, 12, 13], [9, 14, 15, 16], [17, 18, 15, 19]]


def corpus(n, seed=1929):
    rng = np.random.default_rng(seed)
    hyps, refs = [], []
    for i in range(n):
        rs = [[int(t) for t in rng.integers(1, 499, size=int(rng.integers(5, 51)))] for _ in range(5)]
        if i % 2:
            rs[1] = list(NOCHANGE[i % 5])
        h = [t if rng.random() > 0.2 else int(rng.integers(1, 499)) for t in rs[(i + 1) % 5]]
        hyps.append(h)
        refs.append(rs)
    return hyps, refs


def worst_ratio(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return float((np.abs(got - want) / (1e-12 * np.abs(want) + 1e-15)).max())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "caption_metrics.txt"))
    ap.add_argument("--pairs", type=int, default=1929)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    hyps, refs = corpus(args.pairs)
    say(f"caption metrics, {torch.cuda.get_device_name(0)}, csrc {_lib.csrc_digest()}")
    say(f"corpus: {args.pairs} pairs x 5 references, 5..50 words, vocabulary 501; {sum(len(r) for rs in refs for r in rs)} reference tokens")

    torch.zeros(1, device=dev)
    t0 = time.perf_counter()
    scorer = CaptionScorer(dev)
    scorer.add(hyps, refs)
    t1 = time.perf_counter()
    scorer.corpus()
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    say(f"list inputs: pack {1e3 * (t1 - t0):.1f} ms (host), upload {1e3 * (t2 - t1):.2f} ms (four copies, once per validation)")

    idx_n, idx_c, acc_n, acc_c = scorer.split(NOCHANGE)
    say(f"split: {len(idx_n)} no-change pairs (acc {acc_n:.4f}), {len(idx_c)} change pairs (acc {acc_c:.4f})")
    out = scorer.run()
    say(f"table: capacity {out['capacity']} slots, workspace {out['ws'].numel() / 1e6:.1f} MB")

    total_dev, total_wall = 0.0, 0.0
    for name, sel in (("no-change", idx_n), ("change", idx_c), ("all", None)):
        index = scorer._index(sel)
        scorer.run(index)
        torch.cuda.synchronize()
        ms, wall = [], []
        for _ in range(args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            scorer.run(index)
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
            w0 = time.perf_counter()
            scorer.score(index)
            wall.append(1e3 * (time.perf_counter() - w0))
        M = args.pairs if sel is None else len(sel)
        say(f"score {name:9s} M = {M:5d}: device {statistics.median(ms):7.3f} ms ({min(ms):.3f} .. {max(ms):.3f}; memset + 3 launches + "
            f"output allocation), CaptionScorer.score {statistics.median(wall):7.3f} ms wall with its synchronisation")
        total_dev += statistics.median(ms)
        total_wall += statistics.median(wall)
    say(f"three scoring calls: device {total_dev:.3f} ms, wall {total_wall:.3f} ms = {1e3 * total_wall / args.pairs:.2f} us per pair "
        f"(batched beam search: 170 .. 260 us per pair, profiles/cc_eval_batch.txt)")

    worst = {"ROUGE_L": 0.0, "CIDEr": 0.0}
    host = 0.0
    for name, sel in (("no-change", idx_n), ("change", idx_c), ("all", None)):
        idx = list(range(args.pairs)) if sel is None else sel
        t0 = time.perf_counter()
        want = cr.score_corpus([hyps[i] for i in idx], [refs[i] for i in idx])
        host += time.perf_counter() - t0
        scores, per = scorer.score(sel, per_image=True)
        assert torch.equal(per["stats"].cpu().long(), torch.from_numpy(want["stats"])), name
        assert [scores[f"Bleu_{k}"] for k in range(1, 5)] == [want[f"Bleu_{k}"] for k in range(1, 5)], name
        worst["ROUGE_L"] = max(worst["ROUGE_L"], worst_ratio(per["rouge"].cpu().numpy(), want["rouge"]))
        worst["CIDEr"] = max(worst["CIDEr"], worst_ratio(per["cider"].cpu().numpy(), want["cider"]))
        say(f"  {name:9s} Bleu_4 {scores['Bleu_4']:.6f} ROUGE_L {scores['ROUGE_L']:.6f} CIDEr {scores['CIDEr']:.6f}  (restatement "
            f"{want['Bleu_4']:.6f} {want['ROUGE_L']:.6f} {want['CIDEr']:.6f})")
    say(f"restatement on this host, the same three corpora: {host:.2f} s = {host / (1e-3 * total_wall):.0f} x the device scoring")
    say(f"BLEU statistics and Bleu_1..4 equal the restatement; worst |device - restatement| / (1e-12 |x| + 1e-15) per image: "
        f"ROUGE-L {worst['ROUGE_L']:.3e}, CIDEr {worst['CIDEr']:.3e}")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
