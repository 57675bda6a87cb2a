#!/usr/bin/env python
"""Time the captioning `evaluate()` of the CC task: the per-pair loop (`CaptionDecoder.beam_search`) against the batched,
device-resident search (`beam_search_batch`, csrc/caption_beam.hip) at batch 1, 16 and 64 -- all in ONE process and call, after
a warm-up pass of every configuration, with torch.cuda.synchronize() around every timed region; the encoder and the search are
timed separately.

    python tools/cc_eval_step.py --pairs 64 > profiles/cc_eval_batch.txt

Untrained synthetic weights rarely emit a given <end>, so a search would always run all 51 steps.  The tool therefore takes
<end> from a preliminary decode (a word that the first pairs' best hypotheses hold mid-sequence), which ends part of the
hypotheses early, and reports time per decoded step as well as per pair.  A decoded step is one pass of the decoder over the
live hypotheses of ONE pair: `us/step` = search time / sum over the pairs of the steps their searches ran (for the loop the
steps are counted as embedding launches, one per step)."""
import argparse
import contextlib
import io
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from change3d_amd import ops, synthetic as synth  # noqa: E402
from change3d_amd.model.trainer import Trainer  # noqa: E402
from change3d_amd.scripts.train_CC import encode_memory  # noqa: E402


def sync_time(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, time.perf_counter() - t0


def memory_of(model, pre, post):
    return encode_memory(model, pre, post)


def run_loop(model, pre, post, start_id, end_id, beam):
    """Today's evaluate(): one pair at a time.  Returns (encoder s, search s, steps per pair, hypotheses)."""
    t_enc = t_search = 0.0
    steps, hyps = [], []
    counted = [0]
    real = ops.cap_embed_fwd

    def counting(*a, **k):
        counted[0] += 1
        return real(*a, **k)
    ops.cap_embed_fwd = counting
    try:
        for i in range(pre.shape[0]):
            mem, dt = sync_time(lambda: memory_of(model, pre[i:i + 1], post[i:i + 1]))
            t_enc += dt
            counted[0] = 0
            res, dt = sync_time(lambda: model.decoder.beam_search(mem, start_id, end_id, beam))
            t_search += dt
            steps.append(counted[0])
            hyps.append(res[0])
    finally:
        ops.cap_embed_fwd = real
    return t_enc, t_search, steps, hyps


def run_batched(model, pre, post, start_id, end_id, beam, n):
    t_enc = t_search = 0.0
    steps, hyps = [], []
    for i in range(0, pre.shape[0], n):
        mem, dt = sync_time(lambda: memory_of(model, pre[i:i + n], post[i:i + n]))
        t_enc += dt
        res, dt = sync_time(lambda: model.decoder.beam_search_batch(mem, start_id, end_id, beam))
        t_search += dt
        steps += model.decoder.last_search_steps
        hyps += [r[0] for r in res]
    return t_enc, t_search, steps, hyps


def pick_end(model, pre, post, start_id, beam):
    """<end> from a preliminary decode without one: the word that most of the first pairs' surviving best hypotheses hold
    somewhere in positions 3..40, so that part of the searches complete early."""
    mem = memory_of(model, pre[:8], post[:8])
    _, traces = model.decoder.beam_search_batch(mem, start_id, -1, beam, return_trace=True)
    count = {}
    for tr in traces:
        seen = {sel[0][1] for _, sel in tr[2:40]}
        for w in seen:
            count[w] = count.get(w, 0) + 1
    half = [w for w, c in sorted(count.items()) if 2 <= c <= 6]
    return half[0] if half else max(count, key=count.get)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--pairs", type=int, default=64)
    p.add_argument("--size", type=int, default=256)
    p.add_argument("--vocab_size", type=int, default=501)
    p.add_argument("--reps", type=int, default=2)
    a = p.parse_args()
    dev = torch.device("cuda:0")
    print(f"# tools/cc_eval_step.py: {a.pairs} synthetic pairs at {a.size} x {a.size}, vocabulary {a.vocab_size}, "
          f"{torch.cuda.get_device_name(0)}; csrc digest {__import__('change3d_amd')._lib.csrc_digest()}")
    print("# one process, one call; warm-up pass of every configuration first; synchronize around every timed region")
    print("# us/step = search time / decoded steps summed over the pairs; loop = per-pair beam_search (the parent path)")
    pre, post, _ = (t.to(dev) for t in synth.synth_batch(a.pairs, a.size, seed=1))
    for dtype, name in ((torch.float32, "f32"), (torch.bfloat16, "bf16")):
        args = synth.make_cc_args(size=a.size, vocab_size=a.vocab_size, dropout=0.0)
        args.act_dtype = dtype
        torch.manual_seed(16)
        with contextlib.redirect_stdout(io.StringIO()):
            model = Trainer(args).to(dev)
        model.eval()
        with torch.no_grad():
            model.decoder.vocab_embedding.weight.mul_(100.0)      # U(-10, 10): hypotheses that depend on their history
        start_id = a.vocab_size - 2
        for beam in (1, 3):
            with torch.no_grad():
                end_id = pick_end(model, pre, post, start_id, beam)
                configs = [("loop", lambda: run_loop(model, pre, post, start_id, end_id, beam))] + \
                          [(f"batch {n}", (lambda n=n: run_batched(model, pre, post, start_id, end_id, beam, n))) for n in (1, 16, 64)]
                for _, fn in configs:                                 # warm-up
                    fn()
                print(f"\n{name} beam {beam} <end> {end_id}")
                base = None
                for label, fn in configs:
                    rows = [fn() for _ in range(a.reps)]
                    enc = [r[0] / a.pairs * 1e3 for r in rows]
                    srch = [r[1] / a.pairs * 1e3 for r in rows]
                    per_step = [r[1] / max(sum(r[2]), 1) * 1e6 for r in rows]
                    steps, hyps = rows[0][2], rows[0][3]
                    if base is None:
                        base = hyps
                    same = sum(x == y for x, y in zip(hyps, base))
                    spread = (max(per_step) - min(per_step)) / min(per_step) * 100
                    print(f"  {label:9s} encoder {min(enc):8.3f} ms/pair  search {min(srch):8.3f} ms/pair  {min(per_step):8.2f} us/step "
                          f"(reps: {', '.join(f'{x:.2f}' for x in per_step)}; spread {spread:.1f} %)  steps/pair mean "
                          f"{sum(steps) / len(steps):.1f} min {min(steps)} max {max(steps)}  captions {sum(h is not None for h in hyps)}  "
                          f"same best as loop {same}/{len(hyps)}")


if __name__ == "__main__":
    main()
