"""Batched, device-resident beam search (`CaptionDecoder.beam_search_batch`, csrc/caption_beam.hip) on the GPU.

(a) identity with oracle.caption.beam_search, today's `beam_search` and tests/golden/cc_beam.npz on the inputs whose every
    decision has a margin (tests/beam_reference.py MARGIN_ROWS); batch composition does not matter;
(b) validity of every decision, through the trace, on inputs with exact ties (replay against the per-pair kernels);
(c) the key/value cache at op level: logits of the incremental path against the float64 full-window restatement
    (tests/caption_reference.py), and beam reordering against the same prefixes decoded in place, bit for bit;
(d) script level: `evaluate(..., eval_batch=N)` against the per-pair loop, the `--eval_batch` flag, the refused-shape fallback."""
import contextlib
import io
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import beam_reference as BR  # noqa: E402
import caption_reference as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# bf16: largest |score(batched search) - score(per-pair bf16 kernels)| over the trace of the 12-pair batch of (b), measured on
# an MI355X, times 4 as head-room for other machines (profiles/cc_eval_batch.txt holds the measurement)
DELTA_BF16 = 4 * 0.3752


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")


def _decoder(sd, args, dtype=torch.float32):
    from change3d_amd.model.caption_decoder import CaptionDecoder
    args.act_dtype = dtype
    with contextlib.redirect_stdout(io.StringIO()):
        dec = CaptionDecoder(args)
    dec.load_state_dict({k[len("decoder."):]: v for k, v in sd.items() if k.startswith("decoder.")})
    return dec.to(DEV).eval()


def _batch(ora, size, seeds):
    mems = [BR.memory_of(ora, size, d) for d in seeds]
    return mems, torch.cat(mems, dim=1).contiguous()


# ------------------------------------------------------------------------------------------------ (a) identity
@pytest.mark.parametrize("row", range(len(BR.MARGIN_ROWS)))
def test_batched_search_equals_oracle_on_margin_inputs(row, golden_dir):
    _need_gpu()
    from change3d_amd import ops
    from oracle import caption as oc
    (seed, es, end_id, beam), seeds = BR.MARGIN_ROWS[row]
    args, ora, sd, mem_committed = oc.beam_case(seed, es)
    V = args.vocab_size
    dec = _decoder(sd, args)
    mems, batch = _batch(ora, 32, seeds)
    got = dec.beam_search_batch(batch.to(DEV), V - 2, end_id, beam)
    assert ops.last_kernel() == "cap_beam_kernel<float>"
    assert dec.training is False and len(got) == len(seeds)
    golden = np.load(os.path.join(golden_dir, "cc_beam.npz"))
    for b, d in enumerate(seeds):
        margins = BR.search(BR.oracle_scorer(ora.decoder, mems[b]), V - 2, end_id, beam, V).min_gap
        assert min(margins) >= BR.MIN_MARGIN, (seed, d, margins)       # FAIL, not skip: no input may be left out
        want = oc.beam_search(ora.decoder, mems[b], V - 2, end_id, beam, V)
        pair = dec.beam_search(mems[b].to(DEV), V - 2, end_id, beam)
        for name, ref in (("oracle", want), ("per-pair kernels", pair)):
            assert got[b][0] == ref[0] and got[b][1] == ref[1], (name, seed, d, got[b], ref)
            err = np.abs(np.array(got[b][2]) - np.array(ref[2])).max() if ref[2] else 0.0
            print(f"weights {seed} data {d}: {len(ref[1])} completed, max |score - {name}| {err:.3e}")
            assert np.allclose(got[b][2], ref[2], rtol=0, atol=BR.DELTA_F32), (name, got[b][2], ref[2])
        if d == seed + 1:                                               # a committed case: through the REAL reference modules
            i = oc.BEAM_CASES.index((seed, beam, es, end_id))
            assert torch.equal(mems[b], mem_committed)
            assert (got[b][0] or []) == golden["best"][i, :int(golden["best_len"][i])].tolist()


def test_batch_composition_does_not_matter():
    _need_gpu()
    from oracle import caption as oc
    (seed, es, end_id, beam), seeds = BR.MARGIN_ROWS[0]
    args, ora, sd, _ = oc.beam_case(seed, es)
    V = args.vocab_size
    dec = _decoder(sd, args)
    _, batch = _batch(ora, 32, seeds)
    batch = batch.to(DEV)
    whole = dec.beam_search_batch(batch, V - 2, end_id, beam)
    rev = dec.beam_search_batch(batch.flip(1).contiguous(), V - 2, end_id, beam)[::-1]
    split = dec.beam_search_batch(batch[:, :4].contiguous(), V - 2, end_id, beam) + \
        dec.beam_search_batch(batch[:, 4:].contiguous(), V - 2, end_id, beam)
    assert whole == rev and whole == split          # captions and scores (Python floats of the f32 values): bit-identical


# ------------------------------------------------------------------------------------------------ (b) validity with ties
def _replay_batch(dec, mems, start_id, end_id, beam, V, delta):
    batch = torch.cat(mems, dim=1).contiguous().to(DEV)
    results, traces = dec.beam_search_batch(batch, start_id, end_id, beam, return_trace=True)
    plain = dec.beam_search_batch(batch, start_id, end_id, beam)
    assert plain == results                         # the trace buffer changes nothing
    worst, steps = 0.0, []
    for b, m in enumerate(mems):
        sc = BR.device_scorer(dec, m.to(DEV))
        worst = max(worst, BR.replay(results[b], traces[b], sc, start_id, end_id, beam, V, delta))
        steps.append(len(traces[b]))
        best, seqs, scores = results[b]
        assert len(seqs) == len(scores) <= beam and (best is None) == (not seqs)
        for s in seqs:
            assert s[0] == start_id and s[-1] == end_id and end_id not in s[1:-1] and len(s) <= 52
        assert best is None or best in seqs
    return worst, steps, results


def test_every_decision_is_valid_on_the_committed_cases():
    _need_gpu()
    from oracle import caption as oc
    for seed, beam, es, end_id in oc.BEAM_CASES:
        args, ora, sd, memory = oc.beam_case(seed, es)
        V = args.vocab_size
        worst, steps, _ = _replay_batch(_decoder(sd, args), [memory], V - 2, end_id, beam, V, BR.DELTA_F32)
        print(f"case {(seed, beam, es, end_id)}: {steps} steps, max |score - per-pair kernels| {worst:.3e}")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_every_decision_is_valid_on_twelve_tied_pairs(dtype):
    """beam_case(6, 10.0), data seeds 1..12, <end> = 63, beam 4: exact ties in every pair on the CPU, eleven run to step 51,
    completions at lengths 2..36 on the way, seven pairs without a caption."""
    _need_gpu()
    from oracle import caption as oc
    args, ora, sd, _ = oc.beam_case(6, 10.0)
    V = args.vocab_size
    mems = [BR.memory_of(ora, 32, d) for d in range(1, 13)]
    delta = BR.DELTA_F32 if dtype == torch.float32 else DELTA_BF16
    worst, steps, results = _replay_batch(_decoder(sd, args, dtype), mems, V - 2, 63, 4, V, delta)
    print(f"{dtype}: steps {steps}, captions {sum(r[0] is not None for r in results)}, "
          f"max |score - per-pair kernels| {worst:.4e} (delta {delta})")
    assert max(steps) == 51


def test_every_decision_is_valid_at_the_production_memory_size():
    """beam_case(6, 10.0, size=256): S = 256 memory rows, data seeds 1..8, <end> = 84, beam 4 (all run 51 steps on the CPU)."""
    _need_gpu()
    from oracle import caption as oc
    args, ora, sd, _ = oc.beam_case(6, 10.0, size=256)
    V = args.vocab_size
    mems = [BR.memory_of(ora, 256, d) for d in range(1, 9)]
    assert mems[0].shape[0] == 256
    worst, steps, _ = _replay_batch(_decoder(sd, args), mems, V - 2, 84, 4, V, BR.DELTA_F32)
    print(f"S = 256: steps {steps}, max |score - per-pair kernels| {worst:.3e}")


# ------------------------------------------------------------------------------------------------ (c) the cache
N_OPS = 25      # kernels' worth of rounding between the tokens and the logits: 3 layers x 8 stores + the vocabulary projection


def _forced_logits(dec, memory, words, parents=None):
    """Teacher-forced decode: words [steps][beam] (the word slot j takes at step t), parents likewise (default: in place)."""
    steps, beam = words.shape
    forced = torch.zeros((1, steps, beam, 2), dtype=torch.int32)
    forced[0, :, :, 1] = words
    forced[0, :, :, 0] = torch.arange(beam)[None, :] if parents is None else parents
    forced[0, 0, :, 0] = 0                      # step 1 expands hypothesis 0 only
    _, logits = dec._beam_search_batch(memory, dec.vocab_size - 2, -1, beam, steps + 1, False, forced=forced, want_logits=True)
    return logits[0]                            # [steps][beam][V]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("V,S,beam", [(97, 4, 1), (97, 256, 5), (501, 4, 5), (501, 256, 1), (501, 256, 5)])
def test_incremental_logits_against_float64_full_window(V, S, beam, dtype):
    """Logits of the newest position from the key/value-cache path at steps 1, 2, 7, 26 and 51 against the float64
    restatement of the whole window (caption_reference.decoder_forward: no nn.MultiheadAttention in it).  Per element
    |err| <= N_OPS * u * (max|ref| + |ref|), u the per-kernel relative bound of tests/test_caption_ops_gpu.py (2e-5 in f32;
    2^-8, one bf16 ulp, in bf16): each of the N_OPS values stored between the tokens and the logits is rounded once, and a
    logit is a sum of 192 products, so its error scales with the largest logit, not with its own size."""
    _need_gpu()
    from oracle import caption as oc
    args, ora, sd, _ = oc.beam_case(6, 10.0, vocab=V)
    dec = _decoder(sd, args, dtype)
    g = torch.Generator().manual_seed(V + S + beam)
    memory = torch.randn(S, 1, 192, generator=g) * 0.5
    words = torch.randint(1, V - 2, (51, beam), generator=g)
    logits = _forced_logits(dec, memory.to(DEV), words).double().cpu()
    sd64 = {k[len("decoder."):]: v.double() for k, v in sd.items() if k.startswith("decoder.")}
    caps = torch.cat([torch.full((beam, 1), V - 2), words.t()], dim=1)           # [beam][52], <start> first
    ref = R.decoder_forward(sd64, memory.double().expand(S, beam, 192), caps[:, :51], n_head=args.n_head)   # [51][beam][V]
    u = 2e-5 if dtype == torch.float32 else 2.0 ** -8
    for step in (1, 2, 7, 26, 51):
        rows = 1 if step == 1 else beam
        a, b = logits[step - 1, :rows], ref[step - 1, :rows]
        assert torch.isfinite(a).all()
        err, lim = (a - b).abs(), N_OPS * u * (b.abs().max() + b.abs())
        print(f"V {V} S {S} beam {beam} {dtype} step {step}: max err {err.max():.3e}, worst err/lim {(err / lim).max():.3f}")
        assert (err <= lim).all(), (step, err.max().item(), (err / lim).max().item())


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_beam_reordering_gathers_the_cache_exactly(dtype):
    """The same five prefixes decoded in place and with the hypotheses permuted at every step (each slot taking another
    parent's history): the logits of a prefix do not depend on the slot it sits in, bit for bit."""
    _need_gpu()
    from oracle import caption as oc
    V, S, beam, steps = 97, 16, 5, 51
    args, ora, sd, _ = oc.beam_case(6, 10.0, vocab=V)
    dec = _decoder(sd, args, dtype)
    g = torch.Generator().manual_seed(5)
    memory = (torch.randn(S, 1, 192, generator=g) * 0.5).to(DEV)
    words = torch.randint(1, V - 2, (steps, beam), generator=g)           # words[t][h]: word t of logical hypothesis h
    plain = _forced_logits(dec, memory, words)
    holds = torch.arange(beam)                                            # logical hypothesis each slot holds before a step
    perm_words, parents, held = torch.zeros_like(words), torch.zeros_like(words), []
    for t in range(steps):
        new = torch.randperm(beam, generator=g)                           # slot j will hold logical hypothesis new[j]
        for j in range(beam):
            parents[t, j] = 0 if t == 0 else int((holds == new[j]).nonzero()[0])
            perm_words[t, j] = words[t, new[j]]
        held.append(holds.clone())
        holds = new
    moved = _forced_logits(dec, memory, perm_words, parents)
    assert torch.equal(moved[0, 0], plain[0, 0])
    for t in range(1, steps):
        assert torch.equal(moved[t], plain[t][held[t]]), t


# ------------------------------------------------------------------------------------------------ (d) script level
def test_evaluate_with_eval_batch_gives_the_loop_hypotheses():
    _need_gpu()
    from change3d_amd.model.trainer import Trainer
    from change3d_amd.scripts.train_CC import evaluate
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
    for d in seeds[:6]:
        pre, post, _ = synth.synth_batch(1, 32, seed=d)
        pairs.append((pre.to(DEV), post.to(DEV)))
    loop = evaluate(args, net, pairs, V - 2, end_id)
    batched = evaluate(args, net, pairs, V - 2, end_id, eval_batch=4)           # 4 + a ragged batch of 2
    assert len(loop) == 6 and batched == loop
    assert any(h is not None for h in loop)
    args.eval_batch = 4
    assert evaluate(args, net, pairs, V - 2, end_id) == loop


def test_refused_shape_falls_back_to_the_per_pair_search():
    _need_gpu()
    from change3d_amd import ops
    from oracle import caption as oc
    seed, _, es, end_id = oc.BEAM_CASES[4]
    args, ora, sd, _ = oc.beam_case(seed, es)
    V = args.vocab_size
    dec = _decoder(sd, args)
    mems, batch = _batch(ora, 32, (4, 5))
    assert ops.cap_beam_plan(4, 192, args.n_head, args.n_layer, V, 9, 52, 0) is None
    got = dec.beam_search_batch(batch.to(DEV), V - 2, end_id, 9)
    assert "cap_beam_kernel" not in ops.last_kernel()
    for b in range(2):
        assert got[b] == dec.beam_search(mems[b].to(DEV), V - 2, end_id, 9)
    assert any(r[0] is not None for r in got)


def test_train_cc_script_takes_eval_batch():
    _need_gpu()
    out = subprocess.run([sys.executable, "-m", "change3d_amd.scripts.train_CC", "--eval_pairs", "5", "--eval_batch", "4",
                          "--beam_size", "3", "--max_steps", "1", "--batch_size", "2", "--in_height", "64", "--in_width", "64"],
                         cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    line = [ln for ln in out.stdout.splitlines() if ln.startswith("evaluate:")]
    assert len(line) == 1 and line[0].startswith("evaluate: 5 pairs, beam 3, ") and line[0].endswith("ms/pair"), out.stdout[-500:]
