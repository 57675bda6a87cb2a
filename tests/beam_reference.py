"""Test helper for the batched beam search (`CaptionDecoder.beam_search_batch`, csrc/caption_beam.hip): a search loop with
the kernel's tie rule over any step scorer, and a replay that checks a device trace decision by decision.

With synthetic decoder weights most searches meet EXACT f32 ties between candidates (two hypotheses holding the same words in
another order score alike bit for bit), and `torch.topk` documents no order among equals, so a hand-written selection cannot be
compared with it there.  Hence: identity with `oracle.caption.beam_search` only on inputs whose every decision has a margin
(`MARGIN_ROWS`, `search(...).min_gap`), and on every other input `replay`, which accepts any selection that is a top-k up to
`delta` under a reference scorer and is otherwise exact about the bookkeeping.

A scorer is `f(seqs) -> float32 CPU tensor [len(seqs), V]`: log-softmax of the next word for each hypothesis (a list of word
lists, all of one length, `<start>` first)."""
import torch

# (weights seed, embedding scale, <end>, beam) -> data seeds: inputs on which every decision of the f32 CPU oracle has a margin
# (smallest gap inside the top k 6.8e-2 / 9.1e-3, between the k-th and the (k+1)-th candidate 2.0e-2 / 5.8e-3 / 1.2e-2)
MARGIN_ROWS = (((3, 30.0, 9, 3), (1, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12)),
               ((6, 10.0, 84, 4), (2, 4, 7)),
               ((6, 10.0, 84, 1), (7,)))
MIN_MARGIN = 5e-3
DELTA_F32 = 2e-3          # the bound tests/test_cc_gpu.py uses for device scores against the oracle's


def memory_of(ora, size, data_seed):
    """Encoder memory (S, 1, D) of the oracle trainer `ora` on the synthetic pair `data_seed` (as oracle.caption.beam_case)."""
    from oracle import synth
    pre, post, _ = synth.synth_batch(1, size, seed=data_seed)
    with torch.no_grad():
        feat = ora.update_cc(pre, post)
    B, C, H, W = feat.shape
    return feat.permute(2, 3, 0, 1).reshape(H * W, B, C)


def oracle_scorer(decoder, memory, max_len=52):
    """Scorer over `oracle.caption.decoder_step_scores` (the reference's own 52-token window): CPU, f32."""
    from oracle import caption as oc

    def f(seqs):
        s, n = len(seqs), len(seqs[0])
        words = torch.zeros(s, max_len, dtype=torch.int64)
        words[:, :n] = torch.tensor(seqs, dtype=torch.int64)
        enc = memory.expand(memory.shape[0], s, memory.shape[2]).permute(1, 0, 2)
        with torch.no_grad():
            sc = oc.decoder_step_scores(decoder, words, enc)
        return torch.log_softmax(sc[:, n - 1, :], dim=1)
    return f


def device_scorer(dec, memory):
    """Scorer over the per-pair path of `CaptionDecoder.beam_search` (embedding, `_infer_layers` over the whole prefix, the
    vocabulary projection of the last position; no key/value cache): the kernels the batched search is checked against.
    memory (S, 1, D) on the device."""
    from change3d_amd import ops
    from change3d_amd.model.caption_decoder import _infer_layers, project_memory
    S, _, D = memory.shape
    act, dev, V = dec.act_dtype, memory.device, dec.vocab_size
    dt = ops.dt_code(act)
    kv1 = project_memory(dec.transformer, memory)
    pe = dec.position_encoding.pe.view(-1, D)

    def f(seqs):
        s, n = len(seqs), len(seqs[0])
        tok = torch.tensor(seqs, dtype=torch.int64, device=dev)
        kv = [t.view(S, 1, 2 * D).expand(S, s, 2 * D).contiguous().view(S * s, 2 * D) for t in kv1]
        with torch.no_grad():
            x = torch.empty((n * s, D), dtype=act, device=dev)
            ops.cap_embed_fwd(tok, dec.vocab_embedding.weight, pe, x, s, n, D, V, 0.0, 0, dt)
            h = _infer_layers(dec.transformer, x, kv, S, s, n, causal=True)
            logits = torch.empty((s, ops.cpad(V)), dtype=act, device=dev)
            ops.linear_fwd(h[(n - 1) * s:], dec.wdc.weight, dec.wdc.bias, logits, s, D, V, dt)
            return torch.log_softmax(logits[:, :V].float(), dim=1).cpu()
    return f


class Search:
    """What `search` returns: result = (best or None, complete_seqs, complete_scores); trace = per step (live before the step,
    [(parent, word, score)] in rank order); runner_up = per step the (k+1)-th candidate (parent, word, score) or None;
    min_gap = (smallest gap inside the top k, smallest gap between the k-th and the (k+1)-th) over all steps."""

    def __init__(self, result, trace, runner_up, min_gap):
        self.result, self.trace, self.runner_up, self.min_gap = result, trace, runner_up, min_gap


def _finish(complete_seqs, complete_scores):
    if not complete_scores:
        return None, complete_seqs, complete_scores
    return complete_seqs[complete_scores.index(max(complete_scores))], complete_seqs, complete_scores


def search(scorer, start_id, end_id, beam, V, max_len=52):
    """The reference's beam search (oracle/caption.py::beam_search, scripts/train_CC.py:214-330) over `scorer`, with equal
    candidate scores ordered by the lower flat index parent * V + word (a stable descending sort)."""
    k = beam
    seqs = [[start_id] for _ in range(k)]
    run = torch.zeros(k, dtype=torch.float32)
    complete_seqs, complete_scores, trace, runner_up = [], [], [], []
    gap_in, gap_out = float("inf"), float("inf")
    step = 1
    while True:
        rows = seqs[:1] if step == 1 else seqs
        cand = (run[:len(rows), None] + scorer(rows)).reshape(-1)
        val, idx = torch.sort(cand, descending=True, stable=True)
        top_v, top_i = val[:k].tolist(), idx[:k].tolist()
        for a, b in zip(top_v, top_v[1:]):
            gap_in = min(gap_in, a - b)
        if len(val) > k:
            gap_out = min(gap_out, top_v[-1] - val[k].item())
            runner_up.append((idx[k].item() // V, idx[k].item() % V, val[k].item()))
        else:
            runner_up.append(None)
        sel = [(i // V, i % V, v) for i, v in zip(top_i, top_v)]
        trace.append((k, sel))
        nxt, nrun = [], []
        for p, w, v in sel:
            s = seqs[p] + [w]
            if w == end_id:
                complete_seqs.append(s)
                complete_scores.append(v)
            else:
                nxt.append(s)
                nrun.append(v)
        k = len(nxt)
        if k == 0:
            break
        seqs, run = nxt, torch.tensor(nrun, dtype=torch.float32)
        if step > max_len - 2:
            break
        step += 1
    return Search(_finish(complete_seqs, complete_scores), trace, runner_up, (gap_in, gap_out))


def replay(result, trace, scorer, start_id, end_id, beam, V, delta, max_len=52):
    """Walk a search trace step by step against `scorer` and raise AssertionError at the first decision that is not valid:
    the selection must be a top-k of the reference candidates up to `delta`, the reported scores within `delta` of the
    reference's (which adds the running scores the trace itself reported one step earlier, so nothing drifts), ranks in
    non-increasing reported score with equal scores in increasing flat index, and live counts, parents, completion records,
    the winner (first maximum) and the no-caption case exactly what the trace implies.  Returns the largest
    |reported - reference| score difference met."""
    k = beam
    seqs = [[start_id] for _ in range(k)]
    run = torch.zeros(k, dtype=torch.float32)
    complete_seqs, complete_scores = [], []
    worst = 0.0
    step, ended = 1, False
    for live, sel in trace:
        assert not ended, f"step {step}: the trace goes on after the search has ended"
        assert live == k, f"step {step}: live count {live}, the trace so far implies {k}"
        assert len(sel) == k, f"step {step}: {len(sel)} candidates selected for {k} live hypotheses"
        rows = seqs[:1] if step == 1 else seqs
        cand = run[:len(rows), None] + scorer(rows)
        flat = []
        for p, w, _ in sel:
            assert 0 <= p < len(rows) and 0 <= w < V, f"step {step}: candidate ({p}, {w}) outside {len(rows)} x {V}"
            flat.append(p * V + w)
        assert len(set(flat)) == k, f"step {step}: a candidate selected twice: {sel}"
        ref = [cand[p, w].item() for p, w, _ in sel]
        kth = torch.topk(cand.reshape(-1), k).values[-1].item()
        rest = cand.clone().reshape(-1)
        rest[torch.tensor(flat)] = float("-inf")
        for (p, w, v), r in zip(sel, ref):
            assert r >= kth - delta, f"step {step}: ({p}, {w}) scores {r}, the reference's k-th best is {kth}"
            assert abs(v - r) <= delta, f"step {step}: ({p}, {w}) reported {v}, reference {r}"
            worst = max(worst, abs(v - r))
        if rest.numel() > k:
            assert rest.max().item() <= min(ref) + delta, \
                f"step {step}: an unselected candidate scores {rest.max().item()}, above the weakest selected {min(ref)}"
        vals = [v for _, _, v in sel]
        for i in range(k - 1):
            assert vals[i] > vals[i + 1] or (vals[i] == vals[i + 1] and flat[i] < flat[i + 1]), f"step {step}: ranks out of order: {sel}"
        nxt, nrun = [], []
        for p, w, v in sel:
            s = seqs[p] + [w]
            if w == end_id:
                complete_seqs.append(s)
                complete_scores.append(v)
            else:
                nxt.append(s)
                nrun.append(v)
        k = len(nxt)
        seqs, run = nxt, torch.tensor(nrun, dtype=torch.float32)
        if k == 0 or step > max_len - 2:
            ended = True
        step += 1
    assert ended, f"the trace stops after step {step - 1} with {k} hypotheses alive"
    want = _finish(complete_seqs, complete_scores)
    assert result[1] == want[1], f"completed sequences {result[1]}, the trace implies {want[1]}"
    assert list(result[2]) == want[2], f"completed scores {result[2]}, the trace implies {want[2]}"
    assert result[0] == want[0], f"winner {result[0]}, the trace implies {want[0]}"
    return worst
