"""Batched beam search, the parts that need no GPU: the kernel's limits query (c3d_cap_beam_plan) and the trace checker of
tests/beam_reference.py with its negative controls -- a checker that accepts everything would make the GPU tests of
tests/test_beam_batch_gpu.py worthless."""
import copy
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import beam_reference as BR  # noqa: E402

DT_F32, DT_BF16 = 0, 1


def test_plan_takes_the_required_shapes_and_refuses_the_rest():
    """The shapes the captioning evaluation meets are taken (V = 501 reference word map, V = 97 fixtures, S = 4 .. 400, beam
    1 .. 5, f32 and bf16), within the CU's 160 KB of LDS; what the LDS plan or the lane mapping cannot hold is refused before
    anything could be launched (host only: no device is touched)."""
    from change3d_amd import _lib, ops
    for dt in (DT_F32, DT_BF16):
        for V in (97, 501):
            for S in (4, 16, 64, 256, 400):
                for beam in (1, 2, 3, 4, 5):
                    p = ops.cap_beam_plan(S, 192, 8, 3, V, beam, 52, dt, B=64)
                    assert p is not None, (dt, V, S, beam)
                    ws, lds = p
                    assert 0 < lds <= 160 * 1024 and lds % 16 == 0
                    assert ws == 64 * 3 * 52 * beam * 2 * 192 * (4 if dt == DT_F32 else 2)
    assert ops.cap_beam_plan(256, 192, 8, 3, 501, 8, 52, DT_F32) is not None
    assert ops.cap_beam_plan(256, 192, 8, 3, 501, 9, 52, DT_F32) is None          # beam > 8
    assert ops.cap_beam_plan(256, 196, 4, 3, 501, 3, 52, DT_F32) is None          # embed_dim not a multiple of 8
    assert ops.cap_beam_plan(256, 264, 11, 3, 501, 3, 52, DT_F32) is None         # embed_dim > 256
    assert ops.cap_beam_plan(256, 192, 4, 3, 501, 3, 52, DT_F32) is None          # head width 48 > 32
    assert ops.cap_beam_plan(256, 192, 8, 3, 501, 3, 65, DT_F32) is None          # max_len beyond the 64 lanes over positions
    assert ops.cap_beam_plan(256, 192, 8, 9, 501, 3, 52, DT_F32) is None          # more layers than the argument block holds
    assert ops.cap_beam_plan(6000, 192, 8, 3, 501, 3, 52, DT_F32) is None         # one probability row per wave: LDS
    assert ops.cap_beam_plan(256, 192, 8, 3, 5000, 8, 52, DT_F32) is None         # k x V f32 logits: LDS
    with pytest.raises(_lib.Change3DHipError):
        ops.cap_beam_plan(0, 192, 8, 3, 501, 3, 52, DT_F32)                       # C3D_E_BADARG is an error, not a refusal
    assert _lib.lib().c3d_cap_beam_search(None, None) == -1


def test_beam_search_batch_refuses_cpu_tensors():
    import contextlib
    import io
    from change3d_amd import _lib
    from change3d_amd.model.caption_decoder import CaptionDecoder
    from oracle import synth
    with contextlib.redirect_stdout(io.StringIO()):
        dec = CaptionDecoder(synth.make_cc_args(size=32, vocab_size=97, dropout=0.0))
    assert dec.training
    with pytest.raises(_lib.Change3DHipError):
        dec.beam_search_batch(torch.zeros(4, 2, 192), 95, 9, 3)
    assert dec.training                                                           # the training flag is restored


def _case(row, data_seed):
    from oracle import caption as oc
    (seed, es, end_id, beam), _ = row
    args, ora, sd, _ = oc.beam_case(seed, es)
    memory = BR.memory_of(ora, 32, data_seed)
    return args.vocab_size, ora, memory, end_id, beam


@pytest.mark.parametrize("row", range(len(BR.MARGIN_ROWS)))
def test_helper_search_equals_the_oracle_on_the_margin_inputs(row):
    """On inputs whose every decision has a margin the helper's search loop (lower-index tie rule) and
    oracle.caption.beam_search (torch.topk) must agree exactly; the margins are recomputed here and an input below
    MIN_MARGIN FAILS (no case may be dropped); the trace the helper produced passes its own replay."""
    from oracle import caption as oc
    spec, seeds = BR.MARGIN_ROWS[row]
    for d in seeds:
        V, ora, memory, end_id, beam = _case(BR.MARGIN_ROWS[row], d)
        sc = BR.oracle_scorer(ora.decoder, memory)
        got = BR.search(sc, V - 2, end_id, beam, V)
        want = oc.beam_search(ora.decoder, memory, V - 2, end_id, beam, V)
        print(f"weights {spec} data {d}: steps {len(got.trace)} gaps {got.min_gap}")
        assert min(got.min_gap) >= BR.MIN_MARGIN, (spec, d, got.min_gap)
        assert got.result[0] == want[0] and got.result[1] == want[1], (spec, d)
        assert got.result[2] == want[2], (spec, d)
        BR.replay(got.result, got.trace, sc, V - 2, end_id, beam, V, BR.DELTA_F32)


def test_replay_rejects_wrong_traces():
    """Negative controls of the checker on a CPU trace (weights seed 6, data seed 4, beam 4: 22 steps, completions on the
    way): the true trace passes, and each of four wrong ones is rejected."""
    V, ora, memory, end_id, beam = _case(BR.MARGIN_ROWS[1], 4)
    sc = BR.oracle_scorer(ora.decoder, memory)
    s = BR.search(sc, V - 2, end_id, beam, V)
    delta = BR.DELTA_F32
    check = lambda res, tr: BR.replay(res, tr, sc, V - 2, end_id, beam, V, delta)  # noqa: E731
    assert check(s.result, s.trace) == 0.0
    assert len(s.result[1]) >= 1 and len(s.trace) >= 3

    # (1) a selected word replaced by the (k+1)-th candidate, at a step where that candidate is more than delta behind
    t = next(i for i, (ru, (live, sel)) in enumerate(zip(s.runner_up, s.trace))
             if i >= 1 and ru is not None and sel[-1][2] - ru[2] > 2 * delta)
    tr = copy.deepcopy(s.trace)
    tr[t][1][-1] = s.runner_up[t]
    with pytest.raises(AssertionError, match="k-th best"):
        check(s.result, tr)

    # (2) two ranks of different score swapped
    t = next(i for i, (live, sel) in enumerate(s.trace) if live >= 2 and sel[0][2] != sel[1][2])
    tr = copy.deepcopy(s.trace)
    tr[t][1][0], tr[t][1][1] = tr[t][1][1], tr[t][1][0]
    with pytest.raises(AssertionError, match="ranks out of order"):
        check(s.result, tr)

    # (3) a parent index changed (step >= 2: at step 1 every parent is hypothesis 0)
    t = next(i for i, (live, sel) in enumerate(s.trace) if i >= 1 and live >= 2)
    tr = copy.deepcopy(s.trace)
    p, w, v = tr[t][1][0]
    tr[t][1][0] = ((p + 1) % tr[t][0], w, v)
    with pytest.raises(AssertionError):
        check(s.result, tr)

    # (4) a completion dropped from the results
    res = (s.result[0], s.result[1][1:], s.result[2][1:])
    with pytest.raises(AssertionError, match="completed"):
        check(res, s.trace)

    # and: a live count that does not follow from the steps before, a trace cut short
    tr = copy.deepcopy(s.trace)
    tr[-1] = (tr[-1][0] + 1, tr[-1][1])
    with pytest.raises(AssertionError, match="live count"):
        check(s.result, tr)
    if len(s.trace) < 51 and s.trace[-1][0] > sum(w == end_id for _, w, _ in s.trace[-1][1]):
        pytest.fail("the control search must end by emptying its beam")
    with pytest.raises(AssertionError, match="trace stops"):
        check(s.result, s.trace[:-1])
