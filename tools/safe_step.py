"""c3d_outlines_simplify_safe on the MI355X at 1024 x 1024, 8-connectivity, tolerances 1 and 2 px, on the tables of
tools/shared_step.py (blobs, blobs split at R = 3, random at density 0.59, all foreground, serpentine).  Per table and tolerance:
time per call next to c3d_outlines_simplify_shared on the same table in the same run (device events around repeated calls after a
warm-up, median over several rounds, buffers allocated once) -- the shared call is the yardstick, never the new call against
itself --, rounds run and rounds that raised, arcs refined, vertices of both, defective pairs in round 0 and in the last round,
and the cost of a round that returns at once (the call with 8 rounds more, over those 8).  Then the alternative on the host: the
download of the labels and the rings plus the restatement (tests/safe_reference.py: its simplify step timed on the first rings
that hold up to SAMPLE vertices and scaled to all of them and to the rounds run; its all-pairs search timed on the first EDGES
output edges, which grows with the square of their number and is not scaled).  Then the time per kernel of one call on the split
blobs from torch's profiler.  Writes stdout (`python tools/safe_step.py > profiles/outlines_safe.txt`)."""
import os
import re
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import safe_reference as SR  # noqa: E402
import shared_reference as R  # noqa: E402
from change3d_amd import _lib as L  # noqa: E402
from change3d_amd import ops  # noqa: E402
from objects_step import ROUNDS, S, event_us, masks  # noqa: E402

TOLERANCES = (1.0, 2.0)
SPLIT_R = 3
MAX_ROUNDS = 8
SAMPLE = 20000                                            # raw vertices the restatement's simplify step is timed on
EDGES = 3000                                              # output edges its all-pairs search is timed on


def main():
    if not torch.cuda.is_available():
        raise SystemExit("tools/safe_step.py measures on the GPU; there is none here")
    dev = torch.device("cuda:0")
    max_objects = S * S // 2 + 1
    max_rings, max_vertices = S * S // 2 + 1, 2 * S * S + 4  # nothing is cut off on any of the masks
    nbytes = L.lib().c3d_outlines_simplify_safe_ws_bytes(S, S, max_rings, max_vertices, 2 * max_vertices)
    limits = ops.outlines_simplify_safe_limits()
    print(f"# tools/safe_step.py: {S} x {S}, 8-connectivity, max_rounds = {MAX_ROUNDS}; limits {limits}; workspace {nbytes / 2**20:.1f} MiB; "
          f"device events, {ROUNDS} rounds of 10 calls (serpentine: 2), median (min .. max); {os.path.basename(L.LIB_PATH)}", flush=True)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    ws_s = torch.empty(L.lib().c3d_outlines_simplify_shared_ws_bytes(S, S, max_rings, max_vertices), dtype=torch.uint8, device=dev)
    named = masks()
    cases = [(named[0][0], named[0][1], None), (f"blobs split {SPLIT_R}", named[0][1], SPLIT_R)] + [(n, m, None) for n, m in named[1:]]
    profiled = None
    for name, mask_np, split in cases:
        mask = torch.from_numpy(mask_np).to(dev)
        if split is None:
            labels, _, _, _, counts_obj = ops.scene_objects(mask, connectivity=8, max_objects=max_objects, want_object_cls=False)
        else:
            labels, _, _, _, counts_obj, _ = ops.scene_split(mask, split, connectivity=8, max_objects=max_objects)
        raw = ops.scene_outlines(labels, counts_obj, connectivity=8, max_objects=max_objects, max_rings=max_rings, max_vertices=max_vertices)
        print(f"{name}: {int(counts_obj[1])} objects, {int(raw[2][1])} rings, {int(raw[2][3])} raw vertices", flush=True)
        slow = name == "serpentine"
        reps, warm = (2, 1) if slow else (10, 2)
        for tol in TOLERANCES:
            shared_call = lambda: ops.outlines_simplify_shared(labels, counts_obj, *raw, tol, max_objects=max_objects, ws=ws_s)  # noqa: E731
            safe_call = lambda r=MAX_ROUNDS: ops.outlines_simplify_safe(labels, counts_obj, *raw, tol, max_rounds=r, max_objects=max_objects,  # noqa: E731
                                                                        ws=ws)
            shared, safe = shared_call(), safe_call()
            torch.cuda.synchronize()
            t_shared, t_safe = event_us(shared_call, reps=reps, warm=warm), event_us(safe_call, reps=reps, warm=warm)
            t_more = event_us(lambda: safe_call(MAX_ROUNDS + 8), reps=reps, warm=warm)
            s, info = safe[6].tolist(), safe[4].tolist()
            print(f"  tol {tol:g}: shared {t_shared[0]:9.1f} us ({t_shared[1]:.1f} .. {t_shared[2]:.1f});  safe {t_safe[0]:9.1f} us "
                  f"({t_safe[1]:.1f} .. {t_safe[2]:.1f}) = {t_safe[0] / t_shared[0]:.2f} of it;  rounds {s[0]}, raised {s[1]}, status {s[7]}; arcs "
                  f"refined {s[2]} of {info[2]} ring arcs, raw {s[3]}; vertices {int(shared[2][3])} -> {int(safe[2][3])}; defective pairs "
                  f"{s[4]} -> {s[5]}, defective rings in round 0 {s[6]}; grid shift {info[6]}, work {info[7]}; a round that returns at once "
                  f"{(t_more[0] - t_safe[0]) / 8:.1f} us", flush=True)
            if split is not None and tol == TOLERANCES[-1]:
                profiled = (name, safe_call)
            if tol != TOLERANCES[0]:
                continue
            t = []
            for _ in range(3):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                host = [x.cpu().numpy() for x in (labels, counts_obj, raw[0][:int(raw[2][1])], raw[1][:int(raw[2][3])])]
                t.append((time.perf_counter() - t0) * 1e6)
            lab = R.Labels(host[0], host[1], max_objects)
            q = R.tol2_q(tol)
            take = seen = 0
            t0 = time.perf_counter()
            for _, start, nv, *_ in host[2].tolist():
                if seen >= SAMPLE:
                    break
                aug = R.rotate(R.augment([tuple(p) for p in host[3][start:start + nv].tolist()], lab))
                R.simplify_ring(aug, q)
                seen += nv
                take += 1
            py = (time.perf_counter() - t0) * 1e6
            scale = int(raw[2][3]) / seen if seen else 0.0
            out = dict(rings=safe[0].cpu().numpy(), vertices=safe[1].cpu().numpy())
            out["slots"] = {}
            used = 0
            for r, row in enumerate(out["rings"][:int(raw[2][1])].tolist()):
                if row[1] >= 0 and used + row[2] <= EDGES:
                    out["slots"][r] = [0] * row[2]
                    used += row[2]
            edges = SR.edges_of(out)
            t0 = time.perf_counter()
            SR.detect_numpy(edges)
            pairs = (time.perf_counter() - t0) * 1e3
            print(f"  on the host : download of labels and rings {np.median(t):9.1f} us + simplify step {py * scale / 1e3:10.1f} ms per round "
                  f"({py / 1e3:.1f} ms for the first {take} rings, {seen} raw vertices, scaled by {scale:.1f}), times {s[0]} rounds; all pairs "
                  f"of the first {len(edges)} of {int(safe[2][3])} output edges {pairs:.1f} ms", flush=True)

    try:                                                     # the time per kernel of one call
        from torch.profiler import ProfilerActivity, profile
        name, call = profiled
        n = 5
        call()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(n):
                call()
            torch.cuda.synchronize()
        rows = [(e.key, e.count, getattr(e, "device_time_total", None) or getattr(e, "cuda_time_total", 0.0)) for e in prof.key_averages()
                if "safe_" in e.key or "Memset (" in e.key]
        print(f"per kernel, {name}, tol {TOLERANCES[-1]:g}, {n} calls of {MAX_ROUNDS} rounds (torch profiler; launches of the rounds after "
              f"the last one return at once and are in the averages):")
        for key, count, total in sorted(rows, key=lambda r: -r[2]):
            found = re.search(r"safe_\w+(<\d+)?", key)
            print(f"  {found.group(0) if found else key[:40]:32s} {count:5d} launches {total / max(count, 1):9.1f} us each {total / n:10.1f} us per call")
    except Exception as e:                                   # the profiler is a convenience: the totals above stand without it
        print(f"per kernel: torch's profiler is not available here ({type(e).__name__}: {e})")


if __name__ == "__main__":
    main()
