"""c3d_outlines_simplify_shared on the MI355X at 1024 x 1024, tolerance 1.0 px, on the rings that c3d_scene_outlines traces from
the masks of tools/objects_step.py (blobs, random at density 0.59, all foreground, serpentine) and from the blobs split at R = 3,
whose pieces share walls.  Per table: time per call next to c3d_outlines_simplify on the same table (device events around
repeated calls after a warm-up, median over several rounds, buffers allocated once), vertices in and out of both, what the
shared call counted, the c3d_rings_conflicts counts of the plain and of the shared result, and the alternative on the host: the
download of the labels and the rings plus the restatement of the rule (tests/shared_reference.py), timed on the first rings that
hold up to SAMPLE vertices and scaled to all of them.  Then the time per kernel of one call from torch's profiler.  Writes
stdout (`python tools/shared_step.py > profiles/outlines_shared.txt`)."""
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

import shared_reference as R  # noqa: E402
from change3d_amd import _lib as L  # noqa: E402
from change3d_amd import ops  # noqa: E402
from objects_step import ROUNDS, S, event_us, masks  # noqa: E402

TOL = 1.0
SPLIT_R = 3
SAMPLE = 20000                                            # augmented vertices the restatement is timed on


def main():
    if not torch.cuda.is_available():
        raise SystemExit("tools/shared_step.py measures on the GPU; there is none here")
    dev = torch.device("cuda:0")
    max_objects = S * S // 2 + 1
    max_rings, max_vertices = S * S // 2 + 1, 2 * S * S + 4  # nothing is cut off on any of the masks
    nbytes = L.lib().c3d_outlines_simplify_shared_ws_bytes(S, S, max_rings, max_vertices)
    wave, lds = ops.outlines_simplify_shared_limits()
    print(f"# tools/shared_step.py: {S} x {S}, 8-connectivity, tol = {TOL} px; tiers: one wave up to {wave} augmented vertices, LDS up to "
          f"{lds}; workspace {nbytes / 2**20:.1f} MiB; device events, {ROUNDS} rounds of 20 calls (serpentine: 3), median (min .. max); "
          f"{os.path.basename(L.LIB_PATH)}", flush=True)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    ws_s = torch.empty(L.lib().c3d_outlines_simplify_ws_bytes(max_rings, max_vertices), dtype=torch.uint8, device=dev)
    ws_c = torch.empty(L.lib().c3d_rings_conflicts_ws_bytes(max_rings, 2 * max_vertices, max_objects), dtype=torch.uint8, device=dev)
    profiled = {}
    cases = [(name, mask, None) for name, mask in masks()]
    cases.append((f"blobs split {SPLIT_R}", cases[0][1], SPLIT_R))
    for name, mask_np, split in cases:
        mask = torch.from_numpy(mask_np).to(dev)
        if split is None:
            labels, _, _, _, counts_obj = ops.scene_objects(mask, connectivity=8, max_objects=max_objects, want_object_cls=False)
        else:
            labels, _, _, _, counts_obj, _ = ops.scene_split(mask, split, connectivity=8, max_objects=max_objects)
        raw = ops.scene_outlines(labels, counts_obj, connectivity=8, max_objects=max_objects, max_rings=max_rings, max_vertices=max_vertices)
        plain_call = lambda: ops.outlines_simplify(*raw, TOL, ws=ws_s)  # noqa: E731
        shared_call = lambda: ops.outlines_simplify_shared(labels, counts_obj, *raw, TOL, max_objects=max_objects, ws=ws)  # noqa: E731
        plain, shared = plain_call(), shared_call()
        torch.cuda.synchronize()
        slow = name == "serpentine"
        reps, warm = (3, 1) if slow else (20, 3)
        t_plain, t_shared = event_us(plain_call, reps=reps, warm=warm), event_us(shared_call, reps=reps, warm=warm)
        info = shared[4].tolist()
        print(f"{name:14s}: {int(counts_obj[1])} objects, {int(raw[2][1])} rings, {int(raw[2][3])} raw vertices; plain keeps {int(plain[2][3])}, "
              f"shared keeps {int(shared[2][3])} (status {int(shared[2][4])}); nodes inserted {info[0]}, node vertices {info[1]}, arcs {info[2]}, "
              f"closed {info[3]}, with a neighbour {info[4]}, collapsed rings {info[5]}", flush=True)
        print(f"  {'':12s}  shared {t_shared[0]:9.1f} us ({t_shared[1]:.1f} .. {t_shared[2]:.1f});  c3d_outlines_simplify {t_plain[0]:9.1f} us "
              f"({t_plain[1]:.1f} .. {t_plain[2]:.1f}): the shared call costs {t_shared[0] / t_plain[0]:.2f} of it", flush=True)
        for stage, table in (("plain", plain), ("shared", shared[:3])):
            _, c, i = ops.rings_conflicts(*table, 0, max_objects, ws=ws_c)
            c, i = c.tolist(), i.tolist()
            print(f"  {'':12s}  rings_conflicts on the {stage:6s} result: checked {c[0]}, in conflict {c[1]}, crossings {c[5]}, same {c[6]}, "
                  f"opposite {i[6]}, status {c[7]}", flush=True)
        t = []
        for _ in range(5):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            host = [x.cpu().numpy() for x in (labels, counts_obj, raw[0][:int(raw[2][1])], raw[1][:int(raw[2][3])])]
            t.append((time.perf_counter() - t0) * 1e6)
        lab = R.Labels(host[0], host[1], max_objects)
        q = R.tol2_q(TOL)
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
        print(f"  {'':12s}  on the host: download of labels and rings {np.median(t):9.1f} us + restatement {py * scale / 1e3:10.1f} ms "
              f"({py / 1e3:.1f} ms for the first {take} rings, {seen} raw vertices, scaled by {scale:.1f})", flush=True)
        profiled[name] = lambda a=(labels, counts_obj, *raw): ops.outlines_simplify_shared(*a, TOL, max_objects=max_objects, ws=ws)  # noqa: E731

    try:                                                     # the time per kernel of one call
        from torch.profiler import ProfilerActivity, profile
        for name, call in profiled.items():
            n = 2 if name == "serpentine" else 10
            call()
            torch.cuda.synchronize()
            with profile(activities=[ProfilerActivity.CUDA]) as prof:
                for _ in range(n):
                    call()
                torch.cuda.synchronize()
            rows = [(e.key, e.count, getattr(e, "device_time_total", None) or getattr(e, "cuda_time_total", 0.0)) for e in prof.key_averages()
                    if "shared_" in e.key or "Memset (" in e.key]
            print(f"per kernel, {name}, {n} calls (torch profiler):")
            for key, count, total in sorted(rows, key=lambda r: -r[2]):
                found = re.search(r"shared_\w+(<\d+)?", key)
                print(f"  {found.group(0) if found else key[:40]:32s} {count:4d} launches {total / max(count, 1):9.1f} us each")
    except Exception as e:                                   # the profiler is a convenience: the totals above stand without it
        print(f"per kernel: torch's profiler is not available here ({type(e).__name__}: {e})")


if __name__ == "__main__":
    main()
