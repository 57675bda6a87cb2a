"""c3d_rings_conflicts on the MI355X at 1024 x 1024, 8-connectivity, on the masks of tools/valid_step.py plus the blobs split at
R = 3: the traced rings, raw and simplified at 1 px.  Timed with device events around repeated calls after a warm-up, median
over several rounds, in one process, next to c3d_rings_valid and c3d_outlines_simplify on the same table.  Per table: the grid the
device chose (shift, cells, entries, work) next to the number of all edge pairs of different ids, which is what the grid stands
in for; and the host way: the download of the table plus the rule of include/change3d_hip.h in numpy, all pairs behind a
bounding-box prefilter, a block of rows at a time (timed once; tables above HOST_EDGES live edges are left to the device).
Then the time per kernel of one call from torch's profiler.  Writes stdout (`python tools/conflicts_step.py >
profiles/rings_conflicts.txt`)."""
import os
import re
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from change3d_amd import _lib as L  # noqa: E402
from change3d_amd import ops  # noqa: E402
from objects_step import ROUNDS, S, event_us, masks  # noqa: E402

TOL = 1.0
SPLIT_R = 3
HOST_BLOCK = 1 << 24                                         # box tests per numpy block of the host way
HOST_EDGES = 30000                                           # the host way stops at tables of this many live edges


def host_way(table):
    """Download, then (cross, same, opposite, touches) with every pair once, on the host: (seconds, the four sums) or None."""
    t0 = time.perf_counter()
    rings, vertices, counts = (t.cpu().numpy() for t in table)
    ids, a, b = [], [], []
    for i, start, n in rings[:int(counts[1]), :3].tolist():
        if start >= 0 and n >= 3:
            v = vertices[start:start + n].astype(np.int64)
            ids.append(np.full(n, i, np.int64)), a.append(v), b.append(np.roll(v, -1, axis=0))
    if not ids:
        return time.perf_counter() - t0, (0, 0, 0, 0)
    ids, a, b = np.concatenate(ids), np.concatenate(a), np.concatenate(b)
    live = (a != b).any(axis=1)
    ids, a, b = ids[live], a[live], b[live]
    m = len(ids)
    if m > HOST_EDGES:
        return None
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    got = np.zeros(4, dtype=np.int64)
    step = max(1, HOST_BLOCK // m)
    for i0 in range(0, m, step):
        i1 = min(i0 + step, m)
        near = ((lo[i0:i1, None, :] <= hi[None, :, :]) & (lo[None, :, :] <= hi[i0:i1, None, :])).all(-1)
        near &= (ids[i0:i1, None] != ids[None, :]) & (np.arange(i0, i1)[:, None] < np.arange(m)[None, :])
        p, q = np.nonzero(near)
        p += i0
        A, B, C, D = a[p], b[p], a[q], b[q]
        E, F = B - A, D - C
        cr = lambda u, v: np.sign(u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0])  # noqa: E731
        o1, o2, o3, o4 = cr(E, C - A), cr(E, D - A), cr(F, A - C), cr(F, B - C)
        cross = (o1 * o2 < 0) & (o3 * o4 < 0)
        flat = (o1 == 0) & (o2 == 0) & (o3 == 0) & (o4 == 0)
        tc, td, L2 = ((C - A) * E).sum(1), ((D - A) * E).sum(1), (E * E).sum(1)
        t_lo, t_hi = np.maximum(np.minimum(tc, td), 0), np.minimum(np.maximum(tc, td), L2)
        over = flat & (t_lo < t_hi)
        dot = (E * F).sum(1)
        meet = ~cross & ~flat & (o1 * o2 <= 0) & (o3 * o4 <= 0)
        got += (cross.sum(), (over & (dot > 0)).sum(), (over & (dot < 0)).sum(), (flat & (t_lo == t_hi)).sum() + meet.sum())
    return time.perf_counter() - t0, tuple(int(v) for v in got)


def main():
    if not torch.cuda.is_available():
        raise SystemExit("tools/conflicts_step.py measures on the GPU; there is none here")
    dev = torch.device("cuda:0")
    max_objects = S * S // 2 + 1
    max_rings, max_vertices = S * S // 2 + 1, 2 * S * S + 4  # nothing is cut off on any of the masks
    nbytes = L.lib().c3d_rings_conflicts_ws_bytes(max_rings, max_vertices, max_objects)
    limits = ops.rings_conflicts_limits()
    print(f"# tools/conflicts_step.py: {S} x {S}, 8-connectivity, max_work 2^32; workspace {nbytes / 2**20:.1f} MiB; limits (wave, chunk, "
          f"tile, rings, entries per vertex, cells per vertex) {limits}; device events, {ROUNDS} rounds of 20 calls, median (min .. max); "
          f"host way up to {HOST_EDGES} live edges; {os.path.basename(L.LIB_PATH)}")
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    ws_v = torch.empty(L.lib().c3d_rings_valid_ws_bytes(max_rings, max_vertices, max_objects), dtype=torch.uint8, device=dev)
    ws_s = torch.empty(L.lib().c3d_outlines_simplify_ws_bytes(max_rings, max_vertices), dtype=torch.uint8, device=dev)
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
        simplify = lambda: ops.outlines_simplify(*raw, TOL, ws=ws_s)  # noqa: E731
        simple = simplify()
        t_sim = event_us(simplify)
        print(f"{name:14s}: density {mask_np.mean():.2f}, {int(counts_obj[1])} objects, {int(raw[2][2])} raw vertices, {int(simple[2][2])} simplified; "
              f"c3d_outlines_simplify {t_sim[0]:8.1f} us ({t_sim[1]:.1f} .. {t_sim[2]:.1f})")
        for stage, rings in (("raw", raw), ("simplified", simple)):
            call = lambda: ops.rings_conflicts(*rings, 0, max_objects, ws=ws)  # noqa: E731
            conflict, counts, info = call()
            torch.cuda.synchronize()
            c, i = counts.tolist(), info.tolist()
            m = conflict[:sum(c[:1] + c[2:5]), 2].cpu().numpy()
            all_pairs = i[0] * (i[0] - 1) // 2 - int((m * (m - 1) // 2).sum())
            t = event_us(call)
            t_val = event_us(lambda: ops.rings_valid(*rings, 0, max_objects, ws=ws_v))
            host = host_way(rings)
            print(f"  {stage:10s}: checked {c[0]}, in conflict {c[1]}, empty {c[2]}, incomplete {c[3]}, over work {c[4]}, status {c[7]}; crossings "
                  f"{c[5]} same {c[6]} opposite {i[6]} touches {i[7]}")
            print(f"  {'':10s}  {i[0]} live edges, shift {i[1]}, {i[2]} x {i[3]} cells, {i[4]} entries = {i[4] / max(i[0], 1):.2f} per edge, work "
                  f"{i[5]} candidate pairs against {all_pairs} pairs of different ids ({all_pairs / max(i[5], 1):.0f} x)")
            line = (f"  {'':10s}  rings_conflicts {t[0]:8.1f} us ({t[1]:.1f} .. {t[2]:.1f}) = {t[0] / t_sim[0]:.2f} of the simplify call, "
                    f"{t[0] / t_val[0]:.2f} of rings_valid ({t_val[0]:.1f} us);  host way ")
            if host is None:
                print(line + f"not run: more than {HOST_EDGES} live edges")
            else:
                agree = host[1] == (c[5], c[6], i[6], i[7])
                print(line + f"{host[0] * 1e6:10.1f} us (sums {'agree' if agree else 'DIFFER ' + str(host[1])}): {host[0] * 1e6 / t[0]:.1f} x the device")
            if stage == "simplified" and name in ("blobs", "random 0.59", f"blobs split {SPLIT_R}"):
                profiled[name] = lambda r=rings: ops.rings_conflicts(*r, 0, max_objects, ws=ws)  # noqa: E731

    try:                                                     # the time per kernel of one call, simplified stage
        from torch.profiler import ProfilerActivity, profile
        for name, call in profiled.items():
            for _ in range(3):
                call()
            torch.cuda.synchronize()
            with profile(activities=[ProfilerActivity.CUDA]) as prof:
                for _ in range(10):
                    call()
                torch.cuda.synchronize()
            rows = [(e.key, e.count, getattr(e, "device_time_total", None) or getattr(e, "cuda_time_total", 0.0)) for e in prof.key_averages()
                    if "conflicts_" in e.key or "Memset (" in e.key]
            print(f"per kernel, {name} simplified, 10 calls (torch profiler):")
            for key, count, total in sorted(rows, key=lambda r: -r[2]):
                found = re.search(r"conflicts_\w+", key)
                print(f"  {found.group(0) if found else key[:40]:28s} {count:4d} launches {total / max(count, 1):9.1f} us each")
    except Exception as e:                                   # the profiler is a convenience: the totals above stand without it
        print(f"per kernel: torch's profiler is not available here ({type(e).__name__}: {e})")


if __name__ == "__main__":
    main()
