"""c3d_outlines_simplify on the MI355X at 1024 x 1024, tolerance 1.0 px, on the rings that c3d_scene_outlines traces from the
four masks of tools/objects_step.py (blobs, random at density 0.59, all foreground, serpentine: one ring, the deepest
recursion), a checkerboard (the most rings), a comb (one ring of 8228 vertices with teeth of unequal
length: the workspace tier at a shallow depth) and two serpentines side by side joined along the top row (one ring of 4094
vertices, about 515 levels).  Both calls are made through the C entries on buffers allocated once, so that no allocation
and no Python op lies inside the timed span; a call of a few launches on a tiny table is still bound by their enqueue.
The call is timed with device events around repeated calls after a warm-up, median over several rounds, in one process, next to (a) the c3d_scene_outlines call it follows, on the same masks in
the same run, and (b) the alternative on the host: the download of the ring rows and the written vertices, plus the plain
Python restatement of the rule (tests/simplify_reference.py), timed on the first rings that hold up to SAMPLE vertices and
scaled to all of them.  Writes stdout (`python tools/simplify_step.py > profiles/scene_simplify.txt`)."""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import simplify_reference as R  # noqa: E402
from change3d_amd import _lib as L  # noqa: E402
from change3d_amd import ops  # noqa: E402
from objects_step import ROUNDS, S, event_us, masks  # noqa: E402

TOL = 1.0
SAMPLE = 20000                                            # vertices the Python restatement is timed on


def comb():
    rng = np.random.default_rng(4)
    m = np.zeros((S, S), np.uint8)
    m[:, 0] = 1
    for spine in range(8, S, 128):
        m[spine, :] = 1
        for x in range(2, 514, 2):
            m[spine + 1:spine + 6 + int(rng.integers(0, 56)), x] = 1
    return m


def double_serpentine():
    m = np.zeros((S, S), np.uint8)
    for x0, x1 in ((0, S // 2 - 1), (S // 2 + 1, S)):
        m[::2, x0:x1] = 1
        for k, y in enumerate(range(1, S - 1, 2)):
            m[y, x1 - 1 if k % 2 == 0 else x0] = 1
    m[0, :] = 1
    return m


def main():
    if not torch.cuda.is_available():
        raise SystemExit("tools/simplify_step.py measures on the GPU; there is none here")
    dev = torch.device("cuda:0")
    max_rings, max_vertices = S * S // 2 + 1, 2 * S * S + 4  # nothing is cut off on any of the masks
    nbytes = L.lib().c3d_outlines_simplify_ws_bytes(max_rings, max_vertices)
    wave, lds = ops.outlines_simplify_limits()
    print(f"# tools/simplify_step.py: {S} x {S}, 8-connectivity, tol = {TOL} px (tol2_q = {ops.simplify_tol2_q(TOL)}); tiers: one wave up "
          f"to {wave} vertices, LDS up to {lds}; workspace {nbytes / 2**20:.1f} MiB; device events, {ROUNDS} rounds of 20 calls (comb, serpentine x2: 3), "
          f"median (min .. max); {os.path.basename(L.LIB_PATH)}", flush=True)
    ws_o = torch.empty(L.lib().c3d_scene_outlines_ws_bytes(S, S), dtype=torch.uint8, device=dev)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    rings, rings_s = (torch.empty((max_rings, 8), dtype=torch.int32, device=dev) for _ in range(2))
    vertices, vertices_s = (torch.empty((max_vertices, 2), dtype=torch.int32, device=dev) for _ in range(2))
    counts, counts_s = (torch.empty(5, dtype=torch.int32, device=dev) for _ in range(2))
    q = ops.simplify_tol2_q(TOL)
    yy, xx = np.mgrid[0:S, 0:S]
    for name, mask_np in masks() + [("checkerboard", ((yy + xx) % 2 == 0).astype(np.uint8)), ("comb", comb()),
                                    ("serpentine x2", double_serpentine())]:
        mask = torch.from_numpy(mask_np).to(dev)
        labels, _, _, _, counts_obj = ops.scene_objects(mask, connectivity=8, want_object_cls=False)
        # both calls through the C entries on buffers made once: no allocation and no Python op inside the timed span
        stream = torch.cuda.current_stream().cuda_stream
        trace = lambda: L.check(L.lib().c3d_scene_outlines(labels.data_ptr(), counts_obj.data_ptr(), S, S, 8, 65536, max_rings,  # noqa: E731
                                                           max_vertices, rings.data_ptr(), vertices.data_ptr(), counts.data_ptr(),
                                                           ws_o.data_ptr(), stream), "c3d_scene_outlines")
        call = lambda: L.check(L.lib().c3d_outlines_simplify(rings.data_ptr(), vertices.data_ptr(), counts.data_ptr(), max_rings,  # noqa: E731
                                                             max_vertices, q, rings_s.data_ptr(), vertices_s.data_ptr(),
                                                             counts_s.data_ptr(), ws.data_ptr(), stream), "c3d_outlines_simplify")
        trace()
        call()
        torch.cuda.synchronize()
        found, rows, _, written, status = counts.tolist()
        kept, status_s = int(counts_s[2]), int(counts_s[4])
        n = rings[:rows, 2]
        longest = int(n.max()) if rows else 0
        tiers = (int((n <= wave).sum()), int(((n > wave) & (n <= lds)).sum()), int((n > lds).sum())) if rows else (0, 0, 0)
        slow = name in ("comb", "serpentine x2")
        reps = 3 if slow else 20
        med, lo, hi = event_us(call, reps=reps, warm=1 if slow else 3)
        out = event_us(trace)
        print(f"{name:12s}: {found} rings ({tiers[0]} wave, {tiers[1]} LDS, {tiers[2]} workspace tier), longest {longest} vertices; "
              f"vertices {written} -> {kept}, status {status} -> {status_s}", flush=True)
        print(f"              simplify {med:9.1f} us ({lo:.1f} .. {hi:.1f});  (a) c3d_scene_outlines {out[0]:8.1f} us ({out[1]:.1f} .. "
              f"{out[2]:.1f}): the simplification costs {med / out[0]:.2f} of it", flush=True)
        t = []
        for _ in range(5):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            host = (rings[:rows].cpu().numpy(), vertices[:written].cpu().numpy())
            t.append((time.perf_counter() - t0) * 1e6)
        r_np, v_np = host
        take, seen = 0, 0
        while take < rows and seen + int(r_np[take, 2]) <= max(SAMPLE, int(r_np[0, 2])):
            seen += int(r_np[take, 2])
            take += 1
        t0 = time.perf_counter()
        for _, start, nv, *_ in r_np[:take].tolist():
            R.simplify_ring([tuple(p) for p in v_np[start:start + nv].tolist()], q)
        py = (time.perf_counter() - t0) * 1e6
        scale = written / seen if seen else 0.0
        print(f"              (b) on the host: download of the rings {np.median(t):9.1f} us + Python restatement {py * scale / 1e3:10.1f} ms "
              f"({py / 1e3:.1f} ms for the first {take} rings, {seen} vertices, scaled by {scale:.1f})", flush=True)


if __name__ == "__main__":
    main()
