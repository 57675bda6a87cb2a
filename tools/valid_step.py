"""c3d_rings_valid on the MI355X at 1024 x 1024, 8-connectivity, on the masks of tools/objects_step.py: the traced rings of the
mask, raw and simplified at 1 px.  Timed with device events around repeated calls after a warm-up, median over several rounds,
in one process, next to the c3d_outlines_simplify call on the same mask and next to the host way: the download of the tables
plus the rule of include/change3d_hip.h vectorised with numpy, object by object (timed once; objects above HOST_EDGES edges are
left to the device and the pairs the host did cover are stated).  Then one id built to sit at the default max_id_work, and the
time per kernel of one call on the raw rings of the blobs, the noise and the serpentine from torch's profiler.  Writes stdout
(`python tools/valid_step.py > profiles/rings_valid.txt`)."""
import math
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
HOST_BLOCK = 1 << 22                                         # edge pairs per numpy block of the host way
HOST_EDGES = 8192                                            # the host way stops at ids of this many edges


def host_id(a, b, ring, n):
    """(cross, overlap, touch_vv, touch_ve) of one id on the host: a, b i64 [m, 2] the edge ends, ring [m] the place of the
    edge's ring in the id's list, n [m] its vertex count.  The rule of the header, all pairs with j > i, a block of rows at a time."""
    m = len(a)
    pos = np.arange(m)
    live = (a != b).any(axis=1)
    e = b - a
    got = np.zeros(4, dtype=np.int64)
    step = max(1, HOST_BLOCK // m)

    def cross(ux, uy, vx, vy):
        return np.sign(ux * vy - uy * vx)

    for i0 in range(0, m, step):
        i = slice(i0, min(i0 + step, m))
        pair = live[i, None] & live[None, :] & (pos[None, :] > pos[i, None])
        ax, ay, bx, by = (v[i, None] for v in (a[:, 0], a[:, 1], b[:, 0], b[:, 1]))
        cx, cy, dx, dy = (v[None, :] for v in (a[:, 0], a[:, 1], b[:, 0], b[:, 1]))
        ex, ey, fx, fy = e[i, 0, None], e[i, 1, None], e[None, :, 0], e[None, :, 1]
        o1, o2 = cross(ex, ey, cx - ax, cy - ay), cross(ex, ey, dx - ax, dy - ay)
        o3, o4 = cross(fx, fy, ax - cx, ay - cy), cross(fx, fy, bx - cx, by - cy)
        d = np.abs(pos[None, :] - pos[i, None])
        adjacent = (ring[i, None] == ring[None, :]) & ((d == 1) | (d == n[i, None] - 1))
        is_cross = pair & (o1 * o2 < 0) & (o3 * o4 < 0)
        flat = pair & (o1 == 0) & (o2 == 0) & (o3 == 0) & (o4 == 0)
        tc, td, L2 = (cx - ax) * ex + (cy - ay) * ey, (dx - ax) * ex + (dy - ay) * ey, ex * ex + ey * ey
        lo, hi = np.maximum(np.minimum(tc, td), 0), np.minimum(np.maximum(tc, td), L2)
        overlap = flat & (lo < hi)
        meet = pair & ~is_cross & ~flat & (o1 * o2 <= 0) & (o3 * o4 <= 0) & ~adjacent
        ends = ((ax == cx) & (ay == cy)) | ((ax == dx) & (ay == dy)) | ((bx == cx) & (by == cy)) | ((bx == dx) & (by == dy))
        got += (is_cross.sum(), overlap.sum(), (flat & (lo == hi) & ~adjacent).sum() + (meet & ends).sum(), (meet & ~ends).sum())
    return got


def host_way(table, work):
    """Download, then the rule on the host for every id of at most HOST_EDGES edges: (seconds, ids, pairs, {id: counts})."""
    t0 = time.perf_counter()
    rings, vertices, counts = (t.cpu().numpy() for t in table)
    by_id = {}
    for i, start, n in rings[:int(counts[1]), :3].tolist():
        if start >= 0 and n >= 3:
            by_id.setdefault(i, []).append((start, n))
    out, pairs = {}, 0
    for i, rows in by_id.items():
        m = sum(n for _, n in rows)
        if m > HOST_EDGES or m * (m - 1) // 2 > work:
            continue
        a = np.concatenate([vertices[s:s + n] for s, n in rows]).astype(np.int64)
        b = np.concatenate([np.roll(vertices[s:s + n], -1, axis=0) for s, n in rows]).astype(np.int64)
        at = np.cumsum([0] + [n for _, n in rows[:-1]])
        out[i] = host_id(a, b, np.repeat(at, [n for _, n in rows]), np.repeat([n for _, n in rows], [n for _, n in rows]))
        pairs += m * (m - 1) // 2
    return time.perf_counter() - t0, len(out), pairs, out


def circle(n, radius):
    return [(int(round(radius * math.cos(2 * math.pi * k / n))), int(round(radius * math.sin(2 * math.pi * k / n)))) for k in range(n)]


def table(ring, dev):
    rings = np.zeros((2, 8), np.int32)
    rings[0, :3] = (1, 0, len(ring))
    return [torch.from_numpy(a).to(dev) for a in (rings, np.asarray(ring, np.int32), np.array([1, 1, len(ring), len(ring), 0], np.int32))]


def main():
    if not torch.cuda.is_available():
        raise SystemExit("tools/valid_step.py measures on the GPU; there is none here")
    dev = torch.device("cuda:0")
    max_objects = S * S // 2 + 1
    max_rings, max_vertices = S * S // 2 + 1, 2 * S * S + 4  # nothing is cut off on any of the masks
    work = 2 ** 32
    nbytes = L.lib().c3d_rings_valid_ws_bytes(max_rings, max_vertices, max_objects)
    limits = ops.rings_valid_limits()
    print(f"# tools/valid_step.py: {S} x {S}, 8-connectivity, max_id_work 2^32; workspace {nbytes / 2**20:.1f} MiB; limits (wave, chunk, tile, "
          f"rings, long ring) {limits}; device events, {ROUNDS} rounds of 20 calls, median (min .. max); host way up to {HOST_EDGES} edges "
          f"per id; {os.path.basename(L.LIB_PATH)}")
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    ws_s = torch.empty(L.lib().c3d_outlines_simplify_ws_bytes(max_rings, max_vertices), dtype=torch.uint8, device=dev)
    profiled = {}
    for name, mask_np in masks():
        labels, _, _, _, counts_obj = ops.scene_objects(torch.from_numpy(mask_np).to(dev), connectivity=8, max_objects=max_objects,
                                                        want_object_cls=False)
        raw = ops.scene_outlines(labels, counts_obj, connectivity=8, max_objects=max_objects, max_rings=max_rings, max_vertices=max_vertices)
        simplify = lambda: ops.outlines_simplify(*raw, TOL, ws=ws_s)  # noqa: E731
        simple = simplify()
        t_sim = event_us(simplify)
        print(f"{name:12s}: density {mask_np.mean():.2f}, {int(counts_obj[1])} objects, {int(raw[2][2])} raw vertices, {int(simple[2][2])} simplified; "
              f"c3d_outlines_simplify {t_sim[0]:8.1f} us ({t_sim[1]:.1f} .. {t_sim[2]:.1f})")
        for stage, rings in (("raw", raw), ("simplified", simple)):
            call = lambda: ops.rings_valid(*rings, 0, max_objects, max_id_work=work, ws=ws)  # noqa: E731
            valid, counts = call()
            torch.cuda.synchronize()
            c = counts.tolist()
            rows = valid[:sum(c[:1] + c[2:5])].cpu().numpy()
            checked = rows[rows[:, 0] == 0]
            jobs = int((checked[:, 2] + checked[:, 3] > limits[0]).sum())
            pairs = int((checked[:, 2] * (checked[:, 2] - 1) // 2).sum())
            t = event_us(call)
            host = host_way(rings, work)
            agree = all((rows[i - 1, 4:] == got).all() for i, got in host[3].items())
            print(f"  {stage:10s}: checked {c[0]} (wave tier {c[0] - jobs}, job tier {jobs}), invalid {c[1]}, empty {c[2]}, incomplete {c[3]}, over work "
                  f"{c[4]}, status {c[7]}; {pairs / 1e6:.3f} M edge pairs, largest checked id {int(checked[:, 2].max(initial=0))} edges, largest id "
                  f"{int(rows[:, 2].max(initial=0))}; crossings {c[5]} overlaps {c[6]} touches {int(checked[:, 6:].sum())}")
            print(f"  {'':10s}  rings_valid {t[0]:8.1f} us ({t[1]:.1f} .. {t[2]:.1f}) = {t[0] / t_sim[0]:.2f} of the simplify call;  host way "
                  f"{host[0] * 1e6:10.1f} us over {host[1]} ids and {host[2] / 1e6:.3f} M pairs (counts {'agree' if agree else 'DIFFER'}): "
                  f"{host[0] * 1e6 / t[0]:.1f} x the device")
            if stage == "raw" and name.strip() in ("blobs", "random 0.59", "serpentine"):
                profiled[name.strip()] = lambda r=rings: ops.rings_valid(*r, 0, max_objects, max_id_work=work, ws=ws)  # noqa: E731

    n = (1 + math.isqrt(1 + 8 * work)) // 2                  # n (n - 1) / 2 <= 2^32 < (n + 1) n / 2
    one = table(circle(n, 30000 * 256), dev)
    call = lambda: ops.rings_valid(*one, 8, 1, max_id_work=work)  # noqa: E731
    valid, _ = call()
    torch.cuda.synchronize()
    t = event_us(call, reps=3, warm=1)
    print(f"one id at the cap: {n} edges at frac_bits 8, n (n - 1) / 2 = {n * (n - 1) // 2} <= 2^32, row {valid[0].tolist()}: "
          f"{t[0] / 1e3:8.2f} ms ({t[1] / 1e3:.2f} .. {t[2] / 1e3:.2f}), {n * (n - 1) // 2 / t[0] / 1e3:.1f} G edge pairs / s")
    over = ops.rings_valid(*one, 8, 1, max_id_work=n * (n - 1) // 2 - 1)[0]
    t_over = event_us(lambda: ops.rings_valid(*one, 8, 1, max_id_work=n * (n - 1) // 2 - 1))
    print(f"the same id one under the cap: flag {int(over[0, 0])}, {t_over[0]:.1f} us")

    try:                                                     # the time per kernel of one call, raw stage
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
                    if "valid_" in e.key or "Memset (" in e.key]
            print(f"per kernel, {name} raw, 10 calls (torch profiler):")
            for key, count, total in sorted(rows, key=lambda r: -r[2]):
                found = re.search(r"valid_\w+", key)
                print(f"  {found.group(0) if found else key[:40]:24s} {count:4d} launches {total / max(count, 1):9.1f} us each")
    except Exception as e:                                   # the profiler is a convenience: the totals above stand without it
        print(f"per kernel: torch's profiler is not available here ({type(e).__name__}: {e})")


if __name__ == "__main__":
    main()
