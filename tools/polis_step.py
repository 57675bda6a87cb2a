"""c3d_rings_polis on the MI355X at 1024 x 1024, 8-connectivity, on the masks of tools/objects_step.py: the prediction is the
traced rings of the mask (raw, then simplified at 1 px), the ground truth the traced rings of the mask shifted by (2, 3) and,
because that shift leaves the noise and the serpentine without a single match, also the raw rings of the mask itself; the match
is that of c3d_objects_match on the two label maps.  Timed with device events around repeated calls after a warm-up, median
over several rounds, in one process, next to the c3d_outlines_simplify call on the same mask and next to the host way: the
download of the tables plus the rule vectorised with numpy, pair by pair (timed once).  Then one pair built to sit at the
default max_pair_work, and the time per kernel of one call on the blobs and on the noise from torch's profiler.  Writes stdout
(`python tools/polis_step.py > profiles/rings_polis.txt`)."""
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

TOL, SHIFT = 1.0, (2, 3)
HOST_BLOCK = 1 << 22                                         # point-edge values per numpy block of the host way


def group(rings, vertices, counts):
    """id -> list of float64 [n, 2] rings with n >= 3, in row order (every row of a traced table is valid)."""
    out = {}
    for i, start, n in rings[:int(counts[1]), :3].tolist():
        if start >= 0 and n >= 3:
            out.setdefault(i, []).append(vertices[start:start + n].astype(np.float64))
    return out


def host_distances(points, rings):
    """The rule of include/change3d_hip.h in numpy: the distance of every point to the nearest edge of the rings."""
    a = np.concatenate(rings)
    b = np.concatenate([np.roll(r, -1, axis=0) for r in rings])
    e = b - a
    L2 = (e * e).sum(axis=1)
    out = np.empty(len(points))
    step = max(1, HOST_BLOCK // len(a))
    for at in range(0, len(points), step):
        p = points[at:at + step, None, :]
        w = p - a[None]
        t = (w * e[None]).sum(axis=2)
        c = w[..., 0] * e[None, :, 1] - w[..., 1] * e[None, :, 0]
        u = p - b[None]
        with np.errstate(divide="ignore", invalid="ignore"):
            v = np.where((L2[None] == 0) | (t <= 0), (w * w).sum(axis=2), np.where(t >= L2[None], (u * u).sum(axis=2), c * c / L2[None]))
        out[at:at + step] = np.sqrt(v.min(axis=1))
    return out


def host_way(pred, gt, match_p, max_pair_work):
    """Download, then PoLiS of every scored pair on the host: (seconds, pairs, sum of PoLiS)."""
    t0 = time.perf_counter()
    tp, tg = [t.cpu().numpy() for t in pred], [t.cpu().numpy() for t in gt]
    match = match_p.cpu().numpy()
    gp, gg = group(*tp), group(*tg)
    pairs, total = 0, 0.0
    for p in range(1, int(tp[0][:int(tp[2][1]), 0].max(initial=0)) + 1):
        g = int(match[p - 1, 0])
        if g < 1 or p not in gp or g not in gg:
            continue
        vp, vg = np.concatenate(gp[p]), np.concatenate(gg[g])
        if 2 * len(vp) * len(vg) > max_pair_work:
            continue
        total += (host_distances(vp, gg[g]).mean() + host_distances(vg, gp[p]).mean()) / 2
        pairs += 1
    return time.perf_counter() - t0, pairs, total


def circle(n, radius, cx, cy):
    return [(int(round(cx + radius * math.cos(2 * math.pi * k / n))), int(round(cy + radius * math.sin(2 * math.pi * k / n)))) for k in range(n)]


def table(ring, dev):
    rings = np.zeros((2, 8), np.int32)
    rings[0, :3] = (1, 0, len(ring))
    return [torch.from_numpy(a).to(dev) for a in (rings, np.asarray(ring, np.int32), np.array([1, 1, len(ring), len(ring), 0], np.int32))]


def rectangle_table(dev, long_px=40, short_px=25, size=96):
    """Rotated rectangles of 40 x 25 px, rasterised, then traced, simplified at 1 px and regularised on the device, each stage
    scored against the true rectangle at 1/16 px."""
    print(f"rotated rectangles of {long_px} x {short_px} px against the true rectangle (direction, stage, vertices, PoLiS px, vertex Hausdorff px):")
    yy, xx = np.mgrid[:size, :size]
    for d in ((3, 1), (2, 5), (5, -2), (1, 1)):
        norm = math.hypot(*d)
        ux, uy = d[0] / norm, d[1] / norm
        px, py = xx + 0.5 - size / 2, yy + 0.5 - size / 2
        mask = ((np.abs(px * ux + py * uy) <= long_px / 2) & (np.abs(py * ux - px * uy) <= short_px / 2)).astype(np.uint8)
        corners = [(int(round(16 * (size / 2 + a * long_px / 2 * ux - b * short_px / 2 * uy))),
                    int(round(16 * (size / 2 + a * long_px / 2 * uy + b * short_px / 2 * ux)))) for a, b in ((-1, -1), (1, -1), (1, 1), (-1, 1))]
        labels, tab, _, _, counts = ops.scene_objects(torch.from_numpy(mask).to(dev), connectivity=8, max_objects=4)
        raw = ops.scene_outlines(labels, counts, connectivity=8, max_objects=4, max_rings=8, max_vertices=4 * size * size)
        simple = ops.outlines_simplify(*raw, TOL)
        regular = ops.rings_regularize(*simple, *ops.rings_hull(*raw, max_objects=4), frac_bits=4)
        match = torch.tensor([[1, 0, 0, 0]] * 4, dtype=torch.int32, device=dev)
        for stage, rings, f in (("raw", raw, 0), ("simplified", simple, 0), ("regularised", regular, 4)):
            pair, pair_n, _, _ = ops.rings_polis(*rings, f, *table(corners, dev), 4, match, 1)
            print(f"  {str(d):8s} {stage:12s} {int(pair_n[0, 1]):4d}  {float(pair[0, 0]):.3f}  {float(pair[0, 1]):.3f}")


def main():
    if not torch.cuda.is_available():
        raise SystemExit("tools/polis_step.py measures on the GPU; there is none here")
    dev = torch.device("cuda:0")
    max_objects = S * S // 2 + 1
    max_rings, max_vertices = S * S // 2 + 1, 2 * S * S + 4  # nothing is cut off on any of the masks
    work = 2 ** 32
    nbytes = L.lib().c3d_rings_polis_ws_bytes(max_rings, max_vertices, max_objects, max_rings, max_vertices, max_objects)
    limits = ops.rings_polis_limits()
    print(f"# tools/polis_step.py: {S} x {S}, 8-connectivity, ground truth = the mask shifted by {SHIFT}, max_pair_work 2^32; workspace "
          f"{nbytes / 2**20:.1f} MiB; limits (wave, job, tile, rings, long ring) {limits}; device events, {ROUNDS} rounds of 20 calls, median "
          f"(min .. max); {os.path.basename(L.LIB_PATH)}")
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    ws_s = torch.empty(L.lib().c3d_outlines_simplify_ws_bytes(max_rings, max_vertices), dtype=torch.uint8, device=dev)
    profiled = {}
    rectangle_table(dev)
    for name, mask_np in masks():
        moved = np.zeros_like(mask_np)
        moved[SHIFT[0]:, SHIFT[1]:] = mask_np[:S - SHIFT[0], :S - SHIFT[1]]
        sides = []
        for m in (mask_np, moved):
            labels, tab, _, _, counts_obj = ops.scene_objects(torch.from_numpy(m).to(dev), connectivity=8, max_objects=max_objects,
                                                              want_object_cls=False)
            sides.append((labels, tab, counts_obj, ops.scene_outlines(labels, counts_obj, connectivity=8, max_objects=max_objects,
                                                                      max_rings=max_rings, max_vertices=max_vertices)))
        (lp, tp, cp, raw), (lg, tg, cg, gt) = sides
        variants = (("shifted", gt, ops.objects_match(lp, tp, cp, lg, tg, cg)[0]), ("itself", raw, ops.objects_match(lp, tp, cp, lp, tp, cp)[0]))
        simplify = lambda: ops.outlines_simplify(*raw, TOL, ws=ws_s)  # noqa: E731
        simple = simplify()
        t_sim = event_us(simplify)
        print(f"{name:12s}: density {mask_np.mean():.2f}, {int(cp[1])} objects, {int(raw[2][2])} raw vertices, {int(simple[2][2])} simplified; "
              f"c3d_outlines_simplify {t_sim[0]:8.1f} us ({t_sim[1]:.1f} .. {t_sim[2]:.1f})")
        for (truth, gt, match_p), (stage, pred) in ((v, st) for v in variants for st in (("raw", raw), ("simplified", simple))):
            call = lambda: ops.rings_polis(*pred, 0, *gt, 0, match_p, max_objects, max_pair_work=work, ws=ws)  # noqa: E731
            pair, pair_n, counts, sums = call()
            torch.cuda.synchronize()
            c, rows = counts.tolist(), pair_n.cpu().numpy().astype(np.int64)
            rows = rows[(rows[:, 3] == 0) & (rows[:, 1] > 0)]   # the scored pairs: a row past the last object is all zero
            jobs = int(((rows[:, 1] > limits[0]) | (rows[:, 2] > limits[0])).sum())
            evals = int((2 * rows[:, 1] * rows[:, 2]).sum())
            t = event_us(call)
            host = host_way(pred, gt, match_p, work)
            agree = abs(host[2] - float(sums[0])) <= 1e-9 * max(1.0, host[2]) and host[1] == c[0]
            print(f"  {stage:10s} against {truth:7s}: scored {c[0]} (wave tier {c[0] - jobs}, job tier {jobs}), no partner {c[1]}, incomplete {c[2]}, over work {c[3]}, "
                  f"status {c[6]}; {evals / 1e6:.1f} M point-edge values, largest pair {int(rows[:, 1].max(initial=0))} x "
                  f"{int(rows[:, 2].max(initial=0))}; polis mean {float(sums[0]) / max(c[0], 1):.4f} hausdorff max {float(sums[2]):.4f}")
            print(f"  {'':26s}  rings_polis {t[0]:8.1f} us ({t[1]:.1f} .. {t[2]:.1f}) = {t[0] / t_sim[0]:.2f} of the simplify call;  host way "
                  f"{host[0] * 1e6:10.1f} us ({host[1]} pairs, sums {'agree' if agree else 'DIFFER'}): {host[0] * 1e6 / t[0]:.1f} x the device")
            if stage == "raw" and (name.strip(), truth) in (("blobs", "shifted"), ("random 0.59", "itself")):
                profiled[name.strip()] = lambda pr=pred, g=gt, m=match_p: ops.rings_polis(*pr, 0, *g, 0, m, max_objects, max_pair_work=work, ws=ws)  # noqa: E731

    n = int(math.isqrt(work // 2))                           # 2 n^2 <= 2^32 < 2 (n + 1)^2
    a, b = table(circle(n, 30000, 0, 0), dev), table(circle(n, 30000, 40, -25), dev)
    match = torch.tensor([[1, 0, 0, 0]], dtype=torch.int32, device=dev)
    call = lambda: ops.rings_polis(*a, 0, *b, 0, match, 1, max_pair_work=work)  # noqa: E731
    pair, pair_n, counts, _ = call()
    torch.cuda.synchronize()
    t = event_us(call, reps=3, warm=1)
    print(f"one pair at the cap: {n} x {n} vertices, 2 n^2 = {2 * n * n} <= 2^32, flag {int(pair_n[0, 3])}, polis {float(pair[0, 0]):.4f}: "
          f"{t[0] / 1e3:8.2f} ms ({t[1] / 1e3:.2f} .. {t[2] / 1e3:.2f}), {2 * n * n / t[0] / 1e3:.1f} G point-edge values / s")
    over = ops.rings_polis(*a, 0, *b, 0, match, 1, max_pair_work=2 * n * n - 1)[1]
    print(f"the same pair one under the cap: flag {int(over[0, 3])}")

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
                    if "polis_" in e.key or "Memset (" in e.key]
            print(f"per kernel, {name} raw, 10 calls (torch profiler):")
            for key, count, total in sorted(rows, key=lambda r: -r[2]):
                found = re.search(r"polis_\w+", key)
                print(f"  {found.group(0) if found else key[:40]:24s} {count:4d} launches {total / max(count, 1):9.1f} us each")
    except Exception as e:                                   # the profiler is a convenience: the totals above stand without it
        print(f"per kernel: torch's profiler is not available here ({type(e).__name__}: {e})")

if __name__ == "__main__":
    main()
