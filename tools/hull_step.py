"""c3d_rings_hull on the MI355X at 1024 x 1024, 8-connectivity, on the masks of tools/objects_step.py plus the checkerboard and
a lattice disc of radius 500 (one object whose outline alone has some four thousand vertices): the hulls and rectangles of the
rings of c3d_scene_outlines, timed with device events around repeated calls after a warm-up, median over several rounds, in
one process, next to the c3d_scene_outlines call on the same mask.  Then the host way, once: the download of the ring table
and the vertices plus scipy.spatial.ConvexHull per object (objects of fewer than three distinct points or without area are
counted, not hulled), with the share of objects whose vertex set equals the device's.  Writes stdout
(`python tools/hull_step.py > profiles/rings_hull.txt`)."""
import os
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


def host_way(rings, vertices, counts, hulls, hull_vertices):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r, v, c = rings.cpu().numpy(), vertices.cpu().numpy(), counts.cpu().numpy()
    t_down = (time.perf_counter() - t0) * 1e6
    line = f"              host: download of the tables {t_down:10.1f} us;  "
    try:
        from scipy.spatial import ConvexHull, QhullError
    except ImportError:
        print(line + "scipy not installed")
        return
    h, hv = hulls.cpu().numpy(), hull_vertices.cpu().numpy()
    t0 = time.perf_counter()
    rows = r[:int(c[1])]
    order = np.argsort(rows[:, 0], kind="stable")
    cuts = np.flatnonzero(np.diff(rows[order, 0])) + 1
    found = {}
    for group in np.split(order, cuts):
        pts = np.concatenate([v[rows[k, 1]:rows[k, 1] + rows[k, 2]] for k in group])
        try:
            found[int(rows[group[0], 0])] = pts[ConvexHull(pts).vertices]
        except QhullError:
            pass
    t_host = (time.perf_counter() - t0) * 1e6
    same = sum(1 for rid, p in found.items()
               if {tuple(q) for q in p.tolist()} == {tuple(q) for q in hv[h[rid - 1, 1]:h[rid - 1, 1] + h[rid - 1, 2]].tolist()})
    print(line + f"scipy.spatial.ConvexHull per object {t_host:12.1f} us for {len(found)} objects, {same} with the device's vertex set")


def main():
    if not torch.cuda.is_available():
        raise SystemExit("tools/hull_step.py measures on the GPU; there is none here")
    dev = torch.device("cuda:0")
    max_objects = S * S // 2 + 1
    max_rings, max_vertices = S * S // 2 + 1, 2 * S * S + 4  # nothing is cut off on any of the masks
    nbytes = L.lib().c3d_rings_hull_ws_bytes(max_rings, max_vertices, max_objects)
    print(f"# tools/hull_step.py: {S} x {S}, 8-connectivity; workspace {nbytes / 2**20:.1f} MiB; tier limits {ops.rings_hull_limits()}; "
          f"device events, {ROUNDS} rounds of 20 calls, median (min .. max); {os.path.basename(L.LIB_PATH)}")
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    ws_o = torch.empty(L.lib().c3d_scene_outlines_ws_bytes(S, S), dtype=torch.uint8, device=dev)
    yy, xx = np.mgrid[0:S, 0:S]
    extra = [("checkerboard", ((yy + xx) % 2 == 0).astype(np.uint8)),
             ("disc 500", ((yy - S // 2) ** 2 + (xx - S // 2) ** 2 < 500 * 500).astype(np.uint8))]
    for name, mask_np in masks() + extra:
        mask = torch.from_numpy(mask_np).to(dev)
        labels, table, _, _, counts_obj = ops.scene_objects(mask, connectivity=8, max_objects=max_objects, want_object_cls=False)
        trace = lambda: ops.scene_outlines(labels, counts_obj, connectivity=8, max_objects=max_objects, max_rings=max_rings,  # noqa: E731
                                           max_vertices=max_vertices, ws=ws_o)
        raw = trace()
        hull = lambda: ops.rings_hull(*raw, max_objects=max_objects, ws=ws)  # noqa: E731
        hulls, hv, rects, hc = hull()
        torch.cuda.synchronize()
        objects = int(hc[0])
        n_pts = hulls[:int(hc[1]), 7]
        wave, lds = ops.rings_hull_limits()
        print(f"{name:12s}: density {mask_np.mean():.2f}, {objects} objects ({int((n_pts > wave).sum())} in the workgroup tier, "
              f"{int((n_pts > lds).sum())} above its LDS limit, the largest has {int(n_pts.max()) if objects else 0} points and "
              f"{int(hulls[:, 2].max())} hull vertices), {int(raw[2][0])} rings, {int(raw[2][2])} vertices, {int(hc[2])} hull vertices; "
              f"status {int(hc[4])}")
        t_hull, t_trace = event_us(hull), event_us(trace)
        print(f"              hulls {t_hull[0]:8.1f} us ({t_hull[1]:.1f} .. {t_hull[2]:.1f});  c3d_scene_outlines {t_trace[0]:8.1f} us "
              f"({t_trace[1]:.1f} .. {t_trace[2]:.1f}): the hulls cost {t_hull[0] / t_trace[0]:.2f} of it")
        host_way(*raw, hulls, hv)


if __name__ == "__main__":
    main()
