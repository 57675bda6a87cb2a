"""c3d_scene_edt and c3d_boundary_counts on the MI355X at 1024 x 1024, on the four masks of tools/objects_step.py (blobs, random
at density 0.59, all foreground, serpentine) and three more: all background, and a single site in one corner, which is the
uncapped worst case of the row pass (every pixel searches to the end of its row), once for each of the two transforms that see
it (the mask itself, and its INVERT).  Buffers are allocated once; a call is timed with device events around 20 repeated calls
after a warm-up, median over five rounds.  Measured: the transform uncapped and at cap2 = 25; the boundary counts of the mask
against itself shifted by (2, 3) at d = tau = 2 and 5; for scale the c3d_scene_objects call on the same mask (8-connectivity, no
class map, no score); and the host way, the download of the mask plus scipy.ndimage.distance_transform_edt where scipy is
importable, the download alone otherwise.  Writes stdout (`python tools/edt_step.py > profiles/scene_edt.txt`)."""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from change3d_amd import _lib as L  # noqa: E402
from change3d_amd import ops  # noqa: E402
from objects_step import ROUNDS, S, event_us, masks  # noqa: E402


def more_masks():
    corner = np.ones((S, S), np.uint8)
    corner[0, 0] = 0
    return masks() + [("background", np.zeros((S, S), np.uint8)), ("corner site", corner)]


def host_us(mask, ndimage, reps=3):
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        host = mask.cpu().numpy()
        if ndimage is not None:
            ndimage.distance_transform_edt(host)
        t.append((time.perf_counter() - t0) * 1e6)
    return float(np.median(t))


def main():
    dev = torch.device("cuda:0")
    try:
        from scipy import ndimage
    except ImportError:
        ndimage = None
    host_name = "download + scipy.ndimage.distance_transform_edt" if ndimage is not None else "download alone (scipy is not importable)"
    print(f"# tools/edt_step.py: {S} x {S}; device events, 20 calls, {ROUNDS} rounds, median (min .. max) in us; "
          f"{os.path.basename(L.LIB_PATH)}; tile {ops.scene_edt_tile()}")
    print(f"# host: {host_name}, wall clock, median of 3")
    dist2 = torch.empty((S, S), dtype=torch.int32, device=dev)
    ws_edt = torch.empty(L.lib().c3d_scene_edt_ws_bytes(S, S), dtype=torch.uint8, device=dev)
    ws_counts = torch.empty(L.lib().c3d_boundary_counts_ws_bytes(S, S), dtype=torch.uint8, device=dev)
    worst = None
    for name, mask_np in more_masks():
        mask = torch.from_numpy(mask_np).to(dev)
        other = torch.from_numpy(np.ascontiguousarray(np.roll(mask_np, (2, 3), (0, 1)))).to(dev)
        fmt = lambda r: f"{r[0]:9.1f} ({r[1]:.1f} .. {r[2]:.1f})"  # noqa: E731
        full = event_us(lambda: ops.scene_edt(mask, out=dist2, ws=ws_edt))
        far = int((dist2 == L.EDT_FAR).sum())
        reach = int(dist2[dist2 != L.EDT_FAR].max()) if far < S * S else -1
        capped = event_us(lambda: ops.scene_edt(mask, cap2=25, out=dist2, ws=ws_edt))
        inverted = event_us(lambda: ops.scene_edt(mask, invert=True, out=dist2, ws=ws_edt))
        b2 = event_us(lambda: ops.boundary_counts(mask, other, 2, ws=ws_counts))
        b5 = event_us(lambda: ops.boundary_counts(mask, other, 5, ws=ws_counts))
        objects = event_us(lambda: ops.scene_objects(mask, connectivity=8, want_hist=False, want_object_cls=False))
        host = host_us(mask, ndimage)
        slowest = max(full[0], inverted[0])
        if worst is None or slowest / host > worst[1]:
            worst = (name, slowest / host, slowest, host)
        print(f"{name:12s}: density {mask_np.mean():.2f}, largest dist2 {reach}\n"
              f"    edt uncapped   {fmt(full)}   {S * S / full[0]:7.1f} Mpx/s\n"
              f"    edt INVERT     {fmt(inverted)}\n"
              f"    edt cap2 = 25  {fmt(capped)}\n"
              f"    counts d = 2   {fmt(b2)}\n"
              f"    counts d = 5   {fmt(b5)}\n"
              f"    scene_objects  {fmt(objects)}\n"
              f"    host           {host:9.1f}   uncapped device / host = {max(full[0], inverted[0]) / host:.4f}")
    print(f"worst device-against-host: {worst[0]}, {worst[2]:.1f} us against {worst[3]:.1f} us = {worst[1]:.4f}")


if __name__ == "__main__":
    main()
