"""c3d_scene_split on the MI355X at 1024 x 1024, 8-connectivity, no class map and no score, at R = 3 and R = 8, on the four masks
of tools/objects_step.py (blobs, random at density 0.59, all foreground, the 1-px serpentine) and two more: a field of touching
discs (radius 30 on a pitch of 59: every disc overlaps its four neighbours by a pixel, through necks about 11 px wide that R = 8
breaks and R = 3 does not) and the thick
serpentine of tests/split_reference.py (one seed, the front walks every corridor: the worst case of the rounds).  Buffers are
allocated once; a call is timed with device events around repeated calls after a warm-up, median over five rounds.

Per mask and radius: the rounds that changed something (info[2]); the whole call with max_rounds = 32 (the Python default; the
thick serpentine gets what it needs) and with max_rounds = rounds + 1, the fewest that prove convergence; the call with
max_rounds = 1, which is everything but the growth plus one round; the growth as the difference; and the price of a round that
returns at once, from a call with 64 rounds more than needed.  Next to them c3d_scene_objects on the same mask in the same
process, and the host way: the download of the mask, scipy.ndimage.distance_transform_edt and scipy.ndimage.label where scipy
is importable, and the growth of the restatement (a heap Dijkstra in Python, R = 3 only, one run).  Writes stdout
(`python tools/split_step.py > profiles/scene_split.txt`)."""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from change3d_amd import _lib as L  # noqa: E402
from change3d_amd import ops  # noqa: E402
from objects_step import ROUNDS, S, event_us, masks  # noqa: E402
import split_reference as R  # noqa: E402

RADII = (3, 8)
EXTRA = 64


def more_masks():
    yy, xx = np.mgrid[0:S, 0:S]
    discs = (((yy % 59) - 29) ** 2 + ((xx % 59) - 29) ** 2 <= 30 * 30).astype(np.uint8)
    return masks() + [("touching discs", discs), ("thick serpentine", R.thick_serpentine(S, S))]


def host_us(mask, ndimage, r2, grow):
    t0 = time.perf_counter()
    host = mask.cpu().numpy()
    t1 = time.perf_counter()
    if ndimage is None:
        return (t1 - t0) * 1e6, None, None
    core = (ndimage.distance_transform_edt(np.pad(host, 1))[1:-1, 1:-1] ** 2 > r2 + 0.5) & (host != 0)
    ndimage.label(core, structure=np.ones((3, 3), dtype=int))
    t2 = time.perf_counter()
    if not grow:
        return (t1 - t0) * 1e6, (t2 - t1) * 1e6, None
    ids, _ = R.seed_ids(core, 8)
    R.grow_dijkstra(host, ids, 8)
    return (t1 - t0) * 1e6, (t2 - t1) * 1e6, (time.perf_counter() - t2) * 1e6


def main():
    dev = torch.device("cuda:0")
    try:
        from scipy import ndimage
    except ImportError:
        ndimage = None
    print(f"# tools/split_step.py: {S} x {S}, 8-connectivity; device events, 20 calls, {ROUNDS} rounds, median (min .. max) in us; "
          f"{os.path.basename(L.LIB_PATH)}; tile {ops.scene_split_tile()}")
    ws = torch.empty(L.lib().c3d_scene_split_ws_bytes(S, S, 1), dtype=torch.uint8, device=dev)
    fmt = lambda r: f"{r[0]:9.1f} ({r[1]:.1f} .. {r[2]:.1f})"  # noqa: E731
    slower = []
    for name, mask_np in more_masks():
        mask = torch.from_numpy(mask_np).to(dev)
        objects = event_us(lambda: ops.scene_objects(mask, connectivity=8, want_hist=False, want_object_cls=False))
        n_obj = int(ops.scene_objects(mask, connectivity=8, want_hist=False, want_object_cls=False)[4][0])
        print(f"{name:16s}: density {mask_np.mean():.2f}, {n_obj} components; c3d_scene_objects {fmt(objects)}")
        for r in RADII:
            call = lambda m: ops.scene_split(mask, r, connectivity=8, max_rounds=m, want_hist=False, want_object_cls=False, ws=ws)  # noqa: E731
            out = call(16384)
            torch.cuda.synchronize()
            status, seeds, used, _ = out[5].tolist()
            pieces = int(out[4][0])
            assert status == 0, (name, r, status)
            need = used + 1
            default = max(32, need)
            whole, least, one = event_us(lambda: call(default), reps=5), event_us(lambda: call(need), reps=5), event_us(lambda: call(1), reps=5)
            extra = event_us(lambda: call(need + EXTRA), reps=5)
            per_idle = (extra[0] - least[0]) / EXTRA
            download, label, grow = host_us(mask, ndimage, r * r, grow=r == RADII[0])
            host = download + (label or 0.0) + (grow or 0.0)
            print(f"    R = {r}: {seeds} seeds, {pieces} pieces, {used} rounds changed something\n"
                  f"      whole call, max_rounds = {default:<5d} {fmt(whole)}   {S * S / whole[0]:7.1f} Mpx/s   {whole[0] / objects[0]:.2f} x scene_objects\n"
                  f"      whole call, max_rounds = {need:<5d} {fmt(least)}\n"
                  f"      max_rounds = 1 (all but growth) {fmt(one)}   growth rounds ~ {least[0] - one[0]:.1f} us\n"
                  f"      a round that returns at once     {per_idle:9.2f} us each; the {default - need} unused of {default}: {per_idle * (default - need):.1f} us\n"
                  f"      host: download {download:.0f} us" + (f", scipy edt + label {label:.0f} us" if label is not None else "")
                  + (f", Python Dijkstra growth {grow:.0f} us" if grow is not None else "") +
                  f"; device / host (without the growth) = {whole[0] / (download + (label or 0.0)):.4f}")
            if whole[0] > download + (label or 0.0):
                slower.append((name, r, whole[0], download + (label or 0.0), host if grow is not None else None))
    for name, r, d, h, full in slower:
        print(f"SLOWER than the host's download + edt + label, which leaves the growth out: {name}, R = {r}: {d:.1f} us against {h:.1f} us"
              + (f" ({full:.1f} us with the Python growth)" if full is not None else ""))
    if not slower:
        print("no mask is slower on the device than the host's download + scipy edt + label, which leaves the growth out")


if __name__ == "__main__":
    main()
