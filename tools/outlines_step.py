"""c3d_scene_outlines on the MI355X at 1024 x 1024, 8-connectivity, on the four masks of tools/objects_step.py (blobs, random at
density 0.59, all foreground, serpentine: one ring with the longest links) and a checkerboard (the most rings: one outline and
a hole per inner background pixel).  The call is timed with device events around repeated calls after a warm-up, median over
several rounds, in one process, next to two yardsticks taken in the same run on the same masks: (a) c3d_scene_objects, the
labelling it follows -- csrc/scene_objects.hip is the file of the commit before this call existed, so its time here is that
commit's -- and (b) the download of the i32 label map alone, the floor of any host tracer.  With the instrumented library
(`python __graft_entry__.py --tuning`, `C3D_LIB=change3d_amd/lib/libchange3d_hip_tune.so`) the phases are also timed one by
one, as differences of prefixes (its knob C3D_OUTLINES_PHASES; the product library has no such switch).  Writes stdout
(`python tools/outlines_step.py > profiles/scene_outlines.txt`)."""
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

PHASES = ("memset+mark", "scan", "offsets", "link", "double", "ring_count", "scans", "ring_rows", "emit", "finalise")


def main():
    if not torch.cuda.is_available():
        raise SystemExit("tools/outlines_step.py measures on the GPU; there is none here")
    dev = torch.device("cuda:0")
    tuned = "tune" in os.path.basename(L.LIB_PATH)
    nbytes = L.lib().c3d_scene_outlines_ws_bytes(S, S)
    max_rings, max_vertices = S * S // 2 + 1, 2 * S * S + 4  # nothing is cut off on any of the masks
    rounds = int(np.ceil(np.log2(4 * S * S)))
    print(f"# tools/outlines_step.py: {S} x {S}, 8-connectivity; workspace {nbytes / 2**20:.1f} MiB, {rounds} doubling rounds enqueued; "
          f"device events, {ROUNDS} rounds of 20 calls, median (min .. max); {os.path.basename(L.LIB_PATH)}")
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    yy, xx = np.mgrid[0:S, 0:S]
    for name, mask_np in masks() + [("checkerboard", ((yy + xx) % 2 == 0).astype(np.uint8))]:
        mask = torch.from_numpy(mask_np).to(dev)
        label = lambda: ops.scene_objects(mask, connectivity=8, want_object_cls=False)  # noqa: E731
        labels, _, _, _, counts_obj = label()
        call = lambda: ops.scene_outlines(labels, counts_obj, connectivity=8, max_rings=max_rings, max_vertices=max_vertices, ws=ws)  # noqa: E731
        rings, _, counts = call()
        torch.cuda.synchronize()
        found, rows, vfound, vwritten, status = counts.tolist()
        longest = int(rings[:rows, 4].max()) if rows else 0
        med, lo, hi = event_us(call)
        lab = event_us(label)
        print(f"{name:12s}: density {mask_np.mean():.2f}, {int(counts_obj[0])} objects, {found} rings, {vfound} vertices, longest ring "
              f"{longest} edges, status {status}")
        print(f"              outlines {med:8.1f} us ({lo:.1f} .. {hi:.1f})  {S * S / med:7.1f} Mpx/s;  (a) c3d_scene_objects "
              f"{lab[0]:8.1f} us ({lab[1]:.1f} .. {lab[2]:.1f}): the outlines cost {med / lab[0]:.2f} of it")
        if tuned:
            prefix = []
            for k in range(1, 11):
                os.environ["C3D_OUTLINES_PHASES"] = str(k)
                prefix.append(event_us(call)[0])
            del os.environ["C3D_OUTLINES_PHASES"]
            print("              " + "  ".join(f"{p} {t:.1f}" for p, t in zip(PHASES, np.diff([0.0] + prefix))))
        t = []
        for _ in range(5):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            labels.cpu()
            t.append((time.perf_counter() - t0) * 1e6)
        print(f"              (b) host floor: download of the i32 label map alone {np.median(t):10.1f} us (no tracing)")


if __name__ == "__main__":
    main()
