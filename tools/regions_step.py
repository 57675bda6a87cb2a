"""c3d_scene_regions and c3d_regions_sieve on the MI355X at 1024 x 1024, both connectivities, on the masks of
tools/objects_step.py (blobs, noise at 0.59, all foreground, serpentine), each as 0 / 1 keys and with 7 classes painted over it
in 64-pixel blocks, and on a 7-class iid noise map.  c3d_scene_regions is timed next to c3d_scene_objects on the same map
binarised, in the same run: that call is the yardstick (no class map, no score, no painted map on either side).
c3d_regions_sieve is timed at min_area 16 and 64 next to the regions call it contains, with the rounds it used, the regions it
moved, its table entries and the cost of a round that returns at once (the difference between 16 and 8 rounds launched ahead).
Device events around repeated calls after a warm-up, median over several rounds (tools/objects_step.py event_us).  For
context, where scipy is importable: the download plus scipy.ndimage.label per key on the host, and the restatement's sieve
(tests/sieve_reference.py) on two of the maps.  Then a per-kernel ranking of one sieve call from torch's profiler.  Writes stdout
(`python tools/regions_step.py > profiles/scene_regions.txt`)."""
import os
import re
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import sieve_reference as SR  # noqa: E402
from change3d_amd import _lib as L  # noqa: E402
from change3d_amd import ops  # noqa: E402
from objects_step import ROUNDS, S, event_us, masks  # noqa: E402

CLASSES, BLOCK = 7, 64
SIEVES = (16, 64)
MAX_ROUNDS = 8
HOST_SIEVE = ("blobs x 7 classes", "iid 7 classes")       # the maps the restatement's sieve is timed on (plain Python: seconds)


def key_maps():
    rng = np.random.default_rng(2)
    blocks = np.kron(rng.integers(1, CLASSES + 1, size=(S // BLOCK, S // BLOCK), dtype=np.uint8), np.ones((BLOCK, BLOCK), np.uint8))
    out = []
    for name, mask in masks():
        out.append((name + " 0/1", mask))
        out.append((name + f" x {CLASSES} classes", mask * blocks))
    out.append((f"iid {CLASSES} classes", rng.integers(0, CLASSES, size=(S, S), dtype=np.uint8)))
    return out


def main():
    if not torch.cuda.is_available():
        raise SystemExit("tools/regions_step.py measures on the GPU; there is none here")
    dev = torch.device("cuda:0")
    max_objects = S * S
    nbytes, cap = ops.regions_sieve_plan(S, S)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    ws_r = torch.empty(L.lib().c3d_scene_regions_ws_bytes(S, S), dtype=torch.uint8, device=dev)
    print(f"# tools/regions_step.py: {S} x {S}, max_objects = {max_objects}, sieve max_rounds = {MAX_ROUNDS}, table capacity {cap} slots, "
          f"sieve workspace {nbytes / 2**20:.1f} MiB; device events, {ROUNDS} rounds of 10 calls, median (min .. max); "
          f"{os.path.basename(L.LIB_PATH)}", flush=True)
    try:
        from scipy import ndimage
    except ImportError:
        ndimage = None
    profiled = None
    for name, key_np in key_maps():
        key = torch.from_numpy(np.ascontiguousarray(key_np)).to(dev)
        binary = (key > 0).to(torch.uint8)
        for connectivity in (8, 4):
            objects_call = lambda: ops.scene_objects(binary, connectivity=connectivity, max_objects=max_objects, want_object_cls=False)  # noqa: E731
            regions_call = lambda: ops.scene_regions(key, connectivity=connectivity, max_objects=max_objects, want_object_key=False,  # noqa: E731
                                                     ws=ws_r)
            n_obj, n_reg = int(objects_call()[4][0]), int(regions_call()[4][0])
            torch.cuda.synchronize()
            t_obj, t_reg = event_us(objects_call, reps=10, warm=2), event_us(regions_call, reps=10, warm=2)
            print(f"{name:28s} conn {connectivity}: objects of the mask {n_obj:7d} in {t_obj[0]:8.1f} us ({t_obj[1]:.1f} .. {t_obj[2]:.1f});  "
                  f"regions {n_reg:7d} in {t_reg[0]:8.1f} us ({t_reg[1]:.1f} .. {t_reg[2]:.1f}) = {t_reg[0] / t_obj[0]:.2f} of it", flush=True)
            for min_area in SIEVES:
                sieve_call = lambda r=MAX_ROUNDS, a=min_area, c=connectivity: ops.regions_sieve(key, a, connectivity=c, max_rounds=r,  # noqa: E731
                                                                    max_objects=max_objects, ws=ws)
                out = sieve_call()
                torch.cuda.synchronize()
                info, left = out[5].tolist(), int(out[4][0])
                t_s = event_us(sieve_call, reps=10, warm=2)
                t_more = event_us(lambda: sieve_call(2 * MAX_ROUNDS), reps=10, warm=2)
                print(f"    sieve {min_area:3d}: {t_s[0]:9.1f} us ({t_s[1]:.1f} .. {t_s[2]:.1f}) = {t_s[0] / t_reg[0]:.2f} of the regions call;  status "
                      f"{info[0]}, rounds {info[1]}, regions {info[5]} -> {left}, moved {info[2]}, pixels {info[3]}, small left {info[4]}, most table "
                      f"entries {info[6]};  a round that returns at once {(t_more[0] - t_s[0]) / MAX_ROUNDS:.1f} us", flush=True)
                if name.startswith("iid") and connectivity == 8 and min_area == SIEVES[0]:
                    profiled = (name, sieve_call)
            if connectivity != 8:
                continue
            t = []
            for _ in range(3):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                host = key.cpu().numpy()
                t.append((time.perf_counter() - t0) * 1e6)
            line = f"    on the host: download {np.median(t):8.1f} us"
            if ndimage is not None:
                t0 = time.perf_counter()
                for k in np.unique(host[host > 0]):
                    ndimage.label(host == k, structure=np.ones((3, 3), dtype=int))
                line += f" + scipy.ndimage.label per key {(time.perf_counter() - t0) * 1e3:8.1f} ms (labels only: no numbering over all keys, no table)"
            if name in HOST_SIEVE:
                t0 = time.perf_counter()
                ref = SR.sieve(host, SIEVES[0], 8, max_rounds=MAX_ROUNDS)
                line += f"; the restatement's sieve at {SIEVES[0]}: {time.perf_counter() - t0:6.1f} s, {int(ref['info'][1])} rounds"
            print(line, flush=True)

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
        rows = [(e.key, e.count, getattr(e, "device_time_total", None) or getattr(e, "cuda_time_total", 0.0)) for e in prof.key_averages()]
        print(f"per kernel, {name}, conn 8, sieve {SIEVES[0]}, {n} calls of {MAX_ROUNDS} + 1 rounds launched ahead (torch profiler; the launches "
              f"of the rounds after the last one return at once and are in the averages):")
        for key_, count, total in sorted(rows, key=lambda r: -r[2]):
            found = re.search(r"(\w+_kernel)|(Mem\w+ \(\w+.*?\))", key_)
            print(f"  {found.group(0) if found else key_[:40]:34s} {count:5d} launches {total / max(count, 1):9.1f} us each {total / n:10.1f} us per call")
    except Exception as e:                                   # the profiler is a convenience: the totals above stand without it
        print(f"per kernel: torch's profiler is not available here ({type(e).__name__}: {e})")


if __name__ == "__main__":
    main()
