"""c3d_objects_match on the MI355X at 1024 x 1024, 8-connectivity, on the four masks of tools/objects_step.py (blobs, random at
density 0.59, all foreground, serpentine) as prediction against the same mask shifted by (2, 3) pixels as ground truth.  The
match call is timed with device events around repeated calls after a warm-up, median over several rounds, in one process,
next to two yardsticks taken in the same run on the same masks: (a) c3d_scene_objects, the labelling the join follows, and
(b) the host way, the download of both label maps plus `np.unique` over the pair keys.  With the instrumented library
(`python __graft_entry__.py --tuning`, `C3D_LIB=change3d_amd/lib/libchange3d_hip_tune.so`) the memset and the four launches
are also timed one by one, as differences of prefixes (its knob C3D_MATCH_PHASES), the pixel pass with and without its
per-workgroup LDS stage (C3D_MATCH_LDS) and with other spans of a workgroup (C3D_MATCH_SPAN); the product library has no such
switches.  Writes stdout (`python tools/objects_match_step.py > profiles/objects_match.txt`)."""
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
from objects_step import N_CLS, ROUNDS, S, event_us, masks  # noqa: E402

SHIFT = (2, 3)
PHASES = ("memset", "init", "pair_count", "slots", "finalise")


def shifted(mask):
    out = np.zeros_like(mask)
    out[SHIFT[0]:, SHIFT[1]:] = mask[:-SHIFT[0], :-SHIFT[1]]
    return out


def knob(fn, **knobs):
    """Median time of `fn` with the instrumented library's knobs set."""
    for name, value in knobs.items():
        os.environ[name] = str(value)
    try:
        return event_us(fn)[0]
    finally:
        for name in knobs:
            del os.environ[name]


def main():
    if not torch.cuda.is_available():
        raise SystemExit("tools/objects_match_step.py measures on the GPU; there is none here")
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(1)
    cls = torch.from_numpy(rng.integers(0, N_CLS, size=(S, S), dtype=np.uint8)).to(dev)
    tuned = "tune" in os.path.basename(L.LIB_PATH)
    nbytes, cap = ops.objects_match_plan(S, S)
    print(f"# tools/objects_match_step.py: {S} x {S}, 8-connectivity, {N_CLS} classes, ground truth = prediction shifted by {SHIFT}; "
          f"pair table {cap} slots, workspace {nbytes / 2**20:.1f} MiB; device events, {ROUNDS} rounds of 20 calls, median "
          f"(min .. max); {os.path.basename(L.LIB_PATH)}")
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    for name, mask_np in masks():
        label = lambda m: ops.scene_objects(m, cls, None, connectivity=8, n_cls=N_CLS, want_hist=False, want_object_cls=False)  # noqa: E731
        mask_p, mask_g = torch.from_numpy(mask_np).to(dev), torch.from_numpy(shifted(mask_np)).to(dev)
        a, b = label(mask_p), label(mask_g)
        pa, pb = (a[0], a[1], a[4]), (b[0], b[1], b[4])
        call = lambda: ops.objects_match(*pa, *pb, n_cls=N_CLS, ws=ws)  # noqa: E731
        counts = call()[3]
        torch.cuda.synchronize()
        pairs, tp, fp, fn, status = counts.tolist()[:5]
        med, lo, hi = event_us(call)
        lab = event_us(lambda: label(mask_p))
        print(f"{name:12s}: density {mask_np.mean():.2f}, {int(a[4][0])} x {int(b[4][0])} objects, {pairs} pairs, tp {tp} fp {fp} fn {fn}, "
              f"status {status}")
        print(f"              match {med:8.1f} us ({lo:.1f} .. {hi:.1f})  {S * S / med:7.1f} Mpx/s;  (a) c3d_scene_objects on the prediction "
              f"{lab[0]:8.1f} us ({lab[1]:.1f} .. {lab[2]:.1f}): the match costs {med / lab[0]:.2f} of it")
        small = ops.objects_match_plan(S, S, 1 << 16)
        ws_small = ws[:small[0]]
        call_small = lambda: ops.objects_match(*pa, *pb, n_cls=N_CLS, table_capacity=small[1], ws=ws_small)  # noqa: E731
        st = int(call_small()[3][4])
        ms = event_us(call_small)
        print(f"              match with a table of {small[1]} slots (status {st}) {ms[0]:8.1f} us ({ms[1]:.1f} .. {ms[2]:.1f})")
        if tuned:
            prefix = [knob(call, C3D_MATCH_PHASES=k) for k in range(5)]
            print("              " + "  ".join(f"{p} {t:.1f}" for p, t in zip(PHASES, np.diff([0.0] + prefix))))
            off = knob(call, C3D_MATCH_LDS=0), knob(call, C3D_MATCH_LDS=0, C3D_MATCH_PHASES=2)
            print(f"              without the LDS stage: match {off[0]:.1f} us, memset + init + pair_count {off[1]:.1f} us "
                  f"(with it {prefix[2]:.1f} us)")
            spans = [(s, knob(call, C3D_MATCH_SPAN=s)) for s in (1, 2, 4, 8, 16)]
            print("              chunks of 256 pixels per wave: " + "  ".join(f"{s}: {t:.1f} us" for s, t in spans))
        t = []
        for _ in range(3):
            t0 = time.perf_counter()
            lp, lg = a[0].cpu().numpy().astype(np.int64), b[0].cpu().numpy().astype(np.int64)
            both = (lp > 0) & (lg > 0)
            keys, inter = np.unique((lp[both] << 32) | lg[both], return_counts=True)
            t.append((time.perf_counter() - t0) * 1e6)
        assert len(keys) == pairs or status
        print(f"              (b) host: download of both label maps + np.unique over the pair keys {np.median(t):10.1f} us "
              f"(pair counts only: no rows, no confusion matrix)")


if __name__ == "__main__":
    main()
