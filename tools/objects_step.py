"""c3d_scene_objects on the MI355X at 1024 x 1024, 8-connectivity, with a class map (5 classes) and a score, on four masks: blobs
(a thresholded smooth field, what a change map looks like), random at density 0.59 (the percolation threshold: components of
every size), all foreground, and a serpentine (one component, the longest parent chains).  The whole call is timed with
device events around repeated calls after a warm-up, median over several rounds.  With the instrumented library
(`python __graft_entry__.py --tuning`, `C3D_LIB=change3d_amd/lib/libchange3d_hip_tune.so`) the nine launches are also timed
one by one, as differences of prefixes (its knob C3D_OBJECTS_PHASES; the product library has no such switch).  For context,
where scipy is importable: scipy.ndimage.label on the host plus the download of the mask it needs.  Then the share of the
objects in a BDA scene's wall time.  Writes stdout (`python tools/objects_step.py > profiles/scene_objects.txt`)."""
import os
import sys
import time
from types import SimpleNamespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from change3d_amd import _lib as L  # noqa: E402
from change3d_amd import infer, ops  # noqa: E402

S, TILE, N_CLS = 1024, 256, 5
ROUNDS = 5
PHASES = ("memsets+local", "seam", "flatten+area", "count", "scan", "number", "relabel+stats", "finalise", "paint")


def event_us(fn, reps=20, warm=3):
    for _ in range(warm):
        fn()
    out = []
    for _ in range(ROUNDS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / reps * 1e3)
    return float(np.median(out)), min(out), max(out)


def masks():
    rng = np.random.default_rng(0)
    field = rng.standard_normal((S // 16, S // 16)).astype(np.float32)
    field = torch.nn.functional.interpolate(torch.from_numpy(field)[None, None], size=(S, S), mode="bicubic")[0, 0].numpy()
    yy, xx = np.mgrid[0:S, 0:S]
    snake = (yy % 2 == 0) | ((yy % 4 == 1) & (xx == S - 1)) | ((yy % 4 == 3) & (xx == 0))
    return [("blobs", (field > 0.8).astype(np.uint8)), ("random 0.59", (rng.random((S, S)) < 0.59).astype(np.uint8)),
            ("foreground", np.ones((S, S), np.uint8)), ("serpentine", snake.astype(np.uint8))]


def main():
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(1)
    cls = torch.from_numpy(rng.integers(0, N_CLS, size=(S, S), dtype=np.uint8)).to(dev)
    score = torch.from_numpy(rng.random((S, S), dtype=np.float32)).to(dev)
    tuned = "tune" in os.path.basename(L.LIB_PATH)
    print(f"# tools/objects_step.py: {S} x {S}, 8-connectivity, {N_CLS} classes, score; device events, {ROUNDS} rounds, median (min .. max); "
          f"{os.path.basename(L.LIB_PATH)}")
    try:
        from scipy import ndimage
    except ImportError:
        ndimage = None
    for name, mask_np in masks():
        mask = torch.from_numpy(mask_np).to(dev)
        call = lambda: ops.scene_objects(mask, cls, score, connectivity=8, n_cls=N_CLS)  # noqa: E731
        counts = call()[4]
        torch.cuda.synchronize()
        found = int(counts[0])
        med, lo, hi = event_us(call)
        print(f"{name:12s}: density {mask_np.mean():.2f}, {found} objects: {med:8.1f} us ({lo:.1f} .. {hi:.1f})  "
              f"{S * S / med:7.1f} Mpx/s")
        if tuned:
            prefix = []
            for k in range(1, 10):
                os.environ["C3D_OBJECTS_PHASES"] = str(k)
                prefix.append(event_us(call)[0])
            del os.environ["C3D_OBJECTS_PHASES"]
            print("              " + "  ".join(f"{p} {t:.1f}" for p, t in zip(PHASES, np.diff([0.0] + prefix))))
        if ndimage is not None:
            t = []
            for _ in range(3):
                t0 = time.perf_counter()
                host = mask.cpu().numpy()
                ndimage.label(host, structure=np.ones((3, 3), dtype=int))
                t.append((time.perf_counter() - t0) * 1e6)
            print(f"              host: download + scipy.ndimage.label {np.median(t):8.1f} us (labels only: no table, no votes)")

    # a BDA scene end to end, with and without the objects
    from change3d_amd.model.trainer import Trainer
    args = SimpleNamespace(dataset="xBD", in_height=TILE, in_width=TILE, num_perception_frame=2, num_class=N_CLS, pretrained="",
                           act_dtype=torch.bfloat16)
    torch.manual_seed(16)
    net = Trainer(args).to(dev).eval()
    scene = torch.from_numpy(rng.integers(0, 256, size=(S, S, 6), dtype=np.uint8)).to(dev)
    inf = infer.SceneInferencer(net, "bda", stride=128, batch=32)

    def timed(fn, reps=3):
        fn()
        torch.cuda.synchronize()
        out = []
        for _ in range(ROUNDS):
            t0 = time.perf_counter()
            for _ in range(reps):
                fn()
            torch.cuda.synchronize()
            out.append((time.perf_counter() - t0) / reps)
        return float(np.median(out)), min(out), max(out)

    plain, with_objects = timed(lambda: inf.predict(scene)), timed(lambda: inf.predict(scene, objects=True))
    found = int(inf.predict(scene, objects=True)[-1].counts[0])
    print(f"BDA bf16 stride 128: scene -> maps {plain[0] * 1e3:7.2f} ms ({plain[1] * 1e3:.2f} .. {plain[2] * 1e3:.2f});  with objects "
          f"{with_objects[0] * 1e3:7.2f} ms ({with_objects[1] * 1e3:.2f} .. {with_objects[2] * 1e3:.2f}), {found} objects: "
          f"{(with_objects[0] / plain[0] - 1) * 100:5.1f} % on top")


if __name__ == "__main__":
    main()
