"""Test-time augmentation numbers on the MI355X for a synthetic 1024 x 1024 pair at t = 256, strides 256 and 128:
c3d_scene_gather_views at `flips` and `d4` next to c3d_scene_gather followed by torch's flip / transpose / contiguous producing
the same tensor (asserted equal), c3d_scene_fold_views into the stitch ring next to torch's inverse views + stack + mean + the
ring copy, and scene -> mask in bf16 at tta none / flips / d4 with 32 model inputs per forward throughout, with the share of
the time spent outside the forward.  Device events around repeated launches after a warm-up, median and spread over several
rounds; writes nothing but stdout (`python tools/tta_step.py >> profiles/scene_tta.txt`)."""
import os
import sys
import time
from types import SimpleNamespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from change3d_amd import infer, ops  # noqa: E402
from change3d_amd.data.transforms import BCDTransforms as T  # noqa: E402

S, TILE, BATCH = 1024, 256, 32
ROUNDS = 5


def event_us(fn, reps=20, warm=5):
    """Median and (min, max) over ROUNDS rounds of `reps` back-to-back calls, in microseconds per call."""
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


def torch_view(x, v, inverse=False):
    """View `v` (or its inverse) of the last two axes with torch device ops; a strided view until someone makes it contiguous."""
    if inverse:
        x = x.flip(-1) if v & 1 else x
        x = x.flip(-2) if v & 2 else x
        return x.transpose(-2, -1) if v & 4 else x
    x = x.transpose(-2, -1) if v & 4 else x
    x = x.flip(-2) if v & 2 else x
    return x.flip(-1) if v & 1 else x


def main():
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    scene = torch.from_numpy(rng.integers(0, 256, size=(S, S, 6), dtype=np.uint8)).to(dev)
    mean, std = torch.tensor(T.DEFAULT_MEAN, device=dev), torch.tensor(T.DEFAULT_STD, device=dev)
    print(f"# tools/tta_step.py: {S} x {S} scene, tile {TILE}; device events, {ROUNDS} rounds, median (min .. max)")
    for stride in (256, 128):
        py, px = infer.axis_plan(S, TILE, stride), infer.axis_plan(S, TILE, stride)
        n = py.n * px.n
        origins = torch.from_numpy(np.stack([np.repeat(py.starts, px.n), np.tile(px.starts, py.n)], axis=1).astype(np.int32)).to(dev)
        pre1, post1 = torch.empty((n, 3, TILE, TILE), device=dev), torch.empty((n, 3, TILE, TILE), device=dev)
        plain = event_us(lambda: ops.scene_gather(scene, origins, mean, std, pre1, post1, S, S, n, TILE, TILE))
        print(f"stride {stride}: c3d_scene_gather        {n:3d} tiles          : {plain[0]:8.1f} us ({plain[1]:.1f} .. {plain[2]:.1f})")
        for name in ("flips", "d4", "transposing (4..7)"):
            codes = infer.VIEW_SETS.get(name, (4, 5, 6, 7))
            mask, nv = infer.view_mask(codes), len(codes)
            pre, post = torch.empty((n * nv, 3, TILE, TILE), device=dev), torch.empty((n * nv, 3, TILE, TILE), device=dev)
            g_bytes = n * TILE * TILE * (6 + 24 * nv)

            def composed():
                ops.scene_gather(scene, origins, mean, std, pre1, post1, S, S, n, TILE, TILE)
                return [torch.stack([torch_view(x, v) for v in codes], dim=1).reshape(n * nv, 3, TILE, TILE) for x in (pre1, post1)]

            ops.scene_gather_views(scene, origins, mean, std, pre, post, S, S, n, TILE, TILE, mask)
            want = composed()
            assert torch.equal(pre, want[0]) and torch.equal(post, want[1]), name
            del want
            med, lo, hi = event_us(lambda: ops.scene_gather_views(scene, origins, mean, std, pre, post, S, S, n, TILE, TILE, mask))
            tc = event_us(composed)
            print(f"stride {stride}: c3d_scene_gather_views {n:3d} tiles x {nv} views, {name:18s}: {med:8.1f} us ({lo:.1f} .. {hi:.1f})  "
                  f"{g_bytes / med / 1e3:7.1f} GB/s of {g_bytes / 1e6:.1f} MB;  gather + torch flip/transpose/stack: {tc[0]:8.1f} us "
                  f"({tc[1]:.1f} .. {tc[2]:.1f})  {tc[0] / med:.2f} x the kernel  (equal: yes)")
            del pre, post

        for C in (1, 7):
            st = infer.SceneStitcher(py, px, C, "hann", dev, blend=False)
            for name in ("flips", "d4", "transposing (4..7)"):
                codes = infer.VIEW_SETS.get(name, (4, 5, 6, 7))
                mask, nv = infer.view_mask(codes), len(codes)
                values = torch.randn((py.n, px.n * nv, C, TILE, TILE), device=dev)
                f_bytes = n * C * TILE * TILE * 4 * (nv + 1)

                def fold_all():
                    for row in range(py.n):
                        st.fold(row, 0, values[row], mask)

                def torch_all():
                    for row in range(py.n):
                        v = values[row].view(px.n, nv, C, TILE, TILE)
                        st.put(row, 0, torch.stack([torch_view(v[:, j], c, inverse=True) for j, c in enumerate(codes)]).mean(dim=0))

                fold_all()
                got = st.ring.clone()
                torch_all()
                diff = float((got - st.ring).abs().max())
                med, lo, hi = event_us(fold_all)
                tf = event_us(torch_all)
                print(f"stride {stride}: c3d_scene_fold_views C={C} {py.n} rows x {px.n} tiles x {nv} views, {name:18s}: {med:8.1f} us "
                      f"({lo:.1f} .. {hi:.1f})  {f_bytes / med / 1e3:7.1f} GB/s of {f_bytes / 1e6:.1f} MB;  torch inverse views + stack + "
                      f"mean + ring copy: {tf[0]:8.1f} us ({tf[1]:.1f} .. {tf[2]:.1f})  {tf[0] / med:.2f} x the kernel  (max |diff| {diff:.1e})")
                del values

    # end to end: scene (already on the device) -> mask, and the forward alone over the same number of model inputs
    from change3d_amd.model.trainer import Trainer
    args = SimpleNamespace(dataset="LEVIR-CD", in_height=TILE, in_width=TILE, num_perception_frame=1, num_class=1, pretrained="",
                           act_dtype=torch.bfloat16)
    torch.manual_seed(16)
    net = Trainer(args).to(dev).eval()
    pre, post = torch.randn((BATCH, 3, TILE, TILE), device=dev), torch.randn((BATCH, 3, TILE, TILE), device=dev)

    def timed(fn, reps):
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

    for stride in (256, 128):
        n = (-(-S // stride)) ** 2
        base = None
        for tta in (None, "flips", "d4"):
            nv = 1 if tta is None else len(infer.VIEW_SETS[tta])
            inf = infer.SceneInferencer(net, "bcd", stride=stride, batch=BATCH, tta=tta)
            tiles = BATCH // nv                                           # tiles per forward, as predict splits the scene

            def forward_only():
                with torch.no_grad():
                    for j in range(0, n, tiles):
                        b = min(tiles, n - j) * nv
                        net.update_bcd(pre[:b], post[:b])

            reps = 4 if nv == 1 else 2
            e2e, fwd = timed(lambda: inf.predict(scene), reps), timed(forward_only, reps)
            base = base or e2e[0]
            print(f"bf16 stride {stride} tta {str(tta):5s}: scene -> mask {e2e[0] * 1e3:7.2f} ms ({e2e[1] * 1e3:.2f} .. {e2e[2] * 1e3:.2f})  "
                  f"{e2e[0] / base:5.2f} x tta None  {n} tiles x {nv} views;  forward alone {fwd[0] * 1e3:7.2f} ms "
                  f"({n * nv / fwd[0]:.0f} inputs/s);  outside the forward {(1 - fwd[0] / e2e[0]) * 100:5.1f} %")


if __name__ == "__main__":
    main()
