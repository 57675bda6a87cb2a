"""Whole-scene inference numbers on the MI355X for a synthetic 1024 x 1024 pair at t = 256, strides 256 and 128, bf16 and
f32: scene -> mask end to end (Mpx/s), the share of that time spent outside the forward, c3d_scene_gather and
c3d_scene_stitch alone (us, effective GB/s against the bytes they must move), and the same gather and stitch restated with
plain torch device ops (pad, unfold, index_add_) as the comparison.  Device events around repeated launches after a warm-up,
median and spread over several rounds; writes nothing but stdout
(`python tools/scene_step.py >> profiles/scene_infer.txt`)."""
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

S, TILE = 1024, 256
ROUNDS = 5


def event_us(fn, reps=50, warm=10):
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


def torch_gather(scene, py, px, mean, std):
    """pad (reflect) + unfold + normalise with torch device ops: [n, 6, t, t] f32."""
    img = scene.permute(2, 0, 1).float()[None]
    bottom, right = (py.n - 1) * py.stride - py.margin + py.tile - py.extent, (px.n - 1) * px.stride - px.margin + px.tile - px.extent
    img = torch.nn.functional.pad(img, (px.margin, right, py.margin, bottom), mode="reflect")
    tiles = img.unfold(2, py.tile, py.stride).unfold(3, px.tile, px.stride)          # [1, 6, ny, nx, t, t]
    tiles = tiles[0].permute(1, 2, 0, 3, 4).reshape(py.n * px.n, 6, py.tile, px.tile)
    return ((tiles / 255.0) - mean.view(1, 6, 1, 1)) / std.view(1, 6, 1, 1)


def torch_stitch(tiles, py, px, w2, index, canvas_shape):
    """weighted tiles added into a padded canvas with index_add_, divided by the summed weights, cropped, thresholded."""
    num = torch.zeros(canvas_shape[0] * canvas_shape[1], device=tiles.device)
    den = torch.zeros_like(num)
    num.index_add_(0, index, (tiles * w2).reshape(-1))
    den.index_add_(0, index, w2.expand_as(tiles).reshape(-1))
    blend = (num / den).view(canvas_shape)[py.margin:py.margin + py.extent, px.margin:px.margin + px.extent]
    return blend, (blend > 0.5).to(torch.uint8)


def main():
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    scene = torch.from_numpy(rng.integers(0, 256, size=(S, S, 6), dtype=np.uint8)).to(dev)
    mean, std = torch.tensor(T.DEFAULT_MEAN, device=dev), torch.tensor(T.DEFAULT_STD, device=dev)
    print(f"# tools/scene_step.py: {S} x {S} scene, tile {TILE}, hann window; device events, {ROUNDS} rounds, median (min .. max)")
    for stride in (256, 128):
        py, px = infer.axis_plan(S, TILE, stride), infer.axis_plan(S, TILE, stride)
        n = py.n * px.n
        origins = torch.from_numpy(np.stack([np.repeat(py.starts, px.n), np.tile(px.starts, py.n)], axis=1).astype(np.int32)).to(dev)
        pre, post = torch.empty((n, 3, TILE, TILE), device=dev), torch.empty((n, 3, TILE, TILE), device=dev)
        g_bytes = n * TILE * TILE * 30
        med, lo, hi = event_us(lambda: ops.scene_gather(scene, origins, mean, std, pre, post, S, S, n, TILE, TILE))
        print(f"stride {stride}: c3d_scene_gather  {n:3d} tiles: {med:8.1f} us ({lo:.1f} .. {hi:.1f})  {g_bytes / med / 1e3:7.1f} GB/s "
              f"of {g_bytes / 1e6:.1f} MB")
        tg = event_us(lambda: torch_gather(scene, py, px, mean, std), reps=20, warm=5)
        print(f"stride {stride}: torch pad + unfold + normalise : {tg[0]:8.1f} us ({tg[1]:.1f} .. {tg[2]:.1f})  {tg[0] / med:.2f} x the kernel")

        st = infer.SceneStitcher(py, px, 1, "hann", dev, blend=True)
        tiles = torch.rand((py.n, px.n, 1, TILE, TILE), device=dev)

        def stitch_all():
            for row in range(py.n):
                st.put(row, 0, tiles[row])
                st.stitch(row)

        def stitch_only():                      # the ring holds the last k rows: the same launches, without the copies
            for row in range(py.n):
                st.stitch(row)

        taps = py.k * px.k
        s_bytes = S * S * (taps * 4 + 4 + 1)    # every covering tile pixel read once, f32 blend and u8 mask written
        med_s, lo_s, hi_s = event_us(stitch_only)
        med_c = event_us(stitch_all)[0]
        print(f"stride {stride}: c3d_scene_stitch  {py.n} strips, {taps} taps: {med_s:8.1f} us ({lo_s:.1f} .. {hi_s:.1f})  "
              f"{s_bytes / med_s / 1e3:7.1f} GB/s of {s_bytes / 1e6:.1f} MB   (with the ring copies: {med_c:.1f} us)")
        Hc, Wc = (py.n - 1) * stride + TILE, (px.n - 1) * stride + TILE
        yy = (torch.arange(py.n, device=dev) * stride).view(-1, 1, 1, 1) + torch.arange(TILE, device=dev).view(1, 1, -1, 1)
        xx = (torch.arange(px.n, device=dev) * stride).view(1, -1, 1, 1) + torch.arange(TILE, device=dev).view(1, 1, 1, -1)
        index = (yy * Wc + xx).reshape(-1)
        w2 = (st.wy.view(-1, 1) * st.wx.view(1, -1)).view(1, 1, TILE, TILE)
        flat_tiles = tiles[:, :, 0]
        blend_t, mask_t = torch_stitch(flat_tiles, py, px, w2, index, (Hc, Wc))
        stitch_all()
        torch.cuda.synchronize()
        print(f"stride {stride}: torch restatement agrees with the kernel to {float((blend_t - st.blend[0]).abs().max()):.2e}")
        ts = event_us(lambda: torch_stitch(flat_tiles, py, px, w2, index, (Hc, Wc)), reps=20, warm=5)
        print(f"stride {stride}: torch index_add_ + divide + crop: {ts[0]:8.1f} us ({ts[1]:.1f} .. {ts[2]:.1f})  {ts[0] / med_s:.2f} x the kernel")

    # end to end: scene (already on the device) -> mask, and the forward alone over the same tiles
    from change3d_amd.model.trainer import Trainer
    for act, name in ((torch.bfloat16, "bf16"), (torch.float32, "f32")):
        args = SimpleNamespace(dataset="LEVIR-CD", in_height=TILE, in_width=TILE, num_perception_frame=1, num_class=1, pretrained="",
                               act_dtype=act)
        torch.manual_seed(16)
        net = Trainer(args).to(dev).eval()
        for stride in (256, 128):
            inf = infer.SceneInferencer(net, "bcd", stride=stride, batch=32)
            n = (-(-S // stride)) ** 2
            pre, post = torch.randn((min(n, 32), 3, TILE, TILE), device=dev), torch.randn((min(n, 32), 3, TILE, TILE), device=dev)

            def forward_only():
                with torch.no_grad():
                    for j in range(0, n, 32):
                        b = min(32, n - j)
                        net.update_bcd(pre[:b], post[:b])

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

            e2e, fwd = timed(lambda: inf.predict(scene), 4), timed(forward_only, 4)
            print(f"{name} stride {stride}: scene -> mask {e2e[0] * 1e3:7.2f} ms ({e2e[1] * 1e3:.2f} .. {e2e[2] * 1e3:.2f})  "
                  f"{S * S / e2e[0] / 1e6:7.2f} Mpx/s  {n} tiles;  forward alone {fwd[0] * 1e3:7.2f} ms ({n / fwd[0]:.0f} tiles/s);  "
                  f"outside the forward {(1 - fwd[0] / e2e[0]) * 100:5.1f} %")


if __name__ == "__main__":
    main()
