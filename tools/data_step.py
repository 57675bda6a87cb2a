"""Input-pipeline numbers for B = 32 at 256 x 256 on the MI355X: the c3d_augment_gather kernel (crop on all / half / none
of the samples) next to c3d_bcd_preprocess, the DeviceAugmentLoader alone, and the BCD bf16 train step fed by the loader
against the synthetic loader.  Device events around repeated launches; writes nothing but stdout
(`python tools/data_step.py > profiles/data_step.txt`)."""
import os
import sys
import time
from types import SimpleNamespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from change3d_amd import _lib as L, ops  # noqa: E402
from change3d_amd.data.resident import DeviceAugmentLoader, ResidentStore  # noqa: E402
from change3d_amd.data.transforms import BCDTransforms as T, crop_area_of, draw_augmentation_table  # noqa: E402

B, S, N = 32, 256, 1024


def event_ms(fn, reps=200, warm=20):
    for _ in range(warm):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    images = torch.from_numpy(rng.integers(0, 256, size=(N, S, S, 6), dtype=np.uint8))
    labels = torch.from_numpy((rng.integers(0, 2, size=(N, S, S)) * 255).astype(np.uint8))
    store = ResidentStore(images, labels, dev)
    mean, std = torch.tensor(T.DEFAULT_MEAN, device=dev), torch.tensor(T.DEFAULT_STD, device=dev)
    pre, post = torch.empty((B, 3, S, S), device=dev), torch.empty((B, 3, S, S), device=dev)
    lab = torch.empty((B, 1, S, S), device=dev)
    flags = torch.from_numpy((rng.random((B, 3)) < 0.5).astype(np.uint8)).to(dev)
    nbytes = B * S * S * 35
    t_plain = event_ms(lambda: ops.bcd_preprocess(store.images[:B], store.labels[:B], flags, mean, std, pre, post, lab, B, S, S))
    print(f"c3d_bcd_preprocess            B={B} {S}x{S}: {t_plain * 1e3:8.1f} us  {nbytes / t_plain / 1e6:7.1f} GB/s")
    for name, p in (("crop on all", 1.0), ("crop on half", 0.5), ("crop on none", 0.0)):
        tab = draw_augmentation_table(rng.permutation(N)[:B], rng, crop_area_of(S))
        tab[:, 1] = rng.random(B) < p
        tab[:, 2:4] = rng.integers(0, crop_area_of(S) + 1, size=(B, 2)) * tab[:, 1:2]
        dt = torch.from_numpy(tab).to(dev)
        t = event_ms(lambda: ops.augment_gather(store.images, store.labels, dt, mean, std, pre, post, lab, None, None, L.AUG_BCD,
                                                N, S, S, B, S, S))
        print(f"c3d_augment_gather {name:12s} B={B} {S}x{S}: {t * 1e3:8.1f} us  {nbytes / t / 1e6:7.1f} GB/s  {t / t_plain:.2f} x plain")

    loader = DeviceAugmentLoader(store, B, "bcd", True, seed=16)
    for _ in range(2):
        t0 = time.time()
        n = 0
        for img, target in loader:
            n += img.shape[0]
        torch.cuda.synchronize()
        dt_loader = time.time() - t0
    print(f"DeviceAugmentLoader alone (gather + chain + cat): {n / dt_loader:9.0f} img/s over {n} samples")

    # BCD bf16 train step, B = 32: synthetic-fed (one resident batch, as bench.py) against loader-fed
    from change3d_amd.model.trainer import Trainer
    from change3d_amd.model.utils import BCEDiceLoss, FusedAdam, ParamArena, hot_path_named_params
    args = SimpleNamespace(dataset="LEVIR-CD", in_height=S, in_width=S, num_perception_frame=1, num_class=1, pretrained="",
                           act_dtype=torch.bfloat16)
    torch.manual_seed(16)
    net = Trainer(args).to(dev).train()
    opt = FusedAdam(ParamArena(hot_path_named_params(net), dev), 2e-4, (0.9, 0.99), eps=1e-8, weight_decay=1e-4)

    def step(img, target):
        out = net.update_bcd(img[:, 0:3], img[:, 3:6])
        loss = BCEDiceLoss(out, target)
        opt.zero_grad()
        loss.backward()
        opt.step()

    fixed = next(iter(loader))

    def run(feed, steps):
        it = iter(feed())
        for _ in range(5):
            step(*next(it))
        torch.cuda.synchronize()
        t0 = time.time()
        for _ in range(steps):
            step(*next(it))
        torch.cuda.synchronize()
        return B * steps / (time.time() - t0)

    def synthetic():
        while True:
            yield fixed

    def from_loader():
        while True:
            for batch in loader:
                if batch[0].shape[0] == B:
                    yield batch

    rates = {"synthetic": [], "loader": []}
    for _ in range(3):                                   # alternate, so that drift hits both alike
        rates["synthetic"].append(run(synthetic, 40))
        rates["loader"].append(run(from_loader, 40))
    s, l = np.median(rates["synthetic"]), np.median(rates["loader"])
    print(f"BCD bf16 train step B={B}: resident batch {s:7.1f} img/s {['%.1f' % v for v in rates['synthetic']]}")
    print(f"BCD bf16 train step B={B}: loader-fed     {l:7.1f} img/s {['%.1f' % v for v in rates['loader']]}  ({(l / s - 1) * 100:+.2f} %)")


if __name__ == "__main__":
    main()
