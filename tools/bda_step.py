"""Timed BDA training step (the workload bench.py does not have): update_bda forward, CrossEntropyLoss2d(ignore_index=0) +
BCEDiceLoss, backward, fused Adam at 256 x 256, synthetic input resident on the device, HIP events around `--steps` steps
after `--warmup`; prints one JSON line (img/s, ms per step) and, with --kernels, the per-kernel table of one profiled
step (launches, us per launch, billed TB/s).

    python tools/bda_step.py --batch 12 --steps 20 --warmup 5 --kernels --option C3D_OPT_DW_T4=0
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from change3d_amd import _lib, ops, synthetic as synth  # noqa: E402
from change3d_amd.model.trainer import Trainer  # noqa: E402
from change3d_amd.model.utils import BCEDiceLoss, CrossEntropyLoss2d, FusedAdam, ParamArena, hot_path_named_params  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=12)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--act_dtype", choices=["f32", "bf16"], default="bf16")
    ap.add_argument("--kernels", action="store_true", help="per-kernel table of one profiled step")
    ap.add_argument("--option", action="append", default=[], metavar="NAME=VALUE", help="e.g. C3D_OPT_DW_T4=0")
    a = ap.parse_args()
    for o in a.option:
        name, value = o.split("=")
        ops.set_option(getattr(_lib, name.replace("C3D_", "")), int(value))
    dev = torch.device("cuda:0")
    args = synth.make_args(num_perception_frame=2, size=a.size, dataset="xBD", num_class=5)
    args.act_dtype = torch.bfloat16 if a.act_dtype == "bf16" else torch.float32
    net = Trainer(args)
    net.load_state_dict(synth.synth_state_dict(net, seed=16, mask_margin=0.25))
    net = net.to(dev).train()
    opt = FusedAdam(ParamArena(hot_path_named_params(net), dev), 2e-4, (0.9, 0.99), eps=1e-08, weight_decay=1e-4)
    pre, post, _ = (t.to(dev) for t in synth.synth_batch(a.batch, a.size, seed=0))
    label = synth.synth_bda_labels(a.batch, a.size, seed=0).permute(0, 3, 1, 2).to(dev)
    label_loc, label_cls = label[:, 0].float().unsqueeze(1).contiguous(), torch.prod(label, dim=1).long()
    seg_loss = CrossEntropyLoss2d(ignore_index=0)

    def step():
        pc, pl = net.update_bda(pre, post)
        loss = seg_loss(pc, label_cls) + BCEDiceLoss(pl, label_loc)
        opt.zero_grad()
        loss.backward()
        opt.step()
        return loss

    for _ in range(a.warmup):
        step()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(a.steps):
        loss = step()
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / a.steps
    res = dict(task="bda", batch=a.batch, size=a.size, act_dtype=a.act_dtype, options=a.option, ms_per_step=round(ms, 3),
               img_per_s=round(a.batch / ms * 1e3, 1), loss=float(loss))
    if a.kernels:
        ops.profile_begin(serial=True, detail=True)
        step()
        prof = ops.profile_end()
        rows = sorted(prof.items(), key=lambda kv: -kv[1]["ms_total"])
        print(f"{'kernel':58s} {'n':>4s} {'us/launch':>10s} {'ms':>8s} {'TB/s':>6s}")
        for name, r in rows:
            if r["launches"]:
                tbs = r["bytes_total"] / (r["ms_total"] * 1e-3) / 1e12 if r["ms_total"] > 0 else 0.0
                print(f"{name:58s} {r['launches']:4d} {r['ms_total'] / r['launches'] * 1e3:10.1f} {r['ms_total']:8.3f} {tbs:6.2f}")
        res["serial_kernel_ms"] = round(sum(r["ms_total"] for _, r in rows), 3)
        res["dw_ms"] = {k: round(v["ms_total"], 3) for k, v in prof.items() if "dw333" in k}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
