"""Change maps of whole scenes: `python -m change3d_amd.scripts.predict_scene --task BCD --weights best_model.pth
--pre A.png --post B.png`, or `--file_root DIR --split test` for the reference's directory layout
(`<root>/<split>/{t1,t2,label}` for BCD, `{t1,t2,label1,label2,change}` for SCD; change3d_amd/data/dataset.py).

The reference has no such step: its scripts stop at `val()` over pre-cut crops of the training size (reference
scripts/train_BCD.py:92-154, scripts/train_SCD.py:104-178).  A pair of any size is decoded with PIL, uploaded once as
uint8 and tiled, predicted and stitched on the GPU (change3d_amd/infer.py).  The mask (0 / 255) or the two class maps and
the change mask are written as PNG; where labels exist the scene's predictions go to the on-device confusion matrix (BCD)
or joint histogram (SCD) of the training mirrors and the reference's score line is printed
(scripts/train_BCD.py:364-370, scripts/train_SCD.py:172-176).
"""
import os
import sys
from argparse import ArgumentParser
from types import SimpleNamespace

import numpy as np
import torch
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from change3d_amd.data.dataset import BCDDataset, SCDDataset, read_label, read_rgb  # noqa: E402
from change3d_amd.infer import SceneInferencer  # noqa: E402
from change3d_amd.model.trainer import Trainer  # noqa: E402
from change3d_amd.model.utils import SCDHistogram  # noqa: E402
from change3d_amd.utils.metric_tool import ConfuseMatrixMeter  # noqa: E402


def build_model(args, device):
    scd = args.task == "SCD"
    margs = SimpleNamespace(pretrained=args.pretrained, num_perception_frame=3 if scd else 1, in_height=args.in_height,
                            in_width=args.in_width, dataset="SECOND" if scd else "LEVIR-CD",
                            num_class=args.num_class if scd else 1,
                            act_dtype=torch.bfloat16 if args.act_dtype == "bf16" else torch.float32)
    model = Trainer(margs)
    state = torch.load(args.weights, map_location="cpu")
    model.load_state_dict(state["state_dict"] if "state_dict" in state else state)
    return model.to(device)


def scenes(args):
    """(name, image uint8 [H, W, 6], label uint8 or None) per scene."""
    if args.file_root:
        ds = (SCDDataset if args.task == "SCD" else BCDDataset)(args.file_root, args.split)
        for i, name in enumerate(ds.file_list):
            img, label = ds.raw(i)
            yield os.path.splitext(name)[0], img, label
        return
    pre, post = read_rgb(args.pre), read_rgb(args.post)
    if pre.shape != post.shape:
        raise ValueError(f"{args.pre} is {pre.shape[:2]} but {args.post} is {post.shape[:2]}")
    files = [args.label] if args.task == "BCD" else [args.label1, args.label2, args.change]
    label = None
    if all(files):
        labels = [read_label(f) for f in files]
        label = labels[0] if len(labels) == 1 else np.stack(labels, axis=2)
    yield "scene", np.concatenate((pre, post), axis=2), label


def save_png(path, array):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    Image.fromarray(array).save(path)


def main(argv=None):
    args = build_parser().parse_args(argv)
    if not args.file_root and not (args.pre and args.post):
        raise SystemExit("give --pre and --post, or --file_root")
    device = torch.device("cuda", args.gpu_id)
    torch.cuda.set_device(device)
    model = build_model(args, device)
    inf = SceneInferencer(model, args.task.lower(), stride=args.stride, window=args.window, batch=args.batch_size)
    meter = ConfuseMatrixMeter(n_class=2) if args.task == "BCD" else SCDHistogram(args.num_class, device)
    scored = 0
    for name, img, label in scenes(args):
        out = inf.predict(torch.from_numpy(np.ascontiguousarray(img)))
        if args.task == "BCD":
            mask = out[1]
            save_png(os.path.join(args.out_dir, name + ".png"), mask.cpu().numpy() * 255)
            if label is not None:        # ceil(u8 / 255), the label side of c3d_bcd_preprocess
                meter.update_cm_device(mask.float(), (torch.from_numpy(np.ascontiguousarray(label)).to(device) > 0).float())
                scored += 1
        else:
            for sub, m in zip(("pred1", "pred2", "change"), out):
                save_png(os.path.join(args.out_dir, sub, name + ".png"), m.cpu().numpy() * (255 if sub == "change" else 1))
            if label is not None:        # reference scripts/train_SCD.py:216-217: the class labels count inside the change only
                lab = torch.from_numpy(np.ascontiguousarray(label)).to(device).long()
                meter.update(out[0], lab[..., 0] * lab[..., 2])
                meter.update(out[1], lab[..., 1] * lab[..., 2])
                scored += 1
        print(f"{name}: {img.shape[0]} x {img.shape[1]} -> {args.out_dir}")
    if not scored:
        return None
    if args.task == "BCD":
        s = meter.get_scores()
        print(f"\nTest:\t Kappa (te) = {s['Kappa']:.4f}\t IoU (te) = {s['IoU']:.4f}\tF1 (te) = {s['F1']:.4f}\t "
              f"R (te) = {s['recall']:.4f}\tP (te) = {s['precision']:.4f}")
        return s
    Fscd, iou, sek = meter.scores()
    print(f"Fscd: {Fscd * 100:.2f} IoU: {iou * 100:.2f} Sek: {sek * 100:.2f}")
    return Fscd, iou, sek


def build_parser():
    p = ArgumentParser()
    p.add_argument("--task", choices=["BCD", "SCD"], default="BCD")
    p.add_argument("--weights", required=True, help="best_model.pth (a state dict) or checkpoint.pth.tar of the training scripts")
    p.add_argument("--pre", default="")
    p.add_argument("--post", default="")
    p.add_argument("--label", default="", help="BCD change mask of the --pre / --post pair, scored when given")
    p.add_argument("--label1", default="", help="SCD: pre class map; scored when --label1, --label2 and --change are given")
    p.add_argument("--label2", default="")
    p.add_argument("--change", default="")
    p.add_argument("--file_root", default="", help="data set root in the reference's layout, instead of --pre / --post")
    p.add_argument("--split", default="test")
    p.add_argument("--out_dir", default="./scene_out")
    p.add_argument("--stride", type=int, default=None, help="tile stride; default: half the tile")
    p.add_argument("--window", choices=["hann", "flat"], default="hann")
    p.add_argument("--batch_size", type=int, default=32, help="tiles per forward")
    p.add_argument("--act_dtype", choices=["f32", "bf16"], default="bf16")
    p.add_argument("--in_height", type=int, default=256)
    p.add_argument("--in_width", type=int, default=256)
    p.add_argument("--num_class", type=int, default=7, help="SCD classes")
    p.add_argument("--pretrained", default="./pretrained/X3D_L.pyth")
    p.add_argument("--gpu_id", default=0, type=int)
    return p


if __name__ == "__main__":
    main()
