"""MI355X-native mirror of the reference's `scripts/train_BDA.py` (building damage assessment on xBD; reference
scripts/train_BDA.py:102-143 `val`, :146-218 `train`, :221-383 `trainValidate`, :386-490 flags).

Same flags and defaults (`--dataset xBD --num_perception_frame 2 --num_class 5 --batch_size 12 --lr 2e-4 --lr_mode poly`),
same loop order and loss composition
    label_loc = label[:, 0].float(); label_cls = torch.prod(label, dim=1).long()           (:194-195)
    pred_cls, pred_loc = model.update_bda(pre, post)                                       (:208)
    loss = CrossEntropyLoss2d(ignore_index=0)(pred_cls, label_cls) + BCEDiceLoss(pred_loc, label_loc.unsqueeze(1))
same Adam hyper-parameters, log columns, checkpoint layout and "validate on the test split, skip epoch 0" behaviour.
Differences, all deliberate:
  * `--synthetic` draws xBD-shaped synthetic pairs and labels; flips, exchange, normalisation and the label arithmetic run
    on the device (`DeviceBDABatchTransform`: c3d_bcd_preprocess + c3d_bda_label_preprocess).  Without it
    `--file_root/{train,val,test}/{t1,t2,label1,label2}` is decoded once into an HBM-resident uint8 store and the
    reference's whole transform chain runs in one kernel per step (change3d_amd/data/resident.py, c3d_augment_gather);
  * the model is `change3d_amd.model.Trainer` (HIP kernels, T = 4 clips on the four-frame depthwise kernels), the optimizer
    the fused Adam over a ParamArena;
  * `val` accumulates both confusion matrices on the device (`BDAEvaluator`: c3d_bda_confusion) and reads 4 + n*n + 1
    integers back once per pass, instead of both predictions per iteration;
  * launched under torch.distributed.run it trains data-parallel (one rank per GPU).
"""
import os
import sys
import time
from argparse import ArgumentParser
from os.path import join as osp

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from change3d_amd.hostopt import freeze_gc  # noqa: E402
from change3d_amd.data.transforms import DeviceBDABatchTransform, draw_augmentation_flags  # noqa: E402
from change3d_amd.model.trainer import Trainer  # noqa: E402
from change3d_amd.model.utils import (BCEDiceLoss, BDAEvaluator, CrossEntropyLoss2d, FusedAdam, adjust_learning_rate,  # noqa: E402
                                      load_checkpoint, setup_logger)
from change3d_amd.parallel import broadcast_module_state, host_barrier, setup_data_parallel  # noqa: E402
from change3d_amd.synthetic import synth_bda_labels  # noqa: E402


class SyntheticBDALoader:
    """Stand-in for the reference DataLoader over `BDADataset` (reference scripts/train_BDA.py:31-99).  It draws what the
    data set holds BEFORE the tensor-side transforms -- raw uint8 pairs (B, H, W, 6) and uint8 labels (B, H, W, 2) =
    (localisation, damage class) -- and yields `(img f32 [B,6,H,W], label_loc f32 [B,1,H,W], label_cls int64 [B,H,W])` on the
    device.  The images carry the label (footprints are brighter in `post` by a class-dependent amount), so a few
    iterations on a fixed batch bring the loss down."""

    def __init__(self, n_pairs, batch_size, size, num_class, seed, drop_last=False, train=False):
        self.n, self.bs, self.size, self.nc, self.seed, self.train = n_pairs, batch_size, size, num_class, seed, train
        self.nb = n_pairs // batch_size if drop_last else -(-n_pairs // batch_size)
        self.transform = None

    def __len__(self):
        return self.nb

    def __iter__(self):
        rng = np.random.default_rng(self.seed)
        for i in range(self.nb):
            b = min(self.bs, self.n - i * self.bs)
            u8 = rng.integers(0, 128, size=(b, self.size, self.size, 6), dtype=np.uint8)
            lab = synth_bda_labels(b, self.size, seed=self.seed * 1000 + i, num_class=self.nc).numpy()
            u8[..., 3:6] += (lab[..., 0:1] * (lab[..., 1:2] * (127 // max(self.nc - 1, 1)))).astype(np.uint8)
            flags = draw_augmentation_flags(b, rng, train=self.train)
            if self.transform is None:
                self.transform = DeviceBDABatchTransform(torch.device("cuda", torch.cuda.current_device()))
            pre, post, label_loc, label_cls = self.transform(u8, lab, flags)
            yield torch.cat([pre, post], dim=1), label_loc, label_cls


def create_data_loaders(args, rank=0):
    if not args.synthetic:
        if not os.path.isdir(args.file_root):
            raise SystemExit(f"train_BDA: --file_root {args.file_root} is not a directory; point it at an xBD tree with "
                             f"train/val/test splits or run with --synthetic")
        from change3d_amd.data.dataset import BDADataset
        from change3d_amd.data.resident import build_file_loaders
        train, val, test = build_file_loaders(args, BDADataset, "bda", torch.device("cuda", torch.cuda.current_device()),
                                              rank, int(os.environ.get("WORLD_SIZE", "1")))
        print(f"For each epoch, we have {len(train)} batches.")
        return train, val, test, len(train)
    mk = lambda n, seed, **kw: SyntheticBDALoader(n, args.batch_size, args.in_height, args.num_class, seed, **kw)  # noqa: E731
    train = mk(args.synthetic_pairs, 10 + rank, drop_last=True, train=True)
    val = mk(max(args.batch_size, args.synthetic_pairs // 8), 5)
    test = mk(max(args.batch_size, args.synthetic_pairs // 8), 6)
    print(f"For each epoch, we have {len(train)} batches.")
    return train, val, test, len(train)


def bda_loss(seg_loss, pred_cls, pred_loc, label_loc, label_cls):
    """(segment_loss, binary_loss, loss) of reference scripts/train_BDA.py:209-211."""
    segment_loss = seg_loss(pred_cls, label_cls)
    binary_loss = BCEDiceLoss(pred_loc, label_loc)
    return segment_loss, binary_loss, segment_loss + binary_loss


@torch.no_grad()
def val(val_loader, model, seg_loss, evaluator):
    """reference scripts/train_BDA.py:102-143.  Returns (loss of the last batch, loc_f1, harmonic_mean_f1, oaf1,
    damage_f1_score) like the reference; `evaluator` is a BDAEvaluator."""
    model.eval()
    evaluator.reset()
    loss = None
    for img, label_loc, label_cls in val_loader:
        pre, post = img[:, 0:3].cuda().float(), img[:, 3:6].cuda().float()
        pred_cls, pred_loc = model.update_bda(pre, post)
        _, _, loss = bda_loss(seg_loss, pred_cls, pred_loc, label_loc, label_cls)
        evaluator.add_batch(pred_cls, pred_loc, label_loc, label_cls)
    loc_f1_score, harmonic_mean_f1, oaf1, damage_f1_score = evaluator.scores()
    print(f"lofF1 is {loc_f1_score}, clfF1 is {harmonic_mean_f1}, oaF1 is {oaf1}, sub class F1 score is {damage_f1_score} ")
    return float(loss), loc_f1_score, harmonic_mean_f1, oaf1, damage_f1_score


def train(args, train_loader, model, optimizer, sync, epoch, max_batches, cur_iter, seg_loss):
    model.train()
    epoch_loss, lr = [], args.lr
    for iter_idx, (img, label_loc, label_cls) in enumerate(train_loader):
        if iter_idx + cur_iter == 3:   # once per run, after the first iterations have built everything long-lived (hostopt.py)
            freeze_gc()
        pre, post = img[:, 0:3].cuda().float(), img[:, 3:6].cuda().float()
        start_time = time.time()
        lr = adjust_learning_rate(args, optimizer, epoch, iter_idx + cur_iter, max_batches)
        pred_cls, pred_loc = model.update_bda(pre, post)
        segment_loss, binary_loss, loss = bda_loss(seg_loss, pred_cls, pred_loc, label_loc, label_cls)
        optimizer.zero_grad()
        loss.backward()
        sync.finish()
        optimizer.step()
        epoch_loss.append(loss.detach())
        if (iter_idx + 1) % 5 == 0 and args.rank == 0:
            time_taken = time.time() - start_time
            res_time = (max_batches * args.max_epochs - iter_idx - cur_iter) * time_taken / 3600
            print(f"[epoch {epoch}] [iter {iter_idx + 1}/{len(train_loader)} {res_time:.2f}h] "
                  f"[lr {optimizer.param_groups[0]['lr']:.6f}] "
                  f"[seg_loss {segment_loss.item():.4f} bn_loss {binary_loss.item():.4f} sum_loss {loss.item():.4f}] ")
    return float(torch.stack(epoch_loss).mean()), lr


def _log_row(logger, epoch, loss_val, loc_f1_score, harmonic_mean_f1, oaf1, damage_f1_score):
    damage_scores = "\t\t".join(["%.4f"] * len(damage_f1_score))
    logger.write(("\n%d\t\t%.4f\t\t%.4f\t\t%.4f\t\t%.4f\t\t" + damage_scores) % (
        epoch, loss_val, loc_f1_score, harmonic_mean_f1, oaf1, *damage_f1_score))
    logger.flush()


def trainValidate(args):
    world = int(os.environ.get("WORLD_SIZE", "1"))
    args.rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", str(args.gpu_id)))
    torch.cuda.set_device(local)
    if world > 1:
        dist.init_process_group("nccl", device_id=torch.device("cuda", local))
    torch.manual_seed(seed=16)
    torch.cuda.manual_seed(seed=16)
    args.act_dtype = torch.bfloat16 if args.act_dtype == "bf16" else torch.float32
    model = Trainer(args).cuda()
    broadcast_module_state(model)
    seg_loss = CrossEntropyLoss2d(ignore_index=0)
    evaluator = BDAEvaluator(args.num_class, torch.device("cuda", local))
    save_path = osp(args.save_dir, f"{args.dataset}_iter_{args.max_steps}_lr_{args.lr}")
    os.makedirs(save_path, exist_ok=True)
    train_loader, _, test_loader, max_batches = create_data_loaders(args, args.rank)
    args.max_epochs = int(np.ceil(args.max_steps / max_batches))
    start_epoch, cur_iter = load_checkpoint(args, model, save_path, max_batches)
    logger = setup_logger(args, save_path) if args.rank == 0 else None
    arena, sync = setup_data_parallel(model, torch.device("cuda", local))
    optimizer = FusedAdam(arena, args.lr, (0.9, 0.99), eps=1e-08, weight_decay=1e-4)
    best_oa, model_file_name = 0, osp(save_path, "best_model.pth")
    epoch, loss_train, scores = start_epoch, float("nan"), None
    for epoch in range(start_epoch, args.max_epochs):
        loss_train, lr = train(args, train_loader, model, optimizer, sync, epoch, max_batches, cur_iter, seg_loss)
        cur_iter += len(train_loader)
        if epoch == 0:
            continue
        if args.rank != 0:   # rank 0 validates on its own BatchNorm statistics, the others wait on the host (train_BCD.py)
            host_barrier()
            continue
        scores = val(test_loader, model, seg_loss, evaluator)
        loss_val, loc_f1_score, harmonic_mean_f1, oaf1, damage_f1_score = scores
        _log_row(logger, epoch, *scores)
        torch.save({"epoch": epoch + 1, "arch": str(model), "state_dict": model.state_dict(),
                    "optimizer": optimizer.state_dict(), "loss_train": loss_train, "loss_val": loss_val,
                    "loc_f1_score": float(loc_f1_score), "harmonic_mean_f1": float(harmonic_mean_f1), "lr": lr},   # (plain floats: loadable with weights_only)
                   osp(save_path, "checkpoint.pth.tar"))
        if oaf1 > best_oa or not os.path.isfile(model_file_name):
            best_oa = max(best_oa, oaf1)
            torch.save(model.state_dict(), model_file_name)
        print(f"\nEpoch No. {epoch}:\tTrain Loss = {loss_train:.4f}\tVal Loss = {loss_val:.4f}\tloc_f1_score = {loc_f1_score:.4f}\t"
              f"harmonic_mean_f1 = {harmonic_mean_f1:.4f}\toaf1 = {oaf1:.4f}\tdamage_f1_score = {damage_f1_score}")
        host_barrier()
    if args.rank == 0 and os.path.isfile(model_file_name):   # test with the best model (reference :350-380)
        model.load_state_dict(torch.load(model_file_name, map_location="cpu"))
        scores = val(test_loader, model, seg_loss, evaluator)
        _log_row(logger, epoch, *scores)
    if logger:
        logger.close()
    if world > 1:
        dist.destroy_process_group()
    return scores


def build_parser():
    p = ArgumentParser()
    p.add_argument("--dataset", default="xBD", help="Dataset selection | xBD |")
    p.add_argument("--file_root", default="path/to/xBD", help="xBD root with train/val/test splits (read unless --synthetic)")
    p.add_argument("--resident_gb", type=float, default=16.0, help="keep the decoded uint8 store in HBM up to this size")
    p.add_argument("--in_height", type=int, default=256)
    p.add_argument("--in_width", type=int, default=256)
    p.add_argument("--num_perception_frame", type=int, default=2)
    p.add_argument("--num_class", type=int, default=5)
    p.add_argument("--max_steps", type=int, default=200000)
    p.add_argument("--batch_size", type=int, default=12)
    p.add_argument("--num_workers", type=int, default=4)
    p.add_argument("--lr", type=float, default=2e-4)
    p.add_argument("--lr_mode", default="poly")
    p.add_argument("--step_loss", type=int, default=100)
    p.add_argument("--pretrained", default="model/X3D_L.pyth")
    p.add_argument("--save_dir", default="./exp")
    p.add_argument("--resume", default=None)
    p.add_argument("--log_file", default="train_val_log.txt")
    p.add_argument("--gpu_id", default=0, type=int)
    p.add_argument("--synthetic", action="store_true", help="train on synthetic xBD-shaped pairs instead of --file_root")
    p.add_argument("--synthetic_pairs", type=int, default=240, help="pairs per synthetic epoch")
    p.add_argument("--act_dtype", choices=["f32", "bf16"], default="bf16")
    return p


if __name__ == "__main__":
    trainValidate(build_parser().parse_args())
