"""Building damage assessment on the GPU: the two step-shell kernels through the C ABI against numpy statements of the
reference, the f32 train step against the reference-generated fixtures `bda_s{64,256}_b2.npz`, the bf16 step run to run, and
`scripts/train_BDA.py --synthetic` end to end (losses, scores against the host `Evaluator`, checkpoint round trip).
Nothing here reads the reference tree."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NUM_CLASS = 5


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")


# ------------------------------------------------------------------------------------------- step-shell kernels
@pytest.mark.parametrize("shape", [(8, 33, 40), (3, 64, 64), (2, 17, 23)])
def test_bda_label_preprocess_is_bit_exact_for_all_flag_combinations(shape):
    """c3d_bda_label_preprocess against numpy: cv2.flip(., 0) / cv2.flip(., 1) of the HWC label, no exchange of the labels,
    label[:, 0].float() and torch.prod(label, dim=1).long()."""
    _need_gpu()
    from change3d_amd.data.transforms import DeviceBDABatchTransform
    B, H, W = shape
    rng = np.random.default_rng(11)
    img = rng.integers(0, 256, size=(B, H, W, 6), dtype=np.uint8)
    lab = np.stack([rng.integers(0, 2, size=(B, H, W)), rng.integers(0, NUM_CLASS, size=(B, H, W))], axis=-1).astype(np.uint8)
    lab[0, 0, 0] = (200, 3)                                 # the product does not wrap at 256
    flags = np.array([[(k >> 0) & 1, (k >> 1) & 1, (k >> 2) & 1] for k in range(B)], dtype=np.uint8) if B == 8 else \
        (rng.random((B, 3)) < 0.5).astype(np.uint8)
    pre, post, loc, cls = DeviceBDABatchTransform(DEV)(img, lab, flags)
    torch.cuda.synchronize()
    for b in range(B):
        im, lb = img[b], lab[b]
        if flags[b, 0]:
            im, lb = im[::-1], lb[::-1]
        if flags[b, 1]:
            im, lb = im[:, ::-1], lb[:, ::-1]
        if flags[b, 2]:
            im = np.concatenate([im[:, :, 3:6], im[:, :, 0:3]], axis=2)
        imf = (im.astype(np.float32) / 255.0 - np.float32(0.5)) / np.float32(0.5)
        lt = torch.from_numpy(np.ascontiguousarray(lb.transpose(2, 0, 1)))
        assert np.array_equal(pre[b].cpu().numpy(), imf[:, :, 0:3].transpose(2, 0, 1))
        assert np.array_equal(post[b].cpu().numpy(), imf[:, :, 3:6].transpose(2, 0, 1))
        assert torch.equal(loc[b, 0].cpu(), lt[0].float())
        assert torch.equal(cls[b].cpu(), torch.prod(lt, dim=0).long())
    assert loc.dtype == torch.float32 and cls.dtype == torch.int64 and tuple(loc.shape) == (B, 1, H, W)


def _host_matrices(pred_cls, pred_loc, label_loc, label_cls, n):
    from change3d_amd.model.utils import Evaluator
    ev_loc, ev_cls = Evaluator(2), Evaluator(n)
    loc = label_loc.reshape(label_cls.shape)
    ev_loc.add_batch(loc, (pred_loc > 0.5).reshape(loc.shape))
    pc = torch.argmax(torch.from_numpy(pred_cls), dim=1).numpy()
    ev_cls.add_batch(label_cls[loc > 0], pc[loc > 0])
    return ev_loc, ev_cls


def test_bda_confusion_matches_the_reference_generated_metrics(golden_dir):
    """c3d_bda_confusion + BDAEvaluator against tests/golden/bda_metrics.npz (matrices and scores of the REAL reference's
    Evaluator): a class that never occurs, a batch without buildings, ties in the logits, probabilities of exactly 0.5."""
    _need_gpu()
    from change3d_amd.model.utils import BDAEvaluator
    G = np.load(os.path.join(golden_dir, "bda_metrics.npz"))
    for c in [str(c) for c in G["cases"]]:
        label = torch.from_numpy(G[f"{c}_label"])
        label_loc, label_cls = label[:, 0].float().unsqueeze(1), torch.prod(label, dim=1).long()
        ev = BDAEvaluator(NUM_CLASS, DEV)
        ev.add_batch(torch.from_numpy(G[f"{c}_pred_cls"]).to(DEV), torch.from_numpy(G[f"{c}_pred_loc"]).to(DEV),
                     label_loc.to(DEV), label_cls.to(DEV))
        loc, cls = ev.evaluators()
        assert np.array_equal(loc.confusion_matrix, G[f"{c}_cm_loc"]), c
        assert np.array_equal(cls.confusion_matrix, G[f"{c}_cm_cls"]), c
        with np.errstate(divide="ignore", invalid="ignore"):
            loc_f1, harm, oa, dmg = ev.scores()
        assert np.allclose(np.concatenate([[loc_f1, harm, oa], dmg]), G[f"{c}_scores"], rtol=0, atol=1e-12, equal_nan=True), c


@pytest.mark.parametrize("n,B,HW", [(5, 3, 1000), (5, 12, 256 * 256), (16, 2, 777), (1, 2, 64)])
def test_bda_confusion_equals_numpy_accumulates_and_counts_labels_out_of_range(n, B, HW):
    _need_gpu()
    from change3d_amd.model.utils import BDAEvaluator
    rng = np.random.default_rng(5 + n)
    pred_cls = np.round(rng.standard_normal((B, n, HW)).astype(np.float32) * 2) / 2        # ties are common
    pred_loc = rng.random((B, 1, HW)).astype(np.float32)
    pred_loc[0, 0, :7] = 0.5
    label_loc = (rng.random((B, HW)) < 0.2).astype(np.float32)
    label_cls = (rng.integers(0, n, size=(B, HW)) * label_loc).astype(np.int64)
    ev = BDAEvaluator(n, DEV)
    for _ in range(2):                                        # counts accumulate over batches
        ev.add_batch(*(torch.from_numpy(a).to(DEV) for a in (pred_cls, pred_loc, label_loc, label_cls)))
    loc, cls = ev.evaluators()
    h_loc, h_cls = _host_matrices(pred_cls, pred_loc, label_loc, label_cls, n)
    assert np.array_equal(loc.confusion_matrix, 2 * h_loc.confusion_matrix)
    assert np.array_equal(cls.confusion_matrix, 2 * h_cls.confusion_matrix)
    # labels out of range: dropped from the matrices like the reference's mask does, counted, and refused by default
    bad = label_cls.copy()
    k = np.flatnonzero(label_loc.reshape(-1) > 0)[:3]
    bad.reshape(-1)[k] = [n, -1, 99]
    ev.reset()
    ev.add_batch(*(torch.from_numpy(a).to(DEV) for a in (pred_cls, pred_loc, label_loc, bad)))
    assert int(ev.counts[-1]) == 3
    with pytest.raises(ValueError):
        ev.evaluators()
    _, cls_bad = ev.evaluators(strict=False)
    assert cls_bad.confusion_matrix.sum() == h_cls.confusion_matrix.sum() - 3
    # a batch without buildings leaves the damage matrix empty
    ev.reset()
    zero = np.zeros_like(label_loc)
    ev.add_batch(*(torch.from_numpy(a).to(DEV) for a in (pred_cls, pred_loc, zero, label_cls)))
    assert ev.evaluators()[1].confusion_matrix.sum() == 0


def test_ce2d_at_five_classes_with_most_pixels_ignored():
    """CrossEntropyLoss2d(ignore_index=0) where background (ignored) is the majority, as on xBD: loss and gradient against
    torch on the CPU."""
    _need_gpu()
    from change3d_amd.model.utils import CrossEntropyLoss2d
    from change3d_amd.synthetic import synth_bda_labels
    lab = synth_bda_labels(3, 64, seed=2)
    target = (lab[..., 0].long() * lab[..., 1].long())
    assert (target == 0).float().mean() > 0.8
    x = torch.from_numpy(np.random.default_rng(3).standard_normal((3, NUM_CLASS, 64, 64)).astype(np.float32))
    xr = x.clone().requires_grad_(True)
    want = torch.nn.functional.nll_loss(torch.log_softmax(xr, dim=1), target, ignore_index=0)
    want.backward()
    xd = x.to(DEV).requires_grad_(True)
    got = CrossEntropyLoss2d(ignore_index=0)(xd, target.to(DEV))
    got.backward()
    assert abs(got.item() - want.item()) < 1e-5
    assert torch.allclose(xd.grad.cpu(), xr.grad, rtol=1e-4, atol=1e-7)
    assert (xd.grad.cpu()[(target == 0)[:, None].expand_as(x)] == 0).all()


# ------------------------------------------------------------------------------------------- the train step
def _setup(size, batch, dtype, wseed=16, dseed=0):
    from change3d_amd import synthetic as synth
    from change3d_amd.model.trainer import Trainer
    args = synth.make_args(num_perception_frame=2, size=size, dataset="xBD", num_class=NUM_CLASS)
    args.act_dtype = dtype
    net = Trainer(args)
    net.load_state_dict(synth.synth_state_dict(net, seed=wseed, mask_margin=0.25))
    net = net.to(DEV).train()
    pre, post, _ = synth.synth_batch(batch, size, seed=dseed)
    label = synth.synth_bda_labels(batch, size, seed=dseed, num_class=NUM_CLASS).permute(0, 3, 1, 2)
    label_loc, label_cls = label[:, 0].float().unsqueeze(1), torch.prod(label, dim=1).long()
    return net, pre.to(DEV), post.to(DEV), label_loc.to(DEV), label_cls.to(DEV)


def _summ(t):
    t = t.detach().double().cpu().contiguous().view(-1)
    idx = np.random.default_rng(7).integers(0, t.numel(), size=64)
    return np.concatenate([[t.mean().item(), t.std().item(), t.norm().item()], t[idx].numpy()])


@pytest.mark.parametrize("gsize", [64, 256])
def test_e2e_bda_f32_train_steps_against_the_reference_fixture(gsize, golden_dir):
    """Outputs, the three losses, gradients of step 1, the three-step loss curve (FusedAdam + adjust_learning_rate with the
    script's hyper-parameters), final parameter norms, BatchNorm buffers, eval-mode outputs and the `val` matrices / scores
    against what the REAL reference produced on CPU f32."""
    _need_gpu()
    from types import SimpleNamespace
    from change3d_amd.model.utils import (BDAEvaluator, CrossEntropyLoss2d, FusedAdam, ParamArena, adjust_learning_rate,
                                          hot_path_named_params)
    from change3d_amd.scripts.train_BDA import bda_loss
    G = np.load(os.path.join(golden_dir, f"bda_s{gsize}_b2.npz"))
    net, pre, post, label_loc, label_cls = _setup(int(G["meta"][0]), int(G["meta"][1]), torch.float32)
    arena = ParamArena(hot_path_named_params(net), torch.device(DEV))
    opt = FusedAdam(arena, 2e-4, (0.9, 0.99), eps=1e-08, weight_decay=1e-4)
    seg_loss = CrossEntropyLoss2d(ignore_index=0)
    args = SimpleNamespace(lr=2e-4, lr_mode="poly", max_epochs=1, step_loss=100)
    named = dict(hot_path_named_params(net))
    names = [str(n) for n in G["grad_names"]]
    assert set(names) == set(named)
    curve = []
    for it in range(-1, 3):     # the fixture's order: one forward / backward for the gradients, then three optimiser steps
        if it >= 0:
            adjust_learning_rate(args, opt, 0, it, 200000)
        pc, pl = net.update_bda(pre, post)
        seg, bn, loss = bda_loss(seg_loss, pc, pl, label_loc, label_cls)
        opt.zero_grad()
        loss.backward()
        if it < 0:
            torch.cuda.synchronize()
            s_cls, s_loc = _summ(pc), _summ(pl)
            assert np.abs(s_cls - G["cls_summary"]).max() < 2e-4 * max(1.0, np.abs(G["cls_summary"]).max())
            assert np.abs(s_loc - G["loc_summary"]).max() < 2e-4
            gn = np.array([named[n].grad.double().norm().item() for n in names])
            ref = G["grad_summaries"][:, 2]
            rel = np.abs(gn - ref) / (ref + 1e-12)
            # (per-gradient strictness is the subject of the kink analysis of the f32 tests; here: norms, with the few
            # gradients a ReLU unit at its kink can move granted)
            assert np.median(rel) < 1e-3 and (rel > 5e-2).sum() <= 0.02 * len(names), (np.median(rel), rel.max())
            continue
        opt.step()
        curve.append([seg.item(), bn.item(), loss.item()])
    curve = np.array(curve)
    assert np.abs(curve[0] - G["losses"]).max() < 1e-4
    assert np.abs(curve - G["loss_curve"]).max() < 2e-3, (curve, G["loss_curve"])
    pn = np.array([named[n].detach().double().norm().item() for n in names])
    assert np.allclose(pn, G["param_norms"], rtol=1e-4, atol=1e-6)
    bufs = dict(net.named_buffers())
    bn_ = np.array([bufs[str(n)].double().norm().item() for n in G["buffer_names"]])
    assert np.allclose(bn_, G["buffer_norms"], rtol=2e-3, atol=1e-5)
    net.eval()
    with torch.no_grad():
        ec, el = net.update_bda(pre, post)
    # (eval-mode probabilities of the synthetic weights are saturated: a probe on the sigmoid's slope moves by percents
    # for an f32-rounding change of the running statistics; mean / std and the bulk of the probes are tight)
    d_eval = np.abs(_summ(el) - G["eval_loc_summary"])
    assert d_eval[:2].max() < 2e-3 and np.median(d_eval[3:]) < 1e-3 and d_eval[3:].max() < 0.2, d_eval
    ev = BDAEvaluator(NUM_CLASS, DEV)
    ev.add_batch(ec, el, label_loc, label_cls)
    loc, cls = ev.evaluators()
    total = float(G["cm_loc"].sum())
    # pixels at the 0.5 / argmax boundary after three optimiser steps (a flipped pixel counts twice; the weight gradients'
    # f32 atomics make the count vary by a few pixels run to run)
    assert loc.confusion_matrix.sum() == total and cls.confusion_matrix.sum() == G["cm_cls"].sum()
    assert np.abs(loc.confusion_matrix - G["cm_loc"]).sum() <= 5e-3 * total
    assert np.abs(cls.confusion_matrix - G["cm_cls"]).sum() <= 3e-2 * max(1.0, float(G["cm_cls"].sum()))


def test_bda_bf16_step_at_256_batch_12_is_finite_and_reproducible():
    _need_gpu()
    from change3d_amd.model.utils import CrossEntropyLoss2d, hot_path_named_params
    from change3d_amd.scripts.train_BDA import bda_loss
    runs = []
    for _ in range(2):
        net, pre, post, label_loc, label_cls = _setup(256, 12, torch.bfloat16)
        pc, pl = net.update_bda(pre, post)
        assert tuple(pc.shape) == (12, NUM_CLASS, 256, 256) and tuple(pl.shape) == (12, 1, 256, 256)
        _, _, loss = bda_loss(CrossEntropyLoss2d(ignore_index=0), pc, pl, label_loc, label_cls)
        loss.backward()
        torch.cuda.synchronize()
        grads = [p.grad for _, p in hot_path_named_params(net)]
        assert all(g is not None and torch.isfinite(g).all() for g in grads) and torch.isfinite(loss)
        runs.append((pc.detach().clone(), pl.detach().clone(), loss.item(),
                     torch.stack([g.double().norm() for g in grads]).cpu()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1]), "forward is not reproducible"
    assert runs[0][2] == runs[1][2]
    assert torch.allclose(runs[0][3], runs[1][3], rtol=1e-3), "gradient norms differ run to run beyond atomic-order noise"


def test_bda_bf16_step_with_four_frame_kernels_off_gives_the_same_forward():
    """C3D_OPT_DW_T4 = 0 against 1 through the whole network: the depthwise outputs are bit-identical, so is everything
    downstream of them up to the order of the statistics' atomics."""
    _need_gpu()
    from change3d_amd import ops
    outs = []
    try:
        for v in (1, 0):
            ops.set_option(ops.OPT_DW_T4, v)
            net, pre, post, _, _ = _setup(128, 4, torch.bfloat16)
            with torch.no_grad():
                pc, pl = net.update_bda(pre, post)
            torch.cuda.synchronize()
            outs.append((pc.float().cpu(), pl.float().cpu()))
    finally:
        ops.set_option(ops.OPT_DW_T4, 1)
    assert (outs[0][1] - outs[1][1]).abs().max().item() < 2e-2
    assert (outs[0][0] - outs[1][0]).abs().max().item() < 5e-2 * max(1.0, outs[1][0].abs().max().item())


# ------------------------------------------------------------------------------------------- the script
def test_train_bda_synthetic_trains_validates_and_round_trips_a_checkpoint(tmp_path):
    _need_gpu()
    from change3d_amd.model.trainer import Trainer
    from change3d_amd.model.utils import BDAEvaluator, CrossEntropyLoss2d, Evaluator, bda_scores
    from change3d_amd.scripts import train_BDA as S
    argv = ["--synthetic", "--synthetic_pairs", "16", "--batch_size", "4", "--in_height", "64", "--in_width", "64",
            "--max_steps", "8", "--save_dir", str(tmp_path), "--act_dtype", "f32"]
    args = S.build_parser().parse_args(argv)
    scores = S.trainValidate(args)                      # 2 epochs of 4 iterations: epoch 1 validates and saves
    assert scores is not None and np.isfinite(scores[0])
    save_path = os.path.join(str(tmp_path), "xBD_iter_8_lr_0.0002")
    log = open(os.path.join(save_path, "train_val_log.txt")).read()
    assert "epoch\tloss_val\tloc_f1_score\tharmonic_mean_f1\toa_f1\tdamage_f1_scores" in log
    rows = [l for l in log.splitlines() if l.startswith("1\t\t")]
    assert rows and len(rows[0].split("\t\t")) == 5 + (NUM_CLASS - 1)
    ck = torch.load(os.path.join(save_path, "checkpoint.pth.tar"), map_location="cpu")
    assert {"epoch", "arch", "state_dict", "optimizer", "loss_train", "loss_val", "loc_f1_score", "harmonic_mean_f1", "lr"} <= set(ck)
    assert os.path.isfile(os.path.join(save_path, "best_model.pth"))
    # checkpoint round trip: a fresh model with the saved weights reproduces the validation pass, and the device counts
    # give the scores the host Evaluator computes from the same predictions
    net = Trainer(args).to(DEV)
    net.load_state_dict(ck["state_dict"])
    net.eval()
    loader = S.SyntheticBDALoader(8, 4, 64, NUM_CLASS, seed=6)
    ev, h_loc, h_cls = BDAEvaluator(NUM_CLASS, DEV), Evaluator(2), Evaluator(NUM_CLASS)
    with torch.no_grad():
        for img, label_loc, label_cls in loader:
            pc, pl = net.update_bda(img[:, 0:3].contiguous(), img[:, 3:6].contiguous())
            ev.add_batch(pc, pl, label_loc, label_cls)
            loc = label_loc.squeeze(1).cpu().numpy()
            h_loc.add_batch(loc, (pl.cpu().numpy() > 0.5).squeeze(1))
            pcn, lcn = torch.argmax(pc, dim=1).cpu().numpy(), label_cls.cpu().numpy()
            h_cls.add_batch(lcn[loc > 0], pcn[loc > 0])
    d_loc, d_cls = ev.evaluators()
    assert np.array_equal(d_loc.confusion_matrix, h_loc.confusion_matrix)
    assert np.array_equal(d_cls.confusion_matrix, h_cls.confusion_matrix)
    with np.errstate(divide="ignore", invalid="ignore"):
        a, b = bda_scores(d_loc, d_cls), bda_scores(h_loc, h_cls)
    assert all(np.array_equal(np.asarray(x), np.asarray(y), equal_nan=True) for x, y in zip(a, b))


def test_bda_losses_go_down_on_a_fixed_batch():
    _need_gpu()
    from change3d_amd.model.utils import CrossEntropyLoss2d, FusedAdam, ParamArena, hot_path_named_params
    from change3d_amd.scripts.train_BDA import bda_loss
    net, pre, post, label_loc, label_cls = _setup(64, 4, torch.bfloat16)
    arena = ParamArena(hot_path_named_params(net), torch.device(DEV))
    opt = FusedAdam(arena, 2e-4, (0.9, 0.99), eps=1e-08, weight_decay=1e-4)
    seg_loss, losses = CrossEntropyLoss2d(ignore_index=0), []
    for _ in range(6):
        pc, pl = net.update_bda(pre, post)
        _, _, loss = bda_loss(seg_loss, pc, pl, label_loc, label_cls)
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(loss.item())
    assert all(np.isfinite(losses)) and losses[-1] < losses[0], losses
