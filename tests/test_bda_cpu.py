"""CPU suite of the building-damage-assessment task: C-ABI surface (exports, header, option index), the reference-shaped
`Evaluator` against the reference-generated `bda_metrics.npz` (and against the imported reference class when its tree is
present), the oracle's `update_bda` restatement against `bda_s{64,256}_b2.npz`, the script's flags, the drop-in import
lines of the reference's `train_BDA.py`, the synthetic labels, and the 2-rank gloo wiring of a BDA trainer."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NUM_CLASS = 5


def test_library_exports_and_header_declare_the_bda_entry_points():
    from change3d_amd import _lib
    names = _lib.check_exports()
    header = open(os.path.join(ROOT, "include", "change3d_hip.h")).read()
    for sym in ("c3d_bda_label_preprocess", "c3d_bda_confusion"):
        assert sym in names and hasattr(_lib.lib(), sym)
        assert re.search(r"\bint\s+%s\s*\(" % sym, header), sym
    assert re.search(r"C3D_OPT_DW_T4\s*=\s*11\b", header) and _lib.OPT_DW_T4 == 11
    # (c3d_set_option touches host state only: no GPU needed)
    assert _lib.lib().c3d_set_option(_lib.OPT_DW_T4, 0) == 0
    assert _lib.lib().c3d_set_option(_lib.OPT_DW_T4, 1) == 0
    assert _lib.lib().c3d_set_option(_lib.OPT_DW_T4 + 1, 1) != 0


def _val_scores(Evaluator, pred_cls, pred_loc, label):
    """The metric half of reference scripts/train_BDA.py:120-138 on host arrays."""
    label = torch.from_numpy(label)
    label_loc, label_cls = label[:, 0].float().numpy(), torch.prod(label, dim=1).long().numpy()
    ev_loc, ev_cls = Evaluator(num_class=2), Evaluator(num_class=NUM_CLASS)
    ev_loc.add_batch(label_loc, (pred_loc > 0.5).squeeze(1))
    pc = torch.argmax(torch.from_numpy(pred_cls), dim=1).numpy()
    ev_cls.add_batch(label_cls[label_loc > 0], pc[label_loc > 0])
    return ev_loc, ev_cls


def _cases(golden_dir):
    G = np.load(os.path.join(golden_dir, "bda_metrics.npz"))
    return G, [str(c) for c in G["cases"]]


def test_evaluator_matches_the_reference_generated_metrics(golden_dir):
    from change3d_amd.model.utils import Evaluator, bda_scores
    G, cases = _cases(golden_dir)
    assert {"class_never_occurs", "no_building", "ties"} <= set(cases)
    for c in cases:
        ev_loc, ev_cls = _val_scores(Evaluator, G[f"{c}_pred_cls"], G[f"{c}_pred_loc"], G[f"{c}_label"])
        assert ev_loc.confusion_matrix.dtype == np.longlong
        assert np.array_equal(ev_loc.confusion_matrix, G[f"{c}_cm_loc"]), c
        assert np.array_equal(ev_cls.confusion_matrix, G[f"{c}_cm_cls"]), c
        with np.errstate(divide="ignore", invalid="ignore"):
            loc_f1, harm, oa, dmg = bda_scores(ev_loc, ev_cls)
        got = np.concatenate([[loc_f1, harm, oa], dmg])
        assert np.allclose(got, G[f"{c}_scores"], rtol=0, atol=1e-12, equal_nan=True), (c, got, G[f"{c}_scores"])
    ev = Evaluator(3)
    ev.add_batch(np.array([0, 1, 2, 5]), np.array([0, 1, 1, 0]))     # gt 5 is masked out, as in the reference
    assert ev.confusion_matrix.sum() == 3
    ev.reset()
    assert ev.confusion_matrix.sum() == 0


def test_evaluator_equals_the_imported_reference_class(golden_dir):
    from oracle import ref_import
    if not ref_import.reference_available():
        pytest.skip("the reference tree is not present")
    from change3d_amd.model.utils import Evaluator
    _, mu, _ = ref_import.import_reference()
    G, cases = _cases(golden_dir)
    methods = ["Pixel_Accuracy", "Damage_F1_socore", "Mean_Intersection_over_Union", "Kappa_coefficient",
               "Frequency_Weighted_Intersection_over_Union"]
    for c in cases:
        mine = _val_scores(Evaluator, G[f"{c}_pred_cls"], G[f"{c}_pred_loc"], G[f"{c}_label"])
        ref = _val_scores(mu.Evaluator, G[f"{c}_pred_cls"], G[f"{c}_pred_loc"], G[f"{c}_label"])
        for a, b in zip(mine, ref):
            assert np.array_equal(a.confusion_matrix, b.confusion_matrix)
            with np.errstate(divide="ignore", invalid="ignore"):
                for m in methods:
                    assert np.array_equal(np.asarray(getattr(a, m)()), np.asarray(getattr(b, m)()), equal_nan=True), (c, m)
                if a.num_class == 2:
                    for m in ("Pixel_Precision_Rate", "Pixel_Recall_Rate", "Pixel_F1_score", "Intersection_over_Union"):
                        assert np.array_equal(np.asarray(getattr(a, m)()), np.asarray(getattr(b, m)()), equal_nan=True), (c, m)


@pytest.mark.parametrize("gsize", [64, 256])
def test_oracle_bda_matches_reference_golden(gsize, golden_dir):
    """The oracle's `update_bda` restatement + the train_BDA.py loss against the fixtures the real reference produced."""
    from oracle import model as om
    from change3d_amd import synthetic as synth
    G = np.load(os.path.join(golden_dir, f"bda_s{gsize}_b2.npz"))
    size, batch = int(G["meta"][0]), int(G["meta"][1])
    net = om.Trainer(om.make_args(num_perception_frame=int(G["meta"][4]), size=size, dataset="xBD", num_class=int(G["meta"][5])))
    net.load_state_dict(synth.synth_state_dict(net, seed=int(G["meta"][2]), mask_margin=0.25))
    pre, post, _ = synth.synth_batch(batch, size, seed=int(G["meta"][3]))
    label = synth.synth_bda_labels(batch, size, seed=int(G["meta"][3]), num_class=NUM_CLASS).permute(0, 3, 1, 2)
    label_loc, label_cls = label[:, 0].float().unsqueeze(1), torch.prod(label, dim=1).long()
    net.train()
    pc, pl = net.update_bda(pre, post)
    seg, bn = om.cross_entropy_2d(pc, label_cls, ignore_index=0), om.bce_dice_loss(pl, label_loc)
    (seg + bn).backward()
    assert np.abs(np.array([seg.item(), bn.item(), (seg + bn).item()]) - G["losses"]).max() < 1e-5
    idx = np.random.default_rng(7).integers(0, pc.numel(), size=64)
    assert np.abs(pc.detach().double().view(-1)[idx].numpy() - G["cls_summary"][3:]).max() < 2e-5
    named = dict(net.named_parameters())
    gn = np.array([named[str(n)].grad.double().norm().item() for n in G["grad_names"]])
    assert np.allclose(gn, G["grad_summaries"][:, 2], rtol=2e-3, atol=1e-9)
    assert G["loss_curve"].shape == (3, 3) and G["loss_curve"][2, 2] < G["loss_curve"][0, 2]
    assert G["cm_loc"].sum() == batch * size * size and G["cm_cls"].sum() == int((label_loc > 0).sum())


def test_train_bda_flags_equal_the_reference_defaults():
    from change3d_amd.scripts.train_BDA import build_parser
    a = build_parser().parse_args([])
    want = dict(dataset="xBD", file_root="path/to/xBD", in_height=256, in_width=256, num_perception_frame=2, num_class=5,
                max_steps=200000, batch_size=12, num_workers=4, lr=2e-4, lr_mode="poly", step_loss=100,
                pretrained="model/X3D_L.pyth", save_dir="./exp", resume=None, log_file="train_val_log.txt", gpu_id=0)
    for k, v in want.items():
        assert getattr(a, k) == v, k
    assert a.synthetic is False and a.act_dtype == "bf16"


# what the reference's scripts/train_BDA.py imports from its top-level packages (names only)
BDA_IMPORTS = {"model.trainer": ["Trainer"],
               "model.utils": ["adjust_learning_rate", "BCEDiceLoss", "CrossEntropyLoss2d", "load_checkpoint", "setup_logger",
                               "Evaluator"],
               "data.transforms": ["BDATransforms"]}


def test_dropin_resolves_the_import_lines_of_train_bda():
    code = "; ".join(f"from {m} import {', '.join(ns)}" for m, ns in BDA_IMPORTS.items())
    code += ("; import change3d_amd.model.utils as u, change3d_amd.data.transforms as t; assert Evaluator is u.Evaluator; "
             "assert BDATransforms is t.BDATransforms; assert callable(BDATransforms.get_transform_pipelines); print('ok')")
    env = dict(os.environ, PYTHONPATH=os.path.join(ROOT, "change3d_amd", "dropin") + os.pathsep + ROOT)
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, cwd="/")
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stderr


def test_synth_bda_labels_are_deterministic_and_have_every_class():
    from change3d_amd.synthetic import synth_bda_labels
    for size in (64, 256):
        a = synth_bda_labels(3, size, seed=4)
        assert a.dtype == torch.uint8 and tuple(a.shape) == (3, size, size, 2)
        assert torch.equal(a, synth_bda_labels(3, size, seed=4)) and not torch.equal(a, synth_bda_labels(3, size, seed=5))
        cls = (a[..., 0].long() * a[..., 1].long())
        for b in range(3):
            assert set(cls[b].unique().tolist()) == set(range(NUM_CLASS))
        frac = a[..., 0].float().mean().item()
        assert 0.01 < frac < 0.5                         # buildings are a real minority
        assert (a[..., 1][a[..., 0] == 0] == 0).all()


def _bda_ddp_worker(rank, world, port, q):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    sys.path.insert(0, ROOT)
    from change3d_amd.model.trainer import Trainer
    from change3d_amd.parallel import GradSync, broadcast_module_state, setup_data_parallel
    from change3d_amd.synthetic import make_args
    torch.manual_seed(100 + rank)
    net = Trainer(make_args(num_perception_frame=2, size=32, dataset="xBD", num_class=NUM_CLASS))
    broadcast_module_state(net)
    arena, sync = setup_data_parallel(net, torch.device("cpu"), overlap=True)
    assert isinstance(sync, GradSync) and sync.world == world
    names = set(arena.names)
    assert any(n.startswith("decoder_cls.") for n in names) and any(n.startswith("decoder_loc.") for n in names)
    arena.zero_grad()
    for i, p in enumerate(arena.params):
        p.grad.fill_(float(rank + 1) * (1 + i % 3))
    hook = net.encoder.x3d.blocks[3].post_backward
    if hook is not None:
        hook()
    sync.finish()
    want = torch.cat([torch.full((p.numel(),), 1.5 * (1 + i % 3)) for i, p in enumerate(arena.params)])
    got = torch.cat([p.grad.reshape(-1) for p in arena.params])
    q.put((rank, bool(torch.equal(got, want)), float(next(net.parameters()).sum())))
    dist.barrier()
    dist.destroy_process_group()


def test_two_rank_gloo_wiring_takes_a_bda_trainer_unchanged():
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 31500 + (os.getpid() % 2000)
    procs = [ctx.Process(target=_bda_ddp_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=300) for _ in range(2))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert res[0][1] and res[1][1], "all-reduced gradients are not the mean of the ranks'"
    assert res[0][2] == res[1][2], "parameters were not broadcast"
