"""`c3d_augment_gather` and the resident-store loader on the MI355X: bit-identity with the three plain preprocess passes
for a zero table, the crop path against the torch-CPU chain of augment_reference.py, gather, the two-launch path,
argument refusals, loader epochs and placements, and the three script mirrors fed from a PNG tree."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import augment_reference as R  # noqa: E402
from test_data_cpu import write_tree  # noqa: E402

from change3d_amd import _lib as L  # noqa: E402
from change3d_amd import ops  # noqa: E402
from change3d_amd.data.transforms import BCDTransforms as T, crop_area_of, validate_augment_table  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TASK = {"bcd": (L.AUG_BCD, 1), "scd": (L.AUG_SCD, 3), "bda": (L.AUG_BDA, 2)}
CONSTANTS = {"default": (T.DEFAULT_MEAN, T.DEFAULT_STD), "imagenet": (T.IMAGENET_MEAN, T.IMAGENET_STD)}


def run_kernel(images, labels, table, mean, std, H, W, task, fill=None):
    """(pre, post, labels...) on the CPU.  table: int32 numpy [B, 8] (validated here, as the wrapper's callers must) or None."""
    dev = torch.device("cuda:0")
    code, _ = TASK[task]
    N, Hs, Ws = images.shape[:3]
    B = N if table is None else len(table)
    if table is not None:
        validate_augment_table(table, N, H, W)
    di, dl = torch.from_numpy(images).to(dev), torch.from_numpy(labels).to(dev)
    dt = None if table is None else torch.from_numpy(table).to(dev)
    mk = lambda shape, dt_: torch.empty(shape, dtype=dt_, device=dev) if fill is None else torch.full(shape, fill, dtype=dt_, device=dev)  # noqa: E731
    pre, post = mk((B, 3, H, W), torch.float32), mk((B, 3, H, W), torch.float32)
    la = mk((B, 3, H, W), torch.int64) if task == "scd" else mk((B, 1, H, W), torch.float32)
    lb = mk((B, H, W), torch.int64) if task == "bda" else None
    scratch = torch.empty((2, B, 3, H, W), dtype=torch.float32, device=dev) if table is not None and (Hs, Ws) != (H, W) else None
    ops.augment_gather(di, dl, dt, torch.tensor(mean, device=dev), torch.tensor(std, device=dev), pre, post, la, lb, scratch,
                       code, N, Hs, Ws, B, H, W)
    torch.cuda.synchronize()
    return (pre.cpu(), post.cpu(), la.cpu()) + ((lb.cpu(),) if lb is not None else ())


def check_against_chain(images, labels, table, mean, std, H, W, task, tol):
    got = run_kernel(images, labels, table, mean, std, H, W, task)
    pre, post, labs = R.reference_batch(images, labels, table, mean, std, H, W, task)
    assert (got[0] - pre).abs().max().item() <= tol and (got[1] - post).abs().max().item() <= tol
    for g, w in zip(got[2:], labs):
        assert g.dtype == w.dtype and torch.equal(g, w)


@pytest.mark.parametrize("size", [64, 256])
@pytest.mark.parametrize("consts", ["default", "imagenet"])
def test_zero_table_is_bit_identical_to_the_plain_passes(size, consts):
    dev = torch.device("cuda:0")
    mean, std = CONSTANTS[consts]
    dm, ds = torch.tensor(mean, device=dev), torch.tensor(std, device=dev)
    B = 5
    for task in ("bcd", "scd", "bda"):
        images, labels = R.synth_store(B, size, size, TASK[task][1], seed=size + len(task))
        di, dl = torch.from_numpy(images).to(dev), torch.from_numpy(labels).to(dev)
        pre, post = torch.empty((B, 3, size, size), device=dev), torch.empty((B, 3, size, size), device=dev)
        if task == "bcd":
            want_l = [torch.empty((B, 1, size, size), device=dev)]
            ops.bcd_preprocess(di, dl, None, dm, ds, pre, post, want_l[0], B, size, size)
        else:
            ops.bcd_preprocess(di, None, None, dm, ds, pre, post, None, B, size, size)
            if task == "scd":
                want_l = [torch.empty((B, 3, size, size), dtype=torch.int64, device=dev)]
                ops.scd_label_preprocess(dl, None, want_l[0], B, size, size)
            else:
                want_l = [torch.empty((B, 1, size, size), device=dev), torch.empty((B, size, size), dtype=torch.int64, device=dev)]
                ops.bda_label_preprocess(dl, None, want_l[0], want_l[1], B, size, size)
        torch.cuda.synchronize()
        table = np.zeros((B, 8), dtype=np.int32)
        table[:, 0] = np.arange(B)
        for tab in (table, None):
            got = run_kernel(images, labels, tab, mean, std, size, size, task)
            assert torch.equal(got[0], pre.cpu()) and torch.equal(got[1], post.cpu())
            for g, w in zip(got[2:], want_l):
                assert torch.equal(g, w.cpu())


@pytest.mark.parametrize("task", ["bcd", "scd", "bda"])
@pytest.mark.parametrize("size", [(256, 256), (64, 64), (96, 80)])
def test_crop_path_against_the_torch_chain(task, size):
    """Four offset pairs x eight flip / exchange combinations = 32 samples per call, both constant sets.  Tolerance: 1e-5 at
    the power-of-two extents; 1e-4 at 96 x 80, where torch's f32 source coordinate and the kernel's (cv2's) double one
    differ by an ulp (test_data_cpu.py::test_torch_chain_agrees_with_the_kernel_arithmetic)."""
    H, W = size
    ca = crop_area_of(W)
    offsets = [(0, 0), (ca, ca), (0, ca), (1, max(ca - 1, 0))]
    images, labels = R.synth_store(3, H, W, TASK[task][1], seed=H + W)
    table = np.array([[(3 * k + f) % 3, 1, x1, y1, f & 1, (f >> 1) & 1, (f >> 2) & 1, 0]
                      for k, (x1, y1) in enumerate(offsets) for f in range(8)], dtype=np.int32)
    tol = 1e-5 if (H & (H - 1)) == 0 and (W & (W - 1)) == 0 else 1e-4
    for mean, std in CONSTANTS.values():
        check_against_chain(images, labels, table, mean, std, H, W, task, tol)


def test_gather_with_repeated_and_descending_indices():
    images, labels = R.synth_store(37, 64, 64, 3, seed=37)
    idx = [36, 35, 20, 20, 20, 7, 3, 3, 0, 36, 1, 0, 18, 17, 16, 16]
    rng = np.random.default_rng(1)
    table = np.zeros((16, 8), dtype=np.int32)
    table[:, 0] = idx
    table[:, 1] = rng.integers(0, 2, 16)
    table[:, 2:4] = rng.integers(0, 3, (16, 2)) * table[:, 1:2]
    table[:, 4:7] = rng.integers(0, 2, (16, 3))
    check_against_chain(images, labels, table, *CONSTANTS["imagenet"], 64, 64, "scd", 1e-5)


@pytest.mark.parametrize("task", ["bcd", "bda"])
def test_store_of_another_size_scales_and_crops_in_two_launches(task):
    images, labels = R.synth_store(4, 300, 280, TASK[task][1], seed=300)
    check_against_chain(images, labels, None, *CONSTANTS["default"], 256, 256, task, 1e-5)           # scale only: one launch
    table = np.array([[3, 1, 8, 8, 1, 0, 1, 0], [0, 0, 0, 0, 0, 1, 0, 0], [2, 1, 0, 5, 0, 0, 0, 0], [2, 1, 3, 0, 1, 1, 1, 0]], dtype=np.int32)
    check_against_chain(images, labels, table, *CONSTANTS["imagenet"], 256, 256, task, 1e-5)


def test_argument_refusals_leave_the_outputs_untouched():
    dev = torch.device("cuda:0")
    images, labels = R.synth_store(2, 16, 16, 1, seed=0)
    di, dl = torch.from_numpy(images).to(dev), torch.from_numpy(labels).to(dev)
    dm, ds = torch.tensor(T.DEFAULT_MEAN, device=dev), torch.tensor(T.DEFAULT_STD, device=dev)
    pre, post = torch.full((2, 3, 16, 16), 7.0, device=dev), torch.full((2, 3, 16, 16), 7.0, device=dev)
    lab = torch.full((2, 1, 16, 16), 7.0, device=dev)
    tab = torch.zeros((2, 8), dtype=torch.int32, device=dev)
    p = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    call = lambda *a: L.lib().c3d_augment_gather(*a, None)  # noqa: E731
    full = [p(di), p(dl), p(tab), p(dm), p(ds), p(pre), p(post), p(lab), None, None, L.AUG_BCD, 2, 16, 16, 2, 16, 16]
    def variant(**kw):
        names = ["store", "label_store", "table", "mean", "std", "pre", "post", "label_a", "label_b", "scratch", "task", "N", "Hs", "Ws", "B", "H", "W"]
        a = list(full)
        for k, v in kw.items():
            a[names.index(k)] = v
        return call(*a)
    assert variant(store=None) == -1 and variant(pre=None) == -1 and variant(mean=None) == -1
    assert variant(task=7) == -1 and variant(label_store=None) == -1 and variant(label_b=p(lab)) == -1
    assert variant(task=L.AUG_BDA) == -1                       # BDA needs label_b
    assert variant(table=None, B=3) == -1                      # index = b needs B <= N
    assert variant(H=32, W=32) == -1                           # a table with another store size needs the scratch batch
    assert variant(store=p(di) + 1) == -1                      # odd store address
    assert variant(W=18, Ws=18) == -2                          # W % 4
    assert variant(Ws=2000, table=None) == -2                  # staged rows exceed the LDS
    torch.cuda.synchronize()
    assert (pre == 7).all() and (post == 7).all() and (lab == 7).all()
    with pytest.raises(ValueError):                            # the host check in front of the upload
        validate_augment_table(np.array([[2, 0, 0, 0, 0, 0, 0, 0]], dtype=np.int32), 2, 16, 16)
    assert variant() == 0


def test_loader_epochs_and_placements():
    from change3d_amd.data.resident import DeviceAugmentLoader, ResidentStore
    dev = torch.device("cuda:0")
    images, labels = R.synth_store(21, 64, 64, 2, seed=21)
    hbm = ResidentStore(images, labels, dev)
    host = ResidentStore(images, labels, dev, resident_gb=0.0)
    assert hbm.on_device and hbm.images.is_cuda and not host.on_device and host.images.is_pinned()
    mk = lambda st, train=True: DeviceAugmentLoader(st, 8, "bda", train, seed=4)  # noqa: E731
    a, b, c = mk(hbm), mk(hbm), mk(host)
    assert len(a) == 3
    e0 = [tuple(t.cpu() for t in batch) for batch in a]
    e1 = [tuple(t.cpu() for t in batch) for batch in a]
    assert [x[0].shape[0] for x in e0] == [8, 8, 5] and e0[0][0].shape == (8, 6, 64, 64)
    assert e0[0][1].shape == (8, 1, 64, 64) and e0[0][2].shape == (8, 64, 64) and e0[0][2].dtype == torch.int64
    assert not torch.equal(e0[0][0], e1[0][0])                                       # two epochs differ
    b.set_epoch(1)
    for x, y in zip(e1, b):                                                          # the same (seed, epoch) repeats
        assert all(torch.equal(u, v.cpu()) for u, v in zip(x, y))
    for x, y in zip(e0, c):                                                          # pinned-host placement: the same batches
        assert all(torch.equal(u, v.cpu()) for u, v in zip(x, y))
    # the first training batch is what the chain makes of the epoch's table
    table = a.epoch_table(0)[:8]
    pre, post, labs = R.reference_batch(images, labels, table, T.DEFAULT_MEAN, T.DEFAULT_STD, 64, 64, "bda")
    assert (e0[0][0] - torch.cat([pre, post], dim=1)).abs().max().item() <= 1e-5
    assert torch.equal(e0[0][1], labs[0]) and torch.equal(e0[0][2], labs[1])
    for st in (hbm, host):                                                           # validation: in order, no table
        v = [tuple(t.cpu() for t in batch) for batch in mk(st, train=False)]
        pre, post, labs = R.reference_batch(images, labels, None, T.DEFAULT_MEAN, T.DEFAULT_STD, 64, 64, "bda")
        assert torch.equal(torch.cat([x[0] for x in v]), torch.cat([pre, post], dim=1))
        assert torch.equal(torch.cat([x[2] for x in v]), labs[1])


SCRIPTS = [
    ("train_BCD", "bcd", ["--dataset", "LEVIR-CD", "--max_steps", "6", "--batch_size", "4"], "Val Loss"),
    ("train_SCD", "scd", ["--dataset", "SECOND", "--max_steps", "3", "--batch_size", "4", "--num_class", "5"], "Val loss"),
    ("train_BDA", "bda", ["--dataset", "xBD", "--max_steps", "6", "--batch_size", "4", "--num_class", "5"], "Val Loss"),
]


def test_script_mirrors_train_from_a_png_tree(tmp_path):
    """One child process per script, one after the other, each under its own time limit: finite losses, a validation line,
    exit status 0."""
    for script, task, argv, val_marker in SCRIPTS:
        root = tmp_path / task
        for split, n in (("train", 12), ("val", 4), ("test", 4)):
            write_tree(str(root), task, split=split, n=n, height=64, width=64, seed=len(split))
        cmd = [sys.executable, "-m", f"change3d_amd.scripts.{script}", "--file_root", str(root), "--in_height", "64", "--in_width", "64",
               "--num_workers", "2"] + argv
        if script != "train_SCD":
            cmd += ["--save_dir", str(tmp_path / "exp")]
        out = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
        text = out.stdout + out.stderr
        assert out.returncode == 0, text[-3000:]
        assert val_marker in out.stdout, text[-3000:]
        assert "nan" not in out.stdout.lower() and "inf" not in out.stdout.lower().replace("info", ""), out.stdout[-3000:]
