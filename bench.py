#!/usr/bin/env python
"""bench.py — BCD X3D-L train throughput (images/s) on N MI355X, one process per GPU.

    python bench.py --gpus 1 --steps K --warmup W [--dump-outputs DIR] [--full]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...

A "step" = one full training iteration of the reference loop (reference
scripts/train_BCD.py:179-225) on one synthetic LEVIR-CD-shaped batch already resident in HBM:
poly-LR update, Trainer.update_bcd forward (train-mode BN), BCE+Dice, zero_grad, backward,
gradient all-reduce (N>1), Adam, thresholded confusion-matrix update.  Workload = BASELINE.json
configs[1]: BCD X3D-L, bf16 activations, B=32 per GPU, 256x256 pairs, T=3.

Prints ONE JSON line (rank 0).  A plain run does what the headline `value` needs and nothing else: set-up, settling and
warm-up steps, the K timed steps, `--dump-outputs`, the line.  `--full` adds, after the timed steps and without touching
them, `roofline` (dominant kernel, HIP-event timed in one extra step, algorithmic bytes), `also` (short SCD / CC / BCD-f32
runs, a process each) and `cpu_baseline` (the CPU oracle = port of the reference path, timed on host cores).
"""
import argparse
import contextlib
import json
import os
import sys
import time

import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.dont_write_bytecode = True

HBM_PEAK_GBS = 8000.0            # MI355X HBM3E spec peak (MI355X_MICROARCH.md)
A_BCD_ELEMS = 159_784_960        # materialised activation elements per sample
A_SCD_ELEMS = 269_280_000        # same for the SCD path (K=3, T=5; SURVEY.md §8d: 269.28 M)
A_CC_ELEMS = 170_270_000         # change-captioning encoder (blocks 0-4, K=1; SURVEY.md §8d: 170.27 M; decoder < 0.1 %)
DUMP_BUDGET_BYTES = 60 * 10**6   # --dump-outputs writes at most this much array data in all (under 64 MB with the .npy headers)


def parse(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=0, help="per-GPU batch (default: 32 for BCD = BASELINE config, 16 for SCD)")
    ap.add_argument("--task", choices=["bcd", "scd", "cc"], default="bcd",
                    help="bcd = the north-star workload; scd = SURVEY.md 8(f).1 (K=3, T=5, three decoders, 7 classes); "
                         "cc = SURVEY.md 8(f).2 (X3D blocks 0-4 + caption decoder, packed CE, two clipped Adam optimisers)")
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--dtype", choices=["bf16", "f32"], default="bf16")
    ap.add_argument("--graph", action="store_true",
                    help="capture the step in a HIP graph (default: eager launch -- measured faster on MI355X because "
                         "the side-stream weight gradients only overlap the data-gradient chain under eager launch)")
    ap.add_argument("--no-graph", action="store_true", help="(default behaviour; kept for older command lines)")
    ap.add_argument("--input", choices=["device", "host"], default="device",
                    help="host: every step starts from a pinned uint8 host batch (H2D copy + device input pipeline inside the "
                         "timed region) -- the PCIe-inclusive rate quoted in DESIGN.md, never the headline value")
    ap.add_argument("--settle", type=int, default=-1, help="untimed settling steps before the warm-up (default: 40 when --steps >= 10)")
    ap.add_argument("--full", action="store_true",
                    help="after the headline measurement also take everything else this benchmark reports: the per-kernel HIP-event "
                         "profile of one extra step (`roofline`, `--kernel-table`), the short SCD / CC / BCD-f32 runs (`also`) and the "
                         "CPU oracle on the host cores (`cpu_baseline`); about a minute more.  Off by default: a plain run sets up, "
                         "warms up, times the steps, writes `--dump-outputs` and prints the line")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: leave `cpu_baseline` out")
    ap.add_argument("--no-kernel-profile", action="store_true", help="with --full: leave the per-kernel profile step (`roofline`) out")
    ap.add_argument("--no-also", action="store_true",
                    help="with --full: skip the short SCD / CC / BCD-f32 runs appended as `also` (BASELINE configs[3], [4]; "
                         "the parity-grade f32 path's price)")
    ap.add_argument("--windows", type=int, default=1,
                    help="split the K timed steps into this many equal windows (a device sync between them) and report each "
                         "window's ms/step as config.ms_per_step_windows (min / median of a short run); `value` stays K steps / total time")
    ap.add_argument("--dry-run-ranks", type=int, default=0, metavar="N",
                    help="no GPU needed: launch N ranks on the HOST (gloo) through the same self-launch / process-group / GradSync "
                         "code the N-GPU run uses, exchange one synthetic gradient buffer per step, verify the result, and print "
                         "the JSON line with the job geometry (n_gpus, dist_world_size, global_batch) and value = null -- a "
                         "launch-readiness check of the multi-GPU path, never a measurement")
    ap.add_argument("--option", action="append", default=[], metavar="NAME=VALUE",
                    help="c3d_set_option before the run (A/B of the library's run-time options, e.g. FUSE_WGRAD=1)")
    ap.add_argument("--kernel-table", default="", help="with --full: write the per-kernel HIP-event table (JSON) here")
    ap.add_argument("--dump-outputs", default="", metavar="DIR",
                    help="after the timed steps, write what the last timed step computed (loss, network output, parameters after "
                         "the optimiser, their gradients) as DIR/<name>.npy.  That step starts from the seeded weights and a fresh "
                         "optimiser state (three device copies inside the timed region, < 0.01 %% of it), so every input of it is a "
                         "function of the arguments and two builds of the library can be compared output for output")
    a = ap.parse_args(argv)
    if a.kernel_table and (not a.full or a.no_kernel_profile):
        ap.error("--kernel-table is written by the per-kernel profile step: add --full (and drop --no-kernel-profile)")
    return a


def extra_legs(a, world=1):
    """What a run measures besides its headline value, all of it after the timed steps: nothing unless `--full` is given.
    kernel_profile = one extra eager step under HIP events (`roofline`, `--kernel-table`); also = the SCD / CC / BCD-f32
    child runs, appended to the default workload only; cpu_baseline = the CPU oracle on the host cores."""
    return {"kernel_profile": a.full and not a.no_kernel_profile,
            "also": (a.full and not a.no_also and world == 1 and a.task == "bcd" and a.dtype == "bf16" and a.input == "device"
                     and not a.graph),
            "cpu_baseline": a.full and not a.no_cpu_baseline and world == 1}


def usable_cores():
    """Cores this process may really use: scheduler affinity capped by the cgroup CPU quota
    (os.cpu_count() reports the host's 256 logical CPUs inside a small-quota container)."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        with open("/sys/fs/cgroup/cpu.max") as f:
            quota, period = f.read().split()[:2]
        if quota != "max":
            n = min(n, max(1, int(int(quota) / int(period))))
    except OSError:
        pass
    return max(1, min(n, 64))


def _mem_available_gb():
    try:
        with open("/proc/meminfo") as f:
            for line in f:
                if line.startswith("MemAvailable:"):
                    return int(line.split()[1]) / 1e6
    except OSError:
        pass
    return 0.0


def cpu_baseline(size, budget_s=45.0):
    """Reference arithmetic (oracle = torch-CPU fp32 eager NCDHW port of the reference path), same loss /
    Adam, on the usable host cores.  SURVEY.md 8(d) config 1: 32 synthetic pairs as 4 micro-batches of 8
    (fp32 autograd needs ~2.2 GB RSS per sample), one train step per micro-batch, phases timed as the
    reference's own timer does (scripts/train_BCD.py:187-217).  Bounded sample: 1 warm-up micro-batch, then
    micro-batches until the pass of 32 pairs is done or `budget_s` seconds are spent; hosts with < 40 GB of
    free RAM fall back to micro-batches of 2."""
    from oracle import model as om
    from change3d_amd import synthetic as synth
    cores = usable_cores()
    torch.set_num_threads(cores)
    micro = 8 if _mem_available_gb() >= 40.0 else 2
    with contextlib.redirect_stdout(sys.stderr):   # the mirror prints the reference's "pretrained weights" notice
        net = om.Trainer(om.make_args(size=size))
    net.load_state_dict(synth.synth_state_dict(net, seed=16, mask_margin=0.25))
    net.train()
    opt = om.make_adam(net)
    pre, post, tgt = synth.synth_batch(32, size, seed=0)
    phase = [0.0, 0.0, 0.0]

    def one(i, timed=True):
        sl = slice((i * micro) % 32, (i * micro) % 32 + micro)
        t0 = time.time()
        prob = net.update_bcd(pre[sl], post[sl])
        loss = om.bce_dice_loss(prob, tgt[sl])
        t1 = time.time()
        opt.zero_grad()
        loss.backward()
        t2 = time.time()
        opt.step()
        t3 = time.time()
        if timed:
            phase[0] += t1 - t0; phase[1] += t2 - t1; phase[2] += t3 - t2
        return loss.item()

    t0 = time.time()
    one(0, timed=False)
    warm = time.time() - t0
    done, t0 = 0, time.time()
    n_pass = 32 // micro
    if warm > budget_s:  # very slow host: the warm-up step is the sample
        done, dt = 1, warm
    else:
        while done < n_pass and time.time() - t0 < budget_s:
            one(done)
            done += 1
        dt = time.time() - t0
    return {"value": round(micro * done / dt, 4), "unit": "images/s", "cores": cores, "kind": "port",
            "phases_s": {"fwd_loss": round(phase[0], 2), "bwd": round(phase[1], 2), "optimizer": round(phase[2], 3)},
            "sample": f"{done} of the {n_pass} micro-batches of {micro} that make SURVEY 8(d) config 1 (32 {size}x{size} pairs), "
                      f"one train step each (1 warm-up micro-batch, {warm:.1f}s), fp32, torch-CPU eager NCDHW, {cores} threads"}


def dump_outputs(dirname, tensors):
    """`--dump-outputs`: DIR/<name>.npy for each tensor, float64 kept, everything else as float32, DUMP_BUDGET_BYTES in
    all.  Smallest first, each array may take an equal share of the bytes still free; one that is larger is written as a
    fixed sample of its flattened elements (ascending indices drawn from RandomState(0), a function of the sizes only),
    so the same arguments give the same elements in every run and every build.
    Returns {name: [elements written, elements of the tensor]}."""
    import numpy as np
    os.makedirs(dirname, exist_ok=True)
    arrays = {}
    for name, t in tensors.items():
        arr = t.detach().to(torch.float64 if t.dtype == torch.float64 else torch.float32).cpu().numpy()
        arrays[name] = arr.reshape(1) if arr.ndim == 0 else arr
    left, written = DUMP_BUDGET_BYTES, {}
    for i, (name, arr) in enumerate(sorted(arrays.items(), key=lambda kv: kv[1].nbytes)):
        total, keep = arr.size, left // (len(arrays) - i) // arr.itemsize
        if total > keep:
            arr = arr.reshape(-1)[np.sort(np.random.RandomState(0).choice(total, keep, replace=False))]
        np.save(os.path.join(dirname, name + ".npy"), arr)
        left -= arr.nbytes
        written[name] = [int(arr.size), int(total)]
    return written


def pmc_traffic(entry):
    """HBM bytes per launch of `entry` from the committed counter summary (rocprofv3 --pmc cannot run
    inside this process): profiles/r*_pmc_traffic.json, produced by tools/profile_round.sh from separate
    FETCH_SIZE / WRITE_SIZE passes of this same workload and corrected as the MI355X guide prescribes."""
    import glob
    files = sorted(glob.glob(os.path.join(os.path.dirname(os.path.abspath(__file__)), "profiles", "r*_pmc_traffic.json")))
    if not files:
        return {}
    try:
        with open(files[-1]) as f:
            d = json.load(f)
        e = d["by_entry"][entry]
        from change3d_amd._lib import csrc_digest
        if d.get("csrc_sha16") != csrc_digest():   # counters of other kernels than the ones that just ran: not this run's traffic
            return {"traffic": None,
                    "traffic_source": f"profiles/{os.path.basename(files[-1])} was taken at kernel sources {d.get('csrc_sha16')}, this "
                                      f"run has {csrc_digest()}: re-run tools/profile_round.sh"}
        return {"traffic": int(e["hbm_bytes_per_launch"]),
                "traffic_source": f"profiles/{os.path.basename(files[-1])} (kernel sources {d['csrc_sha16']} = this run's): {d['corrections']}"}
    except (KeyError, ValueError, OSError):
        return {}


def also_runs(a):
    """`--full`: short runs of the other workloads BASELINE.json names, each in its own process after the headline measurement
    (30 timed steps in three windows of 10 after 40 settling + 5 warm-up steps -- `value` is the 30-step mean, the per-window
    ms/step give min / median; 120 s per child and 300 s in all, so the headline line is never held up for long; a run whose
    windows disagree by more than 5 % is measured once more and the better-agreeing run is kept, with the other recorded): SCD (configs[3], B=16, T=5), CC (configs[4], B=16) in bf16, and the BCD workload on the
    f32 storage path -- the path every bit-exact / 1e-4 parity statement is made on -- so that it has a price."""
    import subprocess
    res = {}
    t_start, budget_s = time.time(), 300.0   # wall budget for all three children (+ at most one re-measurement each): the headline line must not wait longer
    for key, extra in (("scd", ["--task", "scd"]), ("cc", ["--task", "cc"]), ("bcd_f32", ["--task", "bcd", "--dtype", "f32"])):
        left = budget_s - (time.time() - t_start)
        if left < 30.0:
            res[key] = {"error": "skipped: the auxiliary runs' wall budget was spent"}
            continue
        cmd = [sys.executable, os.path.abspath(__file__), "--gpus", "1", "--steps", "30", "--warmup", "5", "--size", str(a.size),
               "--windows", "3"] + extra   # plain runs: the headline figure of each and nothing more
        try:
            best = None
            for attempt in (0, 1):
                left = budget_s - (time.time() - t_start)
                if attempt and left < 40.0:
                    break
                r = subprocess.run(cmd, capture_output=True, text=True, timeout=min(120.0, left))
                d = json.loads(r.stdout.strip().splitlines()[-1])
                w = d["config"].get("ms_per_step_windows") or [d["ms_per_step"]]
                spread = max(w) / max(min(w), 1e-9)
                cand = {"value": d["value"], "unit": d["unit"], "ms_per_step": d["ms_per_step"], "steps": d["steps"],
                        "warmup": d["warmup"], "dtype": d["dtype"], "global_batch": d["config"]["global_batch"],
                        "workload": d["config"]["workload"], "step_roofline_frac": d["step_roofline"]["frac"],
                        "ms_per_step_windows": d["config"].get("ms_per_step_windows")}
                if attempt:
                    cand["rerun_of_disturbed_run"] = {"ms_per_step_windows": best[1]["ms_per_step_windows"], "value": best[1]["value"]}
                if best is None or spread < best[0]:
                    best = (spread, cand)
                # three windows of ten steps that disagree by more than 5 % mean the box was disturbed during the run (seen once
                # in round 4: 25.3 / 28.1 / 31.1 ms where every other run gives 25.0 +- 0.1): measure once more, keep the run whose
                # windows agree better, and say so in the record
                if spread <= 1.05:
                    break
            res[key] = best[1]
        except Exception as e:  # noqa: BLE001  (an auxiliary number must never cost the headline line)
            res[key] = {"error": f"{type(e).__name__}: {str(e)[:200]}"}
    return res


def self_launch(a):
    """`python bench.py --gpus N` without a launcher: re-exec under torch.distributed.run, one rank per GPU
    (the driver's own multi-GPU command line is exactly this)."""
    import socket
    import subprocess
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={a.gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    raise SystemExit(subprocess.call(cmd, env=env))


def dry_run_ranks(a):
    """`--dry-run-ranks N` (CPU, gloo): everything of an N-rank job except the model step -- launcher, rendezvous on
    127.0.0.1, the world-size check, the BCD parameter arena in all-reduce order, the overlapped tail bucket + head
    all-reduce + 1/world of `GradSync` on rank-dependent synthetic gradients (checked against the closed form), the
    max-over-ranks timing reduction and the JSON line."""
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    if world != a.gpus:
        raise SystemExit(f"--dry-run-ranks {a.gpus} but WORLD_SIZE={world}")
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    dist.init_process_group("gloo")
    from change3d_amd.synthetic import make_args
    from change3d_amd.model.trainer import Trainer
    from change3d_amd.parallel import setup_data_parallel
    with contextlib.redirect_stdout(sys.stderr):
        net = Trainer(make_args(size=a.size))
    arena, sync = setup_data_parallel(net, torch.device("cpu"), overlap=True)
    if dist.get_world_size() != a.gpus or sync.world != a.gpus:
        raise SystemExit(f"process group has {dist.get_world_size()} ranks (GradSync {sync.world}) but --dry-run-ranks {a.gpus}")
    ok = True
    base = torch.linspace(-1.0, 1.0, arena.numel)
    sync.timing = True
    dist.barrier()
    t0 = time.perf_counter()
    for it in range(a.steps):
        arena.flat_grad.copy_(base * (rank + 1 + it))          # rank r contributes (r + 1 + it) * base
        sync.launch_tail()                                     # what the res4 stage hook does from inside backward
        sync.finish()
        want = base * (sum(r + 1 + it for r in range(world)) / world)
        ok = ok and bool(torch.allclose(arena.flat_grad, want, rtol=1e-5, atol=1e-6))
    mine = time.perf_counter() - t0
    dist.barrier()
    tt = torch.tensor([time.perf_counter() - t0, 0.0 if ok else 1.0, mine, -mine], dtype=torch.float64)
    dist.all_reduce(tt, op=dist.ReduceOp.MAX)
    if rank == 0:
        batch = a.batch if a.batch > 0 else 32
        print(json.dumps({"metric": "train images/sec (256x256 pairs, X3D-L BCD)", "value": None, "unit": "images/s", "dry_run": True,
                          "n_gpus": world, "steps": a.steps, "warmup": a.warmup, "ms_per_step": None, "higher_is_better": True,
                          "scaling": "weak", "vs_baseline": None, "dtype": a.dtype, "data": "synthetic",
                          "config": {"workload": "DRY RUN on host cores (gloo): launcher + process group + gradient exchange only",
                                     "global_batch": batch * world, "parallelism": f"dp{world}", "dist_world_size": dist.get_world_size(),
                                     "dist_backend": dist.get_backend(), "exchange_floats": arena.numel,
                                     "exchange_verified": tt[1].item() == 0.0,
                                     "exchange_ms_per_step_host": round(tt[0].item() / max(a.steps, 1) * 1e3, 3)},
                          "dp": {"ms_per_step_rank_max": round(tt[2].item() / max(a.steps, 1) * 1e3, 3),
                                 "ms_per_step_rank_min": round(-tt[3].item() / max(a.steps, 1) * 1e3, 3),
                                 "exposed_comm_ms_per_step": sync.exposed_ms_per_step()}}), flush=True)
    dist.destroy_process_group()
    if tt[1].item() != 0.0:
        raise SystemExit("dry run: the reduced gradient buffer is wrong")


def main():
    a = parse()
    if a.dry_run_ranks > 0:
        a.gpus = a.dry_run_ranks
        if "WORLD_SIZE" not in os.environ:
            self_launch(a)
        return dry_run_ranks(a)
    if a.gpus > 1 and "WORLD_SIZE" not in os.environ:
        self_launch(a)
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if a.gpus != world:
        raise SystemExit(f"--gpus {a.gpus} but WORLD_SIZE={world}: refusing to report a line for a different job size")
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X (the hot path has no CPU fallback)")
    # (test hooks: C3D_DIST_DEVICE / C3D_DIST_BACKEND let a 1-GPU box run the N>1 code path with gloo)
    local = int(os.environ.get("C3D_DIST_DEVICE", local))
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        backend = os.environ.get("C3D_DIST_BACKEND", "nccl")
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=dev)
        else:
            dist.init_process_group(backend)

    from change3d_amd import synthetic as synth   # deterministic synthetic weights / batches (no oracle in the product leg)
    from change3d_amd.synthetic import make_args
    from change3d_amd import ops
    from change3d_amd.model.trainer import Trainer
    from change3d_amd.model.utils import BCEDiceLoss, FusedAdam, adjust_learning_rate
    from change3d_amd.parallel import broadcast_module_state, setup_data_parallel
    from change3d_amd.utils.metric_tool import ConfuseMatrixMeter

    for ov in a.option:
        name, val = ov.split("=")
        ops.set_option(getattr(ops, "OPT_" + name.upper()), int(val))
    act = torch.bfloat16 if a.dtype == "bf16" else torch.float32
    scd, cc = a.task == "scd", a.task == "cc"
    if a.batch <= 0:
        a.batch = 16 if (scd or cc) else 32
    if cc:
        margs = synth.make_cc_args(size=a.size, vocab_size=501, dropout=0.1)   # reference scripts/train_CC.py defaults
    else:
        margs = make_args(num_perception_frame=3, size=a.size, dataset="SECOND", num_class=7) if scd else make_args(size=a.size)
    margs.act_dtype = act
    margs.lr_mode, margs.lr, margs.max_epochs, margs.step_loss = "poly", 2e-4, 1, 100
    with contextlib.redirect_stdout(sys.stderr):   # stdout carries exactly one JSON line
        net = Trainer(margs)
    sd0 = synth.synth_state_dict(net, seed=16, mask_margin=0.25)
    if cc:
        sd0["decoder.position_encoding.pe"] = net.state_dict()["decoder.position_encoding.pe"].clone()   # constant table
    net.load_state_dict(sd0)
    net = net.to(dev).train()
    broadcast_module_state(net)
    if cc:   # two optimisers (reference scripts/train_CC.py:436-458); gradients exchanged as two flat buffers, both
        # launched from the end of res5's backward (change3d_amd/parallel.py::setup_data_parallel_cc)
        from change3d_amd.model.utils import clip_gradient
        from change3d_amd.model.caption_decoder import packed_cross_entropy
        from change3d_amd.parallel import setup_data_parallel_cc
        (arena, _enc_sync), (dec_arena, dec_sync), sync = setup_data_parallel_cc(net, dev, overlap=True)
    else:
        arena, sync = setup_data_parallel(net, dev, overlap=True)
    dist_world = dist.get_world_size() if world > 1 else 1
    if dist_world != a.gpus or sync.world != a.gpus:
        raise SystemExit(f"process group has {dist_world} ranks (GradSync {sync.world}) but --gpus {a.gpus}")
    if cc:
        opt = FusedAdam(arena, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-5, capturable=True)
        dec_opt = FusedAdam(dec_arena, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-5, capturable=True)
        caps, caplens = (t.to(dev) for t in synth.synth_captions(a.batch, seed=rank, vocab_size=501))
    else:
        opt = FusedAdam(arena, lr=margs.lr, capturable=True)
    opts = [opt, dec_opt] if cc else [opt]
    seeded = [o.arena.flat_param.clone() for o in opts] if a.dump_outputs else None
    meter = ConfuseMatrixMeter(2)
    pre, post, tgt = (t.to(dev) for t in synth.synth_batch(a.batch, a.size, seed=rank))
    if scd:
        from change3d_amd.model.utils import ChangeSimilarity, CrossEntropyLoss2d
        from change3d_amd.scripts.train_SCD import scd_loss
        labels = synth.synth_scd_labels(a.batch, a.size, seed=rank).to(dev)
        seg_loss, sim_loss = CrossEntropyLoss2d(ignore_index=0), ChangeSimilarity()
    MAX_ITER = 80000
    state = {"it": 0, "loss": None, "prob": None}
    host_in = None
    if a.input == "host":
        if scd or cc:
            raise SystemExit("--input host is implemented for the BCD task")
        import numpy as np
        from change3d_amd.data.transforms import DeviceBatchTransform, draw_augmentation_flags
        rng = np.random.RandomState(rank)
        host_in = (torch.from_numpy(rng.randint(0, 256, (a.batch, a.size, a.size, 6), dtype=np.uint8)).pin_memory(),
                   torch.from_numpy((rng.rand(a.batch, a.size, a.size) < 0.3).astype(np.uint8) * 255).pin_memory(),
                   torch.from_numpy(draw_augmentation_flags(a.batch, rng)).pin_memory(), DeviceBatchTransform(dev))

    def fwd_bwd():
        opt.zero_grad()
        if cc:    # reference scripts/train_CC.py:111-145
            dec_opt.zero_grad()
            feat = net.update_cc(pre, post)
            Bc, Cc, Hc, Wc = feat.shape
            logits = net.decoder.logits_seq_first(feat.permute(2, 3, 0, 1).reshape(Hc * Wc, Bc, Cc), caps)
            loss, stats = packed_cross_entropy(logits, caps, caplens, 501, ignore_index=0, return_stats=True)
            loss.backward()
            sync.finish()           # both buffers (the decoder's and res5's buckets were launched from inside backward)
            clip_gradient(dec_opt, 5.0)
            dec_opt.launch(*dec_hp)
            return loss.detach(), stats
        if scd:   # reference scripts/train_SCD.py:216-233
            masks = net.update_scd(pre, post)
            loss = scd_loss(seg_loss, sim_loss, masks, labels)[0]
            loss.backward()
            return loss.detach(), masks[2].detach()
        p_, q_, t_ = pre, post, tgt
        if host_in is not None:   # reference data/transforms.py:100-154 on the device, from a pinned uint8 batch
            p_, q_, t_ = host_in[3](host_in[0], host_in[1], host_in[2])
        prob = net.update_bcd(p_, q_)
        loss = BCEDiceLoss(prob, t_)
        loss.backward()
        meter.update_cm_device(prob, t_)
        return loss.detach(), prob.detach()

    graph = None
    use_graph = a.graph and not a.no_graph and world == 1  # N>1: the overlapped all-reduce is issued from inside backward
    torch.autograd.graph.set_warn_on_accumulate_grad_stream_mismatch(False)
    dec_hp = (0.0, 1.0, 1.0)
    if cc:
        use_graph = False
        dec_hp = dec_opt.prepare_step()
    else:
        adjust_learning_rate(margs, opt, 0, 0, MAX_ITER)
    opt.prepare_step()
    if use_graph:
        # every pre-capture step runs on the capture stream (autograd's AccumulateGrad nodes remember
        # the stream they were created on; a default-stream step before capture breaks it)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        try:
            with torch.cuda.stream(side):
                for _ in range(2):
                    state["loss"], state["prob"] = fwd_bwd()
                    opt.launch()
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=side):
                state["loss"], state["prob"] = fwd_bwd()
                opt.launch()
            torch.cuda.synchronize()
        except Exception as e:  # noqa: BLE001
            if rank == 0:
                print(f"[bench] HIP graph capture failed ({type(e).__name__}: {e}); running eagerly", file=sys.stderr)
            graph = None
            torch.cuda.synchronize()
    else:
        state["loss"], state["prob"] = fwd_bwd()
        if cc:
            clip_gradient(opt, 5.0)     # (the exchange of both buffers was completed inside fwd_bwd)
        else:
            sync.finish()
        opt.launch()
        torch.cuda.synchronize()

    def step():
        nonlocal dec_hp
        h0 = time.perf_counter()
        if cc:
            dec_hp = dec_opt.prepare_step()      # StepLR(900, gamma=1): constant learning rate
        else:
            adjust_learning_rate(margs, opt, 0, state["it"], MAX_ITER)
        opt.prepare_step()
        if graph is not None:
            graph.replay()
        else:
            state["loss"], state["prob"] = fwd_bwd()
            if cc:
                clip_gradient(opt, 5.0)
            else:
                sync.finish()
            opt.launch()
        state["host_s"] = state.get("host_s", 0.0) + time.perf_counter() - h0   # enqueue only (no read-back)
        state["it"] += 1
        if state["it"] % 5 == 0:  # reference prints (and syncs on) the loss every 5 iterations
            state["last_loss"] = float(state["loss"])

    def rewind():
        """--dump-outputs: the synthetic weights and a fresh Adam state again (in-place device copies, no sync), so that the
        step that follows computes a function of the command line alone.  Without it the dump is not comparable between two
        runs of ONE build: the chained Adam steps of a run (65 with the default arguments) on this train-mode-BatchNorm
        network amplify the last-bit differences of the f32 atomics (one step: gradients reproducible to 6e-7) to O(1)
        differences of the output."""
        for o, w0 in zip(opts, seeded):
            o.arena.flat_param.copy_(w0)
            o.exp_avg.zero_()
            o.exp_avg_sq.zero_()
            o.step_count = 0
        ops.bump_weights_version()
        torch.default_generator.manual_seed(0)   # the caption decoder draws its dropout seed from torch's CPU generator

    # Settling steps (untimed, reported as config.settle_steps): the first process on a freshly leased box runs its first
    # seconds with cold CPU caches and ramping GPU clocks (measured: 35.0 vs 32.8 ms per step, host enqueue 15.9 vs
    # 6.5 ms); a fixed number of extra steps, the same on every rank, before the W warm-up steps the caller asked for.
    settle = a.settle if a.settle >= 0 else (40 if a.steps >= 10 else 0)
    for _ in range(settle):
        step()
    for _ in range(a.warmup):
        step()
    torch.cuda.synchronize()
    from change3d_amd.hostopt import freeze_gc
    freeze_gc()   # as the training scripts do after their first iterations: no 30 ms full collection inside the loop (hostopt.py)
    all_syncs = [s_ for s_ in getattr(sync, "syncs", [sync])]
    if world > 1:
        for s_ in all_syncs:           # self-diagnosis of the exchange: event pairs per step, read after the timed region
            s_.timing, s_.samples = True, []
        dist.barrier()
    torch.cuda.synchronize()
    state["host_s"] = 0.0
    t0 = time.perf_counter()
    windows = []
    nwin = a.windows if (a.windows > 1 and world == 1 and a.steps % a.windows == 0) else 1
    for w_ in range(nwin):
        for k_ in range(a.steps // nwin):
            if a.dump_outputs and w_ == nwin - 1 and k_ == a.steps // nwin - 1:
                rewind()   # the last timed step is the one that is dumped
            step()
        if nwin > 1:
            torch.cuda.synchronize()
            windows.append(time.perf_counter())
    t_enqueued = state["host_s"]   # host time spent enqueueing the steps (loss read-backs excluded)
    torch.cuda.synchronize()
    own_elapsed = time.perf_counter() - t0      # this rank's K steps, before it waits for the others
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    dp_diag = None
    if world > 1:
        tt = torch.tensor([elapsed, own_elapsed, -own_elapsed], dtype=torch.float64, device=dev)
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        elapsed = float(tt[0].item())
        for s_ in all_syncs:
            s_.timing = False
        # why the scaling efficiency is what it is: the spread of the ranks' own step times (a straggler shows here) and the
        # communication the compute stream actually waited for (rank 0's event pairs: head = the non-overlapped all-reduce,
        # tail_wait = what was left of the overlapped bucket when backward + head were done)
        dp_diag = {"ms_per_step_rank_max": round(float(tt[1].item()) / a.steps * 1e3, 3),
                   "ms_per_step_rank_min": round(-float(tt[2].item()) / a.steps * 1e3, 3),
                   "exposed_comm_ms_per_step": [s_.exposed_ms_per_step() for s_ in all_syncs]}
    final_loss = float(state["loss"])
    if not (final_loss == final_loss):
        raise SystemExit("loss is NaN")
    dumped = None
    if a.dump_outputs and rank == 0:
        # here, before the kernel-profile step below runs the optimiser once more: what the last TIMED step (run from
        # the seeded state, see rewind) returned (loss, output) and left behind (parameters after Adam, the gradients it consumed)
        tensors = {"loss": state["loss"], "output": state["prob"], "params": arena.flat_param, "grads": arena.flat_grad}
        if cc:
            tensors.update({"decoder_params": dec_arena.flat_param, "decoder_grads": dec_arena.flat_grad})
        dumped = dump_outputs(a.dump_outputs, tensors)

    ms_per_step = elapsed / a.steps * 1e3
    value = a.batch * world * a.steps / elapsed
    es = 2 if a.dtype == "bf16" else 4
    bytes_per_sample = 5 * (A_SCD_ELEMS if scd else A_CC_ELEMS if cc else A_BCD_ELEMS) * es * (a.size / 256.0) ** 2
    out = {
        "metric": f"train images/sec (256x256 pairs, X3D-L {a.task.upper()})", "value": round(value, 2), "unit": "images/s",
        "n_gpus": world, "steps": a.steps, "warmup": a.warmup, "ms_per_step": round(ms_per_step, 3),
        "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": a.dtype, "data": "synthetic",
        "config": {"workload": f"{a.task.upper()} X3D-L {a.dtype}, B={a.batch}/GPU, {a.size}x{a.size} synthetic "
                               f"{'SECOND' if scd else 'LEVIR-CC' if cc else 'LEVIR-CD'}-shaped "
                               f"pairs{' + 52-token captions (vocab 501, dropout 0.1)' if cc else ''}, T={5 if scd else 3}, train step "
                               f"(fwd+{'0.5*CE+BCE/Dice+ChangeSimilarity' if scd else 'packed CE' if cc else 'BCE/Dice'}"
                               f"+bwd+{'clip+2xAdam' if cc else 'Adam'})",
                   "global_batch": a.batch * world, "parallelism": f"dp{world}", "dist_world_size": dist_world,
                   "dist_backend": (dist.get_backend() if world > 1 else None),
                   "hip_graph": graph is not None, "full": a.full, "settle_steps": settle, "input": "resident in HBM" if a.input == "device" else
                   "pinned uint8 host batch: H2D + device input pipeline every step (PCIe-inclusive, not the headline)",
                   "final_loss": round(final_loss, 5),
                   "host_enqueue_ms_per_step": round(t_enqueued / a.steps * 1e3, 3),
                   "ms_per_step_windows": ([round((t_ - p_) / (a.steps // nwin) * 1e3, 3) for p_, t_ in zip([t0] + windows[:-1], windows)]
                                           if nwin > 1 else None)},
        "dp": dp_diag, "dumped_outputs": dumped,
        "step_roofline": {"bound": "hbm", "algorithmic_bytes_per_sample": bytes_per_sample,
                          "achieved": round(value / world * bytes_per_sample / 1e9, 1), "peak": HBM_PEAK_GBS,
                          "unit": "GB/s", "frac": round(value / world * bytes_per_sample / 1e9 / HBM_PEAK_GBS, 4)},
    }

    # ---- `--full` only, from here to the print: a plain run has its line already
    # ---- dominant kernel, timed live with HIP events on the launch stream (one extra eager step)
    legs = extra_legs(a, world)
    if rank == 0 and legs["kernel_profile"]:
        net.encoder.x3d.blocks[3].post_backward = None
        net.encoder.x3d.blocks[4].post_backward = None
        # this extra step runs on rank 0 ONLY: no collective may be issued from it (a peer-less all-reduce would block
        # until the RCCL watchdog fires and the JSON line would never be printed) -- every GradSync becomes a no-op
        for s_ in getattr(sync, "syncs", [sync]):
            s_.world = 1
        if cc:
            dec_hp = dec_opt.prepare_step()
        # per-kernel durations are taken with the side stream OFF: launches then do not overlap, so an event pair brackets
        # exactly one kernel (profiles/*_rocprof_kernel_stats_serial.json is the rocprofv3 trace of the same mode; the
        # timed region above runs with the overlap ON).  The residual stages are timed by the C++ stage driver itself
        # (c3d_prof_begin: the product launch sequence, not a copy of it), everything else by the ctypes wrappers.
        ops.profile_begin(serial=True)
        fwd_bwd()
        opt.launch()
        prof = ops.profile_end()
        tot = sum(v["ms_total"] for v in prof.values())
        table = sorted(prof.items(), key=lambda kv: -kv[1]["ms_total"])
        name, d = table[0]
        ach = d["bytes_total"] / max(d["ms_total"], 1e-9) / 1e6
        out["roofline"] = {"bound": "hbm", "kernel": name, "launches_per_step": d["launches"],
                           "avg_us_per_launch": round(d["ms_total"] / d["launches"] * 1e3, 2),
                           "algorithmic_bytes_per_launch": round(d["bytes_total"] / d["launches"]),
                           "achieved": round(ach, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                           "frac": round(ach / HBM_PEAK_GBS, 4), "traffic": None,
                           "share_of_kernel_time": round(d["ms_total"] / max(tot, 1e-9), 3),
                           "timing": "HIP events on the launch stream, one eager step with the side stream off"}
        if not scd and not cc:   # the committed counter summary is a BCD run
            out["roofline"].update(pmc_traffic(name))
        rows = [{"kernel": k, "launches": v["launches"], "ms_total": round(v["ms_total"], 3),
                 "GBps": round(v["bytes_total"] / max(v["ms_total"], 1e-9) / 1e6, 1)} for k, v in table]
        out["kernel_time_ms_eager_step"] = round(tot, 3)
        if a.kernel_table:
            ops.profile_begin(serial=True, detail=True)   # second eager step: pointwise kernels keyed by shape/mode
            fwd_bwd()
            opt.launch()
            shapes = ops.profile_end()
            srows = [{"kernel": k, "launches": v["launches"], "ms_total": round(v["ms_total"], 3),
                      "GBps": round(v["bytes_total"] / max(v["ms_total"], 1e-9) / 1e6, 1)}
                     for k, v in sorted(shapes.items(), key=lambda kv: -kv[1]["ms_total"]) if "[" in k]
            with open(a.kernel_table, "w") as f:
                json.dump({"ms_per_step": ms_per_step, "kernels": rows, "pointwise_by_shape": srows}, f, indent=1)
        for r in rows:
            print(f"[kernels] {r['kernel']:24s} x{r['launches']:4d} {r['ms_total']:9.3f} ms {r['GBps']:8.1f} GB/s",
                  file=sys.stderr)
    if rank == 0 and legs["also"]:
        out["also"] = also_runs(a)
    if rank == 0 and legs["cpu_baseline"]:
        out["cpu_baseline"] = cpu_baseline(a.size) if not (scd or cc) else None   # the CPU leg times the BCD oracle only
    if rank == 0:
        print(json.dumps(out), flush=True)
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
