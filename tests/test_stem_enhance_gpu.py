"""Stem output + enhance without a stored y = relu(bn(u)) / dy (csrc/elementwise.hip `stem_enhance_*`,
model/trainer.py::_ClipStemEnhanceFn, switch `ops.STEM_ENHANCE` / C3D_STEM_ENHANCE).

The fused kernels only move where values are computed, so the yardstick is the sequence they replace:
  * op level   : d, out and g bit-identical to block_out_fwd -> frame_absdiff -> pw_gemm -> enhance_apply and
                 enhance_bwd_mask -> pw_gemm -> enhance_bwd_apply -> block_out_bwd; the BatchNorm-backward sums of both
                 against a float64 torch sum over the same stored tensors (the fused error at most twice the existing
                 kernel's, floor 1e-13 relative: the existing kernel's cross-workgroup f64 atomics are order dependent), and
                 each within the derived absolute bound of tests/test_elementwise_gpu.py
  * model level: Trainer.update_bcd forward + backward, switch on against off: output and loss equal, every parameter
                 gradient within twice the off-vs-off spread of the same test; SCD (T = 5) runs through the new kernels
  * CPU        : which ops each setting of the switch calls, in order (no launch is made)
"""
import pytest
import torch

DEV = "cuda:0"
gpu = pytest.mark.gpu


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")


# ------------------------------------------------------------------------------------------------ op level
def _op_inputs(dtype, T, B, H, W, C=24, seed=0):
    """Random u, a nonzero scale/shift with both signs, a gradient with exact zeros and negatives.  `mean` is NOT the
    mean of u and dout is not centred: the two sums then do not cancel, so an error relative to the sum itself is a
    meaningful figure at every shape (with centred terms the sum is ~sqrt(N) of its terms' magnitude and 'relative'
    measures the cancellation, not the kernel)."""
    g = torch.Generator().manual_seed(1000 * seed + 100 * T + 10 * B + H)
    rn = lambda *s: torch.randn(*s, generator=g)   # noqa: E731
    u = rn(B, T, H, W, C)
    scale = (0.5 + torch.rand(C, generator=g)) * torch.where(torch.rand(C, generator=g) < 0.3, -1.0, 1.0)
    shift = 0.3 * rn(C)
    ss = torch.cat([scale, shift]).float()
    mean = -1.5 + 0.2 * rn(C)
    rstd = 0.5 + torch.rand(C, generator=g)
    mr = torch.cat([mean, rstd]).float()
    dout = rn(B, T, H, W, C) + 1.0
    dout[torch.rand(B, T, H, W, C, generator=g) < 0.1] = 0.0
    assert (dout == 0).any() and (dout < 0).any()
    w = 0.3 * rn(C, C, 1, 1)
    return tuple(t.to(DEV).to(dtype).contiguous() for t in (u, dout)) + (ss.to(DEV), mr.to(DEV), w.to(DEV))


@gpu
@pytest.mark.parametrize("HW", [(20, 28), (64, 64)])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("T", [3, 4, 5])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_stem_enhance_kernels_equal_the_separate_launches(dtype, T, B, HW):
    _need_gpu()
    from change3d_amd import ops
    H, W = HW
    C = 24
    u, dout, ss, mr, w = _op_inputs(dtype, T, B, H, W)
    dt = ops.dt_code(dtype)
    M, M2, hw = B * T * H * W, B * H * W, H * W
    t_pre, t_post, t_mid = 0, T - 1, T // 2       # t_post = K + 1 with K = T - 2 perception frames
    new = lambda *s: torch.empty(*s, dtype=dtype, device=DEV)   # noqa: E731

    # ---- today's chain
    y = torch.empty_like(u)
    ops.block_out_fwd(u, ss, None, None, ops.SC_NONE, y, M, C, dt)
    d0 = new(M2, C)
    ops.frame_absdiff(y, d0, B, T, hw, C, t_pre, t_post, dt)
    e0 = new(M2, C)
    ops.pw_gemm(d0, w, e0, M=M2, K=C, N=C, w_sn=C, w_sk=1, dtype=dt)
    out0 = torch.empty_like(u)
    ops.enhance_apply(y, e0, out0, B, T, hw, C, t_mid, dt)
    de0 = new(M2, C)
    ops.enhance_bwd_mask(dout, e0, de0, B, T, hw, C, t_mid, dt)
    dd0 = new(M2, C)
    ops.pw_gemm(de0, w, dd0, M=M2, K=C, N=C, w_sn=1, w_sk=C, dtype=dt)
    dy = torch.empty_like(u)
    ops.enhance_bwd_apply(dout, y, dd0, dy, B, T, hw, C, t_pre, t_post, dt)
    g0 = torch.empty_like(u)
    ds0 = torch.zeros(2 * C, dtype=torch.float64, device=DEV)
    ops.block_out_bwd(dy, y, u, None, g0, mr, None, ds0, None, M, C, dt)

    # ---- the fused chain (y and dy never exist); NaN-filled outputs: every element must be written
    out1 = torch.full_like(u, float("nan"))
    d1 = torch.full_like(d0, float("nan"))
    ops.stem_enhance_fwd(u, ss, out1, d1, B, T, hw, C, t_pre, t_post, t_mid, dt)
    e1 = new(M2, C)
    ops.pw_gemm(d1, w, e1, M=M2, K=C, N=C, w_sn=C, w_sk=1, dtype=dt)
    ops.stem_enhance_mid(u, ss, e1, out1, B, T, hw, C, t_mid, dt)
    de1 = new(M2, C)
    ops.enhance_bwd_mask(dout, e1, de1, B, T, hw, C, t_mid, dt)
    dd1 = new(M2, C)
    ops.pw_gemm(de1, w, dd1, M=M2, K=C, N=C, w_sn=1, w_sk=C, dtype=dt)
    g1 = torch.full_like(u, float("nan"))
    ds1 = torch.zeros(2 * C, dtype=torch.float64, device=DEV)
    ops.stem_enhance_bwd(dout, u, ss, dd1, mr, g1, ds1, B, T, hw, C, t_pre, t_post, dt)
    torch.cuda.synchronize()

    assert torch.equal(d1, d0)
    assert torch.equal(e1, e0) and torch.equal(dd1, dd0)      # same GEMM launches on equal inputs
    assert torch.equal(out1, out0)
    assert torch.equal(g1, g0)
    assert (g0 != 0).any() and (g0 == 0).any() and (d0 != 0).any()

    # ---- BatchNorm-backward sums: both against a float64 sum over the stored tensors (g is the same tensor for both)
    gd = g0.double().reshape(-1, C)
    chat = (u.double().reshape(-1, C) - mr[:C].double()) * mr[C:].double()
    ref = torch.cat([gd.sum(0), (gd * chat).sum(0)])
    err0, err1 = (ds0 - ref).abs(), (ds1 - ref).abs()
    lim = torch.maximum(2.0 * err0, 1e-13 * ref.abs())
    worst = int((err1 - lim).argmax())
    print(f"dsums {str(dtype)[6:]} T={T} B={B} {H}x{W}: max rel err existing {(err0 / ref.abs()).max().item():.3e} "
          f"fused {(err1 / ref.abs()).max().item():.3e}  max |fused - existing| / |ref| "
          f"{((ds1 - ds0).abs() / ref.abs()).max().item():.3e}")
    assert bool((err1 <= lim).all()), (worst, err1[worst].item(), err0[worst].item(), ref[worst].item())

    # ---- and each against the derived absolute bound of tests/test_elementwise_gpu.py (both launches share one kernel body, so
    # "no worse than the other" alone passes a shared bug): a thread adds n = chain_steps(M, C) terms in f32, three roundings
    # per term, everything after it in f64 -> (n + 3) u of the magnitude sums, n <= 8 at these shapes
    import elementwise_reference as E
    assert E.chain_steps(M, C) <= 8
    mean, rstd = mr[:C].double(), mr[C:].double()
    mag = torch.cat([gd.abs().sum(0), (gd.abs() * (u.double().reshape(-1, C).abs() + mean.abs()) * rstd.abs()).sum(0)])
    r0, r1 = E.sums_ratio(ds0, ref, mag, E.sums_eps(8)), E.sums_ratio(ds1, ref, mag, E.sums_eps(8))
    print(f"dsums error / derived bound: existing {r0:.3f} fused {r1:.3f}")
    assert r0 <= 1.0 and r1 <= 1.0, (r0, r1)


@gpu
def test_stem_enhance_entry_points_refuse_bad_geometry():
    _need_gpu()
    from change3d_amd import _lib, ops
    u = torch.zeros(1, 3, 4, 4, 24, device=DEV)
    ss = torch.ones(48, device=DEV)
    d = torch.zeros(16, 24, device=DEV)
    ds = torch.zeros(48, dtype=torch.float64, device=DEV)
    with pytest.raises(_lib.Change3DHipError):      # t_mid must differ from t_pre / t_post
        ops.stem_enhance_fwd(u, ss, torch.empty_like(u), d, 1, 3, 16, 24, 0, 2, 2, ops.DT_F32)
    with pytest.raises(_lib.Change3DHipError):      # frame index out of range
        ops.stem_enhance_mid(u, ss, d, torch.empty_like(u), 1, 3, 16, 24, 3, ops.DT_F32)
    with pytest.raises(_lib.Change3DHipError):
        ops.stem_enhance_bwd(u, u, ss, d, ss, torch.empty_like(u), ds, 1, 3, 16, 24, 0, 3, ops.DT_F32)


# --------------------------------------------------------------------------------------------- model level
def _trainer(size, k, act_dtype, **kw):
    from oracle import model as om, synth
    from change3d_amd.model.trainer import Trainer
    extra = dict(num_perception_frame=k, dataset="SECOND", num_class=7) if k == 3 else {}
    ref = om.Trainer(om.make_args(size=size, **extra))
    sd = synth.synth_state_dict(ref, seed=16, mask_margin=0.25, **kw)
    args = om.make_args(size=size, **extra)
    args.act_dtype = act_dtype
    net = Trainer(args)
    net.load_state_dict(sd)
    return net.to(DEV).train()


def _count_calls(monkeypatch, ops, names):
    calls = {n: 0 for n in names}
    for n in names:
        def wrapped(*a, _n=n, _f=getattr(ops, n), **k):
            calls[_n] += 1
            return _f(*a, **k)
        monkeypatch.setattr(ops, n, wrapped)
    return calls


NEW_OPS = ("stem_enhance_fwd", "stem_enhance_mid", "stem_enhance_bwd")
OLD_OPS = ("block_out_fwd", "frame_absdiff", "enhance_apply", "enhance_bwd_apply", "block_out_bwd")


@gpu
@pytest.mark.parametrize("act_dtype", [torch.bfloat16, torch.float32])
def test_bcd_step_switch_on_equals_switch_off(act_dtype, monkeypatch):
    """update_bcd forward + backward at B=2, 64x64: output and loss equal; every parameter gradient within twice the
    off-vs-off spread (the largest rel-L2 distance between any two of four switch-off runs from the same state: f32
    leaf-gradient atomics and the f64 statistics atomics make a repeat of the SAME sequence differ by that much)."""
    _need_gpu()
    from change3d_amd import ops
    from change3d_amd.model.utils import BCEDiceLoss
    from oracle import synth
    net = _trainer(64, 1, act_dtype)
    pre, post, tgt = (t.to(DEV) for t in synth.synth_batch(2, 64, seed=3))
    state = {k: v.clone() for k, v in net.state_dict().items()}
    calls = _count_calls(monkeypatch, ops, NEW_OPS + OLD_OPS)

    def run(on):
        monkeypatch.setattr(ops, "STEM_ENHANCE", on)
        net.load_state_dict(state)
        for p in net.parameters():
            p.grad = None
        for n in calls:
            calls[n] = 0
        prob = net.update_bcd(pre, post)
        loss = BCEDiceLoss(prob, tgt)
        loss.backward()
        torch.cuda.synchronize()
        grads = {n: p.grad.detach().double().clone() for n, p in net.named_parameters() if p.grad is not None}
        return prob.detach().clone(), loss.item(), grads, dict(calls)

    offs = [run(False) for _ in range(4)]
    on = run(True)
    assert all(offs[0][3][n] == 0 for n in NEW_OPS) and offs[0][3]["block_out_fwd"] == 1 and offs[0][3]["frame_absdiff"] == 4
    assert all(on[3][n] == 1 for n in NEW_OPS), on[3]
    assert on[3]["block_out_fwd"] == 0 and on[3]["block_out_bwd"] == 0, on[3]
    assert on[3]["frame_absdiff"] == 3 and on[3]["enhance_apply"] == 3 and on[3]["enhance_bwd_apply"] == 3, on[3]
    for o in offs[1:]:
        assert torch.equal(o[0], offs[0][0]) and o[1] == offs[0][1]
    assert torch.equal(on[0], offs[0][0])
    assert on[1] == offs[0][1]
    dist = lambda a, b: ((a - b).norm() / (b.norm() + 1e-30)).item()   # noqa: E731
    g0 = offs[0][2]
    assert set(on[2]) == set(g0)
    worst = (0.0, None)
    for n in g0:
        spread = max(dist(offs[i][2][n], offs[j][2][n]) for i in range(4) for j in range(i))
        dn = dist(on[2][n], g0[n])
        if dn > worst[0]:
            worst = (dn, n, spread)
        assert dn <= 2.0 * spread, (n, dn, spread)
    print(f"{str(act_dtype)[6:]}: largest on-vs-off gradient rel-L2 {worst[0]:.3e} ({worst[1]}, off-vs-off spread {worst[2]:.3e})")


@gpu
def test_scd_step_runs_through_the_fused_stem_enhance(monkeypatch):
    """T = 5 (three perception frames): forward + backward through the new kernels, outputs equal to the old sequence."""
    _need_gpu()
    from change3d_amd import ops
    from oracle import synth
    net = _trainer(64, 3, torch.bfloat16)
    pre, post, _ = (t.to(DEV) for t in synth.synth_batch(2, 64, seed=5))
    state = {k: v.clone() for k, v in net.state_dict().items()}
    calls = _count_calls(monkeypatch, ops, NEW_OPS + OLD_OPS)
    res = {}
    for on in (False, True):
        monkeypatch.setattr(ops, "STEM_ENHANCE", on)
        net.load_state_dict(state)
        for p in net.parameters():
            p.grad = None
        for n in calls:
            calls[n] = 0
        outs = net.update_scd(pre, post)
        sum(o.float().square().mean() for o in outs).backward()
        torch.cuda.synchronize()
        res[on] = ([o.detach().clone() for o in outs], dict(calls),
                   {n: p.grad.detach().clone() for n, p in net.named_parameters() if p.grad is not None})
    assert all(res[True][1][n] == 1 for n in NEW_OPS) and all(res[False][1][n] == 0 for n in NEW_OPS)
    assert res[True][1]["block_out_fwd"] == 0 and res[False][1]["block_out_fwd"] == 1
    for a, b in zip(res[True][0], res[False][0]):
        assert torch.equal(a, b)
    assert set(res[True][2]) == set(res[False][2])
    for n, gr in res[True][2].items():
        assert torch.isfinite(gr).all(), n


# ------------------------------------------------------------------------------------------------------ CPU
LEVEL0_OFF = ["build_clip", "stem_fwd", "bn_finalize", "block_out_fwd", "frame_absdiff", "pw_gemm", "enhance_apply"]
LEVEL0_ON = ["build_clip", "stem_fwd", "bn_finalize", "stem_enhance_fwd", "pw_gemm", "stem_enhance_mid"]
LEVEL_N = ["frame_absdiff", "pw_gemm", "enhance_apply"]
LEVEL_N_BWD = ["frame_scatter", "enhance_bwd_mask", "pw_gemm", "pw_wgrad", "enhance_bwd_apply"]
LEVEL0_BWD_OFF = LEVEL_N_BWD + ["block_out_bwd", "bn_bwd_coef", "stem_bwd_dv", "stem_bwd_wx"]
LEVEL0_BWD_ON = ["frame_scatter", "enhance_bwd_mask", "pw_gemm", "pw_wgrad", "stem_enhance_bwd", "bn_bwd_coef", "stem_bwd_dv",
                 "stem_bwd_wx"]


@pytest.mark.parametrize("on", [False, True])
def test_switch_selects_the_op_sequence(on, monkeypatch):
    """Encoder forward + backward on CPU tensors with every ops.* launcher replaced by a recorder (no library call, no
    values): switch off is today's sequence, block_out_fwd/_EnhanceFn/block_out_bwd at level 0; switch on replaces exactly
    those launches.  The residual stages are stood in for by a strided slice."""
    from change3d_amd import ops
    from change3d_amd.model import trainer as tr
    from oracle import model as om
    seen = []
    launchers = set(LEVEL0_OFF + LEVEL0_ON + LEVEL0_BWD_OFF + LEVEL0_BWD_ON)
    for n in launchers:
        monkeypatch.setattr(ops, n, lambda *a, _n=n, **k: seen.append(_n))
    monkeypatch.setattr(ops, "require_gpu", lambda *a, **k: None)
    monkeypatch.setattr(ops, "side_run", lambda fn, *t: fn())
    monkeypatch.setattr(ops, "STEM_ENHANCE", on)
    monkeypatch.setattr(tr.Encoder, "_clip_stem_ok", lambda self, x, y: True)   # the fused clip + stem path wants a GPU tensor
    net = tr.Trainer(om.make_args(size=32)).train()
    enc = net.encoder
    for i, rep in ((1, 1), (2, 2), (3, 2)):
        monkeypatch.setattr(enc.x3d.blocks[i], "forward", lambda x, _r=rep: x[:, :, :, ::2, ::2].repeat(1, _r, 1, 1, 1))
    x, y = torch.randn(2, 3, 32, 32), torch.randn(2, 3, 32, 32)
    feats = enc(x, y)
    fwd = list(seen)
    assert fwd == (LEVEL0_ON if on else LEVEL0_OFF) + 3 * LEVEL_N
    assert [tuple(f[0].shape) for f in feats] == [(2, 24, 32, 32), (2, 24, 16, 16), (2, 48, 8, 8), (2, 96, 4, 4)]
    del seen[:]
    sum(f[0].sum() for f in feats).backward()
    assert seen == 3 * LEVEL_N_BWD + (LEVEL0_BWD_ON if on else LEVEL0_BWD_OFF)
    assert tuple(enc.perception_frames.grad.shape) == (1, 3, 1, 32, 32)


def test_switch_follows_the_environment():
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for val, want in (("0", "False"), ("1", "True"), (None, "True")):
        env = {k: v for k, v in os.environ.items() if k != "C3D_STEM_ENHANCE"}
        if val is not None:
            env["C3D_STEM_ENHANCE"] = val
        out = subprocess.run([sys.executable, "-c", "from change3d_amd import ops; print(ops.STEM_ENHANCE)"], cwd=root,
                             env=env, capture_output=True, text=True, check=True).stdout.strip()
        assert out == want, (val, out)
