"""Four-frame (T = 4: building damage assessment, num_perception_frame = 2) instantiations of the depthwise 3x3x3 kernels,
through the C ABI: against torch float64 conv3d on the CPU with the tolerances tests/test_ops_gpu.py uses for T = 3 / 5, and
C3D_OPT_DW_T4 = 1 (four-frame instantiations) against 0 (the five-frame instantiation with a zero fifth frame).

The tap order per output is the same in both instantiations (the fifth frame only ever contributed products with zero), so
outputs and data gradients must be bit-identical; per-sample statistics and the weight gradient are sums over tiles whose
walks differ in the stride-1 forward (same 4 x 16 tiles, other walk lengths are possible) and whose f32 / f64 atomics
commute up to rounding: compared to f32 rounding."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DTYPES = [torch.float32, torch.bfloat16]
T4 = 4


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")


def rnd(shape, seed, scale=1.0):
    g = np.random.default_rng(seed)
    return torch.from_numpy((g.standard_normal(shape) * scale).astype(np.float32))


def tol(dtype):
    return (2e-5, 2e-5) if dtype == torch.float32 else (3e-2, 3e-2)


def close(a, b, dtype, what, scale=1.0):
    at, rt = tol(dtype)
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    err = (a - b).abs()
    lim = at * scale + rt * b.abs()
    bad = (err > lim).sum().item()
    assert bad == 0, f"{what}: {bad}/{err.numel()} out of tolerance, max err {err.max().item():.3e}, ref max {b.abs().max().item():.3e}"


def padc(t, cp):
    c = t.shape[-1]
    return t if c == cp else F.pad(t, (0, cp - c))


def q(t, dtype):
    return t.to(dtype).float()


def _bits(t):
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int32)


def _case(B, H, W, C, stride, dtype, seed):
    """Inputs of one forward + fused-backward call and their float64 references."""
    from change3d_amd import ops
    T = T4
    Cp = ops.cpad(C)
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    a = q(rnd((B, T, H, W, C), seed), dtype)
    scale, shift = rnd((C,), seed + 1).abs() + 0.5, rnd((C,), seed + 2, 0.3)
    w = rnd((C, 1, 3, 3, 3), seed + 3, 0.3)
    a_r = a.double().requires_grad_(True)
    w_r = w.double().requires_grad_(True)
    ra = torch.relu(a_r * scale.double() + shift.double()).permute(0, 4, 1, 2, 3)
    bref = F.conv3d(ra, w_r, stride=(1, stride, stride), padding=1, groups=C)   # [B,C,T,Ho,Wo]
    d = dict(B=B, T=T, H=H, W=W, C=C, Cp=Cp, Ho=Ho, Wo=Wo, stride=stride, dtype=dtype, a=a, scale=scale, a_r=a_r, w_r=w_r,
             bref=bref)
    d["ss"] = torch.cat([padc(scale, Cp), padc(shift, Cp)]).to(DEV)
    d["ad"] = padc(a, Cp).to(DEV, dtype).contiguous()
    d["wd"] = w.to(DEV).contiguous()
    d["t1"] = q(rnd((B, T, Ho, Wo, C), seed + 4), dtype)
    d["cA"], d["cC"], d["cB"] = rnd((C,), seed + 5), rnd((C,), seed + 6, 0.1), rnd((B, C), seed + 7, 0.1)
    d["mean_a"], d["rstd_a"] = rnd((C,), seed + 8, 0.5), rnd((C,), seed + 9).abs() + 0.5
    d["mr"] = torch.cat([padc(d["mean_a"], Cp), padc(d["rstd_a"], Cp)]).to(DEV)
    return d


def _run(d):
    """c3d_dw333_fwd, then c3d_dw333_bwd_fused on the forward's own output: (b, nc, t2, dsums, dw) on the device."""
    from change3d_amd import ops
    B, T, H, W, C, Cp, dtype, stride = d["B"], d["T"], d["H"], d["W"], d["C"], d["Cp"], d["dtype"], d["stride"]
    b = torch.full((B, T, d["Ho"], d["Wo"], Cp), float("nan"), dtype=dtype, device=DEV)
    nc = torch.zeros(B * Cp * 2, dtype=torch.float64, device=DEV)
    ops.dw_fwd(d["ad"], d["ss"], d["wd"], b, nc, B, T, H, W, C, stride, ops.dt_code(dtype))
    d["fwd_kernel"] = ops.last_kernel()
    t2 = torch.full_like(d["ad"], float("nan"))
    ds = torch.zeros(2 * C, dtype=torch.float64, device=DEV)
    dw = torch.zeros((C, 27), dtype=torch.float32, device=DEV)
    ops.dw_bwd_fused(padc(d["t1"], Cp).to(DEV, dtype).contiguous(), b, padc(d["cA"], Cp).to(DEV),
                     padc(d["cB"], Cp).to(DEV).contiguous(), padc(d["cC"], Cp).to(DEV), d["wd"], d["ad"], d["ss"], d["mr"], t2, ds,
                     dw, B, T, H, W, C, ops.dt_code(dtype), stride)
    torch.cuda.synchronize()
    return b, nc, t2, ds, dw


def _check_against_float64(d, out):
    b, nc, t2, ds, dw = out
    B, C, Cp, dtype = d["B"], d["C"], d["Cp"], d["dtype"]
    bre = d["bref"].detach().permute(0, 2, 3, 4, 1)
    bf16 = dtype == torch.bfloat16
    if bf16:   # per element: 2^-8 |ref| + 2^-19 sum|term| (dW: 2^-13 sum|term|), derived in tests/test_hotpath_bf16_gpu.py
        import hotpath_reference as R
        f64 = lambda t: t.detach().double().cpu()   # noqa: E731
        r = R.dw_pair_ratios(f64(d["a"]), f64(d["scale"]), f64(d["ss"][Cp:Cp + C]), f64(d["wd"]).view(C, 27), d["stride"], f64(d["t1"]),
                             f64(b[..., :C]), f64(d["cA"]), f64(d["cB"]), f64(d["cC"]), y_dev=f64(b[..., :C]), t2_dev=f64(t2[..., :C]),
                             dw_dev=f64(dw), round_operand=d["fwd_kernel"].startswith("dw_fwd_kernel<"))   # (that kernel's LDS tile is bf16)
        assert max(r.values()) <= 1.0, (d["fwd_kernel"], r)
    else:
        close(b[..., :C], bre, dtype, "dw fwd", scale=bre.abs().max().item())
    if Cp > C:
        assert (b[..., C:].float() == 0).all() and (t2[..., C:].float() == 0).all()
    bq = b[..., :C].float().cpu().double()
    s = nc.cpu().view(B, Cp, 2)[:, :C]
    assert torch.allclose(s[..., 0], bq.sum((1, 2, 3)), rtol=1e-5, atol=1e-3)
    assert torch.allclose(s[..., 1], (bq * bq).sum((1, 2, 3)), rtol=1e-5, atol=1e-3)
    # backward of db = cA * t1 + cB[n] + cC * b (the device's own b), ReLU mask included, BatchNorm_a scale divided out
    db = d["cA"].double() * d["t1"].double() + d["cB"].double()[:, None, None, None, :] + d["cC"].double() * bq
    d["bref"].backward(db.permute(0, 4, 1, 2, 3))
    t2_ref = d["a_r"].grad / d["scale"].double()
    if not bf16:
        close(t2[..., :C], t2_ref, dtype, "dw bwd data", scale=t2_ref.abs().max().item())
    t2q = t2[..., :C].float().cpu().double()
    sd = ds.cpu()
    ahat = (d["a"] - d["mean_a"]) * d["rstd_a"]
    assert torch.allclose(sd[:C], t2q.sum((0, 1, 2, 3)), rtol=1e-5, atol=1e-3 * max(1.0, B / 8))
    assert torch.allclose(sd[C:], (t2q * ahat.double()).sum((0, 1, 2, 3)), rtol=1e-5, atol=1e-3 * max(1.0, B / 8))
    dw_ref = d["w_r"].grad.view(C, 27)
    if not bf16:
        close(dw, dw_ref, dtype, "dw wgrad", scale=dw_ref.abs().max().item())


def _check_t4_off_against_on(d, on):
    """C3D_OPT_DW_T4 = 0 (five-frame instantiation) against 1: same tap order per output in every kernel of the pair."""
    from change3d_amd import ops
    try:
        ops.set_option(ops.OPT_DW_T4, 0)
        off = _run(d)
    finally:
        ops.set_option(ops.OPT_DW_T4, 1)
    assert torch.equal(_bits(on[0]), _bits(off[0])), "forward output differs"
    assert torch.equal(_bits(on[2]), _bits(off[2])), "data gradient differs"
    assert torch.allclose(on[1], off[1], rtol=1e-6, atol=1e-4), "forward statistics differ"
    assert torch.allclose(on[3], off[3], rtol=1e-6, atol=1e-4), "BatchNorm_a sums differ"
    scale = off[4].abs().max().item()
    assert (on[4] - off[4]).abs().max().item() <= 1e-5 * scale, "weight gradient differs"


# the three stage widths of X3D-L's inner channels (54 / 108 / 216: the last vector of a chunk is short or empty), odd
# extents (ragged tiles, partial stride-2 quads), a single tile row, walks across samples
SHAPES = [
    (2, 16, 24, 54, 1), (2, 16, 24, 54, 2), (2, 16, 24, 108, 1), (2, 16, 24, 108, 2), (2, 16, 24, 216, 1), (2, 16, 24, 216, 2),
    (3, 17, 19, 54, 1), (3, 17, 19, 54, 2), (2, 15, 9, 108, 2), (5, 20, 28, 216, 1), (2, 8, 72, 24, 1),
    (3, 40, 40, 108, 1),    # 25 tiles per sample: both ring slots are reused
    (40, 24, 24, 54, 1),    # walks cross sample boundaries
]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,H,W,C,stride", SHAPES)
def test_dw333_four_frames(dtype, B, H, W, C, stride):
    _need_gpu()
    d = _case(B, H, W, C, stride, dtype, 400)
    on = _run(d)
    _check_against_float64(d, on)
    _check_t4_off_against_on(d, on)


# one case per stage at a BDA training geometry (256 x 256 input: 128 / 64 / 32 / 16 maps; first block of a stage = stride 2)
@pytest.mark.parametrize("H,C,stride", [(128, 54, 2), (64, 54, 1), (64, 108, 2), (32, 108, 1), (32, 216, 2), (16, 216, 1)])
def test_dw333_four_frames_at_the_bda_training_geometry(H, C, stride):
    _need_gpu()
    d = _case(2, H, H, C, stride, torch.bfloat16, 500)
    on = _run(d)
    _check_against_float64(d, on)
    _check_t4_off_against_on(d, on)


@pytest.mark.parametrize("ring", [0, 9, 13])
def test_dw_bwd_four_frame_ring_equals_the_register_prefetch_kernel(ring):
    """The four-frame LDS-DMA ring (two slots, `a` rows in LDS) against the four-frame register-prefetch kernel."""
    _need_gpu()
    from change3d_amd import ops
    d = _case(3, 40, 40, 108, 1, torch.bfloat16, 600)
    try:
        ops.set_option(ops.OPT_DW_RING, 0)
        ref = _run(d)
        k_ref = ops.last_kernel()
        ops.set_option(ops.OPT_DW_RING, ring)
        out = _run(d)
        k_out = ops.last_kernel()
    finally:
        ops.set_option(ops.OPT_DW_RING, 13)
    assert k_ref == "dw_bwd_fused_kernel<unsigned short, 4, 1>", k_ref
    assert k_out == (f"dw_bwd_ring_kernel<4, {'true' if ring & 4 else 'false'}>" if ring & 1 else k_ref), k_out
    assert torch.equal(_bits(ref[2]), _bits(out[2])), "data gradient differs"
    assert torch.allclose(ref[3], out[3], rtol=1e-12, atol=0), "BatchNorm_a sums differ"
    assert (ref[4] - out[4]).abs().max().item() <= 1e-5 * ref[4].abs().max().item(), "weight gradient differs"


def test_option_dw_t4_is_accepted_and_unknown_options_are_refused():
    _need_gpu()
    from change3d_amd import _lib, ops
    assert ops.OPT_DW_T4 == 11
    ops.set_option(ops.OPT_DW_T4, 0)
    ops.set_option(ops.OPT_DW_T4, 1)
    assert _lib.lib().c3d_set_option(12, 1) != 0
