"""GPU parity tests, op level: every kernel family called through the C ABI (ctypes) and
compared with a plain PyTorch-CPU fp32 computation of the same operation.
f32 storage: tight tolerances (parity path).  bf16 storage: tolerances sized for bf16 rounding.
"""
import numpy as np
import os

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


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
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    err = (a - b).abs()
    lim = at * scale + rt * b.abs()
    bad = (err > lim).sum().item()
    assert bad == 0, f"{what}: {bad}/{err.numel()} out of tolerance, max err {err.max().item():.3e}, ref max {b.abs().max().item():.3e}"


def padc(t, cp):
    """[..., C] -> [..., Cp] zero padded."""
    c = t.shape[-1]
    return t if c == cp else F.pad(t, (0, cp - c))


DTYPES = [torch.float32, torch.bfloat16]


def q(t, dtype):
    """quantise reference input the way the device tensor stores it."""
    return t.to(dtype).float()


# --------------------------------------------------------------------------- pointwise GEMM
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("K,N", [(24, 54), (54, 24), (48, 108), (108, 48), (96, 216), (216, 96), (24, 24)])
def test_pw_gemm_plain_stats(dtype, K, N):
    _need_gpu()
    from change3d_amd import ops
    M = 16 * 37 + 5
    Kp, Np = ops.cpad(K), ops.cpad(N)
    x = q(rnd((M, K), 1), dtype)
    w = rnd((N, K), 2, 0.2)
    ref = x @ w.t()
    xd = padc(x, Kp).to(DEV, dtype).contiguous()
    y = torch.full((M, Np), float("nan"), dtype=dtype, device=DEV)
    stats = torch.zeros(ops.STAT_STRIPES * 2 * N, dtype=torch.float64, device=DEV)
    ops.pw_gemm(xd, w.to(DEV), y, M=M, K=K, N=N, w_sn=K, w_sk=1, dtype=ops.dt_code(dtype),
                epi_mode=ops.EPI_STATS, stats=stats)
    torch.cuda.synchronize()
    close(y[:, :N], ref, dtype, "y", scale=ref.abs().max().item())
    if Np > N:
        assert (y[:, N:].float() == 0).all(), "pad channels must be zero"
    yq = y[:, :N].float().cpu().double()
    s = stats.cpu().view(ops.STAT_STRIPES, 2 * N).sum(0)
    assert torch.allclose(s[:N], yq.sum(0), rtol=1e-5, atol=1e-3), "column sums"
    assert torch.allclose(s[N:], (yq * yq).sum(0), rtol=1e-5, atol=1e-3), "column sums of squares"


@pytest.mark.parametrize("dtype", DTYPES)
def test_pw_gemm_bn_se_swish_prologue(dtype):
    _need_gpu()
    from change3d_amd import ops
    B, rows, K, N = 3, 48, 54, 24
    M = B * rows
    Kp = ops.cpad(K)
    x = q(rnd((M, K), 3), dtype)
    w = rnd((N, K), 4, 0.2)
    scale, shift = rnd((K,), 5).abs() + 0.5, rnd((K,), 6, 0.3)
    gate = torch.sigmoid(rnd((B, K), 7))
    v = (x * scale + shift).view(B, rows, K) * gate[:, None, :]
    ref = (v * torch.sigmoid(v)).view(M, K) @ w.t()
    ss = torch.cat([padc(scale, Kp), padc(shift, Kp)]).to(DEV)
    y = torch.empty((M, ops.cpad(N)), dtype=dtype, device=DEV)
    ops.pw_gemm(padc(x, Kp).to(DEV, dtype).contiguous(), w.to(DEV), y, M=M, K=K, N=N, w_sn=K, w_sk=1,
                dtype=ops.dt_code(dtype), pro_mode=ops.PRO_BN_SE_SWISH, pro_p=ss,
                pro_gate=padc(gate, Kp).to(DEV).contiguous(), rows_per_sample=rows)
    close(y[:, :N], ref, dtype, "y", scale=ref.abs().max().item())


@pytest.mark.parametrize("dtype", DTYPES)
def test_pw_gemm_affine2_transposed_add(dtype):
    _need_gpu()
    from change3d_amd import ops
    M, K, N = 16 * 9, 54, 24      # data-gradient shape of conv_a: g[M,54] @ W[54,24]
    Kp = ops.cpad(K)
    g, a = q(rnd((M, K), 8), dtype), q(rnd((M, K), 9), dtype)
    A, Bc, Cc = rnd((K,), 10), rnd((K,), 11, 0.1), rnd((K,), 12, 0.1)
    wt = rnd((K, N), 13, 0.2)     # stored as conv weight [out=K][in=N]
    res = q(rnd((M, N), 14), dtype)
    ref = (A * g + Bc + Cc * a) @ wt + res
    coef = torch.cat([padc(A, Kp), padc(Bc, Kp), padc(Cc, Kp)]).to(DEV)
    y = torch.empty((M, ops.cpad(N)), dtype=dtype, device=DEV)
    ops.pw_gemm(padc(g, Kp).to(DEV, dtype).contiguous(), wt.to(DEV), y, M=M, K=K, N=N, w_sn=1, w_sk=N,
                dtype=ops.dt_code(dtype), x2=padc(a, Kp).to(DEV, dtype).contiguous(), pro_mode=ops.PRO_AFFINE2,
                pro_p=coef, epi_mode=ops.EPI_ADD, e1=res.to(DEV, dtype).contiguous(), res_mode=0)
    close(y[:, :N], ref, dtype, "y", scale=ref.abs().max().item())


@pytest.mark.parametrize("dtype", DTYPES)
def test_pw_gemm_stride2_gather_and_scatter_add(dtype):
    _need_gpu()
    from change3d_amd import ops
    BT, H, W, K, N = 4, 8, 12, 24, 48
    x = q(rnd((BT, H, W, K), 15), dtype)
    w = rnd((N, K), 16, 0.2)
    ref = x[:, ::2, ::2].reshape(-1, K) @ w.t()
    Mo = BT * (H // 2) * (W // 2)
    y = torch.empty((Mo, N), dtype=dtype, device=DEV)
    ops.pw_gemm(x.to(DEV, dtype).contiguous(), w.to(DEV), y, M=Mo, K=K, N=N, w_sn=K, w_sk=1,
                dtype=ops.dt_code(dtype), row_mode=ops.ROWS_STRIDE2, H=H, W=W)
    close(y, ref, dtype, "gather", scale=ref.abs().max().item())
    # scatter-add: out[M_full, K2] = z @ w2^T + (res at even pixels)
    K2, N2 = 48, 24
    z = q(rnd((BT * H * W, K2), 17), dtype)
    w2 = rnd((N2, K2), 18, 0.2)
    res = q(rnd((BT, H // 2, W // 2, N2), 19), dtype)
    full = torch.zeros(BT, H, W, N2)
    full[:, ::2, ::2] = res
    ref2 = z @ w2.t() + full.view(-1, N2)
    y2 = torch.empty((BT * H * W, N2), dtype=dtype, device=DEV)
    ops.pw_gemm(z.to(DEV, dtype).contiguous(), w2.to(DEV), y2, M=BT * H * W, K=K2, N=N2, w_sn=K2, w_sk=1,
                dtype=ops.dt_code(dtype), epi_mode=ops.EPI_ADD, e1=res.to(DEV, dtype).contiguous(), res_mode=1,
                H=H, W=W)
    close(y2, ref2, dtype, "scatter-add", scale=ref2.abs().max().item())


@pytest.mark.parametrize("dtype", DTYPES)
def test_pw_gemm_swish_se_bwd_epilogue(dtype):
    _need_gpu()
    from change3d_amd import ops
    B, rows, K, N = 2, 32, 24, 54
    M = B * rows
    Np = ops.cpad(N)
    g = q(rnd((M, K), 20), dtype)
    w = rnd((K, N), 21, 0.2)  # conv_c weight [out=K=24][in=N=54]; data-grad = g @ w
    b = q(rnd((M, N), 22), dtype)
    scale, shift = rnd((N,), 23).abs() + 0.5, rnd((N,), 24, 0.3)
    gate = torch.sigmoid(rnd((B, N), 25))
    dsb = g @ w
    pb = b * scale + shift
    gg = gate.repeat_interleave(rows, 0)
    qv = gg * pb
    sg = torch.sigmoid(qv)
    dq = dsb * sg * (1 + qv * (1 - sg))
    t1 = dq * gg
    y = torch.empty((M, Np), dtype=dtype, device=DEV)
    nc3 = torch.zeros(B * Np * 3, dtype=torch.float64, device=DEV)
    ss = torch.cat([padc(scale, Np), padc(shift, Np)]).to(DEV)
    mean, rstd = rnd((N,), 26, 0.5), rnd((N,), 27).abs() + 0.5
    ident = torch.cat([torch.ones(K), torch.zeros(K), torch.zeros(K)]).to(DEV)  # AFFINE2 with A=1,B=0,C=0
    gd = g.to(DEV, dtype).contiguous()
    ops.pw_gemm(gd, w.to(DEV), y, M=M, K=K, N=N, w_sn=1, w_sk=N, dtype=ops.dt_code(dtype), x2=gd,
                pro_mode=ops.PRO_AFFINE2, pro_p=ident, epi_mode=ops.EPI_SWISH_SE_BWD, e1=padc(b, Np).to(DEV, dtype).contiguous(), epi_p=ss,
                epi_gate=padc(gate, Np).to(DEV).contiguous(),
                epi_q=torch.cat([padc(mean, Np), padc(rstd, Np)]).to(DEV), stats=nc3, rows_per_sample=rows)
    close(y[:, :N], t1, dtype, "t1", scale=t1.abs().max().item())
    s = nc3.cpu().view(B, Np, 3)[:, :N]
    t1q = y[:, :N].float().cpu()
    ref0 = (dq * pb).view(B, rows, N).sum(1).double()
    ref1 = t1q.view(B, rows, N).sum(1).double()
    ref2 = (t1q * ((b - mean) * rstd)).view(B, rows, N).sum(1).double()
    rt = 1e-4 if dtype == torch.float32 else 3e-2
    assert torch.allclose(s[..., 0], ref0, rtol=rt, atol=rt * ref0.abs().max().item()), "sum dq*pb"
    assert torch.allclose(s[..., 1], ref1, rtol=1e-4, atol=1e-3), "sum t1"
    assert torch.allclose(s[..., 2], ref2, rtol=1e-4, atol=1e-3), "sum t1*bhat"


# Long walks: many tiles per wave, several iterations of 1-8 sub-tiles, a partial last iteration and a ragged last
# tile.  The small cases above give every wave at most one tile, so the prefetch ring, the paired sub-tiles, the
# hand-scheduled fragment batches across K steps and the companion-row prefetch chain are only exercised here.
# (120, 80) and (48, 152): output widths whose epilogue takes FEWER passes than the unrolled maximum of their tile bucket
# (10 / 19 channel vectors: 3 of 4 and 6 of 8 passes) with several tiles per iteration -- the pass past the last one used to
# overwrite the next tile's prefetched companion rows (round 5)
@pytest.mark.parametrize("K,N", [(24, 54), (54, 24), (48, 108), (108, 48), (96, 216), (216, 96), (120, 80), (48, 152)])
@pytest.mark.parametrize("mode", ["stats", "swish_stats", "affine2_add", "affine2_swish_se_bwd"])
def test_pw_gemm_long_walks(K, N, mode):
    _need_gpu()
    from change3d_amd import ops
    dtype = torch.bfloat16
    from change3d_amd import _lib
    cus = _lib.lib().c3d_device_cus()
    B = 5
    rows = 16 * ((7 * 8 * cus) // B + 3)               # ~7 tiles per wave at 8 waves per CU, odd tile count per sample
    M = B * rows - 11                                   # ragged last tile (not for the per-sample epilogue)
    if mode in ("swish_stats", "affine2_swish_se_bwd"):
        M = B * rows
    Kp, Np = ops.cpad(K), ops.cpad(N)
    x = q(rnd((M, K), 31), dtype)
    y = torch.full((M, Np), float("nan"), dtype=dtype, device=DEV)
    dt = ops.dt_code(dtype)
    xd = padc(x, Kp).to(DEV, dtype).contiguous()
    if mode == "stats":
        w = rnd((N, K), 32, 0.2)
        ref = x @ w.t()
        stats = torch.zeros(ops.STAT_STRIPES * 2 * N, dtype=torch.float64, device=DEV)
        ops.pw_gemm(xd, w.to(DEV), y, M=M, K=K, N=N, w_sn=K, w_sk=1, dtype=dt, epi_mode=ops.EPI_STATS, stats=stats)
    elif mode == "swish_stats":
        w = rnd((N, K), 33, 0.2)
        scale, shift = rnd((K,), 34).abs() + 0.5, rnd((K,), 35, 0.3)
        gate = torch.sigmoid(rnd((B, K), 36))
        v = (x * scale + shift).view(B, rows, K) * gate[:, None, :]
        ref = (v * torch.sigmoid(v)).view(M, K) @ w.t()
        stats = torch.zeros(ops.STAT_STRIPES * 2 * N, dtype=torch.float64, device=DEV)
        ops.pw_gemm(xd, w.to(DEV), y, M=M, K=K, N=N, w_sn=K, w_sk=1, dtype=dt, pro_mode=ops.PRO_BN_SE_SWISH,
                    pro_p=torch.cat([padc(scale, Kp), padc(shift, Kp)]).to(DEV),
                    pro_gate=padc(gate, Kp).to(DEV).contiguous(), rows_per_sample=rows, epi_mode=ops.EPI_STATS, stats=stats)
    else:
        a2 = q(rnd((M, K), 37), dtype)
        A, Bc, Cc = rnd((K,), 38), rnd((K,), 39, 0.1), rnd((K,), 40, 0.1)
        wt = rnd((K, N), 41, 0.2)                       # conv weight [out=K][in=N]: transposed use
        pre = (A * x + Bc + Cc * a2) @ wt
        coef = torch.cat([padc(A, Kp), padc(Bc, Kp), padc(Cc, Kp)]).to(DEV)
        a2d = padc(a2, Kp).to(DEV, dtype).contiguous()
        if mode == "affine2_add":
            res = q(rnd((M, N), 42), dtype)
            ref = pre + res
            ops.pw_gemm(xd, wt.to(DEV), y, M=M, K=K, N=N, w_sn=1, w_sk=N, dtype=dt, x2=a2d, pro_mode=ops.PRO_AFFINE2,
                        pro_p=coef, epi_mode=ops.EPI_ADD, e1=padc(res, Np).to(DEV, dtype).contiguous(), res_mode=0)
        else:
            b = q(rnd((M, N), 43), dtype)
            scale, shift = rnd((N,), 44).abs() + 0.5, rnd((N,), 45, 0.3)
            gate = torch.sigmoid(rnd((B, N), 46))
            mean, rstd = rnd((N,), 47, 0.5), rnd((N,), 48).abs() + 0.5
            pb = b * scale + shift
            gg = gate.repeat_interleave(rows, 0)
            qv = gg * pb
            sg = torch.sigmoid(qv)
            dq = pre * sg * (1 + qv * (1 - sg))
            ref = dq * gg
            nc3 = torch.zeros(B * Np * 3, dtype=torch.float64, device=DEV)
            ops.pw_gemm(xd, wt.to(DEV), y, M=M, K=K, N=N, w_sn=1, w_sk=N, dtype=dt, x2=a2d, pro_mode=ops.PRO_AFFINE2,
                        pro_p=coef, epi_mode=ops.EPI_SWISH_SE_BWD, e1=padc(b, Np).to(DEV, dtype).contiguous(),
                        epi_p=torch.cat([padc(scale, Np), padc(shift, Np)]).to(DEV),
                        epi_gate=padc(gate, Np).to(DEV).contiguous(),
                        epi_q=torch.cat([padc(mean, Np), padc(rstd, Np)]).to(DEV), stats=nc3, rows_per_sample=rows)
    torch.cuda.synchronize()
    assert torch.isfinite(y.float()).all(), "every row must be written"
    close(y[:, :N], ref, dtype, "y", scale=ref.abs().max().item())
    yq = y[:, :N].float().cpu().double()
    if mode in ("stats", "swish_stats"):
        s = stats.cpu().view(ops.STAT_STRIPES, 2 * N).sum(0)
        assert torch.allclose(s[:N], yq.sum(0), rtol=1e-5, atol=1e-2), "column sums"
        assert torch.allclose(s[N:], (yq * yq).sum(0), rtol=1e-5, atol=1e-2), "column sums of squares"
    if mode == "affine2_swish_se_bwd":
        s = nc3.cpu().view(B, Np, 3)[:, :N]
        ref1 = yq.view(B, rows, N).sum(1)
        ref2 = (yq * ((b - mean) * rstd).double()).view(B, rows, N).sum(1)
        ref0 = (dq * pb).view(B, rows, N).sum(1).double()
        assert torch.allclose(s[..., 1], ref1, rtol=1e-4, atol=1e-2), "sum t1"
        assert torch.allclose(s[..., 2], ref2, rtol=1e-4, atol=1e-2), "sum t1*bhat"
        assert torch.allclose(s[..., 0], ref0, rtol=3e-2, atol=3e-2 * ref0.abs().max().item()), "sum dq*pb"


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("K,N", [(24, 54), (216, 96), (96, 216), (48, 48)])
def test_pw_wgrad(dtype, K, N):
    _need_gpu()
    from change3d_amd import ops
    B, rows = 2, 200
    M = B * rows
    Kp, Np = ops.cpad(K), ops.cpad(N)
    p, p2 = q(rnd((M, N), 30), dtype), q(rnd((M, N), 31), dtype)
    A, Bc, Cc = rnd((N,), 32), rnd((N,), 33, 0.1), rnd((N,), 34, 0.1)
    x = q(rnd((M, K), 35), dtype)
    scale, shift = rnd((K,), 36).abs() + 0.5, rnd((K,), 37, 0.3)
    gate = torch.sigmoid(rnd((B, K), 38))
    P = A * p + Bc + Cc * p2
    v = (x * scale + shift) * gate.repeat_interleave(rows, 0)
    Q = v * torch.sigmoid(v)
    ref = P.t() @ Q + 1.0
    dw = torch.ones((N, K), dtype=torch.float32, device=DEV)  # accumulate semantics (+=)
    ops.pw_wgrad(padc(p, Np).to(DEV, dtype).contiguous(), padc(x, Kp).to(DEV, dtype).contiguous(), dw, M=M, K=K, N=N,
                 dw_sn=K, dw_sk=1, dtype=ops.dt_code(dtype), p2=padc(p2, Np).to(DEV, dtype).contiguous(),
                 p_coef=torch.cat([padc(A, Np), padc(Bc, Np), padc(Cc, Np)]).to(DEV), q_mode=ops.PRO_BN_SE_SWISH,
                 q_ss=torch.cat([padc(scale, Kp), padc(shift, Kp)]).to(DEV),
                 q_gate=padc(gate, Kp).to(DEV).contiguous(), rows_per_sample=rows)
    close(dw, ref, dtype, "dW", scale=ref.abs().max().item())


# Many tiles per workgroup with the per-sample Swish gate cached across tiles: samples that end inside a tile, inside
# a thread's 4-row group (rows_per_sample % 4 != 0) and a ragged last tile.
@pytest.mark.parametrize("K,N,rows", [(216, 96, 148), (216, 96, 150), (108, 48, 301), (54, 24, 1027)])
def test_pw_wgrad_long_walks(K, N, rows):
    _need_gpu()
    from change3d_amd import ops
    dtype = torch.bfloat16
    B = 400000 // rows
    M = B * rows - 5
    Kp, Np = ops.cpad(K), ops.cpad(N)
    # all-positive operands (the sum is coherent, ~M terms of one sign) and gates that alternate between 0.1 and 0.9
    # from sample to sample: a row converted with a neighbouring sample's gate shifts the result by percent
    p, p2 = q(rnd((M, N), 50).abs(), dtype), q(rnd((M, N), 51).abs(), dtype)
    A, Bc, Cc = rnd((N,), 52).abs() + 0.5, torch.zeros(N), rnd((N,), 54, 0.1).abs()
    x = q(rnd((M, K), 55).abs(), dtype)
    scale, shift = rnd((K,), 56).abs() + 0.5, rnd((K,), 57, 0.3).abs()
    gate = torch.where(torch.arange(B)[:, None] % 2 == 0, torch.full((B, K), 0.1), torch.full((B, K), 0.9))
    P = (A * p + Bc + Cc * p2).double()
    v = (x * scale + shift) * gate.repeat_interleave(rows, 0)[:M]
    Q = (v * torch.sigmoid(v)).double()
    ref = (P.t() @ Q).float()
    dw = torch.zeros((N, K), dtype=torch.float32, device=DEV)
    ops.pw_wgrad(padc(p, Np).to(DEV, dtype).contiguous(), padc(x, Kp).to(DEV, dtype).contiguous(), dw, M=M, K=K, N=N,
                 dw_sn=K, dw_sk=1, dtype=ops.dt_code(dtype), p2=padc(p2, Np).to(DEV, dtype).contiguous(),
                 p_coef=torch.cat([padc(A, Np), padc(Bc, Np), padc(Cc, Np)]).to(DEV), q_mode=ops.PRO_BN_SE_SWISH,
                 q_ss=torch.cat([padc(scale, Kp), padc(shift, Kp)]).to(DEV),
                 q_gate=padc(gate, Kp).to(DEV).contiguous(), rows_per_sample=rows)
    rel = ((dw.cpu() - ref).abs() / ref.abs()).max().item()
    assert rel < 4e-3, rel      # bf16 operand rounding is 2^-9 per term and averages out over ~4e5 coherent terms


# conv_c forward of the training path: the workgroup-cooperative kernel (csrc/pw_cfwd.hip, C3D_OPT_PW_CFWD) against the
# wave-private-tile kernel on the same device buffers.  Same converted operand, same weight fragments, same k order of the MFMA
# chain: the output must be BIT-identical; BatchNorm_b scale / shift, the SE gate and the running statistics come from the same
# device functions (identical); the BatchNorm_c statistics group their f32 partial sums differently (1e-6).  Shapes: the three
# stages' layers (two / three / six output tiles), samples that end inside a tile, a ragged last tile, with and without SE.
@pytest.mark.parametrize("se", [False, True])
@pytest.mark.parametrize("K,N,B,rps", [(216, 96, 8, 768), (108, 48, 4, 3072), (54, 24, 4, 3072), (216, 96, 5, 1008), (108, 48, 3, 784)])
def test_conv_c_forward_kernels_agree_bit_for_bit(K, N, B, rps, se):
    _need_gpu()
    import ctypes as C
    from change3d_amd import ops, _lib as L
    Kp, Np = ops.cpad(K), ops.cpad(N)
    M = B * rps
    if rps % 16:
        pytest.skip("rows_per_sample must be a multiple of 16 for the narrow kernels")
    x = padc(rnd((M, K), 90), Kp).to(DEV).to(torch.bfloat16)
    w = rnd((N, K), 91, 0.1).to(DEV)
    xs = x.float().view(B, rps, Kp).double()
    nc = torch.stack([xs.sum(1), (xs * xs).sum(1)], dim=2).contiguous()       # [B][Kp][2] per-sample sums, as c3d_dw333_fwd leaves them
    gamma, beta = (rnd((K,), 92).abs() + 0.5).to(DEV), rnd((K,), 93, 0.2).to(DEV)
    Cr = 16
    w1, b1, w2, b2 = rnd((Cr, K), 94, 0.1).to(DEV), rnd((Cr,), 95, 0.1).to(DEV), rnd((K, Cr), 96, 0.1).to(DEV), rnd((K,), 97, 0.1).to(DEV)
    img = torch.empty(ops.pw_weight_image_bytes(N, K, ops.DT_BF16), dtype=torch.uint8, device=DEV)
    ops.pw_pack_weights([(w, img, N, K, K, 1)], ops.DT_BF16)
    ptr = lambda t: t.data_ptr()
    res = {}
    try:
        for opt in (0, 1):
            ops.set_option(ops.OPT_PW_CFWD, opt)
            y = torch.full((M, Np), 7.0, device=DEV).to(torch.bfloat16)
            stats = torch.zeros(ops.STAT_STRIPES * 2 * N, dtype=torch.float64, device=DEV)
            rm, rv = torch.zeros(K, device=DEV), torch.ones(K, device=DEV)
            nbt = torch.zeros(1, dtype=torch.int64, device=DEV)
            ss, mr = torch.zeros(2 * Kp, device=DEV), torch.zeros(2 * Kp, device=DEV)
            gate, hid = torch.zeros(B, Kp, device=DEV), torch.zeros(B, Cr, device=DEV)
            a = L.PwArgs()
            a.x, a.y, a.w, a.w_img = ptr(x), ptr(y), ptr(w), ptr(img)
            a.M, a.K, a.Kp, a.N, a.Np, a.w_sn, a.w_sk = M, K, Kp, N, Np, K, 1
            a.rows_per_sample, a.dtype = rps, ops.DT_BF16
            a.pro_mode, a.epi_mode = ops.PRO_BN_SE_SWISH, ops.EPI_STATS
            a.pro_p, a.stats = ptr(ss), ptr(stats)
            f = L.BnFin()
            f.gamma, f.beta, f.running_mean, f.running_var, f.nbt, f.ss, f.mr = ptr(gamma), ptr(beta), ptr(rm), ptr(rv), ptr(nbt), ptr(ss), ptr(mr)
            f.count, f.momentum, f.eps, f.training, f.batch, f.sums = float(M), 0.1, 1e-5, 1, B, ptr(nc)
            a.fin = f
            if se:
                a.pro_gate = ptr(gate)
                a.se_w1, a.se_b1, a.se_w2, a.se_b2, a.se_hid, a.se_cr = ptr(w1), ptr(b1), ptr(w2), ptr(b2), ptr(hid), Cr
            rc = L.lib().c3d_pw_gemm(C.byref(a), ops._stream())
            kernel = ops.last_kernel()
            torch.cuda.synchronize()
            assert rc == 0, rc
            res[opt] = dict(y=y.cpu(), stats=stats.cpu().view(ops.STAT_STRIPES, 2, N).sum(0), ss=ss.cpu(), mr=mr.cpu(), gate=gate.cpu(),
                            hid=hid.cpu(), rm=rm.cpu(), rv=rv.cpu(), nbt=int(nbt), kernel=kernel)
    finally:
        ops.set_option(ops.OPT_PW_CFWD, 3)
    r0, r1 = res[0], res[1]
    # the two legs ran two kernels (the dispatcher falls back silently where the cooperative kernel does not apply)
    assert r0["kernel"].startswith("pw_gemm_kernel<") and r1["kernel"].startswith("pw_cfwd_kernel<1, "), (r0["kernel"], r1["kernel"])
    assert torch.isfinite(r1["y"].float()).all() and r1["y"].float().abs().max().item() > 0
    assert torch.equal(r0["y"], r1["y"]), f"{int((r0['y'] != r1['y']).sum())} output elements differ"
    for k in ("ss", "mr", "gate", "hid", "rm", "rv"):
        assert torch.equal(r0[k], r1[k]), k
    assert r0["nbt"] == r1["nbt"] == 1
    yq = r1["y"].float().double()[:, :N]
    assert torch.allclose(r1["stats"][0], yq.sum(0), rtol=1e-5, atol=1e-2) and torch.allclose(r1["stats"][1], (yq * yq).sum(0), rtol=1e-5, atol=1e-2)
    assert torch.allclose(r0["stats"], r1["stats"], rtol=2e-6, atol=1e-3)


# conv_a forward with the previous block's residual add in its prologue (c3d_pw_args.pro_out) on the cooperative kernel
# (C3D_OPT_PW_CFWD bit 1) against the wave-private-tile kernel: y = relu(bn_c(c) + shortcut) written out, the GEMM's output, the
# BatchNorm_c scale / shift / running statistics of the previous block -- all BIT-identical; BatchNorm_a's statistics to 1e-6.
@pytest.mark.parametrize("K,N,M", [(96, 216, 8 * 768), (48, 108, 4 * 3072), (24, 54, 4 * 3072), (96, 216, 5000), (48, 108, 2345), (24, 54, 1031)])
def test_conv_a_forward_kernels_agree_bit_for_bit(K, N, M):
    _need_gpu()
    import ctypes as C
    from change3d_amd import ops, _lib as L
    Kp, Np = ops.cpad(K), ops.cpad(N)
    c = padc(rnd((M, K), 80), Kp).to(DEV).to(torch.bfloat16)
    sc = padc(rnd((M, K), 81), Kp).to(DEV).to(torch.bfloat16)
    w = rnd((N, K), 82, 0.1).to(DEV)
    cd = c.float().double()[:, :K]
    tot = torch.stack([cd.sum(0), (cd * cd).sum(0)])                           # [2][K]
    frac = torch.rand(ops.STAT_STRIPES, 1, 1, dtype=torch.float64, device=DEV)
    sums = (tot[None] * frac / frac.sum()).contiguous()                        # [stripes][2][K], as the producer's epilogue leaves them
    gamma, beta = (rnd((K,), 83).abs() + 0.5).to(DEV), rnd((K,), 84, 0.2).to(DEV)
    img = torch.empty(ops.pw_weight_image_bytes(N, K, ops.DT_BF16), dtype=torch.uint8, device=DEV)
    ops.pw_pack_weights([(w, img, N, K, K, 1)], ops.DT_BF16)
    ptr = lambda t: t.data_ptr()
    res = {}
    try:
        for opt in (1, 3):
            ops.set_option(ops.OPT_PW_CFWD, opt)
            y = torch.full((M, Np), 7.0, device=DEV).to(torch.bfloat16)
            po = torch.full((M, Kp), 5.0, device=DEV).to(torch.bfloat16)
            stats = torch.zeros(ops.STAT_STRIPES * 2 * N, dtype=torch.float64, device=DEV)
            rm, rv = torch.zeros(K, device=DEV), torch.ones(K, device=DEV)
            nbt = torch.zeros(1, dtype=torch.int64, device=DEV)
            ss, mr = torch.zeros(2 * Kp, device=DEV), torch.zeros(2 * Kp, device=DEV)
            a = L.PwArgs()
            a.x, a.x2, a.y, a.w, a.w_img, a.pro_out = ptr(c), ptr(sc), ptr(y), ptr(w), ptr(img), ptr(po)
            a.M, a.K, a.Kp, a.N, a.Np, a.w_sn, a.w_sk = M, K, Kp, N, Np, K, 1
            a.dtype = ops.DT_BF16
            a.pro_mode, a.epi_mode = ops.PRO_AFFINE2, ops.EPI_STATS
            a.pro_p, a.stats = ptr(ss), ptr(stats)
            f = L.BnFin()
            f.gamma, f.beta, f.running_mean, f.running_var, f.nbt, f.ss, f.mr = ptr(gamma), ptr(beta), ptr(rm), ptr(rv), ptr(nbt), ptr(ss), ptr(mr)
            f.count, f.momentum, f.eps, f.training, f.batch, f.sums = float(M), 0.1, 1e-5, 1, 0, ptr(sums)
            a.fin = f
            rc = L.lib().c3d_pw_gemm(C.byref(a), ops._stream())
            kernel = ops.last_kernel()
            torch.cuda.synchronize()
            assert rc == 0, rc
            res[opt] = dict(y=y.cpu(), po=po.cpu(), stats=stats.cpu().view(ops.STAT_STRIPES, 2, N).sum(0), ss=ss.cpu(), mr=mr.cpu(),
                            rm=rm.cpu(), rv=rv.cpu(), nbt=int(nbt), kernel=kernel)
    finally:
        ops.set_option(ops.OPT_PW_CFWD, 3)
    r0, r1 = res[1], res[3]
    assert r0["kernel"].startswith("pw_gemm_kernel<") and r1["kernel"].startswith("pw_cfwd_kernel<2, "), (r0["kernel"], r1["kernel"])
    assert torch.isfinite(r1["y"].float()).all() and r1["y"].float().abs().max().item() > 0
    assert torch.equal(r0["po"], r1["po"]), f"{int((r0['po'] != r1['po']).sum())} residual-output elements differ"
    assert torch.equal(r0["y"], r1["y"]), f"{int((r0['y'] != r1['y']).sum())} output elements differ"
    for k in ("ss", "mr", "rm", "rv"):
        assert torch.equal(r0[k], r1[k]), k
    assert r0["nbt"] == r1["nbt"] == 1
    # and the residual output is what it should be: relu(scale * c + shift + shortcut), bf16-rounded
    ref = torch.relu(c.float().cpu()[:, :K] * r1["ss"][:K] + r1["ss"][Kp:Kp + K] + sc.float().cpu()[:, :K])
    assert (r1["po"].float()[:, :K] - ref).abs().max().item() <= 2 ** -8 * ref.abs().max().item() + 1e-6
    yq = r1["y"].float().double()[:, :N]
    assert torch.allclose(r1["stats"][0], yq.sum(0), rtol=1e-5, atol=1e-2) and torch.allclose(r1["stats"][1], (yq * yq).sum(0), rtol=1e-5, atol=1e-2)
    assert torch.allclose(r0["stats"], r1["stats"], rtol=2e-6, atol=1e-3)


# The flat-staged, transposing-read kernel (csrc/pw_wgrad_v2.hip, C3D_OPT_PW_WGRAD_V2) against the first kernel on the same
# device buffers: same operand arithmetic, another summation order inside a k-step -> agreement to f32 rounding of the sums
# (1e-5 of the largest entry), far inside what either is allowed against the f64 product.  Cases: the res4 layers at their
# real rows_per_sample (a tile never straddles samples there), samples that end inside a tile, a ragged last tile, a block
# without SqueezeExcitation (no gate), the plain-operand form (enhance / decoder 1x1), the narrow res2 / res3 widths, and
# M small enough that most workgroups get no tile.
@pytest.mark.parametrize("K,N,rows,B,mode", [
    (216, 96, 3072, 4, "swish_gate"), (96, 216, 3072, 4, "affine2"), (216, 96, 200, 37, "swish_gate"),
    (216, 96, 3072, 3, "swish_nogate"), (24, 24, 4096, 9, "plain"), (54, 24, 1027, 30, "swish_gate"),
    (48, 108, 777, 21, "affine2"), (108, 48, 64, 50, "swish_gate"), (216, 96, 70, 3, "swish_gate"), (48, 216, 500, 11, "affine2")])
def test_pw_wgrad_v2_matches_the_first_kernel(K, N, rows, B, mode):
    _need_gpu()
    from change3d_amd import ops
    dtype = torch.bfloat16
    M = B * rows - (3 if B > 3 else 0)
    Kp, Np = ops.cpad(K), ops.cpad(N)
    p, p2 = q(rnd((M, N), 60), dtype), q(rnd((M, N), 61), dtype)
    A, Bc, Cc = rnd((N,), 62), rnd((N,), 63, 0.1), rnd((N,), 64, 0.1)
    x = q(rnd((M, K), 65), dtype)
    scale, shift = rnd((K,), 66).abs() + 0.5, rnd((K,), 67, 0.3)
    gate = torch.sigmoid(rnd((B, K), 68))
    kw = dict(M=M, K=K, N=N, dw_sn=K, dw_sk=1, dtype=ops.dt_code(dtype))
    P = p.double()
    if mode != "plain":
        kw.update(p2=padc(p2, Np).to(DEV, dtype).contiguous(), p_coef=torch.cat([padc(A, Np), padc(Bc, Np), padc(Cc, Np)]).to(DEV))
        P = (A * p + Bc + Cc * p2).double()
    Q = x.double()
    if mode.startswith("swish"):
        kw.update(q_mode=ops.PRO_BN_SE_SWISH, q_ss=torch.cat([padc(scale, Kp), padc(shift, Kp)]).to(DEV), rows_per_sample=rows)
        v = x * scale + shift
        if mode == "swish_gate":
            kw.update(q_gate=padc(gate, Kp).to(DEV).contiguous())
            v = v * gate.repeat_interleave(rows, 0)[:M]
        Q = (v * torch.sigmoid(v)).double()
    ref = (P.t() @ Q).float()
    pd, xd = padc(p, Np).to(DEV, dtype).contiguous(), padc(x, Kp).to(DEV, dtype).contiguous()
    out, names = {}, {}
    try:
        for v2 in (0, 1):
            ops.set_option(ops.OPT_PW_WGRAD_V2, v2)
            dw = torch.full((N, K), 0.5, dtype=torch.float32, device=DEV)   # accumulate semantics (+=)
            ops.pw_wgrad(pd, xd, dw, **kw)
            names[v2] = ops.last_kernel()
            torch.cuda.synchronize()
            out[v2] = dw.cpu() - 0.5
    finally:
        ops.set_option(ops.OPT_PW_WGRAD_V2, 1)
    # 48 -> 216 (no layer of the network): 14 output tiles beside the two-tensor P prefetch exceed the flat-staged kernel's item
    # budget at every tile height, the dispatcher answers with the first kernel -- the case covers that fall-back, no second kernel
    v2_name = "pw_wgrad_kernel<" if (K, N) == (48, 216) else "pw_wgrad_v2_kernel<"
    assert names[0].startswith("pw_wgrad_kernel<") and names[1].startswith(v2_name), names
    sc = ref.abs().max().item()
    d12 = (out[1] - out[0]).abs().max().item()
    e0, e1 = (out[0] - ref).abs().max().item(), (out[1] - ref).abs().max().item()
    assert d12 <= 2e-5 * sc + 1e-4, f"v2 vs first kernel {d12:.3e} (scale {sc:.3e}; vs f64: first {e0:.3e}, v2 {e1:.3e})"
    assert e1 <= 2.0 * e0 + 2e-5 * sc + 1e-4, f"v2 vs f64 product {e1:.3e}, first kernel {e0:.3e}"


# Chained launches (c3d_pw_wgrad_args.chain): the partials of launch k are added into dw_k by launch k + 1's prologue (the last
# ones by c3d_pw_wgrad_flush) in the reducer kernel's order -- every dw must equal, BIT FOR BIT, what the same launches give
# with a reducer launch each.  Sequence as the stage driver issues it: conv_c / conv_a of the res4 shapes alternating, a
# strided shortcut gradient in between (first kernel: pending partials are flushed in front of it), two workspaces in turn.
def test_pw_wgrad_chained_reduction_is_bit_identical():
    _need_gpu()
    from change3d_amd import ops
    dtype = torch.bfloat16
    B, rows = 6, 1024
    M = B * rows
    Ci, Co = 216, 96
    Cip, Cop = ops.cpad(Ci), ops.cpad(Co)
    dev = lambda t: t.to(DEV, dtype).contiguous()
    t2, a_, b_ = dev(padc(rnd((M, Ci), 70), Cip)), dev(padc(rnd((M, Ci), 71), Cip)), dev(padc(rnd((M, Ci), 72), Cip))
    g, c, x = dev(padc(rnd((M, Co), 73), Cop)), dev(padc(rnd((M, Co), 74), Cop)), dev(padc(rnd((M, Co), 75), Cop))
    coef_a = torch.cat([padc(rnd((Ci,), 76), Cip), padc(rnd((Ci,), 77, 0.1), Cip), padc(rnd((Ci,), 78, 0.1), Cip)]).to(DEV)
    coef_c = torch.cat([padc(rnd((Co,), 79), Cop), padc(rnd((Co,), 80, 0.1), Cop), padc(rnd((Co,), 81, 0.1), Cop)]).to(DEV)
    ss = torch.cat([padc(rnd((Ci,), 82).abs() + 0.5, Cip), padc(rnd((Ci,), 83, 0.3), Cip)]).to(DEV)
    gate = padc(torch.sigmoid(rnd((B, Ci), 84)), Cip).to(DEV).contiguous()
    Hs = 32
    xs = dev(rnd((B, Hs, Hs, 48), 85))                      # strided shortcut: rows (b, i, j) read pixel (2i, 2j)
    gs = dev(rnd((B * (Hs // 2) * (Hs // 2), Cop), 86))
    dt = ops.dt_code(dtype)
    wsf = int(ops.L.lib().c3d_pw_wgrad_ws_floats(Ci, Cip))
    ws2 = [torch.empty(wsf, dtype=torch.float32, device=DEV) for _ in range(2)]

    def run(chained):
        dws = [torch.full((Co, Ci), 0.25, device=DEV), torch.full((Ci, Co), 0.25, device=DEV), torch.full((Co, 48), 0.25, device=DEV),
               torch.full((Co, Ci), 0.25, device=DEV), torch.full((Ci, Co), 0.25, device=DEV)]
        k = [0]
        def ws():
            k[0] += 1
            return ws2[k[0] & 1] if chained else None
        conv_c = lambda dw: ops.pw_wgrad(g, b_, dw, M=M, K=Ci, N=Co, dw_sn=Ci, dw_sk=1, dtype=dt, p2=c, p_coef=coef_c,
                                         q_mode=ops.PRO_BN_SE_SWISH, q_ss=ss, q_gate=gate, rows_per_sample=rows, chain_ws=ws())
        conv_a = lambda dw: ops.pw_wgrad(t2, x, dw, M=M, K=Co, N=Ci, dw_sn=Co, dw_sk=1, dtype=dt, p2=a_, p_coef=coef_a, chain_ws=ws())
        conv_c(dws[0]); conv_a(dws[1])
        ops.pw_wgrad(gs, xs, dws[2], M=gs.shape[0], K=48, N=Co, dw_sn=48, dw_sk=1, dtype=dt, row_mode=ops.ROWS_STRIDE2, H=Hs, W=Hs,
                     chain_ws=ws())
        conv_c(dws[3]); conv_a(dws[4])
        if chained:
            ops.pw_wgrad_flush()
        torch.cuda.synchronize()
        return [d.cpu() for d in dws]

    plain, chained = run(False), run(True)
    for i, (u, v) in enumerate(zip(plain, chained)):
        assert torch.isfinite(v).all() and (v - 0.25).abs().max().item() > 0, f"launch {i}: nothing was accumulated"
        assert torch.equal(u, v), f"launch {i}: chained reduction differs from the reducer launch by {(u - v).abs().max().item():.3e}"
    ops.pw_wgrad_flush()   # nothing pending: a no-op


# Pending partials are owned by the launch that left them: an UNCHAINED launch that writes the workspace they sit in -- here the
# buffer ops._ws hands out on this stream, which the strided shortcut gradient (first kernel) fills at once -- finds them
# reduced first.  Both dw must equal, BIT FOR BIT, what the two launches give unchained one after the other.
def test_pw_wgrad_unchained_launch_reduces_pending_partials_in_its_workspace():
    _need_gpu()
    from change3d_amd import ops
    dtype = torch.bfloat16
    B, rows = 6, 1024
    M = B * rows
    Ci, Co = 216, 96
    Cip, Cop = ops.cpad(Ci), ops.cpad(Co)
    dev = lambda t: t.to(DEV, dtype).contiguous()
    t2, a_, x = dev(padc(rnd((M, Ci), 70), Cip)), dev(padc(rnd((M, Ci), 71), Cip)), dev(padc(rnd((M, Co), 75), Cop))
    coef_a = torch.cat([padc(rnd((Ci,), 76), Cip), padc(rnd((Ci,), 77, 0.1), Cip), padc(rnd((Ci,), 78, 0.1), Cip)]).to(DEV)
    Hs = 32
    xs = dev(rnd((B, Hs, Hs, 48), 85))
    gs = dev(rnd((B * (Hs // 2) * (Hs // 2), Cop), 86))
    dt = ops.dt_code(dtype)

    def run(shared):
        dws = [torch.full((Ci, Co), 0.25, device=DEV), torch.full((Co, 48), 0.25, device=DEV)]
        ws = ops._ws(t2.device, int(ops.L.lib().c3d_pw_wgrad_ws_floats(Ci, Cip))) if shared else None
        ops.pw_wgrad(t2, x, dws[0], M=M, K=Co, N=Ci, dw_sn=Co, dw_sk=1, dtype=dt, p2=a_, p_coef=coef_a, chain_ws=ws)
        ops.pw_wgrad(gs, xs, dws[1], M=gs.shape[0], K=48, N=Co, dw_sn=48, dw_sk=1, dtype=dt, row_mode=ops.ROWS_STRIDE2, H=Hs, W=Hs)
        if shared:
            assert ops._ws(t2.device, 1).data_ptr() == ws.data_ptr(), "the second launch did not write the first one's workspace"
            ops.pw_wgrad_flush()
        torch.cuda.synchronize()
        return [d.cpu() for d in dws]

    plain, shared = run(False), run(True)
    for i, (u, v) in enumerate(zip(plain, shared)):
        assert torch.isfinite(v).all() and (v - 0.25).abs().max().item() > 0, f"launch {i}: nothing was accumulated"
        assert torch.equal(u, v), f"launch {i}: differs from the unchained launches by {(u - v).abs().max().item():.3e}"


@pytest.mark.parametrize("dtype", DTYPES)
def test_pw_wgrad_row_modes(dtype):
    _need_gpu()
    from change3d_amd import ops
    B, H, W, C = 2, 8, 8, 24
    # stride-2 gather (shortcut conv): dW[n,k] = sum g[m,n] * x[b,2i,2j,k]
    x = q(rnd((B, H, W, C), 40), dtype)
    g = q(rnd((B * (H // 2) * (W // 2), 48), 41), dtype)
    ref = g.t() @ x[:, ::2, ::2].reshape(-1, C)
    dw = torch.zeros((48, C), dtype=torch.float32, device=DEV)
    ops.pw_wgrad(g.to(DEV, dtype).contiguous(), x.to(DEV, dtype).contiguous(), dw, M=g.shape[0], K=C, N=48, dw_sn=C,
                 dw_sk=1, dtype=ops.dt_code(dtype), row_mode=ops.ROWS_STRIDE2, H=H, W=W)
    close(dw, ref, dtype, "stride2", scale=ref.abs().max().item())
    # shifted stride-2 gather with zero padding (ConvTranspose weight gradient, one tap)
    h, w = 4, 4
    t = q(rnd((B * h * w, C), 42), dtype)
    dout = q(rnd((B, 2 * h, 2 * w, C), 43), dtype)
    for (ky, kx) in [(0, 0), (1, 2), (3, 3)]:
        gath = torch.zeros(B, h, w, C)
        for i in range(h):
            for j in range(w):
                yy, xx = 2 * i - 1 + ky, 2 * j - 1 + kx
                if 0 <= yy < 2 * h and 0 <= xx < 2 * w:
                    gath[:, i, j] = dout[:, yy, xx]
        ref = t.t() @ gath.view(-1, C)
        dw16 = torch.zeros((C, C, 16), dtype=torch.float32, device=DEV)
        ops.pw_wgrad(t.to(DEV, dtype).contiguous(), dout.to(DEV, dtype).contiguous(), None, M=B * h * w, K=C, N=C,
                     dw_sn=C * 16, dw_sk=16, dtype=ops.dt_code(dtype), row_mode=ops.ROWS_S2SHIFT, H=2 * h, W=2 * w,
                     dy=ky - 1, dx=kx - 1, dw_ptr=dw16.data_ptr() + (ky * 4 + kx) * 4)
        close(dw16[:, :, ky * 4 + kx], ref, dtype, f"s2shift tap {ky},{kx}", scale=ref.abs().max().item())
        other = dw16.clone()
        other[:, :, ky * 4 + kx] = 0
        assert other.abs().max().item() == 0, "other taps must stay untouched"
    # frame view rows
    T = 3
    full = q(rnd((B, T, h, w, C), 44), dtype)
    p = q(rnd((B * h * w, 48), 45), dtype)
    ref = p.t() @ full[:, 1].reshape(-1, C)
    fd = full.to(DEV, dtype).contiguous()
    dw = torch.zeros((48, C), dtype=torch.float32, device=DEV)
    ops.pw_wgrad(p.to(DEV, dtype).contiguous(), None, dw, M=B * h * w, K=C, N=48, dw_sn=C, dw_sk=1,
                 dtype=ops.dt_code(dtype), row_mode=ops.ROWS_FRAME, rpg=h * w, gstride=T * h * w * C,
                 q_ptr=fd.data_ptr() + 1 * h * w * C * fd.element_size())
    close(dw, ref, dtype, "frame", scale=ref.abs().max().item())


# --------------------------------------------------------------------------------- depthwise
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("C,T", [(54, 3), (108, 5)])
def test_dw333_fwd_bwd(dtype, stride, C, T):
    _need_gpu()
    from change3d_amd import ops
    B, H, W = 2, 16, 24
    Cp = ops.cpad(C)
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    a = q(rnd((B, T, H, W, C), 50), dtype)
    scale, shift = rnd((C,), 51).abs() + 0.5, rnd((C,), 52, 0.3)
    w = rnd((C, 1, 3, 3, 3), 53, 0.3)
    a_r = a.clone().requires_grad_(True)
    w_r = w.clone().requires_grad_(True)
    ra = torch.relu(a_r * scale + shift).permute(0, 4, 1, 2, 3)
    bref = F.conv3d(ra, w_r, stride=(1, stride, stride), padding=1, groups=C)   # [B,C,T,Ho,Wo]
    ss = torch.cat([padc(scale, Cp), padc(shift, Cp)]).to(DEV)
    ad = padc(a, Cp).to(DEV, dtype).contiguous()
    b = torch.full((B, T, Ho, Wo, Cp), float("nan"), dtype=dtype, device=DEV)
    nc = torch.zeros(B * Cp * 2, dtype=torch.float64, device=DEV)
    ops.dw_fwd(ad, ss, w.to(DEV).contiguous(), b, nc, B, T, H, W, C, stride, ops.dt_code(dtype))
    fwd_kernel = ops.last_kernel()
    bre = bref.detach().permute(0, 2, 3, 4, 1)
    if dtype == torch.bfloat16:   # per element: 2^-8 |ref| + 2^-19 sum|term| (tests/test_hotpath_bf16_gpu.py), not 3e-2 of the largest value
        import hotpath_reference as R
        f64 = lambda t: t.detach().double().cpu()   # noqa: E731
        r = R.dw_pair_ratios(f64(a), f64(scale), f64(shift), f64(w).view(C, 27), stride, None, None, None, None, None, y_dev=f64(b[..., :C]),
                             round_operand=fwd_kernel.startswith("dw_fwd_kernel<"))   # (the first kernel rounds its activated tile to bf16)
        assert r["y"] <= 1.0, (fwd_kernel, r)
    else:
        close(b[..., :C], bre, dtype, "dw fwd", scale=bre.abs().max().item())
    if Cp > C:
        assert (b[..., C:].float() == 0).all()
    bq = b[..., :C].float().cpu().double()
    s = nc.cpu().view(B, Cp, 2)[:, :C]
    assert torch.allclose(s[..., 0], bq.sum((1, 2, 3)), rtol=1e-5, atol=1e-3)
    assert torch.allclose(s[..., 1], (bq * bq).sum((1, 2, 3)), rtol=1e-5, atol=1e-3)
    # backward: db = cA*t1 + cB[n] + cC*b ; check data grad (with relu mask) + sums + weight grad
    t1 = q(rnd((B, T, Ho, Wo, C), 54), dtype)
    cA, cC, cB = rnd((C,), 55), rnd((C,), 56, 0.1), rnd((B, C), 57, 0.1)
    bst = b[..., :C].float().cpu()
    db = cA * t1 + cB[:, None, None, None, :] + cC * bst
    bref.backward(db.permute(0, 4, 1, 2, 3))
    t2_ref = a_r.grad                                   # includes relu mask and scale...
    # device returns d(relu out) masked, i.e. grad wrt pa = a*scale+shift  => divide scale out
    t2_ref = t2_ref / scale
    t2 = torch.empty_like(ad)
    dsums = torch.zeros(2 * C, dtype=torch.float64, device=DEV)
    t1d = padc(t1, Cp).to(DEV, dtype).contiguous()
    mean_a, rstd_a = rnd((C,), 58, 0.5), rnd((C,), 59).abs() + 0.5
    mr = torch.cat([padc(mean_a, Cp), padc(rstd_a, Cp)]).to(DEV)
    dw = torch.zeros((C, 27), dtype=torch.float32, device=DEV)
    # one pass: data gradient (with the ReLU mask), BatchNorm_a-backward sums and weight gradient against torch autograd
    _check_fused_dw(ops, t1d, b, padc(cA, Cp).to(DEV), padc(cB, Cp).to(DEV).contiguous(), padc(cC, Cp).to(DEV),
                    w.to(DEV).contiguous(), ad, ss, mr, t2_ref, a, mean_a, rstd_a, w_r.grad.view(C, 27), B, T, H, W, C, dtype, stride)


def _check_fused_dw(ops, t1d, bd, cAd, cBd, cCd, wd, ad, ss, mr, t2_ref, a, mean_a, rstd_a, dw_ref, B, T, H, W, C, dtype, stride=1):
    """c3d_dw333_bwd_fused against torch-CPU autograd of relu(bn(a)) -> conv3d (the separate data-gradient / weight-gradient
    kernels it was once compared with bit for bit were deleted in round 4)."""
    t2f = torch.full_like(ad, float("nan"))
    dsf = torch.zeros(2 * C, dtype=torch.float64, device=DEV)
    dwf = torch.zeros((C, 27), dtype=torch.float32, device=DEV)
    ops.dw_bwd_fused(t1d, bd, cAd, cBd, cCd, wd, ad, ss, mr, t2f, dsf, dwf, B, T, H, W, C, ops.dt_code(dtype), stride)
    torch.cuda.synchronize()
    if dtype == torch.bfloat16:   # per-element bounds against the float64 restatement (f32 legs: autograd, as before)
        import hotpath_reference as R
        f64 = lambda t: t.detach().double().cpu()   # noqa: E731
        Cp = ad.shape[-1]
        r = R.dw_pair_ratios(f64(ad[..., :C]), f64(ss[:C]), f64(ss[Cp:Cp + C]), f64(wd).view(C, 27), stride, f64(t1d[..., :C]), f64(bd[..., :C]),
                             f64(cAd[:C]), f64(cBd[:, :C]), f64(cCd[:C]), t2_dev=f64(t2f[..., :C]), dw_dev=f64(dwf))
        assert r["t2"] <= 1.0 and r["dW"] <= 1.0, r
    else:
        close(t2f[..., :C], t2_ref, dtype, "dw bwd data", scale=t2_ref.abs().max().item())
    if t2f.shape[-1] > C:
        assert (t2f[..., C:].float() == 0).all()
    t2q = t2f[..., :C].float().cpu().double()
    sd = dsf.cpu()
    assert torch.allclose(sd[:C], t2q.sum((0, 1, 2, 3)), rtol=1e-5, atol=1e-3 * max(1.0, B / 8))
    assert torch.allclose(sd[C:], (t2q * ((a - mean_a) * rstd_a).double()).sum((0, 1, 2, 3)), rtol=1e-5, atol=1e-3 * max(1.0, B / 8))
    if dtype != torch.bfloat16:
        close(dwf, dw_ref, dtype, "dw wgrad", scale=dw_ref.abs().max().item())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,H,W,C,stride", [
    (5, 20, 28, 216, 1),    # ragged tiles, 7 channel chunks with an empty last vector
    (3, 18, 18, 54, 2),     # ragged stride-2 map
    (3, 17, 19, 54, 2),     # odd extents under stride 2 (the last 2x2 quad of a row / column is partial)
    (2, 15, 9, 108, 2),
    (40, 24, 24, 54, 1),    # workgroup walks cross sample boundaries (per-sample coefB rows)
    (1100, 8, 8, 54, 1),    # one tile per sample: a walk touches > 8 samples
])
def test_dw333_backward_walks(dtype, B, H, W, C, stride):
    """The fused depthwise backward kernel on shapes that exercise the tile walks (ragged tiles, walks across sample
    boundaries, one tile per sample, odd extents under stride 2)."""
    _need_gpu()
    from change3d_amd import ops
    T = 3
    Cp = ops.cpad(C)
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    a = q(rnd((B, T, H, W, C), 150), dtype)
    scale, shift = rnd((C,), 151).abs() + 0.5, rnd((C,), 152, 0.3)
    w = rnd((C, 1, 3, 3, 3), 153, 0.3)
    a_r = a.clone().requires_grad_(True)
    w_r = w.clone().requires_grad_(True)
    bref = F.conv3d(torch.relu(a_r * scale + shift).permute(0, 4, 1, 2, 3), w_r, stride=(1, stride, stride),
                    padding=1, groups=C)
    bst = q(bref.detach().permute(0, 2, 3, 4, 1), dtype)
    t1 = q(rnd((B, T, Ho, Wo, C), 154), dtype)
    cA, cC, cB = rnd((C,), 155), rnd((C,), 156, 0.1), rnd((B, C), 157, 0.1)
    db = cA * t1 + cB[:, None, None, None, :] + cC * bst
    bref.backward(db.permute(0, 4, 1, 2, 3))
    t2_ref = a_r.grad / scale
    ss = torch.cat([padc(scale, Cp), padc(shift, Cp)]).to(DEV)
    mean_a, rstd_a = rnd((C,), 158, 0.5), rnd((C,), 159).abs() + 0.5
    mr = torch.cat([padc(mean_a, Cp), padc(rstd_a, Cp)]).to(DEV)
    ad = padc(a, Cp).to(DEV, dtype).contiguous()
    bd = padc(bst, Cp).to(DEV, dtype).contiguous()
    t1d = padc(t1, Cp).to(DEV, dtype).contiguous()
    cAd, cBd, cCd = padc(cA, Cp).to(DEV), padc(cB, Cp).to(DEV).contiguous(), padc(cC, Cp).to(DEV)
    wd = w.to(DEV).contiguous()
    _check_fused_dw(ops, t1d, bd, cAd, cBd, cCd, wd, ad, ss, mr, t2_ref, a, mean_a, rstd_a, w_r.grad.view(C, 27), B, T, H, W, C, dtype, stride)


@pytest.mark.parametrize("B,H,W,C", [
    (2, 16, 24, 54),        # two channel chunks, the second one short
    (5, 20, 28, 216),       # ragged tiles, 7 chunks
    (3, 40, 40, 108),       # 25 tiles per sample: walks of more than three tiles (every ring slot is reused)
    (40, 24, 24, 54),       # walks across sample boundaries
    (1100, 8, 8, 54),       # one tile per sample
    (2, 8, 72, 24),         # a single tile row
])
@pytest.mark.parametrize("T,ring", [(3, 9), (3, 13), (5, 9), (5, 13)])   # ring bits: 1 on, 4 requests spread over the tap walk, 8 every map size
def test_dw_bwd_ring_kernel_is_bit_identical_to_the_register_prefetch_kernel(B, H, W, C, T, ring):
    """C3D_OPT_DW_RING bit 0: the LDS-DMA ring variant of c3d_dw333_bwd_fused (bf16, stride 1, T = 3) changes how the raw rows
    reach the workgroup, not one operation of the arithmetic: data gradient, BatchNorm_a sums and weight gradient must be
    bit-identical to the register-prefetch kernel's (the f32 atomics of the flush commute only up to rounding across
    workgroups: the weight gradient is compared at 1e-5 of its scale, everything else exactly)."""
    _need_gpu()
    from change3d_amd import ops
    dtype = torch.bfloat16
    if T == 5 and B > 100:
        B = 300
    Cp = ops.cpad(C)
    t1d = padc(q(rnd((B, T, H, W, C), 250), dtype), Cp).to(DEV, dtype).contiguous()
    bd = padc(q(rnd((B, T, H, W, C), 251), dtype), Cp).to(DEV, dtype).contiguous()
    ad = padc(q(rnd((B, T, H, W, C), 252), dtype), Cp).to(DEV, dtype).contiguous()
    cAd, cCd = padc(rnd((C,), 253), Cp).to(DEV), padc(rnd((C,), 254, 0.1), Cp).to(DEV)
    cBd = padc(rnd((B, C), 255, 0.1), Cp).to(DEV).contiguous()
    wd = rnd((C, 27), 256, 0.3).to(DEV).contiguous()
    ss = torch.cat([padc(rnd((C,), 257).abs() + 0.5, Cp), padc(rnd((C,), 258, 0.3), Cp)]).to(DEV)
    mr = torch.cat([padc(rnd((C,), 259, 0.5), Cp), padc(rnd((C,), 260).abs() + 0.5, Cp)]).to(DEV)
    out, names = {}, {}
    try:
        for rv in (0, ring):
            ops.set_option(ops.OPT_DW_RING, rv)
            t2 = torch.full_like(ad, float("nan"))
            ds = torch.zeros(2 * C, dtype=torch.float64, device=DEV)
            dw = torch.zeros((C, 27), dtype=torch.float32, device=DEV)
            ops.dw_bwd_fused(t1d, bd, cAd, cBd, cCd, wd, ad, ss, mr, t2, ds, dw, B, T, H, W, C, ops.dt_code(dtype), 1)
            names[rv] = ops.last_kernel()
            torch.cuda.synchronize()
            out[rv] = (t2, ds, dw)
    finally:
        ops.set_option(ops.OPT_DW_RING, 13)
    assert names[0] == f"dw_bwd_fused_kernel<unsigned short, {T}, 1>", names
    assert names[ring] == f"dw_bwd_ring_kernel<{T}, {'true' if ring & 4 else 'false'}>", names
    assert torch.equal(out[0][0].view(torch.int16), out[ring][0].view(torch.int16)), "data gradient differs"
    assert torch.allclose(out[0][1], out[ring][1], rtol=1e-12, atol=0), "BatchNorm_a sums differ"
    scale = out[0][2].abs().max().item()
    # (the flush adds one f32 atomic per workgroup and tap: 2 200 of them in arbitrary order at B = 1100 -- 1.3e-6 of the scale
    # between two runs of the SAME kernel)
    assert (out[0][2] - out[ring][2]).abs().max().item() <= 1e-5 * scale, "weight gradient differs"


# --------------------------------------------------------------------------- loss / optimizer
def test_bce_dice_and_adam():
    _need_gpu()
    from change3d_amd.model.utils import BCEDiceLoss
    from change3d_amd import ops
    p = torch.sigmoid(rnd((2, 1, 32, 32), 60, 3.0))
    p[0, 0, 0, 0], p[0, 0, 0, 1] = 1.0, 0.0  # saturated probabilities exercise the clamps
    t = (rnd((2, 1, 32, 32), 61) > 0.8).float()
    pr = p.clone().requires_grad_(True)
    bce = F.binary_cross_entropy(pr, t)
    inter = (pr * t).sum()
    lref = bce + 1 - (2 * inter + 1e-5) / (pr.sum() + t.sum() + 1e-5)
    lref.backward()
    pd = p.to(DEV).requires_grad_(True)
    loss = BCEDiceLoss(pd, t.to(DEV))
    (loss * 1.0).backward()
    assert abs(loss.item() - lref.item()) < 1e-5 * max(1.0, abs(lref.item()))
    gd, gr = pd.grad.cpu(), pr.grad
    assert torch.allclose(gd, gr, rtol=1e-4, atol=1e-6 * gr.abs().max().item() + 1e-9), (gd - gr).abs().max()
    # Adam
    n = 1000
    w0, g0 = rnd((n,), 62), rnd((n,), 63)
    wr = torch.nn.Parameter(w0.clone())
    opt = torch.optim.Adam([wr], 2e-4, (0.9, 0.99), eps=1e-8, weight_decay=1e-4)
    wd = w0.to(DEV)
    m = torch.zeros(n, device=DEV)
    v = torch.zeros(n, device=DEV)
    for step in range(1, 4):
        wr.grad = g0 * step
        opt.step()
        bc1, bc2 = 1 - 0.9 ** step, 1 - 0.99 ** step
        ops.adam_step(wd, (g0 * step).to(DEV), m, v, n, None, 2e-4, bc1, bc2 ** 0.5, 0.9, 0.99, 1e-8, 1e-4)
    assert torch.allclose(wd.cpu(), wr.detach(), rtol=1e-6, atol=1e-7), (wd.cpu() - wr.detach()).abs().max()


def test_confusion_matrix():
    _need_gpu()
    from change3d_amd.utils.metric_tool import ConfuseMatrixMeter, get_confuse_matrix
    p = torch.rand(2, 1, 64, 64)
    p[0, 0, 0, :8] = 0.5  # strict '>' 0.5
    t = (torch.rand(2, 1, 64, 64) > 0.9).float()
    meter = ConfuseMatrixMeter(2)
    meter.update_cm_device(p.to(DEV), t.to(DEV))
    meter.sync()
    pred = torch.where(p > 0.5, torch.ones_like(p), torch.zeros_like(p)).long()
    ref = get_confuse_matrix(2, t.numpy(), pred.numpy())
    assert (meter.sum == ref).all(), (meter.sum, ref)


def test_scd_losses_vs_torch():
    """CrossEntropyLoss2d(ignore_index=0) and ChangeSimilarity (reference model/utils.py:171-203) through the
    C ABI, on channel-sliced logits exactly as scripts/train_SCD.py:226-228 passes them."""
    _need_gpu()
    from change3d_amd.model.utils import ChangeSimilarity, CrossEntropyLoss2d
    B, NC, H, W = 3, 7, 20, 24
    pre, post = rnd((B, NC, H, W), 300, 2.0), rnd((B, NC, H, W), 301, 2.0)
    g = np.random.default_rng(302)
    lab = torch.from_numpy(g.integers(0, NC, size=(B, H, W))).long()
    chg = torch.from_numpy((g.random((B, H, W)) < 0.3).astype(np.int64))
    lab = lab * chg
    pr, qr = pre.clone().requires_grad_(True), post.clone().requires_grad_(True)
    ce_ref = F.nll_loss(F.log_softmax(pr, 1), lab, ignore_index=0)
    p1 = F.softmax(pr[:, 1:], 1).permute(0, 2, 3, 1).reshape(-1, NC - 1)
    p2 = F.softmax(qr[:, 1:], 1).permute(0, 2, 3, 1).reshape(-1, NC - 1)
    tgt = ((~chg.bool()).float() - chg.float()).reshape(-1)
    sim_ref = F.cosine_embedding_loss(p1, p2, tgt, margin=0.0)
    (0.5 * ce_ref + 2.0 * sim_ref).backward()
    pd, qd = pre.to(DEV).requires_grad_(True), post.to(DEV).requires_grad_(True)
    ce = CrossEntropyLoss2d(ignore_index=0)(pd, lab.to(DEV))
    sim = ChangeSimilarity()(pd[:, 1:], qd[:, 1:], chg.to(DEV).unsqueeze(1))
    (0.5 * ce + 2.0 * sim).backward()
    assert abs(ce.item() - ce_ref.item()) < 2e-6 * max(1.0, abs(ce_ref.item()))
    assert abs(sim.item() - sim_ref.item()) < 2e-6
    close(pd.grad, pr.grad, torch.float32, "d pre", scale=pr.grad.abs().max().item())
    close(qd.grad, qr.grad, torch.float32, "d post", scale=qr.grad.abs().max().item())
    # every pixel ignored -> NaN, as torch
    z = torch.zeros_like(lab)
    assert torch.isnan(CrossEntropyLoss2d(ignore_index=0)(pd.detach(), z.to(DEV))).item()


# ---- the same kernels where their grid-stride loops wrap (csrc/train_ops.hip: bce_dice_reduce_kernel and confusion_kernel run
# at most 1024 x 256 threads, ce2d_reduce / cossim_reduce 2048 x 256, the backward kernels and adam_kernel 4096 x 256; the cases
# above stay inside one pass).  u = 2^-24, one f32 rounding; "1 ulp" of a library function is 2 u of its value.
U32 = 2.0 ** -24


def test_bce_dice_and_confusion_where_the_grid_stride_loops_wrap():
    """n = 3 x 262 144 + 77: every thread of the reduce kernels takes three elements, 77 of them a fourth.  Against float64 of the
    same f32 inputs.  Loss: a term (t - 1) log(1 - p) - t log p is computed in f32 -- logf 1 ulp, the product and the difference
    one rounding each: 4 u of |t log p| + |(1 - t) log(1 - p)|, and 1 - p is rounded before the logarithm, u of 1 - p, which moves
    log(1 - p) by u; the sums are double; the finalize kernel rounds bce, the three dice sums, and adds / divides in f32: 16 u of
    |bce| + 1 + dice.  Gradient: (p - t) / max((1 - p) p, 1e-12) / n - (2 t / D - N / D^2): eight f32 roundings in each half."""
    _need_gpu()
    from change3d_amd import ops
    n = 262144 * 3 + 77
    p = torch.sigmoid(rnd((n,), 70, 3.0))
    p[0], p[1], p[n - 1], p[n - 2] = 1.0, 0.0, 1.0, 0.0         # saturated probabilities exercise the clamps, in the first and the last pass
    p[5:13] = 0.5                                                # strict '>' 0.5 in the confusion matrix
    t = (rnd((n,), 71) > 0.8).float()
    t[0], t[1], t[n - 1], t[n - 2] = 0.0, 1.0, 1.0, 0.0
    pd, td = p.to(DEV), t.to(DEV)
    sums4 = torch.zeros(4, dtype=torch.float64, device=DEV)
    loss = torch.full((1,), float("nan"), device=DEV)
    ops.bce_dice_fwd(pd, td, sums4, loss)
    dprob = torch.full((n,), float("nan"), device=DEV)
    dloss = torch.full((1,), 0.75, device=DEV)
    ops.bce_dice_bwd(pd, td, sums4, dloss, dprob)
    cm = torch.zeros(4, dtype=torch.int64, device=DEV)
    ops.confusion2(pd, td, cm)
    torch.cuda.synchronize()
    P, T = p.double(), t.double()
    lp, l1p = torch.log(P).clamp_min(-100.0), torch.log(1 - P).clamp_min(-100.0)
    term_mag = (T * lp).abs() + ((1 - T) * l1p).abs()
    bce = ((T - 1) * l1p - T * lp).mean()
    inter, sp, st = (P * T).sum(), P.sum(), T.sum()
    Dn, Nn = sp + st + 1e-5, 2 * inter + 1e-5
    ref = bce + 1 - Nn / Dn
    tol = (4 * U32 * term_mag + U32).mean() + 16 * U32 * (bce.abs() + 1 + Nn / Dn)
    print(f"\nLOSS-WRAP bce_dice loss error/bound {abs(loss.item() - ref.item()) / tol.item():.3f}")
    assert abs(loss.item() - ref.item()) <= tol.item(), (loss.item(), ref.item(), tol.item())
    gb = (P - T) / ((1 - P) * P).clamp_min(1e-12) / n
    gd = 2 * T / Dn - Nn / (Dn * Dn)
    gref = 0.75 * (gb - gd)
    gtol = 0.75 * 16 * U32 * (gb.abs() + (2 * T / Dn).abs() + Nn / (Dn * Dn))
    err = (dprob.cpu().double() - gref).abs()
    print(f"LOSS-WRAP bce_dice gradient worst error/bound {(err / gtol).max().item():.3f}")
    assert bool((err <= gtol).all()), (err / gtol).max()
    pred = (p > 0.5).long()
    cm_ref = torch.bincount((2 * t.long() + pred), minlength=4)
    assert torch.equal(cm.cpu(), cm_ref), (cm, cm_ref)


def test_scd_losses_where_the_grid_stride_loops_wrap():
    """B x HW = 3 x 592 x 592 = 1 051 392 pixels, just above the 2 x 524 288 the reduce kernels cover in two passes (and above the
    1 048 576 of the backward kernels): some threads take a third pixel (a second one in the backward).  NC = 7 on views whose
    channel AND batch strides differ from a dense tensor's (rows 0 .. H - 1 of channels 1 .. 7 of a [B][8][H + 1][W] tensor).
    Gradients per element against float64 autograd.  A softmax value p_c carries r = (16 + 2 max_c |x_c - max|) u <= 64 u (the
    difference is rounded before expf (2 ulp), seven additions, a reciprocal, a product).  Cross entropy: scale (p_c - onehot):
    scale (r p_c + 4 u |p_c - onehot|).  ChangeSimilarity: dot, |p1|^2, |p2|^2 are 8-term fma sums of such values (2 r + 8 u each),
    den = sqrt(n1 n2) and cos = dot / den follow (4 r + 19 u), g_c = gcos (p2_c / den - cos p1_c / n1) has (6 r + 30 u) of the
    magnitude G_c = |gcos| (p2_c / den + |cos| p1_c / n1), a = sum g_c p1_c adds (r + 8 u) of A = sum G_c p1_c, and
    d_c = p1_c (g_c - a) one more r + 2 u of p1_c (G_c + A)."""
    _need_gpu()
    from change3d_amd import ops
    B, NC, H, W = 3, 7, 592, 592
    assert 2 * 524288 < B * H * W < 2 * 524288 + 4096
    full1, full2 = rnd((B, NC + 1, H + 1, W), 310, 2.0).to(DEV), rnd((B, NC + 1, H + 1, W), 311, 2.0).to(DEV)
    x1, x2 = full1[:, 1:, :H], full2[:, 1:, :H]
    assert x1.stride(1) != H * W and x1.stride(0) != NC * H * W
    g = np.random.default_rng(312)
    chg = torch.from_numpy((g.random((B, H, W)) < 0.3).astype(np.int64))
    lab = (torch.from_numpy(g.integers(0, NC, size=(B, H, W))).long() * chg).to(DEV)
    chg = chg.to(DEV)
    # ---- device
    sums2, ce = torch.zeros(2, dtype=torch.float64, device=DEV), torch.full((1,), float("nan"), device=DEV)
    ops.ce2d_fwd(x1, lab, 0, sums2, ce)
    dl = torch.full((1,), 0.5, device=DEV)
    dce = torch.full((B, NC, H, W), float("nan"), device=DEV)
    ops.ce2d_bwd(x1, lab, 0, sums2, dl, dce)
    sums1, sim = torch.zeros(1, dtype=torch.float64, device=DEV), torch.full((1,), float("nan"), device=DEV)
    ops.cossim_fwd(x1, x2, chg.reshape(B, -1), sums1, sim)
    d2 = torch.full((1,), 2.0, device=DEV)
    dx1, dx2 = torch.full((B, NC, H, W), float("nan"), device=DEV), torch.full((B, NC, H, W), float("nan"), device=DEV)
    ops.cossim_bwd(x1, x2, chg.reshape(B, -1), d2, dx1, dx2)
    torch.cuda.synchronize()
    # ---- float64 autograd, on the device
    a, b = x1.double().clone().requires_grad_(True), x2.double().clone().requires_grad_(True)
    ce_ref = F.nll_loss(F.log_softmax(a, 1), lab, ignore_index=0)
    (0.5 * ce_ref).backward()
    ce_grad = a.grad.clone()
    a.grad = None
    p1 = F.softmax(a, 1).permute(0, 2, 3, 1).reshape(-1, NC)
    p2 = F.softmax(b, 1).permute(0, 2, 3, 1).reshape(-1, NC)
    tgt = ((~chg.bool()).double() - chg.double()).reshape(-1)
    sim_ref = F.cosine_embedding_loss(p1, p2, tgt, margin=0.0)
    (2.0 * sim_ref).backward()
    assert abs(ce.item() - ce_ref.item()) < 2e-6 * max(1.0, abs(ce_ref.item()))
    assert abs(sim.item() - sim_ref.item()) < 2e-6
    with torch.no_grad():
        md = max((a.max(1).values - a.min(1).values).max().item(), (b.max(1).values - b.min(1).values).max().item())
        assert md <= 24.0, md
        r = 64 * U32
        count = (lab != 0).sum().double()
        sm = F.softmax(a, 1)
        onehot = F.one_hot(lab, NC).permute(0, 3, 1, 2).double()
        live = (lab != 0).unsqueeze(1).double()
        tol = 0.5 / count * (r * sm + 4 * U32 * (sm - onehot).abs()) * live
        err = (dce.double() - ce_grad).abs()
        assert bool((dce[(lab == 0).unsqueeze(1).expand_as(dce)] == 0).all())
        worst = (err[tol > 0] / tol[tol > 0]).max().item()
        print(f"\nLOSS-WRAP ce2d gradient worst error/bound {worst:.3f}")
        assert bool((err <= tol).all()), worst
        q1, q2 = F.softmax(a, 1), F.softmax(b, 1)                       # [B][NC][H][W]
        dot, n1, n2 = (q1 * q2).sum(1, keepdim=True), (q1 * q1).sum(1, keepdim=True) + 1e-12, (q2 * q2).sum(1, keepdim=True) + 1e-12
        den = torch.sqrt(n1 * n2)
        cs = dot / den
        gcos = 2.0 / (B * H * W)
        for name, dev, grad, pa, pb, na in (("d x1", dx1, a.grad, q1, q2, n1), ("d x2", dx2, b.grad, q2, q1, n2)):
            G = gcos * (pb / den + cs.abs() * pa / na)
            A = (G * pa).sum(1, keepdim=True)
            eg = (6 * r + 30 * U32) * G
            ea = (eg * pa).sum(1, keepdim=True) + (r + 8 * U32) * A
            tol = pa * (eg + ea) + (r + 2 * U32) * pa * (G + A)
            err = (dev.double() - grad).abs()
            worst = (err / tol).max().item()
            print(f"LOSS-WRAP cossim gradient {name} worst error/bound {worst:.3f}")
            assert bool((err <= tol).all()), (name, worst)


def test_adam_where_the_grid_stride_loop_wraps_with_host_and_device_hyper_parameters():
    """n = 2 x 1 048 576 + 333: adam_kernel runs 4096 x 256 threads, every one takes two elements and 333 a third.  Three steps,
    once with lr / bias corrections as host arguments and once through hparams_dev (the leg the captured step uses): the two runs
    are bit-identical, and both meet the tolerance test_bce_dice_and_adam uses against torch.optim.Adam."""
    _need_gpu()
    from change3d_amd import ops
    n = 1048576 * 2 + 333
    w0, g0 = rnd((n,), 64), rnd((n,), 65)
    wr = torch.nn.Parameter(w0.clone())
    opt = torch.optim.Adam([wr], 2e-4, (0.9, 0.99), eps=1e-8, weight_decay=1e-4)
    state = [(w0.to(DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)) for _ in range(2)]
    for step in range(1, 4):
        wr.grad = g0 * step
        opt.step()
        bc1, bc2 = 1 - 0.9 ** step, 1 - 0.99 ** step
        gd = (g0 * step).to(DEV)
        (wa, ma, va), (wb, mb, vb) = state
        ops.adam_step(wa, gd, ma, va, n, None, 2e-4, bc1, bc2 ** 0.5, 0.9, 0.99, 1e-8, 1e-4)
        hp = torch.tensor([2e-4, bc1, bc2 ** 0.5], dtype=torch.float32, device=DEV)
        ops.adam_step(wb, gd, mb, vb, n, hp, 0.0, 1.0, 1.0, 0.9, 0.99, 1e-8, 1e-4)       # the host values must be ignored
    torch.cuda.synchronize()
    for ta, tb in zip(*state):
        assert torch.equal(ta, tb)
    for wd in (state[0][0], state[1][0]):
        assert torch.allclose(wd.cpu(), wr.detach(), rtol=1e-6, atol=1e-7), (wd.cpu() - wr.detach()).abs().max()


# --------------------------------------------------------------- consumer-side BatchNorm finalisation
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C,T,stride,shape", [(54, 3, 1, (2, 16, 24)), (216, 3, 1, (3, 16, 16)), (108, 5, 1, (2, 16, 24)),
                                              (54, 3, 2, (2, 16, 24)), (432, 3, 2, (2, 8, 8)), (108, 3, 2, (2, 40, 72))])
def test_dw_fwd_with_folded_bn_finalize_is_bit_identical(dtype, C, T, stride, shape):
    """c3d_dw333_fwd_fin (scale/shift rebuilt from the producer's sums in the kernel's prologue, csrc/bn_fin.h) against
    c3d_bn_finalize + c3d_dw333_fwd: output, per-sample statistics, saved scale/shift and mean/rstd, running
    statistics and num_batches_tracked are bit-identical (stride 2, three frames: the polyphase kernel's prologue)."""
    _need_gpu()
    from change3d_amd import ops
    B, H, W = shape
    Cp = ops.cpad(C)
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    count = float(B * T * H * W)
    a = padc(q(rnd((B, T, H, W, C), 60), dtype), Cp).to(DEV, dtype).contiguous()
    w = rnd((C, 1, 3, 3, 3), 61, 0.3).to(DEV).contiguous()
    g = torch.Generator().manual_seed(62)
    sums = torch.zeros(16, 2, C, dtype=torch.float64)
    sums[:, 0] = torch.randn(16, C, generator=g, dtype=torch.float64) * count / 64
    sums[:, 1] = (torch.rand(16, C, generator=g, dtype=torch.float64) + 0.5) * count / 8
    sums = sums.to(DEV)

    def bn():
        m = torch.nn.BatchNorm3d(C)
        with torch.no_grad():
            m.weight.copy_(rnd((C,), 63).abs() + 0.5); m.bias.copy_(rnd((C,), 64, 0.3))
            m.running_mean.copy_(rnd((C,), 65, 0.2)); m.running_var.copy_(rnd((C,), 66).abs() + 0.3)
        return m.to(DEV)

    outs = []
    for folded in (False, True):
        m = bn()
        ss = torch.full((2 * Cp,), float("nan"), device=DEV)
        mr = torch.full((2 * Cp,), float("nan"), device=DEV)
        b = torch.full((B, T, Ho, Wo, Cp), float("nan"), dtype=dtype, device=DEV)
        nc = torch.zeros(B * Cp * 2, dtype=torch.float64, device=DEV)
        if folded:
            ops.dw_fwd_fin(a, ops.fin_consume(sums, m, count, ss, mr), w, b, nc, B, T, H, W, C, stride, ops.dt_code(dtype))
        else:
            ops.bn_finalize(sums, count, m, C, ss, mr, True, stripes=16)
            ops.dw_fwd(a, ss, w, b, nc, B, T, H, W, C, stride, ops.dt_code(dtype))
        torch.cuda.synchronize()
        outs.append((b, nc, ss, mr, m.running_mean.clone(), m.running_var.clone(), m.num_batches_tracked.clone()))
    for i, (x0, x1) in enumerate(zip(*outs)):
        assert torch.equal(x0, x1), i
    assert int(outs[1][6]) == 1 and torch.isfinite(outs[1][0].float()).all() and outs[1][0].float().abs().max() > 0


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C,mode,M", [(96, 1, 3000), (48, 2, 777), (24, 3, 5000), (192, 1, 640), (54, 2, 1024 * 36 + 3000)])
def test_block_out_fwd_with_folded_bn_finalize_is_bit_identical(dtype, C, mode, M):
    """c3d_block_out_fwd_fin against c3d_bn_finalize (x1 or x2) + c3d_block_out_fwd: identical y, vectors and buffers
    (modes: 1 identity shortcut, 2 shortcut conv + BatchNorm, 3 shortcut conv without BatchNorm).  The last case (C = 54:
    36 rows per workgroup) walks past the folded launch's cap of 1024 workgroups; the unfolded leg is tied to float64 by
    tests/test_elementwise_gpu.py."""
    _need_gpu()
    from change3d_amd import ops
    Cp = ops.cpad(C)
    c = padc(q(rnd((M, C), 70), dtype), Cp).to(DEV, dtype).contiguous()
    s = padc(q(rnd((M, C), 71), dtype), Cp).to(DEV, dtype).contiguous()
    g = torch.Generator().manual_seed(72)

    def mk_sums():
        t = torch.zeros(16, 2, C, dtype=torch.float64)
        t[:, 0] = torch.randn(16, C, generator=g, dtype=torch.float64) * M / 64
        t[:, 1] = (torch.rand(16, C, generator=g, dtype=torch.float64) + 0.5) * M / 8
        return t.to(DEV)

    sums_c, sums_1 = mk_sums(), mk_sums()

    def bn(seed):
        m = torch.nn.BatchNorm3d(C)
        with torch.no_grad():
            m.weight.copy_(rnd((C,), seed).abs() + 0.5); m.bias.copy_(rnd((C,), seed + 1, 0.3))
        return m.to(DEV)

    outs = []
    for folded in (False, True):
        mc, m1 = bn(73), bn(75)
        v = [torch.full((2 * Cp,), float("nan"), device=DEV) for _ in range(4)]   # ss_c, mr_c, ss_1, mr_1
        y = torch.full((M, Cp), float("nan"), dtype=dtype, device=DEV)
        if folded:
            f1 = ops.fin_consume(sums_1, m1, float(M), v[2], v[3]) if mode == 2 else None
            ops.block_out_fwd_fin(c, ops.fin_consume(sums_c, mc, float(M), v[0], v[1]), s, f1, mode, y, M, C, ops.dt_code(dtype))
        else:
            ops.bn_finalize(sums_c, float(M), mc, C, v[0], v[1], True, stripes=16)
            if mode == 2:
                ops.bn_finalize(sums_1, float(M), m1, C, v[2], v[3], True, stripes=16)
            ops.block_out_fwd(c, v[0], s, v[2] if mode == 2 else None, mode, y, M, Cp, ops.dt_code(dtype))
        torch.cuda.synchronize()
        keep = [y, v[0], v[1], mc.running_mean.clone(), mc.running_var.clone(), mc.num_batches_tracked.clone()]
        if mode == 2:
            keep += [v[2], v[3], m1.running_mean.clone(), m1.num_batches_tracked.clone()]
        outs.append(keep)
    for i, (x0, x1) in enumerate(zip(*outs)):
        assert torch.equal(x0, x1), i
    assert torch.isfinite(outs[1][0].float()).all() and outs[1][0].float().abs().max() > 0


@pytest.mark.parametrize("C,shape", [(54, (2, 40, 72)), (216, (3, 32, 32)), (108, (1, 64, 64))])
def test_dw_fwd_toeplitz_mfma_experiment_matches_the_valu_kernel(C, shape, monkeypatch):
    """csrc/dw_toeplitz.hip (experiment, C3D_DW_TZ=1): same output and per-sample statistics as the default kernel up
    to the bf16 rounding of its MFMA operands (activations after BN+ReLU and weights).  The experiment is linked into
    the instrumented build only (`python __graft_entry__.py --tuning`, loaded through C3D_LIB)."""
    _need_gpu()
    if "tune" not in os.path.basename(os.environ.get("C3D_LIB", "")):
        pytest.skip("Toeplitz-MFMA experiment: instrumented build only (C3D_LIB=.../libchange3d_hip_tune.so)")
    from change3d_amd import ops
    B, H, W = shape
    T, dtype = 3, torch.bfloat16
    Cp = ops.cpad(C)
    a = padc(q(rnd((B, T, H, W, C), 80), dtype), Cp).to(DEV, dtype).contiguous()
    scale, shift = rnd((C,), 81).abs() + 0.5, rnd((C,), 82, 0.3)
    ss = torch.cat([padc(scale, Cp), padc(shift, Cp)]).to(DEV)
    w = rnd((C, 1, 3, 3, 3), 83, 0.3).to(DEV).contiguous()
    outs = []
    for tz in ("0", "1"):
        monkeypatch.setenv("C3D_DW_TZ", tz)
        b = torch.full((B, T, H, W, Cp), float("nan"), dtype=dtype, device=DEV)
        nc = torch.zeros(B * Cp * 2, dtype=torch.float64, device=DEV)
        ops.dw_fwd(a, ss, w, b, nc, B, T, H, W, C, 1, ops.dt_code(dtype))
        torch.cuda.synchronize()
        outs.append((b.float().cpu(), nc.cpu()))
    (b0, n0), (b1, n1) = outs
    sc = b0.abs().max().item()
    assert sc > 0.1 and torch.isfinite(b1).all()
    assert (b0 - b1).abs().max().item() < 3e-2 * sc and (b0 - b1).abs().mean().item() < 3e-3 * sc
    assert (b1[..., C:] == 0).all()
    assert torch.allclose(n0, n1, rtol=2e-2, atol=2e-2 * n0.abs().max().item())


@pytest.mark.parametrize("Cin,Cinner,M", [(96, 216, 3000), (48, 108, 5003), (24, 54, 8192)])
def test_residual_add_fused_into_conv_a_is_bit_identical(Cin, Cinner, M):
    """conv_a with the previous block's residual add in its prologue (c3d_pw_args.pro_out + fin, bf16) against
    c3d_block_out_fwd_fin followed by the plain conv_a: identical y, conv output, BN_a statistics, BatchNorm_c vectors
    and running statistics."""
    _need_gpu()
    from change3d_amd import ops
    dtype = torch.bfloat16
    dt = ops.dt_code(dtype)
    Cp, Np = ops.cpad(Cin), ops.cpad(Cinner)
    c = padc(q(rnd((M, Cin), 100), dtype), Cp).to(DEV, dtype).contiguous()
    s = padc(q(rnd((M, Cin), 101), dtype), Cp).to(DEV, dtype).contiguous()
    w = rnd((Cinner, Cin), 102, 0.2).to(DEV).contiguous()
    g_ = torch.Generator().manual_seed(103)
    sums = torch.zeros(16, 2, Cin, dtype=torch.float64)
    sums[:, 0] = torch.randn(16, Cin, generator=g_, dtype=torch.float64) * M / 64
    sums[:, 1] = (torch.rand(16, Cin, generator=g_, dtype=torch.float64) + 0.5) * M / 8
    sums = sums.to(DEV)

    def bn():
        m = torch.nn.BatchNorm3d(Cin)
        with torch.no_grad():
            m.weight.copy_(rnd((Cin,), 104).abs() + 0.5); m.bias.copy_(rnd((Cin,), 105, 0.3))
        return m.to(DEV)

    outs = []
    for fused in (False, True):
        m = bn()
        ss, mr = torch.full((2 * Cp,), float("nan"), device=DEV), torch.full((2 * Cp,), float("nan"), device=DEV)
        y = torch.full((M, Cp), float("nan"), dtype=dtype, device=DEV)
        a = torch.full((M, Np), float("nan"), dtype=dtype, device=DEV)
        st = torch.zeros(16 * 2 * Cinner, dtype=torch.float64, device=DEV)
        fin = ops.fin_consume(sums, m, float(M), ss, mr)
        if fused:
            ops.pw_gemm(c, w, a, M=M, K=Cin, N=Cinner, w_sn=Cin, w_sk=1, dtype=dt, x2=s, pro_mode=ops.PRO_AFFINE2, pro_p=ss,
                        epi_mode=ops.EPI_STATS, stats=st, fin=fin, pro_out=y)
        else:
            ops.block_out_fwd_fin(c, fin, s, None, 1, y, M, Cin, dt)
            ops.pw_gemm(y, w, a, M=M, K=Cin, N=Cinner, w_sn=Cin, w_sk=1, dtype=dt, epi_mode=ops.EPI_STATS, stats=st)
        torch.cuda.synchronize()
        outs.append((y, a, st, ss, mr, m.running_mean.clone(), m.running_var.clone(), m.num_batches_tracked.clone()))
    for i, (x0, x1) in enumerate(zip(*outs)):
        assert torch.equal(x0, x1), i
    assert torch.isfinite(outs[1][1].float()).all() and outs[1][0].float().abs().max() > 0 and int(outs[1][7]) == 1


# --------------------------------------------------------------------------- packed weight images
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("K,N,transposed", [(24, 54, False), (54, 24, True), (96, 216, False), (216, 96, True),
                                            (48, 108, True), (108, 48, False), (192, 192, False), (24, 24, True),
                                            (12, 20, False)])
def test_pw_gemm_with_packed_weight_image_is_bit_identical(dtype, K, N, transposed):
    """`c3d_pw_args.w_img` (LDS image written once by c3d_pw_pack_weights, copied by LDS-DMA) against the path
    where every workgroup converts the f32 weights itself: same bytes out, both weight orientations (forward:
    w[n*K + k]; data gradient: w[k*N + n]), ragged row counts, channel counts that need padding."""
    _need_gpu()
    from change3d_amd import ops
    M = 16 * 53 + 7
    Kp, Np = ops.cpad(K), ops.cpad(N)
    dt = ops.dt_code(dtype)
    x = padc(q(rnd((M, K), 31), dtype), Kp).to(DEV, dtype).contiguous()
    if transposed:
        w = rnd((K, N), 32, 0.2).to(DEV)      # conv weight [out = K][in = N] read as W^T
        sn, sk = 1, N
    else:
        w = rnd((N, K), 32, 0.2).to(DEV)
        sn, sk = K, 1
    nbytes = ops.pw_weight_image_bytes(N, K, dt)
    assert nbytes > 0 and nbytes % 16 == 0
    img = torch.full((nbytes + 64,), 0x7F, dtype=torch.uint8, device=DEV)   # +64: the pack kernel must stay inside
    ops.pw_pack_weights([(w, img, N, K, sn, sk)], dt)
    torch.cuda.synchronize()
    assert (img[nbytes:] == 0x7F).all(), "pack kernel wrote past the image"
    outs = []
    for wi in (None, img):
        y = torch.full((M, Np), float("nan"), dtype=dtype, device=DEV)
        stats = torch.zeros(ops.STAT_STRIPES * 2 * N, dtype=torch.float64, device=DEV)
        ops.pw_gemm(x, w, y, M=M, K=K, N=N, w_sn=sn, w_sk=sk, dtype=dt, epi_mode=ops.EPI_STATS, stats=stats, w_img=wi)
        torch.cuda.synchronize()
        outs.append((y.clone(), stats.view(ops.STAT_STRIPES, -1).sum(0).clone()))
    assert torch.equal(outs[0][0].view(torch.uint8), outs[1][0].view(torch.uint8)), "output differs with the weight image"
    assert torch.allclose(outs[0][1], outs[1][1], rtol=1e-12, atol=1e-9)
    ref = x[:, :K].float().cpu() @ (w.cpu() if transposed else w.cpu().t())
    close(outs[1][0][:, :N], ref, dtype, "y", scale=ref.abs().max().item())


def test_pw_pack_weights_many_images_in_one_call():
    """More images than one launch carries (C3D_PW_PACK_MAX = 64): each image equals its single-image packing."""
    _need_gpu()
    from change3d_amd import ops
    dt = ops.dt_code(torch.bfloat16)
    shapes = [(24 + 8 * (i % 5), 216 - 8 * (i % 7)) for i in range(70)]
    ws = [rnd((n, k), 100 + i, 0.3).to(DEV) for i, (n, k) in enumerate(shapes)]
    sizes = [ops.pw_weight_image_bytes(n, k, dt) for n, k in shapes]
    together = [torch.zeros(s, dtype=torch.uint8, device=DEV) for s in sizes]
    ops.pw_pack_weights([(w, im, n, k, k, 1) for w, im, (n, k) in zip(ws, together, shapes)], dt)
    for i in (0, 1, 33, 63, 64, 69):
        alone = torch.zeros(sizes[i], dtype=torch.uint8, device=DEV)
        ops.pw_pack_weights([(ws[i], alone, shapes[i][0], shapes[i][1], shapes[i][1], 1)], dt)
        torch.cuda.synchronize()
        assert torch.equal(alone, together[i]), f"image {i}"
    assert ops.pw_weight_image_bytes(432, 192, dt) == 0      # wide shapes have no image (block-tiled kernel)


# ----------------------------------------------------- round 3: BatchNorm_b of blocks without SqueezeExcitation, consumer side
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,C", [(5, 54), (32, 216), (3, 108)])
def test_bn_b_finalize_folded_into_conv_c_and_fused_depthwise_backward_is_bit_identical(dtype, B, C):
    """Blocks without SE: (a) c3d_pw_gemm's BN_SE_SWISH prologue rebuilding BatchNorm_b's scale / shift from the depthwise
    kernel's per-sample sums (fin.batch) against c3d_bn_se_finalize + the plain call; (b) c3d_dw333_bwd_fused_fin rebuilding
    A | B | C from the Swish-backward epilogue's per-sample sums against c3d_se_bn_bwd_coef + c3d_dw333_bwd_fused:
    outputs, statistics, saved vectors, running statistics and d gamma / d beta are BIT-identical (csrc/bn_fin.h)."""
    _need_gpu()
    from change3d_amd import ops
    T, H, W, N = 3, 16, 24, 48
    Cp, Np = ops.cpad(C), ops.cpad(N)
    dt = ops.dt_code(dtype)
    rps = T * H * W
    M = B * rps
    bt = padc(q(rnd((M, C), 300), dtype), Cp).to(DEV, dtype).contiguous()
    nc = torch.zeros(B, Cp, 2, dtype=torch.float64, device=DEV)
    bq = bt.float().double().view(B, rps, Cp)
    nc[:, :, 0], nc[:, :, 1] = bq.sum(1), (bq * bq).sum(1)
    w = rnd((N, C), 301, 0.2).to(DEV).contiguous()

    def bn_module(seed):
        m = torch.nn.BatchNorm3d(C).to(DEV)
        with torch.no_grad():
            m.weight.copy_(rnd((C,), seed).abs() + 0.5); m.bias.copy_(rnd((C,), seed + 1, 0.3))
            m.running_mean.copy_(rnd((C,), seed + 2, 0.2)); m.running_var.copy_(rnd((C,), seed + 3).abs() + 0.5)
        return m

    outs = []
    for folded in (False, True):
        m = bn_module(310)
        ss, mr = torch.zeros(2 * Cp, device=DEV), torch.zeros(2 * Cp, device=DEV)
        y = torch.full((M, Np), float("nan"), dtype=dtype, device=DEV)
        stats = torch.zeros(ops.STAT_STRIPES * 2 * N, dtype=torch.float64, device=DEV)
        kw = dict(M=M, K=C, N=N, w_sn=C, w_sk=1, dtype=dt, pro_mode=ops.PRO_BN_SE_SWISH, rows_per_sample=rps,
                  epi_mode=ops.EPI_STATS, stats=stats)
        if folded:
            ops.pw_gemm(bt, w, y, pro_p=ss, fin=ops.fin_consume(nc, m, float(M), ss, mr, batch=B), **kw)
        else:
            ops.bn_se_finalize(nc.view(-1), B, rps, m, None, C, ss, mr, None, None, True)
            ops.pw_gemm(bt, w, y, pro_p=ss, **kw)
        torch.cuda.synchronize()
        outs.append(dict(y=y, stats=stats, ss=ss, mr=mr, rm=m.running_mean.clone(), rv=m.running_var.clone(),
                         nbt=m.num_batches_tracked.clone()))
    for k in outs[0]:
        assert torch.equal(outs[0][k], outs[1][k]), f"forward: {k} differs"
    assert torch.isfinite(outs[1]["y"].float()).all() and int(outs[1]["nbt"]) == 1
    ss_b, mr_b = outs[0]["ss"], outs[0]["mr"]

    # ---- backward
    Ho, Wo = H, W
    a = padc(q(rnd((B, T, H, W, C), 320), dtype), Cp).to(DEV, dtype).contiguous()
    b5 = bt.view(B, T, Ho, Wo, Cp)
    t1 = padc(q(rnd((B, T, Ho, Wo, C), 321), dtype), Cp).to(DEV, dtype).contiguous()
    nc3 = torch.zeros(B, Cp, 3, dtype=torch.float64, device=DEV)
    nc3[:, :C] = rnd((B, C, 3), 322).double().to(DEV) * 50.0
    wd = rnd((C, 1, 3, 3, 3), 323, 0.3).to(DEV).contiguous()
    ssa = torch.cat([padc(rnd((C,), 324).abs() + 0.5, Cp), padc(rnd((C,), 325, 0.3), Cp)]).to(DEV)
    mra = torch.cat([padc(rnd((C,), 326, 0.5), Cp), padc(rnd((C,), 327).abs() + 0.5, Cp)]).to(DEV)
    res = []
    for folded in (False, True):
        m = bn_module(310)
        t2 = torch.full_like(a, float("nan"))
        dsums = torch.zeros(2 * C, dtype=torch.float64, device=DEV)
        dw = torch.zeros((C, 27), dtype=torch.float32, device=DEV)
        if folded:
            ops.dw_bwd_fused_fin(t1, b5, ops.fin_b_bwd(nc3, B, m, float(M), mr_b), wd, a, ssa, mra, t2, dsums, dw, B, T, H, W, C, dt)
        else:
            cA, cC, cB = torch.zeros(Cp, device=DEV), torch.zeros(Cp, device=DEV), torch.zeros(B * Cp, device=DEV)
            ops.se_bn_bwd_coef(nc3.view(-1), nc.view(-1), B, rps, m, mr_b, ss_b, None, None, None, C, cA, cC, cB)
            ops.dw_bwd_fused(t1, b5, cA, cB, cC, wd, a, ssa, mra, t2, dsums, dw, B, T, H, W, C, dt)
        torch.cuda.synchronize()
        res.append(dict(t2=t2, dsums=dsums, dgamma=m.weight.grad.clone(), dbeta=m.bias.grad.clone(), dw=dw))
    for k in ("t2", "dsums", "dgamma", "dbeta"):
        assert torch.equal(res[0][k], res[1][k]), f"backward: {k} differs"
    assert torch.isfinite(res[1]["t2"].float()).all() and float(res[1]["dgamma"].abs().max()) > 0
    close(res[1]["dw"], res[0]["dw"], dtype, "dw (f32 atomics)", scale=res[0]["dw"].abs().max().item())


@pytest.mark.parametrize("B,C", [(5, 54), (3, 108)])
def test_bn_b_backward_coefficients_rebuilt_by_every_bf16_depthwise_backward_kernel(B, C):
    """The folded BatchNorm_b coefficient rebuild (fin.sums) is part of the parameter staging that the register-prefetch and the
    LDS-DMA ring kernels share; in bf16 only the ring kernel of the default option ran it under a test.  c3d_dw333_bwd_fused_fin
    under C3D_OPT_DW_RING = 0 (register prefetch), 9 (ring, requests in a burst) and 13 (ring, requests spread): t2, the
    BatchNorm_a sums, d gamma and d beta are bit-equal across the three kernels and to c3d_se_bn_bwd_coef +
    c3d_dw333_bwd_fused; the weight gradient (f32 atomics) as in the test above."""
    _need_gpu()
    from change3d_amd import ops
    dtype = torch.bfloat16
    T, H, W = 3, 16, 24
    Cp = ops.cpad(C)
    dt = ops.dt_code(dtype)
    rps = T * H * W
    M = B * rps
    bt = padc(q(rnd((M, C), 300), dtype), Cp).to(DEV, dtype).contiguous()
    nc = torch.zeros(B, Cp, 2, dtype=torch.float64, device=DEV)
    bq = bt.float().double().view(B, rps, Cp)
    nc[:, :, 0], nc[:, :, 1] = bq.sum(1), (bq * bq).sum(1)

    def bn_module():
        m = torch.nn.BatchNorm3d(C).to(DEV)
        with torch.no_grad():
            m.weight.copy_(rnd((C,), 310).abs() + 0.5); m.bias.copy_(rnd((C,), 311, 0.3))
            m.running_mean.copy_(rnd((C,), 312, 0.2)); m.running_var.copy_(rnd((C,), 313).abs() + 0.5)
        return m

    ss_b, mr_b = torch.zeros(2 * Cp, device=DEV), torch.zeros(2 * Cp, device=DEV)
    ops.bn_se_finalize(nc.view(-1), B, rps, bn_module(), None, C, ss_b, mr_b, None, None, True)
    a = padc(q(rnd((B, T, H, W, C), 320), dtype), Cp).to(DEV, dtype).contiguous()
    b5 = bt.view(B, T, H, W, Cp)
    t1 = padc(q(rnd((B, T, H, W, C), 321), dtype), Cp).to(DEV, dtype).contiguous()
    nc3 = torch.zeros(B, Cp, 3, dtype=torch.float64, device=DEV)
    nc3[:, :C] = rnd((B, C, 3), 322).double().to(DEV) * 50.0
    wd = rnd((C, 1, 3, 3, 3), 323, 0.3).to(DEV).contiguous()
    ssa = torch.cat([padc(rnd((C,), 324).abs() + 0.5, Cp), padc(rnd((C,), 325, 0.3), Cp)]).to(DEV)
    mra = torch.cat([padc(rnd((C,), 326, 0.5), Cp), padc(rnd((C,), 327).abs() + 0.5, Cp)]).to(DEV)
    res, names = {}, {}
    try:
        for leg in ("unfolded", 0, 9, 13):
            ops.set_option(ops.OPT_DW_RING, 13 if leg == "unfolded" else leg)
            m = bn_module()
            t2 = torch.full_like(a, float("nan"))
            dsums = torch.zeros(2 * C, dtype=torch.float64, device=DEV)
            dw = torch.zeros((C, 27), dtype=torch.float32, device=DEV)
            if leg == "unfolded":
                cA, cC, cB = torch.zeros(Cp, device=DEV), torch.zeros(Cp, device=DEV), torch.zeros(B * Cp, device=DEV)
                ops.se_bn_bwd_coef(nc3.view(-1), nc.view(-1), B, rps, m, mr_b, ss_b, None, None, None, C, cA, cC, cB)
                ops.dw_bwd_fused(t1, b5, cA, cB, cC, wd, a, ssa, mra, t2, dsums, dw, B, T, H, W, C, dt)
            else:
                ops.dw_bwd_fused_fin(t1, b5, ops.fin_b_bwd(nc3, B, m, float(M), mr_b), wd, a, ssa, mra, t2, dsums, dw, B, T, H, W, C, dt)
            names[leg] = ops.last_kernel()
            torch.cuda.synchronize()
            res[leg] = dict(t2=t2, dsums=dsums, dgamma=m.weight.grad.clone(), dbeta=m.bias.grad.clone(), dw=dw)
    finally:
        ops.set_option(ops.OPT_DW_RING, 13)
    assert names[0] == "dw_bwd_fused_kernel<unsigned short, 3, 1>", names
    assert names[9] == "dw_bwd_ring_kernel<3, false>" and names[13] == "dw_bwd_ring_kernel<3, true>", names
    assert names["unfolded"] == names[13], names
    ref = res["unfolded"]
    assert torch.isfinite(ref["t2"].float()).all() and float(ref["dgamma"].abs().max()) > 0
    for leg in (0, 9, 13):
        for k in ("t2", "dsums", "dgamma", "dbeta"):
            assert torch.equal(ref[k], res[leg][k]), f"OPT_DW_RING {leg}: {k} differs"
        close(res[leg]["dw"], ref["dw"], dtype, f"dw (f32 atomics), OPT_DW_RING {leg}", scale=ref["dw"].abs().max().item())


def test_block_out_bwd_refuses_misaligned_parameter_vectors():
    """c3d_block_out_bwd reads the mean | rstd rows as 16-byte vectors (one round trip instead of eight dependent ones, round 5):
    a misaligned `mr_c` is an argument error, not a fault."""
    _need_gpu()
    from change3d_amd import ops
    from change3d_amd._lib import Change3DHipError
    M, C = 64, 24
    Cp = ops.cpad(C)
    dy = torch.zeros(M, Cp, dtype=torch.bfloat16, device=DEV)
    y, c, g = torch.ones_like(dy), torch.zeros_like(dy), torch.zeros_like(dy)
    mr = torch.zeros(2 * Cp + 1, dtype=torch.float32, device=DEV)
    ds = torch.zeros(2 * C, dtype=torch.float64, device=DEV)
    ops.block_out_bwd(dy, y, c, None, g, mr[:2 * Cp], None, ds, None, M, C, ops.dt_code(torch.bfloat16))   # aligned: fine
    with pytest.raises(Change3DHipError):
        ops.block_out_bwd(dy, y, c, None, g, mr[1:], None, ds, None, M, C, ops.dt_code(torch.bfloat16))
    torch.cuda.synchronize()


def test_pw_gemm_refuses_an_operand_of_two_gib():
    """The tile loop addresses rows with 32-bit byte offsets into bounds-checked buffer resources whose origin is row 0 (offset
    2^31 = "nowhere"): a call whose largest operand reaches 2 GiB is refused with C3D_E_UNSUPPORTED, not run (per-wave origins
    would lift the limit and were measured: +1.1 .. +1.6 % on the B=32 step).  B <= 96 per GPU at
    256 x 256 in bf16 stays under it."""
    _need_gpu()
    from change3d_amd import ops
    from change3d_amd._lib import Change3DHipError
    K, N = 56, 24
    M = (1 << 31) // (K * 2) + 16
    x = torch.zeros((M, K), dtype=torch.bfloat16, device=DEV)
    y = torch.zeros((M, ops.cpad(N)), dtype=torch.bfloat16, device=DEV)
    w = rnd((N, K), 2, 0.2).to(DEV)
    with pytest.raises(Change3DHipError):
        ops.pw_gemm(x, w, y, M=M, K=K, N=N, w_sn=K, w_sk=1, dtype=ops.dt_code(torch.bfloat16))
    M2 = (1 << 31) // (K * 2) - 16        # just under: runs, and the last (ragged) rows are right
    x[M2 - 40:M2] = torch.randn((40, K), device=DEV).to(torch.bfloat16)
    ops.pw_gemm(x, w, y, M=M2, K=K, N=N, w_sn=K, w_sk=1, dtype=ops.dt_code(torch.bfloat16))
    torch.cuda.synchronize()
    ref = x[M2 - 40:M2].float() @ w.t()
    got = y[M2 - 40:M2, :N].float()
    assert (got - ref).abs().max().item() <= 2e-2 * max(1.0, ref.abs().max().item())
    del x, y
    torch.cuda.empty_cache()
