"""GPU op tests of the pointwise data gradient WITH the weight gradient fused in (`c3d_pw_args.wg_mode`, round 4;
reference model/x3d.py:173-175,214-216: autograd's convolution_backward yields both gradients of a 1x1x1 convolution).

The fused launch must (a) leave the data gradient and its statistics BIT-identical to the unfused launch, (b) reproduce the
weight gradient of the separate `c3d_pw_wgrad` kernel (same bf16 operands, f32 accumulation in another order) and of a
torch-CPU f64 computation of the same contraction.
"""
import pytest
import torch

from test_ops_gpu import DEV, _need_gpu, padc, q, rnd

pytestmark = pytest.mark.gpu
DT = torch.bfloat16


def _rel(a, b):
    return ((a.double().cpu() - b.double().cpu()).abs().max() / b.double().abs().max()).item()


# conv_c of a res2 / res3 block: data gradient rows [M][Co] -> [M][Ci], Swish / SE backward in the epilogue
@pytest.mark.parametrize("Co,Ci,rows", [(24, 54, 16 * 13), (48, 108, 16 * 9), (24, 54, 16 * 120), (48, 108, 16 * 64)])
@pytest.mark.parametrize("ragged", [0, 5])
def test_conv_c_data_gradient_with_fused_weight_gradient(Co, Ci, rows, ragged):
    _need_gpu()
    from change3d_amd import ops
    B = 3
    M = B * rows - ragged
    dt = ops.dt_code(DT)
    Cop, Cip = ops.cpad(Co), ops.cpad(Ci)
    g, c = q(rnd((M, Co), 1), DT), q(rnd((M, Co), 2), DT)
    A, Bc, Cc = rnd((Co,), 3), rnd((Co,), 4, 0.1), rnd((Co,), 5, 0.1)
    w = rnd((Co, Ci), 6, 0.2)                                   # conv_c weight [out][in]; the data gradient reads it transposed
    b = q(rnd((M, Ci), 7), DT)
    scale, shift = rnd((Ci,), 8).abs() + 0.5, rnd((Ci,), 9, 0.3)
    gate = torch.sigmoid(rnd((B, Ci), 10))
    mean, rstd = rnd((Ci,), 11, 0.5), rnd((Ci,), 12).abs() + 0.5
    gd, cd = (padc(t, Cop).to(DEV, DT).contiguous() for t in (g, c))
    bd = padc(b, Cip).to(DEV, DT).contiguous()
    coef = torch.cat([padc(A, Cop), padc(Bc, Cop), padc(Cc, Cop)]).to(DEV)
    ss = torch.cat([padc(scale, Cip), padc(shift, Cip)]).to(DEV)
    mr = torch.cat([padc(mean, Cip), padc(rstd, Cip)]).to(DEV)
    gt = padc(gate, Cip).to(DEV).contiguous()
    wd = w.to(DEV)

    def run(fused):
        t1 = torch.full((M, Cip), float("nan"), dtype=DT, device=DEV)
        nc3 = torch.zeros(B * Cip * 3, dtype=torch.float64, device=DEV)
        dw = torch.ones((Co, Ci), dtype=torch.float32, device=DEV)        # accumulate semantics: += onto ones
        kw = dict(wg_mode=ops.WG_SWISH, wg_dw=dw) if fused else {}
        ops.pw_gemm(gd, wd, t1, M=M, K=Co, N=Ci, w_sn=1, w_sk=Ci, dtype=dt, x2=cd, pro_mode=ops.PRO_AFFINE2, pro_p=coef,
                    epi_mode=ops.EPI_SWISH_SE_BWD, e1=bd, epi_p=ss, epi_gate=gt, epi_q=mr, stats=nc3, rows_per_sample=rows, **kw)
        torch.cuda.synchronize()
        return t1, nc3, dw

    t1_a, nc_a, _ = run(False)
    t1_b, nc_b, dw = run(True)
    assert torch.equal(t1_a.view(torch.int16), t1_b.view(torch.int16)), "the data gradient must not change"
    # (the fused variant prefetches fewer tiles per iteration: another tile -> wave partition, i.e. another grouping of the
    # per-wave f32 partial sums behind the f64 per-sample statistics)
    assert torch.allclose(nc_a, nc_b, rtol=2e-5, atol=1e-5 * nc_a.abs().max().item())
    dw_sep = torch.ones((Co, Ci), dtype=torch.float32, device=DEV)
    ops.pw_wgrad(gd, bd, dw_sep, M=M, K=Ci, N=Co, dw_sn=Ci, dw_sk=1, dtype=dt, p2=cd, p_coef=coef, q_mode=ops.PRO_BN_SE_SWISH,
                 q_ss=ss, q_gate=gt, rows_per_sample=rows)
    torch.cuda.synchronize()
    assert _rel(dw, dw_sep) < 2e-5, _rel(dw, dw_sep)            # same bf16 operands, f32 sums in another order
    P = q(A * g + Bc + Cc * c, DT).double()
    v = (b * scale + shift) * gate.repeat_interleave(rows, 0)[:M]
    Q = q(v * torch.sigmoid(v), DT).double()
    ref = (P.t() @ Q + 1.0).float()
    assert _rel(dw, ref) < 3e-3, _rel(dw, ref)                  # (the device rounds P, Q once more than this reference does)


# conv_a of a res2 / res3 block: data gradient rows [M][Ci] -> [M][Cin] + residual gradient, Q = the layer's forward input
@pytest.mark.parametrize("Ci,Cin,M", [(54, 24, 16 * 37), (108, 48, 16 * 29), (54, 24, 16 * 400 - 3), (108, 48, 16 * 300 - 9)])
@pytest.mark.parametrize("res_mode", [0, 1])
def test_conv_a_data_gradient_with_fused_weight_gradient(Ci, Cin, M, res_mode):
    _need_gpu()
    from change3d_amd import ops
    dt = ops.dt_code(DT)
    H = W = 0
    if res_mode == 1:      # first block of a stage: the shortcut's gradient lives at half resolution
        BT, H, W = 2, 8, 12
        M = BT * H * W
    Cip, Cinp = ops.cpad(Ci), ops.cpad(Cin)
    t2, a_ = q(rnd((M, Ci), 21), DT), q(rnd((M, Ci), 22), DT)
    A, Bc, Cc = rnd((Ci,), 23), rnd((Ci,), 24, 0.1), rnd((Ci,), 25, 0.1)
    w = rnd((Ci, Cin), 26, 0.2)                                 # conv_a weight [out][in]
    xin = q(rnd((M, Cin), 27), DT)
    res = q(rnd((M if res_mode == 0 else M // 4, Cin), 28), DT)
    t2d, ad = (padc(t, Cip).to(DEV, DT).contiguous() for t in (t2, a_))
    xd, rd = (padc(t, Cinp).to(DEV, DT).contiguous() for t in (xin, res))
    coef = torch.cat([padc(A, Cip), padc(Bc, Cip), padc(Cc, Cip)]).to(DEV)
    wd = w.to(DEV)

    def run(fused):
        dx = torch.full((M, Cinp), float("nan"), dtype=DT, device=DEV)
        dw = torch.ones((Ci, Cin), dtype=torch.float32, device=DEV)
        kw = dict(wg_mode=ops.WG_ROWS, wg_dw=dw, wg_x3=xd) if fused else {}
        ops.pw_gemm(t2d, wd, dx, M=M, K=Ci, N=Cin, w_sn=1, w_sk=Cin, dtype=dt, x2=ad, pro_mode=ops.PRO_AFFINE2, pro_p=coef,
                    epi_mode=ops.EPI_ADD, e1=rd, res_mode=res_mode, H=H, W=W, **kw)
        torch.cuda.synchronize()
        return dx, dw

    dx_a, _ = run(False)
    dx_b, dw = run(True)
    assert torch.equal(dx_a.view(torch.int16), dx_b.view(torch.int16)), "the data gradient must not change"
    # the same launches reading the packed weight image (c3d_pw_pack_weights): N = 48 runs the fused kernel on THREE output
    # tiles of an image packed for the four-tile bucket -- the kernel copies the first 48 rows of every k-chunk
    img = torch.zeros(ops.pw_weight_image_bytes(Cin, Ci, dt), dtype=torch.uint8, device=DEV)
    ops.pw_pack_weights([(wd, img, Cin, Ci, 1, Cin)], dt)
    for fused in (False, True):
        dx_i = torch.full((M, Cinp), float("nan"), dtype=DT, device=DEV)
        dw_i = torch.ones((Ci, Cin), dtype=torch.float32, device=DEV)
        kw = dict(wg_mode=ops.WG_ROWS, wg_dw=dw_i, wg_x3=xd) if fused else {}
        ops.pw_gemm(t2d, wd, dx_i, M=M, K=Ci, N=Cin, w_sn=1, w_sk=Cin, dtype=dt, x2=ad, pro_mode=ops.PRO_AFFINE2, pro_p=coef,
                    epi_mode=ops.EPI_ADD, e1=rd, res_mode=res_mode, H=H, W=W, w_img=img, **kw)
        torch.cuda.synchronize()
        assert torch.equal(dx_a.view(torch.int16), dx_i.view(torch.int16)), ("weight image", fused)
    dw_sep = torch.ones((Ci, Cin), dtype=torch.float32, device=DEV)
    ops.pw_wgrad(t2d, xd, dw_sep, M=M, K=Cin, N=Ci, dw_sn=Cin, dw_sk=1, dtype=dt, p2=ad, p_coef=coef)
    torch.cuda.synchronize()
    assert _rel(dw, dw_sep) < 2e-5, _rel(dw, dw_sep)
    P = q(A * t2 + Bc + Cc * a_, DT).double()
    ref = (P.t() @ xin.double() + 1.0).float()
    assert _rel(dw, ref) < 2e-5, _rel(dw, ref)
    # wg_mask_out: the stored data gradient carries the ReLU mask of the previous block's output (= wg_x3), i.e. it IS the
    # g = dy * (y > 0) of c3d_block_out_bwd, whose statistics-only form (y = g = NULL) then gives the same sums
    xin_relu = torch.relu(xin)
    xrd = padc(xin_relu, Cinp).to(DEV, DT).contiguous()
    dx_m = torch.full((M, Cinp), float("nan"), dtype=DT, device=DEV)
    dw_m = torch.zeros((Ci, Cin), dtype=torch.float32, device=DEV)
    ops.pw_gemm(t2d, wd, dx_m, M=M, K=Ci, N=Cin, w_sn=1, w_sk=Cin, dtype=dt, x2=ad, pro_mode=ops.PRO_AFFINE2, pro_p=coef,
                epi_mode=ops.EPI_ADD, e1=rd, res_mode=res_mode, H=H, W=W, wg_mode=ops.WG_ROWS, wg_dw=dw_m, wg_x3=xrd, wg_mask_out=1)
    torch.cuda.synchronize()
    want = torch.where(xrd > 0, dx_a, torch.zeros_like(dx_a))
    assert torch.equal(dx_m.view(torch.int16), want.view(torch.int16))
    cten = q(rnd((M, Cin), 29), DT)
    cd_ = padc(cten, Cinp).to(DEV, DT).contiguous()
    mr = torch.cat([padc(rnd((Cin,), 30, 0.5), Cinp), padc(rnd((Cin,), 31).abs() + 0.5, Cinp)]).to(DEV)
    s_full = torch.zeros(2 * Cin, dtype=torch.float64, device=DEV)
    g_full = torch.empty_like(dx_a)
    ops.block_out_bwd(dx_a, xrd, cd_, None, g_full, mr, None, s_full, None, M, Cin, dt)
    s_pre = torch.zeros(2 * Cin, dtype=torch.float64, device=DEV)
    ops.block_out_bwd(dx_m, None, cd_, None, None, mr, None, s_pre, None, M, Cin, dt)
    torch.cuda.synchronize()
    assert torch.equal(g_full.view(torch.int16), dx_m.view(torch.int16))
    assert torch.allclose(s_full, s_pre, rtol=1e-12, atol=0)
    # add_sums: the same launch also takes those sums (c3d_block_out_bwd is not launched at all); f32 partial sums per lane
    # and wave, f64 across workgroups: the sums of the separate pass to ~1e-6 of their scale
    if res_mode == 0:
        dx_s = torch.full((M, Cinp), float("nan"), dtype=DT, device=DEV)
        dw_s = torch.zeros((Ci, Cin), dtype=torch.float32, device=DEV)
        s_fold = torch.zeros(2 * Cin, dtype=torch.float64, device=DEV)
        ops.pw_gemm(t2d, wd, dx_s, M=M, K=Ci, N=Cin, w_sn=1, w_sk=Cin, dtype=dt, x2=ad, pro_mode=ops.PRO_AFFINE2, pro_p=coef,
                    epi_mode=ops.EPI_ADD, e1=rd, wg_mode=ops.WG_ROWS, wg_dw=dw_s, wg_x3=xrd, wg_mask_out=1,
                    add_c=cd_, add_mr=mr, add_sums=s_fold)
        torch.cuda.synchronize()
        assert torch.equal(dx_s.view(torch.int16), dx_m.view(torch.int16))
        assert torch.equal(dw_s, dw_m)
        scale = s_full.abs().max().item()
        assert (s_fold - s_full).abs().max().item() < 2e-6 * scale + 1e-4, ((s_fold - s_full).abs().max().item(), scale)


def test_fused_weight_gradient_refuses_shapes_it_does_not_take():
    _need_gpu()
    from change3d_amd import ops
    M, Ci, Cin = 64, 216, 96                                     # res4: the accumulator image does not fit beside the tiles
    z = lambda *s: torch.zeros(*s, dtype=DT, device=DEV)  # noqa: E731
    from change3d_amd._lib import Change3DHipError
    with pytest.raises(Change3DHipError):
        ops.pw_gemm(z(M, Ci), torch.zeros(Ci, Cin, device=DEV), z(M, Cin), M=M, K=Ci, N=Cin, w_sn=1, w_sk=Cin,
                    dtype=ops.dt_code(DT), x2=z(M, Ci), pro_mode=ops.PRO_AFFINE2, pro_p=torch.zeros(3 * Ci, device=DEV),
                    epi_mode=ops.EPI_ADD, e1=z(M, Cin), wg_mode=ops.WG_ROWS, wg_x3=z(M, Cin),
                    wg_dw=torch.zeros(Ci, Cin, device=DEV))


@pytest.mark.gpu
@pytest.mark.parametrize("M,Ci,Cin", [(98304 // 8, 216, 96), (1000, 216, 96), (777, 120, 80), (50, 216, 112)])
def test_block_out_bwd_folded_into_the_conv_a_data_gradient(M, Ci, Cin):
    """C3D_WG_MASKSUM (no weight gradient; res4's conv_a data gradient): the stored output is g = (dx + residual) * (y > 0)
    of the PREVIOUS block and the launch accumulates that block's BatchNorm_c-backward sums -- what the pair
    (c3d_pw_gemm EPI_ADD, c3d_block_out_bwd) produces (reference model/x3d.py:229-236 backward)."""
    _need_gpu()
    from change3d_amd import ops
    dt = ops.dt_code(DT)
    Cip, Cinp = ops.cpad(Ci), ops.cpad(Cin)
    t2, a_ = q(rnd((M, Ci), 41), DT), q(rnd((M, Ci), 42), DT)
    A, Bc, Cc = rnd((Ci,), 43), rnd((Ci,), 44, 0.1), rnd((Ci,), 45, 0.1)
    w = rnd((Ci, Cin), 46, 0.2)
    y_prev = torch.relu(q(rnd((M, Cin), 47), DT))
    res = q(rnd((M, Cin), 48), DT)
    cten = q(rnd((M, Cin), 49), DT)
    t2d, ad = (padc(t, Cip).to(DEV, DT).contiguous() for t in (t2, a_))
    yd, rd, cd_ = (padc(t, Cinp).to(DEV, DT).contiguous() for t in (y_prev, res, cten))
    coef = torch.cat([padc(A, Cip), padc(Bc, Cip), padc(Cc, Cip)]).to(DEV)
    mr = torch.cat([padc(rnd((Cin,), 50, 0.5), Cinp), padc(rnd((Cin,), 51).abs() + 0.5, Cinp)]).to(DEV)
    wd = w.to(DEV)
    dx = torch.full((M, Cinp), float("nan"), dtype=DT, device=DEV)
    ops.pw_gemm(t2d, wd, dx, M=M, K=Ci, N=Cin, w_sn=1, w_sk=Cin, dtype=dt, x2=ad, pro_mode=ops.PRO_AFFINE2, pro_p=coef,
                epi_mode=ops.EPI_ADD, e1=rd)
    g_ref = torch.empty_like(dx)
    s_ref = torch.zeros(2 * Cin, dtype=torch.float64, device=DEV)
    ops.block_out_bwd(dx, yd, cd_, None, g_ref, mr, None, s_ref, None, M, Cin, dt)
    g = torch.full((M, Cinp), float("nan"), dtype=DT, device=DEV)
    s = torch.zeros(2 * Cin, dtype=torch.float64, device=DEV)
    ops.pw_gemm(t2d, wd, g, M=M, K=Ci, N=Cin, w_sn=1, w_sk=Cin, dtype=dt, x2=ad, pro_mode=ops.PRO_AFFINE2, pro_p=coef,
                epi_mode=ops.EPI_ADD, e1=rd, wg_mode=ops.WG_MASKSUM, wg_x3=yd, add_c=cd_, add_mr=mr, add_sums=s)
    torch.cuda.synchronize()
    assert torch.equal(g.view(torch.int16), g_ref.view(torch.int16))
    scale = s_ref.abs().max().item()
    assert (s - s_ref).abs().max().item() < 2e-6 * scale + 1e-4, ((s - s_ref).abs().max().item(), scale)
    # and against plain arithmetic (f64 over the stored g)
    gq = g_ref[:, :Cin].double().cpu()
    chat = (cten.double() - mr[:Cin].double().cpu()) * mr[Cinp:Cinp + Cin].double().cpu()
    want = torch.cat([gq.sum(0), (gq * chat).sum(0)])
    assert (s.cpu() - want).abs().max().item() < 2e-6 * scale + 1e-4


@pytest.mark.gpu
def test_masksum_refuses_what_it_does_not_take():
    _need_gpu()
    from change3d_amd import ops
    from change3d_amd._lib import Change3DHipError
    z = lambda *s: torch.zeros(*s, dtype=DT, device=DEV)  # noqa: E731
    M, Ci, Cin = 64, 216, 96
    kw = dict(M=M, K=Ci, N=Cin, w_sn=1, w_sk=Cin, dtype=ops.dt_code(DT), x2=z(M, Ci), pro_mode=ops.PRO_AFFINE2,
              pro_p=torch.zeros(3 * Ci, device=DEV), epi_mode=ops.EPI_ADD, e1=z(M, Cin))
    sums = torch.zeros(2 * Cin, dtype=torch.float64, device=DEV)
    mr = torch.zeros(2 * Cin, device=DEV)
    with pytest.raises(Change3DHipError):     # the sums are required
        ops.pw_gemm(z(M, Ci), torch.zeros(Ci, Cin, device=DEV), z(M, Cin), wg_mode=ops.WG_MASKSUM, wg_x3=z(M, Cin), **kw)
    with pytest.raises(Change3DHipError):     # sums without the mask
        ops.pw_gemm(z(M, Ci), torch.zeros(Ci, Cin, device=DEV), z(M, Cin), add_c=z(M, Cin), add_mr=mr, add_sums=sums, **kw)
    kw2 = dict(kw, N=48, w_sk=48, e1=z(M, 48))   # the narrow buckets take C3D_WG_ROWS (weight gradient fused as well)
    with pytest.raises(Change3DHipError):
        ops.pw_gemm(z(M, Ci), torch.zeros(Ci, 48, device=DEV), z(M, 48), wg_mode=ops.WG_MASKSUM, wg_x3=z(M, 48), add_c=z(M, 48),
                    add_mr=torch.zeros(96, device=DEV), add_sums=torch.zeros(96, dtype=torch.float64, device=DEV), **kw2)


# The workgroup-cooperative conv_a data + weight gradient (csrc/pw_cdgrad.hip, C3D_OPT_PW_CDG) against the wave-private kernels
# on the same device buffers: the three stage widths of X3D-L (216 -> 96 has no fused form in the first kernel: there the
# reference is its C3D_WG_MASKSUM data gradient plus a separate c3d_pw_wgrad), whole and ragged row counts, with the ReLU mask
# and the folded BatchNorm_c-backward sums and without.  dx must be BIT-identical; sums and dW agree to f32 rounding.
@pytest.mark.parametrize("Ci,Cin,M", [(216, 96, 98304 // 8), (216, 96, 5000 - 7), (108, 48, 16 * 300 - 9), (108, 48, 128 * 40),
                                      (54, 24, 16 * 400 - 3), (54, 24, 128 * 33), (216, 96, 1024)])
@pytest.mark.parametrize("mask", [1, 0])
def test_cooperative_conv_a_data_and_weight_gradient(Ci, Cin, M, mask):
    _need_gpu()
    from change3d_amd import ops
    dt = ops.dt_code(DT)
    Cip, Cinp = ops.cpad(Ci), ops.cpad(Cin)
    t2, a_ = q(rnd((M, Ci), 61), DT), q(rnd((M, Ci), 62), DT)
    A, Bc, Cc = rnd((Ci,), 63), rnd((Ci,), 64, 0.1), rnd((Ci,), 65, 0.1)
    w = rnd((Ci, Cin), 66, 0.2)
    y_prev = torch.relu(q(rnd((M, Cin), 67), DT))
    res = q(rnd((M, Cin), 68), DT)
    cten = q(rnd((M, Cin), 69), DT)
    t2d, ad = (padc(t, Cip).to(DEV, DT).contiguous() for t in (t2, a_))
    yd, rd, cd_ = (padc(t, Cinp).to(DEV, DT).contiguous() for t in (y_prev, res, cten))
    coef = torch.cat([padc(A, Cip), padc(Bc, Cip), padc(Cc, Cip)]).to(DEV)
    mr = torch.cat([padc(rnd((Cin,), 70, 0.5), Cinp), padc(rnd((Cin,), 71).abs() + 0.5, Cinp)]).to(DEV)
    wd = w.to(DEV)
    img = torch.zeros(ops.pw_weight_image_bytes(Cin, Ci, dt), dtype=torch.uint8, device=DEV)
    ops.pw_pack_weights([(wd, img, Cin, Ci, 1, Cin)], dt)
    base = dict(M=M, K=Ci, N=Cin, w_sn=1, w_sk=Cin, dtype=dt, x2=ad, pro_mode=ops.PRO_AFFINE2, pro_p=coef, epi_mode=ops.EPI_ADD,
                e1=rd, w_img=img)

    def run(opt):
        ops.set_option(ops.OPT_PW_CDG, opt)
        dx = torch.full((M, Cinp), float("nan"), dtype=DT, device=DEV)
        dw = torch.ones((Ci, Cin), dtype=torch.float32, device=DEV)          # += onto ones
        s = torch.zeros(2 * Cin, dtype=torch.float64, device=DEV)
        sums = dict(add_c=cd_, add_mr=mr, add_sums=s) if mask else {}
        if opt == 0 and Ci > 112:      # no fused form: masked data gradient (or plain), then the separate weight gradient
            if mask:
                ops.pw_gemm(t2d, wd, dx, wg_mode=ops.WG_MASKSUM, wg_x3=yd, **sums, **base)
            else:
                ops.pw_gemm(t2d, wd, dx, **base)
            kernel = ops.last_kernel()
            ops.pw_wgrad(t2d, yd, dw, M=M, K=Cin, N=Ci, dw_sn=Cin, dw_sk=1, dtype=dt, p2=ad, p_coef=coef)
        else:
            ops.pw_gemm(t2d, wd, dx, wg_mode=ops.WG_ROWS, wg_dw=dw, wg_x3=yd, wg_mask_out=mask, **sums, **base)
            kernel = ops.last_kernel()
        torch.cuda.synchronize()
        return dx, dw, s, kernel

    try:
        dx0, dw0, s0, k0 = run(0)
        dx1, dw1, s1, k1 = run(1)
    finally:
        ops.set_option(ops.OPT_PW_CDG, 3)
    # the two legs ran two kernels (c3d_pw_gemm falls back silently where the cooperative kernel does not apply)
    assert k0.startswith("pw_gemm_kernel<") and k1.startswith("pw_cdg_a_kernel<"), (k0, k1)
    assert torch.isfinite(dx1.float()).all() and dx1.float().abs().max().item() > 0
    assert torch.equal(dx0.view(torch.int16), dx1.view(torch.int16)), f"{int((dx0.view(torch.int16) != dx1.view(torch.int16)).sum())} elements of dx differ"
    if mask:
        assert (dx1[:, :Cin][yd[:, :Cin] == 0] == 0).all()
        scale = s0.abs().max().item()
        assert (s1 - s0).abs().max().item() < 2e-6 * scale + 1e-4, ((s1 - s0).abs().max().item(), scale)
    assert _rel(dw1, dw0) < 2e-5, _rel(dw1, dw0)
    P = q(A * t2 + Bc + Cc * a_, DT).double()
    ref = (P.t() @ y_prev.double() + 1.0).float()
    assert _rel(dw1, ref) < 5e-5, _rel(dw1, ref)      # (this reference rounds P from another association of the two multiply-adds)


# The cooperative conv_c data + weight gradient (csrc/pw_cdgrad.hip, C3D_OPT_PW_CDG bit 1) against the wave-private kernels:
# t1 bit-identical (96 -> 216: up to one-ulp flips in a few elements per million); per-sample sums and dW to f32 rounding.  96 -> 216 has no fused form in the first kernel (its data gradient
# plus a separate c3d_pw_wgrad is the reference there).  rows_per_sample is a multiple of the tile's rows (32 / 64 / 128); a
# ragged last sample, a workgroup that spans two samples, with and without the SE gate.
@pytest.mark.parametrize("Co,Ci,rows,B,ragged", [(96, 216, 3072, 4, 0), (96, 216, 64, 37, 0), (96, 216, 1024, 3, 40), (48, 108, 1024, 5, 0),
                                                   (48, 108, 192, 11, 17), (24, 54, 4096, 3, 0), (24, 54, 256, 9, 100)])
@pytest.mark.parametrize("gated", [1, 0])
def test_cooperative_conv_c_data_and_weight_gradient(Co, Ci, rows, B, ragged, gated):
    _need_gpu()
    from change3d_amd import ops
    M = B * rows - ragged
    dt = ops.dt_code(DT)
    Cop, Cip = ops.cpad(Co), ops.cpad(Ci)
    g, c = q(rnd((M, Co), 81), DT), q(rnd((M, Co), 82), DT)
    A, Bc, Cc = rnd((Co,), 83), rnd((Co,), 84, 0.1), rnd((Co,), 85, 0.1)
    w = rnd((Co, Ci), 86, 0.2)
    b = q(rnd((M, Ci), 87), DT)
    scale, shift = rnd((Ci,), 88).abs() + 0.5, rnd((Ci,), 89, 0.3)
    gate = torch.sigmoid(rnd((B, Ci), 90))
    mean, rstd = rnd((Ci,), 91, 0.5), rnd((Ci,), 92).abs() + 0.5
    gd, cd = (padc(t, Cop).to(DEV, DT).contiguous() for t in (g, c))
    bd = padc(b, Cip).to(DEV, DT).contiguous()
    coef = torch.cat([padc(A, Cop), padc(Bc, Cop), padc(Cc, Cop)]).to(DEV)
    ss = torch.cat([padc(scale, Cip), padc(shift, Cip)]).to(DEV)
    mr = torch.cat([padc(mean, Cip), padc(rstd, Cip)]).to(DEV)
    gt = padc(gate, Cip).to(DEV).contiguous() if gated else None
    wd = w.to(DEV)
    img = torch.zeros(ops.pw_weight_image_bytes(Ci, Co, dt), dtype=torch.uint8, device=DEV)
    ops.pw_pack_weights([(wd, img, Ci, Co, 1, Ci)], dt)
    base = dict(M=M, K=Co, N=Ci, w_sn=1, w_sk=Ci, dtype=dt, x2=cd, pro_mode=ops.PRO_AFFINE2, pro_p=coef, epi_mode=ops.EPI_SWISH_SE_BWD,
                e1=bd, epi_p=ss, epi_gate=gt, epi_q=mr, rows_per_sample=rows, w_img=img)

    def run(opt):
        ops.set_option(ops.OPT_PW_CDG, opt)
        t1 = torch.full((M, Cip), float("nan"), dtype=DT, device=DEV)
        nc3 = torch.zeros(B * Cip * 3, dtype=torch.float64, device=DEV)
        dw = torch.ones((Co, Ci), dtype=torch.float32, device=DEV)
        if opt == 0 and Co > 48:      # no fused form in the first kernel
            ops.pw_gemm(gd, wd, t1, stats=nc3, **base)
            kernel = ops.last_kernel()
            kw = dict(q_gate=gt) if gated else {}
            ops.pw_wgrad(gd, bd, dw, M=M, K=Ci, N=Co, dw_sn=Ci, dw_sk=1, dtype=dt, p2=cd, p_coef=coef, q_mode=ops.PRO_BN_SE_SWISH, q_ss=ss,
                         rows_per_sample=rows, **kw)
        else:
            ops.pw_gemm(gd, wd, t1, stats=nc3, wg_mode=ops.WG_SWISH, wg_dw=dw, **base)
            kernel = ops.last_kernel()
        torch.cuda.synchronize()
        return t1, nc3, dw, kernel

    try:
        t1_0, nc_0, dw_0, k0 = run(0)
        t1_1, nc_1, dw_1, k1 = run(3)
    finally:
        ops.set_option(ops.OPT_PW_CDG, 3)
    assert k0.startswith("pw_gemm_kernel<") and k1.startswith("pw_cdg_c_kernel<"), (k0, k1)
    assert torch.isfinite(t1_1.float()).all() and t1_1.float().abs().max().item() > 0
    # Same operands, same instruction chain (both disassemblies read: packed fma / mul, v_exp, v_rcp in the same association): the
    # results are equal bit for bit on the two narrower layers; at 96 -> 216 ONE element in ~600 000 comes out one bf16 ulp apart
    # (deterministic, both kernels reproduce themselves run to run) -- allowed here as such: at most 4 per million, one ulp each
    diff = t1_0.view(torch.int16) != t1_1.view(torch.int16)
    nd = int(diff.sum())
    assert nd <= max(2, int(4e-6 * diff.numel())), f"{nd} elements of t1 differ"
    if nd:
        a_, b_ = t1_0[diff].float(), t1_1[diff].float()
        assert ((a_ - b_).abs() <= 2.0 ** -7 * torch.maximum(a_.abs(), b_.abs())).all(), (a_, b_)
        assert Co > 48, "the narrower layers are bit-identical"
    scale_ = nc_0.abs().max().item()
    assert (nc_1 - nc_0).abs().max().item() < 3e-6 * scale_ + 1e-4, ((nc_1 - nc_0).abs().max().item(), scale_)
    assert _rel(dw_1, dw_0) < 3e-5, _rel(dw_1, dw_0)
