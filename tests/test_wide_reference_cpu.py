"""Pins tests/wide_reference.py: at small shapes every float64 restatement of what csrc/pw_wide.hip computes, with the rounding
steps switched off, equals float64 torch.autograd (F.linear / F.batch_norm / F.silu / F.conv2d) to 1e-10 -- forward and every
gradient.  tests/test_wide_parity_gpu.py compares the kernels with these functions; a wrong restatement must not be able to
agree with a wrong kernel by construction."""
import pytest
import torch
import torch.nn.functional as F

import hotpath_reference as R
import wide_reference as WR

TOL = 1e-10


def rnd(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g, dtype=torch.float64) * scale


def same(a, b, what):
    assert a.shape == b.shape, f"{what}: {tuple(a.shape)} vs {tuple(b.shape)}"
    err = (a - b).abs().max().item()
    assert err <= TOL * max(1.0, b.abs().max().item()), f"{what}: {err:.3e}"


def test_linear_with_bias_forward_and_all_three_gradients():
    M, K, N = 37, 11, 9
    x, w, b = rnd((M, K), 1).requires_grad_(True), rnd((N, K), 2, 0.3).requires_grad_(True), rnd((N,), 3).requires_grad_(True)
    y_ref = F.linear(x, w, b)
    dy = rnd((M, N), 4)
    y_ref.backward(dy)
    y, mag, sl = WR.gemm(*WR.pro_none(x.detach()), w.detach(), bf16=True, bias=b.detach(), rounded=False)
    same(y, y_ref.detach(), "linear forward")
    assert (mag >= y.abs() - 1e-12).all() and (sl == 0).all()
    dx, _, _ = WR.gemm(*WR.pro_none(dy), w.detach().t(), bf16=True, rounded=False)          # the transposed weight view (w_sn = 1)
    same(dx, x.grad, "data gradient")
    dw, dwm, dsl = WR.wgrad(dy, torch.zeros_like(dy), x.detach(), torch.zeros_like(x.detach()))
    same(dw, w.grad, "weight gradient")
    assert (dwm >= dw.abs() - 1e-12).all() and (dsl == 0).all()
    same(R.col_stats(dy)[0][0], b.grad, "bias gradient")
    # rounding on: weights and nothing else move for bf16 storage (x is exact), nothing at all for f32 storage
    yr, _, _ = WR.gemm(*WR.pro_none(x.detach()), w.detach(), bf16=True, bias=b.detach())
    assert not torch.equal(yr, y) and ((yr - y).abs() <= R.BF16_EPS * mag).all()
    yf, _, _ = WR.gemm(*WR.pro_none(x.detach()), w.detach(), bf16=False, bias=b.detach())
    assert torch.equal(yf, y)


def _conv_stride2(v, BT, H, W):
    """Rows [BT * H * W][C] -> the even pixels, through F.conv2d with an identity 1 x 1 kernel and stride 2."""
    Cn = v.shape[1]
    img = v.view(BT, H, W, Cn).permute(0, 3, 1, 2)
    eye = torch.eye(Cn, dtype=v.dtype).view(Cn, Cn, 1, 1)
    return F.conv2d(img, eye, stride=2).permute(0, 2, 3, 1).reshape(-1, Cn)


@pytest.mark.parametrize("H,W", [(6, 8), (4, 2)])
def test_stride2_gather_and_its_adjoint_the_scatter_to_even_pixels(H, W):
    BT, Cn = 3, 5
    v = rnd((BT * H * W, Cn), 10).requires_grad_(True)
    sub = _conv_stride2(v, BT, H, W)
    same(WR.gather_stride2(v.detach(), BT, H, W), sub.detach(), "stride-2 gather")
    res = rnd((BT * (H // 2) * (W // 2), Cn), 11)
    sub.backward(res)
    same(WR.scatter_even(res, BT, H, W), v.grad, "scatter to even pixels")


@pytest.mark.parametrize("res_mode", [0, 1])
def test_residual_add_in_both_modes(res_mode):
    BT, H, W, K, N = 2, 4, 6, 7, 5
    M = BT * H * W
    x, w = rnd((M, K), 20), rnd((N, K), 21, 0.3)
    if res_mode == 0:
        res = rnd((M, N), 22)
        y_ref = F.linear(x, w) + res
    else:
        # the data gradient of a block whose shortcut is a stride-2 1 x 1 convolution: the shortcut's share arrives at half
        # resolution and belongs to the even pixels -- autograd through the strided identity convolution
        res = rnd((BT * (H // 2) * (W // 2), N), 22)
        v = torch.zeros(M, N, dtype=torch.float64, requires_grad=True)
        _conv_stride2(v, BT, H, W).backward(res)
        y_ref = F.linear(x, w) + v.grad
    y, mag, _ = WR.gemm(*WR.pro_none(x), w, bf16=True, rounded=False)
    y, mag = WR.epi_add(y, mag, res, res_mode, BT, H, W)
    same(y, y_ref, "residual add")
    assert (mag >= y.abs() - 1e-12).all()


@pytest.mark.parametrize("gated", [True, False])
@pytest.mark.parametrize("rows,M", [(16, 150), (17, 153), (48, 144)])
def test_bn_se_swish_gemm_and_column_statistics(gated, rows, M):
    K, N = 10, 6
    B = (M + rows - 1) // rows
    b = rnd((M, K), 30)
    gamma, beta = rnd((K,), 31).abs() + 0.5, rnd((K,), 32, 0.2)
    w = rnd((N, K), 33, 0.3)
    gate = torch.sigmoid(rnd((B, K), 34)) if gated else None
    v = F.batch_norm(b, None, None, gamma, beta, training=True, eps=1e-5)
    gr = None if gate is None else WR.sample_rows(gate, M, rows)
    y_ref = F.linear(F.silu(v if gr is None else v * gr), w)
    bn = R.bn_from_sums(b.sum(0), (b * b).sum(0), float(M), gamma, beta, 1e-5)
    P, sl = WR.pro_swish(b, bn["scale"], bn["shift"], gr, bf16=True, rounded=False)
    y, mag, _ = WR.gemm(P, sl, w, bf16=True, rounded=False)
    same(y, y_ref, "BN_SE_SWISH -> GEMM")
    for bf16 in (True, False):          # the error the operand carries is reported in both storage types
        Pr, slr = WR.pro_swish(b, bn["scale"], bn["shift"], gr, bf16=bf16)
        assert ((Pr - P).abs() <= (R.BF16_EPS * P.abs() if bf16 else 0 * P)).all() and (slr >= 0).all()
    s, sm = WR.stripe_stats(y, block_rows=64, stripes=2)
    same(s.sum(0)[0], y_ref.sum(0), "column sums")
    same(s.sum(0)[1], (y_ref * y_ref).sum(0), "column sums of squares")
    blocks = [y_ref[i:i + 64] for i in range(0, M, 64)]
    same(s[1, 0], sum(blk.sum(0) for blk in blocks[1::2]), "stripe 1 = the odd row blocks")
    assert (sm >= s.abs() - 1e-12).all()


def test_affine2_from_sums_equals_the_batchnorm_backward():
    M, Cn, N = 90, 7, 5
    x = (rnd((M, Cn), 40, 2.0) + 0.7).requires_grad_(True)
    gamma, beta = (rnd((Cn,), 41).abs() + 0.5).requires_grad_(True), rnd((Cn,), 42).requires_grad_(True)
    g = rnd((M, Cn), 43)
    F.batch_norm(x, None, None, gamma, beta, training=True, eps=1e-5).backward(g)
    xd = x.detach()
    mean = xd.mean(0)
    rstd = 1.0 / torch.sqrt(((xd - mean) ** 2).mean(0) + 1e-5)
    sums, _ = R.bn_bwd_sums(g, xd, mean, rstd)
    coef, mag, (dgamma, dbeta) = WR.bn_bwd_coef(sums, gamma.detach(), mean, rstd, float(M), rounded=False)
    P, sl = WR.pro_affine2(g, xd, coef[0], coef[1], coef[2], bf16=True, rounded=False)
    same(P, x.grad, "A g + B + C x")
    same(dgamma, gamma.grad, "dgamma")
    same(dbeta, beta.grad, "dbeta")
    assert (mag >= coef.abs() - 1e-12).all() and (sl == 0).all()
    cr, _, _ = WR.bn_bwd_coef(sums, gamma.detach(), mean, rstd, float(M))
    assert torch.equal(cr, coef.float().double()) and ((cr - coef).abs() <= 2.0 ** -24 * mag).all()
    # ... and feeds the GEMM: the data gradient below the BatchNorm
    w = rnd((Cn, N), 44, 0.3)          # conv weight [out = Cn][in = N]
    dx, _, _ = WR.gemm(P, sl, w.t(), bf16=True, rounded=False)
    same(dx, x.grad @ w, "data gradient through the transposed weight")


@pytest.mark.parametrize("gated", [True, False])
@pytest.mark.parametrize("rows,M", [(16, 80), (17, 85), (21, 100), (48, 130)])
def test_swish_se_backward_epilogue_and_its_three_per_sample_sums(gated, rows, M):
    N = 6
    B = (M + rows - 1) // rows          # (the last sample may be partial)
    b = rnd((M, N), 50)
    scale, shift = rnd((N,), 51).abs() + 0.5, rnd((N,), 52, 0.3)
    mean, rstd = rnd((N,), 53, 0.5), rnd((N,), 54).abs() + 0.5
    d = rnd((M, N), 55)
    gate = torch.sigmoid(rnd((B, N), 56)).requires_grad_(True)
    pb = (b * scale + shift).requires_grad_(True)
    q = pb * WR.sample_rows(gate, M, rows) if gated else pb
    F.silu(q).backward(d)
    gr = WR.sample_rows(gate.detach(), M, rows) if gated else None
    o = WR.epi_swish_se_bwd(d, torch.zeros_like(d), b, scale, shift, gr)
    same(o["t"], pb.grad, "t = dq gate: the gradient at the BatchNorm output")
    if gated:
        same(WR.sample_sum(o["s0_term"], rows), gate.grad, "s0 = sum dq pb: the gradient at the gate")
    else:
        same(WR.sample_sum(o["s0_term"], rows), WR.sample_sum(pb.grad * pb.detach(), rows), "s0 without a gate")
    s1, s2, m1, m2 = WR.se_bwd_sums_of_stored(o["t"], b, mean, rstd, rows)
    assert s1.shape == (B, N)
    for n in range(B):
        r = slice(n * rows, min(M, (n + 1) * rows))
        same(s1[n], pb.grad[r].sum(0), "s1")
        same(s2[n], (pb.grad[r] * (b[r] - mean) * rstd).sum(0), "s2")
    assert (m1 >= s1.abs() - 1e-12).all() and (m2 >= s2.abs() - 1e-12).all()
    assert (o["t_err"] >= 0).all() and (o["s0_err"] >= 0).all()


@pytest.mark.parametrize("gated", [True, False])
def test_weight_gradient_operand_forms(gated):
    """dW = P^T Q with P = A p + B + C p2 and Q = swish(gate (q scale + shift)): the gradient of the layer y = Q W^T at W."""
    M, K, N, rows = 75, 9, 7, 17
    B = (M + rows - 1) // rows
    p, p2, qx = rnd((M, N), 60), rnd((M, N), 61), rnd((M, K), 62)
    A, Bc, Cc = rnd((N,), 63), rnd((N,), 64, 0.1), rnd((N,), 65, 0.1)
    scale, shift = rnd((K,), 66).abs() + 0.5, rnd((K,), 67, 0.3)
    gr = WR.sample_rows(torch.sigmoid(rnd((B, K), 68)), M, rows) if gated else None
    w = rnd((N, K), 69).requires_grad_(True)
    pre = qx * scale + shift
    F.linear(F.silu(pre * gr if gated else pre), w).backward(A * p + Bc + Cc * p2)
    P, ps = WR.pro_affine2(p, p2, A, Bc, Cc, bf16=True, rounded=False)
    Q, qs = WR.pro_swish(qx, scale, shift, gr, bf16=True, rounded=False)
    dw, mag, sl = WR.wgrad(P, ps, Q, qs)
    same(dw, w.grad, "weight gradient")
    assert (mag >= dw.abs() - 1e-12).all() and (sl == 0).all()
    for bf16 in (True, False):
        Pr, psr = WR.pro_affine2(p, p2, A, Bc, Cc, bf16=bf16)
        Qr, qsr = WR.pro_swish(qx, scale, shift, gr, bf16=bf16)
        dwr, _, slr = WR.wgrad(Pr, psr, Qr, qsr)
        assert ((dwr - dw).abs() <= 2.01 * R.BF16_EPS * mag).all() and (slr >= 0).all()


def test_weight_gradient_row_split_plan():
    # launch_wide_wgrad on 256 CUs: 432 x 192 is 7 x 3 blocks of 64 x 64
    assert WR.wgrad_plan(3072, 432, 192, 256) == (128, 24)
    assert WR.wgrad_plan(450, 432, 192, 256) == (128, 4)           # a short last split: 66 rows
    assert WR.wgrad_plan(128, 432, 192, 256) == (128, 1)
    assert WR.wgrad_plan(31, 192, 576, 256) == (32, 1) and WR.wgrad_plan(5, 96, 432, 256) == (32, 1)
    assert WR.wgrad_plan(3072, 192, 576, 256) == (192, 16)         # limited by the workgroups wanted, not by the rows
