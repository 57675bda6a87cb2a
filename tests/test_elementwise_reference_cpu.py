"""tests/elementwise_reference.py against torch.autograd in float64 (no GPU): the restatements the block-output and enhance
kernels are compared with (tests/test_elementwise_gpu.py) are themselves the operations of the model."""
import pytest
import torch
import torch.nn.functional as F

import elementwise_reference as E

TOL = 1e-12
F64 = torch.float64


def _close(a, b, what):
    scale = max(float(b.abs().max()), 1e-300)
    err = float((a - b).abs().max()) / scale
    assert err <= TOL, (what, err)


def _rn(g, *shape, scale=1.0):
    return torch.randn(*shape, generator=g, dtype=F64) * scale


def _bn_stats(x, gamma, beta, eps):
    mean = x.mean(0)
    rstd = 1.0 / torch.sqrt(x.var(0, unbiased=False) + eps)
    scale = gamma * rstd
    return mean, rstd, scale, beta - mean * scale


@pytest.mark.parametrize("form", ["none", "identity", "bn"])
@pytest.mark.parametrize("M,C", [(5, 8), (37, 24), (301, 54)])
def test_block_output_restatement_equals_autograd(form, M, C):
    g = torch.Generator().manual_seed(100 * M + C)
    eps = 1e-5
    c = (_rn(g, M, C) * (0.5 + torch.rand(C, generator=g, dtype=F64)) + _rn(g, C)).requires_grad_()
    s = (_rn(g, M, C) + 0.3).requires_grad_()
    gam_c, bet_c = (_rn(g, C)).requires_grad_(), _rn(g, C, scale=0.3).requires_grad_()      # both signs
    gam_1, bet_1 = (_rn(g, C)).requires_grad_(), _rn(g, C, scale=0.3).requires_grad_()
    dy = _rn(g, M, C) + 1.0
    dy[torch.rand(M, C, generator=g) < 0.1] = 0.0

    pre = F.batch_norm(c, None, None, gam_c, bet_c, training=True, eps=eps)
    if form == "identity":
        pre = pre + s
    elif form == "bn":
        pre = pre + F.batch_norm(s, None, None, gam_1, bet_1, training=True, eps=eps)
    y = torch.relu(pre)
    y.backward(dy)

    with torch.no_grad():
        mean_c, rstd_c, a, b = _bn_stats(c, gam_c, bet_c, eps)
        mean_1, rstd_1, a1, b1 = _bn_stats(s, gam_1, bet_1, eps)
        if form == "none":
            y_ref, mag = E.block_out_fwd(c, a, b)
            bwd = E.block_out_bwd(dy, y_ref, c, mean_c, rstd_c)
        elif form == "identity":
            y_ref, mag = E.block_out_fwd(c, a, b, s)
            bwd = E.block_out_bwd(dy, y_ref, c, mean_c, rstd_c)
        else:
            y_ref, mag = E.block_out_fwd(c, a, b, s, a1, b1)
            bwd = E.block_out_bwd(dy, y_ref, c, mean_c, rstd_c, s, mean_1, rstd_1)
        _close(y_ref, y.detach(), "y")
        assert bool((mag >= y_ref).all())                     # the magnitude sum dominates the value
        gg = bwd["g"]
        assert bool((gg != 0).any()) and bool((gg == 0).any())
        assert bool((bwd["mag_c"] >= bwd["sums_c"].abs() * (1 - 1e-12)).all())
        k = E.bn_bwd_coef(bwd["sums_c"], float(M), gam_c, mean_c, rstd_c)
        _close(k["A"] * gg + k["B"] + k["C"] * c, c.grad, "dc")
        _close(k["dgamma"], gam_c.grad, "dgamma_c")
        _close(k["dbeta"], bet_c.grad, "dbeta_c")
        if form == "identity":
            _close(gg, s.grad, "ds")
        if form == "bn":
            k1 = E.bn_bwd_coef(bwd["sums_1"], float(M), gam_1, mean_1, rstd_1)
            _close(k1["A"] * gg + k1["B"] + k1["C"] * s, s.grad, "ds")
            _close(k1["dgamma"], gam_1.grad, "dgamma_1")
            _close(k1["dbeta"], bet_1.grad, "dbeta_1")
            assert torch.equal(bwd["sums_1"][0], bwd["sums_c"][0])


@pytest.mark.parametrize("T,frames", [(3, (0, 2, 1)), (4, (0, 3, 2)), (5, (0, 4, 2)), (5, (3, 1, 0))])
@pytest.mark.parametrize("B", [1, 3])
def test_enhance_restatement_equals_autograd(T, frames, B):
    t_pre, t_post, t_mid = frames
    HW, C = 35, 24
    g = torch.Generator().manual_seed(10 * T + B)
    y = _rn(g, B, T, HW, C)
    same = torch.rand(B, HW, C, generator=g) < 0.2          # y_pre == y_post: the sign there is 0
    y[:, t_post] = torch.where(same, y[:, t_pre], y[:, t_post])
    y.requires_grad_()
    w = _rn(g, C, C, scale=0.3)
    dout = _rn(g, B, T, HW, C) + 0.5

    out = y.clone()
    e_ag = F.conv1d((y[:, t_pre] - y[:, t_post]).abs().transpose(1, 2), w[:, :, None]).transpose(1, 2)     # the 1x1 convolution
    out[:, t_mid] = out[:, t_mid] + torch.relu(e_ag)
    out.backward(dout)

    with torch.no_grad():
        yd = y.detach()
        d = E.frame_absdiff(yd, t_pre, t_post)
        assert bool((d == 0).any()) and bool((d > 0).any())
        e = d @ w.t()
        assert bool((e > 0).any()) and bool((e < 0).any())
        _close(E.enhance_apply(yd, e, t_mid), out.detach(), "out")
        de = E.enhance_bwd_mask(dout, e, t_mid)
        dd = de @ w
        _close(E.enhance_bwd_apply(dout, yd, dd, t_pre, t_post), y.grad, "dy")
        assert torch.equal(E.enhance_bwd_apply(dout, yd, dd, -1, T), dout)      # no frame matches


def test_enhance_bwd_apply_refuses_one_index_out_of_range():
    x = torch.zeros(1, 3, 4, 8, dtype=F64)
    with pytest.raises(ValueError):
        E.enhance_bwd_apply(x, x, x[:, 0], 0, 3)


@pytest.mark.parametrize("accumulate", [False, True])
def test_frame_scatter_restatement(accumulate):
    g = torch.Generator().manual_seed(5)
    src, dst = _rn(g, 2, 7, 8), _rn(g, 2, 4, 7, 8)
    out = E.frame_scatter(src, dst, 2, accumulate)
    want = torch.stack([dst[:, 0], dst[:, 1], dst[:, 2] + src if accumulate else src, dst[:, 3]], 1)
    assert torch.equal(out, want)


def test_launch_rule_and_the_sums_bound():
    """The shapes of tests/test_elementwise_gpu.py come from this rule: (Cp, G, blk) per width, one grid stride S = 384 rows
    per workgroup, the longest f32 chain of a thread and the eps it gives."""
    want = {8: (8, 1, 256), 24: (24, 3, 255), 54: (56, 7, 252), 108: (112, 14, 252), 216: (216, 27, 243), 256: (256, 32, 256)}
    for C, (Cp, G, blk) in want.items():
        assert E.launch_rule(C)[:3] == (Cp, G, blk)
        S = E.launch_rule(C)[4]
        assert S == 384 * (256 // G)
        assert [E.chain_steps(M, C) for M in (1, S, S + 1, 4 * S + 1, 5 * S + S // 2 + 3, 7 * S + 5)] == [1, 1, 2, 5, 6, 8]
    assert 7 * E.launch_rule(24)[4] + 5 == 228485
    assert E.sums_eps(8) == 2.0 ** -20 and E.sums_eps(1) == 2.0 ** -22 and E.sums_eps(13) == 2.0 ** -20 and E.sums_eps(14) == 2.0 ** -19


def test_f32_operation_then_rounding_equals_direct_rounding_of_absdiff():
    """|p - q| of bf16 values over a 1000 x range of magnitudes: the f32 operation followed by the bf16 rounding (what the
    device does) equals rounding the exact float64 result once (the difference of two bf16 values within 2^16 of each
    other in magnitude is exact in f32, so there is no double rounding)."""
    g = torch.Generator().manual_seed(9)
    mag = 10.0 ** (3.0 * torch.rand(100000, generator=g, dtype=F64) - 1.5)
    p = E.round_bf16(_rn(g, 100000) * mag)
    q = E.round_bf16(_rn(g, 100000) * mag.flip(0))
    dev = (p.float() - q.float()).abs().to(torch.bfloat16).double()
    assert int((dev != E.round_bf16((p - q).abs())).sum()) == 0
