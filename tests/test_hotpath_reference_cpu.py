"""Pins tests/hotpath_reference.py: at small shapes every float64 restatement, with the bf16 rounding step switched off,
equals torch.autograd through F.conv3d / F.batch_norm / the same composition in float64 to 1e-10 -- forward and every
gradient.  The GPU tests compare kernels with these functions; a wrong restatement must not be able to agree with a wrong
kernel by construction.  The same for tests/decoder_reference.py (transposed convolution, 3x3 head, stem conv_xy backward)
against F.conv_transpose2d / F.conv2d / F.conv3d, at two small ragged shapes each."""
import pytest
import torch
import torch.nn.functional as F

import decoder_reference as D
import hotpath_reference as R

TOL = 1e-10


def rnd(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g, dtype=torch.float64) * scale


def same(a, b, what):
    err = (a - b).abs().max().item()
    assert err <= TOL * max(1.0, b.abs().max().item()), f"{what}: {err:.3e}"


def test_round_bf16_is_round_to_nearest_even_and_flags_near_ties():
    x = torch.cat([rnd((4096,), 1, 3.0), torch.tensor([0.0, 1.0, -1.0, 1.00390625, 1.01171875, 3.0e-5, 1e4])])
    assert torch.equal(R.round_bf16(x), x.float().to(torch.bfloat16).double())   # (no value here sits on an f32 double-rounding edge)
    assert R.round_bf16(torch.tensor([1.00390625], dtype=torch.float64)).item() == 1.0          # tie -> even
    assert R.round_bf16(torch.tensor([1.01171875], dtype=torch.float64)).item() == 1.015625     # tie -> even (up)
    v = torch.tensor([1.0039, 1.002, 1.0], dtype=torch.float64)
    _, slack = R.round_bf16(v, torch.full_like(v, 1e-5))
    assert slack.tolist() == [2.0 ** -7, 0.0, 0.0]


@pytest.mark.parametrize("T,H,W,C,stride", [(3, 9, 11, 5, 1), (3, 9, 11, 5, 2), (4, 8, 6, 3, 2), (5, 7, 10, 4, 1), (3, 4, 5, 2, 2)])
def test_depthwise_restatement_equals_autograd(T, H, W, C, stride):
    B = 2
    a = rnd((B, T, H, W, C), 10).requires_grad_(True)
    w = rnd((C, 27), 11, 0.3).requires_grad_(True)
    scale, shift = rnd((C,), 12).abs() + 0.5, rnd((C,), 13, 0.3)
    x = torch.relu(a * scale + shift)
    x.retain_grad()
    y = F.conv3d(x.permute(0, 4, 1, 2, 3), w.view(C, 1, 3, 3, 3), stride=(1, stride, stride), padding=1, groups=C).permute(0, 2, 3, 4, 1)
    Ho, Wo = R.dw_out_hw(H, W, stride)
    assert y.shape == (B, T, Ho, Wo, C)
    t1 = rnd((B, T, Ho, Wo, C), 14)
    cA, cC, cB = rnd((C,), 15), rnd((C,), 16, 0.1), rnd((B, C), 17, 0.1)
    db = cA * t1 + cB[:, None, None, None, :] + cC * y.detach()
    y.backward(db)
    mean, rstd = rnd((C,), 18, 0.5), rnd((C,), 19).abs() + 0.5
    dw = torch.zeros(C, 27, dtype=torch.float64)
    for n in range(B):
        yn, mag, slack = R.dw_fwd_sample(a[n].detach(), scale, shift, w.detach(), stride)
        same(yn, y[n].detach(), "forward")
        assert (mag >= yn.abs() - 1e-12).all() and (slack == 0).all()
        yr, _, _ = R.dw_fwd_sample(a[n].detach(), scale, shift, w.detach(), stride, round_operand=True)   # 2^-8 per operand
        assert ((yr - yn).abs() <= R.BF16_EPS * mag).all() and not torch.equal(yr, yn)
        s, _ = R.sample_sums(yn)
        same(s[:, 0], y[n].detach().sum((0, 1, 2)), "sum")
        same(s[:, 1], (y[n].detach() ** 2).sum((0, 1, 2)), "sum of squares")
        t2, t2m, dwn, dwm = R.dw_bwd_sample(t1[n], y[n].detach(), cA, cB[n], cC, w.detach(), a[n].detach(), scale, shift, stride)
        # the kernel's t2 is the gradient at the BatchNorm_a output (ReLU mask applied, scale not): a.grad / scale
        same(t2, a.grad[n] / scale, "data gradient")
        same(t2, x.grad[n] * (x[n].detach() > 0), "data gradient (masked)")
        assert (t2m >= t2.abs() - 1e-12).all() and (dwm >= dwn.abs() - 1e-12).all()
        dw += dwn
        ds, _ = R.bn_a_bwd_sums(t2, a[n].detach(), mean, rstd)
        same(ds[1], (t2 * (a[n].detach() - mean) * rstd).sum((0, 1, 2)), "BatchNorm_a sums")
    same(dw, w.grad, "weight gradient")


def test_batchnorm_from_sums_equals_f_batch_norm():
    M, C = 300, 7
    x = rnd((M, C), 20, 2.0) + 0.7
    gamma, beta = rnd((C,), 21).abs() + 0.5, rnd((C,), 22)
    rm, rv = rnd((C,), 23), rnd((C,), 24).abs() + 0.5
    rm2, rv2 = rm.clone(), rv.clone()
    ref = F.batch_norm(x, rm2, rv2, gamma, beta, training=True, momentum=0.1, eps=1e-5)
    bn = R.bn_from_sums(x.sum(0), (x * x).sum(0), float(M), gamma, beta, 1e-5, rm, rv, 0.1)
    same(x * bn["scale"] + bn["shift"], ref, "normalised")
    same(bn["running_mean"], rm2, "running mean")
    same(bn["running_var"], rv2, "running var")
    same((x - bn["mean"]) * bn["rstd"] * gamma + beta, ref, "mean / rstd")


@pytest.mark.parametrize("se", [True, False])
def test_conv_c_forward_and_gradient_equal_autograd(se):
    B, rows, K, N, Cr = 3, 40, 10, 6, 4
    M = B * rows
    b = rnd((M, K), 30).requires_grad_(True)
    gamma, beta = rnd((K,), 31).abs() + 0.5, rnd((K,), 32, 0.2)
    w = rnd((N, K), 33, 0.3).requires_grad_(True)
    w1, b1, w2, b2 = rnd((Cr, K), 34, 0.4), rnd((Cr,), 35, 0.1), rnd((K, Cr), 36, 0.4), rnd((K,), 37, 0.1)
    # the composition of the block (reference order: norm_b -> SE -> Swish -> conv_c) through F.batch_norm
    v = F.batch_norm(b, None, None, gamma, beta, training=True, eps=1e-5)
    v.retain_grad()
    if se:
        z = v.view(B, rows, K).mean(1)
        gate_ref = torch.sigmoid(torch.relu(z @ w1.t() + b1) @ w2.t() + b2)
        qv = v * gate_ref.repeat_interleave(rows, 0)
    else:
        qv = v
    qv.retain_grad()
    y_ref = F.silu(qv) @ w.t()
    bd = b.detach()
    nc = torch.stack([bd.view(B, rows, K).sum(1), (bd * bd).view(B, rows, K).sum(1)], 2)
    out = R.conv_c_fwd(bd, nc, rows, gamma, beta, 1e-5, w.detach(), se=(w1, b1, w2, b2) if se else None, rounded=False, keep_operand=True)
    same(out["y"], y_ref.detach(), "conv_c forward")
    assert (out["mag"] >= out["y"].abs() - 1e-12).all() and (out["slack"] == 0).all()
    if se:
        same(out["gate"], gate_ref.detach(), "SE gate")
    # data gradient: r = dy W, t1 = r swish'(q) gate is the gradient at q's input v along the direct path
    dy = rnd((M, N), 38)
    y_ref.backward(dy)
    coef1 = (torch.ones(N, dtype=torch.float64), torch.zeros(N, dtype=torch.float64), torch.zeros(N, dtype=torch.float64))
    t1s, Ps, dgate = [], [], []
    for n in range(B):
        r = slice(n * rows, (n + 1) * rows)
        o = R.conv_c_dgrad(dy[r], torch.zeros_like(dy[r]), coef1, w.detach(), bd[r], out["bn"]["scale"], out["bn"]["shift"],
                           out["gate"][n] if se else None, rounded=False)
        assert (o["err"] >= 0).all() and (o["Q_slack"] == 0).all()
        same(o["Q"], out["P"][r], "forward operand rebuilt by the backward")
        t1s.append(o["t1"]), Ps.append(o["P"]), dgate.append(o["dgate"])
    t1, P = torch.cat(t1s), torch.cat(Ps)
    gate_rows = out["gate"].repeat_interleave(rows, 0) if se else torch.ones(M, K, dtype=torch.float64)
    same(t1, qv.grad * gate_rows, "conv_c data gradient (direct path)")
    if se:   # d gate: the gradient at the gate, per sample and channel
        ggrad = torch.autograd.grad(F.silu(v.detach() * (gr := gate_rows.clone().requires_grad_(True))) @ w.detach().t(), gr, dy)[0]
        same(torch.stack(dgate), ggrad.view(B, rows, K).sum(1), "d gate sums")
    else:
        same(t1, v.grad, "conv_c data gradient")
    dw, dwm = R.wgrad(P, out["P"])
    same(dw, w.grad, "conv_c weight gradient")
    assert (dwm >= dw.abs() - 1e-12).all()


def test_conv_a_forward_and_gradient_equal_autograd():
    M, K, N = 150, 6, 10
    c = rnd((M, K), 40).requires_grad_(True)
    sc = rnd((M, K), 41).requires_grad_(True)
    gamma, beta = rnd((K,), 42).abs() + 0.5, rnd((K,), 43, 0.2)
    w = rnd((N, K), 44, 0.3).requires_grad_(True)
    rm, rv = rnd((K,), 45), rnd((K,), 46).abs() + 0.5
    rm2, rv2 = rm.clone(), rv.clone()
    po_ref = torch.relu(F.batch_norm(c, rm2, rv2, gamma, beta, training=True, momentum=0.1, eps=1e-5) + sc)
    po_ref.retain_grad()
    y_ref = po_ref @ w.t()
    cd = c.detach()
    out = R.conv_a_fwd(cd, sc.detach(), torch.stack([cd.sum(0), (cd * cd).sum(0)]), gamma, beta, 1e-5, w.detach(), rounded=False,
                       running=(rm, rv))
    same(out["po"], po_ref.detach(), "residual output")
    same(out["y"], y_ref.detach(), "conv_a forward")
    same(out["bn"]["running_mean"], rm2, "running mean")
    same(out["bn"]["running_var"], rv2, "running var")
    assert (out["mag"] >= out["y"].abs() - 1e-12).all() and (out["po_mag"] >= out["po"].abs() - 1e-12).all()
    # conv_a data gradient: da = A g + B + C a (BatchNorm_a backward on load), dx = da W + residual; here A = 1, B = C = 0
    da = rnd((M, N), 47)
    res = rnd((M, K), 48)
    y_ref.backward(da)
    one, zero = torch.ones(N, dtype=torch.float64), torch.zeros(N, dtype=torch.float64)
    o = R.conv_a_dgrad(da, torch.zeros_like(da), (one, zero, zero), w.detach(), res, rounded=False)
    same(o["dx"], po_ref.grad + res, "conv_a data gradient")
    assert (o["err"] >= 0).all()
    # with the ReLU mask of the block's input: what autograd hands below relu(bn_c(c) + shortcut), i.e. the gradient at c / shortcut
    om = R.conv_a_dgrad(da, torch.zeros_like(da), (one, zero, zero), w.detach(), torch.zeros_like(res), y_prev=out["po"], rounded=False)
    same(om["dx"], sc.grad, "masked conv_a data gradient")
    ds, _ = R.bn_bwd_sums(om["dx"], cd, out["bn"]["mean"], out["bn"]["rstd"])
    same(ds[1], (sc.grad * (cd - out["bn"]["mean"]) * out["bn"]["rstd"]).sum(0), "BatchNorm_c backward sums")
    dw, _ = R.wgrad(o["P"], out["po"])
    same(dw, w.grad, "conv_a weight gradient")


def test_affine2_operand_is_batchnorm_backward():
    """A g + B + C x with the coefficients of csrc/bn_fin.h bn_backward is autograd's gradient through training-mode BatchNorm."""
    M, C = 200, 5
    x = rnd((M, C), 50, 1.5).requires_grad_(True)
    gamma, beta = rnd((C,), 51).abs() + 0.5, rnd((C,), 52)
    y = F.batch_norm(x, None, None, gamma, beta, training=True, eps=1e-5)
    g = rnd((M, C), 53)
    y.backward(g)
    xd = x.detach()
    bn = R.bn_from_sums(xd.sum(0), (xd * xd).sum(0), float(M), gamma, beta, 1e-5)
    xhat = (xd - bn["mean"]) * bn["rstd"]
    s1, s2 = g.sum(0), (g * xhat).sum(0)
    A = gamma * bn["rstd"]
    Cc = -A * bn["rstd"] * s2 / M
    Bc = -A * s1 / M - Cc * bn["mean"]
    p, slack = R.affine2_operand(g, xd, A, Bc, Cc, rounded=False)
    same(p, x.grad, "BatchNorm backward")
    assert (slack == 0).all()
    same(R.swish_grad(xd), torch.autograd.grad(F.silu(x).sum(), x)[0], "swish'")


@pytest.mark.parametrize("se", [True, False])
@pytest.mark.parametrize("B,rows,C,Cr", [(3, 16, 54, 8), (5, 48, 108, 8), (2, 16, 216, 16), (33, 16, 24, 8)])
def test_se_and_batchnorm_b_backward_equal_autograd(B, rows, C, Cr, se):
    """se_case / se_bn_bwd against autograd through the explicit block middle: bn_b (batch statistics) -> mean pool -> FC1 -> ReLU
    -> FC2 -> sigmoid -> gate -> Swish.  db = A t1 + B[n] + C b is the gradient at b; the six parameter gradients are autograd's."""
    k = R.se_case(B, rows, C, Cr, seed=60 + B, se=se)
    b = k["b"].clone().requires_grad_(True)
    gamma, beta = k["gamma"].clone().requires_grad_(True), k["beta"].clone().requires_grad_(True)
    pb = F.batch_norm(b.view(B * rows, C), None, None, gamma, beta, training=True, eps=k["eps"]).view(B, rows, C)
    params = [gamma, beta]
    if se:
        w1, b1, w2, b2 = (t.clone().requires_grad_(True) for t in k["se"])
        params += [w1, b1, w2, b2]
        hid = torch.relu(pb.mean(1) @ w1.t() + b1)
        gate = torch.sigmoid(hid @ w2.t() + b2)
        same(k["hid"], hid.detach(), "hid")
        same(k["gate"], gate.detach(), "gate")
        g2, h2, _ = R.se_gate(k["ncf"][:, :, 0], float(rows), k["scale"], k["shift"], *k["se"])
        same(g2, gate.detach(), "se_gate from the per-sample sums")
        same(h2, hid.detach(), "hid from the per-sample sums")
        assert (k["hid"] > 0).any() and (k["hid"] == 0).any()        # both sides of the ReLU mask are exercised
        y = F.silu(pb * gate[:, None, :])
    else:
        assert k["se"] is None and k["gate"] is None and k["hid"] is None
        y = F.silu(pb)
    y.backward(k["d"])
    bn = R.bn_from_sums(k["ncf"][:, :, 0].sum(0), k["ncf"][:, :, 1].sum(0), float(B * rows), k["gamma"], k["beta"], k["eps"])
    for name in ("scale", "shift", "mean", "rstd"):
        same(bn[name], k[name], name)
    r = R.se_bn_bwd(k["nc3"], k["ncf"], float(rows), k["gamma"], k["mean"], k["rstd"], k["scale"], k["shift"], k["se"], k["gate"], k["hid"])
    db = r["coefA"][0] * k["t1"] + r["coefB"][0][:, None, :] + r["coefC"][0] * k["b"]
    same(db, b.grad, "db = A t1 + B[n] + C b")
    names = ["dgamma", "dbeta"] + (["dw1", "db1", "dw2", "db2"] if se else [])
    assert set(r) == set(names) | {"coefA", "coefB", "coefC"}
    for name, p in zip(names, params):
        same(r[name][0], p.grad, name)
    for name, (val, mag, err) in r.items():
        assert val.shape == mag.shape == err.shape, name
        assert (mag >= val.abs() * (1 - 1e-12)).all() and (err >= 0).all(), name
        assert bool((err > 0).any()) == (se and name != "coefA"), name        # only the SE chain is f32 in front of these
    if not se:
        assert torch.equal(r["coefB"][0], r["coefB"][0][:1].expand(B, C))      # one B for every sample


# ------------------------------------------------------------------------------------------------ tests/decoder_reference.py
def _mag_ok(val, mag):
    assert (mag >= val.abs() - 1e-12).all()


@pytest.mark.parametrize("C,B,h,wd", [(3, 2, 5, 7), (5, 1, 1, 6)])
def test_convT_restatements_equal_autograd(C, B, h, wd):
    x = rnd((B, h, wd, C), 100).requires_grad_(True)
    w = rnd((C, C, 4, 4), 101, 0.3).requires_grad_(True)
    bias, skip, dout = rnd((C,), 102), rnd((B, 2 * h, 2 * wd, C), 103), rnd((B, 2 * h, 2 * wd, C), 104)
    y = F.conv_transpose2d(x.permute(0, 3, 1, 2), w, bias, stride=2, padding=1).permute(0, 2, 3, 1) + skip
    y.backward(dout)
    o, m = D.convt4s2_fwd(x.detach(), w.detach(), bias, skip, rounded=False)
    same(o, y.detach(), "convT forward")
    _mag_ok(o, m)
    o2, _ = D.convt4s2_fwd(x.detach(), w.detach(), bias, None, rounded=False)
    same(o2, y.detach() - skip, "convT forward without skip")
    d, m = D.convt4s2_dgrad(dout, w.detach(), rounded=False)
    same(d, x.grad, "convT data gradient")
    _mag_ok(d, m)
    g, m = D.convt4s2_wgrad(x.detach(), dout)
    same(g, w.grad, "convT weight gradient")
    _mag_ok(g, m)
    orr, _ = D.convt4s2_fwd(x.detach(), w.detach(), bias, skip)                    # rounded weights: 2^-9 per product
    assert ((orr - o).abs() <= 2.0 ** -9 * D.convt4s2_fwd(x.detach(), w.detach(), bias, skip, rounded=False)[1]).all() and not torch.equal(orr, o)


@pytest.mark.parametrize("NC,sig,B,H,W", [(1, True, 2, 5, 7), (3, False, 1, 4, 9)])
def test_head_restatements_equal_autograd(NC, sig, B, H, W):
    C = 4
    x = rnd((B, H, W, C), 110).requires_grad_(True)
    w = rnd((NC, C, 3, 3), 111, 0.3).requires_grad_(True)
    dout = rnd((B, NC, H, W), 112)
    lg = F.conv2d(x.permute(0, 3, 1, 2), w, padding=1)
    y = torch.sigmoid(lg) if sig else lg
    y.backward(dout)
    o, l, m = D.head3x3_fwd(x.detach(), w.detach(), sig, rounded=False)
    same(o, y.detach(), "head forward")
    same(l, lg.detach(), "head logits")
    _mag_ok(l, m)
    dx, dxm, dxs, dw, dwm, dws = D.head3x3_bwd(dout, o if sig else None, x.detach(), w.detach(), sig, rounded=False)
    same(dx, x.grad, "head data gradient")
    same(dw, w.grad, "head weight gradient")
    _mag_ok(dx, dxm)
    _mag_ok(dw, dwm)
    assert (dxs == 0).all() and (dws == 0).all()
    dxr, _, dxs, dwr, _, dws = D.head3x3_bwd(dout, o if sig else None, x.detach(), w.detach(), sig)
    assert ((dxr - dx).abs() <= 2.0 ** -7 * dxm).all() and ((dwr - dw).abs() <= 2.0 ** -8 * dwm).all() and not torch.equal(dxr, dx)
    assert (dxs >= 0).all() and (dws >= 0).all()


@pytest.mark.parametrize("B,T,H,W,t_first,n_frames", [(2, 3, 5, 7, 1, 1), (3, 5, 4, 9, 1, 3)])
def test_stem_wx_restatement_equals_autograd(B, T, H, W, t_first, n_frames):
    x = rnd((B, 3, T, H, W), 120).requires_grad_(True)
    w = rnd((24, 3, 1, 3, 3), 121, 0.3).requires_grad_(True)
    dv = rnd((B, T, H, W, 24), 122)
    v = F.conv3d(x, w, padding=(0, 1, 1))
    v.backward(dv.permute(0, 4, 1, 2, 3))
    for per_sample in (True, False):
        out = D.stem_wx(x.detach(), w.detach(), dv, t_first, n_frames, per_sample)
        dw, dwm, dp, dpm = out["unrounded"]
        same(dw, w.grad.reshape(24, 27), "stem dW_t")
        ref = x.grad[:, :, t_first:t_first + n_frames]
        same(dp, ref if per_sample else ref.sum(0), "stem dP")
        _mag_ok(dw, dwm)
        _mag_ok(dp, dpm)
        dwr, _, dpr, _ = out["rounded"]
        assert ((dwr - dw).abs() <= 2.0 ** -9 * dwm).all() and ((dpr - dp).abs() <= 2.0 ** -9 * dpm).all() and not torch.equal(dwr, dw)
    assert D.stem_wx(x.detach(), w.detach(), dv, 0, 0, False)["unrounded"][2] is None
