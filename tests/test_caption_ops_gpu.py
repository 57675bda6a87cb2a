"""Caption-decoder kernels (csrc/caption_ops.hip), one entry point at a time, against the float64 restatements of
tests/caption_reference.py -- with dropout ON.  The device draws its masks from (seed, element index); the tests never
restate that formula: they read the mask back through the op itself (a tensor without zeros goes in, `!= 0` comes out; for
the attention weights, one-hot value rows), hand it to the float64 reference, and require the forward AND the backward to
agree with it.  A backward that regenerates another mask than its forward drew fails here.

Branches of the file that only these shapes reach (test ids in brackets):
  attention  Lq < 16: one workgroup per head; Lq = 17: uneven 5,5,5,2 split      [test_attention Lq 1 / 7 / 15 / 16 / 17]
             Lk > 512: the two `j = lane + 512` tails of the backward            [test_attention 4x600]
             hd 7 (9 lane groups, lane 63 idle), 16, 32, 40 (one group, 24 idle lanes), 64; Lk 1, 2, 65 (unrolled-by-4 key
             loop and its remainder)                                             [test_attention]
             forward takes, backward refuses (52 x 400, hd 24)                    [test_attention_forward_takes_backward_refuses]
  LayerNorm  rows > 1024: more than one row per wave in the backward              [test_layernorm 1025x192, 3001x24]
             D = 512 (all 8 registers), 513 refused, 65 (lane 0 holds two values), D % 8 != 0 (zero padding columns)
  grid cap   4096 workgroups: dropout, embedding (both directions), cross-entropy backward, clamp each run once above
             1 048 576 elements
  CE         declen 0 and L, the last step (l + 1 = L) never counted, nothing counted at all -> loss 0, zero gradient
Tolerances are per element: |err| <= at * max|ref| + rt * |ref| with (2e-5, 2e-5) for f32 storage and (2e-5, 2^-8) for bf16
(compute is f32 either way; bf16 adds one rounding of the output, at most 2^-8 relative)."""
import contextlib
import io
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import caption_reference as R  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DTYPES = [torch.float32, torch.bfloat16]
CANARY = -768.0                      # exact in bf16
GRID_CAP = 4096 * 256                # elements one sweep of a capped element-wise launch covers
E_BADARG, E_UNSUPPORTED = -1, -2


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")


def rnd(shape, seed, scale=1.0):
    g = np.random.default_rng(seed)
    return torch.from_numpy((g.standard_normal(shape) * scale).astype(np.float32))


def nonzero(shape, seed):
    """Random values with |x| in [0.5, 1.5): dropping one is visible as an exact zero."""
    g = np.random.default_rng(seed)
    return torch.from_numpy(((g.random(shape) + 0.5) * g.choice([-1.0, 1.0], size=shape)).astype(np.float32))


def tol(dtype):
    return (2e-5, 2e-5) if dtype == torch.float32 else (2e-5, 2.0 ** -8)


def close(a, b, dtype, what, scale=None, extra=0.0):
    at, rt = tol(dtype)
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    assert a.shape == b.shape, (what, a.shape, b.shape)
    assert torch.isfinite(a).all(), f"{what}: non-finite device values"
    scale = max(b.abs().max().item(), 1e-30) if scale is None else scale
    err = (a - b).abs()
    lim = at * scale + rt * b.abs() + extra
    bad = (err > lim).sum().item()
    assert bad == 0, f"{what}: {bad}/{err.numel()} out of tolerance, worst err/lim {(err / lim).max().item():.2f}, max err {err.max().item():.3e}, ref max {b.abs().max().item():.3e}"


def padded(t, dtype, fill=0.0):
    """[rows, D] -> device [rows, round_up(D, 8)] in the storage dtype, padding columns = fill."""
    from change3d_amd import ops
    rows, D = t.shape
    out = torch.full((rows, ops.cpad(D)), fill, dtype=torch.float32)
    out[:, :D] = t
    return out.to(DEV, dtype).contiguous()


def keep_rate_ok(keep, p, what):
    n = keep.numel()
    rate = keep.double().mean().item()
    assert abs(rate - (1 - p)) <= 5 * math.sqrt(p * (1 - p) / n), f"{what}: keep rate {rate:.4f} of {n} at p = {p}"


# ------------------------------------------------------------------ reading the device's masks back, formula unknown
def elementwise_mask(rows, D, p, seed, dtype=torch.float32):
    from change3d_amd import ops
    x = padded(torch.ones(rows, D), dtype)
    y = torch.empty_like(x)
    ops.cap_dropout(x, y, rows, D, p, seed, ops.dt_code(dtype))
    return (y[:, :D] != 0).cpu()


def embed_mask(tokens, D, V, p, seed, dtype=torch.float32):
    """Embedding rows in [2, 3] and |pe| <= 1: emb + pe is never 0, so a zero is a dropped element."""
    from change3d_amd import ops
    B, L = tokens.shape
    g = np.random.default_rng(1)
    emb = torch.from_numpy((g.random((V, D)) + 2.0).astype(np.float32)).to(DEV)
    pe = rnd((L, D), 2).clamp(-1, 1).to(DEV)
    out = torch.empty((L * B, ops.cpad(D)), dtype=dtype, device=DEV)
    ops.cap_embed_fwd(tokens.to(DEV), emb, pe, out, B, L, D, V, p, seed, ops.dt_code(dtype))
    return (out[:, :D] != 0).cpu().view(L, B, D)


def attention_mask(B, H, Lq, Lk, hd, causal, p, seed, dtype=torch.float32):
    """The mask of the attention weights does not depend on v: with v_k = e_(k - off) for the keys of one block of hd,
    o[i][c] = dropped P[i][off + c].  q = k = 0 makes P uniform over the allowed keys, so every observable weight is > 0;
    where the saved P is 0 (above the causal diagonal) the mask cannot matter and is reported as kept."""
    from change3d_amd import ops
    D, dt = H * hd, ops.dt_code(dtype)
    qz = torch.zeros((Lq * B, D), dtype=dtype, device=DEV)
    kz = torch.zeros((Lk * B, D), dtype=dtype, device=DEV)
    P = torch.empty((H * B, Lq, Lk), dtype=torch.float32, device=DEV)
    keep = torch.ones((B, H, Lq, Lk), dtype=torch.bool)
    for off in range(0, Lk, hd):
        n = min(hd, Lk - off)
        v = torch.zeros((Lk, B, H, hd), dtype=torch.float32)
        v[torch.arange(off, off + n), :, :, torch.arange(n)] = 1.0
        o = torch.empty((Lq * B, D), dtype=dtype, device=DEV)
        ops.cap_attn_fwd(qz, kz, v.view(Lk * B, D).to(DEV, dtype), D, D, D, o, D, P, B, H, Lq, Lk, hd, 1.0, causal, p, seed, dt)
        keep[..., off:off + n] = (o.view(Lq, B, H, hd).permute(1, 2, 0, 3)[..., :n] != 0).cpu()
    return keep | (P.view(H, B, Lq, Lk).permute(1, 0, 2, 3) == 0).cpu()


def rows_of(t):
    """[B, H, L, hd] -> sequence-first rows [L*B, H*hd]."""
    B, H, L, hd = t.shape
    return t.permute(2, 0, 1, 3).reshape(L * B, H * hd)


def heads_of(rows, B, H, L, hd):
    return rows.reshape(L, B, H, hd).permute(1, 2, 0, 3)


# ------------------------------------------------------------------------------------------------------- dropout
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rows,D,p,inplace", [(7, 20, 0.1, True), (156, 192, 0.5, True), (6000, 192, 0.1, False)])
def test_dropout(dtype, rows, D, p, inplace):
    """(6000, 192) is above the grid cap; D = 20 walks Dp = 24 columns while the mask index walks D."""
    _need_gpu()
    from change3d_amd import ops
    dt, Dp = ops.dt_code(dtype), ops.cpad(D)
    assert (rows * Dp > GRID_CAP) == (rows == 6000)
    x = R.q(nonzero((rows, D), 3), dtype)
    xd = padded(x, dtype, fill=CANARY)
    yd = xd if inplace else torch.full_like(xd, CANARY)
    ops.cap_dropout(xd, yd, rows, D, p, 77, dt)
    y = yd.float().cpu()
    keep = y[:, :D] != 0
    assert torch.equal(keep, elementwise_mask(rows, D, p, 77, dtype)), "the mask must not depend on the data"
    close(y[:, :D], R.drop(x, keep, p), dtype, "y")
    assert (y[:, D:] == 0).all(), "padding columns must be written as zero"
    if rows * D >= 1000:
        keep_rate_ok(keep, p, "dropout")
        assert not torch.equal(keep, elementwise_mask(rows, D, p, 78, dtype)), "another seed, another mask"
        assert not torch.equal(keep[: rows // 2], keep[rows - rows // 2:]), "rows must not repeat a pattern"
    # backward is the same call on the gradient: a second application with the same seed keeps the same set
    y2 = torch.empty_like(yd)
    ops.cap_dropout(yd, y2, rows, D, p, 77, dt)
    close(y2[:, :D], R.drop(R.q(y[:, :D], dtype), keep, p), dtype, "second application")
    assert torch.equal(y2[:, :D].cpu() != 0, keep)


# ----------------------------------------------------------------------------------------------------- embedding
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,L,D,V,p", [(3, 52, 192, 203, 0.1), (3, 52, 192, 203, 0.0), (2, 9, 20, 5, 0.1), (110, 52, 192, 11, 0.1)])
def test_embedding(dtype, B, L, D, V, p):
    """Few distinct tokens (V 5 / 11): hundreds of atomic adds land on one embedding row.  Tokens outside [0, V) are clamped
    (include/change3d_hip.h).  (110, 52, 192) is above the grid cap in both directions; D = 20: forward walks Dp, backward D."""
    _need_gpu()
    from change3d_amd import ops
    dt, Dp = ops.dt_code(dtype), ops.cpad(D)
    assert (L * B * D > GRID_CAP) == (B == 110)
    g = np.random.default_rng(5)
    tokens = torch.from_numpy(g.integers(0, V, size=(B, L)))
    tokens[0, 1], tokens[1, 2], tokens[B - 1, L - 1] = -3, V + 2, V
    emb, pe = rnd((V, D), 6, 0.1), rnd((L + 3, D), 7)
    out = torch.full((L * B, Dp), CANARY, dtype=dtype, device=DEV)
    ops.cap_embed_fwd(tokens.to(DEV), emb.to(DEV), pe.to(DEV), out, B, L, D, V, p, 4321, dt)
    mask = embed_mask(tokens, D, V, p, 4321, dtype) if p > 0 else None
    if p > 0:
        keep_rate_ok(mask, p, "embedding")
        assert not torch.equal(mask, embed_mask(tokens, D, V, p, 4322, dtype))
        assert not torch.equal(mask[:, 0], mask[:, 1]), "two samples must not share a mask"
    e64 = emb.double().requires_grad_(True)
    ref = R.embed(tokens, e64, pe.double(), mask, p)
    o = out.float().cpu()
    close(o[:, :D], ref.reshape(L * B, D), dtype, "embedding forward")
    assert (o[:, D:] == 0).all(), "padding columns must be zero"
    dout = R.q(rnd((L * B, D), 8), dtype)
    (ref.reshape(L * B, D) * dout).sum().backward()
    start = rnd((V, D), 9)
    demb = start.to(DEV)
    ops.cap_embed_bwd(tokens.to(DEV), padded(dout, dtype, fill=CANARY), demb, B, L, D, V, p, 4321, dt)
    close(demb.cpu() - start, e64.grad, torch.float32, "embedding gradient (accumulated onto a non-zero start)",
          scale=max(e64.grad.abs().max().item(), start.abs().max().item()))


# ----------------------------------------------------------------------------------------------------- LayerNorm
def _layernorm_case(dtype, rows, D, with_a, offset=0.0):
    from change3d_amd import ops
    dt, Dp = ops.dt_code(dtype), ops.cpad(D)
    x = R.q(rnd((rows, D), 10, 0.1) + offset if offset else rnd((rows, D), 10) + rnd((rows, 1), 11), dtype)
    a = R.q(rnd((rows, D), 12, 0.5), dtype) if with_a else None
    ln = torch.nn.LayerNorm(D).to(DEV)
    gamma, beta = rnd((D,), 13, 0.3) + 1.0, rnd((D,), 14, 0.2)
    g0, b0 = rnd((D,), 15), rnd((D,), 16)
    with torch.no_grad():
        ln.weight.copy_(gamma); ln.bias.copy_(beta)
    ln.weight.grad, ln.bias.grad = g0.to(DEV), b0.to(DEV)
    xd, ad = padded(x.float(), dtype, fill=CANARY), (padded(a.float(), dtype, fill=CANARY) if with_a else None)
    y = torch.full((rows, Dp), CANARY, dtype=dtype, device=DEV)
    mr = torch.full((rows, 2), float("nan"), dtype=torch.float32, device=DEV)
    ops.cap_layernorm_fwd(xd, ad, ln, y, mr, rows, D, dt)
    x64, a64 = x.clone().requires_grad_(True), (a.clone().requires_grad_(True) if with_a else None)
    g64, b64 = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    ref, mean, rstd = R.layernorm(x64, a64, g64, b64, ln.eps)
    shift = 2.0 ** -18 * rstd.max().item() * gamma.abs().max().item() if offset else 0.0
    yc = y.float().cpu()
    close(yc[:, :D], ref, dtype, "y", extra=shift)
    assert (yc[:, D:] == 0).all(), "padding columns of y must be zero"
    mrc = mr.double().cpu()                       # f64 statistics of x + a (an f32 sum), rounded once to f32
    tmax = (x if a is None else x + a).abs().max(-1).values
    assert ((mrc[:, 0] - mean.detach()).abs() <= 2.0 ** -23 * tmax).all(), "saved mean"
    assert ((mrc[:, 1] - rstd.detach()).abs() <= 2.0 ** -22 * rstd.detach()).all(), "saved rstd"
    dy = R.q(rnd((rows, D), 17), dtype)
    (ref * dy).sum().backward()
    dx = torch.full((rows, Dp), CANARY, dtype=dtype, device=DEV)
    ops.cap_layernorm_bwd(xd, ad, padded(dy.float(), dtype, fill=CANARY), ln, mr, dx, rows, D, dt)
    dxc = dx.float().cpu()
    close(dxc[:, :D], x64.grad, dtype, "dx")
    if with_a:
        assert torch.equal(x64.grad, a64.grad)       # one device gradient serves both
    assert (dxc[:, D:] == 0).all(), "padding columns of dx must be zero"
    col = shift * dy.abs().sum(0).max().item()
    close(ln.weight.grad.cpu() - g0, g64.grad, torch.float32, "dgamma (accumulated)", scale=max(g64.grad.abs().max().item(), 1.0), extra=col)
    close(ln.bias.grad.cpu() - b0, b64.grad, torch.float32, "dbeta (accumulated)", scale=max(b64.grad.abs().max().item(), 1.0))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rows,D,with_a", [(832, 192, True), (1025, 192, True), (3001, 24, False), (5, 512, True), (7, 65, False), (9, 20, True)])
def test_layernorm(dtype, rows, D, with_a):
    _need_gpu()
    _layernorm_case(dtype, rows, D, with_a)


def test_layernorm_rows_of_mean_100_std_0_1():
    """f32 storage (bf16 cannot hold 100 +- 0.1).  The statistics are f64 on the device; what remains is the saved mean's
    rounding to f32 (2^-18 at 100), which shifts a whole row of xhat by up to 2^-18 * rstd: that bound, nothing more, is added
    to the tolerances.  No `a`: x + a is formed in f32 and would round by as much again."""
    _need_gpu()
    _layernorm_case(torch.float32, 832, 192, False, offset=100.0)


def test_layernorm_refuses_513_columns():
    _need_gpu()
    from change3d_amd import _lib, ops
    rows, D = 3, 513
    x = torch.zeros((rows, ops.cpad(D)), device=DEV)
    y = torch.full_like(x, CANARY)
    w, mr = torch.ones(D, device=DEV), torch.zeros((rows, 2), device=DEV)
    s = torch.cuda.current_stream().cuda_stream
    p = lambda t: t.data_ptr()  # noqa: E731
    assert _lib.lib().c3d_cap_layernorm_fwd(p(x), None, p(w), p(w), p(y), p(mr), rows, D, 1e-5, ops.DT_F32, s) == E_BADARG
    assert _lib.lib().c3d_cap_layernorm_bwd(p(x), None, p(x), p(w), p(mr), p(y), p(w), p(w), rows, D, ops.DT_F32, s) == E_BADARG
    torch.cuda.synchronize()
    assert (y == CANARY).all() and (w == 1).all()


# ----------------------------------------------------------------------------------------------------- attention
ATTN_CASES = [  # (B, H, Lq, Lk, hd, causal)
    (3, 8, 52, 52, 24, True),      # the training pair: self-attention ...
    (2, 8, 52, 256, 24, False),    # ... and cross-attention over the 16 x 16 memory
    (2, 2, 1, 1, 7, True),         # Lq 1, Lk 1, hd 7: 9 lane groups, lane 63 idle
    (2, 3, 7, 2, 16, False),       # Lk 2 (< the 4 lane groups of hd 16)
    (2, 2, 7, 65, 7, False),       # Lk 65 over 9 groups: unrolled-by-4 loop and remainder
    (1, 2, 15, 65, 32, False),     # Lq 15: the last unsplit length
    (2, 2, 16, 16, 40, True),      # Lq 16: first split length; hd 40: one group, 24 idle lanes
    (2, 1, 17, 17, 64, True),      # Lq 17: split 5, 5, 5, 2; hd 64
    (1, 2, 4, 600, 24, False),     # Lk > 512: the tails of the backward's register-held row
]


def _attention_case(dtype, B, H, Lq, Lk, hd, causal, p, seed=991):
    from change3d_amd import ops
    dt, D, PAD = ops.dt_code(dtype), H * hd, 8
    scale = 1.0 / math.sqrt(hd)
    qh, kh, vh = rnd((B, H, Lq, hd), 20), rnd((B, H, Lk, hd), 21), rnd((B, H, Lk, hd), 22)
    qh[:, 0::2] *= 8.0            # scores of +-30: softmax rows near one-hot ...
    qh[:, 1::2] *= 0.3            # ... and nearly flat ones
    qh, kh, vh = (R.q(t, dtype) for t in (qh, kh, vh))
    new = lambda rows, cols: torch.full((rows, cols), CANARY, dtype=dtype, device=DEV)  # noqa: E731
    if Lq == Lk:                  # as the module passes self-attention: column slices of one packed [R][3D] buffer
        buf = new(Lq * B, 3 * D + PAD)
        for i, t in enumerate((qh, kh, vh)):
            buf[:, i * D:(i + 1) * D] = rows_of(t).to(DEV, dtype)
        qb = kb = vb = buf
        ldq = ldk = ldv = 3 * D + PAD
        qo, ko, vo = 0, D, 2 * D
        gq = gk = gv = new(Lq * B, 3 * D + PAD)
    else:                         # cross-attention: q alone, k | v packed [S*B][2D]
        qb, kb = new(Lq * B, D + PAD), new(Lk * B, 2 * D + PAD)
        qb[:, :D] = rows_of(qh).to(DEV, dtype)
        kb[:, :D], kb[:, D:2 * D] = rows_of(kh).to(DEV, dtype), rows_of(vh).to(DEV, dtype)
        vb = kb
        ldq, ldk, ldv = D + PAD, 2 * D + PAD, 2 * D + PAD
        qo, ko, vo = 0, 0, D
        gq, gk = new(Lq * B, D + PAD), new(Lk * B, 2 * D + PAD)
        gv = gk
    operands = [qb] if qb is kb else [qb, kb]
    before = [t.clone() for t in operands]
    o = new(Lq * B, D + PAD)
    P = torch.full((H * B, Lq, Lk), float("nan"), dtype=torch.float32, device=DEV)
    ops.cap_attn_fwd(qb, kb, vb, ldq, ldk, ldv, o, D + PAD, P, B, H, Lq, Lk, hd, scale, causal, p, seed, dt, q_off=qo, k_off=ko, v_off=vo)
    mask = attention_mask(B, H, Lq, Lk, hd, causal, p, seed, dtype) if p > 0 else None
    q64, k64, v64 = (t.clone().requires_grad_(True) for t in (qh, kh, vh))
    Pref, oref = R.attention(q64, k64, v64, scale, causal, mask, p)
    Pd = P.view(H, B, Lq, Lk).permute(1, 0, 2, 3).cpu()
    assert (Pd.double().sum(-1) - 1).abs().max().item() < 1e-6, "rows of P must sum to 1"
    if causal:
        assert (Pd[..., torch.triu(torch.ones(Lq, Lk, dtype=torch.bool), 1)] == 0).all(), "causal upper triangle must be exactly 0"
    close(Pd, Pref, torch.float32, "P", scale=1.0)
    close(heads_of(o[:, :D].float().cpu(), B, H, Lq, hd), oref, dtype, "o")
    assert (o[:, D:] == CANARY).all(), "forward wrote outside its head columns"
    # backward, gradients into one packed buffer as the module does
    doh = R.q(rnd((B, H, Lq, hd), 23), dtype)
    dob = new(Lq * B, D + PAD)
    dob[:, :D] = rows_of(doh).to(DEV, dtype)
    (oref * doh).sum().backward()
    ops.cap_attn_bwd(qb, kb, vb, ldq, ldk, ldv, dob, D + PAD, P, gq, gk, gv, gq.shape[1], gk.shape[1], gv.shape[1], B, H, Lq, Lk, hd,
                     scale, p, seed, dt, q_off=qo, k_off=ko, v_off=vo, dq_off=qo, dk_off=ko, dv_off=vo)
    for name, g, off, L_, ref in (("dq", gq, qo, Lq, q64.grad), ("dk", gk, ko, Lk, k64.grad), ("dv", gv, vo, Lk, v64.grad)):
        close(heads_of(g[:, off:off + D].float().cpu(), B, H, L_, hd), ref, dtype, name)
    for g in (gq, gk):
        assert (g[:, -PAD:] == CANARY).all(), "backward wrote outside its head columns"
    for t, b in zip(operands, before):
        assert torch.equal(t, b), "operands must not be modified"
    return mask


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("case", ATTN_CASES, ids=lambda c: "B{}H{}_{}x{}_hd{}_{}".format(*c[:5], "causal" if c[5] else "cross"))
def test_attention(dtype, p, case):
    _need_gpu()
    _attention_case(dtype, *case, p)


def test_attention_half_dropped():
    _need_gpu()
    _attention_case(torch.float32, 2, 2, 16, 16, 40, True, 0.5)
    _attention_case(torch.float32, 2, 8, 52, 256, 24, False, 0.5)


def test_attention_mask_statistics():
    """Keep rate, and no mask shared between seeds, samples or heads."""
    _need_gpu()
    m = attention_mask(2, 2, 52, 52, 24, False, 0.1, 5)
    keep_rate_ok(m, 0.1, "attention weights")
    assert not torch.equal(m, attention_mask(2, 2, 52, 52, 24, False, 0.1, 6))
    assert not torch.equal(m[0, 0], m[0, 1]) and not torch.equal(m[0, 0], m[1, 0]) and not torch.equal(m[0, 1], m[1, 0])
    assert not torch.equal(m[0, 0, :26], m[0, 0, 26:])


def _attn_rc(fn, bwd, B, H, Lq, Lk, hd, bufs):
    from change3d_amd import ops
    q, k, o, P, g = bufs
    D, s = H * hd, torch.cuda.current_stream().cuda_stream
    p = lambda t: t.data_ptr()  # noqa: E731
    if bwd:
        return fn(p(q), p(k), p(k), D, D, D, p(o), D, p(P), p(g[0]), p(g[1]), p(g[2]), D, D, D, B, H, Lq, Lk, hd, 0.2, 0.0, 0, ops.DT_F32, s)
    return fn(p(q), p(k), p(k), D, D, D, p(o), D, p(P), B, H, Lq, Lk, hd, 0.2, 0, 0.0, 0, ops.DT_F32, s)


def test_attention_forward_takes_backward_refuses():
    """Lq 52, Lk 400, hd 24: 92 KB of LDS forward, 174 KB backward.  The entry points say so by return code, the refused call
    writes nothing, and the Python-side arithmetic the decoder uses to refuse such a step up front agrees with both."""
    _need_gpu()
    from change3d_amd import _lib
    from change3d_amd.model.caption_decoder import ATTN_LDS_LIMIT, attn_lds_bytes
    B, H, Lq, Lk, hd = 1, 1, 52, 400, 24
    fwd, bwd = attn_lds_bytes(Lq, Lk, hd)
    assert fwd <= ATTN_LDS_LIMIT < bwd
    z = lambda *s: torch.zeros(s, device=DEV)  # noqa: E731
    g = [torch.full((Lk, hd), CANARY, device=DEV) for _ in range(3)]
    bufs = (z(Lq, hd), z(Lk, hd), z(Lq, hd), z(H * B, Lq, Lk), g)
    assert _attn_rc(_lib.lib().c3d_cap_attn_fwd, False, B, H, Lq, Lk, hd, bufs) == 0
    assert _attn_rc(_lib.lib().c3d_cap_attn_bwd, True, B, H, Lq, Lk, hd, bufs) == E_UNSUPPORTED
    torch.cuda.synchronize()
    assert all((t == CANARY).all() for t in g), "a refused call must not write"
    assert abs(bufs[3].sum().item() - Lq) < 1e-3          # the forward did run: 52 rows of uniform probabilities
    for Lq_, Lk_ in ((52, 256), (4, 600), (52, 380), (52, 370)):   # the two budgets, either side of the backward limit
        fwd, bwd = attn_lds_bytes(Lq_, Lk_, hd)
        assert fwd <= ATTN_LDS_LIMIT
        bufs = (z(Lq_, hd), z(Lk_, hd), z(Lq_, hd), z(1, Lq_, Lk_), [z(Lk_, hd) for _ in range(3)])
        assert (_attn_rc(_lib.lib().c3d_cap_attn_bwd, True, 1, 1, Lq_, Lk_, hd, bufs) == 0) == (bwd <= ATTN_LDS_LIMIT), (Lq_, Lk_)
    torch.cuda.synchronize()


def test_attention_refuses_head_width_65():
    _need_gpu()
    from change3d_amd import _lib
    g = [torch.full((4, 65), CANARY, device=DEV) for _ in range(3)]
    bufs = (torch.zeros(4, 65, device=DEV), torch.zeros(4, 65, device=DEV), torch.full((4, 65), CANARY, device=DEV),
            torch.zeros(1, 4, 4, device=DEV), g)
    assert _attn_rc(_lib.lib().c3d_cap_attn_fwd, False, 1, 1, 4, 4, 65, bufs) == E_BADARG
    assert _attn_rc(_lib.lib().c3d_cap_attn_bwd, True, 1, 1, 4, 4, 65, bufs) == E_BADARG
    torch.cuda.synchronize()
    assert (bufs[2] == CANARY).all() and all((t == CANARY).all() for t in g)


def test_decoder_refuses_a_step_its_backward_cannot_take():
    """Train mode, S = 400: refused before the first launch, naming S and L; the same geometry in eval mode (no backward) runs."""
    _need_gpu()
    from change3d_amd import synthetic as synth
    from change3d_amd.model.caption_decoder import CaptionDecoder
    args = synth.make_cc_args(size=64, vocab_size=31, dropout=0.1)
    with contextlib.redirect_stdout(io.StringIO()):
        dec = CaptionDecoder(args).to(DEV).train()
    mem = synth.synth_tensor((400, 1, 192), 3).to(DEV)
    caps, _ = synth.synth_captions(1, seed=1, vocab_size=31)
    with pytest.raises(NotImplementedError, match=r"L = 52 .*S = 400"):
        dec.logits_seq_first(mem, caps.to(DEV))
    with torch.no_grad():
        assert torch.isfinite(dec.eval().logits_seq_first(mem, caps.to(DEV))[:, :31]).all()


# ------------------------------------------------------------------------------------------------- cross-entropy
def _ce_inputs(B, L, V, dtype, seed):
    g = np.random.default_rng(seed)
    logits = rnd((L, B, V), seed + 1, 3.0)
    logits[1, 0, V - 1], logits[2, 2, 0], logits[0, B - 1, 3] = 80.0, -80.0, 80.0     # a stable log-sum-exp is needed
    caps = torch.from_numpy(g.integers(1, V, size=(B, L)))
    caps[0, 3], caps[2, 2] = 0, 0                                                       # ignore_index inside the counted range
    j1, j2 = (5, 64) if V > 64 else (2, 7)                                             # a tie: the higher index sits in the lower lane
    logits[3, 0, j1] = logits[3, 0, j2] = logits[4, 2, j1] = logits[4, 2, j2] = 90.0
    caps[0, 4], caps[2, 5] = j1, j2                                                     # first index wins: a hit, then a miss
    declen = torch.tensor(([L, 0, L - 1, 3] * B)[:B])
    return R.q(logits, dtype), caps, declen


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,L,V", [(4, 7, 11), (3, 9, 64), (4, 7, 65), (3, 52, 203), (4, 52, 501), (101, 52, 203)])
def test_cross_entropy(dtype, B, L, V):
    """declen holds L (its last step has no target and is never counted), 0 and values between.  (101, 52, 203): the backward
    above the grid cap."""
    _need_gpu()
    from change3d_amd import ops
    dt, Vp = ops.dt_code(dtype), ops.cpad(V)
    assert (L * B * Vp > GRID_CAP) == (B == 101)
    logits, caps, declen = _ce_inputs(B, L, V, dtype, 30)
    lg = torch.full((L * B, Vp), 55.0, dtype=dtype, device=DEV)      # padding columns hold a value that would win every max
    lg[:, :V] = logits.reshape(L * B, V).to(DEV, dtype)
    acc = torch.full((3,), float("nan"), dtype=torch.float64, device=DEV)
    lse = torch.full((L * B,), float("nan"), dtype=torch.float32, device=DEV)
    loss = torch.full((1,), float("nan"), dtype=torch.float32, device=DEV)
    ops.cap_ce_fwd(lg, caps.to(DEV), declen.to(DEV), acc, lse, loss, B, L, V, 0, dt)
    l64 = logits.clone().requires_grad_(True)
    ref, n, hits = R.packed_ce(l64, caps, declen, 0)
    assert n > 0 and acc[1].item() == n and acc[2].item() == hits, (acc.tolist(), n, hits)
    assert abs(acc[0].item() - ref.item() * n) <= 2e-5 * max(1.0, ref.item() * n)
    assert abs(loss.item() - ref.item()) <= 2e-5 * max(1.0, ref.item())
    # against torch's own loss on the packed rows, as the reference training script computes it
    tgt = torch.cat([caps[:, 1:], torch.zeros(B, 1, dtype=torch.int64)], 1).t()
    sel = torch.arange(L)[:, None] < declen[None, :]
    torch_loss = torch.nn.functional.cross_entropy(logits[sel], tgt[sel], ignore_index=0)
    assert abs(ref.item() - torch_loss.item()) < 1e-12 * max(1.0, torch_loss.item())
    dloss = 0.37
    (ref * dloss).backward()
    d = torch.full((L * B, Vp), CANARY, dtype=dtype, device=DEV)
    ops.cap_ce_bwd(lg, caps.to(DEV), declen.to(DEV), acc, lse, torch.tensor([dloss], device=DEV), d, B, L, V, 0, dt)
    dc = d.float().cpu()
    close(dc[:, :V], l64.grad.reshape(L * B, V), dtype, "dlogits")
    assert (dc[:, V:] == 0).all(), "padding columns of dlogits must be zero"
    ops.cap_ce_bwd(lg, caps.to(DEV), declen.to(DEV), acc, lse, None, d, B, L, V, 0, dt)          # dloss NULL = 1
    close(d.float().cpu()[:, :V], l64.grad.reshape(L * B, V) / dloss, dtype, "dlogits, dloss NULL")


@pytest.mark.parametrize("dtype", DTYPES)
def test_cross_entropy_nothing_counted(dtype):
    """No counted step (all decode lengths 0, or every target ignore_index): torch's mean over nothing is NaN; this kernel
    defines loss = 0, acc2 = (0, 0, 0) and a zero gradient (include/change3d_hip.h) -- a skipped batch, not a poisoned one."""
    _need_gpu()
    from change3d_amd import ops
    B, L, V = 3, 7, 11
    dt, Vp = ops.dt_code(dtype), ops.cpad(V)
    logits, caps, _ = _ce_inputs(B, L, V, dtype, 31)
    lg = padded(logits.reshape(L * B, V).float(), dtype)
    for caps_, declen in ((caps, torch.zeros(B, dtype=torch.int64)), (torch.zeros_like(caps), torch.full((B,), L))):
        acc = torch.full((3,), float("nan"), dtype=torch.float64, device=DEV)
        lse = torch.full((L * B,), float("nan"), dtype=torch.float32, device=DEV)
        loss = torch.full((1,), float("nan"), dtype=torch.float32, device=DEV)
        ops.cap_ce_fwd(lg, caps_.to(DEV), declen.to(DEV), acc, lse, loss, B, L, V, 0, dt)
        assert loss.item() == 0.0 and acc.tolist() == [0.0, 0.0, 0.0]
        ref, n, hits = R.packed_ce(logits, caps_, declen, 0)
        assert ref.item() == 0.0 and n == 0 and hits == 0
        d = torch.full((L * B, Vp), CANARY, dtype=dtype, device=DEV)
        ops.cap_ce_bwd(lg, caps_.to(DEV), declen.to(DEV), acc, lse, torch.ones(1, device=DEV), d, B, L, V, 0, dt)
        assert (d == 0).all()


# ---------------------------------------------------------------------------------------------------------- clamp
def test_clamp_keeps_nan_and_clips_everything_else():
    """torch semantics (`param.grad.data.clamp_(-c, c)` of the reference's clip_gradient): NaN stays NaN, +-inf go to the limit.
    n is above the grid cap, with special values in the part only the second sweep reaches."""
    _need_gpu()
    from change3d_amd import _lib, ops
    n, lim = GRID_CAP + 77, 5.0
    g = rnd((n,), 40, 4.0)
    for base in (0, GRID_CAP + 3):
        g[base:base + 8] = torch.tensor([lim, -lim, lim + 1e-3, -lim - 1e-3, float("inf"), float("-inf"), float("nan"), 0.0])
    assert (g.abs() > lim).sum() > 1000 and (g.abs() < lim).sum() > 1000
    d = g.to(DEV)
    ops.clamp_(d, lim)
    want = g.clamp(-lim, lim)
    got = d.cpu()
    assert torch.equal(got.isnan(), want.isnan()), "NaN must stay NaN: clipping must not hide a diverged gradient"
    assert torch.equal(got.nan_to_num(7.0), want.nan_to_num(7.0))
    keep = torch.full((16,), 9.0, device=DEV)
    s = torch.cuda.current_stream().cuda_stream
    for bad in (0.0, -1.0, float("nan")):
        assert _lib.lib().c3d_clamp_(keep.data_ptr(), 16, bad, s) == E_BADARG
    torch.cuda.synchronize()
    assert (keep == 9.0).all()


# --------------------------------------------------------------------------------- linear layers and their bias sum
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("M,C_", [(832, 203), (5, 20), (517, 576)])
def test_col_sum(dtype, M, C_):
    _need_gpu()
    from change3d_amd import ops
    x = R.q(rnd((M, C_), 50), dtype)
    start = rnd((C_,), 51)
    out = start.to(DEV)
    ops.col_sum(padded(x.float(), dtype, fill=CANARY), out, M, C_, ops.dt_code(dtype))
    close(out.cpu() - start, x.sum(0), torch.float32, "column sums (accumulated)", scale=max(x.sum(0).abs().max().item(), 1.0))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("M,K,N,rows_from,acc", [(832, 192, 576, 0, "separate"), (512, 192, 384, 192, "inplace"), (832, 192, 203, 0, None),
                                                 (517, 192, 192, 0, "separate")])
def test_linear_forward_backward(dtype, M, K, N, rows_from, acc):
    """nn.Linear on c3d_pw_gemm (bias) / EPI_ADD (residual gradient) / c3d_pw_wgrad / c3d_col_sum at the decoder's shapes:
    in_proj (192 -> 576), the memory projection on the row-slice view in_proj_weight[D:] with its gradient slices gw[D:] /
    gb[D:] (non-zero storage offset) accumulating into dmem in place, wdc (192 -> 203, Np 208), and a ragged M."""
    _need_gpu()
    from change3d_amd import ops
    dt, Np = ops.dt_code(dtype), ops.cpad(N)
    x, dy = R.q(rnd((M, K), 60), dtype), R.q(rnd((M, N), 61), dtype)
    wfull = R.q(rnd((rows_from + N, K), 62, 0.1), dtype)        # bf16-representable weights: the bf16 path rounds them
    bfull = rnd((rows_from + N,), 63, 0.5).double()
    wd, bd = wfull.float().to(DEV), bfull.float().to(DEV)
    y = torch.full((M, Np), CANARY, dtype=dtype, device=DEV)
    xd = padded(x.float(), dtype)
    ops.linear_fwd(xd, wd[rows_from:], bd[rows_from:], y, M, K, N, dt)
    w64, x64 = wfull.clone().requires_grad_(True), x.clone().requires_grad_(True)
    b64 = bfull.clone().requires_grad_(True)
    ref = x64 @ w64[rows_from:].t() + b64[rows_from:]
    yc = y.float().cpu()
    close(yc[:, :N], ref, dtype, "y")
    assert (yc[:, N:] == 0).all(), "padding columns of y must be zero"
    (ref * dy).sum().backward()
    gw0, gb0, res = rnd(tuple(wfull.shape), 64), rnd(tuple(bfull.shape), 65), R.q(rnd((M, K), 66), dtype)
    gw, gb = gw0.to(DEV), gb0.to(DEV)
    dx = padded(res.float(), dtype) if acc == "inplace" else torch.full((M, K), CANARY, dtype=dtype, device=DEV)
    e1 = dx if acc == "inplace" else (padded(res.float(), dtype) if acc else None)
    ops.linear_bwd(xd, wd[rows_from:], padded(dy.float(), dtype), dx, gw[rows_from:], gb[rows_from:], M, K, N, dt, accumulate_dx=e1)
    # bf16 storage: the narrow kernel (192 x 192) stages its result tile in LDS as bf16 (pw_gemm_impl.h OutStage), so the
    # product is rounded once before the f32 residual add -- 2^-8 of the product, on top of the output's own rounding
    staged = 2.0 ** -8 * x64.grad.abs().max().item() if acc and dtype == torch.bfloat16 else 0.0
    close(dx.float().cpu(), x64.grad + (res if acc else 0.0), dtype, "dx", extra=staged)
    close(gw.cpu() - gw0, w64.grad, torch.float32, "weight gradient (accumulated)", scale=w64.grad.abs().max().item())
    close(gb.cpu() - gb0, b64.grad, torch.float32, "bias gradient (accumulated)", scale=b64.grad.abs().max().item())
    if rows_from:
        assert torch.equal(gw[:rows_from].cpu(), gw0[:rows_from]) and torch.equal(gb[:rows_from].cpu(), gb0[:rows_from])


# ------------------------------------------------------------------------- the whole decoder in train mode, dropout on
@pytest.mark.parametrize("dtype,tol_", [(torch.float32, 2e-4), (torch.bfloat16, 6e-2)])
@pytest.mark.parametrize("p", [0.0, 0.1])
def test_decoder_train_mode_with_dropout_vs_float64(dtype, tol_, p):
    """`CaptionDecoder` in train mode as the training script runs it (--dropout 0.1, the position encoding's own 0.1 on) under
    torch.manual_seed: every one of the 2 + 4 x 3 masks is read back from the device with the seed `dropout_seed` gives its
    site, the float64 layer stack gets them, and logits, loss, memory gradient and every parameter gradient must agree at the
    bounds tests/test_cc_gpu.py::test_caption_decoder_module_vs_oracle uses at p = 0.  p = 0 is the control on the yardstick."""
    _need_gpu()
    from change3d_amd import synthetic as synth
    from change3d_amd.model.caption_decoder import CaptionDecoder, dropout_seed, packed_cross_entropy
    V, S, B, L, D, H = 203, 37, 3, 52, 192, 8
    args = synth.make_cc_args(size=64, vocab_size=V, dropout=p)
    args.act_dtype = dtype
    with contextlib.redirect_stdout(io.StringIO()):
        mine = CaptionDecoder(args)
    sd = synth.synth_state_dict(mine, seed=9)
    sd["position_encoding.pe"] = mine.state_dict()["position_encoding.pe"].clone()
    mine.load_state_dict(sd)
    mine = mine.to(DEV).train()
    p_pos = mine.position_encoding.dropout.p if p > 0 else 0.0
    mine.position_encoding.dropout.p = p_pos
    mem = synth.synth_tensor((S, B, D), 11)
    caps, caplens = synth.synth_captions(B, seed=4, vocab_size=V)
    torch.manual_seed(1234)
    base = int(torch.randint(0, 2 ** 31 - 1, (1,)).item())          # the draw logits_seq_first makes
    torch.manual_seed(1234)
    md = mem.to(DEV).requires_grad_(True)
    lg = mine.logits_seq_first(md, caps.to(DEV))
    loss, acc = packed_cross_entropy(lg, caps.to(DEV), caplens.to(DEV), V, return_stats=True)
    loss.backward()
    torch.cuda.synchronize()
    masks = {}
    if p > 0:
        masks["pos"] = embed_mask(caps, D, V, p_pos, dropout_seed(base, "pos"), dtype)
        masks["out"] = elementwise_mask(L * B, D, p, dropout_seed(base, "out"), dtype)
        for li in range(args.n_layer):
            masks[li, "attn1"] = attention_mask(B, H, L, L, D // H, True, p, dropout_seed(base, "attn1", li), dtype)
            masks[li, "drop1"] = elementwise_mask(L * B, D, p, dropout_seed(base, "drop1", li), dtype)
            masks[li, "attn2"] = attention_mask(B, H, L, S, D // H, False, p, dropout_seed(base, "attn2", li), dtype)
            masks[li, "drop3"] = elementwise_mask(L * B, D, p, dropout_seed(base, "drop3", li), dtype)
        assert len(masks) == 2 + 4 * args.n_layer
        assert len({m.numpy().tobytes() for m in masks.values()}) == len(masks), "every site draws its own mask"
    sd64 = {k: v.double().requires_grad_(True) for k, v in sd.items() if v.is_floating_point()}
    m64 = R.q(mem, dtype).requires_grad_(True)
    ref = R.decoder_forward(sd64, m64, caps, masks, H, p, p_pos, p)
    lref, n, hits = R.packed_ce(ref, caps, caplens.reshape(-1) - 1, 0)
    lref.backward()
    rel = lambda a, b: ((a.detach().double().cpu() - b).norm() / (b.norm() + 1e-30)).item()  # noqa: E731
    got = lg.detach().float().cpu().view(L, B, -1)[:, :, :V]
    e_logits = (got - ref.detach()).abs().max().item()
    e_mem = rel(md.grad, m64.grad)
    used = {id(q_) for q_ in mine.used_parameters()}
    errs = {k: rel(q_.grad, sd64[k].grad) for k, q_ in mine.named_parameters() if id(q_) in used}
    worst = max(errs, key=errs.get)
    print(f"decoder p={p} {dtype}: max|logit err| {e_logits:.2e}, loss {loss.item():.6f} vs {lref.item():.6f}, memory gradient rel-L2 "
          f"{e_mem:.2e}, worst parameter gradient {worst} {errs[worst]:.2e}")
    assert e_logits < tol_ * max(1.0, ref.abs().max().item())
    assert abs(loss.item() - lref.item()) < tol_ * max(1.0, abs(lref.item()))
    assert acc[1].item() == n
    assert e_mem < 10 * tol_, ("memory gradient", e_mem)
    assert len(errs) == len(used) and errs[worst] < 10 * tol_, sorted(errs.items(), key=lambda kv: -kv[1])[:5]
    assert all(q_.grad is None for q_ in mine.parameters() if id(q_) not in used)
