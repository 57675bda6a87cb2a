"""Float64 restatement of the folded-BatchNorm inference forward of a residual stage (csrc/stage_driver.hip, "eval" section:
c3d_stage_fold_bn + c3d_stage_fwd_folded): plain torch on the CPU, nothing imported from the package, the oracle or the
reference tree.  tests/test_folded_reference_cpu.py pins it against float64 eval() modules with the rounding steps switched
off; tests/test_folded_parity_gpu.py compares the device with it.  The arithmetic shared with the training kernels comes from
tests/hotpath_reference.py (round_bf16 with its near-boundary marks, dw_fwd_sample, se_gate, swish_operand, gemm_with_bound).

Conventions as there: activations are the storage-type values the device gets, as float64, [B,T,H,W,C] WITHOUT padding
channels; parameters are the f32 values the device gets, as float64.  A block is a plain dict
    cin, cinner, cout, stride, w_a [Ci][Cin], w_b [Ci][27], w_c [Co][Ci], w_sc [Co][Cin] or None,
    bn_a, bn_b, bn_c, bn_sc (each (gamma, beta, running_mean, running_var); bn_sc None without a shortcut BatchNorm),
    se (w1 [Cr][Ci], b1, w2 [Ci][Cr], b2) or None.

Where the device rounds (read off the code):
  fold_bn_kernel        rstd = (float)(1 / sqrt((double)var + (double)eps)); sc = gamma * rstd; sh = beta - mean * sc (the
                        compiler may contract it into one fma); wf = w * sc.  ss = (1 | sh): what is left of a BatchNorm is a bias.
                        A shortcut convolution without BatchNorm is copied as it is.
  c3d_pw_gemm           conv_a / shortcut: no prologue, the stored input IS the operand.  bf16 storage rounds the f32 (folded)
                        weights to bf16 on their way to LDS; f32 storage multiplies f32 x f32 (v_mfma_f32_16x16x4_f32).  The f32
                        accumulator is rounded to the storage type on store.
  c3d_dw333_fwd         x = max(fma(a, 1, sh_a), 0) inside the image, 0 outside (the padding is applied AFTER the activation), 27
                        fma with the folded taps, rounded on store.  The stride-2 kernel of four- and five-frame clips
                        (dw_fwd_kernel) keeps x in LDS in the storage type: bf16 storage rounds the operand there.  The per-sample
                        sums (SE blocks) are over the STORED values.
  c3d_bn_se_finalize    training = 2: z = fma(1, (float)(sum / rows), sh_b), the two FC layers in f32, gate = 1 / (1 + expf(-a)).
  conv_c                q = gate * fma(b, 1, sh_b), operand q sigmoid(q), rounded to bf16 for the matrix cores (bf16 storage).
  c3d_block_out_fwd     y = max(fma(c, 1, sh_c) + fma(s, 1, sh_1), 0) (sh_1 = 0 and s the block's input or the raw shortcut
                        convolution in the two modes without a shortcut BatchNorm), rounded on store.

Error model.  Every stored tensor t comes as (t, slack): t is the reference's own stored value, slack >= |t_device - t| for any
correct device.  With v the value in front of the store and err the absolute error of the device's f32 value of it
(eps * sum|term| of the kernel's own roundings + what its operands' slack brings along), the device stores the SAME value as the
reference unless a rounding boundary of the storage type lies within err of v: slack = err + one ulp there, 0 elsewhere (for f32
storage err exceeds an ulp almost everywhere and slack = err + ulp).  That keeps the bound of a chain as tight as the bound of
one kernel.  `widen=True` budgets the rounding steps themselves as well (slack = err + ulp everywhere): the bound that must then
contain the UNROUNDED float64 result, which is how tests/test_folded_reference_cpu.py checks the propagation.
The final check of a block's output is the neighbouring files' form, against the unrounded v:
    |device - v| <= rel (|v| + err) + err,   rel = 2^-8 (bf16) or 2^-24 (f32 storage).
"""
import torch

import hotpath_reference as R

U = 1.001 * 2.0 ** -24          # unit roundoff of f32 (1.001: second-order terms of the chains)
EPS_DW = R.EPS_DW + 4 * U       # depthwise: 27 fma + the operand (tests/test_hotpath_bf16_gpu.py) + the folded taps' own error
EPS_NC = 2.0 ** -15             # per-sample sums of the depthwise forward: a lane's f32 chain over its walk (same file)
EPS_OUT = 2.0 ** -22            # block_out_fwd: two fma and one add (tests/elementwise_reference.py EPS_FWD)


def storage_eps(bf16):
    return R.BF16_EPS if bf16 else 2.0 ** -24


def eps_gemm(K, bf16):
    """The matrix cores add K products into an f32 accumulator, one rounding per product charged; f32 x f32 products are
    charged a second one (bf16 x bf16 products are exact): (K + 2) u or (2 K + 2) u, rounded up to a power of two -- the
    figure of tests/test_wide_parity_gpu.py, which equals tests/test_hotpath_bf16_gpu.py's 2^-16 at K <= 224 (bf16)."""
    n, p = (K if bf16 else 2 * K) + 2, 1
    while p < n:
        p *= 2
    return p * 2.0 ** -24


def _f32(t):
    return t.float().to(t.dtype)


def _ulp(x, bits):
    _, e = torch.frexp(x)
    return torch.ldexp(torch.ones_like(x), e - bits)


def round_f32(x, err):
    """f32 counterpart of hotpath_reference.round_bf16(x, err): the value and one ulp where a boundary lies within err."""
    m, e = torch.frexp(x)
    s = m * 2.0 ** 24
    ulp = torch.ldexp(torch.ones_like(x), e - 24)
    near = ((s - torch.floor(s) - 0.5).abs() * ulp) <= err
    return _f32(x), torch.where(near, ulp, torch.zeros_like(x))


def store(v, err, bf16, rounded=True, widen=False, relu=False):
    """A value rounded to bf16 (bf16=True) or f32 where the device rounds it -> (t, slack) as the module text defines them.
    relu: the device clips before it rounds; an element whose pre-activation lies within err of zero may come out as
    anything up to err."""
    r = torch.relu(v) if relu else v
    err = err + torch.zeros_like(r)
    if not rounded:
        return r, err
    t, mark = R.round_bf16(r, err) if bf16 else round_f32(r, err)
    ulp = _ulp(r, 8 if bf16 else 24)
    if widen:
        return t, err + ulp
    near = (mark > 0) | ((v.abs() <= err) & (err > 0))
    return t, torch.where(near, err + ulp, torch.zeros_like(err))


def operand(p, err, bf16, rounded=True, widen=False):
    """A converted operand on its way to the matrix cores (or to the LDS tile of dw_fwd_kernel): bf16 storage rounds it, f32
    storage keeps the f32 value, whose error is the slack."""
    if bf16:
        return store(p, err, True, rounded, widen)
    return p, err + torch.zeros_like(p)


# ------------------------------------------------------------------------------------------------ fold_bn_kernel
def fold(w, gamma, beta, mean, var, eps, rounded=True):
    """w [N][K] -> dict(w, w_err [N][K], shift, shift_err [N], scale).  rounded: rstd in float64 rounded to f32 once, then one
    f32 operation each for sc, sh and w sc; eps is the f32 value the descriptor carries.  The error bounds allow rstd to fall
    on the neighbouring f32 (the device's float64 sqrt and division may differ from the host's in the last bit) and sh to be
    contracted or not."""
    if not rounded:
        sc = gamma / torch.sqrt(var + eps)
        wf = w * sc[:, None]
        return dict(w=wf, w_err=torch.zeros_like(wf), shift=beta - mean * sc, shift_err=torch.zeros_like(sc), scale=sc)
    eps32 = float(torch.tensor(eps, dtype=torch.float32))
    rstd = _f32(1.0 / torch.sqrt(var + eps32))
    sc = _f32(gamma * rstd)
    sh = _f32(beta - mean * sc)
    wf = _f32(w * sc[:, None])
    e_sc = 2 * U * sc.abs()
    return dict(w=wf, w_err=w.abs() * e_sc[:, None] + U * wf.abs(), shift=sh,
                shift_err=mean.abs() * e_sc + 2 * U * (beta.abs() + (mean * sc).abs()), scale=sc)


def plain(w):
    """A convolution without BatchNorm (the res2 shortcut): the weights as they are, no shift."""
    z = torch.zeros(w.shape[0], dtype=w.dtype)
    return dict(w=w, w_err=torch.zeros_like(w), shift=z, shift_err=z, scale=z + 1)


# ------------------------------------------------------------------------------------------------ pieces of one block
def pointwise(P, sP, fw, bf16, rounded=True, widen=False):
    """P [M][K] operand with its slack, fw a folded layer: the f32 tile in front of the store, and its absolute error."""
    Wr, sW = operand(fw["w"], fw["w_err"], bf16, rounded, widen)
    y, mag, sl = R.gemm_with_bound(P, sP, Wr)
    return y, (eps_gemm(P.shape[1], bf16) * mag if rounded else 0.0) + sl + (P.abs() + sP) @ sW.t()


def depthwise(a, sa, fa, fb, stride, bf16, rounded=True, widen=False, pad_bug=False):
    """One sample: a [T,H,W,C] stored conv_a output with its slack, fa / fb the folded BatchNorm_a (its shift) and conv_b
    (its taps) -> the f32 value in front of the store [T,Ho,Wo,C] and its error.  pad_bug (negative control): the activation
    applied to the zero padding of H and W, max(0 + sh_a, 0) instead of 0."""
    T = a.shape[0]
    one = torch.ones_like(fa["shift"])
    lds_round = bf16 and rounded and stride == 2 and T > 3        # dw_fwd_kernel<bf16, 2, 4, 8, T>: the tile is bf16
    y, mag, mark = R.dw_fwd_sample(a, one, fa["shift"], fb["w"], stride, round_operand=lds_round)
    # what the operand's own error brings along: relu is 1-Lipschitz, the padding stays zero
    e_x = sa + fa["shift_err"]
    if lds_round:       # an operand whose input already differs may round to the neighbour
        x = torch.relu(a + fa["shift"])
        e_x = e_x + torch.where(sa > 0, _ulp(x, 8), torch.zeros_like(x))
    if widen and bf16 and stride == 2 and T > 3:
        e_x = e_x + _ulp(torch.relu(a + fa["shift"]), 8)
    prop = R.dw_fwd_sample(e_x, one, torch.zeros_like(one), fb["w"].abs(), stride)[0]
    if pad_bug:
        w3 = fb["w"].view(-1, 3, 3, 3)
        inb = R.dw_fwd_sample(torch.zeros_like(a), one, one, fb["w"], stride)[0]       # sum of the taps that fall inside
        full = torch.stack([w3[:, [kt for kt in range(3) if 0 <= t + kt - 1 < T]].sum((1, 2, 3)) for t in range(T)])
        y = y + torch.relu(fa["shift"]) * (full[:, None, None, :] - inb)
    return y, (EPS_DW * mag if rounded else 0.0) + mark + prop


def gate_of(b, sb, fb, se, rounded=True):
    """SE gate from the stored conv_b output b [B,T,Ho,Wo,C] (c3d_bn_se_finalize, training = 2) -> gate [B][C] and its error,
    the chain of tests/test_bn_se_gpu.py with the error of the per-sample sums in front."""
    w1, b1, w2, b2 = se
    rows = float(b.shape[1] * b.shape[2] * b.shape[3])
    C, Cr = b.shape[-1], w1.shape[0]
    per = [R.sample_sums(b[n]) for n in range(b.shape[0])]          # what the forward leaves in nc [B][Cp][2]; the gate uses the sums
    sums, abs_sums = torch.stack([s[:, 0] for s, _ in per]), torch.stack([m[:, 0] for _, m in per])
    one = torch.ones_like(fb["shift"])
    gate, _, mag = R.se_gate(sums, rows, one, fb["shift"], w1, b1, w2, b2)
    if not rounded:
        return gate, torch.zeros_like(gate)
    m = sums / rows
    z_err = (EPS_NC * abs_sums + sb.sum((1, 2, 3))) / rows + 2 * U * (m.abs() + fb["shift"].abs()) + fb["shift_err"]
    h_err = ((C + 7) // 8 + 4) * U * mag["hid_mag"] + z_err @ w1.abs().t()
    a_err = Cr * U * mag["gate_mag"] + h_err @ w2.abs().t()
    return gate, 0.25 * a_err + 4 * U


def swish_rows(b_rows, sb_rows, fb, gate_row, gate_err, bf16, rounded=True, widen=False):
    """conv_c's operand of one sample's rows [M][K]: q = gate (b + sh_b), q sigmoid(q); gate_row [K] or None.  f32 error of
    the value as hotpath_reference.swish_operand states it, plus the operands' own errors through the slope of Swish (< 1.1)."""
    one = torch.ones_like(fb["shift"])
    g = None if gate_row is None else gate_row.expand_as(b_rows)
    p, _ = R.swish_operand(b_rows, one, fb["shift"], g, rounded=False)
    pre = b_rows + fb["shift"]
    e_q = sb_rows + fb["shift_err"]
    own = b_rows.abs() + fb["shift"].abs()
    if gate_row is not None:
        e_q, own = e_q * gate_row.abs() + gate_err * pre.abs(), own * gate_row.abs()
    err = 1.1 * e_q + ((2.0 ** -22 * own + 2.0 ** -17 * p.abs()) if rounded else 0.0)
    return operand(p, err, bf16, rounded, widen)


def gather_stride2(x, off=0):
    """C3D_ROWS_STRIDE2: output pixel (ho, wo) of the (H + 1) / 2 x (W + 1) / 2 map reads input pixel (2 ho + off, 2 wo)."""
    return x[:, :, off::2, 0::2]


def block(x, slack_x, p, eps, bf16, rounded=True, widen=False, tamper=None, gate_given=None):
    """One block of c3d_stage_fwd_folded.  x [B,T,H,W,Cin] with its slack -> dict: y (stored) and slack [B,T,Ho,Wo,Co] for the
    next block, v (the value in front of the store), err and bound for the check of the device's y, a / b / c, and the
    reference's own gate with its error bound gate_err.
    gate_given [B][Ci]: the f32 gate the DEVICE computed (it is a tensor of the eval workspace).  conv_c is then restated
    on that gate, without error, and the caller checks |gate_given - gate| <= gate_err on its own: the worst-case bound of
    the gate (a per-sample f32 sum and two FC layers, no cancellation credited) would otherwise dominate the bound of y.
    tamper (negative controls): a dict with pad_bug, swap_gates (i, j), sc_offset."""
    tamper = tamper or {}
    B, T, H, W, Cin = x.shape
    s, Ci, Co = p["stride"], p["cinner"], p["cout"]
    Ho, Wo = R.dw_out_hw(H, W, s)
    fa, fb, fc = (fold(p["w_" + k], *p["bn_" + k], eps, rounded) for k in "abc")
    kw = dict(bf16=bf16, rounded=rounded, widen=widen)
    # conv_a
    va, ea = pointwise(x.reshape(-1, Cin), slack_x.reshape(-1, Cin), fa, **kw)
    a, sa = store(va, ea, **kw)
    a, sa = a.view(B, T, H, W, Ci), sa.view(B, T, H, W, Ci)
    # depthwise, sample by sample
    bs = [store(*depthwise(a[n], sa[n], fa, fb, s, pad_bug=bool(tamper.get("pad_bug")), **kw), **kw) for n in range(B)]
    b, sb = torch.stack([t for t, _ in bs]), torch.stack([e for _, e in bs])
    # SE gate
    gate = gate_err = gate_ref = gate_ref_err = None
    if p["se"] is not None:
        gate, gate_err = gate_ref, gate_ref_err = gate_of(b, sb, fb, p["se"], rounded)
        if gate_given is not None:
            gate, gate_err = gate_given, torch.zeros_like(gate_given)
        if tamper.get("swap_gates"):
            i, j = tamper["swap_gates"]
            perm = list(range(B))
            perm[i], perm[j] = j, i
            gate, gate_err = gate[perm], gate_err[perm]
    # conv_c
    vc, ec = [], []
    for n in range(B):
        P, sP = swish_rows(b[n].reshape(-1, Ci), sb[n].reshape(-1, Ci), fb, None if gate is None else gate[n],
                           None if gate is None else gate_err[n], **kw)
        y, e = pointwise(P, sP, fc, **kw)
        vc.append(y), ec.append(e)
    c, sc = store(torch.cat(vc), torch.cat(ec), **kw)
    # shortcut
    sh_1, sh_1_err = torch.zeros_like(fc["shift"]), torch.zeros_like(fc["shift"])
    if p["w_sc"] is None:
        sv, ss = x.reshape(-1, Cin), slack_x.reshape(-1, Cin)
    else:
        f1 = fold(p["w_sc"], *p["bn_sc"], eps, rounded) if p["bn_sc"] is not None else plain(p["w_sc"])
        xs, sxs = (x, slack_x) if s == 1 else (gather_stride2(x, tamper.get("sc_offset", 0)), gather_stride2(slack_x, tamper.get("sc_offset", 0)))
        sv, ss = store(*pointwise(xs.reshape(-1, Cin), sxs.reshape(-1, Cin), f1, **kw), **kw)
        sh_1, sh_1_err = f1["shift"], f1["shift_err"]
    # block output
    r = c + fc["shift"] + sv + sh_1
    mag = c.abs() + fc["shift"].abs() + sv.abs() + sh_1.abs()
    err = (EPS_OUT * mag if rounded else 0.0) + sc + ss + fc["shift_err"] + sh_1_err
    y, sy = store(r, err, relu=True, **kw)
    v = torch.relu(r)
    shape = (B, T, Ho, Wo, Co)
    rel = storage_eps(bf16)
    return dict(y=y.view(shape), slack=sy.view(shape), v=v.view(shape), err=err.view(shape),
                bound=(rel * (v.abs() + err) + err).view(shape), a=a, b=b, c=c.view(shape), gate=gate_ref, gate_err=gate_ref_err)


def stage(x, blocks, eps, bf16, slack_x=None, rounded=True, widen=False, tamper=None):
    """The blocks in turn, the slack carried from one to the next; the last block's dict.  tamper: the negative controls of
    `block`, for block number tamper["block"] (default 0).
    The propagated bound is a worst case without cancellation: an SE block multiplies it by about 200 (the gate's two FC
    layers), so beyond one block it says little; tests/test_folded_parity_gpu.py judges the blocks of a chain one by one,
    each on the input the device itself stored."""
    tamper = tamper or {}
    cur, sl = x, torch.zeros_like(x) if slack_x is None else slack_x
    out = None
    for i, p in enumerate(blocks):
        out = block(cur, sl, p, eps, bf16, rounded, widen, tamper if tamper.get("block", 0) == i else None)
        cur, sl = out["y"], out["slack"]
    return out


def ratio(dev, ref, bound):
    """|dev - ref| / bound per element; an error where the bound is 0 and any non-finite device value are inf."""
    err = (dev - ref).abs()
    r = torch.where(err > 0, err / bound, torch.zeros_like(err))
    return torch.where(torch.isfinite(dev), r, torch.full_like(r, float("inf")))
