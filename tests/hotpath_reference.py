"""Float64 restatements of the operations behind the bf16-only training kernels (depthwise 3x3x3 forward / backward, the
cooperative pointwise forward GEMMs, the pointwise data gradients and the weight-gradient operand forms): plain torch on
the CPU, nothing imported from the package, the oracle or the reference tree.  tests/test_hotpath_reference_cpu.py pins
every function here against torch.autograd through F.conv3d / F.batch_norm in float64; tests/test_hotpath_bf16_gpu.py
compares the kernels with them, tests/test_bn_se_gpu.py the BatchNorm / SqueezeExcitation finalize and coefficient kernels
(se_case / se_bn_bwd at the end of this file).

Conventions.  Activations are the bf16-quantised values the device gets, as float64, in the repository's channels-last
layouts ([T,H,W,C] per sample for the depthwise functions, [rows, C] for the pointwise ones) WITHOUT padding channels;
parameters are the f32 values the device gets, as float64.  Beside every result comes what a per-element error bound
needs: the magnitude sum  sum |term|  of the same sum, and -- where the kernel rounds a converted operand to bf16 before
the matrix cores -- the slack of operands that sit so close to a bf16 rounding boundary that f32 arithmetic may round
them the other way than float64 does (`round_bf16(x, err)`).

The depthwise functions work on ONE sample (a 32 x 3 x 256 x 256 x 54 clip is 5.4 GB in float64); callers loop.
"""
import torch
import torch.nn.functional as F

BF16_EPS = 2.0 ** -8     # one bf16 rounding (8 significant bits): half an ulp is at most 2^-8 of the value, just above a power of two


def round_bf16(x, err=None):
    """Round-to-nearest-even to 8 significant bits, directly from float64 (no intermediate f32 rounding).  With `err`
    (absolute error of the f32 value the device rounds, same shape): also returns, per element, one bf16 ulp where a
    rounding boundary lies within `err` of x (the device may legitimately land on the neighbouring bf16 value), else 0."""
    m, e = torch.frexp(x)
    s = m * 256.0
    r = torch.ldexp(torch.round(s) / 256.0, e)
    if err is None:
        return r
    ulp = torch.ldexp(torch.ones_like(x), e - 8)
    near = ((s - torch.floor(s) - 0.5).abs() * ulp) <= err
    return r, torch.where(near, ulp, torch.zeros_like(x))


# ------------------------------------------------------------------------------------------------ depthwise 3x3x3
# weight [C][27], tap k = (kt * 3 + ky) * 3 + kx (nn.Conv3d's [C,1,3,3,3] flattened), padding 1, stride (1, s, s)
def _taps():
    return [(kt, ky, kx) for kt in range(3) for ky in range(3) for kx in range(3)]


def dw_out_hw(H, W, stride):
    return (H - 1) // stride + 1, (W - 1) // stride + 1


def dw_fwd_sample(a, scale, shift, w, stride, round_operand=False):
    """One sample.  a [T,H,W,C] (raw conv_a output), x = relu(a * scale + shift), y = depthwise conv of x.
    Returns y, mag = sum_k |x_k| |w_k|, slack (all [T,Ho,Wo,C]).  round_operand: x is rounded to bf16 before the taps, as
    csrc/dw_conv.hip's first kernel does (dw_fwd_kernel<bf16, ...> keeps its activated tile in LDS as bf16, LdsStore<bf16_t>;
    the v2 kernels keep f32); slack is then the ulp of operands that may round the other way, times |w| (else zero)."""
    T, H, W, C = a.shape
    Ho, Wo = dw_out_hw(H, W, stride)
    x = torch.relu(a * scale + shift)
    xs = torch.zeros_like(x)
    if round_operand:
        x, xs = round_bf16(x, 2.0 ** -24 * ((a * scale).abs() + shift.abs()))
    xp, xsp = F.pad(x, (0, 0, 1, 1, 1, 1, 1, 1)), F.pad(xs, (0, 0, 1, 1, 1, 1, 1, 1))
    y = torch.zeros(T, Ho, Wo, C, dtype=a.dtype)
    mag, slack = torch.zeros_like(y), torch.zeros_like(y)
    for k, (kt, ky, kx) in enumerate(_taps()):
        sl = (slice(kt, kt + T), slice(ky, ky + stride * Ho, stride), slice(kx, kx + stride * Wo, stride))
        term = xp[sl] * w[:, k]
        y += term
        mag += term.abs()
        if round_operand:
            slack += xsp[sl] * w[:, k].abs()
    return y, mag, slack


def sample_sums(y):
    """Per-(sample, channel) statistics the forward leaves in nc [B][Cp][2]: (sum, sum of squares) of the STORED output
    of one sample, y [T,Ho,Wo,C] -> [C][2]; second result: the magnitude sums (sum |y|, sum y^2)."""
    s = torch.stack([y.sum((0, 1, 2)), (y * y).sum((0, 1, 2))], 1)
    return s, torch.stack([y.abs().sum((0, 1, 2)), (y * y).sum((0, 1, 2))], 1)


def dw_bwd_sample(t1, b, cA, cB_n, cC, w, a, scale, shift, stride):
    """One sample of c3d_dw333_bwd_fused.  db = cA t1 + cB[n] + cC b  ([T,Ho,Wo,C]); x = relu(a scale + shift);
    t2 = (d conv / d x)(db) * (a scale + shift > 0)  [T,H,W,C];  dW[c][k] = sum db * x(shifted by tap k).
    Returns t2, t2_mag, dW, dW_mag; the magnitudes carry |cA t1| + |cB| + |cC b| in the place of |db| (the three products
    are rounded before they cancel)."""
    T, H, W, C = a.shape
    Ho, Wo = dw_out_hw(H, W, stride)
    db = cA * t1 + cB_n + cC * b
    dbm = (cA * t1).abs() + cB_n.abs() + (cC * b).abs()
    pre = a * scale + shift
    xp = F.pad(torch.relu(pre), (0, 0, 1, 1, 1, 1, 1, 1))
    g = torch.zeros(T + 2, H + 2, W + 2, C, dtype=a.dtype)
    gm = torch.zeros_like(g)
    dw = torch.zeros(C, 27, dtype=a.dtype)
    dwm = torch.zeros_like(dw)
    for k, (kt, ky, kx) in enumerate(_taps()):
        sl = (slice(kt, kt + T), slice(ky, ky + stride * Ho, stride), slice(kx, kx + stride * Wo, stride))
        g[sl] += db * w[:, k]
        gm[sl] += dbm * w[:, k].abs()
        xs = xp[sl]
        dw[:, k] = (db * xs).sum((0, 1, 2))
        dwm[:, k] = (dbm * xs).sum((0, 1, 2))
    mask = (pre > 0).to(a.dtype)
    return g[1:-1, 1:-1, 1:-1] * mask, gm[1:-1, 1:-1, 1:-1] * mask, dw, dwm


def bn_a_bwd_sums(t2, a, mean, rstd):
    """BatchNorm_a-backward sums of one sample over the STORED data gradient t2: (sum t2, sum t2 * ahat), ahat = (a - mean)
    * rstd -> [2][C], and their magnitude sums."""
    ah = (a - mean) * rstd
    ahm = (a.abs() + mean.abs()) * rstd.abs()
    return (torch.stack([t2.sum((0, 1, 2)), (t2 * ah).sum((0, 1, 2))]),
            torch.stack([t2.abs().sum((0, 1, 2)), (t2.abs() * ahm).sum((0, 1, 2))]))


# f32 roundings in front of a depthwise output (27 fma + the operand's) and of a dW entry (a lane's chain along its walk, the
# workgroup tree, the f32 atomics); derived in tests/test_hotpath_bf16_gpu.py
EPS_DW, EPS_DW_DW = 2.0 ** -19, 2.0 ** -13


def dw_pair_ratios(a, scale, shift, w, stride, t1, b, cA, cB, cC, y_dev=None, t2_dev=None, dw_dev=None, round_operand=False):
    """The bf16 depthwise pair against the restatements above, whole batch (a [B,T,H,W,C], cB [B][C], everything float64 on the
    CPU): worst |dev - ref| / (2^-8 (|ref| + E) + E), E = eps sum|term| + slack, over the elements of each given device result (dW without the
    2^-8 term: it is an f32 sum).  b is the tensor the backward was handed."""
    out = {}
    dw, dwm = torch.zeros_like(w), torch.zeros_like(w)

    def worst(key, dev, ref, lim):
        err = (dev - ref).abs()
        r = torch.where(err > 0, err / lim, torch.zeros_like(err))      # (an error where the bound is 0 is inf)
        r = torch.where(torch.isfinite(dev), r, torch.full_like(r, float("inf")))
        out[key] = max(out.get(key, 0.0), float(r.max()))

    for n in range(a.shape[0]):
        if y_dev is not None:
            y, mag, slack = dw_fwd_sample(a[n], scale, shift, w, stride, round_operand)
            e = EPS_DW * mag + slack
            worst("y", y_dev[n], y, BF16_EPS * (y.abs() + e) + e)
        if t2_dev is not None or dw_dev is not None:
            t2, t2m, d, dm = dw_bwd_sample(t1[n], b[n], cA, cB[n], cC, w, a[n], scale, shift, stride)
            dw += d
            dwm += dm
            if t2_dev is not None:
                worst("t2", t2_dev[n], t2, BF16_EPS * (t2.abs() + EPS_DW * t2m) + EPS_DW * t2m)
    if dw_dev is not None:
        worst("dW", dw_dev, dw, EPS_DW_DW * dwm)
    return out


# ------------------------------------------------------------------------------------------------ BatchNorm / SE pieces
def bn_from_sums(s1, s2, count, gamma, beta, eps, running_mean=None, running_var=None, momentum=0.1):
    """Training-mode BatchNorm from completed sums (csrc/bn_fin.h bn_consume): scale, shift, mean, rstd and the updated running
    statistics (biased variance for the normalisation, unbiased for running_var)."""
    mean = s1 / count
    var = (s2 / count - mean * mean).clamp_min(0)
    rstd = 1.0 / torch.sqrt(var + eps)
    scale = gamma * rstd
    out = dict(scale=scale, shift=beta - mean * scale, mean=mean, rstd=rstd)
    if running_mean is not None:
        unb = var * count / (count - 1) if count > 1 else var
        out["running_mean"] = (1 - momentum) * running_mean + momentum * mean
        out["running_var"] = (1 - momentum) * running_var + momentum * unb
    return out


def se_gate(nc_sum, rows_per_sample, scale, shift, w1, b1, w2, b2):
    """SqueezeExcitation gate from the per-sample sums nc_sum [B][C] of the raw conv_b output: pooled = scale * mean_n + shift
    (the mean of bn_b over the sample), hid = relu(W1 pooled + b1) [B][Cr], gate = sigmoid(W2 hid + b2) [B][C].  Third
    result: the magnitude sums of the two pre-activations (hid_mag [B][Cr], gate_mag [B][C], the latter with the hidden
    units' own magnitude carried through |W2|)."""
    z = scale * (nc_sum / rows_per_sample) + shift
    zm = (scale * (nc_sum / rows_per_sample)).abs() + shift.abs()
    hid = torch.relu(z @ w1.t() + b1)
    hm = zm @ w1.abs().t() + b1.abs()
    return torch.sigmoid(hid @ w2.t() + b2), hid, dict(hid_mag=hm, gate_mag=hm @ w2.abs().t() + b2.abs())


def swish(q):
    return q * torch.sigmoid(q)


def gemm_with_bound(P, slack, W):
    """P [M][K] (already rounded where the kernel rounds), W [N][K] (bf16-rounded weights): P W^T, |P| |W|^T and slack |W|^T."""
    Wa = W.abs().t()
    return P @ W.t(), P.abs() @ Wa, slack @ Wa


def col_stats(y):
    """BatchNorm statistics epilogue over STORED rows y [M][N]: [2][N] (sum, sum of squares) and magnitudes."""
    return torch.stack([y.sum(0), (y * y).sum(0)]), torch.stack([y.abs().sum(0), (y * y).sum(0)])


# ------------------------------------------------------------------------------------------------ pointwise forms
# Where the kernels round: csrc/pw_cfwd.hip CF_CONVERT stores the converted operand of a tile to LDS as bf16
# (Vec8<bf16_t>::store for conv_c, pack_bf16x2 for conv_a, whose rounded y is ALSO what pro_out receives);
# c3d_pw_pack_weights rounds the weights to bf16 once; the matrix cores accumulate in f32; the result is rounded to bf16 on
# store and the statistics are taken over the rounded values.  csrc/pw_cdgrad.hip and csrc/pw_wgrad_v2.hip round both
# converted operands of their products to bf16 the same way.
def swish_operand(x, scale, shift, gate_rows=None, rounded=True):
    """conv_c's operand: swish(gate * (x * scale + shift)) [rows][K]; gate_rows [rows][K] or None (no SE).  Returns P, slack.
    f32 error of the value before rounding: 2^-22 of |gate| (|x scale| + |shift|) through the slope of swish (< 1.1) plus 2^-17
    of the result (v_exp_f32 and v_rcp_f32 are 1 ulp each, the exponent's argument error scales with |q|, the f32 gate itself is
    good to 2^-18)."""
    pre = x * scale + shift
    prem = (x * scale).abs() + shift.abs()
    if gate_rows is not None:
        pre, prem = pre * gate_rows, prem * gate_rows.abs()
    p = swish(pre)
    if not rounded:
        return p, torch.zeros_like(p)
    return round_bf16(p, 2.0 ** -22 * prem + 2.0 ** -17 * p.abs())


def conv_c_fwd(b_rows, nc, rows_per_sample, gamma, beta, eps, w, se=None, rounded=True, running=None, momentum=0.1,
               keep_operand=False):
    """conv_c forward as the stage driver issues it (C3D_PRO_BN_SE_SWISH + C3D_EPI_STATS, BatchNorm_b and the SE gate rebuilt
    from the per-sample sums).  b_rows [M][K] raw conv_b output, nc [B][K][2] per-sample sums, w [N][K], se = (w1, b1, w2,
    b2) or None, running = (running_mean, running_var) or None.  Returns a dict: y, mag, slack [M][N] (unrounded y), bn
    (scale / shift / mean / rstd / running), gate [B][K], hid, se_mag; the rows are processed sample by sample."""
    M, K = b_rows.shape
    B = nc.shape[0]
    tot = nc.sum(0)
    rm, rv = running if running is not None else (None, None)
    bn = bn_from_sums(tot[:, 0], tot[:, 1], float(M), gamma, beta, eps, rm, rv, momentum)
    gate = hid = se_mag = None
    if se is not None:
        gate, hid, se_mag = se_gate(nc[:, :, 0], float(rows_per_sample), bn["scale"], bn["shift"], *se)
    Wr = round_bf16(w) if rounded else w
    ys, mags, slacks, Ps = [], [], [], []
    for n in range(B):
        rows = b_rows[n * rows_per_sample:min(M, (n + 1) * rows_per_sample)]
        P, slack = swish_operand(rows, bn["scale"], bn["shift"], None if gate is None else gate[n], rounded)
        y, mag, sl = gemm_with_bound(P, slack, Wr)
        ys.append(y), mags.append(mag), slacks.append(sl)
        if keep_operand:
            Ps.append(P)
    return dict(y=torch.cat(ys), mag=torch.cat(mags), slack=torch.cat(slacks), bn=bn, gate=gate, hid=hid, se_mag=se_mag,
                P=torch.cat(Ps) if keep_operand else None)


def conv_a_fwd(c_rows, sc_rows, sums_c, gamma, beta, eps, w, rounded=True, running=None, momentum=0.1):
    """conv_a forward with the previous block's residual add in its prologue (C3D_PRO_AFFINE2 + pro_out + C3D_EPI_STATS):
    pro_out = relu(bn_c(c) + shortcut) (stored, bf16), y = pro_out W^T.  sums_c [2][K]: completed BatchNorm_c sums of c_rows.
    Returns a dict: po, po_mag (unrounded residual output and |c scale| + |shift| + |shortcut|), y, mag, slack, bn."""
    M, K = c_rows.shape
    rm, rv = running if running is not None else (None, None)
    bn = bn_from_sums(sums_c[0], sums_c[1], float(M), gamma, beta, eps, rm, rv, momentum)
    Wr = round_bf16(w) if rounded else w
    pos, poms, ys, mags, slacks = [], [], [], [], []
    for r0 in range(0, M, 1 << 16):
        cr, sr = c_rows[r0:r0 + (1 << 16)], sc_rows[r0:r0 + (1 << 16)]
        po = torch.relu(cr * bn["scale"] + bn["shift"] + sr)
        pom = (cr * bn["scale"]).abs() + bn["shift"].abs() + sr.abs()
        P, slack = round_bf16(po, 2.0 ** -22 * pom) if rounded else (po, torch.zeros_like(po))
        y, mag, sl = gemm_with_bound(P, slack, Wr)
        pos.append(po), poms.append(pom), ys.append(y), mags.append(mag), slacks.append(sl)
    return dict(po=torch.cat(pos), po_mag=torch.cat(poms), y=torch.cat(ys), mag=torch.cat(mags), slack=torch.cat(slacks), bn=bn)


def affine2_operand(g, x2, A, Bc, Cc, rounded=True):
    """C3D_PRO_AFFINE2: A g + B + C x2 (a BatchNorm backward applied on load), bf16-rounded for the matrix cores."""
    p = A * g + Bc + Cc * x2
    pm = (A * g).abs() + Bc.abs() + (Cc * x2).abs()
    if not rounded:
        return p, torch.zeros_like(p)
    return round_bf16(p, 2.0 ** -22 * pm)


def staged_product(P, slack, Wr, eps, rounded=True):
    """P Wr as csrc/pw_cdgrad.hip hands it to its epilogue: the f32 result tile is staged in LDS as bf16 (CD_EPI / CC_EPI read
    `Os`, written with pack_bf16x2), so the product itself is rounded once before the epilogue's arithmetic.  Returns the
    (rounded) product and the absolute error the device's value may have: f32 accumulation (eps |P| |W|), operands that may
    round the other way (slack |W|) and one bf16 ulp where the product lies that close to a rounding boundary."""
    r, mag, sl = P @ Wr, P.abs() @ Wr.abs(), slack @ Wr.abs()
    err = eps * mag + sl
    if not rounded:
        return r, err
    rb, tie = round_bf16(r, err)
    return rb, err + tie


def conv_a_dgrad(g, a, coef, w, res, y_prev=None, eps=2.0 ** -16, rounded=True):
    """conv_a data gradient (C3D_PRO_AFFINE2 + C3D_EPI_ADD, C3D_WG_ROWS): P = A g + B + C a (BatchNorm_a backward on load,
    [M][Ci]); dx = P W + res with W [Ci][Cin] the conv weight; with y_prev (the block's input, a ReLU output) the stored
    gradient is dx (y_prev > 0) -- the previous block's ReLU mask (wg_mask_out).  dW = P^T y_prev is the caller's (wgrad).
    Returns a dict: dx, err (absolute error of the value the kernel rounds on store), P, P_slack."""
    P, ps = affine2_operand(g, a, *coef, rounded=rounded)
    r, err = staged_product(P, ps, round_bf16(w) if rounded else w, eps, rounded)
    dx, err = r + res, err + 2.0 ** -24 * (r.abs() + res.abs())
    if y_prev is not None:
        m = (y_prev > 0).to(dx.dtype)
        dx, err = dx * m, err * m
    return dict(dx=dx, err=err, P=P, P_slack=ps)


def bn_bwd_sums(gstored, x, mean, rstd):
    """(sum g, sum g xhat) over rows, xhat = (x - mean) rstd: [2][N], and the magnitude sums."""
    xh, xm = (x - mean) * rstd, (x.abs() + mean.abs()) * rstd.abs()
    return torch.stack([gstored.sum(0), (gstored * xh).sum(0)]), torch.stack([gstored.abs().sum(0), (gstored.abs() * xm).sum(0)])


def swish_grad(q):
    s = torch.sigmoid(q)
    return s * (1 + q * (1 - s))


def conv_c_dgrad(g, c, coef, w, b_rows, scale, shift, gate_row=None, eps=2.0 ** -16, rounded=True):
    """conv_c data gradient of ONE sample's rows (C3D_PRO_AFFINE2 + C3D_EPI_SWISH_SE_BWD, C3D_WG_SWISH): P = A g + B + C c
    [M][Co]; d = P W (W [Co][Ci], the gradient at the Swish output); pb = b scale + shift, q = gate pb;
    dq = d swish'(q); t1 = dq gate (stored); the per-sample sums are (sum dq pb [d gate], sum t1, sum t1 bhat), the last
    two over the STORED t1 (bn_bwd_sums).  gate_row [Ci] or None (a block without SqueezeExcitation: gate 1).
    Returns a dict: t1, err, dgate [Ci] with dgate_err, P, P_slack, and the forward operand Q = swish(q) (bf16) with Q_slack
    for dW = P^T Q."""
    P, ps = affine2_operand(g, c, *coef, rounded=rounded)
    d, err = staged_product(P, ps, round_bf16(w) if rounded else w, eps, rounded)
    gate = torch.ones_like(scale) if gate_row is None else gate_row
    pb = b_rows * scale + shift
    sp = swish_grad(gate * pb)
    dq = d * sp
    # swish'(q) = sg (1 + q (1 - sg)) crosses zero at q = -1.278: its error is absolute there.  sg = v_rcp(1 + v_exp(-q log2 e)) is
    # good to (2 + |q|) 2^-23 of itself (1 ulp each, the exponent's argument rounded once), the derivative's slope in sg is
    # 1 + q (1 - 2 sg), four more roundings in the polynomial: (1 + |q|)(3 + |q|) 2^-23 sg <= (1 + |q|)^2 2^-21 sg
    aq = (gate * pb).abs()
    dq_err = err * sp.abs() + d.abs() * 2.0 ** -21 * (1 + aq) ** 2 * torch.sigmoid(gate * pb)
    Q, qs = swish_operand(b_rows, scale, shift, gate_row, rounded)
    return dict(t1=dq * gate, err=dq_err * gate.abs() + 2.0 ** -24 * (dq * gate).abs(),
                dgate=(dq * pb).sum(0), dgate_err=(dq_err * pb.abs() + 2.0 ** -22 * dq.abs() * ((b_rows * scale).abs() + shift.abs())).sum(0),
                dgate_mag=(dq * pb).abs().sum(0), P=P, P_slack=ps, Q=Q, Q_slack=qs)


def wgrad(P, Q):
    """c3d_pw_wgrad: dW [N][K] = P^T Q over the rows, with its magnitude sum."""
    return P.t() @ Q, P.abs().t() @ Q.abs()


# ------------------------------------------------------------------------------------------------ BatchNorm_b / SE backward
# The middle of a residual block, from its definition: pb = bn_b(b) (batch statistics over all B * R rows), z = the mean of pb
# over a sample's rows, hid = relu(W1 z + b1), gate = sigmoid(W2 hid + b2), q = gate pb, Swish(q) goes on to conv_c.  With d
# the gradient at the Swish output, conv_c's data-gradient epilogue leaves dq = d swish'(q), t1 = dq gate and, per (sample,
# channel), nc3 = (sum dq pb [the gradient at the gate], sum t1, sum t1 bhat), bhat = (b - mean) rstd; the depthwise forward
# left ncf = (sum b, sum b^2).  c3d_se_bn_bwd_coef (csrc/bn_se.hip) turns those O(B C) numbers into the SE parameter gradients
# and into db = A t1 + B[n] + C b, the gradient at b, applied on operand load by the depthwise backward.
def se_case(B, R, C, Cr, seed, se=True, eps=1e-5):
    """A small block middle in float64: b [B][R][C] (conv_b output), d (gradient at the Swish output), gamma, beta and the four
    SE tensors (se = (w1 [Cr][C], b1, w2 [C][Cr], b2); parameters are f32-representable, as the device gets them), and -- from
    the definition above, nothing taken from the kernels -- ncf [B][C][2], nc3 [B][C][3], mean, rstd, scale, shift, gate [B][C],
    hid [B][Cr] and t1 [B][R][C].  se=False: a block without SqueezeExcitation (gate 1; se, gate and hid are None)."""
    g = torch.Generator().manual_seed(seed)

    def rn(shape, scale=1.0):
        return (torch.randn(shape, generator=g, dtype=torch.float32) * scale).double()

    def f32(t):
        return t.float().double()

    b = rn((B, R, C)) * (rn((C,)).abs() + 0.5) + rn((C,), 0.5) + rn((B, 1, C), 0.3)     # per-sample means differ: the gate does too
    d = rn((B, R, C))
    gamma, beta = f32(rn((C,)).abs() + 0.5), rn((C,), 0.3)
    mean = b.mean((0, 1))
    var = ((b - mean) ** 2).mean((0, 1))
    rstd = 1.0 / torch.sqrt(var + eps)
    scale = gamma * rstd
    shift = beta - mean * scale
    pb = (b - mean) * rstd * gamma + beta
    out = dict(B=B, R=R, C=C, Cr=Cr, eps=eps, b=b, d=d, gamma=gamma, beta=beta, mean=mean, rstd=rstd, scale=scale, shift=shift,
               ncf=torch.stack([b.sum(1), (b * b).sum(1)], 2), se=None, gate=None, hid=None)
    gate_rows = torch.ones_like(pb)
    if se:
        w1, b1 = rn((Cr, C), 2.0 / C ** 0.5), rn((Cr,), 0.3)
        w2, b2 = rn((C, Cr), 1.0 / Cr ** 0.5), rn((C,), 0.3)
        hid = torch.relu(pb.mean(1) @ w1.t() + b1)
        gate = torch.sigmoid(hid @ w2.t() + b2)
        out.update(se=(w1, b1, w2, b2), gate=gate, hid=hid)
        gate_rows = gate[:, None, :].expand_as(pb)
    dq = d * swish_grad(gate_rows * pb)
    t1 = dq * gate_rows
    bhat = (b - mean) * rstd
    out.update(t1=t1, nc3=torch.stack([(dq * pb).sum(1), t1.sum(1), (t1 * bhat).sum(1)], 2))
    return out


def se_bn_bwd(nc3, ncf, R, gamma, mean, rstd, scale, shift, se=None, gate=None, hid=None):
    """SE backward + BatchNorm_b backward coefficients from the per-sample sums, every argument as the kernel gets it (float64 of
    its f32 inputs): nc3 [B][C][3], ncf [B][C][2], R rows per sample, se = (w1, b1, w2, b2) or None, gate [B][C], hid [B][Cr].
        du = nc3_0 gate (1 - gate)                 gradient at the gate's pre-activation
        dh = (hid > 0) du W2                       hid is the SUPPLIED one: no mask can flip between device and reference
        dz = dh W1                                 gradient at z, spread evenly over the sample's R rows of pb
        dW2 = du^T hid, db2 = sum_n du, dW1 = dh^T z, db1 = sum_n dh,  z = scale ncf_0 / R + shift
        s1 = sum_n (nc3_1 + dz), s2 = sum_n (nc3_2 + dz / R * rstd (ncf_0 - R mean))       = (d beta, d gamma)
        A = gamma rstd, C = -A rstd s2 / (B R), B[n] = A dz[n] / R - A s1 / (B R) - C mean
    Returns a dict name -> (value, mag, err) for coefA [C], coefB [B][C], coefC [C], dgamma, dbeta, dw1 [Cr][C], db1, dw2 [C][Cr],
    db2 (the SE gradients only with se): mag is the magnitude sum of the LAST sum in front of the value (what an eps per rounding
    of that sum multiplies), err the absolute error its inputs bring along when the chain in front is done in f32 the way
    csrc/bn_se.hip does it -- err(du) 4 u |du| (one conversion, 1 - gate, two products), err(z) 2 u (|scale m| + |shift|), err(dh)
    through the ceil(C / 8)-step chains and their three-level tree, err(dz) through the Cr-step chain -- carried into coefB, s1, s2
    the way conv_c_dgrad carries `err`.  Without se, coefB is the same for every sample."""
    u = 1.001 * 2.0 ** -24        # (1.001: the second-order terms of chains of up to ~100 roundings)
    B, C = nc3.shape[0], nc3.shape[1]
    count = float(B) * R
    zero = torch.zeros(B, C, dtype=nc3.dtype)
    dz, dz_err = zero, zero
    out = {}
    if se is not None:
        w1, _, w2, _ = se
        Cr = w1.shape[0]
        du = nc3[:, :, 0] * gate * (1 - gate)
        du_err = 4 * u * du.abs()
        m = ncf[:, :, 0] / R
        z = scale * m + shift
        z_mag = (scale * m).abs() + shift.abs()
        z_err = 2 * u * z_mag
        mask = (hid > 0).to(nc3.dtype)
        dh = (du @ w2) * mask
        dh_mag = (du.abs() @ w2.abs()) * mask
        dh_err = ((C + 7) // 8 + 3) * u * dh_mag + (du_err @ w2.abs()) * mask
        dz = dh @ w1
        dz_mag = dh.abs() @ w1.abs()
        dz_err = Cr * u * dz_mag + dh_err @ w1.abs()
        out["dw2"] = (du.t() @ hid, du.abs().t() @ hid.abs(), du_err.t() @ hid.abs())
        out["db2"] = (du.sum(0), du.abs().sum(0), du_err.sum(0))
        out["dw1"] = (dh.t() @ z, dh.abs().t() @ z.abs(), dh_err.t() @ z.abs() + dh.abs().t() @ z_err)
        out["db1"] = (dh.sum(0), dh.abs().sum(0), dh_err.sum(0))
    sb = rstd * (ncf[:, :, 0] / R - mean)            # (sum of bhat over the sample's rows) / R
    s1 = (nc3[:, :, 1] + dz).sum(0)
    s1_mag, s1_err = (nc3[:, :, 1].abs() + dz.abs()).sum(0), dz_err.sum(0)
    s2 = (nc3[:, :, 2] + dz * sb).sum(0)
    s2_mag, s2_err = (nc3[:, :, 2].abs() + (dz * sb).abs()).sum(0), (dz_err * sb.abs()).sum(0)
    A = gamma * rstd
    k = A * rstd / count
    Cc, Cc_mag, Cc_err = -k * s2, k.abs() * s2_mag, k.abs() * s2_err
    Bn = A * dz / R - A * s1 / count - Cc * mean
    Bn_mag = (A * dz / R).abs() + (A / count).abs() * s1_mag + Cc_mag * mean.abs()
    Bn_err = A.abs() / R * dz_err + (A / count).abs() * s1_err + Cc_err * mean.abs()
    out.update(coefA=(A, A.abs(), torch.zeros_like(A)), coefB=(Bn, Bn_mag, Bn_err), coefC=(Cc, Cc_mag, Cc_err),
               dgamma=(s2, s2_mag, s2_err), dbeta=(s1, s1_mag, s1_err))
    return out
