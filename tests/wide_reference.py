"""Float64 restatements of everything csrc/pw_wide.hip computes (pw_wide_kernel<T, PRO, EPI>, pw_wide_wgrad_kernel<T>): plain
torch on the CPU, nothing imported from the package.  tests/test_wide_reference_cpu.py pins every function here against
float64 torch.autograd with the rounding steps switched off; tests/test_wide_parity_gpu.py compares the kernels with them.
The arithmetic shared with the narrow kernels comes from tests/hotpath_reference.py (round_bf16 with its near-boundary marks,
gemm_with_bound, swish_operand, affine2_operand, col_stats, wgrad, swish_grad, bn_bwd_sums).

Conventions as there: activations are the storage-type values the device gets, as float64, [rows][C] without padding
channels; parameters are the f32 values the device gets, as float64.  `bf16` says which storage type the kernel was built
for.  Beside every result comes the magnitude sum of its sum and the absolute error (`slack`) its operands bring along.

Where the wide kernels differ from the narrow ones (read off csrc/pw_wide.hip):
  * operands: Mma<bf16>::store8 / cvt round the converted X operand AND the f32 weights to bf16 in the kernel (weights need
    not be bf16 values); Mma<float> keeps f32 and multiplies with the f32 matrix instruction -- nothing is rounded before the
    products, the operand's own f32 error is what `slack` carries.
  * the block result reaches the epilogue through an f32 LDS tile: no bf16 staging rounding (hotpath_reference.staged_product
    does not apply).
  * bias is added to the f32 result before the epilogue.
  * STATS sums the value as stored (round_as<T>); SWISH_SE_BWD: s0 sums dq * pb unrounded, s1 and s2 use the stored t.
  * the AFFINE2 coefficients may be rebuilt in the kernel from completed BatchNorm-backward sums (csrc/bn_fin.h
    bn_bwd_coef_consume): float64 arithmetic, each coefficient rounded to f32 once.
"""
import torch

import hotpath_reference as R

U = 2.0 ** -24


def f32(t):
    """Round float64 to f32 once (kept as float64)."""
    return t.float().double()


def operand(p, err, bf16, rounded=True):
    """The value the matrix cores get for a converted operand whose exact value is p and whose f32 value is within err of it.
    bf16: rounded, slack = one ulp where a rounding boundary lies within err; f32: as computed, slack = err."""
    if not rounded:
        return p, torch.zeros_like(p)
    if bf16:
        return R.round_bf16(p, err)
    return p, err


def weights(w, bf16, rounded=True):
    return R.round_bf16(w) if (bf16 and rounded) else w


# ------------------------------------------------------------------------------------------------ prologues
def pro_none(x):
    return x, torch.zeros_like(x)


def pro_swish(x, scale, shift, gate_rows, bf16, rounded=True):
    """C3D_PRO_BN_SE_SWISH: q = gate * fma(x, scale, shift), operand q sigmoid(q); gate_rows [rows][K] or None.  The error of the
    f32 value is hotpath_reference.swish_operand's (2^-22 of the pre-activation's magnitude, 2^-17 of the result)."""
    if bf16 or not rounded:
        return R.swish_operand(x, scale, shift, gate_rows, rounded)
    p, _ = R.swish_operand(x, scale, shift, gate_rows, False)
    prem = (x * scale).abs() + shift.abs()
    if gate_rows is not None:
        prem = prem * gate_rows.abs()
    return p, 2.0 ** -22 * prem + 2.0 ** -17 * p.abs()


def pro_affine2(g, x2, A, Bc, Cc, bf16, rounded=True):
    """C3D_PRO_AFFINE2: fma(A, g, fma(C, x2, B))."""
    if bf16 or not rounded:
        return R.affine2_operand(g, x2, A, Bc, Cc, rounded)
    p, _ = R.affine2_operand(g, x2, A, Bc, Cc, False)
    return p, 2.0 ** -22 * ((A * g).abs() + Bc.abs() + (Cc * x2).abs())


def gather_stride2(x, BT, H, W):
    """C3D_ROWS_STRIDE2: output row (bt, ho, wo) reads input pixel (bt, 2 ho, 2 wo) of x [BT * H * W][K]."""
    K = x.shape[1]
    return x.view(BT, H, W, K)[:, 0:2 * (H // 2):2, 0:2 * (W // 2):2].reshape(-1, K)


def bn_bwd_coef(sums, gamma, mean, rstd, count, rounded=True):
    """bn_bwd_coef_consume: sums [2][C] = (sum g, sum g xhat) -> A = gamma rstd, C = -A rstd s2 / count, B = -A s1 / count -
    C mean, so that dx = A g + B + C x is the BatchNorm backward.  rounded: each coefficient rounded to f32 once.  Second
    result: the magnitude in front of each coefficient's one rounding ([3][C]); third: (dgamma, dbeta) = (s2, s1)."""
    s1, s2 = sums[0], sums[1]
    A = gamma * rstd
    Cc = -A * rstd * s2 / count
    Bc = -A * s1 / count - Cc * mean
    mag = torch.stack([A.abs(), (A * s1 / count).abs() + (Cc * mean).abs(), Cc.abs()])
    coef = torch.stack([A, Bc, Cc])
    return (f32(coef) if rounded else coef), mag, (s2, s1)


# ------------------------------------------------------------------------------------------------ GEMM + epilogues
def gemm(P, slack, w, bf16, bias=None, rounded=True):
    """P [M][K] (operand as the matrix cores get it), w [N][K] f32 weights: the f32 tile the epilogue reads, P W^T + bias.
    Returns y, mag = |P| |W|^T + |bias|, slack |W|^T."""
    y, mag, sl = R.gemm_with_bound(P, slack, weights(w, bf16, rounded))
    if bias is not None:
        y, mag = y + bias, mag + bias.abs()
    return y, mag, sl


def scatter_even(res, BT, H, W):
    """res_mode 1: res [BT * (H/2) * (W/2)][N] is added where h and w are even -> the dense [BT * H * W][N] addend."""
    N = res.shape[1]
    full = torch.zeros(BT, H, W, N, dtype=res.dtype)
    full[:, 0:2 * (H // 2):2, 0:2 * (W // 2):2] = res.view(BT, H // 2, W // 2, N)
    return full.view(-1, N)


def epi_add(y, mag, res, res_mode=0, BT=0, H=0, W=0):
    """C3D_EPI_ADD: y + res (dense) or + res scattered to the even pixels."""
    full = res if res_mode == 0 else scatter_even(res, BT, H, W)
    return y + full, mag + full.abs()


def stripe_stats(y_stored, block_rows=64, stripes=16):
    """C3D_EPI_STATS of the block-tiled kernel: row block i (64 rows) adds its column sums of the STORED rows into stripe
    i % 16.  Returns sums [16][2][N] and their magnitude sums."""
    M, N = y_stored.shape
    s = torch.zeros(stripes, 2, N, dtype=y_stored.dtype)
    m = torch.zeros_like(s)
    idx = (torch.arange(M) // block_rows) % stripes
    s[:, 0].index_add_(0, idx, y_stored)
    s[:, 1].index_add_(0, idx, y_stored * y_stored)
    m[:, 0].index_add_(0, idx, y_stored.abs())
    m[:, 1].index_add_(0, idx, y_stored * y_stored)
    return s, m


def sample_rows(v, M, rows_per_sample):
    """[B][C] per-sample values -> [M][C] rows (row m belongs to sample m // rows_per_sample; the last sample may be partial)."""
    return v[torch.arange(M) // rows_per_sample]


def sample_sum(t, rows_per_sample):
    """[M][C] -> [B][C] sums over each sample's rows (B = ceil(M / rows_per_sample))."""
    M = t.shape[0]
    B = (M + rows_per_sample - 1) // rows_per_sample
    out = torch.zeros(B, t.shape[1], dtype=t.dtype)
    out.index_add_(0, torch.arange(M) // rows_per_sample, t)
    return out


def epi_swish_se_bwd(d, d_err, b, scale, shift, gate_rows=None):
    """C3D_EPI_SWISH_SE_BWD on the f32 tile d (absolute error d_err): pb = fma(b, scale, shift), q = gate pb,
    dq = d swish'(q), t = dq gate (stored), s0 terms dq pb.  Errors, f32 throughout:
      q      two roundings of |gate| (|b scale| + |shift|): 2^-23 of it (the product does not see the cancellation in pb)
      swish' (1 + |q|)^2 2^-21 sigmoid(q) from the exponential, the reciprocal and four roundings (hotpath_reference
             .conv_c_dgrad), plus |swish''| <= 1/2 times the error of q
      t      one more product
    Returns a dict: t, t_err, s0_term (dq pb), s0_err (per row, absolute), s0_mag."""
    gate = torch.ones_like(b) if gate_rows is None else gate_rows
    prem = (b * scale).abs() + shift.abs()
    pb = b * scale + shift
    q = gate * pb
    q_err = 2.0 ** -23 * gate.abs() * prem
    sp = R.swish_grad(q)
    sp_err = 2.0 ** -21 * (1 + q.abs()) ** 2 * torch.sigmoid(q) + 0.5 * q_err
    dq = d * sp
    dq_err = d_err * (sp.abs() + sp_err) + d.abs() * sp_err
    t = dq * gate
    term = dq * pb
    return dict(t=t, t_err=dq_err * gate.abs() + U * t.abs(), s0_term=term,
                s0_err=dq_err * (pb.abs() + U * prem) + dq.abs() * U * prem, s0_mag=term.abs())


def se_bwd_sums_of_stored(t_stored, b, mean, rstd, rows_per_sample):
    """s1 = sum t, s2 = sum t bhat over each sample's rows of the STORED t, bhat = (b - mean) rstd: [B][N] each, and their
    magnitude sums (|t| and |t| (|b| + |mean|) |rstd|)."""
    bh = (b - mean) * rstd
    bm = (b.abs() + mean.abs()) * rstd.abs()
    return (sample_sum(t_stored, rows_per_sample), sample_sum(t_stored * bh, rows_per_sample),
            sample_sum(t_stored.abs(), rows_per_sample), sample_sum(t_stored.abs() * bm, rows_per_sample))


# ------------------------------------------------------------------------------------------------ weight gradient
def wgrad(P, p_slack, Q, q_slack):
    """pw_wide_wgrad_kernel: dW [N][K] = P^T Q over the rows.  Returns dW, mag = |P|^T |Q| and the slack of both operands."""
    dw, mag = R.wgrad(P, Q)
    sl = p_slack.t() @ (Q.abs() + q_slack) + P.abs().t() @ q_slack
    return dw, mag, sl


def wgrad_plan(M, K, N, cus):
    """launch_wide_wgrad's row split: (rows per split, splits).  64 x 64 blocks of dW, at least 2 workgroups per CU wanted, at
    least 128 rows per split, rows a multiple of the 32-row chunk."""
    Kp, Np = (K + 7) // 8 * 8, (N + 7) // 8 * 8
    blocks = ((Np + 63) // 64) * ((Kp + 63) // 64)
    split = max(1, min((2 * cus + blocks - 1) // blocks, (M + 127) // 128))
    rows = ((M + split - 1) // split + 31) // 32 * 32
    return rows, (M + rows - 1) // rows
