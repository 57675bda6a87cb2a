"""Restatements of the operations in csrc/elementwise.hip (res-block / stem output forward and backward, the BatchNorm-backward
coefficients its ticket tail writes, the pieces of Encoder.enhance, frame_scatter): plain torch on the CPU, nothing imported
from the package, the oracle or the reference tree.  tests/test_elementwise_reference_cpu.py pins every function here against
torch.autograd in float64; tests/test_elementwise_gpu.py compares the kernels with them.

Conventions are those of tests/hotpath_reference.py.  Activations are the bf16-quantised (or f32) values the device gets, as
float64, channels-last ([rows, C] for the block output, [B, T, HW, C] for the enhance pieces) WITHOUT padding channels;
parameters are the f32 values the device gets, as float64.  Beside every result comes the magnitude sum  sum |term|  its
error bound needs.  The enhance pieces and frame_scatter do one operation per element and are written over whatever
floating type they are given: float64 for the autograd pin, float32 where a test wants the device's own IEEE operation.

The launch rule of block_out_bwd_kernel is restated at the end (launch_rule / chain_steps / sums_eps): the bound of the
BatchNorm-backward sums counts the f32 additions of one thread, which is the number of grid strides in the rows.
"""
import math

import torch

from hotpath_reference import round_bf16  # noqa: F401  (callers quantise with it)

U = 2.0 ** -24            # unit roundoff of f32
EPS_FWD = 2.0 ** -22      # block_out_fwd: two fma and one add, 3 u of the magnitude
EPS_COEF = 2.0 ** -21     # f64 -> f32 vectors of the BatchNorm finalize / coefficient kernels (tests/test_hotpath_bf16_gpu.py)


# ------------------------------------------------------------------------------------------------ block output
def block_out_fwd(c, scale_c, shift_c, s=None, scale_1=None, shift_1=None):
    """y = relu(c a + b [+ s a1 + b1]) and mag = |c||a| + |b| (+ |s||a1| + |b1|).  A shortcut without BatchNorm (identity, or a
    convolution without BatchNorm) passes s alone: a1 = 1, b1 = 0."""
    r = c * scale_c + shift_c
    mag = c.abs() * scale_c.abs() + shift_c.abs()
    if s is not None:
        a1 = torch.ones_like(scale_c) if scale_1 is None else scale_1
        b1 = torch.zeros_like(shift_c) if shift_1 is None else shift_1
        r = r + s * a1 + b1
        mag = mag + s.abs() * a1.abs() + b1.abs()
    return torch.relu(r), mag


def _sums(g, x, mean, rstd):
    xh = (x - mean) * rstd
    xm = (x.abs() + mean.abs()) * rstd.abs()
    return torch.stack([g.sum(0), (g * xh).sum(0)]), torch.stack([g.abs().sum(0), (g.abs() * xm).sum(0)])


def block_out_bwd(dy, y, c, mean_c, rstd_c, s=None, mean_1=None, rstd_1=None):
    """g = dy (y > 0); sums_c = (sum g, sum g (c - mean_c) rstd_c) [2][C]; sums_1 the same over the shortcut s when it is
    given; mag_c / mag_1 = (sum |g|, sum |g| (|x| + |mean|) |rstd|)."""
    g = dy * (y > 0).to(dy.dtype)
    out = dict(g=g)
    out["sums_c"], out["mag_c"] = _sums(g, c, mean_c, rstd_c)
    if s is not None:
        out["sums_1"], out["mag_1"] = _sums(g, s, mean_1, rstd_1)
    return out


def bn_bwd_coef(sums, count, gamma, mean, rstd):
    """BatchNorm backward as dx = A g + B + C x from sums = (sum g, sum g xhat):  A = gamma rstd,  C = -A rstd sums[1] / count,
    B = -A sums[0] / count - C mean;  dgamma = sums[1], dbeta = sums[0].  mag: the magnitude of each (B's counts its two
    products separately)."""
    A = gamma * rstd
    Cc = -A * rstd * sums[1] / count
    B = -A * sums[0] / count - Cc * mean
    mag = dict(A=A.abs(), B=(A * sums[0] / count).abs() + (Cc * mean).abs(), C=Cc.abs(), dgamma=sums[1].abs(), dbeta=sums[0].abs())
    return dict(A=A, B=B, C=Cc, dgamma=sums[1], dbeta=sums[0], mag=mag)


# ------------------------------------------------------------------------------------------------ enhance pieces
# y, out, dout, dy: [B, T, HW, C];  d, e, de, dd: [B, HW, C]
def frame_absdiff(y, t_pre, t_post):
    return (y[:, t_pre] - y[:, t_post]).abs()


def enhance_apply(y, e, t_mid):
    out = y.clone()
    out[:, t_mid] = y[:, t_mid] + torch.relu(e)
    return out


def enhance_bwd_mask(dout, e, t_mid):
    return dout[:, t_mid] * (e > 0).to(dout.dtype)


def enhance_bwd_apply(dout, y, dd, t_pre, t_post):
    """dy = dout; dy[:, t_pre] += sign(y_pre - y_post) dd; dy[:, t_post] -= the same (sign(0) = 0).  A frame index outside
    [0, T) matches no frame."""
    T = dout.shape[1]
    dy = dout.clone()
    if not (0 <= t_pre < T and 0 <= t_post < T):
        if 0 <= t_pre < T or 0 <= t_post < T:
            raise ValueError("one frame index in range, one outside: the kernel would read the partner frame out of range")
        return dy
    sd = torch.sign(y[:, t_pre] - y[:, t_post]) * dd
    if t_pre == t_post:         # sign(0) = 0 everywhere
        return dy
    dy[:, t_pre] = dout[:, t_pre] + sd
    dy[:, t_post] = dout[:, t_post] - sd
    return dy


def frame_scatter(src, dst, t_dst, accumulate):
    out = dst.clone()
    out[:, t_dst] = src + dst[:, t_dst] if accumulate else src
    return out


# ------------------------------------------------------------------------------------------------ launch rule
BOB_GRID_CAP, BOB_U = 384, 4         # block_out_bwd_kernel: workgroups at most, rows in flight per thread
FWD_GRID_CAP, FWD_FIN_GRID_CAP = 4096, 1024


def launch_rule(C):
    """Cp, G (8-channel vectors per row), blk (threads: whole rows, 256 at most), rows per workgroup, S (rows in one grid
    stride of the capped backward grid)."""
    Cp = (C + 7) // 8 * 8
    G = Cp // 8
    rows = 256 // G
    return Cp, G, G * rows, rows, BOB_GRID_CAP * rows


def chain_steps(M, C):
    """f32 additions one thread of block_out_bwd_kernel makes into each of its partial sums."""
    _, G, blk, rows, _ = launch_rule(C)
    grid = min((M * G + blk - 1) // blk, BOB_GRID_CAP)
    return (M + grid * rows - 1) // (grid * rows)


def sums_eps(n_max):
    """Smallest power of two >= (n_max + 3) u: a term costs three roundings (the subtraction, times rstd, times g), the
    thread's chain one per step; everything after the thread is f64."""
    return 2.0 ** math.ceil(math.log2((n_max + 3) * U))


def sums_ratio(dev, ref, mag, eps):
    """max |dev - ref| / (eps mag) over the elements (0 where they agree exactly, inf where a bound of 0 is missed)."""
    err, lim = (dev.double() - ref).abs(), eps * mag
    ratio = torch.where(err > 0, err / lim, torch.zeros_like(err))
    ratio = torch.where(torch.isfinite(dev.double()), ratio, torch.full_like(ratio, float("inf")))
    return float(ratio.max())
