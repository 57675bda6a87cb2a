"""Float64 restatements of the ChangeDecoder's transposed convolutions, its 3x3 head and the stem's weight / input gradient,
written from the operations' definitions (shifted slices and matmul; nothing follows a kernel's loop structure): plain torch,
on whatever device the arguments live on (torch.double matmul runs on the GPU, so a multi-tile case takes seconds), nothing
imported from the package.  tests/test_hotpath_reference_cpu.py pins every function here, unrounded, against torch.autograd
in float64; tests/test_decoder_parity_gpu.py compares the kernels with them.

Conventions, as in hotpath_reference.py: activations are the bf16 values the device gets, as float64, channels-last; parameters
are the f32 values the device gets, as float64.  Beside every value comes the magnitude sum  sum |term|  of the same sum, and --
where a kernel rounds a computed operand to bf16 -- the slack of operands within their f32 error of a rounding boundary.

Weight rounding.  The kernels convert f32 weights with f32_to_bf16 (csrc/common.h), which is pack_bf16x2 = clang's
__builtin_convertvector(float2 -> bf16x2): round to nearest, ties to even (v_cvt_pk_bf16_f32 on gfx950), no truncation.
round_bf16 of hotpath_reference.py is that rounding, taken from the float64 copy of the f32 value (exact).
"""
import torch
import torch.nn.functional as F

from hotpath_reference import round_bf16


def _w(w, rounded):
    return round_bf16(w) if rounded else w


# ------------------------------------------------------------------------------------ ConvTranspose2d k4 s2 p1, channels-last
# out[b, 2 iy - 1 + ky, 2 ix - 1 + kx, co] += x[b, iy, ix, ci] W[ci][co][ky][kx]      (nn.ConvTranspose2d weight layout)
def convt4s2_fwd(x, w, bias, skip=None, rounded=True):
    """x [B,h,wd,C], w [C,C,4,4], bias [C], skip [B,2h,2wd,C] or None.  Returns out [B,2h,2wd,C] and its magnitude sum
    (|bias| and |skip| included: the bias starts the accumulator, the skip is added in f32 before the store)."""
    B, h, wd, C = x.shape
    Wr = _w(w, rounded)
    o = torch.zeros(B, 2 * h + 2, 2 * wd + 2, C, dtype=x.dtype, device=x.device)     # row oy + 1, column ox + 1
    m = torch.zeros_like(o)
    xa = x.abs()
    for ky in range(4):
        for kx in range(4):
            sl = (slice(None), slice(ky, ky + 2 * h, 2), slice(kx, kx + 2 * wd, 2))
            o[sl] += x @ Wr[:, :, ky, kx]
            m[sl] += xa @ Wr[:, :, ky, kx].abs()
    o, m = o[:, 1:-1, 1:-1] + bias, m[:, 1:-1, 1:-1] + bias.abs()
    if skip is not None:
        o, m = o + skip, m + skip.abs()
    return o, m


def convt4s2_dgrad(dout, w, rounded=True):
    """dout [B,2h,2wd,C] -> din [B,h,wd,C] = sum_{ky,kx,co} dout[b, 2iy-1+ky, 2ix-1+kx, co] W[ci][co][ky][kx], and its magnitude sum."""
    B, H, W, C = dout.shape
    h, wd = H // 2, W // 2
    Wr = _w(w, rounded)
    dp = F.pad(dout, (0, 0, 1, 1, 1, 1))
    dpa = dp.abs()
    din = torch.zeros(B, h, wd, C, dtype=dout.dtype, device=dout.device)
    mag = torch.zeros_like(din)
    for ky in range(4):
        for kx in range(4):
            sl = (slice(None), slice(ky, ky + 2 * h, 2), slice(kx, kx + 2 * wd, 2))
            din += dp[sl] @ Wr[:, :, ky, kx].t()
            mag += dpa[sl] @ Wr[:, :, ky, kx].abs().t()
    return din, mag


def convt4s2_wgrad(t, dcur):
    """t [B,h,wd,C] (the layer's input), dcur [B,2h,2wd,C] -> dW [C,C,4,4] = sum_{b,i,j} t[b,i,j,ci] dcur[b, 2i-1+ky, 2j-1+kx, co] and its
    magnitude sum.  Both operands are stored bf16 values: nothing is rounded."""
    B, h, wd, C = t.shape
    dp = F.pad(dcur, (0, 0, 1, 1, 1, 1))
    tt = t.reshape(-1, C).t()
    tta = tt.abs()
    dw = torch.zeros(C, C, 4, 4, dtype=t.dtype, device=t.device)
    mag = torch.zeros_like(dw)
    for ky in range(4):
        for kx in range(4):
            d = dp[:, ky:ky + 2 * h:2, kx:kx + 2 * wd:2].reshape(-1, C)
            dw[:, :, ky, kx] = tt @ d
            mag[:, :, ky, kx] = tta @ d.abs()
    return dw, mag


# ------------------------------------------------------------------------------------ Conv2d 3x3 pad 1, 24 -> NC, no bias (+ sigmoid)
def head3x3_fwd(x, w, sigmoid, rounded=True):
    """x [B,H,W,C], w [NC,C,3,3].  Returns out [B,NC,H,W] (sigmoid(logit) or logit), logit, and the logit's magnitude sum."""
    B, H, W, C = x.shape
    Wr = _w(w, rounded)
    xp = F.pad(x, (0, 0, 1, 1, 1, 1))
    xpa = xp.abs()
    lg = torch.zeros(B, H, W, w.shape[0], dtype=x.dtype, device=x.device)
    mag = torch.zeros_like(lg)
    for ky in range(3):
        for kx in range(3):
            lg += xp[:, ky:ky + H, kx:kx + W] @ Wr[:, :, ky, kx].t()
            mag += xpa[:, ky:ky + H, kx:kx + W] @ Wr[:, :, ky, kx].abs().t()
    lg, mag = lg.permute(0, 3, 1, 2), mag.permute(0, 3, 1, 2)
    return (torch.sigmoid(lg) if sigmoid else lg), lg, mag


def head3x3_bwd(dout, prob, x, w, sigmoid, rounded=True):
    """dout [B,NC,H,W] (f32 values), prob the forward's stored output (sigmoid head) or None, x [B,H,W,C], w [NC,C,3,3].
    DL = dout p (1 - p) (or dout), rounded to bf16 for the matrix cores: round_bf16(DL, err) with err = 4 u |DL| (1 - p, the two
    products and the conversion in f32; without the sigmoid DL is an f32 input and err = 0).  Returns
        dx [B,H,W,C], dx_mag, dx_slack          dx[y][x][c] = sum_{n,ky,kx} DL[n][y+1-ky][x+1-kx] W[n][c][ky][kx]
        dW [NC,C,3,3], dW_mag, dW_slack         dW[n][c][ky][kx] = sum_{b,y,x} DL[n][y][x] x[y-1+ky][x-1+kx][c]
    slack = the ulp of DL values that may round the other way, times |W| (dx) or |x| (dW)."""
    B, NC, H, W = dout.shape
    C = x.shape[-1]
    Wr = _w(w, rounded)
    dl = dout * prob * (1 - prob) if sigmoid else dout
    sl = torch.zeros_like(dl)
    if rounded:
        dl, sl = round_bf16(dl, (4 * 2.0 ** -24 if sigmoid else 0.0) * dl.abs())
    dl, sl = dl.permute(0, 2, 3, 1), sl.permute(0, 2, 3, 1)                     # [B,H,W,NC]
    dlp, slp = F.pad(dl, (0, 0, 1, 1, 1, 1)), F.pad(sl, (0, 0, 1, 1, 1, 1))
    dlpa = dlp.abs()
    xp = F.pad(x, (0, 0, 1, 1, 1, 1))
    dx = torch.zeros(B, H, W, C, dtype=x.dtype, device=x.device)
    dxm, dxs = torch.zeros_like(dx), torch.zeros_like(dx)
    dw = torch.zeros(NC, C, 3, 3, dtype=x.dtype, device=x.device)
    dwm, dws = torch.zeros_like(dw), torch.zeros_like(dw)
    dlt, slt = dl.reshape(-1, NC).t(), sl.reshape(-1, NC).t()
    dlta = dlt.abs()
    for ky in range(3):
        for kx in range(3):
            s = (slice(None), slice(2 - ky, 2 - ky + H), slice(2 - kx, 2 - kx + W))
            Wk = Wr[:, :, ky, kx]
            dx += dlp[s] @ Wk
            dxm += dlpa[s] @ Wk.abs()
            dxs += slp[s] @ Wk.abs()
            xs = xp[:, ky:ky + H, kx:kx + W].reshape(-1, C)
            dw[:, :, ky, kx] = dlt @ xs
            dwm[:, :, ky, kx] = dlta @ xs.abs()
            dws[:, :, ky, kx] = slt @ xs.abs()
    return dx, dxm, dxs, dw, dwm, dws


# ------------------------------------------------------------------------------------ stem: conv_xy backward (1x3x3, 3 -> 24, pad 1)
# v[b][c][t][y][x] = sum_{ci,ky,kx} x[b][ci][t][y-1+ky][x-1+kx] w_t[c][ci][0][ky][kx];  dv [B,T,H,W,24] is the gradient at v
def stem_wx(x, w_t, dv, t_first, n_frames, per_sample):
    """x [B,3,T,H,W] (f32 values), w_t [24,3,1,3,3], dv [B,T,H,W,24] (bf16 values): the dW_t [24][27] (column ci 9 + ky 3 + kx) and dP
    of c3d_stem_bwd_wx.  dP is the input gradient of frames t_first .. t_first + n_frames - 1: per_sample -> [B,3,n_frames,H,W],
    otherwise summed over the batch -> [3,n_frames,H,W]; None when n_frames == 0.
    Returns {"rounded": (dW, dW_mag, dP, dP_mag), "unrounded": (...)}: rounded = x and w_t rounded to bf16 for the products (what
    C3D_OPT_STEM_MFMA = 2 multiplies: x enters dW only, w_t enters dP only), unrounded = the f32 values."""
    B, _, T, H, W = x.shape
    C = dv.shape[-1]
    out = {}
    dvt = dv.reshape(-1, C).t()
    dvta = dvt.abs()
    for key, rnd in (("rounded", True), ("unrounded", False)):
        xr, wr = _w(x, rnd), _w(w_t, rnd)[:, :, 0]                                    # [24][3][3][3]
        xp = F.pad(xr, (1, 1, 1, 1)).permute(0, 2, 3, 4, 1)                             # [B,T,H+2,W+2,3]
        dw = torch.zeros(C, 3, 3, 3, dtype=x.dtype, device=x.device)
        dwm = torch.zeros_like(dw)
        for ky in range(3):
            for kx in range(3):
                xs = xp[:, :, ky:ky + H, kx:kx + W].reshape(-1, 3)
                dw[:, :, ky, kx] = dvt @ xs
                dwm[:, :, ky, kx] = dvta @ xs.abs()
        dp = dpm = None
        if n_frames > 0:
            d = F.pad(dv[:, t_first:t_first + n_frames], (0, 0, 1, 1, 1, 1))            # [B,n,H+2,W+2,24]
            da = d.abs()
            dp = torch.zeros(B, n_frames, H, W, 3, dtype=x.dtype, device=x.device)
            dpm = torch.zeros_like(dp)
            for ky in range(3):
                for kx in range(3):
                    s = (slice(None), slice(None), slice(2 - ky, 2 - ky + H), slice(2 - kx, 2 - kx + W))
                    dp += d[s] @ wr[:, :, ky, kx]
                    dpm += da[s] @ wr[:, :, ky, kx].abs()
            dp, dpm = dp.permute(0, 4, 1, 2, 3), dpm.permute(0, 4, 1, 2, 3)             # [B,3,n,H,W]
            if not per_sample:
                dp, dpm = dp.sum(0), dpm.sum(0)
        out[key] = (dw.reshape(C, 27), dwm.reshape(C, 27), dp, dpm)
    return out
