"""The decoder and stem kernels against float64 on their MULTI-TILE paths, at the smallest shapes that reach them.

tests/test_decoder_ops_gpu.py and the stem tests of tests/test_model_gpu.py run every one of these kernels where a workgroup
handles one tile and every grid-stride loop runs once; the benchmark step (B = 32, 256 x 256, bf16) runs each of them on another
path.  Here every case computes its walk from c3d_device_cus() with the host arithmetic of the launcher, ASSERTS the walk it
intends (a later change of a launch heuristic fails the test instead of returning it to the one-tile path), calls the kernel
through the C ABI with NaN-filled outputs and non-zero accumulate-into buffers, and compares every written element with the
float64 restatement in tests/decoder_reference.py (pinned against torch.autograd by tests/test_hotpath_reference_cpu.py), the
way tests/test_hotpath_bf16_gpu.py does; `Bound` is that file's.  The restatements run in double on the device.

Kernel, path asserted (numbers for 256 compute units), eps (u = 2^-24; "next power of two" = the smallest 2^k >= count * u)

  convt_fwd_mfma_kernel<C>        grid = min(CUs * (6 if C == 24 else 2), ceil(wave_tiles / 4)), wave_tiles = B h ceil(wd / 16).
  convt_bwd_data_mfma_kernel<C>   C 48: B 3, h 56, wd 404 -> 4368 wave tiles on 512 workgroups: 3 iterations, the last ragged
                                  (4368 = 2 x 2048 + 272).  C 24: B 4, h 64, wd 773 -> 12 544 on 1536: 3 iterations (2 x 6144 + 256).
                                  The forward re-uses its per-wave LDS output tile across iterations, the data gradient runs its
                                  register prefetch `issue(t + gridDim.x * 4, nx)` twice per wave.  Controls: h 1, wd 13, one iteration.
                                  Outputs are bf16: |dev - ref| <= 2^-8 (|ref| + E) + E, E = eps * sum|term|.
                                  forward: the bias starts the accumulator, 4 C products are added by the matrix cores, the skip
                                  is added before the store: 4 C + 2 additions -> 98 u -> 2^-17 (C 24), 194 u -> 2^-16 (C 48).
                                  data gradient: 16 C products: 384 u -> 2^-15, 768 u -> 2^-14.  bf16 x bf16 products are exact.
  convt_wgrad_mfma_kernel<C>      grid = min(2 CUs, tiles), tiles = B ceil(h / 4) ceil(wd / 32).  C 24: h 67, wd 200 (17 x 7 tiles,
  + convt_wgrad_reduce_kernel     both ragged), B chosen so that 2 grid < tiles < 3 grid (B 11: 1309 tiles on 512 workgroups: 285
                                  accumulate 3 tiles, 227 two; the __syncthreads() at the loop top separates tiles).  C 48: B 2,
                                  h 9, wd 130 -> 30 tiles = 30 workgroups: the reducer's 4-way unrolled branch (nwg >= 25) with one
                                  tile each.  dW starts at ones.  eps: a workgroup contracts 128 pixels per tile into one f32
                                  accumulator, the reducer adds at most nwg / 8 + 8 values in a chain: (3 x 128 + 72) u -> 2^-15;
                                  (128 + 12) u -> 2^-16.  The workspace size must be grid * 16 C^2 floats.
  head_fwd_mfma_kernel            tpw halves from 4 (forward) / 8 (backward) until ceil(ntiles / tpw) B >= 768.  188 x 1000 (24 x 32
  head_bwd_mfma_kernel            = 768 ragged tiles): B 2 -> tpw 2 / 2, B 4 -> tpw 4 / 4; parts = 768 partial dW images, the
  + head_dw_reduce_kernel         reducer's unrolled branch needs parts > 96.  Reached: the register prefetch of the next X tile,
                                  dwa accumulating over tiles.  forward: f32 output, 216 products (9 k-steps of 32 with 24 used):
                                  eps = 2^-16; with the sigmoid the bound is E / 4 (the slope) + 10 u p: expf 2 ulp = 4 u on
                                  e^-v, which enters 1 + e^-v by (1 - p); the sum 1 u; the division 2.5 ulp = 5 u (1 ulp = 2 u).
                                  dx: bf16, 9 NC products: 9 u -> 2^-20 (NC 1), 63 u -> 2^-18 (NC 7), + the slack of DL = dout p (1 - p)
                                  values within 4 u of a bf16 rounding boundary (ulp x |W|).  dW: a wave adds 64 pixels per tile
                                  over tpw tiles, three adds join the waves, the reducer's lane adds ceil(parts / 32) values, then
                                  2 + 5 shuffle adds and the += : (64 tpw + 3 + parts / 32 + 8) u -> 2^-16 at tpw 2, 2^-15 at tpw 4.
  stem_fwd / stem_bwd_dv          fwd_t halves tpw from 8 until ceil(ntiles / tpw) B >= 1024, dv_t from 16 until >= 512.  B 4 at
  (MFMA, any storage)             512 x 512 and at 505 x 500 (1024 tiles, ragged): tpw 4 forward, tpw 8 dv.  u, dv and the
                                  per-sample dP must be bit-identical to the scalar kernels (C3D_OPT_STEM_MFMA = 0), the
                                  atomically summed outputs within 2e-6 of their largest entry, as at tpw 1 in test_model_gpu.py.
  stem_bwd_wx_bf16_kernel<3>      grid (ntiles, bsplit), bsplit = min(B, ceil(512 / ntiles)).  B 20 at 128 x 128: 64 tiles, bsplit 8,
  (C3D_OPT_STEM_MFMA = 2)         three batch iterations, the last short (20 = 8 + 8 + 4).  B 2 at 256 x 512: 512 tiles, gridDim.y
                                  == 1: two iterations and the "sole owner" plain += of dP.  Against stem_wx ROUNDED (x and w_t as
                                  bf16, products exact): dW_t: a wave adds 64 pixels x T frames per sample, 3 adds join the
                                  waves, ntiles x bsplit atomics land on one value: (576 + 4 + 512) u -> 2^-13, (384 + 4 + 512) u
                                  -> 2^-14; dP summed: 216 products per sample and iteration + bsplit atomics + the += : 657 u
                                  -> 2^-14, 434 u -> 2^-15; per sample 216 u -> 2^-16.  Against stem_wx UNROUNDED: 2^-8 sum|term|
                                  (two operand roundings of 2^-9).

Measured worst error / bound (one MI355X, 256 CUs; every case is listed in profiles/decoder_parity.txt):
  convt_fwd_mfma_kernel<24>       out 0.993          convt_fwd_mfma_kernel<48>       out 0.984
  convt_bwd_data_mfma_kernel<24>  din 0.955          convt_bwd_data_mfma_kernel<48>  din 0.912
  convt_wgrad_mfma_kernel<24>     dW < 0.0005        convt_wgrad_mfma_kernel<48>     dW 0.001
  head_fwd_mfma_kernel            prob 0.003, logit 0.008
  head_bwd_mfma_kernel            dx 0.996, dW 0.015
  stem_bwd_wx_bf16_kernel<3>      rounded: dW_t < 0.0005, dP summed 0.004, dP per sample 0.008
                                  unrounded: dW_t 0.002, dP summed 0.157, dP per sample 0.258
  stem forward / dv at tpw 4 / 8  bit-identical to the scalar kernels; sums within 2e-6
The bf16 outputs sit just under 1 for the reason given in test_hotpath_bf16_gpu.py: half an ulp is 2^-8 of a value just above a
power of two, so the bound is attained by a correctly rounded result.  The f32 sums are far below their worst-case bounds, as
independent rounding errors are (the bound grows with the chain length n, their sum with sqrt(n)); the negative controls show
what those bounds still see: one missing tile of 1309 (convT dW, 9 x the bound) or of 1536 (head dW, 18 x).

Negative controls, one per family, each in an ordinary valid launch in which the device's input differs from the reference's in
one place: a convT weight tap scaled by 1 + 2^-5 (forward), a dout row that only second-iteration tiles read zeroed (data
gradient), an input tile that is a workgroup's second tile zeroed (convT weight gradient, head dW), one head weight changed.  The
same comparison must raise."""
import math

import pytest
import torch

import decoder_reference as D
from test_hotpath_bf16_gpu import BF, DEV, U, Bound, _check, _need_gpu, _randn

pytestmark = pytest.mark.gpu

R8 = 2.0 ** -8


def eps_for(additions):
    """The smallest power of two that is >= additions * u."""
    return 2.0 ** math.ceil(math.log2(additions * U))


def _cdiv(a, b):
    return (a + b - 1) // b


def _cus():
    from change3d_amd import _lib
    return _lib.lib().c3d_device_cus()


def _d(t):
    return t.detach().double()


def _neg(bound, what=None):
    print(f"\nDECODER-NEG {bound.kernel} | {bound.shape} | error/bound {bound.worst():.2f}")
    if what is not None:
        assert bound.rows[what] > 1.0, (what, bound.rows)
    with pytest.raises(AssertionError, match="bound exceeded"):
        bound.check(record=False)


# ================================================================================================ convT forward / data gradient
def convt_walk(C, B, h, wd):
    """(wave tiles, workgroups, iterations of the longest-running wave) of launch_fwd / launch_bwd_data (csrc/convt_mfma.hip)."""
    wave_tiles = B * h * _cdiv(wd, 16)
    grid = max(1, min(_cus() * (6 if C <= 24 else 2), _cdiv(wave_tiles, 4)))
    return wave_tiles, grid, _cdiv(wave_tiles, 4 * grid)


def run_convt_fwd(C, B, h, wd, with_skip, tamper=None, seed=7000):
    from change3d_amd import ops
    x = _randn((B, h, wd, C), seed, dtype=BF)
    w = _randn((C, C, 4, 4), seed + 1, 0.2)
    bias = _randn((C,), seed + 2, 0.5)
    skip_full = _randn((B, 3, 2 * h, 2 * wd, C), seed + 3, dtype=BF) if with_skip else None      # NDHWC; frame 1 is the skip
    w_ref = _d(w)
    if tamper is not None:
        tamper(dict(w=w))
    out = torch.full((B, 2 * h, 2 * wd, C), float("nan"), dtype=BF, device=DEV)
    if with_skip:
        frame = skip_full[:, 1]
        assert skip_full.stride(0) != 4 * h * wd * C
        ops.convT_fwd(x, w, bias, frame.data_ptr(), skip_full.stride(0), out, B, h, wd, C, ops.DT_BF16)
    else:
        ops.convT_fwd(x, w, bias, None, 0, out, B, h, wd, C, ops.DT_BF16)
    k = ops.last_kernel()
    torch.cuda.synchronize()
    assert k == f"convt_fwd_mfma_kernel<{C}>", k
    bd = Bound(k, f"B {B} h {h} wd {wd} {'skip' if with_skip else 'no skip'}")
    ref, mag = D.convt4s2_fwd(_d(x), w_ref, _d(bias), _d(skip_full[:, 1]) if with_skip else None)
    bd.add("out", out, ref, mag, eps_for(4 * C + 2), rel=R8)
    return bd


def run_convt_dgrad(C, B, h, wd, tamper=None, seed=7100):
    from change3d_amd import ops
    dout = _randn((B, 2 * h, 2 * wd, C), seed, dtype=BF)
    w = _randn((C, C, 4, 4), seed + 1, 0.2)
    dout_ref = _d(dout)
    if tamper is not None:
        tamper(dict(dout=dout))
    din = torch.full((B, h, wd, C), float("nan"), dtype=BF, device=DEV)
    ops.convT_bwd_data(dout, w, din, B, h, wd, C, ops.DT_BF16)
    k = ops.last_kernel()
    torch.cuda.synchronize()
    assert k == f"convt_bwd_data_mfma_kernel<{C}>", k
    bd = Bound(k, f"B {B} h {h} wd {wd}")
    ref, mag = D.convt4s2_dgrad(dout_ref, _d(w))
    bd.add("din", din, ref, mag, eps_for(16 * C), rel=R8)
    return bd


CONVT_MULTI = [(48, 3, 56, 404), (24, 4, 64, 773)]
CONVT_ONE = [(48, 2, 1, 13), (24, 3, 1, 13)]


def _assert_multi_iteration_walk(C, B, h, wd):
    wave_tiles, grid, iters = convt_walk(C, B, h, wd)
    assert iters >= 3 and wave_tiles % (4 * grid) != 0 and wd % 16 != 0, (wave_tiles, grid, iters)
    return wave_tiles, grid, iters


@pytest.mark.parametrize("with_skip", [True, False])
@pytest.mark.parametrize("C,B,h,wd", CONVT_MULTI)
def test_convT_forward_over_three_iterations_per_wave(C, B, h, wd, with_skip):
    _need_gpu()
    _assert_multi_iteration_walk(C, B, h, wd)
    _check(run_convt_fwd(C, B, h, wd, with_skip))


@pytest.mark.parametrize("C,B,h,wd", CONVT_MULTI)
def test_convT_data_gradient_over_three_iterations_per_wave(C, B, h, wd):
    _need_gpu()
    _assert_multi_iteration_walk(C, B, h, wd)
    _check(run_convt_dgrad(C, B, h, wd))


@pytest.mark.parametrize("C,B,h,wd", CONVT_ONE)
def test_convT_forward_and_data_gradient_below_the_cap(C, B, h, wd):
    """Control: one row, less than one wave tile across, one iteration."""
    _need_gpu()
    assert convt_walk(C, B, h, wd)[2] == 1 and h == 1 and wd < 16
    _check(run_convt_fwd(C, B, h, wd, True), run_convt_fwd(C, B, h, wd, False), run_convt_dgrad(C, B, h, wd))


def test_convT_forward_bound_sees_a_scaled_tap():
    _need_gpu()

    def scale_one_tap(d):                                   # the largest one: the control must not depend on a tap that happens to be tiny
        d["w"].view(-1)[d["w"].abs().argmax()] *= 1 + 2.0 ** -5

    _neg(run_convt_fwd(24, 4, 64, 773, True, tamper=scale_one_tap))


def test_convT_data_gradient_bound_sees_a_missing_row_of_the_second_iteration():
    """dout row 2 iy of sample b is read by the input rows iy - 1 and iy only; both rows' wave tiles are chosen inside the second
    iteration [4 grid, 8 grid), which no wave reaches without the prefetch `issue(t + gridDim.x * 4, nx)`."""
    _need_gpu()
    C, B, h, wd = 48, 3, 56, 404
    wave_tiles, grid, iters = _assert_multi_iteration_walk(C, B, h, wd)
    tiles_x = _cdiv(wd, 16)
    row = (4 * grid + 8 * grid) // 2 // tiles_x            # b * h + iy in the middle of the second iteration
    if row % h == 0:
        row += 1
    b, iy = divmod(row, h)
    assert 4 * grid <= (row - 1) * tiles_x and (row + 1) * tiles_x <= min(8 * grid, wave_tiles) and iy >= 1 and b < B

    def zero_a_row(d):
        d["dout"][b, 2 * iy] = 0

    _neg(run_convt_dgrad(C, B, h, wd, tamper=zero_a_row))


# ================================================================================================ convT weight gradient
def wgrad_walk(B, h, wd):
    tiles = B * _cdiv(h, 4) * _cdiv(wd, 32)
    grid = max(1, min(2 * _cus(), tiles))
    return tiles, grid


def run_convt_wgrad(C, B, h, wd, tamper=None, seed=7200):
    from change3d_amd import ops, _lib
    tiles, grid = wgrad_walk(B, h, wd)
    assert _lib.lib().c3d_convT4s2_wgrad_ws_floats(B, h, wd, C) == grid * 16 * C * C
    t = _randn((B, h, wd, C), seed, dtype=BF)
    dcur = _randn((B, 2 * h, 2 * wd, C), seed + 1, dtype=BF)
    t_ref = _d(t)
    if tamper is not None:
        tamper(dict(t=t))
    dw = torch.ones((C, C, 4, 4), dtype=torch.float32, device=DEV)          # the kernel accumulates into it
    ops.convT_wgrad(t, dcur, dw, B, h, wd, C, ops.DT_BF16)
    k = ops.last_kernel()
    torch.cuda.synchronize()
    assert k == f"convt_wgrad_mfma_kernel<{C}>", k
    bd = Bound(k, f"B {B} h {h} wd {wd}: {tiles} tiles on {grid} workgroups")
    ref, mag = D.convt4s2_wgrad(t_ref, _d(dcur))
    bd.add("dW", _d(dw) - 1.0, ref, mag + 1.0, eps_for(_cdiv(tiles, grid) * 128 + grid / 8 + 8))
    return bd


def _wgrad_three_and_two(cus):
    """h 67 x wd 200 = 17 x 7 ragged tiles per sample; B so that 2 grid < tiles < 3 grid."""
    h, wd = 67, 200
    return (2 * cus * 7 // 3) // (17 * 7) + 1, h, wd


def test_convT_weight_gradient_accumulates_three_and_two_tiles_per_workgroup():
    _need_gpu()
    B, h, wd = _wgrad_three_and_two(_cus())
    tiles, grid = wgrad_walk(B, h, wd)
    assert tiles == B * 17 * 7 and grid == 2 * _cus() and 2 * grid < tiles < 3 * grid and tiles % grid != 0 and h % 4 and wd % 32, (tiles, grid)
    _check(run_convt_wgrad(24, B, h, wd))


def test_convT_weight_gradient_reducer_unrolled_branch_with_one_tile_each():
    _need_gpu()
    B, h, wd = 2, 9, 130
    tiles, grid = wgrad_walk(B, h, wd)
    assert tiles == 30 and 25 <= tiles <= 2 * _cus() and grid == tiles, (tiles, grid)
    _check(run_convt_wgrad(48, B, h, wd))


def test_convT_weight_gradient_bound_sees_a_missing_second_tile():
    _need_gpu()
    B, h, wd = _wgrad_three_and_two(_cus())
    tiles, grid = wgrad_walk(B, h, wd)
    tl = grid + 5                                           # the second tile of workgroup 5
    assert tl < tiles
    tx, r = tl % 7, tl // 7
    ty, b = r % 17, r // 17

    def zero_a_tile(d):
        d["t"][b, 4 * ty:4 * ty + 4, 32 * tx:32 * tx + 32] = 0

    _neg(run_convt_wgrad(24, B, h, wd, tamper=zero_a_tile))


# ================================================================================================ head
def head_tpw(ntiles, B, dflt):
    tpw = dflt
    while tpw > 1 and _cdiv(ntiles, tpw) * B < 3 * 256:
        tpw >>= 1
    return min(tpw, ntiles)


def head_walk(B, H, W):
    ntiles = _cdiv(W, 32) * _cdiv(H, 8)
    tf, tb = head_tpw(ntiles, B, 4), head_tpw(ntiles, B, 8)
    return ntiles, tf, tb, _cdiv(ntiles, tb) * B


def run_head(NC, sig, B, H, W, tamper=None, seed=7300):
    from change3d_amd import ops, _lib
    C = 24
    ntiles, tf, tb, parts = head_walk(B, H, W)
    assert _lib.lib().c3d_head3x3_bwd_ws_floats(B, H, W, NC) == parts * NC * C * 9
    shape = f"NC {NC}{' sigmoid' if sig else ''} B {B} {H}x{W}: tpw {tf} / {tb}, {parts} parts"
    x = _randn((B, H, W, C), seed, dtype=BF)
    w = _randn((NC, C, 3, 3), seed + 1, 0.2)
    dout = _randn((B, NC, H, W), seed + 2)
    x_ref, w_ref = _d(x), _d(w)
    if tamper is not None:
        tamper(dict(x=x, w=w))
    out = torch.full((B, NC, H, W), float("nan"), device=DEV)
    ops.head_fwd(x, w, out, B, H, W, C, NC, sig, ops.DT_BF16)
    dx = torch.full((B, H, W, C), float("nan"), dtype=BF, device=DEV)
    dw = torch.ones((NC, C, 3, 3), device=DEV)                              # accumulate semantics
    ops.head_bwd(dout, out if sig else None, x, w, dx, dw, B, H, W, C, NC, sig, ops.DT_BF16)
    torch.cuda.synchronize()
    bf, bb = Bound("head_fwd_mfma_kernel", shape), Bound("head_bwd_mfma_kernel", shape)
    ref, _, mag = D.head3x3_fwd(x_ref, w_ref, sig)
    if sig:
        bf.add("prob", out, ref, mag / 4, 2.0 ** -16, slack=10 * U * ref)
    else:
        bf.add("logit", out, ref, mag, 2.0 ** -16)
    # the backward is handed the DEVICE's probabilities: the restatement starts from the same f32 values
    rdx, dxm, dxs, rdw, dwm, dws = D.head3x3_bwd(_d(dout), _d(out) if sig else None, x_ref, w_ref, sig)
    bb.add("dx", dx, rdx, dxm, eps_for(9 * NC), rel=R8, slack=dxs)
    bb.add("dW", _d(dw) - 1.0, rdw, dwm + 1.0, eps_for(64 * tb + 3 + _cdiv(parts, 32) + 8), slack=dws)
    return bf, bb


@pytest.mark.parametrize("NC,sig", [(1, True), (7, False)])
@pytest.mark.parametrize("B,tpw", [(2, 2), (4, 4)])
def test_head_forward_and_backward_over_several_tiles_per_workgroup(B, tpw, NC, sig):
    _need_gpu()
    H, W = 188, 1000                                       # 24 x 32 tiles, ragged in both directions
    ntiles, tf, tb, parts = head_walk(B, H, W)
    assert ntiles == 768 and tf == tpw and tb >= tpw and parts > 96 and H % 8 and W % 32, (ntiles, tf, tb, parts)
    _check(*run_head(NC, sig, B, H, W))


def test_head_forward_over_full_tiles():
    """192 x 1024: the same walks without a ragged edge."""
    _need_gpu()
    assert head_walk(2, 192, 1024) == (768, 2, 2, 768)
    _check(*run_head(1, True, 2, 192, 1024))


def test_head_bounds_see_a_changed_weight_and_a_missing_second_tile():
    _need_gpu()
    B, H, W = 4, 188, 1000
    ntiles, tf, tb, parts = head_walk(B, H, W)
    assert tb >= 2

    def change_one_weight(d):
        d["w"][3, 11, 1, 2] *= 1 + 2.0 ** -3

    bf, _ = run_head(7, False, B, H, W, tamper=change_one_weight)
    _neg(bf)
    B = 2
    ntiles, tf, tb, parts = head_walk(B, H, W)
    assert tb >= 2
    tl = 7 * tb + 1                                        # the second tile of workgroup 7 of sample 1
    ty, tx = divmod(tl, _cdiv(W, 32))

    def zero_a_tile(d):
        d["x"][1, 8 * ty:8 * ty + 8, 32 * tx:32 * tx + 32] = 0

    _, bb = run_head(7, False, B, H, W, tamper=zero_a_tile)
    _neg(bb, "dW")


# ================================================================================================ stem
def stem_tpw(ntiles, B, dflt, floor):
    tpw = dflt
    while tpw > 1 and _cdiv(ntiles, tpw) * B < floor:
        tpw >>= 1
    return tpw


@pytest.mark.parametrize("B,H,W", [(4, 512, 512), (4, 505, 500)])
def test_stem_mfma_kernels_equal_the_scalar_kernels_over_several_tiles_per_workgroup(B, H, W):
    _need_gpu()
    from change3d_amd import ops
    T, dtype = 3, BF
    ntiles = _cdiv(W, 32) * _cdiv(H, 8)
    tf, tv = stem_tpw(ntiles, B, 8, 1024), min(stem_tpw(ntiles, B, 16, 512), ntiles)
    assert tf >= 4 and tv >= 4 and stem_tpw(ntiles, B - 1, 8, 1024) < 4, (ntiles, tf, tv)     # the smallest B that reaches tpw 4
    dt = ops.dt_code(dtype)
    x = _randn((B, 3, T, H, W), 7400)
    w_t, w_xy = _randn((24, 3, 1, 3, 3), 7401, 0.3), _randn((24, 1, 5, 1, 1), 7402, 0.5)
    g0 = _randn((B, T, H, W, 24), 7403, dtype=dtype)
    coef = _randn((72,), 7404)

    def run(opt):
        ops.set_option(ops.OPT_STEM_MFMA, opt)
        u = torch.full((B, T, H, W, 24), float("nan"), dtype=dtype, device=DEV)
        sums = torch.zeros(48, dtype=torch.float64, device=DEV)
        ops.stem_fwd(x, w_t, w_xy, u, sums, B, T, H, W, dt)
        dv = torch.full_like(u, float("nan"))
        dw_xy = torch.zeros(24, 5, device=DEV)
        ops.stem_bwd_dv(x, w_t, w_xy, g0, u, coef, dv, dw_xy, B, T, H, W, dt)
        dw_t = torch.zeros(24, 27, device=DEV)
        dP = torch.zeros(B, 3, T, H, W, device=DEV)
        ops.stem_bwd_wx(x, w_t, dv, dw_t, dP, B, T, H, W, 0, T, True, dt)
        torch.cuda.synchronize()
        return dict(u=u, dv=dv, dP=dP), dict(sums=sums, dw_xy=dw_xy, dw_t=dw_t)

    try:
        (ea, sa), (eb, sb) = run(1), run(0)
    finally:
        ops.set_option(ops.OPT_STEM_MFMA, 2)
    for k in ea:
        assert bool(torch.isfinite(ea[k].float()).all()), k
        assert torch.equal(ea[k], eb[k]), k
    for k in sa:
        assert (sa[k] - sb[k]).abs().max().item() <= 2e-6 * sb[k].abs().max().item(), k
    assert eb["u"].float().abs().max().item() > 0.1 and eb["dP"].abs().max().item() > 0.1


@pytest.mark.parametrize("B,H,W,bsplit,iters", [(20, 128, 128, 8, 3), (2, 256, 512, 1, 2)])
def test_stem_bwd_wx_bf16_walks_the_batch(B, H, W, bsplit, iters):
    _need_gpu()
    from change3d_amd import ops
    T = 3
    ntiles = _cdiv(W, 32) * _cdiv(H, 8)
    bs = max(1, min(B, _cdiv(2 * 256, ntiles)))
    assert bs == bsplit and _cdiv(B, bs) == iters and (bs == 1 or B % bs != 0) and (bs > 1 or ntiles >= 512), (ntiles, bs)
    dt = ops.DT_BF16
    x = _randn((B, 3, T, H, W), 7500)
    w_t = _randn((24, 3, 1, 3, 3), 7501, 0.3)
    dv = _randn((B, T, H, W, 24), 7502, dtype=BF)
    ops.set_option(ops.OPT_STEM_MFMA, 2)
    dw1, dw2, dw3 = (torch.ones(24, 27, device=DEV) for _ in range(3))           # accumulate semantics
    dPs = torch.ones(3, 1, H, W, device=DEV)
    ops.stem_bwd_wx(x, w_t, dv, dw1, dPs, B, T, H, W, 1, 1, False, dt)
    k = ops.last_kernel()
    dP = torch.full((B, 3, T, H, W), float("nan"), device=DEV)
    ops.stem_bwd_wx(x, w_t, dv, dw2, dP, B, T, H, W, 1, 1, True, dt)
    ops.stem_bwd_wx(x, w_t, dv, dw3, None, B, T, H, W, 0, 0, False, dt)
    torch.cuda.synchronize()
    assert k == "stem_bwd_wx_bf16_kernel<3>" and ops.last_kernel() == k, k
    assert bool(torch.isnan(dP[:, :, 0]).all()) and bool(torch.isnan(dP[:, :, 2]).all())    # only the perception frame is written
    xs, ws, ds = _d(x), _d(w_t), _d(dv)
    summed, per = D.stem_wx(xs, ws, ds, 1, 1, False), D.stem_wx(xs, ws, ds, 1, 1, True)
    bd = Bound(k, f"B {B} {H}x{W}: grid ({ntiles}, {bs}), {iters} batch iterations")
    e_dw = eps_for(iters * T * 64 + 4 + ntiles * bs)
    rw, rwm, rp, rpm = summed["rounded"]
    uw, uwm, up, upm = summed["unrounded"]
    for name, dw in (("dW_t (dP summed)", dw1), ("dW_t (dP per sample)", dw2), ("dW_t (no dP)", dw3)):
        bd.add(name, _d(dw) - 1.0, rw, rwm + 1.0, e_dw)
        bd.add(name + " vs f32 operands", _d(dw) - 1.0, uw, uwm, R8)
    bd.add("dP summed", _d(dPs) - 1.0, rp, rpm + 1.0, eps_for(216 * iters + bs + 1))
    bd.add("dP summed vs f32 operands", _d(dPs) - 1.0, up, upm, R8)
    bd.add("dP per sample", dP[:, :, 1:2], per["rounded"][2], per["rounded"][3], eps_for(216))
    bd.add("dP per sample vs f32 operands", dP[:, :, 1:2], per["unrounded"][2], per["unrounded"][3], R8)
    _check(bd)
