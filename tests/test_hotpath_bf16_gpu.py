"""The bf16-only training kernels against float64, directly, at the shapes the benchmark runs.

Every case calls one kernel through the C ABI, asserts WHICH kernel ran (c3d_last_kernel: the dispatchers fall through to an
older kernel where the new one does not apply, silently) and compares every output the kernel writes with the float64
restatement of the operation in tests/hotpath_reference.py (pinned against torch.autograd by
tests/test_hotpath_reference_cpu.py), element by element.  Output buffers are pre-filled with NaN; padding channels must come
back as exact zeros.

Kernels and the branch of each that a case must reach
  dw_fwd_v2_kernel<bf16, T, PK, HV>      stride-1 forward: HV half-vector lanes (C3D_OPT_DW_FWD_HV bit 0, T = 3), PK packed slot
                                         descriptors (tile-relative offsets under 2^22 elements)
  dw_fwd_v2s2_kernel<bf16, 3, PK, W8>    stride-2 forward: W8 eight waves per tile (C3D_OPT_DW_FWD_HV bit 2)
  dw_fwd_kernel<bf16, 2, 4, 8, T>        stride-2 forward of four- and five-frame clips (the polyphase tile does not fit).  This
                                         first kernel keeps its activated tile in LDS as bf16: relu(a scale + shift) is ROUNDED
                                         before the taps (the v2 kernels and the backward's dW use the f32 value).  The
                                         restatement rounds there too for this kernel; without that step it is 2^-9 per
                                         operand, up to 1000 x the bound -- this file's first run found it
  dw_bwd_ring_kernel<T, SPREAD>          stride-1 backward on the LDS-DMA ring (C3D_OPT_DW_RING, default 13)
  dw_bwd_fused_kernel<bf16, T, 2>        stride-2 backward
  pw_cfwd_kernel<1, NTW, KS, true>       conv_c forward, cooperative (C3D_OPT_PW_CFWD bit 0): BatchNorm_b + SE gate from per-sample sums
  pw_cfwd_kernel<2, NTW, KS, true>       conv_a forward with the residual prologue (bit 1)
  pw_cdg_a_kernel<...>                   conv_a data gradient + dW, cooperative (C3D_OPT_PW_CDG bit 0): ReLU mask, BatchNorm_c-backward sums
  pw_cdg_c_kernel<...>                   conv_c data gradient + dW (bit 1): Swish / SE backward epilogue, per-sample sums
  pw_wgrad_v2_kernel<HASP2, QSW, ..>     weight gradient, flat-staged (C3D_OPT_PW_WGRAD_V2): affine / swish (gated or not) operands

Shapes.  Group A is the BCD benchmark step (X3D-L, B = 32, T = 3, 256 x 256 input; change3d_amd/model/x3d.py: stage widths
24 / 48 / 96, inner 54 / 108 / 216, the first block of a stage has stride 2):
                         res2                       res3                    res4
  depthwise stride 1     128 x 128, C 54            64 x 64, C 108          32 x 32, C 216
  depthwise stride 2     256 x 256 -> 128, C 54     128 -> 64, C 108        64 -> 32, C 216
  conv_c (inner -> out)  54 -> 24, M 1 572 864      108 -> 48, M 393 216    216 -> 96, M 98 304     rows / sample M / 32
  conv_a (out -> inner)  24 -> 54                   48 -> 108               96 -> 216
Group B: the SCD step's five-frame pair (B = 16) and BDA's four-frame pair (B = 8) at the same six depthwise shapes.  Group C: edges --
extents that are no tile multiples under both strides, one tile per sample with walks over many samples, walks that cross a
sample boundary, C = 24 (one short chunk) and 216 (seven chunks, empty last vector), a bf16 call that cannot use packed
descriptors (PK = false), every value of C3D_OPT_DW_FWD_HV in 0 / 1 / 4 / 5; for the GEMMs M just above the 1024 floor, a
ragged last tile, samples that end inside a tile, a workgroup spanning two samples, tiles_per_wg 2 and 3.

Bound, per element, derived (u = 2^-24, the unit roundoff of f32):
    bf16 outputs   |dev - ref| <= 2^-8 (|ref| + E) + E,   E = eps * sum|term| (+ slack)
    f32 / f64 sums |dev - ref| <= E
2^-8 |ref| is the one rounding of the stored value (bf16 keeps 8 significant bits: half an ulp is 2^-8 of a value just above a
power of two -- the bound is tight there, and the worst ratios below sit at 0.99 for that reason), taken of the value the
device rounds, which is within E of ref (2^-8 E matters where a flipped operand moves a small result: found on one element
of 17.7 million at T = 5, 64 x 64, C = 216, stride 2, which sat at 1.0002 of the bound without it).  eps counts the f32 roundings in front of it:
  depthwise forward / data gradient   27 fma steps + the operand (one fma for relu(a scale + shift); two for db = cA t1 + cB +
                                      cC b, whose magnitude counts the three products separately): 30 u -> eps = 2^-19
  per-sample / BatchNorm_a sums       a lane adds its pixels of a walk in f32 (at most 64 tiles x 4 rows x 5 frames = 1280 values),
                                      then a 6-step wave tree, then f64 atomics: 1286 u -> eps = 2^-13 for the backward sums;
                                      the forward's walks are 16 tiles: 326 u -> eps = 2^-15.  Compared with float64 sums of the
                                      kernel's OWN stored output (which the element check has just tied to the reference).
  depthwise dW                        the same per-lane chain per tap, a workgroup tree, one f32 atomic per workgroup (at most
                                      2 x 256 of them land on one value): 1280 + 9 + 512 u -> eps = 2^-13
  GEMM outputs                        K <= 224 products added in f32 by the matrix cores: eps = 2^-16; the operands are bf16 values
                                      on both sides, so the products are exact.  slack: a converted operand whose f32 value lies
                                      within its own error of a bf16 rounding boundary may round the other way than float64; the
                                      restatement marks those (round_bf16(x, err)) and adds their ulp times |W|.  err: 2 fma and the
                                      SE-gate product (2^-22 of the magnitude), v_exp_f32 / v_rcp_f32 of the Swish at 1 ulp each with
                                      an argument error that grows with |q|, and the f32 gate itself (2^-18): 2^-17 of the value
  data gradients                      the product is staged in LDS as bf16 before the epilogue (one more rounding, restated with its own
                                      near-boundary ulp), then f32: + residual (1 u), or x swish'(q) gate, whose error is ABSOLUTE near the zero of swish'
                                      at q = -1.278: (1 + |q|)^2 2^-21 sigmoid(q) from v_exp_f32 / v_rcp_f32 and four roundings (derived in the restatement)
  GEMM statistics                     a lane adds at most 24 tiles x 4 passes in f32, 128 lanes are added per workgroup: 224 u ->
                                      eps = 2^-16; over the stored output, as above
  pointwise dW (M rows)               bf16 x bf16 products exact, f32 accumulation in the matrix cores along a workgroup's rows
                                      (M / workgroups / 32 k-steps of 32 rows, at most 192 steps at M = 1 572 864), then the reducer's
                                      f32 tree over <= 256 partials: 200 u -> eps = 2^-16, plus the slack of both operands
BatchNorm scale / shift / mean / rstd / running statistics are computed in f64 from the sums the test supplies and rounded to
f32 up to five times on the way (shift = beta - f32(mean) * f32(gamma * f32(rstd))): 8 u = 2^-21 of their magnitude.  The SE
gate is two f32 fma chains of at most 27 + 3 and 16 steps and an expf: 32 u of the pre-activations' magnitude sums (+ 1).
The worst error / bound of every case is printed (HOTPATH lines; run with -s).

Negative controls (one per family): the device gets an input that differs from the reference's in one place -- a tap scaled by
1 + 2^-5, an input row at a tile edge zeroed, one SE gate weight of one channel changed, one weight of the packed image -- in an
ordinary valid launch, and the same comparison must raise."""
import ctypes as C

import pytest
import torch

import hotpath_reference as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BF = torch.bfloat16
U = 2.0 ** -24
EPS_DW, EPS_DW_DW = R.EPS_DW, R.EPS_DW_DW          # 2^-19, 2^-13 (shared with the bf16 legs of the older depthwise tests)
EPS_DW_NC, EPS_DW_SUMS = 2.0 ** -15, 2.0 ** -13
EPS_GEMM, EPS_STATS, EPS_PW_DW = 2.0 ** -16, 2.0 ** -16, 2.0 ** -16
WORST = {}


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")


class Bound:
    """Collects error / bound of one case; `check()` raises at the end so that every output is reported."""

    def __init__(self, kernel, shape):
        self.kernel, self.shape, self.rows = kernel, shape, {}

    def add(self, what, dev, ref, mag, eps, rel=0.0, slack=None):
        dev, ref = dev.double(), ref.double()
        e = eps * mag if slack is None else eps * mag + slack
        lim = rel * (ref.abs() + e) + e           # the stored value is rounded from the DEVICE's f32 value, |ref| + e at most
        err = (dev - ref).abs()
        ratio = torch.where(err > 0, err / lim, torch.zeros_like(err))      # (an error where the bound is 0 is inf)
        ratio = torch.where(torch.isfinite(dev), ratio, torch.full_like(ratio, float("inf")))
        self.rows[what] = max(self.rows.get(what, 0.0), float(ratio.max()) if ratio.numel() else 0.0)

    def exact_zero(self, what, t):
        if t.numel():
            assert bool((t.float() == 0).all()), f"{self.kernel} {self.shape}: {what} must be exact zeros"

    def worst(self):
        return max(self.rows.values())

    def check(self, record=True):
        line = ", ".join(f"{k} {v:.3f}" for k, v in self.rows.items())
        if record:
            print(f"\nHOTPATH {self.kernel} | {self.shape} | error/bound: {line}")
            WORST[self.kernel] = max(WORST.get(self.kernel, 0.0), self.worst())
        assert self.worst() <= 1.0, f"bound exceeded: {self.kernel} {self.shape}: {line}"


def _randn(shape, seed, scale=1.0, dtype=torch.float32):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return (torch.randn(shape, generator=g, device=DEV, dtype=torch.float32) * scale).to(dtype)


def _padded(shape, c, seed, dtype=BF, absolute=False, scale=1.0):
    """[..., Cp] random tensor on the device in the storage type, padding channels zero."""
    t = _randn(shape, seed, scale)
    if absolute:
        t = t.abs()
    t[..., c:] = 0
    return t.to(dtype).contiguous()


def _cpu(t):
    return t.detach().cpu().double()


# ================================================================================================ depthwise
def _dw_pk(T, H, W, Cp, B, stride):
    if stride == 1:
        ih = 10 if T <= 3 else 6
        rel = (((T - 1) * H + ih) * W + 18) * Cp + Cp
        return rel < (1 << 22) and B * T * H * W * Cp < (1 << 31)
    rel = (((T - 1) * H + 9) * W + 33) * Cp + Cp
    return (rel >> 3) < (1 << 21) and B * T * H * W * Cp < (1 << 31)


def _b(v):
    return "true" if v else "false"


def dw_fwd_name(T, H, W, Cp, B, stride, hv_opt=5):
    pk = _dw_pk(T, H, W, Cp, B, stride)
    if stride == 1:
        return f"dw_fwd_v2_kernel<unsigned short, {T}, {_b(pk)}, {_b(T == 3 and hv_opt & 1)}>"
    if T <= 3:
        return f"dw_fwd_v2s2_kernel<unsigned short, 3, {_b(pk)}, {_b(hv_opt & 4)}>"
    return f"dw_fwd_kernel<unsigned short, 2, 4, 8, {T}>"


def dw_bwd_name(T, H, W, stride, ring_opt=13):
    if stride == 1 and (ring_opt & 1) and ((ring_opt & 8) or T > 3 or H * W >= 64 * 64):
        return f"dw_bwd_ring_kernel<{T}, {_b(ring_opt & 4)}>"
    return f"dw_bwd_fused_kernel<unsigned short, {T}, {stride}>"


def run_dw(B, T, H, W, C, stride, hv_opt=5, tamper=None, seed=1000):
    """c3d_dw333_fwd, then c3d_dw333_bwd_fused on the forward's own output, each against float64, sample by sample."""
    from change3d_amd import ops
    Cp = ops.cpad(C)
    Ho, Wo = R.dw_out_hw(H, W, stride)
    shape = f"B {B} T {T} {H}x{W} C {C} stride {stride}"
    a = _padded((B, T, H, W, Cp), C, seed)
    scale, shift = _randn((Cp,), seed + 1).abs() + 0.5, _randn((Cp,), seed + 2, 0.3)
    scale[C:], shift[C:] = 0, 0
    w = _randn((C, 27), seed + 3, 0.3)
    t1 = _padded((B, T, Ho, Wo, Cp), C, seed + 4, absolute=True)       # one sign: dW and the sums are coherent, not a random walk
    cA, cC = _randn((Cp,), seed + 5).abs() + 0.25, _randn((Cp,), seed + 6, 0.1)
    cB = _randn((B, Cp), seed + 7, 0.1)
    mean, rstd = _randn((Cp,), seed + 8, 0.5), _randn((Cp,), seed + 9).abs() + 0.5
    for v in (cA, cC, cB, mean, rstd):
        v[..., C:] = 0
    ss, mr = torch.cat([scale, shift]).contiguous(), torch.cat([mean, rstd]).contiguous()
    ref = dict(w=_cpu(w), scale=_cpu(scale[:C]), shift=_cpu(shift[:C]), cA=_cpu(cA[:C]), cC=_cpu(cC[:C]), cB=_cpu(cB[:, :C]),
               mean=_cpu(mean[:C]), rstd=_cpu(rstd[:C]))
    a_ref = a if tamper is None else a.clone()      # what the reference sees; `tamper` changes what the device gets
    if tamper is not None:
        tamper(dict(a=a, w=w))
    y = torch.full((B, T, Ho, Wo, Cp), float("nan"), dtype=BF, device=DEV)
    nc = torch.zeros(B * Cp * 2, dtype=torch.float64, device=DEV)
    t2 = torch.full((B, T, H, W, Cp), float("nan"), dtype=BF, device=DEV)
    ds = torch.zeros(2 * C, dtype=torch.float64, device=DEV)
    dw = torch.zeros((C, 27), dtype=torch.float32, device=DEV)
    try:
        ops.set_option(ops.OPT_DW_FWD_HV, hv_opt)
        ops.dw_fwd(a, ss, w, y, nc, B, T, H, W, C, stride, ops.DT_BF16)
        kf = ops.last_kernel()
    finally:
        ops.set_option(ops.OPT_DW_FWD_HV, 5)
    torch.cuda.synchronize()
    ops.dw_bwd_fused(t1, y, cA, cB.contiguous(), cC, w, a, ss, mr, t2, ds, dw, B, T, H, W, C, ops.DT_BF16, stride)
    kb = ops.last_kernel()
    torch.cuda.synchronize()
    assert kf == dw_fwd_name(T, H, W, Cp, B, stride, hv_opt), kf
    assert kb == dw_bwd_name(T, H, W, stride), kb
    bf, bb = Bound(kf, shape), Bound(kb, shape)
    bf.exact_zero("padding channels of y", y[..., C:])
    bb.exact_zero("padding channels of t2", t2[..., C:])
    ncd = _cpu(nc).view(B, Cp, 2)
    assert bool((ncd[:, C:] == 0).all())
    dw_ref = torch.zeros(C, 27, dtype=torch.float64)
    dw_mag = torch.zeros_like(dw_ref)
    ds_ref = torch.zeros(2, C, dtype=torch.float64)
    ds_mag = torch.zeros_like(ds_ref)
    for n in range(B):
        an, yn, t1n, t2n = _cpu(a_ref[n, ..., :C]), _cpu(y[n, ..., :C]), _cpu(t1[n, ..., :C]), _cpu(t2[n, ..., :C])
        yr, ym, ysl = R.dw_fwd_sample(an, ref["scale"], ref["shift"], ref["w"], stride, round_operand=kf.startswith("dw_fwd_kernel<"))
        bf.add("y", yn, yr, ym, EPS_DW, rel=R.BF16_EPS, slack=ysl)
        s, sm = R.sample_sums(yn)
        bf.add("nc", ncd[n, :C], s, sm, EPS_DW_NC)
        t2r, t2m, dwn, dwm = R.dw_bwd_sample(t1n, yn, ref["cA"], ref["cB"][n], ref["cC"], ref["w"], an, ref["scale"], ref["shift"], stride)
        bb.add("t2", t2n, t2r, t2m, EPS_DW, rel=R.BF16_EPS)
        dw_ref += dwn
        dw_mag += dwm
        d, dm = R.bn_a_bwd_sums(t2n, an, ref["mean"], ref["rstd"])
        ds_ref += d
        ds_mag += dm
    bb.add("dsums", _cpu(ds).view(2, C), ds_ref, ds_mag, EPS_DW_SUMS)
    bb.add("dW", _cpu(dw), dw_ref, dw_mag, EPS_DW_DW)
    return bf, bb


def _check(*bounds):
    failed = []
    for b in bounds:
        try:
            b.check()
        except AssertionError as e:
            failed.append(str(e))
    assert not failed, "\n".join(failed)


# group A: the BCD benchmark step
@pytest.mark.parametrize("H,C,stride", [(128, 54, 1), (64, 108, 1), (32, 216, 1), (256, 54, 2), (128, 108, 2), (64, 216, 2)])
def test_depthwise_pair_at_the_bcd_benchmark_shapes(H, C, stride):
    _need_gpu()
    _check(*run_dw(32, 3, H, H, C, stride))


# group B: SCD (five frames, B = 16) and BDA (four frames, B = 8) at the same six stage shapes
@pytest.mark.parametrize("B,T", [(16, 5), (8, 4)])
@pytest.mark.parametrize("H,C,stride", [(128, 54, 1), (64, 108, 1), (32, 216, 1), (256, 54, 2), (128, 108, 2), (64, 216, 2)])
def test_depthwise_pair_at_the_scd_and_bda_shapes(B, T, H, C, stride):
    _need_gpu()
    _check(*run_dw(B, T, H, H, C, stride))


# group C: edges
@pytest.mark.parametrize("B,T,H,W,C,stride,hv", [
    (3, 3, 17, 19, 54, 1, 5), (3, 3, 17, 19, 54, 2, 5), (2, 3, 15, 9, 108, 1, 1), (2, 3, 15, 9, 108, 2, 1),   # no tile multiples
    (2, 3, 8, 72, 24, 1, 5), (2, 3, 8, 72, 24, 2, 4),        # a single tile row; C = 24: one short chunk
    (300, 3, 8, 8, 54, 1, 5),                                 # one tile per sample: a walk runs over more than 8 samples
    (40, 3, 24, 24, 54, 1, 0), (40, 3, 24, 24, 54, 2, 0),     # walks cross sample boundaries; option 0: 8-channel lanes, four waves
    (5, 3, 20, 28, 216, 1, 4), (5, 3, 20, 28, 216, 2, 1),     # seven chunks, the last vector empty
    (1, 3, 256, 256, 54, 1, 5),                               # tile-relative offsets past 2^22 elements: PK = false on bf16
    (3, 5, 17, 19, 54, 1, 5), (3, 4, 17, 19, 54, 2, 5),       # the four- and five-frame instantiations on ragged maps
])
def test_depthwise_pair_edges(B, T, H, W, C, stride, hv):
    _need_gpu()
    from change3d_amd import ops
    bf, bb = run_dw(B, T, H, W, C, stride, hv_opt=hv)
    if (B, H, C, stride) == (1, 256, 54, 1):
        assert bf.kernel == "dw_fwd_v2_kernel<unsigned short, 3, false, true>", bf.kernel
    _check(bf, bb)
    assert ops.OPT_DW_FWD_HV == 8


def _scale_one_tap(d):
    d["w"][17, 13] *= 1 + 2.0 ** -5          # one tap of one channel


def _zero_an_edge_row(d):
    d["a"][1, 1, 8, :, :] = 0                # the first input row of the second tile row (8-row tiles), one frame of one sample


@pytest.mark.parametrize("tamper", [_scale_one_tap, _zero_an_edge_row])
@pytest.mark.parametrize("stride", [1, 2])
def test_depthwise_bound_sees_a_wrong_tap_and_a_missing_edge_row(stride, tamper):
    """Negative control: the device's input differs from the reference's in one place; forward AND backward must be rejected."""
    _need_gpu()
    bf, bb = run_dw(2, 3, 32, 32, 54, stride, tamper=tamper)
    print(f"\nHOTPATH-NEG {tamper.__name__} stride {stride}: forward {bf.kernel} error/bound {bf.worst():.2f}, backward {bb.kernel} {bb.worst():.2f}")
    for b in (bf, bb):
        with pytest.raises(AssertionError, match="bound exceeded"):
            b.check(record=False)


# ================================================================================================ pointwise forward
def _fin(gamma, beta, rm, rv, nbt, ss, mr, count, batch, sums):
    from change3d_amd import _lib as L
    f = L.BnFin()
    f.gamma, f.beta, f.running_mean, f.running_var, f.nbt, f.ss, f.mr = (t.data_ptr() for t in (gamma, beta, rm, rv, nbt, ss, mr))
    f.count, f.momentum, f.eps, f.training, f.batch, f.sums = float(count), 0.1, 1e-5, 1, batch, sums.data_ptr()
    return f


def _bn_checks(bd, out, ss, mr, rm, rv, K, Kp, rm0, rv0):
    bn = out["bn"]
    t = 2.0 ** -21
    bd.add("scale", _cpu(ss[:K]), bn["scale"], bn["scale"].abs(), t)
    bd.add("shift", _cpu(ss[Kp:Kp + K]), bn["shift"], (bn["mean"] * bn["scale"]).abs() + (bn["shift"] + bn["mean"] * bn["scale"]).abs(), t)
    bd.add("mean", _cpu(mr[:K]), bn["mean"], bn["mean"].abs(), t)
    bd.add("rstd", _cpu(mr[Kp:Kp + K]), bn["rstd"], bn["rstd"].abs(), t)
    bd.add("running_mean", _cpu(rm), bn["running_mean"], rm0.abs() + bn["mean"].abs(), t)
    bd.add("running_var", _cpu(rv), bn["running_var"], bn["running_var"].abs(), t)
    bd.exact_zero("padding of scale / shift", torch.cat([ss[K:Kp], ss[Kp + K:]]))


def _pw_tiles(K, N, conv_a):
    ntn = (N + 7) // 8 * 8
    ntn = (ntn + 15) // 16
    ks = ((K + 7) // 8 * 8 + 31) // 32
    if conv_a:
        return (2, 7 if ntn > 4 else 4, ks)
    return (1, 3 if ntn > 3 else max(ntn, 2), ks)


def run_conv_c(K, N, B, rps, se=True, tamper=None, seed=2000):
    from change3d_amd import ops, _lib as L
    Kp, Np, M, Cr = ops.cpad(K), ops.cpad(N), B * rps, 16
    shape = f"{K} -> {N} M {M} ({B} x {rps}) {'SE' if se else 'no SE'}"
    x = _padded((M, Kp), K, seed)
    w = _randn((N, K), seed + 1, 0.1)
    gamma, beta = _randn((K,), seed + 2).abs() + 0.5, _randn((K,), seed + 3, 0.2)
    w1, b1, w2, b2 = _randn((Cr, K), seed + 4, 0.1), _randn((Cr,), seed + 5, 0.1), _randn((K, Cr), seed + 6, 0.3), _randn((K,), seed + 7, 0.1)
    rm, rv = _randn((K,), seed + 8, 0.3), _randn((K,), seed + 9).abs() + 0.5
    rm0, rv0 = _cpu(rm), _cpu(rv)
    xs = x.view(B, rps, Kp).double()
    nc = torch.stack([xs.sum(1), (xs * xs).sum(1)], dim=2).contiguous()        # [B][Kp][2], as c3d_dw333_fwd leaves them
    ref_in = dict(w=_cpu(w), w2=_cpu(w2))
    img = torch.empty(ops.pw_weight_image_bytes(N, K, ops.DT_BF16), dtype=torch.uint8, device=DEV)
    if tamper is not None:
        tamper(dict(w=w, w2=w2))
    ops.pw_pack_weights([(w, img, N, K, K, 1)], ops.DT_BF16)
    y = torch.full((M, Np), float("nan"), dtype=BF, device=DEV)
    stats = torch.zeros(ops.STAT_STRIPES * 2 * N, dtype=torch.float64, device=DEV)
    nbt = torch.zeros(1, dtype=torch.int64, device=DEV)
    ss, mr = torch.full((2 * Kp,), float("nan"), device=DEV), torch.full((2 * Kp,), float("nan"), device=DEV)
    gate, hid = torch.full((B, Kp), float("nan"), device=DEV), torch.full((B, Cr), float("nan"), device=DEV)
    a = L.PwArgs()
    a.x, a.y, a.w, a.w_img = x.data_ptr(), y.data_ptr(), w.data_ptr(), img.data_ptr()
    a.M, a.K, a.Kp, a.N, a.Np, a.w_sn, a.w_sk = M, K, Kp, N, Np, K, 1
    a.rows_per_sample, a.dtype = rps, ops.DT_BF16
    a.pro_mode, a.epi_mode = ops.PRO_BN_SE_SWISH, ops.EPI_STATS
    a.pro_p, a.stats = ss.data_ptr(), stats.data_ptr()
    a.fin = _fin(gamma, beta, rm, rv, nbt, ss, mr, M, B, nc)
    if se:
        a.pro_gate = gate.data_ptr()
        a.se_w1, a.se_b1, a.se_w2, a.se_b2, a.se_hid, a.se_cr = w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), b2.data_ptr(), hid.data_ptr(), Cr
    rc = L.lib().c3d_pw_gemm(C.byref(a), ops._stream())
    k = ops.last_kernel()
    torch.cuda.synchronize()
    assert rc == 0, rc
    assert k == "pw_cfwd_kernel<%d, %d, %d, true>" % _pw_tiles(K, N, False), k
    bd = Bound(k, shape)
    bd.exact_zero("padding channels of y", y[:, N:])
    assert int(nbt) == 1
    out = R.conv_c_fwd(_cpu(x[:, :K]), _cpu(nc[:, :K]), rps, _cpu(gamma), _cpu(beta), 1e-5, ref_in["w"],
                       se=(_cpu(w1), _cpu(b1), ref_in["w2"], _cpu(b2)) if se else None, running=(rm0, rv0))
    _bn_checks(bd, out, ss, mr, rm, rv, K, Kp, rm0, rv0)
    if se:
        bd.add("hid", _cpu(hid), out["hid"], out["se_mag"]["hid_mag"], 32 * U)
        bd.add("gate", _cpu(gate[:, :K]), out["gate"], 1.0 + out["se_mag"]["gate_mag"], 32 * U)
        bd.exact_zero("padding channels of the gate", gate[:, K:])
    yd = _cpu(y[:, :N])
    bd.add("y", yd, out["y"], out["mag"], EPS_GEMM, rel=R.BF16_EPS, slack=out["slack"])
    s, sm = R.col_stats(yd)
    bd.add("stats", _cpu(stats).view(ops.STAT_STRIPES, 2, N).sum(0), s, sm, EPS_STATS)
    return bd


def run_conv_a(K, N, M, tamper=None, seed=3000):
    from change3d_amd import ops, _lib as L
    Kp, Np = ops.cpad(K), ops.cpad(N)
    shape = f"{K} -> {N} M {M} residual prologue"
    c, sc = _padded((M, Kp), K, seed), _padded((M, Kp), K, seed + 1)
    w = _randn((N, K), seed + 2, 0.1)
    gamma, beta = _randn((K,), seed + 3).abs() + 0.5, _randn((K,), seed + 4, 0.2)
    rm, rv = _randn((K,), seed + 5, 0.3), _randn((K,), seed + 6).abs() + 0.5
    rm0, rv0 = _cpu(rm), _cpu(rv)
    cd = c[:, :K].double()
    tot = torch.stack([cd.sum(0), (cd * cd).sum(0)])                            # [2][K]
    g = torch.Generator(device=DEV).manual_seed(seed + 7)
    frac = torch.rand(ops.STAT_STRIPES, 1, 1, dtype=torch.float64, device=DEV, generator=g) + 0.1
    sums = (tot[None] * frac / frac.sum()).contiguous()                         # [stripes][2][K], as the producer's epilogue leaves them
    w_ref = _cpu(w)
    if tamper is not None:
        tamper(dict(w=w))
    img = torch.empty(ops.pw_weight_image_bytes(N, K, ops.DT_BF16), dtype=torch.uint8, device=DEV)
    ops.pw_pack_weights([(w, img, N, K, K, 1)], ops.DT_BF16)
    y = torch.full((M, Np), float("nan"), dtype=BF, device=DEV)
    po = torch.full((M, Kp), float("nan"), dtype=BF, device=DEV)
    stats = torch.zeros(ops.STAT_STRIPES * 2 * N, dtype=torch.float64, device=DEV)
    nbt = torch.zeros(1, dtype=torch.int64, device=DEV)
    ss, mr = torch.full((2 * Kp,), float("nan"), device=DEV), torch.full((2 * Kp,), float("nan"), device=DEV)
    a = L.PwArgs()
    a.x, a.x2, a.y, a.w, a.w_img, a.pro_out = (t.data_ptr() for t in (c, sc, y, w, img, po))
    a.M, a.K, a.Kp, a.N, a.Np, a.w_sn, a.w_sk = M, K, Kp, N, Np, K, 1
    a.dtype = ops.DT_BF16
    a.pro_mode, a.epi_mode = ops.PRO_AFFINE2, ops.EPI_STATS
    a.pro_p, a.stats = ss.data_ptr(), stats.data_ptr()
    a.fin = _fin(gamma, beta, rm, rv, nbt, ss, mr, M, 0, sums)
    rc = L.lib().c3d_pw_gemm(C.byref(a), ops._stream())
    k = ops.last_kernel()
    torch.cuda.synchronize()
    assert rc == 0, rc
    assert k == "pw_cfwd_kernel<%d, %d, %d, true>" % _pw_tiles(K, N, True), k
    bd = Bound(k, shape)
    bd.exact_zero("padding channels of y", y[:, N:])
    bd.exact_zero("padding channels of pro_out", po[:, K:])
    assert int(nbt) == 1
    out = R.conv_a_fwd(_cpu(c[:, :K]), _cpu(sc[:, :K]), _cpu(sums.sum(0)), _cpu(gamma), _cpu(beta), 1e-5, w_ref, running=(rm0, rv0))
    _bn_checks(bd, out, ss, mr, rm, rv, K, Kp, rm0, rv0)
    # the residual output: bn_c(c) by one fma, the add, ReLU, one bf16 rounding
    bd.add("pro_out", _cpu(po[:, :K]), out["po"], out["po_mag"], 4 * U, rel=R.BF16_EPS)
    yd = _cpu(y[:, :N])
    bd.add("y", yd, out["y"], out["mag"], EPS_GEMM, rel=R.BF16_EPS, slack=out["slack"])
    s, sm = R.col_stats(yd)
    bd.add("stats", _cpu(stats).view(ops.STAT_STRIPES, 2, N).sum(0), s, sm, EPS_STATS)
    return bd


# group A (rows per sample = M / 32: 49 152 / 12 288 / 3 072), SE blocks and blocks without (every second block of a stage)
@pytest.mark.parametrize("K,N,rps,se", [(54, 24, 49152, True), (108, 48, 12288, True), (216, 96, 3072, True), (216, 96, 3072, False),
                                        (54, 24, 49152, False)])
def test_conv_c_forward_at_the_bcd_benchmark_shapes(K, N, rps, se):
    _need_gpu()
    _check(run_conv_c(K, N, 32, rps, se))


@pytest.mark.parametrize("K,N,M", [(24, 54, 1572864), (48, 108, 393216), (96, 216, 98304)])
def test_conv_a_forward_at_the_bcd_benchmark_shapes(K, N, M):
    _need_gpu()
    _check(run_conv_a(K, N, M))


# group C.  conv_c: 216 -> 96 walks 64-row tiles, the narrower layers 128-row tiles; the kernel refuses M < 1024, rows per sample
# under a tile and more than four samples per workgroup.  With W workgroups at most (256 compute units, twice that for 54 -> 24)
# tiles_per_wg is 2 up to 2 W tiles and 3 from 2 W + 1 tiles on.
@pytest.mark.parametrize("K,N,B,rps,se", [
    (216, 96, 1, 1024, True),        # M at the floor: 16 tiles, 8 workgroups of 2
    (216, 96, 3, 352, True),         # M 1056: samples end inside a tile (352 = 5.5 tiles), a workgroup spans two samples
    (108, 48, 5, 208, True),         # ragged last tile (1040 = 8 tiles + 16 rows), samples end inside tiles
    (54, 24, 3, 1360, False),        # ragged last tile, no SE
    (216, 96, 3, 10928, True),       # 513 tiles of 64 rows: the smallest count with tiles_per_wg 3
    (216, 96, 2, 16384, True),       # 512 tiles: the largest with tiles_per_wg 2
])
def test_conv_c_forward_edges(K, N, B, rps, se):
    _need_gpu()
    _check(run_conv_c(K, N, B, rps, se))


@pytest.mark.parametrize("K,N,M", [(96, 216, 1024), (96, 216, 1031), (48, 108, 2345), (24, 54, 1029), (48, 108, 65536), (48, 108, 65537),
                                   (96, 216, 32769)])
def test_conv_a_forward_edges(K, N, M):
    """M at and just above the 1024 floor, ragged last tiles, 512 tiles of 128 rows (the largest count with tiles_per_wg 2), 513
    (the smallest with 3), and 513 tiles of the 216-wide layer's 64 rows."""
    _need_gpu()
    _check(run_conv_a(K, N, M))


def _change_one_gate_weight(d):
    d["w2"][5, 3] += 0.5             # the gate of channel 5 moves in every sample


def _change_one_weight(d):
    d["w"][7, 11] *= 1 + 2.0 ** -3   # one element of the packed image (an eighth: bf16 keeps 8 bits)


def test_conv_c_bound_sees_a_changed_gate_and_a_changed_weight():
    _need_gpu()
    for tamper in (_change_one_gate_weight, _change_one_weight):
        bd = run_conv_c(108, 48, 4, 1024, True, tamper=tamper)
        print(f"\nHOTPATH-NEG {tamper.__name__}: {bd.kernel} error/bound {bd.worst():.2f}")
        with pytest.raises(AssertionError, match="bound exceeded"):
            bd.check(record=False)


def test_conv_a_bound_sees_a_changed_weight():
    _need_gpu()
    bd = run_conv_a(48, 108, 4096, tamper=_change_one_weight)
    print(f"\nHOTPATH-NEG _change_one_weight: {bd.kernel} error/bound {bd.worst():.2f}")
    with pytest.raises(AssertionError, match="bound exceeded"):
        bd.check(record=False)


# ================================================================================================ pointwise data gradients
def run_conv_a_dgrad(Ci, Cin, M, tamper=None, seed=5000):
    """conv_a data + weight gradient on the cooperative kernel, with the ReLU mask of the block's input and the folded
    BatchNorm_c-backward sums of the block below, as c3d_stage_bwd issues it."""
    from change3d_amd import ops
    Cip, Cinp = ops.cpad(Ci), ops.cpad(Cin)
    shape = f"{Ci} -> {Cin} M {M}"
    t2, a_ = _padded((M, Cip), Ci, seed), _padded((M, Cip), Ci, seed + 1)
    A, Bc, Cc = _randn((Cip,), seed + 2), _randn((Cip,), seed + 3, 0.1), _randn((Cip,), seed + 4, 0.1)
    for v in (A, Bc, Cc):
        v[Ci:] = 0
    w = _randn((Ci, Cin), seed + 5, 0.2)
    y_prev = torch.relu(_padded((M, Cinp), Cin, seed + 6))
    res, cten = _padded((M, Cinp), Cin, seed + 7), _padded((M, Cinp), Cin, seed + 8)
    mean, rstd = _randn((Cinp,), seed + 9, 0.5), _randn((Cinp,), seed + 10).abs() + 0.5
    w_ref = _cpu(w)
    if tamper is not None:
        tamper(dict(w=w))
    img = torch.zeros(ops.pw_weight_image_bytes(Cin, Ci, ops.DT_BF16), dtype=torch.uint8, device=DEV)
    ops.pw_pack_weights([(w, img, Cin, Ci, 1, Cin)], ops.DT_BF16)
    dx = torch.full((M, Cinp), float("nan"), dtype=BF, device=DEV)
    dw = torch.ones((Ci, Cin), dtype=torch.float32, device=DEV)          # += onto ones
    sums = torch.zeros(2 * Cin, dtype=torch.float64, device=DEV)
    ops.pw_gemm(t2, w, dx, M=M, K=Ci, N=Cin, w_sn=1, w_sk=Cin, dtype=ops.DT_BF16, x2=a_, pro_mode=ops.PRO_AFFINE2,
                pro_p=torch.cat([A, Bc, Cc]).contiguous(), epi_mode=ops.EPI_ADD, e1=res, w_img=img, wg_mode=ops.WG_ROWS, wg_dw=dw,
                wg_x3=y_prev, wg_mask_out=1, add_c=cten, add_mr=torch.cat([mean, rstd]).contiguous(), add_sums=sums)
    k = ops.last_kernel()
    torch.cuda.synchronize()
    assert k.startswith("pw_cdg_a_kernel<"), k
    bd = Bound(k, shape)
    bd.exact_zero("padding channels of dx", dx[:, Cin:])
    coef = (_cpu(A[:Ci]), _cpu(Bc[:Ci]), _cpu(Cc[:Ci]))
    dwr, dwm, dws = (torch.zeros(Ci, Cin, dtype=torch.float64) for _ in range(3))
    sr, sm = torch.zeros(2, Cin, dtype=torch.float64), torch.zeros(2, Cin, dtype=torch.float64)
    for r0 in range(0, M, 1 << 16):
        r = slice(r0, min(M, r0 + (1 << 16)))
        yp = _cpu(y_prev[r, :Cin])
        o = R.conv_a_dgrad(_cpu(t2[r, :Ci]), _cpu(a_[r, :Ci]), coef, w_ref, _cpu(res[r, :Cin]), y_prev=yp, eps=EPS_GEMM)
        dxd = _cpu(dx[r, :Cin])
        bd.add("dx", dxd, o["dx"], o["err"], 1.0, rel=R.BF16_EPS)
        d, m = R.wgrad(o["P"], yp)
        dwr += d
        dwm += m
        dws += o["P_slack"].t() @ yp
        d, m = R.bn_bwd_sums(dxd, _cpu(cten[r, :Cin]), _cpu(mean[:Cin]), _cpu(rstd[:Cin]))
        sr += d
        sm += m
    bd.add("add_sums", _cpu(sums).view(2, Cin), sr, sm, EPS_STATS)
    bd.add("dW", _cpu(dw) - 1.0, dwr, dwm + 1.0, EPS_PW_DW, slack=dws)
    return bd


def run_conv_c_dgrad(Co, Ci, B, rows, gated=True, tamper=None, seed=6000):
    """conv_c data + weight gradient on the cooperative kernel: Swish / SE backward epilogue, per-sample sums nc3."""
    from change3d_amd import ops
    Cop, Cip, M = ops.cpad(Co), ops.cpad(Ci), B * rows
    shape = f"{Co} -> {Ci} M {M} ({B} x {rows}) {'SE' if gated else 'no SE'}"
    g, c, b = _padded((M, Cop), Co, seed), _padded((M, Cop), Co, seed + 1), _padded((M, Cip), Ci, seed + 2)
    A, Bc, Cc = _randn((Cop,), seed + 3), _randn((Cop,), seed + 4, 0.1), _randn((Cop,), seed + 5, 0.1)
    scale, shift = _randn((Cip,), seed + 6).abs() + 0.5, _randn((Cip,), seed + 7, 0.3)
    mean, rstd = _randn((Cip,), seed + 8, 0.5), _randn((Cip,), seed + 9).abs() + 0.5
    gate = torch.sigmoid(_randn((B, Cip), seed + 10))
    for v in (A, Bc, Cc):
        v[Co:] = 0
    for v in (scale, shift, mean, rstd, gate):
        v[..., Ci:] = 0
    w = _randn((Co, Ci), seed + 11, 0.2)
    w_ref = _cpu(w)
    if tamper is not None:
        tamper(dict(w=w))
    img = torch.zeros(ops.pw_weight_image_bytes(Ci, Co, ops.DT_BF16), dtype=torch.uint8, device=DEV)
    ops.pw_pack_weights([(w, img, Ci, Co, 1, Ci)], ops.DT_BF16)
    t1 = torch.full((M, Cip), float("nan"), dtype=BF, device=DEV)
    nc3 = torch.zeros(B * Cip * 3, dtype=torch.float64, device=DEV)
    dw = torch.ones((Co, Ci), dtype=torch.float32, device=DEV)
    ops.pw_gemm(g, w, t1, M=M, K=Co, N=Ci, w_sn=1, w_sk=Ci, dtype=ops.DT_BF16, x2=c, pro_mode=ops.PRO_AFFINE2,
                pro_p=torch.cat([A, Bc, Cc]).contiguous(), epi_mode=ops.EPI_SWISH_SE_BWD, e1=b, epi_p=torch.cat([scale, shift]).contiguous(),
                epi_gate=gate.contiguous() if gated else None, epi_q=torch.cat([mean, rstd]).contiguous(), rows_per_sample=rows, w_img=img,
                stats=nc3, wg_mode=ops.WG_SWISH, wg_dw=dw)
    k = ops.last_kernel()
    torch.cuda.synchronize()
    assert k.startswith("pw_cdg_c_kernel<"), k
    bd = Bound(k, shape)
    bd.exact_zero("padding channels of t1", t1[:, Ci:])
    coef = (_cpu(A[:Co]), _cpu(Bc[:Co]), _cpu(Cc[:Co]))
    ncd = _cpu(nc3).view(B, Cip, 3)
    dwr, dwm, dws = (torch.zeros(Co, Ci, dtype=torch.float64) for _ in range(3))
    for n in range(B):
        r = slice(n * rows, (n + 1) * rows)
        bn = _cpu(b[r, :Ci])
        o = R.conv_c_dgrad(_cpu(g[r, :Co]), _cpu(c[r, :Co]), coef, w_ref, bn, _cpu(scale[:Ci]), _cpu(shift[:Ci]),
                           _cpu(gate[n, :Ci]) if gated else None, eps=EPS_GEMM)
        t1d = _cpu(t1[r, :Ci])
        bd.add("t1", t1d, o["t1"], o["err"], 1.0, rel=R.BF16_EPS)
        bd.add("nc3 d gate", ncd[n, :Ci, 0], o["dgate"], o["dgate_err"] + EPS_STATS * o["dgate_mag"], 1.0)
        d, m = R.bn_bwd_sums(t1d, bn, _cpu(mean[:Ci]), _cpu(rstd[:Ci]))
        bd.add("nc3 sums", ncd[n, :Ci, 1:].t(), d, m, EPS_STATS)
        d, m = R.wgrad(o["P"], o["Q"])
        dwr += d
        dwm += m
        dws += o["P_slack"].t() @ o["Q"].abs() + o["P"].abs().t() @ o["Q_slack"]
    bd.add("dW", _cpu(dw) - 1.0, dwr, dwm + 1.0, EPS_PW_DW, slack=dws)
    return bd


@pytest.mark.parametrize("Ci,Cin,M", [(54, 24, 1572864), (108, 48, 393216), (216, 96, 98304)])
def test_conv_a_gradient_at_the_bcd_benchmark_shapes(Ci, Cin, M):
    _need_gpu()
    _check(run_conv_a_dgrad(Ci, Cin, M))


@pytest.mark.parametrize("Co,Ci,rows,gated", [(24, 54, 49152, True), (48, 108, 12288, True), (96, 216, 3072, True), (96, 216, 3072, False)])
def test_conv_c_gradient_at_the_bcd_benchmark_shapes(Co, Ci, rows, gated):
    _need_gpu()
    _check(run_conv_c_dgrad(Co, Ci, 32, rows, gated))


# edges: M at the kernels' 1024 floor, ragged last tiles (conv_a), a workgroup spanning samples (conv_c: rows_per_sample must be a
# multiple of the tile's rows, 64 here and 128 on the narrower layers)
@pytest.mark.parametrize("Ci,Cin,M", [(216, 96, 1024), (216, 96, 4993), (108, 48, 4791), (54, 24, 6397)])
def test_conv_a_gradient_edges(Ci, Cin, M):
    _need_gpu()
    _check(run_conv_a_dgrad(Ci, Cin, M))


@pytest.mark.parametrize("Co,Ci,B,rows,gated", [(96, 216, 37, 64, True), (96, 216, 1, 1024, False), (48, 108, 11, 256, True), (24, 54, 9, 256, True)])
def test_conv_c_gradient_edges(Co, Ci, B, rows, gated):
    _need_gpu()
    _check(run_conv_c_dgrad(Co, Ci, B, rows, gated))


def test_data_gradient_bounds_see_a_changed_weight():
    _need_gpu()
    for bd in (run_conv_a_dgrad(108, 48, 4096, tamper=_change_one_weight), run_conv_c_dgrad(48, 108, 4, 1024, tamper=_change_one_weight)):
        print(f"\nHOTPATH-NEG _change_one_weight: {bd.kernel} error/bound {bd.worst():.2f}")
        with pytest.raises(AssertionError, match="bound exceeded"):
            bd.check(record=False)


# ================================================================================================ pointwise weight gradient
def run_wgrad_v2(K, N, B, rows, mode, ragged=0, tamper=None, seed=4000):
    """c3d_pw_wgrad on the flat-staged kernel: dW[N][K] += P^T Q, P = A p + B + C p2 (BatchNorm backward on load) or plain,
    Q = swish(gate (x scale + shift)) (conv_c), or plain rows (conv_a: the stored residual output)."""
    from change3d_amd import ops
    Kp, Np, M = ops.cpad(K), ops.cpad(N), B * rows - ragged
    shape = f"dW[{N}][{K}] M {M} ({B} x {rows}) {mode}"
    p, p2, x = _padded((M, Np), N, seed), _padded((M, Np), N, seed + 1), _padded((M, Kp), K, seed + 2)
    A, Bc, Cc = _randn((Np,), seed + 3), _randn((Np,), seed + 4, 0.1), _randn((Np,), seed + 5, 0.1)
    scale, shift = _randn((Kp,), seed + 6).abs() + 0.5, _randn((Kp,), seed + 7, 0.3)
    gate = torch.sigmoid(_randn((B, Kp), seed + 8))
    for v in (A, Bc, Cc):
        v[N:] = 0
    for v in (scale, shift, gate):
        v[..., K:] = 0
    kw = dict(M=M, K=K, N=N, dw_sn=K, dw_sk=1, dtype=ops.DT_BF16)
    x_ref = x if tamper is None else x.clone()
    if tamper is not None:
        tamper(dict(x=x))
    if mode != "plain":
        kw.update(p2=p2, p_coef=torch.cat([A, Bc, Cc]).contiguous())
    if mode.startswith("swish"):
        kw.update(q_mode=ops.PRO_BN_SE_SWISH, q_ss=torch.cat([scale, shift]).contiguous(), rows_per_sample=rows)
        if mode == "swish_gate":
            kw.update(q_gate=gate.contiguous())
    ref, mag, slack = (torch.zeros(N, K, dtype=torch.float64) for _ in range(3))
    for n in range(B):                                       # the float64 product, sample by sample
        r0, r1 = n * rows, min(M, (n + 1) * rows)
        P, Q = _cpu(p[r0:r1, :N]), _cpu(x_ref[r0:r1, :K])
        ps = qs = None
        if mode != "plain":
            P, ps = R.affine2_operand(P, _cpu(p2[r0:r1, :N]), _cpu(A[:N]), _cpu(Bc[:N]), _cpu(Cc[:N]))
        if mode.startswith("swish"):
            Q, qs = R.swish_operand(Q, _cpu(scale[:K]), _cpu(shift[:K]), _cpu(gate[n, :K]) if mode == "swish_gate" else None)
        d, m = R.wgrad(P, Q)
        ref += d
        mag += m
        if ps is not None:
            slack += ps.t() @ Q.abs()
        if qs is not None:
            slack += P.abs().t() @ qs
    dw = torch.full((N, K), 0.5, dtype=torch.float32, device=DEV)          # accumulate semantics (+=)
    ops.pw_wgrad(p, x, dw, **kw)
    k = ops.last_kernel()
    torch.cuda.synchronize()
    assert k.startswith("pw_wgrad_v2_kernel<%s, %s, " % (_b(mode != "plain"), _b(mode.startswith("swish")))), k
    bd = Bound(k, shape)
    bd.add("dW", _cpu(dw) - 0.5, ref, mag + 0.5, EPS_PW_DW, slack=slack)
    return bd


# what the BCD step still launches on this kernel: the weight gradients the cooperative data-gradient kernels do not fuse run
# here only where those kernels refuse a layer; the stage driver's separate launches have these operand forms at the stage
# shapes (conv_c: swish operand, gated in SE blocks and ungated in the others; conv_a: affine operand against stored rows)
@pytest.mark.parametrize("K,N,B,rows,mode", [
    (216, 96, 32, 3072, "swish_gate"), (216, 96, 32, 3072, "swish_nogate"), (96, 216, 32, 3072, "affine2"),
    (108, 48, 32, 12288, "swish_gate"), (48, 108, 32, 12288, "affine2"), (54, 24, 32, 49152, "swish_gate"), (24, 54, 32, 49152, "affine2"),
])
def test_pw_wgrad_v2_at_the_bcd_benchmark_shapes(K, N, B, rows, mode):
    _need_gpu()
    _check(run_wgrad_v2(K, N, B, rows, mode))


@pytest.mark.parametrize("K,N,B,rows,mode,ragged", [
    (216, 96, 37, 200, "swish_gate", 3),      # samples end inside tiles, ragged end
    (24, 24, 9, 4096, "plain", 0), (216, 96, 3, 70, "swish_gate", 0),      # M small: most workgroups get no tile
])
def test_pw_wgrad_v2_edges(K, N, B, rows, mode, ragged):
    _need_gpu()
    _check(run_wgrad_v2(K, N, B, rows, mode, ragged))


def _zero_some_rows(d):
    d["x"][1000:1032] = 0            # 32 rows of 24 576: one k-step's worth of one operand


def test_pw_wgrad_v2_bound_sees_missing_rows():
    _need_gpu()
    bd = run_wgrad_v2(108, 48, 8, 3072, "swish_nogate", tamper=_zero_some_rows)
    print(f"\nHOTPATH-NEG _zero_some_rows: {bd.kernel} error/bound {bd.worst():.2f}")
    with pytest.raises(AssertionError, match="bound exceeded"):
        bd.check(record=False)


def test_zz_report_worst_ratio_per_kernel():
    """Printed last: the worst error / bound seen per kernel by the cases above (informational; each case asserted its own)."""
    _need_gpu()
    for k in sorted(WORST):
        print(f"\nHOTPATH-WORST {k}: {WORST[k]:.3f}")
