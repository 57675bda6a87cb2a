"""The BatchNorm / SqueezeExcitation finalize and coefficient kernels (csrc/bn_se.hip) against float64, directly, and the gate
folded into c3d_pw_gemm (csrc/bn_fin.h se_gate_consume) against the separate launch, bit for bit.

Every case calls one kernel through the C ABI (ctypes: training = 2, NULL hid / mr / gate and the refusals cannot be said through
ops.py) and compares EVERY element the kernel writes with the restatement in tests/hotpath_reference.py (se_case / se_bn_bwd /
se_gate / bn_from_sums, pinned against torch.autograd by tests/test_hotpath_reference_cpu.py).  Outputs are pre-filled with NaN,
accumulators (dgamma, dbeta, dw1, db1, dw2, db2) with non-zero values (the kernels add), the padding channels of the INPUTS
with NaN (no kernel may read them); padding channels of ss, mr, coef, gate and coefB must come back as exact zeros;
num_batches_tracked goes up by exactly 1 when training == 1 and stays put otherwise (this file's first run of training = 2
with a non-NULL counter found it incremented in that folded-eval mode; the stage driver passes NULL there).  R = 16 rows per sample throughout: none
of these kernels reads the rows.  One float64 case per (B, C, Cr) is built once and shared, unchanged, by all tests.

Kernels, cases (C, Cr, B) and the branch each reaches
  bn_se_finalize_kernel, SE on, training 1 / 0 / 2 (8 channel slices, 4 lanes per channel, 4 samples per thread)
    (8,8,2)       one channel per slice; C < 32: the stride-8 tail loop only; B < 4: clamped sample tails
    (24,8,2)      C < 32, C & 31 == 24 (Cw = C + 16)
    (40,8,6)      C & 31 == 8 (Cw == C); one pass of the unrolled-by-32 loop, then one tail step; B % 4 == 2
    (54,8,1)      B = 1: three of a thread's four samples clamped; Cp (56) != C
    (54,8,3)      B % 4 == 3; also run with hid = NULL (optional output)
    (54,8,32)     B a multiple of 4, eight sample groups
    (108,8,5)     B % 4 == 1; Cp (112) != C
    (216,16,4)    Cr 16
    (216,16,33)   B > 32, B % 4 == 1
    (432,32,16)   the last accepted LDS size (159 744 of 163 840 bytes)
  bn_se_finalize_kernel, SE off: (54, B 7), (216, B 33) -- the single-workgroup path, NULL gate and hid
  se_bn_bwd_coef_kernel, SE on: the list above and
    (64,8,5)      8 Cr == C: the FC2-backward partial sums live inside the dz region (so do (108,8,.), (216,16,.), (432,32,.));
                  (8,8,.), (24,8,.), (40,8,.), (54,8,.) have 8 Cr > C: their own region behind hids
    (54,8,29)     prefetch path (B <= 32), the last prefetch slot used by lane q = 0 only; (54,8,32): every slot used
    (216,16,33), (216,16,48)  B > 32: the loop path; 144 384 bytes of LDS accepted
  se_bn_bwd_coef_kernel, SE off: (54, B 7), (216, B 33) -- coefB the same for every sample
  bn_finalize_kernel / bn_bwd_coef_kernel (16 lanes per channel, one stripe each): C in 24 / 54 / 432 (Cp * 16 = 384, 896: no
    multiple of the 256-thread workgroup; 6912: one), stripes in 1 / 16 (STAT_STRIPES) / 37 (a lane with 0, 1, 2 or 3 stripes);
    count = 1 (unbiased-variance guard), one constant channel (variance clamped at 0, the same clamp in bn_from_sums),
    training 0 (running statistics untouched, num_batches_tracked too), mr = NULL
Refusals (return code checked, every output still holds its pre-fill): c3d_se_bn_bwd_coef at (216,16,64) and (432,32,24)
(187 904 and 185 856 bytes of LDS), c3d_bn_se_finalize at (432,32,24) (182 784), Cp < C, B = 0, SE weights with a NULL gate,
training with stripes = 0.

Bound, per element, derived (u = 2^-24; chains count first-order roundings, 1.001 u covers the second order):
    |dev - ref| <= eps * sum|term| + propagated error of the inputs of that sum
  f64 parts    mean, rstd, scale, shift, the running statistics, A, C, B[n], s1 (d beta), s2 (d gamma) are computed in f64 from
               the f64 sums and rounded to f32 up to five times on the way (shift = beta - f32(mean) * f32(gamma * f32(rstd));
               d gamma: f32(s2), then the f32 add onto the pre-fill, whose magnitude joins the sum): 8 u of the magnitude sum,
               the figure tests/test_hotpath_bf16_gpu.py states for them
  z            fma(scale, f32(sum / R), shift): 2 u (|scale m| + |shift|), plus the 8 u of scale and shift when the kernel made them
  hid          8 partial chains of ceil(C / 8) fma, the three-level tree, the bias: (ceil(C / 8) + 4) u of |W1| z_mag + |b1|,
               plus |W1| err(z)
  gate         a = b2 + a Cr-step fma chain: Cr u (|b2| + |W2| hid_mag) + |W2| err(hid); sigmoid' <= 1/4; expf (1 ulp = 2 u), 1 + e,
               the division: 4 u of the gate itself.  |dev - ref| <= err(a) / 4 + 4 u
  du           f32(nc3_0) * gate * (1 - gate): 4 u |du|
  dh           as hid without the bias: (ceil(C / 8) + 3) u |W2| |du| + |W2| err(du), where the SUPPLIED hid is positive
  dz           Cr-step chain: Cr u |W1| |dh| + |W1| err(dh)
  dw1 / dw2    B-step fma chains of dh z / du hid, one f32 atomic add onto the pre-fill: (B + 1) u mag + u |pre-fill| + the inputs' errors
  db1 / db2    B-term f32 sums and the atomic: B u mag + u |pre-fill| + the inputs' errors
  coefB, s1, s2, C   the f64 part above plus A / R err(dz), sum_n err(dz), sum_n err(dz) |bhat-sum / R|, carried through
The worst error / bound per kernel and output is printed (BNSE-WORST lines; run with -s).  Measured on an MI355X:
  bn_se_finalize   scale 0.22, shift 0.30, mean 0.12, rstd 0.12, running_mean 0.09, running_var 0.13, hid 0.08, gate 0.02
  se_bn_bwd_coef   coefA 0.12, coefB 0.07, coefC 0.09, dgamma 0.17, dbeta 0.14, dw1 0.37, db1 0.16, dw2 0.81, db2 0.78
  bn_finalize      scale 0.22, shift 0.38, mean 0.12, rstd 0.12, running_mean 0.11, running_var 0.13
  bn_bwd_coef      coefA 0.12, coefB 0.11, coefC 0.12, dgamma 0.12, dbeta 0.12
(hid and gate sit low because their bound carries the 8 u of the kernel's own scale / shift through |W1|; dw2 / db2 are short f32
sums whose few roundings can all point the same way.)  The negative controls, same run: forward gate 273 x the bound; backward
dropped sample 8e4 .. 2e6 x on every output but coefA, flipped mask 2e4 .. 4e6 x (db2, which does not see hid, 0.4); missing
stripe 4e4 .. 1.5e6 x (coefA, which does not see the sums, 0.1).

Negative controls (one per kernel; an ordinary valid launch whose device input differs from the reference's in one place; the
same comparison must raise): forward -- one w2 entry scaled by 1 + 2^-5; backward -- nc3[B - 1, c, 0] of one channel zeroed
(the last sample of a B % 4 != 0 case), and one hid entry's sign flipped; striped kernels -- the last stripe zeroed.

Bit-identity of the folded gate: c3d_pw_gemm with fin.batch = B and the se_* fields against a separate c3d_bn_se_finalize on the
same sums -- gate, hid, ss, mr, running_mean, running_var torch.equal, on both C3D_OPT_PW_CFWD legs.  c3d_pw_gemm answers a call
whose workgroups would span more than PW_SE_NS = 4 samples with that same separate launch in front of the GEMM; the last kernel
is a GEMM kernel either way, so the case asserts that the call made ONE launch (c3d_launch_count).  Rows per sample at B = 5 are
the smallest multiple of 16 the in-kernel gate takes (a workgroup of pw_gemm_kernel walks 512 rows at K = 54 and 128 at K = 216
there, and 3 rps + 2 must exceed that: 176 and 48; at 160 and 32 the call makes two launches, measured): a workgroup spans
PW_SE_NS samples, with sample boundaries inside its rows.  M < 1024 is not taken by the cooperative kernel, so two more shapes
(M = 1408 and 1280, rows per sample no multiple of its 256- / 128-row workgroups) put pw_cfwd_kernel on the second leg."""
import ctypes as C
import functools
import math

import pytest
import torch

import hotpath_reference as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
U = 1.001 * 2.0 ** -24
ROWS = 16
EPS, MOM = 1e-5, 0.1
NAN = float("nan")
E_BADARG, E_UNSUPPORTED = -1, -2
WORST = {}

SE_SHAPES = [(8, 8, 2), (24, 8, 2), (40, 8, 6), (54, 8, 1), (54, 8, 3), (54, 8, 32), (108, 8, 5), (216, 16, 4), (216, 16, 33), (432, 32, 16)]
BWD_SHAPES = SE_SHAPES + [(64, 8, 5), (54, 8, 29), (216, 16, 48)]
NOSE_SHAPES = [(54, 7), (216, 33)]


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")


class Bound:
    """Collects error / bound of one case; `check()` raises at the end so that every output is reported."""

    def __init__(self, kernel, shape):
        self.kernel, self.shape, self.rows = kernel, shape, {}

    def add(self, what, dev, ref, lim):
        dev = dev.detach().cpu().double()
        assert dev.shape == ref.shape, (what, dev.shape, ref.shape)
        err = (dev - ref).abs()
        ratio = torch.where(err > 0, err / lim, torch.zeros_like(err))      # (an error where the bound is 0 is inf)
        ratio = torch.where(torch.isfinite(dev), ratio, torch.full_like(ratio, float("inf")))
        self.rows[what] = max(self.rows.get(what, 0.0), float(ratio.max()) if ratio.numel() else 0.0)

    def exact_zero(self, what, t):
        if t.numel():
            assert bool((t == 0).all()), f"{self.kernel} {self.shape}: {what} must be exact zeros"

    def worst(self):
        return max(self.rows.values())

    def check(self, record=True):
        line = ", ".join(f"{k} {v:.3f}" for k, v in self.rows.items())
        if record:
            print(f"\nBNSE {self.kernel} | {self.shape} | error/bound: {line}")
            for k, v in self.rows.items():
                WORST[(self.kernel, k)] = max(WORST.get((self.kernel, k), 0.0), v)
        assert self.worst() <= 1.0, f"bound exceeded: {self.kernel} {self.shape}: {line}"


def _cpad(c):
    return (c + 7) // 8 * 8


def _f32(t):
    """float64 -> the f32 value the device gets, as float64."""
    return t.float().double()


def _dev(t, dtype=torch.float32):
    return None if t is None else t.to(dtype).to(DEV).contiguous()


def _padc(t, Cp, dim, fill=NAN):
    """Pad dimension `dim` (the channels) to Cp with `fill`."""
    shape = list(t.shape)
    shape[dim] = Cp - shape[dim]
    return torch.cat([t, torch.full(shape, fill, dtype=t.dtype)], dim)


def _vec2(a, b, Cp, fill=NAN):
    """(a | b) [2][Cp] as the kernels lay out ss and mr."""
    return torch.cat([_padc(a, Cp, 0, fill), _padc(b, Cp, 0, fill)])


def _nan(*shape):
    return torch.full(shape, NAN, dtype=torch.float32, device=DEV)


def _rand(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g, dtype=torch.float32) * scale).double()          # (f32 values, as the device gets them)


def _p(t):
    return None if t is None else t.data_ptr()


def _lib():
    from change3d_amd import _lib as L
    return L.lib()


def _stream():
    from change3d_amd import ops
    return ops._stream()


def _same_bits(a, b):
    """torch.equal with NaN == NaN (pre-fills are NaN)."""
    if not a.is_floating_point():
        return torch.equal(a, b)
    return torch.equal(torch.nan_to_num(a, nan=12345.0), torch.nan_to_num(b, nan=12345.0))


@functools.lru_cache(maxsize=None)
def case(B, C, Cr, se=True):
    """One float64 block middle per shape (tests/hotpath_reference.py se_case), shared and never modified, with the f32 values of
    what the device is handed (mean / rstd / scale / shift / gate / hid are outputs of the forward kernels: f32 in memory)."""
    k = R.se_case(B, ROWS, C, Cr, seed=7000 + 97 * B + C, se=se)
    for name in ("mean", "rstd", "scale", "shift") + (("gate", "hid") if se else ()):
        k[name + "32"] = _f32(k[name])
    k["rm0"], k["rv0"] = _rand((C,), 7100 + C, 0.3), _f32(_rand((C,), 7101 + C).abs() + 0.5)
    return k


# ================================================================================================ c3d_bn_se_finalize
def run_finalize(C_, Cr, B, training, se=True, hid_null=False, tamper=None):
    k = case(B, C_, Cr, se)
    Cp = _cpad(C_)
    shape = f"C {C_} Cr {Cr if se else 0} B {B} training {training}" + (" hid NULL" if hid_null else "")
    nc = _dev(_padc(k["ncf"], Cp, 1), torch.float64)
    gamma, beta = _dev(k["gamma"]), _dev(k["beta"])
    rm, rv = _dev(k["rm0"]), _dev(k["rv0"])
    nbt = torch.full((1,), 7, dtype=torch.int64, device=DEV)
    w1 = b1 = w2 = b2 = gate = hid = None
    if se:
        w1, b1, w2, b2 = (_dev(t) for t in k["se"])
        if tamper is not None:
            tamper(k, dict(w2=w2))
        gate = _nan(B, Cp)
        hid = None if hid_null else _nan(B, Cr)
    if training == 2:     # folded eval: scale / shift are given (live channels), the kernel zeroes their padding
        ss, mr = _dev(_vec2(k["scale32"], k["shift32"], Cp)), None
    else:
        ss, mr = _nan(2 * Cp), _nan(2 * Cp)
    rc = _lib().c3d_bn_se_finalize(_p(nc), B, float(ROWS), _p(gamma), _p(beta), _p(rm), _p(rv), _p(nbt), MOM, EPS, C_, Cp, training,
                                   _p(w1), _p(b1), _p(w2), _p(b2), Cr if se else 0, _p(ss), _p(mr), _p(gate), _p(hid), _stream())
    torch.cuda.synchronize()
    assert rc == 0, rc
    bd = Bound("bn_se_finalize", shape)
    t = 8 * U
    zero = torch.zeros(C_, dtype=torch.float64)
    if training == 1:
        tot = k["ncf"].sum(0)
        bn = R.bn_from_sums(tot[:, 0], tot[:, 1], float(B * ROWS), k["gamma"], k["beta"], EPS, k["rm0"], k["rv0"], MOM)
        scale, shift, mean, rstd = bn["scale"], bn["shift"], bn["mean"], bn["rstd"]
        bd.add("running_mean", rm, bn["running_mean"], t * (k["rm0"].abs() + mean.abs()))
        bd.add("running_var", rv, bn["running_var"], t * bn["running_var"].abs())
        assert int(nbt) == 8, int(nbt)
    else:
        assert torch.equal(rm.cpu().double(), k["rm0"]) and torch.equal(rv.cpu().double(), k["rv0"]), "running statistics touched in eval"
        assert int(nbt) == 7, int(nbt)
        if training == 0:
            mean, rstd = k["rm0"], 1.0 / torch.sqrt(k["rv0"] + EPS)
            scale = k["gamma"] * rstd
            shift = k["beta"] - mean * scale
    if training == 2:
        scale, shift = k["scale32"], k["shift32"]
        assert torch.equal(ss[:C_].cpu().double(), scale) and torch.equal(ss[Cp:Cp + C_].cpu().double(), shift), "given scale / shift changed"
        sc_err = sh_err = zero
    else:
        sh_mag = (mean * scale).abs() + (shift + mean * scale).abs()
        sc_err, sh_err = t * scale.abs(), t * sh_mag
        bd.add("scale", ss[:C_], scale, sc_err)
        bd.add("shift", ss[Cp:Cp + C_], shift, sh_err)
        bd.add("mean", mr[:C_], mean, t * mean.abs())
        bd.add("rstd", mr[Cp:Cp + C_], rstd, t * rstd.abs())
        bd.exact_zero("padding of mean / rstd", torch.cat([mr[C_:Cp], mr[Cp + C_:]]))
    bd.exact_zero("padding of scale / shift", torch.cat([ss[C_:Cp], ss[Cp + C_:]]))
    if se:
        rw1, rb1, rw2, rb2 = k["se"]
        m = k["ncf"][:, :, 0] / ROWS
        g_ref, h_ref, mag = R.se_gate(k["ncf"][:, :, 0], float(ROWS), scale, shift, rw1, rb1, rw2, rb2)
        z_err = 2 * U * ((scale * m).abs() + shift.abs()) + sc_err * m.abs() + sh_err
        h_err = ((C_ + 7) // 8 + 4) * U * mag["hid_mag"] + z_err @ rw1.abs().t()
        a_err = Cr * U * mag["gate_mag"] + h_err @ rw2.abs().t()
        if hid is not None:
            bd.add("hid", hid, h_ref, h_err)
        bd.add("gate", gate[:, :C_], g_ref, 0.25 * a_err + 4 * U)
        bd.exact_zero("padding channels of the gate", gate[:, C_:])
    return bd


@pytest.mark.parametrize("training", [1, 0, 2])
@pytest.mark.parametrize("C_,Cr,B", SE_SHAPES)
def test_bn_se_finalize_with_se(C_, Cr, B, training):
    _need_gpu()
    run_finalize(C_, Cr, B, training).check()


@pytest.mark.parametrize("training", [1, 0])
@pytest.mark.parametrize("C_,B", NOSE_SHAPES)
def test_bn_se_finalize_without_se(C_, B, training):
    _need_gpu()
    run_finalize(C_, 8, B, training, se=False).check()


def test_bn_se_finalize_hid_is_optional():
    _need_gpu()
    run_finalize(54, 8, 3, 1, hid_null=True).check()


def _scale_one_w2(k, d):
    """The w2 entry that moves a gate most: w2[c][r] *= 1 + 2^-5 on the device only."""
    _, _, w2, _ = k["se"]
    idx = int((w2.abs() * k["hid"].max(0).values[None, :]).argmax())
    d["w2"].view(-1)[idx] *= 1 + 2.0 ** -5


def test_bn_se_finalize_bound_sees_one_changed_gate_weight():
    _need_gpu()
    bd = run_finalize(54, 8, 3, 1, tamper=_scale_one_w2)
    print(f"\nBNSE-NEG forward, one w2 entry * (1 + 2^-5): gate error/bound {bd.rows['gate']:.1f}")
    assert max(v for n, v in bd.rows.items() if n != "gate") <= 1.0      # only the gate moves
    with pytest.raises(AssertionError, match="bound exceeded"):
        bd.check(record=False)


# ================================================================================================ c3d_se_bn_bwd_coef
def _acc(shape, seed):
    """A non-zero pre-fill of an accumulator (the kernels add)."""
    return _f32(_rand(shape, seed, 0.5) + 0.25)


def run_bwd_coef(C_, Cr, B, se=True, tamper=None):
    k = case(B, C_, Cr, se)
    Cp = _cpad(C_)
    shape = f"C {C_} Cr {Cr if se else 0} B {B}"
    nc3, ncf = _dev(_padc(k["nc3"], Cp, 1), torch.float64), _dev(_padc(k["ncf"], Cp, 1), torch.float64)
    gamma = _dev(k["gamma"])
    mr, ss = _dev(_vec2(k["mean32"], k["rstd32"], Cp)), _dev(_vec2(k["scale32"], k["shift32"], Cp))
    w1 = w2 = gate = hid = None
    pre = dict(dgamma=_acc((C_,), 1), dbeta=_acc((C_,), 2))
    if se:
        w1, w2 = _dev(k["se"][0]), _dev(k["se"][2])
        gate, hid = _dev(_padc(k["gate32"], Cp, 1)), _dev(k["hid32"])
        pre.update(dw1=_acc((Cr, C_), 3), db1=_acc((Cr,), 4), dw2=_acc((C_, Cr), 5), db2=_acc((C_,), 6))
    if tamper is not None:
        tamper(k, dict(nc3=nc3, hid=hid))
    acc = {n: _dev(v) for n, v in pre.items()}
    cA, cC, cB = _nan(Cp), _nan(Cp), _nan(B, Cp)
    g = lambda n: _p(acc.get(n))   # noqa: E731
    rc = _lib().c3d_se_bn_bwd_coef(_p(nc3), _p(ncf), B, float(ROWS), _p(gamma), _p(mr), _p(ss), C_, Cp, _p(w1), _p(w2), _p(gate), _p(hid),
                                   Cr if se else 0, _p(cA), _p(cC), _p(cB), g("dgamma"), g("dbeta"), g("dw1"), g("db1"), g("dw2"), g("db2"),
                                   _stream())
    torch.cuda.synchronize()
    assert rc == 0, rc
    r = R.se_bn_bwd(k["nc3"], k["ncf"], float(ROWS), k["gamma"], k["mean32"], k["rstd32"], k["scale32"], k["shift32"], k["se"],
                    k["gate32"] if se else None, k["hid32"] if se else None)
    bd = Bound("se_bn_bwd_coef", shape)
    for name, dev in (("coefA", cA[:C_]), ("coefB", cB[:, :C_]), ("coefC", cC[:C_])):
        val, mag, err = r[name]
        bd.add(name, dev, val, 8 * U * mag + err)
    chain = dict(dgamma=8, dbeta=8, dw1=B + 1, dw2=B + 1, db1=B, db2=B)            # roundings of the last sum (docstring)
    last = dict(dgamma=8, dbeta=8, dw1=1, dw2=1, db1=1, db2=1)                      # ... and of the add onto the pre-fill
    for name in pre:
        val, mag, err = r[name]
        p32 = _f32(pre[name])
        bd.add(name, acc[name], p32 + val, chain[name] * U * mag + last[name] * U * p32.abs() + err)
    bd.exact_zero("padding of coefA / coefC", torch.cat([cA[C_:], cC[C_:]]))
    bd.exact_zero("padding channels of coefB", cB[:, C_:])
    if not se:
        assert torch.equal(cB, cB[:1].expand(B, Cp)), "coefB differs between samples without SE"
    return bd


@pytest.mark.parametrize("C_,Cr,B", BWD_SHAPES)
def test_se_bn_bwd_coef_with_se(C_, Cr, B):
    _need_gpu()
    run_bwd_coef(C_, Cr, B).check()


@pytest.mark.parametrize("C_,B", NOSE_SHAPES)
def test_se_bn_bwd_coef_without_se(C_, B):
    _need_gpu()
    run_bwd_coef(C_, 8, B, se=False).check()


def _zero_last_samples_gate_gradient(k, d):
    c = int(k["nc3"][-1, :, 0].abs().argmax())
    d["nc3"][-1, c, 0] = 0.0


def _flip_one_hid(k, d):
    """The largest hidden activation turns negative on the device only: its ReLU mask closes there."""
    idx = int(k["hid32"].argmax())
    d["hid"].view(-1)[idx] *= -1.0


@pytest.mark.parametrize("tamper", [_zero_last_samples_gate_gradient, _flip_one_hid])
def test_se_bn_bwd_coef_bound_sees_a_dropped_sample_and_a_flipped_mask(tamper):
    _need_gpu()
    bd = run_bwd_coef(54, 8, 3, tamper=tamper)           # B % 4 == 3: the tampered sample is the last of a clamped tail
    print(f"\nBNSE-NEG backward, {tamper.__name__}: error/bound " + ", ".join(f"{n} {v:.1f}" for n, v in bd.rows.items()))
    assert bd.rows["coefA"] <= 1.0                       # A does not depend on the SE chain
    with pytest.raises(AssertionError, match="bound exceeded"):
        bd.check(record=False)


# ================================================================================================ the striped kernels
def _stripe_data(C_, stripes, count, seed, constant=None):
    """x [count][C] split over the stripes (row i -> stripe i % stripes): sums [stripes][2][C] = (sum, sum of squares)."""
    x = _rand((count, C_), seed, 1.5) + _rand((C_,), seed + 1, 0.7)
    if constant is not None:
        x[:, constant] = 0.7
    sums = torch.zeros(stripes, 2, C_, dtype=torch.float64)
    for s in range(min(stripes, count)):
        sums[s, 0], sums[s, 1] = x[s::stripes].sum(0), (x[s::stripes] ** 2).sum(0)
    return sums


def run_bn_finalize(C_, stripes, count=200, training=1, mr_null=False, constant=None, tamper=False):
    Cp = _cpad(C_)
    shape = f"C {C_} stripes {stripes} count {count} training {training}" + (" mr NULL" if mr_null else "") + \
            (" constant channel" if constant is not None else "")
    sums = _stripe_data(C_, stripes, count, 8000 + C_ + stripes, constant)
    gamma0, beta0 = _f32(_rand((C_,), 8001).abs() + 0.5), _rand((C_,), 8002, 0.3)
    rm0, rv0 = _rand((C_,), 8003, 0.3), _f32(_rand((C_,), 8004).abs() + 0.5)
    sd = _dev(sums, torch.float64)
    if tamper:
        sd[-1] = 0.0
    gamma, beta, rm, rv = _dev(gamma0), _dev(beta0), _dev(rm0), _dev(rv0)
    nbt = torch.full((1,), 7, dtype=torch.int64, device=DEV)
    ss, mr = _nan(2 * Cp), None if mr_null else _nan(2 * Cp)
    rc = _lib().c3d_bn_finalize(_p(sd), stripes, float(count), _p(gamma), _p(beta), _p(rm), _p(rv), _p(nbt), MOM, EPS, C_, Cp, training,
                                _p(ss), _p(mr), _stream())
    torch.cuda.synchronize()
    assert rc == 0, rc
    bd = Bound("bn_finalize", shape)
    t = 8 * U
    if training:
        tot = sums.sum(0)
        bn = R.bn_from_sums(tot[0], tot[1], float(count), gamma0, beta0, EPS, rm0, rv0, MOM)
        scale, shift, mean, rstd = bn["scale"], bn["shift"], bn["mean"], bn["rstd"]
        if constant is not None:      # s2 / count - mean^2 is rounding noise there: the clamp holds it at >= 0 on both sides
            assert abs(float(rstd[constant]) - EPS ** -0.5) < 1e-6 * EPS ** -0.5
        bd.add("running_mean", rm, bn["running_mean"], t * (rm0.abs() + mean.abs()))
        bd.add("running_var", rv, bn["running_var"], t * bn["running_var"].abs())
        assert int(nbt) == 8, int(nbt)
    else:
        mean, rstd = rm0, 1.0 / torch.sqrt(rv0 + EPS)
        scale = gamma0 * rstd
        shift = beta0 - mean * scale
        assert torch.equal(rm.cpu().double(), rm0) and torch.equal(rv.cpu().double(), rv0), "running statistics touched in eval"
        assert int(nbt) == 7, int(nbt)
    bd.add("scale", ss[:C_], scale, t * scale.abs())
    bd.add("shift", ss[Cp:Cp + C_], shift, t * ((mean * scale).abs() + (shift + mean * scale).abs()))
    bd.exact_zero("padding of scale / shift", torch.cat([ss[C_:Cp], ss[Cp + C_:]]))
    if mr is not None:
        bd.add("mean", mr[:C_], mean, t * mean.abs())
        bd.add("rstd", mr[Cp:Cp + C_], rstd, t * rstd.abs())
        bd.exact_zero("padding of mean / rstd", torch.cat([mr[C_:Cp], mr[Cp + C_:]]))
    return bd


def run_bn_bwd_coef(C_, stripes, count=200, tamper=False):
    Cp = _cpad(C_)
    dsums = _rand((stripes, 2, C_), 8100 + C_ + stripes, 20.0)
    gamma0 = _f32(_rand((C_,), 8101).abs() + 0.5)
    mean0, rstd0 = _rand((C_,), 8102, 0.5), _f32(_rand((C_,), 8103).abs() + 0.5)
    pre = dict(dgamma=_acc((C_,), 11), dbeta=_acc((C_,), 12))
    sd = _dev(dsums, torch.float64)
    if tamper:
        sd[-1] = 0.0
    gamma, mr = _dev(gamma0), _dev(_vec2(mean0, rstd0, Cp))
    acc = {n: _dev(v) for n, v in pre.items()}
    coef = _nan(3 * Cp)
    rc = _lib().c3d_bn_bwd_coef(_p(sd), stripes, float(count), _p(gamma), _p(mr), C_, Cp, _p(coef), _p(acc["dgamma"]), _p(acc["dbeta"]), _stream())
    torch.cuda.synchronize()
    assert rc == 0, rc
    # the stripes in the place of the samples of the no-SE restatement: nc3[k] = (-, sum g, sum g xhat), count = stripes * R
    nc3 = torch.stack([torch.zeros(stripes, C_, dtype=torch.float64), dsums[:, 0], dsums[:, 1]], 2)
    r = R.se_bn_bwd(nc3, torch.zeros(stripes, C_, 2, dtype=torch.float64), float(count) / stripes, gamma0, mean0, rstd0,
                    torch.zeros(C_, dtype=torch.float64), torch.zeros(C_, dtype=torch.float64))
    bd = Bound("bn_bwd_coef", f"C {C_} stripes {stripes} count {count}")
    for i, name in enumerate(("coefA", "coefB", "coefC")):
        val, mag, _ = r[name]
        if name == "coefB":
            val, mag = val[0], mag[0]
        bd.add(name, coef[i * Cp:i * Cp + C_], val, 8 * U * mag)
        bd.exact_zero(f"padding of {name}", coef[i * Cp + C_:(i + 1) * Cp])
    for name in pre:
        val, mag, _ = r[name]
        p32 = _f32(pre[name])
        bd.add(name, acc[name], p32 + val, 8 * U * (mag + p32.abs()))
    return bd


@pytest.mark.parametrize("stripes", [1, 16, 37])
@pytest.mark.parametrize("C_", [24, 54, 432])
def test_striped_bn_finalize_and_bwd_coef(C_, stripes):
    _need_gpu()
    from change3d_amd import ops
    assert ops.STAT_STRIPES == 16
    bf, bb = run_bn_finalize(C_, stripes), run_bn_bwd_coef(C_, stripes)
    bf.check(), bb.check()


@pytest.mark.parametrize("kw", [dict(count=1, stripes=1), dict(count=1, stripes=16), dict(constant=3), dict(training=0), dict(mr_null=True),
                                dict(training=0, mr_null=True)], ids=lambda kw: "-".join(f"{a}{b}" for a, b in kw.items()))
def test_striped_bn_finalize_edges(kw):
    _need_gpu()
    kw = dict(kw)
    run_bn_finalize(54, kw.pop("stripes", 16), **kw).check()


def test_striped_kernels_bound_sees_a_missing_stripe():
    _need_gpu()
    for run in (run_bn_finalize, run_bn_bwd_coef):
        bd = run(54, 37, tamper=True)
        print(f"\nBNSE-NEG {bd.kernel}, last stripe zeroed: error/bound " + ", ".join(f"{n} {v:.1f}" for n, v in bd.rows.items()))
        with pytest.raises(AssertionError, match="bound exceeded"):
            bd.check(record=False)


# ================================================================================================ refusals
def _finalize_args(C_, Cr, B, Cp=None):
    Cp = _cpad(C_) if Cp is None else Cp
    Cq = max(Cp, C_)
    d = dict(nc=torch.zeros(max(B, 1), Cq, 2, dtype=torch.float64, device=DEV), gamma=torch.ones(C_, device=DEV), beta=torch.zeros(C_, device=DEV),
             rm=torch.zeros(C_, device=DEV), rv=torch.ones(C_, device=DEV), nbt=torch.full((1,), 7, dtype=torch.int64, device=DEV),
             w1=torch.zeros(Cr, C_, device=DEV), b1=torch.zeros(Cr, device=DEV), w2=torch.zeros(C_, Cr, device=DEV), b2=torch.zeros(C_, device=DEV),
             ss=_nan(2 * Cq), mr=_nan(2 * Cq), gate=_nan(max(B, 1), Cq), hid=_nan(max(B, 1), Cr))
    return d, Cp


@pytest.mark.parametrize("what,C_,Cr,B,rc_want", [("LDS", 432, 32, 24, E_UNSUPPORTED), ("Cp < C", 54, 8, 3, E_BADARG), ("B = 0", 54, 8, 0, E_BADARG),
                                                  ("NULL gate", 54, 8, 3, E_BADARG)])
def test_bn_se_finalize_refuses(what, C_, Cr, B, rc_want):
    _need_gpu()
    d, Cp = _finalize_args(C_, Cr, B, Cp=C_ - 6 if what == "Cp < C" else None)
    outs = {n: d[n] for n in ("ss", "mr", "gate", "hid", "rm", "rv", "nbt")}
    fills = {n: t.clone() for n, t in outs.items()}
    gate = None if what == "NULL gate" else d["gate"]
    rc = _lib().c3d_bn_se_finalize(_p(d["nc"]), B, float(ROWS), _p(d["gamma"]), _p(d["beta"]), _p(d["rm"]), _p(d["rv"]), _p(d["nbt"]), MOM, EPS,
                                   C_, Cp, 1, _p(d["w1"]), _p(d["b1"]), _p(d["w2"]), _p(d["b2"]), Cr, _p(d["ss"]), _p(d["mr"]), _p(gate),
                                   _p(d["hid"]), _stream())
    torch.cuda.synchronize()
    assert rc == rc_want, rc
    for n in outs:
        assert _same_bits(outs[n], fills[n]), f"{n} written by a refused call"


@pytest.mark.parametrize("what,C_,Cr,B,rc_want", [("LDS", 216, 16, 64, E_UNSUPPORTED), ("LDS", 432, 32, 24, E_UNSUPPORTED), ("Cp < C", 54, 8, 3, E_BADARG),
                                                  ("B = 0", 54, 8, 0, E_BADARG), ("NULL gate", 54, 8, 3, E_BADARG)])
def test_se_bn_bwd_coef_refuses(what, C_, Cr, B, rc_want):
    _need_gpu()
    d, Cp = _finalize_args(C_, Cr, B, Cp=C_ - 6 if what == "Cp < C" else None)
    Cq, Bq = max(Cp, C_), max(B, 1)
    nc3 = torch.zeros(Bq, Cq, 3, dtype=torch.float64, device=DEV)
    gate, hid = torch.full((Bq, Cq), 0.5, device=DEV), torch.ones(Bq, Cr, device=DEV)
    outs = dict(cA=_nan(Cq), cC=_nan(Cq), cB=_nan(Bq, Cq), dgamma=torch.ones(C_, device=DEV), dbeta=torch.ones(C_, device=DEV),
                dw1=torch.ones(Cr, C_, device=DEV), db1=torch.ones(Cr, device=DEV), dw2=torch.ones(C_, Cr, device=DEV), db2=torch.ones(C_, device=DEV))
    fills = {n: t.clone() for n, t in outs.items()}
    mr = ss = torch.ones(2 * Cq, device=DEV)
    rc = _lib().c3d_se_bn_bwd_coef(_p(nc3), _p(d["nc"]), B, float(ROWS), _p(d["gamma"]), _p(mr), _p(ss), C_, Cp, _p(d["w1"]), _p(d["w2"]),
                                   None if what == "NULL gate" else _p(gate), _p(hid), Cr, _p(outs["cA"]), _p(outs["cC"]), _p(outs["cB"]),
                                   _p(outs["dgamma"]), _p(outs["dbeta"]), _p(outs["dw1"]), _p(outs["db1"]), _p(outs["dw2"]), _p(outs["db2"]),
                                   _stream())
    torch.cuda.synchronize()
    assert rc == rc_want, rc
    for n in outs:
        assert _same_bits(outs[n], fills[n]), f"{n} written by a refused call"


def test_striped_kernels_refuse_training_without_stripes():
    _need_gpu()
    C_, Cp = 54, 56
    sums = torch.zeros(2 * C_, dtype=torch.float64, device=DEV)
    gamma, beta, rm, rv = torch.ones(C_, device=DEV), torch.zeros(C_, device=DEV), torch.zeros(C_, device=DEV), torch.ones(C_, device=DEV)
    nbt = torch.full((1,), 7, dtype=torch.int64, device=DEV)
    ss, mr, coef = _nan(2 * Cp), _nan(2 * Cp), _nan(3 * Cp)
    rc = _lib().c3d_bn_finalize(_p(sums), 0, 200.0, _p(gamma), _p(beta), _p(rm), _p(rv), _p(nbt), MOM, EPS, C_, Cp, 1, _p(ss), _p(mr), _stream())
    rc2 = _lib().c3d_bn_finalize(_p(sums), 1, 200.0, _p(gamma), _p(beta), _p(rm), _p(rv), _p(nbt), MOM, EPS, C_, C_ - 6, 1, _p(ss), _p(mr), _stream())
    dg, db = torch.ones(C_, device=DEV), torch.ones(C_, device=DEV)
    rc3 = _lib().c3d_bn_bwd_coef(_p(sums), 0, 200.0, _p(gamma), _p(rm), C_, Cp, _p(coef), _p(dg), _p(db), _stream())
    torch.cuda.synchronize()
    assert (rc, rc2, rc3) == (E_BADARG, E_BADARG, E_BADARG)
    assert int(nbt) == 7 and bool(torch.isnan(ss).all()) and bool(torch.isnan(mr).all()) and bool(torch.isnan(coef).all())
    assert bool((rm == 0).all()) and bool((rv == 1).all()) and bool((dg == 1).all()) and bool((db == 1).all())


# ================================================================================================ the gate folded into c3d_pw_gemm
# (K, N, Cr, B, rows per sample, the cooperative kernel takes it): the smallest multiple of 16 at which c3d_pw_gemm keeps the gate in
# the GEMM at B = 5 (one step lower it makes the separate launch: a workgroup would span five samples), and one shape per width that
# the cooperative kernel takes too (M >= 1024, rows per sample >= its row tile, sample boundaries inside a workgroup's rows)
FOLDED = [(54, 24, 8, 5, 176, False), (216, 96, 16, 5, 48, False), (54, 24, 8, 8, 176, True), (216, 96, 16, 16, 80, True)]


@pytest.mark.parametrize("K,N,Cr,B,rps,coop", FOLDED)
def test_gate_folded_into_the_gemm_is_bit_identical_to_the_separate_launch(K, N, Cr, B, rps, coop):
    _need_gpu()
    from change3d_amd import ops, _lib as L
    Kp, Np, M = _cpad(K), _cpad(N), B * rps
    x = _padc(_rand((M, K), 9000 + K), Kp, 1, 0.0).to(torch.bfloat16).to(DEV).contiguous()
    w = _dev(_rand((N, K), 9001, 0.1))
    xs = x.view(B, rps, Kp).double()
    nc = torch.stack([xs.sum(1), (xs * xs).sum(1)], dim=2).contiguous()        # [B][Kp][2], as c3d_dw333_fwd leaves them
    gamma, beta = _dev(_rand((K,), 9002).abs() + 0.5), _dev(_rand((K,), 9003, 0.2))
    w1, b1 = _dev(_rand((Cr, K), 9004, 2.0 / K ** 0.5)), _dev(_rand((Cr,), 9005, 0.3))
    w2, b2 = _dev(_rand((K, Cr), 9006, 1.0 / Cr ** 0.5)), _dev(_rand((K,), 9007, 0.3))
    rm0, rv0 = _rand((K,), 9008, 0.3), _rand((K,), 9009).abs() + 0.5
    img = torch.empty(ops.pw_weight_image_bytes(N, K, ops.DT_BF16), dtype=torch.uint8, device=DEV)
    ops.pw_pack_weights([(w, img, N, K, K, 1)], ops.DT_BF16)

    def buffers():
        return dict(ss=_nan(2 * Kp), mr=_nan(2 * Kp), gate=_nan(B, Kp), hid=_nan(B, Cr), rm=_dev(rm0), rv=_dev(rv0),
                    nbt=torch.full((1,), 7, dtype=torch.int64, device=DEV))

    sep = buffers()
    rc = L.lib().c3d_bn_se_finalize(_p(nc), B, float(rps), _p(gamma), _p(beta), _p(sep["rm"]), _p(sep["rv"]), _p(sep["nbt"]), MOM, EPS, K, Kp, 1,
                                    _p(w1), _p(b1), _p(w2), _p(b2), Cr, _p(sep["ss"]), _p(sep["mr"]), _p(sep["gate"]), _p(sep["hid"]), _stream())
    torch.cuda.synchronize()
    assert rc == 0, rc
    assert bool(torch.isfinite(sep["gate"]).all()) and float(sep["hid"].max()) > 0 and int(sep["nbt"]) == 8
    try:
        for opt in (0, 1):
            ops.set_option(ops.OPT_PW_CFWD, opt)
            f = buffers()
            y = torch.full((M, Np), NAN, dtype=torch.bfloat16, device=DEV)
            stats = torch.zeros(ops.STAT_STRIPES * 2 * N, dtype=torch.float64, device=DEV)
            a = L.PwArgs()
            a.x, a.y, a.w, a.w_img = _p(x), _p(y), _p(w), _p(img)
            a.M, a.K, a.Kp, a.N, a.Np, a.w_sn, a.w_sk = M, K, Kp, N, Np, K, 1
            a.rows_per_sample, a.dtype = rps, ops.DT_BF16
            a.pro_mode, a.epi_mode = ops.PRO_BN_SE_SWISH, ops.EPI_STATS
            a.pro_p, a.stats, a.pro_gate = _p(f["ss"]), _p(stats), _p(f["gate"])
            fin = L.BnFin()
            fin.gamma, fin.beta, fin.running_mean, fin.running_var, fin.nbt, fin.ss, fin.mr = (_p(t) for t in (gamma, beta, f["rm"], f["rv"], f["nbt"], f["ss"], f["mr"]))
            fin.count, fin.momentum, fin.eps, fin.training, fin.batch, fin.sums = float(M), MOM, EPS, 1, B, _p(nc)
            a.fin = fin
            a.se_w1, a.se_b1, a.se_w2, a.se_b2, a.se_hid, a.se_cr = _p(w1), _p(b1), _p(w2), _p(b2), _p(f["hid"]), Cr
            n0 = ops.launch_count()
            rc = L.lib().c3d_pw_gemm(C.byref(a), _stream())
            launches, kernel = ops.launch_count() - n0, ops.last_kernel()
            torch.cuda.synchronize()
            assert rc == 0, rc
            want = "pw_cfwd_kernel<1, " if (opt and coop) else "pw_gemm_kernel<"
            assert kernel.startswith(want), (opt, kernel)
            assert launches == 1, f"{launches} launches: the gate came from the separate c3d_bn_se_finalize launch"
            for n in ("gate", "hid", "ss", "mr", "rm", "rv", "nbt"):
                assert _same_bits(f[n], sep[n]), f"CFWD {opt} ({kernel}): {n} differs from the separate launch"
            assert bool(torch.isfinite(y[:, :N].float()).all())
    finally:
        ops.set_option(ops.OPT_PW_CFWD, 3)


def test_zz_report_worst_ratio_per_kernel_and_output():
    _need_gpu()
    for (kernel, what), v in sorted(WORST.items()):
        print(f"\nBNSE-WORST {kernel} {what} {v:.3f}")
    assert all(math.isfinite(v) and v <= 1.0 for v in WORST.values())
