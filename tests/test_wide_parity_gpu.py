"""The wide pointwise GEMM and weight-gradient kernels (csrc/pw_wide.hip) against float64, element by element.

c3d_pw_gemm / c3d_pw_wgrad hand a call to pw_wide_kernel<T, PRO, EPI> / pw_wide_wgrad_kernel<T> when Kp > 224, Np > 224 or a
bias is given: the res5 stage of the change-captioning step (96 / 192 -> 432 -> 192) and every linear layer of the caption
decoder.  Every case calls one kernel through the C ABI, asserts WHICH kernel ran (c3d_last_kernel), pre-fills the outputs
with NaN, requires exact zeros in the padding channels and compares every output element with the float64 restatement in
tests/wide_reference.py (pinned against torch.autograd by tests/test_wide_reference_cpu.py).  Both storage types.

What each gap of the kernels' earlier coverage maps to
  1 dispatch pairs never launched      test_none_add (NONE+ADD, res_mode 1), test_bn_se_swish_store_and_stats (BN_SE_SWISH+STATS),
                                       test_affine2_store_and_add (AFFINE2+STORE), test_stride2_gather (wide_row_offset)
  2 the `fin` forms                    test_affine2_store_and_add (fin.sums, dgamma / dbeta, fin.ss),
                                       test_wgrad (p_fin, through ops.pw_wgrad's new keyword)
  3 SWISH_SE_BWD sample slots          test_affine2_swish_se_bwd (rows_per_sample 17: five slots, 16 / 21: four, a partial last
                                       sample for nmax, the sums bit-identical between two runs)
  4 weight staging                     test_linear_bias: layout "kc" = contiguous K, float4 path (K % 4 == 0 at every shape);
                                       "tr" = transposed (w_sn = 1), float4 path at N = 576 / 192 / 1024, scalar path at
                                       N = 203 / 5; "slice" = contiguous K from a base 4 bytes off a 16-byte boundary, scalar path
  5 K chunks, LDS size                 Kp = 432 in every res5 case (last chunk 48 of 64 for bf16, 16 of 32 for f32),
                                       test_linear_bias (130, 1024, 1024): 80 768 bytes of dynamic LDS
  6 statistics stripes                 test_none_stats: 20 row blocks, checked stripe by stripe
  7 weight-gradient splits             test_wgrad: M = 5 / 31 (below one chunk), 128 (one split), 450 (short last split), 3072;
                                       dW a strided, offset view with a non-zero start; (192, 203) reaches the kernel
                                       through the narrow kernels' refusal, not through the 224 rule
  8 c3d_last_kernel names them         every case

Bound, per element (u = 2^-24), the form of tests/test_hotpath_bf16_gpu.py:
    stored outputs  |dev - ref| <= rel (|ref| + E) + E,  E = eps * sum|term| + slack,  rel = 2^-8 (bf16) or 2^-24 (f32 storage)
    f32 / f64 sums  |dev - ref| <= E
eps counts the f32 roundings of the code path, rounded up to a power of two:
  GEMM tile      the matrix cores add K products into an f32 accumulator: one rounding per product is charged (the adder tree
                 inside one instruction is not documented to be exact); bf16 x bf16 products are exact, f32 x f32 products are
                 charged a second rounding.  + the bias, + the residual: (K + 2) u for bf16, (2 K + 2) u for f32 storage --
                 K = 192: 2^-16 / 2^-15, K = 432: 2^-15 / 2^-14, K = 1024: 2^-13 / 2^-12 (EPS_GEMM below).
  operands       what the prologue's f32 arithmetic brings along is `slack`: one bf16 ulp times |W| where the converted operand lies
                 within its own f32 error of a rounding boundary (bf16), that error itself times |W| (f32); the errors are
                 hotpath_reference's (two fma: 2^-22 of the magnitude; the Swish: + 2^-17 of the value).
  STATS          a thread adds the 4 rows of its row group (3 additions, 1 product for the square), 18 row groups are added in
                 turn, then f64 atomics: 22 u -> 2^-19, of the sums over the kernel's OWN stored rows, stripe by stripe.
  SWISH_SE_BWD   element: derived in wide_reference.epi_swish_se_bwd.  Sums: a thread adds at most 4 rows in f32 (s0: 1 product +
                 3 additions -> 2^-22; s1: 3 additions -> 2^-22; s2: subtraction, 2 products, 3 additions -> 6 u -> 2^-21), then
                 2^-40 fixed point: 2^-41 per flush, at most 18 (rows_per_sample / 64 + 2) flushes per value.  s1 / s2 against
                 float64 sums of the kernel's own stored output, s0 against the reference.
  coefficients   float64 arithmetic rounded to f32 once: 2^-24 of the magnitude -> 2^-23 (the device may contract the float64
                 products into fma).  dgamma / dbeta: one f32 conversion and one f32 addition, reproduced exactly.
  weight grad.   a split adds its rows' products in the matrix cores (as above: 1 or 2 roundings per row), then one f32 atomic
                 per split on top of the start value.  The launcher's plan (wide_reference.wgrad_plan, asserted) gives at
                 most 256 rows per split and 32 splits at these shapes: 288 u -> 2^-15 (bf16), 544 u -> 2^-14 (f32), of
                 sum|term| + |start|.

Worst error / bound per kernel (WIDE-WORST lines of this file, run with -s, MI355X; <PRO, EPI>: PRO 0 none, 1 BN_SE_SWISH,
2 AFFINE2; EPI 0 store, 1 STATS, 2 SWISH_SE_BWD, 3 ADD):
    pw_wide_kernel           <0, 0>   <0, 1>   <0, 3>   <1, 0>   <1, 1>   <2, 0>   <2, 2>   <2, 3>      pw_wide_wgrad_kernel
    bf16 storage              0.974    0.990    0.974    0.958    0.958    0.949    0.985    0.954       0.931
    f32 storage               0.019    0.138    0.008    0.006    0.168    0.005    0.176    0.007       0.006
The bf16 figures are the one rounding of the stored value (2^-8 |ref| is tight just above a power of two), the weight gradient's
an operand that rounded the other way (its ulp times |Q| IS the slack); the f32 bound charges every product, its errors add like
a random walk.  No case exceeded its bound; the (130, 1024, 1024) launch with 80 768 bytes of dynamic LDS is granted as it is.
The negative controls sit at 5.5 (one weight, bf16) to 9 000 times the bound.

Negative controls (one per family): an ordinary valid launch whose device input differs from the reference's in one place --
one weight in the last partial K chunk, one input element in channel K - 1 of the last row, one SE gate entry of the fifth
slot's sample, one bias entry above column 224, one row at the end of a weight-gradient split, the stride-2 gather fed the
dense rows -- and the same comparison must raise."""
import pytest
import torch

import wide_reference as WR
from test_hotpath_bf16_gpu import Bound

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BF, F32 = torch.bfloat16, torch.float32
DTYPES = [BF, F32]
U = 2.0 ** -24
EPS_STATS, EPS_S0, EPS_S1, EPS_S2, EPS_COEF = 2.0 ** -19, 2.0 ** -22, 2.0 ** -22, 2.0 ** -21, 2.0 ** -23
WORST = {}
PRO = {"none": 0, "swish": 1, "affine": 2}
EPI = {"store": 0, "stats": 1, "sebwd": 2, "add": 3}


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")


def _pow2ceil(n):
    p = 1
    while p < n:
        p *= 2
    return p


def EPS_GEMM(K, dtype):
    return _pow2ceil((K if dtype == BF else 2 * K) + 2) * U


def EPS_WGRAD(dtype):
    return _pow2ceil((256 if dtype == BF else 512) + 32) * U


class WideBound(Bound):
    """tests/test_hotpath_bf16_gpu.py's Bound; the report lines of this file are WIDE lines."""

    def check(self, record=True):
        line = ", ".join(f"{k} {v:.3f}" for k, v in self.rows.items())
        if record:
            print(f"\nWIDE {self.kernel} | {self.shape} | error/bound: {line}")
            WORST[self.kernel] = max(WORST.get(self.kernel, 0.0), self.worst())
        assert self.worst() <= 1.0, f"bound exceeded: {self.kernel} {self.shape}: {line}"


def _tn(dtype):
    return "unsigned short" if dtype == BF else "float"


def _rnd(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g, dtype=torch.float32) * scale


def _act(shape, seed, dtype, scale=1.0):
    """Activations: f32 values that are exact in the storage type."""
    return _rnd(shape, seed, scale).to(dtype).float()


def _pad(t, cp):
    return t if t.shape[-1] == cp else torch.nn.functional.pad(t, (0, cp - t.shape[-1]))


def _dev(t, cp=None, dtype=F32):
    return (_pad(t, cp) if cp is not None else t).to(DEV, dtype).contiguous()


def _d(t):
    return t.detach().cpu().double()


def _weight_view(w, layout):
    """The f32 weight [N][K] on the device in one of three layouts -> (tensor handed to the kernel, w_sn, w_sk)."""
    N, K = w.shape
    if layout == "kc":
        return w.to(DEV).contiguous(), K, 1
    if layout == "tr":
        return w.t().contiguous().to(DEV), 1, N
    store = torch.zeros(N * K + 1, dtype=F32, device=DEV)          # "slice": rows of K from a base 4 bytes off 16
    store[1:] = w.to(DEV).reshape(-1)
    v = store[1:]
    assert v.data_ptr() % 16 == 4
    return v, K, 1


def _coef_case(K, count, seed):
    """Completed BatchNorm-backward sums and the saved statistics, and the coefficients rebuilt from them (f32, float64 reference)."""
    sums = torch.stack([_rnd((K,), seed, 3.0), _rnd((K,), seed + 1, 3.0)]).double() * 1.0000001   # (not f32 values)
    gamma, mean, rstd = _rnd((K,), seed + 2).abs() + 0.5, _rnd((K,), seed + 3, 0.5), _rnd((K,), seed + 4).abs() + 0.5
    coef, mag, (dgamma, dbeta) = WR.bn_bwd_coef(sums, gamma.double(), mean.double(), rstd.double(), float(count))
    return dict(sums=sums, gamma=gamma, mean=mean, rstd=rstd, coef=coef, mag=mag, dgamma=dgamma, dbeta=dbeta, count=float(count))


def _fin_bwd(cc, K, Kp, keep):
    """c3d_bn_fin for the consumer-side coefficient rebuild (training = 0).  dgamma / dbeta start non-zero, ss is NaN-filled."""
    from change3d_amd import _lib as L
    t = dict(sums=cc["sums"].to(DEV).contiguous(), gamma=cc["gamma"].to(DEV),
             mr=torch.cat([_pad(cc["mean"], Kp), _pad(cc["rstd"], Kp)]).to(DEV),
             dgamma=_rnd((K,), 901).to(DEV), dbeta=_rnd((K,), 902).to(DEV),
             ss=torch.full((3 * Kp,), float("nan"), dtype=F32, device=DEV))
    t["dgamma0"], t["dbeta0"] = t["dgamma"].clone(), t["dbeta"].clone()
    f = L.BnFin()
    f.sums, f.gamma, f.mr, f.ss = t["sums"].data_ptr(), t["gamma"].data_ptr(), t["mr"].data_ptr(), t["ss"].data_ptr()
    f.running_mean, f.running_var = t["dgamma"].data_ptr(), t["dbeta"].data_ptr()
    f.count, f.training, f.batch = cc["count"], 0, 0
    keep.update(t)
    return f


def _check_fin(bd, cc, t, K, Kp):
    """fin.ss against the float64 coefficients, zeros in its padding; dgamma / dbeta = start + sums, added exactly once."""
    ss = _d(t["ss"]).view(3, Kp)
    bd.add("fin.ss", ss[:, :K], cc["coef"], cc["mag"], EPS_COEF)
    bd.exact_zero("padding of fin.ss", t["ss"].view(3, Kp)[:, K:])
    assert torch.equal(t["dgamma"].cpu(), t["dgamma0"].cpu() + cc["dgamma"].float()), "dgamma = start + (float) s2, once"
    assert torch.equal(t["dbeta"].cpu(), t["dbeta0"].cpu() + cc["dbeta"].float()), "dbeta = start + (float) s1, once"


# ================================================================================================ forward
def run_gemm(dtype, M, K, N, pro="none", epi="store", *, bias=False, layout="kc", gated=True, rps=0, res_mode=0, BT=0, H=0, W=0,
             stride2=False, use_fin=False, pro_p_from=None, alias=False, tamper=None, dense_instead=False, seed=100):
    """One c3d_pw_gemm launch on the wide kernel against the float64 restatement.  With stride2, M counts the OUTPUT rows
    (BT * H/2 * W/2).  tamper(d): changes the device's inputs (a dict of CPU tensors) after the reference has taken its copy.
    Returns the bound and a dict of the launch's device tensors."""
    from change3d_amd import ops
    bf16 = dtype == BF
    Kp, Np = ops.cpad(K), ops.cpad(N)
    B = (M + rps - 1) // rps if rps else 1
    rows_in = BT * H * W if stride2 else M
    d = dict(x=_act((rows_in, K), seed, dtype), w=_rnd((N, K), seed + 1, 0.1))
    if bias:
        d["bias"] = _rnd((N,), seed + 2, 0.5)
    cc = None
    if pro == "swish":
        d["scale"], d["shift"] = _rnd((K,), seed + 3).abs() + 0.5, _rnd((K,), seed + 4, 0.3)
        if gated:
            d["gate"] = torch.sigmoid(_rnd((B, K), seed + 5))
    elif pro == "affine":
        d["x2"] = _act((rows_in, K), seed + 6, dtype)
        cc = _coef_case(K, M, seed + 20)
        d["coef"] = cc["coef"].float() if pro_p_from is None else pro_p_from.cpu().view(3, Kp)[:, :K].clone()
    if epi == "add":
        d["res"] = _act((M, N) if res_mode == 0 else (BT * (H // 2) * (W // 2), N), seed + 7, dtype)
    elif epi == "sebwd":
        d["b"] = _act((M, N), seed + 8, dtype)
        d["escale"], d["eshift"] = _rnd((N,), seed + 9).abs() + 0.5, _rnd((N,), seed + 10, 0.3)
        d["emean"], d["erstd"] = _rnd((N,), seed + 11, 0.5), _rnd((N,), seed + 12).abs() + 0.5
        if gated:
            d["egate"] = torch.sigmoid(_rnd((B, N), seed + 13))
    r = {k: v.clone().double() for k, v in d.items()}          # what the reference sees
    if tamper is not None:
        tamper(d)

    # ---- the launch
    wv, w_sn, w_sk = _weight_view(d["w"], layout)
    kw, keep = {}, {}
    if pro == "swish":
        kw.update(pro_p=_dev(torch.cat([_pad(d["scale"], Kp), _pad(d["shift"], Kp)])), rows_per_sample=rps,
                  pro_gate=_dev(d["gate"], Kp) if gated else None)
    elif pro == "affine":
        kw["x2"] = _dev(d["x2"], Kp, dtype)
        if use_fin:
            kw["fin"] = _fin_bwd(cc, K, Kp, keep)
        else:
            kw["pro_p"] = _dev(_pad(d["coef"], Kp).reshape(-1))
    y = torch.full((M, Np), float("nan"), dtype=dtype, device=DEV)
    if epi == "add":
        if alias:          # the in-place dx accumulation of linear_bwd: the residual IS the output buffer
            y = _dev(d["res"], Np, dtype)
            kw["e1"] = y
        else:
            kw["e1"] = _dev(d["res"], Np, dtype)
        kw.update(res_mode=res_mode, H=H, W=W)
    stats = None
    if epi == "stats":
        stats = torch.zeros(ops.STAT_STRIPES * 2 * N, dtype=torch.float64, device=DEV)
    elif epi == "sebwd":
        stats = torch.zeros(B * Np * 3, dtype=torch.float64, device=DEV)
        kw.update(e1=_dev(d["b"], Np, dtype), epi_p=_dev(torch.cat([_pad(d["escale"], Np), _pad(d["eshift"], Np)])),
                  epi_q=_dev(torch.cat([_pad(d["emean"], Np), _pad(d["erstd"], Np)])),
                  epi_gate=_dev(d["egate"], Np) if gated else None, rows_per_sample=rps)
    if stride2 and not dense_instead:
        kw.update(row_mode=ops.ROWS_STRIDE2, H=H, W=W)
    xd = _dev(d["x"], Kp, dtype)
    ops.pw_gemm(xd, wv, y, M=M, K=K, N=N, w_sn=w_sn, w_sk=w_sk, dtype=ops.dt_code(dtype), pro_mode=PRO[pro], epi_mode=EPI[epi],
                stats=stats, bias=_dev(d["bias"]) if bias else None, **kw)
    kernel = ops.last_kernel()
    torch.cuda.synchronize()
    assert kernel == f"pw_wide_kernel<{_tn(dtype)}, {PRO[pro]}, {EPI[epi]}>", kernel

    # ---- the float64 restatement
    what = f"M {M} K {K} N {N} {pro}+{epi}" + (" bias" if bias else "") + f" w:{layout}" + (f" rows/sample {rps}" + ("" if gated else " no gate") if rps else "") \
        + (f" res_mode {res_mode}" if epi == "add" else "") + (" aliased" if alias else "") + (" stride2" if stride2 else "") + (" fin" if use_fin else "")
    bd = WideBound(kernel, what)
    xr = WR.gather_stride2(r["x"], BT, H, W) if stride2 else r["x"]
    if pro == "none":
        P, ps = WR.pro_none(xr)
    elif pro == "swish":
        P, ps = WR.pro_swish(xr, r["scale"], r["shift"], WR.sample_rows(r["gate"], M, rps) if gated else None, bf16)
    else:
        x2r = WR.gather_stride2(r["x2"], BT, H, W) if stride2 else r["x2"]
        P, ps = WR.pro_affine2(xr, x2r, r["coef"][0], r["coef"][1], r["coef"][2], bf16)
    yr, mag, sl = WR.gemm(P, ps, r["w"], bf16, r.get("bias"))
    eps, rel = EPS_GEMM(K, dtype), (2.0 ** -8 if bf16 else 2.0 ** -24)
    yd = _d(y)
    bd.exact_zero("padding channels of y", y[:, N:])
    if epi == "add":
        yr, mag = WR.epi_add(yr, mag, r["res"], res_mode, BT, H, W)
    if epi != "sebwd":
        bd.add("y", yd[:, :N], yr, mag, eps, rel=rel, slack=sl)
    else:
        o = WR.epi_swish_se_bwd(yr, eps * mag + sl, r["b"], r["escale"], r["eshift"], WR.sample_rows(r["egate"], M, rps) if gated else None)
        bd.add("t", yd[:, :N], o["t"], o["t_err"], 1.0, rel=rel)
        nc3 = _d(stats).view(B, Np, 3)
        assert bool((nc3[:, N:] == 0).all()), "padding channels of the per-sample sums must be exact zeros"
        fix = 18 * (rps // 64 + 2) * 2.0 ** -41
        bd.add("s0", nc3[:, :N, 0], WR.sample_sum(o["s0_term"], rps), WR.sample_sum(o["s0_mag"], rps), EPS_S0, slack=WR.sample_sum(o["s0_err"], rps) + fix)
        s1, s2, m1, m2 = WR.se_bwd_sums_of_stored(yd[:, :N], r["b"], r["emean"], r["erstd"], rps)
        bd.add("s1", nc3[:, :N, 1], s1, m1, EPS_S1, slack=torch.full_like(s1, fix))
        bd.add("s2", nc3[:, :N, 2], s2, m2, EPS_S2, slack=torch.full_like(s2, fix))
    if epi == "stats":
        s, sm = WR.stripe_stats(yd[:, :N])
        bd.add("stats", _d(stats).view(ops.STAT_STRIPES, 2, N), s, sm, EPS_STATS)
    if use_fin:
        _check_fin(bd, cc, keep, K, Kp)
    return bd, dict(y=y, stats=stats, keep=keep, x=xd)


# ---- linear layers: NONE + STORE with bias
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("layout", ["kc", "tr", "slice"])
@pytest.mark.parametrize("M,K,N", [(343, 192, 576), (343, 192, 203), (70, 20, 5), (517, 192, 192), (130, 1024, 1024)])
def test_linear_bias(dtype, layout, M, K, N):
    """Weight staging.  "kc": w_sk = 1, float4 path (K % 4 == 0 at all five shapes).  "tr": w_sn = 1, float4 path at N = 576, 192, 1024,
    scalar path at N = 203 and 5.  "slice": w_sk = 1 from a base that is 4 bytes off a 16-byte boundary, scalar path.
    (70, 20, 5) reaches the wide kernel through the bias alone; (130, 1024, 1024) is the largest shape c3d_pw_gemm admits."""
    _need_gpu()
    run_gemm(dtype, M, K, N, bias=True, layout=layout, seed=100 + K + N)[0].check()


# ---- NONE + STATS
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("K", [96, 192])
def test_none_stats(dtype, K):
    """20 row blocks: the 16 stripes wrap, the last block has 23 rows; every stripe is compared on its own."""
    _need_gpu()
    run_gemm(dtype, 64 * 19 + 23, K, 432, epi="stats", seed=200 + K)[0].check()


# ---- NONE + ADD
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("res_mode,alias", [(0, False), (0, True), (1, False)])
def test_none_add(dtype, res_mode, alias):
    _need_gpu()
    run_gemm(dtype, 5 * 6 * 8, 192, 432, epi="add", res_mode=res_mode, alias=alias, BT=5, H=6, W=8, seed=300)[0].check()


# ---- BN_SE_SWISH + STORE / STATS
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("gated", [True, False])
@pytest.mark.parametrize("rps,M", [(16, 176), (17, 153), (48, 144), (192, 232)])
def test_bn_se_swish_store_and_stats(dtype, gated, rps, M):
    """432 -> 192, three or four row blocks with a ragged last one (at 192 rows per sample the second sample is partial)."""
    _need_gpu()
    for epi in ("store", "stats"):
        run_gemm(dtype, M, 432, 192, pro="swish", epi=epi, gated=gated, rps=rps, seed=400 + rps)[0].check()


# ---- AFFINE2 + STORE / ADD, coefficients from pro_p and from fin.sums
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N", [192, 96])
@pytest.mark.parametrize("epi,res_mode", [("store", 0), ("add", 0), ("add", 1)])
def test_affine2_store_and_add(dtype, N, epi, res_mode):
    """432 -> 192 (4 x 2 workgroups) and 432 -> 96.  The fin launch: workgroup (0, 0) alone adds dgamma / dbeta (they start non-zero and
    must hold start + sums, once), fin.ss holds the coefficients, and its output is bit-identical to a pro_p launch fed fin.ss."""
    _need_gpu()
    a = dict(pro="affine", epi=epi, res_mode=res_mode, BT=5, H=6, W=8, layout="tr", seed=500 + N)
    run_gemm(dtype, 240, 432, N, **a)[0].check()
    bd, out = run_gemm(dtype, 240, 432, N, use_fin=True, **a)
    bd.check()
    _, again = run_gemm(dtype, 240, 432, N, pro_p_from=out["keep"]["ss"], **a)
    assert torch.equal(out["y"].view(torch.int16 if dtype == BF else torch.int32), again["y"].view(torch.int16 if dtype == BF else torch.int32))


# ---- AFFINE2 + SWISH_SE_BWD
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("gated", [True, False])
@pytest.mark.parametrize("rps,M", [(16, 176), (17, 153), (21, 147), (48, 144), (192, 344), (200, 400)])
def test_affine2_swish_se_bwd(dtype, gated, rps, M):
    """192 -> 432.  A 64-row block spans 5 samples at 17 rows per sample, 4 at 16 and 21.  M is no multiple of 64; at 192 rows per
    sample (a multiple of 64 itself) the second sample is partial, which is what nmax is for.  Two runs: bit-identical sums."""
    _need_gpu()
    a = dict(pro="affine", epi="sebwd", gated=gated, rps=rps, layout="tr", seed=600 + rps)
    bd, one = run_gemm(dtype, M, 192, 432, **a)
    bd.check()
    _, two = run_gemm(dtype, M, 192, 432, **a)
    assert torch.equal(one["stats"].view(torch.int64), two["stats"].view(torch.int64)), "the fixed-point sums must not depend on the order of arrival"


# ---- the stride-2 gather
@pytest.mark.parametrize("dtype", DTYPES)
def test_stride2_gather(dtype):
    """K = 432 on 6 x 8 maps, 11 frames: 132 output rows (three row blocks, the last ragged)."""
    _need_gpu()
    run_gemm(dtype, 11 * 3 * 4, 432, 192, stride2=True, BT=11, H=6, W=8, seed=700)[0].check()


# ---- the res5 layers at the change-captioning benchmark's shape (B = 16, three frames: 16 x 16 maps in, 8 x 8 inside; model/x3d.py)
RES5 = {
    "conv_a of block 0": dict(M=12288, K=96, N=432, epi="stats"),
    "conv_a": dict(M=3072, K=192, N=432, epi="stats"),
    "conv_c": dict(M=3072, K=432, N=192, pro="swish", epi="stats", rps=192),
    "conv_c data gradient": dict(M=3072, K=192, N=432, pro="affine", epi="sebwd", rps=192, layout="tr"),
    "conv_a data gradient": dict(M=3072, K=432, N=192, pro="affine", epi="add", layout="tr"),
    "conv_a data gradient of block 0": dict(M=12288, K=432, N=96, pro="affine", epi="add", res_mode=1, BT=48, H=16, W=16, layout="tr"),
}


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("layer", list(RES5))
def test_res5_layers_at_the_cc_benchmark_shape(dtype, layer):
    _need_gpu()
    a = dict(RES5[layer])
    run_gemm(dtype, a.pop("M"), a.pop("K"), a.pop("N"), seed=800, **a)[0].check()


# ---- refusals
def _refused(fn, *untouched):
    from change3d_amd import ops
    from change3d_amd._lib import Change3DHipError
    run_gemm(BF, 70, 20, 5, bias=True)                       # a wide launch of another instantiation in front
    before, count = ops.last_kernel(), ops.launch_count()
    assert before == "pw_wide_kernel<unsigned short, 0, 0>"
    with pytest.raises(Change3DHipError, match="code -2"):          # C3D_E_UNSUPPORTED
        fn(ops)
    torch.cuda.synchronize()
    assert ops.last_kernel() == before and ops.launch_count() == count, "nothing may be launched"
    for t, v in untouched:
        assert bool(torch.isnan(t).all()) if v is None else bool((t == v).all()), "outputs must stay untouched"


@pytest.mark.parametrize("which", ["rows_per_sample 15", "Kp 1032", "fin.ticket", "pro_out"])
def test_refusals_return_unsupported_and_launch_nothing(which):
    _need_gpu()
    from change3d_amd import ops
    from change3d_amd import _lib as L
    M, K, N = 150, (1032 if which == "Kp 1032" else 432), 192
    Kp, Np = ops.cpad(K), ops.cpad(N)
    x = _dev(_act((M, K), 1, BF), Kp, BF)
    w = _rnd((N, K), 2, 0.1).to(DEV)
    y = torch.full((M, Np), float("nan"), dtype=BF, device=DEV)
    stats = torch.zeros(10 * Kp * 3, dtype=torch.float64, device=DEV)
    coef = torch.ones(3 * Kp, dtype=F32, device=DEV)
    out2 = torch.full((M, Kp), float("nan"), dtype=BF, device=DEV)
    ticket = torch.zeros(4, dtype=torch.int32, device=DEV)
    base = dict(M=M, K=K, N=N, w_sn=K, w_sk=1, dtype=ops.DT_BF16)
    if which == "rows_per_sample 15":
        yb = torch.full((M, Kp), float("nan"), dtype=BF, device=DEV)
        ones = torch.ones(2 * Kp, dtype=F32, device=DEV)

        def fn(o):          # 192 -> 432 as the conv_c data gradient, 15 rows per sample: a block could span six samples
            o.pw_gemm(y, w, yb, M=M, K=N, N=K, w_sn=1, w_sk=K, dtype=o.DT_BF16, x2=y, pro_mode=o.PRO_AFFINE2, pro_p=coef, epi_mode=o.EPI_SWISH_SE_BWD,
                      e1=x, epi_p=ones, epi_q=ones, stats=stats, rows_per_sample=15)
        y.zero_()
        _refused(fn, (yb, None), (stats, 0))
        return
    if which == "Kp 1032":
        def fn(o):
            o.pw_gemm(x, w, y, **base)
    elif which == "fin.ticket":
        f = L.BnFin()
        f.ticket = ticket.data_ptr()

        def fn(o):
            o.pw_gemm(x, w, y, epi_mode=o.EPI_STATS, stats=stats, fin=f, **base)
    else:
        def fn(o):
            o.pw_gemm(x, w, y, x2=x, pro_mode=o.PRO_AFFINE2, pro_p=coef, pro_out=out2, **base)
    _refused(fn, (y, None), (out2, None), (stats, 0), (ticket, 0))


# ================================================================================================ weight gradient
def run_wgrad(dtype, M, K, N, form, rps=0, gated=True, tamper=None, seed=1000):
    """One c3d_pw_wgrad launch, dW accumulated into a strided, offset view that starts non-zero.  form: "plain"; "coef": p affine
    through p_coef, q Swish; "fin": the same with the coefficients rebuilt from p_fin.  Returns the bound and the view's storage."""
    from change3d_amd import ops
    bf16 = dtype == BF
    Kp, Np = ops.cpad(K), ops.cpad(N)
    B = (M + rps - 1) // rps if rps else 1
    d = dict(p=_act((M, N), seed, dtype), q=_act((M, K), seed + 1, dtype))
    cc = None
    if form != "plain":
        d["p2"] = _act((M, N), seed + 2, dtype)
        cc = _coef_case(N, M, seed + 20)
        d["scale"], d["shift"] = _rnd((K,), seed + 3).abs() + 0.5, _rnd((K,), seed + 4, 0.3)
        if gated:
            d["gate"] = torch.sigmoid(_rnd((B, K), seed + 5))
    r = {k: v.clone().double() for k, v in d.items()}
    if tamper is not None:
        tamper(d)
    full = _rnd((N + 9, K + 3), seed + 6).to(DEV)          # dW = rows 5 .. 5 + N, columns 0 .. K of this
    start = full.clone()
    dw = full[5:5 + N, :K]
    kw, keep = {}, {}
    if form != "plain":
        kw.update(p2=_dev(d["p2"], Np, dtype), q_mode=ops.PRO_BN_SE_SWISH, q_ss=_dev(torch.cat([_pad(d["scale"], Kp), _pad(d["shift"], Kp)])),
                  q_gate=_dev(d["gate"], Kp) if gated else None, rows_per_sample=rps)
        if form == "fin":
            f = _fin_bwd(cc, N, Np, keep)
            f.running_mean = f.running_var = f.ss = None          # (the weight gradient accumulates nothing of these)
            kw["p_fin"] = f
        else:
            kw["p_coef"] = _dev(_pad(cc["coef"].float(), Np).reshape(-1))
    ops.pw_wgrad(_dev(d["p"], Np, dtype), _dev(d["q"], Kp, dtype), dw, M=M, K=K, N=N, dw_sn=K + 3, dw_sk=1, dtype=ops.dt_code(dtype), **kw)
    kernel = ops.last_kernel()
    torch.cuda.synchronize()
    # (192 x 203 pads to 192 x 208, under the 224 of the dispatch rule: both narrow kernels answer C3D_E_UNSUPPORTED for its tile
    # plan and c3d_pw_wgrad falls through to the block-tiled kernel)
    assert kernel == f"pw_wide_wgrad_kernel<{_tn(dtype)}>", kernel
    rows, split = WR.wgrad_plan(M, K, N, torch.cuda.get_device_properties(0).multi_processor_count)
    assert rows <= 256 and split <= 32, (rows, split)          # what EPS_WGRAD counts
    what = f"M {M} K {K} N {N} {form}" + (f" rows/sample {rps}" + ("" if gated else " no gate") if form != "plain" else "")
    bd = WideBound(kernel, what)
    if form == "plain":
        (P, ps), (Q, qs) = WR.pro_none(r["p"]), WR.pro_none(r["q"])
    else:
        P, ps = WR.pro_affine2(r["p"], r["p2"], cc["coef"][0], cc["coef"][1], cc["coef"][2], bf16)
        Q, qs = WR.pro_swish(r["q"], r["scale"], r["shift"], WR.sample_rows(r["gate"], M, rps) if gated else None, bf16)
    ref, mag, sl = WR.wgrad(P, ps, Q, qs)
    s0 = _d(start[5:5 + N, :K])
    bd.add("dW", _d(dw), s0 + ref, mag + s0.abs(), EPS_WGRAD(dtype), slack=sl)
    outside = torch.ones_like(full, dtype=torch.bool)
    outside[5:5 + N, :K] = False
    assert torch.equal(full[outside], start[outside]), "rows and columns outside the dW view must stay untouched"
    return bd, full


WG_ROWS = {5: 16, 31: 17, 128: 192, 450: 17, 3072: 192}          # rows per sample of the Swish operand at each M


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("M", [5, 31, 128, 450, 3072])
@pytest.mark.parametrize("K,N", [(432, 192), (192, 432), (96, 432), (192, 576), (192, 203)])
def test_wgrad(dtype, M, K, N):
    """M = 5 and 31: less than one 32-row chunk; 128: one split; 450: a short last split (66 rows of 128); 3072: the res5 shape.
    Plain operands; p affine through p_coef with q Swish, gated and ungated, at 16 / 17 / 192 rows per sample; the same with the
    coefficients rebuilt from p_fin, bit-identical to the p_coef launch wherever one split fixes the order of the sum (M <= 128).  (192, 203) pads to 192 x 208: it reaches
    the block-tiled kernel because both narrow kernels refuse its tile plan."""
    _need_gpu()
    seed = 1000 + M + K
    failed = []
    bd, _ = run_wgrad(dtype, M, K, N, "plain", seed=seed)
    failed += _failure(bd)
    for rps, gated in ((WG_ROWS[M], True), (16 if WG_ROWS[M] != 16 else 17, False)):
        bd, a = run_wgrad(dtype, M, K, N, "coef", rps, gated, seed=seed)
        failed += _failure(bd)
        bd, b = run_wgrad(dtype, M, K, N, "fin", rps, gated, seed=seed)
        failed += _failure(bd)
        # one split: start + sum, nothing depends on an order of arrival.  With several splits each adds its f32 partial to dW
        # with an atomic, in whatever order they finish: two launches of the SAME form need not agree in the last bit, so
        # there the two forms are tied through the bound alone
        if WR.wgrad_plan(M, K, N, torch.cuda.get_device_properties(0).multi_processor_count)[1] == 1:
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), "p_fin must equal p_coef bit for bit"
    assert not failed, "\n".join(failed)


def _failure(bd):
    try:
        bd.check()
    except AssertionError as e:
        return [str(e)]
    return []


# ================================================================================================ negative controls
def _weight_in_last_chunk(d):
    n = int(d["w"][:, 430].abs().argmax())
    d["w"][n, 430] *= 1 + 2.0 ** -5          # channel 430: the last, partial K chunk of both storage types (48 of 64, 16 of 32)


def _last_input_element(d):
    d["x"][-1, -1] += 1.0                    # channel K - 1 of the last row


def _gate_of_fifth_slot(d):
    d["egate"][7, 200] *= 1.05               # 17 rows per sample: rows 64 .. 127 touch samples 3 .. 7, the fifth slot is sample 7


def _bias_above_224(d):
    d["bias"][300] += 0.05


def _zero_last_row_of_a_split(d):
    d["p"][127] = 0                          # M = 450: four splits of 128 rows


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("control", ["weight", "input", "gate", "bias", "gather", "wgrad"])
def test_bound_sees_one_wrong_input(dtype, control):
    """Negative controls: the device's input differs from the reference's in one place; the comparison must raise."""
    _need_gpu()
    if control == "weight":
        bd, _ = run_gemm(dtype, 144, 432, 192, pro="swish", gated=True, rps=48, tamper=_weight_in_last_chunk, seed=448)
    elif control == "input":
        bd, _ = run_gemm(dtype, 240, 192, 432, epi="add", tamper=_last_input_element, seed=300)
    elif control == "gate":
        bd, _ = run_gemm(dtype, 153, 192, 432, pro="affine", epi="sebwd", gated=True, rps=17, layout="tr", tamper=_gate_of_fifth_slot, seed=617)
    elif control == "bias":
        bd, _ = run_gemm(dtype, 343, 192, 576, bias=True, tamper=_bias_above_224, seed=868)
    elif control == "gather":
        bd, _ = run_gemm(dtype, 132, 432, 192, stride2=True, BT=11, H=6, W=8, dense_instead=True, seed=700)
    else:
        bd, _ = run_wgrad(dtype, 450, 432, 192, "plain", tamper=_zero_last_row_of_a_split, seed=1882)
    print(f"\nWIDE-NEG {control} {bd.kernel}: error/bound {bd.worst():.2f}")
    with pytest.raises(AssertionError, match="bound exceeded"):
        bd.check(record=False)


def test_zz_report_worst_ratio_per_kernel():
    """Printed last: the worst error / bound seen per kernel by the cases above (informational; each case asserted its own)."""
    _need_gpu()
    for k in sorted(WORST):
        print(f"\nWIDE-WORST {k}: {WORST[k]:.3f}")
