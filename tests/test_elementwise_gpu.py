"""csrc/elementwise.hip against float64, kernel by kernel: the res-block / stem output forward and backward (with the shortcut
BatchNorm branch, the pre-masked form and the fin.ticket tail of c3d_block_out_bwd_fin), the pieces of Encoder.enhance and
frame_scatter.

Every case calls ONE entry point through `ops`, asserts which instantiation ran (c3d_last_kernel), pre-fills every output with
NaN, requires the padding channels of every output to come back as exact zeros and compares every output element by element
with the restatement in tests/elementwise_reference.py (pinned against torch.autograd by
tests/test_elementwise_reference_cpu.py).  The worst error / bound per kernel is printed by the closing test (ELEMWISE lines;
run with -s).

Shapes: the smallest that reach each branch.  A thread keeps one 8-channel vector: G = Cp / 8 vectors per row, workgroups of
blk = G * (256 // G) threads, i.e. 256 // G whole rows.  The backward grid is min(ceil(rows / (256 // G)), 384) workgroups, so
S = 384 * (256 // G) rows are one grid stride, and a thread has four rows in flight (BOB_U): one load batch covers 4 S rows.
  widths   C -> (Cp, G, blk): 8 -> (8, 1, 256), 24 -> (24, 3, 255), 54 -> (56, 7, 252), 108 -> (112, 14, 252),
           216 -> (216, 27, 243: blockDim & ~15 = 240 in the ticket tail), 256 -> (256, 32, 256) the limit.  54 and 108 are the
           widths where the `ch < C` guard matters and dsums is [2][C], not [2][Cp].
  rows     1;  256 // G - 1 and + 1 (one workgroup short / over);  S and S + 1;  4 S + 1 (the second batch holds one row, in
           workgroup 0);  5 S + S // 2 + 3 (slot 0 full, slot 1 half, slots 2 and 3 empty);  7 S + 5 (all four slots, the last
           partial) for C = 24, 54, 216;  1, S + 1 and 5 S + S // 2 + 3 for the other widths.  The largest is C = 24 with
           228 485 rows, 5.5 M elements.
  forward  the one-workgroup cases, C = 216 with 4096 * 9 + 3000 rows (the grid-stride loop wraps past the 4096-workgroup
           cap); the wrap of c3d_block_out_fwd_fin past ITS cap of 1024 is a case of the bit-identity test in tests/test_ops_gpu.py,
           whose unfolded leg this file ties to float64.
  enhance  T in 3 / 4 / 5, B in 1 / 3, Cp in 24 / 56, 20 x 28 pixels (a frame is no multiple of 256 vectors: workgroups straddle
           samples), t_pre > t_post once, both frame indices out of range; one bf16 case past 4096 workgroups (Cp = 256, B = 3,
           T = 3, 112 x 112).
The walk cases assume the default grid caps and are skipped when the instrumented build's C3D_BOB_GRID / C3D_BOF_GRID is set.

Bounds, derived (u = 2^-24, the unit roundoff of f32):
  g        a copy of dy under the mask of the stored y: EXACTLY the restatement, both storage types.
  forward  two fma and one add: 3 u of mag = |c||a| + |b| + |s||a1| + |b1|, eps = 2^-22, E = eps mag.
           f32 storage |dev - ref| <= E;  bf16 storage |dev - ref| <= 2^-8 (|ref| + E) + E (the one rounding of the stored value,
           taken of the device's f32 value, which is within E of ref).  ReLU is 1-Lipschitz: the kink needs nothing extra.
  dsums    a thread adds its terms in f32, everything after that (workgroup reduction, atomics) is f64.  A term costs three
           roundings (c - mean, times rstd, times g), the chain of n = ceil(rows / (grid * rows per workgroup)) steps one each,
           every one at most u of the magnitude sum  sum |g| (|c| + |mean|) |rstd|  (sum |g| for the first row): E = eps times
           that, eps the smallest power of two >= (n_max + 3) u.  n_max is the longest chain among the cases: computed from the
           launch rule and asserted to be 8 (eps = 2^-20), so that a changed grid cap fails loudly.  dsums is pre-filled with
           non-zero values (the contract is +=) and carries a sentinel tail past 2 C.
  ticket   c3d_block_out_bwd_fin: fin.ss = A|B|C [3][Cp], fin.running_mean / running_var += dgamma / dbeta.  Bit for bit what
           c3d_bn_bwd_coef gives on the dsums the same call left (csrc/bn_fin.h promises the same arithmetic), and within 2^-21
           of the restatement's magnitude: computed in f64 from those sums and rounded to f32 at most twice on the way (the figure
           tests/test_hotpath_bf16_gpu.py derives for these vectors).  g is bit-identical to the same call without fin.  dsums
           too where that can be promised: one workgroup (the order of its atomics is fixed), and at the capped grid on inputs
           whose every f32 operation is exact (multiples of 1/4, rstd a power of two): there the sums do not depend on the order
           in which 384 workgroups' f64 atomics land; on random data they do, in the last bits, with or without fin.
  enhance  one f32 operation on stored values and one rounding (the product with the sign is exact): EXACTLY `.float()`, the
           operation, `.to(dtype)` in torch on the CPU.

Negative controls, one per family, each an ordinary valid launch whose input differs from the reference's in one place; the
same comparison must raise: a dy row zeroed in the partial slot of the last load batch; mean_1 of one channel scaled by
1 + 2^-10 (dsums_1's second row must see it, dsums_c must not); scale_c of one channel scaled by 1 + 2^-5; a t_post one frame
off in enhance_bwd_apply (t_pre and t_post SWAPPED is no control: the operation is symmetric in them, and a test here requires
the swapped launch to give the same dy bit for bit); a ticket pre-set to 1 in a one-workgroup launch (the tail never fires: the NaN-filled coefficient
vector comes back unchanged; nothing waits on the ticket)."""
import os
import types

import pytest
import torch

import elementwise_reference as E

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BF = torch.bfloat16
DTYPES = [torch.bfloat16, torch.float32]
WORST, CONTROLS = {}, {}
TAIL = 8
SENTINEL = -777.25

WIDTHS_FULL, WIDTHS_SHORT = (24, 54, 216), (8, 108, 256)


def _rows(C, full):
    _, G, _, rows, S = E.launch_rule(C)
    if full:
        return [1, rows - 1, rows + 1, S, S + 1, 4 * S + 1, 5 * S + S // 2 + 3, 7 * S + 5]
    return [1, S + 1, 5 * S + S // 2 + 3]


BWD_CASES = [(C, M) for C in WIDTHS_FULL for M in _rows(C, True)] + [(C, M) for C in WIDTHS_SHORT for M in _rows(C, False)]
N_MAX = max(E.chain_steps(M, C) for C, M in BWD_CASES)
EPS_SUMS = E.sums_eps(N_MAX)


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")


def _walks_need_default_caps(M, C):
    _, _, _, rows, _ = E.launch_rule(C)
    if M > rows + 1 and (os.environ.get("C3D_BOB_GRID") or os.environ.get("C3D_BOF_GRID")):
        pytest.skip("walk case: the shapes assume the default grid caps (C3D_BOB_GRID / C3D_BOF_GRID is set)")


def _tn(dtype):
    return "float" if dtype == torch.float32 else "unsigned short"


class Bound:
    """Collects error / bound of one case; `check()` raises at the end so that every output is reported."""

    def __init__(self, kernel, shape):
        self.kernel, self.shape, self.rows = kernel, shape, {}

    def _put(self, what, r):
        self.rows[what] = max(self.rows.get(what, 0.0), r)

    def add(self, what, dev, ref, mag, eps, rel=0.0):
        dev, ref = dev.double(), ref.double()
        e = eps * mag
        lim = rel * (ref.abs() + e) + e
        err = (dev - ref).abs()
        ratio = torch.where(err > 0, err / lim, torch.zeros_like(err))      # (an error where the bound is 0 is inf)
        ratio = torch.where(torch.isfinite(dev), ratio, torch.full_like(ratio, float("inf")))
        self._put(what, float(ratio.max()) if ratio.numel() else 0.0)

    def exact(self, what, dev, ref):
        """bit-for-bit as values (NaN equals NaN: an untouched NaN-filled vector is `exact` against itself)"""
        same = (dev == ref) | (torch.isnan(dev) & torch.isnan(ref))
        self._put(what, 0.0 if bool(same.all()) else float("inf"))

    def exact_zero(self, what, t):
        if t.numel():
            assert bool((t.float() == 0).all()), f"{self.kernel} {self.shape}: {what} must be exact zeros"

    def worst(self):
        return max(self.rows.values())

    def check(self, record=True):
        line = ", ".join(f"{k} {v:.3f}" for k, v in self.rows.items())
        if record:
            print(f"\nELEMWISE {self.kernel} | {self.shape} | error/bound: {line}")
            for k, v in self.rows.items():
                key = (self.kernel, k.split("[")[0])
                WORST[key] = max(WORST.get(key, 0.0), v)
        assert self.worst() <= 1.0, f"bound exceeded: {self.kernel} {self.shape}: {line}"


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def _randn(g, *shape):
    return torch.randn(*shape, generator=g, device=DEV, dtype=torch.float32)


def _rand(g, *shape):
    return torch.rand(*shape, generator=g, device=DEV, dtype=torch.float32)


def _store(t, C, Cp, dtype):
    """[..., C] f32 -> the device's tensor [..., Cp] in the storage type, padding channels zero"""
    out = torch.zeros(*t.shape[:-1], Cp, dtype=dtype, device=DEV)
    out[..., :C] = t.to(dtype)
    return out.contiguous()


def _vec(*rows_, C, Cp):
    """f32 rows [C] -> one [len(rows) * Cp] vector with zeros in [C, Cp) of every row"""
    out = torch.zeros(len(rows_), Cp, dtype=torch.float32, device=DEV)
    for i, r in enumerate(rows_):
        out[i, :C] = r
    return out.reshape(-1).contiguous()


def _ref(t, C):
    return t[..., :C].detach().cpu().double()


# ================================================================================================ block output, backward
def bwd_inputs(C, M, dtype, seed=0, exact=False):
    """dy with exact zeros and negatives (not centred: the sums do not cancel), y with a real share of zeros, scales of both
    signs in c, `mean` NOT the mean of c.  exact: every value a multiple of 1/4 and rstd a power of two -- all f32 arithmetic
    of the kernel is exact then, so the sums do not depend on the order of the atomics."""
    Cp = E.launch_rule(C)[0]
    g = _gen(7919 * C + M + 1000003 * seed + (1 if dtype == BF else 0))
    if exact:
        q = lambda t, lim: (t * 4).round().clamp(-4 * lim, 4 * lim) / 4    # noqa: E731
        dy, c, s = q(_randn(g, M, C) + 1.0, 2), q(_randn(g, M, C) * 2, 4), q(_randn(g, M, C) * 2 + 0.25, 4)
        mean_c, mean_1 = q(_randn(g, C) - 1.5, 3), q(_randn(g, C) + 0.75, 3)
        rstd_c = 2.0 ** torch.randint(-1, 2, (C,), generator=g, device=DEV).float()
        rstd_1 = 2.0 ** torch.randint(-1, 2, (C,), generator=g, device=DEV).float()
    else:
        dy = _randn(g, M, C) + 1.0
        c = _randn(g, M, C) * (0.5 + _rand(g, C)) * torch.where(_rand(g, C) < 0.3, -1.0, 1.0)
        s = _randn(g, M, C) + 0.3
        mean_c, rstd_c = -1.5 + 0.2 * _randn(g, C), 0.5 + _rand(g, C)
        mean_1, rstd_1 = 0.7 + 0.2 * _randn(g, C), 0.5 + _rand(g, C)
    dy[_rand(g, M, C) < 0.1] = 0.0
    y = torch.relu(_randn(g, M, C))
    y[0, 0], y[0, 1], dy[0, 1] = 0.0, 1.0, 1.5          # one masked and one live element even in a single row
    d = types.SimpleNamespace(C=C, Cp=Cp, M=M, dtype=dtype)
    d.dy, d.y, d.c, d.s = (_store(t, C, Cp, dtype) for t in (dy, y, c, s))
    d.dy_masked = torch.where(d.y > 0, d.dy, torch.zeros_like(d.dy))
    d.mr_c, d.mr_1 = _vec(mean_c, rstd_c, C=C, Cp=Cp), _vec(mean_1, rstd_1, C=C, Cp=Cp)
    d.gamma_c = (_randn(g, C).abs() + 0.5) * torch.where(_rand(g, C) < 0.3, -1.0, 1.0)
    d.gamma_1 = (_randn(g, C).abs() + 0.5) * torch.where(_rand(g, C) < 0.3, -1.0, 1.0)
    if exact:
        d.fill_c = torch.randint(-8, 9, (2 * C,), generator=g, device=DEV).double() + 0.5
        d.fill_1 = torch.randint(-8, 9, (2 * C,), generator=g, device=DEV).double() + 0.5
    else:
        d.fill_c, d.fill_1 = _randn(g, 2 * C).double() + 0.25, _randn(g, 2 * C).double() - 0.25
    d.fill_dg = _randn(g, 4, C)                         # dgamma_c | dbeta_c | dgamma_1 | dbeta_1 before the launch
    d.ref = None
    return d


def bwd_reference(d):
    """float64 restatement over what the reference sees (computed once per input set, before any tamper)"""
    if d.ref is None:
        C = d.C
        mc, m1 = d.mr_c.cpu().double().reshape(2, -1)[:, :C], d.mr_1.cpu().double().reshape(2, -1)[:, :C]
        d.ref = E.block_out_bwd(_ref(d.dy, C), _ref(d.y, C), _ref(d.c, C), mc[0], mc[1], _ref(d.s, C), m1[0], m1[1])
        d.ref["mc"], d.ref["m1"] = mc, m1
        assert bool((d.ref["g"] != 0).any()) and bool((d.ref["g"] == 0).any())
    return d.ref


def launch_bwd(d, shortcut, premasked, fin=False, ticket0=0):
    """one c3d_block_out_bwd(_fin) launch on NaN-filled / pre-filled outputs; returns what it left"""
    from change3d_amd import _lib, ops
    C, Cp, M, dtype = d.C, d.Cp, d.M, d.dtype
    o = types.SimpleNamespace(fin=fin, shortcut=shortcut, premasked=premasked)
    o.g = None if premasked else torch.full((M, Cp), float("nan"), dtype=dtype, device=DEV)
    tail = torch.full((TAIL,), SENTINEL, dtype=torch.float64, device=DEV)
    o.ds_c = torch.cat([d.fill_c, tail])
    o.ds_1 = torch.cat([d.fill_1, tail]) if shortcut else None
    args = (d.dy_masked if premasked else d.dy, None if premasked else d.y, d.c, d.s if shortcut else None, o.g, d.mr_c,
            d.mr_1 if shortcut else None, o.ds_c, o.ds_1, M, C, ops.dt_code(dtype))
    if fin:
        o.ticket = torch.full((1,), ticket0, dtype=torch.int32, device=DEV)
        o.coef_c, o.coef_1 = (torch.full((3 * Cp,), float("nan"), device=DEV) for _ in range(2))
        o.dg = d.fill_dg.clone()
        fc, f1 = _lib.BnFin(), _lib.BnFin()
        fc.ticket, fc.gamma, fc.ss, fc.mr, fc.count = o.ticket.data_ptr(), d.gamma_c.data_ptr(), o.coef_c.data_ptr(), d.mr_c.data_ptr(), float(M)
        fc.running_mean, fc.running_var = o.dg[0].data_ptr(), o.dg[1].data_ptr()
        f1.gamma, f1.ss, f1.mr, f1.count = d.gamma_1.data_ptr(), o.coef_1.data_ptr(), d.mr_1.data_ptr(), float(M)
        f1.running_mean, f1.running_var = o.dg[2].data_ptr(), o.dg[3].data_ptr()
        ops.block_out_bwd_fin(*args, fc, f1 if shortcut else None)
    else:
        ops.block_out_bwd(*args)
    o.kernel = ops.last_kernel()
    torch.cuda.synchronize()
    assert o.kernel == f"block_out_bwd_kernel<StoredOperands<{_tn(dtype)}, {'true' if premasked else 'false'}>>", o.kernel
    return o


def check_bwd(d, o, ref, b, tag=""):
    """g exactly, the sums under the derived bound, the sentinel tails, the padding channels"""
    C = d.C
    if not o.premasked:
        b.exact("g" + tag, o.g[:, :C].cpu().double(), ref["g"])
        b.exact_zero("g padding", o.g[:, C:])
    fill_c, fill_1 = d.fill_c.cpu().reshape(2, C), d.fill_1.cpu().reshape(2, C)
    b.add("dsums_c" + tag, o.ds_c[:2 * C].cpu().reshape(2, C), fill_c + ref["sums_c"], ref["mag_c"], EPS_SUMS)
    assert bool((o.ds_c[2 * C:] == SENTINEL).all()), "dsums_c: written past 2 C"
    if o.shortcut:
        s1, mg1 = ref["sums_1"], ref["mag_1"]
        b.add("dsums_1[0]" + tag, o.ds_1[:C].cpu(), fill_1[0] + s1[0], mg1[0], EPS_SUMS)
        b.add("dsums_1[1]" + tag, o.ds_1[C:2 * C].cpu(), fill_1[1] + s1[1], mg1[1], EPS_SUMS)
        assert bool((o.ds_1[2 * C:] == SENTINEL).all()), "dsums_1: written past 2 C"


def check_fin(d, o, b):
    """the ticket tail: bit for bit c3d_bn_bwd_coef on the dsums the call left, within 2^-21 of the restatement from them,
    zeros in the padding channels of the coefficient vectors"""
    from change3d_amd import ops
    C, Cp, M = d.C, d.Cp, d.M
    legs = [("c", o.ds_c, d.gamma_c, d.mr_c, o.coef_c, 0)] + ([("1", o.ds_1, d.gamma_1, d.mr_1, o.coef_1, 2)] if o.shortcut else [])
    for name, ds, gamma, mr, coef, k in legs:
        bn = types.SimpleNamespace(weight=torch.nn.Parameter(gamma.clone()), bias=torch.nn.Parameter(torch.zeros_like(gamma)))
        bn.weight.grad, bn.bias.grad = d.fill_dg[k].clone(), d.fill_dg[k + 1].clone()
        coef2 = torch.full((3 * Cp,), float("nan"), device=DEV)
        ops.bn_bwd_coef(ds, float(M), bn, mr, C, coef2)
        torch.cuda.synchronize()
        b.exact(f"coef_{name} = bn_bwd_coef", coef, coef2)
        b.exact(f"dgamma_{name} = bn_bwd_coef", o.dg[k], bn.weight.grad)
        b.exact(f"dbeta_{name} = bn_bwd_coef", o.dg[k + 1], bn.bias.grad)
        m2 = mr.cpu().double().reshape(2, Cp)[:, :C]
        r = E.bn_bwd_coef(ds[:2 * C].cpu().reshape(2, C), float(M), gamma.cpu().double(), m2[0], m2[1])
        cf = coef.cpu().reshape(3, Cp)
        for i, key in enumerate("ABC"):
            b.add(f"{key}_{name}", cf[i, :C], r[key], r["mag"][key], E.EPS_COEF)
        b.exact(f"coef_{name} padding = 0", cf[:, C:], torch.zeros(3, Cp - C))
        fill = d.fill_dg.cpu().double()
        b.add(f"dgamma_{name}", o.dg[k].cpu(), fill[k] + r["dgamma"], fill[k].abs() + r["mag"]["dgamma"], E.EPS_COEF)
        b.add(f"dbeta_{name}", o.dg[k + 1].cpu(), fill[k + 1] + r["dbeta"], fill[k + 1].abs() + r["mag"]["dbeta"], E.EPS_COEF)
    if not o.shortcut:
        assert bool(torch.isnan(o.coef_1).all()) and torch.equal(o.dg[2:], d.fill_dg[2:]), "fin_1 written without a shortcut"


def test_longest_chain_is_what_the_bound_assumes():
    """n_max from the launch rule: 8 steps at 7 S + 5 rows, eps = 2^-20.  A changed grid cap or load batch changes the walks
    these shapes were chosen for."""
    assert N_MAX == 8 and EPS_SUMS == 2.0 ** -20
    assert (E.BOB_GRID_CAP, E.BOB_U) == (384, 4)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f32"])
@pytest.mark.parametrize("C,M", BWD_CASES)
def test_block_out_bwd_against_float64(C, M, dtype):
    """without shortcut, with s_bn + mr_1 + dsums_1, and both pre-masked forms, on one input set and one reference"""
    _need_gpu()
    _walks_need_default_caps(M, C)
    d = bwd_inputs(C, M, dtype)
    ref = bwd_reference(d)
    for premasked in (False, True):
        for shortcut in (False, True):
            o = launch_bwd(d, shortcut, premasked)
            b = Bound(o.kernel, f"C {C} M {M} n {E.chain_steps(M, C)}{' shortcut' if shortcut else ''}")
            check_bwd(d, o, ref, b)
            b.check()


FIN_CASES = [(C, M) for C in WIDTHS_FULL for M in (1, 5 * E.launch_rule(C)[4] + E.launch_rule(C)[4] // 2 + 3)]


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f32"])
@pytest.mark.parametrize("shortcut", [False, True], ids=["plain", "shortcut"])
@pytest.mark.parametrize("C,M", FIN_CASES)
def test_block_out_bwd_fin_ticket_tail(C, M, shortcut, dtype):
    _need_gpu()
    _walks_need_default_caps(M, C)
    d = bwd_inputs(C, M, dtype, seed=1)
    ref = bwd_reference(d)
    o = launch_bwd(d, shortcut, False, fin=True)
    assert int(o.ticket) == min((M * (d.Cp // 8) + E.launch_rule(C)[2] - 1) // E.launch_rule(C)[2], E.BOB_GRID_CAP)   # every workgroup drew one
    b = Bound(o.kernel + " fin", f"C {C} M {M}{' shortcut' if shortcut else ''}")
    check_bwd(d, o, ref, b)
    check_fin(d, o, b)
    o0 = launch_bwd(d, shortcut, False)
    b.exact("g = without fin", o.g, o0.g)
    if M == 1:                                            # one workgroup: the order of the atomics is fixed
        b.exact("dsums = without fin", o.ds_c, o0.ds_c)
        if shortcut:
            b.exact("dsums_1 = without fin", o.ds_1, o0.ds_1)
    else:                                                 # 384 workgroups: on inputs whose f32 arithmetic is exact
        dx = bwd_inputs(C, M, dtype, seed=2, exact=True)
        rx = bwd_reference(dx)
        ox, ox0 = launch_bwd(dx, shortcut, False, fin=True), launch_bwd(dx, shortcut, False)
        b.exact("g = without fin (exact inputs)", ox.g, ox0.g)
        b.exact("dsums = without fin", ox.ds_c, ox0.ds_c)
        b.exact("dsums = float64 (exact inputs)", ox.ds_c[:2 * C].cpu(), dx.fill_c.cpu() + rx["sums_c"].reshape(-1))
        if shortcut:
            b.exact("dsums_1 = without fin", ox.ds_1, ox0.ds_1)
            b.exact("dsums_1 = float64 (exact inputs)", ox.ds_1[:2 * C].cpu(), dx.fill_1.cpu() + rx["sums_1"].reshape(-1))
        check_fin(dx, ox, b)
    b.check()


# ---- negative controls
def _control(name, b, what=None):
    rows = {k: v for k, v in b.rows.items() if what is None or k in what}
    CONTROLS[name] = max(rows.values())
    print(f"\nELEMWISE control {name}: error/bound " + ", ".join(f"{k} {v:.3g}" for k, v in b.rows.items()))
    with pytest.raises(AssertionError):
        b.check(record=False)
    assert CONTROLS[name] > 1.0


def test_control_a_zeroed_dy_row_in_the_last_partial_slot():
    _need_gpu()
    C = 24
    S = E.launch_rule(C)[4]
    M = 7 * S + 5
    _walks_need_default_caps(M, C)
    d = bwd_inputs(C, M, BF)
    ref = bwd_reference(d)
    d.dy[7 * S + 2] = 0          # row 2 of the five rows of slot 3 in the second batch; the reference keeps its dy
    o = launch_bwd(d, False, False)
    b = Bound(o.kernel, "control")
    b.add("dsums_c", o.ds_c[:2 * C].cpu().reshape(2, C), d.fill_c.cpu().reshape(2, C) + ref["sums_c"], ref["mag_c"], EPS_SUMS)
    _control("dy row zeroed in the last partial slot -> dsums_c", b)


def test_control_a_changed_shortcut_mean():
    _need_gpu()
    C = 54
    M = E.launch_rule(C)[4] + 1
    _walks_need_default_caps(M, C)
    d = bwd_inputs(C, M, torch.float32)
    ref = bwd_reference(d)
    d.mr_1[5] *= 1.0 + 2.0 ** -10
    o = launch_bwd(d, True, False)
    b = Bound(o.kernel, "control")
    check_bwd(d, o, ref, b)
    assert b.rows["dsums_c"] <= 1.0 and b.rows["dsums_1[0]"] <= 1.0 and b.rows["g"] == 0.0     # only the shat sums see it
    _control("mean_1 of one channel x (1 + 2^-10) -> dsums_1[1]", b, ("dsums_1[1]",))


def test_control_a_ticket_that_is_not_zero():
    """ticket = 1 before a one-workgroup launch: the workgroup draws 1, not gridDim - 1 = 0, so the tail never fires"""
    _need_gpu()
    d = bwd_inputs(54, 1, BF, seed=1)
    ref = bwd_reference(d)
    o = launch_bwd(d, True, False, fin=True, ticket0=1)
    assert int(o.ticket) == 2
    assert bool(torch.isnan(o.coef_c).all()) and bool(torch.isnan(o.coef_1).all()) and torch.equal(o.dg, d.fill_dg)
    b = Bound(o.kernel + " fin", "control")
    check_bwd(d, o, ref, b)                       # the sums themselves are complete
    assert b.worst() <= 1.0
    check_fin(d, o, b)
    _control("ticket pre-set to 1 -> coefficients", b)


# ================================================================================================ block output, forward
def _fwd_rows(C):
    rows = E.launch_rule(C)[3]
    return [1, rows - 1, rows + 1] if C in WIDTHS_FULL else [1]


FWD_CASES = [(C, M) for C in WIDTHS_FULL + WIDTHS_SHORT for M in _fwd_rows(C)] + [(216, 4096 * 9 + 3000)]


def run_fwd(C, M, dtype, mode, tamper=None):
    from change3d_amd import ops
    Cp = E.launch_rule(C)[0]
    g = _gen(104729 * C + M + (1 if dtype == BF else 0))
    c, s = _store(_randn(g, M, C), C, Cp, dtype), _store(_randn(g, M, C) + 0.3, C, Cp, dtype)
    sign = lambda: torch.where(_rand(g, C) < 0.3, -1.0, 1.0)      # noqa: E731
    ss_c = _vec((0.5 + _rand(g, C)) * sign(), 0.3 * _randn(g, C), C=C, Cp=Cp)
    ss_1 = _vec((0.5 + _rand(g, C)) * sign(), 0.3 * _randn(g, C), C=C, Cp=Cp)
    a, a1 = ss_c.cpu().double().reshape(2, Cp)[:, :C], ss_1.cpu().double().reshape(2, Cp)[:, :C]
    if mode == 0:
        ref, mag = E.block_out_fwd(_ref(c, C), a[0], a[1])
    elif mode == 2:
        ref, mag = E.block_out_fwd(_ref(c, C), a[0], a[1], _ref(s, C), a1[0], a1[1])
    else:
        ref, mag = E.block_out_fwd(_ref(c, C), a[0], a[1], _ref(s, C))
    if tamper is not None:
        tamper(ss_c)
    y = torch.full((M, Cp), float("nan"), dtype=dtype, device=DEV)
    ops.block_out_fwd(c, ss_c, s if mode else None, ss_1 if mode == 2 else None, mode, y, M, Cp, ops.dt_code(dtype))
    k = ops.last_kernel()
    torch.cuda.synchronize()
    assert k == f"block_out_fwd_kernel<{_tn(dtype)}>", k
    b = Bound(k, f"C {C} M {M} mode {mode}")
    b.add("y", y[:, :C].cpu(), ref, mag, E.EPS_FWD, rel=2.0 ** -8 if dtype == BF else 0.0)
    b.exact_zero("y padding", y[:, C:])
    if M > 1:
        assert bool((ref == 0).any()) and bool((ref > 0).any())
    return b


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f32"])
@pytest.mark.parametrize("C,M", FWD_CASES)
def test_block_out_fwd_against_float64(C, M, dtype):
    _need_gpu()
    _walks_need_default_caps(M, C)
    for mode in (0, 1, 2, 3):
        run_fwd(C, M, dtype, mode).check()


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f32"])
def test_control_a_changed_forward_scale(dtype):
    _need_gpu()

    def tamper(ss_c):
        ss_c[3] *= 1.0 + 2.0 ** -5

    _control(f"scale_c of one channel x (1 + 2^-5) -> y ({_tn(dtype)})", run_fwd(54, E.launch_rule(54)[3] + 1, dtype, 2, tamper))


# ================================================================================================ enhance pieces
def _rounded(t, dtype):
    return t.to(dtype)


def run_enhance(dtype, T, B, C, frames, H=20, W=28, bwd_apply_frames=None):
    """the five kernels on one input set: EXACTLY the same IEEE operation in torch on the CPU (f32, rounded to the storage
    type once).  One Bound per kernel.  bwd_apply_frames: the (t_pre, t_post) the DEVICE's enhance_bwd_apply gets, where they
    are to differ from the reference's."""
    from change3d_amd import ops
    t_pre, t_post, t_mid = frames
    Cp, HW = E.launch_rule(C)[0], H * W
    dt = ops.dt_code(dtype)
    g = _gen(31 * T + 7 * B + C + (1 if dtype == BF else 0))
    y = _randn(g, B, T, HW, C)
    y[:, t_post] = torch.where(_rand(g, B, HW, C) < 0.2, y[:, t_pre], y[:, t_post])       # y_pre == y_post: the sign is 0
    y, dout = _store(y, C, Cp, dtype), _store(_randn(g, B, T, HW, C) + 0.5, C, Cp, dtype)
    e = _randn(g, B, HW, C)
    e[_rand(g, B, HW, C) < 0.1] = 0.0
    e, dd, src = _store(e, C, Cp, dtype), _store(_randn(g, B, HW, C), C, Cp, dtype), _store(_randn(g, B, HW, C), C, Cp, dtype)
    yc, doc, ec, ddc, srcc = (t.cpu().float() for t in (y, dout, e, dd, src))
    shape = f"B {B} T {T} {H}x{W} Cp {Cp} frames {frames}"
    nan = lambda t: torch.full_like(t, float("nan"))      # noqa: E731
    out = []

    def done(name, dev, ref):
        k = ops.last_kernel()
        torch.cuda.synchronize()
        assert k == f"{name}<{_tn(dtype)}>", k
        b = Bound(k, shape)
        b.exact("out", dev.cpu(), _rounded(ref, dtype))
        b.exact_zero("padding", dev[..., C:])
        out.append(b)

    d = nan(e)
    ops.frame_absdiff(y, d, B, T, HW, Cp, t_pre, t_post, dt)
    done("frame_absdiff_kernel", d, E.frame_absdiff(yc, t_pre, t_post))
    assert bool((d == 0).any()) and bool((d > 0).any())
    o = nan(y)
    ops.enhance_apply(y, e, o, B, T, HW, Cp, t_mid, dt)
    done("enhance_apply_kernel", o, E.enhance_apply(yc, ec, t_mid))
    de = nan(e)
    ops.enhance_bwd_mask(dout, e, de, B, T, HW, Cp, t_mid, dt)
    done("enhance_bwd_mask_kernel", de, E.enhance_bwd_mask(doc, ec, t_mid))
    dy = nan(y)
    ops.enhance_bwd_apply(dout, y, dd, dy, B, T, HW, Cp, *(bwd_apply_frames or (t_pre, t_post)), dt)
    done("enhance_bwd_apply_kernel", dy, E.enhance_bwd_apply(doc, yc, ddc, t_pre, t_post))
    dy = nan(y)
    ops.enhance_bwd_apply(dout, y, dd, dy, B, T, HW, Cp, -1, T, dt)      # no frame matches: dy == dout
    done("enhance_bwd_apply_kernel", dy, doc)
    for acc in (0, 1):
        dst = dout.clone()
        ops.frame_scatter(src, dst, B, T, HW, Cp, t_mid, acc, dt)
        done("frame_scatter_kernel", dst, E.frame_scatter(srcc, doc, t_mid, acc))
    return out


ENHANCE_FRAMES = [(3, (0, 2, 1)), (4, (0, 3, 2)), (5, (0, 4, 2)), (5, (3, 1, 0))]


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f32"])
@pytest.mark.parametrize("C", [24, 54])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("T,frames", ENHANCE_FRAMES)
def test_enhance_pieces_equal_the_ieee_operation(T, frames, B, C, dtype):
    _need_gpu()
    bounds = run_enhance(dtype, T, B, C, frames)
    for b in bounds:
        b.check()


def test_enhance_pieces_where_the_grid_wraps():
    """Cp = 256, B = 3, T = 3, 112 x 112: 1.2 M vectors per frame set, more than 4096 workgroups of 256"""
    _need_gpu()
    if os.environ.get("C3D_BOF_GRID") or os.environ.get("C3D_BOB_GRID"):
        pytest.skip("walk case: the shapes assume the default grid caps (C3D_BOB_GRID / C3D_BOF_GRID is set)")
    assert 3 * 112 * 112 * 32 > E.FWD_GRID_CAP * 256
    for b in run_enhance(BF, 3, 3, 256, (0, 2, 1), H=112, W=112):
        b.check()


def test_swapped_frames_in_enhance_bwd_apply_change_nothing():
    """t_pre and t_post swapped: dy[:, t_post] = dout + sign(y_post - y_pre) dd = dout - sign(y_pre - y_post) dd, the value the
    unswapped call stores there -- |p - q| is symmetric, so is its gradient, and a correct kernel gives the SAME dy bit for
    bit (this launch cannot serve as a negative control; the next test is this family's)."""
    _need_gpu()
    for dtype in DTYPES:
        for b in run_enhance(dtype, 5, 3, 54, (0, 4, 2), bwd_apply_frames=(4, 0)):
            b.check(record=False)


def test_control_a_wrong_frame_in_enhance_bwd_apply():
    _need_gpu()
    bounds = run_enhance(BF, 4, 1, 24, (0, 3, 2), bwd_apply_frames=(0, 1))
    bad = [b for b in bounds if b.worst() > 1.0]
    assert len(bad) == 1 and bad[0].kernel.startswith("enhance_bwd_apply_kernel")
    _control("t_post one frame off in enhance_bwd_apply -> dy", bad[0])


def test_enhance_bwd_apply_refuses_one_frame_index_out_of_range():
    """on a matching frame the kernel reads y on BOTH frames: one index in range with the other outside is refused (no launch)"""
    _need_gpu()
    from change3d_amd import _lib, ops
    x = torch.zeros(1, 3, 16, 24, device=DEV)
    dd = torch.zeros(1, 16, 24, device=DEV)
    for t_pre, t_post in ((0, 3), (-1, 2)):
        with pytest.raises(_lib.Change3DHipError):
            ops.enhance_bwd_apply(x, x, dd, torch.empty_like(x), 1, 3, 16, 24, t_pre, t_post, ops.DT_F32)


# ================================================================================================ report
def test_zz_report_worst_error_over_bound():
    """(named to run last in this file) one ELEMWISE line per kernel and output, then the negative controls"""
    if not WORST:
        pytest.skip("no case ran")
    print(f"\nELEMWISE n_max {N_MAX}  eps_sums 2^{int(torch.log2(torch.tensor(EPS_SUMS)))}")
    for (kernel, what), v in sorted(WORST.items()):
        print(f"ELEMWISE worst {kernel} | {what}: {v:.3f}")
        assert v <= 1.0
    for name, v in CONTROLS.items():
        print(f"ELEMWISE control {name}: {v:.3g}")
        assert v > 1.0
