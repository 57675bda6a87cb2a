"""The folded-BatchNorm inference forward of a residual stage (c3d_stage_fold_bn + c3d_stage_fwd_folded, csrc/stage_driver.hip
"eval" section) against float64, element by element, in both storage types.

Every inference feature goes through this launch sequence, which shares no step with the training forward: fold_bn_kernel,
c3d_pw_gemm on folded f32 weights without weight images, c3d_dw333_fwd with a (1, shift) operand map, c3d_bn_se_finalize in
training = 2, conv_c on a shift-only ss_b, the three shortcut modes of c3d_block_out_fwd, all over a ring workspace.  The tests
call ops.stage_fold_sizes / stage_fold_bn / stage_fwd_folded directly on a StageBinding (the sequence of _StageFn.forward), so
they own fold, ws and y; y is pre-filled with NaN.  The reference is tests/folded_reference.py (pinned by
tests/test_folded_reference_cpu.py, which also shows that its bound holds for a correct implementation); parameters and
running statistics are drawn explicitly (tests/folded_cases.py: running_var = 0 on one channel, negative gammas, one gamma 0).

How a case is judged.  EVERY element of the device's y must satisfy |device - v| <= rel (|v| + err) + err (rel = 2^-8 / 2^-24),
v and err from folded_reference.block on the block's input.  The SE gate is judged on its own: the device's f32 gate [B][Ci]
is a tensor of the workspace the test owns (the layout of make_fold_plan is restated in `ws_layout` and its total asserted
against c3d_stage_fold_bytes); it must lie within the reference's gate_err of the reference's gate, and conv_c is then restated on
the device's gate.  Without that split the gate's worst-case bound (a per-sample f32 sum and two FC layers, no cancellation
credited) would make up nearly all of the bound of y -- at the res2 form 6 % of the value instead of 0.4 % for bf16, 1.5 %
instead of 0.02 % for f32 (with the split: 0.4 - 3 % / 0.02 - 0.8 % over all forms, the 432-channel form at the upper end) --
and a chain's propagated bound grows about 200-fold per SE block.
Chains (depth 2, 3, 5 of 24 / 54 / 24, depth 3 of 96 / 432 / 192) are therefore judged block by block on what the device itself
stored: the ring keeps the outputs of the last two intermediate blocks (y0 / y1), so the last two blocks of every chain (only
those: blocks 0 to 2 of the depth-5 chain are held by the shorter chains' checks of the same block forms and ring slots) --
block 0 and 1 of depth 2, 1 and 2 of depth 3, 3 and 4 of depth 5: the last block writing y_out from an odd and from an even
index, both ping-pong directions, a / b / c / sc reused by blocks of different size, the per-SE-block nc_b regions -- get the
single-block check, and the end-to-end result is also compared with `stage`'s propagated bound.

Odd map sizes at the stride-2 forms.  The shortcut gather C3D_ROWS_STRIDE2 used to decode its rows over [H / 2][W / 2] where the
plan, the depthwise kernel and the modules have (H + 1) / 2 rows: at an odd extent it sampled wrong pixels and ran past the input.
The decode is fixed (five sites: csrc/pw_gemm_impl.h, pw_wide.hip, pw_wgrad.hip); (2, 3, 17, 32), (2, 3, 17, 31) and (2, 4, 17, 8)
run at the three narrow stride-2 forms and (2, 3, 17, 22) at the wide one, the depthwise rows and the gather against the
reference.  (2, 3, 17, 22) itself stays REFUSED at the narrow forms (C3D_E_UNSUPPORTED from c3d_stage_fold_bytes, before anything is
launched): their conv_c takes an SE gate only where T Ho Wo is a multiple of 16 (297 here; c3d_pw_gemm answered C3D_E_BADARG in
the middle of the pass).  test_rows_per_sample_off_16_is_refused holds the refusal.

Negative controls: a reference variant that restates a plausible defect must land outside the bound of at least one element
of a correct device result (FOLDED-NEG lines): the shift_a activation applied to the zero padding of H / W (border pixels only),
the gates of two samples swapped, one channel's gamma_a sign flipped before folding, the stride-2 shortcut sampled at
(2 ho + 1, 2 wo), the second block of a chain fed block 0's input instead of y0.

Which new test notices which defect of the driver (from the CPU-side tampers above and the code):
  relu(a + shift) applied before the padding is zeroed     test_bound_sees_a_plausible_defect[pad] (every single-block case fails)
  the per-sample index of the gate                         test_bound_sees_a_plausible_defect[gates], and the gate check of every SE case with B > 1
  the zero fill of the accumulator tail (nc_b)             test_workspace_hygiene: ws full of 0xFF bytes makes the per-sample sums NaN, a
                                                           reused ws doubles them -- the gate check fails"""
import time

import pytest
import torch

import folded_cases as FC
import folded_reference as FR

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BF, F32 = torch.bfloat16, torch.float32
DTYPES = [BF, F32]
REPORT = {}          # (case family, storage type) -> list of per-case (worst, median) error / bound
_NEG = {}            # device runs shared by the negative controls
CLOCK = {}


@pytest.fixture(scope="module", autouse=True)
def _module_state():
    """The file's clock starts with its first test (not at collection); the report and the shared device runs go with its last."""
    CLOCK["t0"] = time.time()
    yield
    REPORT.clear()
    _NEG.clear()


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")


def _tn(dtype):
    return "bf16" if dtype == BF else "f32"


def _cpad(c):
    return (c + 7) // 8 * 8


# ------------------------------------------------------------------------------------------------ the device side
def build(stage, blocks, dtype):
    from change3d_amd.model.x3d import X3DResStage
    net = X3DResStage(*stage, dtype)
    net.load_state_dict(FC.state_dict_of(blocks), strict=True)
    for b, m in zip(blocks, net.res_blocks):
        assert (b["se"] is not None) == bool(m.use_se) and (b["w_sc"] is None) == (m.branch1_conv is None) \
            and (b["bn_sc"] is None) == (m.branch1_norm is None)
        if b["se"] is not None:
            assert m.branch2.norm_b[1].block[0].weight.shape[0] == b["se"][0].shape[0]
    return net.to(DEV).eval()


def bind_for(net, shape, dtype):
    from change3d_amd import ops
    B, T, H, W = shape
    bn0 = net.res_blocks[0].branch2.norm_a
    assert float(bn0.eps) == FC.EPS
    bind = net.binding()
    bind.desc.flags = 0
    bind.refresh(B, T, H, W, ops.dt_code(dtype), False, float(bn0.momentum), float(bn0.eps), with_grads=False)
    return bind


def ws_layout(blocks, shape, dtype):
    """make_fold_plan (csrc/stage_plan.h) restated: byte offsets of a, b, c, sc, y0, y1, gate, hid, the total, and the output
    shape of every block.  One set of activations for all blocks, each region the largest any block asks for, 256-byte steps;
    then one per-sample-sum region per SE block."""
    B, T, H, W = shape
    es = 2 if dtype == BF else 4
    al = lambda v: (v + 255) // 256 * 256          # noqa: E731
    mx = dict(a=0, b=0, c=0, gate=0, hid=0)
    shapes, nc = [], 0
    for b in blocks:
        Ho, Wo = (H - 1) // b["stride"] + 1, (W - 1) // b["stride"] + 1
        cip, cop = _cpad(b["cinner"]), _cpad(b["cout"])
        mx["a"] = max(mx["a"], B * T * H * W * cip * es)
        mx["b"] = max(mx["b"], B * T * Ho * Wo * cip * es)
        mx["c"] = max(mx["c"], B * T * Ho * Wo * cop * es)
        mx["gate"] = max(mx["gate"], B * cip * 4)
        mx["hid"] = max(mx["hid"], B * max(b["se"][0].shape[0] if b["se"] is not None else 0, 1) * 4)
        if b["se"] is not None:
            nc += al(B * cip * 2 * 8)
        shapes.append((B, T, Ho, Wo, cop))
        H, W = Ho, Wo
    off, o = {}, 0
    for name, size in (("a", mx["a"]), ("b", mx["b"]), ("c", mx["c"]), ("sc", mx["c"]), ("y0", mx["c"]), ("y1", mx["c"]),
                       ("gate", mx["gate"]), ("hid", mx["hid"])):
        off[name] = o
        o += al(size)
    return off, o + nc, shapes


def run(net, blocks, x, dtype, ws=None, fold=None, fill_fold=False):
    """One eval forward through the C ABI.  x [B,T,H,W,cin] f32 (exact in the storage type).  Returns y (NaN pre-filled), ws,
    fold and the workspace layout."""
    from change3d_amd import ops
    shape = tuple(x.shape[:4])
    bind = bind_for(net, shape, dtype)
    _, _, y_bytes, _ = bind.sizes()
    fold_bytes, ws_bytes = ops.stage_fold_sizes(bind)
    off, total, shapes = ws_layout(blocks, shape, dtype)
    assert total == ws_bytes, (total, ws_bytes)
    if fold is None:
        fold = torch.full((fold_bytes,), 0xFF if fill_fold else 0, dtype=torch.uint8, device=DEV)
        ops.stage_fold_bn(bind, fold)
    if ws is None:
        ws = torch.zeros(ws_bytes, dtype=torch.uint8, device=DEV)
    assert ws.numel() >= ws_bytes and fold.numel() == fold_bytes
    y = torch.full(shapes[-1], float("nan"), dtype=dtype, device=DEV)
    assert y.numel() * y.element_size() == y_bytes
    xin = x.to(DEV, dtype).contiguous()
    assert xin.shape[-1] % 8 == 0
    ops.stage_fwd_folded(bind, fold, xin, ws, y)
    torch.cuda.synchronize()
    return dict(y=y, ws=ws, fold=fold, off=off, shapes=shapes, x=x)


def region(r, name, shape, dtype):
    n = 1
    for s in shape:
        n *= s
    n *= 4 if dtype == F32 else 2
    o = r["off"][name]
    return r["ws"][o:o + n].view(dtype).view(shape)


# ------------------------------------------------------------------------------------------------ the judgement
def judge_block(what, p, x_in, y_dev, gate_dev, dtype, tamper=None, record=None):
    """One block on the input the device stored.  x_in, y_dev: CPU float64 [B,T,H,W,C]; gate_dev: CPU float64 [B][Ci] or None.
    Returns (worst error / bound of y, median over the elements with an error, worst of the gate)."""
    bf16 = dtype == BF
    ref = FR.block(x_in, torch.zeros_like(x_in), p, FC.EPS, bf16, tamper=tamper, gate_given=gate_dev)
    rg = 0.0
    if p["se"] is not None:
        assert gate_dev is not None
        rg = float(FR.ratio(gate_dev, ref["gate"], ref["gate_err"]).max())
    assert tuple(y_dev.shape) == tuple(ref["v"].shape), (y_dev.shape, ref["v"].shape)
    r = FR.ratio(y_dev, ref["v"], ref["bound"])
    worst, med = float(r.max()), float(r[r > 0].median()) if bool((r > 0).any()) else 0.0
    print(f"\nFOLDED {what} {_tn(dtype)}: y error/bound worst {worst:.3f} median {med:.3f}, gate {rg:.3f}")
    if record is not None:
        REPORT.setdefault((record, _tn(dtype)), []).append((max(worst, rg), med))
    return worst, med, rg, r


def judge_stage(what, blocks, r, dtype, record=None, e2e=True):
    """The last two blocks of the stage, each on the input the device stored (x for block 0, else the other ring buffer), the
    gate of the one of them that has SE, and the end-to-end result against the propagated bound."""
    bd = FC.to_double(blocks)
    n = len(bd)
    d = lambda t: t.detach().double().cpu()          # noqa: E731
    ybuf = lambda i: r["y"] if i == n - 1 else region(r, "y0" if i % 2 == 0 else "y1", r["shapes"][i], dtype)   # noqa: E731
    x0 = r["x"].double()
    fails = []
    for i in range(max(0, n - 2), n):
        p = bd[i]
        gate = None
        if p["se"] is not None:          # the gate buffer holds the gate of the LAST SE block that ran: of i or of i + 1, never both
            assert i == n - 1 or bd[i + 1]["se"] is None
            B = x0.shape[0]
            gate = d(region(r, "gate", (B, _cpad(p["cinner"])), F32))
            assert bool((gate[:, p["cinner"]:] == 0).all()), "padding channels of the gate must be exact zeros"
            gate = gate[:, :p["cinner"]]
        x_in = x0 if i == 0 else d(ybuf(i - 1))
        worst, _, rg, _ = judge_block(f"{what} block {i}/{n}", p, x_in, d(ybuf(i)), gate, dtype, record=record)
        if not worst <= 1.0 or not rg <= 1.0:
            fails.append((i, worst, rg))
        if n == 1 and p["se"] is not None:
            # and against the reference's OWN gate, as one piece: the wider bound, the gate's worst-case error included
            own = FR.block(x_in, torch.zeros_like(x_in), p, FC.EPS, dtype == BF)
            w = float(FR.ratio(d(ybuf(i)), own["v"], own["bound"]).max())
            print(f"FOLDED {what} {_tn(dtype)}: on the reference's own gate {w:.3f}")
            if not w <= 1.0:
                fails.append(("own gate", w))
    if e2e and n > 1:
        ref = FR.stage(x0, bd, FC.EPS, dtype == BF)
        w = float(FR.ratio(d(r["y"]), ref["v"], ref["bound"]).max())
        print(f"FOLDED {what} {_tn(dtype)}: end to end against the propagated bound {w:.3g}")
        if not w <= 1.0:
            fails.append(("end to end", w))
    assert not fails, f"bound exceeded: {what} {_tn(dtype)}: {fails}"


def _case(stage, shape, dtype, seed=21):
    blocks = FC.draw_blocks(stage, seed)
    x = FC.draw_input(shape, stage[1], dtype == BF, seed + 1)
    return blocks, x


# ================================================================================================ every block form, depth 1
@pytest.mark.parametrize("dtype", DTYPES, ids=_tn)
@pytest.mark.parametrize("form,shape", FC.SINGLE, ids=[f"{f}-{'x'.join(map(str, s))}" for f, s in FC.SINGLE])
def test_block_form(form, shape, dtype):
    _need_gpu()
    stage = FC.FORMS[form]
    blocks, x = _case(stage, shape, dtype)
    net = build(stage, blocks, dtype)
    judge_stage(f"{form} {shape}", blocks, run(net, blocks, x, dtype), dtype, record=form)


@pytest.mark.parametrize("dtype", DTYPES, ids=_tn)
@pytest.mark.parametrize("form", [f for f, s in FC.FORMS.items() if s[4] == 2 and s[2] <= 224])
def test_rows_per_sample_off_16_is_refused(form, dtype):
    """(2, 3, 17, 22) at the narrow stride-2 forms: the training plan takes it (Ho = 9, Wo = 11), the eval plan refuses it before
    anything is launched -- T Ho Wo = 297 is no multiple of 16, the narrow conv_c cannot take its SE gate.  (The wide form runs
    this shape, the narrow forms run the odd shapes of folded_cases.ODD_NARROW: test_block_form.)"""
    _need_gpu()
    from change3d_amd import ops
    from change3d_amd import _lib as L
    stage = FC.FORMS[form]
    blocks, x = _case(stage, FC.ODD_SHAPE, dtype)
    net = build(stage, blocks, dtype)
    bind = bind_for(net, FC.ODD_SHAPE, dtype)
    B, T, H, W = FC.ODD_SHAPE
    assert bind.sizes()[2] == B * T * 9 * 11 * stage[3] * (2 if dtype == BF else 4)
    a, b = ops.C.c_int64(-1), ops.C.c_int64(-1)
    assert L.lib().c3d_stage_fold_bytes(ops.C.byref(bind.desc), ops.C.byref(a), ops.C.byref(b)) == -2          # C3D_E_UNSUPPORTED
    assert a.value == -1 and b.value == -1
    with pytest.raises(L.Change3DHipError, match="does not take the stage geometry"):
        ops.stage_fold_sizes(bind)
    with pytest.raises(L.Change3DHipError, match="does not take the stage geometry"), torch.no_grad():
        net(x.permute(0, 4, 1, 2, 3).to(DEV))
    # an even size with T Ho Wo a multiple of 16 right after it: the binding is not left in a refusing state
    blocks2, x2 = blocks, FC.draw_input((2, 3, 8, 8), stage[1], dtype == BF, 5)
    judge_stage(f"{form} after the refusal", blocks2, run(net, blocks2, x2, dtype), dtype)


# ================================================================================================ chains
@pytest.mark.parametrize("dtype", DTYPES, ids=_tn)
@pytest.mark.parametrize("name", list(FC.CHAINS))
def test_chain(name, dtype):
    _need_gpu()
    stage, shape = FC.CHAINS[name]
    blocks, x = _case(stage, shape, dtype)
    net = build(stage, blocks, dtype)
    judge_stage(f"{name} {shape}", blocks, run(net, blocks, x, dtype), dtype, record=name)


# ================================================================================================ buffer hygiene
@pytest.mark.parametrize("dtype", DTYPES, ids=_tn)
def test_workspace_hygiene(dtype):
    """Depth 3, inner width 54 (56 padded channels).  (a) ws full of 0xFF bytes, (b) fold full of 0xFF bytes before
    c3d_stage_fold_bn, (c) the same ws for a second call on another input and for a call with a smaller batch: every run passes
    the parity check of the clean run -- nothing is read before it is written, the accumulators are zeroed per call, the padding
    channels of ss_* are defined."""
    _need_gpu()
    from change3d_amd import ops
    stage, shape = FC.HYGIENE
    blocks, x = _case(stage, shape, dtype, seed=31)
    net = build(stage, blocks, dtype)
    clean = run(net, blocks, x, dtype)
    judge_stage("hygiene clean", blocks, clean, dtype, record="hygiene")
    ws_bytes = ops.stage_fold_sizes(bind_for(net, shape, dtype))[1]
    dirty = torch.full((ws_bytes,), 0xFF, dtype=torch.uint8, device=DEV)
    a = run(net, blocks, x, dtype, ws=dirty)
    judge_stage("hygiene (a) ws = 0xFF", blocks, a, dtype, record="hygiene")
    b = run(net, blocks, x, dtype, fill_fold=True)
    judge_stage("hygiene (b) fold = 0xFF", blocks, b, dtype, record="hygiene")
    x2 = FC.draw_input(shape, stage[1], dtype == BF, 77) * 1.5
    x2 = x2.bfloat16().float() if dtype == BF else x2
    c = run(net, blocks, x2, dtype, ws=a["ws"], fold=a["fold"])
    judge_stage("hygiene (c) ws reused, other input", blocks, c, dtype, record="hygiene")
    x3 = x2[:2].contiguous()
    c2 = run(net, blocks, x3, dtype, ws=a["ws"], fold=a["fold"])
    judge_stage("hygiene (c) ws reused, smaller batch", blocks, c2, dtype, record="hygiene")


# ================================================================================================ cache rules of X3DResStage
CACHE_STAGE, CACHE_SHAPE = FC.FORMS["s2-raw-se-24"], (2, 3, 16, 16)


def _module_eval(net, x, dtype):
    with torch.no_grad():
        y = net(x.permute(0, 4, 1, 2, 3).to(DEV))
    torch.cuda.synchronize()
    return y.permute(0, 2, 3, 4, 1).contiguous()


def _judge_module(what, net, x, y, dtype, expect_inside=True):
    """Through the module there is no workspace to read the gate from: the reference's own gate, and with it the wider bound."""
    blocks = FC.to_double(FC.blocks_of(net.state_dict(), CACHE_STAGE))
    return _judge_with(what, blocks, x, y, dtype, expect_inside)


def _judge_with(what, blocks, x, y, dtype, expect_inside=True):
    ref = FR.stage(x.double(), blocks, FC.EPS, dtype == BF)
    w = float(FR.ratio(y.double().cpu(), ref["v"], ref["bound"]).max())
    print(f"\nFOLDED cache {what} {_tn(dtype)}: error/bound {w:.3g}")
    assert (w <= 1.0) == expect_inside, (what, w)
    return w


@pytest.mark.parametrize("dtype", DTYPES, ids=_tn)
def test_folded_copy_follows_an_optimizer_step(dtype):
    _need_gpu()
    from change3d_amd.model.utils import FusedAdam, ParamArena
    blocks, x = _case(CACHE_STAGE, CACHE_SHAPE, dtype, seed=41)
    net = build(CACHE_STAGE, blocks, dtype)
    arena = ParamArena(list(net.named_parameters()), DEV)
    opt = FusedAdam(arena, lr=0.05, weight_decay=0.0)
    y0 = _module_eval(net, x, dtype)
    _judge_module("before the step", net, x, y0, dtype)
    old = FC.to_double(FC.blocks_of(net.state_dict(), CACHE_STAGE))
    net.train()
    for _ in range(2):
        opt.zero_grad()
        out = net(x.permute(0, 4, 1, 2, 3).to(DEV).requires_grad_(True))
        out.float().square().mean().backward()
        opt.step()
    torch.cuda.synchronize()
    net.eval()
    y1 = _module_eval(net, x, dtype)
    _judge_module("after two FusedAdam steps", net, x, y1, dtype)
    # the step was large enough to matter: the same output is far outside the bound of the OLD parameters and statistics
    _judge_with("after the steps, against the old parameters", old, x, y1, dtype, expect_inside=False)


@pytest.mark.parametrize("dtype", DTYPES, ids=_tn)
def test_folded_copy_and_a_hand_edit_of_running_var(dtype):
    _need_gpu()
    blocks, x = _case(CACHE_STAGE, CACHE_SHAPE, dtype, seed=43)
    net = build(CACHE_STAGE, blocks, dtype)
    y0 = _module_eval(net, x, dtype)
    _judge_module("before the edit", net, x, y0, dtype)
    with torch.no_grad():
        net.res_blocks[0].branch2.norm_a.running_var.mul_(4.0).add_(0.5)
    y_stale = _module_eval(net, x, dtype)
    assert torch.equal(y_stale, y0), "without invalidate_folded_bn() the folded copy is the stale one, bit for bit"
    _judge_module("stale copy against the new statistics", net, x, y_stale, dtype, expect_inside=False)
    net.invalidate_folded_bn()
    y1 = _module_eval(net, x, dtype)
    _judge_module("after invalidate_folded_bn()", net, x, y1, dtype)


# ================================================================================================ negative controls
def _neg_run(which, dtype):
    key = (which, dtype)
    if key not in _NEG:
        stage, shape = (FC.CHAINS["chain-2"]) if which == "chain" else (FC.FORMS["s2-raw-se-24"], (3, 3, 16, 24))
        blocks, x = _case(stage, shape, dtype, seed=51)
        net = build(stage, blocks, dtype)
        _NEG[key] = (blocks, run(net, blocks, x, dtype))
    return _NEG[key]


def _flip_gamma(p):
    q = dict(p)
    g, b, m, v = p["bn_a"]
    g = g.clone()
    c = int(torch.argmax(g.abs() * (v > 0.5)))
    g[c] = -g[c]
    q["bn_a"] = (g, b, m, v)
    return q


@pytest.mark.parametrize("dtype", DTYPES, ids=_tn)
@pytest.mark.parametrize("control", ["pad", "gates", "gamma", "shortcut", "stale"])
def test_bound_sees_a_plausible_defect(control, dtype):
    _need_gpu()
    d = lambda t: t.detach().double().cpu()          # noqa: E731
    blocks, r = _neg_run("chain" if control == "stale" else "single", dtype)
    bd = FC.to_double(blocks)
    x0 = r["x"].double()
    B = x0.shape[0]
    if control == "stale":
        # block 1 of the depth-2 chain (no SE) fed block 0's input, sampled at block 0's stride, instead of y0
        y0 = d(region(r, "y0", r["shapes"][0], dtype))
        ok = judge_block("control: chain block 1 on y0", bd[1], y0, d(r["y"]), None, dtype)[0]
        bad = judge_block("control: chain block 1 on block 0's input", bd[1], x0[:, :, ::2, ::2].contiguous(), d(r["y"]), None, dtype)[0]
    else:
        p = bd[0]
        gate = d(region(r, "gate", (B, _cpad(p["cinner"])), F32))[:, :p["cinner"]]
        ok, _, rg, _ = judge_block("control: the correct reference", p, x0, d(r["y"]), gate, dtype)
        assert rg <= 1.0
        tamper = {"pad": dict(pad_bug=True), "gates": dict(swap_gates=(0, 1)), "shortcut": dict(sc_offset=1), "gamma": None}[control]
        bad, _, _, ratios = judge_block(f"control: {control}", _flip_gamma(p) if control == "gamma" else p, x0, d(r["y"]), gate, dtype,
                                        tamper=tamper)
        if control == "pad":
            assert float(ratios[:, :, 1:-1, 1:-1].max()) <= 1.0, "the padding defect shows at border pixels only"
        if control == "gates":
            assert float(ratios[2].max()) <= 1.0, "the third sample keeps its gate"
    print(f"FOLDED-NEG {control} {_tn(dtype)}: correct reference {ok:.3f}, defect {bad:.3g}")
    REPORT.setdefault(("neg-" + control, _tn(dtype)), []).append((bad, ok))
    assert ok <= 1.0 < bad


def test_zz_report_worst_ratio_per_form():
    """Worst and median error / bound per case family and storage type (run with -s), and the wall time of this file."""
    _need_gpu()
    print()
    for (fam, tn), rows in sorted(REPORT.items()):
        if fam.startswith("neg-"):
            print(f"FOLDED-WORST {fam:16s} {tn:5s} defect at {max(b for b, _ in rows):.3g} x the bound (correct reference {max(o for _, o in rows):.3f})")
        else:
            ws, ms = [w for w, _ in rows], sorted(m for _, m in rows)
            print(f"FOLDED-WORST {fam:16s} {tn:5s} worst {max(ws):.3f}  median {ms[len(ms) // 2]:.3f}  ({len(rows)} block checks)")
    print(f"FOLDED-WORST wall time of the file {time.time() - CLOCK['t0']:.1f} s")
    assert all(w <= 1.0 for (fam, _), rows in REPORT.items() if not fam.startswith("neg-") for w, _ in rows)
