"""Pins tests/folded_reference.py, the float64 restatement of the folded-BatchNorm inference forward.

1. With the rounding steps switched off, `stage` agrees with a float64 eval() evaluation of the same modules (the oracle's
   ResStage / ResBlock under .double().eval()) to 1e-12 of the largest output: every block form, T = 3, 4 and 5, odd map
   sizes at stride 1 and 2, and a chain of three blocks.  `fold` is pinned against gamma / sqrt(var + eps) in float64.
2. The bound must hold for a correct implementation before it is used to judge one.  For every case the GPU file runs, in
   both storage types:
     f32 storage   the UNROUNDED float64 result lies inside the bound of the rounded reference (the rounding steps of f32
                   storage are below the arithmetic allowances of every kernel);
     bf16 storage  the unrounded result lies inside the bound once the rounding steps themselves are budgeted (`widen=True`:
                   the same propagation code with err + ulp at every rounding point) -- the tight bound cannot contain it,
                   the storage roundings alone are 2^-8 of every stored tensor;
     both          a second evaluation in other arithmetic -- folded_reference.block itself run on float32 tensors (f32 products,
                   torch's summation orders, f32 sqrt / exp; it shares every structural choice with the reference, so it
                   tests the error allowances and the near-boundary marks, not the structure, which part 1 pins) -- judged exactly as the GPU file
                   judges the device: block by block on the input it stored itself, its gate within gate_err of the reference's, conv_c restated on its
                   gate.  Every element lies inside the tight bound, and its stored tensors differ from the reference's only
                   where the reference says they may (slack > 0, else bit-equal).
3. The eval plan's refusal of T Ho Wo % 16 != 0 at the narrow SE forms, and its acceptance of odd extents, on the host
   (c3d_stage_fold_bytes launches nothing)."""
import pytest
import torch

import folded_cases as FC
import folded_reference as FR


def _oracle(stage):
    from oracle import model as om, pv
    depth, cin, cinner, cout, stride, ratio = stage
    if ratio > 0:
        return om.build_stage(depth, cin, cinner, cout, (1, stride, stride))
    assert depth == 1
    return pv.ResStage(res_blocks=torch.nn.ModuleList([om.build_res_block(cin, cinner, cout, (1, stride, stride), use_se=False)]))


def _module_eval(stage, blocks, x):
    m = _oracle(stage)
    m.load_state_dict(FC.state_dict_of(blocks), strict=True)
    m = m.double().eval()
    with torch.no_grad():
        return m(x.double().permute(0, 4, 1, 2, 3)).permute(0, 2, 3, 4, 1)


PIN = [(f, (2, T, 8, 8)) for f in FC.FORMS for T in (3, 4, 5)] + [("id-se-24", (2, 3, 9, 11)), ("id-24", (1, 4, 7, 13)),
                                                                      ("s2-raw-se-24", (2, 3, 17, 11)), ("s2-bn-se-48", (1, 4, 9, 7)),
                                                                      ("s2-bn-se-192w", (1, 5, 7, 9))]


@pytest.mark.parametrize("form,shape", PIN)
def test_unrounded_stage_is_the_float64_eval_of_the_modules(form, shape):
    stage = FC.FORMS[form]
    blocks = FC.draw_blocks(stage, 11)
    x = FC.draw_input(shape, stage[1], False, 12)
    ref = _module_eval(stage, blocks, x)
    out = FR.stage(x.double(), FC.to_double(blocks), FC.EPS, False, rounded=False)
    assert out["v"].shape == ref.shape
    assert float((out["v"] - ref).abs().max()) <= 1e-12 * max(1.0, float(ref.abs().max()))
    assert float(out["err"].max()) == 0.0          # nothing is charged when nothing is rounded


@pytest.mark.parametrize("name", ["chain-3", "chain-3w"])
def test_unrounded_chain_is_the_float64_eval_of_the_modules(name):
    stage, shape = FC.CHAINS[name]
    blocks = FC.draw_blocks(stage, 13)
    x = FC.draw_input(shape, stage[1], False, 14)
    ref = _module_eval(stage, blocks, x)
    out = FR.stage(x.double(), FC.to_double(blocks), FC.EPS, False, rounded=False)
    assert float((out["v"] - ref).abs().max()) <= 1e-12 * max(1.0, float(ref.abs().max()))


def test_fold_is_gamma_over_sqrt_var_plus_eps():
    g = torch.Generator().manual_seed(5)
    w = torch.randn(54, 24, generator=g, dtype=torch.float32).double()
    gamma, beta, mean, var = (t.double() for t in FC._bn(54, g))
    exact = FR.fold(w, gamma, beta, mean, var, FC.EPS, rounded=False)
    sc = gamma / torch.sqrt(var + FC.EPS)
    assert torch.equal(exact["scale"], sc) and torch.equal(exact["w"], w * sc[:, None]) and torch.equal(exact["shift"], beta - mean * sc)
    f = FR.fold(w, gamma, beta, mean, var, FC.EPS)
    # the f32 fold: f32 values, within its own error bound (+ one f32 rounding, + eps as an f32 value) of the exact one
    for k in ("w", "shift", "scale"):
        assert torch.equal(f[k], f[k].float().double()), k
    eps_term = 2.0 ** -24 * FC.EPS / (var + FC.EPS)          # d rstd / rstd for eps -> (float) eps
    assert bool(((f["w"] - exact["w"]).abs() <= f["w_err"] + (2.0 ** -24 + eps_term)[:, None] * exact["w"].abs()).all())
    assert bool(((f["shift"] - exact["shift"]).abs() <= f["shift_err"] + 2.0 ** -24 * exact["shift"].abs()
                 + eps_term * (mean * sc).abs()).all())
    assert float(f["scale"][1]) == 0.0 and float(f["w"][1].abs().max()) == 0.0          # gamma = 0
    assert abs(float(f["scale"][2]) + 2.0 ** -7 / FC.EPS ** 0.5) < 1e-4                # running_var = 0: rstd = eps^-1/2


def _f32(blocks):
    return [{k: (tuple(t.float() for t in v) if isinstance(v, tuple) else v.float() if torch.is_tensor(v) else v) for k, v in b.items()}
            for b in blocks]


def _other_implementation_blockwise(x, blocks, bf16):
    """The blocks evaluated in f32 arithmetic, one by one; the float64 reference judges each on the input (and, as the GPU file
    does, on the gate) the other implementation stored."""
    cur, worst = x.float(), 0.0
    for p, p32 in zip(FC.to_double(blocks), _f32(blocks)):
        o = FR.block(cur, torch.zeros_like(cur), p32, FC.EPS, bf16)
        cd = cur.double()
        ref = FR.block(cd, torch.zeros_like(cd), p, FC.EPS, bf16, gate_given=None if o["gate"] is None else o["gate"].double())
        if o["gate"] is not None:
            assert float(FR.ratio(o["gate"].double(), ref["gate"], ref["gate_err"]).max()) <= 1.0
        assert float(FR.ratio(o["v"].double(), ref["v"], ref["bound"]).max()) <= 1.0
        assert float(FR.ratio(o["y"].double(), ref["y"], ref["slack"]).max()) <= 1.0
        worst = max(worst, float((ref["bound"] / ref["v"])[ref["v"] > 0.1 * ref["v"].max()].median()))
        cur = o["y"]
    return worst


GPU_CASES = [(f, FC.FORMS[f], s) for f, s in FC.SINGLE] + [(n, st, sh) for n, (st, sh) in FC.CHAINS.items()]


@pytest.mark.parametrize("bf16", [True, False], ids=["bf16", "f32"])
@pytest.mark.parametrize("name,stage,shape", GPU_CASES, ids=[f"{n}-{'x'.join(map(str, s))}" for n, _, s in GPU_CASES])
def test_reference_stays_inside_its_own_bound(name, stage, shape, bf16):
    blocks = FC.draw_blocks(stage, 21)
    x = FC.draw_input(shape, stage[1], bf16, 22)
    bd, xd = FC.to_double(blocks), x.double()
    ref = FR.stage(xd, bd, FC.EPS, bf16)
    exact = FR.stage(xd, bd, FC.EPS, bf16, rounded=False)["v"]
    assert bool(torch.isfinite(ref["bound"]).all()) and float(ref["v"].abs().max()) > 0
    if bf16:
        wide = FR.stage(xd, bd, FC.EPS, bf16, widen=True)
        assert float(FR.ratio(exact, wide["v"], wide["bound"]).max()) <= 1.0
        assert bool((wide["bound"] >= ref["bound"]).all())
    else:
        assert float(FR.ratio(exact, ref["v"], ref["bound"]).max()) <= 1.0
    rel = _other_implementation_blockwise(x, blocks, bf16)
    print(f"\nFOLDED-REF {name} {shape} {'bf16' if bf16 else 'f32'}: median bound / value of a block on a given gate {rel:.2e}")


@pytest.mark.parametrize("form", [f for f, s in FC.FORMS.items() if s[4] == 2])
def test_eval_plan_refuses_rows_per_sample_off_16(form):
    """Host only (c3d_stage_fold_bytes launches nothing): the training plan takes every shape; the eval plan answers
    C3D_E_UNSUPPORTED where a narrow SE block has T Ho Wo % 16 != 0 (297, 264 rows per sample) and takes odd extents otherwise."""
    from change3d_amd import ops, _lib as L
    from change3d_amd.model.x3d import X3DResStage
    stage = FC.FORMS[form]
    wide = stage[2] > 224
    net = X3DResStage(*stage, torch.float32).eval()
    bind = net.binding()
    for shape, ok in ((FC.ODD_SHAPE, wide), ((2, 3, 16, 22), wide), ((2, 3, 16, 24), True), ((2, 3, 17, 31), True), ((2, 4, 17, 8), True)):
        bind.refresh(*shape, ops.DT_F32, False, 0.1, FC.EPS, with_grads=False)
        assert bind.sizes()[2] > 0
        if ok:
            assert ops.stage_fold_sizes(bind)[1] > 0
        else:
            with pytest.raises(L.Change3DHipError, match="does not take the stage geometry"):
                ops.stage_fold_sizes(bind)
