"""Cases of the folded-BatchNorm inference parity tests: block forms, shapes, and explicitly drawn parameters and inputs,
shared by tests/test_folded_reference_cpu.py (which checks the reference's own bound on every GPU case) and
tests/test_folded_parity_gpu.py.  Plain torch; nothing imported from the package.

A stage is (depth, cin, cinner, cout, stride, se_ratio), built the way X3DResStage builds it: block 0 takes cin and the stride,
the others cout and stride 1; blocks 0, 2, 4 have SqueezeExcitation when se_ratio > 0; a block has a shortcut convolution when
its channel count changes or it strides, and a shortcut BatchNorm when its channel count changes."""
import torch

EPS = 1e-5          # every BatchNorm of a stage (model/x3d.py BN_EPS and nn.BatchNorm3d's default)

# every block form as a depth-1 stage
FORMS = {
    "s2-raw-se-24": (1, 24, 54, 24, 2, 0.0625),        # stride 2, shortcut convolution WITHOUT BatchNorm (res2 block 0)
    "s2-bn-se-48": (1, 24, 108, 48, 2, 0.0625),        # stride 2, shortcut convolution + BatchNorm
    "s2-bn-se-96": (1, 48, 216, 96, 2, 0.0625),
    "s2-bn-se-192w": (1, 96, 432, 192, 2, 0.0625),     # the same on the wide kernels
    "id-se-24": (1, 24, 54, 24, 1, 0.0625),            # identity shortcut
    "id-se-96": (1, 96, 216, 96, 1, 0.0625),
    "id-24": (1, 24, 54, 24, 1, 0.0),                  # identity shortcut, no SE
    "id-96": (1, 96, 216, 96, 1, 0.0),
}
SHAPES = [(3, 3, 16, 24), (2, 4, 16, 16), (1, 5, 8, 8), (5, 3, 8, 8)]      # (B, T, H, W)
WIDE_SHAPES = [(2, 4, 8, 8), (1, 5, 8, 8), (5, 3, 8, 8)]                    # the 432-channel form needs no more than 8 x 8
ODD_SHAPE = (2, 3, 17, 22)          # odd height at the stride-2 forms: Ho = 9, Wo = 11.  T Ho Wo = 297 is no multiple of 16: the
#                                     narrow forms' conv_c cannot take its SE gate (refused by the eval plan); the wide form runs it
ODD_NARROW = [(2, 3, 17, 32), (2, 3, 17, 31), (2, 4, 17, 8)]      # odd extents the narrow forms take: 432, 432, 144 rows per sample
SINGLE = [(f, s) for f in FORMS for s in (WIDE_SHAPES if f.endswith("w") else SHAPES)] \
    + [(f, s) for f, st in FORMS.items() if st[4] == 2 for s in ([ODD_SHAPE] if f.endswith("w") else ODD_NARROW)]

CHAINS = {
    "chain-2": ((2, 24, 54, 24, 2, 0.0625), (3, 3, 16, 24)),
    "chain-3": ((3, 24, 54, 24, 2, 0.0625), (3, 3, 16, 24)),
    "chain-5": ((5, 24, 54, 24, 2, 0.0625), (2, 3, 16, 16)),
    "chain-3w": ((3, 96, 432, 192, 2, 0.0625), (2, 3, 8, 8)),
}
HYGIENE = ((3, 24, 54, 24, 2, 0.0625), (3, 3, 16, 24))     # inner width 54 -> 56 padded channels


def se_width(cinner, ratio):
    """pytorchvideo's round_width(cinner, ratio) (min width 8, divisor 8)."""
    w = cinner * ratio
    out = max(8, int(w + 4) // 8 * 8)
    return out + 8 if out < 0.9 * w else out


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _bn(n, g):
    """(gamma, beta, running_mean, running_var), f32: mean within +-1, var in [0.05, 4]; channel 2 has var = 0 (rstd = 316: its
    gamma is small, so that a chain of such layers stays in range), gamma is negative on about a quarter of the channels and
    exactly 0 on channel 1."""
    r = lambda: torch.randn(n, generator=g, dtype=torch.float32)                                  # noqa: E731
    u = lambda: torch.rand(n, generator=g, dtype=torch.float32)                                   # noqa: E731
    gamma = (r().abs() + 0.5) * torch.where(u() < 0.25, -1.0, 1.0)
    beta, mean, var = r() * 0.3, u() * 2 - 1, 0.05 + 3.95 * u()
    gamma[1], gamma[2], var[2] = 0.0, -2.0 ** -7, 0.0
    return gamma, beta, mean, var


def draw_blocks(stage, seed):
    """The blocks of a stage as tests/folded_reference.py takes them, every tensor f32."""
    depth, cin, cinner, cout, stride, ratio = stage
    g = _gen(seed)
    w = lambda n, k: torch.randn(n, k, generator=g, dtype=torch.float32) / k ** 0.5              # noqa: E731
    blocks = []
    for i in range(depth):
        ci, s = (cin, stride) if i == 0 else (cout, 1)
        conv, se = ci != cout or s > 1, bool((i + 1) % 2) and ratio > 0
        b = dict(cin=ci, cinner=cinner, cout=cout, stride=s, w_a=w(cinner, ci), w_b=w(cinner, 27) * 2, w_c=w(cout, cinner),
                 w_sc=w(cout, ci) if conv else None, bn_a=_bn(cinner, g), bn_b=_bn(cinner, g), bn_c=_bn(cout, g),
                 bn_sc=_bn(cout, g) if ci != cout else None, se=None)
        if se:
            cr = se_width(cinner, ratio)
            b["se"] = (w(cr, cinner) * 2, torch.randn(cr, generator=g) * 0.3, w(cinner, cr), torch.randn(cinner, generator=g) * 0.3)
        blocks.append(b)
    return blocks


def draw_input(shape, cin, bf16, seed):
    """[B,T,H,W,cin] f32 values that are exact in the storage type."""
    B, T, H, W = shape
    x = torch.randn(B, T, H, W, cin, generator=_gen(seed), dtype=torch.float32)
    return x.bfloat16().float() if bf16 else x


def to_double(blocks):
    cv = lambda v: None if v is None else tuple(t.double() for t in v) if isinstance(v, tuple) else v.double() if torch.is_tensor(v) else v  # noqa: E731
    return [{k: cv(v) for k, v in b.items()} for b in blocks]


_BN_KEYS = ("weight", "bias", "running_mean", "running_var")


def state_dict_of(blocks):
    """The blocks as the state dict of an oracle ResStage / an X3DResStage (the two share their keys)."""
    sd = {}
    for i, b in enumerate(blocks):
        p = f"res_blocks.{i}."
        sd[p + "branch2.conv_a.weight"] = b["w_a"].reshape(b["cinner"], b["cin"], 1, 1, 1)
        sd[p + "branch2.conv_b.weight"] = b["w_b"].reshape(b["cinner"], 1, 3, 3, 3)
        sd[p + "branch2.conv_c.weight"] = b["w_c"].reshape(b["cout"], b["cinner"], 1, 1, 1)
        norms = [("branch2.norm_a.", b["bn_a"]), ("branch2.norm_b.0.", b["bn_b"]), ("branch2.norm_c.", b["bn_c"])]
        if b["w_sc"] is not None:
            sd[p + "branch1_conv.weight"] = b["w_sc"].reshape(b["cout"], b["cin"], 1, 1, 1)
        if b["bn_sc"] is not None:
            norms.append(("branch1_norm.", b["bn_sc"]))
        for name, bn in norms:
            for k, t in zip(_BN_KEYS, bn):
                sd[p + name + k] = t.clone()
            sd[p + name + "num_batches_tracked"] = torch.tensor(0)
        if b["se"] is not None:
            w1, b1, w2, b2 = b["se"]
            q = p + "branch2.norm_b.1.block."
            sd[q + "0.weight"], sd[q + "0.bias"] = w1.reshape(*w1.shape, 1, 1, 1), b1.clone()
            sd[q + "2.weight"], sd[q + "2.bias"] = w2.reshape(*w2.shape, 1, 1, 1), b2.clone()
    return sd


def blocks_of(module_state, stage):
    """The inverse: blocks (f32, on the CPU) from the state dict of a module of that stage."""
    sd = {k: v.detach().cpu() for k, v in module_state.items()}
    blocks = draw_blocks(stage, 0)
    for i, b in enumerate(blocks):
        p = f"res_blocks.{i}."
        b["w_a"] = sd[p + "branch2.conv_a.weight"].reshape(b["cinner"], b["cin"]).float()
        b["w_b"] = sd[p + "branch2.conv_b.weight"].reshape(b["cinner"], 27).float()
        b["w_c"] = sd[p + "branch2.conv_c.weight"].reshape(b["cout"], b["cinner"]).float()
        bn = lambda name: tuple(sd[p + name + k].float() for k in _BN_KEYS)                       # noqa: E731
        b["bn_a"], b["bn_b"], b["bn_c"] = bn("branch2.norm_a."), bn("branch2.norm_b.0."), bn("branch2.norm_c.")
        if b["w_sc"] is not None:
            b["w_sc"] = sd[p + "branch1_conv.weight"].reshape(b["cout"], b["cin"]).float()
        if b["bn_sc"] is not None:
            b["bn_sc"] = bn("branch1_norm.")
        if b["se"] is not None:
            q = p + "branch2.norm_b.1.block."
            b["se"] = (sd[q + "0.weight"].flatten(1).float(), sd[q + "0.bias"].float(), sd[q + "2.weight"].flatten(1).float(),
                       sd[q + "2.bias"].float())
    return blocks
