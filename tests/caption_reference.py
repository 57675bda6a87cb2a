"""Host reference for the caption-decoder kernels (helper of test_caption_ops_gpu.py / test_cpu.py, not a test module).

Plain torch-CPU float64 restatements of the operations `include/change3d_hip.h` declares for the change-captioning
decoder, written from those definitions: nothing here goes through `nn.MultiheadAttention`, `nn.LayerNorm` or
`F.cross_entropy`.  Where the device draws a dropout mask, the function takes the KEEP mask (1 = kept, 0 = dropped, or None
for "keep everything") and the probability, so a test can hand it the mask it read back from the device.  Gradients come
from autograd on the float64 graph.

Layouts: activations are sequence-first, [L, B, D] (device row l*B + b); per-head tensors are [B, H, L, hd]; the device's
saved probabilities [(h*B + b)][Lq][Lk] are `P.permute(1, 0, 2, 3)` of the [B, H, Lq, Lk] used here."""
import math

import numpy as np
import torch


def q(t, dtype):
    """Quantise a reference input the way the device tensor stores it, then compute in float64."""
    return t.to(dtype).double()


def keep_scale(p):
    """1 / (1 - p) as the kernels evaluate it (float32 arithmetic)."""
    p32 = np.float32(p)
    return 1.0 if p32 <= 0 else float(np.float32(1.0) / (np.float32(1.0) - p32))


def drop(x, mask, p):
    """x * mask / (1 - p); mask None = nothing dropped."""
    return x if mask is None or p <= 0 else x * (mask.to(x.dtype).reshape(x.shape) * keep_scale(p))


def embed(tokens, emb, pe, mask=None, p=0.0):
    """tokens int64 [B, L] (clamped into [0, V)), emb [V, D], pe [>= L, D] -> dropout(emb[tokens] + pe) as [L, B, D]."""
    V = emb.shape[0]
    L = tokens.shape[1]
    t = tokens.clamp(0, V - 1).t()                                  # [L, B]
    return drop(emb[t] + pe[:L, None, :], mask, p)


def layernorm(x, a, gamma, beta, eps=1e-5):
    """LayerNorm(x + a) over the last dimension (a may be None) -> (y, mean, rstd)."""
    t = x if a is None else x + a
    mean = t.mean(-1, keepdim=True)
    var = ((t - mean) ** 2).mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    return (t - mean) * rstd * gamma + beta, mean.squeeze(-1), rstd.squeeze(-1)


def attention(q_, k, v, scale, causal, mask=None, p=0.0):
    """q_ [B, H, Lq, hd], k / v [B, H, Lk, hd] -> (P, o): P = softmax(scale * q k^T (+ -inf above the diagonal)) BEFORE
    dropout, o = dropout(P) v."""
    s = scale * (q_ @ k.transpose(-1, -2))
    if causal:
        Lq, Lk = s.shape[-2:]
        upper = torch.arange(Lk)[None, :] > torch.arange(Lq)[:, None]
        s = s.masked_fill(upper, float("-inf"))
    e = torch.exp(s - s.max(-1, keepdim=True).values)
    P = e / e.sum(-1, keepdim=True)
    return P, drop(P, mask, p) @ v


def packed_ce(logits, caps, declen, ignore_index=0):
    """logits [L, B, V]; target of step (l, b) = caps[b][l + 1]; counted iff l < declen[b], l + 1 < L and target != ignore_index.
    -> (mean negative log-likelihood over the counted steps (0 when there are none), counted steps, top-1 hits with the first
    index winning a tie)."""
    L, B, V = logits.shape
    tgt = torch.full((L, B), ignore_index, dtype=torch.int64)
    tgt[:L - 1] = caps[:, 1:].t()
    counted = (torch.arange(L)[:, None] < declen[None, :]) & (tgt != ignore_index)
    mx = logits.max(-1, keepdim=True).values
    lse = mx.squeeze(-1) + torch.log(torch.exp(logits - mx).sum(-1))
    picked = logits.gather(-1, tgt.clamp(0, V - 1)[..., None]).squeeze(-1)
    n = int(counted.sum())
    nll = ((lse - picked) * counted).sum()
    first_max = (logits == mx).double().argmax(-1)                  # argmax returns the first of equal maxima
    hits = int(((first_max == tgt) & counted).sum())
    return (nll / n if n else nll * 0.0), n, hits


def _heads(t, H):
    L, B, D = t.shape
    return t.reshape(L, B, H, D // H).permute(1, 2, 0, 3)           # [B, H, L, hd]


def _merge(t):
    B, H, L, hd = t.shape
    return t.permute(2, 0, 1, 3).reshape(L, B, H * hd)


def decoder_forward(sd, memory, caps, masks=None, n_head=8, p_attn=0.0, p_pos=0.0, p_out=0.0):
    """The layer stack of `CaptionDecoder` on a state dict of float64 tensors: memory [S, B, D], caps int64 [B, L] -> logits
    [L, B, V].  masks: dict of keep masks, keys "pos" [L, B, D], "out" [L, B, D] and per layer i (i, "attn1") [B, H, L, L],
    (i, "drop1") [L, B, D], (i, "attn2") [B, H, L, S], (i, "drop3") [L, B, D]; a missing key keeps everything."""
    masks = masks or {}
    D = memory.shape[-1]
    H, scale = n_head, 1.0 / math.sqrt(D // n_head)
    L = caps.shape[1]
    x = embed(caps, sd["vocab_embedding.weight"], sd["position_encoding.pe"].reshape(-1, D)[:L], masks.get("pos"), p_pos)
    li = 0
    while f"transformer.layers.{li}.norm1.weight" in sd:
        g = lambda name: sd[f"transformer.layers.{li}.{name}"]  # noqa: E731
        qkv = x @ g("self_attn.in_proj_weight").t() + g("self_attn.in_proj_bias")
        qh, kh, vh = (_heads(t, H) for t in qkv.split(D, dim=-1))
        _, o = attention(qh, kh, vh, scale, True, masks.get((li, "attn1")), p_attn)
        a = _merge(o) @ g("self_attn.out_proj.weight").t() + g("self_attn.out_proj.bias")
        x1, _, _ = layernorm(x, drop(a, masks.get((li, "drop1")), p_attn), g("norm1.weight"), g("norm1.bias"))
        w, b = g("multihead_attn2.in_proj_weight"), g("multihead_attn2.in_proj_bias")
        q2 = x1 @ w[:D].t() + b[:D]
        kv = memory @ w[D:].t() + b[D:]
        _, o = attention(_heads(q2, H), _heads(kv[..., :D], H), _heads(kv[..., D:], H), scale, False,
                         masks.get((li, "attn2")), p_attn)
        a = _merge(o) @ g("multihead_attn2.out_proj.weight").t() + g("multihead_attn2.out_proj.bias")
        x2, _, _ = layernorm(x1, drop(a, masks.get((li, "drop3")), p_attn), g("norm2.weight"), g("norm2.bias"))
        x = x2
        li += 1
    return drop(x, masks.get("out"), p_out) @ sd["wdc.weight"].t() + sd["wdc.bias"]
