"""Float64 references of the trainable encoder's dropout-on arithmetic with EXPLICIT masks (test infrastructure; plain torch on the
CPU, imported by the GPU tests and by their CPU companions in tests/test_dropout_ref.py).

  attention(qkv, cu, heads, masks)     packed self-attention per sequence, O = (softmax(Q K^T) o M) V  (Models/Bert/modeling.py:224-250
                                       with the attention-probability dropout of :244-246 as a given multiplier M of 0 or 1/(1-p),
                                       shape (heads, query, key-in-sequence) per sequence); queries arrive pre-scaled, as in
                                       tests/test_gpu_train_kernels.py
  encoder_mixed(w, cfg, ...)           BERT encoder on a packed stream, oracle.ruart_oracle.bert_forward's semantics, one mask per
                                       dropout site; returns sum_l layer_w[l] * layer_l, differentiable in every parameter and in layer_w
  mutation=...                         deliberately WRONG backward passes.  They exist only to show that the bounds the GPU tests hold
                                       the kernels to would catch such a kernel: (a) "delta_no_D", (b) "ds_no_D", (c) "next_head",
                                       (d) "transposed" for the attention, ``bwd_masks`` (a site's backward multiplies with another
                                       mask than its forward) for the encoder.

Mask sites of the encoder, as keys of the ``masks`` dict:  "emb" (T, H): after the embeddings' LayerNorm;  ("attn", l): list of
(heads, n, n) per sequence;  ("ao", l) (T, H): attention-output dense, before residual + LayerNorm;  ("out", l) (T, H): output dense,
before residual + LayerNorm.  A missing key is the identity."""
import math

import torch
import torch.nn.functional as F

ATTN_MUTATIONS = ("delta_no_D", "ds_no_D", "next_head", "transposed")


class _DropAttention(torch.autograd.Function):
    """One sequence, all heads: q, k, v (heads, n, 64), M (heads, n, n).  The backward is written out the way the kernels compute it
    (csrc/bert_train_attn.hip: dPd = dO V^T, delta = sum_k P D dPd, dS = P o (D o dPd - delta)), so that single terms can be broken
    on purpose; ``mutation`` None must equal plain autograd (tests/test_dropout_ref.py checks that)."""

    @staticmethod
    def forward(ctx, q, k, v, M, Mb, mutation):
        P = torch.softmax(q @ k.transpose(1, 2), -1)
        ctx.save_for_backward(q, k, v, P, M, Mb)
        ctx.mutation = mutation
        return (P * M) @ v

    @staticmethod
    def backward(ctx, dO):
        q, k, v, P, M, Mb = ctx.saved_tensors
        mut = ctx.mutation
        D = M if Mb is None else Mb                           # the multiplier the BACKWARD regenerates
        if mut == "next_head":
            D = torch.roll(M, -1, 0)                          # head h reads head h+1's stream
        elif mut == "transposed":
            D = M.transpose(1, 2)                             # query token and key offset exchanged in the index
        dV = (P * D).transpose(1, 2) @ dO
        dPd = dO @ v.transpose(1, 2)
        delta = (P * dPd).sum(-1, keepdim=True) if mut == "delta_no_D" else (P * D * dPd).sum(-1, keepdim=True)
        dS = P * (dPd - delta) if mut == "ds_no_D" else P * (D * dPd - delta)
        return dS @ k, dS.transpose(1, 2) @ q, dV, None, None, None


def attention(qkv, cu, heads, masks=None, mutation=None, bwd_masks=None, plain=False):
    """qkv (T, 3 * heads * 64) float64 = [Q | K | V] rows of the packed stream, Q pre-scaled; ``cu``: sequence boundaries; ``masks``:
    per sequence (heads, n, n) or None.  ``plain``: the forward as ordinary torch ops (autograd derives the backward)."""
    H = heads * 64
    outs = []
    for s, (a, b) in enumerate(zip(cu[:-1], cu[1:])):
        a, b = int(a), int(b)
        q, k, v = [qkv[a:b, i * H:(i + 1) * H].reshape(b - a, heads, 64).transpose(0, 1) for i in range(3)]
        M = torch.ones(heads, b - a, b - a, dtype=qkv.dtype) if masks is None else masks[s]
        if plain:
            o = (torch.softmax(q @ k.transpose(1, 2), -1) * M) @ v
        else:
            o = _DropAttention.apply(q, k, v, M, None if bwd_masks is None else bwd_masks[s], mutation)
        outs.append(o.transpose(0, 1).reshape(b - a, H))
    return torch.cat(outs, 0)


class _MaskFwdBwd(torch.autograd.Function):
    """y = x o A in the forward, dx = dy o B in the backward: a backward that regenerates another site's mask."""

    @staticmethod
    def forward(ctx, x, A, B):
        ctx.save_for_backward(B)
        return x * A

    @staticmethod
    def backward(ctx, g):
        return g * ctx.saved_tensors[0], None, None


def encoder_mixed(w, cfg, ids, pos, cu, layer_w, masks, bwd_masks=None):
    """sum_l layer_w[l] * layer_l, (T, H): oracle.ruart_oracle.bert_forward (modeling.py:185-199 embeddings, :224-250 self-attention,
    :260-264 / :299-303 dense -> dropout -> + input -> LayerNorm, :286-289 GELU) on a packed stream of whole sequences, token type 0.
    ``w``: parameters under the encoder's own names (no "bert." prefix), float64; ``bwd_masks``: sites whose backward multiplies with
    another mask than the forward (same keys as ``masks``)."""
    H, nh = int(cfg["hidden_size"]), int(cfg["num_attention_heads"])
    bwd_masks = bwd_masks or {}

    def drop(x, key):
        if key not in masks:
            return x
        return _MaskFwdBwd.apply(x, masks[key], bwd_masks[key]) if key in bwd_masks else x * masks[key]

    def ln(x, name):
        return F.layer_norm(x, (H,), w[name + ".gamma"], w[name + ".beta"], 1e-12)

    e = "embeddings."
    x = w[e + "word_embeddings.weight"][ids] + w[e + "position_embeddings.weight"][pos] + w[e + "token_type_embeddings.weight"][0]
    x = drop(ln(x, e + "LayerNorm"), "emb")
    mixed = 0.0
    for l in range(int(cfg["num_hidden_layers"])):
        p = "encoder.layer.%d." % l

        def lin(name, t, scale=1.0):
            return F.linear(t, w[p + name + ".weight"], w[p + name + ".bias"]) * scale

        qkv = torch.cat([lin("attention.self.query", x, 1.0 / math.sqrt(H // nh)), lin("attention.self.key", x),
                         lin("attention.self.value", x)], 1)
        ctx = attention(qkv, cu, nh, masks.get(("attn", l)), bwd_masks=bwd_masks.get(("attn", l)))
        a = ln(drop(lin("attention.output.dense", ctx), ("ao", l)) + x, p + "attention.output.LayerNorm")
        f = F.gelu(lin("intermediate.dense", a))
        x = ln(drop(lin("output.dense", f), ("out", l)) + a, p + "output.LayerNorm")
        mixed = mixed + layer_w[l] * x
    return mixed


def bernoulli_masks(g, p, cu, heads):
    """synthetic attention masks: per sequence (heads, n, n) float64 of 0 or 1/(1-p)"""
    return [(torch.rand(heads, int(b - a), int(b - a), generator=g) >= p).double() / (1.0 - p) for a, b in zip(cu[:-1], cu[1:])]


# ---- statistics of recovered masks ---------------------------------------------------------------------------------------------
def keep_sigmas(keep, p):
    """|kept share - (1 - p)| of a boolean tensor in binomial standard deviations"""
    n = keep.numel()
    return abs(float(keep.double().mean()) - (1.0 - p)) / math.sqrt(p * (1.0 - p) / n)


def agree_sigmas(a, b, p):
    """|share of equal entries - (p^2 + (1-p)^2)| of two boolean tensors in standard deviations of independent Bernoulli(1 - p) streams"""
    r = p * p + (1.0 - p) * (1.0 - p)
    n = a.numel()
    return abs(float((a == b).double().mean()) - r) / math.sqrt(r * (1.0 - r) / n)


def shifted_agree_sigmas(a, b, d, p):
    """agreement of a[i + d] with b[i] over the overlap of two flat boolean streams, in sigmas of that overlap; None when out of range"""
    n = a.numel()
    if abs(d) >= n:
        return None
    if d >= 0:
        return agree_sigmas(a[d:], b[:n - d], p)
    return agree_sigmas(a[:n + d], b[-d:], p)


# ---- the whole-encoder case shared by tests/test_gpu_bert_train_dropout.py and its CPU companion ----------------------------------
ENCODER_LENS = [5, 64, 1, 30, 130, 65, 33]            # windows of several sequences, a window of exactly 64, chunks with ragged tails
ENCODER_LAYER_W = [0.7, -0.45]


def encoder_case():
    """(cfg, checkpoint as numpy arrays, ids (N, L) int64, mask (N, L) bool, cu): a two-layer encoder small enough for a float64
    autograd pass on the CPU in a second, hidden and intermediate sizes the 16-bit path takes (multiples of 256)"""
    import numpy as np
    from ruart_amd import synth
    cfg = synth.bert_config(hidden_size=256, num_attention_heads=4, intermediate_size=512, num_hidden_layers=2, max_position_embeddings=256)
    state = synth.make_bert_weights(cfg, seed=41, w_std=0.05)
    g = torch.Generator().manual_seed(41)
    L = max(ENCODER_LENS)
    ids = torch.randint(5, int(cfg["vocab_size"]), (len(ENCODER_LENS), L), generator=g)
    mask = torch.arange(L).unsqueeze(0) < torch.tensor(ENCODER_LENS).unsqueeze(1)
    ids[~mask] = 0
    cu = np.concatenate([[0], np.cumsum(ENCODER_LENS)])
    return cfg, state, ids, mask, cu


def encoder_reference(cfg, params64, ids, mask, cu, g_mixed, masks, bwd_masks=None):
    """One float64 forward + backward of <g_mixed, mixed>: (mixed, gradients by parameter name, d layer_w).  ``params64``: name ->
    float64 tensor (left untouched: fresh leaves are made here)."""
    w = {n: t.detach().clone().requires_grad_() for n, t in params64.items()}
    lw = torch.tensor(ENCODER_LAYER_W, dtype=torch.float64, requires_grad=True)
    pos = torch.arange(ids.shape[1]).unsqueeze(0).expand_as(ids)[mask]
    mixed = encoder_mixed(w, cfg, ids[mask], pos, cu, lw, masks, bwd_masks)
    (mixed * g_mixed).sum().backward()
    return mixed.detach(), {n: (t.grad if t.grad is not None else torch.zeros_like(t)) for n, t in w.items()}, lw.grad


def rel_l2(got, want):
    return float((got.double() - want.double()).norm() / want.double().norm())


# ---- the attention cases shared by tests/test_gpu_train_kernels.py and its CPU companion ------------------------------------------
ATTN_FAMILIES = {"window": ([5, 1, 64, 3, 8, 30, 30, 7, 50, 2, 2, 2, 63], 3),             # (sequence lengths, heads)
                 "long": ([5, 65, 64, 130, 3, 512, 30, 128, 200, 40], 2)}
ATTN_BOUNDS = (4e-2, 1.5e-2)      # per sequence and block of [dQ | dK | dV]: max |err| / max |ref|, rel-L2 (the p = 0 tests' bf16 bounds)


def attention_inputs(family, seed=31):
    """(lens, heads, cu, qkv f16-exact float64 (T, 3H) with peaked rows, dO bf16-exact float64 (T, H))"""
    import numpy as np
    lens, heads = ATTN_FAMILIES[family]
    H = heads * 64
    cu = np.concatenate([[0], np.cumsum(lens)])
    T = int(cu[-1])
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(T, 3 * H, generator=g)
    qkv[:, :H] *= 0.125 * 3                                       # queries arrive pre-scaled; *3: peaked rows too
    dO = torch.randn(T, H, generator=g) * 1e-3
    return lens, heads, cu, qkv.half().double(), dO.bfloat16().double()


def attention_grads(qkv, dO, cu, heads, masks, mutation=None, plain=False):
    """(context rows, d[Q | K | V] rows) of <dO, O>"""
    x = qkv.clone().requires_grad_()
    out = attention(x, cu, heads, masks, mutation=mutation, plain=plain)
    out.backward(dO)
    return out.detach(), x.grad


def block_errors(got, want):
    """(max |err| / max |ref|, rel-L2) of one block"""
    got, want = got.double(), want.double()
    return float((got - want).abs().max()) / float(want.abs().max()), float((got - want).norm() / want.norm())
