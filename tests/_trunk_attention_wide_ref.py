"""Cases, float64 reference and a CPU emulation for the trunk's fused cross-attention at 385 .. 1024 keys (csrc/sdnet_attention_wide.hip:
ruart_attn_fwd_wide / ruart_attn_bwd_wide).  Test infrastructure: torch on the CPU, no GPU import; used by
tests/test_gpu_trunk_attention_wide.py and proven on the CPU by tests/test_trunk_attention_wide_ref.py.

The operation, the float64 reference, the gradient formulas and every bound are those of tests/_trunk_attention_ref.py (``R``), taken
from there unchanged: R._mask, R.reference_forward, R._finish, R.forward_bounds, R.backward_bounds, R.ratio, R.worst_ratios,
R.effective_keys.  No constant is added and none was fitted to a GPU result.  Why R's counts hold for the key-block kernels as they are:
  N_SUM     the softmax normaliser and the backward's row sum are taken ONCE over the complete row, by the reduction R.n_sum describes
            (16 strided lanes of ceil(L2 / 16) terms, 4 shuffle steps); the single-query form's block reduction passes a term through
            ceil(L2 / 256) + 6 + 4 additions at most, fewer than that at every L2 here.
  chains    a score accumulates over h in 64-wide chunks in order, inside one key block (h terms, as R counts); the context and
            grad_pa = dS k accumulators run through the key blocks in order without a break: one chain over L2 keys, g(L2 + C_PS) and
            g(L2), as R counts.  grad_pk / grad_v come from the 384-key kernels' own per-16-key-rows product (chains over L1).
The case table is this file's own (R._CASES is left alone: the existing parametrisations are taken from it); inputs are scaled per
regime exactly as R.case does.  KB = 256 restates the kernels' key-block size (source_key_block() reads it out of the source): the
cases sit on both sides of the block edges 512 and 768 and at the upper end 1024.

emulate_forward / emulate_backward redo the block-wise arithmetic in fp32 torch; ``defect`` breaks one thing a block-wise kernel can
get wrong (DEFECTS), to show that the bounds would catch it (defect_shows says where each can show)."""
import functools
import os
import re

import torch

from tests import _trunk_attention_ref as R

KB = 256
MIN_L2, MAX_L2 = 385, 1024

DEFECTS = ("block_unmasked", "norm_drop_last_block", "v_block_stale", "rowsum_one_block")
FORWARD_DEFECTS = ("block_unmasked", "norm_drop_last_block", "v_block_stale")

# name: (B, L1, L2, h, D3, relu, diag ("none" | "one" | "vec"), prob_scale, regime, mask kind, form ("wide" | "attn1w"))
_CASES = {
    "a1_385_ragged":  (3, 1, 385, 64, 64, 0, "none", False, "soft", "ragged", "attn1w"),
    "a1_1024_full":   (1, 1, 1024, 250, 250, 0, "none", False, "soft", "full", "attn1w"),
    "q1_400_relu":    (1, 1, 400, 3, 5, 1, "none", False, "soft", "holes", "wide"),
    "q1_513_ps":      (3, 1, 513, 65, 63, 0, "none", True, "soft", "first", "wide"),
    "k385_one":       (1, 15, 385, 1, 1, 0, "one", False, "soft", "full", "wide"),
    "k400_ps":        (3, 17, 400, 63, 64, 1, "vec", True, "soft", "holes", "wide"),
    "k512_relu_one":  (1, 16, 512, 64, 65, 1, "one", False, "soft", "full", "wide"),
    "k513_offset":    (3, 15, 513, 63, 63, 0, "vec", False, "offset", "holes", "wide"),
    "k513_onelast":   (3, 33, 513, 250, 64, 1, "vec", True, "soft", "onelast", "wide"),
    "k767_peaked":    (3, 17, 767, 64, 5, 1, "vec", False, "peaked", "ragged", "wide"),
    "k768_relu":      (1, 33, 768, 65, 250, 1, "none", False, "soft", "first", "wide"),
    "k769_offset":    (3, 16, 769, 250, 65, 0, "one", False, "offset", "first", "wide"),
    "k1023_vec":      (1, 33, 1023, 250, 250, 0, "vec", False, "soft", "holes", "wide"),
    "k1024_full":     (3, 16, 1024, 3, 63, 0, "none", False, "soft", "full", "wide"),
    "k1024_ragged":   (3, 17, 1024, 65, 250, 1, "one", False, "soft", "ragged", "wide"),
    "k1024_peaked":   (3, 15, 1024, 64, 1, 0, "none", False, "peaked", "holes", "wide"),
}
REGIMES = R.REGIMES
CHAINED = {"soft": "k400_ps", "peaked": "k767_peaked", "offset": "k513_offset"}      # one forward -> backward chain per regime
AUTOGRAD_CASES = ("k400_ps", "k1024_ragged")                                         # formulas against float64 autograd


def cases():
    return list(_CASES)


def dispatch_form(L1, relu, diag_len, ps):
    """the kernel form ruart_attn_fwd_wide / _bwd_wide launch: the single-query pair or the key-block kernels"""
    return "attn1w" if (L1 == 1 and not relu and diag_len == 0 and not ps) else "wide"


def source_key_block():
    """(KB, lowest, highest accepted L2) as csrc/sdnet_attention_wide.hip states them"""
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ruart_amd", "csrc", "sdnet_attention_wide.hip")).read()
    return tuple(int(re.search(r"#define %s (\d+)" % n, text).group(1)) for n in ("KB", "ATTN_WIDE_MIN_L2", "ATTN_WIDE_MAX_L2"))


@functools.lru_cache(maxsize=None)
def case(name):
    """inputs (fp32), float64 reference forward and backward of one case; built once and shared - do not modify.  R.case's construction,
    line by line, on this file's table (other seeds)."""
    B, L1, L2, h, D3, relu, diag_kind, use_ps, regime, mask_kind, form = _CASES[name]
    c = R.Case()
    c.name, c.B, c.L1, c.L2, c.h, c.D3, c.relu, c.regime, c.mask_kind, c.form = name, B, L1, L2, h, D3, relu, regime, mask_kind, form
    c.diag_len = {"none": 0, "one": 1, "vec": h}[diag_kind]
    c.diag_kind = diag_kind
    g = torch.Generator().manual_seed(1001 + sorted(_CASES).index(name))
    pa, pk = torch.randn(B, L1, h, generator=g), torch.randn(B, L2, h, generator=g)
    c.v, c.gout = torch.randn(B, L2, D3, generator=g), torch.randn(B, L1, D3, generator=g)
    c.mask = R._mask(mask_kind, B, L2, g)
    c.diag = None
    if diag_kind == "one":
        c.diag = torch.tensor([-0.6])
    elif diag_kind == "vec":
        c.diag = torch.randn(h, generator=g)
        c.diag = torch.where(c.diag.abs() < 0.1, torch.full_like(c.diag, 0.5), c.diag)
    c.ps = None
    if use_ps:
        c.ps = (torch.rand(B, L1, L2, generator=g) >= R.DROP_P).float() / (1.0 - R.DROP_P)
        c.ps[B - 1, L1 - 1] = 0.0                       # a row whose kept set is empty
    if regime in ("soft", "offset"):                    # scale pa and pk so that the live scores of a row spread by about SOFT_STD
        _, _, S, _, _ = R.reference_forward(pa, pk, c.v, c.mask, c.diag, relu, None)
        live = (c.mask != 0)[:, None, :].expand_as(S)
        n = live.sum(-1, keepdim=True).clamp(min=1)
        S0 = torch.where(live, S, torch.zeros_like(S))
        mean = S0.sum(-1, keepdim=True) / n
        std = float((torch.where(live, S - mean, torch.zeros_like(S)) ** 2).sum() / max(float(live.sum()), 1.0)) ** 0.5
        n_live = (c.mask != 0).sum(-1)
        target = R.SOFT_STD_FEW if bool(((n_live >= 8) & (n_live < R.SOFT_FEW)).any()) else R.SOFT_STD
        if std > 0:
            s = float(torch.tensor((target / std) ** 0.5, dtype=torch.float32))
            pa, pk = pa * s, pk * s
    if regime == "offset":                              # a common shift of a whole row's scores through column 0: +80, -100, others
        assert not relu and h >= 2 and B * L1 >= 2
        d0 = 1.0 if c.diag is None else float(c.diag[0])
        shift = torch.randn(B, L1, generator=g) * 20.0
        shift.view(-1)[0], shift.view(-1)[1] = 80.0, -100.0
        pa[:, :, 0] = shift / d0
        pk[:, :, 0] = 1.0
    c.pa, c.pk = pa.contiguous(), pk.contiguous()
    return R._finish(c)


def variant(base, tag, **attrs):
    """the case ``base`` with some inputs replaced (``pa``: other projected queries; ``diag`` with ``diag_len`` / ``diag_kind``), its
    float64 reference rebuilt"""
    c = R.Case()
    c.__dict__.update(base.__dict__)
    c.__dict__.update(attrs)
    c.name = base.name + "+" + tag
    return R._finish(c)


# ------------------------------------------------------------------------------------------------------------------------------
# emulation of the key-block kernels' arithmetic in fp32
# ------------------------------------------------------------------------------------------------------------------------------


def _blocks(L2p):
    return [(j0, min(KB, L2p - j0)) for j0 in range(0, L2p, KB)]


def _blocks_mm(x, y, stale=False):
    """x (B, M, L2p) @ y (B, L2p, N) in fp32, one accumulator through the key blocks in order.  stale: the last block's product takes
    the rows of y the block before it staged"""
    acc = torch.zeros(x.shape[0], x.shape[1], y.shape[2], dtype=torch.float32)
    bl = _blocks(x.shape[2])
    for i, (j0, nb) in enumerate(bl):
        y0 = j0 - KB if (stale and i == len(bl) - 1 and i > 0) else j0
        acc = acc + x[:, :, j0:j0 + nb] @ y[:, y0:y0 + nb]
    return acc


def _block_scores(a, kp):
    """a (B, L1, n) . kp (B, L2p, n)^T: per key block, accumulated over the 64-wide chunks of n in order"""
    return torch.cat([R._chunked_mm(a, kp[:, j0:j0 + nb].transpose(1, 2)) for j0, nb in _blocks(kp.shape[1])], -1)


def emulate_forward(c, defect=None):
    """(probs (B, L1, L2), out (B, L1, D3)) fp32.  defect: None or
      "block_unmasked"        the mask is not applied to the keys of the last key block (its pad keys stay out)
      "norm_drop_last_block"  the last (partial) key block is left out of the normaliser's sum
      "v_block_stale"         the context product of the last key block runs on the value rows staged for the block before it"""
    assert defect is None or defect in DEFECTS
    L2, L2p = c.L2, R.up16(c.L2)
    last0 = _blocks(L2p)[-1][0]
    a, k = R._act(c, None)
    S = _block_scores(a, R._pad_keys(k, L2p))
    livep = torch.zeros(c.B, L2p, dtype=torch.bool)
    livep[:, :L2] = c.live
    if defect == "block_unmasked":
        livep[:, last0:L2] = True
    S = S.masked_fill(~livep[:, None, :], float("-inf"))
    mx = S.amax(-1, keepdim=True)
    e = torch.exp(S - mx)
    es = e.clone()
    if defect == "norm_drop_last_block":
        es[..., last0:] = 0.0
    inv = 1.0 / R._lanes16_sum(es)
    p = e * inv
    pc = p.clone()
    if c.ps is not None:
        pc[..., :L2] = pc[..., :L2] * c.ps
    out = _blocks_mm(pc, R._pad_keys(c.v, L2p), stale=(defect == "v_block_stale"))
    return p[..., :L2].contiguous(), out


def emulate_backward(c, probs, defect=None):
    """dict(grad_pa, grad_pk, grad_v, grad_diag_partial, dS) fp32 from fp32 ``probs``.  defect: None or
      "rowsum_one_block"   rowsum(dP o P) taken over the first key block only"""
    assert defect is None or defect in DEFECTS
    L2, L2p = c.L2, R.up16(c.L2)
    a, k = R._act(c, None)
    dP = _block_scores(c.gout, R._pad_keys(c.v, L2p))[..., :L2]
    if c.ps is not None:
        dP = dP * c.ps
    prod = torch.cat([dP * probs, torch.zeros(c.B, c.L1, L2p - L2)], -1)
    if defect == "rowsum_one_block":
        prod[..., KB:] = 0.0
    dot = R._lanes16_sum(prod)
    dS = probs * (dP - dot)
    Rm = _blocks_mm(torch.cat([dS, torch.zeros(c.B, c.L1, L2p - L2)], -1), R._pad_keys(k, L2p))
    apa = torch.relu(c.pa) if c.relu else c.pa
    ga = Rm if c.diag is None else Rm * c.diag.view(1, 1, -1)
    gk = R._chunked_mm(dS.transpose(1, 2), a)
    if c.relu:
        ga = torch.where(c.pa > 0, ga, torch.zeros_like(ga))
        gk = torch.where(c.pk > 0, gk, torch.zeros_like(gk))
    gv = R._chunked_mm((probs if c.ps is None else probs * c.ps).transpose(1, 2), c.gout)
    nt = (c.L1 + 15) // 16
    t = torch.zeros(c.B, nt * 16, c.h)
    t[:, :c.L1] = Rm * apa
    return dict(grad_pa=ga, grad_pk=gk, grad_v=gv, grad_diag_partial=t.view(c.B, nt, 16, c.h).sum(2), dS=dS)


def defect_shows(name, defect):
    """whether ``defect`` can move a result of case ``name`` past rounding at all (read from the case's regime and mask); soft scores
    everywhere: peaked ones can leave the whole affected block without weight
      block_unmasked        a masked key inside the last key block
      norm_drop_last_block  a live key inside the last key block
      v_block_stale         a live key inside the last key block
      rowsum_one_block      a sample with live keys in the first block and behind it"""
    c = case(name)
    if c.regime != "soft":
        return False
    last0 = _blocks(R.up16(c.L2))[-1][0]
    if defect == "block_unmasked":
        return bool((~c.live[:, last0:]).any())
    if defect in ("norm_drop_last_block", "v_block_stale"):
        return bool(c.live[:, last0:].any())
    if defect == "rowsum_one_block":
        return bool((c.live[:, :KB].any(-1) & c.live[:, KB:].any(-1)).any())
    raise KeyError(defect)


def control_cases():
    """(case name, defect) of every negative control that can show"""
    return [(n, d) for n in cases() for d in DEFECTS if defect_shows(n, d)]
