"""Float64 reference, derived element-wise error bounds and a CPU emulation of the trunk's fused cross-attention (csrc/sdnet_attention.hip:
attn_fwd / attn_bwd_q / attn_bwd_kv, their register-prefetched forms and the single-query attn1 pair).  Test infrastructure: numpy /
torch on the CPU, no GPU import; used by tests/test_gpu_trunk_attention.py and proven on the CPU by tests/test_trunk_attention_ref.py.

The operation (include/ruart_hip.h), per batch element, restated here in float64 on the fp32 inputs:
    a = act(pa) diag,  k = act(pk)            act = ReLU when relu != 0; diag_len 0: no diag, 1: one scalar, h: per column
    S = a k^T,  S[:, j] = -inf where mask[j] == 0;  P = softmax_j(S);  out = (P o ps) v        ps = prob_scale, optional
and its gradients for a given gO = d loss / d out, as formulas (reference_backward; checked against float64 autograd on the CPU):
    dP = (gO v^T) o ps        dS = P o (dP - rowsum(dP o P))        R = dS k
    grad_pa = R o diag o relu'(pa)        grad_pk = (dS^T a) o relu'(pk)        grad_v = (P o ps)^T gO
    grad_diag_partial[b, t] = sum over the 16 query rows of tile t of  R o act(pa)        (vector diag only)

The bounds.  u = 2^-24 is the unit roundoff of fp32; every product below is an fp32 FMA chain (v_mfma_f32_16x16x4_f32; the attn1
kernels: fmaf chains and wave / block reductions), and a chain or tree over n non-zero terms errs by at most n u times the sum of
the terms' absolute values (zero padding adds exact zeros).  Everything is a quantity of the float64 reference; |.| is element-wise.

  forward
    score       E_s(i,j) = (h + C_ACT) u sum_d |a_id| |k_jd|          C_ACT = 1: the one rounding of act(pa) diag
                E_i = max over the live keys j of E_s(i,j)
    softmax     p_j = exp(s_j - m) / sum_l exp(s_l - m) is invariant under the computed maximum; score errors of at most E_i move every
                numerator and the normaliser by factors within exp(+-E_i): relative exp(2 E_i) - 1.  Then, relative to p_j:
                  C_ARG u (|s_j - m| + D_i)        the rounding of s_j - m (and of a product with log2(e) where expf goes through exp2:
                                                   C_ARG = 2), on the numerator and, probability-weighted, D_i = sum_l p_l |s_l - m|,
                                                   on the normaliser
                  2 C_EXP u                        expf itself, C_EXP = 2 (a 1-ulp function = 2 u), numerator and normaliser
                  N_SUM u                          the normaliser's sum of positive terms: 16 strided lanes of ceil(L2 / 16) terms, then
                                                   4 shuffle steps: N_SUM = ceil(L2 / 16) + 4 (the attn1 block reduction passes a term
                                                   through no more additions than that)
                  (C_RCP + 1) u                    1 / sum (C_RCP = 2: a 1-ulp reciprocal) and the product e inv
                T(i,j) = C_ARG u (|s_ij - m_i| + D_i) + (2 C_EXP + N_SUM + C_RCP + 1) u
                rel_p(i,j) = exp(2 E_i + T (1 + SECOND_ORDER)) - 1
                Every factor 1 + x is at most exp(x) and every 1 / (1 - x) at most exp(x + x^2): with T < 2^-11 (asserted per case)
                SECOND_ORDER = 2^-10 covers the x^2, so the bound is not a first-order one however large E_i is (peaked scores
                of h = 250 reach E_i = 2^-9).
                b_probs = rel_p P + P_FLOOR        P_FLOOR = 2^-126: results below the normal range (flushed or rounded)
                A masked key's probability is exactly 0 (the tests ask for the bits), and so are its gradients.
    context     b_out = (b_probs o |ps|) |v|  +  g(L2 + C_PS) ((P + b_probs) o |ps|) |v|  +  u |out|          (g: below)
                the P error through the product, the chain over L2 keys with the rounding of p ps (C_PS = 1), the fp32 store
  backward, for probabilities that arrive with an absolute error dPin (u P + 2^-149 for the float64 P rounded to fp32; b_probs when
  the kernel's own forward output is fed back), dPin = 0 on masked keys.  g(n) = n u / (1 - n u); the computed magnitudes are
  bounded by P^ = P + dPin, dP^ = |dP| + E_dP, dS^ = |dS| + E_dS, R^ = |R| + E_R, so that no cross term is dropped:
    dP          E_dP = g(D3 + C_PS) |ps| (|gO| |v|^T)                                     chain over D3, the product with ps
    rowsum      E_dot = sum_j (E_dP P^ + |dP| dPin) + g(N_SUM + 1) sum_j dP^ P^           the same 16-lane reduction, one product each
    dS          E_dS = dPin (|dP - dot| + E_dP + E_dot) + P (E_dP + E_dot) + g(2) P^ (dP^ + |dot| + E_dot)
                                                                                          subtraction and product roundings
    R = dS k    E_R = E_dS |k| + g(L2) dS^ |k|                                            chain over L2
    grad_pa     relu'(pa) (|diag| E_R + u (|grad_pa| + |diag| E_R))                       one rounding of R diag
    grad_pk     relu'(pk) (E_dS^T |a| + g(L1 + C_ACT) dS^^T |a|)                          chain over L1, a recomputed with one rounding
    grad_v      (dPin o |ps|)^T |gO| + g(L1 + C_PS) (P^ o |ps|)^T |gO|                    chain over L1, the product p ps
    grad_diag_partial   sum_rows E_R |act(pa)| + g(N_TILE) sum_rows R^ |act(pa)|          N_TILE = 16: the tile's query rows
  The forward's chains use g(n) as well.
  Where a bound is 0 the result has to be the reference exactly.

No constant above was fitted to a GPU result.  emulate_forward / emulate_backward redo the kernels' arithmetic in fp32 torch on the CPU
(64-wide chunks of the contraction, 16-key tiles zero-padded to L2p, the 16-lane strided softmax / rowsum reduction with its xor
butterfly); ``defect`` breaks one thing on purpose (DEFECTS) to show that the bounds would catch such a kernel (defect_shows says
where each one can show).  cases() is the list the CPU and the GPU tests share; case(name) builds inputs and reference once.
"""
import functools
import os
import re

import torch

U32 = 2.0 ** -24
C_ACT = 1.0
C_ARG = 2.0
C_EXP = 2.0
C_RCP = 2.0
C_PS = 1.0
N_TILE = 16.0
SECOND_ORDER = 2.0 ** -10
T_MAX = 2.0 ** -11
P_FLOOR = 2.0 ** -126
SOFT_STD = 1.0                    # the score standard deviation the soft regime is scaled to: about e live keys per effective key
SOFT_STD_FEW = 0.7                # ... and where some sample has 8 to SOFT_FEW - 1 live keys: exp(0.49) = 1.6 keys per effective key, so
SOFT_FEW = 24                     # that 8 live keys still give the 4 effective ones the soft condition asks for
DROP_P = 0.3

DEFECTS = ("norm_drop_last_tile", "tile_unmasked", "p_bf16", "rowsum_no_ps", "pk_no_relu_grad", "diag_on_k", "diag_partial_skip",
           "h_tail_dropped", "v_pass_stale")
FORWARD_DEFECTS = ("norm_drop_last_tile", "tile_unmasked", "p_bf16", "diag_on_k", "h_tail_dropped", "v_pass_stale")


def up16(n):
    return (n + 15) & ~15


PF_EDGES = ((48, 12), (64, 16), (112, 28))     # L2p <= edge -> prefetch unroll width; above the last edge PF_LAST, above STAGED_ABOVE the
PF_LAST, STAGED_ABOVE, MAX_L2 = 32, 128, 384   # staged kernels.  source_dispatch() reads the same table out of csrc/sdnet_attention.hip.
ATTN1_CONDITION = "if (L1 == 1 && !relu && diag_len == 0 && !prob_scale) {"


def dispatch_form(L1, L2, relu, diag_len, ps, prefetch=True):
    """the kernel form ruart_attn_fwd_pscale / _bwd_pscale launch: "attn1", "staged", or the prefetch unroll width 12 / 16 / 28 / 32"""
    if L1 == 1 and not relu and diag_len == 0 and not ps:
        return "attn1"
    L2p = up16(L2)
    if not prefetch or L2p > STAGED_ABOVE:
        return "staged"
    for edge, width in PF_EDGES:
        if L2p <= edge:
            return width
    return PF_LAST


def source_dispatch():
    """the dispatch of ruart_attn_fwd_pscale (macro RUART_AF) and ruart_attn_bwd_pscale (RUART_AQ) as the library's source states it:
    {"AF" | "AQ": (edges, last width, staged-above)}, the number of entry points with the attn1 condition, ATTN_MAX_L2.  The tests'
    restatement above is compared with this on the CPU, so that moving an edge in the library without moving the cases fails."""
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ruart_amd", "csrc", "sdnet_attention.hip")).read()
    forms = {}
    for m in ("AF", "AQ"):
        edges = tuple((int(a), int(b)) for a, b in re.findall(r"else if \(L2p <= (\d+)\) RUART_%s\((\d+)\);" % m, text))
        last = re.findall(r"else RUART_%s\((\d+)\);" % m, text)
        staged = re.findall(r"if \(!g_attn_prefetch \|\| L2p > (\d+)\)\s+hipLaunchKernelGGL\(attn_%s_kernel," % ("fwd" if m == "AF" else "bwd_q"), text)
        assert len(last) == 1 and len(staged) == 1, (m, last, staged)
        forms[m] = (edges, int(last[0]), int(staged[0]))
    return forms, text.count(ATTN1_CONDITION), int(re.search(r"#define ATTN_MAX_L2 (\d+)", text).group(1))


# name: (B, L1, L2, h, D3, relu, diag ("none" | "one" | "vec"), prob_scale, regime, mask kind, form with prefetch on)
_CASES = {
    "a1_min":        (1, 1, 1, 1, 1, 0, "none", False, "soft", "full", "attn1"),
    "a1_ragged":     (3, 1, 100, 250, 250, 0, "none", False, "soft", "ragged", "attn1"),
    "a1_offset":     (3, 1, 128, 64, 64, 0, "none", False, "offset", "full", "attn1"),
    "q1_relu":       (1, 1, 17, 3, 5, 1, "none", False, "soft", "holes", 12),
    "q1_ps":         (3, 1, 49, 65, 63, 0, "none", True, "soft", "first", 16),
    "q1_ps_staged":  (3, 1, 383, 4, 65, 0, "none", True, "peaked", "ragged", "staged"),
    "k1_general":    (1, 16, 1, 3, 1, 1, "vec", False, "soft", "full", 12),
    "k16_one":       (1, 15, 16, 4, 5, 0, "one", False, "soft", "full", 12),
    "k17_onelast":   (3, 33, 17, 1, 250, 1, "one", False, "soft", "onelast", 12),
    "k48_vec":       (3, 17, 48, 63, 64, 0, "vec", False, "soft", "holes", 12),
    "k48_offset":    (1, 33, 48, 65, 65, 0, "one", False, "offset", "first", 12),
    "k49_relu_one":  (1, 16, 49, 64, 65, 1, "one", False, "soft", "ragged", 16),
    "k64_relu_vec":  (3, 33, 64, 65, 63, 1, "vec", False, "soft", "full", 16),
    "k64_peaked":    (1, 16, 64, 250, 250, 0, "none", False, "peaked", "holes", 16),
    "k65_ps":        (1, 33, 65, 250, 250, 1, "vec", True, "soft", "holes", 28),
    "k112_peaked":   (3, 16, 112, 64, 64, 0, "none", False, "peaked", "first", 28),
    "k113_relu":     (1, 17, 113, 250, 65, 1, "none", False, "soft", "ragged", 32),      # U = 32 with four h chunks and two D3 passes
    "k128_ps":       (3, 15, 128, 4, 1, 0, "vec", True, "soft", "holes", 32),
    "k129_relu_one": (1, 33, 129, 65, 65, 1, "one", False, "soft", "full", "staged"),
    "k129_peaked":   (3, 17, 129, 64, 5, 1, "vec", False, "peaked", "ragged", "staged"),
    "k383_full":     (1, 17, 383, 64, 63, 1, "vec", False, "soft", "full", "staged"),
    "k384_full":     (3, 16, 384, 3, 5, 0, "none", False, "soft", "full", "staged"),
    "k384_onelast":  (3, 15, 384, 250, 64, 1, "vec", True, "soft", "onelast", "staged"),
    "k384_offset":   (3, 15, 384, 63, 63, 0, "vec", False, "offset", "holes", "staged"),
}
REGIMES = ("soft", "peaked", "offset")
CHAINED = {"soft": "k65_ps", "peaked": "k129_peaked", "offset": "k48_offset"}      # one forward -> backward chain per regime
GLUE_CASE = "k64_relu_vec"                                                        # soft, vector diag, L1 = 33: the autograd test


def cases():
    return list(_CASES)


class Case:
    pass


def _mask(kind, B, L2, g):
    m = torch.ones(B, L2, dtype=torch.uint8)
    if kind == "full":
        return m
    if kind in ("holes", "first", "onelast"):
        m = (torch.rand(B, L2, generator=g) > 0.3).to(torch.uint8)
        m[:, L2 // 2] = 1                               # every sample keeps a live key
        if kind == "first":
            m[:, 0] = 0
            m[:, L2 - 1] = 1
        if kind == "onelast":                            # sample B // 2: one live key, the last position of the last tile
            m[B // 2] = 0
            m[B // 2, L2 - 1] = 1
        return m
    if kind == "ragged":                                 # per-sample prefixes: all keys, one key, a random cut between
        lens = [L2, 1, max(2, int(torch.randint(2, max(L2, 3), (1,), generator=g)))]
        if B == 1:
            lens = [max(1, (3 * L2) // 5)]
        m.zero_()
        for b in range(B):
            m[b, :lens[b % 3]] = 1
        return m
    raise KeyError(kind)


def reference_forward(pa, pk, v, mask, diag, relu, ps):
    """float64 (a, k, S, P, out) of fp32 / float64 inputs; S holds -inf on masked keys"""
    pa, pk, v = pa.double(), pk.double(), v.double()
    a = torch.relu(pa) if relu else pa
    k = torch.relu(pk) if relu else pk
    if diag is not None:
        a = a * diag.double().view(1, 1, -1)
    S = a @ k.transpose(1, 2)
    S = S.masked_fill(mask[:, None, :] == 0, float("-inf"))
    P = torch.softmax(S, -1)
    out = (P if ps is None else P * ps.double()) @ v
    return a, k, S, P, out


def reference_backward(c, P=None):
    """the gradient formulas of the module docstring in float64: dict(dP, dot, dS, R, grad_pa, grad_pk, grad_v, grad_diag_partial)"""
    P = c.P if P is None else P
    gO, v = c.gout.double(), c.v.double()
    psd = None if c.ps is None else c.ps.double()
    dP = gO @ v.transpose(1, 2)
    if psd is not None:
        dP = dP * psd
    dot = (dP * P).sum(-1, keepdim=True)
    dS = P * (dP - dot)
    R = dS @ c.k
    pa, pk = c.pa.double(), c.pk.double()
    ga = R if c.diag is None else R * c.diag.double().view(1, 1, -1)
    gk = dS.transpose(1, 2) @ c.a
    if c.relu:
        ga = ga * (pa > 0)
        gk = gk * (pk > 0)
    gv = (P if psd is None else P * psd).transpose(1, 2) @ gO
    apa = torch.relu(pa) if c.relu else pa
    nt = (c.L1 + 15) // 16
    prod = torch.zeros(c.B, nt * 16, c.h, dtype=torch.float64)
    prod[:, :c.L1] = R * apa
    return dict(dP=dP, dot=dot, dS=dS, R=R, grad_pa=ga, grad_pk=gk, grad_v=gv, grad_diag_partial=prod.view(c.B, nt, 16, c.h).sum(2))


@functools.lru_cache(maxsize=None)
def case(name):
    """inputs (fp32), float64 reference forward and backward of one case; built once and shared - do not modify"""
    B, L1, L2, h, D3, relu, diag_kind, use_ps, regime, mask_kind, form = _CASES[name]
    c = Case()
    c.name, c.B, c.L1, c.L2, c.h, c.D3, c.relu, c.regime, c.mask_kind, c.form = name, B, L1, L2, h, D3, relu, regime, mask_kind, form
    c.diag_len = {"none": 0, "one": 1, "vec": h}[diag_kind]
    c.diag_kind = diag_kind
    g = torch.Generator().manual_seed(1 + sorted(_CASES).index(name))
    pa, pk = torch.randn(B, L1, h, generator=g), torch.randn(B, L2, h, generator=g)
    c.v, c.gout = torch.randn(B, L2, D3, generator=g), torch.randn(B, L1, D3, generator=g)
    c.mask = _mask(mask_kind, B, L2, g)
    c.diag = None
    if diag_kind == "one":
        c.diag = torch.tensor([-0.6])
    elif diag_kind == "vec":
        c.diag = torch.randn(h, generator=g)
        c.diag = torch.where(c.diag.abs() < 0.1, torch.full_like(c.diag, 0.5), c.diag)
    c.ps = None
    if use_ps:
        c.ps = (torch.rand(B, L1, L2, generator=g) >= DROP_P).float() / (1.0 - DROP_P)
        c.ps[B - 1, L1 - 1] = 0.0                       # a row whose kept set is empty
    if regime in ("soft", "offset"):                    # scale pa and pk so that the live scores of a row spread by about SOFT_STD
        _, _, S, _, _ = reference_forward(pa, pk, c.v, c.mask, c.diag, relu, None)
        live = (c.mask != 0)[:, None, :].expand_as(S)
        n = live.sum(-1, keepdim=True).clamp(min=1)
        S0 = torch.where(live, S, torch.zeros_like(S))
        mean = S0.sum(-1, keepdim=True) / n
        std = float((torch.where(live, S - mean, torch.zeros_like(S)) ** 2).sum() / max(float(live.sum()), 1.0)) ** 0.5
        n_live = (c.mask != 0).sum(-1)
        target = SOFT_STD_FEW if bool(((n_live >= 8) & (n_live < SOFT_FEW)).any()) else SOFT_STD
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
    return _finish(c)


def _finish(c):
    c.a, c.k, c.S, c.P, c.out = reference_forward(c.pa, c.pk, c.v, c.mask, c.diag, c.relu, c.ps)
    c.live = (c.mask != 0)
    c.bwd = reference_backward(c)
    return c


def case_with_pa(base, pa):
    """the case ``base`` with other projected queries (fp32, same shape): the autograd test's pa = x W^T as the GPU computed it"""
    c = Case()
    c.__dict__.update(base.__dict__)
    c.name, c.pa = base.name + "+pa", pa.float().contiguous()
    return _finish(c)


def effective_keys(c):
    """(B,) median over a sample's query rows of 1 / sum_j p_j^2, and (B,) live keys per sample"""
    return (1.0 / (c.P ** 2).sum(-1)).median(-1).values, c.live.sum(-1)


# ------------------------------------------------------------------------------------------------------------------------------
# bounds
# ------------------------------------------------------------------------------------------------------------------------------


def gamma(n):
    return n * U32 / (1.0 - n * U32)


def n_sum(L2):
    return float((L2 + 15) // 16 + 4)


def forward_bounds(c):
    """(b_probs (B, L1, L2), b_out (B, L1, D3)) float64, module docstring"""
    live = c.live[:, None, :]
    A = c.a.abs() @ c.k.abs().transpose(1, 2)
    E_s = torch.where(live, gamma(c.h + C_ACT) * A, torch.zeros_like(A))
    E = E_s.amax(-1, keepdim=True)
    m = c.S.amax(-1, keepdim=True)
    sm = torch.where(live, (c.S - m).abs(), torch.zeros_like(A))
    D = (c.P * sm).sum(-1, keepdim=True)
    T = C_ARG * U32 * (sm + D) + (2 * C_EXP + n_sum(c.L2) + C_RCP + 1) * U32
    assert float(T.max()) < T_MAX, (c.name, float(T.max()))
    rel = torch.expm1(2 * E + T * (1 + SECOND_ORDER))
    b_probs = rel * c.P + P_FLOOR
    absps = torch.ones_like(c.P) if c.ps is None else c.ps.double().abs()
    va = c.v.double().abs()
    b_out = (b_probs * absps) @ va + gamma(c.L2 + C_PS) * (((c.P + b_probs) * absps) @ va) + U32 * c.out.abs()
    return b_probs, b_out


def probs_input_error(c, chained=False):
    """dPin: the absolute error of the probabilities the backward is given - the float64 P rounded to fp32, or the kernel's own forward
    output (its bound); 0 on masked keys, whose probability is exactly 0 either way"""
    e = forward_bounds(c)[0] if chained else U32 * c.P + 2.0 ** -149
    return torch.where(c.live[:, None, :], e, torch.zeros_like(e))


def backward_bounds(c, chained=False):
    """dict of float64 bounds for grad_pa, grad_pk, grad_v, grad_diag_partial (and dS: the workspace), module docstring"""
    r, P = c.bwd, c.P
    dPin = probs_input_error(c, chained)
    absps = torch.ones_like(P) if c.ps is None else c.ps.double().abs()
    gOa, va, ka, aa = c.gout.double().abs(), c.v.double().abs(), c.k.abs(), c.a.abs()
    dP, dot, dS = r["dP"], r["dot"], r["dS"]
    E_dP = gamma(c.D3 + C_PS) * absps * (gOa @ va.transpose(1, 2))
    Pm, dPm = P + dPin, dP.abs() + E_dP
    E_dot = (E_dP * Pm + dP.abs() * dPin).sum(-1, keepdim=True) + gamma(n_sum(c.L2) + 1) * (dPm * Pm).sum(-1, keepdim=True)
    E_dS = dPin * ((dP - dot).abs() + E_dP + E_dot) + P * (E_dP + E_dot) + gamma(2) * Pm * (dPm + dot.abs() + E_dot)
    dSm = dS.abs() + E_dS
    E_R = E_dS @ ka + gamma(c.L2) * (dSm @ ka)
    pa, pk = c.pa.double(), c.pk.double()
    dg = torch.ones(1, 1, 1, dtype=torch.float64) if c.diag is None else c.diag.double().abs().view(1, 1, -1)
    b_pa = dg * E_R + U32 * (r["grad_pa"].abs() + dg * E_R)
    b_pk = E_dS.transpose(1, 2) @ aa + gamma(c.L1 + C_ACT) * (dSm.transpose(1, 2) @ aa)
    if c.relu:
        b_pa = b_pa * (pa > 0)
        b_pk = b_pk * (pk > 0)
    b_v = (dPin * absps).transpose(1, 2) @ gOa + gamma(c.L1 + C_PS) * ((Pm * absps).transpose(1, 2) @ gOa)
    apa = (torch.relu(pa) if c.relu else pa).abs()
    nt = (c.L1 + 15) // 16
    t = torch.zeros(c.B, nt * 16, c.h, dtype=torch.float64)
    t[:, :c.L1] = E_R * apa + gamma(N_TILE) * (r["R"].abs() + E_R) * apa
    return dict(grad_pa=b_pa, grad_pk=b_pk, grad_v=b_v, grad_diag_partial=t.view(c.B, nt, 16, c.h).sum(2), dS=E_dS + U32 * dS.abs())


def ratio(got, ref, bound):
    """worst |got - ref| / bound; an error where the bound is 0 counts as infinite, a NaN anywhere as infinite"""
    err = (got.double() - ref).abs()
    if bool(torch.isnan(err).any()):
        return float("inf")
    r = torch.where(err == 0, torch.zeros_like(err), err / bound)
    return float(r.max()) if r.numel() else 0.0


# ------------------------------------------------------------------------------------------------------------------------------
# emulation of the kernels' arithmetic in fp32
# ------------------------------------------------------------------------------------------------------------------------------
CH = 64


def _chunked_mm(x, y):
    """x (B, M, K) @ y (B, K, N) in fp32, accumulated over 64-wide chunks of K in order (the kernels' staging)"""
    acc = torch.zeros(x.shape[0], x.shape[1], y.shape[2], dtype=torch.float32)
    for c0 in range(0, x.shape[2], CH):
        acc = acc + x[:, :, c0:c0 + CH] @ y[:, c0:c0 + CH]
    return acc


def _lanes16_sum(x):
    """sum over the last axis (a multiple of 16 long) as the kernels take it: lane c adds the elements c, c + 16, ... in order, then
    the 16 lanes go through the xor butterfly 8, 4, 2, 1"""
    t = x.view(*x.shape[:-1], -1, 16)
    lane = torch.zeros(*x.shape[:-1], 16, dtype=torch.float32)
    for i in range(t.shape[-2]):
        lane = lane + t[..., i, :]
    idx = torch.arange(16)
    for o in (8, 4, 2, 1):
        lane = lane + lane[..., idx ^ o]
    return lane[..., :1]


def _pad_keys(t, L2p):
    return torch.cat([t, torch.zeros(t.shape[0], L2p - t.shape[1], t.shape[2])], 1) if L2p > t.shape[1] else t


def _act(c, defect):
    a = torch.relu(c.pa) if c.relu else c.pa
    k = torch.relu(c.pk) if c.relu else c.pk
    if c.diag is not None:
        a = a * c.diag.view(1, 1, -1)
        if defect == "diag_on_k":
            k = k * c.diag.view(1, 1, -1)
    return a, k


def emulate_forward(c, defect=None):
    """(probs (B, L1, L2), out (B, L1, D3)) fp32.  defect: None or
      "norm_drop_last_tile"  the last 16-key tile is left out of the normaliser's sum
      "tile_unmasked"        in a partial last tile neither the mask nor the end of the keys is honoured: zero-padded keys score 0
      "p_bf16"               P rounded to bf16 before the context product
      "diag_on_k"            diag multiplies k as well as a
      "h_tail_dropped"       the last h % 4 columns of the contraction left out of the scores (the kc = (h - c0 + 3) & ~3 zero-fill path)
      "v_pass_stale"         the context columns of every 64-column pass after the first computed from the pass before's value panel"""
    assert defect is None or defect in DEFECTS
    L2, L2p = c.L2, up16(c.L2)
    a, k = _act(c, defect)
    if defect == "h_tail_dropped" and c.h % 4:
        a = a.clone()
        a[..., c.h & ~3:] = 0.0
    S = _chunked_mm(a, _pad_keys(k, L2p).transpose(1, 2))                       # (B, L1, L2p), 0 on the pad keys
    livep = torch.zeros(c.B, L2p, dtype=torch.bool)
    livep[:, :L2] = c.live
    if defect == "tile_unmasked" and L2 % 16:
        livep[:, L2p - 16:] = True
    S = S.masked_fill(~livep[:, None, :], float("-inf"))
    mx = S.amax(-1, keepdim=True)
    e = torch.exp(S - mx)
    es = e.clone()
    if defect == "norm_drop_last_tile" and L2p > 16:
        es[..., L2p - 16:] = 0.0
    inv = 1.0 / _lanes16_sum(es)
    p = e * inv
    pc = p[..., :L2] if c.ps is None else p[..., :L2] * c.ps
    if defect == "p_bf16":
        pc = pc.to(torch.bfloat16).float()
    out = _chunked_mm(pc, c.v)
    if defect == "v_pass_stale" and c.D3 > CH:
        out[..., CH:] = out[..., :c.D3 - CH].clone()
    return p[..., :L2].contiguous(), out


def emulate_backward(c, probs, defect=None):
    """dict(grad_pa, grad_pk, grad_v, grad_diag_partial, dS) fp32 from fp32 ``probs``.  defect: None or
      "rowsum_no_ps"       rowsum(dP o P) taken before dP is multiplied by prob_scale
      "pk_no_relu_grad"    relu'(pk) missing from grad_pk
      "diag_on_k"          as in the forward: k = act(pk) diag in R = dS k
      "diag_partial_skip"  the grad_diag partial of every sample's second query tile left out (zero)"""
    assert defect is None or defect in DEFECTS
    L2, L2p = c.L2, up16(c.L2)
    a, k = _act(c, defect)
    dP = _chunked_mm(c.gout, c.v.transpose(1, 2))
    raw = dP
    if c.ps is not None:
        dP = dP * c.ps
    pad = torch.zeros(c.B, c.L1, L2p - L2)
    dot = _lanes16_sum(torch.cat([(raw if defect == "rowsum_no_ps" else dP) * probs, pad], -1))
    dS = probs * (dP - dot)
    R = _chunked_mm(dS, k)
    apa = torch.relu(c.pa) if c.relu else c.pa
    ga = R if c.diag is None else R * c.diag.view(1, 1, -1)
    gk = _chunked_mm(dS.transpose(1, 2), a)
    if c.relu:
        ga = torch.where(c.pa > 0, ga, torch.zeros_like(ga))
        if defect != "pk_no_relu_grad":
            gk = torch.where(c.pk > 0, gk, torch.zeros_like(gk))
    gv = _chunked_mm((probs if c.ps is None else probs * c.ps).transpose(1, 2), c.gout)
    nt = (c.L1 + 15) // 16
    prod = torch.zeros(c.B, nt * 16, c.h)
    prod[:, :c.L1] = R * apa
    gd = prod.view(c.B, nt, 16, c.h).sum(2)
    if defect == "diag_partial_skip" and nt > 1:
        gd[:, 1] = 0.0
    return dict(grad_pa=ga, grad_pk=gk, grad_v=gv, grad_diag_partial=gd, dS=dS)


def defect_shows(name, defect):
    """whether ``defect`` can move a result of case ``name`` past rounding at all (read from the case's shape, flags and mask):
      norm_drop_last_tile  soft scores, more than one key tile, a live key in the last one
      tile_unmasked        soft scores (a pad key's score 0 is then an ordinary score) and a partial last tile
      p_bf16               soft scores and a sample with two live keys or more (a single key's p = 1 is exact in bf16)
      rowsum_no_ps         a prob_scale
      pk_no_relu_grad      relu, and soft scores (peaked ones leave dS, hence every grad_pk, close to 0)
      diag_on_k            a diag
      diag_partial_skip    a vector diag and more than one query tile
      h_tail_dropped       h % 4 != 0 and a sample with two live keys or more (a shift of a single key's score moves nothing)
      v_pass_stale         D3 > 64"""
    B, L1, L2, h, D3, relu, diag_kind, use_ps, regime, mask_kind, _ = _CASES[name]
    soft = regime == "soft"
    if defect == "norm_drop_last_tile":
        return soft and up16(L2) > 16 and bool(case(name).live[:, up16(L2) - 16:].any())
    if defect == "tile_unmasked":
        return soft and L2 % 16 != 0
    if defect == "p_bf16":
        return soft and int(case(name).live.sum(-1).max()) >= 2
    if defect == "rowsum_no_ps":
        return use_ps
    if defect == "pk_no_relu_grad":
        return bool(relu) and soft and int(case(name).live.sum(-1).max()) >= 2
    if defect == "diag_on_k":
        return diag_kind != "none" and int(case(name).live.sum(-1).max()) >= 2
    if defect == "diag_partial_skip":
        return diag_kind == "vec" and L1 > 16
    if defect == "h_tail_dropped":
        return h % 4 != 0 and int(case(name).live.sum(-1).max()) >= 2
    if defect == "v_pass_stale":
        return D3 > CH
    raise KeyError(defect)


def control_cases():
    """(case name, defect) of every negative control that can show"""
    return [(n, d) for n in cases() for d in DEFECTS if defect_shows(n, d)]


def worst_ratios(c, probs=None, out=None, grads=None, chained=False):
    """{quantity: worst error / bound} of whatever is given (fp32 results against the case's float64 reference)"""
    res = {}
    if probs is not None or out is not None:
        b_probs, b_out = forward_bounds(c)
        if probs is not None:
            res["probs"] = ratio(probs, c.P, b_probs)
        if out is not None:
            res["out"] = ratio(out, c.out, b_out)
    if grads is not None:
        bb = backward_bounds(c, chained)
        for key in ("grad_pa", "grad_pk", "grad_v"):
            res[key] = ratio(grads[key], c.bwd[key], bb[key])
        if c.diag_len > 1:
            res["grad_diag_partial"] = ratio(grads["grad_diag_partial"], c.bwd["grad_diag_partial"], bb["grad_diag_partial"])
            res["grad_diag"] = ratio(grads["grad_diag_partial"].double().sum((0, 1)), c.bwd["grad_diag_partial"].sum((0, 1)),
                                     bb["grad_diag_partial"].sum((0, 1)))
    return res
