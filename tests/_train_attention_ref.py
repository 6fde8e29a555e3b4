"""Float64 reference, derived element-wise error bounds and a CPU emulation of the trained encoder's attention kernels
(csrc/bert_train_attn.hip: attn_train_fwd, attn_train_bwd, attn_train_fwd_long, attn_train_bwd_long_dq, attn_train_bwd_long_dkv behind
ruart_attn_train_fwd / _bwd / _fwd_long / _bwd_long).  Test infrastructure: numpy / torch on the CPU, no GPU import; used by
tests/test_gpu_train_attention.py and proven on the CPU by tests/test_train_attention_ref.py.

The operation, per sequence and head, restated in float64 on the kernels' own inputs (f16 Q | K | V rows with Q pre-scaled, bf16 dO,
an optional multiplier M of 0 or 1 / (1 - p) on the probabilities, D = M):
    S = Q K^T    P = softmax(S)    Pd = P o M    O = Pd V    lse2 = log2 sum_k exp(s_k)
    dPd = dO V^T    dP = D o dPd    delta = rowsum(P o dP)    dS = P o (dP - delta)    dQ = dS K    dK = dS^T Q    dV = Pd^T dO
    the query / value bias parts of a window or chunk = the column sums of its tokens' dQ / dV rows
(_seq_reference(); tests/test_train_attention_ref.py shows the gradient formulas equal to float64 autograd).

The bounds.  u = 2^-24 (fp32), h = 2^-11 (f16), b = 2^-8 (bf16: common.h's store4 converts with a plain cast, round to nearest even), all
unit roundoffs; F = 2^-25 the absolute error of a conversion to f16 below its normal range (|x| < 2^-14: half a subnormal step) and
2^-134 the same for bf16; g(n) = n u / (1 - n u) bounds an fp32 chain of n additions (an MFMA pair is counted as the chain over its 64
products; products of two f16 values are exact in fp32).  Every bound is a quantity of the float64 reference, per output element, and
computed magnitudes enter as reference + bound (X^ = |X| + E_X) so that no cross term is dropped.  nt = number of 64-key tiles of a
long sequence (1 for a window); masked keys (another sequence of the window, the zero-staged tail of a ragged tile) have P exactly 0
and add exact zeros everywhere.

  forward
    scores      E_s(i,j) = g(64) sum_d |q_id| |k_jd|,   E_i = max_j E_s(i,j)
    softmax     the result is invariant under the computed maximum (window kernel) and under every running maximum (long kernel: a
                weight exp(s - mn_t) prod_t' alpha_t' telescopes to exp(s - m), and the arguments' magnitudes |s - mn_t| +
                sum |mn_t'-1 - mn_t'| add up to |s - m|), so relative to p_j, with sm = |s_ij - m_i| and D_i = sum_l p_l sm_il:
                  C_ARG u (sm + D_i)          exp2((s - m) * log2e): the subtraction, the product, the rounded constant (C_ARG = 3),
                                              numerator and, probability-weighted, normaliser
                  2 C_EXP u                   v_exp_f32 itself, 1 ulp = 2 u (C_EXP = 2: the instruction's published accuracy; the
                                              guides give issue costs for it, no tighter figure), numerator and normaliser
                  N_SUM u                     the normaliser: 16 registers, two shuffle steps (N_SUM = 18); long kernel + nt for the
                                              l * alpha + rs additions
                  (C_RCP + 1) u               1 / sum (C_RCP = 2) and the product with it
                  2 (nt - 1) (C_EXP + 1) u    long kernel: one alpha = exp2(.) and one product with it per later tile, in o and in l
                T(i,j) = their sum;  rel_p = exp(2 E_i + T (1 + SECOND_ORDER)) - 1  (T < 2^-11 asserted per case; SECOND_ORDER = 2^-10
                covers the x^2 of 1 / (1 - x) <= exp(x + x^2));  E_P = rel_p P + 2^-126 (v_exp_f32 flushes)
    multiplier  E_Pd32 = M (E_P + C_MULT u P^)      C_MULT = 3: keep_inv = 1 / (1 - p) in fp32 and the product; 0 when p = 0
    P -> f16    E_Pd = E_Pd32 + h (Pd + E_Pd32) + F [Pd > 0]; the long kernel rounds the UNNORMALISED weight, relative to the running
                maximum: its floor is F in units of exp(s - m) and becomes F (1 + max_j rel_p) / L after the division, L = sum exp(s - m) >= 1
    P . V       pre = E_Pd |V| + g(64 nt + nt) (Pd + E_Pd) |V|;     store: b_ctx = pre + h (|O| + pre) + F
    lse2        m * log2e + log2(l):  log2e (E_i + T_norm (1 + SECOND_ORDER)) with T_norm = C_ARG u D_i + (C_EXP + N_SUM + nt +
                (nt - 1)(C_EXP + 1)) u (the normaliser alone: the computed m and l are consistent, so only the scores' error E_i and
                the sum's own roundings remain), + 2 u log2e (|m| + E_i) (product, constant) + C_LOG u max(|log2 L|, 1) (v_log_f32,
                1 ulp = 2 u of the result; near l = 1 the result's ulp collapses, so its error is counted against 1) + u |lse2| (the add)
  backward (everything in units of the scaled dO of the query's window or chunk: dsc = 2^-e with max |dO| = m 2^e, m in [0.5, 1), 1 for
  an all-zero block - exact, dO is bf16; results are divided by dsc, exactly, per query row)
    dO -> f16   g = dO dsc.  A conversion to f16 errs by h |g| for |g| >= 2^-14 and by F below; dO however is bf16, 8 significant
                bits, and the scale a power of two, so g lies on f16's grid down to 2^-17 (normal: 11 bits; subnormal: steps of 2^-24 =
                2^(-17 - 7)) and converts exactly.  E_g = F for 0 < |g| < 2^-17, else 0.  This floor, divided by dsc, reaches every
                result: a sequence 2^-12 below its window neighbour keeps its leading entries and loses what lies 2^4 below them.
    dPd         E_dPd = E_g |V|^T + g(64) (|g| + E_g) |V|^T;     E_dP = D (E_dPd + C_MULT u dPd^)
    P           window kernel: the forward's fp32 P (E_P above; not rounded to f16).  Long kernels: P = exp2(s * log2e - lse):
                rel = exp(E_s(i,j) + ln2 E_lse + T_L (1 + SECOND_ORDER)) - 1,  T_L = u (2 |s| + |s - LSE|) + C_EXP u  (product and
                constant, subtraction, exp2);  E_lse = u |lse2| + 2^-149 for the float64 lse2 rounded to fp32 (controlled run), the
                forward's lse2 bound when its output is fed back (chained run)
    delta       E_delta = sum_j (E_P dP^ + P E_dP) + g(N_D) sum_j P^ dP^      N_D = 18 + 1 (window), 16 nt + 2 + 2 (long; fp32 in
                the workspace, re-read exactly)
    dS          E_dS32 = E_P (|dP - delta| + E_dP + E_delta) + P (E_dP + E_delta) + g(2) P^ (dP^ + |delta| + E_delta)
                E_dS = E_dS32 + h dS32^ + F [dS32^ > 0];     Pd: E_Pd = E_Pd32 + h Pd32^ + F [Pd > 0]
                A one-token sequence has P = 1 exactly (exp2(0) = 1, 1 / 1 = 1), delta = dP and dS = 0 exactly: E_dS = 0 - as
                long as the subtraction sees the ROUNDED product D dPd that delta was summed from (defect ds_product_fused).
    dQ          pre = (E_dS |K| + g(64 nt) dS^ |K|) / dsc_i
    dK          pre = (E_dS / dsc)^T |Q| + g(64 + nt) (dS^ / dsc)^T |Q|          (one scale and one fp32 add per query tile)
    dV          pre = E_Pd^T (|g| / dsc) + Pd^T (E_g / dsc) + E_Pd^T (E_g / dsc) + g(64 + nt) (Pd + E_Pd)^T ((|g| + E_g) / dsc)
    store       bf16: pre + b (|x| + pre) + 2^-134, and exactly 0 where |x| + pre = 0 (another sequence's keys never enter; a
                one-token sequence's dQ = dK = 0; an all-zero dO block)
    bias parts  fp32, taken before the bf16 rounding: sum over the block's tokens of pre + g(7) sum (|x| + pre)  (four shuffle steps,
                three additions over the waves; the product with 1 / dsc is exact) - an fp32-class bound on top of the operands' f16 errors

No constant above was fitted to a GPU result.  emulate_*() redo the kernels' arithmetic in fp32 torch on the CPU with the same rounding
points (64-key tiles and the online softmax in the long forward, one power of two per window or chunk for dO, f16 for P, Pd and dS,
bf16 stores; sums in torch's order, which the chain bounds cover); ``defect`` breaks one thing on purpose (DEFECTS) and defect_shows()
says on which cases it can show.  cases() is the list the CPU and the GPU tests share; case(name) builds inputs and reference once.

Negative controls that show narrowly - a smallest ratio below 2, or a single kind of case (tests/test_train_attention_ref.py prints the
ratios; profiles/train_attention_tests.txt holds them):
  do_unscaled           in the dK / dV kernel it reaches 1.4 only: a key's row sums the lost low entries of up to 64 queries against a
                        bound that sums their floors F / dsc the same way; the window and dQ kernels show it at over 200.
  ds_bf16               dQ and dK are themselves stored in bf16: b |x| is in their bound, and a bf16 dS adds about as much again.  It shows
                        in the elements that cancellation makes small against sum_k |dS_k| |K_k|, and in the fp32 bias parts.
  bias_after_rounding   a sum of bf16-rounded rows errs like b |x| sqrt(n) while the bias bound grows with n times the f16 terms
                        (h on Pd, E_g / dsc on dO): it shows only in a window that holds one token, where b = 8 h stands against 2 h.
"""
import functools
import math
import os
import re

import numpy as np
import torch

from tests import _dropout_ref as DR
from tests import _encoder_ref as ER

U32 = 2.0 ** -24
UH = ER.UNIT["f16"]
UB = ER.UNIT["bf16"]
F16_FLOOR = 2.0 ** -25
F16_MIN_NORMAL = 2.0 ** -14
F16_EXACT_BF16 = 2.0 ** -17       # a bf16 value (8 significant bits) of at least this magnitude lies on f16's grid, subnormals included
BF16_FLOOR = 2.0 ** -134
F32_FLOOR = 2.0 ** -126
C_ARG = 3.0
C_EXP = 2.0
C_RCP = 2.0
C_LOG = 2.0
C_MULT = 3.0
N_SUM = 18.0
N_BIAS = 7.0
SECOND_ORDER = 2.0 ** -10
T_MAX = 2.0 ** -11
LOG2E = 1.4426950408889634
LN2 = math.log(2.0)
# what the emulation restates of csrc/bert_train_attn.hip (source_constants() reads the same out of its text)
TILE = 64
DROP_IDX_STRIDE = 4096
HEAD_SEED_STRIDE = 0x9E3779B1
DSC_RANGE = (0.5, 1.0)

SOFT_FLOOR = 0.25                 # a soft case: median effective keys 1 / sum p^2 of a sequence of n >= 8 tokens is at least n / 4
PEAK_LEVEL = 0.9                  # a peaked case: the median over the rows of the largest probability (sequences of n >= 8)
DROP_P = 0.1

DEFECTS = ("p_bf16", "ds_bf16", "key_tail_unmasked", "window_neighbour_leak", "alpha_skipped", "delta_from_ctx", "dkv_first_tile_scale",
           "do_unscaled", "lse_natural", "next_head", "last_query_dropped", "bias_after_rounding", "ds_product_fused")
KERNELS = ("win_fwd", "win_bwd", "long_fwd", "dq", "dkv")
# the kernels in which a defect can move a result at all (read from the source: the dQ kernel rounds no P; a zero-staged key row
# gives dP = 0 and K = 0, so an unmasked tail reaches neither delta nor dQ, only the forward's normaliser and the dK / dV kernel's
# value-bias sum; delta is formed in the window and the dQ kernels, and the dK / dV kernel re-reads it)
DEFECT_KERNELS = {
    "p_bf16": ("win_fwd", "win_bwd", "long_fwd", "dkv"),
    "ds_bf16": ("win_bwd", "dq", "dkv"),
    "key_tail_unmasked": ("long_fwd", "dkv"),
    "window_neighbour_leak": ("win_fwd", "win_bwd"),
    "alpha_skipped": ("long_fwd",),
    "delta_from_ctx": ("win_bwd", "dq", "dkv"),
    "dkv_first_tile_scale": ("dkv",),
    "do_unscaled": ("win_bwd", "dq", "dkv"),
    "lse_natural": ("long_fwd", "dq", "dkv"),
    "next_head": KERNELS,
    "last_query_dropped": KERNELS,
    "bias_after_rounding": ("win_bwd",),
    "ds_product_fused": ("win_bwd",),
}

# name: heads, sequence lengths of the packed stream, score regime, dO regime, padded pitches, dropout p
_CASES = {
    "win_soft":      (2, [1, 2, 15, 16, 17, 1, 1, 1, 63, 1, 64, 30, 34, 40, 64, 1, 64, 7], "soft", "uniform", False, 0.0),
    "win_peaked":    (3, [17, 1, 16, 15, 2, 64, 63, 1, 33, 31, 9], "peaked", "uniform", True, 0.0),
    "win_offset":    (2, [16, 17, 15, 1, 64, 20, 2, 30, 63], "offset", "uniform", False, 0.0),
    "win_disparity": (2, [20, 24, 17, 30, 30, 41, 1, 15, 64, 33, 31], "soft", "disparity", True, 0.0),
    "win_drop":      (2, [5, 1, 30, 17, 64, 16, 15, 2, 63, 1], "soft", "uniform", False, DROP_P),
    "long_soft":     (2, [65, 5, 127, 128, 3, 129, 200, 40, 1, 64], "soft", "uniform", False, 0.0),
    "long_peaked":   (3, [200, 7, 65, 129, 1, 128], "peaked", "uniform", True, 0.0),
    "long_rising":   (2, [129, 200, 10, 65], "rising", "uniform", False, 0.0),
    "long_first":    (2, [129, 200, 10, 65], "first", "uniform", True, 0.0),
    "long_offset":   (2, [130, 65, 20, 127], "offset", "uniform", False, 0.0),
    "long_scales":   (2, [512, 9, 128, 64, 65], "soft", "scales", True, 0.0),
    "long_drop":     (2, [65, 200, 30, 129], "soft", "uniform", False, DROP_P),
}
REGIMES = ("soft", "peaked", "offset", "rising", "first")
BOTH_PATHS_CASE = "long_scales"          # holds a 64-token sequence: the GPU test pushes it through both kernel families


def cases():
    return list(_CASES)


def window_cases():
    return [n for n in _CASES if len(case(n).win[0])]


def long_cases():
    return [n for n in _CASES if len(case(n).ch[0])]


def source_text():
    return open(os.path.join(ER.ROOT, "ruart_amd", "csrc", "bert_train_attn.hip")).read()


def source_constants():
    """what csrc/bert_train_attn.hip states of the constants restated above: dict(tile steps, tile clamps, drop index stride, head seed
    strides, the dO scale's frexp / ldexp pairs) - the CPU test compares them, so that changing one there without the tests fails"""
    text = source_text()
    return dict(
        tile_steps=[int(x) for x in re.findall(r"for \(int [kq]t = [ks]0; [kq]t < [ks]1; [kq]t \+= (\d+)", text)],
        tile_clamps=[int(x) for x in re.findall(r"const int (?:tn|nq) = min\((\d+), [ks]1 - [kq]t\);", text)],
        drop_stride=[int(x) for x in re.findall(r"\(unsigned\)q_tok \* (\d+)u \+ \(unsigned\)\(key_tok - seq_lo\)", text)],
        head_stride=[int(x, 16) for x in re.findall(r"seed \+ \(unsigned\)h \* (0x[0-9A-Fa-f]+)u", text)],
        dsc_range=re.findall(r"frexpf\(mx, &e\);\s*// mx = m \* 2\^e, m in \[([0-9.]+), ([0-9.]+)\)\s*\n\s*dsc = ldexpf\(1\.0f, -e\);", text),
        bf16_store_is_a_cast="bf16x4_t r = {(bf16_t)v[0], (bf16_t)v[1], (bf16_t)v[2], (bf16_t)v[3]};"
                             in open(os.path.join(ER.ROOT, "ruart_amd", "csrc", "common.h")).read())


def plan(lens):
    """(cu, win (2, nw): q0 q1, ch (5, nc): q0 q1 k0 k1 first, tok_lo (T,)) as bert.PackedTokens cuts a packed stream for the 16-bit
    trainable path: whole short sequences in <= 64-token windows, every longer one in 64-token chunks against the whole sequence"""
    from ruart_amd.bert import PackedTokens
    lens = np.asarray(lens, dtype=np.int64)
    cu = np.zeros(len(lens) + 1, dtype=np.int64)
    np.cumsum(lens, out=cu[1:])
    blk, _ = PackedTokens._plan_blocks(lens, cu, mfma_long=False)
    own = (blk[0] == blk[2]) & (blk[1] == blk[3])
    win = blk[:2, own].astype(np.int64)
    ch = blk[:, ~own].astype(np.int64)
    first = np.array([int(np.nonzero(ch[0] == k0)[0][0]) for k0 in ch[2]], dtype=np.int64)
    return cu, win, np.concatenate([ch, first[None, :]], 0), np.repeat(cu[:-1], lens).astype(np.int32)


class Case:
    pass


class _Seq:
    pass


def _heads64(x, a, b, col0, heads):
    """rows a:b, columns col0 .. col0 + 64 heads of a (T, *) tensor as float64 (heads, n, 64)"""
    return x[a:b, col0:col0 + heads * 64].double().reshape(b - a, heads, 64).transpose(0, 1).contiguous()


def _rows(x):
    """(heads, n, 64) -> (n, heads * 64)"""
    return x.transpose(0, 1).reshape(x.shape[1], -1)


def _scale_of(mx):
    """the power of two that brings mx into [0.5, 1) (1 for mx = 0), float64 tensor in, float64 out"""
    _, e = torch.frexp(mx)
    return torch.where(mx > 0, torch.ldexp(torch.ones_like(mx), -e), torch.ones_like(mx))


@functools.lru_cache(maxsize=None)
def case(name):
    """inputs (f16 qkv, bf16 dO, descriptors) and the float64 reference of one case; built once and shared - do not modify"""
    heads, lens, regime, do_regime, padded, p = _CASES[name]
    c = Case()
    c.name, c.heads, c.H, c.lens, c.regime, c.do_regime, c.padded, c.p = name, heads, heads * 64, list(lens), regime, do_regime, padded, p
    c.cu, c.win, c.ch, c.tok_lo = plan(lens)
    c.T = int(c.cu[-1])
    c.ld, c.ldc, c.ldd = (3 * c.H + 8, c.H + 8, 3 * c.H + 4) if padded else (3 * c.H, c.H, 3 * c.H)
    g = torch.Generator().manual_seed(100 + sorted(_CASES).index(name))
    H, T = c.H, c.T
    q = torch.randn(T, heads, 64, generator=g) * 0.125
    k = torch.randn(T, heads, 64, generator=g)
    v = torch.randn(T, heads, 64, generator=g)
    c.long_seq = np.isin(c.cu[:-1], c.ch[2])
    if regime in ("peaked", "rising", "first"):           # Q_i = half a soft row + (12 / 64) K_j(i): score about 12 on key j(i)
        for s, n in enumerate(lens):
            a = int(c.cu[s])
            lo, hi = 0, n
            if regime == "rising":
                lo = TILE * ((n - 1) // TILE)
            elif regime == "first":
                hi = min(n, TILE)
            j = torch.randint(lo, hi, (n, heads), generator=g)
            kj = torch.gather(k[a:a + n], 0, j[:, :, None].expand(n, heads, 64))
            q[a:a + n] = 0.5 * q[a:a + n] + (12.0 / 64.0) * kj
    if regime == "offset":                                 # a common shift of a whole row's scores through column 0
        shift = torch.randn(T, heads, generator=g) * 20.0
        big = int(c.cu[int(np.argmax(lens))])
        shift[big], shift[big + 1] = 80.0, -100.0
        q[:, :, 0] = shift
        k[:, :, 0] = 1.0
    c.qkv16 = torch.cat([q.reshape(T, H), k.reshape(T, H), v.reshape(T, H)], 1).half()
    dO = (torch.randn(T, H, generator=g) * 1e-3).bfloat16().float()
    c.small_seqs, c.zero_blocks, c.tiny_blocks = [], [], []
    if do_regime == "disparity":                           # by window: 0 and the last: second sequence 2^-12 below; 1: zero; 2: about 1e-6
        nw = c.win.shape[1]
        for w in range(nw):
            q0, q1 = int(c.win[0, w]), int(c.win[1, w])
            seqs = [s for s in range(len(lens)) if q0 <= c.cu[s] < q1]
            if w in (0, nw - 1) and len(seqs) >= 2:
                s = seqs[1]
                dO[int(c.cu[s]):int(c.cu[s + 1])] *= 2.0 ** -12
                c.small_seqs.append(s)
            elif w == 1:
                dO[q0:q1] = 0.0
                c.zero_blocks.append(("win", w))
            elif w == 2:
                dO[q0:q1] *= 2.0 ** -10
                c.tiny_blocks.append(("win", w))
    elif do_regime == "scales":                            # the 512-token sequence's chunks at 2^0, 2^-6, 2^-12; a zero chunk in the 128
        for b in range(c.ch.shape[1]):
            q0, q1, k0, k1, first = (int(x) for x in c.ch[:, b])
            if k1 - k0 == 512:
                dO[q0:q1] *= 2.0 ** (-6 * ((b - first) % 3))
            elif k1 - k0 == 128 and b - first == 1:
                dO[q0:q1] = 0.0
                c.zero_blocks.append(("long", b))
    else:
        assert do_regime == "uniform"
    c.dO16 = dO.bfloat16()
    assert torch.equal(c.dO16.float(), dO)
    masks = None if p == 0 else DR.bernoulli_masks(g, p, c.cu, heads)
    return _finish(c, masks)


def with_masks(base, masks):
    """the case ``base`` with other probability multipliers (per sequence (heads, n, n) float64): the GPU tests' recovered masks"""
    c = Case()
    c.__dict__.update(base.__dict__)
    c.name = base.name + "+masks"
    return _finish(c, masks)


def as_long(base, s):
    """the case ``base`` with sequence s - a window of its own - planned as ONE chunk of the *_long kernels instead: same inputs, same
    float64 values, the long kernels' bounds for its rows"""
    a, b = int(base.cu[s]), int(base.cu[s + 1])
    w = np.nonzero((base.win[0] == a) & (base.win[1] == b))[0]
    assert len(w) == 1 and b - a <= TILE
    c = Case()
    c.__dict__.update(base.__dict__)
    c.name = "%s+seq%d_long" % (base.name, s)
    c.win = np.delete(base.win, int(w[0]), 1)
    c.ch = np.concatenate([base.ch, np.array([[a], [b], [a], [b], [base.ch.shape[1]]], dtype=np.int64)], 1)
    c.long_seq = base.long_seq.copy()
    c.long_seq[s] = True
    return _finish(c, base.masks)


def _block_scales(c, blocks):
    """(n_blocks, heads) float64: the power of two of every (block, head) of dO"""
    out = torch.ones(blocks.shape[1], c.heads, dtype=torch.float64)
    for b in range(blocks.shape[1]):
        q0, q1 = int(blocks[0, b]), int(blocks[1, b])
        out[b] = _scale_of(c.dO16[q0:q1].double().abs().reshape(q1 - q0, c.heads, 64).amax((0, 2)))
    return out


def _finish(c, masks):
    heads, H, T = c.heads, c.H, c.T
    c.masks = masks
    c.win_scale, c.ch_scale = _block_scales(c, c.win), _block_scales(c, c.ch)
    c.dsc = torch.ones(T, heads, dtype=torch.float64)                     # per query row and head
    for blocks, sc in ((c.win, c.win_scale), (c.ch, c.ch_scale)):
        for b in range(blocks.shape[1]):
            c.dsc[int(blocks[0, b]):int(blocks[1, b])] = sc[b]
    c.win_rows, c.long_rows = torch.zeros(T, dtype=torch.bool), torch.zeros(T, dtype=torch.bool)
    for b in range(c.win.shape[1]):
        c.win_rows[int(c.win[0, b]):int(c.win[1, b])] = True
    for b in range(c.ch.shape[1]):
        c.long_rows[int(c.ch[0, b]):int(c.ch[1, b])] = True
    assert bool((c.win_rows ^ c.long_rows).all())
    c.ctx = torch.zeros(T, H, dtype=torch.float64)
    c.lse2 = torch.full((T, heads), float("nan"), dtype=torch.float64)
    c.dqkv = torch.zeros(T, 3 * H, dtype=torch.float64)
    c.seq = []
    for s in range(len(c.lens)):
        r = _seq_reference(c, s)
        c.seq.append(r)
        c.ctx[r.a:r.b] = _rows(r.O)
        if r.long:
            c.lse2[r.a:r.b] = r.lse2[:, :, 0].t()
        c.dqkv[r.a:r.b] = torch.cat([_rows(r.dQ), _rows(r.dK), _rows(r.dV)], 1)
    c.bias_win, c.bias_long = _block_sums(c, c.dqkv, c.win), _block_sums(c, c.dqkv, c.ch)
    c._fb, c._bb = None, {}
    return c


def _block_sums(c, dqkv, blocks):
    """(n_blocks, 2H): the column sums of the blocks' dQ | dV rows"""
    H = c.H
    out = torch.zeros(blocks.shape[1], 2 * H, dtype=dqkv.dtype)
    for b in range(blocks.shape[1]):
        q0, q1 = int(blocks[0, b]), int(blocks[1, b])
        out[b, :H] = dqkv[q0:q1, :H].sum(0)
        out[b, H:] = dqkv[q0:q1, 2 * H:].sum(0)
    return out


def _seq_reference(c, s):
    """float64 forward and gradient formulas of sequence s, all heads: the module docstring's operation"""
    r = _Seq()
    r.s, r.a, r.b = s, int(c.cu[s]), int(c.cu[s + 1])
    r.n, r.long = r.b - r.a, bool(c.long_seq[s])
    r.nt = (r.n + TILE - 1) // TILE if r.long else 1
    H, heads = c.H, c.heads
    r.q, r.k, r.v = (_heads64(c.qkv16, r.a, r.b, i * H, heads) for i in range(3))
    r.g_un = _heads64(c.dO16, r.a, r.b, 0, heads)
    r.M = torch.ones(heads, r.n, r.n, dtype=torch.float64) if c.masks is None else c.masks[s].double()
    r.dsc = c.dsc[r.a:r.b].t().reshape(heads, r.n, 1)
    r.S = r.q @ r.k.transpose(1, 2)
    r.m = r.S.amax(-1, keepdim=True)
    e = torch.exp(r.S - r.m)
    r.L = e.sum(-1, keepdim=True)
    r.P = e / r.L
    r.Pd = r.P * r.M
    r.O = r.Pd @ r.v
    r.lse2 = (r.m + torch.log(r.L)) * LOG2E
    r.dPd = r.g_un @ r.v.transpose(1, 2)
    r.dP = r.M * r.dPd
    r.delta = (r.P * r.dP).sum(-1, keepdim=True)
    r.dS = r.P * (r.dP - r.delta)
    r.dQ, r.dK, r.dV = r.dS @ r.k, r.dS.transpose(1, 2) @ r.q, r.Pd.transpose(1, 2) @ r.g_un
    return r


def effective_keys(r):
    """median over the rows (all heads) of 1 / sum_j p_j^2, and of the largest probability"""
    return float((1.0 / (r.P ** 2).sum(-1)).median()), float(r.P.amax(-1).median())


# ------------------------------------------------------------------------------------------------------------------------------
# bounds
# ------------------------------------------------------------------------------------------------------------------------------


def gamma(n):
    return n * U32 / (1.0 - n * U32)


def _c_mult(c):
    return C_MULT if c.p > 0 else 0.0


def _forward_terms(c, r):
    """per sequence: E_s, E_P, E_Pd32 (forward's softmax) and the bounds b_ctx (heads, n, 64), b_lse2 (heads, n, 1)"""
    nt, lg = r.nt, r.long
    va = r.v.abs()
    E_s = gamma(64) * (r.q.abs() @ r.k.abs().transpose(1, 2))
    E_i = E_s.amax(-1, keepdim=True)
    sm = (r.S - r.m).abs()
    D = (r.P * sm).sum(-1, keepdim=True)
    n_sum = N_SUM + (nt if lg else 0)
    tiles = (nt - 1) * (C_EXP + 1) if lg else 0.0
    Tt = C_ARG * U32 * (sm + D) + (2 * C_EXP + n_sum + C_RCP + 1 + 2 * tiles) * U32
    assert float(Tt.max()) < T_MAX, (c.name, r.s, float(Tt.max()))
    rel = torch.expm1(2 * E_i + Tt * (1 + SECOND_ORDER))
    E_P = rel * r.P + F32_FLOOR
    E_Pd32 = r.M * (E_P + _c_mult(c) * U32 * (r.P + E_P))
    live = (r.Pd > 0).double()
    floor = F16_FLOOR * (1 + rel.amax(-1, keepdim=True)) / r.L * live if lg else F16_FLOOR * live
    E_Pd = E_Pd32 + UH * (r.Pd + E_Pd32) + floor
    pre = E_Pd @ va + gamma(64 * nt + (nt if lg else 0)) * ((r.Pd + E_Pd) @ va)
    b_ctx = pre + UH * (r.O.abs() + pre) + F16_FLOOR
    T_norm = C_ARG * U32 * D + (C_EXP + n_sum + tiles) * U32
    b_lse = LOG2E * (E_i + T_norm * (1 + SECOND_ORDER)) + 2 * U32 * LOG2E * (r.m.abs() + E_i) \
        + C_LOG * U32 * torch.log2(r.L).abs().clamp(min=1.0)
    b_lse = b_lse + U32 * (r.lse2.abs() + b_lse)
    return dict(E_s=E_s, E_P=E_P, E_Pd32=E_Pd32, b_ctx=b_ctx, b_lse2=b_lse)


def forward_bounds(c):
    """dict(ctx (T, H), lse2 (T, heads)) float64; lse2 is NaN on window tokens"""
    if c._fb is None:
        ctx = torch.zeros(c.T, c.H, dtype=torch.float64)
        lse = torch.full((c.T, c.heads), float("nan"), dtype=torch.float64)
        c._ft = []
        for r in c.seq:
            f = _forward_terms(c, r)
            c._ft.append(f)
            ctx[r.a:r.b] = _rows(f["b_ctx"])
            if r.long:
                lse[r.a:r.b] = f["b_lse2"][:, :, 0].t()
        c._fb = dict(ctx=ctx, lse2=lse)
    return c._fb


def _backward_terms(c, r, f, chained):
    """per sequence: the pre-rounding error bounds of dQ, dK, dV (heads, n, 64), module docstring"""
    nt, lg = r.nt, r.long
    qa, ka, va = r.q.abs(), r.k.abs(), r.v.abs()
    inv = 1.0 / r.dsc
    g = r.g_un * r.dsc
    ga = g.abs()
    E_g = torch.where((ga > 0) & (ga < F16_EXACT_BF16), torch.full_like(ga, F16_FLOOR), torch.zeros_like(ga))
    dPd = g @ r.v.transpose(1, 2)
    E_dPd = E_g @ va.transpose(1, 2) + gamma(64) * ((ga + E_g) @ va.transpose(1, 2))
    dP = r.M * dPd
    E_dP = r.M * (E_dPd + _c_mult(c) * U32 * (dPd.abs() + E_dPd))
    if lg:
        lse_nat = r.m + torch.log(r.L)
        e_lse = LN2 * (f["b_lse2"] if chained else U32 * r.lse2.abs() + 2.0 ** -149)
        T_L = U32 * (2 * r.S.abs() + (r.S - lse_nat).abs()) + C_EXP * U32
        assert float(T_L.max()) < T_MAX, (c.name, r.s, float(T_L.max()))
        E_P = torch.expm1(f["E_s"] + e_lse + T_L * (1 + SECOND_ORDER)) * r.P + F32_FLOOR
        n_delta = 16 * nt + 2 + 2
    else:
        E_P = f["E_P"]
        n_delta = N_SUM + 1
    E_Pd32 = r.M * (E_P + _c_mult(c) * U32 * (r.P + E_P))
    Ph, dPh = r.P + E_P, dP.abs() + E_dP
    delta = (r.P * dP).sum(-1, keepdim=True)
    E_delta = (E_P * dPh + r.P * E_dP).sum(-1, keepdim=True) + gamma(n_delta) * (Ph * dPh).sum(-1, keepdim=True)
    dS = r.P * (dP - delta)
    E_dS32 = E_P * ((dP - delta).abs() + E_dP + E_delta) + r.P * (E_dP + E_delta) + gamma(2) * Ph * (dPh + delta.abs() + E_delta)
    if r.n == 1:
        E_dS = torch.zeros_like(E_dS32)
    else:
        dSh = dS.abs() + E_dS32
        E_dS = E_dS32 + UH * dSh + F16_FLOOR * (dSh > 0).double()
    E_Pd = E_Pd32 + UH * (r.Pd + E_Pd32) + F16_FLOOR * (r.Pd > 0).double()
    dSh = dS.abs() + E_dS
    pre_q = (E_dS @ ka + gamma(64 * nt) * (dSh @ ka)) * inv
    pre_k = (E_dS * inv).transpose(1, 2) @ qa + gamma(64 + nt) * ((dSh * inv).transpose(1, 2) @ qa)
    gi, Egi = ga * inv, E_g * inv
    PdT, EPdT = r.Pd.transpose(1, 2), E_Pd.transpose(1, 2)
    pre_v = EPdT @ gi + PdT @ Egi + EPdT @ Egi + gamma(64 + nt) * ((PdT + EPdT) @ (gi + Egi))
    return pre_q, pre_k, pre_v


def _stored_bf16(x, pre):
    mag = x.abs() + pre
    return torch.where(mag > 0, pre + UB * mag + BF16_FLOOR, torch.zeros_like(mag))


def backward_bounds(c, chained=False):
    """dict(dqkv (T, 3H), bias_win (nw, 2H), bias_long (nc, 2H), pre (T, 3H): the bounds before the bf16 store) float64.  ``chained``:
    the long kernels' lse2 input is ruart_attn_train_fwd_long's own output (its bound is the input error), else the float64 lse2 in fp32"""
    if chained not in c._bb:
        forward_bounds(c)
        pre = torch.zeros(c.T, 3 * c.H, dtype=torch.float64)
        for r, f in zip(c.seq, c._ft):
            pq, pk, pv = _backward_terms(c, r, f, chained)
            pre[r.a:r.b] = torch.cat([_rows(pq), _rows(pk), _rows(pv)], 1)
        mag = c.dqkv.abs() + pre
        bias = {}
        for key, blocks in (("bias_win", c.win), ("bias_long", c.ch)):
            bias[key] = _block_sums(c, pre, blocks) + gamma(N_BIAS) * _block_sums(c, mag, blocks)
        c._bb[chained] = dict(dqkv=_stored_bf16(c.dqkv, pre), pre=pre, **bias)
    return c._bb[chained]


def ratio(got, ref, bound):
    """worst |got - ref| / bound; an error where the bound is 0 counts as infinite, a NaN anywhere as infinite"""
    err = (got.double() - ref).abs()
    if bool(torch.isnan(err).any()):
        return float("inf")
    r = torch.where(err == 0, torch.zeros_like(err), err / bound)
    return float(r.max()) if r.numel() else 0.0


def kernel_ratios(c, win_fwd=None, long_fwd=None, win_bwd=None, long_bwd=None, chained=False):
    """{"<kernel>.<output>": worst error / bound} of whatever is given, every element of the rows (and blocks) the kernel owns:
    win_fwd = ctx (T, H); long_fwd = (ctx, lse2 (T, heads)); win_bwd = (dqkv (T, 3H), bias (nw, 2H)); long_bwd = (dqkv, bias (nc, 2H)),
    bias = None for none.  The long backward's outputs are split by the kernel that writes them (dq: dQ and the query bias part;
    dkv: dK, dV and the value bias part)."""
    H, res = c.H, {}
    fb = forward_bounds(c)
    if win_fwd is not None:
        w = c.win_rows
        res["win_fwd.ctx"] = ratio(win_fwd[w], c.ctx[w], fb["ctx"][w])
    if long_fwd is not None:
        w = c.long_rows
        res["long_fwd.ctx"] = ratio(long_fwd[0][w], c.ctx[w], fb["ctx"][w])
        res["long_fwd.lse2"] = ratio(long_fwd[1][w], c.lse2[w], fb["lse2"][w])
    if win_bwd is not None:
        bb, w = backward_bounds(c), c.win_rows
        for i, nm in enumerate(("dQ", "dK", "dV")):
            sl = slice(i * H, (i + 1) * H)
            res["win_bwd." + nm] = ratio(win_bwd[0][w][:, sl], c.dqkv[w][:, sl], bb["dqkv"][w][:, sl])
        if win_bwd[1] is not None:
            res["win_bwd.bias"] = ratio(win_bwd[1], c.bias_win, bb["bias_win"])
    if long_bwd is not None:
        bb, w = backward_bounds(c, chained), c.long_rows
        for i, nm in enumerate(("dq.dQ", "dkv.dK", "dkv.dV")):
            sl = slice(i * H, (i + 1) * H)
            res[nm] = ratio(long_bwd[0][w][:, sl], c.dqkv[w][:, sl], bb["dqkv"][w][:, sl])
        if long_bwd[1] is not None:
            res["dq.bias"] = ratio(long_bwd[1][:, :H], c.bias_long[:, :H], bb["bias_long"][:, :H])
            res["dkv.bias"] = ratio(long_bwd[1][:, H:], c.bias_long[:, H:], bb["bias_long"][:, H:])
    return res


def quiet_sequence_precision(c):
    """for every sequence whose dO lies 2^-12 below its window neighbour's: {(sequence, block): (max bound / max |ref|,
    ||bound|| / ||ref||)} - what precision the derived bound leaves a quiet sequence beside a loud one (recorded, not judged)"""
    bb, H, out = backward_bounds(c), c.H, {}
    for s in c.small_seqs:
        a, b = int(c.cu[s]), int(c.cu[s + 1])
        for i, nm in enumerate(("dQ", "dK", "dV")):
            ref, bd = c.dqkv[a:b, i * H:(i + 1) * H], bb["dqkv"][a:b, i * H:(i + 1) * H]
            out[(s, nm)] = (float(bd.max() / ref.abs().max()), float(bd.norm() / ref.norm()))
    return out


# ------------------------------------------------------------------------------------------------------------------------------
# emulation of the kernels' arithmetic in fp32
# ------------------------------------------------------------------------------------------------------------------------------


def _h32(x, a, b, col0, heads):
    return x[a:b, col0:col0 + heads * 64].float().reshape(b - a, heads, 64).transpose(0, 1).contiguous()


def _k_col(c, defect):
    return c.H + (64 if defect == "next_head" else 0)      # head h reads head h + 1's key columns (the last head: V's first)


def _t16(x, bf):
    return x.to(torch.bfloat16 if bf else torch.float16).float()


def _exp2(x):
    return torch.exp2(x)


def _window_mult(c, q0, q1):
    """(heads, n, n) fp32 multiplier of a window: the sequences' masks on the diagonal blocks, 1 elsewhere (masked keys have P = 0)"""
    n = q1 - q0
    M = torch.ones(c.heads, n, n)
    if c.masks is not None:
        for s in range(len(c.lens)):
            a, b = int(c.cu[s]), int(c.cu[s + 1])
            if q0 <= a < q1:
                M[:, a - q0:b - q0, a - q0:b - q0] = c.masks[s].float()
    return M


def _window_probs(c, w, defect):
    q0, q1 = int(c.win[0, w]), int(c.win[1, w])
    n, heads, H = q1 - q0, c.heads, c.H
    Q, K, V = _h32(c.qkv16, q0, q1, 0, heads), _h32(c.qkv16, q0, q1, _k_col(c, defect), heads), _h32(c.qkv16, q0, q1, 2 * H, heads)
    lo = torch.from_numpy(c.tok_lo[q0:q1].astype(np.int64))
    same = lo[:, None] == lo[None, :]
    if defect == "window_neighbour_leak":                 # the keys of the next sequence of the window pass the mask as well
        idx = torch.searchsorted(torch.unique(lo), lo)
        same = same | (idx[None, :] == idx[:, None] + 1)
    s = torch.where(same, Q @ K.transpose(1, 2), torch.full((), -1e30))
    mx = s.amax(-1, keepdim=True)
    p = torch.where(s > -1e29, _exp2((s - mx) * LOG2E), torch.zeros(()))
    P = p * (1.0 / p.sum(-1, keepdim=True))
    return q0, q1, n, Q, K, V, P


def emulate_window_forward(c, defect=None):
    """ctx (T, H) fp32 holding f16 values; NaN where the window kernel writes nothing"""
    assert defect is None or defect in DEFECTS
    ctx = torch.full((c.T, c.H), float("nan"))
    for w in range(c.win.shape[1]):
        q0, q1, n, Q, K, V, P = _window_probs(c, w, defect)
        if c.p > 0:
            P = P * _window_mult(c, q0, q1)
        O = _rows((_t16(P, defect == "p_bf16") @ V).half().float())
        nv = n - 1 if defect == "last_query_dropped" else n
        ctx[q0:q0 + nv] = O[:nv]
    return ctx


def _emu_scale(dO, defect):
    """(heads, 1, 1) fp32 power of two of a block's dO (heads, n, 64)"""
    sc = _scale_of(dO.abs().amax((1, 2), keepdim=True))
    return torch.ones_like(sc) if defect == "do_unscaled" else sc


def emulate_window_backward(c, defect=None):
    """(dqkv (T, 3H) fp32 holding bf16 values, NaN where nothing is written; bias (nw, 2H) fp32)"""
    assert defect is None or defect in DEFECTS
    H, heads = c.H, c.heads
    dqkv = torch.full((c.T, 3 * H), float("nan"))
    bias = torch.zeros(c.win.shape[1], 2 * H)
    for w in range(c.win.shape[1]):
        q0, q1, n, Q, K, V, P = _window_probs(c, w, defect)
        nv = n - 1 if defect == "last_query_dropped" else n
        if nv < n:
            P[:, nv:] = 0.0
        dO = _h32(c.dO16, q0, q1, 0, heads)
        dsc = _emu_scale(dO, defect)
        g16 = (dO * dsc).half().float()
        D = _window_mult(c, q0, q1) if c.p > 0 else torch.ones(())
        pd = P * D
        dp_raw = g16 @ V.transpose(1, 2)
        dp = dp_raw * D
        if defect == "delta_from_ctx":
            O16 = (pd.half().float() @ V).half().float()
            delta = (g16 * O16).sum(-1, keepdim=True)
        else:
            delta = (P * dp).sum(-1, keepdim=True)
        diff = dp - delta
        if defect == "ds_product_fused":                    # fma(dPd, D, -delta): the product unrounded, delta from the rounded one
            diff = (dp_raw.double() * D.double() - delta.double()).float()
        dS16 = _t16(P * diff, defect == "ds_bf16")
        Pd16 = _t16(pd, defect == "p_bf16")
        inv = 1.0 / dsc
        dq, dk, dv = (dS16 @ K), dS16.transpose(1, 2) @ Q, Pd16.transpose(1, 2) @ g16
        out = torch.cat([_rows(dq * inv), _rows(dk * inv), _rows(dv * inv)], 1).bfloat16().float()
        dqkv[q0:q0 + nv] = out[:nv]
        if defect == "bias_after_rounding":
            bias[w] = torch.cat([out[:, :H].sum(0), out[:, 2 * H:].sum(0)])
        else:
            bias[w] = torch.cat([_rows(dq.sum(1, keepdim=True) * inv)[0], _rows(dv.sum(1, keepdim=True) * inv)[0]])
    return dqkv, bias


def _tile(x, kt, tn, col0, heads):
    """64 staged rows of a key / query tile: rows kt .. kt + tn, zeros behind"""
    t = torch.zeros(heads, TILE, 64)
    t[:, :tn] = _h32(x, kt, kt + tn, col0, heads)
    return t


def _seq_of_chunk(c, b):
    return int(np.nonzero(c.cu[:-1] == c.ch[2, b])[0][0])


def _chunk_mult(c, b, q0, n, kt, tn):
    """(heads, n, 64) fp32 multiplier of the chunk's queries against one key tile (1 behind the sequence's end)"""
    M = torch.ones(c.heads, n, TILE)
    if c.masks is not None:
        k0 = int(c.ch[2, b])
        M[:, :, :tn] = c.masks[_seq_of_chunk(c, b)][:, q0 - k0:q0 - k0 + n, kt - k0:kt - k0 + tn].float()
    return M


def emulate_long_forward(c, defect=None):
    """(ctx (T, H) fp32 holding f16 values, lse2 (T, heads) fp32); NaN where the long kernel writes nothing"""
    assert defect is None or defect in DEFECTS
    H, heads = c.H, c.heads
    ctx, lse2 = torch.full((c.T, H), float("nan")), torch.full((c.T, heads), float("nan"))
    key = torch.arange(TILE)
    for b in range(c.ch.shape[1]):
        q0, q1, k0, k1 = (int(x) for x in c.ch[:4, b])
        n = q1 - q0
        Q = _h32(c.qkv16, q0, q1, 0, heads)
        m, l, o = torch.full((heads, n, 1), -1e30), torch.zeros(heads, n, 1), torch.zeros(heads, n, 64)
        for kt in range(k0, k1, TILE):
            tn = min(TILE, k1 - kt)
            K, V = _tile(c.qkv16, kt, tn, _k_col(c, defect), heads), _tile(c.qkv16, kt, tn, 2 * H, heads)
            valid = key < (TILE if defect == "key_tail_unmasked" else tn)
            s = torch.where(valid, Q @ K.transpose(1, 2), torch.full((), -1e30))
            mn = torch.maximum(m, s.amax(-1, keepdim=True))
            alpha = _exp2((m - mn) * LOG2E)
            if defect == "alpha_skipped":
                alpha = torch.ones_like(alpha)
            p = torch.where(s > -1e29, _exp2((s - mn) * LOG2E), torch.zeros(()))
            l = l * alpha + p.sum(-1, keepdim=True)
            m = mn
            if c.p > 0:
                p = p * _chunk_mult(c, b, q0, n, kt, tn)
            o = o * alpha + _t16(p, defect == "p_bf16") @ V
        nv = n - 1 if defect == "last_query_dropped" else n
        ctx[q0:q0 + nv] = _rows((o * (1.0 / l)).half().float())[:nv]
        out = m + torch.log(l) if defect == "lse_natural" else m * LOG2E + torch.log2(l)
        lse2[q0:q0 + nv] = out[:, :nv, 0].t()
    return ctx, lse2


def emulate_long_backward(c, lse2, defect=None):
    """(dqkv (T, 3H) fp32 holding bf16 values, NaN where nothing is written; bias (nc, 2H) fp32) from lse2 (T, heads) fp32: the dQ
    kernel per chunk (delta over all key tiles first, then dS and dQ), then the dK / dV kernel per chunk against every query tile"""
    assert defect is None or defect in DEFECTS
    H, heads, nc = c.H, c.heads, c.ch.shape[1]
    dqkv = torch.full((c.T, 3 * H), float("nan"))
    bias = torch.zeros(nc, 2 * H)
    delta_ws, scale_ws = torch.zeros(c.T, heads), torch.ones(nc, heads)
    key = torch.arange(TILE)
    lse_in = lse2.float().nan_to_num(0.0)

    def probs(sc, lse, valid):
        arg = sc * LOG2E - (lse * LOG2E if defect == "lse_natural" else lse)
        return torch.where(valid, _exp2(arg), torch.zeros(()))

    for b in range(nc):
        q0, q1, k0, k1 = (int(x) for x in c.ch[:4, b])
        n = q1 - q0
        nv = n - 1 if defect == "last_query_dropped" else n
        Q = _h32(c.qkv16, q0, q1, 0, heads)
        dO = _h32(c.dO16, q0, q1, 0, heads)
        dsc = _emu_scale(dO, defect)
        g16 = (dO * dsc).half().float()
        lse = lse_in[q0:q1].t().reshape(heads, n, 1)
        qvalid = (torch.arange(n) < nv).view(1, n, 1)
        tiles = []
        delta = torch.zeros(heads, n, 1)
        for kt in range(k0, k1, TILE):
            tn = min(TILE, k1 - kt)
            K, V = _tile(c.qkv16, kt, tn, _k_col(c, defect), heads), _tile(c.qkv16, kt, tn, 2 * H, heads)
            P = probs(Q @ K.transpose(1, 2), lse, (key < tn) & qvalid)
            dp = g16 @ V.transpose(1, 2)
            if c.p > 0:
                dp = dp * _chunk_mult(c, b, q0, n, kt, tn)
            delta = delta + (P * dp).sum(-1, keepdim=True)
            tiles.append((K, P, dp))
        if defect == "delta_from_ctx":
            ctx16 = emulate_long_forward(c)[0][q0:q1].nan_to_num(0.0)
            delta = (g16 * ctx16.reshape(n, heads, 64).transpose(0, 1)).sum(-1, keepdim=True)
        dq = torch.zeros(heads, n, 64)
        for K, P, dp in tiles:
            dq = dq + _t16(P * (dp - delta), defect == "ds_bf16") @ K
        inv = 1.0 / dsc
        out = _rows(dq * inv).bfloat16().float()
        dqkv[q0:q0 + nv, :H] = out[:nv]
        delta_ws[q0:q0 + nv] = delta[:, :nv, 0].t()
        scale_ws[b] = dsc.view(heads)
        bias[b, :H] = out.sum(0) if defect == "bias_after_rounding" else _rows(dq.sum(1, keepdim=True) * inv)[0]
    for b in range(nc):
        kq0, kq1, s0, s1, first = (int(x) for x in c.ch[:, b])
        nk = kq1 - kq0
        Kc, Vc = _tile(c.qkv16, kq0, nk, _k_col(c, defect), heads), _tile(c.qkv16, kq0, nk, 2 * H, heads)
        kvalid = key < (TILE if defect == "key_tail_unmasked" else nk)
        dv, dk = torch.zeros(heads, TILE, 64), torch.zeros(heads, TILE, 64)
        for t, qt in enumerate(range(s0, s1, TILE)):
            nq = min(TILE, s1 - qt)
            nqv = nq - 1 if defect == "last_query_dropped" else nq
            dsc = scale_ws[first if defect == "dkv_first_tile_scale" else first + t].view(heads, 1, 1)
            inv = 1.0 / dsc
            Qt = _tile(c.qkv16, qt, nq, 0, heads)
            g16 = (_tile(c.dO16, qt, nq, 0, heads) * dsc).half().float()
            lse, delta = torch.zeros(heads, TILE, 1), torch.zeros(heads, TILE, 1)
            lse[:, :nq, 0], delta[:, :nq, 0] = lse_in[qt:qt + nq].t(), delta_ws[qt:qt + nq].t()
            qvalid = (torch.arange(TILE) < nqv).view(1, TILE, 1)
            P = probs(Qt @ Kc.transpose(1, 2), lse, kvalid & qvalid)
            dp = g16 @ Vc.transpose(1, 2)
            D = torch.ones(())
            if c.p > 0:
                D = torch.ones(heads, TILE, TILE)
                D[:, :nq, :nk] = c.masks[_seq_of_chunk(c, b)][:, qt - s0:qt - s0 + nq, kq0 - s0:kq0 - s0 + nk].float()
            Pd16 = _t16(P * D, defect == "p_bf16")
            dS16 = _t16(P * (D * dp - delta), defect == "ds_bf16")
            dv = dv + (Pd16.transpose(1, 2) @ g16) * inv
            dk = dk + (dS16.transpose(1, 2) @ Qt) * inv
        outk, outv = _rows(dk).bfloat16().float(), _rows(dv).bfloat16().float()
        dqkv[kq0:kq1, H:2 * H], dqkv[kq0:kq1, 2 * H:] = outk[:nk], outv[:nk]
        bias[b, H:] = outv.sum(0) if defect == "bias_after_rounding" else _rows(dv.sum(1, keepdim=True))[0]
    return dqkv, bias


def emulate(c, defect=None, chained=False):
    """every kernel the case runs, as kernel_ratios() takes them.  The long backward reads the float64 lse2 rounded to fp32, or with
    ``chained`` the emulated forward's own; a defective forward feeds only its own outputs' ratios (the backward stays controlled)"""
    out = {}
    if c.win.shape[1]:
        out["win_fwd"] = emulate_window_forward(c, defect)
        out["win_bwd"] = emulate_window_backward(c, defect)
    if c.ch.shape[1]:
        out["long_fwd"] = emulate_long_forward(c, defect)
        lse = out["long_fwd"][1] if chained else c.lse2.float()
        out["long_bwd"] = emulate_long_backward(c, lse, defect)
    return out


def defect_shows(name, defect):
    """whether ``defect`` can move a result of case ``name`` past rounding at all, read from the case's lengths, regimes and dO:
      p_bf16, ds_bf16       everywhere (every case holds a sequence of two tokens or more)
      key_tail_unmasked     a long sequence with a ragged last tile and soft or offset scores (a zero-staged key's score 0 is then an
                            ordinary or a dominant score; beside a key at 12 it stays inside the f16 terms)
      window_neighbour_leak a window of several sequences
      alpha_skipped         a long sequence where a later tile raises the maximum: every regime but "first"
      delta_from_ctx        peaked scores (peaked, rising, first).  The f16 context row's rounding puts eps = h <|dO|, |O|> into delta, a
                            common-mode error P eps of the row's dS.  The element-wise dS bound already holds h |dS| per key for dS's own
                            f16 rounding, and over a soft row of n_eff effective keys |O| - hence eps - is 1 / sqrt(n_eff) of that: an
                            element-wise bound cannot see it there; with one dominant key O = V_j and eps stands alone, because dS is
                            small (P (1 - P)) while eps is not
      dkv_first_tile_scale  a long sequence whose chunks carry different powers of two (read from the reference's scales)
      do_unscaled           a block whose LARGEST dO entry lies below f16's normal range 2^-14 (bf16 entries convert exactly down to
                            2^-17; what a block at 1e-3 loses below that is dwarfed by its other entries)
      lse_natural           a long sequence
      next_head, last_query_dropped   everywhere
      bias_after_rounding   a window that holds a single token (module docstring: everywhere else the sum's bound hides it)
      ds_product_fused      dropout on and a one-token sequence in a window: D o dPd fused into the subtraction of delta leaves the
                            product's rounding residual where dS = 0 exactly (what the window backward did before this test existed:
                            4 of a lane's 16 subtractions were contracted; csrc/bert_train_attn.hip now keeps the product rounded)"""
    c = case(name)
    has_win, has_long = c.win.shape[1] > 0, c.ch.shape[1] > 0
    if defect in ("p_bf16", "ds_bf16", "next_head", "last_query_dropped"):
        return True
    if defect == "delta_from_ctx":
        return c.regime in ("peaked", "rising", "first")
    if defect == "key_tail_unmasked":
        return has_long and c.regime in ("soft", "offset") and any(r.long and r.n % TILE for r in c.seq)
    if defect == "window_neighbour_leak":
        return any(len(np.unique(c.tok_lo[int(a):int(b)])) > 1 for a, b in zip(c.win[0], c.win[1]))
    if defect == "alpha_skipped":
        return has_long and c.regime != "first"
    if defect == "dkv_first_tile_scale":
        return any(bool((c.ch_scale[b] != c.ch_scale[int(c.ch[4, b])]).any()) for b in range(c.ch.shape[1]))
    if defect == "do_unscaled":
        tops = [float(c.dO16[int(a):int(b)].double().abs().max()) for bl in (c.win, c.ch) for a, b in zip(bl[0], bl[1])]
        return any(0 < t < F16_MIN_NORMAL for t in tops)
    if defect == "lse_natural":
        return has_long
    if defect == "bias_after_rounding":
        return any(int(b - a) == 1 for a, b in zip(c.win[0], c.win[1]))
    if defect == "ds_product_fused":
        return c.p > 0 and any(r.n == 1 for r in c.seq)
    raise KeyError(defect)


def kernels_of(name):
    c = case(name)
    return tuple(k for k in KERNELS if (c.win.shape[1] if k.startswith("win") else c.ch.shape[1]))


def control_cases():
    """(case name, defect) of every negative control that can show"""
    return [(n, d) for n in cases() for d in DEFECTS if defect_shows(n, d)]
