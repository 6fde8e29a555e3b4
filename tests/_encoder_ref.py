"""Float64 references, derived error bounds and CPU emulations of the frozen encoder's attention and row kernels (test infrastructure:
numpy / torch on the CPU, no GPU import; used by tests/test_gpu_encoder_kernels.py and proven on the CPU by tests/test_encoder_ref.py).

  formats        header_shifts() reads the fp16c exponents out of csrc/common.h; e4m3_decode / e4m3_encode are written from the format's
                 definition (1-4-3, bias 7, no infinities, 0x7f = NaN, saturating at 448), split_ref / split_decode from the comment
                 in common.h: hi = f16(v), lo8 = e4m3((v - hi) 2^SA_LO), hi8 = e4m3(v 2^SA_HI), a row of bytes = [lo8 (H) | hi8 (H)].
  attention      attention_case(layout, H, scale, in_type) -> inputs, descriptors (PackedTokens' own host plan), the float64
                 softmax(Q K^T + bias) V over every token's own sequence, and the per-element quantities of the bound:
                     S = max_j sum_d |q_d| |k_jd|      B = sum_j p_j |v_j|      vmax = max_j |v_j|      n_keys
                 attention_bound(case, kind): the element-wise bound (below).  attention_emulate(case, kind, defect): the kernel's
                 arithmetic in torch - fp32 scores, fp32 exp2 with the folded log2(e), online softmax over 64-key tiles, P rounded
                 to the kernel's type (split kernel: f16 hi + lo for every operand, three products), output rounded / split as stored;
                 ``defect`` breaks one thing on purpose (DEFECTS) to show that the bound would catch such a kernel.
  LayerNorm      layernorm_ref (float64), layernorm_fp32 (the kernel's formula and order in fp32 on the CPU), layernorm_allowance.
  ulp            ulp_of(values, type): spacing of the 16-bit type at a value (subnormal range included).

The attention bound, per output element (Q arrives pre-scaled; eps_s = 2^-20 S):
    arithmetic   ARITH_C eps_s B      fp32-class scores (split products good to 2^-22 each, fp32 accumulation over 64 terms); a score error
                                      e moves numerator and normaliser by about e each, hence ARITH_C = 2
    P rounding   u B                  16-bit kernels only, u = 2^-11 (f16) / 2^-8 (bf16): the normaliser sums the unrounded fp32 p;
                 + n_keys 2^-25 vmax  f16 only: probabilities below f16's normal range
    storage      u |ref|              16-bit output;  2^-24 |ref|  fp32 output;
                 2^-15 |ref| + 2^-21  split output decoded as ctx16 + e4m3(lo8) / 2^SA_LO (f16 half-ulp x e4m3 half-ulp, plus the e4m3
                                      subnormal half-step / 2^11)
"""
import functools
import os
import re

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# ------------------------------------------------------------------------------------------------------------------------------
# formats
# ------------------------------------------------------------------------------------------------------------------------------


def header_shifts():
    """(SA_LO, SA_HI, SW_HI, SW_LO) as csrc/common.h defines them (the library reports the same through ruart_f16c_shifts)."""
    text = open(os.path.join(ROOT, "ruart_amd", "csrc", "common.h")).read()
    v = {}
    for name in ("SA_LO", "SA_HI", "SW_HI"):
        v[name] = int(re.search(r"#define\s+RUART_C8_%s\s+(\d+)\s*$" % name, text, re.M).group(1))
    return v["SA_LO"], v["SA_HI"], v["SW_HI"], v["SA_LO"] + v["SW_HI"] - v["SA_HI"]


def _e4m3_table():
    """the 127 non-negative finite e4m3 values by code 0x00 .. 0x7e: subnormals m 2^-9 (exponent field 0), else (1 + m/8) 2^(e-7)"""
    t = np.zeros(127, dtype=np.float64)
    for c in range(127):
        e, m = c >> 3, c & 7
        t[c] = m * 2.0 ** -9 if e == 0 else (1.0 + m / 8.0) * 2.0 ** (e - 7)
    return t


E4M3 = _e4m3_table()
assert E4M3[-1] == 448.0 and E4M3[1] == 2.0 ** -9 and E4M3[8] == 2.0 ** -6


def e4m3_decode(b):
    """uint8 array -> float64 (0x7f / 0xff: NaN)"""
    b = np.asarray(b, dtype=np.uint8)
    mag = np.append(E4M3, np.nan)[b & 0x7f]
    return np.where(b & 0x80, -mag, mag)


def e4m3_encode(x):
    """float array -> uint8: round to nearest e4m3 value, ties to the even code, saturating at +-448 (the kernels clamp first)"""
    x = np.asarray(x, dtype=np.float64)
    a = np.minimum(np.abs(x), 448.0)
    hi = np.clip(np.searchsorted(E4M3, a, side="left"), 0, 126)
    lo = np.maximum(hi - 1, 0)
    dl, dh = a - E4M3[lo], E4M3[hi] - a
    code = np.where(dl < dh, lo, np.where(dh < dl, hi, np.where(lo % 2 == 0, lo, hi)))
    code = np.where(E4M3[hi] == a, hi, code)
    return (code | np.where(np.signbit(x), 0x80, 0)).astype(np.uint8)


def split_ref(x, sa_lo, sa_hi):
    """fp32 (M, K) -> (f16 (M, K), uint8 (M, 2K)): the split operand form as common.h describes it, computed in numpy / float64"""
    x = np.asarray(x, dtype=np.float32)
    with np.errstate(over="ignore", invalid="ignore"):           # (|x| > 65504: inf, as the kernels' conversion gives)
        hi = x.astype(np.float16)
        lo = x.astype(np.float64) - hi.astype(np.float64)        # exact
    return hi, np.concatenate([e4m3_encode(lo * 2.0 ** sa_lo), e4m3_encode(x.astype(np.float64) * 2.0 ** sa_hi)], 1)


def split_decode(c16, c8, H, sa_lo, sa_hi):
    """(f16 (M, >=H), bytes (M, >=2H) laid out [lo8 (H) | hi8 (H)]) -> (hi + lo8 / 2^SA_LO, hi8 / 2^SA_HI) as float64"""
    c16, c8 = np.asarray(c16), np.asarray(c8)
    fine = c16[:, :H].astype(np.float64) + e4m3_decode(c8[:, :H]) / 2.0 ** sa_lo
    return fine, e4m3_decode(c8[:, H:2 * H]) / 2.0 ** sa_hi


_FMT = {"f16": (10, -14), "bf16": (7, -126)}


def ulp_of(x, kind):
    """spacing of the 16-bit type ``kind`` at |x| (float64 array): 2^(max(floor(log2 |x|), emin) - mantissa bits)"""
    mant, emin = _FMT[kind]
    a = np.abs(np.asarray(x, dtype=np.float64))
    e = np.floor(np.log2(np.maximum(a, 2.0 ** emin)))
    return 2.0 ** (np.maximum(e, emin) - mant)


TORCH_TYPE = {"f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32, "split": torch.float32}
UNIT = {"f16": 2.0 ** -11, "bf16": 2.0 ** -8}

# ------------------------------------------------------------------------------------------------------------------------------
# attention
# ------------------------------------------------------------------------------------------------------------------------------
SHORT_LENS = [1, 3, 8, 64, 17, 2, 33, 30, 1, 63, 5]
LONG_LENS = [65, 7, 129, 130, 200, 3, 512]
MIXED_LENS = [3, 64, 70, 5, 130]
LAYOUTS = ("short", "long", "bias_short", "bias_long")
_SEED = {"short": 0, "long": 1, "bias_short": 2, "bias_long": 3, "mixed": 4}
SCALES = (0.3, 1.2)
ARITH_C = 2.0
DEFECTS = ("qk_f16", "p_f16", "tile_unmasked", "bias_shift")


def ragged_group(lens):
    """(ids, mask) of one PackedTokens group: row i keeps its first lens[i] positions"""
    L = max(lens)
    ids = torch.zeros(len(lens), L, dtype=torch.int64)
    mask = torch.zeros(len(lens), L, dtype=torch.bool)
    for i, n in enumerate(lens):
        ids[i, :n] = 5 + (torch.arange(n) * 7 + i) % 90
        mask[i, :n] = True
    return ids, mask


def layout_group(layout):
    """the PackedTokens group and its ``pack`` flag of a layout.  The bias layouts keep every position (pack=False) and turn ragged
    masks into the -10000 key bias: "bias_short" holds rows with a biased tail, a one-key row and a row whose FIRST keys are biased;
    "bias_long" rows of 192 with 100, 192 and 65 open keys (the first row's trailing 64-key tile is biased as a whole)."""
    if layout == "short":
        return ragged_group(SHORT_LENS), True
    if layout == "long":
        return ragged_group(LONG_LENS), True
    if layout == "mixed":                 # the strides cases: short windows and, for the 16-bit kernels, long blocks in one call
        return ragged_group(MIXED_LENS), True
    if layout == "bias_short":
        ids, mask = ragged_group([20, 7, 1, 13, 20])
        ids[:] = 7
        mask[3] = False
        mask[3, 3:10] = True
        return (ids, mask), False
    if layout == "bias_long":
        ids, mask = ragged_group([100, 192, 65])
        ids[:] = 7
        return (ids, mask), False
    raise KeyError(layout)


def packed_tokens(layout, mfma_long, device=None):
    """the descriptors the host really plans for a layout (ruart_amd.bert.PackedTokens; device None: host arrays only)"""
    from ruart_amd.bert import PackedTokens
    group, pack = layout_group(layout)
    return PackedTokens([group], device, pack=pack, mfma_long=mfma_long)


def host_plan(p):
    """(tok_lo, tok_hi, blk (4, nb), lblk (4, nlb)) of a PackedTokens out of its host buffer"""
    T, Tp, nb, nlb = p.T, p.Tp, p.n_blocks, p.n_long_blocks
    o = 2 * Tp
    lo, hi = p.host[o:o + T], p.host[o + T:o + 2 * T]
    o += 2 * T
    return lo.copy(), hi.copy(), p.host[o:o + 4 * nb].reshape(4, nb).copy(), p.host[o + 4 * nb:o + 4 * nb + 4 * nlb].reshape(4, nlb).copy()


def attention_reference(x, tok_lo, tok_hi, n_heads, bias=None):
    """x: (T, 3H) float64 [Q | K | V] rows, Q pre-scaled.  Returns float64 arrays ref (T, H), B (T, H), vmax (T, H), S (T, n_heads),
    n_keys (T,): softmax(Q K^T + bias) V over each token's own sequence [tok_lo, tok_hi) and the bound's ingredients."""
    T, H = x.shape[0], x.shape[1] // 3
    ref, B, vmax = (torch.zeros(T, H, dtype=torch.float64) for _ in range(3))
    S = torch.zeros(T, n_heads, dtype=torch.float64)
    nk = torch.zeros(T, dtype=torch.float64)
    s0 = 0
    while s0 < T:
        assert int(tok_lo[s0]) == s0
        s1 = int(tok_hi[s0])
        n = s1 - s0
        q, k, v = (x[s0:s1, i * H:(i + 1) * H].reshape(n, n_heads, 64).permute(1, 0, 2) for i in range(3))
        sc = q @ k.transpose(1, 2)
        if bias is not None:
            sc = sc + bias[s0:s1].double()
        P = torch.softmax(sc, -1)
        ref[s0:s1] = (P @ v).permute(1, 0, 2).reshape(n, H)
        B[s0:s1] = (P @ v.abs()).permute(1, 0, 2).reshape(n, H)
        vmax[s0:s1] = v.abs().amax(1).reshape(1, H)
        S[s0:s1] = (q.abs() @ k.abs().transpose(1, 2)).amax(-1).t()
        nk[s0:s1] = n
        s0 = s1
    return ref, B, vmax, S, nk


class AttentionCase:
    pass


@functools.lru_cache(maxsize=None)
def attention_case(layout, H, scale, in_type):
    """Inputs, plan and float64 reference of one case.  ``in_type``: "f32" (fp32 randn: the split and fp32 kernels), "f16" / "bf16" (the
    inputs are the already-rounded 16-bit values and the reference uses exactly those).  Q = randn * scale, K = V = randn * 1.2."""
    c = AttentionCase()
    c.layout, c.H, c.n_heads, c.scale, c.in_type = layout, H, H // 64, scale, in_type
    p = packed_tokens(layout, True)
    c.T, c.Tp = p.T, p.Tp
    c.tok_lo, c.tok_hi, _, _ = host_plan(p)
    c.bias = torch.from_numpy(p.bias_host.copy()) if p.bias_host is not None else None
    g = torch.Generator().manual_seed(1000 * _SEED[layout] + H + int(10 * scale))
    x = torch.randn(c.T, 3 * H, generator=g) * 1.2
    x[:, :H] *= scale / 1.2
    c.x = x.to(TORCH_TYPE[in_type]).float()                     # fp32 holding the values the kernel reads
    c.ref, c.B, c.vmax, c.S, c.n_keys = attention_reference(c.x.double(), c.tok_lo, c.tok_hi, c.n_heads, c.bias)
    return c


def attention_bound(c, kind, arith_c=ARITH_C):
    """element-wise bound (T, H) float64 of kernel kind "f16" | "bf16" | "f32" | "split" on case ``c`` (module docstring)"""
    eps_s = (2.0 ** -20 * c.S).repeat_interleave(64, dim=1)
    b = arith_c * eps_s * c.B
    if kind in UNIT:
        u = UNIT[kind]
        b = b + u * c.B + u * c.ref.abs()
        if kind == "f16":
            b = b + c.n_keys[:, None] * 2.0 ** -25 * c.vmax
    elif kind == "f32":
        b = b + 2.0 ** -24 * c.ref.abs()
    elif kind == "split":
        b = b + 2.0 ** -15 * c.ref.abs() + 2.0 ** -21
    else:
        raise KeyError(kind)
    return b


def hi8_bound(ref):
    """the hi8 half of a split row is e4m3 of the fp32 value: within one e4m3 step of it, 2^-3 relative, 2^-9 below 2^-6"""
    return torch.maximum(2.0 ** -3 * ref.abs(), torch.full_like(ref, 2.0 ** -9))


_LOG2E = float(np.float32(1.4426950408889634))


def _f16_hi_lo(t):
    hi = t.to(torch.float16).float()
    return hi, (t - hi).to(torch.float16).float()


def _fma32(a, b, c):
    """fp32 fma of tensors (a, c) with the scalar b: one rounding (the float64 intermediate holds the 48-bit product exactly)"""
    return (a.double() * b + c.double()).float()


def attention_emulate(c, kind, defect=None):
    """The kernels' arithmetic on case ``c`` in torch on the CPU (module docstring).  Returns (out, hi8): out (T, H) float64 = the stored
    result decoded (16-bit: the rounded value; split: ctx16 + lo8 / 2^SA_LO), hi8 = the decoded hi8 half (split only, else None).
    defect: None, or one of DEFECTS -
      "qk_f16"         split kernel with Q and K rounded to f16 (their low halves dropped)
      "p_f16"          split kernel with P rounded to f16 and no low half
      "tile_unmasked"  the keys past a sequence's end in its last 64-key tile are not masked: zero K / V rows with score 0 join the softmax
      "bias_shift"     the staged bias row is off by one key"""
    assert defect in (None,) + DEFECTS
    H, NH, T = c.H, c.n_heads, c.T
    out = torch.zeros(T, H, dtype=torch.float32)
    bias = c.bias
    if defect == "bias_shift" and bias is not None:
        bias = torch.roll(bias, -1)
    t16 = TORCH_TYPE[kind] if kind in UNIT else None
    s0 = 0
    while s0 < T:
        s1 = int(c.tok_hi[s0])
        n = s1 - s0
        q, k, v = (c.x[s0:s1, i * H:(i + 1) * H].reshape(n, NH, 64).permute(1, 0, 2).contiguous() for i in range(3))
        if kind == "split":
            qh, ql = _f16_hi_lo(q)
            kh, kl = _f16_hi_lo(k)
            vh, vl = _f16_hi_lo(v)
            if defect == "qk_f16":
                ql, kl = torch.zeros_like(ql), torch.zeros_like(kl)
        m = torch.full((NH, n), -1e30)
        l = torch.zeros(NH, n)
        o = torch.zeros(NH, n, 64)
        for kt in range(0, n, 64):
            tn = min(64, n - kt)
            sl = slice(kt, kt + tn)
            if kind == "split":
                s = (ql @ kh[:, sl].transpose(1, 2) + qh @ kl[:, sl].transpose(1, 2)) + qh @ kh[:, sl].transpose(1, 2)
            else:
                s = q @ k[:, sl].transpose(1, 2)
            if bias is not None:
                s = s + bias[s0 + kt:s0 + kt + tn]
            pad = 64 - tn if defect == "tile_unmasked" else 0
            if pad:
                s = torch.cat([s, torch.zeros(NH, n, pad)], -1)
            mn = torch.maximum(m, s.amax(-1))
            mn2 = mn * _LOG2E
            p = torch.exp2(_fma32(s, _LOG2E, -mn2[..., None]))
            scl = torch.exp2(m * _LOG2E - mn2)
            l = l * scl + p.sum(-1)
            p = p[..., :tn]
            if kind == "split":
                ph, pl = _f16_hi_lo(p)
                if defect == "p_f16":
                    pl = torch.zeros_like(pl)
                pv = (ph @ vl[:, sl] + pl @ vh[:, sl]) + ph @ vh[:, sl]
            elif t16 is not None:
                pv = p.to(t16).float() @ v[:, sl]
            else:
                pv = p @ v[:, sl]
            o = o * scl[..., None] + pv
            m = mn
        out[s0:s1] = (o * (1.0 / l)[..., None]).permute(1, 0, 2).reshape(n, H)
        s0 = s1
    if kind == "split":
        sa_lo, sa_hi, _, _ = header_shifts()
        h16, h8 = split_ref(out.numpy(), sa_lo, sa_hi)
        fine, coarse = split_decode(h16, h8, H, sa_lo, sa_hi)
        return torch.from_numpy(fine), torch.from_numpy(coarse)
    if t16 is not None:
        return out.to(t16).double(), None
    return out.double(), None


def defect_shows(kind, layout, defect):
    """whether ``defect`` can change anything on a case of (kind, layout) at all (a control is only required to break the bound where it
    can): the low halves exist in the split kernel only, a bias row only under pack=False, and a last key tile has keys to unmask only
    where some sequence length is no multiple of 64 (read from the plan alone: no reference is computed for this)"""
    if defect in ("qk_f16", "p_f16"):
        return kind == "split"
    if defect == "bias_shift":
        return layout.startswith("bias")
    if defect == "tile_unmasked":
        lo, hi, _, _ = host_plan(packed_tokens(layout, True))
        return bool(((hi - lo) % 64 != 0).any())
    return False


def control_cases():
    """(kind, layout, H, scale, defect) of every negative control that can show"""
    return [c + (d,) for c in attention_cases() for d in DEFECTS if defect_shows(c[0], c[1], d)]


def attention_cases():
    """(kind, layout, H, scale) of every attention case of the kernel tests"""
    out = []
    for kind, hs in (("split", (128, 192, 768)), ("f32", (128, 768)), ("f16", (128, 768)), ("bf16", (128, 768))):
        for layout in LAYOUTS:
            for H in hs:
                for scale in SCALES:
                    out.append((kind, layout, H, scale))
    return out


def in_type_of(kind):
    return kind if kind in UNIT else "f32"


# ------------------------------------------------------------------------------------------------------------------------------
# LayerNorm rows
# ------------------------------------------------------------------------------------------------------------------------------
LN_EPS = 1e-12
LN_INPUTS = ("randn", "offset30", "outlier", "exact")


def layernorm_rows(kind, rows, H, seed):
    """fp32 (rows, H) inputs: "randn" randn 2 + 0.3; "offset30" mean 30, std 1; "outlier" randn rows, row 0 with a single 400;
    "exact" row 0 all zero, row 1 (if any) constant 0.5, the rest randn (every partial sum of rows 0 / 1 is exact: out == beta)"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, H, generator=g)
    if kind == "randn":
        return x * 2 + 0.3
    if kind == "offset30":
        return x + 30.0
    if kind == "outlier":
        x[0, H // 3] = 400.0
        return x
    if kind == "exact":
        x[0] = 0.0
        if rows > 1:
            x[1] = 0.5
        return x
    raise KeyError(kind)


def layernorm_ref(x, gamma, beta, eps=LN_EPS):
    x = x.double()
    mu = x.mean(1, keepdim=True)
    var = ((x - mu) ** 2).mean(1, keepdim=True)
    return (x - mu) / torch.sqrt(var + eps) * gamma.double() + beta.double()


def layernorm_fp32(x, gamma, beta, eps=LN_EPS):
    """the kernel's formula (ln_row_finish) in its order, all fp32: mean, then the centred second moment, then 1 / sqrtf; a row with
    mean^2 > var takes the kernel's compensated mean - the sum of the centred values over H as a separate low part - and its second
    moment again, so that the out32 allowance tracks what the kernel computes on rows far from zero too"""
    H = x.shape[1]
    mean = x.sum(1, keepdim=True) / float(H)
    d = x - mean
    var = (d * d).sum(1, keepdim=True) / float(H)
    far = mean * mean > var
    mlo = torch.where(far, d.sum(1, keepdim=True) / float(H), torch.zeros_like(mean))
    d = d - mlo
    var = torch.where(far, (d * d).sum(1, keepdim=True) / float(H), var)
    rstd = 1.0 / torch.sqrt(var + torch.tensor(eps, dtype=torch.float32))
    return gamma * (d * rstd) + beta


def layernorm_allowance(cpu_out, ref):
    """(allowance, cpu_err) from ``cpu_out`` = layernorm_fp32 of the case: the kernel may be off by 4 x the worst error of the fp32 formula
    on the CPU (the wave reduction sums in another order than the CPU), with a floor of 2^-22 max|ref|"""
    cpu_err = float((cpu_out.double() - ref).abs().max())
    return max(4.0 * cpu_err, 2.0 ** -22 * float(ref.abs().max())), cpu_err


# ------------------------------------------------------------------------------------------------------------------------------
# row statistics from partial sums (ruart_rows_stats_finish)
# ------------------------------------------------------------------------------------------------------------------------------


def stats_partials(x, n_parts):
    """fp32 [rows][4][2] (sum, sumsq) partials of the rows of x over ``n_parts`` column slices, built in float64 and rounded to fp32;
    the slots >= n_parts hold NaN"""
    rows, H = x.shape
    part = torch.full((rows, 4, 2), float("nan"), dtype=torch.float32)
    edges = [H * i // n_parts for i in range(n_parts + 1)]
    for i in range(n_parts):
        blk = x[:, edges[i]:edges[i + 1]].double()
        part[:, i, 0] = blk.sum(1).float()
        part[:, i, 1] = (blk * blk).sum(1).float()
    return part


def stats_from_partials(part, n_parts, H, eps=LN_EPS):
    """(mu, rstd) float64 from the same fp32 partials: var = max(q / H - mu^2, 0)"""
    s = part[:, :n_parts, 0].double().sum(1)
    q = part[:, :n_parts, 1].double().sum(1)
    mu = s / H
    var = torch.clamp(q / H - mu * mu, min=0.0)
    return mu, 1.0 / torch.sqrt(var + eps)


def stats_var_forms_fp32(part, n_parts, H):
    """the kernel's variance before its clamp, var = q inv_h - mu mu in fp32, in the three forms a compiler may give it: both products
    rounded, q inv_h fused into the subtraction, mu mu fused into it.  Returns a (3, rows) float64 array (the test's constant row is
    chosen so that all three are negative: the clamp is then what keeps rstd finite, however the expression is contracted)."""
    p = part.numpy()
    inv_h = np.float32(1.0 / H)
    s, q = np.zeros(p.shape[0], np.float32), np.zeros(p.shape[0], np.float32)
    for k in range(n_parts):
        s, q = s + p[:, k, 0], q + p[:, k, 1]
    mu = s * inv_h
    qd, md, ih = q.astype(np.float64), mu.astype(np.float64), np.float64(inv_h)
    qh, mm = (q * inv_h).astype(np.float64), (mu * mu).astype(np.float64)
    r32 = lambda a: a.astype(np.float32).astype(np.float64)       # noqa: E731
    return np.stack([r32(qh - mm), r32(qd * ih - mm), r32(qh - md * md)])


def stats_bound(part, n_parts, H, eps=LN_EPS):
    """(|mu| bound, relative rstd bound) float64 per row, for fp32 evaluation of  mu = (sum ps) inv_h,  var = (sum pq) inv_h - mu^2,
    rstd = 1 / sqrt(var + eps)  against float64 on the same partials, with u = 2^-24:
      mu    <= np - 1 additions (u sum|ps| each at most), inv_h = fp32(1 / H) and the product: dm = (np - 1) u sum|ps| / H + 2 u |mu|
      var   the same for q (all terms positive): (np + 1) u q / H; mu^2: 2 |mu| dm + u mu^2; the subtraction: u |var|
      rstd  relative dvar / (2 (var + eps)) to first order, + 3 u for the addition of eps, the root and the division"""
    u = 2.0 ** -24
    ps, pq = part[:, :n_parts, 0].double(), part[:, :n_parts, 1].double()
    mu = ps.sum(1) / H
    qh = pq.sum(1) / H
    var = torch.clamp(qh - mu * mu, min=0.0)
    dm = (n_parts - 1) * u * ps.abs().sum(1) / H + 2 * u * mu.abs()
    dvar = (n_parts + 1) * u * qh + 2 * mu.abs() * dm + u * mu * mu + u * var
    return dm + 2.0 ** -149, dvar / (2 * (var + eps)) + 3 * u
