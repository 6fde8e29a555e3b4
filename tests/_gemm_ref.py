"""Float64 references, derived per-element bounds and CPU emulations of the encoder's dense products (csrc/gemm.hip, csrc/gemm_corr.hip;
test infrastructure: numpy / torch on the CPU, no GPU import; used by tests/test_gpu_gemm.py and proven on the CPU by
tests/test_gemm_ref.py).  The e4m3 codec, split_ref / split_decode, ulp_of, hi8_bound and header_shifts are tests/_encoder_ref.py's.

  plan       tile_of, xcd_remap, tile_group_m, tail_plan: Python restatements of csrc/gemm_shared.h / common.h (checked against the
             library's ruart_gemm_16*_tail_ws_bytes and for the properties the kernel tests rely on by tests/test_gemm_ref.py).
  plain      plain_case(dt, M, N, K, epi): operands holding 16-bit values, float64 C = epi(A W^T + bias [, residual]) and the bound's
             ingredients; plain_bound(case, slices); plain_emulate(case, defect, ...).
  fp16c      corr_case(M, N, K, epi): fp32 operands, their split forms (A16, A8 = [lo8 | hi8]; W16, W8 = [hi8 | lo8]), reference (a) = F,
             the function of the bytes the kernel computes, reference (b) = the product of the unrounded operands, S over the three
             decoded products; corr_bound (kernel against (a)), format_bound (F against (b)); corr_emulate(case, defect, ...).

The bound of a product, per output element, with u = 2^-24, S = sum_k |a_ik| |w_jk| (fp16c: over the three decoded products, the fp8
ones at their 2^-SHIFT), pre = the float64 pre-activation sum + bias:
    accumulation   ACC_C n u S         n = the fp32 roundings a sum can pass through: one per product (K; fp16c: 3 K, the fp8 phase adds
                                       its 2 K products to the same accumulators) + the slices of a split tile.  ACC_C = 2 allows for the
                                       rounding inside the matrix unit, which nobody has measured here; it was fixed before any GPU run.
    epilogue       u (S + |bias|)      v = acc + bias: one rounding of a value no larger than S + |bias|
                   u (S + |bias| + |res|)   v += residual (a 16-bit residual converts to fp32 exactly): one more rounding
    GELU           1.13 x (the two lines above)        max |gelu'| = 1.13 (at |x| = sqrt 2)
                   + GELU_APPROX[form]  the approximation + fp32 evaluation error of the kernel's formula against erf-GELU in float64,
                                        measured on |x| <= 12 by measure_gelu (test_gemm_ref.py asserts the constants used here)
                   + 2^-22 |g|          v_exp_f32 and v_rcp_f32 are 1 ulp by the ISA document; nobody has measured them here
    storage        16-bit: ulp_of(|ref| + bound) / 2;  fp32: u |ref|;  split (C16 + lo8 / 2^SA_LO): 2^-15 |ref| + 2^-21;
                   hi8 half: hi8_bound(ref) + 1.125 x the bound above (one e4m3 step of a value that is itself off by the bound)

The format bound of the fp16c product, F against (b) (a property of the number format, not of the kernel).  Write a = a16 + ra,
w = w16 + rw with ra, rw the exact f16 rounding residuals.  Then a w = a16 w16 + ra w16 + a rw EXACTLY - the hi8 byte of an activation
encodes a itself, not a16, so the product hi8 . w_lo8 carries a16 rw AND the ra rw term a split into two f16 halves would drop.  The
kernel's two fp8 products stand for ra w16 and a rw with every factor rounded to e4m3:
    e(x) = 2^-4 |x| + 2^-10 + max(|x| - 448, 0)       |e4m3(x) - x| <= e(x): half a step of 2^-3 relative for normal numbers, half the
                                                      subnormal step 2^-9 below 2^-6 (underflow), the excess over 448 (saturation)
    factor errors   E_alo = e(ra 2^SA_LO) / 2^SA_LO    E_whi = e(w16 2^SW_HI) / 2^SW_HI    E_ahi = e(a 2^SA_HI) / 2^SA_HI    E_wlo = e(rw 2^SW_LO) / 2^SW_LO
    |x' y' - x y| <= |x| Ey + Ex |y| + Ex Ey, summed over k:
    format bound = |ra| E_whi^T + E_alo |w16|^T + E_alo E_whi^T  +  |a| E_wlo^T + E_ahi |rw|^T + E_ahi E_wlo^T
The leading part is 2^-3 (|ra| |w16| + |a| |rw|) <= 2^-13 sum |a| |w| (|ra| <= 2^-11 |a|, |rw| <= 2^-11 |w|); the absolute underflow terms are,
per k, 2^-10-SA_LO |w16| + 2^-10-SW_HI |ra| (first product) and 2^-10-SA_HI |rw| + 2^-10-SW_LO |a| (second): 2^-21 |w16| + 2^-17 |ra| + 2^-10 |rw| +
2^-28 |a| at the shipped exponents (11, 0, 7, 18); saturation enters for |a| > 448 or |w16| > 3.5 only.
"""
import functools
import math

import numpy as np
import torch

from tests import _encoder_ref as E

U = 2.0 ** -24
ACC_C = 2.0
GELU_SLOPE = 1.13
# measured by measure_gelu (fp32 numpy evaluation of the kernels' formulas against erf-GELU in float64, |x| <= 12); test_gemm_ref.py
# re-measures them and asserts that these cover the measurement and stay under the figures the kernel sources quote
GELU_APPROX = {"pk": 3.43e-6, "pk_d": 6.9e-6, "erfc7": 3.9e-7}
EPIS = ("plain", "gelu", "gelu_f32", "res16_out_f32", "res_f32_out16")
PLAIN_SHAPES = ((128, 384, 64), (256, 256, 192), (256, 256, 128), (512, 768, 256), (1280, 512, 256))
SPLIT_SHAPES = ((1280, 256, 768, 4), (1280, 768, 2048, 10), (1280, 256, 256, 4))           # (M, N, K, cus) of the tail-split cases
LEFT_ALONE = (512, 256, 256, 4)                                                             # 2 tiles <= 4 CUs: one partial round
CORR_SHAPES = ((256, 256, 128), (512, 768, 256), (1280, 512, 768))
CORR_EPIS = ("plain", "res", "gelu")
SEL_SHAPE = {256: (512, 768, 256), 768: (1280, 512, 768)}          # the on-device negative control (ruart_gemm_16c_nt_sel), by K

# ------------------------------------------------------------------------------------------------------------------------------
# the plan: csrc/gemm_shared.h and common.h restated
# ------------------------------------------------------------------------------------------------------------------------------


def xcd_remap(bid, nwg):
    q, r, xcd = nwg >> 3, nwg & 7, bid & 7
    base = xcd * (q + 1) if xcd < r else r * (q + 1) + (xcd - r) * q
    return base + (bid >> 3)


def tile_of(i, ntm, ntn, order):
    """(tm, tn) of logical tile i under the GROUP_M walk (order 0: row-major)"""
    if order == 0:
        return i // ntn, i % ntn
    per_group = order * ntn
    g = i // per_group
    first = g * order
    gsz = min(ntm - first, order)
    r = i - g * per_group
    return first + r % gsz, r // gsz


def tile_group_m(row_tiles, col_tiles, K, precise):
    g = 8
    if precise:
        if col_tiles >= 8:
            g = 8 if K >= 1024 else 16
        elif K >= 2048:
            g = 6
    if row_tiles < 96 and not precise:
        g = 4
    return g


def tail_plan(tiles, kt, cus, even_S):
    """(n_full, r, S): tiles [0, n_full) whole, the last r in S slices each (r == 0: no split).  kt: K-tiles of a whole tile in the
    kernel's unit (K / 64 plain, 2 K / 64 fp16c, which also wants S even)."""
    if cus <= 0 or tiles <= cus:
        return tiles, 0, 0
    r = tiles % cus
    long_kt = 64 if even_S else 32
    if r == 0 or (4 * r > cus and not (5 * r <= 3 * cus and kt >= long_kt)):
        return tiles, 0, 0
    step = 2 if even_S else 1
    S = min(cus // r, 8)
    S -= S % step
    while S >= 2 and (kt % S != 0 or (kt // S) % 2 != 0 or kt // S < 2):
        S -= step
    if S < 2:
        return tiles, 0, 0
    return tiles - r, r, S


def tail_bytes(plan):
    return plan[1] * plan[2] * 256 * 256 * 4


def plain_plan(M, N, K, cus):
    return tail_plan((M // 256) * (N // 256), K // 64, cus, False)


def corr_plan(M, N, K, cus):
    return tail_plan((M // 256) * (N // 256), 2 * (K // 64), cus, True)


def plain_walk(M, N, K):
    """(tile, GROUP_M) of the kernel launch_one (gemm.hip) picks at the default variant and tile-order setting: the four-phase 256 kernel
    takes the per-problem rule, the two-stage 256 kernel and the 128 kernel the fixed default of 8"""
    if M % 256 == 0 and N % 256 == 0:
        return (256, tile_group_m(M // 256, N // 256, K, False)) if K % 128 == 0 else (256, 8)
    return 128, 8


def split_tiles(M, N, plan, order):
    """(tm, tn) of the tiles a plan cuts into slices: logical tiles n_full .. n_full + r - 1 of the walk"""
    n_full, r, _ = plan
    return [tile_of(n_full + q, M // 256, N // 256, order) for q in range(r)]


# ------------------------------------------------------------------------------------------------------------------------------
# GELU: the kernels' formulas in fp32 numpy
# ------------------------------------------------------------------------------------------------------------------------------
_F = np.float32


def gelu_erf64(x):
    x = np.asarray(x, dtype=np.float64)
    return x * 0.5 * (1.0 + torch.erf(torch.from_numpy(x / math.sqrt(2.0))).numpy())


def gelu_d64(x):
    x = np.asarray(x, dtype=np.float64)
    return 0.5 * (1.0 + torch.erf(torch.from_numpy(x / math.sqrt(2.0))).numpy()) + x * np.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


_PK = [_F(-3.228988589e-06), _F(8.823813550e-05), _F(3.602745419e-04), _F(-1.052266881e-01), _F(-2.302045345e+00)]


def _pk_logit(x, fused):
    """p(x) of gelu_pk in fp32: products and sums rounded one by one, or - ``fused`` - each p x2 + c as one fma (the compiler may
    contract them)"""
    x2 = x * x
    p = _PK[0]
    for c in _PK[1:]:
        p = (p.astype(np.float64) * x2.astype(np.float64) + np.float64(c)).astype(np.float32) if fused else (p * x2 + c).astype(np.float32)
    return (p * x).astype(np.float32), x2


def gelu_pk32(x, fused=False):
    """gelu_pk (gemm_shared.h): x / (1 + exp2(p(x)))"""
    x = np.asarray(x, dtype=np.float32)
    with np.errstate(over="ignore", invalid="ignore"):          # (an infinite input - a control's - gives NaN, as in the kernel)
        p, _ = _pk_logit(x, fused)
        r = (_F(1.0) / (_F(1.0) + np.exp2(p))).astype(np.float32)
        return (x * r).astype(np.float32)


def gelu_fwd_bwd32(x, fused=False):
    """gelu_fwd_bwd_pk: (g, dg/dx) = (x cdf, cdf + x phi 0.3989...)"""
    x = np.asarray(x, dtype=np.float32)
    with np.errstate(over="ignore"):
        p, x2 = _pk_logit(x, fused)
        cdf = (_F(1.0) / (_F(1.0) + np.exp2(p))).astype(np.float32)
        phi = np.exp2((x2 * _F(-0.72134752044)).astype(np.float32)).astype(np.float32)
    return (x * cdf).astype(np.float32), (cdf + ((x * phi).astype(np.float32) * _F(0.3989422804)).astype(np.float32)).astype(np.float32)


_E7 = [8.470145706e-06, -5.390352871e-05, -4.212367312e-04, 7.389273853e-03, -5.269111326e-02, -4.591531477e-01, -1.151110943e+00,
       -9.999998964e-01]


def gelu_erfc732(x):
    """gelu_erfc7 (gemm_corr.hip): max(x, 0) - |x| exp2(P7(min(|x|, 7.07...))), every step one fp32 fma"""
    x = np.asarray(x, dtype=np.float32)
    a = np.minimum(np.abs(x), _F(7.0710678)).astype(np.float64)
    p = np.float64(_F(_E7[0]))
    for c in _E7[1:]:
        p = (p * a + np.float64(_F(c))).astype(np.float32).astype(np.float64)
    r = np.exp2(p.astype(np.float32)).astype(np.float64)
    with np.errstate(invalid="ignore"):
        return (-np.abs(x).astype(np.float64) * r + np.maximum(x, _F(0.0)).astype(np.float64)).astype(np.float32)


def gelu_tanh64(x):
    x = np.asarray(x, dtype=np.float64)
    return 0.5 * x * (1.0 + np.tanh(math.sqrt(2.0 / math.pi) * (x + 0.044715 * x ** 3)))


def measure_gelu():
    """max |formula in fp32 - float64| over a dense grid of |x| <= 12: {"pk": gelu_pk, "pk_d": the derivative of gelu_fwd_bwd_pk,
    "erfc7": gelu_erfc7}"""
    x = np.concatenate([np.linspace(-12.0, 12.0, 1200001), np.random.RandomState(0).randn(200000) * 2.0]).astype(np.float32)
    x = x[np.abs(x) <= 12.0]
    g64, d64 = gelu_erf64(x.astype(np.float64)), gelu_d64(x.astype(np.float64))
    out = {"pk": 0.0, "pk_d": 0.0}
    for fused in (False, True):
        out["pk"] = max(out["pk"], float(np.abs(gelu_pk32(x, fused).astype(np.float64) - g64).max()))
        g, d = gelu_fwd_bwd32(x, fused)
        out["pk"] = max(out["pk"], float(np.abs(g.astype(np.float64) - g64).max()))
        out["pk_d"] = max(out["pk_d"], float(np.abs(d.astype(np.float64) - d64).max()))
    out["erfc7"] = float(np.abs(gelu_erfc732(x).astype(np.float64) - g64).max())
    return out


# ------------------------------------------------------------------------------------------------------------------------------
# the plain 16-bit product
# ------------------------------------------------------------------------------------------------------------------------------
class Case:
    pass


def _operand_a(M, K, g):
    """randn rows, one in ten of 4 x the magnitude"""
    return torch.randn(M, K, generator=g) * (1.0 + 3.0 * (torch.rand(M, 1, generator=g) > 0.9))


@functools.lru_cache(maxsize=None)
def plain_case(dt, M, N, K, epi):
    """dt "bf16" | "f16"; epi one of EPIS.  A, W, res16 hold values of the 16-bit type (as fp32 tensors); bias and res32 are fp32."""
    c = Case()
    c.dt, c.M, c.N, c.K, c.epi = dt, M, N, K, epi
    t16 = E.TORCH_TYPE[dt]
    g = torch.Generator().manual_seed(7 * M + 3 * N + K + EPIS.index(epi))
    c.A = _operand_a(M, K, g).to(t16).float()
    c.W = (torch.randn(N, K, generator=g) * 0.05).to(t16).float()
    c.bias = torch.randn(N, generator=g)
    c.bias[3::16] *= 100.0                     # (some large entries: their 16-bit rounding is what the bias_16 / res_16 controls are about)
    c.res = None
    if epi == "res16_out_f32":
        c.res = torch.randn(M, N, generator=g).to(t16).float()
    elif epi == "res_f32_out16":
        c.res = torch.randn(M, N, generator=g)
        c.res[:, 5::16] *= 100.0
    c.out = "f32" if epi in ("gelu_f32", "res16_out_f32") else dt
    c.gelu = epi.startswith("gelu")
    c.pre = c.A.double() @ c.W.double().t() + c.bias.double()
    c.S = c.A.double().abs() @ c.W.double().abs().t()
    if c.gelu:
        c.ref = torch.from_numpy(gelu_erf64(c.pre.numpy()))
    elif c.res is not None:
        c.ref = c.pre + c.res.double()
    else:
        c.ref = c.pre
    return c


def _pre_bound(S, bias, res, n):
    b = ACC_C * n * U * S + U * (S + bias.double().abs())
    if res is not None:
        b = b + U * (S + bias.double().abs() + res.double().abs())
    return b


def _store_bound(ref, b, out):
    if out == "f32":
        return b + U * ref.abs()
    return b + torch.from_numpy(0.5 * E.ulp_of((ref.abs() + b).numpy(), out))


def plain_bound(c, slices=0, form="pk"):
    """element-wise bound (M, N) float64 of the kernel's stored output against c.ref; ``slices``: the K slices of a split tile (counted for
    every element: the tiles a plan leaves whole are held to the same, slightly wider, bound)"""
    b = _pre_bound(c.S, c.bias, c.res, c.K + slices)
    if c.gelu:
        b = GELU_SLOPE * b + GELU_APPROX[form] + 2.0 ** -22 * c.ref.abs()
    return _store_bound(c.ref, b, c.out)


PLAIN_DEFECTS = ("chunk_drop", "bias_16", "res_16", "walk_partial_group", "slice_twice", "slice_missing", "gelu_tanh")


def _ktile_sums(A, W, k0, k1):
    """sum over the 64-wide K-tiles [k0, k1) in tile order, fp32"""
    acc = torch.zeros(A.shape[0], W.shape[0])
    for t in range(k0, k1):
        acc = acc + A[:, 64 * t:64 * t + 64] @ W[:, 64 * t:64 * t + 64].t()
    return acc


def _round_out(v, out):
    return v.double() if out == "f32" else v.to(E.TORCH_TYPE[out]).double()


def plain_emulate(c, defect=None, plan=None, order=0):
    """The kernels' arithmetic in torch fp32 on the CPU: K-tiles of 64 in order, a split tile (``plan`` = (n_full, r, S), ``order`` = the
    GROUP_M of the walk) as S slice sums added in slice order, then bias, GELU (gelu_pk's formula), residual, the store's rounding.
    defect (PLAIN_DEFECTS):
      chunk_drop          k-values 8 .. 15 of the last K-tile missing from the last 256-row (128 in the 128-tile kernel) tile
      bias_16 / res_16    bias / fp32 residual rounded to the operand type before the add
      walk_partial_group  the walk treats the last, partial GROUP_M group as full (gsz = order): some of its ids land past the last row
                          panel and the tiles they stood for are never written (they hold 0 here)
      slice_twice / slice_missing   the first split tile adds its first slice twice / omits its last slice
      gelu_tanh           tanh-form GELU"""
    assert defect is None or defect in PLAIN_DEFECTS
    M, N, K = c.M, c.N, c.K
    nt = K // 64
    t16 = E.TORCH_TYPE[c.dt]
    acc = _ktile_sums(c.A, c.W, 0, nt)
    tile = 256 if (M % 256 == 0 and N % 256 == 0) else 128
    if plan is not None and plan[1] > 0:
        n_full, r, S = plan
        L = nt // S
        for q, (tm, tn) in enumerate(split_tiles(M, N, plan, order)):
            rows, cols = slice(256 * tm, 256 * tm + 256), slice(256 * tn, 256 * tn + 256)
            parts = [_ktile_sums(c.A[rows], c.W[cols], s * L, s * L + L) for s in range(S)]
            if q == 0 and defect == "slice_twice":
                parts.insert(1, parts[0])
            if q == 0 and defect == "slice_missing":
                parts.pop()
            tot = torch.zeros(256, 256)
            for p in parts:
                tot = tot + p
            acc[rows, cols] = tot
    if defect == "chunk_drop":
        rows, cols, ks = slice(M - tile, M), slice(N - tile, N), slice(64 * (nt - 1) + 8, 64 * (nt - 1) + 16)
        acc[rows, cols] = acc[rows, cols] - c.A[rows, ks] @ c.W[cols, ks].t()
    bias = c.bias.to(t16).float() if defect == "bias_16" else c.bias
    v = acc + bias
    if c.gelu:
        v = torch.from_numpy(gelu_tanh64(v.double().numpy())).float() if defect == "gelu_tanh" else torch.from_numpy(gelu_pk32(v.numpy()))
    if c.res is not None:
        v = v + (c.res.to(t16).float() if defect == "res_16" else c.res)
    out = _round_out(v, c.out)
    if defect == "walk_partial_group":
        ntm, ntn = M // tile, N // tile
        reached = set()
        for i in range(ntm * ntn):
            g = i // (order * ntn)
            r = i - g * order * ntn
            reached.add((g * order + r % order, r // order))              # tile_of with gsz = order
        out = out.clone()
        for tm in range(ntm):
            for tn in range(ntn):
                if (tm, tn) not in reached:
                    out[tile * tm:tile * tm + tile, tile * tn:tile * tn + tile] = 0.0
    return out


def plain_defect_shows(c, defect, plan=None, order=0):
    """whether ``defect`` can change anything on the case at all (a control is only required to break the bound where it can)"""
    if defect in ("chunk_drop", "bias_16"):
        return True
    if defect == "res_16":
        return c.epi == "res_f32_out16"
    if defect == "walk_partial_group":
        tile = 256 if (c.M % 256 == 0 and c.N % 256 == 0) else 128
        return order > 0 and (c.M // tile) % order != 0 and c.N // tile > 1
    if defect in ("slice_twice", "slice_missing"):
        return plan is not None and plan[1] > 0
    if defect == "gelu_tanh":
        if not c.gelu:
            return False
        d = torch.from_numpy(np.abs(gelu_tanh64(c.pre.numpy()) - gelu_erf64(c.pre.numpy())))
        return bool((d > 2.0 * plain_bound(c)).any())          # (exceeds the bound even with the faithful kernel's error against it)
    return False


# ------------------------------------------------------------------------------------------------------------------------------
# the fp16c product
# ------------------------------------------------------------------------------------------------------------------------------
EDGE_ROW = (0.0, 1e-6, -1e-4, 90.0, -440.0, 3e-3, 1.0, -1.0)         # the range edges of the fp8 halves (test_gemm_16c_fp8_correction)


def weight_split_ref(w):
    """fp32 (N, K) -> (f16 (N, K), uint8 (N, 2K)) = [e4m3(w16 2^SW_HI) | e4m3((w - w16) 2^SW_LO)] (common.h), in numpy / float64"""
    _, _, sw_hi, sw_lo = E.header_shifts()
    w = np.asarray(w, dtype=np.float32)
    hi = w.astype(np.float16)
    lo = w.astype(np.float64) - hi.astype(np.float64)
    return hi, np.concatenate([E.e4m3_encode(hi.astype(np.float64) * 2.0 ** sw_hi), E.e4m3_encode(lo * 2.0 ** sw_lo)], 1)


@functools.lru_cache(maxsize=None)
def corr_case(M, N, K, epi):
    """epi "plain" | "res" | "gelu".  Row 0 of A starts with EDGE_ROW; one row in ten has 4 x the magnitude."""
    c = Case()
    c.M, c.N, c.K, c.epi = M, N, K, epi
    sa_lo, sa_hi, sw_hi, sw_lo = E.header_shifts()
    shift = sa_lo + sw_hi
    g = torch.Generator().manual_seed(11 * M + 5 * N + K + CORR_EPIS.index(epi))
    A = _operand_a(M, K, g)
    A[0, :8] = torch.tensor(EDGE_ROW)
    W = torch.randn(N, K, generator=g) * 0.03
    # Coherent rows.  On random operands a missing correction term is a random walk, sqrt(K) 2^-12 |a| |w|, and stays inside ANY bound that
    # is linear in K - at K = 768 the accumulation term alone, 2 x 3 K x 2^-24 S = 2^-12 S, is the f16 product's own error level.  The
    # correction matters most where the rounding residuals line up, and there the controls can show: row 1 of A and of W hold one positive
    # value 0.49 ulp above an f16 number (every ra, rw of the same sign), row 2 of W the f16 number itself (rw = 0).
    A[1::256] = 1.0 + 0.49 * 2.0 ** -10          # (row 1 / 2 of every 256-row tile: a split tile has them too)
    W[1::256] = 2.0 ** -5 * (1.0 + 0.49 * 2.0 ** -10)
    W[2::256] = 2.0 ** -5
    c.A, c.W = A, W
    c.bias = torch.randn(N, generator=g) * 0.1
    c.bias[3::16] *= 1000.0                    # (some large entries: bias_16 / res_16 must be able to show at fp32 precision;
    c.bias.clamp_(-200.0, 200.0)               # a GELU output stays below the 448 of its hi8 byte)
    c.res = None
    if epi == "res":
        c.res = torch.randn(M, N, generator=g)
        c.res[:, 5::16] *= 100.0
    c.gelu = epi == "gelu"
    c.out = "split" if c.gelu else "f32"
    c.A16, c.A8 = E.split_ref(A.numpy(), sa_lo, sa_hi)
    c.W16, c.W8 = weight_split_ref(W.numpy())
    a16, w16 = torch.from_numpy(c.A16.astype(np.float64)), torch.from_numpy(c.W16.astype(np.float64))
    a8, w8 = torch.from_numpy(E.e4m3_decode(c.A8)), torch.from_numpy(E.e4m3_decode(c.W8))
    c.a16f, c.w16f, c.a8f, c.w8f = a16.float(), w16.float(), a8.float(), w8.float()
    sc = 2.0 ** -shift
    c.pre_a = a16 @ w16.t() + sc * (a8 @ w8.t()) + c.bias.double()                    # (a): F
    c.S = a16.abs() @ w16.abs().t() + sc * (a8.abs() @ w8.abs().t())
    c.pre_b = A.double() @ W.double().t() + c.bias.double()                           # (b): the unrounded operands
    # the format bound (module docstring)
    e = lambda x: 2.0 ** -4 * x.abs() + 2.0 ** -10 + torch.clamp(x.abs() - 448.0, min=0.0)       # noqa: E731
    a, w = A.double(), W.double()
    ra, rw = a - a16, w - w16
    e_alo, e_whi = e(ra * 2.0 ** sa_lo) / 2.0 ** sa_lo, e(w16 * 2.0 ** sw_hi) / 2.0 ** sw_hi
    e_ahi, e_wlo = e(a * 2.0 ** sa_hi) / 2.0 ** sa_hi, e(rw * 2.0 ** sw_lo) / 2.0 ** sw_lo
    c.fmt = (ra.abs() @ e_whi.t() + e_alo @ w16.abs().t() + e_alo @ e_whi.t()
             + a.abs() @ e_wlo.t() + e_ahi @ rw.abs().t() + e_ahi @ e_wlo.t())

    def fin(pre):
        if c.gelu:
            return torch.from_numpy(gelu_erf64(pre.numpy()))
        return pre + c.res.double() if c.res is not None else pre
    c.ref_a, c.ref_b = fin(c.pre_a), fin(c.pre_b)
    return c


def corr_bound(c, slices=0, against="a"):
    """element-wise bound of the decoded output (fp32, or C16 + lo8 / 2^SA_LO) against reference (a) = F, or - ``against`` "b" - against
    the product of the unrounded operands: (a)'s bound plus the format bound, through the GELU's slope where there is one"""
    b = _pre_bound(c.S, c.bias, c.res, 3 * c.K + slices)
    ref = c.ref_a
    if against == "b":
        b = b + c.fmt
        ref = c.ref_b
    if c.gelu:
        b = GELU_SLOPE * b + GELU_APPROX["erfc7"] + 2.0 ** -22 * ref.abs()
        return b + 2.0 ** -15 * ref.abs() + 2.0 ** -21
    return b + U * ref.abs()


def corr_hi8_bound(c, slices=0):
    b = _pre_bound(c.S, c.bias, c.res, 3 * c.K + slices)
    b = GELU_SLOPE * b + GELU_APPROX["erfc7"] + 2.0 ** -22 * c.ref_a.abs()
    return E.hi8_bound(c.ref_a) + 1.125 * b


CORR_DEFECTS = ("chunk_drop", "bias_16", "res_16", "slice_twice", "slice_missing", "corr_a_only", "corr_w_only", "corr_none", "corr_scale",
                "gelu_tanh")
_CORR_SEL = {"corr_none": 0, "corr_a_only": 1, "corr_w_only": 2}


def _corr_ktile(c, rows, cols, t, scale):
    """K-tile t of the kernel's 2 K / 64 + ... stream over rows x cols: t < K / 64 the f16 phase, then the fp8 phase over 128-byte tiles"""
    nt = c.K // 64
    if t < nt:
        return c.a16f[rows, 64 * t:64 * t + 64] @ c.w16f[cols, 64 * t:64 * t + 64].t()
    t -= nt
    return (c.a8f[rows, 128 * t:128 * t + 128] @ c.w8f[cols, 128 * t:128 * t + 128].t()) * scale


def corr_emulate(c, defect=None, plan=None, order=0, corr=3):
    """The fp16c kernel's arithmetic in torch fp32 on the CPU: the f16 K-tiles in order, then the fp8 tiles (a_lo8 . w_hi8 over the first
    K bytes, a_hi8 . w_lo8 over the second) at 2^-SHIFT into the same sums; split tiles as slice sums in slice order; bias, residual or
    GELU (gelu_erfc7's formula) and the store.  Returns (out, hi8): the decoded output and - GELU - the decoded hi8 half.
    ``corr`` 0 / 1 / 2 / 3: ruart_gemm_16c_nt_sel's subsets of the correction terms (the corr_* defects set it)."""
    assert defect is None or defect in CORR_DEFECTS
    sa_lo, sa_hi, sw_hi, _ = E.header_shifts()
    corr = _CORR_SEL.get(defect, corr)
    scale = 2.0 ** -(sa_lo + sw_hi - 1) if defect == "corr_scale" else 2.0 ** -(sa_lo + sw_hi)
    M, N, K = c.M, c.N, c.K
    nt = K // 64
    f8 = {0: [], 1: list(range(nt, nt + nt // 2)), 2: list(range(nt + nt // 2, 2 * nt)), 3: list(range(nt, 2 * nt))}[corr]
    stream = list(range(nt)) + f8
    everything, all_cols = slice(0, M), slice(0, N)
    acc = torch.zeros(M, N)
    for t in stream:
        acc = acc + _corr_ktile(c, everything, all_cols, t, scale)
    if plan is not None and plan[1] > 0:
        assert corr == 3
        n_full, r, S = plan
        L = 2 * nt // S
        for q, (tm, tn) in enumerate(split_tiles(M, N, plan, order)):
            rows, cols = slice(256 * tm, 256 * tm + 256), slice(256 * tn, 256 * tn + 256)
            parts = []
            for s in range(S):
                p = torch.zeros(256, 256)
                for t in range(s * L, s * L + L):
                    p = p + _corr_ktile(c, rows, cols, t, scale)
                parts.append(p)
            if q == 0 and defect == "slice_twice":
                parts.insert(1, parts[0])
            if q == 0 and defect == "slice_missing":
                parts.pop()
            tot = torch.zeros(256, 256)
            for p in parts:
                tot = tot + p
            acc[rows, cols] = tot
    if defect == "chunk_drop":
        rows, cols, ks = slice(M - 256, M), slice(N - 256, N), slice(64 * (nt - 1) + 8, 64 * (nt - 1) + 16)
        acc[rows, cols] = acc[rows, cols] - c.a16f[rows, ks] @ c.w16f[cols, ks].t()
    v = acc + (c.bias.half().float() if defect == "bias_16" else c.bias)
    if c.gelu:
        v = torch.from_numpy(gelu_tanh64(v.double().numpy())).float() if defect == "gelu_tanh" else torch.from_numpy(gelu_erfc732(v.numpy()))
        h16, h8 = E.split_ref(v.numpy(), sa_lo, sa_hi)
        fine, coarse = E.split_decode(h16, h8, N, sa_lo, sa_hi)
        return torch.from_numpy(fine), torch.from_numpy(coarse)
    if c.res is not None:
        v = v + (c.res.half().float() if defect == "res_16" else c.res)
    return v.double(), None


def corr_defect_shows(c, defect, plan=None):
    if defect in ("chunk_drop", "bias_16", "corr_scale"):
        return True
    if defect == "res_16":
        return c.res is not None
    if defect in ("slice_twice", "slice_missing"):          # (the last slice of an fp16c tile is fp8 K-tiles only, a part of the correction:
        return plan is not None and plan[1] > 0            # the coherent rows of every 256-row tile are what lets its absence show)
    if defect in ("corr_a_only", "corr_w_only", "corr_none"):       # (the entry point refuses the half products at other K, and
        return plan is None and (defect == "corr_none" or c.K % 256 == 0)          # never splits a subset of the correction)
    if defect == "gelu_tanh":
        if not c.gelu:
            return False
        d = torch.from_numpy(np.abs(gelu_tanh64(c.pre_a.numpy()) - gelu_erf64(c.pre_a.numpy())))
        return bool((d > 2.0 * corr_bound(c)).any())
    return False


# ------------------------------------------------------------------------------------------------------------------------------
# the cases of the kernel tests
# ------------------------------------------------------------------------------------------------------------------------------
SPLIT_EPIS = ("plain", "res_f32_out16", "gelu")


def plain_cases():
    """(dt, M, N, K, epi) of ruart_gemm_16_nt"""
    return [(dt,) + s + (e,) for dt in ("bf16", "f16") for s in PLAIN_SHAPES for e in EPIS]


def plain_split_cases():
    """(dt, M, N, K, cus, epi) of ruart_gemm_16_nt_ws"""
    return [(dt,) + s + (e,) for dt in ("bf16", "f16") for s in SPLIT_SHAPES for e in SPLIT_EPIS]


def corr_cases():
    """(M, N, K, epi) of ruart_gemm_16c_nt"""
    return [s + (e,) for s in CORR_SHAPES for e in CORR_EPIS]


def corr_split_cases():
    """(M, N, K, cus, epi) of ruart_gemm_16c_nt_ws"""
    return [s + (e,) for s in SPLIT_SHAPES for e in CORR_EPIS]


def plain_controls():
    """(case, defect) of every negative control of the plain product that can show; a case of plain_split_cases carries its plan"""
    out = []
    for case in plain_cases():
        c = plain_case(*case)
        order = plain_walk(*case[1:4])[1]
        out += [(case, d) for d in PLAIN_DEFECTS if plain_defect_shows(c, d, None, order)]
    for case in plain_split_cases():
        dt, M, N, K, cus, epi = case
        c = plain_case(dt, M, N, K, epi)
        out += [(case, d) for d in PLAIN_DEFECTS if plain_defect_shows(c, d, plain_plan(M, N, K, cus), plain_walk(M, N, K)[1])]
    return out


def corr_controls():
    out = []
    for case in corr_cases():
        out += [(case, d) for d in CORR_DEFECTS if corr_defect_shows(corr_case(*case), d)]
    for case in corr_split_cases():
        M, N, K, cus, epi = case
        out += [(case, d) for d in CORR_DEFECTS if corr_defect_shows(corr_case(M, N, K, epi), d, corr_plan(M, N, K, cus))]
    return out


def worst(out, ref, bound):
    """worst error / bound over every element (NaN anywhere: inf)"""
    r = (out - ref).abs() / bound
    return float("inf") if bool(torch.isnan(r).any()) else float(r.max())


# ------------------------------------------------------------------------------------------------------------------------------
# the training products: gelu2, gelu_bwd, split-K (NT and TN) + ruart_splitk_reduce
# ------------------------------------------------------------------------------------------------------------------------------
TRAIN_SHAPES = ((256, 256, 128), (512, 512, 256))


def gelu2_bounds(c):
    """(bound of H, bound of G) of ruart_gemm_16_nt_gelu2 on a plain_case(dt, M, N, K, "gelu"): H = the pre-activation rounded to the
    operands' type, G = gelu of the UNROUNDED fp32 pre-activation (the bound of the GELU epilogue)"""
    return _store_bound(c.pre, _pre_bound(c.S, c.bias, None, c.K), c.dt), plain_bound(c)


def gelu2_emulate(c, defect=None):
    """(H, G) in the kernel's arithmetic; defect "chunk_drop" | "bias_16" as plain_emulate, "g_from_h": G computed from the rounded H"""
    t16 = E.TORCH_TYPE[c.dt]
    acc = _ktile_sums(c.A, c.W, 0, c.K // 64)
    if defect == "chunk_drop":
        rows, cols, ks = slice(c.M - 256, c.M), slice(c.N - 256, c.N), slice(c.K - 56, c.K - 48)
        acc[rows, cols] = acc[rows, cols] - c.A[rows, ks] @ c.W[cols, ks].t()
    v = acc + (c.bias.to(t16).float() if defect == "bias_16" else c.bias)
    h = v.to(t16)
    g = torch.from_numpy(gelu_pk32((h.float() if defect == "g_from_h" else v).numpy())).to(t16)
    return h.double(), g.double()


GELU2_DEFECTS = ("chunk_drop", "bias_16", "g_from_h")


@functools.lru_cache(maxsize=None)
def gelu_bwd_case(M, N, K):
    """ruart_gemm_16_nt_gelu_bwd: dY (M, K) bf16 ~ 1e-3, Wt (N, K) bf16, H (M, N) f16 ~ N(0, 2).  Float64: acc = dY Wt^T, dH = acc gelu'(H),
    G = gelu(H), colsum[strip] = the sums of dH over the strip's 128 rows; and the element-wise bounds:
      dH   acc carries ea = ACC_C K u S, the derivative ed = GELU_APPROX["pk_d"] + 2^-22 (1 + |d|) (two v_exp_f32 and a v_rcp_f32):
           ea |d| + |acc| ed + ea ed, + u |dH| for the product, then bf16 storage
      G    GELU_APPROX["pk"] + 2^-22 |g|, then bf16 storage
      colsum  the sum of the 128 rows' dH bounds before storage + 34 u sum |dH| (a lane adds its 32 rows one by one, then two
              cross-lane additions)"""
    c = Case()
    c.M, c.N, c.K = M, N, K
    g = torch.Generator().manual_seed(13 * M + N + K)
    c.dY = (_operand_a(M, K, g) * 1e-3).bfloat16().float()
    c.Wt = (torch.randn(N, K, generator=g) * 0.05).bfloat16().float()
    c.H = (2.0 * torch.randn(M, N, generator=g)).half().float()
    acc = c.dY.double() @ c.Wt.double().t()
    S = c.dY.double().abs() @ c.Wt.double().abs().t()
    d = torch.from_numpy(gelu_d64(c.H.double().numpy()))
    c.ref_dh = acc * d
    c.ref_g = torch.from_numpy(gelu_erf64(c.H.double().numpy()))
    ea = ACC_C * K * U * S
    ed = GELU_APPROX["pk_d"] + 2.0 ** -22 * (1.0 + d.abs())
    pre = ea * d.abs() + acc.abs() * ed + ea * ed + U * c.ref_dh.abs()
    c.b_dh = _store_bound(c.ref_dh, pre, "bf16")
    c.b_g = _store_bound(c.ref_g, GELU_APPROX["pk"] + 2.0 ** -22 * c.ref_g.abs(), "bf16")
    c.ref_col = c.ref_dh.view(M // 128, 128, N).sum(1)
    c.b_col = pre.view(M // 128, 128, N).sum(1) + 34 * U * c.ref_dh.abs().view(M // 128, 128, N).sum(1)
    return c


GELU_BWD_DEFECTS = ("chunk_drop", "colsum_rounded", "deriv_tanh")


def gelu_bwd_emulate(c, defect=None):
    """(dH, G, colsum) in the kernel's arithmetic.  defect: "chunk_drop"; "colsum_rounded": the strip sums add the bf16 dH, not the
    unrounded product; "deriv_tanh": the derivative of the tanh-form GELU"""
    acc = _ktile_sums(c.dY, c.Wt, 0, c.K // 64)
    if defect == "chunk_drop":
        rows, cols, ks = slice(c.M - 256, c.M), slice(c.N - 256, c.N), slice(c.K - 56, c.K - 48)
        acc[rows, cols] = acc[rows, cols] - c.dY[rows, ks] @ c.Wt[cols, ks].t()
    gf, df = gelu_fwd_bwd32(c.H.numpy())
    if defect == "deriv_tanh":
        x = c.H.double().requires_grad_()
        torch.nn.functional.gelu(x, approximate="tanh").sum().backward()
        df = x.grad.float().numpy()
    v = acc * torch.from_numpy(df)
    dh = v.bfloat16()
    src = dh.float() if defect == "colsum_rounded" else v
    col = torch.zeros(c.M // 128, c.N)
    for r in range(128):                                   # (row by row in fp32: the order inside a strip is the kernel's business, the
        col = col + src.view(c.M // 128, 128, c.N)[:, r]   # bound allows for any)
    return dh.double(), torch.from_numpy(gf).bfloat16().double(), col.double()


SPLITK_SHAPES = ((256, 512, 384, 256), (256, 512, 256, 128))          # (M, N, K, kchunk): a partial last chunk; two whole ones
TN_T, TN_REAL, TN_CHUNK = 384, 300, 256


@functools.lru_cache(maxsize=None)
def splitk_case(dt, M, N, K, kchunk, tn=False):
    """A (M, K), W (N, K) of the 16-bit type, slabs z = A[:, z kchunk ..] W[:, z kchunk ..]^T in float64 with their bounds
    ACC_C k_z u S_z + u |slab| (fp32 store), and C = scale sum_z slab_z (+ C0) with the bound of ruart_splitk_reduce on top: the slabs'
    bounds, nz - 1 additions, the scale and the accumulate at u each of the magnitudes added.  ``tn``: the same product given as P = A^T
    (K, M) and Q = W^T (K, N) - token rows [TN_REAL, K) are padding: zero in A, large and finite in W."""
    c = Case()
    c.dt, c.M, c.N, c.K, c.kchunk = dt, M, N, K, kchunk
    t16 = E.TORCH_TYPE[dt]
    g = torch.Generator().manual_seed(M + N + K + kchunk + (1 if tn else 0))
    c.A = (_operand_a(M, K, g) * (1e-3 if dt == "bf16" else 1.0)).to(t16).float()
    c.W = torch.randn(N, K, generator=g).to(t16).float()
    if tn:
        c.A[:, TN_REAL:] = 0.0
        c.W[:, TN_REAL:] = 3.0e4                           # (finite in f16 and bf16; a product with a real row would dwarf every sum)
    c.C0 = torch.randn(M, N, generator=g) * float(c.A.abs().mean()) * 10.0
    c.scale = 0.5
    c.nz = (K + kchunk - 1) // kchunk
    c.slabs, c.b_slabs = [], []
    for z in range(c.nz):
        a, w = c.A[:, z * kchunk:(z + 1) * kchunk].double(), c.W[:, z * kchunk:(z + 1) * kchunk].double()
        ref = a @ w.t()
        c.slabs.append(ref)
        c.b_slabs.append(ACC_C * a.shape[1] * U * (a.abs() @ w.abs().t()) + U * ref.abs())
    tot, mag = sum(c.slabs), sum(s.abs() for s in c.slabs)
    c.ref = {0: c.scale * tot, 1: c.scale * tot + c.C0.double()}
    base = c.scale * (sum(c.b_slabs) + (c.nz - 1) * U * mag + U * mag)
    c.bound = {0: base, 1: base + U * (c.scale * mag + c.C0.double().abs())}
    return c


SPLITK_DEFECTS = ("chunk_drop", "last_chunk_unclamped", "slab_twice", "tn_pad_rows")


def splitk_emulate(c, defect=None):
    """(slabs, C overwrite, C accumulate) in fp32.  defect: "chunk_drop" (8 k-values of the last K-tile of the last slab missing);
    "last_chunk_unclamped" / "tn_pad_rows" (NT / TN): the partial last chunk runs to a whole kchunk, over columns / token rows past K that
    hold 1.0 in both operands here; "slab_twice": the reduction adds slab 0 twice"""
    A, W = c.A, c.W
    if defect in ("last_chunk_unclamped", "tn_pad_rows"):
        extra = c.nz * c.kchunk - c.K
        A, W = torch.cat([A, torch.ones(c.M, extra)], 1), torch.cat([W, torch.ones(c.N, extra)], 1)
    slabs = []
    for z in range(c.nz):
        k0, k1 = z * c.kchunk, min((z + 1) * c.kchunk, A.shape[1])
        s = torch.zeros(c.M, c.N)
        for k in range(k0, k1, 64):
            s = s + A[:, k:k + 64] @ W[:, k:k + 64].t()
        slabs.append(s)
    if defect == "chunk_drop":
        ks = slice(c.K - 56, c.K - 48)
        slabs[-1] = slabs[-1] - c.A[:, ks] @ c.W[:, ks].t()
    s = slabs[0].clone()
    for z in range(0 if defect == "slab_twice" else 1, c.nz):
        s = s + slabs[z]
    s = s * c.scale
    return [x.double() for x in slabs], s.double(), (s + c.C0).double()


def splitk_defect_shows(c, defect, tn):
    if defect in ("last_chunk_unclamped", "tn_pad_rows"):
        return c.K % c.kchunk != 0 and (defect == "tn_pad_rows") == tn
    if defect == "chunk_drop":
        return not tn                                       # (the last K-tile of the TN case is padding: zeros times finite values)
    return True


def splitk_cases():
    """(dt, M, N, K, kchunk, tn): both NT shapes, and the TN product at T = 384, tchunk = 256"""
    return [(dt,) + s + (False,) for dt in ("bf16", "f16") for s in SPLITK_SHAPES] + [(dt,) + SPLITK_SHAPES[0] + (True,) for dt in ("bf16", "f16")]


# ------------------------------------------------------------------------------------------------------------------------------
# the LayerNorm fold: consumer (kinds 0 / 2) and producer (kind 3) of ruart_gemm_16c_nt_fold / ruart_gemm_16_nt_fold
# ------------------------------------------------------------------------------------------------------------------------------
FOLD_EPS = 1e-12
CONSUMER_SHAPES = ((256, 512, 256), (512, 768, 1024))
PRODUCER_SHAPES = ((256, 256, 128), (512, 1024, 256))
FOLD_KINDS = ("c8", "bf16", "f16")                      # the fp16c entry, and the plain 16-bit entry in its two types


def row_partials(y):
    """fp32 [M][4][2] (sum, sumsq) of the rows of y per 256-column tile, summed in float64 and rounded; unused slots hold NaN"""
    M, H = y.shape
    p = torch.full((M, 4, 2), float("nan"), dtype=torch.float32)
    for t in range(H // 256):
        blk = y[:, t * 256:(t + 1) * 256].double()
        p[:, t, 0] = blk.sum(1).float()
        p[:, t, 1] = (blk * blk).sum(1).float()
    return p


def _stats32(part, n_parts, H, eps, no_eps=False):
    """fold_row_stat_of in fp32: (mu, rstd); ``no_eps``: without the clamp at 0 and without eps (the fold_no_clamp_eps defect)"""
    p = part.numpy()
    s, q = np.zeros(p.shape[0], np.float32), np.zeros(p.shape[0], np.float32)
    for k in range(n_parts):
        s, q = s + p[:, k, 0], q + p[:, k, 1]
    inv_h = np.float32(1.0 / H)
    mu = s * inv_h
    var = q * inv_h - mu * mu
    with np.errstate(divide="ignore", invalid="ignore"):
        rstd = np.float32(1.0) / np.sqrt(var if no_eps else np.maximum(var, np.float32(0.0)) + np.float32(eps))
    return torch.from_numpy(mu.astype(np.float32)), torch.from_numpy(rstd.astype(np.float32))


def _operand_products(kind, X, Wm):
    """the operands as ``kind`` stores them and the float64 product of exactly those: returns (ops, acc64, S, n, emulate_acc) with ops
    the host arrays the kernel is given, n the products per output element"""
    o = Case()
    K = X.shape[1]
    if kind == "c8":
        sa_lo, sa_hi, sw_hi, _ = E.header_shifts()
        o.A16, o.A8 = E.split_ref(X.numpy(), sa_lo, sa_hi)
        o.W16, o.W8 = weight_split_ref(Wm.numpy())
        a16, w16 = torch.from_numpy(o.A16.astype(np.float64)), torch.from_numpy(o.W16.astype(np.float64))
        a8, w8 = torch.from_numpy(E.e4m3_decode(o.A8)), torch.from_numpy(E.e4m3_decode(o.W8))
        sc = 2.0 ** -(sa_lo + sw_hi)
        acc = a16 @ w16.t() + sc * (a8 @ w8.t())
        S = a16.abs() @ w16.abs().t() + sc * (a8.abs() @ w8.abs().t())
        a16f, w16f, a8f, w8f = a16.float(), w16.float(), a8.float(), w8.float()

        def emu():
            e = torch.zeros(X.shape[0], Wm.shape[0])
            for t in range(K // 64):
                e = e + a16f[:, 64 * t:64 * t + 64] @ w16f[:, 64 * t:64 * t + 64].t()
            for t in range(K // 64):
                e = e + (a8f[:, 128 * t:128 * t + 128] @ w8f[:, 128 * t:128 * t + 128].t()) * sc
            return e
        return o, acc, S, 3 * K, emu
    t16 = E.TORCH_TYPE[kind]
    o.A, o.W = X.to(t16).float(), Wm.to(t16).float()
    acc = o.A.double() @ o.W.double().t()
    S = o.A.double().abs() @ o.W.double().abs().t()
    return o, acc, S, K, lambda: _ktile_sums(o.A, o.W, 0, K // 64)


def _finish(kind, gelu, v64, b):
    """GELU and storage of a fold product: (ref, bound, out type) from the float64 value and its bound before them"""
    form = "erfc7" if kind == "c8" else "pk"
    ref = v64
    if gelu:
        ref = torch.from_numpy(gelu_erf64(v64.numpy()))
        b = GELU_SLOPE * b + GELU_APPROX[form] + 2.0 ** -22 * ref.abs()
    if kind != "c8":
        return ref, _store_bound(ref, b, kind)
    if gelu:
        return ref, b + 2.0 ** -15 * ref.abs() + 2.0 ** -21
    return ref, b + U * ref.abs()


@functools.lru_cache(maxsize=None)
def consumer_case(kind, M, N, K, gelu):
    """Kinds 0 / 2: rows y with an outlier dimension, a constant row (its variance is 0: only the clamp and eps keep rstd finite) and a gamma
    with one large gain, so that the fp16c weights W' = W diag(gamma) 2^-s need s >= 1.  The reference is the function the kernel computes of
    what it is given, in float64:  rstd 2^s (acc - mu c) + d  with acc the product of the stored operands, (mu, rstd) from the fp32 row
    partials (E.stats_from_partials) and the fp32 vectors c, d.  Bound, before GELU and storage, with ea = ACC_C n u S, (dm, drel) =
    E.stats_bound, sc = rstd 2^s, t = acc - mu c:
        e_t = ea + dm |c| + u (|acc| + |mu c|)         (one fma: the rounding of mu c counts at |mu c|, the difference cancels)
        e_v = sc e_t + |sc t| (drel + u) + u (|sc t| + |d|)"""
    c = Case()
    c.kind, c.M, c.N, c.K, c.gelu = kind, M, N, K, gelu
    g = torch.Generator().manual_seed(17 * M + N + K + int(gelu) + FOLD_KINDS.index(kind))
    y = torch.randn(M, K, generator=g) * (0.5 + 2.0 * torch.rand(M, 1, generator=g)) + 0.3 * torch.randn(M, 1, generator=g)
    y[:, 5] += 20.0
    y[3] = 0.75
    W = torch.randn(N, K, generator=g) * 0.03
    bias = torch.randn(N, generator=g) * 0.1
    gam, bet = 1.0 + 0.2 * torch.randn(K, generator=g), 0.1 * torch.randn(K, generator=g)
    gam[7] = 40.0
    wf = W * gam[None, :]
    c.s = 0
    if kind == "c8":
        while float(wf.abs().max()) * 2.0 ** -c.s >= 3.4:
            c.s += 1
        assert c.s >= 1
    wf = wf * 2.0 ** -c.s
    c.ops, acc, S, n, c.emu_acc = _operand_products(kind, y, wf)
    y_stored = y if kind == "c8" else c.ops.A
    c.part, c.np = row_partials(y_stored), K // 256
    c.dvec = (bias.double() + W.double() @ bet.double()).float()
    c.cvec = (torch.from_numpy(c.ops.W16.astype(np.float64)) if kind == "c8" else c.ops.W.double()).sum(1).float()
    mu, rstd = E.stats_from_partials(c.part, c.np, K, FOLD_EPS)
    dm, drel = E.stats_bound(c.part, c.np, K, FOLD_EPS)
    mu, rstd, dm, drel = mu[:, None], rstd[:, None], dm[:, None], drel[:, None]
    cc, dd = c.cvec.double()[None, :], c.dvec.double()[None, :]
    sc = rstd * 2.0 ** c.s
    t = acc - mu * cc
    v = sc * t + dd
    e_t = ACC_C * n * U * S + dm * cc.abs() + U * (acc.abs() + (mu * cc).abs())
    e_v = sc * e_t + (sc * t).abs() * (drel + U) + U * ((sc * t).abs() + dd.abs())
    c.ref, c.bound = _finish(kind, gelu, v, e_v)
    return c


CONSUMER_DEFECTS = ("chunk_drop", "fold_no_clamp_eps", "slot_missing", "scale_missing")


def consumer_emulate(c, defect=None):
    """the kernel's arithmetic; returns (out, hi8).  defect: "chunk_drop"; "fold_no_clamp_eps" (statistics without the clamp and eps: the
    constant row); "slot_missing" (the last partial slot left out of the statistics: shows where there are two or more); "scale_missing" (2^s left out: shows where s >= 1)"""
    acc = c.emu_acc()
    if defect == "chunk_drop":
        ks = slice(c.K - 56, c.K - 48)
        a, w = (c.ops.A16.astype(np.float32), c.ops.W16.astype(np.float32)) if c.kind == "c8" else (c.ops.A.numpy(), c.ops.W.numpy())
        acc[-256:, -256:] = acc[-256:, -256:] - torch.from_numpy(a[-256:, ks]) @ torch.from_numpy(w[-256:, ks]).t()
    mu, rstd = _stats32(c.part, c.np - 1 if defect == "slot_missing" else c.np, c.K, FOLD_EPS, defect == "fold_no_clamp_eps")
    sc = rstd * (1.0 if defect == "scale_missing" else 2.0 ** c.s)
    t = (acc.double() - mu.double()[:, None] * c.cvec.double()[None, :]).float()
    v = (sc.double()[:, None] * t.double() + c.dvec.double()[None, :]).float()
    if c.gelu:
        v = torch.from_numpy((gelu_erfc732 if c.kind == "c8" else gelu_pk32)(v.numpy()))
    if c.kind != "c8":
        return v.to(E.TORCH_TYPE[c.kind]).double(), None
    if c.gelu:
        sa_lo, sa_hi, _, _ = E.header_shifts()
        h16, h8 = E.split_ref(v.numpy(), sa_lo, sa_hi)
        fine, coarse = E.split_decode(h16, h8, c.N, sa_lo, sa_hi)
        return torch.from_numpy(fine), torch.from_numpy(coarse)
    return v.double(), None


def consumer_defect_shows(c, defect):
    if defect == "slot_missing":
        return c.np >= 2
    return c.s >= 1 if defect == "scale_missing" else True


@functools.lru_cache(maxsize=None)
def producer_case(kind, M, N, K, res_ln):
    """Kind 3: y = acc + bias + r, r the residual rows as given (fp32 for the fp16c entry, the 16-bit type otherwise) or - res_ln - their
    LayerNorm g (res - mu) rstd + beta with (mu, rstd) from the residual's fp32 row partials.  Reference in float64 on the stored operands
    and the same partials.  Bound before storage: the product's (_pre_bound with the residual's rounding) plus, under res_ln, the error of
    the normalised residual  z = res - mu: dm + u |z|;  z rstd: |z rstd| (drel + u) + rstd (dm + u |z|);  the fma with gamma, beta: |g| x
    that + u |r|.  Row partials of the y written: (sum, sumsq) per 256-column tile against float64 sums at PART_DEPTH u sum |y| and
    (PART_DEPTH + 1) u sum y^2 - a lane adds four values, four DPP steps join 16 lanes, two additions the four column groups: nine
    additions deep, and the squares are rounded once more."""
    c = Case()
    c.kind, c.M, c.N, c.K, c.res_ln = kind, M, N, K, res_ln
    g = torch.Generator().manual_seed(19 * M + N + K + int(res_ln) + FOLD_KINDS.index(kind))
    A = _operand_a(M, K, g)
    W = torch.randn(N, K, generator=g) * 0.03
    c.bias = torch.randn(N, generator=g) * 0.1
    c.bias[3::16] *= 1000.0                     # (some large entries, so that bias_16 can show)
    c.bias.clamp_(-200.0, 200.0)
    R = torch.randn(M, N, generator=g) * 1.5 + 0.2
    c.res = R if kind == "c8" else R.to(E.TORCH_TYPE[kind]).float()
    c.gam, c.bet = 1.0 + 0.3 * torch.randn(N, generator=g), 0.1 * torch.randn(N, generator=g)
    c.ops, acc, S, n, c.emu_acc = _operand_products(kind, A, W)
    c.np = N // 256
    c.part = row_partials(c.res) if res_ln else None
    r, e_r = c.res.double(), torch.zeros(M, N, dtype=torch.float64)
    if res_ln:
        mu, rstd = E.stats_from_partials(c.part, c.np, N, FOLD_EPS)
        dm, drel = E.stats_bound(c.part, c.np, N, FOLD_EPS)
        mu, rstd, dm, drel = mu[:, None], rstd[:, None], dm[:, None], drel[:, None]
        z = c.res.double() - mu
        r = c.gam.double() * (z * rstd) + c.bet.double()
        e_r = c.gam.double().abs() * ((z * rstd).abs() * (drel + U) + rstd * (dm + U * z.abs())) + U * r.abs()
    c.ref = acc + c.bias.double() + r
    c.pre_bound = ACC_C * n * U * S + U * (S + c.bias.double().abs()) + e_r + U * (S + c.bias.double().abs() + r.abs())
    c.bound = _store_bound(c.ref, c.pre_bound, "f32" if kind == "c8" else kind)
    return c


PART_DEPTH = 9


def partial_bounds(y, n_tiles):
    """(float64 (sum, sumsq) [M][n_tiles][2], their fp32 summation bounds) of the rows of y per 256-column tile"""
    M = y.shape[0]
    blk = y.double().view(M, n_tiles, 256)
    want = torch.stack([blk.sum(2), (blk * blk).sum(2)], 2)
    bound = torch.stack([PART_DEPTH * U * blk.abs().sum(2), (PART_DEPTH + 1) * U * (blk * blk).sum(2)], 2)
    return want, bound + 2.0 ** -149


PRODUCER_DEFECTS = ("chunk_drop", "bias_16", "res_16", "res_ln_no_beta", "partials_of_rounded")


def producer_emulate(c, defect=None):
    """(y as stored, decoded; the fp32 y before storage; partials [M][np][2] fp32).  defect: chunk_drop, bias_16, res_16 (fp32 residual
    rounded to f16; fp16c entry), res_ln_no_beta (the normalised residual without beta), partials_of_rounded (16-bit entries: the row
    partials taken from the stored y, not from the fp32 y)"""
    acc = c.emu_acc()
    if defect == "chunk_drop":
        ks = slice(c.K - 56, c.K - 48)
        a, w = (c.ops.A16.astype(np.float32), c.ops.W16.astype(np.float32)) if c.kind == "c8" else (c.ops.A.numpy(), c.ops.W.numpy())
        acc[-256:, -256:] = acc[-256:, -256:] - torch.from_numpy(a[-256:, ks]) @ torch.from_numpy(w[-256:, ks]).t()
    v = acc + (c.bias.half().float() if defect == "bias_16" else c.bias)
    r = c.res.half().float() if defect == "res_16" else c.res
    if c.res_ln:
        mu, rstd = _stats32(c.part, c.np, c.N, FOLD_EPS)
        r = (c.gam.double() * ((r - mu[:, None]) * rstd[:, None]).double() + (0.0 if defect == "res_ln_no_beta" else c.bet.double())).float()
    v = v + r
    stored = v if c.kind == "c8" else v.to(E.TORCH_TYPE[c.kind]).float()
    src = stored if defect == "partials_of_rounded" else v
    blk = src.view(c.M, c.np, 256)
    part = torch.stack([blk.sum(2), (blk * blk).sum(2)], 2)
    return stored.double(), v, part


def producer_defect_shows(c, defect):
    if defect == "res_16":
        return c.kind == "c8"
    if defect == "res_ln_no_beta":
        return c.res_ln
    if defect == "partials_of_rounded":
        return c.kind != "c8"
    return True


def consumer_cases():
    return [(k,) + s + (gelu,) for k in FOLD_KINDS for s in CONSUMER_SHAPES for gelu in (False, True)]


def producer_cases():
    return [(k,) + s + (ln,) for k in FOLD_KINDS for s in PRODUCER_SHAPES for ln in (False, True)]
