"""Float64 references, derived per-element bounds, a Python restatement of the plan and dispatch, and a CPU emulation of the trunk's
split-bf16 products (csrc/sdnet_gemm.hip: ruart_gemm_x3, ruart_gemm_x1, ruart_gemm_bf16_tn, ruart_gemm_x3_tn_grouped and the two
slice-sum kernels).  Test infrastructure: numpy / torch on the CPU, no GPU import; used by tests/test_gpu_x3_gemm.py and proven on the
CPU, negative controls included, by tests/test_x3_ref.py.  worst-style ratios, ACC_C, GELU_SLOPE and the operand generator are
tests/_gemm_ref.py's.

  plan       make_plan, slices, load_width, dispatch: what gemm_xn decides, restated at the defaults of the source (fill 128, nosplit 160,
             fill256 256, min256 192 - the four RUART_X3_* overrides must be unset: env_is_default); INSTANTIATIONS: the 54 kernel
             instantiations the X3W / X3S / X3M macros can reach.
  operands   split(x): hi = bf16(x), lo = bf16(x - hi).  common.h types bf16_t as the compiler's __bf16, whose conversion from float is
             round-to-nearest-even (v_cvt_pk_bf16_f32 on gfx950; the software sequence elsewhere rounds the same way) - torch's
             .bfloat16() is the same rounding.  A masked operand is first fp32(x * keep_scale) where the byte is non-zero and 0
             elsewhere: one fp32 rounding, the one x * mask makes; the references start from that product ("multiply first").
  references per output element in float64, with ah, al, bh, bl the halves, ra = a - ah - al, rb = b - bh - bl, u = 2^-24:
             (a) the function of its inputs the kernel computes: F = sum_k (ah bh + ah bl + al bh) - each product of two bf16 values
                 is exact in fp32 -, S3 the same sum over absolute values; x1 and bf16_tn: F1 = sum_k ah bh, S1.
                 Kernel against (a): ACC_C n u S, n = 3 K + slices (x1: K + slices; slices = 1 when unsplit).  ACC_C = 2 allows for
                 the rounding inside the matrix unit, which nobody has measured here; it was fixed before any GPU run.
             (b) the product of the unrounded fp32 operands: (a)'s bound plus the format bound
                 fmt = sum_k (|al| |bl| + |ra| |b| + |ah + al| |rb|)        (x1: sum_k (|a - ah| |b| + |ah| |b - bh|))
                 from a b - (ah bh + ah bl + al bh) = al bl + ra b + (ah + al) rb, an exact identity: nothing is estimated.
  epilogue   v = acc + bias: u (S + |bias|);  GELU (exact-erf form in fp32, v * 0.5 * (1 + erff(v / sqrt 2))): GELU_SLOPE x (bound so
             far) + E_ERF, E_ERF = 2 x ERF_GELU_MEASURED + 2^-21 |v|: the fp32 evaluation of the formula with torch's fp32 erf against
             float64 over |x| <= 12 (measure_erf_gelu; test_x3_ref.py asserts the constant covers it), doubled, plus an allowance
             for the device's erff, which nobody has measured;  c_scale: (bound so far) x |c_scale| + u |v c_scale|;  residual:
             u (|v| + |residual|);  storage in fp32: u |ref|.
  cases      x3_case(M, N, K, ...): A ~ randn with one row in ten at 4 x (G._operand_a), B ~ 0.1 randn, and COHERENT rows - on random data
             a missing cross term is a random walk and hides inside any bound linear in K, so every 128th row of A from row 1 holds
             COH = 1 + 0.49 2^-7 + 0.3 2^-16 (every lo of the same sign, a non-zero residual), every 128th column of B from column 1
             0.125 COH and from column 2 0.125 (its lo is 0): each 128- and 256-tile holds them.  The discrimination decays as 1 / K
             (about 10 x the bound at K = 1040, gone near 10^4): every controlled case keeps K <= 2100.
  emulation  x3_emulate(case, np, tm, splitk, defect): the kernels' arithmetic in torch fp32 - K steps of 32 in order, per step the terms
             in the source's order (bl.ah, bh.al, bh.ah), slices summed in slice order, then bias, GELU, c_scale, residual.
             DEFECTS are the negative controls; x3_defect_shows says where one can change anything at all.
"""
import collections
import functools
import os

import numpy as np
import torch

from tests import _gemm_ref as G

U = G.U
ACC_C = G.ACC_C
GELU_SLOPE = G.GELU_SLOPE
XBK = 32
X3G_MAX = 44
COH = 1.0 + 0.49 * 2.0 ** -7 + 0.3 * 2.0 ** -16
KEEP_P = 0.7
# max |fp32 evaluation of v 0.5 (1 + erf(v / sqrt 2)) with torch's fp32 erf - float64| over |x| <= 12 (measure_erf_gelu)
ERF_GELU_MEASURED = 4.45e-7
ENV_OVERRIDES = ("RUART_X3_FILL", "RUART_X3_NOSPLIT_TILES", "RUART_X3_T256_FILL", "RUART_X3_T256_MIN")


def env_is_default():
    return not any(os.environ.get(k) for k in ENV_OVERRIDES)


# ------------------------------------------------------------------------------------------------------------------------------
# the plan and the dispatch of gemm_xn, restated
# ------------------------------------------------------------------------------------------------------------------------------


def ksteps_of(K):
    return (K + XBK - 1) // XBK


def make_plan(M, N, K, amode, bmode, fill=128, nosplit=160, fill256=256, min256=192):
    """(tm, tiles, splitk) of make_plan (sdnet_gemm.hip); amode / bmode 0: the operand's K index is contiguous"""
    ksteps = ksteps_of(K)

    def split_for(tiles):
        if tiles >= nosplit or ksteps < 16:
            return 1
        s = min((fill + tiles - 1) // tiles, ksteps // 4, 64)
        return max(s, 1)
    t256 = ((M + 255) // 256) * ((N + 255) // 256)
    t128 = ((M + 127) // 128) * ((N + 127) // 128)
    s256 = 1
    if t256 < 200 and ksteps >= 16:
        s256 = max(min((fill256 + t256 - 1) // t256, ksteps // 8), 1)
    waste = t256 * 65536.0 / (float(M) * N)
    if bmode == 0 and M * N >= 4096 * 1024 and t256 * s256 >= min256 and waste < 1.25:
        return 256, t256, s256
    return 128, t128, split_for(t128)


def ws_bytes_of(plan):
    tm, tiles, splitk = plan
    return tiles * splitk * tm * tm * 4 if splitk > 1 else 0


def slices(ksteps, splitk):
    """[(kbeg, kend)] per slice, in K steps; a slice with kbeg >= kend is empty"""
    per = (ksteps + splitk - 1) // splitk
    return [(s * per, min(ksteps, s * per + per)) for s in range(splitk)]


def load_width(base_offset_floats, pitch, extent, mask_offset_bytes=None):
    """floats per load along an operand's contiguous index: the operand starts ``base_offset_floats`` into a 16-byte aligned buffer, a
    fused mask ``mask_offset_bytes`` into one (None: no mask)"""
    bits = 4 * base_offset_floats
    mbits = mask_offset_bytes or 0
    if bits % 16 == 0 and mbits % 4 == 0 and pitch % 4 == 0 and extent % 4 == 0:
        return 4
    if bits % 8 == 0 and mbits % 2 == 0 and pitch % 2 == 0 and extent % 2 == 0:
        return 2
    return 1


def dispatch_raw(M, N, K, amode, bmode, a_off, a_pitch, b_off, b_pitch, msk=0, mask_off=0, have_ws=True):
    """(tm, amode, bmode, vwa, vwb, msk, splitk) of the kernel gemm_xn launches (msk 1: a_keep, 2: b_keep), or None where it refuses"""
    tm, tiles, splitk = make_plan(M, N, K, amode, bmode)
    if not have_ws:
        splitk = 1
    vwa = load_width(a_off, a_pitch, K if amode == 0 else M, mask_off if msk == 1 else None)
    vwb = load_width(b_off, b_pitch, K if bmode == 0 else N, mask_off if msk == 2 else None)
    if tm == 256 and (vwa == 1 or vwb == 1):
        tm, splitk = 128, 1
    if msk:
        if (msk == 1 and amode != 0) or (msk == 2 and bmode != 1):
            return None
        vw = min(vwa, vwb)
        if msk == 1 and bmode == 0:
            if tm == 256 and vw >= 2:
                return 256, 0, 0, vw, vw, 1, splitk
            if tm == 256:
                tm, splitk = 128, 1
            return 128, 0, 0, vw, vw, 1, splitk
        if tm == 256:
            tm, splitk = 128, 1
        if msk == 2 and amode == 1:
            return 128, 1, 1, vw, vw, 2, splitk
        return 128, 0, 1, 1, 1, msk, splitk
    if tm == 256 and bmode != 0:
        return None
    return tm, amode, bmode, vwa, vwb, 0, splitk


def _instantiations():
    """(tm, amode, bmode, vwa, vwb, msk): X3W over the four layouts of the 128 tile (with X3S: nine width pairs) and the two of the
    256 tile (four pairs), and the ten X3M forms"""
    out = []
    for am in (0, 1):
        for bm in (0, 1):
            out += [(128, am, bm, va, vb, 0) for va in (4, 2, 1) for vb in (4, 2, 1)]
    for am in (0, 1):
        out += [(256, am, 0, va, vb, 0) for va in (4, 2) for vb in (4, 2)]
    out += [(256, 0, 0, 4, 4, 1), (256, 0, 0, 2, 2, 1)]
    out += [(128, 0, 0, w, w, 1) for w in (4, 2, 1)] + [(128, 1, 1, w, w, 2) for w in (4, 2, 1)]
    out += [(128, 0, 1, 1, 1, 1), (128, 0, 1, 1, 1, 2)]
    return tuple(out)


INSTANTIATIONS = _instantiations()
assert len(INSTANTIATIONS) == 54 and len(set(INSTANTIATIONS)) == 54

# ------------------------------------------------------------------------------------------------------------------------------
# a call: the shape, the layout and every alignment the dispatch and the epilogue look at
# ------------------------------------------------------------------------------------------------------------------------------
# lay: "nt" A and B K-contiguous (x W^T), "nn" A K-, B N-contiguous (dX = dY W), "tn" A M-, B N-contiguous (dW = dY^T X), "tt" A M-, B
# K-contiguous.  aoff / boff: floats from a 16-byte aligned buffer start to the operand; apad / bpad: pitch - contiguous extent.
# msk 1 a_keep / 2 b_keep with ``rpm`` rows per mask row, the mask ``moff`` bytes into its buffer; cs: c_scale (rpm again).
# ws "plan" (ruart_gemm_x3_plan's bytes) | "null" | "short" (4 bytes less).  coff, cpad, rpad, biasoff: C base offset, ldc - N, ldr - N and
# the bias base offset, in floats.
Spec = collections.namedtuple("Spec", "M N K lay np aoff apad boff bpad bias gelu cs res msk rpm moff ws coff cpad rpad biasoff")


def spec(M, N, K, lay="nt", np_=3, wa=4, wb=4, bias=False, gelu=False, cs=False, res=False, msk=0, rpm=1, moff=0, ws="plan", coff=0, cpad=4,
         rpad=8, biasoff=0):
    """a Spec whose operands aim at the load widths wa / wb by base offset (0 / 2 / 1 floats) and pitch (+4 / +2 / +1)"""
    off = {4: (0, 4), 2: (2, 2), 1: (1, 1)}
    return Spec(M, N, K, lay, np_, off[wa][0], off[wa][1], off[wb][0], off[wb][1], bias, gelu, cs, res, msk, rpm, moff, ws, coff, cpad, rpad,
                biasoff)


def modes(lay):
    return (0 if lay[0] == "n" else 1), (0 if lay[1] == "t" else 1)


def pitches(s):
    am, bm = modes(s.lay)
    return (s.K if am == 0 else s.M) + s.apad, (s.K if bm == 0 else s.N) + s.bpad


def dispatch(s):
    am, bm = modes(s.lay)
    pa, pb = pitches(s)
    return dispatch_raw(s.M, s.N, s.K, am, bm, s.aoff, pa, s.boff, pb, s.msk, s.moff, s.ws == "plan")


def planned(s):
    """(tm, splitk) the call runs with"""
    d = dispatch(s)
    return d[0], d[6]


def epilogue_is_vector(s):
    """whether the 16-byte epilogue form is open to the call at all (the last partial column group is element-wise regardless)"""
    return (s.coff % 4 == 0 and (not s.bias or s.biasoff % 4 == 0) and (s.N + s.cpad) % 4 == 0 and (not s.res or (s.N + s.rpad) % 4 == 0)
            and (not s.cs or s.N % 4 == 0))


def data_key(s):
    return (s.M, s.N, s.K, s.bias, s.gelu, s.cs, s.res, s.msk, s.rpm)


# ------------------------------------------------------------------------------------------------------------------------------
# the operands as the kernel sees them, the references and the bounds
# ------------------------------------------------------------------------------------------------------------------------------


def split(x):
    """(hi, lo) as fp32 tensors holding bf16 values: hi = bf16(x), lo = bf16(x - hi), round-to-nearest-even"""
    hi = x.bfloat16().float()
    return hi, (x - hi).bfloat16().float()


def gelu_erf32(v):
    """the kernels' epilogue formula in torch fp32"""
    return v * 0.5 * (1.0 + torch.erf(v * np.float32(0.70710678118654752440)))


def measure_erf_gelu():
    x = torch.cat([torch.linspace(-12.0, 12.0, 1200001, dtype=torch.float64).float(),
                   torch.randn(200000, generator=torch.Generator().manual_seed(0)) * 2.0])
    x = x[x.abs() <= 12.0]
    return float((gelu_erf32(x).double() - torch.from_numpy(G.gelu_erf64(x.double().numpy()))).abs().max())


class Case:
    pass


class _Prod:
    pass


def _build_case(M, N, K, bias, gelu, cs, res, msk, rpm, acc_seed=0):
    c = Case()
    c.M, c.N, c.K, c.gelu, c.msk, c.rpm = M, N, K, gelu, msk, rpm
    g = torch.Generator().manual_seed(1000003 * M + 1009 * N + K + 17 * (int(bias) + 2 * int(gelu) + 4 * int(cs) + 8 * int(res) + 16 * msk) + 7 * rpm + acc_seed)
    A = G._operand_a(M, K, g)
    B = torch.randn(K, N, generator=g) * 0.1
    A[1::128] = COH
    B[:, 1::128] = 0.125 * COH
    B[:, 2::128] = 0.125
    c.A, c.B = A, B
    c.bias = c.cscale = c.res = c.keep = None
    c.keep_scale = 1.0
    if bias:
        c.bias = torch.randn(N, generator=g)
        c.bias[3::16] *= 100.0
    if res:
        c.res = torch.randn(M, N, generator=g)
        c.res[:, 5::16] *= 100.0

    def mask(rows, cols, kept_row):
        m = (torch.rand(rows, cols, generator=g) < KEEP_P)
        m[rows // 2] = False                      # one all-dropped mask row (not the last: a b_keep's would zero the K tail) ...
        m[kept_row] = True                        # ... and one all-kept one (the coherent row's, so that it stays whole)
        return m
    if cs:
        assert M % rpm == 0
        c.cscale = mask(M // rpm, N, 1 // rpm).float() * np.float32(1.0 / KEEP_P)
    if msk:
        rows = (M if msk == 1 else K)
        assert rows % rpm == 0
        c.keep = mask(rows // rpm, K if msk == 1 else N, min(1 // rpm, rows // rpm - 1)).to(torch.uint8)
        c.keep[c.keep != 0] = 3                   # (any non-zero byte keeps)
        c.keep_scale = float(np.float32(1.0 / KEEP_P))
    # the operands after the fused mask: fp32(x * keep_scale) where kept, 0 elsewhere
    c.Am, c.Bm = A, B
    if msk == 1:
        c.Am = torch.where(c.keep.repeat_interleave(rpm, 0) != 0, A * np.float32(c.keep_scale), torch.zeros(()))
    if msk == 2:
        c.Bm = torch.where(c.keep.repeat_interleave(rpm, 0) != 0, B * np.float32(c.keep_scale), torch.zeros(()))
    c._prod = {}
    return c


@functools.lru_cache(maxsize=None)
def _small_case(*key):
    return _build_case(*key)


@functools.lru_cache(maxsize=2)
def _big_case(*key):
    return _build_case(*key)


def x3_case(M, N, K, bias=False, gelu=False, cs=False, res=False, msk=0, rpm=1):
    """the data of a call (seeded from the arguments; cached - the big ones two at a time)"""
    key = (M, N, K, bias, gelu, cs, res, msk, rpm)
    return _big_case(*key) if M * N > (1 << 20) else _small_case(*key)


def case_of(s):
    return x3_case(*data_key(s))


def products(c, np_):
    """float64 ingredients: F (reference (a) before the epilogue), S, P (the product of the unrounded operands), fmt"""
    if np_ in c._prod:
        return c._prod[np_]
    p = _Prod()
    a, b = c.Am.double(), c.Bm.double()
    ah, al = (x.double() for x in split(c.Am))
    bh, bl = (x.double() for x in split(c.Bm))
    p.P = a @ b
    if np_ == 3:
        p.F = (ah + al) @ bh + ah @ bl
        p.S = (ah.abs() + al.abs()) @ bh.abs() + ah.abs() @ bl.abs()
        ra, rb = a - ah - al, b - bh - bl
        p.fmt = al.abs() @ bl.abs() + ra.abs() @ b.abs() + (ah + al).abs() @ rb.abs()
    else:
        p.F = ah @ bh
        p.S = ah.abs() @ bh.abs()
        p.fmt = (a - ah).abs() @ b.abs() + ah.abs() @ (b - bh).abs()
    c._prod = {np_: p}                            # (one at a time: the big cases' matrices are 100 MB each)
    return p


def x3_bound(c, np_=3, nslices=1, against="a"):
    """(ref, bound), both (M, N) float64, of the stored output against reference (a) or (b), term by term (module docstring)"""
    p = products(c, np_)
    n = (3 if np_ == 3 else 1) * c.K + nslices
    b = ACC_C * n * U * p.S
    ref = p.F
    if against == "b":
        b = b + p.fmt
        ref = p.P
    if c.bias is not None:
        ref = ref + c.bias.double()
        b = b + U * (p.S + c.bias.double().abs())
    if c.gelu:
        v = ref
        ref = torch.from_numpy(G.gelu_erf64(v.numpy()))
        b = GELU_SLOPE * b + 2.0 * ERF_GELU_MEASURED + 2.0 ** -21 * v.abs()
    if c.cscale is not None:
        sc = c.cscale.repeat_interleave(c.rpm, 0).double()
        ref = ref * sc
        b = b * sc.abs() + U * ref.abs()
    if c.res is not None:
        b = b + U * (ref.abs() + c.res.double().abs())
        ref = ref + c.res.double()
    return ref, b + U * ref.abs()


def worst(out, ref, bound):
    """worst error / bound over every element; an element whose bound is 0 (a c_scale of 0) must be exact; NaN anywhere: inf"""
    err = (out - ref).abs()
    if bool(torch.isnan(err).any()):
        return float("inf")
    r = torch.where(err == 0, torch.zeros_like(err), err / bound)
    return float(r.max())


# ------------------------------------------------------------------------------------------------------------------------------
# the emulation and its defects
# ------------------------------------------------------------------------------------------------------------------------------
DEFECTS = ("drop_hl", "drop_lh", "ktail_dup", "kstep_drop", "slice_twice", "slice_missing", "empty_slice_stale", "mask_unscaled",
           "mask_row_off", "mask_tail_ignored", "cscale_row", "bias_lost_on_split", "residual_twice", "gelu_tanh", "accumulate_lost",
           "x1_lo_kept")


def _masked_operands(c, defect):
    """(A, B) fp32 after the fused mask, with the mask defects"""
    if not c.msk:
        return c.A, c.B
    rows = c.M if c.msk == 1 else c.K
    idx = torch.arange(rows)
    idx = torch.clamp((idx + 1) // c.rpm, max=rows // c.rpm - 1) if defect == "mask_row_off" else idx // c.rpm
    keep = c.keep[idx] != 0
    scale = np.float32(1.0 if defect == "mask_unscaled" else c.keep_scale)
    x = c.A if c.msk == 1 else c.B
    y = torch.where(keep, x * scale, torch.zeros(()))
    if defect == "mask_tail_ignored":             # the last K step reads the operand without its mask
        k0 = XBK * (ksteps_of(c.K) - 1)
        if c.msk == 1:
            y[:, k0:] = x[:, k0:]
        else:
            y[k0:] = x[k0:]
    return (y, c.B) if c.msk == 1 else (c.A, y)


def x3_emulate(c, np_=3, tm=128, splitk=1, defect=None, accumulate=True):
    """The kernels' arithmetic in torch fp32 (module docstring).  defect (DEFECTS):
      drop_hl / drop_lh     the ah.bl / al.bh cross term missing
      ktail_dup             k >= K not zeroed: the clamped last element counted again for every k of the last step past K
      kstep_drop            k-values 8 .. 15 of the last step missing from the last tile
      slice_twice / slice_missing   the first slice added twice / the last non-empty slice left out
      empty_slice_stale     the slab of an empty slice holds 1.0
      mask_unscaled / mask_row_off / mask_tail_ignored   keep_scale not applied / mask row (r + 1) / rpm / no mask in the last K step
      cscale_row            c_scale indexed by m instead of m / rpm
      bias_lost_on_split    the slice sum forgets the bias
      residual_twice        both launches of a split product add the residual
      gelu_tanh             tanh-form GELU
      accumulate_lost       (grouped launch: the residual is the C to accumulate into) the product overwrites
      x1_lo_kept            the one-product form computed as the three-product one"""
    assert defect is None or defect in DEFECTS
    M, N, K = c.M, c.N, c.K
    A, B = _masked_operands(c, defect)
    ks = ksteps_of(K)
    pad = ks * XBK - K
    if pad:
        if defect == "ktail_dup":
            A = torch.cat([A, A[:, K - 1:K].expand(M, pad)], 1)
            B = torch.cat([B, B[K - 1:K].expand(pad, N)], 0)
        else:
            A, B = torch.cat([A, torch.zeros(M, pad)], 1), torch.cat([B, torch.zeros(pad, N)], 0)
    ah, al = split(A)
    bh, bl = split(B)
    three = (np_ == 3) != (defect == "x1_lo_kept" and np_ == 1)

    def step(acc, t, rows=slice(None), cols=slice(None), kk=slice(0, XBK), sign=1.0):
        """one K step into ``acc``, the terms in the source's order: bl.ah, bh.al, bh.ah"""
        k = slice(XBK * t + kk.start, XBK * t + kk.stop)
        if three and defect != "drop_hl":
            acc = acc + sign * (ah[rows, k] @ bl[k, cols])
        if three and defect != "drop_lh":
            acc = acc + sign * (al[rows, k] @ bh[k, cols])
        return acc + sign * (ah[rows, k] @ bh[k, cols])
    parts, empty = [], []
    for kb, ke in slices(ks, splitk):
        acc = torch.zeros(M, N)
        for t in range(kb, ke):
            acc = step(acc, t)
        if ke == ks and kb < ke and defect == "kstep_drop":
            rows, cols = slice(((M - 1) // tm) * tm, M), slice(((N - 1) // tm) * tm, N)
            acc[rows, cols] = step(acc[rows, cols], ks - 1, rows, cols, slice(8, 16), -1.0)
        parts.append(acc)
        empty.append(kb >= ke)
    if defect == "empty_slice_stale":
        parts = [torch.ones(M, N) if e else p for p, e in zip(parts, empty)]
    if defect == "slice_twice":
        parts.insert(1, parts[0])
    if defect == "slice_missing":
        parts.pop(max(i for i, e in enumerate(empty) if not e))
    v = parts[0]
    for p in parts[1:]:
        v = v + p
    if c.bias is not None and not (defect == "bias_lost_on_split" and splitk > 1):
        v = v + c.bias
    if c.gelu:
        v = torch.from_numpy(G.gelu_tanh64(v.double().numpy())).float() if defect == "gelu_tanh" else gelu_erf32(v)
    if c.cscale is not None:
        rows = torch.clamp(torch.arange(M), max=M // c.rpm - 1) if defect == "cscale_row" else torch.arange(M) // c.rpm
        v = v * c.cscale[rows]
    if c.res is not None and not (defect == "accumulate_lost" and accumulate):
        v = v + c.res
        if defect == "residual_twice" and splitk > 1:
            v = v + c.res
    return v.double()


def x3_defect_shows(c, defect, np_=3, splitk=1, accumulate=False):
    """whether ``defect`` can change anything on the case at all (a control is only required to break the bound where it can).  The
    cross-term controls need output element (1, 1), where a coherent row meets a coherent column (x3_case keeps the c_scale row and the
    a_keep row of row 1 whole)"""
    ks = ksteps_of(c.K)
    if defect in ("drop_hl", "drop_lh"):
        return np_ == 3 and c.M >= 2 and c.N >= 2
    if defect == "x1_lo_kept":
        return np_ == 1 and c.M >= 2 and c.N >= 2
    if defect == "ktail_dup":
        return c.K % XBK != 0
    if defect == "kstep_drop":
        return c.K - XBK * (ks - 1) > 8
    if defect in ("slice_twice", "slice_missing"):
        return splitk > 1
    if defect == "empty_slice_stale":
        return any(kb >= ke for kb, ke in slices(ks, splitk))
    if defect in ("mask_unscaled", "mask_tail_ignored"):
        return c.msk != 0
    if defect == "mask_row_off":
        return c.msk != 0 and (c.M if c.msk == 1 else c.K) // c.rpm > 1
    if defect == "cscale_row":
        return c.cscale is not None and c.rpm > 1
    if defect == "bias_lost_on_split":
        return c.bias is not None and splitk > 1
    if defect == "residual_twice":
        return c.res is not None and splitk > 1
    if defect == "accumulate_lost":
        return accumulate and c.res is not None
    if defect == "gelu_tanh":
        if not c.gelu:
            return False
        ref, bound = x3_bound(c, np_, splitk)
        pre = products(c, np_).F + c.bias.double() if c.bias is not None else products(c, np_).F
        d = torch.from_numpy(np.abs(G.gelu_tanh64(pre.numpy()) - G.gelu_erf64(pre.numpy())))
        sc = c.cscale.repeat_interleave(c.rpm, 0).double().abs() if c.cscale is not None else 1.0
        return bool((d * sc > 2.0 * bound).any())
    return False


# ------------------------------------------------------------------------------------------------------------------------------
# the cases of the kernel tests
# ------------------------------------------------------------------------------------------------------------------------------
_DIM = {"M": {4: 132, 2: 130, 1: 131}, "N": {4: 72, 2: 70, 1: 71}, "K": {4: 100, 2: 98, 1: 97}}
BIG, BIG2, BIG_SPLIT = (4000, 3000, 72), (3840, 3584, 70), 2048          # the 256 tile: unsplit at widths with a 4 / at (2, 2); split
K_LIST = (1, 31, 32, 33, 64, 65, 96, 97, 127, 128, 129, 160, 161, 192, 193)


def small_dims(lay, wa, wb, K=None):
    """(M, N, K) of a 128-tile case: each contiguous extent a multiple of 4 / of 2 (not of 4) / odd as the wider of the operands that
    run along it asks; an extent no operand runs along is odd"""
    am, bm = modes(lay)
    need = {"M": 1, "N": 1, "K": 1}
    for d, w in (("K" if am == 0 else "M", wa), ("K" if bm == 0 else "N", wb)):
        need[d] = max(need[d], w)
    return _DIM["M"][need["M"]], _DIM["N"][need["N"]], (_DIM["K"][need["K"]] if K is None else K)


def instantiation_specs():
    """one Spec per entry of INSTANTIATIONS, in its order, plus the split 256 plans at (4, 4) nt and (2, 2) A-transposed"""
    out = []
    for tm, am, bm, va, vb, msk in INSTANTIATIONS:
        lay = "nt"[am] + "tn"[bm]
        if tm == 256:
            M, N, K = BIG2 if (va, vb) == (2, 2) else BIG
            out.append(spec(M, N, K, lay, wa=va, wb=vb, msk=msk))
        elif msk and (am, bm) == (0, 1):                # the width-1 forms whatever the alignment: one operand at 4, one at 1
            M, N, K = small_dims(lay, 4, 4)
            out.append(spec(M, N, K, lay, wa=4 if msk == 1 else 1, wb=1 if msk == 1 else 4, msk=msk))
        else:
            M, N, K = small_dims(lay, va, vb)
            out.append(spec(M, N, K, lay, wa=va, wb=vb, msk=msk))
    out.append(spec(BIG_SPLIT, BIG_SPLIT, 772, "nt", wa=4, wb=4))
    out.append(spec(BIG_SPLIT, BIG_SPLIT, 770, "tt", wa=2, wb=2))
    return out


def k_loop_specs():
    out = []
    for K in K_LIST:
        w = 4 if K % 4 == 0 else 1
        for lay in ("nt", "tn"):
            M, N, _ = small_dims(lay, w, w, K)
            out += [spec(M, N, K, lay, np_, w, w) for np_ in (3, 1)]
    return out


SPLIT_SHAPES = ((64, 40, 520, "tn", 4), (65, 40, 520, "tn", 1), (129, 131, 545, "nn", 1), (200, 125, 1040, "tn", 1), (512, 512, 1040, "nt", 4))


def split_specs():
    return [spec(M, N, K, lay, wa=w, wb=w) for M, N, K, lay, w in SPLIT_SHAPES]


def _al(N):
    """the smallest pad > 0 that makes N + pad a multiple of 4"""
    return 4 - N % 4


def epilogue_specs():
    """A designed subset of bias x GELU x c_scale (rpm 1, 5) x residual on (130, 70, 97) unsplit [x3_tile] and (65, 40, 520) split
    [x3_reduce_body]: every option in the 16-byte form (every base and pitch aligned; c_scale at N = 72 / 40) and in the element-wise
    form, forced in turn by ldc odd, C base + 1 float, ldr odd, a bias base + 1 float, N % 4 != 0 with c_scale, and the last partial
    column group (N = 70 / 42); then the x3 encoder's two forms on the 256 tile."""
    out = []
    for M, N, K, lay, Nv, Ne in ((130, 70, 97, "nt", 72, 70), (65, 40, 520, "tn", 40, 42)):
        def e(N_, **kw):
            kw.setdefault("cpad", _al(N_))
            kw.setdefault("rpad", _al(N_) + 4)
            return spec(M, N_, K, lay, wa=1, wb=1, **kw)
        out += [e(N, bias=True), e(N, bias=True, gelu=True), e(N, res=True), e(N, bias=True, gelu=True, res=True),
                e(Nv, cs=True, rpm=1), e(Nv, bias=True, cs=True, rpm=5, res=True), e(Nv, bias=True, gelu=True, cs=True, rpm=5),
                e(N, bias=True, res=True, cpad=_al(N) + 1), e(N, bias=True, gelu=True, coff=1), e(N, bias=True, res=True, rpad=_al(N) + 3),
                e(N, bias=True, biasoff=1), e(Ne, bias=True, res=True), e(Ne, bias=True, cs=True, rpm=5),
                e(Ne, bias=True, gelu=True, cs=True, rpm=1, res=True)]
    out += [spec(*BIG, "nt", bias=True, gelu=True), spec(*BIG, "nt", bias=True, res=True)]
    return out


def mask_specs():
    out = []
    for w, K in ((4, 36), (2, 34), (1, 33)):
        for rpm in (1, 3, 7):
            M = {1: 131, 3: 132, 7: 133}[rpm]
            out.append(spec(M, 71, K, "nt", wa=w, wb=w, msk=1, rpm=rpm))                     # a_keep, the forward form
            Kb = {1: 97, 3: 99, 7: 98}[rpm]
            Mb, Nb = {4: (132, 72), 2: (130, 70), 1: (131, 71)}[w]
            out.append(spec(Mb, Nb, Kb, "tn", wa=w, wb=w, msk=2, rpm=rpm))                   # b_keep, the dW form
    out.append(spec(132, 71, 36, "nt", wa=4, wb=4, msk=1, rpm=3, moff=1))                    # a mask base off by a byte: width 1
    out.append(spec(132, 72, 99, "tn", wa=4, wb=4, msk=2, rpm=3, moff=1))
    out.append(spec(132, 71, 36, "nt", wa=4, wb=4, msk=1, rpm=3, moff=2))                    # ... by two: width 2
    out += [spec(132, 72, 36, "nn", wa=4, wb=4, msk=1, rpm=3), spec(132, 72, 99, "nn", wa=4, wb=4, msk=2, rpm=3)]
    out += [spec(*BIG, "nt", wa=4, wb=4, msk=1, rpm=1), spec(*BIG2, "nt", wa=2, wb=2, msk=1, rpm=3)]
    return out


def x1_specs():
    return [spec(130, 70, 97, lay, 1, 1, 1) for lay in ("nt", "nn", "tn", "tt")] + [spec(64, 40, 520, "tn", 1, 4, 4), spec(*BIG, "nt", 1)]


BF16_TN_ROWS = (520, 1040)              # ruart_gemm_bf16_tn: C (64, 40) = A^T B over that many rows


def bf16_tn_specs():
    return [spec(64, 40, rows, "tn", 1, 4, 4) for rows in BF16_TN_ROWS]


def grouped_problems():
    """[(M, N, K, class, accumulate)] of the grouped launch: 45 problems of class 3 (both operands 16-byte loadable) - more than
    X3G_MAX, so that class launches twice - and one of each other class (class bit 0: A loadable, bit 1: B), K cycling so that unsplit
    problems (K = 40) sit between split ones and at the end, accumulate on some of each"""
    out = []
    ks = (520, 40, 1040, 40, 545, 520, 40)
    for i in range(45):
        M = 8 + 4 * ((i * 7) % 34)                  # 8 .. 140, multiples of 4
        N = 4 + 4 * ((i * 5) % 32)                  # 4 .. 128
        out.append((M, N, ks[i % 7], 3, int(i % 3 == 1)))
    out[3] = (140, 128, 1040, 3, 1)
    out[44] = (12, 8, 40, 3, 1)                     # the last of its launch: unsplit, accumulating
    out += [(137, 130, 545, 0, 1), (64, 41, 520, 1, 0), (35, 64, 40, 2, 1)]
    return out


def grouped_spec(prob):
    M, N, K, cls, acc = prob
    return spec(M, N, K, "tn", 3, 4 if cls & 1 else 1, 4 if cls & 2 else 1, res=bool(acc))


def all_specs():
    """every single-launch case of tests/test_gpu_x3_gemm.py that is held to the bounds"""
    return (instantiation_specs() + k_loop_specs() + split_specs() + epilogue_specs() + mask_specs() + x1_specs() + bf16_tn_specs()
            + [grouped_spec(p) for p in grouped_problems()])


def emulation_keys():
    """the distinct (data key, np, tm, splitk, accumulate) behind all_specs, with the unsplit fallback of every split plan"""
    seen, out = set(), []
    grouped = {grouped_spec(p) for p in grouped_problems()}
    for s in all_specs():
        tm, sk = planned(s)
        for k in {sk, 1}:
            key = (data_key(s), s.np, tm, k, s in grouped and s.res)
            if key not in seen:
                seen.add(key)
                out.append(key)
    return out


def controls():
    """(emulation key, defect) of every negative control that can show"""
    out = []
    for key in emulation_keys():
        dk, np_, tm, sk, acc = key
        c = x3_case(*dk)
        out += [(key, d) for d in DEFECTS if x3_defect_shows(c, d, np_, sk, acc)]
    return out


def key_id(key):
    dk, np_, tm, sk, acc = key
    M, N, K, bias, gelu, cs, res, msk, rpm = dk
    flags = "".join(f for f, on in (("b", bias), ("g", gelu), ("c", cs), ("r", res), ("A", msk == 1), ("B", msk == 2), ("+", acc)) if on)
    return "%dx%dx%d-x%d-t%d-s%d-rpm%d-%s" % (M, N, K, np_, tm, sk, rpm, flags or "plain")


def spec_id(s):
    return "%dx%dx%d-%s-x%d-a%d.%d-b%d.%d-%s%s%s%s-m%d.%d.%d-%s-c%d.%d.%d.%d" % (
        s.M, s.N, s.K, s.lay, s.np, s.aoff, s.apad, s.boff, s.bpad, "b" if s.bias else "", "g" if s.gelu else "", "c" if s.cs else "",
        "r" if s.res else "", s.msk, s.rpm, s.moff, s.ws, s.coff, s.cpad, s.rpad, s.biasoff)
