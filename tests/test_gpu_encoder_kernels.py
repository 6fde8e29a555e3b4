"""The frozen encoder's attention and row kernels (csrc/bert_kernels.hip), each called by name through the C ABI and held to a float64
reference of the same operation at bounds derived from the reference and the number formats (tests/_encoder_ref.py; proven on the CPU,
negative controls included, by tests/test_encoder_ref.py).  Descriptors are the ones PackedTokens plans.  Every test prints its worst
error / bound ratio before it asserts (profiles/encoder_kernel_tests.txt holds the measured values)."""
import ctypes
import os

import numpy as np
import pytest
import torch

from ruart_amd import hip
from tests import _encoder_ref as E

pytestmark = pytest.mark.gpu

INVALID = 1                      # hipErrorInvalidValue: what an entry point returns for arguments it refuses before launching
DT = {"f32": hip.DT_F32, "bf16": hip.DT_BF16, "f16": hip.DT_F16}
_ID = lambda c: "%s-%s-H%d-q%s" % c          # noqa: E731


def dev():
    return torch.device("cuda:0")


def test_library_shifts_are_the_header_values():
    assert hip.f16c_shifts() == E.header_shifts()


# ---------------------------------------------------------------------------------------------------------
# attention
# ---------------------------------------------------------------------------------------------------------


def _device_rows(x, rows, ld, dtype, d):
    """(rows, ld) device tensor of ``dtype``: NaN everywhere but [:T, :width] = x (pad columns and pad rows must never reach a result)"""
    buf = torch.full((rows, ld), float("nan"), dtype=dtype)
    buf[:x.shape[0], :x.shape[1]] = x.to(dtype)
    return buf.to(d)


def _run_attention(kind, c, p, x, ld=None, ldc=None):
    """one launch of the kernel of ``kind`` on case ``c`` with the device plan ``p``; returns the raw output buffers on the CPU"""
    lib, d = hip.load(), dev()
    H, NH, Tp = c.H, c.n_heads, c.Tp
    ld, ldc = ld or 3 * H, ldc or H
    blk = [hip.ptr(t) for t in p.blk]
    lblk = [hip.ptr(t) if p.n_long_blocks else None for t in p.lblk]
    xd = _device_rows(x, Tp, ld, E.TORCH_TYPE[kind], d)
    if kind == "split":
        c16 = torch.full((Tp, ldc), float("nan"), dtype=torch.float16, device=d)
        c8 = torch.full((Tp, 2 * ldc), 0x7f, dtype=torch.uint8, device=d)
        rc = lib.ruart_bert_attention_split(hip.ptr(xd), ld, hip.ptr(c16), hip.ptr(c8), ldc, H, NH, p.n_blocks, *blk, hip.ptr(p.tok_lo),
                                            hip.ptr(p.tok_hi), hip.ptr(p.key_bias), hip.stream_ptr())
        assert rc == 0
        torch.cuda.synchronize()
        return c16.cpu(), c8.cpu()
    ctx = torch.full((Tp, ldc), float("nan"), dtype=E.TORCH_TYPE[kind], device=d)
    rc = lib.ruart_bert_attention(hip.ptr(xd), ld, hip.ptr(ctx), ldc, DT[kind], H, NH, p.n_blocks, *blk, hip.ptr(p.tok_lo), hip.ptr(p.tok_hi),
                                  hip.ptr(p.key_bias), p.n_long_blocks, *lblk, hip.stream_ptr())
    assert rc == 0
    torch.cuda.synchronize()
    return ctx.cpu(), None


def _check_attention(kind, c, out, out8, ldc, tag):
    """valid rows written and inside the bound, everything else still the sentinel; returns the worst error / bound"""
    T, H = c.T, c.H
    if kind == "split":
        sa_lo, sa_hi, _, _ = hip.f16c_shifts()
        b8 = out8.view(-1, 2 * ldc)
        assert bool(torch.isnan(out[T:]).all()) and bool(torch.isnan(out[:T, H:]).all())
        assert bool((b8[T:] == 0x7f).all()) and bool((b8[:T, 2 * H:] == 0x7f).all())         # pad rows, and the bytes past [lo8 | hi8]
        assert not bool(torch.isnan(out[:T, :H]).any())
        fine, coarse = E.split_decode(out[:T].numpy(), b8[:T].numpy(), H, sa_lo, sa_hi)
        assert not np.isnan(fine).any() and not np.isnan(coarse).any()
        got = torch.from_numpy(fine)
        h8 = float(((torch.from_numpy(coarse) - c.ref).abs() / E.hi8_bound(c.ref)).max())
        print("%s: hi8 half worst error / one e4m3 step %.3f" % (tag, h8))
        assert h8 <= 1.0
    else:
        assert bool(torch.isnan(out[T:]).all()) and bool(torch.isnan(out[:T, H:]).all())
        assert not bool(torch.isnan(out[:T, :H]).any())
        got = out[:T, :H].double()
    r = float(((got - c.ref).abs() / E.attention_bound(c, kind)).max())
    print("%s: worst error / bound %.3f" % (tag, r))
    assert r <= 1.0
    return r


def _split_kernel_is_the_default():
    """the split cases are about the library's default choice of kernel (two heads per workgroup where 2 divides the head count, else
    the one-head kernel): RUART_ATTN_SPLIT_HEADS / RUART_ATTN_SPLIT_VALU in the environment would run another one and prove nothing"""
    assert "RUART_ATTN_SPLIT_HEADS" not in os.environ and "RUART_ATTN_SPLIT_VALU" not in os.environ and "RUART_HIP_LIB" not in os.environ
    hip.check(hip.load().ruart_bert_attention_split_set_heads(2), "set_heads")          # the default, whatever an earlier test left


@pytest.mark.parametrize("case", E.attention_cases(), ids=_ID)
def test_attention_against_float64(case):
    """ruart_bert_attention_split (kind "split": at the default heads-per-workgroup setting, H = 128 / 192 / 768 take the two-head form,
    the one-head kernel - 2 does not divide 3 - and the production width) and ruart_bert_attention (f32: attn_varlen_kernel<float>;
    f16 / bf16: attn_flash_kernel and, for sequences over 64, attn_flash_long_kernel) against float64 softmax(Q K^T + bias) V, element by
    element at the bound of tests/_encoder_ref.py.  Layouts: short windows; long sequences (16-bit: 11 blocks of <= 128 queries, last
    ATTN_QGROUP group of 3, partial query blocks and partial last key tiles; split / fp32: 64-query blocks over several key tiles);
    pack=False with ragged masks as the -10000 key bias.  Under a bias the result must not depend on the biased keys' V rows at all:
    their probabilities are exactly 0."""
    kind, layout, H, scale = case
    _split_kernel_is_the_default()
    c = E.attention_case(layout, H, scale, E.in_type_of(kind))
    p = E.packed_tokens(layout, kind in E.UNIT, dev())
    if layout == "long":
        assert (p.n_long_blocks, p.n_blocks) == ((11, 2) if kind in E.UNIT else (0, 22))
    assert (p.key_bias is not None) == layout.startswith("bias")
    out, out8 = _run_attention(kind, c, p, c.x)
    _check_attention(kind, c, out, out8, H, "attention " + _ID(case))
    if c.bias is not None:
        x2 = c.x.clone()
        dead = c.bias < 0
        x2[dead, 2 * H:] = x2[dead, 2 * H:] * -3.0 + 100.0
        out2, out82 = _run_attention(kind, c, p, x2)
        assert torch.equal(out2[:c.T].view(torch.int16 if out.element_size() == 2 else torch.int32),
                           out[:c.T].view(torch.int16 if out.element_size() == 2 else torch.int32))
        if out8 is not None:
            assert torch.equal(out82, out8)


@pytest.mark.parametrize("kind", ["split", "f32", "f16", "bf16"])
def test_attention_row_strides(kind):
    """ld = 3H + 8 and ldc = H + 8 (short windows and - 16-bit - long blocks in one call): every valid row is written and inside the bound,
    the pad columns and the rows >= T keep their sentinel (NaN, 0x7f for bytes), NaN pad columns / rows of the input reach no result"""
    H, scale = 128, 0.3
    _split_kernel_is_the_default()
    c = E.attention_case("mixed", H, scale, E.in_type_of(kind))
    p = E.packed_tokens("mixed", kind in E.UNIT, dev())
    assert p.n_blocks > 0 and (p.n_long_blocks > 0) == (kind in E.UNIT)
    out, out8 = _run_attention(kind, c, p, c.x, ld=3 * H + 8, ldc=H + 8)
    _check_attention(kind, c, out, out8, H + 8, "attention strides %s" % kind)


def test_attention_refusals():
    """arguments the entry points reject before they launch anything (every pointer handed over is valid all the same)"""
    lib, d = hip.load(), dev()
    H = 128
    c = E.attention_case("mixed", H, 0.3, "f32")
    p = E.packed_tokens("mixed", False, d)
    pl = E.packed_tokens("mixed", True, d)
    x = torch.zeros(c.Tp, 3 * H, device=d)
    c16 = torch.zeros(c.Tp, H + 8, dtype=torch.float16, device=d)
    c8 = torch.zeros(c.Tp, 2 * (H + 8), dtype=torch.uint8, device=d)
    blk = [hip.ptr(t) for t in p.blk]

    def split(ctx16=c16, ctx8=c8, ldc=H, n_heads=2, n_blocks=p.n_blocks):
        return lib.ruart_bert_attention_split(hip.ptr(x), 3 * H, hip.ptr(ctx16), hip.ptr(ctx8), ldc, H, n_heads, n_blocks, *blk, hip.ptr(p.tok_lo),
                                              hip.ptr(p.tok_hi), None, hip.stream_ptr())
    assert split(n_heads=3) == INVALID and split(ldc=H + 2) == INVALID and split(n_blocks=0) == INVALID
    assert split(ctx16=None) == INVALID and split(ctx8=None) == INVALID
    ctx = torch.zeros(c.Tp, H, device=d)
    lblk = [hip.ptr(t) for t in pl.lblk]

    def plain(dtype=hip.DT_F32, n_heads=2, n_blocks=p.n_blocks, n_long=0):
        return lib.ruart_bert_attention(hip.ptr(x), 3 * H, hip.ptr(ctx), H, dtype, H, n_heads, n_blocks, *blk, hip.ptr(p.tok_lo), hip.ptr(p.tok_hi),
                                        None, n_long, *lblk, hip.stream_ptr())
    assert plain(n_heads=3) == INVALID and plain(n_blocks=0) == INVALID and plain(n_blocks=-1) == INVALID
    assert plain(n_long=pl.n_long_blocks) == INVALID and plain(n_blocks=0, n_long=pl.n_long_blocks) == INVALID        # long blocks are 16-bit only
    assert plain(n_long=-1) == INVALID
    torch.cuda.synchronize()
    assert float(ctx.abs().max()) == 0.0 and float(c16.abs().max()) == 0.0


# ---------------------------------------------------------------------------------------------------------
# LayerNorm rows
# ---------------------------------------------------------------------------------------------------------
LN_ROWS = (1, 5, 37)


def _ordered(t):
    return t.view(torch.int16).to(torch.int32)


def _check_ln_outputs(tag, outs, ref, cpu_out, rows, H, ldo, beta, exact_rows):
    """outs: {"f32", "bf16", "f16", "s32", "s16", "s8"} device buffers of rows + 3 rows, ldo columns (s8: 2 ldo), sentinel-filled"""
    from ruart_amd.bert import split_f16c
    allow, cpu_err = E.layernorm_allowance(cpu_out, ref)
    worst = 0.0
    for k in ("f32", "s32"):
        o = outs[k].cpu()
        assert bool(torch.isnan(o[rows:]).all()) and bool(torch.isnan(o[:rows, H:]).all())
        err = float((o[:rows, :H].double() - ref).abs().max())
        worst = max(worst, err / allow)
        for r in exact_rows:
            assert torch.equal(o[r, :H], beta), (tag, k, r)
    assert torch.equal(outs["f32"].cpu()[:rows, :H], outs["s32"].cpu()[:rows, :H])          # one row routine, two stores
    print("%s: out32 worst error %.3g = %.3f of the allowance %.3g (fp32 formula on the CPU: %.3g)" % (tag, worst * allow, worst, allow, cpu_err))
    assert worst <= 1.0
    for k in ("f16", "bf16"):
        o = outs[k].cpu()
        assert bool(torch.isnan(o[rows:]).all()) and bool(torch.isnan(o[:rows, H:]).all())
        ref16 = torch.from_numpy(ref.numpy().astype(np.float16)) if k == "f16" else ref.to(torch.bfloat16)
        ulps = (o[:rows, :H].double() - ref16.double()).abs().numpy() / E.ulp_of(ref16.double().numpy(), k)
        print("%s: %s worst error %.2f ulp, %.4f %% of the elements differ from the rounded float64 value" % (tag, k, ulps.max(), 100.0 * (ulps > 0).mean()))
        assert ulps.max() <= 1.0
        for r in exact_rows:
            assert torch.equal(_ordered(o[r, :H]), _ordered(beta.to(o.dtype))), (tag, k, r)
    s32, s16, s8 = outs["s32"].cpu(), outs["s16"].cpu(), outs["s8"].cpu()
    assert bool(torch.isnan(s16[rows:]).all()) and bool(torch.isnan(s16[:rows, H:]).all())
    assert bool((s8[rows:] == 0x7f).all()) and bool((s8[:rows, 2 * H:] == 0x7f).all())
    h16, h8 = split_f16c(s32[:rows, :H].contiguous())
    assert torch.equal(_ordered(h16), _ordered(s16[:rows, :H])) and torch.equal(h8, s8[:rows, :2 * H])
    return worst


def _ln_buffers(rows, ldo, d):
    nan = lambda dt: torch.full((rows + 3, ldo), float("nan"), dtype=dt, device=d)       # noqa: E731
    return {"f32": nan(torch.float32), "bf16": nan(torch.bfloat16), "f16": nan(torch.float16), "s32": nan(torch.float32),
            "s16": nan(torch.float16), "s8": torch.full((rows + 3, 2 * ldo), 0x7f, dtype=torch.uint8, device=d)}


@pytest.mark.parametrize("H", [4, 132, 256, 768, 1024])
@pytest.mark.parametrize("kind", E.LN_INPUTS)
def test_rows_layernorm_plain_and_split(H, kind):
    """ruart_rows_layernorm (fp32 / bf16 / f16 output) and ruart_rows_layernorm_split on 1, 5 and 37 rows (never a multiple of the four rows
    of a workgroup), ldx = H + 4, ldo = H + 8: out32 within 4 x the error of the fp32 formula on the CPU (floor 2^-22 max|ref|) of float64;
    16-bit outputs within one ulp of the rounded float64 value; the split triple the split of out32 bit for bit; all-zero and constant
    rows give beta bit for bit; pad columns and the rows past the last keep their sentinel.  The rows of mean 30, std 1 are what the
    compensated mean of ln_row_finish is for: with the plain fp32 row sum their f16 outputs were up to 8 ulp off
    (profiles/encoder_kernel_tests.txt)."""
    lib, d = hip.load(), dev()
    g = torch.Generator().manual_seed(H + 1)
    gamma, beta = 1 + 0.1 * torch.randn(H, generator=g), 0.1 * torch.randn(H, generator=g)
    gd, bd = gamma.to(d), beta.to(d)
    ldx, ldo = H + 4, H + 8
    for rows in LN_ROWS:
        x = E.layernorm_rows(kind, rows, H, seed=H + rows)
        ref = E.layernorm_ref(x, gamma, beta)
        xd = _device_rows(x, rows, ldx, torch.float32, d)
        outs = _ln_buffers(rows, ldo, d)
        for k in ("f32", "bf16", "f16"):
            assert lib.ruart_rows_layernorm(hip.ptr(xd), ldx, hip.ptr(gd), hip.ptr(bd), E.LN_EPS, hip.ptr(outs[k]), ldo, DT[k], rows, H,
                                            hip.stream_ptr()) == 0
        assert lib.ruart_rows_layernorm_split(hip.ptr(xd), ldx, hip.ptr(gd), hip.ptr(bd), E.LN_EPS, hip.ptr(outs["s32"]), hip.ptr(outs["s16"]),
                                              hip.ptr(outs["s8"]), ldo, rows, H, hip.stream_ptr()) == 0
        torch.cuda.synchronize()
        exact = list(range(min(rows, 2))) if kind == "exact" else []
        _check_ln_outputs("rows_layernorm %s H=%d rows=%d" % (kind, H, rows), outs, ref, E.layernorm_fp32(x, gamma, beta), rows, H, ldo, beta, exact)


@pytest.mark.parametrize("H", [4, 132, 256, 768, 1024])
@pytest.mark.parametrize("kind", E.LN_INPUTS)
def test_embed_ln_plain_and_split(H, kind):
    """ruart_bert_embed_ln and ruart_bert_embed_ln_split: LayerNorm of (word[id] + position[pos]) + type[0], the row form's four inputs
    built from the tables and the row form's bounds; ids / positions include row 0 and the last row of their tables and repeat.
      randn     randn tables, against the float64 sum and LayerNorm
      outlier   the same with one entry of 400 in the word row that row 0 reads
      exact     all three tables on a 2^-16 grid (every three-term sum is exact in fp32), position row 0 zero, one word row -type[0]
                (row 0 sums to all zero) and one 0.5 - type[0] (row 1 to the constant 0.5): out32 must equal beta bit for bit through
                the gather and the three-table add.  (With only type[0] on the grid the case's other, random rows carry the fp32
                additions' 2^-24 |x|: at 37 rows, H = 768 two bf16 outputs near zero came out 2 ulp off the rounded
                float64 value.  A 16-bit ulp near zero is finer than fp32 arithmetic on O(1) inputs; the one-ulp
                bound holds on these seeded inputs and is not a property an fp32 LayerNorm has for every output that close to zero.)
      offset30  word table randn + 30, free entries.  Reference: the float64 LayerNorm of the fp32 sum (word + position) + type[0], taken
                on the CPU in the kernel's order (three IEEE additions: the same bits).  Against the float64 SUM the fp32 additions alone
                (2^-24 * 30 per element, as in the reference model, which adds the same fp32 tables) put outputs near zero 2-4 f16 ulp
                off: measured (profiles/encoder_kernel_tests.txt) and not the LayerNorm's doing, which is what this case is about."""
    lib, d = hip.load(), dev()
    g = torch.Generator().manual_seed(7 * H + E.LN_INPUTS.index(kind))
    V, P = 50, 40
    word, ptab, ttab = torch.randn(V, H, generator=g), torch.randn(P, H, generator=g), torch.randn(2, H, generator=g)
    if kind == "offset30":
        word += 30.0
    elif kind == "outlier":
        word[V - 1, H // 3] = 400.0
    elif kind == "exact":
        word, ptab, ttab = ((t * 65536.0).round() / 65536.0 for t in (word, ptab, ttab))
        ptab[0] = 0.0
        word[V - 1] = -ttab[0]
        word[0] = 0.5 - ttab[0]
        assert torch.equal((word[0] + ptab[0]) + ttab[0], torch.full((H,), 0.5)) and not bool(((word[V - 1] + ptab[0]) + ttab[0]).any())
    gamma, beta = 1 + 0.1 * torch.randn(H, generator=g), 0.1 * torch.randn(H, generator=g)
    wd, pd, td, gd, bd = (t.to(d) for t in (word, ptab, ttab, gamma, beta))
    ldo = H + 8
    for rows in LN_ROWS:
        ids = torch.randint(0, V, (rows,), generator=g)
        pos = torch.randint(0, P, (rows,), generator=g)
        ids[0], pos[0] = V - 1, 0
        if rows > 1:
            ids[1], pos[1] = 0, (0 if kind == "exact" else P - 1)
            ids[2:5] = ids[0]
            pos[2], pos[rows - 1] = P - 1, pos[0]
        x32 = (word[ids] + ptab[pos]) + ttab[0]
        x64 = x32.double() if kind == "offset30" else word.double()[ids] + ptab.double()[pos] + ttab.double()[0]
        ref = E.layernorm_ref(x64, gamma, beta)
        cpu_out = E.layernorm_fp32(x32, gamma, beta)
        idd, posd = ids.int().to(d), pos.int().to(d)
        outs = _ln_buffers(rows, ldo, d)
        for k in ("f32", "bf16", "f16"):
            assert lib.ruart_bert_embed_ln(hip.ptr(idd), hip.ptr(posd), hip.ptr(wd), hip.ptr(pd), hip.ptr(td), hip.ptr(gd), hip.ptr(bd), E.LN_EPS,
                                           hip.ptr(outs[k]), ldo, DT[k], rows, H, hip.stream_ptr()) == 0
        assert lib.ruart_bert_embed_ln_split(hip.ptr(idd), hip.ptr(posd), hip.ptr(wd), hip.ptr(pd), hip.ptr(td), hip.ptr(gd), hip.ptr(bd), E.LN_EPS,
                                             hip.ptr(outs["s32"]), hip.ptr(outs["s16"]), hip.ptr(outs["s8"]), ldo, rows, H, hip.stream_ptr()) == 0
        torch.cuda.synchronize()
        exact = list(range(min(rows, 2))) if kind == "exact" else []
        _check_ln_outputs("embed_ln %s H=%d rows=%d" % (kind, H, rows), outs, ref, cpu_out, rows, H, ldo, beta, exact)


def test_layernorm_refusals():
    lib, d = hip.load(), dev()
    H, rows = 1028, 3
    x = torch.zeros(rows, 1032, device=d)
    gb = torch.zeros(1032, device=d)
    o32 = torch.zeros(rows, 1040, device=d)
    o16 = torch.zeros(rows, 1040, dtype=torch.float16, device=d)
    o8 = torch.zeros(rows, 2080, dtype=torch.uint8, device=d)
    ids = torch.zeros(rows, dtype=torch.int32, device=d)
    st = hip.stream_ptr()

    def ln(H=8, ldo=16, rows=rows):
        return lib.ruart_rows_layernorm(hip.ptr(x), 1032, hip.ptr(gb), hip.ptr(gb), E.LN_EPS, hip.ptr(o32), ldo, hip.DT_F32, rows, H, st)

    def ln_split(H=8, ldo=16, a=o32, b=o16, c=o8):
        return lib.ruart_rows_layernorm_split(hip.ptr(x), 1032, hip.ptr(gb), hip.ptr(gb), E.LN_EPS, hip.ptr(a), hip.ptr(b), hip.ptr(c), ldo, rows, H, st)

    def emb(H=8, ldo=16):
        return lib.ruart_bert_embed_ln(hip.ptr(ids), hip.ptr(ids), hip.ptr(x), hip.ptr(x), hip.ptr(x), hip.ptr(gb), hip.ptr(gb), E.LN_EPS,
                                       hip.ptr(o32), ldo, hip.DT_F32, rows, H, st)

    def emb_split(H=8, ldo=16, a=o32, b=o16, c=o8):
        return lib.ruart_bert_embed_ln_split(hip.ptr(ids), hip.ptr(ids), hip.ptr(x), hip.ptr(x), hip.ptr(x), hip.ptr(gb), hip.ptr(gb), E.LN_EPS,
                                             hip.ptr(a), hip.ptr(b), hip.ptr(c), ldo, rows, H, st)
    for f in (ln, ln_split, emb, emb_split):
        assert f(H=6) == INVALID and f(H=1028, ldo=1040) == INVALID and f(ldo=18) == INVALID, f.__name__
    assert ln(rows=0) == INVALID
    for f in (ln_split, emb_split):
        assert f(a=None) == INVALID and f(b=None) == INVALID and f(c=None) == INVALID, f.__name__
    torch.cuda.synchronize()
    assert float(o32.abs().max()) == 0.0 and int(o8.max()) == 0


# ---------------------------------------------------------------------------------------------------------
# ruart_rows_gather, ruart_cast_f32_to_16, ruart_rows_stats_finish
# ---------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("n", [1, 37])
@pytest.mark.parametrize("slots", [3, 1])
def test_rows_gather(n, slots):
    """dst_k[i] = src_k[rows[i]] for three byte matrices of different widths (16 B; 4 H - over 4096 B, so the lanes go round twice; a 2 H
    byte row), source and destination strides larger than the widths, repeated and descending indices: bit-equal to torch indexing, the
    destination's padding and the rows past n untouched.  slots = 1 ends the list with src1 = NULL."""
    lib, d = hip.load(), dev()
    H, R = 1032, 50
    g = torch.Generator().manual_seed(n)
    widths = (16, 4 * H, 2 * H)
    sp, dp = (48, 4 * H + 32, 2 * H + 16), (32, 4 * H + 16, 2 * H + 48)
    src = [torch.randint(0, 256, (R, s), generator=g, dtype=torch.uint8) for s in sp]
    idx = torch.tensor([R - 1] if n == 1 else ([R - 1 - i for i in range(30)] + [3, 3, 0, R - 1, 3, 7, 7]), dtype=torch.int32)
    assert idx.numel() == n
    srcd = [s.to(d) for s in src]
    dst = [torch.full((n + 2, s), 0x7f, dtype=torch.uint8, device=d) for s in dp]
    idxd = idx.to(d)
    args = []
    for k in range(3):
        args += [hip.ptr(srcd[k]) if k < slots else None, sp[k], hip.ptr(dst[k]) if k < slots else None, dp[k], widths[k]]
    assert lib.ruart_rows_gather(hip.ptr(idxd), n, *args, hip.stream_ptr()) == 0
    torch.cuda.synchronize()
    for k in range(3):
        got = dst[k].cpu()
        if k < slots:
            assert torch.equal(got[:n, :widths[k]], src[k][idx.long(), :widths[k]]), k
            assert bool((got[:n, widths[k]:] == 0x7f).all()) and bool((got[n:] == 0x7f).all()), k
        else:
            assert bool((got == 0x7f).all()), k


def test_rows_gather_refusals():
    lib, d = hip.load(), dev()
    src = torch.zeros(8, 64, dtype=torch.uint8, device=d)
    dst = torch.zeros(8, 64, dtype=torch.uint8, device=d)
    idx = torch.zeros(4, dtype=torch.int32, device=d)

    def call(n=4, rows=idx, s=src.data_ptr(), sp=64, dptr=dst.data_ptr(), dp=64, nbytes=32, s1=None, d1=None, b1=0):
        P = ctypes.c_void_p
        return lib.ruart_rows_gather(hip.ptr(rows), n, P(s), sp, P(dptr), dp, nbytes, P(s1) if s1 else None, 64, P(d1) if d1 else None, 64, b1,
                                     None, 0, None, 0, 0, hip.stream_ptr())
    assert call() == 0
    assert call(nbytes=24) == INVALID and call(nbytes=0) == INVALID and call(sp=40) == INVALID and call(dp=72) == INVALID
    assert call(s=src.data_ptr() + 4) == INVALID and call(dptr=dst.data_ptr() + 8) == INVALID
    assert call(n=0) == INVALID and call(n=-3) == INVALID and call(rows=None) == INVALID and call(s=0) == INVALID and call(dptr=0) == INVALID
    assert call(s1=src.data_ptr(), d1=None, b1=16) == INVALID and call(s1=src.data_ptr(), d1=dst.data_ptr(), b1=20) == INVALID
    torch.cuda.synchronize()


CAST_WRAP_N = 2048 * 256 * 4 + 1028            # past one pass of the 2048-workgroup grid: the grid-stride loop goes round again


@pytest.mark.parametrize("n", [4, 1028, CAST_WRAP_N])
@pytest.mark.parametrize("scale", [1.0, 0.125])
@pytest.mark.parametrize("kind", ["f16", "bf16"])
def test_cast_f32_to_16(kind, scale, n):
    """bit-equal to (x * scale).to(type): values at the f16 overflow edge (65504, the tie 65520, beyond), f16 subnormals and the ties
    around the smallest one, signed zeros; the 8 elements past n keep their sentinel"""
    lib, d = hip.load(), dev()
    g = torch.Generator().manual_seed(n)
    x = torch.randn(n, generator=g) * 10.0 ** torch.randint(-8, 5, (n,), generator=g).float()
    edge = torch.tensor([65504.0, 65519.0, 65520.0, 65536.0, -65520.0, 70000.0, 2.0 ** -24, 2.0 ** -25, 1.5 * 2.0 ** -25, -2.0 ** -25, 6e-8, 3e-5,
                         0.0, -0.0, 2.0 ** -14, 1.0009765625, 1.00048828125]) / scale
    m = min(n, edge.numel())
    x[:m] = edge[:m]
    x = torch.where(x.abs() < 2.0 ** -120, torch.zeros_like(x), x)          # (fp32 subnormals: not an encoder input)
    want = (x * scale).to(E.TORCH_TYPE[kind])
    xd = x.to(d)
    out = torch.full((n + 8,), float("nan"), dtype=E.TORCH_TYPE[kind], device=d)
    assert lib.ruart_cast_f32_to_16(hip.ptr(xd), hip.ptr(out), DT[kind], n, scale, hip.stream_ptr()) == 0
    torch.cuda.synchronize()
    got = out.cpu()
    assert torch.equal(got[:n].view(torch.int16), want.view(torch.int16))
    assert bool(torch.isnan(got[n:]).all())


def test_cast_refusals():
    lib, d = hip.load(), dev()
    x = torch.zeros(16, device=d)
    out = torch.zeros(16, dtype=torch.float32, device=d)
    assert lib.ruart_cast_f32_to_16(hip.ptr(x), hip.ptr(out), hip.DT_F16, 6, 1.0, hip.stream_ptr()) == INVALID
    assert lib.ruart_cast_f32_to_16(hip.ptr(x), hip.ptr(out), hip.DT_F32, 8, 1.0, hip.stream_ptr()) == INVALID


@pytest.mark.parametrize("n_parts", [1, 2, 3, 4])
@pytest.mark.parametrize("rows", [1, 255, 257])
def test_rows_stats_finish(n_parts, rows):
    """(mu, rstd) from fp32 (sum, sumsq) partials against float64 on the SAME partials, at the rounding of the formula
    var = q / H - mu^2 in fp32 (E.stats_bound); slots >= n_parts hold NaN and must be ignored; a constant row whose fp32 variance comes
    out negative must give rstd = 1 / sqrt(eps), not NaN; rows with mean 30, std 1 are held to the same bound.  What the cancelling
    form costs against the rows' true statistics is printed, not asserted."""
    lib, d = hip.load(), dev()
    H = 768
    g = torch.Generator().manual_seed(10 * rows + n_parts)
    x = torch.randn(rows, H, generator=g) * 2 + 0.3
    x[1::3] = torch.randn(x[1::3].shape, generator=g) + 30.0
    const = list(range(0, rows, 64))
    for i, r in enumerate(const):
        x[r] = (1.1, 30.1)[i % 2]
    part = E.stats_partials(x, n_parts)
    forms = E.stats_var_forms_fp32(part, n_parts, H)
    assert (forms[:, const] < 0).all()                      # however the compiler contracts the expression, only the clamp saves these rows
    mu64, rstd64 = E.stats_from_partials(part, n_parts, H)
    dmu, drel = E.stats_bound(part, n_parts, H)
    pd = part.to(d)
    stats = torch.full((rows + 2, 2), float("nan"), device=d)
    assert lib.ruart_rows_stats_finish(hip.ptr(pd), n_parts, rows, 1.0 / H, E.LN_EPS, hip.ptr(stats), hip.stream_ptr()) == 0
    torch.cuda.synchronize()
    got = stats.cpu()
    assert bool(torch.isnan(got[rows:]).all()) and not bool(torch.isnan(got[:rows]).any())
    mu, rstd = got[:rows, 0].double(), got[:rows, 1].double()
    r_mu = float(((mu - mu64).abs() / dmu).max())
    live = torch.ones(rows, dtype=torch.bool)
    live[const] = False
    r_rstd = float((((rstd - rstd64).abs() / rstd64)[live] / drel[live]).max()) if bool(live.any()) else 0.0
    print("rows_stats_finish np=%d rows=%d: mu worst error / bound %.3f, rstd worst error / bound %.3f" % (n_parts, rows, r_mu, r_rstd))
    assert r_mu <= 1.0 and r_rstd <= 1.0
    top = 1.0 / np.sqrt(np.float64(np.float32(E.LN_EPS)))
    assert bool(((rstd[const] - top).abs() <= 2.0 ** -22 * top).all()), rstd[const]
    if rows > 1:
        true_mu = x.double().mean(1)
        true_rstd = 1.0 / torch.sqrt(((x.double() - true_mu[:, None]) ** 2).mean(1) + E.LN_EPS)
        off30 = torch.zeros(rows, dtype=torch.bool)
        off30[1::3] = True
        off30[const] = False
        rel = (rstd - true_rstd).abs() / true_rstd
        print("rows_stats_finish np=%d rows=%d: against the rows' true statistics rstd is off by %.3g (mean 30, std 1 rows), %.3g (mean 0.3, std 2 rows)"
              % (n_parts, rows, float(rel[off30].max()), float(rel[live & ~off30].max())))


def test_rows_stats_finish_refusals():
    lib, d = hip.load(), dev()
    part = torch.zeros(4, 8, device=d)
    stats = torch.zeros(4, 2, device=d)
    st = hip.stream_ptr()
    assert lib.ruart_rows_stats_finish(hip.ptr(part), 0, 4, 1.0, 1e-12, hip.ptr(stats), st) == INVALID
    assert lib.ruart_rows_stats_finish(hip.ptr(part), 5, 4, 1.0, 1e-12, hip.ptr(stats), st) == INVALID
    assert lib.ruart_rows_stats_finish(hip.ptr(part), 2, 0, 1.0, 1e-12, hip.ptr(stats), st) == INVALID
    assert lib.ruart_rows_stats_finish(None, 2, 4, 1.0, 1e-12, hip.ptr(stats), st) == INVALID
    assert lib.ruart_rows_stats_finish(hip.ptr(part), 2, 4, 1.0, 1e-12, None, st) == INVALID
