"""The encoder's dense products (csrc/gemm.hip, csrc/gemm_corr.hip), each called by name through the C ABI and held, element by element,
to a float64 reference of the same operation at the bounds tests/_gemm_ref.py derives from the reference and the number formats (proven
on the CPU, negative controls included, by tests/test_gemm_ref.py).  Every operand has row pitches wider than its width and NaN (0x7f
for e4m3 bytes) in its pad columns and extra rows; every output starts as NaN / 0x7f, must be finite and inside the bound on [:M, :N] and
still the sentinel everywhere else.  Every test prints its worst error / bound ratio before it asserts (profiles/gemm_kernel_tests.txt
holds the measured values)."""
import numpy as np
import pytest
import torch

from ruart_amd import hip
from tests import _encoder_ref as E
from tests import _gemm_ref as G

pytestmark = pytest.mark.gpu

INVALID = 1                      # hipErrorInvalidValue: what an entry point returns for arguments it refuses before launching
DT = {"f32": hip.DT_F32, "bf16": hip.DT_BF16, "f16": hip.DT_F16}
_PID = lambda c: "-".join(str(x) for x in c)          # noqa: E731
# Row pitches.  Widest accesses: operands 16 bytes (LDS-DMA: 8 elements, 16 e4m3 bytes - the byte rows share the 16-bit rows' pitch),
# 16-bit residual / output 8 bytes and fp32 residual / output 16 bytes (four elements either way), split output 8 + 4 + 4 bytes.
PA, PW, PC, PR = 8, 16, 4, 8


def dev():
    return torch.device("cuda:0")


def _pad(x, rows, ld, dtype, d):
    """(rows, ld) device tensor of ``dtype``: NaN everywhere but [:x.rows, :x.cols] = x"""
    buf = torch.full((rows, ld), float("nan"), dtype=dtype)
    buf[:x.shape[0], :x.shape[1]] = x.to(dtype)
    return buf.to(d)


def _pad8(b, rows, pitch, d):
    """(rows, pitch) device bytes: 0x7f (e4m3 NaN) everywhere but the top left = b"""
    buf = torch.full((rows, pitch), 0x7f, dtype=torch.uint8)
    buf[:b.shape[0], :b.shape[1]] = torch.from_numpy(np.ascontiguousarray(b))
    return buf.to(d)


def _out(rows, ld, dtype, d):
    return torch.full((rows, ld), float("nan"), dtype=dtype, device=d)


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def _inside(buf, M, N, tag):
    """[:M, :N] finite, everything else still NaN; returns the valid part as float64"""
    got = buf.cpu()
    assert bool(torch.isnan(got[M:]).all()) and bool(torch.isnan(got[:M, N:]).all()), tag + ": a pad element was written"
    assert bool(torch.isfinite(got[:M, :N].float()).all()), tag + ": an element was not written (or is not finite)"
    return got[:M, :N].double()


def _held(got, ref, bound, tag):
    r = G.worst(got, ref, bound)
    print("%s: worst error / bound %.4f" % (tag, r))
    assert r <= 1.0, tag
    return r


# ---------------------------------------------------------------------------------------------------------
# ruart_gemm_16_nt / _ws
# ---------------------------------------------------------------------------------------------------------


class _Plain:
    """the device operands of a plain_case, padded"""

    def __init__(self, c):
        d = dev()
        t16 = E.TORCH_TYPE[c.dt]
        self.c, self.t16 = c, t16
        self.lda, self.ldw, self.ldc, self.ldr = c.K + PA, c.K + PW, c.N + PC, c.N + PR
        self.A = _pad(c.A, c.M + 3, self.lda, t16, d)
        self.W = _pad(c.W, c.N + 1, self.ldw, t16, d)
        self.bias = c.bias.to(d)
        self.R, self.rdt = None, DT[c.dt]
        if c.res is not None:
            r32 = c.epi == "res_f32_out16"
            self.R = _pad(c.res, c.M + 2, self.ldr, torch.float32 if r32 else t16, d)
            self.rdt = hip.DT_F32 if r32 else DT[c.dt]
        self.act = hip.ACT_GELU if c.gelu else hip.ACT_NONE
        self.odt = torch.float32 if c.out == "f32" else t16

    def run(self, ws=None, nbytes=0, cus=0):
        c, lib = self.c, hip.load()
        C = _out(c.M + 2, self.ldc, self.odt, dev())
        rc = lib.ruart_gemm_16_nt_ws(hip.ptr(self.A), self.lda, hip.ptr(self.W), self.ldw, hip.ptr(self.bias), hip.ptr(self.R), self.ldr, self.rdt,
                                     hip.ptr(C), self.ldc, DT[c.out], c.M, c.N, c.K, self.act, DT[c.dt], hip.ptr(ws), nbytes, cus, hip.stream_ptr())
        assert rc == 0
        torch.cuda.synchronize()
        return C


@pytest.mark.parametrize("case", G.plain_cases(), ids=_PID)
def test_gemm_16_against_float64(case):
    """ruart_gemm_16_nt over the kernels launch_one picks - (128, 384, 64) the 128-tile kernel on one K-tile, (256, 256, 192) the two-stage
    256 kernel on an odd K-tile count, (256, 256, 128) and (512, 768, 256) the four-phase kernel at its shortest loops, (1280, 512, 256)
    five row tiles under GROUP_M 4 (a partial last group) - and the epilogues plain, GELU (16-bit and fp32 out), 16-bit residual -> fp32
    out, fp32 residual -> 16-bit out, in bf16 and f16."""
    c = G.plain_case(*case)
    got = _inside(_Plain(c).run(), c.M, c.N, _PID(case))
    _held(got, c.ref, G.plain_bound(c), "gemm_16 " + _PID(case))


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("epi", ["plain", "res_f32_out16"])
def test_gemm_16_pinned_tile_orders(dt, epi):
    """(1280, 512, 256) with ruart_gemm_set_tile_order pinned to 0 (row-major), 3 (two groups, the last of two panels) and 64 (one group
    taller than the matrix): the walk only moves tiles between workgroups, so every order gives the bits of the default rule's run"""
    lib = hip.load()
    c = G.plain_case(dt, 1280, 512, 256, epi)
    p = _Plain(c)
    base = p.run()
    _held(_inside(base, c.M, c.N, "auto"), c.ref, G.plain_bound(c), "gemm_16 tile order auto %s %s" % (dt, epi))
    try:
        for order in (0, 3, 64):
            assert lib.ruart_gemm_set_tile_order(order) == 0
            C = p.run()
            _inside(C, c.M, c.N, "order %d" % order)
            assert torch.equal(_bits(C[:c.M, :c.N]), _bits(base[:c.M, :c.N])), order
    finally:
        assert lib.ruart_gemm_set_tile_order(-1) == 0


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("epi", G.EPIS)
def test_gemm_16_variants_are_bitwise_equal(dt, epi):
    """variants 0 (128 tile), 3 (two-stage 256), 5 (four-phase) and 7 (one wave per SIMD) at (512, 512, 256): the header says they sum in
    the same order; each is held to the bound and all four give the same bits"""
    lib = hip.load()
    c = G.plain_case(dt, 512, 512, 256, epi)
    p = _Plain(c)
    outs = {}
    try:
        for v in (0, 3, 5, 7):
            assert lib.ruart_gemm_set_variant(v) == 0
            outs[v] = p.run()
    finally:
        assert lib.ruart_gemm_set_variant(5) == 0
    for v, C in outs.items():
        _held(_inside(C, c.M, c.N, "variant %d" % v), c.ref, G.plain_bound(c), "gemm_16 variant %d %s %s" % (v, dt, epi))
    for v in (0, 3, 7):
        assert torch.equal(_bits(outs[v][:c.M, :c.N]), _bits(outs[5][:c.M, :c.N])), v


@pytest.mark.parametrize("case", G.plain_split_cases(), ids=_PID)
def test_gemm_16_tail_split_against_float64(case):
    """ruart_gemm_16_nt_ws at five row tiles: (1280, 256, 768) on 4 CUs - one tail tile in three slices -, (1280, 768, 2048) on 10 - five
    tail tiles (a half-full round, long K) in two -, (1280, 256, 256) on 4 - two slices of two K-tiles; the slices count in the bound's n.
    Bit-identical between two runs, every element written, the workspace size the restated plan's."""
    dt, M, N, K, cus, epi = case
    lib = hip.load()
    c = G.plain_case(dt, M, N, K, epi)
    plan = G.plain_plan(M, N, K, cus)
    nbytes = int(lib.ruart_gemm_16_tail_ws_bytes(M, N, K, cus))
    assert plan[1] > 0 and nbytes == G.tail_bytes(plan)
    ws = torch.full((nbytes // 4,), float("nan"), device=dev())
    p = _Plain(c)
    C1, C2 = p.run(ws, nbytes, cus), p.run(ws, nbytes, cus)
    got = _inside(C1, M, N, _PID(case))
    assert torch.equal(_bits(C1[:M, :N]), _bits(C2[:M, :N]))
    _held(got, c.ref, G.plain_bound(c, plan[2]), "gemm_16 tail split %s S=%d" % (_PID(case), plan[2]))
    single = _inside(p.run(), M, N, "single")
    _held(single, c.ref, G.plain_bound(c), "gemm_16 single launch %s" % _PID(case))
    whole = torch.ones(M, N, dtype=torch.bool)                   # the tiles the plan leaves whole are the single launch's, bit for bit
    for tm, tn in G.split_tiles(M, N, plan, G.plain_walk(M, N, K)[1]):
        whole[256 * tm:256 * tm + 256, 256 * tn:256 * tn + 256] = False
    assert int((~whole).sum()) == plan[1] * 65536 and torch.equal(got[whole], single[whole])


@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_gemm_16_shape_left_alone_is_the_single_launch(dt):
    M, N, K, cus = G.LEFT_ALONE
    lib = hip.load()
    assert int(lib.ruart_gemm_16_tail_ws_bytes(M, N, K, cus)) == 0
    p = _Plain(G.plain_case(dt, M, N, K, "plain"))
    ws = torch.full((64,), float("nan"), device=dev())
    C0, C1 = p.run(), p.run(ws, 256, cus)
    assert torch.equal(_bits(C0[:M, :N]), _bits(C1[:M, :N])) and bool(torch.isnan(ws).all())
    _inside(C1, M, N, "left alone")


# ---------------------------------------------------------------------------------------------------------
# ruart_gemm_16c_nt / _sel / _ws / set_dual
# ---------------------------------------------------------------------------------------------------------


class _Corr:
    """the device operands of a corr_case, padded: A16 / W16 f16 rows and A8 / W8 byte rows of the same pitch in bytes (2 lda, 2 ldw)"""

    def __init__(self, c):
        d = dev()
        self.c = c
        self.lda, self.ldw, self.ldc, self.ldr = c.K + PA, c.K + PW, c.N + PC, c.N + PR
        self.A16 = _pad(torch.from_numpy(c.A16.astype(np.float32)), c.M + 3, self.lda, torch.float16, d)
        self.W16 = _pad(torch.from_numpy(c.W16.astype(np.float32)), c.N + 1, self.ldw, torch.float16, d)
        self.A8, self.W8 = _pad8(c.A8, c.M + 3, 2 * self.lda, d), _pad8(c.W8, c.N + 1, 2 * self.ldw, d)
        self.bias = c.bias.to(d)
        self.R = _pad(c.res, c.M + 2, self.ldr, torch.float32, d) if c.res is not None else None
        self.act = hip.ACT_GELU if c.gelu else hip.ACT_NONE

    def run(self, corr=3, ws=None, nbytes=0, cus=0):
        c, lib, d = self.c, hip.load(), dev()
        C = _out(c.M + 2, self.ldc, torch.float16 if c.gelu else torch.float32, d)
        C8 = torch.full((c.M + 2, 2 * self.ldc), 0x7f, dtype=torch.uint8, device=d) if c.gelu else None
        rc = lib.ruart_gemm_16c_nt_ws(hip.ptr(self.A16), hip.ptr(self.A8), self.lda, hip.ptr(self.W16), hip.ptr(self.W8), self.ldw, hip.ptr(self.bias),
                                      hip.ptr(self.R), self.ldr, hip.ptr(C), self.ldc, hip.ptr(C8), c.M, c.N, c.K, self.act, corr, hip.ptr(ws), nbytes, cus,
                                      hip.stream_ptr())
        assert rc == 0
        torch.cuda.synchronize()
        return C, C8

    def decode(self, C, C8, tag):
        """(decoded output, decoded hi8 half or None) of the valid part, every sentinel checked"""
        c = self.c
        if C8 is None:
            return _inside(C, c.M, c.N, tag), None
        _inside(C, c.M, c.N, tag)
        b8 = C8.cpu()
        assert bool((b8[c.M:] == 0x7f).all()) and bool((b8[:c.M, 2 * c.N:] == 0x7f).all()), tag + ": a pad byte was written"
        sa_lo, sa_hi, _, _ = hip.f16c_shifts()
        fine, coarse = E.split_decode(C.cpu()[:c.M].numpy(), b8[:c.M].numpy(), c.N, sa_lo, sa_hi)
        assert not np.isnan(fine).any() and not np.isnan(coarse).any(), tag
        return torch.from_numpy(fine), torch.from_numpy(coarse)


def _hold_corr(c, got, hi8, slices, tag):
    _held(got, c.ref_a, G.corr_bound(c, slices), tag + " against the function of its bytes")
    _held(got, c.ref_b, G.corr_bound(c, slices, "b"), tag + " against the unrounded product")
    if hi8 is not None:
        _held(hi8, c.ref_a, G.corr_hi8_bound(c, slices), tag + " hi8 half")


@pytest.mark.parametrize("case", G.corr_cases(), ids=_PID)
def test_gemm_16c_against_float64(case):
    """ruart_gemm_16c_nt (through _ws, corr 3): (256, 256, 128) the shortest loops, (512, 768, 256), (1280, 512, 768) five row tiles;
    epilogues plain, fp32 residual, GELU + split out.  Operands: the range-edge row, rows of 4 x magnitude, coherent rows (_gemm_ref).
    Held to (a), the function of the bytes, at the kernel's bound and to (b), the unrounded product, at that plus the format bound.  The
    256 x 128 two-workgroups form (no residual) gives the same bits."""
    lib = hip.load()
    c = G.corr_case(*case)
    p = _Corr(c)
    was = lib.ruart_gemm_16c_set_dual(0)
    try:
        C, C8 = p.run()
        got, hi8 = p.decode(C, C8, _PID(case))
        _hold_corr(c, got, hi8, 0, "gemm_16c " + _PID(case))
        lib.ruart_gemm_16c_set_dual(1)
        D, D8 = p.run()
        p.decode(D, D8, _PID(case) + " dual")
        assert torch.equal(_bits(D[:c.M, :c.N]), _bits(C[:c.M, :c.N])) and (C8 is None or torch.equal(D8, C8))
    finally:
        lib.ruart_gemm_16c_set_dual(was)


@pytest.mark.parametrize("case", G.corr_split_cases(), ids=_PID)
def test_gemm_16c_tail_split_against_float64(case):
    """ruart_gemm_16c_nt_ws on the small split shapes (four slices at K = 768 and 256, the f16 and the fp8 phase as the two slices at
    K = 2048): bound with the slices in n, bit-identical between two runs, every element written, the restated plan's workspace size"""
    M, N, K, cus, epi = case
    lib = hip.load()
    c = G.corr_case(M, N, K, epi)
    plan = G.corr_plan(M, N, K, cus)
    nbytes = int(lib.ruart_gemm_16c_tail_ws_bytes(M, N, K, cus))
    assert plan[1] > 0 and nbytes == G.tail_bytes(plan)
    ws = torch.full((nbytes // 4,), float("nan"), device=dev())
    p = _Corr(c)
    was = lib.ruart_gemm_16c_set_dual(0)
    try:
        C1, C81 = p.run(3, ws, nbytes, cus)
        C2, C82 = p.run(3, ws, nbytes, cus)
    finally:
        lib.ruart_gemm_16c_set_dual(was)
    got, hi8 = p.decode(C1, C81, _PID(case))
    assert torch.equal(_bits(C1[:M, :N]), _bits(C2[:M, :N])) and (C81 is None or torch.equal(C81, C82))
    _hold_corr(c, got, hi8, plan[2], "gemm_16c tail split %s S=%d" % (_PID(case), plan[2]))


def test_gemm_16c_shape_left_alone_is_the_single_launch():
    M, N, K, cus = G.LEFT_ALONE
    lib = hip.load()
    assert int(lib.ruart_gemm_16c_tail_ws_bytes(M, N, K, cus)) == 0
    p = _Corr(G.corr_case(M, N, K, "plain"))
    ws = torch.full((64,), float("nan"), device=dev())
    (C0, _), (C1, _) = p.run(), p.run(3, ws, 256, cus)
    assert torch.equal(_bits(C0[:M, :N]), _bits(C1[:M, :N])) and bool(torch.isnan(ws).all())
    _inside(C1, M, N, "left alone")


@pytest.mark.parametrize("K", [256, 768])
def test_gemm_16c_subsets_of_the_correction_leave_the_bound(K):
    """The negative control that needs no broken kernel: ruart_gemm_16c_nt_sel with corr 0 (none), 1 (a_lo . w_hi only) and 2 (a_hi . w_lo
    only) falls outside the full product's bound against the unrounded reference (b) - settled on the CPU by test_gemm_ref.py, confirmed
    here -, and corr 3 stays inside."""
    c = G.corr_case(*G.SEL_SHAPE[K], "plain")
    p = _Corr(c)
    bound = G.corr_bound(c, 0, "b")
    for corr in (3, 0, 1, 2):
        C, _ = p.run(corr)
        r = G.worst(_inside(C, c.M, c.N, "corr %d" % corr), c.ref_b, bound)
        print("gemm_16c_nt_sel K=%d corr %d against the unrounded product: worst error / corr-3 bound %.3f" % (K, corr, r))
        assert (r <= 1.0) if corr == 3 else (r > 1.0), corr


# ---------------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------------


def _refused(call, base, bad, tag):
    """``call(**base)`` succeeds; with each override of ``bad`` it returns hipErrorInvalidValue"""
    assert call(**base) == 0, tag
    for over in bad:
        assert call(**dict(base, **over)) == INVALID, (tag, over)


def test_gemm_16_refusals():
    """ruart_gemm_16_nt / _ws refuse, before launching: misaligned pitches, pitches below the width, NULL A / W / C, sizes that are not
    positive or not on the tile grid, GELU with a residual, types that do not go together.  The sentinel output stays untouched."""
    lib, d = hip.load(), dev()
    M, N, K = 256, 256, 128
    x = torch.zeros(M, K + 16, dtype=torch.bfloat16, device=d)
    r = torch.zeros(M, N + 8, dtype=torch.float32, device=d)
    bias = torch.zeros(N, device=d)
    C = torch.full((M, N + 8), float("nan"), dtype=torch.bfloat16, device=d)

    def call(A=x, lda=K + 8, W=x, ldw=K + 16, R=None, ldr=N + 8, rdt=hip.DT_F32, Cc=C, ldc=N + 4, odt=hip.DT_BF16, M=M, N=N, K=K, act=hip.ACT_NONE,
             idt=hip.DT_BF16, ws=False):
        args = (hip.ptr(A), lda, hip.ptr(W), ldw, hip.ptr(bias), hip.ptr(R), ldr, rdt, hip.ptr(Cc), ldc, odt, M, N, K, act, idt)
        if ws:
            return lib.ruart_gemm_16_nt_ws(*args, None, 0, 4, hip.stream_ptr())
        return lib.ruart_gemm_16_nt(*args, hip.stream_ptr())
    bad = [dict(lda=K + 4), dict(ldw=K + 4), dict(ldc=N + 2), dict(lda=K - 8), dict(ldw=K - 8), dict(ldc=N - 4), dict(A=None), dict(W=None), dict(Cc=None),
           dict(M=0), dict(M=-256), dict(N=0), dict(K=0), dict(M=100), dict(M=M + 64), dict(N=N + 64), dict(K=K + 32),
           dict(R=r, ldr=N + 2), dict(R=r, ldr=N - 4), dict(R=r, act=hip.ACT_GELU), dict(act=hip.ACT_RELU), dict(idt=hip.DT_F32), dict(odt=hip.DT_F16),
           dict(R=r, rdt=hip.DT_F16)]
    for ws in (False, True):
        _refused(call, dict(ws=ws), bad, "gemm_16_nt ws=%s" % ws)
        assert call(ws=ws, R=r) == 0 and call(ws=ws, act=hip.ACT_GELU) == 0
    torch.cuda.synchronize()
    C[:] = float("nan")
    for over in bad:
        if "Cc" not in over:
            assert call(**over) == INVALID
    torch.cuda.synchronize()
    assert bool(torch.isnan(C).all())


def test_gemm_16c_refusals():
    """ruart_gemm_16c_nt / _sel / _ws: the same classes of argument, plus GELU without C8 / a plain product with one, and the half
    corrections at K % 256 != 0"""
    lib, d = hip.load(), dev()
    M, N, K = 256, 256, 128
    a16 = torch.zeros(M, K + 16, dtype=torch.float16, device=d)
    a8 = torch.zeros(M, 2 * (K + 16), dtype=torch.uint8, device=d)
    r = torch.zeros(M, N + 8, device=d)
    bias = torch.zeros(N, device=d)
    C = torch.full((M, N + 8), float("nan"), device=d)
    C16 = torch.full((M, N + 8), float("nan"), dtype=torch.float16, device=d)
    C8 = torch.full((M, 2 * (N + 8)), 0x7f, dtype=torch.uint8, device=d)

    def call(A16=a16, A8=a8, lda=K + 8, W16=a16, W8=a8, ldw=K + 16, R=None, ldr=N + 8, Cc=C, ldc=N + 4, c8=None, M=M, N=N, K=K, act=hip.ACT_NONE, corr=3,
             entry="ws"):
        args = (hip.ptr(A16), hip.ptr(A8), lda, hip.ptr(W16), hip.ptr(W8), ldw, hip.ptr(bias), hip.ptr(R), ldr, hip.ptr(Cc), ldc, hip.ptr(c8), M, N, K, act)
        if entry == "ws":
            return lib.ruart_gemm_16c_nt_ws(*args, corr, None, 0, 4, hip.stream_ptr())
        if entry == "sel":
            return lib.ruart_gemm_16c_nt_sel(*args, corr, hip.stream_ptr())
        return lib.ruart_gemm_16c_nt(*args, hip.stream_ptr()) if corr == 3 else INVALID
    bad = [dict(lda=K + 4), dict(ldw=K + 4), dict(ldc=N + 2), dict(lda=K - 8), dict(ldw=K - 8), dict(ldc=N - 4), dict(A16=None), dict(A8=None), dict(W16=None),
           dict(W8=None), dict(Cc=None), dict(M=0), dict(M=-256), dict(N=0), dict(K=0), dict(M=M + 128), dict(N=N + 128), dict(K=K + 64),
           dict(R=r, ldr=N + 2), dict(R=r, ldr=N - 4), dict(c8=C8), dict(act=hip.ACT_GELU, Cc=C16), dict(act=hip.ACT_GELU, Cc=C16, c8=C8, R=r),
           dict(act=hip.ACT_GELU, Cc=C16, c8=C8, ldc=N - 4), dict(act=hip.ACT_RELU), dict(corr=1), dict(corr=2), dict(corr=4), dict(corr=-1)]
    for entry in ("ws", "sel", "nt"):
        _refused(call, dict(entry=entry), bad, "gemm_16c " + entry)
        assert call(entry=entry, R=r) == 0 and call(entry=entry, act=hip.ACT_GELU, Cc=C16, c8=C8) == 0
    torch.cuda.synchronize()
    C[:] = float("nan")
    C16[:] = float("nan")
    C8[:] = 0x7f
    for over in bad:
        if "Cc" not in over or over["Cc"] is not None:
            assert call(**over) == INVALID
    torch.cuda.synchronize()
    assert bool(torch.isnan(C).all()) and bool(torch.isnan(C16).all()) and bool((C8 == 0x7f).all())


# ---------------------------------------------------------------------------------------------------------
# the training products
# ---------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("shape", G.TRAIN_SHAPES, ids=_PID)
def test_gemm_16_gelu2_against_float64(dt, shape):
    """ruart_gemm_16_nt_gelu2: H, the pre-activation in the operands' type, and G = gelu of the unrounded fp32 pre-activation, per element"""
    lib, d = hip.load(), dev()
    c = G.plain_case(dt, *shape, "gelu")
    p = _Plain(c)
    Hh, Gg = _out(c.M + 2, p.ldc, p.t16, d), _out(c.M + 2, p.ldc, p.t16, d)
    assert lib.ruart_gemm_16_nt_gelu2(hip.ptr(p.A), p.lda, hip.ptr(p.W), p.ldw, hip.ptr(p.bias), hip.ptr(Hh), hip.ptr(Gg), p.ldc, c.M, c.N, c.K, DT[dt],
                                      hip.stream_ptr()) == 0
    torch.cuda.synchronize()
    bh, bg = G.gelu2_bounds(c)
    tag = "gelu2 %s %s" % (dt, _PID(shape))
    _held(_inside(Hh, c.M, c.N, tag), c.pre, bh, tag + " H")
    _held(_inside(Gg, c.M, c.N, tag), c.ref, bg, tag + " G")


@pytest.mark.parametrize("shape", G.TRAIN_SHAPES, ids=_PID)
def test_gemm_16_gelu_bwd_against_float64(shape):
    """ruart_gemm_16_nt_gelu_bwd with ldh != N: dH and G per element, the strip column sums against the float64 sums of the UNROUNDED dH
    at an fp32 summation bound; without a colpart the two matrices come out the same"""
    lib, d = hip.load(), dev()
    M, N, K = shape
    c = G.gelu_bwd_case(M, N, K)
    lda, ldw, ldh, ldc = K + PA, K + PW, N + 4, N + 8
    dY, Wt = _pad(c.dY, M + 3, lda, torch.bfloat16, d), _pad(c.Wt, N + 1, ldw, torch.bfloat16, d)
    Hh = _pad(c.H, M + 2, ldh, torch.float16, d)
    strips = M // 128
    assert int(lib.ruart_gemm_16_nt_gelu_bwd_ws_floats(M, N)) == strips * N
    outs = []
    for with_col in (True, False):
        dH, Gg = _out(M + 2, ldc, torch.bfloat16, d), _out(M + 2, ldc, torch.bfloat16, d)
        col = torch.full((strips + 1, N), float("nan"), device=d)
        assert lib.ruart_gemm_16_nt_gelu_bwd(hip.ptr(dY), lda, hip.ptr(Wt), ldw, hip.ptr(Hh), ldh, hip.ptr(dH), hip.ptr(Gg), ldc,
                                             hip.ptr(col) if with_col else None, M, N, K, hip.stream_ptr()) == 0
        torch.cuda.synchronize()
        outs.append((dH, Gg, col))
    dH, Gg, col = outs[0]
    tag = "gelu_bwd " + _PID(shape)
    _held(_inside(dH, M, N, tag), c.ref_dh, c.b_dh, tag + " dH")
    _held(_inside(Gg, M, N, tag), c.ref_g, c.b_g, tag + " G")
    _held(_inside(col, strips, N, tag), c.ref_col, c.b_col, tag + " strip column sums")
    assert torch.equal(_bits(outs[1][0][:M, :N]), _bits(dH[:M, :N])) and torch.equal(_bits(outs[1][1][:M, :N]), _bits(Gg[:M, :N]))
    assert bool(torch.isnan(outs[1][2]).all())


def _reduce(part, slab_floats, nz, n_floats, scale, C0):
    """ruart_splitk_reduce over flat slabs: (overwrite, accumulate) results"""
    lib, d = hip.load(), dev()
    over = torch.full((n_floats + 8,), float("nan"), device=d)
    acc = torch.full((n_floats + 8,), float("nan"), device=d)
    acc[:n_floats] = C0
    assert lib.ruart_splitk_reduce(hip.ptr(part), slab_floats, nz, hip.ptr(over), n_floats, scale, 0, hip.stream_ptr()) == 0
    assert lib.ruart_splitk_reduce(hip.ptr(part), slab_floats, nz, hip.ptr(acc), n_floats, scale, 1, hip.stream_ptr()) == 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(over[n_floats:]).all()) and bool(torch.isnan(acc[n_floats:]).all())
    return over[:n_floats].cpu(), acc[:n_floats].cpu()


def _check_slabs(c, part, ldc, tag):
    """every slab inside its bound, pad columns and the slab past the last untouched; then ruart_splitk_reduce over the whole pitched slabs
    (the pad columns reduce to NaN and stay out of [:M, :N]) in its overwrite and accumulate forms"""
    M, N = c.M, c.N
    host = part.cpu()
    assert bool(torch.isnan(host[c.nz]).all())
    for z in range(c.nz):
        _held(_inside(host[z], M, N, tag), c.slabs[z], c.b_slabs[z], "%s slab %d" % (tag, z))
    C0 = torch.zeros(M, ldc)
    C0[:, :N] = c.C0
    over, acc = _reduce(part, M * ldc, c.nz, M * ldc, c.scale, C0.flatten().to(dev()))
    _held(_inside(over.view(M, ldc), M, N, tag), c.ref[0], c.bound[0], tag + " reduced, overwrite")
    _held(_inside(acc.view(M, ldc), M, N, tag), c.ref[1], c.bound[1], tag + " reduced, accumulate")


@pytest.mark.parametrize("case", [x for x in G.splitk_cases() if not x[5]], ids=_PID)
def test_gemm_16_nt_splitk_against_float64(case):
    """ruart_gemm_16_nt_splitk + ruart_splitk_reduce: K = 384 in chunks of 256 (a partial last chunk) and K = 256 in two of 128"""
    dt, M, N, K, kchunk, _ = case
    lib, d = hip.load(), dev()
    c = G.splitk_case(dt, M, N, K, kchunk)
    t16 = E.TORCH_TYPE[dt]
    lda, ldw, ldc = K + PA, K + PW, N + 4
    A, W = _pad(c.A, M + 3, lda, t16, d), _pad(c.W, N + 1, ldw, t16, d)
    part = torch.full((c.nz + 1, M, ldc), float("nan"), device=d)
    assert lib.ruart_gemm_16_nt_splitk(hip.ptr(A), lda, hip.ptr(W), ldw, hip.ptr(part), ldc, M, N, K, kchunk, DT[dt], hip.stream_ptr()) == 0
    torch.cuda.synchronize()
    _check_slabs(c, part, ldc, "nt_splitk " + _PID(case[:5]))


@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_gemm_16_tn_splitk_against_float64(dt):
    """ruart_gemm_16_tn_splitk at T = 384, tchunk = 256, ldp / ldq wider than M / N: the token rows past the 300 real ones are padding as
    the header allows it - zero in P, large and finite in Q - and the result is bitwise what zeros in both give"""
    lib, d = hip.load(), dev()
    M, N, T, tchunk = G.SPLITK_SHAPES[0]
    c = G.splitk_case(dt, M, N, T, tchunk, tn=True)
    t16 = E.TORCH_TYPE[dt]
    ldp, ldq, ldc = M + 8, N + 16, N + 4
    P, Q = _pad(c.A.t(), T + 3, ldp, t16, d), _pad(c.W.t(), T + 3, ldq, t16, d)
    assert float(P[G.TN_REAL:T, :M].float().abs().max()) == 0.0 and float(Q[G.TN_REAL:T, :N].float().min()) >= 2.9e4
    Qz = Q.clone()
    Qz[G.TN_REAL:T, :N] = 0.0
    parts = []
    for q in (Q, Qz):
        part = torch.full((c.nz + 1, M, ldc), float("nan"), device=d)
        assert lib.ruart_gemm_16_tn_splitk(hip.ptr(P), ldp, hip.ptr(q), ldq, hip.ptr(part), ldc, M, N, T, tchunk, DT[dt], hip.stream_ptr()) == 0
        torch.cuda.synchronize()
        parts.append(part)
    _check_slabs(c, parts[0], ldc, "tn_splitk %s" % dt)
    assert torch.equal(_bits(parts[0][:c.nz, :, :N]), _bits(parts[1][:c.nz, :, :N]))


def test_training_product_refusals():
    """ruart_gemm_16_nt_gelu2, _gelu_bwd, _nt_splitk and _tn_splitk refuse misaligned or short pitches, NULL pointers, sizes that are not
    positive or not on the tile grid and types they do not take, before launching"""
    lib, d = hip.load(), dev()
    M, N, K = 256, 256, 128
    x = torch.zeros(M + 128, K + 144, dtype=torch.bfloat16, device=d)
    h = torch.zeros(M, N + 8, dtype=torch.float16, device=d)
    bias = torch.zeros(N, device=d)
    o1 = torch.full((M, N + 8), float("nan"), dtype=torch.bfloat16, device=d)
    o2 = torch.full((M, N + 8), float("nan"), dtype=torch.bfloat16, device=d)
    part = torch.full((2, M, N + 8), float("nan"), device=d)
    st = hip.stream_ptr()

    def gelu2(A=x, lda=K + 8, W=x, ldw=K + 16, H=o1, Gg=o2, ldc=N + 4, M=M, N=N, K=K, dt=hip.DT_BF16):
        return lib.ruart_gemm_16_nt_gelu2(hip.ptr(A), lda, hip.ptr(W), ldw, hip.ptr(bias), hip.ptr(H), hip.ptr(Gg), ldc, M, N, K, dt, st)

    def bwd(A=x, lda=K + 8, W=x, ldw=K + 16, H=h, ldh=N + 4, dH=o1, Gg=o2, ldc=N + 4, M=M, N=N, K=K):
        return lib.ruart_gemm_16_nt_gelu_bwd(hip.ptr(A), lda, hip.ptr(W), ldw, hip.ptr(H), ldh, hip.ptr(dH), hip.ptr(Gg), ldc, None, M, N, K, st)

    def splitk(A=x, lda=K + 8, W=x, ldw=K + 16, P=part, ldc=N + 4, M=M, N=N, K=K, kchunk=128, dt=hip.DT_BF16):
        return lib.ruart_gemm_16_nt_splitk(hip.ptr(A), lda, hip.ptr(W), ldw, hip.ptr(P), ldc, M, N, K, kchunk, dt, st)

    def tn(A=x, lda=M + 8, W=x, ldw=N + 16, P=part, ldc=N + 4, M=M, N=N, K=K, kchunk=128, dt=hip.DT_BF16):
        return lib.ruart_gemm_16_tn_splitk(hip.ptr(A), lda, hip.ptr(W), ldw, hip.ptr(P), ldc, M, N, K, kchunk, dt, st)
    sizes = [dict(M=0), dict(M=-256), dict(N=0), dict(K=0), dict(M=M + 128), dict(N=N + 128), dict(K=K + 64), dict(A=None), dict(W=None),
             dict(lda=K + 4), dict(ldw=K + 4), dict(ldc=N + 2), dict(ldc=N - 4)]
    short = [dict(lda=K - 8), dict(ldw=K - 8)]
    _refused(gelu2, {}, sizes + short + [dict(H=None), dict(Gg=None), dict(dt=hip.DT_F32)], "gelu2")
    _refused(splitk, {}, sizes + short + [dict(P=None), dict(kchunk=0), dict(kchunk=64), dict(dt=hip.DT_F32)], "nt_splitk")
    _refused(tn, {}, sizes + [dict(lda=M - 8), dict(ldw=N - 8), dict(P=None), dict(kchunk=0), dict(kchunk=64), dict(dt=hip.DT_F32)], "tn_splitk")
    _refused(bwd, {}, [dict(M=0), dict(M=M + 128), dict(N=N + 128), dict(K=K + 64), dict(A=None), dict(W=None), dict(H=None), dict(dH=None), dict(Gg=None),
                       dict(lda=K + 4), dict(ldw=K + 4), dict(ldc=N + 2), dict(ldh=N + 2), dict(lda=K - 8), dict(ldw=K - 8), dict(ldc=N - 4), dict(ldh=N - 4),
                       dict(N=0), dict(K=0)], "gelu_bwd")
    torch.cuda.synchronize()
    o1[:], o2[:], part[:] = float("nan"), float("nan"), float("nan")
    for f, bad in ((gelu2, sizes + short), (splitk, sizes + short), (tn, sizes), (bwd, [dict(M=0), dict(lda=K + 4), dict(ldh=N + 2)])):
        for over in bad:
            assert f(**over) == INVALID
    torch.cuda.synchronize()
    assert bool(torch.isnan(o1).all()) and bool(torch.isnan(o2).all()) and bool(torch.isnan(part).all())


# ---------------------------------------------------------------------------------------------------------
# the LayerNorm fold: ruart_gemm_16c_nt_fold / ruart_gemm_16_nt_fold
# ---------------------------------------------------------------------------------------------------------


class _FoldOps:
    """the padded device operands of a fold case (fp16c: A16 / A8 / W16 / W8; 16-bit: A / W)"""

    def __init__(self, c):
        d = dev()
        self.lda, self.ldw, self.ldc, self.ldr = c.K + PA, c.K + PW, c.N + PC, c.N + PR
        o = c.ops
        if c.kind == "c8":
            self.A16 = _pad(torch.from_numpy(o.A16.astype(np.float32)), c.M + 3, self.lda, torch.float16, d)
            self.W16 = _pad(torch.from_numpy(o.W16.astype(np.float32)), c.N + 1, self.ldw, torch.float16, d)
            self.A8, self.W8 = _pad8(o.A8, c.M + 3, 2 * self.lda, d), _pad8(o.W8, c.N + 1, 2 * self.ldw, d)
        else:
            t16 = E.TORCH_TYPE[c.kind]
            self.A, self.W = _pad(o.A, c.M + 3, self.lda, t16, d), _pad(o.W, c.N + 1, self.ldw, t16, d)

    def head(self):
        if hasattr(self, "A16"):
            return (hip.ptr(self.A16), hip.ptr(self.A8), self.lda, hip.ptr(self.W16), hip.ptr(self.W8), self.ldw)
        return (hip.ptr(self.A), self.lda, hip.ptr(self.W), self.ldw)


def _part_dev(part, M):
    """row partials with two extra NaN rows"""
    buf = torch.full((M + 2, 4, 2), float("nan"))
    buf[:M] = part
    return buf.to(dev())


@pytest.mark.parametrize("case", G.consumer_cases(), ids=_PID)
def test_fold_consumer_against_float64(case):
    """kinds 0 / 2 of ruart_gemm_16c_nt_fold ("c8") and ruart_gemm_16_nt_fold (bf16, f16) at (256, 512, 256) and (512, 768, 1024): rows with
    an outlier dimension and a constant row, a gamma with one large gain (fp16c: s = 1), against rstd 2^s (acc - mu c) + d in float64 on
    the stored operands and the same fp32 partials; unused partial slots and the partials' extra rows hold NaN"""
    lib, d = hip.load(), dev()
    c = G.consumer_case(*case)
    o = _FoldOps(c)
    kind = 2 if c.gelu else 0
    part, cv, dv = _part_dev(c.part, c.M), c.cvec.to(d), c.dvec.to(d)
    tag = "fold consumer " + _PID(case)
    if c.kind == "c8":
        C = _out(c.M + 2, o.ldc, torch.float16 if c.gelu else torch.float32, d)
        C8 = torch.full((c.M + 2, 2 * o.ldc), 0x7f, dtype=torch.uint8, device=d) if c.gelu else None
        was = lib.ruart_gemm_16c_set_dual(0)
        try:
            rc = lib.ruart_gemm_16c_nt_fold(*o.head(), hip.ptr(dv), kind, hip.ptr(part), c.np, hip.ptr(cv), float(2.0 ** c.s), None, 0, None, 0, None, None,
                                            hip.ptr(C), o.ldc, None, hip.ptr(C8), None, c.M, c.N, c.K, c.K, G.FOLD_EPS, hip.stream_ptr())
        finally:
            lib.ruart_gemm_16c_set_dual(was)
        assert rc == 0
        torch.cuda.synchronize()
        if c.gelu:
            _inside(C, c.M, c.N, tag)
            b8 = C8.cpu()
            assert bool((b8[c.M:] == 0x7f).all()) and bool((b8[:c.M, 2 * c.N:] == 0x7f).all())
            sa_lo, sa_hi, _, _ = hip.f16c_shifts()
            fine, coarse = E.split_decode(C.cpu()[:c.M].numpy(), b8[:c.M].numpy(), c.N, sa_lo, sa_hi)
            assert not np.isnan(fine).any() and not np.isnan(coarse).any()
            got = torch.from_numpy(fine)
        else:
            got = _inside(C, c.M, c.N, tag)
    else:
        C = _out(c.M + 2, o.ldc, E.TORCH_TYPE[c.kind], d)
        rc = lib.ruart_gemm_16_nt_fold(*o.head(), hip.ptr(dv), kind, hip.ptr(part), c.np, hip.ptr(cv), 1.0, None, 0, None, 0, None, None, hip.ptr(C), o.ldc,
                                       None, c.M, c.N, c.K, c.K, G.FOLD_EPS, DT[c.kind], hip.stream_ptr())
        assert rc == 0
        torch.cuda.synchronize()
        got = _inside(C, c.M, c.N, tag)
    _held(got, c.ref, c.bound, tag)
    live = torch.ones(c.M, dtype=torch.bool)
    live[3] = False                                             # (the constant row's rstd of 1e6 widens its own bound: the others apart)
    _held(got[live], c.ref[live], c.bound[live], tag + ", without the constant row")


@pytest.mark.parametrize("case", G.producer_cases(), ids=_PID)
def test_fold_producer_against_float64(case):
    """kind 3 at (256, 256, 128) and (512, 1024, 256), with and without the residual's LayerNorm: y per element; fp16c: C16 / C8 exactly the
    split of the C written and the row partials against the float64 sums of the C written; 16-bit: the partials of the unrounded y against
    the reference's sums, y's own bound added; unused slots and extra rows untouched"""
    lib, d = hip.load(), dev()
    c = G.producer_case(*case)
    o = _FoldOps(c)
    rtype = torch.float32 if c.kind == "c8" else E.TORCH_TYPE[c.kind]
    R = _pad(c.res, c.M + 2, o.ldr, rtype, d)
    bias, gam, bet = c.bias.to(d), c.gam.to(d), c.bet.to(d)
    rpart = _part_dev(c.part, c.M) if c.res_ln else None
    opart = torch.full((c.M + 2, 4, 2), float("nan"), device=d)
    tag = "fold producer " + _PID(case)
    tail = (hip.ptr(R), o.ldr, hip.ptr(rpart), c.np, hip.ptr(gam), hip.ptr(bet))
    if c.kind == "c8":
        C, C16 = _out(c.M + 2, o.ldc, torch.float32, d), _out(c.M + 2, o.ldc, torch.float16, d)
        C8 = torch.full((c.M + 2, 2 * o.ldc), 0x7f, dtype=torch.uint8, device=d)
        rc = lib.ruart_gemm_16c_nt_fold(*o.head(), hip.ptr(bias), 3, None, 0, None, 1.0, *tail, hip.ptr(C), o.ldc, hip.ptr(C16), hip.ptr(C8), hip.ptr(opart),
                                        c.M, c.N, c.K, c.N, G.FOLD_EPS, hip.stream_ptr())
    else:
        C = _out(c.M + 2, o.ldc, rtype, d)
        rc = lib.ruart_gemm_16_nt_fold(*o.head(), hip.ptr(bias), 3, None, 0, None, 1.0, *tail, hip.ptr(C), o.ldc, hip.ptr(opart), c.M, c.N, c.K, c.N,
                                       G.FOLD_EPS, DT[c.kind], hip.stream_ptr())
    assert rc == 0
    torch.cuda.synchronize()
    got = _inside(C, c.M, c.N, tag)
    _held(got, c.ref, c.bound, tag + " y")
    op = opart.cpu()
    assert bool(torch.isnan(op[c.M:]).all()) and bool(torch.isnan(op[:c.M, c.np:]).all()) and bool(torch.isfinite(op[:c.M, :c.np]).all())
    if c.kind == "c8":
        sa_lo, sa_hi, _, _ = hip.f16c_shifts()
        h16, h8 = E.split_ref(C.cpu()[:c.M, :c.N].numpy(), sa_lo, sa_hi)
        _inside(C16, c.M, c.N, tag + " C16")
        b8 = C8.cpu()
        assert bool((b8[c.M:] == 0x7f).all()) and bool((b8[:c.M, 2 * c.N:] == 0x7f).all())
        assert np.array_equal(C16.cpu()[:c.M, :c.N].numpy().view(np.uint16), h16.view(np.uint16)) and np.array_equal(b8[:c.M, :2 * c.N].numpy(), h8)
        want, pb = G.partial_bounds(got, c.np)
    else:
        want, pb = G.partial_bounds(c.ref, c.np)
        blk = c.pre_bound.view(c.M, c.np, 256)
        pb = pb + torch.stack([blk.sum(2), (2.0 * c.ref.abs().view(c.M, c.np, 256) * blk + blk * blk).sum(2)], 2)
    _held(op[:c.M, :c.np].double(), want, pb, tag + " row partials")


def test_fold_refusals():
    """both fold entries: pitches, NULL pointers, sizes, kinds, slot counts; kinds 0 / 2 of the 16-bit entry need their partials, kind 3
    its residual and out_part, a normalised residual its gamma and beta"""
    lib, d = hip.load(), dev()
    M, N, K = 256, 256, 256
    a16 = torch.zeros(M, K + 16, dtype=torch.float16, device=d)
    a8 = torch.zeros(M, 2 * (K + 16), dtype=torch.uint8, device=d)
    vec = torch.zeros(N, device=d)
    part = torch.zeros(M, 4, 2, device=d)
    r32 = torch.zeros(M, N + 8, device=d)
    r16 = torch.zeros(M, N + 8, dtype=torch.float16, device=d)
    C32 = torch.full((M, N + 8), float("nan"), device=d)
    C16 = torch.full((M, N + 8), float("nan"), dtype=torch.float16, device=d)
    C8 = torch.full((M, 2 * (N + 8)), 0x7f, dtype=torch.uint8, device=d)
    opart = torch.full((M, 4, 2), float("nan"), device=d)
    st = hip.stream_ptr()

    def c8(A16=a16, A8=a8, lda=K + 8, W16=a16, W8=a8, ldw=K + 16, kind=0, ip=part, inp=1, colc=vec, R=None, ldr=N + 8, rp=None, rnp=1, rg=vec, rb=vec, C=C32,
           ldc=N + 4, c16=None, cb=None, op=None, M=M, N=N, K=K, sl=K):
        return lib.ruart_gemm_16c_nt_fold(hip.ptr(A16), hip.ptr(A8), lda, hip.ptr(W16), hip.ptr(W8), ldw, hip.ptr(vec), kind, hip.ptr(ip), inp, hip.ptr(colc),
                                          2.0, hip.ptr(R), ldr, hip.ptr(rp), rnp, hip.ptr(rg), hip.ptr(rb), hip.ptr(C), ldc, hip.ptr(c16), hip.ptr(cb),
                                          hip.ptr(op), M, N, K, sl, 1e-12, st)

    def p16(A=a16, lda=K + 8, W=a16, ldw=K + 16, kind=0, ip=part, inp=1, colc=vec, R=None, ldr=N + 8, rp=None, rnp=1, rg=vec, rb=vec, C=C16, ldc=N + 4,
            op=None, M=M, N=N, K=K, sl=K, dt=hip.DT_F16):
        return lib.ruart_gemm_16_nt_fold(hip.ptr(A), lda, hip.ptr(W), ldw, hip.ptr(vec), kind, hip.ptr(ip), inp, hip.ptr(colc), 1.0, hip.ptr(R), ldr,
                                         hip.ptr(rp), rnp, hip.ptr(rg), hip.ptr(rb), hip.ptr(C), ldc, hip.ptr(op), M, N, K, sl, 1e-12, dt, st)
    common = [dict(lda=K + 4), dict(ldw=K + 4), dict(ldc=N + 2), dict(lda=K - 8), dict(ldw=K - 8), dict(C=None), dict(M=0), dict(M=M + 128), dict(N=N + 128),
              dict(K=K + 64), dict(sl=0), dict(kind=1), dict(kind=4), dict(inp=0), dict(inp=5), dict(colc=None)]
    _refused(c8, {}, common + [dict(A16=None), dict(A8=None), dict(W16=None), dict(W8=None), dict(cb=C8), dict(kind=2), dict(ldc=N - 4), dict(kind=2, C=C16, cb=C8, ldc=N - 4)],
             "16c fold consumer")
    _refused(p16, {}, common + [dict(A=None), dict(W=None), dict(ip=None), dict(dt=hip.DT_F32), dict(ldc=N - 4)], "16 fold consumer")
    prod8 = dict(kind=3, ip=None, R=r32, c16=C16, cb=C8, op=opart, sl=N)
    _refused(c8, prod8, [dict(R=None), dict(c16=None), dict(cb=None), dict(op=None), dict(ldc=N - 4), dict(ldr=N + 2), dict(ldr=N - 4), dict(rnp=5), dict(rp=part, rg=None), dict(rp=part, rb=None),
                         dict(rp=part, rnp=0), dict(N=5 * 256)], "16c fold producer")
    prod16 = dict(kind=3, ip=None, R=r16, op=opart, sl=N)
    _refused(p16, prod16, [dict(R=None), dict(op=None), dict(ldr=N + 2), dict(ldr=N - 4), dict(rnp=5), dict(rp=part, rg=None), dict(rp=part, rb=None), dict(rp=part, rnp=0),
                           dict(N=5 * 256)], "16 fold producer")
    torch.cuda.synchronize()
    C32[:], C16[:], opart[:] = float("nan"), float("nan"), float("nan")
    C8[:] = 0x7f
    for over in common:
        if over.get("C", 0) is not None:
            assert c8(**over) == INVALID and p16(**over) == INVALID, over
    for over in (dict(lda=K + 4), dict(ldw=K - 8), dict(ldc=N + 2), dict(ldr=N + 2), dict(ldr=N - 4), dict(M=0), dict(K=K + 64), dict(rnp=5)):
        assert c8(**dict(prod8, **over)) == INVALID and p16(**dict(prod16, **over)) == INVALID, over
    torch.cuda.synchronize()
    assert bool(torch.isnan(C32).all()) and bool(torch.isnan(C16).all()) and bool((C8 == 0x7f).all()) and bool(torch.isnan(opart).all())
