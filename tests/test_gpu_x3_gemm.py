"""The trunk's split-bf16 products (csrc/sdnet_gemm.hip), each called by name through the C ABI - ruart_gemm_x3, ruart_gemm_x1,
ruart_gemm_bf16_tn, ruart_gemm_x3_tn_grouped - and held, element by element, to two float64 references at the bounds tests/_x3_ref.py
derives: (a) the function of its inputs the kernel computes and (b) the product of the unrounded operands (proven on the CPU, negative
controls included, by tests/test_x3_ref.py).  Every operand has a pitch wider than its rows and NaN in its pads; every output starts as
NaN with ldc > N and two extra rows, must be finite and inside both bounds on [:M, :N] and still NaN everywhere else; a workspace has 64
guard floats behind it; every call is made twice and must give the same bits.  Every test prints its worst error / bound ratios before
it asserts (profiles/x3_kernel_tests.txt holds the measured values)."""
import ctypes

import pytest
import torch

from ruart_amd import hip
from tests import _x3_ref as X
from tests.test_gpu_gemm import INVALID, _bits

pytestmark = pytest.mark.gpu
NAN = float("nan")


def dev():
    return torch.device("cuda:0")


def _addr(t, off_elems=0):
    return ctypes.c_void_p(t.data_ptr() + off_elems * t.element_size()) if t is not None else ctypes.c_void_p(0)


def _operand(x, pitch, off, extra_rows=1):
    """x (rows, ext) -> flat device buffer of NaN holding x at ``off`` floats with row pitch ``pitch``, one NaN row behind it"""
    rows, ext = x.shape
    buf = torch.full((off + (rows + extra_rows) * pitch,), NAN)
    buf[off:off + rows * pitch].view(rows, pitch)[:, :ext] = x
    return buf.to(dev())


def _plan_bytes(M, N, K, am, bm):
    sk, nb = ctypes.c_int(-1), ctypes.c_size_t(1)
    assert hip.load().ruart_gemm_x3_plan(M, N, K, int(am == 0), int(bm == 0), ctypes.byref(sk), ctypes.byref(nb)) == 0
    plan = X.make_plan(M, N, K, am, bm)
    assert (sk.value, nb.value) == (plan[2], X.ws_bytes_of(plan))
    return int(nb.value)


class _Call:
    """the device arguments of a Spec; ``A`` / ``B`` replace the case's operands (the property tests)"""

    def __init__(self, s, A=None, B=None):
        assert X.env_is_default()
        c = X.case_of(s)
        self.s, self.c = s, c
        am, bm = X.modes(s.lay)
        pa, pb = X.pitches(s)
        A, B = (c.A if A is None else A), (c.B if B is None else B)
        self.A = _operand(A if am == 0 else A.t(), pa, s.aoff)
        self.B = _operand(B.t() if bm == 0 else B, pb, s.boff)
        self.sa = (pa, 1) if am == 0 else (1, pa)                    # (sam, sak)
        self.sb = (1, pb) if bm == 0 else (pb, 1)                    # (sbk, sbn)
        d = dev()
        self.bias = self.cs = self.R = self.keep = None
        if c.bias is not None:
            self.bias = torch.full((s.biasoff + s.N + 4,), NAN)
            self.bias[s.biasoff:s.biasoff + s.N] = c.bias
            self.bias = self.bias.to(d)
        if c.cscale is not None:
            self.cs = torch.cat([c.cscale.flatten(), torch.full((4,), NAN)]).to(d)
        if c.res is not None:
            self.R = _operand(c.res, s.N + s.rpad, 0)
        if c.keep is not None:
            self.keep = torch.cat([torch.full((s.moff,), 0xff, dtype=torch.uint8), c.keep.flatten(), torch.full((8,), 0xff, dtype=torch.uint8)]).to(d)
        self.ldc, self.ldr = s.N + s.cpad, s.N + s.rpad
        self.nbytes = _plan_bytes(s.M, s.N, s.K, am, bm)
        self.ws = torch.full((self.nbytes // 4 + 64,), NAN, device=d)

    def run(self, entry=None, **over):
        """one call; returns the flat C buffer.  ``over``: argument overrides by name (the refusal test)"""
        s, lib = self.s, hip.load()
        C = torch.full((s.coff + (s.M + 2) * self.ldc,), NAN, device=dev())
        ws, nb = (_addr(self.ws), self.nbytes) if s.ws == "plan" else ((None, 0) if s.ws == "null" else (_addr(self.ws), self.nbytes - 4))
        a = dict(A=_addr(self.A, s.aoff), sam=self.sa[0], sak=self.sa[1], B=_addr(self.B, s.boff), sbk=self.sb[0], sbn=self.sb[1],
                 bias=_addr(self.bias, s.biasoff), R=_addr(self.R), ldr=self.ldr if self.R is not None else 0,
                 act=hip.ACT_GELU if s.gelu else hip.ACT_NONE, C=_addr(C, s.coff), ldc=self.ldc, M=s.M, N=s.N, K=s.K, ws=ws, nb=nb,
                 a_keep=_addr(self.keep, s.moff) if s.msk == 1 else None, b_keep=_addr(self.keep, s.moff) if s.msk == 2 else None,
                 keep_scale=self.c.keep_scale, cs=_addr(self.cs), rpm=s.rpm)
        a.update(over)
        entry = entry or ("x3" if s.np == 3 else "x1")
        if entry == "bf16_tn":
            rc = lib.ruart_gemm_bf16_tn(a["A"], a["sak"], a["B"], a["sbk"], a["C"], a["ldc"], a["M"], a["N"], a["K"], a["ws"], a["nb"], hip.stream_ptr())
        else:
            fn = lib.ruart_gemm_x3 if entry == "x3" else lib.ruart_gemm_x1
            rc = fn(a["A"], a["sam"], a["sak"], a["B"], a["sbk"], a["sbn"], a["bias"], a["R"], a["ldr"], a["act"], a["C"], a["ldc"], a["M"], a["N"],
                    a["K"], a["ws"], a["nb"], a["a_keep"], a["b_keep"], a["keep_scale"], a["cs"], a["rpm"], hip.stream_ptr())
        torch.cuda.synchronize()
        self.rc = rc
        return C

    def view(self, C, tag, finite=True):
        """the (M, N) result on the host after the sentinel checks: nothing written outside [:M, :N], the workspace guard intact (and
        the whole workspace where the call had none to use)"""
        s = self.s
        host = C.cpu()
        v = host[s.coff:].view(s.M + 2, self.ldc)
        assert bool(torch.isnan(host[:s.coff]).all()) and bool(torch.isnan(v[s.M:]).all()) and bool(torch.isnan(v[:s.M, s.N:]).all()), tag + ": a pad element was written"
        if finite:
            assert bool(torch.isfinite(v[:s.M, :s.N]).all()), tag + ": an element was not written (or is not finite)"
        ws = self.ws.cpu()
        assert bool(torch.isnan(ws[self.nbytes // 4:]).all()), tag + ": a workspace guard float was written"
        if s.ws != "plan":
            assert bool(torch.isnan(ws).all()), tag + ": the workspace was touched"
        return v[:s.M, :s.N].clone()


def _held(got, c, np_, sk, tag):
    """inside bound (a) and bound (b); prints both ratios first"""
    ra = X.worst(got.double(), *X.x3_bound(c, np_, sk, "a"))
    rb = X.worst(got.double(), *X.x3_bound(c, np_, sk, "b"))
    print("%s: worst error / bound %.4f (a) %.4f (b)" % (tag, ra, rb))
    assert ra <= 1.0 and rb <= 1.0, tag
    return ra, rb


def _check(s, tag, entry=None):
    """run ``s`` twice: the sentinels, the same bits, both bounds with the slices the dispatch runs; returns the result"""
    d = X.dispatch(s)
    call = _Call(s)
    C1, C2 = call.run(entry), call.run(entry)
    assert call.rc == 0, tag
    got = call.view(C1, tag)
    assert torch.equal(_bits(got), _bits(call.view(C2, tag))), tag + ": two runs differ"
    _held(got, call.c, s.np, d[6], "%s %s -> tile %d modes %d%d widths %d %d mask %d splitk %d" % ((tag, X.spec_id(s)) + d))
    return got


@pytest.mark.parametrize("s", X.instantiation_specs(), ids=X.spec_id)
def test_every_instantiation(s):
    """one case per kernel instantiation gemm_xn can launch (X.INSTANTIATIONS: 36 of the 128 tile, 8 of the 256 tile, 10 masked), the
    width pair picked by base offset, pitch and extent; the 256 tile also in its split plan at (4, 4) nt and (2, 2) A-transposed"""
    _check(s, "x3 instantiation")


@pytest.mark.parametrize("s", X.k_loop_specs(), ids=X.spec_id)
def test_k_loop_boundaries(s):
    """K across the pair-loop boundaries of the 128 tile - KFULL against the general form, the odd-step tail, the K tail - with partial
    tiles both ways, nt and tn, 16-byte loads where K % 4 == 0 and scalar ones otherwise, x3 and x1"""
    _check(s, "x3 K loop")


@pytest.mark.parametrize("s", X.split_specs(), ids=X.spec_id)
def test_split_k(s):
    """the split plans - slices of 5, 5, 5, 2 steps with the K tail in the last, partial tiles, and the EMPTY eighth slice of K = 1040 (its
    slab must be written, and zero: the workspace starts as NaN) - and the fallback without a workspace or with one 4 bytes short: the
    unsplit product, bit-equal between the two, inside the bound with one slice, workspace untouched"""
    assert X.dispatch(s)[6] > 1
    _check(s, "x3 split")
    alone = [_check(s._replace(ws=w), "x3 split, workspace %s" % w) for w in ("null", "short")]
    assert torch.equal(_bits(alone[0]), _bits(alone[1]))


@pytest.mark.parametrize("s", X.epilogue_specs(), ids=X.spec_id)
def test_epilogues(s):
    """bias, exact-erf GELU, c_scale with rows_per_scale_row 1 and 5, residual with ldr != N: in x3_tile (unsplit) and in x3_reduce_body
    (split), each in the 16-byte and in the element-wise form (X.epilogue_specs); the pad columns of C stay untouched"""
    _check(s, "x3 epilogue (%s form open)" % ("16-byte" if X.epilogue_is_vector(s) else "element-wise only"))


def test_fused_masks():
    """a_keep (forward) and b_keep (dW) at load widths 4, 2 and 1 with the K tail crossing the mask bytes, rows_per_scale_row 1, 3 and 7,
    the (A K-contiguous, B N-contiguous) forms, the 256 tile; a mask base one (two) byte(s) off falls to width 1 (2) and gives the same
    bits.  Reference: multiply first."""
    aligned = {}
    for s in X.mask_specs():
        got = _check(s, "x3 fused mask")
        key = X.data_key(s) + (s.lay,)
        if s.moff == 0:
            aligned[key] = got
        else:
            assert torch.equal(_bits(got), _bits(aligned[key])), X.spec_id(s)


def test_x1_and_bf16_tn():
    """ruart_gemm_x1 in the four layouts, split and on the 256 tile, and ruart_gemm_bf16_tn over 520 and 1040 rows, against F1 = sum ah bh
    and against the unrounded product at the one-product format bound"""
    for s in X.x1_specs():
        _check(s, "x1")
    for s in X.bf16_tn_specs():
        assert X.dispatch(s)[6] > 1
        assert _plan_bytes(s.M, s.N, s.K, 0, 0) == _plan_bytes(s.M, s.N, s.K, 1, 1)          # (the header sizes its workspace from the nt plan)
        got = _check(s, "bf16_tn", "bf16_tn")
        assert torch.equal(_bits(got), _bits(_check(s, "x1 on the same operands")))


def test_grouped_weight_gradients():
    """48 problems in one ruart_gemm_x3_tn_grouped call: 45 of the class with both operands 16-byte loadable - two launches, X3G_MAX is 44 -
    and one of each other class, split (K = 520, 545, 1040) and unsplit (K = 40) in turn, accumulate on some of each over a pre-filled C.
    Every problem is bit-equal to ruart_gemm_x3 alone on the same operands (residual = the C it accumulates into) and inside the
    bounds; pads and the workspace guard stay untouched; two calls give the same bits."""
    lib, d = hip.load(), dev()
    probs = X.grouped_problems()
    calls = [_Call(X.grouped_spec(p)) for p in probs]
    arr = (hip.X3TnProblemC * len(probs))()

    def fill():
        Cs = []
        for q, call, (M, N, K, cls, acc) in zip(arr, calls, probs):
            s = call.s
            C = torch.full((M + 2, call.ldc), NAN)
            if acc:
                C[:M, :N] = call.c.res
            C = C.to(d)
            Cs.append(C)
            q.A, q.B, q.C = _addr(call.A, s.aoff).value, _addr(call.B, s.boff).value, C.data_ptr()
            q.lda, q.ldb, q.ldc, q.M, q.N, q.K, q.accumulate = call.sa[1], call.sb[0], call.ldc, M, N, K, acc
        return Cs
    first = fill()
    nbytes = int(lib.ruart_gemm_x3_tn_grouped_ws(arr, len(probs)))
    assert nbytes == sum(X.ws_bytes_of(X.make_plan(M, N, K, 1, 1)) for M, N, K, _, _ in probs)
    ws = torch.full((nbytes // 4 + 64,), NAN, device=d)
    assert lib.ruart_gemm_x3_tn_grouped(arr, len(probs), _addr(ws), nbytes, hip.stream_ptr()) == 0
    torch.cuda.synchronize()
    second = fill()
    assert lib.ruart_gemm_x3_tn_grouped(arr, len(probs), _addr(ws), nbytes, hip.stream_ptr()) == 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(ws[nbytes // 4:]).all())
    worst = [0.0, 0.0]
    for i, (call, (M, N, K, cls, acc)) in enumerate(zip(calls, probs)):
        tag = "grouped problem %d (%d, %d, %d) class %d accumulate %d" % (i, M, N, K, cls, acc)
        host = first[i].cpu()
        assert bool(torch.isnan(host[M:]).all()) and bool(torch.isnan(host[:M, N:]).all()), tag + ": a pad element was written"
        got = host[:M, :N]
        assert bool(torch.isfinite(got).all()), tag
        assert torch.equal(_bits(got), _bits(second[i].cpu()[:M, :N])), tag + ": two calls differ"
        alone = call.view(call.run(), tag)
        assert call.rc == 0 and torch.equal(_bits(got), _bits(alone)), tag + ": not the bits of ruart_gemm_x3 alone"
        sk = X.make_plan(M, N, K, 1, 1)[2]
        ra, rb = X.worst(got.double(), *X.x3_bound(call.c, 3, sk, "a")), X.worst(got.double(), *X.x3_bound(call.c, 3, sk, "b"))
        assert ra <= 1.0 and rb <= 1.0, (tag, ra, rb)
        worst = [max(worst[0], ra), max(worst[1], rb)]
    print("x3 grouped, %d problems: worst error / bound %.4f (a) %.4f (b)" % (len(probs), worst[0], worst[1]))


@pytest.mark.parametrize("s", [X.spec(130, 70, 97, "nt", wa=1, wb=1), X.spec(65, 40, 520, "tn", wa=1, wb=4)], ids=X.spec_id)
def test_properties_scaling_is_exact(s):
    """A 2^-40 and B 2^20 give the unscaled result times 2^-20, bit for bit: the halves keep fp32's exponent range, tiny gradients need no
    scaling"""
    c = X.case_of(s)
    base = _Call(s)
    scaled = _Call(s, A=c.A * 2.0 ** -40, B=c.B * 2.0 ** 20)
    r0, r1 = base.view(base.run(), "base"), scaled.view(scaled.run(), "scaled")
    assert base.rc == 0 and scaled.rc == 0
    assert float(r0.abs().min()) > 2.0 ** -100                       # (far from the denormals even after the scaling)
    assert torch.equal(_bits(r0 * 2.0 ** -20), _bits(r1))
    print("x3 scaling %s: bit-equal" % X.spec_id(s))


@pytest.mark.parametrize("lay", ["nt", "tn"])
def test_properties_non_finite_inputs_stay_in_their_row_and_column(lay):
    """+inf in the last real row of A: the clamped loads copy that row into the tile's padding rows, which nothing stores - only output
    row M - 1 may be non-finite, every other element keeps its bits; likewise the last real column of B"""
    s = X.spec(131, 71, 97, lay, wa=1, wb=1)
    c = X.case_of(s)
    base = _Call(s)
    r0 = base.view(base.run(), "base")
    A, B = c.A.clone(), c.B.clone()
    A[s.M - 1, 5] = float("inf")
    B[7, s.N - 1] = float("inf")
    ca, cb = _Call(s, A=A), _Call(s, B=B)
    ra, rb = ca.view(ca.run(), "inf in A", finite=False), cb.view(cb.run(), "inf in B", finite=False)
    assert ca.rc == 0 and cb.rc == 0
    assert torch.equal(_bits(ra[:s.M - 1]), _bits(r0[:s.M - 1])) and not bool(torch.isfinite(ra[s.M - 1]).any())
    assert torch.equal(_bits(rb[:, :s.N - 1]), _bits(r0[:, :s.N - 1])) and not bool(torch.isfinite(rb[:, s.N - 1]).any())


def test_refusals():
    """every refusal of gemm_xn (through ruart_gemm_x3 and ruart_gemm_x1), of ruart_gemm_x3_plan and of ruart_gemm_x3_tn_grouped returns
    hipErrorInvalidValue before anything is launched: C stays NaN"""
    lib, d = hip.load(), dev()
    s = X.spec(64, 48, 40, "nn", bias=True, res=True)
    call = _Call(s)
    keep = torch.ones(1 << 23, dtype=torch.uint8, device=d)          # (large enough for the masks of the 2^20 cases below)
    big = torch.zeros(1 << 20, device=d)
    k = _addr(keep)
    pa, pb = X.pitches(s)
    bad = [dict(A=None), dict(B=None), dict(C=None), dict(M=0), dict(M=-64), dict(N=0), dict(N=-1), dict(K=0), dict(K=-40), dict(ldc=s.N - 1),
           dict(ldr=s.N - 1), dict(act=hip.ACT_RELU), dict(act=3), dict(a_keep=k, b_keep=k),
           dict(a_keep=k, sam=1, sak=pa), dict(b_keep=k, sbk=1, sbn=pb),                    # a_keep needs sak == 1, b_keep sbn == 1
           dict(b_keep=k, sbk=1, sbn=1),                                                    # ... and a B that is not K-contiguous (what ops.mm multiplies first for)
           dict(sam=pa, sak=2), dict(sbk=pb, sbn=2), dict(sam=-pa), dict(sbk=-pb), dict(sak=-1), dict(sbn=-1),
           dict(sam=(1 << 30) // (s.M - 1) + 1), dict(sbk=(1 << 30) // (s.K - 1) + 1)]      # a span >= 2^30 (refused before any launch)
    for entry in ("x3", "x1"):
        C = call.run(entry)
        assert call.rc == 0
        call.view(C, "valid")
        for over in bad:
            C = call.run(entry, **over)
            assert call.rc == INVALID, (entry, over)
            assert bool(torch.isnan(C).all()) and bool(torch.isnan(call.ws).all()), (entry, over)
        # a fused mask whose operand has 2^20 rows or a K of 2^20: the mask-row index is exact below that only.  Every pointer is good
        # for the sizes given (zero pitches fold the long extents onto one row), so nothing here depends on the refusal for its safety
        M20 = 1 << 20
        out = torch.full((M20,), NAN, device=d)
        st = hip.stream_ptr()
        fn = lib.ruart_gemm_x3 if entry == "x3" else lib.ruart_gemm_x1
        args = lambda M, N, K, sam, sbk, ak, bk, rpm: (_addr(big), sam, 1, _addr(big), sbk, 1, None, None, 0, hip.ACT_NONE, _addr(out), N, M, N, K, None, 0,          # noqa: E731
                                                       ak, bk, 1.0, None, rpm, st)
        assert fn(*args(M20, 1, 8, 0, 1, k, None, 1)) == INVALID                       # a_keep, M = 2^20
        assert fn(*args(4, 4, M20, 0, 0, k, None, 1)) == INVALID                       # a_keep, K = 2^20
        assert fn(*args(4, 4, M20, 0, 0, None, k, 1)) == INVALID                       # b_keep, K = 2^20
        assert fn(*args(1, M20, 8, 8, 0, None, k, 1)) == INVALID                       # b_keep, N = 2^20
        assert fn(*args(4, 4, M20 - 32, 0, 0, k, None, 4)) == 0                        # ... and just below it the product runs
        torch.cuda.synchronize()
        assert bool(torch.isnan(out[16:]).all()) and bool(torch.isfinite(out[:16]).all())
    sk, nb = ctypes.c_int(0), ctypes.c_size_t(0)
    for M, N, K in ((0, 4, 4), (4, 0, 4), (4, 4, 0), (-1, 4, 4)):
        assert lib.ruart_gemm_x3_plan(M, N, K, 1, 1, ctypes.byref(sk), ctypes.byref(nb)) == INVALID
    # the grouped launch: n <= 0, NULL probs, a workspace one byte short, lda < M
    gs = X.spec(64, 40, 520, "tn")
    g = _Call(gs)
    arr = (hip.X3TnProblemC * 1)()
    C = torch.full((gs.M + 2, g.ldc), NAN, device=d)
    q = arr[0]
    q.A, q.B, q.C = _addr(g.A, gs.aoff).value, _addr(g.B, gs.boff).value, C.data_ptr()
    q.lda, q.ldb, q.ldc, q.M, q.N, q.K, q.accumulate = g.sa[1], g.sb[0], g.ldc, gs.M, gs.N, gs.K, 0
    nbytes = int(lib.ruart_gemm_x3_tn_grouped_ws(arr, 1))
    assert nbytes == g.nbytes > 0
    st = hip.stream_ptr()
    assert lib.ruart_gemm_x3_tn_grouped(arr, 0, _addr(g.ws), nbytes, st) == INVALID
    assert lib.ruart_gemm_x3_tn_grouped(arr, -1, _addr(g.ws), nbytes, st) == INVALID
    assert lib.ruart_gemm_x3_tn_grouped(None, 1, _addr(g.ws), nbytes, st) == INVALID
    assert lib.ruart_gemm_x3_tn_grouped(arr, 1, _addr(g.ws), nbytes - 1, st) == INVALID
    q.lda = gs.M - 1
    assert lib.ruart_gemm_x3_tn_grouped(arr, 1, _addr(g.ws), nbytes, st) == INVALID
    torch.cuda.synchronize()
    assert bool(torch.isnan(C).all()) and bool(torch.isnan(g.ws).all())
    q.lda = g.sa[1]
    assert lib.ruart_gemm_x3_tn_grouped(arr, 1, _addr(g.ws), nbytes, st) == 0
    torch.cuda.synchronize()
    assert bool(torch.isfinite(C[:gs.M, :gs.N]).all())


@pytest.mark.parametrize("B,T,K,N", [(1, 1, 1, 1), (1, 1, 4, 1), (2, 1, 1, 3)])
def test_linear_with_a_byte_mask_at_degenerate_shapes(B, T, K, N):
    """ops.linear(x, w, b, mask=) with the byte form of the mask at sizes of 1: a single column (or K = 1) makes an operand's two
    strides both 1, and the dW product then reaches the C entry as (b_keep, B K-contiguous), a layout the fused forms do not take - ops.mm
    multiplies first there.  Values and all three gradients against multiply-first in float64, at 4e-5 sum |x m| |w| (twice the peak of
    the format bound, 2.0e-5 sum |a| |b|, over at most 4 products)."""
    from ruart_amd import ops
    mode = ops.trunk_mode()
    assert mode.fuse_masks and mode.gemm == "x3" and not mode.defer_dw
    g = torch.Generator().manual_seed(100 * B + 10 * K + N)
    x = torch.randn(B, T, K, generator=g).cuda().requires_grad_(True)
    w = torch.randn(N, K, generator=g).cuda().requires_grad_(True)
    b = torch.randn(N, generator=g).cuda().requires_grad_(True)
    mask = torch.full((B, K), 1.0 / 0.7)
    mask[B - 1, K - 1] = 0.0 if B * K > 1 else 1.0 / 0.7
    mask = mask.cuda()
    mask.keep, mask.keep_scale = (mask != 0).view(torch.uint8), 1.0 / 0.7
    gy = torch.randn(B, T, N, generator=g).cuda()
    y = ops.linear(x, w, b, mask=mask)
    y.backward(gy)
    torch.cuda.synchronize()
    x64, w64, b64 = (t.detach().double().cpu().requires_grad_(True) for t in (x, w, b))
    m64 = mask.double().cpu()
    y64 = torch.nn.functional.linear(x64 * m64.unsqueeze(1), w64, b64)
    y64.backward(gy.double().cpu())
    xm, gy64 = (x64 * m64.unsqueeze(1)).detach().abs().view(-1, K), gy.double().cpu().abs().view(-1, N)
    bounds = (xm @ w64.detach().abs().t() + b64.detach().abs(), (gy64 @ w64.detach().abs()) * m64.unsqueeze(1).expand(B, T, K).reshape(-1, K),
              gy64.t() @ xm, gy64.sum(0))
    for name, got, ref, bd in zip(("y", "gx", "gw", "gb"), (y.detach(), x.grad, w.grad, b.grad), (y64.detach(), x64.grad, w64.grad, b64.grad), bounds):
        err = (got.double().cpu().reshape(ref.shape) - ref).abs()
        assert bool((err <= 4e-5 * bd.reshape(ref.shape) + 1e-30).all()), (name, float(err.max()))


def _linear_case():
    g = torch.Generator().manual_seed(2 * 48 * 64 + 32)
    x, w, b, gy = (torch.randn(s, generator=g).cuda() for s in ((2, 48, 64), (32, 64), (32,), (2, 48, 32)))
    return x.requires_grad_(True), torch.nn.Parameter(w), b.requires_grad_(True), gy


def test_linear_backward_keeps_the_product_form_of_its_forward():
    """ops.linear under ``use_trunk_mode(grad_gemm='x1')``, its backward after the scope has ended (where the mode in effect says x3):
    dX and dW are bit for bit the one-product forms, which differ from the three-product forms of the same operands."""
    from ruart_amd import ops
    x, w, b, gy = _linear_case()
    with ops.use_trunk_mode(grad_gemm="x1"):
        y = ops.linear(x, w, b)
    assert ops.trunk_mode().backward_gemm == "x3"
    y.backward(gy)
    torch.cuda.synchronize()
    gy2, x2, wd = gy.view(-1, 32), x.detach().view(-1, 64), w.detach()
    want = {m: (ops.mm(gy2, wd, mode=m), ops.mm(gy2.t(), x2, mode=m)) for m in ("x1", "x3")}
    assert not torch.equal(want["x1"][0], want["x3"][0]) and not torch.equal(want["x1"][1], want["x3"][1])
    assert torch.equal(x.grad.view(-1, 64), want["x1"][0])
    assert torch.equal(w.grad, want["x1"][1])


def test_linear_backward_keeps_the_deferral_of_its_forward():
    """``defer_dw`` is the forward's too: on around the forward only, the backward hands dW to the end-of-backward group (once) and the
    gradient has the bits of the undeferred one; on around the backward only, nothing is deferred."""
    from ruart_amd import ops
    entered = []
    real = ops._defer_weight_grad
    ops._defer_weight_grad = lambda *a: (entered.append(1), real(*a))[1]
    try:
        x, w, b, gy = _linear_case()
        ops.linear(x, w, b).backward(gy)                                   # the default: per site
        assert not entered
        x2, w2, b2, _ = _linear_case()
        with ops.use_trunk_mode(defer_dw=True):
            y = ops.linear(x2, w2, b2)
        y.backward(gy)
        torch.cuda.synchronize()
        assert len(entered) == 1 and not ops._deferred
        assert torch.equal(w2.grad, w.grad) and torch.equal(x2.grad, x.grad) and torch.equal(b2.grad, b.grad)
        x3, w3, b3, _ = _linear_case()
        y = ops.linear(x3, w3, b3)
        with ops.use_trunk_mode(defer_dw=True):
            y.backward(gy)
        torch.cuda.synchronize()
        assert len(entered) == 1 and torch.equal(w3.grad, w.grad)
    finally:
        ops._defer_weight_grad = real
