"""The trained encoder's attention kernels (csrc/bert_train_attn.hip), called through the C ABI and held element by element to the
float64 reference of the same operation at the bounds derived in tests/_train_attention_ref.py (proven on the CPU, negative controls
included, by tests/test_train_attention_ref.py).  Every element of every output is checked, none exempt: context rows and lse2, the
[dQ | dK | dV] rows and the bias parts of all four entry points; exact zeros where the bound is 0; pad columns, rows no window or
chunk owns, guard rows behind every buffer and the lse2 / delta rows of window tokens come back bit-equal (inputs hold NaN there); a
second launch repeats the bits; bias_part == NULL writes the same rows; every refusal leaves its outputs untouched.  The long
backward runs on the float64 lse2 rounded to fp32 (controlled) and on ruart_attn_train_fwd_long's own output (chained).

Every one of the five kernels is reached by at least one case of every defect that can show in it (R.DEFECT_KERNELS;
test_every_defect_reaches_every_kernel_it_lives_in shows it on the CPU): attn_train_fwd and attn_train_bwd by the win_* cases and the
windows beside every long case, attn_train_fwd_long, attn_train_bwd_long_dq and attn_train_bwd_long_dkv by the long_* cases - ragged
tails under soft and offset scores (an unmasked tail), rising maxima (a skipped alpha), peaked rows (delta from the context row), chunk
scales 2^0 / 2^-6 / 2^-12 (the first tile's scale), blocks below f16's normal range (an unscaled dO), a window of one token (bias sums
taken after rounding).  Every test prints its worst error / bound before it asserts (profiles/train_attention_tests.txt)."""
import functools

import numpy as np
import pytest
import torch

from ruart_amd import hip
from tests import _dropout_probe as PB
from tests import _train_attention_ref as R

pytestmark = pytest.mark.gpu

INVALID = 1                      # hipErrorInvalidValue
SEED = 0x2F6E2B1
GUARD_ROWS = 64                  # rows behind every output that no kernel may touch: one tile of query rows past the last token
DEV = "cuda:0"


def _fmt(res):
    return ", ".join("%s %.3g" % kv for kv in res.items())


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


class _Out:
    """an output of ``rows`` x ``pitch`` elements and GUARD_ROWS rows behind it, prefilled with NaN; take() returns the owned part and
    asserts that everything else kept its bits"""

    def __init__(self, rows, pitch, dtype):
        self.rows = rows
        self.buf = torch.full((rows + GUARD_ROWS, pitch), float("nan"), dtype=dtype, device=DEV)
        self.before = _bits(self.buf).cpu().clone()

    def take(self, owned_rows, width, what):
        after = self.buf.cpu()
        own = torch.zeros(after.shape, dtype=torch.bool)
        own[:self.rows][owned_rows, :width] = True
        assert torch.equal(_bits(after)[~own], self.before[~own]), "%s: an element outside the rows and columns the launch owns was written" % what
        return after[:self.rows, :width]

    def untouched(self):
        return torch.equal(_bits(self.buf.cpu()), self.before)


def _input(t, pitch, owned_rows):
    """(T, W) CPU tensor -> device (T, pitch): NaN in the pad columns and in every row the launch does not own"""
    buf = torch.full((t.shape[0], pitch), float("nan"), dtype=t.dtype)
    buf[owned_rows, :t.shape[1]] = t[owned_rows]
    return buf.to(DEV)


def _i32(a):
    return torch.from_numpy(np.ascontiguousarray(a).astype(np.int32)).to(DEV)


class _Dev:
    """device copies of one case: inputs per kernel family (the other family's rows hold NaN), descriptors"""

    def __init__(self, c):
        self.win = [_i32(c.win[0]), _i32(c.win[1])]
        self.ch = [_i32(c.ch[i]) for i in range(5)]
        self.tok_lo = _i32(c.tok_lo)
        self.qkv = {"win": _input(c.qkv16, c.ld, c.win_rows), "long": _input(c.qkv16, c.ld, c.long_rows)}
        self.dO = {"win": _input(c.dO16, c.ldc, c.win_rows), "long": _input(c.dO16, c.ldc, c.long_rows)}


@functools.lru_cache(maxsize=None)
def _case(name):
    """(case, device copies); a dropout case's multipliers are recovered from the forward kernels first (tests/_dropout_probe.py) and
    the float64 reference is rebuilt with them"""
    c = R.case(name)
    d = _Dev(c)
    if c.p > 0:
        masks, dev = PB.attn_masks(hip.load(), c.heads, c.cu, d.win, d.ch if c.ch.shape[1] else None, d.tok_lo, c.p, SEED)
        print("train attention %s: recovered multipliers within %.2e of 1 / (n (1 - p))" % (name, dev))
        c = R.with_masks(c, masks)
    return c, d


def _sync(rc):
    torch.cuda.synchronize()
    assert rc == 0


def _win_fwd(c, d):
    ctx = _Out(c.T, c.ldc, torch.float16)
    _sync(hip.load().ruart_attn_train_fwd(hip.ptr(d.qkv["win"]), c.ld, hip.ptr(ctx.buf), c.ldc, c.H, c.heads, c.win.shape[1], hip.ptr(d.win[0]),
                                          hip.ptr(d.win[1]), hip.ptr(d.tok_lo), c.p, SEED, hip.stream_ptr()))
    return ctx.take(c.win_rows, c.H, "window forward ctx")


def _win_bwd(c, d, with_bias=True):
    dqkv = _Out(c.T, c.ldd, torch.bfloat16)
    bias = _Out(c.win.shape[1], 2 * c.H, torch.float32)
    _sync(hip.load().ruart_attn_train_bwd(hip.ptr(d.qkv["win"]), c.ld, hip.ptr(d.dO["win"]), c.ldc, hip.ptr(dqkv.buf), c.ldd, c.H, c.heads,
                                          c.win.shape[1], hip.ptr(d.win[0]), hip.ptr(d.win[1]), hip.ptr(d.tok_lo), c.p, SEED,
                                          hip.ptr(bias.buf) if with_bias else None, hip.stream_ptr()))
    if not with_bias:
        assert bias.untouched()
    return (dqkv.take(c.win_rows, 3 * c.H, "window backward dqkv"),
            bias.take(torch.ones(c.win.shape[1], dtype=torch.bool), 2 * c.H, "window backward bias") if with_bias else None)


def _long_fwd(c, d):
    ctx = _Out(c.T, c.ldc, torch.float16)
    lse = _Out(c.T, c.heads, torch.float32)
    _sync(hip.load().ruart_attn_train_fwd_long(hip.ptr(d.qkv["long"]), c.ld, hip.ptr(ctx.buf), c.ldc, c.H, c.heads, c.ch.shape[1], hip.ptr(d.ch[0]),
                                               hip.ptr(d.ch[1]), hip.ptr(d.ch[2]), hip.ptr(d.ch[3]), c.p, SEED, hip.ptr(lse.buf), hip.stream_ptr()))
    return ctx.take(c.long_rows, c.H, "long forward ctx"), lse.take(c.long_rows, c.heads, "long forward lse2")


def _long_bwd(c, d, lse2, with_bias=True):
    """lse2: (T, heads) fp32 CPU tensor, NaN on the window tokens' rows"""
    nc = c.ch.shape[1]
    dqkv = _Out(c.T, c.ldd, torch.bfloat16)
    bias = _Out(nc, 2 * c.H, torch.float32)
    delta, scale = _Out(c.T, c.heads, torch.float32), _Out(nc, c.heads, torch.float32)
    lse_d = lse2.to(DEV)
    _sync(hip.load().ruart_attn_train_bwd_long(hip.ptr(d.qkv["long"]), c.ld, hip.ptr(d.dO["long"]), c.ldc, hip.ptr(dqkv.buf), c.ldd, c.H, c.heads, nc,
                                               hip.ptr(d.ch[0]), hip.ptr(d.ch[1]), hip.ptr(d.ch[2]), hip.ptr(d.ch[3]), hip.ptr(d.ch[4]), c.p, SEED,
                                               hip.ptr(lse_d), hip.ptr(delta.buf), hip.ptr(scale.buf), hip.ptr(bias.buf) if with_bias else None,
                                               hip.stream_ptr()))
    every = torch.ones(nc, dtype=torch.bool)
    delta.take(c.long_rows, c.heads, "long backward delta workspace")
    got_scale = scale.take(every, c.heads, "long backward scale workspace")
    assert torch.equal(got_scale.double(), c.ch_scale), "a chunk's dO scale is not the power of two that brings its largest entry to [0.5, 1)"
    if not with_bias:
        assert bias.untouched()
    return dqkv.take(c.long_rows, 3 * c.H, "long backward dqkv"), bias.take(every, 2 * c.H, "long backward bias") if with_bias else None


def _exact_zeros(c, got, rows, chained=False):
    z = (R.backward_bounds(c, chained)["dqkv"] == 0) & rows[:, None]
    assert not z.any() or float(got[z].float().abs().max()) == 0.0, "a result whose bound is 0 is not 0"
    return int(z.sum())


@pytest.mark.parametrize("name", R.window_cases())
def test_window_forward_against_float64(name):
    c, d = _case(name)
    ctx = _win_fwd(c, d)
    res = R.kernel_ratios(c, win_fwd=ctx)
    print("train attention window forward %s: worst error / bound: %s" % (name, _fmt(res)))
    assert max(res.values()) <= 1.0
    assert torch.equal(_bits(_win_fwd(c, d)), _bits(ctx))                      # fixed order, no atomics: the bits repeat


@pytest.mark.parametrize("name", R.window_cases())
def test_window_backward_against_float64(name):
    c, d = _case(name)
    dqkv, bias = _win_bwd(c, d)
    res = R.kernel_ratios(c, win_bwd=(dqkv, bias))
    nz = _exact_zeros(c, dqkv, c.win_rows)
    print("train attention window backward %s: worst error / bound: %s; %d elements exactly 0" % (name, _fmt(res), nz))
    for s, q in R.quiet_sequence_precision(c).items():
        a, b = int(c.cu[s[0]]), int(c.cu[s[0] + 1])
        sl = slice({"dQ": 0, "dK": 1, "dV": 2}[s[1]] * c.H, ({"dQ": 0, "dK": 1, "dV": 2}[s[1]] + 1) * c.H)
        err = (dqkv[a:b, sl].double() - c.dqkv[a:b, sl]).abs()
        print("quiet sequence %s: %d of %d tokens, %s: bound max / max |ref| %.3g; measured max error / max |ref| %.3g, rel-L2 %.3g"
              % (name, s[0], c.lens[s[0]], s[1], q[0], float(err.max() / c.dqkv[a:b, sl].abs().max()), float(err.norm() / c.dqkv[a:b, sl].norm())))
    assert max(res.values()) <= 1.0
    again = _win_bwd(c, d)
    assert torch.equal(_bits(again[0]), _bits(dqkv)) and torch.equal(_bits(again[1]), _bits(bias))
    assert torch.equal(_bits(_win_bwd(c, d, with_bias=False)[0]), _bits(dqkv))  # bias_part == NULL: the same rows


@pytest.mark.parametrize("name", R.long_cases())
def test_long_forward_against_float64(name):
    c, d = _case(name)
    ctx, lse = _long_fwd(c, d)
    res = R.kernel_ratios(c, long_fwd=(ctx, lse))
    print("train attention long forward %s: worst error / bound: %s" % (name, _fmt(res)))
    assert max(res.values()) <= 1.0
    again = _long_fwd(c, d)
    assert torch.equal(_bits(again[0]), _bits(ctx)) and torch.equal(_bits(again[1]), _bits(lse))


@pytest.mark.parametrize("mode", ["controlled", "chained"])
@pytest.mark.parametrize("name", R.long_cases())
def test_long_backward_against_float64(name, mode):
    c, d = _case(name)
    chained = mode == "chained"
    lse = _long_fwd(c, d)[1] if chained else c.lse2.float()
    dqkv, bias = _long_bwd(c, d, lse)
    res = R.kernel_ratios(c, long_bwd=(dqkv, bias), chained=chained)
    nz = _exact_zeros(c, dqkv, c.long_rows, chained)
    print("train attention long backward %s (%s lse2): worst error / bound: %s; %d elements exactly 0" % (name, mode, _fmt(res), nz))
    assert max(res.values()) <= 1.0
    again = _long_bwd(c, d, lse)
    assert torch.equal(_bits(again[0]), _bits(dqkv)) and torch.equal(_bits(again[1]), _bits(bias))
    if not chained:
        assert torch.equal(_bits(_long_bwd(c, d, lse, with_bias=False)[0]), _bits(dqkv))


def test_a_64_token_sequence_through_both_kernel_families():
    """one 64-token sequence as a window of its own and as ONE chunk of the *_long kernels: the same float64 values, each result
    inside the bound of the kernel that made it"""
    base, dbase = _case(R.BOTH_PATHS_CASE)
    s = [i for i, n in enumerate(base.lens) if n == 64][0]
    a, b = int(base.cu[s]), int(base.cu[s + 1])
    c = R.as_long(base, s)
    assert torch.equal(c.ctx, base.ctx) and torch.equal(c.dqkv, base.dqkv) and bool(c.long_rows[a:b].all()) and bool(base.win_rows[a:b].all())
    d = _Dev(c)
    ctx_l, lse = _long_fwd(c, d)
    dq_l, bias_l = _long_bwd(c, d, lse)
    res_l = R.kernel_ratios(c, long_fwd=(ctx_l, lse), long_bwd=(dq_l, bias_l), chained=True)
    ctx_w = _win_fwd(base, dbase)
    dq_w, bias_w = _win_bwd(base, dbase)
    res_w = R.kernel_ratios(base, win_fwd=ctx_w, win_bwd=(dq_w, bias_w))
    rows = slice(a, b)
    print("train attention, one 64-token sequence: as a chunk %s; as a window %s; the two differ by at most %.3g (ctx) and %.3g of the largest gradient entry"
          % (_fmt(res_l), _fmt(res_w), float((ctx_l[rows].double() - ctx_w[rows].double()).abs().max()),
             float((dq_l[rows].double() - dq_w[rows].double()).abs().max() / base.dqkv[rows].abs().max())))
    assert max(res_l.values()) <= 1.0 and max(res_w.values()) <= 1.0
    fb_l, fb_w = R.forward_bounds(c)["ctx"][rows], R.forward_bounds(base)["ctx"][rows]
    assert bool(((ctx_l[rows].double() - ctx_w[rows].double()).abs() <= fb_l + fb_w).all())
    bb_l, bb_w = R.backward_bounds(c, True)["dqkv"][rows], R.backward_bounds(base)["dqkv"][rows]
    assert bool(((dq_l[rows].double() - dq_w[rows].double()).abs() <= bb_l + bb_w).all())


def test_refusals_leave_the_outputs_untouched():
    """every refused call returns hipErrorInvalidValue before any launch: wrong head count, no blocks, ld & 7, a misaligned ldc / ldd
    of each entry point, p outside [0, 1), a null lse2 / delta_ws / scale_ws"""
    lib = hip.load()
    c, d = _case("long_soft")
    H, nh, nw, nc, st = c.H, c.heads, c.win.shape[1], c.ch.shape[1], hip.stream_ptr()
    ctx, dqkv = _Out(c.T, c.ldc + 8, torch.float16), _Out(c.T, c.ldd + 8, torch.bfloat16)
    lse, delta, scale = _Out(c.T, nh, torch.float32), _Out(c.T, nh, torch.float32), _Out(nc, nh, torch.float32)
    bias = _Out(max(nw, nc), 2 * H, torch.float32)
    lse_in = c.lse2.float().to(DEV)
    P = hip.ptr

    def fwd(heads=nh, n=nw, ld=c.ld, ldc=c.ldc, p=0.0):
        return lib.ruart_attn_train_fwd(P(d.qkv["win"]), ld, P(ctx.buf), ldc, H, heads, n, P(d.win[0]), P(d.win[1]), P(d.tok_lo), p, SEED, st)

    def bwd(heads=nh, n=nw, ld=c.ld, ldc=c.ldc, ldd=c.ldd, p=0.0):
        return lib.ruart_attn_train_bwd(P(d.qkv["win"]), ld, P(d.dO["win"]), ldc, P(dqkv.buf), ldd, H, heads, n, P(d.win[0]), P(d.win[1]),
                                        P(d.tok_lo), p, SEED, P(bias.buf), st)

    def fwd_long(heads=nh, n=nc, ld=c.ld, ldc=c.ldc, p=0.0, lse2=lse.buf):
        return lib.ruart_attn_train_fwd_long(P(d.qkv["long"]), ld, P(ctx.buf), ldc, H, heads, n, P(d.ch[0]), P(d.ch[1]), P(d.ch[2]), P(d.ch[3]), p,
                                             SEED, P(lse2), st)

    def bwd_long(heads=nh, n=nc, ld=c.ld, ldc=c.ldc, ldd=c.ldd, p=0.0, lse2=lse_in, dws=delta.buf, sws=scale.buf):
        return lib.ruart_attn_train_bwd_long(P(d.qkv["long"]), ld, P(d.dO["long"]), ldc, P(dqkv.buf), ldd, H, heads, n, P(d.ch[0]), P(d.ch[1]),
                                             P(d.ch[2]), P(d.ch[3]), P(d.ch[4]), p, SEED, P(lse2), P(dws), P(sws), P(bias.buf), st)

    calls = []
    for f in (fwd, bwd, fwd_long, bwd_long):
        calls += [(f, dict(heads=nh + 1)), (f, dict(n=0)), (f, dict(ld=c.ld + 4)), (f, dict(p=-0.1)), (f, dict(p=1.0))]
    calls += [(fwd, dict(ldc=c.ldc + 2)), (fwd_long, dict(ldc=c.ldc + 2)), (bwd, dict(ldc=c.ldc + 4)), (bwd, dict(ldd=c.ldd + 2)),
              (bwd_long, dict(ldc=c.ldc + 4)), (bwd_long, dict(ldd=c.ldd + 2)), (fwd_long, dict(lse2=None)), (bwd_long, dict(lse2=None)),
              (bwd_long, dict(dws=None)), (bwd_long, dict(sws=None))]
    for f, kw in calls:
        assert f(**kw) == INVALID, (f.__name__, kw)
    torch.cuda.synchronize()
    for o in (ctx, dqkv, lse, delta, scale, bias):
        assert o.untouched()
    print("train attention refusals: %d calls refused with hipErrorInvalidValue, outputs untouched" % len(calls))
