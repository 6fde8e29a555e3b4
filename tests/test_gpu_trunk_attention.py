"""The trunk's fused cross-attention (csrc/sdnet_attention.hip), called by name through the C ABI and held element by element to the float64
reference of the same operation at the bounds derived in tests/_trunk_attention_ref.py (proven on the CPU, negative controls included,
by tests/test_trunk_attention_ref.py).  The case list covers every dispatch form - the prefetch widths 12 / 16 / 28 / 32 on both sides of
each L2p edge, the staged kernels, attn1 - with soft, peaked and offset scores and full, holed, first-key-masked, one-live-key and ragged
masks.  Every test prints its worst error / bound ratio before it asserts (profiles/trunk_attention_tests.txt holds the measured values)."""
import pytest
import torch

from ruart_amd import hip
from tests import _trunk_attention_ref as R

pytestmark = pytest.mark.gpu

INVALID = 1                      # hipErrorInvalidValue
GUARD = 1234.5                   # what the guard region behind every output buffer holds


def dev():
    return torch.device("cuda:0")


def _bits(t):
    return t.contiguous().view(torch.int32)


class _Guarded:
    """an output buffer of ``shape`` prefilled with NaN, with a guard region behind it that no kernel may touch: 16 rows of the widest
    dimension, so that a store for the dead rows (>= L1, or keys >= L2) of the last 16-row tile of the last sample lands in it"""

    def __init__(self, shape, c, d):
        self.n = 1
        for s in shape:
            self.n *= s
        self.flat = torch.full((self.n + 16 * max(c.L2, c.h, c.D3) + 64,), float("nan"), device=d)
        self.flat[self.n:] = GUARD
        self.t = self.flat[:self.n].view(shape)

    def cpu(self, what):
        assert bool((self.flat[self.n:] == GUARD).all()), "%s: the guard region behind the buffer was written" % what
        return self.t.cpu()


def _set_prefetch(on):
    hip.check(hip.load().ruart_attn_set_prefetch(on), "ruart_attn_set_prefetch")


def _inputs(c, d, pk=None, v=None):
    diag = None if c.diag is None else c.diag.to(d)
    ps = None if c.ps is None else c.ps.to(d)
    return c.pa.to(d), (c.pk if pk is None else pk).to(d), (c.v if v is None else v).to(d), c.mask.to(d), diag, ps


def _forward(c, prefetch, pk=None, v=None):
    """one launch of ruart_attn_fwd_pscale on case ``c``: (probs, out) on the CPU; NaN-prefilled, guarded outputs"""
    lib, d = hip.load(), dev()
    pa, pk, v, mask, diag, ps = _inputs(c, d, pk, v)
    out, probs = _Guarded((c.B, c.L1, c.D3), c, d), _Guarded((c.B, c.L1, c.L2), c, d)
    try:
        _set_prefetch(prefetch)
        rc = lib.ruart_attn_fwd_pscale(pa, pk, v, mask, diag, c.diag_len, c.relu, ps, out.t, probs.t, c.B, c.L1, c.L2, c.h, c.D3, hip.stream_ptr())
        torch.cuda.synchronize()
    finally:
        _set_prefetch(1)
    assert rc == 0
    return probs.cpu("probs"), out.cpu("out")


def _backward(c, probs, prefetch, pk=None, v=None):
    """one launch of ruart_attn_bwd_pscale on case ``c`` with the given fp32 probabilities: dict of CPU tensors.  Outputs and the dS
    workspace are prefilled with NaN (attn_bwd_kv must read nothing attn_bwd_q did not write) and guarded."""
    lib, d = hip.load(), dev()
    pa, pk, v, mask, diag, ps = _inputs(c, d, pk, v)
    nt = (c.L1 + 15) // 16
    ga, gk, gv = _Guarded((c.B, c.L1, c.h), c, d), _Guarded((c.B, c.L2, c.h), c, d), _Guarded((c.B, c.L2, c.D3), c, d)
    gd = _Guarded((c.B, nt, c.h), c, d) if c.diag_len > 1 else None
    ds = _Guarded((c.B, c.L1, c.L2), c, d)
    try:
        _set_prefetch(prefetch)
        rc = lib.ruart_attn_bwd_pscale(pa, pk, v, probs.to(d), c.gout.to(d), diag, c.diag_len, c.relu, ps, ga.t, gk.t, gv.t,
                                       gd.t if gd is not None else None, ds.t, c.B, c.L1, c.L2, c.h, c.D3, hip.stream_ptr())
        torch.cuda.synchronize()
    finally:
        _set_prefetch(1)
    assert rc == 0
    res = dict(grad_pa=ga.cpu("grad_pa"), grad_pk=gk.cpu("grad_pk"), grad_v=gv.cpu("grad_v"), dS=ds.cpu("ds_ws"))
    if gd is not None:
        res["grad_diag_partial"] = gd.cpu("grad_diag_partial")
    return res


def _fmt(res):
    return ", ".join("%s %.3g" % kv for kv in res.items())


def _rewritten_masked_rows(c):
    """pk and v with the rows of masked keys replaced by other finite values"""
    dead = ~c.live
    pk, v = c.pk.clone(), c.v.clone()
    pk[dead] = pk[dead] * -3.0 + 2.0
    v[dead] = v[dead] * -3.0 + 100.0
    return pk, v


def _check_form(c):
    """the kernel form this case reaches with prefetch on is the one the case table names (prefetch off: the staged kernels, or attn1).
    R.dispatch_form restates the library's launch code; tests/test_trunk_attention_ref.py compares it with csrc/sdnet_attention.hip."""
    L2p = R.up16(c.L2)
    form = R.dispatch_form(c.L1, c.L2, c.relu, c.diag_len, c.ps is not None)
    assert form == c.form
    if form not in ("attn1", "staged"):
        assert {12: L2p <= 48, 16: 48 < L2p <= 64, 28: 64 < L2p <= 112, 32: 112 < L2p <= 128}[form]
    elif form == "staged":
        assert L2p > 128
    assert R.dispatch_form(c.L1, c.L2, c.relu, c.diag_len, c.ps is not None, prefetch=False) in ("attn1", "staged")


@pytest.mark.parametrize("name", R.cases())
def test_forward_against_float64(name):
    """out and probs inside their element-wise bounds with prefetch on and off (the same bits both ways); a masked key's probability is
    exactly 0 and its pk / v rows reach no result bit; a second launch gives the same bits; NaN prefill fully overwritten, guards intact"""
    c = R.case(name)
    _check_form(c)
    dead = ~c.live
    res = {}
    for on in (1, 0):
        probs, out = _forward(c, on)
        r = R.worst_ratios(c, probs=probs, out=out)
        print("trunk attention forward %s (%s, prefetch %d): worst error / bound: %s" % (name, c.form, on, _fmt(r)))
        assert max(r.values()) <= 1.0
        if dead.any():
            assert float(probs.transpose(1, 2)[dead].abs().max()) == 0.0
        res[on] = (probs, out)
    assert torch.equal(_bits(res[0][0]), _bits(res[1][0])) and torch.equal(_bits(res[0][1]), _bits(res[1][1]))
    again = _forward(c, 1)
    assert torch.equal(_bits(again[0]), _bits(res[1][0])) and torch.equal(_bits(again[1]), _bits(res[1][1]))
    if dead.any():
        pk2, v2 = _rewritten_masked_rows(c)
        other = _forward(c, 1, pk2, v2)
        assert torch.equal(_bits(other[0]), _bits(res[1][0])) and torch.equal(_bits(other[1]), _bits(res[1][1]))


def _check_backward(c, g, tag, chained=False):
    r = R.worst_ratios(c, grads=g, chained=chained)
    r["dS"] = R.ratio(g["dS"], c.bwd["dS"], R.backward_bounds(c, chained)["dS"]) if c.form != "attn1" else 0.0
    print("trunk attention backward %s: worst error / bound: %s" % (tag, _fmt(r)))
    assert max(r.values()) <= 1.0
    dead = ~c.live
    if dead.any():
        assert float(g["grad_pk"][dead].abs().max()) == 0.0 and float(g["grad_v"][dead].abs().max()) == 0.0
    return r


@pytest.mark.parametrize("name", R.cases())
def test_backward_against_float64(name):
    """the backward on inputs the test controls - probs = the float64 P rounded to fp32, so that no forward error can hide or cancel a
    backward one: grad_pa, grad_pk, grad_v, every grad_diag partial and their sum inside their bounds, prefetch on and off (same bits);
    masked keys: gradients exactly 0, their pk / v rows reach no bit of a live row's gradients; a second launch gives the same bits"""
    c = R.case(name)
    _check_form(c)
    probs = c.P.float()
    res = {}
    for on in (1, 0):
        res[on] = _backward(c, probs, on)
        _check_backward(c, res[on], "%s (%s, prefetch %d)" % (name, c.form, on))
    keys = [k for k in res[1] if not (k == "dS" and c.form == "attn1")]
    for k in keys:
        assert torch.equal(_bits(res[0][k]), _bits(res[1][k])), k
    again = _backward(c, probs, 1)
    for k in keys:
        assert torch.equal(_bits(again[k]), _bits(res[1][k])), k
    dead = ~c.live
    if dead.any():
        pk2, v2 = _rewritten_masked_rows(c)
        other = _backward(c, probs, 1, pk2, v2)
        assert float(other["grad_pk"][dead].abs().max()) == 0.0 and float(other["grad_v"][dead].abs().max()) == 0.0
        for k in ("grad_pk", "grad_v"):
            assert torch.equal(_bits(other[k][c.live]), _bits(res[1][k][c.live])), k
        for k in keys:
            if k not in ("grad_pk", "grad_v", "dS"):
                assert torch.equal(_bits(other[k]), _bits(res[1][k])), k


@pytest.mark.parametrize("regime", R.REGIMES)
def test_forward_into_backward_chain(regime):
    """the kernel's own forward probabilities fed to the backward: the same bounds, widened by the forward's P bound as the derivation
    propagates it (R.backward_bounds(chained=True))"""
    c = R.case(R.CHAINED[regime])
    assert c.regime == regime
    probs, out = _forward(c, 1)
    r = R.worst_ratios(c, probs=probs, out=out)
    assert max(r.values()) <= 1.0
    _check_backward(c, _backward(c, probs, 1), "%s chained on the forward's probabilities (%s)" % (c.name, regime), chained=True)


def test_refusals_leave_the_outputs_untouched():
    """L2 = 385, a diag_len outside {0, 1, h} and a non-positive dimension: hipErrorInvalidValue from both entry points, nothing launched"""
    lib, d = hip.load(), dev()
    B, L1, L2, h, D3 = 2, 5, 385, 8, 6
    z = lambda *s: torch.zeros(*s, device=d)           # noqa: E731
    f = lambda *s: torch.full(s, GUARD, device=d)      # noqa: E731
    pa, pk, v, mask, diag = z(B, L1, h), z(B, L2, h), z(B, L2, D3), torch.ones(B, L2, dtype=torch.uint8, device=d), torch.ones(h, device=d)
    probs_in, gout, ps = z(B, L1, L2), z(B, L1, D3), torch.ones(B, L1, L2, device=d)
    outs = [f(B, L1, D3), f(B, L1, L2), f(B, L1, h), f(B, L2, h), f(B, L2, D3), f(B, 1, h), f(B, L1, L2)]
    out, probs, ga, gk, gv, gd, ds = outs
    st = hip.stream_ptr()

    def fwd(B=B, L1=L1, L2=16, h=h, D3=D3, dl=h, ps=None, relu=1):
        return lib.ruart_attn_fwd_pscale(pa, pk, v, mask, diag, dl, relu, ps, out, probs, B, L1, L2, h, D3, st)

    def bwd(B=B, L1=L1, L2=16, h=h, D3=D3, dl=h, ps=None, relu=1):
        return lib.ruart_attn_bwd_pscale(pa, pk, v, probs_in, gout, diag, dl, relu, ps, ga, gk, gv, gd, ds, B, L1, L2, h, D3, st)

    for call in (fwd, bwd):
        assert call(L2=385) == INVALID and call(L2=385, ps=ps) == INVALID
        assert call(dl=2) == INVALID and call(dl=h + 1) == INVALID and call(dl=-1) == INVALID
        for dim in ("B", "L1", "L2", "h", "D3"):
            assert call(**{dim: 0}) == INVALID and call(**{dim: -3}) == INVALID, dim
        assert R.dispatch_form(1, 384, 0, 0, False) == "attn1"
        assert call(L1=1, dl=0, relu=0, L2=385) == INVALID and call(L1=1, dl=0, relu=0, D3=0) == INVALID      # arguments that would take attn1
    assert lib.ruart_attn_fwd(pa, pk, v, mask, diag, h, 1, out, probs, B, L1, 385, h, D3, st) == INVALID
    assert lib.ruart_attn_bwd(pa, pk, v, probs_in, gout, diag, h, 1, ga, gk, gv, gd, ds, B, L1, 385, h, D3, st) == INVALID
    torch.cuda.synchronize()
    for t in outs:
        assert bool((t == GUARD).all())


@pytest.mark.parametrize("path", ["general", "attn1"])
def test_a_sample_without_live_keys_raises_the_nan_flag(path):
    """every key of a sample masked: no softmax exists (the reference asserts on the NaN); the kernel raises the device flag registered
    through ruart_set_nan_flag, the step's one check reports it, and the flag is clear afterwards.  Live samples raise nothing."""
    from ruart_amd import ops
    lib, d = hip.load(), dev()
    B, L1, L2, h, D3 = (2, 5, 20, 8, 6) if path == "general" else (2, 1, 20, 8, 6)
    assert R.dispatch_form(L1, L2, 0, 0, False) == (12 if path == "general" else "attn1")
    g = torch.Generator().manual_seed(11)
    pa, pk, v = (torch.randn(*s, generator=g).to(d) for s in ((B, L1, h), (B, L2, h), (B, L2, D3)))
    out, probs = torch.empty(B, L1, D3, device=d), torch.empty(B, L1, L2, device=d)
    flag = ops.nan_flag.ensure(d)
    ops.nan_flag.check_and_clear()
    mask = torch.ones(B, L2, dtype=torch.uint8)
    assert lib.ruart_attn_fwd(pa, pk, v, mask.to(d), None, 0, 0, out, probs, B, L1, L2, h, D3, hip.stream_ptr()) == 0
    torch.cuda.synchronize()
    assert int(flag.item()) == 0 and bool(torch.isfinite(out).all())
    ops.nan_flag.check_and_clear()
    mask[1] = 0
    assert lib.ruart_attn_fwd(pa, pk, v, mask.to(d), None, 0, 0, out, probs, B, L1, L2, h, D3, hip.stream_ptr()) == 0
    torch.cuda.synchronize()
    assert int(flag.item()) == 1 and bool(torch.isnan(out[1]).all()) and bool(torch.isfinite(out[0]).all())
    with pytest.raises(AssertionError):
        ops.nan_flag.check_and_clear()
    assert int(flag.item()) == 0
    ops.nan_flag.check_and_clear()


def test_autograd_glue_against_float64():
    """ops.fused_attention end to end on a soft case with a vector diag and L1 = 33 (three query tiles per sample): the context, the
    gradients of pk and v, diag.grad = the sum of the nine per-tile partials, and W.grad through pa = x W^T, all at the float64 bounds
    (the kernel's own probabilities go into the backward: the chained bounds; the partial sum and the x^T grad_pa product add their
    own fp32 chains)."""
    from ruart_amd import ops
    d = dev()
    base = R.case(R.GLUE_CASE)
    assert base.regime == "soft" and base.diag_len == base.h and base.L1 == 33
    g = torch.Generator().manual_seed(77)
    x = base.pa.clone()
    W = torch.eye(base.h) + 0.05 * torch.randn(base.h, base.h, generator=g)
    xd = x.to(d)
    Wd, pkd, vd = (t.to(d).requires_grad_(True) for t in (W, base.pk, base.v))
    diagd = base.diag.view(1, 1, -1).to(d).requires_grad_(True)
    pa = xd @ Wd.t()
    y = ops.fused_attention(pa, pkd, vd, base.mask.to(d), diag=diagd, relu=True)
    y.backward(base.gout.to(d))
    torch.cuda.synchronize()
    c = R.case_with_pa(base, pa.detach().cpu())
    neff, nlive = R.effective_keys(c)
    assert int(nlive.min()) >= 8 and float(neff.min()) >= 4.0             # still a soft case with the perturbed projection
    _, b_out = R.forward_bounds(c)
    bb = R.backward_bounds(c, chained=True)
    res = {"out": R.ratio(y.detach().cpu(), c.out, b_out), "grad_pk": R.ratio(pkd.grad.cpu(), c.bwd["grad_pk"], bb["grad_pk"]),
           "grad_v": R.ratio(vd.grad.cpu(), c.bwd["grad_v"], bb["grad_v"])}
    part, bpart = c.bwd["grad_diag_partial"], bb["grad_diag_partial"]
    n_part = part.shape[0] * part.shape[1]
    res["diag.grad"] = R.ratio(diagd.grad.cpu().view(-1), part.sum((0, 1)),
                               bpart.sum((0, 1)) + R.gamma(n_part) * (part.abs() + bpart).sum((0, 1)))
    rows = c.B * c.L1
    gpa, bpa, xa = c.bwd["grad_pa"].view(rows, c.h), bb["grad_pa"].view(rows, c.h), x.double().view(rows, c.h)
    res["W.grad"] = R.ratio(Wd.grad.cpu(), gpa.t() @ xa, bpa.t() @ xa.abs() + R.gamma(rows) * ((gpa.abs() + bpa).t() @ xa.abs()))
    print("trunk attention through ops.fused_attention (%s): worst error / bound: %s" % (c.name, _fmt(res)))
    assert max(res.values()) <= 1.0


def test_scalar_diag_through_ops_frozen_and_trainable():
    """The scalar diag of do_similarity through ops.fused_attention (k129_relu_one: L1 = 33, three query tiles, the staged kernels).  Frozen,
    as the model holds it: the context and the gradients of pa, pk, v at the float64 bounds.  Trainable: the kernels return grad_diag
    partials per column for a vector diag only, so the backward runs with the scalar spread over the h columns - every other gradient
    keeps its bits - and diag.grad = sum over samples, tiles and columns of the partials, R o act(pa) summed, held to the partials' bounds
    plus the fp32 chain of that sum."""
    from ruart_amd import ops
    d = dev()
    c1 = R.case("k129_relu_one")
    assert c1.diag_len == 1 and c1.L1 == 33 and c1.h > 1
    bb1 = R.backward_bounds(c1, chained=True)
    got = {}
    for kind in ("frozen", "trainable"):
        pa1, pk1, v1 = (t.to(d).requires_grad_(True) for t in (c1.pa, c1.pk, c1.v))
        diag1 = c1.diag.view(1, 1, 1).to(d).requires_grad_(kind == "trainable")
        y1 = ops.fused_attention(pa1, pk1, v1, c1.mask.to(d), diag=diag1, relu=True)
        y1.backward(c1.gout.to(d))
        torch.cuda.synchronize()
        res1 = {"out": R.ratio(y1.detach().cpu(), c1.out, R.forward_bounds(c1)[1])}
        for k, t in (("grad_pa", pa1), ("grad_pk", pk1), ("grad_v", v1)):
            res1[k] = R.ratio(t.grad.cpu(), c1.bwd[k], bb1[k])
        if kind == "trainable":
            part, bpart = c1.bwd["grad_diag_partial"], bb1["grad_diag_partial"]
            n_terms = part.shape[0] * part.shape[1] + c1.h              # the partial rows of a column, then the h columns
            assert diag1.grad is not None and diag1.grad.shape == diag1.shape
            res1["diag.grad"] = R.ratio(diag1.grad.cpu().view(1), part.sum().view(1),
                                        (bpart.sum() + R.gamma(n_terms) * (part.abs() + bpart).sum()).view(1))
        print("trunk attention through ops.fused_attention (%s, %s scalar diag): worst error / bound: %s" % (c1.name, kind, _fmt(res1)))
        assert max(res1.values()) <= 1.0
        got[kind] = [y1.detach().cpu(), pa1.grad.cpu(), pk1.grad.cpu(), v1.grad.cpu()]
    for t0, t1 in zip(got["frozen"], got["trainable"]):
        assert torch.equal(_bits(t0), _bits(t1))
