"""CPU proof of the cases, the bounds and the emulation that tests/test_gpu_trunk_attention_wide.py holds the 385 .. 1024-key attention
kernels to (tests/_trunk_attention_wide_ref.py): the gradient formulas equal float64 autograd at these sizes, a faithful fp32 emulation of
the key-block arithmetic stays inside every bound of tests/_trunk_attention_ref.py on every case - the chosen inputs are fair: the
reference arithmetic alone passes, no case left out -, the same emulation with one block-wise defect leaves a bound wherever the defect
can show, and the soft cases really are soft.  No kernel runs here."""
import pytest
import torch

from tests import _trunk_attention_ref as R
from tests import _trunk_attention_wide_ref as W

CASES = W.cases()


def _fmt(res):
    return ", ".join("%s %.3g" % kv for kv in res.items())


@pytest.mark.parametrize("name", W.AUTOGRAD_CASES)
def test_formula_backward_equals_float64_autograd(name):
    c = W.case(name)
    pa, pk, v = (t.double().requires_grad_(True) for t in (c.pa, c.pk, c.v))
    diag = None if c.diag is None else c.diag.double().requires_grad_(True)
    _, _, _, P, out = R.reference_forward(pa, pk, v, c.mask, diag, c.relu, c.ps)
    assert torch.equal(out.detach(), c.out) and torch.equal(P.detach(), c.P)
    (out * c.gout.double()).sum().backward()
    r = c.bwd
    for got, want in ((r["grad_pa"], pa.grad), (r["grad_pk"], pk.grad), (r["grad_v"], v.grad)):
        assert float((got - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max()))
    apa = torch.relu(c.pa.double()) if c.relu else c.pa.double()
    got = r["grad_diag_partial"].sum((0, 1)) if c.diag_len > 1 else (r["R"] * apa).sum().view(1)
    assert float((got - diag.grad).abs().max()) <= 1e-12 * max(1.0, float(diag.grad.abs().max()))
    dead = ~c.live
    assert bool(dead.any())
    for t in (c.P.transpose(1, 2), r["grad_pk"], r["grad_v"]):       # masked keys: probability and gradients exactly 0
        assert float(t[dead].abs().max()) == 0.0


@pytest.mark.parametrize("name", CASES)
def test_faithful_emulation_stays_inside_every_bound(name):
    c = W.case(name)
    probs, out = W.emulate_forward(c)
    res = R.worst_ratios(c, probs=probs, out=out, grads=W.emulate_backward(c, c.P.float()))
    print("emulation %s: worst error / bound: %s" % (name, _fmt(res)))
    assert max(res.values()) <= 1.0
    chained = R.worst_ratios(c, grads=W.emulate_backward(c, probs), chained=True)
    print("emulation %s, own forward probabilities: %s" % (name, _fmt(chained)))
    assert max(chained.values()) <= 1.0
    dead = ~c.live
    if dead.any():
        assert float(probs.transpose(1, 2)[dead].abs().max()) == 0.0


@pytest.mark.parametrize("control", W.control_cases(), ids=lambda c: "%s-%s" % (c[1], c[0]))
def test_negative_controls_break_a_bound(control):
    """every (case, defect) pair where the defect can show (W.defect_shows); a forward defect has to break ``probs`` or ``out``, the
    backward one a gradient computed from the float64 probabilities"""
    name, defect = control
    c = W.case(name)
    if defect in W.FORWARD_DEFECTS:
        probs, out = W.emulate_forward(c, defect)
        res = R.worst_ratios(c, probs=probs, out=out)
    else:
        res = R.worst_ratios(c, grads=W.emulate_backward(c, c.P.float(), defect))
    print("control %s on %s: worst error / bound: %s" % (defect, name, _fmt(res)))
    assert max(res.values()) > 1.0


def test_every_defect_has_controls():
    cc = W.control_cases()
    for d in W.DEFECTS:
        assert sum(1 for _, dd in cc if dd == d) >= 2, d
    assert not W.defect_shows("k1024_full", "block_unmasked") and W.defect_shows("k1023_vec", "block_unmasked")
    assert W.defect_shows("k513_onelast", "norm_drop_last_block") and not W.defect_shows("k767_peaked", "v_block_stale")


@pytest.mark.parametrize("name", [n for n in CASES if W.case(n).regime == "soft"])
def test_soft_cases_are_not_saturated(name):
    """per sample, the median effective key count 1 / sum p^2 is at least 4, or at least n_live / 2 where fewer than 8 keys are live"""
    c = W.case(name)
    neff, nlive = R.effective_keys(c)
    print("soft %s: median effective keys %s of %s live" % (name, [round(float(x), 2) for x in neff], nlive.tolist()))
    for e, n in zip(neff.tolist(), nlive.tolist()):
        assert e >= (4.0 if n >= 8 else n / 2.0) - 1e-9


def test_case_list_covers_what_the_issue_lists():
    shp = [W._CASES[n] for n in CASES]
    assert 14 <= len(shp) <= 18
    assert W.source_key_block() == (W.KB, W.MIN_L2, W.MAX_L2) and R.MAX_L2 + 1 == W.MIN_L2
    edges = set(range(2 * W.KB, W.MAX_L2, W.KB))                                 # the key-block edges inside 385 .. 1024
    assert edges == {512, 768}
    assert {s[2] for s in shp} >= {385, 400, 512, 513, 767, 1023, 1024} | edges | {e + 1 for e in edges}
    assert all(W.MIN_L2 <= s[2] <= W.MAX_L2 for s in shp)
    assert {s[1] for s in shp} >= {1, 15, 16, 17, 33}
    assert {s[3] for s in shp} >= {1, 3, 63, 64, 65, 250}
    assert {s[4] for s in shp} >= {1, 5, 63, 64, 65, 250}
    assert {s[0] for s in shp} == {1, 3}
    assert {(s[5], s[6]) for s in shp} == {(r, d) for r in (0, 1) for d in ("none", "one", "vec")}
    assert {s[8] for s in shp} == set(W.REGIMES) and {s[9] for s in shp} == {"full", "holes", "first", "onelast", "ragged"}
    assert all(s[2] >= 513 for s in shp if s[8] == "offset")
    assert sum(1 for s in shp if s[7]) >= 3
    for n in CASES:
        B, L1, L2, h, D3, relu, dk, ps, _, _, form = W._CASES[n]
        assert W.dispatch_form(L1, relu, {"none": 0, "one": 1, "vec": h}[dk], ps) == form, n
    # L1 == 1 three ways: the single-query form, and the general form through relu and through prob_scale
    assert sum(1 for s in shp if s[10] == "attn1w") >= 2
    assert any(s[1] == 1 and s[10] == "wide" and s[5] for s in shp) and any(s[1] == 1 and s[10] == "wide" and s[7] for s in shp)
    assert all(W.case(W.CHAINED[r]).regime == r for r in W.REGIMES)
    for n in CASES:
        c = W.case(n)
        assert bool(c.live.any(-1).all())
        if c.ps is not None:                                                       # a row whose kept set is empty
            assert float(c.ps[c.B - 1, c.L1 - 1].abs().max()) == 0.0
        if c.mask_kind == "onelast":                                               # every key block before the last is dead
            assert c.live[c.B // 2].nonzero().view(-1).tolist() == [c.L2 - 1] and c.L2 - 1 >= 2 * W.KB
        if c.mask_kind == "ragged" and c.B == 3:                                   # every key block behind the first is dead
            assert c.live[1].nonzero().view(-1).tolist() == [0]
        if c.mask_kind == "first":
            assert not bool(c.live[:, 0].any())
    off = W.case("k513_offset")
    m = off.S.amax(-1).view(-1)
    assert float(m[0]) > 70 and float(m[1]) < -90            # without the max subtraction expf would overflow / underflow
