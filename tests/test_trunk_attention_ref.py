"""CPU proof of the reference, the bounds and the case list that tests/test_gpu_trunk_attention.py holds the trunk's attention kernels to
(tests/_trunk_attention_ref.py): the gradient formulas equal float64 autograd, a faithful fp32 emulation of the kernels' arithmetic
stays inside every element-wise bound on every case, the same emulation with one defect leaves a bound wherever the defect can show -
so the GPU tests can fail -, and the soft cases really are soft.  No kernel runs here."""
import pytest
import torch

from tests import _trunk_attention_ref as R

CASES = R.cases()


def _fmt(res):
    return ", ".join("%s %.3g" % kv for kv in res.items())


@pytest.mark.parametrize("name", CASES)
def test_formula_backward_equals_float64_autograd(name):
    c = R.case(name)
    pa, pk, v = (t.double().requires_grad_(True) for t in (c.pa, c.pk, c.v))
    diag = None if c.diag is None else c.diag.double().requires_grad_(True)
    _, _, _, P, out = R.reference_forward(pa, pk, v, c.mask, diag, c.relu, c.ps)
    assert torch.equal(out.detach(), c.out) and torch.equal(P.detach(), c.P)
    (out * c.gout.double()).sum().backward()
    r = c.bwd
    for got, want in ((r["grad_pa"], pa.grad), (r["grad_pk"], pk.grad), (r["grad_v"], v.grad)):
        assert float((got - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max()))
    if diag is not None:
        apa = torch.relu(c.pa.double()) if c.relu else c.pa.double()
        want = diag.grad
        got = r["grad_diag_partial"].sum((0, 1)) if c.diag_len > 1 else (r["R"] * apa).sum().view(1)
        assert float((got - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max()))
    # masked keys: probability and gradients exactly 0 in the reference too
    dead = ~c.live
    if dead.any():
        for t in (c.P.transpose(1, 2), r["grad_pk"], r["grad_v"]):
            assert float(t[dead].abs().max()) == 0.0


@pytest.mark.parametrize("name", CASES)
def test_faithful_emulation_stays_inside_every_bound(name):
    c = R.case(name)
    probs, out = R.emulate_forward(c)
    res = R.worst_ratios(c, probs=probs, out=out, grads=R.emulate_backward(c, c.P.float()))
    print("emulation %s: worst error / bound: %s" % (name, _fmt(res)))
    assert max(res.values()) <= 1.0
    chained = R.worst_ratios(c, grads=R.emulate_backward(c, probs), chained=True)
    print("emulation %s, own forward probabilities: %s" % (name, _fmt(chained)))
    assert max(chained.values()) <= 1.0
    dead = ~c.live
    if dead.any():
        assert float(probs.transpose(1, 2)[dead].abs().max()) == 0.0


@pytest.mark.parametrize("control", R.control_cases(), ids=lambda c: "%s-%s" % (c[1], c[0]))
def test_negative_controls_break_a_bound(control):
    """every (case, defect) pair where the defect can show (R.defect_shows); a forward defect has to break ``probs`` or ``out``, a backward
    one a gradient computed from the float64 probabilities (the GPU tests' controlled backward)"""
    name, defect = control
    c = R.case(name)
    res = {}
    if defect in R.FORWARD_DEFECTS:
        probs, out = R.emulate_forward(c, defect)
        res.update(R.worst_ratios(c, probs=probs, out=out))
    if defect not in R.FORWARD_DEFECTS or defect == "diag_on_k":
        res.update(R.worst_ratios(c, grads=R.emulate_backward(c, c.P.float(), defect)))
    print("control %s on %s: worst error / bound: %s" % (defect, name, _fmt(res)))
    assert max(res.values()) > 1.0


def test_every_defect_has_a_control_and_the_table_is_right():
    cc = R.control_cases()
    for d in R.DEFECTS:
        assert sum(1 for _, dd in cc if dd == d) >= 2, d
    assert R.defect_shows("k65_ps", "rowsum_no_ps") and not R.defect_shows("k64_relu_vec", "rowsum_no_ps")
    assert R.defect_shows("k64_relu_vec", "diag_partial_skip") and not R.defect_shows("k1_general", "diag_partial_skip")
    assert not R.defect_shows("k384_full", "tile_unmasked") and R.defect_shows("k383_full", "tile_unmasked")
    assert not R.defect_shows("k16_one", "norm_drop_last_tile") and R.defect_shows("k384_full", "norm_drop_last_tile")


@pytest.mark.parametrize("name", [n for n in CASES if R.case(n).regime == "soft"])
def test_soft_cases_are_not_saturated(name):
    """the guard against sliding back to one-hot softmaxes: per sample, the median effective key count 1 / sum p^2 is at least 4, or at
    least n_live / 2 where fewer than 8 keys are live"""
    c = R.case(name)
    neff, nlive = R.effective_keys(c)
    print("soft %s: median effective keys %s of %s live" % (name, [round(float(x), 2) for x in neff], nlive.tolist()))
    for e, n in zip(neff.tolist(), nlive.tolist()):
        assert e >= (4.0 if n >= 8 else n / 2.0) - 1e-9


def test_dispatch_restatement_is_the_library_source():
    """R.dispatch_form - what the case table's ``form`` column and the GPU tests' asserts rest on - against the launch code of
    csrc/sdnet_attention.hip itself: both entry points, the same edges, the attn1 condition and the key limit"""
    forms, n_attn1, max_l2 = R.source_dispatch()
    assert forms["AF"] == forms["AQ"] == (R.PF_EDGES, R.PF_LAST, R.STAGED_ABOVE)
    assert n_attn1 == 2 and max_l2 == R.MAX_L2
    assert [R.dispatch_form(16, n, 0, 0, False) for n in (48, 49, 64, 65, 112, 113, 128, 129, 384)] == [12, 16, 16, 28, 28, 32, 32, "staged", "staged"]
    assert R.dispatch_form(1, 48, 0, 0, False) == "attn1" and R.dispatch_form(1, 48, 1, 0, False) == 12 and R.dispatch_form(1, 48, 0, 0, True) == 12
    assert R.dispatch_form(16, 48, 0, 0, False, prefetch=False) == "staged"


def test_case_list_covers_what_the_issue_lists():
    shp = [R._CASES[n] for n in CASES]
    assert 20 <= len(shp) <= 25
    assert {s[2] for s in shp} >= {1, 16, 17, 48, 49, 64, 65, 112, 113, 128, 129, 383, 384}
    assert {s[1] for s in shp} >= {1, 15, 16, 17, 33}
    assert {s[3] for s in shp} >= {1, 3, 4, 63, 64, 65, 250}
    assert {s[4] for s in shp} >= {1, 5, 63, 64, 65, 250}
    assert {s[0] for s in shp} == {1, 3}
    assert {(s[5], s[6]) for s in shp} == {(r, d) for r in (0, 1) for d in ("none", "one", "vec")}
    assert {s[8] for s in shp} == set(R.REGIMES) and {s[9] for s in shp} == {"full", "holes", "first", "onelast", "ragged"}
    # every dispatch form, both sides of each edge (L2p = 48 | 64 | 112 | 128 | 144), as the case table states it
    for n in CASES:
        B, L1, L2, h, D3, relu, dk, ps, _, _, form = R._CASES[n]
        assert R.dispatch_form(L1, L2, relu, {"none": 0, "one": 1, "vec": h}[dk], ps) == form, n
    forms = {}
    for s in shp:
        forms.setdefault(s[10], set()).add(R.up16(s[2]))
    assert forms[12] >= {16, 32, 48} and forms[16] == {64} and forms[28] >= {80, 112} and forms[32] == {128} and forms["staged"] >= {144, 384}
    assert "attn1" in forms
    for form in (12, 16, 28, 32, "staged"):          # each form also with several h chunks and D3 passes: the prefetch under the MFMAs
        assert any(s[10] == form and s[3] > 64 and s[4] > 64 for s in shp), form
    # L1 == 1 both ways; a full mask at 383 and 384; a prob_scale row with nothing kept; one live key at the end of the last tile
    assert any(s[1] == 1 and s[10] != "attn1" and s[5] for s in shp) and any(s[1] == 1 and s[10] != "attn1" and s[7] for s in shp)
    assert R._CASES["k383_full"][9] == "full" and R._CASES["k384_full"][9] == "full"
    for n in CASES:
        c = R.case(n)
        assert bool(c.live.any(-1).all())
        if c.ps is not None:
            rest = c.ps.view(-1, c.L2)[:-1]                   # every row but the emptied one
            assert float(c.ps[c.B - 1, c.L1 - 1].abs().max()) == 0.0 and abs(float((rest == 0).float().mean()) - R.DROP_P) < 0.15
            assert bool(((rest == 0) | (rest == rest.max())).all()) and abs(float(rest.max()) - 1 / (1 - R.DROP_P)) < 1e-6
        if c.mask_kind == "onelast":
            assert c.live[c.B // 2].nonzero().view(-1).tolist() == [c.L2 - 1]
        if c.mask_kind == "first":
            assert not bool(c.live[:, 0].any())
    off = R.case("k48_offset")
    m = off.S.amax(-1).view(-1)
    assert float(m[0]) > 70 and float(m[1]) < -90            # without the max subtraction expf would overflow / underflow
