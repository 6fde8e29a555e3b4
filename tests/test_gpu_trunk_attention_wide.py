"""The trunk's fused cross-attention at 385 .. 1024 keys (csrc/sdnet_attention_wide.hip: ruart_attn_fwd_wide / ruart_attn_bwd_wide), called by
name through the C ABI and held element by element to the float64 reference at the bounds of tests/_trunk_attention_ref.py, on the cases
of tests/_trunk_attention_wide_ref.py (proven on the CPU, negative controls included, by tests/test_trunk_attention_wide_ref.py); then
ops.fused_attention through autograd at 400 keys, and SDNet / SDNetTrainer with 400 OCR items or objects.  Every kernel test prints its
worst error / bound ratio before it asserts."""
import numpy as np
import pytest
import torch

from ruart_amd import hip, synth
from ruart_amd.arguments import default_opt
from tests import _trunk_attention_ref as R
from tests import _trunk_attention_wide_ref as W
from tests.test_gpu_trunk_attention import GUARD, INVALID, _bits, _fmt, _Guarded, _inputs, _rewritten_masked_rows, dev

pytestmark = pytest.mark.gpu


def _forward(c, pk=None, v=None):
    """one launch of ruart_attn_fwd_wide on case ``c``: (probs, out) on the CPU; NaN-prefilled, guarded outputs"""
    lib, d = hip.load(), dev()
    pa, pk, v, mask, diag, ps = _inputs(c, d, pk, v)
    out, probs = _Guarded((c.B, c.L1, c.D3), c, d), _Guarded((c.B, c.L1, c.L2), c, d)
    rc = lib.ruart_attn_fwd_wide(pa, pk, v, mask, diag, c.diag_len, c.relu, ps, out.t, probs.t, c.B, c.L1, c.L2, c.h, c.D3, hip.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0
    return probs.cpu("probs"), out.cpu("out")


def _backward(c, probs, pk=None, v=None):
    """one launch of ruart_attn_bwd_wide on case ``c`` with the given fp32 probabilities: dict of CPU tensors.  Outputs and the dS
    workspace are prefilled with NaN (the kv kernel must read nothing the q kernel did not write) and guarded."""
    lib, d = hip.load(), dev()
    pa, pk, v, mask, diag, ps = _inputs(c, d, pk, v)
    nt = (c.L1 + 15) // 16
    ga, gk, gv = _Guarded((c.B, c.L1, c.h), c, d), _Guarded((c.B, c.L2, c.h), c, d), _Guarded((c.B, c.L2, c.D3), c, d)
    gd = _Guarded((c.B, nt, c.h), c, d) if c.diag_len > 1 else None
    ds = _Guarded((c.B, c.L1, c.L2), c, d)
    rc = lib.ruart_attn_bwd_wide(pa, pk, v, probs.to(d), c.gout.to(d), diag, c.diag_len, c.relu, ps, ga.t, gk.t, gv.t,
                                 gd.t if gd is not None else None, ds.t, c.B, c.L1, c.L2, c.h, c.D3, hip.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0
    res = dict(grad_pa=ga.cpu("grad_pa"), grad_pk=gk.cpu("grad_pk"), grad_v=gv.cpu("grad_v"), dS=ds.cpu("ds_ws"))
    if gd is not None:
        res["grad_diag_partial"] = gd.cpu("grad_diag_partial")
    return res


def _check_form(c):
    assert W.MIN_L2 <= c.L2 <= W.MAX_L2 and W.dispatch_form(c.L1, c.relu, c.diag_len, c.ps is not None) == c.form


@pytest.mark.parametrize("name", W.cases())
def test_forward_against_float64(name):
    """out and probs inside their element-wise bounds; a masked key's probability is exactly 0 and its pk / v rows reach no result bit; a
    second launch gives the same bits; NaN prefill fully overwritten, guards intact"""
    c = W.case(name)
    _check_form(c)
    dead = ~c.live
    probs, out = _forward(c)
    r = R.worst_ratios(c, probs=probs, out=out)
    print("wide attention forward %s (%s): worst error / bound: %s" % (name, c.form, _fmt(r)))
    assert max(r.values()) <= 1.0
    if dead.any():
        assert not bool(_bits(probs.transpose(1, 2)[dead]).any())
    again = _forward(c)
    assert torch.equal(_bits(again[0]), _bits(probs)) and torch.equal(_bits(again[1]), _bits(out))
    if dead.any():
        pk2, v2 = _rewritten_masked_rows(c)
        other = _forward(c, pk2, v2)
        assert torch.equal(_bits(other[0]), _bits(probs)) and torch.equal(_bits(other[1]), _bits(out))


def _check_backward(c, g, tag, chained=False):
    r = R.worst_ratios(c, grads=g, chained=chained)
    r["dS"] = R.ratio(g["dS"], c.bwd["dS"], R.backward_bounds(c, chained)["dS"]) if c.form != "attn1w" else 0.0
    print("wide attention backward %s: worst error / bound: %s" % (tag, _fmt(r)))
    assert max(r.values()) <= 1.0
    dead = ~c.live
    if dead.any():                                            # masked keys: zero bits in the grad_pk / grad_v rows
        assert not bool(_bits(g["grad_pk"][dead]).any()) and not bool(_bits(g["grad_v"][dead]).any())
    return r


@pytest.mark.parametrize("name", W.cases())
def test_backward_against_float64(name):
    """the backward on inputs the test controls - probs = the float64 P rounded to fp32: grad_pa, grad_pk, grad_v, every grad_diag partial
    and their sum inside their bounds; masked keys: gradients exactly 0, their pk / v rows reach no bit of a live row's gradients; a second
    launch gives the same bits"""
    c = W.case(name)
    _check_form(c)
    probs = c.P.float()
    res = _backward(c, probs)
    _check_backward(c, res, "%s (%s)" % (name, c.form))
    keys = [k for k in res if not (k == "dS" and c.form == "attn1w")]
    again = _backward(c, probs)
    for k in keys:
        assert torch.equal(_bits(again[k]), _bits(res[k])), k
    dead = ~c.live
    if dead.any():
        pk2, v2 = _rewritten_masked_rows(c)
        other = _backward(c, probs, pk2, v2)
        assert not bool(_bits(other["grad_pk"][dead]).any()) and not bool(_bits(other["grad_v"][dead]).any())
        for k in ("grad_pk", "grad_v"):
            assert torch.equal(_bits(other[k][c.live]), _bits(res[k][c.live])), k
        for k in keys:
            if k not in ("grad_pk", "grad_v", "dS"):
                assert torch.equal(_bits(other[k]), _bits(res[k])), k


@pytest.mark.parametrize("regime", W.REGIMES)
def test_forward_into_backward_chain(regime):
    """the kernel's own forward probabilities fed to the backward: the bounds widened by the forward's P bound (chained=True)"""
    c = W.case(W.CHAINED[regime])
    assert c.regime == regime
    probs, out = _forward(c)
    r = R.worst_ratios(c, probs=probs, out=out)
    assert max(r.values()) <= 1.0
    _check_backward(c, _backward(c, probs), "%s chained on the forward's probabilities (%s)" % (c.name, regime), chained=True)


def test_refusals_leave_the_outputs_untouched():
    """L2 = 384 and 1025, a diag_len outside {0, 1, h} and a non-positive dimension: hipErrorInvalidValue from both entry points, nothing
    launched; ruart_attn_fwd_pscale / _bwd_pscale still refuse 385"""
    lib, d = hip.load(), dev()
    B, L1, L2, h, D3 = 2, 5, 1025, 8, 6
    z = lambda *s: torch.zeros(*s, device=d)           # noqa: E731
    f = lambda *s: torch.full(s, GUARD, device=d)      # noqa: E731
    pa, pk, v, mask, diag = z(B, L1, h), z(B, L2, h), z(B, L2, D3), torch.ones(B, L2, dtype=torch.uint8, device=d), torch.ones(h, device=d)
    probs_in, gout, ps = z(B, L1, L2), z(B, L1, D3), torch.ones(B, L1, L2, device=d)
    outs = [f(B, L1, D3), f(B, L1, L2), f(B, L1, h), f(B, L2, h), f(B, L2, D3), f(B, 1, h), f(B, L1, L2)]
    out, probs, ga, gk, gv, gd, ds = outs
    st = hip.stream_ptr()

    def fwd(B=B, L1=L1, L2=400, h=h, D3=D3, dl=h, ps=None, relu=1):
        return lib.ruart_attn_fwd_wide(pa, pk, v, mask, diag, dl, relu, ps, out, probs, B, L1, L2, h, D3, st)

    def bwd(B=B, L1=L1, L2=400, h=h, D3=D3, dl=h, ps=None, relu=1):
        return lib.ruart_attn_bwd_wide(pa, pk, v, probs_in, gout, diag, dl, relu, ps, ga, gk, gv, gd, ds, B, L1, L2, h, D3, st)

    for call in (fwd, bwd):
        for n in (384, 1025, 16, 1):
            assert call(L2=n) == INVALID and call(L2=n, ps=ps) == INVALID, n
        assert call(dl=2) == INVALID and call(dl=h + 1) == INVALID and call(dl=-1) == INVALID
        for dim in ("B", "L1", "L2", "h", "D3"):
            assert call(**{dim: 0}) == INVALID and call(**{dim: -3}) == INVALID, dim
        assert W.dispatch_form(1, 0, 0, False) == "attn1w"                                 # arguments that would take the single-query form
        for n in (384, 1025):
            assert call(L1=1, dl=0, relu=0, L2=n) == INVALID
        assert call(L1=1, dl=0, relu=0, D3=0) == INVALID
    assert lib.ruart_attn_fwd_pscale(pa, pk, v, mask, diag, h, 1, None, out, probs, B, L1, 385, h, D3, st) == INVALID
    assert lib.ruart_attn_bwd_pscale(pa, pk, v, probs_in, gout, diag, h, 1, None, ga, gk, gv, gd, ds, B, L1, 385, h, D3, st) == INVALID
    torch.cuda.synchronize()
    for t in outs:
        assert bool((t == GUARD).all())


@pytest.mark.parametrize("path", ["general", "single-query"])
def test_a_sample_without_live_keys_raises_the_nan_flag(path):
    """every key of a sample masked: no softmax exists (the reference asserts on the NaN); the kernel raises the device flag registered
    through ruart_set_nan_flag, the step's one check reports it, and the flag is clear afterwards.  Live samples raise nothing - a sample
    whose only live key sits in the last key block included."""
    from ruart_amd import ops
    lib, d = hip.load(), dev()
    B, L1, L2, h, D3 = (2, 5, 530, 8, 6) if path == "general" else (2, 1, 530, 8, 6)
    assert W.dispatch_form(L1, 0, 0, False) == ("wide" if path == "general" else "attn1w")
    g = torch.Generator().manual_seed(11)
    pa, pk, v = (torch.randn(*s, generator=g).to(d) for s in ((B, L1, h), (B, L2, h), (B, L2, D3)))
    out, probs = torch.empty(B, L1, D3, device=d), torch.empty(B, L1, L2, device=d)
    flag = ops.nan_flag.ensure(d)
    ops.nan_flag.check_and_clear()
    mask = torch.ones(B, L2, dtype=torch.uint8)
    mask[1] = 0
    mask[1, L2 - 1] = 1                                        # two dead key blocks, then one live key
    assert lib.ruart_attn_fwd_wide(pa, pk, v, mask.to(d), None, 0, 0, None, out, probs, B, L1, L2, h, D3, hip.stream_ptr()) == 0
    torch.cuda.synchronize()
    assert int(flag.item()) == 0 and bool(torch.isfinite(out).all())
    ops.nan_flag.check_and_clear()
    mask[1] = 0
    assert lib.ruart_attn_fwd_wide(pa, pk, v, mask.to(d), None, 0, 0, None, out, probs, B, L1, L2, h, D3, hip.stream_ptr()) == 0
    torch.cuda.synchronize()
    assert int(flag.item()) == 1 and bool(torch.isnan(out[1]).all()) and bool(torch.isfinite(out[0]).all())
    with pytest.raises(AssertionError):
        ops.nan_flag.check_and_clear()
    assert int(flag.item()) == 0
    ops.nan_flag.check_and_clear()


def test_autograd_glue_against_float64_at_400_keys():
    """ops.fused_attention end to end at L2 = 400 (k400_ps: soft, relu, a trainable vector diag, prob_scale, two query tiles per sample):
    the context, the gradients of pk and v, diag.grad = the sum of the per-tile partials, and W.grad through pa = x W^T, all at the float64
    bounds (the kernel's own probabilities go into the backward: the chained bounds; the partial sum and the x^T grad_pa product add
    their own fp32 chains)"""
    from ruart_amd import ops
    d = dev()
    base = W.case("k400_ps")
    assert base.regime == "soft" and base.diag_len == base.h and base.L1 == 17 and base.L2 == 400
    g = torch.Generator().manual_seed(77)
    x = base.pa.clone()
    Wm = torch.eye(base.h) + 0.05 * torch.randn(base.h, base.h, generator=g)
    xd = x.to(d)
    Wd, pkd, vd = (t.to(d).requires_grad_(True) for t in (Wm, base.pk, base.v))
    diagd = base.diag.view(1, 1, -1).to(d).requires_grad_(True)
    pa = xd @ Wd.t()
    y = ops.fused_attention(pa, pkd, vd, base.mask.to(d), diag=diagd, relu=True, prob_scale=base.ps.to(d))
    y.backward(base.gout.to(d))
    torch.cuda.synchronize()
    c = W.variant(base, "pa", pa=pa.detach().cpu().float().contiguous())
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
    print("wide attention through ops.fused_attention (%s): worst error / bound: %s" % (c.name, _fmt(res)))
    assert max(res.values()) <= 1.0


def test_scalar_diag_through_ops_frozen_and_trainable_at_400_keys():
    """The scalar diag of do_similarity through ops.fused_attention at L2 = 400 (k400_ps with its vector diag replaced by the scalar -0.6).
    Frozen, as the model holds it: the context and the gradients of pa, pk, v at the float64 bounds.  Trainable: the backward runs with
    the scalar spread over the h columns - every other gradient keeps its bits - and diag.grad = sum over samples, tiles and columns of
    the partials, held to the partials' bounds plus the fp32 chain of that sum."""
    from ruart_amd import ops
    d = dev()
    c1 = W.variant(W.case("k400_ps"), "scalar", diag=torch.tensor([-0.6]), diag_len=1, diag_kind="one")
    assert c1.L2 == 400 and c1.h > 1
    bb1 = R.backward_bounds(c1, chained=True)
    got = {}
    for kind in ("frozen", "trainable"):
        pa1, pk1, v1 = (t.to(d).requires_grad_(True) for t in (c1.pa, c1.pk, c1.v))
        diag1 = c1.diag.view(1, 1, 1).to(d).requires_grad_(kind == "trainable")
        y1 = ops.fused_attention(pa1, pk1, v1, c1.mask.to(d), diag=diag1, relu=True, prob_scale=c1.ps.to(d))
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
        print("wide attention through ops.fused_attention (%s, %s scalar diag): worst error / bound: %s" % (c1.name, kind, _fmt(res1)))
        assert max(res1.values()) <= 1.0
        got[kind] = [y1.detach().cpu(), pa1.grad.cpu(), pk1.grad.cpu(), v1.grad.cpu()]
    for t0, t1 in zip(got["frozen"], got["trainable"]):
        assert torch.equal(_bits(t0), _bits(t1))


# ------------------------------------------------------------------------------------------------------------------------------
# model level: 400 OCR items / objects
# ------------------------------------------------------------------------------------------------------------------------------
def _T(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def _model(max_ocr_num, max_od_num):
    from ruart_amd.sdnet import SDNet
    opt = default_opt(vocab_size=400, cuda=True, device="cuda:0", bert_precision="x3", max_ocr_num=max_ocr_num, max_od_num=max_od_num)
    cfg = synth.bert_config(vocab_size=500)
    opt["bert_state"], opt["bert_config"] = synth.make_bert_weights(cfg, seed=7, w_std=0.02), cfg
    sw = synth.make_sdnet_weights(opt, seed=7)
    net = SDNet(opt, {"glove_embedding": _T(sw["glove_embed.weight"]), "fast_embedding": _T(sw["fast_embed.weight"])})
    net.load_state_dict({k: _T(v) for k, v in sw.items()})
    return net.to("cuda:0"), opt


def _float64_attention(a, k, v, mask, diag=None, relu=False, prob_scale=None):
    """ops.fused_attention as the float64 composition R.reference_forward, evaluated on the CPU through torch autograd"""
    cpu = lambda t: None if t is None else t.cpu()      # noqa: E731
    out = R.reference_forward(cpu(a), cpu(k), cpu(v), cpu(mask), cpu(diag), relu, cpu(prob_scale))[4]
    return out.float().to(a.device)


def test_sdnet_with_400_ocr_items_against_float64_attention(monkeypatch):
    """SDNet forward + loss + backward at max_ocr_num = 400 (OCR counts [400, 308]: the self-attention and the deep attention levels take
    400 keys), precision x3, dropout 0: as shipped, and with ops.fused_attention replaced by the float64 composition on the CPU.  The two
    runs agree within the x3 tolerances of test_sdnet_forward_backward_vs_reference: probabilities 2e-4, gradient norms 1e-2 relative,
    gradient elements 2e-2 of the tensor's maximum."""
    import ruart_amd.layers as L
    from ruart_amd import ops
    net, opt = _model(400, 40)
    q, ocr, od, gt, _ = synth.synthetic_batch(opt, 2, seed=3, n_q=8, n_ocr=400, n_od=5, bert_vocab=500, ragged=True)
    assert ocr["num_cnt"] == [400, 308]
    L.set_dropout_prob(0.0)
    net.train()
    net.drop_emb = False
    runs = []
    for kind in ("shipped", "float64"):
        if kind == "float64":
            monkeypatch.setattr(ops, "fused_attention", _float64_attention)
        net.zero_grad(set_to_none=True)
        scores, _ = net(q, ocr, od)
        net.check_nan()
        g = gt.to(scores.device)
        loss = torch.nn.functional.binary_cross_entropy_with_logits(scores, g) * g.size(1)
        loss.backward()
        torch.cuda.synchronize()
        runs.append((scores.detach().cpu(), {n: (None if p.grad is None else p.grad.detach().cpu().double()) for n, p in net.named_parameters()}))
    (p0, g0), (p1, g1) = runs
    assert p0.shape == (2, 401) and bool(torch.isfinite(p0).all())
    assert float((p0.sum(1) - 1).abs().max()) <= 1e-5 and float((p1.sum(1) - 1).abs().max()) <= 1e-5
    assert float(p0.max()) < 0.5                                               # not saturated: the comparison below says something
    err = float((p0 - p1).abs().max())
    worst_norm, worst_elem, n_grads = (0.0, ""), (0.0, ""), 0
    for name, ref in g1.items():
        got = g0[name]
        assert (got is None) == (ref is None), name
        if ref is None:
            continue
        n_grads += 1
        worst_norm = max(worst_norm, (abs(float(got.norm()) - float(ref.norm())) / max(float(ref.norm()), 1e-4), name))
        worst_elem = max(worst_elem, (float((got - ref).abs().max()) / max(float(ref.abs().max()), 1e-5), name))
    print("SDNet, 400 OCR items, shipped against float64 attention: max p %.3f, max |dp| %.2e; worst grad-norm rel err %.2e (%s); worst "
          "grad element err / max|g| %.2e (%s); %d gradients" % (float(p0.max()), err, worst_norm[0], worst_norm[1], worst_elem[0],
                                                                   worst_elem[1], n_grads))
    assert n_grads > 20
    assert err < 2e-4
    assert worst_norm[0] < 1e-2, worst_norm
    assert worst_elem[0] < 2e-2, worst_elem


def test_sdnet_with_400_objects_forward():
    """max_od_num = 400 with 400 objects: od_ocr_attn takes 400 keys.  Forward only: finite scores, rows sum to 1."""
    import ruart_amd.layers as L
    net, opt = _model(400, 400)
    q, ocr, od, gt, _ = synth.synthetic_batch(opt, 2, seed=3, n_q=8, n_ocr=400, n_od=400, bert_vocab=500, ragged=True)
    assert max(od["num_cnt"]) == 400
    L.set_dropout_prob(0.0)
    net.eval()
    with torch.no_grad():
        scores, _ = net(q, ocr, od)
    net.check_nan()
    p = scores.cpu()
    assert p.shape == (2, 401) and bool(torch.isfinite(p).all()) and float((p.sum(1) - 1).abs().max()) <= 1e-5


def test_trainer_update_and_predict_with_400_ocr_items():
    """one SDNetTrainer.update() and one predict() at max_ocr_num = 400, built as in test_trainer_update_and_predict"""
    from ruart_amd.trainer import SDNetTrainer
    opt = default_opt(vocab_size=1500, cuda=True, DROPOUT=0.0, dropout_emb=0.0, max_ocr_num=400)
    cfg = synth.bert_config(vocab_size=2000)
    opt["bert_state"], opt["bert_config"] = synth.make_bert_weights(cfg, seed=1033), cfg
    sw = synth.make_sdnet_weights(opt, seed=1033)
    tr = SDNetTrainer(opt, device="cuda:0")
    tr.setup_model({"glove_embedding": _T(sw["glove_embed.weight"]), "fast_embedding": _T(sw["fast_embed.weight"])})
    batch = synth.synthetic_batch(opt, 2, seed=11, n_q=12, n_ocr=400, n_od=9, bert_vocab=2000, ragged=True)
    assert max(batch[1]["num_cnt"]) == 400
    loss = tr.update(tr.ToCUDA(batch), 0)
    assert np.isfinite(loss)
    _, _, _, res, _ = tr.predict(tr.ToCUDA(batch))
    assert len(res) == 2 and all("answer" in r for r in res)
