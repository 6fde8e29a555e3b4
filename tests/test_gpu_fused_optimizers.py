"""The optimizer confs 'SGD', 'ADAM2' and 'ADAM' on the fused step (``ruart_sgd_step``, ``ruart_adam_step``, ``ruart_adamax_l2_step`` through
``optim.FusedSGD`` / ``FusedAdam`` / ``FusedAdamax(weight_decay=)``): against torch.optim on the device, pinned rows and ``extra_sq``, the
'#' step left bit-identical, the C ABI's refusals, the state round trip, one ``update()`` through the trainer against the unfused arm, and
an exact resume.  Inputs, bounds and the element-wise allowance of the L2 Adamax rule: tests/_optim_ref.py."""
import functools
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from ruart_amd import hip                                  # noqa: E402
from ruart_amd import optim                                # noqa: E402
from ruart_amd import synth                                # noqa: E402
from ruart_amd.arguments import default_opt               # noqa: E402
from tests import _optim_ref as R                          # noqa: E402

DEV = "cuda:0"
RULES = list(R.RULES)
_SECOND = {"ADAM2": "exp_avg_sq", "ADAM": "exp_inf"}


def _fused(rule, params, pinned=None):
    lr, wd = R.RULES[rule]["lr"], R.RULES[rule]["wd"]
    if rule == "SGD":
        return optim.FusedSGD(params, lr=lr, pinned=pinned)
    if rule == "ADAM2":
        return optim.FusedAdam(params, lr=lr, pinned=pinned)
    return optim.FusedAdamax(params, lr=lr, weight_decay=wd, pinned=pinned)


def _torch(rule, params):
    lr, wd = R.RULES[rule]["lr"], R.RULES[rule]["wd"]
    if rule == "SGD":
        return torch.optim.SGD(params, lr=lr)
    if rule == "ADAM2":
        return torch.optim.Adam(params, lr=lr)
    return torch.optim.Adamax(params, lr=lr, weight_decay=wd)


def _adamax_allowance(o_ref, params, before):
    """Per parameter of the torch arm (clipped ``p.grad``, ``before`` the step, its ``exp_inf`` and step count after it): the
    element-wise allowance, None for a tensor that sat the step out."""
    g0 = o_ref.param_groups[0]
    out = []
    for p, b in zip(params, before):
        if p.grad is None:
            out.append(None)
            continue
        clr = g0["lr"] / (1.0 - g0["betas"][0] ** int(o_ref.state[p]["step"]))
        scale = max(1.0, float(p.detach().abs().max()))
        out.append(R.allowance(scale, clr, p.grad, g0["weight_decay"], b, o_ref.state[p]["exp_inf"]))
    return out


@pytest.mark.parametrize("rule", RULES)
def test_matches_torch(rule):
    """The kernel through the optimizer against clip_grad_norm_ + the matching torch.optim class on the device, five steps."""
    init, grads = R.inputs()
    ref = [torch.nn.Parameter(p.to(DEV)) for p in init]
    mine = [torch.nn.Parameter(p.to(DEV)) for p in init]
    o_ref, o = _torch(rule, ref), _fused(rule, mine)
    assert o.param_groups[0]["weight_decay"] == R.RULES[rule]["wd"] and o.param_groups[0]["lr"] == R.RULES[rule]["lr"]
    norms = []
    for step in range(R.STEPS):
        R.set_grads(ref, grads, step)
        R.set_grads(mine, grads, step)
        before = [p.detach().clone() for p in ref]
        norm = float(torch.nn.utils.clip_grad_norm_(ref, R.CLIP))
        o_ref.step()
        o.clip_and_step(R.CLIP)
        norms.append(norm)
        moments = []
        if rule != "SGD":
            moments = [(o_ref.state[a][k], o.state[id(b)][k]) for a, b in zip(ref, mine) if len(o_ref.state[a]) for k in ("exp_avg", _SECOND[rule])]
            assert len(moments) == 2 * (len(R.SHAPES) - (step == 0))
        allow = _adamax_allowance(o_ref, ref, before) if rule == "ADAM" else None
        R.check_step(step, float(o.norm_coef[0]), norm, list(zip(ref, mine)), moments, allow)
        assert abs(float(o.norm_coef[1]) - min(1.0, R.CLIP / norm)) <= 1e-4
    assert norms[1] > 50 * R.CLIP and max(norms[0], norms[2]) < R.CLIP          # step 1 is clipped hard, the others are not
    assert o.steps[id(mine[R.SKIP])] == 2 and o.steps[id(mine[0])] == R.STEPS and o.step_count == R.STEPS
    if rule != "SGD":
        assert int(o_ref.state[ref[R.SKIP]]["step"]) == 2
    assert set(o.state[id(mine[0])]) == ({"exp_avg", _SECOND[rule]} if rule != "SGD" else set())
    assert float((mine[-1].detach().cpu() - init[-1]).abs().max()) > 1e-3       # the updates are orders of magnitude above the bound


@pytest.mark.parametrize("rule", RULES)
def test_pinned_rows_and_extra_sq(rule):
    """A (40, 300) table with 8 trained rows: the others keep their bits; with the left-out rows' squared gradient norm as
    ``extra_sq`` the norm and the clip coefficient are those of the full norm."""
    rows = 8
    init, grads = R.inputs([(40, 300), (8193,)], seed=5)
    gr = grads[1]                                          # the hard-clipped set
    extra = torch.tensor([float(gr[0][rows:].double().pow(2).sum())], device=DEV)
    out = []
    for with_extra in (False, True):
        ps = [torch.nn.Parameter(p.to(DEV)) for p in init]
        o = _fused(rule, ps, pinned={ps[0]: rows})
        assert o.pinned == {id(ps[0]): rows}
        for p, x in zip(ps, gr):
            p.grad = x.to(DEV).clone()
        o.clip_and_step(R.CLIP, extra_sq=extra if with_extra else None)
        out.append(([p.detach().clone() for p in ps], o.norm_coef.double().cpu()))
        assert torch.equal(ps[0].detach()[rows:].cpu(), init[0][rows:])
        assert bool((ps[0].detach()[:rows].cpu() != init[0][:rows]).any(dim=1).all()) and not torch.equal(ps[1].detach().cpu(), init[1])
        if rule != "SGD":
            assert float(o.state[id(ps[0])]["exp_avg"][rows:].abs().max()) == 0 and float(o.state[id(ps[0])]["exp_avg"][:rows].abs().max()) > 0
    (pa, na), (pb, nb) = out
    want = float(torch.cat([x.flatten() for x in gr]).double().norm())
    assert abs(float(na[0]) - want) <= 1e-4 * want and float(na[1]) < 0.05
    assert bool(((na - nb).abs() <= 1e-6 * na.abs()).all()), (na, nb)


def test_adamax_without_decay_is_the_step_it_was():
    """``FusedAdamax(weight_decay=0)`` against an instance built without the argument: parameters and moments bit-equal after five steps
    (both launch ``ruart_adamax_step``), and both differ from the decayed rule."""
    init, grads = R.inputs()
    arms = []
    for kw in ({}, {"weight_decay": 0}, {"weight_decay": 0.5}):
        ps = [torch.nn.Parameter(p.to(DEV)) for p in init]
        o = optim.FusedAdamax(ps, lr=2e-3, **kw)
        assert o.param_groups[0]["weight_decay"] == kw.get("weight_decay", 0)
        for step in range(R.STEPS):
            R.set_grads(ps, grads, step)
            o.clip_and_step(R.CLIP)
        arms.append((ps, o))
    (pa, oa), (pb, ob), (pc, _) = arms
    for x, y, z in zip(pa, pb, pc):
        assert torch.equal(x, y) and not torch.equal(x, z)
        assert all(torch.equal(oa.state[id(x)][k], ob.state[id(y)][k]) for k in ("exp_avg", "exp_inf"))
    assert torch.equal(oa.norm_coef, ob.norm_coef)


def test_c_abi_refusals():
    """``ruart_sgd_step`` and ``ruart_adamax_l2_step`` with no chunks or without a table: hipErrorInvalidValue, nothing launched."""
    lib = hip.load()
    n = 4096
    p, g, m, u = (torch.full((n,), x, device=DEV) for x in (1.0, 0.5, 0.25, 0.125))
    tabs = torch.tensor([[t.data_ptr()] for t in (p, g, m, u)], dtype=torch.int64, device=DEV)
    chunk = torch.tensor([0, 0, n], dtype=torch.int32, device=DEV)
    clr = torch.tensor([1e-2], device=DEV)
    P = hip.ptr
    invalid = 1                                             # hipErrorInvalidValue

    def sgd(n_chunks=1, params=P(tabs[0]), grads_=P(tabs[1]), ct=P(chunk[0:1])):
        return lib.ruart_sgd_step(params, grads_, ct, P(chunk[1:2]), P(chunk[2:3]), n_chunks, None, 0.1, hip.stream_ptr())

    def l2(n_chunks=1, params=P(tabs[0]), table=P(clr), second=P(tabs[3])):
        return lib.ruart_adamax_l2_step(params, P(tabs[1]), P(tabs[2]), second, P(chunk[0:1]), P(chunk[1:2]), P(chunk[2:3]), n_chunks, None,
                                        table, 0.9, 0.999, 1e-8, 0.5, hip.stream_ptr())

    assert [sgd(0), sgd(-1), sgd(params=None), sgd(grads_=None), sgd(ct=None)] == [invalid] * 5
    assert [l2(0), l2(-1), l2(params=None), l2(table=None), l2(second=None)] == [invalid] * 5
    torch.cuda.synchronize()
    for t, x in ((p, 1.0), (g, 0.5), (m, 0.25), (u, 0.125)):
        assert bool((t == x).all())
    assert sgd() == 0                                       # the same arguments, complete: it runs
    torch.cuda.synchronize()
    assert bool(((p - 0.95).abs() < 1e-6).all()) and bool((g == 0.5).all()) and bool((m == 0.25).all())      # p - lr g
    assert l2() == 0
    torch.cuda.synchronize()
    assert bool((p < 0.949).all()) and bool((m != 0.25).all()) and bool((u != 0.125).all()) and bool((g == 0.5).all())


@pytest.mark.parametrize("rule", RULES)
def test_state_dict_round_trip(rule):
    """Three steps, save, load into a fresh optimizer over cloned parameters, two more steps on both: bit-equal to the uninterrupted run."""
    init, grads = R.inputs([(50, 30), (1000,), (300, 1024), (768,), (8193,)], seed=3)
    skip = 3
    make = lambda params: _fused(rule, params, pinned={params[0]: 20})
    a = [torch.nn.Parameter(p.to(DEV)) for p in init]
    oa = make(a)
    for step in range(3):
        R.set_grads(a, grads, step, skip)
        oa.clip_and_step(R.CLIP)
    b = [torch.nn.Parameter(p.detach().clone()) for p in a]
    ob = make(b)
    sd = oa.state_dict()
    assert sd["param_groups"][0]["weight_decay"] == R.RULES[rule]["wd"] and "params" not in sd["param_groups"][0]
    ob.load_state_dict(sd)
    assert [ob.steps[id(p)] for p in b] == [3, 3, 3, 1, 3] and ob.step_count == 3
    for step in (3, 4):
        R.set_grads(a, grads, step, skip)
        R.set_grads(b, grads, step, skip)
        oa.clip_and_step(R.CLIP)
        ob.clip_and_step(R.CLIP)
        assert torch.equal(oa.norm_coef, ob.norm_coef)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
        assert oa.state[id(x)].keys() == ob.state[id(y)].keys()
        assert all(torch.equal(oa.state[id(x)][k], ob.state[id(y)][k]) for k in oa.state[id(x)])
    assert not torch.equal(a[2].detach().cpu(), init[2])


# -- through the trainer --------------------------------------------------------------------------------------------------------
CONFS = {"SGD": ("FusedSGD", "SGD", dict(lr=0.1)), "ADAM2": ("FusedAdam", "Adam", {}), "ADAM": ("FusedAdamax", "Adamax", {})}


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a))


@functools.lru_cache(maxsize=None)
def _bert():
    """(synthetic bert-base checkpoint, its config with both dropouts 0) - built once per module and never written to"""
    cfg = synth.bert_config(vocab_size=2000, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    return synth.make_bert_weights(cfg, seed=7, w_std=0.02), cfg


def _opt(conf, **extra):
    # (tune_partial: the shipped 1000 is beyond this vocabulary - 100 leaves 500 re-pinned rows per table to look at)
    opt = default_opt(vocab_size=600, cuda=True, DROPOUT=0.0, dropout_emb=0.0, optimizer=conf, tune_partial=100)
    opt.update(CONFS[conf][2])
    opt.update(extra)
    assert "TUNE_PARTIAL" in opt and "LOCK_BERT" in opt
    opt["bert_state"], opt["bert_config"] = _bert()
    return opt


def _trainer(opt):
    from ruart_amd.trainer import SDNetTrainer
    sw = synth.make_sdnet_weights(opt, seed=7)
    tr = SDNetTrainer(dict(opt), device=DEV)
    tr.setup_model({"glove_embedding": T(sw["glove_embed.weight"]), "fast_embedding": T(sw["fast_embed.weight"])})
    return tr


def _batch(tr, opt, i=0):
    return tr.ToCUDA(synth.synthetic_batch(opt, 3, seed=31 + i, n_q=10, n_ocr=14, n_od=5, bert_vocab=2000, ragged=True))


def _snapshot(tr):
    return {n: p.detach().clone() for n, p in tr.network.named_parameters()}


def _pinned_rows_hold(tr, opt):
    tp = opt["tune_partial"]
    for flag, name, fixed in (("FastText", "fast_embed", "fixed_embedding_fast"), ("GLOVE", "glove_embed", "fixed_embedding_glove")):
        if flag in opt:
            assert getattr(tr.network, fixed).shape[0] == 600 - tp
            assert torch.equal(getattr(tr.network, name).weight.detach()[tp:], getattr(tr.network, fixed)), name


@pytest.mark.parametrize("conf", RULES)
def test_fused_update_matches_unfused(conf, monkeypatch):
    """One ``update()`` of two trainers built from the same seeds, ``ruart_fused_optimizer`` True against False - the step is
    deterministic, so both arms see the same gradients."""
    norms = []
    clip = torch.nn.utils.clip_grad_norm_

    def spy(*a, **kw):
        norms.append(float(clip(*a, **kw)))
        return norms[-1]
    monkeypatch.setattr(torch.nn.utils, "clip_grad_norm_", spy)
    res = []
    for fused in (True, False):
        opt = _opt(conf, ruart_fused_optimizer=fused)
        tr = _trainer(opt)
        o = tr.optimizer
        assert type(o) is (getattr(optim, CONFS[conf][0]) if fused else getattr(torch.optim, CONFS[conf][1]))
        assert hasattr(o, "clip_and_step") == fused and len(o.param_groups) == 1
        want_lr = {"SGD": 0.1, "ADAM2": opt["lr"], "ADAM": 1e-3}[conf]
        assert o.param_groups[0]["lr"] == want_lr and o.param_groups[0]["weight_decay"] == (0.5 if conf == "ADAM" else 0)
        if fused:
            tables = [tr.network.fast_embed.weight, tr.network.glove_embed.weight]
            assert o.pinned == {id(w): opt["tune_partial"] for w in tables if w.requires_grad} and o.pinned
        before = _snapshot(tr)
        loss = float(tr.update(_batch(tr, opt), 0))
        torch.cuda.synchronize()
        _pinned_rows_hold(tr, opt)
        allow = None
        if fused:
            assert not norms
            norm = float(o.norm_coef[0])
        else:
            assert len(norms) == 1
            norm = norms[0]
            if conf == "ADAM":
                named = [(n, p) for n, p in tr.network.named_parameters()]
                al = _adamax_allowance(o, [p for _, p in named], [before[n] for n, _ in named])      # (a frozen tensor has no gradient: None)
                allow = {n: a for (n, _), a in zip(named, al)}
        res.append((loss, before, _snapshot(tr), norm, allow))
        tr.close()
    (la, b_a, a, na, _), (lb, b_b, b, nb, allow) = res
    assert la == lb and la == la and all(torch.equal(b_a[n], b_b[n]) for n in b_a)
    names = list(a)
    R.check_step(0, na, nb, [(b[n], a[n]) for n in names], [], [allow[n] for n in names] if allow is not None else None)
    moved = sum(1 for n in names if not n.startswith("Bert.") and not torch.equal(a[n], b_a[n]))
    assert moved >= 10, moved
    assert all(torch.equal(a[n], b_a[n]) for n in names if n.startswith("Bert.bert_model."))       # LOCK_BERT: frozen in both arms


def test_without_the_key_the_confs_stay_on_torch_optim():
    for conf in RULES:
        opt = _opt(conf)
        assert "ruart_fused_optimizer" not in opt
        tr = _trainer(opt)
        assert type(tr.optimizer) is getattr(torch.optim, CONFS[conf][1]) and not hasattr(tr.optimizer, "clip_and_step")
        tr.close()


def _state(tr, losses):
    tr.flush_readback()
    torch.cuda.synchronize()
    o = tr.optimizer
    out = {"losses": losses, "updates": tr.updates, "step_count": o.step_count}
    for n, p in tr.network.named_parameters():
        out["p." + n] = p.detach().cpu().clone()
        if id(p) in o.state:
            out["steps." + n] = o.steps[id(p)]
            for k, v in o.state[id(p)].items():
                out[k + "." + n] = v.detach().cpu().clone()
    return out


def test_adam2_resumes_bit_for_bit(tmp_path):
    """'ADAM2' on the fused step: three ``update()``s, ``save``, a new trainer, ``load_state``, two more - losses, parameters, moments and
    step counts bit-equal to five uninterrupted steps; a file of another weight decay or class is refused."""
    opt = _opt("ADAM2", ruart_fused_optimizer=True)
    path = os.path.join(str(tmp_path), "adam2.pt")

    tr = _trainer(opt)
    batches = [_batch(tr, opt, i) for i in range(5)]                 # (every trainer ships its own copies)
    want = _state(tr, [float(tr.update(batches[i], i)) for i in range(5)])
    tr.close()

    tr = _trainer(opt)
    batches = [_batch(tr, opt, i) for i in range(5)]
    first = [float(tr.update(batches[i], i)) for i in range(3)]
    tr.flush_readback()
    tr.save(path, epoch=0)
    tr.close()
    ckpt = torch.load(path, map_location="cpu", weights_only=True)
    assert ckpt["ruart"]["optimizer_class"] == "FusedAdam" == optim.FusedAdam.__name__ and ckpt["state_dict"]["updates"] == 3
    assert max(ckpt["state_dict"]["optimizer"]["steps"]) == 3

    tr = _trainer(opt)
    assert tr.load_state(path) == 3
    batches = [_batch(tr, opt, i) for i in range(5)]
    got = _state(tr, first + [float(tr.update(batches[i], i)) for i in range(3, 5)])
    tr.close()
    assert set(got) == set(want) and len([k for k in want if k.startswith("exp_avg_sq.")]) > 10
    bad = [k for k, v in want.items() if not (torch.equal(v, got[k]) if torch.is_tensor(v) else v == got[k])]
    assert not bad, "%d differences between the resumed and the uninterrupted run, e.g. %s" % (len(bad), bad[:6])
    assert want["updates"] == 5 and want["step_count"] == 5 and all(x == x for x in want["losses"])
    assert max(v for k, v in want.items() if k.startswith("steps.")) == 5

    tr = _trainer(_opt("ADAM", ruart_fused_optimizer=True))
    with pytest.raises(ValueError, match="optimizer class FusedAdam in the file.*FusedAdamax"):
        tr.load_state(path)
    tr.close()
