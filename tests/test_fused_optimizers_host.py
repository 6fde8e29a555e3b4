"""The optimizer confs 'SGD', 'ADAM2' and 'ADAM' without a GPU: the float64 restatement (tests/_optim_ref.py) holds torch.optim in fp32
inside the bounds the GPU tests use, three deliberately wrong restatements break them by two orders of magnitude, ``select_optimizer``
names the class of every conf, and ``train_state.check`` refuses a file written under another weight decay."""
import pytest
import torch

from ruart_amd import layers as L
from ruart_amd import optim
from ruart_amd import train_state as TS
from tests import _optim_ref as R


def _torch_optimizer(rule, params):
    lr, wd = R.RULES[rule]["lr"], R.RULES[rule]["wd"]
    if rule == "SGD":
        return torch.optim.SGD(params, lr=lr)
    if rule == "ADAM2":
        return torch.optim.Adam(params, lr=lr)
    return torch.optim.Adamax(params, lr=lr, weight_decay=wd)


_SECOND = {"ADAM2": "exp_avg_sq", "ADAM": "exp_inf"}


@pytest.mark.parametrize("rule", list(R.RULES))
def test_torch_fp32_is_inside_the_bounds(rule):
    """clip_grad_norm_ + torch.optim in fp32 on the CPU against the restatement, five steps; at most half of any bound is used."""
    init, grads = R.inputs()
    lr, wd = R.RULES[rule]["lr"], R.RULES[rule]["wd"]
    ps = [torch.nn.Parameter(p.clone()) for p in init]
    o = _torch_optimizer(rule, ps)
    ref = R.Reference(rule, init, lr, wd)
    norms, worst = [], 0.0
    for step in range(R.STEPS):
        R.set_grads(ps, grads, step)
        norm = float(torch.nn.utils.clip_grad_norm_(ps, R.CLIP))
        o.step()
        norm_ref, _ = ref.step(R.step_grads(grads, step))
        norms.append(norm_ref)
        moments, allow = [], None
        if rule != "SGD":
            moments = [(ref_t[k], o.state[p][name]) for k, p in enumerate(ps) if len(o.state[p])
                       for ref_t, name in ((ref.m, "exp_avg"), (ref.s, _SECOND[rule]))]
            assert len(moments) == 2 * (len(R.SHAPES) - (step == 0))
        if rule == "ADAM":
            allow = []
            for k in range(len(ps)):
                if ref.last[k] is None or R.step_grads(grads, step)[k] is None:
                    allow.append(None)
                    continue
                g, before, clr = ref.last[k]
                allow.append(R.allowance(max(1.0, float(ref.p[k].abs().max())), clr, g, wd, before, ref.s[k]))
        worst = max(worst, R.check_step(step, norm, norm_ref, list(zip(ref.p, ps)), moments, allow))
    assert norms[1] > 50 * R.CLIP and max(norms[0], norms[2]) < R.CLIP            # step 1 is clipped hard, the others are not
    assert ref.steps[R.SKIP] == 2 and ref.steps[0] == R.STEPS
    if rule != "SGD":
        assert int(o.state[ps[R.SKIP]]["step"]) == 2 and int(o.state[ps[0]]["step"]) == R.STEPS
    assert float((ps[-1].detach() - init[-1]).abs().max()) > 1e-3                 # the updates are orders of magnitude above the bound
    assert worst < 0.5, worst


@pytest.mark.parametrize("rule,wrong", [("SGD", "no_clip"), ("ADAM2", "no_bc2"), ("ADAM", "decoupled")])
def test_wrong_restatements_break_the_bound(rule, wrong):
    """The clip coefficient not applied, the second bias correction missing, the decay decoupled: each is off by at least 100 times
    the parameter bound on the same inputs."""
    init, grads = R.inputs()
    lr, wd = R.RULES[rule]["lr"], R.RULES[rule]["wd"]
    good, bad = R.Reference(rule, init, lr, wd), R.Reference(rule, init, lr, wd, wrong=wrong)
    for step in range(R.STEPS):
        good.step(R.step_grads(grads, step))
        bad.step(R.step_grads(grads, step))
    a, b = good.p[-1], bad.p[-1]
    scale = max(1.0, float(a.abs().max()))
    err = float((a - b).abs().max())
    print("%s / %s: error %.3g of the scale" % (rule, wrong, err / scale))
    assert err >= 100 * R.P_TOL * scale, (err, scale)


def test_reference_pinned_rows_and_extra_sq():
    """The restatement's own pinned rows: left alone, and with the left-out rows' squared norm as ``extra_sq`` the norm is the full one."""
    init, grads = R.inputs([(40, 300), (100,)], seed=5)
    for rule in R.RULES:
        full = R.Reference(rule, init, R.RULES[rule]["lr"], R.RULES[rule]["wd"], pinned={0: 8})
        part = R.Reference(rule, init, R.RULES[rule]["lr"], R.RULES[rule]["wd"], pinned={0: 8})
        n0, c0 = full.step(grads[1])
        n1, c1 = part.step(grads[1], extra_sq=float(grads[1][0][8:].double().pow(2).sum()))
        assert abs(n0 - n1) <= 1e-12 * n0 and abs(c0 - c1) <= 1e-12 * c0
        assert torch.equal(full.p[0][8:], init[0][8:].double()) and not torch.equal(full.p[0][:8], init[0][:8].double())
        assert torch.equal(full.p[0], part.p[0])


@pytest.mark.parametrize("device_type", ["cpu", "cuda"])
@pytest.mark.parametrize("key", ["absent", True, False])
@pytest.mark.parametrize("o", ["#", "ADAM", "ADAM2", "SGD"])
def test_select_optimizer(o, key, device_type):
    opt = {"optimizer": o, "lr": 0.1}
    if key != "absent":
        opt["ruart_fused_optimizer"] = key
    plain = {"#": "Adamax", "ADAM": "Adamax", "ADAM2": "Adam", "SGD": "SGD"}[o]
    fused = {"#": "FusedAdamax", "ADAM": "FusedAdamax", "ADAM2": "FusedAdam", "SGD": "FusedSGD"}[o]
    on = device_type == "cuda" and (key is True or (key == "absent" and o == "#"))      # only '#' is fused without the key
    assert optim.select_optimizer(opt, device_type) == (fused if on else plain)
    assert hasattr(optim, fused) and hasattr(torch.optim, plain)
    if o == "#":
        assert optim.select_optimizer(dict(opt, bert_optimizer="adamw"), device_type) == ("FusedAdamaxAdam" if on else "AdamaxAdam")


def test_select_optimizer_refuses_an_unknown_value():
    with pytest.raises(ValueError, match="optimizer is wrong"):
        optim.select_optimizer({"optimizer": "RMSPROP", "ruart_fused_optimizer": True}, "cuda")


class _Meter:
    val, avg, sum, count = 0.25, 0.5, 1.5, 3


def test_train_state_refuses_another_weight_decay():
    """'#' and 'ADAM' build one class: a file of the one must not load into a run of the other (both ways), the same decay passes."""
    named = {"w": torch.nn.Parameter(torch.ones(4, 3)), "b": torch.nn.Parameter(torch.ones(3))}
    ps = list(named.values())
    make = lambda wd: torch.optim.Adamax(ps, lr=1e-3, weight_decay=wd)
    ranks = [TS.capture_rank(None, {"front": L.MaskBank()})]
    files = {wd: TS.pack(dict(named), make(wd), 0, _Meter, {}, trainable=list(named), ranks=ranks) for wd in (0, 0.5)}
    for wd in (0, 0.5):
        assert files[wd]["state_dict"]["optimizer"]["param_groups"][0]["weight_decay"] == wd
        TS.check(files[wd], make(wd), named, list(named), world=1)
    with pytest.raises(ValueError, match="weight decay 0.5 in the file.*has 0"):
        TS.check(files[0.5], make(0), named, list(named), world=1)
    with pytest.raises(ValueError, match="weight decay 0 in the file.*has 0.5"):
        TS.check(files[0], make(0.5), named, list(named), world=1)
