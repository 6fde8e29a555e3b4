"""opt['bert_optimizer'] without a device: the schedule, the grouping over parameter names, the conf refusals, and the unfused two-group
optimizer (``optim.AdamaxAdam``) in float64 against a step-by-step restatement of both rules."""
import math

import pytest
import torch

from ruart_amd import optim
from ruart_amd.arguments import default_opt


def test_schedule_values():
    m = optim.multiplier
    # x = k / t_total; x / warmup while x < warmup, then 1 - x, never below 0
    assert m(0, 0.5, 8) == 0.0
    assert m(1, 0.5, 8) == (1 / 8) / 0.5 == 0.25
    assert m(3, 0.5, 8) == 0.75
    assert m(4, 0.5, 8) == 0.5                      # the knee: x = warmup is past the warm-up, 1 - x
    assert m(6, 0.5, 8) == 0.25
    assert m(8, 0.5, 8) == 0.0
    assert m(9, 0.5, 8) == 0.0 and m(100, 0.5, 8) == 0.0        # clamped (the reference's goes negative here)
    assert m(1, 0.1, 100) == pytest.approx(0.1, abs=1e-15) and m(10, 0.1, 100) == 0.9
    assert m(0, -1, 8) == 1.0 and m(2, -1, 8) == 0.75            # no warm-up: decay from the first step
    assert m(0, 0.0, 8) == 1.0
    for k in (0, 1, 7, 10 ** 6):
        assert m(k, 0.5, -1) == 1.0 and m(k, -1, -1) == 1.0      # t_total = -1: constant


def test_coefficients_of_both_rules():
    b = (0.9, 0.999)
    a, dec, c = optim.adam_coefficients("adamw", 1e-3, 0.01, b, 3)
    assert a == 1e-3 / (1 - 0.9 ** 3) and dec == 1 - 1e-3 * 0.01 and c == 1 / math.sqrt(1 - 0.999 ** 3)
    assert optim.adam_coefficients("bertadam", 1e-3, 0.01, b, 3) == (1e-3, 1 - 1e-3 * 0.01, 1.0)
    # the schedule reads the COMPLETED steps: the first step of a warmed-up run has lr_t = 0
    assert optim.adam_coefficients("bertadam", 1e-3, 0.01, b, 1, 0.5, 8) == (0.0, 1.0, 1.0)
    assert optim.adam_coefficients("adamw", 1e-3, 0.01, b, 1, 0.5, 8)[:2] == (0.0, 1.0)
    assert optim.adam_coefficients("bertadam", 1e-3, 0.0, b, 3, 0.5, 8) == (1e-3 * 0.5, 1.0, 1.0)
    with pytest.raises(ValueError):
        optim.adam_coefficients("adam", 1e-3, 0.01, b, 1)


NAMES = [
    ("vocab_embed.weight", False), ("fast_embed.weight", True), ("glove_embed.weight", True), ("alphaBERT", True), ("gammaBERT", True),
    ("pre_align.linear.weight", True), ("context_rnn.rnns.0.weight_ih_l0", True), ("context_rnn.rnns.0.bias_ih_l0", True),
    ("ocr_final.LayerNorm.weight", True), ("get_answer.attn.linear.bias", True),
    ("Bert.bert_model.embeddings.word_embeddings.weight", False), ("Bert.bert_model.embeddings.LayerNorm.gamma", False),
    ("Bert.bert_model.encoder.layer.3.attention.self.query.weight", False), ("Bert.bert_model.encoder.layer.3.output.dense.bias", False),
    ("Bert.bert_model.encoder.layer.10.attention.self.query.weight", True), ("Bert.bert_model.encoder.layer.10.attention.self.query.bias", True),
    ("Bert.bert_model.encoder.layer.10.attention.output.LayerNorm.gamma", True),
    ("Bert.bert_model.encoder.layer.10.attention.output.LayerNorm.beta", True),
    ("Bert.bert_model.encoder.layer.11.output.dense.weight", True), ("Bert.bert_model.encoder.layer.11.output.dense.bias", True),
    ("Bert.bert_model.encoder.layer.11.output.LayerNorm.weight", True), ("Bert.bert_model.encoder.layer.11.output.LayerNorm.bias", True),
    ("Bert.bert_model.pooler.dense.weight", True),
]


def test_grouping_over_names():
    named = [(n, torch.nn.Parameter(torch.zeros(2), requires_grad=t)) for n, t in NAMES]
    by_id = {id(p): n for n, p in named}
    trunk, encoder, no_decay = optim.split_parameters(named)
    assert [by_id[id(p)] for p in trunk] == [n for n, t in NAMES[:10] if t]            # the whole trunk, in order, biases and LN included
    assert "alphaBERT" in [by_id[id(p)] for p in trunk] and "glove_embed.weight" in [by_id[id(p)] for p in trunk]
    assert [by_id[id(p)] for p in encoder] == [n for n, t in NAMES[10:] if t]
    assert [by_id[id(p)] for p in no_decay] == [
        "Bert.bert_model.encoder.layer.10.attention.self.query.bias", "Bert.bert_model.encoder.layer.10.attention.output.LayerNorm.gamma",
        "Bert.bert_model.encoder.layer.10.attention.output.LayerNorm.beta", "Bert.bert_model.encoder.layer.11.output.dense.bias",
        "Bert.bert_model.encoder.layer.11.output.LayerNorm.weight", "Bert.bert_model.encoder.layer.11.output.LayerNorm.bias"]
    frozen = set(n for n, t in NAMES if not t)
    assert not frozen & set(by_id[id(p)] for p in trunk + encoder)                       # frozen tensors: in no group
    assert optim.group_of("context_rnn.rnns.0.bias_ih_l0") == "trunk" and optim.group_of("ocr_final.LayerNorm.weight") == "trunk"
    assert optim.group_of("Bert.bert_model.pooler.dense.weight") == "decay"
    assert optim.group_of("Bert.bert_model.embeddings.LayerNorm.gamma") == "no_decay"


def _conf(**kw):
    opt = default_opt(vocab_size=600)
    opt.pop("LOCK_BERT")
    opt.update(kw)
    return opt


def test_conf_keys_and_defaults():
    assert optim.check_bert_optimizer(_conf()) is None
    assert optim.check_bert_optimizer(default_opt()) is None                              # LOCK_BERT without the key: today's conf
    assert optim.check_bert_optimizer(_conf(bert_optimizer="adamw")) == {
        "rule": "adamw", "bert_lr": 5e-5, "weight_decay": 0.01, "warmup": -1, "t_total": -1, "adam_eps": 1e-6}
    got = optim.check_bert_optimizer(_conf(bert_optimizer="bertadam", bert_lr=3e-5, bert_weight_decay=0.0, bert_warmup=0.1, bert_t_total=1000,
                                           bert_adam_eps=1e-8, bert_train_gemm="x3"))
    assert got == {"rule": "bertadam", "bert_lr": 3e-5, "weight_decay": 0.0, "warmup": 0.1, "t_total": 1000, "adam_eps": 1e-8}


@pytest.mark.parametrize("bad", [
    dict(bert_optimizer="adam"),                                   # an unknown rule
    dict(bert_optimizer="adamw", LOCK_BERT=True),                  # nothing of the encoder trains
    dict(bert_optimizer="adamw", optimizer="ADAM2"),               # the group joins the '#' optimizer only
    dict(bert_optimizer="adamw", optimizer="SGD", lr=0.1),
    dict(bert_optimizer="bertadam", bert_warmup=1.0),
    dict(bert_optimizer="bertadam", bert_warmup=-0.5),
    dict(bert_optimizer="bertadam", bert_warmup=1.5),
])
def test_refusals(bad):
    """ValueError from the conf check, and from ``setup_model`` itself before it builds anything."""
    from ruart_amd.trainer import SDNetTrainer
    opt = _conf(**bad)
    with pytest.raises(ValueError):
        optim.check_bert_optimizer(opt)
    tr = SDNetTrainer(dict(opt), device="cpu")
    with pytest.raises(ValueError, match="bert_optimizer|bert_warmup"):
        tr.setup_model(None)
    assert not hasattr(tr, "network")


def _restated_run(rule, steps, lr, bert_lr, wd, eps_a, warmup, t_total, max_norm, shapes_t, shapes_e, no_decay_idx, skip):
    """Both groups step by step in float64, written out here: returns the parameters after every step, and the norms."""
    g = torch.Generator().manual_seed(3)
    rnd = lambda s, scale: torch.randn(*s, generator=g, dtype=torch.float64) * scale
    P = [rnd(s, 0.5) for s in shapes_t + shapes_e]
    nt = len(shapes_t)
    grads = []
    for step in range(steps):
        gs = [rnd(s, 4.0 if step == 1 else 0.05) for s in shapes_t + shapes_e]
        for i in skip:
            if step % 2 == 0:
                gs[i] = None
        grads.append(gs)
    init = [p.clone() for p in P]
    b1, b2 = 0.9, 0.999
    M = [torch.zeros_like(p) for p in P]
    V = [torch.zeros_like(p) for p in P]
    K = [0] * len(P)
    out, norms = [], []
    for gs in grads:
        norm = math.sqrt(sum(float((x * x).sum()) for x in gs if x is not None))
        coef = min(1.0, max_norm / (norm + 1e-6))
        norms.append(norm)
        for i, x in enumerate(gs):
            if x is None:
                continue
            x = x * coef
            K[i] += 1
            k = K[i]
            if i < nt:                                     # Adamax
                M[i] = b1 * M[i] + (1 - b1) * x
                V[i] = torch.maximum(b2 * V[i], x.abs() + 1e-8)
                P[i] = P[i] - lr / (1 - b1 ** k) * M[i] / V[i]
                continue
            done = k - 1                                   # the schedule reads the completed steps
            xs = done / t_total
            mult = 1.0 if t_total == -1 else (xs / warmup if xs < warmup else max(0.0, 1.0 - xs))
            lr_t = bert_lr * mult
            w = 0.0 if (i - nt) in no_decay_idx else wd
            M[i] = b1 * M[i] + (1 - b1) * x
            V[i] = b2 * V[i] + (1 - b2) * x * x
            if rule == "adamw":
                P[i] = P[i] * (1 - lr_t * w) - lr_t / (1 - b1 ** k) * M[i] / (V[i].sqrt() / math.sqrt(1 - b2 ** k) + eps_a)
            else:
                P[i] = P[i] - lr_t * (M[i] / (V[i].sqrt() + eps_a) + w * P[i])
        out.append([p.clone() for p in P])
    return init, grads, out, norms


@pytest.mark.parametrize("rule", ["adamw", "bertadam"])
def test_unfused_two_groups_against_the_restatement(rule):
    shapes_t, shapes_e = [(5, 3), (7,)], [(4, 6), (6,), (9,), (2, 2, 3)]
    conf = dict(lr=2e-3, bert_lr=1e-3, wd=0.01, eps_a=1e-6, warmup=0.25, t_total=8, max_norm=10.0)
    init, grads, want, norms = _restated_run(rule, 6, shapes_t=shapes_t, shapes_e=shapes_e, no_decay_idx={1, 3}, skip={1, 4}, **conf)
    params = [torch.nn.Parameter(p.clone()) for p in init]
    trunk, enc = params[:2], params[2:]
    o = optim.AdamaxAdam(trunk, enc, [enc[1], enc[3]], lr=conf["lr"], bert_lr=conf["bert_lr"], rule=rule, weight_decay=conf["wd"],
                         warmup=conf["warmup"], t_total=conf["t_total"], adam_eps=conf["eps_a"])
    assert [g["lr"] for g in o.param_groups] == [2e-3, 1e-3] and o.pinned == {}
    assert norms[1] > 10.0 > norms[0]                                                    # step 1 clips, the others do not
    for step, gs in enumerate(grads):
        o.zero_grad()
        for p, x in zip(params, gs):
            p.grad = None if x is None else x.clone()
        o.clip_and_step(conf["max_norm"])
        assert abs(float(o.norm_coef[0]) - norms[step]) <= 1e-6 * norms[step]              # (norm_coef is kept in fp32)
        for p, w in zip(params, want[step]):
            assert float((p.detach() - w).abs().max()) <= 1e-12, (step, tuple(p.shape))
    assert o.steps[id(trunk[1])] == 3 and o.steps[id(enc[2])] == 3 and o.steps[id(enc[0])] == 6
    st = o.state
    assert set(st[id(enc[0])]) >= {"exp_avg", "exp_avg_sq"} and set(st[id(trunk[0])]) >= {"exp_avg", "exp_inf"}
    # the first step of the warmed-up run moved no encoder parameter (lr_t = 0) ...
    assert all(torch.equal(want[0][2 + j], init[2 + j]) for j in range(4))
    # ... and the state survives a round trip: one more step on a reloaded copy is bit-equal
    clones = [torch.nn.Parameter(p.detach().clone()) for p in params]
    o2 = optim.AdamaxAdam(clones[:2], clones[2:], [clones[3], clones[5]], lr=conf["lr"], bert_lr=conf["bert_lr"], rule=rule,
                          weight_decay=conf["wd"], warmup=conf["warmup"], t_total=conf["t_total"], adam_eps=conf["eps_a"])
    o2.load_state_dict(o.state_dict())
    for a, b in zip(params, clones):
        a.grad = torch.full_like(a, 0.01)
        b.grad = torch.full_like(b, 0.01)
    o.clip_and_step(10.0)
    o2.clip_and_step(10.0)
    assert all(torch.equal(a, b) for a, b in zip(params, clones))
