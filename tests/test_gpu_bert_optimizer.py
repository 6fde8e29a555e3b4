"""opt['bert_optimizer'] through the trainer on the GPU: who sits in which group, the fused step against the unfused one, warm-up, and the
conf without the key left as it was.  Set-up of tests/test_gpu_bert_train_layers.py (``_trainer``): the top two layers of a synthetic
bert-base train on the 16-bit kernels, every dropout off, the trunk's learning rate left at its default."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from ruart_amd import synth                               # noqa: E402
from ruart_amd.arguments import default_opt               # noqa: E402

DEV = "cuda:0"
ENC = "Bert.bert_model."


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a))


@functools.lru_cache(maxsize=None)
def _bert():
    """(synthetic bert-base checkpoint, its config with both dropouts 0) - built once per module and never written to"""
    cfg = synth.bert_config(vocab_size=2000, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    return synth.make_bert_weights(cfg, seed=7, w_std=0.02), cfg


def _opt(**extra):
    opt = default_opt(vocab_size=600, cuda=True, DROPOUT=0.0, dropout_emb=0.0, bert_train_gemm="16", bert_train_layers=2)
    opt.pop("LOCK_BERT")
    opt.update(extra)
    opt["bert_state"], opt["bert_config"] = _bert()
    return opt


def _trainer(**extra):
    from ruart_amd.trainer import SDNetTrainer
    opt = _opt(**extra)
    sw = synth.make_sdnet_weights(opt, seed=7)
    tr = SDNetTrainer(opt, device=DEV)
    tr.setup_model({"glove_embedding": T(sw["glove_embed.weight"]), "fast_embedding": T(sw["fast_embed.weight"])})
    return tr, opt


def _batch(tr, opt):
    return tr.ToCUDA(synth.synthetic_batch(opt, 3, seed=31, n_q=10, n_ocr=14, n_od=5, bert_vocab=2000, ragged=True))


def _snapshot(tr):
    return {n: p.detach().clone() for n, p in tr.network.named_parameters()}


def test_group_membership_on_the_model():
    from ruart_amd.optim import FusedAdamaxAdam
    tr, opt = _trainer(bert_optimizer="adamw", bert_lr=3e-5)
    o = tr.optimizer
    assert isinstance(o, FusedAdamaxAdam)
    assert len(o.param_groups) == 2 and [g["lr"] for g in o.param_groups] == [opt["lr"], 3e-5]      # the conf's trunk rate, untouched
    assert o.param_groups[1]["weight_decay"] == 0.01 and o.param_groups[1]["eps"] == 1e-6 and o.param_groups[1]["rule"] == "adamw"
    trunk, enc = set(id(p) for p in o.param_groups[0]["params"]), set(id(p) for p in o.param_groups[1]["params"])
    names = dict(tr.network.named_parameters())
    n_enc = 0
    for n, p in names.items():
        if not p.requires_grad:                             # frozen: in no group, no state
            assert id(p) not in trunk and id(p) not in enc and id(p) not in o.state, n
        elif n.startswith(ENC):
            n_enc += 1
            # (the pooler is trainable by name and never gets a gradient: in the group, never stepped)
            assert ".layer.10." in n or ".layer.11." in n or ".pooler." in n, n
            assert id(p) in enc and id(p) not in trunk and set(o.state[id(p)]) == {"exp_avg", "exp_avg_sq"}, n
            assert (id(p) in o.no_decay) == (n.endswith(".bias") or "LayerNorm" in n), n
        else:
            assert id(p) in trunk and id(p) not in enc and set(o.state[id(p)]) == {"exp_avg", "exp_inf"}, n
    assert n_enc == 32 + 2 and len(o.no_decay) == 2 * 10 + 1     # per layer: six biases, two LayerNorms of two tensors; the pooler's bias
    assert sum(1 for n in names if ".layer.10." in n or ".layer.11." in n) == 32
    assert sum(1 for n, p in names.items() if n.startswith(ENC) and not p.requires_grad) == 5 + 160
    for n in ("alphaBERT", "gammaBERT"):                    # the linear-combine weights stay with the trunk
        assert id(names[n]) in trunk
    if "TUNE_PARTIAL" in opt:
        assert o.pinned and set(o.pinned) <= trunk
    tr.close()


def test_fused_update_matches_unfused():
    """One ``update()`` of two trainers built from the same seeds - the step is deterministic, so both arms see the same gradients."""
    from ruart_amd.optim import AdamaxAdam, FusedAdamaxAdam
    res = []
    for fused in (True, False):
        tr, opt = _trainer(bert_optimizer="adamw", ruart_fused_optimizer=fused)
        assert type(tr.optimizer) is (FusedAdamaxAdam if fused else AdamaxAdam)
        before = _snapshot(tr)
        loss = float(tr.update(_batch(tr, opt), 0))
        res.append((loss, before, _snapshot(tr), float(tr.optimizer.norm_coef[0])))
        tr.close()
    (la, b_a, a, na), (lb, b_b, b, nb) = res
    assert la == lb and all(torch.equal(b_a[n], b_b[n]) for n in b_a)
    assert abs(na - nb) <= 1e-4 * nb
    moved = 0
    for n in a:
        err = float((a[n] - b[n]).abs().max())
        assert err <= 2e-6 * max(1.0, float(b[n].abs().max())), (n, err)
        moved += int(n.startswith(ENC) and not torch.equal(a[n], b_a[n]))
    weights = [n for n in a if (".layer.10." in n or ".layer.11." in n) and n.endswith("dense.weight")]
    assert len(weights) == 6 and moved >= 6 and not [n for n in weights if torch.equal(a[n], b_a[n])]      # the encoder group stepped


def test_warmup_through_the_trainer():
    tr, opt = _trainer(bert_optimizer="bertadam", bert_warmup=0.5, bert_t_total=4)
    batch = _batch(tr, opt)
    s0 = _snapshot(tr)
    losses = [float(tr.update(batch, 0))]
    s1 = _snapshot(tr)
    enc = [n for n in s0 if n.startswith(ENC)]
    assert all(torch.equal(s0[n], s1[n]) for n in enc), [n for n in enc if not torch.equal(s0[n], s1[n])][:3]     # lr_t = 0
    assert not torch.equal(s0["alphaBERT"], s1["alphaBERT"])
    assert sum(1 for n in s0 if not n.startswith(ENC) and not torch.equal(s0[n], s1[n])) > 10                     # the trunk has moved
    w11 = ENC + "encoder.layer.11.output.dense.weight"
    assert float(tr.optimizer.state[id(dict(tr.network.named_parameters())[w11])]["exp_avg_sq"].abs().max()) > 0
    losses.append(float(tr.update(batch, 1)))
    s2 = _snapshot(tr)
    w3 = ENC + "encoder.layer.3.output.dense.weight"
    assert not torch.equal(s1[w11], s2[w11]) and torch.equal(s0[w3], s2[w3])
    losses += [float(tr.update(batch, i)) for i in (2, 3)]
    assert len(losses) == 4 and all(np.isfinite(losses)), losses
    tr.close()


def test_default_untouched():
    """Without the key: a ``FusedAdamax`` over one list, as before; and the key does not combine with LOCK_BERT."""
    from ruart_amd.optim import FusedAdamax
    from ruart_amd.trainer import SDNetTrainer
    res = []
    for _ in range(2):
        tr, opt = _trainer()
        assert "bert_optimizer" not in opt and type(tr.optimizer) is FusedAdamax and len(tr.optimizer.param_groups) == 1
        assert any(id(p) in tr.optimizer.state for n, p in tr.network.named_parameters() if n.startswith(ENC + "encoder.layer.11."))
        batch = _batch(tr, opt)
        res.append(([float(tr.update(batch, i)) for i in range(3)], _snapshot(tr)))
        tr.close()
    assert res[0][0] == res[1][0], (res[0][0], res[1][0])
    assert not [n for n in res[0][1] if not torch.equal(res[0][1][n], res[1][1][n])]
    opt = _opt(bert_optimizer="adamw")
    opt.pop("bert_train_layers")
    opt["LOCK_BERT"] = True
    with pytest.raises(ValueError, match="LOCK_BERT"):
        SDNetTrainer(opt, device=DEV).setup_model(None)
