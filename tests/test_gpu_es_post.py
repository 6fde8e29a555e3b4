"""``no_Context_Self_Attention`` on the MI355X: SDNet end to end against the unmodified reference (tests/golden/sdnet_e2e_noctx.npz,
written by tools/gen_golden_es_post.py), the conf in the three-stream schedule and SDNetTrainer (update, predict, checkpoint).  And the
attention kernels at the shape and masks the ES tail of ``ES_using_way post_process`` would call them with, against float64 - that
branch itself is not part of the model (the constructor refuses it), and the captured trunk (opt['ruart_graph_trunk']) refuses the new
conf (tests/test_es_post_host.py)."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from ruart_amd import synth                               # noqa: E402
from ruart_amd.arguments import default_opt               # noqa: E402
from tests.test_es_post_host import T                      # noqa: E402

DEV = "cuda:0"
# the project's standing end-to-end bounds (test_sdnet_yesno_forward_backward_vs_reference): scores / gradient norms per precision
BOUNDS = {"fp32": (5e-5, 2e-3), "x3": (2e-4, 1e-2), "fp16c": (2e-4, 1e-2)}


def maxerr(a, b):
    return float((a.detach().double().cpu() - b.detach().double().cpu()).abs().max())


# ---- attention at the ES tail's shape: 10 query rows (less than one 16-row tile), a 90-key panel ---------------------------------------------
def _attn_case(live, seed):
    B, L1, L2, h, D3 = len(live), 10, 90, 125, 500
    g = torch.Generator().manual_seed(seed)
    pa, pk, v = torch.randn(B, L1, h, generator=g), torch.randn(B, L2, h, generator=g), torch.randn(B, L2, D3, generator=g)
    gy = torch.randn(B, L1, D3, generator=g)
    mask = torch.zeros(B, L2, dtype=torch.uint8)
    for b, n in enumerate(live):
        mask[b, :n] = 1
    diag = torch.full((1, 1, 1), 1.0 / h ** 0.5)
    return pa, pk, v, gy, mask, diag


def _attn_float64(pa, pk, v, gy, mask, diag):
    leaves = [t.double().requires_grad_() for t in (pa, pk, v)]
    s = torch.bmm(torch.relu(leaves[0]) * diag.double(), torch.relu(leaves[1]).transpose(1, 2))
    ref = torch.bmm(torch.softmax(s.masked_fill(mask.eq(0).unsqueeze(1), float("-inf")), 2), leaves[2])
    ref.backward(gy.double())
    return ref.detach(), [t.grad for t in leaves]


def _attn_device(pa, pk, v, gy, mask, diag):
    from ruart_amd import ops
    leaves = [t.to(DEV).requires_grad_() for t in (pa, pk, v)]
    y = ops.fused_attention(leaves[0], leaves[1], leaves[2], mask.to(DEV), diag=diag.to(DEV), relu=True)
    y.backward(gy.to(DEV))
    return y.detach(), [t.grad for t in leaves]


@pytest.mark.parametrize("live", [(1, 90), (6, 80)])
def test_es_tail_attention_vs_float64(live):
    """ruart_attn_fwd / _bwd at the shape post_process's ES_ocr_att would call them with (B = 2, L1 = 10, L2 = 90, h = 125, D3 = 500, scalar diagonal, ReLU)
    against float64 autograd, at test_fused_attention_shapes' bounds: output 2e-5, gradients 5e-5 of max(1, |ref|).  Live keys per
    sample {1, 90} (one live key: the softmax is a one-hot, its gradient to the projections is 0) and {6, 80}.
    Measured: {1, 90} out 3.6e-08, gradients 2.8e-07 / 2.7e-07 / 9.1e-08; {6, 80} out 2.2e-07, gradients 3.7e-07 / 3.8e-07 / 2.0e-07
    (pa / pk / v)."""
    from ruart_amd import ops
    case = _attn_case(live, 900 + sum(live))
    ref, gref = _attn_float64(*case)
    y, grads = _attn_device(*case)
    ops.nan_flag.check_and_clear()
    e_y = maxerr(y, ref) / max(1.0, float(ref.abs().max()))
    e_g = [maxerr(a, b) / max(1.0, float(b.abs().max())) for a, b in zip(grads, gref)]
    print("ES tail attention, live keys %s: out %.2e, gradients pa %.2e pk %.2e v %.2e" % (live, e_y, *e_g))
    assert e_y < 2e-5
    assert max(e_g) < 5e-5, e_g
    if live[0] == 1:              # masked keys receive exactly nothing
        assert float(grads[1][0, 1:].abs().max()) == 0.0 and float(grads[2][0, 1:].abs().max()) == 0.0


def test_es_tail_attention_wholly_masked_panel_raises_the_nan_flag():
    """Live keys {90, 0}: the second sample's softmax runs over an empty set.  The reference's ``assert isnan == 0`` fires there
    (Models/Layers.py:290); here the kernel raises the device flag, ``check_and_clear`` turns it into the AssertionError, the first
    sample is computed as usual (float64 bounds as above), backward runs, and the device is healthy afterwards."""
    from ruart_amd import ops
    case = _attn_case((90, 0), 990)
    pa, pk, v, gy, mask, diag = case
    y, grads = _attn_device(*case)
    with pytest.raises(AssertionError):
        ops.nan_flag.check_and_clear()
    ops.nan_flag.check_and_clear()                      # cleared by the check
    torch.cuda.synchronize()
    assert bool(torch.isnan(y[1]).all()) and bool(torch.isfinite(y[0]).all())
    ref, gref = _attn_float64(pa[:1], pk[:1], v[:1], gy[:1], mask[:1], diag)
    assert maxerr(y[:1], ref) < 2e-5 * max(1.0, float(ref.abs().max()))
    for a, b in zip(grads, gref):
        assert maxerr(a[:1], b) < 5e-5 * max(1.0, float(b.abs().max()))


# ---- end to end ---------------------------------------------------------------------------------------------------------------------
NAME, KEYS = "sdnet_e2e_noctx", dict(no_Context_Self_Attention=True)


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, NAME + ".npz"))


@pytest.fixture(scope="module")
def bert_weights():
    cfg = synth.bert_config(vocab_size=2000)
    return cfg, synth.make_bert_weights(cfg, seed=1033)


def _opt_and_weights(z, bert_weights, **extra):
    opt = default_opt(vocab_size=int(z["vocab_size"]), cuda=True, **KEYS, **extra)
    opt["bert_config"], opt["bert_state"] = bert_weights
    return opt, synth.make_sdnet_weights(opt, seed=int(z["seed"]))


def _net(z, bert_weights, **extra):
    import ruart_amd.layers as L
    from ruart_amd.sdnet import SDNet
    opt, sw = _opt_and_weights(z, bert_weights, device=DEV, **extra)
    net = SDNet(opt, {"glove_embedding": T(sw["glove_embed.weight"]), "fast_embedding": T(sw["fast_embed.weight"])})
    missing, unexpected = net.load_state_dict({k: T(v) for k, v in sw.items()}, strict=False)
    assert not missing and not unexpected, (missing, unexpected)      # state-dict keys == the reference's
    net = net.to(DEV)
    L.set_dropout_prob(0.0)
    net.train()
    net.drop_emb = False
    return net, opt


def _batch(opt, z):
    q, ocr, od, gt, _ = synth.synthetic_batch(opt, int(z["B"]), seed=int(z["batch_seed"]), n_q=30, n_ocr=100, n_od=30, bert_vocab=2000,
                                              ragged=True)
    assert ocr["num_cnt"] == z["ocr_num_cnt"].tolist() and np.array_equal(gt.numpy(), z["gt"])
    return q, ocr, od, gt


def _loss_backward(net, scores, gt):
    net.zero_grad(set_to_none=True)
    gt = gt.to(scores.device)
    loss = torch.nn.functional.binary_cross_entropy_with_logits(scores, gt) * gt.size(1)
    loss.backward()
    return loss


def _gradient_errors(net, z):
    """worst relative gradient-norm error and worst element error / max |g| against the fixture; no gradient exactly where it has none"""
    params = dict(net.named_parameters())
    assert sorted(params) == sorted(z["grad_names"].tolist())
    worst_norm, worst_elem = (0.0, ""), (0.0, "")
    for name, ref_norm in zip(z["grad_names"].tolist(), z["grad_norms"].tolist()):
        gr = params[name].grad
        if ref_norm < 0:
            assert gr is None, name
            continue
        if gr is None:             # (a bias under a softmax: shift invariant, the fused kernel does not materialise its rounding-noise gradient)
            assert name == "ques_merger.linear.bias" and ref_norm < 1e-6, (name, ref_norm)
            continue
        worst_norm = max(worst_norm, (abs(float(gr.double().norm()) - ref_norm) / max(ref_norm, 1e-4), name))
        if "grad:" + name in z.files:
            ref = z["grad:" + name]
            worst_elem = max(worst_elem, (float(np.abs(gr.detach().cpu().numpy() - ref).max() / max(np.abs(ref).max(), 1e-5)), name))
    return worst_norm, worst_elem


@pytest.mark.parametrize("precision", ["fp32", "x3", "fp16c"])
def test_sdnet_noctx_forward_backward_vs_reference(golden, bert_weights, precision):
    """SDNet with no_Context_Self_Attention against the unmodified reference's scores (B, 101), loss and gradients on the same seeded
    inputs, at the bounds test_sdnet_yesno_forward_backward_vs_reference holds these precision modes to (scores 5e-5 / 2e-4 / 2e-4,
    gradient norms 2e-3 / 1e-2 / 1e-2, small gradients' elements twice that).  The fixture's gradients are of ordinary size (86 of its 87
    gradient norms at or above the 1e-4 floor).
    Measured max |dp| / worst gradient-norm error / worst element error: fp32 4.7e-06 / 5.8e-05 / 5.8e-05, x3 6.8e-06 / 1.3e-04 /
    3.7e-04, fp16c 7.6e-05 / 8.3e-04 / 8.3e-04."""
    z = golden
    tol_p, tol_g = BOUNDS[precision]
    net, opt = _net(z, bert_weights, bert_precision=precision)
    assert not hasattr(net, "highlvl_self_att")
    q, ocr, od, gt = _batch(opt, z)
    scores, _ = net(q, ocr, od)
    net.check_nan()
    got = scores.detach().cpu().numpy()
    err = np.abs(got - z["scores"]).max()
    assert got.shape == z["scores"].shape == (int(z["B"]), opt["max_ocr_num"] + 1) and np.allclose(got.sum(1), 1.0, atol=1e-5)
    loss = _loss_backward(net, scores, gt)
    worst_norm, worst_elem = _gradient_errors(net, z)
    print("%s, precision %s: max |dp| %.2e; worst grad-norm rel err %.2e (%s); worst grad element err / max|g| %.2e (%s)"
          % (NAME, precision, err, worst_norm[0], worst_norm[1], worst_elem[0], worst_elem[1]))
    assert err < tol_p, "max |p - p_ref| = %.3e" % err
    assert abs(loss.item() - float(z["loss"])) < 10 * tol_p
    assert worst_norm[0] < tol_g, worst_norm
    assert worst_elem[0] < 2 * tol_g, worst_elem


def _scores_and_gradients(net, q, ocr, od, gt, z):
    scores, _ = net(q, ocr, od)
    net.check_nan()
    _loss_backward(net, scores, gt)
    return scores.detach().clone(), _gradient_errors(net, z)


def test_noctx_three_stream_schedule_is_bit_equal_to_one_stream(golden, bert_weights):
    """opt['ruart_streams'] on (the three branches overlapped) and off: the same kernels on the same operands, so forward scores are
    bit-equal; the gradients of both stay within the fixture's bound (x3: 1e-2)."""
    z = golden
    net, opt = _net(z, bert_weights, bert_precision="x3")
    q, ocr, od, gt = _batch(opt, z)
    assert net._use_streams()
    s_on, (norm_on, elem_on) = _scores_and_gradients(net, q, ocr, od, gt, z)
    net.opt["ruart_streams"] = False
    assert not net._use_streams()
    s_off, (norm_off, elem_off) = _scores_and_gradients(net, q, ocr, od, gt, z)
    assert torch.equal(s_on, s_off)
    tol_g = BOUNDS["x3"][1]
    print("%s streams on / off: worst grad-norm rel err %.2e / %.2e" % (NAME, norm_on[0], norm_off[0]))
    assert max(norm_on[0], norm_off[0]) < tol_g and max(elem_on[0], elem_off[0]) < 2 * tol_g


def test_trainer_noctx_update_predict_and_checkpoint(golden, bert_weights, tmp_path):
    """Three SDNetTrainer.update() steps on the no_Context_Self_Attention conf: finite losses; the narrower high-level RNN's input
    weights move; predict() decodes No + 1 columns; the checkpoint holds no highlvl_self_att key; save_for_predict -> load_model into a
    fresh trainer gives bit-equal scores."""
    from ruart_amd.trainer import SDNetTrainer
    z = golden
    opt, sw = _opt_and_weights(z, bert_weights, DROPOUT=0.0, dropout_emb=0.0)
    emb = {"glove_embedding": T(sw["glove_embed.weight"]), "fast_embedding": T(sw["fast_embed.weight"])}
    tr = SDNetTrainer(opt, device=DEV)
    tr.setup_model(emb)
    B = int(z["B"])
    make = lambda: synth.synthetic_batch(opt, B, seed=int(z["batch_seed"]), n_q=30, n_ocr=100, n_od=30, bert_vocab=2000, ragged=True)
    batch = tr.ToCUDA(make())
    w = tr.network.high_lvl_context_rnn.rnns[0].weight_ih_l0
    assert tuple(w.shape) == (500, 250)
    before = w.detach().clone()
    losses = [float(tr.update(batch, i)) for i in range(3)]
    assert all(np.isfinite(l) for l in losses), losses
    assert not torch.equal(w.detach(), before)
    width = opt["max_ocr_num"] + 1
    loss, anls, acc, res, save_res = tr.predict(batch)
    assert len(res) == B and all(r["ids_len"] == width and 0 <= r["idx"] < width for r in save_res)
    path = str(tmp_path / "ruart_noctx_ckpt.pt")
    tr.save_for_predict(path)
    ck = torch.load(path, map_location="cpu")["state_dict"]["network"]
    assert "high_lvl_context_rnn.rnns.0.weight_ih_l0" in ck and not any(k.startswith("highlvl_self_att") for k in ck)

    def eval_scores(t):
        t.network.eval()
        with torch.no_grad():
            s, _ = t.network(*t.ToCUDA(make())[:3])
        t.network.check_nan()
        return s.clone()

    want = eval_scores(tr)
    tr2 = SDNetTrainer(opt, device=DEV)
    tr2.setup_model(emb)
    assert not torch.equal(eval_scores(tr2), want)
    tr2.load_model(path)
    assert torch.equal(eval_scores(tr2), want)
    tr.close()
    tr2.close()
