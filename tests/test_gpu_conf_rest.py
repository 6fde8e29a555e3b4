"""``multi2one_bidir`` (with ``no_DeepAttention``), ``no_DeepAttention`` and last-layer BERT (a conf without ``BERT_LINEAR_COMBINE``) on
the MI355X: SDNet end to end against the unmodified reference (tests/golden/sdnet_e2e_{bidir_nodeep, nodeep, lastlayer,
bidir_nodeep_lastlayer}.npz, written by tools/gen_golden_conf_rest.py); the reverse direction of multi2one - its shared-chain shortcut
against the per-item run, and one dropout-on forward + backward against a dense, padded float64 LSTM under the SAME masks -; the
last-layer pooling against the twelve-layer pooling with a one-hot mix; the trained encoder; the three-stream schedule and SDNetTrainer."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from ruart_amd import synth                               # noqa: E402
from tests._conf_rest import CONFS, T, batch, conf_opt      # noqa: E402

DEV = "cuda:0"
# the project's standing end-to-end bounds (tests/test_gpu_es_post.py): scores / gradient norms per precision
BOUNDS = {"fp32": (5e-5, 2e-3), "x3": (2e-4, 1e-2), "fp16c": (2e-4, 1e-2)}
# tests/test_gpu_bert_train_dropout.py's bounds of a dropout-on pass against its same-mask float64 reference: forward max |err|,
# rel-L2 per gradient tensor
FWD_BOUND, GRAD_BOUND = 4e-3, 3e-2


@pytest.fixture(scope="module")
def goldens(golden_dir):
    return {name: np.load(os.path.join(golden_dir, name + ".npz")) for name in CONFS}


@pytest.fixture(scope="module")
def bert_weights():
    cfg = synth.bert_config(vocab_size=2000)
    return cfg, synth.make_bert_weights(cfg, seed=1033)


def _opt_and_weights(name, bert_weights, **extra):
    opt = conf_opt(name, cuda=True, **extra)
    opt["bert_config"], opt["bert_state"] = bert_weights
    return opt, synth.make_sdnet_weights(opt, seed=1033)


def _net(name, bert_weights, **extra):
    import ruart_amd.layers as L
    from ruart_amd.sdnet import SDNet
    opt, sw = _opt_and_weights(name, bert_weights, device=DEV, **extra)
    net = SDNet(opt, {"glove_embedding": T(sw["glove_embed.weight"]), "fast_embedding": T(sw["fast_embed.weight"])})
    missing, unexpected = net.load_state_dict({k: T(v) for k, v in sw.items()}, strict=False)
    if "LOCK_BERT" in opt:
        assert not missing and not unexpected, (missing, unexpected)      # state-dict keys == the reference's
    else:
        assert not unexpected and all(k.startswith("Bert.bert_model.") for k in missing)
    net = net.to(DEV)
    L.set_dropout_prob(0.0)
    net.train()
    net.drop_emb = False
    return net, opt


def _loss_backward(net, scores, gt):
    net.zero_grad(set_to_none=True)
    gt = gt.to(scores.device)
    loss = torch.nn.functional.binary_cross_entropy_with_logits(scores, gt) * gt.size(1)
    loss.backward()
    return loss


def _gradient_errors(net, z):
    """worst relative gradient-norm error and worst element error / max |g| against the fixture (small tensors whole, rows 0 and 1 of the
    word / POS / entity tables); no gradient exactly where the reference has none"""
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
        for key, got in (("grad:" + name, gr), ("grad_rows01:" + name, gr[:2])):
            if key in z.files:
                ref = z[key]
                worst_elem = max(worst_elem, (float(np.abs(got.detach().cpu().numpy() - ref).max() / max(np.abs(ref).max(), 1e-5)), key))
    return worst_norm, worst_elem


# ---- end to end against the reference ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp32", "x3", "fp16c"])
@pytest.mark.parametrize("name", list(CONFS))
def test_sdnet_forward_backward_vs_reference(goldens, bert_weights, name, precision):
    """Each conf against the unmodified reference's scores (B, 101), loss and gradients on the same seeded inputs, at the standing
    end-to-end bounds of these precision modes (scores 5e-5 / 2e-4 / 2e-4, gradient norms 2e-3 / 1e-2 / 1e-2, the small gradients'
    elements twice that) - every recorded norm, every gradient of up to 4096 elements, and rows 0 and 1 of the word, POS and entity
    tables' gradients: row 0 is the pad id, which only the reverse direction of a bidirectional multi2one feeds (the fixture's row 0 of
    fast_embed: norm 0.088 with multi2one_bidir, exactly 0 without).
    Measured max |dp| / worst gradient-norm error / worst element error, fp32 | x3 | fp16c:
      bidir_nodeep            2.2e-06 / 5.3e-05 / 9.1e-05 | 1.1e-05 / 3.0e-04 / 3.0e-04 | 1.5e-04 / 4.4e-03 / 9.0e-03
      nodeep                  8.5e-06 / 9.0e-05 / 9.0e-05 | 3.6e-05 / 2.2e-04 / 2.2e-04 | 1.5e-04 / 1.4e-03 / 1.8e-03
      lastlayer               6.7e-06 / 1.4e-05 / 4.0e-05 | 7.5e-05 / 5.7e-04 / 1.4e-03 | 1.0e-04 / 6.5e-04 / 4.1e-03
      bidir_nodeep_lastlayer  2.6e-06 / 6.1e-05 / 2.2e-04 | 3.8e-05 / 9.2e-04 / 3.9e-03 | 3.7e-05 / 6.7e-04 / 1.8e-03"""
    z = goldens[name]
    tol_p, tol_g = BOUNDS[precision]
    net, opt = _net(name, bert_weights, bert_precision=precision)
    set_keys, drop_keys = CONFS[name]
    assert net.bert_last_only == ("BERT_LINEAR_COMBINE" in drop_keys) and hasattr(net, "alphaBERT") == (not net.bert_last_only)
    assert net.m2o_bidir == ("multi2one_bidir" in set_keys)
    q, ocr, od, gt, _ = batch(opt, z)
    scores, _ = net(q, ocr, od)
    net.check_nan()
    got = scores.detach().cpu().numpy()
    err = np.abs(got - z["scores"]).max()
    assert got.shape == z["scores"].shape == (2, opt["max_ocr_num"] + 1) and np.allclose(got.sum(1), 1.0, atol=1e-5)
    loss = _loss_backward(net, scores, gt)
    worst_norm, worst_elem = _gradient_errors(net, z)
    print("%s, precision %s: max |dp| %.2e; worst grad-norm rel err %.2e (%s); worst grad element err / max|g| %.2e (%s)"
          % (name, precision, err, worst_norm[0], worst_norm[1], worst_elem[0], worst_elem[1]))
    if net.m2o_bidir:
        assert "grad_rows01:fast_embed.weight" in z.files and float(np.abs(z["grad_rows01:fast_embed.weight"][0]).max()) > 0
        assert float(net.fast_embed.weight.grad[0].abs().max()) > 0
    assert err < tol_p, "max |p - p_ref| = %.3e" % err
    assert abs(loss.item() - float(z["loss"])) < 10 * tol_p
    assert worst_norm[0] < tol_g, worst_norm
    assert worst_elem[0] < 2 * tol_g, worst_elem


def _scores_and_gradients(net, q, ocr, od, gt, z):
    scores, _ = net(q, ocr, od)
    net.check_nan()
    _loss_backward(net, scores, gt)
    return scores.detach().clone(), _gradient_errors(net, z)


@pytest.mark.parametrize("name", ["sdnet_e2e_bidir_nodeep_lastlayer", "sdnet_e2e_nodeep"])
def test_three_stream_schedule_is_bit_equal_to_one_stream(goldens, bert_weights, name):
    """opt['ruart_streams'] on (the three branches overlapped) and off: the same kernels on the same operands, so forward scores are
    bit-equal; the gradients of both stay within the fixture's bound (x3: 1e-2)."""
    z = goldens[name]
    net, opt = _net(name, bert_weights, bert_precision="x3")
    q, ocr, od, gt, _ = batch(opt, z)
    assert net._use_streams()
    s_on, (norm_on, elem_on) = _scores_and_gradients(net, q, ocr, od, gt, z)
    net.opt["ruart_streams"] = False
    assert not net._use_streams()
    s_off, (norm_off, elem_off) = _scores_and_gradients(net, q, ocr, od, gt, z)
    assert torch.equal(s_on, s_off)
    tol_g = BOUNDS["x3"][1]
    print("%s streams on / off: worst grad-norm rel err %.2e / %.2e" % (name, norm_on[0], norm_off[0]))
    assert max(norm_on[0], norm_off[0]) < tol_g and max(elem_on[0], elem_off[0]) < 2 * tol_g


# ---- the reverse direction of multi2one ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def bidir_net(bert_weights):
    """one bidirectional model (split-bf16 trunk) for the two tests below; they leave its parameters unchanged"""
    return _net("sdnet_e2e_bidir_nodeep", bert_weights, bert_precision="x3")


def _front_inputs(net, opt, seed):
    """the fixtures' OCR group with seeded stand-ins for the two inputs of the item front that other modules produce: the pooled encoder
    features (W, 768) and the pre-align block (W, 300)"""
    q, ocr, od, _, _ = batch(opt)
    bi = net.prepare(q, ocr, od)
    g = torch.Generator().manual_seed(seed)
    W = bi.ocr.W
    return ocr, bi.ocr, torch.randn(W, 768, generator=g), torch.randn(W, 300, generator=g) * 0.5, torch.randn(bi.ocr.N, 600, generator=g)


def test_bidir_shared_chain_equals_the_per_item_run(bidir_net):
    """Dropout off: every item has the same pad input, so ``_multi2one_reverse`` steps ONE row 19 times and lets each item pick the
    state after its pad count; ``per_item=True`` steps all items through the pad-run schedule instead.  Both run the same cell kernel
    and the same split-bf16 recurrent product per step, on the same operand rows; the product's result for a row may differ in the
    summation order of its K = 300 terms when the row count changes the launch plan (M = 1 against M = up to 148 rows).  Bound: per
    step one fp32 reordering of 300 terms of |h w| <= 1 / sqrt(300) each, 300 * 2^-24 / sqrt(300) = 1e-6 on a pre-activation, through
    at most 20 steps of a cell whose gates have slope <= 1: 2e-5 on the states (|h| < 1), and 1e-4 of each gradient's max.
    Measured: states bit-equal, gradients within 6.9e-06 of their max (the sums over the items run in another order)."""
    from ruart_amd import ops
    net, opt = bidir_net
    ocr, idx, mix, pre, g_out = _front_inputs(net, opt, 3)
    rnn = net.multi2one.rnns[0]
    params = [rnn.weight_ih_l0_reverse, rnn.weight_hh_l0_reverse, rnn.bias_ih_l0_reverse, net.pos_embedding.weight, net.ent_embedding.weight]
    outs = []
    with ops.use_trunk_mode(gemm="x3", grad_gemm="x3", defer_dw=False):
        for per_item in (False, True):
            net.zero_grad(set_to_none=True)
            words, raw, pad = net._embed_items(ocr, idx, mix.to(DEV))
            assert [c for c, _ in pad] == [0, 1068, 1080] and all(b.size(0) == 1 for _, b in pad)      # fasttext, POS, entity blocks
            x = torch.cat([words, pre.to(DEV)], 1)
            h = net._multi2one_reverse(x, idx, pad, None, per_item=per_item)
            (h * g_out[:, :300].to(DEV)).sum().backward()
            outs.append((h.detach().clone(), [p.grad.detach().clone() for p in params]))
    net.check_nan()
    (h_s, g_s), (h_p, g_p) = outs
    e_h = float((h_s - h_p).abs().max())
    e_g = [float((a - b).abs().max() / b.abs().max()) for a, b in zip(g_s, g_p)]
    print("reverse run, shared chain against per item: states %.2e, gradients %s" % (e_h, ["%.1e" % e for e in e_g]))
    assert float(h_p.abs().max()) > 0.05 and e_h <= 2e-5
    assert max(e_g) <= 1e-4, e_g
    # items without a pad step start from the zero state: their reverse state is one step on their last word
    full = idx.dev["rev_pad"] == 0
    assert int(full.sum()) == 3


class _RecordingBank:
    """layers.MaskBank that keeps what it hands out"""

    def __init__(self):
        import ruart_amd.layers as L
        self.bank, self.taken = L.MaskBank(), []

    def begin_step(self, device):
        self.bank.begin_step(device)

    def take(self, rows, cols, p, like):
        m = self.bank.take(rows, cols, p, like)
        self.taken.append((p, m.detach().clone()))
        return m


def _dense_reference(net, ocr, idx, mix, pre, masks, g_out, shift_pad_masks=False):
    """multi2one as the reference runs it, in float64 on the CPU: the padded (N, Lw, D) input - pad positions hold row 0 of the word /
    POS / entity tables and zeros in the BERT and pre-align blocks -, ``dropout_emb``'s per-item masks on the word and BERT blocks, the
    LSTM's variational input mask over all Lw positions, torch's bidirectional nn.LSTM, the output at each item's last real word.
    ``shift_pad_masks``: a deliberately WRONG reference whose pad positions take the NEXT item's masks."""
    m_fast, m_bert, m_in = [m.double().cpu() for m in masks]
    N, Lw = ocr["fasttext"].shape
    lens = torch.tensor([l for s_ in ocr["len_cnt"] for l in s_])
    leaves = {"fast": net.fast_embed.weight, "pos": net.pos_embedding.weight, "ent": net.ent_embedding.weight}
    leaves = {k: v.detach().double().cpu().requires_grad_() for k, v in leaves.items()}
    leaves["mix"], leaves["pre"] = mix.double().requires_grad_(), pre.double().requires_grad_()
    real = (torch.arange(Lw)[None, :] < lens[:, None])
    flat = real.reshape(-1).nonzero().squeeze(1)

    def dense(packed):
        return torch.zeros(N * Lw, packed.size(1), dtype=torch.float64).index_copy(0, flat, packed).view(N, Lw, -1)

    def item_mask(m):
        if not shift_pad_masks:
            return m[:, None, :].expand(N, Lw, -1)
        return torch.where(real[:, :, None], m[:, None, :], torch.roll(m, -1, 0)[:, None, :])

    x = torch.cat([leaves["fast"][ocr["fasttext"]] * item_mask(m_fast), dense(leaves["mix"]) * item_mask(m_bert),
                   leaves["pos"][ocr["pos"]], leaves["ent"][ocr["ent"]], dense(leaves["pre"])], 2)
    lstm = torch.nn.LSTM(x.size(2), 300, num_layers=1, bidirectional=True, batch_first=True).double()
    lstm.load_state_dict({k: v.detach().double().cpu() for k, v in net.multi2one.rnns[0].state_dict().items()})
    out = lstm(x * item_mask(m_in))[0][torch.arange(N), lens - 1]
    (out * g_out.double()).sum().backward()
    grads = {k: v.grad for k, v in leaves.items()}
    grads.update({"lstm." + k: v.grad for k, v in lstm.named_parameters()})
    return out.detach(), grads


def test_bidir_dropout_on_vs_dense_float64_under_the_same_masks(bidir_net):
    """One training forward + backward of the item front (embedding blocks, ``dropout_emb`` 0.4, multi2one under DROPOUT 0.3, both
    variational) against the dense float64 restatement fed the masks the bank handed out: the state at every item's last real word,
    both directions, and the gradients of the eight LSTM tensors, of the three tables (row 0, the pad id, included), of the pooled
    encoder features and of the pre-align block.  Bounds of tests/test_gpu_bert_train_dropout.py: forward 4e-3, gradients 3e-2 rel-L2
    per tensor (the split-bf16 trunk is far inside: measured forward 2.5e-05, worst gradient 1.1e-05, row 0 of the three tables 7e-06 to 8e-06).  Row 0 of the word table, zero in the synthetic weights, is given
    values for this test, so that the pad input's word block is under ``dropout_emb``'s mask for real.  The same reference with the pad
    positions under the NEXT item's masks differs from the right one by more than 10 times the forward bound (float64 against float64:
    1.4): a pad input under the wrong item's mask cannot pass."""
    import ruart_amd.layers as L
    from ruart_amd import ops
    net, opt = bidir_net
    ocr, idx, mix, pre, g_out = _front_inputs(net, opt, 4)
    rec = _RecordingBank()
    saved_bank, L.mask_bank = L.mask_bank, rec
    mix_d, pre_d = mix.to(DEV).requires_grad_(), pre.to(DEV).requires_grad_()
    row0_saved = net.fast_embed.weight.data[0].clone()
    try:
        net.fast_embed.weight.data[0] = (torch.randn(300, generator=torch.Generator().manual_seed(1)) * 0.5).to(DEV)
        L.set_dropout_prob(0.3)
        net.drop_emb = True
        net.zero_grad(set_to_none=True)
        with ops.use_trunk_mode(gemm="x3", grad_gemm="x3", defer_dw=False):
            rec.begin_step(torch.device(DEV))
            words, raw, pad = net._embed_items(ocr, idx, mix_d)
            assert all(b.size(0) == (idx.N if c == 0 else 1) for c, b in pad)       # the word block under its per-item mask
            out = net._multi2one_last(torch.cat([words, pre_d], 1), idx, None, pad)
            # item order: sample b, slot k
            rows = torch.cat([b * idx.max_num + torch.arange(n) for b, n in enumerate(ocr["num_cnt"])]).to(DEV)
            got = out.reshape(-1, 600).index_select(0, rows)
            (got * g_out.to(DEV)).sum().backward()
        net.check_nan()
        ref, gref = _dense_reference(net, ocr, idx, mix, pre, [m for _, m in rec.taken], g_out)
        wrong, _ = _dense_reference(net, ocr, idx, mix, pre, [m for _, m in rec.taken], g_out, shift_pad_masks=True)
    finally:
        L.mask_bank = saved_bank
        L.set_dropout_prob(0.0)
        net.drop_emb = False
        net.fast_embed.weight.data[0] = row0_saved
    assert [(p, tuple(m.shape)) for p, m in rec.taken] == [(0.4, (idx.N, 300)), (0.4, (idx.N, 768)), (0.3, (idx.N, 1388))]
    masks = [m for _, m in rec.taken]
    assert all(0.2 < float((m == 0).double().mean()) < 0.5 for m in masks)
    e_f = float((got.detach().double().cpu() - ref).abs().max())
    rnn = net.multi2one.rnns[0]
    have = {"fast": net.fast_embed.weight.grad, "pos": net.pos_embedding.weight.grad, "ent": net.ent_embedding.weight.grad,
            "mix": mix_d.grad, "pre": pre_d.grad}
    have.update({"lstm." + k: v.grad for k, v in rnn.named_parameters()})
    assert sorted(have) == sorted(gref) and len(have) == 13
    errs = {k: float((have[k].double().cpu() - gref[k]).norm() / gref[k].norm()) for k in gref}
    row0 = {k: float((have[k][0].double().cpu() - gref[k][0]).norm() / gref[k][0].norm()) for k in ("fast", "pos", "ent")}
    e_wrong = float((ref - wrong).abs().max())
    print("bidirectional multi2one, dropout on: forward max err %.2e; worst gradient rel-L2 %.2e (%s); row 0 of the tables %s; the wrong-item-mask "
          "reference differs by %.2e" % (e_f, max(errs.values()), max(errs, key=errs.get), {k: "%.1e" % v for k, v in row0.items()}, e_wrong))
    assert e_f < FWD_BOUND
    assert max(errs.values()) <= GRAD_BOUND, errs
    assert max(row0.values()) <= GRAD_BOUND, row0
    assert e_wrong > 10 * FWD_BOUND


# ---- last-layer BERT --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("last_rows", [True, False])
@pytest.mark.parametrize("precision", ["fp16c", "fp32"])
def test_last_layer_pooling_equals_the_one_hot_mix(bert_weights, precision, last_rows):
    """``bert.pool_last`` (the pooling entry points with n_layers = 1 on the last layer's matrix; fp16c: the LayerNorm-folded pass,
    ruart_bert_pool_mix_ln with that layer's statistics and gamma / beta) against ``_PoolMix`` over all twelve layers with the one-hot
    weight vector, on the three groups of the fixtures' batch, with the compacted last layer (``bert_last_rows``) and without.
    Both form, per element, the mean of the word's n <= 2 piece values in fp32 (the folded pass: of (y - mu) rstd, then one multiply by
    gamma / n and one add of beta); the twelve-layer kernels add eleven exact zeros and may associate the products differently, so the
    results agree to a few roundings of the largest intermediate: bound (n_max + 4) * 2^-23 * max |layer output| with n_max the
    longest span.  Measured: bit-equal in all four cases, at a bound of 2.9e-06 (n_max 2, max |layer output| 4.0)."""
    from ruart_amd import hip
    from ruart_amd.batch import BatchIndex
    from ruart_amd.bert import Bert, _PoolMix, layer_outputs, pool_last
    opt, _ = _opt_and_weights("sdnet_e2e_lastlayer", bert_weights, device=DEV, bert_precision=precision, bert_last_rows=last_rows)
    bert = Bert(opt, device=DEV)
    bert.lock()
    assert bool(getattr(bert.weights, "ln_fold", False)) == (precision == "fp16c")
    q, ocr, od, _, _ = batch(opt)
    bi = BatchIndex(q, ocr, od, opt, DEV, bert=bert)
    assert (bi._n_last > 0) == last_rows
    layers = bert.layers_for(bi.packed)
    ln = getattr(layers, "_ln", None) or (None, None, None)
    assert (ln[0] is not None) == (precision == "fp16c")
    NL = layers.shape[0]
    onehot = torch.zeros(NL, device=DEV)
    onehot[NL - 1] = 1.0
    scale = float(layer_outputs(layers)[NL - 1, :(bi._n_last or bi.packed.T)].abs().max())
    worst, n_max = 0.0, 0
    for g in range(3):
        s_, l_, dst, rows, s_last = bi.spans[g]
        assert (s_last is not None) == last_rows
        got = pool_last(layers, s_, l_, dst, rows, s_last)
        want = _PoolMix.apply(onehot, layers, s_, l_, dst, rows, hip.dtype_code(layers), s_last, *ln)
        assert got.shape == want.shape == (rows, 768) and float(want.abs().max()) > 0.5
        worst = max(worst, float((got - want).abs().max()))
        n_max = max(n_max, int(l_.max()))
    bound = (n_max + 4) * 2.0 ** -23 * scale
    print("last-layer pooling against the one-hot mix, %s, last rows %s: max |diff| %.2e, bound %.2e (n_max %d, max |layer| %.1f)"
          % (precision, last_rows, worst, bound, n_max, scale))
    assert worst <= bound


@pytest.mark.parametrize("mode", ["16", "16-dropout", "x3"])
def test_last_layer_with_the_encoder_trained(bert_weights, mode):
    """A conf without BERT_LINEAR_COMBINE and without LOCK_BERT on a small batch: the gradient enters the encoder through the last layer
    alone and reaches layer 0 - both carry non-zero, finite gradients -, there are no mix parameters, and the scores are a distribution.
    '16': the 16-bit encoder, dropout off (the fp16c forward, its last layer's fp32 rows the output); '16-dropout': BERT's own dropouts
    on (the f16 training kernels, ruart_mix_rows over the one layer); 'x3': the fp32-class graph.  With ``bert_train_layers`` = 2 the ten
    lower layers stay without a gradient."""
    cfg, state = bert_weights
    if mode != "16-dropout":
        cfg = dict(cfg, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    extra = dict(bert_train_gemm="x3") if mode == "x3" else dict(bert_train_gemm="16", bert_train_layers=2 if mode == "16" else 12)
    opt = conf_opt("sdnet_e2e_lastlayer", cuda=True, device=DEV, **extra)
    del opt["LOCK_BERT"]
    if opt.get("bert_train_layers") == 12:
        del opt["bert_train_layers"]
    opt["bert_config"], opt["bert_state"] = cfg, state
    from ruart_amd.sdnet import SDNet
    import ruart_amd.layers as L
    sw = synth.make_sdnet_weights(opt, seed=1033)
    net = SDNet(opt, {"glove_embedding": T(sw["glove_embed.weight"]), "fast_embedding": T(sw["fast_embed.weight"])})
    missing, unexpected = net.load_state_dict({k: T(v) for k, v in sw.items()}, strict=False)
    assert not unexpected and all(k.startswith("Bert.bert_model.") for k in missing) and not hasattr(net, "alphaBERT")
    net = net.to(DEV)
    L.set_dropout_prob(0.0)
    net.train()
    net.drop_emb = False
    q, ocr, od, gt, _ = synth.synthetic_batch(opt, 2, seed=7, n_q=12, n_ocr=16, n_od=6, bert_vocab=2000, ragged=True)
    scores, _ = net(q, ocr, od)
    _loss_backward(net, scores, gt)
    net.check_nan()
    assert np.allclose(scores.detach().cpu().numpy().sum(1), 1.0, atol=1e-5)
    grads = {n: p.grad for n, p in net.named_parameters() if p.grad is not None}
    top = "Bert.bert_model.encoder.layer.11.output.dense.weight"
    low = "Bert.bert_model.encoder.layer.%d.attention.self.query.weight" % (10 if mode == "16" else 0)
    for n in (top, low):
        assert n in grads and bool(torch.isfinite(grads[n]).all()) and float(grads[n].abs().max()) > 0, n
    if mode == "16":
        assert not any(n.startswith("Bert.bert_model.encoder.layer.%d." % l) for n in grads for l in range(10))
    assert float(grads["Bert.bert_model.encoder.layer.11.output.LayerNorm.gamma"].abs().max()) > 0


# ---- trainer ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CONFS))
def test_trainer_update_predict_and_checkpoint(goldens, bert_weights, tmp_path, name):
    """Two SDNetTrainer.update() steps per conf, dropout on as the conf says (DROPOUT 0.3, dropout_emb 0.4: the pad inputs of the reverse
    direction run under per-item masks): finite losses, multi2one's (reverse) input weights move; predict() decodes No + 1 columns; the
    checkpoint holds the conf's keys; save_for_predict -> load_model into a fresh trainer gives bit-equal scores."""
    from ruart_amd.trainer import SDNetTrainer
    set_keys, drop_keys = CONFS[name]
    bidir = "multi2one_bidir" in set_keys
    opt, sw = _opt_and_weights(name, bert_weights)
    emb = {"glove_embedding": T(sw["glove_embed.weight"]), "fast_embedding": T(sw["fast_embed.weight"])}
    tr = SDNetTrainer(opt, device=DEV)
    tr.setup_model(emb)
    make = lambda: batch(opt)
    b = tr.ToCUDA(make())
    rnn = tr.network.multi2one.rnns[0]
    w = rnn.weight_ih_l0_reverse if bidir else rnn.weight_ih_l0
    assert tr.network.context_rnn.rnns[0].weight_ih_l0.shape[1] == (600 if bidir else 300)
    before = w.detach().clone()
    losses = [float(tr.update(b, i)) for i in range(2)]
    assert all(np.isfinite(l) for l in losses), losses
    assert not torch.equal(w.detach(), before)
    width = opt["max_ocr_num"] + 1
    loss, anls, acc, res, save_res = tr.predict(b)
    assert len(res) == 2 and all(r["ids_len"] == width and 0 <= r["idx"] < width for r in save_res)
    path = str(tmp_path / "ruart_conf_rest_ckpt.pt")
    tr.save_for_predict(path)
    ck = torch.load(path, map_location="cpu")["state_dict"]["network"]
    assert ("multi2one.rnns.0.weight_hh_l0_reverse" in ck) == bidir
    assert ("alphaBERT" in ck) == ("BERT_LINEAR_COMBINE" not in drop_keys)
    assert any(k.startswith("deep_attn.int_attn_list.") for k in ck) == ("no_DeepAttention" not in set_keys)

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
