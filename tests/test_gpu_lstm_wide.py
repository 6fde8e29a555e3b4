"""The streamed LSTM recurrence for 128 < hidden <= 256 on the MI355X (ruart_lstm_fwd / _bwd's streamed kernels through ops.lstm_layer and
layers.StackedBRNN): against the float64 restatement of tests/_lstm_wide_ref.py at the bounds test_lstm_layer holds the resident
kernels to, the forward-only call, the NaN flag, the module's routing, and SDNet end to end at hidden_size 144 against the unmodified
reference (tests/golden/sdnet_e2e_hidden144.npz, written by tools/gen_golden_hidden.py)."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from ruart_amd import synth                               # noqa: E402
from ruart_amd.arguments import default_opt               # noqa: E402
from tests import _lstm_wide_ref as R                      # noqa: E402
from tests import test_gpu_es_post as E                    # noqa: E402  (the end-to-end helpers and the standing bounds)
from tests.test_es_post_host import T                      # noqa: E402

DEV = "cuda:0"


def _device_layer(shape, grad=True):
    from ruart_amd import ops
    x, P, gy = R.make_case(shape)
    xd = x.to(DEV).requires_grad_(grad)
    Pd = [[t.to(DEV).requires_grad_(grad) for t in p] for p in P]
    y = ops.lstm_layer(xd, *Pd[0], *(Pd[1] if len(Pd) > 1 else []))
    if grad:
        y.backward(gy.to(DEV))
    return y.detach(), xd, Pd


@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: "x".join(str(int(v)) for v in s))
def test_lstm_layer_wide_vs_float64(shape):
    """ops.lstm_layer forward + backward for 128 < h <= 256 against float64, at test_lstm_layer's bounds: output 2e-5, dx
    5e-5 max(1, |ref|max), every parameter gradient 1e-4 max(1, |ref|max).
    Measured on the MI355X, output / dx / worst parameter gradient over its bound:
      (3, 5, 12, 129)    1.9e-06 / 2.9e-06 / 0.094 (w_ih)     (17, 7, 8, 256)    9.1e-07 / 3.1e-06 / 0.048 (w_ih)
      (2, 1, 5, 200)     4.0e-07 / 1.1e-06 / 0.032 (w_ih)     (33, 40, 20, 250)  1.4e-06 / 3.1e-06 / 0.047 (w_ih)
      (64, 100, 16, 256) 1.4e-06 / 4.7e-06 / 0.049 (w_ih)
    The parameter gradients' error is mostly the split-bf16 weight-gradient GEMM's (the float64 reference of tests/_lstm_wide_ref.py's
    emulation takes those products exactly: 0.004-0.045 there)."""
    from ruart_amd import ops
    y, xd, Pd = _device_layer(shape)
    ops.nan_flag.check_and_clear()
    errs = R.errors((y, xd.grad, [[t.grad for t in p] for p in Pd]), shape)
    print(shape, " ".join("%s %.2e/%.1e" % e for e in errs))
    for name, err, bound in errs:
        assert err < bound, (name, err, bound)


@pytest.mark.parametrize("shape", [R.SHAPES[0], R.SHAPES[3]], ids=["129", "250"])
def test_forward_only_call_is_bit_equal_to_the_training_forward(shape):
    """No requires_grad anywhere: gates / cells / hprev are NULL and the kernel skips their stores; the output is the training call's."""
    from ruart_amd import ops
    y_train, _, _ = _device_layer(shape)
    y_eval, _, _ = _device_layer(shape, grad=False)
    ops.nan_flag.check_and_clear()
    assert torch.equal(y_train, y_eval)


def test_nan_in_one_batch_row_raises_the_flag_and_leaves_the_other_rows():
    """A NaN in xproj of one batch row: the device flag goes up (check_and_clear -> AssertionError), that row's output is NaN from the
    poisoned step on, every other row - the 15 that share its 16-row tile included - matches float64, and the device works afterwards."""
    from ruart_amd import ops
    B, Tn, h = 18, 4, 144
    g = torch.Generator().manual_seed(144)
    xproj = torch.randn(B, Tn, 4 * h, generator=g)
    w_hh = (torch.rand(1, 4 * h, h, generator=g) * 2 - 1) / np.sqrt(h)
    xproj[5, 1, 7] = float("nan")
    y = ops._LstmRecurrence.apply(xproj.to(DEV), w_hh.to(DEV), 1)
    with pytest.raises(AssertionError):
        ops.nan_flag.check_and_clear()
    ops.nan_flag.check_and_clear()                      # cleared by the check
    torch.cuda.synchronize()
    ref = R._recur_fwd(xproj.double(), w_hh[0].double(), False, torch.float64, False)[0]
    keep = [b for b in range(B) if b != 5]
    assert bool(torch.isfinite(y[keep]).all()) and bool(torch.isnan(y[5, 1:]).any())
    assert R.maxerr(y[keep], ref[keep]) < R.OUT_BOUND and R.maxerr(y[5, 0], ref[5, 0]) < R.OUT_BOUND
    y2, _, _ = _device_layer(R.SHAPES[2])
    ops.nan_flag.check_and_clear()
    assert R.maxerr(y2, R.reference64(R.SHAPES[2])[0]) < R.OUT_BOUND


class _SteppedRoute(Exception):
    pass


def test_stacked_brnn_routes_up_to_256_to_the_persistent_kernels(monkeypatch):
    """hidden_size 144: forward and backward never touch the stepped route (layers.lstm_layer_stepped); hidden_size 300 still takes it."""
    import ruart_amd.layers as L

    def refuse(*a, **k):
        raise _SteppedRoute()
    monkeypatch.setattr(L, "lstm_layer_stepped", refuse)
    L.set_dropout_prob(0.0)
    torch.manual_seed(0)
    m = L.StackedBRNN(20, 144, 2, bidirectional=True).to(DEV)
    x = torch.randn(3, 6, 20, device=DEV, requires_grad=True)
    y = m(x, None)
    y.sum().backward()
    assert y.shape == (3, 6, 288) and bool(torch.isfinite(x.grad).all()) and m.rnns[1].weight_hh_l0_reverse.grad is not None
    wide = L.StackedBRNN(20, 300, 1, bidirectional=True).to(DEV)
    with pytest.raises(_SteppedRoute):
        wide(x.detach(), None)


# ---- end to end ---------------------------------------------------------------------------------------------------------------------
NAME, KEYS = "sdnet_e2e_hidden144", dict(hidden_size=144, highlvl_hidden_size=144)


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, NAME + ".npz"))


@pytest.fixture(scope="module")
def bert_weights():
    cfg = synth.bert_config(vocab_size=2000)
    return cfg, synth.make_bert_weights(cfg, seed=1033)


def _net(z, bert_weights, **extra):
    import ruart_amd.layers as L
    from ruart_amd.sdnet import SDNet
    opt = default_opt(vocab_size=int(z["vocab_size"]), cuda=True, device=DEV, **KEYS, **extra)
    opt["bert_config"], opt["bert_state"] = bert_weights
    sw = synth.make_sdnet_weights(opt, seed=int(z["seed"]))
    net = SDNet(opt, {"glove_embedding": T(sw["glove_embed.weight"]), "fast_embedding": T(sw["fast_embed.weight"])})
    missing, unexpected = net.load_state_dict({k: T(v) for k, v in sw.items()}, strict=False)
    assert not missing and not unexpected, (missing, unexpected)      # state-dict keys == the reference's
    assert sorted(net.state_dict().keys()) == sorted(z["keys"].tolist())
    net = net.to(DEV)
    L.set_dropout_prob(0.0)
    net.train()
    net.drop_emb = False
    return net, opt


@pytest.mark.parametrize("precision", ["fp32", "x3", "fp16c"])
def test_sdnet_hidden144_forward_backward_vs_reference(golden, bert_weights, precision):
    """SDNet at hidden_size = highlvl_hidden_size = 144 against the unmodified reference's scores, loss and gradients on the same seeded
    inputs, at the standing end-to-end bounds (tests/test_gpu_es_post.py BOUNDS: scores / gradient norms (5e-5, 2e-3) for fp32,
    (2e-4, 1e-2) for x3 and fp16c; small gradients' elements twice that).  Which route the trunk's (Bi)LSTMs take is the routing test's business, not this one's.
    Measured max |dp| / worst gradient-norm error / worst element error: fp32 3.6e-06 / 8.1e-05 / 6.7e-05, x3 1.0e-04 / 2.8e-04 /
    2.4e-04, fp16c 4.7e-05 / 4.4e-04 / 3.5e-04."""
    z = golden
    tol_p, tol_g = E.BOUNDS[precision]
    net, opt = _net(z, bert_weights, bert_precision=precision)
    assert net.context_rnn.hidden_size == 144
    q, ocr, od, gt = E._batch(opt, z)
    scores, _ = net(q, ocr, od)
    net.check_nan()
    got = scores.detach().cpu().numpy()
    err = np.abs(got - z["scores"]).max()
    assert got.shape == z["scores"].shape == (int(z["B"]), opt["max_ocr_num"] + 1) and np.allclose(got.sum(1), 1.0, atol=1e-5)
    loss = E._loss_backward(net, scores, gt)
    worst_norm, worst_elem = E._gradient_errors(net, z)
    print("%s, precision %s: max |dp| %.2e; worst grad-norm rel err %.2e (%s); worst grad element err / max|g| %.2e (%s)"
          % (NAME, precision, err, worst_norm[0], worst_norm[1], worst_elem[0], worst_elem[1]))
    assert err < tol_p, "max |p - p_ref| = %.3e" % err
    assert abs(loss.item() - float(z["loss"])) < 10 * tol_p
    assert worst_norm[0] < tol_g, worst_norm
    assert worst_elem[0] < 2 * tol_g, worst_elem


def test_hidden144_three_stream_schedule_is_bit_equal_to_one_stream(golden, bert_weights):
    """opt['ruart_streams'] on and off: the same kernels on the same operands - each streamed LSTM call with a workspace of its own -, so
    the forward scores are bit-equal; the gradients of both stay within the fixture's bound (x3: 1e-2)."""
    z = golden
    net, opt = _net(z, bert_weights, bert_precision="x3")
    q, ocr, od, gt = E._batch(opt, z)
    assert net._use_streams()
    s_on, (norm_on, elem_on) = E._scores_and_gradients(net, q, ocr, od, gt, z)
    net.opt["ruart_streams"] = False
    assert not net._use_streams()
    s_off, (norm_off, elem_off) = E._scores_and_gradients(net, q, ocr, od, gt, z)
    assert torch.equal(s_on, s_off)
    tol_g = E.BOUNDS["x3"][1]
    print("%s streams on / off: worst grad-norm rel err %.2e / %.2e" % (NAME, norm_on[0], norm_off[0]))
    assert max(norm_on[0], norm_off[0]) < tol_g and max(elem_on[0], elem_off[0]) < 2 * tol_g
