"""The whole 16-bit trainable encoder (bert_train16.py) with dropout ON against a float64 encoder that applies the SAME masks.

The masks are not restated: the pass's stream id is the first draw of the CPU generator (``_Run.__init__``), the per-site seeds come
from the project's own ``_Run._seed``, and every site's mask is recovered through the C ABI from the kernel that draws it
(tests/_dropout_probe.py).  What this holds that repeatability tests cannot: every site's backward regenerates ITS OWN forward mask
(a swap of two sites' seeds in ``_Run.backward`` is repeatable and still trains), layers and heads draw their own streams, and the
attention backward carries the multiplier through delta and dS.  tests/test_dropout_ref.py shows that such mix-ups move gradient
tensors by 0.49 or more, against the 0.03 asserted here."""
import types

import pytest
import torch

pytestmark = pytest.mark.gpu

from ruart_amd import hip                                  # noqa: E402
from tests import _dropout_probe as PB                     # noqa: E402
from tests import _dropout_ref as R                        # noqa: E402

DEV = "cuda:0"
GRAD_BOUND = 3e-2            # rel-L2 per gradient tensor: the bound test_unlocked_bert_gradients_vs_reference ("x3+16") holds norms to
FWD_BOUND = 4e-3             # f16 activations of O(1) values (tests/test_gpu_train_kernels.py), on the scale of the mixed stream


@pytest.fixture(scope="module")
def case():
    """model, packed stream and float64 copies of its parameters (built once; a test sets the model's dropout probabilities and nothing else)"""
    from ruart_amd.bert import PackedTokens
    from ruart_amd.bert_train16 import BertModelTrainable16
    cfg, state, ids, mask, cu = R.encoder_case()
    model = BertModelTrainable16(state, cfg, torch.device(DEV))
    model.accurate_forward = False                          # p = 0 too runs the f16 training kernels (the rounding baseline)
    packed = PackedTokens([(ids, mask)], torch.device(DEV))
    plan = packed.train_plan(torch.device(DEV))
    assert model.supports(packed) and plan["ok"] and plan["n_win"] >= 2 and plan["n_chunks"] == 3 + 2       # 130 and 65 tokens
    assert packed.T == int(cu[-1]) and packed.Tp % 256 == 0
    params64 = {n: model._p[n].detach().double().cpu() for n in model._order}
    g_mixed = torch.randn(packed.T, int(cfg["hidden_size"]), generator=torch.Generator().manual_seed(8))
    return cfg, model, packed, ids, mask, cu, params64, g_mixed


def _site_masks(model, packed, cu, p_h, p_a, seed):
    """every dropout site's mask of a pass with stream id ``seed``, through the kernels, at the pass's own (Tp, H) and attention plan"""
    from ruart_amd.bert_train16 import _Run
    lib = hip.load()
    stub = types.SimpleNamespace(seed=seed)
    site = lambda l, k: _Run._seed(stub, l, k)
    T, Tp, H = packed.T, packed.Tp, model.hidden
    plan = packed.train_plan(torch.device(DEV))
    masks = {"emb": PB.ln_mask(lib, Tp, H, p_h, site(-1, 0), 1)[:T]}
    worst = 0.0
    for l in range(model.n_layers):
        masks["attn", l], dev = PB.attn_masks(lib, model.n_heads, cu, plan["win"], plan["chunks"], packed.tok_lo, p_a, site(l, 0))
        worst = max(worst, dev)
        masks["ao", l] = PB.ln_mask(lib, Tp, H, p_h, site(l, 1), 0)[:T]
        masks["out", l] = PB.ln_mask(lib, Tp, H, p_h, site(l, 2), 0)[:T]
    return masks, worst


@pytest.mark.parametrize("p", [0.0, 0.1])
def test_encoder16_gradients_vs_float64_with_the_same_masks(case, p):
    """forward_mixed(training=True) with p_hidden = p_attn = p on windows and chunks (sequences of 5, 64, 1, 30, 130, 65, 33 pieces):
    the mixed stream within 4e-3 of the float64 encoder's (f16 activations), and EVERY parameter's gradient tensor and d layer_w
    within 3e-2 rel-L2 of float64 autograd fed with the masks the kernels drew (p = 0.1: BERT's shipped probabilities), resp. with no
    mask on the same f16 kernels (p = 0: the rounding baseline of the same tensors).  The key biases' gradient is exactly zero here
    and rounding noise in float64.  Measured (MI355X, profiles/dropout_gradient_tests.txt): mixed 7.1e-4 (p = 0: 6.8e-4); worst
    gradient tensor 4.98e-3, a key weight (p = 0: 4.94e-3), median 3.2e-3 (3.3e-3) - dropout adds nothing to the rounding error."""
    cfg, model, packed, ids, mask, cu, params64, g_mixed = case
    model.p_hidden = model.p_attn = p
    for t in model._p.values():
        t.grad = None
    layer_w = torch.tensor(R.ENCODER_LAYER_W, device=DEV, requires_grad=True)
    torch.manual_seed(1234)
    seed = int(torch.randint(0, 2 ** 31 - 1, (1,)).item())       # the stream id the pass will draw (_Run.__init__)
    torch.manual_seed(1234)
    mixed = model.forward_mixed(packed, layer_w, training=True)
    (mixed * g_mixed.to(DEV)).sum().backward()
    torch.cuda.synchronize()
    if p > 0:
        masks, dev = _site_masks(model, packed, cu, p, p, seed)
        kept = torch.cat([masks["emb"].reshape(-1)] + [masks[k, l].reshape(-1) for k in ("ao", "out") for l in range(model.n_layers)]) > 0
        assert R.keep_sigmas(kept, p) < 5
    else:
        masks, dev = {}, 0.0
    ref_mixed, ref_g, ref_lw = R.encoder_reference(cfg, params64, ids, mask, cu, g_mixed.double(), masks)
    f_err = float((mixed.detach().double().cpu() - ref_mixed).abs().max()) / max(1.0, float(ref_mixed.abs().max()))
    errs = {"layer_w": R.rel_l2(layer_w.grad.cpu(), ref_lw)}
    floor = 1e-12 * float(ref_g["encoder.layer.1.output.dense.weight"].norm())
    for n in model._order:
        got = model._p[n].grad
        assert got is not None, n
        if float(ref_g[n].norm()) <= floor:                      # key biases: the softmax ignores a shift of a query row's scores
            assert n.endswith("attention.self.key.bias") and float(got.abs().max()) == 0.0, n
            continue
        errs[n] = R.rel_l2(got.cpu(), ref_g[n])
    order = sorted(errs, key=errs.get, reverse=True)
    print("encoder16 p=%.1f: attention mask entries off by <= %.2e; mixed %.2e of max(1, |ref|); gradient rel-L2: worst %s, median %.2e"
          % (p, dev, f_err, ", ".join("%s %.2e" % (n, errs[n]) for n in order[:4]), errs[order[len(order) // 2]]))
    assert f_err < FWD_BOUND
    assert errs[order[0]] <= GRAD_BOUND, [(n, errs[n]) for n in order if errs[n] > GRAD_BOUND]


def test_encoder16_masks_differ_between_sites_layers_and_passes(case):
    """The masks one pass draws: two layers' attention masks, and the two dense-output sites of a layer, agree as independent streams
    do (p^2 + (1-p)^2 within 5 sigma) - one mask shared by layers or sites would agree at 1.  Measured: 1.8 sigma at the worst."""
    cfg, model, packed, ids, mask, cu, params64, g_mixed = case
    p = 0.1
    masks, _ = _site_masks(model, packed, cu, p, p, 0x3C0FFEE)
    flat = lambda ms: torch.cat([m.reshape(-1) for m in ms]) > 0
    cells = {"attention, layers 0 / 1": (flat(masks["attn", 0]), flat(masks["attn", 1])),
             "layer 0: attention-output / output": (masks["ao", 0] > 0, masks["out", 0] > 0),
             "output, layers 0 / 1": (masks["out", 0] > 0, masks["out", 1] > 0),
             "embeddings / layer 0 attention-output": (masks["emb"] > 0, masks["ao", 0] > 0)}
    sig = {k: R.agree_sigmas(a, b, p) for k, (a, b) in cells.items()}
    print("encoder16 site masks: agreement off by <= %.2f sigma (%s)" % (max(sig.values()), max(sig, key=sig.get)))
    assert max(sig.values()) < 5, sig
