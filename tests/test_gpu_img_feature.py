"""Region image features (``img_feature`` / ``img_fea_way replace_od``, overlay and pure form) on the MI355X: the projection and the
attention kernels at the shapes the feature calls them with, against float64; SDNet end to end against the unmodified reference
(tests/golden/sdnet_e2e_img_overlay.npz / sdnet_e2e_img_pure.npz, written by tools/gen_golden_img_feature.py) with the exchanged
features as the negative control; the pure form's independence of the object list; the three-stream schedule; SDNetTrainer (update,
predict, checkpoint), once through a DataLoader worker that prepares the batch index."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from ruart_amd import synth                               # noqa: E402
from ruart_amd.arguments import default_opt               # noqa: E402
from tests.test_img_feature_host import CONFS, T           # noqa: E402

DEV = "cuda:0"
# the project's standing end-to-end bounds (tests/test_gpu_es_post.py): scores / gradient norms per precision
BOUNDS = {"fp32": (5e-5, 2e-3), "x3": (2e-4, 1e-2), "fp16c": (2e-4, 1e-2)}
FORMS = {"overlay": "sdnet_e2e_img_overlay", "pure": "sdnet_e2e_img_pure"}


def maxerr(a, b):
    return float((a.detach().double().cpu() - b.detach().double().cpu()).abs().max())


# ---- 1. the projection at its shape: M = 2 * 36 rows (a partial tile), K = 2048, N = 300 ---------------------------------------------
def test_projection_linear_at_the_image_feature_shape_vs_float64():
    """ops.linear (split-bf16 ruart_gemm_x3) for img_fea2od: x (72, 2048) non-negative like the features, W (300, 2048), bias.  y, dW =
    dY^T x and db against float64 at test_gemm_x3_all_layouts' bound, |err| <= 2.5e-5 * sum |a||b| + 1e-6 per element, each over its
    own contraction (db: over the 72 rows of dY); the input requires no gradient and gets none; two launches are bit-equal.
    Measured worst err / bound: y 0.024, dW 0.18, db 0.002."""
    from ruart_amd import ops
    assert ops.trunk_mode().gemm == "x3"
    M, K, N = 72, 2048, 300
    g = torch.Generator().manual_seed(72 * 7 + 300 * 3 + 2048)
    x = torch.randn(M, K, generator=g).abs()
    w = (torch.rand(N, K, generator=g) * 2 - 1) / K ** 0.5
    b = (torch.rand(N, generator=g) * 2 - 1) * 0.05
    gy = torch.randn(M, N, generator=g)
    xd = x.to(DEV)
    outs = []
    for _ in range(2):
        wd, bd = w.to(DEV).requires_grad_(), b.to(DEV).requires_grad_()
        y = ops.linear(xd, wd, bd)
        y.backward(gy.to(DEV))
        outs.append((y.detach(), wd.grad, bd.grad))
    assert xd.grad is None and not xd.requires_grad
    for a_, b_ in zip(*outs):
        assert torch.equal(a_, b_)
    y, gw, gb = (t.double().cpu() for t in outs[0])
    xx, ww, gg = x.double(), w.double(), gy.double()
    checks = {"y": (y, xx @ ww.t() + b.double(), x.abs().double() @ w.abs().double().t()),
              "dW": (gw, gg.t() @ xx, gg.abs().t() @ xx.abs()),
              "db": (gb, gg.sum(0), gg.abs().sum(0))}
    for name, (got, ref, mag) in checks.items():
        err, bound = (got - ref).abs(), 2.5e-5 * mag + 1e-6
        print("img_fea2od %s: worst err / bound %.3f, max err %.2e" % (name, float((err / bound).max()), float(err.max())))
        assert got.shape == ref.shape and bool((err <= bound).all()), (name, float((err / bound).max()))


# ---- 2. attention with an all-ones key mask over the 36 image rows -----------------------------------------------------------------------
def _attn_case(form, seed):
    B, L1, L2, h, D3 = 2, 100, 36, 125, 250
    g = torch.Generator().manual_seed(seed)
    if form == "qk":          # od_ocr_attn: projections of the two branches' high-level states
        pa, pk = torch.randn(B, L1, h, generator=g), torch.randn(B, L2, h, generator=g)
    else:                     # position_attn: projections of inputs of width 8 in [0, 1) - box corners - through one (125, 8) matrix
        W = (torch.rand(h, 8, generator=g) * 2 - 1) / 8 ** 0.5
        pa, pk = torch.rand(B, L1, 8, generator=g) @ W.t(), torch.rand(B, L2, 8, generator=g) @ W.t()
    v, gy = torch.randn(B, L2, D3, generator=g), torch.randn(B, L1, D3, generator=g)
    return pa, pk, v, gy, torch.ones(B, L2, dtype=torch.uint8), torch.full((1, 1, 1), 1.0 / h ** 0.5)


@pytest.mark.parametrize("form", ["qk", "position"])
def test_attention_over_all_live_image_rows_vs_float64(form):
    """ruart_attn_fwd / _bwd as od_ocr_attn and position_attn call them under img_feature (B = 2, L1 = 100 OCR slots, L2 = 36 image
    rows all live, h = 125, D3 = 250, scalar diagonal, ReLU) against float64 autograd at test_fused_attention_shapes' bounds: output
    2e-5, gradients 5e-5 of max(1, |ref|).
    Measured: qk form out 2.9e-07, gradients 3.8e-07 / 3.7e-07 / 4.9e-07; position form out 1.7e-07, gradients 7.8e-08 / 3.5e-07 /
    3.6e-07 (pa / pk / v)."""
    from ruart_amd import ops
    pa, pk, v, gy, mask, diag = _attn_case(form, 3600 + len(form))
    leaves = [t.double().requires_grad_() for t in (pa, pk, v)]
    s = torch.bmm(torch.relu(leaves[0]) * diag.double(), torch.relu(leaves[1]).transpose(1, 2))
    ref = torch.bmm(torch.softmax(s.masked_fill(mask.eq(0).unsqueeze(1), float("-inf")), 2), leaves[2])
    ref.backward(gy.double())
    ref = ref.detach()
    dl =[t.to(DEV).requires_grad_() for t in (pa, pk, v)]
    y = ops.fused_attention(dl[0], dl[1], dl[2], mask.to(DEV), diag=diag.to(DEV), relu=True)
    y.backward(gy.to(DEV))
    ops.nan_flag.check_and_clear()
    e_y = maxerr(y, ref) / max(1.0, float(ref.abs().max()))
    e_g = [maxerr(a.grad, b.grad) / max(1.0, float(b.grad.abs().max())) for a, b in zip(dl, leaves)]
    print("attention over 36 live rows, %s form: out %.2e, gradients pa %.2e pk %.2e v %.2e" % (form, e_y, *e_g))
    assert e_y < 2e-5
    assert max(e_g) < 5e-5, e_g


# ---- 3. end to end ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def goldens(golden_dir):
    return {form: np.load(os.path.join(golden_dir, name + ".npz")) for form, name in FORMS.items()}


@pytest.fixture(scope="module")
def bert_weights():
    cfg = synth.bert_config(vocab_size=2000)
    return cfg, synth.make_bert_weights(cfg, seed=1033)


def _opt_and_weights(form, z, bert_weights, **extra):
    opt = default_opt(vocab_size=int(z["vocab_size"]), cuda=True, **CONFS[FORMS[form]], **extra)
    opt["bert_config"], opt["bert_state"] = bert_weights
    return opt, synth.make_sdnet_weights(opt, seed=int(z["seed"]))


def _net(form, z, bert_weights, **extra):
    import ruart_amd.layers as L
    from ruart_amd.sdnet import SDNet
    opt, sw = _opt_and_weights(form, z, bert_weights, device=DEV, **extra)
    net = SDNet(opt, {"glove_embedding": T(sw["glove_embed.weight"]), "fast_embedding": T(sw["fast_embed.weight"])})
    missing, unexpected = net.load_state_dict({k: T(v) for k, v in sw.items()}, strict=False)
    assert not missing and not unexpected, (missing, unexpected)      # state-dict keys == the reference's
    net = net.to(DEV)
    L.set_dropout_prob(0.0)
    net.train()
    net.drop_emb = False
    return net, opt


def _with_features(q, fea, spa):
    q = {k: v for k, v in q.items() if not k.startswith("_ruart")}
    q["img_features"], q["img_spatials"] = fea, spa
    return q


def _batch(opt, z, prefix=""):
    """the fixture's first batch (prefix '') or its forward-only second one ('b2_'), regenerated from the stored seeds"""
    B = int(z["B"])
    q, ocr, _, gt, _ = synth.synthetic_batch(opt, B, seed=int(z[prefix + ("seed" if prefix else "batch_seed")]), n_q=30, n_ocr=100, n_od=5,
                                             bert_vocab=2000, ragged=True)
    od, _ = synth.synthetic_objects(opt, z[prefix + "od_num_cnt"].tolist(), seed=int(z[prefix + "od_seed"]), bert_vocab=2000)
    fea, spa = synth.synthetic_image_features(opt, B, seed=int(z[prefix + "fea_seed"]))
    assert ocr["num_cnt"] == z[prefix + "ocr_num_cnt"].tolist() and od["num_cnt"] == z[prefix + "od_num_cnt"].tolist()
    return _with_features(q, fea, spa), ocr, od, gt


def _loss_backward(net, scores, gt):
    net.zero_grad(set_to_none=True)
    gt = gt.to(scores.device)
    loss = torch.nn.functional.binary_cross_entropy_with_logits(scores, gt) * gt.size(1)
    loss.backward()
    return loss


def _gradient_errors(net, z):
    """worst relative gradient-norm error and worst element error / max |g| against the fixture (the stored slices of img_fea2od.weight's
    gradient among the elements); no gradient exactly where the reference has none"""
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
        got = gr.detach().cpu().numpy()
        for key, part in (("grad:" + name, got), ("gradrows:" + name, got[:4]), ("gradcols:" + name, got[:, :8] if got.ndim == 2 else got)):
            if key in z.files:
                ref = z[key]
                worst_elem = max(worst_elem, (float(np.abs(part - ref).max() / max(np.abs(ref).max(), 1e-5)), key))
    return worst_norm, worst_elem


def _scores(net, q, ocr, od):
    with torch.no_grad():
        s, _ = net(q, ocr, od)
    net.check_nan()
    return s.cpu().numpy()


@pytest.mark.parametrize("precision", ["fp32", "x3", "fp16c"])
@pytest.mark.parametrize("form", list(FORMS))
def test_sdnet_img_feature_forward_backward_vs_reference(goldens, bert_weights, form, precision):
    """SDNet with region image features against the unmodified reference's scores (B, 101), loss and gradients on the same seeded
    inputs - object counts (5, 4), so 31 and 32 of the 36 object-branch rows are image rows -, at the standing bounds (scores 5e-5 /
    2e-4 / 2e-4, gradient norms 2e-3 / 1e-2 / 1e-2, elements twice that; img_fea2od.weight's norm and its stored slices [:4, :] and
    [:, :8] among them).  ``b2_scores``: forward only, object counts (36, 1) - in the overlay form sample 0 has no image row left.
    Negative control: with the two samples' features and boxes exchanged the device reproduces the reference's ``swap_scores`` at the
    same bound - which the generator asserted to lie at least 1e-2 from ``scores``: a model that ignored or misplaced the features
    could not pass both.
    Measured max |dp| (first batch / swapped / second batch), worst gradient-norm error, worst element error:
    overlay fp32 9.8e-06 / 2.9e-06 / 2.9e-06, 9.5e-05, 3.1e-05; x3 3.0e-06 / 8.8e-06 / 7.3e-05, 2.9e-04, 2.9e-04; fp16c 6.9e-05 /
    2.9e-05 / 7.9e-05, 1.1e-03, 4.2e-04; pure fp32 8.3e-06 / 1.5e-06 / 3.8e-06, 2.1e-04, 2.3e-04; x3 8.3e-06 / 8.7e-06 / 4.3e-05,
    5.6e-05, 1.0e-04; fp16c 3.9e-05 / 8.0e-06 / 3.0e-05, 1.1e-03, 2.4e-03 (a slice of img_fea2od.weight's gradient)."""
    z = goldens[form]
    tol_p, tol_g = BOUNDS[precision]
    net, opt = _net(form, z, bert_weights, bert_precision=precision)
    q, ocr, od, gt = _batch(opt, z)
    scores, _ = net(q, ocr, od)
    net.check_nan()
    got = scores.detach().cpu().numpy()
    err = np.abs(got - z["scores"]).max()
    assert got.shape == z["scores"].shape == (int(z["B"]), opt["max_ocr_num"] + 1) and np.allclose(got.sum(1), 1.0, atol=1e-5)
    loss = _loss_backward(net, scores, gt)
    assert "img_fea2od.weight" in z["grad_names"].tolist() and "gradrows:img_fea2od.weight" in z.files
    assert net.img_fea2od.weight.grad is not None and q["img_features"].grad is None
    worst_norm, worst_elem = _gradient_errors(net, z)
    swap = _scores(net, _with_features(q, q["img_features"].flip(0).contiguous(), q["img_spatials"].flip(0).contiguous()), ocr, od)
    err_swap = np.abs(swap - z["swap_scores"]).max()
    q2, ocr2, od2, _ = _batch(opt, z, "b2_")
    err_b2 = np.abs(_scores(net, q2, ocr2, od2) - z["b2_scores"]).max()
    print("%s, precision %s: max |dp| %.2e (swapped features %.2e, second batch %.2e); worst grad-norm rel err %.2e (%s); worst grad "
          "element err / max|g| %.2e (%s)" % (FORMS[form], precision, err, err_swap, err_b2, worst_norm[0], worst_norm[1], worst_elem[0],
                                              worst_elem[1]))
    assert err < tol_p, "max |p - p_ref| = %.3e" % err
    assert abs(loss.item() - float(z["loss"])) < 10 * tol_p
    assert worst_norm[0] < tol_g, worst_norm
    assert worst_elem[0] < 2 * tol_g, worst_elem
    assert err_swap < tol_p, "swapped features: max |p - p_ref| = %.3e" % err_swap
    assert np.abs(z["swap_scores"] - z["scores"]).max() >= 1e-2 and np.abs(swap - got).max() >= 1e-2 - 2 * tol_p
    assert err_b2 < tol_p, "second batch: max |p - p_ref| = %.3e" % err_b2


# ---- 4. the pure form does not see the object list ------------------------------------------------------------------------------------------
def _scores_and_gradients(net, q, ocr, od, gt):
    """-> scores, {name: gradient}, rows of the packed encoder stream (a fresh question dict each time: the batch index is cached on it)"""
    qq = _with_features(q, q["img_features"], q["img_spatials"])
    scores, _ = net(qq, ocr, od)
    net.check_nan()
    _loss_backward(net, scores, gt)
    grads = {n: p.grad.detach().clone() for n, p in net.named_parameters() if p.grad is not None}
    return scores.detach().clone(), grads, qq["_ruart_index"].packed.T


def test_pure_form_is_bit_equal_for_any_object_list(goldens, bert_weights):
    """img_feature_replace_od: scores and every gradient are bit-equal for the fixture's object list (counts 5, 4), its second one
    (36, 32; the reference's ``od2_scores`` equal its ``scores`` bit for bit too) and a list of one sentinel item per sample - the
    encoder stream holds no object item, and multi2one's gradient comes from the OCR items alone."""
    z = goldens["pure"]
    assert np.array_equal(z["od2_scores"], z["scores"])
    net, opt = _net("pure", z, bert_weights, bert_precision="x3")
    q, ocr, od, gt = _batch(opt, z)
    od2, _ = synth.synthetic_objects(opt, z["od2_num_cnt"].tolist(), seed=int(z["od2_seed"]), bert_vocab=2000)
    od1, _ = synth.synthetic_objects(opt, (1, 1), seed=1, bert_vocab=2000)
    assert od2["num_cnt"] == [36, 32] and od1["num_cnt"] == [1, 1] and od1["fasttext"][:, 0].tolist() == [4, 4]
    s_a, g_a, T_a = _scores_and_gradients(net, q, ocr, od, gt)
    s_b, g_b, T_b = _scores_and_gradients(net, q, ocr, od2, gt)
    s_c, g_c, T_c = _scores_and_gradients(net, q, ocr, od1, gt)
    assert T_a == T_b == T_c <= int(q["bert_mask"].sum()) + int(ocr["bert_mask"].sum())     # (identical sequences are packed once)
    assert torch.equal(s_a, s_b) and torch.equal(s_a, s_c)
    assert sorted(g_a) == sorted(g_b) == sorted(g_c) and any(n.startswith("multi2one.") for n in g_a) and "img_fea2od.weight" in g_a
    for n in g_a:
        assert torch.equal(g_a[n], g_b[n]), n
    for n in g_a:
        if n.startswith("multi2one."):
            assert torch.equal(g_a[n], g_c[n]) and float(g_a[n].abs().max()) > 0, n


# ---- 5. schedule -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", list(FORMS))
def test_img_feature_three_stream_schedule_is_bit_equal_to_one_stream(goldens, bert_weights, form):
    """opt['ruart_streams'] on (the three branches overlapped; the projection runs on the object branch's stream) and off: the same
    kernels on the same operands, so forward scores are bit-equal; the gradients of both stay within the fixture's bound (x3: 1e-2)."""
    z = goldens[form]
    net, opt = _net(form, z, bert_weights, bert_precision="x3")
    q, ocr, od, gt = _batch(opt, z)

    def run():
        scores, _ = net(_with_features(q, q["img_features"], q["img_spatials"]), ocr, od)
        net.check_nan()
        _loss_backward(net, scores, gt)
        return scores.detach().clone(), _gradient_errors(net, z)

    assert net._use_streams()
    s_on, (norm_on, elem_on) = run()
    net.opt["ruart_streams"] = False
    assert not net._use_streams()
    s_off, (norm_off, elem_off) = run()
    assert torch.equal(s_on, s_off)
    tol_g = BOUNDS["x3"][1]
    print("%s streams on / off: worst grad-norm rel err %.2e / %.2e" % (FORMS[form], norm_on[0], norm_off[0]))
    assert max(norm_on[0], norm_off[0]) < tol_g and max(elem_on[0], elem_off[0]) < 2 * tol_g


# ---- 6. trainer ------------------------------------------------------------------------------------------------------------------------
class _Samples(torch.utils.data.Dataset):
    def __init__(self, samples):
        self.samples = samples

    def __len__(self):
        return len(self.samples)

    def __getitem__(self, i):
        return self.samples[i]


@pytest.mark.parametrize("form,loader", [("overlay", False), ("pure", True)])
def test_trainer_img_feature_update_predict_and_checkpoint(goldens, bert_weights, tmp_path, form, loader):
    """Two SDNetTrainer.update() steps on a batch that carries img_features / img_spatials: finite losses, img_fea2od.weight moves;
    predict() decodes No + 1 columns; the checkpoint keeps img_fea2od.*; save_for_predict -> load_model into a fresh trainer gives
    bit-equal scores.  The pure form's batch comes out of a DataLoader with one worker (a spawned one: this process holds GPU state)
    whose collate prepared the batch index (VQA_collate(prepare_index=True)): SDNet.prepare accepts that index - built without the
    object group - as it is."""
    import copy
    from ruart_amd.batch import VQA_collate
    from ruart_amd.trainer import SDNetTrainer
    z = goldens[form]
    opt, sw = _opt_and_weights(form, z, bert_weights, DROPOUT=0.0, dropout_emb=0.0)
    emb = {"glove_embedding": T(sw["glove_embed.weight"]), "fast_embedding": T(sw["fast_embed.weight"])}
    tr = SDNetTrainer(opt, device=DEV)
    tr.setup_model(emb)
    B = 2
    if loader:
        from tests.test_host_logic import _samples_like_generator
        samples = _samples_like_generator(opt, B, 5)
        fea, spa = synth.synthetic_image_features(opt, B, seed=3)
        for i, s_ in enumerate(samples):
            s_["q"]["img_features"], s_["q"]["img_spatials"] = fea[i:i + 1], spa[i:i + 1]

        # the worker is a fresh interpreter (spawn): a process that holds GPU state is not forked.  Its collate gets the conf without
        # the encoder's weights (they would travel through a pickle); the batch is collated once and copied for every use
        copt = {k: v for k, v in opt.items() if k != "bert_state"}
        dl = torch.utils.data.DataLoader(_Samples(samples), batch_size=B, num_workers=1, multiprocessing_context="spawn",
                                         collate_fn=VQA_collate(copt, prepare_index=True).VQA_collate_fun)
        (collated,) = list(dl)
        del dl

        def make():
            return copy.deepcopy(collated)
    else:
        def make():
            q, ocr, od, gt, extra = synth.synthetic_batch(opt, B, seed=int(z["batch_seed"]), n_q=30, n_ocr=100, n_od=5, bert_vocab=2000,
                                                          ragged=True)
            return _with_features(q, *synth.synthetic_image_features(opt, B, seed=3)), ocr, od, gt, extra
    raw = make()
    batch = tr.ToCUDA(raw)
    if loader:
        host = raw[0]["_ruart_host_index"]
        assert host.od is None and batch[0]["_ruart_index"] is host and host.device == torch.device(DEV)
    assert batch[0]["img_features"].device == torch.device(DEV) and tuple(batch[0]["img_features"].shape) == (B, 36, 2048)
    w = tr.network.img_fea2od.weight
    before = w.detach().clone()
    losses = [float(tr.update(batch, i)) for i in range(2)]
    assert all(np.isfinite(l) for l in losses), losses
    assert not torch.equal(w.detach(), before)
    width = opt["max_ocr_num"] + 1
    loss, anls, acc, res, save_res = tr.predict(batch)
    assert len(res) == B and all(r["ids_len"] == width and 0 <= r["idx"] < width for r in save_res)
    path = str(tmp_path / "ruart_img_ckpt.pt")
    tr.save_for_predict(path)
    ck = torch.load(path, map_location="cpu")["state_dict"]["network"]
    assert torch.equal(ck["img_fea2od.weight"], w.detach().cpu()) and "img_fea2od.bias" in ck

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
    assert torch.equal(tr2.network.img_fea2od.weight, w) and torch.equal(eval_scores(tr2), want)
    tr.close()
    tr2.close()
