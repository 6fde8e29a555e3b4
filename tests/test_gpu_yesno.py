"""``label_yesno`` on the MI355X: the scorer-heads kernels (ruart_scorer_heads_fwd / _bwd, csrc/sdnet_scorer.hip) against a float64
restatement, the argument contract, ``GetFinalScores(yesno=True)`` against the reference's vectors (tests/golden/yesno_layers.npz) and
against its own op-by-op form with dropout on, and SDNet / SDNetTrainer end to end (tests/golden/sdnet_e2e_yesno.npz)."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from ruart_amd import hip, synth                          # noqa: E402
from ruart_amd.arguments import default_opt               # noqa: E402
from tests.test_yesno_host import T, check_module_against_golden      # noqa: E402

DEV = "cuda:0"
HIP_ERROR_INVALID_VALUE = 1


def maxerr(a, b):
    return float((a.detach().double().cpu() - b.detach().double().cpu()).abs().max())


def _heads_ref(x, u1, u2, uh, w, bh, mask, ES, n_front, mask_flag):
    """float64 restatement of the scorer with H pooled heads (include/ruart_hip.h):
    score_i = x_i . u(i) (u2 for i < ES, else u1; -inf where masked if mask_flag);  a_h = softmax_i(mask(x_i . uh_h)),
    s_h = w_h . sum_i a_hi x_i + bh_h;  probs = softmax([s_0 .. s_{nf-1}, score_0 .. score_{L-1}, s_nf .. s_{H-1}])"""
    L = x.shape[1]
    first = (torch.arange(L) < ES).view(1, L, 1)
    s = (x * torch.where(first, u2.unsqueeze(1), u1.unsqueeze(1))).sum(-1)
    if mask_flag:
        s = s.masked_fill(mask.eq(0), float("-inf"))
    a = torch.softmax(torch.einsum("bld,bhd->bhl", x, uh).masked_fill(mask.eq(0).unsqueeze(1), float("-inf")), 2)
    sh = (torch.einsum("bhl,bld->bhd", a, x) * w.unsqueeze(0)).sum(-1) + bh
    return torch.softmax(torch.cat([sh[:, :n_front], s, sh[:, n_front:]], 1), 1)


def _heads_inputs(B, L, D, H, g):
    x = torch.randn(B, L, D, generator=g)
    u1, u2 = (torch.randn(B, D, generator=g) / D ** 0.5 for _ in range(2))            # scores of O(1)
    uh = torch.randn(B, H, D, generator=g) / D ** 0.5
    w, bh = torch.randn(H, D, generator=g) / D ** 0.5, torch.randn(H, generator=g)
    mask = (torch.rand(B, L, generator=g) < 0.8).to(torch.uint8)                      # holes everywhere, inside the first ES slots too
    for i in range(B):
        mask[i, int(torch.randint(1, L + 1, (1,), generator=g)):] = 0                 # ragged tails
        mask[i, int(torch.randint(0, L, (1,), generator=g))] = 1                      # at least one live slot
    if B > 1:
        mask[B - 1] = 0
        mask[B - 1, L // 2] = 1                                                       # one sample with a single unmasked slot
    return x, u1, u2, uh, w, bh, mask


def _run_kernels(lib, ins, mask, gp, ES, H, n_front, mask_flag):
    """both entry points through the C ABI; returns probs, gx, gu1, gu2, guh, gw (batch sum), gb (batch sum)"""
    x, u1, u2, uh, w, bh = ins
    B, L, D = x.shape
    d = x.device
    probs, a = torch.empty(B, H + L, device=d), torch.empty(B, H, L, device=d)
    st = hip.stream_ptr()
    lib.ruart_scorer_heads_fwd(x, u1, u2, uh, w, bh, mask, probs, a, B, L, D, ES, H, n_front, mask_flag, st)
    gx, gu1, gu2 = torch.empty_like(x), torch.empty_like(u1), torch.empty_like(u2)
    guh, gwp, gbp = torch.empty_like(uh), torch.empty(B, H, D, device=d), torch.empty(B, H, device=d)
    lib.ruart_scorer_heads_bwd(x, u1, u2, uh, w, probs, a, gp, gx, gu1, gu2, guh, gwp, gbp, B, L, D, ES, H, n_front, st)
    return [probs, gx, gu1, gu2, guh, gwp.sum(0), gbp.sum(0)], a, gwp, gbp


@pytest.mark.parametrize("B,L,D", [(3, 13, 12), (2, 9, 260), (1, 5, 4)])
def test_scorer_heads_kernels_vs_float64(B, L, D):
    """The C-ABI entry points against float64 autograd of ``_heads_ref``: probabilities within 2e-5, the gradients of x, u1, u2, uh, w
    and bh within 5e-5 of max(1, |ref|) (the bounds the one-head kernels are held to), for H in {1, 3, 4}, n_front in {0, 3} (where
    <= H), ES in {0, 2}, mask_flag in {0, 1}.  Shapes: L = 13 is no multiple of the 4 waves; D = 260 wraps a lane's 256-float stride
    with a partial second trip; D = 4 is one float4 per row.  The last sample of the B > 1 shapes has a single unmasked slot.  A second
    call gives bit-equal outputs (every sum in a fixed order), the saved pooling weights and per-sample partials included.
    Measured worst over the grid: (3, 13, 12) probs 7.6e-08, gradients 1.5e-07 (gu1); (2, 9, 260) probs 8.8e-08, gradients 3.2e-07 (gw);
    (1, 5, 4) probs 7.5e-08, gradients 8.7e-08 (gu1)."""
    from ruart_amd import ops
    lib = hip.kernels()
    ops.nan_flag.ensure(torch.device(DEV))
    worst_p, worst_g = 0.0, (0.0, "")
    for H in (1, 3, 4):
        g = torch.Generator().manual_seed(B * 1000 + L + D + H)
        ins = _heads_inputs(B, L, D, H, g)
        mask = ins[6]
        gp = torch.randn(B, H + L, generator=g)
        dl = [t.to(DEV) for t in ins[:6]]
        for n_front in (0, 3):
            if n_front > H:
                continue
            for ES in (0, 2):
                for mask_flag in (0, 1):
                    leaves = [t.double().requires_grad_() for t in ins[:6]]
                    ref = _heads_ref(*leaves, mask, ES, n_front, mask_flag)
                    (ref * gp.double()).sum().backward()
                    got, a, gwp, gbp = _run_kernels(lib, dl, mask.to(DEV), gp.to(DEV), ES, H, n_front, mask_flag)
                    again, a2, gwp2, gbp2 = _run_kernels(lib, dl, mask.to(DEV), gp.to(DEV), ES, H, n_front, mask_flag)
                    ops.nan_flag.check_and_clear()
                    what = "H %d front %d ES %d flag %d" % (H, n_front, ES, mask_flag)
                    ref = ref.detach()
                    e_p = maxerr(got[0], ref) / max(1.0, float(ref.abs().max()))
                    refs = [t.grad for t in leaves]
                    e_g = {n: maxerr(t, r) / max(1.0, float(r.abs().max()))
                           for n, t, r in zip(("gx", "gu1", "gu2", "guh", "gw", "gb"), got[1:], refs)}
                    worst_p = max(worst_p, e_p)
                    worst_g = max(worst_g, max((v, n + " " + what) for n, v in e_g.items()))
                    assert abs(float(got[0].sum()) - B) < 1e-5 * B, what
                    assert e_p < 2e-5, (what, e_p)
                    assert max(e_g.values()) < 5e-5, (what, e_g)
                    assert all(torch.equal(p, q) for p, q in zip(got + [a, gwp, gbp], again + [a2, gwp2, gbp2])), what
    print("scorer heads (%d, %d, %d): probs %.2e; gradients <= %.2e (%s)" % (B, L, D, worst_p, worst_g[0], worst_g[1]))


def test_scorer_heads_refuse_shapes_outside_the_contract_and_the_module_falls_back():
    """H = 5, D = 6 and a D past the LDS rule (B = 1, L = 4, H = 4: 4 * (4 + 8 + 32 + 4 D) <= 65536 holds up to D = 4084) return
    hipErrorInvalidValue from both entry points, as do ES = L and n_front > H; D = 4084 - the largest LDS request the contract admits -
    runs.  On the refused width the module takes the op-by-op form after one refused attempt, and gives that form's answer."""
    import ruart_amd.layers as L
    from ruart_amd import ops
    lib = hip.load()
    st = hip.stream_ptr()

    def call(B, Ls, D, ES, H, n_front):
        x, u, uh = torch.randn(B, Ls, D, device=DEV), torch.randn(B, D, device=DEV) / D ** 0.5, torch.randn(B, H, D, device=DEV) / D ** 0.5
        w, bh, mask = torch.randn(H, D, device=DEV) / D ** 0.5, torch.zeros(H, device=DEV), torch.ones(B, Ls, dtype=torch.uint8, device=DEV)
        probs, a = torch.zeros(B, H + Ls, device=DEV), torch.zeros(B, H, Ls, device=DEV)
        gx, gu, gu2, guh, gw, gb = (torch.zeros_like(x), torch.zeros_like(u), torch.zeros_like(u), torch.zeros_like(uh),
                                    torch.zeros(B, H, D, device=DEV), torch.zeros(B, H, device=DEV))
        p = hip.ptr
        rc_f = lib.ruart_scorer_heads_fwd(p(x), p(u), p(u), p(uh), p(w), p(bh), p(mask), p(probs), p(a), B, Ls, D, ES, H, n_front, 1, st)
        rc_b = lib.ruart_scorer_heads_bwd(p(x), p(u), p(u), p(uh), p(w), p(probs), p(a), p(probs), p(gx), p(gu), p(gu2), p(guh), p(gw),
                                          p(gb), B, Ls, D, ES, H, n_front, st)
        return rc_f, rc_b, probs, gx

    for args in ((1, 4, 8, 2, 5, 3), (1, 4, 6, 2, 4, 3), (1, 4, 4088, 2, 4, 3), (1, 4, 8, 4, 4, 3), (1, 4, 8, 2, 3, 4), (1, 1025, 8, 2, 1, 0)):
        rc_f, rc_b, probs, gx = call(*args)
        assert rc_f == HIP_ERROR_INVALID_VALUE and rc_b == HIP_ERROR_INVALID_VALUE, (args, rc_f, rc_b)
        assert float(probs.abs().max()) == 0.0 and float(gx.abs().max()) == 0.0, args          # nothing was launched
    rc_f, rc_b, probs, gx = call(1, 4, 4084, 2, 4, 3)
    assert (rc_f, rc_b) == (0, 0) and abs(float(probs.sum()) - 1.0) < 1e-5 and bool(torch.isfinite(gx).all())

    g = torch.Generator().manual_seed(23)
    D, Hh, Ls = 4088, 8, 4
    ga = L.GetFinalScores(D, Hh, yesno=True, no_answer=True, useES=True)
    with torch.no_grad():
        for prm in ga.parameters():
            prm.copy_(torch.randn(prm.shape, generator=g) / max(prm.shape[-1], 1) ** 0.5)
    ga = ga.to(DEV).eval()
    x, h0 = torch.randn(1, Ls, D, generator=g).to(DEV), torch.randn(1, Hh, generator=g).to(DEV)
    mask = torch.tensor([[1, 1, 1, 0]], device=DEV)
    attempts = []
    real = ops.fused_scorer_heads
    saved = L.dropout_p
    try:
        ops.fused_scorer_heads = lambda *a, **k: (attempts.append(1), real(*a, **k))[1]
        L.set_dropout_prob(0.0)
        with torch.no_grad(), ops.use_trunk_mode(gemm="x3", fused_scorer=True):
            got = ga(x, h0, mask, 2, mask_flag=True)
            assert len(attempts) == 1
            with ops.use_trunk_mode(fused_scorer=False):
                want = ga(x, h0, mask, 2, mask_flag=True)
            assert len(attempts) == 1
    finally:
        ops.fused_scorer_heads = real
        L.dropout_p = saved
    assert got.shape == (1, 3 + Ls + 1) and torch.equal(got, want)


@pytest.fixture(scope="module")
def layers_golden(golden_dir):
    return np.load(os.path.join(golden_dir, "yesno_layers.npz"))


@pytest.mark.parametrize("gemm", ["fp32", "x3"])
@pytest.mark.parametrize("k", [0, 1, 2])
def test_get_final_scores_yesno_vs_reference(layers_golden, k, gemm):
    """The module on the GPU against the reference's vectors, forward and every gradient, at test_get_final_scores_vs_reference's
    tolerances; under x3 the fused form runs (once), under fp32 it does not."""
    import ruart_amd.layers as L
    from ruart_amd import ops
    calls = []
    real = ops.fused_scorer_heads
    saved = L.dropout_p
    try:
        ops.fused_scorer_heads = lambda *a, **kw: (calls.append(1), real(*a, **kw))[1]
        L.set_dropout_prob(0.0)
        with ops.use_trunk_mode(gemm=gemm, fused_scorer=True):
            check_module_against_golden(layers_golden, k, DEV, 1e-6 if gemm == "fp32" else 2e-5)
        ops.nan_flag.check_and_clear()
    finally:
        ops.fused_scorer_heads = real
        L.dropout_p = saved
    assert len(calls) == (1 if gemm == "x3" else 0)


@pytest.mark.parametrize("useES,no_answer", [(True, True), (False, True), (True, False)])
def test_fused_heads_equal_the_elementwise_form_with_variational_dropout(useES, no_answer):
    """GetFinalScores(yesno=True) in training mode with VARIATIONAL dropout (p = 0.3), the construction and bounds of
    test_fused_scorer_equals_the_elementwise_form_with_variational_dropout: from the same generator state and an unfilled MaskBank the
    fused and the op-by-op form give the same probabilities (2e-5) and the same gradients of x, h0 and every parameter (5e-5 of
    max(1, |ref|)) - the masks of x folded into u1 / u2 and the dropouts of h0 (attn, attn2, the yes/no heads', then the no-answer head's
    on the already dropped vector) drawn in the op-by-op order; one drawn out of order moves the results by O(1).
    Measured: (useES, no_answer) probs 2.4e-07, gradients 8.0e-06; (no useES) 1.5e-08, 6.1e-06; (no no_answer) 3.6e-12, 1.5e-07
    (the worst gradient is attn.linear.weight's every time)."""
    import ruart_amd.layers as L
    from ruart_amd import ops
    g = torch.Generator().manual_seed(17)
    B, Ls, D, Hh, ES = 3, 41, 252, 250, 9
    ga = L.GetFinalScores(D, Hh, yesno=True, no_answer=no_answer, useES=useES)
    with torch.no_grad():
        for prm in ga.parameters():
            prm.copy_(torch.randn(prm.shape, generator=g) / max(prm.shape[-1], 1) ** 0.5)
    ga = ga.to(DEV).train()
    x0, h00 = torch.randn(B, Ls, D, generator=g), torch.randn(B, Hh, generator=g)
    mask = (torch.rand(B, Ls, generator=g) < 0.8).float()
    mask[0, 30:], mask[1, 12:], mask[:, 3], mask[2, 1] = 0, 0, 1, 0
    gp = torch.randn(B, 3 + Ls + int(no_answer), generator=g).to(DEV)
    calls = []
    real = ops.fused_scorer_heads
    saved = (L.do_seq_dropout, L.dropout_p, L.mask_bank)

    def run(fused):
        L.mask_bank = L.MaskBank()                           # unfilled: every site draws its own mask from the generator
        torch.manual_seed(5)
        ga.zero_grad(set_to_none=True)
        x, h0 = x0.to(DEV).requires_grad_(), h00.to(DEV).requires_grad_()
        with ops.use_trunk_mode(gemm="x3", fused_scorer=fused):
            probs = ga(x, h0, mask.to(DEV), ES if useES else None, mask_flag=True)
        (probs * gp).sum().backward()
        ops.nan_flag.check_and_clear()
        return probs.detach(), {"x": x.grad, "h0": h0.grad, **{n: p.grad.clone() for n, p in ga.named_parameters() if p.grad is not None}}

    try:
        ops.fused_scorer_heads = lambda *a, **k: (calls.append(1), real(*a, **k))[1]
        L.set_dropout_prob(0.3)
        L.set_seq_dropout(True)
        p_ref, g_ref = run(False)
        assert not calls
        p_fus, g_fus = run(True)
        assert len(calls) == 1
    finally:
        ops.fused_scorer_heads = real
        L.do_seq_dropout, L.dropout_p, L.mask_bank = saved
    expect = {"x", "h0", "attn.linear.weight", "no_linear.weight", "yes_linear.bias", "no_read_linear.weight", "no_w.weight", "yes_w.bias",
              "no_read_w.weight"} | ({"attn2.linear.bias"} if useES else set()) | ({"noanswer_linear.weight", "noanswer_w.bias"} if no_answer else set())
    assert g_ref.keys() == g_fus.keys() and expect <= set(g_ref)
    e_p = float((p_fus - p_ref).abs().max()) / max(1.0, float(p_ref.abs().max()))
    e_g = {n: float((g_fus[n] - g_ref[n]).abs().max()) / max(1.0, float(g_ref[n].abs().max())) for n in g_ref}
    worst = max(e_g, key=e_g.get)
    print("fused heads vs op-by-op, dropout 0.3, useES %d no_answer %d: probs %.2e, gradients <= %.2e (%s)"
          % (useES, no_answer, e_p, e_g[worst], worst))
    assert float((p_ref[:, 3:3 + Ls][mask.to(DEV) == 0]).abs().max()) == 0.0 and float(g_ref["x"].abs().max()) > 0
    assert e_p < 2e-5
    assert e_g[worst] < 5e-5, e_g


# ---- end to end ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def e2e_golden(golden_dir):
    return np.load(os.path.join(golden_dir, "sdnet_e2e_yesno.npz"))


def _opt_and_weights(z, **extra):
    opt = default_opt(vocab_size=int(z["vocab_size"]), cuda=True, label_yesno=True, **extra)
    cfg = synth.bert_config(vocab_size=2000)
    opt["bert_state"], opt["bert_config"] = synth.make_bert_weights(cfg, seed=int(z["seed"])), cfg
    return opt, synth.make_sdnet_weights(opt, seed=int(z["seed"]))


@pytest.mark.parametrize("precision,tol_p,tol_g", [("fp32", 5e-5, 2e-3), ("x3", 2e-4, 1e-2), ("fp16c", 2e-4, 1e-2)])
def test_sdnet_yesno_forward_backward_vs_reference(e2e_golden, precision, tol_p, tol_g):
    """SDNet with opt['label_yesno'] against the unmodified reference's scores (B, 3 + 100 + 1), loss and gradients on the same seeded
    inputs, at the bounds test_sdnet_forward_backward_vs_reference holds these precision modes to.
    Measured max |dp| / worst gradient-norm error: fp32 2.1e-06 / 4.5e-05, x3 8.2e-06 / 5.8e-04, fp16c 4.0e-05 / 1.3e-03."""
    import ruart_amd.layers as L
    from ruart_amd.sdnet import SDNet
    z = e2e_golden
    opt, sw = _opt_and_weights(z, device=DEV, bert_precision=precision)
    net = SDNet(opt, {"glove_embedding": T(sw["glove_embed.weight"]), "fast_embedding": T(sw["fast_embed.weight"])})
    missing, unexpected = net.load_state_dict({k: T(v) for k, v in sw.items()}, strict=False)
    assert not missing and not unexpected, (missing, unexpected)      # state-dict keys == the reference's
    net = net.to(DEV)
    q, ocr, od, gt, _ = synth.synthetic_batch(opt, int(z["B"]), seed=int(z["batch_seed"]), n_q=30, n_ocr=100, n_od=30, bert_vocab=2000, ragged=True)
    assert ocr["num_cnt"] == z["ocr_num_cnt"].tolist() and np.array_equal(gt.numpy(), z["gt"]) and float(gt[:, :3].sum()) >= 1
    L.set_dropout_prob(0.0)
    net.train()
    net.drop_emb = False
    scores, _ = net(q, ocr, od)
    net.check_nan()
    got = scores.detach().cpu().numpy()
    err = np.abs(got - z["scores"]).max()
    assert got.shape == z["scores"].shape == (int(z["B"]), 3 + opt["max_ocr_num"] + 1) and np.allclose(got.sum(1), 1.0, atol=1e-5)
    assert err < tol_p, "max |p - p_ref| = %.3e" % err
    gt = gt.to(scores.device)
    loss = torch.nn.functional.binary_cross_entropy_with_logits(scores, gt) * gt.size(1)
    assert abs(loss.item() - float(z["loss"])) < 10 * tol_p
    loss.backward()
    params = dict(net.named_parameters())
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
    print("label_yesno, precision %s: max |dp| %.2e; worst grad-norm rel err %.2e (%s); worst grad element err / max|g| %.2e (%s)"
          % (precision, err, worst_norm[0], worst_norm[1], worst_elem[0], worst_elem[1]))
    assert worst_norm[0] < tol_g, worst_norm
    assert worst_elem[0] < 2 * tol_g, worst_elem


def test_trainer_yesno_update_predict_and_checkpoint(e2e_golden, tmp_path):
    """One SDNetTrainer.update() on the golden's batch returns a finite loss; predict() decodes B answers through decode_slots
    (ids_len = the score width, idx inside it); save_for_predict -> load_model brings the six new modules back."""
    from ruart_amd.trainer import SDNetTrainer
    z = e2e_golden
    opt, sw = _opt_and_weights(z, DROPOUT=0.0, dropout_emb=0.0)
    tr = SDNetTrainer(opt, device=DEV)
    tr.setup_model({"glove_embedding": T(sw["glove_embed.weight"]), "fast_embedding": T(sw["fast_embed.weight"])})
    B = int(z["B"])
    batch = tr.ToCUDA(synth.synthetic_batch(opt, B, seed=int(z["batch_seed"]), n_q=30, n_ocr=100, n_od=30, bert_vocab=2000, ragged=True))
    loss = float(tr.update(batch, 0))
    assert np.isfinite(loss)
    width = 3 + opt["max_ocr_num"] + 1
    loss, anls, acc, res, save_res = tr.predict(batch)
    assert len(res) == B and all("answer" in r for r in res)
    assert all(r["ids_len"] == width and 0 <= r["idx"] < width for r in save_res)
    path = str(tmp_path / "ruart_yesno_ckpt.pt")
    tr.save_for_predict(path)
    ga = tr.network.get_answer
    new = [n for n, _ in ga.named_parameters() if n.startswith(("no_", "yes_", "no_read_"))]
    assert len(new) == 12
    ck = torch.load(path, map_location="cpu")["state_dict"]["network"]
    assert all("get_answer." + n in ck for n in new)
    before = {n: p.detach().clone() for n, p in ga.named_parameters() if n in new}
    with torch.no_grad():
        for n, p in ga.named_parameters():
            if n in new:
                p.add_(1.0)
    tr.load_model(path)
    assert all(torch.equal(p.detach(), before[n]) for n, p in ga.named_parameters() if n in new)
