"""opt['bert_train_layers'] = N on the GPU: the embeddings and the encoder layers below k = n_layers - N stay frozen, the top N train on
the 16-bit kernels (bert_train16.py); with BERT dropout active the frozen part runs on the frozen path's fp16c kernels - one step ahead
when the trainer knows the next batch - and ``ruart_rows_ln_to_16`` hands its rows over."""
import functools
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from ruart_amd import hip, synth                         # noqa: E402
from ruart_amd.arguments import default_opt               # noqa: E402

DEV = "cuda:0"


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a))


@functools.lru_cache(maxsize=None)
def _bert(seed, w_std, dropout):
    """(synthetic bert-base checkpoint, its config) - built once per module and never written to"""
    kw = {} if dropout else {"hidden_dropout_prob": 0.0, "attention_probs_dropout_prob": 0.0}
    cfg = synth.bert_config(vocab_size=2000, **kw)
    return synth.make_bert_weights(cfg, seed=seed, w_std=w_std), cfg


def _is_frozen(name, k):
    if not name.startswith("Bert.bert_model."):
        return False
    rest = name[len("Bert.bert_model."):]
    if rest.startswith("embeddings."):
        return True
    return rest.startswith("encoder.layer.") and int(rest.split(".")[2]) < k


def _net(z, **extra):
    """SDNet of the unlocked golden file (tests/test_gpu_sdnet.py, ``_unlocked``) in the default fp16c encoder precision, 16-bit trainable
    encoder, BERT dropout probabilities 0 in the config."""
    from ruart_amd.sdnet import SDNet
    opt = default_opt(vocab_size=int(z["vocab_size"]), cuda=True, device=DEV, bert_train_gemm="16", **extra)
    opt.pop("LOCK_BERT")
    opt["bert_state"], opt["bert_config"] = _bert(int(z["seed"]), 0.05, False)
    sw = synth.make_sdnet_weights(opt, seed=int(z["seed"]))
    net = SDNet(opt, {"glove_embedding": T(sw["glove_embed.weight"]), "fast_embedding": T(sw["fast_embed.weight"])})
    missing, unexpected = net.load_state_dict({k: T(v) for k, v in sw.items()}, strict=False)
    assert not unexpected and all(k.startswith("Bert.bert_model.") for k in missing)
    import ruart_amd.layers as L
    L.set_dropout_prob(0.0)
    net = net.to(DEV)
    net.train()
    net.drop_emb = False
    return net, opt


def _batch(z, opt):
    return synth.synthetic_batch(opt, int(z["B"]), seed=int(z["batch_seed"]), n_q=12, n_ocr=16, n_od=6, bert_vocab=2000, ragged=True)


def _fwd_bwd(net, batch):
    q, ocr, od, gt, _ = batch
    net.zero_grad(set_to_none=True)
    scores, _ = net(q, ocr, od)
    gt = gt.to(scores.device)
    (torch.nn.functional.binary_cross_entropy_with_logits(scores, gt) * gt.size(1)).backward()
    net.check_nan()
    return scores.detach().clone(), {n: p.grad.detach().clone() for n, p in net.named_parameters() if p.grad is not None}


@pytest.fixture(scope="module")
def z(golden_dir):
    return np.load(os.path.join(golden_dir, "sdnet_e2e_unlocked.npz"))


@pytest.fixture(scope="module")
def full_unlock(z):
    """scores and gradients of the fully unlocked 16-bit encoder on the golden batch, dropout off (computed once; read-only)"""
    net, opt = _net(z)
    scores, grads = _fwd_bwd(net, _batch(z, opt))
    assert "Bert.bert_model.encoder.layer.0.output.dense.weight" in grads and "Bert.bert_model.embeddings.word_embeddings.weight" in grads
    return scores, grads


@pytest.mark.parametrize("n_train", [1, 2, 11])
def test_frozen_means_frozen(z, full_unlock, n_train):
    """Dropout off: the forward is the whole fp16c pass over the live parameters either way and the backward runs the same kernels in
    the same order, it only ends with layer k - scores and every gradient that exists are bit-equal to the full unlock's, and nothing
    below the cut has a gradient.  (Without the feature the key is ignored and layer 0 gets one.)"""
    k = 12 - n_train
    net, opt = _net(z, bert_train_layers=n_train)
    names = dict(net.named_parameters())
    frozen = [n for n in names if _is_frozen(n, k)]
    assert len(frozen) == 5 + 16 * k
    assert all(not names[n].requires_grad for n in frozen)
    assert all(p.requires_grad for n, p in names.items() if n.startswith("Bert.bert_model.encoder.layer.") and not _is_frozen(n, k))
    scores, grads = _fwd_bwd(net, _batch(z, opt))
    assert all(names[n].grad is None for n in frozen), [n for n in frozen if names[n].grad is not None][:3]
    ref_scores, ref_grads = full_unlock
    assert torch.equal(scores, ref_scores)
    assert set(grads) == set(n for n in ref_grads if not _is_frozen(n, k))
    assert sum(n.startswith("Bert.bert_model.encoder.layer.") for n in grads) == 16 * n_train
    assert "alphaBERT" in grads and "gammaBERT" in grads
    diff = [n for n in grads if not torch.equal(grads[n], ref_grads[n])]
    assert not diff, diff[:5]


@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("n_tok", [5, 300])
def test_handover_kernel_through_the_c_abi(k, n_tok):
    """ruart_rows_ln_to_16 against (y - mu) rstd gamma + beta in fp64 rounded to f16, bound: one f16 ulp (the spacing of f16 numbers at
    the reference value, subnormal range included).  Rows of |y| up to 450 (the outlier fixture's range), near-constant rows (rstd ~ 1e3);
    T = 5: one 256-row tile with 251 pad rows, T = 300: two tiles with 212.  Pad rows exactly zero and never read (their inputs are NaN),
    the planes k .. of the destination untouched.  Measured: at most 1.00 ulp, 0.006 % of the elements off the rounded fp64 value."""
    H, NL = 768, k + 2
    Tp = (n_tok + 255) // 256 * 256
    rng = np.random.RandomState(100 * k + n_tok)
    mu_r = rng.uniform(-300.0, 300.0, size=(k, n_tok, 1))
    sg_r = np.exp(rng.uniform(np.log(1e-3), np.log(60.0), size=(k, n_tok, 1)))
    sg_r[:, 0] = 1e-3                                       # a near-constant row at a large offset ...
    mu_r[:, 0] = 290.0
    sg_r[:, 2] = 60.0                                       # ... and a wide one, clipped at 450
    mu_r[:, 2] = 290.0
    y = np.full((k, Tp, H), np.nan, dtype=np.float32)
    y[:, :n_tok] = np.clip(mu_r + sg_r * rng.standard_normal((k, n_tok, H)), -450.0, 450.0).astype(np.float32)
    real = y[:, :n_tok].astype(np.float64)
    assert np.abs(real).max() > 400.0
    stats = np.full((k, Tp, 2), np.nan, dtype=np.float32)
    stats[:, :n_tok, 0] = real.mean(-1)
    stats[:, :n_tok, 1] = 1.0 / np.sqrt(real.var(-1) + 1e-12)
    assert stats[:, :n_tok, 1].max() > 500.0
    g = (1.0 + 0.3 * rng.standard_normal((k, H))).astype(np.float32)
    b = (0.2 * rng.standard_normal((k, H))).astype(np.float32)
    mu64, rs64 = stats[:, :n_tok, 0:1].astype(np.float64), stats[:, :n_tok, 1:2].astype(np.float64)
    ref16 = ((real - mu64) * rs64 * g[:, None, :].astype(np.float64) + b[:, None, :].astype(np.float64)).astype(np.float16)
    assert np.isfinite(ref16).all()

    lib = hip.load()
    d = lambda a: torch.from_numpy(a).to(DEV)
    y_d, st_d, g_d, b_d = d(y), d(stats), d(g), d(b)
    out = torch.full((NL, Tp, H), 7.0, dtype=torch.float16, device=DEV)
    rc = lib.ruart_rows_ln_to_16(hip.ptr(y_d), Tp * H, H, hip.ptr(st_d), Tp, hip.ptr(g_d), hip.ptr(b_d), hip.ptr(out), Tp * H, H, k, n_tok, Tp, H,
                                 hip.stream_ptr())
    assert rc == 0
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert (got[k:] == np.float16(7.0)).all()                               # planes k .. untouched
    assert (got[:k, n_tok:].view(np.uint16) == 0).all()                     # pad rows: +0 exactly
    ulp = np.spacing(np.abs(ref16)).astype(np.float64)
    err = np.abs(got[:k, :n_tok].astype(np.float64) - ref16.astype(np.float64)) / ulp
    print("ruart_rows_ln_to_16 k=%d T=%d: worst error %.2f f16 ulp, %.4f %% of the elements differ from the rounded fp64 value"
          % (k, n_tok, err.max(), 100.0 * (err > 0).mean()))
    assert err.max() <= 1.0
    # argument checks: more tokens than rows, a destination plane stride shorter than a plane
    assert lib.ruart_rows_ln_to_16(hip.ptr(y_d), Tp * H, H, hip.ptr(st_d), Tp, hip.ptr(g_d), hip.ptr(b_d), hip.ptr(out), Tp * H, H, k, Tp + 1, Tp, H,
                                   hip.stream_ptr()) != 0
    assert lib.ruart_rows_ln_to_16(hip.ptr(y_d), Tp * H, H, hip.ptr(st_d), Tp, hip.ptr(g_d), hip.ptr(b_d), hip.ptr(out), Tp * H - 4, H, k, n_tok, Tp,
                                   H, hip.stream_ptr()) != 0


def test_dropout_on_is_repeatable_and_saves_memory(z):
    """N = 2 with BERT dropout 0.1 / 0.1: the frozen layers run the frozen path's deterministic pass, the two trained ones draw
    hash-generated masks - two passes from one generator state agree bit for bit, another seed gives other scores; no frozen tensor has a
    gradient; the peak of allocated memory over a forward and backward is below the full unlock's on the same batch (ten layers' saved
    activations and transposed weights are gone; the frozen pass's own buffers, allocated in this very pass, are counted)."""
    def peak_of_one_pass(net, batch):
        torch.manual_seed(5)
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        _fwd_bwd(net, batch)
        torch.cuda.synchronize()
        net.zero_grad(set_to_none=True)
        return torch.cuda.max_memory_allocated() - base

    full, opt_f = _net(z)
    part, opt = _net(z, bert_train_layers=2)
    for net in (full, part):
        net.Bert.bert_model.p_hidden = net.Bert.bert_model.p_attn = 0.1
    batch = _batch(z, opt)
    peak_part = peak_of_one_pass(part, batch)                # the first pass of each: nothing is warm
    peak_full = peak_of_one_pass(full, _batch(z, opt_f))
    print("peak allocated over one forward + backward: N = 2 %.1f MB, full unlock %.1f MB" % (peak_part / 2 ** 20, peak_full / 2 ** 20))
    assert peak_part < peak_full
    del full

    def run(seed):
        torch.manual_seed(seed)
        return _fwd_bwd(part, batch)

    s1, g1 = run(5)
    s2, g2 = run(5)
    s3, _ = run(6)
    assert torch.equal(s1, s2) and not torch.equal(s1, s3)
    assert g1.keys() == g2.keys() and all(torch.equal(g1[n], g2[n]) for n in g1), [n for n in g1 if not torch.equal(g1[n], g2[n])][:3]
    assert sum(n.startswith("Bert.bert_model.encoder.layer.") for n in g1) == 32 and not any(_is_frozen(n, 10) for n in g1)
    assert all(p.grad is None for n, p in part.named_parameters() if _is_frozen(n, 10))


def test_mixed_kernel_forward_against_the_reference(z):
    """Dropout probabilities 0 but ``bert_train_accurate_fwd`` off, N = 6: six frozen layers on the fp16c kernels, the hand-over, six
    layers on the plain f16 training kernels.  Bounds: the project's own for a plain 16-bit forward - scores 3e-3 (the x3+16gemm row of
    test_unlocked_bert_gradients_vs_reference), gradient norms of the trained encoder tensors 3e-2 (that test's bound for them).
    Measured: max |dp| 5.5e-4, worst gradient-norm error 1.2e-2 (layer 6, key weight); the test prints both."""
    net, opt = _net(z, bert_train_layers=6, bert_train_accurate_fwd=False)
    assert net.Bert.bert_model.mixed_pass(True) and not net.Bert.bert_model.accurate_forward
    scores, grads = _fwd_bwd(net, _batch(z, opt))
    err = float(np.abs(scores.cpu().numpy() - z["scores"]).max())
    worst, n_held = (0.0, ""), 0
    for name, ref_norm in zip(z["grad_names"].tolist(), z["grad_norms"].tolist()):
        if not name.startswith("Bert.bert_model.encoder.layer.") or _is_frozen(name, 6):
            assert not _is_frozen(name, 6) or name not in grads, name
            continue
        if ref_norm < 0:
            assert name not in grads or float(grads[name].norm()) == 0.0, name
            continue
        n_held += 1
        worst = max(worst, (abs(float(grads[name].double().norm()) - ref_norm) / max(ref_norm, 1e-4), name))
    print("mixed-kernel forward, N = 6: max |dp| %.2e, worst gradient-norm error of %d trained encoder tensors %.2e (%s)"
          % (err, n_held, worst[0], worst[1]))
    assert n_held == 6 * 16
    assert err < 3e-3, "max |p - p_ref| = %.3e" % err
    assert worst[0] < 3e-2, worst


def _trainer(prefetch=None, **extra):
    from ruart_amd.trainer import SDNetTrainer
    opt = default_opt(vocab_size=600, cuda=True, DROPOUT=0.0, dropout_emb=0.0, lr=2e-4, bert_train_gemm="16", bert_train_layers=2, **extra)
    opt.pop("LOCK_BERT")
    if prefetch is not None:
        opt["bert_train_prefetch"] = prefetch
    opt["bert_state"], opt["bert_config"] = _bert(7, 0.02, True)          # BERT dropout 0.1 / 0.1
    sw = synth.make_sdnet_weights(opt, seed=7)
    tr = SDNetTrainer(opt, device=DEV)
    tr.setup_model({"glove_embedding": T(sw["glove_embed.weight"]), "fast_embedding": T(sw["fast_embed.weight"])})
    return tr, opt


def test_run_ahead_equals_inline_bitwise():
    """The frozen layers' pass of the NEXT batch on the CU-masked stream (two buffer sets in turn) against the same pass inline
    (``bert_train_prefetch`` = False): three batches in rotation, five updates with lookahead, an evaluation in between, two more
    updates - every loss, the prediction, every parameter and both Adamax moments bit for bit.  One-stream trunk in both arms."""
    def run(prefetch):
        tr, opt = _trainer(prefetch=prefetch, ruart_streams=False)
        bs = [tr.ToCUDA(synth.synthetic_batch(opt, 3, seed=50 + i, n_q=10 + i, n_ocr=14 + i, n_od=5 + (i % 2), bert_vocab=2000, ragged=True))
              for i in range(3)]
        torch.manual_seed(99)
        assert tr.network.Bert.n_frozen == 10
        tr.network.train()
        assert tr.network.Bert.runs_ahead() == (prefetch is not False)
        out = []
        for i in range(5):
            out.append(float(tr.update(bs[i % 3], i, next_batch=bs[(i + 1) % 3])))      # the fifth leaves a pass in flight
        if prefetch is not False:
            assert tr.network.Bert._pending is not None
        out.append(tr.predict(bs[0]))
        for i in range(5, 7):
            out.append(float(tr.update(bs[i % 3], i, next_batch=bs[(i + 1) % 3])))
        tr.close()
        params = {n: p.detach().clone() for n, p in tr.network.named_parameters()}
        moments = {n: {m: v.clone() for m, v in tr.optimizer.state[id(p)].items()} for n, p in tr.network.named_parameters()
                   if id(p) in tr.optimizer.state}
        return out, params, moments

    oa, pa, ma = run(False)
    ob, pb, mb = run(None)                                   # the default: run ahead
    assert oa == ob, (oa, ob)
    assert pa.keys() == pb.keys() and ma.keys() == mb.keys()
    assert not [n for n in pa if not torch.equal(pa[n], pb[n])]
    assert not [n for n in ma if not (torch.equal(ma[n]["exp_avg"], mb[n]["exp_avg"]) and torch.equal(ma[n]["exp_inf"], mb[n]["exp_inf"]))]
    assert any(n.startswith("Bert.bert_model.encoder.layer.11.") for n in ma)


def test_trainer_end_to_end(tmp_path):
    """N = 2 through the trainer: the loss on a fixed batch comes down, layer 11 moves, layer 3 and the word-embedding table keep their
    bits, the optimizer knows no frozen tensor, and the prediction checkpoint carries the two trained layers - a fresh trainer of the
    same conf that loads it predicts exactly the same."""
    tr, opt = _trainer()
    names = dict(tr.network.named_parameters())
    w3, w11, emb = ("Bert.bert_model.encoder.layer.3.output.dense.weight", "Bert.bert_model.encoder.layer.11.output.dense.weight",
                    "Bert.bert_model.embeddings.word_embeddings.weight")
    before = {n: names[n].detach().clone() for n in (w3, w11, emb)}
    frozen = [n for n in names if _is_frozen(n, 10)]
    assert len(frozen) == 5 + 160 and all(id(names[n]) not in tr.optimizer.state for n in frozen)
    assert all(id(p) in tr.optimizer.state for n, p in names.items() if n.startswith("Bert.bert_model.encoder.layer.1") and not _is_frozen(n, 10))
    batch = tr.ToCUDA(synth.synthetic_batch(opt, 3, seed=31, n_q=10, n_ocr=14, n_od=5, bert_vocab=2000, ragged=True))
    losses = [float(v) for v in [tr.update(batch, i) for i in range(6)]]
    assert all(np.isfinite(losses)), losses
    assert min(losses[3:]) < losses[0], losses
    assert not torch.equal(before[w11], names[w11].detach())
    assert torch.equal(before[w3], names[w3].detach()) and torch.equal(before[emb], names[emb].detach())
    assert all(names[n].grad is None for n in frozen)
    assert all(id(names[n]) not in tr.optimizer.state for n in frozen)
    pred = tr.predict(batch)
    tr.network.eval()
    with torch.no_grad():
        s_a, _ = tr.network(batch[0], batch[1], batch[2])
    path = str(tmp_path / "ruart_ckpt_top2.pt")
    tr.save_for_predict(path)
    keys = list(torch.load(path, map_location="cpu")["state_dict"]["network"])
    bert_keys = [k for k in keys if k.startswith("Bert")]
    assert sorted(bert_keys) == sorted(n for n in names if n.startswith("Bert.bert_model.encoder.layer.1") and not _is_frozen(n, 10))
    assert len(bert_keys) == 32 and any(".layer.10." in k for k in bert_keys) and any(".layer.11." in k for k in bert_keys)
    assert not any(".layer.0." in k or "embeddings" in k for k in bert_keys)
    tr.close()

    tr2, _ = _trainer()
    assert not torch.equal(dict(tr2.network.named_parameters())[w11].detach(), names[w11].detach())
    tr2.load_model(path)
    assert torch.equal(dict(tr2.network.named_parameters())[w11].detach(), names[w11].detach())
    assert tr2.predict(batch) == pred
    tr2.network.eval()
    with torch.no_grad():
        s_b, _ = tr2.network(batch[0], batch[1], batch[2])
    assert torch.equal(s_a, s_b)
    tr2.close()
