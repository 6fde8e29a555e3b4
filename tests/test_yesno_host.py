"""``label_yesno`` without a GPU: the op-by-op ``GetFinalScores(yesno=True)`` on the CPU against the reference's own vectors
(tests/golden/yesno_layers.npz, written by tools/gen_golden_yesno.py from the unmodified reference), its state-dict keys, the decode of
the slot layout with three front slots (predict_decode_yesno.json) and the draw order of the synthetic weights."""
import json
import os

import numpy as np
import pytest
import torch

from ruart_amd import synth
from ruart_amd.arguments import default_opt


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def _close(got, ref, atol, rtol, what):
    got = got.detach().float().cpu().numpy() if isinstance(got, torch.Tensor) else got
    err = np.abs(got - ref).max()
    assert got.shape == ref.shape and err <= atol + rtol * np.abs(ref).max(), "%s: max err %.3e" % (what, err)


@pytest.fixture(scope="module")
def layers_golden(golden_dir):
    return np.load(os.path.join(golden_dir, "yesno_layers.npz"))


def build_module(z, k, device="cpu"):
    import ruart_amd.layers as L
    tag = "c%d_" % k
    X, Hh = z[tag + "x"].shape[2], z[tag + "h0"].shape[1]
    m = L.GetFinalScores(X, Hh, yesno=True, no_answer=bool(z[tag + "no_answer"]), useES=bool(z[tag + "useES"])).to(device)
    for n_, p in m.named_parameters():
        p.data = T(z[tag + "w_" + n_]).to(device)
    return m


def check_module_against_golden(z, k, device, tol):
    """forward and every gradient of case k; tolerances as test_get_final_scores_vs_reference scales them from ``tol``"""
    tag = "c%d_" % k
    m = build_module(z, k, device)
    x = T(z[tag + "x"]).to(device).requires_grad_()
    h0 = T(z[tag + "h0"]).to(device).requires_grad_()
    ES = int(z[tag + "ES"]) if bool(z[tag + "useES"]) else None            # (SDNet passes None without useES)
    y = m(x, h0, T(z[tag + "mask"]).to(device), ES, mask_flag=True)
    _close(y, z[tag + "y"], tol, 1e-5, "scores")
    y.backward(T(z[tag + "gy"]).to(device))
    _close(x.grad, z[tag + "gx"], 10 * tol, 1e-4, "gx")
    _close(h0.grad, z[tag + "gh0"], 10 * tol, 1e-4, "gh0")
    nograd = set(z[tag + "nograd"].tolist())
    for n_, p in m.named_parameters():
        if n_ in nograd:
            assert p.grad is None, n_
        else:
            _close(p.grad, z[tag + "g_" + n_], 10 * tol, 1e-4, "g " + n_)


@pytest.mark.parametrize("k", [0, 1, 2])
def test_get_final_scores_yesno_cpu_vs_reference(layers_golden, k):
    """Layers.py:352-432 with yesno (and with / without useES, no_answer), mask_flag set: probabilities, gx, gh0, every parameter
    gradient, and no gradient exactly where the reference has none (the dead GRU; attn2 without useES)."""
    import ruart_amd.layers as L
    from ruart_amd import ops
    saved = L.dropout_p
    L.set_dropout_prob(0.0)
    try:
        with ops.use_trunk_mode(gemm="fp32"):
            check_module_against_golden(layers_golden, k, "cpu", 1e-6)
    finally:
        L.dropout_p = saved


@pytest.mark.parametrize("k", [0, 1, 2])
def test_get_final_scores_yesno_state_dict_keys(layers_golden, k):
    """reference checkpoints load: the same keys, in the same order"""
    assert list(build_module(layers_golden, k).state_dict().keys()) == layers_golden["c%d_keys" % k].tolist()


def test_get_final_scores_yesno_compounds_the_h0_dropout(layers_golden):
    """(sic) Layers.py:406 / :414: the no-answer head sees dropout(dropout(h0)).  With p = 0.5 in training mode, the elements of h0 that
    reach the no-answer projection are a subset of those that reach the yes/no projections, scaled 4x against 2x."""
    import ruart_amd.layers as L
    from ruart_amd import ops
    saved = (L.dropout_p, L.do_seq_dropout)
    seen = []
    m = build_module(layers_golden, 0).train()
    real = ops.linear
    try:
        L.set_dropout_prob(0.5)
        L.set_seq_dropout(True)
        ops.linear = lambda x, w, b=None, **kw: (seen.append((x.detach().clone(), w)), real(x, w, b, **kw))[1]
        torch.manual_seed(3)
        z = layers_golden
        h0 = torch.ones(3, z["c0_h0"].shape[1])
        with ops.use_trunk_mode(gemm="fp32"):
            m(T(z["c0_x"]), h0, T(z["c0_mask"]), int(z["c0_ES"]), mask_flag=True)
    finally:
        ops.linear = real
        L.dropout_p, L.do_seq_dropout = saved
    inputs = {id(w): x for x, w in seen}
    yn = [inputs[id(l.weight)] for l in (m.no_linear, m.yes_linear, m.no_read_linear)]
    na = inputs[id(m.noanswer_linear.weight)]
    assert torch.equal(yn[0], yn[1]) and torch.equal(yn[0], yn[2])                    # the three heads share one dropped h0
    assert set(yn[0].unique().tolist()) <= {0.0, 2.0} and set(na.unique().tolist()) <= {0.0, 4.0}
    assert bool(((na != 0) <= (yn[0] != 0)).all()) and 0 < int((na != 0).sum()) < int((yn[0] != 0).sum())


@pytest.mark.parametrize("variant", ["no_answer", "plain"])
def test_decode_slots_matches_reference(golden_dir, variant):
    """``trainer.decode_slots`` against the reference's own predict loop (Models/SDNetTrainer.py:396-448, yesno_num = 3) on prepared
    scores: each front slot, a real OCR item, the skipped slot len(ocr_list) - 1, the sentinel slot 3 + num_cnt - 1 (decodes to
    "<OCR>"), padding slots and the no-answer slot on top, and a row with nothing admissible."""
    from ruart_amd.trainer import decode_predictions, decode_slots
    with open(os.path.join(golden_dir, "predict_decode_yesno.json")) as f:
        z = json.load(f)
    cases, want = z["cases"], z["expected"][variant]
    width = z["n_slots"] if variant == "no_answer" else z["n_slots"] - 1
    scores = torch.tensor([c["prob"][:width] for c in cases])
    extra = [{"q_id": c["q_id"], "answers": c["answers"], "ocr_list": c["ocr_list"], "image_path": "x"} for c in cases]
    opt = {"label_yesno": True}
    if variant == "no_answer":
        opt["label_no_answer"] = True
    counts = [c["num_cnt"] for c in cases]
    anls, acc, res, save_res = decode_slots(scores, counts, extra, opt)
    assert res == want["res"]
    assert [r["idx"] for r in save_res] == [r["idx"] for r in want["save_res"]]
    for got, ref in zip(save_res, want["save_res"]):
        assert got == ref, (got, ref)
    assert abs(anls - want["ANLS"]) < 1e-9 and abs(acc - want["ACC"]) < 1e-9
    # the fixture does cover what it says: front slots, the sentinel's string, the no-answer slot
    answers = [r["prediction"] for r in want["save_res"]]
    assert {"yes", "no", "answering does not require reading text in the image", "<OCR>", "unanswerable"} <= set(answers)
    with pytest.raises(NotImplementedError):
        decode_predictions(scores, counts, extra, opt)
    with pytest.raises(NotImplementedError):
        decode_slots(scores, counts, extra, dict(opt, fixed_answers=True))


def test_synth_weights_keep_their_draw_order(golden_dir, layers_golden):
    """The six new modules' tensors come after every existing entry: a conf without the key regenerates the weights the existing
    goldens were made with (two stored tensors, and the float64 checksums sdnet_e2e.npz has carried since it was written); with the
    key the existing entries are the same arrays and twelve are new."""
    opt = default_opt(vocab_size=1500)
    base = synth.make_sdnet_weights(opt, seed=1033)
    for name in ("alphaBERT", "get_answer.attn2.linear.bias"):
        assert np.array_equal(base[name], layers_golden["synth:" + name]), name
    wsum = np.array([float(np.sum(v.astype(np.float64))) for _, v in sorted(base.items())])
    assert np.array_equal(wsum, np.load(os.path.join(golden_dir, "sdnet_e2e.npz"))["sdnet_wsum"])
    yn = synth.make_sdnet_weights(default_opt(vocab_size=1500, label_yesno=True), seed=1033)
    assert list(yn)[:len(base)] == list(base) and all(np.array_equal(yn[k], base[k]) for k in base)
    new = list(yn)[len(base):]
    assert len(new) == 12 and all(n.startswith(("get_answer.no_", "get_answer.yes_", "get_answer.no_read_")) for n in new)


def test_synthetic_batch_targets_follow_the_slot_layout():
    opt = default_opt(vocab_size=1500)
    No = opt["max_ocr_num"]
    kw = dict(seed=7, n_q=6, n_ocr=opt["ES_ocr_len"] + 4, n_od=4, bert_vocab=2000, ragged=True)
    assert synth.synthetic_batch(opt, 2, **kw)[3].shape == (2, No + 1)
    gt = synth.synthetic_batch(dict(opt, label_yesno=True), 2, **kw)[3]
    assert gt.shape == (2, 3 + No + 1) and gt.sum(1).tolist() == [1.0, 1.0] and float(gt[:, :3].sum()) == 1.0
    opt_plain = {k: v for k, v in opt.items() if k != "label_no_answer"}
    assert synth.synthetic_batch(dict(opt_plain, label_yesno=True), 2, **kw)[3].shape == (2, 3 + No)
