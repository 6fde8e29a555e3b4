#!/usr/bin/env python3
"""Generate the fixtures of the confs ``multi2one_bidir``, ``no_DeepAttention`` and last-layer BERT (a conf without
``BERT_LINEAR_COMBINE``) under tests/golden/ by running the UNMODIFIED reference on the CPU.

TEST INFRASTRUCTURE ONLY - runs where the reference tree is mounted (``oracle._refshim.REF``), and nowhere else; nothing of the
reference is copied, it is imported from where it lies through ``oracle._refshim``.  The fixtures are plain arrays: seeded synthetic
inputs and the reference's outputs and gradients for them.

    python tools/gen_golden_conf_rest.py                 # all four files
    python tools/gen_golden_conf_rest.py sdnet_e2e_nodeep  # some of them
    python tools/gen_golden_conf_rest.py bidir_alone       # shows that the reference cannot run multi2one_bidir with the deep attention

  sdnet_e2e_bidir_nodeep.npz, sdnet_e2e_nodeep.npz, sdnet_e2e_lastlayer.npz, sdnet_e2e_bidir_nodeep_lastlayer.npz
      SDNet.forward + loss + backward, dropout off, sizes and seeds as sdnet_e2e_yesno.npz (B = 2, ragged, n_ocr 100, n_od 30), with a
      few items rewritten to other word counts (``conf_rest_batch``: OCR items of 1 word, of max_ocr_len words - no pad step - and in
      between, in both samples; an object item of max_od_len words; the second sample holds fewer items than the first): scores, loss,
      gt, counts, the rewritten items' word counts, gradient names and norms, gradients of tensors up to 4096 elements - and rows 0
      and 1 of the word, POS and entity tables' gradients (row 0 is the pad id: the reverse direction of a bidirectional multi2one
      feeds it) -, the state-dict key list.
"""
import os
import shutil
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
from oracle import _refshim  # noqa: E402

_refshim.install()
from ruart_amd import synth  # noqa: E402
from ruart_amd.arguments import default_opt  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
torch.set_num_threads(8)

SEED, BATCH_SEED, LEN_SEED = 1033, 7, 19
# fixture name -> (conf keys set, conf keys removed)
# (multi2one_bidir WITHOUT no_DeepAttention cannot run in the reference: Models/Layers.py:227 fails on the question side's 800-wide rows,
# the levels' matrices being built for the item side's 1100 - ``bidir_alone_fails`` shows it)
CONFS = {"sdnet_e2e_bidir_nodeep": (dict(multi2one_bidir=True, no_DeepAttention=True), ()),
         "sdnet_e2e_nodeep": (dict(no_DeepAttention=True), ()),
         "sdnet_e2e_lastlayer": ({}, ("BERT_LINEAR_COMBINE",)),
         "sdnet_e2e_bidir_nodeep_lastlayer": (dict(multi2one_bidir=True, no_DeepAttention=True), ("BERT_LINEAR_COMBINE",))}
# rewritten items, rows counted over the batch (sample 0 holds OCR rows 0 .. 99 and object rows 0 .. 29): row -> words
OCR_LENGTHS = {0: 20, 1: 1, 2: 11, 7: 19, 40: 2, 98: 20, 101: 20, 103: 7, 104: 1}
OD_LENGTHS = {0: 10, 2: 6, 31: 10, 33: 1}
ROW0_TABLES = ("fast_embed.weight", "pos_embedding.weight", "ent_embedding.weight")


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def conf_opt(set_keys, drop_keys, **extra):
    opt = default_opt(vocab_size=1500, **set_keys, **extra)
    for k in drop_keys:
        del opt[k]
    return opt


def conf_rest_batch(opt, B=2):
    q, ocr, od, gt, extra = synth.synthetic_batch(opt, B, seed=BATCH_SEED, n_q=30, n_ocr=100, n_od=30, bert_vocab=2000, ragged=True)
    synth.set_item_lengths(opt, ocr, OCR_LENGTHS, seed=LEN_SEED, bert_vocab=2000, group="ocr")
    synth.set_item_lengths(opt, od, OD_LENGTHS, seed=LEN_SEED + 1, bert_vocab=2000, group="od")
    return q, ocr, od, gt, extra


def reference_net(bert_dir, set_keys, drop_keys):
    from Models.SDNet import SDNet
    import Models.Layers as L
    opt = conf_opt(set_keys, drop_keys)
    opt["BERT_model_file"], opt["datadir"] = bert_dir, ""
    sw = synth.make_sdnet_weights(opt, seed=SEED)
    net = SDNet(opt, {"glove_embedding": T(sw["glove_embed.weight"]).clone(), "fast_embedding": T(sw["fast_embed.weight"]).clone()})
    missing, unexpected = net.load_state_dict({k: T(v) for k, v in sw.items()}, strict=False)
    assert not unexpected and all(k.startswith("Bert.") for k in missing), (missing, unexpected)
    L.set_dropout_prob(0.0)          # dropout off everywhere, the encoder in eval mode (oracle/gen_golden.py gen_e2e)
    net.train()
    net.Bert.bert_model.eval()
    net.drop_emb = False
    return net, opt


def gen(name, bert_dir):
    set_keys, drop_keys = CONFS[name]
    net, opt = reference_net(bert_dir, set_keys, drop_keys)
    B = 2
    q, ocr, od, gt, _ = conf_rest_batch(opt, B)
    counts = list(ocr["num_cnt"])
    assert counts[1] < counts[0] and od["num_cnt"][1] < od["num_cnt"][0]
    flat = lambda d: np.array([l for s_ in d["len_cnt"] for l in s_])
    assert flat(ocr).max() == opt["max_ocr_len"] and flat(ocr).min() == 1 and flat(od).max() == opt["max_od_len"]
    scores, _ = net(q, ocr, od)
    assert scores.shape == (B, opt["max_ocr_num"] + 1) and torch.allclose(scores.sum(1), torch.ones(B), atol=1e-5)
    loss = torch.nn.functional.binary_cross_entropy_with_logits(scores, gt) * gt.size(1)
    loss.backward()
    arrays = dict(seed=np.array(SEED), batch_seed=np.array(BATCH_SEED), len_seed=np.array(LEN_SEED), B=np.array(B),
                  vocab_size=np.array(1500), scores=scores.detach().numpy(), loss=np.array(loss.item()), gt=gt.numpy(),
                  ocr_num_cnt=np.array(counts), od_num_cnt=np.array(od["num_cnt"]), ocr_len_cnt=flat(ocr), od_len_cnt=flat(od),
                  ocr_lengths=np.array(sorted(OCR_LENGTHS.items())), od_lengths=np.array(sorted(OD_LENGTHS.items())),
                  keys=np.array([k for k in net.state_dict().keys() if not k.startswith("Bert.")]))
    names, norms = [], []
    for n_, p in net.named_parameters():
        if n_.startswith("Bert."):
            continue
        names.append(n_)
        norms.append(-1.0 if p.grad is None else float(p.grad.double().norm()))
        if p.grad is not None and p.numel() <= 4096:
            arrays["grad:" + n_] = p.grad.numpy().copy()
        if p.grad is not None and n_ in ROW0_TABLES:
            arrays["grad_rows01:" + n_] = p.grad[:2].numpy().copy()
    arrays["grad_names"] = np.array(names)
    arrays["grad_norms"] = np.array(norms)
    print(name, "scores", tuple(scores.shape), "loss %.6f" % loss.item(), "counts", counts, od["num_cnt"],
          "no gradient:", [n for n, v in zip(names, norms) if v < 0],
          "row 0 gradient norms:", {n_: float(np.linalg.norm(arrays["grad_rows01:" + n_][0])) for n_ in ROW0_TABLES
                                    if "grad_rows01:" + n_ in arrays})
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **arrays)
    print("wrote %s (%.1f KB, %d arrays)" % (path, os.path.getsize(path) / 1024, len(arrays)))


def bidir_alone_fails(bert_dir):
    net, opt = reference_net(bert_dir, dict(multi2one_bidir=True), ())
    q, ocr, od, _, _ = conf_rest_batch(opt, 2)
    try:
        with torch.no_grad():
            net(q, ocr, od)
    except RuntimeError as e:
        print("multi2one_bidir with the deep attention: the reference raises %s: %s" % (type(e).__name__, e))
        return
    raise AssertionError("the reference ran multi2one_bidir with the deep attention")


if __name__ == "__main__":
    which = sys.argv[1:] or list(CONFS)
    cfg = synth.bert_config(vocab_size=2000)
    bert_dir = _refshim.write_bert_dir(cfg, synth.make_bert_weights(cfg, seed=SEED))
    try:
        for w in which:
            bidir_alone_fails(bert_dir) if w == "bidir_alone" else gen(w, bert_dir)
    finally:
        shutil.rmtree(bert_dir, ignore_errors=True)
