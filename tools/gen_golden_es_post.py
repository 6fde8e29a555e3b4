#!/usr/bin/env python3
"""Generate the ``ES_using_way post_process`` / ``no_Context_Self_Attention`` fixtures under tests/golden/ by running the UNMODIFIED
reference on the CPU.

TEST INFRASTRUCTURE ONLY - runs where the reference tree is mounted (``oracle._refshim.REF``), and nowhere else; nothing of the
reference is copied, it is imported from where it lies through ``oracle._refshim``.  The fixtures are plain arrays: seeded synthetic
inputs and the reference's outputs, gradients and masks for them.

    python tools/gen_golden_es_post.py            # all four files
    python tools/gen_golden_es_post.py e2e        # one of: e2e | masks

  sdnet_e2e_es_post.npz        SDNet.forward + loss + backward with ES_using_way post_process, sizes / seeds / content as
                               sdnet_e2e_yesno.npz (B = 2, ragged, n_ocr 100, n_od 30): scores, loss, gt, counts, gradient names and
                               norms, gradients of tensors up to 4096 elements, the state-dict key list; plus ``b2_*``: a forward-only
                               second batch with 6 items per sample (fewer than ES_ocr_len) and a few ``synth:`` tensors of the conf
                               WITHOUT the keys (the draw order of the synthetic weights)
  sdnet_e2e_noctx.npz          the same with no_Context_Self_Attention
  sdnet_e2e_es_post_noctx.npz  the same with both keys
  es_post_masks.npz            per item count in CNTS (one sample each): the key mask ES_ocr_att receives, the mask get_answer
                               receives, the positions position_attn receives (forward pre-hooks), and which slots of ES_linear's and of
                               context_rnn's input hold an item (a non-zero row)
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

SEED, BATCH_SEED, SMALL_SEED, MASK_SEED = 1033, 7, 11, 13
CONFS = {"sdnet_e2e_es_post": dict(ES_using_way="post_process"),
         "sdnet_e2e_noctx": dict(no_Context_Self_Attention=True),
         "sdnet_e2e_es_post_noctx": dict(ES_using_way="post_process", no_Context_Self_Attention=True)}
CNTS = (3, 6, 11, 12, 40, 100)          # below ES_ocr_len (the kept quirk), just above it (one and two live keys), mid, full
SYNTH_NAMES = ("alphaBERT", "high_lvl_context_rnn.rnns.0.weight_ih_l0", "highlvl_self_att.scoring.linear.weight",
               "get_answer.attn2.linear.bias")


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def save(name, **arrays):
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **arrays)
    print("wrote %s (%.1f KB, %d arrays)" % (path, os.path.getsize(path) / 1024, len(arrays)))


def reference_net(bert_dir, **keys):
    from Models.SDNet import SDNet
    import Models.Layers as L
    opt = default_opt(vocab_size=1500, **keys)
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


def gen_e2e(bert_dir):
    base = synth.make_sdnet_weights(default_opt(vocab_size=1500), seed=SEED)
    for name, keys in CONFS.items():
        net, opt = reference_net(bert_dir, **keys)
        B = 2
        q, ocr, od, gt, _ = synth.synthetic_batch(opt, B, seed=BATCH_SEED, n_q=30, n_ocr=100, n_od=30, bert_vocab=2000, ragged=True)
        counts = list(ocr["num_cnt"])
        scores, _ = net(q, ocr, od)
        assert scores.shape == (B, opt["max_ocr_num"] + 1) and torch.allclose(scores.sum(1), torch.ones(B), atol=1e-5)
        loss = torch.nn.functional.binary_cross_entropy_with_logits(scores, gt) * gt.size(1)
        loss.backward()
        arrays = dict(seed=np.array(SEED), batch_seed=np.array(BATCH_SEED), B=np.array(B), vocab_size=np.array(1500),
                      scores=scores.detach().numpy(), loss=np.array(loss.item()), gt=gt.numpy(),
                      ocr_num_cnt=np.array(counts), od_num_cnt=np.array(od["num_cnt"]),
                      keys=np.array([k for k in net.state_dict().keys() if not k.startswith("Bert.")]))
        names, norms = [], []
        for n_, p in net.named_parameters():
            if n_.startswith("Bert."):
                continue
            names.append(n_)
            norms.append(-1.0 if p.grad is None else float(p.grad.double().norm()))
            if p.grad is not None and p.numel() <= 4096:
                arrays["grad:" + n_] = p.grad.numpy().copy()
        arrays["grad_names"] = np.array(names)
        arrays["grad_norms"] = np.array(norms)
        print(name, "scores", tuple(scores.shape), "loss %.6f" % loss.item(), "counts", counts,
              "no gradient:", [n for n, v in zip(names, norms) if v < 0])
        if name == "sdnet_e2e_es_post":
            # forward only, every sample with fewer items than ES_ocr_len: the trunk's slots are empty and the first cnt of them stay live
            q, ocr, od, _, _ = synth.synthetic_batch(opt, B, seed=SMALL_SEED, n_q=30, n_ocr=6, n_od=30, bert_vocab=2000, ragged=False)
            with torch.no_grad():
                s2, _ = net(q, ocr, od)
            arrays.update(b2_seed=np.array(SMALL_SEED), b2_scores=s2.numpy(), b2_ocr_num_cnt=np.array(ocr["num_cnt"]))
            for n_ in SYNTH_NAMES:       # tensors of the conf WITHOUT the keys (the first two rows of the matrices): the existing
                arrays["synth:" + n_] = base[n_][:2] if base[n_].ndim == 2 else base[n_]      # entries' draw order must not move
        save(name, **arrays)


def gen_masks(bert_dir):
    net, opt = reference_net(bert_dir, ES_using_way="post_process")
    cap = {}
    net.ES_ocr_att.register_forward_pre_hook(lambda m, a: cap.__setitem__("att_mask", a[2].numpy().copy()))
    net.get_answer.register_forward_pre_hook(lambda m, a: cap.__setitem__("score_mask", a[2].numpy().copy()))
    net.position_attn.register_forward_pre_hook(lambda m, a: cap.__setitem__("pos", a[0].numpy().copy()))
    net.ES_linear.register_forward_pre_hook(lambda m, a: cap.__setitem__("es_live", (a[0].abs().sum(-1) > 0).numpy()))

    def first_context_input(m, a):       # context_rnn runs on the OCR slots first (Models/SDNet.py:338): keep the first call's input
        if "trunk_live" not in cap:
            cap["trunk_live"] = (a[0].abs().sum(-1) > 0).numpy()
    net.context_rnn.register_forward_pre_hook(first_context_input)
    out = {"cnts": np.array(CNTS), "E": np.array(opt["ES_ocr_len"]), "seed": np.array(MASK_SEED)}
    for cnt in CNTS:
        q, ocr, od, _, _ = synth.synthetic_batch(opt, 1, seed=MASK_SEED, n_q=8, n_ocr=cnt, n_od=3, bert_vocab=2000, ragged=False)
        pos_before = ocr["position"].clone()
        cap.clear()
        with torch.no_grad():
            net(q, ocr, od)
        assert ocr["num_cnt"] == [cnt] and torch.equal(cap_t(cap["pos"]), pos_before[:, opt["ES_ocr_len"]:])
        for k, v in cap.items():
            out["c%d_%s" % (cnt, k)] = v.astype(np.float32 if k == "pos" else np.uint8)
        print("cnt %3d: attention mask %s sum %d, scorer mask %s sum %d, ES slots live %d, trunk slots live %d"
              % (cnt, cap["att_mask"].shape, cap["att_mask"].sum(), cap["score_mask"].shape, cap["score_mask"].sum(),
                 cap["es_live"].sum(), cap["trunk_live"].sum()))
    save("es_post_masks", **out)


def cap_t(a):
    return torch.from_numpy(a)


if __name__ == "__main__":
    which = sys.argv[1:] or ["e2e", "masks"]
    cfg = synth.bert_config(vocab_size=2000)
    bert_dir = _refshim.write_bert_dir(cfg, synth.make_bert_weights(cfg, seed=SEED))
    try:
        for w in which:
            {"e2e": gen_e2e, "masks": gen_masks}[w](bert_dir)
    finally:
        shutil.rmtree(bert_dir, ignore_errors=True)
