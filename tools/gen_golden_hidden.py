#!/usr/bin/env python3
"""Generate the wide-hidden-size fixture under tests/golden/ by running the UNMODIFIED reference on the CPU.

TEST INFRASTRUCTURE ONLY - runs where the reference tree is mounted (``oracle._refshim.REF``), and nowhere else; nothing of the
reference is copied, it is imported from where it lies through ``oracle._refshim``.  The fixture is plain arrays: seeded synthetic
inputs and the reference's outputs and gradients for them.

    python tools/gen_golden_hidden.py

  sdnet_e2e_hidden144.npz   SDNet.forward + loss + backward with hidden_size = highlvl_hidden_size = 144 - the smallest width above the
                            register-resident LSTM kernels' 128 that is a multiple of 16 and not of 32 (a half-used last k-step of the
                            streamed kernels) -, sizes / seeds / content as sdnet_e2e_noctx.npz (B = 2, ragged, n_ocr 100, n_od 30):
                            scores, loss, gt, counts, gradient names and norms, gradients of tensors up to 4096 elements, the
                            state-dict key list
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

SEED, BATCH_SEED = 1033, 7
NAME, KEYS = "sdnet_e2e_hidden144", dict(hidden_size=144, highlvl_hidden_size=144)


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a))


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


def gen(bert_dir):
    net, opt = reference_net(bert_dir, **KEYS)
    assert net.context_rnn.rnns[0].hidden_size == 144 and net.high_lvl_context_rnn.rnns[0].hidden_size == 144
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
    print(NAME, "scores", tuple(scores.shape), "loss %.6f" % loss.item(), "counts", counts,
          "no gradient:", [n for n, v in zip(names, norms) if v < 0])
    path = os.path.join(OUT, NAME + ".npz")
    np.savez_compressed(path, **arrays)
    print("wrote %s (%.1f KB, %d arrays)" % (path, os.path.getsize(path) / 1024, len(arrays)))


if __name__ == "__main__":
    cfg = synth.bert_config(vocab_size=2000)
    bert_dir = _refshim.write_bert_dir(cfg, synth.make_bert_weights(cfg, seed=SEED))
    try:
        gen(bert_dir)
    finally:
        shutil.rmtree(bert_dir, ignore_errors=True)
