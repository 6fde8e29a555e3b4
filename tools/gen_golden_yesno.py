#!/usr/bin/env python3
"""Generate the ``label_yesno`` fixtures under tests/golden/ by running the UNMODIFIED reference on the CPU.

TEST INFRASTRUCTURE ONLY - runs where the reference tree is mounted (``oracle._refshim.REF``), and nowhere else; nothing of the
reference is copied, it is imported from where it lies through ``oracle._refshim``.  The fixtures are plain arrays / JSON: seeded
synthetic inputs and the reference's outputs and gradients for them.

    python tools/gen_golden_yesno.py            # all three
    python tools/gen_golden_yesno.py layers     # one of: layers | e2e | predict

  yesno_layers.npz           GetFinalScores(yesno=True) (Models/Layers.py:352-432): output, every gradient, the names without one and the
                             state-dict key list, dropout 0, mask_flag set, three cases (see CASES)
  sdnet_e2e_yesno.npz        SDNet.forward + loss + backward with opt['label_yesno'] as oracle/gen_golden.py's gen_e2e runs it (same
                             sizes; the intermediate captures, which no yes/no test reads, are left out to keep the file small)
  predict_decode_yesno.json  the reference's predict loop (Models/SDNetTrainer.py:378-451) on prepared scores, with and without
                             label_no_answer
"""
import json
import os
import sys
import types

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

# (B, L, X, Hh, ES, useES, no_answer): more than one sample with an odd L; a feature width past one 256-float lane trip without
# useES / no_answer; one float4 per row with a single sample
CASES = [(3, 13, 12, 7, 4, True, True), (2, 9, 260, 5, 0, False, False), (1, 5, 4, 3, 2, True, True)]


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def save(name, **arrays):
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **arrays)
    print("wrote %s (%.1f KB, %d arrays)" % (path, os.path.getsize(path) / 1024, len(arrays)))


def gen_layers():
    import Models.Layers as L
    L.set_dropout_prob(0.0)
    L.set_seq_dropout(True)
    g = np.random.default_rng(29)
    out = {"n_cases": np.array(len(CASES))}
    for k, (B, Ln, X, Hh, ES, useES, no_answer) in enumerate(CASES):
        tag = "c%d_" % k
        m = L.GetFinalScores(X, Hh, yesno=True, no_answer=no_answer, useES=useES)
        for n_, p in m.named_parameters():
            a = g.uniform(-0.4, 0.4, tuple(p.shape)).astype(np.float32)
            p.data = T(a)
            out[tag + "w_" + n_] = a
        x = T(g.standard_normal((B, Ln, X)).astype(np.float32)).requires_grad_()
        h0 = T(g.standard_normal((B, Hh)).astype(np.float32)).requires_grad_()
        mask = np.ones((B, Ln), dtype=np.uint8)
        for b in range(B):                       # a ragged masked tail
            mask[b, Ln - 1 - (b % 3) - (1 if B == 1 else 0) + 1:] = 0
        if useES:
            mask[B - 1, 1] = 0                   # one masked slot inside the ES range
        y = m(x, h0, T(mask), ES, mask_flag=True)
        assert torch.allclose(y.sum(1), torch.ones(B), atol=1e-5) and y.shape == (B, 3 + Ln + int(no_answer))
        gy = T(g.standard_normal(tuple(y.shape)).astype(np.float32))
        y.backward(gy)
        out.update({tag + "x": x.detach().numpy(), tag + "h0": h0.detach().numpy(), tag + "mask": mask, tag + "ES": np.array(ES),
                    tag + "useES": np.array(useES), tag + "no_answer": np.array(no_answer), tag + "y": y.detach().numpy(),
                    tag + "gy": gy.numpy(), tag + "gx": x.grad.numpy(), tag + "gh0": h0.grad.numpy()})
        for n_, p in m.named_parameters():
            if p.grad is not None:
                out[tag + "g_" + n_] = p.grad.numpy()
        out[tag + "nograd"] = np.array([n_ for n_, p in m.named_parameters() if p.grad is None])
        out[tag + "keys"] = np.array(list(m.state_dict().keys()))
        print(tag, "mask", mask.tolist(), "nograd", out[tag + "nograd"].tolist())
    # two tensors of the synthetic SDNet weights of a conf WITHOUT the key: the draw order of the existing entries must not move
    sw = synth.make_sdnet_weights(default_opt(vocab_size=1500), seed=1033)
    for name in ("alphaBERT", "get_answer.attn2.linear.bias"):
        out["synth:" + name] = sw[name]
    save("yesno_layers", **out)


def gen_e2e():
    from Models.SDNet import SDNet
    import Models.Layers as L
    opt = default_opt(vocab_size=1500, label_yesno=True)
    bert_cfg = synth.bert_config(vocab_size=2000)
    seed = 1033
    bw = synth.make_bert_weights(bert_cfg, seed=seed)
    opt["BERT_model_file"] = _refshim.write_bert_dir(bert_cfg, bw)
    opt["datadir"] = ""
    sw = synth.make_sdnet_weights(opt, seed=seed)
    net = SDNet(opt, {"glove_embedding": T(sw["glove_embed.weight"]).clone(), "fast_embedding": T(sw["fast_embed.weight"]).clone()})
    missing, unexpected = net.load_state_dict({k: T(v) for k, v in sw.items()}, strict=False)
    assert not unexpected and all(k.startswith("Bert.") for k in missing), (missing, unexpected)
    B = 2
    q, ocr, od, gt, _ = synth.synthetic_batch(opt, B, seed=7, n_q=30, n_ocr=100, n_od=30, bert_vocab=2000, ragged=True)
    assert gt.shape[1] == 3 + opt["max_ocr_num"] + 1 and float(gt[:, :3].sum()) >= 1.0      # mass on a yes/no slot
    L.set_dropout_prob(0.0)          # dropout off everywhere, the encoder in eval mode (gen_e2e)
    net.train()
    net.Bert.bert_model.eval()
    net.drop_emb = False
    scores, _ = net(q, ocr, od)
    loss = torch.nn.functional.binary_cross_entropy_with_logits(scores, gt) * gt.size(1)
    loss.backward()
    arrays = dict(seed=np.array(seed), batch_seed=np.array(7), B=np.array(B), vocab_size=np.array(1500),
                  scores=scores.detach().numpy(), loss=np.array(loss.item()), gt=gt.numpy(),
                  ocr_num_cnt=np.array(ocr["num_cnt"]), od_num_cnt=np.array(od["num_cnt"]))
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
    print("scores", tuple(scores.shape), "loss %.6f" % loss.item(), "no gradient:", [n for n, v in zip(names, norms) if v < 0])
    save("sdnet_e2e_yesno", **arrays)


def predict_cases(seed=5):
    """Score rows for the decode with three front slots: one case per slot kind on top, one with nothing admissible, random ones."""
    g = np.random.default_rng(seed)
    n_ocr_slots = 12
    n_slots = 3 + n_ocr_slots + 1                 # front slots, max_ocr_num, no-answer
    words = ["stop", "exit", "coca cola", "north", "bus", "2nd", "cafe", "park", "shop", "street", "sign", "yes", "no"]
    cases = []

    def case(n, top, answers, low=None):
        """n items incl. the trailing sentinel; ``top``: slots put on top, highest first"""
        ocr = [words[int(k)] for k in g.integers(0, len(words), size=n - 1)] + ["<OCR>"]
        p = g.random(n_slots).astype(np.float32)
        for r, idx in enumerate(top):
            p[idx] = 3.0 - 0.25 * r
        ans = {"first": [ocr[0]], "ten": (ocr * 10)[:10], "yes": ["yes", "Yes", "yes"], "none": None, "zzz": ["zzz"],
               "noread": ["answering does not require reading text in the image"]}[answers]
        cases.append({"prob": p.tolist(), "num_cnt": n, "ocr_list": ocr, "answers": ans, "q_id": 700 + len(cases)})

    case(6, [0], "noread")                         # each of the three front slots
    case(6, [1], "yes")
    case(6, [2], "yes")
    case(7, [3], "first")                          # a real OCR item
    case(7, [3 + 4], "ten")
    case(7, [7 - 1, 3], "first")                   # the skipped slot len(ocr_list) - 1 (a real OCR item), then a real one
    case(3, [3 - 1, 1], "yes")                     # the skipped slot is the front slot "no"
    case(5, [3 + 5 - 1], "zzz")                    # the sentinel slot 3 + num_cnt - 1: admissible, decodes to "<OCR>"
    case(5, [3 + 5, 3 + 1], "first")               # a padding slot, then a real item
    case(5, [3 + 9, 3 + 5, 0], "noread")           # two padding slots, then a front slot
    case(6, [n_slots - 1, 3], "first")             # the no-answer slot (without label_no_answer the column is cut off)
    case(6, [6 - 1, n_slots - 1, 4], "none")       # skipped, then no-answer
    # nothing admissible (without label_no_answer): the front slots are admissible for every num_cnt >= 0, so only a count that cancels
    # them (3 + num_cnt = 0; no dataset produces it) makes the walk run out and leaves it with the lowest-scored slot
    p = g.random(n_slots).astype(np.float32)
    cases.append({"prob": p.tolist(), "num_cnt": -3, "ocr_list": ["<OCR>"], "answers": ["zzz"], "q_id": 700 + len(cases)})
    for i in range(8):                             # random rows
        case([1, 2, 5, 12, 7, 3, 9, 4][i], [], ["none", "first", "ten", "yes", "zzz"][i % 5])
    return cases, n_slots


def gen_predict():
    import Models.SDNetTrainer as M
    cases, n_slots = predict_cases()
    out = {"cases": cases, "n_slots": n_slots, "expected": {}}
    for name, no_answer in (("no_answer", True), ("plain", False)):
        width = n_slots if no_answer else n_slots - 1
        scores = torch.tensor([c["prob"][:width] for c in cases])
        opt = {"label_yesno": True}
        if no_answer:
            opt["label_no_answer"] = True

        class Net:
            drop_emb = False

            def eval(self):
                pass

            def __call__(self, q, ocr, od):
                return scores, None

        fake = types.SimpleNamespace(network=Net(), opt=opt, fixed_answers_len=0, fixed_answers_entry=None,
                                     loss_func=lambda s, g: torch.zeros(()))
        batch = (None, {"num_cnt": [c["num_cnt"] for c in cases]}, None, torch.zeros(len(cases), width),
                 [{"q_id": c["q_id"], "answers": c["answers"], "ocr_list": c["ocr_list"], "image_path": "x"} for c in cases])
        loss, anls, acc, res, save_res = M.SDNetTrainer.predict(fake, batch)
        out["expected"][name] = {"ANLS": float(anls), "ACC": float(acc), "res": res, "save_res": save_res}
        print(name, "ANLS %.4f ACC %.4f" % (anls, acc), [(r["idx"], r["prediction"]) for r in save_res])
    path = os.path.join(OUT, "predict_decode_yesno.json")
    with open(path, "w") as f:
        json.dump(out, f)
    print("wrote", path, os.path.getsize(path) // 1024, "KB")


if __name__ == "__main__":
    which = sys.argv[1:] or ["layers", "e2e", "predict"]
    for w in which:
        {"layers": gen_layers, "e2e": gen_e2e, "predict": gen_predict}[w]()
