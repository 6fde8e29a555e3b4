#!/usr/bin/env python3
"""Generate the region-image-feature fixtures (conf keys ``img_feature``, ``img_fea_way replace_od``, ``img_feature_replace_od``) under
tests/golden/ by running the UNMODIFIED reference on the CPU.

TEST INFRASTRUCTURE ONLY - runs where the reference tree is mounted (``oracle._refshim.REF``), and nowhere else; nothing of the
reference is copied, it is imported from where it lies through ``oracle._refshim``.  The fixtures are plain arrays: seeds of the
synthetic inputs (never the inputs themselves) and the reference's outputs and gradients for them.

    python tools/gen_golden_img_feature.py            # all three files
    python tools/gen_golden_img_feature.py e2e        # one of: e2e | dataset

  sdnet_e2e_img_overlay.npz  SDNet.forward + loss + backward with img_feature / replace_od (the object items' states written over the
                             first rows of the projected features): B = 2, ragged, n_ocr 100, max_od_num 36, object counts (5, 4), so
                             at least 31 of the 36 rows of each sample are image rows.  Scores, loss, gt, counts, gradient names and
                             norms, gradients of tensors up to 4096 elements, two slices of img_fea2od.weight's gradient, the state-dict
                             key list, ``synth:`` tensors of the conf WITHOUT the keys; ``b2_*``: a forward-only second batch with object
                             counts (36, 1) - sample 0 has no image row left; ``swap_scores``: the first batch with the two samples'
                             features and boxes exchanged
  sdnet_e2e_img_pure.npz     the same with img_feature_replace_od (the object items contribute nothing), plus ``od2_scores``: the first
                             batch with another object list (counts 36, 32)
  img_feature_dataset.npz    VQA_Dataset.get_image_feature for synth.synthetic_region_records: the folder path (files written to a
                             temporary folder, train and test mode) and the table path

The generator ASSERTS that the fixtures can tell the feature from its absence: the swapped features move the scores by at least 1e-2
(50 times the loosest score bound of the tests), zeroed features by at least 0.1, and od2_scores is bit-equal to scores in the pure
form.  A failing assert means other seeds, never another bound.
"""
import os
import shutil
import sys
import tempfile

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

SEED, BATCH_SEED, FEA_SEED, B2_SEED, B2_FEA_SEED, REC_SEED = 1033, 7, 3, 11, 5, 3
IMG_KEYS = dict(img_feature=True, img_fea_way="replace_od", img_fea_num=36, img_fea_dim=2048, img_spa_dim=8, max_od_num=36)
CONFS = {"sdnet_e2e_img_overlay": dict(IMG_KEYS), "sdnet_e2e_img_pure": dict(IMG_KEYS, img_feature_replace_od=True)}
OD_COUNTS, B2_OD_COUNTS, OD2_COUNTS = (5, 4), (36, 1), (36, 32)
SYNTH_NAMES = ("alphaBERT", "ques_merger.linear.weight", "get_answer.noanswer_linear.weight", "get_answer.attn2.linear.bias")
MAX_KB = 200


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def save(name, **arrays):
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **arrays)
    kb = os.path.getsize(path) / 1024
    print("wrote %s (%.1f KB, %d arrays)" % (path, kb, len(arrays)))
    assert kb <= MAX_KB, "%s: %.1f KB" % (name, kb)


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


def with_features(q, fea, spa):
    q = dict(q)
    q["img_features"], q["img_spatials"] = fea, spa
    return q


def forward(net, q, ocr, od):
    with torch.no_grad():
        return net(q, ocr, od)[0].numpy().copy()


def gen_e2e(bert_dir):
    base = synth.make_sdnet_weights(default_opt(vocab_size=1500), seed=SEED)
    for name, keys in CONFS.items():
        net, opt = reference_net(bert_dir, **keys)
        B = 2
        q, ocr, _, gt, _ = synth.synthetic_batch(opt, B, seed=BATCH_SEED, n_q=30, n_ocr=100, n_od=5, bert_vocab=2000, ragged=True)
        od, od_seed = synth.synthetic_objects(opt, OD_COUNTS, seed=BATCH_SEED, bert_vocab=2000)
        fea, spa = synth.synthetic_image_features(opt, B, seed=FEA_SEED)
        q = with_features(q, fea, spa)
        scores, _ = net(q, ocr, od)
        assert scores.shape == (B, opt["max_ocr_num"] + 1) and torch.allclose(scores.sum(1), torch.ones(B), atol=1e-5)
        loss = torch.nn.functional.binary_cross_entropy_with_logits(scores, gt) * gt.size(1)
        loss.backward()
        arrays = dict(seed=np.array(SEED), batch_seed=np.array(BATCH_SEED), fea_seed=np.array(FEA_SEED), od_seed=np.array(od_seed),
                      B=np.array(B), vocab_size=np.array(1500), scores=scores.detach().numpy(), loss=np.array(loss.item()), gt=gt.numpy(),
                      ocr_num_cnt=np.array(ocr["num_cnt"]), od_num_cnt=np.array(od["num_cnt"]),
                      keys=np.array([k for k in net.state_dict().keys() if not k.startswith("Bert.")]))
        names, norms = [], []
        for n_, p in net.named_parameters():
            if n_.startswith("Bert."):
                continue
            names.append(n_)
            norms.append(-1.0 if p.grad is None else float(p.grad.double().norm()))
            if p.grad is not None and p.numel() <= 4096:
                arrays["grad:" + n_] = p.grad.numpy().copy()
        gw = net.img_fea2od.weight.grad.numpy()
        arrays["gradrows:img_fea2od.weight"] = gw[:4, :].copy()
        arrays["gradcols:img_fea2od.weight"] = gw[:, :8].copy()
        arrays["grad_names"] = np.array(names)
        arrays["grad_norms"] = np.array(norms)
        print(name, "scores", tuple(scores.shape), "loss %.6f" % loss.item(), "ocr counts", ocr["num_cnt"], "object counts", od["num_cnt"],
              "no gradient:", [n for n, v in zip(names, norms) if v < 0])
        s0 = arrays["scores"]
        # negative controls: the two samples' features exchanged; the features zeroed
        swap = forward(net, with_features(q, fea.flip(0).contiguous(), spa.flip(0).contiguous()), ocr, od)
        zero = forward(net, with_features(q, torch.zeros_like(fea), spa), ocr, od)
        d_swap, d_zero = float(np.abs(swap - s0).max()), float(np.abs(zero - s0).max())
        print(name, "max |swap_scores - scores| %.3e, zeroed features %.3e" % (d_swap, d_zero))
        assert d_swap >= 1e-2, d_swap
        assert d_zero >= 0.1, d_zero
        arrays.update(swap_scores=swap, zero_delta=np.array(d_zero))
        if "img_feature_replace_od" in keys:
            od2, od2_seed = synth.synthetic_objects(opt, OD2_COUNTS, seed=BATCH_SEED, bert_vocab=2000)
            # (with autograd recording, as ``scores`` was: the reference's CPU forward differs by 1e-6 between the two modes)
            s_od2 = net(q, ocr, od2)[0].detach().numpy().copy()
            assert np.array_equal(s_od2, s0), float(np.abs(s_od2 - s0).max())
            arrays.update(od2_scores=s_od2, od2_seed=np.array(od2_seed), od2_num_cnt=np.array(od2["num_cnt"]))
        # forward only: sample 0 full of object items (no image row left in the overlay form), sample 1 with the sentinel alone
        q2, ocr2, _, _, _ = synth.synthetic_batch(opt, B, seed=B2_SEED, n_q=30, n_ocr=100, n_od=5, bert_vocab=2000, ragged=True)
        od_b2, b2_od_seed = synth.synthetic_objects(opt, B2_OD_COUNTS, seed=B2_SEED, bert_vocab=2000)
        fea2, spa2 = synth.synthetic_image_features(opt, B, seed=B2_FEA_SEED)
        s2 = forward(net, with_features(q2, fea2, spa2), ocr2, od_b2)
        arrays.update(b2_seed=np.array(B2_SEED), b2_fea_seed=np.array(B2_FEA_SEED), b2_od_seed=np.array(b2_od_seed), b2_scores=s2,
                      b2_ocr_num_cnt=np.array(ocr2["num_cnt"]), b2_od_num_cnt=np.array(od_b2["num_cnt"]))
        for n_ in SYNTH_NAMES:       # tensors of the conf WITHOUT the keys (the first two rows of the matrices): the existing
            arrays["synth:" + n_] = base[n_][:2] if base[n_].ndim == 2 else base[n_]      # entries' draw order must not move
        save(name, **arrays)


def gen_dataset(_bert_dir=None):
    from Utils.VQA_Dataset import VQA_Dataset
    recs = synth.synthetic_region_records(seed=REC_SEED)
    opt = {k: v for k, v in default_opt(img_feature=True).items() if k != "BERT"}
    out = {"rec_seed": np.array(REC_SEED), "paths": np.array([r["path"] for r in recs])}
    folder = tempfile.mkdtemp(prefix="ruart_imgfea_")
    try:
        opt["img_fea_folder"] = folder
        for split in ("train", "test"):
            for r in recs[:2]:
                name = "".join(r["path"].split(".")[:-1])            # the reader's own rule (Utils/VQA_Dataset.py:177)
                os.makedirs(os.path.dirname(os.path.join(folder, split, name)), exist_ok=True)
                np.save(os.path.join(folder, split, name + ".npy"), r["features"])
                np.save(os.path.join(folder, split, name + "_info.npy"),
                        {"bbox": r["bbox"].copy(), "image_width": r["image_width"], "image_height": r["image_height"]})
        for mode in ("train", "test"):
            ds = VQA_Dataset([], opt, mode=mode)
            for i, r in enumerate(recs[:2]):
                fea, spa = ds.get_image_feature(r["path"], i)
                assert fea.dtype == torch.float32 and spa.dtype == torch.float32 and tuple(spa.shape) == (1, 36, 8)
                assert ds.get_image_feature(r["path"], i)[0] is fea            # the cache
                if mode == "train" or i == 1:            # (test mode reads the other folder's copy of the same files: one record's features do)
                    out["folder_%s_%d_features" % (mode, i)] = fea.numpy()
                out["folder_%s_%d_spatials" % (mode, i)] = spa.numpy()
    finally:
        shutil.rmtree(folder, ignore_errors=True)
    # the table path: boxes normalised ahead (as an exported table holds them); ids 2 and 0 are known, 1 is not
    table = {"img_id2idx": {2: 0, 0: 1},
             "img_features": torch.stack([T(r["features"]) for r in recs]),
             "img_spatials": torch.stack([T((r["bbox"] / np.array([r["image_width"], r["image_height"]] * 2)).astype(np.float32)) for r in recs])}
    ds = VQA_Dataset([], opt, mode="train", image_features=table)
    for q_id in (2, 0):
        fea, spa = ds.get_image_feature("unused.jpg", q_id)
        out["table_%d_features" % q_id] = fea.numpy()
        out["table_%d_spatials" % q_id] = spa.numpy()
    try:
        ds.get_image_feature("unused.jpg", 1)
        raise AssertionError("question id 1 is not in img_id2idx")
    except KeyError:
        pass
    out["table_ids"] = np.array([2, 0])
    save("img_feature_dataset", **out)


if __name__ == "__main__":
    which = sys.argv[1:] or ["e2e", "dataset"]
    bert_dir = None
    try:
        if "e2e" in which:
            cfg = synth.bert_config(vocab_size=2000)
            bert_dir = _refshim.write_bert_dir(cfg, synth.make_bert_weights(cfg, seed=SEED))
        for w in which:
            {"e2e": gen_e2e, "dataset": gen_dataset}[w](bert_dir)
    finally:
        if bert_dir is not None:
            shutil.rmtree(bert_dir, ignore_errors=True)
