"""The confs ``multi2one_bidir`` (with ``no_DeepAttention``), ``no_DeepAttention`` and last-layer BERT (no ``BERT_LINEAR_COMBINE``): what
tests/test_conf_rest_host.py and tests/test_gpu_conf_rest.py share (test infrastructure).  The constants restate those of
tools/gen_golden_conf_rest.py, which wrote the fixtures; the fixtures record the rewritten items, and ``batch`` checks them."""
import numpy as np
import torch

from ruart_amd import synth
from ruart_amd.arguments import default_opt

# fixture name -> (conf keys set, conf keys removed)
CONFS = {"sdnet_e2e_bidir_nodeep": (dict(multi2one_bidir=True, no_DeepAttention=True), ()),
         "sdnet_e2e_nodeep": (dict(no_DeepAttention=True), ()),
         "sdnet_e2e_lastlayer": ({}, ("BERT_LINEAR_COMBINE",)),
         "sdnet_e2e_bidir_nodeep_lastlayer": (dict(multi2one_bidir=True, no_DeepAttention=True), ("BERT_LINEAR_COMBINE",))}
OCR_LENGTHS = {0: 20, 1: 1, 2: 11, 7: 19, 40: 2, 98: 20, 101: 20, 103: 7, 104: 1}
OD_LENGTHS = {0: 10, 2: 6, 31: 10, 33: 1}
ROW0_TABLES = ("fast_embed.weight", "pos_embedding.weight", "ent_embedding.weight")


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def conf_opt(name, **extra):
    set_keys, drop_keys = CONFS[name]
    opt = default_opt(vocab_size=1500, **set_keys, **extra)
    for k in drop_keys:
        del opt[k]
    return opt


def batch(opt, z=None, B=2, seed=7, len_seed=19):
    """the fixtures' batch: synthetic_batch at sdnet_e2e_yesno.npz's sizes with a few items rewritten to other word counts"""
    q, ocr, od, gt, extra = synth.synthetic_batch(opt, B, seed=seed, n_q=30, n_ocr=100, n_od=30, bert_vocab=2000, ragged=True)
    synth.set_item_lengths(opt, ocr, OCR_LENGTHS, seed=len_seed, bert_vocab=2000, group="ocr")
    synth.set_item_lengths(opt, od, OD_LENGTHS, seed=len_seed + 1, bert_vocab=2000, group="od")
    if z is not None:
        assert int(z["B"]) == B and int(z["batch_seed"]) == seed and int(z["len_seed"]) == len_seed
        assert z["ocr_lengths"].tolist() == [list(kv) for kv in sorted(OCR_LENGTHS.items())]
        assert z["od_lengths"].tolist() == [list(kv) for kv in sorted(OD_LENGTHS.items())]
        assert ocr["num_cnt"] == z["ocr_num_cnt"].tolist() and od["num_cnt"] == z["od_num_cnt"].tolist()
        assert [l for s_ in ocr["len_cnt"] for l in s_] == z["ocr_len_cnt"].tolist()
        assert [l for s_ in od["len_cnt"] for l in s_] == z["od_len_cnt"].tolist()
        assert np.array_equal(gt.numpy(), z["gt"])
    return q, ocr, od, gt, extra
