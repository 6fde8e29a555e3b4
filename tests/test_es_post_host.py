"""``no_Context_Self_Attention`` and the host side of ``ES_using_way post_process`` without a GPU: the batch index's masks, gather
split and positions against what the unmodified reference hands to its modules (tests/golden/es_post_masks.npz, written by
tools/gen_golden_es_post.py), the state-dict key lists of the three confs, the draw order of the synthetic weights, and which conf keys
the constructor accepts (no_Context_Self_Attention) and refuses (post_process: its trunk is not part of the model yet)."""
import os
import pickle

import numpy as np
import pytest
import torch

from ruart_amd import synth
from ruart_amd.arguments import default_opt
from ruart_amd.batch import BatchIndex

# fixture name -> the conf keys it was written with
CONFS = {"sdnet_e2e_es_post": dict(ES_using_way="post_process"),
         "sdnet_e2e_noctx": dict(no_Context_Self_Attention=True),
         "sdnet_e2e_es_post_noctx": dict(ES_using_way="post_process", no_Context_Self_Attention=True)}


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a))


@pytest.fixture(scope="module")
def masks_golden(golden_dir):
    return np.load(os.path.join(golden_dir, "es_post_masks.npz"))


def _opt(**keys):
    opt = default_opt(vocab_size=1500, **keys)
    return {k: v for k, v in opt.items() if k != "BERT"}           # no encoder: the index's BERT part is not what is tested here


@pytest.mark.parametrize("cnt", [3, 6, 11, 12, 40, 100])
def test_batch_index_masks_split_and_positions_match_the_reference(masks_golden, cnt):
    """One sample with ``cnt`` items (sentinel included), E = ES_ocr_len = 10.  The (B, No - E) trunk mask - with the kept quirk: cnt < E
    leaves the first cnt slots of the (empty) trunk part live -, the scorer mask [ones | trunk mask], the positions of the trunk's
    slots, and the split of the item slots into the ES part and the trunk part (which gathered slots hold an item) equal what the
    reference's ES_ocr_att, get_answer, position_attn, ES_linear and context_rnn received.  The caller's position tensor is untouched."""
    z = masks_golden
    assert cnt in z["cnts"].tolist()
    opt = _opt(ES_using_way="post_process")
    E, No = int(z["E"]), opt["max_ocr_num"]
    assert E == opt["ES_ocr_len"]
    q, ocr, od, _, _ = synth.synthetic_batch(opt, 1, seed=int(z["seed"]), n_q=8, n_ocr=cnt, n_od=3, bert_vocab=2000, ragged=False)
    pos = ocr["position"]
    pos_before = pos.clone()
    bi = BatchIndex(q, ocr, od, opt)
    tag = "c%d_" % cnt
    assert bi.es_post == E and ocr["num_cnt"] == [cnt]
    assert bi.trunk_mask.dtype == np.uint8 and np.array_equal(bi.trunk_mask, z[tag + "att_mask"]) and bi.trunk_mask.shape == (1, No - E)
    assert np.array_equal(bi.score_mask, z[tag + "score_mask"]) and bi.score_mask.shape == (1, No)
    assert int(bi.trunk_mask.sum()) == (cnt - E if cnt >= E else cnt) and int(bi.score_mask.sum()) == E + int(bi.trunk_mask.sum())
    assert np.array_equal(bi.trunk_pos.numpy(), z[tag + "pos"])
    assert ocr["position"] is pos and torch.equal(pos, pos_before) and tuple(pos.shape) == (1, No, 8)
    slot_live = bi.ocr.mask.reshape(-1)                             # slots of the (B * No, D) item matrix that hold an item
    assert np.array_equal(slot_live[bi.es_rows].reshape(1, E), z[tag + "es_live"])
    assert np.array_equal(slot_live[bi.trunk_rows].reshape(1, No - E), z[tag + "trunk_live"])
    assert np.array_equal(np.sort(np.concatenate([bi.es_rows, bi.trunk_rows])), np.arange(No))      # every slot exactly once


def test_batch_index_split_over_several_samples_and_through_a_pickle():
    """B = 3 ragged: the row indices address the flat (B * No, D) matrix sample by sample; the host-side index (what the collate builds
    in DataLoader workers under ``prepare_index=True``) carries the same arrays through a pickle; a conf without the key builds none
    of them."""
    opt = _opt(ES_using_way="post_process")
    E, No = opt["ES_ocr_len"], opt["max_ocr_num"]
    q, ocr, od, _, _ = synth.synthetic_batch(opt, 3, seed=5, n_q=8, n_ocr=30, n_od=3, bert_vocab=2000, ragged=True)
    bi = BatchIndex(q, ocr, od, opt)
    rows = np.arange(3 * No).reshape(3, No)
    assert np.array_equal(bi.es_rows, rows[:, :E].reshape(-1)) and np.array_equal(bi.trunk_rows, rows[:, E:].reshape(-1))
    cnt = np.array(ocr["num_cnt"])
    assert (cnt >= E + 2).all() and np.array_equal(bi.trunk_mask.sum(1), cnt - E)
    assert torch.equal(bi.trunk_pos, ocr["position"][:, E:]) and bi.trunk_pos.is_contiguous()
    host = pickle.loads(pickle.dumps(bi))
    for f in ("es_rows", "trunk_rows", "trunk_mask", "score_mask"):
        assert np.array_equal(getattr(host, f), getattr(bi, f)), f
    assert torch.equal(host.trunk_pos, bi.trunk_pos)
    plain = BatchIndex(q, ocr, od, _opt())
    assert plain.es_post == 0 and not hasattr(plain, "es_rows")


@pytest.mark.parametrize("name", list(CONFS))
def test_state_dict_keys_match_the_reference(golden_dir, name):
    """The synthetic weights of each of the three confs name exactly the reference's state-dict keys (ES_linear and ES_ocr_att with
    post_process; no highlvl_self_att without the context self-attention).  For no_Context_Self_Attention, the conf the model
    accepts, a reference checkpoint loads: the module has the same keys in the same order, with the synthetic weights' shapes.  It is
    built without the encoder, which needs the device: its two mixing parameters (alphaBERT, gammaBERT) are the only other keys the
    fixture lists."""
    from ruart_amd.sdnet import SDNet
    want = [k for k in np.load(os.path.join(golden_dir, name + ".npz"))["keys"].tolist()]
    assert {"alphaBERT", "gammaBERT"} <= set(want)
    assert ("ES_linear.weight" in want) == ("ES_using_way" in CONFS[name])
    assert ("highlvl_self_att.scoring.linear.weight" in want) == ("no_Context_Self_Attention" not in CONFS[name])
    sw = synth.make_sdnet_weights(default_opt(vocab_size=1500, **CONFS[name]), seed=1033)
    assert sorted(sw) == sorted(want)
    if "ES_using_way" in CONFS[name]:
        return
    net = SDNet(_opt(**CONFS[name]), {"glove_embedding": torch.zeros(1500, 300), "fast_embedding": torch.zeros(1500, 300)})
    sd = net.state_dict()
    assert list(sd.keys()) == [k for k in want if k not in ("alphaBERT", "gammaBERT")]
    assert all(tuple(sd[k].shape) == sw[k].shape for k in sd if not k.startswith(("multi2one", "ques_rnn")))   # (input widths: no BERT)


def test_synth_weights_keep_their_draw_order(golden_dir):
    """A conf without the keys regenerates the weights the existing goldens were made with (tensors stored in sdnet_e2e_es_post.npz,
    and the float64 checksums sdnet_e2e.npz carries).  post_process appends four tensors; no_Context_Self_Attention drops the
    self-attention's two and narrows the high-level RNN's input weights to their first 250 columns - every other tensor is unchanged."""
    z = np.load(os.path.join(golden_dir, "sdnet_e2e_es_post.npz"))
    opt = default_opt(vocab_size=1500)
    base = synth.make_sdnet_weights(opt, seed=1033)
    stored = [k[len("synth:"):] for k in z.files if k.startswith("synth:")]
    assert len(stored) >= 4
    for n_ in stored:
        assert np.array_equal(base[n_][:2] if base[n_].ndim == 2 else base[n_], z["synth:" + n_]), n_
    wsum = np.array([float(np.sum(v.astype(np.float64))) for _, v in sorted(base.items())])
    assert np.array_equal(wsum, np.load(os.path.join(golden_dir, "sdnet_e2e.npz"))["sdnet_wsum"])
    es = synth.make_sdnet_weights(default_opt(vocab_size=1500, ES_using_way="post_process"), seed=1033)
    assert list(es)[:len(base)] == list(base) and all(np.array_equal(es[k], base[k]) for k in base)
    assert list(es)[len(base):] == ["ES_linear.weight", "ES_linear.bias", "ES_ocr_att.scoring.linear.weight", "ES_ocr_att.scoring.diagonal"]
    assert es["ES_linear.weight"].shape == (500, 300) and es["ES_ocr_att.scoring.linear.weight"].shape == (125, 500)
    assert es["ES_ocr_att.scoring.diagonal"].shape == (1, 1, 1) and abs(es["ES_ocr_att.scoring.diagonal"].item() - 125 ** -0.5) < 1e-7
    nc = synth.make_sdnet_weights(default_opt(vocab_size=1500, ES_using_way="post_process", no_Context_Self_Attention=True), seed=1033)
    assert set(es) - set(nc) == {"highlvl_self_att.scoring.linear.weight", "highlvl_self_att.scoring.diagonal"} and set(nc) <= set(es)
    for k in nc:
        if k.startswith("high_lvl_context_rnn.") and "weight_ih" in k:
            assert nc[k].shape == (500, 250) and np.array_equal(nc[k], es[k][:, :250]) and nc[k].flags["C_CONTIGUOUS"], k
        else:
            assert np.array_equal(nc[k], es[k]), k


def test_constructor_accepts_no_context_self_attention_and_refuses_the_rest():
    """no_Context_Self_Attention constructs (no highlvl_self_att, a 250-wide high-level RNN input); ES_using_way post_process - alone or
    with it -, fixed_answers and PRE_ALIGN_after_rnn raise.  opt['ruart_graph_trunk'] is refused together with the new key: the captured
    trunk was never run without the self-attention."""
    from ruart_amd.sdnet import SDNet
    emb = {"glove_embedding": torch.zeros(1500, 300), "fast_embedding": torch.zeros(1500, 300)}
    net = SDNet(_opt(no_Context_Self_Attention=True), emb)
    assert not hasattr(net, "highlvl_self_att") and net.high_lvl_context_rnn.rnns[0].weight_ih_l0.shape[1] == 250
    base = SDNet(_opt(), emb)
    assert hasattr(base, "highlvl_self_att") and base.high_lvl_context_rnn.rnns[0].weight_ih_l0.shape[1] == 500
    for keys in (dict(ES_using_way="post_process"), dict(ES_using_way="post_process", no_Context_Self_Attention=True),
                 dict(fixed_answers=True), dict(PRE_ALIGN_after_rnn=True), dict(no_Context_Self_Attention=True, ruart_graph_trunk=True)):
        with pytest.raises(NotImplementedError):
            SDNet(_opt(**keys), emb)
    SDNet(_opt(ruart_graph_trunk=True), emb)
