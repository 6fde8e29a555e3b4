"""Region image features (conf keys ``img_feature`` / ``img_fea_way replace_od`` / ``img_feature_replace_od``) without a GPU: which
confs the constructors accept and refuse, ``VQA_Dataset.get_image_feature`` against the unmodified reference's for both of its paths
(tests/golden/img_feature_dataset.npz, written by tools/gen_golden_img_feature.py), the collate passthrough, the batch index of the
two forms (the overlay rows; the pure form's encoder stream without the object group), the draw order of the synthetic weights and the
state-dict key list."""
import os
import pickle

import numpy as np
import pytest
import torch

from ruart_amd import synth
from ruart_amd.arguments import default_opt
from ruart_amd.batch import BatchIndex, VQA_collate, img_feature_form

IMG_KEYS = dict(img_feature=True, img_fea_way="replace_od", img_fea_num=36, img_fea_dim=2048, img_spa_dim=8, max_od_num=36)
# fixture name -> the conf keys it was written with
CONFS = {"sdnet_e2e_img_overlay": dict(IMG_KEYS), "sdnet_e2e_img_pure": dict(IMG_KEYS, img_feature_replace_od=True)}


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def _opt(**keys):
    opt = default_opt(vocab_size=1500, **keys)
    return {k: v for k, v in opt.items() if k != "BERT"}           # no encoder: it needs the device


def _emb():
    return {"glove_embedding": torch.zeros(1500, 300), "fast_embedding": torch.zeros(1500, 300)}


# ---- constructors ---------------------------------------------------------------------------------------------------------------------
def test_constructor_accepts_replace_od_in_both_forms():
    from ruart_amd.sdnet import SDNet
    for name, keys in CONFS.items():
        net = SDNet(_opt(**keys), _emb())
        assert net.img_form == ("pure" if "img_feature_replace_od" in keys else "overlay")
        assert tuple(net.img_fea2od.weight.shape) == (300, 2048) and tuple(net.img_fea2od.bias.shape) == (300,)
    assert img_feature_form(_opt()) is None and not hasattr(SDNet(_opt(), _emb()), "img_fea2od")


def test_constructor_refusals_name_their_reason():
    from ruart_amd.sdnet import SDNet
    with pytest.raises(NotImplementedError, match="3 \\* ques_final_size"):
        SDNet(_opt(**dict(IMG_KEYS, img_fea_way="final_att")), _emb())
    with pytest.raises(NotImplementedError, match="replace_od"):
        SDNet(_opt(**dict(IMG_KEYS, img_fea_way="something")), _emb())
    with pytest.raises(ValueError, match="img_spa_dim 4 != position_dim 8"):
        SDNet(_opt(**dict(IMG_KEYS, img_spa_dim=4)), _emb())
    with pytest.raises(NotImplementedError, match="ruart_graph_trunk"):
        SDNet(_opt(**dict(IMG_KEYS, ruart_graph_trunk=True)), _emb())
    for keys in (dict(fixed_answers=True), dict(IMG_KEYS, fixed_answers=True)):
        with pytest.raises(NotImplementedError, match="fixed_ocr_alpha"):
            SDNet(_opt(**keys), _emb())


def test_dataset_constructor_accepts_image_features_and_refuses_fixed_answers():
    from ruart_amd.dataset import VQA_Dataset
    ds = VQA_Dataset([], _opt(**IMG_KEYS), image_features={"img_id2idx": {}})
    assert ds.image_features == {"img_id2idx": {}} and ds.img_features_cache == {}
    assert VQA_Dataset([], _opt(**IMG_KEYS)).image_features is None
    with pytest.raises(NotImplementedError):
        VQA_Dataset([], _opt(fixed_answers=True))
    with pytest.raises(NotImplementedError):
        VQA_Dataset([], _opt(), fixed_answers_entry={})


def test_trainer_hands_its_table_to_the_datasets(monkeypatch):
    """SDNetTrainer.img_features (default None: the folder path) reaches every VQA_Dataset the trainer builds."""
    import ruart_amd.dataset as D
    from ruart_amd.trainer import SDNetTrainer
    tr = SDNetTrainer(_opt(**IMG_KEYS), device="cpu")
    assert tr.img_features is None
    tr.img_features = table = {"img_id2idx": {}}
    seen = []

    class Stop(Exception):
        pass

    def spy(data, opt, mode="train", image_features=None, fixed_answers_entry=None):
        seen.append((mode, image_features))
        raise Stop

    monkeypatch.setattr(D, "VQA_Dataset", spy)
    monkeypatch.setattr(tr, "_records", lambda split: [])
    monkeypatch.setattr(tr, "_setup_from_meta", lambda: None)
    monkeypatch.setattr(tr, "getSaveFolder", lambda: None)
    monkeypatch.setattr(tr, "load_model", lambda path: None)
    monkeypatch.setattr(tr, "close", lambda final=False: None)
    with pytest.raises(Stop):
        tr.train()
    tr.opt.update(RESUME=True, MODEL_PATH="x")
    with pytest.raises(Stop):
        tr.predict_for_test()
    assert seen == [("train", table), ("test", table)]


# ---- dataset ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ds_golden(golden_dir):
    return np.load(os.path.join(golden_dir, "img_feature_dataset.npz"))


@pytest.fixture(scope="module")
def records(ds_golden):
    recs = synth.synthetic_region_records(seed=int(ds_golden["rec_seed"]))
    assert [r["path"] for r in recs] == ds_golden["paths"].tolist()
    assert recs[0]["bbox"].dtype == np.float32 and recs[1]["bbox"].dtype == np.float64
    assert all(r["image_width"] % 2 == 1 and r["image_height"] % 2 == 1 for r in recs)
    return recs


def _write(folder, split, rec, name):
    path = os.path.join(str(folder), split, name)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    np.save(path + ".npy", rec["features"])
    np.save(path + "_info.npy", {"bbox": rec["bbox"].copy(), "image_width": rec["image_width"], "image_height": rec["image_height"]})


@pytest.mark.parametrize("mode", ["train", "test"])
def test_dataset_folder_path_matches_the_reference(ds_golden, records, tmp_path, mode):
    """<folder>/{train|test}/<name>.npy + <name>_info.npy, <name> = the path's dot-separated parts without the last joined WITHOUT dots
    (sic): 'scene.v0/im.000.jpg' is read from 'scenev0/im000'.  Only the split the mode selects is written, so the other one cannot
    serve.  Boxes float32 and float64, odd image sizes: features and the eight-column corner layout bit-equal to the reference's; the
    second request of a path is the cached pair."""
    from ruart_amd.dataset import VQA_Dataset
    z = ds_golden
    assert records[0]["path"] == "scene.v0/im.000.jpg"
    for i, name in enumerate(("scenev0/im000", "scenev1/im001")):
        _write(tmp_path, "train" if mode != "test" else "test", records[i], name)
    ds = VQA_Dataset([], _opt(**dict(IMG_KEYS, img_fea_folder=str(tmp_path))), mode=mode)
    for i in (0, 1):
        fea, spa = ds.get_image_feature(records[i]["path"], 5)
        assert fea.dtype == torch.float32 and spa.dtype == torch.float32
        assert tuple(fea.shape) == (1, 36, 2048) and tuple(spa.shape) == (1, 36, 8)
        if "folder_%s_%d_features" % (mode, i) in z.files:
            assert np.array_equal(fea.numpy(), z["folder_%s_%d_features" % (mode, i)])
        assert np.array_equal(fea.numpy()[0], records[i]["features"])
        assert np.array_equal(spa.numpy(), z["folder_%s_%d_spatials" % (mode, i)])
        s = spa[0]
        assert torch.equal(s[:, 3], s[:, 1]) and torch.equal(s[:, 4], s[:, 2]) and torch.equal(s[:, 6], s[:, 0]) and torch.equal(s[:, 7], s[:, 5])
        assert 0.0 <= float(s.min()) and float(s.max()) <= 1.0
        again = ds.get_image_feature(records[i]["path"], 6)
        assert again[0] is fea and again[1] is spa                      # the cache, keyed by the image path
    assert sorted(ds.img_features_cache) == sorted(r["path"] for r in records[:2])
    with pytest.raises(AssertionError):
        ds.get_image_feature("scene.v0/missing.jpg", 0)


def test_dataset_getitem_attaches_the_features(records, tmp_path, golden_dir):
    """__getitem__ puts the pair into the question dict (Utils/VQA_Dataset.py:143-144) and the collate stacks it."""
    import copy
    import json
    from ruart_amd.dataset import VQA_Dataset
    with open(os.path.join(golden_dir, "dataset_input.json"), encoding="utf-8") as f:
        inp = json.load(f)
    vocab = tmp_path / "vocab.txt"
    vocab.write_text("\n".join(inp["vocab"]) + "\n", encoding="utf-8")
    recs = copy.deepcopy(inp["records"])[:2]
    for i, r in enumerate(recs):
        r["filename"] = records[i]["path"]
    for i, name in enumerate(("scenev0/im000", "scenev1/im001")):
        _write(tmp_path, "train", records[i], name)
    opt = default_opt(datadir="", BERT_tokenizer_file=str(vocab), **dict(IMG_KEYS, img_fea_folder=str(tmp_path)))
    ds = VQA_Dataset(recs, opt)
    samples = [ds[i] for i in range(2)]
    assert all(tuple(s_["q"]["img_features"].shape) == (1, 36, 2048) for s_ in samples)
    q = VQA_collate(opt).VQA_collate_fun(samples)[0]
    assert tuple(q["img_features"].shape) == (2, 36, 2048) and tuple(q["img_spatials"].shape) == (2, 36, 8)
    assert np.array_equal(q["img_features"][1].numpy(), records[1]["features"])


def test_dataset_table_path_indexes_by_question_id(ds_golden, records):
    """The table path requires q_id in img_id2idx and then indexes the tables by q_id ITSELF (sic): with {2: 0, 0: 1} question 2 gets
    row 2, not row 0; question 1 is unknown (KeyError).  Shapes other than (1, 36, 2048) / (1, 36, 8) trip the asserts."""
    from ruart_amd.dataset import VQA_Dataset
    z = ds_golden
    table = {"img_id2idx": {2: 0, 0: 1},
             "img_features": torch.stack([T(r["features"]) for r in records]),
             "img_spatials": torch.stack([T((r["bbox"] / np.array([r["image_width"], r["image_height"]] * 2)).astype(np.float32)) for r in records])}
    ds = VQA_Dataset([], _opt(**IMG_KEYS), image_features=table)
    for q_id in z["table_ids"].tolist():
        fea, spa = ds.get_image_feature("unused.jpg", q_id)
        assert np.array_equal(fea.numpy(), z["table_%d_features" % q_id]) and np.array_equal(spa.numpy(), z["table_%d_spatials" % q_id])
        assert np.array_equal(fea.numpy()[0], records[q_id]["features"])
    assert ds.img_features_cache == {}
    with pytest.raises(KeyError):
        ds.get_image_feature("unused.jpg", 1)
    short = dict(table, img_features=table["img_features"][:, :35])
    with pytest.raises(AssertionError):
        VQA_Dataset([], _opt(**IMG_KEYS), image_features=short).get_image_feature("unused.jpg", 0)


# ---- collate and batch index ---------------------------------------------------------------------------------------------------------
def test_collate_passes_the_features_through_with_a_prepared_index():
    """VQA_collate(prepare_index=True) on samples that carry the two tensors: stacked along the batch, and the host index (pure form)
    is built in the collate, survives a pickle and carries the pure form's plan."""
    from tests.test_host_logic import _samples_like_generator
    opt = default_opt(**dict(IMG_KEYS, img_feature_replace_od=True))
    samples = _samples_like_generator(opt, 3, 5)
    fea, spa = synth.synthetic_image_features(opt, 3, seed=3)
    for i, s_ in enumerate(samples):
        s_["q"]["img_features"], s_["q"]["img_spatials"] = fea[i:i + 1], spa[i:i + 1]
    q, ocr, od, gt, extra = VQA_collate(opt, prepare_index=True).VQA_collate_fun(samples)
    assert torch.equal(q["img_features"], fea) and torch.equal(q["img_spatials"], spa)
    host = pickle.loads(pickle.dumps(q["_ruart_host_index"]))
    assert host.img_form == "pure" and host.od is None and host.plan == (True, False, True, "no_od_group")
    dev = host.to("cpu")
    assert len(dev.spans) == 2 and tuple(dev.od_mask.shape) == (3, 36) and bool(dev.od_mask.all()) and dev.od_mask.dtype == torch.uint8


def _batch(opt, od_counts, seed=7):
    q, ocr, _, _, _ = synth.synthetic_batch(opt, len(od_counts), seed=seed, n_q=8, n_ocr=14, n_od=3, bert_vocab=2000, ragged=True)
    od, _ = synth.synthetic_objects(opt, od_counts, seed=seed, bert_vocab=2000)
    assert od["num_cnt"] == list(od_counts)
    return q, ocr, od


def test_batch_index_pure_form_packs_question_and_ocr_alone():
    """img_feature_replace_od: the encoder stream holds the question's and the OCR items' word pieces and nothing of the object items
    (two span groups, no object ItemIndex, no object embedding sorts), whatever the object list; ``plan`` tells the forms apart, so
    an index built in a loader worker for one form is not accepted for the other."""
    base = default_opt(vocab_size=1500, **IMG_KEYS)
    pure = dict(base, img_feature_replace_od=True)
    q, ocr, od = _batch(base, (36, 32))
    bi = BatchIndex(q, ocr, od, pure)
    n_q, n_ocr, n_od = (int(d["bert_mask"].sum()) for d in (q, ocr, od))
    full = BatchIndex(q, ocr, od, dict(base, bert_dedup=False))
    lean = BatchIndex(q, ocr, od, dict(pure, bert_dedup=False))
    assert n_od > 0 and full.packed.T == n_q + n_ocr + n_od and lean.packed.T == n_q + n_ocr
    assert bi.od is None and len(bi._spans_host[1]) == 2 and len(full._spans_host[1]) == 3
    assert not any(k[0] == "od" for k in bi._emb_host) and any(k[0] == "od" for k in full._emb_host)
    over = BatchIndex(q, ocr, od, base)
    assert bi.plan != over.plan and over.plan == (True, False, True) and bi.plan[:3] == over.plan
    # the stream does not depend on the object list at all
    other = BatchIndex(q, ocr, _batch(base, (5, 4))[2], pure)
    assert np.array_equal(other.packed.host, bi.packed.host) and np.array_equal(other._spans_host[0], bi._spans_host[0])
    dev = bi.to("cpu")
    assert len(dev.spans) == 2 and tuple(dev.od_mask.shape) == (2, 36) and bool(dev.od_mask.all())
    assert len(dev._staged()["item_sizes"]) == len(dev.ocr.fields())


@pytest.mark.parametrize("counts", [(5, 4), (36, 1)])
def test_overlay_row_index(counts):
    """Overlay form: item k of sample b lands on row b * img_fea_num + k of the projected features - one flat index of distinct rows, in
    multi2one's item order (as flat_slot); the object mask is all ones over (B, img_fea_num)."""
    opt = _opt(**dict(IMG_KEYS, max_od_num=40))                    # position rows (40) and image rows (36) differ
    q, ocr, od = _batch(opt, counts)
    bi = BatchIndex(q, ocr, od, opt)
    idx = bi.od
    rows = idx.extra["flat_img"]
    assert np.array_equal(rows, idx.sorted_sample * 36 + idx.sorted_slot) and len(np.unique(rows)) == len(rows) == sum(counts)
    assert sorted(rows.tolist()) == [b * 36 + k for b, n in enumerate(counts) for k in range(n)]
    assert np.array_equal(idx.flat_slot, idx.sorted_sample * 40 + idx.sorted_slot)
    dev = bi.to("cpu")
    assert torch.equal(dev.od.dev["flat_img"], torch.from_numpy(rows)) and dev.od.dev["flat_slot"].numel() == sum(counts)
    assert tuple(dev.od_mask.shape) == (2, 36) and bool(dev.od_mask.all()) and dev.od_mask.dtype == torch.uint8
    plain = BatchIndex(q, ocr, od, _opt(max_od_num=40))
    assert "flat_img" not in plain.od.fields() and plain.img_form is None and int(plain.od.mask.sum()) == sum(counts)


def test_overlay_refuses_more_object_items_than_image_rows():
    """37 object items against img_fea_num 36: the reference dies with an IndexError inside its loop; here a ValueError names the
    sample.  The pure form does not look at the object list."""
    opt = _opt(**dict(IMG_KEYS, max_od_num=40))
    q, ocr, od = _batch(opt, (37, 2))
    with pytest.raises(ValueError, match="sample 0 holds 37 object items, img_fea_num is 36"):
        BatchIndex(q, ocr, od, opt)
    assert BatchIndex(q, ocr, od, dict(opt, img_feature_replace_od=True)).od is None


# ---- synthetic weights and state-dict keys -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CONFS))
def test_synth_weights_keep_their_draw_order(golden_dir, name):
    """The conf without the keys regenerates the tensors the fixture stored for it, bit for bit; the image-feature confs append
    img_fea2od.weight / .bias after every existing draw and change nothing else."""
    z = np.load(os.path.join(golden_dir, name + ".npz"))
    base = synth.make_sdnet_weights(default_opt(vocab_size=1500), seed=int(z["seed"]))
    stored = [k[len("synth:"):] for k in z.files if k.startswith("synth:")]
    assert len(stored) >= 4
    for n_ in stored:
        assert np.array_equal(base[n_][:2] if base[n_].ndim == 2 else base[n_], z["synth:" + n_]), n_
    wsum = np.array([float(np.sum(v.astype(np.float64))) for _, v in sorted(base.items())])
    assert np.array_equal(wsum, np.load(os.path.join(golden_dir, "sdnet_e2e.npz"))["sdnet_wsum"])
    img = synth.make_sdnet_weights(default_opt(vocab_size=1500, **CONFS[name]), seed=int(z["seed"]))
    assert list(img)[:len(base)] == list(base) and all(np.array_equal(img[k], base[k]) for k in base)
    assert list(img)[len(base):] == ["img_fea2od.weight", "img_fea2od.bias"]
    assert img["img_fea2od.weight"].shape == (300, 2048) and img["img_fea2od.bias"].shape == (300,)
    assert float(np.abs(img["img_fea2od.weight"]).max()) <= 2048 ** -0.5


@pytest.mark.parametrize("name", list(CONFS))
def test_state_dict_keys_match_the_reference(golden_dir, name):
    """Same keys in the same order as the reference's module (img_fea2od between ques_merger and get_answer), so its checkpoints
    load; built without the encoder, whose two mixing parameters are the only other keys the fixture lists."""
    from ruart_amd.sdnet import SDNet
    want = np.load(os.path.join(golden_dir, name + ".npz"))["keys"].tolist()
    assert want.index("ques_merger.linear.bias") + 1 == want.index("img_fea2od.weight") == want.index("img_fea2od.bias") - 1
    assert want.index("img_fea2od.bias") + 1 == want.index("get_answer.noanswer_linear.weight")
    sw = synth.make_sdnet_weights(default_opt(vocab_size=1500, **CONFS[name]), seed=1033)
    assert sorted(sw) == sorted(want)
    sd = SDNet(_opt(**CONFS[name]), _emb()).state_dict()
    assert list(sd.keys()) == [k for k in want if k not in ("alphaBERT", "gammaBERT")]
    assert all(tuple(sd[k].shape) == sw[k].shape for k in sd if not k.startswith(("multi2one", "ques_rnn")))   # (input widths: no BERT)


def test_synthetic_image_features_are_seeded_and_post_relu_like():
    opt = _opt(**IMG_KEYS)
    fea, spa = synth.synthetic_image_features(opt, 2, seed=3)
    fea2, spa2 = synth.synthetic_image_features(opt, 2, seed=3)
    assert torch.equal(fea, fea2) and torch.equal(spa, spa2) and not torch.equal(fea, synth.synthetic_image_features(opt, 2, seed=4)[0])
    assert tuple(fea.shape) == (2, 36, 2048) and tuple(spa.shape) == (2, 36, 8) and fea.dtype == spa.dtype == torch.float32
    assert float(fea.min()) >= 0.0 and 0.7 < float(fea.mean()) < 0.9 and 0.0 <= float(spa.min()) and float(spa.max()) < 1.0
    assert fea.device.type == "cpu"
