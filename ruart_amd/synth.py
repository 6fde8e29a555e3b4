"""Seeded synthetic weights and batches in the reference's layouts.

There is no network on any box, so checkpoints and datasets are synthetic:
  * BERT weights under the HF-0.x names the reference loads
    (``Models/Bert/modeling.py:497-521``: ``bert.`` prefix, ``LayerNorm.gamma/beta``);
  * SDNet weights under the reference's state-dict names;
  * batches in the ``VQA_collate_fun`` 5-tuple layout
    (``Utils/VQA_Dataset.py:448-542``): dicts of int64 id matrices, bool masks,
    python offset / count lists, ``position (B, max_num, 8)`` and ``gt (B, No+1)`` (``label_yesno``: ``(B, 3+No(+1))``).

Everything is drawn from ``numpy.random.default_rng(seed)`` in a fixed order so the
build container (golden generator) and the GPU box regenerate identical arrays.
"""
import math

import numpy as np
import torch

BERT_BASE = dict(vocab_size=30522, hidden_size=768, num_hidden_layers=12,
                 num_attention_heads=12, intermediate_size=3072, hidden_act="gelu",
                 hidden_dropout_prob=0.1, attention_probs_dropout_prob=0.1,
                 max_position_embeddings=512, type_vocab_size=2, initializer_range=0.02)


def bert_config(**kw):
    cfg = dict(BERT_BASE)
    cfg.update(kw)
    return cfg


def make_bert_weights(cfg, seed=1033, w_std=0.05):
    """name -> float32 array.  Linear / embedding weights N(0, w_std); LayerNorm
    gamma ~ 1 + 0.1 N, beta ~ 0.1 N; biases ~ 0.02 N (non-trivial on purpose so
    every epilogue term is exercised by parity tests)."""
    g = np.random.default_rng(seed)
    H, I = cfg["hidden_size"], cfg["intermediate_size"]
    w = {}

    def lin(name, o, i):
        w[name + ".weight"] = (g.standard_normal((o, i)) * w_std).astype(np.float32)
        w[name + ".bias"] = (g.standard_normal(o) * 0.02).astype(np.float32)

    def ln(name):
        w[name + ".gamma"] = (1.0 + 0.1 * g.standard_normal(H)).astype(np.float32)
        w[name + ".beta"] = (0.1 * g.standard_normal(H)).astype(np.float32)

    e = "bert.embeddings."
    w[e + "word_embeddings.weight"] = (g.standard_normal((cfg["vocab_size"], H)) * w_std).astype(np.float32)
    w[e + "position_embeddings.weight"] = (g.standard_normal((cfg["max_position_embeddings"], H)) * w_std).astype(np.float32)
    w[e + "token_type_embeddings.weight"] = (g.standard_normal((cfg["type_vocab_size"], H)) * w_std).astype(np.float32)
    ln(e + "LayerNorm")
    for l in range(cfg["num_hidden_layers"]):
        p = "bert.encoder.layer.%d." % l
        lin(p + "attention.self.query", H, H)
        lin(p + "attention.self.key", H, H)
        lin(p + "attention.self.value", H, H)
        lin(p + "attention.output.dense", H, H)
        ln(p + "attention.output.LayerNorm")
        lin(p + "intermediate.dense", I, H)
        lin(p + "output.dense", H, I)
        ln(p + "output.LayerNorm")
    lin("bert.pooler.dense", H, H)
    return w


def add_bert_outliers(w, cfg, seed=77, n_dims=4, gain=(10.0, 30.0), emb_scale=20.0, n_emb_dims=3):
    """Give seeded random encoder weights the heavy tails a PRETRAINED BERT has and N(0, s) weights lack (in place, deterministic):
    a few hidden dimensions - the same ones in every LayerNorm, as in the published checkpoints, where a handful of dimensions carry
    activations an order of magnitude above the rest - get their gain multiplied by U(gain), and a few columns of the word-embedding
    table are scaled by ``emb_scale``.  Used by the fp16c range test (tests/golden/sdnet_e2e_outliers.npz): LayerNorm outputs of
    30-100 and embedding entries of ~1 push the e4m3 correction operands (csrc/common.h: |v| < 112, |w| < 3.5) to their limits."""
    g = np.random.default_rng(seed)
    H = cfg["hidden_size"]
    dims = g.choice(H, size=n_dims, replace=False)
    for name in sorted(w):
        if name.endswith("LayerNorm.gamma"):
            w[name][dims] *= g.uniform(gain[0], gain[1], size=n_dims).astype(np.float32)
    edims = g.choice(H, size=n_emb_dims, replace=False)
    w["bert.embeddings.word_embeddings.weight"][:, edims] *= np.float32(emb_scale)
    return w


# --------------------------------------------------------------------------------------
# SDNet parameter table (names and shapes follow the reference constructor,
# Models/SDNet.py:21-251 and Models/Layers.py; verified against the instantiated
# reference by oracle/gen_golden.py).
# --------------------------------------------------------------------------------------
def sdnet_dims(opt):
    bert_dim, bert_layers = (1024, 24) if "BERT_LARGE" in opt else (768, 12)
    q_names = opt["q_embedding"].split(",")
    o_names = opt["ocr_embedding"].split(",")

    def width(names):
        n = 0
        n += opt["glove_dim"] if "glove" in names else 0
        n += opt["fast_dim"] if "fasttext" in names else 0
        n += int(opt["phoc_dim"]) if "phoc" in names else 0
        n += bert_dim if "bert" in names else 0
        n += opt["pos_dim"] if "pos" in names else 0
        n += opt["ent_dim"] if "ent" in names else 0
        return n

    x_in = width(o_names) + (300 if "PRE_ALIGN_befor_rnn" in opt else 0)
    q_in = width(q_names)
    h = opt["hidden_size"]
    hh = opt["highlvl_hidden_size"]
    m2o = opt["multi2one_hidden_size"] * (2 if opt["multi2one_bidir"] else 1)
    nl = opt["in_rnn_layers"]
    att_size = 2 * h * nl + m2o
    deep_rnn_in = 2 * h * nl * 2 + 2 * hh
    self_att_in = 2 * hh + deep_rnn_in + m2o
    return dict(bert_dim=bert_dim, bert_layers=bert_layers, x_in=x_in, q_in=q_in, h=h, hh=hh,
                m2o=m2o, nl=nl, att_size=att_size, deep_rnn_in=deep_rnn_in,
                self_att_in=self_att_in, ctx_final=2 * hh, q_final=2 * hh,
                ocr_final=4 * hh if opt["pos_att_merge_mod"] == "cat" else 2 * hh)


def sdnet_param_shapes(opt):
    """name -> shape, in the order make_sdnet_weights draws.  Always the table WITH the context self-attention and the deep attention:
    the conf keys ``no_Context_Self_Attention`` and ``no_DeepAttention`` are applied by make_sdnet_weights to what it drew, so that
    they move no other tensor."""
    d = sdnet_dims(opt)
    V = int(opt["vocab_size"])
    s = {}
    s["alphaBERT"] = (d["bert_layers"],)
    s["gammaBERT"] = (1, 1)
    s["fast_embed.weight"] = (V, opt["fast_dim"])
    s["glove_embed.weight"] = (V, opt["glove_dim"])
    if "PHOC" in opt:
        s["phoc_embed.weight"] = (V, int(opt["phoc_dim"]))      # values: phoc_vocab_words() through the PHOC builder, not random

    def attn(name, din, hid, similarity=False):
        s[name + ".scoring.linear.weight"] = (hid, din)
        s[name + ".scoring.diagonal"] = (1, 1, 1) if similarity else (1, 1, hid)

    def lstm(name, din, hid, layers, bidir=True):
        for l in range(layers):
            i = din if l == 0 else hid * (2 if bidir else 1)
            for sfx in ([""] + (["_reverse"] if bidir else [])):
                p = "%s.rnns.%d." % (name, l)
                s[p + "weight_ih_l0" + sfx] = (4 * hid, i)
                s[p + "weight_hh_l0" + sfx] = (4 * hid, hid)
                s[p + "bias_ih_l0" + sfx] = (4 * hid,)
                s[p + "bias_hh_l0" + sfx] = (4 * hid,)

    attn("pre_align", 300, opt["prealign_hidden"], True)
    s["pos_embedding.weight"] = (opt["pos_vocab_size"], opt["pos_dim"])
    s["ent_embedding.weight"] = (opt["ent_vocab_size"], opt["ent_dim"])
    lstm("multi2one", d["x_in"], opt["multi2one_hidden_size"], 1, bool(opt["multi2one_bidir"]))
    lstm("context_rnn", d["m2o"], d["h"], d["nl"])
    lstm("ques_rnn", d["q_in"], d["h"], d["nl"])
    for i in range(d["nl"] + 1):
        attn("deep_attn.int_attn_list.%d" % i, d["att_size"], opt["deep_att_hidden_size_per_abstr"])
    lstm("deep_attn.rnn", d["deep_rnn_in"], d["hh"], 1)
    lstm("high_lvl_ques_rnn", 2 * d["h"] * d["nl"], d["hh"], opt["question_high_lvl_rnn_layers"])
    attn("highlvl_self_att", d["self_att_in"], opt["deep_att_hidden_size_per_abstr"])
    lstm("high_lvl_context_rnn", 4 * d["hh"], d["hh"], 1)
    attn("ques_self_attn", d["q_final"], opt["query_self_attn_hidden_size"])
    attn("od_ocr_attn", d["ctx_final"], d["h"], True)
    attn("position_attn", opt["position_dim"], d["h"], True)
    s["ques_merger.linear.weight"] = (1, d["q_final"])
    s["ques_merger.linear.bias"] = (1,)
    xs, hs = d["ocr_final"], d["q_final"]
    s["get_answer.noanswer_linear.weight"] = (xs, hs)
    s["get_answer.noanswer_linear.bias"] = (xs,)
    s["get_answer.noanswer_w.weight"] = (1, xs)
    s["get_answer.noanswer_w.bias"] = (1,)
    s["get_answer.attn.linear.weight"] = (xs, hs)
    s["get_answer.attn.linear.bias"] = (xs,)
    s["get_answer.rnn.weight_ih"] = (3 * hs, xs)
    s["get_answer.rnn.weight_hh"] = (3 * hs, hs)
    s["get_answer.rnn.bias_ih"] = (3 * hs,)
    s["get_answer.rnn.bias_hh"] = (3 * hs,)
    s["get_answer.attn2.linear.weight"] = (xs, hs)
    s["get_answer.attn2.linear.bias"] = (xs,)
    if "label_yesno" in opt:
        # after every existing entry: make_sdnet_weights draws in this order, so the weights of a conf without the key do not move
        for head in ("no", "yes", "no_read"):
            s["get_answer.%s_linear.weight" % head] = (xs, hs)
            s["get_answer.%s_linear.bias" % head] = (xs,)
            s["get_answer.%s_w.weight" % head] = (1, xs)
            s["get_answer.%s_w.bias" % head] = (1,)
    if "ES_ocr" in opt and opt.get("ES_using_way") == "post_process":      # Models/SDNet.py:246-248; again after every earlier entry
        s["ES_linear.weight"] = (xs, d["m2o"])
        s["ES_linear.bias"] = (xs,)
        attn("ES_ocr_att", xs, d["h"], True)
    if "img_feature" in opt:                     # Models/SDNet.py:226; after every earlier entry once more
        s["img_fea2od.weight"] = (d["m2o"], int(opt["img_fea_dim"]))
        s["img_fea2od.bias"] = (d["m2o"],)
    return s


def _draw(g, name, shape, opt):
    """one tensor of the table from the generator ``g`` (float64; the kind of draw goes by the parameter's name)"""
    if name == "alphaBERT":
        return 1.0 + 0.5 * g.standard_normal(shape)
    if name == "gammaBERT":
        return np.full(shape, 0.9)
    if name.endswith("embed.weight"):
        a = g.standard_normal(shape)
        a[0] = 0.0
        return a
    if name.endswith("scoring.diagonal"):
        return (np.full(shape, 1.0 / math.sqrt(opt_hidden_for(name, opt))) if shape == (1, 1, 1)
                else 1.0 + 0.2 * g.standard_normal(shape))
    if name.endswith("embedding.weight"):
        return g.standard_normal(shape)
    fan = shape[-1] if len(shape) > 1 else None
    if "rnn" in name:            # torch LSTM/GRU init: U(-1/sqrt(hidden), +)
        hid = shape[0] // (3 if name.startswith("get_answer.rnn") else 4)
        k = 1.0 / math.sqrt(hid)
    elif fan is not None:
        k = 1.0 / math.sqrt(fan)
    else:
        k = 0.05
    return g.uniform(-k, k, shape)


def make_sdnet_weights(opt, seed=1033):
    """name -> float32 array for every entry of sdnet_param_shapes(opt).  ``no_Context_Self_Attention`` (Models/SDNet.py:180-188)
    draws that table too and then drops the self-attention's tensors and keeps the first columns of the narrower
    ``high_lvl_context_rnn`` input weights (the ones that multiply deep_attn's output in either form): every other tensor is the one
    the conf without the key gets.  ``no_DeepAttention`` (Models/Layers.py:477-479) is applied the same way: the attention levels'
    tensors are dropped, ``deep_attn.rnn`` keeps the first columns of its input weights (the ones that multiply the abstraction layers
    in either form) and ``highlvl_self_att`` the columns of what is left of its input [deep_attn output | abstraction layers | words].
    A conf without ``BERT_LINEAR_COMBINE`` draws alphaBERT and drops the two mix parameters.  ``multi2one_bidir`` draws the table of
    the uni-directional conf first and everything it adds afterwards, in table order: the reverse direction's four tensors, and for
    every tensor the 600-wide multi2one output widens the block that is new, appended to the uni-directional conf's tensor - which
    stays its leading block; tensors of unchanged shape are the uni-directional conf's."""
    g = np.random.default_rng(seed + 17)
    out = {}
    no_ctx = "no_Context_Self_Attention" in opt
    no_deep = "no_DeepAttention" in opt
    no_mix = "BERT_LINEAR_COMBINE" not in opt
    d = sdnet_dims(opt)
    abstr = 2 * d["h"] * d["nl"]
    table = sdnet_param_shapes(opt)
    bidir = bool(opt["multi2one_bidir"])
    uni = sdnet_param_shapes(dict(opt, multi2one_bidir=False)) if bidir else table
    drawn = {name: _draw(g, name, shape, opt) for name, shape in uni.items()}
    if bidir:
        for name, shape in table.items():
            if name not in drawn:
                drawn[name] = _draw(g, name, shape, opt)
            elif shape != uni[name]:
                ax = [i for i, (a_, b_) in enumerate(zip(shape, uni[name])) if a_ != b_]
                assert len(ax) == 1 and len(shape) == len(uni[name]), (name, shape, uni[name])
                extra = list(shape)
                extra[ax[0]] = shape[ax[0]] - uni[name][ax[0]]
                drawn[name] = np.concatenate([drawn[name], _draw(g, name, tuple(extra), opt)], ax[0])
    for name, shape in table.items():
        a = drawn[name]
        if no_mix and name in ("alphaBERT", "gammaBERT"):
            continue
        if no_ctx and name.startswith("highlvl_self_att."):
            continue
        if no_ctx and name.startswith("high_lvl_context_rnn.") and "weight_ih" in name:
            a = a[:, :shape[1] // 2]
        if no_deep and name.startswith("deep_attn.int_attn_list."):
            continue
        if no_deep and name.startswith("deep_attn.rnn.") and "weight_ih" in name:
            a = a[:, :abstr]
        if no_deep and name == "highlvl_self_att.scoring.linear.weight":
            a = np.concatenate([a[:, :2 * d["hh"] + abstr], a[:, 2 * d["hh"] + d["deep_rnn_in"]:]], 1)
        out[name] = np.ascontiguousarray(a, dtype=np.float32)
    return out


def opt_hidden_for(name, opt):
    if name.startswith("pre_align"):
        return opt["prealign_hidden"]
    return opt["hidden_size"]


# --------------------------------------------------------------------------------------
# Batches
# --------------------------------------------------------------------------------------
def _bertify(g, n_words, bert_vocab, max_bert_len, p2=0.4):
    """[CLS] pieces... [SEP]; returns (ids, offsets[[st, ed], ...]) like
    VQA_Dataset.bertify (Utils/VQA_Dataset.py:415-436)."""
    pieces = 1 + (g.random(n_words) < p2).astype(np.int64)
    while pieces.sum() > max_bert_len - 2:
        pieces[np.argmax(pieces)] -= 1
    ids = [101]
    offs = []
    for c in pieces:
        offs.append([len(ids), len(ids) + int(c)])
        ids.extend(int(v) for v in g.integers(1000 if bert_vocab > 1500 else 10, bert_vocab, size=int(c)))
    ids.append(102)
    return ids, offs


def phoc_vocab_words(V, seed=1033):
    """A deterministic spelling for every word id (ids 0..4 = padding / unknown / sentinels get the empty word): the PHOC
    table of a synthetic vocabulary is built from these, on the reference side with its ``build_phoc``, here with
    ``ruart_amd.phoc.phoc_table``."""
    g = np.random.default_rng(seed + 41)
    alpha = "abcdefghijklmnopqrstuvwxyz0123456789"
    return ["" if i < 5 else "".join(alpha[int(k)] for k in g.integers(0, 36, size=int(g.integers(1, 13)))) for i in range(V)]


def synthetic_image_features(opt, B, seed=3):
    """(img_features (B, img_fea_num, img_fea_dim), img_spatials (B, img_fea_num, img_spa_dim)) float32 for a batch's question dict:
    features |N(0, 1)| - non-negative like the pooled post-ReLU activations of a detector -, box coordinates U[0, 1).  A CPU
    torch generator, so that every box draws the same values."""
    g = torch.Generator().manual_seed(int(seed))
    fea = torch.randn(B, int(opt["img_fea_num"]), int(opt["img_fea_dim"]), generator=g).abs_()
    spa = torch.rand(B, int(opt["img_fea_num"]), int(opt["img_spa_dim"]), generator=g)
    return fea, spa


def synthetic_objects(opt, counts, seed=7, bert_vocab=30522):
    """The object group of ``synthetic_batch`` with exactly ``counts`` items per sample (the ``<OD>`` sentinel included, counts[0] the
    largest): of the ragged batches of seeds ``seed``, ``seed + 1``, ... the first whose draw gives these counts.
    Returns (od_list, the seed it came from)."""
    counts = [int(c) for c in counts]
    lo = min(opt["max_ocr_num"], opt.get("ES_ocr_len", 0) + 2)
    for s in range(seed, seed + 4096):
        od = synthetic_batch(opt, len(counts), seed=s, n_q=2, n_ocr=lo, n_od=counts[0], bert_vocab=bert_vocab, ragged=True, targets=False)[2]
        if od["num_cnt"] == counts:
            return od, s
    raise ValueError("no ragged draw with object counts %s" % (counts,))


def synthetic_region_records(seed=3, n=3, n_box=36, dim=2048):
    """``n`` per-image region records as a bottom-up detector's export holds them: {'path', 'features' (n_box, dim) float32, 'bbox'
    (n_box, 4) pixel boxes x0 y0 x1 y1 - float32 for even records, float64 for odd ones -, 'image_width', 'image_height' (odd
    numbers)}.  The features take four values (0, 0.5, 1, 1.5), so that a fixture holding them compresses; the paths carry dots in
    their folder and stem (dataset.VQA_Dataset.get_image_feature joins the parts without them)."""
    g = np.random.default_rng(seed)
    recs = []
    for i in range(n):
        w, h = 2 * int(g.integers(200, 600)) + 1, 2 * int(g.integers(150, 400)) + 1
        x = np.sort(g.uniform(0, w, size=(n_box, 2)), axis=1)
        y = np.sort(g.uniform(0, h, size=(n_box, 2)), axis=1)
        bbox = np.stack([x[:, 0], y[:, 0], x[:, 1], y[:, 1]], 1).astype(np.float32 if i % 2 == 0 else np.float64)
        fea = np.minimum(np.floor(np.abs(g.standard_normal((n_box, dim))) * 2.0) / 2.0, 1.5).astype(np.float32)
        recs.append({"path": "scene.v%d/im.%03d.jpg" % (i, i), "features": fea, "bbox": bbox, "image_width": w, "image_height": h})
    return recs


def synthetic_batch(opt, B, seed=7, n_q=30, n_ocr=100, n_od=None, bert_vocab=30522,
                    ragged=False, targets=True):
    """One batch in VQA_collate_fun layout.  ``n_ocr`` / ``n_od`` count items *including*
    the trailing <OCR>/<OD> sentinel (word id 3 / 4, Utils/VQA_Dataset.py:336-349).
    ``ragged=True`` draws a different item count per sample (>= ES_ocr_len + 2)."""
    g = np.random.default_rng(seed)
    V = int(opt["vocab_size"])
    n_od = opt["max_od_num"] if n_od is None else n_od
    Q, Qb = opt["max_q_len"], opt["max_q_bert_len"]
    n_q = min(n_q, Q)

    def fill(rows, width, dtype=np.int64):
        a = np.zeros((len(rows), width), dtype=dtype)
        for i, r in enumerate(rows):
            a[i, :len(r)] = r
        return a

    # ---- question ----
    q_word, q_pos, q_ent, q_bert, q_off = [], [], [], [], []
    for _ in range(B):
        nq = int(g.integers(max(2, n_q - 6), n_q + 1)) if ragged else n_q
        q_word.append(g.integers(5, V, size=nq))
        q_pos.append(g.integers(0, opt["pos_vocab_size"], size=nq))
        q_ent.append(g.integers(0, opt["ent_vocab_size"], size=nq))
        ids, offs = _bertify(g, nq, bert_vocab, Qb, p2=0.3)
        q_bert.append(ids)
        q_off.append(offs)
    q = {}
    q["glove"] = torch.from_numpy(fill(q_word, Q))
    q["glove_mask"] = ~q["glove"].eq(0)
    q["pos"] = torch.from_numpy(fill(q_pos, Q))
    q["ent"] = torch.from_numpy(fill(q_ent, Q))
    q["bert"] = torch.from_numpy(fill(q_bert, Qb))
    q["bert_mask"] = ~q["bert"].eq(0)
    q["bert_offsets"] = q_off

    def items(n_items, max_num, max_len, max_bert_len, sentinel, max_words):
        word, pos, ent, bert, off = [], [], [], [], []
        num_cnt, len_cnt = [], []
        position = np.zeros((B, max_num, 8), dtype=np.float32)
        for b in range(B):
            if ragged and b > 0:      # sample 0 stays at the maximum item count
                lo = min(max_num, opt.get("ES_ocr_len", 0) + 2) if sentinel == 3 else 1
                n = int(g.integers(lo, min(n_items, max_num) + 1))
            else:
                n = min(n_items, max_num)
            lens = []
            for k in range(n):
                last = (k == n - 1)
                nw = 1 if last else int(g.integers(1, max_words + 1))
                nw = min(nw, max_len)
                word.append([sentinel] if last else g.integers(5, V, size=nw))
                pos.append([0] if last else g.integers(0, opt["pos_vocab_size"], size=nw))
                ent.append([0] if last else g.integers(0, opt["ent_vocab_size"], size=nw))
                ids, offs = _bertify(g, nw, bert_vocab, max_bert_len)
                bert.append(ids)
                off.append(offs)
                lens.append(nw)
                if not last:
                    position[b, k] = g.random(8, dtype=np.float32)
            num_cnt.append(n)
            len_cnt.append(lens)
        d = {}
        d["fasttext"] = torch.from_numpy(fill(word, max_len))
        d["pos"] = torch.from_numpy(fill(pos, max_len))
        d["ent"] = torch.from_numpy(fill(ent, max_len))
        d["bert"] = torch.from_numpy(fill(bert, max_bert_len))
        d["bert_offsets"] = off
        d["position"] = torch.from_numpy(position)
        d["fasttext_mask"] = ~d["fasttext"].eq(0)
        if "phoc" in opt["ocr_embedding"].split(","):            # the PHOC table is indexed by the same word ids
            d["phoc"], d["phoc_mask"] = d["fasttext"].clone(), d["fasttext_mask"].clone()
        d["bert_mask"] = ~d["bert"].eq(0)
        d["num_cnt"] = num_cnt
        d["len_cnt"] = len_cnt
        return d

    ocr = items(n_ocr, opt["max_ocr_num"], opt["max_ocr_len"], opt["max_ocr_bert_len"], 3, 3)
    od = items(n_od, opt["max_od_num"], opt["max_od_len"], opt["max_od_bert_len"], 4, 2)

    gt = None
    if targets:
        front = 3 if "label_yesno" in opt else 0          # no_read / yes / no in front of the OCR slots (dataset.py)
        gt = torch.zeros(B, front + opt["max_ocr_num"] + (1 if front == 0 or "label_no_answer" in opt else 0))
        for b in range(B):
            k = int(g.integers(0, max(1, ocr["num_cnt"][b] - 1)))
            # label_yesno: every second sample's answer is one of the three front slots
            gt[b, k % 3 if front and b % 2 else front + k] = 1.0
    extra = [{"q_id": b, "answers": None,
              "ocr_list": ["w%d" % k for k in range(ocr["num_cnt"][b] - 1)] + ["<OCR>"],
              "image_path": "synthetic/%d.jpg" % b} for b in range(B)]
    return q, ocr, od, gt, extra


def set_item_lengths(opt, items, lengths, seed=19, bert_vocab=30522, group="ocr"):
    """Rewrite items of one group of a ``synthetic_batch`` (in place) to the given word counts: ``lengths`` = {item row: words}, rows
    counted over the whole batch, never a sample's trailing sentinel item.  ``synthetic_batch`` draws at most three words per item; the
    reverse direction of a bidirectional multi2one depends on an item's distance to the padded width, so its fixtures need items of
    one word, of the full width ``max_{ocr,od}_len`` and in between.  An item whose words outnumber the word pieces its BERT row can
    hold gets empty piece spans for the surplus, as ``_bertify`` cuts them."""
    g = np.random.default_rng(seed)
    V = int(opt["vocab_size"])
    max_len, max_bert_len = opt["max_%s_len" % group], opt["max_%s_bert_len" % group]
    ends = np.cumsum(items["num_cnt"]) - 1                       # the sentinel rows
    flat_len = [l for sample in items["len_cnt"] for l in sample]
    for row, nw in sorted(lengths.items()):
        if row in ends or not 1 <= nw <= max_len:
            raise ValueError("item %d: a sentinel item, or %d words outside 1 .. %d" % (row, nw, max_len))
        for key, hi in (("fasttext", V), ("pos", opt["pos_vocab_size"]), ("ent", opt["ent_vocab_size"])):
            items[key][row] = 0
            items[key][row, :nw] = torch.from_numpy(g.integers(5 if key == "fasttext" else 0, hi, size=nw))
        ids, offs = _bertify(g, nw, bert_vocab, max_bert_len)
        items["bert"][row] = 0
        items["bert"][row, :len(ids)] = torch.tensor(ids)
        items["bert_offsets"][row] = offs
        flat_len[row] = nw
    items["fasttext_mask"] = ~items["fasttext"].eq(0)
    items["bert_mask"] = ~items["bert"].eq(0)
    if "phoc" in items:
        items["phoc"], items["phoc_mask"] = items["fasttext"].clone(), items["fasttext_mask"].clone()
    it = iter(flat_len)
    items["len_cnt"] = [[next(it) for _ in sample] for sample in items["len_cnt"]]
    return items

