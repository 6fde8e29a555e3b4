"""opt['bert_train_layers'] = N (train only the top N encoder layers): the pure parts - the switch's validation and the cut it yields
(bert.train_layer_split), and the key set of the prediction checkpoint (trainer.predict_checkpoint_keys).  No GPU."""
import pytest

from ruart_amd.bert import train_layer_split
from ruart_amd.trainer import predict_checkpoint_keys


def _opt(**kw):
    opt = {"BERT": True, "BERT_LINEAR_COMBINE": True, "bert_train_gemm": "16"}
    opt.update(kw)
    return opt


def test_absent_key_is_todays_path_whatever_else_the_conf_says():
    assert train_layer_split({"LOCK_BERT": True}, 12) == 0
    assert train_layer_split({"bert_train_gemm": "x3", "bert_no_pack": True}, 12) == 0
    assert train_layer_split({}, 24) == 0


@pytest.mark.parametrize("n,k", [(1, 11), (2, 10), (12, 0)])
def test_cut_for_bert_base(n, k):
    assert train_layer_split(_opt(bert_train_layers=n), 12) == k


def test_cut_for_bert_large_and_a_conf_file_value():
    assert train_layer_split(_opt(bert_train_layers=4), 24) == 20
    assert train_layer_split(_opt(bert_train_layers=2, bert_train_gemm=16), 12) == 10      # `bert_train_gemm 16` read from a conf is an int


@pytest.mark.parametrize("extra", [
    {"bert_train_layers": 0},
    {"bert_train_layers": -1},
    {"bert_train_layers": 13},
    {"bert_train_layers": True},                 # a bare key in a conf file
    {"bert_train_layers": 2.0},
    {"bert_train_layers": "2"},
    {"bert_train_layers": 2, "LOCK_BERT": True},
    {"bert_train_layers": 12, "LOCK_BERT": True},
    {"bert_train_layers": 2, "bert_train_gemm": "x3"},
    {"bert_train_layers": 2, "bert_train_gemm": "16gemm"},
    {"bert_train_layers": 2, "bert_no_pack": True},
])
def test_refusals_name_the_key(extra):
    opt = _opt(**extra)
    with pytest.raises(ValueError, match="bert_train_layers"):
        train_layer_split(opt, 12)


def test_missing_train_gemm_is_refused():
    opt = _opt(bert_train_layers=2)
    del opt["bert_train_gemm"]                   # the default is the fp32-class graph
    with pytest.raises(ValueError, match="bert_train_layers"):
        train_layer_split(opt, 12)


_KEYS = ["vocab_embed.weight", "alphaBERT", "gammaBERT", "eval_embed.weight", "fixed_embedding_fast", "fixed_embedding_glove",
         "Bert.bert_model.embeddings.word_embeddings.weight", "Bert.bert_model.encoder.layer.0.output.dense.weight",
         "Bert.bert_model.encoder.layer.10.attention.self.query.weight", "Bert.bert_model.encoder.layer.11.output.LayerNorm.beta",
         "CoVe.rnn.weight", "get_answer.attn.linear.weight"]
_TODAY = ["vocab_embed.weight", "alphaBERT", "gammaBERT", "get_answer.attn.linear.weight"]
_TRAINED = ["alphaBERT", "gammaBERT", "get_answer.attn.linear.weight", "Bert.bert_model.encoder.layer.10.attention.self.query.weight",
            "Bert.bert_model.encoder.layer.11.output.LayerNorm.beta"]


def test_checkpoint_keys_without_the_key_are_todays():
    assert predict_checkpoint_keys(_KEYS, {}, _TRAINED) == _TODAY
    assert predict_checkpoint_keys(_KEYS, {"bert_train_gemm": "16"}, _TRAINED) == _TODAY       # full unlock: the reference's habit stays


def test_checkpoint_keys_with_the_key_add_the_trained_encoder_tensors_only():
    got = predict_checkpoint_keys(_KEYS, _opt(bert_train_layers=2), _TRAINED)
    assert got == ["vocab_embed.weight", "alphaBERT", "gammaBERT", "Bert.bert_model.encoder.layer.10.attention.self.query.weight",
                   "Bert.bert_model.encoder.layer.11.output.LayerNorm.beta", "get_answer.attn.linear.weight"]
    assert not any(k.startswith("Bert.bert_model.embeddings") or ".layer.0." in k for k in got)
    # a trained name outside Bert.bert_model.* does not bring a dropped key back
    assert "eval_embed.weight" not in predict_checkpoint_keys(_KEYS, _opt(bert_train_layers=2), _TRAINED + ["eval_embed.weight", "CoVe.rnn.weight"])
