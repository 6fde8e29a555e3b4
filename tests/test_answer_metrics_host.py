"""Host side of the answer table (ruart_amd/metrics.py): string packing, the tensor label rule against ``VQA_Dataset.get_label``, the
dataset / collate route of opt['label_from_answers'], and the argument checks of ``ruart_edit_distance_pairs`` (which run before
anything is launched and need no device)."""
import copy
import ctypes
import gzip
import json
import os
import re

import numpy as np
import pytest
import torch

from ruart_amd import hip, metrics
from ruart_amd.arguments import default_opt
from ruart_amd.metrics import note_stvqa, note_textvqa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = 1          # hipErrorInvalidValue
OCR_SOURCES = ("ocr_PMTD_ASTER", "ocr_PMTD_ASTER_gram2", "ES_ocr")


# -- packing -------------------------------------------------------------------------------------------------------------
def unpack(chars, off):
    return ["".join(map(chr, chars[off[i]:off[i + 1]])) for i in range(len(off) - 1)]


def test_pack_strings_round_trips_offsets_and_code_points():
    strings = ["stop", "", "café au lait", "\U0001F600x", "", "中国", "i̇"]
    chars, off = metrics.pack_strings(strings)
    assert chars.dtype == np.int32 and off.dtype == np.int32
    assert off.tolist() == [0] + np.cumsum([len(s) for s in strings]).tolist() and len(chars) == off[-1]
    assert unpack(chars, off) == strings
    assert chars[off[3]] == 0x1F600                      # a code point above U+FFFF is ONE unit, not a surrogate pair
    chars, off = metrics.pack_strings([])
    assert off.tolist() == [0] and len(chars) == 0
    chars, off = metrics.pack_strings(["", ""])
    assert off.tolist() == [0, 0, 0] and len(chars) == 0


def sections(pack):
    buf, out, o = pack["buf"].numpy(), {}, 0
    for name, n in zip(metrics._SECTIONS, pack["sizes"]):
        out[name] = buf[o:o + n]
        o += n
    assert o == len(buf)
    return out


def test_pack_answer_table_lowers_with_str_lower_and_lists_every_pair():
    """``str.lower()`` can change a string's length (U+0130 becomes two code points): lengths and offsets are those of the lowered
    strings.  The candidate flags carry ``word == word.lower()`` (note_textvqa does not lower-case the word)."""
    cands = [["İstanbul", "stop", ""], ["\U0001F600", "STOP"]]
    answers = [["ISTANBUL", "stop"], None]
    assert len("İ".lower()) == 2
    pack = metrics.pack_answer_table(cands, answers)
    s = sections(pack)
    strings = unpack(s["chars"], s["off"])
    assert strings == ["i̇stanbul", "stop", "", "\U0001F600", "stop", "istanbul", "stop"]
    assert (pack["B"], pack["Cmax"], pack["Amax"], pack["n_pairs"]) == (2, 3, 2, 6) and pack["patch"] is None
    pairs = list(zip(s["pair_a"].tolist(), s["pair_b"].tolist()))
    assert pairs == [(0, 5), (0, 6), (1, 5), (1, 6), (2, 5), (2, 6)]            # sample 1 has no answers: no pairs
    assert s["flat"].tolist() == [0, 1, 2, 3, 4, 5]
    assert s["maxlen"].tolist() == [9, 9, 8, 4, 8, 4]
    assert s["flag"].tolist() == [1, 3, 3, 3, 1, 0]      # "İstanbul" and "STOP" are not their own lower(); the last slot is padding


def test_pack_answer_table_scores_over_cap_pairs_on_the_host():
    long = "a" * (metrics.EDIT_MAX_LEN + 1)
    pack = metrics.pack_answer_table([["ab", long]], [["ab", long[:-1] + "b"]])
    s = sections(pack)
    assert pack["n_pairs"] == 1 and s["pair_a"].tolist() == [0] and s["pair_b"].tolist() == [2]
    flat, score, eq = pack["patch"]
    assert flat.tolist() == [1, 2, 3] and eq.tolist() == [0, 0, 0]
    assert score.tolist() == [metrics.stvqa_score(long[:-1] + "b", "ab"), metrics.stvqa_score("ab", long),
                              metrics.stvqa_score(long[:-1] + "b", long)]
    with open(os.path.join(ROOT, "include", "ruart_hip.h")) as f:
        cap = int(re.search(r"#define\s+RUART_EDIT_MAX_LEN\s+(\d+)", f.read()).group(1))
    assert cap == metrics.EDIT_MAX_LEN >= 128


def test_answer_table_refuses_a_cpu_device():
    with pytest.raises(hip.HipError):
        metrics.answer_table([["a"]], [["a"]], "cpu")


# -- the label rule ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fixture(golden_dir, tmp_path_factory):
    with open(os.path.join(golden_dir, "dataset_input.json"), encoding="utf-8") as f:
        inp = json.load(f)
    vocab = tmp_path_factory.mktemp("vocab") / "vocab.txt"
    vocab.write_text("\n".join(inp["vocab"]) + "\n", encoding="utf-8")
    return inp, str(vocab)


def twins(records):
    """(scored, stripped): the score fields filled in with the host functions on the string the dataset holds (lower-cased), and
    the same records without them.  A few strings are planted so that every branch of the rule is met: an exact answer twice (a tie
    for the maximum), a record whose candidates are all far from its answer (best < 0.1), near misses around the thresholds."""
    scored = copy.deepcopy(records)
    for k, rec in enumerate(scored):
        if k % 3 == 0:
            rec["orign_answers"] = ["stop", "Stop sign", "stop"]
            items = rec["ocr_PMTD_ASTER"]
            items[0]["original"], items[-1]["original"] = "STOP", "stop"
            if len(items) > 2:
                items[1]["original"] = "stoq"
        elif k % 3 == 1:
            rec["orign_answers"] = ["qqqqqqqqqqqqqqqqqqqqqqqqqqqqqqqqqqqqqqqqqqqq"]
        for name in OCR_SOURCES:
            for item in rec.get(name, []):
                word = item["original"].lower()
                item["ANLS"], item["ACC"] = note_stvqa(rec["orign_answers"], word), note_textvqa(rec["orign_answers"], word)
    stripped = copy.deepcopy(scored)
    for rec in stripped:
        for name in OCR_SOURCES:
            for item in rec.get(name, []):
                del item["ANLS"], item["ACC"]
    return scored, stripped


def host_table(extra, opt):
    note = note_stvqa if opt["score_name"] == "ANLS" else note_textvqa
    cands = metrics.label_candidates(extra, opt)
    table = torch.zeros(len(cands), max(len(c) for c in cands), dtype=torch.float64)
    for b, c in enumerate(cands):
        for i, w in enumerate(c):
            table[b, i] = note(extra[b]["answers"], w)
    return table, [len(c) for c in cands]


WAYS = ("lable_all_with_threshold", "lable_one_offical", "lable_one", "lable_all")


@pytest.mark.parametrize("score_name", ["ANLS", "ACC"])
@pytest.mark.parametrize("way", WAYS)
@pytest.mark.parametrize("yesno,no_answer", [(False, True), (True, False), (True, True), (False, False)])
def test_tensor_label_rule_equals_get_label(fixture, way, score_name, yesno, no_answer):
    """``labels_from_table`` fed a table of host ``note_*`` values equals ``VQA_Dataset.get_label`` on the scored twins bit for bit -
    and the stripped twins travel through the dataset and the collate without a target, with the packed strings instead."""
    from ruart_amd.batch import VQA_collate
    from ruart_amd.dataset import VQA_Dataset
    inp, vocab = fixture
    opt = default_opt(datadir="", BERT_tokenizer_file=vocab, lable_way=way, score_name=score_name)
    opt.pop("label_no_answer", None)
    if no_answer:
        opt["label_no_answer"] = True
    if yesno:
        opt["label_yesno"] = True
    scored, stripped = twins(inp["records"])
    want = [s["gt"] for s in (lambda ds: [ds[i] for i in range(len(ds))])(VQA_Dataset(scored, opt))]
    opt2 = dict(opt, label_from_answers=True)
    ds = VQA_Dataset(stripped, opt2)
    samples = [ds[i] for i in range(len(ds))]
    assert all(s["gt"] is None for s in samples)
    q, ocr, od, gt, extra = VQA_collate(opt2).VQA_collate_fun(samples)
    assert gt is None
    pack = q["_ruart_label_pack"]
    assert pack["n_scored"].tolist() == [(3 if yesno else 0) + len(e["ocr_list"]) - 1 for e in extra]
    table, n_scored = host_table(extra, opt2)
    got = metrics.labels_from_table(table, n_scored, opt2)
    want = torch.cat(want, dim=0)
    assert got.dtype == torch.float32 and got.shape == want.shape == (len(samples), (3 if yesno else 0) + opt["max_ocr_num"] + int(no_answer))
    assert torch.equal(got, want)
    # the planted cases are there: a tie for the maximum (the first wins), a best below 0.1, the sentinel's zero inside the list
    width = got.shape[1] - int(no_answer)
    if score_name == "ANLS":
        best = torch.stack([table[b, :n].max() for b, n in enumerate(n_scored)])
        assert (best < 0.1).any() and (best == 1).any()
        tie = [b for b, n in enumerate(n_scored) if (table[b, :n] == 1).sum() >= 2]
        assert tie
        if way == "lable_one":
            for b in tie:
                first = int((table[b] == 1).nonzero()[0])
                assert got[b, first] == 1 and got[b, :width].sum() == 1
        if no_answer:
            assert got[:, -1].tolist() == (best < 0.1).float().tolist()
    for b, n in enumerate(n_scored):
        assert got[b, n:width].abs().sum() == 0


def test_unscored_records_without_the_key_behave_as_before(fixture):
    from ruart_amd.dataset import VQA_Dataset
    inp, vocab = fixture
    opt = default_opt(datadir="", BERT_tokenizer_file=vocab)
    _, stripped = twins(inp["records"])
    assert VQA_Dataset(stripped, opt)[0]["gt"] == (None, None)


def test_labels_from_table_refuses_a_table_wider_than_the_slots():
    opt = {"max_ocr_num": 4, "lable_way": "lable_all", "score_name": "ANLS"}
    with pytest.raises(ValueError):
        metrics.labels_from_table(torch.zeros(1, 4, dtype=torch.float64), [4], opt)
    with pytest.raises(AssertionError):
        metrics.labels_from_table(torch.zeros(1, 3, dtype=torch.float64), [3], dict(opt, lable_way="other"))


# -- C ABI refusals --------------------------------------------------------------------------------------------------------
def test_edit_distance_argument_errors_return_invalid_value_before_any_launch():
    """No device here: a call that got as far as a launch would fail with another code (or crash on the fake pointers)."""
    lib = hip.load()
    p = ctypes.c_void_p(4096)          # never dereferenced on the host, never launched with

    def call(ptrs=(p,) * 6, n_chars=8, n_str=2, n_pairs=3):
        chars, off, pa, pb, dist, eq = ptrs
        return lib.ruart_edit_distance_pairs(chars, n_chars, off, n_str, pa, pb, n_pairs, dist, eq, None)

    for j in range(6):
        assert call(ptrs=tuple(None if i == j else p for i in range(6))) == INVALID, j
        assert call(ptrs=tuple(None if i == j else p for i in range(6)), n_pairs=0) == INVALID, j
    for bad in (dict(n_chars=-1), dict(n_str=-1), dict(n_pairs=-1), dict(n_str=0), dict(n_str=-1, n_pairs=0), dict(n_chars=-1, n_pairs=0)):
        assert call(**bad) == INVALID, bad
    assert call(n_pairs=0) == 0
    assert call(n_pairs=0, n_str=0, n_chars=0) == 0
    with pytest.raises(hip.HipError):
        hip.kernels().ruart_edit_distance_pairs(None, 0, p, 1, p, p, 1, p, p, None)
