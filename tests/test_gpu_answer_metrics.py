"""The answer table on a real MI355X: ``ruart_edit_distance_pairs`` (exact integers), ``metrics.answer_table`` (bit-equal float64),
the decode's device route against its CPU route, opt['eval_upper_bound'] and opt['label_from_answers'].  The host functions of
ruart_amd/metrics.py are the reference throughout."""
import copy
import json
import os
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from ruart_amd import hip, metrics, synth                                  # noqa: E402
from ruart_amd.arguments import default_opt                                # noqa: E402
from ruart_amd.metrics import note_stvqa, note_textvqa, stvqa_score        # noqa: E402

DEV = "cuda:0"
CAP = metrics.EDIT_MAX_LEN


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def host_distance(a, b):
    """The integer inside ``stvqa_score``: ld = (1 - score) * max(len), exactly an integer up to rounding far below 1/2."""
    m = max(len(a), len(b))
    if m == 0:
        return 0
    assert a == a.lower() and b == b.lower()
    return round((1 - stvqa_score(a, b)) * m)


def run_pairs(chars, off, pair_a, pair_b):
    """One launch on buffers of exactly the stated sizes; -> (dist, equal) as lists."""
    d = lambda a: torch.tensor(np.asarray(a, dtype=np.int32), device=DEV)
    n_pairs = len(pair_a)
    dist = torch.full((n_pairs,), -7, dtype=torch.int32, device=DEV)
    eq = torch.full((n_pairs,), -7, dtype=torch.int32, device=DEV)
    bufs = d(chars if len(chars) else [0]), d(off), d(pair_a), d(pair_b)
    hip.kernels().ruart_edit_distance_pairs(bufs[0], len(chars), bufs[1], len(off) - 1, bufs[2], bufs[3], n_pairs, dist, eq,
                                            hip.stream_ptr(torch.device(DEV)))
    torch.cuda.synchronize()
    return dist.tolist(), eq.tolist()


def edge_pairs():
    rng = random.Random(5)
    word = lambda n, alphabet="abc ": "".join(rng.choice(alphabet) for _ in range(n))
    pairs = [("", ""), ("", "abc"), ("abc", ""), ("a", "a"), ("a", "b"), ("a", "ba"), ("stop", "stop"), ("aaaa", "aa"), ("aa", "aaaa"),
             ("aaaa", "aaaa"), ("\U0001F600\U00020000x", "\U0001F600\U00020001x"), ("\U0001F600", "\ud83d"), ("\U00010000", "\x00")]
    for la in (63, 64, 65):                               # the lane-block boundary, along either string
        for lb in (1, 64, 65):
            a, b = word(la), word(lb)
            pairs += [(a, b), (b, a)]
        a = word(la)
        pairs += [(a, a), (a, a[:-1] + "z"), (a, "z" + a[1:]), (a[1:], a)]
    full = word(CAP)                                      # the cap exactly
    pairs += [(full, full), (full, word(CAP)), (full, "a"), ("", full), (full, full[1:] + "q"), (word(CAP, "ab"), word(CAP - 1, "ab"))]
    return pairs


def test_edit_distance_pairs_exact_on_seeded_and_edge_pairs():
    rng = random.Random(11)
    alphabet = "abcdefghijklmnopqrstuvwxyz "
    pairs = edge_pairs()
    for k in range(300):                                  # the shape of the data: 3-25 code points, some near-duplicates
        a = "".join(rng.choice(alphabet) for _ in range(rng.randint(3, 25)))
        if k % 4 == 0:
            cut = rng.randrange(len(a))
            b = a[:cut] + rng.choice(alphabet) + a[cut + rng.randint(0, 1):]
        elif k % 7 == 0:
            b = a
        else:
            b = "".join(rng.choice(alphabet if k % 3 else "ab") for _ in range(rng.randint(2, 40)))
        pairs.append((a, b))
    strings = sorted(set(s for p in pairs for s in p))
    index = {s: i for i, s in enumerate(strings)}
    chars, off = metrics.pack_strings(strings)
    dist, eq = run_pairs(chars, off, [index[a] for a, _ in pairs], [index[b] for _, b in pairs])
    want = [host_distance(a, b) for a, b in pairs]
    bad = [(a, b, g, w) for (a, b), g, w in zip(pairs, dist, want) if g != w]
    assert not bad, bad[:5]
    assert eq == [int(a == b) for a, b in pairs]


def test_bad_indices_give_minus_one_and_nothing_else_changes():
    """The contract for index arrays that do not describe the buffers - every pair handed in still lies inside buffers of the stated
    sizes: a string index equal to n_str, a string whose offsets run backwards, a string longer than the cap."""
    strings = ["stop", "shop", "", "a" * (CAP + 1), "stoop", "st"]
    chars, off = metrics.pack_strings(strings)
    off = off.copy()
    n_str = len(strings)
    off[1] = off[2] + 1                      # string 1's offsets run backwards; string 0 = chars[0 : off[1]) now runs on to "stopshopa"
    assert off[1] > off[2] and 0 <= off[1] <= len(chars)                # (inside the buffer: this is not a fault test)
    s0 = "".join(map(chr, chars[off[0]:off[1]]))
    assert s0 == "stopshopa"
    pair_a = [4, n_str, 0, 1, 5, 0, 3, 2, -1]
    pair_b = [5, 0, n_str, 5, 1, 4, 4, 2, 0]
    dist, eq = run_pairs(chars, off, pair_a, pair_b)
    want = [host_distance("stoop", "st"), -1, -1, -1, -1, host_distance(s0, "stoop"), -1, 0, -1]
    assert dist == want
    assert eq == [0, 0, 0, 0, 0, 0, 0, 1, 0]


def test_answer_table_is_bit_equal_to_the_host_functions():
    long = "the quick brown fox " * 7            # 140 code points: over the cap, scored on the host and patched in
    assert len(long) > CAP
    cands = [["stop", "Stop", "st0p", "", "İstanbul", "i̇stanbul"],
             ["yes"],
             ["coca cola", "cola", long, long[:-1], "COLA"] + ["w%d" % k for k in range(9)],
             ["a", "b"]]
    answers = [["stop", "STOP", "İSTANBUL", ""],
               None,
               ["coca cola", "Coca-Cola", "cola", "coca cola", "coke", "coca", "cocacola", "coca cola", "the coca cola", long],
               []]
    assert len(answers[2]) == 10
    anls, acc = metrics.answer_table(cands, answers, DEV)
    assert anls.dtype == acc.dtype == torch.float64 and anls.shape == acc.shape == (4, 14) and anls.device.type == "cuda"
    anls, acc = anls.cpu(), acc.cpu()
    for b, cs in enumerate(cands):
        for i, w in enumerate(cs):
            if answers[b] is None:
                want_a, want_c = -1, 0.0
            else:
                want_a, want_c = note_stvqa(answers[b], w), note_textvqa(answers[b], w)
            assert anls[b, i].item() == want_a and acc[b, i].item() == want_c, (b, i, w, anls[b, i].item(), want_a, acc[b, i].item(), want_c)
        assert anls[b, len(cs):].abs().sum() == 0 and acc[b, len(cs):].abs().sum() == 0
    assert acc[0, 1] == 0 and acc[0, 0] == 0.2          # an upper-case letter in the word: note_textvqa counts nothing
    assert acc[2, 2] == 0.1 and anls[2, 2] == 1          # the over-cap string meets itself among the answers


def test_answer_table_quotients_are_correctly_rounded():
    """Every quotient ld / n with n <= 24 (sample n: "a" * i + "b" * (n - i) against "a" * n), and every count / 10: the float64 finish
    on the device must round as Python's ``1 - ld / max(len)`` and ``count / 10.0`` do (a reciprocal product would not)."""
    cands = [["a" * i + "b" * (n - i) for i in range(n + 1)] for n in range(1, 25)]
    answers = [["a" * n] * min(n, 10) for n in range(1, 25)]
    anls, acc = (t.cpu() for t in metrics.answer_table(cands, answers, DEV))
    for b, cs in enumerate(cands):
        assert anls[b, :len(cs)].tolist() == [note_stvqa(answers[b], w) for w in cs]
        assert acc[b, :len(cs)].tolist() == [note_textvqa(answers[b], w) for w in cs]
    assert sorted(set(acc.flatten().tolist())) == [k / 10.0 for k in range(11)]


@pytest.mark.parametrize("fixture,variant", [("predict_decode.json", "plain"), ("predict_decode.json", "no_answer"),
                                             ("predict_decode_yesno.json", "plain"), ("predict_decode_yesno.json", "no_answer")])
def test_decode_on_device_scores_equals_the_cpu_path(golden_dir, fixture, variant):
    from ruart_amd.trainer import decode_predictions, decode_slots
    with open(os.path.join(golden_dir, fixture)) as f:
        z = json.load(f)
    cases = z["cases"]
    width = z["n_slots"] if variant == "no_answer" else z["n_slots"] - 1
    scores = torch.tensor([c["prob"][:width] for c in cases])
    extra = [{"q_id": c["q_id"], "answers": c["answers"], "ocr_list": c["ocr_list"], "image_path": "x"} for c in cases]
    opt = {"label_no_answer": True} if variant == "no_answer" else {}
    decode = decode_predictions
    if "yesno" in fixture:
        opt["label_yesno"] = True
        decode = decode_slots
    counts = [c["num_cnt"] for c in cases]
    bound_h, bound_d = [], []
    want = decode(scores, counts, extra, opt, bound=bound_h)
    got = decode(scores.to(DEV), counts, extra, opt, bound=bound_d)
    assert got[2] == want[2] and got[3] == want[3]
    assert got[0] == want[0] and got[1] == want[1]                       # the two sums: equal floats, not close ones
    assert any(e["answers"] is not None for e in extra) and want[0] > 0
    assert bound_d == bound_h and len(bound_d) == len(cases)
    assert decode(scores.to(DEV), counts, extra, opt)[:2] == want[:2]


def small_trainer(**extra):
    from ruart_amd.trainer import SDNetTrainer
    opt = default_opt(vocab_size=1500, cuda=True, DROPOUT=0.0, dropout_emb=0.0, **extra)
    cfg = synth.bert_config(vocab_size=2000)
    opt["bert_state"], opt["bert_config"] = synth.make_bert_weights(cfg, seed=1033), cfg
    sw = synth.make_sdnet_weights(opt, seed=1033)
    tr = SDNetTrainer(opt, device=DEV)
    tr.setup_model({"glove_embedding": T(sw["glove_embed.weight"]), "fast_embedding": T(sw["fast_embed.weight"])})
    return tr, opt


def worded_batch(opt, B, seed):
    """A synthetic batch whose ``extra_info`` carries answers and real strings (``ocr_list`` keeps its length, the sentinel its place)."""
    rng = random.Random(seed)
    batch = list(synth.synthetic_batch(opt, B, seed=seed, n_q=10, n_ocr=20, n_od=5, bert_vocab=2000, ragged=True))
    vocab = ["stop", "shop", "coca cola", "cola", "exit", "exit 12", "12", "main st", "main street", "open", "yes", "no"]
    for b, e in enumerate(batch[4]):
        n = len(e["ocr_list"]) - 1
        e["ocr_list"] = [rng.choice(vocab) for _ in range(n)] + ["<OCR>"]
        if b == 0:
            e["answers"] = [rng.choice(vocab) for _ in range(10)]
        elif b == 1:
            e["answers"] = ["Main Street", "main st."]
        else:
            e["answers"] = ["zzzzzzzzzzzzzzzzzzzzzzzzzzzzzz"]
    return batch


def test_eval_upper_bound_equals_the_host_bound():
    from ruart_amd.trainer import _credit
    tr, opt = small_trainer(eval_upper_bound=True)
    try:
        batch = worded_batch(opt, 3, seed=31)
        loss, anls, acc, res = tr.evaluate([copy.deepcopy(batch)])
        got = tr.eval_bound
        want_a = want_c = 0
        for b, e in enumerate(batch[4]):
            n = int(batch[1]["num_cnt"][b])
            slots = [s for s in range(n) if s != len(e["ocr_list"]) - 1]
            words = [e["ocr_list"][s] for s in slots] + (["unanswerable"] if "label_no_answer" in opt else [])
            credit = [_credit(note_stvqa(e["answers"], w), note_textvqa(e["answers"], w), len(e["answers"])) for w in words]
            want_a, want_c = want_a + max(c[0] for c in credit), want_c + max(c[1] for c in credit)
        assert got == {"ANLS": want_a / 3, "ACC": want_c / 3}
        assert got["ANLS"] >= anls and got["ACC"] >= acc and got["ANLS"] > 0
        tr.opt.pop("eval_upper_bound")
        assert tr.evaluate([copy.deepcopy(batch)])[1:3] == (anls, acc)
        assert not hasattr(tr, "eval_bound")
    finally:
        tr.close(final=True)


def test_label_from_answers_update_uses_the_get_label_targets(golden_dir, tmp_path):
    """Stripped records: the collate's pack -> ``ToCUDA`` -> the targets one ``update()`` trains on, bit-equal to ``get_label`` on the
    scored twins (score fields filled in with the host functions)."""
    from ruart_amd.dataset import VQA_Dataset
    tr, opt = small_trainer(label_from_answers=True)
    try:
        batch = worded_batch(opt, 3, seed=32)
        extra = batch[4]
        with open(os.path.join(golden_dir, "dataset_input.json"), encoding="utf-8") as f:
            vocab = tmp_path / "vocab.txt"
            vocab.write_text("\n".join(json.load(f)["vocab"]) + "\n", encoding="utf-8")
        ds = VQA_Dataset([], dict(opt, datadir="", BERT_tokenizer_file=str(vocab)))
        want = []
        for e in extra:
            items = [{"original": w, "ANLS": note_stvqa(e["answers"], w), "ACC": note_textvqa(e["answers"], w)} for w in e["ocr_list"][:-1]]
            items.append({"original": "<OCR>", "ANLS": 0.0, "ACC": 0.0})
            want.append(ds.get_label(items, answers=e["answers"]))
        want = torch.cat(want, dim=0)
        batch[0]["_ruart_label_pack"] = metrics.pack_label_table(extra, opt)          # what VQA_collate attaches
        batch[3] = None
        shipped = tr.ToCUDA(batch)
        assert shipped[3].device.type == "cuda" and shipped[3].dtype == torch.float32
        assert torch.equal(shipped[3].cpu(), want)
        assert want.sum() > 0 and want[2, :-1].sum() == 0 and want[2, -1] == 1       # sample 2: nothing near its answer -> no-answer
        seen = []
        inner = tr.loss_func
        tr.loss_func = lambda scores, labels: seen.append(labels) or inner(scores, labels)
        assert np.isfinite(float(tr.update(shipped, 0)))
        assert len(seen) == 1 and torch.equal(seen[0].cpu(), want)
    finally:
        tr.close(final=True)
