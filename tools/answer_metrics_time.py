#!/usr/bin/env python3
"""Time of the answer metrics at the evaluation shape: B = 64 samples, 100 OCR candidates each, 10 (and 2) answers per question; code
points drawn uniformly from a-z and blank, seeded.

    python tools/answer_metrics_time.py [--repeats 9] [--warmup 3] [--parent-trainer FILE] [--host-only]

One process, medians over ``--repeats`` runs after ``--warmup``; every timed call ends with the readback it needs anyway (the decode) or
a device synchronise (the table).  Per shape:

  decode           one ``trainer.decode_predictions`` call on CUDA scores (B, 101), ``label_no_answer`` on: candidates of 3-25 code points
  decode (parent)  the same call through ``--parent-trainer``: a copy of the parent commit's ruart_amd/trainer.py
                   (``git show <parent>:ruart_amd/trainer.py > FILE``), loaded beside the package - the host loop the table replaces
  decode (cpu)     the same call on CPU scores (today's host path, for orientation)
  table            ``metrics.answer_table`` alone, 100 candidates of 2-20 code points against every answer (64 000 pairs at 10 answers):
                   total, and the share of it that is host packing (``pack_answer_table``)

``--host-only`` (no GPU): the two host figures of the same shapes - the metric calls of one decode batch, and the full table through
``note_stvqa`` / ``note_textvqa`` per cell."""
import argparse
import importlib.util
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
B, N_CAND = 64, 100
ALPHABET = "abcdefghijklmnopqrstuvwxyz "


def words(rng, n, lo, hi):
    return ["".join(rng.choice(ALPHABET) for _ in range(rng.randint(lo, hi))) for _ in range(n)]


def make_shape(n_answers, cand_len, seed=7):
    rng = random.Random(seed)
    return [{"q_id": b, "answers": words(rng, n_answers, 3, 25), "ocr_list": words(rng, N_CAND - 1, *cand_len) + ["<OCR>"],
             "image_path": "x"} for b in range(B)]


def median_ms(fn, repeats, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return round(statistics.median(ts), 3)


def load_parent(path):
    spec = importlib.util.spec_from_file_location("ruart_amd._parent_trainer", path)
    mod = importlib.util.module_from_spec(spec)
    mod.__package__ = "ruart_amd"
    spec.loader.exec_module(mod)
    return mod


def host_figures(repeats, warmup):
    from ruart_amd.metrics import note_stvqa, note_textvqa
    for n_answers in (10, 2):
        rng = random.Random(3)
        extra = make_shape(n_answers, (3, 25))
        picks = [rng.choice(e["ocr_list"][:-1]) for e in extra]
        one = lambda: [(note_stvqa(e["answers"], w), note_textvqa(e["answers"], w)) for e, w in zip(extra, picks)]
        extra_t = make_shape(n_answers, (2, 20))
        full = lambda: [[(note_stvqa(e["answers"], w), note_textvqa(e["answers"], w)) for w in e["ocr_list"]] for e in extra_t]
        print(json.dumps({"answers": n_answers, "host_decode_metric_calls_ms": median_ms(one, repeats, warmup),
                          "host_full_table_ms": median_ms(full, max(1, repeats // 3), 1)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--parent-trainer", default=None)
    ap.add_argument("--host-only", action="store_true")
    a = ap.parse_args()
    if a.host_only:
        return host_figures(a.repeats, a.warmup)
    import torch
    from ruart_amd import metrics
    from ruart_amd.trainer import decode_predictions
    dev = torch.device("cuda:0")
    parent = load_parent(a.parent_trainer) if a.parent_trainer else None
    opt = {"label_no_answer": True}
    for n_answers in (10, 2):
        extra = make_shape(n_answers, (3, 25))
        gen = torch.Generator().manual_seed(5)
        scores_h = torch.rand(B, N_CAND + 1, generator=gen)
        scores = scores_h.to(dev)
        counts = [N_CAND] * B
        row = {"answers": n_answers, "pairs_in_table": B * (N_CAND + 1) * n_answers}
        want = decode_predictions(scores_h, counts, extra, opt)
        got = decode_predictions(scores, counts, extra, opt)
        assert got == want, "device decode differs from the CPU path"
        row["decode_ms"] = median_ms(lambda: decode_predictions(scores, counts, extra, opt), a.repeats, a.warmup)
        if parent is not None:
            assert parent.decode_predictions(scores, counts, extra, opt) == want
            row["decode_parent_ms"] = median_ms(lambda: parent.decode_predictions(scores, counts, extra, opt), a.repeats, a.warmup)
        row["decode_cpu_scores_ms"] = median_ms(lambda: decode_predictions(scores_h, counts, extra, opt), a.repeats, a.warmup)
        extra_t = make_shape(n_answers, (2, 20))
        cands, answers = [e["ocr_list"] for e in extra_t], [e["answers"] for e in extra_t]

        def table():
            out = metrics.answer_table(cands, answers, dev)
            torch.cuda.synchronize()
            return out

        row["table_ms"] = median_ms(table, a.repeats, a.warmup)
        row["table_pack_ms"] = median_ms(lambda: metrics.pack_answer_table(cands, answers), a.repeats, a.warmup)
        row["table_pack_share"] = round(row["table_pack_ms"] / row["table_ms"], 3)
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    sys.exit(main())
