#!/usr/bin/env python3
"""What opt['save_every'] costs the training loop: (a) the per-step time of the steps that do NOT save, with and without the key, and
(b) the wall time of one ``SDNetTrainer.save``.

Bench workload (B = 64, 30-word questions, 100 OCR items, 36 objects, bert-base, fp16c, LOCK_BERT) through ``SDNetTrainer.train()`` over
a loader of 5 warm-up + 40 timed batches - the real loop: step stream, one batch of lookahead, loss read back one step late.  Arm
``nokey`` is the unchanged loop, the yardstick; arm ``save10`` sets ``save_every = 10`` (four saves among the timed steps, to a
temporary folder).  ``update`` and ``save`` are wrapped with a host clock; a step's time is the wall time of its ``update`` call
(in the steady state the host waits there for the previous step's loss).

    python tools/train_state_cost.py [--rounds 3] [--child-timeout 300]

As in tools/es_post_time.py every measurement runs in a FRESH child process, one after the other, each under its own time limit; the
chain stops at the first child that fails; the rounds alternate the order of the arms.  Per arm: the median step of every round and
the median of those.  (a) holds when the steps between saves are not slower than the yardstick by more than the spread (max - min)
the yardstick's own rounds show; (b) is reported, not bounded."""
import argparse
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARMS = ["nokey", "save10"]
BATCH, WARMUP, STEPS, EVERY = 64, 5, 40, 10


def child(arm, steps, warmup):
    import torch
    sys.path.insert(0, ROOT)
    import bench
    from ruart_amd import synth
    from ruart_amd.arguments import default_opt
    dev = torch.device("cuda:0")
    folder = tempfile.mkdtemp(prefix="train_state_cost_")
    opt = default_opt(vocab_size=20000, cuda=True, device=dev, max_od_num=36, batch_size=BATCH, saveFolder=folder)
    if arm == "save10":
        opt["save_every"] = EVERY
    tr, _ = bench.build_trainer(opt, synth.bert_config(), dev)
    host = [synth.synthetic_batch(opt, BATCH, seed=7 + i, n_q=30, n_ocr=100, n_od=36) for i in range(2)]
    step_ms, save_ms, saved_after = [], [], set()
    update, save = tr.update, tr.save

    def timed_update(batch, batch_i=0, **kw):
        t0 = time.perf_counter()
        out = update(batch, batch_i, **kw)
        step_ms.append((time.perf_counter() - t0) * 1e3)
        return out

    def timed_save(*a, **kw):
        t0 = time.perf_counter()
        save(*a, **kw)
        save_ms.append((time.perf_counter() - t0) * 1e3)
        saved_after.add(len(step_ms) - 1)

    tr.update, tr.save = timed_update, timed_save
    try:
        # batch_i counts from 0: with 5 warm-up steps the saves fall after timed steps 4, 14, 24, 34
        tr.train((host[i % 2] for i in range(warmup + steps)), None, log_every=10 ** 9)
        torch.cuda.synchronize()
        timed = step_ms[warmup:]
        # "the steps that do not save": every timed step but the ones a save followed (the save itself is clocked apart)
        plain = sorted(ms for i, ms in enumerate(timed) if (i + warmup) not in saved_after)
        size = os.path.getsize(os.path.join(folder, "train_state.pt")) if save_ms else 0
        res = {"arm": arm, "step_ms_median": round(plain[len(plain) // 2], 3), "steps": len(plain), "saves": len(save_ms),
               "save_ms": [round(v, 1) for v in save_ms], "file_mb": round(size / 2 ** 20, 1),
               "alloc_reserved_mb": round(torch.cuda.memory_reserved(dev) / 2 ** 20, 1)}
    finally:
        tr.close(final=True)
        shutil.rmtree(folder, ignore_errors=True)
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", default=None, help="run ONE arm in this process and print its JSON line")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=STEPS)
    ap.add_argument("--warmup", type=int, default=WARMUP)
    ap.add_argument("--child-timeout", type=int, default=300, help="seconds one child may take")
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.steps, a.warmup)
    results = {m: [] for m in ARMS}
    for r in range(a.rounds):
        for m in (ARMS if r % 2 == 0 else ARMS[::-1]):            # alternate the order: drift of the box does not favour an arm
            cmd = [sys.executable, os.path.abspath(__file__), "--child", m, "--steps", str(a.steps), "--warmup", str(a.warmup)]
            try:
                p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=a.child_timeout)
            except subprocess.TimeoutExpired:
                print("round %d arm %s: no result within %d s - stopping here" % (r, m, a.child_timeout), flush=True)
                return 1
            if p.returncode != 0:
                print("round %d arm %s: exit status %d - stopping here\n%s" % (r, m, p.returncode, p.stderr[-2000:]), flush=True)
                return 1
            res = json.loads(p.stdout.strip().splitlines()[-1])
            res["round"] = r
            results[m].append(res)
            print(json.dumps(res), flush=True)
    med = {m: sorted(x["step_ms_median"] for x in results[m])[len(results[m]) // 2] for m in ARMS}
    print("\n(a) steps that do not save: median ms per step")
    print("arm      per round                      median   vs nokey")
    for m in ARMS:
        ms = [x["step_ms_median"] for x in results[m]]
        print("%-7s  %-30s %7.3f  %+8.3f" % (m, " ".join("%.3f" % v for v in ms), med[m], med[m] - med["nokey"]))
    base = [x["step_ms_median"] for x in results["nokey"]]
    spread = max(base) - min(base)
    slower = med["save10"] - med["nokey"]
    print("spread of the nokey rounds (max - min): %.3f ms; save10 - nokey: %+.3f ms  =>  (a) %s"
          % (spread, slower, "holds" if slower <= spread else "FAILS"))
    saves = sorted(v for x in results["save10"] for v in x["save_ms"])
    print("\n(b) one save: median %.1f ms (min %.1f, max %.1f, %d saves), file %.1f MB"
          % (saves[len(saves) // 2], saves[0], saves[-1], len(saves), results["save10"][0]["file_mb"]))
    print("allocator reserved at the end, MB: nokey %s, save10 %s" % (" ".join("%.0f" % x["alloc_reserved_mb"] for x in results["nokey"]),
                                                                       " ".join("%.0f" % x["alloc_reserved_mb"] for x in results["save10"])))
    return 0


if __name__ == "__main__":
    sys.exit(main())
