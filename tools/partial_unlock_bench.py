#!/usr/bin/env python3
"""Training-step time of the partly trained encoder (opt['bert_train_layers'] = N) beside the two schedules it sits between: the frozen
encoder (LOCK_BERT, its pass one step ahead) and the full unlock (opt['bert_train_gemm'] = '16').

Bench workload (B = 64, 30-word questions, 100 OCR items, 36 objects, bert-base, fp16c), 5 warm-up and 20 timed steps through
``SDNetTrainer.update`` with one batch of lookahead inside ``step_stream()``, loss read back one step late - what bench.py times.

    python tools/partial_unlock_bench.py [--rounds 3] [--modes lock,full,n1,n2,n4,n6,n2-inline] [--child-timeout 240]

(a mode ``n<N>-adamw``, not in the default list, steps the trained layers under opt['bert_optimizer'] = 'adamw'; the table's ratio
columns need ``full`` / ``lock`` among the modes and show ``-`` otherwise)

Every mode runs in a FRESH child process (a second CU-masked stream in one process lands on a used hardware queue slot), one after the
other, each under its own time limit; the chain stops at the first child that fails.  The rounds alternate through the modes inside one
invocation, and only ratios inside one invocation mean anything: boxes differ by 5 %.  Per mode: ms per step, samples / s, peak
allocated memory of the timed steps; then the ratios against the full unlock and LOCK_BERT of the same invocation.

    rocprofv3 --kernel-trace --stats -d OUT -- python tools/partial_unlock_bench.py --child n2

is one mode alone, e.g. under the profiler (a run of its own: the tool adds to every launch)."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = ["lock", "full", "n1", "n2", "n4", "n6", "n2-inline"]
BATCH, WARMUP, STEPS = 64, 5, 20


def child(mode, steps, warmup):
    import torch
    sys.path.insert(0, ROOT)
    import bench
    from ruart_amd import synth
    from ruart_amd.arguments import default_opt
    dev = torch.device("cuda:0")
    opt = default_opt(vocab_size=20000, cuda=True, device=dev, max_od_num=36, batch_size=BATCH)
    opt["ruart_defer_readback"] = True
    if mode != "lock":
        opt.pop("LOCK_BERT")
        opt["bert_train_gemm"] = "16"
    if mode.startswith("n"):
        opt["bert_train_layers"] = int(mode[1:].split("-")[0])
        if mode.endswith("-inline"):
            opt["bert_train_prefetch"] = False
        if mode.endswith("-adamw"):          # e.g. n2-adamw: the trained layers as an Adam group of their own (opt['bert_optimizer'])
            opt["bert_optimizer"] = "adamw"
    tr, _ = bench.build_trainer(opt, synth.bert_config(), dev)
    bs = [tr.ToCUDA(synth.synthetic_batch(opt, BATCH, seed=7 + i, n_q=30, n_ocr=100, n_od=36)) for i in range(4)]
    tokens = bs[0][0]["_ruart_index"].packed.T

    def step(i):
        return tr.update(bs[i % len(bs)], i, next_batch=bs[(i + 1) % len(bs)])

    with tr.step_stream():
        for i in range(warmup):
            step(i)
            torch.cuda.synchronize()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    t0 = time.perf_counter()
    with tr.step_stream():
        for i in range(steps):
            loss = step(warmup + i)
        tr.flush_readback()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    res = {"mode": mode, "ms_per_step": round(dt / steps * 1e3, 3), "samples_per_s": round(BATCH * steps / dt, 1),
           "peak_allocated_gb": round(torch.cuda.max_memory_allocated() / 2 ** 30, 3), "tokens": int(tokens), "last_loss": float(loss),
           "trained_encoder_tensors": sum(1 for n, p in tr.network.named_parameters() if n.startswith("Bert.") and p.requires_grad)}
    tr.close(final=True)
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", default=None, help="run ONE mode in this process and print its JSON line")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--modes", default=",".join(MODES))
    ap.add_argument("--steps", type=int, default=STEPS)
    ap.add_argument("--warmup", type=int, default=WARMUP)
    ap.add_argument("--child-timeout", type=int, default=240, help="seconds one child may take")
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.steps, a.warmup)
    modes = a.modes.split(",")
    results = {m: [] for m in modes}
    for r in range(a.rounds):
        for m in (modes if r % 2 == 0 else modes[::-1]):          # alternate the order: drift of the box does not favour a mode
            cmd = [sys.executable, os.path.abspath(__file__), "--child", m, "--steps", str(a.steps), "--warmup", str(a.warmup)]
            try:
                p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=a.child_timeout)
            except subprocess.TimeoutExpired:
                print("round %d mode %s: no result within %d s - stopping here" % (r, m, a.child_timeout), flush=True)
                return 1
            if p.returncode != 0:
                print("round %d mode %s: exit status %d - stopping here\n%s" % (r, m, p.returncode, p.stderr[-2000:]), flush=True)
                return 1
            res = json.loads(p.stdout.strip().splitlines()[-1])
            res["round"] = r
            results[m].append(res)
            print(json.dumps(res), flush=True)
    print("\nmode        ms/step per round              median  samples/s  peak GB   vs full  vs lock")
    med = {m: sorted(x["ms_per_step"] for x in results[m])[len(results[m]) // 2] for m in modes}
    for m in modes:
        ms = [x["ms_per_step"] for x in results[m]]
        row = "%-10s  %-30s %7.2f  %9.1f  %7.2f" % (m, " ".join("%.2f" % v for v in ms), med[m], BATCH * 1e3 / med[m],
                                                     max(x["peak_allocated_gb"] for x in results[m]))
        for base in ("full", "lock"):
            row += "  %7.3f" % (med[m] / med[base]) if base in med else "        -"
        print(row)
    return 0


if __name__ == "__main__":
    sys.exit(main())
