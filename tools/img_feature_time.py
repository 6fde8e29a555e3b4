#!/usr/bin/env python3
"""Training-step time of the two region-image-feature forms beside the shipped conf: ``overlay`` (``img_feature``, ``img_fea_way
replace_od``: the object items' states written over the projected features) and ``pure`` (``img_feature_replace_od`` too: no object
item is embedded or encoded), and the rows of the packed encoder stream of each.

Bench workload (B = 64, 30-word questions, 100 OCR items, 36 objects, 36 x 2048 features per image, bert-base, fp16c, LOCK_BERT), 5
warm-up and 20 timed steps through ``SDNetTrainer.update`` with one batch of lookahead inside ``step_stream()``, loss read back one step
late - what bench.py times.

    python tools/img_feature_time.py [--rounds 3] [--modes shipped,overlay,pure] [--child-timeout 240]

As in tools/es_post_time.py every measurement runs in a FRESH child process (a second CU-masked stream in one process lands on a used
hardware queue slot), one after the other, each under its own time limit; the chain stops at the first child that fails.  The rounds
alternate through the modes inside one invocation, and only ratios inside one invocation mean anything: boxes differ by 5 %.
Per mode: ms per step of every round, the median, samples / s, the ratio against the shipped conf and the packed token count."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = ["shipped", "overlay", "pure"]
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
    if mode != "shipped":
        opt.update(img_feature=True, img_fea_way="replace_od", img_fea_num=36, img_fea_dim=2048, img_spa_dim=8)
    if mode == "pure":
        opt["img_feature_replace_od"] = True
    tr, _ = bench.build_trainer(opt, synth.bert_config(), dev)
    bs = []
    for i in range(2):
        b = list(synth.synthetic_batch(opt, BATCH, seed=7 + i, n_q=30, n_ocr=100, n_od=36))
        if mode != "shipped":
            b[0]["img_features"], b[0]["img_spatials"] = synth.synthetic_image_features(opt, BATCH, seed=3 + i)
        bs.append(tr.ToCUDA(b))
    tokens = int(bs[0][0]["_ruart_index"].packed.T)

    def step(i):
        return tr.update(bs[i % len(bs)], i, next_batch=bs[(i + 1) % len(bs)])

    with tr.step_stream():
        for i in range(warmup):
            step(i)
            torch.cuda.synchronize()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    with tr.step_stream():
        for i in range(steps):
            loss = step(warmup + i)
        tr.flush_readback()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    res = {"mode": mode, "ms_per_step": round(dt / steps * 1e3, 3), "samples_per_s": round(BATCH * steps / dt, 1), "packed_tokens": tokens,
           "last_loss": float(loss)}
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
    print("\nmode      ms/step per round              median  samples/s  vs shipped  packed tokens")
    med = {m: sorted(x["ms_per_step"] for x in results[m])[len(results[m]) // 2] for m in modes}
    for m in modes:
        ms = [x["ms_per_step"] for x in results[m]]
        row = "%-8s  %-30s %7.2f  %9.1f" % (m, " ".join("%.2f" % v for v in ms), med[m], BATCH * 1e3 / med[m])
        row += "  %10.3f" % (med[m] / med["shipped"]) if "shipped" in med else "           -"
        print(row + "  %13d" % results[m][0]["packed_tokens"])
    return 0


if __name__ == "__main__":
    sys.exit(main())
