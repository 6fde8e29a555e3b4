#!/usr/bin/env python3
"""What opt['dp_global_batch'] costs: the B = 64 bench-shape training step (pipelined as bench.py runs it: the next batch's encoder
pass beside this step's trunk) under a world-size-1 RCCL group, with the switch off and on.  Both trainers live in one process and are
timed in alternating rounds of STEPS steps after WARMUP steps each, with a hipEvent pair on the trainer's step stream around each round.
The switch adds 27 exchanges per step (9 layer norms x (2 forward + 1 backward)), each a memset, a partials kernel and an RCCL
all-reduce of 256 / 512 floats on the branch's own group, where the plain op runs 3 + 2 kernels.

    python tools/dp_global_batch_cost.py [STEPS=20] [WARMUP=5] [ROUNDS=3]"""
import os
import socket
import sys

import numpy as np
import torch
import torch.distributed as dist

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench                                            # noqa: E402
from ruart_amd import dp, synth                         # noqa: E402
from ruart_amd.arguments import default_opt             # noqa: E402


def main():
    steps, warmup, rounds = (int(sys.argv[i]) if len(sys.argv) > i else d for i, d in ((1, 20), (2, 5), (3, 3)))
    dev = torch.device("cuda:0")
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    dp.init_process_group(dev, "nccl", rank=0, world_size=1)
    opt = default_opt(vocab_size=20000, cuda=True, device=dev, max_od_num=36, batch_size=64)
    cfg = synth.bert_config()
    trainers = {}
    for flag in (False, True):
        tr, _ = bench.build_trainer(dict(opt, dp_global_batch=flag), cfg, dev, process_group=dist.group.WORLD)
        assert tr.grad_sync is not None and tr.global_batch == flag
        trainers[flag] = tr
    batches = {flag: [tr.ToCUDA(synth.synthetic_batch(opt, 64, seed=7 + i, n_q=30, n_ocr=100, n_od=36)) for i in range(4)]
               for flag, tr in trainers.items()}
    torch.cuda.synchronize()
    times = {False: [], True: []}

    def run(flag, n):
        tr, bs = trainers[flag], batches[flag]
        with tr.step_stream():
            st = torch.cuda.current_stream()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            for i in range(n):
                tr.update(bs[i % 4], i, next_batch=bs[(i + 1) % 4])
            e1.record(st)
            tr.flush_readback()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / n

    for r in range(rounds):
        for flag in ((False, True) if r % 2 == 0 else (True, False)):
            run(flag, warmup)
            times[flag].append(run(flag, steps))
            print("round %d  dp_global_batch=%-5s  %.3f ms/step" % (r, flag, times[flag][-1]), flush=True)
    off, on = float(np.median(times[False])), float(np.median(times[True]))
    print("median over %d rounds of %d steps (B = 64, world-1 RCCL group): off %.3f ms, on %.3f ms, cost %+.3f ms (%+.1f %%)"
          % (rounds, steps, off, on, on - off, 100.0 * (on - off) / off), flush=True)
    for tr in trainers.values():
        tr.close(final=True)
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
