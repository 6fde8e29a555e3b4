#!/usr/bin/env python3
"""Times of the answer scorer with the yes/no heads at the conf shape (B = 64, L = 100, D = 500; h0 250 wide), device events, each the
median of ``--calls`` single calls after ``--warmup`` ones, the three groups interleaved round by round:

  * ruart_scorer_heads_fwd / _bwd at H = 4, n_front = 3 (no_read, yes, no in front; noanswer behind)
  * ruart_scorer_fwd / _bwd (one head) on the same x
  * GetFinalScores(yesno=True), op by op (``fused_scorer`` of the trunk mode off), forward + backward, and the same module on the fused form

    python tools/yesno_scorer_time.py [--calls 50] [--warmup 10] > profiles/yesno_scorer.txt
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ruart_amd import hip, ops          # noqa: E402
import ruart_amd.layers as L            # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    a = ap.parse_args()
    assert a.calls >= 20
    d = torch.device("cuda:0")
    B, Ls, D, Hh, ES, H, NF = 64, 100, 500, 250, 36, 4, 3
    g = torch.Generator().manual_seed(3)
    lib = hip.kernels()
    ops.nan_flag.ensure(d)
    x = torch.randn(B, Ls, D, generator=g).to(d)
    u1, u2 = (torch.randn(B, D, generator=g).to(d) / D ** 0.5 for _ in range(2))
    uh = (torch.randn(B, H, D, generator=g) / D ** 0.5).to(d)
    w, bh = (torch.randn(H, D, generator=g) / D ** 0.5).to(d), torch.randn(H, generator=g).to(d)
    mask = torch.ones(B, Ls, dtype=torch.uint8)
    for b in range(B):
        mask[b, 40 + (b * 7) % 61:] = 0
    mask = mask.to(d)
    probs4, a4, gp4 = torch.empty(B, H + Ls, device=d), torch.empty(B, H, Ls, device=d), torch.randn(B, H + Ls, generator=g).to(d)
    probs1, a1, gp1 = torch.empty(B, 1 + Ls, device=d), torch.empty(B, Ls, device=d), torch.randn(B, 1 + Ls, generator=g).to(d)
    gx, gu1, gu2 = torch.empty_like(x), torch.empty_like(u1), torch.empty_like(u2)
    guh4, gwp4, gbp4 = torch.empty_like(uh), torch.empty(B, H, D, device=d), torch.empty(B, H, device=d)
    guh1, gwp1, gbp1 = torch.empty(B, D, device=d), torch.empty(B, D, device=d), torch.empty(B, device=d)
    uh1, w1, b1 = uh[:, 3].contiguous(), w[3].contiguous(), bh[3:4].contiguous()
    st = hip.stream_ptr()

    ga = L.GetFinalScores(D, Hh, yesno=True, no_answer=True, useES=True)
    with torch.no_grad():
        for prm in ga.parameters():
            prm.copy_(torch.randn(prm.shape, generator=g) / max(prm.shape[-1], 1) ** 0.5)
    ga = ga.to(d).train()
    L.set_dropout_prob(0.0)
    xm, h0 = x.clone().requires_grad_(), torch.randn(B, Hh, generator=g).to(d).requires_grad_()

    def module(fused):
        def run():
            ga.zero_grad(set_to_none=True)
            xm.grad = h0.grad = None
            with ops.use_trunk_mode(gemm="x3", fused_scorer=fused):
                probs = ga(xm, h0, mask, ES, mask_flag=True)
            (probs * gp4).sum().backward()
        return run

    work = {
        "heads_fwd  H=4 n_front=3": lambda: lib.ruart_scorer_heads_fwd(x, u1, u2, uh, w, bh, mask, probs4, a4, B, Ls, D, ES, H, NF, 1, st),
        "heads_bwd  H=4 n_front=3": lambda: lib.ruart_scorer_heads_bwd(x, u1, u2, uh, w, probs4, a4, gp4, gx, gu1, gu2, guh4, gwp4, gbp4, B, Ls,
                                                                       D, ES, H, NF, st),
        "scorer_fwd (one head)": lambda: lib.ruart_scorer_fwd(x, u1, u2, uh1, w1, b1, mask, probs1, a1, B, Ls, D, ES, 1, st),
        "scorer_bwd (one head)": lambda: lib.ruart_scorer_bwd(x, u1, u2, uh1, w1, probs1, a1, gp1, gx, gu1, gu2, guh1, gwp1, gbp1, B, Ls, D, ES, st),
        "GetFinalScores(yesno) op-by-op fwd+bwd": module(False),
        "GetFinalScores(yesno) fused    fwd+bwd": module(True),
    }
    times = {k: [] for k in work}
    for r in range(a.warmup + a.calls):
        for k, fn in work.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if r >= a.warmup:
                times[k].append(e0.elapsed_time(e1) * 1e3)
    ops.nan_flag.check_and_clear()
    print("answer scorer, B = %d, L = %d, D = %d, ES = %d; %s; device events, median [min .. max] of %d calls after %d, microseconds"
          % (B, Ls, D, ES, torch.cuda.get_device_name(0), a.calls, a.warmup))
    for k, v in times.items():
        print("%-42s %9.1f  [%8.1f .. %8.1f]" % (k, statistics.median(v), min(v), max(v)))
    m = {k: statistics.median(v) for k, v in times.items()}
    print("four heads / one head: forward %.2fx, backward %.2fx" % (m["heads_fwd  H=4 n_front=3"] / m["scorer_fwd (one head)"],
                                                                     m["heads_bwd  H=4 n_front=3"] / m["scorer_bwd (one head)"]))


if __name__ == "__main__":
    main()
