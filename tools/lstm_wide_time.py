#!/usr/bin/env python3
"""Time one bidirectional LSTM layer, forward + backward, on the streamed persistent kernels (ops.lstm_layer, 128 < hidden <= 256)
against the stepped route (layers.lstm_layer_stepped: one GEMM and one cell kernel per time step and direction).

    python tools/lstm_wide_time.py time [--runs 25] [--warmup 5] [--resources FILE] [--out profiles/lstm_wide.txt]     (needs the GPU)
    python tools/lstm_wide_time.py resources                                                                          (needs hipcc only)

``time``: both routes alternate in one process on the same seeded operands; after the warm-up every run is timed with device events,
and the report gives the median, the fastest and the slowest run and the 10th / 90th percentile of each route, the median per time
step (layer time / T) and the ratio of the medians.  ``resources`` prints the register, scratch and LDS use of the streamed kernels as
hipcc reports them; ``--resources FILE`` copies such a listing into the report.
"""
import argparse
import os
import re
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)

SHAPES = [(64, 100, 300, 256), (64, 40, 1088, 144)]          # (B, T, D_in, hidden), bidirectional


def resources():
    from ruart_amd import build
    src = os.path.join(build.CSRC, "sdnet_lstm.hip")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cmd = [hipcc] + build.FLAGS + ["-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", os.devnull]
    text = subprocess.run(cmd, stderr=subprocess.PIPE, stdout=subprocess.DEVNULL, check=True, text=True).stderr
    rows, name = [], None
    for line in text.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            continue
        m = re.search(r"\s(TotalSGPRs|VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\d+) \[", line)
        if m and name and "lstm_wide" in name:
            rows.append((name, m.group(1), int(m.group(2))))
    out = []
    for n in dict.fromkeys(r[0] for r in rows):
        vals = {k: v for nn, k, v in rows if nn == n}
        kernel = re.sub(r"^_Z\d+", "", n).split("kernel")[0] + "kernel"
        out.append("%-28s VGPRs %3d  AGPRs %3d  SGPRs %3d  scratch %d B/lane  LDS %6d B  waves/SIMD %d"
                   % (kernel, vals["VGPRs"], vals["AGPRs"], vals["TotalSGPRs"], vals["ScratchSize [bytes/lane]"],
                      vals["LDS Size [bytes/block]"], vals["Occupancy [waves/SIMD]"]))
    return "\n".join(out)


def time_routes(runs, warmup):
    import numpy as np
    import torch
    import ruart_amd.layers as L
    from ruart_amd import ops
    dev = "cuda:0"
    lines = []
    for B, T, Din, h in SHAPES:
        g = torch.Generator().manual_seed(h + T)
        k = 1.0 / np.sqrt(h)
        sizes = [(4 * h, Din), (4 * h, h), (4 * h,), (4 * h,)] * 2
        P = [((torch.rand(s, generator=g) * 2 - 1) * k).to(dev).requires_grad_() for s in sizes]
        x = torch.randn(B, T, Din, generator=g).to(dev).requires_grad_()
        gy = torch.randn(B, T, 2 * h, generator=g).to(dev)
        routes = {"streamed (ops.lstm_layer)": lambda: ops.lstm_layer(x, *P),
                  "stepped (layers.lstm_layer_stepped)": lambda: L.lstm_layer_stepped(x, *P)}
        outs, times = {}, {n: [] for n in routes}
        for it in range(warmup + runs):
            for name, fn in routes.items():
                for t in [x] + P:
                    t.grad = None
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                y = fn()
                y.backward(gy)
                e1.record()
                e1.synchronize()
                if it >= warmup:
                    times[name].append(e0.elapsed_time(e1) * 1e3)
                outs[name] = y.detach()
        ops.nan_flag.check_and_clear()
        diff = float((outs["streamed (ops.lstm_layer)"] - outs["stepped (layers.lstm_layer_stepped)"]).abs().max())
        lines.append("(B, T, D_in, hidden) = (%d, %d, %d, %d), bidirectional, forward + backward, %d timed runs after %d warm-up, us"
                     % (B, T, Din, h, runs, warmup))
        med = {}
        for name, ts in times.items():
            ts = np.array(ts)
            med[name] = float(np.median(ts))
            lines.append("  %-34s median %9.1f   min %9.1f   p10 %9.1f   p90 %9.1f   max %9.1f   per step (median / T) %7.2f"
                         % (name, med[name], ts.min(), np.percentile(ts, 10), np.percentile(ts, 90), ts.max(), med[name] / T))
        a, b = med["streamed (ops.lstm_layer)"], med["stepped (layers.lstm_layer_stepped)"]
        lines.append("  stepped / streamed = %.2f   (max |y_streamed - y_stepped| = %.2e)" % (b / a, diff))
        # the recurrence alone: forward kernel time per step, the figure the streamed design was estimated by
        xp = ops.linear(x.detach(), torch.cat([P[0], P[4]], 0), torch.cat([P[2] + P[3], P[6] + P[7]], 0)).contiguous()
        whh = torch.stack([P[1].detach(), P[5].detach()], 0).contiguous()
        ts = []
        for it in range(warmup + runs):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            ops._LstmRecurrence.apply(xp, whh, 2)
            e1.record()
            e1.synchronize()
            if it >= warmup:
                ts.append(e0.elapsed_time(e1) * 1e3)
        ts = np.array(ts)
        lines.append("  forward recurrence alone (preparation + persistent kernel, both directions side by side): median %.1f, min %.1f, "
                     "max %.1f -> %.2f us per step" % (np.median(ts), ts.min(), ts.max(), np.median(ts) / T))
        lines.append("")
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["time", "resources"])
    ap.add_argument("--runs", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--resources", default=None, help="time: a listing written by the resources mode, copied into the report")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.mode == "resources":
        text = resources()
    else:
        if a.runs < 20:
            ap.error("--runs: at least 20")
        text = time_routes(a.runs, a.warmup)
        if a.resources:
            text += "\nkernel resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950)\n" + open(a.resources).read().rstrip() + "\n"
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
