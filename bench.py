#!/usr/bin/env python3
"""Headline benchmark of the RUArt hot path on MI355X (contract: one JSON line on rank 0).

    python bench.py --gpus 1 --steps 10 --warmup 3
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P bench.py --gpus N ...

Metric (BASELINE.json): VQA samples/sec, forward + backward training step, B=64 per GPU, question 30 words, 100 OCR
items, 36 objects, bert-base (12 x 768, 12 heads, FFN 3072), Adamax - every rank runs the full reference step
(frozen BERT forward, SDNet forward, BCE loss, backward, global-norm clip, optimizer step, embedding re-pin), gradients
averaged over ranks with RCCL.  A "step" is one such pass over one synthetic batch whose tensors and index vectors are
already resident in HBM when the timed region starts.  Weak scaling: B per GPU is fixed.

A plain run sets up, warms up, times the --steps steps, writes the last timed step's outputs if --dump-outputs is given, and prints the
line; "step_ms" (the spread of the timed steps) and "peak_hbm_gb" come from the timed region itself.  Every other figure takes work of
its own and is measured only with --full:
  python bench.py --gpus 1 --steps 10 --warmup 3 --full
  python bench.py --gpus 1 --steps 10 --warmup 3 --dump-outputs DIR

--dump-outputs DIR: what the timed path computed in its LAST timed step (rank 0), as DIR/<name>.npy (float32; float64 for the loss),
written right after the timed region (before anything --full adds): training - "loss", the answer "scores" of the step's forward and every
trainable parameter after the step's update ("param.<name>"); --mode fwd - "scores"; --mode bert512 - the encoder's layer outputs of
every part ("encoder_layers.part<i>", real token rows only).  Inputs are seeded, so two builds run with the same arguments can be
compared output for output.  An array of more than 2^20 values is written as a fixed, seeded sample of its flattened values (the same
positions in every run), so that the files stay under 64 MB in all.

Extra objects on the same line (--full only):
  roofline     - the dominant kernel (the encoder's 768x768 / 768x3072 projections: gemm_16c_nt_256p8 in the default precision,
                 gemm_16_nt_256p8 in the plain 16-bit modes): ALGORITHMIC FLOPs (2 * real_tokens * N * K per launch, counted once -
                 the fp8 correction product of the default mode is overhead, not credit) / its HIP-event time measured live on
                 the launch stream, against the 2.5 PFLOP/s dense 16-bit MFMA peak.  ``frac`` is the figure of the TIMED schedule
                 (encoder of batch t+1 beside the trunk of batch t); ``alone`` is the same kernel with the device to itself.
  parity       - max |p - p_ref| of this run's answer probabilities against the reference's own fp32 CPU output for batch 0 of
                 this workload (tests/golden/sdnet_e2e_full.npz, written by oracle/gen_golden.py from the unmodified reference).
  bert512      - the north-star shape: BERT-base + attention forward over (64, 512) valid tokens in plain f16, ms and fraction
                 of the 2.5 PFLOP/s peak.
  cpu_baseline - the CPU oracle (oracle/ruart_oracle.py, kind "port": the reference cannot travel) timed on this box's
                 host cores on a bounded sample of the same workload (rank 0, N=1 only): one warm-up, median of three runs.
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

PEAK_TFLOPS = 2500.0        # MI355X dense bf16/f16 MFMA (MI355X_MICROARCH.md); sparsity figures are never used
SUSTAINED_F16_TFLOPS, SUSTAINED_FP8_TFLOPS = 2165.0, 4763.0      # pure MFMA streams at the power cap (tools/r06_mfma_power.hip; a note on the line, not a peak)
DTYPE = {"fp16": "f16", "bf16": "bf16", "fp32": "f32", "x3": "f32 storage, split-bf16 MFMA",
         "fp16c": "f16 MFMA + block-scaled fp8 (e4m3) MFMA correction, f32 accumulate / residual stream"}
GEMM_KERNEL = {"fp16": "gemm_16_nt_256p8", "bf16": "gemm_16_nt_256p8", "fp16c": "gemm_16c_nt_256p8"}
TRAFFIC_FILE = "r05_gemm_traffic.json"


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--precision", default="fp16c", choices=["fp16c", "fp16", "bf16", "fp32", "x3"],
                    help="encoder precision.  The default is the fastest mode that holds the north-star bound (every answer probability "
                         "within 1e-3 of the reference's fp32 CPU output at B = 64, tests/test_gpu_parity_full.py): fp16c = f16 MFMA "
                         "products + block-scaled fp8 MFMA correction of both operands' rounding residuals, fp32 residual stream.  "
                         "fp16 / bf16 are faster and miss the bound (2.2e-3 / 1.5e-2 on this workload)")
    ap.add_argument("--no-parity", action="store_true", help="skip the live comparison with the reference's golden scores")
    ap.add_argument("--no-bert512", action="store_true", help="skip the north-star (64, 512) encoder-forward measurement")
    ap.add_argument("--mode", default="train", choices=["train", "fwd", "bert512"])
    ap.add_argument("--seq-len", type=int, default=512)
    ap.add_argument("--parts", type=int, default=2, help="bert512: run the batch as this many independent parts on their own streams")
    ap.add_argument("--n-batches", type=int, default=2, help="distinct pre-staged synthetic batches cycled through")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--cpu-samples", type=int, default=4)
    ap.add_argument("--no-roofline", action="store_true")
    ap.add_argument("--no-prefetch", action="store_true", help="run the encoder inline instead of one step ahead")
    ap.add_argument("--include-h2d", action="store_true",
                    help="secondary: every timed step starts from the collated HOST batch (ids, masks, positions and the host-built "
                         "batch index, as a DataLoader worker with VQA_collate(prepare_index=True) hands it over) and ships it itself")
    ap.add_argument("--stress", action="store_true",
                    help="secondary: BASELINE's stress shapes - 300 OCR items, 100 objects, bert-large 24 x 1024 (use with --precision bf16)")
    ap.add_argument("--force-dp", action="store_true",
                    help="rehearsal on one GPU: a world-size-1 RCCL process group, so the gradient hooks, the bucketed all-reduce and "
                         "the barriers of the N > 1 path all run")
    ap.add_argument("--frozen-dropout", action="store_true",
                    help="opt['bert_frozen_dropout']: the frozen encoder's training passes with BERT's own dropout on, as the reference's "
                         "update() really runs them (Models/SDNetTrainer.py:332); nothing runs ahead in this mode")
    ap.add_argument("--train-gemm", default="16", choices=["x3", "16", "16gemm"], help="with --unlock-bert: GEMM form of the trainable encoder")
    ap.add_argument("--unlock-bert", action="store_true",
                    help="secondary: conf without LOCK_BERT - the encoder is trained too (fp32 storage, split-bf16 MFMA products)")
    ap.add_argument("--graph-trunk", type=int, default=None, help="1/0: replay the fixed-shape trunk as captured hipGraphs")
    ap.add_argument("--no-timeline", action="store_true", help="skip the timeline pass (device times of the step's two chains)")
    ap.add_argument("--launch-check", action="store_true",
                    help="plumbing check of the --gpus N self-launch: rendezvous (gloo on the CPU when there is no GPU), count the ranks "
                         "with an all-reduce, print {launch_check, ranks_seen} on rank 0 and exit - no product code runs")
    ap.add_argument("--full", action="store_true",
                    help="also measure everything beyond the headline figure: parity against the reference's golden scores, the "
                         "roofline and timeline passes, the (64, 512) encoder forward, the CPU baseline (train / fwd); the one-pass "
                         "schedule and the GEMM share (--mode bert512).  The --no-* options still skip their part")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step computed as DIR/<name>.npy (see the module docstring)")
    return ap.parse_args()


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a))


_T0 = time.perf_counter()


def note(msg):
    """progress on stderr (the JSON line on stdout stays alone)"""
    if int(os.environ.get("RANK", "0")) == 0:
        print("[bench %7.1fs] %s" % (time.perf_counter() - _T0, msg), file=sys.stderr, flush=True)


DUMP_SAMPLE = 1 << 20           # --dump-outputs: values per array before it is sampled
DUMP_BUDGET = 64 << 20          # --dump-outputs: bytes in all


def dump_outputs(out_dir, arrays):
    """--dump-outputs: write each (name, tensor or float) of ``arrays`` as out_dir/<name>.npy - tensors as float32, Python floats as
    float64.  A tensor of more than DUMP_SAMPLE values is written as the values at a seeded sample of DUMP_SAMPLE flat positions (sorted;
    the same positions for the same shape in every run); the sample shrinks further if the files would exceed DUMP_BUDGET."""
    os.makedirs(out_dir, exist_ok=True)
    cap = DUMP_SAMPLE
    while sum(min(v.numel(), cap) * 4 for _, v in arrays if torch.is_tensor(v)) > DUMP_BUDGET:
        cap //= 2
    total = 0
    for name, v in arrays:
        if torch.is_tensor(v):
            flat = v.detach().reshape(-1)
            if flat.numel() > cap:
                idx = np.sort(np.random.default_rng(1033).choice(flat.numel(), size=cap, replace=False))
                flat = flat[torch.from_numpy(idx).to(flat.device)]
                arr = flat.float().cpu().numpy()
            else:
                arr = v.detach().float().cpu().numpy()
        else:
            arr = np.array([float(v)], dtype=np.float64)
        np.save(os.path.join(out_dir, name + ".npy"), arr)
        total += arr.nbytes
    note("outputs of the last timed step: %d arrays, %.1f MB in %s" % (len(arrays), total / 2 ** 20, out_dir))


def build_trainer(opt, cfg, device, seed=1033, process_group=None):
    from ruart_amd import synth
    from ruart_amd.trainer import SDNetTrainer
    opt = dict(opt)
    opt["bert_state"] = synth.make_bert_weights(cfg, seed=seed, w_std=0.02)
    opt["bert_config"] = cfg
    sw = synth.make_sdnet_weights(opt, seed=seed)
    tr = SDNetTrainer(opt, device=device, process_group=process_group)
    tr.setup_model({"glove_embedding": T(sw["glove_embed.weight"]), "fast_embedding": T(sw["fast_embed.weight"])})
    missing, unexpected = tr.network.load_state_dict({k: T(v) for k, v in sw.items()}, strict=False)
    assert not unexpected and all(k.startswith("Bert.bert_model.") for k in missing), (missing, unexpected)
    del opt["bert_state"]
    return tr, sw


def cpu_baseline(opt, cfg, n_samples, seed=1033, runs=3):
    """Time the CPU oracle's forward + loss + backward on `n_samples` samples of the bench workload: one warm-up run on one
    sample, then the median of `runs` runs (the stress shapes - bert-large, 300 OCR items - take one run of one
    sample: ~20 s of 16 cores)."""
    from oracle import ruart_oracle as O          # CPU baseline leg: allowed importer
    from ruart_amd import synth
    try:
        cores = len(os.sched_getaffinity(0))
    except AttributeError:
        cores = os.cpu_count() or 1
    cores = max(1, min(cores, 16))          # the GPU box gives one-GPU jobs a 16-core share; oversubscribing stalls torch
    torch.set_num_threads(cores)
    bw = {k: T(v) for k, v in synth.make_bert_weights(cfg, seed=seed, w_std=0.02).items()}
    sw = synth.make_sdnet_weights(opt, seed=seed)

    def run(n, bseed):
        P = {k: T(v).requires_grad_(v.shape != (1, 1, 1)) for k, v in sw.items()}
        q, ocr, od, gt, _ = synth.synthetic_batch(opt, n, seed=bseed, n_q=30, n_ocr=opt["max_ocr_num"], n_od=opt["max_od_num"])
        t0 = time.perf_counter()
        scores = O.sdnet_forward(P, opt, bw, cfg, q, ocr, od)
        O.instance_bce_with_logits(scores, gt).backward()
        return time.perf_counter() - t0

    run(1, 98)
    times = sorted(run(n_samples, 99 + i) for i in range(runs))
    dt = times[len(times) // 2]
    out = {"value": round(n_samples / dt, 4), "unit": "samples/s", "cores": int(torch.get_num_threads()), "kind": "port",
           "sample": "%d sample(s) of the bench workload (q=30, ocr=%d, obj=%d, %s), fwd+loss+bwd: 1 warm-up run, median of %d (%s s)"
                     % (n_samples, opt["max_ocr_num"], opt["max_od_num"], "bert-large" if cfg["hidden_size"] == 1024 else "bert-base", runs,
                        " / ".join("%.1f" % t for t in times))}
    if cfg["hidden_size"] == 768 and opt["max_ocr_num"] == 100:      # the reference was timed on the headline workload only
        out["reference_itself"] = {"value": 0.312, "unit": "samples/s", "threads": 8, "samples": 4,
                                   "measured": "once, in the build container, round 1 - a constant of this file, NOT timed in this run",
                                   "where": "build container - the reference cannot travel to the GPU box; the oracle ran 0.374 samples/s "
                                            "beside it, outputs equal to 1.7e-6", "source": "oracle/time_reference.py"}
    return out


def live_parity(tr, opt, batch, golden):
    """max |p - p_ref| of the product's answer probabilities for the bench's batch 0 against the reference's own output."""
    import ruart_amd.layers as L
    z = np.load(golden)
    if int(z["B"]) != batch[3].shape[0] or batch[1]["num_cnt"] != z["ocr_num_cnt"].tolist():
        return None
    L.set_dropout_prob(0.0)
    tr.network.train()
    tr.network.drop_emb = False
    def fwd():
        with torch.no_grad():
            return tr.network(batch[0], batch[1], batch[2])[0]
    # (on the trainer's step stream, as every forward of the timed region)
    scores = tr.on_step_stream(fwd)
    tr.network.check_nan()
    d = np.abs(scores.float().cpu().numpy() - z["scores"])
    L.set_dropout_prob(0.0 if "DROPOUT" not in opt else float(opt["DROPOUT"]))
    return {"max_abs_err_vs_reference": float("%.3g" % d.max()), "mean_abs_err": float("%.3g" % d.mean()), "outputs": int(d.size),
            "bound": 1e-3, "holds": bool(d.max() < 1e-3),
            "reference": "unmodified reference, fp32 CPU, same seeded batch and weights (tests/golden/sdnet_e2e_full.npz)"}


def bert512_measure(a, device, lib, precision, batch=64, steps=None, warmup=None, full=True, dump=None):
    """North-star shape: BERT-base + fused attention FORWARD on input_ids (B, L) all valid (default (64, 512)).
    Achieved TFLOP/s on the algorithmic 169 869 312 + 36 864 L flop per token against the 2.5 PF MFMA peak.
    The batch runs as ``--parts`` independent groups of sequences on their own streams: at 32 768 rows the two N = 768 products
    have 384 tiles = 1.5 rounds of the 256 CUs, and a second stream's kernels fill the half-empty rounds (tools/bert512_split.py).
    ``full``: the one-pass schedule is timed too and reported beside it, and its GEMMs are timed in a pass of their own (dt1 / gemm_*
    are None without it).  ``dump``: a directory for the layer outputs of the timed schedule's last step (dump_outputs)."""
    from ruart_amd import hip, synth
    from ruart_amd.bert import BertEncoderWeights, PackedTokens, bert_encode, layer_outputs, _Buffers
    steps = steps or a.steps
    warmup = a.warmup if warmup is None else warmup
    cfg = synth.bert_config()
    # round 6: the plain 16-bit pass with its LayerNorms folded into the projections (ruart_gemm_16_nt_fold; RUART_LN_FOLD=0: the seven-launch layer)
    W = BertEncoderWeights(synth.make_bert_weights(cfg, seed=1033, w_std=0.02), cfg, device, precision,
                           ln_fold=os.environ.get("RUART_LN_FOLD", "1") != "0")
    W.c_model.tail_cus = int(os.environ.get("RUART_TAIL_CUS", 0))       # experiments: tail split of the GEMMs (off: DESIGN.md section 5, round 4)
    if os.environ.get("RUART_TILE_ORDER"):              # experiments: GROUP_M of the encoder GEMM's tile walk
        hip.check(lib.ruart_gemm_set_tile_order(int(os.environ["RUART_TILE_ORDER"])), "set_tile_order")
    L = a.seq_len
    ids = torch.randint(1000, cfg["vocab_size"], (batch, L), generator=torch.Generator().manual_seed(1033))
    flops = batch * L * (169869312 + 36864 * L)

    def schedule(P):
        per = (batch + P - 1) // P
        parts = [PackedTokens([(ids[i:i + per], torch.ones_like(ids[i:i + per], dtype=torch.bool))], device,
                              mfma_long=precision in ("fp16", "bf16")) for i in range(0, batch, per)]
        bufs = [_Buffers() for _ in parts]
        streams = [torch.cuda.Stream(device=device) for _ in parts] if P > 1 else [torch.cuda.current_stream()]
        outs = [None] * len(parts)

        def step():
            for j, (p, b, s) in enumerate(zip(parts, bufs, streams)):
                with torch.cuda.stream(s):
                    outs[j] = bert_encode(W, p, b)
        step.outputs = lambda: [("encoder_layers.part%d" % j, layer_outputs(o)[:, :p.T]) for j, (p, o) in enumerate(zip(parts, outs))]
        return step

    def timed(step):
        for _ in range(warmup):
            step()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            step()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / steps

    one = schedule(1) if full or a.parts <= 1 else None
    dt1 = timed(one) if one is not None else None
    headline = schedule(a.parts) if a.parts > 1 else one
    dt = timed(headline) if a.parts > 1 else dt1
    if dump:
        dump_outputs(dump, headline.outputs())
    r = {"flops": flops, "dt": dt, "dt1": dt1 if full else None, "gemm_ms": None, "gemm_n": 0, "gemm_flops": None, "steps": steps, "L": L}
    if full:
        hip.check(lib.ruart_prof_enable(1), "prof_enable")
        for _ in range(steps):
            one()
        torch.cuda.synchronize()
        ms, n, fl = ctypes.c_double(), ctypes.c_longlong(), ctypes.c_double()
        hip.check(lib.ruart_prof_read(ctypes.byref(ms), ctypes.byref(n), ctypes.byref(fl)), "prof_read")
        lib.ruart_prof_enable(0)
        r.update(gemm_ms=ms.value, gemm_n=n.value, gemm_flops=fl.value)
    return r


def bert512(a, device, lib, out_stream=sys.stdout):
    note("bert512: building weights")
    r = bert512_measure(a, device, lib, a.precision, batch=a.batch, full=a.full, dump=a.dump_outputs)
    flops, dt, dt1, L = r["flops"], r["dt"], r["dt1"], r["L"]
    one_pass = None
    if dt1 is not None:
        one_pass = {"ms_per_step": round(dt1 * 1e3, 3), "achieved": round(flops / dt1 / 1e12, 1),
                    "frac": round(flops / dt1 / 1e12 / PEAK_TFLOPS, 4),
                    "gemm_only_tflops": round(r["gemm_flops"] / (r["gemm_ms"] * 1e-3) / 1e12, 1) if r["gemm_n"] else None,
                    "gemm_share": round(r["gemm_ms"] / r["steps"] / (dt1 * 1e3), 3) if r["gemm_n"] else None}
    out = {"metric": "BERT-base + attention forward, (B=%d, L=%d), achieved TFLOP/s" % (a.batch, L), "value": round(flops / dt / 1e12, 1),
           "unit": "TFLOP/s", "n_gpus": 1, "steps": a.steps, "warmup": a.warmup, "ms_per_step": round(dt * 1e3, 3),
           "higher_is_better": True, "dtype": DTYPE[a.precision], "data": "synthetic",
           "config": {"workload": "north-star shape: bert-base forward over %d x %d valid tokens" % (a.batch, L),
                      "schedule": "%d independent group(s) of sequences, one stream each" % a.parts},
           "roofline": {"bound": "mfma", "achieved": round(flops / dt / 1e12, 1), "peak": PEAK_TFLOPS, "unit": "TFLOP/s",
                        "frac": round(flops / dt / 1e12 / PEAK_TFLOPS, 4), "traffic": None, "one_pass": one_pass}}
    print(json.dumps(out), file=out_stream, flush=True)


def _claim_stdout():
    """The contract is ONE JSON line on stdout.  Libraries print there too (RCCL writes a version banner at its first collective):
    keep the real stdout for the line and send everything else that is written to fd 1 to stderr."""
    sys.stdout.flush()
    real = os.fdopen(os.dup(1), "w")
    os.dup2(2, 1)
    return real


def self_launch(a):
    """``python bench.py --gpus N`` without a launcher: start N ranks of this file under torch.distributed.run (one process per GPU,
    rendezvous on 127.0.0.1) as CHILD processes and hand their exit code back.  Runs before anything touches the GPU; the children
    inherit stdout, so rank 0's JSON line is this process's line."""
    import socket
    import subprocess
    port = os.environ.get("MASTER_PORT")
    if not port:
        with socket.socket() as sk:
            sk.bind(("127.0.0.1", 0))
            port = str(sk.getsockname()[1])
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env.pop("MASTER_PORT", None)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(a.gpus), "--master-addr", "127.0.0.1",
           "--master-port", port, os.path.abspath(__file__)] + sys.argv[1:]
    note("--gpus %d without a launcher: starting %s" % (a.gpus, " ".join(cmd[1:8])))
    sys.stdout.flush()
    return subprocess.call(cmd, env=env)


def launch_check(a, out_stream, world, rank):
    """--launch-check: what the self-launch has to get right, without the product - every rank arrives, sees the others, and rank 0
    alone writes the line."""
    import torch.distributed as dist
    n = 1
    if world > 1:
        gpu = torch.cuda.is_available() and torch.cuda.device_count() >= world
        if gpu:
            torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", "0")))
        dist.init_process_group("nccl" if gpu else "gloo")
        t = torch.ones(1, device="cuda" if gpu else "cpu")
        dist.all_reduce(t)
        n = int(t.item())
        dist.barrier()
        dist.destroy_process_group()
    if rank == 0:
        print(json.dumps({"launch_check": True, "ranks_seen": n, "n_gpus": a.gpus}), file=out_stream, flush=True)
    return 0 if n == a.gpus else 1


def _dist(ms):
    """{min, median, p90, max, first} of a list of per-step times (ms)."""
    v = sorted(ms)
    return {"min": round(v[0], 3), "median": round(v[len(v) // 2], 3), "p90": round(v[min(len(v) - 1, int(0.9 * len(v)))], 3),
            "max": round(v[-1], 3), "first": round(ms[0], 3)}


def _steps_of(b, f):
    marks = [(float(t), int(-fl)) for t, fl in zip(b, f) if fl < 0]
    starts = [t for t, tag in marks if tag == 1]
    return marks, starts


def _timeline(b, e, f):
    """Medians over the steps of one marks-only pass of the timed schedule (records of ruart_prof_timeline: markers with flops = -tag),
    every time in ms from the step's own start (mark 1: the step stream reaches the forward, i.e. the previous encoder pass has
    ended).  The encoder pass launched inside step t serves batch t+1: its end ends step t's device work."""
    marks, starts = _steps_of(b, f)
    ends6 = sorted(t for t, tag in marks if tag == 6)
    rows = []
    for k in range(1, len(starts) - 1):                  # (the first step of the pass refills the pipeline after a sync)
        s0, s1 = starts[k], starts[k + 1]
        m = {tag: t - s0 for t, tag in marks if s0 <= t < s1 and tag != 6}
        if not all(t in m for t in (2, 3, 4, 5)):
            continue
        # the pass launched in this step starts (mark 5, on the in-order encoder stream) when the pass before it has ended, and may
        # end inside the NEXT step's window (round 5: the next step's trunk no longer waits for it)
        after = [t for t in ends6 if t > s0 + m[5]]
        if not after:
            continue
        rows.append((s1 - s0, m[2], m[3], m[4], m[5], after[0] - s0))
    if not rows:
        return {}
    med = [float(np.median([r[i] for r in rows])) for i in range(6)]
    return {"steps": len(rows), "step": round(med[0], 3), "step_max": round(max(r[0] for r in rows), 3),
            "trunk_forward_end": round(med[1], 3), "trunk_backward_end": round(med[2], 3), "optimizer_end": round(med[3], 3),
            "encoder_pass_start": round(med[4], 3), "encoder_pass_end": round(med[5], 3),
            "what": "medians over the steps of a separate pass of the timed schedule with six hipEvents per step (step stream: forward "
                    "start / forward end / backward end / optimizer end; encoder stream: before / after the pass launched in the step, "
                    "which encodes batch t+1); ms from the step's forward start.  The encoder stream runs its passes back to back: "
                    "encoder_pass_start is where the previous pass ended, and a pass may end after the next step has started "
                    "(encoder_pass_end > step)"}


def _gemm_split(b, e, f):
    """From the GEMM-bracketed pass: mean launch-to-finish time of the encoder GEMMs that start while the trunk is on the device and of
    those that start after its optimizer step, medians over the steps."""
    marks, starts = _steps_of(b, f)
    rows = []
    for k in range(1, len(starts) - 1):
        s0, s1 = starts[k], starts[k + 1]
        m = {tag: t for t, tag in marks if s0 <= t < s1}
        g = [(bb, ee) for bb, ee, fl in zip(b, e, f) if fl > 0 and s0 <= bb < s1]
        if not g or 4 not in m:
            continue
        beside = [ee - bb for bb, ee in g if bb < m[4]]
        after = [ee - bb for bb, ee in g if bb >= m[4]]
        rows.append((1e3 * float(np.mean(beside)) if beside else float("nan"), 1e3 * float(np.mean(after)) if after else float("nan"), len(after), s1 - s0))
    if not rows:
        return {}
    def med(col):                                   # (a column may be all-NaN: no GEMM launch after the trunk in any step)
        v = [r[col] for r in rows if r[col] == r[col]]
        return round(float(np.median(v)), 1) if v else None
    return {"beside_trunk": med(0), "after_trunk": med(1),
            "launches_after_trunk": int(np.median([r[2] for r in rows])), "step_ms_of_this_pass": round(float(np.median([r[3] for r in rows])), 3),
            "note": "the ~100 events per step of this pass stretch the step; timeline_ms is the unperturbed schedule"}


def main():
    a = parse()
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if a.gpus > 1 and "WORLD_SIZE" not in os.environ:
        raise SystemExit(self_launch(a))           # (no GPU call has been made yet: children are fresh processes)
    out_stream = _claim_stdout()
    if world != a.gpus and world > 1:
        raise SystemExit("--gpus %d but WORLD_SIZE=%d" % (a.gpus, world))
    if a.launch_check:
        raise SystemExit(launch_check(a, out_stream, world, rank))
    assert torch.cuda.is_available(), "bench.py needs an MI355X; there is no CPU fallback of the product path"
    # RUART_BENCH_REHEARSE_ONE_GPU=1: every rank on device 0, gradients over gloo - the N-rank control flow of this file (rank 0's
    # parity trainer while the others wait, the barriers, the all-reduced fields) rehearsed on a one-GPU box; its numbers mean nothing
    rehearse = os.environ.get("RUART_BENCH_REHEARSE_ONE_GPU") == "1"
    if rehearse:
        local = 0
    torch.cuda.set_device(local)
    device = torch.device("cuda", local)
    import torch.distributed as dist
    if rehearse and world > 1:
        dist.init_process_group("gloo")
    elif world > 1 or a.force_dp:
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        if a.force_dp and world == 1:
            os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
            os.environ.setdefault("MASTER_PORT", "29531")
            os.environ.setdefault("RANK", "0")
            os.environ.setdefault("WORLD_SIZE", "1")
        # the gradient all-reduce sits on the step's critical path (the optimizer waits for it) while the next batch's encoder
        # GEMMs fill the device from a normal-priority stream: give RCCL's stream the priority of the step's own streams
        pg_opts = dist.ProcessGroupNCCL.Options(is_high_priority_stream=os.environ.get("RUART_RCCL_PRIORITY", "1") != "0")
        dist.init_process_group("nccl", device_id=device, pg_options=pg_opts)

    from ruart_amd import hip, synth
    from ruart_amd.arguments import default_opt
    lib = hip.load()
    if a.mode == "bert512":
        return bert512(a, device, lib, out_stream)
    opt = default_opt(vocab_size=20000, cuda=True, device=device, bert_precision=a.precision, max_od_num=36, batch_size=a.batch)
    if os.environ.get("RUART_DP_PINNED_SCALAR"):          # experiments: the one-scalar form of the re-pinned rows' clip-norm share (dp.py)
        opt["dp_pinned_scalar"] = True
    if os.environ.get("RUART_STREAMS"):                   # experiments: 0 = the trunk's three branches on ONE stream
        opt["ruart_streams"] = os.environ["RUART_STREAMS"] != "0"
    # the loss / NaN readback of a step one step late, as SDNetTrainer.train() does inside its loop (trainer._defer_readback): this file
    # drives update() itself, so it asks for the same explicitly; RUART_DEFER_READBACK=0 = the per-step sync of a bare update() call
    opt["ruart_defer_readback"] = os.environ.get("RUART_DEFER_READBACK", "1") != "0"
    if os.environ.get("RUART_TILE_ORDER_TRAIN"):          # experiments: one GROUP_M for every encoder GEMM of the training step
        from ruart_amd import hip as _hip
        _hip.check(_hip.load().ruart_gemm_set_tile_order(int(os.environ["RUART_TILE_ORDER_TRAIN"])), "set_tile_order")
    if os.environ.get("RUART_TRUNK_GRAD_GEMM"):           # experiments: x1 = one bf16 product for the trunk's gradient GEMMs
        opt["ruart_trunk_grad_gemm"] = os.environ["RUART_TRUNK_GRAD_GEMM"]
    if os.environ.get("RUART_DP_OVERLAP"):                # experiments: bucket exchange overlapped with backward (dp.py)
        opt["dp_overlap_backward"] = True
    if a.graph_trunk is not None:
        opt["ruart_graph_trunk"] = bool(a.graph_trunk)
    if a.frozen_dropout:
        opt["bert_frozen_dropout"] = True
    if a.unlock_bert:
        opt.pop("LOCK_BERT")
        opt["bert_train_gemm"] = a.train_gemm
        a.no_roofline = True                     # the 16-bit encoder GEMM is not on this path
    cfg = synth.bert_config()                       # bert-base-uncased shape, vocab 30522
    n_ocr, n_od = 100, 36
    if a.stress:
        opt.update(BERT_LARGE=True, BERT_large_model_file="unused", max_ocr_num=300, max_od_num=100)
        cfg = synth.bert_config(hidden_size=1024, num_hidden_layers=24, num_attention_heads=16, intermediate_size=4096)
        n_ocr, n_od = 300, 100
    note("building model")
    tr, _ = build_trainer(opt, cfg, device, process_group=dist.group.WORLD if a.force_dp else None)
    dp = world > 1 or a.force_dp
    note("model ready; staging %d batches" % a.n_batches)

    # pre-stage synthetic batches (different data per rank), index vectors included
    batches = []
    for i in range(a.n_batches):
        b = synth.synthetic_batch(opt, a.batch, seed=7 + 1000 * rank + i, n_q=30, n_ocr=n_ocr, n_od=n_od)
        batches.append(tr.ToCUDA(b))
    host_batches = None
    if a.include_h2d:                            # what a loader worker produces: tensors on the host + the numpy batch index
        from ruart_amd.batch import BatchIndex
        host_batches = []
        for i in range(max(a.n_batches, 4)):     # four objects in rotation: current, lookahead, the one being staged, the one just retired
            hb = synth.synthetic_batch(opt, a.batch, seed=7 + 1000 * rank + i, n_q=30, n_ocr=n_ocr, n_od=n_od)
            hb[0]["_ruart_host_index"] = BatchIndex(hb[0], hb[1], hb[2], opt)
            if not os.environ.get("RUART_BENCH_PAGEABLE"):       # what DataLoader(pin_memory=True) does on its pinning thread
                from torch.utils.data._utils.pin_memory import pin_memory as _pin
                hb = _pin(hb)
            host_batches.append(hb)
    bi = batches[0][0]["_ruart_index"]
    real_tokens = bi.packed.T
    torch.cuda.synchronize()
    note("batches staged: %d real word pieces per batch" % real_tokens)
    parity = None
    golden = os.path.join(ROOT, "tests", "golden", "sdnet_e2e_full.npz")
    want_parity = (a.full and rank == 0 and not a.no_parity and not a.stress and not a.unlock_bert and a.batch == 64
                   and os.path.exists(golden))
    # The parity check runs AFTER the timed region, on a second trainer built from the same seeds (the weights the timed one started
    # from).  Round 5: run first, on the timed trainer, its no-grad forward left torch's caching allocator with a block layout the
    # training steps then reused - and the timed steps ran 0.7-1.0 ms slower for it (22.7 -> 23.5 ms on the same box, interleaved,
    # profiles/r05_knob_sweep.log; emptying the cache afterwards recovered most runs, not all).  RUART_BENCH_PARITY_FIRST=1: the old order.
    if want_parity and os.environ.get("RUART_BENCH_PARITY_FIRST") == "1":
        parity = live_parity(tr, opt, batches[0], golden)
        if parity is not None:
            parity["checked_on"] = "the timed trainer, before its warm-up (RUART_BENCH_PARITY_FIRST=1)"
        note("parity vs the reference's golden scores: %s" % parity)
        want_parity = False
    # Round 6 (advisor): the TIMED trainer is checked too - one forward of batch 0 in the timed schedule (the encoder pass on the
    # run-ahead stream, three-stream trunk, on the step stream) while its weights are still the seeded ones; the scores stay on the
    # device and are compared with the reference's after the timed region (no host sync here).  RUART_BENCH_TIMED_PARITY=0 skips it.
    timed_scores = None
    if want_parity and a.mode == "train" and os.environ.get("RUART_BENCH_TIMED_PARITY", "1") != "0":
        import ruart_amd.layers as _L
        _L.set_dropout_prob(0.0)
        tr.network.train()
        tr.network.drop_emb = False
        b0_ = batches[0]

        def _fwd0():
            if not a.no_prefetch:
                tr.network.prefetch_bert(b0_[0], b0_[1], b0_[2])        # the pass runs where the timed steps' passes run
            with torch.no_grad():
                return tr.network(b0_[0], b0_[1], b0_[2])[0].float().clone()
        timed_scores = tr.on_step_stream(_fwd0)
        _L.set_dropout_prob(0.0 if "DROPOUT" not in opt else float(opt["DROPOUT"]))

    def fresh(i):
        """The batch of step i: pre-staged on the device (default) or shipped from its host copy now (--include-h2d)."""
        if host_batches is None:
            return batches[i % len(batches)]
        hb = host_batches[i % len(host_batches)]
        hb[0].pop("_ruart_index", None)          # forget the previous round's device copy: ToCUDA ships everything again
        hb[0]["_ruart_host_index"].device = None
        return tr.ToCUDA(hb)

    staged = {}

    def step(i):
        b = staged.pop(i, None) or fresh(i)
        if host_batches is not None and not a.no_prefetch and i + 1 not in staged:
            staged[i + 1] = fresh(i + 1)           # the lookahead batch has to be on the device for its encoder pass
        if a.mode == "train":
            # steady-state pipeline: the frozen encoder pass of the NEXT batch overlaps this step's trunk; every timed step
            # still launches exactly one encoder pass and one full trunk forward/backward/optimizer step
            nb = None if a.no_prefetch else (staged[i + 1] if host_batches is not None else batches[(i + 1) % len(batches)])
            if host_batches is not None and not a.no_prefetch:
                # as SDNetTrainer.train does: the batch after next is shipped inside update(), where the host waits for the step anyway
                loss = tr.update(b, i, next_batch=nb, stage_next=lambda: fresh(i + 2))
                staged[i + 2] = tr.staged
                return loss
            return tr.update(b, i, next_batch=nb)
        else:
            tr.network.eval()
            tr.network.drop_emb = False
            if not a.no_prefetch:                 # same pipeline as training: the next batch's encoder pass beside this trunk
                nb = staged[i + 1] if host_batches is not None else batches[(i + 1) % len(batches)]
                tr.network.prefetch_bert(nb[0], nb[1], nb[2])
            def fwd_only():
                with torch.no_grad():
                    scores, _ = tr.network(b[0], b[1], b[2])
                scores.sum().item()               # as SDNetTrainer.predict: the host waits for every batch's scores (loss, decode)
            tr.on_step_stream(fwd_only)           # ... on the trainer's non-blocking step stream, as predict() runs (trainer.on_step_stream)

    def sync():
        torch.cuda.synchronize()
        if dp:
            dist.barrier()

    # Host pauses: a full (generation-2) collection of the interpreter walks every container object alive - the model, the staged
    # batches with the reference's nested python lists of word-piece offsets (~10^5 lists per batch) - and stops the host for tens
    # of ms once per ~25 steps: a 60 ms step in a 20-step run (round 5).  What is alive here stays alive for the
    # whole run, so it is moved out of the collector's sight (gc.freeze: a permanent generation), as a long-running trainer would do
    # after its set-up; collections still run, over the objects a step creates.  Every pause is logged and reported on the line.
    import gc
    gc_log = []

    def _gc_cb(phase, info, _t=[0.0]):
        if phase == "start":
            _t[0] = time.perf_counter()
        else:
            gc_log.append((time.perf_counter(), info["generation"], (time.perf_counter() - _t[0]) * 1e3))
    gc.callbacks.append(_gc_cb)
    if os.environ.get("RUART_BENCH_GC_FREEZE", "1") != "0":
        gc.collect()
        gc.freeze()
    import contextlib

    def caller_stream():
        """The loop that drives update() runs where SDNetTrainer.train() runs its own: with the training step stream current
        (trainer.step_stream; from torch's default stream every step is joined with the LEGACY stream on both sides, and those markers
        hold the next step's trunk back until the encoder pass beside it has ended: 22.75 -> 22.00 ms, profiles/HISTORY.md round 5 (12)).
        RUART_BENCH_CALLER_DEFAULT_STREAM=1: the caller on torch's default stream, as in rounds 1-4."""
        if a.mode != "train" or os.environ.get("RUART_BENCH_CALLER_DEFAULT_STREAM") == "1":
            return contextlib.nullcontext()
        return tr.step_stream()
    with caller_stream():
        for i in range(a.warmup):
            step(i)
            torch.cuda.synchronize()
            note("warmup step %d done" % i)
    # --dump-outputs: the last timed step's forward hands its answer scores to this hook (registered for that step only)
    last_scores, hook, loss = [], None, None
    sync()
    t0 = time.perf_counter()
    marks, enq = [], []
    with caller_stream():
        for i in range(a.steps):
            ts = time.perf_counter()
            if a.dump_outputs and rank == 0 and i == a.steps - 1:
                hook = tr.network.register_forward_hook(lambda m, args, out: last_scores.append(out[0]))
            # the step index runs on from the warm-up: timed step 0 consumes the encoder pass that the last warm-up step launched ahead,
            # so all K timed steps are the pipelined schedule (rounds 1-5 restarted at 0: with an odd warm-up the first timed step asked
            # for the batch that had NOT been encoded ahead and ran a 15-ms encoder pass inline, ~+0.2 ms on the 20-step mean)
            loss = step(a.warmup + i)
            marks.append(time.perf_counter())     # (host time at which step i's call returned: update() ends with the step's loss readback)
            enq.append((getattr(tr, "host_enqueued_at", ts) - ts) * 1e3)      # host time until the whole step was enqueued (train mode)
        if a.mode == "train":
            tr.flush_readback()               # the last step's loss and NaN flag are read (and asserted) inside the bracket too
    sync()
    dt = time.perf_counter() - t0
    if hook is not None:
        hook.remove()
        outputs = [("scores", last_scores[-1])]
        if a.mode == "train":
            outputs = [("loss", float(loss))] + outputs + [("param." + n, p) for n, p in tr.network.named_parameters() if p.requires_grad]
        dump_outputs(a.dump_outputs, outputs)
    # the spread of the timed steps, always on the line: a uniform slow run, a transient and a slow first step look different here
    per_step = [(b - a_) * 1e3 for a_, b in zip([t0] + marks[:-1], marks)]
    step_ms = _dist(per_step)
    step_ms["what"] = "host time between the returns of consecutive update() calls in the timed region (each ends with its step's loss readback)"
    step_ms["first_is"] = ("the first timed step: it starts behind the bracket's synchronisation (nothing queued ahead of it) and, since the step "
                           "index runs on from the warm-up, consumes the encoder pass the last warm-up step launched ahead")
    if a.mode == "train":
        step_ms["host_enqueue_median"] = round(sorted(enq)[len(enq) // 2], 3)
    pauses = [(g, ms) for t, g, ms in gc_log if t0 <= t <= t0 + dt]
    step_ms["gc"] = {"collections": len(pauses), "full_collections": sum(1 for g, _ in pauses if g == 2),
                     "total_ms": round(sum(ms for _, ms in pauses), 3), "longest_ms": round(max([ms for _, ms in pauses] + [0.0]), 3),
                     "frozen_setup": os.environ.get("RUART_BENCH_GC_FREEZE", "1") != "0"}
    if os.environ.get("RUART_BENCH_STEP_TIMES"):      # diagnostics: every timed step (stderr)
        note("per-step ms: " + " ".join("%.1f" % t for t in per_step))
    ranks_seen = 1
    if dp:
        t = torch.tensor([dt], device=device, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
        t = torch.ones(1, device=device, dtype=torch.float64)
        dist.all_reduce(t)                         # every rank that timed the region counts itself
        ranks_seen = int(t.item())
        dist.barrier()

    note("timed region: %.3f s for %d steps" % (dt, a.steps))
    # Two more passes of the same K steps with hipEvent pairs around every GEMM launch (on the stream it is launched on):
    #  * "inline": the encoder runs inside its own step, so each GEMM has the device to itself - the kernel's own roofline
    #    position (roofline.achieved / frac / avg_launch_us);
    #  * "timed": the schedule of the timed region (encoder of the next batch beside the trunk).  There a GEMM shares the CUs
    #    with the trunk's kernels, so its launch-to-finish time also contains the trunk's work (roofline.timed_region).
    roof = timeline = None
    if a.full and not a.no_roofline and a.precision in GEMM_KERNEL:
        def profiled_pass(prefetch, mode):
            """K more steps under the library's event recorder.  mode 1: a hipEvent pair around every encoder GEMM launch (the roofline
            figures; ~100 events per step, which stretch the pipelined step by 2-3 ms) plus the step-stream marks; mode 2: marks only -
            step stream at forward start / forward end / backward end / optimizer end, encoder stream before / after the pass that
            is launched in the step (six events per step: the schedule as it is timed).  Returns the recorder's arrays."""
            import ruart_amd.bert as bert_mod
            saved = a.no_prefetch
            a.no_prefetch = not prefetch
            net, optim = tr.network, tr.optimizer
            orig_fwd, orig_cs, orig_enc = net.forward, getattr(optim, "clip_and_step", None), bert_mod.bert_encode

            def mark(tag):
                lib.ruart_prof_mark(tag, hip.stream_ptr(device))

            def fwd(*x, **k):
                mark(1)
                out = orig_fwd(*x, **k)
                mark(2)
                return out

            def cs(*x, **k):
                mark(3)
                out = orig_cs(*x, **k)
                mark(4)
                return out

            def enc(*x, **k):
                mark(5)
                out = orig_enc(*x, **k)
                mark(6)
                return out
            if orig_cs is not None:
                net.forward, optim.clip_and_step = fwd, cs
                bert_mod.bert_encode = enc
            try:
                with caller_stream():                                     # (the timed region's schedule: see caller_stream)
                    step(0)                                               # settle the pipeline state of this schedule
                    torch.cuda.synchronize()
                    hip.check(lib.ruart_prof_enable(mode), "prof_enable")
                    for i in range(a.steps):
                        step(i + 1)
                    torch.cuda.synchronize()
                M = 8192
                b_, e_, f_, n_ = (ctypes.c_float * M)(), (ctypes.c_float * M)(), (ctypes.c_double * M)(), ctypes.c_int(0)
                hip.check(lib.ruart_prof_timeline(b_, e_, f_, M, ctypes.byref(n_)), "prof_timeline")
                lib.ruart_prof_enable(0)
            finally:
                a.no_prefetch = saved
                bert_mod.bert_encode = orig_enc
                if orig_cs is not None:
                    del net.forward                       # (instance attributes shadowing the class's methods)
                    del optim.clip_and_step
            return np.array(b_[:n_.value]), np.array(e_[:n_.value]), np.array(f_[:n_.value])

        def gemm_pass(prefetch, gemm_split=None):
            b_, e_, f_ = profiled_pass(prefetch, 1)
            g = f_ > 0
            if gemm_split is not None:
                gemm_split.update(_gemm_split(b_, e_, f_))
            return float((e_[g] - b_[g]).sum()), int(g.sum()), float(f_[g].sum())

        ms_i, n_i, fl_i = gemm_pass(False)
        pipelined = a.mode == "train" and not a.no_prefetch
        gsplit = {}
        ms_t, n_t, fl_t = gemm_pass(True, gsplit) if pipelined else (ms_i, n_i, fl_i)
        if pipelined and not a.no_timeline:
            timeline = _timeline(*profiled_pass(True, 2))
        if n_i and n_t:
            ach = fl_i / (ms_i * 1e-3) / 1e12
            ach_t = fl_t / (ms_t * 1e-3) / 1e12
            traffic = traffic_source = None
            tf = os.path.join(ROOT, "profiles", TRAFFIC_FILE)                    # PMC passes cannot run inside this process:
            if os.path.exists(tf) and a.batch == 64 and not a.stress:           # the committed rocprofv3 summary of this shape
                traffic = json.load(open(tf)).get(GEMM_KERNEL[a.precision], {}).get("avg_bytes_per_launch")
                traffic_source = "profiles/%s: a committed rocprofv3 --pmc summary of this kernel on this workload, NOT measured in this run" % TRAFFIC_FILE
            roof = {"bound": "mfma", "kernel": GEMM_KERNEL[a.precision], "achieved": round(ach_t, 1), "peak": PEAK_TFLOPS, "unit": "TFLOP/s",
                    "frac": round(ach_t / PEAK_TFLOPS, 4), "traffic": traffic, "traffic_source": traffic_source, "launches": n_t,
                    "avg_launch_us": round(ms_t * 1e3 / n_t, 2),
                    "schedule": "the timed region's: encoder of batch t+1 beside the trunk of batch t" if pipelined else "encoder inline",
                    "flops": "algorithmic, 2 * real_rows * N * K per launch" + (
                        "; the kernel also runs the fp8 correction product (same MFMA time again), which is not counted"
                        if a.precision == "fp16c" else ""),
                    "alone": {"schedule": "encoder inline (each GEMM alone on the device), same K steps", "achieved": round(ach, 1),
                              "frac": round(ach / PEAK_TFLOPS, 4), "avg_launch_us": round(ms_i * 1e3 / n_i, 2), "launches": n_i},
                    "gemm_share_of_step": round(ms_i / a.steps / (dt / a.steps * 1e3), 3),
                    # what `peak` is not: round 6 measured this kernel AT the socket's 1 400 W cap (1.84-1.91 GHz, profiles/r06_gemm_power.log)
                    "power_note": "peak is the nominal 2.4-GHz figure; NOT measured in this run: a pure f16 16x16x32 MFMA stream on random operands "
                                  "sustains %.0f TFLOP/s on this chip (fp8 16x16x128: %.0f), and this kernel runs at the socket power cap "
                                  "(profiles/r06_mfma_power.log, r06_gemm_power.log)" % (SUSTAINED_F16_TFLOPS, SUSTAINED_FP8_TFLOPS)}
            if gsplit:
                roof["timed_gemm_us"] = gsplit

    if want_parity:
        note("parity check on a second trainer built from the same seeds ...")
        torch.cuda.synchronize()
        tr2, _ = build_trainer(dict(opt, ruart_dp=False), cfg, device)      # rank 0 alone: a plain replica, no collective in its set-up
        try:
            b0 = tr2.ToCUDA(synth.synthetic_batch(opt, a.batch, seed=7 + 1000 * rank, n_q=30, n_ocr=n_ocr, n_od=n_od))
            parity = live_parity(tr2, opt, b0, golden)
            if parity is not None:
                parity["checked_on"] = "a replica: a second trainer built from the same seeds after the timed region (inline encoder pass)"
                if timed_scores is not None:
                    zz = np.load(golden)
                    if tuple(zz["scores"].shape) == tuple(timed_scores.shape):
                        dd = np.abs(timed_scores.cpu().numpy() - zz["scores"])
                        parity["timed_trainer"] = {"max_abs_err_vs_reference": float("%.3g" % dd.max()), "holds": bool(dd.max() < 1e-3),
                                                   "what": "the timed trainer's own forward of batch 0 before its first update, in the timed "
                                                           "schedule (run-ahead encoder stream, three-stream trunk)"}
        finally:
            torch.cuda.synchronize()
            tr2.network.Bert.close(destroy=True)
            del tr2
        note("parity vs the reference's golden scores: %s" % parity)

    b512 = None
    if a.full and rank == 0 and world == 1 and not a.no_bert512 and a.mode == "train" and not a.stress and not a.unlock_bert:
        note("north-star shape (64, 512), plain f16 ...")
        torch.cuda.empty_cache()
        r = bert512_measure(a, device, lib, "fp16", batch=64, steps=10, warmup=3)
        b512 = {"workload": "bert-base + attention forward over 64 x %d valid tokens, plain f16" % r["L"],
                "ms": round(r["dt"] * 1e3, 3), "tflops": round(r["flops"] / r["dt"] / 1e12, 1),
                "frac_of_peak": round(r["flops"] / r["dt"] / 1e12 / PEAK_TFLOPS, 4), "schedule": "%d stream(s)" % a.parts,
                "one_pass_ms": round(r["dt1"] * 1e3, 3), "one_pass_frac": round(r["flops"] / r["dt1"] / 1e12 / PEAK_TFLOPS, 4),
                "gemm_only_tflops": round(r["gemm_flops"] / (r["gemm_ms"] * 1e-3) / 1e12, 1) if r["gemm_n"] else None}

    if rank == 0:
        out = {"metric": ("VQA samples/sec fwd+bwd (B=64, q=30, ocr=%d)" if a.mode == "train" else "VQA samples/sec fwd-only (B=64, q=30, ocr=%d)") % n_ocr,
               "value": round(world * a.batch * a.steps / dt, 2), "unit": "samples/s", "n_gpus": world, "ranks_seen": ranks_seen, "steps": a.steps,
               "warmup": a.warmup, "ms_per_step": round(dt / a.steps * 1e3, 3), "higher_is_better": True, "scaling": "weak",
               "vs_baseline": None,
               "dtype": ("f16 activations / bf16 gradients, fp32 accumulate and master weights" if a.train_gemm == "16"
                         else "f32 storage, split-bf16 MFMA") if a.unlock_bert and a.precision != "fp32" else DTYPE[a.precision],
               "data": "synthetic",
               "config": {"workload": "RUArt training step, synthetic ST-VQA-shaped batch: B=%d/GPU, q=30 words, %d OCR items, "
                                      "%d objects, %s %s, SDNet trunk fwd+bwd, Adamax"
                                      % (a.batch, n_ocr, n_od, "bert-large 24x1024" if a.stress else "bert-base 12x768",
                                         "TRAINED (no LOCK_BERT)" if a.unlock_bert else "frozen"),
                          "global_batch": world * a.batch, "real_wordpieces_per_batch": int(real_tokens),
                          "parallelism": "dp%d" % world, "mode": a.mode,
                          "loop": ("update() driven as SDNetTrainer.train() drives it: on the trainer's step stream, the loss of a step "
                                   "read back one step late" if opt.get("ruart_defer_readback") else
                                   "update() with its per-step loss readback") if a.mode == "train" else None},
               "step_ms": step_ms, "timeline_ms": timeline if roof is not None else None,
               "roofline": roof, "parity": parity, "bert512": b512,
               "peak_hbm_gb": round(torch.cuda.max_memory_allocated(device) / 2 ** 30, 2)}
        if a.full and world == 1 and not a.no_cpu_baseline:
            note("cpu baseline (oracle) ...")
            out["cpu_baseline"] = cpu_baseline(opt, cfg, 1, runs=1) if a.stress else cpu_baseline(opt, cfg, a.cpu_samples)
        print(json.dumps(out), file=out_stream, flush=True)
    if dp:
        dist.barrier()
        dist.destroy_process_group()
    torch.cuda.synchronize()
    if getattr(tr.network, "Bert", None) is not None:
        tr.network.Bert.close(destroy=True)     # the CU-masked streams must not outlive the interpreter (hip.destroy_stream)
    tr._destroy_masked_streams()


if __name__ == "__main__":
    main()
