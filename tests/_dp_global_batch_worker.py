"""One rank of the two-rank opt['dp_global_batch'] checks (started by tests/test_gpu_dp_global_batch.py, one process per rank).

    python tests/_dp_global_batch_worker.py RANK WORLD PORT BACKEND DEVICE_INDEX PART

PART op:    each rank holds half of a tensor; the cross-rank layer norm's y and grad_x match the rows of the single-tensor op within
            1e-6 relative, the stats are bit-identical on both ranks.
PART model: a B = 8 single-process step against 2 x 4 shards (one at full item counts, one ragged and short), dropout off, the trunk's
            x3 products.  First: the front of the model (frozen encoder, embeddings, multi2one) gives every sample the same bits in
            one B = 8 pass as in two B = 4 passes.  With the switch: loss within 1e-6 relative, every averaged gradient within 1e-4
            (|delta| / |g|), after three update() calls (SGD, see part_model) parameters bit-identical across ranks and within 1e-5
            of the single process's.  Control: without the switch at least one gradient misses by more than 1e-2.
            The front is NOT bit-independent of batch composition (x_ocr / x_od 6.5e-6 / 6.9e-6 relative: reported, bounded at
            1e-5); the step comparisons pin the trunk's inputs to the B = 8 pass's front output (pin_front).
PART eval:  evaluate() over the golden dataset records at batch 2 per rank against one process at batch 4: answers, idx and the
            written files in the same order, ANLS / ACC within 1e-9, scores within 1e-4 (the unpinned front, see part_eval).
BACKEND gloo with both ranks on one device, or nccl (RCCL) with one GPU per rank.  Process-group timeout 120 s: a mismatched exchange
fails instead of hanging."""
import copy
import datetime
import json
import os
import sys
import tempfile

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def cat_batches(a, b):
    """Two collated batches -> one (samples of a, then of b): items are packed sample-major, so every field concatenates."""
    out = []
    for x, y in zip(a, b):
        if isinstance(x, dict):
            out.append({k: torch.cat([x[k], y[k]]) if isinstance(x[k], torch.Tensor) else x[k] + y[k] for k in x})
        elif isinstance(x, torch.Tensor):
            out.append(torch.cat([x, y]))
        else:
            out.append(x + y)
    return tuple(out)


def rel(a, b):
    return float((a - b).norm()) / max(float(b.norm()), 1e-30)


def part_op(rank, world, device):
    from ruart_amd import hip, ops
    from ruart_amd.dp import make_ln_groups
    g = make_ln_groups()[0]
    lib = hip.load()
    for shape in ((64, 100, 250), (64, 36, 250), (64, 40, 250), (6, 7, 13)):
        gen = torch.Generator().manual_seed(11)
        xf = (torch.randn(*shape, generator=gen) * 1.7 + 0.3).to(device)
        gyf = torch.randn(*shape, generator=gen).to(device)
        h = shape[0] // world
        x, gy = xf[rank * h:(rank + 1) * h].contiguous(), gyf[rank * h:(rank + 1) * h].contiguous()
        ref = xf.clone().requires_grad_(True)
        yr = ops.whole_layer_norm(ref)
        yr.backward(gyf)
        y, stats = ops.whole_ln_global_fwd(x, 1e-5, g)
        gx = ops.whole_ln_global_bwd(y, gy, stats, g)
        xa = x.clone().requires_grad_(True)                  # the autograd Function: the same bits
        ya = ops.whole_layer_norm(xa, group=g)
        ya.backward(gy)
        assert torch.equal(ya, y) and torch.equal(xa.grad, gx), shape
        assert rel(y, yr[rank * h:(rank + 1) * h].detach()) < 1e-6, (shape, rel(y, yr[rank * h:(rank + 1) * h].detach()))
        assert rel(gx, ref.grad[rank * h:(rank + 1) * h]) < 1e-6, (shape, rel(gx, ref.grad[rank * h:(rank + 1) * h]))
        s0 = stats.clone()
        dist.broadcast(s0, src=0)
        assert torch.equal(s0, stats), shape
        # against the single-tensor statistics: fp32 summation order only
        ws, st1 = torch.empty(4096, device=device), torch.empty(2, device=device)
        hip.check(lib.ruart_whole_ln_fwd(hip.ptr(xf), hip.ptr(torch.empty_like(xf)), hip.ptr(st1), hip.ptr(ws), xf.numel(), 1e-5,
                                         hip.stream_ptr()), "ruart_whole_ln_fwd")
        assert abs(float(stats[0] - st1[0])) <= 1e-6 * max(1.0, abs(float(st1[0]))) and abs(float(stats[1] / st1[1]) - 1) < 1e-6
    torch.cuda.synchronize(device)
    return "op: 4 shapes"


def _model_opt(batch_size):
    from ruart_amd import synth
    from ruart_amd.arguments import default_opt
    opt = default_opt(vocab_size=1500, cuda=True, DROPOUT=0.0, dropout_emb=0.0)
    opt["batch_size"] = batch_size
    cfg = synth.bert_config(vocab_size=2000)
    opt["bert_state"], opt["bert_config"] = synth.make_bert_weights(cfg, seed=1033), cfg
    return opt, synth.make_sdnet_weights(opt, seed=1033)


def part_model(rank, world, device):
    from ruart_amd import synth
    from ruart_amd.trainer import SDNetTrainer
    assert world == 2
    opt, sw = _model_opt(4)
    # the three update() calls use SGD: Adamax normalises each element's step by its max |g|, so an element whose gradient is near zero
    # moves by +-lr on summation-order noise (measured: parameters 1.8e-3 apart after three Adamax steps with gradients within 1e-4);
    # SGD's step is the gradient's, which is what the 1e-5 bound is about (at lr 0.1 the largest difference after three steps was
    # 6.4e-4, in deep_attn.int_attn_list.2.scoring.linear.weight; it scales with lr).  Gradients do not depend on the optimizer.
    opt.update(optimizer="SGD", lr=1e-3)
    emb = {"glove_embedding": T(sw["glove_embed.weight"]), "fast_embedding": T(sw["fast_embed.weight"])}

    def make(data_parallel, global_batch):
        o = dict(opt, ruart_dp=data_parallel, dp_global_batch=global_batch)
        tr = SDNetTrainer(o, device=device, process_group=dist.group.WORLD if data_parallel else None)
        tr.setup_model(emb)
        tr.network.load_state_dict({k: T(v) for k, v in sw.items()})
        return tr

    def shards(seed):
        full = synth.synthetic_batch(opt, 4, seed=seed, n_q=10, n_ocr=24, n_od=7, bert_vocab=2000, ragged=False)
        short = synth.synthetic_batch(opt, 4, seed=seed + 1, n_q=6, n_ocr=16, n_od=4, bert_vocab=2000, ragged=True)
        return [full, short]

    sh = shards(5)
    whole = cat_batches(sh[0], sh[1])
    plain = make(False, False)
    assert plain.grad_sync is None and not plain.global_batch

    # 1. the front of the model is per-sample: one B = 8 pass == two B = 4 passes, bit for bit
    def front(tr, batch):
        got = {}

        def cap(*args):
            got["args"] = [a.detach().clone() for a in args]
            return lambda *a: None
        tr.network._trunk_callable = cap
        try:
            b = tr.ToCUDA(batch)
            tr.network.eval()
            with torch.no_grad():
                tr.network(b[0], b[1], b[2])
        finally:
            del tr.network._trunk_callable
        torch.cuda.synchronize(device)
        return got["args"]
    f8, f4 = front(plain, whole), [front(plain, s) for s in sh]
    names = ("q_input", "q_raw", "q_mask", "x_ocr", "x_od", "ocr_mask", "od_mask", "ocr_pos", "od_pos")
    front_diff = {}
    for i, a in enumerate(f8):
        if a.dim() == 0 or a.size(0) != 8:
            continue
        if not (torch.equal(a[:4], f4[0][i]) and torch.equal(a[4:], f4[1][i])):
            b = torch.cat([f4[0][i], f4[1][i]]).float()
            front_diff[names[i]] = rel(a.float(), b)
    # Reported, not asserted: the OCR words' front is not bit-independent of batch composition (the ragged packed multi2one
    # recurrence runs GEMMs whose row count is the batch's number of live items).  It stays at the level of fp32 summation order,
    # and the bounds below are checked unchanged on top of it.
    print("rank %d front: not bit-identical in %s" % (rank, {k: "%.2e" % v for k, v in front_diff.items()}), flush=True)
    assert all(v < 1e-5 for v in front_diff.values()), front_diff

    def pin_front(tr, target, rows):
        """The trunk of ``tr`` sees exactly ``target[i][rows]`` (a B = 8 pass's front output) as its batched float inputs - value
        (x - x.detach()) + t == t bit for bit, gradient still flowing into this rank's own front - so that what is compared below is
        the trunk, the part whose layer norms couple the samples, not the front's summation-order sensitivity reported above."""
        def patched(*args):
            new = [(a - a.detach()) + target[i][rows] if (a.dim() > 0 and a.is_floating_point() and a.size(0) == len(range(8)[rows]))
                   else a for i, a in enumerate(args)]
            trunk = type(tr.network)._trunk_callable(tr.network, *new)
            return lambda *_: trunk(*new)
        tr.network._trunk_callable = patched

    def grads(tr, batch):
        b = tr.ToCUDA(batch)
        tr.network.train()
        tr.network.drop_emb = True
        scores, _ = tr.network(b[0], b[1], b[2])
        loss = tr.loss_func(scores, b[3])
        tr.optimizer.zero_grad(set_to_none=True)
        loss.backward()
        if tr.grad_sync is not None:
            tr.grad_sync.average_gradients()
        torch.cuda.synchronize(device)
        return float(loss.detach()), {n: p.grad.detach().clone() for n, p in tr.network.named_parameters() if p.grad is not None}

    mine = slice(4 * rank, 4 * rank + 4)
    pin_front(plain, f8, slice(0, 8))
    l_ref, g_ref = grads(plain, whole)
    glob = make(True, True)
    assert glob.global_batch and glob.network.ln_groups()[0] is not None
    ctrl = make(True, False)
    assert not ctrl.global_batch and ctrl.network.ln_groups() == (None, None, None)
    pin_front(glob, f8, mine)
    pin_front(ctrl, f8, mine)

    def dp_check(tr):
        l, g = grads(tr, sh[rank])
        lt = torch.tensor([l], dtype=torch.float64, device=device)
        dist.all_reduce(lt)
        worst = {}
        for n, r in g_ref.items():
            d = g.get(n, torch.zeros_like(r))
            worst[n] = float((d - r).norm()) / float(r.norm()) if float(r.norm()) > 0 else float((d - r).norm())
        return float(lt) / world, worst
    lg, wg = dp_check(glob)
    lc, wc = dp_check(ctrl)
    print("rank %d: loss %.9g vs %.9g; worst gradients %s; control %.3e" % (rank, lg, l_ref, [(n, "%.2e" % v) for n, v in sorted(
        wg.items(), key=lambda t: -t[1])[:3]], max(wc.values())), flush=True)
    assert abs(lg - l_ref) <= 1e-6 * abs(l_ref), (lg, l_ref)
    bad = {n: v for n, v in wg.items() if v > 1e-4}
    assert not bad, "rank %d: gradients off the B = 8 step: %s" % (rank, sorted(bad.items(), key=lambda t: -t[1])[:5])
    assert max(wc.values()) > 1e-2, "control: without the switch every gradient is within 1e-2 (max %.3e)" % max(wc.values())

    # 2. three optimizer steps: replicas bit-identical, and the single process at B = 8
    steps = [shards(50 + 10 * i) for i in range(3)]
    lp, lq = [], []
    for i, s_ in enumerate(steps):
        for tr in (plain, glob):
            del tr.network._trunk_callable
        f = front(plain, cat_batches(s_[0], s_[1]))
        pin_front(plain, f, slice(0, 8))
        pin_front(glob, f, mine)
        lp.append(float(plain.update(plain.ToCUDA(cat_batches(s_[0], s_[1])), i)))
        lq.append(float(glob.update(glob.ToCUDA(s_[rank]), i)))
    assert all(np.isfinite(lp)) and all(np.isfinite(lq))
    torch.cuda.synchronize(device)
    sp = dict(plain.network.named_parameters())
    diverged, far = [], []
    for n, p in glob.network.named_parameters():
        t = p.detach().clone()
        dist.broadcast(t, src=0)
        if not torch.equal(t, p.detach()):
            diverged.append(n)
        d = float((p.detach() - sp[n].detach()).abs().max()) if p.numel() else 0.0
        if d > 1e-5:
            far.append((n, d))
    assert not diverged, "rank %d: replicas diverged in %s" % (rank, diverged[:5])
    assert not far, "rank %d: parameters off the single process's after 3 steps: %s" % (rank, sorted(far, key=lambda t: -t[1])[:5])
    for tr in (glob, ctrl, plain):
        tr.close()
    return "model: loss %.8f vs %.8f, worst gradient %.2e (control %.2e), 3 steps" % (lg, l_ref, max(wg.values()), max(wc.values()))


def part_eval(rank, world, device):
    from ruart_amd import synth
    from ruart_amd.arguments import default_opt
    from ruart_amd.dataset import VQA_Dataset
    from ruart_amd.trainer import SDNetTrainer
    with open(os.path.join(ROOT, "tests", "golden", "dataset_input.json"), encoding="utf-8") as f:
        inp = json.load(f)
    tmp = tempfile.mkdtemp(prefix="dpgb_eval_%d_" % rank)
    vocab = os.path.join(tmp, "vocab.txt")
    with open(vocab, "w", encoding="utf-8") as f:
        f.write("\n".join(inp["vocab"]) + "\n")
    opt = default_opt(datadir="", BERT_tokenizer_file=vocab, cuda=True, DROPOUT=0.0, dropout_emb=0.0)
    cfg = synth.bert_config(vocab_size=2000)
    opt["bert_state"], opt["bert_config"] = synth.make_bert_weights(cfg, seed=77), cfg
    sw = synth.make_sdnet_weights(opt, seed=77)
    emb = {"glove_embedding": T(sw["glove_embed.weight"]), "fast_embedding": T(sw["fast_embed.weight"])}
    B = 2

    def make(data_parallel, batch_size, folder):
        o = dict(opt, ruart_dp=data_parallel, dp_global_batch=data_parallel, batch_size=batch_size)
        tr = SDNetTrainer(o, device=device, process_group=dist.group.WORLD if data_parallel else None)
        tr.setup_model(emb)
        tr.network.load_state_dict({k: T(v) for k, v in sw.items()})
        os.makedirs(folder, exist_ok=True)
        tr.saveFolder = folder
        return tr

    single = make(False, world * B, os.path.join(tmp, "single"))
    glob = make(True, B, os.path.join(tmp, "dp"))
    out = []
    for mode, fname in (("dev", "save_res_last.json"), ("test", "submission.json")):
        ds = VQA_Dataset(copy.deepcopy(inp["records"]), opt, mode=mode)
        assert len(ds) % (world * B) != 0, len(ds)
        r1 = single.evaluate(ds, 0, mode)
        r2 = glob.evaluate(ds, 0, mode)
        assert [x["question_id"] for x in r1[3]] == [x["question_id"] for x in r2[3]], mode
        assert [x["answer"] for x in r1[3]] == [x["answer"] for x in r2[3]], mode
        assert abs(r1[1] - r2[1]) <= 1e-9 and abs(r1[2] - r2[2]) <= 1e-9, (mode, r1[1:3], r2[1:3])
        assert abs(r1[0] - r2[0]) <= 1e-5 * max(1.0, abs(r1[0])), (mode, r1[0], r2[0])
        for t in (r2[0], r2[1], r2[2]):                       # every rank returns the same global metrics
            v = torch.tensor([t], dtype=torch.float64, device=device)
            dist.broadcast(v, src=0)
            assert float(v) == t
        written = os.path.exists(os.path.join(glob.saveFolder, fname))
        assert written == (rank == 0), (mode, rank, written)
        if rank == 0:
            with open(os.path.join(single.saveFolder, fname)) as f:
                a = json.load(f)
            with open(os.path.join(glob.saveFolder, fname)) as f:
                b = json.load(f)
            assert len(a) == len(b) and len(a) > 0, (len(a), len(b))
            for x, y in zip(a, b):
                assert set(x) == set(y)
                for k in x:
                    if k == "score":
                        # not 1e-5: evaluation runs the front unpinned, and the front's output depends on batch composition at
                        # ~7e-6 relative (part_model); measured 5.8e-5 on the top score of one record
                        assert abs(x[k] - y[k]) <= 1e-4, (mode, x[k], y[k])
                    else:
                        assert x[k] == y[k], (mode, k, x[k], y[k])
        out.append("%s: %d results, ANLS %.4f ACC %.4f" % (mode, len(r2[3]), r2[1], r2[2]))
    single.close(final=True)
    glob.close(final=True)
    return "eval: " + "; ".join(out)


def main():
    rank, world, port, backend, dev_index, part = (int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], sys.argv[4], int(sys.argv[5]),
                                                   sys.argv[6])
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=port, HSA_ENABLE_IPC_MODE_LEGACY="0")
    from ruart_amd import dp
    device = torch.device("cuda", dev_index)
    torch.cuda.set_device(device)
    timeout = datetime.timedelta(seconds=120)
    if backend == "nccl":
        dp.init_process_group(device, "nccl", rank=rank, world_size=world, timeout=timeout)
    else:
        dist.init_process_group("gloo", rank=rank, world_size=world, timeout=timeout)
    msg = {"op": part_op, "model": part_model, "eval": part_eval}[part](rank, world, device)
    dist.barrier()
    dist.destroy_process_group()
    print("rank %d ok: %s" % (rank, msg), flush=True)


if __name__ == "__main__":
    main()
