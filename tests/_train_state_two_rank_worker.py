"""One rank of the two-rank run-state check (started by tests/test_gpu_train_state.py, one process per rank and launch).

    python tests/_train_state_two_rank_worker.py RANK WORLD RENDEZVOUS_FILE BACKEND DEVICE_INDEX PHASE FOLDER

The shipped conf with its dropouts on, a DIFFERENT shard per rank and step, the frozen encoder one step ahead, gradients averaged by
``dp.GradSync``.  PHASE ``first``: two steps, ``save`` (a collective: every rank contributes its streams and banks, rank 0 writes
FOLDER/train_state.pt), then - a new trainer in the same process - the uninterrupted run of four steps, whose parameters go to
FOLDER/straight_r<RANK>.pt.  PHASE ``second``, in fresh processes: ``load_state``, the remaining two steps, parameters to
FOLDER/resumed_r<RANK>.pt.  The parent compares the files."""
import copy
import datetime
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEPS, CUT = 4, 2


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def main():
    rank, world, rdzv, backend, dev_index, phase, folder = (int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], sys.argv[4], int(sys.argv[5]),
                                                            sys.argv[6], sys.argv[7])
    os.environ.update(HSA_ENABLE_IPC_MODE_LEGACY="0")
    # a rendezvous file, not a port probed free by the parent: another process can take such a port before rank 0 listens on it
    kw = dict(init_method="file://" + rdzv, rank=rank, world_size=world, timeout=datetime.timedelta(seconds=120))
    from ruart_amd import dp, synth
    from ruart_amd import layers as L
    from ruart_amd.arguments import default_opt
    from ruart_amd.trainer import SDNetTrainer
    device = torch.device("cuda", dev_index)
    torch.cuda.set_device(device)
    if backend == "nccl":
        dp.init_process_group(device, "nccl", **kw)
    else:
        dist.init_process_group("gloo", **kw)

    opt = default_opt(vocab_size=1500, cuda=True)
    assert float(opt["DROPOUT"]) > 0 and float(opt["dropout_emb"]) > 0
    cfg = synth.bert_config(vocab_size=2000)
    opt["bert_state"], opt["bert_config"] = synth.make_bert_weights(cfg, seed=1033), cfg
    sw = synth.make_sdnet_weights(opt, seed=1033)
    emb = {"glove_embedding": T(sw["glove_embed.weight"]), "fast_embedding": T(sw["fast_embed.weight"])}
    host = [synth.synthetic_batch(opt, 3 + rank, seed=50 + 10 * i + rank, n_q=10, n_ocr=14, n_od=5, bert_vocab=2000, ragged=True)
            for i in range(STEPS)]
    path = os.path.join(folder, "train_state.pt")

    def make():
        L.mask_bank = L.MaskBank()                   # every arm starts with a bank of its own
        tr = SDNetTrainer(dict(opt), device=device, process_group=dist.group.WORLD)
        tr.setup_model(emb)
        tr.network.load_state_dict({k: T(v) for k, v in sw.items()})
        assert tr.grad_sync is not None and tr.grad_sync.world == world
        return tr, [tr.ToCUDA(b) for b in copy.deepcopy(host)]

    def run(tr, batches, lo, hi):
        losses = [float(tr.update(batches[i], i, next_batch=batches[i + 1] if i + 1 < STEPS else None)) for i in range(lo, hi)]
        assert all(np.isfinite(losses)), losses
        return losses

    def dump(tr, name):
        torch.cuda.synchronize(device)
        torch.save({"params": {n: p.detach().cpu() for n, p in tr.network.named_parameters()}, "updates": tr.updates},
                   os.path.join(folder, "%s_r%d.pt" % (name, rank)))

    if phase == "first":
        tr, batches = make()
        run(tr, batches, 0, CUT)
        tr.save(path)
        tr.close(final=True)
        dist.barrier()
        assert os.path.exists(path)
        tr, batches = make()
        losses = run(tr, batches, 0, STEPS)
        dump(tr, "straight")
    else:
        tr, batches = make()
        L.mask_bank.demand = {0.4: 12345}            # restoring replaces the bank's state
        assert tr.load_state(path) == CUT and tr.updates == CUT
        losses = run(tr, batches, CUT, STEPS)
        dump(tr, "resumed")
    tr.close(final=True)
    dist.barrier()
    dist.destroy_process_group()
    print("rank %d ok: %s, losses %s" % (rank, phase, ["%.6f" % l for l in losses]), flush=True)


if __name__ == "__main__":
    main()
