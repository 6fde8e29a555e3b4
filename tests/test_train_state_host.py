"""ruart_amd/train_state.py without a GPU: the random streams, a mask bank on the CPU device, the file (written through ``pack``, read
with ``weights_only=True``, restored into fresh clones of a toy ``AdamaxAdam`` run), the refusals, and two gloo ranks whose per-rank
streams go into rank 0's file and come back to their own rank."""
import os
import random

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from ruart_amd import layers as L
from ruart_amd import train_state as TS

CPU = torch.device("cpu")


def _draws():
    return torch.rand(5), torch.randint(0, 2 ** 31 - 1, (1,)), np.random.rand(3), np.random.permutation(7), random.random(), random.gauss(0, 1)


def _same(a, b):
    return all(torch.equal(x, y) if torch.is_tensor(x) else np.array_equal(x, y) for x, y in zip(a, b))


def test_streams_round_trip():
    torch.manual_seed(11)
    np.random.seed(12)
    random.seed(13)
    np.random.standard_normal(1)            # leaves numpy with a cached gaussian, random with a gauss_next below
    random.gauss(0, 1)
    state = TS.to_plain(TS.capture_streams(None))
    assert "torch_cuda" not in state and state["numpy"]["has_gauss"] in (0, 1)
    first = _draws()
    second = _draws()
    assert not _same(first, second)
    TS.restore_streams(state, None)
    assert _same(_draws(), first)
    assert _same(_draws(), second)


# (rows, cols, p) of one step's dropout sites: two probabilities, a repeated shape, sizes that are no multiple of four
TAKES = [(3, 8, 0.3), (5, 7, 0.4), (3, 8, 0.3), (7, 13, 0.3), (2, 5, 0.4)]
TAKES_BIG = TAKES + [(9, 300, 0.3)]        # beyond what the pre-drawn buffer of the earlier demand holds (n * 1.05 + 1024): fallback


def _bank_step(bank, takes=TAKES):
    bank.begin_step(CPU)
    like = torch.zeros(1)
    return [bank.take(r, c, p, like).clone() for r, c, p in takes]


def test_mask_bank_round_trip_on_cpu():
    torch.manual_seed(21)
    bank = L.MaskBank()
    _bank_step(bank)                        # fresh bank: every site draws its own mask
    _bank_step(bank)                        # warm bank: slices of the pre-drawn buffers
    demand = TS.capture_bank(bank)
    gen = TS.capture_streams(None)
    assert sorted(p for p, _ in demand) == [0.3, 0.4] and all(n > 0 for _, n in demand)
    want = _bank_step(bank, TAKES_BIG)

    fresh = L.MaskBank()
    fresh.demand, fresh.used = {0.9: 77}, {0.9: 5}      # what an earlier trainer left behind: replaced, not merged
    TS.restore_bank(fresh, TS.to_plain(demand))
    TS.restore_streams(gen, None)
    assert fresh.buf == {} and fresh.used == {} and TS.capture_bank(fresh) == demand
    got = _bank_step(fresh, TAKES_BIG)
    assert len(got) == len(want) and all(torch.equal(a, b) for a, b in zip(got, want))
    assert TS.capture_bank(fresh) == TS.capture_bank(bank)        # (the restored bank's demand grows as the original's does)

    # control: the generator alone, into a bank with empty demand - the fallback path draws differently
    cold = L.MaskBank()
    TS.restore_streams(gen, None)
    ctrl = _bank_step(cold, TAKES_BIG)
    assert any(not torch.equal(a, b) for a, b in zip(ctrl, want))


class _Meter:
    val, avg, sum, count = 0.25, 0.5, 1.5, 3


def _toy(seed=3):
    """(name -> parameter, AdamaxAdam over them): two trunk tensors, two encoder tensors (one without decay), warm-up in effect"""
    from ruart_amd.optim import AdamaxAdam
    g = torch.Generator().manual_seed(seed)
    named = {"trunk.w": torch.randn(4, 3, generator=g), "trunk.b": torch.randn(3, generator=g),
             "Bert.bert_model.enc.weight": torch.randn(3, 3, generator=g), "Bert.bert_model.enc.bias": torch.randn(3, generator=g)}
    named = {k: torch.nn.Parameter(v) for k, v in named.items()}
    ps = list(named.values())
    return named, AdamaxAdam(ps[:2], ps[2:], [ps[3]], lr=2e-3, bert_lr=1e-3, rule="adamw", warmup=0.5, t_total=6)


def _toy_step(named, optimizer, i):
    x = torch.arange(12, dtype=torch.float32).reshape(4, 3).mul(0.1).add(i)
    w, b, ew, eb = named.values()
    loss = (((x.t() @ w + b) @ ew + eb) ** 2).sum()
    optimizer.zero_grad(set_to_none=True)
    loss.backward()
    optimizer.clip_and_step(10.0)


def _toy_ckpt(steps=3, ranks=None, **kw):
    named, optimizer = _toy()
    for i in range(steps):
        _toy_step(named, optimizer, i)
    ranks = ranks if ranks is not None else [TS.capture_rank(None, {"front": L.MaskBank()})]
    ckpt = TS.pack({k: v for k, v in named.items()}, optimizer, steps, _Meter, {"lr": 2e-3, "SEED": 1033, "skipped": [1, 2]}, epoch=0,
                   trainable=list(named), next_batch=steps, best={"ANLS": 0.5, "ACC": 0.25, "ANLS_batch": 0, "ACC_batch": 0}, ranks=ranks, **kw)
    return named, optimizer, ckpt


def test_file_round_trip(tmp_path):
    named, optimizer, ckpt = _toy_ckpt()
    path = str(tmp_path / "train_state.pt")
    TS.write(ckpt, path)
    assert os.listdir(tmp_path) == ["train_state.pt"]              # the temporary name is gone
    back = TS.read(path)                                            # torch.load(weights_only=True) inside
    assert torch.load(path, map_location="cpu", weights_only=True)["ruart"]["version"] == TS.FORMAT_VERSION
    assert back["config"] == {"lr": 2e-3, "SEED": 1033} and back["epoch"] == 0 and back["state_dict"]["updates"] == 3
    assert back["train_loss"] == {"val": 0.25, "avg": 0.5, "sum": 1.5, "count": 3}
    assert back["ruart"]["next_batch"] == 3 and back["ruart"]["world"] == 1 and back["ruart"]["optimizer_class"] == "AdamaxAdam"
    # readable the way load_model reads it: name -> tensor under ['state_dict']['network']
    net = back["state_dict"]["network"]
    assert set(net) == set(named) and all(torch.equal(net[k], named[k].detach()) for k in named)
    assert all(net[k].data_ptr() != named[k].data_ptr() for k in named)

    named2, optimizer2 = _toy(seed=99)                              # other weights, no steps taken
    TS.check(back, optimizer2, named2, list(named2), world=1)
    ptrs = {k: v.data_ptr() for k, v in named2.items()}
    TS.restore_tensors(back, named2)
    optimizer2.load_state_dict(back["state_dict"]["optimizer"])
    assert ptrs == {k: v.data_ptr() for k, v in named2.items()}     # in place
    _toy_step(named, optimizer, 3)
    _toy_step(named2, optimizer2, 3)
    assert optimizer.step_count == optimizer2.step_count == 4
    for (k, p), q in zip(named.items(), named2.values()):
        assert torch.equal(p.detach(), q.detach()), k
        assert optimizer.steps[id(p)] == optimizer2.steps[id(q)] == 4, k
        sa, sb = optimizer.state[id(p)], optimizer2.state[id(q)]
        assert set(sa) == set(sb) and len(sa) >= 3
        for name in sa:
            assert torch.equal(torch.as_tensor(sa[name]), torch.as_tensor(sb[name])), (k, name)
    # control: the weights-only way (fresh moments, step counts and warm-up position) takes another step
    named3, optimizer3 = _toy(seed=99)
    TS.restore_tensors(back, named3)
    _toy_step(named3, optimizer3, 3)
    assert any(not torch.equal(p.detach(), q.detach()) for p, q in zip(named.values(), named3.values()))


def test_pack_refuses_what_is_no_plain_container():
    named, optimizer = _toy()
    with pytest.raises(TypeError, match="plain container"):
        TS.pack(dict(named), optimizer, 0, _Meter, {}, trainable=list(named), ranks=[{"streams": object()}])
    with pytest.raises(ValueError, match="trunk.b"):
        TS.pack({k: v for k, v in named.items() if k != "trunk.b"}, optimizer, 0, _Meter, {}, trainable=list(named))


def test_refusals(tmp_path):
    from ruart_amd.optim import AdamaxAdam
    named, optimizer, ckpt = _toy_ckpt()
    names = list(named)
    TS.check(ckpt, optimizer, named, names, world=1)
    with pytest.raises(ValueError, match="world size 1.*world size 2"):
        TS.check(ckpt, optimizer, named, names, world=2)
    with pytest.raises(ValueError, match="optimizer class AdamaxAdam.*Adamax"):
        TS.check(ckpt, torch.optim.Adamax(list(named.values())), named, names, world=1)
    ps = list(named.values())
    with pytest.raises(ValueError, match="rule 'adamw'.*'bertadam'"):
        TS.check(ckpt, AdamaxAdam(ps[:2], ps[2:], [ps[3]], rule="bertadam"), named, names, world=1)
    less = dict(ckpt, state_dict=dict(ckpt["state_dict"], network={k: v for k, v in ckpt["state_dict"]["network"].items() if k != "trunk.b"}))
    with pytest.raises(ValueError, match="trunk.b is missing"):
        TS.check(less, optimizer, named, names, world=1)
    other = dict(named, **{"trunk.w": torch.nn.Parameter(torch.zeros(5, 3))})
    with pytest.raises(ValueError, match=r"trunk.w has shape \(4, 3\) in the file and \(5, 3\)"):
        TS.check(ckpt, optimizer, other, names, world=1)
    with pytest.raises(ValueError, match="trains tensors this run does not"):
        TS.check(ckpt, optimizer, named, names[:-1], world=1)
    future = dict(ckpt, ruart=dict(ckpt["ruart"], version=TS.FORMAT_VERSION + 1))
    with pytest.raises(ValueError, match="unknown format version %d" % (TS.FORMAT_VERSION + 1)):
        TS.check(future, optimizer, named, names, world=1)
    path = str(tmp_path / "future.pt")
    TS.write(future, path)
    with pytest.raises(ValueError, match="unknown run-state format version"):
        TS.read(path)
    torch.save({"state_dict": {"network": {}}, "config": {}}, path)          # a save_for_predict file
    with pytest.raises(ValueError, match="not a run-state checkpoint"):
        TS.read(path)


def _rank_draws():
    return [torch.rand(4), torch.from_numpy(np.random.rand(3)), torch.tensor([random.random()], dtype=torch.float64)]


def _gloo_worker(rank, world, folder):
    dist.init_process_group("gloo", init_method="file://" + os.path.join(folder, "rendezvous"), rank=rank, world_size=world)
    try:
        torch.manual_seed(1033 + 7919 * rank)            # the trainer's per-rank reseeding
        np.random.seed(40 + rank)
        random.seed(50 + rank)
        bank = L.MaskBank()
        bank.demand = {0.3: 100 + rank}
        bank.used = {0.3: 7, 0.4: 50 + rank}
        _rank_draws()
        ranks = TS.gather_ranks(TS.capture_rank(None, {"front": bank}), world, None)      # collective: every rank contributes
        cont = _rank_draws()                              # what this rank goes on to draw
        path = os.path.join(folder, "train_state.pt")
        if rank == 0:
            TS.write(_toy_ckpt(ranks=ranks)[2], path)     # one file, a per-rank list
        dist.barrier()
        torch.manual_seed(999)
        np.random.seed(999)
        random.seed(999)
        ckpt = TS.read(path)
        fresh = L.MaskBank()
        TS.restore_rank(ckpt["ruart"]["ranks"][rank], None, {"front": fresh})
        torch.save({"cont": cont, "again": _rank_draws(), "demand": TS.capture_bank(fresh), "world": ckpt["ruart"]["world"]},
                   os.path.join(folder, "r%d.pt" % rank))
    finally:
        dist.destroy_process_group()


def test_two_gloo_ranks_keep_their_own_streams(tmp_path):
    world = 2
    mp.spawn(_gloo_worker, args=(world, str(tmp_path)), nprocs=world, join=True)
    ckpt = TS.read(str(tmp_path / "train_state.pt"))
    assert ckpt["ruart"]["world"] == 2 and len(ckpt["ruart"]["ranks"]) == 2
    r = [torch.load(str(tmp_path / ("r%d.pt" % i)), weights_only=True) for i in range(world)]
    for i in range(world):
        assert all(torch.equal(a, b) for a, b in zip(r[i]["cont"], r[i]["again"])), i
        assert r[i]["demand"] == [[0.3, 100 + i], [0.4, 50 + i]] and r[i]["world"] == 2
    assert all(not torch.equal(a, b) for a, b in zip(r[0]["again"], r[1]["again"]))
    with pytest.raises(ValueError, match="world size 2"):
        named, optimizer = _toy()
        TS.check(ckpt, optimizer, named, list(named), world=1)
