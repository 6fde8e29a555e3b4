"""Run-state checkpoints: everything a training step depends on, captured and restored so that a resumed run IS the uninterrupted
run, bit for bit (``SDNetTrainer.save`` / ``load_state``, opt['save_every'] / opt['resume_state']).

The file is the reference's dictionary (Models/SDNetTrainer.py:468-490), so ``SDNetTrainer.load_model`` reads it as a weights-only
checkpoint, plus one key of this project's own:

    {'state_dict': {'network', 'optimizer', 'updates'}, 'train_loss': {val, avg, sum, count}, 'config': ..., 'epoch': ...,
     'ruart': {'version', 'world', 'optimizer_class', 'optimizer_rule', 'trainable', 'next_batch', 'best', 'ranks': [per rank]}}

What a step depends on beyond the weights:
  * the optimizer: moments, the global and the per-tensor step counts (bias corrections, the encoder group's warm-up position, and the
    fused step's choice between its two staging buffers);
  * the counters ``updates`` (the deferred readback alternates two pinned slots by it) and the ``train_loss`` meter, the best-model
    records (or the first evaluation after a restart overwrites the best checkpoint with whatever it sees);
  * four random streams: torch's CPU generator (the trained encoder draws one seed per pass from it, and every DataLoader iterator
    one), the device's generator (the mask banks' ``bernoulli_``, the fp32-class encoder's dropouts), numpy's and ``random``'s;
  * BOTH mask banks' ``demand`` (``layers.mask_bank`` and the trunk's own): a bank sizes its pre-drawn buffer from the earlier steps'
    demand and a site the buffer cannot serve draws its own mask, so a fresh bank consumes the device generator differently from a
    warm one - restoring the generator alone diverges at the first step.
Parameters and optimizer state are the same on every data-parallel rank; streams and banks are not, hence ``ranks``.

Tensors and plain containers only: ``torch.load(path, map_location='cpu', weights_only=True)`` reads the file.  Generator states are
byte tensors, numpy's and ``random``'s states lists of ints.
"""
import os
import random

import numpy as np
import torch

FORMAT_VERSION = 1


# -- plain containers ---------------------------------------------------------------------------------------------------------
def to_plain(obj):
    """``obj`` with every tensor detached, on the CPU and in storage of its own, numpy scalars / arrays as python numbers / lists;
    containers keep their kind (dict, list, tuple).  Anything else is refused: the file holds no pickled classes."""
    if torch.is_tensor(obj):
        return obj.detach().to("cpu", copy=True).contiguous()
    if obj is None or isinstance(obj, (bool, int, float, str)):
        return obj
    if isinstance(obj, np.generic):
        return obj.item()
    if isinstance(obj, np.ndarray):
        return obj.tolist()
    if isinstance(obj, dict):
        return {to_plain(k): to_plain(v) for k, v in obj.items()}
    if isinstance(obj, (list, tuple)):
        return type(obj)(to_plain(v) for v in obj) if type(obj) in (list, tuple) else [to_plain(v) for v in obj]
    raise TypeError("train_state: %s is neither a tensor nor a plain container" % type(obj).__name__)


# -- random streams -----------------------------------------------------------------------------------------------------------
def capture_streams(device=None):
    """The four generators' states: torch's CPU generator, the device generator of ``device`` (a CUDA device; None / CPU: left out),
    numpy's global generator and ``random``'s."""
    name, keys, pos, has_gauss, cached = np.random.get_state()
    ver, internal, gauss_next = random.getstate()
    out = {"torch_cpu": torch.get_rng_state().clone(),
           "numpy": {"name": str(name), "keys": [int(k) for k in keys], "pos": int(pos), "has_gauss": int(has_gauss),
                     "cached_gaussian": float(cached)},
           "random": {"version": int(ver), "internal": [int(k) for k in internal], "gauss_next": gauss_next}}
    device = torch.device(device) if device is not None else None
    if device is not None and device.type == "cuda":
        out["torch_cuda"] = torch.cuda.get_rng_state(device).clone()
    return out


def restore_streams(streams, device=None):
    """Inverse of ``capture_streams``.  A device generator's state is required when ``device`` is a CUDA device."""
    torch.set_rng_state(streams["torch_cpu"].to(torch.uint8).cpu())
    n = streams["numpy"]
    np.random.set_state((n["name"], np.asarray(n["keys"], dtype=np.uint32), int(n["pos"]), int(n["has_gauss"]), float(n["cached_gaussian"])))
    r = streams["random"]
    random.setstate((int(r["version"]), tuple(int(k) for k in r["internal"]), r["gauss_next"]))
    device = torch.device(device) if device is not None else None
    if device is not None and device.type == "cuda":
        if "torch_cuda" not in streams:
            raise ValueError("train state: no device generator state in the file (it was written by a run on the CPU device)")
        torch.cuda.set_rng_state(streams["torch_cuda"].to(torch.uint8).cpu(), device)


# -- mask banks ---------------------------------------------------------------------------------------------------------------
def capture_bank(bank):
    """What ``MaskBank.begin_step`` will size the next step's buffers from: ``demand`` with the finished step's ``used`` folded in, as
    begin_step itself would do first.  [[p, elements], ...] in the bank's own order (one bernoulli_ launch per entry, in that order)."""
    demand = dict(bank.demand)
    for p, n in bank.used.items():
        demand[p] = max(demand.get(p, 0), n)
    return [[float(p), int(n)] for p, n in demand.items()]


def restore_bank(bank, demand):
    """REPLACE the bank's state - ``demand`` set, ``used`` and ``buf`` cleared; nothing of an earlier trainer's steps is merged in (the
    module-level ``layers.mask_bank`` survives from one trainer to the next inside a process)."""
    bank.demand = {float(p): int(n) for p, n in demand}
    bank.used = {}
    bank.buf = {}


def capture_rank(device, banks):
    """One rank's share of the file: its streams and its banks (``banks``: name -> MaskBank)."""
    return {"streams": capture_streams(device), "banks": {k: capture_bank(b) for k, b in banks.items()}}


def gather_ranks(entry, world=1, group=None):
    """Every rank's ``capture_rank`` entry, in rank order, on every rank (a collective over ``group`` when ``world`` > 1)."""
    if world <= 1:
        return [entry]
    out = [None] * world
    torch.distributed.all_gather_object(out, entry, group=group)
    return out


def restore_rank(entry, device, banks):
    for k, b in banks.items():
        if k not in entry["banks"]:
            raise ValueError("train state: no mask bank %r in the file" % (k,))
        restore_bank(b, entry["banks"][k])
    restore_streams(entry["streams"], device)


# -- optimizer ----------------------------------------------------------------------------------------------------------------
def optimizer_kind(optimizer):
    """(class name, rule of the encoder group or '') - what must agree between the run that saved and the run that resumes."""
    groups = getattr(optimizer, "param_groups", None) or []
    rule = groups[1].get("rule", "") if len(groups) > 1 and isinstance(groups[1], dict) else ""
    return type(optimizer).__name__, str(rule)


# -- the file -----------------------------------------------------------------------------------------------------------------
def pack(network_state, optimizer, updates, train_loss, config, epoch=None, trainable=(), next_batch=0, best=None, ranks=(), extra=None):
    """The checkpoint dictionary.  ``network_state``: name -> tensor (what ``load_model`` will read); ``optimizer``: the optimizer
    (its ``state_dict()`` is taken); ``train_loss``: an AverageMeter; ``trainable``: names of the parameters with requires_grad (all of
    them must be in ``network_state``); ``ranks``: one ``capture_rank`` entry per data-parallel rank, in rank order."""
    missing = [n for n in trainable if n not in network_state]
    if missing:
        raise ValueError("train state: trainable tensors not in the network state: %s" % missing[:5])
    cls, rule = optimizer_kind(optimizer)
    ruart = {"version": FORMAT_VERSION, "world": len(ranks), "optimizer_class": cls, "optimizer_rule": rule,
             "trainable": [str(n) for n in trainable], "next_batch": int(next_batch), "best": to_plain(dict(best or {})),
             "ranks": to_plain(list(ranks))}
    ruart.update(to_plain(dict(extra or {})))
    return {"state_dict": {"network": {k: to_plain(v) for k, v in network_state.items()},
                           "optimizer": to_plain(optimizer.state_dict()), "updates": int(updates)},
            "train_loss": {k: to_plain(getattr(train_loss, k)) for k in ("val", "avg", "sum", "count")},
            "config": {k: v for k, v in dict(config).items() if isinstance(v, (int, float, str, bool))},
            "epoch": to_plain(epoch), "ruart": ruart}


def write(ckpt, filename):
    """``torch.save`` under a temporary name in the same folder, then ``os.replace``: a job killed in mid-write leaves the previous
    file whole."""
    tmp = "%s.tmp.%d" % (filename, os.getpid())
    try:
        torch.save(ckpt, tmp)
        os.replace(tmp, filename)
    finally:
        if os.path.exists(tmp):
            os.remove(tmp)


def read(filename):
    """The dictionary of ``filename``; ValueError for a file that is no run state or of an unknown format version."""
    ckpt = torch.load(filename, map_location="cpu", weights_only=True)
    ruart = ckpt.get("ruart") if isinstance(ckpt, dict) else None
    if not isinstance(ruart, dict) or "version" not in ruart:
        raise ValueError("%s is not a run-state checkpoint (no 'ruart' entry): a weights-only file goes through load_model" % (filename,))
    if ruart["version"] != FORMAT_VERSION:
        raise ValueError("%s: unknown run-state format version %r (this code reads version %d)" % (filename, ruart["version"], FORMAT_VERSION))
    return ckpt


def check(ckpt, optimizer, named_tensors, trainable, world=1):
    """Refuse (ValueError naming the mismatch) a state that does not fit the run it is loaded into: format version, world size,
    optimizer class / rule / weight decay of the first group, a trainable tensor missing from the file, a tensor of another shape.  ``named_tensors``: name -> tensor of
    the live network (parameters and buffers); ``trainable``: the names with requires_grad."""
    ruart = ckpt.get("ruart")
    if not isinstance(ruart, dict) or ruart.get("version") != FORMAT_VERSION:
        raise ValueError("train state: unknown format version %r (this code reads version %d)"
                         % (ruart.get("version") if isinstance(ruart, dict) else None, FORMAT_VERSION))
    if int(ruart["world"]) != int(world) or len(ruart["ranks"]) != int(world):
        raise ValueError("train state: written by a run of world size %d, this run has world size %d: the per-rank random streams and "
                         "mask banks cannot be dealt out" % (int(ruart["world"]), int(world)))
    cls, rule = optimizer_kind(optimizer)
    if ruart["optimizer_class"] != cls:
        raise ValueError("train state: optimizer class %s in the file, this run steps with %s" % (ruart["optimizer_class"], cls))
    if ruart["optimizer_rule"] != rule:
        raise ValueError("train state: encoder group rule %r in the file, this run's is %r" % (ruart["optimizer_rule"], rule))
    # '#' and 'ADAM' step with one class (FusedAdamax, torch.optim.Adamax) and differ in the decay alone, which load_state_dict would overwrite
    saved = ckpt["state_dict"].get("optimizer")
    mine, theirs = getattr(optimizer, "param_groups", None) or [], (saved.get("param_groups") if isinstance(saved, dict) else None) or []
    if mine and theirs and isinstance(mine[0], dict) and isinstance(theirs[0], dict):
        wd, wd_file = float(mine[0].get("weight_decay", 0)), float(theirs[0].get("weight_decay", 0))
        if wd != wd_file:
            raise ValueError("train state: weight decay %g in the file, this run's optimizer has %g" % (wd_file, wd))
    net = ckpt["state_dict"]["network"]
    for n in trainable:
        if n not in net:
            raise ValueError("train state: trainable tensor %s is missing from the file" % (n,))
    for n, v in net.items():
        if n in named_tensors and tuple(named_tensors[n].shape) != tuple(v.shape):
            raise ValueError("train state: tensor %s has shape %s in the file and %s in this run"
                             % (n, tuple(v.shape), tuple(named_tensors[n].shape)))
    unknown = [n for n in ruart.get("trainable", ()) if n not in trainable]
    if unknown:
        raise ValueError("train state: the file trains tensors this run does not (%s): the optimizer states would not line up" % unknown[:5])


def restore_tensors(ckpt, named_tensors):
    """Copy the file's network tensors IN PLACE into the live ones (the fused optimizers hold raw pointers to them; the in-place copy
    also bumps their version counters, which the trained encoder's operand cache is keyed on).  Keys the network does not have are
    dropped, as ``load_model`` drops them."""
    with torch.no_grad():
        for n, v in ckpt["state_dict"]["network"].items():
            if n in named_tensors:
                named_tensors[n].copy_(v)


def restore_meter(meter, d):
    for k in ("val", "avg", "sum", "count"):
        setattr(meter, k, d[k])
