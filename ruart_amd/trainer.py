"""``SDNetTrainer`` / ``BaseTrainer`` - the reference's training-loop surface (Models/SDNetTrainer.py:29-518,
Models/BaseTrainer.py:6-69) over the MI355X hot path, plus single-node data parallelism.

Kept from the reference: ``setup_model(vocab_embedding)``, ``update(batch, batch_i) -> float``, ``predict(batch)``,
``evaluate(data_loader, ...)``, ``ToCUDA(batch)``, ``load_model(path)``, ``save_for_predict(path)``,
``instance_bce_with_logits`` (the probabilities are fed to BCE-with-logits and scaled by the label width, :510-518),
optimizer selection by ``opt['optimizer']`` (:307-317), global-norm clipping (:366), re-pinning of embedding rows
>= ``tune_partial`` after every step (:369-373), checkpoint format (:492-509, 453-466), ``save(filename, epoch, prev_filename)``
(:468-490) - extended to the whole run state, with ``load_state`` as its inverse and opt['save_every'] / opt['resume_state'] in
``train()``: a resumed run is the uninterrupted run bit for bit (train_state.py).

New: ``world_size > 1`` => one process per GPU, gradients averaged with RCCL (dp.GradSync) before clipping; every rank
holds identical parameters, so the step is "N independent B-sample reference steps with averaged gradients"
(SURVEY.md section 8e).  ``opt['dp_global_batch']`` (off by default) makes the W-rank step the single-process step at batch
W * batch_size instead: the trunk's whole-tensor layer norms take their statistics over all ranks (SDNet.set_ln_groups) and
``evaluate`` deals the global batches over the ranks and gathers the results back in the single process's order.  With it on,
``update()``, ``predict()`` and ``evaluate()`` are collective calls: every rank calls them the same number of times, with shards
of ``batch_size`` samples.  ``train()`` / ``predict_for_test()`` without arguments follow the reference end to end - vocabulary and
word vectors from ``train_meta.msgpack``, records from ``{train,val,test}-preprocessed.msgpack`` through ``dataset.VQA_Dataset``,
run folder, best-model checkpoints, ``submission.json`` - and ``train`` also takes any iterable of collated batches.  The offline
preprocessing itself (spaCy / fastText / detector outputs -> msgpack) stays out of scope.
"""
import json
import logging
import os
import random
import time

import numpy as np
import torch
import torch.nn as nn
import torch.optim as optim

from . import layers as L
from .batch import VQA_collate, to_device
from .metrics import FRONT_ANSWERS as _FRONT_ANSWERS         # the no_read / yes / no slots of ``label_yesno``, in slot order
from .sampler import VQA_Sampler, merge_rank_shards
from .sdnet import SDNet

log = logging.getLogger(__name__)


class _PendingLoss:
    """What ``update`` returns while the readback of its step is deferred: ``float()`` / ``item()`` resolve it (a device sync if the
    step is still running)."""

    def __init__(self, trainer, pending):
        self._trainer, self._pending = trainer, pending

    def item(self):
        if self._pending["value"] is None:          # still the trainer's outstanding step: resolve it (and only it) now
            self._trainer.flush_readback()
        return self._pending["value"]

    __float__ = item

    def __format__(self, spec):
        return format(self.item(), spec)

    def __repr__(self):
        return repr(self.item())

    # arithmetic and comparisons resolve the value (the reference's update() returns a float)
    def __add__(self, o): return self.item() + o
    def __radd__(self, o): return o + self.item()
    def __sub__(self, o): return self.item() - o
    def __rsub__(self, o): return o - self.item()
    def __mul__(self, o): return self.item() * o
    def __rmul__(self, o): return o * self.item()
    def __truediv__(self, o): return self.item() / o
    def __rtruediv__(self, o): return o / self.item()
    def __neg__(self): return -self.item()
    # comparisons with anything that is not a number answer as a plain float's would (NotImplemented -> False / TypeError from
    # Python itself), and the value hashes as the float it stands for: ``loss == None``, ``loss in some_list`` and set / dict
    # membership stay legal, as they are for the float the reference's update() returns
    @staticmethod
    def _num(o):
        if isinstance(o, _PendingLoss):
            return o.item()
        if isinstance(o, (bool, int, float)):
            return float(o)
        try:
            import numbers
            if isinstance(o, numbers.Real) or (hasattr(o, "__float__") and getattr(o, "ndim", 0) == 0):
                return float(o)
        except (TypeError, ValueError):
            pass
        return None

    def _cmp(self, o, op):
        v = self._num(o)
        return NotImplemented if v is None else op(self.item(), v)

    def __lt__(self, o): return self._cmp(o, lambda a, b: a < b)
    def __le__(self, o): return self._cmp(o, lambda a, b: a <= b)
    def __gt__(self, o): return self._cmp(o, lambda a, b: a > b)
    def __ge__(self, o): return self._cmp(o, lambda a, b: a >= b)
    def __eq__(self, o): return self._cmp(o, lambda a, b: a == b)
    def __hash__(self): return hash(self.item())


class AverageMeter:
    """Utils/CoQAUtils.py:837-858."""

    def __init__(self):
        self.val = self.avg = self.sum = self.count = 0

    def update(self, val, n=1):
        self.val = val
        self.sum += val * n
        self.count += n
        self.avg = self.sum / self.count


def _credit(a, c, n_answers):
    """What one decoded answer adds to the ANLS / ACC sums (Models/SDNetTrainer.py:441-446): the ten-answers rule and the 0.5 floor."""
    return (a if a >= 0.5 else 0), (min(c * 10 / 3.0, 1) if n_answers == 10 else min(c * 10, 1))


def _slot_metrics(scores, idx, valid, cnt, n_front, extra_info, want_bound):
    """The metric values of a decode on the GPU: the (candidate x answer) table of the batch once (metrics.answer_table: one launch of
    ``ruart_edit_distance_pairs``), the chosen slot's ANLS / ACC gathered on the device and brought back with the chosen index in ONE
    readback.  Sample b's candidates are the front answers, its ``ocr_list`` strings and "unanswerable": slot s decodes to candidate s
    while s < n_front + num_cnt, to "unanswerable" behind that - the decode's own rule.  ``want_bound``: also the best credit over the
    admitted slots (``valid``, plus the fallback slot when nothing is admissible).  -> rows [idx, anls, acc (, best ANLS credit, best
    ACC credit)] as python floats."""
    from .metrics import answer_table
    dev = scores.device
    n_ocr = [len(e["ocr_list"]) for e in extra_info]
    for i, e in enumerate(extra_info):                       # (the host path's ocr_list[idx] raises the same way)
        if int(cnt[i]) > n_ocr[i]:
            raise IndexError("sample %d: num_cnt %d exceeds its %d ocr_list strings" % (i, int(cnt[i]), n_ocr[i]))
    front = list(_FRONT_ANSWERS[:n_front])
    anls, acc = answer_table([front + list(e["ocr_list"]) + ["unanswerable"] for e in extra_info], [e["answers"] for e in extra_info], dev)
    ar = torch.arange(scores.shape[1], device=dev).unsqueeze(0)
    cnt_t = torch.as_tensor([int(c) for c in cnt], device=dev).unsqueeze(1)
    last = torch.as_tensor(n_ocr, device=dev).unsqueeze(1) + n_front
    cand = torch.where(ar < n_front + cnt_t, ar, last)
    slot_anls, slot_acc = anls.gather(1, cand), acc.gather(1, cand)
    pick = idx.unsqueeze(1)
    cols = [idx.double(), slot_anls.gather(1, pick).squeeze(1), slot_acc.gather(1, pick).squeeze(1)]
    if want_bound:
        adm = valid.scatter(1, pick, True)
        ten = torch.as_tensor([e["answers"] is not None and len(e["answers"]) == 10 for e in extra_info], device=dev).unsqueeze(1)
        zero = torch.zeros((), dtype=torch.float64, device=dev)
        a = torch.where(slot_anls >= 0.5, slot_anls, zero)
        three = torch.full((), 3.0, dtype=torch.float64, device=dev)        # (a tensor divisor: a scalar one becomes a reciprocal product)
        c = torch.where(ten, (slot_acc * 10 / three).clamp(max=1), (slot_acc * 10).clamp(max=1))
        cols += [torch.where(adm, a, zero).max(dim=1).values, torch.where(adm, c, zero).max(dim=1).values]
    return torch.stack(cols, dim=1).cpu().tolist()


def _host_bound(valid_row, idx, answer_of, answers):
    """The CPU path of ``opt['eval_upper_bound']`` for one sample: the best credit over the admitted slots, with the host functions."""
    from .metrics import note_stvqa, note_textvqa
    slots = [s for s, v in enumerate(valid_row) if v or s == idx]
    got = [_credit(note_stvqa(answers, answer_of(s)), note_textvqa(answers, answer_of(s)), len(answers)) for s in slots]
    return max(g[0] for g in got), max(g[1] for g in got)


def decode_predictions(scores, num_cnt, extra_info, opt, bound=None):
    """The answer decode of Models/SDNetTrainer.py:391-450 for scores (B, n_slots) on any device: per sample the reference walks
    the slots by descending score, skips the ``<OCR>`` sentinel and the padding slots (>= num_cnt), stops at the first real OCR
    token - or at the no-answer slot (last column, ``label_no_answer``) if that comes first.  A descending walk that stops at the
    first admissible slot is a masked arg-max, done here in one device op for the batch.  When nothing is admissible the
    reference's loop runs out and is left with the LOWEST-scored slot; that case is reproduced too.
    Returns (ANLS sum, ACC sum, res, save_res) as the reference's ``predict`` does after the loss.  Scores on the GPU: the per-sample
    metric values come out of the batch's answer table (``_slot_metrics``) instead of ``note_stvqa`` / ``note_textvqa`` calls per sample;
    they are the same floats, and they are added up here in sample order as before.  ``bound`` (a list, ``opt['eval_upper_bound']``)
    receives per sample the best (ANLS, ACC) credit any admitted slot would have earned, None for a sample without answers."""
    from .metrics import note_stvqa, note_textvqa
    if "label_yesno" in opt or "fixed_answers" in opt:
        raise NotImplementedError("yes/no and fixed-answer slots are outside the accelerated path (SURVEY section 8)")
    B, n_slots = scores.shape
    no_answer = "label_no_answer" in opt
    cnt = torch.as_tensor(list(num_cnt), device=scores.device)
    sentinel = torch.as_tensor([len(e["ocr_list"]) - 1 for e in extra_info], device=scores.device)
    ar = torch.arange(n_slots, device=scores.device).unsqueeze(0)
    valid = (ar < cnt.unsqueeze(1)) & (ar != sentinel.unsqueeze(1))
    if no_answer:
        valid[:, -1] = True
    best = scores.masked_fill(~valid, -1.0).argmax(dim=1)
    idx_t = torch.where(valid.any(dim=1), best, scores.argmin(dim=1))
    rows = _slot_metrics(scores, idx_t, valid, num_cnt, 0, extra_info, bound is not None) if scores.is_cuda else None
    idxs = [int(r[0]) for r in rows] if rows is not None else idx_t.cpu().tolist()
    valid_h = valid.tolist() if bound is not None and rows is None else None
    prob = scores.detach().cpu()
    res, save_res, ANLS, ACC = [], [], 0, 0
    for i, idx in enumerate(idxs):
        def answer_of(s):
            return extra_info[i]["ocr_list"][s] if s < int(num_cnt[i]) else "unanswerable"
        answer = answer_of(idx)
        res.append({"question_id": extra_info[i]["q_id"], "answer": answer})
        save_res.append({"question_id": extra_info[i]["q_id"], "prediction": answer, "answers": extra_info[i]["answers"],
                         "score": prob[i, idx].item(), "idx": idx, "ids_len": n_slots, "ocr_list": extra_info[i]["ocr_list"]})
        if extra_info[i]["answers"] is not None:
            if rows is None:
                a = note_stvqa(extra_info[i]["answers"], answer)
                c = note_textvqa(extra_info[i]["answers"], answer)
            else:
                a, c = rows[i][1], rows[i][2]
            ACC += min(c * 10 / 3.0, 1) if len(extra_info[i]["answers"]) == 10 else min(c * 10, 1)
            ANLS += a if a >= 0.5 else 0
            if bound is not None:
                bound.append(tuple(rows[i][3:5]) if rows is not None else _host_bound(valid_h[i], idx, answer_of, extra_info[i]["answers"]))
        elif bound is not None:
            bound.append(None)
    return ANLS, ACC, res, save_res


def decode_slots(scores, num_cnt, extra_info, opt, bound=None):
    """``decode_predictions`` for the layout of ``label_yesno``: scores (B, 3 + n_ocr_slots (+ 1)) with the no_read / yes / no slots in
    front (Models/SDNetTrainer.py:396-448 with fixed_answers_len = 0, yesno_num = 3), again as one masked arg-max on the device.
    A slot is admissible when idx < 3 + num_cnt - or it is the no-answer slot (last column, ``label_no_answer``), where the walk stops
    first - and idx != len(ocr_list) - 1.  Both of the reference's quirks are kept (sic): that sentinel test is not offset by the three
    front slots, so slot len(ocr_list) - 1 - a real OCR item (or a front slot) - is skipped, and slot 3 + num_cnt - 1, the ``<OCR>``
    sentinel itself, is admissible and decodes to "<OCR>".  Nothing admissible: the lowest-scored slot, as in ``decode_predictions``.
    Scores on the GPU and ``bound``: as in ``decode_predictions``."""
    from .metrics import note_stvqa, note_textvqa
    if "fixed_answers" in opt:
        raise NotImplementedError("fixed-answer slots are outside the accelerated path (SURVEY section 8)")
    front = len(_FRONT_ANSWERS)
    B, n_slots = scores.shape
    no_answer = "label_no_answer" in opt
    cnt = torch.as_tensor(list(num_cnt), device=scores.device)
    skipped = torch.as_tensor([len(e["ocr_list"]) - 1 for e in extra_info], device=scores.device)
    ar = torch.arange(n_slots, device=scores.device).unsqueeze(0)
    valid = (ar < front + cnt.unsqueeze(1)) & (ar != skipped.unsqueeze(1))
    if no_answer:
        valid[:, -1] = True                      # (tested before the skip: the walk stops there even when it is the skipped index)
    best = scores.masked_fill(~valid, -1.0).argmax(dim=1)
    idx_t = torch.where(valid.any(dim=1), best, scores.argmin(dim=1))
    rows = _slot_metrics(scores, idx_t, valid, num_cnt, front, extra_info, bound is not None) if scores.is_cuda else None
    idxs = [int(r[0]) for r in rows] if rows is not None else idx_t.cpu().tolist()
    valid_h = valid.tolist() if bound is not None and rows is None else None
    prob = scores.detach().cpu()
    res, save_res, ANLS, ACC = [], [], 0, 0
    for i, idx in enumerate(idxs):
        def answer_of(s):
            if s < front:
                return _FRONT_ANSWERS[s]
            if s < front + int(num_cnt[i]):
                return extra_info[i]["ocr_list"][s - front]
            return "unanswerable"
        answer = answer_of(idx)
        res.append({"question_id": extra_info[i]["q_id"], "answer": answer})
        save_res.append({"question_id": extra_info[i]["q_id"], "prediction": answer, "answers": extra_info[i]["answers"],
                         "score": prob[i, idx].item(), "idx": idx, "ids_len": n_slots, "ocr_list": extra_info[i]["ocr_list"]})
        if extra_info[i]["answers"] is not None:
            if rows is None:
                a = note_stvqa(extra_info[i]["answers"], answer)
                c = note_textvqa(extra_info[i]["answers"], answer)
            else:
                a, c = rows[i][1], rows[i][2]
            ACC += min(c * 10 / 3.0, 1) if len(extra_info[i]["answers"]) == 10 else min(c * 10, 1)
            ANLS += a if a >= 0.5 else 0
            if bound is not None:
                bound.append(tuple(rows[i][3:5]) if rows is not None else _host_bound(valid_h[i], idx, answer_of, extra_info[i]["answers"]))
        elif bound is not None:
            bound.append(None)
    return ANLS, ACC, res, save_res


class BaseTrainer:
    """Models/BaseTrainer.py:6-69: option plumbing, the feature folder, the run folder."""

    def __init__(self, opt):
        self.opt = opt
        self.isTrain = False
        self.use_cuda = opt.get("cuda") is True
        self.saveFolder = opt.get("saveFolder", ".")
        self.opt.setdefault("logFile", "log.txt")
        if "source_dir" in opt and "datadir" in opt:     # :20-21; a caller-provided FEATURE_FOLDER stands otherwise
            opt["FEATURE_FOLDER"] = os.path.join(opt["datadir"], "./source/data/" + opt["source_dir"] + "/")

    def getSaveFolder(self):
        """Training: the first free ``<datadir>/conf~/run_<n>``; otherwise the folder the loaded model lives in (:49-62)."""
        if self.isTrain:
            runid = 1
            while os.path.exists(os.path.join(self.opt["datadir"], "conf~", "run_" + str(runid))):
                runid += 1
            self.saveFolder = os.path.join(self.opt["datadir"], "conf~", "run_" + str(runid))
            os.makedirs(self.saveFolder)
            log.info("Saving logs, model and evaluation in %s", self.saveFolder)
        else:
            self.saveFolder = os.path.join(self.opt["datadir"], "/".join(self.opt["MODEL_PATH"].split("/")[:2]))
            os.makedirs(self.saveFolder, exist_ok=True)

    def saveConf(self):
        if "confFile" not in self.opt:
            return
        with open(self.opt["confFile"], encoding="utf-8") as f, \
                open(os.path.join(self.saveFolder, "conf_copy"), "w", encoding="utf-8") as fw:
            fw.writelines(f)


def predict_checkpoint_keys(keys, opt, trained=()):
    """The keys ``save_for_predict`` writes, in order: the reference's set (Models/SDNetTrainer.py:492-509 drops every contextual
    encoder's and the fixed embeddings' tensors) and - with ``opt['bert_train_layers']``, and only then - the ``Bert.bert_model.*``
    tensors among ``trained`` (the names of the parameters with ``requires_grad``): the encoder layers this conf trains, which the
    BERT checkpoint a predictor starts from does not hold."""
    skip = ("CoVe", "ELMo", "AllenELMo", "Bert")
    drop = ("eval_embed.weight", "fixed_embedding_fast", "fixed_embedding_glove")
    keep = set(k for k in trained if k.startswith("Bert.bert_model.")) if "bert_train_layers" in opt else set()
    return [k for k in keys if (not k.startswith(skip) and k not in drop) or k in keep]


class SDNetTrainer(BaseTrainer):
    def __init__(self, opt, device=None, process_group=None):
        super().__init__(opt)
        L.set_dropout_prob(0.0 if "DROPOUT" not in opt else float(opt["DROPOUT"]))
        self.seed = int(opt["SEED"])
        random.seed(self.seed)
        np.random.seed(self.seed)
        torch.manual_seed(self.seed)
        self._rank_seeded = False
        self.batch_size = opt["batch_size"]
        self.device = torch.device(device if device is not None else "cuda")
        if self.device.type == "cuda":
            # one process drives ONE GPU: make it the current device, so that every stream query, allocation and kernel launch
            # below (the ctypes-launched HIP kernels take torch's current stream) targets this rank's device
            torch.cuda.set_device(self.device if self.device.index is not None else torch.cuda.current_device())
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.process_group = process_group
        self.grad_sync = None
        self.global_batch = False          # opt['dp_global_batch'] in effect (setup_model)
        self.fixed_answers_len = 0
        # conf key img_feature: a ready region-feature table {'img_id2idx', 'img_features', 'img_spatials'} for every VQA_Dataset this
        # trainer builds (the reference fills it from hdf5, Models/SDNetTrainer.py load_image_features - not rebuilt here: set the
        # attribute); None: the datasets read per-image files under opt['img_fea_folder']
        self.img_features = None
        self.updates = 0
        self.next_batch_i = 0              # index of the batch the next update() is due (save / load_state)
        self.best_ANLS = self.best_ACC = -1
        self.best_ANLS_batch = self.best_ACC_batch = -1

    # -- model / optimizer ------------------------------------------------------------------------------------
    def setup_model(self, vocab_embedding):
        from .optim import check_bert_optimizer
        bert_group = check_bert_optimizer(self.opt)          # opt['bert_optimizer']: refuses a conf that cannot have the group (ValueError)
        if self.opt.get("dp_global_batch"):
            if self.opt.get("dp_overlap_backward"):
                raise ValueError("opt['dp_global_batch'] does not combine with opt['dp_overlap_backward']: the gradient hooks' collectives "
                                 "would interleave with the layer norms' exchanges in backward")
            if self.opt.get("ruart_graph_trunk"):
                raise ValueError("opt['dp_global_batch'] does not combine with opt['ruart_graph_trunk']: the cross-rank layer norms "
                                 "exchange statistics with collectives, which the captured trunk cannot replay")
        self.train_loss = AverageMeter()
        self.staged = None                 # what update(stage_next=...) staged last
        opt = dict(self.opt)
        opt["device"] = self.device
        self.network = SDNet(opt, vocab_embedding).to(self.device)
        for name in ("fixed_embedding_fast", "fixed_embedding_glove"):
            if hasattr(self.network, name):
                setattr(self.network, name, getattr(self.network, name).to(self.device))
        params = [p for p in self.network.parameters() if p.requires_grad]
        from .optim import select_optimizer
        o = self.opt["optimizer"]
        # '#' steps fused unless opt['ruart_fused_optimizer'] is false; 'ADAM', 'ADAM2' and 'SGD' only with the key present and true
        kind = select_optimizer(self.opt, self.device.type)
        fused = kind.startswith("Fused")
        pinned = {}
        if "TUNE_PARTIAL" in self.opt and (fused or bert_group is not None):
            # rows >= tune_partial are re-pinned after every step: the fused optimizers never update them
            for flag, name in (("FastText", "fast_embed"), ("GLOVE", "glove_embed")):
                if flag in self.opt and getattr(self.network, name).weight.requires_grad:
                    pinned[getattr(self.network, name).weight] = self.opt["tune_partial"]
        if o == "ADAM":
            if fused:
                from .optim import FusedAdamax
                self.optimizer = FusedAdamax(params, lr=1e-3, weight_decay=0.5, pinned=pinned)
            else:
                self.optimizer = optim.Adamax(params, weight_decay=0.5, lr=1e-3)
        elif o == "#":
            if bert_group is not None:
                # opt['bert_optimizer']: the trained encoder steps as an Adam-family group of its own, the rest stays under Adamax
                from .optim import AdamaxAdam, FusedAdamaxAdam, split_parameters
                trunk, encoder, no_decay = split_parameters(self.network.named_parameters())
                self.optimizer = (FusedAdamaxAdam if fused else AdamaxAdam)(trunk, encoder, no_decay, lr=self.opt.get("lr", 2e-3),
                                                                            pinned=pinned, **bert_group)
            elif fused:
                from .optim import FusedAdamax
                self.optimizer = FusedAdamax(params, lr=self.opt.get("lr", 2e-3), pinned=pinned)
            else:
                self.optimizer = optim.Adamax(params, lr=self.opt.get("lr", 2e-3))
        elif o == "ADAM2":
            if fused:
                from .optim import FusedAdam
                self.optimizer = FusedAdam(params, lr=self.opt.get("lr", 1e-3), pinned=pinned)
            else:
                self.optimizer = optim.Adam(params, lr=self.opt.get("lr", 1e-3))
        else:                # 'SGD' (select_optimizer has refused anything else)
            if fused:
                from .optim import FusedSGD
                self.optimizer = FusedSGD(params, lr=self.opt["lr"], pinned=pinned)
            else:
                self.optimizer = optim.SGD(params, lr=self.opt["lr"])
        if self.opt["loss"] in ("BCE", "BCE_D1"):
            self.loss_func = self.instance_bce_with_logits
        elif self.opt["loss"] == "CE":
            self.loss_func = nn.functional.cross_entropy
        else:
            raise ValueError("loss parameter is error")
        self.updates = 0
        # opt['ruart_dp'] = False: a plain single-replica trainer even inside an initialised process group (tests compare against it)
        if self.opt.get("ruart_dp", True) and (self.process_group is not None or (
                torch.distributed.is_available() and torch.distributed.is_initialized() and torch.distributed.get_world_size() > 1)):
            from .dp import GradSync
            # default: the embedding tables are exchanged whole, so the clip norm is the exact norm of the averaged gradient;
            # opt['dp_pinned_scalar'] (fused optimizer only) represents the re-pinned rows by one scalar instead (dp.py)
            self.grad_sync = GradSync(self.network, self.opt, group=self.process_group,
                                      pinned_scalar=bool(self.opt.get("dp_pinned_scalar")) and hasattr(self.optimizer, "clip_and_step"))
            self.grad_sync.broadcast_parameters()
            if self.opt.get("dp_global_batch"):
                # the step of one process at the global batch: layer-norm statistics over all ranks, one process group per trunk branch
                from .dp import make_ln_groups
                self.network.set_ln_groups(make_ln_groups(self.process_group))
                self.global_batch = True
            # the replicas share their parameters, not their dropout masks: every rank seeded torch identically above (so that the
            # initial weights agree even before the broadcast), which would make all ranks draw the SAME variational-dropout masks
            # step after step.  From here on each rank's generators run their own stream.
            rank = torch.distributed.get_rank(self.process_group)
            if rank > 0 and not self._rank_seeded:
                torch.manual_seed(self.seed + 7919 * rank)
            self._rank_seeded = True

    def close(self, final=False):
        """End of a session: the deferred loss check, the encoder pass still running ahead (``Bert.close``).  ``final=True`` - the
        END OF THE PROCESS's use of this trainer (bench.py, the tools, ``__graft_entry__``, a script's last call) - also destroys the
        CU-masked run-ahead stream (hipExtStreamCreateWithCUMask, the default in the fp16c mode): alive at static destruction it takes a
        process with a tool library loaded (rocprofv3, any other HSA tool) down in __cxa_finalize.  Between
        sessions (``train()``, a stand-alone ``evaluate()``, ``predict_for_test()`` call this without ``final`` on every exit path) the
        stream is KEPT: a re-created one can land on a trunk stream's hardware queue slot (``Bert.close``).  The decision is the
        caller's, not a guess from the environment (round 5 looked for "rocprof" in environment variables; RUART_DESTROY_STREAMS=1
        still forces the destruction for experiments)."""
        import sys
        unwinding = sys.exc_info()[0] is not None      # called from a ``finally`` while another exception propagates
        try:
            self.flush_readback()
        except AssertionError as e:
            if not unwinding:
                raise                        # nothing else is propagating: the deferred NaN / loss assert IS the error
            print("ruart_amd: deferred loss check failed during unwinding: %s" % (e,), file=sys.stderr)
        finally:
            bert = getattr(getattr(self, "network", None), "Bert", None)
            if bert is not None:
                bert.close(destroy=True if final else None)
            if final:
                self._destroy_masked_streams()

    def _destroy_masked_streams(self):
        """``close(final=True)``: the step's CU-masked streams (SDNet.trunk_stream_cus) go the way of the encoder's masked stream."""
        from . import hip
        for cache in (self.__dict__.get("_step_streams"), getattr(getattr(self, "network", None), "__dict__", {}).get("_streams")):
            for key, v in list((cache or {}).items()):
                sts = v if isinstance(v, tuple) else (v,)
                if any(getattr(s, "_ruart_masked", False) for s in sts):
                    del cache[key]
                    for s in sts:
                        hip.destroy_stream(s)

    def ToCUDA(self, batch):
        """Models/SDNetTrainer.py:208-230.  Index vectors and the packed BERT stream are prepared here, from the host copies,
        before the tensors move - unless the batch already carries them (``VQA_collate(opt, prepare_index=True)`` builds the
        host part in the DataLoader workers; then this is copies only)."""
        q, ocr, od = batch[0], batch[1], batch[2]
        if hasattr(self, "network"):
            self.network.prepare(q, ocr, od)
        out = to_device(batch, self.device)
        if "_ruart_index" in q:
            out[0]["_ruart_index"] = q["_ruart_index"]
        pack = out[0].pop("_ruart_label_pack", None)
        if pack is not None and out[3] is None:
            # opt['label_from_answers']: the collate packed the strings (batch.VQA_collate); upload, one launch, the label rule in tensors
            from .metrics import labels_from_pack
            out[3] = labels_from_pack(pack, self.opt, self.device)
        return out

    def instance_bce_with_logits(self, logits, labels):
        assert logits.dim() == 2
        loss = nn.functional.binary_cross_entropy_with_logits(logits, labels)
        if self.opt["loss"] == "BCE_D1":
            loss = loss * labels.size(1)
        return loss

    # -- one optimizer step -----------------------------------------------------------------------------------
    def update(self, batch, batch_i=0, next_batch=None, stage_next=None):
        """One optimizer step.  ``stage_next`` (optional callable): run once after the whole step has been enqueued and BEFORE the
        host waits for its loss - the place to fetch the batch after next from the loader and ship it (``ToCUDA``): that costs
        0.5-0.7 ms of host time per step, which delays the next encoder launch by as much when it sits between two ``update`` calls and
        nothing when it sits where the host waits anyway.  Its return value is kept in ``self.staged``.  ``next_batch`` (already through ToCUDA) lets the frozen BERT pass of the following step run
        concurrently with this step's SDNet trunk, on its own stream.  The step runs on a stream of its own too, whose priority ``SDNet.trunk_stream_priority``
        chooses (see there and DESIGN.md section 5)."""
        self.network.train()                      # (the step stream's priority depends on the mode: set it before choosing)
        return self.on_step_stream(self._update, batch, batch_i, next_batch, stage_next)

    def on_step_stream(self, fn, *args):
        """Run ``fn(*args)`` - a training step or an evaluation forward - with the trainer's step stream current, and join it with the
        caller's stream on both sides.  Needed for the encoder pass that runs one batch ahead to overlap anything: its CU-masked stream
        (hipExtStreamCreateWithCUMask takes no flags) is a BLOCKING stream, i.e. every launch on the legacy default stream - torch's
        current stream unless told otherwise - waits for all of the encoder's enqueued work and the two run strictly one after the
        other (forward-only steps: 27 ms = 20 + 7, `tools/step_timeline.py --fwd`).  The step stream is a non-blocking pool stream.
        (A trainable encoder: nothing runs ahead, the caller's stream is used as it is.)"""
        st = self._step_stream()
        if st is None:
            return fn(*args)
        cur = torch.cuda.current_stream(self.device)
        if cur == st:                       # the caller already runs on the step stream (train(), step_stream()): nothing to join
            return fn(*args)
        st.wait_stream(cur)
        with torch.cuda.stream(st):
            out = fn(*args)
        cur.wait_stream(st)
        return out

    def _step_stream(self):
        """The step stream of the network's CURRENT mode (created on first use; one per priority: the process keeps the streams it
        starts with, profiles/HISTORY.md round 5 (6b) / (9)); None on the CPU and with a trainable encoder none of whose layers run ahead."""
        dev = self.device
        bert = getattr(self.network, "Bert", None)
        unlocked = getattr(bert, "bert_model", None) is not None
        if unlocked and bert.runs_ahead():
            unlocked = False                # opt['bert_train_layers']: the frozen lower layers run ahead as the frozen encoder does
        if dev.type != "cuda" or unlocked:
            return None
        pr = self.network.trunk_stream_priority()       # (differs between training and evaluation in the fp16c schedule)
        cache = self.__dict__.setdefault("_step_streams", {})
        st = cache.get(pr)
        if st is None:
            ncu = self.network.trunk_stream_cus()                   # an experiment's CU mask (SDNet.trunk_stream_cus; 0 by default)
            if ncu != 0:
                from . import hip
                st = hip.cu_masked_stream(ncu, dev)
            elif pr > 0:                                        # LOW priority: not in torch's pool
                from . import hip
                st = hip.priority_stream(pr, dev)
            else:
                st = torch.cuda.Stream(device=dev, priority=pr)
            cache[pr] = st
        return st

    def step_stream(self):
        """Context manager: the TRAINING step stream as torch's current stream - for a loop that stages batches and calls ``update``
        many times (``train()`` runs inside it; a script that drives ``update`` itself should too).  Called from torch's default
        stream, every ``update`` has to join that stream with the step stream on both sides, and the default stream is the LEGACY
        stream: each of those two markers waits for - and holds back - the CU-masked encoder stream (a blocking stream), so the
        next step's trunk cannot start before the encoder pass that runs beside it has ended.  With the caller on the step stream
        the first kernels of step t+1 (embeddings, the question branch) run under the tail of that pass: 22.75 -> 22.00 ms per step
        (interleaved, three rounds; profiles/HISTORY.md round 5 (12)).  Everything the loop enqueues - ``ToCUDA`` copies included - is then
        ordered on that one stream; results handed to another stream need the usual ``wait_stream``."""
        import contextlib
        self.network.train()
        st = self._step_stream()
        return torch.cuda.stream(st) if st is not None else contextlib.nullcontext()

    def _global_world(self):
        """World size of the cross-rank layer norms (1 without opt['dp_global_batch'] in effect)."""
        return torch.distributed.get_world_size(self.process_group) if self.global_batch else 1

    def _check_shard(self, ocr_list):
        """opt['dp_global_batch']: the global element count of a layer norm is W times the local one, so every rank's shard must hold
        batch_size samples (what VQA_Sampler deals, evaluation's wrap-around included)."""
        if self._global_world() > 1 and len(ocr_list["num_cnt"]) != self.batch_size:
            raise ValueError("opt['dp_global_batch']: every rank's shard holds batch_size = %d samples, this one %d"
                             % (self.batch_size, len(ocr_list["num_cnt"])))

    def _update(self, batch, batch_i, next_batch, stage_next=None):
        self.network.train()
        self.network.drop_emb = True
        q_list, ocr_list, od_list, targets, extra_info = batch
        self._check_shard(ocr_list)
        if next_batch is not None:
            self.network.prefetch_bert(next_batch[0], next_batch[1], next_batch[2])
        scores, _ = self.network(q_list, ocr_list, od_list)
        if self.opt["loss"] == "CE":
            targets = torch.nonzero(targets)[:, 1]
        loss = self.loss_func(scores, targets)
        self.optimizer.zero_grad(set_to_none=True)
        loss.backward()
        if self.grad_sync is not None:
            self.grad_sync.average_gradients()
        if hasattr(self.optimizer, "clip_and_step"):       # fused: global-norm clip + the conf's update rule in three launches
            self.optimizer.clip_and_step(self.opt["grad_clipping"],
                                         extra_sq=self.grad_sync.pinned_sq if self.grad_sync is not None else None)
        else:
            torch.nn.utils.clip_grad_norm_(self.network.parameters(), self.opt["grad_clipping"])
            self.optimizer.step()
        self.updates += 1
        self.next_batch_i = batch_i + 1
        if "TUNE_PARTIAL" in self.opt:
            # Models/SDNetTrainer.py:369-373 re-pins the rows >= tune_partial after every step.  The fused optimizer never writes them
            # (FusedAdamax(pinned=): their update is left out), so they still hold the pinned values: the two 23 MB copies per step
            # are skipped for the tables it knows as pinned
            tp = self.opt["tune_partial"]
            kept = getattr(self.optimizer, "pinned", {})
            if "FastText" in self.opt and id(self.network.fast_embed.weight) not in kept:
                self.network.fast_embed.weight.data[tp:] = self.network.fixed_embedding_fast
            if "GLOVE" in self.opt and id(self.network.glove_embed.weight) not in kept:
                self.network.glove_embed.weight.data[tp:] = self.network.fixed_embedding_glove
        if self._defer_readback():
            lazy = self._readback_later(loss, stage_next)
            return lazy
        if stage_next is not None:
            self.staged = stage_next()
        self.host_enqueued_at = time.perf_counter()      # (bench.py: how long the host took to enqueue the step)
        # the reference's NaN contract (SDNetTrainer.py:339-359 + the asserts inside forward): one sync, here
        loss_val = loss.item()
        self.network.check_nan()
        assert loss_val == loss_val, "loss nan"
        self.train_loss.update(loss_val, 1)
        return loss_val

    # -- loss / NaN readback one step late (trained encoder) ------------------------------------------------------------
    # With the encoder trained nothing runs ahead of a step: encoder forward -> trunk -> encoder backward is one chain, its two
    # encoder parts bound by the GPU (10 + 21 ms of GEMMs, the host idle) and its trunk part by the host (~15 ms of enqueueing
    # ~850 small launches, the GPU mostly idle).  A ``loss.item()`` at the end of every step welds the two together; reading the
    # loss and the NaN flag of step t at the END of step t+1 instead lets the host enqueue the trunk of step t+1 while the GPU is
    # still in the encoder backward of step t.  The reference's contract is kept one step late: the same asserts fire, before
    # any checkpoint or evaluation can see the weights (``flush_readback`` runs first there), and ``train_loss`` sees every
    # step's value in order.  The frozen-encoder pipeline keeps its per-step sync: there it was measured FASTER.
    # Round 5: since the training loop runs on the step stream (step_stream) the frozen pipeline's trunk chain is as long as its encoder
    # chain, and the host sits on it once per step (loss.item(): 22.28 ms per step against 22.03 deferred, and every host hiccup is a
    # slow step).  ``train()`` therefore defers inside its own loop - it only logs the loss, and flush_readback keeps the asserts ahead
    # of every evaluation and checkpoint; a direct ``update()`` call keeps the reference's contract (a float, asserts in the same
    # step) unless opt['ruart_defer_readback'] says otherwise.
    def _defer_readback(self):
        d = self.opt.get("ruart_defer_readback")
        if d is None:
            d = getattr(getattr(self.network, "Bert", None), "bert_model", None) is not None or getattr(self, "_in_train_loop", False)
        return bool(d) and self.device.type == "cuda"

    def _readback_later(self, loss, stage_next=None):
        from . import ops
        slots = self.__dict__.setdefault("_rb_slots", [torch.empty(2, dtype=torch.float32).pin_memory() for _ in range(2)])
        host = slots[self.updates & 1]
        flag = ops.nan_flag.flag
        host[0:1].copy_(loss.detach().reshape(1), non_blocking=True)
        if flag is not None and flag.device == loss.device:
            host[1:2].copy_(flag, non_blocking=True)        # int32 -> float32: 0 stays 0
            flag.zero_()
        else:
            host[1] = 0.0
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(self.device))
        prev, self._rb_pending = self.__dict__.get("_rb_pending"), {"host": host, "event": ev, "value": None}
        lazy = _PendingLoss(self, self._rb_pending)
        if stage_next is not None:
            self.staged = stage_next()
        self.host_enqueued_at = time.perf_counter()      # (bench.py: how long the host took to enqueue the step)
        if prev is not None:
            self._resolve(prev)
        return lazy

    def _resolve(self, pending):
        if pending["value"] is None:
            pending["event"].synchronize()
            host = pending["host"]              # (reused two steps later: the value is taken out now)
            loss_val, bad = float(host[0]), float(host[1])
            assert bad == 0, "NaN produced inside the SDNet kernels (reference: assert torch.sum(torch.isnan(x)) == 0)"
            assert loss_val == loss_val, "loss nan"
            self.train_loss.update(loss_val, 1)
            pending["value"] = loss_val
        return pending["value"]

    def flush_readback(self):
        """Resolve the step whose loss / NaN flag have not been read back yet (no-op otherwise); returns its loss or None."""
        pending, self._rb_pending = self.__dict__.get("_rb_pending"), None
        return self._resolve(pending) if pending is not None else None

    # -- inference --------------------------------------------------------------------------------------------
    def predict(self, batch, all_ans=False, next_batch=None):
        """Models/SDNetTrainer.py:378-451: arg-max over VALID answer slots, ANLS / ACC when answers are known.
        ``next_batch`` (already through ToCUDA): its frozen-encoder pass is started beside this batch's trunk, as in ``update``."""
        self.network.eval()
        return self.on_step_stream(self._predict, batch, all_ans, next_batch)

    def _predict(self, batch, all_ans=False, next_batch=None):
        self.flush_readback()                  # (a deferred training step's asserts come before anything reads the weights)
        self.network.eval()
        self.network.drop_emb = False
        q_list, ocr_list, od_list, gt_list, extra_info = batch
        self._check_shard(ocr_list)
        if next_batch is not None:
            self.network.prefetch_bert(next_batch[0], next_batch[1], next_batch[2])
        with torch.no_grad():
            scores, _ = self.network(q_list, ocr_list, od_list)
            loss = self.loss_func(scores, gt_list).item() if gt_list is not None else 0
        self.network.check_nan()
        decode = decode_slots if "label_yesno" in self.opt else decode_predictions
        if self.opt.get("eval_upper_bound"):
            # per sample the best credit any admitted slot would have earned; ``_evaluate`` collects them (the return value stays)
            self._bound_rows = []
            ANLS, ACC, res, save_res = decode(scores, ocr_list["num_cnt"], extra_info, self.opt, bound=self._bound_rows)
        else:
            ANLS, ACC, res, save_res = decode(scores, ocr_list["num_cnt"], extra_info, self.opt)
        return loss, ANLS, ACC, res, save_res

    def _is_main(self):
        """Rank 0 (or no process group): the only rank that creates the run folder and writes checkpoints / predictions."""
        d = torch.distributed
        return not (d.is_available() and d.is_initialized()) or d.get_rank(self.process_group) == 0

    def _loader(self, data, sampler, workers=0):
        from torch.utils.data import DataLoader
        collate = VQA_collate(self.opt, prepare_index=workers > 0).VQA_collate_fun
        # pinned batches (tensors and, through BatchIndex.pin_memory, the host-built index): ToCUDA becomes asynchronous copies
        return DataLoader(data, batch_sampler=sampler, collate_fn=collate, num_workers=workers,
                          pin_memory=self.device.type == "cuda")

    def evaluate(self, val_data, batch_i=0, mode="dev"):
        """Models/SDNetTrainer.py:127-176.  ``val_data`` is a ``VQA_Dataset`` (batched here in the reference's deterministic
        order; ``dev`` keeps the best-ANLS / best-ACC checkpoints and ``save_res_last.json``, ``test`` writes
        ``submission.json`` without the wrap-around padding of the last batch) or any iterable of collated batches (metrics
        only).  Returns (mean loss, ANLS, ACC, predictions)."""
        assert mode in ("train", "dev", "test")
        try:
            return self._evaluate(val_data, batch_i, mode)
        finally:
            if not getattr(self, "_in_train", False):     # stand-alone evaluation: nothing else will release the stream
                self.close()
            elif self.device.type == "cuda" and self.opt.get("ruart_empty_cache_after_eval", True):
                # an evaluation inside train(): its no-grad forwards leave the caching allocator with a block layout the training steps
                # would go on reusing - measured 0.7-1.0 ms per training step under the schedule of the time (bench.py's parity check,
                # profiles/HISTORY.md round 5 (11); under the final schedule of (12) the effect was no longer measurable); handing the cached
                # blocks back costs a few re-allocations in the next step
                torch.cuda.synchronize(self.device)
                torch.cuda.empty_cache()

    def _evaluate(self, val_data, batch_i, mode):
        from torch.utils.data import Dataset
        is_dataset = isinstance(val_data, Dataset)
        # opt['dp_global_batch'] over W > 1 ranks: the reference's evaluation stream in global batches of W * batch_size, rank r
        # predicting global[r::W]; the results are gathered back into the single process's order (sampler.merge_rank_shards)
        world = self._global_world() if is_dataset else 1
        rank = torch.distributed.get_rank(self.process_group) if world > 1 else 0
        loader = self._loader(val_data, VQA_Sampler(val_data, self.opt["max_batch_num"], self.batch_size, False, rank=rank,
                                                    world_size=world)) if is_dataset else val_data
        loss = ANLS = ACC = n = nb = 0
        res, save_res = [], []
        want_bound = bool(self.opt.get("eval_upper_bound"))
        b_anls = b_acc = 0
        self.__dict__.pop("eval_bound", None)
        it = iter(loader)
        nxt = next(it, None)
        nxt = self.ToCUDA(nxt) if nxt is not None else None
        while nxt is not None:
            batch = nxt
            nxt = next(it, None)
            nxt = self.ToCUDA(nxt) if nxt is not None else None       # lookahead: the next batch's encoder pass runs beside this trunk
            l, a, c, r, sr = self.predict(batch, next_batch=nxt)
            loss, ANLS, ACC, n, nb = loss + l, ANLS + a, ACC + c, n + len(r), nb + 1
            if want_bound:
                for row in self._bound_rows:              # in sample order, as the ANLS / ACC sums are formed
                    if row is not None:
                        b_anls, b_acc = b_anls + row[0], b_acc + row[1]
            res.extend(r)
            save_res.extend(sr)
        if world > 1:
            # every rank ends with the same global sums and lists (added in rank order), so no rank's control flow can diverge
            parts = [None] * world
            torch.distributed.all_gather_object(parts, (loss, ANLS, ACC, res, save_res), group=self.process_group)
            loss, ANLS, ACC = (sum(p[k] for p in parts) for k in range(3))
            loss = loss / world                         # the loss of a global batch is the mean of its W equal shards' losses
            res = merge_rank_shards([p[3] for p in parts], self.batch_size)
            save_res = merge_rank_shards([p[4] for p in parts], self.batch_size)
            if want_bound:
                parts = [None] * world
                torch.distributed.all_gather_object(parts, (b_anls, b_acc), group=self.process_group)
                b_anls, b_acc = sum(p[0] for p in parts), sum(p[1] for p in parts)
        n_items = len(val_data) if is_dataset else n
        loss, ANLS, ACC = loss / max(nb, 1), ANLS / max(n_items, 1), ACC / max(n_items, 1)
        if want_bound:
            # opt['eval_upper_bound']: what a perfect scorer could reach over the slots the decode admits - the OCR upper bound
            self.eval_bound = {"ANLS": b_anls / max(n_items, 1), "ACC": b_acc / max(n_items, 1)}
            log.info("Dataset: %s Batch: %7d OCR upper bound ANLS: %.3f ACC: %.3f", mode, batch_i, self.eval_bound["ANLS"],
                     self.eval_bound["ACC"])
        if not is_dataset or not self._is_main():
            return loss, ANLS, ACC, res
        if mode == "test":
            gb = self.batch_size * world
            end = len(val_data) % gb
            if end != 0:
                res = res[:-(gb - end)]
            path = os.path.join(self.saveFolder, "submission.json")
            with open(path, "w") as wf:
                json.dump(res, wf, indent=2)
            log.info("%d test samples are predicted, %d predictions saved in %s", len(val_data), len(res), path)
            return loss, ANLS, ACC, res
        if mode == "dev":
            with open(os.path.join(self.saveFolder, "save_res_last.json"), "w") as wf:
                json.dump(save_res, wf, indent=2)
            if ANLS > self.best_ANLS:
                self.best_ANLS, self.best_ANLS_batch = ANLS, batch_i
                self.save_for_predict(os.path.join(self.saveFolder, "ANLS_best_model.pt"))
            if ACC > self.best_ACC:
                self.best_ACC, self.best_ACC_batch = ACC, batch_i
                self.save_for_predict(os.path.join(self.saveFolder, "ACC_best_model.pt"))
        log.info("Dataset: %s Batch: %7d ANLS: %.3f Best ANLS: %.3f Batch: %d ACC: %.3f Best ACC:%.3f Batch:%d", mode, batch_i, ANLS,
                 self.best_ANLS, self.best_ANLS_batch, ACC, self.best_ACC, self.best_ACC_batch)
        return loss, ANLS, ACC, res

    def _setup_from_meta(self):
        from .dataset import load_meta
        self.vocab, self.char_vocab, vocab_embedding = load_meta(self.opt)
        self.setup_model(vocab_embedding)

    def _records(self, split):
        from .dataset import load_msgpack
        return load_msgpack(os.path.join(self.opt["FEATURE_FOLDER"], split + "-preprocessed.msgpack"))["data"]

    def train(self, train_loader=None, val_loader=None, eval_every=1500, log_every=30):
        """The outer loop of Models/SDNetTrainer.py:50-123.  Without arguments it is the reference's ``train()``: run folder,
        model from ``train_meta.msgpack`` (+ ``RESUME``), ``VQA_Dataset`` over the train / val msgpack records, the deterministic
        ``VQA_Sampler`` stream, evaluation every ``eval_every`` batches and once more on both sets at the end.  With a loader it
        runs over any iterable of collated batches.  Either way the next batch is staged one step ahead so that its frozen-BERT
        pass overlaps this step's trunk."""
        self.isTrain = True
        self._in_train = True
        try:
            self._train(train_loader, val_loader, eval_every, log_every)
        finally:
            self._in_train = False
            self._in_train_loop = False
            if self.__dict__.pop("_gc_frozen", False):
                import gc
                gc.unfreeze()                # the permanent generation of _train is handed back: train() leaves the interpreter as it found it
            self.close()

    def _train(self, train_loader, val_loader, eval_every, log_every):
        train_data = None
        batch_st = 0
        # opt['save_every'] = N: the run state (save) after every N-th update; opt['resume_state'] = path: continue the run that file
        # was written by.  Both absent by default: the loop below is then the loop it always was.
        save_every = int(self.opt.get("save_every") or 0)
        resume = self.opt.get("resume_state")
        state = None
        if save_every < 0:
            raise ValueError("opt['save_every'] = %r: a positive number of updates" % (self.opt.get("save_every"),))
        if save_every or resume:
            self._refuse_state_conf("opt['save_every'] / opt['resume_state']")
        if resume:
            from . import train_state as TS
            state = TS.read(resume)
            batch_st = int(state["ruart"]["next_batch"])
            if "batch_st" in self.opt and int(self.opt["batch_st"]) != batch_st:
                raise ValueError("opt['batch_st'] = %r, the run state %s continues at batch %d" % (self.opt["batch_st"], resume, batch_st))
            # the run goes on where it was: no new run_<n>, conf_copy left alone
            self.saveFolder = os.path.dirname(os.path.abspath(resume))
        if train_loader is None:
            from .dataset import VQA_Dataset
            if self._is_main() and not resume:
                self.getSaveFolder()
                self.saveConf()
            self._setup_from_meta()
            if "RESUME" in self.opt:
                self.load_model(os.path.join(self.opt["datadir"], self.opt["MODEL_PATH"]))
            if not resume:
                batch_st = self.opt.get("batch_st", 0)
            train_data = VQA_Dataset(self._records("train"), self.opt, image_features=self.img_features)
            dist = torch.distributed
            rank, world = (dist.get_rank(self.process_group), dist.get_world_size(self.process_group)) \
                if dist.is_available() and dist.is_initialized() else (0, 1)
            sampler = VQA_Sampler(train_data, self.opt["max_batch_num"], self.batch_size, True, batch_st=batch_st,
                                  epoch=self.opt.get("epoch"), rank=rank, world_size=world)
            train_loader = self._loader(train_data, sampler, workers=self.opt.get("num_worker", 0))
            val_loader = VQA_Dataset(self._records("val"), self.opt, image_features=self.img_features)
        it = iter(train_loader)
        # Everything alive at this point - the model, the optimizer state, the dataset records with the reference's nested python lists -
        # stays alive for the whole run: move it out of the garbage collector's sight (a permanent generation), or every full collection
        # walks all of it and stops the host for ~45 ms, i.e. one 70 ms step in ~25 (measured).  The
        # collector keeps running over what the steps themselves create.  opt['ruart_gc_freeze'] = False leaves the interpreter alone.
        if self.opt.get("ruart_gc_freeze", True):
            import gc
            gc.collect()
            gc.freeze()
            self._gc_frozen = True           # (train()'s finally unfreezes)

        def stage():                                                  # the next batch of the loader, shipped to the device (or None)
            b = next(it, None)
            return self.ToCUDA(b) if b is not None else None

        # the whole loop - staging copies, steps, the evaluations in between - with the training step stream current: no step has to be
        # joined with torch's (legacy) default stream, whose markers would hold the next step back until the encoder pass beside it
        # has ended (step_stream)
        with self.step_stream():
            self._in_train_loop = True                                    # (the loss of a step is read back one step late: _defer_readback)
            batch, nxt = stage(), None
            if batch is not None:
                nxt = stage()                                             # one batch of lookahead feeds the BERT prefetch
            if state is not None:
                # applied HERE: the loader's iterator drew its seed from torch's CPU generator and the sampler reseeded numpy on its
                # way to the two staged batches - in the uninterrupted run both lay before the save, so the streams go in after them
                self._apply_state(state)
                state = None
            batch_i = batch_st
            while batch is not None:
                if val_loader is not None and batch_i % eval_every == 0:
                    self.evaluate(val_loader, batch_i)
                # the batch after next is fetched and shipped inside update(), where the host waits for the step anyway
                loss = self.update(batch, batch_i, next_batch=nxt, stage_next=stage if nxt is not None else None)
                batch, nxt = nxt, (self.staged if nxt is not None else None)
                self.staged = None
                if batch_i % log_every == 0:
                    # (a deferred loss is resolved by float(): the running average beside it then includes this step, as in the reference)
                    cur = float(loss)
                    log.info("updates[%6d] train loss[%8.5f / %8.5f]", self.updates, self.train_loss.avg, cur)
                batch_i += 1
                if save_every and batch_i % save_every == 0:
                    # before the evaluation batch_i may start with: the resumed run repeats it, as this run goes on to do
                    epoch = batch_i * self.batch_size * self._state_ranks()[1] // max(len(train_data), 1) if train_data is not None else None
                    self.save(os.path.join(self.saveFolder, "train_state.pt"), epoch=epoch)
            self._in_train_loop = False
            self.flush_readback()                            # the last step's loss and asserts
            if train_data is not None:                       # :121-122
                self.evaluate(val_loader, batch_i - 1)
                self.evaluate(train_data, batch_i - 1, mode="train")
                log.info("Training over")

    def predict_for_test(self):
        """Models/SDNetTrainer.py:231-251: load the model named by ``MODEL_PATH``, predict the test records, write
        ``submission.json`` next to it."""
        from .dataset import VQA_Dataset
        assert "RESUME" in self.opt
        self.isTrain = False
        self.getSaveFolder()
        self._setup_from_meta()
        self.load_model(os.path.join(self.opt["datadir"], self.opt["MODEL_PATH"]))
        test_data = VQA_Dataset(self._records("test"), self.opt, mode="test", image_features=self.img_features)
        return self.evaluate(test_data, 0, "test")          # a stand-alone evaluate(): closes the run-ahead stream on exit

    # -- checkpoints ------------------------------------------------------------------------------------------
    def load_model(self, model_path):
        """:453-466 - tolerant load: unknown keys dropped, missing keys keep their current value."""
        ckpt = torch.load(model_path, map_location="cpu")
        state = ckpt["state_dict"]["network"]
        cur = self.network.state_dict()
        state = {k: v for k, v in state.items() if k in cur}
        for k, v in cur.items():
            state.setdefault(k, v)
        self.network.load_state_dict(state)

    def _predict_state(self):
        """name -> tensor of what ``save_for_predict`` writes (live tensors, nothing copied)."""
        full = self.network.state_dict()
        # (of the encoder, only tensors its passes use: the checkpoint's pooler head is a parameter too and never gets a gradient)
        used = set("Bert.bert_model." + n for n in getattr(getattr(getattr(self.network, "Bert", None), "bert_model", None), "_order", ()))
        trained = [n for n, p in self.network.named_parameters() if p.requires_grad and (not n.startswith("Bert.bert_model.") or n in used)]
        return {k: full[k] for k in predict_checkpoint_keys(full, self.opt, trained)}

    def save_for_predict(self, filename):
        """:492-509 - network weights without BERT / fixed embeddings, plus the config."""
        self.flush_readback()
        state = self._predict_state()
        cfg = {k: v for k, v in self.opt.items() if isinstance(v, (int, float, str, bool))}
        try:
            torch.save({"state_dict": {"network": state}, "config": cfg}, filename)
        except BaseException:
            log.info("[ WARN: Saving failed... continuing anyway. ]")

    # -- run state: resume a run exactly (train_state.py) --------------------------------------------------------------
    def _refuse_state_conf(self, what):
        """Confs whose resumed run was never established to be the uninterrupted run are refused, not served inexactly."""
        if self.opt.get("ruart_graph_trunk", False):
            raise ValueError("%s does not combine with opt['ruart_graph_trunk']: the captured trunk draws its dropout masks inside a "
                             "replayed graph, and an exact resume was never established there" % what)

    def _state_ranks(self):
        """(rank, world) of the run state: the data-parallel group's when this trainer exchanges gradients, else (0, 1)."""
        if self.grad_sync is None:
            return 0, 1
        return torch.distributed.get_rank(self.process_group), torch.distributed.get_world_size(self.process_group)

    def _banks(self):
        """The two mask banks a step draws from: the module-level one (embedding and multi2one masks) and the trunk's own."""
        return {"front": L.mask_bank, "trunk": self.network._trunk_module()._bank}

    def _trainable_names(self):
        return [n for n, p in self.network.named_parameters() if p.requires_grad]

    def _pack_state(self, epoch, ranks):
        from . import train_state as TS
        full = self.network.state_dict()
        state = self._predict_state()
        trainable = self._trainable_names()
        for n in trainable:                  # a trained encoder's tensors included; a frozen encoder comes from BERT_model_file again
            state.setdefault(n, full[n])
        best = {"ANLS": self.best_ANLS, "ACC": self.best_ACC, "ANLS_batch": self.best_ANLS_batch, "ACC_batch": self.best_ACC_batch}
        return TS.pack(state, self.optimizer, self.updates, self.train_loss, self.opt, epoch=epoch, trainable=trainable,
                       next_batch=self.next_batch_i, best=best, ranks=ranks, extra={"rank_seeded": bool(self._rank_seeded)})

    def save(self, filename, epoch=None, prev_filename=None):
        """Models/SDNetTrainer.py:468-490, extended to the whole run state (train_state.py): network (what ``save_for_predict`` writes
        plus every trained tensor), optimizer, ``updates``, ``train_loss``, ``epoch`` - and the best-model records, the index of the
        next batch, every rank's random streams and mask banks.  ``load_model`` reads the file as a weights-only checkpoint,
        ``load_state`` continues the run bit for bit.  With data parallelism a COLLECTIVE call: every rank contributes its streams and
        banks, rank 0 writes.  The file appears under its name whole or not at all (temporary name + rename); a failed write is
        logged and training goes on, as in ``save_for_predict``."""
        from . import train_state as TS
        self._refuse_state_conf("SDNetTrainer.save")
        self.flush_readback()                  # the deferred asserts come before any weight is written
        rank, world = self._state_ranks()
        ranks = TS.gather_ranks(TS.capture_rank(self.device, self._banks()), world, self.process_group)
        if rank != 0:
            return
        # read on the step stream: ordered behind the optimizer's raw-pointer writes without a device-wide synchronise
        ckpt = self.on_step_stream(self._pack_state, epoch, ranks)
        try:
            TS.write(ckpt, filename)
            log.info("run state saved to %s", filename)
            if prev_filename and os.path.abspath(prev_filename) != os.path.abspath(filename) and os.path.exists(prev_filename):
                os.remove(prev_filename)
        except Exception:
            log.info("[ WARN: Saving failed... continuing anyway. ]")

    def load_state(self, filename):
        """Continue the run ``save`` wrote: returns the index of the next batch.  After ``setup_model`` (and after ``load_model``, if
        both are wanted).  Everything is copied in place - the fused optimizers' pointer tables stay valid - and each data-parallel
        rank takes its own random streams and mask banks.  ValueError, naming the mismatch, for a state that does not fit this run:
        optimizer class or rule, a missing or mis-shaped trainable tensor, the world size, the format version."""
        from . import train_state as TS
        if not hasattr(self, "network"):
            raise RuntimeError("load_state needs setup_model() done")
        self._refuse_state_conf("SDNetTrainer.load_state")
        return self._apply_state(TS.read(filename))

    def _apply_state(self, ckpt):
        from . import train_state as TS
        rank, world = self._state_ranks()
        named = dict(self.network.named_buffers())
        named.update(self.network.named_parameters())
        TS.check(ckpt, self.optimizer, named, self._trainable_names(), world)
        self.flush_readback()

        def copy_in():
            TS.restore_tensors(ckpt, named)
            self.optimizer.load_state_dict(ckpt["state_dict"]["optimizer"])

        self.on_step_stream(copy_in)
        ruart = ckpt["ruart"]
        self.updates = int(ckpt["state_dict"]["updates"])
        TS.restore_meter(self.train_loss, ckpt["train_loss"])
        b = ruart["best"]
        self.best_ANLS, self.best_ACC, self.best_ANLS_batch, self.best_ACC_batch = b["ANLS"], b["ACC"], b["ANLS_batch"], b["ACC_batch"]
        self._rank_seeded = bool(ruart.get("rank_seeded", self._rank_seeded))
        self.next_batch_i = int(ruart["next_batch"])
        TS.restore_rank(ruart["ranks"][rank], self.device, self._banks())       # last: nothing above may draw from a stream
        return self.next_batch_i
