"""``FusedAdamax`` - torch.optim.Adamax + torch.nn.utils.clip_grad_norm_ of the training step (Models/SDNetTrainer.py:307-317,
366-367) as three HIP launches over all trainable tensors (csrc/sdnet_optim.hip) instead of ~20 multi-tensor launches.

Same update rule, same defaults (betas 0.9 / 0.999, eps 1e-8, no weight decay), same ``param_groups`` / ``zero_grad`` /
``state_dict`` surface, so it stands in for the ``'#'`` optimizer of the shipped configuration.  Extra: ``pinned`` maps an
embedding Parameter to the number of leading rows that are really trained; the remaining rows - which the trainer overwrites with
their fixed values after every step (:369-373) - are left out of the update (their gradients still enter the clipping norm,
exactly as in the reference).

The reference's other three ``optimizer`` values step the same way, from one shared base (``_FusedGroup``): ``FusedAdamax(weight_decay=0.5)``
is 'ADAM' (Adamax with coupled L2 decay, ``ruart_adamax_l2_step``), ``FusedAdam`` is 'ADAM2' (torch.optim.Adam, ``ruart_adam_step``),
``FusedSGD`` is 'SGD' (``ruart_sgd_step``).  ``select_optimizer`` names the class the trainer builds for a conf.

``FusedAdamaxAdam`` / ``AdamaxAdam`` (further down): the same step with a trained encoder as an Adam-family group of its own -
opt['bert_optimizer']."""
import copy

import numpy as np
import torch

from . import hip

_CHUNK = 8192


class _FusedGroup:
    """What the fused optimizers over ONE parameter group share - everything but the update rule: the chunk plan, the two staging
    buffers, the per-step table of gradient pointers and coefficients, ``pinned``, ``extra_sq``, ``norm_coef``, the torch.optim surface
    and the version bumps.  A rule names its state tensors (``_STATE``, in the order of its kernel's tables), the number of fp32
    coefficients it sends per tensor and step (``_NCOEF``), and supplies ``_coefficients`` and ``_launch``."""
    _STATE = ()
    _NCOEF = 0

    def __init__(self, params, group, pinned=None):
        self.params = [p for p in params]
        for p in self.params:
            if not (p.is_cuda and p.dtype == torch.float32 and p.is_contiguous()):
                raise ValueError("%s: contiguous fp32 device parameters only" % type(self).__name__)
        self.param_groups = [dict({"params": self.params}, **group)]
        self.pinned = {id(p): int(n) for p, n in (pinned or {}).items()}
        self.state = {id(p): {k: torch.zeros_like(p) for k in self._STATE} for p in self.params}
        self.step_count = 0
        self.steps = {id(p): 0 for p in self.params}      # torch.optim counts every parameter's own steps
        self._plan_key = None
        self.norm_coef = None             # device tensor [total_norm, clip_coef] of the last clip_and_step

    # -- torch.optim surface --------------------------------------------------------------------------------------
    def zero_grad(self, set_to_none=True):
        for p in self.params:
            if p.grad is not None:
                if set_to_none:
                    p.grad = None
                else:
                    p.grad.zero_()

    def state_dict(self):
        return {"step": self.step_count, "steps": [self.steps[id(p)] for p in self.params], "param_groups": [{k: v for k, v in g.items() if k != "params"} for g in self.param_groups],
                "state": [{k: v.clone() for k, v in self.state[id(p)].items()} for p in self.params]}

    def load_state_dict(self, sd):
        self.step_count = int(sd["step"])
        for p, n in zip(self.params, sd.get("steps", [self.step_count] * len(self.params))):
            self.steps[id(p)] = int(n)
        for g, s in zip(self.param_groups, sd["param_groups"]):
            g.update(s)
        for p, st in zip(self.params, sd["state"]):
            for k in self._STATE:
                self.state[id(p)][k].copy_(st[k])

    # -- the step -----------------------------------------------------------------------------------------------------
    def _plan(self, live):
        """Chunk lists (norm: every element with a gradient; update: without the re-pinned rows) and the static pointer tables."""
        dev = live[0].device
        tn, sn, cn, tu, su, cu = [], [], [], [], [], []
        for t, p in enumerate(live):
            n = p.numel()
            n_upd = n
            if id(p) in self.pinned:
                n_upd = min(n, self.pinned[id(p)] * (n // p.shape[0]))
            for s in range(0, n, _CHUNK):
                tn.append(t); sn.append(s); cn.append(min(_CHUNK, n - s))
            for s in range(0, n_upd, _CHUNK):
                tu.append(t); su.append(s); cu.append(min(_CHUNK, n_upd - s))
        ints = torch.tensor(np.concatenate([tn, sn, cn, tu, su, cu]).astype(np.int32), device=dev)
        a, b = len(tn), len(tu)
        ptrs = torch.tensor([[p.data_ptr() for p in live]] + [[self.state[id(p)][k].data_ptr() for p in live] for k in self._STATE],
                            dtype=torch.int64, device=dev)
        n_slots = len(live) + (self._NCOEF * len(live) + 1) // 2
        self._plan_val = {"norm": (ints[0:a], ints[a:2 * a], ints[2 * a:3 * a], a),
                          "upd": (ints[3 * a:3 * a + b], ints[3 * a + b:3 * a + 2 * b], ints[3 * a + 2 * b:], b),
                          "ints": ints, "ptrs": ptrs, "partial": torch.empty(a, dtype=torch.float32, device=dev),
                          # gradient tensors are new every step: their pointer table is re-sent (two pinned staging buffers in
                          # turn, so the one of the previous step may still be in flight)
                          # per step and tensor: gradient pointer (int64), behind them the rule's fp32 coefficients (_NCOEF per tensor,
                          # two to an int64 slot)
                          "gptr_host": [torch.empty(n_slots, dtype=torch.int64).pin_memory() for _ in range(2)],
                          "gptr": torch.empty(n_slots, dtype=torch.int64, device=dev)}
        self._plan_val["gptr_np"] = [h.numpy() for h in self._plan_val["gptr_host"]]
        self.norm_coef = torch.zeros(2, dtype=torch.float32, device=dev)

    def clip_and_step(self, max_norm=None, extra_sq=None):
        """clip_grad_norm_(params, max_norm) (skipped when None) followed by step().  The total norm and the clip coefficient
        stay on the device in ``self.norm_coef``.  ``extra_sq`` (device float tensor): the norm runs over the UPDATED elements only
        (the re-pinned embedding rows left out) and this squared norm is added in their place - dp.GradSync.pinned_sq."""
        live = [p for p in self.params if p.grad is not None]
        if not live:
            return
        key = tuple(id(p) for p in live)
        if key != self._plan_key:
            self._plan(live)
            self._plan_key = key
        pl = self._plan_val
        slot = self.step_count & 1
        tab = pl["gptr_np"][slot]
        g0 = self.param_groups[0]
        n_live = len(live)
        nc = self._NCOEF
        tab_f = tab[n_live:].view(np.float32) if nc else None      # the rule's coefficients, nc fp32 per tensor
        for i, p in enumerate(live):
            g = p.grad
            if not (g.is_contiguous() and g.dtype == torch.float32):
                g = p.grad = g.contiguous().float()
            tab[i] = g.data_ptr()
            self.steps[id(p)] += 1
            if nc:
                j = nc * i
                for c in self._coefficients(g0, self.steps[id(p)]):
                    tab_f[j] = c
                    j += 1
        pl["gptr"].copy_(pl["gptr_host"][slot], non_blocking=True)
        tab_dev = pl["gptr"][n_live:].view(torch.float32) if nc else None
        lib = hip.kernels()
        st = hip.stream_ptr()
        self.step_count += 1
        coef = None
        if max_norm is not None:
            ct, cs, cc, n = pl["norm"] if extra_sq is None else pl["upd"]
            lib.ruart_grad_norm_clip(pl["gptr"], ct, cs, cc, n, float(max_norm), pl["partial"], self.norm_coef, extra_sq, st)
            coef = self.norm_coef
        self._launch(lib, g0, pl["ptrs"], pl["gptr"], pl["upd"], coef, tab_dev, st)
        # the kernel wrote the parameters through raw pointers: tell torch (version counters feed autograd's saved-tensor checks and
        # the trainable encoder's operand cache, bert_train16.accurate_weights)
        bump = getattr(torch.autograd.graph, "increment_version", None)
        if bump is None:
            raise RuntimeError("torch.autograd.graph.increment_version is missing: caches keyed on parameter versions "
                               "(bert_train16.accurate_weights) would go stale after this step")
        for p in live:
            bump(p)

    def step(self):
        self.clip_and_step(None)


class FusedAdamax(_FusedGroup):
    """torch.optim.Adamax, the '#' optimizer; with ``weight_decay`` > 0 the coupled L2 form of the 'ADAM' conf
    (torch.optim.Adamax(weight_decay=) behind clip_grad_norm_: the decay enters the gradient after the clip).  Without decay the
    launch is ``ruart_adamax_step``, unchanged."""
    _STATE = ("exp_avg", "exp_inf")
    _NCOEF = 1

    def __init__(self, params, lr=2e-3, betas=(0.9, 0.999), eps=1e-8, pinned=None, weight_decay=0):
        if weight_decay < 0:
            raise ValueError("FusedAdamax: weight_decay %r is negative" % (weight_decay,))
        super().__init__(params, {"lr": lr, "betas": betas, "eps": eps, "weight_decay": weight_decay}, pinned)

    @staticmethod
    def _coefficients(g0, k):
        return (g0["lr"] / (1.0 - g0["betas"][0] ** k),)      # lr / (1 - beta1^step)

    @staticmethod
    def _launch(lib, g0, ptrs, gptr, upd, coef, tab, st):
        ct, cs, cc, n = upd
        b1, b2, eps, wd = float(g0["betas"][0]), float(g0["betas"][1]), float(g0["eps"]), float(g0["weight_decay"])
        if wd == 0.0:
            lib.ruart_adamax_step(ptrs[0], gptr, ptrs[1], ptrs[2], ct, cs, cc, n, coef, tab, b1, b2, eps, st)
        else:
            lib.ruart_adamax_l2_step(ptrs[0], gptr, ptrs[1], ptrs[2], ct, cs, cc, n, coef, tab, b1, b2, eps, wd, st)


class FusedAdam(_FusedGroup):
    """torch.optim.Adam without weight decay (the 'ADAM2' conf) on ``ruart_adam_step``: per step and tensor the host sends
    {a = lr / (1 - beta1^k), dec = 1, c = 1 / sqrt(1 - beta2^k)}, k the tensor's own step count."""
    _STATE = ("exp_avg", "exp_avg_sq")
    _NCOEF = 3

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, pinned=None):
        super().__init__(params, {"lr": lr, "betas": betas, "eps": eps, "weight_decay": 0}, pinned)

    @staticmethod
    def _coefficients(g0, k):
        return adam_coefficients("adamw", g0["lr"], 0.0, g0["betas"], k)

    @staticmethod
    def _launch(lib, g0, ptrs, gptr, upd, coef, tab, st):
        ct, cs, cc, n = upd
        lib.ruart_adam_step(ptrs[0], gptr, ptrs[1], ptrs[2], ct, cs, cc, n, coef, tab, float(g0["betas"][0]), float(g0["betas"][1]),
                            float(g0["eps"]), st)


class FusedSGD(_FusedGroup):
    """torch.optim.SGD without momentum or decay (the 'SGD' conf) on ``ruart_sgd_step``; no state tensors."""

    def __init__(self, params, lr, pinned=None):
        super().__init__(params, {"lr": lr, "weight_decay": 0}, pinned)

    @staticmethod
    def _launch(lib, g0, ptrs, gptr, upd, coef, tab, st):
        ct, cs, cc, n = upd
        lib.ruart_sgd_step(ptrs[0], gptr, ct, cs, cc, n, coef, float(g0["lr"]), st)


_TORCH_NAME = {"#": "Adamax", "ADAM": "Adamax", "ADAM2": "Adam", "SGD": "SGD"}
_FUSED_NAME = {"#": "FusedAdamax", "ADAM": "FusedAdamax", "ADAM2": "FusedAdam", "SGD": "FusedSGD"}


def select_optimizer(opt, device_type):
    """Name of the class ``SDNetTrainer.setup_model`` builds for ``opt['optimizer']`` on a device of ``device_type``.  The fused
    classes need a CUDA device.  '#' takes them unless opt['ruart_fused_optimizer'] is false (and, with opt['bert_optimizer'], the
    two-group forms); 'ADAM', 'ADAM2' and 'SGD' take them only when the key is PRESENT and true - without it they stay on torch.optim."""
    o = opt["optimizer"]
    if o not in _TORCH_NAME:
        raise ValueError("optimizer is wrong")
    fused = device_type == "cuda" and bool(opt.get("ruart_fused_optimizer", o == "#"))
    if o == "#" and "bert_optimizer" in opt:
        return "FusedAdamaxAdam" if fused else "AdamaxAdam"
    return (_FUSED_NAME if fused else _TORCH_NAME)[o]


# -- the trained encoder as a parameter group of its own (opt['bert_optimizer']) ------------------------------------------------
# Fine-tuning an encoder wants an Adam-family rule with a small learning rate of its own, warm-up and linear decay, and decoupled weight
# decay that skips biases and LayerNorm parameters; the trunk keeps Adamax.  ``FusedAdamaxAdam`` steps both groups under ONE global clip
# norm in four launches (norm partials, norm, Adamax over the trunk, Adam over the encoder); ``AdamaxAdam`` is the same thing in plain
# torch ops on any device - what opt['ruart_fused_optimizer'] = False selects, and what the fused form is tested against.
#
# Two rules, one update form (csrc/sdnet_optim.hip, adam_update_kernel):  m = b1 m + (1 - b1) g;  v = b2 v + (1 - b2) g^2;
# p = p dec - a m / (sqrt(v) c + eps).
#   'adamw'     torch.optim.AdamW:  a = lr_t / (1 - b1^k), c = 1 / sqrt(1 - b2^k), dec = 1 - lr_t wd; k = the tensor's own step count,
#               this step included
#   'bertadam'  the reference's BertAdam (Models/Bert/optimization.py:129-152), which has no bias correction:  a = lr_t, c = 1,
#               dec = 1 - lr_t wd.  Its per-parameter ``max_grad_norm`` clipping is NOT built: the trainer's global clip runs already.
# lr_t = lr * multiplier(k - 1, warmup, t_total): the schedule reads the steps the tensor has COMPLETED, so the first step of a
# warmed-up run has lr_t = 0, as in the reference (:145-154).
RULES = ("adamw", "bertadam")
ENCODER_PREFIX = "Bert.bert_model."
_NO_DECAY = (".bias", "LayerNorm.gamma", "LayerNorm.beta", "LayerNorm.weight", "LayerNorm.bias")


def multiplier(k, warmup, t_total):
    """Learning-rate multiplier after ``k`` completed steps: linear warm-up over the first ``warmup`` portion of ``t_total`` steps,
    then linear decay 1 - k / t_total (the reference's ``warmup_linear``, Models/Bert/optimization.py:32-35); constant 1 when
    ``t_total`` is -1.  Deliberate departure: the reference's multiplier goes NEGATIVE past ``t_total`` (gradient ascent); here it is
    clamped at 0."""
    if t_total == -1:
        return 1.0
    x = k / t_total
    if x < warmup:
        return x / warmup
    return max(0.0, 1.0 - x)


def adam_coefficients(rule, lr, weight_decay, betas, k, warmup=-1, t_total=-1):
    """(a, dec, c) of the update form above for a tensor taking its ``k``-th step (k >= 1)."""
    lr_t = lr * multiplier(k - 1, warmup, t_total)
    dec = 1.0 - lr_t * weight_decay
    if rule == "adamw":
        return lr_t / (1.0 - betas[0] ** k), dec, 1.0 / (1.0 - betas[1] ** k) ** 0.5
    if rule == "bertadam":
        return lr_t, dec, 1.0
    raise ValueError("opt['bert_optimizer'] = %r: the encoder group's rule is one of %s" % (rule, ", ".join(RULES)))


def group_of(name):
    """Group of a TRAINABLE tensor by its name in ``SDNet.named_parameters()``: 'trunk' (Adamax: everything outside the encoder, the
    linear-combine weights and the embedding tables included), 'decay' or 'no_decay' (the encoder's Adam group; biases and LayerNorm
    parameters take no weight decay)."""
    if not name.startswith(ENCODER_PREFIX):
        return "trunk"
    return "no_decay" if name.endswith(_NO_DECAY) else "decay"


def split_parameters(named_parameters):
    """(trunk, encoder, no_decay) - lists of the parameters with ``requires_grad`` in the order given, ``no_decay`` a subset of
    ``encoder``.  Frozen tensors (opt['bert_train_layers']) are in no group."""
    trunk, encoder, no_decay = [], [], []
    for name, p in named_parameters:
        if not p.requires_grad:
            continue
        g = group_of(name)
        if g == "trunk":
            trunk.append(p)
        else:
            encoder.append(p)
            if g == "no_decay":
                no_decay.append(p)
    return trunk, encoder, no_decay


def check_bert_optimizer(opt):
    """The conf keys of the encoder group; raises ValueError for a conf that cannot have one.  Returns None without
    opt['bert_optimizer'], else the keyword arguments of ``FusedAdamaxAdam`` / ``AdamaxAdam``."""
    if "bert_optimizer" not in opt:
        return None
    rule = opt["bert_optimizer"]
    if rule not in RULES:
        raise ValueError("opt['bert_optimizer'] = %r: the encoder group's rule is one of %s" % (rule, ", ".join(RULES)))
    if "LOCK_BERT" in opt:
        raise ValueError("opt['bert_optimizer'] steps a trained encoder, LOCK_BERT freezes it: a conf has one or the other")
    if opt.get("optimizer") != "#":
        raise ValueError("opt['bert_optimizer'] adds a group to the '#' optimizer (Adamax trunk), not to optimizer = %r" % (opt.get("optimizer"),))
    warmup = opt.get("bert_warmup", -1)
    if not (warmup == -1 or 0.0 <= warmup < 1.0):
        raise ValueError("opt['bert_warmup'] = %r: a portion of bert_t_total in [0, 1), or -1 for none" % (warmup,))
    return {"rule": rule, "bert_lr": float(opt.get("bert_lr", 5e-5)), "weight_decay": float(opt.get("bert_weight_decay", 0.01)),
            "warmup": warmup, "t_total": int(opt.get("bert_t_total", -1)), "adam_eps": float(opt.get("bert_adam_eps", 1e-6))}


class _TwoGroups:
    """What the fused and the unfused form share: the two ``param_groups``, per-tensor step counts, ``zero_grad``."""

    def _init_groups(self, trunk, encoder, no_decay, lr, bert_lr, rule, weight_decay, warmup, t_total, betas, eps, adam_betas, adam_eps):
        if rule not in RULES:
            raise ValueError("rule %r: one of %s" % (rule, ", ".join(RULES)))
        if not (warmup == -1 or 0.0 <= warmup < 1.0):
            raise ValueError("warmup %r: in [0, 1), or -1" % (warmup,))
        self.trunk, self.encoder = list(trunk), list(encoder)
        self.params = self.trunk + self.encoder
        self.no_decay = set(id(p) for p in no_decay)
        if len(set(id(p) for p in self.params)) != len(self.params) or not self.no_decay <= set(id(p) for p in self.encoder):
            raise ValueError("a parameter is in one group, once; no_decay is a subset of the encoder group")
        self.param_groups = [{"params": self.trunk, "lr": lr, "betas": betas, "eps": eps, "weight_decay": 0},
                             {"params": self.encoder, "lr": bert_lr, "betas": adam_betas, "eps": adam_eps, "weight_decay": weight_decay,
                              "rule": rule, "warmup": warmup, "t_total": t_total}]
        self.step_count = 0
        self.steps = {id(p): 0 for p in self.params}      # every parameter's own steps: bias corrections and schedule position

    def zero_grad(self, set_to_none=True):
        for p in self.params:
            if p.grad is not None:
                if set_to_none:
                    p.grad = None
                else:
                    p.grad.zero_()

    def step(self):
        self.clip_and_step(None)

    def _coefficients(self, p):
        """(a, dec, c) of encoder tensor ``p``, whose step count already includes this step."""
        g = self.param_groups[1]
        return adam_coefficients(g["rule"], g["lr"], 0.0 if id(p) in self.no_decay else g["weight_decay"], g["betas"], self.steps[id(p)],
                                 g["warmup"], g["t_total"])

    def _group_dicts(self):
        return [{k: v for k, v in g.items() if k != "params"} for g in self.param_groups]


class FusedAdamaxAdam(_TwoGroups):
    """Adamax over ``trunk`` (``pinned`` as in FusedAdamax) and Adam over ``encoder`` under one global clip norm, on the HIP kernels."""

    def __init__(self, trunk, encoder, no_decay=(), lr=2e-3, bert_lr=5e-5, rule="adamw", weight_decay=0.01, warmup=-1, t_total=-1,
                 betas=(0.9, 0.999), eps=1e-8, adam_betas=(0.9, 0.999), adam_eps=1e-6, pinned=None):
        self._init_groups(trunk, encoder, no_decay, lr, bert_lr, rule, weight_decay, warmup, t_total, betas, eps, adam_betas, adam_eps)
        for p in self.params:
            if not (p.is_cuda and p.dtype == torch.float32 and p.is_contiguous()):
                raise ValueError("FusedAdamaxAdam: contiguous fp32 device parameters only")
        self.pinned = {id(p): int(n) for p, n in (pinned or {}).items()}
        if not set(self.pinned) <= set(id(p) for p in self.trunk):
            raise ValueError("FusedAdamaxAdam: pinned rows belong to trunk tensors")
        self.state = {id(p): {"exp_avg": torch.zeros_like(p), "exp_inf": torch.zeros_like(p)} for p in self.trunk}
        self.state.update({id(p): {"exp_avg": torch.zeros_like(p), "exp_avg_sq": torch.zeros_like(p)} for p in self.encoder})
        self._plan_key = None
        self.norm_coef = None             # device tensor [total_norm, clip_coef] of the last clip_and_step

    def state_dict(self):
        return {"step": self.step_count, "steps": [self.steps[id(p)] for p in self.params], "param_groups": self._group_dicts(),
                "state": [{k: v.clone() for k, v in self.state[id(p)].items()} for p in self.params]}

    def load_state_dict(self, sd):
        self.step_count = int(sd["step"])
        for p, n in zip(self.params, sd["steps"]):
            self.steps[id(p)] = int(n)
        for g, s in zip(self.param_groups, sd["param_groups"]):
            g.update(s)
        for p, st in zip(self.params, sd["state"]):
            for k, v in self.state[id(p)].items():
                v.copy_(st[k])

    def _plan(self, live, n_trunk):
        """Chunk lists - the norm's over every live tensor (indices into ``live``), one update list per group (indices inside the
        group) - and the static pointer tables.  Sent anew every step, in one copy: gradient pointers (int64), then the trunk's
        lr / (1 - beta1^step) and the encoder's {a, dec, c} as fp32 in the int64 slots behind them."""
        dev = live[0].device
        lists = [[], [], [], [], [], [], [], [], []]         # norm t/s/c, trunk update t/s/c, encoder update t/s/c
        for t, p in enumerate(live):
            n = p.numel()
            n_upd = n
            if id(p) in self.pinned:
                n_upd = min(n, self.pinned[id(p)] * (n // p.shape[0]))
            for s in range(0, n, _CHUNK):
                lists[0].append(t); lists[1].append(s); lists[2].append(min(_CHUNK, n - s))
            o, tl = (3, t) if t < n_trunk else (6, t - n_trunk)
            for s in range(0, n_upd, _CHUNK):
                lists[o].append(tl); lists[o + 1].append(s); lists[o + 2].append(min(_CHUNK, n_upd - s))
        ints = torch.tensor(np.concatenate([np.asarray(v, dtype=np.int64) for v in lists]).astype(np.int32), device=dev)
        cut = np.cumsum([0] + [len(v) for v in lists])
        part = [ints[cut[i]:cut[i + 1]] for i in range(9)]
        second = lambda p: self.state[id(p)]["exp_inf" if "exp_inf" in self.state[id(p)] else "exp_avg_sq"]
        n_live, n_enc = len(live), len(live) - n_trunk
        off_clr = n_live                                   # int64 slot where the trunk's fp32 table starts
        off_tab = off_clr + (n_trunk + 1) // 2             # ... and the encoder's
        n_slots = off_tab + (3 * n_enc + 1) // 2
        host = [torch.empty(n_slots, dtype=torch.int64).pin_memory() for _ in range(2)]
        self._plan_val = {"norm": (part[0], part[1], part[2], len(lists[0])), "norm_upd": None,
                          "trunk": (part[3], part[4], part[5], len(lists[3])), "enc": (part[6], part[7], part[8], len(lists[6])),
                          "ints": ints, "partial": torch.empty(len(lists[0]), dtype=torch.float32, device=dev),
                          "ptrs": torch.tensor([[p.data_ptr() for p in live], [self.state[id(p)]["exp_avg"].data_ptr() for p in live],
                                                [second(p).data_ptr() for p in live]], dtype=torch.int64, device=dev),
                          "host": host, "host_np": [h.numpy() for h in host], "dev": torch.empty(n_slots, dtype=torch.int64, device=dev),
                          "off": (off_clr, off_tab)}
        if self.pinned:
            # extra_sq (dp.GradSync.pinned_sq) stands for the re-pinned rows: that norm runs over the updated elements only
            t2 = torch.cat([part[3], part[6] + n_trunk]); s2 = torch.cat([part[4], part[7]]); c2 = torch.cat([part[5], part[8]])
            self._plan_val["norm_upd"] = (t2, s2, c2, int(t2.numel()))
        self.norm_coef = torch.zeros(2, dtype=torch.float32, device=dev)

    def clip_and_step(self, max_norm=None, extra_sq=None):
        """clip_grad_norm_(all parameters of both groups, max_norm) (skipped when None), then Adamax over the trunk and Adam over the
        encoder.  One norm; both update launches read its clip coefficient from ``self.norm_coef`` on the device.  ``extra_sq`` as in
        ``FusedAdamax.clip_and_step``."""
        live = [p for p in self.params if p.grad is not None]      # trunk tensors first
        if not live:
            return
        n_live = len(live)
        n_trunk = sum(1 for p in self.trunk if p.grad is not None)
        key = tuple(id(p) for p in live)
        if key != self._plan_key:
            self._plan(live, n_trunk)
            self._plan_key = key
        pl = self._plan_val
        slot = self.step_count & 1
        tab = pl["host_np"][slot]
        off_clr, off_tab = pl["off"]
        g0 = self.param_groups[0]
        clr = tab[off_clr:off_tab].view(np.float32)
        adam = tab[off_tab:].view(np.float32)
        for i, p in enumerate(live):
            g = p.grad
            if not (g.is_contiguous() and g.dtype == torch.float32):
                g = p.grad = g.contiguous().float()
            tab[i] = g.data_ptr()
            self.steps[id(p)] += 1
            if i < n_trunk:
                clr[i] = g0["lr"] / (1.0 - g0["betas"][0] ** self.steps[id(p)])
            else:
                j = 3 * (i - n_trunk)
                adam[j:j + 3] = self._coefficients(p)
        dev_tab = pl["dev"]
        dev_tab.copy_(pl["host"][slot], non_blocking=True)
        lib = hip.kernels()
        st = hip.stream_ptr()
        self.step_count += 1
        coef = None
        if max_norm is not None:
            ct, cs, cc, n = pl["norm"] if extra_sq is None or pl["norm_upd"] is None else pl["norm_upd"]
            lib.ruart_grad_norm_clip(dev_tab, ct, cs, cc, n, float(max_norm), pl["partial"], self.norm_coef, extra_sq, st)
            coef = self.norm_coef
        ptrs = pl["ptrs"]
        ct, cs, cc, n = pl["trunk"]
        if n:
            lib.ruart_adamax_step(ptrs[0], dev_tab, ptrs[1], ptrs[2], ct, cs, cc, n, coef, dev_tab[off_clr:off_tab].view(torch.float32),
                                  float(g0["betas"][0]), float(g0["betas"][1]), float(g0["eps"]), st)
        ct, cs, cc, n = pl["enc"]
        if n:
            g1 = self.param_groups[1]
            lib.ruart_adam_step(ptrs[0, n_trunk:], dev_tab[n_trunk:n_live], ptrs[1, n_trunk:], ptrs[2, n_trunk:], ct, cs, cc, n, coef,
                                dev_tab[off_tab:].view(torch.float32), float(g1["betas"][0]), float(g1["betas"][1]), float(g1["eps"]), st)
        # the kernels wrote the parameters through raw pointers: tell torch (see FusedAdamax.clip_and_step)
        bump = getattr(torch.autograd.graph, "increment_version", None)
        if bump is None:
            raise RuntimeError("torch.autograd.graph.increment_version is missing: caches keyed on parameter versions "
                               "(bert_train16.accurate_weights) would go stale after this step")
        for p in live:
            bump(p)


class AdamaxAdam(_TwoGroups):
    """The same two groups in plain torch ops, on any device and in any float type: ``clip_grad_norm_`` over both groups,
    ``torch.optim.Adamax`` over the trunk, and over the encoder ``torch.optim.AdamW`` ('adamw': one torch group per tensor, since
    every tensor's learning rate follows its own step count) or the BertAdam rule restated below ('bertadam').  ``pinned`` is taken
    for the norm under ``extra_sq`` only - the rows are updated like any other and the trainer re-pins them, as it does for
    torch.optim.Adamax: the public ``pinned`` stays empty."""

    def __init__(self, trunk, encoder, no_decay=(), lr=2e-3, bert_lr=5e-5, rule="adamw", weight_decay=0.01, warmup=-1, t_total=-1,
                 betas=(0.9, 0.999), eps=1e-8, adam_betas=(0.9, 0.999), adam_eps=1e-6, pinned=None):
        self._init_groups(trunk, encoder, no_decay, lr, bert_lr, rule, weight_decay, warmup, t_total, betas, eps, adam_betas, adam_eps)
        self.pinned = {}
        self._norm_rows = {id(p): int(n) for p, n in (pinned or {}).items()}
        self._adamax = torch.optim.Adamax(self.trunk, lr=lr, betas=betas, eps=eps) if self.trunk else None
        self._adamw = None
        self._moments = {}
        if rule == "adamw" and self.encoder:
            self._adamw = torch.optim.AdamW([{"params": [p], "weight_decay": 0.0 if id(p) in self.no_decay else weight_decay}
                                             for p in self.encoder], lr=bert_lr, betas=adam_betas, eps=adam_eps)
        elif rule == "bertadam":
            self._moments = {id(p): {"exp_avg": torch.zeros_like(p), "exp_avg_sq": torch.zeros_like(p)} for p in self.encoder}
        self.norm_coef = None

    @property
    def state(self):
        """id(p) -> the moments, under torch's names (a tensor torch has not stepped yet has none)."""
        out = dict(self._moments)
        for o in (self._adamax, self._adamw):
            if o is not None:
                out.update({id(p): o.state[p] for g in o.param_groups for p in g["params"]})
        return out

    def state_dict(self):
        return {"step": self.step_count, "steps": [self.steps[id(p)] for p in self.params], "param_groups": self._group_dicts(),
                # (torch's state_dict hands out the live moment tensors, and its load_state_dict adopts tensors that already fit: copies)
                "adamax": copy.deepcopy(self._adamax.state_dict()) if self._adamax is not None else None,
                "adamw": copy.deepcopy(self._adamw.state_dict()) if self._adamw is not None else None,
                "moments": [{k: v.clone() for k, v in self._moments[id(p)].items()} for p in self.encoder if id(p) in self._moments]}

    def load_state_dict(self, sd):
        self.step_count = int(sd["step"])
        for p, n in zip(self.params, sd["steps"]):
            self.steps[id(p)] = int(n)
        for g, s in zip(self.param_groups, sd["param_groups"]):
            g.update(s)
        if self._adamax is not None:
            self._adamax.load_state_dict(sd["adamax"])
        if self._adamw is not None:
            self._adamw.load_state_dict(sd["adamw"])
        for p, st in zip([p for p in self.encoder if id(p) in self._moments], sd["moments"]):
            for k, v in self._moments[id(p)].items():
                v.copy_(st[k])

    def clip_and_step(self, max_norm=None, extra_sq=None):
        live = [p for p in self.params if p.grad is not None]
        if not live:
            return
        if max_norm is not None:
            if extra_sq is None:
                norm = torch.nn.utils.clip_grad_norm_(live, max_norm)
                coef = torch.clamp(max_norm / (norm + 1e-6), max=1.0)
            else:
                sq = [(p.grad[:self._norm_rows[id(p)]] if id(p) in self._norm_rows else p.grad).float().pow(2).sum() for p in live]
                norm = (torch.stack(sq).sum() + extra_sq.reshape(())).sqrt()
                coef = torch.clamp(max_norm / (norm + 1e-6), max=1.0)
                for p in live:
                    p.grad.mul_(coef.to(p.grad.dtype))
            self.norm_coef = torch.stack([norm.float().reshape(()), coef.float().reshape(())])
        self.step_count += 1
        for p in live:
            self.steps[id(p)] += 1
        g0, g1 = self.param_groups
        if self._adamax is not None:
            self._adamax.param_groups[0]["lr"] = g0["lr"]
            self._adamax.step()
        if self._adamw is not None:
            for g in self._adamw.param_groups:
                p = g["params"][0]
                if p.grad is not None:
                    g["lr"] = g1["lr"] * multiplier(self.steps[id(p)] - 1, g1["warmup"], g1["t_total"])
            self._adamw.step()
        elif self._moments:
            b1, b2 = g1["betas"]
            with torch.no_grad():
                for p in self.encoder:
                    if p.grad is None:
                        continue
                    # BertAdam: moments without bias correction; the decay is taken from the parameter itself, scaled by the
                    # scheduled learning rate like the Adam term - p <- p (1 - lr_t wd) - lr_t m / (sqrt(v) + eps)
                    a, dec, _ = self._coefficients(p)
                    m, v = self._moments[id(p)]["exp_avg"], self._moments[id(p)]["exp_avg_sq"]
                    m.mul_(b1).add_(p.grad, alpha=1.0 - b1)
                    v.mul_(b2).addcmul_(p.grad, p.grad, value=1.0 - b2)
                    p.mul_(dec).addcdiv_(m, v.sqrt().add_(g1["eps"]), value=-a)
