"""Float64 restatement of the three single-group update rules behind ``clip_grad_norm_`` - 'SGD' (torch.optim.SGD), 'ADAM2'
(torch.optim.Adam) and 'ADAM' (torch.optim.Adamax with coupled L2 decay) - with per-tensor step counts and pinned rows, plus the inputs
and the bounds that tests/test_fused_optimizers_host.py and tests/test_gpu_fused_optimizers.py share.

Bounds, per step (those of tests/test_gpu_fused_adam.py):  |norm - ref| <= 1e-4 ref;  per tensor max |p - p_ref| <= 2e-6 max(1, max |p_ref|);
moments within 1e-4 max |ref|.  The L2 Adamax rule adds an element-wise term to the parameter bound: g' = g coef + wd p can cancel, and
m / u then amplifies the rounding of that sum (at most 2 ulp of its larger operand, doubled for the two roundings of the products) by 1 / u:

    allow_i = 2e-6 scale + 4 clr_t 2^-23 (|g_i coef| + wd |p_i|) / u_i

with u_i the reference's exp_inf after the step and p_i the reference's parameter before it.  The term is meant for a handful of
cancelling elements: per step at most 1e-3 of the live elements may have allow_i > 1e-5 scale (``check_step`` asserts it)."""
import torch

# every boundary of the chunk (8192) and vector (4) logic, a tensor of two chunks and a tail, one of 38 chunks
SHAPES = [(1,), (3,), (4,), (5,), (8191,), (8192,), (8193,), (16389,), (7, 3, 5), (300, 1024)]
SKIP = 8                              # this tensor has no gradient on even steps: its own step count drives its coefficients
CLIP, STEPS = 10.0, 5
RULES = {"SGD": {"lr": 0.1, "wd": 0.0}, "ADAM2": {"lr": 1e-3, "wd": 0.0}, "ADAM": {"lr": 1e-3, "wd": 0.5}}
BETAS, EPS = (0.9, 0.999), 1e-8
P_TOL, NORM_TOL, MOMENT_TOL = 2e-6, 1e-4, 1e-4


def inputs(shapes=SHAPES, seed=0):
    """(initial parameters, per step a list of gradients) on the host in fp32; step 1 is clipped hard, the others are not."""
    g = torch.Generator().manual_seed(seed)
    init = [torch.randn(*s, generator=g) * 0.1 for s in shapes]
    grads = [[torch.randn(*s, generator=g) * (5.0 if step == 1 else 0.01) for s in shapes] for step in range(STEPS)]
    return init, grads


def step_grads(grads, step, skip=SKIP):
    """The gradients of ``step``; None for the tensor that sits this step out."""
    return [None if (k == skip and step % 2 == 0) else gr for k, gr in enumerate(grads[step])]


def set_grads(params, grads, step, skip=SKIP):
    for p, gr in zip(params, step_grads(grads, step, skip)):
        p.grad = None if gr is None else gr.to(device=p.device, dtype=p.dtype).clone()


class Reference:
    """One rule in float64.  ``wrong``: a deliberately wrong form ('no_clip', 'no_bc2', 'decoupled') that the bounds must tell apart."""

    def __init__(self, rule, init, lr, wd=0.0, pinned=None, wrong=None):
        assert rule in RULES and wrong in (None, "no_clip", "no_bc2", "decoupled")
        self.rule, self.lr, self.wd, self.wrong = rule, lr, wd, wrong
        self.p = [x.detach().double().clone() for x in init]
        self.m = [torch.zeros_like(x) for x in self.p]          # exp_avg
        self.s = [torch.zeros_like(x) for x in self.p]          # exp_avg_sq ('ADAM2') / exp_inf ('ADAM')
        self.steps = [0] * len(self.p)
        self.pinned = dict(pinned or {})                        # tensor index -> leading rows that are trained
        self.norm = self.coef = None
        self.last = [None] * len(self.p)                        # per tensor (clipped gradient, parameter before the step, clr)

    def step(self, grads, max_norm=CLIP, extra_sq=None):
        live = [k for k, g in enumerate(grads) if g is not None]
        gs = {k: grads[k].detach().double().cpu() for k in live}
        coef = 1.0
        if max_norm is not None:
            if extra_sq is None:
                sq = sum(float(gs[k].pow(2).sum()) for k in live)
            else:                                               # the updated elements only, the scalar in place of the rest
                sq = sum(float((gs[k][:self.pinned[k]] if k in self.pinned else gs[k]).pow(2).sum()) for k in live) + float(extra_sq)
            self.norm = sq ** 0.5
            self.coef = coef = min(1.0, max_norm / (self.norm + 1e-6))
        if self.wrong == "no_clip":
            coef = 1.0
        b1, b2 = BETAS
        for k in live:
            self.steps[k] += 1
            n = self.steps[k]
            rows = slice(0, self.pinned[k]) if k in self.pinned else slice(None)
            p, m, s, g = self.p[k][rows], self.m[k][rows], self.s[k][rows], gs[k][rows] * coef
            before = p.clone()
            if self.rule == "SGD":
                p -= self.lr * g
                clr = self.lr
            elif self.rule == "ADAM2":
                m.mul_(b1).add_(g, alpha=1 - b1)
                s.mul_(b2).add_(g * g, alpha=1 - b2)
                clr = self.lr / (1 - b1 ** n)
                bc2 = 1.0 if self.wrong == "no_bc2" else 1 - b2 ** n
                p -= clr * m / ((s / bc2).sqrt() + EPS)
            else:
                clr = self.lr / (1 - b1 ** n)
                if self.wrong == "decoupled":
                    gd = g
                    p.mul_(1 - self.lr * self.wd)
                else:
                    gd = g + self.wd * p                        # coupled: the decay joins the gradient after the clip
                m += (1 - b1) * (gd - m)
                torch.maximum(s * b2, gd.abs() + EPS, out=s)
                p -= clr * m / s
            self.last[k] = (g, before, clr)
        return self.norm, self.coef


def allowance(scale, clr, g_clipped, wd, p_before, u_after):
    """Element-wise parameter bound of the L2 Adamax rule (module docstring), float64."""
    g, p, u = (x.detach().double() for x in (g_clipped, p_before, u_after))
    return P_TOL * scale + 4.0 * clr * 2.0 ** -23 * (g.abs() + wd * p.abs()) / u


def check_step(step, norm, norm_ref, pairs, moments, allow=None):
    """``pairs``: (reference, tested) parameters; ``moments`` likewise; ``allow``: per pair None or the element-wise allowance.  Prints
    the figures, then asserts.  Returns the largest parameter error as a multiple of its bound."""
    assert abs(norm - norm_ref) <= NORM_TOL * norm_ref, (step, norm, norm_ref)
    worst, wide, total = 0.0, 0, 0
    for i, (a, b) in enumerate(pairs):
        a = a.detach().to(device=b.device, dtype=torch.float64)
        err = (a - b.detach().double()).abs()
        scale = max(1.0, float(a.abs().max()))
        al = allow[i] if allow is not None else None
        if al is None:
            ratio = float(err.max()) / (P_TOL * scale)
        else:
            al = al.to(err.device).reshape(err.shape)
            assert bool((al >= P_TOL * scale).all())
            ratio = float((err / al).max())
            wide += int((al > 1e-5 * scale).sum())
            total += al.numel()
        worst = max(worst, ratio)
        assert ratio <= 1.0, (step, i, tuple(b.shape), float(err.max()), ratio)
    for a, b in moments:
        a = a.detach().to(device=b.device, dtype=torch.float64)
        err = float((a - b.detach().double()).abs().max())
        assert err <= MOMENT_TOL * float(a.abs().max()), (step, tuple(b.shape), err)
    print("step %d: norm rel err %.2e, worst parameter err/bound %.3f, widened elements %d of %d"
          % (step, abs(norm - norm_ref) / norm_ref, worst, wide, total))
    assert wide <= 1e-3 * total, (step, wide, total)
    return worst
