"""``ruart_adam_step`` and ``optim.FusedAdamaxAdam`` on the GPU: the encoder group's Adam rule against torch.optim.AdamW ('adamw') and
against the unfused restatement in float64 ('bertadam'), the two groups under one clip norm, the C ABI's refusals, the state round trip.

Bounds (those of ``test_fused_adamax_matches_torch``): per step |norm - ref| <= 1e-4 norm; per tensor max |p - p_ref| <= 2e-6 max(1, max |p_ref|);
moments within 1e-4 max |ref| - the relative slack the accepted norm tolerance can put on g * coef."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from ruart_amd import hip                                  # noqa: E402
from ruart_amd.optim import AdamaxAdam, FusedAdamaxAdam    # noqa: E402

DEV = "cuda:0"
# every boundary of the chunk (8192) and vector (4) logic, a tensor of two chunks and a tail, one of 38 chunks
SHAPES = [(1,), (3,), (4,), (5,), (8191,), (8192,), (8193,), (16389,), (7, 3, 5), (300, 1024)]
NO_DECAY = (1, 3, 5, 7, 9)            # half of the tensors take no weight decay
SKIP = 8                              # this tensor has no gradient on even steps: its own step count drives its coefficients
LR, WD, EPS, CLIP, STEPS = 1e-3, 0.01, 1e-6, 10.0, 5


def _inputs(shapes, seed=0):
    """(initial parameters, per step a list of gradients) on the host in fp32; step 1 is clipped hard, the others are not."""
    g = torch.Generator().manual_seed(seed)
    init = [torch.randn(*s, generator=g) * 0.1 for s in shapes]
    grads = [[torch.randn(*s, generator=g) * (5.0 if step == 1 else 0.01) for s in shapes] for step in range(STEPS)]
    return init, grads


def _set_grads(params, grads, step, skip, dtype=torch.float32):
    for k, (p, gr) in enumerate(zip(params, grads[step])):
        p.grad = None if (k == skip and step % 2 == 0) else gr.to(device=p.device, dtype=dtype).clone()


def _check(step, norm, norm_ref, pairs, moments):
    assert abs(norm - norm_ref) <= 1e-4 * norm_ref, (step, norm, norm_ref)
    for a, b in pairs:                                      # (reference, fused)
        a = a.detach().to(device=b.device, dtype=torch.float64)
        err, scale = float((a - b.detach().double()).abs().max()), max(1.0, float(a.abs().max()))
        assert err <= 2e-6 * scale, (step, tuple(b.shape), err)
    for a, b in moments:
        a = a.to(device=b.device, dtype=torch.float64)
        err = float((a - b.double()).abs().max())
        assert err <= 1e-4 * float(a.abs().max()), (step, tuple(b.shape), err)


def test_adamw_matches_torch():
    """The kernel through the optimizer against torch.optim.AdamW on the device, five steps."""
    init, grads = _inputs(SHAPES)
    ref = [torch.nn.Parameter(p.to(DEV)) for p in init]
    mine = [torch.nn.Parameter(p.to(DEV)) for p in init]
    o_ref = torch.optim.AdamW([{"params": [p for k, p in enumerate(ref) if k not in NO_DECAY], "weight_decay": WD},
                               {"params": [ref[k] for k in NO_DECAY], "weight_decay": 0.0}], lr=LR, eps=EPS)
    o = FusedAdamaxAdam([], mine, [mine[k] for k in NO_DECAY], bert_lr=LR, rule="adamw", weight_decay=WD, adam_eps=EPS)
    norms = []
    for step in range(STEPS):
        _set_grads(ref, grads, step, SKIP)
        _set_grads(mine, grads, step, SKIP)
        norm = float(torch.nn.utils.clip_grad_norm_(ref, CLIP))
        o_ref.step()
        o.clip_and_step(CLIP)
        norms.append(norm)
        moments = [(o_ref.state[a][k], o.state[id(b)][k]) for a, b in zip(ref, mine) if len(o_ref.state[a]) for k in ("exp_avg", "exp_avg_sq")]
        assert len(moments) == 2 * (len(SHAPES) - (step == 0))
        _check(step, float(o.norm_coef[0]), norm, zip(ref, mine), moments)
    assert norms[1] > 50 * CLIP and max(norms[0], norms[2]) < CLIP          # step 1 is clipped hard, the others are not
    assert o.steps[id(mine[SKIP])] == 2 and o.steps[id(mine[0])] == STEPS and int(o_ref.state[ref[SKIP]]["step"]) == 2
    assert float((mine[-1].detach().cpu() - init[-1]).abs().max()) > 1e-3   # the updates are orders of magnitude above the bound


def test_bertadam_matches_the_float64_restatement():
    """Rule 'bertadam' with warm-up 0.5 of 8 steps against ``AdamaxAdam`` in float64 on the CPU from the same inputs; the first step
    (lr_t = 0) leaves every parameter's bits alone while both moments move."""
    init, grads = _inputs(SHAPES, seed=1)
    ref = [torch.nn.Parameter(p.double()) for p in init]
    mine = [torch.nn.Parameter(p.to(DEV)) for p in init]
    kw = dict(bert_lr=LR, rule="bertadam", weight_decay=WD, adam_eps=EPS, warmup=0.5, t_total=8)
    o_ref = AdamaxAdam([], ref, [ref[k] for k in NO_DECAY], **kw)
    o = FusedAdamaxAdam([], mine, [mine[k] for k in NO_DECAY], **kw)
    for step in range(STEPS):
        _set_grads(ref, grads, step, SKIP, dtype=torch.float64)
        _set_grads(mine, grads, step, SKIP)
        o_ref.clip_and_step(CLIP)
        o.clip_and_step(CLIP)
        live = [(a, b) for a, b in zip(ref, mine) if a.grad is not None or step > 0]
        moments = [(o_ref.state[id(a)][k], o.state[id(b)][k]) for a, b in live for k in ("exp_avg", "exp_avg_sq")]
        _check(step, float(o.norm_coef[0]), float(o_ref.norm_coef[0]), zip(ref, mine), moments)
        if step == 0:
            for k, (p, p0) in enumerate(zip(mine, init)):
                assert torch.equal(p.detach().cpu(), p0), k
                if k != SKIP:
                    assert float(o.state[id(p)]["exp_avg"].abs().max()) > 0 and float(o.state[id(p)]["exp_avg_sq"].abs().max()) > 0
    assert float((mine[-1].detach().cpu() - init[-1]).abs().max()) > 1e-4


def test_two_groups_one_norm():
    """Trunk-like tensors under Adamax (one with re-pinned rows) and encoder-like ones under 'adamw' in one ``clip_and_step`` against
    clip_grad_norm_(all) + Adamax.step + AdamW.step."""
    t_shapes, e_shapes = [(2000, 300), (1000,), (33, 129)], [(768, 768), (768,), (8193,), (5,)]
    init, grads = _inputs(t_shapes + e_shapes, seed=2)
    nt, rows = len(t_shapes), 100
    ref = [torch.nn.Parameter(p.to(DEV)) for p in init]
    mine = [torch.nn.Parameter(p.to(DEV)) for p in init]
    fixed = init[0][rows:].to(DEV)
    o_max = torch.optim.Adamax(ref[:nt], lr=2e-3)
    o_adam = torch.optim.AdamW([{"params": [ref[nt], ref[nt + 2]], "weight_decay": WD}, {"params": [ref[nt + 1], ref[nt + 3]], "weight_decay": 0.0}],
                               lr=LR, eps=EPS)
    o = FusedAdamaxAdam(mine[:nt], mine[nt:], [mine[nt + 1], mine[nt + 3]], lr=2e-3, bert_lr=LR, rule="adamw", weight_decay=WD, adam_eps=EPS,
                        pinned={mine[0]: rows})
    assert [g["lr"] for g in o.param_groups] == [2e-3, LR] and len(o.param_groups) == 2
    skip = nt + 2
    for step in range(STEPS):
        _set_grads(ref, grads, step, skip)
        _set_grads(mine, grads, step, skip)
        both = float(torch.cat([p.grad.flatten() for p in ref if p.grad is not None]).double().norm())
        norm = float(torch.nn.utils.clip_grad_norm_(ref, CLIP))                # one norm over both groups, pinned rows included
        assert abs(norm - both) <= 1e-5 * both
        o_max.step()
        o_adam.step()
        ref[0].data[rows:] = fixed                                              # the trainer's re-pin (the fused step never wrote them)
        o.clip_and_step(CLIP)
        assert torch.equal(mine[0].detach()[rows:], fixed)
        moments = [(o_max.state[a]["exp_avg"][:rows], o.state[id(b)]["exp_avg"][:rows]) for a, b in zip(ref[:1], mine[:1])]
        moments += [(o_adam.state[a][k], o.state[id(b)][k]) for a, b in zip(ref[nt:], mine[nt:]) if len(o_adam.state[a])
                    for k in ("exp_avg", "exp_avg_sq")]
        _check(step, float(o.norm_coef[0]), norm, zip(ref, mine), moments)
    assert set(o.state[id(mine[0])]) == {"exp_avg", "exp_inf"} and set(o.state[id(mine[nt])]) == {"exp_avg", "exp_avg_sq"}


def test_extra_sq_stands_for_the_pinned_rows():
    """``extra_sq`` (data parallelism, dp.GradSync.pinned_sq): the norm runs over the updated elements of both groups and the scalar is
    added in place of the re-pinned rows - fused and unfused against the sum written out here; with the rows' own squared norm as
    the scalar the step is the one without ``extra_sq``."""
    shapes, rows = [(300, 50), (1000,), (768, 12), (8193,)], 40
    init, grads = _inputs(shapes, seed=4)
    gr = grads[1]                                          # the hard-clipped set
    extra = float(gr[0][rows:].double().pow(2).sum())
    want = (sum(float(x.double().pow(2).sum()) for x in gr[1:]) + float(gr[0][:rows].double().pow(2).sum()) + extra) ** 0.5
    out = []
    for cls, with_extra in ((FusedAdamaxAdam, True), (AdamaxAdam, True), (FusedAdamaxAdam, False)):
        ps = [torch.nn.Parameter(p.to(DEV)) for p in init]
        o = cls(ps[:2], ps[2:], [ps[3]], lr=2e-3, bert_lr=LR, rule="adamw", weight_decay=WD, adam_eps=EPS, pinned={ps[0]: rows})
        for p, x in zip(ps, gr):
            p.grad = x.to(DEV).clone()
        o.clip_and_step(CLIP, extra_sq=torch.tensor([extra], device=DEV) if with_extra else None)
        assert abs(float(o.norm_coef[0]) - want) <= 1e-4 * want, (cls.__name__, with_extra)
        assert abs(float(o.norm_coef[1]) - CLIP / want) <= 1e-4 * CLIP / want
        out.append([p.detach().clone() for p in ps])
    assert torch.equal(out[0][0][rows:], init[0][rows:].to(DEV))                   # the fused step leaves the pinned rows alone
    for k in range(len(shapes)):
        a, b, c = (o[k][:rows] if k == 0 else o[k] for o in out)
        assert float((a - b).abs().max()) <= 2e-6 * max(1.0, float(b.abs().max())), k
        assert float((a - c).abs().max()) <= 2e-6 * max(1.0, float(c.abs().max())), k
        assert not torch.equal(a, init[k].to(DEV)[:a.shape[0]])


def test_c_abi_refusals():
    """``ruart_adam_step`` with no chunks or without its coefficient table: hipErrorInvalidValue, nothing launched."""
    lib = hip.load()
    n = 4096
    p, g, m, v = (torch.full((n,), x, device=DEV) for x in (1.0, 0.5, 0.25, 0.125))
    tabs = torch.tensor([[t.data_ptr()] for t in (p, g, m, v)], dtype=torch.int64, device=DEV)
    chunk = torch.tensor([0, 0, n], dtype=torch.int32, device=DEV)
    tab = torch.tensor([1e-3, 1.0, 1.0], device=DEV)
    P = hip.ptr
    args = lambda n_chunks, table: (P(tabs[0]), P(tabs[1]), P(tabs[2]), P(tabs[3]), P(chunk[0:1]), P(chunk[1:2]), P(chunk[2:3]), n_chunks,
                                    None, table, 0.9, 0.999, 1e-6, hip.stream_ptr())
    invalid = 1                                             # hipErrorInvalidValue
    assert lib.ruart_adam_step(*args(0, P(tab))) == invalid
    assert lib.ruart_adam_step(*args(-1, P(tab))) == invalid
    assert lib.ruart_adam_step(*args(1, None)) == invalid
    torch.cuda.synchronize()
    for t, x in ((p, 1.0), (g, 0.5), (m, 0.25), (v, 0.125)):
        assert bool((t == x).all())
    assert lib.ruart_adam_step(*args(1, P(tab))) == 0       # the same arguments, complete: it runs
    torch.cuda.synchronize()
    assert bool((p != 1.0).all()) and bool((m != 0.25).all()) and bool((v != 0.125).all()) and bool((g == 0.5).all())


def test_state_dict_round_trip():
    """Three steps, save, load into a fresh optimizer over cloned parameters, one more step on both: parameters and moments bit-equal
    (the per-tensor step counts carry the bias corrections and the schedule position)."""
    t_shapes, e_shapes = [(50, 30), (1000,)], [(300, 1024), (768,), (8193,)]
    init, grads = _inputs(t_shapes + e_shapes, seed=3)
    nt = len(t_shapes)

    def make(params):
        return FusedAdamaxAdam(params[:nt], params[nt:], [params[nt + 1]], lr=2e-3, bert_lr=LR, rule="adamw", weight_decay=WD, adam_eps=EPS,
                               warmup=0.25, t_total=8, pinned={params[0]: 20})

    a = [torch.nn.Parameter(p.to(DEV)) for p in init]
    oa = make(a)
    for step in range(3):
        _set_grads(a, grads, step, nt + 1)
        oa.clip_and_step(CLIP)
    b = [torch.nn.Parameter(p.detach().clone()) for p in a]
    ob = make(b)
    ob.load_state_dict(oa.state_dict())
    assert [ob.steps[id(p)] for p in b] == [3, 3, 3, 1, 3] and ob.step_count == 3
    _set_grads(a, grads, 3, nt + 1)
    _set_grads(b, grads, 3, nt + 1)
    oa.clip_and_step(CLIP)
    ob.clip_and_step(CLIP)
    assert torch.equal(oa.norm_coef, ob.norm_coef)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
        assert oa.state[id(x)].keys() == ob.state[id(y)].keys()
        assert all(torch.equal(oa.state[id(x)][k], ob.state[id(y)][k]) for k in oa.state[id(x)])
    assert not torch.equal(a[nt].detach().cpu(), init[nt])
