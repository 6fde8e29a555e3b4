"""CPU proof of the reference, the bounds and the case list that tests/test_gpu_train_attention.py holds the trained encoder's attention
kernels to (tests/_train_attention_ref.py): the gradient formulas equal float64 autograd, a faithful fp32 emulation of the kernels'
arithmetic stays inside every element-wise bound on every case, the same emulation with one defect leaves a bound wherever the defect
can show - so the GPU tests can fail -, the cases are what they claim to be, and the constants the emulation restates are the ones in
csrc/bert_train_attn.hip.  No kernel runs here."""
import numpy as np
import pytest
import torch

from tests import _dropout_ref as DR
from tests import _train_attention_ref as R

CASES = R.cases()


def _fmt(res):
    return ", ".join("%s %.3g" % kv for kv in res.items())


@pytest.mark.parametrize("name", CASES)
def test_formulas_equal_float64_autograd(name):
    c = R.case(name)
    x = c.qkv16.double().requires_grad_(True)
    out = DR.attention(x, c.cu, c.heads, masks=c.masks, plain=True)
    assert float((out.detach() - c.ctx).abs().max()) <= 1e-12 * max(1.0, float(c.ctx.abs().max()))
    (out * c.dO16.double()).sum().backward()
    H = c.H
    for i in range(3):
        want, got = x.grad[:, i * H:(i + 1) * H], c.dqkv[:, i * H:(i + 1) * H]
        assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())
    for r in c.seq:                                                       # lse2 = log2 sum exp(s), and a one-token sequence's dQ = dK = 0
        if r.long:
            want = torch.logsumexp(r.S, -1, keepdim=True) * R.LOG2E
            assert float((r.lse2 - want).abs().max()) <= 1e-12 * float(want.abs().max())
        if r.n == 1:
            assert float(r.dQ.abs().max()) == 0.0 and float(r.dK.abs().max()) == 0.0
    for blocks, bias in ((c.win, c.bias_win), (c.ch, c.bias_long)):
        for b in range(blocks.shape[1]):
            q0, q1 = int(blocks[0, b]), int(blocks[1, b])
            want = torch.cat([x.grad[q0:q1, :H].sum(0), x.grad[q0:q1, 2 * H:].sum(0)])
            assert float((bias[b] - want).abs().max()) <= 1e-12 * max(float(want.abs().max()), 1e-30)


@pytest.mark.parametrize("name", CASES)
def test_faithful_emulation_stays_inside_every_bound(name):
    c = R.case(name)
    plain = R.emulate(c)
    res = R.kernel_ratios(c, **plain)
    print("emulation %s: worst error / bound: %s" % (name, _fmt(res)))
    assert max(res.values()) <= 1.0
    if c.ch.shape[1]:
        out = R.emulate(c, chained=True)
        chained = R.kernel_ratios(c, long_bwd=out["long_bwd"], chained=True)
        print("emulation %s, own forward lse2: %s" % (name, _fmt(chained)))
        assert max(chained.values()) <= 1.0
    for key, b in list(R.forward_bounds(c).items()) + [(k, v) for k, v in R.backward_bounds(c).items()]:
        assert bool(torch.isfinite(b[~torch.isnan(b)]).all()), key
    # exact zeros where the bound is 0: emulation and reference agree bit for bit there
    if c.win.shape[1]:
        z = (R.backward_bounds(c)["dqkv"] == 0) & c.win_rows[:, None]
        if c.do_regime == "disparity" or 1 in c.lens:
            assert bool(z.any())
        assert not z.any() or float(plain["win_bwd"][0][z].abs().max()) == 0.0
    for s, q in R.quiet_sequence_precision(c).items():
        print("quiet sequence %s: %s of %d tokens, %s: max bound / max |ref| %.3g, ||bound|| / ||ref|| %.3g" % ((name, s[0], c.lens[s[0]], s[1]) + q))


@pytest.mark.parametrize("control", R.control_cases(), ids=lambda c: "%s-%s" % (c[1], c[0]))
def test_negative_controls_break_a_bound(control):
    """every (case, defect) pair where the defect can show (R.defect_shows): the worst ratio over the outputs of the kernels the defect
    lives in (R.DEFECT_KERNELS) exceeds 1"""
    name, defect = control
    c = R.case(name)
    res = R.kernel_ratios(c, **R.emulate(c, defect))
    res = {k: v for k, v in res.items() if k.split(".")[0] in R.DEFECT_KERNELS[defect]}
    print("control %s on %s: worst error / bound: %s" % (defect, name, _fmt(res)))
    assert max(res.values()) > 1.0


def test_every_defect_reaches_every_kernel_it_lives_in():
    """per defect: at least one showing case, and for every kernel of R.DEFECT_KERNELS[defect] a case whose outputs OF THAT KERNEL
    leave their bound; prints the smallest per-case ratio of every defect (the figure the module docstring of the reference explains
    where it is below 2)"""
    cc = R.control_cases()
    for d in R.DEFECTS:
        names = [n for n, dd in cc if dd == d]
        assert names, d
        per_case = []
        reached = {k: 0.0 for k in R.DEFECT_KERNELS[d]}
        for n in names:
            c = R.case(n)
            res = R.kernel_ratios(c, **R.emulate(c, d))
            worst = 0.0
            for k, v in res.items():
                kern = k.split(".")[0]
                if kern in reached:
                    reached[kern] = max(reached[kern], v)
                    worst = max(worst, v)
            per_case.append(worst)
        print("defect %-22s %2d cases, smallest worst ratio %.3g; best per kernel: %s" % (d, len(names), min(per_case), _fmt(reached)))
        assert min(per_case) > 1.0, d
        for kern, v in reached.items():
            assert v > 1.0, (d, kern)
    assert not R.defect_shows("win_soft", "lse_natural") and R.defect_shows("long_soft", "lse_natural")
    assert R.defect_shows("long_scales", "dkv_first_tile_scale") and not R.defect_shows("win_soft", "dkv_first_tile_scale")
    assert R.defect_shows("win_disparity", "do_unscaled") and not R.defect_shows("win_soft", "do_unscaled")
    assert not R.defect_shows("long_first", "alpha_skipped") and R.defect_shows("long_rising", "alpha_skipped")


def test_kernel_constants_are_the_source():
    k = R.source_constants()
    assert k["tile_steps"] == [R.TILE] * 4 and k["tile_clamps"] == [R.TILE] * 4           # forward, two dQ passes, the dK / dV query tiles
    assert k["drop_stride"] == [R.DROP_IDX_STRIDE]
    assert k["head_stride"] == [R.HEAD_SEED_STRIDE] * 5                                  # one per kernel
    assert [(float(a), float(b)) for a, b in k["dsc_range"]] == [R.DSC_RANGE] * 2        # the window kernel and stage_scaled_dO
    assert k["bf16_store_is_a_cast"]
    assert R.source_text().count("pack_cols<f16_t>") == 4 and "pack_cols<bf16_t>" not in R.source_text()
    assert max(R.case(n).T for n in CASES) < 2 ** 32 // R.DROP_IDX_STRIDE and max(max(R.case(n).lens) for n in CASES) <= R.DROP_IDX_STRIDE


def test_case_conditions_hold_for_the_reference():
    """asserted on the float64 reference alone: soft cases are not saturated, peaked ones are, the offset rows need the maximum
    subtraction, rising / first put the dominant key where they say, and the dO regimes are what they are named"""
    for name in CASES:
        c = R.case(name)
        for r in c.seq:
            if r.n < 8:
                continue
            eff, pmax = R.effective_keys(r)
            if c.regime == "soft":
                assert eff >= R.SOFT_FLOOR * r.n, (name, r.n, eff)
            if c.regime in ("peaked", "rising", "first"):
                assert pmax >= R.PEAK_LEVEL, (name, r.n, pmax)
                top = r.P.argmax(-1)
                if c.regime == "rising" and r.long:
                    assert bool((top >= R.TILE * ((r.n - 1) // R.TILE)).all())
                    first_max = r.S[:, :, :R.TILE].amax(-1)
                    assert bool((r.m[:, :, 0] > first_max + 1.0).all())                   # a later tile raises the maximum
                if c.regime == "first" and r.long:
                    assert bool((top < R.TILE).all())
        if c.regime == "offset":
            m = torch.cat([r.m.reshape(-1) for r in c.seq])
            assert float(m.max()) > 70 and float(m.min()) < -90
    c = R.case("win_disparity")
    assert len(c.small_seqs) == 2 and c.zero_blocks == [("win", 1)] and c.tiny_blocks == [("win", 2)]
    for s in c.small_seqs:                              # the quiet sequence's scaled dO really lies in f16's subnormal range
        a, b = int(c.cu[s]), int(c.cu[s + 1])
        g = (c.dO16[a:b].double().reshape(b - a, c.heads, 64) * c.dsc[a:b, :, None]).abs()
        assert float(((g > 0) & (g < R.F16_MIN_NORMAL)).double().mean()) > 0.5
        w = int(np.nonzero((c.win[0] <= a) & (a < c.win[1]))[0][0])
        loud = c.dO16[int(c.win[0, w]):int(c.win[1, w])].double().abs().max()
        assert float(loud / c.dO16[a:b].double().abs().max()) > 2.0 ** 11
    q0, q1 = (int(x) for x in c.win[:, 1])
    assert float(c.dO16[q0:q1].abs().max()) == 0.0 and bool((c.win_scale[1] == 1.0).all())
    assert float(R.backward_bounds(c)["dqkv"][q0:q1].abs().max()) == 0.0                # an all-zero block: exact zeros asked for
    q0, q1 = (int(x) for x in c.win[:, 2])
    assert 2e-7 < float(c.dO16[q0:q1].double().abs().mean()) < 3e-6
    c = R.case("long_scales")
    (b0,) = [b for b in range(c.ch.shape[1]) if c.ch[3, b] - c.ch[2, b] == 512 and c.ch[4, b] == b]
    sc = c.ch_scale[b0:b0 + 8, 0].log2()
    for i in range(8):                                  # 2^0, 2^-6, 2^-12 in turn; a chunk's largest entry may sit either side of a power of two
        assert abs(float(sc[i] - sc[0]) - 6 * (i % 3)) <= 1, (i, sc.tolist())
    assert c.zero_blocks and all(bool((c.ch_scale[b] == 1.0).all()) for _, b in c.zero_blocks)
    for name in CASES:                                   # uniform dO sits at about 1e-3
        c = R.case(name)
        if c.do_regime == "uniform":
            assert 5e-4 < float(c.dO16.double().abs().mean()) < 1.5e-3


def test_case_list_covers_what_the_issue_lists():
    assert set(R.REGIMES) == {R._CASES[n][2] for n in CASES}
    assert {R._CASES[n][0] for n in CASES} == {2, 3}
    assert all(200 <= R.case(n).T <= 1500 for n in CASES)
    short = set()
    for n in R.window_cases():
        c = R.case(n)
        short |= {x for x in c.lens if x <= 64}
    assert short >= {1, 2, 15, 16, 17, 63, 64}
    longs = set()
    for n in R.long_cases():
        longs |= {x for x in R.case(n).lens if x > 64}
    assert longs >= {65, 127, 128, 129, 200, 512}
    c = R.case("win_soft")
    per_win = [[int(x) for x in c.lens[i:j]] for i, j in
               zip(np.searchsorted(c.cu, c.win[0]), np.searchsorted(c.cu, c.win[1]))]
    assert any(sum(1 for x in w if x == 1) >= 3 and len(w) > 3 for w in per_win)         # several one-token sequences in one mixed window
    assert any(sum(w) == 64 and len(w) >= 2 for w in per_win)                           # a window that is exactly full, of several
    assert [64] in per_win and [40] in per_win                                          # a window of one sequence, full and not
    assert [1] in per_win                                                               # a window that holds a single token
    for n in R.long_cases():                                                            # long sequences beside short ones in the stream
        assert R.case(n).win.shape[1] >= 1
    assert {R._CASES[n][3] for n in CASES} == {"uniform", "disparity", "scales"}
    assert any(R.case(n).padded for n in R.window_cases()) and any(not R.case(n).padded for n in R.window_cases())
    assert any(R.case(n).padded for n in R.long_cases()) and any(not R.case(n).padded for n in R.long_cases())
    for n in CASES:
        c = R.case(n)
        assert (c.ld, c.ldc, c.ldd) == ((3 * c.H + 8, c.H + 8, 3 * c.H + 4) if c.padded else (3 * c.H, c.H, 3 * c.H))
        assert c.ld % 8 == 0 and c.ldc % 8 == 0 and c.ldd % 4 == 0
    drop = [n for n in CASES if R.case(n).p > 0]
    assert len(drop) == 2 and {bool(R.case(n).ch.shape[1] > 1) for n in drop} == {True, False} and all(R.case(n).p == 0.1 for n in drop)
    assert 64 in R.case(R.BOTH_PATHS_CASE).lens
    for k in R.KERNELS:
        assert any(k in R.kernels_of(n) for n in CASES)
