"""CPU proof of the references, bounds, plan and dispatch that tests/test_gpu_x3_gemm.py holds the trunk's split-bf16 products to
(tests/_x3_ref.py): a faithful emulation of the kernels' arithmetic stays inside bound (a) and bound (b) on every case of the GPU file,
the same emulation with one defect leaves bound (a) wherever the defect can show - so the GPU tests can fail -, the restated plan gives
the plans the shapes were chosen for and agrees with the library's, the GPU file's case list reaches every one of the 54 kernel
instantiations, and the GELU allowance covers its measurement.  No kernel runs here."""
import ctypes

import pytest
import torch

from tests import _x3_ref as X


def _ratios(key, defect=None):
    dk, np_, tm, sk, acc = key
    c = X.x3_case(*dk)
    out = X.x3_emulate(c, np_, tm, sk, defect, acc)
    ra = X.worst(out, *X.x3_bound(c, np_, sk, "a"))
    return ra, (X.worst(out, *X.x3_bound(c, np_, sk, "b")) if defect is None else None)


def test_the_environment_overrides_are_unset():
    assert X.env_is_default()


@pytest.mark.parametrize("key", X.emulation_keys(), ids=X.key_id)
def test_emulation_stays_inside_both_bounds(key):
    ra, rb = _ratios(key)
    print("emulation %s: worst error / bound %.4f (a) %.4f (b)" % (X.key_id(key), ra, rb))
    assert ra <= 1.0 and rb <= 1.0


@pytest.mark.parametrize("control", X.controls(), ids=lambda x: "%s-%s" % (x[1], X.key_id(x[0])))
def test_controls_break_the_bound(control):
    key, defect = control
    ra, _ = _ratios(key, defect)
    print("control %s %s: worst error / bound (a) %.3g" % (defect, X.key_id(key), ra))
    assert ra > 1.0


def test_controls_cover_every_defect_and_every_case():
    cs = X.controls()
    assert {d for _, d in cs} == set(X.DEFECTS)
    with_control = {k for k, _ in cs}
    assert all(k in with_control for k in X.emulation_keys())
    # a defect is required to show only where it can: the one-product form with its lo halves kept on a three-product case, a split
    # defect on an unsplit plan, a mask defect without a mask
    c = X.x3_case(130, 70, 97)
    assert not X.x3_defect_shows(c, "x1_lo_kept", 3) and X.x3_defect_shows(c, "x1_lo_kept", 1) and not X.x3_defect_shows(c, "drop_hl", 1)
    assert not any(X.x3_defect_shows(c, d) for d in ("slice_twice", "empty_slice_stale", "mask_unscaled", "cscale_row", "gelu_tanh", "accumulate_lost"))
    assert torch.equal(X.x3_emulate(c, 1, defect="drop_hl"), X.x3_emulate(c, 1))


def test_the_named_shapes_plan_what_they_are_meant_to():
    P, S, ks = X.make_plan, X.slices, X.ksteps_of
    for K in X.K_LIST:
        for M, N in ((130, 70), (131, 71), (132, 72)):
            assert P(M, N, K, 0, 0) == P(M, N, K, 1, 1) == (128, 2, 1)
    assert P(64, 40, 520, 1, 1) == P(65, 40, 520, 1, 1) == (128, 1, 4) and S(ks(520), 4) == [(0, 5), (5, 10), (10, 15), (15, 17)]
    assert 520 % 32 != 0                                                           # (the last slice holds the K tail)
    assert P(129, 131, 545, 0, 1) == (128, 4, 4) and ks(545) == 18
    assert P(200, 125, 1040, 1, 1) == (128, 2, 8) and P(512, 512, 1040, 0, 0) == (128, 16, 8) and ks(1040) == 33
    assert S(33, 8)[6:] == [(30, 33), (35, 33)]                                    # slice 7 is empty: it starts past the last step
    assert P(4000, 3000, 72, 0, 0) == (256, 192, 1) and P(3840, 3584, 70, 0, 0) == (256, 210, 1) and ks(72) == ks(70) == 3
    assert P(4000, 3000, 72, 0, 1) == (128, 32 * 24, 1)                            # (the big tile is for a K-contiguous B only)
    for K in (770, 772):
        assert P(2048, 2048, K, 0, 0) == P(2048, 2048, K, 1, 0) == (256, 64, 3) and S(ks(K), 3) == [(0, 9), (9, 18), (18, 25)]
    # the fallbacks of the dispatch: a width-1 operand or a masked form the big tile lacks go to the unsplit 128 tile, no workspace: unsplit
    assert X.dispatch_raw(2048, 2048, 772, 0, 0, 1, 773, 0, 776) == (128, 0, 0, 1, 4, 0, 1)
    assert X.dispatch_raw(2048, 2048, 772, 0, 0, 0, 776, 0, 776, 1, 1) == (128, 0, 0, 1, 1, 1, 1)
    assert X.dispatch_raw(2048, 2048, 772, 0, 0, 0, 776, 0, 776, have_ws=False) == (256, 0, 0, 4, 4, 0, 1)
    assert X.dispatch_raw(200, 125, 1040, 1, 1, 0, 200, 0, 128, have_ws=False)[6] == 1
    assert X.dispatch_raw(64, 64, 64, 1, 1, 0, 64, 0, 64, 1) is None and X.dispatch_raw(64, 64, 64, 0, 0, 0, 64, 0, 64, 2) is None
    assert [X.load_width(o, p, e) for o, p, e in ((0, 8, 4), (4, 8, 4), (2, 8, 4), (0, 6, 4), (0, 8, 6), (1, 8, 4), (0, 7, 4), (0, 8, 5))] == [4, 4, 2, 2, 2, 1, 1, 1]
    assert [X.load_width(0, 8, 4, m) for m in (0, 4, 2, 6, 1, 3)] == [4, 4, 2, 2, 1, 1]


def test_library_plan_agrees_with_the_restated_plan():
    from ruart_amd import hip
    lib = hip.load()
    assert X.env_is_default()
    shapes = {(s.M, s.N, s.K) + X.modes(s.lay) for s in X.all_specs()}
    for M in (1, 100, 128, 129, 500, 1000, 2048, 4000, 6400, 12800):
        for N in (1, 125, 250, 1000, 1200, 3000):
            for K in (1, 250, 500, 511, 512, 513, 800, 1388, 1800, 6400):
                shapes |= {(M, N, K, a, b) for a in (0, 1) for b in (0, 1)}
    for M, N, K, am, bm in sorted(shapes):
        sk, nb = ctypes.c_int(-1), ctypes.c_size_t(1)
        assert lib.ruart_gemm_x3_plan(M, N, K, int(am == 0), int(bm == 0), ctypes.byref(sk), ctypes.byref(nb)) == 0
        plan = X.make_plan(M, N, K, am, bm)
        assert (sk.value, nb.value) == (plan[2], X.ws_bytes_of(plan)), (M, N, K, am, bm)


def test_the_case_list_reaches_every_instantiation():
    specs = X.instantiation_specs()
    assert [X.dispatch(s)[:6] for s in specs[:len(X.INSTANTIATIONS)]] == list(X.INSTANTIATIONS)
    assert {X.dispatch(s)[:6] for s in specs} == set(X.INSTANTIATIONS) and len(X.INSTANTIATIONS) == 54
    # the big tile in both its plans at (4, 4) nt and (2, 2) A-transposed
    plans = {(X.dispatch(s)[:5], X.dispatch(s)[6] > 1) for s in specs}
    for inst in ((256, 0, 0, 4, 4), (256, 1, 0, 2, 2)):
        assert (inst, False) in plans and (inst, True) in plans
    # what the other case lists are meant to run
    for s in X.k_loop_specs():
        d = X.dispatch(s)
        assert d[0] == 128 and d[6] == 1 and d[3] == d[4] == (4 if s.K % 4 == 0 else 1)
    assert [X.dispatch(s)[6] for s in X.split_specs()] == [4, 4, 4, 8, 8]
    masks = [X.dispatch(s) for s in X.mask_specs()]
    assert {d[:6] for d in masks} == {i for i in X.INSTANTIATIONS if i[5]}
    byte_off = [X.dispatch(s) for s in X.mask_specs() if s.moff]
    assert [d[3] for d in byte_off] == [1, 1, 2]
    epi = X.epilogue_specs()
    assert {(X.dispatch(s)[0], X.dispatch(s)[6] > 1) for s in epi} == {(128, False), (128, True), (256, False)}
    for split in (False, True):                          # every option in the 16-byte and in the element-wise form, in both kernels
        mine = [s for s in epi if X.dispatch(s)[0] == 128 and (X.dispatch(s)[6] > 1) == split]
        for opt in ("bias", "gelu", "cs", "res"):
            forms = {X.epilogue_is_vector(s) for s in mine if getattr(s, opt)}
            assert forms == {True, False}, (split, opt)
        assert {s.rpm for s in mine if s.cs} == {1, 5}
    probs = X.grouped_problems()
    assert len(probs) > X.X3G_MAX and sum(1 for p in probs if p[3] == 3) > X.X3G_MAX and {p[3] for p in probs} == {0, 1, 2, 3}
    sk = [X.make_plan(M, N, K, 1, 1)[2] for M, N, K, _, _ in probs]
    acc = [p[4] for p in probs]
    assert any(a and s > 1 for a, s in zip(acc, sk)) and any(a and s == 1 for a, s in zip(acc, sk))
    assert any(sk[i - 1] > 1 and sk[i] == 1 and sk[i + 1] > 1 for i in range(1, 43)) and sk[43] == 1 and sk[44] == 1
    assert all(8 <= M <= 140 and 4 <= N <= 130 and K in (40, 520, 545, 1040) for M, N, K, _, _ in probs)


def test_the_gelu_allowance_covers_its_measurement():
    m = X.measure_erf_gelu()
    print("exact-erf GELU in fp32 (torch erf) against float64, max abs error over |x| <= 12: %.4g" % m)
    assert m <= X.ERF_GELU_MEASURED <= 1.05 * m


def test_split_is_the_kernels_rounding():
    """hi + lo carries 16 significand bits; both halves are bf16 values; the rounding is to nearest even"""
    x = torch.tensor([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, X.COH, -X.COH, 3.0e-30, 1.0e30])
    hi, lo = X.split(x)
    assert hi[:2].tolist() == [1.0, 1.0 + 2.0 ** -6]                  # ties go to the even neighbour
    assert torch.equal(hi.bfloat16().float(), hi) and torch.equal(lo.bfloat16().float(), lo)
    assert bool(((x - hi - lo).abs() <= 2.0 ** -17 * x.abs()).all()) and float(lo[2]) > 0 and float((x - hi - lo)[2]) != 0
