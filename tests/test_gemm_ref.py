"""CPU proof of the references and bounds that tests/test_gpu_gemm.py holds the encoder's dense products to (tests/_gemm_ref.py): a
faithful emulation of each product stays inside its element-wise bound on every case, the same emulation with one defect leaves it - so
the GPU tests can fail -, the format bound of the fp16c product holds, the GELU approximation figures are measured, and the restated
tile walk and tail plan have the properties the kernel tests rely on.  No kernel runs here."""
import os
import re

import numpy as np
import pytest
import torch

from tests import _encoder_ref as E
from tests import _gemm_ref as G

_PID = lambda c: "-".join(str(x) for x in c)          # noqa: E731


def _plain(case):
    if len(case) == 5:
        dt, M, N, K, epi = case
        return G.plain_case(*case), None, G.plain_walk(M, N, K)[1]
    dt, M, N, K, cus, epi = case
    return G.plain_case(dt, M, N, K, epi), G.plain_plan(M, N, K, cus), G.plain_walk(M, N, K)[1]


def _corr(case):
    if len(case) == 4:
        return G.corr_case(*case), None, 0
    M, N, K, cus, epi = case
    return G.corr_case(M, N, K, epi), G.corr_plan(M, N, K, cus), G.tile_group_m(M // 256, N // 256, K, True)


@pytest.mark.parametrize("case", G.plain_cases() + G.plain_split_cases(), ids=_PID)
def test_plain_emulation_stays_inside_the_bound(case):
    c, plan, order = _plain(case)
    r = G.worst(G.plain_emulate(c, None, plan, order), c.ref, G.plain_bound(c, plan[2] if plan else 0))
    print("emulation gemm_16 %s: worst error / bound %.4f" % (_PID(case), r))
    assert r <= 1.0


@pytest.mark.parametrize("control", G.plain_controls(), ids=lambda x: "%s-%s" % (x[1], _PID(x[0])))
def test_plain_controls_break_the_bound(control):
    case, defect = control
    c, plan, order = _plain(case)
    r = G.worst(G.plain_emulate(c, defect, plan, order), c.ref, G.plain_bound(c, plan[2] if plan else 0))
    print("control %s gemm_16 %s: worst error / bound %.3g" % (defect, _PID(case), r))
    assert r > 1.0


@pytest.mark.parametrize("case", G.corr_cases() + G.corr_split_cases(), ids=_PID)
def test_corr_emulation_stays_inside_both_bounds(case):
    """against (a), the function of the bytes, at the kernel's bound; against (b), the unrounded operands, at that plus the format
    bound; and F itself against (b) inside the format bound alone (range-edge row and coherent rows included)"""
    c, plan, order = _corr(case)
    sl = plan[2] if plan else 0
    out, hi8 = G.corr_emulate(c, None, plan, order)
    ra, rb = G.worst(out, c.ref_a, G.corr_bound(c, sl)), G.worst(out, c.ref_b, G.corr_bound(c, sl, "b"))
    rf = G.worst(c.pre_a, c.pre_b, c.fmt)
    print("emulation gemm_16c %s: worst error / bound %.4f (a) %.4f (b); F against the unrounded product / format bound %.3f" % (_PID(case), ra, rb, rf))
    assert ra <= 1.0 and rb <= 1.0 and rf <= 1.0
    edge = (c.pre_a - c.pre_b).abs()[0] / c.fmt[0]
    assert float(edge.max()) <= 1.0 and tuple(c.A[0, :8].tolist()) == tuple(torch.tensor(G.EDGE_ROW).tolist())
    if hi8 is not None:
        assert G.worst(hi8, c.ref_a, G.corr_hi8_bound(c, sl)) <= 1.0


@pytest.mark.parametrize("control", G.corr_controls(), ids=lambda x: "%s-%s" % (x[1], _PID(x[0])))
def test_corr_controls_break_the_bound(control):
    case, defect = control
    c, plan, order = _corr(case)
    out, _ = G.corr_emulate(c, defect, plan, order)
    r = G.worst(out, c.ref_a, G.corr_bound(c, plan[2] if plan else 0))
    print("control %s gemm_16c %s: worst error / bound %.3g" % (defect, _PID(case), r))
    assert r > 1.0


@pytest.mark.parametrize("K", [256, 768])
@pytest.mark.parametrize("defect", ["corr_none", "corr_a_only", "corr_w_only"])
def test_missing_correction_terms_leave_the_corr3_bound_against_the_unrounded_product(defect, K):
    """what the on-device negative control (ruart_gemm_16c_nt_sel with corr 0 / 1 / 2) confirms: against reference (b) at the full
    product's bound the subsets of the correction fall outside (the coherent rows of corr_case: module docstring of _gemm_ref)"""
    c = G.corr_case(*G.SEL_SHAPE[K], "plain")
    out, _ = G.corr_emulate(c, defect)
    r = G.worst(out, c.ref_b, G.corr_bound(c, 0, "b"))
    print("control %s gemm_16c K=%d against (b): worst error / bound %.3g" % (defect, K, r))
    assert r > 1.0


def test_controls_cover_every_case_where_a_defect_can_show():
    pc, cc = G.plain_controls(), G.corr_controls()
    count = lambda cs, d: sum(1 for _, x in cs if x == d)          # noqa: E731
    n_plain, n_split = len(G.plain_cases()), len(G.plain_split_cases())
    assert (n_plain, n_split, len(G.corr_cases()), len(G.corr_split_cases())) == (50, 18, 9, 9)
    # chunk_drop and bias_16 everywhere; res_16 where the residual is fp32; the slice defects on every split case (all three plans
    # split); the walk wherever the row-tile count is no multiple of GROUP_M and there is more than one column tile: every plain shape
    # but (256, 256, K) [one column tile], and of the split shapes (1280, 768, 2048)
    assert count(pc, "chunk_drop") == count(pc, "bias_16") == n_plain + n_split
    assert count(pc, "res_16") == 2 * len(G.PLAIN_SHAPES) + 2 * len(G.SPLIT_SHAPES)
    assert count(pc, "slice_twice") == count(pc, "slice_missing") == n_split
    assert count(pc, "walk_partial_group") == 2 * 3 * len(G.EPIS) + 2 * len(G.SPLIT_EPIS)
    assert all(G.plain_plan(M, N, K, cus)[1] > 0 for M, N, K, cus in G.SPLIT_SHAPES)
    assert count(pc, "gelu_tanh") >= 2 * 2 * len(G.PLAIN_SHAPES) - 2          # (a 16-bit output can hide it: plain_defect_shows)
    assert count(cc, "chunk_drop") == count(cc, "bias_16") == count(cc, "corr_scale") == 18 and count(cc, "corr_none") == 9
    assert count(cc, "res_16") == 6 and count(cc, "slice_twice") == count(cc, "slice_missing") == 9
    assert count(cc, "corr_a_only") == count(cc, "corr_w_only") == 6          # unsplit, K % 256 == 0: every shape but (256, 256, 128)
    c = G.plain_case("bf16", 256, 256, 128, "plain")
    assert not G.plain_defect_shows(c, "res_16") and not G.plain_defect_shows(c, "gelu_tanh") and not G.plain_defect_shows(c, "slice_twice")


def test_gelu_approximation_is_measured():
    """the kernels' GELU formulas in fp32 numpy against erf-GELU in float64 over |x| <= 12: the constants of the bound cover the
    measurement, and the measurement stays under the figures the kernel sources quote"""
    m = G.measure_gelu()
    print("GELU approximation, max abs error over |x| <= 12: gelu_pk %.4g, gelu_fwd_bwd_pk derivative %.4g, gelu_erfc7 %.4g" % (m["pk"], m["pk_d"], m["erfc7"]))
    for k in m:
        assert m[k] <= G.GELU_APPROX[k] <= 1.05 * m[k], k
    src = lambda n: open(os.path.join(E.ROOT, "ruart_amd", "csrc", n)).read()          # noqa: E731
    quoted_pk = float(re.search(r"Max abs error ([0-9.e-]+) in", src("gemm_shared.h")).group(1))
    quoted_e7 = float(re.search(r"\|GELU error\| <= ([0-9.e-]+) over \[-12, 12\]", src("gemm_corr.hip")).group(1))
    assert m["pk"] <= quoted_pk and m["erfc7"] <= quoted_e7, (quoted_pk, quoted_e7)
    x = np.array([-20.0, -12.0, 0.0, 12.0, 30.0], dtype=np.float32)
    assert np.array_equal(G.gelu_pk32(x), np.array([-0.0, -0.0, 0.0, 12.0, 30.0], dtype=np.float32))          # saturates without a clamp


def test_tile_walk_is_a_bijection():
    for order in range(0, 65):
        for ntm in range(1, 10):
            for ntn in range(1, 10):
                seen = {G.tile_of(i, ntm, ntn, order) for i in range(ntm * ntn)}
                assert seen == {(a, b) for a in range(ntm) for b in range(ntn)}, (order, ntm, ntn)
    for n in (1, 5, 8, 15, 243):
        assert sorted(G.xcd_remap(b, n) for b in range(n)) == list(range(n))
    assert G.plain_walk(1280, 512, 256) == (256, 4) and 5 % 4 != 0          # five row tiles, GROUP_M 4: the last group is partial
    assert G.plain_walk(256, 256, 192) == (256, 8) and G.plain_walk(128, 384, 64) == (128, 8)


def test_small_shapes_plan_the_splits_they_are_meant_to():
    assert G.plain_plan(1280, 256, 768, 4) == (4, 1, 3)          # 5 tiles, r = 1: min(cus / r, 8) = 4 does not divide 12 K-tiles evenly
    assert G.plain_plan(1280, 768, 2048, 10) == (10, 5, 2)       # 15 tiles, r = 5: half full, long K
    assert G.plain_plan(1280, 768, 1024, 10) == (15, 0, 0)       # ... and left alone at a shorter K
    assert G.plain_plan(1280, 256, 256, 4) == (4, 1, 2)          # 4 K-tiles: two slices of two
    assert G.plain_plan(1280, 256, 128, 4) == (5, 0, 0)          # 2 K-tiles: no valid S
    assert G.corr_plan(1280, 256, 768, 4) == (4, 1, 4) and G.corr_plan(1280, 768, 2048, 10) == (10, 5, 2)
    assert G.corr_plan(1280, 256, 256, 4) == (4, 1, 4) and G.corr_plan(1280, 256, 128, 4) == (4, 1, 2)
    assert G.plain_plan(*G.LEFT_ALONE) == (2, 0, 0) and G.corr_plan(*G.LEFT_ALONE) == (2, 0, 0)
    for M, N, K, cus in G.SPLIT_SHAPES:                            # a slice is an even number >= 2 of K-tiles, inside one phase (fp16c)
        for plan, kt in ((G.plain_plan(M, N, K, cus), K // 64), (G.corr_plan(M, N, K, cus), 2 * (K // 64))):
            assert plan[1] > 0 and kt % plan[2] == 0 and (kt // plan[2]) % 2 == 0 and kt // plan[2] >= 2
        assert G.corr_plan(M, N, K, cus)[2] % 2 == 0


def test_library_workspace_sizes_agree_with_the_restated_plan():
    from ruart_amd import hip
    lib = hip.load()
    shapes = [s for s in G.SPLIT_SHAPES] + [G.LEFT_ALONE, (1280, 768, 1024, 10), (1280, 256, 128, 4), (81 * 256, 768, 768, 240),
                                             (128 * 256, 768, 3072, 256), (85 * 256, 1024, 3072, 240), (43 * 256, 768, 3072, 120)]
    for M in (256, 1280, 2304):
        for N in (256, 768):
            for K in (128, 256, 768, 2048, 3072):
                shapes += [(M, N, K, cus) for cus in (0, 1, 2, 3, 4, 7, 10, 16)]
    for M, N, K, cus in shapes:
        assert int(lib.ruart_gemm_16_tail_ws_bytes(M, N, K, cus)) == G.tail_bytes(G.plain_plan(M, N, K, cus)), (M, N, K, cus)
        assert int(lib.ruart_gemm_16c_tail_ws_bytes(M, N, K, cus)) == G.tail_bytes(G.corr_plan(M, N, K, cus)), (M, N, K, cus)
    assert int(lib.ruart_gemm_16_tail_ws_bytes(1280, 256, 192, 4)) == 0 and int(lib.ruart_gemm_16c_tail_ws_bytes(1280, 128, 256, 4)) == 0


def test_weight_split_is_the_format_of_common_h():
    """the W8 bytes the cases are built from are the ones the host prepares weights with (e4m3 of w16 2^SW_HI and of (w - w16) 2^SW_LO)"""
    _, _, sw_hi, sw_lo = E.header_shifts()
    W = torch.randn(64, 128, generator=torch.Generator().manual_seed(2)) * 0.03
    W[0, :4] = torch.tensor([0.0, 3.4, -1e-6, 2.0 ** -5])
    hi = W.to(torch.float16).float()
    pair = torch.cat([hi * 2.0 ** sw_hi, (W - hi) * 2.0 ** sw_lo], 1).clamp_(-448.0, 448.0).to(torch.float8_e4m3fn).view(torch.uint8)
    w16, w8 = G.weight_split_ref(W.numpy())
    assert np.array_equal(w16.view(np.uint16), W.to(torch.float16).numpy().view(np.uint16)) and np.array_equal(w8, pair.numpy())


# ---- the training products -------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("shape", G.TRAIN_SHAPES, ids=_PID)
def test_gelu2_emulation_and_controls(dt, shape):
    c = G.plain_case(dt, *shape, "gelu")
    bh, bg = G.gelu2_bounds(c)
    h, g = G.gelu2_emulate(c)
    rh, rg = G.worst(h, c.pre, bh), G.worst(g, c.ref, bg)
    line = "emulation gelu2 %s %s: worst error / bound H %.4f G %.4f;" % (dt, _PID(shape), rh, rg)
    assert rh <= 1.0 and rg <= 1.0
    for defect in G.GELU2_DEFECTS:
        h, g = G.gelu2_emulate(c, defect)
        r = max(G.worst(h, c.pre, bh), G.worst(g, c.ref, bg))
        line += " %s %.3g" % (defect, r)
        assert r > 1.0, defect
    print(line)


@pytest.mark.parametrize("shape", G.TRAIN_SHAPES, ids=_PID)
def test_gelu_bwd_emulation_and_controls(shape):
    c = G.gelu_bwd_case(*shape)
    ratios = lambda o: (G.worst(o[0], c.ref_dh, c.b_dh), G.worst(o[1], c.ref_g, c.b_g), G.worst(o[2], c.ref_col, c.b_col))          # noqa: E731
    r = ratios(G.gelu_bwd_emulate(c))
    line = "emulation gelu_bwd %s: worst error / bound dH %.4f G %.4f column sums %.4f;" % ((_PID(shape),) + r)
    assert max(r) <= 1.0
    for defect in G.GELU_BWD_DEFECTS:
        rd = ratios(G.gelu_bwd_emulate(c, defect))
        line += " %s %.3g" % (defect, max(rd))
        assert max(rd) > 1.0, defect
        if defect == "colsum_rounded":
            assert rd[0] <= 1.0 and rd[2] > 1.0          # only the strip sums can tell
    print(line)


@pytest.mark.parametrize("case", G.splitk_cases(), ids=_PID)
def test_splitk_emulation_and_controls(case):
    dt, shape, tn = case[0], case[1:5], case[5]
    c = G.splitk_case(dt, *shape, tn=tn)

    def ratios(o):
        return max([G.worst(s, r, b) for s, r, b in zip(o[0], c.slabs, c.b_slabs)] + [G.worst(o[1], c.ref[0], c.bound[0]), G.worst(o[2], c.ref[1], c.bound[1])])
    r = ratios(G.splitk_emulate(c))
    line = "emulation splitk %s %s %s: worst error / bound %.4f;" % ("tn" if tn else "nt", dt, _PID(shape), r)
    assert r <= 1.0
    for defect in G.SPLITK_DEFECTS:
        if G.splitk_defect_shows(c, defect, tn):
            rd = ratios(G.splitk_emulate(c, defect))
            line += " %s %.3g" % (defect, rd)
            assert rd > 1.0, defect
    print(line)


# ---- the LayerNorm fold ------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("case", G.consumer_cases(), ids=_PID)
def test_fold_consumer_emulation_and_controls(case):
    c = G.consumer_case(*case)
    out, hi8 = G.consumer_emulate(c)
    r = G.worst(out, c.ref, c.bound)
    line = "emulation fold consumer %s (s = %d): worst error / bound %.4f;" % (_PID(case), c.s, r)
    assert r <= 1.0
    live = torch.ones(c.M, dtype=torch.bool)
    live[3] = False                                             # (the constant row: rstd = 1e6 amplifies everything, bound included)
    assert G.worst(out[live], c.ref[live], c.bound[live]) <= 1.0
    for defect in G.CONSUMER_DEFECTS:
        if G.consumer_defect_shows(c, defect):
            o, _ = G.consumer_emulate(c, defect)
            rd = G.worst(o, c.ref, c.bound)
            line += " %s %.3g" % (defect, rd)
            assert rd > 1.0, defect
    print(line)
    assert (c.s >= 1) == (case[0] == "c8")


@pytest.mark.parametrize("case", G.producer_cases(), ids=_PID)
def test_fold_producer_emulation_and_controls(case):
    c = G.producer_case(*case)

    def ratios(o):
        stored, v, part = o
        if c.kind == "c8":
            want, pb = G.partial_bounds(stored, c.np)                       # the partials of the y WRITTEN
        else:
            want, pb = G.partial_bounds(c.ref, c.np)                        # 16-bit entries: of the unrounded y, which nobody stores
            blk = c.pre_bound.view(c.M, c.np, 256)
            pb = pb + torch.stack([blk.sum(2), (2.0 * c.ref.abs().view(c.M, c.np, 256) * blk + blk * blk).sum(2)], 2)
        return G.worst(stored, c.ref, c.bound), G.worst(part.double(), want, pb)
    r = ratios(G.producer_emulate(c))
    line = "emulation fold producer %s: worst error / bound y %.4f partials %.4f;" % ((_PID(case),) + r)
    assert max(r) <= 1.0
    for defect in G.PRODUCER_DEFECTS:
        if G.producer_defect_shows(c, defect):
            rd = ratios(G.producer_emulate(c, defect))
            line += " %s %.3g" % (defect, max(rd))
            assert max(rd) > 1.0, defect
    print(line)
