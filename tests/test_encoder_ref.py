"""CPU proof of the references and bounds that tests/test_gpu_encoder_kernels.py holds the encoder's kernels to (tests/_encoder_ref.py):
a faithful emulation of each attention kernel stays inside its element-wise bound on every case, and the same emulation with one
defect leaves it - so the GPU tests can fail.  No kernel runs here.  Also pins bert.split_f16c against the format of csrc/common.h."""
import numpy as np
import pytest
import torch

from tests import _encoder_ref as E

CASES = E.attention_cases()
_ID = lambda c: "%s-%s-H%d-q%s" % c          # noqa: E731


def _ratio(out, c, kind):
    return float(((out - c.ref).abs() / E.attention_bound(c, kind)).max())


@pytest.mark.parametrize("case", CASES, ids=_ID)
def test_faithful_emulation_stays_inside_the_bound(case):
    kind, layout, H, scale = case
    c = E.attention_case(layout, H, scale, E.in_type_of(kind))
    out, hi8 = E.attention_emulate(c, kind)
    r = _ratio(out, c, kind)
    print("emulation %s: worst error / bound %.3f" % (_ID(case), r))
    assert r <= 1.0
    if hi8 is not None:
        assert bool(((hi8 - c.ref).abs() <= E.hi8_bound(c.ref)).all())


@pytest.mark.parametrize("control", E.control_cases(), ids=lambda c: "%s-%s" % (c[4], _ID(c[:4])))
def test_negative_controls_break_the_bound(control):
    """every (case, defect) pair where the defect can show (E.defect_shows): the pairs where it cannot - no low halves outside the split
    kernel, no bias row to shift, every sequence a multiple of 64 keys - are not generated"""
    kind, layout, H, scale, defect = control
    c = E.attention_case(layout, H, scale, E.in_type_of(kind))
    out, _ = E.attention_emulate(c, kind, defect)
    r = _ratio(out, c, kind)
    print("control %s %s: worst error / bound %.3g" % (defect, _ID(control[:4]), r))
    assert r > 1.0


def test_controls_cover_every_case_where_a_defect_can_show():
    cc = E.control_cases()
    assert len(cc) == 24 + 24 + 54 + 36            # qk_f16, p_f16: the split cases; tile: all but "bias_long" (rows of 192); bias: pack=False
    assert not E.defect_shows("f16", "bias_long", "tile_unmasked") and E.defect_shows("f16", "long", "tile_unmasked")
    assert all(E.defect_shows(k, lay, "bias_shift") == lay.startswith("bias") for k, lay, _, _ in CASES)


def test_layouts_plan_what_the_kernel_tests_rely_on():
    """the long layout plans 11 blocks of <= 128 queries (last ATTN_QGROUP group of 3; partial blocks of 1, 2, 65 and 72 queries; partial last
    key tiles of 1, 1, 2 and 8 keys), as 64-query blocks 22; the short layout has a full window and a one-token sequence; every bias row
    keeps an open key and one has a whole trailing 64-key tile biased"""
    p = E.packed_tokens("long", True)
    lo, hi, blk, lblk = E.host_plan(p)
    assert p.n_long_blocks == 11 and p.n_long_blocks % 4 == 3
    assert sorted((lblk[1] - lblk[0])[(lblk[1] - lblk[0]) < 128].tolist()) == [1, 2, 65, 72]
    seq = {(int(a), int(b)) for a, b in zip(lblk[2], lblk[3])}
    assert sorted((b - a) % 64 for a, b in seq) == [0, 1, 1, 2, 8]
    p64 = E.packed_tokens("long", False)
    assert p64.n_long_blocks == 0 and p64.n_blocks == 2 + sum((n + 63) // 64 for n in E.LONG_LENS if n > 64)
    ps = E.packed_tokens("short", True)
    _, _, sblk, _ = E.host_plan(ps)
    assert 64 in (sblk[1] - sblk[0]).tolist() and 1 in E.SHORT_LENS and ps.n_long_blocks == 0
    assert int((sblk[1] - sblk[0]).max()) <= 64
    for layout in ("bias_short", "bias_long"):
        (ids, mask), pack = E.layout_group(layout)
        assert not pack and bool(mask.any(1).all()) and not bool(mask.all())
    (_, mask), _ = E.layout_group("bias_long")
    assert not bool(mask[0, 128:192].any()) and E.packed_tokens("bias_long", True).n_long_blocks == 6


def test_e4m3_codec_matches_torch_and_the_format():
    codes = np.arange(256, dtype=np.uint8)
    want = torch.from_numpy(codes).view(torch.float8_e4m3fn).float().numpy().astype(np.float64)
    got = E.e4m3_decode(codes)
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(got[~np.isnan(got)], want[~np.isnan(want)])
    g = torch.Generator().manual_seed(3)
    x = torch.cat([torch.randn(20000, generator=g) * s for s in (1e-3, 0.05, 1.0, 40.0, 300.0)])
    mid = torch.from_numpy((E.E4M3[:-1] + E.E4M3[1:]) / 2).float()                 # every tie
    x = torch.cat([x, mid, -mid, torch.from_numpy(E.E4M3).float(), torch.tensor([0.0, -0.0, 448.0, -448.0])])
    ref = x.clamp(-448, 448).to(torch.float8_e4m3fn).view(torch.uint8).numpy()
    assert np.array_equal(E.e4m3_encode(x.numpy()), ref)


def test_split_f16c_is_the_format_of_common_h():
    """bert.split_f16c (the host's producer of the split form, and the idiom the kernel tests compare against) against the format written
    out from common.h's description: f16(v), e4m3((v - f16(v)) 2^SA_LO), e4m3(v 2^SA_HI), saturating, row = [lo8 | hi8]"""
    from ruart_amd.bert import split_f16c
    sa_lo, sa_hi, sw_hi, sw_lo = E.header_shifts()
    assert (sa_lo, sa_hi) == (11, 0) and sa_lo + sw_hi == sa_hi + sw_lo
    g = torch.Generator().manual_seed(5)
    x = torch.cat([torch.randn(64, 96, generator=g) * s for s in (1e-4, 0.02, 1.0, 30.0, 400.0)])
    x[0, :8] = torch.tensor([0.0, -0.0, 448.0, -448.0, 1000.0, -70000.0, 2.0 ** -24, 65504.0])
    h16, h8 = split_f16c(x, lo_shift=sa_lo, hi_shift=sa_hi)
    r16, r8 = E.split_ref(x.numpy(), sa_lo, sa_hi)
    finite = np.isfinite(r16.astype(np.float32))
    finite2 = np.concatenate([finite, finite], 1)            # (an f16 overflow has no residual: inf - inf; the encoder never holds one)
    assert np.array_equal(h16.numpy().view(np.uint16), r16.view(np.uint16))
    assert np.array_equal(h8.numpy()[finite2], r8[finite2])
    fine, coarse = E.split_decode(r16, r8, 96, sa_lo, sa_hi)
    v = x.double().numpy()
    ok = finite & (np.abs(v) < 448)
    assert (np.abs(fine - v)[ok] <= 2.0 ** -15 * np.abs(v)[ok] + 2.0 ** -21).all()
    assert (np.abs(coarse - v)[ok] <= np.maximum(2.0 ** -4 * np.abs(v)[ok], 2.0 ** -10)).all()


def test_ulp_of_matches_numpy_spacing_for_f16():
    x = np.concatenate([np.random.RandomState(0).randn(1000) * s for s in (1e-7, 1e-4, 1.0, 500.0)])
    x16 = x.astype(np.float16)
    assert np.array_equal(E.ulp_of(x16.astype(np.float64), "f16"), np.spacing(np.abs(x16)).astype(np.float64))
    assert E.ulp_of(np.array([1.0, 1.5, 2.0, 0.0]), "bf16").tolist() == [2.0 ** -7, 2.0 ** -7, 2.0 ** -6, 2.0 ** -133]


@pytest.mark.parametrize("H", [4, 132, 256, 768, 1024])
@pytest.mark.parametrize("kind", E.LN_INPUTS)
def test_layernorm_fp32_formula_and_exact_rows(H, kind):
    """the fp32 formula in the kernel's order is an fp32-class evaluation of the float64 reference on every input kind, and on the
    all-zero and constant rows it returns beta bit for bit (what the kernel tests demand of the kernels)"""
    x = E.layernorm_rows(kind, 5, H, seed=H)
    g = torch.Generator().manual_seed(H + 1)
    gamma, beta = 1 + 0.1 * torch.randn(H, generator=g), 0.1 * torch.randn(H, generator=g)
    ref = E.layernorm_ref(x, gamma, beta)
    allow, cpu_err = E.layernorm_allowance(E.layernorm_fp32(x, gamma, beta), ref)
    print("layernorm fp32 formula %s H=%d: worst error %.3g, allowance %.3g" % (kind, H, cpu_err, allow))
    assert cpu_err < 2.0 ** -18 * float(ref.abs().max()) and allow >= 4 * cpu_err
    if kind == "exact":
        out = E.layernorm_fp32(x, gamma, beta)
        assert torch.equal(out[0], beta) and torch.equal(out[1], beta)
        assert torch.equal(ref[0].float(), beta) and torch.equal(ref[1].float(), beta)


def test_stats_reference_clamps_and_ignores_unused_slots():
    x = torch.full((3, 256), 7.0)
    x[1] = 30.0 + torch.randn(256, generator=torch.Generator().manual_seed(1))
    part = E.stats_partials(x, 3)
    assert bool(torch.isnan(part[:, 3]).all()) and not bool(torch.isnan(part[:, :3]).any())
    mu, rstd = E.stats_from_partials(part, 3, 256)
    assert float(mu[0]) == 7.0 and float(rstd[0]) == 1.0 / np.sqrt(E.LN_EPS)
    assert abs(float(mu[1]) - float(x[1].double().mean())) < 1e-5 and bool(torch.isfinite(rstd).all())
