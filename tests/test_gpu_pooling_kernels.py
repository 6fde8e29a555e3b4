"""The sub-word pooling kernels (csrc/bert_kernels.hip), called by name through the C ABI and held to the float64 reference of
tests/_pooling_ref.py at its counted, element-wise bounds (proven on the CPU, negative controls included, by tests/test_pooling_ref.py).
Every test prints its worst error / bound ratio before it asserts (profiles/pooling_kernel_tests.txt holds the values of one run).

Per case and kernel form: the forward output, partial_ws (W x n_layers: an output buffer) and grad_layer_w inside the bound element by
element; no NaN in any result (every row no span covers, every pad column and every grad_out row no word owns is NaN on the way in);
the rows of `out` no word owns and its pad columns still the sentinel bit for bit, as the words past the ends of partial_ws and
grad_layer_w; a second launch bit-equal to the first.

Which kernel a case reaches (P.CASES: p-<type>-H<H>-L<n_layers>-W<words> the plain pair, l-... the pair over pre-LayerNorm rows):
  pool_mix_kernel<T, NG> / pool_mix_bwd_kernel<T, NG>, NG = ceil(H / 256): every p- case in the backward; in the forward the cases with
      H % 256 != 0 (H = 4, 128: NG = 1, lanes past the row's end; H = 260: NG = 2, the clamped last group) and, at
      ruart_bert_pool_set_variant(0), the others (H = 256 / 768 / 1024: NG = 1 / 3 / 4).  <float, 1..4>, <f16_t, 1..4>, <bf16_t, 1..4> all
      occur.  n_layers = 1 (one wave works), 3 (fewer layers than waves), 5 / 6 / 7 and 12 / 13 (per = 2, 3, 4: a block of three short of
      one, exact, plus one), 24, 32.
  pool_mix_cols_kernel<T>: the p- cases with H % 256 == 0 at variant 1 (n_layers 1, 3, 6, 12, 13, 24, 32 around its blocks of six).
  pool_mix_cols_ln_kernel: the l- cases with n_layers != 12, and those with 12 at ruart_bert_pool_ln_set_variant(0).
  pool_mix_cols_ln_reg_kernel<12>: the l- cases with n_layers = 12 at variants 1 and 2 (H = 256, 768, 1024; W = 1, 3, 4, 5, 41, 301).
  pool_mix_bwd_ln_kernel<NG>: every l- case (NG = 1, 3, 4) but
  pool_mix_bwd_ln_reg_kernel<3, 12>: the l- cases with n_layers = 12, H = 768 at variant 2.
  reduce_partials_kernel: every case; W = 301 takes its loop past the 256 threads.

Why a kernel with one of P.DEFECTS would fail here: tests/test_pooling_ref.py shows each defect outside the bound on every case of
P.control_cases(defect), in the CPU emulation of these kernels' arithmetic, and each kernel above runs at least one of those cases:
skip_third_piece and stats_of_first_piece / beta_per_piece need a word of three / two pieces (every "prefix" case with W >= 3 / 2, in
each kernel's list), last_layer_start a case with span_start_last (eight p-, seven l- cases, in every kernel's list),
pad_layer_weighted n_layers % 6 != 0 (1, 3, 5, 7, 13, 32 ...), clamped_lane_counted the eight H % 256 != 0 cases,
last_word_of_group_dropped the n_layers = 12 l- cases with W = 1, 3, 5, 41, 301, acc16 every case but the one-piece 16-bit one.
"""
import types

import numpy as np
import pytest
import torch

from ruart_amd import hip
from tests import _pooling_ref as P

pytestmark = pytest.mark.gpu

INVALID = 1                      # hipErrorInvalidValue: what an entry point returns for arguments it refuses before launching
SENTINEL = -7.0e30
DT = {"f32": hip.DT_F32, "bf16": hip.DT_BF16, "f16": hip.DT_F16}
TORCH_TYPE = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
PARTIAL_SPARE, GW_SPARE = 8, 4


def dev():
    return torch.device("cuda:0")


@pytest.fixture
def pool_variant(request):
    """(ruart_bert_pool_set_variant, ruart_bert_pool_ln_set_variant) for one test; the defaults (1, 1) afterwards"""
    lib = hip.load()
    cols, reg = request.param
    assert lib.ruart_bert_pool_set_variant(cols) == 0 and lib.ruart_bert_pool_ln_set_variant(reg) == 0
    yield request.param
    assert lib.ruart_bert_pool_set_variant(1) == 0 and lib.ruart_bert_pool_ln_set_variant(1) == 0


def _runs(form):
    runs = []
    for name in P.cases(form):
        _, _, H, NL = P.CASES[name][:4]
        if form == "plain":
            variants = [(1, 1), (0, 1)] if H % 256 == 0 else [(1, 1)]
        else:
            variants = [(1, 1), (1, 0)] + ([(1, 2)] if H == 768 else []) if NL == 12 else [(1, 1)]
        runs += [(name, v) for v in variants]
    return runs


_RUN_ID = lambda v: v if isinstance(v, str) else "v%d%d" % v          # noqa: E731


def _i32(a, d):
    return None if a is None else torch.from_numpy(np.array(a, dtype=np.int32)).to(d)           # (a copy: the cached case is read-only)


def _f32(a, d):
    return None if a is None else torch.from_numpy(np.array(a, dtype=np.float32)).to(d)


def _device_inputs(c, d):
    """the case on the device: the layer matrices layer_stride apart in one NaN-filled buffer, in the case's type"""
    layers = torch.full((c.NL * c.layer_stride,), float("nan"), dtype=torch.float32)
    for l in range(c.NL):
        layers[l * c.layer_stride:l * c.layer_stride + c.Tp * c.ldl] = torch.from_numpy(c.layers[l].reshape(-1).copy())          # (the cached case is read-only)
    layers = layers.to(TORCH_TYPE[c.kind])                   # exact: the case holds values of the type
    return types.SimpleNamespace(layers=layers.to(d), stats=_f32(c.stats, d), gamma=_f32(c.gamma, d), beta=_f32(c.beta, d),
                                 start=_i32(c.span_start, d), start_last=_i32(c.span_start_last, d), lens=_i32(c.span_len, d),
                                 dst=_i32(c.dst_row, d), wl=_f32(c.layer_w, d), gout=_f32(c.grad_out, d))


def _forward(c, t, out, **over):
    lib = hip.load()
    a = dict(ldl=c.ldl, ldo=c.ldo, NL=c.NL, W=c.W, H=c.H, stats=t.stats, gamma=t.gamma, beta=t.beta)
    a.update(over)
    if c.form == "ln":
        return lib.ruart_bert_pool_mix_ln(hip.ptr(t.layers), c.layer_stride, a["ldl"], a["NL"], hip.ptr(a["stats"]) if a["stats"] is not None else None,
                                          c.stats_stride, hip.ptr(a["gamma"]) if a["gamma"] is not None else None,
                                          hip.ptr(a["beta"]) if a["beta"] is not None else None, hip.ptr(t.start),
                                          hip.ptr(t.start_last) if t.start_last is not None else None, hip.ptr(t.lens), hip.ptr(t.dst), hip.ptr(t.wl),
                                          hip.ptr(out), a["ldo"], a["W"], a["H"], hip.stream_ptr())
    return lib.ruart_bert_pool_mix(hip.ptr(t.layers), c.layer_stride, a["ldl"], DT[c.kind], a["NL"], hip.ptr(t.start),
                                   hip.ptr(t.start_last) if t.start_last is not None else None, hip.ptr(t.lens), hip.ptr(t.dst), hip.ptr(t.wl),
                                   hip.ptr(out), a["ldo"], a["W"], a["H"], hip.stream_ptr())


def _backward(c, t, partial, gw, **over):
    lib = hip.load()
    a = dict(ldl=c.ldl, ldg=c.ldg, NL=c.NL, W=c.W, H=c.H, stats=t.stats, gamma=t.gamma, beta=t.beta)
    a.update(over)
    if c.form == "ln":
        return lib.ruart_bert_pool_mix_ln_bwd(hip.ptr(t.layers), c.layer_stride, a["ldl"], a["NL"],
                                              hip.ptr(a["stats"]) if a["stats"] is not None else None, c.stats_stride,
                                              hip.ptr(a["gamma"]) if a["gamma"] is not None else None,
                                              hip.ptr(a["beta"]) if a["beta"] is not None else None, hip.ptr(t.start),
                                              hip.ptr(t.start_last) if t.start_last is not None else None, hip.ptr(t.lens), hip.ptr(t.dst),
                                              hip.ptr(t.gout), a["ldg"], hip.ptr(partial), hip.ptr(gw), a["W"], a["H"], hip.stream_ptr())
    return lib.ruart_bert_pool_mix_bwd(hip.ptr(t.layers), c.layer_stride, a["ldl"], DT[c.kind], a["NL"], hip.ptr(t.start),
                                       hip.ptr(t.start_last) if t.start_last is not None else None, hip.ptr(t.lens), hip.ptr(t.dst),
                                       hip.ptr(t.gout), a["ldg"], hip.ptr(partial), hip.ptr(gw), a["W"], a["H"], hip.stream_ptr())


def _buffers(c, d):
    return (torch.full((c.n_rows, c.ldo), SENTINEL, dtype=torch.float32, device=d),
            torch.full((c.W * c.NL + PARTIAL_SPARE,), SENTINEL, dtype=torch.float32, device=d),
            torch.full((c.NL + GW_SPARE,), SENTINEL, dtype=torch.float32, device=d))


def _launch(c, t):
    """one forward and one backward launch into sentinel-filled buffers; the raw buffers on the CPU"""
    out, partial, gw = _buffers(c, t.layers.device)
    assert _forward(c, t, out) == 0
    assert _backward(c, t, partial, gw) == 0
    torch.cuda.synchronize()
    return out.cpu(), partial.cpu(), gw.cpu()


def _bits(t):
    return t.contiguous().view(torch.int32)


def _is_sentinel(t):
    return bool((_bits(t) == _bits(torch.full((1,), SENTINEL, dtype=torch.float32))).all())


@pytest.fixture(scope="module")
def references():
    """float64 reference and bounds per case, computed once and shared between the kernel forms"""
    cache = {}

    def get(name):
        if name not in cache:
            c = P.pooling_case(name)
            cache[name] = (c, P.reference64(c), P.bound(c))
        return cache[name]
    return get


def _check_case(name, variant, references):
    c, ref, bnd = references(name)
    t = _device_inputs(c, dev())
    out, partial, gw = _launch(c, t)
    owned = np.zeros(c.n_rows, dtype=bool)
    owned[c.dst_row] = True
    got = (out[:, :c.H].numpy(), partial[:c.W * c.NL].view(c.W, c.NL).numpy(), gw[:c.NL].numpy())
    ratios = [P.worst_ratio(g, r, b) for g, r, b in zip(got, ref, bnd)]
    print("%s variant (%d, %d): worst error / bound: out %.3f partial %.3f grad_layer_w %.3f" % ((name,) + tuple(variant) + tuple(ratios)))
    assert not np.isnan(got[0][owned]).any() and not np.isnan(got[1]).any() and not np.isnan(got[2]).any()
    assert max(ratios) <= 1.0
    assert _is_sentinel(out[torch.from_numpy(~owned)]) and _is_sentinel(out[:, c.H:])
    assert _is_sentinel(partial[c.W * c.NL:]) and _is_sentinel(gw[c.NL:])
    out2, partial2, gw2 = _launch(c, t)
    assert torch.equal(_bits(out2), _bits(out)) and torch.equal(_bits(partial2), _bits(partial)) and torch.equal(_bits(gw2), _bits(gw))


@pytest.mark.parametrize("name,pool_variant", _runs("plain"), indirect=["pool_variant"], ids=_RUN_ID)
def test_pool_mix_against_float64(name, pool_variant, references):
    """ruart_bert_pool_mix + ruart_bert_pool_mix_bwd, f32 / f16 / bf16 rows: pool_mix_cols_kernel<T> (variant 1, H % 256 == 0) or
    pool_mix_kernel<T, NG>, pool_mix_bwd_kernel<T, NG>, reduce_partials_kernel (module docstring: which case reaches which)"""
    _check_case(name, pool_variant, references)


@pytest.mark.parametrize("name,pool_variant", _runs("ln"), indirect=["pool_variant"], ids=_RUN_ID)
def test_pool_mix_ln_against_float64(name, pool_variant, references):
    """ruart_bert_pool_mix_ln + ruart_bert_pool_mix_ln_bwd over pre-LayerNorm fp32 rows with given (mu, rstd): pool_mix_cols_ln_kernel,
    pool_mix_cols_ln_reg_kernel<12> (n_layers = 12, variants 1 and 2), pool_mix_bwd_ln_kernel<NG>, pool_mix_bwd_ln_reg_kernel<3, 12>
    (n_layers = 12, H = 768, variant 2), reduce_partials_kernel"""
    _check_case(name, pool_variant, references)


def test_the_variant_setters_clamp_and_reach_their_kernels(references):
    """ruart_bert_pool_ln_set_variant clamps to 0..2 and ruart_bert_pool_set_variant to 0 / 1; whatever they are set to, the results stay
    inside the bound (the setters' range is part of the contract the A/B tools rely on)"""
    lib = hip.load()
    try:
        for cols, reg in ((7, 9), (-3, -1)):
            assert lib.ruart_bert_pool_set_variant(cols) == 0 and lib.ruart_bert_pool_ln_set_variant(reg) == 0
            for name in ("p-f32-H256-L6-W4", "l-H768-L12-W5"):
                _check_case(name, (cols, reg), references)
    finally:
        assert lib.ruart_bert_pool_set_variant(1) == 0 and lib.ruart_bert_pool_ln_set_variant(1) == 0


@pytest.mark.parametrize("name", ["p-f32-H256-L6-W4", "p-f16-H260-L5-W5", "l-H768-L12-W5"])
def test_refusals(name):
    """arguments the four entry points reject before they launch anything (include/ruart_hip.h; every pointer handed over is valid all the
    same): the buffers keep their sentinel"""
    c = P.pooling_case(name)
    t = _device_inputs(c, dev())
    out, partial, gw = _buffers(c, dev())
    H = c.H
    bad = [dict(H=H + 2), dict(H=1028), dict(H=2048), dict(H=0), dict(W=0), dict(W=-1), dict(NL=0), dict(NL=-1), dict(NL=33),
           dict(ldl=c.ldl + 2), dict(ldl=c.ldl + 1), dict(ldl=H - 4)]
    if c.form == "ln":
        bad += [dict(H=H + 4), dict(H=H - 128), dict(stats=None), dict(gamma=None), dict(beta=None)]
    for over in bad + [dict(ldo=c.ldo + 2), dict(ldo=c.ldo + 3), dict(ldo=H - 4)]:
        assert _forward(c, t, out, **over) == INVALID, over
    for over in bad + [dict(ldg=c.ldg + 2), dict(ldg=c.ldg + 1), dict(ldg=H - 4)]:
        assert _backward(c, t, partial, gw, **over) == INVALID, over
    torch.cuda.synchronize()
    assert _is_sentinel(out.cpu()) and _is_sentinel(partial.cpu()) and _is_sentinel(gw.cpu())
    assert _forward(c, t, out) == 0 and _backward(c, t, partial, gw) == 0          # and the same call with nothing wrong goes through
    torch.cuda.synchronize()
    assert not _is_sentinel(out.cpu()[c.dst_row.tolist()]) and not bool(torch.isnan(gw[:c.NL]).any())


# ---------------------------------------------------------------------------------------------------------
# the Python layer, without an encoder in front of it
# ---------------------------------------------------------------------------------------------------------
NL_PY, H_PY = 12, 256


def _python_case(ln, poison=True):
    """PackedTokens of the small ragged group of P.ragged_batch, random (NL, Tp, H) rows (NaN where no word reads, `poison`), optionally
    with the (stats, gamma, beta) of a LayerNorm-folded pass attached; the float64 case from descriptors written from the definition"""
    from ruart_amd.bert import PackedTokens
    ids, mask, offsets, word_mask = P.ragged_batch()
    d = dev()
    packed = PackedTokens([(torch.from_numpy(ids), torch.from_numpy(mask))], d)
    start, lens, dst, rows = P.spans_from_definition(packed.group_index[0], offsets, word_mask)
    rng = np.random.default_rng(29)
    x = (0.3 + rng.standard_normal((NL_PY, packed.Tp, H_PY))).astype(np.float32)
    tables = None
    if ln:
        mu = x.astype(np.float64).mean(2)
        stats = np.stack([mu, 1.0 / np.sqrt(x.astype(np.float64).var(2) + 1e-12)], axis=2).astype(np.float32)
        tables = (stats, (1.0 + 0.3 * rng.standard_normal((NL_PY, H_PY))).astype(np.float32),
                  (0.2 * rng.standard_normal((NL_PY, H_PY))).astype(np.float32))
    cover = np.zeros(packed.Tp, dtype=bool)
    for s, n in zip(start, lens):
        cover[s:s + n] = True
    assert not cover.all()
    gout = rng.standard_normal((rows, H_PY)).astype(np.float32)
    if poison:
        x[:, ~cover] = np.nan
        owned = np.zeros(rows, dtype=bool)
        owned[dst] = True
        gout[~owned] = np.nan
        if ln:
            tables[0][:, ~cover] = np.nan
    wl = ((0.2 + rng.random(NL_PY)) * rng.choice([-1.0, 1.0], size=NL_PY)).astype(np.float32)
    c = P.case_from_spans(x, tables, start, lens, dst, rows, wl, gout)
    layers = torch.from_numpy(x).to(d)
    if ln:
        layers._ln = tuple(torch.from_numpy(a).to(d) for a in tables)
    return c, packed, layers, offsets, torch.from_numpy(word_mask)


def _stub(trained):
    """what Bert.pool_mix reads of its module: no encoder weights, no checkpoint"""
    return types.SimpleNamespace(_device=dev(), bert_model=object() if trained else None, weights=types.SimpleNamespace(hidden=H_PY))


def _check_rows(tag, out, c, ref_out, b_out):
    """out (n_rows, H) on the CPU: the words' rows inside the bound, every other row exactly zero"""
    owned = np.zeros(c.n_rows, dtype=bool)
    owned[c.dst_row] = True
    r = P.worst_ratio(out.numpy(), ref_out, b_out)
    print("%s: out worst error / bound %.3f" % (tag, r))
    assert r <= 1.0
    assert c.n_rows - c.W == 6 and bool((_bits(out[torch.from_numpy(~owned)]) == 0).all())         # masked words, empty spans: +0.0


@pytest.mark.parametrize("ln", [False, True], ids=["rows", "prelayernorm"])
def test_python_layer_frozen(ln):
    """Bert.pool_mix -> _PoolMix (layer_w given: the mix and, through autograd, layer_w's gradient) and -> pool_last (layer_w None: the last
    layer's matrix alone, n_layers = 1, with its own statistics and tables), on plain rows and on the pre-LayerNorm rows of a folded pass"""
    from ruart_amd.bert import Bert
    c, packed, layers, offsets, word_mask = _python_case(ln)
    ref, bnd = P.reference64(c), P.bound(c)
    layer_w = torch.from_numpy(c.layer_w).to(dev()).requires_grad_()
    out = Bert.pool_mix(_stub(False), packed, layers, 0, offsets, word_mask, layer_w)
    assert out.shape == (3, 5, H_PY)
    _check_rows("python frozen ln=%d mix" % ln, out.detach().cpu().view(c.n_rows, c.H), c, ref[0], bnd[0])
    out.backward(torch.from_numpy(c.grad_out).to(dev()).view_as(out))
    r = P.worst_ratio(layer_w.grad.cpu().numpy(), ref[2], bnd[2])
    print("python frozen ln=%d: grad_layer_w worst error / bound %.3f" % (ln, r))
    assert r <= 1.0
    last = P.case_from_spans(c.layers[-1:], None if not ln else (c.stats[-1:], c.gamma[-1:], c.beta[-1:]), c.span_start, c.span_len, c.dst_row,
                             c.n_rows, np.ones(1, dtype=np.float32), c.grad_out)
    out = Bert.pool_mix(_stub(False), packed, layers, 0, offsets, word_mask, None)
    _check_rows("python frozen ln=%d last layer" % ln, out.cpu().view(c.n_rows, c.H), last, P.reference64(last)[0], P.bound(last)[0])


def test_python_layer_trained():
    """bert_train.pool_mix, the differentiable form the trained encoder takes (through Bert.pool_mix and directly): its output, layer_w's
    gradient and the gradient w.r.t. the rows against float64 at bounds counted one rounding per torch op (P.torch_form_bounds,
    P.layers_grad64).  The mix reads every row (0 x NaN would reach layer_w's gradient), so nothing is NaN here."""
    from ruart_amd.bert import Bert
    c, packed, layers, offsets, word_mask = _python_case(False, poison=False)
    owned = np.zeros(c.n_rows, dtype=bool)
    owned[c.dst_row] = True
    ref = P.reference64(c)
    b_out, b_gw = P.torch_form_bounds(c)
    ref_gl, b_gl = P.layers_grad64(c)
    layer_w = torch.from_numpy(c.layer_w).to(dev()).requires_grad_()
    layers.requires_grad_()
    out = Bert.pool_mix(_stub(True), packed, layers, 0, offsets, word_mask, layer_w)
    _check_rows("python trained mix", out.detach().cpu().view(c.n_rows, c.H), c, ref[0], b_out)
    out.backward(torch.from_numpy(c.grad_out).to(dev()).view_as(out))
    r_w = P.worst_ratio(layer_w.grad.cpu().numpy(), ref[2], b_gw)
    r_l = P.worst_ratio(layers.grad.cpu().numpy(), ref_gl, b_gl)
    print("python trained: grad_layer_w worst error / bound %.3f, layers gradient %.3f" % (r_w, r_l))
    assert r_w <= 1.0 and r_l <= 1.0
    last = P.case_from_spans(c.layers[-1:], None, c.span_start, c.span_len, c.dst_row, c.n_rows, np.ones(1, dtype=np.float32), c.grad_out)
    out = Bert.pool_mix(_stub(True), packed, layers.detach(), 0, offsets, word_mask, None)
    b_last = P.torch_form_bounds(last)[0]
    _check_rows("python trained last layer", out.cpu().view(c.n_rows, c.H), last, P.reference64(last)[0], b_last)
