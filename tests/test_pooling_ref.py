"""tests/_pooling_ref.py proven on the CPU: its float64 reference is the oracle's pool_subwords + linear_sum, the kernels' arithmetic in
fp32 stays inside the counted bounds on every case, and each defect a pooling kernel can have (P.DEFECTS) leaves them on every case
where it changes a result.  ``word_spans`` is held to the oracle's treatment of masked words and empty spans here: the kernels cannot
see a span of length 0 (include/ruart_hip.h), so the descriptors must not contain one."""
import numpy as np
import pytest
import torch

from oracle import ruart_oracle as O
from tests import _pooling_ref as P


def small_batch(NL=4, H=8):
    from ruart_amd.bert import PackedTokens
    ids, mask, offsets, word_mask = P.ragged_batch()
    packed = PackedTokens([(torch.from_numpy(ids), torch.from_numpy(mask))])
    layers = np.random.default_rng(3).standard_normal((NL, packed.Tp, H)).astype(np.float32)
    return packed, offsets, torch.from_numpy(word_mask), layers


@pytest.fixture
def float64_default():
    """the oracle allocates its pooled rows in torch's default type: float64 for the comparisons 'to float64 rounding'"""
    before = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    yield
    torch.set_default_dtype(before)


def test_word_spans_drops_masked_words_and_empty_spans():
    from ruart_amd.bert import word_spans
    packed, offsets, word_mask, _ = small_batch()
    s, n, d, rows = word_spans(packed, 0, offsets, word_mask)
    hs, hn, hd, hrows = P.spans_from_definition(packed.group_index[0], offsets, word_mask)
    assert (list(s), list(n), list(d), rows) == (hs, hn, hd, hrows)
    assert len(n) == 9 and int(n.min()) >= 1                      # 15 slots: 4 masked, [5, 5) and [6, 5) empty


def test_reference64_is_the_oracle(float64_default):
    from ruart_amd.bert import word_spans
    packed, offsets, word_mask, layers = small_batch()
    NL, Tp, H = layers.shape
    s, n, d, rows = word_spans(packed, 0, offsets, word_mask)
    alpha = torch.tensor([0.3, -0.2, 0.9, 0.1], dtype=torch.float64)
    gamma = torch.tensor(1.7, dtype=torch.float64)
    gidx = torch.from_numpy(packed.group_index[0])
    padded = [torch.from_numpy(layers[l].astype(np.float64))[gidx.clamp(min=0)] for l in range(NL)]
    pooled = O.pool_subwords(padded, offsets, word_mask)
    want = O.linear_sum(pooled, alpha, gamma).reshape(rows, H).numpy()
    wl = (torch.softmax(alpha, 0) * gamma).numpy()
    g = np.random.default_rng(5).standard_normal((rows, H)).astype(np.float32)
    c = P.case_from_spans(layers, None, s, n, d, rows, wl, g)
    out, partial, gw = P.reference64(c)
    owned = np.zeros(rows, dtype=bool)
    owned[d] = True
    assert np.isnan(out[~owned]).all() and (want[~owned] == 0.0).all()          # masked words and empty spans: the oracle's zero rows
    np.testing.assert_allclose(out[owned], want[owned], rtol=1e-13, atol=1e-14)
    # the gradient of <grad_out, out> w.r.t. the mix weights, through the oracle and autograd
    w_t = torch.from_numpy(wl).requires_grad_()
    res = sum(t * w_t[i] for i, t in enumerate(pooled)).reshape(rows, H)
    (res * torch.from_numpy(g.astype(np.float64))).sum().backward()
    np.testing.assert_allclose(gw, w_t.grad.numpy(), rtol=1e-12, atol=1e-13)
    np.testing.assert_allclose(partial.sum(0), gw, rtol=0, atol=0)
    # ... and w.r.t. the rows (the trained encoder's form)
    lay = torch.from_numpy(layers.astype(np.float64)).requires_grad_()
    pooled = O.pool_subwords([lay[l][gidx.clamp(min=0)] for l in range(NL)], offsets, word_mask)
    res = sum(t * float(wl[i]) for i, t in enumerate(pooled)).reshape(rows, H)
    (res * torch.from_numpy(g.astype(np.float64))).sum().backward()
    gl, _ = P.layers_grad64(c)
    np.testing.assert_allclose(gl, lay.grad.numpy(), rtol=1e-13, atol=1e-14)


def test_the_ln_form_of_the_reference_is_the_plain_form_on_normalised_rows():
    c = P.pooling_case("l-H256-L3-W3")
    y = c.layers[:, :, :c.H].astype(np.float64)
    st = c.stats[:, :c.Tp].astype(np.float64)
    rows = (y - st[:, :, 0:1]) * st[:, :, 1:2] * c.gamma[:, None, :].astype(np.float64) + c.beta[:, None, :].astype(np.float64)
    plain = P.case_from_spans(np.zeros((c.NL, c.Tp, c.H)), None, c.span_start, c.span_len, c.dst_row, c.n_rows, c.layer_w, c.grad_out[:, :c.H])
    plain.layers = rows                                            # float64 rows: not representable in fp32, so set past the cast
    for a, b in zip(P.reference64(c), P.reference64(plain)):
        np.testing.assert_allclose(a, b, rtol=1e-12, atol=1e-13)


def test_case_data_is_what_the_issue_asks_for():
    seen = {k: set() for k in ("H", "NL", "W", "kind", "last", "pad", "stride")}
    for name in P.cases():
        c = P.pooling_case(name)
        form = c.form
        for k, v in (("H", c.H), ("NL", c.NL), ("W", c.W), ("kind", c.kind), ("last", c.span_start_last is not None),
                     ("pad", (c.ldl > c.H, c.ldo > c.H, c.ldg > c.H)), ("stride", c.layer_stride > c.Tp * c.ldl)):
            seen[k].add((form, v))
        assert c.Tp <= 64 and (c.W <= 41 or c.W == 301)
        assert np.isnan(c.layers[~c.cover]).all() and np.isnan(c.layers[:, :, c.H:]).all()
        assert not np.isnan(c.layers[:, :, :c.H][c.cover]).any()
        assert (~c.cover).any(axis=1).all()                                   # every layer has rows no span covers
        assert np.array_equal(P.round_to(c.layers, c.kind), c.layers, equal_nan=True)
        assert len(set(c.dst_row.tolist())) == c.W and c.n_rows > c.W
        assert int(c.span_len.min()) >= 1 and int((c.span_start + c.span_len).max()) <= c.Tp
        if c.span_start_last is not None:
            assert int((c.span_start_last + c.span_len).max()) <= c.Tp
            assert c.W == 1 or (c.span_start_last != c.span_start).any()
        if form == "ln":
            assert np.isnan(c.stats[:, :c.Tp][~c.cover]).all() and not np.isnan(c.stats[:, :c.Tp][c.cover]).any()
        big = np.abs(c.layers[:, :, :c.H][c.cover])
        assert big.size < 1000 or (np.median(big) < 1.5 and (big > 10.0).mean() > 0.005)        # an offset body and a heavy tail
    for form in ("plain", "ln"):
        for H in ((4, 128, 260, 256, 768, 1024) if form == "plain" else (256, 768, 1024)):
            assert (form, H) in seen["H"]
        for NL in (1, 3, 5, 6, 7, 12, 13, 24, 32):
            assert (form, NL) in seen["NL"]
        for W in (1, 3, 4, 5, 41, 301):
            assert (form, W) in seen["W"]
        assert {(form, True), (form, False)} <= seen["last"] and {(form, True), (form, False)} <= seen["stride"]
        assert (form, (False, False, False)) in seen["pad"] and (form, (True, True, True)) in seen["pad"]
    assert {("plain", k) for k in ("f32", "f16", "bf16")} <= seen["kind"]
    for spans in ("ones", "twos"):
        for form in ("plain", "ln"):
            assert any(v[0] == form and v[5] == spans for v in P.CASES.values())
    assert int(P.pooling_case("p-f16-H768-L12-W41").span_len.max()) == 9


@pytest.mark.parametrize("name", P.cases())
def test_honest_emulation_is_inside_the_bound(name):
    c = P.pooling_case(name)
    ref, bnd, got = P.reference64(c), P.bound(c), P.emulate(c)
    ratios = [P.worst_ratio(g, r, b) for g, r, b in zip(got, ref, bnd)]
    print("%s: fp32 emulation worst error / bound: out %.3f partial %.3f grad_layer_w %.3f" % ((name,) + tuple(ratios)))
    assert max(ratios) <= 1.0
    owned = np.zeros(c.n_rows, dtype=bool)
    owned[c.dst_row] = True
    assert not np.isnan(got[0][owned]).any() and not np.isnan(got[1]).any() and not np.isnan(got[2]).any()


@pytest.mark.parametrize("defect", P.DEFECTS)
def test_every_defect_leaves_the_bound_on_its_control_cases(defect):
    names = P.control_cases(defect)
    assert names
    for name in names:
        c = P.pooling_case(name)
        ref, bnd, got = P.reference64(c), P.bound(c), P.emulate(c, defect)
        ratios = dict(zip(("out", "partial", "grad_w"), (P.worst_ratio(g, r, b) for g, r, b in zip(got, ref, bnd))))
        shown = {k: ratios[k] for k in P.DEFECT_OUTPUTS[defect]}
        print("%s on %s: worst error / bound %s" % (defect, name, " ".join("%s %.3g" % kv for kv in shown.items())))
        assert max(shown.values()) > 1.0, (defect, name, ratios)
