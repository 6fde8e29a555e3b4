"""Float64 reference, counted element-wise error bounds and a CPU emulation of the sub-word pooling kernels (csrc/bert_kernels.hip:
ruart_bert_pool_mix / _bwd and the pair over pre-LayerNorm rows, ruart_bert_pool_mix_ln / _ln_bwd).  Test infrastructure: numpy on the
CPU, no GPU import; used by tests/test_gpu_pooling_kernels.py and proven on the CPU by tests/test_pooling_ref.py.

The operation (include/ruart_hip.h; Models/Bert/Bert.py:149-165 + Models/SDNet.py:573-581), restated in float64 on the kernels' inputs.
Word w has n = span_len[w] pieces; its rows in layer l start at span_start[w], in the LAST layer at span_start_last[w] where that is given:
    row_l[p]             = layers[l][start_l(w) + p][:H]                                   plain form
                         = (y - mu) rstd gamma_l + beta_l,  (mu, rstd) = stats[l][start_l(w) + p]      _ln form, y the stored row
    m[l, w]              = mean_p row_l[p]
    out[dst_row[w]]      = sum_l wl[l] m[l, w]
    partial[w, l]        = <grad_out[dst_row[w]], m[l, w]>
    grad_layer_w[l]      = sum_w partial[w, l]
The statistics are inputs: the kernels do not compute them, and neither does the reference.

The bounds.  u = 2^-24, the unit roundoff of fp32.  Every kernel forms its result from the inputs (exact in fp32; the 16-bit types widen
exactly) by fp32 products and sums; a result that is a sum of terms, each of which went through at most k roundings, differs from the
exact value by at most ((1 + u)^k - 1) A <= 1.01 k u A for k u < 0.01 (k <= 482 here), A = the same expression with every term replaced
by its absolute value.  The bound does not depend on the order of any sum, so every form of a kernel is held to the same one.
  forward      A = sum_l |wl| mean_p |row|                         _ln:  sum_l |wl| (|gamma| mean_p |(y - mu) rstd| + |beta|)
               k = NL (n + c) + 2,  c = 2 plain, c = 5 _ln.  Counted in the source, longest path of one term to the stored element:
               1 / n and wl / n: 2 (once: the "+ 2"); per layer the piece sum (v0 + v1: 1), the product with the weight (1), the sum
               into the accumulator (1) and one product and one sum per further piece, n - 2 sums into the accumulator at most: an early
               term passes at most NL (n - 1) accumulator sums, the layer-split form NL / 4 of them and 3 more across the waves; its own
               2 roundings are within the c = 2 per layer.  _ln adds y - mu, the product with rstd, the product with gamma (3), and beta
               enters through one product and one sum (pool_mix_cols_ln_kernel) or NL sums of the table prologue
               (pool_mix_cols_ln_reg_kernel): c = 5.  FMA contraction only removes roundings.
  partial      A = sum_c |g_c| mean_p |row_c|                      _ln:  sum_c |g_c| (|gamma_c| mean_p |x_c| + |beta_c|)
               k = (n + c) + H + 2: the piece sums (n - 1), the product with the gradient (1), 1 / n and the product with it (2), _ln's
               three and the sum with beta (1); then the dot product: sums over column groups, the four elements of a lane and the
               wave - a zero summand rounds nothing, so at most H - 1 of them whatever their order.
  grad_layer_w A = sum_w A_partial[w, l],  k = k_partial(longest word) + W: the reduction's W - 1 sums in any order.
  the trained encoder's form, bert_train.pool_mix (torch ops, one rounding per op; torch_form_bounds, layers_grad64), same A:
               forward k = 2 NL + n (NL products, NL - 1 sums, the division, the index_add's n sums); layer_w's gradient
               k = 2 + W + (covered rows) H (grad_mixed, the product, a sum over every element of the span rows in any order);
               the layers' gradient wl[l] / n grad_out[dst[w]] scattered to the span rows: the division, the product with wl, and one
               sum per further word that covers the row: k = 2 + further covering words.
No constant above was fitted to a result.  emulate() redoes the kernels' arithmetic in fp32 on the CPU (1 / n in fp32, wl / n formed
first, beta once per layer); ``defect`` breaks one thing on purpose (DEFECTS), each a way these kernels can go wrong, to show that the
bounds would catch such a kernel: control_cases(defect) names the cases on which it must show, DEFECT_OUTPUTS where.

Cases.  ``CASES`` lists (form, type, H, n_layers, W, spans, last, pads, stride): ``spans`` "prefix" = lengths 1, 2, 3, 4, 9 then random 1..3,
"ones" / "twos" = every word that long; ``last`` = span_start_last given (the last layer's rows in an order of their own); ``pads`` = what
ldl / ldo / ldg exceed H by; ``stride`` = what layer_stride (and the stats' stride) exceed Tp ldl (Tp) by.  Rows are 0.3 + N(0, 1) with one
element in 32 about 25 times larger, as a pretrained encoder's outlier columns are; 16-bit cases hold values of the type exactly;
every row no span covers and every pad column is NaN in the rows, the statistics and grad_out; dst_row is a permutation into a
buffer with three rows no word owns.
"""
import functools
import types

import numpy as np

U32 = 2.0 ** -24
SLACK = 1.01
C_PLAIN, C_LN = 2, 5
TP = 64
SPARE_ROWS = 3
PREFIX = (1, 2, 3, 4, 9)
WPB = 4                          # words per workgroup of the register-table kernels (RUART_POOL_LN_WPB)

DEFECTS = ("skip_third_piece", "last_layer_start", "pad_layer_weighted", "stats_of_first_piece", "beta_per_piece", "clamped_lane_counted",
           "last_word_of_group_dropped", "acc16")
DEFECT_OUTPUTS = {"skip_third_piece": ("out", "partial", "grad_w"), "last_layer_start": ("out", "partial", "grad_w"),
                  "pad_layer_weighted": ("out",), "stats_of_first_piece": ("out", "partial", "grad_w"),
                  "beta_per_piece": ("out", "partial", "grad_w"), "clamped_lane_counted": ("partial", "grad_w"),
                  "last_word_of_group_dropped": ("out", "partial"), "acc16": ("out", "partial")}

#        name                 form     type    H     NL  W    spans     last   pads         stride
CASES = {
    "p-f32-H4-L1-W1":        ("plain", "f32", 4, 1, 1, "prefix", False, (0, 0, 0), 0),
    "p-f32-H128-L3-W3":      ("plain", "f32", 128, 3, 3, "prefix", True, (4, 8, 12), 40),
    "p-f16-H260-L5-W5":      ("plain", "f16", 260, 5, 5, "prefix", False, (4, 4, 4), 0),
    "p-bf16-H260-L7-W41":    ("plain", "bf16", 260, 7, 41, "prefix", True, (0, 0, 0), 0),
    "p-f32-H256-L6-W4":      ("plain", "f32", 256, 6, 4, "prefix", True, (8, 4, 4), 0),
    "p-f16-H768-L12-W41":    ("plain", "f16", 768, 12, 41, "prefix", False, (0, 0, 0), 0),
    "p-bf16-H768-L13-W5":    ("plain", "bf16", 768, 13, 5, "prefix", True, (4, 8, 4), 24),
    "p-f32-H1024-L24-W5":    ("plain", "f32", 1024, 24, 5, "prefix", False, (0, 0, 0), 0),
    "p-f32-H1024-L32-W3":    ("plain", "f32", 1024, 32, 3, "twos", True, (0, 0, 0), 0),
    "p-f16-H1024-L32-W4":    ("plain", "f16", 1024, 32, 4, "ones", False, (0, 0, 0), 0),
    "p-f32-H768-L12-W301":   ("plain", "f32", 768, 12, 301, "prefix", True, (0, 0, 0), 0),
    "p-f32-H128-L13-W5":     ("plain", "f32", 128, 13, 5, "ones", False, (0, 0, 0), 0),
    "p-bf16-H4-L32-W5":      ("plain", "bf16", 4, 32, 5, "twos", False, (4, 4, 4), 8),
    "p-f32-H260-L12-W4":     ("plain", "f32", 260, 12, 4, "prefix", True, (4, 4, 8), 0),
    "p-f16-H128-L6-W41":     ("plain", "f16", 128, 6, 41, "prefix", False, (0, 0, 0), 0),
    "p-bf16-H256-L1-W5":     ("plain", "bf16", 256, 1, 5, "prefix", True, (0, 0, 0), 0),
    "p-f32-H768-L1-W41":     ("plain", "f32", 768, 1, 41, "prefix", False, (0, 0, 0), 0),
    "p-bf16-H1024-L3-W3":    ("plain", "bf16", 1024, 3, 3, "prefix", False, (0, 0, 0), 0),
    "l-H256-L1-W5":          ("ln", "f32", 256, 1, 5, "prefix", True, (0, 0, 0), 0),
    "l-H256-L3-W3":          ("ln", "f32", 256, 3, 3, "prefix", False, (4, 8, 12), 40),
    "l-H768-L5-W4":          ("ln", "f32", 768, 5, 4, "prefix", False, (0, 0, 0), 0),
    "l-H768-L6-W5":          ("ln", "f32", 768, 6, 5, "twos", True, (0, 0, 0), 0),
    "l-H1024-L7-W41":        ("ln", "f32", 1024, 7, 41, "prefix", False, (8, 4, 4), 0),
    "l-H768-L12-W41":        ("ln", "f32", 768, 12, 41, "prefix", True, (0, 0, 0), 0),
    "l-H768-L12-W5":         ("ln", "f32", 768, 12, 5, "prefix", False, (4, 8, 4), 24),
    "l-H768-L12-W3":         ("ln", "f32", 768, 12, 3, "ones", False, (0, 0, 0), 0),
    "l-H768-L12-W1":         ("ln", "f32", 768, 12, 1, "prefix", True, (0, 0, 0), 0),
    "l-H768-L12-W4":         ("ln", "f32", 768, 12, 4, "twos", True, (0, 0, 0), 0),
    "l-H256-L12-W5":         ("ln", "f32", 256, 12, 5, "prefix", False, (0, 0, 0), 0),
    "l-H1024-L12-W5":        ("ln", "f32", 1024, 12, 5, "prefix", True, (0, 0, 0), 0),
    "l-H768-L13-W5":         ("ln", "f32", 768, 13, 5, "prefix", False, (0, 0, 0), 0),
    "l-H1024-L24-W5":        ("ln", "f32", 1024, 24, 5, "prefix", True, (0, 0, 0), 0),
    "l-H256-L32-W4":         ("ln", "f32", 256, 32, 4, "prefix", False, (0, 0, 0), 0),
    "l-H768-L12-W301":       ("ln", "f32", 768, 12, 301, "prefix", True, (0, 0, 0), 0),
    "l-H768-L1-W41":         ("ln", "f32", 768, 1, 41, "prefix", False, (0, 0, 0), 0),
}


def cases(form=None):
    return [n for n, c in CASES.items() if form is None or c[0] == form]


def round_to(x, kind):
    """float32 array -> the nearest value of ``kind`` (round to nearest even), as float32"""
    x = np.asarray(x, dtype=np.float32)
    if kind == "f32":
        return x
    if kind == "f16":
        return x.astype(np.float16).astype(np.float32)
    b = x.view(np.uint32).astype(np.uint64)
    b = (b + 0x7fff + ((b >> 16) & 1)) & 0xffff0000
    return b.astype(np.uint32).view(np.float32).reshape(x.shape)


def span_lengths(spans, W, rng):
    if spans == "ones":
        return np.ones(W, dtype=np.int32)
    if spans == "twos":
        return np.full(W, 2, dtype=np.int32)
    n = list(PREFIX[:W]) + [int(v) for v in rng.integers(1, 4, size=max(0, W - len(PREFIX)))]
    return np.asarray(n, dtype=np.int32)


def _place(lens, order, Tp, at):
    """first rows for the words taken in ``order`` from row ``at`` on: packed one after the other with an uncovered row after every third
    word; a word that no longer fits shares the rows of an earlier word at least as long (as the duplicates of a de-duplicated batch do)"""
    start = np.zeros(len(lens), dtype=np.int32)
    placed = []
    for k, w in enumerate(order):
        n = int(lens[w])
        if at + n <= Tp:
            start[w] = at
            placed.append(w)
            at += n + (1 if k % 3 == 2 else 0)
        else:
            longer = [v for v in placed if lens[v] >= n]
            start[w] = start[longer[k % len(longer)]]
    return start


def _covered(start, lens, Tp):
    m = np.zeros(Tp, dtype=bool)
    for s, n in zip(start, lens):
        m[s:s + n] = True
    return m


def _make(name, form, kind, H, NL, lens, start, start_last, dst, n_rows, pads, stride, seed, poison=True, Tp=TP):
    """the case object: arrays as the kernels take them (float32 / int32), NaN where nothing may be read"""
    rng = np.random.default_rng(seed)
    W = len(lens)
    ldl, ldo, ldg = (H + p for p in pads)
    x = (0.3 + rng.standard_normal((NL, Tp, ldl))).astype(np.float32)
    x = np.where(rng.random(x.shape) < 1.0 / 32, x * 25.0, x).astype(np.float32)
    c = types.SimpleNamespace(name=name, form=form, kind=kind, H=H, NL=NL, W=W, Tp=Tp, ldl=ldl, ldo=ldo, ldg=ldg, n_rows=n_rows,
                              layer_stride=Tp * ldl + stride, stats_stride=Tp + (stride // 8 if stride else 0),
                              span_start=np.asarray(start, dtype=np.int32), span_len=np.asarray(lens, dtype=np.int32),
                              span_start_last=None if start_last is None else np.asarray(start_last, dtype=np.int32),
                              dst_row=np.asarray(dst, dtype=np.int32), stats=None, gamma=None, beta=None)
    cover = np.stack([_covered(c.span_start, lens, Tp)] * NL)
    if start_last is not None:
        cover[NL - 1] = _covered(c.span_start_last, lens, Tp)
    c.cover = cover
    if form == "ln":
        mu = (0.3 + 0.5 * rng.standard_normal((NL, Tp))).astype(np.float32)
        sd = (0.5 + rng.random((NL, Tp)) * 2.0).astype(np.float32)
        x = (mu[:, :, None] + sd[:, :, None] * (x - 0.3)).astype(np.float32)
        xs = x[:, :, :H].astype(np.float64)
        stats = np.stack([xs.mean(2), 1.0 / np.sqrt(xs.var(2) + 1e-12)], axis=2).astype(np.float32)
        c.stats = np.full((NL, c.stats_stride, 2), np.nan, dtype=np.float32)
        c.stats[:, :Tp] = stats
        g = (1.0 + 0.3 * rng.standard_normal((NL, H))).astype(np.float32)
        c.gamma = np.where(rng.random(g.shape) < 1.0 / 64, g * 8.0, g).astype(np.float32)
        c.beta = (0.2 * rng.standard_normal((NL, H))).astype(np.float32)
        if poison:
            c.stats[:, :Tp][~cover] = np.nan
    x = round_to(x, kind)
    if poison:
        x[~cover] = np.nan
        x[:, :, H:] = np.nan
    c.layers = x
    c.layer_w = ((0.2 + rng.random(NL)) * rng.choice([-1.0, 1.0], size=NL)).astype(np.float32)
    g = rng.standard_normal((n_rows, ldg)).astype(np.float32)
    if poison:
        owned = np.zeros(n_rows, dtype=bool)
        owned[c.dst_row] = True
        g[~owned] = np.nan
        g[:, H:] = np.nan
    c.grad_out = g
    return c


@functools.lru_cache(maxsize=None)
def pooling_case(name):
    """everything one launch of the case ``name`` needs, seeded by the name; read-only (shared between tests)"""
    form, kind, H, NL, W, spans, last, pads, stride = CASES[name]
    seed = int.from_bytes(name.encode(), "little") % (2 ** 31)
    rng = np.random.default_rng(seed)
    lens = span_lengths(spans, W, rng)
    start = _place(lens, list(range(W)), TP, 1)
    # the compacted last layer keeps its rows in an order of its own: longest words first, ties backwards, from row 2 on
    start_last = _place(lens, sorted(range(W), key=lambda w: (-int(lens[w]), -w)), TP, 2) if last else None
    n_rows = W + SPARE_ROWS
    dst = rng.permutation(n_rows)[:W]
    c = _make(name, form, kind, H, NL, lens, start, start_last, dst, n_rows, pads, stride, seed + 1)
    for a in vars(c).values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return c


def case_from_spans(layers, ln, start, lens, dst, n_rows, layer_w, grad_out, start_last=None, name="batch"):
    """a case around given (NL, Tp, H) rows and descriptors (the Python layer's tests): no pads, no poison of its own"""
    layers = np.asarray(layers, dtype=np.float32)
    NL, Tp, H = layers.shape
    c = types.SimpleNamespace(name=name, form="ln" if ln is not None else "plain", kind="f32", H=H, NL=NL, W=len(lens), Tp=Tp, ldl=H, ldo=H, ldg=H,
                              n_rows=n_rows, layer_stride=Tp * H, stats_stride=Tp, span_start=np.asarray(start, dtype=np.int32),
                              span_len=np.asarray(lens, dtype=np.int32),
                              span_start_last=None if start_last is None else np.asarray(start_last, dtype=np.int32),
                              dst_row=np.asarray(dst, dtype=np.int32), layers=layers, layer_w=np.asarray(layer_w),
                              grad_out=np.asarray(grad_out, dtype=np.float32), stats=None, gamma=None, beta=None)
    if ln is not None:
        c.stats, c.gamma, c.beta = (np.asarray(t, dtype=np.float32) for t in ln)
    return c


def ragged_batch():
    """a small ragged group for the Python layer: (ids (3, 12), mask, offsets [3][5][2], word_mask (3, 5)) - rows of 12 / 7 / 9 pieces,
    words of 1..4 pieces, four masked words, an empty span [5, 5) and an inverted one [6, 5)"""
    rng = np.random.default_rng(11)
    mask = np.zeros((3, 12), dtype=bool)
    for i, n in enumerate((12, 7, 9)):
        mask[i, :n] = True
    ids = rng.integers(1, 90, size=(3, 12))
    offsets = [[[1, 2], [2, 5], [5, 5], [5, 7], [7, 11]],
               [[1, 3], [3, 4], [4, 6], [6, 5], [1, 1]],
               [[1, 5], [5, 6], [6, 8], [0, 0], [0, 0]]]
    word_mask = np.array([[1, 1, 1, 0, 1], [1, 1, 1, 1, 0], [1, 1, 1, 0, 0]], dtype=bool)
    return ids, mask, offsets, word_mask


def spans_from_definition(group_index, offsets, word_mask):
    """the pooling descriptors of one group as Models/Bert/Bert.py:155-165 defines the words (a masked word and a span with ed <= st
    are zero rows: no descriptor), written without ruart_amd.bert.word_spans: (start, length, dst_row, n_rows)"""
    N, Lw = word_mask.shape
    start, lens, dst = [], [], []
    for i in range(N):
        for j in range(Lw):
            st, ed = offsets[i][j]
            if bool(word_mask[i, j]) and ed > st:
                start.append(int(group_index[i, st]))
                lens.append(ed - st)
                dst.append(i * Lw + j)
    return start, lens, dst, N * Lw


# ---------------------------------------------------------------------------------------------------------
# float64 reference and bounds
# ---------------------------------------------------------------------------------------------------------
def _start(c, l, w):
    return int(c.span_start_last[w]) if (c.span_start_last is not None and l == c.NL - 1) else int(c.span_start[w])


def _rows64(c, l, w, absolute=False):
    """the n rows of word w in layer l as the operation defines them, float64 (n, H); ``absolute``: every term by its absolute value,
    returned as (|scaled part|, |constant part|)"""
    s, n, H = _start(c, l, w), int(c.span_len[w]), c.H
    y = c.layers[l, s:s + n, :H].astype(np.float64)
    if c.form != "ln":
        return (np.abs(y), 0.0) if absolute else y
    st = c.stats[l, s:s + n].astype(np.float64)
    x = (y - st[:, 0:1]) * st[:, 1:2]
    g, b = c.gamma[l].astype(np.float64), c.beta[l].astype(np.float64)
    return (np.abs(x) * np.abs(g), np.abs(b)) if absolute else x * g + b


def reference64(c):
    """(out (n_rows, H), partial (W, NL), grad_layer_w (NL,)) in float64, from the definition; rows of out no word owns are NaN"""
    out = np.full((c.n_rows, c.H), np.nan)
    partial = np.zeros((c.W, c.NL))
    wl = c.layer_w.astype(np.float64)
    for w in range(c.W):
        d = int(c.dst_row[w])
        g = c.grad_out[d, :c.H].astype(np.float64)
        acc = np.zeros(c.H)
        for l in range(c.NL):
            m = _rows64(c, l, w).mean(0)
            acc += wl[l] * m
            partial[w, l] = float(g @ m)
        out[d] = acc
    return out, partial, partial.sum(0)


def rounding_counts(c):
    """k of the module docstring: (forward (W,), partial (W,), grad_layer_w scalar)"""
    cc = C_LN if c.form == "ln" else C_PLAIN
    n = c.span_len.astype(np.float64)
    k_fwd = c.NL * (n + cc) + 2
    k_par = (n + cc) + c.H + 2
    return k_fwd, k_par, float(k_par.max()) + c.W


def magnitudes(c):
    """A of the module docstring: (A_out (n_rows, H), NaN on rows no word owns; A_partial (W, NL))"""
    a_out = np.full((c.n_rows, c.H), np.nan)
    a_par = np.zeros((c.W, c.NL))
    wl = np.abs(c.layer_w.astype(np.float64))
    for w in range(c.W):
        d = int(c.dst_row[w])
        g = np.abs(c.grad_out[d, :c.H].astype(np.float64))
        a = np.zeros(c.H)
        for l in range(c.NL):
            scaled, const = _rows64(c, l, w, absolute=True)
            m = scaled.mean(0) + const
            a += wl[l] * m
            a_par[w, l] = float(g @ m)
        a_out[d] = a
    return a_out, a_par


def bound(c):
    """element-wise bounds of the three results, shaped like reference64's (rows of out no word owns: NaN)"""
    k_fwd, k_par, k_gw = rounding_counts(c)
    assert k_fwd.max() * U32 < 0.01 and k_gw * U32 < 0.01
    a_out, a_par = magnitudes(c)
    k_rows = np.ones((c.n_rows, 1))
    k_rows[c.dst_row, 0] = k_fwd
    return SLACK * U32 * k_rows * a_out, SLACK * U32 * k_par[:, None] * a_par, SLACK * U32 * k_gw * a_par.sum(0)


def torch_form_bounds(c):
    """bert_train.pool_mix, a composition of torch ops with one rounding each, on a plain fp32 case: (bound of out, of layer_w's gradient).
    Forward: NL products, NL - 1 sums over the layers, the division by n, the n sums of the index_add: k = 2 NL + n.  layer_w's gradient
    is the sum over all Tp H elements of layers[l] * grad_mixed, non-zero on the span rows only: grad_mixed (division, one sum per further
    word on the row: 1 + W at most), the product (1), and at most (covered rows) H - 1 sums in any order."""
    assert c.form == "plain" and c.kind == "f32"
    a_out, a_par = magnitudes(c)
    k_rows = np.ones((c.n_rows, 1))
    k_rows[c.dst_row, 0] = 2 * c.NL + c.span_len.astype(np.float64)
    k_gw = 2.0 + c.W + float(c.span_len.sum()) * c.H
    assert k_gw * U32 < 0.01
    return SLACK * U32 * k_rows * a_out, SLACK * U32 * k_gw * a_par.sum(0)


def layers_grad64(c):
    """d loss / d layers of the plain form for the given grad_out, by hand: wl[l] / n grad_out[dst[w]] on every row of word w's span;
    (gradient (NL, Tp, H) float64, its bound: 2 roundings - the division, the product - and one per further word on the same row)"""
    g = np.zeros((c.NL, c.Tp, c.H))
    a = np.zeros((c.NL, c.Tp, c.H))
    cnt = np.zeros((c.NL, c.Tp, 1))
    wl = c.layer_w.astype(np.float64)
    for w in range(c.W):
        n = int(c.span_len[w])
        go = c.grad_out[int(c.dst_row[w]), :c.H].astype(np.float64)
        for l in range(c.NL):
            s = _start(c, l, w)
            g[l, s:s + n] += wl[l] / n * go
            a[l, s:s + n] += abs(wl[l]) / n * np.abs(go)
            cnt[l, s:s + n] += 1
    return g, SLACK * U32 * (2 + np.maximum(cnt - 1, 0)) * a


def worst_ratio(got, ref, bnd):
    """max |got - ref| / bound over the elements that have a bound; inf where got is not finite or the bound is 0 and the result differs"""
    ok = ~np.isnan(bnd)
    got, ref, bnd = np.asarray(got, dtype=np.float64)[ok], ref[ok], bnd[ok]
    if got.size == 0:
        return 0.0
    if not np.isfinite(got).all():
        return float("inf")
    err = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0.0, 0.0, err / bnd)
    return float(r.max())


# ---------------------------------------------------------------------------------------------------------
# the kernels' arithmetic in fp32
# ---------------------------------------------------------------------------------------------------------
def control_cases(defect):
    """the cases on which ``defect`` changes a result by construction"""
    names = []
    for name, (form, kind, H, NL, W, spans, last, pads, stride) in CASES.items():
        longest = {"ones": 1, "twos": 2}.get(spans, max(PREFIX[:W]))
        show = {"skip_third_piece": longest >= 3,
                "last_layer_start": last and W > 1,
                "pad_layer_weighted": NL % 6 != 0,
                "stats_of_first_piece": form == "ln" and longest >= 2,
                "beta_per_piece": form == "ln" and longest >= 2,
                "clamped_lane_counted": form == "plain" and H % 256 != 0,
                "last_word_of_group_dropped": form == "ln" and NL == 12 and W % WPB != 0,
                "acc16": kind == "f32" or longest >= 2}[defect]       # one 16-bit piece is its own f16 / fits f16 exactly
        if show:
            names.append(name)
    return names


def emulate(c, defect=None):
    """(out, partial, grad_layer_w) float32 as the kernels compute them (any summation order is within the bound: numpy's here);
    ``defect``: one of DEFECTS.  Rows of out no word owns, and anything a defect leaves unwritten, are NaN."""
    assert defect is None or defect in DEFECTS
    f = np.float32
    H, NL = c.H, c.NL
    out = np.full((c.n_rows, H), np.nan, dtype=f)
    partial = np.full((c.W, NL), np.nan, dtype=f)
    ln = c.form == "ln"
    n_clamped = ((H + 255) // 256 * 256 - H) // 4
    for w in range(c.W):
        if defect == "last_word_of_group_dropped" and w >= c.W // WPB * WPB:
            continue
        n = int(c.span_len[w])
        d = int(c.dst_row[w])
        inv = f(1.0) / f(n)
        go = c.grad_out[d, :H]
        acc = np.zeros(H, dtype=f)
        for l in range(NL):
            s = int(c.span_start[w]) if defect == "last_layer_start" else _start(c, l, w)
            np_ = min(n, 2) if defect == "skip_third_piece" else n
            y = c.layers[l, s:s + np_, :H]
            wgt = c.layer_w[l] * inv
            if ln:
                st = c.stats[l, s:s + np_]
                if defect == "stats_of_first_piece":
                    st = np.repeat(st[:1], np_, axis=0)
                x = ((y - st[:, 0:1]) * st[:, 1:2]).astype(f).sum(0, dtype=f)
            else:
                x = y.sum(0, dtype=f)
            if defect == "acc16":
                x = x.astype(np.float16).astype(f)
            if ln:
                be = c.beta[l] * f(n) if defect == "beta_per_piece" else c.beta[l]
                term = (x * c.gamma[l]) * wgt + be * c.layer_w[l]
                row = (x * c.gamma[l]) * inv + be
                prod = row * go
            else:
                term = x * wgt
                prod = x * go
            reps = 1
            if defect == "pad_layer_weighted" and l == NL - 1:
                reps += (-NL) % 6                      # the padding slots of the last block of six re-read the last layer's rows
            for _ in range(reps):
                acc = acc + term
            dot = prod.sum(dtype=f)
            if defect == "clamped_lane_counted":
                dot = dot + f(n_clamped) * prod[H - 4:].sum(dtype=f)
            partial[w, l] = dot if ln else dot * inv
        out[d] = acc
    with np.errstate(invalid="ignore"):
        gw = partial.sum(0, dtype=f)
    return out, partial, gw
