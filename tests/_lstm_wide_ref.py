"""References for the streamed LSTM recurrence (128 < h <= 256 of ruart_lstm_fwd / _bwd), shared by test_lstm_wide_ref.py (CPU) and
test_gpu_lstm_wide.py (GPU).

  reference64(shape)  one nn.LSTM layer (batch_first, zero state, gate order i, f, g, o, padding not masked) and its BPTT gradients,
                      restated in float64 - no autograd.  Computed once per shape and shared; callers must not modify it.
  emulate(shape)      the same layer with the KERNELS' arithmetic in fp32: W_hh and the running h (forward) / da (backward) split into
                      bf16 hi + lo, the recurrent product as lo.hi + hi.lo + hi.hi with fp32 accumulation, everything else of the
                      recurrence in fp32.  The three plain GEMMs around the recurrence (input projection, dx, the weight gradients) are
                      not what these tests are about: they are taken in float64 from the fp32 tensors the kernels see.
                      ``defect`` emulates one way the kernels can be wrong (negative controls).

The bounds are the ones tests/test_gpu_kernels.py::test_lstm_layer holds the resident kernels to - the same arithmetic:
output 2e-5, dx 5e-5 max(1, |ref|max), every parameter gradient 1e-4 max(1, |ref|max).
"""
import functools

import numpy as np
import torch

# (B, T, D_in, h, bidirectional)
SHAPES = [(3, 5, 12, 129, True),        # first width past the resident limit; h % 4 != 0: clamped units, unaligned 16-byte row starts
          (17, 7, 8, 256, True),        # full width; two row tiles, the second one clamped
          (2, 1, 5, 200, False),        # T = 1: no prefetch, no previous step
          (33, 40, 20, 250, False),     # duplicated ownership positions, three row tiles, a longer chain
          (64, 100, 16, 256, True)]     # the trunk's own length: error growth over 100 steps
# With T = 1 the recurrent product is h_0 W^T = 0 whatever the weights' arithmetic: the negative controls need a previous step.
CONTROL_SHAPES = [s for s in SHAPES if s[1] > 1]
OUT_BOUND, DX_BOUND, DP_BOUND = 2e-5, 5e-5, 1e-4
NAMES = ("w_ih", "w_hh", "b_ih", "b_hh")
DEFECTS = ("drop_lo", "dup_counted_twice", "swap_g_o", "tail_group_zero")


def make_case(shape):
    """Seeded inputs of one shape, drawn like test_lstm_layer's: x, P[direction][w_ih, w_hh, b_ih, b_hh], gy (fp32, CPU)."""
    B, T, Din, h, bid = shape
    g = torch.Generator().manual_seed(B + T + h)
    k = 1.0 / np.sqrt(h)
    nd = 2 if bid else 1
    sizes = [(4 * h, Din), (4 * h, h), (4 * h,), (4 * h,)]
    P = [[(torch.rand(s, generator=g) * 2 - 1) * k for s in sizes] for _ in range(nd)]
    x = torch.randn(B, T, Din, generator=g)
    gy = torch.randn(B, T, nd * h, generator=g)
    return x, P, gy


def _bf16(t):
    return t.to(torch.bfloat16).to(t.dtype)


def _split(t):
    hi = _bf16(t)
    return hi, _bf16(t - hi)


def _dup_units(h):
    """Units that a clamped ownership group repeats although a natural position already covers them (csrc lstm_counted)."""
    b0 = (h - 4) & ~3
    return list(range(h - 4, min(b0 + 4, h))) if h % 4 else []


def _tail_units(h):
    """Units only the clamped group covers: the last, partial group of four."""
    b0 = (h - 4) & ~3
    return list(range(b0 + 4, h))


def _recur_fwd(xproj, w_hh, reverse, dtype, split, defect=None):
    """xproj (B, T, 4h), w_hh (4h, h) -> y, gates, cells, hprev in forward-time layout.  ``split``: the kernels' three-product form."""
    B, T, G = xproj.shape
    h = G // 4
    hcur = torch.zeros(B, h, dtype=dtype)
    c = torch.zeros(B, h, dtype=dtype)
    y = torch.zeros(B, T, h, dtype=dtype)
    gates, cells, hprev = torch.zeros(B, T, G, dtype=dtype), torch.zeros(B, T, h, dtype=dtype), torch.zeros(B, T, h, dtype=dtype)
    if split:
        wh, wl = _split(w_hh)
        wht, wlt = wh.t().contiguous(), wl.t().contiguous()
    dup = _dup_units(h)
    for t in (range(T - 1, -1, -1) if reverse else range(T)):
        if split:
            hh, hl = _split(hcur)
            if defect == "drop_lo":
                p = hh @ wht
            else:
                p = (hh @ wlt + hl @ wht) + hh @ wht
            if defect == "dup_counted_twice" and dup:
                p = p + ((hh[:, dup] @ wlt[dup] + hl[:, dup] @ wht[dup]) + hh[:, dup] @ wht[dup])
        else:
            p = hcur @ w_hh.t()
        pre = xproj[:, t] + p
        i, f = torch.sigmoid(pre[:, :h]), torch.sigmoid(pre[:, h:2 * h])
        if defect == "swap_g_o":
            o, gg = torch.sigmoid(pre[:, 2 * h:3 * h]), torch.tanh(pre[:, 3 * h:])
        else:
            gg, o = torch.tanh(pre[:, 2 * h:3 * h]), torch.sigmoid(pre[:, 3 * h:])
        c = f * c + i * gg
        hn = o * torch.tanh(c)
        if defect == "tail_group_zero":
            hn = hn.clone()
            hn[:, _tail_units(h)] = 0
        hprev[:, t] = hcur
        gates[:, t] = torch.cat([i, f, gg, o], 1)
        cells[:, t] = c
        y[:, t] = hn
        hcur = hn
    return y, gates, cells, hprev


def _recur_bwd(gy, w_hh, gates, cells, reverse, dtype, split):
    """BPTT of _recur_fwd: grad_y (B, T, h) -> grad_xproj (B, T, 4h), walking the forward order backwards."""
    B, T, h = gy.shape
    gx = torch.zeros(B, T, 4 * h, dtype=dtype)
    dh_rec = torch.zeros(B, h, dtype=dtype)
    dc_next = torch.zeros(B, h, dtype=dtype)
    if split:
        wh, wl = _split(w_hh)
    order = list(range(T - 1, -1, -1) if reverse else range(T))
    for n in range(T - 1, -1, -1):
        t = order[n]
        i, f, gg, o = gates[:, t, :h], gates[:, t, h:2 * h], gates[:, t, 2 * h:3 * h], gates[:, t, 3 * h:]
        c_prev = cells[:, order[n - 1]] if n > 0 else torch.zeros(B, h, dtype=dtype)
        dh = gy[:, t] + dh_rec
        tc = torch.tanh(cells[:, t])
        dc = dc_next + dh * o * (1 - tc * tc)
        da = torch.cat([dc * gg * i * (1 - i), dc * c_prev * f * (1 - f), dc * i * (1 - gg * gg), dh * tc * o * (1 - o)], 1)
        dc_next = dc * f
        gx[:, t] = da
        if split:
            dah, dal = _split(da)
            dh_rec = (dah @ wl + dal @ wh) + dah @ wh
        else:
            dh_rec = da @ w_hh
    return gx


def _layer(shape, dtype, split, defect=None):
    x, P, gy = make_case(shape)
    B, T, Din, h, bid = shape
    x64 = x.double().reshape(B * T, Din)
    ys, dx, grads = [], torch.zeros(B * T, Din, dtype=torch.float64), []
    for d, (w_ih, w_hh, b_ih, b_hh) in enumerate(P):
        xproj = (x64 @ w_ih.double().t() + (b_ih.double() + b_hh.double())).reshape(B, T, 4 * h).to(dtype)
        y, gates, cells, hprev = _recur_fwd(xproj, w_hh.to(dtype), d == 1, dtype, split, defect)
        gx = _recur_bwd(gy[:, :, d * h:(d + 1) * h].to(dtype), w_hh.to(dtype), gates, cells, d == 1, dtype, split)
        gx64 = gx.double().reshape(B * T, 4 * h)
        ys.append(y)
        dx += gx64 @ w_ih.double()
        gb = gx64.sum(0)
        grads.append([gx64.t() @ x64, gx64.t() @ hprev.double().reshape(B * T, h), gb, gb])
    return torch.cat(ys, 2).double(), dx.reshape(B, T, Din), grads


@functools.lru_cache(maxsize=None)
def reference64(shape):
    """(y, dx, [direction][w_ih, w_hh, b_ih, b_hh gradients]) in float64.  Shared: read-only."""
    return _layer(shape, torch.float64, False)


def emulate(shape, defect=None):
    """The same in the kernels' arithmetic (module docstring)."""
    return _layer(shape, torch.float32, True, defect)


def maxerr(a, b):
    return float((a.double().cpu() - b.double().cpu()).abs().max())


def errors(got, shape):
    """[(name, error, bound)] of a (y, dx, grads) triple against reference64(shape), bounds as in the module docstring."""
    y, dx, grads = reference64(shape)
    out = [("y", maxerr(got[0], y), OUT_BOUND), ("dx", maxerr(got[1], dx), DX_BOUND * max(1.0, float(dx.abs().max())))]
    for d, (gd, wd) in enumerate(zip(got[2], grads)):
        for n, a, b in zip(NAMES, gd, wd):
            out.append(("%s[%d]" % (n, d), maxerr(a, b), DP_BOUND * max(1.0, float(b.abs().max()))))
    return out
