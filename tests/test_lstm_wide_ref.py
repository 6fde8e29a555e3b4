"""The references test_gpu_lstm_wide.py measures the streamed LSTM kernels against, checked on the CPU (tests/_lstm_wide_ref.py): the
float64 restatement against torch's own LSTM and autograd, the fp32 emulation of the kernels' arithmetic inside the bounds, and four
emulated kernel defects outside them."""
import pytest
import torch

from tests import _lstm_wide_ref as R


def test_float64_restatement_matches_torch_lstm_and_autograd():
    """reference64 (explicit recurrence and BPTT) against nn.LSTM in float64 with autograd: output and every gradient to 1e-12 of
    max(1, |ref|) - float64 rounding over a 5-step chain."""
    shape = R.SHAPES[0]
    B, T, Din, h, bid = shape
    x, P, gy = R.make_case(shape)
    m = torch.nn.LSTM(Din, h, batch_first=True, bidirectional=bid).double()
    sd = {}
    for d, sfx in enumerate(["", "_reverse"][:len(P)]):
        for n, t in zip(("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0"), P[d]):
            sd[n + sfx] = t.double()
    m.load_state_dict(sd)
    xd = x.double().requires_grad_()
    yr = m(xd)[0]
    yr.backward(gy.double())
    y, dx, grads = R.reference64(shape)
    assert R.maxerr(y, yr.detach()) < 1e-12 and R.maxerr(dx, xd.grad) < 1e-12 * max(1.0, float(xd.grad.abs().max()))
    for d, sfx in enumerate(["", "_reverse"][:len(P)]):
        for n, g in zip(("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0"), grads[d]):
            want = getattr(m, n + sfx).grad
            assert R.maxerr(g, want) < 1e-12 * max(1.0, float(want.abs().max())), (d, n)


@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: "x".join(str(int(v)) for v in s))
def test_emulated_kernel_arithmetic_stays_inside_the_bounds(shape):
    """bf16 hi / lo split of W_hh and of h (forward) / da (backward), lo.hi + hi.lo + hi.hi with fp32 accumulation, against float64, at
    test_lstm_layer's bounds (output 2e-5, dx 5e-5 max(1, |ref|), parameter gradients 1e-4 max(1, |ref|)).
    Measured, output / dx / worst parameter gradient over its bound:
      (3, 5, 12, 129)    2.3e-07 / 5.2e-07 / 0.009       (17, 7, 8, 256)     1.3e-07 / 6.0e-07 / 0.007
      (2, 1, 5, 200)     9.1e-09 / 1.8e-08 / 0.002       (33, 40, 20, 250)   2.9e-07 / 6.4e-07 / 0.009
      (64, 100, 16, 256) 2.6e-07 / 8.5e-07 / 0.011
    The defects of the test below leave the output bound of 2e-5 by: lo terms dropped 8.7e-05 .. 1.5e-04, duplicate counted twice
    6.7e-03 / 7.3e-03, g and o swapped 0.24 .. 0.40, partial group zero 0.13 / 0.19."""
    errs = R.errors(R.emulate(shape), shape)
    print(shape, " ".join("%s %.2e/%.1e" % e for e in errs))
    for name, err, bound in errs:
        assert err < bound, (name, err, bound)


@pytest.mark.parametrize("shape", R.CONTROL_SHAPES, ids=lambda s: "x".join(str(int(v)) for v in s))
@pytest.mark.parametrize("defect", R.DEFECTS)
def test_emulated_defects_leave_the_output_bound(shape, defect):
    """Negative controls: the lo terms dropped, a duplicated ownership position counted twice (h = 250), gates g and o swapped, the last
    partial unit group left at zero (h = 129) - each must exceed the OUTPUT bound at every shape where the defect exists (T > 1: with
    one step the recurrent product is 0 . W; the duplicate and the partial group exist only where h % 4 != 0)."""
    h = shape[3]
    if defect in ("dup_counted_twice", "tail_group_zero") and h % 4 == 0:
        assert R._dup_units(h) == [] and R._tail_units(h) == []
        return
    if defect == "dup_counted_twice":
        assert h != 250 or R._dup_units(h) == [246, 247]
    if defect == "tail_group_zero":
        assert h != 129 or R._tail_units(h) == [128]
    err = R.maxerr(R.emulate(shape, defect)[0], R.reference64(shape)[0])
    print(shape, defect, "%.2e" % err)
    assert err > R.OUT_BOUND, (defect, err)
