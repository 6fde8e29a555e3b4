"""``ops.TrunkMode`` without a GPU: the scope restores and nests, bad fields and values are refused, the five module variables the mode
replaced can be neither read nor assigned, and the mode in effect routes ``ops.linear``."""
import dataclasses

import pytest
import torch

import ruart_amd.layers as L
from ruart_amd import hip, ops

RETIRED = [(ops, "trunk_gemm"), (ops, "trunk_grad_gemm"), (ops, "defer_weight_grads"), (ops, "fuse_operand_masks"), (L, "fused_scorer_enabled")]


def test_scope_restores_on_exit_and_on_exception_and_nests():
    before = ops.trunk_mode()
    assert (before.gemm, before.grad_gemm, before.defer_dw) == ("x3", "x3", False) and before.backward_gemm == "x3"
    with ops.use_trunk_mode(gemm="fp32") as outer:
        assert ops.trunk_mode() is outer and outer == before.replace(gemm="fp32") and outer.backward_gemm == "fp32"
        with ops.use_trunk_mode(defer_dw=True, grad_gemm="x1") as inner:                  # changes apply to the mode in effect
            assert ops.trunk_mode() is inner and inner == outer.replace(defer_dw=True, grad_gemm="x1")
            assert inner.backward_gemm == "fp32"                                         # grad_gemm is the form under an x3 forward only
            with ops.use_trunk_mode(before, grad_gemm="x1") as given:                     # an explicit mode, with changes
                assert ops.trunk_mode() == before.replace(grad_gemm="x1") and given.backward_gemm == "x1"
            assert ops.trunk_mode() is inner
        assert ops.trunk_mode() is outer
    assert ops.trunk_mode() is before
    with pytest.raises(KeyError):
        with ops.use_trunk_mode(gemm="fp32", fused_scorer=False):
            raise KeyError("from the body")
    assert ops.trunk_mode() is before
    with pytest.raises(dataclasses.FrozenInstanceError):
        before.gemm = "fp32"


@pytest.mark.parametrize("changes", [{"gem": "x3"}, {"gemm": "x1"}, {"gemm": "bf16"}, {"grad_gemm": "fp32"}, {"defer_dw": 1}, {"fuse_masks": None},
                                     {"fused_scorer": "0"}, {"gemm": "fp32", "streams": 3}])
def test_bad_field_or_value_raises_value_error(changes):
    before = ops.trunk_mode()
    with pytest.raises(ValueError):
        with ops.use_trunk_mode(**changes):
            pass
    with pytest.raises(ValueError):
        before.replace(**changes)
    assert ops.trunk_mode() is before


@pytest.mark.parametrize("module,name", RETIRED, ids=[n for _, n in RETIRED])
def test_retired_module_variables_raise_on_read_and_on_write(module, name):
    with pytest.raises(AttributeError, match="use_trunk_mode"):
        getattr(module, name)
    with pytest.raises(AttributeError, match="use_trunk_mode"):
        setattr(module, name, "fp32")
    assert name not in vars(module) and not hasattr(module, name)                         # no dead attribute was created
    # what the modules do hold can still be replaced (the tests wrap ops.mm, layers keeps the reference's dropout state)
    real = ops.mm
    ops.mm = real
    L.set_dropout_prob(L.dropout_p)


def test_linear_follows_the_mode_in_effect():
    g = torch.Generator().manual_seed(0)
    x, w, b = torch.randn(2, 5, 8, generator=g), torch.randn(3, 8, generator=g), torch.randn(3, generator=g)
    with ops.use_trunk_mode(gemm="fp32"):
        assert torch.equal(ops.linear(x, w, b), torch.nn.functional.linear(x, w, b))
    with pytest.raises(hip.HipError):                                                     # the default has no CPU path
        ops.linear(x, w, b)
