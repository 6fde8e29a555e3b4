"""C ABI of the persistent LSTM recurrence (ruart_lstm_ws_bytes / ruart_lstm_fwd / _bwd, one entry pair for every hidden size): declared,
bound, exported; the workspace size; and the argument checks, which run before anything is launched and therefore need no device."""
import ctypes
import os
import re

from ruart_amd import hip, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ruart_lstm_ws_bytes", "ruart_lstm_fwd", "ruart_lstm_bwd")
REMOVED = tuple(n.replace("ruart_lstm_", "ruart_lstm_wide_") for n in NAMES)      # the streamed route's former entry set
INVALID = 1          # hipErrorInvalidValue


def ws_bytes(h, ndir=2):
    n = ctypes.c_size_t(0)
    rc = hip.load().ruart_lstm_ws_bytes(h, ndir, ctypes.byref(n))
    return rc, n.value


def test_the_three_symbols_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "ruart_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    lib = hip.load()
    for name in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in hip.exported_symbols() and hasattr(lib, name), name
        assert hasattr(hip.kernels(), name)
    for name in REMOVED:
        assert not re.search(r"\b%s\b" % name, header), name
        assert name not in hip.exported_symbols(), name
        assert name not in hip._SIGNATURES, name
    assert hip._SIGNATURES["ruart_lstm_fwd"][1][-2] is ctypes.c_size_t and hip._SIGNATURES["ruart_lstm_bwd"][1][-2] is ctypes.c_size_t


def test_workspace_size_is_zero_when_resident_then_positive_and_monotone():
    for h in range(1, 129):
        assert ws_bytes(h, 2) == (0, 0) and ws_bytes(h, 1) == (0, 0), h
    last = 0
    for h in range(129, 257):
        rc, n = ws_bytes(h, 2)
        assert rc == 0 and n > 0, h
        assert n >= last, h
        last = n
        rc1, n1 = ws_bytes(h, 1)
        assert rc1 == 0 and 0 < n1 <= n, h
    # the bf16 hi / lo image of both directions at full width: 2 x 4 x 256 x 256 x 4 bytes
    assert ws_bytes(256, 2) == (0, 2 * 4 * 256 * 256 * 4)
    assert ws_bytes(144, 2)[1] < ws_bytes(256, 2)[1]


def test_workspace_size_rejects_what_the_kernels_do_not_take():
    for h, ndir in ((0, 1), (257, 2), (200, 0), (200, 3), (125, 0), (125, 3)):
        assert ws_bytes(h, ndir)[0] == INVALID, (h, ndir)
    assert hip.load().ruart_lstm_ws_bytes(200, 2, None) == INVALID
    assert hip.load().ruart_lstm_ws_bytes(125, 2, None) == INVALID


def test_python_routing_constant_matches_the_library():
    """StackedBRNN routes by ops.LSTM_MAX_HIDDEN; the library's own limit must be the same number."""
    assert ws_bytes(ops.LSTM_MAX_HIDDEN, 2)[0] == 0
    assert ws_bytes(ops.LSTM_MAX_HIDDEN + 1, 2)[0] == INVALID


def test_argument_errors_return_invalid_value_before_any_launch():
    """No device here: a call that got as far as a launch would fail with another code (or crash on the fake pointers)."""
    lib = hip.load()
    p = ctypes.c_void_p(4096)          # never dereferenced on the host, never launched with
    big = 1 << 22

    def fwd(B=2, T=3, h=200, ndir=2, ws=p, n=big, ptrs=(p, p, p)):
        return lib.ruart_lstm_fwd(*ptrs, None, None, None, B, T, h, ndir, ws, n, None)

    def bwd(B=2, T=3, h=200, ndir=2, ws=p, n=big, ptrs=(p, p, p, p, p)):
        return lib.ruart_lstm_bwd(*ptrs, B, T, h, ndir, ws, n, None)

    def each_null(k):
        return [dict(ptrs=tuple(None if i == j else p for i in range(k))) for j in range(k)]

    need = ws_bytes(200, 2)[1]
    assert ws_bytes(128, 2) == ws_bytes(125, 2) == ws_bytes(3, 1) == (0, 0)      # valid widths of the one pair now: no workspace
    for call, k in ((fwd, 3), (bwd, 5)):
        # streamed widths: the sizes, the workspace, each required pointer
        for bad in [dict(h=257), dict(h=0), dict(ndir=0), dict(ndir=3), dict(B=0), dict(B=-1), dict(T=0),
                    dict(ws=None), dict(n=need - 1), dict(n=0)] + each_null(k):
            assert call(**bad) == INVALID, (call.__name__, bad)
        # resident widths, no workspace given: the same checks, before the device is touched
        for h in (125, 128, 3):
            for bad in [dict(B=0), dict(B=-1), dict(T=0), dict(ndir=0), dict(ndir=3)] + each_null(k):
                assert call(h=h, ws=None, n=0, **bad) == INVALID, (call.__name__, h, bad)
        # the first width that needs a workspace is refused without one
        assert call(h=129, ws=None, n=0) == INVALID, call.__name__
        assert call(h=129, ws=None, n=big) == INVALID, call.__name__
