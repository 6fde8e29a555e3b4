"""C ABI of the streamed LSTM recurrence (ruart_lstm_wide_ws_bytes / _fwd / _bwd): declared, bound, exported; the workspace size; and the
argument checks, which run before anything is launched and therefore need no device."""
import ctypes
import os
import re

from ruart_amd import hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ruart_lstm_wide_ws_bytes", "ruart_lstm_wide_fwd", "ruart_lstm_wide_bwd")
INVALID = 1          # hipErrorInvalidValue


def ws_bytes(h, ndir=2, with_backward=1):
    n = ctypes.c_size_t(0)
    rc = hip.load().ruart_lstm_wide_ws_bytes(h, ndir, with_backward, ctypes.byref(n))
    return rc, n.value


def test_the_three_symbols_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "ruart_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    lib = hip.load()
    for name in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in hip.exported_symbols() and hasattr(lib, name), name
        assert hasattr(hip.kernels(), name)
    assert hip._SIGNATURES["ruart_lstm_wide_fwd"][1][-2] is ctypes.c_size_t and hip._SIGNATURES["ruart_lstm_wide_bwd"][1][-2] is ctypes.c_size_t


def test_workspace_size_is_positive_and_monotone():
    last = 0
    for h in range(129, 257):
        rc0, n0 = ws_bytes(h, 2, 0)
        rc1, n1 = ws_bytes(h, 2, 1)
        assert rc0 == 0 and rc1 == 0 and 0 < n0 <= n1, h
        assert n1 >= last, h
        last = n1
        assert ws_bytes(h, 1, 1)[1] <= n1
    # the bf16 hi / lo image of both directions at full width: 2 x 4 x 256 x 256 x 4 bytes
    assert ws_bytes(256, 2, 1) == (0, 2 * 4 * 256 * 256 * 4)
    assert ws_bytes(144, 2, 1)[1] < ws_bytes(256, 2, 1)[1]


def test_workspace_size_rejects_what_the_kernels_do_not_take():
    for h, ndir in ((128, 2), (257, 2), (3, 1), (0, 1), (200, 0), (200, 3)):
        assert ws_bytes(h, ndir)[0] == INVALID, (h, ndir)
    assert hip.load().ruart_lstm_wide_ws_bytes(200, 2, 1, None) == INVALID


def test_argument_errors_return_invalid_value_before_any_launch():
    """No device here: a call that got as far as a launch would fail with another code (or crash on the fake pointers)."""
    lib = hip.load()
    p = ctypes.c_void_p(4096)          # never dereferenced on the host, never launched with
    big = 1 << 22

    def fwd(B=2, T=3, h=200, ndir=2, ws=p, n=big):
        return lib.ruart_lstm_wide_fwd(p, p, p, None, None, None, B, T, h, ndir, ws, n, None)

    def bwd(B=2, T=3, h=200, ndir=2, ws=p, n=big):
        return lib.ruart_lstm_wide_bwd(p, p, p, p, p, B, T, h, ndir, ws, n, None)

    need = ws_bytes(200, 2)[1]
    for call in (fwd, bwd):
        for bad in (dict(h=128), dict(h=125), dict(h=257), dict(h=3), dict(ndir=0), dict(ndir=3), dict(B=0), dict(B=-1), dict(T=0),
                    dict(ws=None), dict(n=need - 1), dict(n=0)):
            assert call(**bad) == INVALID, (call.__name__, bad)
    # the resident pair keeps its contract: h > 128 is refused there
    assert lib.ruart_lstm_fwd(p, p, p, None, None, None, 2, 3, 129, 2, None) == INVALID
    assert lib.ruart_lstm_bwd(p, p, p, p, p, 2, 3, 129, 2, None) == INVALID
