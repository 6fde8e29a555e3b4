"""The two typed handles of ruart_amd/hip.py on the one shared object: ``hip.kernels()`` (pointer arguments take the tensor itself, a
non-zero hipError_t raises) and ``hip.load()`` (the raw surface of the tests and tools: ``hip.ptr`` / ``hip.check`` by hand).  The CPU tests
call only entry points that launch nothing."""
import ast
import ctypes
import os

import pytest
import torch

from ruart_amd import hip, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "ruart_amd")


# ---- pointer conversion ---------------------------------------------------------------------------------------------------------
def test_tensor_argument_is_its_full_address():
    t = torch.arange(8, dtype=torch.float32)
    assert t.data_ptr() > 2 ** 32            # (a conversion through a 32-bit C int could not pass)
    p = hip.TensorPtr.from_param(t)
    assert isinstance(p, ctypes.c_void_p) and p.value == t.data_ptr()
    p = hip.TensorPtr.from_param(torch.nn.Parameter(t))
    assert isinstance(p, ctypes.c_void_p) and p.value == t.data_ptr()


def test_none_is_null():
    p = hip.TensorPtr.from_param(None)
    assert isinstance(p, ctypes.c_void_p) and p.value is None


def test_c_void_p_passes_through():
    p = hip.ptr(torch.zeros(4))
    assert hip.TensorPtr.from_param(p) is p
    s = ctypes.c_void_p(0x7F0012345678)
    assert hip.TensorPtr.from_param(s) is s


def test_int_round_trips():
    v = (1 << 40) + 0x1234
    p = hip.TensorPtr.from_param(v)
    assert isinstance(p, ctypes.c_void_p) and p.value == v


def test_host_buffers_of_ctypes_pass_as_before():
    """the profiling entry points fill host arrays (bench.py's timeline pass): a pointer argument still takes what c_void_p takes"""
    n = ctypes.c_int(-1)
    begin, end, flops = (ctypes.c_float * 4)(), (ctypes.c_float * 4)(), (ctypes.c_double * 4)()
    assert hip.load().ruart_prof_enable(0) == 0          # off, and the record count cleared: nothing another test left is read below
    for lib in (hip.load(), hip.kernels()):
        assert lib.ruart_prof_timeline(begin, end, flops, 4, ctypes.byref(n)) == 0 and n.value == 0      # nothing was recorded
    with pytest.raises(hip.HipError, match="ruart_prof_timeline"):
        hip.kernels().ruart_prof_timeline(begin, end, flops, 4, None)


def test_anything_else_is_refused():
    with pytest.raises(TypeError):
        hip.TensorPtr.from_param(1.5)
    with pytest.raises(TypeError):
        hip.TensorPtr.from_param([1, 2])


# ---- checked against raw --------------------------------------------------------------------------------------------------------
def test_checked_handle_raises_where_the_raw_one_returns_the_code():
    raw, chk = hip.load(), hip.kernels()
    assert raw.ruart_gemm_set_tile_order is not chk.ruart_gemm_set_tile_order
    # 65 is past the largest group (csrc/gemm.hip): refused before any global changes
    assert raw.ruart_gemm_set_tile_order(65) != 0
    with pytest.raises(hip.HipError, match="ruart_gemm_set_tile_order") as e:
        chk.ruart_gemm_set_tile_order(65)
    assert "hipError_t %d" % raw.ruart_gemm_set_tile_order(65) in str(e.value)
    # and a call that succeeds returns the zero on both
    out_r, out_c = (ctypes.c_int * 4)(), (ctypes.c_int * 4)()
    assert raw.ruart_f16c_shifts(out_r) == 0 and chk.ruart_f16c_shifts(out_c) == 0
    assert list(out_r) == list(out_c) == list(hip.f16c_shifts())


def test_handles_share_one_library():
    """One mapped object behind both handles: the same dlopen handle and the same address for a symbol, so the library's switches
    (globals of the shared object) are common to both."""
    raw, chk = hip.load(), hip.kernels()
    assert raw is not chk and raw._handle == chk._handle
    addr = lambda fn: ctypes.cast(fn, ctypes.c_void_p).value
    assert addr(raw.ruart_gemm_set_variant) == addr(chk.ruart_gemm_set_variant)


# ---- the unchecked set ----------------------------------------------------------------------------------------------------------
def test_unchecked_set():
    sig = hip._SIGNATURES
    assert hip._UNCHECKED <= set(sig)
    assert {n for n, (res, _) in sig.items() if res is not ctypes.c_int} <= hip._UNCHECKED
    chk, raw = hip.kernels(), hip.load()
    for name in sig:
        assert getattr(raw, name).errcheck is not hip._errcheck, name
        assert (getattr(chk, name).errcheck is hip._errcheck) == (name not in hip._UNCHECKED), name
    # the ints of the set are values: a count, a level, a previous state
    assert {n for n in hip._UNCHECKED if sig[n][0] is ctypes.c_int} == {"ruart_whole_ln_blocks", "ruart_stream_create_priority",
                                                                        "ruart_gemm_16c_set_dual"}


def test_size_function_through_both_handles():
    # a case of tests/test_cabi_sizes.py (M = 256 * 81, N = 768, K = 3072, 11 CUs: TAIL_WS_BYTES_16)
    args = (256 * 81, 768, 3072, 11)
    assert hip.kernels().ruart_gemm_16_tail_ws_bytes(*args) == hip.load().ruart_gemm_16_tail_ws_bytes(*args) == 2097152
    assert hip.kernels().ruart_whole_ln_blocks() == hip.load().ruart_whole_ln_blocks() > 0


# ---- no stragglers --------------------------------------------------------------------------------------------------------------
# product functions that keep the raw handle (hip.load) because they read the return code as a value
RAW_SITES = [("ops.py", "_dw_bf16")]          # a non-zero code selects the split-bf16 product
CHECK_SITES = []                                # hip.check( outside hip.py: none is left


def _hip_calls(attr):
    """(file, enclosing function) of every ``hip.<attr>(...)`` call in the package outside hip.py"""
    found = []
    for fn in sorted(os.listdir(PKG)):
        if not fn.endswith(".py") or fn == "hip.py":
            continue
        tree = ast.parse(open(os.path.join(PKG, fn)).read())

        def walk(node, scope):
            for ch in ast.iter_child_nodes(node):
                inner = ch.name if isinstance(ch, (ast.FunctionDef, ast.AsyncFunctionDef)) else scope
                if (isinstance(ch, ast.Call) and isinstance(ch.func, ast.Attribute) and ch.func.attr == attr
                        and isinstance(ch.func.value, ast.Name) and ch.func.value.id == "hip"):
                    found.append((fn, scope))
                walk(ch, inner)
        walk(tree, "<module>")
    return found


def test_product_modules_marshal_nothing_by_hand():
    for fn in sorted(os.listdir(PKG)):
        if fn.endswith(".py") and fn != "hip.py":
            text = open(os.path.join(PKG, fn)).read()
            assert "hip.ptr(" not in text, fn
            assert text.count("hip.check(") == sum(1 for f, _ in CHECK_SITES if f == fn), fn
    assert _hip_calls("ptr") == []
    assert sorted(_hip_calls("check")) == sorted(CHECK_SITES)
    assert sorted(_hip_calls("load")) == sorted(RAW_SITES)


# ---- one launch through each handle ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_colsum_through_both_handles():
    """ruart_colsum_f32 on (65, 8): the first row count at which ops.colsum takes the kernel.  Raw handle with hip.ptr / hip.check
    against the checked handle with the tensors themselves: the same bits, and x.sum(0) within the rounding of a 65-term fp32 sum
    (any order: (n - 1) 2^-24 sum |x_i|)."""
    dev = torch.device("cuda:0")
    rows, cols = 65, 8
    x = torch.randn(rows, cols, generator=torch.Generator().manual_seed(11)).to(dev)
    raw, chk = hip.load(), hip.kernels()
    n_ws = int(raw.ruart_colsum_f32_ws_floats(rows, cols))
    assert n_ws == int(chk.ruart_colsum_f32_ws_floats(rows, cols))
    ws_raw = torch.empty(max(n_ws, 1), dtype=torch.float32, device=dev)
    ws_chk = torch.empty(max(n_ws, 1), dtype=torch.float32, device=dev)
    out_raw = torch.full((cols,), float("nan"), dtype=torch.float32, device=dev)
    out_chk = torch.full((cols,), float("nan"), dtype=torch.float32, device=dev)
    st = hip.stream_ptr(dev)
    hip.check(raw.ruart_colsum_f32(hip.ptr(x), x.stride(0), rows, cols, hip.ptr(out_raw), 0, hip.ptr(ws_raw), st), "ruart_colsum_f32")
    assert chk.ruart_colsum_f32(x, x.stride(0), rows, cols, out_chk, 0, ws_chk, st) == 0
    torch.cuda.synchronize()
    assert torch.equal(out_raw, out_chk)
    x64 = x.double().cpu()
    bound = (rows - 1) * 2.0 ** -24 * x64.abs().sum(0)
    assert ((out_chk.double().cpu() - x64.sum(0)).abs() <= bound).all()
    assert torch.equal(out_chk, ops.colsum(x))
