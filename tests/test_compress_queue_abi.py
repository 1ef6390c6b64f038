"""The compress queue's C ABI and Python surface, without a GPU: the four sz4_cq_* symbols are exported and
described, null handles are refused before any device work, and the Python methods exist.  (That the header
declares exactly what the library exports is test_abi.py's check.)"""
import ctypes
import inspect

import smallz4_amd
from smallz4_amd import _native

ARITY = {"sz4_cq_create": 6, "sz4_cq_destroy": 1, "sz4_cq_bound": 1, "sz4_cq_enqueue": 9}


def test_symbols_are_exported_and_described():
    lib = ctypes.CDLL(_native.LIB_PATH)
    for name, arity in ARITY.items():
        assert hasattr(lib, name), name
        assert name in _native.SIGNATURES, name
        res, args = _native.SIGNATURES[name]
        assert len(args) == arity, name
    assert _native.SIGNATURES["sz4_cq_create"][0] is ctypes.c_int
    assert _native.SIGNATURES["sz4_cq_enqueue"][0] is ctypes.c_int
    assert _native.SIGNATURES["sz4_cq_bound"][0] is ctypes.c_uint64
    assert _native.SIGNATURES["sz4_cq_destroy"][0] is None


def test_null_handles_are_refused():
    lib = _native.lib()
    sizes = (ctypes.c_uint32 * 2)(100, 200)
    h = ctypes.c_void_p(0xDEAD)  # a failed create hands back no handle
    assert lib.sz4_cq_create(None, sizes, None, 2, 65535, ctypes.byref(h)) == _native.SZ4_E_ARG
    assert h.value is None
    assert lib.sz4_cq_create(None, sizes, None, 2, 65535, None) == _native.SZ4_E_ARG
    assert lib.sz4_cq_enqueue(None, None, None, 0, None, None, None, None, None) == _native.SZ4_E_ARG
    lib.sz4_cq_destroy(None)  # a no-op
    assert lib.sz4_cq_bound(None) == 0


def test_python_surface():
    assert callable(smallz4_amd.Compressor.compress_queue)
    params = list(inspect.signature(smallz4_amd.Compressor.compress_queue).parameters)
    assert params == ["self", "sizes", "elems", "max_chain_length"]
    q = smallz4_amd.CompressQueue
    for name in ("enqueue", "tensor_tables", "close", "__del__"):
        assert callable(getattr(q, name)), name
    params = list(inspect.signature(q.enqueue).parameters)
    assert params == ["self", "src_ptrs", "out", "block_ptrs", "block_sizes", "status", "total", "stream"]
