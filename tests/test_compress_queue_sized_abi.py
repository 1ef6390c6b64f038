"""The sized compress queue's C ABI and Python surface, without a GPU: sz4_cq_create_sized and
sz4_cq_enqueue_sized are exported and described, null handles and a null size table are refused before any
device work, and the Python methods exist.  (That the header declares exactly what the library exports is
test_abi.py's check.)"""
import ctypes
import inspect

import smallz4_amd
from smallz4_amd import _native

ARITY = {"sz4_cq_create_sized": 6, "sz4_cq_enqueue_sized": 10}


def test_symbols_are_exported_and_described():
    lib = ctypes.CDLL(_native.LIB_PATH)
    for name, arity in ARITY.items():
        assert hasattr(lib, name), name
        assert name in _native.SIGNATURES, name
        res, args = _native.SIGNATURES[name]
        assert len(args) == arity, name
        assert res is ctypes.c_int, name


def test_null_handles_and_a_null_size_table_are_refused():
    lib = _native.lib()
    caps = (ctypes.c_uint32 * 2)(100, 200)
    h = ctypes.c_void_p(0xDEAD)  # a failed create hands back no handle
    assert lib.sz4_cq_create_sized(None, caps, None, 2, 65535, ctypes.byref(h)) == _native.SZ4_E_ARG
    assert h.value is None
    assert lib.sz4_cq_create_sized(None, caps, None, 2, 65535, None) == _native.SZ4_E_ARG
    assert lib.sz4_cq_enqueue_sized(None, None, None, None, 0, None, None, None, None, None) == _native.SZ4_E_ARG
    # a size table alone does not make a null queue acceptable, and a null size table is refused whatever else
    # is passed (the queue is not looked at: any non-null value stands in for it)
    sizes = (ctypes.c_uint32 * 2)(1, 2)
    p = ctypes.cast(sizes, ctypes.c_void_p)
    assert lib.sz4_cq_enqueue_sized(None, p, p, p, 1 << 20, p, p, p, None, None) == _native.SZ4_E_ARG
    assert lib.sz4_cq_enqueue_sized(p, p, None, p, 1 << 20, p, p, p, None, None) == _native.SZ4_E_ARG


def test_python_surface():
    params = list(inspect.signature(smallz4_amd.Compressor.compress_queue_sized).parameters)
    assert params == ["self", "capacities", "elems", "max_chain_length"]
    assert inspect.signature(smallz4_amd.Compressor.compress_queue_sized).parameters["max_chain_length"].default == \
        smallz4_amd.MaxChainLength
    q = smallz4_amd.SizedCompressQueue
    for name in ("enqueue", "tensor_tables", "close", "__del__"):
        assert callable(getattr(q, name)), name
    params = list(inspect.signature(q.enqueue).parameters)
    assert params == ["self", "src_ptrs", "src_sizes", "out", "block_ptrs", "block_sizes", "status", "total", "stream"]
    assert list(inspect.signature(q.tensor_tables).parameters) == ["self", "t"]
    # the fixed queue keeps its signatures
    params = list(inspect.signature(smallz4_amd.CompressQueue.enqueue).parameters)
    assert params == ["self", "src_ptrs", "out", "block_ptrs", "block_sizes", "status", "total", "stream"]
