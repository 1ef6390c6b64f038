"""The typed batch API's C symbols: exported, described in the ctypes binding, and they refuse a NULL
context.  No compute calls here (no GPU on the CPU runner)."""
import ctypes

from smallz4_amd import _native

TYPED = ("sz4_compress_batch_typed_device", "sz4_unlz4_batch_typed_device", "sz4_last_merge_ms")


def test_typed_symbols_exported_and_described():
    lib = ctypes.CDLL(_native.LIB_PATH)
    for name in TYPED:
        assert hasattr(lib, name), name
        assert name in _native.SIGNATURES, name
    res, args = _native.SIGNATURES["sz4_compress_batch_typed_device"]
    assert res is ctypes.c_int and len(args) == 10
    res, args = _native.SIGNATURES["sz4_unlz4_batch_typed_device"]
    assert res is ctypes.c_int and len(args) == 9
    res, args = _native.SIGNATURES["sz4_last_merge_ms"]
    assert res is ctypes.c_float and len(args) == 1


def test_typed_calls_reject_null_context():
    lib = _native.lib()
    off = (ctypes.c_uint64 * 2)()
    ptrs = (ctypes.c_void_p * 1)()
    sizes = (ctypes.c_uint32 * 1)(0)
    elems = (ctypes.c_uint8 * 1)(4)
    assert lib.sz4_compress_batch_typed_device(None, ptrs, sizes, elems, 1, 9, None, 0, off, None) == _native.SZ4_E_ARG
    assert lib.sz4_unlz4_batch_typed_device(None, None, off, elems, 1, None, 0, off, None) == _native.SZ4_E_ARG
    assert lib.sz4_last_merge_ms(None) == 0.0


def test_host_model_is_importable_without_a_gpu():
    from smallz4_amd import planes
    assert planes.merge(planes.split(b"0123456789", 4), 4) == b"0123456789"
