"""The filtered batch entry points of the C ABI: exported, described by the binding, and refusing a NULL context.
No GPU."""
import ctypes

from smallz4_amd import _native

NAMES = ("sz4_compress_batch_filtered_device", "sz4_unlz4_batch_filtered_device")


def test_symbols_are_exported_and_described():
    lib = ctypes.CDLL(_native.LIB_PATH)
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in _native.SIGNATURES
    res, args = _native.SIGNATURES[NAMES[0]]
    assert res is ctypes.c_int and len(args) == 11
    res, args = _native.SIGNATURES[NAMES[1]]
    assert res is ctypes.c_int and len(args) == 10
    assert (_native.SZ4_FILTER_BYTES, _native.SZ4_FILTER_BITS) == (0, 1)


def test_null_context_is_refused():
    lib = _native.lib()
    off = (ctypes.c_uint64 * 2)()
    assert lib.sz4_compress_batch_filtered_device(None, None, None, None, None, 0, 7, None, 0, off, None) == _native.SZ4_E_ARG
    assert lib.sz4_unlz4_batch_filtered_device(None, None, off, None, None, 0, None, 0, off, None) == _native.SZ4_E_ARG
