"""The ragged batch API's C symbols: exported, described in the ctypes binding, and their pure parts
behave.  No compute calls here (no GPU on the CPU runner)."""
import ctypes

from smallz4_amd import _native

BATCH = ("sz4_batch_bound", "sz4_compress_batch_device", "sz4_unlz4_batch_device")


def test_batch_symbols_exported_and_described():
    lib = ctypes.CDLL(_native.LIB_PATH)
    for name in BATCH:
        assert hasattr(lib, name), name
        assert name in _native.SIGNATURES, name
    res, args = _native.SIGNATURES["sz4_compress_batch_device"]
    assert res is ctypes.c_int and len(args) == 9
    res, args = _native.SIGNATURES["sz4_unlz4_batch_device"]
    assert res is ctypes.c_int and len(args) == 8


def test_batch_bound():
    lib = _native.lib()
    sizes = (ctypes.c_uint32 * 3)(0, 1, 65536)
    assert lib.sz4_batch_bound(sizes, 3) == 65537 + 12
    assert lib.sz4_batch_bound(sizes, 0) == 0
    assert lib.sz4_batch_bound(None, 0) == 0
    big = (ctypes.c_uint32 * 2)(0xFFFFFFFF, 0xFFFFFFFF)  # summed in 64 bits
    assert lib.sz4_batch_bound(big, 2) == 2 * 0xFFFFFFFF + 8


def test_batch_calls_reject_null_context():
    lib = _native.lib()
    off = (ctypes.c_uint64 * 2)()
    ptrs = (ctypes.c_void_p * 1)()
    sizes = (ctypes.c_uint32 * 1)(0)
    assert lib.sz4_compress_batch_device(None, ptrs, sizes, 1, 9, None, 0, off, None) == -1
    assert lib.sz4_unlz4_batch_device(None, None, off, 1, None, 0, off, None) == -1
