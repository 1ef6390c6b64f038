"""The decode queue's C symbols: exported, described in the ctypes binding, and they refuse a NULL context
or queue.  No compute calls here (no GPU on the CPU runner)."""
import ctypes
import os

from smallz4_amd import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QUEUE = ("sz4_dq_create", "sz4_dq_destroy", "sz4_dq_enqueue")


def test_queue_symbols_exported_and_described():
    lib = ctypes.CDLL(_native.LIB_PATH)
    for name in QUEUE:
        assert hasattr(lib, name), name
        assert name in _native.SIGNATURES, name
    res, args = _native.SIGNATURES["sz4_dq_create"]
    assert res is ctypes.c_int and len(args) == 4
    res, args = _native.SIGNATURES["sz4_dq_destroy"]
    assert res is None and len(args) == 1
    res, args = _native.SIGNATURES["sz4_dq_enqueue"]
    assert res is ctypes.c_int and len(args) == 10


def test_queue_calls_reject_null_context_and_queue():
    lib = _native.lib()
    q = ctypes.c_void_p(1)
    assert lib.sz4_dq_create(None, 16, 1 << 20, ctypes.byref(q)) == _native.SZ4_E_ARG
    assert q.value is None  # no handle comes back from a failed create
    assert lib.sz4_dq_create(None, 16, 1 << 20, None) == _native.SZ4_E_ARG
    # a null queue is refused before any table is looked at (the addresses are never used)
    t = ctypes.c_void_p(64)
    assert lib.sz4_dq_enqueue(None, t, t, t, t, None, 1, t, t, None) == _native.SZ4_E_ARG
    assert lib.sz4_dq_enqueue(None, None, None, None, None, None, 0, None, None, None) == _native.SZ4_E_ARG
    lib.sz4_dq_destroy(None)  # a no-op


def test_status_constants():
    want = {"SZ4_ITEM_OK": 0, "SZ4_ITEM_CORRUPT": 1, "SZ4_ITEM_CAPACITY": 2, "SZ4_ITEM_ARG": 3, "SZ4_ITEM_QUEUE": 4,
            "SZ4_ITEM_INTERNAL": 5}
    for name, value in want.items():
        assert getattr(_native, name) == value, name
    header = open(os.path.join(ROOT, "include", "smallz4_amd.h")).read()
    for name, value in want.items():
        assert f"#define {name}" in header
        assert int(header.split(f"#define {name}")[1].split()[0]) == value, name


def test_python_surface():
    import smallz4_amd
    assert hasattr(smallz4_amd.Compressor, "decode_queue")
    for name in ("enqueue", "tensor_tables", "close"):
        assert hasattr(smallz4_amd.DecodeQueue, name), name
    assert smallz4_amd.get_version() == "1.5"
