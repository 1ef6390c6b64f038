"""smallz4_amd -- LZ4 optimal-parse compression (smallz4 semantics) on MI355X.

Python mirror of the reference's public interface (reference smallz4.h:38-80):

    smallz4_amd.lz4(data, max_chain_length=65535, dictionary=b"", use_legacy_format=False)
        == bytes the reference's smallz4::lz4(...) emits for `data`
    smallz4_amd.ShortChainsGreedy / ShortChainsLazy / get_version()

plus the data-parallel entry point the GPU is built for:

    Compressor().compress_blocks(data, block_size=65536, max_chain_length=65535)
        -> frame whose every block equals smallz4's output for that block alone
    Compressor().compress_batch(items, max_chain_length=65535) / unlz4_batch(blocks)
        -> many separate buffers of different sizes, one independently decodable LZ4 block each
    Compressor().compress_batch_typed(items, elem_sizes) / unlz4_batch_typed(blocks, elem_sizes)
    Compressor().compress_tensor(t) / decompress_tensor(ct)
        -> the same for items of fixed-width elements, split into byte planes (planes.py) on the way;
           filters="bits" / filter="bits" shuffles them into bit planes instead (planes.bit_split)
    Compressor().decode_queue(max_items, max_src_bytes) -> DecodeQueue.enqueue(...) / tensor_tables(ct, out)
        -> the batch decoders as an enqueue over device tables: no host synchronisation, graph-capturable
    Compressor().compress_queue(sizes, elems, max_chain_length) -> CompressQueue.enqueue(...) / tensor_tables(t)
        -> the typed batch compressor as an enqueue for a fixed set of item sizes, graph-capturable as well
    Compressor().compress_queue_sized(capacities, elems, max_chain_length) -> SizedCompressQueue.enqueue(...)
        -> the same with the item sizes read from a device table at every enqueue, up to fixed capacities

All compression runs in the HIP library smallz4_amd/lib/libsmallz4_amd.so; there
is no CPU fallback.
"""
from __future__ import annotations

import ctypes
import dataclasses

from . import _native

ShortChainsGreedy = 3   # smallz4.h:77
ShortChainsLazy = 6     # smallz4.h:79
MaxChainLength = 65535  # smallz4.h:115 ("-9")

# per-stage device timings reported by sz4_last_stage_ms (include/smallz4_amd.h)
STAGES = ("runs", "sort", "find_sorted", "find_long", "parse", "assemble")

# the per-item filters of the filtered batch calls (SZ4_FILTER_* in include/smallz4_amd.h)
FILTERS = {"bytes": _native.SZ4_FILTER_BYTES, "bits": _native.SZ4_FILTER_BITS}

HEADERS = {"smallz4": _native.SZ4_HEADER_SMALLZ4, "independent": _native.SZ4_HEADER_INDEPENDENT,
           "none": _native.SZ4_HEADER_NONE}


def get_version() -> str:
    return _native.lib().sz4_version().decode()


def level_to_chain(level: int) -> int:
    """CLI level -0..-9 -> maxChainLength (smallz4.cpp:175, 232-239)."""
    if not 0 <= level <= 9:
        raise ValueError("level must be 0..9")
    return 65535 if level == 9 else level


@dataclasses.dataclass
class CompressedTensor:
    """What compress_tensor returns: typed blocks on the device (no serialised format)."""
    blocks: object       # device uint8 tensor: the bare LZ4 blocks, back to back
    offsets: list        # chunk i is blocks[offsets[i]:offsets[i + 1]]
    dtype: object        # the tensor's torch dtype (its element size is every chunk's width)
    shape: tuple
    chunk_bytes: int     # bytes of the tensor per chunk (the last chunk holds the rest)
    filter: str = "bytes"  # every chunk's filter: "bytes" (planes.split) or "bits" (planes.bit_split)

    @property
    def nbytes(self) -> int:
        return int(self.offsets[-1])


@dataclasses.dataclass
class DecodeTables:
    """The device tables of one enqueue (DecodeQueue.tensor_tables builds them for a CompressedTensor)."""
    src_ptrs: object     # int64: where every block starts
    src_sizes: object    # int32: its bytes, size word included
    dst_ptrs: object     # int64: where it decodes to
    dst_caps: object     # int32: the room there
    elems: object        # uint8: element width per item (or None: every width 1)
    out_sizes: object    # int32, written by the enqueue: decoded bytes per item
    status: object       # int32, written by the enqueue: SZ4_ITEM_* per item
    count: int
    keep: tuple = ()     # the tensors the pointers point into


class DecodeQueue:
    """An enqueue-only batch decoder (sz4_dq_*): device tables in, per-item sizes and statuses out on the
    device, no host synchronisation -- an enqueue can be captured in a graph (torch.cuda.graph) and replayed
    after the tables were rewritten.  Holds its scratch until close(); close it before its Compressor, and
    after every graph captured from it is gone."""

    def __init__(self, comp: "Compressor", max_items: int, max_src_bytes: int):
        self._comp = comp
        self._lib = comp._lib
        self.device = comp.device
        self.max_items, self.max_src_bytes = int(max_items), int(max_src_bytes)
        h = ctypes.c_void_p()
        comp._check(self._lib.sz4_dq_create(comp._h, self.max_items, self.max_src_bytes, ctypes.byref(h)), "sz4_dq_create")
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            if self._comp._h:  # a closed Compressor has released the scratch already
                self._lib.sz4_dq_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @staticmethod
    def _table(t, dtype, count, name):
        # shape and type only: nothing here reads a tensor's contents
        if t.dtype != dtype or not t.is_cuda or not t.is_contiguous() or t.numel() < count:
            raise TypeError(f"{name} must be a contiguous device tensor of {dtype} with at least {count} entries")
        return ctypes.c_void_p(t.data_ptr())

    def enqueue(self, src_ptrs, src_sizes, dst_ptrs, dst_caps, out_sizes, status, elems=None, count=None, stream=None):
        """Item i, the bare block of src_sizes[i] bytes at address src_ptrs[i], decodes to address dst_ptrs[i]
        (room dst_caps[i]) as an item of width elems[i]; out_sizes[i] and status[i] (SZ4_ITEM_*) receive the
        result when the stream gets there (see sz4_dq_enqueue).  Device tensors: int64 pointers, int32 sizes,
        capacities, results and statuses, uint8 widths.  stream: a raw HIP stream (default: torch's current one)."""
        import torch
        if count is None:
            count = src_ptrs.numel()
        count = int(count)
        if stream is None:
            stream = torch.cuda.current_stream(self.device).cuda_stream
        rc = self._lib.sz4_dq_enqueue(
            self._h, self._table(src_ptrs, torch.int64, count, "src_ptrs"), self._table(src_sizes, torch.int32, count, "src_sizes"),
            self._table(dst_ptrs, torch.int64, count, "dst_ptrs"), self._table(dst_caps, torch.int32, count, "dst_caps"),
            None if elems is None else self._table(elems, torch.uint8, count, "elems"), count,
            self._table(out_sizes, torch.int32, count, "out_sizes"), self._table(status, torch.int32, count, "status"),
            ctypes.c_void_p(stream))
        if rc != _native.SZ4_OK:
            raise _native.NativeError(f"sz4_dq_enqueue failed ({rc})")

    def enqueue_tables(self, t: DecodeTables, stream=None):
        self.enqueue(t.src_ptrs, t.src_sizes, t.dst_ptrs, t.dst_caps, t.out_sizes, t.status, t.elems, t.count, stream)

    def tensor_tables(self, ct: "CompressedTensor", out) -> DecodeTables:
        """The tables that decode `ct` into the preallocated tensor `out` (ct's dtype and shape, contiguous, on
        the device), built once: chunk pointers cut from ct.blocks and from out, every width the dtype's.
        Enqueue them, or replay a captured enqueue, any number of times."""
        import torch
        if getattr(ct, "filter", "bytes") != "bytes":
            raise ValueError("the decode queue merges byte planes only: decode a filter='bits' tensor with decompress_tensor")
        dev = torch.device("cuda", self.device)
        if out.dtype != ct.dtype or tuple(out.shape) != tuple(ct.shape) or not out.is_contiguous() or out.device != dev:
            raise TypeError("out must be a contiguous device tensor of the compressed tensor's dtype and shape")
        if not ct.blocks.is_cuda or ct.blocks.device != dev:
            raise TypeError("ct.blocks must be on the queue's device")
        e = out.element_size()
        n = out.numel() * e
        count = len(ct.offsets) - 1
        if count != (n + ct.chunk_bytes - 1) // ct.chunk_bytes:
            raise ValueError("the compressed tensor's chunks do not cover its shape")
        caps = [min(ct.chunk_bytes, n - k * ct.chunk_bytes) for k in range(count)]
        src, dst = ct.blocks.data_ptr(), out.data_ptr()

        def table(values, dtype):
            return torch.tensor(values, dtype=dtype).to(dev) if values else torch.empty(0, dtype=dtype, device=dev)

        return DecodeTables(
            table([src + int(ct.offsets[k]) for k in range(count)], torch.int64),
            table([int(ct.offsets[k + 1]) - int(ct.offsets[k]) for k in range(count)], torch.int32),
            table([dst + k * ct.chunk_bytes for k in range(count)], torch.int64), table(caps, torch.int32),
            table([e] * count, torch.uint8), torch.zeros(count, dtype=torch.int32, device=dev),
            torch.zeros(count, dtype=torch.int32, device=dev), count, (ct.blocks, out))


class CompressQueue:
    """An enqueue-only batch compressor (sz4_cq_*): the item count, sizes, widths and level are fixed here; the
    sources come from a device table of pointers, the blocks go to one output buffer and their addresses, sizes
    and statuses to device tables, with no host synchronisation -- an enqueue can be captured in a graph
    (torch.cuda.graph) and replayed after the pointer table or the data was rewritten.  block_ptrs and
    block_sizes are a DecodeQueue's src_ptrs and src_sizes.  Holds its scratch (about 50 bytes per staged byte)
    until close(); close it before its Compressor, and after every graph captured from it is gone."""

    _create = "sz4_cq_create"

    def __init__(self, comp: "Compressor", sizes, elems=None, max_chain_length: int = MaxChainLength):
        self._comp = comp
        self._lib = comp._lib
        self.device = comp.device
        self.sizes = [int(x) for x in sizes]
        self.elems = None if elems is None else [int(x) for x in elems]
        self.count = len(self.sizes)
        if self.elems is not None and len(self.elems) != self.count:
            raise ValueError("sizes and elems differ in length")
        if any(not 0 <= x < 1 << 32 for x in self.sizes):
            raise ValueError("an item size is not a uint32")
        z = (ctypes.c_uint32 * max(self.count, 1))(*self.sizes)
        w = None
        if self.elems is not None:
            w = (ctypes.c_uint8 * max(self.count, 1))(*[x & 0xFF if 0 <= x < 256 else 0 for x in self.elems])
        h = ctypes.c_void_p()
        comp._check(getattr(self._lib, self._create)(comp._h, z, w, self.count, int(max_chain_length), ctypes.byref(h)),
                    self._create)
        self._h = h
        self.bound = int(self._lib.sz4_cq_bound(h))

    def close(self):
        if getattr(self, "_h", None):
            if self._comp._h:  # a closed Compressor has released the scratch already
                self._lib.sz4_cq_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def enqueue(self, src_ptrs, out, block_ptrs, block_sizes, status, total=None, stream=None):
        """Item i, sizes[i] bytes of width elems[i] at address src_ptrs[i], is compressed into `out` (a uint8
        device tensor of at least `bound` bytes); block_ptrs[i], block_sizes[i] and status[i] (SZ4_ITEM_*) and
        total[0] receive the result when the stream gets there (see sz4_cq_enqueue).  Device tensors: int64
        pointers and total, int32 sizes and statuses.  stream: a raw HIP stream (default: torch's current one)."""
        import torch
        table = DecodeQueue._table
        if stream is None:
            stream = torch.cuda.current_stream(self.device).cuda_stream
        rc = self._lib.sz4_cq_enqueue(
            self._h, table(src_ptrs, torch.int64, self.count, "src_ptrs"), table(out, torch.uint8, 0, "out"), out.numel(),
            table(block_ptrs, torch.int64, self.count, "block_ptrs"), table(block_sizes, torch.int32, self.count, "block_sizes"),
            table(status, torch.int32, self.count, "status"), None if total is None else table(total, torch.int64, 1, "total"),
            ctypes.c_void_p(stream))
        if rc != _native.SZ4_OK:
            raise _native.NativeError(f"sz4_cq_enqueue failed ({rc})")

    def tensor_tables(self, t):
        """The source pointer table (int64, on the device) for the contiguous device tensor `t` cut into the
        queue's items in order: sum(sizes) must be t's bytes.  The table points into t, which the caller
        keeps alive and may rewrite in place between enqueues."""
        import torch
        dev = torch.device("cuda", self.device)
        if not t.is_contiguous() or t.device != dev:
            raise TypeError("t must be a contiguous tensor on the queue's device")
        if t.numel() * t.element_size() != sum(self.sizes):
            raise ValueError("the queue's items do not cover the tensor")
        ptrs, at = [], t.data_ptr()
        for n in self.sizes:
            ptrs.append(at)
            at += n
        return torch.tensor(ptrs, dtype=torch.int64).to(dev)


class SizedCompressQueue(CompressQueue):
    """A CompressQueue whose item sizes are read from a device table at every enqueue (sz4_cq_create_sized /
    sz4_cq_enqueue_sized): what is fixed here is every item's CAPACITY, the largest size it may have.  Item i
    of an enqueue has src_sizes[i] bytes: 0 gives an empty item, more than capacities[i] an empty item with
    status SZ4_ITEM_CAPACITY.  The scratch and the launches are those of the capacities, whatever the sizes.
    close / __del__ as on CompressQueue."""

    _create = "sz4_cq_create_sized"

    def __init__(self, comp: "Compressor", capacities, elems=None, max_chain_length: int = MaxChainLength):
        super().__init__(comp, capacities, elems, max_chain_length)
        self.capacities = self.sizes
        del self.sizes  # an enqueue's sizes are its src_sizes table

    def enqueue(self, src_ptrs, src_sizes, out, block_ptrs, block_sizes, status, total=None, stream=None):
        """As CompressQueue.enqueue, with src_sizes: an int32 device tensor of this enqueue's item sizes, read
        when the stream gets there (see sz4_cq_enqueue_sized)."""
        import torch
        table = DecodeQueue._table
        if stream is None:
            stream = torch.cuda.current_stream(self.device).cuda_stream
        rc = self._lib.sz4_cq_enqueue_sized(
            self._h, table(src_ptrs, torch.int64, self.count, "src_ptrs"), table(src_sizes, torch.int32, self.count, "src_sizes"),
            table(out, torch.uint8, 0, "out"), out.numel(),
            table(block_ptrs, torch.int64, self.count, "block_ptrs"), table(block_sizes, torch.int32, self.count, "block_sizes"),
            table(status, torch.int32, self.count, "status"), None if total is None else table(total, torch.int64, 1, "total"),
            ctypes.c_void_p(stream))
        if rc != _native.SZ4_OK:
            raise _native.NativeError(f"sz4_cq_enqueue_sized failed ({rc})")

    def tensor_tables(self, t):
        """(src_ptrs, src_sizes) for the contiguous device tensor `t` cut at the capacities in order
        (sum(capacities) must be t's bytes): the int64 pointer table, and an int32 size table preset to the
        capacities, which the caller -- or a kernel of its own -- rewrites between enqueues."""
        import torch
        dev = torch.device("cuda", self.device)
        if not t.is_contiguous() or t.device != dev:
            raise TypeError("t must be a contiguous tensor on the queue's device")
        if t.numel() * t.element_size() != sum(self.capacities):
            raise ValueError("the queue's capacities do not cover the tensor")
        ptrs, at = [], t.data_ptr()
        for n in self.capacities:
            ptrs.append(at)
            at += n
        return torch.tensor(ptrs, dtype=torch.int64).to(dev), torch.tensor(self.capacities, dtype=torch.int32).to(dev)


class Compressor:
    """A device context (HBM scratch stays allocated between calls)."""

    def __init__(self, device: int = 0, reserve_bytes: int = 0):
        self._lib = _native.lib()
        h = ctypes.c_void_p()
        rc = self._lib.sz4_create(ctypes.byref(h), device, reserve_bytes)
        if rc != _native.SZ4_OK:
            raise _native.NativeError(f"sz4_create failed ({rc}): no usable HIP device {device}")
        self._h = h
        self.device = device

    def close(self):
        if getattr(self, "_h", None):
            self._lib.sz4_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc: int, what: str):
        if rc != _native.SZ4_OK:
            msg = self._lib.sz4_last_error(self._h).decode()
            raise _native.NativeError(f"{what} failed ({rc}): {msg}")

    # -- reference entry point ------------------------------------------------------------------
    def lz4(self, data: bytes, max_chain_length: int = MaxChainLength, dictionary: bytes = b"",
            use_legacy_format: bool = False) -> bytes:
        """Byte-identical to smallz4::lz4 (smallz4.h:47-64) on the same input."""
        data = bytes(data)
        cap = self._lib.sz4_lz4_bound(len(data), int(use_legacy_format))
        out = ctypes.create_string_buffer(cap)
        size = ctypes.c_uint64()
        dic = bytes(dictionary)
        rc = self._lib.sz4_lz4(self._h, data, len(data), int(max_chain_length), dic if dic else None, len(dic),
                               int(use_legacy_format), out, cap, ctypes.byref(size))
        self._check(rc, "sz4_lz4")
        return out.raw[:size.value]

    def lz4_into(self, src, dst, max_chain_length: int = MaxChainLength, dictionary: bytes = b"",
                 use_legacy_format: bool = False) -> int:
        """sz4_lz4 between caller-owned host buffers (numpy uint8 arrays, no Python copies): compresses
        src into dst (at least sz4_lz4_bound(len(src)) bytes) and returns the frame length."""
        import numpy as np
        if isinstance(src, np.ndarray):
            src = np.ascontiguousarray(src, dtype=np.uint8)
        else:  # bytes-like: wrapped without a copy (read-only is fine, the library only reads it)
            src = np.frombuffer(memoryview(src).cast("B"), dtype=np.uint8)
        if not (isinstance(dst, np.ndarray) and dst.dtype == np.uint8 and dst.flags.c_contiguous):
            raise TypeError("dst must be a contiguous numpy uint8 array")
        size = ctypes.c_uint64()
        dic = bytes(dictionary)
        rc = self._lib.sz4_lz4(self._h, ctypes.c_void_p(src.ctypes.data), src.size, int(max_chain_length),
                               dic if dic else None, len(dic), int(use_legacy_format),
                               ctypes.c_void_p(dst.ctypes.data), dst.size, ctypes.byref(size))
        self._check(rc, "sz4_lz4")
        return size.value

    def lz4_stream(self, read, write, max_chain_length: int = MaxChainLength, dictionary: bytes = b"",
                   use_legacy_format: bool = False) -> None:
        """smallz4::lz4 over callbacks (sz4_lz4_stream): read(n) -> bytes (b"" at the end), write(bytes).
        Bounded memory: the input is compressed chunk by chunk (set_stream_chunk)."""
        err = []

        def get(data, n, _user):
            try:
                b = read(n)
            except BaseException as e:  # noqa: BLE001 -- re-raised after the call
                err.append(e)
                return 0
            if b is None:
                return 0
            if len(b) > n:
                # the native buffer holds n bytes: more is a caller error, not a silent overrun
                err.append(ValueError(f"read({n}) returned {len(b)} bytes"))
                return 0
            if b:
                ctypes.memmove(data, b, len(b))
            return len(b)

        def send(data, n, _user):
            try:
                write(ctypes.string_at(data, n) if n else b"")
            except BaseException as e:  # noqa: BLE001
                err.append(e)

        g, s = _native.GET_BYTES(get), _native.SEND_BYTES(send)
        dic = bytes(dictionary)
        rc = self._lib.sz4_lz4_stream(self._h, g, s, int(max_chain_length), dic if dic else None, len(dic),
                                      int(use_legacy_format), None)
        if err:
            raise err[0]
        self._check(rc, "sz4_lz4_stream")

    def set_stream_chunk(self, nbytes: int):
        """Input bytes per chunk of the stream paths (whole blocks; 0 = default 64 MiB)."""
        self._lib.sz4_set_stream_chunk(self._h, int(nbytes))

    def set_batch_chunk(self, nbytes: int):
        """Input bytes per internal piece of compress_blocks(_device) (whole blocks; 0 = default 448 MiB)."""
        self._lib.sz4_set_batch_chunk(self._h, int(nbytes))

    # -- data-parallel entry point --------------------------------------------------------------
    def compress_blocks_device(self, d_in: int, n: int, d_out: int, out_cap: int, block_size: int = 65536,
                               max_chain_length: int = MaxChainLength, header: str = "smallz4",
                               stream: int = 0) -> int:
        """Device pointers in, frame size out (see sz4_compress_blocks_device)."""
        size = ctypes.c_uint64()
        rc = self._lib.sz4_compress_blocks_device(self._h, ctypes.c_void_p(d_in), n, block_size, int(max_chain_length),
                                                  HEADERS[header], ctypes.c_void_p(d_out), out_cap,
                                                  ctypes.byref(size), ctypes.c_void_p(stream))
        self._check(rc, "sz4_compress_blocks_device")
        return size.value

    def compress_blocks(self, data, block_size: int = 65536, max_chain_length: int = MaxChainLength,
                        header: str = "smallz4") -> bytes:
        """Host bytes (or a uint8 torch tensor on the GPU) in, frame bytes out."""
        import torch
        if isinstance(data, torch.Tensor):
            t = data.contiguous().view(torch.uint8).reshape(-1)
            if not t.is_cuda:
                t = t.cuda(self.device)
        else:
            raw = bytes(data)
            t = torch.frombuffer(bytearray(raw), dtype=torch.uint8) if raw else torch.empty(0, dtype=torch.uint8)
            t = t.cuda(self.device)
        n = t.numel()
        cap = self._lib.sz4_bound(n, block_size)
        out = torch.empty(max(cap, 16), dtype=torch.uint8, device=t.device)
        stream = torch.cuda.current_stream(t.device).cuda_stream
        size = self.compress_blocks_device(t.data_ptr() if n else out.data_ptr(), n, out.data_ptr(), cap,
                                           block_size, max_chain_length, header, stream)
        return out[:size].cpu().numpy().tobytes()

    # -- ragged batch: many separate buffers, one LZ4 block each ---------------------------------
    def compress_batch_device(self, ptrs, sizes, d_out: int, out_cap: int, max_chain_length: int = MaxChainLength,
                              stream: int = 0) -> list[int]:
        """Device pointers and sizes of the items in, the blocks' offsets in d_out (len(sizes) + 1) out
        (see sz4_compress_batch_device): item i is d_out[off[i]:off[i + 1]], empty for an empty item."""
        count = len(sizes)
        if len(ptrs) != count:
            raise ValueError("ptrs and sizes differ in length")
        p = (ctypes.c_void_p * max(count, 1))(*[int(x) or None for x in ptrs])
        z = (ctypes.c_uint32 * max(count, 1))(*[int(x) for x in sizes])
        off = (ctypes.c_uint64 * (count + 1))()
        rc = self._lib.sz4_compress_batch_device(self._h, p, z, count, int(max_chain_length), ctypes.c_void_p(d_out),
                                                 out_cap, off, ctypes.c_void_p(stream))
        self._check(rc, "sz4_compress_batch_device")
        return list(off)

    def batch_bound(self, sizes) -> int:
        """Worst-case output bytes of compress_batch_device for these item sizes (sz4_batch_bound)."""
        z = (ctypes.c_uint32 * max(len(sizes), 1))(*[int(x) for x in sizes])
        return int(self._lib.sz4_batch_bound(z, len(sizes)))

    def unlz4_batch_device(self, d_blocks: int, offsets, d_out: int, out_cap: int, stream: int = 0) -> list[int]:
        """Bare blocks d_blocks[offsets[i]:offsets[i + 1]] in, each decoded on its own into d_out; returns
        the output offsets (see sz4_unlz4_batch_device).  d_out = 0, out_cap = 0 queries the offsets."""
        count = len(offsets) - 1
        if count < 0:
            raise ValueError("offsets needs count + 1 entries")
        o = (ctypes.c_uint64 * (count + 1))(*[int(x) for x in offsets])
        res = (ctypes.c_uint64 * (count + 1))()
        rc = self._lib.sz4_unlz4_batch_device(self._h, ctypes.c_void_p(d_blocks), o, count, ctypes.c_void_p(d_out), out_cap,
                                              res, ctypes.c_void_p(stream))
        if not (rc == _native.SZ4_E_CAPACITY and not d_out and not out_cap):
            self._check(rc, "sz4_unlz4_batch_device")
        return list(res)

    def compress_batch(self, items, max_chain_length: int = MaxChainLength) -> list[bytes]:
        """Every item (bytes-like, or a uint8 torch tensor) compressed as one LZ4 block on its own:
        [oz_block(item) for item in items], in one call.  A device tensor is used in place, whatever its
        storage offset; host items go up in one transfer."""
        import torch
        dev = torch.device("cuda", self.device)
        views = [None] * len(items)
        host = []
        for i, it in enumerate(items):
            if isinstance(it, torch.Tensor):
                if it.dtype != torch.uint8:
                    raise TypeError("tensor items must be uint8")
                t = it.reshape(-1) if it.is_contiguous() else it.contiguous().reshape(-1)
                views[i] = t if t.is_cuda and t.device == dev else t.to(dev)
            else:
                host.append((i, memoryview(it).cast("B")))
        if host:
            joined = bytearray().join(m for _, m in host)
            up = (torch.frombuffer(joined, dtype=torch.uint8).to(dev) if joined
                  else torch.empty(0, dtype=torch.uint8, device=dev))
            at = 0
            for i, m in host:
                views[i] = up[at:at + len(m)]
                at += len(m)
        sizes = [v.numel() for v in views]
        cap = self.batch_bound(sizes)
        out = torch.empty(max(cap, 16), dtype=torch.uint8, device=dev)
        stream = torch.cuda.current_stream(dev).cuda_stream
        off = self.compress_batch_device([v.data_ptr() if n else 0 for v, n in zip(views, sizes)], sizes,
                                         out.data_ptr(), cap, max_chain_length, stream)
        raw = out[:off[-1]].cpu().numpy().tobytes()
        return [raw[off[i]:off[i + 1]] for i in range(len(sizes))]

    def unlz4_batch(self, blocks) -> list[bytes]:
        """The reverse of compress_batch: every bare block (size word + payload, b"" for an empty item)
        decoded on its own, as the reference decoder reads a frame holding that block alone."""
        import torch
        dev = torch.device("cuda", self.device)
        blocks = [bytes(b) for b in blocks]
        offsets = [0]
        for b in blocks:
            offsets.append(offsets[-1] + len(b))
        joined = bytearray().join(blocks)
        d = (torch.frombuffer(joined, dtype=torch.uint8).to(dev) if joined
             else torch.empty(16, dtype=torch.uint8, device=dev))
        stream = torch.cuda.current_stream(dev).cuda_stream
        sizes = self.unlz4_batch_device(d.data_ptr(), offsets, 0, 0, stream)
        out = torch.empty(max(sizes[-1], 16), dtype=torch.uint8, device=dev)
        off = self.unlz4_batch_device(d.data_ptr(), offsets, out.data_ptr(), sizes[-1], stream)
        raw = out[:off[-1]].cpu().numpy().tobytes()
        return [raw[off[i]:off[i + 1]] for i in range(len(blocks))]

    def last_gather_ms(self) -> float:
        """Device time of the last compress_batch_device call's gather kernels (with set_timing on)."""
        return float(self._lib.sz4_last_gather_ms(self._h))

    # -- typed ragged batch: items of fixed-width elements, split into byte planes (planes.py) ------
    def compress_batch_typed_device(self, ptrs, sizes, elems, d_out: int, out_cap: int,
                                    max_chain_length: int = MaxChainLength, stream: int = 0) -> list[int]:
        """compress_batch_device with item i split by its element width elems[i] (1, 2, 4 or 8) while it is
        staged: block i is oz_block(planes.split(item i, elems[i])) (see sz4_compress_batch_typed_device)."""
        count = len(sizes)
        if len(ptrs) != count or len(elems) != count:
            raise ValueError("ptrs, sizes and elems differ in length")
        p = (ctypes.c_void_p * max(count, 1))(*[int(x) or None for x in ptrs])
        z = (ctypes.c_uint32 * max(count, 1))(*[int(x) for x in sizes])
        w = (ctypes.c_uint8 * max(count, 1))(*[int(x) & 0xFF if 0 <= int(x) < 256 else 0 for x in elems])
        off = (ctypes.c_uint64 * (count + 1))()
        rc = self._lib.sz4_compress_batch_typed_device(self._h, p, z, w, count, int(max_chain_length),
                                                       ctypes.c_void_p(d_out), out_cap, off, ctypes.c_void_p(stream))
        self._check(rc, "sz4_compress_batch_typed_device")
        return list(off)

    def unlz4_batch_typed_device(self, d_blocks: int, offsets, elems, d_out: int, out_cap: int,
                                 stream: int = 0) -> list[int]:
        """unlz4_batch_device with item i merged by elems[i] on its way to d_out, which then holds the
        original items (see sz4_unlz4_batch_typed_device).  d_out = 0, out_cap = 0 queries the offsets."""
        count = len(offsets) - 1
        if count < 0:
            raise ValueError("offsets needs count + 1 entries")
        if len(elems) != count:
            raise ValueError("offsets and elems differ in length")
        o = (ctypes.c_uint64 * (count + 1))(*[int(x) for x in offsets])
        w = (ctypes.c_uint8 * max(count, 1))(*[int(x) & 0xFF if 0 <= int(x) < 256 else 0 for x in elems])
        res = (ctypes.c_uint64 * (count + 1))()
        rc = self._lib.sz4_unlz4_batch_typed_device(self._h, ctypes.c_void_p(d_blocks), o, w, count, ctypes.c_void_p(d_out),
                                                    out_cap, res, ctypes.c_void_p(stream))
        if not (rc == _native.SZ4_E_CAPACITY and not d_out and not out_cap):
            self._check(rc, "sz4_unlz4_batch_typed_device")
        return list(res)

    # -- filtered ragged batch: the bit-plane shuffle (planes.bit_split) beside the byte-plane split --
    def compress_batch_filtered_device(self, ptrs, sizes, elems, filters, d_out: int, out_cap: int,
                                       max_chain_length: int = MaxChainLength, stream: int = 0) -> list[int]:
        """compress_batch_typed_device with a filter per item (SZ4_FILTER_BYTES / SZ4_FILTER_BITS, or None for
        the typed call): a BITS item's block is oz_block(planes.bit_split(item i, elems[i])) (see
        sz4_compress_batch_filtered_device)."""
        count = len(sizes)
        if len(ptrs) != count or len(elems) != count or (filters is not None and len(filters) != count):
            raise ValueError("ptrs, sizes, elems and filters differ in length")
        p = (ctypes.c_void_p * max(count, 1))(*[int(x) or None for x in ptrs])
        z = (ctypes.c_uint32 * max(count, 1))(*[int(x) for x in sizes])
        w = (ctypes.c_uint8 * max(count, 1))(*[int(x) & 0xFF if 0 <= int(x) < 256 else 0 for x in elems])
        f = None if filters is None else (ctypes.c_uint8 * max(count, 1))(*[int(x) if 0 <= int(x) < 256 else 255 for x in filters])
        off = (ctypes.c_uint64 * (count + 1))()
        rc = self._lib.sz4_compress_batch_filtered_device(self._h, p, z, w, f, count, int(max_chain_length),
                                                          ctypes.c_void_p(d_out), out_cap, off, ctypes.c_void_p(stream))
        self._check(rc, "sz4_compress_batch_filtered_device")
        return list(off)

    def unlz4_batch_filtered_device(self, d_blocks: int, offsets, elems, filters, d_out: int, out_cap: int,
                                    stream: int = 0) -> list[int]:
        """unlz4_batch_typed_device with a filter per item (as above): a BITS item passes through
        planes.bit_merge on its way to d_out (see sz4_unlz4_batch_filtered_device)."""
        count = len(offsets) - 1
        if count < 0:
            raise ValueError("offsets needs count + 1 entries")
        if len(elems) != count or (filters is not None and len(filters) != count):
            raise ValueError("offsets, elems and filters differ in length")
        o = (ctypes.c_uint64 * (count + 1))(*[int(x) for x in offsets])
        w = (ctypes.c_uint8 * max(count, 1))(*[int(x) & 0xFF if 0 <= int(x) < 256 else 0 for x in elems])
        f = None if filters is None else (ctypes.c_uint8 * max(count, 1))(*[int(x) if 0 <= int(x) < 256 else 255 for x in filters])
        res = (ctypes.c_uint64 * (count + 1))()
        rc = self._lib.sz4_unlz4_batch_filtered_device(self._h, ctypes.c_void_p(d_blocks), o, w, f, count,
                                                       ctypes.c_void_p(d_out), out_cap, res, ctypes.c_void_p(stream))
        if not (rc == _native.SZ4_E_CAPACITY and not d_out and not out_cap):
            self._check(rc, "sz4_unlz4_batch_filtered_device")
        return list(res)

    @staticmethod
    def _filters(filters, count):
        """"bytes" / "bits" per item, or one string for all -> SZ4_FILTER_* per item; None stays None."""
        if filters is None:
            return None
        if isinstance(filters, str):
            filters = [filters] * count
        if len(filters) != count:
            raise ValueError("items and filters differ in length")
        for f in filters:
            if f not in FILTERS:
                raise ValueError(f"filter {f!r} is not 'bytes' or 'bits'")
        return [FILTERS[f] for f in filters]

    def compress_batch_typed(self, items, elem_sizes=None, max_chain_length: int = MaxChainLength, filters=None) -> list[bytes]:
        """compress_batch for typed items: [oz_block(planes.split(item, E)) for item in items].  A torch tensor
        of any dtype is taken as its bytes with E = its element size (1, 2, 4 or 8; any other: TypeError);
        a bytes-like needs its width in elem_sizes (one entry per item; None for a tensor = its dtype's).
        filters: "bytes" or "bits" per item, or one string for all; a "bits" item's block is
        oz_block(planes.bit_split(item, E))."""
        import torch
        dev = torch.device("cuda", self.device)
        if elem_sizes is not None and len(elem_sizes) != len(items):
            raise ValueError("items and elem_sizes differ in length")
        views, elems = [], []
        for i, it in enumerate(items):
            e = elem_sizes[i] if elem_sizes is not None else None
            if isinstance(it, torch.Tensor):
                e = it.element_size() if e is None else e
                t = it.to(dev).contiguous().reshape(-1).view(torch.uint8)
            else:
                if e is None:
                    raise TypeError("a bytes-like item needs its element width in elem_sizes")
                m = memoryview(it).cast("B")
                t = (torch.frombuffer(bytearray(m), dtype=torch.uint8).to(dev) if len(m)
                     else torch.empty(0, dtype=torch.uint8, device=dev))
            if e not in (1, 2, 4, 8):
                raise TypeError(f"element width {e} is not 1, 2, 4 or 8")
            views.append(t)
            elems.append(e)
        sizes = [v.numel() for v in views]
        cap = self.batch_bound(sizes)
        out = torch.empty(max(cap, 16), dtype=torch.uint8, device=dev)
        stream = torch.cuda.current_stream(dev).cuda_stream
        ptrs = [v.data_ptr() if n else 0 for v, n in zip(views, sizes)]
        if filters is None:
            off = self.compress_batch_typed_device(ptrs, sizes, elems, out.data_ptr(), cap, max_chain_length, stream)
        else:
            off = self.compress_batch_filtered_device(ptrs, sizes, elems, self._filters(filters, len(sizes)), out.data_ptr(),
                                                      cap, max_chain_length, stream)
        raw = out[:off[-1]].cpu().numpy().tobytes()
        return [raw[off[i]:off[i + 1]] for i in range(len(sizes))]

    def unlz4_batch_typed(self, blocks, elem_sizes, filters=None) -> list[bytes]:
        """The reverse of compress_batch_typed: every bare block decoded on its own and merged by its width
        (and its filter, given as there)."""
        import torch
        dev = torch.device("cuda", self.device)
        blocks = [bytes(b) for b in blocks]
        filters = self._filters(filters, len(blocks))
        offsets = [0]
        for b in blocks:
            offsets.append(offsets[-1] + len(b))
        joined = bytearray().join(blocks)
        d = (torch.frombuffer(joined, dtype=torch.uint8).to(dev) if joined
             else torch.empty(16, dtype=torch.uint8, device=dev))
        stream = torch.cuda.current_stream(dev).cuda_stream

        def decode(d_out, cap):
            if filters is None:
                return self.unlz4_batch_typed_device(d.data_ptr(), offsets, elem_sizes, d_out, cap, stream)
            return self.unlz4_batch_filtered_device(d.data_ptr(), offsets, elem_sizes, filters, d_out, cap, stream)

        sizes = decode(0, 0)
        out = torch.empty(max(sizes[-1], 16), dtype=torch.uint8, device=dev)
        off = decode(out.data_ptr(), sizes[-1])
        raw = out[:off[-1]].cpu().numpy().tobytes()
        return [raw[off[i]:off[i + 1]] for i in range(len(blocks))]

    def compress_tensor(self, t, chunk_bytes: int = 65536, max_chain_length: int = MaxChainLength,
                        filter: str = "bytes") -> "CompressedTensor":
        """A tensor as typed blocks of chunk_bytes each (the last one shorter), all of width t.element_size()
        and of one filter ("bytes": the byte-plane split; "bits": the bit-plane shuffle).
        The tensor is made contiguous and cut by pointer: its payload is not copied, and the blocks stay on
        the device -- only their offsets come to the host."""
        import torch
        dev = torch.device("cuda", self.device)
        e = t.element_size()
        if e not in (1, 2, 4, 8):
            raise TypeError(f"element width {e} is not 1, 2, 4 or 8")
        if not 0 < chunk_bytes <= 4 << 20 or chunk_bytes % e:
            raise ValueError("chunk_bytes must be a multiple of the element size, at most 4 MiB")
        if filter not in FILTERS:
            raise ValueError(f"filter {filter!r} is not 'bytes' or 'bits'")
        flat = t.detach().to(dev).contiguous().reshape(-1).view(torch.uint8)
        n = flat.numel()
        sizes = [min(chunk_bytes, n - o) for o in range(0, n, chunk_bytes)]
        base = flat.data_ptr()
        cap = self.batch_bound(sizes)
        out = torch.empty(max(cap, 16), dtype=torch.uint8, device=dev)
        stream = torch.cuda.current_stream(dev).cuda_stream
        ptrs = [base + k * chunk_bytes for k in range(len(sizes))]
        if filter == "bytes":
            off = self.compress_batch_typed_device(ptrs, sizes, [e] * len(sizes), out.data_ptr(), cap, max_chain_length, stream)
        else:
            off = self.compress_batch_filtered_device(ptrs, sizes, [e] * len(sizes), [FILTERS[filter]] * len(sizes),
                                                      out.data_ptr(), cap, max_chain_length, stream)
        return CompressedTensor(out[:off[-1]].clone(), off, t.dtype, tuple(t.shape), chunk_bytes, filter)

    def decompress_tensor(self, ct: "CompressedTensor"):
        """The tensor compress_tensor took, on the device, in its dtype and shape."""
        import torch
        dev = torch.device("cuda", self.device)
        e = torch.empty(0, dtype=ct.dtype).element_size()
        n = e
        for d in ct.shape:
            n *= d
        blocks = ct.blocks.to(dev)
        out = torch.empty(n, dtype=torch.uint8, device=dev)
        stream = torch.cuda.current_stream(dev).cuda_stream
        count = len(ct.offsets) - 1
        if ct.filter == "bytes":
            off = self.unlz4_batch_typed_device(blocks.data_ptr(), ct.offsets, [e] * count, out.data_ptr(), n, stream)
        else:
            off = self.unlz4_batch_filtered_device(blocks.data_ptr(), ct.offsets, [e] * count,
                                                   self._filters(ct.filter, count), out.data_ptr(), n, stream)
        if off[-1] != n:
            raise _native.NativeError(f"the blocks decode to {off[-1]} bytes, the tensor has {n}")
        return out.view(ct.dtype).reshape(ct.shape)

    def decode_queue(self, max_items: int, max_src_bytes: int) -> "DecodeQueue":
        """An enqueue-only batch decoder for up to max_items items of max_src_bytes of blocks in all per
        enqueue (sz4_dq_create); its scratch counts as this context's until the queue is closed."""
        return DecodeQueue(self, max_items, max_src_bytes)

    def compress_queue(self, sizes, elems=None, max_chain_length: int = MaxChainLength) -> "CompressQueue":
        """An enqueue-only batch compressor for items of these sizes and element widths (None: every width 1)
        at this level (0 or 7 .. 65535) (sz4_cq_create); its scratch counts as this context's until the queue
        is closed."""
        return CompressQueue(self, sizes, elems, max_chain_length)

    def compress_queue_sized(self, capacities, elems=None, max_chain_length: int = MaxChainLength) -> "SizedCompressQueue":
        """An enqueue-only batch compressor whose item sizes come from a device table at every enqueue, each up
        to its capacity (sz4_cq_create_sized); otherwise as compress_queue."""
        return SizedCompressQueue(self, capacities, elems, max_chain_length)

    def last_merge_ms(self) -> float:
        """Device time of the last unlz4_batch_typed_device call's merge kernel (with set_timing on)."""
        return float(self._lib.sz4_last_merge_ms(self._h))

    # -- decoder: the reference's smallz4cat -----------------------------------------------------
    def unlz4(self, frame: bytes, dictionary: bytes = b"") -> bytes:
        """smallz4cat's unlz4 (smallz4cat.c:112-360) on the GPU: the bytes `frame` decodes to.
        Raises NativeError for a frame the reference decoder rejects."""
        frame, dic = bytes(frame), bytes(dictionary)
        size = ctypes.c_uint64()
        rc = self._lib.sz4_unlz4(self._h, frame, len(frame), dic or None, len(dic), None, 0, ctypes.byref(size))
        if rc == _native.SZ4_OK:
            return b""
        if rc != _native.SZ4_E_CAPACITY:
            self._check(rc, "sz4_unlz4")
        out = ctypes.create_string_buffer(size.value)
        rc = self._lib.sz4_unlz4(self._h, frame, len(frame), dic or None, len(dic), out, size.value, ctypes.byref(size))
        self._check(rc, "sz4_unlz4")
        return out.raw[:size.value]

    def unlz4_stream(self, read_byte, write, dictionary: bytes = b"") -> None:
        """smallz4cat's unlz4_userPtr over callbacks (sz4_unlz4_stream): read_byte() -> int,
        write(bytes) -- called with 64 KiB pieces and the remainder, as the reference flushes."""
        err = []

        def get(_user):
            try:
                return read_byte()
            except BaseException as e:  # noqa: BLE001
                err.append(e)
                return 0

        def send(data, n, _user):
            try:
                write(ctypes.string_at(data, n) if n else b"")
            except BaseException as e:  # noqa: BLE001
                err.append(e)

        g, s = _native.GET_BYTE(get), _native.SEND_OUT(send)
        dic = bytes(dictionary)
        rc = self._lib.sz4_unlz4_stream(self._h, g, s, dic if dic else None, len(dic), None)
        if err:
            raise err[0]
        self._check(rc, "sz4_unlz4_stream")

    def unlz4_device(self, d_frame: int, n: int, d_out: int, out_cap: int, d_dict: int = 0, dict_len: int = 0,
                     stream: int = 0) -> int:
        """Device pointers in, decoded size out (see sz4_unlz4_device); raises when out_cap is too small."""
        size = ctypes.c_uint64()
        rc = self._lib.sz4_unlz4_device(self._h, ctypes.c_void_p(d_frame), n, ctypes.c_void_p(d_dict), dict_len,
                                        ctypes.c_void_p(d_out), out_cap, ctypes.byref(size), ctypes.c_void_p(stream))
        self._check(rc, "sz4_unlz4_device")
        return size.value

    def last_block_sizes(self, nblocks: int) -> list[int]:
        arr = (ctypes.c_uint32 * max(nblocks, 1))()
        k = self._lib.sz4_last_block_sizes(self._h, arr, nblocks)
        if k < 0:
            raise _native.NativeError("sz4_last_block_sizes failed")
        return list(arr[:k])

    def debug_stop_after(self, stage: int):
        self._lib.sz4_debug_stop_after(self._h, int(stage))

    def debug_matches(self, n: int, parse_input: bool = False):
        """Per-position (length, distance) of the last call (sz4_debug_matches); parse_input=True: always
        the match arrays the parse was given, never its choices (sz4_debug_parse_input)."""
        import numpy as np
        ln = np.zeros(n, dtype=np.uint32)
        ds = np.zeros(n, dtype=np.uint16)
        name = "sz4_debug_parse_input" if parse_input else "sz4_debug_matches"
        self._check(getattr(self._lib, name)(self._h, ln.ctypes.data, ds.ctypes.data, n), name)
        return ln, ds

    def debug_memory(self) -> dict:
        """The accounting's diagnostics (sz4_debug_memory): buffer growths and injected allocation failures
        since the context was created, and the last blocks or batch call's piece retries and smallest piece."""
        arr = (ctypes.c_uint64 * 4)()
        self._check(self._lib.sz4_debug_memory(self._h, arr), "sz4_debug_memory")
        return dict(zip(("growths", "injected", "retries", "min_piece"), (int(x) for x in arr)))

    def last_error(self) -> str:
        """The message of the last call's error ("" when it had none) (sz4_last_error)."""
        return self._lib.sz4_last_error(self._h).decode()

    def device_bytes(self) -> int:
        """Device memory held by this context (scratch, staging, output buffers)."""
        return int(self._lib.sz4_device_bytes(self._h))

    def trim(self):
        """Release every device and pinned host buffer this context holds (sz4_trim)."""
        self._lib.sz4_trim(self._h)

    def set_device_limit(self, nbytes: int):
        """Bound this context's device memory (sz4_set_device_limit; 0 = no bound)."""
        self._lib.sz4_set_device_limit(self._h, int(nbytes))

    def released_buffers(self) -> int:
        """Buffers released so far under the device bound or memory pressure (sz4_released_buffers)."""
        return int(self._lib.sz4_released_buffers(self._h))

    def dict_rounds(self) -> int:
        """Dictionary mode: match-finder rounds of the last chunk (sz4_dict_rounds; 0xFFFFFFFF: the
        chunk fell back to the in-order replay)."""
        return int(self._lib.sz4_dict_rounds(self._h))

    def unlz4_resolve_passes(self) -> int:
        """Longest reference chain (hops) the last split-mode decode followed while packing its output
        (0: decoded block by block, or no byte referred to another sub-segment)."""
        return int(self._lib.sz4_unlz4_resolve_passes(self._h))

    def unlz4_index_parallel(self) -> bool:
        """Whether the last decode's block index came from the parallel index (not the serial walk)."""
        return bool(self._lib.sz4_unlz4_index_parallel(self._h))

    def set_timing(self, on: bool):
        self._lib.sz4_set_timing(self._h, int(on))

    def last_stage_ms(self) -> dict:
        arr = (ctypes.c_float * len(STAGES))()
        self._lib.sz4_last_stage_ms(self._h, arr, len(STAGES))
        return dict(zip(STAGES, list(arr)))


_default = None


def _ctx() -> Compressor:
    global _default
    if _default is None:
        _default = Compressor()
    return _default


def lz4(data: bytes, max_chain_length: int = MaxChainLength, dictionary: bytes = b"",
        use_legacy_format: bool = False) -> bytes:
    """smallz4::lz4 (smallz4.h:47-64) on the GPU."""
    return _ctx().lz4(data, max_chain_length, dictionary, use_legacy_format)


def compress_blocks(data, block_size: int = 65536, max_chain_length: int = MaxChainLength,
                    header: str = "smallz4") -> bytes:
    return _ctx().compress_blocks(data, block_size, max_chain_length, header)


def unlz4(frame: bytes, dictionary: bytes = b"") -> bytes:
    """smallz4cat's decoder (smallz4cat.c:112-360) on the GPU."""
    return _ctx().unlz4(frame, dictionary)


def compress_batch(items, max_chain_length: int = MaxChainLength) -> list[bytes]:
    """Every item compressed as one LZ4 block on its own (Compressor.compress_batch)."""
    return _ctx().compress_batch(items, max_chain_length)


def unlz4_batch(blocks) -> list[bytes]:
    """Every bare block decoded on its own (Compressor.unlz4_batch)."""
    return _ctx().unlz4_batch(blocks)


def compress_batch_typed(items, elem_sizes=None, max_chain_length: int = MaxChainLength, filters=None) -> list[bytes]:
    """Every item split into its byte planes (or, with filters, shuffled into its bit planes) and compressed as
    one LZ4 block (Compressor.compress_batch_typed)."""
    return _ctx().compress_batch_typed(items, elem_sizes, max_chain_length, filters)


def unlz4_batch_typed(blocks, elem_sizes, filters=None) -> list[bytes]:
    """Every bare block decoded on its own and merged by its width and filter (Compressor.unlz4_batch_typed)."""
    return _ctx().unlz4_batch_typed(blocks, elem_sizes, filters)


def compress_tensor(t, chunk_bytes: int = 65536, max_chain_length: int = MaxChainLength,
                    filter: str = "bytes") -> CompressedTensor:
    """A tensor as typed blocks on the device (Compressor.compress_tensor)."""
    return _ctx().compress_tensor(t, chunk_bytes, max_chain_length, filter)


def decompress_tensor(ct: CompressedTensor):
    """The tensor compress_tensor took, on the device (Compressor.decompress_tensor)."""
    return _ctx().decompress_tensor(ct)
