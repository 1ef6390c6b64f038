"""The byte-plane split of typed items, stated in numpy (host side; the device does it inside the batch
gather and after the batch decoder, see include/smallz4_amd.h).

An item of n bytes holding elements of width E has m = n // E whole elements and t = n % E tail bytes:

    split[k * m + e] = item[e * E + k]      0 <= k < E, 0 <= e < m
    split[E * m + j] = item[E * m + j]      0 <= j < t       (the tail, unchanged, after the planes)

E = 1 and n < E are the identity; merge is the inverse.  A block written by compress_batch_typed is an
ordinary LZ4 block of split(item, E): any LZ4 decoder followed by merge(..., E) reads it.

The bit-plane shuffle (SZ4_FILTER_BITS, filters="bits") goes one step further.  Of the m whole elements the
first g = m - m % 8 are shuffled into 8 * E bit rows of G = g // 8 bytes each; bits are numbered from the least
significant:

    bit (e & 7) of shuf[(8 * k + b) * G + (e >> 3)] = bit b of item[e * E + k]     0 <= k < E, 0 <= b < 8, 0 <= e < g
    shuf[j] = item[j]                                                              g * E <= j < n

This is the byte-plane split of the first g elements followed by a bit transpose of every plane into its 8 bit
rows; the m % 8 left-over elements and the n % E tail bytes keep their place after the rows.  It changes no size,
is the identity for g = 0 (n < 8 * E), and E = 1 is meaningful (the bit rows of the bytes).  bit_merge is the
inverse.
"""
from __future__ import annotations

import numpy as np

WIDTHS = (1, 2, 4, 8)


def _check(elem: int) -> int:
    if elem not in WIDTHS:
        raise ValueError("element width must be 1, 2, 4 or 8")
    return int(elem)


def split(data, elem: int) -> bytes:
    """Byte k of every whole element together, plane after plane, then the tail bytes."""
    elem = _check(elem)
    a = np.frombuffer(bytes(data), dtype=np.uint8)
    m = len(a) // elem
    body = a[:m * elem].reshape(m, elem).T  # row k = plane k
    return body.tobytes() + a[m * elem:].tobytes()


def merge(data, elem: int) -> bytes:
    """The inverse of split."""
    elem = _check(elem)
    a = np.frombuffer(bytes(data), dtype=np.uint8)
    m = len(a) // elem
    body = a[:m * elem].reshape(elem, m).T  # row e = element e
    return body.tobytes() + a[m * elem:].tobytes()


def bit_split(data, elem: int) -> bytes:
    """Bit b of byte k of the first g elements together, row after row, then the left-over elements and the tail."""
    elem = _check(elem)
    a = np.frombuffer(bytes(data), dtype=np.uint8)
    g = len(a) // elem // 8 * 8
    bits = np.unpackbits(a[:g * elem].reshape(g, elem), axis=1, bitorder="little").reshape(g, elem, 8)  # [e, k, b]
    rows = np.packbits(bits.transpose(1, 2, 0), axis=2, bitorder="little")  # [k, b, e >> 3]
    return rows.tobytes() + a[g * elem:].tobytes()


def bit_merge(data, elem: int) -> bytes:
    """The inverse of bit_split."""
    elem = _check(elem)
    a = np.frombuffer(bytes(data), dtype=np.uint8)
    g = len(a) // elem // 8 * 8
    bits = np.unpackbits(a[:g * elem].reshape(elem, 8, g // 8), axis=2, bitorder="little")  # [k, b, e]
    body = np.packbits(bits.transpose(2, 0, 1), axis=2, bitorder="little")  # [e, k]
    return body.tobytes() + a[g * elem:].tobytes()
