"""The byte-plane split of typed items, stated in numpy (host side; the device does it inside the batch
gather and after the batch decoder, see include/smallz4_amd.h).

An item of n bytes holding elements of width E has m = n // E whole elements and t = n % E tail bytes:

    split[k * m + e] = item[e * E + k]      0 <= k < E, 0 <= e < m
    split[E * m + j] = item[E * m + j]      0 <= j < t       (the tail, unchanged, after the planes)

E = 1 and n < E are the identity; merge is the inverse.  A block written by compress_batch_typed is an
ordinary LZ4 block of split(item, E): any LZ4 decoder followed by merge(..., E) reads it.
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
