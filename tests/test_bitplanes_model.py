"""The bit-plane shuffle in numpy (smallz4_amd/planes.py: bit_split, bit_merge) against its definition, and the
two oracle results the filter exists for.  No GPU."""
import numpy as np
import pytest

from oracle import pyoracle
from smallz4_amd import planes

WIDTHS = (1, 2, 4, 8)


def by_definition(item, E):
    """bit (e & 7) of shuf[(8k + b) * G + (e >> 3)] = bit b of item[e * E + k]; the rest keeps its place."""
    n = len(item)
    m = n // E
    g = m - m % 8
    G = g // 8
    out = bytearray(n)
    out[g * E:] = item[g * E:]
    for e in range(g):
        for k in range(E):
            for b in range(8):
                if (item[e * E + k] >> b) & 1:
                    out[(8 * k + b) * G + (e >> 3)] |= 1 << (e & 7)
    return bytes(out)


def some_bytes(n, seed):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


@pytest.mark.parametrize("E", WIDTHS)
def test_bit_split_is_the_definition(E):
    for n in range(301):
        x = some_bytes(n, 1000 * E + n)
        s = planes.bit_split(x, E)
        assert s == by_definition(x, E), (n, E)
        assert len(s) == n and planes.bit_merge(s, E) == x, (n, E)


@pytest.mark.parametrize("E", WIDTHS)
@pytest.mark.parametrize("n", [4095, 4096, 4097, 65537])
def test_round_trip_of_larger_items(n, E):
    x = some_bytes(n, n + E)
    s = planes.bit_split(x, E)
    assert len(s) == n and s != x
    assert planes.bit_merge(s, E) == x


@pytest.mark.parametrize("E", WIDTHS)
def test_identity_below_eight_elements(E):
    for n in range(8 * E):
        x = some_bytes(n, 77 + n)
        assert planes.bit_split(x, E) == x and planes.bit_merge(x, E) == x


@pytest.mark.parametrize("E", WIDTHS)
def test_body_is_the_bit_transpose_of_the_byte_planes(E):
    for n in (8 * E, 8 * E + 1, 129 * E + 3, 1032 * E + 1, 4097):
        x = some_bytes(n, 5 * n + E)
        g = n // E // 8 * 8
        G = g // 8
        split = planes.split(x[:g * E], E)  # plane k at [k * g, (k + 1) * g)
        want = bytearray()
        for k in range(E):
            plane = np.frombuffer(split[k * g:(k + 1) * g], dtype=np.uint8)
            for b in range(8):
                want += np.packbits((plane >> b) & 1, bitorder="little").tobytes()
        assert len(want) == 8 * E * G
        s = planes.bit_split(x, E)
        assert s[:g * E] == bytes(want) and s[g * E:] == x[g * E:], (n, E)


def test_bad_width_is_refused():
    for bad in (0, 3, 16):
        with pytest.raises(ValueError):
            planes.bit_split(b"abcdefgh" * 8, bad)
        with pytest.raises(ValueError):
            planes.bit_merge(b"abcdefgh" * 8, bad)


def test_fp16_weights_gain_only_from_the_bit_shuffle():
    """Why the filter exists: 64 KiB of fp16 weights are stored raw and byte-split, and compress bit-shuffled."""
    x = np.random.default_rng(70).normal(0, 0.02, 200000).astype(np.float16).tobytes()[:65536]
    shuffled = pyoracle.oz_block(planes.bit_split(x, 2), 65535)
    assert len(shuffled) < 65536
    assert not int.from_bytes(shuffled[:4], "little") & 0x80000000
    split = pyoracle.oz_block(planes.split(x, 2), 65535)
    assert int.from_bytes(split[:4], "little") & 0x80000000  # stored
