"""The constructed-sequence case set (tests/golden/lz4seq.py) on the CPU: the plain expander against the
oracle's decoder (oz_unlz4) and, where it was compiled, the reference's own smallz4cat; the malformed cases
rejected by the oracle; the decoder boundaries the case set must keep landing on; the encoder against a
small parser.  The GPU side is tests/test_unlz4_sequences.py."""
import os
import random
import subprocess

import pytest

import lz4seq
from oracle import pyoracle

# ---- the boundaries the case set pins, written out (one group per bullet of the case-set plan) -----------
OVERLAP_OFFSETS = (1, 2, 3, 4, 5, 7, 8, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129)
OVERLAP_LENGTHS = (4, 5, 63, 64, 65, 127, 128, 129, 200, 4099)
OVERLAP_POS = (0, 1, 37, 63)
LITERAL_RUNS = (0, 1, 14, 15, 16, 64, 65, 269, 270, 271, 524, 525, 526, 780)
MATCH_LENGTHS = (4, 18, 19, 20, 272, 273, 274, 275, 528, 529, 784)
SEQ_COUNTS = (1, 2, 63, 64, 65, 127, 128, 129, 4097)
RING_OFFSETS = (8191, 8192, 8193, 16319, 16320, 16321, 16383, 16384, 16385, 16447, 16448, 32768, 65535)
RING_LENGTHS = (4, 64, 65, 300)
SPLIT_RING_OFFSETS = (1023, 1024, 1025, 1983, 1984, 1985, 2047, 2048, 2049, 2111, 2112, 2113)
BOTH_DECODERS = ("", " (sequence-wise decoder)")  # unlz4_decode_vec, and unlz4_decode after a hand-over in batch 0

REQUIRED = (
    # overlap periods
    [f"overlap offset {o} length {m} at output offset {p} mod 64{via}"
     for o in OVERLAP_OFFSETS for m in OVERLAP_LENGTHS for p in OVERLAP_POS for via in BOTH_DECODERS]
    # length fields
    + [f"literal run {n}{via}" for n in LITERAL_RUNS for via in BOTH_DECODERS]
    + [f"match length {m}{via}" for m in MATCH_LENGTHS for via in BOTH_DECODERS]
    + [f"match-length extension byte {x} directly after an offset" for x in (0, 254, 255)]
    # sequence counts
    + [f"block of {n} sequences" for n in SEQ_COUNTS]
    + ["3-byte sequences: nseq == len / 3 + 1"]
    + [f"ending {e} at {n} sequences" for e in ("literals", "empty", "match") for n in (64, 65)]
    + ["empty final sequence in a block of more than 64 sequences"]
    # literal windows
    + ["batch of 64 sequences whose literals span 500-512 frame bytes",
       "batch of 64 sequences whose literals span 513-530 frame bytes",
       "literal run of 64 bytes inside a register-window batch",
       "literal run of 65 bytes inside a register-window batch",
       "literal run of 66 bytes inside a register-window batch"]
    + [f"header's last byte at header-window offset {q}" for q in (254, 255, 256, 257)]
    + [f"token at header-window offset {q}" for q in (191, 192)]
    # ring and drain
    + ["block decoding to >= 80 KiB", "offset 16384 with source straddling the ring edge"]
    + [f"ring offset {o} length {m} just {side} a drain multiple{via}"
       for o in RING_OFFSETS for m in RING_LENGTHS for side in ("after", "before") for via in BOTH_DECODERS]
    + [f"match of 20000 bytes at offset {o}{via}" for o in (1, 63, 64, 65, 16385) for via in BOTH_DECODERS]
    + [f"match of 70000 bytes at offset {o}{via}" for o in (1, 8192, 65535) for via in BOTH_DECODERS]
    + [f"split-mode match offset {o} length {m} with its source inside its sub-segment" for o in SPLIT_RING_OFFSETS
       for m in RING_LENGTHS]
    # below the block start
    + ["match below block start in batch 0", "match below block start in batch 1",
       "match below block start in batch 2 or later", "match reaching into the previous block",
       "match reaching two blocks back", "match reaching into a stored block",
       "match below output byte 0 without a dictionary", "no dictionary", "dictionary of 10 bytes",
       "dictionary of 65536 bytes", "dictionary of 70000 bytes", "match below a short dictionary",
       "self-overlapping match straddling the dictionary/output edge",
       "self-overlapping match straddling the zero/dictionary edge", "legacy single-block frame"]
    # split mode
    + [f"token start at payload offset {t}" for t in (8191, 8192, 8193)]
    + [f"token start at sub-segment offset {t}" for t in (0, 1, 8191)]
    + ["two-byte literal-length extension across a sub-segment edge",
       "match-length extension chain of 100 x 255 across a sub-segment edge",
       "literal run covering a whole sub-segment of random bytes",
       "literal run covering a whole sub-segment of 0xFF bytes",
       "literal run covering a whole sub-segment of valid-looking tokens",
       "payload of exactly 3 sub-segments", "last sub-segment of 1 byte",
       "payload of kUnSplitMin - 1 bytes", "payload of kUnSplitMin bytes"]
    # random family
    + ["stored block", "ending literals", "ending empty", "ending match"]
)

MALFORMED = {"offset0-seq65-of-130", "match-extension-to-end", "literal-run-past-end", "one-offset-byte",
             "split-offset0", "split-match-extension-to-end", "split-literal-run-past-end", "split-one-offset-byte"}


def first_diff(got, want):
    n = min(len(got), len(want))
    return next((i for i in range(n) if got[i] != want[i]), n)


def test_model_matches_oracle():
    """expand() is what oz_unlz4 decodes, for every well-formed case."""
    for case in lz4seq.well_formed():
        want = case.expected()
        got = pyoracle.oz_unlz4(case.frame(), case.dictionary, cap=len(want) + 64)
        assert got == want, (case, len(got), len(want), first_diff(got, want))


def test_model_independent_blocks():
    """expand(independent=True) is every block decoded as a frame of its own, without the dictionary."""
    for case in lz4seq.well_formed():
        want = b"".join(pyoracle.oz_unlz4(lz4seq.build_frame(0x40, [item]), cap=1 << 20) for item in case.items())
        assert lz4seq.expand(case.blocks, independent=True) == want, case
        assert [lz4seq.expand([b], independent=True) for b in case.blocks] == \
               [pyoracle.oz_unlz4(lz4seq.build_frame(0x40, [item]), cap=1 << 20) for item in case.items()], case


def test_malformed_cases_rejected_by_oracle():
    cases = lz4seq.malformed()
    assert {c.name for c in cases} == MALFORMED
    for case in cases:
        with pytest.raises(ValueError):
            pyoracle.oz_unlz4(case.frame())


@pytest.mark.skipif(not os.path.exists(pyoracle.REF_CAT), reason="reference decoder not compiled")
def test_model_matches_reference_binary(tmp_path):
    """The reference's own smallz4cat writes expand()'s bytes for every well-formed case whose matches stay
    inside the history.  (Its history[] is an uninitialised stack array, smallz4cat.c:164, so a match reading
    before the dictionary or before output byte 0 has no defined bytes there; oz_unlz4 defines them as 0.)"""
    compared = [c for c in lz4seq.well_formed() if not lz4seq.reads_before_history(c)]
    assert len(compared) >= 30 and {c.family for c in compared} == {c.family for c in lz4seq.well_formed()}
    for case in compared:
        args = [pyoracle.REF_CAT]
        if case.dictionary:
            d = tmp_path / "dict.bin"
            d.write_bytes(case.dictionary)
            args += ["-D", str(d)]
        ref = subprocess.run(args, input=case.frame(), capture_output=True)
        assert ref.returncode == 0, (case, ref.stderr)
        want = case.expected()
        assert ref.stdout == want, (case, len(ref.stdout), len(want), first_diff(ref.stdout, want))


def test_case_set_covers_every_boundary():
    """The case set lands on every decoder boundary named above; an edit of the generator or its seeds that
    loses one fails here, before any GPU run."""
    seen = set()
    for case in lz4seq.well_formed():
        seen |= lz4seq.features(case)
    missing = [name for name in REQUIRED if name not in seen]
    assert not missing, missing
    assert len(set(REQUIRED)) == len(REQUIRED)


def test_case_set_shape():
    """Deterministic, tens of frames, 40 random ones, sizes as planned."""
    cases = lz4seq.cases()
    again = [c.frame() for c in lz4seq._overlap_cases(False) + lz4seq._random_cases()]
    assert again == [c.frame() for c in cases if c.family == "overlap" and "seqwise" not in c.name or c.family == "random"]
    assert sum(c.family == "random" for c in cases) == 40
    assert len(cases) < 120
    for case in lz4seq.well_formed():
        assert len(case.expected()) <= 310 << 10, case
        assert 1 <= len(case.blocks) <= 9 or case.family != "random"
        assert case.auto_split == any(n >= lz4seq.SPLIT_MIN for n, _ in case.items() if not n >> 31), case
    assert sum(c.device for c in cases) >= 8 and {c.family for c in cases if c.device} == \
        {c.family for c in cases if c.blocks is not None}


def test_encoder_against_parser():
    """encode()'s payload parses back to the same sequences, ending and final literals: the 255-run
    extension edges (15 + 255 k literals, 19 + 255 k match bytes need a trailing 0) included."""
    edges = [0, 1, 14, 15, 16, 269, 270, 271, 524, 525, 526, 15 + 255 * 3, 15 + 255 * 3 + 1]
    medges = [4, 18, 19, 20, 273, 274, 275, 528, 529, 530, 19 + 255 * 3, 19 + 255 * 3 + 1, 70000]
    for n in edges:
        for m in medges:
            p = lz4seq.encode(lz4seq.Block([(b"x" * n, 7, m)], "match"))
            assert len(p) == lz4seq.seq_size(n, m)
            assert p[-1] != 255 or m < 19
            assert lz4seq.parse(p) == ([(b"x" * n, 7, m)], "match", b"")
    assert lz4seq.encode(lz4seq.Block([(b"", 1, 19)], "match")) == b"\x0f\x01\x00\x00"
    assert lz4seq.encode(lz4seq.Block([(b"", 1, 274)], "match")) == b"\x0f\x01\x00\xff\x00"
    assert lz4seq.encode(lz4seq.Block([], "literals", b"y" * 270)) == b"\xf0\xff\x00" + b"y" * 270
    rng = random.Random(31)
    for _ in range(200):
        seqs = []
        for _ in range(rng.randrange(0, 30)):
            n = rng.choice(edges) if rng.random() < 0.3 else rng.randrange(0, 40)
            m = rng.choice(medges[:-1]) if rng.random() < 0.3 else rng.randrange(4, 40)
            seqs.append((rng.randbytes(n), rng.randrange(1, 65536), m))
        ending = rng.choice(("literals", "empty", "match"))
        if not seqs and ending == "match":
            ending = "empty"
        tail = rng.randbytes(rng.choice(edges[1:])) if ending == "literals" else b""
        blk = lz4seq.Block(seqs, ending, tail or b".")
        assert lz4seq.parse(lz4seq.encode(blk)) == (blk.seqs, ending, blk.tail)
        rows, plen, olen = lz4seq.layout(blk)
        assert plen == len(lz4seq.encode(blk)) and olen == len(lz4seq.expand([blk]))
        assert len(rows) == blk.recorded
