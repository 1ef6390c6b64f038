"""LZ4 blocks built from explicit sequence lists (plain Python, no GPU, no oracle).

A sequence is (literal bytes, offset, match length).  A block is a list of sequences plus one of three
endings the reference decoder accepts (oz_unlz4, oracle/smallz4_oracle.c):

  "literals"  a final sequence of >= 1 literals and no match
  "empty"     a final token 0x00 (no literals, no match)
  "match"     the block ends directly after the last sequence's match

encode() writes the payload, expand() is the trivial reference expander (one history across blocks, the
dictionary's last 64 KiB before it, zeros before that; independent=True: every block starts from zeros),
frame() assembles modern and legacy frames, features() names the decoder boundaries a case lands on, and
cases() is the deterministic case set of tests/test_unlz4_sequences.py and tests/test_lz4seq_model.py.
"""
import random
import struct

MAGIC = bytes([0x04, 0x22, 0x4D, 0x18])
LEGACY_MAGIC = bytes([0x02, 0x21, 0x4C, 0x18])
HISTORY = 65536
SUB = 8192            # split mode's sub-segment (kUnSub)
SPLIT_MIN = 256 << 10  # automatic split mode from this payload size on (kUnSplitMin)
SYNC = 8192           # the whole-block decoder drains every kSync bytes
RING = 16384          # ... and keeps the last kRing bytes in LDS


class Block:
    """A compressed block: sequences, an ending, and the final literals of a "literals" ending."""

    def __init__(self, seqs, ending="literals", tail=b"."):
        assert ending in ("literals", "empty", "match")
        assert ending != "literals" or len(tail) >= 1
        self.seqs = [(bytes(l), int(o), int(m)) for l, o, m in seqs]
        self.ending = ending
        self.tail = bytes(tail) if ending == "literals" else b""

    @property
    def recorded(self):
        """Sequences as the decoder counts them: the final literal-only or empty sequence included."""
        return len(self.seqs) + (self.ending != "match")


class Stored:
    """An uncompressed block (modern frames only)."""

    def __init__(self, data):
        assert len(data) >= 1
        self.data = bytes(data)


def _ext(v):
    """Extension bytes of a length field whose nibble is 15: v = length - 15 (>= 0)."""
    return b"\xff" * (v // 255) + bytes([v % 255])


def _ext_len(v):
    return 0 if v < 0 else v // 255 + 1


def seq_size(nlit, mlen):
    """Payload bytes of a sequence with nlit literals and a match of mlen."""
    return 1 + _ext_len(nlit - 15) + nlit + 2 + _ext_len(mlen - 19)


def encode(block):
    """The payload of a Block: token nibbles, 255-run extension bytes, little-endian offsets."""
    out = bytearray()
    for lits, off, mlen in block.seqs:
        assert mlen >= 4 and 0 <= off <= 0xFFFF
        n = len(lits)
        out.append((min(n, 15) << 4) | min(mlen - 4, 15))
        if n >= 15:
            out += _ext(n - 15)
        out += lits
        out += struct.pack("<H", off)
        if mlen - 4 >= 15:
            out += _ext(mlen - 19)
    if block.ending == "literals":
        n = len(block.tail)
        out.append(min(n, 15) << 4)
        if n >= 15:
            out += _ext(n - 15)
        out += block.tail
    elif block.ending == "empty":
        out.append(0)
    return bytes(out)


def expand(blocks, dictionary=b"", independent=False):
    """What the blocks decode to.  Slice copies; a match overlapping itself is its period tiled."""
    buf = bytearray(HISTORY) + bytes(dictionary)[-HISTORY:]
    base = len(buf)
    out = bytearray()
    for blk in blocks:
        if independent:
            out += buf[base:]
            buf = bytearray(HISTORY)
            base = HISTORY
        if isinstance(blk, Stored):
            buf += blk.data
            continue
        for lits, off, mlen in blk.seqs:
            buf += lits
            assert 1 <= off <= 0xFFFF
            src = len(buf) - off
            if off >= mlen:
                buf += buf[src:src + mlen]
            else:
                period = bytes(buf[src:])
                buf += (period * (mlen // off + 1))[:mlen]
        buf += blk.tail
    out += buf[base:]
    return bytes(out)


def build_frame(flags, blocks, content=0, tail=b""):
    """A modern frame with descriptor FLG `flags` over (word, payload) pairs: optional content size,
    dictionary ID, block and content checksums (arbitrary bytes: the reference skips them).  The layout of
    tests/test_unlz4.py's build_frame."""
    hdr = MAGIC + bytes([flags, 0x70])
    if flags & 8:
        hdr += struct.pack("<Q", content)
    if flags & 1:
        hdr += b"\x11\x22\x33\x44"
    hdr += b"\xAB"
    body = b""
    for word, payload in blocks:
        body += struct.pack("<I", word) + payload
        if flags & 16:
            body += b"\xDE\xAD\xBE\xEF"
    return hdr + body + b"\0\0\0\0" + (b"\x01\x02\x03\x04" if flags & 4 else b"") + tail


class Case:
    """One frame of the case set.  Well formed: `blocks` (Block / Stored).  Malformed: `raw`, the block
    payloads as bytes, and blocks is None."""

    def __init__(self, family, name, blocks=None, dictionary=b"", flags=0x40, legacy=False, raw=None, device=False,
                 auto_split=False):
        self.family, self.name = family, name
        self.blocks, self.raw = blocks, raw
        self.dictionary, self.flags, self.legacy = bytes(dictionary), flags, legacy
        self.device = device          # also goes through the device-pointer route at every alignment
        self.auto_split = auto_split  # its block reaches kUnSplitMin: the default context splits it

    def __repr__(self):
        return f"{self.family}/{self.name}"

    def items(self):
        """(size word, payload) of every block."""
        if self.raw is not None:
            return [(len(p), p) for p in self.raw]
        out = []
        for b in self.blocks:
            if isinstance(b, Stored):
                out.append((len(b.data) | 0x80000000, b.data))
            else:
                p = encode(b)
                out.append((len(p), p))
        return out

    def frame(self):
        items = self.items()
        if self.legacy:
            assert len(items) == 1
            return LEGACY_MAGIC + struct.pack("<I", items[0][0]) + items[0][1]
        return build_frame(self.flags, items, content=0)

    def first_src(self):
        """Frame offset of the first block's payload."""
        if self.legacy:
            return 8
        return 4 + 2 + (8 if self.flags & 8 else 0) + (4 if self.flags & 1 else 0) + 1 + 4

    def expected(self):
        return expand(self.blocks, self.dictionary)


# ---- layout and features ---------------------------------------------------------------------------
def layout(block):
    """Per recorded sequence: (token payload offset, literals, offset, match length, payload offset of the
    literals, block-relative output offset of the literals, payload offset of the header's last byte)."""
    rows, p, o = [], 0, 0
    seqs = list(block.seqs)
    if block.ending == "literals":
        seqs.append((block.tail, 0, 0))
    elif block.ending == "empty":
        seqs.append((b"", 0, 0))
    for lits, off, mlen in seqs:
        n = len(lits)
        fr = p + 1 + _ext_len(n - 15)
        last = fr + n - 1 if not mlen else fr + n + 1 + _ext_len(mlen - 19)
        rows.append((p, n, off, mlen, fr, o, max(last, p)))
        p = last + 1 if (mlen or n) else p + 1
        o += n + mlen
    return rows, p, o


def _walk_windows(rows, src, length):
    """The 256-byte register windows the whole-block header walk (unlz4_walk<Walk::kBlock>) fills over a block
    whose payload starts at frame offset `src`: yields (token window offset, header's last window offset) for
    every token of the chain lying in the window that is current when the walk reaches it, and for the tokens
    beyond the refill edge (window offsets 192..255) of that same window.  The speculative mode
    (Walk::kSpec) of the same function walks the same windows over sub-segment 0 of a split block, which
    starts at the block's first token: every family also runs through the `split` fixture."""
    seen = set()
    fast_end = length - 20 if length > 20 else 0
    toks = [r[0] for r in rows]
    i = 0
    while i < len(rows):
        base = (src + toks[i]) & ~3
        wb = base - src
        # every chain token inside this window
        j = i
        while j < len(rows) and toks[j] - wb < 256:
            seen.add((toks[j] - wb, rows[j][6] - wb))
            j += 1
        # the walk: pre-decoded headers until the refill edge, a header it cannot pre-decode, or the tail
        while i < len(rows):
            t, n, off, mlen = rows[i][0], rows[i][1], rows[i][2], rows[i][3]
            q = t - wb
            if t >= fast_end:
                i += 1  # byte-wise, then a fresh window
                break
            if q >= 192:
                break
            pre = n < 15 and mlen and mlen - 19 < 255 and off != 0 and rows[i][6] - wb < 256
            if not pre:
                if q >= 64:
                    break  # the walk refills at the token first: it then sits in the window's first 4 bytes
                i += 1     # byte-wise
                break
            i += 1
    return seen


def reads_before_history(case):
    """True when a match of the case reads before the dictionary tail (or before output byte 0 without one):
    zeros in oz_unlz4 and in this project, but bytes of an uninitialised array in the reference's decoder."""
    dl = min(len(case.dictionary), HISTORY)
    out0 = 0
    for blk in case.blocks:
        if isinstance(blk, Stored):
            out0 += len(blk.data)
            continue
        rows, _, olen = layout(blk)
        if any(m and out0 + o + n - off < -dl for _, n, off, m, _, o, _ in rows):
            return True
        out0 += olen
    return False


def features(case):
    """The edge names (section by section of the case set) that a well-formed case lands on."""
    F = set()
    if case.blocks is None:
        return F
    dl = min(len(case.dictionary), HISTORY)
    F.add(f"dictionary of {len(case.dictionary)} bytes" if case.dictionary else "no dictionary")
    if case.legacy:
        F.add("legacy single-block frame")
    src = case.first_src()
    out0 = 0  # frame-wide output offset of the block
    starts = []  # (output offset, is stored) of every block
    for bi, blk in enumerate(case.blocks):
        starts.append((out0, isinstance(blk, Stored)))
        if isinstance(blk, Stored):
            F.add("stored block")
            src += len(blk.data) + 4 + (4 if case.flags & 16 else 0)
            out0 += len(blk.data)
            continue
        rows, plen, olen = layout(blk)
        payload = encode(blk)
        assert plen == len(payload)
        nrec = len(rows)
        F.add(f"block of {nrec} sequences")
        F.add(f"ending {blk.ending}")
        if nrec in (64, 65):
            F.add(f"ending {blk.ending} at {nrec} sequences")
        if blk.ending == "empty" and nrec > 64:
            F.add("empty final sequence in a block of more than 64 sequences")
        if nrec == plen // 3 + 1 and nrec > 1000:
            F.add("3-byte sequences: nseq == len / 3 + 1")
        if olen >= 80 << 10:
            F.add("block decoding to >= 80 KiB")
        if plen == 3 * SUB:
            F.add("payload of exactly 3 sub-segments")
        if plen == 3 * SUB + 1:
            F.add("last sub-segment of 1 byte")
        if plen == SPLIT_MIN - 1:
            F.add("payload of kUnSplitMin - 1 bytes")
        if plen == SPLIT_MIN:
            F.add("payload of kUnSplitMin bytes")
        # literal register window of every batch of 64 sequences (unlz4_decode)
        for b0 in range(0, nrec, 64):
            batch = rows[b0:b0 + 64]
            fb = (src + batch[0][4]) & ~7
            fe = src + batch[-1][4] + batch[-1][1]
            span = fe - fb
            if len(batch) == 64 and 500 <= span <= 512:
                F.add("batch of 64 sequences whose literals span 500-512 frame bytes")
                for r in batch:
                    if r[1] in (64, 65, 66):
                        F.add(f"literal run of {r[1]} bytes inside a register-window batch")
            if len(batch) == 64 and 513 <= span <= 530:
                F.add("batch of 64 sequences whose literals span 513-530 frame bytes")
        for q, last in _walk_windows(rows, src, plen):
            if q in (191, 192):
                F.add(f"token at header-window offset {q}")
            if last in (254, 255, 256, 257):
                F.add(f"header's last byte at header-window offset {last}")
        # the first batch with a match below the block start or an empty sequence hands the rest of the
        # block to the sequence-wise decoder (unlz4_decode)
        handover = min([i // 64 for i, r in enumerate(rows) if (r[3] and r[2] > r[5] + r[1]) or not (r[1] or r[3])],
                       default=1 << 30)
        sub_first = {}  # sub-segment -> output offset of its first token's literals (k_unlz4_sub's D0)
        for r in rows:
            sub_first.setdefault(r[0] // SUB, r[5])
        for i, (tok, n, off, mlen, fr, o, last) in enumerate(rows):
            via = " (sequence-wise decoder)" if i // 64 >= handover else ""
            if n in LITERAL_RUNS:
                F.add(f"literal run {n}" + via)
            if tok and tok % SUB in (0, 1, SUB - 1) and plen >= 3 * SUB:
                F.add(f"token start at sub-segment offset {tok % SUB}")
            if tok in (SUB - 1, SUB, SUB + 1) and plen >= 3 * SUB:
                F.add(f"token start at payload offset {tok}")
            if n >= 15 + 255 and n < 15 + 510 and tok < SUB <= tok + 2 and plen >= 3 * SUB:
                F.add("two-byte literal-length extension across a sub-segment edge")
            if n:
                for k in range((fr + SUB - 1) // SUB, (fr + n) // SUB):
                    seg = payload[k * SUB:(k + 1) * SUB]
                    if seg == b"\xff" * SUB:
                        F.add("literal run covering a whole sub-segment of 0xFF bytes")
                    elif seg[0::4] == b"\x11" * (SUB // 4) and seg[2::4] == b"\x01" * (SUB // 4) and seg[3::4] == bytes(SUB // 4):
                        F.add("literal run covering a whole sub-segment of valid-looking tokens")
                    else:
                        F.add("literal run covering a whole sub-segment of random bytes")
            if not mlen:
                continue
            q = o + n  # block-relative output offset of the match
            if mlen in MATCH_LENGTHS:
                F.add(f"match length {mlen}" + via)
            if mlen >= 19 and min(mlen - 19, 255) in (0, 254, 255):
                F.add(f"match-length extension byte {min(mlen - 19, 255)} directly after an offset")
            if mlen - 19 >= 255 * 100 and fr + n + 2 < SUB < fr + n + 2 + 100:
                F.add("match-length extension chain of 100 x 255 across a sub-segment edge")
            if off <= q and off in SPLIT_RING_OFFSETS and mlen in RING_LENGTHS and plen >= 3 * SUB:
                where = "inside its sub-segment" if q - off >= sub_first[tok // SUB] else "in an earlier sub-segment"
                F.add(f"split-mode match offset {off} length {mlen} with its source {where}")
            if off <= q:
                if off in OVERLAP_OFFSETS and mlen in OVERLAP_LENGTHS and q % 64 in OVERLAP_POS:
                    F.add(f"overlap offset {off} length {mlen} at output offset {q % 64} mod 64" + via)
                if mlen in (20000, 70000):
                    F.add(f"match of {mlen} bytes at offset {off}" + via)
                if off not in RING_OFFSETS or mlen not in RING_LENGTHS:
                    continue
                if q % SYNC == 1 and q > SYNC:
                    F.add(f"ring offset {off} length {mlen} just after a drain multiple" + via)
                if q % SYNC == SYNC - 1:
                    F.add(f"ring offset {off} length {mlen} just before a drain multiple" + via)
                if off == RING and mlen > 1:
                    F.add("offset 16384 with source straddling the ring edge")
            else:
                # the match reads below the block start
                lo = out0 + q - off  # frame-wide output offset of its first source byte
                batch = i // 64
                F.add(f"match below block start in batch {min(batch, 2)}" + (" or later" if batch >= 2 else ""))
                if lo >= 0:
                    owner = max(k for k, (s, _) in enumerate(starts) if s <= lo)
                    if owner == bi - 1:
                        F.add("match reaching into the previous block")
                    if owner <= bi - 2:
                        F.add("match reaching two blocks back")
                    if starts[owner][1]:
                        F.add("match reaching into a stored block")
                elif not dl:
                    F.add("match below output byte 0 without a dictionary")
                else:
                    hi = lo + mlen  # one past its last source byte, were it not overlapping
                    if lo >= -dl and off < mlen and hi > 0:
                        F.add("self-overlapping match straddling the dictionary/output edge")
                    if lo < -dl and off < mlen and lo + off > -dl:
                        F.add("self-overlapping match straddling the zero/dictionary edge")
                    if lo < -dl:
                        F.add("match below a short dictionary")
        src += plen + 4 + (4 if case.flags & 16 else 0)
        out0 += olen
    return F


# ---- the case set ----------------------------------------------------------------------------------
OVERLAP_OFFSETS = (1, 2, 3, 4, 5, 7, 8, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129)
OVERLAP_LENGTHS = (4, 5, 63, 64, 65, 127, 128, 129, 200, 4099)
OVERLAP_POS = (0, 1, 37, 63)
LITERAL_RUNS = (0, 1, 14, 15, 16, 64, 65, 269, 270, 271, 524, 525, 526, 15 + 255 * 3)
MATCH_LENGTHS = (4, 18, 19, 20, 272, 273, 274, 275, 528, 529, 19 + 255 * 3)
SEQ_COUNTS = (1, 2, 63, 64, 65, 127, 128, 129, 4097)
RING_OFFSETS = (8191, 8192, 8193, 16319, 16320, 16321, 16383, 16384, 16385, 16447, 16448, 32768, 65535)
RING_LENGTHS = (4, 64, 65, 300)
SPLIT_RING_OFFSETS = (1023, 1024, 1025, 1983, 1984, 1985, 2047, 2048, 2049, 2111, 2112, 2113)  # kRingU = 2048, kSyncU = 1024
DICT_LENGTHS = (0, 10, 65536, 70000)


class _Builder:
    """Appends sequences while tracking the payload and output lengths of the block."""

    def __init__(self, rng):
        self.rng, self.seqs, self.plen, self.olen = rng, [], 0, 0

    def lit(self, n):
        return self.rng.randbytes(n)

    def add(self, lits, off, mlen):
        if isinstance(lits, int):
            lits = self.lit(lits)
        self.seqs.append((lits, off, mlen))
        self.plen += seq_size(len(lits), mlen)
        self.olen += len(lits) + mlen

    def add_at(self, mod, res, off, mlen, history=None):
        """A sequence whose match starts at an output offset == res (mod `mod`) with at least `history`
        bytes (default: off) of block output before it."""
        history = off if history is None else history
        n = (res - self.olen) % mod
        while self.olen + n < history:
            n += mod
        self.add(n, off, mlen)

    def token_at(self, target, off=1, mlen=4):
        """One sequence after which the next token starts at payload offset `target`."""
        gap = target - self.plen
        for m in (mlen, 19, 20 + 255):
            for n in range(gap - 3, max(gap - 300, -1), -1):
                if n >= 0 and seq_size(n, m) == gap and (n > 0 or self.olen >= off):
                    self.add(n, off, m)
                    return
        raise AssertionError(f"no sequence of {gap} payload bytes")

    def fill(self, payload_bytes):
        """Short sequences of a few literals and a near match for about `payload_bytes` of payload."""
        stop = self.plen + payload_bytes
        if self.olen < 64:
            self.add(64, 3, 9)
        while self.plen < stop:
            self.add(self.rng.randrange(0, 9), self.rng.randrange(1, 64), self.rng.randrange(4, 40))

    def block(self, ending="literals", tail=None):
        if tail is None:
            tail = self.lit(5)
        return Block(self.seqs, ending, tail)


def _overlap_cases(seqwise):
    """seqwise: the block's first match reads below the block start, so the whole block is replayed by the
    sequence-wise decoder (unlz4_decode) instead of the 64-bytes-per-step one (unlz4_decode_vec)."""
    out = []
    for pos in OVERLAP_POS:
        b = _Builder(random.Random(1000 + pos))
        if seqwise:
            b.add(0, 1, 4)
        b.add(200, 100, 4)
        for mlen in OVERLAP_LENGTHS:
            for off in OVERLAP_OFFSETS:
                b.add_at(64, pos, off, mlen)
        out.append(Case("overlap", f"pos{pos}" + ("-seqwise" if seqwise else ""), [b.block()], device=pos == 37))
    return out


def _length_cases(seqwise):
    rng = random.Random(2000)
    b = _Builder(rng)
    if seqwise:
        b.add(0, 1, 4)
    b.add(300, 7, 4)
    for n in LITERAL_RUNS:
        for mlen in MATCH_LENGTHS:
            b.add(n, rng.choice((1, 2, 5, 64, 100, 290)), mlen)
    return [Case("lengths", "grid" + ("-seqwise" if seqwise else ""), [b.block()], device=True)]


def _counted_block(rng, recorded, ending, first=None):
    b = _Builder(rng)
    nseq = recorded - (ending != "match")
    for i in range(nseq):
        if i == 0:
            b.add(first if first is not None else 40, 8, 6)
        else:
            b.add(rng.randrange(0, 6), rng.randrange(1, 40), rng.randrange(4, 24))
    return b.block(ending, tail=b.lit(rng.randrange(1, 30)))


def _count_cases():
    rng = random.Random(3000)
    out = [Case("counts", "exact", [_counted_block(rng, n, "literals") for n in SEQ_COUNTS], device=True)]
    out.append(Case("counts", "endings", [_counted_block(rng, n, e) for n in (64, 65, 130)
                                          for e in ("literals", "empty", "match")]))
    # one literal, then 3-byte sequences (token 0x00, offset) and an empty final token: nseq = len / 3 + 1
    b = _Builder(rng)
    b.add(1, 1, 4)
    for _ in range(2999):
        b.add(0, rng.choice((1, 2, 3)), 4)
    out.append(Case("counts", "three-byte", [b.block("empty")]))
    return out


def _window_cases():
    rng = random.Random(4000)
    out = []
    # batches of 64 sequences whose literals (and the headers between them) span a chosen number of bytes
    # (the register window belongs to the sequence-wise decoder: a first match below the block start
    # hands the whole block to it; 63 more short sequences complete the first batch)
    b = _Builder(rng)
    b.add(0, 1, 4)
    for _ in range(63):
        b.add(rng.randrange(0, 5), rng.randrange(1, 5), 4)
    for span in list(range(498, 514)) + list(range(514, 531, 2)):
        # 63 headers of 3 bytes between the 64 literal runs: 189 bytes; the rest are literals
        lits = span - 189
        runs = [lits // 64] * 64
        for k in range(lits % 64):
            runs[k] += 1
        if span % 3 == 0:  # one run of 66 bytes: it leaves the register path inside a window batch
            runs[5:20] = [sum(runs[5:20]) - 66] + [0] * 13 + [66]
        elif span % 3 == 1:  # one run of exactly 64 bytes, the longest the register path takes
            runs[5:20] = [sum(runs[5:20]) - 64] + [0] * 13 + [64]
        else:  # one run of 65 bytes
            runs[5:20] = [sum(runs[5:20]) - 65] + [0] * 13 + [65]
            runs[20:36] = [0] * 15 + [sum(runs[20:36])]
        for n in runs:
            b.add(n, rng.randrange(1, 30), 4)
    out.append(Case("windows", "literal-spans", [b.block("match")], device=True))
    # header-window edges: the first literal run padded byte by byte over 8 paddings, then headers of 4 bytes
    # (a match-length byte each) and of 3 + 14 bytes up to the refill edge at 192 and the window end at 256
    blocks = []
    for pad in range(8):
        b = _Builder(rng)
        b.add(20 + pad, 5, 19 + pad)
        for i in range(130):
            if i % 13 == 12:
                b.add(14, 9, 19 + 254)
            else:
                b.add(0, 11, 19 + (i % 3))
        blocks.append(b.block())
    out.append(Case("windows", "header-edges", blocks))
    return out


def _ring_cases(seqwise):
    out = []
    sfx = "-seqwise" if seqwise else ""
    for mlen in RING_LENGTHS:
        rng = random.Random(5000 + mlen)
        b = _Builder(rng)
        if seqwise:
            b.add(0, 1, 4)

        def advance(target):
            # literals and long near matches up to output offset `target` (the payload stays small)
            while target - b.olen > 6000:
                b.add(rng.randrange(300, 900), rng.randrange(1, 300), rng.randrange(2000, 5000))
            assert target - b.olen >= 4
            b.add(target - b.olen - 4, 7, 4)
        k = 8
        for off in RING_OFFSETS:
            for res in (1, SYNC - 1):
                target = k * SYNC + (1 if res == 1 else -1)
                if target <= b.olen:
                    k += 1
                    target += SYNC
                advance(target - 10)
                b.add(10, off, mlen)
                assert (b.olen - mlen) % SYNC == res
                if res != 1:
                    k += 1
        out.append(Case("ring", f"len{mlen}" + sfx, [b.block()], device=mlen == 65))
    if not seqwise:
        # split mode's sub-segment decoder keeps 2048 image words in LDS and drains every 1024
        rng = random.Random(5800)
        b = _Builder(rng)
        b.add(3000, 100, 50)
        for shift in (0, 517):
            b.add(shift, 9, 5)
            for mlen in RING_LENGTHS:
                for off in SPLIT_RING_OFFSETS:
                    for res in (1, 1023):
                        b.add_at(1024, res, off, mlen)
        out.append(Case("ring", "split-ring", [b.block()]))
    rng = random.Random(5900)
    b = _Builder(rng)
    if seqwise:
        b.add(0, 1, 4)
    b.add(17000, 4000, 40)
    for off in (1, 63, 64, 65, 16385):
        b.add(rng.randrange(1, 90), off, 20000)
    b.add(3, 1, 70000)
    out.append(Case("ring", "long-a" + sfx, [b.block()]))
    b = _Builder(rng)
    if seqwise:
        b.add(0, 1, 4)
    b.add(3000, 1000, 60000)
    b.add(HISTORY - b.olen, 8192, 70000)
    b.add(11, 65535, 70000)
    out.append(Case("ring", "long-b" + sfx, [b.block("match")], device=not seqwise))
    return out


def _below_cases():
    rng = random.Random(6000)
    out = []

    def reaching(at):
        """A block whose sequence number `at` (0-based) reads 500 bytes below the block start."""
        b = _Builder(rng)
        for i in range(at):
            b.add(rng.randrange(0, 4) if i else 8, rng.randrange(1, 8), rng.randrange(4, 12))
        b.add(2, b.olen + 2 + 500, 300)
        for _ in range(20):
            b.add(rng.randrange(0, 4), rng.randrange(1, 200), rng.randrange(4, 12))
        return b.block()
    first = Block([(rng.randbytes(900), 30, 100)], "literals", rng.randbytes(7))
    out.append(Case("below", "previous-block", [first, reaching(0), reaching(64), reaching(129)], device=True))
    # blocks of 100 bytes; the fourth reads 300 back: two blocks back and the one between
    small = [Block([(rng.randbytes(60), 13, 30)], "literals", rng.randbytes(10)) for _ in range(3)]
    small.append(Block([(rng.randbytes(20), 320, 250)], "match"))
    small.append(Block([(b"", 1, 4)], "empty"))
    out.append(Case("below", "two-blocks-back", small))
    out.append(Case("below", "stored", [Stored(rng.randbytes(700)), Block([(b"ab", 400, 900)], "literals", b"z"),
                                        Stored(rng.randbytes(3)), Block([(b"", 2, 40), (b"q", 906, 5)], "match")]))
    out.append(Case("below", "zeros", [Block([(b"", 9, 30), (b"abc", 50, 10), (b"", 65535, 70)], "literals", b"end")]))
    for n in DICT_LENGTHS:
        d = random.Random(6100 + n).randbytes(n)
        seqs = [(b"abc", 8, 40),        # 5 bytes of the dictionary, then its own output, overlapping
                (b"", 40000, 20),       # far back: the dictionary, or zeros before a short one
                (b"xy", 65 + 15, 40),   # 65 bytes decoded so far: 15 below output byte 0
                (rng.randbytes(70), 65535, 300)]
        blocks = [Block(seqs, "literals", b"t"), Block([(b"", 180, 40), (b"k", 65535, 19)], "empty")]
        out.append(Case("below", f"dict{n}", blocks, dictionary=d, device=n == 10))
    # the zero/dictionary edge: 10 dictionary bytes, a match starting 15 back at output byte 0
    d = random.Random(6200).randbytes(10)
    out.append(Case("below", "zero-dict-edge", [Block([(b"", 15, 60), (b"m", 13, 33)], "literals", b"e")], dictionary=d))
    b = _Builder(rng)
    b.add(30, 40, 50)  # legacy: zeros below the block
    b.fill(3000)
    out.append(Case("below", "legacy", [b.block()], legacy=True, device=True))
    return out


def _split_cases():
    out = []
    rng = random.Random(7000)
    blocks = []
    for tok in (SUB - 1, SUB, SUB + 1):
        b = _Builder(rng)
        b.fill(SUB - 400)
        b.token_at(tok)
        b.fill(SUB - 300)
        b.token_at(2 * SUB + (tok - SUB))
        b.fill(SUB + 900)
        blocks.append(b.block())
    out.append(Case("split", "token-edges", blocks, device=True))
    blocks = []
    for tok in (SUB - 2, SUB - 1):  # token, then two extension bytes: 8190 8191 | 8192 and 8191 | 8192 8193
        b = _Builder(rng)
        b.fill(SUB - 400)
        b.token_at(tok)
        b.add(15 + 255 + 77, 33, 12)
        b.fill(2 * SUB)
        blocks.append(b.block())
    out.append(Case("split", "literal-extension-across-edge", blocks))
    blocks = []
    for at in (SUB - 50, SUB - 99, SUB - 1):  # first of the 100 extension bytes of 255
        b = _Builder(rng)
        b.fill(SUB - 400)
        b.token_at(at - 3)
        b.add(0, 17, 19 + 255 * 100 + 9)
        b.fill(SUB + 1000)
        blocks.append(b.block("empty"))
    out.append(Case("split", "match-extension-across-edge", blocks))
    for kind in ("random", "ff", "tokens"):
        b = _Builder(rng)
        b.fill(SUB - 1000)
        b.token_at(SUB - 40)
        fr = b.plen + 1 + _ext_len(20000 - 15)
        if kind == "random":
            lits = b.lit(20000)
        elif kind == "ff":
            lits = b"\xff" * 20000
        else:
            pat = bytes([0x11, 0x41, 0x01, 0x00])
            lits = bytes(pat[(fr + k) % 4] if (fr + k) % 4 != 1 else rng.randrange(256) for k in range(20000))
        b.add(lits, 21, 40)
        b.fill(2000)
        out.append(Case("split", f"literal-run-{kind}", [b.block()]))
    for extra in (0, 1):
        b = _Builder(rng)
        b.fill(3 * SUB - 300)
        tail = 7
        b.token_at(3 * SUB + extra - 1 - tail)
        out.append(Case("split", f"payload-3x8192+{extra}", [b.block(tail=b.lit(tail))]))
    for plen in (SPLIT_MIN - 1, SPLIT_MIN):
        b = _Builder(rng)
        while b.plen < plen - 40000:
            b.add(rng.randrange(14000, 30000), rng.randrange(1, 5000), rng.randrange(4, 100))
            for _ in range(30):
                b.add(rng.randrange(0, 9), rng.randrange(1, 64), rng.randrange(4, 40))
        tail = 9
        b.add(plen - b.plen - 1400, 77, 6)
        b.fill(1000)
        b.token_at(plen - 1 - tail)
        out.append(Case("split", f"auto-{plen}", [b.block(tail=b.lit(tail))], auto_split=plen >= SPLIT_MIN))
    return out


def _random_cases():
    out = []
    lit_pool = LITERAL_RUNS
    len_pool = MATCH_LENGTHS + OVERLAP_LENGTHS
    off_pool = OVERLAP_OFFSETS + RING_OFFSETS
    for seed in range(40):
        rng = random.Random(8000 + seed)
        dictionary = rng.randbytes(rng.choice((10, 300, 65536, 70000))) if seed % 5 == 4 else b""
        blocks = []
        total = 0
        for _ in range(rng.randrange(1, 5)):
            if rng.random() < 0.2:
                blocks.append(Stored(rng.randbytes(rng.randrange(1, 3000))))
                total += len(blocks[-1].data)
                continue
            b = _Builder(rng)
            for _ in range(rng.randrange(1, 400)):
                n = rng.choice(lit_pool) if rng.random() < 0.5 else rng.randrange(0, 20)
                mlen = rng.choice(len_pool) if rng.random() < 0.5 else rng.randrange(4, 40)
                off = rng.choice(off_pool) if rng.random() < 0.5 else rng.randrange(1, 300)
                if b.olen + mlen + n > 70000:
                    break
                b.add(n, off, mlen)
            ending = rng.choice(("literals", "empty", "match"))
            blocks.append(b.block(ending, tail=b.lit(rng.randrange(1, 40))))
            total += b.olen
        flags = rng.choice((0x40, 0x40, 0x50, 0x48, 0x44, 0x41, 0x5D, 0x60))
        out.append(Case("random", f"seed{seed}", blocks, dictionary=dictionary, flags=flags, device=seed in (0, 4)))
    return out


def _malformed_tails():
    """(name, the bytes that make a block malformed when they end it)."""
    return [("literal-run-past-end", b"\x80abcdefg"),                  # 8 literals announced, 7 left
            ("match-extension-to-end", b"\x1fa\x05\x00" + b"\xff" * 6),  # the chain of 255s reaches the end
            ("one-offset-byte", b"\x10a\x05")]


def _malformed_cases():
    rng = random.Random(9000)
    out = []
    b = _Builder(rng)
    for i in range(129):
        b.add(rng.randrange(1, 5), 0 if i == 64 else 1, rng.randrange(4, 12))
    out.append(Case("malformed", "offset0-seq65-of-130", raw=[encode(b.block())]))
    for name, tail in _malformed_tails():
        b = _Builder(rng)
        b.fill(300)
        out.append(Case("malformed", name, raw=[encode(b.block("match")) + tail]))
    # the same in the last sub-segment of a block of three
    b = _Builder(rng)
    b.fill(2 * SUB + 500)
    good = len(b.seqs)
    b.add(3, 0, 8)
    b.fill(300)
    assert b.seqs[good][1] == 0
    out.append(Case("malformed", "split-offset0", raw=[encode(b.block())]))
    for name, tail in _malformed_tails():
        b = _Builder(rng)
        b.fill(2 * SUB + 500)
        out.append(Case("malformed", "split-" + name, raw=[encode(b.block("match")) + tail]))
    return out


_CASES = None


def cases():
    """The whole case set (built once; treat it as read-only)."""
    global _CASES
    if _CASES is None:
        _CASES = (_overlap_cases(False) + _overlap_cases(True) + _length_cases(False) + _length_cases(True) + _count_cases() + _window_cases() +
                  _ring_cases(False) + _ring_cases(True) + _below_cases() + _split_cases() + _random_cases() + _malformed_cases())
    return _CASES


def well_formed(family=None):
    return [c for c in cases() if c.blocks is not None and (family is None or c.family == family)]


def malformed():
    return [c for c in cases() if c.blocks is None]


def parse(payload):
    """encode()'s inverse for the self-check: (sequences, ending, tail) of a payload."""
    seqs, r, end = [], 0, len(payload)
    while r < end:
        tok = payload[r]
        r += 1
        n = tok >> 4
        if n == 15:
            while True:
                x = payload[r]
                r += 1
                n += x
                if x != 255:
                    break
        lits = payload[r:r + n]
        r += n
        if r == end:
            return seqs, ("literals" if n else "empty"), lits
        off = payload[r] | (payload[r + 1] << 8)
        r += 2
        m = 4 + (tok & 15)
        if m == 19:
            while True:
                x = payload[r]
                r += 1
                m += x
                if x != 255:
                    break
        seqs.append((lits, off, m))
    return seqs, "match", b""
