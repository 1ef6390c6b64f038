"""Constructed compressor inputs and their census, for the per-position parity tests of the parse.

Plain Python and numpy: no GPU and no oracle call in here.  The oracle's stage arrays come in as
arguments of `census`; tests/test_parse_model.py (CPU) pins what the case set lands on, and
tests/test_parse_choices.py (GPU) compares the device's per-position arrays with the oracle's.

Inputs are scripts of pieces, built by `Script`:
  rand(n)          fresh random bytes from the case's seeded generator
  copy(back, len)  a copy from `back` bytes earlier of exactly `len` bytes; the piece that follows
                   starts with a byte different from the source's next byte, so the match that
                   starts here against that source is exactly `len` long
  run(byte, n)     a same-letter run
  lit(bytes)       bytes from elsewhere (the synth generators' text)

Every case is named, seeded and deterministic, and records the levels (maxChainLength) it is meant for.

Sweeps (`variants(case)`): parse segments and their 64-position chunks are aligned on the block's LAST
parsed position n - 6, token-walk sub-segments (4096 positions) on the block START.  So
  * 64 end-trimmed variants (the block cut by 0..63 bytes) move every chunk, batch and parse-segment
    boundary across the content: 64 is the chunk size, so every alignment of the content to the chunks
    (and to the 4-position batches inside them) occurs once;
  * 16 front-padded variants (k * 273 random bytes prepended, k = 0..15) move the walk boundaries and,
    because the padding lengthens the block, leave the end alignment alone: 273 * k covers the residues
    mod 4096 in steps of 273 (15 * 273 = 4095), so a content feature of 273 positions or more -- every
    long match of the `edges` and `junction` families, every periodic stretch -- lies across a walk
    boundary in at least one of them, and 273 mod 64 = 17 is odd, so the 16 paddings also visit 16
    different alignments to the 64-position windows the walk works in.
  Trim 0 and pad 0 are the base case itself: 64 + 16 - 2 = 78 further inputs per swept base case.
  The sweeps apply to the `edges`, `junction` and `periodic` families.  Their per-position choices are compared
  at level 65535, their frames at 65535 and at one lazy (4) and one greedy (1) level: the other levels differ
  from these in the match search, not in how a boundary is handled.
"""
from __future__ import annotations

import numpy as np

# constants of the reference (smallz4.h) and of the device plan (smallz4_amd/csrc/sz4_internal.h)
MIN_MATCH = 4
TAIL_NOMATCH = 12
TAIL_LITS = 5
SAME_LETTER = 19 + 255 * 256  # MaxSameLetter = kSameLetter
RMQ_LEN = 274                 # kRmqLen
WALK_SEG = 4096               # kWalkSeg
PAR_RMQ_MIN_SEGS = 64         # kParRmqMinSegs
GREEDY_MAX = 3
LAZY_MAX = 6

OPTIMAL = (65535, 16, 8, 7, 5)
GREEDY = (1, 2, 3)
LAZY = (4, 6)
ALL_LEVELS = OPTIMAL + GREEDY + LAZY

SWEPT = ("edges", "junction", "periodic")
TRIMS = 64
PADS = 16
PAD_STEP = 273
SWEEP_LEVELS = (65535, 4, 1)   # choices at 65535; frames also at one lazy and one greedy level


class Script:
    """Builds one input from pieces; see the module docstring."""

    def __init__(self, seed: int):
        self.rng = np.random.default_rng(seed)
        self.out = bytearray()
        self.avoid = None  # the byte the next piece must not start with

    def __len__(self):
        return len(self.out)

    def _first(self, b: int) -> int:
        if self.avoid is not None and b == self.avoid:
            b = (b + 1 + int(self.rng.integers(0, 255))) & 0xFF
            if b == self.avoid:
                b = (b + 1) & 0xFF
        self.avoid = None
        return b

    def rand(self, n: int) -> int:
        at = len(self.out)
        if n:
            b = bytearray(self.rng.integers(0, 256, size=n, dtype=np.uint8).tobytes())
            b[0] = self._first(b[0])
            self.out += b
        return at

    def lit(self, data: bytes) -> int:
        at = len(self.out)
        if data:
            assert self.avoid is None or data[0] != self.avoid, "lit piece would lengthen the copy before it"
            self.avoid = None
            self.out += data
        return at

    def run(self, byte: int, n: int) -> int:
        at = len(self.out)
        assert self.avoid is None or byte != self.avoid, "run piece would lengthen the copy before it"
        self.avoid = None
        self.out += bytes([byte]) * n
        return at

    def copy(self, back: int, n: int) -> int:
        at = len(self.out)
        assert 0 < back <= at and n > 0
        assert self.avoid is None or self.out[at - back] != self.avoid, "copy piece would lengthen the copy before it"
        for _ in range(n):  # byte by byte: back < n is a periodic copy
            self.out.append(self.out[len(self.out) - back])
        self.avoid = self.out[len(self.out) - back]
        return at

    def copy_from(self, src: int, n: int) -> int:
        return self.copy(len(self.out) - src, n)

    def filler(self, n: int, lo: int = 4, hi: int = 40) -> int:
        """About n bytes of short random gaps and short copies from anywhere earlier: overlapping short
        matches, so that every parse segment it covers holds matches."""
        at = len(self.out)
        if at < 256:
            self.rand(256 - at)
        end = at + n
        while len(self.out) < end:
            self.rand(int(self.rng.integers(3, 24)))
            ln = int(self.rng.integers(lo, hi + 1))
            for _ in range(64):
                src = int(self.rng.integers(0, len(self.out) - ln))
                if self.avoid is None or self.out[src] != self.avoid:
                    break
            else:
                self.rand(1)
            self.copy_from(src, ln)
        return at

    def bytes(self) -> bytes:
        return bytes(self.out)


class Case:
    def __init__(self, name: str, family: str, data: bytes, levels=ALL_LEVELS, note: str = ""):
        self.name, self.family, self.data, self.levels, self.note = name, family, bytes(data), tuple(levels), note

    def __repr__(self):
        return f"Case({self.name}, {len(self.data)} B)"


# ---- families -----------------------------------------------------------------------------------
EDGE_LENGTHS = (4, 5, 18, 19, 20, 63, 64, 65, 66, 272, 273, 274, 275, 528, 529, 530, 783, 784)
EDGE_GAPS = (14, 15, 16, 17)
LONG_GAPS = (269, 270, 271)


def _edges(seed: int) -> bytes:
    """Every exact-length copy of EDGE_LENGTHS followed by a random gap of each of EDGE_GAPS; then gaps of
    LONG_GAPS between copies; then copies back to back (literal runs of 0).  Sources are distinct
    stretches of a 2 KiB random head, so a copy's longest match is its own length."""
    s = Script(seed)
    head = 2048
    s.rand(head)
    order = [(ln, g) for g in EDGE_GAPS for ln in EDGE_LENGTHS]
    s.rng.shuffle(order)
    for ln, g in order:
        s.copy_from(int(s.rng.integers(1, head - ln - 1)), ln)
        s.rand(g)
    for g in LONG_GAPS:
        s.copy_from(int(s.rng.integers(1, head - 40)), 24)
        s.rand(g)
    for ln in (4, 19, 65, 274):  # back to back: no literal between two matches
        for _ in range(64):
            src = int(s.rng.integers(1, head - ln - 1))
            if s.out[src] != s.avoid:
                break
        s.copy_from(src, ln)
    s.rand(40)
    return s.bytes()


def _junction_piece(s: Script, p: int, q: int, t: int, tail_gap: int | None = None):
    """P Q x ... Q T y ... P Q T: at the last P the longest match is |P| + |Q| (against the first P Q),
    but Q T continues in the second occurrence, so ending the first match after P can be cheaper."""
    pq = s.rand(p + q)
    s.rand(int(s.rng.integers(5, 12)))          # x ...
    s.copy_from(pq + p, q)                      # Q
    tt = s.rand(t)                              # T (starts with a byte other than x)
    s.rand(int(s.rng.integers(5, 12)))          # y ...
    s.copy_from(pq, p + q)                      # P Q
    s.copy_from(tt, t)                          # T
    s.rand(int(s.rng.integers(5, 12)) if tail_gap is None else tail_gap)


def _junction_long(seed: int) -> bytes:
    s = Script(seed)
    s.rand(64)
    for e in (18, 273, 528, 783, 1038):
        for q in (1, 2, 3):
            _junction_piece(s, e, q, 11 if q == 2 else 6)
    return s.bytes()


def _junction_short(seed: int) -> bytes:
    s = Script(seed)
    s.rand(64)
    while len(s) < 14000:
        p = int(s.rng.integers(4, 61))   # with |Q| up to 19: longest matches on both sides of 64, none near 274
        q = int(s.rng.choice((1, 2, 3, 4, 5, 17, 18, 19)))
        _junction_piece(s, p, q, int(s.rng.integers(1, 12)))
    return s.bytes()


def _junction_inside(seed: int) -> bytes:
    """The optimum strictly inside a length piece k >= 1: P Q T with |Q| = |T| = 3 and 12..14 literals
    after T.  Ending the match after P (a length inside its 255-wide piece, with the full length in the
    same piece) and taking Q T as a 6-byte match leaves a literal run below 15; the full length leaves
    T as literals and pushes the run to 15+, one length byte more."""
    s = Script(seed)
    s.rand(64)
    for p in (300, 400, 600, 700, 900):
        for g in (12, 13, 14):
            _junction_piece(s, p, 3, 3, tail_gap=g)
            s.copy_from(int(s.rng.integers(0, 40)), 8)   # a match ends the literal run
            s.rand(7)
    return s.bytes()


PERIODS = (1, 2, 3, 7, 64, 255, 256, 300)


def _periodic(seed: int) -> bytes:
    """Every period of PERIODS repeated for 1500 bytes, then broken: carried chains that share an end E."""
    s = Script(seed)
    s.rand(100)
    for p in PERIODS:
        if p == 1:
            s.run(int(s.rng.integers(0, 256)), 1500)
            s.rand(30)
        else:
            s.rand(p)
            s.copy(p, 1500 - p)
            s.rand(30)
    s.rand(300)
    return s.bytes()


def _periodic_margin(seed: int) -> bytes:
    """A carried chain with a second, better match that starts inside it: a period-7 stretch of 998 bytes
    whose last 200 bytes and the 400 bytes after it repeat an earlier stretch.  The chain's matches
    (distance 7) all end where the period breaks; from 200 before that point a match of 600 reaches far
    beyond it, so the full chain length is not optimal and the closed form must be refused."""
    s = Script(seed)
    s.rand(80)
    blocks = []
    for period, total in ((7, 998), (3, 1400), (64, 1224)):
        unit = s.rng.integers(0, 256, size=period, dtype=np.uint8).tobytes()
        early = s.lit((unit * (200 // period + 2))[:200])
        s.rand(400)
        s.rand(int(s.rng.integers(200, 400)))
        blocks.append((unit, period, total, early))
    for unit, period, total, early in blocks:
        assert (total - 200) % period == 0
        s.rand(50)
        s.lit((unit * (total // period + 2))[:total - 200])
        s.copy_from(early, 600)
        s.rand(40)
    s.filler(5000)
    return s.bytes()


def _nomatch(seed: int, where: str) -> bytes:
    """A random stretch of 9000 bytes (at least one whole 4096-position parse segment whatever the block's
    length) between matching segments, as the top of the block or as its bottom."""
    s = Script(seed)
    if where == "middle":
        s.filler(6000)
        s.rand(9000)
        s.filler(5000)
    elif where == "top":
        s.filler(9000)
        s.rand(9000)
    else:
        s.rand(9000)
        # copies from the matching part only: the random stretch stays without a match
        base = len(s)
        s.rand(256)
        while len(s) < base + 9000:
            s.rand(int(s.rng.integers(3, 24)))
            ln = int(s.rng.integers(4, 41))
            for _ in range(64):
                src = int(s.rng.integers(base, len(s) - ln))
                if s.avoid is None or s.out[src] != s.avoid:
                    break
            s.copy_from(src, ln)
    return s.bytes()


def _text(n: int, seed: int) -> bytes:
    from smallz4_amd import synth
    return synth.enwik8_like(n, seed=seed)


def _same_letter(run: int) -> bytes:
    """A run of `run` bytes inside a 128 KiB block, text before and after: its first searched position
    finds (distance 1, length run - 1)."""
    head = _text(20000, 41)
    tail = _text(131072 - 20000 - run, 42)
    letter = 0x5A if tail[0] != 0x5A and head[-1] != 0x5A else 0x7E
    return head + bytes([letter]) * run + tail


def _many_segments(n: int) -> bytes:
    from smallz4_amd import synth
    return synth.repeats(600000, seed=77, unit=20000, mutate_every=3000)[:n]


# stored_edge: random data with `copies` short copies; the scripts below were found by the search in
# tests/test_parse_model.py (stored_edge_search) and are fixed here: (size, seed, copies) -> encLen - n
STORED_EDGE = {
    # name: (n, seed, number of copies); the suffix is encLen - n at level 65535
    "stored_300_m1": (300, 2, 1), "stored_300_0": (300, 1, 2), "stored_300_p1": (300, 1, 1),
    "stored_4000_m1": (4000, 12, 6), "stored_4000_0": (4000, 1, 6), "stored_4000_p1": (4000, 3, 6),
    "stored_70000_m1": (70000, 1, 94), "stored_70000_0": (70000, 1, 103), "stored_70000_p1": (70000, 3, 98),
}
STORED_DELTA = {"m1": -1, "0": 0, "p1": 1}


def stored_edge_data(n: int, seed: int, copies: int) -> bytes:
    """n random bytes in which `copies` stretches of 5..7 bytes, evenly spread, repeat the bytes 16..40
    before them."""
    s = Script(seed)
    if copies == 0:
        s.rand(n)
        return s.bytes()
    step = max(48, (n - 64) // copies)
    s.rand(48)
    done = 0
    while done < copies and len(s) + 8 + 12 < n:
        ln = int(s.rng.integers(5, 8))
        s.copy(int(s.rng.integers(16, 41)), ln)
        done += 1
        s.rand(min(step - ln, n - len(s)))
    if len(s) < n:
        s.rand(n - len(s))
    return s.bytes()[:n]


def base_cases() -> list[Case]:
    c = [
        Case("edges", "edges", _edges(101)),
        Case("junction_long", "junction", _junction_long(102)),
        Case("junction_short", "junction", _junction_short(103)),
        Case("junction_inside", "junction", _junction_inside(104)),
        Case("periodic", "periodic", _periodic(105)),
        Case("periodic_margin", "periodic", _periodic_margin(106)),
        Case("nomatch_middle", "nomatch", _nomatch(107, "middle")),
        Case("nomatch_top", "nomatch", _nomatch(108, "top")),
        Case("nomatch_bottom", "nomatch", _nomatch(109, "bottom")),
        Case("text16k", "overlap_text", _text(16384, 43)),
    ]
    from smallz4_amd import synth
    c.append(Case("alpha2", "overlap_text", synth.small_alphabet(12288, k=2, seed=44)))
    c.append(Case("alpha4", "overlap_text", synth.small_alphabet(12288, k=4, seed=45)))
    # the reference's search and parse are quadratic in a same-letter run at the levels that search every
    # position (7 and up): about 8 s per oracle call on a `same_letter` case at 65535, 16, 8 and 7, against
    # milliseconds at the greedy/lazy levels, whose skip scan leaves most of the run unsearched.  So these
    # four run at 65535 and at every level up to 6; 16, 8 and 7 stay out (24 more calls of 8 s per stage)
    for run in (65298, 65299, 65300, 65301):
        c.append(Case(f"same_letter_{run}", "same_letter", _same_letter(run), levels=(65535, 5) + GREEDY + LAZY))
    # (about 2.5 s per oracle call at 65535, 16, 8 and 7, milliseconds below)
    c.append(Case("many_segments_74", "many_segments", _many_segments(600000)))
    c.append(Case("many_segments_64", "many_segments", _many_segments(64 * 8192)))
    for name, (n, seed, copies) in STORED_EDGE.items():
        c.append(Case(name, "stored_edge", stored_edge_data(n, seed, copies)))
    return c


def variants(case: Case) -> list[Case]:
    """The sweep of a base case (module docstring); empty for the families that are not swept."""
    if case.family not in SWEPT:
        return []
    out = []
    for k in range(1, TRIMS):
        out.append(Case(f"{case.name}-trim{k}", case.family, case.data[:len(case.data) - k], levels=SWEEP_LEVELS))
    pad = np.random.default_rng(9000 + len(case.data)).integers(0, 256, size=(PADS - 1) * PAD_STEP, dtype=np.uint8).tobytes()
    for k in range(1, PADS):
        out.append(Case(f"{case.name}-pad{k}", case.family, pad[:k * PAD_STEP] + case.data, levels=SWEEP_LEVELS))
    return out


# ---- the small token encoder ----------------------------------------------------------------------
def path_of(l2, n: int):
    """Positions the emitted path visits: (position, chosen length) of every match, in order."""
    out = []
    at = 0
    while at < n:
        L = int(l2[at])
        if L > 1:
            out.append((at, L))
            at += L
        else:
            at += 1
    return out


def _put_len(o: bytearray, v: int):
    while v >= 255:
        o.append(255)
        v -= 255
    o.append(v)


def encode_choices(data: bytes, l2, d) -> bytes:
    """LZ4 block payload of the walk through the per-position choices from position 0 (what
    selectBestMatches emits, smallz4.h:259-371)."""
    n = len(data)
    o = bytearray()
    lit0 = 0
    for at, L in path_of(l2, n) + [(n, 0)]:
        lits = at - lit0
        mcode = L - MIN_MATCH if L else 0
        o.append((min(lits, 15) << 4) | min(mcode, 15))
        if lits >= 15:
            _put_len(o, lits - 15)
        o += data[lit0:at]
        if not L:
            break
        dist = int(d[at])
        o += bytes([dist & 0xFF, dist >> 8])
        if mcode >= 15:
            _put_len(o, mcode - 15)
        lit0 = at + L
    return bytes(o)


# ---- census ---------------------------------------------------------------------------------------
LONGEST = (18, 19, 64, 65, 273, 274, 528, 529, 783, 784)
PATH_MATCH = (4, 18, 19, 64, 65, 273, 274, 528, 529)
PATH_LITS = (0, 14, 15, 16, 269, 270, 271)


def dp_segments(n: int):
    """(lo, hi) of the block's parse segments, top segment first, as Plan::finish_plan lays them out
    (smallz4_amd/csrc/sz4_plan.cpp, "parse segments: positions [0, n - 6] ...": top = n - 1 - kTailLiterals,
    dp_segment_size(n) = 4096 up to 64 KiB and 8192 above, every segment [hi + 1 - seg, hi] downwards from
    the top, the last one clipped at 0).  The parse's 64-position chunks go downwards from each hi."""
    if n <= TAIL_NOMATCH:
        return []
    seg = 4096 if n <= 65536 else 8192
    out = []
    hi = n - 1 - TAIL_LITS
    while True:
        lo = hi + 1 - seg if hi + 1 >= seg else 0
        out.append((lo, hi))
        if lo == 0:
            break
        hi -= seg
    return out


def strictly_inside(l1, l2, n: int) -> int:
    """Positions whose chosen length lies strictly inside a length piece k >= 1 (lengths 19 + 255 k ..
    273 + 255 k share their extra cost): shorter than the longest, at least 274, not a piece's upper end."""
    top = n - TAIL_LITS
    a, b = np.asarray(l1[:top], dtype=np.int64), np.asarray(l2[:top], dtype=np.int64)
    return int(((b >= RMQ_LEN) & (b < a) & ((b - 18) % 255 != 0)).sum())


def census(data: bytes, l0, l1, l2, d, chain: int) -> set:
    """Feature names of one block at one level, from the oracle's stage arrays: l0 = longest match at
    every position (stage 0), l1 = the matches the parse (or, at greedy levels, the emitter) receives
    (stage 1), l2 = the choices (stage 2), d = their distances."""
    n = len(data)
    f = set()
    if n <= TAIL_NOMATCH:
        return f
    top = n - TAIL_LITS            # positions [0, top) are parsed
    l0 = np.asarray(l0, dtype=np.int64)
    l1 = np.asarray(l1, dtype=np.int64)
    l2 = np.asarray(l2, dtype=np.int64)
    d = np.asarray(d, dtype=np.int64)
    optimal = chain > GREEDY_MAX
    for L in LONGEST:
        if (l0 == L).any():
            f.add(f"longest_{L}")
    path = path_of(l2, n)
    on = np.zeros(n, dtype=bool)
    lit0 = 0
    for at, L in path:
        on[at] = True
        if L in PATH_MATCH:
            f.add(f"path_match_{L}")
        if at - lit0 in PATH_LITS:
            f.add(f"path_lits_{at - lit0}")
        lit0 = at + L
        if at // WALK_SEG != (at + L) // WALK_SEG:
            f.add("chosen_crosses_walk_boundary")
    # stored / compressed decision (the reference stores unless encLen < size)
    enc = len(encode_choices(data, l2, d))
    if enc == n:
        f.add("stored_enc_n")
    elif enc == n + 1:
        f.add("stored_enc_n_plus_1")
    elif enc == n - 1:
        f.add("compressed_enc_n_minus_1")

    if not optimal:
        # greedy: after a fresh match one more linked position is searched (lazy evaluation)
        linked = np.flatnonzero(l0 > 0)
        m = np.flatnonzero(l1 >= MIN_MATCH)
        if len(m) and len(linked):
            nxt = np.searchsorted(linked, m, side="right")
            ok = nxt < len(linked)
            q = linked[nxt[ok]]
            if ((l1[q] > 0) & (q < m[ok] + l1[m[ok]])).any():
                f.add("greedy_lazy_eval_searched")
        if (l1 != l0).any():
            f.add("greedy_stage1_differs")
        return f
    if chain <= LAZY_MAX and (l1 != l0).any():
        f.add("lazy_stage1_differs")

    # shortened choices
    a, b = l1[:top], l2[:top]
    short = (b > 1) & (b < a)
    if (short & on[:top]).any():
        f.add("short_on_path")
    if (short & ~on[:top]).any():
        f.add("short_off_path")
    if (short & (b >= RMQ_LEN) & on[:top]).any():
        f.add("short_rmq_on_path")
    if (short & (b >= RMQ_LEN) & ~on[:top]).any():
        f.add("short_rmq_off_path")
    if (short & (b > 64)).any():
        f.add("short_above_64")
    if strictly_inside(l1, l2, n):
        f.add("short_strictly_inside_piece")

    # parse segments and chunks
    segs = dp_segments(n)
    seg_size = 4096 if n <= 65536 else 8192
    if len(segs) > PAR_RMQ_MIN_SEGS:
        f.add("more_than_64_segments")
    rmq_flag = bool(((a >= RMQ_LEN) & ~((d[:top] == 1) & (a >= SAME_LETTER))).any())
    if rmq_flag:
        f.add("rmq_flag")
        f.add("rmq_parallel_repair" if len(segs) > PAR_RMQ_MIN_SEGS else "rmq_serial_repair")
    has = np.concatenate(([0], np.cumsum(a >= MIN_MATCH)))
    for k, (lo, hi) in enumerate(segs):
        if len(segs) >= 2 and has[hi + 1] == has[lo]:
            f.add("nomatch_segment_" + ("top" if k == 0 else "bottom" if lo == 0 else "middle"))
    # chunks of 64 downwards from every hi: with segments of a multiple of 64 positions, chunk c of the
    # block is [top - 64 c - 64, top - 64 c) (the lowest one clipped at 0)
    rev = a[::-1] > 64
    pad = (-len(rev)) % 64
    big = np.concatenate((rev, np.zeros(pad, dtype=bool))).reshape(-1, 64).any(axis=1)
    per_seg = seg_size // 64
    differs = big[1:] != big[:-1]
    differs[per_seg - 1::per_seg] = False       # neighbours in two different segments do not count
    if differs.any():
        f.add("chunk_le64_next_to_chunk_above_64")
    m = np.flatnonzero(b > 1)
    if len(m):
        seg_of = (top - 1 - m) // seg_size             # 0 = top segment
        land = np.minimum(m + b[m], top - 1)
        seg_land = (top - 1 - land) // seg_size
        if (seg_land < seg_of).any():
            f.add("chosen_crosses_parse_boundary")
        if (seg_land + 1 < seg_of).any():
            f.add("chosen_jumps_parse_segment")

    # literal-length bumps (estimateCosts' numLiterals reaching 15, 270, ...) by batch of their chunk:
    # numLiterals at i = distance to the nearest chosen match above i, or to the block's end
    idx = np.arange(top)
    above = np.where(b != 1, idx, top + TAIL_LITS)     # a match at j restarts the count: i = j - k has k
    nxt = np.minimum.accumulate(above[::-1])[::-1]
    nxt = np.concatenate((nxt[1:], [top + TAIL_LITS]))  # nearest match strictly above i
    lits = nxt - idx
    batch = ((top - 1 - idx) % seg_size % 64) // 4
    for which, hit in (("15", lits == 15), ("270", (lits >= 270) & ((lits - 15) % 255 == 0))):
        if (hit & (batch == 0)).any():
            f.add(f"bump_{which}_first_batch")
        if (hit & (batch == 15)).any():
            f.add(f"bump_{which}_last_batch")

    # carried chains: consecutive positions whose matches share their end
    end = np.where(a >= MIN_MATCH, idx + a, -1 - idx)  # (positions without a match: all different)
    cut = np.flatnonzero(np.concatenate(([True], end[1:] != end[:-1], [True])))
    full = np.concatenate(([0], np.cumsum(b == a)))
    for i, j in zip(cut[:-1], cut[1:]):
        if j - i >= 64 and end[i] >= 0:
            f.add("chain_full_lengths" if full[j] - full[i] == j - i else "chain_shortened")

    # same-letter matches around MaxSameLetter
    one = d[:top] == 1
    if (one & (a >= SAME_LETTER)).any():
        f.add("same_letter_at_least_max")
    if (one & (a == SAME_LETTER)).any():
        f.add("same_letter_equal_max")
    if (one & (a == SAME_LETTER - 1)).any():
        f.add("same_letter_max_minus_1")
    if (one & (a > SAME_LETTER)).any():
        f.add("same_letter_shortcut_interval")
    return f
