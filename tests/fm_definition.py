"""FM-index tests from the definition: an index (rows, '#' rows, '$' row, suffix array) made in plain numpy / Python for
any collection, the small collections that sit on the edges of the 384-row rank line, and brute-force answers of every
FM query from the record strings and that suffix array.  Nothing here calls the library.

The order is the project's: codes 0..5 = A < C < G < T < '#' < '$', suffixes compared symbol by symbol; '$' is unique and
last, so no suffix is a prefix of another and the suffix array of a text is unique.  Row r of the BWT holds the symbol
before suffix sa[r] (cyclically: '$' before position 0), packed as code min(symbol, 3) at bits 2 * (31 - r % 32) of word
r // 32; the rows that hold '#' and the row that holds '$' are listed beside the words.

The high 24 bits of the separators-before count of a rank line (more than 2^24 records in front of a line) are beyond
every collection here: many_records_ref.py makes the index of 2^24 + 300 one-base records in closed form, and
test_fm_many_records_gpu.py runs the queries on it."""
import bisect
import functools

import numpy as np

from kmer_ref import Ref as KmerRef
from overlap_mm_ref import brute as overlap_mm_brute
from overlap_ref import Ref as OverlapRef
from overlap_ref import longest_of

ROWS = 384                     # rows of one rank line (VB_ROWS)
SEP, END = 4, 5
ACGT = "ACGT"
_LUT = np.full(256, 9, dtype=np.uint8)                   # ASCII -> code; 9: a character that equals no base
for _i, _c in enumerate(ACGT):
    _LUT[ord(_c)] = _LUT[ord(_c.lower())] = _i
_COMP = str.maketrans("ACGTacgt", "TGCAtgca")


def revcomp(p):
    """reverse complement of a str; a character outside ACGTacgt stays a non-base ('N')"""
    return "".join(c.translate(_COMP) if c in "ACGTacgt" else "N" for c in reversed(p))


def strings(records):
    return ["".join(ACGT[c] for c in np.asarray(r).tolist()) for r in records]


def text_symbols(records):
    """r0 # r1 # ... $ as codes 0..5"""
    parts = []
    for i, r in enumerate(records):
        parts.append(np.asarray(r, dtype=np.uint8))
        parts.append(np.array([END if i + 1 == len(records) else SEP], dtype=np.uint8))
    return np.concatenate(parts)


def pack_rows(L):
    """symbols of the rows (0..5) -> packed words, '#' and '$' as code 3"""
    n = len(L)
    code = np.zeros((n + 31) // 32 * 32, dtype=np.uint64)
    code[:n] = np.minimum(L, 3)
    shift = (2 * (31 - np.arange(32))).astype(np.uint64)
    return np.bitwise_or.reduce(code.reshape(-1, 32) << shift[None, :], axis=1)


def definition_index(records):
    """(sym, sa, L, words, hash_rows, dollar_row) of the collection, from the definition"""
    sym = text_symbols(records)
    n = len(sym)
    b = sym.tobytes()
    sa = np.array(sorted(range(n), key=lambda i: b[i:]), dtype=np.int64)
    L = sym[(sa - 1) % n]
    hash_rows = np.nonzero(L == SEP)[0].astype(np.uint64)
    dollar = np.nonzero(L == END)[0]
    assert len(dollar) == 1
    return sym, sa, L, pack_rows(L), hash_rows, int(dollar[0])


def suffix_array(sym):
    """The same suffix array for a text of any size, by prefix doubling in numpy: rank[i] is the first slot of the group
    of suffixes that share suffix i's first h symbols; a round orders every group of two or more by the rank of the
    suffix h symbols further on and splits it, h doubles, and it ends when every group is one suffix.  Behind the text
    stand zeros: two suffixes differ at or before the '$' of the shorter one, so the padding is never what decides."""
    sym = np.asarray(sym, dtype=np.uint8)
    n, h = len(sym), 21
    pad = np.concatenate([sym, np.zeros(h, dtype=np.uint8)]).astype(np.uint64)
    key = np.zeros(n, dtype=np.uint64)
    for j in range(h):
        key = (key << np.uint64(3)) | pad[j:j + n]
    order = np.argsort(key).astype(np.int64)
    k = key[order]
    first = np.concatenate([[True], k[1:] != k[:-1]])                   # a slot that begins a group
    rank = np.empty(n, dtype=np.int64)
    rank[order] = np.maximum.accumulate(np.where(first, np.arange(n), 0))
    while True:
        single = first & np.concatenate([first[1:], [True]])
        slots = np.nonzero(~single)[0]
        if not len(slots):
            return order
        idx = order[slots]
        g = rank[idx]
        nxt = idx + h
        k2 = np.where(nxt < n, rank[np.minimum(nxt, n - 1)], -1)
        o = np.argsort(g.astype(np.uint64) * np.uint64(n + 1) + (k2 + 1).astype(np.uint64))   # by (g, k2); n^2 < 2^64
        idx, g, k2 = idx[o], g[o], k2[o]
        order[slots] = idx
        new = np.concatenate([[True], (g[1:] != g[:-1]) | (k2[1:] != k2[:-1])])
        first[slots] = new
        rank[idx] = np.maximum.accumulate(np.where(new, slots, 0))
        h *= 2


def samples(sa, s):
    """the sampled suffix array of an index with sa_sample = s: the position of every row r with r % s == 0"""
    return np.ascontiguousarray(sa[::s]).astype(np.uint64)


def packed_text(records):
    """(words, sep) as debwt_fm_text_fetch documents them: ((n + 63) >> 5) + 2 words, base j at bits 2 * (31 - j % 32) of
    word j // 32, separators as 'T', 32 'T' behind position n - 1 and zeros behind; the nrec separator positions"""
    return packed_text_of(text_symbols(records))


def packed_text_of(sym):
    """packed_text from the text's codes 0..5"""
    n = len(sym)
    nw = ((n + 63) >> 5) + 2
    code = np.zeros(nw * 32, dtype=np.uint64)
    code[:n] = np.minimum(sym, 3)
    code[n:n + 32] = 3
    shift = (2 * (31 - np.arange(32))).astype(np.uint64)
    words = np.bitwise_or.reduce(code.reshape(-1, 32) << shift[None, :], axis=1)
    return words, np.nonzero(sym > 3)[0].astype(np.uint64)


def line_profile(L):
    """per rank line (rows grouped in 384s, n // 384 + 1 lines as the rank build allocates them): (separator rows in
    the line, 'T' rows in the line, separator rows before the line)"""
    n = len(L)
    out, before = [], 0
    for b in range(n // ROWS + 1):
        part = L[b * ROWS:(b + 1) * ROWS]
        seps = int(np.count_nonzero(part > 3))
        out.append((seps, int(np.count_nonzero(part == 3)), before))
        before += seps
    return out


def header_branch_lines(L):
    """lines that hold 'T' rows, no separator row, and have separators before them: occ('T') there takes the count from
    the header words, and the count is not zero"""
    return [b for b, (seps, ts, before) in enumerate(line_profile(L)) if ts and not seps and before]


# ---- the collections ---------------------------------------------------------------------------------------------------

def _padded(recs, n, R):
    have = sum(len(r) for r in recs) + len(recs)
    assert have <= n
    recs = list(recs)
    if n > have:
        recs[-1] = np.concatenate([recs[-1], R(n - have)])
    return recs


@functools.lru_cache(maxsize=None)
def _geometry_cases():
    from conftest import outside_domain_cases
    rng = np.random.default_rng(1)
    R = lambda m: rng.integers(0, 4, m).astype(np.uint8)                             # noqa: E731
    T = lambda m: np.full(m, 3, dtype=np.uint8)                                      # noqa: E731
    c = {}
    c["n2"] = [np.array([0], dtype=np.uint8)]
    c["n32"] = _padded([R(5)], 32, R)
    c["n33"] = _padded([R(5)], 33, R)
    c["n64"] = _padded([R(5), R(7)], 64, R)
    for n in (383, 384, 385):
        c[f"n{n}"] = _padded([R(50), R(60)], n, R)
    c["n768"] = _padded([R(100), R(100), R(100)], 768, R)
    c["n1152_single"] = [R(1151)]
    c["ones_600"] = [R(1) for _ in range(600)]
    c["short_1to3_x500"] = [R(int(m)) for m in rng.integers(1, 4, 500)]
    c["all_T_x3"] = [T(400), T(37), T(1)]
    c["T_ones_400"] = [T(1) for _ in range(400)]
    c["dup_40x20"] = [R(40)] * 20
    for name, seed in (("dollar_383", 362), ("dollar_384", 152)):
        g = np.random.default_rng(seed)
        c[name] = [g.integers(0, 4, m).astype(np.uint8) for m in (300, 250, 200)]
    for name, recs in outside_domain_cases().items():
        assert name not in c
        c[name] = [np.asarray(r, dtype=np.uint8) for r in recs]
    return c


def geometry_cases():
    """name -> records (uint8 code arrays): the collections on the edges of the rank line, then the nine collections of
    conftest.outside_domain_cases() as they are.  test_fm_definition_ref.py asserts what each is here for."""
    return dict(_geometry_cases())


BUILDER_CASES = ("n383", "n384", "n385", "n768", "n1152_single", "dup_40x20", "dollar_383", "dollar_384")


# ---- brute-force answers -----------------------------------------------------------------------------------------------

class Definition:
    """One collection: its definition index and the answer of every FM query by brute force over the record strings and
    the suffix array.  A suffix "cut" is the suffix up to its first separator."""

    def __init__(self, records):
        self.records = [np.asarray(r, dtype=np.uint8) for r in records]
        self.strs = strings(self.records)
        self.sym, self.sa, self.L, self.words, self.hash_rows, self.dollar_row = definition_index(self.records)
        self.n, self.nrec = len(self.sym), len(self.records)
        b = self.sym.tobytes()
        self._keys = [b[int(i):] for i in self.sa]                      # the suffixes in row order
        self.starts = np.concatenate([[0], np.nonzero(self.sym > 3)[0][:-1] + 1]).astype(np.uint64)
        self.joined = "#".join(self.strs) + "$"
        self._csep = np.concatenate([[0], np.cumsum(self.sym > 3)])
        self._mem_s = {}

    # -- rows --
    def interval(self, p):
        """[lo, hi) of the rows whose cut suffix starts with p (str or bytes, either case); (0, 0) for an empty pattern
        and for one with a character outside ACGTacgt"""
        if isinstance(p, str):
            p = p.encode()
        if not p:
            return 0, 0
        c = _LUT[np.frombuffer(p, dtype=np.uint8)]
        if (c > 3).any():
            return 0, 0
        key = c.tobytes()
        lo = bisect.bisect_left(self._keys, key)
        hi = bisect.bisect_left(self._keys, key + b"\x06")             # above every symbol, '$' = 5 included
        return lo, hi

    def locate(self, p, cap=None):
        lo, hi = self.interval(p)
        out = self.sa[lo:hi]
        return out if cap is None else out[:cap]

    def census(self):
        """rows per 2-bit code, '#' and '$' rows counted as 3"""
        return np.bincount(np.minimum(self.L, 3), minlength=4).astype(np.uint64)

    # -- search with substitutions --
    def _windows(self, q, K):
        """{text string: mismatches} of the windows inside one record within K substitutions of q (str)"""
        m, n = len(q), self.n
        if m == 0 or m > n:
            return {}
        qc = _LUT[np.frombuffer(q.encode(), dtype=np.uint8)]
        w = n - m + 1
        dist = np.zeros(w, dtype=np.int64)
        for j in range(m):
            dist += self.sym[j:j + w] != qc[j]
        ok = (self._csep[m:m + w] - self._csep[:w] == 0) & (dist <= K)
        out = {}
        for p in np.nonzero(ok)[0].tolist():
            out[self.joined[p:p + m]] = int(dist[p])
        return out

    def search(self, p, K, both=False, best=False):
        """[(lo, hi, mismatches, strand)] per distinct text string, ascending by (strand, mismatches, lo)"""
        hits = []
        for strand, q in ((0, p), (1, revcomp(p))):
            if strand and not both:
                break
            for w, d in self._windows(q, K).items():
                lo, hi = self.interval(w)
                hits.append((lo, hi, d, strand))
        if best and hits:
            least = min(h[2] for h in hits)
            hits = [h for h in hits if h[2] == least]
        return sorted(hits, key=lambda h: (h[3], h[2], h[0]))

    # -- maximal exact matches --
    def _s_of(self, q):
        """s(e) of debwt_fm_mems for every e of q (upper case): non-decreasing, so a two-pointer walk"""
        got = self._mem_s.get(q)
        if got is None:
            s, got = 0, []
            for e in range(len(q)):
                while s <= e and q[s:e + 1] not in self.joined:         # an ACGT string never spans a separator
                    s += 1
                got.append(s)
            self._mem_s[q] = got
        return got

    def mems(self, p, min_len, both=False):
        """sorted (strand, qbeg, qend) in the coordinates of p as given"""
        out, m = [], len(p)
        for strand, q in ((0, p.upper()), (1, revcomp(p).upper())):
            if strand and not both:
                break
            q = "".join(c if c in ACGT else "N" for c in q)
            s = self._s_of(q)
            for e in range(m):
                if s[e] <= e and (e == m - 1 or s[e + 1] > s[e]) and e + 1 - s[e] >= min_len:
                    a, b = s[e], e + 1
                    out.append((0, a, b) if strand == 0 else (1, m - b, m - a))
        return sorted(out)

    # -- overlaps --
    @functools.lru_cache(maxsize=None)
    def _overlap_ref(self, min_overlap):
        return OverlapRef(self.strs, min_overlap)

    def overlaps(self, p, min_overlap, both=False, longest=False):
        """[(record, length, strand, flags)] by (strand, length descending, record ascending)"""
        R = self._overlap_ref(min_overlap)
        out = R.hits(p, 0) + (R.hits(p, 1) if both else [])
        return longest_of(out) if longest else out

    def overlaps_mm(self, p, min_overlap, K, both=False, longest=False):
        """as overlaps(), with up to K mismatches and the count in bits 8-15 of the flags"""
        out = overlap_mm_brute(self.strs, p, min_overlap, K, 0, 0)
        if both:
            out += overlap_mm_brute(self.strs, revcomp(p), min_overlap, K, 0, 1)
        return longest_of(out) if longest else out

    # -- k-mers --
    @functools.lru_cache(maxsize=None)
    def _kmer_ref(self, k, both):
        return KmerRef(self.strs, k, both)

    def kmer_profile(self, p, k, both=False):
        return self._kmer_ref(k, both).profile(p)

    # -- text --
    def substring(self, record, offset=0, length=None):
        s = self.strs[record]
        return s[offset:] if length is None else s[offset:offset + length]


@functools.lru_cache(maxsize=None)
def definition_of(name):
    """the Definition of a geometry case, made once"""
    return Definition(_geometry_cases()[name])


# ---- the patterns of the GPU tests -------------------------------------------------------------------------------------

def mixed_case(p, rng):
    b = np.frombuffer(p.encode(), dtype=np.uint8).copy()
    b[rng.random(len(b)) < 0.4] |= 0x20
    return b.tobytes().decode()


@functools.lru_cache(maxsize=None)
def range_patterns(name):
    """The patterns of the range and locate tests, as bytes: every distinct substring of the records up to length 6, each
    of them with each base in front, every record prefix and suffix, 200 sampled substrings of 7..64 bases where a
    record is long enough, mixed-case copies and the odd patterns."""
    D = definition_of(name)
    rng = np.random.default_rng(len(D.sym))
    seen, pats = set(), []

    def add(p):
        if p not in seen:
            seen.add(p)
            pats.append(p)

    distinct = set()
    for s in set(D.strs):
        for m in range(1, 7):
            for i in range(len(s) - m + 1):
                distinct.add(s[i:i + m])
    for w in sorted(distinct):
        add(w)
    for w in sorted(distinct):
        for c in ACGT:
            add(c + w)
    for s in sorted(set(D.strs)):
        for m in range(1, len(s) + 1):
            add(s[:m])
            add(s[len(s) - m:])
    longer = [s for s in D.strs if len(s) >= 7]
    sampled = []
    for _ in range(200 if longer else 0):
        s = longer[int(rng.integers(0, len(longer)))]
        m = int(rng.integers(7, min(64, len(s)) + 1))
        a = int(rng.integers(0, len(s) - m + 1))
        sampled.append(s[a:a + m])
        add(sampled[-1])
    short = sorted(distinct)
    for w in sampled + [short[int(i)] for i in rng.integers(0, len(short), 200)]:
        add(mixed_case(w, rng))
        add(w.lower())
    for w in ("", "N", "ACGNT"):
        add(w)
    return tuple(p.encode() for p in pats)
