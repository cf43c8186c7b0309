"""A definition index with more than 2^24 records, without sorting 3 * 10^7 suffixes.  Nothing here calls the library.

The text is  L1 # L2 # L3 # (A#)^NA (T#)^(NT-1) T $ : three head records over {C, G, T} that begin and end with C or G,
then NA records of the one base A and NT records of the one base T.  Its suffix array is known once the order of the
head's few thousand suffixes is known, and that order is taken from fm_definition.definition_index of the small text
with the same head, two A records and two T records.  In row order (codes A < C < G < T < '#' < '$'):

    1. the A# suffixes, ascending by position (the one with more A records behind it is smaller)
    2. the base suffixes of the head, in the small text's order (they begin with C, G or T; a T of the head is followed
       by a base, so they stand before every T#)
    3. the T# suffixes of the one-base records, ascending by position ('#' < '$')
    4. the '#' suffixes: the head's last '#' (all NA A records follow), the '#' behind each A but the last, ascending,
       the head's other '#' in the small text's order (C or G follows), the '#' behind the last A (T follows), the '#'
       between the T records, ascending
    5. '$'

head_order() asserts what this rests on: no two neighbouring head suffixes share a prefix that reaches the first one-base
record, so every comparison among them is decided by symbols both texts hold.

With NA >= 2^24 every rank line behind the A# rows has at least 2^24 separator rows before it, so the lines of the
head's suffixes (2) and of the 'T' rows of the '#' suffixes (4) that hold no separator row take their 'T' count from the
header words, high 24 bits included.  RankModel is the rank line of verify_kernels.h in numpy with a switch that drops
those bits: it shows that a test can fail, it is no reference -- the reference is sa and sym."""
import functools
from collections import Counter

import numpy as np

import esa_ref
import fm_definition as F
import kmer_ref as KR

ROWS = F.ROWS
HIGH = 1 << 24
SEED, HEAD_LENS = 3, (2500, 2000, 1500)
FULL = (HIGH + 300, 3000)               # (NA, NT) of the large instance
SCALED = (600, 50)                      # of the instance small enough for fm_definition.Definition
A1, T1 = np.array([0], dtype=np.uint8), np.array([3], dtype=np.uint8)
CNT_MASK = (1 << 40) - 1


@functools.lru_cache(maxsize=None)
def head(seed=SEED, lens=HEAD_LENS):
    """the head records: codes 1..3, the first and the last of each 1 or 2"""
    rng = np.random.default_rng(seed)
    out = []
    for m in lens:
        r = rng.integers(1, 4, m).astype(np.uint8)
        r[0], r[-1] = rng.integers(1, 3, 2)
        r.setflags(write=False)
        out.append(r)
    return tuple(out)


def neighbour_reach(sym, order):
    """per neighbouring pair (p, q) of `order` the largest text position read to tell the two suffixes apart"""
    p, q = order[:-1], order[1:]
    h = np.zeros(len(p), dtype=np.int64)
    live = np.arange(len(p))
    while len(live):
        live = live[sym[p[live] + h[live]] == sym[q[live] + h[live]]]
        h[live] += 1
    return np.maximum(p, q) + h


def head_order(recs):
    """(positions of the head's base suffixes, positions of the head's '#' but the last), each in the order of the small
    text; the guard on that order"""
    sym, sa = F.definition_index(list(recs) + [A1, A1, T1, T1])[:2]
    H = sum(len(r) for r in recs) + len(recs)
    inside = sa[sa < H]
    bases = inside[sym[inside] <= 3]
    hashes = inside[(sym[inside] == F.SEP) & (inside < H - 1)]
    for order in (bases, hashes):
        if len(order) > 1:
            # position H holds the first 'A' in every instance; what stands behind it differs between instances
            assert (neighbour_reach(sym, order) <= H).all(), "a pair of head suffixes is told apart behind the head only"
    return bases, hashes


def analytic_index(recs, NA, NT):
    """(sym, sa) of the text with the head `recs`, NA records 'A' and NT records 'T' (NA, NT >= 1)"""
    assert NA >= 1 and NT >= 1
    assert all((r > 0).all() and r[0] in (1, 2) and r[-1] in (1, 2) for r in recs)     # rules 1, 2 and 4 rest on it
    bases, hashes = head_order(recs)
    H = sum(len(r) for r in recs) + len(recs)
    TB = H + 2 * NA                                            # the first T record
    n = TB + 2 * NT
    sym = np.empty(n, dtype=np.uint8)
    sym[:H] = F.text_symbols(list(recs))
    sym[H - 1] = F.SEP
    sym[H:TB:2], sym[H + 1:TB:2] = 0, F.SEP
    sym[TB::2], sym[TB + 1::2] = 3, F.SEP
    sym[n - 1] = F.END
    ar = lambda m: np.arange(m, dtype=np.int64)                                      # noqa: E731
    sa = np.concatenate([H + 2 * ar(NA), bases, TB + 2 * ar(NT),                                           # 1, 2, 3
                         [H - 1], H + 1 + 2 * ar(NA - 1), hashes, [TB - 1], TB + 1 + 2 * ar(NT - 1),       # 4
                         [n - 1]]).astype(np.int64)
    assert len(sa) == n
    return sym, sa


def line_profile(L):
    """fm_definition.line_profile as whole arrays: (separator rows in the line, 'T' rows in the line, separator rows
    before the line) for the n // 384 + 1 lines"""
    n = len(L)
    nl = n // ROWS + 1
    pad = np.zeros(nl * ROWS, dtype=np.uint8)
    pad[:n] = L
    g = pad.reshape(nl, ROWS)
    seps = np.count_nonzero(g > 3, axis=1).astype(np.int64)
    ts = np.count_nonzero(g == 3, axis=1).astype(np.int64)
    return seps, ts, np.cumsum(seps) - seps


class Index:
    """One instance: the definition index, the intervals of patterns from it, and the regions of its rows."""

    def __init__(self, recs, NA, NT):
        self.recs, self.NA, self.NT = recs, NA, NT
        self.head_strs = F.strings(recs)
        self.H = sum(len(r) for r in recs) + len(recs)
        self.sym, self.sa = analytic_index(recs, NA, NT)
        n = self.n = len(self.sym)
        self.nrec = len(recs) + NA + NT
        self.L = self.sym[(self.sa - 1) % n]
        self.words = F.pack_rows(self.L)
        self.hash_rows = np.nonzero(self.L == F.SEP)[0].astype(np.uint64)
        dollar = np.nonzero(self.L == F.END)[0]
        assert len(dollar) == 1
        self.dollar_row = int(dollar[0])
        self._bytes = self.sym.tobytes()
        self.seps, self.ts, self.before = line_profile(self.L)
        self.head_rows = (NA, NA + self.H - len(recs))                   # rows of the head's base suffixes
        self.tail_rows = (n - NT, n)                                     # rows of the '#' between the T records, and '$'
        for a in (self.sym, self.sa, self.L, self.words, self.hash_rows):
            a.setflags(write=False)

    # -- facts --
    def census(self):
        return np.bincount(np.minimum(self.L, 3), minlength=4).astype(np.uint64)

    def starts(self):
        seppos = np.nonzero(self.sym > 3)[0]
        return np.concatenate([[0], seppos[:-1] + 1]).astype(np.uint64)

    def record_string(self, r):
        k = len(self.recs)
        return self.head_strs[r] if r < k else "A" if r < k + self.NA else "T"

    def high_lines(self, rows=None):
        """the lines that hold 'T' rows, no separator row and have at least 2^24 separator rows before them: occ('T')
        there needs the high bits of the header; with rows = (lo, hi) only the lines that hold some of those rows"""
        ok = (self.ts > 0) & (self.seps == 0) & (self.before >= HIGH)
        b = np.nonzero(ok)[0]
        if rows is not None:
            b = b[((b + 1) * ROWS > rows[0]) & (b * ROWS < rows[1])]
        return b

    # -- rows --
    def interval(self, p):
        """[lo, hi) of the rows whose suffix starts with p (str or bytes, either case), by binary search over sa with byte
        compares of sym; (0, 0) for an empty pattern and for one with a character outside ACGTacgt"""
        if isinstance(p, str):
            p = p.encode()
        if not p:
            return 0, 0
        c = F._LUT[np.frombuffer(p, dtype=np.uint8)]
        if (c > 3).any():
            return 0, 0
        key, m, b, sa = c.tobytes(), len(p), self._bytes, self.sa
        ends = []
        for above in (False, True):                                      # first row >= key, first row > key
            lo, hi = 0, self.n
            while lo < hi:
                mid = (lo + hi) >> 1
                s = b[int(sa[mid]):int(sa[mid]) + m]
                if s > key if above else s >= key:
                    hi = mid
                else:
                    lo = mid + 1
            ends.append(lo)
        return ends[0], ends[1]


@functools.lru_cache(maxsize=None)
def index(NA=FULL[0], NT=FULL[1], seed=SEED, lens=HEAD_LENS):
    return Index(head(seed, lens), NA, NT)


@functools.lru_cache(maxsize=None)
def esa(NA=FULL[0], NT=FULL[1], seed=SEED, lens=HEAD_LENS):
    """da, d, lcp, summary and profile of the instance"""
    X = index(NA, NT, seed, lens)
    return esa_ref.Esa.from_index(X.sym, X.sa)


@functools.lru_cache(maxsize=None)
def scaled(seed=SEED, lens=HEAD_LENS):
    """The same head with 600 A records and 50 T records as a fm_definition.Definition: the hit strings, mismatch counts,
    MEM spans and overlap flags of the large instance are those of this one, by brute force; only rows and record numbers
    differ."""
    recs = head(seed, lens)
    D = F.Definition(list(recs) + [A1] * SCALED[0] + [T1] * SCALED[1])
    X = index(SCALED[0], SCALED[1], seed, lens)
    assert np.array_equal(D.sa, X.sa) and np.array_equal(D.sym, X.sym)
    return D


# ---- the rank line in numpy --------------------------------------------------------------------------------------------

class RankModel:
    """k_vidx_write's line header and the three ways the kernels read it, as far as they differ: occ() is v_occ and
    fm_occ2 (one code from its header word), occ4() is fm_line_occ4 (codes 1..3 counted, code 0 by subtraction).  With
    drop_high the separators-before count of a line without separator rows is read from header[0] alone."""

    def __init__(self, X):
        self.X, n = X, X.n
        self.code = np.minimum(X.L, 3)
        nl = n // ROWS + 1
        pad = np.full(nl * ROWS, 9, dtype=np.uint8)
        pad[:n] = self.code
        g = pad.reshape(nl, ROWS)
        per = np.stack([np.count_nonzero(g == c, axis=1) for c in range(4)], axis=1).astype(np.uint64)
        before = np.cumsum(per, axis=0, dtype=np.uint64) - per
        self.srows = np.sort(np.concatenate([X.hash_rows, [X.dollar_row]]).astype(np.int64))
        sb, sin = X.before.astype(np.uint64), X.seps.astype(np.uint64)
        s40 = np.uint64(40)
        self.hdr = np.stack([before[:, 0] | ((sb & np.uint64(0xFFFFFF)) << s40),
                             before[:, 1] | (((sb >> np.uint64(24)) & np.uint64(0xFFFFFF)) << s40),
                             before[:, 2] | (sin << s40), before[:, 3]], axis=1)
        tot = before[-1] + per[-1]
        nt = int(tot[3]) - len(self.srows)                               # 'T' rows
        self.C = [0, int(tot[0]), int(tot[0] + tot[1]), int(tot[0] + tot[1] + tot[2])]
        self.C += [self.C[3] + nt, n - 1]

    def _sep(self, b, i, drop_high):
        h = self.hdr[b]
        if int(h[2]) >> 40:
            return int(np.searchsorted(self.srows, i, side="left"))
        low, high = (int(h[0]) >> 40) & 0xFFFFFF, (int(h[1]) >> 40) & 0xFFFFFF
        return low if drop_high else low | (high << 24)

    def occ(self, s, i, drop_high=False):
        b = i // ROWS
        cnt = (int(self.hdr[b, s]) & CNT_MASK) + int(np.count_nonzero(self.code[b * ROWS:i] == s))
        return cnt - self._sep(b, i, drop_high) if s == 3 else cnt

    def occ4(self, i, drop_high=False):
        b = i // ROWS
        part = self.code[b * ROWS:i]
        c = [int(np.count_nonzero(part == s)) for s in (1, 2, 3)]
        h = self.hdr[b]
        return [(int(h[0]) & CNT_MASK) + (i - b * ROWS - sum(c)), (int(h[1]) & CNT_MASK) + c[0],
                (int(h[2]) & CNT_MASK) + c[1], (int(h[3]) & CNT_MASK) + c[2] - self._sep(b, i, drop_high)]

    def backward(self, p, drop_high=False, four=False):
        """(lo, hi) of k_fm_count's loop over pattern p (bytes or str of ACGT, either case), and the kinds of its 'T' steps
        that read a line of X.high_lines(): "one" when lo and hi lie in one line, "two" when they do not"""
        if isinstance(p, str):
            p = p.encode()
        high = self._high()
        lo, hi, kinds = 0, self.X.n if p else 0, set()
        for ch in reversed(p):
            if lo >= hi:
                break
            s = int(F._LUT[ch])
            if s > 3:
                return (0, 0), kinds
            if s == 3 and (lo // ROWS in high or hi // ROWS in high):
                kinds.add("one" if lo // ROWS == hi // ROWS else "two")
            if four:
                lo, hi = self.C[s] + self.occ4(lo, drop_high)[s], self.C[s] + self.occ4(hi, drop_high)[s]
            else:
                lo, hi = self.C[s] + self.occ(s, lo, drop_high), self.C[s] + self.occ(s, hi, drop_high)
        return (lo, max(lo, hi)), kinds

    @functools.lru_cache(maxsize=None)
    def _high(self):
        return frozenset(self.X.high_lines().tolist())

    def lf(self, r, drop_high=False):
        """v_lf: (the row of the suffix one position earlier, the symbol of row r)"""
        s, X = int(self.code[r]), self.X
        if s == 3 and int(self.hdr[r // ROWS, 2]) >> 40:
            if r == X.dollar_row:
                return X.n - 1, F.END
            j = int(np.searchsorted(X.hash_rows, r))
            if j < len(X.hash_rows) and int(X.hash_rows[j]) == r:
                return self.C[4] + j, F.SEP
        return self.C[s] + self.occ(s, r, drop_high), s


@functools.lru_cache(maxsize=None)
def model(NA=FULL[0], NT=FULL[1]):
    return RankModel(index(NA, NT))


# ---- what the GPU tests send --------------------------------------------------------------------------------------------

SHORT_PATTERNS = ("A", "T", "C", "AA", "AT", "TA", "TT")


@functools.lru_cache(maxsize=None)
def range_patterns():
    """Every distinct substring of the head up to length 4, 300 sampled substrings of 5..64 bases, each of them with each
    base in front, the short patterns around the one-base records, mixed case and a pattern with N; as bytes."""
    strs = F.strings(head())
    rng = np.random.default_rng(24)
    pats = {}
    distinct = sorted({s[i:i + m] for s in strs for m in range(1, 5) for i in range(len(s) - m + 1)})
    sampled = []
    for _ in range(300):
        s = strs[int(rng.integers(0, len(strs)))]
        m = int(rng.integers(5, 65))
        a = int(rng.integers(0, len(s) - m + 1))
        sampled.append(s[a:a + m])
    for w in distinct + sampled:
        pats[w] = None
    for w in distinct + sampled:
        for c in F.ACGT:
            pats[c + w] = None
    for w in SHORT_PATTERNS:
        pats[w] = None
    for w in sampled[:40]:
        pats[F.mixed_case(w, rng)] = None
        pats[w.lower()] = None
    for w in ("", "N", "CGNT", sampled[0][:9] + "N" + sampled[0][10:]):
        pats[w] = None
    return tuple(p.encode() for p in pats)


@functools.lru_cache(maxsize=None)
def locate_patterns():
    """200 head substrings of 12..40 bases (each occurs once or a few times): the rows the sa_sample = 1024 test walks"""
    strs = F.strings(head())
    rng = np.random.default_rng(1024)
    out = {}
    while len(out) < 200:
        s = strs[int(rng.integers(0, len(strs)))]
        m = int(rng.integers(12, 41))
        a = int(rng.integers(0, len(s) - m + 1))
        out[s[a:a + m]] = None
    return tuple(p.encode() for p in out)


def tail_t_rows(X, count=64):
    """`count` rows that hold 'T' in the lines of X.high_lines(X.tail_rows), spread over them"""
    lines = X.high_lines(X.tail_rows)
    rows = np.concatenate([b * ROWS + np.nonzero(X.L[b * ROWS:(b + 1) * ROWS] == 3)[0] for b in lines.tolist()])
    return rows[np.linspace(0, len(rows) - 1, count).astype(np.int64)]


@functools.lru_cache(maxsize=None)
def reads():
    """40 reads of 24..60 bases cut from the head with up to two substitutions, every fifth in lower case, every eighth
    as its reverse complement (the head holds no 'A', so a read has hits on one strand only), one with an N"""
    strs = F.strings(head())
    rng = np.random.default_rng(40)
    out = []
    for i in range(40):
        s = strs[i % len(strs)]
        m = int(rng.integers(24, 61))
        a = int(rng.integers(0, len(s) - m + 1))
        t = list(s[a:a + m])
        for j in rng.integers(0, m, i % 3).tolist():
            t[j] = F.ACGT[(F.ACGT.index(t[j]) + 1 + int(rng.integers(0, 3))) % 4]
        if i == 7:
            t[m // 2] = "N"
        r = "".join(t)
        if i % 8 == 3:
            r = F.revcomp(r)
        out.append(r.lower() if i % 5 == 4 else r)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def search_reference(NA=FULL[0], NT=FULL[1]):
    """per read the hits at K = 2 on both strands as (lo, hi, mismatches, strand), sorted as Definition.search sorts them:
    strings and mismatch counts from the scaled instance, rows from this instance's sa"""
    D, X = scaled(), index(NA, NT)
    out = []
    for p in reads():
        hits = []
        for strand, q in ((0, p), (1, F.revcomp(p))):
            for w, d in D._windows(q.upper(), 2).items():
                hits.append(X.interval(w) + (d, strand))
        out.append(sorted(hits, key=lambda h: (h[3], h[2], h[0])))
    return tuple(out)


def kmer_ref(k, both, NA=FULL[0], NT=FULL[1]):
    """kmer_ref.Ref over the head; for k = 1 the one-base records are added"""
    R = KR.Ref(F.strings(head()), k, both)
    if k == 1:
        R.c["A"] += NA
        R.c["T"] += NT
    return R


def kmer_occ(k, NA=FULL[0], NT=FULL[1]):
    """Counter of the k-mers inside records"""
    return Counter(kmer_ref(k, False, NA, NT).c)
