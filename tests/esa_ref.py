"""Definition 10 written out on the CPU: suffix array, record array, LCP array, summary and profile of a collection, from
fm_definition alone (definition_index for the small texts, suffix_array by prefix doubling for the larger ones).  Nothing
here calls the library, and the LCP values are taken by comparing the two suffixes of every pair of neighbouring rows
symbol by symbol: no carry, no chunk, so the kernel's way of getting them is not repeated here.

    sa[r]   text position of the suffix of row r
    da[r]   the record that holds sa[r]; a separator belongs to the record in front of it
    d[r]    d(sa[r]): the bases from sa[r] up to the next separator
    lcp[r]  0 for r = 0, else the largest h <= min(d[r-1], d[r]) with T[sa[r-1] .. +h) == T[sa[r] .. +h)

facts() asserts the three facts the kernels rest on."""
import functools

import numpy as np

import fm_definition as F

U32_MAX = 2 ** 32 - 1
KMAX = 4096
SMALL = 2000                   # up to here the suffixes are sorted as byte strings (definition_index)


class Esa:
    def __init__(self, records, sa=None):
        self.records = [np.asarray(r, dtype=np.uint8) for r in records]
        sym = F.text_symbols(self.records)
        if sa is None:
            sa = F.definition_index(self.records)[1] if len(sym) <= SMALL else F.suffix_array(sym)
        self._arrays(sym, sa)

    @classmethod
    def from_index(cls, sym, sa):
        """The second way in: the text as codes 0..5 and its suffix array, for a collection of so many records that a
        list of them is not made (many_records_ref).  records is None then; everything else is as __init__ leaves it."""
        E = cls.__new__(cls)
        E.records = None
        E._arrays(np.asarray(sym, dtype=np.uint8), sa)
        return E

    def _arrays(self, sym, sa):
        self.sym = sym
        n = self.n = len(sym)
        self.sa = np.asarray(sa, dtype=np.int64)
        assert np.array_equal(np.sort(self.sa), np.arange(n))
        self.seppos = np.nonzero(self.sym > 3)[0].astype(np.int64)
        self.starts = np.concatenate([[0], self.seppos[:-1] + 1]).astype(np.int64)
        rec = np.searchsorted(self.seppos, self.sa, side="left")        # the first separator at or behind the position
        self.da = rec.astype(np.uint32)
        self.d = self.seppos[rec] - self.sa
        self.lcp_full = self._lcp()

    def _lcp(self):
        """the definition, all rows at once: a pair stays in the round while its next two symbols are bases and equal"""
        n, sym, sa, d = self.n, self.sym, self.sa, self.d
        h = np.zeros(n, dtype=np.int64)
        lim = np.zeros(n, dtype=np.int64)
        lim[1:] = np.minimum(d[:-1], d[1:])
        rows = np.nonzero(lim > 0)[0]
        while len(rows):
            rows = rows[h[rows] < lim[rows]]
            rows = rows[sym[sa[rows - 1] + h[rows]] == sym[sa[rows] + h[rows]]]
            h[rows] += 1
        return h

    def lcp(self, max_lcp=0):
        """the stored array: min(lcp, cap) as uint32"""
        return np.minimum(self.lcp_full, cap_of(max_lcp)).astype(np.uint32)

    def summary(self, max_lcp=0):
        cap = cap_of(max_lcp)
        st = np.minimum(self.lcp_full, cap)
        mx = int(st.max())
        row = int(np.nonzero(st == mx)[0][0])
        return {"n": self.n, "max": mx, "max_row": row, "sum": int(st.sum()),
                "capped": int(np.count_nonzero(st == cap)) if max_lcp else 0,
                "pos_prev": int(self.sa[row - 1 if row else 0]), "pos": int(self.sa[row]), "cap": cap}

    def profile(self, kmax, max_lcp=0):
        """distinct[k - 1] = #{ r : lcp[r] < k <= d[r] } for k = 1 .. kmax; needs kmax <= cap"""
        assert 1 <= kmax <= min(cap_of(max_lcp), KMAX)
        st = np.minimum(self.lcp_full, cap_of(max_lcp))
        return [int(np.count_nonzero((st < k) & (k <= self.d))) for k in range(1, kmax + 1)]

    def plcp(self, max_lcp=0):
        out = np.zeros(self.n, dtype=np.int64)
        out[self.sa] = np.minimum(self.lcp_full, cap_of(max_lcp))
        return out

    def resolve(self, p):
        """(record, offset) of a text position"""
        j = int(np.searchsorted(self.seppos, p, side="left"))
        return j, int(p - self.starts[j])


def cap_of(max_lcp):
    return int(max_lcp) if max_lcp else U32_MAX


def compare_bound(E, chunk, max_lcp=0):
    """The most symbol pairs a chunked Kasai walk may examine, a whole word step counting 32: per position the growth of
    the match length over what it starts from, h_start[i] = max(plcp[i-1] - 1, 0) and 0 at a chunk's first position, plus
    two words of over-read."""
    p = E.plcp(max_lcp)
    start = np.zeros(E.n, dtype=np.int64)
    start[1:] = np.maximum(p[:-1] - 1, 0)
    start[np.arange(0, E.n, int(chunk))] = 0
    assert (p >= start).all()                                           # fact 2
    return int((p - start).sum()) + 64 * E.n


def cut_common_prefix(E, p, q):
    """of the suffixes at positions p and q, by the definition"""
    sym, h = E.sym, 0
    while sym[p + h] <= 3 and sym[q + h] <= 3 and sym[p + h] == sym[q + h]:
        h += 1
    return h


def brute_distinct(E, k):
    """the number of distinct strings of k bases inside records"""
    seen = set()
    for s in F.strings(E.records):
        for i in range(len(s) - k + 1):
            seen.add(s[i:i + k])
    return len(seen)


def facts(E, caps=(0, 1, 7), pairs=400, ks=(1, 2, 3, 5, 8, 13)):
    """asserts the three facts of Definition 10 on one collection"""
    n, sa, lcp = E.n, E.sa, E.lcp_full
    # 1. range minimum: every pair of rows up to 3 apart, and `pairs` seeded pairs
    rng = np.random.default_rng(n)
    todo = [(a, b) for a in range(n) for b in range(a + 1, min(a + 4, n))]
    if n > 1:
        for _ in range(pairs):
            a, b = sorted(int(x) for x in rng.integers(0, n, 2))
            if a < b:
                todo.append((a, b))
    for a, b in todo:
        assert cut_common_prefix(E, int(sa[a]), int(sa[b])) == int(lcp[a + 1:b + 1].min()), (a, b)
    # 2. Kasai's carry, for the capped values too
    for c in caps:
        p = E.plcp(c)
        assert (p[1:] >= p[:-1] - 1).all(), c
    # 3. distinct k-mers from the array (k <= cap)
    for k in ks:
        assert E.profile(k)[k - 1] == brute_distinct(E, k), k
        if k <= 7:
            assert E.profile(k, 7)[k - 1] == brute_distinct(E, k), k


@functools.lru_cache(maxsize=None)
def of_case(name):
    """the Esa of a geometry case, made once (its suffix array is the one of fm_definition.definition_of)"""
    D = F.definition_of(name)
    return Esa(D.records, D.sa)


@functools.lru_cache(maxsize=None)
def of_read_set():
    from kmer_ref import read_set
    from overlap_ref import codes
    return Esa(codes(read_set()["records"]))


@functools.lru_cache(maxsize=None)
def of_homopolymer(m=20000):
    return Esa([np.full(m, 3, dtype=np.uint8)])
