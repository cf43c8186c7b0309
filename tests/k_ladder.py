"""Two texts whose structure changes at every k from 12 to 32 (plain numpy, seeded, no GPU).

The BWT of a collection does not depend on k, what the build does on its way there does: the node length K = k - 1 decides
which nodes repeat, branch or stand at a record end.  The goldens repeat at lengths above 32 only, so their counters are the
same number at every k; these texts hold, for every length from 10 to 34, something that exists at that length alone:

  units      for every L in 10..34 one random unit of L bases, three times between random flanks of 3..8 bases
  tandems    for every period p in 1..33 a tandem repeat of 35 + 2p bases at the least
  ends       for every L in 10..34 two records of 33..60 bases that end in the same L bases and differ in front of them
             (the record-end context of the special-region module)
  starts     for L = 10, 13, ..., 34 two records that begin with the same L bases and differ behind them
  the rest   one exact duplicate record, one record of 70 x G, one record of 33 x A plus 10 random bases

small(): those records, about 10 k symbols -- the naive suffix sort stays cheap.  mid(): the same records plus three
30,000-base near-copies of one random record (0.5 % substitutions), about 100 k symbols: more than the 2^14 keys at which
the hybrid sort takes two prefix digits.  Every record is longer than 32 bases.

tests/test_k_ladder_ref.py proves on the CPU, with the oracle alone, that the texts do what the GPU tests rely on."""
import functools

import numpy as np

KS = tuple(range(12, 33))
SEED = 1


def node_keys(recs, k):
    """(node << 2 | pred) of every main position, by definition: the one of tests/test_gpu_parity.py."""
    from test_gpu_parity import _node_keys
    return _node_keys(recs, k)


def _records(rng):
    rnd = lambda m: rng.integers(0, 4, size=int(m)).astype(np.uint8)               # noqa: E731
    other = lambda c: np.uint8((int(c) + int(rng.integers(1, 4))) & 3)             # noqa: E731 -- any base but c
    flank = lambda: rnd(rng.integers(3, 9))                                        # noqa: E731
    parts = [flank()]
    for L in range(10, 35):                                    # units: an exact repeat of L bases, three copies
        unit = rnd(L)
        for _ in range(3):
            parts += [unit, flank()]
    for p in range(1, 34):                                     # tandem repeats of every period up to 33
        reps = -(-(35 + 2 * p) // p)
        parts += [np.tile(rnd(p), reps), flank()]
    recs = [np.concatenate(parts)]
    for L in range(10, 35):                                    # shared record ends of exactly L bases
        end = rnd(L)
        a = np.concatenate([rnd(max(int(rng.integers(33, 61)), L + 2) - L), end])
        b = np.concatenate([rnd(max(int(rng.integers(33, 61)), L + 2) - L), end])
        b[len(b) - L - 1] = other(a[len(a) - L - 1])
        recs += [a, b]
    for L in range(10, 35, 3):                                 # shared record starts of exactly L bases
        start = rnd(L)
        a = np.concatenate([start, rnd(max(int(rng.integers(33, 61)), L + 2) - L)])
        b = np.concatenate([start, rnd(max(int(rng.integers(33, 61)), L + 2) - L)])
        b[L] = other(a[L])
        recs += [a, b]
    dup = rnd(47)
    recs += [dup, dup.copy(), np.full(70, 2, dtype=np.uint8), np.concatenate([np.zeros(33, dtype=np.uint8), rnd(10)])]
    return recs


@functools.lru_cache(maxsize=None)
def small():
    recs = _records(np.random.default_rng(SEED))
    for r in recs:
        r.setflags(write=False)
    return tuple(recs)


@functools.lru_cache(maxsize=None)
def mid():
    rng = np.random.default_rng(SEED + 1000)
    base = rng.integers(0, 4, size=30_000).astype(np.uint8)
    copies = []
    for _ in range(3):
        cp = base.copy()
        hit = rng.random(len(cp)) < 0.005
        cp[hit] = (cp[hit] + rng.integers(1, 4, size=int(hit.sum())).astype(np.uint8)) & 3
        cp.setflags(write=False)
        copies.append(cp)
    return small() + tuple(copies)


TEXTS = {"small": small, "mid": mid}


def records(name):
    return list(TEXTS[name]())


def n_symbols(name):
    recs = TEXTS[name]()
    return sum(len(r) for r in recs) + len(recs)


@functools.lru_cache(maxsize=None)
def sorted_keys(name, k):
    """np.sort of the keys of a text by definition (read-only; shared by the tests that need it)"""
    want = np.sort(node_keys(records(name), k))
    want.setflags(write=False)
    return want


class Expected:
    """What the oracle gives for a text: words / hrows / drow / rows once (they do not depend on k -- checked, not
    assumed: every k's build is compared with the first), and stats, SP symbols and red array per k."""

    def __init__(self, recs):
        from oracle import oracle as O
        self.sym = O.sym_from_codes(recs)
        self.n = len(self.sym)
        self.stats, self.sp, self.red, self.k_invariant = {}, {}, {}, True
        for k in KS:
            w, h, d, st, sp, red = O.build_bwt(self.sym, k, want_intermediates=True)
            if k == KS[0]:
                self.words, self.hrows, self.drow = w, h, d
            elif not (np.array_equal(w, self.words) and np.array_equal(h, self.hrows) and d == self.drow):
                self.k_invariant = False
            self.stats[k], self.sp[k], self.red[k] = st, sp, red
        self.rows = O.unpack_bwt(self.words, self.n, self.hrows, self.drow)
        for a in (self.words, self.hrows, self.rows, *self.sp.values(), *self.red.values()):
            a.setflags(write=False)

    def same_bwt(self, words, hrows, drow):
        return bool(np.array_equal(words, self.words) and np.array_equal(hrows, self.hrows) and drow == self.drow)


@functools.lru_cache(maxsize=None)
def expected(name):
    return Expected(records(name))
