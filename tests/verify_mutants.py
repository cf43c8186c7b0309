"""Near-misses of the true rows for the inverse-BWT verifiers (debwt_verify_device, debwt_fm_create, debwt_fm_open, the
host tool debwt_verify_inverse), enumerated instead of sampled, and a plain reference of the verdict.  Nothing here
calls the library.

The BWT is a function of the text, so a verifier must accept (rows below n, '#' rows, '$' row) exactly when they equal
the definition's (fm_definition.definition_index).  The collections have 383 to 1,152 rows, small enough to try every
single-row change, every adjacent swap and every move of a listed row.

Cases: the eight fm_definition.BUILDER_CASES and three more that the loader takes (every record longer than 32 bases):
  all_T_400_37_33    records of 400, 37 and 33 'T': every row holds code 3 and C['T'] is 0
  recs_30x33         thirty random records of 33 bases: n = 1,020 just clears the loader's n > nrec * 32, which is why
                     the GPU tests keep k = 32 (a smaller k would not let shorter records in: the bound is fixed)
  no_T_200_150_100   random A/C/G only: every code-3 row is a separator, the census has tot[3] == nrec

Mutant classes, each a generator of (class, words, hash_rows, dollar_row); "row" is a row below n:
  A    one base row set to each of the three other codes
  B1   rows (i, i + 1) swapped              } both rows outside the lists, their symbols differ;
  B2   rows (i, i + 32) and (i, i + 384)    } the census survives
  B3   1,000 seeded random pairs            }
  C1   a '#' row moved to the nearest 'T' row (code 3, no separator) on either side, between its neighbours in the
       list; words unchanged
  C2   the '$' row and one '#' row exchange roles; words and the set of separator rows unchanged
  C3   a '#' row moved by +-1 onto any row that is no other '#' row (the '$' row included)
  D    dollar_row set to every other row, '#' rows included
  E    the code under a separator row set to 0, 1 or 2
  F    malformed lists: descending, repeated, a '#' row >= n, dollar_row >= n
  P    bits of rows >= n in the last word set: no mutants, the verdict must not change
  T    (text_mutants) the text changes and the rows stay: every base replaced by the next code; every '#' exchanged
       with the base before or behind it where both records stay longer than 32 (the '$' stays last: a text that
       does not end in '$' cannot be loaded)"""
import collections
import functools

import numpy as np

import fm_definition as F

CLASSES = ("A", "B1", "B2", "B3", "C1", "C2", "C3", "D", "E", "F", "P")
ROW_CLASSES = CLASSES[:9]                # A .. E: the triple differs from the definition's
U64_MAX = 2**64 - 1


@functools.lru_cache(maxsize=None)
def _new_cases():
    rng = np.random.default_rng(20)
    T = lambda m: np.full(m, 3, dtype=np.uint8)                                      # noqa: E731
    c = {}
    c["all_T_400_37_33"] = [T(400), T(37), T(33)]
    c["recs_30x33"] = [rng.integers(0, 4, 33).astype(np.uint8) for _ in range(30)]
    c["no_T_200_150_100"] = [rng.integers(0, 3, m).astype(np.uint8) for m in (200, 150, 100)]
    return c


NEW_CASES = ("all_T_400_37_33", "recs_30x33", "no_T_200_150_100")
CASE_NAMES = F.BUILDER_CASES + NEW_CASES


@functools.lru_cache(maxsize=None)
def case(name):
    """the fm_definition.Definition of a case, made once"""
    return F.definition_of(name) if name in F.BUILDER_CASES else F.Definition(_new_cases()[name])


# ---- rows --------------------------------------------------------------------------------------------------------------

def _shift(r):
    return 2 * (31 - (r & 31))


def code_at(words, r):
    return (int(words[r >> 5]) >> _shift(r)) & 3


def with_codes(words, changes):
    """a copy of the words with row r set to code c for every (r, c)"""
    out = words.copy()
    for r, c in changes:
        w = int(out[r >> 5])
        out[r >> 5] = np.uint64((w & ~(3 << _shift(r))) | (c << _shift(r)))
    return out


def codes_of(words, n):
    shift = (2 * (31 - np.arange(32))).astype(np.uint64)
    return ((words[:, None] >> shift[None, :]) & np.uint64(3)).astype(np.uint8).reshape(-1)[:n]


def _u64(rows):
    return np.array(rows, dtype=np.uint64)


# ---- the mutant classes ------------------------------------------------------------------------------------------------

def _free_rows(D):
    """rows outside the lists: their symbol is their code"""
    return np.nonzero(D.L <= 3)[0]


def _gen_A(D):
    for r in _free_rows(D).tolist():
        for c in range(4):
            if c != int(D.L[r]):
                yield "A", with_codes(D.words, [(r, c)]), D.hash_rows, D.dollar_row


def _swap(D, cls, i, j):
    return cls, with_codes(D.words, [(i, int(D.L[j])), (j, int(D.L[i]))]), D.hash_rows, D.dollar_row


def _swaps(D, cls, steps):
    for d in steps:
        for i in range(D.n - d):
            a, b = int(D.L[i]), int(D.L[i + d])
            if a <= 3 and b <= 3 and a != b:
                yield _swap(D, cls, i, i + d)


def _gen_B1(D):
    return _swaps(D, "B1", (1,))


def _gen_B2(D):
    return _swaps(D, "B2", (32, 384))


def _gen_B3(D):
    rng = np.random.default_rng(D.n)
    free = _free_rows(D)
    by_code = [free[D.L[free] == c] for c in range(4)]
    if sum(1 for g in by_code if len(g)) < 2:
        return                                                  # one symbol outside the lists: no pair differs
    for _ in range(1000):
        i = int(free[rng.integers(0, len(free))])
        others = np.concatenate([g for c, g in enumerate(by_code) if c != int(D.L[i])])
        yield _swap(D, "B3", i, int(others[rng.integers(0, len(others))]))


def _gen_C1(D):
    h = [int(x) for x in D.hash_rows]
    for i, r in enumerate(h):
        below, above = (h[i - 1] if i else -1), (h[i + 1] if i + 1 < len(h) else D.n)
        t = np.nonzero(D.L[below + 1:r] == 3)[0]
        if len(t):
            yield "C1", D.words, _u64(h[:i] + [below + 1 + int(t[-1])] + h[i + 1:]), D.dollar_row
        t = np.nonzero(D.L[r + 1:above] == 3)[0]
        if len(t):
            yield "C1", D.words, _u64(h[:i] + [r + 1 + int(t[0])] + h[i + 1:]), D.dollar_row


def _gen_C2(D):
    h = [int(x) for x in D.hash_rows]
    for i, r in enumerate(h):
        yield "C2", D.words, _u64(sorted(h[:i] + h[i + 1:] + [D.dollar_row])), r


def _gen_C3(D):
    h = [int(x) for x in D.hash_rows]
    for i, r in enumerate(h):
        for to in (r - 1, r + 1):
            if 0 <= to < D.n and to not in h:
                yield "C3", D.words, _u64(h[:i] + [to] + h[i + 1:]), D.dollar_row


def _gen_D(D):
    for r in range(D.n):
        if r != D.dollar_row:
            yield "D", D.words, D.hash_rows, r


def _gen_E(D):
    for r in sorted([int(x) for x in D.hash_rows] + [D.dollar_row]):
        for c in range(3):
            yield "E", with_codes(D.words, [(r, c)]), D.hash_rows, D.dollar_row


def _gen_F(D):
    h = [int(x) for x in D.hash_rows]
    if len(h) >= 2:
        yield "F", D.words, _u64(h[::-1]), D.dollar_row                          # descending
        yield "F", D.words, _u64([h[0]] + h[:-1]), D.dollar_row                  # the first row twice
        yield "F", D.words, _u64(h[:-1] + [h[-2]]), D.dollar_row                 # the last but one twice
    if h:
        for big in (D.n, D.n + 31, U64_MAX):
            yield "F", D.words, _u64(h[:-1] + [big]), D.dollar_row               # a '#' row >= n
    for big in (D.n, D.n + 31, U64_MAX):
        yield "F", D.words, D.hash_rows, big                                     # dollar_row >= n


def _gen_P(D):
    n = D.n
    if n % 32 == 0:
        return                                                  # the last word holds rows only
    pad = list(range(n, (n + 31) // 32 * 32))
    yield "P", with_codes(D.words, [(r, 3) for r in pad]), D.hash_rows, D.dollar_row
    yield "P", with_codes(D.words, [(r, 1 + (r & 1)) for r in pad]), D.hash_rows, D.dollar_row
    yield "P", with_codes(D.words, [(pad[0], 3)]), D.hash_rows, D.dollar_row
    yield "P", with_codes(D.words, [(pad[-1], 2)]), D.hash_rows, D.dollar_row


GENERATORS = collections.OrderedDict((c, globals()["_gen_" + c]) for c in CLASSES)


def mutants(D, classes=CLASSES):
    """every mutant of the classes, class by class; hash_rows is a uint64 array, dollar_row a Python int"""
    for c in classes:
        for cls, words, hrows, drow in GENERATORS[c](D):
            yield cls, words, np.asarray(hrows, dtype=np.uint64), int(drow)


def guard_applies(D, cls, words, hrows, drow):
    """Whether a mutant is a refused input (DEBWT_EINVAL from a list check or the code-under-separator guard) rather
    than a well-formed triple that the walk has to reject.  E and F always are; of the rest only a C3 or D mutant can
    be: when the row it moves a list entry onto holds a code other than 3, or the '$' row lands among the '#' rows.
    test_verify_mutants_ref.py holds this against reference_verdict on every mutant."""
    if cls in ("E", "F"):
        return True
    if cls not in ("C3", "D"):
        return False
    rows = set(hrows.tolist())
    moved = drow if cls == "D" else (rows - set(D.hash_rows.tolist())).pop()
    return code_at(D.words, moved) != 3 or drow in rows


@functools.lru_cache(maxsize=None)
def mutant_list(name):
    """every mutant of a case, made once and left unchanged"""
    return tuple(mutants(case(name)))


def text_mutants(records):
    """("T", records) per mutated text; n and the record count stay"""
    records = [np.asarray(r, dtype=np.uint8) for r in records]
    for i, r in enumerate(records):
        for j in range(len(r)):
            m = r.copy()
            m[j] = (int(m[j]) + 1) & 3
            yield "T", records[:i] + [m] + records[i + 1:]
    for i in range(len(records) - 1):                           # the '#' between records i and i + 1
        a, b = records[i], records[i + 1]
        if len(a) - 1 > 32:                                     # exchanged with the base before it
            yield "T", records[:i] + [a[:-1], np.concatenate([a[-1:], b])] + records[i + 2:]
        if len(b) - 1 > 32:                                     # exchanged with the base behind it
            yield "T", records[:i] + [np.concatenate([a, b[:1]]), b[1:]] + records[i + 2:]


# ---- the reference -----------------------------------------------------------------------------------------------------

Verdict = collections.namedtuple("Verdict", "accepted refused")     # refused: the reason of a format refusal, or None


def reference_verdict(words, n, hash_rows, dollar_row, sym):
    """The verdict of a verifier of (words, '#' rows, '$' row) against the text sym (codes 0..5).  The format checks of
    the library's guards come first: a '$' row and strictly ascending '#' rows below n, one '#' row per '#' of the text,
    the '$' row not among them, code 3 under every listed row.  Then LF by a stable counting sort of the six symbols and
    one walk from row n - 1 (the suffix "$"): accepted exactly when the walk spells sym and ends on the '$' row."""
    sym = np.asarray(sym, dtype=np.uint8)
    assert len(sym) == n and int(sym[-1]) == F.END
    h = [int(x) for x in hash_rows]
    dollar_row = int(dollar_row)
    if dollar_row >= n:
        return Verdict(False, "'$' row outside the BWT")
    if len(h) != int(np.count_nonzero(sym == F.SEP)):
        return Verdict(False, "'#' rows: nrec - 1 rows expected")
    for i, r in enumerate(h):
        if r >= n or (i and r <= h[i - 1]) or r == dollar_row:
            return Verdict(False, "'#' rows are not ascending rows of the BWT")
    L = codes_of(np.asarray(words, dtype=np.uint64), n)
    if any(int(L[r]) != 3 for r in h + [dollar_row]):
        return Verdict(False, "a '#' row or the '$' row holds a code other than 3")
    L[np.array(h, dtype=np.int64)] = F.SEP
    L[dollar_row] = F.END
    lf = np.empty(n, dtype=np.int64)
    lf[np.argsort(L, kind="stable")] = np.arange(n)
    lf, Ll, want = lf.tolist(), L.tolist(), sym.tolist()
    r = n - 1
    for p in range(n - 1, 0, -1):
        if Ll[r] != want[p - 1]:
            return Verdict(False, None)
        r = lf[r]
    return Verdict(Ll[r] == F.END, None)


def expected_bounds(sym, sa, n, segments):
    """The segment boundaries debwt_verify_device keeps on the true rows, as (position, row): boundary j extends the
    left context of q = (j + 1) * gap one symbol at a time, up to maxm symbols and not past a '$', until exactly one
    suffix of the text starts with it; that suffix's position is kept when it lies above the previous kept position and
    below n - 1.  gap, nbound and maxm as the library computes them."""
    sym = np.asarray(sym, dtype=np.uint8)
    if not segments:
        segments = min(max(n // 16384, 1), 1 << 20)
    gap = max(n // segments, 2)
    nbound = (n - 2) // gap if n > 2 else 0
    maxm = min(max(gap // 2, 1), 1 << 16)
    row_of = np.empty(n, dtype=np.int64)
    row_of[np.asarray(sa)] = np.arange(n)
    kept, last = [], 0
    for j in range(nbound):
        q = (j + 1) * gap
        starts = np.arange(n + 1)                               # suffixes that start with the (empty) context
        pos = None
        for m in range(1, min(maxm, q) + 1):
            s = int(sym[q - m])
            if s == F.END:
                break
            starts = starts[starts > 0] - 1
            starts = starts[sym[starts] == s]
            assert len(starts)                                  # a substring of the text occurs in it
            if len(starts) == 1:
                pos = q - m
                assert int(starts[0]) == pos
                break
        if pos is not None and last < pos < n - 1:
            kept.append((pos, int(row_of[pos])))
            last = pos
    return kept


def segmented_report(words, n, hash_rows, dollar_row, sym, segments):
    """The counters of debwt_verify_device restated step by step, for rows that pass the format checks: C[] from the
    rows' own census, occ('T') = code-3 rows minus listed rows, a backward search per boundary, one walk per segment
    that stops at its first symbol mismatch, a broken link where a walk without mismatch ends on another row than the
    boundary's, the '$' check of segment 0.  Sums over boundaries and segments, so no order is involved."""
    codes = codes_of(np.asarray(words, dtype=np.uint64), n)
    h = [int(x) for x in hash_rows]
    dollar_row, nrec, symt = int(dollar_row), len(h) + 1, np.asarray(sym).tolist()
    mark = np.zeros((2, n + 1), dtype=np.int64)                 # listed rows / '#' rows below i
    mark[0, np.array(h + [dollar_row], dtype=np.int64) + 1] = 1
    mark[1, np.array(h, dtype=np.int64) + 1] = 1
    listed_below, hash_below = np.cumsum(mark, axis=1).tolist()
    cum = np.zeros((4, n + 1), dtype=np.int64)
    for s in range(4):
        cum[s, 1:] = np.cumsum(codes == s)
    tot = cum[:, n].tolist()
    C = [0, tot[0], tot[0] + tot[1], tot[0] + tot[1] + tot[2], tot[0] + tot[1] + tot[2] + tot[3] - nrec, n - 1]
    cum, codes, hash_index = cum.tolist(), codes.tolist(), {r: j for j, r in enumerate(h)}

    def occ(s, i):
        if s == F.SEP:
            return hash_below[i]
        return cum[s][i] - listed_below[i] if s == 3 else cum[s][i]

    def lf(r):
        s = codes[r]
        if s == 3 and r == dollar_row:
            return F.END, n - 1
        if s == 3 and r in hash_index:
            return F.SEP, C[4] + hash_index[r]
        return s, C[s] + occ(s, r)

    if not segments:
        segments = min(max(n // 16384, 1), 1 << 20)
    gap = max(n // segments, 2)
    nbound = (n - 2) // gap if n > 2 else 0
    maxm = min(max(gap // 2, 1), 1 << 16)
    mismatches = broken_links = search_failures = search_steps = steps = 0
    bounds, last = [(0, dollar_row)], 0
    for j in range(nbound):
        q = (j + 1) * gap
        lo, hi, pos, row = 0, n, None, 0
        for m in range(1, min(maxm, q) + 1):
            s = symt[q - m]
            if s == F.END:
                break
            lo, hi = C[s] + occ(s, lo), C[s] + occ(s, hi)
            search_steps += 1
            if hi <= lo:
                search_failures += 1
                break
            if hi - lo == 1:
                pos, row = q - m, lo
                break
        if pos is not None and last < pos < n - 1:
            bounds.append((pos, row))
            last = pos
    bounds.append((n - 1, n - 1))
    for j in range(len(bounds) - 1):
        (p0, r0), (p, r), ok = bounds[j], bounds[j + 1], True
        while p > p0:
            s, nr = lf(r)
            if s != symt[p - 1]:
                ok, mismatches = False, mismatches + 1
                break
            r, p, steps = nr, p - 1, steps + 1
        if ok and r != r0:
            ok, broken_links = False, broken_links + 1
        if ok and j == 0 and lf(r)[0] != F.END:
            mismatches += 1
    return {"segments": len(bounds) - 1, "steps": steps, "mismatches": mismatches, "broken_links": broken_links,
            "search_failures": search_failures, "search_steps": search_steps}


def report_accepts(rep, n):
    """the verdict debwt_verify_device draws from its counters"""
    return rep["mismatches"] == 0 and rep["broken_links"] == 0 and rep["search_failures"] == 0 and rep["steps"] == n - 1


def expected_segments(sym, sa, n, segments):
    """report["segments"] of debwt_verify_device on the true rows: the kept boundaries cut the text into one more"""
    return len(expected_bounds(sym, sa, n, segments)) + 1
