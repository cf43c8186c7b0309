"""Definition 12 written out on the CPU: prev, dup, the prefix P, records(lo, hi) and the multi-MUMs of a collection, from
esa_ref.Esa and repeat_ref.intervals alone.  Nothing here calls the library, and there is no sort by record and no
hierarchy: prev comes from one pass over da with a dictionary, the leftmost argmin from np.argmin of the slice (which
answers the first of equal values), so the kernels' way of getting either is not repeated here.

    prev[r]          the largest r' < r with da[r'] == da[r], -1 without one
    dup[m]           the rows r that have a prev and whose leftmost argmin of lcp[prev[r]+1 .. r] is m
    P[r]             dup[0] + .. + dup[r]
    closed [lo, hi)  hi - lo <= 1, or every lcp[lo+1 .. hi-1] above lcp[lo] and above lcp[hi] (hi < n)
    records(lo, hi)  0 for an empty range, else (hi - lo) - (P[hi-1] - P[lo])
    multi-MUM        a maximal interval with count == records >= q (q: every record by default)

facts() asserts fact 4: for a closed range records(lo, hi) is the number of distinct values of da[lo .. hi)."""
import functools

import numpy as np

import fm_definition as F
import repeat_ref as RR


def prev_rows(da):
    last, prev = {}, np.full(len(da), -1, dtype=np.int64)
    for r, d in enumerate(np.asarray(da).tolist()):
        prev[r] = last.get(d, -1)
        last[d] = r
    return prev


@functools.lru_cache(maxsize=None)
def dup(E, max_lcp=0):
    lcp = E.lcp(max_lcp)
    out = np.zeros(E.n, dtype=np.int64)
    for r, p in enumerate(prev_rows(E.da).tolist()):
        if p >= 0:
            out[p + 1 + int(np.argmin(lcp[p + 1:r + 1]))] += 1
    assert int(out.sum()) == E.n - len(np.unique(E.da)) and out[0] == 0
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def prefix(E, max_lcp=0):
    """P as the library keeps and fetches it"""
    P = np.cumsum(dup(E, max_lcp)).astype(np.uint64)
    P.setflags(write=False)
    return P


def records(P, lo, hi):
    """the formula, for closed ranges and for others"""
    lo, hi = int(lo), int(hi)
    return 0 if hi <= lo else (hi - lo) - (int(P[hi - 1]) - int(P[lo]))


def records_of(P, ranges):
    """as debwt_fm_record_counts answers: u64 arithmetic, so the formula of a range that is not closed may wrap"""
    return np.array([records(P, lo, hi) % 2 ** 64 for lo, hi in np.asarray(ranges).reshape(-1, 2).tolist()], dtype=np.uint64)


def is_closed(lcp, lo, hi):
    n = len(lcp)
    if hi - lo <= 1:
        return True
    inner = lcp[lo + 1:hi]
    return bool((inner > lcp[lo]).all() and (hi == n or (inner > lcp[hi]).all()))


def distinct(E, lo, hi):
    return len(set(E.da[int(lo):int(hi)].tolist()))


def interval_records(E, max_lcp=0):
    """records of every interval of repeat_ref.intervals(E, max_lcp), in its order"""
    rec = RR.intervals(E, max_lcp)[0]
    P = prefix(E, max_lcp)
    return records_of(P, np.stack([rec["row_lo"], rec["row_lo"] + rec["count"]], axis=1)) if len(rec) else np.zeros(0, np.uint64)


def pattern_range(E, r, k, max_lcp=0):
    """the rows whose suffixes share their first k bases with row r (k <= d[r], k <= cap): what debwt_fm_count answers
    for that string"""
    lcp = E.lcp(max_lcp)
    lo = int(np.nonzero(lcp[:r + 1] < k)[0][-1])
    right = np.nonzero(lcp[r + 1:] < k)[0]
    return lo, (r + 1 + int(right[0])) if len(right) else E.n


def facts(E, max_lcp=0, seeded=200):
    """asserts fact 4 on one collection: every interval, and `seeded` ranges of strings taken from the rows (single rows
    among them: closed ranges that are no interval)"""
    lcp, P = E.lcp(max_lcp), prefix(E, max_lcp)
    rec = RR.intervals(E, max_lcp)[0]
    got = interval_records(E, max_lcp)
    for x, g in zip(rec, got.tolist()):
        lo, hi = int(x["row_lo"]), int(x["row_lo"] + x["count"])
        assert is_closed(lcp, lo, hi) and g == distinct(E, lo, hi), (lo, hi)
    rng = np.random.default_rng(E.n + max_lcp)
    cap = max_lcp if max_lcp else 1 << 30
    singles = 0
    for r in rng.integers(0, E.n, seeded).tolist():
        top = min(int(E.d[r]), cap)
        if top < 1:
            continue
        k = int(rng.integers(1, top + 1))
        lo, hi = pattern_range(E, r, k, max_lcp)
        assert lo <= r < hi and is_closed(lcp, lo, hi), (r, k)
        assert records(P, lo, hi) == distinct(E, lo, hi), (r, k)
        singles += hi - lo == 1
    for r in range(min(E.n, 50)):
        assert records(P, r, r + 1) == 1 and records(P, r, r) == 0
    return len(rec), singles


def repeats(E, min_len=1, min_occ=2, max_occ=None, kind="maximal", min_records=1, max_records=None, unique=False, max_lcp=0):
    """(list, records) as debwt_fm_repeats_records answers"""
    every, rc = RR.intervals(E, max_lcp)[0], interval_records(E, max_lcp)
    keep = (every["len"] >= min_len) & (every["count"] >= min_occ)
    if max_occ:
        keep &= every["count"] <= max_occ
    if kind != "intervals":
        keep &= (every["flags"] & (RR.IS_MAXIMAL if kind == "maximal" else RR.IS_SUPERMAXIMAL)) != 0
    keep &= rc >= min_records
    if max_records:
        keep &= rc <= max_records
    if unique:
        keep &= rc == every["count"]
    return every[keep], rc[keep].astype(np.uint32)


def mums(E, min_len=20, min_records=None, max_lcp=0):
    q = len(E.records) if min_records is None else int(min_records)
    return repeats(E, min_len=min_len, min_occ=max(q, 2), kind="maximal", min_records=q, unique=True, max_lcp=max_lcp)


def mum_strings(E, rec):
    """{string: ((record, offset), ...) ascending by record} of a list of multi-MUMs"""
    out = {}
    for x, w in zip(rec, RR.strings_of(E, rec)):
        lo, hi = int(x["row_lo"]), int(x["row_lo"] + x["count"])
        out[w] = tuple(sorted(E.resolve(int(p)) for p in E.sa[lo:hi].tolist()))
    return out


def occurrences(s, w):
    out, at = [], s.find(w)
    while at >= 0:
        out.append(at)
        at = s.find(w, at + 1)
    return out


def brute_mums(E, min_len=1):
    """The multi-MUMs from the record strings alone: a string that occurs exactly once in every record, whose left
    neighbours are not all the same base and whose right neighbours are not either (a record's start and end are symbols
    of their own, different in every record).  {string: ((record, offset), ...)}"""
    strs = F.strings(E.records)
    first, out = strs[0], {}
    for a in range(len(first)):
        for b in range(a + max(min_len, 1), len(first) + 1):
            w = first[a:b]
            occ = [occurrences(s, w) for s in strs]
            if any(len(o) != 1 for o in occ):
                if any(len(o) == 0 for o in occ):
                    break                                              # no longer string from a occurs everywhere
                continue
            at = [o[0] for o in occ]
            lefts = {s[p - 1] if p else ("start", j) for j, (s, p) in enumerate(zip(strs, at))}
            rights = {s[p + len(w)] if p + len(w) < len(s) else ("end", j) for j, (s, p) in enumerate(zip(strs, at))}
            if len(lefts) > 1 and len(rights) > 1:
                out[w] = tuple((j, p) for j, p in enumerate(at))
    return out


def mutated_copies(seed, copies=3, length=150, rate=0.05):
    """`copies` records: one random genome and copies of it with substitutions at `rate`"""
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 4, length).astype(np.uint8)
    out = [base]
    for _ in range(copies - 1):
        c = base.copy()
        hit = rng.random(length) < rate
        c[hit] = (c[hit] + rng.integers(1, 4, int(hit.sum()))) % 4
        out.append(c.astype(np.uint8))
    return out
