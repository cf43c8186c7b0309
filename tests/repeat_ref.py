"""Definition 11 written out on the CPU: the intervals of an LCP array, their left counts, the maximal and the supermaximal
repeats, from esa_ref.Esa alone.  Nothing here calls the library, and there is no hierarchy and no search: one pass over
the array with a stack closes every interval when a smaller value arrives, so the kernel's way of finding the interval
ends is not repeated here.

    interval (l, i, j)  l >= 1, i < j, lcp[i] < l, (j = n - 1 or lcp[j + 1] < l), min(lcp[i+1 .. j]) = l
    rep                 the smallest r in (i, j] with lcp[r] = l
    left[c]             rows of [i, j] whose BWT symbol is base c (c = 0..3) or a separator (c = 4)
    maximal             max(left[0..3]) < j - i + 1
    supermaximal        every lcp[i+1 .. j] == l and every left[0..3] <= 1

brute(E) takes the same three sets from the record strings alone: every substring with two or more occurrences, its sets
of left and right neighbours with record starts and ends as symbols of their own."""
import functools

import numpy as np

import esa_ref as ER
import fm_definition as F

IS_MAXIMAL, IS_SUPERMAXIMAL = 1, 2
KINDS = ("maximal", "supermaximal", "intervals")
DTYPE = np.dtype([("row_lo", "<u8"), ("count", "<u8"), ("left", "<u8", (5,)), ("len", "<u4"), ("flags", "<u4")])
assert DTYPE.itemsize == 64


def bwt_symbols(E):
    """L[r], the symbol in front of sa[r]; '$' in front of position 0"""
    return E.sym[(E.sa - 1) % E.n]


@functools.lru_cache(maxsize=None)
def intervals(E, max_lcp=0):
    """(records, rep, capped): every interval of the stored array below the cap as DTYPE records, ascending by
    representative row; their representatives; the number of intervals whose stored value is the cap"""
    n = E.n
    lcp = E.lcp(max_lcp).astype(np.int64).tolist()
    out = []                                                            # (l, i, j, rep, flat)
    stack = []                                                          # [l, i, rep, flat]: open intervals, l ascending
    for r in range(1, n + 1):
        cur = lcp[r] if r < n else 0
        i, child = r - 1, False
        while stack and stack[-1][0] > cur:
            l, i, rep, flat = stack.pop()
            out.append((l, i, r - 1, rep, flat))
            child = True
            if stack and stack[-1][0] > cur:
                stack[-1][3] = False                                    # the one below holds what was closed
        if cur > 0:
            if not stack or stack[-1][0] < cur:
                stack.append([cur, i, r, not child])                    # the rows of (i, r) were above cur: r is the first
            elif child:
                stack[-1][3] = False
    assert not stack
    a = np.array(out, dtype=np.int64).reshape(-1, 5)
    a = a[np.argsort(a[:, 3], kind="stable")]
    l, i, j, rep, flat = a.T
    assert len(np.unique(rep)) == len(rep)
    Lc = np.minimum(bwt_symbols(E), 4)
    cum = np.zeros((5, n + 1), dtype=np.int64)
    for c in range(5):
        cum[c, 1:] = np.cumsum(Lc == c)
    left = (cum[:, j + 1] - cum[:, i]).T
    count = j - i + 1
    assert (left.sum(axis=1) == count).all()
    top = left[:, :4].max(axis=1) if len(a) else np.zeros(0, dtype=np.int64)
    maximal = top < count
    sup = flat.astype(bool) & (top <= 1)
    assert not (sup & ~maximal).any()
    keep = l < ER.cap_of(max_lcp) if max_lcp else np.ones(len(a), dtype=bool)
    rec = np.zeros(len(a), dtype=DTYPE)
    rec["row_lo"], rec["count"], rec["left"], rec["len"] = i, count, left, l
    rec["flags"] = maximal * IS_MAXIMAL + sup * IS_SUPERMAXIMAL
    rec, reps = rec[keep], rep[keep]
    rec.setflags(write=False)
    reps.setflags(write=False)
    return rec, reps, int(len(a) - keep.sum())


def repeats(E, min_len=1, min_occ=2, max_occ=None, kind="maximal", max_lcp=0):
    """the list debwt_fm_repeats answers"""
    rec = intervals(E, max_lcp)[0]
    keep = (rec["len"] >= min_len) & (rec["count"] >= min_occ)
    if max_occ:
        keep &= rec["count"] <= max_occ
    if kind != "intervals":
        keep &= (rec["flags"] & (IS_MAXIMAL if kind == "maximal" else IS_SUPERMAXIMAL)) != 0
    return rec[keep]


def capped_intervals(E, max_lcp):
    return intervals(E, max_lcp)[2]


def strings_of(E, rec):
    """the string of every record, from the text"""
    sym, sa = E.sym, E.sa
    return ["".join(F.ACGT[c] for c in sym[int(sa[int(x["row_lo"])]):int(sa[int(x["row_lo"])]) + int(x["len"])]) for x in rec]


def brute(E):
    """{string: (occurrences, is_maximal, is_supermaximal)} of every right-diverse repeat, from the record strings: a
    substring with two or more occurrences inside records whose right neighbours are not all the same base (a record end
    is a symbol of its own, different at every occurrence).  Maximal: the left neighbours are not all the same base
    either.  Supermaximal: maximal, and a substring of no other maximal repeat."""
    strs = F.strings(E.records)
    found = {}
    live = [(a, b) for a, s in enumerate(strs) for b in range(len(s))]
    k = 0
    while live:
        k += 1
        groups = {}
        for a, b in live:
            if b + k <= len(strs[a]):
                groups.setdefault(strs[a][b:b + k], []).append((a, b))
        live = []
        for w, occ in groups.items():
            if len(occ) < 2:
                continue
            live.extend(occ)
            right = [strs[a][b + k] if b + k < len(strs[a]) else ("end", a) for a, b in occ]
            lefts = [strs[a][b - 1] if b else ("start", a) for a, b in occ]
            if len(set(right)) > 1:
                found[w] = (len(occ), len(set(lefts)) > 1)
    maximal = [w for w, (_, m) in found.items() if m]
    out = {}
    for w, (occ, m) in found.items():
        out[w] = (occ, m, m and not any(w != x and w in x for x in maximal))
    return out
