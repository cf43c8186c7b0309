"""Shared by the spectrum tests: Definition 9 of include/debwt_hip.h written out in plain Python -- a Counter over the
record strings, the canonical rule, histogram, totals, list and threshold.  Nothing here calls the library.  The two
switches of members() build the wrong references the self-check tells apart."""
import functools
from collections import Counter

import kmer_ref as KR

U32_MAX = 2 ** 32 - 1


def code_of(w):
    c = 0
    for ch in w:
        c = c * 4 + "ACGT".index(ch)
    return c


def string_of(code, k):
    return "".join("ACGT"[(code >> (2 * (k - 1 - i))) & 3] for i in range(k))


def members(strs, k, both, palindromes_twice=True, across_separators=False):
    """{code: mult} of D.  strs: the records as strings of ACGT.  The switches are for the self-check only."""
    if across_separators:                                       # wrong on purpose: k-mers of the joined text
        joined = "".join(strs)
        occ = Counter(joined[j:j + k] for j in range(len(joined) - k + 1))
    else:
        occ = Counter(s[j:j + k] for s in strs for j in range(len(s) - k + 1))
    return members_of(occ, both, palindromes_twice)


def members_of(occ, both, palindromes_twice=True):
    """{code: mult} of D from the occurrences of every k-mer inside records ({string: count})"""
    if not both:
        return {code_of(w): c for w, c in occ.items()}
    out = {}
    for w, c in occ.items():
        r = KR.revcomp(w)
        m = min(w, r)
        if m in out:
            continue
        if w == r:
            out[m] = 2 * c if palindromes_twice else c
        else:
            out[m] = c + occ.get(r, 0)
    return {code_of(w): c for w, c in out.items()}


def histogram(D, nbins):
    hist = [0] * nbins
    for m in D.values():
        hist[min(m, nbins - 1)] += 1
    return hist


def totals(D, nbins):
    """(distinct, total, overflow_total)"""
    return len(D), sum(D.values()), sum(m for m in D.values() if m >= nbins - 1)


def listing(D, min_mult=1, max_mult=U32_MAX):
    """[(code, mult)] ascending by code, mult clamped to u32 before the filter"""
    return [(c, min(m, U32_MAX)) for c, m in sorted(D.items()) if min_mult <= min(m, U32_MAX) <= max_mult]


def threshold(hist, total):
    """(valley, peak, est_size); (0, 0, 0) without a valley"""
    nbins = len(hist)
    valley = next((c for c in range(1, nbins - 2) if hist[c + 1] > hist[c]), 0)
    if not valley:
        return 0, 0, 0
    peak = max(range(valley + 1, nbins - 1), key=lambda c: (hist[c], -c))
    return valley, peak, (total - sum(c * hist[c] for c in range(valley))) // peak


def forward_total(strs, k):
    return sum(max(0, len(s) - k + 1) for s in strs)


def palindrome_occ(strs, k):
    """the sum of occ over the k-mers that equal their own reverse complement"""
    return sum(1 for s in strs for j in range(len(s) - k + 1) if s[j:j + k] == KR.revcomp(s[j:j + k]))


@functools.lru_cache(maxsize=None)
def of_read_set(k, both):
    return members(KR.read_set()["records"], k, both)
