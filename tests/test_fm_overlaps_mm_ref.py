"""The reference of overlaps with mismatches (overlap_mm_ref.brute) checked on its own, without a GPU: at K = 0 it is the
exact reference of overlap_ref.py, and at K = 2 the query set holds every kind of hit the GPU comparison is meant to
cover; the rate rule removes and keeps what it should."""
import pytest

from overlap_mm_ref import brute, mutated_reads, queries
from overlap_ref import CONTAINS, WHOLE, Ref


@pytest.fixture(scope="module")
def data():
    strs, orig = mutated_reads()
    return strs, orig, queries(strs, orig, 20)


def test_recipe_sizes(data):
    strs, orig, pats = data
    assert len(strs) == len(orig) == 436 and len(pats) == 165
    assert min(len(s) for s in strs) >= 40
    diff = [sum(a != b for a, b in zip(s, o)) for s, o in zip(strs, orig)]
    assert all(len(s) == len(o) for s, o in zip(strs, orig))
    for i, d in enumerate(diff):
        want = 2 if i % 23 == 0 else 1 if i % 19 == 0 or i % 17 == 0 else i % 3
        assert d == want, i
    assert strs[17][0] != orig[17][0] and strs[19][-1] != orig[19][-1] and strs[23][30] != orig[23][30] and strs[23][31] != orig[23][31]


def test_zero_mismatches_is_the_exact_reference(data):
    strs, _, pats = data
    R = Ref(strs, 20)
    total = 0
    for p in pats:
        want = R.hits(p)
        assert brute(strs, p, 20, 0) == want, p              # the mm field is 0
        total += len(want)
    assert total > len(pats)


def test_reference_has_every_kind_of_hit(data):
    """at min_overlap 20, K = 2 the reference alone holds each category the GPU comparison is meant to cover"""
    strs, _, pats = data
    K, last = 2, len(strs) - 1
    kinds = set()
    for p in pats:
        hits = brute(strs, p, 20, K)
        m = len(p)
        by_len, by_rec = {}, {}
        for j, L, _, fl in hits:
            mm = fl >> 8
            cols = [c for c in range(L) if p[m - L + c].upper() != strs[j][c]]
            assert len(cols) == mm <= K and L <= len(strs[j])
            by_len.setdefault(L, set()).add(mm)
            by_rec.setdefault(j, set()).add(mm)
            for kind, holds in (("mm = K", mm == K), ("first column", 0 in cols), ("query's last base", L - 1 in cols),
                                ("adjacent", any(c + 1 in cols for c in cols)), ("contains, mm > 0", fl & CONTAINS and mm),
                                ("whole, mm > 0", fl & WHOLE and mm),
                                ("query N", any(p[m - L + c] == "N" for c in cols)),
                                ("record 0", j == 0), ("last record", j == last)):
                if holds:
                    kinds.add(kind)
        if any(len(v) > 1 for v in by_len.values()):
            kinds.add("one length, records of different mm")
        if any(len(v) > 1 for v in by_rec.values()):
            kinds.add("one record at lengths of different mm")
    assert kinds == {"mm = K", "first column", "query's last base", "adjacent", "contains, mm > 0", "whole, mm > 0", "query N",
                     "record 0", "last record", "one length, records of different mm", "one record at lengths of different mm"}


def test_hit_counts_grow_with_the_budget(data):
    strs, _, pats = data
    n = [sum(len(brute(strs, p, 20, K)) for p in pats) for K in (0, 1, 2, 3)]
    assert n[0] < n[1] < n[2] < n[3]
    print("hits at K = 0..3:", n)


def test_rate_rule(data):
    """permille 25 with K = 4: a hit needs 40 columns per mismatch, so some hits K alone admits go and some with mm > 0 stay"""
    strs, _, pats = data
    removed = kept = 0
    for p in pats:
        free = brute(strs, p, 20, 4)
        rated = brute(strs, p, 20, 4, permille=25)
        assert rated == [h for h in free if 1000 * (h[3] >> 8) <= 25 * h[1]]
        removed += len(free) - len(rated)
        kept += sum(1 for h in rated if h[3] >> 8)
    assert removed >= 1 and kept >= 1
