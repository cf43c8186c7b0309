"""The helper of the FM-index geometry tests checked on the CPU (tests/fm_definition.py): the definition index against
the oracle's builder and its naive BWT, the inverse BWT of its rows, the property every geometry case is there for, and
each brute-force reference against a second formulation that shares no code with it."""
import numpy as np
import pytest

import fm_definition as F
from conftest import golden_id, golden_manifest, golden_records, outside_domain_cases

CASES = F.geometry_cases()
OUTSIDE = list(outside_domain_cases())
LONG_RECORDS = [name for name, recs in CASES.items() if min(len(r) for r in recs) > 32]
SMALL_GOLDENS = list({e["name"]: e for e in golden_manifest() if e["n"] < 8000}.values())
TWO = ("short_1to3_x500", "dup_40x20")          # the cases of the second formulations: short records, equal records


def check_against_oracle(oracle, records):
    sym, sa, L, words, hrows, drow = F.definition_index(records)
    assert np.array_equal(sym, oracle.sym_from_codes(records))
    assert np.array_equal(np.sort(sa), np.arange(len(sym)))
    assert np.array_equal(L, oracle.naive_bwt(sym))
    ow, oh, od, _ = oracle.build_bwt(sym, 32)
    assert np.array_equal(words, ow) and np.array_equal(hrows, oh) and drow == od
    return len(sym)


@pytest.mark.parametrize("name", list(CASES))
def test_prefix_doubling_gives_the_same_suffix_array(name):
    D = F.definition_of(name)
    assert np.array_equal(F.suffix_array(D.sym), D.sa)


def test_prefix_doubling_on_a_repetitive_text():
    """groups that stay together over many rounds: copies of one sequence with a few substitutions, and a homopolymer"""
    rng = np.random.default_rng(8)
    g = rng.integers(0, 4, 900).astype(np.uint8)
    recs = []
    for _ in range(4):
        c = g.copy()
        c[rng.integers(0, 900, 3)] ^= 1
        recs.append(c)
    recs.append(np.zeros(700, dtype=np.uint8))
    sym, sa = F.definition_index(recs)[:2]
    assert np.array_equal(F.suffix_array(sym), sa)


def test_the_case_list():
    assert list(CASES)[:16] == ["n2", "n32", "n33", "n64", "n383", "n384", "n385", "n768", "n1152_single", "ones_600",
                                "short_1to3_x500", "all_T_x3", "T_ones_400", "dup_40x20", "dollar_383", "dollar_384"]
    assert list(CASES)[16:] == OUTSIDE and len(OUTSIDE) == 9
    for name, recs in outside_domain_cases().items():                    # as they are
        assert len(recs) == len(CASES[name]) and all(np.array_equal(a, b) for a, b in zip(recs, CASES[name]))
    assert set(F.BUILDER_CASES) == {n for n in LONG_RECORDS if n not in OUTSIDE}
    assert max(len(F.text_symbols(r)) for r in CASES.values()) <= 1500


@pytest.mark.parametrize("name", LONG_RECORDS)
def test_definition_index_equals_the_oracle(oracle, name):
    assert name in F.BUILDER_CASES or name in OUTSIDE
    check_against_oracle(oracle, CASES[name])


@pytest.mark.parametrize("entry", SMALL_GOLDENS, ids=golden_id)
def test_definition_index_equals_the_oracle_on_goldens(oracle, entry):
    assert check_against_oracle(oracle, golden_records(entry)) == entry["n"]


@pytest.mark.parametrize("name", list(CASES))
def test_inverse_bwt_of_the_definition_rows(oracle, name):
    D = F.definition_of(name)
    rc, inv = oracle.inverse_bwt(D.words, D.n, D.hash_rows, D.dollar_row)
    assert rc == 0 and np.array_equal(inv, D.sym)
    assert np.array_equal(oracle.unpack_bwt(D.words, D.n, D.hash_rows, D.dollar_row), D.L)
    # LF by hand: walking from the row of '$' (row n - 1) spells the text backwards, and the rows met are the inverse of sa
    C = np.concatenate([[0], np.cumsum(np.bincount(D.sym, minlength=6))])
    rank = np.zeros(D.n, dtype=np.int64)
    seen = np.zeros(6, dtype=np.int64)
    for r, s in enumerate(D.L.tolist()):
        rank[r] = seen[s]
        seen[s] += 1
    r, p = D.n - 1, D.n - 1
    while p > 0:
        assert D.sa[r] == p and D.L[r] == D.sym[p - 1]
        r, p = int(C[D.L[r]] + rank[r]), p - 1
    assert r == D.dollar_row and D.sa[r] == 0


def facts(name):
    D = F.definition_of(name)
    prof = F.line_profile(D.L)
    assert len(prof) == D.n // F.ROWS + 1
    assert sum(s for s, _, _ in prof) == D.nrec
    assert [b for _, _, b in prof] == list(np.cumsum([0] + [s for s, _, _ in prof[:-1]]))
    return D, prof


def test_property_n2():
    D, prof = facts("n2")
    assert D.n == 2 and D.nrec == 1 and D.dollar_row == 0 and D.strs == ["A"] and len(prof) == 1


@pytest.mark.parametrize("name,n,nrec", [("n32", 32, 1), ("n33", 33, 1), ("n64", 64, 2)])
def test_property_word_boundaries(name, n, nrec):
    D, prof = facts(name)
    assert D.n == n and D.nrec == nrec and len(prof) == 1
    assert D.n % 32 == {"n32": 0, "n33": 1, "n64": 0}[name]
    assert len(D.words) == (n + 31) // 32


@pytest.mark.parametrize("name,n", [("n383", 383), ("n384", 384), ("n385", 385)])
def test_property_line_boundaries(name, n):
    D, prof = facts(name)
    assert D.n == n and D.nrec == 2 and D.n % F.ROWS == {383: 383, 384: 0, 385: 1}[n]
    assert len(prof) == (1 if n == 383 else 2)
    if n == 384:
        assert prof[1] == (0, 0, 2)                                     # the empty extra line occ(s, n) reads
    if n == 385:
        assert prof[1] == (0, 1, 2) and F.header_branch_lines(D.L) == [1]   # a 'T' row, no separator inside, two before


def test_property_n768():
    D, prof = facts("n768")
    assert D.n == 768 and D.n % F.ROWS == 0 and D.nrec == 3 and len(prof) == 3
    assert prof[0][0] > 0 and prof[1][0] > 0 and prof[2] == (0, 0, 3)


def test_property_n1152_single():
    D, prof = facts("n1152_single")
    assert D.n == 1152 and D.n % F.ROWS == 0 and D.nrec == 1 and len(D.hash_rows) == 0
    assert len(prof) == 4 and prof[3] == (0, 0, 1)                      # three full lines and the empty extra one
    assert sum(1 for s, _, _ in prof if s) == 1


def test_property_ones_600():
    D, prof = facts("ones_600")
    assert D.n == 1200 and D.nrec == 600 and all(len(s) == 1 for s in D.strs)
    assert sum(1 for s, _, _ in prof if s == F.ROWS) >= 1
    assert len(F.header_branch_lines(D.L)) >= 2
    assert prof[0] == (384, 0, 0) and F.header_branch_lines(D.L) == [2, 3] and prof[2][2] == 600


def test_property_short_1to3_x500():
    D, prof = facts("short_1to3_x500")
    assert D.nrec == 500 and {len(s) for s in D.strs} == {1, 2, 3}
    assert sum(1 for s, t, _ in prof if s and t) >= 3


def test_property_all_T_x3():
    D, prof = facts("all_T_x3")
    assert D.strs == ["T" * 400, "T" * 37, "T"] and D.dollar_row == 0
    assert set(np.minimum(D.L, 3).tolist()) == {3} and not (D.words ^ np.uint64(2 ** 64 - 1))[:-1].any()


def test_property_T_ones_400():
    D, prof = facts("T_ones_400")
    assert D.n == 800 and D.n % 32 == 0 and D.strs == ["T"] * 400
    assert prof[0] == (384, 0, 0)                                       # only separator rows
    assert prof[2] == (0, 32, 400) and F.header_branch_lines(D.L) == [2]   # only 'T' rows, 400 separators before
    assert sum(1 for s, _, _ in prof if s == F.ROWS) == 1


def test_property_dup_40x20():
    D, prof = facts("dup_40x20")
    assert D.nrec == 20 and len(set(D.strs)) == 1 and len(D.strs[0]) == 40
    # the suffixes that begin with '#' are ordered by what follows the separator: equal records, so by the number of
    # records that follow -- the '#' before the last record (then '$') is the largest, the first separator the smallest
    first = int(np.searchsorted(D.sym[D.sa], F.SEP))
    assert D.sa[first:first + 19].tolist() == [41 * j + 40 for j in range(19)]
    assert D.sa[-1] == D.n - 1


@pytest.mark.parametrize("name,row", [("dollar_383", 383), ("dollar_384", 384)])
def test_property_dollar_row(name, row):
    D, prof = facts(name)
    assert D.n == 753 and [len(s) for s in D.strs] == [300, 250, 200]
    assert D.dollar_row == row and D.L[row] == F.END and D.sa[row] == 0   # the last row of line 0 / the first of line 1
    assert row // F.ROWS == (0 if row == 383 else 1)


def test_packed_text_layout():
    from debwt_amd import api
    for name in F.BUILDER_CASES:
        words, sep = F.packed_text(CASES[name])
        w, n, s = api.pack_records(CASES[name])
        assert len(words) == len(w) + 1 and np.array_equal(words[:len(w)], w) and not words[len(w):].any()
        assert np.array_equal(sep, s) and n == sep[-1] + 1
    words, sep = F.packed_text(CASES["n32"])                            # n % 32 == 0: the 32 'T' fill word 1 exactly
    assert len(words) == 4 and words[1] == np.uint64(2 ** 64 - 1) and words[0] & np.uint64(3) == 3 and not words[2:].any()


# ---- the brute-force references against second formulations ------------------------------------------------------------

def occurrences(strs, w):
    """(record, offset) of every occurrence of w inside a record, overlapping ones included"""
    out = []
    for j, s in enumerate(strs):
        i = s.find(w)
        while i >= 0:
            out.append((j, i))
            i = s.find(w, i + 1)
    return out


def hamming(a, b):
    return sum(1 for x, y in zip(a, b) if x != y or x not in "ACGT")


@pytest.mark.parametrize("name", TWO + ("n385", "T_ones_400"))
def test_intervals_against_substring_counts(name):
    D = F.definition_of(name)
    starts = D.starts.astype(np.int64)
    pats = F.range_patterns(name)
    assert b"" in pats and b"N" in pats and b"ACGNT" in pats and any(p != p.upper() for p in pats)
    empty = 0
    for p in pats:
        w = p.decode().upper()
        occ = occurrences(D.strs, w) if w and set(w) <= set("ACGT") else []
        lo, hi = D.interval(p)
        assert hi - lo == len(occ), p
        assert sorted(D.locate(p).tolist()) == sorted(int(starts[j]) + i for j, i in occ)
        assert np.array_equal(D.locate(p, 3), D.sa[lo:hi][:3])
        empty += hi == lo
    assert empty > 3 and empty < len(pats)


@pytest.mark.parametrize("name", TWO)
def test_search_against_a_scan_of_the_records(name):
    D = F.definition_of(name)
    pats = [p.decode() for p in F.range_patterns(name)[::7]][:40] + ["ACNT", "NN", "TTTTTTT"]
    for p in pats:
        for K in (0, 1, 2):
            want = {}
            for strand, q in ((0, p), (1, F.revcomp(p))):
                for s in D.strs:
                    for i in range(len(s) - len(q) + 1 if q else 0):
                        d = hamming(q.upper(), s[i:i + len(q)])
                        if d <= K:
                            want[(strand, s[i:i + len(q)])] = d
            got = D.search(p, K, both=True)
            assert sorted((D.interval(w) + (d, st)) for (st, w), d in want.items()) == sorted(got), (p, K)
            assert got == sorted(got, key=lambda h: (h[3], h[2], h[0]))
            assert [h for h in got if h[3] == 0] == D.search(p, K)
            if got:
                least = min(h[2] for h in got)
                assert D.search(p, K, both=True, best=True) == [h for h in got if h[2] == least]
            if K == 0:
                lo, hi = D.interval(p)
                assert D.search(p, 0) == ([(lo, hi, 0, 0)] if hi > lo else [])


@pytest.mark.parametrize("name", TWO)
def test_mems_against_all_substrings(name):
    """a MEM is a span that occurs and whose extension by one base on either side does not: from all O(m^2) spans"""
    D = F.definition_of(name)
    reads = list(dict.fromkeys(D.strs))[:12] + ["ACGTTGCANNAC", "acgtacgt", "T", ""]
    reads += [r[:len(r) // 2] + "G" + r[len(r) // 2 + 1:] for r in reads[:6] if r]
    for p in reads:
        m = len(p)
        for min_len in (1, 5, 19):
            want = []
            for strand, q in ((0, p.upper()), (1, F.revcomp(p).upper())):
                occ = lambda a, b: a >= 0 and b <= m and any(q[a:b] in s for s in D.strs)      # noqa: E731
                for a in range(m):
                    for b in range(a + 1, m + 1):
                        if occ(a, b) and not occ(a - 1, b) and not occ(a, b + 1) and b - a >= min_len:
                            want.append((0, a, b) if strand == 0 else (1, m - b, m - a))
            assert D.mems(p, min_len, both=True) == sorted(want), (p, min_len)
            assert D.mems(p, min_len) == sorted(w for w in want if w[0] == 0)


@pytest.mark.parametrize("name", TWO)
def test_overlaps_against_each_other(name):
    """the dictionary of prefixes (overlap_ref) and the column count (overlap_mm_ref) are two formulations; at K = 0 they
    agree, and a third one by str.startswith agrees with both"""
    D = F.definition_of(name)
    queries = list(dict.fromkeys(D.strs))[:20] + [s[1:] for s in D.strs[:5] if len(s) > 1] + ["ACGTNAC", "", "acg"]
    for q in queries:
        for min_overlap in (1, 8, 40):
            exact = D.overlaps(q, min_overlap, both=True)
            assert exact == D.overlaps_mm(q, min_overlap, 0, both=True)
            third = []
            for strand, w in ((0, q.upper()), (1, F.revcomp(q).upper())):
                for L in range(len(w), min_overlap - 1, -1):
                    tail = w[len(w) - L:]
                    if L and set(tail) <= set("ACGT"):
                        third += [(j, L, strand, (1 if L == len(s) else 0) | (2 if L == len(w) else 0))
                                  for j, s in enumerate(D.strs) if s.startswith(tail)]
            assert exact == third
            two = D.overlaps_mm(q, min_overlap, 2, both=True)
            assert [h for h in two if h[3] >> 8 == 0] == exact
            assert D.overlaps(q, min_overlap, both=True, longest=True) == F.longest_of(exact)


@pytest.mark.parametrize("name", TWO)
def test_kmer_profiles_against_intervals(name):
    D = F.definition_of(name)
    reads = list(dict.fromkeys(D.strs))[:30] + ["ACGTNACGT", "acgt", ""]
    for k in (1, 2, 11, 12, 13):
        for both in (False, True):
            for p in reads:
                want = []
                for j in range(len(p) - k + 1):
                    w = p[j:j + k]
                    lo, hi = D.interval(w)
                    c = hi - lo
                    if both:
                        lo, hi = D.interval(F.revcomp(w))
                        c += hi - lo
                    want.append(c)
                assert D.kmer_profile(p, k, both) == want
