"""The reference of Definition 10 (esa_ref.py) against itself, without a GPU: the three facts the kernels rest on, on every
geometry case; the profile against a brute-force set of substrings; the stored values, the summary and the compare bound
on inputs small enough to do by hand."""
import numpy as np
import pytest

import esa_ref as ER
import fm_definition as F

CASES = F.geometry_cases()


@pytest.mark.parametrize("name", list(CASES))
def test_facts(name):
    E = ER.of_case(name)
    assert E.n == len(F.text_symbols(CASES[name])) and np.array_equal(E.sa, F.definition_of(name).sa)
    ER.facts(E)


@pytest.mark.parametrize("name", list(CASES))
def test_profile_against_substrings(name):
    E = ER.of_case(name)
    prof = E.profile(13)
    for k in (1, 2, 3, 5, 8, 13):
        assert prof[k - 1] == ER.brute_distinct(E, k)
    if name == "n2":
        assert prof == [1] + [0] * 12                                   # one base: no k-mer above k = 1


@pytest.mark.parametrize("name", list(CASES))
def test_arrays_by_hand(name):
    """sa, da, d and lcp of every case, each value from the joined string"""
    E, D = ER.of_case(name), F.definition_of(name)
    T = D.joined
    assert len(T) == E.n and E.lcp_full[0] == 0
    for r in range(E.n):
        p = int(E.sa[r])
        stop = min(T.index("#", p) if "#" in T[p:] else E.n, T.index("$", p))
        assert int(E.d[r]) == stop - p
        j = int(E.da[r])
        assert int(D.starts[j]) <= p <= int(D.starts[j]) + len(D.strs[j])
        if T[p] in "#$":
            assert E.lcp_full[r] == 0
        if r:
            a, b = T[int(E.sa[r - 1]):], T[p:]
            h = 0
            while a[h] == b[h] and a[h] in "ACGT":
                h += 1
            assert int(E.lcp_full[r]) == h


def test_known_values():
    E = ER.Esa([np.array([3, 3, 3, 3], dtype=np.uint8)])               # TTTT$
    # 'T' < '$': the longer run of T is the smaller suffix
    assert E.sa.tolist() == [0, 1, 2, 3, 4] and E.lcp_full.tolist() == [0, 3, 2, 1, 0] and E.da.tolist() == [0] * 5
    assert E.summary() == {"n": 5, "max": 3, "max_row": 1, "sum": 6, "capped": 0, "pos_prev": 0, "pos": 1, "cap": ER.U32_MAX}
    assert E.summary(2) == {"n": 5, "max": 2, "max_row": 1, "sum": 5, "capped": 2, "pos_prev": 0, "pos": 1, "cap": 2}
    assert E.profile(4) == [1, 1, 1, 1] and E.lcp(2).tolist() == [0, 2, 2, 1, 0]
    E = ER.Esa([np.array([0, 1], dtype=np.uint8)] * 2)                   # AC#AC$: the equal records stop at their separators
    assert E.sa.tolist() == [0, 3, 1, 4, 2, 5] and E.lcp_full.tolist() == [0, 2, 0, 1, 0, 0]
    assert E.da.tolist() == [0, 1, 0, 1, 0, 1] and E.d.tolist() == [2, 2, 1, 1, 0, 0]
    assert E.resolve(2) == (0, 2) and E.resolve(3) == (1, 0)
    E = ER.Esa([np.array([0], dtype=np.uint8)])                         # A$: every value is 0, the first row holds the maximum
    assert E.summary()["max_row"] == 0 and E.summary()["pos_prev"] == E.summary()["pos"] == 0


def test_compare_bound():
    E = ER.Esa([np.full(1000, 3, dtype=np.uint8)])
    n = E.n
    assert n == 1001 and E.plcp().tolist() == [0] + [1000 - i for i in range(1, 1000)] + [0]   # row 0 is position 0
    # one chunk: position 1 grows from 0 to 999, every later position starts at its own value
    assert ER.compare_bound(E, n + 1) == 999 + 64 * n
    # chunks of 100: every chunk start pays its whole value again
    assert ER.compare_bound(E, 100) == 999 + sum(1000 - i for i in range(100, 1000, 100)) + 64 * n
    assert ER.compare_bound(E, 1) == int(E.plcp().sum()) + 64 * n
    assert 64 * n < ER.compare_bound(E, 100, 40) < ER.compare_bound(E, 100)


def test_large_text_path():
    """above SMALL the suffix array comes from prefix doubling: the same arrays as by sorting"""
    recs = CASES["n1152_single"] + CASES["dup_40x20"]
    a, b = ER.Esa(recs), ER.Esa(recs, F.suffix_array(F.text_symbols(recs)))
    assert np.array_equal(a.sa, b.sa) and np.array_equal(a.lcp_full, b.lcp_full)


def test_the_traps_are_in_the_cases():
    """what the cases are here for, so that a changed collection cannot empty the tests above"""
    assert ER.of_case("homopolymer_only_one_record").summary()["max"] == 499
    assert ER.of_case("dup_40x20").summary()["max"] == 40 == ER.of_case("three_identical_40_base_records").summary()["max"]
    assert ER.of_case("all_T_x3").summary()["max"] == 399 and ER.of_case("T_ones_400").summary()["max"] == 1
    assert ER.of_case("tandem_repeat_of_two_symbols").summary()["max"] > 64
    assert ER.of_case("n2").n == 2 and {ER.of_case(f"n{n}").n for n in (383, 384, 385)} == {383, 384, 385}
