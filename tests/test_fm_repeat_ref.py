"""The reference of Definition 11 (repeat_ref.py) without a GPU: against a brute force over the record strings on every
geometry case of at most 700 rows, against the invariants of the definition on every case and on the seeded read set, and
on arrays small enough to do by hand."""
import numpy as np
import pytest

import esa_ref as ER
import fm_definition as F
import repeat_ref as RR

CASES = F.geometry_cases()
SMALL = [name for name in CASES if ER.of_case(name).n <= 700]


def test_the_small_cases_hold_the_traps():
    assert len(SMALL) >= 16 and sum(len(RR.intervals(ER.of_case(name))[0]) for name in SMALL) >= 2780
    for name in ("n2", "all_T_x3", "three_identical_40_base_records", "tandem_repeat_of_two_symbols", "one_symbol_per_record"):
        assert name in SMALL, name


def test_the_cases_hold_the_edges():
    """what the cases are here for: rows 0 and n - 1 as interval ends, wide flat intervals behind separators alone"""
    ends = {name: RR.intervals(ER.of_case(name))[0] for name in ("one_symbol_per_record", "all_T_x3", "dup_40x20",
                                                                 "three_identical_40_base_records")}
    for name in ("one_symbol_per_record", "all_T_x3"):
        rec, n = ends[name], ER.of_case(name).n
        assert (rec["row_lo"] == 0).any() or (rec["row_lo"] + rec["count"] == n).any(), name
    for name in ("dup_40x20", "three_identical_40_base_records"):
        rec = ends[name]
        wide = rec[(rec["len"] == 40) & (rec["flags"] & RR.IS_SUPERMAXIMAL != 0)]
        assert len(wide) == 1 and wide[0]["left"][4] == wide[0]["count"] >= 3, name
    assert len(RR.intervals(ER.of_case("n2"))[0]) == 0


@pytest.mark.parametrize("name", SMALL)
def test_against_the_strings(name):
    """the same intervals, the same maximal and supermaximal sets and the same occurrence counts as the brute force"""
    E = ER.of_case(name)
    rec = RR.intervals(E)[0]
    got = {}
    for w, x in zip(RR.strings_of(E, rec), rec):
        assert w not in got                                             # one interval per string
        got[w] = (int(x["count"]), bool(x["flags"] & RR.IS_MAXIMAL), bool(x["flags"] & RR.IS_SUPERMAXIMAL))
    assert got == RR.brute(E)


def invariants(E, caps=(1, 7, 40)):
    rec, rep, capped = RR.intervals(E)
    assert capped == 0
    n, lcp = E.n, E.lcp_full
    i, j, l = rec["row_lo"].astype(np.int64), (rec["row_lo"] + rec["count"] - 1).astype(np.int64), rec["len"].astype(np.int64)
    assert (l >= 1).all() and (i < j).all() and (j < n).all()
    assert (lcp[i] < l).all() and (lcp[np.minimum(j + 1, n - 1)] * (j + 1 < n) < l).all()
    assert (lcp[rep] == l).all() and (i < rep).all() and (rep <= j).all()
    assert (np.diff(rep) > 0).all()                                     # distinct and ascending
    for x, r in list(zip(rec, rep))[:: max(1, len(rec) // 300)]:       # the inner rows of a sample, one by one
        a, b = int(x["row_lo"]), int(x["row_lo"] + x["count"] - 1)
        inner = lcp[a + 1:b + 1]
        assert inner.min() == x["len"] and a + 1 + int(np.argmax(inner == x["len"])) == r
        assert bool(x["flags"] & RR.IS_SUPERMAXIMAL) == bool((inner == x["len"]).all() and x["left"][:4].max() <= 1)
    assert (rec["left"].sum(axis=1) == rec["count"]).all()
    mx, sp = (rec["flags"] & RR.IS_MAXIMAL) != 0, (rec["flags"] & RR.IS_SUPERMAXIMAL) != 0
    assert not (sp & ~mx).any()                                         # supermaximal within maximal within intervals
    assert np.array_equal(mx, rec["left"][:, :4].max(axis=1) < rec["count"])
    a, b, c = (RR.repeats(E, kind=k) for k in RR.KINDS)
    assert np.array_equal(a, rec[mx]) and np.array_equal(b, rec[sp]) and np.array_equal(c, rec)
    for cap in caps:
        crec, crep, ccapped = RR.intervals(E, cap)
        below = rec["len"] < cap
        assert np.array_equal(crec, rec[below]) and np.array_equal(crep, rep[below])
        st = E.lcp(cap)
        # the cap is the largest stored value: an interval of that value is a run of it, begun behind a smaller value
        assert ccapped == int(np.count_nonzero((st[1:] == cap) & (st[:-1] < cap)))


@pytest.mark.parametrize("name", list(CASES))
def test_invariants(name):
    invariants(ER.of_case(name))


def test_invariants_of_the_read_set():
    E = ER.of_read_set()
    invariants(E)
    rec = RR.intervals(E)[0]
    assert len(rec) > 1000 and int(RR.repeats(E)["len"].max()) == E.summary()["max"]


def test_known_values():
    E = ER.Esa([np.array([3, 3, 3, 3], dtype=np.uint8)])               # TTTT$: lcp 0 3 2 1 0, L = $ T T T T
    rec, rep, _ = RR.intervals(E)
    assert rep.tolist() == [1, 2, 3] and rec["len"].tolist() == [3, 2, 1] and rec["row_lo"].tolist() == [0, 0, 0]
    assert rec["count"].tolist() == [2, 3, 4] and rec["left"].tolist() == [[0, 0, 0, 1, 1], [0, 0, 0, 2, 1], [0, 0, 0, 3, 1]]
    assert rec["flags"].tolist() == [3, 1, 1]                           # TTT is supermaximal, TT and T are maximal
    assert RR.capped_intervals(E, 2) == 1 and RR.intervals(E, 2)[0]["len"].tolist() == [1]
    E = ER.Esa([np.array([0, 1], dtype=np.uint8)] * 2)                   # AC#AC$: lcp 0 2 0 1 0 0
    rec, rep, _ = RR.intervals(E)
    assert rep.tolist() == [1, 3] and rec["len"].tolist() == [2, 1] and rec["left"].tolist() == [[0, 0, 0, 0, 2], [2, 0, 0, 0, 0]]
    assert rec["flags"].tolist() == [3, 0]                              # AC starts both records; C follows A twice
    assert len(RR.repeats(E, kind="intervals")) == 2 and len(RR.repeats(E)) == 1
    assert len(RR.intervals(ER.Esa([np.array([0], dtype=np.uint8)]))[0]) == 0              # A$: no interval


def test_a_flat_tail_under_a_taller_head_is_not_flat():
    """lcp 0 2 1 0: the interval of value 1 begins under a row of value 2 -- nothing above 1 stands to the right of its
    representative, and still it is not flat"""
    E = ER.Esa([np.array([0, 0, 0], dtype=np.uint8)])                   # AAA$
    assert E.lcp_full.tolist() == [0, 2, 1, 0]
    rec = RR.intervals(E)[0]
    assert rec["len"].tolist() == [2, 1] and rec["flags"].tolist() == [3, 1]


def test_filters():
    E = ER.of_case("dup_40x20")
    rec = RR.intervals(E)[0]
    assert len(RR.repeats(E, min_len=40, kind="intervals")) == 1 and RR.repeats(E, min_len=40)[0]["count"] == 20
    for lo, hi in ((2, None), (5, None), (2, 2), (3, 10), (21, None)):
        got = RR.repeats(E, min_occ=lo, max_occ=hi, kind="intervals")
        want = rec[(rec["count"] >= lo) & (rec["count"] <= (hi or E.n))]
        assert np.array_equal(got, want)
